#!/usr/bin/env python3
"""Train the reference's recurrent policy with PPO, IMPALA or behaviour cloning on the multi-agent grid environment (HIP engine), everything on the
device.

Counterpart of the reference's training mode (main.py with ``ALGO_NAME = "PPO"``; the settings are those of
src/agents/ppo.py): every iteration collects one fragment of ``--T`` steps from ``--num-envs`` envs with the fused policy
launch, computes GAE, runs the PPO epochs and pushes the new weights to the policy kernel.  With ``--algo IMPALA`` (main.py
with ``ALGO_NAME = "IMPALA"``, the settings of src/agents/impala.py) there is no GAE step: one pass over the fragment with
V-trace targets recomputed from the current network in every minibatch, and the weights are pushed every ``--push-every``
iterations, so the collecting policy may lag the learner.  One JSON line per iteration; at
the end (and every ``--save-every`` iterations) a checkpoint that ``scripts/evaluate_multi_agent_env.py --policy NEURAL
--checkpoint`` accepts.  The env is either a named workload of ``dl_reference_models_amd.workloads`` (``--workload``) or
given by the shape options of the evaluation script.

    python scripts/train_multi_agent_env.py --workload ref_training_4096x32x32_n16 --iters 200 --checkpoint policy.pt
    python scripts/train_multi_agent_env.py --env-name ReferenceModel-2-1 --num-agents 4 --num-envs 1024 --iters 50 --checkpoint p.pt
    python scripts/train_multi_agent_env.py --algo IMPALA --push-every 2 --workload ref_training_4096x32x32_n16 --checkpoint policy.pt
    python scripts/train_multi_agent_env.py --algo DQN --workload ref_training_4096x32x32_n16 --checkpoint qnet.pt
    python scripts/train_multi_agent_env.py --execution-mode DTE --workload ref_training_4096x32x32_n16 --checkpoint dte.pt
    python scripts/train_multi_agent_env.py --algo BC --expert windowed --beta-start 1 --beta-end 0 --beta-iters 50 --checkpoint bc.pt
    python scripts/train_multi_agent_env.py --algo PPO --init-checkpoint bc.pt --checkpoint policy.pt

With ``--algo DQN`` (main.py with ``ALGO_NAME = "DQN"``, the settings of src/agents/dqn.py) the net is the dueling 32-32
``dqn.QNetwork``, exploration is epsilon-greedy, every fragment goes into a prioritised replay ring on the device and the
checkpoint is of kind ``q_network``.

With ``--algo BC`` (no counterpart in the reference, which only names the expert's actions "an imitation target") every
step of the fragment is labelled with the action of a device planner (``--expert``), the learner minimises the cross-entropy
of the policy against those labels, and a share ``beta`` of the steps executes the expert's action instead of the policy's
(DAgger mixing), falling linearly from ``--beta-start`` to ``--beta-end`` over ``--beta-iters`` iterations.  The checkpoint is
an ordinary policy checkpoint: ``--policy NEURAL`` evaluates it and ``--init-checkpoint`` starts PPO, IMPALA or BC from it
(``--bc-vf-coeff`` above 0 also regresses the value head to GAE's targets, which PPO then starts from).

``--execution-mode DTE`` (main.py's ``training_execution_mode = "DTE"``, src/agents/ppo.py:77-88) trains one policy per agent,
each on its own agent's experience: a ``PerAgentPolicy``, PPO only, and a checkpoint of kind ``per_agent``.  The default,
CTDE, is one policy shared by all agents.

``--guidance`` (no counterpart in the reference) puts the shortest-path guidance into the observation the policy sees:
six floats per agent from one more launch per step (``mapf_observe_guided``: which moves shorten the agent's path to its
goal, whether it stands on it, and the path length).  PPO, IMPALA and BC, CTDE and DTE; the evaluation script needs
``--guidance`` too, since a checkpoint does not record it.

    python scripts/train_multi_agent_env.py --algo BC --expert independent --guidance --checkpoint bc_guided.pt

``--population P`` (main.py:409 hands its config to src/trainers/tuner.py, which trains a population of trials under a
population-based scheduler) trains P shared policies side by side on the one env handle, env b with member b % P, each with
its own lr, entropy coefficient, clip, gamma and lambda; every ``--perturb-every`` iterations the worst quarter clone a
member of the best quarter and perturb its settings inside tuner.py:19-26's ranges (``population.PBT``, seeded by
``--pbt-seed``).  PPO and CTDE only.  ``--epochs`` is one value for the whole population and is not searched: the members
share one minibatch loop, and a member cannot skip an Adam step inside it without its moments still moving.
``--checkpoint`` receives the best member's ordinary checkpoint, ``--population-checkpoint`` the whole population.

    python scripts/train_multi_agent_env.py --population 8 --perturb-every 10 --workload ref_training_4096x32x32_n16 --checkpoint best.pt
"""

from __future__ import annotations

import argparse
import json
import sys
import time
from pathlib import Path

PROJECT_ROOT = Path(__file__).resolve().parents[1]
if str(PROJECT_ROOT) not in sys.path:
    sys.path.insert(0, str(PROJECT_ROOT))

def beta_schedule(args) -> list:
    """The (iteration, beta) points of --beta-start / --beta-end / --beta-iters."""
    if args.beta_iters > 0:
        return [(0, args.beta_start), (args.beta_iters, args.beta_end)]
    return [(0, args.beta_start)]


def load_initial(cls, path, env, has_mask: bool, device, obs_len: int | None = None):
    """The module of --init-checkpoint, refused where it is not what the env and the run need (obs_len: what the policy sees,
    default the env's observation; with --guidance six floats more)."""
    module = cls.load(path)
    obs_len = env.obs_len if obs_len is None else obs_len
    if module.obs_len != obs_len or bool(module.has_mask) != bool(has_mask) or getattr(module, "num_agents", env.num_agents) != env.num_agents:
        raise SystemExit(f"--init-checkpoint {path} was trained on another env: its config is {module.config()}, this env has "
                         f"{obs_len} floats per observation, {env.num_agents} agents and has_mask = {has_mask}")
    return module.to(device)


def kl_settings(args) -> dict:
    """The PPOLearner arguments of --kl-coeff / --kl-target / --fused-objective."""
    on = args.kl_coeff is not None or args.kl_target is not None
    return {"kl_coeff": (0.2 if args.kl_coeff is None else args.kl_coeff) if on else None,
            "kl_target": 0.01 if args.kl_target is None else args.kl_target, "fused_objective": args.fused_objective}


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--workload", default=None, help="a multi-agent workload of dl_reference_models_amd.workloads (overrides the shape options)")
    p.add_argument("--env-name", default="ReferenceModel-2-1")
    p.add_argument("--num-agents", type=int, default=4)
    p.add_argument("--sensor-range", type=int, default=2)
    p.add_argument("--steps-per-episode", type=int, default=100)
    p.add_argument("--lifelong", action="store_true", help="lifelong_mapf")
    p.add_argument("--deterministic", action="store_true")
    p.add_argument("--num-envs", type=int, default=None, help="default: the workload's, or 1024")
    p.add_argument("--seed", type=int, default=42, help="env b is seeded with seed + b (a workload's grids are those of env indices 0 .. B - 1 whatever the seed); "
                                                          "weights, minibatches and sampling draw from it too")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--T", type=int, default=32, help="steps per fragment")
    p.add_argument("--algo", choices=("PPO", "IMPALA", "DQN", "BC"), default="PPO")
    p.add_argument("--execution-mode", choices=("CTDE", "DTE"), default="CTDE", help="CTDE: one shared policy; DTE: one policy per agent (PPO only)")
    dqn = p.add_argument_group("DQN only (main.py with ALGO_NAME = \"DQN\", the settings of src/agents/dqn.py; --lr is not read, --dqn-lr is)")
    dqn.add_argument("--dqn-lr", type=float, default=3e-4)
    dqn.add_argument("--train-batch", type=int, default=4000, help="transitions per update")
    dqn.add_argument("--capacity", type=int, default=50_000, help="replay transitions (raised to one fragment where that is more)")
    dqn.add_argument("--updates", type=int, default=4, help="learner updates per iteration")
    dqn.add_argument("--target-update-every", type=int, default=100, help="updates between hard copies to the target net")
    dqn.add_argument("--learning-starts", type=int, default=1000, help="stored transitions before the first update")
    dqn.add_argument("--epsilon-steps", type=int, default=1250, help="vector steps over which epsilon falls from 1.0 to --epsilon-final")
    dqn.add_argument("--epsilon-final", type=float, default=0.05)
    dqn.add_argument("--no-double-q", action="store_true")
    bc = p.add_argument_group("BC only (behaviour cloning of a device planner; --execution-mode DTE clones one policy per agent)")
    bc.add_argument("--expert", choices=("yielding", "independent", "windowed"), default="yielding", help="the planner that labels every step")
    bc.add_argument("--expert-window", type=int, default=8, help="the window of --expert windowed")
    bc.add_argument("--beta-start", type=float, default=0.0, help="the share of steps that execute the expert's action, at iteration 0")
    bc.add_argument("--beta-end", type=float, default=0.0, help="... and from iteration --beta-iters on")
    bc.add_argument("--beta-iters", type=int, default=0, help="iterations over which beta goes from --beta-start to --beta-end")
    bc.add_argument("--bc-vf-coeff", type=float, default=0.0, help="above 0: also regress the value head to GAE's targets")
    bc.add_argument("--bc-ent-coeff", type=float, default=0.0)
    p.add_argument("--guidance", action="store_true", help="PPO / IMPALA / BC: the policy sees the shortest-path guidance, six floats more per "
                   "observation (which moves shorten the agent's path, whether it stands on its goal, the path length); evaluate the "
                   "checkpoint with --guidance too, it does not record the option")
    p.add_argument("--init-checkpoint", type=Path, default=None, help="PPO / IMPALA / BC: start from this saved module (of the kind "
                   "the run trains: a shared policy, or with --execution-mode DTE a per-agent one)")
    p.add_argument("--push-every", type=int, default=1, help="push the weights to the policy kernel every K iterations")
    p.add_argument("--epochs", type=int, default=None, help="default: 12 (PPO), 1 (IMPALA, BC)")
    p.add_argument("--minibatches", type=int, default=8)
    p.add_argument("--lr", type=float, default=1e-3)
    p.add_argument("--feed-forward", action="store_true", help="no LSTM")
    p.add_argument("--torch-learner", action="store_true", help="the recurrence (and the IMPALA objective) in torch ops instead of the fused kernels")
    p.add_argument("--kl-coeff", type=float, default=None, help="PPO only: RLlib's adaptive KL penalty, starting at this coefficient (the "
                   "reference trains with 0.2); with neither this nor --kl-target there is no KL term")
    p.add_argument("--kl-target", type=float, default=None, help="PPO only: the KL the coefficient is adapted towards (default 0.01; given "
                   "alone it switches the term on at a coefficient of 0.2)")
    p.add_argument("--fused-objective", action=argparse.BooleanOptionalAction, default=None,
                   help="PPO only: the objective in one launch of mapf_ppo_loss instead of torch ops (default: the learner's)")
    p.add_argument("--fused-trunk", action="store_true", help="PPO / IMPALA / BC with one shared policy: fc1, fc2 and the input half of the "
                   "gates of a minibatch in one launch forward and one backward (mapf_trunk_*) instead of torch ops")
    p.add_argument("--fused-grads", action="store_true", help="PPO / IMPALA / BC / --population: the parameter gradients that are sums "
                   "over a minibatch's rows (dW_hh always, the trunk's with --fused-trunk) as one split-row reduction each "
                   "(mapf_lstm_seq_param_grad, mapf_trunk_param_grad) instead of GEMMs and column sums")
    pop = p.add_argument_group("population-based training (--algo PPO --execution-mode CTDE only)")
    pop.add_argument("--population", type=int, default=None, help="train P policies side by side on the one env (num-envs must be a "
                     "multiple of P); --epochs is one value for all members and is not searched")
    pop.add_argument("--perturb-every", type=int, default=10, help="iterations between two perturbations")
    pop.add_argument("--pbt-seed", type=int, default=0, help="seed of the perturbation decisions")
    pop.add_argument("--population-checkpoint", type=Path, default=None, help="where the whole population is written (PopulationTrainer.save)")
    p.add_argument("--checkpoint", type=Path, default=None, help="where the trained policy is written (with --population: the best member's)")
    p.add_argument("--save-every", type=int, default=0)
    p.add_argument("--log", type=Path, default=None, help="also append the per-iteration lines to this file")
    return p.parse_args(argv)


def make_env(args):
    from dl_reference_models_amd import workloads as wl
    from dl_reference_models_amd.vec_env import VecReferenceModel

    if args.workload:
        if args.workload not in wl.WORKLOADS or wl.is_single_agent(args.workload):
            raise SystemExit(f"--workload must be one of {[k for k in wl.WORKLOADS if not wl.is_single_agent(k)]}")
        b = args.num_envs or wl.WORKLOADS[args.workload][0]
        cfg = wl.workload_config(args.workload, list(range(b)))
        cfg["seeds"] = [args.seed + i for i in range(b)]
        cfg["device"] = args.device
        return VecReferenceModel(cfg), bool(cfg.get("include_action_mask_in_obs", False))
    cfg = {"env_name": args.env_name, "seed": args.seed, "deterministic": args.deterministic, "num_agents": args.num_agents,
           "steps_per_episode": args.steps_per_episode, "sensor_range": args.sensor_range, "lifelong_mapf": args.lifelong,
           "training_execution_mode": "CTDE", "render_env": False, "num_envs": args.num_envs or 1024, "device": args.device}
    # (as in the evaluation script: no action mask in the observation, so its --policy NEURAL takes the checkpoint)
    return VecReferenceModel(cfg), False


def main(argv=None) -> dict:
    args = parse_args(argv)
    if args.execution_mode == "DTE" and args.algo not in ("PPO", "BC"):
        raise SystemExit(f"--execution-mode DTE trains with --algo PPO or BC only ({args.algo} has no per-agent learner)")
    if args.init_checkpoint is not None and args.algo == "DQN":
        raise SystemExit("--init-checkpoint starts PPO, IMPALA or BC from a policy checkpoint; DQN trains a Q-network")
    for name, given in (("--population", args.population is not None), ("--population-checkpoint", args.population_checkpoint is not None)):
        if given and (args.algo != "PPO" or args.execution_mode != "CTDE" or args.population is None):
            raise SystemExit(f"{name} trains a population with --algo PPO --execution-mode CTDE only (and needs --population P)")
    if args.population is not None and (args.population < 1 or args.init_checkpoint is not None or args.push_every != 1):
        raise SystemExit("--population needs P >= 1 and takes neither --init-checkpoint nor --push-every")
    if args.guidance and (args.algo == "DQN" or args.population is not None):
        raise SystemExit("--guidance is offered with --algo PPO, IMPALA or BC only: " + ("--algo DQN's rollout" if args.algo == "DQN" else
                         "--population's trainer") + " collects the plain observation")
    if args.fused_trunk and (args.algo == "DQN" or args.population is not None):
        raise SystemExit("--fused-trunk is offered with --algo PPO, IMPALA or BC on one shared policy only: " +
                         ("DQN trains a Q-network" if args.algo == "DQN" else "the trunk kernels do not cover a PopulationPolicy"))
    if args.fused_grads and args.algo == "DQN":
        raise SystemExit("--fused-grads is offered with --algo PPO, IMPALA or BC only: DQN trains a Q-network")
    import torch

    from dl_reference_models_amd.learner import BCLearner, IMPALALearner, PPOLearner, Trainer
    from dl_reference_models_amd.policy import MaskedRecurrentPolicy, PerAgentPolicy

    env, has_mask = make_env(args)
    torch.manual_seed(args.seed)
    if args.algo == "DQN":
        return train_dqn(args, env)
    if args.population is not None:
        return train_population(args, env, has_mask)
    cls = PerAgentPolicy if args.execution_mode == "DTE" else MaskedRecurrentPolicy
    obs_len = env.guided_obs_len if args.guidance else env.obs_len  # what the policy sees
    if args.init_checkpoint is not None:
        module = load_initial(cls, args.init_checkpoint, env, has_mask, env.device, obs_len)
    elif args.execution_mode == "DTE":
        module = PerAgentPolicy(env.num_agents, obs_len, has_mask=has_mask, recurrent=not args.feed_forward).to(env.device)
    else:
        module = MaskedRecurrentPolicy(obs_len, has_mask=has_mask, recurrent=not args.feed_forward).to(env.device)
    if args.algo == "BC":
        learner = BCLearner(module, lr=args.lr, epochs=args.epochs or 1, minibatches=args.minibatches, seed=args.seed,
                            fused=not args.torch_learner, fused_objective=False if args.torch_learner else args.fused_objective,
                            vf_coeff=args.bc_vf_coeff, ent_coeff=args.bc_ent_coeff, expert=args.expert, expert_window=args.expert_window,
                            beta_schedule=beta_schedule(args), fused_trunk=args.fused_trunk)
    elif args.algo == "IMPALA":
        learner = IMPALALearner(module, lr=args.lr, epochs=args.epochs or 1, minibatches=args.minibatches, seed=args.seed,
                                fused=not args.torch_learner, fused_trunk=args.fused_trunk)
    else:
        learner = PPOLearner(module, lr=args.lr, epochs=args.epochs or 12, minibatches=args.minibatches, seed=args.seed,
                             fused=not args.torch_learner, fused_trunk=args.fused_trunk, **kl_settings(args))
    trainer = Trainer(env, module, T=args.T, learner=learner, sample_seed=args.seed, push_every=args.push_every,
                      guidance=args.guidance, fused_grads=args.fused_grads)
    return run(args, env, module, trainer)


def train_dqn(args, env) -> dict:
    from dl_reference_models_amd.dqn import DQNLearner, DQNTrainer, QNetwork

    module = QNetwork(env.obs_len).to(env.device)
    learner = DQNLearner(module, lr=args.dqn_lr, train_batch=args.train_batch,
                         double_q=not args.no_double_q, target_update_every=args.target_update_every, seed=args.seed,
                         fused=not args.torch_learner)
    trainer = DQNTrainer(env, module, T=args.T, learner=learner, capacity=args.capacity,
                         epsilon=((0, 1.0), (args.epsilon_steps, args.epsilon_final)), learning_starts=args.learning_starts,
                         updates=args.updates, seed=args.seed)
    return run(args, env, module, trainer)


def train_population(args, env, has_mask: bool) -> dict:
    from dl_reference_models_amd.policy import PopulationPolicy
    from dl_reference_models_amd.population import PBT, Hyper, PopulationTrainer

    if env.num_envs % args.population:
        raise SystemExit(f"--population {args.population} does not divide the {env.num_envs} envs")
    module = PopulationPolicy(args.population, env.num_agents, env.obs_len, has_mask=has_mask, recurrent=not args.feed_forward).to(env.device)
    kl = kl_settings(args)
    if kl["fused_objective"] is False or args.torch_learner:
        raise SystemExit("--population runs on the fused kernels only: it takes neither --no-fused-objective nor --torch-learner")
    trainer = PopulationTrainer(env, module, T=args.T, hyper=Hyper(lr=args.lr), pbt=PBT(args.perturb_every, args.pbt_seed),
                                epochs=args.epochs or 12, minibatches=args.minibatches, kl_coeff=kl["kl_coeff"],
                                kl_target=kl["kl_target"], seed=args.seed, sample_seed=args.seed, fused_grads=args.fused_grads)
    return run(args, env, module, trainer)


def run(args, env, module, trainer) -> dict:
    population = getattr(args, "population", None) is not None
    # --checkpoint of a population: the best member, an ordinary policy checkpoint
    save = (lambda path: trainer.best().save(path)) if population else module.save
    if args.checkpoint:
        args.checkpoint.parent.mkdir(parents=True, exist_ok=True)
    log = args.log.open("a", encoding="utf-8") if args.log else None
    history = []
    rows = env.num_envs * env.num_agents
    for it in range(args.iters):
        t0 = time.perf_counter()
        stats = trainer.iterate()
        stats["seconds"] = time.perf_counter() - t0
        stats["agent_steps_per_s"] = rows * args.T / stats["seconds"]
        stats["terminated_share"] = stats["terminated"] / stats["episodes"] if stats["episodes"] else None  # the success rate
        line = json.dumps(stats)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
        history.append(stats)
        if args.checkpoint and args.save_every and (it + 1) % args.save_every == 0:
            save(args.checkpoint)
    env.poll_error()
    if population and args.population_checkpoint:
        args.population_checkpoint.parent.mkdir(parents=True, exist_ok=True)
        trainer.save(args.population_checkpoint)
        print(f"Population saved to {args.population_checkpoint}")
    if args.checkpoint:
        save(args.checkpoint)
        print(f"Checkpoint saved to {args.checkpoint}")
    if log:
        log.close()
    env.close()
    return {"history": history, "checkpoint": args.checkpoint, "config": module.config()}


if __name__ == "__main__":
    main()
