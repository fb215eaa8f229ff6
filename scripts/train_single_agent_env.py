#!/usr/bin/env python3
"""Train the reference's joint-action policy with PPO, IMPALA or behaviour cloning on the single-agent grid environment (HIP engine), everything
on the device.

Counterpart of ``scripts/train_multi_agent_env.py`` for the reference's ``training_execution_mode = "CTE"``: one policy moves
all N agents of an env, the observation is the full grid, the action is ``MultiDiscrete([5] * N)``.  Every iteration
collects one fragment of ``--T`` steps from ``--num-envs`` envs with the joint policy launch (``JointRollout``), computes
GAE, runs the PPO epochs and pushes the new weights to the policy kernel.  The defaults are the reference's CTE PPO
settings (src/agents/ppo.py:25-64): lr 1e-4, clip 0.2, entropy 0.01, 10 epochs, 8 minibatches; vf_coeff 1.0 is RLlib's
default (the reference sets none); gamma 0.99, lambda 0.95.  One JSON line per iteration; at the end (and every
``--save-every`` iterations) a checkpoint that ``JointActionPolicy.load`` reads and that
``scripts/evaluate_single_agent_env.py --policy NEURAL --checkpoint`` scores.  The env is a single-agent workload of
``dl_reference_models_amd.workloads`` (``--workload``, default ``cte_8192x16x16_n4``) or given by ``--env-name``.

``--algo IMPALA`` is the reference's CTE IMPALA configuration (src/agents/impala.py:16-51): the feed-forward 256-256 net
(``--hidden 256``, which the policy kernel runs feed-forward only), lr 1e-3, gamma 0.99, vf_coeff 0.3, entropy 0.001, one
pass per fragment with V-trace targets from the current network (no GAE step), and the weights pushed to the policy kernel
every ``--push-every`` iterations.  Every option given on the command line overrides these; without ``--algo`` nothing
changes.  ``--hidden 64`` with either algorithm is the recurrent 64-64 net (feed-forward with ``--feed-forward``).

    python scripts/train_single_agent_env.py --iters 300 --checkpoint joint.pt
    python scripts/train_single_agent_env.py --algo IMPALA --iters 300 --checkpoint joint_impala.pt
    python scripts/train_single_agent_env.py --env-name ReferenceModel-2-1 --num-agents 4 --num-envs 1024 --iters 50 --checkpoint p.pt
    python scripts/train_single_agent_env.py --algo BC --expert yielding --beta-start 1 --beta-end 0 --beta-iters 50 --checkpoint bc.pt
    python scripts/train_single_agent_env.py --init-checkpoint bc.pt --iters 300 --checkpoint joint.pt

``--algo BC`` clones a device planner (``--expert yielding`` or ``independent``; the windowed planner is offered on the
multi-agent env only): every step is labelled with the expert's actions, the learner minimises the cross-entropy of the N
heads against them, and a share ``beta`` of the steps executes the expert's actions (``--beta-start`` to ``--beta-end`` over
``--beta-iters`` iterations).  Its defaults: the recurrent 64-64 net, lr 1e-3, one epoch, no entropy bonus, and no value
regression unless ``--vf-coeff`` is above 0.  ``--init-checkpoint`` starts any of the three from a saved joint policy.
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

DEFAULT_WORKLOAD = "cte_8192x16x16_n4"
# what an option left out means, by algorithm: PPO as before --algo existed, IMPALA the reference's CTE IMPALA settings
ALGO_DEFAULTS = {
    "PPO": {"hidden": 64, "lr": 1e-4, "ent_coeff": 0.01, "vf_coeff": 1.0, "epochs": 10},
    "IMPALA": {"hidden": 256, "lr": 1e-3, "ent_coeff": 0.001, "vf_coeff": 0.3, "epochs": 1},
    "BC": {"hidden": 64, "lr": 1e-3, "ent_coeff": 0.0, "vf_coeff": 0.0, "epochs": 1},
}



def kl_settings(args) -> dict:
    """The PPOLearner arguments of --kl-coeff / --kl-target / --fused-objective."""
    on = args.kl_coeff is not None or args.kl_target is not None
    return {"kl_coeff": (0.2 if args.kl_coeff is None else args.kl_coeff) if on else None,
            "kl_target": 0.01 if args.kl_target is None else args.kl_target, "fused_objective": args.fused_objective}


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--workload", default=None, help=f"a single-agent workload of dl_reference_models_amd.workloads (default {DEFAULT_WORKLOAD} "
                                                    "unless --env-name is given)")
    p.add_argument("--env-name", default=None, help="a named grid of the reference instead of a workload")
    p.add_argument("--num-agents", type=int, default=4, help="with --env-name")
    p.add_argument("--steps-per-episode", type=int, default=None, help="default: the workload's, or 100")
    p.add_argument("--deterministic", action="store_true")
    p.add_argument("--num-envs", type=int, default=None, help="default: the workload's, or 1024")
    p.add_argument("--seed", type=int, default=42, help="env b is seeded with seed + b; weights, minibatches and sampling draw from it too")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--iters", type=int, default=100)
    p.add_argument("--T", type=int, default=32, help="steps per fragment")
    p.add_argument("--algo", choices=tuple(ALGO_DEFAULTS), default="PPO")
    p.add_argument("--hidden", type=int, choices=(64, 256), default=None, help="default: 64 (PPO, BC), 256 (IMPALA); 256 is feed-forward")
    p.add_argument("--push-every", type=int, default=1, help="push the weights to the policy kernel every K iterations")
    p.add_argument("--epochs", type=int, default=None, help="default: 10 (PPO), 1 (IMPALA)")
    p.add_argument("--minibatches", type=int, default=8)
    p.add_argument("--lr", type=float, default=None, help="default: 1e-4 (PPO), 1e-3 (IMPALA)")
    p.add_argument("--clip", type=float, default=0.2, help="PPO only")
    p.add_argument("--ent-coeff", type=float, default=None, help="default: 0.01 (PPO), 0.001 (IMPALA)")
    p.add_argument("--vf-coeff", type=float, default=None, help="default: 1.0 (PPO), 0.3 (IMPALA)")
    p.add_argument("--gamma", type=float, default=0.99)
    p.add_argument("--lam", type=float, default=0.95, help="PPO only (GAE)")
    p.add_argument("--feed-forward", action="store_true", help="no LSTM (always so with --hidden 256)")
    p.add_argument("--torch-learner", action="store_true", help="the recurrence as a loop of torch ops instead of the fused kernels")
    p.add_argument("--kl-coeff", type=float, default=None, help="PPO only: RLlib's adaptive KL penalty, starting at this coefficient (the "
                   "reference trains with 0.2); with neither this nor --kl-target there is no KL term")
    p.add_argument("--kl-target", type=float, default=None, help="PPO only: the KL the coefficient is adapted towards (default 0.01; given "
                   "alone it switches the term on at a coefficient of 0.2)")
    p.add_argument("--fused-objective", action=argparse.BooleanOptionalAction, default=None,
                   help="PPO only: the objective in one launch of mapf_ppo_loss instead of torch ops (default: the learner's)")
    p.add_argument("--fused-trunk", action="store_true", help="refused here: the trunk kernels (mapf_trunk_*) take the multi-agent env's "
                   "shared policy, not a joint policy (scripts/train_multi_agent_env.py offers it)")
    p.add_argument("--fused-grads", action="store_true", help="dW_hh of the recurrence as one split-row reduction "
                   "(mapf_lstm_seq_param_grad) instead of a GEMM over a materialised hprev")
    bc = p.add_argument_group("BC only (behaviour cloning of a device planner)")
    bc.add_argument("--expert", choices=("yielding", "independent", "windowed"), default="yielding",
                    help="the planner that labels every step (windowed: refused, it is offered on the multi-agent env only)")
    bc.add_argument("--expert-window", type=int, default=8)
    bc.add_argument("--beta-start", type=float, default=0.0, help="the share of steps that execute the expert's actions, at iteration 0")
    bc.add_argument("--beta-end", type=float, default=0.0, help="... and from iteration --beta-iters on")
    bc.add_argument("--beta-iters", type=int, default=0, help="iterations over which beta goes from --beta-start to --beta-end")
    p.add_argument("--init-checkpoint", type=Path, default=None, help="start from this saved joint policy (JointActionPolicy.load)")
    p.add_argument("--checkpoint", type=Path, default=None, help="where the trained policy is written")
    p.add_argument("--save-every", type=int, default=0)
    p.add_argument("--log", type=Path, default=None, help="also append the per-iteration lines to this file")
    args = p.parse_args(argv)
    for name, value in ALGO_DEFAULTS[args.algo].items():
        if getattr(args, name) is None:
            setattr(args, name, value)
    args.feed_forward = args.feed_forward or args.hidden == 256
    return args


def make_module(args, grid_cells: int, num_agents: int):
    """The module the parsed arguments ask for (on the CPU)."""
    from dl_reference_models_amd.policy import JointActionPolicy

    return JointActionPolicy(grid_cells, num_agents, recurrent=not args.feed_forward, hidden=args.hidden)


def make_env(args):
    from dl_reference_models_amd import workloads as wl
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    if args.env_name and not args.workload:
        cfg = {"env_name": args.env_name, "seed": args.seed, "deterministic": args.deterministic, "num_agents": args.num_agents,
               "steps_per_episode": args.steps_per_episode or 100, "num_envs": args.num_envs or 1024, "device": args.device}
        return VecSingleAgentReferenceModel(cfg)
    name = args.workload or DEFAULT_WORKLOAD
    if name not in wl.WORKLOADS or not wl.is_single_agent(name):
        raise SystemExit(f"--workload must be one of {[k for k in wl.WORKLOADS if wl.is_single_agent(k)]}")
    b = args.num_envs or wl.WORKLOADS[name][0]
    cfg = wl.workload_config(name, list(range(b)))
    cfg["seeds"] = [args.seed + i for i in range(b)]
    cfg["device"] = args.device
    if args.steps_per_episode:
        cfg["steps_per_episode"] = args.steps_per_episode
    if args.deterministic:
        cfg["deterministic"] = True
    return VecSingleAgentReferenceModel(cfg)


def main(argv=None) -> dict:
    args = parse_args(argv)
    import torch

    from dl_reference_models_amd.learner import BCLearner, IMPALALearner, PPOLearner, Trainer
    from dl_reference_models_amd.policy import JointActionPolicy

    if args.fused_trunk:  # the learners' own refusal, before an env is built
        from dl_reference_models_amd.learner import check_trunk_module

        try:
            check_trunk_module(JointActionPolicy(4, 1))
        except ValueError as e:
            raise SystemExit(f"--fused-trunk: {e}") from None
    env = make_env(args)
    torch.manual_seed(args.seed)
    H, W = env.grid_shape
    if args.init_checkpoint is not None:
        module = JointActionPolicy.load(args.init_checkpoint)
        if module.grid_cells != H * W or module.num_agents != env.num_agents:
            raise SystemExit(f"--init-checkpoint {args.init_checkpoint} was trained on another env: its config is {module.config()}, "
                             f"this env has {H * W} cells and {env.num_agents} agents")
        module = module.to(env.device)
    else:
        module = make_module(args, H * W, env.num_agents).to(env.device)
    if args.algo == "BC":
        schedule = [(0, args.beta_start), (args.beta_iters, args.beta_end)] if args.beta_iters > 0 else [(0, args.beta_start)]
        learner = BCLearner(module, lr=args.lr, vf_coeff=args.vf_coeff, ent_coeff=args.ent_coeff, epochs=args.epochs,
                            minibatches=args.minibatches, seed=args.seed, fused=not args.torch_learner,
                            fused_objective=False if args.torch_learner else args.fused_objective, expert=args.expert,
                            expert_window=args.expert_window, beta_schedule=schedule)
    elif args.algo == "IMPALA":
        learner = IMPALALearner(module, lr=args.lr, vf_coeff=args.vf_coeff, ent_coeff=args.ent_coeff, gamma=args.gamma,
                                epochs=args.epochs, minibatches=args.minibatches, seed=args.seed, fused=not args.torch_learner)
    else:
        learner = PPOLearner(module, lr=args.lr, clip=args.clip, vf_coeff=args.vf_coeff, ent_coeff=args.ent_coeff, epochs=args.epochs,
                             minibatches=args.minibatches, seed=args.seed, fused=not args.torch_learner, **kl_settings(args))
    trainer = Trainer(env, module, T=args.T, learner=learner, gamma=args.gamma, lam=args.lam, sample_seed=args.seed,
                      push_every=args.push_every, fused_grads=args.fused_grads)
    if args.checkpoint:
        args.checkpoint.parent.mkdir(parents=True, exist_ok=True)
    log = args.log.open("a", encoding="utf-8") if args.log else None
    history = []
    for it in range(args.iters):
        t0 = time.perf_counter()
        stats = trainer.iterate()
        stats["seconds"] = time.perf_counter() - t0
        stats["env_steps_per_s"] = env.num_envs * args.T / stats["seconds"]
        stats["terminated_share"] = stats["terminated"] / stats["episodes"] if stats["episodes"] else None  # the success rate
        line = json.dumps(stats)
        print(line, flush=True)
        if log:
            log.write(line + "\n")
            log.flush()
        history.append(stats)
        if args.checkpoint and args.save_every and (it + 1) % args.save_every == 0:
            module.save(args.checkpoint)
    env.poll_error()
    if args.checkpoint:
        module.save(args.checkpoint)
        print(f"Checkpoint saved to {args.checkpoint} (evaluate it with scripts/evaluate_single_agent_env.py --policy NEURAL "
              f"--checkpoint {args.checkpoint})")
    if log:
        log.close()
    env.close()
    return {"history": history, "checkpoint": args.checkpoint, "config": module.config()}


if __name__ == "__main__":
    main()
