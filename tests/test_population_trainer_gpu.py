"""A population of policies on the device: the PPO learner of P members with their own hyperparameters on the fused kernels
against the float64 CPU recomputation per member, and the chain PopulationTrainer -> perturbation -> best() -> evaluate, and
the training script with --population, end to end.

Tolerances of the learner test: ``dev`` is the deviation of the same computation in fp32 on the CPU from the float64 one
(population_util.ppo_by_hand: learner_util's chained ``forward`` calls and PPO objective on each member's own net, envs and
hyperparameters; it shares no code with the learner).  The margins are the next power of two at or above twice the largest
ratio measured on the MI355X (DESIGN.md 4aa holds the table, profiles/r25/population/parity_deviation.txt the raw lines):
forward 2.39 x dev (loss terms 0.18) -> 8, gradient 1.81 x dev -> 4, on the fused recurrence and on torch ops alike (the DTE
learner's, DESIGN.md 4r: 2.3 and 0.93, margins 16 and 32)."""

import copy
import importlib.util
import os

import numpy as np
import pytest
import torch

import learner_util as lu
import population_util as popu
from population_util import DEV
from trace_util import ROOT, synth_grids

pytestmark = pytest.mark.gpu

FORWARD_MARGIN = 8  # 2 x 2.39 = 4.8
GRAD_MARGIN = 4  # 2 x 1.81 = 3.6
HYPERS = ({"clip": 0.25, "vf_coeff": 0.5, "ent_coeff": 0.015625, "vf_clip": 1.0},
          {"clip": 0.125, "vf_coeff": 0.75, "ent_coeff": 0.0, "vf_clip": 2.0})  # (exact in float32, as the learner stores them)
GAMMAS, LAMS = (0.9, 0.99), (0.8, 0.95)


def test_loss_and_gradient_of_p_members_against_the_float64_recomputation():
    """(P, N, B, T) = (2, 3, 12, 5), the mask on, three-step episodes (an env ends one every third step, staggered over the
    envs): 36 interleaved rows in 6 groups of 6.  Every member has its own clip, vf_clip, vf_coeff, ent_coeff, gamma and
    lambda; both clips bind on a part of its elements."""
    from dl_reference_models_amd import learner as ln

    P, N, B, T, L = 2, 3, 12, 5, 16
    trunc = ((np.arange(T)[:, None] + np.arange(B)[None, :]) % 3 == 2).astype(np.uint8)
    frag = lu.synthetic_fragment(T, B, N, L, True, seed=8, flags=(trunc, trunc))
    frag64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}
    adv64, tgt64 = torch.zeros(T, B, N, dtype=torch.float64), torch.zeros(T, B, N, dtype=torch.float64)
    for p in range(P):
        a, t = lu.gae64(popu.member_fragment(frag, p, P), GAMMAS[p], LAMS[p])
        adv64[:, p::P], tgt64[:, p::P] = torch.from_numpy(a), torch.from_numpy(t)
    adv64 = popu.standardised_per_member(adv64, P)
    module = popu.make_population(P, N, L, True, True).train()
    want = popu.ppo_by_hand(copy.deepcopy(module).double(), frag64, adv64, tgt64, HYPERS)
    cpu32 = popu.ppo_by_hand(copy.deepcopy(module), frag, adv64.float(), tgt64.float(), HYPERS)
    for p in range(P):
        assert 0.02 < want["ratio_binds"][p] < 0.98 and 0.02 < want["vf_binds"][p] < 0.98, (want["ratio_binds"], want["vf_binds"])
    dev = {k: float(np.abs(cpu32[k] - want[k]).max()) for k in ("forward", "gradient")}
    assert 0 < dev["forward"] < 1e-5 and 0 < dev["gradient"] < 1e-4
    frag_dev = {k: v.to(DEV) for k, v in frag.items()}
    # the advantages the learner is handed: gae with per-row discounts on the device, standardised by update()'s rule
    env_of = lambda xs: torch.tensor(xs, dtype=torch.float64, device=DEV).repeat(B // P)[:, None]  # noqa: E731
    adv_g, tgt_g = ln.gae(frag_dev, env_of(GAMMAS), env_of(LAMS))
    raw64 = torch.zeros_like(adv64)
    for p in range(P):
        raw64[:, p::P] = torch.from_numpy(lu.gae64(popu.member_fragment(frag, p, P), GAMMAS[p], LAMS[p])[0])
    assert float((adv_g.double().cpu() - raw64).abs().max()) <= 1e-5 and float((tgt_g.double().cpu() - tgt64).abs().max()) <= 1e-5
    adv_d, tgt_d = adv64.float().to(DEV), tgt64.float().to(DEV)
    f64 = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
    for fused in (True, False):
        m = copy.deepcopy(module).to(DEV)
        learner = ln.PPOLearner(m, fused=fused)
        assert learner.fused_objective
        for p, h in enumerate(HYPERS):
            learner.set_hyper(p, **h)
        logits, value = ln.sequence_forward(m, frag_dev, fused=fused)
        assert logits.shape == (T, B // P, P * N, 5) and value.shape == (T, B // P, P * N)
        terms = learner.losses(frag_dev, adv_d, tgt_d)
        terms["total_loss"].backward()
        got = {"forward": popu.forward_by_member(f64(logits).reshape(T, B, N, 5), f64(value).reshape(T, B, N), P),
               "loss": np.stack([f64(terms["per_policy"][k]) for k in lu.LOSS_TERMS], axis=1),
               "gradient": f64(torch.cat([x.grad.reshape(-1) for x in m.parameters()]))}
        err = {k: float(np.abs(got[k] - want[k]).max()) for k in got}
        total = abs(float(terms["total_loss"].detach()) - want["loss"][:, 0].sum())
        print(f"population learner, fused={fused}: forward {err['forward']:.3e} / {dev['forward']:.3e} = {err['forward'] / dev['forward']:.2f}, "
              f"loss terms {err['loss']:.3e} = {err['loss'] / dev['forward']:.2f}, summed loss {total:.3e}, "
              f"gradient {err['gradient']:.3e} / {dev['gradient']:.3e} = {err['gradient'] / dev['gradient']:.2f}")
        assert err["forward"] <= FORWARD_MARGIN * dev["forward"], (fused, err, dev)
        assert err["loss"] <= FORWARD_MARGIN * dev["forward"] and total <= P * FORWARD_MARGIN * dev["forward"], (fused, err, total)
        assert err["gradient"] <= GRAD_MARGIN * dev["gradient"], (fused, err, dev)


def _env(B=16, N=3, spe=8, mask=True):
    from dl_reference_models_amd.vec_env import VecReferenceModel

    return VecReferenceModel({"grid": synth_grids(B, 8, 8, 0.15, N), "num_envs": B, "num_agents": N, "sensor_range": 1,
                              "steps_per_episode": spe, "seeds": list(range(B)), "include_action_mask_in_obs": mask, "device": DEV})


def test_trainer_perturbs_exploits_saves_and_its_best_member_evaluates(tmp_path):
    """P = 4, 16 envs, T = 8 = steps_per_episode: every env ends an episode in every fragment, so no member is left out of a
    perturbation; two perturbations in four iterations."""
    from dl_reference_models_amd import evaluation as ev
    from dl_reference_models_amd import population as pop
    from dl_reference_models_amd.policy import MaskedRecurrentPolicy

    P, B, N, T = 4, 16, 3, 8
    env = _env(B, N, T)
    module = popu.make_population(P, N, env.obs_len, True, True, seed=2).train().to(DEV)
    hypers = [pop.Hyper(lr=1e-3 / (p + 1), clip=0.05 * (p + 1)) for p in range(P)]
    trainer = pop.PopulationTrainer(env, module, T=T, hyper=hypers, pbt=pop.PBT(perturb_every=2, seed=1), epochs=2, minibatches=2,
                                    kl_coeff=0.2, seed=3, sample_seed=5)
    assert trainer.policy.population
    with pytest.raises(ValueError, match="no multiple"):
        pop.PopulationTrainer(_env(6, N, T), popu.make_population(P, N, env.obs_len, True, True).to(DEV))
    count = module.members[0].flat_params().numel()
    perturbations = 0
    for it in range(4):
        before = [m.flat_params().clone() for m in module.members]
        out = trainer.iterate()
        assert out["iteration"] == it + 1 and out["episodes"] >= B and np.isfinite(out["reward_per_step"])
        per = out["per_member"]
        assert all(len(per[k]) == P and np.isfinite(per[k]).all() for k in lu.LOSS_TERMS + ("kl", "kl_coeff"))
        assert all(s is not None and np.isfinite(s) for s in per["score"]), per["score"]  # no member without an ended episode
        assert out["best_score"] == max(per["score"]) and abs(out["mean_score"] - np.mean(per["score"])) < 1e-9
        assert [h["vf_coeff"] for h in per["hyper"]] == [0.5] * P
        if (it + 1) % 2:
            assert out["perturbed"] == [] and all(not torch.equal(m.flat_params(), b) for m, b in zip(module.members, before))
            continue
        perturbations += 1
        assert len(out["perturbed"]) == 1  # ceil(4 / 4) receivers
        (receiver, donor), = out["perturbed"]
        ranked = sorted(range(P), key=lambda p: (per["score"][p], p))
        assert receiver == ranked[0] and donor == ranked[-1]
        # the exploit: the receiver's weights are the donor's in the module, in what the policy kernel was handed, and in
        # what the kernel computes -- the same observation in one env of each gives the same bits
        assert torch.equal(module.members[receiver].flat_params(), module.members[donor].flat_params())
        staged = trainer.policy._params.view(P, count)
        assert torch.equal(staged[receiver], staged[donor]) and torch.equal(staged[donor], module.members[donor].flat_params())
        assert not torch.equal(staged[receiver], staged[ranked[1]])
        rng = np.random.default_rng(it)
        one = rng.integers(0, 2, size=(N, env.obs_len)).astype(np.float32)
        one[:, env.obs_len - 5] = 1.0
        obs = torch.from_numpy(np.tile(one, (B, 1))).to(DEV)
        ones = torch.ones((B,), dtype=torch.uint8, device=DEV)
        logits = trainer.policy.act(obs, start=(ones, None), peek=True)["logits"].view(B, N, 5).clone()
        assert torch.equal(logits[receiver].view(torch.uint8), logits[donor].view(torch.uint8))
        assert not torch.equal(logits[receiver], logits[ranked[1]])
        # a rebuilt trial: no Adam state, the initial KL coefficient, the donor's hyperparameters explored inside the ranges,
        # a cleared recurrent state in its envs and a score window that starts again
        assert all(prm not in trainer.learner.optimizer.state for prm in module.members[receiver].parameters())
        assert float(trainer.learner.kl_coeff[receiver]) == pytest.approx(0.2)
        h = trainer.hypers[receiver]
        assert all(lo <= getattr(h, k) <= hi for k, (lo, hi) in pop.DEFAULT_RANGES.items())
        assert trainer.learner.optimizer.param_groups[receiver]["lr"] == h.lr
        assert float(trainer.learner.hp[receiver, 0]) == pytest.approx(h.clip)
        hstate = trainer.policy.h.view(B // P, P, N, 64)
        assert not hstate[:, receiver].any() and hstate[:, donor].any()
        # ... (every env has just ended an episode at the time limit or is inside one: only those lose their first end)
        assert not trainer.score.count.any() and torch.equal(trainer.score.skip.view(-1, P)[:, receiver], trainer.score.open.view(-1, P)[:, receiver])
        assert not trainer.score.skip.view(-1, P)[:, donor].any()
    assert perturbations == 2 and len(trainer.perturbations) == 2 and trainer.rollout._graph is not None
    env.poll_error()
    # save -> load into a second trainer: the same members, hyperparameters, optimizer and generators
    path = tmp_path / "population.pt"
    trainer.save(path)
    other_module = popu.make_population(P, N, env.obs_len, True, True, seed=9).train().to(DEV)
    other = pop.PopulationTrainer(_env(B, N, T), other_module, T=T, pbt=pop.PBT(perturb_every=2, seed=77), epochs=2, minibatches=2,
                                  kl_coeff=0.2, seed=3, sample_seed=5)
    other.load(path)
    assert torch.equal(other_module.flat_params(), module.flat_params()) and other.hypers == trainer.hypers
    assert other.iterations == 4 and other.perturbations == trainer.perturbations and other.scores == trainer.scores
    assert torch.equal(other.learner.hp, trainer.learner.hp) and torch.equal(other.learner.kl_coeff, trainer.learner.kl_coeff)
    assert torch.equal(other.pbt.state(), trainer.pbt.state())
    scores = [1.0, 4.0, 2.0, 3.0]
    assert other.pbt.perturb(scores, other.hypers) == trainer.pbt.perturb(scores, trainer.hypers)
    # the best member is an ordinary shared policy that the evaluation takes
    best = trainer.best()
    assert isinstance(best, MaskedRecurrentPolicy) and trainer.best_member() == int(np.argmax(trainer.scores))
    assert torch.equal(best.flat_params(), module.members[trainer.best_member()].flat_params())
    env2 = _env(6, N, T)
    res, heat = ev.evaluate(env2, ev.neural_policy(env2, best), 2)
    assert len(res["env"]) == 12 and int(heat.sum()) > 0


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_trains_a_population_and_its_checkpoints_load(tmp_path, capsys):
    from dl_reference_models_amd.policy import load_policy

    train, evaluate = _script("train_multi_agent_env"), _script("evaluate_multi_agent_env")
    path, whole = tmp_path / "ckpt" / "best.pt", tmp_path / "ckpt" / "population.pt"
    shape = ["--env-name", "ReferenceModel-2-1", "--num-agents", "4", "--sensor-range", "2", "--steps-per-episode", "8"]
    out = train.main(shape + ["--population", "4", "--perturb-every", "1", "--pbt-seed", "2", "--num-envs", "16", "--iters", "2", "--T", "8",
                              "--epochs", "2", "--minibatches", "2", "--checkpoint", str(path), "--population-checkpoint", str(whole)])
    lines = [ln_ for ln_ in capsys.readouterr().out.splitlines() if ln_.startswith("{")]
    assert len(lines) == len(out["history"]) == 2 and out["history"][1]["iteration"] == 2
    last = out["history"][1]
    assert len(last["per_member"]["total_loss"]) == 4 and last["best_score"] is not None and last["mean_score"] <= last["best_score"]
    assert len(last["perturbed"]) == 1 and out["config"]["members"] == 4
    assert torch.load(path, map_location="cpu", weights_only=True)["kind"] == "masked_recurrent"
    assert type(load_policy(path)).__name__ == "MaskedRecurrentPolicy"
    assert torch.load(whole, map_location="cpu", weights_only=True)["kind"] == "population_trainer"
    res = evaluate.main(shape + ["--policy", "NEURAL", "--checkpoint", str(path), "--num-envs", "8", "--episodes", "1",
                                 "--output-dir", str(tmp_path / "eval")])
    assert len(res["table"]) == 8
    with pytest.raises(SystemExit, match="does not divide"):
        train.main(shape + ["--population", "3", "--num-envs", "16", "--iters", "1"])
