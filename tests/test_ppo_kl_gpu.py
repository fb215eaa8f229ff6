"""PPO's KL penalty on the device, on real fragments of the three layouts (shared rows, joint rows with N heads, one policy
per agent): the logits slab of the rollout, the learner's objective through ``mapf_ppo_loss`` and through torch ops against
the float64 oracle of ppo_loss_util, the coefficient's adaptation, and a ``Trainer`` that runs it."""

import copy

import numpy as np
import pytest
import torch

import dte_util as du
import joint_learner_util as jl
import joint_policy_util as ju
import learner_util as lu
import policy_util as pu
import ppo_loss_util as plu
from trace_util import synth_grids

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LAYOUTS = ("shared", "joint", "per_agent")
B, N, T = 6, 3, 5
# a second length, beyond one chunk of the objective kernel: with 7-step episodes the second fragment collected has episode
# ends on both sides of t = 8 and of t = 32, where V-trace's and PPO's chunks of 40 steps begin
T_LONG, SPE_LONG = 40, 7
LOGITS_MARGIN = 16  # what tests/test_policy_gpu.py allows the act kernels' logits, times dev


def _env(layout, spe=3):
    from dl_reference_models_amd.vec_env import VecReferenceModel
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    cfg = {"grid": synth_grids(B, 8, 8, 0.15, N), "num_envs": B, "num_agents": N, "steps_per_episode": spe, "seeds": list(range(B)),
           "device": DEV}
    if layout == "joint":
        return VecSingleAgentReferenceModel(cfg)
    return VecReferenceModel(dict(cfg, sensor_range=1, include_action_mask_in_obs=True))


def _module(layout, env, seed=2):
    if layout == "joint":
        return ju.make_module(64, N, True, seed=seed).train()
    if layout == "per_agent":
        return du.make_per_agent(N, env.obs_len, True, True, seed=seed).train()
    return pu.make_module(env.obs_len, True, True, seed=seed).train()


def _rollout(layout, env, module, T=T, **kw):
    from dl_reference_models_amd.policy import DevicePolicy, JointDevicePolicy
    from dl_reference_models_amd.rollout import JointRollout, Rollout

    if layout == "joint":
        return JointRollout(env, JointDevicePolicy(module, B, DEV), T, sample=True, seed=11, **kw)
    return Rollout(env, DevicePolicy(module, B * N, N, DEV), T, sample=True, seed=11, **kw)


def _real(layout, T, spe):
    """The second fragment of a sampling rollout that keeps its logits (h0, c0 and prev_action0 are not zero), on the device
    and on the host, with the module that produced it."""
    env = _env(layout, spe)
    module = _module(layout, env)
    ro = _rollout(layout, env, module, T, keep_logits=True)
    ro.collect()
    frag_dev = {k: v.clone() for k, v in ro.collect().items()}
    torch.cuda.synchronize()
    env.poll_error()
    frag = {k: v.cpu() for k, v in frag_dev.items()}
    assert (frag["terminated"] | frag["truncated"]).any() and frag["h0"].abs().max() > 0
    return {"layout": layout, "T": T, "module": module, "frag_dev": frag_dev, "frag": frag,
            "frag64": {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}}


@pytest.fixture(scope="module", params=LAYOUTS)
def real(request):
    return _real(request.param, T, 3)


@pytest.fixture(scope="module", params=LAYOUTS)
def real_long(request):
    """A fragment of 40 steps: the objective kernel takes it as two chunks, and episodes end in both and at neither edge."""
    r = _real(request.param, T_LONG, SPE_LONG)
    steps = torch.nonzero((r["frag"]["terminated"] | r["frag"]["truncated"]).reshape(T_LONG, -1).any(dim=1)).reshape(-1)
    assert (steps < 8).any() and (steps >= 32).any() and ((steps >= 8) & (steps < 32)).any(), steps.tolist()
    return r


def _chained(layout, module, frag):
    return (jl if layout == "joint" else lu).chained_forward(module, frag)


def _slab_check(real):
    from dl_reference_models_amd import learner as ln

    layout, module, frag, T = real["layout"], real["module"], real["frag"], real["T"]
    heads = N if layout == "joint" else 1
    R = B if layout == "joint" else B * N
    assert tuple(frag["logits"].shape) == ((T, B, 5 * N) if layout == "joint" else (T, B, N, 5))
    want, _ = _chained(layout, copy.deepcopy(module).double(), real["frag64"])
    cpu32, _ = _chained(layout, copy.deepcopy(module), frag)
    want = want.detach().numpy().reshape(T, R, 5 * heads)
    dev = float(np.abs(cpu32.detach().numpy().reshape(T, R, 5 * heads) - want).max())
    assert 0 < dev < 1e-5
    slab = frag["logits"].reshape(T, R, 5 * heads).numpy()
    again, _ = ln.sequence_forward(copy.deepcopy(module).to(DEV), real["frag_dev"])
    again = again.detach().cpu().reshape(T, R, 5 * heads).numpy()
    err = [float(np.abs(x.astype(np.float64) - want).max()) for x in (slab, again)]
    print(f"ppo kl, {layout} T={T}: logits slab {err[0]:.3e}, recomputed {err[1]:.3e} / dev {dev:.3e}")
    assert max(err) <= LOGITS_MARGIN * dev
    # and the KL between the two, evaluated in float64 (in fp32 the sum is rounding noise of the order of 1e-7)
    t64 = {k: torch.from_numpy(np.ascontiguousarray(x)).double() for k, x in (("new", again), ("old", slab))}
    z = torch.zeros(T, R, dtype=torch.float64)
    out = plu.ppo_terms(t64["new"], z, t64["old"], real["frag"]["actions"].reshape(T, R, heads), z, z, z,
                        torch.ones(1, dtype=torch.float64), {"clip": 0.2, "vf_clip": 1.0, "vf_coeff": 0.0, "ent_coeff": 0.0})
    assert -1e-15 <= float(out["kl"].min()) and float(out["kl"].max()) <= (LOGITS_MARGIN * dev) ** 2 * heads


def test_the_slab_holds_the_logits_the_learner_recomputes(real):
    _slab_check(real)


def test_the_slab_holds_the_logits_of_a_fragment_beyond_one_chunk(real_long):
    _slab_check(real_long)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_without_keep_logits_the_fragment_is_todays(layout):
    frags = []
    for keep in (False, True):
        env = _env(layout)
        ro = _rollout(layout, env, _module(layout, env), **({"keep_logits": True} if keep else {}))
        per_call = []
        for _ in range(3):  # launched, captured, replayed
            per_call.append({k: v.clone() for k, v in ro.collect().items()})
        torch.cuda.synchronize()
        env.poll_error()
        frags.append(per_call)
        assert ro.keep_logits == keep and (ro._logits is not None) == keep
    from dl_reference_models_amd import learner as ln

    for bare, kept in zip(*frags):
        assert "logits" not in bare and set(bare) == set(ln.FRAGMENT_KEYS) and set(kept) == set(bare) | {"logits"}
        for k, v in bare.items():
            assert torch.equal(v, kept[k]) and v.dtype == kept[k].dtype, k
        assert kept["logits"].abs().max() > 0


def _perturbed(real):
    """The module after one Adam step of the torch learner on the CPU: the behaviour policy is no longer the current one."""
    from dl_reference_models_amd import learner as ln

    module = copy.deepcopy(real["module"])
    frag = {k: v for k, v in real["frag"].items() if k != "logits"}
    adv, tgt = ln.gae(frag)
    ln.PPOLearner(module, fused=False, lr=5e-3, epochs=1, minibatches=1).update(frag, adv, tgt)
    return module


def _by_hand(layout, module, frag, adv, targets, hp, coeff, groups):
    """ppo_loss_util.ppo_terms on T chained ``module.forward`` calls in the module's dtype on the CPU: the loss terms per
    group and the flat parameter gradient, as float64 NumPy."""
    module.zero_grad()
    logits, values = _chained(layout, module, frag)
    T, R = values.shape
    heads = N if layout == "joint" else 1
    dt = values.dtype
    out = plu.ppo_terms(logits.reshape(T, R, 5 * heads), values, frag["logits"].reshape(T, R, 5 * heads).to(dt),
                        frag["actions"].reshape(T, R, heads), frag["logp"].reshape(T, R).to(dt), adv.reshape(T, R).to(dt),
                        targets.reshape(T, R).to(dt), coeff.to(dt), hp, groups)
    out["total_loss"].backward()
    loss = torch.stack([out["total_loss"].detach().reshape(1).expand(groups)] + [out[k].detach() for k in plu.SUMMED])
    return {"loss": loss.double().numpy(), "gradient": torch.cat([p.grad.reshape(-1) for p in module.parameters()]).double().numpy(),
            "kl": out["kl_mean"].detach().double().numpy()}


def _learner_terms(ln, module, frag, adv, targets, hp, coeff, fused_objective):
    learner = ln.PPOLearner(module, kl_coeff=0.2, fused_objective=fused_objective, **hp)
    learner.kl_coeff.copy_(coeff)
    module.zero_grad()
    terms = learner.losses(frag, adv, targets)
    terms["total_loss"].backward()
    per = terms.get("per_policy", terms)
    G = learner.kl_coeff.numel()
    loss = torch.stack([terms["total_loss"].detach().reshape(1).expand(G)]
                       + [per[k].detach().reshape(G) for k in ("policy_loss", "vf_loss", "entropy", "kl")])
    flat = torch.cat([p.grad.reshape(-1) for p in module.parameters()])
    return {"loss": loss.double().cpu().numpy(), "gradient": flat.detach().double().cpu().numpy()}


def _oracle_check(real):
    """dev: the deviation of the same by-hand computation in fp32 on the CPU from the float64 one, for the loss terms together
    and for the flat gradient; the fused objective and the torch ops on the device within ppo_loss_util.GEMM_MARGIN times it."""
    from dl_reference_models_amd import learner as ln

    layout, frag, frag64 = real["layout"], real["frag"], real["frag64"]
    G = N if layout == "per_agent" else 1
    module = _perturbed(real)
    util = jl if layout == "joint" else lu
    adv64, tgt64 = (torch.from_numpy(x) for x in util.gae64(frag, 0.99, 0.95))
    adv64 = du.standardised_per_agent(adv64) if layout == "per_agent" else util.standardised(adv64)
    hp = {"clip": 0.2, "vf_clip": 0.8, "vf_coeff": 0.7, "ent_coeff": 0.03}
    coeff = torch.from_numpy(plu.group_coeffs(G, 0.2))
    want = _by_hand(layout, copy.deepcopy(module).double(), frag64, adv64, tgt64, hp, coeff, G)
    cpu32 = _by_hand(layout, copy.deepcopy(module), frag, adv64.float(), tgt64.float(), hp, coeff, G)
    dev = {k: float(np.abs(cpu32[k] - want[k]).max()) for k in ("loss", "gradient")}
    assert 0 < dev["loss"] < 1e-5 and 0 < dev["gradient"] < 1e-4
    assert want["kl"].min() > 1e-5 and np.abs(want["gradient"]).max() > 1e-3  # the step moved every policy
    adv_d, tgt_d = adv64.float().to(DEV), tgt64.float().to(DEV)
    for fused_objective in (True, False):
        got = _learner_terms(ln, copy.deepcopy(module).to(DEV), real["frag_dev"], adv_d, tgt_d, hp, coeff.to(DEV), fused_objective)
        err = {k: float(np.abs(got[k] - want[k]).max()) for k in got}
        print(f"ppo kl on a real fragment, {layout} T={real['T']} fused_objective={fused_objective}: loss terms {err['loss']:.3e} / "
              f"{dev['loss']:.3e} = {err['loss'] / dev['loss']:.2f}, gradient {err['gradient']:.3e} / {dev['gradient']:.3e} = "
              f"{err['gradient'] / dev['gradient']:.2f}")
        assert err["loss"] <= plu.GEMM_MARGIN * dev["loss"], (fused_objective, err, dev)
        assert err["gradient"] <= plu.GEMM_MARGIN * dev["gradient"], (fused_objective, err, dev)


def test_losses_and_gradient_against_the_float64_oracle(real):
    _oracle_check(real)


def test_losses_and_gradient_of_a_fragment_beyond_one_chunk(real_long):
    """rollout -> fragment view -> forward -> fused objective -> autograd at T = 40: the kernel's second chunk, on real data."""
    _oracle_check(real_long)


@pytest.mark.parametrize("fused_objective", (True, False), ids=("fused", "torch_ops"))
def test_update_adapts_the_coefficient_on_the_device(real, fused_objective):
    from dl_reference_models_amd import learner as ln

    layout = real["layout"]
    G = N if layout == "per_agent" else 1
    module = copy.deepcopy(real["module"]).to(DEV)
    frag = real["frag_dev"]
    adv, tgt = ln.gae(frag)
    # targets on both sides of what a first update samples: policy by policy x 1.5, x 0.5 or unchanged
    probe = ln.PPOLearner(copy.deepcopy(module), kl_coeff=0.2, epochs=2, minibatches=2, seed=3, fused_objective=fused_objective)
    kl0 = probe.update(frag, adv, tgt)["kl"]
    for scale in (0.1, 1.0, 10.0):
        learner = ln.PPOLearner(copy.deepcopy(module), kl_coeff=0.2, kl_target=scale * float(kl0), epochs=2, minibatches=2, seed=3,
                                fused_objective=fused_objective)
        before = learner.kl_coeff.clone()
        out = learner.update(frag, adv, tgt)
        assert all(v.is_cuda for k, v in out.items() if k != "per_policy") and learner.kl_coeff.is_cuda and learner.sampled_kl.is_cuda
        kl = (out["per_policy"]["kl"] if G > 1 else out["kl"].reshape(1)).cpu()
        assert tuple(kl.shape) == (G,) and torch.equal(kl, learner.sampled_kl.cpu())
        target = learner.kl_target
        factor = torch.where(kl > 2.0 * target, 1.5, torch.where(kl < 0.5 * target, 0.5, 1.0)).to(torch.float32)
        assert torch.equal(learner.kl_coeff.cpu(), before.cpu() * factor), (scale, kl, learner.kl_coeff)
        assert torch.equal(out["kl_coeff"].cpu(), learner.kl_coeff.mean().cpu())
        assert set(factor.tolist()) == {{0.1: 1.5, 1.0: 1.0, 10.0: 0.5}[scale]} or G > 1
        if G > 1:
            assert torch.equal(out["per_policy"]["kl_coeff"], learner.kl_coeff)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_trainer_reports_kl_and_its_coefficient(layout):
    from dl_reference_models_amd import learner as ln

    env = _env(layout)
    module = _module(layout, env, seed=3).to(DEV)
    learner = ln.PPOLearner(module, epochs=2, minibatches=3, seed=1, kl_coeff=0.2, fused_objective=True)
    trainer = ln.Trainer(env, module, T=T, learner=learner, sample_seed=5)
    assert trainer.rollout.keep_logits
    stats = [trainer.iterate() for _ in range(2)]  # the second fragment is a graph replay
    for s in stats:
        assert all(np.isfinite(s[k]) for k in ("total_loss", "policy_loss", "vf_loss", "entropy", "kl", "kl_coeff")) and s["kl"] > -1e-6
        if layout == "per_agent":
            assert len(s["per_policy"]["kl"]) == N and len(s["per_policy"]["kl_coeff"]) == N
    assert stats[1]["kl_coeff"] in (pytest.approx(0.2 * f * g) for f in (0.5, 1.0, 1.5) for g in (0.5, 1.0, 1.5)) or layout == "per_agent"
    plain = ln.Trainer(_env(layout), module, T=T, learner=ln.PPOLearner(module, epochs=1, minibatches=2), sample_seed=5)
    assert not plain.rollout.keep_logits and "kl" not in plain.iterate()
    env.poll_error()
