"""One policy per agent (DTE) on the device: a per-agent handle of the fused policy (mapf_policy_create_per_agent, then the
usual mapf_policy_* calls) through the raw C ABI with every output and state buffer guarded and poisoned (guard_util), the
learner of N independent nets on the fused kernels and on torch ops against the float64 CPU recomputation, and the chain
Rollout -> Trainer -> checkpoint -> evaluate end to end.

Bitwise: row r of a per-agent handle must equal, bit for bit, row r of a shared handle made from agent r % N's net and run
on the same full inputs and state -- the two launches differ in which rows share a tile, and a row's arithmetic does not
depend on its tile-mates.  Against the rule: 16 x dev on logits / value / h / c and 32 x dev on logp, the margins of
test_policy_gpu, dev = the deviation of the fp32 CPU module from the float64 restatement on the same case (dte_util.case).

Largest kernel deviations measured (DESIGN.md 4r holds the table): logits 2.77, value 2.00, h 1.46, c 3.01, logp 5.76 x dev."""

import copy
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import dte_util as du
import learner_util as lu
import policy_util as pu
from guard_util import GuardedBuffer
from trace_util import ROOT, synth_grids

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BYTE = 0xFF
OUTPUTS = ("action", "logp", "value", "logits")
STATE = ("h", "c", "draws")


def _lib():
    from dl_reference_models_amd import _lib as L

    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


class RawPolicy:
    """A policy handle through the raw C ABI with guarded state (h, c, draws) and guarded outputs.  module: a
    ``PerAgentPolicy`` (a per-agent handle) or a ``MaskedRecurrentPolicy`` (a shared one)."""

    def __init__(self, module, rows, n, set_params=True):
        self.L, self.lib = _lib()
        self.rows, self.n, self.module = rows, n, module
        self.per_agent = hasattr(module, "agents")
        self.h_ = C.c_void_p()
        cfg = self.L.MapfPolicyConfig(module.obs_len, module.mask_off, int(module.recurrent), n, 64, 0)
        create = self.lib.mapf_policy_create_per_agent if self.per_agent else self.lib.mapf_policy_create
        assert create(C.byref(cfg), C.byref(self.h_)) == self.L.MAPF_OK
        self.flat = module.flat_params().to(DEV)
        assert self.lib.mapf_policy_param_count(self.h_) == self.flat.numel()
        if set_params:
            self.set_params(self.flat)
        shapes = {"h": ((rows, 64), np.float32), "c": ((rows, 64), np.float32), "draws": ((rows,), np.uint32),
                  "action": ((rows,), np.int8), "logp": ((rows,), np.float32), "value": ((rows,), np.float32),
                  "logits": ((rows, 5), np.float32)}
        self.buf = {k: GuardedBuffer(s, d, DEV, name=k) for k, (s, d) in shapes.items()}
        self.zero_state()

    def set_params(self, flat):
        assert self.lib.mapf_policy_set_params(self.h_, _p(flat), flat.numel(), _stream()) == self.L.MAPF_OK

    def zero_state(self):
        for k in STATE:
            self.buf[k].poison()
            self.buf[k].payload_view().zero_()

    def poison_outputs(self):
        for k in OUTPUTS:
            self.buf[k].poison()

    def act(self, obs, pa=None, pr=None, sa=None, sb=None, mode=0, seed=0, outputs=("logp", "value", "logits"), rows=None,
            draws="draws"):
        b = self.buf
        return self.lib.mapf_policy_act(
            self.h_, self.rows if rows is None else rows, _p(obs), _p(pa), _p(pr), _p(sa), _p(sb), b["h"].ptr, b["c"].ptr,
            b[draws].ptr if draws else None, C.c_uint64(seed), mode, b["action"].ptr,
            *(b[k].ptr if k in outputs else None for k in ("logp", "value", "logits")), _stream())

    def close(self):
        self.lib.mapf_policy_destroy(self.h_)


def _step_inputs(c, t):
    flags = _dev(c["flags"][t], np.uint8)
    which = du.START_STEPS.get(t)
    return (_dev(c["obs"][t], np.float32), _dev(c["prev_action"][t], np.int8), _dev(c["prev_reward"][t], np.float32),
            flags if which == "a" else None, flags if which == "b" else None)


def _checked(pol, c, t, what):
    """The outputs and the state of a handle after step t, each checked as fully written between intact guards."""
    snap = {k: pol.buf[k].check(True, f"{what}, step {t}") for k in OUTPUTS}
    if c["recurrent"]:
        snap["h"], snap["c"] = pol.buf["h"].check(True, f"{what}, step {t}"), pol.buf["c"].check(True, f"{what}, step {t}")
    else:  # a feed-forward policy has no state to write (the buffers hold the zeros they were given)
        assert pol.buf["h"].guards_intact() and pol.buf["c"].guards_intact()
    if c["sample"]:
        snap["draws"] = pol.buf["draws"].check(True, f"{what}, step {t}")
    else:
        pol.buf["draws"].check(False, f"{what}, step {t}, greedy")
    return snap


@pytest.fixture(scope="module")
def runs():
    """case key -> the per-agent handle's snapshots of the six chained steps (computed once per case; read-only)."""
    return {}


def _run_case(c, runs):
    """Six chained steps on a per-agent handle; at every step each agent's net runs as a SHARED handle on the same full
    inputs and the same state, and its rows a::N must equal the per-agent handle's bit for bit."""
    key = (c["shape"], c["recurrent"], c["sample"])
    if key in runs:
        return runs[key]
    B, N, L, mask = c["shape"]
    rows = B * N
    mode = 1 if c["sample"] else 0
    pol = RawPolicy(c["module"], rows, N)
    shared = [RawPolicy(agent, rows, N) for agent in c["module"].agents]
    got = []
    for t in range(du.STEPS):
        inputs = _step_inputs(c, t)
        before = {k: pol.buf[k].payload_view().clone() for k in STATE}
        pol.poison_outputs()
        if not c["sample"]:
            pol.buf["draws"].poison()  # greedy mode neither reads nor writes draws
        assert pol.act(*inputs, mode=mode, seed=c["seed"]) == 0
        torch.cuda.synchronize()
        snap = _checked(pol, c, t, "per-agent")
        if c["sample"]:
            assert (snap["draws"] == t + 1).all()
        for a, sh in enumerate(shared):
            for k in STATE:
                sh.buf[k].poison()
                if c["sample"] or k != "draws":
                    sh.buf[k].payload_view().copy_(before[k])
            sh.poison_outputs()
            assert sh.act(*inputs, mode=mode, seed=c["seed"]) == 0
            torch.cuda.synchronize()
            want = _checked(sh, c, t, f"shared handle of agent {a}")
            for k, v in want.items():
                assert np.array_equal(_bits(snap[k][a::N]), _bits(v[a::N])), f"{k}, agent {a}, step {t}: not bit for bit"
        got.append(snap)
    for p in [pol] + shared:
        p.close()
    runs[key] = got
    return got


CASES = [(s, r, m) for s in du.SHAPES for r in (True, False) for m in (False, True)]
IDS = lambda v: str(v).replace(" ", "")  # noqa: E731


@pytest.mark.parametrize("shape,recurrent,sample", CASES, ids=IDS)
def test_rows_equal_the_shared_handle_of_their_agent_bit_for_bit(shape, recurrent, sample, runs):
    _run_case(du.case(shape, recurrent, sample), runs)


@pytest.mark.parametrize("shape,recurrent,sample", CASES, ids=IDS)
def test_parity_with_the_rule_on_each_rows_own_parameters(shape, recurrent, sample, runs):
    c = du.case(shape, recurrent, sample)
    got = _run_case(c, runs)
    dev = c["dev"]
    assert 0 < dev < 1e-5
    keys = ("logits", "value") + (("h", "c") if recurrent else ())
    worst = {k: 0.0 for k in keys + ("logp",)}
    for t, (g, e) in enumerate(zip(got, c["steps"])):
        for k in keys:
            assert np.isfinite(g[k]).all(), (k, t)
            worst[k] = max(worst[k], float(np.abs(g[k] - e[k]).max()))
        assert ((g["action"] >= 0) & (g["action"] <= 4)).all() and np.isfinite(g["logp"]).all()
        # against the rule's log-probability of the kernel's OWN action, so that no row is exempt
        worst["logp"] = max(worst["logp"], float(np.abs(g["logp"] - pu.logp_of(e["logits"], g["action"])).max()))
    print(f"per-agent policy parity {shape} recurrent={recurrent} sample={sample}: dev {dev:.3e}, kernel deviation "
          + ", ".join(f"{k} {v:.3e} ({v / dev:.2f} x dev)" for k, v in worst.items()))
    for k, v in worst.items():
        assert v <= (32 if k == "logp" else 16) * dev, (k, v, dev)


def test_identical_nets_equal_the_shared_handle_on_every_row():
    from dl_reference_models_amd.policy import PerAgentPolicy

    c = du.case((13, 5, 33, True), True, True)
    B, N, L, mask = c["shape"]
    one = pu.make_module(L, mask, True, seed=9)
    pol, sh = RawPolicy(PerAgentPolicy.from_shared(one, N), B * N, N), RawPolicy(one, B * N, N)
    for t in range(du.STEPS):
        inputs = _step_inputs(c, t)
        for p in (pol, sh):
            p.poison_outputs()
            assert p.act(*inputs, mode=1, seed=c["seed"]) == 0
        torch.cuda.synchronize()
        a, b = _checked(pol, c, t, "per-agent"), _checked(sh, c, t, "shared")
        for k in a:
            assert np.array_equal(_bits(a[k]), _bits(b[k])), (k, t)
    pol.close(), sh.close()


def _one(sample=True, set_params=True):
    c = du.case((13, 5, 33, True), True, sample)
    B, N, L, _ = c["shape"]
    return c, RawPolicy(c["module"], B * N, N, set_params=set_params), _step_inputs(c, 1)[:3]


def test_null_outputs_and_peek():
    c, pol, (obs, pa, pr) = _one()
    assert pol.act(_dev(c["obs"][0], np.float32), mode=1, seed=3) == 0  # a non-trivial state
    torch.cuda.synchronize()
    before = {k: pol.buf[k].array() for k in STATE}
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5) == 0
    torch.cuda.synchronize()
    full = {k: pol.buf[k].check(True, "peek") for k in OUTPUTS}
    for k in before:  # PEEK leaves h, c and draws untouched
        assert pol.buf[k].guards_intact() and np.array_equal(_bits(pol.buf[k].array()), _bits(before[k])), k
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5, outputs=()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pol.buf["action"].check(True, "action only"), full["action"])
    for k in ("logp", "value", "logits"):
        pol.buf[k].check(False, "pointer not passed")
    pol.close()


def test_second_set_params_takes_effect_without_a_synchronisation():
    c, pol, (obs, pa, pr) = _one(sample=False)
    B, N, L, mask = c["shape"]
    other = du.make_per_agent(N, L, mask, True, seed=5)
    flat2 = other.flat_params().to(DEV)
    first = GuardedBuffer((B * N, 5), np.float32, DEV, name="logits1")
    torch.cuda.synchronize()
    args = (B * N, _p(obs), _p(pa), _p(pr), None, None, pol.buf["h"].ptr, pol.buf["c"].ptr, None, C.c_uint64(0), 2)
    assert pol.lib.mapf_policy_act(pol.h_, *args, pol.buf["action"].ptr, None, None, first.ptr, _stream()) == 0
    pol.set_params(flat2)
    assert pol.lib.mapf_policy_act(pol.h_, *args, pol.buf["action"].ptr, None, None, pol.buf["logits"].ptr, _stream()) == 0
    torch.cuda.synchronize()
    e1 = du.forward64(c["module"], c["obs"][1], c["prev_action"][1], c["prev_reward"][1])[0]
    e2 = du.forward64(other, c["obs"][1], c["prev_action"][1], c["prev_reward"][1])[0]
    assert np.abs(e1 - e2).max() > 1e-2
    assert np.abs(first.check(True) - e1).max() <= 16 * c["dev"] and np.abs(pol.buf["logits"].check(True) - e2).max() <= 16 * c["dev"]
    pol.close()


def test_refused_arguments_launch_nothing():
    c, pol, (obs, pa, pr) = _one()
    _c, fresh, _ = _one(set_params=False)
    L, lib = pol.L, pol.lib
    for b in list(pol.buf.values()) + list(fresh.buf.values()):
        b.poison()
    torch.cuda.synchronize()
    CFG = L.MAPF_ERR_CONFIG
    assert pol.act(obs, rows=64) == CFG  # 64 rows are no whole number of 5-agent envs: refused without start flags too
    assert pol.act(obs, rows=4) == CFG
    assert pol.act(obs, rows=0) == CFG
    assert fresh.act(obs) == L.MAPF_ERR_STATE
    for count in (pol.flat.numel() - 1, pol.flat.numel() // pol.n, pol.flat.numel() + 1):  # one policy's vector is not enough
        assert lib.mapf_policy_set_params(pol.h_, _p(pol.flat), count, _stream()) == CFG
    for bad in (0, 65, -1):
        h = C.c_void_p(1)
        cfg = L.MapfPolicyConfig(33, 28, 1, bad, 64, 0)
        assert lib.mapf_policy_create_per_agent(C.byref(cfg), C.byref(h)) == CFG and not h.value, bad
    h = C.c_void_p()
    assert lib.mapf_policy_create_per_agent(C.byref(L.MapfPolicyConfig(33, 28, 1, 64, 64, 0)), C.byref(h)) == 0
    assert lib.mapf_policy_param_count(h) == 64 * lib.mapf_policy_param_count(pol.h_) // pol.n
    lib.mapf_policy_destroy(h)
    torch.cuda.synchronize()
    for b in list(pol.buf.values()) + list(fresh.buf.values()):
        b.check(False, "refused call")
    pol.zero_state()
    assert pol.act(obs, rows=60) == 0  # a whole number of envs is accepted
    torch.cuda.synchronize()
    assert pol.buf["h"].guards_intact() and pol.buf["logits"].guards_intact()
    pol.close(), fresh.close()


def test_graph_capture_from_the_very_first_act():
    c = du.case((13, 5, 33, True), True, True)
    B, N, L, _ = c["shape"]
    rows = B * N
    pol = RawPolicy(c["module"], rows, N)
    obs, pa, pr = _dev(c["obs"][0], np.float32), _dev(c["prev_action"][0], np.int8), _dev(c["prev_reward"][0], np.float32)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pol.act(obs, pa, pr, mode=1, seed=c["seed"]) == 0  # the handle's first act ever
    state = None
    for i in range(3):
        pol.poison_outputs()
        g.replay()
        torch.cuda.synchronize()
        logits, value, state = du.forward64(c["module"], c["obs"][0], c["prev_action"][0], c["prev_reward"][0], None, state)
        got = {k: pol.buf[k].check(True, f"replay {i}") for k in OUTPUTS + STATE}
        assert (got["draws"] == i + 1).all()
        assert np.abs(got["logits"] - logits).max() <= 16 * c["dev"] and np.abs(got["h"] - state[0]).max() <= 16 * c["dev"]
        action, _logp, gap = pu.choose(logits, pu.gumbel_np(c["seed"], np.arange(rows), np.full(rows, i)))
        decided = gap >= 32 * c["dev"]
        assert decided.mean() >= 0.99 and (got["action"][decided] == action[decided]).all()  # the noise of the GLOBAL row
    pol.close()


# ---- the learner -----------------------------------------------------------------------------------------------------------
def test_loss_and_gradient_of_n_nets_against_the_float64_recomputation():
    """B = 40 envs, N = 3, T = 5: 120 interleaved rows, 40 per group, one ragged 128-row workgroup per group.  The
    oracle shares no code with the learner: learner_util's chained ``forward`` calls and PPO objective on each agent's own
    net and slice of the fragment, in float64 on the CPU; dev is the same computation in fp32.  As in test_learner_gpu the
    loss terms take the forward quantities' dev and the parameter gradient, which comes out of GEMMs, GRAD_MARGIN."""
    from dl_reference_models_amd import learner as ln

    T, B, N, L = 5, 40, 3, 16
    frag = lu.synthetic_fragment(T, B, N, L, True, seed=8)
    frag64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}
    adv64, tgt64 = (torch.from_numpy(x) for x in lu.gae64(frag, 0.99, 0.95))
    adv64 = du.standardised_per_agent(adv64)
    module = du.make_per_agent(N, L, True, True).train()
    want = du.ppo_by_hand(copy.deepcopy(module).double(), frag64, adv64, tgt64)
    cpu32 = du.ppo_by_hand(copy.deepcopy(module), frag, adv64.float(), tgt64.float())
    dev = {k: float(np.abs(cpu32[k] - want[k]).max()) for k in ("forward", "gradient")}
    assert 0 < dev["forward"] < 1e-5 and 0 < dev["gradient"] < 1e-4
    frag_dev = {k: v.to(DEV) for k, v in frag.items()}
    adv_d, tgt_d = adv64.float().to(DEV), tgt64.float().to(DEV)
    f64 = lambda x: x.detach().double().cpu().numpy()  # noqa: E731
    for fused in (True, False):
        m = copy.deepcopy(module).to(DEV)
        learner = ln.PPOLearner(m, fused=fused)
        logits, value = ln.sequence_forward(m, frag_dev, fused=fused)
        assert logits.shape == (T, B, N, 5) and value.shape == (T, B, N)
        terms = learner.losses(frag_dev, adv_d, tgt_d)
        terms["total_loss"].backward()
        got = {"forward": np.concatenate([f64(logits).ravel(), f64(value).ravel()]),
               "loss": np.stack([f64(terms["per_policy"][k]) for k in lu.LOSS_TERMS], axis=1),
               "gradient": f64(torch.cat([p.grad.reshape(-1) for p in m.parameters()]))}
        err = {k: float(np.abs(got[k] - want[k]).max()) for k in got}
        total = abs(float(terms["total_loss"].detach()) - want["loss"][:, 0].sum())
        print(f"per-agent learner, fused={fused}: forward {err['forward']:.3e} / {dev['forward']:.3e}, loss terms {err['loss']:.3e}, "
              f"summed loss {total:.3e}, gradient {err['gradient']:.3e} / {dev['gradient']:.3e} = {err['gradient'] / dev['gradient']:.2f}")
        assert err["forward"] <= lu.FORWARD_MARGIN * dev["forward"], (fused, err, dev)
        assert err["loss"] <= lu.FORWARD_MARGIN * dev["forward"] and total <= N * lu.FORWARD_MARGIN * dev["forward"], (fused, err, total)
        assert err["gradient"] <= lu.GRAD_MARGIN * dev["gradient"], (fused, err, dev)


# ---- end to end ------------------------------------------------------------------------------------------------------------
def _env(B=6, N=3, spe=3, mask=True):
    from dl_reference_models_amd.vec_env import VecReferenceModel

    return VecReferenceModel({"grid": synth_grids(B, 8, 8, 0.15, N), "num_envs": B, "num_agents": N, "sensor_range": 1,
                              "steps_per_episode": spe, "seeds": list(range(B)), "include_action_mask_in_obs": mask, "device": DEV})


def test_rollout_needs_no_change_and_equals_the_python_loop():
    from dl_reference_models_amd.policy import DevicePolicy
    from dl_reference_models_amd.rollout import Rollout

    B, N, T = 6, 3, 4
    a, b = _env(B, N), _env(B, N)
    module = du.make_per_agent(N, a.obs_len, True, True, seed=2)
    pa_, pb_ = DevicePolicy(module, B * N, N, DEV), DevicePolicy(module, B * N, N, DEV)
    assert pa_.per_agent and not DevicePolicy(module.agents[0], B * N, N, DEV).per_agent
    with pytest.raises(ValueError, match="one policy for each of 3 agents"):
        DevicePolicy(module, B * 2, 2, DEV)
    ro = Rollout(a, pa_, T, sample=True, seed=11)
    obs = b.reset().clone()
    prev_a = torch.zeros((B, N), dtype=torch.int8, device=DEV)
    prev_r = torch.zeros((B, N), dtype=torch.float32, device=DEV)
    term = torch.ones((B,), dtype=torch.uint8, device=DEV)
    trunc = torch.zeros((B,), dtype=torch.uint8, device=DEV)
    for f in range(2):
        got = {k: v.clone() for k, v in ro.collect().items()}
        torch.cuda.synchronize()
        want = {k: [] for k in ("obs", "actions", "logp", "value", "rewards", "terminated", "truncated", "first")}
        want["h0"], want["c0"] = pb_.h.clone(), pb_.c.clone()
        for t in range(T):
            out = pb_.act(obs, prev_a, prev_r, start=(term, trunc), sample=True, seed=11)
            want["obs"].append(obs.clone())
            want["first"].append(term | trunc)
            want["actions"].append(out["action"].view(B, N).clone())
            want["logp"].append(out["logp"].view(B, N).clone())
            want["value"].append(out["value"].view(B, N).clone())
            prev_a = out["action"].view(B, N).clone()
            st = b.step(prev_a)
            obs, prev_r, term, trunc = st["obs"].clone(), st["rewards"].clone(), st["terminated"].clone(), st["truncated"].clone()
            want["rewards"].append(prev_r)
            want["terminated"].append(term)
            want["truncated"].append(trunc)
        want["last_value"] = pb_.act(obs, prev_a, prev_r, start=(term, trunc), sample=True, peek=True, seed=11)["value"].view(B, N).clone()
        for k, v in want.items():
            v = torch.stack(v) if isinstance(v, list) else v
            assert got[k].shape == v.shape and torch.equal(got[k].view(torch.uint8), v.contiguous().view(torch.uint8)), (f, k)
        assert got["terminated"].any() or got["truncated"].any()  # 3-step episodes end inside a 4-step fragment
    assert ro._graph is not None  # the second fragment was a replay
    a.poll_error()
    b.poll_error()


def test_trainer_changes_every_agents_own_parameters():
    from dl_reference_models_amd import learner as ln

    B, N = 6, 3
    env = _env(B, N)
    module = du.make_per_agent(N, env.obs_len, True, True, seed=3).train().to(DEV)
    before = [a.flat_params().clone() for a in module.agents]
    trainer = ln.Trainer(env, module, T=5, learner=ln.PPOLearner(module, epochs=2, minibatches=3, seed=1), sample_seed=5)
    assert trainer.policy.per_agent
    stats = [trainer.iterate() for _ in range(2)]  # the second fragment is a graph replay
    assert trainer.rollout._graph is not None and stats[1]["iteration"] == 2
    for s in stats:
        assert all(np.isfinite(s[k]) for k in ("reward_per_step",) + lu.LOSS_TERMS)
        assert all(len(s["per_policy"][k]) == N and np.isfinite(s["per_policy"][k]).all() for k in lu.LOSS_TERMS)
        assert abs(np.mean(s["per_policy"]["vf_loss"]) - s["vf_loss"]) <= 1e-5 * max(1.0, abs(s["vf_loss"]))
    after = [a.flat_params() for a in module.agents]
    for a in range(N):
        assert (after[a] - before[a]).abs().max() > 1e-4, a
        assert not torch.equal(after[a], after[(a + 1) % N]), a
    # the policy kernel holds the updated weights of every agent: a peek on a fixed observation against the rule
    rng = np.random.default_rng(0)
    L = env.obs_len
    obs = rng.integers(0, 2, size=(B * N, L)).astype(np.float32)
    obs[:, L - 5] = 1.0
    ones = torch.ones((B,), dtype=torch.uint8, device=DEV)
    out = trainer.policy.act(torch.from_numpy(obs).to(DEV), start=(ones, None), peek=True)
    torch.cuda.synchronize()
    host = copy.deepcopy(module).cpu().eval()
    want, want_v, _ = du.forward64(host, obs, None, None, np.ones(B * N, bool))
    with torch.no_grad():
        l32, v32, _ = host(torch.from_numpy(obs), start=torch.ones(B * N, dtype=torch.uint8))
    dev = max(float(np.abs(l32.numpy() - want).max()), float(np.abs(v32.numpy() - want_v).max()))
    assert 0 < dev < 1e-5 and np.abs(out["logits"].cpu().numpy() - want).max() <= 16 * dev
    assert np.abs(out["value"].cpu().numpy() - want_v).max() <= 16 * dev
    env.poll_error()


def test_evaluate_with_a_saved_per_agent_checkpoint_honours_first(tmp_path):
    from dl_reference_models_amd import evaluation as ev
    from dl_reference_models_amd.policy import DevicePolicy

    B, N, E = 6, 3, 2
    env0 = _env()
    module = du.make_per_agent(N, env0.obs_len, True, True, seed=4)
    path = tmp_path / "dte.pt"
    module.save(path)
    fn = ev.neural_policy(env0, str(path))
    assert fn.policy.per_agent
    res, heat = ev.evaluate(env0, fn, E)
    assert len(res["env"]) == B * E and int(heat.sum()) > 0

    def by_hand(clear):
        env = _env()
        pol = DevicePolicy(module, B * N, N, DEV)
        e = ev.Evaluator(env, E)
        obs = e.begin()
        first = torch.ones((B,), dtype=torch.uint8, device=DEV)
        none = torch.zeros_like(first)
        for t in range(e.max_steps):
            start = first if (clear or t == 0) else none
            act = pol.act(obs, pol.action, env._rewards, start=(start, None))["action"].view(B, N)
            obs, first = e.step(act)
        assert e.done()
        out = e.results()
        e.end()
        return out, pol.h.cpu().numpy()

    (same, h_same), (_other, h_other) = by_hand(True), by_hand(False)
    for k in ("timesteps", "total_reward", "agent_reward", "starts", "goals", "terminated"):
        assert np.array_equal(res[k], same[k]), k
    h = fn.policy.h.cpu().numpy()
    assert np.array_equal(h, h_same) and not np.array_equal(h, h_other)
    with pytest.raises(ValueError, match="one policy for each of 3 agents"):
        ev.neural_policy(_env(4, 2), str(path))


def _script(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_script_trains_in_dte_and_its_checkpoint_evaluates(tmp_path, capsys):
    train, evaluate = _script("train_multi_agent_env"), _script("evaluate_multi_agent_env")
    path = tmp_path / "ckpt" / "dte.pt"
    shape = ["--env-name", "ReferenceModel-2-1", "--num-agents", "4", "--sensor-range", "2", "--steps-per-episode", "12"]
    out = train.main(shape + ["--execution-mode", "DTE", "--num-envs", "16", "--iters", "2", "--T", "8", "--epochs", "2",
                              "--minibatches", "2", "--checkpoint", str(path)])
    lines = [ln_ for ln_ in capsys.readouterr().out.splitlines() if ln_.startswith("{")]
    assert len(lines) == len(out["history"]) == 2 and out["history"][1]["iteration"] == 2
    assert path.exists() and out["config"]["num_agents"] == 4 and len(out["history"][1]["per_policy"]["total_loss"]) == 4
    blob = torch.load(path, map_location="cpu", weights_only=True)
    assert blob["kind"] == "per_agent"
    res = evaluate.main(shape + ["--policy", "NEURAL", "--checkpoint", str(path), "--num-envs", "8", "--episodes", "1",
                                 "--output-dir", str(tmp_path / "eval")])
    assert len(res["table"]) == 8
