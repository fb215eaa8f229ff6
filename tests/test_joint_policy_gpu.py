"""The joint-action policy on the device (mapf_jpolicy_act through the raw C ABI, JointDevicePolicy, JointRollout) against
the float64 restatement of the rule (joint_policy_util), with every output and state buffer guarded and poisoned
(guard_util) and the observation between NaN guards.

Margins, from the issue of the feature: 16 x dev on logits / value / h / c, dev = the deviation of the module's fp32 CPU
forward from the restatement on the same case; 32 x dev_logp on logp against the restatement's log-probability of the
kernel's OWN actions, every row, dev_logp = the fp32 CPU module's deviation of that same sum.  Both are computed here, not
hard-coded.  DESIGN.md 4n holds the measured ratios."""

import ctypes as C

import numpy as np
import pytest
import torch

import joint_policy_util as ju
from guard_util import GuardedBuffer
from trace_util import synth_grids

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BYTE = 0xFF  # a guard of 0xFF bytes reads as NaN in float32
OUTPUTS = ("action", "logp", "value", "logits")


def _lib():
    from dl_reference_models_amd import _lib as L

    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(DEV)


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class RawJoint:
    """A joint policy handle through the raw C ABI, with guarded state (h, c, draws) and guarded outputs."""

    def __init__(self, module, rows, set_params=True):
        self.L, self.lib = _lib()
        self.rows, self.n, self.module = rows, module.num_agents, module
        self.h_ = C.c_void_p()
        cfg = self.L.MapfJPolicyConfig(module.grid_cells, module.num_agents, int(module.recurrent), 64, 0)
        assert self.lib.mapf_jpolicy_create(C.byref(cfg), C.byref(self.h_)) == self.L.MAPF_OK
        self.flat = module.flat_params().to(DEV)
        assert self.lib.mapf_jpolicy_param_count(self.h_) == self.flat.numel()
        if set_params:
            self.set_params(self.flat)
        n = self.n
        shapes = {"h": ((rows, 64), np.float32), "c": ((rows, 64), np.float32), "draws": ((rows,), np.uint32),
                  "action": ((rows, n), np.int8), "logp": ((rows,), np.float32), "value": ((rows,), np.float32),
                  "logits": ((rows, 5 * n), np.float32)}
        self.buf = {k: GuardedBuffer(s, d, DEV, name=k) for k, (s, d) in shapes.items()}
        self.zero_state()

    def set_params(self, flat):
        assert self.lib.mapf_jpolicy_set_params(self.h_, _p(flat), flat.numel(), _stream()) == self.L.MAPF_OK

    def zero_state(self):
        for k in ("h", "c", "draws"):
            self.buf[k].poison()
            self.buf[k].payload_view().zero_()

    def poison_outputs(self):
        for k in OUTPUTS:
            self.buf[k].poison()

    def act(self, obs, pa=None, pr=None, sa=None, sb=None, mode=0, seed=0, outputs=("logp", "value", "logits"), action=None,
            h="h", c="c", draws="draws", rows=None, handle=True):
        """obs / pa / pr / sa / sb: device tensors, raw pointers (c_void_p) or None.  Returns the return code."""
        def ptr(x):
            return x if isinstance(x, C.c_void_p) or x is None else _p(x)

        b = self.buf
        return self.lib.mapf_jpolicy_act(
            self.h_ if handle else None, self.rows if rows is None else rows, ptr(obs), ptr(pa), ptr(pr), ptr(sa), ptr(sb),
            b[h].ptr if h else None, b[c].ptr if c else None, b[draws].ptr if draws else None, C.c_uint64(seed), mode,
            b["action"].ptr if action is None else action, *(b[k].ptr if k in outputs else None for k in ("logp", "value", "logits")),
            _stream())

    def close(self):
        self.lib.mapf_jpolicy_destroy(self.h_)


def _run_case(c):
    """The six chained steps of a case on the device, the observation between NaN guards; returns per-step snapshots."""
    rows, H, W, N = c["shape"]
    L = H * W + 5 * N
    pol = RawJoint(c["module"], rows)
    mode = 1 if c["sample"] else 0
    obs_buf = GuardedBuffer((rows, L), np.float32, DEV, fill=NAN_BYTE, name="obs")
    got = []
    for t in range(ju.STEPS):
        obs_buf.payload_view().copy_(_dev(c["obs"][t], np.float32))
        flags = _dev(c["flags"][t], np.uint8)
        which = ju.START_STEPS.get(t)
        pa, pr = _dev(c["prev_action"][t], np.int8), _dev(c["prev_reward"][t], np.float64)
        pol.poison_outputs()
        if not c["sample"]:
            pol.buf["draws"].poison()  # greedy mode neither reads nor writes draws
        rc = pol.act(obs_buf.ptr, pa, pr, flags if which == "a" else None, flags if which == "b" else None, mode, c["seed"])
        assert rc == 0
        torch.cuda.synchronize()
        snap = {k: pol.buf[k].check(True, f"step {t}") for k in OUTPUTS}
        if c["recurrent"]:
            snap["h"], snap["c"] = pol.buf["h"].check(True, f"step {t}"), pol.buf["c"].check(True, f"step {t}")
        else:  # a feed-forward policy has no state to write (the buffers were zeroed, so look at the bytes)
            assert not pol.buf["h"].array().any() and not pol.buf["c"].array().any()
            assert pol.buf["h"].guards_intact() and pol.buf["c"].guards_intact()
        if c["sample"]:
            assert (pol.buf["draws"].check(True, f"step {t}") == t + 1).all()
        else:
            pol.buf["draws"].check(False, f"step {t}, greedy")
        got.append(snap)
    pol.close()
    return got


CASES = [(s, r, m) for s in ju.SHAPES for r in (True, False) for m in (False, True)]


@pytest.mark.parametrize("shape,recurrent,sample", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_parity_with_the_restatement(shape, recurrent, sample):
    c = ju.case(shape, recurrent, sample)
    got = _run_case(c)
    dev = c["dev"]
    assert 0 < dev < 1e-5
    keys = ("logits", "value") + (("h", "c") if recurrent else ())
    worst = {k: 0.0 for k in keys}
    und_dec, und_rows, worst_logp = [], [], 0.0
    for t, (g, e) in enumerate(zip(got, c["steps"])):
        for k in keys:
            assert np.isfinite(g[k]).all(), (k, t)
            worst[k] = max(worst[k], float(np.abs(g[k] - e[k]).max()))
        assert ((g["action"] >= 0) & (g["action"] <= 4)).all()
        assert np.isfinite(g["logp"]).all()
        # logp against the rule's log-probability of the kernel's own actions: no row is exempt
        worst_logp = max(worst_logp, float(np.abs(g["logp"] - ju.logp_of(e["logits"], g["action"])).max()))
        decided = e["gap"] >= ju.UNDECIDED_FACTOR * dev
        und_dec.append(~decided)
        und_rows.append((~decided).any(axis=1))
        assert (g["action"][decided] == e["action"][decided]).all(), f"step {t}"
    dlp = ju.dev_logp(c, [g["action"] for g in got])
    assert dlp > 0
    print(f"joint parity {shape} recurrent={recurrent} sample={sample}: dev {dev:.3e}, kernel deviation "
          + ", ".join(f"{k} {v:.3e} ({v / dev:.1f} x dev)" for k, v in worst.items())
          + f", logp {worst_logp:.3e} ({worst_logp / dlp:.1f} x dev_logp {dlp:.3e}), undecided decisions "
          f"{int(np.sum(und_dec))}/{np.size(und_dec)}, rows {int(np.sum(und_rows))}/{np.size(und_rows)}")
    for k, v in worst.items():
        assert v <= 16 * dev, (k, v, dev)
    assert worst_logp <= 32 * dlp, (worst_logp, dlp)
    assert np.mean(und_dec) <= ju.MAX_UNDECIDED_DECISIONS and np.mean(und_rows) <= ju.MAX_UNDECIDED_ROWS


ONE = (65, 16, 16, 4)


def _one(shape=ONE, recurrent=True, sample=True):
    c = ju.case(shape, recurrent, sample)
    return c, RawJoint(c["module"], shape[0]), _dev(c["obs"][1], np.float32), _dev(c["prev_action"][1], np.int8), \
        _dev(c["prev_reward"][1], np.float64)


def _prime(pol, c):
    """A non-trivial state: one sampled step from zeros."""
    assert pol.act(_dev(c["obs"][0], np.float32), mode=1, seed=3) == 0
    torch.cuda.synchronize()


def test_null_outputs_peek_and_repeatability():
    c, pol, obs, pa, pr = _one()
    _prime(pol, c)
    before = {k: pol.buf[k].array() for k in ("h", "c", "draws")}
    # PEEK: every output, no state and no draw counter
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5) == 0
    torch.cuda.synchronize()
    full = {k: pol.buf[k].check(True, "peek") for k in OUTPUTS}
    for k in before:
        assert pol.buf[k].guards_intact() and np.array_equal(pol.buf[k].array().view(np.uint8), before[k].view(np.uint8)), k
    # the same call again: bit-identical
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5) == 0
    torch.cuda.synchronize()
    for k, v in full.items():
        assert np.array_equal(pol.buf[k].check(True, "peek again").view(np.uint8), v.view(np.uint8)), k
    # the optional outputs NULL: the actions alone, and the same ones
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5, outputs=()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pol.buf["action"].check(True, "action only"), full["action"])
    for k in ("logp", "value", "logits"):
        pol.buf[k].check(False, "pointer not passed")
    # NULL prev_action / prev_reward mean zeros
    pol.poison_outputs()
    assert pol.act(obs, None, None, mode=2) == 0
    torch.cuda.synchronize()
    a = {k: pol.buf[k].check(True) for k in ("action", "logits", "value", "logp")}
    pol.poison_outputs()
    assert pol.act(obs, torch.zeros_like(pa), torch.zeros_like(pr), mode=2) == 0
    torch.cuda.synchronize()
    for k, v in a.items():
        assert np.array_equal(pol.buf[k].check(True), v), k
    pol.close()


def test_two_state_writing_runs_are_bitwise_equal():
    c, pol, obs, pa, pr = _one()
    _prime(pol, c)
    state = {k: pol.buf[k].payload_view().clone() for k in ("h", "c", "draws")}
    runs = []
    for _ in range(2):
        for k, v in state.items():
            pol.buf[k].payload_view().copy_(v)
        pol.poison_outputs()
        assert pol.act(obs, pa, pr, mode=1, seed=9) == 0
        torch.cuda.synchronize()
        runs.append({k: pol.buf[k].check(True) for k in OUTPUTS + ("h", "c", "draws")})
    for k in runs[0]:
        assert np.array_equal(runs[0][k].view(np.uint8), runs[1][k].view(np.uint8)), k
    pol.close()


# partial quarters in wave 3 and in wave 2 of the second staging buffer (joint_policy_util.SPLIT_SHAPES): one tile per wave
# and eight full tiles
SPLIT_PAIR = ((17, 14, 14, 25), (7, 20, 20, 51))


@pytest.mark.parametrize("shape", SPLIT_PAIR, ids=lambda v: str(v).replace(" ", ""))
def test_a_row_does_not_see_how_full_its_tile_is(shape):
    """Recurrent and sampled, from a non-trivial state: two runs are bitwise equal, and a call on rows - 1 rows gives the
    first rows - 1 rows the same bits in every output and in h, c and draws, and leaves the last row alone."""
    rows = shape[0]
    assert shape in ju.SPLIT_SHAPES and ju.upper_partial(shape)
    c, pol, obs, pa, pr = _one(shape)
    _prime(pol, c)
    state = {k: pol.buf[k].payload_view().clone() for k in ("h", "c", "draws")}
    runs = []
    for n in (rows, rows, rows - 1):
        for k, v in state.items():
            pol.buf[k].poison()
            pol.buf[k].payload_view().copy_(v)
        pol.poison_outputs()
        assert pol.act(obs, pa, pr, mode=1, seed=9, rows=n) == 0
        torch.cuda.synchronize()
        called = np.arange(rows) < n
        run = {k: pol.buf[k].check(called, f"{n} rows") for k in OUTPUTS}
        for k in ("h", "c", "draws"):
            assert pol.buf[k].guards_intact(), k
            run[k] = pol.buf[k].array()
        runs.append(run)
    full, again, less = runs
    for k in full:
        assert np.array_equal(full[k].view(np.uint8), again[k].view(np.uint8)), k
        assert np.array_equal(full[k][:rows - 1].view(np.uint8), less[k][:rows - 1].view(np.uint8)), k
    for k, v in state.items():  # the state of the row that was not called is the one it had, and the call moved the others
        assert np.array_equal(less[k][rows - 1:].view(np.uint8), v[rows - 1:].cpu().numpy().view(np.uint8)), k
        assert not np.array_equal(full[k][rows - 1:].view(np.uint8), v[rows - 1:].cpu().numpy().view(np.uint8)), k
    assert (full["draws"] == 2).all()
    pol.close()


def test_prev_action_may_alias_action():
    c, pol, obs, pa, pr = _one()
    _prime(pol, c)
    state = {k: pol.buf[k].payload_view().clone() for k in ("h", "c", "draws")}
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1, seed=9) == 0
    torch.cuda.synchronize()
    want = {k: pol.buf[k].check(True) for k in OUTPUTS + ("h", "c", "draws")}
    for k, v in state.items():
        pol.buf[k].payload_view().copy_(v)
    pol.poison_outputs()
    pol.buf["action"].payload_view().copy_(pa)
    assert pol.act(obs, pol.buf["action"].ptr, pr, mode=1, seed=9) == 0
    torch.cuda.synchronize()
    for k, v in want.items():
        assert np.array_equal(pol.buf[k].check(True, "aliased").view(np.uint8), v.view(np.uint8)), k
    pol.close()


def test_second_set_params_takes_effect_without_a_synchronisation():
    c, pol, obs, pa, pr = _one(sample=False)
    other = ju.make_module(ONE[1] * ONE[2], ONE[3], True, seed=5)
    flat2 = other.flat_params().to(DEV)
    out1 = {k: GuardedBuffer(pol.buf[k].shape, pol.buf[k].dtype, DEV, name=k + "1") for k in ("action", "logits")}
    torch.cuda.synchronize()
    lib = pol.lib
    args = (pol.rows, _p(obs), _p(pa), _p(pr), None, None, pol.buf["h"].ptr, pol.buf["c"].ptr, None, C.c_uint64(0), 2)
    assert lib.mapf_jpolicy_act(pol.h_, *args, out1["action"].ptr, None, None, out1["logits"].ptr, _stream()) == 0
    pol.set_params(flat2)
    assert lib.mapf_jpolicy_act(pol.h_, *args, pol.buf["action"].ptr, None, None, pol.buf["logits"].ptr, _stream()) == 0
    torch.cuda.synchronize()
    first, second = out1["logits"].check(True), pol.buf["logits"].check(True)
    p1, p2 = ju.params64(c["module"]), ju.params64(other)
    e1 = ju.forward64(p1, c["cfg"], c["obs"][1], c["prev_action"][1], c["prev_reward"][1])[0]
    e2 = ju.forward64(p2, c["cfg"], c["obs"][1], c["prev_action"][1], c["prev_reward"][1])[0]
    assert np.abs(e1 - e2).max() > 1e-2
    assert np.abs(first - e1).max() <= 16 * c["dev"] and np.abs(second - e2).max() <= 16 * c["dev"]
    pol.close()


def test_refused_arguments_launch_nothing():
    c, pol, obs, pa, pr = _one()
    L = pol.L
    fresh = RawJoint(c["module"], pol.rows, set_params=False)
    for b in list(pol.buf.values()) + list(fresh.buf.values()):
        b.poison()
    torch.cuda.synchronize()
    CFG, STATE = L.MAPF_ERR_CONFIG, L.MAPF_ERR_STATE
    assert pol.act(obs, handle=False) == CFG
    assert pol.act(None) == CFG
    assert pol.act(obs, action=C.c_void_p(None)) == CFG
    assert pol.act(obs, h=None) == CFG
    assert pol.act(obs, c=None) == CFG
    assert pol.act(obs, mode=1, draws=None) == CFG
    assert pol.act(obs, rows=0) == CFG
    assert pol.act(obs, rows=-5) == CFG
    assert pol.act(obs, mode=4) == CFG
    assert pol.act(obs, mode=-1) == CFG
    assert fresh.act(obs) == STATE
    assert fresh.act(obs, pa, pr, mode=1) == STATE
    assert pol.lib.mapf_jpolicy_set_params(pol.h_, _p(pol.flat), pol.flat.numel() - 1, _stream()) == CFG
    assert pol.lib.mapf_jpolicy_set_params(pol.h_, None, pol.flat.numel(), _stream()) == CFG
    assert pol.lib.mapf_jpolicy_set_params(None, _p(pol.flat), pol.flat.numel(), _stream()) == CFG
    for cells, agents, rec, hidden in ((0, 4, 1, 64), (4097, 4, 1, 64), (256, 0, 1, 64), (256, 65, 1, 64), (256, 4, 2, 64),
                                       (256, 4, 1, 32), (-1, 4, 1, 64)):
        h = C.c_void_p()
        cfg = L.MapfJPolicyConfig(cells, agents, rec, hidden, 0)
        assert pol.lib.mapf_jpolicy_create(C.byref(cfg), C.byref(h)) == CFG and not h.value, (cells, agents, rec, hidden)
    assert pol.lib.mapf_jpolicy_param_count(None) == 0
    torch.cuda.synchronize()
    for b in list(pol.buf.values()) + list(fresh.buf.values()):
        b.check(False, "refused call")
    # the existing policy entry point still refuses mode 4
    mp = C.c_void_p()
    mcfg = L.MapfPolicyConfig(33, 28, 1, 5, 64, 0)
    assert pol.lib.mapf_policy_create(C.byref(mcfg), C.byref(mp)) == 0
    assert pol.lib.mapf_policy_act(mp, 5, _p(obs), None, None, None, None, pol.buf["h"].ptr, pol.buf["c"].ptr, None, C.c_uint64(0), 4,
                                   pol.buf["action"].ptr, None, None, None, _stream()) == CFG
    pol.lib.mapf_policy_destroy(mp)
    # a greedy feed-forward call needs no state at all; the far ends of the configuration are accepted
    ff = RawJoint(ju.make_module(ONE[1] * ONE[2], ONE[3], False), pol.rows)
    assert ff.act(obs, h=None, c=None, draws=None) == 0
    torch.cuda.synchronize()
    ff.buf["logits"].check(True)
    for p in (pol, fresh, ff):
        p.close()


def test_graph_capture_from_the_very_first_act():
    c = ju.case(ONE, True, True)
    rows, N = ONE[0], ONE[3]
    pol = RawJoint(c["module"], rows)
    obs, pa, pr = _dev(c["obs"][0], np.float32), _dev(c["prev_action"][0], np.int8), _dev(c["prev_reward"][0], np.float64)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pol.act(obs, pa, pr, mode=1, seed=c["seed"]) == 0  # the handle's first act ever
    p = ju.params64(c["module"])
    state = None
    for i in range(3):
        pol.poison_outputs()
        g.replay()
        torch.cuda.synchronize()
        logits, value, state = ju.forward64(p, c["cfg"], c["obs"][0], c["prev_action"][0], c["prev_reward"][0], None, state)
        action, logp, gap = ju.choose(logits, ju.gumbel_np(c["seed"], np.arange(rows), np.full(rows, i), N))
        got = {k: pol.buf[k].check(True, f"replay {i}") for k in OUTPUTS + ("h", "c", "draws")}
        assert (got["draws"] == i + 1).all()
        assert np.abs(got["logits"] - logits).max() <= 16 * c["dev"] and np.abs(got["h"] - state[0]).max() <= 16 * c["dev"]
        decided = gap >= 32 * c["dev"]
        assert decided.mean() >= 0.99 and (got["action"][decided] == action[decided]).all()
    pol.close()


# ---- JointDevicePolicy, JointRollout -----------------------------------------------------------------------------------
def _env(B=6, N=3, spe=3):
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    return VecSingleAgentReferenceModel({"grid": synth_grids(B, 8, 8, 0.15, N), "num_envs": B, "num_agents": N,
                                         "steps_per_episode": spe, "seeds": list(range(B)), "device": DEV})


def test_rollout_equals_the_python_loop():
    from dl_reference_models_amd.policy import JointDevicePolicy
    from dl_reference_models_amd.rollout import JointRollout

    B, N, T = 6, 3, 5
    a, b = _env(B, N), _env(B, N)
    assert a.obs_len == 64 + 5 * N
    module = ju.make_module(64, N, True, seed=2)
    pa_, pb_ = JointDevicePolicy(module, B, DEV), JointDevicePolicy(module, B, DEV)
    ro = JointRollout(a, pa_, T, sample=True, seed=11)
    # the same loop by hand on the second env and policy
    obs = b.reset().clone()
    prev_a = torch.zeros((B, N), dtype=torch.int8, device=DEV)
    prev_r = torch.zeros((B,), dtype=torch.float64, device=DEV)
    term = torch.ones((B,), dtype=torch.uint8, device=DEV)
    trunc = torch.zeros((B,), dtype=torch.uint8, device=DEV)
    frags = []
    for f in range(2):
        got = {k: v.clone() for k, v in ro.collect().items()}
        torch.cuda.synchronize()
        want = {k: [] for k in ("obs", "actions", "logp", "value", "rewards", "prev_rewards", "terminated", "truncated", "first")}
        want["h0"], want["c0"], want["prev_action0"] = pb_.h.clone(), pb_.c.clone(), prev_a.clone()
        for t in range(T):
            out = pb_.act(obs, prev_a, prev_r, start=(term, trunc), sample=True, seed=11)
            want["obs"].append(obs.clone())
            want["first"].append(term | trunc)
            want["prev_rewards"].append(prev_r.clone())
            want["actions"].append(out["action"].clone())
            want["logp"].append(out["logp"].clone())
            want["value"].append(out["value"].clone())
            prev_a = out["action"].clone()
            st = b.step(prev_a)
            obs, prev_r, term, trunc = st["obs"].clone(), st["reward"].clone(), st["terminated"].clone(), st["truncated"].clone()
            want["rewards"].append(prev_r)
            want["terminated"].append(term)
            want["truncated"].append(trunc)
        want["last_value"] = pb_.act(obs, prev_a, prev_r, start=(term, trunc), sample=True, peek=True, seed=11)["value"].clone()
        for k, v in want.items():
            v = torch.stack(v) if isinstance(v, list) else v
            assert got[k].shape == v.shape and got[k].dtype == v.dtype, (f, k, got[k].shape, v.shape)
            assert torch.equal(got[k].contiguous().view(torch.uint8), v.contiguous().view(torch.uint8)), (f, k)
        assert got["obs"].shape == (T, B, 64 + 5 * N) and got["actions"].shape == (T, B, N) and got["logp"].shape == (T, B)
        assert got["rewards"].dtype == torch.float64 and got["last_value"].shape == (B,)
        assert got["first"][0].all() if f == 0 else True
        assert torch.equal(got["first"][1:], got["terminated"][:-1] | got["truncated"][:-1])
        assert got["terminated"].any() or got["truncated"].any()  # 3-step episodes end inside a 5-step fragment
        frags.append(got)
    assert ro._graph is not None  # the second fragment was a replay
    assert torch.equal(frags[0]["last_value"], frags[1]["value"][0])
    assert torch.equal(frags[1]["first"][0], frags[0]["terminated"][-1] | frags[0]["truncated"][-1])
    assert torch.equal(frags[1]["prev_action0"], frags[0]["actions"][-1])
    a.poll_error()
    b.poll_error()


def test_rollout_refuses_the_other_env_and_policy():
    from dl_reference_models_amd.policy import JointDevicePolicy
    from dl_reference_models_amd.rollout import JointRollout, Rollout

    env = _env()
    pol = JointDevicePolicy(ju.make_module(64, 3, True), 6, DEV)
    with pytest.raises(TypeError, match="VecReferenceModel"):
        Rollout(env, pol, 4)
    with pytest.raises(TypeError, match="VecSingleAgentReferenceModel"):
        JointRollout(object(), pol, 4)
    with pytest.raises(ValueError, match="rows"):
        JointRollout(env, JointDevicePolicy(ju.make_module(64, 3, True), 7, DEV), 4)
