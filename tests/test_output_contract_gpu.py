"""WHERE every device-writing entry point of the C ABI stores (include/mapf_step.h), on every kernel family mapf_create can
pick: each output lives in a guarded, poisoned arena (tests/guard_util.py).  After every call the guards must be intact, no
element the contract says is written may still be poison, every element it says is left alone must still be poison -- and
the values are, bit for bit, those of the CPU oracle / the NumPy restatements.  The cases are the smallest shapes at which
the kernel families still differ (guard_util.CASES; tests/test_guard_util_host.py proves on the oracle alone that every
one of them has episode ends in the middle of a batch).  Run with `pytest -m gpu` on an MI355X.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

import eval_util as eu
import guard_util as gu
import render_util as ru
from guard_util import CASE_BY_ID, GuardedBuffer, case_inputs, case_params, device_bytes, guard_bytes_for, make_engine, make_oracle
from trace_util import _eq, compare_steppers

pytestmark = pytest.mark.gpu

ALL = case_params()
MA = case_params(gu.MA_CASES)
LARGEST = [(c["id"], gu.case_batches(c)[-1]) for c in gu.CASES]  # B = 3G - 1: two full waves and a ragged one
ERR_BAD_ACTION, ERR_CONFIG = -1, -4


def _sync(env):
    import torch

    torch.cuda.synchronize(env.device)


def _assert_path(case, env):
    """The kernel the case is in the table for is the one mapf_create picked."""
    li = env.launch_info()
    if case["expect"][3] and not li["jit"]:
        pytest.skip(f"no run-time specialisation here: {li['jit_note']}")
    got = (li["specialized_kernel"], li["lanes_per_env"], li["threads"], li["jit"])
    assert got == case["expect"], (case["id"], got, li)
    if case["kind"] == "cte":
        assert env.launch_info(fused=True)["lanes_per_env"] == case["many_lanes"], env.launch_info(fused=True)


def _outputs(case):
    return gu.MA_OUTPUTS if case["kind"] == "ma" else gu.CTE_OUTPUTS


def _started(case, inp, steps=0, **kw):
    """(engine, oracle) after reset, with the staggered step counters set and `steps` steps of the action stream made."""
    eng, orc = make_engine(case, inp, **kw), make_oracle(case, inp)
    _assert_path(case, eng.env)
    _eq("reset obs", eng.reset(), orc.reset())
    eng.set_step_counts(inp["step_counts"])
    orc.set_step_counts(inp["step_counts"])
    for t in range(steps):
        eng.step(inp["actions"][t])
        orc.step(inp["actions"][t])
    return eng, orc


def _oracle_step_subset(case, orc, actions, mask, auto_reset):
    """The step of the envs with mask != 0 alone, each through its own oracle handle: expected rows of every output (rows of
    other envs are zero and mean nothing) and ``done``."""
    B = orc.B
    exp = {k: np.zeros(shape, dt) for k, (shape, dt) in
           (gu.ma_output_specs(B, orc.N, orc.L) if case["kind"] == "ma" else gu.cte_output_specs(B, orc.L)).items()}
    done = np.zeros(B, bool)
    envs = orc.batch.envs if case["kind"] == "ma" else orc.envs
    for b in np.flatnonzero(mask):
        e = envs[b]
        if case["kind"] == "ma":
            rc, obs, rew, term, trunc, info_all, info_agent = e.step(actions[b])
            exp["rewards"][b], exp["info_all"][b], exp["info_agent"][b] = rew, info_all, info_agent
        else:
            rc, obs, rew, term, trunc, info = e.step(actions[b])
            exp["reward"][b], exp["info"][b] = rew, info
        assert rc == 0, (rc, b)
        exp["terminated"][b], exp["truncated"][b] = term, trunc
        done[b] = term or trunc
        if done[b] and auto_reset:
            exp["final_obs"][b] = obs
            obs = e.reset()
            obs = obs[1] if case["kind"] == "ma" else obs
        exp["obs"][b] = obs
    return exp, done


def _oracle_reset_subset(case, orc, mask):
    envs = orc.batch.envs if case["kind"] == "ma" else orc.envs
    out = {}
    for b in np.flatnonzero(mask):
        r = envs[b].reset()
        out[b] = r[1] if case["kind"] == "ma" else r
    return out


def _check_rows(eng, names, rows, exp, what):
    """Guards intact; rows `rows` of every output in `names` written and equal to exp, every other row still poison."""
    for k in names:
        got = eng.buf[k].check(rows, what)
        _eq(f"{k} ({what})", got[rows], exp[k][rows])


# ---- mapf_reset / mapf_step / mapf_bind_outputs + mapf_step_bound and their single-agent counterparts ----------------------
@pytest.mark.parametrize("cid,B", ALL)
def test_step_and_reset_write_every_row_and_nothing_else(cid, B):
    """40 steps against the oracle with auto_reset = 1 and final_obs passed: obs, rewards, flags and infos fully written
    every step; final_obs written for exactly the envs that finished (every kernel family leaves the other rows alone);
    then every single output alone with all other pointers NULL, the bound call and the masked entry point with an all-one
    mask against that run."""
    case = CASE_BY_ID[cid]
    inp = case_inputs(case, B)
    eng, orc = make_engine(case, inp), make_oracle(case, inp)
    _assert_path(case, eng.env)
    outs = _outputs(case)
    if case["kind"] == "ma":
        stats = compare_steppers(eng, orc, inp["actions"], step_counts=inp["step_counts"])
        assert stats["episodes"] >= 2 * B
    else:
        _eq("reset obs", eng.reset(), orc.reset())
        eng.set_step_counts(inp["step_counts"])
        orc.set_step_counts(inp["step_counts"])
        for t, a in enumerate(inp["actions"]):
            ra, rb = eng.step(a), orc.step(a)
            for k in outs:
                _eq(k, ra[k], rb[k], t)
            done = (ra["terminated"] | ra["truncated"]).astype(bool)
            _eq("final_obs", ra["final_obs"][done], rb["final_obs"][done], t)
        _eq("final rng state", eng.rng_words(), orc.rng_words())
    eng.env.poll_error()
    ref = eng.history
    variants = [{"only": (k,)} for k in outs] + [{"call": "masked"}] + ([{"call": "bound"}] if case["kind"] == "ma" else [])
    for kw in variants:
        e2 = make_engine(case, inp, **kw)
        _eq("reset obs", e2.reset(), eng.reset_obs0)
        e2.set_step_counts(inp["step_counts"])
        for t in range(10):
            out = e2.step(inp["actions"][t])
            for k in outs:
                if out[k] is not None:
                    _eq(f"{k} {kw}", out[k], ref[t][k], t)
        e2.env.poll_error()


@pytest.mark.parametrize("cid,B", ALL)
def test_step_without_auto_reset_and_masked_reset(cid, B):
    """auto_reset = 0: the six outputs fully written, final_obs -- passed all the same -- not touched at all.  Finished envs
    are then reset through mapf_reset with a mask: rows of the selected envs written, all others still poison; every other
    time with obs = NULL (state only)."""
    case = CASE_BY_ID[cid]
    inp = case_inputs(case, B)
    eng, orc = _started(case, inp)
    outs = _outputs(case)
    resets = 0
    for t in range(20):
        a = inp["actions"][t]
        got = eng.step(a, auto_reset=False)  # (asserts final_obs untouched)
        exp, done = _oracle_step_subset(case, orc, a, np.ones(B, bool), auto_reset=False)
        for k in outs:
            _eq(k, got[k], exp[k], t)
        if done.any():
            want = _oracle_reset_subset(case, orc, done)
            with_obs = resets % 2 == 0
            obs = eng.reset_masked(done.astype(np.uint8), with_obs=with_obs)
            if with_obs:
                for b, o in want.items():
                    _eq(f"masked reset obs of env {b}", obs[b], o, t)
            resets += 1
        _eq("positions", eng.positions(), orc.positions(), t)
        _eq("goals", eng.goals(), orc.goals(), t)
    assert resets >= 2
    _eq("rng", eng.rng_words(), orc.rng_words())
    eng.env.poll_error()


# ---- mapf_step_masked / mapf_cte_step_masked ------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,B", ALL)
def test_masked_step_leaves_rows_and_state_of_other_envs_alone(cid, B):
    case = CASE_BY_ID[cid]
    inp = case_inputs(case, B)
    eng, orc = _started(case, inp, steps=2)
    outs = _outputs(case)
    rng = np.random.default_rng(7)
    masks = [rng.random(B) < 0.5, np.zeros(B, bool), np.ones(B, bool)] + [rng.random(B) < 0.75 for _ in range(12)]
    ends = 0
    for i, mask in enumerate(masks):
        a = inp["actions"][2 + i]
        ar = i % 2 == 0
        st0 = eng.env.get_state()
        m = device_bytes(eng.env, mask, np.uint8)
        eng.launch(a, auto_reset=ar, mask_ptr=C.c_void_p(m.data_ptr()))
        exp, done = _oracle_step_subset(case, orc, a, mask, auto_reset=ar)
        what = f"masked step {i}, auto_reset={int(ar)}"
        _check_rows(eng, outs, mask, exp, what)
        _check_rows(eng, ("final_obs",), done & ar, exp, what)
        st1 = eng.env.get_state()
        for k in st0:
            _eq(f"state {k} of masked-off envs ({what})", st1[k][~mask], st0[k][~mask])
        if not ar and done.any():  # the next-step autoreset of the vector protocol: reset with the complementary rows idle
            want = _oracle_reset_subset(case, orc, done)
            obs = eng.reset_masked(done.astype(np.uint8))
            for b, o in want.items():
                _eq(f"reset obs of env {b}", obs[b], o)
        ends += int(done.sum())
        _eq("positions", eng.positions(), orc.positions(), i)
    assert ends >= 1
    _eq("rng", eng.rng_words(), orc.rng_words())
    eng.env.poll_error()


# ---- a latched invalid action -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,B", LARGEST)
def test_invalid_action_rows_of_the_failed_env_are_not_written(cid, B):
    """Action 7 for one agent of one env: every other env's rows are exact, the record names env, agent and value, and
    -- every kernel family alike -- NO row of the failed env is stored in any output (the reference raises there)."""
    case = CASE_BY_ID[cid]
    inp = case_inputs(case, B)
    eng, orc = _started(case, inp, steps=3)
    outs = _outputs(case)
    e, j = B // 2, case["N"] // 2
    for ar in (True, False):
        a = inp["actions"][3 + int(ar)].copy()
        a[e, j] = 7
        ok = np.arange(B) != e
        eng.launch(a, auto_reset=ar)
        exp, done = _oracle_step_subset(case, orc, a, ok, auto_reset=ar)
        what = f"step with an invalid action in env {e}, auto_reset={int(ar)}"
        _check_rows(eng, outs, ok, exp, what)
        _check_rows(eng, ("final_obs",), done & ar & ok, exp, what)
        rc, env_i, agent, value = eng.env._poll()
        assert (rc, env_i, value) == (ERR_BAD_ACTION, e, 7), (rc, env_i, agent, value)
        if case["kind"] == "ma":
            assert agent == j
        assert eng.env._poll()[0] == 0  # (cleared)
        if not ar and (done & ok).any():
            _oracle_reset_subset(case, orc, done & ok)
            eng.reset_masked((done & ok).astype(np.uint8))
        _eq("positions of the other envs", eng.positions()[ok], orc.positions()[ok])


# ---- fused launches -----------------------------------------------------------------------------------------------------------
def _many(case, eng, T, actions, obs_buf, mode, bufs):
    env = eng.env
    a = device_bytes(env, actions, np.int8)
    for b in list(bufs.values()) + [obs_buf]:
        b.poison()
    if case["kind"] == "ma":
        rc = env._lib.mapf_step_many(env._h, T, C.c_void_p(a.data_ptr()), obs_buf.ptr, mode, bufs["rewards"].ptr,
                                     bufs["terminated"].ptr, bufs["truncated"].ptr, bufs["info_all"].ptr, bufs["info_agent"].ptr,
                                     env._stream())
    else:
        rc = env._lib.mapf_cte_step_many(env._h, T, C.c_void_p(a.data_ptr()), obs_buf.ptr, mode, bufs["reward"].ptr,
                                         bufs["terminated"].ptr, bufs["truncated"].ptr, bufs["info"].ptr, env._stream())
    env._check(rc)
    _sync(env)


@pytest.mark.parametrize("cid,B", ALL)
def test_fused_steps_write_exactly_their_slabs(cid, B):
    """mapf_step_many / mapf_cte_step_many, T in {1, 2, 7}: the per-step outputs are T slabs, each what T single steps give;
    obs_mode 0 writes not one byte of a non-NULL obs, mode 1 exactly one slab (the guard behind it is as large as a slab: a
    mode-2 layout would land there), mode 2 all T.  Then mapf_observe and the device-side episode sums."""
    case = CASE_BY_ID[cid]
    inp = case_inputs(case, B)
    eng, orc = _started(case, inp)
    env = eng.env
    outs = [k for k in _outputs(case) if k != "obs"]
    specs = {k: v for k, v in eng.specs.items() if k in outs}
    obs_shape, slab = eng.specs["obs"][0], int(np.prod(eng.specs["obs"][0])) * 4
    t0 = 0
    steps = inp["actions"].shape[0]
    for T in (1, 2, 7):
        bufs = gu.guarded_outputs(specs, env.device, lead=(T,))
        for mode in (0, 1, 2):
            if t0 + T > steps:
                break
            acts = inp["actions"][t0:t0 + T]
            t0 += T
            obs_buf = GuardedBuffer(((T,) if mode == 2 else ()) + obs_shape, np.float32, env.device, guard_bytes_for(slab), name="obs")
            _many(case, eng, T, acts, obs_buf, mode, bufs)
            want = [orc.step(a) for a in acts]
            what = f"fused T={T} obs_mode={mode}"
            for k in outs:
                _eq(f"{k} ({what})", bufs[k].check(True, what), np.stack([w[k] for w in want]))
            obs = obs_buf.check(mode != 0, what)
            if mode == 1:
                _eq(f"obs ({what})", obs, want[-1]["obs"])
            if mode == 2:
                _eq(f"obs ({what})", obs, np.stack([w["obs"] for w in want]))
            _eq(f"positions ({what})", eng.positions(), orc.positions())
    _eq("rng", eng.rng_words(), orc.rng_words())
    env.poll_error()
    # mapf_episode_stats_async: exactly 12 int64 values, those of mapf_get_episode_stats (into a guarded host array)
    dev = GuardedBuffer((12,), np.int64, env.device, name="episode_stats_async")
    env._check(env._lib.mapf_episode_stats_async(env._h, dev.ptr, env._stream()))
    _sync(env)
    host = GuardedBuffer((12,), np.int64, "numpy", name="get_episode_stats")
    env._check(env._lib.mapf_get_episode_stats(env._h, host.ptr, 0))
    _eq("episode sums", dev.check(True), host.check(True))
    assert host.array()[0] >= 1
    if case["kind"] == "ma":  # mapf_observe: [B][N][L] fully written, nothing modified
        st0 = env.get_state()
        ob = GuardedBuffer(obs_shape, np.float32, env.device, guard_bytes_for(slab), name="observe")
        env._check(env._lib.mapf_observe(env._h, ob.ptr, env._stream()))
        _sync(env)
        _eq("observe", ob.check(True, "mapf_observe"), env.observe().cpu().numpy())
        st1 = env.get_state()
        for k in st0:
            _eq(f"state {k} after mapf_observe", st1[k], st0[k])


@pytest.mark.parametrize("cid,B", [(c, B) for c, B in MA if CASE_BY_ID[c]["cfg"].get("include_action_mask_in_obs")])
def test_sampled_fused_steps_write_everything_and_replay(cid, B):
    """mapf_step_many_sampled: actions_out, obs [T] and the per-step outputs fully written; the observation right after a
    reset equals mapf_observe's; replaying actions_out through guarded single steps (and the oracle) gives the same."""
    case = CASE_BY_ID[cid]
    inp = case_inputs(case, B)
    eng, orc = _started(case, inp)
    env = eng.env
    T = 5
    ob = GuardedBuffer(eng.specs["obs"][0], np.float32, env.device, name="observe")
    env._check(env._lib.mapf_observe(env._h, ob.ptr, env._stream()))
    _sync(env)
    _eq("observe after reset", ob.check(True, "mapf_observe"), eng.reset_obs0)
    bufs = gu.guarded_outputs({k: v for k, v in eng.specs.items() if k != "final_obs"}, env.device, lead=(T,))
    bufs["actions_out"] = GuardedBuffer((T, B, case["N"]), np.int8, env.device, guard_bytes_for(B * case["N"]), name="actions_out")
    for b in bufs.values():
        b.poison()
    env._check(env._lib.mapf_step_many_sampled(
        env._h, T, ob.ptr, C.c_uint64(0x1234_5678_9ABC), bufs["actions_out"].ptr, bufs["obs"].ptr, bufs["rewards"].ptr,
        bufs["terminated"].ptr, bufs["truncated"].ptr, bufs["info_all"].ptr, bufs["info_agent"].ptr, env._stream()))
    _sync(env)
    got = {k: b.check(True, "mapf_step_many_sampled") for k, b in bufs.items()}
    assert got["actions_out"].min() >= 0 and got["actions_out"].max() <= 4
    e2, _ = _started(case, inp)
    for t in range(T):
        ra, rb = e2.step(got["actions_out"][t]), orc.step(got["actions_out"][t])
        for k in gu.MA_OUTPUTS:
            _eq(f"{k} of the replay", ra[k], got[k][t], t)
            _eq(f"{k} of the oracle", rb[k], got[k][t], t)
    _eq("positions", eng.positions(), e2.positions())
    _eq("rng", eng.rng_words(), orc.rng_words())
    env.poll_error()


# ---- mapf_render -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c3_three_wave", "wide_n33_finite", "cte_n4_6x7_lanes16"])
@pytest.mark.parametrize("cell_px", [4, 5])
def test_render_writes_exactly_k_frames(cid, cell_px):
    case = CASE_BY_ID[cid]
    B = gu.case_batches(case)[-1]
    inp = case_inputs(case, B)
    eng, _ = _started(case, inp, steps=3)
    env = eng.env
    H, W = case["H"], case["W"]
    st = env.get_state()
    sr = case["cfg"]["sensor_range"] if case["kind"] == "ma" else None
    dup = np.array(([B - 1, 0, B - 1] + list(range(B - 1, -1, -1)))[:B], np.int32)  # duplicates, reversed order
    frame_bytes = H * W * cell_px * cell_px * 3

    def render(ids, K, what):
        d = None if ids is None else device_bytes(env, ids, np.int32)
        frames = GuardedBuffer((K, H * cell_px, W * cell_px, 3), np.uint8, env.device, guard_bytes_for(frame_bytes), name="frames")

        def call():
            env._check(env._lib.mapf_render(env._h, None if d is None else C.c_void_p(d.data_ptr()), K, cell_px, frames.ptr,
                                            env._stream()))
            _sync(env)

        return gu.two_fill(frames, call, what)

    for ids, K in ((None, 1), (None, B), (np.array([B // 2], np.int32), 1), (dup, B)):
        got = render(ids, K, f"K={K} ids {None if ids is None else ids.tolist()}")
        _eq("frames", got, ru.render_envs(inp["grids"], st["positions"], st["goals"], range(K) if ids is None else ids, cell_px, sr))
    assert env._poll()[0] == 0
    # one id outside [0, B): an all-zero frame and the latched record (env = k, value = the id)
    got = render(np.array([0, B + 3, B - 1], np.int32), 3, "one id out of range")
    assert not got[1].any()
    _eq("frames", got[[0, 2]], ru.render_envs(inp["grids"], st["positions"], st["goals"], [0, B - 1], cell_px, sr))
    rc, k, _agent, value = env._poll()
    assert (rc, k, value) == (ERR_CONFIG, 1, B + 3)
    st1 = env.get_state()
    for key in st:
        _eq(f"state {key} after mapf_render", st1[key], st[key])


# ---- mapf_eval_begin / mapf_eval_record ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["c3_three_wave", "train16_bit_rows", "c5_stepw_lifelong"])
def test_eval_record_writes_only_the_records_it_books(cid):
    """E = 2 with all seven buffers guarded and never cleared: after every record they equal the NumPy recorder, record
    slots k >= episodes_recorded[b] are still poison (the header: the records need no clearing) and an env with
    active == 0 gets nothing written (its rows stay what the recorder says while the others move on)."""
    case = CASE_BY_ID[cid]
    B = gu.case_batches(case)[-1]
    inp = case_inputs(case, B)
    eng, orc = make_engine(case, inp), make_oracle(case, inp)
    _assert_path(case, eng.env)
    env, N, H, W, E = eng.env, case["N"], case["H"], case["W"], 2
    shapes = {"heat": ((B, H, W), np.uint32), "ep_i32": ((B, E, 2 + 4 * N), np.int32), "ep_f64": ((B, E, 1 + N), np.float64),
              "ep_info": ((B, E, 14), np.float32), "episodes_recorded": ((B,), np.int32), "active": ((B,), np.uint8),
              "reset_mask": ((B,), np.uint8)}
    g = {k: GuardedBuffer(s, dt, env.device, guard_bytes_for(int(np.prod(s)) * np.dtype(dt).itemsize), name=k)
         for k, (s, dt) in shapes.items()}
    rec = eu.HostRecorder(B, N, H, W, E)

    def check(what):
        booked = np.arange(E)[None, :] < rec.episodes_recorded[:, None]
        for k in ("heat", "episodes_recorded", "active", "reset_mask"):
            _eq(f"{k} ({what})", g[k].check(True, what), getattr(rec, k))
        for k in ("ep_i32", "ep_f64", "ep_info"):
            got = g[k].check(booked, what)
            _eq(f"{k} ({what})", got[booked], getattr(rec, k)[booked])

    env._check(env._lib.mapf_eval_begin(env._h, E, *(g[k].ptr for k in shapes), env._stream()), ValueError)
    _sync(env)
    check("mapf_eval_begin")
    _eq("reset obs", eng.reset(), orc.reset())
    envs = orc.batch.envs
    t = 0
    while rec.active.any():
        a = inp["actions"][t % inp["actions"].shape[0]]
        active = rec.active.astype(bool)
        eng.launch(a, auto_reset=False, mask_ptr=g["active"].ptr, sync=False)
        b_ = eng.buf
        env._check(env._lib.mapf_eval_record(env._h, b_["rewards"].ptr, b_["terminated"].ptr, b_["truncated"].ptr,
                                             b_["info_all"].ptr, env._stream()))
        _sync(env)
        exp, done = _oracle_step_subset(case, orc, a, active, auto_reset=False)
        _check_rows(eng, gu.MA_OUTPUTS, active, exp, f"evaluation step {t}")
        for b in np.flatnonzero(active):
            e = envs[b]
            rec.record(b, e.positions, e.starts, e.goals, exp["rewards"][b], bool(exp["terminated"][b]), bool(exp["truncated"][b]),
                       exp["info_all"][b])
        check(f"mapf_eval_record {t}")
        again = rec.reset_mask.astype(bool)
        want = _oracle_reset_subset(case, orc, again)
        env._check(env._lib.mapf_reset(env._h, g["reset_mask"].ptr, eng.buf["obs"].ptr, env._stream()))
        _sync(env)
        obs = eng.buf["obs"].check(active, f"reset after evaluation step {t}")  # (rows of the step, some overwritten by the reset)
        for b, o in want.items():
            _eq(f"reset obs of env {b}", obs[b], o, t)
        t += 1
        assert t <= E * case["cfg"]["steps_per_episode"] + 1
    assert (rec.episodes_recorded == E).all()
    env._check(env._lib.mapf_eval_end(env._h))
    env.poll_error()


# ---- host-pointer outputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["train16_lifelong_generic", "cte_n8_9x11_lanes8"])
def test_host_pointer_outputs_stay_inside_their_arrays(cid):
    from dl_reference_models_amd import _lib as L

    case = CASE_BY_ID[cid]
    B = gu.case_batches(case)[-1]
    inp = case_inputs(case, B)
    eng, orc = _started(case, inp, steps=9)
    env = eng.env
    want = env.get_state()
    g = {k: GuardedBuffer(v.shape, v.dtype, "numpy", guard_bytes_for(v.nbytes), name=f"mapf_state.{k}") for k, v in want.items()}
    s = L.MapfState(**{k: b.ptr for k, b in g.items()})
    env._check(env._lib.mapf_get_state(env._h, C.byref(s)))
    for k, b in g.items():
        _eq(f"mapf_get_state {k}", b.check(True, "mapf_get_state"), want[k])
    _eq("positions", want["positions"], orc.positions())
    stats = GuardedBuffer((12,), np.int64, "numpy", name="get_episode_stats")
    env._check(env._lib.mapf_get_episode_stats(env._h, stats.ptr, 1))
    assert stats.check(True)[0] >= 1
    stats.poison()
    env._check(env._lib.mapf_get_episode_stats(env._h, stats.ptr, 0))
    assert not stats.check(True).any()  # (cleared by the call before)
    if case["kind"] == "ma":
        goal = GuardedBuffer((2,), np.int16, "numpy", name="new_goal")
        e, j = B - 1, case["N"] - 1
        env._check(env._lib.mapf_assign_new_goal(env._h, e, j, goal.ptr, env._stream()))
        assert orc.batch.envs[e].assign_new_goal(j) == 0
        _eq("new goal", goal.check(True, "mapf_assign_new_goal"), orc.goals()[e, j])
        _eq("goals", env.get_state()["goals"], orc.goals())
        _eq("rng", eng.rng_words(), orc.rng_words())
