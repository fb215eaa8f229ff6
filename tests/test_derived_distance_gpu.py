"""Derived-distance history (``derived_distance_history``; mapf_kernels.inl, device-side data layout): a finite
handle whose lock windows are both <= 16 steps keeps one bit per step, "the distance went down", instead of the 16 goal-distance
bytes -- 16 instead of 32 state bytes per agent.  Every kernel family that reads or writes the history of such a handle, against
the C oracle (which keeps numeric distances): 19 envs of eight agents are two full workgroups plus a ragged one (the three-wave
kernel and its two-wave fallback in one launch), 130 steps with staggered phases and 40-step episodes cross at least three
in-kernel resets per env.

Every trace test first asserts FROM THE ORACLE ALONE that its trace is not a quiet one: both lock flags occur, and every env
ends at least three episodes."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from trace_util import EngineStepper, OracleStepper, _eq, synth_grids

pytestmark = pytest.mark.gpu

ACTION_LAW = [0.1, 0.1, 0.5, 0.2, 0.1]
OUT_KEYS = ("obs", "rewards", "terminated", "truncated", "info_all", "info_agent")
DERIVED, COMPACT, WIDE = 16, 32, 48
B, N, SPE, T_TRACE = 19, 8, 40, 130
PHASES = (np.arange(B) * 7) % SPE  # staggered episode boundaries


def _cfg(dw=8, lw=16, **over):
    # the headline specialisation: 8 agents, sensor range 2, mask + blocking pressure + lock metrics (flags 45), windows 8 / 16,
    # nearby 2, min neighbours 1 (the defaults)
    cfg = {"env_name": "synthetic", "num_agents": N, "sensor_range": 2, "steps_per_episode": SPE,
           "include_action_mask_in_obs": True, "enable_lock_metrics": True, "derived_distance_history": True,
           "deadlock_window_steps": dw, "livelock_window_steps": lw}
    cfg.update(over)
    return cfg


@functools.lru_cache(maxsize=None)
def _world():
    return synth_grids(B, 8, 8, 0.10, N), np.random.default_rng(3).choice(5, (T_TRACE, B, N), p=ACTION_LAW).astype(np.int8)


def _oracle(cfg):
    grids, _ = _world()
    orc = OracleStepper(grids, cfg, seeds=list(range(B)))
    return orc


@functools.lru_cache(maxsize=None)
def _loud(dw, lw):
    """The oracle alone on the trace: (deadlock env-steps, livelock env-steps, fewest episodes any env ended)."""
    _, acts = _world()
    orc = _oracle(_cfg(dw, lw))
    orc.reset()
    orc.set_step_counts(PHASES)
    dl = ll = 0
    ep = np.zeros(B, int)
    for t in range(T_TRACE):
        r = orc.step(acts[t])
        dl += int(r["info_all"][:, 4].sum())
        ll += int(r["info_all"][:, 5].sum())
        ep += r["terminated"].astype(bool) | r["truncated"].astype(bool)
    return dl, ll, int(ep.min())


def _assert_loud(dw=8, lw=16):
    dl, ll, ep = _loud(dw, lw)
    assert dl >= 1 and ll >= 1 and ep >= 3, f"quiet trace: deadlock {dl}, livelock {ll}, fewest episodes per env {ep}"


def _engine(cfg, **knobs):
    grids, _ = _world()
    return EngineStepper(grids, cfg, seeds=list(range(B)), **knobs)


def _layout(eng):
    return eng.env.launch_info()["state_bytes_per_agent"]


def _oracle_counters(orc, hs):
    rows = []
    for e in orc.batch.envs:
        c = e.counters()
        rows.append([c["step_count"], e.hist["count"], c["episode_blocking_count"], c["episode_goals_reached_total"],
                     c["episode_deadlock_events"], c["episode_livelock_events"], c["episode_deadlock_steps"],
                     c["episode_livelock_steps"]])
    return np.asarray(rows, dtype=np.int64)


def _engine_counters(eng, hs):
    c = eng.env.get_state()["counters"].astype(np.int64)
    c[:, 1] = np.minimum(c[:, 1], hs)  # the engine counts rows, the reference's count stops at its history size
    return c[:, :8]


def _check_step(tag, t, got, want, eng, orc, hs, rows=None):
    sel = slice(None) if rows is None else rows
    for k in OUT_KEYS:
        _eq(f"{tag}: {k}", np.asarray(got[k])[sel], np.asarray(want[k])[sel], t)
    _eq(f"{tag}: counters", _engine_counters(eng, hs), _oracle_counters(orc, hs), t)


def _start(eng, orc):
    _eq("reset obs", eng.reset(), orc.reset())
    eng.set_step_counts(PHASES)
    orc.set_step_counts(PHASES)


def _oracle_masked_step(orc, actions, mask):
    """The envs of `mask` step (and auto-reset) in the oracle, one by one; the others are not touched."""
    out = {"obs": np.zeros((B, N, orc.L), np.float32), "rewards": np.zeros((B, N), np.float32),
           "terminated": np.zeros(B, np.uint8), "truncated": np.zeros(B, np.uint8),
           "info_all": np.zeros((B, 14), np.float32), "info_agent": np.zeros((B, N, 2), np.uint8)}
    for b in np.flatnonzero(mask):
        e = orc.batch.envs[b]
        rc, obs, rew, term, trunc, ia, ig = e.step(actions[b].astype(np.int32))
        assert rc == 0
        if term or trunc:
            rc, obs = e.reset()
            assert rc == 0
        out["obs"][b], out["rewards"][b], out["terminated"][b], out["truncated"][b] = obs, rew, term, trunc
        out["info_all"][b], out["info_agent"][b] = ia, ig
    return out


# ---- 1. trace parity through every kernel family -----------------------------------------------------------------------------
@pytest.mark.parametrize("mode,knobs", [
    ("single", {}),                                        # k_step3 + its two-wave fallback for the ragged workgroup
    ("single", {"register_budget": "dense"}),              # the dense two-wave build (k_step, WPS = 4)
    ("single", {"force_generic_kernel": True}),            # the runtime-config kernels on the same layout
    ("many", {}),                                          # k_step_many, T in {1, 7, 33}, alternating with single steps
    ("masked", {}),                                        # masked steps in between
])
def test_trace_parity_with_the_oracle(mode, knobs):
    import torch

    _assert_loud()
    _, acts = _world()
    cfg = _cfg()
    eng, orc = _engine(cfg, **knobs), _oracle(cfg)
    info = eng.env.launch_info()
    assert info["state_bytes_per_agent"] == DERIVED, info
    if not knobs:
        assert info["specialized_kernel"] == 1 and info["threads"] == 192, info
    if "register_budget" in knobs:
        assert info["specialized_kernel"] == 1 and info["threads"] == 128, info
    if "force_generic_kernel" in knobs:
        assert info["specialized_kernel"] == 0, info
    hs = 16
    _start(eng, orc)
    t = rep = 0
    mask_rng = np.random.default_rng(11)
    while t < T_TRACE:
        if mode == "many":
            T = min((1, 7, 33)[rep % 3], T_TRACE - t)
            out = eng.env.step_many(torch.from_numpy(acts[t:t + T]).to(eng.env.device), obs_mode=2)
            out = {k: v.cpu().numpy() for k, v in out.items()}
            for i in range(T):
                r = orc.step(acts[t + i])
                for k in OUT_KEYS:
                    _eq(f"fused T={T}: {k}", out[k][i], r[k], t + i)
            _eq("fused: counters", _engine_counters(eng, hs), _oracle_counters(orc, hs), t + T - 1)
            t += T
            if t >= T_TRACE:
                break
        if mode == "masked" and t % 3 == 1:
            mask = mask_rng.random(B) < 0.5
            mask[t % B] = True
            m = torch.from_numpy(mask.astype(np.uint8)).to(eng.env.device)
            a = torch.from_numpy(acts[t]).to(eng.env.device)
            got = {k: (v.cpu().numpy() if v is not None else None) for k, v in eng.env.step(a, env_mask=m).items()}
            want = _oracle_masked_step(orc, acts[t], mask)
            _check_step("masked", t, got, want, eng, orc, hs, rows=mask)
        else:
            _check_step(mode, t, eng.step(acts[t]), orc.step(acts[t]), eng, orc, hs)
        t += 1
        rep += 1
    _eq("rng words", eng.rng_words(), orc.rng_words())
    _eq("positions", eng.positions(), orc.positions())
    assert _layout(eng) == DERIVED  # nothing on the way made the handle leave the layout
    eng.env.poll_error()


# ---- 2. other windows through the runtime-config kernels; the boundary -----------------------------------------------------------
@pytest.mark.parametrize("dw,lw,layout", [(3, 5, DERIVED), (16, 16, DERIVED), (8, 17, WIDE)])
def test_other_windows_on_the_runtime_config_kernels(dw, lw, layout):
    _assert_loud(dw, lw)
    _, acts = _world()
    cfg = _cfg(dw, lw)
    eng, orc = _engine(cfg), _oracle(cfg)
    info = eng.env.launch_info()
    assert info["state_bytes_per_agent"] == layout and info["specialized_kernel"] == 0, info
    hs = max(dw, lw)
    _start(eng, orc)
    for t in range(T_TRACE):
        _check_step(f"windows {dw}/{lw}", t, eng.step(acts[t]), orc.step(acts[t]), eng, orc, hs)
    _eq("rng words", eng.rng_words(), orc.rng_words())
    eng.env.poll_error()


def test_the_layout_is_on_request_and_finite_only():
    grids, _ = _world()
    plain = dict(_cfg())
    del plain["derived_distance_history"]
    assert _layout(EngineStepper(grids[:2], plain, seeds=[0, 1])) == COMPACT
    assert _layout(EngineStepper(grids[:2], _cfg(lifelong_mapf=True), seeds=[0, 1])) == COMPACT
    assert _layout(EngineStepper(grids[:2], _cfg(enable_lock_metrics=False), seeds=[0, 1])) == DERIVED


# ---- 3. state parity ---------------------------------------------------------------------------------------------------------
def _oracle_ring(orc, rows_written, lw):
    """The oracle's numeric distances in the mapf_state layout [B][lw][N]: slot = history row index mod lw."""
    ring = np.zeros((B, lw, N), np.int16)
    for b, e in enumerate(orc.batch.envs):
        h = e.hist
        hs, t = h["distance"].shape[0], int(rows_written[b])
        assert h["count"] == min(t, hs)
        for k in range(min(t, lw)):
            ring[b, (t - 1 - k) % lw] = h["distance"][(h["head"] - 1 - k) % hs]
    return ring


def test_get_state_rebuilds_the_numeric_ring_and_snapshots_resume():
    _assert_loud()
    _, acts = _world()
    cfg = _cfg()
    a, orc = _engine(cfg), _oracle(cfg)
    _eq("reset obs", a.reset(), orc.reset())  # in phase: the rows written are the steps taken, for every env
    rows = np.zeros(B, int)
    checked_after_reset = checked_three_later = False
    since_reset = np.full(B, -1)
    snap = b = None
    for t in range(70):
        ra, ro = a.step(acts[t]), orc.step(acts[t])
        for k in OUT_KEYS:
            _eq(k, ra[k], ro[k], t)
        done = (ro["terminated"] | ro["truncated"]).astype(bool)
        rows = np.where(done, 0, rows + 1)
        since_reset = np.where(done, 0, np.where(since_reset >= 0, since_reset + 1, -1))
        if b is not None:
            rb = b.step(acts[t])
            for k in OUT_KEYS:
                _eq(f"resumed: {k}", rb[k], ro[k], t)
        after_reset, three_later = bool(done.any()), bool((since_reset == 3).any())
        if t + 1 in (1, 5, 16, 17) or after_reset or three_later:
            st = a.env.get_state()
            _eq("history rows", st["counters"][:, 1], rows, t)
            _eq("distance_ring", st["distance_ring"], _oracle_ring(orc, rows, 16), t)
            checked_after_reset |= after_reset
            checked_three_later |= three_later
            a.env.set_state(**st)  # set_state(get_state()) changes nothing
            back = a.env.get_state()
            for k in st:
                assert np.array_equal(st[k], back[k]), (k, t)
            assert _layout(a) == DERIVED
        if t + 1 == 23:  # a snapshot resumed in a fresh engine (other streams until it lands) continues bit-exact
            snap = a.env.get_state()
            b = _engine(cfg)
            b.env.reset()
            b.env.set_state(**snap)
            assert _layout(b) == DERIVED
            back = b.env.get_state()
            for k in snap:
                assert np.array_equal(snap[k], back[k]), k
    assert checked_after_reset and checked_three_later
    for eng in (a, b):
        _eq("rng words", eng.rng_words(), orc.rng_words())
        eng.env.poll_error()


# ---- 4. demotion: states the bits cannot express ----------------------------------------------------------------------------
def _ten_steps(cfg):
    _, acts = _world()
    eng, orc = _engine(cfg), _oracle(cfg)
    _eq("reset obs", eng.reset(), orc.reset())
    for t in range(10):
        ra, ro = eng.step(acts[t]), orc.step(acts[t])
        for k in OUT_KEYS:
            _eq(k, ra[k], ro[k], t)
        assert not (ro["terminated"] | ro["truncated"]).any()  # a 10-row history in every env
    assert _layout(eng) == DERIVED
    return eng, orc


def _forty_more(eng, orc, twin=None):
    """40 more steps against the oracle; returns (deadlock, livelock) env-steps and events, and whether `twin` (an oracle
    without the hand-made change) ever gave other lock figures."""
    _, acts = _world()
    seen = np.zeros(4)
    differs = False
    for t in range(10, 50):
        ra, ro = eng.step(acts[t]), orc.step(acts[t])
        for k in OUT_KEYS:
            _eq(f"after the demotion: {k}", ra[k], ro[k], t)
        _eq("lock flags and events", ra["info_all"][:, 4:12], ro["info_all"][:, 4:12], t)
        seen += ro["info_all"][:, 4:8].sum(0)
        if twin is not None:
            differs |= not np.array_equal(twin.step(acts[t])["info_all"][:, 4:12], ro["info_all"][:, 4:12])
    _eq("rng words", eng.rng_words(), orc.rng_words())
    _eq("positions", eng.positions(), orc.positions())
    eng.env.poll_error()
    assert _layout(eng) == COMPACT
    return seen, differs


def test_demotion_by_a_ring_with_a_jump_of_three():
    cfg = _cfg(steps_per_episode=200)
    eng, orc = _ten_steps(cfg)
    twin = _oracle(cfg)
    twin.reset()
    _, acts = _world()
    for t in range(10):
        twin.step(acts[t])
    st = eng.env.get_state()
    ring = st["distance_ring"].copy()
    ring[:, (10 - 1 - 2) % 16, :] += 3  # the row two back, every agent: no one-cell walk leads there
    for e in orc.batch.envs:
        h = e.hist
        h["distance"][(h["head"] - 1 - 2) % h["distance"].shape[0]] += 3
    eng.env.set_state(distance_ring=ring)
    assert _layout(eng) == COMPACT and eng.env.launch_info()["specialized_kernel"] == 1
    _eq("the ring as supplied", eng.env.get_state()["distance_ring"], ring)
    seen, differs = _forty_more(eng, orc, twin)
    assert seen[1] >= 1 and differs, (seen, differs)  # livelock steps occur, and the hand-made row changed a lock figure


def test_demotion_by_positions_moved_under_a_history():
    cfg = _cfg(steps_per_episode=200)
    eng, orc = _ten_steps(cfg)
    grids, _ = _world()
    st = eng.env.get_state()
    pos, goals = st["positions"].copy(), st["goals"]
    for b in range(B):  # agent 0 of every env goes to the first free, unoccupied cell at another distance from its goal
        d_now = np.abs(goals[b, 0] - pos[b, 0]).sum()
        taken = {tuple(p) for p in pos[b]}
        for r, c in np.argwhere(grids[b] == 0):
            if (r, c) not in taken and abs(goals[b, 0, 0] - r) + abs(goals[b, 0, 1] - c) not in (d_now, 0):
                pos[b, 0] = (r, c)
                break
        else:
            raise AssertionError("no cell to move to")
    ring_before = st["distance_ring"]
    eng.env.set_state(positions=pos)
    for b, e in enumerate(orc.batch.envs):
        e.positions[:] = pos[b]
        e.rebuild_owner_maps()
    assert _layout(eng) == COMPACT
    _eq("the history stays what it was", eng.env.get_state()["distance_ring"], ring_before)
    seen, _ = _forty_more(eng, orc)
    assert seen[1] >= 1, seen


def test_demotion_by_assign_new_goal_on_a_finite_handle():
    cfg = _cfg(steps_per_episode=200)
    eng, orc = _ten_steps(cfg)
    ring_before = eng.env.get_state()["distance_ring"]
    for b in (0, 7, 18):
        want = orc.batch.envs[b]
        assert want.assign_new_goal(b % N) == 0
        got = eng.env.assign_new_goal(b, b % N)
        _eq("new goal", got, want.goals[b % N])
    assert _layout(eng) == COMPACT
    _eq("the history stays what it was", eng.env.get_state()["distance_ring"], ring_before)
    _eq("rng words", eng.rng_words(), orc.rng_words())
    seen, _ = _forty_more(eng, orc)
    assert seen[1] >= 1, seen
