"""Compact lock-history planes: a handle whose lock windows are both <= 16 steps keeps 32 instead of 48 state bytes per
agent (16 bits of each shift register, the 16 distance bytes; mapf_kernels.inl, device-side data layout).  Every kernel that
reads or writes the history planes, on both layouts, against the oracle on traces in which the lock detector fires:
nine envs of eight agents are one full workgroup plus a ragged one (the three-wave kernel and its two-wave fallback in one
launch), 130 steps push more than 64 history bits through every register and cross three episode ends per env.

Every test first asserts FROM THE ORACLE ALONE that its trace is not a quiet one: both lock flags occur and episodes end
(the counts below are what the oracle gives for these inputs on the CPU)."""

from __future__ import annotations

import functools

import numpy as np
import pytest

from trace_util import EngineStepper, OracleStepper, _eq, compare_steppers, synth_grids

pytestmark = pytest.mark.gpu

ACTION_LAW = [0.1, 0.1, 0.5, 0.2, 0.1]
OUT_KEYS = ("obs", "rewards", "terminated", "truncated", "info_all", "info_agent")
COMPACT, WIDE = 32, 48


def _cfg(dw, lw, **over):
    cfg = {"env_name": "synthetic", "num_agents": 8, "sensor_range": 2, "steps_per_episode": 40,
           "include_action_mask_in_obs": True, "enable_lock_metrics": True,
           "deadlock_window_steps": dw, "livelock_window_steps": lw}
    cfg.update(over)
    return cfg


def _actions(T, B, N):
    return np.random.default_rng(3).choice(5, (T, B, N), p=ACTION_LAW).astype(np.int8)


@functools.lru_cache(maxsize=None)
def _case(kind, dw, lw, mask=True):
    """(grids, config, seeds, actions) of a case and the oracle's own (deadlock env-steps, livelock env-steps, finished
    episodes) on it, computed once."""
    if kind == "n8":
        grids, cfg, acts = synth_grids(9, 8, 8, 0.10, 8), _cfg(dw, lw), _actions(130, 9, 8)
    elif kind == "n16":  # specialisation 6 (16 lanes per env, bit rows)
        grids, acts = synth_grids(5, 10, 10, 0.10, 16), _actions(130, 5, 16)
        cfg = _cfg(dw, lw, num_agents=16, sensor_range=3, include_action_mask_in_obs=mask)
    else:  # "n40": wide groups (k_stepw), lifelong
        grids, cfg, acts = synth_grids(3, 12, 12, 0.10, 40), _cfg(dw, lw, num_agents=40, lifelong_mapf=True), _actions(80, 3, 40)
    seeds = list(range(grids.shape[0]))
    orc = OracleStepper(grids, cfg, seeds=seeds)
    orc.reset()
    dl = ll = ep = 0
    for t in range(acts.shape[0]):
        r = orc.step(acts[t])
        dl += int(r["info_all"][:, 4].sum())
        ll += int(r["info_all"][:, 5].sum())
        ep += int((r["terminated"].astype(bool) | r["truncated"].astype(bool)).sum())
    return grids, cfg, seeds, acts, (dl, ll, ep)


def _loud_case(kind, dw, lw, want, min_episodes=15, mask=True):
    """The case, after asserting from the oracle's info_all that both lock flags occurred and enough episodes ended."""
    grids, cfg, seeds, acts, seen = _case(kind, dw, lw, mask)
    dl, ll, ep = seen
    assert dl >= 1 and ll >= 1 and ep >= min_episodes, f"quiet trace: {seen}"
    assert seen == want, (seen, want)  # (the oracle's figures for these inputs)
    return grids, dict(cfg), seeds, acts


def _layout(eng):
    return eng.env.launch_info()["state_bytes_per_agent"]


# ---- 1. parity on both sides of the kernel choice, 2. the window boundary ---------------------------------------------------
@pytest.mark.parametrize("dw,lw,want,layout,knobs", [
    (8, 16, (78, 554, 27), COMPACT, {}),                              # the prebuilt specialisation: k_step3
    (8, 16, (78, 554, 27), COMPACT, {"force_generic_kernel": True}),  # the runtime-config kernels on the same handle layout
    (16, 16, (7, 623, 27), COMPACT, {}),                              # both windows use every kept bit
    (3, 5, (406, 609, 27), COMPACT, {}),
    (8, 17, (78, 522, 27), WIDE, {}),                                 # one step past the boundary: wide planes, int16 ring
])
def test_parity_with_the_oracle_on_either_layout(dw, lw, want, layout, knobs):
    grids, cfg, seeds, acts = _loud_case("n8", dw, lw, want)
    eng = EngineStepper(grids, cfg, seeds=seeds, **knobs)
    info = eng.env.launch_info()
    assert info["state_bytes_per_agent"] == layout
    if (dw, lw) == (8, 16) and not knobs:
        assert info["threads"] == 192 and info["specialized_kernel"] == 1, info  # k_step3 of specialisation 1
    if knobs:
        assert info["specialized_kernel"] == 0, info
    stats = compare_steppers(eng, OracleStepper(grids, cfg, seeds=seeds), acts)
    assert stats["episodes"] == want[2]
    eng.env.poll_error()


# ---- 3. sixteen lanes per env ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mask,special", [(True, 0), (False, 6)])
def test_sixteen_lane_groups_with_bit_rows(mask, special):
    """16 lanes per env on 10 x 10 with 7 x 7 windows (bit rows).  With the action mask in the
    observation (the common setup) no prebuilt shape matches and the runtime-config kernels run; without it the
    configuration is specialisation 6, the reference's training setup (its observation carries no mask).  The mask changes
    the observation only, so the oracle's lock figures are the same for both."""
    grids, cfg, seeds, acts = _loud_case("n16", 8, 16, (65, 312, 15), mask=mask)
    eng = EngineStepper(grids, cfg, seeds=seeds)
    info = eng.env.launch_info()
    assert info["state_bytes_per_agent"] == COMPACT and info["specialized_kernel"] == special, info
    compare_steppers(eng, OracleStepper(grids, cfg, seeds=seeds), acts)
    eng.env.poll_error()


# ---- 4. wide groups ----------------------------------------------------------------------------------------------------------
def test_wide_groups_lifelong():
    """N = 40 on 12 x 12, lifelong: k_stepw.  (Three envs of two 40-step episodes: six episode ends are all there can be,
    so the episode floor of this case is 6; both flags still have to occur.)"""
    grids, cfg, seeds, acts = _loud_case("n40", 8, 16, (101, 52, 6), min_episodes=6)
    eng = EngineStepper(grids, cfg, seeds=seeds)
    info = eng.env.launch_info()
    assert info["state_bytes_per_agent"] == COMPACT and info["threads"] == 192, info
    compare_steppers(eng, OracleStepper(grids, cfg, seeds=seeds), acts)
    eng.env.poll_error()


# ---- 5. fused launches -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("knobs", [{}, {"force_generic_kernel": True}])
def test_fused_launches_alternating_with_single_steps(knobs):
    """k_step_many (state in registers for T = 7 steps, the planes touched at its ends) alternating with single steps."""
    import torch

    grids, cfg, seeds, acts = _loud_case("n8", 8, 16, (78, 554, 27))
    eng, orc = EngineStepper(grids, cfg, seeds=seeds, **knobs), OracleStepper(grids, cfg, seeds=seeds)
    assert _layout(eng) == COMPACT
    _eq("reset", eng.reset(), orc.reset())
    t = rep = 0
    while t < acts.shape[0]:
        T = min(7, acts.shape[0] - t)
        out = eng.env.step_many(torch.from_numpy(acts[t:t + T]).to(eng.env.device), obs_mode=2)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        for i in range(T):
            r = orc.step(acts[t + i])
            for k in OUT_KEYS:
                _eq(f"fused {k} rep {rep}", out[k][i], r[k], t + i)
        t += T
        for _ in range(min(1 + rep % 3, acts.shape[0] - t)):
            ra, rb = eng.step(acts[t]), orc.step(acts[t])
            for k in OUT_KEYS:
                _eq(f"single {k} rep {rep}", ra[k], rb[k], t)
            t += 1
        _eq("rng words", eng.rng_words(), orc.rng_words(), rep)
        _eq("positions", eng.positions(), orc.positions(), rep)
        rep += 1
    eng.env.poll_error()


# ---- 6. snapshots ------------------------------------------------------------------------------------------------------------
def test_snapshot_keeps_sixteen_history_bits_and_resumes_identically():
    grids, cfg, seeds, acts = _loud_case("n8", 8, 16, (78, 554, 27))
    a, orc = EngineStepper(grids, cfg, seeds=seeds), OracleStepper(grids, cfg, seeds=seeds)
    assert _layout(a) == COMPACT
    a.reset()
    orc.reset()
    for t in range(57):
        a.step(acts[t])
        orc.step(acts[t])
    snap = a.env.get_state()
    assert snap["lock_history"].any(), "no history to snapshot"
    assert not (snap["lock_history"] >> np.uint64(16)).any(), "a compact handle reports history bits at or above 16"
    b = EngineStepper(grids, cfg, seeds=[1000 + s for s in seeds])  # other streams until the snapshot lands
    b.reset()
    b.env.set_state(**snap)
    dirty = dict(snap)
    dirty["lock_history"] = snap["lock_history"] | np.uint64(0xFFFFFFFFFFFF0000)  # all upper bits set by hand
    c = EngineStepper(grids, cfg, seeds=[2000 + s for s in seeds])
    c.reset()
    c.env.set_state(**dirty)
    for other in (b, c):
        back = other.env.get_state()
        for k in snap:  # get_state -> set_state -> get_state is the identity; the upper bits are not kept
            assert np.array_equal(snap[k], back[k]), k
    for t in range(57, 130):
        ro = orc.step(acts[t])
        for name, eng in (("original", a), ("resumed", b), ("resumed from upper bits set", c)):
            r = eng.step(acts[t])
            for k in OUT_KEYS:
                _eq(f"{name}: {k}", r[k], ro[k], t)
    for eng in (a, b, c):
        _eq("rng words", eng.rng_words(), orc.rng_words())
        eng.env.poll_error()
