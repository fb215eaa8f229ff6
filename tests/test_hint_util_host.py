"""hint_util on the CPU, with the oracle alone: the carved near-finish states are what the device tests of the "may finish"
hint (test_finish_hint_gpu.py) take them for -- a property of the inputs, not of luck."""
from __future__ import annotations

import numpy as np
import pytest

import guard_util as gu
import hint_util as hu
from trace_util import OracleStepper

SPE = hu.STEPS_PER_EPISODE


def _oracle(case, carved, seed):
    cfg = dict(case["cfg"], steps_per_episode=SPE)
    orc = OracleStepper(carved["grid"][None], cfg, seeds=[seed])
    orc.reset()
    orc.set_state(carved["positions"][None], carved["goals"][None])
    return orc


def test_can_end_formula():
    pos = np.array([[[0, 0], [3, 3]], [[0, 0], [3, 3]], [[0, 0], [3, 3]]])
    goal = np.array([[[0, 1], [3, 3]], [[1, 1], [3, 3]], [[1, 1], [3, 3]]])  # distances (1, 0), (2, 0), (2, 0)
    assert hu.can_end(pos, goal, np.array([0, 0, 4]), 6).tolist() == [True, False, False]
    assert hu.can_end(pos, goal, np.array([0, 4, 5]), 6).tolist() == [True, False, True]  # 5 + 1 >= 6: the step limit is due
    assert bool(hu.can_end(pos[1], goal[1], 0, 1)) and not bool(hu.can_end(pos[1], goal[1], 0, 2))


@pytest.mark.parametrize("variant", hu.VARIANTS)
@pytest.mark.parametrize("cid", hu.MA_CASE_IDS)
def test_carved_state_is_one_respawn_from_the_end(cid, variant):
    case = gu.CASE_BY_ID[cid]
    n, h, w = case["N"], case["H"], case["W"]
    cv = hu.carved_case(n, h, w, variant)
    assert cv["grid"].shape == (h, w)
    assert cv["n_free"] == int((cv["grid"] == 0).sum()) == 2 * n + (variant == "B")
    assert len({tuple(p) for p in cv["positions"].tolist()}) == n and len({tuple(g) for g in cv["goals"].tolist()}) == n
    for cell in np.concatenate([cv["positions"], cv["goals"], cv["x"][None]] + ([cv["y"][None]] if variant == "B" else [])):
        assert cv["grid"][cell[0], cell[1]] == 0, cell
    assert tuple(cv["goals"][0]) == tuple(cv["positions"][1])
    assert np.abs(cv["positions"][0].astype(int) - cv["goals"][0]).sum() >= 2
    assert (np.abs(cv["positions"][1:].astype(int) - cv["goals"][1:]).sum(axis=-1) == 1).all()
    allowed = {tuple(cv["x"].tolist())} | ({tuple(cv["y"].tolist())} if variant == "B" else set())
    seen = set()
    for seed in range(6):
        orc = _oracle(case, cv, 700 + seed)
        e = orc.batch.envs[0]
        noop = np.zeros((1, n), np.int8)
        out = orc.step(noop)  # the step that writes the hint on the device
        assert out["rc"] == 0 and not out["terminated"][0] and not out["truncated"][0]
        assert not hu.can_end(e.positions, e.goals, e.step_count, SPE)
        before = e.rng_words().copy()
        assert e.assign_new_goal(0) == 0
        g0 = tuple(e.goals[0].tolist())
        assert g0 in allowed, (g0, allowed)
        seen.add(g0)
        assert np.array_equal(e.rng_words(), before) == (variant == "A")  # k = 1 draws nothing, k = 2 draws once
        assert hu.can_end(e.positions, e.goals, e.step_count, SPE)
        out = orc.step(hu.finish_actions(cv, g0)[None])
        assert out["rc"] == 0 and out["terminated"][0] and not out["truncated"][0]
        assert (out["rewards"][0] >= 1.0).all()  # the success bonus of every agent (MA-env:668-690)
        # the oracle has reset (auto-reset: all 2N placement cells from the 2N or 2N + 1 free ones) and goes on
        assert e.step_count == 0
        rng = np.random.default_rng(seed)
        ends = 0
        for _ in range(3 * SPE):
            out = orc.step(rng.integers(0, 5, size=(1, n)).astype(np.int8))
            assert out["rc"] == 0
            ends += int(out["terminated"][0] | out["truncated"][0])
        assert ends >= 2, ends
    if variant == "B":
        assert seen == allowed, seen  # six seeds reach both candidates
