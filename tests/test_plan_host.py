"""The shortest-path planner without a GPU: the C ABI declares it, the NumPy restatement of its rule (plan_util) gives the
known answers, the case table holds every decision the rule makes, and the bit-row formulation the kernel runs gives the
same fields as the plain breadth-first search."""

import os
import re

import numpy as np
import pytest

import plan_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PLAN_SYMBOLS = ("mapf_expert_actions", "mapf_path_lengths", "mapf_distance_field")


def test_header_and_bindings_carry_the_three_entry_points():
    from dl_reference_models_amd import _lib as L

    with open(os.path.join(ROOT, "include", "mapf_step.h"), encoding="utf-8") as f:
        header = f.read()
    for name in PLAN_SYMBOLS:
        assert re.search(r"^int " + name + r"\(mapf_handle h,", header, re.M), name
        assert name in L.EXPORTED_SYMBOLS, name
    # the write contracts, in the header
    assert header.count("nothing else.") >= 3


def test_the_planner_is_a_launch_unit_of_every_variant():
    from dl_reference_models_amd import build

    assert build.PLAN_SOURCE in build.SOURCES and os.path.exists(build.PLAN_SOURCE)
    for name, (_so, _flags, units) in build.VARIANTS.items():
        assert [u for u in units if u[0] == "plan" and u[1] == build.PLAN_SOURCE], name


@pytest.mark.parametrize("shape", pu.SERPENTINES)
def test_serpentine_known_answers(shape):
    g = pu.serpentine(*shape)
    f = pu.field(g, (0, 0))
    farthest, n_free = pu.SERPENTINE_ANSWERS[shape]
    assert int((g == 0).sum()) == n_free
    assert int(f.max()) == farthest and int((f >= 0).sum()) == n_free
    assert (f[g != 0] == -1).all()


def test_serpentine_answers_are_what_the_issue_states():
    assert pu.SERPENTINE_ANSWERS[(11, 12)] == (76, 77)
    assert [pu.SERPENTINE_ANSWERS[s][0] for s in pu.SERPENTINES] == [76, 453, 2079, 1086]


@pytest.mark.parametrize("case", pu.RULE_CASES, ids=lambda c: c["name"])
def test_hand_cases(case):
    for mode, name in ((0, "independent"), (1, "yielding")):
        acts, dist = pu.expert_env(case["grid"], case["positions"], case["goals"], mode)
        assert acts.tolist() == case[name], (name, acts)
        assert dist.tolist() == case["dist"], (name, dist)


def test_case_table_holds_every_decision_of_the_rule():
    by = {c["name"]: c for c in pu.RULE_CASES}
    c = by["unreachable_pair"]
    assert c["dist"][0] == -1 and c["independent"][0] == 0 and c["yielding"][0] == 0
    c = by["agent_on_its_goal"]
    assert tuple(c["positions"][0]) == tuple(c["goals"][0]) and c["dist"][0] == 0 and c["independent"][0] == 0
    # two optimal moves: both neighbours are one step nearer, the lower id is taken
    c = by["two_optimal_moves_lowest_id"]
    f = pu.field(c["grid"], c["goals"][0])
    r, col = (int(v) for v in c["positions"][0])
    nearer = [a for a, (dr, dc) in pu.DELTAS.items()
              if 0 <= r + dr < 3 and 0 <= col + dc < 3 and f[r + dr, col + dc] == c["dist"][0] - 1]
    assert nearer == [1, 2] and c["independent"][0] == 1
    c = by["yields_to_another_optimal_move"]
    assert c["independent"][0] == 1 and c["yielding"][0] == 2
    blocked = tuple(int(v) for v in c["positions"][0] + np.array(pu.DELTAS[1]))
    assert blocked == tuple(int(v) for v in c["positions"][1])
    c = by["yielding_agent_waits"]
    assert c["independent"][0] == 2 and c["yielding"][0] == 0 and c["dist"][0] > 0
    c = by["path_longer_than_h_plus_w"]
    assert c["dist"][0] > sum(c["grid"].shape)


def test_three_by_three_hand_fields():
    want = np.array([[0, -1, -1], [1, -1, -1], [2, -1, -1]], np.int32)
    assert np.array_equal(pu.field(pu.WALL3, (0, 0)), want)
    assert np.array_equal(pu.field(pu.OPEN3, (1, 1)), np.array([[2, 1, 2], [1, 0, 1], [2, 1, 2]], np.int32))
    assert (pu.field(pu.WALL3, (1, 1)) == -1).all()  # a destination on an obstacle
    assert (pu.field(pu.OPEN3, (3, 0)) == -1).all() and (pu.field(pu.OPEN3, (0, -1)) == -1).all()  # outside the grid
    assert pu.distance(pu.OPEN3, (0, 3), (0, 0)) == -1 and pu.distance(pu.OPEN3, (-1, 0), (0, 0)) == -1
    assert pu.field_u16(pu.WALL3, (0, 0))[0, 2] == 0xFFFF


def _sample_dsts(grid, rng, n):
    cells = pu.free_cells(grid)
    return [tuple(int(v) for v in cells[i]) for i in rng.integers(len(cells), size=n)]


def test_random_grids_give_unreachable_cells_long_paths_and_ties():
    """What density 0.4 gives without looking for it: cells no path reaches, paths longer than H + W, cells with two
    optimal moves; density 0.2 at 64 x 64 is the connected case."""
    rng = np.random.default_rng(0)
    for (H, W) in ((12, 12), (12, 33), (64, 64)):
        unreachable = longest = ties = free = 0
        for b in range(4):
            g = pu.random_grids(H, W, 4)[b]
            for dst in _sample_dsts(g, rng, 4):
                f = pu.field(g, dst)
                free += int((g == 0).sum())
                unreachable += int(((g == 0) & (f < 0)).sum())
                longest = max(longest, int(f.max()))
                for r, c in np.argwhere(f > 0):
                    n = sum(1 for dr, dc in pu.DELTAS.values()
                            if 0 <= r + dr < H and 0 <= c + dc < W and f[r + dr, c + dc] == f[r, c] - 1)
                    ties += n >= 2
        assert unreachable > 0.3 * free, (H, W, unreachable, free)
        assert ties > 50, (H, W, ties)
        if (H, W) == (64, 64):  # (the small shapes have their long paths from the serpentines)
            assert longest > H + W, (H, W, longest)
    g = pu.random_grids(64, 64, 1, pu.DENSITY_CONNECTED)[0]
    f = pu.field(g, _sample_dsts(g, rng, 1)[0])
    assert ((g == 0) & (f < 0)).sum() < 0.02 * (g == 0).sum()


@pytest.mark.parametrize("shape", pu.SHAPES + pu.SERPENTINES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_bit_row_expansion_gives_the_same_fields(shape):
    """reach' = (reach | reach << 1 | reach >> 1 | above | below) & free on Python ints against the deque search."""
    H, W = shape
    rng = np.random.default_rng(H * 100 + W)
    grids = [pu.random_grids(H, W, 2)[b] for b in range(2)] if shape in pu.SHAPES else []
    if shape in pu.SERPENTINES:
        grids += [pu.serpentine(H, W)]
    for g in grids:
        dsts = _sample_dsts(g, rng, 2) + [(0, 0), (H - 1, W - 1)]
        if (g != 0).any():
            dsts.append(tuple(int(v) for v in np.argwhere(g != 0)[0]))
        for dst in dsts:
            assert np.array_equal(pu.bit_row_field(g, dst), pu.field(g, dst)), (shape, dst)


def test_queries_cover_the_special_sources():
    grids = pu.random_grids(12, 12, 5)
    env_ids, src, dst = pu.queries(grids, 67, 1)
    assert tuple(src[0]) == tuple(dst[0]) and len(set(env_ids.tolist())) < len(env_ids)
    assert grids[env_ids[1]][tuple(src[1])] != 0
    d = [pu.distance(grids[e], s, t) for e, s, t in zip(env_ids, src, dst)]
    assert d[0] == 0 and d[1] == -1 and min(d) == -1 and max(d) > 0


def test_bounds_from_lengths():
    from dl_reference_models_amd.evaluation import bounds_from_lengths

    b = bounds_from_lengths(np.array([[3, 5, 0], [4, -1, 2]], np.int32))
    assert b["sum_of_costs_lower_bound"].tolist() == [8, -1]
    assert b["makespan_lower_bound"].tolist() == [5, -1]
    assert b["shortest_path"].dtype == np.int32 and b["shortest_path"].shape == (2, 3)
