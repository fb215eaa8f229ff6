"""Conflict-based search without a GPU: the C ABI declares it; the two restatements of its rule (cbs_util: on sets, on bit
rows with the kernel's node store) agree; every solved plan executes under the restated move phase and on the CPU oracle of
the env without a failed move, so the rule is pinned against the env itself and not against the kernel; the hand cases hold
what the rule decides; the sum of costs is the optimum of an exhaustive joint-state search, never above the prioritised
planner's and never below the shortest-path bound; and the instance tables hold what the GPU tests need of them."""

import os
import re

import numpy as np
import pytest

import cbs_util as cu
import plan_util as pu
import prioritized_util as pq
from test_prioritized_host import _execute_on_oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_and_bindings_carry_the_entry_point():
    from dl_reference_models_amd import _lib as L

    with open(os.path.join(ROOT, "include", "mapf_step.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"^int mapf_plan_cbs\(mapf_handle h, int32_t horizon, int32_t max_nodes, const uint8_t \*mask", header, re.M)
    assert re.search(r"^int mapf_plan_cbs_max_nodes\(mapf_handle h\);", header, re.M)
    assert re.search(r"^int64_t mapf_plan_cbs_workspace_bytes\(mapf_handle h, int32_t horizon, int32_t max_nodes\);", header, re.M)
    for name in ("mapf_plan_cbs", "mapf_plan_cbs_max_nodes", "mapf_plan_cbs_workspace_bytes"):
        assert name in L.EXPORTED_SYMBOLS
    assert int(re.search(r"^#define MAPF_CBS_MAX_HORIZON (\d+)", header, re.M).group(1)) == 128 == L.CBS_MAX_HORIZON
    assert int(re.search(r"^#define MAPF_CBS_MAX_NODES (\d+)", header, re.M).group(1)) == 1024 == L.CBS_MAX_NODES
    for name, code in (("SOLVED", cu.SOLVED), ("BUDGET", cu.BUDGET), ("INFEASIBLE", cu.INFEASIBLE), ("NO_PATH", cu.NO_PATH)):
        assert int(re.search(rf"^#define MAPF_CBS_{name} (\d+)", header, re.M).group(1)) == code == getattr(L, "CBS_" + name)
    # the rule is stated above the call
    rule = header[header.index("Conflict-based search"):header.index("int mapf_plan_cbs(")]
    for word in ("constraint (a, x, t)", "reach[0] = {p_a}", "lowest action id", "c_i[t + 1] == c_k[t]", "(cost, node id)",
                 "16 + 2 * P", "not larger"):
        assert word in rule, word


def test_policy_and_script_names():
    from dl_reference_models_amd import evaluation as evm

    assert "cbs" in evm.STRING_POLICIES
    with open(os.path.join(ROOT, "scripts", "evaluate_multi_agent_env.py"), encoding="utf-8") as f:
        text = f.read()
    assert '"CBS"' in text and "--max-nodes" in text


def test_cbs_summary():
    from dl_reference_models_amd.evaluation import cbs_summary

    got = cbs_summary(np.array([0, 0, 1, 3], np.int32), np.array([1, 5, 8, 0], np.int32))
    assert got == {"solved": 0.5, "budget": 0.25, "infeasible": 0.0, "no_path": 0.25, "mean_nodes": 3.5, "max_nodes_created": 8}


# ---- the two restatements ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(cu.CASES)), ids=cu.CASE_IDS)
def test_the_two_restatements_agree(i):
    _kind, _H, _W, N, _d, T, max_nodes, B, _seed = cu.CASES[i]
    grids, pos, goals = cu.case_instances(i)
    plan, arrival, status, nodes, cells = cu.restated(i)
    for b in range(B):
        p2, a2, s2, n2, c2 = cu.cbs_sets(grids[b], pos[b], goals[b], T, max_nodes)
        assert (status[b], nodes[b]) == (s2, n2), (b, status[b], nodes[b], s2, n2)
        assert np.array_equal(arrival[b], a2) and np.array_equal(plan[b], p2) and np.array_equal(cells[b], c2), b
    # what the outputs look like: nothing but zeros and -1 unless solved, nothing after the arrival, nodes within the budget
    assert plan.min() >= 0 and plan.max() <= 4
    assert ((nodes >= 1) & (nodes <= max_nodes))[status != cu.NO_PATH].all() and (nodes[status == cu.NO_PATH] == 0).all()
    for b in range(B):
        if status[b] != cu.SOLVED:
            assert not plan[b].any() and (arrival[b] == -1).all()
            continue
        for j in range(N):
            assert not plan[b, arrival[b, j]:, j].any()
            assert (cells[b, 0, j] == pos[b, j]).all() and (cells[b, arrival[b, j]:, j] == goals[b, j]).all()
        assert cu.first_conflict([[tuple(c) for c in cells[b, :, j]] for j in range(N)], T) is None


# ---- executability on the env's own rule ---------------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(len(cu.CASES)), ids=cu.CASE_IDS)
def test_solved_plans_execute_on_the_oracle_without_a_failed_move(i):
    T = cu.CASES[i][5]
    grids, pos, goals = cu.case_instances(i)
    plan, arrival, status, _nodes, cells = cu.restated(i)
    for b in np.flatnonzero(status == cu.SOLVED):
        p = pos[b]
        for t in range(1, int(arrival[b].max()) + 1):
            p, failed = pq.simulate_moves(grids[b], p, plan[b, t - 1])
            assert not failed.any() and np.array_equal(p, cells[b, t]), (b, t)
        done_at = _execute_on_oracle(grids[b], pos[b], goals[b], plan[b], cells[b], T)
        want = pq.first_all_on_goal(cells[b], goals[b])
        assert done_at == want and want <= max(int(arrival[b].max()), 1), (b, done_at, want)


# ---- hand cases ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cu.HAND_CASES, ids=lambda c: c["name"])
def test_hand_cases(case):
    g, pos, goals, T = case["grid"], case["positions"], case["goals"], case["T"]
    for fn in (cu.cbs_sets, cu.cbs_bit_rows):
        plan, arrival, status, nodes, cells = fn(g, pos, goals, T, case["max_nodes"])
        assert (status, nodes) == (case["status"], case["nodes"]), fn.__name__
        assert arrival.tolist() == (case["arrival"] if status == cu.SOLVED else [-1] * len(pos)), fn.__name__
        for j, path in case["cells"].items():
            assert [tuple(c) for c in cells[:len(path), j].tolist()] == path, (fn.__name__, j)
    if status == cu.SOLVED:
        assert _execute_on_oracle(g, pos, goals, plan, cells, T) == pq.first_all_on_goal(cells, goals)


def test_case_table_holds_every_property():
    by = {c["name"]: c for c in cu.HAND_CASES}
    assert len(by) == len(cu.HAND_CASES) and {c["status"] for c in cu.HAND_CASES} == set(cu.STATUS_NAMES)
    # the earlier agent steps aside: the prioritised planner fails agent 1 on the same instance, CBS solves it
    c = by["head_on_earlier_agent_steps_aside"]
    _plan, arrival, _cells = pq.plan_bit_rows(c["grid"], c["positions"], c["goals"], c["T"])
    assert arrival.tolist() == [4, -1] and c["status"] == cu.SOLVED and (0, 1) in c["cells"][0]
    # the O conflict at time 0 and its one child
    c = by["o_conflict_at_time_0_has_one_child"]
    root = [cu.low_level_sets(c["grid"], c["positions"][j], c["goals"][j], c["T"], set())[1] for j in range(2)]
    conflict = cu.first_conflict(root, c["T"])
    assert conflict == ("O", 0, 1, 0, (0, 1)) and cu.children_of(conflict) == [(0, (0, 1), 1)] and c["nodes"] == 2
    # a constraint on the goal after the first arrival delays the arrival
    h = cu.HAND_LOW_LEVEL
    assert cu.low_level_sets(h["grid"], h["p"], h["g"], h["T"], set())[0] == 1
    A, cells = cu.low_level_sets(h["grid"], h["p"], h["g"], h["T"], h["cons"])
    assert A == h["arrival"] and cells[:A + 1] == h["cells"]
    # the prioritised planner's unsolved instance, unchanged
    c, p = by["parked_goal_cuts_the_corridor_ends_in_budget"], {x["name"]: x for x in pq.HAND_CASES}["parked_goal_cuts_the_corridor"]
    assert all(np.array_equal(c[k], p[k]) for k in ("grid", "positions", "goals")) and c["T"] == p["T"]
    # one node: the same instance as the head-on case, and a budget of exactly the root
    assert by["one_node_solves_a_conflict_free_root"]["max_nodes"] == by["one_node_is_budget_at_the_first_conflict"]["max_nodes"] == 1
    # equal costs: the two children of the root cost the same, and the solution is the second
    c = by["equal_costs_are_taken_in_node_order"]
    root = [cu.low_level_sets(c["grid"], c["positions"][j], c["goals"][j], c["T"], set()) for j in range(2)]
    kids = cu.children_of(cu.first_conflict([r[1] for r in root], c["T"]))
    costs = [cu.low_level_sets(c["grid"], c["positions"][a], c["goals"][a], c["T"], {(x, t)})[0] - root[a][0] for a, x, t in kids]
    assert costs == [1, 1] and c["arrival"] == [root[0][0], root[1][0] + 1] and c["nodes"] == 5


# ---- optimality ------------------------------------------------------------------------------------------------------------
def test_moves_is_simulate_moves():
    rng = np.random.default_rng(3)
    grid = pu.random_grids(4, 4, 1, 0.2, 6)[0]
    free = {(r, c) for r in range(4) for c in range(4) if grid[r, c] == 0}
    cells = pu.free_cells(grid)
    for _ in range(200):
        pos = cells[rng.permutation(len(cells))[:3]]
        acts = rng.integers(0, 5, 3)
        want, _failed = pq.simulate_moves(grid, pos, acts)
        assert cu.moves(free, tuple(map(tuple, pos.tolist())), tuple(int(a) for a in acts)) == tuple(map(tuple, want.tolist()))


@pytest.mark.parametrize("H,W,N,density,T,B", [(3, 3, 2, 0.0, 8, 24), (4, 4, 3, 0.2, 10, 6)], ids=["3x3_n2", "4x4_n3"])
def test_sum_of_costs_is_the_optimum_of_an_exhaustive_search(H, W, N, density, T, B):
    grids, pos, goals = pq.instances("random", H, W, N, density, B, 3)
    n_conflicts = 0
    for b in range(B):
        _plan, arrival, status, nodes, _cells = cu.cbs_bit_rows(grids[b], pos[b], goals[b], T, 1024)
        best = cu.optimal_sum_of_costs(grids[b], pos[b], goals[b], T)
        assert status in (cu.SOLVED, cu.INFEASIBLE, cu.NO_PATH), (b, status)  # (the budget is no limit here)
        assert (int(arrival.sum()) if status == cu.SOLVED else -1) == best, (b, status, arrival, best)
        n_conflicts += nodes > 1
    assert n_conflicts >= 2  # (the search had something to resolve)


@pytest.mark.parametrize("i", range(len(cu.CASES)), ids=cu.CASE_IDS)
def test_cost_lies_between_the_lower_bound_and_the_prioritised_plan(i):
    from dl_reference_models_amd.evaluation import bounds_from_lengths, plan_costs

    kind, H, W, N, density, T, _m, B, seed = cu.CASES[i]
    grids, pos, goals = cu.case_instances(i)
    _plan, arrival, status, _nodes, _cells = cu.restated(i)
    prio = plan_costs(pq.plan_batch(pq.plan_bit_rows, grids, pos, goals, T)[1])
    got = plan_costs(arrival)
    assert np.array_equal(got["solved"], status == cu.SOLVED)
    sp = np.array([[pu.distance(grids[b], pos[b, j], goals[b, j]) for j in range(N)] for b in range(B)], np.int32)
    bounds = bounds_from_lengths(sp)
    s = got["solved"]
    assert (got["sum_of_costs"][s] >= bounds["sum_of_costs_lower_bound"][s]).all() and (bounds["sum_of_costs_lower_bound"][s] >= 0).all()
    assert (got["makespan"][s] >= bounds["makespan_lower_bound"][s]).all()
    both = s & prio["solved"]
    assert (got["sum_of_costs"][both] <= prio["sum_of_costs"][both]).all()
    # a root without a path: some agent has none at all, or none within the horizon
    assert np.array_equal(status == cu.NO_PATH, ((sp < 0) | (sp > T)).any(axis=1))


# ---- the instance tables -----------------------------------------------------------------------------------------------------
def test_instance_tables_hold_what_the_tests_need():
    seen, only_cbs = set(), 0
    for i, (kind, H, W, N, density, T, _m, B, seed) in enumerate(cu.CASES):
        status = cu.restated(i)[2]
        seen |= set(status.tolist())
        grids, pos, goals = cu.case_instances(i)
        prio_solved = (pq.plan_batch(pq.plan_bit_rows, grids, pos, goals, T)[1] >= 0).all(axis=1)
        only_cbs += int(((status == cu.SOLVED) & ~prio_solved).sum())
        if i in cu.CLOSED_LOOP_CASES:
            assert 2 * int((status == cu.SOLVED).sum()) >= B, (cu.CASE_IDS[i], status.tolist())
    assert [(c[1], c[2], c[3]) for c in (cu.CASES[i] for i in cu.CLOSED_LOOP_CASES)] == [(12, 12, 8), (33, 12, 16)]
    assert seen == set(cu.STATUS_NAMES)
    assert only_cbs >= 1
    # the parity table of the GPU test: shape, max_nodes, horizon
    table = [((3, 3, 2), 1, 16), ((3, 3, 2), 8, 16), ((3, 3, 2), 64, 16), ((5, 5, 4), 64, 32), ((12, 12, 8), 64, 64),
             ((12, 33, 8), 32, 96), ((33, 12, 16), 32, 96), ((64, 64, 64), 4, 128), ((11, 12, 2), 8, 128)]
    assert [((c[1], c[2], c[3]), c[6], c[5]) for c in cu.CASES[:len(table)]] == table
    assert cu.CASES[7][7] == 3 and all(c[7] == pq.batch_of(c[1]) for c in cu.CASES[:7])
    # the case whose envs per workgroup LDS limits: 8-byte words of an env as csrc/mapf_engine.h counts them
    _k, H, _W, N, _d, T, M, B, _s = cu.CASES[cu.LDS_CAPPED_CASE]
    words = N * ((T + 5) & ~3) // 4 + ((M + 1) & ~1) * 3 // 2 + ((T + 4) & ~3) // 4
    assert 65536 // (8 * words) == 5 < 64 // pq.group_width(H) == 16 and B > 2 * 5
