"""Conflict-based search without a GPU: the C ABI declares it; the two restatements of its rule (cbs_util: on sets, on bit
rows with the kernel's node store) agree; every solved plan executes under the restated move phase and on the CPU oracle of
the env without a failed move, so the rule is pinned against the env itself and not against the kernel; the hand cases hold
what the rule decides; the sum of costs is the optimum of an exhaustive joint-state search, never above the prioritised
planner's and never below the shortest-path bound; the instance tables hold what the GPU tests need of them; and the limit
tables (cbs_util.LIMIT_CASES) reach the far ends of the kernel's packed fields: every condition a table names holds on the
restatement's trace, and restatements with a field one bit short differ on them."""

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
    # the case whose envs per workgroup LDS limits: 8-byte words of an env as csrc/mapf_plan.hip counts them
    _k, H, _W, N, _d, T, M, B, _s = cu.CASES[cu.LDS_CAPPED_CASE]
    words = N * ((T + 5) & ~3) // 4 + ((M + 1) & ~1) * 3 // 2 + ((T + 4) & ~3) // 4
    assert 65536 // (8 * words) == 5 < 64 // pq.group_width(H) == 16 and B > 2 * 5


# ---- the limit tables: the far ends of the packed fields ---------------------------------------------------------------------
def test_the_trace_changes_no_result():
    for i in (2, 4, 7):  # exhausted trees, a dropped child at the horizon, the narrowest group
        grids, pos, goals = cu.limit_instances(i)
        want = cu.limit_restated(i)
        for b in range(len(pos)):
            got = cu.cbs_bit_rows(grids[b], pos[b], goals[b], cu.LIMIT_CASES[i]["T"], cu.LIMIT_CASES[i]["max_nodes"])
            assert cu.same_result(got, [w[b] for w in want[:4]]) and np.array_equal(got[4], want[4][b]), (i, b)
        assert all(set(t) == set(cu.TRACE_KEYS) for t in want[5])


@pytest.mark.parametrize("i", range(len(cu.LIMIT_CASES)), ids=cu.LIMIT_IDS)
def test_limit_tables_reach_their_ends(i):
    """Every condition a table exists for, on the restatement's trace alone."""
    case = cu.LIMIT_CASES[i]
    grids, pos, goals = cu.limit_instances(i)
    _plan, _arrival, status, nodes, _cells, traces = cu.limit_restated(i)
    assert grids.shape[0] == pos.shape[0] == goals.shape[0] == len(case["envs"]) and pos.shape == goals.shape
    assert 1 <= case["T"] <= 128 and 1 <= case["max_nodes"] <= 1024 and case["conditions"]
    for b in range(len(pos)):  # what the engine asks of a state: two free cells per agent, agents and goals on distinct free cells
        assert int((grids[b] == 0).sum()) >= 2 * pos.shape[1], b
        for cells in (pos[b], goals[b]):
            assert len({tuple(c) for c in cells.tolist()}) == len(cells) and all(grids[b][tuple(c)] == 0 for c in cells.tolist()), b
    for what, holds in case["conditions"]:
        assert holds(traces), f"{case['name']}: {what}: {[(cu.STATUS_NAMES[t['status']], t['nodes']) for t in traces]}"
    assert [t["status"] for t in traces] == status.tolist() and [t["nodes"] for t in traces] == nodes.tolist()
    assert all(b < len(pos) for b in case["mask_out"])


def test_limit_tables_cover_every_group_width_and_the_lds_cap():
    widths = {pq.group_width(cu.limit_instances(i)[0].shape[1]) for i in range(len(cu.LIMIT_CASES))}
    assert widths == {4, 8, 16, 64}
    assert {cu.limit_instances(i)[1].shape[1] for i in range(len(cu.LIMIT_CASES))} >= {2, 3, 8, 64}

    def envs_per_workgroup(i):  # 8-byte words of an env as csrc/mapf_plan.hip counts them (cbs_env_words)
        H, N, T, M = cu.limit_instances(i)[0].shape[1], cu.limit_instances(i)[1].shape[1], cu.LIMIT_CASES[i]["T"], cu.LIMIT_CASES[i]["max_nodes"]
        words = N * ((T + 5) & ~3) // 4 + ((M + 1) & ~1) * 3 // 2 + ((T + 4) & ~3) // 4
        return min(64 // pq.group_width(H), 65536 // (8 * words)), 64 // pq.group_width(H)

    # the deep table fills its wavefronts; the capped one leaves three groups of every wavefront idle, its deep envs lie in two
    # workgroups and in none of them in group 0, and the batch is more than two workgroups' share
    assert envs_per_workgroup(cu.LIMIT_DEEP) == (4, 4)
    epw, per_wave = envs_per_workgroup(cu.LIMIT_LDS_CAPPED)
    assert (epw, per_wave) == (5, 8)
    nodes = cu.limit_restated(cu.LIMIT_LDS_CAPPED)[3]
    deep = np.flatnonzero(nodes == 1024)
    assert len(deep) == 4 and (deep % epw != 0).all() and len(set((deep // epw).tolist())) == 2 and len(nodes) > 2 * epw
    # the walled-off column changes nothing: the search on the block is the open 2 x 2 grid's
    for i in (2, 3):
        grids, pos, goals = cu.limit_instances(i)
        want = cu.limit_restated(i)
        for b in range(len(pos)):
            got = cu.cbs_bit_rows(np.zeros((2, 2), np.uint8), pos[b], goals[b], cu.LIMIT_CASES[i]["T"], cu.LIMIT_CASES[i]["max_nodes"])
            assert cu.same_result(got, [w[b] for w in want[:4]]), (i, b)
    # the closed loop of the GPU test steps the deep solved plans and the late ones
    status, nodes = cu.limit_restated(cu.LIMIT_DEEP)[2:4]
    assert sorted(nodes[(status == cu.SOLVED) & (nodes > 512)].tolist(), reverse=True) == list(cu.LIMIT_DEEP_SOLVED_NODES)
    arrival, status = cu.limit_restated(cu.LIMIT_LATE)[1:3]
    assert sorted(arrival[status == cu.SOLVED].max(axis=1).tolist()) == [126, 126, 126, 127, 128]


@pytest.mark.parametrize("i", range(len(cu.LIMIT_CASES)), ids=cu.LIMIT_IDS)
def test_the_two_restatements_agree_on_the_limit_tables(i):
    """The set-based restatement keeps whole constraint sets and plans per node -- no ids, no links, no packed times -- and
    runs every env at the table's full budget: none needs a reduced one (the slowest envs, 64 x 64 at horizon 128, take it two
to three seconds each, a 12 x 12 env of 1024 nodes about one)."""
    case = cu.LIMIT_CASES[i]
    grids, pos, goals = cu.limit_instances(i)
    plan, arrival, status, nodes, cells, _traces = cu.limit_restated(i)
    for b in range(len(pos)):
        p2, a2, s2, n2, c2 = cu.cbs_sets(grids[b], pos[b], goals[b], case["T"], case["max_nodes"])
        assert (status[b], nodes[b]) == (s2, n2), (b, status[b], nodes[b], s2, n2)
        assert np.array_equal(arrival[b], a2) and np.array_equal(plan[b], p2) and np.array_equal(cells[b], c2), b


@pytest.mark.parametrize("i", range(len(cu.LIMIT_CASES)), ids=cu.LIMIT_IDS)
def test_limit_solved_plans_execute_on_the_oracle_without_a_failed_move(i):
    T = cu.LIMIT_CASES[i]["T"]
    grids, pos, goals = cu.limit_instances(i)
    plan, arrival, status, _nodes, cells, _traces = cu.limit_restated(i)
    for b in np.flatnonzero(status == cu.SOLVED):
        N = pos.shape[1]
        assert cu.first_conflict([[tuple(c) for c in cells[b, :, j]] for j in range(N)], T) is None
        p = pos[b]
        for t in range(1, int(arrival[b].max()) + 1):
            p, failed = pq.simulate_moves(grids[b], p, plan[b, t - 1])
            assert not failed.any() and np.array_equal(p, cells[b, t]), (b, t)
        done_at = _execute_on_oracle(grids[b], pos[b], goals[b], plan[b], cells[b], T)
        want = pq.first_all_on_goal(cells[b], goals[b])
        assert done_at == want and want <= max(int(arrival[b].max()), 1), (b, done_at, want)


def _first_difference(fn, tables):
    """The first (table, env) on which ``fn`` differs from the unmutated restatement (a mutant that raises differs)."""
    for name, insts, want, T, M in tables:
        grids, pos, goals = insts
        for b in range(len(pos)):
            try:
                same = cu.same_result(fn(grids[b] if grids.ndim == 3 else grids, pos[b], goals[b], T, M), [w[b] for w in want[:4]])
            except (AssertionError, IndexError, ValueError):
                same = False
            if not same:
                return name, b
    return None


@pytest.mark.parametrize("name", list(cu.MUTATIONS), ids=[n.replace(" ", "_") for n in cu.MUTATIONS])
def test_a_restatement_with_a_field_one_bit_short_differs_on_a_limit_table(name):
    """Copies of cbs_bit_rows with one field cut down -- what a kernel that masked the node id with 511, dropped bit 7 of a
    time, shifted the mask of filled agents as 32 bits, followed `same` once, or forgot `last` would compute -- each differ
    from the restatement on some limit table, so parity on those tables pins the field.  Only the Python restatement is ever
    mutated.  Recorded, not asserted: over all of CASES the node id, time and agent mutants equal the restatement on every
    env (the tables never reach those bits); the `same` and `last` mutants differ on 27 and 26 of their envs, first on
    random_3x3_n2_t16_m8_s0.  On the limit tables the node id mutant differs on the 876- and 573-node envs of the deep
    table, the time mutant on the env whose constraint sits at time 128, the agent mutant on all four 64-agent envs."""
    fn = cu.mutant(name)
    tables = [(c["name"], cu.limit_instances(i), cu.limit_restated(i), c["T"], c["max_nodes"]) for i, c in enumerate(cu.LIMIT_CASES)]
    assert _first_difference(fn, tables) is not None, f"no limit table notices: {name}"
    # (the unmutated text compiled the same way equals the restatement: the harness itself changes nothing)
    cu.MUTATIONS["none"] = []
    try:
        assert _first_difference(cu.mutant("none"), tables[2:5]) is None
    finally:
        del cu.MUTATIONS["none"]
