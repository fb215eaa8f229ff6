"""Conflict-based search as include/mapf_step.h states it above mapf_plan_cbs, restated twice in plain Python -- once on
sets of cells with every node holding its whole constraint sets and plan, once on bit rows (Python ints) with the node
store as the kernel keeps it: a record per node with its parent, its one constraint, its cost and the replanned agent's
path, joint plans and constraint sets assembled by walking the parent chain, constraints bucketed by time -- the instances
its tests run on (``prioritized_util.instances``), an exhaustive joint-state search that pins optimality on small grids,
and the hand cases that pin what the rule decides.

The rule in one paragraph: a constraint (a, x, t) keeps agent a off cell x at time t.  The low level floods space-time for
one agent under its own constraints only and arrives at the first time its goal is in the set and no later constraint sits
on the goal.  The first conflict of a joint plan is the first in (time, V before O, pair i < k): V, two agents on one cell;
O, the earlier mover enters the cell the later one stands on.  The high level expands the open node of smallest (cost,
id), and each of the two agents of its first conflict is replanned with one more constraint as a child node.
"""

from __future__ import annotations

import functools
import heapq
import itertools

import numpy as np

import prioritized_util as pz

DELTA = pz.DELTA
SOLVED, BUDGET, INFEASIBLE, NO_PATH = 0, 1, 2, 3
STATUS_NAMES = {SOLVED: "SOLVED", BUDGET: "BUDGET", INFEASIBLE: "INFEASIBLE", NO_PATH: "NO_PATH"}


def _cell(x):
    return (int(x[0]), int(x[1]))


def _result(T, N, status, n_nodes, paths=None):
    """(plan int8 [T, N], arrival int32 [N], status, nodes, cells int16 [T + 1, N, 2]); paths[j] = (A, cells 0 .. T)."""
    plan, arrival, cells = np.zeros((T, N), np.int8), np.full(N, -1, np.int32), np.zeros((T + 1, N, 2), np.int16)
    if status == SOLVED:
        for j, (A, c) in enumerate(paths):
            arrival[j] = A
            cells[:, j] = c
            for t in range(T):
                d = (c[t + 1][0] - c[t][0], c[t + 1][1] - c[t][1])
                plan[t, j] = next(a for a in range(5) if DELTA[a] == d)
    return plan, arrival, status, n_nodes, cells


def children_of(conflict):
    """The child constraints (agent, cell, time) of a conflict (kind, i, k, t, x), in order, without those at time 0."""
    kind, i, k, t, x = conflict
    return [c for c in ((i, x, t + 1 if kind == "O" else t), (k, x, t)) if c[2] >= 1]


# ---- 1. on sets ------------------------------------------------------------------------------------------------------
def low_level_sets(grid: np.ndarray, p, g, T: int, cons):
    """One agent under its constraints ``cons`` = {(cell, time)}: (A, [c_0 .. c_T]) or None where the low level fails."""
    H, W = grid.shape
    p, g = _cell(p), _cell(g)
    inside = lambda x: 0 <= x[0] < H and 0 <= x[1] < W
    if not (inside(p) and inside(g)):
        return None
    free = {(r, c) for r in range(H) for c in range(W) if grid[r, c] == 0}
    reach, A = [{p}], -1
    for t in range(T + 1):
        if t > 0:
            grown = {(x[0] + dr, x[1] + dc) for x in reach[t - 1] for dr, dc in DELTA.values()}
            reach.append((grown & free) - {x for x, tc in cons if tc == t})
        if g in reach[t] and not any(x == g and tc >= t for x, tc in cons):
            A = t
            break
        if not reach[t]:
            break
    if A < 0:
        return None
    cells = [g] * (T + 1)
    c = g
    for t in range(A, 0, -1):
        a = next(a for a in range(5) if (c[0] - DELTA[a][0], c[1] - DELTA[a][1]) in reach[t - 1])
        c = (c[0] - DELTA[a][0], c[1] - DELTA[a][1])
        cells[t - 1] = c
    assert c == p
    return A, cells


def first_conflict(cells, T: int):
    """cells[j][t]: (kind, i, k, t, x) of the first conflict, None where the joint plan has none."""
    N = len(cells)
    pairs = list(itertools.combinations(range(N), 2))
    for t in range(T + 1):
        if t >= 1:
            for i, k in pairs:
                if cells[i][t] == cells[k][t]:
                    return ("V", i, k, t, cells[i][t])
        if t <= T - 1:
            for i, k in pairs:
                if cells[i][t + 1] == cells[k][t]:
                    return ("O", i, k, t, cells[k][t])
    return None


def cbs_sets(grid: np.ndarray, positions, goals, T: int, max_nodes: int):
    N = len(positions)
    paths = [low_level_sets(grid, positions[j], goals[j], T, set()) for j in range(N)]
    if any(p is None for p in paths):
        return _result(T, N, NO_PATH, 0)
    nodes = [{"cons": [set() for _ in range(N)], "paths": paths, "cost": sum(p[0] for p in paths)}]
    open_ids = {0}
    while open_ids:
        n = min(open_ids, key=lambda i: (nodes[i]["cost"], i))
        open_ids.remove(n)
        node = nodes[n]
        conflict = first_conflict([p[1] for p in node["paths"]], T)
        if conflict is None:
            return _result(T, N, SOLVED, len(nodes), node["paths"])
        for a, x, t in children_of(conflict):
            if len(nodes) >= max_nodes:
                return _result(T, N, BUDGET, len(nodes))
            cons = [set(c) for c in node["cons"]]
            cons[a].add((x, t))
            path = low_level_sets(grid, positions[a], goals[a], T, cons[a])
            if path is None:
                continue
            new_paths = list(node["paths"])
            new_paths[a] = path
            nodes.append({"cons": cons, "paths": new_paths, "cost": node["cost"] - node["paths"][a][0] + path[0]})
            open_ids.add(len(nodes) - 1)
    return _result(T, N, INFEASIBLE, len(nodes))


# ---- 2. on bit rows, with the node store as the kernel keeps it ------------------------------------------------------
# A path is [c_0 .. c_T, A] with cells as row << 8 | col.  `root` holds the N unconstrained paths; record n holds the path
# of the one agent node n replanned.  info[n] = (parent, agent, time, cell, same): `same` is the nearest ancestor that
# constrains the same agent at the same time (0: none -- node 0 has no constraint).  key[n] = cost << 10 | n while open.
_CLOSED = 0xFFFFFFFF


TRACE_KEYS = ("nodes", "status", "max_expanded", "max_parent", "max_agent", "max_time", "max_row", "max_col", "max_chain",
              "max_same_chain", "max_last", "dropped", "max_last_dropped", "root_conflict_time", "max_conflict_time",
              "solved_node", "solved_chain_agents")


def cbs_bit_rows(grid: np.ndarray, positions, goals, T: int, max_nodes: int, trace: dict | None = None):
    """``trace``, where given, is filled with what the search reached (TRACE_KEYS; -1: nothing of the kind): nodes created
    and the status; the largest node id taken from the open list and the largest that became a parent; the largest
    constrained agent, constraint time, row and column over every child tried; the longest parent chain and ``same`` chain
    (in links) of a child tried; the largest ``last`` handed to a low-level search; how many children were dropped because
    their search failed and the largest ``last`` among them; the time of the root's first conflict and the latest first
    conflict of any node; the solved node and the agents its chain replanned.  The results do not depend on it."""
    H, W = grid.shape
    N = len(positions)
    full = (1 << W) - 1
    free = [full & ~sum(1 << c for c in range(W) if grid[r, c] != 0) for r in range(H)]

    def low_level(a, head, info, last):
        (pr, pc), (gr, gc) = _cell(positions[a]), _cell(goals[a])
        if not (0 <= pr < H and 0 <= pc < W and 0 <= gr < H and 0 <= gc < W) or last >= T:
            return None
        reach = [0] * H
        reach[pr] = 1 << pc
        hist, A = [reach], -1
        if last < 0 and (pr, pc) == (gr, gc):
            A = 0
        t = 0
        while A < 0 and t < T:
            t += 1
            blocked = [0] * H
            e = head[t] if head is not None else 0
            while e:
                cell, e = info[e][3], info[e][4]
                blocked[cell >> 8] |= 1 << (cell & 255)
            reach = [(reach[r] | (reach[r] << 1) | (reach[r] >> 1) | (reach[r - 1] if r > 0 else 0)
                      | (reach[r + 1] if r + 1 < H else 0)) & free[r] & ~blocked[r] for r in range(H)]
            hist.append(reach)
            if (reach[gr] >> gc) & 1 and t > last:
                A = t
            elif not any(reach):
                break
        if A < 0:
            return None
        path = [gr << 8 | gc] * (T + 1) + [A]
        cr, cc = gr, gc
        for t in range(A, 0, -1):
            prev = hist[t - 1]
            cand = [(prev[cr] >> cc) & 1,
                    (prev[cr + 1] >> cc) & 1 if cr + 1 < H else 0,   # came UP from the row below
                    (prev[cr] >> (cc - 1)) & 1 if cc >= 1 else 0,    # came RIGHT from the column before
                    (prev[cr - 1] >> cc) & 1 if cr >= 1 else 0,      # came DOWN from the row above
                    (prev[cr] >> (cc + 1)) & 1]                      # came LEFT from the column after
            a_t = cand.index(1)
            cr, cc = cr - DELTA[a_t][0], cc - DELTA[a_t][1]
            path[t - 1] = cr << 8 | cc
        assert (cr, cc) == _cell(positions[a])
        return path

    tr = dict.fromkeys(TRACE_KEYS, -1)
    tr.update(dropped=0, solved_chain_agents=())

    def result(status, n_nodes, cells=None):
        if trace is not None:
            trace.update(tr, nodes=n_nodes, status=status)
        paths = None
        if status == SOLVED:
            paths = [(cells[j][T + 1], [(c >> 8, c & 255) for c in cells[j][:T + 1]]) for j in range(N)]
        return _result(T, N, status, n_nodes, paths)

    root = [low_level(j, None, None, -1) for j in range(N)]
    if any(p is None for p in root):
        return result(NO_PATH, 0)
    recs = [None] * max_nodes
    info = [(0, 0, 0, 0, 0)] * max_nodes
    key = [_CLOSED] * max_nodes
    key[0] = sum(p[T + 1] for p in root) << 10
    n_nodes = 1
    for _expansion in range(max_nodes + 1):  # (an expansion closes a node, so the last of these returns)
        m = min(key[:n_nodes])
        if m == _CLOSED:
            return result(INFEASIBLE, n_nodes)
        cur, cur_cost = m & 1023, m >> 10
        key[cur] = _CLOSED
        tr["max_expanded"] = max(tr["max_expanded"], cur)
        # the joint plan: of every agent the path of the deepest node of the chain that replanned it, else the root's
        cells, n, depth = [None] * N, cur, 0
        while n:
            if cells[info[n][1]] is None:
                cells[info[n][1]] = recs[n]
            n, depth = info[n][0], depth + 1
        cells = [root[j] if cells[j] is None else cells[j] for j in range(N)]
        # the first conflict: the smallest t << 13 | kind << 12 | i << 6 | k
        conf = None
        for t in range(T + 1):
            best = [kind << 12 | i << 6 | k for i in range(N) for k in range(i + 1, N) for kind in (0, 1)
                    if (kind == 0 and t >= 1 and cells[i][t] == cells[k][t])
                    or (kind == 1 and t <= T - 1 and cells[i][t + 1] == cells[k][t])]
            if best:
                conf = t << 13 | min(best)
                break
        if conf is None:
            tr.update(solved_node=cur, solved_chain_agents=tuple(j for j in range(N) if cells[j] is not root[j]))
            return result(SOLVED, n_nodes, cells)
        t, kind, i, k = conf >> 13, (conf >> 12) & 1, (conf >> 6) & 63, conf & 63
        tr["max_conflict_time"] = max(tr["max_conflict_time"], t)
        if cur == 0:
            tr["root_conflict_time"] = t
        x = cells[k][t]
        for a, ct in ((i, t + kind), (k, t)):
            if ct < 1:
                continue
            if n_nodes >= max_nodes:
                return result(BUDGET, n_nodes)
            gcell = int(goals[a][0]) << 8 | int(goals[a][1])
            head, last, n = [0] * (T + 1), -1, cur
            while n:
                _parent, na, nt, ncell, _same = info[n]
                if na == a:
                    if ncell == gcell:
                        last = max(last, nt)
                    if head[nt] == 0:
                        head[nt] = n
                n = info[n][0]
            if x == gcell:
                last = max(last, ct)
            info[n_nodes] = (cur, a, ct, x, head[ct])  # the child's own entry; it counts once the search succeeds
            head[ct] = n_nodes
            links, e = 0, info[n_nodes][4]
            while e:
                links, e = links + 1, info[e][4]
            for name, v in (("max_agent", a), ("max_time", ct), ("max_row", x >> 8), ("max_col", x & 255), ("max_chain", depth + 1),
                            ("max_same_chain", links), ("max_last", last)):
                tr[name] = max(tr[name], v)
            path = low_level(a, head, info, last)
            if path is None:
                tr["dropped"] += 1
                tr["max_last_dropped"] = max(tr["max_last_dropped"], last)
                continue
            tr["max_parent"] = max(tr["max_parent"], cur)
            recs[n_nodes] = path
            key[n_nodes] = (cur_cost - cells[a][T + 1] + path[T + 1]) << 10 | n_nodes
            n_nodes += 1
    raise AssertionError("more expansions than nodes")


def cbs_batch(fn, grids, positions, goals, T, max_nodes):
    """fn (one of the two restatements) over a batch: (plan [B, T, N], arrival [B, N], status [B], nodes [B],
    cells [B, T + 1, N, 2])."""
    res = [fn(grids[b] if grids.ndim == 3 else grids, positions[b], goals[b], T, max_nodes) for b in range(positions.shape[0])]
    return (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32),
            np.array([r[3] for r in res], np.int32), np.stack([r[4] for r in res]))


# ---- instances: prioritized_util's, with the node budgets of the GPU tests ------------------------------------------------
# (kind, H, W, N, density, horizon, max_nodes, B, seed)
def _case(shape, max_nodes, B=None, seed=0, T=None):
    kind, H, W, N, density, horizon = shape
    return (kind, H, W, N, density, horizon if T is None else T, max_nodes, pz.batch_of(H) if B is None else B, seed)


CASES = [_case(pz.SHAPES[0], 1), _case(pz.SHAPES[0], 8), _case(pz.SHAPES[0], 64), _case(pz.SHAPES[1], 64),
         _case(pz.SHAPES[2], 64), _case(pz.SHAPES[3], 32), _case(pz.SHAPES[4], 32), _case(pz.SHAPES[5], 4, B=3),
         _case(pz.SHAPES[6], 8),
         # horizons short enough for the tree to run out (INFEASIBLE), which the horizons above never are
         _case(pz.SHAPES[0], 64, T=2), _case(pz.SHAPES[1], 64, T=6),
         # the closed-loop shapes with a budget and a seed at which most envs are solved
         _case(pz.SHAPES[2], 256, seed=1), _case(pz.SHAPES[4], 256, seed=20),
         # the largest budget on the narrowest group: the node tables of 5 envs fill a workgroup's 64 KiB of LDS, so 11 of
         # the 16 groups of every wavefront idle and the 47 envs take 10 workgroups
         _case(pz.SHAPES[0], 1024),
         # groups of 32 lanes, two to a wavefront: NO_PATH, SOLVED, SOLVED, BUDGET, SOLVED with 0, 31, 7, 32 and 19 nodes
         _case(pz.SHAPES[7], 32)]
LDS_CAPPED_CASE = 13
CASE_IDS = [f"{k}_{H}x{W}_n{N}_t{T}_m{m}_s{seed}" for k, H, W, N, _d, T, m, _B, seed in CASES]
CLOSED_LOOP_CASES = (11, 12)  # indices into CASES
CHECK_BUILD_CASES = [i for i, c in enumerate(CASES) if c[3] <= 16]  # the checking build holds the step kernels of up to 16 agents


def case_instances(i: int):
    kind, H, W, N, density, _T, _m, B, seed = CASES[i]
    return pz.instances(kind, H, W, N, density, B, seed)


@functools.lru_cache(maxsize=None)
def restated(i: int):
    """The bit-row restatement over a case's instances, computed once: (plan, arrival, status, nodes, cells), read-only."""
    grids, pos, goals = case_instances(i)
    out = cbs_batch(cbs_bit_rows, grids, pos, goals, CASES[i][5], CASES[i][6])
    for a in out:
        a.setflags(write=False)
    return out


# ---- the far ends of the packed fields: a second table, from literals ------------------------------------------------------
# MAPF_CBS_MAX_NODES = 1024 and MAPF_CBS_MAX_HORIZON = 128 are where the widths of the kernel's packed fields run out (node
# id and parent 10 bits, agent 6, time 8, cell 16, `same` 10, key cost << 10 | id, conflict t << 13 | kind << 12 | i << 6 | k,
# the 64-bit mask of filled agents); CASES above comes near none of them.  An env is a reference into
# ``prioritized_util.instances`` -- an instance depends on (seed, env) only, not on the batch it is drawn in -- or a grid with
# positions and goals; the envs of a table share (H, W, N), a horizon and a budget.  Every table names the conditions it
# exists for as (what, predicate over the traces of its envs): test_cbs_host asserts them on the restatement's trace alone, so
# a table cannot silently stop reaching its end when a generator changes.
def _ref(H, W, N, density, seed, env):
    return ("ref", "random", H, W, N, density, seed, env)


def _env(grid, positions, goals):
    return ("grid", grid, np.array(positions, np.int16), np.array(goals, np.int16))


def _solved(t):
    return t["status"] == SOLVED


def _any(pred):
    return lambda traces: any(pred(t) for t in traces)


def _count(pred, n):
    return lambda traces: sum(1 for t in traces if pred(t)) >= n


_D12 = (12, 12, 8, 0.2)   # G = 16: four envs per wavefront, and four fit a workgroup's LDS at M = 1024
_D8 = (8, 8, 8, 0.1)      # G = 8: eight envs per wavefront, of which five fit a workgroup's LDS at M = 1024
# the 2 x 2 block left of a wall, with a walled-off column so that the engine finds its two free cells per agent: the search
# is the open 2 x 2 grid's (test_cbs_host compares the two)
BLOCK_2X2 = pz._grid("..#.",
                     "..#.")
_ROTATE = ([(0, 0), (0, 1), (1, 0)], [(0, 1), (0, 0), (1, 0)])  # agents 0 and 1 swap in a 2 x 2 block, agent 2 holds the third cell
OPEN64, OPEN4X64, OPEN12 = np.zeros((64, 64), np.uint8), np.zeros((4, 64), np.uint8), np.zeros((12, 12), np.uint8)
WALLED64 = OPEN64.copy()          # row 0 is a corridor that opens at column 0 only: from (0, s) every cell of row 63 is
WALLED64[1, 1:] = 1               # s steps further than its Manhattan distance from (0, 0)
# row 0 a corridor that opens at column 63 only, and a wall above-left of the far corner: the agent from (1, 0) walks down
# column 0 and along row 63 and enters its goal (63, 63) at 125; the agent from (0, 2), 124 steps from that corner down column
# 63, stands on it at 124 and steps on to its own goal (63, 62) as the first leaves that -- an O conflict at 124 whose child
# for the first agent sits on that agent's goal at time 125
END_SWAP64 = OPEN64.copy()
END_SWAP64[1, 1:63] = 1
END_SWAP64[62, 62] = END_SWAP64[0, 0] = 1
_END_SWAP = _env(END_SWAP64, [(1, 0), (0, 2)], [(63, 63), (63, 62)])
# two regions that meet on row 63 only, each cut by a wall that opens at row 0, so both agents walk up, across and down: the
# agent from (33, 0) is 128 steps from its goal (63, 32) and enters it from the left; the agent from (33, 63) is 127 steps from
# that cell, enters it from above and steps on to its own goal (63, 33), a pocket behind it.  The O conflict at 127 has a child
# at time 128 = T, on the first agent's goal, and one that makes the second agent late: neither is made
LAST_STEP64 = OPEN64.copy()
LAST_STEP64[0:63, 31] = LAST_STEP64[1:64, 15] = LAST_STEP64[1:64, 48] = 1
LAST_STEP64[62, 33] = LAST_STEP64[63, 34] = 1
_LAST_STEP = _env(LAST_STEP64, [(33, 0), (33, 63)], [(63, 32), (63, 33)])
_FAR_PARKED = _env(OPEN64, [(0, 0), (63, 62)], [(63, 63), (63, 62)])
_PARK12 = [(r, c) for r in range(5) for c in range(12)]
_PARK64 = [(0, c) for c in range(60)]


def _limit(name, envs, T, max_nodes, conditions, mask_out=()):
    return {"name": name, "envs": envs, "T": T, "max_nodes": max_nodes, "conditions": conditions, "mask_out": mask_out}


LIMIT_CASES = [
    # wavefront 0 holds a deep solved env (876 nodes), one that spends the budget, one solved at the root and another deep one
    # (573); wavefront 1 the third deep one (635) between two that spend the budget; the last is ragged, with a root that fails
    _limit("deep_12x12_n8_t64_m1024",
           [_ref(*_D12, 6, 4), _ref(*_D12, 0, 1), _ref(*_D12, 2, 7), _ref(*_D12, 8, 8),
            _ref(*_D12, 9, 3), _ref(*_D12, 0, 3), _ref(*_D12, 0, 2), _ref(*_D12, 0, 4),
            _ref(*_D12, 0, 10), _ref(*_D12, 0, 0), _ref(*_D12, 0, 5)], 64, 1024,
           [("two solved envs above 512 nodes with a parent id >= 512", _count(lambda t: _solved(t) and t["nodes"] > 512 and t["max_parent"] >= 512, 2)),
            ("a third solved env above 512 nodes", _count(lambda t: _solved(t) and t["nodes"] > 512, 3)),
            ("an env at BUDGET with exactly 1024 nodes", _any(lambda t: t["status"] == BUDGET and t["nodes"] == 1024)),
            ("a `same` chain of 5 links or more", _any(lambda t: t["max_same_chain"] >= 5)),
            ("wavefront 0 mixes deep, BUDGET and root-solved", lambda tr: _solved(tr[0]) and tr[0]["nodes"] > 512 and tr[1]["status"] == BUDGET
             and _solved(tr[2]) and tr[2]["nodes"] == 1 and _solved(tr[3]) and tr[3]["nodes"] > 512),
            ("a root that fails in the last wavefront", lambda tr: tr[9]["status"] == NO_PATH)],
           mask_out=(1, 10)),  # the second run takes the BUDGET env out of wavefront 0 (and one out of the last)
    # five envs fill a workgroup's LDS: workgroups 0 and 1 hold two envs each that spend the budget, in groups 1, 3 and 2, 4
    _limit("deep_8x8_n8_t32_m1024_lds_capped",
           [_ref(*_D8, 0, 0), _ref(*_D8, 0, 4), _ref(*_D8, 0, 2), _ref(*_D8, 1, 5), _ref(*_D8, 0, 3),
            _ref(*_D8, 0, 5), _ref(*_D8, 0, 9), _ref(*_D8, 2, 1), _ref(*_D8, 0, 12), _ref(*_D8, 2, 6),
            _ref(*_D8, 0, 13), _ref(*_D8, 0, 15)], 32, 1024,
           [("four envs at BUDGET with 1024 nodes and a parent id above 640", _count(lambda t: t["status"] == BUDGET and t["nodes"] == 1024 and t["max_parent"] > 640, 4)),
            ("a parent id above 800", _any(lambda t: t["max_parent"] > 800)),
            ("the deep envs are 1, 3, 7, 9 and the rest is shallow", lambda tr: [b for b, t in enumerate(tr) if t["nodes"] > 64] == [1, 3, 7, 9])]),
    # G = 4, sixteen groups per wavefront
    _limit("block_2x2_n3_t4_exhausted",
           [_env(BLOCK_2X2, *_ROTATE), _env(BLOCK_2X2, [(0, 0), (0, 1), (1, 0)], [(0, 0), (0, 1), (1, 1)]),
            _env(BLOCK_2X2, [(1, 0), (0, 0), (0, 1)], [(1, 0), (0, 1), (0, 0)])], 4, 1024,
           [("an exhausted tree of more than 100 nodes", _any(lambda t: t["status"] == INFEASIBLE and t["nodes"] > 100)),
            ("more than 100 dropped children, one with last = T", _any(lambda t: t["dropped"] > 100 and t["max_last_dropped"] == 4))]),
    _limit("block_2x2_n3_t5_m1024",
           [_env(BLOCK_2X2, *_ROTATE), _env(BLOCK_2X2, [(0, 0), (0, 1), (1, 0)], [(0, 0), (0, 1), (1, 1)]),
            _env(BLOCK_2X2, [(1, 0), (0, 0), (0, 1)], [(1, 0), (0, 1), (0, 0)])], 5, 1024,
           [("BUDGET at 1024 nodes with a parent id >= 990", _any(lambda t: t["status"] == BUDGET and t["nodes"] == 1024 and t["max_parent"] >= 990))]),
    _limit("line4_head_on_t6_exhausted",
           [_env(pz.DEAD_END, [(0, 0), (0, 3)], [(0, 3), (0, 0)]), _env(pz.DEAD_END, [(0, 0), (0, 3)], [(0, 1), (0, 0)])], 6, 1024,
           [("the head-on tree is exhausted after 65 nodes", lambda tr: (tr[0]["status"], tr[0]["nodes"]) == (INFEASIBLE, 65))]),
    # G = 64, one env per wavefront: constraints and arrivals at the end of the 8 bits of a time
    _limit("late_64x64_n2_t128",
           [_FAR_PARKED,                                                                  # constraint at 125, arrival 126
            _env(OPEN64, [(0, 0), (63, 63)], [(63, 63), (0, 0)]),                         # the corner swap: both arrive at 126
            _env(WALLED64, [(0, 1), (63, 62)], [(63, 63), (63, 62)]),                     # constraint at 126, arrival 127
            _env(WALLED64, [(0, 2), (63, 62)], [(63, 63), (63, 62)]),                     # constraint at 127, arrival 128 = T
            _END_SWAP,                                                                    # the goal constrained at 125, a return at 126
            _LAST_STEP],                                                                  # a constraint at 128 = T
           128, 64,
           [("the first five envs are solved with more than the root", lambda tr: all(_solved(t) and t["nodes"] > 1 for t in tr[:5])),
            ("a constraint at time 128 on the agent's goal: both children dropped, one with last = T", lambda tr: (tr[5]["status"], tr[5]["nodes"],
             tr[5]["max_time"], tr[5]["dropped"], tr[5]["max_last_dropped"]) == (INFEASIBLE, 1, 128, 2, 128)),
            ("constraint times 125, 126 and 127", lambda tr: [t["max_time"] for t in tr[:1] + tr[2:4]] == [125, 126, 127]),
            ("arrivals at 126 need row 63 and column 0 constrained at 63", lambda tr: (tr[1]["max_time"], tr[1]["max_row"], tr[1]["max_col"]) == (63, 63, 0)),
            ("last >= 125 in a solved env, with a return after it", _any(lambda t: _solved(t) and t["max_last"] >= 125 and t["dropped"] == 0)),
            ("an agent constrained on its own goal at 125, and replanned in the solved chain", lambda tr: tr[4]["max_last"] == 125 and tr[4]["solved_chain_agents"] == (0,))]),
    # the horizon equal to that `last`: neither child of the root is made, the tree is the root
    _limit("late_64x64_n2_t125_last_is_the_horizon", [_END_SWAP, _FAR_PARKED], 125, 64,
           [("both children dropped, one with last = T = 125", lambda tr: (tr[0]["status"], tr[0]["nodes"], tr[0]["dropped"], tr[0]["max_last_dropped"]) == (INFEASIBLE, 1, 2, 125)),
            ("a root that fails by one step", lambda tr: tr[1]["status"] == NO_PATH)]),
    # G = 4: the first conflict lies in chunk 15 of the conflict scan
    _limit("late_4x64_n2_t128",
           [_env(OPEN4X64, [(0, 0), (0, 63)], [(0, 63), (0, 62)]), _env(OPEN4X64, [(0, 0), (0, 62)], [(0, 63), (0, 62)]),
            _env(OPEN4X64, [(0, 0), (0, 63)], [(0, 63), (0, 0)])], 128, 64,
           [("a first conflict at 60 or later in a solved env", _count(lambda t: _solved(t) and t["nodes"] > 1 and t["root_conflict_time"] >= 60, 2))]),
    # 64 agents, solved: 62 stand on their goals, the last two move
    _limit("n64_12x12_t32",
           [_env(OPEN12, _PARK12 + [(5, 0), (5, 1), (8, 0), (8, 11)], _PARK12 + [(5, 0), (5, 1), (8, 11), (8, 0)]),       # 62 and 63 swap along row 8
            _env(OPEN12, _PARK12 + [(7, 5), (10, 5), (6, 0), (9, 0)], _PARK12 + [(7, 5), (10, 5), (7, 11), (10, 11)])],   # each walks into a parked agent
           32, 64,
           [("solved with more than one node and agent 63 constrained", lambda tr: all(_solved(t) and t["nodes"] > 1 and t["max_agent"] == 63 for t in tr)),
            ("agents 62 and 63 both replanned in the solved node's chain", _any(lambda t: t["solved_chain_agents"] == (62, 63)))]),
    _limit("n64_64x64_t128",
           [_env(OPEN64, _PARK64 + [(0, 60), (0, 61), (1, 0), (63, 62)], _PARK64 + [(0, 60), (0, 61), (63, 63), (63, 62)]),
            _env(OPEN64, _PARK64 + [(41, 20), (63, 62), (1, 0), (1, 5)], _PARK64 + [(41, 20), (63, 62), (63, 63), (41, 45)])],
           128, 16,
           [("solved with more than one node and agent 63 constrained", lambda tr: all(_solved(t) and t["nodes"] > 1 and t["max_agent"] == 63 for t in tr)),
            ("a constraint at 124 and an arrival at 125", lambda tr: all(t["max_time"] == 124 for t in tr)),
            ("agents 62 and 63 both replanned in the solved node's chain", _any(lambda t: t["solved_chain_agents"] == (62, 63)))]),
]
LIMIT_IDS = [c["name"] for c in LIMIT_CASES]
LIMIT_DEEP, LIMIT_LDS_CAPPED, LIMIT_LATE = 0, 1, 5  # indices into LIMIT_CASES
LIMIT_CLOSED_LOOP = (LIMIT_DEEP, LIMIT_LATE)
# the nodes the deep solved envs end at, and the latest arrival of the late table (the closed loop steps these plans)
LIMIT_DEEP_SOLVED_NODES = (876, 635, 573)


@functools.lru_cache(maxsize=None)
def limit_instances(i: int):
    """(grids uint8 [B, H, W], positions int16 [B, N, 2], goals int16 [B, N, 2]) of a limit table, read-only."""
    grids, pos, goals = [], [], []
    for e in LIMIT_CASES[i]["envs"]:
        if e[0] == "ref":
            _tag, kind, H, W, N, density, seed, env = e
            g, p, q = pz.instances(kind, H, W, N, density, (env | 15) + 1, seed)
            g, p, q = g[env], p[env], q[env]
        else:
            _tag, g, p, q = e
        grids.append(g)
        pos.append(p)
        goals.append(q)
    out = (np.stack(grids).astype(np.uint8), np.stack(pos).astype(np.int16), np.stack(goals).astype(np.int16))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def limit_restated(i: int):
    """The bit-row restatement over a limit table, computed once: (plan, arrival, status, nodes, cells) read-only, and the
    traces of its envs."""
    grids, pos, goals = limit_instances(i)
    traces = [{} for _ in range(len(pos))]
    res = [cbs_bit_rows(grids[b], pos[b], goals[b], LIMIT_CASES[i]["T"], LIMIT_CASES[i]["max_nodes"], traces[b]) for b in range(len(pos))]
    out = (np.stack([r[0] for r in res]), np.stack([r[1] for r in res]), np.array([r[2] for r in res], np.int32),
           np.array([r[3] for r in res], np.int32), np.stack([r[4] for r in res]))
    for a in out:
        a.setflags(write=False)
    return out + (traces,)


# ---- mutants of the bit-row restatement: what a kernel with a field one bit short would compute ---------------------------
# (name, [(text of cbs_bit_rows, its replacement)]); every text occurs exactly once.  A mutant that loops is stopped by the
# bound on the expansions and raises.
MUTATIONS = {
    "node id masked with 511": [("cur, cur_cost = m & 1023, m >> 10", "cur, cur_cost = m & 511, m >> 10"),
                                ("            n, depth = info[n][0], depth + 1", "            n, depth = info[n][0] & 511, depth + 1"),
                                ("                n = info[n][0]\n", "                n = info[n][0] & 511\n")],
    "time masked with 127": [("            if n_nodes >= max_nodes:\n", "            ct &= 127\n            if n_nodes >= max_nodes:\n")],
    "agent masked with 31": [("(conf >> 6) & 63, conf & 63", "(conf >> 6) & 31, conf & 31")],
    "same ignored beyond the first link": [("cell, e = info[e][3], info[e][4]", "cell, e = info[e][3], 0")],
    "the goal constraint last ignored": [("path = low_level(a, head, info, last)", "path = low_level(a, head, info, -1)")],
}


@functools.lru_cache(maxsize=None)
def mutant(name: str):
    import inspect

    src = inspect.getsource(cbs_bit_rows)
    for old, new in MUTATIONS[name]:
        assert src.count(old) == 1, (name, old, src.count(old))
        src = src.replace(old, new)
    scope = dict(globals())
    exec(compile(src, f"<cbs_bit_rows: {name}>", "exec"), scope)
    return scope["cbs_bit_rows"]


def same_result(a, b) -> bool:
    """Two results of a restatement: plan, arrival, status and nodes."""
    return a[2] == b[2] and a[3] == b[3] and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the optimum by exhaustive search: Dijkstra over (cells, parked set) under the env's move phase -------------------
def moves(free, cells, actions):
    """``prioritized_util.simulate_moves`` on tuples (free: set of cells; an agent whose move fails stays)."""
    pos = list(cells)
    for i, a in enumerate(actions):
        if a:
            t = (pos[i][0] + DELTA[a][0], pos[i][1] + DELTA[a][1])
            if t in free and t not in pos:
                pos[i] = t
    return tuple(pos)


def optimal_sum_of_costs(grid: np.ndarray, positions, goals, T: int):
    """The least sum over agents of the step after which the agent is parked on its goal, over every way to play at most T
    steps; a parked agent never moves again and a step costs the number of agents not yet parked.  -1: none."""
    H, W = grid.shape
    N = len(positions)
    free = {(r, c) for r in range(H) for c in range(W) if grid[r, c] == 0}
    start, goal = tuple(_cell(x) for x in positions), tuple(_cell(x) for x in goals)

    def park_options(cells, parked):
        on = [j for j in range(N) if j not in parked and cells[j] == goal[j]]
        return [parked | frozenset(s) for n in range(len(on) + 1) for s in itertools.combinations(on, n)]

    best = {}
    heap = [(0, 0, start, p) for p in park_options(start, frozenset())]
    while heap:
        cost, t, cells, parked = heapq.heappop(heap)
        if len(parked) == N:
            return cost
        if best.get((cells, parked, t), 1 << 30) < cost or t == T:
            continue
        step_cost = N - len(parked)
        for acts in itertools.product(*[(0,) if j in parked else range(5) for j in range(N)]):
            nxt = moves(free, cells, acts)
            for p in park_options(nxt, parked):
                k = (nxt, p, t + 1)
                if cost + step_cost < best.get(k, 1 << 30):
                    best[k] = cost + step_cost
                    heapq.heappush(heap, (cost + step_cost, t + 1, nxt, p))
    return -1


# ---- hand cases: one property each -----------------------------------------------------------------------------------
_grid = pz._grid

POCKET_LEFT = _grid("#.###",
                    ".....")        # a corridor (row 1) with one pocket above its second cell
TWO_ROWS = _grid("...",
                 "...")
WALLED = _grid("..#..")           # (the engine wants two free cells per agent: both grids have four)
TWO_CELLS = _grid("..#..")        # a dead end of two cells left of the wall


def _hand(name, grid, positions, goals, T, max_nodes, status, nodes, arrival=None, cells=None):
    """arrival: the expected A_j (SOLVED only); cells: {agent: its cells from time 0 on (the rest is the goal)}."""
    return {"name": name, "grid": grid, "positions": np.array(positions, np.int16), "goals": np.array(goals, np.int16),
            "T": T, "max_nodes": max_nodes, "status": status, "nodes": nodes, "arrival": arrival, "cells": cells or {}}


HAND_CASES = [
    # head-on in a corridor whose only pocket lies next to the EARLIER agent's start: agent 1 cannot reach it in time, so
    # plan_prioritized, which lets agent 0 walk straight through, fails agent 1.  The optimum: agent 0 steps to the pocket's
    # mouth and up, agent 1 walks its four cells without a wait (it enters the mouth at time 3, after 0 left it at time 2).
    # Agent 0 moves first within a step, so at step 4 agent 1 still stands on the mouth: 0 comes down at time 5, when the
    # mouth is empty, and walks its three cells: 0 arrives at 8, 1 at 4.  Arrivals and path are derived by hand; the node count, 60, is NOT: it
    # is what both restatements count, recorded here so that the kernel's expansion order is held to theirs
    _hand("head_on_earlier_agent_steps_aside", POCKET_LEFT, [(1, 0), (1, 4)], [(1, 4), (1, 0)], 12, 256, SOLVED, 60,
          arrival=[8, 4], cells={0: [(1, 0), (1, 1), (0, 1), (0, 1), (0, 1), (1, 1), (1, 2), (1, 3), (1, 4)]}),
    # agent 1 stands where agent 0 enters at time 1: an O conflict at t = 0.  Its second constraint would sit at time 0 and
    # makes no child, so the root has ONE child -- agent 0 waits once, agent 1 is gone by then -- and two nodes exist
    _hand("o_conflict_at_time_0_has_one_child", TWO_ROWS, [(0, 0), (0, 1)], [(0, 2), (1, 1)], 8, 64, SOLVED, 2,
          arrival=[3, 1], cells={0: [(0, 0), (0, 0), (0, 1), (0, 2)]}),
    # agent 0 parks on its goal (1, 2) at time 1, agent 1 crosses that cell at time 2: V at t = 2.  Node 1 constrains agent 0
    # there AFTER its arrival, which moves the arrival to 3 (HAND_LOW_LEVEL below); node 2 makes
    # agent 1 wait, which only moves the conflict.  Coming down at time 3 agent 0, the earlier mover, would enter the cell
    # agent 1 still stands on, so it waits once more: it arrives at 4, agent 1 passes under the pocket without a wait
    # (arrivals and path are derived by hand; the node count, 20, is what both restatements count, recorded)
    _hand("constraint_on_the_goal_after_arrival_delays_it", pz.POCKET_MID, [(1, 1), (1, 0)], [(1, 2), (1, 4)], 10, 64, SOLVED, 20,
          arrival=[4, 4], cells={0: [(1, 1), (1, 2), (0, 2), (0, 2), (1, 2)]}),
    # prioritized_util's parked_goal_cuts_the_corridor: no plan exists, every node has a conflict, and the tree of waits
    # within 10 steps is far larger than 64 nodes
    _hand("parked_goal_cuts_the_corridor_ends_in_budget", pz.DEAD_END, [(0, 0), (0, 3)], [(0, 1), (0, 0)], 10, 64, BUDGET, 64),
    # the goal lies behind a wall: the root's low level fails, no node is created
    _hand("goal_behind_walls_is_no_path", WALLED, [(0, 0), (0, 4)], [(0, 3), (0, 1)], 8, 64, NO_PATH, 0),
    # two agents that must swap in a two-cell dead end, horizon 2.  Root: O at t = 0 (agent 0 enters agent 1's cell), one
    # child.  Node 1, agent 0 waits once (cost 3): V at t = 1 on (0, 0); agent 0 kept off both cells at time 1 fails, agent 1
    # kept off (0, 0) at time 1 waits once (node 2, cost 4).  Node 2: O at t = 1; agent 0 kept off its goal at time 2 = T
    # fails, agent 1 kept off both cells at time 1 fails.  The open list is empty after 3 nodes
    _hand("two_cell_dead_end_is_infeasible", TWO_CELLS, [(0, 0), (0, 1)], [(0, 1), (0, 0)], 2, 64, INFEASIBLE, 3),
    # max_nodes = 1 solves exactly the roots without a conflict: following is none ...
    _hand("one_node_solves_a_conflict_free_root", pz.LINE5, [(0, 1), (0, 0)], [(0, 4), (0, 3)], 8, 1, SOLVED, 1, arrival=[3, 3]),
    # ... head-on is one
    _hand("one_node_is_budget_at_the_first_conflict", POCKET_LEFT, [(1, 0), (1, 4)], [(1, 4), (1, 0)], 12, 1, BUDGET, 1),
    # paths that cross at (1, 1) at time 1: both children cost 5.  Node 1 (agent 0 waits) is taken first by its id, but
    # agent 0 then enters the cell agent 1 stands on at time 1 (O): two more nodes of cost 6.  Node 2 (agent 1 waits, and
    # follows agent 0 into the cell it leaves) is next and has no conflict: 5 nodes, not 3
    _hand("equal_costs_are_taken_in_node_order", pz.OPEN3, [(0, 1), (1, 0)], [(2, 1), (1, 2)], 8, 64, SOLVED, 5,
          arrival=[2, 3], cells={1: [(1, 0), (1, 0), (1, 1), (1, 2)]}),
]

# the low level alone, under the one constraint of the case above: kept off its goal (1, 2) at time 2 -- after its first
# arrival at time 1 -- the agent arrives at 3; the walk back takes the lowest action id, the wait, so it waits twice on its
# start and then steps onto the goal
HAND_LOW_LEVEL = {"grid": pz.POCKET_MID, "p": (1, 1), "g": (1, 2), "T": 10, "cons": {((1, 2), 2)},
                  "arrival": 3, "cells": [(1, 1), (1, 1), (1, 1), (1, 2)]}
