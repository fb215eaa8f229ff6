"""The prioritised planner's rule (include/mapf_step.h above mapf_plan_prioritized) restated twice in plain Python -- once
on sets of cells per time step, once on bit rows (Python ints), the form the kernel runs -- the instances its tests run on,
a sequential-move simulator of the env's move phase, and the hand cases that pin what the rule decides.

The rule in one paragraph: the agents of an env are planned in index order, which is the order the env moves them in
within a step (MA-env:502-526).  Agent j floods space-time from its cell, ``reach[t] = (reach[t-1] and its four
neighbours) & free & ~blocked[t]``, where ``blocked[t] = occ[t] | occ[t+1]`` are the cells the agents planned before it
stand on at time t or enter at time t + 1 (``occ[T+1] = occ[T]``), and ``blocked[1]`` also holds the cells of the agents
after it, which have not moved when j makes its first move.  It arrives at the first time its goal is in the set and no
earlier plan needs the goal from then on, parks there, and its path is walked back from the goal taking the lowest action
id at every step.  An agent without such a time fails: arrival -1, all actions 0, it stands still for those after it.
"""

from __future__ import annotations

import functools

import numpy as np

import plan_util as pu

# action id -> (d row, d col); 0 waits
DELTA = {0: (0, 0), 1: (-1, 0), 2: (0, 1), 3: (1, 0), 4: (0, -1)}


def _cell(x):
    return (int(x[0]), int(x[1]))


# ---- 1. on sets ------------------------------------------------------------------------------------------------------
def plan_sets(grid: np.ndarray, positions, goals, T: int):
    """(plan int8 [T, N], arrival int32 [N], cells int16 [T + 1, N, 2]) of one env; cells[t, j] is c_t of agent j."""
    H, W = grid.shape
    N = len(positions)
    free = {(r, c) for r in range(H) for c in range(W) if grid[r, c] == 0}
    inside = lambda x: 0 <= x[0] < H and 0 <= x[1] < W
    step_to = {x: tuple(n for n in ((x[0] + dr, x[1] + dc) for dr, dc in DELTA.values()) if n in free)
               for x in {(r, c) for r in range(H) for c in range(W)}}
    plan, arrival = np.zeros((T, N), np.int8), np.full(N, -1, np.int32)
    cells = np.zeros((T + 1, N, 2), np.int16)
    p, g = [_cell(x) for x in positions], [_cell(x) for x in goals]
    for j in range(N):
        occ = [{_cell(cells[min(t, T), k]) for k in range(j)} for t in range(T + 2)]
        blocked = [occ[t] | occ[t + 1] for t in range(T + 1)]
        if T >= 1:
            blocked[1] = blocked[1] | {p[k] for k in range(j + 1, N)}
        # goal_free_from[t]: the goal is in no blocked[t'] for t' in t .. T
        goal_free_from = [False] * (T + 2)
        goal_free_from[T + 1] = True
        for t in range(T, -1, -1):
            goal_free_from[t] = goal_free_from[t + 1] and g[j] not in blocked[t]
        reach = [{p[j]} if inside(p[j]) and inside(g[j]) else set()]
        A = -1
        for t in range(T + 1):
            if t > 0:
                reach.append({n for x in reach[t - 1] for n in step_to[x]} - blocked[t])
            if g[j] in reach[t] and goal_free_from[t]:
                A = t
                break
            if not reach[t]:
                break
        arrival[j] = A
        if A < 0:
            cells[:, j] = p[j]
            continue
        c = g[j]
        cells[A:, j] = c
        for t in range(A, 0, -1):
            a = next(a for a in range(5) if (c[0] - DELTA[a][0], c[1] - DELTA[a][1]) in reach[t - 1])
            plan[t - 1, j] = a
            c = (c[0] - DELTA[a][0], c[1] - DELTA[a][1])
            cells[t - 1, j] = c
        assert c == p[j]
    return plan, arrival, cells


# ---- 2. on bit rows: rows are Python ints, bit c = column c; the occupancy of the agents planned so far is kept as one
#         cell per agent and time step and turned into a row mask when the flood needs it, as the kernel keeps it -------
def plan_bit_rows(grid: np.ndarray, positions, goals, T: int):
    H, W = grid.shape
    N = len(positions)
    full = (1 << W) - 1
    free = [full & ~sum(1 << c for c in range(W) if grid[r, c] != 0) for r in range(H)]
    plan, arrival = np.zeros((T, N), np.int8), np.full(N, -1, np.int32)
    pos = [[None] * N for _ in range(T + 1)]  # pos[t][k] = (row, col) of planned agent k at time t

    def occ_rows(t, j):
        m = [0] * H
        for k in range(j):
            r, c = pos[min(t, T)][k]
            if 0 <= r < H and 0 <= c < W:
                m[r] |= 1 << c
        return m

    later = [0] * H  # the cells of the agents that have not been planned yet (the one being planned included)
    for k in range(N):
        r, c = _cell(positions[k])
        if 0 <= r < H and 0 <= c < W:
            later[r] |= 1 << c
    for j in range(N):
        (pr, pc), (gr, gc) = _cell(positions[j]), _cell(goals[j])
        valid = 0 <= pr < H and 0 <= pc < W and 0 <= gr < H and 0 <= gc < W
        if 0 <= pr < H and 0 <= pc < W:
            later[pr] &= ~(1 << pc)
            for k in range(j + 1, N):  # (two agents on one cell: the later one still stands there)
                if _cell(positions[k]) == (pr, pc):
                    later[pr] |= 1 << pc
        A = -1
        hist = []
        if valid:
            # the last time an earlier plan holds the goal: blocked[t] has it for t = that time and the one before
            last = -1
            for t in range(T + 1):
                if any(pos[t][k] == (gr, gc) for k in range(j)):
                    last = t
            if T >= 1 and (later[gr] >> gc) & 1:
                last = max(last, 1)
            reach = [0] * H
            reach[pr] = 1 << pc
            m_now, m_next = occ_rows(0, j), occ_rows(1, j)
            for t in range(T + 1):
                if t > 0:
                    m_now, m_next = m_next, occ_rows(t + 1, j)
                    blk = [m_now[r] | m_next[r] | (later[r] if t == 1 else 0) for r in range(H)]
                    reach = [(reach[r] | (reach[r] << 1) | (reach[r] >> 1) | (reach[r - 1] if r > 0 else 0)
                              | (reach[r + 1] if r + 1 < H else 0)) & free[r] & ~blk[r] for r in range(H)]
                hist.append(reach)
                if t > last and (reach[gr] >> gc) & 1:
                    A = t
                    break
                if not any(reach):
                    break
        arrival[j] = A
        if A < 0:
            for t in range(T + 1):
                pos[t][j] = (pr, pc)
            continue
        cr, cc = gr, gc
        for t in range(A, T + 1):
            pos[t][j] = (gr, gc)
        for t in range(A, 0, -1):
            prev = hist[t - 1]
            cand = [(prev[cr] >> cc) & 1,
                    (prev[cr + 1] >> cc) & 1 if cr + 1 < H else 0,   # came UP from the row below
                    (prev[cr] >> (cc - 1)) & 1 if cc >= 1 else 0,    # came RIGHT from the column before
                    (prev[cr - 1] >> cc) & 1 if cr >= 1 else 0,      # came DOWN from the row above
                    (prev[cr] >> (cc + 1)) & 1]                      # came LEFT from the column after
            a = cand.index(1)
            plan[t - 1, j] = a
            cr, cc = cr - DELTA[a][0], cc - DELTA[a][1]
            pos[t - 1][j] = (cr, cc)
        assert (cr, cc) == (pr, pc)
    cells = np.array(pos, np.int16).reshape(T + 1, N, 2)
    return plan, arrival, cells


def plan_batch(fn, grids, positions, goals, T):
    """fn (one of the two restatements) over a batch: (plan [B, T, N], arrival [B, N], cells [B, T + 1, N, 2])."""
    res = [fn(grids[b] if grids.ndim == 3 else grids, positions[b], goals[b], T) for b in range(positions.shape[0])]
    return tuple(np.stack([r[i] for r in res]) for i in range(3))


def costs(arrival: np.ndarray):
    """(solved bool [B], sum_of_costs int64 [B], makespan int32 [B]) restated: -1 where an agent failed."""
    a = np.asarray(arrival, np.int32)
    solved = (a >= 0).all(axis=1)
    return solved, np.where(solved, a.astype(np.int64).sum(axis=1), -1), np.where(solved, a.max(axis=1), -1).astype(np.int32)


def first_all_on_goal(cells: np.ndarray, goals: np.ndarray) -> int:
    """The first time t >= 1 at which every planned cell is its goal (the env says ``terminated`` after that step; an env
    that starts solved says so after its first step); -1: never."""
    for t in range(1, cells.shape[0]):
        if (cells[t] == goals).all():
            return t
    return -1


# ---- the env's move phase, restated (MA-env:502-526): agents move in index order against live occupancy ------------------
def simulate_moves(grid: np.ndarray, positions, actions):
    """One step: (new positions int16 [N, 2], failed bool [N]).  A move fails when its target is outside the grid, an
    obstacle, or a cell an agent stands on at that moment."""
    H, W = grid.shape
    pos = [_cell(x) for x in positions]
    failed = np.zeros(len(pos), bool)
    for i, a in enumerate(actions):
        if int(a) == 0:
            continue
        t = (pos[i][0] + DELTA[int(a)][0], pos[i][1] + DELTA[int(a)][1])
        if 0 <= t[0] < H and 0 <= t[1] < W and grid[t] == 0 and t not in pos:
            pos[i] = t
        else:
            failed[i] = True
    return np.array(pos, np.int16), failed


# ---- instances -------------------------------------------------------------------------------------------------------
# (kind, H, W, N, density, horizon): one group width each, a width above 32, one row more than a group width; the last
# one has groups of 32 lanes, two to a wavefront (the cross-lane row shift meets a group's edge in the middle of the wave)
SHAPES = (("random", 3, 3, 2, 0.0, 16), ("random", 5, 5, 4, 0.1, 32), ("random", 12, 12, 8, 0.2, 64),
          ("random", 12, 33, 8, 0.2, 96), ("random", 33, 12, 16, 0.1, 96), ("random", 64, 64, 64, 0.2, 128),
          ("serpentine", 11, 12, 2, 0.0, 128), ("random", 20, 20, 12, 0.2, 64))
SHAPE_IDS = [f"{k}_{H}x{W}_n{N}" for k, H, W, N, _d, _T in SHAPES]
CLOSED_LOOP_SHAPES = (SHAPES[2], SHAPES[4])


def group_width(H: int) -> int:
    return next(g for g in (4, 8, 16, 32, 64) if g >= H)


def batch_of(H: int) -> int:
    """Envs of a GPU test: a wavefront plans 64 / G envs; 3 of them less one leaves a ragged last wavefront, 3 envs when
    an env takes the whole wavefront."""
    per_wave = 64 // group_width(H)
    return 3 if per_wave == 1 else 3 * per_wave - 1


@functools.lru_cache(maxsize=None)
def instances(kind: str, H: int, W: int, N: int, density: float, B: int, seed: int = 0):
    """(grids uint8 [B, H, W], positions int16 [B, N, 2], goals int16 [B, N, 2]): a different grid per env, starts
    distinct, goals distinct (read-only: shared among the tests)."""
    grids = pu.random_grids(H, W, B, density, 2 * N) if kind == "random" else pu.serpentine_grids(H, W, B)
    pos, goals = np.zeros((B, N, 2), np.int16), np.zeros((B, N, 2), np.int16)
    for b in range(B):
        free = pu.free_cells(grids[b])
        rng = np.random.default_rng(7_000 + 131 * seed + b)
        pos[b] = free[rng.permutation(len(free))[:N]]
        goals[b] = free[rng.permutation(len(free))[:N]]
    for a in (grids, pos, goals):
        a.setflags(write=False)
    return grids, pos, goals


@functools.lru_cache(maxsize=None)
def restated(kind: str, H: int, W: int, N: int, density: float, T: int, B: int, seed: int = 0):
    """The bit-row restatement over ``instances(...)``, computed once: (plan, arrival, cells), read-only."""
    grids, pos, goals = instances(kind, H, W, N, density, B, seed)
    out = plan_batch(plan_bit_rows, grids, pos, goals, T)
    for a in out:
        a.setflags(write=False)
    return out


# ---- hand cases: one property each -----------------------------------------------------------------------------------
def _grid(*rows):
    return np.array([[1 if ch == "#" else 0 for ch in row] for row in rows], np.uint8)


def _hand(name, grid, positions, goals, T, arrival, plan=None, cells=None):
    """plan: {agent: actions of its first steps (the rest are 0)}; cells: {agent: its cells from time 0 on}."""
    return {"name": name, "grid": grid, "positions": np.array(positions, np.int16), "goals": np.array(goals, np.int16),
            "T": T, "arrival": arrival, "plan": plan or {}, "cells": cells or {}}


CORRIDOR = _grid("###.#",
                 ".....")           # a corridor (row 1) with one pocket above its fourth cell
POCKET_MID = _grid("##.##",
                   ".....")         # the pocket above the middle cell
LINE5 = _grid(".....")
DEAD_END = _grid("....")
OPEN3 = np.zeros((3, 3), np.uint8)

HAND_CASES = [
    # agent 0 walks the corridor left to right; agent 1, head-on, goes to the pocket's mouth, steps up, waits while 0
    # passes, and comes down into the cell 0 leaves in the same step
    _hand("head_on_later_agent_waits_in_the_pocket", CORRIDOR, [(1, 0), (1, 4)], [(1, 4), (1, 0)], 12, [4, 7],
          plan={0: [2, 2, 2, 2], 1: [4, 1, 0, 3, 4, 4, 4]},
          cells={1: [(1, 4), (1, 3), (0, 3), (0, 3), (1, 3), (1, 2), (1, 1), (1, 0)]}),
    # agent 0 ahead, agent 1 directly behind: 0 moves first and frees the cell 1 enters, both move at every step
    _hand("following_both_move_every_step", LINE5, [(0, 1), (0, 0)], [(0, 4), (0, 3)], 8, [3, 3],
          plan={0: [2, 2, 2], 1: [2, 2, 2]}),
    # agent 1 ahead of agent 0: 1 has not moved when 0 makes its first move, so 0 waits once and a one-cell gap forms
    _hand("reverse_order_a_gap_forms", LINE5, [(0, 0), (0, 1)], [(0, 3), (0, 4)], 8, [4, 3],
          plan={0: [0, 2, 2, 2], 1: [2, 2, 2]},
          cells={0: [(0, 0), (0, 0), (0, 1), (0, 2), (0, 3)]}),
    # agent 1 stands on its goal in agent 0's way: it steps into the pocket and comes back, so its arrival is above 0
    _hand("agent_on_its_goal_steps_aside_and_returns", POCKET_MID, [(1, 0), (1, 2)], [(1, 4), (1, 2)], 12, [4, 3],
          plan={0: [2, 2, 2, 2], 1: [1, 0, 3]},
          cells={1: [(1, 2), (0, 2), (0, 2), (1, 2)]}),
    # agent 0 parks on its goal in the middle of the only corridor: agent 1 cannot pass, fails, and the env is unsolved
    _hand("parked_goal_cuts_the_corridor", DEAD_END, [(0, 0), (0, 3)], [(0, 1), (0, 0)], 10, [1, -1],
          plan={0: [2], 1: []}),
    # the horizon equal to the latest arrival is enough ...
    _hand("horizon_equal_to_the_arrival", LINE5, [(0, 0), (0, 1)], [(0, 3), (0, 4)], 4, [4, 3],
          plan={0: [0, 2, 2, 2], 1: [2, 2, 2]}),
    # ... one step less is not: agent 0 fails, and agent 1, planned against an agent that stands still, still arrives
    _hand("horizon_one_short_of_the_arrival", LINE5, [(0, 0), (0, 1)], [(0, 3), (0, 4)], 3, [-1, 3],
          plan={0: [], 1: [2, 2, 2]}),
    # the walk back decides the LAST step first and takes the lowest id.  Agent 0: RIGHT and DOWN in any order are
    # shortest; UP < RIGHT < DOWN, so its path ends with RIGHT, RIGHT.  Agent 1's goal is crossed by agent 0 at time 3, so
    # it arrives at 4 with one step to spare: it spends it waiting (id 0) on (1, 1), and DOWN (3) beats LEFT (4) before
    _hand("walk_back_takes_the_lowest_id_wait_included", OPEN3, [(0, 0), (0, 2)], [(2, 2), (2, 1)], 8, [4, 4],
          plan={0: [3, 3, 2, 2], 1: [4, 3, 0, 3]},
          cells={1: [(0, 2), (0, 1), (1, 1), (1, 1), (2, 1)]}),
]
