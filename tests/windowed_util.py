"""The windowed prioritised planner's rule (include/mapf_step.h above mapf_plan_windowed) restated twice in plain Python --
once on sets of cells per time step with ``plan_util.field`` for the distances, once on bit rows (Python ints) with the
goal flood that meets ``reach[w]``, the form the kernel runs -- a batch wrapper, and the hand cases that pin what the rule
decides.  Instances, the sequential-move simulator and the group widths are those of ``prioritized_util``.

The rule in one paragraph: the agents of an env are planned in index order, the env's move order.  Agent j floods
space-time from its cell for w steps, ``reach[t] = (reach[t-1] and its four neighbours) & free & ~blocked[t]`` with
``blocked[t] = occ[t] | occ[t+1]`` of the agents planned before it (``occ[w+1] = occ[w]``) and, at t = 1, the cells of the
agents after it.  An empty set at any time FAILS the agent: remaining -1, arrival -1, all actions 0, it stands still for
those after it.  Otherwise it ends the window on the cell of ``reach[w]`` with the smallest (distance to its goal, row,
col), no path counting as farther than any; ``remaining`` is that distance (-2: no path), the path is walked back taking
the lowest action id at every step, and ``arrival`` is the first time the path is on the goal (-1: never).
"""

from __future__ import annotations

import functools

import numpy as np

import plan_util as pu
import prioritized_util as pq
from prioritized_util import DELTA, _cell

WINDOWS = (1, 4, 16)


# ---- 1. on sets ------------------------------------------------------------------------------------------------------
def plan_sets(grid: np.ndarray, positions, goals, w: int):
    """(plan int8 [w, N], arrival int32 [N], remaining int32 [N], cells int16 [w + 1, N, 2]) of one env."""
    H, W = grid.shape
    N = len(positions)
    free = {(r, c) for r in range(H) for c in range(W) if grid[r, c] == 0}
    inside = lambda x: 0 <= x[0] < H and 0 <= x[1] < W
    plan = np.zeros((w, N), np.int8)
    arrival, remaining = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    cells = np.zeros((w + 1, N, 2), np.int16)
    p, g = [_cell(x) for x in positions], [_cell(x) for x in goals]
    for j in range(N):
        occ = [{_cell(cells[min(t, w), k]) for k in range(j)} for t in range(w + 2)]
        blocked = [occ[t] | occ[t + 1] for t in range(w + 1)]
        blocked[1] = blocked[1] | {p[k] for k in range(j + 1, N)}
        reach = [{p[j]} if inside(p[j]) else set()]
        for t in range(1, w + 1):
            grown = {(x[0] + dr, x[1] + dc) for x in reach[t - 1] for dr, dc in DELTA.values()}
            reach.append((grown & free) - blocked[t])
        if not all(reach):
            cells[:, j] = p[j]
            continue
        d = pu.field(grid, g[j])
        key = lambda x: (d[x] if d[x] >= 0 else np.iinfo(np.int32).max, x[0], x[1])
        c = min(reach[w], key=key)
        remaining[j] = d[c] if d[c] >= 0 else -2
        cells[w, j] = c
        for t in range(w, 0, -1):
            a = next(a for a in range(5) if (c[0] - DELTA[a][0], c[1] - DELTA[a][1]) in reach[t - 1])
            plan[t - 1, j] = a
            c = (c[0] - DELTA[a][0], c[1] - DELTA[a][1])
            cells[t - 1, j] = c
        assert c == p[j]
        on_goal = [t for t in range(w + 1) if _cell(cells[t, j]) == g[j]]
        arrival[j] = on_goal[0] if on_goal else -1
    return plan, arrival, remaining, cells


# ---- 2. on bit rows: rows are Python ints, bit c = column c; one cell per planned agent and time step, turned into a
#         row mask when the flood needs it; the end cell from a flood of the goal that meets reach[w] ------------------
def plan_bit_rows(grid: np.ndarray, positions, goals, w: int):
    H, W = grid.shape
    N = len(positions)
    full = (1 << W) - 1
    free = [full & ~sum(1 << c for c in range(W) if grid[r, c] != 0) for r in range(H)]
    plan = np.zeros((w, N), np.int8)
    arrival, remaining = np.full(N, -1, np.int32), np.full(N, -1, np.int32)
    pos = [[None] * N for _ in range(w + 1)]  # pos[t][k] = (row, col) of planned agent k at time t

    def expand(s, inside_of):
        return [(s[r] | (s[r] << 1) | (s[r] >> 1) | (s[r - 1] if r > 0 else 0) | (s[r + 1] if r + 1 < H else 0)) & inside_of[r]
                for r in range(H)]

    def occ_rows(t, j):
        m = [0] * H
        for k in range(j):
            r, c = pos[min(t, w)][k]
            if 0 <= r < H and 0 <= c < W:
                m[r] |= 1 << c
        return m

    for j in range(N):
        (pr, pc), (gr, gc) = _cell(positions[j]), _cell(goals[j])
        p_in, g_in = 0 <= pr < H and 0 <= pc < W, 0 <= gr < H and 0 <= gc < W
        later = [0] * H  # the cells of the agents after j
        for k in range(j + 1, N):
            r, c = _cell(positions[k])
            if 0 <= r < H and 0 <= c < W:
                later[r] |= 1 << c
        reach = [0] * H
        if p_in:
            reach[pr] = 1 << pc
        hist = [reach]
        alive = p_in
        m_next = occ_rows(1, j)
        for t in range(1, w + 1):
            if not alive:
                break
            m_now, m_next = m_next, occ_rows(t + 1, j)
            open_ = [free[r] & ~(m_now[r] | m_next[r] | (later[r] if t == 1 else 0)) for r in range(H)]
            reach = expand(reach, open_)
            hist.append(reach)
            alive = any(reach)
        if not alive:
            for t in range(w + 1):
                pos[t][j] = (pr, pc)
            continue
        # the goal's flood on free alone: the first level that meets reach[w] is the distance of the cells it meets in
        gv = [0] * H
        if g_in:
            gv[gr] = (1 << gc) & free[gr]
        D, k = -2, 0
        while True:
            if any(gv[r] & reach[r] for r in range(H)):
                D = k
                break
            nv = expand(gv, free)
            if nv == gv:
                break
            gv, k = nv, k + 1
            assert k <= H * W
        cand = [gv[r] & reach[r] for r in range(H)] if D >= 0 else reach
        cr = next(r for r in range(H) if cand[r])
        cc = (cand[cr] & -cand[cr]).bit_length() - 1
        remaining[j] = D
        pos[w][j] = (cr, cc)
        arr = w if (cr, cc) == (gr, gc) else -1
        for t in range(w, 0, -1):
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
            if (cr, cc) == (gr, gc):
                arr = t - 1
        assert (cr, cc) == (pr, pc)
        arrival[j] = arr
    cells = np.array(pos, np.int16).reshape(w + 1, N, 2)
    return plan, arrival, remaining, cells


def plan_batch(fn, grids, positions, goals, w):
    """fn (one of the two restatements) over a batch: (plan [B, w, N], arrival [B, N], remaining [B, N],
    cells [B, w + 1, N, 2])."""
    res = [fn(grids[b] if grids.ndim == 3 else grids, positions[b], goals[b], w) for b in range(positions.shape[0])]
    return tuple(np.stack([r[i] for r in res]) for i in range(4))


def costs(arrival: np.ndarray, remaining: np.ndarray):
    """(consistent bool [B], arrived int32 [B], remaining_sum int64 [B]) restated: -1 where the env is inconsistent, and
    for the sum also where a goal is unreachable."""
    a, rem = np.asarray(arrival, np.int32), np.asarray(remaining, np.int32)
    consistent = (rem != -1).all(axis=1)
    arrived = np.where(consistent, (a >= 0).sum(axis=1), -1).astype(np.int32)
    summable = consistent & (rem >= 0).all(axis=1)
    return consistent, arrived, np.where(summable, rem.astype(np.int64).sum(axis=1), -1)


@functools.lru_cache(maxsize=None)
def restated(kind: str, H: int, W: int, N: int, density: float, w: int, B: int, seed: int = 0):
    """The bit-row restatement over ``prioritized_util.instances(...)``, computed once: (plan, arrival, remaining, cells),
    read-only."""
    grids, pos, goals = pq.instances(kind, H, W, N, density, B, seed)
    out = plan_batch(plan_bit_rows, grids, pos, goals, w)
    for a in out:
        a.setflags(write=False)
    return out


# ---- hand cases (the grids of prioritized_util): one property each ---------------------------------------------------
def _hand(name, grid, positions, goals, w, plan, arrival, remaining, end=None):
    """plan: the w actions of every agent; end: {agent: its cell at time w}."""
    return {"name": name, "grid": grid, "positions": np.array(positions, np.int16), "goals": np.array(goals, np.int16),
            "w": w, "plan": plan, "arrival": arrival, "remaining": remaining, "end": end or {}}


HAND_CASES = [
    _hand("window_shorter_than_the_path", pq.LINE5, [(0, 0)], [(0, 4)], 2, [[2, 2]], [-1], [2]),
    _hand("arrives_and_waits", pq.LINE5, [(0, 0)], [(0, 4)], 6, [[2, 2, 2, 2, 0, 0]], [4], [0]),
    _hand("unreachable_goal_stays_put", pq._grid(".#."), [(0, 0)], [(0, 2)], 2, [[0, 0]], [-1], [-2]),
    _hand("head_on_in_the_corridor", pq.CORRIDOR, [(1, 0), (1, 4)], [(1, 4), (1, 0)], 8,
          [[2, 2, 2, 2, 0, 0, 0, 0], [4, 1, 0, 3, 4, 4, 4, 0]], [4, 7], [0, 0]),
    _hand("head_on_cut_mid_manoeuvre", pq.CORRIDOR, [(1, 0), (1, 4)], [(1, 4), (1, 0)], 3,
          [[2, 2, 2], [4, 1, 0]], [-1, -1], [1, 4]),
    _hand("swap_in_a_dead_end_line_the_later_agent_fails", pq._grid("..."), [(0, 2), (0, 0)], [(0, 0), (0, 2)], 3,
          [[4, 4, 0], [0, 0, 0]], [2, -1], [0, -1]),
    _hand("tie_on_distance_lowest_row_then_column", pq.OPEN3, [(0, 0)], [(2, 2)], 2, [[2, 2]], [-1], [2], end={0: (0, 2)}),
    _hand("agent_on_its_goal_steps_aside_and_returns", pq.POCKET_MID, [(1, 0), (1, 2)], [(1, 4), (1, 2)], 6,
          [[2, 2, 2, 2, 0, 0], [1, 0, 3, 0, 0, 0]], [4, 0], [0, 0]),
    _hand("window_one_the_later_agents_cell_blocks_the_first_move", pq.LINE5, [(0, 0), (0, 1)], [(0, 3), (0, 4)], 1,
          [[0], [2]], [-1, -1], [3, 2]),
]
