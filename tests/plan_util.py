"""The shortest-path planner's rule (include/mapf_step.h above mapf_expert_actions) restated in NumPy, the grids its tests
run on and the hand cases that pin what "expert" means.

The graph: the cells of a grid that are not obstacles, joined to their four neighbours; agents are never obstacles for a
distance.  ``field(grid, dst)[r, c]`` is the number of moves of a shortest path from (r, c) to dst, -1 where there is none
or where (r, c) or dst is an obstacle or outside the grid.  Everything here is plain Python on the host: a deque
breadth-first search, and a second statement of the same search on bit rows (Python ints), which is the formulation the
kernel runs.
"""

from __future__ import annotations

import functools
from collections import deque

import numpy as np

from trace_util import synth_grid

# action id -> (d row, d col), the reference's ids (MA-env:104-113); 0 is NO_OP
DELTAS = {1: (-1, 0), 2: (0, 1), 3: (1, 0), 4: (0, -1)}
MODES = {"independent": 0, "yielding": 1}
NO_PATH_U16 = 0xFFFF


def field(grid: np.ndarray, dst) -> np.ndarray:
    """int32 [H, W]: d((r, c) -> dst) of every cell, -1 where there is none."""
    H, W = grid.shape
    out = np.full((H, W), -1, np.int32)
    r0, c0 = int(dst[0]), int(dst[1])
    if not (0 <= r0 < H and 0 <= c0 < W) or grid[r0, c0] != 0:
        return out
    out[r0, c0] = 0
    q = deque([(r0, c0)])
    while q:
        r, c = q.popleft()
        for dr, dc in DELTAS.values():
            rr, cc = r + dr, c + dc
            if 0 <= rr < H and 0 <= cc < W and grid[rr, cc] == 0 and out[rr, cc] < 0:
                out[rr, cc] = out[r, c] + 1
                q.append((rr, cc))
    return out


def distance(grid: np.ndarray, src, dst, fld: np.ndarray | None = None) -> int:
    H, W = grid.shape
    r, c = int(src[0]), int(src[1])
    if not (0 <= r < H and 0 <= c < W):
        return -1
    return int((field(grid, dst) if fld is None else fld)[r, c])


def field_u16(grid: np.ndarray, dst) -> np.ndarray:
    """What mapf_distance_field stores: uint16, 0xFFFF for -1."""
    f = field(grid, dst)
    return np.where(f < 0, NO_PATH_U16, f).astype(np.uint16)


def expert_env(grid: np.ndarray, positions, goals, mode: int, fields=None):
    """(actions int8 [N], D int32 [N]) of one env under the rule.  fields: ``[field(grid, g) for g in goals]`` when the
    caller already has them (both modes read the same fields)."""
    H, W = grid.shape
    N = len(positions)
    occupied = {(int(p[0]), int(p[1])) for p in positions}
    acts, dist = np.zeros(N, np.int8), np.zeros(N, np.int32)
    for a in range(N):
        f = field(grid, goals[a]) if fields is None else fields[a]
        D = dist[a] = distance(grid, positions[a], goals[a], f)
        if D <= 0:
            continue
        for act, (dr, dc) in DELTAS.items():  # ascending ids: the lowest one decides
            r, c = int(positions[a][0]) + dr, int(positions[a][1]) + dc
            if 0 <= r < H and 0 <= c < W and grid[r, c] == 0 and f[r, c] == D - 1:
                if mode == 1 and (r, c) in occupied:
                    continue
                acts[a] = act
                break
    return acts, dist


def goal_fields(grids: np.ndarray, goals: np.ndarray) -> list:
    """[B][N] fields of the agents' goals; grids [B, H, W] or one shared [H, W]."""
    return [[field(grids[b] if grids.ndim == 3 else grids, g) for g in goals[b]] for b in range(goals.shape[0])]


def expert(grids: np.ndarray, positions: np.ndarray, goals: np.ndarray, mode: int, fields=None):
    """(actions int8 [B, N], D int32 [B, N]); grids [B, H, W] or one shared [H, W]; fields: ``goal_fields(grids, goals)``."""
    B = positions.shape[0]
    fields = goal_fields(grids, goals) if fields is None else fields
    res = [expert_env(grids[b] if grids.ndim == 3 else grids, positions[b], goals[b], mode, fields[b]) for b in range(B)]
    return np.stack([r[0] for r in res]), np.stack([r[1] for r in res])


# ---- the same search on bit rows: rows are Python ints, bit c = column c.  One expansion is
#      reach' = (reach | reach << 1 | reach >> 1 | row above | row below) & free
def bit_row_field(grid: np.ndarray, dst) -> np.ndarray:
    H, W = grid.shape
    out = np.full((H, W), -1, np.int32)
    full = (1 << W) - 1
    free = [full & ~sum(1 << c for c in range(W) if grid[r, c] != 0) for r in range(H)]
    r0, c0 = int(dst[0]), int(dst[1])
    reach = [0] * H
    fresh = [0] * H
    if 0 <= r0 < H and 0 <= c0 < W:
        fresh[r0] = (1 << c0) & free[r0]
    d = 0
    while any(fresh):
        for r in range(H):
            m = fresh[r]
            while m:
                c = (m & -m).bit_length() - 1
                out[r, c] = d
                m &= m - 1
            reach[r] |= fresh[r]
        nxt = [(reach[r] | (reach[r] << 1) | (reach[r] >> 1) | (reach[r - 1] if r > 0 else 0) | (reach[r + 1] if r + 1 < H else 0))
               & free[r] for r in range(H)]
        fresh = [nxt[r] & ~reach[r] for r in range(H)]
        d += 1
        assert d <= H * W + 1
    return out


# ---- grids -----------------------------------------------------------------------------------------------------------
def serpentine(H: int, W: int) -> np.ndarray:
    """Odd rows are walls with one gap, alternating at the last and the first column: one corridor through every free
    cell, the longest shortest path a grid of the size can hold."""
    g = np.zeros((H, W), np.uint8)
    for r in range(1, H, 2):
        g[r, :] = 1
        g[r, W - 1 if (r // 2) % 2 == 0 else 0] = 0
    return g


# (H, W) of the random grids: every group width (4 ... 64 lanes), widths at and around 32 and the sentinel-column limit
# (W <= 54 carries col_pad = 5, wider rows none), one row more than a group width (33)
SHAPES = ((3, 3), (12, 12), (12, 31), (12, 32), (12, 33), (33, 12), (5, 64), (64, 64))
SERPENTINES = ((11, 12), (13, 64), (64, 64), (63, 33))
# farthest cell from (0, 0) and number of free cells of the serpentines
SERPENTINE_ANSWERS = {(11, 12): (76, 77), (13, 64): (453, 454), (64, 64): (2079, 2080), (63, 33): (1086, 1087)}
DENSITY = 0.4
DENSITY_CONNECTED = 0.2


@functools.lru_cache(maxsize=None)
def random_grids(H: int, W: int, B: int, density: float = DENSITY, need_free: int = 2, base_seed: int = 40_000) -> np.ndarray:
    """[B, H, W], a different grid per env (read-only: shared among the tests)."""
    assert need_free <= H * W // 2, "synth_grid loops until it finds need_free free cells"
    g = np.stack([synth_grid(base_seed + b, H, W, density, need_free) for b in range(B)])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def serpentine_grids(H: int, W: int, B: int) -> np.ndarray:
    """[B, H, W]: the serpentine, and -- so that the envs differ -- flipped left-right in odd envs."""
    s = serpentine(H, W)
    g = np.stack([s if b % 2 == 0 else s[:, ::-1] for b in range(B)])
    g.setflags(write=False)
    return g


def free_cells(grid: np.ndarray) -> np.ndarray:
    return np.argwhere(grid == 0)


def queries(grids: np.ndarray, K: int, seed: int, n_dst: int = 6):
    """K queries (env_ids int32 [K], src int16 [K, 2], dst int16 [K, 2]) on ``grids``: repeated env ids, destinations from
    a pool of n_dst (env, cell) pairs -- free cells, and one obstacle if the grid has any -- sources anywhere in the grid,
    obstacles included; query 0 has src = dst, query 1 (K > 1) starts on an obstacle when the env has one."""
    rng = np.random.default_rng(seed)
    B, H, W = grids.shape
    pool = []
    for i in range(n_dst):
        b = int(rng.integers(B))
        cells = free_cells(grids[b])
        if i == n_dst - 1 and (grids[b] != 0).any():
            cells = np.argwhere(grids[b] != 0)
        pool.append((b, tuple(int(v) for v in cells[rng.integers(len(cells))])))
    env_ids, src, dst = np.zeros(K, np.int32), np.zeros((K, 2), np.int16), np.zeros((K, 2), np.int16)
    for k in range(K):
        b, d = pool[int(rng.integers(len(pool)))] if k else pool[0]
        env_ids[k], dst[k] = b, d
        src[k] = (rng.integers(H), rng.integers(W))
    src[0] = dst[0]
    if K > 1 and (grids[env_ids[1]] != 0).any():
        walls = np.argwhere(grids[env_ids[1]] != 0)
        src[1] = walls[rng.integers(len(walls))]
    return env_ids, src, dst


# ---- hand cases: what the rule decides, one property each ------------------------------------------------------------
OPEN3 = np.zeros((3, 3), np.uint8)
WALL3 = np.array([[0, 1, 0], [0, 1, 0], [0, 1, 0]], np.uint8)


def _case(name, grid, positions, goals, independent, yielding, dist):
    return {"name": name, "grid": grid, "positions": np.array(positions, np.int16), "goals": np.array(goals, np.int16),
            "independent": independent, "yielding": yielding, "dist": dist}


# positions / goals per agent (row, col); expected actions per mode and D per agent
RULE_CASES = [
    _case("unreachable_pair", WALL3, [(0, 0), (2, 2)], [(2, 2), (0, 2)], [0, 1], [0, 1], [-1, 2]),
    _case("agent_on_its_goal", OPEN3, [(1, 1), (0, 0)], [(1, 1), (0, 2)], [0, 2], [0, 2], [0, 2]),
    _case("two_optimal_moves_lowest_id", OPEN3, [(2, 0), (0, 0)], [(0, 2), (2, 2)], [1, 2], [1, 2], [4, 4]),
    _case("yields_to_another_optimal_move", OPEN3, [(2, 0), (1, 0)], [(0, 2), (1, 2)], [1, 2], [2, 2], [4, 2]),
    _case("yielding_agent_waits", OPEN3, [(0, 0), (0, 1)], [(0, 2), (2, 1)], [2, 3], [0, 3], [2, 2]),
    _case("path_longer_than_h_plus_w", serpentine(5, 5), [(0, 0), (4, 4)], [(4, 0), (2, 4)], [2, 4], [2, 4], [12, 10]),
]
