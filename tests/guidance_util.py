"""The shortest-path guidance rule (include/mapf_step.h above mapf_observe_guided) restated in NumPy on plan_util's
breadth-first search, the rows ``mapf_observe_guided`` builds from it, and the cases its host and GPU tests share: random
grids of every shape of plan_util.SHAPES at both densities and serpentines, with placements ``mapf_set_state`` accepts
(agents on distinct free cells, distinct goals) that hold every class of the rule, and the hand cases the rule decides.
"""

from __future__ import annotations

import functools

import numpy as np

import plan_util as pu

GUIDANCE_LEN = 6


def guidance_ref(grids: np.ndarray, positions: np.ndarray, goals: np.ndarray, fields=None) -> np.ndarray:
    """float32 [B, N, 6] under the rule; grids [B, H, W] or one shared [H, W]; fields: ``plan_util.goal_fields(grids, goals)``."""
    B, N = positions.shape[:2]
    fields = pu.goal_fields(grids, goals) if fields is None else fields
    q = np.zeros((B, N, GUIDANCE_LEN), np.float32)
    for b in range(B):
        grid = grids[b] if grids.ndim == 3 else grids
        H, W = grid.shape
        for j in range(N):
            f = fields[b][j]
            D = pu.distance(grid, positions[b, j], goals[b, j], f)
            if D < 0:
                q[b, j, 5] = -1.0
                continue
            q[b, j, 0] = 1.0 if D == 0 else 0.0
            q[b, j, 5] = np.float32(D) / np.float32(H * W)  # (the correctly rounded fp32 quotient)
            for a, (dr, dc) in pu.DELTAS.items():
                r, c = int(positions[b, j, 0]) + dr, int(positions[b, j, 1]) + dc
                if D > 0 and 0 <= r < H and 0 <= c < W and grid[r, c] == 0 and f[r, c] == D - 1:
                    q[b, j, a] = 1.0
    return q


def guided_rows_ref(obs: np.ndarray, q: np.ndarray, tail: int) -> np.ndarray:
    """[B, N, L + 6]: obs[..., :L - tail], q, obs[..., L - tail:]; moved as 4-byte words, whatever dtype ``obs`` has."""
    L = obs.shape[-1]
    words = np.ascontiguousarray(q, np.float32).view(obs.dtype) if obs.dtype.itemsize == 4 else q
    return np.concatenate([obs[..., :L - tail], words, obs[..., L - tail:]], axis=-1)


def decoded_action(q: np.ndarray) -> np.ndarray:
    """int8 [...]: the lowest a in 1..4 with q[a] == 1, else 0 -- what mapf_expert_actions mode 0 gives."""
    bits = q[..., 1:5] == 1.0
    return np.where(bits.any(axis=-1), bits.argmax(axis=-1) + 1, 0).astype(np.int8)


def decoded_distance(q: np.ndarray, HW: int) -> np.ndarray:
    """int32 [...]: D from q[5] (exact: D <= H W <= 4096 and the quotient is correctly rounded)."""
    return np.where(q[..., 5] < 0, -1, np.rint(q[..., 5].astype(np.float64) * HW)).astype(np.int32)


def classes(q: np.ndarray) -> dict:
    """How many agents of ``q`` fall into each class of the rule."""
    n = (q[..., 1:5] == 1.0).sum(axis=-1)
    return {"on_goal": int((q[..., 0] == 1.0).sum()), "no_path": int((q[..., 5] < 0).sum()), "one_move": int((n == 1).sum()),
            "two_moves": int((n == 2).sum())}


# ---- the shared cases: (kind, H, W, N, density, B).  N in {1, 3, 8, 64}; B N searches leave the last workgroup of
# 256 / G searches partly filled wherever N allows it (G = the group width of H: 4 ... 64), and fill more than one.
def _shape_cases(kind, density):
    return [(kind, 3, 3, 1, density, 67), (kind, 12, 12, 3, density, 7), (kind, 12, 31, 8, density, 5), (kind, 12, 32, 3, density, 7),
            (kind, 12, 33, 64, density, 2), (kind, 33, 12, 1, density, 13), (kind, 5, 64, 8, density, 5), (kind, 64, 64, 3, density, 7)]


CASES = _shape_cases("random", pu.DENSITY) + _shape_cases("random", pu.DENSITY_CONNECTED) + [
    ("serpentine", 11, 12, 8, 0.0, 3), ("serpentine", 13, 64, 3, 0.0, 7)]
CASE_IDS = [f"{k}_{H}x{W}_n{N}_d{int(d * 10)}_b{B}" for k, H, W, N, d, B in CASES]
PLACEMENT_SEED = 81_000


def case_grids(kind, H, W, N, density, B) -> np.ndarray:
    # (a 3 x 3 grid cannot promise more than two free cells; the others hold the 2 N the engine asks for)
    return pu.random_grids(H, W, B, density, min(2 * N, H * W // 2)) if kind == "random" else pu.serpentine_grids(H, W, B)


@functools.lru_cache(maxsize=None)
def case_state(case) -> dict:
    """grids, positions and goals (int16 [B, N, 2]) of a case, its fields and its guidance (read-only: shared).  Agents
    stand on distinct free cells and goals are distinct, as mapf_set_state demands.  Of the agents k = b N + j, every
    fourth has its own cell as goal (D = 0) and every fourth, one further, an obstacle cell where the grid has one
    (D < 0); the others aim at random free cells, reachable or not."""
    kind, H, W, N, density, B = case
    grids = case_grids(*case)
    rng = np.random.default_rng(PLACEMENT_SEED + 131 * H + W + N)
    positions, goals = np.zeros((B, N, 2), np.int16), np.zeros((B, N, 2), np.int16)
    for b in range(B):
        free = pu.free_cells(grids[b])
        walls = np.argwhere(grids[b] != 0)
        positions[b] = free[rng.permutation(len(free))[:N]]
        own = [k for k in range(N) if (b * N + k) % 4 == 0]
        taken = {tuple(positions[b, k]) for k in own}
        for k in range(N):
            if k in own:
                goals[b, k] = positions[b, k]
                continue
            pool = walls if (b * N + k) % 4 == 1 and len(walls) else free
            cand = [c for c in pool[rng.permutation(len(pool))] if tuple(c) not in taken]
            if not cand:  # (a crowded tiny grid: any cell of the grid no goal sits on yet)
                cand = [c for c in np.argwhere(np.ones((H, W), bool)) if tuple(c) not in taken]
            goals[b, k] = cand[0]
            taken.add(tuple(cand[0]))
    fields = pu.goal_fields(grids, goals)
    out = {"grids": grids, "positions": positions, "goals": goals, "fields": fields, "q": guidance_ref(grids, positions, goals, fields)}
    for v in (positions, goals, out["q"]):
        v.setflags(write=False)
    return out


# ---- hand cases: one decision of the rule each.  (name, grid, [(position, goal, q[0..4], D)])
OPEN3, WALL3 = pu.OPEN3, pu.WALL3
OPEN3x5, OPEN3x64 = np.zeros((3, 5), np.uint8), np.zeros((3, 64), np.uint8)  # (with and without the sentinel columns)
HAND_CASES = [
    ("agent_on_its_goal", OPEN3, [((1, 1), (1, 1), [1, 0, 0, 0, 0], 0), ((0, 0), (0, 2), [0, 0, 1, 0, 0], 2)]),
    ("walled_off_goal", WALL3, [((0, 0), (2, 2), [0, 0, 0, 0, 0], -1), ((2, 2), (0, 2), [0, 1, 0, 0, 0], 2)]),
    ("goal_on_an_obstacle", WALL3, [((0, 0), (1, 1), [0, 0, 0, 0, 0], -1), ((2, 0), (0, 0), [0, 1, 0, 0, 0], 2)]),
    ("two_optimal_moves", OPEN3, [((2, 0), (0, 2), [0, 1, 1, 0, 0], 4), ((1, 2), (2, 1), [0, 0, 0, 1, 1], 2)]),
    ("corners_targets_outside_the_grid", OPEN3, [((0, 0), (2, 2), [0, 0, 1, 1, 0], 4), ((2, 2), (0, 0), [0, 1, 0, 0, 1], 4)]),
    ("left_at_column_1_right_at_column_w_minus_2", OPEN3x5, [((1, 1), (1, 0), [0, 0, 0, 0, 1], 1), ((1, 3), (1, 4), [0, 0, 1, 0, 0], 1)]),
    ("the_same_on_rows_without_sentinel_columns", OPEN3x64, [((1, 1), (1, 0), [0, 0, 0, 0, 1], 1), ((1, 62), (1, 63), [0, 0, 1, 0, 0], 1)]),
]
HAND_IDS = [c[0] for c in HAND_CASES]


def hand_state(case):
    """(grid, positions int16 [1, N, 2], goals, q float32 [1, N, 6]) of a hand case, q as the case states it."""
    _name, grid, agents = case
    H, W = grid.shape
    pos = np.array([[a[0] for a in agents]], np.int16)
    goals = np.array([[a[1] for a in agents]], np.int16)
    q = np.array([[list(a[2]) + [-1.0 if a[3] < 0 else np.float32(a[3]) / np.float32(H * W)] for a in agents]], np.float32)
    return grid, pos, goals, q
