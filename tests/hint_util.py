"""Helpers for the tests of the engine's "may finish" hint (MAPF_CTR_MAY_FINISH, include/mapf_step.h): NumPy only, nothing
of the library is imported here.

The hint is one word per env, written by every finite-mode step: 0 = the env CANNOT end its episode in its next step.  The
background placement draws (sliced draw, sampler workgroups, the single-agent env's sampler) touch an env's stream and
slot on the strength of that word alone, so the invariant the tests pin is

    hint == 0  implies  not can_end(state)

with ``can_end`` below evaluated on the CPU oracle's state.

``carved_case`` builds states that sit one stand-alone respawn away from an episode end: an all-obstacle grid with exactly
2N (variant "A") or 2N + 1 (variant "B") free cells,

    row 0:   Y P X . . .        P = agent 0, X its free right neighbour, Y (variant B only) its free left neighbour
    row 1:   all obstacles
    row 2..: L R L R L R ...    agent i = 1 .. N-1 stands on L, its goal is the R next to it

Agent 0's goal is the cell agent 1 stands on (L1 distance 3: the episode cannot end in the next step; occupied, hence no
respawn candidate).  Every free cell but X (and Y) holds an agent or somebody else's goal, so `_assign_new_goal(0)` has
k = 1 candidate (X, no draw) in variant A and k = 2 (X or Y, one draw) in variant B -- both within one move of agent 0.
The 1 x 4 corridor of test_round4_gpu.py (two agents, F = 2N) is the smallest layout of this kind.
"""

from __future__ import annotations

import numpy as np

NO_OP, UP, RIGHT, DOWN, LEFT = 0, 1, 2, 3, 4
STEPS_PER_EPISODE = 6
VARIANTS = ("A", "B")
# guard_util.CASES ids: one per background-draw mechanism / kernel family (the issue's table), and the single-agent case
MA_CASE_IDS = ("c3_three_wave", "c3_dense_two_wave", "runtime_sliced_sr1", "runtime_sampler_workgroups", "partial_n12",
               "train16_bit_rows", "wide_n33_finite")
CTE_CASE_ID = "cte_n4_6x7_default"


def can_end(positions, goals, step_count, steps_per_episode):
    """True where an env can end its episode in its NEXT step: every agent within one move of its goal (L1 distance <= 1),
    or the step limit due (step_count + 1 >= steps_per_episode).  positions / goals: [..., N, 2]; step_count: [...]."""
    d = np.abs(np.asarray(positions, np.int64) - np.asarray(goals, np.int64)).sum(axis=-1)
    return (d <= 1).all(axis=-1) | (np.asarray(step_count, np.int64) + 1 >= int(steps_per_episode))


def carved_case(n: int, h: int, w: int, variant: str) -> dict:
    """The carved near-finish state of the module docstring for N = n agents on an h x w grid.  Returns grid uint8 [h, w]
    (1 = obstacle), positions / goals int16 [n, 2], x / y (int16 [2]; y is None in variant A), n_free, and
    actions_x / actions_y: the int8 [n] action rows that put every agent on its goal, without a conflict, once agent 0's
    goal is X / Y."""
    assert variant in VARIANTS, variant
    assert n >= 2 and w >= 3
    per_row = w // 2
    rows = -(-(n - 1) // per_row)
    assert 2 + rows <= h, f"{n} agents do not fit the layout on {h} x {w}"
    grid = np.ones((h, w), np.uint8)
    pos = np.zeros((n, 2), np.int16)
    goal = np.zeros((n, 2), np.int16)
    pos[0] = (0, 1)
    x = np.array((0, 2), np.int16)
    y = np.array((0, 0), np.int16) if variant == "B" else None
    grid[0, 1] = grid[0, 2] = 0
    if y is not None:
        grid[0, 0] = 0
    for i in range(1, n):
        r, c = 2 + (i - 1) // per_row, 2 * ((i - 1) % per_row)
        pos[i] = (r, c)
        goal[i] = (r, c + 1)
        grid[r, c] = grid[r, c + 1] = 0
    goal[0] = pos[1]
    actions_x = np.full(n, RIGHT, np.int8)
    actions_y = actions_x.copy()
    actions_y[0] = LEFT
    return {"grid": grid, "positions": pos, "goals": goal, "x": x, "y": y, "n_free": int((grid == 0).sum()),
            "actions_x": actions_x, "actions_y": None if y is None else actions_y}


def finish_actions(carved: dict, goal0) -> np.ndarray:
    """The action row that ends the episode, given agent 0's goal after the respawn (X, or Y in variant B)."""
    g = tuple(int(v) for v in goal0)
    if g == tuple(int(v) for v in carved["x"]):
        return carved["actions_x"]
    assert carved["y"] is not None and g == tuple(int(v) for v in carved["y"]), (g, carved["x"], carved["y"])
    return carved["actions_y"]
