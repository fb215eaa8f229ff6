"""Derived-distance layout, host side (no GPU): the two pure conversions behind mapf_get_state / mapf_set_state of a handle
that keeps one bit per step ("the distance went down") instead of the goal-distance bytes -- mapf_derived_to_ring and
mapf_derived_from_ring (include/mapf_step.h) -- against a NumPy restatement written here from the definition alone:

    a move is one cell, so it changes the L1 distance to the fixed goal by exactly one; a step without a move leaves it.
    Row k + 1 back is therefore row k back, + 1 after a step down, - 1 after any other move, + 0 without a move.

The walks are random walks of 40 steps on an 8 x 8 grid with resets inside them; after every step the numeric ring the walk
itself kept must survive ring -> bits -> ring, for every window pair the engine treats differently."""

from __future__ import annotations

import ctypes as C

import numpy as np
import pytest


def _lib():
    try:
        from dl_reference_models_amd import _lib as L

        return L.load()
    except Exception as e:  # no library / no loadable HIP runtime on this host
        pytest.skip(f"the engine library cannot be loaded here: {e}")


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


# ---- NumPy restatement -------------------------------------------------------------------------------------------------------
def np_to_ring(down, lw, t, pos, goal, moved):
    N = len(down)
    ring = np.zeros((lw, N), np.int16)
    for a in range(N):
        d = abs(int(goal[a, 0]) - int(pos[a, 0])) + abs(int(goal[a, 1]) - int(pos[a, 1]))
        for k in range(min(t, lw)):
            ring[(t - 1 - k) % lw, a] = d
            if (int(moved[a]) >> k) & 1:
                d += 1 if (int(down[a]) >> k) & 1 else -1
    return ring


def np_from_ring(ring, lw, t, pos, goal, moved):
    N = ring.shape[1]
    down = np.zeros(N, np.uint16)
    ok = True
    n = min(t, lw)
    for a in range(N):
        back = [int(ring[(t - 1 - k) % lw, a]) for k in range(n)]
        d = abs(int(goal[a, 0]) - int(pos[a, 0])) + abs(int(goal[a, 1]) - int(pos[a, 1]))
        if n and back[0] != d:
            ok = False
        for k in range(n - 1):
            diff, mv = back[k + 1] - back[k], (int(moved[a]) >> k) & 1
            if mv and abs(diff) != 1 or not mv and diff != 0:
                ok = False
            if mv and diff == 1:
                down[a] |= 1 << k
    return ok, down


def lib_to_ring(L, down, lw, t, pos, goal, moved):
    N = len(down)
    hist = np.zeros((N, 3), np.uint64)
    hist[:, 0] = moved
    ring = np.full((lw, N), -7, np.int16)
    L.mapf_derived_to_ring(_p(np.ascontiguousarray(down, np.uint16)), lw, N, t, _p(np.ascontiguousarray(pos, np.int16)),
                           _p(np.ascontiguousarray(goal, np.int16)), _p(hist), _p(ring))
    return ring


def lib_from_ring(L, ring, lw, t, pos, goal, moved):
    N = ring.shape[1]
    hist = np.zeros((N, 3), np.uint64)
    hist[:, 0] = moved
    down = np.full(N, 0xAAAA, np.uint16)
    ok = L.mapf_derived_from_ring(_p(np.ascontiguousarray(ring, np.int16)), lw, N, t, _p(np.ascontiguousarray(pos, np.int16)),
                                  _p(np.ascontiguousarray(goal, np.int16)), _p(hist), _p(down))
    return bool(ok), down


# ---- random walks ------------------------------------------------------------------------------------------------------------
MOVES = np.array([[0, 0], [-1, 0], [0, 1], [1, 0], [0, -1]])


@pytest.mark.parametrize("dw,lw", [(8, 16), (16, 16), (3, 5)])
def test_ring_bits_ring_is_the_identity_along_random_walks(dw, lw):
    L = _lib()
    rng = np.random.default_rng(100 * dw + lw)
    N, side = 5, 8
    short = full = 0
    for walk in range(6):
        pos, goal = rng.integers(0, side, (N, 2)), rng.integers(0, side, (N, 2))
        moved, down, rows = np.zeros(N, np.uint64), np.zeros(N, np.uint64), []
        reset_at = set(rng.integers(3, 38, 2).tolist())
        for step in range(40):
            if step in reset_at:  # reset(): new placement, lock tracking cleared, the row count starts over
                pos, goal = rng.integers(0, side, (N, 2)), rng.integers(0, side, (N, 2))
                moved[:], down[:], rows = 0, 0, []
            d_before = np.abs(goal - pos).sum(1)
            new = np.clip(pos + MOVES[rng.integers(0, 5, N)], 0, side - 1)
            mv = (new != pos).any(1)
            pos = new
            d = np.abs(goal - pos).sum(1)
            moved = ((moved << np.uint64(1)) | mv.astype(np.uint64)) & np.uint64(0xFFFF)
            down = ((down << np.uint64(1)) | (mv & (d < d_before)).astype(np.uint64)) & np.uint64(0xFFFF)
            rows.append(d.astype(np.int16))
            t = len(rows)
            ring = np.zeros((lw, N), np.int16)  # the numeric ring as the reference keeps it: slot = row index mod lw
            for k in range(min(t, lw)):
                ring[(t - 1 - k) % lw] = rows[t - 1 - k]
            short += t < lw
            full += t >= lw
            ok, bits = lib_from_ring(L, ring, lw, t, pos, goal, moved)
            ok_np, bits_np = np_from_ring(ring, lw, t, pos, goal, moved)
            assert ok and ok_np, (walk, step)
            assert np.array_equal(bits, bits_np), (walk, step)
            n = min(t, lw)
            keep = np.uint64((1 << max(n - 1, 0)) - 1)  # the step that wrote the oldest row has no row before it
            assert np.array_equal(bits.astype(np.uint64), down & keep), (walk, step)
            back = lib_to_ring(L, bits, lw, t, pos, goal, moved)
            assert np.array_equal(back, ring), (walk, step)
            assert np.array_equal(np_to_ring(bits, lw, t, pos, goal, moved), ring), (walk, step)
            # the engine's own register (with the bits the ring cannot know) gives the same ring
            assert np.array_equal(lib_to_ring(L, down.astype(np.uint16), lw, t, pos, goal, moved), ring), (walk, step)
    assert short >= 10 and full >= 10, (short, full)  # histories shorter than the window, and full ones


def test_no_history_gives_an_empty_ring_and_no_bits():
    L = _lib()
    pos, goal = np.array([[1, 1], [2, 5]]), np.array([[4, 4], [0, 0]])
    moved = np.array([0xFFFF, 0x1234], np.uint64)
    ok, bits = lib_from_ring(L, np.full((16, 2), 9, np.int16), 16, 0, pos, goal, moved)
    assert ok and not bits.any()
    assert not lib_to_ring(L, np.array([0xFFFF, 1], np.uint16), 16, 0, pos, goal, moved).any()


def _flat_case():
    """Two agents, five rows of history with window 8: agent 0 walked 6, 5, 4, 4, 3 towards its goal, agent 1 stood still."""
    lw, t = 8, 5
    pos, goal = np.array([[0, 3], [7, 7]]), np.array([[0, 0], [7, 5]])
    rows = np.array([[6, 2], [5, 2], [4, 2], [4, 2], [3, 2]], np.int16)
    ring = np.zeros((lw, 2), np.int16)
    ring[:t] = rows
    # bit k = the step that wrote the row k back moved: 4 -> 3 (bit 0), 4 -> 4 stood (bit 1), 5 -> 4, 6 -> 5, ? -> 6
    moved = np.array([0b11101, 0], np.uint64)
    return lw, t, pos, goal, ring, moved


def test_the_crafted_walk_is_representable():
    L = _lib()
    lw, t, pos, goal, ring, moved = _flat_case()
    ok, bits = lib_from_ring(L, ring, lw, t, pos, goal, moved)
    assert ok and np_from_ring(ring, lw, t, pos, goal, moved)[0]
    assert bits.tolist() == [0b1101, 0], bits  # every move of the four known steps went down; the oldest step is unknown
    assert np.array_equal(lib_to_ring(L, bits, lw, t, pos, goal, moved), ring)


def test_a_jump_of_three_is_not_representable():
    L = _lib()
    lw, t, pos, goal, ring, moved = _flat_case()
    ring[1, 0] = 7  # 6, 7, 4: the step from row 1 to row 2 would have covered three cells
    assert not lib_from_ring(L, ring, lw, t, pos, goal, moved)[0]
    assert not np_from_ring(ring, lw, t, pos, goal, moved)[0]


def test_a_ring_that_disagrees_with_the_moved_bits_is_not_representable():
    L = _lib()
    lw, t, pos, goal, ring, moved = _flat_case()
    still = moved.copy()
    still[0] = 0b11001  # says: no move between rows 1 and 2 -- the ring steps from 5 to 4 there
    assert not lib_from_ring(L, ring, lw, t, pos, goal, still)[0]
    assert not np_from_ring(ring, lw, t, pos, goal, still)[0]
    walked = moved.copy()
    walked[1] = 0b00010  # says agent 1 moved, its distance did not change
    assert not lib_from_ring(L, ring, lw, t, pos, goal, walked)[0]
    assert not np_from_ring(ring, lw, t, pos, goal, walked)[0]


def test_a_newest_row_that_is_not_the_current_distance_is_not_representable():
    L = _lib()
    lw, t, pos, goal, ring, moved = _flat_case()
    pos = pos.copy()
    pos[0] = (2, 3)  # moved by hand: two cells further from the goal than the newest row says
    assert not lib_from_ring(L, ring, lw, t, pos, goal, moved)[0]
    assert not np_from_ring(ring, lw, t, pos, goal, moved)[0]
