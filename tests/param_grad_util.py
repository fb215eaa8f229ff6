"""What the tests of the fused parameter gradients share (include/mapf_step.h, "Fused parameter gradients of the learner").

The trunk's gradients are ``trunk_util``'s: ``trunk_case`` holds the float64 oracle of ``PARAM_GRADS`` and ``dev``, the deviation
of the same computation in fp32 on the CPU (the larger of two summation orders).  dW_hh is restated here from the header's
formula in NumPy -- nothing below imports the learner or the library -- in float64 (the oracle) and in float32, as one product
over all rows and as a sum of products over chunks of 1 000 rows (``dev``: the larger deviation of the two).

A GPU result may deviate from the float64 oracle by a margin times ``dev``.  The project's rule (learner_util.py,
trunk_util.py): the next power of two at or above twice the largest ratio measured on the MI355X over all cases of
tests/test_param_grad_gpu.py / tests/test_param_grad_learner_gpu.py; profiles/r29/param_grad/parity_ratios.txt holds every
line, DESIGN.md 4ad the table.  The reference of every ratio is the float64 oracle, never the kernel."""

from __future__ import annotations

import functools

import numpy as np

import trunk_util as tu

HIDDEN, GATES = 64, 256
SLAB_ROWS, MAX_SLABS = 1024, 256  # MAPF_PARAM_GRAD_SLAB_ROWS / _MAX_SLABS (tests/test_param_grad_host.py reads the header)

TRUNK_MARGIN = 8  # largest ratio measured: 2.91 (dw1, M = 1 023, F = 1, feed-forward): 2 x 2.91 = 5.8
DWHH_MARGIN = 8  # largest ratio measured: 2.22 (T = 5, 205 rows, every row of step 1 reset): 2 x 2.22 = 4.4
LEARNER_MARGIN = 8  # largest ratio measured: 2.84 (BCLearner's flat gradient, feed-forward fragment, as without the option): 2 x 2.84 = 5.7

S = SLAB_ROWS
TRUNK_ROWS = (1, 2, 3, 31, 32, 33, 65, S - 1, S, S + 1, 2 * S + 3)
CAPPED_ROWS = S * MAX_SLABS + 1
DWHH_SHAPES = ((1, 1, 1), (1, 33, 1), (2, 31, 1), (5, 64, 1), (3, 66, 2), (4, 63, 3), (32, 96, 16),
               (5, S // 5 + 1, 1),       # T R just above S
               (3, 2 * S // 3 + 2, 1))   # T R just above 2 S
DWHH_CAPPED = (5, -(-(S * MAX_SLABS + 1) // 5), 1)
RESETS = ("null", "zero", "quarter", "step1")
CHUNK = 1000


def slabs_of(rows: int) -> tuple:
    """(slab count, rows per slab) of ``rows`` rows of one group, restated from the header: slabs of SLAB_ROWS rows while that
    gives at most MAX_SLABS, otherwise ceil(rows / MAX_SLABS) rows rounded up to a multiple of 32."""
    ceil = lambda a, b: -(-a // b)  # noqa: E731
    per = SLAB_ROWS if ceil(rows, SLAB_ROWS) <= MAX_SLABS else 32 * ceil(ceil(rows, MAX_SLABS), 32)
    return ceil(rows, per), per


def trunk_pairs():
    """(M, (F, L), recurrent) pruned from the cross product: row count i meets feature shapes i and i + 2 (mod 5) recurrent
    and shapes i + 1 and i + 3 feed-forward, so every M and every (F, L) occurs with both kinds."""
    out = []
    n = len(tu.FEATURE_SHAPES)
    for i, M in enumerate(TRUNK_ROWS):
        for d, rec in ((0, True), (2, True), (1, False), (3, False)):
            out.append((M, tu.FEATURE_SHAPES[(i + d) % n], rec))
    return out


def trunk_kernel_inputs(case: dict) -> dict:
    """What mapf_trunk_param_grad reads, from the case: the oracle's a1, a2, dpre1, dpre2 rounded to fp32 (what the trunk kernels
    hand over, to their own margin), and prev_action / prev_reward of the rows that start an episode made unreadable: a byte
    of 77 and NaN (the oracle never looks at them)."""
    inp, want = case["inp"], case["want"]
    out = {k: np.ascontiguousarray(want[k], np.float32) for k in ("a1", "a2", "dpre1", "dpre2")}
    out["obs"] = inp["obs"]
    if inp["recurrent"]:
        started = inp["first"] != 0
        pa, pr = inp["prev_action"].copy(), inp["prev_reward"].copy()
        pa[started], pr[started] = 77, np.nan
        out.update(prev_action=pa, prev_reward=pr, first=inp["first"], dxg=inp["dxg"])
    return out


def trunk_dev(case: dict, q: str) -> float:
    """``dev`` of a parameter gradient, not below one fp32 rounding of the oracle's largest entry: the kernel is handed fp32
    roundings of a1 .. dpre2, and at one or two rows the CPU's own fp32 result can be exact by chance."""
    return max(case["dev"][q], 2.0 ** -24 * float(np.abs(case["want"][q]).max()))


def reset_pattern(kind: str, T: int, R: int, rng):
    if kind == "null":
        return None
    reset = np.zeros((T, R), np.uint8)
    if kind == "quarter":
        reset[rng.random((T, R)) < 0.25] = 1
        reset[:, 0] = 3  # row 0 of every step, t = 0 included; any non-zero byte counts
    elif kind == "step1" and T > 1:
        reset[1] = 1
    return reset


def dwhh_np(dxg, h, h0, reset, groups: int, dtype, chunked: bool = False) -> np.ndarray:
    """dWhh[g] = sum over t and r = g (mod groups) of dxg[t][r]^T hp[t][r]; hp[0] = h0, hp[t] = h[t-1], 0 where reset.
    chunked: the same sum in another order, one product per 1 000 rows, the products added one after the other."""
    T, R = dxg.shape[:2]
    hp = np.concatenate([h0[None], h[:-1]]).astype(dtype)
    if reset is not None:
        hp = np.where(reset[:, :, None] != 0, dtype(0), hp)
    out = np.zeros((groups, GATES, HIDDEN), dtype)
    for g in range(groups):
        p, q = dxg[:, g::groups].reshape(-1, GATES).astype(dtype), hp[:, g::groups].reshape(-1, HIDDEN)
        if chunked:
            n = len(p) // CHUNK * CHUNK
            parts = np.matmul(p[:n].reshape(-1, CHUNK, GATES).transpose(0, 2, 1), q[:n].reshape(-1, CHUNK, HIDDEN))
            for part in parts:
                out[g] += part
            out[g] += p[n:].T @ q[n:]
        else:
            out[g] = p.T @ q
    assert out.dtype == dtype
    return out.astype(np.float64)


@functools.lru_cache(maxsize=None)
def dwhh_case(T: int, R: int, groups: int, reset_kind: str) -> dict:
    """Inputs, the float64 oracle and ``dev`` of one dW_hh case; computed once, shared: treat as read-only.  h0 is not zero, so a
    reset missed at t = 0 shows."""
    rng = np.random.default_rng(104729 * T + 31 * R + 7 * groups)  # (the same dxg, h and h0 under every reset variant)
    f32 = np.float32
    inp = {"T": T, "R": R, "groups": groups, "dxg": rng.standard_normal((T, R, GATES)).astype(f32),
           "h": rng.uniform(-1, 1, (T, R, HIDDEN)).astype(f32), "h0": rng.uniform(0.25, 1, (R, HIDDEN)).astype(f32),
           "reset": reset_pattern(reset_kind, T, R, np.random.default_rng(T + R + RESETS.index(reset_kind)))}
    args = (inp["dxg"], inp["h"], inp["h0"], inp["reset"], groups)
    want = dwhh_np(*args, np.float64)
    dev = max(float(np.abs(dwhh_np(*args, np.float32, chunked=c) - want).max()) for c in (False, True))
    return {"inp": inp, "want": want, "dev": max(dev, 2.0 ** -24 * float(np.abs(want).max()))}
