"""What the behaviour-cloning tests share: the objective and its closed-form gradients written out in elementary float64
NumPy (``bc_terms`` / ``oracle``), the learner's own fp32 torch statement on the CPU (``torch_path32``, which defines
``dev``), a deterministic generator of synthetic cases of five kinds, and the margins.  The oracle shares no code with
learner.py; only ``torch_path32`` calls into it."""

from __future__ import annotations

import functools

import numpy as np
import torch

import ppo_loss_util as plu
from dqn_util import floor_dev

NUM_ACTIONS = 5
MASK_EPS = 1e-6
TILE_ROWS = 32  # MAPF_BC_TILE_ROWS: rows of one group per workgroup, hence per partial
CHUNK = 32  # MAPF_BC_CHUNK: steps the kernel takes per chunk
assert (TILE_ROWS, CHUNK) == (plu.TILE_ROWS, plu.CHUNK)  # the shapes below are ppo_loss_util's, stated against its tile and chunk
# both coefficients on, so that every term reaches the gradients
SETTINGS = {"vf_coeff": 0.7, "ent_coeff": 0.03}

# (T, rows, heads, groups): ppo_loss_util's edges (a single step; a partial last tile; fewer rows than a tile, three heads; the
# largest head count; a group of exactly one tile; a group with a one-row tile tail) and the smallest call there is
SHAPES = plu.SHAPES + ((1, 1, 1, 1),)
LONG_SHAPES = plu.LONG_SHAPES  # T = 32, 33, 64, 65 and 40: the chunk edges
KINDS = ("plain", "saturated", "masked", "bad_action", "ties")

# What the kernel returns.  ``hits`` (the fourth column of the partials) is compared exactly.  Every other tensor may deviate
# from the float64 oracle by a margin times ``dev``, the deviation of the learner's fp32 torch path on the CPU
# (learner.bc_objective) from the same oracle, floored at half an ulp of the largest magnitude (dqn_util.floor_dev).  The
# three summed terms are compared as the kernel returns them, one partial per 32-row tile of one group: [tiles, 3] sums of
# nll, v and H over the tile's (t, row).
ELEMENTWISE = ("nll", "dlogits", "dvalues")
SUMMED = ("nll_mean", "vf_loss", "entropy")
QUANTITIES = ELEMENTWISE + ("partials",)
# Largest kernel error / dev measured on the MI355X over every case of tests/test_bc_loss_gpu.py (DESIGN.md 4z holds the
# table, profiles/r24/bc/parity_deviation.txt the raw lines); each margin is the next power of two above its ratio, at least 2
# nll 3.29 (T = 2, 33 rows, 64 heads: a row's nll is a sum over 64 heads, which the kernel adds head by head and torch
# pairwise; 2.82 at T = 33, 34 rows, 64 heads), dlogits 1.94 (the one-element call, where dev is its floor), dvalues 1.65
# (T = 33, 65 rows, 3 heads), partials 1.48 (T = 65, 33 rows, 16 heads)
MEASURED = {"nll": 3.29, "dlogits": 1.94, "dvalues": 1.65, "partials": 1.48}
MARGINS = {"nll": 4, "dlogits": 2, "dvalues": 2, "partials": 2}
# Loss terms and flat parameter gradient of a module on a real fragment (tests/test_bc_rollout_gpu.py), what the GEMMs before
# and after the kernel sum, measured and set the same way (ppo_loss_util.GEMM_MARGIN's convention): loss terms at most 1.00,
# gradient 2.43 (the joint fragment, fused objective)
GEMM_MEASURED = 2.43
GEMM_MARGIN = 4


def bc_terms(logits, expert, values=None, targets=None, vf_coeff: float = 0.0, ent_coeff: float = 0.0, groups: int = 1) -> dict:
    """The objective in elementary float64 NumPy.  logits [T, R, 5 heads]; expert [T, R, heads] (any bytes: clamped to
    0 .. 4); values, targets [T, R] or both None.  Row r is group r % groups; every term is a [groups] array of group means,
    total_loss their weighted sum added over the groups.  Also the elementwise nll, entropy, hits and value error, and the
    closed-form gradients of total_loss with respect to logits and values.  The argmax is taken on the logits as they come
    (no arithmetic), the lowest index on ties."""
    T, R, heads = expert.shape
    raw = np.asarray(logits).reshape(T, R, heads, NUM_ACTIONS)
    x = raw.astype(np.float64)
    z = x - x.max(axis=3, keepdims=True)
    lp = z - np.log(np.exp(z).sum(axis=3, keepdims=True))
    p = np.exp(lp)
    e = np.clip(expert.astype(np.int64), 0, NUM_ACTIONS - 1)
    onehot = (e[..., None] == np.arange(NUM_ACTIONS)).astype(np.float64)
    nll = -(lp * onehot).sum(axis=3).sum(axis=2)
    Hk = -(p * lp).sum(axis=3)  # (lp is finite, so p = 0 adds 0)
    top = np.full(e.shape, NUM_ACTIONS, np.int64)
    best = raw.max(axis=3)
    for j in range(NUM_ACTIONS - 1, -1, -1):
        top = np.where(raw[..., j] == best, j, top)
    hits = (top == e).sum(axis=2)
    n = T * R // groups
    c = 1.0 / n
    if values is None:
        assert targets is None
        v = np.zeros((T, R))
        dvalues = None
    else:
        d = values.astype(np.float64) - targets.astype(np.float64)
        v = 0.5 * d * d
        dvalues = c * vf_coeff * d
    dlogits = c * ((p - onehot) + ent_coeff * p * (lp + Hk[..., None]))

    def gmean(a):
        return a.reshape(T, R // groups, groups).sum(axis=(0, 1)) / n

    H = Hk.sum(axis=2)
    out = {"nll_mean": gmean(nll), "vf_loss": gmean(v), "entropy": gmean(H), "accuracy": gmean(hits.astype(np.float64)) / heads}
    out["total"] = out["nll_mean"] + vf_coeff * out["vf_loss"] - ent_coeff * out["entropy"]
    out.update(total_loss=float(out["total"].sum()), nll=nll, hits=hits, dlogits=dlogits.reshape(T, R, heads * NUM_ACTIONS),
               dvalues=dvalues, el={"nll_mean": nll, "vf_loss": v, "entropy": H})
    return out


def oracle(inp: dict, hp: dict, groups: int = 1) -> dict:
    res = bc_terms(inp["logits"], inp["expert"], inp["values"], inp["targets"], hp["vf_coeff"], hp["ent_coeff"], groups)
    if res["dvalues"] is None:
        res["dvalues"] = np.zeros(inp["expert"].shape[:2])  # (no such output: compared as 0 against 0 nowhere)
    return res


def torch_path32(inp: dict, hp: dict, groups: int = 1) -> dict:
    """The same quantities from the learner's own ``fused_objective=False`` statement in fp32 on the CPU
    (``learner.bc_objective``, gradients by autograd), as float64 NumPy: what ``dev`` is measured with."""
    from dl_reference_models_amd import learner as ln

    t = {k: (None if v is None else torch.from_numpy(v)) for k, v in inp.items()}
    logits = t["logits"].clone().requires_grad_(True)
    values = None if t["values"] is None else t["values"].clone().requires_grad_(True)
    per, extra = ln.bc_objective(logits, t["expert"], values, t["targets"], hp["vf_coeff"], hp["ent_coeff"], groups, True)
    grads = torch.autograd.grad(per["total_loss"].sum(), [logits] + ([] if values is None else [values]))
    res = {"nll": extra["nll"], "hits": extra["hits"], "dlogits": grads[0], "dvalues": grads[1] if values is not None else torch.zeros_like(extra["nll"]),
           "nll_mean": per["nll"], "vf_loss": per["vf_loss"], "entropy": per["entropy"], "accuracy": per["accuracy"]}
    res = {k: v.detach().double().numpy() for k, v in res.items()}
    res["total_loss"] = float(per["total_loss"].sum().detach())
    return res


tiles_of = plu.tiles_of


def _partials(fn, inp: dict, hp: dict, groups: int) -> np.ndarray:
    """[tiles, 3]: the three sums over every tile's rows and all t, from ``fn`` (oracle or torch_path32) on those rows alone."""
    T, R = inp["expert"].shape[:2]
    out = []
    for idx in tiles_of(R, groups):
        sub = {k: (None if v is None else np.ascontiguousarray(v[:, idx])) for k, v in inp.items()}
        res = fn(sub, hp, 1)
        out.append([float(res[k][0]) * T * len(idx) for k in SUMMED])
    return np.array(out)


def tile_hits(hits: np.ndarray, groups: int) -> np.ndarray:
    """[tiles]: the hit count of every tile, an integer."""
    return np.array([int(hits[:, idx].sum()) for idx in tiles_of(hits.shape[1], groups)], np.int64)


def deviation(got32: dict, want: dict) -> dict:
    """``dev`` per quantity: the largest deviation of the fp32 torch statement from the oracle, floored."""
    for k in QUANTITIES:
        assert np.isfinite(np.asarray(want[k])).all() and np.isfinite(np.asarray(got32[k])).all(), k
    return {k: floor_dev(float(np.abs(np.asarray(got32[k]) - np.asarray(want[k])).max()), want[k]) for k in QUANTITIES}


def make_inputs(T: int, rows: int, heads: int, groups: int = 1, kind: str = "plain", with_values: bool = True, seed: int = 0) -> dict:
    """float32 / int8 NumPy inputs of one case.  logits ~ N(0, 2^2); labels uniform over the five actions; values and
    targets - values ~ N(0, 1).
    saturated: one logit of every head of the odd rows is raised by 200, so the other four probabilities are exactly 0 in
      fp32; half of those heads are labelled with the raised action, half with another.
    masked: two of the five logits of a third of the (t, row, head) are lowered by log(MASK_EPS), as the policy's mask term
      does; a quarter of those heads are labelled with a masked action.
    bad_action: a third of the label bytes are outside 0 .. 4 (-128, -1, 5, 127).
    ties: the logits are multiples of 0.5, and in half of the heads the largest is copied onto another action, so that two
      (or more) top logits are exactly equal; the label is the lower of the two, the higher or neither."""
    rng = np.random.default_rng(100003 * T + 101 * rows + heads + 13 * groups + 7 * KINDS.index(kind) + 1000 * seed)
    logits = 2.0 * rng.standard_normal((T, rows, heads, NUM_ACTIONS))
    expert = rng.integers(0, NUM_ACTIONS, size=(T, rows, heads)).astype(np.int8)
    if kind == "saturated":
        up = rng.integers(0, NUM_ACTIONS, size=(T, rows, heads))
        odd = (np.arange(rows) % 2 == 1)[None, :, None] | (rows == 1)
        logits += np.where(odd[..., None] & (np.arange(NUM_ACTIONS) == up[..., None]), 200.0, 0.0)
        same = rng.random((T, rows, heads)) < 0.5
        expert = np.where(odd & same, up, expert).astype(np.int8)
    elif kind == "masked":
        masked = rng.random((T, rows, heads)) < 1 / 3
        for j in (1, 3):
            logits[..., j] += np.where(masked, np.log(MASK_EPS), 0.0)
        on_mask = masked & (rng.random((T, rows, heads)) < 0.25)
        free = 2 * rng.integers(0, 3, size=(T, rows, heads))
        expert = np.where(masked, np.where(on_mask, 1 + 2 * rng.integers(0, 2, size=(T, rows, heads)), free), expert).astype(np.int8)
    elif kind == "bad_action":
        wild = rng.random((T, rows, heads)) < 1 / 3
        expert = np.where(wild, rng.choice(np.array([-128, -1, 5, 127]), size=(T, rows, heads)), expert).astype(np.int8)
    elif kind == "ties":
        logits = np.round(2.0 * logits) / 2.0
        tie = rng.random((T, rows, heads)) < 0.5
        to = rng.integers(0, NUM_ACTIONS, size=(T, rows, heads))
        best = logits.max(axis=3)
        logits = np.where(tie[..., None] & (np.arange(NUM_ACTIONS) == to[..., None]), best[..., None], logits)
        expert = np.where(rng.random((T, rows, heads)) < 0.5, to, expert).astype(np.int8)
    values = rng.standard_normal((T, rows)).astype(np.float32)
    targets = (values.astype(np.float64) + rng.standard_normal((T, rows))).astype(np.float32)
    return {"logits": logits.astype(np.float32).reshape(T, rows, heads * NUM_ACTIONS), "expert": np.ascontiguousarray(expert),
            "values": values if with_values else None, "targets": targets if with_values else None}


def check_conditions(c: dict) -> dict:
    """What a case of a kind must show before anything is compared (assertions, not measurements); returns the shares."""
    inp, want = c["inp"], c["want"]
    T, R, heads = inp["expert"].shape
    lg = inp["logits"].reshape(T, R, heads, NUM_ACTIONS)
    top = lg.max(axis=3, keepdims=True)
    p32 = np.exp((lg - top).astype(np.float32))
    n_top = (lg == top).sum(axis=3)
    e = inp["expert"]
    shares = {"hit": float(want["hits"].sum()) / e.size, "tied": float((n_top > 1).mean()), "zero_p": float((p32 == 0).mean()),
              "wild": float(((e < 0) | (e > 4)).mean())}
    big = T * R * heads >= 60  # (the one-element case shows what it shows)
    if c["kind"] == "saturated":
        assert shares["zero_p"] > (0.3 if big else 0) and float(want["nll"].max()) > (150 if big else -1), shares
    elif c["kind"] == "masked":
        on_mask = np.take_along_axis(lg, np.clip(e, 0, 4).astype(np.int64)[..., None], axis=3)[..., 0] < top[..., 0] - 10
        shares["label_on_mask"] = float(on_mask.mean())
        assert not big or 0.02 < shares["label_on_mask"] < 0.3, shares
    elif c["kind"] == "bad_action":
        assert not big or 0.2 < shares["wild"] < 0.5, shares
    elif c["kind"] == "ties":
        ec = np.clip(e, 0, 4).astype(np.int64)
        label_is_top = np.take_along_axis(lg, ec[..., None], axis=3)[..., 0] == top[..., 0]
        first = np.argmax(lg == top, axis=3)
        shares["label_tied_not_lowest"] = float(((n_top > 1) & label_is_top & (first != ec)).mean())
        shares["label_tied_lowest"] = float(((n_top > 1) & (first == ec)).mean())
        assert not big or (shares["tied"] > 0.3 and shares["label_tied_not_lowest"] > 0.02 and shares["label_tied_lowest"] > 0.02), shares
    assert np.array_equal(c["got32"]["hits"].astype(np.int64), want["hits"])  # both pick the lowest index
    return shares


@functools.lru_cache(maxsize=None)
def case(T: int, rows: int, heads: int, groups: int = 1, kind: str = "plain", with_values: bool = True) -> dict:
    """Inputs, the float64 oracle and ``dev`` per quantity of one case, its conditions checked; computed once, shared: treat
    as read-only.  with_values False: the call without values and targets."""
    hp = SETTINGS
    inp = make_inputs(T, rows, heads, groups, kind, with_values)
    want, got32 = oracle(inp, hp, groups), torch_path32(inp, hp, groups)
    want["partials"], got32["partials"] = _partials(oracle, inp, hp, groups), _partials(torch_path32, inp, hp, groups)
    want["tile_hits"] = tile_hits(want["hits"], groups)
    dev = deviation(got32, want)
    c = {"T": T, "rows": rows, "heads": heads, "groups": groups, "kind": kind, "hp": hp, "inp": inp, "want": want, "got32": got32,
         "dev": dev, "with_values": with_values}
    c["shares"] = check_conditions(c)
    return c


def time_slice(inp: dict, a: int, b: int) -> dict:
    """Steps a .. b - 1 of the inputs of a case."""
    return {k: (None if v is None else np.ascontiguousarray(v[a:b])) for k, v in inp.items()}


def followed_share_bound(n: int, beta: float, sigmas: float = 5.0) -> float:
    """How far the share of set bytes among n independent draws with probability beta may lie from beta: ``sigmas`` standard
    deviations of the binomial share, sqrt(beta (1 - beta) / n).  Five of them are exceeded by one draw in 1.7 million."""
    return sigmas * float(np.sqrt(beta * (1.0 - beta) / n))
