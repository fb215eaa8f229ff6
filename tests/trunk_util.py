"""The dense trunk's rule (include/mapf_step.h, "Fused dense trunk of the learner") restated for the tests in NumPy: the
forward pass, and the backward pass by a hand-written chain rule with every parameter gradient, in float64 (the oracle) and
in float32 (``dev``: how far the same computation in fp32 on the CPU lies from the oracle, taken additionally with the hidden
units relabelled by a fixed permutation, i.e. in another summation order, as ``regime_util.lstm_case`` does), plus the cases
the tests share.  Nothing here imports the learner or the library; a case's weights are a freshly initialised module's."""

from __future__ import annotations

import functools

import numpy as np

HIDDEN = 64
GATES = 256
NUM_ACTIONS = 5
ZIN = HIDDEN + NUM_ACTIONS + 1

FORWARD = ("a1", "a2", "xg")
KERNEL_GRADS = ("dpre2", "dpre1")
PARAM_GRADS = ("dw1", "db1", "dw2", "db2", "dwih", "dbl")  # dbl: d / d bias_ih = d / d bias_hh
WEIGHTS = ("w1", "b1", "w2", "b2", "wih", "bih", "bhh")
REGIMES = ("fresh", "saturated", "large_obs", "wide_wih")
PERM_SEED = 4242

# (F, L): odd and even F, both ends of the range, with and without the 5 mask columns
FEATURE_SHAPES = ((1, 1), (2, 7), (11, 11), (53, 58), (125, 130))
# one row; one short of a tile; a tile; one past it; four tiles and a row (a ragged second workgroup half); more than one
# workgroup of 8 tiles with a ragged last tile
ROWS = (1, 31, 32, 33, 129, 4 * 32 * 3 + 5)

# A GPU result may deviate from the float64 oracle by a margin times ``dev``.  The project's rule (learner_util.py): the next
# power of two at or above twice the largest ratio measured over all cases of tests/test_trunk_gpu.py on the GPU, taken
# separately for what the forward kernel returns, for what the backward kernel returns and for what a GEMM after it sums, so
# that the GEMM's does not loosen the kernel's (DESIGN.md 4ac holds the table, profiles/r28/trunk/parity_ratios.txt the raw
# lines).  The existing margins of the same three roles are 16, 8 and 32 (learner_util.py).
FORWARD_MARGIN = 8  # largest ratio measured: 2.84 (xg, one row, F = 53; a2 2.68, a1 1.93): 2 x 2.84 = 5.7
KERNEL_GRAD_MARGIN = 16  # largest ratio measured: 5.01 (dpre2, one row, F = 2, recurrent; dpre1 2.81): 2 x 5.01 = 10.0
GRAD_MARGIN = 8  # largest ratio measured: 2.84 (BCLearner's flat gradient, feed-forward fragment; dense_trunk's own 1.00): 2 x 2.84 = 5.7


def margin_of(quantity: str) -> int:
    return FORWARD_MARGIN if quantity in FORWARD else KERNEL_GRAD_MARGIN if quantity in KERNEL_GRADS else GRAD_MARGIN


def side_columns(inp: dict, dtype) -> np.ndarray:
    """[M, 6]: onehot5 of the previous action and the previous reward, both 0 -- action 0 -- on a row that starts an episode;
    a byte outside 0 .. 4 sets no entry."""
    keep = inp["first"] == 0
    pa = np.where(keep, inp["prev_action"].astype(np.int64), 0)
    side = np.zeros((len(pa), NUM_ACTIONS + 1), dtype)
    for k in range(NUM_ACTIONS):
        side[:, k] = pa == k
    side[:, NUM_ACTIONS] = np.where(keep, inp["prev_reward"], 0).astype(dtype)
    return side


def trunk_np(inp: dict, dtype, perm=None) -> dict:
    """Every quantity of FORWARD, KERNEL_GRADS and PARAM_GRADS in ``dtype`` as float64 NumPy.  The upstream gradient is
    ``inp["dxg"]`` [M, 256] of a recurrent net, ``inp["da2"]`` [M, 64] of a feed-forward one.  perm: (p1, p2, pg), permutations
    of the units of fc1, fc2 and the gates -- the same computation with the units relabelled; results are permuted back."""
    rec, F = inp["recurrent"], inp["F"]
    w = {k: (None if inp[k] is None else inp[k].astype(dtype)) for k in WEIGHTS}
    up = inp["dxg" if rec else "da2"].astype(dtype)
    if perm is not None:
        p1, p2, pg = perm
        w["w1"], w["b1"] = w["w1"][p1], w["b1"][p1]
        w["w2"], w["b2"] = w["w2"][p2][:, p1], w["b2"][p2]
        if rec:
            cols = np.concatenate([p2, np.arange(HIDDEN, ZIN)])
            w["wih"], w["bih"], w["bhh"] = w["wih"][pg][:, cols], w["bih"][pg], w["bhh"][pg]
            up = up[:, pg]
        else:
            up = up[:, p2]
    x = inp["obs"][:, :F].astype(dtype)
    a1 = np.tanh(x @ w["w1"].T + w["b1"])
    a2 = np.tanh(a1 @ w["w2"].T + w["b2"])
    out = {"a1": a1, "a2": a2}
    if rec:
        z = np.concatenate([a2, side_columns(inp, dtype)], axis=1)
        out["xg"] = z @ w["wih"].T + (w["bih"] + w["bhh"])
        da2 = up @ w["wih"][:, :HIDDEN]
        out["dwih"], out["dbl"] = up.T @ z, up.sum(axis=0)
    else:
        da2 = up
    one = dtype(1)
    dpre2 = da2 * (one - a2 * a2)
    dpre1 = (dpre2 @ w["w2"]) * (one - a1 * a1)
    out.update(dpre2=dpre2, dpre1=dpre1, dw2=dpre2.T @ a1, db2=dpre2.sum(axis=0), dw1=dpre1.T @ x, db1=dpre1.sum(axis=0))
    assert all(v.dtype == dtype for v in out.values())
    if perm is not None:
        i1, i2, ig = (np.argsort(p) for p in perm)
        out["a1"], out["dpre1"], out["dw1"], out["db1"] = out["a1"][:, i1], out["dpre1"][:, i1], out["dw1"][i1], out["db1"][i1]
        out["a2"], out["dpre2"], out["dw2"], out["db2"] = out["a2"][:, i2], out["dpre2"][:, i2], out["dw2"][i2][:, i1], out["db2"][i2]
        if rec:
            cols = np.concatenate([i2, np.arange(HIDDEN, ZIN)])
            out["xg"], out["dwih"], out["dbl"] = out["xg"][:, ig], out["dwih"][ig][:, cols], out["dbl"][ig]
    return {k: v.astype(np.float64) for k, v in out.items()}


def quantities(recurrent: bool) -> tuple:
    return tuple(q for q in FORWARD + KERNEL_GRADS + PARAM_GRADS if recurrent or q not in ("xg", "dwih", "dbl"))


def flat_gradient(res: dict, recurrent: bool) -> np.ndarray:
    """The parameter gradients in the order of the module's trunk parameters: fc1.weight, fc1.bias, fc2.weight, fc2.bias,
    lstm.weight_ih, lstm.bias_ih, lstm.bias_hh."""
    parts = [res["dw1"], res["db1"], res["dw2"], res["db2"]] + ([res["dwih"], res["dbl"], res["dbl"]] if recurrent else [])
    return np.concatenate([np.asarray(p, np.float64).ravel() for p in parts])


def make_inputs(M: int, F: int, L: int, recurrent: bool, regime: str = "fresh", seed: int = 0) -> dict:
    """float32 / int8 / uint8 NumPy inputs of one case.  obs: 0 / 1 cells with three real-valued features, as the env's; the
    mask columns F .. L are NaN (a read past F shows); ``first`` on about a third of the rows; one prev_action byte of 7 and
    one of -1 (where there are rows for them).  Regimes: ``saturated`` -- every weight x 8, so pre-activations reach about +-20
    and 1 - a^2 is exactly 0 on part of the entries; ``large_obs`` -- the real-valued features of magnitude 1e3; ``wide_wih``
    -- W_ih uniform in +-1 and prev_reward up to +-50."""
    from policy_util import make_module

    assert regime in REGIMES and L in (F, F + NUM_ACTIONS)
    rng = np.random.default_rng(7919 * M + 131 * F + 17 * REGIMES.index(regime) + int(recurrent) + 1000003 * seed)
    f32 = np.float32
    module = make_module(L, L != F, recurrent, seed=F + seed)
    sd = {k: v.detach().numpy().astype(f32) for k, v in module.state_dict().items()}
    inp = {"M": M, "F": F, "L": L, "recurrent": recurrent, "regime": regime,
           "w1": sd["fc1.weight"], "b1": sd["fc1.bias"], "w2": sd["fc2.weight"], "b2": sd["fc2.bias"],
           "wih": sd.get("lstm.weight_ih"), "bih": sd.get("lstm.bias_ih"), "bhh": sd.get("lstm.bias_hh")}
    obs = rng.integers(0, 2, size=(M, L)).astype(f32)
    real = min(3, F)
    obs[:, :real] = rng.uniform(-1, 1, size=(M, real))
    if regime == "large_obs":
        obs[:, :real] *= f32(1e3)
    obs[:, F:] = np.nan
    inp["obs"] = obs
    if regime == "saturated":
        for k in WEIGHTS:
            if inp[k] is not None:
                inp[k] = inp[k] * f32(8)
    inp["prev_action"] = rng.integers(0, NUM_ACTIONS, size=M).astype(np.int8)
    if M >= 2:
        inp["prev_action"][M // 2] = 7
        inp["prev_action"][M - 1] = -1
    inp["prev_reward"] = rng.uniform(-1, 1, size=M).astype(f32)
    inp["first"] = (rng.random(M) < 1 / 3).astype(np.uint8)
    if M >= 2:
        inp["first"][M // 2], inp["first"][M - 1] = 0, 0  # (the two odd bytes are read)
    if M >= 3:
        inp["first"][0] = 2  # any non-zero byte counts
    if regime == "wide_wih" and recurrent:
        inp["wih"] = rng.uniform(-1, 1, size=(GATES, ZIN)).astype(f32)
        inp["prev_reward"] = rng.uniform(-50, 50, size=M).astype(f32)
    inp["dxg"] = rng.standard_normal((M, GATES)).astype(f32) if recurrent else None
    inp["da2"] = None if recurrent else rng.standard_normal((M, HIDDEN)).astype(f32)
    return inp


@functools.lru_cache(maxsize=None)
def trunk_case(M: int, F: int, L: int, recurrent: bool, regime: str = "fresh", seed: int = 0) -> dict:
    """Inputs, the float64 oracle and ``dev`` per quantity of one case; computed once, shared: treat as read-only.  The NaN
    mask columns never enter: the oracle reads obs[:, :F]."""
    inp = make_inputs(M, F, L, recurrent, regime, seed)
    want = trunk_np(inp, np.float64)
    prng = np.random.default_rng(PERM_SEED)
    perm = (prng.permutation(HIDDEN), prng.permutation(HIDDEN), prng.permutation(GATES))
    plain32, perm32 = trunk_np(inp, np.float32), trunk_np(inp, np.float32, perm)
    qs = quantities(recurrent)
    dev_plain = {q: float(np.abs(plain32[q] - want[q]).max()) for q in qs}
    dev_perm = {q: float(np.abs(perm32[q] - want[q]).max()) for q in qs}
    dev = {q: max(dev_plain[q], dev_perm[q]) for q in qs}
    g_want = flat_gradient(want, recurrent)
    g_dev = max(float(np.abs(flat_gradient(r, recurrent) - g_want).max()) for r in (plain32, perm32))
    return {"inp": inp, "want": want, "dev": dev, "dev_plain": dev_plain, "dev_perm": dev_perm, "gradient": g_want,
            "gradient_dev": g_dev}


def ratio(err: float, dev: float) -> float:
    """err / dev; 0 where both are 0 (a quantity that is exact in every precision, such as a saturated tanh)."""
    return 0.0 if err == 0 else float("inf") if dev == 0 else err / dev


def load_module(module, inp: dict):
    """The case's weights into a ``MaskedRecurrentPolicy`` of its shape (the heads keep their own)."""
    import torch

    names = {"w1": "fc1.weight", "b1": "fc1.bias", "w2": "fc2.weight", "b2": "fc2.bias", "wih": "lstm.weight_ih",
             "bih": "lstm.bias_ih", "bhh": "lstm.bias_hh"}
    with torch.no_grad():
        for k, name in names.items():
            if inp[k] is not None:
                dict(module.named_parameters())[name].copy_(torch.from_numpy(inp[k]))
    return module
