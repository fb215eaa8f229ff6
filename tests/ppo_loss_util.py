"""What the PPO objective tests share: the objective with the KL penalty written out in elementary float64 torch ops with
the gradient by autograd (``ppo_terms`` / ``oracle``), the learner's own fp32 torch statement on the CPU (``torch_path32``,
which defines ``dev``), a deterministic generator of synthetic cases with the conditions it must meet, and the margins.
The oracle shares no code with learner.py; only ``torch_path32`` calls into it."""

from __future__ import annotations

import functools

import numpy as np
import torch

NUM_ACTIONS = 5
MASK_EPS = 1e-6
TILE_ROWS = 32  # MAPF_PPO_TILE_ROWS: rows of one group per workgroup, hence per partial
CHUNK = 32  # MAPF_PPO_CHUNK: steps the kernel takes per chunk
LOSS_TERMS = ("total_loss", "policy_loss", "vf_loss", "entropy", "kl")
# nothing is switched off: both clips bind on a good share of the elements, both coefficients and the KL term are on
SETTINGS = {"clip": 0.2, "vf_clip": 0.8, "vf_coeff": 0.7, "ent_coeff": 0.03, "kl_coeff": 0.2}
# the reference's: src/agents/ppo.py over RLlib's defaults (vf_clip 10 hardly ever binds on errors ~ N(0, 1))
REFERENCE = {"clip": 0.05, "vf_clip": 10.0, "vf_coeff": 0.5, "ent_coeff": 0.001, "kl_coeff": 0.2}
RATIO_BAND, ERROR_BAND = 2e-3, 4e-3  # no element nearer than this to a boundary at which the gradient jumps

# What the kernel returns, by kind.  A GPU result may deviate from the float64 oracle by a margin times ``dev``, the
# deviation of the learner's fp32 torch path on the CPU from the same oracle: the next power of two at or above twice the
# largest ratio measured over all cases of tests/test_ppo_loss_gpu.py on the GPU (DESIGN.md 4y holds the table,
# profiles/r22/ppo/parity_deviation.txt the raw ratios).  The four summed terms are compared as the kernel returns them, one
# partial per 32-row tile of one group: [tiles, 4] sums of -s, v, H and KL over the tile's (t, row), against the same sums
# of the oracle and of the fp32 torch path on those rows.
ELEMENTWISE = ("logp", "kl", "dlogits", "dvalues")
SUMMED = ("policy_loss", "vf_loss", "entropy", "kl_mean")
QUANTITIES = ELEMENTWISE + ("partials",)
# largest ratios measured: logp 2.45, kl 1.26, dlogits 2.81 (all three at T = 2, 33 rows, 64 heads: a row's logp is a sum
# over 64 heads, which the kernel adds head by head and torch pairwise), dvalues 1.76, partials 2.12.  Over LONG_SHAPES below
# (fragments of one 32-step chunk and beyond, profiles/r23/long_fragments/parity_deviation.txt): logp 2.48, kl 1.29, dlogits 2.55,
# dvalues 1.69, partials 2.86 (one full chunk at the reference's settings; a thread's share of a partial is a serial sum over
# up to 65 steps there, and dev grows with it): twice each is inside the same margins, no long case has one of its own
MARGINS = {"logp": 8, "kl": 4, "dlogits": 8, "dvalues": 4, "partials": 8}
# Loss terms and parameter gradient of a module on a real fragment (tests/test_ppo_kl_gpu.py), what the GEMMs before and
# after the kernel sum: largest ratio measured 2.05 (the gradient on the joint fragment, both paths; loss terms at most
# 1.80, one policy per agent): 2 x 2.05 = 4.1; on fragments of T = 40 loss terms 1.76, gradient 2.65 (one policy per agent,
# both paths): 2 x 2.65 = 5.3
GEMM_MARGIN = 8


def group_coeffs(groups: int, base: float) -> np.ndarray:
    """The KL coefficients of a case: ``base`` for one group, distinct values from it upwards for more."""
    return (base + 0.15 * np.arange(groups)).astype(np.float32)


def ppo_terms(logits, values, old_logits, actions, old_logp, adv, targets, kl_coeff, hp: dict, groups: int = 1) -> dict:
    """The objective in elementary torch ops in the dtype of ``logits`` [T, R, 5 heads] and ``values`` [T, R] (which may
    require grad).  old_logits as logits, or None with kl_coeff None; actions [T, R, heads]; old_logp, adv, targets [T, R];
    kl_coeff [groups] or None.  Row r is group r % groups; every term is a [groups] tensor of group means and total_loss
    their weighted sum added over the groups.  Also the elementwise logp, kl, surrogate, clipped error and entropy."""
    T, R = values.shape
    heads = actions.shape[2]
    dt = logits.dtype

    def log_softmax(z):
        z = z.reshape(T, R, heads, NUM_ACTIONS)
        x = z - z.max(dim=3, keepdim=True).values.detach()
        return x - torch.log(torch.exp(x).sum(dim=3, keepdim=True))

    lp_all = log_softmax(logits)
    p_all = torch.exp(lp_all)
    taken = (actions.reshape(T, R, heads, 1).to(torch.int64) == torch.arange(NUM_ACTIONS)).to(dt)
    logp = (lp_all * taken).sum(dim=3).sum(dim=2)
    entropy = -(p_all * lp_all).sum(dim=3).sum(dim=2)
    if kl_coeff is None:
        kl = torch.zeros_like(logp)
        coeff = torch.zeros(groups, dtype=dt)
    else:
        lq_all = log_softmax(old_logits)
        kl = (torch.exp(lq_all) * (lq_all - lp_all)).sum(dim=3).sum(dim=2)
        coeff = kl_coeff.to(dt)
    ratio = torch.exp(logp - old_logp)
    surrogate = torch.minimum(adv * ratio, adv * torch.clamp(ratio, 1.0 - hp["clip"], 1.0 + hp["clip"]))
    err = (values - targets) * (values - targets)
    clipped = torch.clamp(err, max=hp["vf_clip"])
    n = T * R // groups

    def gmean(x):
        return x.reshape(T, R // groups, groups).sum(dim=(0, 1)) / n

    policy_loss, vf_loss, ent, klm = -gmean(surrogate), gmean(clipped), gmean(entropy), gmean(kl)
    total = (policy_loss + hp["vf_coeff"] * vf_loss - hp["ent_coeff"] * ent + coeff * klm).sum()
    return {"total_loss": total, "policy_loss": policy_loss, "vf_loss": vf_loss, "entropy": ent, "kl_mean": klm, "logp": logp,
            "kl": kl, "ratio": ratio, "err": err, "el": {"policy_loss": -surrogate, "vf_loss": clipped, "entropy": entropy, "kl_mean": kl}}


def _tensors(inp: dict, dtype):
    t = {k: (None if v is None else torch.from_numpy(v)) for k, v in inp.items()}
    return {k: (v.to(dtype) if v is not None and v.is_floating_point() else v) for k, v in t.items()}


def oracle(inp: dict, hp: dict, groups: int = 1) -> dict:
    """Every quantity of QUANTITIES but the partials (and the loss terms per group) from ``ppo_terms`` in float64, as NumPy."""
    t = _tensors(inp, torch.float64)
    logits, values = t["logits"].requires_grad_(True), t["values"].requires_grad_(True)
    out = ppo_terms(logits, values, t["old_logits"], t["actions"], t["old_logp"], t["adv"], t["targets"], t["kl_coeff"], hp, groups)
    dlogits, dvalues = torch.autograd.grad(out["total_loss"], [logits, values])
    res = {k: out[k].detach().numpy() for k in ("logp", "kl", "ratio", "err") + SUMMED}
    res.update(total_loss=float(out["total_loss"].detach()), dlogits=dlogits.numpy(), dvalues=dvalues.numpy(),
               el={k: v.detach().numpy() for k, v in out["el"].items()})
    return res


def torch_path32(inp: dict, hp: dict, groups: int = 1) -> dict:
    """The same quantities from the learner's own ``fused_objective=False`` statement in fp32 on the CPU
    (``learner.ppo_objective``, gradients by autograd), as float64 NumPy: what ``dev`` is measured with."""
    from dl_reference_models_amd import learner as ln

    t = _tensors(inp, torch.float32)
    logits, values = t["logits"].clone().requires_grad_(True), t["values"].clone().requires_grad_(True)
    per, extra = ln.ppo_objective(logits, values, t["actions"], t["old_logp"], t["adv"], t["targets"], hp["clip"], hp["vf_clip"],
                                  hp["vf_coeff"], hp["ent_coeff"], t["old_logits"], t["kl_coeff"], groups, True)
    dlogits, dvalues = torch.autograd.grad(per["total_loss"].sum(), [logits, values])
    zero = torch.zeros_like(extra["logp"])
    res = {"logp": extra["logp"], "kl": zero if extra["kl"] is None else extra["kl"], "dlogits": dlogits, "dvalues": dvalues,
           "policy_loss": per["policy_loss"], "vf_loss": per["vf_loss"], "entropy": per["entropy"],
           "kl_mean": per.get("kl", torch.zeros_like(per["entropy"]))}
    res = {k: v.detach().double().numpy() for k, v in res.items()}
    res["total_loss"] = float(per["total_loss"].sum().detach())
    return res


def tiles_of(rows: int, groups: int) -> list:
    """The row indices of every tile, in the order of the partials: group-major, 32 rows of one group each."""
    per = rows // groups
    return [g + groups * np.arange(a, min(a + TILE_ROWS, per)) for g in range(groups) for a in range(0, per, TILE_ROWS)]


def _partials(fn, inp: dict, hp: dict, groups: int) -> np.ndarray:
    """[tiles, 4]: the four sums over every tile's rows and all t, from ``fn`` (oracle or torch_path32) on those rows alone."""
    T, R = inp["values"].shape
    out = []
    for idx in tiles_of(R, groups):
        g = int(idx[0]) % groups
        sub = {k: (None if v is None else v[g:g + 1] if k == "kl_coeff" else np.ascontiguousarray(v[:, idx])) for k, v in inp.items()}
        res = fn(sub, hp, 1)
        out.append([float(res[k][0]) * T * len(idx) for k in SUMMED])
    return np.array(out)


KINDS = ("plain", "overflow", "one_left")


def deviation(got32: dict, want: dict) -> dict:
    """``dev`` per quantity: the largest deviation of the fp32 torch statement from the oracle.  Where that statement has no
    number -- autograd multiplies a zero gradient by a ratio of +inf in the overflow case, which ``check_conditions`` pins
    to exactly those rows -- the largest over the elements where it has one; the kernel is compared on every element."""
    assert all(np.isfinite(np.asarray(want[k])).all() for k in QUANTITIES)
    return {k: float(np.nanmax(np.abs(np.asarray(got32[k]) - np.asarray(want[k])))) for k in QUANTITIES}


def make_inputs(T: int, rows: int, heads: int, groups: int = 1, kind: str = "plain", settings: str = "SETTINGS", seed: int = 0) -> dict:
    """float32 / int8 NumPy inputs of one case.  logits ~ N(0, 2^2), two of the five logits of a quarter of the (t, row, head)
    lowered by log(MASK_EPS) as the policy's mask term does; old_logits = logits + N(0, 0.3^2) (the same mask term); an
    unmasked action; old_logp = logp - d, d ~ N(0, 0.15^2); adv, values and targets - values ~ N(0, 1).  Any d nearer
    than RATIO_BAND to log(1 +- clip) is moved out of the band, and so is a squared value error nearer than ERROR_BAND to
    vf_clip: the gradient jumps there.  kl_coeff: ``group_coeffs``.
    overflow: where adv > 0, old_logp is 100 below logp, so the ratio exp(100) is +inf in fp32.  one_left: head 0 of every
    (t, row) has four of its five logits lowered -- by log(MASK_EPS) in both sets of logits in rows 0, 3, ..; by 200 in
    ``logits`` alone in rows 1, 4, .. and in ``old_logits`` alone in rows 2, 5, .. (there four probabilities are exactly 0 in
    fp32) -- and the action left was taken."""
    hp = {"SETTINGS": SETTINGS, "REFERENCE": REFERENCE}[settings]
    rng = np.random.default_rng(100003 * T + 101 * rows + heads + 13 * groups + 7 * KINDS.index(kind) + 1000 * seed
                                + (500 if settings == "REFERENCE" else 0))
    logits = 2.0 * rng.standard_normal((T, rows, heads, NUM_ACTIONS))
    masked = rng.random((T, rows, heads)) < 0.25
    for j in (1, 3):
        logits[..., j] += np.where(masked, np.log(MASK_EPS), 0.0)
    old_logits = logits + 0.3 * rng.standard_normal(logits.shape)
    actions = rng.integers(0, NUM_ACTIONS, size=(T, rows, heads)).astype(np.int8)
    actions[masked] = 2 * rng.integers(0, 3, size=int(masked.sum())).astype(np.int8)  # an unmasked action was taken
    if kind == "one_left":
        r3 = (np.arange(rows) % 3)[None, :, None]
        keep = rng.integers(0, NUM_ACTIONS, size=(T, rows))
        lowered = np.arange(NUM_ACTIONS)[None, None, :] != keep[..., None]
        base = 2.0 * rng.standard_normal((T, rows, NUM_ACTIONS))
        logits[:, :, 0, :] = base + np.where(lowered, np.where(r3 == 1, -200.0, np.log(MASK_EPS)), 0.0)
        old_logits[:, :, 0, :] = (base + 0.3 * rng.standard_normal(base.shape)
                                  + np.where(lowered, np.where(r3 == 2, -200.0, np.log(MASK_EPS)), 0.0))
        actions[:, :, 0] = keep
    logits = logits.astype(np.float32).reshape(T, rows, heads * NUM_ACTIONS)
    old_logits = old_logits.astype(np.float32).reshape(T, rows, heads * NUM_ACTIONS)
    lg = logits.astype(np.float64).reshape(T, rows, heads, NUM_ACTIONS)
    lp = lg - lg.max(axis=3, keepdims=True)
    lp = lp - np.log(np.exp(lp).sum(axis=3, keepdims=True))
    logp = np.take_along_axis(lp, actions.astype(np.int64)[..., None], axis=3)[..., 0].sum(axis=2)
    d = 0.15 * rng.standard_normal((T, rows))
    for edge in (np.log1p(hp["clip"]), np.log1p(-hp["clip"])):
        near = np.abs(d - edge) < 2 * RATIO_BAND
        d = np.where(near, edge + np.where(d >= edge, 2 * RATIO_BAND, -2 * RATIO_BAND), d)
    adv = rng.standard_normal((T, rows))
    if kind == "overflow":
        d = np.where(adv > 0, 100.0, d)
    values = rng.standard_normal((T, rows)).astype(np.float32)
    diff = rng.standard_normal((T, rows))
    root = np.sqrt(hp["vf_clip"])
    near = np.abs(diff * diff - hp["vf_clip"]) < 2 * ERROR_BAND
    diff = np.where(near, np.sign(diff) * np.sqrt(hp["vf_clip"] + np.where(np.abs(diff) >= root, 2, -2) * 2 * ERROR_BAND), diff)
    f32 = np.float32
    return {"logits": logits, "old_logits": old_logits, "actions": actions, "old_logp": (logp - d).astype(f32), "adv": adv.astype(f32),
            "values": values, "targets": (values.astype(np.float64) + diff).astype(f32),
            "kl_coeff": group_coeffs(groups, hp["kl_coeff"])}


def branches(res: dict, inp: dict, hp: dict) -> dict:
    """Which side of every boundary an element is on, from a result's ratio / err (or logp) in ITS precision."""
    if "ratio" in res:
        ratio, err = res["ratio"], res["err"]
    else:  # the fp32 statement: the ratio and the error as fp32 computes them
        with np.errstate(over="ignore"):
            ratio = np.exp((res["logp"].astype(np.float32) - inp["old_logp"]).astype(np.float32))
        err = (inp["values"] - inp["targets"]).astype(np.float32) ** 2
        hp = {k: np.float32(v) for k, v in hp.items()}
    one = ratio.dtype.type(1)
    return {"above": ratio > one + hp["clip"], "below": ratio < one - hp["clip"], "vclip": err > hp["vf_clip"]}


def check_conditions(c: dict) -> dict:
    """The conditions a case must meet before anything is compared (assertions, not measurements); returns the shares.
    Every case: no element is excluded from any comparison (nothing here masks one), the fp32 CPU statement is on the same
    side of all three boundaries as the float64 oracle in every element, and no element is inside a guard band.  The
    plain and one_left cases at SETTINGS also: zero policy gradient on >= 5 % of the elements, the ratio above 1 + clip on
    >= 5 % and below 1 - clip on >= 3 %, the value clip binding on 20 .. 50 %.  (The overflow case moves half the ratios
    to +inf and REFERENCE's vf_clip of 10 is RLlib's, which errors ~ N(0, 1) hardly reach: the shares are not theirs.)"""
    inp, hp, want = c["inp"], c["hp"], c["want"]
    b64, b32 = branches(want, inp, hp), branches(c["got32"], inp, hp)
    for k in b64:
        assert np.array_equal(b64[k], b32[k]), (k, int((b64[k] != b32[k]).sum()))
    for k in QUANTITIES:  # the fp32 statement has a number everywhere, but for the gradient behind a ratio of +inf
        nan = np.isnan(np.asarray(c["got32"][k]))
        if nan.any():
            with np.errstate(over="ignore"):
                inf32 = np.isinf(np.exp((want["logp"] - inp["old_logp"]).astype(np.float32)))
            assert c["kind"] == "overflow" and k == "dlogits" and np.array_equal(nan.all(axis=2), inf32) and not nan[~inf32].any()
    logr = np.log(want["ratio"])
    gap_ratio = min(float(np.abs(logr - np.log1p(s * hp["clip"])).min()) for s in (1, -1))
    gap_err = float(np.abs(want["err"] - hp["vf_clip"]).min())
    assert gap_ratio >= RATIO_BAND and gap_err >= ERROR_BAND, (gap_ratio, gap_err)
    adv = inp["adv"]
    zero = (b64["above"] & (adv > 0)) | (b64["below"] & (adv < 0))
    shares = {"zero_grad": float(zero.mean()), "above": float(b64["above"].mean()), "below": float(b64["below"].mean()),
              "vclip": float(b64["vclip"].mean()), "gap_ratio": gap_ratio, "gap_err": gap_err}
    if c["kind"] != "overflow" and c["settings"] == "SETTINGS":
        assert shares["zero_grad"] >= 0.05 and shares["above"] >= 0.05 and shares["below"] >= 0.03, shares
        assert 0.2 <= shares["vclip"] <= 0.5, shares
    return shares


@functools.lru_cache(maxsize=None)
def case(T: int, rows: int, heads: int, groups: int = 1, kind: str = "plain", settings: str = "SETTINGS", kl: bool = True) -> dict:
    """Inputs, the float64 oracle and ``dev`` per quantity of one case, its conditions checked; computed once, shared: treat
    as read-only.  kl False: no coefficient and no behaviour logits (the call without the KL term)."""
    hp = {"SETTINGS": SETTINGS, "REFERENCE": REFERENCE}[settings]
    inp = make_inputs(T, rows, heads, groups, kind, settings)
    if not kl:
        inp = dict(inp, kl_coeff=None, old_logits=None)
    want, got32 = oracle(inp, hp, groups), torch_path32(inp, hp, groups)
    want["partials"], got32["partials"] = _partials(oracle, inp, hp, groups), _partials(torch_path32, inp, hp, groups)
    dev = deviation(got32, want)
    c = {"T": T, "rows": rows, "heads": heads, "groups": groups, "kind": kind, "settings": settings, "hp": hp, "inp": inp,
         "want": want, "got32": got32, "dev": dev}
    c["shares"] = check_conditions(c)
    return c


# (T, rows, heads, groups): a single step; a partial last tile; rows below one tile... of three heads; the largest head count;
# a group of exactly one tile; a group with a partial tile
SHAPES = ((1, 257, 1, 1), (2, 63, 3, 1), (5, 65, 16, 1), (2, 33, 64, 1), (3, 96, 1, 3), (2, 130, 1, 2))
# fragments of one chunk and beyond: exactly one full chunk on the one-head path with a one-row last tile; a full chunk and a
# one-step chunk, multi-head (pass C and both barriers around the reuse of s_g); three chunks, multi-head; the largest head
# count across a chunk edge (pass C's nT * vrows * heads at its largest); two full chunks, three groups of exactly one tile; a
# short second chunk, two groups with a one-row last tile each
LONG_SHAPES = ((32, 33, 1, 1), (33, 65, 3, 1), (65, 33, 16, 1), (33, 34, 64, 1), (64, 96, 1, 3), (40, 130, 1, 2))
assert CHUNK == 32  # the lengths above are stated against it


def reversed_in_time(inp: dict) -> dict:
    """The inputs of a case with t running backwards (the coefficients have no t)."""
    return {k: (v if v is None or k == "kl_coeff" else np.ascontiguousarray(v[::-1])) for k, v in inp.items()}


def time_slice(inp: dict, a: int, b: int) -> dict:
    """Steps a .. b - 1 of the inputs of a case."""
    return {k: (v if v is None or k == "kl_coeff" else np.ascontiguousarray(v[a:b])) for k, v in inp.items()}
