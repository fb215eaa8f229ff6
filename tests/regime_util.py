"""Cases beyond a freshly initialised net, for both act kernels and the LSTM sequence kernels, shared by the host and the
GPU tests.  The existing parity cases (policy_util, joint_policy_util, learner_util) run a network as nn.Linear /
nn.LSTMCell initialise it, from a zero state: logits of a few tenths, gate pre-activations inside +-5.  Here the same
modules are scaled (``scale_params``) until gates saturate and logits pass the range of fp32 ``exp``, masks are 0 or 0.5
on whole rows, and the paths the ABI states but no parity case walks (both start arrays, prev_action bytes outside 0..4,
draw counters at the top of their range, seeds with the top bit set) get a case each.

Every case is UNCHAINED: each step of every evaluation (the float64 restatement, the fp32 CPU module, the fp32
other-order evaluation, the device) starts from the restatement's state of the step before, rounded to fp32, so a step's
deviation is that step's alone and ``dev`` measures one step, not six steps of amplification through a high-gain net.
``dev`` is the larger of the fp32 CPU module's deviation from the restatement and that of ``fp32_other_order``; both come
from the reference side, neither from the code under test.

Kind ``"wide"`` is the 256-256 feed-forward joint net of the wide act kernel (wide_joint_util.make_module) on the geometry
of ``"joint"``: its own entry in the rng key, so its inputs are not the joint ones, and feed-forward only.

``compare`` holds the assertions of the GPU parity tests; the host test runs it on the float32 restatement
(``restate32``) and on four mutants of it, so every gap named above is shown closed without a GPU.

Nothing here imports the library (the modules come through policy_util.make_module / joint_policy_util.make_module)."""

from __future__ import annotations

import functools

import numpy as np

import joint_policy_util as ju
import learner_util as lu
import policy_util as pu

HIDDEN = 64
NUM_ACTIONS = 5
STEPS = 6
START_STEPS = pu.START_STEPS
DEFAULT_SEED = 11

# name -> (body, head): the factor on every tensor but the heads', and the factor on pi.* / vf.*
REGIMES = {"default": (1, 1),  # today's regime, for reference
           "hot": (4, 16),  # gates partly saturated, |logit| up to about 25
           "saturated": (8, 64),  # |h| reaches 1.000, |logit| up to about 70
           "peaked": (8, 256)}  # |logit| 170 - 290: past the range of fp32 exp
NEW_REGIMES = ("hot", "saturated", "peaked")
AGENT_SHAPES = ((65, 5, 33, True), (96, 16, 52, False))  # (rows, agents per env, L, mask), from policy_util.SHAPES
JOINT_SHAPES = ((33, 5, 7, 3), (65, 16, 16, 4), (34, 32, 32, 16))  # (rows, H, W, N), from joint_policy_util.SHAPES
# one of joint_policy_util.SPLIT_SHAPES, recurrent and sampled in the "hot" regime only: a partly filled quarter of fc1's K in
# wave 2 of the second staging buffer, eight full head tiles, 128 extra k-steps of the gates
JOINT_SPLIT_SHAPE = (7, 20, 20, 51)
JOINT_SPLIT_CASE = ("joint", JOINT_SPLIT_SHAPE, "hot", True, True, None)  # the key of ``case``
# kind "wide": the 256-256 feed-forward joint net (wide_joint_util.make_module) with the geometry of "joint": those three,
# and one whose fc1 walk ends in an odd tail behind its loop (wide_joint_util.fc1_groups: 3 groups)
WIDE_SHAPES = JOINT_SHAPES + ((33, 9, 9, 2),)
KINDS = ("agent", "joint", "wide")  # the position is the kind's entry in a case's rng key
ABI_SHAPE = {"agent": (65, 5, 33, True), "joint": (65, 16, 16, 4), "wide": (65, 16, 16, 4)}
FEED_FORWARD_SHAPE = ABI_SHAPE
VARIANTS = ("both_starts", "bad_bytes", "counters", "seeds")
BAD_BYTES = (-128, -1, 5, 127)
TOP_COUNTERS = (0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF)
TOP_SEEDS = (0xFFFFFFFFFFFFFFFF, 0x8000000000000001)
MAX_UNDECIDED_AGENT_ROWS = 0.01  # test_policy_gpu's cap
# (kind, shape, regime, recurrent, sample, variant) -> noise seed, for a case that DEFAULT_SEED would land above a cap.
# Seed 11 keeps every case used by the tests under its caps (test_regimes_host prints the shares), so the table is empty.
CASE_SEEDS = {}


def scale_params(module, body: float, head: float):
    """In place: pi.* and vf.* times ``head``, every other tensor (biases included) times ``body``."""
    import torch

    with torch.no_grad():
        for name, v in module.state_dict().items():
            v.mul_(head if name.startswith(("pi.", "vf.")) else body)
    return module


def _util(kind: str):
    return {"agent": pu, "joint": ju, "wide": ju}[kind]  # the feed-forward rule of joint_policy_util has no width in it


def geometry(kind: str, shape):
    """(rows, N decisions per row, rows per start flag, observation length)."""
    if kind == "agent":
        rows, n, L, _mask = shape
        return rows, 1, n, L
    rows, H, W, N = shape
    return rows, N, 1, H * W + NUM_ACTIONS * N


def start_rows(kind: str, shape, sa, sb, only_a: bool = False):
    """bool [rows]: the rule's episode start, the OR of the two optional flag arrays (per env for the per-agent policy, per
    row for the joint one).  ``only_a``: the mutant that looks at start_a alone when both are given."""
    rows, _N, per, _L = geometry(kind, shape)
    s = np.zeros(rows // per, bool)
    if sa is not None:
        s |= np.asarray(sa) != 0
    if sb is not None and not (only_a and sa is not None):
        s |= np.asarray(sb) != 0
    return np.repeat(s, per)


def noise(kind: str, seed: int, rows: int, draws, N: int, counter_bits: int = 32):
    """Gumbel noise [rows, 5 N] of the rule for draw counters ``draws`` (uint32)."""
    d = np.asarray(draws, np.uint64) & np.uint64((1 << counter_bits) - 1)
    return pu.gumbel_np(seed, np.arange(rows), d) if kind == "agent" else ju.gumbel_np(seed, np.arange(rows), d, N)


def logp_of(logits, actions):
    """Summed log-probability [R] of actions [R] or [R, N] under float64 logits [R, 5 N]."""
    R = logits.shape[0]
    return ju.logp_of(logits, np.asarray(actions).reshape(R, -1))


def choose(logits, g=None):
    """actions [R, N], summed logp [R], gap [R, N] from float64 logits [R, 5 N] (joint_policy_util.choose)."""
    return ju.choose(logits, g)


# ---- the rule once more in float32, in another summation order ---------------------------------------------------------
def _mm4(x, w):
    """x [R, K] @ w [O, K].T in float32, every product summed as four interleaved partial sums (k = 0, 4, 8, ...; then
    1, 5, ...; ...), each in ascending k, combined as (s0 + s1) + (s2 + s3)."""
    f32 = np.float32
    x, w = np.asarray(x, f32), np.asarray(w, f32)
    parts = []
    for r in range(4):
        prod = x[:, None, r::4] * w[None, :, r::4]  # [R, O, ceil((K - r) / 4)] float32
        # (a float32 cumsum adds one element after the other; np.sum would add pairwise)
        parts.append(np.cumsum(prod, axis=2, dtype=f32)[:, :, -1] if prod.shape[2] else np.zeros(prod.shape[:2], f32))
    return (parts[0] + parts[1]) + (parts[2] + parts[3])


def _sig32(x):
    with np.errstate(over="ignore"):
        return (np.float32(1) / (np.float32(1) + np.exp(-x))).astype(np.float32)


def params32(module) -> dict:
    return {k: v.detach().cpu().numpy().astype(np.float32) for k, v in module.state_dict().items()}


def fp32_other_order(p: dict, cfg: dict, obs, prev_action=None, prev_reward=None, start=None, state=None, wrap_bytes: bool = False):
    """The rule of either policy (``cfg`` of a MaskedRecurrentPolicy or a JointActionPolicy says which) in float32 NumPy
    with ``_mm4`` products: a second legitimate fp32 evaluation beside the torch module's.  Arguments as ``forward64`` of
    policy_util / joint_policy_util; returns float32 logits [R, 5 N], value [R], (h', c').  ``wrap_bytes``: the mutant that
    wraps a prev_action byte outside 0..4 into that range instead of dropping it."""
    f32 = np.float32
    obs = np.asarray(obs, f32)
    R = obs.shape[0]
    joint = "grid_cells" in cfg
    if joint:
        F, N, mask = cfg["grid_cells"], cfg["num_agents"], True
    else:
        N, mask = 1, cfg["has_mask"]
        F = obs.shape[1] - NUM_ACTIONS if mask else obs.shape[1]
    a1 = np.tanh(_mm4(obs[:, :F], p["fc1.weight"]) + p["fc1.bias"])
    a2 = np.tanh(_mm4(a1, p["fc2.weight"]) + p["fc2.bias"])
    if cfg["recurrent"]:
        h, c = (np.zeros((R, HIDDEN), f32), np.zeros((R, HIDDEN), f32)) if state is None else (np.array(state[0], f32), np.array(state[1], f32))
        pa = np.zeros((R, N), np.int64) if prev_action is None else np.asarray(prev_action, np.int64).reshape(R, N).copy()
        pr = np.zeros(R, f32) if prev_reward is None else np.asarray(prev_reward).astype(f32)  # float64 rounds to nearest
        if start is not None:
            s = np.asarray(start, bool)
            h[s], c[s], pa[s], pr[s] = 0, 0, 0, 0
        if wrap_bytes:
            pa = pa % NUM_ACTIONS
        onehot = (pa[:, :, None] == np.arange(NUM_ACTIONS)[None, None, :]).astype(f32).reshape(R, NUM_ACTIONS * N)
        z = np.concatenate([a2, onehot, pr[:, None]], axis=1)
        g = (_mm4(z, p["lstm.weight_ih"]) + p["lstm.bias_ih"]) + (_mm4(h, p["lstm.weight_hh"]) + p["lstm.bias_hh"])
        gi, gf, gg, go = (g[:, k * HIDDEN:(k + 1) * HIDDEN] for k in range(4))
        c = _sig32(gf) * c + _sig32(gi) * np.tanh(gg)
        h = _sig32(go) * np.tanh(c)
        u, state = h, (h, c)
    else:
        u = a2
    logits = _mm4(u, p["pi.weight"]) + p["pi.bias"]
    if mask:
        logits = logits + np.log(obs[:, F:] + f32(pu.MASK_EPS))
    value = _mm4(u, p["vf.weight"])[:, 0] + p["vf.bias"][0]
    return logits.astype(f32), value.astype(f32), state


def logp32(logits32, actions, subtract_max: bool = True):
    """float32 summed log-probability [R] of actions under float32 logits [R, 5 N], written out as the kernels write it;
    ``subtract_max`` False is the mutant whose log-softmax forgot the maximum."""
    f32 = np.float32
    R = logits32.shape[0]
    lg = np.asarray(logits32, f32).reshape(R, -1, NUM_ACTIONS)
    a = np.asarray(actions, np.int64).reshape(R, -1)
    m = lg.max(axis=2, keepdims=True) if subtract_max else np.zeros_like(lg[:, :, :1])
    with np.errstate(over="ignore", invalid="ignore", divide="ignore"):
        ls = lg - (m + np.log(np.exp(lg - m).sum(axis=2, keepdims=True, dtype=f32)))
        return np.take_along_axis(ls, a[:, :, None], axis=2)[:, :, 0].sum(axis=1, dtype=f32)


# ---- the cases ------------------------------------------------------------------------------------------------------------
def case_seed(key) -> int:
    return CASE_SEEDS.get(key, DEFAULT_SEED)


def _draw_inputs(kind, shape, rng):
    """obs [STEPS, rows, L] float32, prev_action int8 [STEPS, rows(, N)], prev_reward [STEPS, rows]: the generators of
    policy_util.case / joint_policy_util.case with row 0 fully masked, row 1 masked 0.5 throughout, the three real
    observation columns of the per-agent policy in [-8, 8] (unnormalised goal deltas) and prev_reward in [-3, 3]
    (per-agent, float32) or [-3 N, 3 N] (joint, float64: the env's reward is a sum over agents)."""
    if kind == "agent":
        rows, _n, L, mask = shape
        F = L - NUM_ACTIONS if mask else L
        obs = rng.integers(0, 2, size=(STEPS, rows, L)).astype(np.float32)
        real = rng.choice(F, size=min(3, F), replace=False)
        obs[:, :, real] = rng.uniform(-8, 8, size=(STEPS, rows, len(real))).astype(np.float32)
        if mask:
            obs[:, :, F] = 1.0
            obs[:, 0, F:], obs[:, 1, F:] = 0.0, 0.5
        pa = rng.integers(0, NUM_ACTIONS, size=(STEPS, rows)).astype(np.int8)
        pr = rng.uniform(-3, 3, size=(STEPS, rows)).astype(np.float32)
    else:
        rows, H, W, N = shape
        obs = np.stack([ju.draw_obs(rng, rows, H, W, N) for _ in range(STEPS)])
        obs[:, 0, H * W:], obs[:, 1, H * W:] = 0.0, 0.5
        pa = rng.integers(0, NUM_ACTIONS, size=(STEPS, rows, N)).astype(np.int8)
        pr = rng.uniform(-3 * N, 3 * N, size=(STEPS, rows))
    return obs, pa, pr


def _flag_units(kind, shape):
    rows, _N, per, _L = geometry(kind, shape)
    return pu.start_envs(rows, per) if kind == "agent" else ju.start_rows(rows)


@functools.lru_cache(maxsize=None)
def case(kind: str, shape, regime: str = "default", recurrent: bool = True, sample: bool = False, variant=None) -> dict:
    """One unchained case (computed once, shared: treat as read-only).  ``variant`` (default regime only):
      both_starts  start_a and start_b both given at every step, flagging disjoint sets plus one unit in common (the one
                   of row 32, across the tile edge)
      bad_bytes    prev_action bytes -128, -1, 5, 127 on 40 % of the entries, and on every row that starts an episode
      counters     draws preloaded with 0x7FFFFFFF, 0x80000000, 0xFFFFFFFE, 0xFFFFFFFF on half of the rows (both tiles);
                   the last step is a PEEK
      seeds        the noise seed alternates 0xFFFFFFFFFFFFFFFF / 0x8000000000000001
    Every step holds its inputs (obs, prev_action, prev_reward, start_a, start_b, h_in, c_in, draws_in, seed, peek) and the
    restatement's float64 logits, value, h, c, action [R, N], logp, gap [R, N], draws_out, and ``logits32``: the fp32
    evaluations' logits of the same inputs.  ``dev`` as the module docstring says; ``dev_module`` / ``dev_other`` its two parts."""
    import torch

    util = _util(kind)
    rows, N, per, _L = geometry(kind, shape)
    key = (kind, tuple(shape), regime, bool(recurrent), bool(sample), variant)
    seed = case_seed(key)
    if kind == "wide" and recurrent:
        raise ValueError("kind 'wide' is the 256-wide joint net, which is feed-forward only: pass recurrent=False")
    rng = np.random.default_rng([KINDS.index(kind), *[int(v) for v in shape], list(REGIMES).index(regime),
                                 int(recurrent), int(sample), 0 if variant is None else 1 + VARIANTS.index(variant)])
    if kind == "agent":
        module = pu.make_module(shape[2], shape[3], recurrent)
    elif kind == "joint":
        module = ju.make_module(shape[1] * shape[2], N, recurrent)
    else:
        import wide_joint_util as wu

        module = wu.make_module(shape[1] * shape[2], N)
    scale_params(module, *REGIMES[regime])
    cfg, p64, p32 = module.config(), util.params64(module), params32(module)
    obs, pa, pr = _draw_inputs(kind, shape, rng)
    units = rows // per
    edge = min(32 // per, units - 1)
    out = {"kind": kind, "shape": shape, "regime": regime, "recurrent": recurrent, "sample": sample, "variant": variant,
           "module": module, "cfg": cfg, "steps": []}
    dev_m = dev_o = 0.0
    h_in, c_in = np.zeros((rows, HIDDEN), np.float32), np.zeros((rows, HIDDEN), np.float32)
    for t in range(STEPS):
        st = {"obs": obs[t], "prev_action": pa[t].copy(), "prev_reward": pr[t], "start_a": None, "start_b": None, "h_in": h_in,
              "c_in": c_in, "draws_in": np.full(rows, t, np.uint32), "seed": seed, "peek": False}
        flags = np.zeros(units, np.uint8)
        if t in START_STEPS:
            flags[_flag_units(kind, shape)] = 1 + t  # any non-zero byte counts
            st["start_" + START_STEPS[t]] = flags
        if variant == "both_starts":
            perm = rng.permutation(np.setdiff1d(np.arange(units), [edge]))
            k = max(1, units // 5)
            sa, sb = np.zeros(units, np.uint8), np.zeros(units, np.uint8)
            sa[perm[:k]], sb[perm[k:2 * k]] = 1, 200
            sa[edge], sb[edge] = 3, 1
            st["start_a"], st["start_b"] = sa, sb
        elif variant == "bad_bytes":
            bad = rng.random(pa[t].shape) < 0.4
            bad[np.repeat(flags != 0, per)] = True
            st["prev_action"][bad] = rng.choice(np.array(BAD_BYTES, np.int8), size=int(bad.sum()))
        elif variant == "counters":
            d = rng.integers(0, 1 << 32, size=rows, dtype=np.uint64).astype(np.uint32)
            d[::2] = np.resize(np.roll(np.array(TOP_COUNTERS, np.uint32), t), len(d[::2]))
            st["draws_in"], st["peek"] = d, t == STEPS - 1
        elif variant == "seeds":
            st["seed"] = TOP_SEEDS[t % 2]
        srow = start_rows(kind, shape, st["start_a"], st["start_b"])
        state_in = (h_in, c_in) if recurrent else None
        logits, value, state = util.forward64(p64, cfg, st["obs"], st["prev_action"], st["prev_reward"], srow, state_in)
        evals = [fp32_other_order(p32, cfg, st["obs"], st["prev_action"], st["prev_reward"], srow, state_in)]
        # the torch module cannot take a byte outside 0..4 (one_hot raises): its deviation is then measured on the same
        # inputs with those bytes dropped to 0, against the restatement of THOSE inputs, and its logits are not kept
        pam = np.where((st["prev_action"] < 0) | (st["prev_action"] > 4), 0, st["prev_action"]).astype(np.int8)
        same_inputs = np.array_equal(pam, st["prev_action"])
        with torch.no_grad():
            m32 = module(torch.from_numpy(st["obs"]), torch.from_numpy(pam), torch.from_numpy(np.asarray(st["prev_reward"])),
                         torch.from_numpy(srow), None if state_in is None else tuple(torch.from_numpy(x) for x in state_in))
        m32 = (m32[0].numpy(), m32[1].numpy(), None if m32[2] is None else tuple(x.numpy() for x in m32[2]))
        ref_m = (logits, value, state) if same_inputs else util.forward64(p64, cfg, st["obs"], pam, st["prev_reward"], srow, state_in)

        def deviation(got, ref):
            d = [np.abs(got[0] - ref[0]).max(), np.abs(got[1] - ref[1]).max()]
            if recurrent:
                d += [np.abs(got[2][0] - ref[2][0]).max(), np.abs(got[2][1] - ref[2][1]).max()]
            return float(max(d))

        dev_m, dev_o = max(dev_m, deviation(m32, ref_m)), max(dev_o, deviation(evals[0], (logits, value, state)))
        if same_inputs:
            evals.append(m32)
        g = noise(kind, st["seed"], rows, st["draws_in"], N) if sample else None
        action, logp, gap = choose(logits, g)
        st.update({"logits": logits, "value": value, "h": state[0] if recurrent else None, "c": state[1] if recurrent else None,
                   "action": action, "logp": logp, "gap": gap, "logits32": [e[0].copy() for e in evals],
                   "draws_out": st["draws_in"] if (st["peek"] or not sample) else st["draws_in"] + np.uint32(1)})
        out["steps"].append(st)
        if recurrent:
            h_in, c_in = state[0].astype(np.float32), state[1].astype(np.float32)
    out["dev"], out["dev_module"], out["dev_other"] = max(dev_m, dev_o), dev_m, dev_o
    out["max_abs_logit"] = max(float(np.abs(s["logits"] - (np.log(s["obs"][:, -NUM_ACTIONS * N:].astype(np.float64) + pu.MASK_EPS)
                                                             if (kind != "agent" or shape[3]) else 0.0)).max()) for s in out["steps"])
    out["max_abs_h"] = max(float(np.abs(s["h"]).max()) for s in out["steps"]) if recurrent else 0.0
    return out


def dev_logp(c: dict, actions) -> float:
    """The largest deviation, over the case's steps, rows and fp32 evaluations, of torch's float32 log-softmax
    log-probability of ``actions`` (per step) under the evaluation's logits from the float64 rule's: what fp32 evaluation
    of that sum costs on this case (joint_policy_util.dev_logp, over both fp32 evaluations)."""
    import torch

    worst = 0.0
    for s, act in zip(c["steps"], actions):
        R = s["logits"].shape[0]
        a = torch.from_numpy(np.asarray(act, np.int64).reshape(R, -1))
        want = logp_of(s["logits"], act)
        for l32 in s["logits32"]:
            lp = torch.log_softmax(torch.from_numpy(l32).reshape(R, -1, NUM_ACTIONS), dim=2).gather(2, a[:, :, None])[:, :, 0].sum(dim=1)
            worst = max(worst, float(np.abs(lp.numpy().astype(np.float64) - want).max()))
    return worst


def undecided(c: dict):
    """(share of decisions, share of rows with one) whose two best scores lie within 32 dev, over all steps."""
    und = np.stack([s["gap"] for s in c["steps"]]) <= ju.UNDECIDED_FACTOR * c["dev"]
    return float(und.mean()), float(und.any(axis=2).mean())


def restate32(c: dict, mutant=None) -> list:
    """The case through the float32 restatement, in the shape the device runs return: per step action, logp, value,
    logits, h, c, draws.  ``mutant``: None, or one of
      no_max        log-softmax without the maximum subtracted
      start_a_only  the episode start taken from start_a alone when both arrays are given
      wrap_bytes    a prev_action byte outside 0..4 wrapped into that range instead of dropped
      counter31     the draw counter truncated to 31 bits"""
    kind, shape = c["kind"], c["shape"]
    rows, N, _per, _L = geometry(kind, shape)
    p32 = params32(c["module"])
    got = []
    for s in c["steps"]:
        srow = start_rows(kind, shape, s["start_a"], s["start_b"], only_a=mutant == "start_a_only")
        logits, value, state = fp32_other_order(p32, c["cfg"], s["obs"], s["prev_action"], s["prev_reward"], srow,
                                                (s["h_in"], s["c_in"]) if c["recurrent"] else None, wrap_bytes=mutant == "wrap_bytes")
        g = noise(kind, s["seed"], rows, s["draws_in"], N, 31 if mutant == "counter31" else 32) if c["sample"] else None
        action = choose(logits.astype(np.float64), g)[0]  # the fp32 logit plus the noise, in double
        got.append({"action": action[:, 0] if kind == "agent" else action, "logp": logp32(logits, action, mutant != "no_max"),
                    "value": value, "logits": logits, "h": state[0] if c["recurrent"] else None,
                    "c": state[1] if c["recurrent"] else None, "draws": s["draws_out"] if c["sample"] else None})
    return got


def compare(c: dict, got: list):
    """What a parity test asserts of per-step results ``got`` (action, logp, value, logits, h, c, draws; draws None in
    greedy mode), with the project's margins: logits / value / h / c within 16 dev, logp on EVERY row within 32 dev_logp
    of the restatement's log-probability of the results' own actions, everything finite, actions in 0..4 and equal to the
    restatement's wherever its gap is at least 32 dev, draws as the rule leaves them, the undecided shares under the
    caps, 0 < dev < 1e-2.  Returns (the line a parity test prints, the list of failed assertions)."""
    kind, dev = c["kind"], c["dev"]
    rows, N, _per, _L = geometry(kind, c["shape"])
    keys = ("logits", "value") + (("h", "c") if c["recurrent"] else ())
    worst, worst_logp, fails = {k: 0.0 for k in keys}, 0.0, []
    und = []
    for t, (g, e) in enumerate(zip(got, c["steps"])):
        for k in keys:
            if e["peek"] and k in ("h", "c"):  # a PEEK writes no state: the caller checks that it is left as it was
                continue
            if not np.isfinite(g[k]).all():
                fails.append(f"step {t}: {k} not finite")
            worst[k] = max(worst[k], float(np.abs(np.asarray(g[k], np.float64).reshape(e[k].shape) - e[k]).max()))
        act = np.asarray(g["action"]).reshape(rows, N)
        if not ((act >= 0) & (act <= 4)).all():
            fails.append(f"step {t}: action outside 0..4")
            act = np.clip(act, 0, 4)
        if not np.isfinite(g["logp"]).all():
            fails.append(f"step {t}: logp not finite on rows {np.flatnonzero(~np.isfinite(g['logp']))[:8].tolist()}")
        with np.errstate(invalid="ignore"):
            worst_logp = max(worst_logp, float(np.nan_to_num(np.abs(g["logp"] - logp_of(e["logits"], act)), nan=np.inf, posinf=np.inf).max()))
        decided = e["gap"] >= ju.UNDECIDED_FACTOR * dev
        und.append(~decided)
        if not (act[decided] == e["action"][decided]).all():
            fails.append(f"step {t}: {int((act[decided] != e['action'][decided]).sum())} decided actions differ")
        if c["sample"] and not np.array_equal(np.asarray(g["draws"], np.uint32), e["draws_out"]):
            fails.append(f"step {t}: draws")
    dlp = dev_logp(c, [np.clip(np.asarray(g["action"]), 0, 4) for g in got])
    und = np.stack(und)
    und_dec, und_rows = float(und.mean()), float(und.any(axis=2).mean())
    tag = c["regime"] + (f" {c['variant']}" if c["variant"] else "")
    line = (f"{kind} regime parity {c['shape']} {tag} recurrent={c['recurrent']} sample={c['sample']}: dev {dev:.3e}, deviation "
            + ", ".join(f"{k} {v:.3e} ({v / dev:.1f} x dev)" for k, v in worst.items())
            + f", logp {worst_logp:.3e} ({worst_logp / dlp if dlp > 0 else float('nan'):.1f} x dev_logp {dlp:.3e}), undecided decisions "
            f"{int(und.sum())}/{und.size}, rows {int(und.any(axis=2).sum())}/{und.any(axis=2).size}")
    if not 0 < dev < 1e-2:
        fails.append(f"dev {dev}")
    if not dlp > 0:
        fails.append(f"dev_logp {dlp}")
    for k, v in worst.items():
        if not v <= 16 * dev:
            fails.append(f"{k}: {v:.3e} > 16 x dev {dev:.3e}")
    if not worst_logp <= 32 * dlp:
        fails.append(f"logp: {worst_logp:.3e} > 32 x dev_logp {dlp:.3e}")
    if kind != "agent":
        if und_dec > ju.MAX_UNDECIDED_DECISIONS or und_rows > ju.MAX_UNDECIDED_ROWS:
            fails.append(f"undecided decisions {und_dec}, rows {und_rows}")
    elif und_rows > MAX_UNDECIDED_AGENT_ROWS:
        fails.append(f"undecided rows {und_rows}")
    return line, fails


# ---- the LSTM sequence kernels ----------------------------------------------------------------------------------------------
# name -> (T, rows, sx, sw, fbias)
LSTM_REGIMES = {"long": (128, 33, 1.0, 0.125, 0.0),
                "hot": (128, 33, 4.0, 0.5, 4.0),  # |G| to 22, |c| to 11
                "saturated": (64, 65, 12.0, 1.0, 10.0),  # |G| to 63, the input gate saturated on 45 % of the entries
                "overflow": (8, 33, 40.0, 1.0, 30.0)}  # |G| to about 190: expf(-x) is +inf in the kernels' sigmoid
LSTM_PERM_SEED = 5


def stable_sig(x):
    """sigmoid by e = exp(-|x|): 1 / (1 + e) for x >= 0, e / (1 + e) otherwise.  Elementary ops; finite gradients under
    autograd at any x (learner_util._sig gives NaN gradients in fp32 once exp(-x) overflows)."""
    import torch

    e = torch.exp(torch.where(x >= 0, -x, x))
    return torch.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def _lstm_loop(xg, whh, reset, h0, c0):
    """learner_util.lstm_loop with ``stable_sig``."""
    import torch

    h, c = h0, c0
    hs, cs, gs = [], [], []
    for t in range(xg.shape[0]):
        if reset is not None:
            keep = (reset[t] == 0).to(xg.dtype)[:, None]
            h, c = h * keep, c * keep
        g = xg[t] + h @ whh.t()
        i, f, o = stable_sig(g[:, :HIDDEN]), stable_sig(g[:, HIDDEN:2 * HIDDEN]), stable_sig(g[:, 3 * HIDDEN:])
        gg = torch.tanh(g[:, 2 * HIDDEN:3 * HIDDEN])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h), cs.append(c), gs.append(torch.cat([i, f, gg, o], dim=1))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def lstm_with_grads(inp: dict, dtype, perm=None) -> dict:
    """learner_util.loop_with_grads over ``_lstm_loop``.  ``perm`` (a permutation of the 64 hidden units): the same
    computation with the hidden units relabelled, i.e. in another summation order; results are permuted back."""
    import torch

    if perm is not None:
        gp = np.concatenate([k * HIDDEN + perm for k in range(4)])
        inp = dict(inp, xg=inp["xg"][:, :, gp], whh=inp["whh"][gp][:, perm], h0=inp["h0"][:, perm], c0=inp["c0"][:, perm],
                   dh=inp["dh"][:, :, perm], dhT=inp["dhT"][:, perm], dcT=inp["dcT"][:, perm])
    t = {k: (None if v is None else torch.from_numpy(np.ascontiguousarray(v))) for k, v in inp.items()}
    leaf = {k: t[k].to(dtype).requires_grad_(True) for k in ("xg", "whh", "h0", "c0")}
    h, c, gates = _lstm_loop(leaf["xg"], leaf["whh"], t["reset"], leaf["h0"], leaf["c0"])
    loss = (h * t["dh"].to(dtype)).sum() + (h[-1] * t["dhT"].to(dtype)).sum() + (c[-1] * t["dcT"].to(dtype)).sum()
    dxg, dwhh, dh0, dc0 = torch.autograd.grad(loss, [leaf["xg"], leaf["whh"], leaf["h0"], leaf["c0"]])
    out = {"h": h, "c": c, "gates": gates, "dxg": dxg, "dwhh": dwhh, "dh0": dh0, "dc0": dc0}
    out = {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}
    if perm is not None:
        inv = np.argsort(perm)
        ginv = np.argsort(gp)
        out = {"h": out["h"][:, :, inv], "c": out["c"][:, :, inv], "gates": out["gates"][:, :, ginv], "dxg": out["dxg"][:, :, ginv],
               "dwhh": out["dwhh"][ginv][:, inv], "dh0": out["dh0"][:, inv], "dc0": out["dc0"][:, inv]}
    return out


@functools.lru_cache(maxsize=None)
def lstm_case(name: str) -> dict:
    """A case in the format of learner_util.lstm_case (``inp``, ``want``, ``dev`` per quantity; computed once, shared:
    treat as read-only) for LSTM_REGIMES[name] = (T, rows, sx, sw, fbias): xg ~ N(0, sx^2) with fbias added to the forget-gate
    quarter, whh uniform in +-sw, c0 ~ 3 N(0, 1), resets on 3 % of all (t, row).  ``dev`` is the larger of the fp32 CPU
    loop's deviation from the float64 oracle and that of the same loop with the hidden units relabelled (``dev_loop`` /
    ``dev_perm``).  ``G`` [T, rows, 256]: the oracle's gate pre-activations."""
    import torch

    T, R, sx, sw, fbias = LSTM_REGIMES[name]
    rng = np.random.default_rng([77, list(LSTM_REGIMES).index(name)])
    f32 = np.float32
    xg = sx * rng.standard_normal((T, R, lu.GATES))
    xg[:, :, HIDDEN:2 * HIDDEN] += fbias
    inp = {"xg": xg.astype(f32), "whh": rng.uniform(-sw, sw, (lu.GATES, HIDDEN)).astype(f32),
           "reset": (rng.random((T, R)) < 0.03).astype(np.uint8),
           "h0": rng.uniform(-1, 1, (R, HIDDEN)).astype(f32), "c0": (3 * rng.standard_normal((R, HIDDEN))).astype(f32),
           "dh": rng.standard_normal((T, R, HIDDEN)).astype(f32),
           "dhT": rng.standard_normal((R, HIDDEN)).astype(f32), "dcT": rng.standard_normal((R, HIDDEN)).astype(f32)}
    want = lstm_with_grads(inp, torch.float64)
    perm = np.random.default_rng(LSTM_PERM_SEED).permutation(HIDDEN)
    loop32, perm32 = lstm_with_grads(inp, torch.float32), lstm_with_grads(inp, torch.float32, perm)
    dev_loop = {k: float(np.abs(loop32[k] - want[k]).max()) for k in lu.QUANTITIES}
    dev_perm = {k: float(np.abs(perm32[k] - want[k]).max()) for k in lu.QUANTITIES}
    hp = np.concatenate([inp["h0"][None].astype(np.float64), want["h"][:-1]]) * (inp["reset"] == 0)[:, :, None]
    G = inp["xg"].astype(np.float64) + hp @ inp["whh"].astype(np.float64).T
    return {"name": name, "shape": (T, R), "reset_kind": name, "inp": inp, "want": want, "G": G,
            "dev": {k: max(dev_loop[k], dev_perm[k]) for k in lu.QUANTITIES}, "dev_loop": dev_loop, "dev_perm": dev_perm}
