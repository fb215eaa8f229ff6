"""What the learner's tests share: the LSTM recurrence written out in elementary torch ops (float64 on the CPU is the oracle,
the same code in float32 measures ``dev``; gradients by autograd), the synthetic cases of the sequence kernels, a synthetic
``Rollout``-shaped fragment, GAE restated in float64 NumPy, a fragment's policy run step by step with ``module.forward``, and
the PPO objective written out on that run's logits and values.  Nothing here imports the library."""

from __future__ import annotations

import functools

import numpy as np
import torch

HIDDEN = 64
GATES = 256

# (T, rows): one row; one row past a tile; one row past two tiles; the training fragment length on three full tiles; many
# workgroups with a ragged last one
SHAPES = ((1, 1), (2, 33), (5, 65), (32, 96), (3, 2049))
RESETS = ("none", "first_step", "scattered")
QUANTITIES = ("h", "c", "gates", "dxg", "dh0", "dc0", "dwhh")
FORWARD = ("h", "c", "gates")
KERNEL_GRADS = ("dxg", "dh0", "dc0")
# A GPU result may deviate from the float64 oracle by a margin times ``dev``, the deviation of the same computation in fp32
# on the CPU.  Forward quantities: the 16 of tests/test_policy_gpu.py.  Gradients: the next power of two at or above twice
# the largest ratio measured over all cases of tests/test_lstm_seq_gpu.py on the GPU (DESIGN.md 4m holds the table,
# profiles/r12/learner/parity_deviation.txt the raw ratios), taken separately for what the backward kernel itself returns
# and for what a GEMM after it sums (dwhh, and with it a module's parameter gradient), so that the wider one does not
# loosen the bound on the kernel.
FORWARD_MARGIN = 16
KERNEL_GRAD_MARGIN = 8  # largest ratio measured: 2.88 (dxg, T = 32, 96 rows; dh0 1.60, dc0 1.85): 2 x 2.88 = 5.8
GRAD_MARGIN = 32  # largest ratio measured: 12.32 (dwhh, T = 3, 2 049 rows, no reset): 2 x 12.32 = 24.6


def margin_of(quantity: str) -> int:
    return FORWARD_MARGIN if quantity in FORWARD else KERNEL_GRAD_MARGIN if quantity in KERNEL_GRADS else GRAD_MARGIN


def _sig(x):
    return 1.0 / (1.0 + torch.exp(-x))


def lstm_loop(xg, whh, reset, h0, c0):
    """h, c [T, R, 64] and the activated gates [T, R, 256] in the dtype of the inputs; reset bool / uint8 [T, R] or None.
    Elementary ops only (no LSTMCell, no torch.sigmoid)."""
    h, c = h0, c0
    hs, cs, gs = [], [], []
    for t in range(xg.shape[0]):
        if reset is not None:
            keep = (reset[t] == 0).to(xg.dtype)[:, None]
            h, c = h * keep, c * keep
        g = xg[t] + h @ whh.t()
        i, f, o = _sig(g[:, :HIDDEN]), _sig(g[:, HIDDEN:2 * HIDDEN]), _sig(g[:, 3 * HIDDEN:])
        gg = torch.tanh(g[:, 2 * HIDDEN:3 * HIDDEN])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        hs.append(h), cs.append(c), gs.append(torch.cat([i, f, gg, o], dim=1))
    return torch.stack(hs), torch.stack(cs), torch.stack(gs)


def loop_with_grads(inp: dict, dtype) -> dict:
    """Every quantity of QUANTITIES from the loop in ``dtype`` on the CPU, as float64 NumPy.  The scalar that is
    differentiated is sum(h * dh) + sum(h_T * dhT) + sum(c_T * dcT): its gradients are what the backward call returns."""
    t = {k: (None if v is None else torch.from_numpy(v)) for k, v in inp.items()}
    leaf = {k: t[k].to(dtype).requires_grad_(True) for k in ("xg", "whh", "h0", "c0")}
    h, c, gates = lstm_loop(leaf["xg"], leaf["whh"], t["reset"], leaf["h0"], leaf["c0"])
    loss = (h * t["dh"].to(dtype)).sum() + (h[-1] * t["dhT"].to(dtype)).sum() + (c[-1] * t["dcT"].to(dtype)).sum()
    dxg, dwhh, dh0, dc0 = torch.autograd.grad(loss, [leaf["xg"], leaf["whh"], leaf["h0"], leaf["c0"]])
    out = {"h": h, "c": c, "gates": gates, "dxg": dxg, "dwhh": dwhh, "dh0": dh0, "dc0": dc0}
    return {k: v.detach().to(torch.float64).numpy() for k, v in out.items()}


def reset_pattern(kind: str, T: int, R: int, rng) -> np.ndarray | None:
    if kind == "none":
        return None
    m = np.zeros((T, R), np.uint8)
    if kind == "first_step":
        m[0] = 1
    else:  # scattered: a tenth of all (t, row), plus the last step and two consecutive steps of fixed rows; any byte counts
        m[rng.random((T, R)) < 0.1] = 1
        m[T - 1, 0] = 7
        m[T - 1, R - 1] = 1
        if T >= 2:
            m[T - 2, R - 1] = 255
            m[0, R // 2], m[1, R // 2] = 1, 1
    return m


@functools.lru_cache(maxsize=None)
def lstm_case(shape, reset_kind: str) -> dict:
    """Inputs (float32 NumPy), the float64 oracle and ``dev`` per quantity (largest deviation of the fp32 CPU loop from the
    oracle) of one case; computed once, shared: treat as read-only.  xg ~ N(0, 1), whh at torch's init scale (uniform in
    +-1/8), non-zero h0, c0, dh, dhT, dcT."""
    T, R = shape
    rng = np.random.default_rng(1000 * T + R + 17 * RESETS.index(reset_kind))
    f32 = np.float32
    inp = {"xg": rng.standard_normal((T, R, GATES)).astype(f32),
           "whh": rng.uniform(-0.125, 0.125, (GATES, HIDDEN)).astype(f32),
           "reset": reset_pattern(reset_kind, T, R, rng),
           "h0": rng.uniform(-1, 1, (R, HIDDEN)).astype(f32), "c0": rng.standard_normal((R, HIDDEN)).astype(f32),
           "dh": rng.standard_normal((T, R, HIDDEN)).astype(f32),
           "dhT": rng.standard_normal((R, HIDDEN)).astype(f32), "dcT": rng.standard_normal((R, HIDDEN)).astype(f32)}
    want = loop_with_grads(inp, torch.float64)
    got32 = loop_with_grads(inp, torch.float32)
    dev = {k: float(np.abs(got32[k] - want[k]).max()) for k in QUANTITIES}
    return {"shape": shape, "reset_kind": reset_kind, "inp": inp, "want": want, "dev": dev}


# ---- fragments -------------------------------------------------------------------------------------------------------------
def synthetic_fragment(T: int, B: int, N: int, L: int, mask: bool, seed: int = 0, flags=None) -> dict:
    """A ``Rollout.collect()``-shaped dict of CPU tensors with random content.  flags: (terminated, truncated) uint8 [T, B]
    arrays, default random ends in a tenth of the steps; ``first`` follows from them (first[0] random)."""
    rng = np.random.default_rng(seed)
    F = L - 5 if mask else L
    obs = rng.integers(0, 2, size=(T, B, N, L)).astype(np.float32)
    obs[..., :min(3, F)] = rng.uniform(-1, 1, size=(T, B, N, min(3, F)))
    if mask:
        obs[..., F] = 1.0
    if flags is None:
        term = (rng.random((T, B)) < 0.1).astype(np.uint8)
        trunc = ((rng.random((T, B)) < 0.1) & (term == 0)).astype(np.uint8)
    else:
        term, trunc = (np.asarray(f, np.uint8) for f in flags)
    first = np.zeros((T, B), np.uint8)
    first[0] = rng.random(B) < 0.5
    first[1:] = (term | trunc)[:-1]
    rewards = rng.uniform(-1, 1, size=(T, B, N)).astype(np.float32)
    prev_rewards = np.concatenate([rng.uniform(-1, 1, size=(1, B, N)).astype(np.float32), rewards[:-1]])
    frag = {"obs": obs, "actions": rng.integers(0, 5, size=(T, B, N)).astype(np.int8),
            "logp": np.log(rng.uniform(0.1, 0.9, size=(T, B, N))).astype(np.float32),
            "value": rng.standard_normal((T, B, N)).astype(np.float32), "rewards": rewards, "terminated": term,
            "truncated": trunc, "first": first, "h0": rng.uniform(-1, 1, (B * N, HIDDEN)).astype(np.float32),
            "c0": rng.standard_normal((B * N, HIDDEN)).astype(np.float32),
            "last_value": rng.standard_normal((B, N)).astype(np.float32),
            "prev_action0": rng.integers(0, 5, size=(B, N)).astype(np.int8), "prev_rewards": prev_rewards}
    return {k: torch.from_numpy(v) for k, v in frag.items()}


def rows_as_fragment(frag: dict, rows) -> dict:
    """The agent rows ``rows`` (indices into B * N) as a fragment of their own: one env per row, one agent per env."""
    T, B, N = frag["actions"].shape
    R, out = B * N, {}
    for k, v in frag.items():
        if k in ("h0", "c0"):
            out[k] = v[rows]
        elif k in ("terminated", "truncated", "first"):
            out[k] = v[:, :, None].expand(T, B, N).reshape(T, R)[:, rows].contiguous()
        elif k in ("last_value", "prev_action0"):
            out[k] = v.reshape(R)[rows][:, None]
        else:
            out[k] = v.reshape(T, R, *v.shape[3:])[:, rows].unsqueeze(2)
    return out


def gae64(frag: dict, gamma: float, lam: float, boot_value=None):
    """The rule of learner.gae in float64 NumPy, one (t, env, agent) at a time."""
    f = {k: v.detach().cpu().numpy() for k, v in frag.items()}
    v, r = f["value"].astype(np.float64), f["rewards"].astype(np.float64)
    T, B, N = v.shape
    adv = np.zeros((T, B, N))
    for b in range(B):
        for n in range(N):
            nxt = 0.0
            for t in range(T - 1, -1, -1):
                term, trunc = bool(f["terminated"][t, b]), bool(f["truncated"][t, b])
                if trunc:  # (the engine raises both flags at the time limit: a truncation)
                    nv = 0.0 if boot_value is None else float(boot_value[t, b, n])
                elif term:
                    nv = 0.0
                else:
                    nv = float(f["last_value"][b, n]) if t == T - 1 else v[t + 1, b, n]
                delta = r[t, b, n] + gamma * nv - v[t, b, n]
                adv[t, b, n] = delta + (0.0 if (term or trunc) else gamma * lam * nxt)
                nxt = adv[t, b, n]
    return adv, adv + v


def chained_forward(module, frag: dict):
    """Logits [T, R, 5] and values [T, R]: T calls of ``module.forward`` fed the way ``Rollout`` feeds the device policy."""
    T, B, N, L = frag["obs"].shape
    R = B * N
    state = (frag["h0"].to(frag["obs"].dtype), frag["c0"].to(frag["obs"].dtype)) if module.recurrent else None
    logits, values = [], []
    for t in range(T):
        pa = frag["prev_action0"] if t == 0 else frag["actions"][t - 1]
        start = frag["first"][t][:, None].expand(B, N).reshape(R)
        lg, v, state = module(frag["obs"][t].reshape(R, L), pa.reshape(R), frag["prev_rewards"][t].reshape(R), start, state)
        logits.append(lg), values.append(v)
    return torch.stack(logits), torch.stack(values)


# ---- the PPO objective -----------------------------------------------------------------------------------------------------
def standardised(adv):
    """(adv - mean) / standard deviation (the population one), over the whole fragment."""
    mean = adv.sum() / adv.numel()
    return (adv - mean) / torch.sqrt(((adv - mean) ** 2).sum() / adv.numel())


def ppo_terms(logits, values, frag: dict, adv, targets, clip: float, vf_coeff: float, ent_coeff: float, vf_clip: float) -> dict:
    """The clipped-surrogate objective in elementary torch ops, in the dtype of ``logits`` [T, R, 5] (masked, as
    ``chained_forward`` returns them) and ``values`` [T, R]; adv (already standardised) and targets [T, B, N].  Besides the four
    loss terms, the share of elements at which the ratio clip and the value clip bind."""
    T, R, A = logits.shape
    dt = logits.dtype
    x = logits - logits.max(dim=2, keepdim=True).values.detach()
    logp_all = x - torch.log(torch.exp(x).sum(dim=2, keepdim=True))
    p_all = torch.exp(logp_all)
    taken = (frag["actions"].reshape(T, R, 1).to(torch.int64) == torch.arange(A)).to(dt)
    logp = (logp_all * taken).sum(dim=2)
    ratio = torch.exp(logp - frag["logp"].reshape(T, R).to(dt))
    a, tgt = adv.reshape(T, R).to(dt), targets.reshape(T, R).to(dt)
    lo, hi = torch.full_like(ratio, 1.0 - clip), torch.full_like(ratio, 1.0 + clip)
    clipped = torch.where(ratio < lo, lo, torch.where(ratio > hi, hi, ratio))
    plain, bounded = a * ratio, a * clipped
    ratio_binds = bounded < plain
    surrogate = torch.where(ratio_binds, bounded, plain)
    sq = (values - tgt) * (values - tgt)
    vf_binds = sq > vf_clip
    sq = torch.where(vf_binds, torch.full_like(sq, vf_clip), sq)
    n = T * R
    policy_loss, vf_loss, entropy = -(surrogate.sum() / n), sq.sum() / n, -((p_all * logp_all).sum() / n)
    return {"total_loss": policy_loss + vf_coeff * vf_loss - ent_coeff * entropy, "policy_loss": policy_loss, "vf_loss": vf_loss,
            "entropy": entropy, "ratio_binds": float(ratio_binds.to(dt).mean()), "vf_binds": float(vf_binds.to(dt).mean())}


LOSS_TERMS = ("total_loss", "policy_loss", "vf_loss", "entropy")


def ppo_by_hand(module, frag: dict, adv, targets, clip=0.05, vf_coeff=0.5, ent_coeff=0.001, vf_clip=10.0) -> dict:
    """``chained_forward`` and ``ppo_terms`` on it, in the module's dtype on the CPU, as float64 NumPy: ``forward`` (logits
    and values, flat), ``loss`` (LOSS_TERMS), ``gradient`` (of the total loss, flat over the parameters) and the two shares."""
    module.zero_grad()
    logits, values = chained_forward(module, frag)
    terms = ppo_terms(logits, values, frag, adv, targets, clip, vf_coeff, ent_coeff, vf_clip)
    terms["total_loss"].backward()
    flat = torch.cat([p.grad.reshape(-1) for p in module.parameters()])
    f64 = lambda x: x.detach().double().numpy()  # noqa: E731
    return {"forward": np.concatenate([f64(logits).ravel(), f64(values).ravel()]),
            "loss": np.array([float(terms[k].detach()) for k in LOSS_TERMS]), "gradient": f64(flat),
            "ratio_binds": terms["ratio_binds"], "vf_binds": terms["vf_binds"]}
