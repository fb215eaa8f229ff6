"""What the joint learner's tests share: a synthetic ``JointRollout``-shaped fragment, GAE restated in float64 NumPy, a
fragment's policy run step by step with ``module.forward``, and the PPO objective of a MultiDiscrete([5] * N) action written
out in elementary torch ops on that run's logits and values (float64 on the CPU is the oracle, the same code in float32
measures ``dev``; gradients by autograd).  Nothing here imports the library or shares code with learner.py."""

from __future__ import annotations

import numpy as np
import torch

import joint_policy_util as ju

HIDDEN = 64
LOSS_TERMS = ("total_loss", "policy_loss", "vf_loss", "entropy")


def synthetic_fragment(T: int, B: int, H: int, W: int, N: int, seed: int = 0, flags=None) -> dict:
    """A ``JointRollout.collect()``-shaped dict of CPU tensors with random content (observations drawn like the env's).
    flags: (terminated, truncated) uint8 [T, B], default random ends in a tenth of the steps; ``first`` follows from them
    (first[0] random)."""
    rng = np.random.default_rng(seed)
    obs = np.stack([ju.draw_obs(rng, B, H, W, N) for _ in range(T)])
    if flags is None:
        term = (rng.random((T, B)) < 0.1).astype(np.uint8)
        trunc = ((rng.random((T, B)) < 0.1) & (term == 0)).astype(np.uint8)
    else:
        term, trunc = (np.asarray(f, np.uint8) for f in flags)
    first = np.zeros((T, B), np.uint8)
    first[0] = rng.random(B) < 0.5
    first[1:] = (term | trunc)[:-1]
    rewards = rng.uniform(-1, 1, size=(T, B))  # float64, as the step writes them
    prev_rewards = np.concatenate([rng.uniform(-1, 1, size=(1, B)), rewards[:-1]])
    frag = {"obs": obs, "actions": rng.integers(0, 5, size=(T, B, N)).astype(np.int8),
            "logp": np.log(rng.uniform(0.1, 0.9, size=(T, B, N))).sum(axis=2).astype(np.float32),
            "value": rng.standard_normal((T, B)).astype(np.float32), "rewards": rewards, "terminated": term,
            "truncated": trunc, "first": first, "h0": rng.uniform(-1, 1, (B, HIDDEN)).astype(np.float32),
            "c0": rng.standard_normal((B, HIDDEN)).astype(np.float32), "last_value": rng.standard_normal(B).astype(np.float32),
            "prev_action0": rng.integers(0, 5, size=(B, N)).astype(np.int8), "prev_rewards": prev_rewards}
    return {k: torch.from_numpy(v) for k, v in frag.items()}


def gae64(frag: dict, gamma: float, lam: float, boot_value=None):
    """Generalised advantage estimation per env in float64 NumPy, one (t, env) at a time; the rewards enter as the fp32
    numbers the learner casts them to."""
    f = {k: v.detach().cpu().numpy() for k, v in frag.items()}
    v, r = f["value"].astype(np.float64), f["rewards"].astype(np.float32).astype(np.float64)
    T, B = v.shape
    adv = np.zeros((T, B))
    for b in range(B):
        nxt = 0.0
        for t in range(T - 1, -1, -1):
            term, trunc = bool(f["terminated"][t, b]), bool(f["truncated"][t, b])
            if trunc:  # (the engine raises both flags at the time limit: a truncation)
                nv = 0.0 if boot_value is None else float(boot_value[t, b])
            elif term:
                nv = 0.0
            else:
                nv = float(f["last_value"][b]) if t == T - 1 else v[t + 1, b]
            delta = r[t, b] + gamma * nv - v[t, b]
            adv[t, b] = delta + (0.0 if (term or trunc) else gamma * lam * nxt)
            nxt = adv[t, b]
    return adv, adv + v


def chained_forward(module, frag: dict):
    """Logits [T, B, 5N] and values [T, B]: T calls of ``module.forward`` fed the way ``JointRollout`` feeds the device
    policy (the float64 reward rounded to fp32, as the kernel's load does)."""
    T = frag["obs"].shape[0]
    dt = frag["obs"].dtype
    state = (frag["h0"].to(dt), frag["c0"].to(dt)) if module.recurrent else None
    logits, values = [], []
    for t in range(T):
        pa = frag["prev_action0"] if t == 0 else frag["actions"][t - 1]
        pr = frag["prev_rewards"][t].to(torch.float32).to(dt)
        lg, v, state = module(frag["obs"][t], pa, pr, frag["first"][t], state)
        logits.append(lg), values.append(v)
    return torch.stack(logits), torch.stack(values)


def standardised(adv):
    """(adv - mean) / standard deviation (the population one), over the whole fragment."""
    mean = adv.sum() / adv.numel()
    return (adv - mean) / torch.sqrt(((adv - mean) ** 2).sum() / adv.numel())


def ppo_terms(logits, values, frag: dict, adv, targets, clip: float, vf_coeff: float, ent_coeff: float, vf_clip: float) -> dict:
    """The clipped-surrogate objective of a MultiDiscrete([5] * N) action in elementary torch ops, in the dtype of ``logits``
    [T, B, 5N] and ``values`` [T, B]; adv (already standardised) and targets [T, B].  Per agent a log-softmax over its five
    logits; the row's log-probability is the sum over the agents of the taken action's, its entropy the sum of the
    per-agent entropies.  Besides the four loss terms, the share of elements at which the ratio clip and the value clip
    bind."""
    T, B, A = logits.shape
    N = A // 5
    dt = logits.dtype
    lg = logits.reshape(T, B, N, 5)
    x = lg - lg.max(dim=3, keepdim=True).values.detach()
    logp_all = x - torch.log(torch.exp(x).sum(dim=3, keepdim=True))
    p_all = torch.exp(logp_all)
    taken = (frag["actions"].reshape(T, B, N, 1).to(torch.int64) == torch.arange(5)).to(dt)
    logp = (logp_all * taken).sum(dim=3).sum(dim=2)
    ratio = torch.exp(logp - frag["logp"].to(dt))
    a, tgt = adv.to(dt), targets.to(dt)
    lo, hi = torch.full_like(ratio, 1.0 - clip), torch.full_like(ratio, 1.0 + clip)
    clipped = torch.where(ratio < lo, lo, torch.where(ratio > hi, hi, ratio))
    plain, bounded = a * ratio, a * clipped
    ratio_binds = bounded < plain
    surrogate = torch.where(ratio_binds, bounded, plain)
    sq = (values - tgt) * (values - tgt)
    vf_binds = sq > vf_clip
    sq = torch.where(vf_binds, torch.full_like(sq, vf_clip), sq)
    n = T * B
    entropy_rows = -((p_all * logp_all).sum(dim=3)).sum(dim=2)
    policy_loss, vf_loss, entropy = -(surrogate.sum() / n), sq.sum() / n, entropy_rows.sum() / n
    return {"total_loss": policy_loss + vf_coeff * vf_loss - ent_coeff * entropy, "policy_loss": policy_loss, "vf_loss": vf_loss,
            "entropy": entropy, "ratio_binds": float(ratio_binds.to(dt).mean()), "vf_binds": float(vf_binds.to(dt).mean())}


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
