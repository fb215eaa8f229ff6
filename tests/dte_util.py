"""What the tests of one policy per agent (DTE) share: N modules drawn from different seeds as one ``PerAgentPolicy``, the
float64 restatement of the rule with each row's own parameters (policy_util.forward64 on the rows of an agent), the chained
cases of the act kernel, the grouped cases of the LSTM sequence kernels and the per-agent PPO objective by hand
(learner_util on each agent's slice of a fragment).  Nothing here imports the library."""

from __future__ import annotations

import copy
import functools

import numpy as np
import torch

import learner_util as lu
import policy_util as pu

# (B, N, L, mask): less than one tile per agent; the masked mid-size observation; a second tile of one row per agent at the
# longest observation; the training setup's row (16 agents, L = 52); three tiles per agent; one agent (the per-agent launch
# on a shared-shaped problem); the most agents a handle takes
SHAPES = ((3, 5, 11, False), (13, 5, 33, True), (33, 3, 130, True), (6, 16, 52, False), (70, 2, 52, False), (40, 1, 52, False),
          (2, 64, 11, False))
STEPS = pu.STEPS
START_STEPS = pu.START_STEPS


def make_per_agent(N: int, L: int, mask: bool, recurrent: bool, seed: int = 0):
    """A ``PerAgentPolicy`` whose agent a is policy_util.make_module(..., seed = 100 + 7 * seed + a): N different nets."""
    from dl_reference_models_amd.policy import PerAgentPolicy

    m = PerAgentPolicy(N, L, has_mask=mask, recurrent=recurrent).eval()
    for a, agent in enumerate(m.agents):
        agent.load_state_dict(pu.make_module(L, mask, recurrent, seed=100 + 7 * seed + a).state_dict())
    return m


def forward64(module, obs, prev_action=None, prev_reward=None, start=None, state=None):
    """policy_util.forward64 with each row's own parameters: rows a::N through agent a's.  start bool [R] per row."""
    N, R = module.num_agents, obs.shape[0]
    cfg = module.agents[0].config()
    logits, value = np.zeros((R, pu.NUM_ACTIONS)), np.zeros(R)
    h, c = (np.zeros((R, pu.HIDDEN)), np.zeros((R, pu.HIDDEN))) if module.recurrent else (None, None)
    for a, agent in enumerate(module.agents):
        s = slice(a, None, N)
        lg, v, st = pu.forward64(pu.params64(agent), cfg, obs[s], None if prev_action is None else prev_action[s],
                                 None if prev_reward is None else prev_reward[s], None if start is None else start[s],
                                 None if state is None else (state[0][s], state[1][s]))
        logits[s], value[s] = lg, v
        if module.recurrent:
            h[s], c[s] = st
    return logits, value, ((h, c) if module.recurrent else None)


@functools.lru_cache(maxsize=None)
def case(shape, recurrent: bool, sample: bool, seed: int = 11) -> dict:
    """policy_util.case for N different nets: six chained steps, episode starts at steps 2 and 4 through start_a / start_b,
    the float64 expectations with each row's own parameters, and ``dev``, the largest deviation of the fp32 CPU module
    (``PerAgentPolicy.forward``) from them.  Computed once, shared: treat as read-only."""
    B, N, L, mask = shape
    rows = B * N
    rng = np.random.default_rng(hash((B, N, L, mask, recurrent, sample, 77)) % (2 ** 31))
    module = make_per_agent(N, L, mask, recurrent)
    F = L - pu.NUM_ACTIONS if mask else L
    obs = rng.integers(0, 2, size=(STEPS, rows, L)).astype(np.float32)
    real = rng.choice(F, size=min(3, F), replace=False)
    obs[:, :, real] = rng.uniform(-1, 1, size=(STEPS, rows, len(real))).astype(np.float32)
    if mask:
        obs[:, :, F] = 1.0
    pa = rng.integers(0, pu.NUM_ACTIONS, size=(STEPS, rows)).astype(np.int8)
    pr = rng.uniform(-1, 1, size=(STEPS, rows)).astype(np.float32)
    flags = np.zeros((STEPS, B), np.uint8)
    for t in START_STEPS:
        flags[t, sorted({0, B - 1, min(32, B - 1)})] = 1 + t  # the first env, the last, and the first of a second tile
    out = {"shape": shape, "recurrent": recurrent, "sample": sample, "seed": seed, "module": module, "obs": obs,
           "prev_action": pa, "prev_reward": pr, "flags": flags, "steps": []}
    state, state32, dev = None, None, 0.0
    with torch.no_grad():
        for t in range(STEPS):
            srow = np.repeat(flags[t] != 0, N)
            logits, value, state = forward64(module, obs[t], pa[t], pr[t], srow, state)
            l32, v32, state32 = module(torch.from_numpy(obs[t]), torch.from_numpy(pa[t]), torch.from_numpy(pr[t]),
                                       torch.from_numpy(srow), state32)
            devs = [np.abs(l32.numpy() - logits).max(), np.abs(v32.numpy() - value).max()]
            if recurrent:
                devs += [np.abs(state32[0].numpy() - state[0]).max(), np.abs(state32[1].numpy() - state[1]).max()]
            dev = max(dev, float(max(devs)))
            out["steps"].append({"logits": logits, "value": value, "h": None if state is None else state[0],
                                 "c": None if state is None else state[1]})
    out["dev"] = dev
    return out


# ---- grouped LSTM sequences ----------------------------------------------------------------------------------------------
# (T, rows per group, G): one row; one row past a tile in three groups; one row past two tiles in five; one row past a
# 128-row workgroup in two; the training setup's 16 agents on less than a tile; the most groups on one row each
LSTM_SHAPES = ((1, 1, 1), (2, 33, 3), (5, 65, 5), (3, 129, 2), (4, 7, 16), (2, 1, 64))


@functools.lru_cache(maxsize=None)
def lstm_case(shape, reset_kind: str) -> dict:
    """Inputs of one grouped case in the style of learner_util.lstm_case: R = rows per group x G interleaved rows (row r in
    group r % G), whh [G, 256, 64]; ``want`` / ``dev`` for dwhh [G, 256, 64] from the float64 / fp32 loops of learner_util on
    each group's rows gathered with whh[g] (dev: over the whole tensor).  Computed once, shared: treat as read-only."""
    T, per, G = shape
    R = per * G
    rng = np.random.default_rng(100000 * G + 1000 * T + per + 17 * lu.RESETS.index(reset_kind))
    f32 = np.float32
    inp = {"xg": rng.standard_normal((T, R, lu.GATES)).astype(f32),
           "whh": rng.uniform(-0.125, 0.125, (G, lu.GATES, lu.HIDDEN)).astype(f32),
           "reset": lu.reset_pattern(reset_kind, T, R, rng),
           "h0": rng.uniform(-1, 1, (R, lu.HIDDEN)).astype(f32), "c0": rng.standard_normal((R, lu.HIDDEN)).astype(f32),
           "dh": rng.standard_normal((T, R, lu.HIDDEN)).astype(f32),
           "dhT": rng.standard_normal((R, lu.HIDDEN)).astype(f32), "dcT": rng.standard_normal((R, lu.HIDDEN)).astype(f32)}
    want = np.stack([lu.loop_with_grads(group_inputs(inp, g, G), torch.float64)["dwhh"] for g in range(G)])
    got32 = np.stack([lu.loop_with_grads(group_inputs(inp, g, G), torch.float32)["dwhh"] for g in range(G)])
    return {"shape": shape, "reset_kind": reset_kind, "inp": inp, "want_dwhh": want, "dev_dwhh": float(np.abs(got32 - want).max())}


def group_inputs(inp: dict, g: int, G: int) -> dict:
    """The rows of group g gathered contiguously, with whh[g]: what the ungrouped calls take."""
    out = {}
    for k, v in inp.items():
        if v is None:
            out[k] = None
        elif k == "whh":
            out[k] = np.ascontiguousarray(v[g])
        elif k in ("h0", "c0", "dhT", "dcT"):
            out[k] = np.ascontiguousarray(v[g::G])
        else:
            out[k] = np.ascontiguousarray(v[:, g::G])
    return out


# ---- N independent PPO learners by hand ------------------------------------------------------------------------------------
def standardised_per_agent(adv):
    """learner_util.standardised over each agent's [T, B] of adv [T, B, N]."""
    return torch.stack([lu.standardised(adv[:, :, a]) for a in range(adv.shape[2])], dim=2)


def agent_fragment(frag: dict, a: int) -> dict:
    """Agent a's slice of a fragment as a fragment of its own, [T, B, 1, ...]."""
    T, B, N = frag["actions"].shape
    return lu.rows_as_fragment(frag, torch.arange(a, B * N, N))


def ppo_by_hand(module, frag: dict, adv, targets, **kw) -> dict:
    """learner_util.ppo_by_hand on every agent's own net and slice, in the module's dtype on the CPU: ``forward`` (logits
    [T, B, N, 5] then values [T, B, N], flat), ``loss`` (the four terms, [N, 4]) and ``gradient`` (policy-major, flat, in the
    order of ``module.parameters()``).  adv: already standardised per agent."""
    T, B, N = frag["actions"].shape
    outs = [lu.ppo_by_hand(copy.deepcopy(module.agents[a]), agent_fragment(frag, a), adv[:, :, a:a + 1], targets[:, :, a:a + 1], **kw)
            for a in range(N)]
    logits = np.stack([o["forward"][:T * B * 5].reshape(T, B, 5) for o in outs], axis=2)
    values = np.stack([o["forward"][T * B * 5:].reshape(T, B) for o in outs], axis=2)
    return {"forward": np.concatenate([logits.ravel(), values.ravel()]), "loss": np.stack([o["loss"] for o in outs]),
            "gradient": np.concatenate([o["gradient"] for o in outs])}
