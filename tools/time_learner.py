#!/usr/bin/env python3
"""What the learner costs (a measurement, modelled on tools/time_policy.py), fused kernels against the torch loop, all in this
process:

    lstm      learner.lstm_sequence forward plus backward (one launch each plus the dW_hh GEMM, against T steps of torch ops),
              T = 32 at 8 192 and 65 536 rows
    epoch     one PPOLearner.update epoch (8 minibatches) on a synthetic fragment of the training setup's shape at both sizes
    iterate   one Trainer.iterate() at the reference's training setup, broken into collect, gae and update

Three alternating rounds each, medians.  One JSON object per line; the raw lines are kept when --out is given.

    python tools/time_learner.py [--out profiles/r12/learner/time_learner.jsonl] [--sections lstm,epoch,iterate]
"""
import copy, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dl_reference_models_amd import learner as ln
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import MaskedRecurrentPolicy
from dl_reference_models_amd.vec_env import VecReferenceModel

T = 32
ROUNDS = 3
SIZES = (8192, 65536)
TRAINING = "ref_training_4096x32x32_n16"
DEV = "cuda:0"
# the floor of the forward pass at T = 32 and 65 536 rows, from counted bytes and flops (not measured): 2.5 KB of HBM traffic
# per row-step at 8 TB/s, 69 GFLOP on the f32-input MFMA at 157 TF
FLOOR_MS = {"hbm": 0.7, "mfma": 0.45}


def timed(fn, reps):
    """ms per call: `reps` calls between two events, after two calls outside them."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def rounds(fns: dict, reps: dict) -> dict:
    out = {}
    for r in range(ROUNDS):
        for kind, fn in fns.items():
            out[f"{kind}_ms_round{r}"] = timed(fn, reps[kind])
    for kind in fns:
        out[kind + "_ms"] = float(np.median([out[f"{kind}_ms_round{r}"] for r in range(ROUNDS)]))
    out["fused_faster_in_every_round"] = all(out[f"fused_ms_round{r}"] < out[f"torch_ms_round{r}"] for r in range(ROUNDS))
    out["torch_over_fused"] = out["torch_ms"] / out["fused_ms"]
    return out


def run_lstm(rows, emit):
    g = torch.Generator(device=DEV).manual_seed(0)
    xg = torch.randn((T, rows, 256), device=DEV, generator=g).requires_grad_(True)
    whh = ((torch.rand((256, 64), device=DEV, generator=g) - 0.5) / 4).requires_grad_(True)
    reset = (torch.rand((T, rows), device=DEV, generator=g) < 0.05).to(torch.uint8)
    h0 = torch.zeros((rows, 64), device=DEV).requires_grad_(True)
    c0 = torch.zeros((rows, 64), device=DEV).requires_grad_(True)
    dh = torch.randn((T, rows, 64), device=DEV, generator=g)

    def both(fused):
        def fn():
            h, _ = ln.lstm_sequence(xg, whh, reset, h0, c0, fused=fused)
            torch.autograd.grad((h * dh).sum(), [xg, whh, h0, c0])
        return fn

    def forward_only():
        with torch.no_grad():
            ln.lstm_sequence(xg, whh, reset, h0, c0, fused=True)

    out = {"section": "lstm", "T": T, "rows": rows}
    out.update(rounds({"fused": both(True), "torch": both(False)}, {"fused": 10, "torch": 3}))
    out["fused_forward_only_ms"] = float(np.median([timed(forward_only, 10) for _ in range(ROUNDS)]))
    if rows == 65536:
        out["forward_floor_ms"] = FLOOR_MS
    emit(out)


def synthetic_fragment(rows, n=16, L=52):
    g = torch.Generator(device=DEV).manual_seed(1)
    B = rows // n
    r = lambda *s: torch.rand(s, device=DEV, generator=g)  # noqa: E731
    end = r(T, B) < 1 / 64
    first = torch.cat([torch.ones((1, B), dtype=torch.bool, device=DEV), end[:-1]])
    rewards = r(T, B, n) - 0.5
    return {"obs": (r(T, B, n, L) < 0.3).float(), "actions": (r(T, B, n) * 5).to(torch.int8).clamp_(0, 4), "logp": -1.6 + 0.1 * r(T, B, n),
            "value": r(T, B, n) - 0.5, "rewards": rewards, "terminated": (end & (r(T, B) < 0.5)).to(torch.uint8),
            "truncated": torch.zeros((T, B), dtype=torch.uint8, device=DEV), "first": first.to(torch.uint8),
            "h0": torch.zeros((rows, 64), device=DEV), "c0": torch.zeros((rows, 64), device=DEV), "last_value": r(B, n) - 0.5,
            "prev_action0": torch.zeros((B, n), dtype=torch.int8, device=DEV),
            "prev_rewards": torch.cat([torch.zeros((1, B, n), device=DEV), rewards[:-1]])}


def run_epoch(rows, emit):
    frag = synthetic_fragment(rows)
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(52, has_mask=False, recurrent=True).to(DEV)
    adv, targets = ln.gae(frag)
    learners = {k: ln.PPOLearner(copy.deepcopy(module), epochs=1, minibatches=8, fused=(k == "fused")) for k in ("fused", "torch")}
    out = {"section": "epoch", "T": T, "rows": rows, "minibatches": 8}
    out.update(rounds({k: (lambda le=le: le.update(frag, adv, targets)) for k, le in learners.items()}, {"fused": 3, "torch": 2}))
    emit(out)


def run_iterate(emit, iters=4):
    b = wl.WORKLOADS[TRAINING][0]
    cfg = wl.workload_config(TRAINING, list(range(b)))
    for fused in (True, False):
        env = VecReferenceModel(cfg)
        torch.manual_seed(0)
        module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
        tr = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module, fused=fused))
        for _ in range(2):  # the launch and the capture
            tr.iterate()
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        parts = {"collect": [], "gae": [], "update": [], "load_params": []}
        for _ in range(iters):
            ev[0].record()
            frag = tr.rollout.collect()
            ev[1].record()
            adv, targets = ln.gae(frag, tr.gamma, tr.lam, out=(tr._adv, tr._targets))
            ev[2].record()
            tr.learner.update(frag, adv, targets)
            ev[3].record()
            tr.policy.load_params(module)
            ev[4].record()
            torch.cuda.synchronize()
            for i, k in enumerate(parts):
                parts[k].append(ev[i].elapsed_time(ev[i + 1]))
        env.poll_error()
        med = {k + "_ms": float(np.median(v)) for k, v in parts.items()}
        total = sum(med.values())
        emit(dict({"section": "iterate", "workload": TRAINING, "rows": b * env.num_agents, "T": T, "fused": fused, "epochs": 12,
                   "minibatches": 8, "iterate_ms": total, "gae_share": med["gae_ms"] / total, "collect_share": med["collect_ms"] / total,
                   "agent_steps_per_s": b * env.num_agents * T / (total * 1e-3)}, **med))
        env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections = None, ("lstm", "epoch", "iterate")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if "--sections" in argv:
        i = argv.index("--sections")
        sections = tuple(argv[i + 1].split(","))
        del argv[i:i + 2]
    sink = open(path, "w", encoding="utf-8") if path else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if "lstm" in sections:
        for rows in SIZES:
            run_lstm(rows, emit)
    if "epoch" in sections:
        for rows in SIZES:
            run_epoch(rows, emit)
    if "iterate" in sections:
        run_iterate(emit)
