#!/usr/bin/env python3
"""What the learner's dense trunk costs (a measurement, modelled on tools/time_learner.py), the fused kernels (mapf_trunk_*)
against the composition of torch ops, all in this process:

    trunk     learner.dense_trunk forward plus backward (one launch each plus the parameter-gradient GEMMs, against fc1 / tanh
              / fc2 / tanh / one_hot / cat / the W_ih GEMM under autograd) on M = 32 x 8 192 and 32 x 65 536 rows, recurrent and
              feed-forward, at the training setup's observation (F = 53, L = 58) and the headline shape's (F = 28, L = 33); the
              two launches alone next to their floors
    epoch     one PPOLearner.update epoch (8 minibatches) on the training setup's fragment, with and without fused_trunk
    iterate   one Trainer.iterate() at the reference's training setup, with and without fused_trunk

Three alternating rounds each, medians.  One JSON object per line; the raw lines are kept when --out is given.

    python tools/time_trunk.py [--out profiles/r28/trunk/time_trunk.jsonl] [--sections trunk,epoch,iterate]
                               [--root DIR] [--variants off,on] [--tag NAME]

--root: import the package from another checkout (the parent commit's, to show that the path without the option did not
move: run --sections iterate --variants off alternately from both trees; a tree without the option takes --variants off only).
"""
import copy, ctypes as C, json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if "--root" in sys.argv:
    ROOT = os.path.abspath(sys.argv[sys.argv.index("--root") + 1])
sys.path.insert(0, ROOT)
import torch
from dl_reference_models_amd import _lib as L
from dl_reference_models_amd import learner as ln
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import MaskedRecurrentPolicy
from dl_reference_models_amd.vec_env import VecReferenceModel

T = 32
ROUNDS = 3
SIZES = (8192, 65536)
OBS = {"training": (53, 58), "headline": (28, 33)}  # (F, L)
TRAINING = "ref_training_4096x32x32_n16"
DEV = "cuda:0"
HBM_BYTES_PER_S, MFMA_FLOP_PER_S = 8e12, 157e12


def floors_us(M, F, L, recurrent):
    """Derived, not measured: the bytes each launch must move at 8 TB/s and its products on the f32-input MFMA at 157 TF."""
    out_f = 4 * M * (64 + 64 + (256 if recurrent else 0))
    flop_f = 2 * M * (F * 64 + 64 * 64 + (70 * 256 if recurrent else 0))
    in_b = 4 * M * ((256 if recurrent else 64) + 64 + 64)
    flop_b = 2 * M * ((256 * 64 if recurrent else 0) + 64 * 64)
    return {"forward_hbm_us": 1e6 * (4 * M * L + out_f) / HBM_BYTES_PER_S, "forward_mfma_us": 1e6 * flop_f / MFMA_FLOP_PER_S,
            "backward_hbm_us": 1e6 * (in_b + 4 * M * 128) / HBM_BYTES_PER_S, "backward_mfma_us": 1e6 * flop_b / MFMA_FLOP_PER_S}


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
    if "fused" in fns and "torch" in fns:
        out["fused_faster_in_every_round"] = all(out[f"fused_ms_round{r}"] < out[f"torch_ms_round{r}"] for r in range(ROUNDS))
        out["torch_over_fused"] = out["torch_ms"] / out["fused_ms"]
    return out


def run_trunk(rows, name, recurrent, emit):
    F, Lo = OBS[name]
    M = T * rows
    g = torch.Generator(device=DEV).manual_seed(0)
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(Lo, has_mask=True, recurrent=recurrent).to(DEV)
    obs = (torch.rand((T, rows, Lo), device=DEV, generator=g) < 0.3).float()
    pa = (torch.rand((T, rows, 1), device=DEV, generator=g) * 5).to(torch.int8).clamp_(0, 4)
    pr = torch.rand((T, rows), device=DEV, generator=g) - 0.5
    first = (torch.rand((T, rows), device=DEV, generator=g) < 1 / 64).to(torch.uint8)
    up = torch.randn((T, rows, 256 if recurrent else 64), device=DEV, generator=g)
    params = [p for n, p in module.named_parameters() if n.split(".")[0] in ("fc1", "fc2", "lstm") and n != "lstm.weight_hh"]

    def both(fused):
        def fn():
            a2, xg = ln.dense_trunk(module, obs, pa, pr, first, fused=fused)
            torch.autograd.grad(xg if recurrent else a2, params, grad_outputs=up)
        return fn

    # the two launches alone, on the tensors an autograd pass would hand them
    lib, vp = L.load(), lambda t: None if t is None else C.c_void_p(t.data_ptr())  # noqa: E731
    a1, a2 = torch.empty((M, 64), device=DEV), torch.empty((M, 64), device=DEV)
    xg = torch.empty((M, 256), device=DEV) if recurrent else None
    d2, d1 = torch.empty_like(a2), torch.empty_like(a1)
    w = {n: p.detach() for n, p in module.named_parameters()}
    wih, bih, bhh = (w.get("lstm." + k) for k in ("weight_ih", "bias_ih", "bias_hh"))
    pa8, f8 = pa.reshape(M).contiguous(), first.reshape(M).contiguous()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def forward_only():
        rc = lib.mapf_trunk_forward(M, F, Lo, int(recurrent), vp(obs), vp(pa8), vp(pr), vp(f8), vp(w["fc1.weight"]), vp(w["fc1.bias"]),
                                    vp(w["fc2.weight"]), vp(w["fc2.bias"]), vp(wih), vp(bih), vp(bhh), vp(a1), vp(a2), vp(xg), stream)
        assert rc == 0, rc

    def backward_only():
        rc = lib.mapf_trunk_backward(M, int(recurrent), vp(up) if recurrent else None, None if recurrent else vp(up), vp(a1), vp(a2),
                                     vp(wih), vp(w["fc2.weight"]), vp(d2), vp(d1), stream)
        assert rc == 0, rc

    out = {"section": "trunk", "T": T, "rows": rows, "M": M, "obs": name, "F": F, "L": Lo, "recurrent": recurrent}
    out.update(rounds({"fused": both(True), "torch": both(False)}, {"fused": 5, "torch": 3}))
    out["forward_kernel_us"] = 1e3 * float(np.median([timed(forward_only, 10) for _ in range(ROUNDS)]))
    out["backward_kernel_us"] = 1e3 * float(np.median([timed(backward_only, 10) for _ in range(ROUNDS)]))
    out["floors"] = floors_us(M, F, Lo, recurrent)
    emit(out)


def training_env():
    b = wl.WORKLOADS[TRAINING][0]
    return VecReferenceModel(wl.workload_config(TRAINING, list(range(b))))


def learner_kw(variant):
    return {"fused_trunk": True} if variant == "on" else {}  # (off: the keyword is not passed, so an older tree takes it)


def run_epoch(variants, emit):
    env = training_env()
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
    tr = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module))
    tr.rollout.collect()
    frag = {k: v.clone() for k, v in tr.rollout.collect().items()}
    adv, targets = (x.clone() for x in ln.gae(frag))
    learners = {v: ln.PPOLearner(copy.deepcopy(module), epochs=1, minibatches=8, **learner_kw(v)) for v in variants}
    names = {"on": "fused", "off": "torch"}
    out = {"section": "epoch", "workload": TRAINING, "T": T, "rows": env.num_envs * env.num_agents, "L": env.obs_len, "minibatches": 8,
           "note": "fused = fused_trunk=True, torch = the option not passed; the recurrence and the objective are as in the defaults"}
    out.update(rounds({names[v]: (lambda le=le: le.update(frag, adv, targets)) for v, le in learners.items()}, {"fused": 3, "torch": 3}))
    env.poll_error()
    emit(out)
    env.close()


def run_iterate(variants, emit, tag, iters=3):
    envs, trainers = {}, {}
    for v in variants:  # (an env of its own each: a trainer owns its env's rollout)
        env = envs[v] = training_env()
        torch.manual_seed(0)
        module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
        trainers[v] = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module, **learner_kw(v)))
        for _ in range(2):  # the launch and the capture
            trainers[v].iterate()
    out = {"section": "iterate", "workload": TRAINING, "rows": env.num_envs * env.num_agents, "T": T, "epochs": 12, "minibatches": 8,
           "tree": tag}
    for r in range(ROUNDS):
        for v, tr in trainers.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(iters):
                tr.iterate()
            e1.record()
            torch.cuda.synchronize()
            out[f"fused_trunk_{v}_ms_round{r}"] = e0.elapsed_time(e1) / iters
    for v in trainers:
        out[f"fused_trunk_{v}_ms"] = float(np.median([out[f"fused_trunk_{v}_ms_round{r}"] for r in range(ROUNDS)]))
    if len(trainers) == 2:
        out["on_faster_in_every_round"] = all(out[f"fused_trunk_on_ms_round{r}"] < out[f"fused_trunk_off_ms_round{r}"] for r in range(ROUNDS))
        out["off_over_on"] = out["fused_trunk_off_ms"] / out["fused_trunk_on_ms"]
    for env in envs.values():
        env.poll_error()
    emit(out)
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections, variants, tag = None, ("trunk", "epoch", "iterate"), ("off", "on"), "this"

    def option(name, default):
        if name in argv:
            i = argv.index(name)
            value = argv[i + 1]
            del argv[i:i + 2]
            return value
        return default

    path = option("--out", None)
    sections = tuple(option("--sections", ",".join(sections)).split(","))
    variants = tuple(option("--variants", ",".join(variants)).split(","))
    tag = option("--tag", tag)
    option("--root", None)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    sink = open(path, "a", encoding="utf-8") if path else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if "trunk" in sections:
        for rows in SIZES:
            for name in OBS:
                for recurrent in (True, False):
                    run_trunk(rows, name, recurrent, emit)
    if "epoch" in sections:
        run_epoch(variants, emit)
    if "iterate" in sections:
        run_iterate(variants, emit, tag)
