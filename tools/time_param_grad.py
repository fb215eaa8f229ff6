#!/usr/bin/env python3
"""What the learner's parameter gradients cost (a measurement, modelled on tools/time_trunk.py): the split-row reductions
(mapf_trunk_param_grad, mapf_lstm_seq_param_grad; ``fused_grads=True``) against the GEMMs and column sums, all in this process:

    kernels   the two C calls alone on M = 32 x 8 192 and 32 x 65 536 rows at the training setup's observation (F = 53, L = 58),
              recurrent and feed-forward, dW_hh with 1 and 16 groups, next to their derived floors (traffic at 8 TB/s, products
              on the f32-input MFMA at 157 TF)
    trunk     learner.dense_trunk(fused=True) forward plus backward with the option on and off, same shapes
    lstm      learner.lstm_sequence(fused=True) forward plus backward with the option on and off, groups 1 and 16
    epoch     one PPOLearner.update epoch (8 minibatches) on the training setup's fragment: the defaults (off), fused_trunk
              alone (trunk), fused_trunk with fused_grads (on)
    iterate   one Trainer.iterate() at the reference's training setup, the same three variants

Three alternating rounds each, medians.  One JSON object per line; the raw lines are kept when --out is given.

    python tools/time_param_grad.py [--out profiles/r29/param_grad/time_param_grad.jsonl] [--sections kernels,trunk,lstm,epoch,iterate]
                                    [--root DIR] [--variants off,trunk,on] [--tag NAME]

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
F, LO = 53, 58
GROUPS = (1, 16)
TRAINING = "ref_training_4096x32x32_n16"
DEV = "cuda:0"
HBM_BYTES_PER_S, MFMA_FLOP_PER_S = 8e12, 157e12
KW = {"off": {}, "trunk": {"fused_trunk": True}, "on": {"fused_trunk": True, "fused_grads": True}}  # (off: no keyword: any tree takes it)


def floors_us(M, recurrent):
    """Derived, not measured: the operand rows at 8 TB/s and the products (bias columns included) at 157 TF."""
    trunk_b = 4 * M * (F + 4 * 64 + (256 + 3 if recurrent else 0))
    trunk_f = 2 * M * (64 * (F + 1) + 64 * 65 + (256 * 71 if recurrent else 0))
    return {"trunk_hbm_us": 1e6 * trunk_b / HBM_BYTES_PER_S, "trunk_mfma_us": 1e6 * trunk_f / MFMA_FLOP_PER_S,
            "dwhh_hbm_us": 1e6 * 4 * M * (256 + 64 + 0.25) / HBM_BYTES_PER_S, "dwhh_mfma_us": 1e6 * 2 * M * 256 * 64 / MFMA_FLOP_PER_S}


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


def rounds(fns: dict, reps: int) -> dict:
    out = {}
    for r in range(ROUNDS):
        for kind, fn in fns.items():
            out[f"{kind}_ms_round{r}"] = timed(fn, reps)
    for kind in fns:
        out[kind + "_ms"] = float(np.median([out[f"{kind}_ms_round{r}"] for r in range(ROUNDS)]))
    if "on" in fns:
        base = "trunk" if "trunk" in fns else "off"
        out[f"on_faster_than_{base}_in_every_round"] = all(out[f"on_ms_round{r}"] < out[f"{base}_ms_round{r}"] for r in range(ROUNDS))
        out[f"{base}_over_on"] = out[base + "_ms"] / out["on_ms"]
    return out


def vp(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def trunk_inputs(rows, recurrent):
    g = torch.Generator(device=DEV).manual_seed(0)
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(LO, has_mask=True, recurrent=recurrent).to(DEV)
    obs = (torch.rand((T, rows, LO), device=DEV, generator=g) < 0.3).float()
    pa = (torch.rand((T, rows, 1), device=DEV, generator=g) * 5).to(torch.int8).clamp_(0, 4)
    pr = torch.rand((T, rows), device=DEV, generator=g) - 0.5
    first = (torch.rand((T, rows), device=DEV, generator=g) < 1 / 64).to(torch.uint8)
    up = torch.randn((T, rows, 256 if recurrent else 64), device=DEV, generator=g)
    return module, obs, pa, pr, first, up


def run_kernels(rows, emit):
    lib, M = L.load(), T * rows
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    out = {"section": "kernels", "T": T, "rows": rows, "M": M, "F": F, "L": LO}
    for recurrent in (True, False):
        _module, obs, pa, pr, first, up = trunk_inputs(rows, recurrent)
        a1, a2, d1, d2 = (torch.randn((M, 64), device=DEV) for _ in range(4))
        dw1, db1, dw2, db2 = (torch.empty(s, device=DEV) for s in ((64, F), (64,), (64, 64), (64,)))
        dwih, dbl = (torch.empty((256, 70), device=DEV), torch.empty(256, device=DEV)) if recurrent else (None, None)
        size = int(lib.mapf_param_grad_workspace_bytes(M, F, int(recurrent), 0))
        ws = torch.empty(size, dtype=torch.uint8, device=DEV)
        pa8, f8 = pa.reshape(M).contiguous(), first.reshape(M).contiguous()

        def trunk_only():
            rc = lib.mapf_trunk_param_grad(M, F, LO, int(recurrent), vp(obs), vp(pa8), vp(pr), vp(f8), vp(a1), vp(a2), vp(d1), vp(d2),
                                           vp(up) if recurrent else None, vp(dw1), vp(db1), vp(dw2), vp(db2), vp(dwih), vp(dbl), vp(ws), size, stream)
            assert rc == 0, rc

        key = "trunk_recurrent" if recurrent else "trunk_feed_forward"
        out[key + "_us"] = 1e3 * float(np.median([timed(trunk_only, 10) for _ in range(ROUNDS)]))
        out[key + "_workspace_bytes"] = size
        fl = floors_us(M, recurrent)
        out[key + "_floors"] = {k: v for k, v in fl.items() if k.startswith("trunk")}
        out[key + "_over_floor"] = out[key + "_us"] / max(fl["trunk_hbm_us"], fl["trunk_mfma_us"])
        del a1, a2, d1, d2, obs, up, ws
    dxg, h = torch.randn((T, rows, 256), device=DEV), torch.rand((T, rows, 64), device=DEV)
    h0, reset = torch.rand((rows, 64), device=DEV), (torch.rand((T, rows), device=DEV) < 1 / 64).to(torch.uint8)
    for groups in GROUPS:
        dwhh = torch.empty((groups, 256, 64), device=DEV)
        size = int(lib.mapf_param_grad_workspace_bytes(M, 0, 0, groups))
        ws = torch.empty(size, dtype=torch.uint8, device=DEV)

        def dwhh_only():
            rc = lib.mapf_lstm_seq_param_grad(T, rows, groups, vp(dxg), vp(h), vp(h0), vp(reset), vp(dwhh), vp(ws), size, stream)
            assert rc == 0, rc

        out[f"dwhh_groups{groups}_us"] = 1e3 * float(np.median([timed(dwhh_only, 10) for _ in range(ROUNDS)]))
        out[f"dwhh_groups{groups}_workspace_bytes"] = size
        fl = floors_us(M, True)
        out[f"dwhh_groups{groups}_over_floor"] = out[f"dwhh_groups{groups}_us"] / max(fl["dwhh_hbm_us"], fl["dwhh_mfma_us"])
    out["dwhh_floors"] = {k: v for k, v in floors_us(M, True).items() if k.startswith("dwhh")}
    emit(out)


def run_trunk(rows, recurrent, emit):
    module, obs, pa, pr, first, up = trunk_inputs(rows, recurrent)
    params = [p for n, p in module.named_parameters() if n.split(".")[0] in ("fc1", "fc2", "lstm") and n != "lstm.weight_hh"]

    def both(fused_grads):
        def fn():
            a2, xg = ln.dense_trunk(module, obs, pa, pr, first, fused=True, fused_grads=fused_grads)
            torch.autograd.grad(xg if recurrent else a2, params, grad_outputs=up)
        return fn

    out = {"section": "trunk", "T": T, "rows": rows, "M": T * rows, "F": F, "L": LO, "recurrent": recurrent,
           "note": "dense_trunk(fused=True) forward + backward; on = fused_grads=True, off = the GEMMs and column sums"}
    out.update(rounds({"on": both(True), "off": both(False)}, 5))
    emit(out)


def run_lstm(rows, groups, emit):
    g = torch.Generator(device=DEV).manual_seed(0)
    xg = torch.randn((T, rows, 256), device=DEV, generator=g)
    whh = ((torch.rand((groups, 256, 64) if groups > 1 else (256, 64), device=DEV, generator=g) - 0.5) / 4).requires_grad_(True)
    reset = (torch.rand((T, rows), device=DEV, generator=g) < 1 / 64).to(torch.uint8)
    h0, c0 = torch.rand((rows, 64), device=DEV, generator=g) - 0.5, torch.randn((rows, 64), device=DEV, generator=g)
    dh = torch.randn((T, rows, 64), device=DEV, generator=g)

    def both(fused_grads):
        def fn():
            h, _state = ln.lstm_sequence(xg, whh, reset, h0, c0, fused=True, fused_grads=fused_grads)
            torch.autograd.grad(h, [whh], grad_outputs=dh)
        return fn

    out = {"section": "lstm", "T": T, "rows": rows, "M": T * rows, "groups": groups,
           "note": "lstm_sequence(fused=True) forward + backward; on = fused_grads=True, off = hprev built and one (batched) GEMM"}
    out.update(rounds({"on": both(True), "off": both(False)}, 5))
    emit(out)


def training_env():
    b = wl.WORKLOADS[TRAINING][0]
    return VecReferenceModel(wl.workload_config(TRAINING, list(range(b))))


def run_epoch(variants, emit):
    env = training_env()
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
    tr = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module))
    tr.rollout.collect()
    frag = {k: v.clone() for k, v in tr.rollout.collect().items()}
    adv, targets = (x.clone() for x in ln.gae(frag))
    learners = {v: ln.PPOLearner(copy.deepcopy(module), epochs=1, minibatches=8, **KW[v]) for v in variants}
    out = {"section": "epoch", "workload": TRAINING, "T": T, "rows": env.num_envs * env.num_agents, "L": env.obs_len, "minibatches": 8,
           "note": "off = no keyword, trunk = fused_trunk=True, on = fused_trunk=True and fused_grads=True"}
    out.update(rounds({v: (lambda le=le: le.update(frag, adv, targets)) for v, le in learners.items()}, 3))
    env.poll_error()
    emit(out)
    env.close()


def run_iterate(variants, emit, tag, iters=3):
    envs, trainers = {}, {}
    for v in variants:  # (an env of its own each: a trainer owns its env's rollout)
        env = envs[v] = training_env()
        torch.manual_seed(0)
        module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
        trainers[v] = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module, **KW[v]))
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
            out[f"{v}_ms_round{r}"] = e0.elapsed_time(e1) / iters
    for v in trainers:
        out[f"{v}_ms"] = float(np.median([out[f"{v}_ms_round{r}"] for r in range(ROUNDS)]))
    if "on" in trainers:
        for base in ("off", "trunk"):
            if base in trainers:
                out[f"on_faster_than_{base}_in_every_round"] = all(out[f"on_ms_round{r}"] < out[f"{base}_ms_round{r}"] for r in range(ROUNDS))
                out[f"{base}_over_on"] = out[f"{base}_ms"] / out["on_ms"]
    for env in envs.values():
        env.poll_error()
    emit(out)
    for env in envs.values():
        env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections, variants, tag = None, ("kernels", "trunk", "lstm", "epoch", "iterate"), ("off", "trunk", "on"), "this"

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

    if "kernels" in sections:
        for rows in SIZES:
            run_kernels(rows, emit)
    if "trunk" in sections:
        for rows in SIZES:
            for recurrent in (True, False):
                run_trunk(rows, recurrent, emit)
    if "lstm" in sections:
        for rows in SIZES:
            for groups in GROUPS:
                run_lstm(rows, groups, emit)
    if "epoch" in sections:
        run_epoch(variants, emit)
    if "iterate" in sections:
        run_iterate(variants, emit, tag)
