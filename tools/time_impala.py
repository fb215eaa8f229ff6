#!/usr/bin/env python3
"""What the IMPALA learner costs (a measurement, modelled on tools/time_learner.py), the fused path against the torch
composition, all in this process:

    losses    IMPALALearner.losses plus backward on a synthetic fragment of the training setup's shape, T = 32 at 8 192 and
              65 536 rows, fused (sequence kernels + mapf_vtrace_loss) against fused=False (torch ops throughout)
    objective the objective alone on given logits and values, forward plus backward: learner._VtraceLoss (one launch, the sum of
              the partials, two scalings) against learner.impala_objective (torch ops), with the number of kernels the torch
              composition launches (torch.profiler) next to its time
    kernel    the bare mapf_vtrace_loss launch at both sizes, next to its traffic at 8 TB/s
    iterate   one Trainer.iterate() with an IMPALALearner at the reference's training setup, next to the PPO iteration of the
              same session

Three alternating rounds each, medians.  One JSON object per line; the raw lines are kept when --out is given.

    python tools/time_impala.py [--out profiles/r15/impala/time_impala.jsonl] [--sections losses,objective,kernel,iterate]
"""
import copy, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from dl_reference_models_amd import _lib as L
from dl_reference_models_amd import learner as ln
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import MaskedRecurrentPolicy
from dl_reference_models_amd.vec_env import VecReferenceModel
from time_learner import DEV, ROUNDS, SIZES, T, TRAINING, rounds, synthetic_fragment, timed

# bytes the kernel moves per (t, row) with one head, each counted once (the second read of the logits comes from L2): logits
# 20 in, dlogits 20 out, behaviour logp / value / reward 12 in, action and flag 2 in, vs / pg_adv / dvalues 12 out
BYTES_PER_ELEMENT = 66
HBM_BYTES_PER_S = 8e12


def objective_inputs(rows):
    g = torch.Generator(device=DEV).manual_seed(2)
    r = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
    logits = (2 * r(T, rows, 5)).requires_grad_(True)
    values = r(T, rows).requires_grad_(True)
    actions = (torch.rand((T, rows, 1), device=DEV, generator=g) * 5).to(torch.int8).clamp_(0, 4)
    with torch.no_grad():
        logp = torch.log_softmax(logits, dim=2).gather(2, actions.to(torch.int64))[..., 0]
    ended = (torch.rand((T, rows), device=DEV, generator=g) < 1 / 64).to(torch.uint8)
    return logits, values, actions, logp + 0.5 * r(T, rows), r(T, rows), ended, r(rows)


def run_losses(rows, emit):
    frag = synthetic_fragment(rows)
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(52, has_mask=False, recurrent=True).to(DEV)
    learners = {k: ln.IMPALALearner(copy.deepcopy(module), fused=(k == "fused")) for k in ("fused", "torch")}

    def both(le):
        view = ln.fragment_view(frag, le.module)

        def fn():
            le.module.zero_grad(set_to_none=True)
            le.losses(frag, None, view)["total_loss"].backward()
        return fn

    out = {"section": "losses", "T": T, "rows": rows}
    out.update(rounds({k: both(le) for k, le in learners.items()}, {"fused": 5, "torch": 2}))
    emit(out)


def count_kernels(fn):
    """Kernels one call of fn launches, from torch.profiler; None (and why) when the profiler gives no device events here."""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        n = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
        return (n or None), (None if n else "the profiler recorded no device events")
    except Exception as e:  # a measurement aid: say so and go on
        return None, repr(e)


def run_objective(rows, emit):
    logits, values, actions, mu, rewards, ended, boot = objective_inputs(rows)
    scalars = (0.99, 1.0, 1.0, 1.0, 1.0, 0.5, 0.0)

    def fused():
        total = ln._VtraceLoss.apply(logits, values, actions, mu, rewards, ended, boot, 1, scalars)[0]
        torch.autograd.grad(total, [logits, values])

    def composed():
        terms, _ = ln.impala_objective(logits, values, actions, mu, rewards, ended, boot, *scalars)
        torch.autograd.grad(terms["total_loss"], [logits, values])

    out = {"section": "objective", "T": T, "rows": rows}
    out.update(rounds({"fused": fused, "torch": composed}, {"fused": 20, "torch": 5}))
    for name, fn in (("fused", fused), ("torch", composed)):
        out[name + "_kernels"], why = count_kernels(fn)
        if why:
            out[name + "_kernels_note"] = why
    emit(out)


def run_kernel(rows, emit):
    lib = L.load()
    logits, values, actions, mu, rewards, ended, boot = (x.detach() for x in objective_inputs(rows))
    vs, pg, dv = (torch.empty((T, rows), device=DEV) for _ in range(3))
    dl = torch.empty_like(logits)
    partials = torch.empty((lib.mapf_vtrace_partials(rows), 4), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.mapf_vtrace_loss(T, rows, 1, p(logits), p(actions), p(mu), p(values), p(rewards), p(ended), p(boot), 0.99, 1.0, 1.0,
                                  1.0, 1.0, 0.5, 0.0, p(vs), p(pg), None, p(dl), p(dv), p(partials), stream)
        assert rc == 0

    ms = [timed(fn, 50) for _ in range(ROUNDS)]
    floor_us = T * rows * BYTES_PER_ELEMENT / HBM_BYTES_PER_S * 1e6
    emit({"section": "kernel", "T": T, "rows": rows, "workgroups": int(partials.shape[0]), "kernel_us_rounds": [1e3 * m for m in ms],
          "kernel_us": 1e3 * float(np.median(ms)), "bytes_per_element": BYTES_PER_ELEMENT, "traffic_floor_us_at_8TBps": floor_us})


def run_iterate(emit, iters=4):
    b = wl.WORKLOADS[TRAINING][0]
    cfg = wl.workload_config(TRAINING, list(range(b)))
    for algo, fused in (("IMPALA", True), ("IMPALA", False), ("PPO", True)):
        env = VecReferenceModel(cfg)
        torch.manual_seed(0)
        module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
        learner = ln.IMPALALearner(module, fused=fused) if algo == "IMPALA" else ln.PPOLearner(module, fused=fused)
        tr = ln.Trainer(env, module, T=T, learner=learner)
        for _ in range(2):  # the launch and the capture
            tr.iterate()
        ms, update_ms = [], []
        for _ in range(iters):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            tr.iterate()
            ms.append(1e3 * (time.perf_counter() - t0))
        if algo == "IMPALA":
            frag = tr.rollout.collect()
            update_ms = [timed(lambda: learner.update(frag), 2) for _ in range(ROUNDS)]
        env.poll_error()
        total = float(np.median(ms))
        emit({"section": "iterate", "workload": TRAINING, "algo": algo, "fused": fused, "rows": b * env.num_agents, "T": T,
              "epochs": learner.epochs, "minibatches": learner.minibatches, "iterate_ms_each": ms, "iterate_ms": total,
              "update_ms": float(np.median(update_ms)) if update_ms else None,
              "agent_steps_per_s": b * env.num_agents * T / (total * 1e-3)})
        env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections = None, ("losses", "objective", "kernel", "iterate")
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

    for name, fn in (("losses", run_losses), ("objective", run_objective), ("kernel", run_kernel)):
        if name in sections:
            for rows in SIZES:
                fn(rows, emit)
    if "iterate" in sections:
        run_iterate(emit)
