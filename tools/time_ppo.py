#!/usr/bin/env python3
"""What PPO's objective costs with the KL penalty (a measurement, modelled on tools/time_impala.py), the fused objective
(mapf_ppo_loss) against the torch composition, all in this process:

    objective the objective alone on given logits and values, forward plus backward: learner._PPOLoss (one launch, the sum of
              the partials, two scalings) against learner.ppo_objective (torch ops), T = 32 at 8 192 and 65 536 rows with one
              head and at 8 192 env rows with 4 heads, with the number of kernels each launches (torch.profiler)
    kernel    the bare mapf_ppo_loss launch at the same shapes, next to its traffic at 8 TB/s
    epoch     one PPOLearner.update epoch (8 minibatches) with a KL coefficient on a synthetic fragment, fused objective
              against torch ops (the recurrence on the sequence kernels in both)
    iterate   one Trainer.iterate() at the reference's training setup: kl_coeff None (the defaults), 0.2 with torch ops, 0.2
              with the fused objective
    plain     the kl_coeff None iteration alone, through nothing newer than Trainer / PPOLearner(module): with --tree DIR the
              package is imported from DIR, so another checkout (the parent commit, built) is timed by the same code in the
              same session

Three alternating rounds each, medians.  One JSON object per line; the raw lines are appended when --out is given.

    python tools/time_ppo.py [--out profiles/r22/ppo/time_ppo.jsonl] [--sections objective,kernel,epoch,iterate] [--tree DIR]
"""
import copy, ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TREE = os.path.abspath(sys.argv[sys.argv.index("--tree") + 1]) if "--tree" in sys.argv else ROOT
sys.path.insert(0, TREE)
sys.path.insert(0, os.path.join(TREE, "tools"))
import torch
from dl_reference_models_amd import _lib as L
from dl_reference_models_amd import learner as ln
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import MaskedRecurrentPolicy
from dl_reference_models_amd.vec_env import VecReferenceModel
from time_learner import DEV, ROUNDS, SIZES, T, TRAINING, rounds, synthetic_fragment, timed
from time_impala import count_kernels

HBM_BYTES_PER_S = 8e12
SHAPES = tuple((rows, 1) for rows in SIZES) + ((SIZES[0], 4),)  # (rows, heads)
SCALARS = (0.05, 10.0, 0.5, 0.001)  # clip, vf_clip, vf_coeff, ent_coeff: the reference's
KL = 0.2


def bytes_per_element(heads):
    """Each array counted once (the second read of the logits comes from L2): both sets of logits 40 h in, dlogits 20 h out,
    old_logp / adv / value / target 16 in, the action bytes h in, logp / kl / dvalues 12 out."""
    return 61 * heads + 28


def objective_inputs(rows, heads):
    g = torch.Generator(device=DEV).manual_seed(2)
    r = lambda *s: torch.randn(s, device=DEV, generator=g)  # noqa: E731
    logits = (2 * r(T, rows, 5 * heads)).requires_grad_(True)
    values = r(T, rows).requires_grad_(True)
    actions = (torch.rand((T, rows, heads), device=DEV, generator=g) * 5).to(torch.int8).clamp_(0, 4)
    with torch.no_grad():
        old_logits = logits + 0.3 * r(T, rows, 5 * heads)
        logp = torch.log_softmax(logits.unflatten(2, (heads, 5)), dim=3).gather(3, actions.to(torch.int64)[..., None])[..., 0].sum(2)
    coeff = torch.full((1,), KL, device=DEV)
    return logits, values, actions, logp + 0.05 * r(T, rows), r(T, rows), values.detach() + r(T, rows), old_logits, coeff


def run_objective(rows, heads, emit):
    logits, values, actions, old_logp, adv, targets, old_logits, coeff = objective_inputs(rows, heads)

    def fused():
        total = ln._PPOLoss.apply(logits, values, actions, old_logp, adv, targets, old_logits, coeff, heads, 1, SCALARS)[0]
        torch.autograd.grad(total.sum(), [logits, values])

    def composed():
        per, _ = ln.ppo_objective(logits, values, actions, old_logp, adv, targets, *SCALARS, old_logits, coeff)
        torch.autograd.grad(per["total_loss"], [logits, values])

    out = {"section": "objective", "T": T, "rows": rows, "heads": heads}
    out.update(rounds({"fused": fused, "torch": composed}, {"fused": 20, "torch": 5}))
    for name, fn in (("fused", fused), ("torch", composed)):
        out[name + "_kernels"], why = count_kernels(fn)
        if why:
            out[name + "_kernels_note"] = why
    emit(out)


def run_kernel(rows, heads, emit):
    lib = L.load()
    logits, values, actions, old_logp, adv, targets, old_logits, coeff = (x.detach() for x in objective_inputs(rows, heads))
    logp, kl, dv = (torch.empty((T, rows), device=DEV) for _ in range(3))
    dl = torch.empty_like(logits)
    partials = torch.empty((lib.mapf_ppo_partials(rows, 1), 5), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fn():
        rc = lib.mapf_ppo_loss(T, rows, heads, 1, p(logits), p(old_logits), p(actions), p(old_logp), p(adv), p(values), p(targets),
                               *SCALARS, p(coeff), p(logp), p(kl), p(dl), p(dv), p(partials), stream)
        assert rc == 0

    ms = [timed(fn, 50) for _ in range(ROUNDS)]
    floor_us = T * rows * bytes_per_element(heads) / HBM_BYTES_PER_S * 1e6
    emit({"section": "kernel", "T": T, "rows": rows, "heads": heads, "workgroups": int(partials.shape[0]),
          "kernel_us_rounds": [1e3 * m for m in ms], "kernel_us": 1e3 * float(np.median(ms)),
          "bytes_per_element": bytes_per_element(heads), "traffic_floor_us_at_8TBps": floor_us})


def run_epoch(rows, emit):
    frag = synthetic_fragment(rows)
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(52, has_mask=False, recurrent=True).to(DEV)
    with torch.no_grad():
        frag["logits"] = ln.sequence_forward(module, frag)[0].unflatten(1, frag["value"].shape[1:]).contiguous()
    adv, targets = ln.gae(frag)
    learners = {k: ln.PPOLearner(copy.deepcopy(module), epochs=1, minibatches=8, kl_coeff=KL, fused_objective=(k == "fused"))
                for k in ("fused", "torch")}
    out = {"section": "epoch", "T": T, "rows": rows, "minibatches": 8, "kl_coeff": KL}
    out.update(rounds({k: (lambda le=le: le.update(frag, adv, targets)) for k, le in learners.items()}, {"fused": 3, "torch": 3}))
    emit(out)


def _iterate(make_learner, iters):
    b = wl.WORKLOADS[TRAINING][0]
    env = VecReferenceModel(wl.workload_config(TRAINING, list(range(b))))
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(env.obs_len, has_mask=False, recurrent=True).to(env.device)
    learner = make_learner(module)
    tr = ln.Trainer(env, module, T=T, learner=learner)
    for _ in range(2):  # the launch and the capture
        tr.iterate()
    ms = []
    for _ in range(iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        tr.iterate()
        ms.append(1e3 * (time.perf_counter() - t0))
    env.poll_error()
    rows = b * env.num_agents
    env.close()
    return {"workload": TRAINING, "rows": rows, "T": T, "epochs": learner.epochs, "minibatches": learner.minibatches,
            "iterate_ms_each": ms, "iterate_ms": float(np.median(ms)), "agent_steps_per_s": rows * T / (float(np.median(ms)) * 1e-3)}


def run_iterate(emit, iters=3):
    for r in range(ROUNDS):
        for name, kw in (("none", {}), ("kl_torch", {"kl_coeff": KL, "fused_objective": False}),
                         ("kl_fused", {"kl_coeff": KL, "fused_objective": True})):
            emit({"section": "iterate", "round": r, "learner": name, **_iterate(lambda m: ln.PPOLearner(m, **kw), iters)})


def run_plain(emit, iters=4):
    emit({"section": "plain", "tree": os.path.relpath(TREE, ROOT), **_iterate(lambda m: ln.PPOLearner(m), iters)})


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections = None, ("objective", "kernel", "epoch", "iterate")
    if "--tree" in argv:
        i = argv.index("--tree")
        del argv[i:i + 2]
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    if "--sections" in argv:
        i = argv.index("--sections")
        sections = tuple(argv[i + 1].split(","))
        del argv[i:i + 2]
    sink = open(path, "a", encoding="utf-8") if path else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    for name, fn in (("objective", run_objective), ("kernel", run_kernel)):
        if name in sections:
            for rows, heads in SHAPES:
                fn(rows, heads, emit)
    if "epoch" in sections:
        for rows in SIZES:
            run_epoch(rows, emit)
    if "iterate" in sections:
        run_iterate(emit)
    if "plain" in sections:
        run_plain(emit)
