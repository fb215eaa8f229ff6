#!/usr/bin/env python3
"""What DQN costs on the device (a measurement, after tools/time_impala.py): each fused path against its torch composition, all
in this process, three alternating rounds each, medians.  Rows 8 192 and 65 536, L = 52, a ring of 64 slots, K = 4 000.

    act       mapf_qnet_act against the same module composed of torch ops (forward, argmax and the epsilon draw), each replayed
              from its own captured graph, next to the launch's traffic at 8 TB/s
    sample    mapf_replay_sample against torch.cumsum + torch.searchsorted on the same weights
    objective the TD objective forward plus backward: dqn._TDLoss (one launch) against dqn.td_objective (torch ops), with the
              bare launch next to its traffic
    append    ReplayBuffer.append of one T = 32 fragment, next to its traffic
    iterate   one DQNTrainer.iterate() at the reference's training setup, fused and not

One JSON object per line; the raw lines are kept when --out is given.

    python tools/time_dqn.py [--out profiles/r16/dqn/time_dqn.jsonl] [--sections act,sample,objective,append,iterate]
"""
import ctypes as C, json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from dl_reference_models_amd import _lib as L
from dl_reference_models_amd import dqn
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.vec_env import VecReferenceModel
from time_learner import DEV, ROUNDS, SIZES, T, TRAINING, rounds, timed

OBS_LEN, SLOTS, K = 52, 64, 4000
HBM_BYTES_PER_S = 8e12


def run_act(rows, emit):
    torch.manual_seed(0)
    module = dqn.QNetwork(OBS_LEN).to(DEV)
    pol = dqn.DeviceQPolicy(module, rows, DEV)
    g0 = torch.Generator(device=DEV).manual_seed(1)
    obs = torch.rand((rows, OBS_LEN), device=DEV, generator=g0)
    eps = torch.full((1,), 0.3, device=DEV)
    u = torch.empty((rows,), device=DEV)
    r = torch.empty((rows,), device=DEV)
    action = torch.empty((rows,), dtype=torch.int64, device=DEV)

    def composed():
        with torch.no_grad():
            q = module(obs)
            u.uniform_()
            r.uniform_()
            torch.where(u < eps, (r * 5).to(torch.int64).clamp_(max=4), q.argmax(dim=1), out=action)

    graphs = {}
    for name, fn in (("fused", lambda: pol.act(obs, epsilon=eps)), ("torch", composed)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            fn()
        graphs[name] = g
    out = {"section": "act", "rows": rows, "obs_len": OBS_LEN}
    out.update(rounds({k: g.replay for k, g in graphs.items()}, {"fused": 50, "torch": 50}))
    nbytes = rows * (4 * OBS_LEN + 4 + 4 + 1 + 20)  # obs in, draws in and out, action and q out
    out.update(bytes=nbytes, traffic_floor_us_at_8TBps=nbytes / HBM_BYTES_PER_S * 1e6,
               mfma_instructions_per_tile=(OBS_LEN + 1) // 2 + 32)
    emit(out)
    pol.close()


def run_sample(rows, emit):
    buf = dqn.ReplayBuffer(rows, 1, (SLOTS - 1) * rows, DEV)
    assert buf.slots == SLOTS
    g0 = torch.Generator(device=DEV).manual_seed(2)
    buf.w.copy_((torch.rand(buf.w.shape, device=DEV, generator=g0) * (1 << 18)).to(torch.int32) + 1)
    buf.w[3].zero_()
    flat = buf.w.view(-1)

    def composed():
        cs = torch.cumsum(flat, 0, dtype=torch.int64)
        W = cs[-1]
        k = torch.arange(K, device=DEV, dtype=torch.int64)
        lo, hi = k * W // K, (k + 1) * W // K
        x = torch.randint(0, 1 << 62, (K,), device=DEV)
        idx = torch.searchsorted(cs, lo + x % (hi - lo).clamp_(min=1), right=True)
        return idx, flat[idx], W, (flat != 0).sum()

    out = {"section": "sample", "rows": rows, "slots": SLOTS, "count": buf.count, "K": K}
    out.update(rounds({"fused": lambda: buf.sample(K, 0), "torch": composed}, {"fused": 50, "torch": 20}))
    out.update(bytes=4 * buf.count, traffic_floor_us_at_8TBps=4 * buf.count / HBM_BYTES_PER_S * 1e6, launches=3)
    emit(out)


def run_objective(rows, emit):
    g0 = torch.Generator(device=DEV).manual_seed(3)
    r = lambda *s: torch.randn(s, device=DEV, generator=g0)  # noqa: E731
    q = (2 * r(K, 5)).requires_grad_(True)
    on, tg, reward = 2 * r(K, 5), 2 * r(K, 5), r(K)
    action = (torch.rand((K,), device=DEV, generator=g0) * 5).to(torch.int8).clamp_(0, 4)
    ended = (torch.rand((K,), device=DEV, generator=g0) < 0.05).to(torch.uint8)
    isw = torch.rand((K,), device=DEV, generator=g0)
    scalars = (C.c_float(0.99), C.c_float(1.0), C.c_float(0.6))

    def fused():
        torch.autograd.grad(dqn._TDLoss.apply(q, on, tg, action, reward, ended, isw, scalars, None, None)[0], q)

    def composed():
        torch.autograd.grad(dqn.td_objective(q, on, tg, action, reward, ended, isw)["loss"], q)

    out = {"section": "objective", "K": K, "note": "K does not depend on the rows; one line"}
    out.update(rounds({"fused": fused, "torch": composed}, {"fused": 50, "torch": 20}))
    lib = L.load()
    dq, new_w = torch.empty((K, 5), device=DEV), torch.empty((K,), dtype=torch.int32, device=DEV)
    partials = torch.empty((lib.mapf_dqn_td_partials(K), 2), device=DEV)
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    qd = q.detach()

    def bare():
        assert lib.mapf_dqn_td_loss(K, p(qd), p(on), p(tg), p(action), p(reward), p(ended), p(isw), *scalars, None, None, 0, None, p(dq),
                                    p(new_w), p(partials), stream) == 0

    ms = [timed(bare, 100) for _ in range(ROUNDS)]
    nbytes = K * (60 + 1 + 4 + 1 + 4 + 20 + 4)
    out.update(kernel_us_rounds=[1e3 * m for m in ms], kernel_us=1e3 * float(np.median(ms)), bytes=nbytes,
               traffic_floor_us_at_8TBps=nbytes / HBM_BYTES_PER_S * 1e6)
    emit(out)


def run_append(rows, emit):
    B, N = rows // 16, 16
    buf = dqn.ReplayBuffer(rows, OBS_LEN, (SLOTS - 1) * rows, DEV)
    g0 = torch.Generator(device=DEV).manual_seed(4)
    frag = {"obs": torch.rand((T + 1, B, N, OBS_LEN), device=DEV, generator=g0), "actions": torch.zeros((T, B, N), dtype=torch.int8, device=DEV),
            "rewards": torch.rand((T, B, N), device=DEV, generator=g0), "terminated": torch.zeros((T, B), dtype=torch.uint8, device=DEV),
            "truncated": torch.zeros((T, B), dtype=torch.uint8, device=DEV)}
    ms = [timed(lambda: buf.append(frag), 10) for _ in range(ROUNDS)]
    nbytes = 2 * T * rows * (4 * OBS_LEN + 1 + 4 + 1) + T * rows * 4  # every slab read and written once, the weights written
    emit({"section": "append", "rows": rows, "T": T, "obs_len": OBS_LEN, "append_ms_rounds": ms, "append_ms": float(np.median(ms)),
          "bytes": nbytes, "traffic_floor_ms_at_8TBps": nbytes / HBM_BYTES_PER_S * 1e3})


def run_iterate(emit, iters=6):
    b = wl.WORKLOADS[TRAINING][0]
    cfg = wl.workload_config(TRAINING, list(range(b)))
    results = {}
    trainers = {}
    for fused in (True, False):
        env = VecReferenceModel(cfg)
        torch.manual_seed(0)
        module = dqn.QNetwork(env.obs_len).to(env.device)
        tr = dqn.DQNTrainer(env, module, T=T, learner=dqn.DQNLearner(module, fused=fused))
        for _ in range(2):  # the launch and the capture
            tr.iterate()
        trainers[fused] = (env, tr)
        results[fused] = []
    for _ in range(ROUNDS):  # alternating rounds
        for fused, (env, tr) in trainers.items():
            ms = []
            for _ in range(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.iterate()
                ms.append(1e3 * (time.perf_counter() - t0))
            results[fused].append(float(np.median(ms)))
    for fused, (env, tr) in trainers.items():
        upd = [timed(lambda: tr.learner.update(tr.buffer, tr.updates), 3) for _ in range(ROUNDS)]
        env.poll_error()
        total = float(np.median(results[fused]))
        emit({"section": "iterate", "workload": TRAINING, "fused": fused, "rows": b * env.num_agents, "T": T, "updates": tr.updates,
              "train_batch": tr.learner.train_batch, "slots": tr.buffer.slots, "iterate_ms_rounds": results[fused], "iterate_ms": total,
              "update_ms": float(np.median(upd)), "agent_steps_per_s": b * env.num_agents * T / (total * 1e-3)})
        env.close()
    emit({"section": "iterate", "fused_faster_in_every_round": all(a < c for a, c in zip(results[True], results[False]))})


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections = None, ("act", "sample", "objective", "append", "iterate")
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

    for name, fn in (("act", run_act), ("sample", run_sample), ("append", run_append)):
        if name in sections:
            for rows in SIZES:
                fn(rows, emit)
    if "objective" in sections:
        run_objective(SIZES[0], emit)
    if "iterate" in sections:
        run_iterate(emit)
