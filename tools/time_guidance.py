#!/usr/bin/env python3
"""What the shortest-path guidance costs (a measurement, not a test), all in this process, three alternating rounds, medians:

    launch   mapf_observe_guided (observation rows in, guided rows out) against mapf_expert_actions(mode 0, dist) on the same
             handle and state, each as a captured graph of 20 launches, at the headline shape, the reference's training
             setup and 1 024 x 64x64 x 64; next to the row traffic the guided launch adds, B N (2 L + 6) 4 bytes, at 8 TB/s
    rollout  Rollout.collect() per step at the training setup with and without guidance
    iterate  one Trainer.iterate() (PPO with its defaults) at the training setup with and without guidance

The paths a caller without the option runs are timed against another checkout by tools/time_bc.py --sections plain --tree DIR
and bench.py.  One JSON object per line; the raw lines are appended when --out is given.

    python tools/time_guidance.py [--out profiles/r26/guidance/time_guidance.jsonl] [--sections launch,rollout,iterate]
"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch
from dl_reference_models_amd import _lib as L
from dl_reference_models_amd import learner as ln
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import DevicePolicy, MaskedRecurrentPolicy
from dl_reference_models_amd.rollout import Rollout
from dl_reference_models_amd.vec_env import VecReferenceModel
from time_learner import DEV, ROUNDS, T, TRAINING, timed

HBM_BYTES_PER_S = 8e12
SHAPES = ("c3_8192x32x32_n8", TRAINING, "c5_1024x64x64_n64_lifelong")
LAUNCHES = 20  # per graph


def _env(shape):
    b = wl.WORKLOADS[shape][0]
    return VecReferenceModel(dict(wl.workload_config(shape, list(range(b))), device=DEV))


def _graph_of(fn):
    fn()
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        for _ in range(LAUNCHES):
            fn()
    torch.cuda.synchronize()
    return g


def run_launch(shape, emit):
    env = _env(shape)
    B, N, Lo = env.num_envs, env.num_agents, env.obs_len
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(B, N)).astype(np.int8)).to(env.device)
    for _ in range(10):  # agents off their start cells, no episode boundary yet
        obs = env.step(acts)["obs"]
    rows = torch.empty((B, N, env.guided_obs_len), dtype=torch.float32, device=env.device)
    six = torch.empty((B, N, L.GUIDANCE_LEN), dtype=torch.float32, device=env.device)
    a_out = torch.empty((B, N), dtype=torch.int8, device=env.device)
    d_out = torch.empty((B, N), dtype=torch.int32, device=env.device)
    stream = lambda: env._stream()  # noqa: E731
    calls = {"expert": lambda: env._check(env._lib.mapf_expert_actions(env._h, 0, a_out.data_ptr(), d_out.data_ptr(), stream())),
             "guided": lambda: env.guided_obs(obs, out=rows), "guidance_only": lambda: env.guidance(out=six)}
    graphs = {k: _graph_of(fn) for k, fn in calls.items()}
    d = d_out.cpu().numpy()
    out = {"section": "launch", "shape": shape, "searches": B * N, "obs_len": Lo, "launches_per_graph": LAUNCHES,
           "unreachable": round(float((d < 0).mean()), 4), "mean_path": round(float(d[d >= 0].mean()), 2),
           "added_bytes": B * N * (2 * Lo + L.GUIDANCE_LEN) * 4,
           "added_traffic_floor_us_at_8TBps": B * N * (2 * Lo + L.GUIDANCE_LEN) * 4 / HBM_BYTES_PER_S * 1e6}
    for r in range(ROUNDS):
        for k, g in graphs.items():
            out[f"{k}_us_round{r}"] = 1e3 * timed(g.replay, 20) / LAUNCHES
    for k in graphs:
        out[k + "_us"] = float(np.median([out[f"{k}_us_round{r}"] for r in range(ROUNDS)]))
    out["guided_minus_expert_us"] = out["guided_us"] - out["expert_us"]
    env.poll_error()
    env.close()
    emit(out)


def _module(env, guidance):
    torch.manual_seed(0)
    return MaskedRecurrentPolicy(env.guided_obs_len if guidance else env.obs_len, has_mask=False, recurrent=True)


def run_rollout(emit, reps=5):
    made = {}
    for name, guidance in (("plain", False), ("guided", True)):
        env = _env(TRAINING)
        ro = Rollout(env, DevicePolicy(_module(env, guidance), env.num_envs * env.num_agents, env.num_agents, env.device), T,
                     guidance=guidance)
        for _ in range(3):  # the launch, the capture and a replay
            ro.collect()
        made[name] = (env, ro)
    out = {"section": "rollout", "workload": TRAINING, "T": T}
    for r in range(ROUNDS):
        for name, (_env_, ro) in made.items():
            out[f"{name}_us_per_step_round{r}"] = 1e3 * timed(ro.collect, reps) / T
    for name, (env, _ro) in made.items():
        out[name + "_us_per_step"] = float(np.median([out[f"{name}_us_per_step_round{r}"] for r in range(ROUNDS)]))
        env.poll_error()
        env.close()
    out["guided_minus_plain_us_per_step"] = out["guided_us_per_step"] - out["plain_us_per_step"]
    emit(out)


def run_iterate(emit, iters=3):
    made = {}
    for name, guidance in (("plain", False), ("guided", True)):
        env = _env(TRAINING)
        module = _module(env, guidance).to(env.device)
        tr = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module), guidance=guidance)
        for _ in range(2):  # the launch and the capture
            tr.iterate()
        made[name] = (env, tr)
    out = {"section": "iterate", "workload": TRAINING, "T": T, "learner": "PPOLearner(module)"}
    for r in range(ROUNDS):
        for name, (_env_, tr) in made.items():
            ms = []
            for _ in range(iters):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                tr.iterate()
                ms.append(1e3 * (time.perf_counter() - t0))
            out[f"{name}_iterate_ms_round{r}"] = float(np.median(ms))
    for name, (env, _tr) in made.items():
        out[name + "_iterate_ms"] = float(np.median([out[f"{name}_iterate_ms_round{r}"] for r in range(ROUNDS)]))
        env.poll_error()
        env.close()
    emit(out)


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, sections = None, ("launch", "rollout", "iterate")
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

    if "launch" in sections:
        for shape in SHAPES:
            run_launch(shape, emit)
    if "rollout" in sections:
        run_rollout(emit)
    if "iterate" in sections:
        run_iterate(emit)
