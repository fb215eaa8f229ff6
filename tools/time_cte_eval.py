"""Time of the batched evaluation of the single-agent env (mapf_cte_eval_record, evaluation.JointEvaluator) on the device
(not a test).  One JSON line per case and shape; the shapes are the two single-agent workloads, 8192 envs x 16x16 x 4
agents and 1024 envs x 32x32 x 8 agents.

  step    us per call from device events around `reps` back-to-back calls of (i) mapf_cte_step_masked alone with every
          env active and no auto-reset, (ii) JointEvaluator.step -- the same masked step, the recorder launch and the
          masked reset, (iii) the recorder launch alone (terminated / truncated cleared, so every launch books a step
          of every env and ends no episode).  Run under `rocprofv3 --kernel-trace --stats` the same process gives the
          kernel times of the step kernel, k_cte_eval_record and the reset kernel side by side.
  ma      (iii) for the multi-agent recorder, k_eval_record, at its own headline shape (8192 envs x 32x32 x 8 agents) in
          the same process: the one comparison this tool is for.
  wall    evaluate(env, "random", 4) end to end (host wall clock, results and heatmap copied back), the same with a
          freshly initialised recurrent joint policy (joint_neural_policy), and the same bookkeeping through the
          per-object facade in a Python loop (main.py's loop for a gym.Env) for 8 envs x 4 episodes.

    python tools/time_cte_eval.py [--cases step ma wall] [--reps 300] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = ("cte_8192x16x16_n4", "cte_1024x32x32_n8")
MA_HEADLINE = "c3_8192x32x32_n8"


def _events(fn, reps):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def _make(name):
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel
    from dl_reference_models_amd.workloads import WORKLOADS, workload_config

    return VecSingleAgentReferenceModel(dict(workload_config(name, range(WORKLOADS[name][0])), device="cuda:0"))


def time_step(name, reps):
    import torch

    from dl_reference_models_amd.evaluation import JointEvaluator

    env = _make(name)
    B, N = env.num_envs, env.num_agents
    gen = torch.Generator(device=env.device)
    gen.manual_seed(0)
    acts = torch.randint(0, 5, (64, B, N), generator=gen, device=env.device, dtype=torch.int8)
    ones = torch.ones((B,), dtype=torch.uint8, device=env.device)
    # E large enough that no env finishes inside the timed windows: every launch does the full work
    ev = JointEvaluator(env, max(4, (3 * reps + 200) // env.steps_per_episode + 2))
    ev.begin()
    i = [0]

    def masked_alone():
        env.step_masked(acts[i[0] % 64], ones, auto_reset=False)
        i[0] += 1

    def three_launches():
        ev.step(acts[i[0] % 64])
        i[0] += 1

    lib, h = env._lib, env._h
    outs = (env._reward.data_ptr(), env._terminated.data_ptr(), env._truncated.data_ptr(), env._info.data_ptr())

    def record_alone():
        lib.mapf_cte_eval_record(h, *outs, env._stream())

    for _ in range(50):
        three_launches()
    torch.cuda.synchronize()
    us3 = _events(three_launches, reps)
    env._terminated.zero_()
    env._truncated.zero_()
    for _ in range(20):
        record_alone()
    torch.cuda.synchronize()
    us_rec = _events(record_alone, reps)
    # the masked step by itself needs its resets too, or every env sits at the step limit: time it on the same handle
    # after a reset of every env, for less than one episode
    env.reset()
    torch.cuda.synchronize()
    us1 = _events(masked_alone, min(reps, env.steps_per_episode - 1))
    env.poll_error()
    line = {"case": "step_" + name, "us_masked_step_alone": round(us1, 2), "us_three_launch_step": round(us3, 2),
            "us_record_launch_alone": round(us_rec, 2), "ns_record_per_env": round(us_rec * 1e3 / B, 3), "reps": reps,
            "lanes_per_env_step": env.launch_info()["lanes_per_env"],
            "timing": "device events around back-to-back calls from Python"}
    ev.end()
    env.close()
    return line


def time_ma_record(reps):
    import torch

    from dl_reference_models_amd.evaluation import Evaluator
    from dl_reference_models_amd.vec_env import VecReferenceModel
    from dl_reference_models_amd.workloads import workload_config

    env = VecReferenceModel(dict(workload_config(MA_HEADLINE, range(8192)), device="cuda:0"))
    B, N = env.num_envs, env.num_agents
    ev = Evaluator(env, 4)
    ev.begin()
    env.step(torch.ones((B, N), dtype=torch.int8, device=env.device), auto_reset=False)
    env._terminated.zero_()
    env._truncated.zero_()
    lib, h = env._lib, env._h
    outs = (env._rewards.data_ptr(), env._terminated.data_ptr(), env._truncated.data_ptr(), env._info_all.data_ptr())

    def record_alone():
        lib.mapf_eval_record(h, *outs, env._stream())

    for _ in range(20):
        record_alone()
    torch.cuda.synchronize()
    runs = [_events(record_alone, reps) for _ in range(3)]
    line = {"case": "ma_record_" + MA_HEADLINE, "us_record_launch_alone": [round(r, 2) for r in runs],
            "ns_record_per_env": round(min(runs) * 1e3 / B, 3), "reps": reps,
            "timing": "device events around back-to-back calls from Python"}
    ev.end()
    env.close()
    return line


def time_wall(name):
    import numpy as np
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.policy import JointActionPolicy
    from dl_reference_models_amd.reference_model_single_agent import ReferenceModel
    from dl_reference_models_amd.workloads import WORKLOADS, synthetic_grid, workload_config

    E = 4
    _b, H, W, N, density = WORKLOADS[name][:5]
    out = {"case": "wall_" + name + "_E4"}
    torch.manual_seed(0)
    module = JointActionPolicy(H * W, N, recurrent=True)
    for key, make in (("random", lambda env: "random"), ("recurrent_joint_policy", lambda env: evm.joint_neural_policy(env, module))):
        runs = []
        for _ in range(3):
            env = _make(name)
            policy = make(env)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res, _heat = evm.evaluate(env, policy, E)
            runs.append(time.perf_counter() - t)
            env.close()
        out[f"evaluate_{key}_wall_s"] = [round(r, 3) for r in runs]
        out[f"evaluate_{key}_wall_s_best"] = round(min(runs), 3)
        out[f"{key}_episodes"], out[f"{key}_env_steps"] = len(res["env"]), int(res["timesteps"].sum())

    # the per-object loop: 8 envs one after another, main.py's bookkeeping in Python
    rng = np.random.default_rng(0)
    cfg = {k: v for k, v in workload_config(name, range(8)).items() if k not in ("grid", "seeds", "num_envs")}
    t = time.perf_counter()
    f_steps = 0
    for b in range(8):
        env = ReferenceModel(dict(cfg, grid=synthetic_grid(b, H, W, density, N), seed=b))
        occupancy = np.zeros((H, W), dtype=int)
        for _ep in range(E):
            env.reset()
            done, total = False, 0
            while not done:
                _obs, reward, terminated, truncated, _info = env.step(rng.integers(0, 5, size=N))
                done = terminated or truncated
                total += reward
                f_steps += 1
                for y, x in env.positions.values():
                    occupancy[y, x] += 1
    facade = time.perf_counter() - t
    out.update(facade_loop_8_envs_s=round(facade, 3), facade_env_steps=f_steps,
               note="the facade loop is serial per env: 8 envs measured, nothing extrapolated")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["step", "ma", "wall"])
    ap.add_argument("--shapes", nargs="*", default=list(SHAPES))
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    for case in args.cases:
        lines = [time_ma_record(args.reps)] if case == "ma" else \
            [time_step(s, args.reps) if case == "step" else time_wall(s) for s in args.shapes]
        for line in lines:
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
