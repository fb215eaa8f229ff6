"""Time of the shortest-path planner (mapf_expert_actions, csrc/mapf_plan.hip) on the device (not a test).  One JSON line
per case:

  launch  one workload of dl_reference_models_amd.workloads (--shape): us per call of expert_actions in both modes and of
          the step, device events around `reps` back-to-back calls from Python, three rounds alternating the three; plus
          what the searches looked like (share of unreachable goals, mean and longest path).  Run under
          `rocprofv3 --kernel-trace --stats` the same process gives the kernel times of k_plan_expert<false> /
          k_plan_expert<true> and the step kernel side by side.
  wall    evaluate(env, "shortest_path", 4) next to evaluate(env, "random", 4) at 8192 envs of the headline shape, host
          wall clock, results and heatmap copied back, alternating, three rounds.

    python tools/time_plan.py launch --shape c3_8192x32x32_n8 [--reps 300] [--out FILE]
    python tools/time_plan.py wall [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HEADLINE = "c3_8192x32x32_n8"


def _events(fn, reps):
    import torch

    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def time_launch(shape, reps):
    import numpy as np
    import torch

    from dl_reference_models_amd.vec_env import VecReferenceModel
    from dl_reference_models_amd.workloads import WORKLOADS, workload_config

    B = WORKLOADS[shape][0]
    env = VecReferenceModel(dict(workload_config(shape, range(B)), device="cuda:0"))
    N = env.num_agents
    env.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(B, N)).astype(np.int8)).to(env.device)
    for _ in range(10):  # agents off their start cells, no episode boundary yet
        env.step(acts)
    out = torch.empty((B, N), dtype=torch.int8, device=env.device)
    _a, d = env.expert_actions("independent", return_distance=True)
    d = d.cpu().numpy()
    line = {"case": "launch_" + shape, "lib": os.environ.get("MAPF_LIB", "shipped"), "searches": int(d.size),
            "unreachable": round(float((d < 0).mean()), 4), "mean_path": round(float(d[d >= 0].mean()), 2),
            "longest_path": int(d.max()), "reps": reps, "timing": "device events around back-to-back calls from Python"}
    calls = {"us_expert_independent": lambda: env.expert_actions("independent", out=out),
             "us_expert_yielding": lambda: env.expert_actions("yielding", out=out),
             "us_step": lambda: env.step(acts)}
    for _round in range(3):
        for name, fn in calls.items():
            for _ in range(20):
                fn()
            line.setdefault(name, []).append(round(_events(fn, reps), 2))
    env.poll_error()
    env.close()
    return line


def time_wall():
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.vec_env import VecReferenceModel
    from dl_reference_models_amd.workloads import workload_config

    E = 4
    cfg = dict(workload_config(HEADLINE, range(8192)), device="cuda:0")
    line = {"case": "wall_8192x32x32_n8_E4"}
    for _round in range(3):
        for policy in ("random", "shortest_path"):
            env = VecReferenceModel(cfg)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res, _heat = evm.evaluate(env, policy, E)
            line.setdefault(policy + "_wall_s", []).append(round(time.perf_counter() - t, 3))
            line[policy + "_env_steps"] = int(res["timesteps"].sum())
            line[policy + "_success_rate"] = round(float((res["terminated"] & ~res["truncated"]).mean()), 4)
            if policy == "shortest_path" and _round == 0:
                b = evm.path_length_bounds(env, res)
                ok = b["sum_of_costs_lower_bound"] >= 0
                line["episodes_with_a_path_for_every_agent"] = round(float(ok.mean()), 4)
            env.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["launch", "wall"])
    ap.add_argument("--shape", default=HEADLINE)
    ap.add_argument("--reps", type=int, default=300)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = time_launch(args.shape, args.reps) if args.case == "launch" else time_wall()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
