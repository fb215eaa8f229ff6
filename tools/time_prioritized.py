"""Time of the prioritised planner (mapf_plan_prioritized, csrc/mapf_plan.hip) on the device (not a test).  One JSON line
per case:

  launch  one workload of dl_reference_models_amd.workloads (--shape) on connected grids (--density, default 0.2): us per
          call of plan_prioritized at --horizon, of expert_actions("yielding") and of the step, device events around `reps`
          back-to-back calls from Python, three rounds alternating the three; the ratio to one expert launch and to
          makespan expert launches (what replanning every step costs for the same episode); the share of solved envs and
          the plans' sum-of-costs and makespan over their shortest-path lower bounds.  Run under
          `rocprofv3 --kernel-trace --stats` the same process gives the kernel times side by side.
  wall    evaluate(env, "prioritized", 4) next to evaluate(env, "shortest_path", 4) on the training setup (finite mode),
          host wall clock, results and heatmap copied back, alternating, three rounds, and the share of terminated episodes.

    python tools/time_prioritized.py launch --shape c3_8192x32x32_n8 [--horizon 128] [--reps 50] [--out FILE]
    python tools/time_prioritized.py wall [--out FILE]
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
TRAINING = "ref_training_4096x32x32_n16"


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


def _config(shape, density):
    from dl_reference_models_amd.workloads import WORKLOADS, synthetic_grids, workload_config

    B, H, W, N, _d, _over = WORKLOADS[shape]
    cfg = dict(workload_config(shape, range(B)), device="cuda:0")
    cfg["grid"] = synthetic_grids(range(B), H, W, density, N)
    return cfg


def time_launch(shape, horizon, density, reps):
    import numpy as np
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.vec_env import VecReferenceModel

    env = VecReferenceModel(_config(shape, density))
    B, N = env.num_envs, env.num_agents
    env.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(B, N)).astype(np.int8)).to(env.device)
    out = torch.empty((B, N), dtype=torch.int8, device=env.device)
    bufs = env.plan_prioritized(horizon)
    _a, d = env.expert_actions("independent", return_distance=True)
    costs, bounds = evm.plan_costs(bufs[1]), evm.bounds_from_lengths(d.cpu().numpy())
    ok = costs["solved"]
    line = {"case": "launch_" + shape, "lib": os.environ.get("MAPF_LIB", "shipped"), "envs": B, "agents": N, "density": density,
            "horizon": horizon, "solved": round(float(ok.mean()), 4),
            "envs_with_a_path_for_every_agent": round(float((bounds["sum_of_costs_lower_bound"] >= 0).mean()), 4),
            "reps": reps, "timing": "device events around back-to-back calls from Python"}
    if ok.any():
        line["mean_makespan"] = round(float(costs["makespan"][ok].mean()), 2)
        line["sum_of_costs_over_lower_bound"] = round(float(
            (costs["sum_of_costs"][ok] / np.maximum(bounds["sum_of_costs_lower_bound"][ok], 1)).mean()), 4)
        line["makespan_over_lower_bound"] = round(float(
            (costs["makespan"][ok] / np.maximum(bounds["makespan_lower_bound"][ok], 1)).mean()), 4)
    calls = {"us_plan_prioritized": lambda: env.plan_prioritized(horizon, out=bufs),
             "us_expert_yielding": lambda: env.expert_actions("yielding", out=out),
             "us_step": lambda: env.step(acts)}
    # (the planner calls come first in every round: the step moves the agents, the planners' work depends on where they are)
    for _round in range(3):
        for name, fn in calls.items():
            n = reps if name != "us_step" else 10
            for _ in range(3):
                fn()
            line.setdefault(name, []).append(round(_events(fn, n), 2))
        env.reset()
    p, e = min(line["us_plan_prioritized"]), min(line["us_expert_yielding"])
    line["ratio_to_one_expert_launch"] = round(p / e, 2)
    if ok.any():
        line["ratio_to_makespan_expert_launches"] = round(p / (e * line["mean_makespan"]), 3)
    env.poll_error()
    env.close()
    return line


def time_wall():
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.vec_env import VecReferenceModel

    E = 4
    cfg = _config(TRAINING, 0.2)
    line = {"case": "wall_" + TRAINING + "_E4"}
    for _round in range(3):
        for policy in ("shortest_path", "prioritized"):
            env = VecReferenceModel(cfg)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res, _heat = evm.evaluate(env, policy, E)
            line.setdefault(policy + "_wall_s", []).append(round(time.perf_counter() - t, 3))
            line[policy + "_env_steps"] = int(res["timesteps"].sum())
            line[policy + "_terminated"] = round(float((res["terminated"] & ~res["truncated"]).mean()), 4)
            env.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["launch", "wall"])
    ap.add_argument("--shape", default=HEADLINE)
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = time_launch(args.shape, args.horizon, args.density, args.reps) if args.case == "launch" else time_wall()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
