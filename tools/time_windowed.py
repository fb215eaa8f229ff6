"""Time of the windowed prioritised planner (mapf_plan_windowed, csrc/mapf_plan.hip) on the device (not a test).  One JSON
line per case:

  launch  one workload of dl_reference_models_amd.workloads (--shape) on connected grids (--density, default 0.2): us per
          call of plan_windowed at every --windows, of plan_prioritized at --horizon, of expert_actions("yielding") and of
          the step, and of both planners with an all-zero mask (the idle call of a policy that has nothing to replan);
          device events around `reps` back-to-back calls from Python, three rounds alternating all of them in one
          process; the share of consistent envs and the agents that arrive within each window.
  wall    evaluate(env, policy, 2) in LIFELONG mode on --shape: "shortest_path" next to "windowed" at the default (16, 8)
          and windowed with replan_on_arrival; host wall clock, results and heatmap copied back, alternating, three
          rounds; mean goals_reached_total and throughput of the episodes.

    python tools/time_windowed.py launch --shape c3_8192x32x32_n8 [--windows 8 16 32] [--horizon 128] [--reps 50] [--out FILE]
    python tools/time_windowed.py wall --shape ref_training_4096x32x32_n16 [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_prioritized import HEADLINE, _config, _events  # noqa: E402


def time_launch(shape, windows, horizon, density, reps):
    import numpy as np
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.vec_env import VecReferenceModel

    env = VecReferenceModel(_config(shape, density))
    B, N = env.num_envs, env.num_agents
    env.reset()
    acts = torch.from_numpy(np.random.default_rng(0).integers(0, 5, size=(B, N)).astype(np.int8)).to(env.device)
    out = torch.empty((B, N), dtype=torch.int8, device=env.device)
    zero = torch.zeros((B,), dtype=torch.uint8, device=env.device)
    prio = env.plan_prioritized(horizon)
    line = {"case": "launch_" + shape, "lib": os.environ.get("MAPF_LIB", "shipped"), "envs": B, "agents": N, "density": density,
            "horizon": horizon, "windows": list(windows), "solved_prioritized": round(float(evm.plan_costs(prio[1])["solved"].mean()), 4),
            "reps": reps, "timing": "device events around back-to-back calls from Python"}
    win = {}
    for w in windows:
        win[w] = env.plan_windowed(w)
        costs = evm.window_costs(win[w][1], win[w][2])
        ok = costs["consistent"]
        line[f"consistent_w{w}"] = round(float(ok.mean()), 4)
        if ok.any():
            line[f"mean_arrived_w{w}"] = round(float(costs["arrived"][ok].mean()), 2)
    calls = {f"us_plan_windowed_w{w}": (lambda w=w: env.plan_windowed(w, out=win[w])) for w in windows}
    calls["us_plan_prioritized"] = lambda: env.plan_prioritized(horizon, out=prio)
    w_idle = windows[len(windows) // 2]
    calls[f"us_idle_windowed_w{w_idle}"] = lambda: env.plan_windowed(w_idle, mask=zero, out=win[w_idle])
    calls["us_idle_prioritized"] = lambda: env.plan_prioritized(horizon, mask=zero, out=prio)
    calls["us_expert_yielding"] = lambda: env.expert_actions("yielding", out=out)
    calls["us_step"] = lambda: env.step(acts)
    # (the planner calls come first in every round: the step moves the agents, the planners' work depends on where they are)
    for _round in range(3):
        for name, fn in calls.items():
            n = reps if name != "us_step" else 10
            for _ in range(3):
                fn()
            line.setdefault(name, []).append(round(_events(fn, n), 2))
        env.reset()
    line["idle_windowed_over_idle_prioritized"] = round(min(line[f"us_idle_windowed_w{w_idle}"]) / min(line["us_idle_prioritized"]), 4)
    env.poll_error()
    env.close()
    return line


def time_wall(shape, density):
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.vec_env import VecReferenceModel

    E = 2
    cfg = dict(_config(shape, density), lifelong_mapf=True)
    line = {"case": "wall_lifelong_" + shape + "_E2", "density": density, "steps_per_episode": cfg["steps_per_episode"]}
    policies = {"shortest_path": lambda env: "shortest_path", "windowed_16_8": lambda env: "windowed",
                "windowed_16_8_on_arrival": lambda env: evm.windowed_policy(env, 16, 8, replan_on_arrival=True)}
    for _round in range(3):
        for name, make in policies.items():
            env = VecReferenceModel(cfg)
            policy = make(env)
            torch.cuda.synchronize()
            t = time.perf_counter()
            res, _heat = evm.evaluate(env, policy, E)
            line.setdefault(name + "_wall_s", []).append(round(time.perf_counter() - t, 3))
            stats = evm.summary(res, lifelong=True)
            line[name + "_env_steps"] = int(res["timesteps"].sum())
            line[name + "_mean_goals_reached_total"] = round(stats["average goals_reached_total"], 3)
            line[name + "_mean_throughput"] = round(stats["average throughput"], 5)
            line[name + "_mean_completion_ratio"] = round(stats["average completion_ratio"], 4)
            env.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("case", choices=["launch", "wall"])
    ap.add_argument("--shape", default=HEADLINE)
    ap.add_argument("--windows", type=int, nargs="+", default=[8, 16, 32])
    ap.add_argument("--horizon", type=int, default=128)
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = time_launch(args.shape, args.windows, args.horizon, args.density, args.reps) if args.case == "launch" \
        else time_wall(args.shape, args.density)
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
