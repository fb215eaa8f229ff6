"""Time and quality of conflict-based search (mapf_plan_cbs, csrc/mapf_plan.hip) on the device (not a test).  One JSON line
per case:

  launch  one workload of dl_reference_models_amd.workloads (--shape) on connected grids (--density, default 0.2): us per
          call of plan_cbs at --horizon and every --max-nodes, and of plan_prioritized at the same horizon as the yardstick,
          device events around `reps` back-to-back calls from Python, three rounds alternating them, and the ratio of the
          lowest rounds; the share of envs per status next to the prioritised planner's solved share, the mean nodes created,
          the share of envs only CBS solves, and sum of costs and makespan over their shortest-path lower bounds for both
          planners on the envs both solve; LDS bytes per env and the node store's bytes.
  wall    evaluate(env, "cbs", 4) next to evaluate(env, "prioritized", 4) on the training setup (finite mode), host wall
          clock, results and heatmap copied back, alternating, three rounds, and the share of terminated episodes.

    python tools/time_cbs.py launch --shape c3_8192x32x32_n8 [--horizon 128] [--max-nodes 16 64 256] [--reps 50] [--out FILE]
    python tools/time_cbs.py wall [--out FILE]
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

from time_prioritized import HEADLINE, TRAINING, _config, _events  # noqa: E402


def lds_bytes_per_env(N, T, M):
    """csrc/mapf_plan.hip cbs_env_words: the joint plan, 12 bytes per node, 2 bytes per time step."""
    return 8 * (N * ((T + 5) & ~3) // 4 + ((M + 1) & ~1) * 3 // 2 + ((T + 4) & ~3) // 4)


def time_launch(shape, horizon, budgets, density, reps):
    import numpy as np

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.vec_env import VecReferenceModel

    env = VecReferenceModel(_config(shape, density))
    B, N = env.num_envs, env.num_agents
    env.reset()
    prio = env.plan_prioritized(horizon)
    _a, d = env.expert_actions("independent", return_distance=True)
    bounds = evm.bounds_from_lengths(d.cpu().numpy())
    pc = evm.plan_costs(prio[1])
    line = {"case": "launch_" + shape, "lib": os.environ.get("MAPF_LIB", "shipped"), "envs": B, "agents": N, "density": density,
            "horizon": horizon, "max_nodes": list(budgets), "solved_prioritized": round(float(pc["solved"].mean()), 4),
            "envs_with_a_path_for_every_agent": round(float((bounds["sum_of_costs_lower_bound"] >= 0).mean()), 4),
            "reps": reps, "timing": "device events around back-to-back calls from Python"}
    over = lambda costs, ok, key: round(float((costs[key][ok] / np.maximum(bounds[key + "_lower_bound"][ok], 1)).mean()), 4)
    calls, bufs = {}, {}
    for M in budgets:
        bufs[M] = env.plan_cbs(horizon, M)
        cc = evm.plan_costs(bufs[M]["arrival"])
        both = cc["solved"] & pc["solved"]
        q = dict(evm.cbs_summary(bufs[M]["status"], bufs[M]["nodes"]), only_cbs_solves=round(float((cc["solved"] & ~pc["solved"]).mean()), 4),
                 both_solve=round(float(both.mean()), 4), lds_bytes_per_env=lds_bytes_per_env(N, horizon, M),
                 workspace_bytes=env.plan_cbs_workspace_bytes(horizon, M))
        if both.any():
            for key in ("sum_of_costs", "makespan"):
                q[f"cbs_{key}_over_lower_bound"] = over(cc, both, key)
                q[f"prioritized_{key}_over_lower_bound"] = over(pc, both, key)
        line[f"quality_m{M}"] = {k: round(v, 4) if isinstance(v, float) else v for k, v in q.items()}
        calls[f"us_plan_cbs_m{M}"] = lambda M=M: env.plan_cbs(horizon, M, out=bufs[M])
    env.plan_cbs(horizon, max(budgets))  # (the node store is sized for the largest budget before the timed calls)
    calls["us_plan_prioritized"] = lambda: env.plan_prioritized(horizon, out=prio)
    for _round in range(3):
        for name, fn in calls.items():
            for _ in range(2):
                fn()
            line.setdefault(name, []).append(round(_events(fn, reps), 2))
    for M in budgets:
        line[f"cbs_m{M}_over_prioritized"] = round(min(line[f"us_plan_cbs_m{M}"]) / min(line["us_plan_prioritized"]), 2)
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
        for policy in ("prioritized", "cbs"):
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
    ap.add_argument("--max-nodes", type=int, nargs="+", default=[16, 64, 256])
    ap.add_argument("--density", type=float, default=0.2)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    line = time_launch(args.shape, args.horizon, args.max_nodes, args.density, args.reps) if args.case == "launch" else time_wall()
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
