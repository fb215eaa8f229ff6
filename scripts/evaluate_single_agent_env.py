#!/usr/bin/env python3
"""Evaluate a policy on the single-agent grid environment (HIP engine): result rows and visit heatmap.

Sibling of ``scripts/evaluate_multi_agent_env.py`` for the reference's ``training_execution_mode = "CTE"``, where one policy
moves all N agents of an env.  The reference's test mode has no such branch ("test only works with CTDE for now",
main.py:37); this is its loop (main.py:172-324) restated for a gym.Env.  It runs ``--episodes`` episodes of ``--num-envs``
envs -- env b seeded with ``--seed`` + b -- in one batch on the device, writes one CSV row per episode (``episode``,
``seed``, ``total_reward``, ``timesteps``, ``goals_reached_total``, ``blocking_count_total``, the agents' starts and goals,
``env``) and the "Number of visits" heatmap as ``.npy`` (and as ``.pdf`` when matplotlib is there).  Policies: ``RANDOM``,
``SHORTEST_PATH`` / ``SHORTEST_PATH_INDEPENDENT`` (the on-device shortest-path expert, yielding to other agents or ignoring
them; the summary then also holds the mean sum-of-costs and makespan lower bounds of the episodes), or ``NEURAL``: a
``JointActionPolicy`` checkpoint as ``scripts/train_single_agent_env.py`` writes it, given as ``--checkpoint PATH``, run as
one fused launch per step; greedy, or sampled with ``--sample``.  The env is a single-agent workload of
``dl_reference_models_amd.workloads`` (``--workload``, default ``cte_8192x16x16_n4``) or given by ``--env-name``.
``--save-video`` and ``--save-trajectories`` write a GIF and the ``.npz`` of the first ``--video-episodes`` episodes of
``--video-envs``, as in the multi-agent script; the CSV rows of those episodes then end with the path columns.

    python scripts/evaluate_single_agent_env.py --policy NEURAL --checkpoint joint.pt --episodes 4
    python scripts/evaluate_single_agent_env.py --env-name ReferenceModel-2-1 --num-agents 4 --num-envs 1024 --episodes 4
"""

from __future__ import annotations

import argparse
import json
import sys
from datetime import datetime, timezone
from pathlib import Path

import numpy as np

PROJECT_ROOT = Path(__file__).resolve().parents[1]
if str(PROJECT_ROOT) not in sys.path:
    sys.path.insert(0, str(PROJECT_ROOT))

DEFAULT_WORKLOAD = "cte_8192x16x16_n4"
BUILTIN_POLICIES = ("RANDOM", "SHORTEST_PATH", "SHORTEST_PATH_INDEPENDENT", "NEURAL")


def parse_args(argv=None) -> argparse.Namespace:
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--policy", default="RANDOM", help="RANDOM, SHORTEST_PATH, SHORTEST_PATH_INDEPENDENT or NEURAL (with --checkpoint)")
    p.add_argument("--checkpoint", default=None, help="NEURAL: a file written by JointActionPolicy.save")
    p.add_argument("--sample", action="store_true", help="NEURAL: sample from the policy instead of taking the greedy action")
    p.add_argument("--workload", default=None, help=f"a single-agent workload of dl_reference_models_amd.workloads (default {DEFAULT_WORKLOAD} "
                                                    "unless --env-name is given)")
    p.add_argument("--env-name", default=None, help="a named grid of the reference instead of a workload")
    p.add_argument("--num-agents", type=int, default=4, help="with --env-name")
    p.add_argument("--steps-per-episode", type=int, default=None, help="default: the workload's, or 100")
    p.add_argument("--deterministic", action="store_true")
    p.add_argument("--num-envs", type=int, default=None, help="default: the workload's, or 1 with --env-name")
    p.add_argument("--episodes", type=int, default=100, help="episodes per env (main.py: num_episodes)")
    p.add_argument("--seed", type=int, default=42, help="env b is seeded with seed + b; RANDOM and --sample draw from this seed too")
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--poll-every", type=int, default=32)
    p.add_argument("--output-dir", type=Path, default=Path("experiments/results"))
    add_trace_arguments(p)
    return p.parse_args(argv)


def add_trace_arguments(p: argparse.ArgumentParser) -> None:
    """main.py's SAVE_VIDEO switches (main.py:49-52, same defaults) and the trajectories behind the video."""
    p.add_argument("--save-video", action="store_true", help="write a GIF of the first episodes of --video-envs (main.py: SAVE_VIDEO; needs PIL)")
    p.add_argument("--save-trajectories", action="store_true", help="write the traced episodes as .npz (evaluation.Trace.load reads it)")
    p.add_argument("--video-envs", type=int, nargs="+", default=[0], help="envs of the batch to trace")
    p.add_argument("--video-episodes", type=int, default=5, help="episodes per traced env (main.py: VIDEO_EPISODES_TO_SAVE)")
    p.add_argument("--video-fps", type=int, default=5, help="main.py: VIDEO_FRAME_RATE")
    p.add_argument("--video-final-hold", type=int, default=3, help="main.py: VIDEO_FINAL_FRAME_HOLD")
    p.add_argument("--video-cell-px", type=int, default=32, help="pixels per grid cell of a frame")


def make_env(args):
    """``(env, name, env_config)``: the env, the name the output files carry and what the summary records."""
    from dl_reference_models_amd import workloads as wl
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    if args.env_name and not args.workload:
        cfg = {"env_name": args.env_name, "seed": args.seed, "deterministic": args.deterministic, "num_agents": args.num_agents,
               "steps_per_episode": args.steps_per_episode or 100}
        return VecSingleAgentReferenceModel(dict(cfg, num_envs=args.num_envs or 1, device=args.device)), args.env_name, cfg
    name = args.workload or DEFAULT_WORKLOAD
    if name not in wl.WORKLOADS or not wl.is_single_agent(name):
        raise SystemExit(f"--workload must be one of {[k for k in wl.WORKLOADS if wl.is_single_agent(k)]}")
    b = args.num_envs or wl.WORKLOADS[name][0]
    cfg = wl.workload_config(name, list(range(b)))
    cfg["seeds"] = [args.seed + i for i in range(b)]
    cfg["device"] = args.device
    if args.steps_per_episode:
        cfg["steps_per_episode"] = args.steps_per_episode
    if args.deterministic:
        cfg["deterministic"] = True
    env = VecSingleAgentReferenceModel(cfg)
    return env, name, {"workload": name, "seed": args.seed, "deterministic": env.deterministic, "num_agents": env.num_agents,
                       "steps_per_episode": env.steps_per_episode}


def main(argv=None) -> dict:
    args = parse_args(argv)
    algo = args.policy.upper()
    if algo not in BUILTIN_POLICIES:
        raise SystemExit(f"--policy must be one of {BUILTIN_POLICIES} (the coordinated planners are stated for the multi-agent "
                         "env only: scripts/evaluate_multi_agent_env.py)")
    if algo == "NEURAL" and not args.checkpoint:
        raise SystemExit("--policy NEURAL needs --checkpoint PATH")
    from dl_reference_models_amd import evaluation as ev

    env, name, env_config = make_env(args)
    policy = algo.lower()
    if algo == "NEURAL":
        policy = ev.joint_neural_policy(env, args.checkpoint, sample=args.sample, seed=args.seed)
    spec = ev.TraceSpec(args.video_envs, args.video_episodes) if args.save_video or args.save_trajectories else None
    results, heat, *rest = ev.evaluate(env, policy, args.episodes, poll_every=args.poll_every, seed=args.seed, trace=spec)
    trace = rest[0] if rest else None
    table = ev.results_table(results, trace=trace)  # (traced episodes: with the planner result files' path columns)
    stats = ev.summary(results)
    print("Average reward:", stats["average reward"])
    print("Average timesteps:", stats["average timesteps"])
    print("Success rate:", stats["success rate"] * 100, "%")
    if algo.startswith("SHORTEST_PATH"):
        # what the expert's own episodes are measured against: no plan beats these (episodes with an unreachable goal
        # carry -1 and are left out of the means)
        bounds = ev.path_length_bounds(env, results)
        ok = bounds["sum_of_costs_lower_bound"] >= 0
        stats["episodes with a path for every agent"] = int(ok.sum())
        for key in ("sum_of_costs_lower_bound", "makespan_lower_bound"):
            stats["average " + key] = float(bounds[key][ok].mean()) if ok.any() else None
            print(f"Average {key}:", stats["average " + key])

    args.output_dir.mkdir(parents=True, exist_ok=True)
    stamp = datetime.now(timezone.utc).strftime("%Y-%m-%d_%H-%M-%S")
    stem = f"{name}_{algo}_{env.num_agents}_agents_{stamp}"
    csv_path = args.output_dir / f"{stem}.csv"
    heat_path = args.output_dir / f"{stem}_heatmap.npy"
    ev.write_results_csv(csv_path, table)
    np.save(heat_path, heat)
    with (args.output_dir / f"{stem}_summary.json").open("w", encoding="utf-8") as f:
        json.dump(dict(stats, env_config=env_config, num_envs=env.num_envs, episodes_per_env=args.episodes), f, indent=2)
    print(f"Results saved to {csv_path}")
    print(f"Heatmap saved to {heat_path}")
    traced = ev.write_trace_outputs(trace, args.output_dir, stem, video=args.save_video, trajectories=args.save_trajectories,
                                    fps=args.video_fps, hold=args.video_final_hold, cell_px=args.video_cell_px)
    pdf_path = None
    try:
        import matplotlib

        matplotlib.use("Agg")
        import matplotlib.pyplot as plt
    except ImportError:
        plt = None
    if plt is not None:
        fig, ax = plt.subplots()
        ax.set_xlabel("X")
        ax.set_ylabel("Y")
        fig.colorbar(ax.imshow(heat, origin="upper"), label="Number of visits")
        pdf_path = args.output_dir / f"{stem}_heatmap.pdf"
        fig.savefig(pdf_path, bbox_inches="tight")
        plt.close(fig)
        print(f"Heatmap saved to {pdf_path}")
    env.close()
    return {"summary": stats, "csv": csv_path, "heatmap": heat_path, "pdf": pdf_path, "table": table, **traced}


if __name__ == "__main__":
    main()
