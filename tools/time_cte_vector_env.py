"""Wall time per VECTOR step of the single-agent (CTE) env as an RLlib env runner would drive it (not a test):
ReferenceModelSingleAgentVectorEnv (one handle, next-step autoreset) against the same number of drop-in
reference_model_single_agent.ReferenceModel objects stepped one after another (reset when done), on ReferenceModel-2-1.

    python tools/time_cte_vector_env.py [--num-envs 4 32] [--num-agents 16] [--steps 400] [--warmup 50]

Prints one JSON line per (num_envs, implementation): us per vector step (median of 5 repetitions, min beside it)."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def time_adapter(cfg, B, acts, warmup):
    from dl_reference_models_amd.vector_env_single_agent import ReferenceModelSingleAgentVectorEnv

    vec = ReferenceModelSingleAgentVectorEnv(dict(cfg, seed=0), num_envs=B)
    vec.reset()
    for t in range(warmup):
        vec.step(acts[t % len(acts)])
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for a in acts:
            vec.step(a)
        reps.append((time.perf_counter() - t0) / len(acts) * 1e6)
    vec.close()
    return reps


def time_dropins(cfg, B, acts, warmup):
    from dl_reference_models_amd.reference_model_single_agent import ReferenceModel

    objs = [ReferenceModel(dict(cfg, seed=b)) for b in range(B)]
    for o in objs:
        o.reset()

    def vector_step(a):
        for b, o in enumerate(objs):
            _, _, te, tr, _ = o.step(a[b])
            if te or tr:
                o.reset()

    for t in range(warmup):
        vector_step(acts[t % len(acts)])
    reps = []
    for _ in range(5):
        t0 = time.perf_counter()
        for a in acts:
            vector_step(a)
        reps.append((time.perf_counter() - t0) / len(acts) * 1e6)
    for o in objs:
        o.close()
    return reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--num-envs", type=int, nargs="+", default=[4, 32])
    ap.add_argument("--num-agents", type=int, default=16)
    ap.add_argument("--steps-per-episode", type=int, default=100)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    cfg = {"env_name": "ReferenceModel-2-1", "num_agents": args.num_agents, "steps_per_episode": args.steps_per_episode}
    rng = np.random.default_rng(0)
    for B in args.num_envs:
        acts = rng.integers(0, 5, size=(args.steps, B, args.num_agents))
        for impl, fn in (("vector_env", time_adapter), ("dropin_objects", time_dropins)):
            reps = fn(cfg, B, acts, args.warmup)
            print(json.dumps({"impl": impl, "num_envs": B, "num_agents": args.num_agents, "env_name": cfg["env_name"],
                              "steps_per_episode": args.steps_per_episode, "steps": args.steps,
                              "us_per_vector_step": round(statistics.median(reps), 1), "us_min": round(min(reps), 1)}),
                  flush=True)


if __name__ == "__main__":
    main()
