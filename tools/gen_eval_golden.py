"""Record the evaluation fixtures tests/golden/ge_eval_*.npz from the UNMODIFIED reference env.  TEST INFRASTRUCTURE.

Runs only where the reference tree lies (oracle/ref_harness.py imports it from there).  Per seed one reference env runs
the loop of the reference's test mode (main.py test_trained_model) restated: E times reset(), then step() until
``__all__`` is done, keeping per episode what main.py:232-324 keeps -- total reward, per-agent reward, steps, how the episode
ended, starts and goals as env.starts / env.goals hold them after the last step, the terminal info["__all__"] -- and the
visit count of main.py:262-267 per env.  Actions: with probability p a step along the larger goal-delta axis, else
uniform, from default_rng(1000 + seed); the actions taken are stored [T_max][B][N] (env b's t-th step overall is
actions[t, b]) and replayed by the tests, so nothing depends on the policy.  Data only.

    python tools/gen_eval_golden.py            writes the four fixtures
    python tools/gen_eval_golden.py --check    regenerates and compares every array with the committed files
"""

from __future__ import annotations

import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import gen_golden as gg  # noqa: E402  (info_all_vector, pcg_words: the helpers of the other fixtures)
import ref_harness as rh  # noqa: E402
from eval_util import EVAL_FIXTURES, greedy_actions  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def record_eval(cfg: dict, seeds, E: int, p_greedy: float) -> dict:
    B, N = len(seeds), int(cfg["num_agents"])
    lifelong = bool(cfg.get("lifelong_mapf", False))
    T_max = E * int(cfg["steps_per_episode"])
    out = None
    columns = None
    for b, seed in enumerate(seeds):
        env = rh.make_reference_env(dict(cfg, seed=int(seed)))
        agents = [f"agent_{i}" for i in range(N)]
        H, W = env.grid.shape
        if out is None:
            out = {
                "config": np.array(json.dumps(cfg)), "E": np.int32(E), "p_greedy": np.float64(p_greedy),
                "seeds": np.asarray(seeds, np.int64), "grids": np.zeros((B, H, W), np.uint8),
                "rng_words": np.zeros((B, 6), np.uint64), "ctor_starts": np.zeros((B, N, 2), np.int16),
                "ctor_goals": np.zeros((B, N, 2), np.int16), "actions": np.zeros((T_max, B, N), np.int8),
                "timesteps": np.zeros((B, E), np.int32), "terminated": np.zeros((B, E), np.bool_),
                "truncated": np.zeros((B, E), np.bool_), "total_reward": np.zeros((B, E), np.float64),
                "agent_reward": np.zeros((B, E, N), np.float64), "starts": np.zeros((B, E, N, 2), np.int32),
                "goals": np.zeros((B, E, N, 2), np.int32), "info_all": np.zeros((B, E, 14), np.float32),
                "heat": np.zeros((B, H, W), np.int64), "env_steps": np.zeros(B, np.int32),
            }
            if lifelong:
                for k in ("goals_reached_total", "throughput", "completion_ratio"):
                    out[k] = np.zeros((B, E), np.float64)
        out["grids"][b] = env.grid
        out["rng_words"][b] = gg.pcg_words(np.random.default_rng(int(seed)).bit_generator.state)
        out["ctor_starts"][b], out["ctor_goals"][b] = env._starts_arr, env._goals_arr
        rng = np.random.default_rng(1000 + int(seed))
        t = 0
        for ep in range(E):
            obs, _infos = env.reset()
            done, steps, episode_reward = False, 0, 0
            agent_rewards = dict.fromkeys(obs, 0.0)
            term_all = trunc_all = False
            last_info = {}
            while not done:
                steps += 1
                act = greedy_actions(env._positions_arr, env._goals_arr, rng, p_greedy)
                out["actions"][t, b] = act
                t += 1
                obs, rewards, terminateds, truncateds, infos = env.step({a: int(act[i]) for i, a in enumerate(agents)})
                term_all, trunc_all = bool(terminateds.get("__all__", False)), bool(truncateds.get("__all__", False))
                last_info = infos.get("__all__", {})
                done = term_all or trunc_all
                episode_reward += sum(rewards.values())
                for a in obs:
                    agent_rewards[a] += rewards[a]
                    y, x = env.positions[a]
                    if 0 <= y < H and 0 <= x < W:
                        out["heat"][b, y, x] += 1
            row = {"episode": ep + 1, "seed": env.seed, "total_reward": episode_reward, "timesteps": steps}
            if lifelong:
                grt = float(last_info.get("goals_reached_total", 0.0))
                row["goals_reached_total"] = grt
                row["throughput"] = float(last_info.get("throughput", grt / float(max(steps, 1))))
                row["completion_ratio"] = float(last_info.get("completion_ratio", 0.0))
                for k in ("goals_reached_total", "throughput", "completion_ratio"):
                    out[k][b, ep] = row[k]
            for i, a in enumerate(agents):  # (main.py:310 asks env.get_agent_ids(), which the env does not have: its agents in order)
                idx = a.split("_")[1]
                s, g = np.asarray(env.starts[a]).tolist(), np.asarray(env.goals[a]).tolist()
                row[f"agent_{idx}_reward"] = agent_rewards[a]
                row[f"agent_{idx}_start_x"], row[f"agent_{idx}_start_y"] = s[0], s[1]
                row[f"agent_{idx}_goal_x"], row[f"agent_{idx}_goal_y"] = g[0], g[1]
                out["agent_reward"][b, ep, i] = agent_rewards[a]
                out["starts"][b, ep, i], out["goals"][b, ep, i] = s, g
            out["timesteps"][b, ep], out["total_reward"][b, ep] = steps, episode_reward
            out["terminated"][b, ep], out["truncated"][b, ep] = term_all, trunc_all
            out["info_all"][b, ep] = gg.info_all_vector(env, last_info)
            columns = list(row.keys()) + ["env"]
        out["env_steps"][b] = t
    out["columns"] = np.array(columns)
    out["actions"] = out["actions"][: int(out["env_steps"].max())]
    return out


def fixtures() -> dict:
    base = {"env_name": "ReferenceModel-2-1", "sensor_range": 2, "steps_per_episode": 100, "training_execution_mode": "CTDE",
            "render_env": False}
    seeds = list(range(6))
    fx = {
        EVAL_FIXTURES[0]: record_eval(dict(base, num_agents=2), seeds, 4, 0.9),
        # the reference's parity configuration (tests/test_reference_model_multi_agent_parity.py)
        EVAL_FIXTURES[1]: record_eval(dict(base, num_agents=4, include_action_mask_in_obs=True,
                                           include_blocking_pressure_in_obs=False), seeds[:4], 4, 0.8),
        EVAL_FIXTURES[2]: record_eval(dict(base, num_agents=4, steps_per_episode=40, lifelong_mapf=True), seeds[:4], 4, 0.8),
        EVAL_FIXTURES[3]: record_eval(dict(base, num_agents=4, steps_per_episode=40, deterministic=True), seeds[:4], 4, 0.8),
    }
    first = fx[EVAL_FIXTURES[0]]
    ok = first["terminated"] & ~first["truncated"]
    assert ok.any() and first["truncated"].any(), "the first fixture must hold a success and a truncation"
    return fx


def main() -> int:
    check = "--check" in sys.argv
    bad = 0
    for name, data in fixtures().items():
        path = os.path.join(GOLDEN, name + ".npz")
        succ = int((data["terminated"] & ~data["truncated"]).sum())
        print(f"  {name}: {data['timesteps'].size} episodes, {succ} successes, {int(data['truncated'].sum())} truncations, "
              f"steps per env {data['env_steps'].tolist()}")
        if check:
            with np.load(path, allow_pickle=False) as z:
                for k, v in data.items():
                    if k not in z.files or z[k].dtype != v.dtype or z[k].shape != v.shape or not np.array_equal(z[k], v):
                        print(f"MISMATCH {name}: {k}")
                        bad += 1
        else:
            np.savez_compressed(path, **data)
            print(f"    {os.path.getsize(path) / 1024:.1f} KiB")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
