"""Record the single-agent evaluation fixtures tests/golden/ge_cte_eval_*.npz from the UNMODIFIED reference env.  TEST
INFRASTRUCTURE.

Runs only where the reference tree lies (oracle/ref_harness.py imports it from there).  The reference's test mode has no
single-agent branch (main.py:37), so the loop recorded here is main.py's own (main.py:172-324) restated for a gym.Env: per
seed one reference env runs E times reset(), then step() until ``terminated or truncated``, ``episode_reward += reward``,
one visit on the cell of every agent after every step, one record per episode -- total reward, steps, how the episode
ended, starts and goals as env.starts / env.goals hold them after the last step, the terminal info -- and the visit count
per env.  Actions: ``eval_util.greedy_actions`` (with probability p a step along the larger goal-delta axis, else uniform)
from default_rng(1000 + seed); the actions taken are stored [T_max][B][N] (env b's t-th step overall is actions[t, b]) and
replayed by the tests, so nothing depends on the policy.  Data only.

    python tools/gen_cte_eval_golden.py            writes the three fixtures
    python tools/gen_cte_eval_golden.py --check    regenerates and compares every array with the committed files
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

import gen_golden as gg  # noqa: E402  (pcg_words)
import ref_harness as rh  # noqa: E402
from cte_eval_util import CTE_EVAL_FIXTURES  # noqa: E402
from eval_util import greedy_actions  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
INFO_KEYS = ("blocking_count_step", "goals_reached_step", "goals_reached_total", "blocking_count_total")


def record_eval(cfg: dict, seeds, E: int, p_greedy: float) -> dict:
    B, N = len(seeds), int(cfg["num_agents"])
    T_max = E * int(cfg["steps_per_episode"])
    agents = [f"agent_{i}" for i in range(N)]
    out = None
    columns = None
    for b, seed in enumerate(seeds):
        env = rh.make_reference_single_agent_env(dict(cfg, seed=int(seed)))
        H, W = env.grid.shape
        if out is None:
            out = {
                "config": np.array(json.dumps(cfg)), "E": np.int32(E), "p_greedy": np.float64(p_greedy),
                "seeds": np.asarray(seeds, np.int64), "grids": np.zeros((B, H, W), np.uint8),
                "rng_words": np.zeros((B, 6), np.uint64), "ctor_starts": np.zeros((B, N, 2), np.int16),
                "ctor_goals": np.zeros((B, N, 2), np.int16), "actions": np.zeros((T_max, B, N), np.int8),
                "timesteps": np.zeros((B, E), np.int32), "terminated": np.zeros((B, E), np.bool_),
                "truncated": np.zeros((B, E), np.bool_), "total_reward": np.zeros((B, E), np.float64),
                "starts": np.zeros((B, E, N, 2), np.int32), "goals": np.zeros((B, E, N, 2), np.int32),
                "info": np.zeros((B, E, 4), np.float32), "heat": np.zeros((B, H, W), np.int64),
                "env_steps": np.zeros(B, np.int32),
            }
        out["grids"][b] = env.grid
        out["rng_words"][b] = gg.pcg_words(np.random.default_rng(int(seed)).bit_generator.state)
        out["ctor_starts"][b] = [np.asarray(env.starts[a]) for a in agents]
        out["ctor_goals"][b] = [np.asarray(env.goals[a]) for a in agents]
        rng = np.random.default_rng(1000 + int(seed))
        t = 0
        for ep in range(E):
            env.reset()
            done, steps, episode_reward = False, 0, 0
            terminated = truncated = False
            info = {}
            while not done:
                steps += 1
                act = greedy_actions([env.positions[a] for a in agents], [env.goals[a] for a in agents], rng, p_greedy)
                out["actions"][t, b] = act
                t += 1
                _obs, reward, terminated, truncated, info = env.step(act)
                done = terminated or truncated
                episode_reward += reward
                for a in agents:
                    y, x = env.positions[a]
                    out["heat"][b, y, x] += 1
            row = {"episode": ep + 1, "seed": env.seed, "total_reward": episode_reward, "timesteps": steps,
                   "goals_reached_total": info["goals_reached_total"], "blocking_count_total": info["blocking_count_total"]}
            for i, a in enumerate(agents):
                s, g = np.asarray(env.starts[a]).tolist(), np.asarray(env.goals[a]).tolist()
                row[f"agent_{i}_start_x"], row[f"agent_{i}_start_y"] = s[0], s[1]
                row[f"agent_{i}_goal_x"], row[f"agent_{i}_goal_y"] = g[0], g[1]
                out["starts"][b, ep, i], out["goals"][b, ep, i] = s, g
            out["timesteps"][b, ep], out["total_reward"][b, ep] = steps, episode_reward
            out["terminated"][b, ep], out["truncated"][b, ep] = bool(terminated), bool(truncated)
            out["info"][b, ep] = [info[k] for k in INFO_KEYS]
            columns = list(row.keys()) + ["env"]
        out["env_steps"][b] = t
    out["columns"] = np.array(columns)
    out["actions"] = out["actions"][: int(out["env_steps"].max())]
    return out


def check_conditions(fx: dict) -> None:
    """What the fixtures must exercise (asserted here, on the CPU, so that the tests can rely on it)."""
    success = sum(int((d["terminated"] & ~d["truncated"]).sum()) for d in fx.values())
    truncations = sum(int(d["truncated"].sum()) for d in fx.values())
    assert success >= 1 and truncations >= 1, "the fixtures must hold a success and a truncation"
    overlap = early = fractional = False
    for d in fx.values():
        ends = np.cumsum(d["timesteps"], axis=1)  # launch index after which episode k of env b is over
        # a later episode of one env starts while another env still runs an earlier one
        for k in range(1, ends.shape[1]):
            overlap |= bool((ends[:, k - 1][:, None] < ends[:, k - 1][None, :]).any())
        early |= bool((d["env_steps"] < d["env_steps"].max()).any())
        r = d["total_reward"]
        fractional |= bool(np.any(np.abs(r * 2 - np.round(r * 2)) > 1e-9))
    assert overlap, "no env starts a later episode while another still runs an earlier one"
    assert early, "no env finishes all its episodes strictly before the slowest"
    assert fractional, "no episode's total reward carries a blocking or move-after-goal penalty"


def fixtures() -> dict:
    base = {"env_name": "ReferenceModel-2-1", "steps_per_episode": 40, "render_env": False}
    fx = {
        CTE_EVAL_FIXTURES[0]: record_eval(dict(base, num_agents=2, steps_per_episode=100), list(range(6)), 3, 0.9),
        CTE_EVAL_FIXTURES[1]: record_eval(dict(base, num_agents=4), list(range(4)), 3, 0.8),
        CTE_EVAL_FIXTURES[2]: record_eval(dict(base, num_agents=4, deterministic=True), list(range(4)), 3, 0.8),
    }
    check_conditions(fx)
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
