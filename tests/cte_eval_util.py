"""Helpers of the single-agent (CTE) evaluation tests: the evaluation loop of the reference's test mode restated for a
gym.Env in plain Python on top of the CPU oracle's single-agent env (the one tests/test_oracle_single_agent.py pins), the
loader of the ``ge_cte_eval_*`` fixtures recorded from the reference (tools/gen_cte_eval_golden.py), and the exact
comparison of two sets of records.

A set of records ("dense records") is a dict of arrays over [B][E]:
    timesteps int32, terminated / truncated bool, total_reward float64, starts / goals int32 [B][E][N][2],
    info float32 [B][E][4], heat int64 [B][H][W]
"""

from __future__ import annotations

import json
import os

import numpy as np

from eval_util import greedy_actions

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

CTE_EVAL_FIXTURES = ["ge_cte_eval_2_1_n2", "ge_cte_eval_2_1_n4", "ge_cte_eval_2_1_n4_deterministic"]
RECORD_KEYS = ("timesteps", "terminated", "truncated", "total_reward", "starts", "goals", "info", "heat")


def load_fixture(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config"]))
    d["columns"] = [str(c) for c in d["columns"]]
    d["E"] = int(d["E"])
    return d


def run_oracle_eval(grids, cfg: dict, E: int, *, rng_words, actions=None, greedy=None, action_seeds=None, fixed_starts=None,
                    fixed_goals=None) -> dict:
    """main.py's test loop for a gym.Env, per env and in plain Python, on the CPU oracle's single-agent env:

        for episode in range(E):  reset();  while not (terminated or truncated):  step();  episode_reward += reward

    with one visit per agent cell after every step and one record per episode.  actions [T][B][N]: env b's t-th step
    overall takes actions[t, b]; else greedy = p: ``greedy_actions`` from default_rng(action_seeds[b]).  Returns the dense
    records plus ``actions`` [T][B][N], ``env_steps`` [B] and ``state`` (positions, goals, starts and generator words of
    every env right after its E-th episode)."""
    import oracle as orc

    grids = np.ascontiguousarray(grids, np.uint8)
    B, (H, W), N = grids.shape[0], grids.shape[1:], int(cfg["num_agents"])
    T_max = E * int(cfg.get("steps_per_episode", 100))
    out = {"timesteps": np.zeros((B, E), np.int32), "terminated": np.zeros((B, E), np.bool_),
           "truncated": np.zeros((B, E), np.bool_), "total_reward": np.zeros((B, E), np.float64),
           "starts": np.zeros((B, E, N, 2), np.int32), "goals": np.zeros((B, E, N, 2), np.int32),
           "info": np.zeros((B, E, 4), np.float32), "heat": np.zeros((B, H, W), np.int64),
           "env_steps": np.zeros(B, np.int32)}
    taken = np.zeros((T_max, B, N), np.int8)
    state = {"positions": np.zeros((B, N, 2), np.int32), "goals": np.zeros((B, N, 2), np.int32),
             "starts": np.zeros((B, N, 2), np.int32), "rng_words": np.zeros((B, 6), np.uint64)}
    for b in range(B):
        kw = {}
        if cfg.get("deterministic", False):
            kw = dict(fixed_starts=fixed_starts[b], fixed_goals=fixed_goals[b])
        env = orc.OracleCteEnv(grids[b], cfg, rng_words=rng_words[b], **kw)
        rng = None if actions is not None else np.random.default_rng(int(action_seeds[b]))
        t = 0
        for ep in range(E):
            env.reset()
            done, steps, episode_reward = False, 0, 0
            while not done:
                act = actions[t, b] if actions is not None else greedy_actions(env.positions, env.goals, rng, greedy)
                taken[t, b] = act
                t += 1
                rc, _obs, reward, terminated, truncated, info = env.step(act)
                assert rc == 0, (rc, b, t)
                steps += 1
                episode_reward += reward
                for y, x in env.positions:
                    out["heat"][b, y, x] += 1
                done = terminated or truncated
            out["timesteps"][b, ep], out["total_reward"][b, ep] = steps, episode_reward
            out["terminated"][b, ep], out["truncated"][b, ep] = terminated, truncated
            out["starts"][b, ep], out["goals"][b, ep], out["info"][b, ep] = env.starts, env.goals, info
        out["env_steps"][b] = t
        state["positions"][b], state["goals"][b], state["starts"][b] = env.positions, env.goals, env.starts
        state["rng_words"][b] = env.rng_words()
    out["actions"] = taken[: int(out["env_steps"].max())]
    out["state"] = state
    return out


def dense_from_results(res: dict, heat_per_env, E: int) -> dict:
    """JointEvaluator.results() (rows ordered by env, episode) of a finished evaluation as dense records."""
    B = len(res["episodes_recorded"])
    assert (res["episodes_recorded"] == E).all(), res["episodes_recorded"]
    assert np.array_equal(res["env"], np.repeat(np.arange(B), E)) and np.array_equal(res["episode"], np.tile(np.arange(E), B))
    out = {k: np.asarray(res[k]).reshape((B, E) + np.asarray(res[k]).shape[1:])
           for k in ("timesteps", "terminated", "truncated", "total_reward", "starts", "goals", "info")}
    out["heat"] = np.asarray(heat_per_env, np.int64)
    return out


def results_from_dense(d: dict, seeds) -> dict:
    """Dense records in the form of JointEvaluator.results() (what results_table takes)."""
    B, E = d["timesteps"].shape
    flat = {k: np.asarray(d[k]).reshape((B * E,) + np.asarray(d[k]).shape[2:])
            for k in ("timesteps", "terminated", "truncated", "total_reward", "starts", "goals", "info")}
    flat["env"] = np.repeat(np.arange(B), E).astype(np.int32)
    flat["episode"] = np.tile(np.arange(E), B).astype(np.int32)
    flat["episodes_recorded"] = np.full(B, E, np.int32)
    flat["seeds"] = [int(s) for s in seeds]
    return flat


def assert_records_equal(got: dict, want: dict, what: str = "") -> None:
    """Every element equal; total_reward compared as bit patterns."""
    for k in RECORD_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        if k == "total_reward":
            g, w = g.view(np.uint64), w.view(np.uint64)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what} {k}: {len(bad)} elements differ, first at {bad[0].tolist()}: "
                                 f"got {np.asarray(got[k])[tuple(bad[0])]!r} want {np.asarray(want[k])[tuple(bad[0])]!r}")


def engine_config(fx: dict, device="cuda:0", **extra) -> dict:
    """env_config of a VecSingleAgentReferenceModel that runs a fixture's envs."""
    cfg = dict(fx["config"])
    cfg.pop("seed", None)
    cfg.update(grid=np.asarray(fx["grids"], np.uint8), num_envs=int(fx["grids"].shape[0]), device=device,
               seeds=[int(s) for s in fx["seeds"]])
    if cfg.get("deterministic", False):
        cfg.update(fixed_starts=np.asarray(fx["ctor_starts"], np.int16), fixed_goals=np.asarray(fx["ctor_goals"], np.int16))
    cfg.update(extra)
    return cfg


def first_flags(timesteps, T: int) -> np.ndarray:
    """uint8 [T][B]: the launches after which an env starts a new episode -- E - 1 per env, at its episode boundaries."""
    ends = np.cumsum(timesteps, axis=1)[:, :-1] - 1
    want = np.zeros((T, timesteps.shape[0]), np.uint8)
    for b in range(ends.shape[0]):
        want[ends[b], b] = 1
    return want
