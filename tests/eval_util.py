"""Helpers of the evaluation tests: the recorder kernel (mapf_eval_record, include/mapf_step.h) restated in NumPy on top
of the CPU oracle's per-env handles, the loader of the ``ge_eval_*`` fixtures recorded from the reference
(tools/gen_eval_golden.py), and the comparison of a set of records with another, element by element, exactly.

A set of records ("dense records") is a dict of arrays over [B][E]:
    timesteps int32, terminated / truncated bool, total_reward float64, agent_reward float64 [B][E][N],
    starts / goals int32 [B][E][N][2], info_all float32 [B][E][14], heat int64 [B][H][W]
"""

from __future__ import annotations

import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")

EVAL_FIXTURES = ["ge_eval_2_1_n2", "ge_eval_2_1_n4", "ge_eval_2_1_n4_lifelong", "ge_eval_2_1_n4_deterministic"]
RECORD_KEYS = ("timesteps", "terminated", "truncated", "total_reward", "agent_reward", "starts", "goals", "info_all", "heat")


def load_eval_fixture(name: str) -> dict:
    with np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False) as z:
        d = {k: z[k] for k in z.files}
    d["config"] = json.loads(str(d["config"]))
    d["columns"] = [str(c) for c in d["columns"]]
    d["E"] = int(d["E"])
    return d


def greedy_actions(positions, goals, rng, p_greedy: float) -> np.ndarray:
    """The action stream of oracle/gen_golden.py ('greedy'): with probability p step along the larger goal-delta axis,
    else uniform.  Same order of draws: N uniform actions first, then one uniform float per agent."""
    n = len(positions)
    out = rng.integers(0, 5, size=n)
    pick = rng.random(n) < p_greedy  # (n consecutive draws, the stream of one draw per agent)
    d = np.asarray(goals, np.int64) - np.asarray(positions, np.int64)
    dr, dc = d[:, 0], d[:, 1]
    vert = pick & (np.abs(dr) >= np.abs(dc)) & (dr != 0)
    horz = pick & ~vert & (dc != 0)
    out = np.where(vert, np.where(dr > 0, 3, 1), np.where(horz, np.where(dc > 0, 2, 4), out))
    return out.astype(np.int8)


class HostRecorder:
    """k_eval_record in NumPy: the same buffers, the same rule, one env at a time."""

    def __init__(self, B: int, N: int, H: int, W: int, E: int):
        self.B, self.N, self.H, self.W, self.E = B, N, H, W, E
        self.heat = np.zeros((B, H, W), np.uint32)
        self.ep_i32 = np.zeros((B, E, 2 + 4 * N), np.int32)
        self.ep_f64 = np.zeros((B, E, 1 + N), np.float64)
        self.ep_info = np.zeros((B, E, 14), np.float32)
        self.episodes_recorded = np.zeros(B, np.int32)
        self.active = np.ones(B, np.uint8)
        self.reset_mask = np.zeros(B, np.uint8)
        self.run_reward = np.zeros((B, N), np.float64)
        self.run_steps = np.zeros(B, np.int32)

    def record(self, b: int, positions, starts, goals, rewards, terminated: bool, truncated: bool, info_all) -> None:
        """Books one step of env b (the caller steps only envs with active[b] != 0)."""
        assert self.active[b]
        self.run_reward[b] += np.asarray(rewards, np.float32).astype(np.float64)
        self.run_steps[b] += 1
        pos = np.asarray(positions, np.int64)
        inside = (pos[:, 0] >= 0) & (pos[:, 0] < self.H) & (pos[:, 1] >= 0) & (pos[:, 1] < self.W)
        np.add.at(self.heat[b], (pos[inside, 0], pos[inside, 1]), 1)
        if not (terminated or truncated):
            self.reset_mask[b] = 0
            return
        k = int(self.episodes_recorded[b])
        rec = self.ep_i32[b, k]
        rec[0], rec[1] = self.run_steps[b], (1 if terminated else 0) | (2 if truncated else 0)
        rec[2:] = np.concatenate([np.asarray(starts, np.int32), np.asarray(goals, np.int32)], axis=1).reshape(-1)
        self.ep_f64[b, k, 0] = self.run_reward[b].sum()
        self.ep_f64[b, k, 1:] = self.run_reward[b]
        self.ep_info[b, k] = info_all
        self.run_reward[b] = 0.0
        self.run_steps[b] = 0
        self.episodes_recorded[b] = k + 1
        if k + 1 < self.E:
            self.reset_mask[b] = 1
        else:
            self.active[b] = 0
            self.reset_mask[b] = 0

    def dense(self) -> dict:
        assert (self.episodes_recorded == self.E).all(), self.episodes_recorded
        return dense_from_buffers(self.ep_i32, self.ep_f64, self.ep_info, self.heat, self.N)


def dense_from_buffers(ep_i32, ep_f64, ep_info, heat, N: int) -> dict:
    B, E = ep_i32.shape[:2]
    sg = ep_i32[:, :, 2:].reshape(B, E, N, 4)
    return {
        "timesteps": ep_i32[:, :, 0].astype(np.int32), "terminated": (ep_i32[:, :, 1] & 1) != 0,
        "truncated": (ep_i32[:, :, 1] & 2) != 0, "total_reward": ep_f64[:, :, 0].astype(np.float64),
        "agent_reward": ep_f64[:, :, 1:].astype(np.float64), "starts": sg[..., 0:2].astype(np.int32),
        "goals": sg[..., 2:4].astype(np.int32), "info_all": np.asarray(ep_info, np.float32),
        "heat": np.asarray(heat).astype(np.int64),
    }


def dense_from_results(res: dict, heat_per_env, E: int) -> dict:
    """Evaluator.results() (rows ordered by env, episode) of a finished evaluation as dense records."""
    B = len(res["episodes_recorded"])
    assert (res["episodes_recorded"] == E).all(), res["episodes_recorded"]
    assert np.array_equal(res["env"], np.repeat(np.arange(B), E)) and np.array_equal(res["episode"], np.tile(np.arange(E), B))
    out = {k: np.asarray(res[k]).reshape((B, E) + np.asarray(res[k]).shape[1:])
           for k in ("timesteps", "terminated", "truncated", "total_reward", "agent_reward", "starts", "goals", "info_all")}
    out["heat"] = np.asarray(heat_per_env, np.int64)
    return out


def run_oracle_eval(grids, cfg: dict, E: int, *, rng_words=None, seeds=None, actions=None, greedy=None, action_seed=1000,
                    fixed_starts=None, fixed_goals=None) -> dict:
    """The evaluation loop on the CPU oracle: every env reset(), then step until done, E times, each env through its own
    handle (an env that has finished is simply not called any more); the bookkeeping by HostRecorder.

    actions [T][B][N]: env b takes actions[t, b] at the t-th launch (it is active from launch 0 until it finishes);
    else greedy = p: greedy_actions from default_rng(action_seed + b) per env, and the actions taken are returned.
    Returns the dense records plus ``actions`` [T][B][N], ``launches`` (T) and ``state``: per env positions, goals,
    starts, reached, completed_once, step_count and generator words as they are when the run ends, i.e. for every env
    right after its E-th episode."""
    import oracle as orc

    grids = np.ascontiguousarray(grids, np.uint8)
    batch = orc.OracleBatch(grids, cfg, seeds=seeds, rng_words=rng_words, ctor_draw=True)
    if cfg.get("deterministic", False):
        for b, e in enumerate(batch.envs):
            e.set_fixed_starts_goals(fixed_starts[b], fixed_goals[b])
    B, N = batch.B, batch.N
    H, W = grids.shape[1:]
    rec = HostRecorder(B, N, H, W, E)
    for e in batch.envs:
        rc, _ = e.reset()
        assert rc == 0, rc
    rngs = None if actions is not None else [np.random.default_rng(action_seed + b) for b in range(B)]
    T_max = E * int(cfg.get("steps_per_episode", 100))
    taken = np.zeros((T_max, B, N), np.int8)
    t = 0
    while rec.active.any():
        assert t < T_max
        for b, e in enumerate(batch.envs):
            if not rec.active[b]:
                continue
            act = actions[t, b] if actions is not None else greedy_actions(e.positions, e.goals, rngs[b], greedy)
            taken[t, b] = act
            rc, _obs, rew, term, trunc, info_all, _ia = e.step(act)
            assert rc == 0, (rc, b, t)
            rec.record(b, e.positions, e.starts, e.goals, rew, term, trunc, info_all)
            if rec.reset_mask[b]:
                rc, _ = e.reset()
                assert rc == 0, rc
        t += 1
    out = rec.dense()
    out["actions"] = taken[:t]
    out["launches"] = t
    out["state"] = batch.state()
    return out


def assert_records_equal(got: dict, want: dict, what: str = "") -> None:
    for k in RECORD_KEYS:
        g, w = np.asarray(got[k]), np.asarray(want[k])
        assert g.shape == w.shape, (what, k, g.shape, w.shape)
        if not np.array_equal(g, w):
            bad = np.argwhere(g != w)
            raise AssertionError(f"{what} {k}: {len(bad)} elements differ, first at {bad[0].tolist()}: "
                                 f"got {g[tuple(bad[0])]} want {w[tuple(bad[0])]}")


def results_from_dense(d: dict, seeds) -> dict:
    """Dense records in the form of Evaluator.results() (what results_table takes)."""
    B, E = d["timesteps"].shape
    flat = {k: np.asarray(d[k]).reshape((B * E,) + np.asarray(d[k]).shape[2:])
            for k in ("timesteps", "terminated", "truncated", "total_reward", "agent_reward", "starts", "goals", "info_all")}
    flat["env"] = np.repeat(np.arange(B), E).astype(np.int32)
    flat["episode"] = np.tile(np.arange(E), B).astype(np.int32)
    flat["episodes_recorded"] = np.full(B, E, np.int32)
    flat["seeds"] = [int(s) for s in seeds]
    return flat


def engine_config(fx: dict, device="cuda:0") -> dict:
    """env_config of a VecReferenceModel that runs a fixture's envs."""
    cfg = dict(fx["config"])
    cfg.pop("seed", None)
    cfg.update(grid=np.asarray(fx["grids"], np.uint8), num_envs=int(fx["grids"].shape[0]), device=device,
               seeds=[int(s) for s in fx["seeds"]])
    if cfg.get("deterministic", False):
        cfg.update(fixed_starts=np.asarray(fx["ctor_starts"], np.int16), fixed_goals=np.asarray(fx["ctor_goals"], np.int16))
    return cfg
