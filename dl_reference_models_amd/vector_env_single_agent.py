"""Vector-env adapter of the single-agent (CTE) sibling env: the envs of one RLlib env runner served by ONE batched handle.

In CTE mode the reference trains the single-agent env (``main.py:70-73``) on RLlib's new API stack with
``num_envs_per_env_runner=4`` (``src/agents/ppo.py:24-44``).  Its single-agent env runner drives a gymnasium
``VectorEnv`` with NEXT-STEP autoreset: a row that finished is reset by the following ``step`` call, which returns its
reset observation, reward 0.0 and ``False`` flags for it and ignores the action sent for it.  With one drop-in
``reference_model_single_agent.ReferenceModel`` per env that costs a launch, five device->host copies and a full
``get_state`` per env per step.  Here the runner's envs are rows of one ``VecSingleAgentReferenceModel``:

    vec = ReferenceModelSingleAgentVectorEnv(dict(env_config, num_envs=4))
    vec.reset()          -> (obs float32 [B, H*W + 5N], infos)
    vec.step(actions)    -> (obs, rewards float64 [B], terminations bool [B], truncations bool [B], infos)
    vec.envs[b]          -> ``SingleAgentRow``: what ``ReferenceModelCallbacks`` read from a sub-env at episode end
                            (``_episode_blocking_count``, ``goal_reached_once``, ``step_count``; callbacks.py:236-345)

``infos`` is a gymnasium vector info dict: every key of SA-env's info (:355-361) maps to a ``[B]`` array (``[B, 5N]`` for
``action_mask``) and ``"_<key>"`` to the boolean mask of the rows that carry it; rows that restart carry
``action_mask`` only.  ``gymnasium`` and ``ray`` are not installed where this was written and tested, so the class is
duck-typed against their documented interfaces (spaces come from ``spaces.py``); nobody has handed it to a live runner
yet (INTEGRATION.md says so).

Cost model per vector step: one launch (``mapf_cte_step``; two on a step in which some rows restart:
``mapf_cte_step_masked`` of the others, then the masked ``mapf_cte_reset``), one host->device copy (actions and masks in
one pinned buffer), one stream sync and two device->host copies into pinned mirrors: the observations, and the blob of
reward, flags and info.  Row state (positions, counters ...) comes from one batched ``get_state``, fetched lazily, at most
once per vector step and only if somebody reads it.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .engine_handle import RENDER_CELL_PX, _raw_stream
from .host_mirror import VectorAdapter
from .reference_model_multi_agent import render_mode_frame
from .spaces import Box, MultiBinary, MultiDiscrete
from .vec_env_single_agent import INFO_KEYS, VecSingleAgentReferenceModel


class SingleAgentRow:
    """Row ``b`` of a ``ReferenceModelSingleAgentVectorEnv`` with the attribute surface of the drop-in object that callers
    read (``callbacks.py:21-67`` resolve the sub-env, ``:236-345`` read it at episode end).  After a row's episode ends the
    views show its terminal state until the ``step`` call that resets it."""

    def __init__(self, vec: "ReferenceModelSingleAgentVectorEnv", b: int):
        self._vec, self._b = vec, b
        e = vec._engine
        self.num_agents = vec.num_agents
        self.steps_per_episode = vec.steps_per_episode
        self.deterministic = vec.deterministic
        self.grid = e.grids[b if e.grids.shape[0] > 1 else 0]
        self.observation_space, self.action_space = vec.single_observation_space, vec.single_action_space
        self._grid_obs_space, self._action_mask_space = vec._grid_obs_space, vec._action_mask_space
        self._obs_slices = vec._obs_slices
        self._ids = [f"agent_{i}" for i in range(self.num_agents)]
        self._agent_ids = set(self._ids)

    def _s(self):
        return self._vec._state()

    def _dict(self, key):
        a = self._s()[key][self._b]
        return {aid: a[i].astype(np.int64) for i, aid in enumerate(self._ids)}

    positions = property(lambda self: self._dict("positions"))
    goals = property(lambda self: self._dict("goals"))
    starts = property(lambda self: self._dict("starts"))
    step_count = property(lambda self: int(self._s()["counters"][self._b, L.CTR_STEP_COUNT]))
    _episode_blocking_count = property(lambda self: float(self._s()["counters"][self._b, L.CTR_BLOCKING_COUNT]))

    @property
    def goal_reached_once(self):
        r = self._s()["reached"][self._b]
        return {aid: bool(r[i]) for i, aid in enumerate(self._ids)}

    @property
    def unwrapped(self):
        return self

    def split_flat_observation(self, flat_obs: np.ndarray):
        grid = flat_obs[self._obs_slices["grid"]].reshape(self._grid_obs_space.shape)
        return {"observations": grid, "action_mask": flat_obs[self._obs_slices["action_mask"]]}

    def render(self, mode="human"):
        """``"rgb_array"``: this row's frame (a new uint8 [H*32, W*32, 3] array, no sensor windows); ``"human"``: None."""
        return render_mode_frame(self, mode, lambda: self._vec._engine.render([self._b], RENDER_CELL_PX)[0])


class ReferenceModelSingleAgentVectorEnv(VectorAdapter):
    """gymnasium ``VectorEnv`` surface (next-step autoreset) over ONE single-agent engine handle: see the module docstring.

    ``env_config`` takes the drop-in's keys (``env_name`` / ``grid``, ``num_agents``, ``steps_per_episode``,
    ``deterministic``, ``blocking_penalty``, ``move_after_goal_penalty``, ``seed`` -> row b is seeded ``seed + b``, or
    ``seeds``) and the extension keys of ``VecSingleAgentReferenceModel`` (``device``, ``rng_words``, ``fixed_starts`` /
    ``fixed_goals``), plus ``num_envs`` (argument or key)."""

    metadata = {"autoreset_mode": "NextStep"}  # (the value of gymnasium.vector.AutoresetMode.NEXT_STEP)

    def __init__(self, env_config: dict, num_envs: int | None = None):
        cfg = dict(env_config)
        if num_envs is not None:
            cfg["num_envs"] = int(num_envs)
        super().__init__(cfg, cfg.get("num_envs", 1))
        B = self.num_envs
        self._attach(VecSingleAgentReferenceModel(cfg))
        e, m = self._engine, self._mirror
        self.num_agents = N = e.num_agents
        self.steps_per_episode = e.steps_per_episode
        self.deterministic = e.deterministic
        # spaces: the drop-in object's per env (reference_model_single_agent.ReferenceModel), batched along a leading B axis
        H, W = e.grid_shape
        hw, Lo = H * W, e.obs_len
        self._grid_obs_space = Box(low=0, high=2 * N + 1, shape=(H, W), dtype=np.uint8)
        self._action_mask_space = MultiBinary(5 * N)
        self._obs_slices = {"grid": slice(0, hw), "action_mask": slice(hw, hw + 5 * N)}
        low = np.zeros(Lo, dtype=np.float32)
        high = np.concatenate([np.full(hw, 2 * N + 1, dtype=np.float32), np.ones(5 * N, np.float32)])
        self.single_observation_space = Box(low=low, high=high, dtype=np.float32)
        self.single_action_space = MultiDiscrete([5] * N)
        self.observation_space = Box(low=np.tile(low, (B, 1)), high=np.tile(high, (B, 1)), dtype=np.float32)
        self.action_space = MultiDiscrete(np.full((B, N), 5, dtype=np.int64))
        # host -> device: actions [B][N] | step mask [B] | reset mask [B], one pinned buffer and one copy
        nin = B * N + 2 * B
        self._h_in = torch.zeros((nin,), dtype=torch.uint8).pin_memory()
        self._d_in = torch.zeros((nin,), dtype=torch.uint8, device=self.device)
        hin = self._h_in.numpy()
        self._h_acts = hin[:B * N].view(np.int8).reshape(B, N)
        self._h_step_mask, self._h_reset_mask = hin[B * N:B * N + B], hin[B * N + B:]
        dp = self._d_in.data_ptr()
        self._p_acts, self._p_step_mask, self._p_reset_mask = C.c_void_p(dp), C.c_void_p(dp + B * N), C.c_void_p(dp + B * N + B)
        self._v_rew, self._v_info = m.view(e._reward, np.float64), m.view(e._info, np.float32)
        self._v_term, self._v_trunc = m.view(e._terminated, np.uint8), m.view(e._truncated, np.uint8)
        self._p_out = tuple(C.c_void_p(t.data_ptr()) for t in (e._obs, e._reward, e._terminated, e._truncated, e._info))
        self._dev_index = int(self.device.index)
        self._needs_reset = np.zeros(B, dtype=bool)
        self.envs = [SingleAgentRow(self, b) for b in range(B)]

    # ------------------------------------------------------------------------------------------------------
    def episode_metrics(self, reset: bool = False) -> dict:
        """The callbacks' per-episode means over every episode the rows finished (VecSingleAgentReferenceModel)."""
        return self._engine.episode_metrics(reset)

    def poll_error(self):
        self._engine.poll_error()

    def close(self, **kwargs):
        self._engine.close()

    def _mask_info(self, obs):
        return obs[:, self._obs_slices["action_mask"]].astype(self._action_mask_space.dtype)

    # ---- gymnasium VectorEnv ------------------------------------------------------------------------------
    def reset(self, *, seed=None, options=None):
        """Resets every row (one launch).  ``seed`` and ``options`` are ignored, as by the reference env (SA-env:222)."""
        e = self._engine
        rc = e._lib.mapf_cte_reset(e._h, None, self._p_out[0], C.c_void_p(_raw_stream(self._dev_index)))
        if rc != L.MAPF_OK:
            e._check(rc)
        self._needs_reset[:] = False
        self._state_cache = None
        obs = self._mirror.fetch(want_small=False)
        return obs, {"action_mask": self._mask_info(obs), "_action_mask": np.ones(self.num_envs, dtype=bool)}

    def step(self, actions):
        """actions: int [B, N], the reference's MultiDiscrete([5]*N) action per row."""
        B, N, e = self.num_envs, self.num_agents, self._engine
        a = np.asarray(actions)
        if a.shape != (B, N):
            raise ValueError(f"actions must have shape {(B, N)}")
        restart = self._needs_reset
        stepped = ~restart
        n_restart = int(restart.sum())
        bad = bool(((a < 0) | (a > 4))[stepped].any())
        # an out-of-range action becomes 5: the kernel stops that env's agent loop there, like the reference (SA-env:401-403)
        np.copyto(self._h_acts, np.where((a < 0) | (a > 4), 5, a), casting="unsafe")
        if n_restart:
            self._h_step_mask[:] = stepped
            self._h_reset_mask[:] = restart
        self._d_in.copy_(self._h_in, non_blocking=True)
        stream = _raw_stream(self._dev_index)
        po = self._p_out
        lib, h = e._lib, e._h
        if n_restart == 0:
            rc = lib.mapf_cte_step(h, self._p_acts, po[0], po[1], po[2], po[3], po[4], None, 0, stream)
        elif n_restart < B:
            rc = lib.mapf_cte_step_masked(h, self._p_acts, self._p_step_mask, po[0], po[1], po[2], po[3], po[4], None, 0,
                                          stream)
        else:
            rc = L.MAPF_OK
        if rc == L.MAPF_OK and n_restart:
            rc = lib.mapf_cte_reset(h, self._p_reset_mask, po[0], C.c_void_p(stream))
        if rc != L.MAPF_OK:
            e._check(rc)
        self._state_cache = None
        obs = self._mirror.fetch(want_small=True)
        if bad:
            try:
                e.poll_error()
            except ValueError:
                pass
            raise ValueError("Invalid action")
        rew = np.where(stepped, self._v_rew, 0.0)
        term = self._v_term.astype(bool) & stepped
        trunc = self._v_trunc.astype(bool) & stepped
        info = self._v_info
        infos = {"action_mask": self._mask_info(obs), "_action_mask": np.ones(B, dtype=bool)}
        if n_restart < B:  # (a key appears when some row carries it)
            for k, key in enumerate(INFO_KEYS):
                infos[key] = np.where(stepped, info[:, k].astype(np.float64), 0.0)
                infos["_" + key] = stepped.copy()
        self._needs_reset = term | trunc
        return obs, rew, term, trunc, infos
