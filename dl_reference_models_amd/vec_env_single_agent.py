"""Batched tensor API of the single-agent (CTE) sibling env: B independent copies of the reference's
``src/environments/reference_model_single_agent.py::ReferenceModel`` ("SA-env") on one GPU.

Same construction keys as the reference (``steps_per_episode``, ``num_agents``, ``deterministic``,
``blocking_penalty`` -0.2, ``move_after_goal_penalty`` -0.05, ``seed``, ``env_name``; SA-env:84-114) plus the
extension keys of ``VecReferenceModel`` (``num_envs``, ``device``, ``grid``, ``seeds``, ``rng_words``,
``fixed_starts`` / ``fixed_goals``).  ``evaluation.evaluate`` / ``evaluation.JointEvaluator`` run batched evaluations on it.
"""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from .engine_handle import EngineHandle, _raw_stream

INFO_KEYS = ("blocking_count_step", "goals_reached_step", "goals_reached_total", "blocking_count_total")


def output_sections(B: int):
    """The small per-step outputs of ``VecSingleAgentReferenceModel`` as (attribute, shape, dtype), in their order in
    ``_out_blob``."""
    return (("_reward", (B,), torch.float64), ("_info", (B, 4), torch.float32), ("_terminated", (B,), torch.uint8),
            ("_truncated", (B,), torch.uint8))


class VecSingleAgentReferenceModel(EngineHandle):
    def __init__(self, env_config: dict):
        super().__init__(env_config)
        cfg = self.env_config
        B = self.num_envs
        H, W = self.grid_shape
        self._out_ptrs = None
        flags = L.FLAG_SINGLE_AGENT | (L.FLAG_DETERMINISTIC if self.deterministic else 0)
        self._open(L.MapfConfig(B, H, W, self.num_agents, 0, self.steps_per_episode, flags, 1, 1, 1, 1, 0.0,
                                int(self.device.index), int(cfg.get("lanes_per_env", 0))))
        self._reset_fn = self._lib.mapf_cte_reset
        self._check(self._lib.mapf_cte_configure(self._h, float(cfg.get("blocking_penalty", -0.2)),
                                                 float(cfg.get("move_after_goal_penalty", -0.05))))
        self._upload_config()
        self._alloc_outputs((B, self.obs_len), output_sections(B))
        self._place()

    def step(self, actions: torch.Tensor, auto_reset: bool = True, want_final_obs: bool = False) -> dict:
        """actions: int8 [B, N] (the reference's MultiDiscrete([5]*N) action per env)."""
        if actions.dtype != torch.int8 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int8).contiguous()
        if tuple(actions.shape) != (self.num_envs, self.num_agents):
            raise ValueError(f"actions must have shape {(self.num_envs, self.num_agents)}")
        # (the output tensors live as long as the handle: their pointers are marshalled once, the per-call cost is the
        #  actions' pointer, the raw handle of the current stream and one ctypes call)
        po = self._out_ptrs
        if po is None:
            po = self._out_ptrs = tuple(C.c_void_p(t.data_ptr()) for t in (self._obs, self._reward, self._terminated, self._truncated,
                                                                          self._info, self._final_obs))
            self._out_plain = {"obs": self._obs, "reward": self._reward, "terminated": self._terminated, "truncated": self._truncated,
                               "info": self._info, "final_obs": None}
            self._out_final = dict(self._out_plain, final_obs=self._final_obs)
            self._act_shape = (self.num_envs, self.num_agents)
        final = want_final_obs and auto_reset
        rc = self._lib.mapf_cte_step(self._h, actions.data_ptr(), po[0], po[1], po[2], po[3], po[4], po[5] if final else None,
                                     1 if auto_reset else 0, _raw_stream(self._dev_index))
        if rc != 0:
            self._check(rc)
        return self._out_final if final else self._out_plain

    def step_masked(self, actions: torch.Tensor, env_mask: torch.Tensor, auto_reset: bool = False) -> dict:
        """step() of the envs whose ``env_mask`` byte is nonzero (mapf_cte_step_masked); every other env -- state, stream,
        counters, episode statistics -- and its rows of the output tensors are left exactly as they were.  Returns the
        same preallocated outputs as step() (``final_obs`` None)."""
        actions = self._int8_actions(actions, (self.num_envs, self.num_agents))
        env_mask = self._env_mask(env_mask)
        self._check(self._lib.mapf_cte_step_masked(
            self._h, C.c_void_p(actions.data_ptr()), C.c_void_p(env_mask.data_ptr()), C.c_void_p(self._obs.data_ptr()),
            C.c_void_p(self._reward.data_ptr()), C.c_void_p(self._terminated.data_ptr()),
            C.c_void_p(self._truncated.data_ptr()), C.c_void_p(self._info.data_ptr()), None, 1 if auto_reset else 0,
            self._stream()))
        return {"obs": self._obs, "reward": self._reward, "terminated": self._terminated, "truncated": self._truncated,
                "info": self._info, "final_obs": None}

    def step_many(self, actions: torch.Tensor, obs_mode: int = 1) -> dict:
        """T fused steps in one launch (mapf_cte_step_many).  actions: int8 [T, B, N].  Returns fresh tensors: obs
        ([B, row] for obs_mode 1, [T, B, row] for 2, None for 0), reward [T, B] float64, terminated / truncated [T, B],
        info [T, B, 4].  Finished envs are reset inside the launch (their row of that step is the reset observation).
        Call poll_error() afterwards: an invalid action is latched there, and the rows of that env from that step on are
        zeros, not results."""
        B = self.num_envs
        actions = self._int8_actions(actions, (None, B, self.num_agents))
        T = int(actions.shape[0])
        dev = self.device
        obs = None
        if obs_mode == 1:
            obs = torch.empty((B, self.obs_len), dtype=torch.float32, device=dev)
        elif obs_mode == 2:
            obs = torch.empty((T, B, self.obs_len), dtype=torch.float32, device=dev)
        # zero-filled, not empty: the kernel skips the output stores of a step in which an env hit an invalid action
        # (SA-env:401-403 raises there), so those [t, env] rows would otherwise hold uninitialised memory.  Such an env is
        # reported by poll_error(), which a caller of step_many must consult (it synchronises, so it is not done here).
        out = {"obs": obs, "reward": torch.zeros((T, B), dtype=torch.float64, device=dev),
               "terminated": torch.zeros((T, B), dtype=torch.uint8, device=dev),
               "truncated": torch.zeros((T, B), dtype=torch.uint8, device=dev),
               "info": torch.zeros((T, B, 4), dtype=torch.float32, device=dev)}
        self._check(self._lib.mapf_cte_step_many(
            self._h, T, C.c_void_p(actions.data_ptr()), None if obs is None else C.c_void_p(obs.data_ptr()), int(obs_mode),
            C.c_void_p(out["reward"].data_ptr()), C.c_void_p(out["terminated"].data_ptr()),
            C.c_void_p(out["truncated"].data_ptr()), C.c_void_p(out["info"].data_ptr()), self._stream()))
        return out

    def set_step_counts(self, counts) -> None:
        """Put env b `counts[b]` steps into its episode (staggered episode boundaries for benchmarks and tests)."""
        c = self.get_state()["counters"]
        c[:, L.CTR_STEP_COUNT] = np.asarray(counts, dtype=np.int32)
        s = L.MapfState(counters=c.ctypes.data_as(C.c_void_p))
        self._check(self._lib.mapf_set_state(self._h, C.byref(s)), ValueError)

    def launch_info(self, fused: bool = False) -> dict:
        """Launch shape of ``step()`` (``fused=True``: of ``step_many()`` with T > 1, which picks its own group width)."""
        _, b, _, l, p = self._launch_shape(self._lib.mapf_cte_many_launch_info if fused else self._lib.mapf_launch_info)
        return {"blocks": b, "threads": 128, "lds_bytes": l, "lanes_per_env": p, "specialized_kernel": 0,
                "jit": False, "jit_note": "single-agent env"}

    def guided_obs(self, obs=None, out=None):
        """Not offered: the shortest-path guidance (``VecReferenceModel.guided_obs``) is for the multi-agent env's local
        observation; this env's observation holds the whole grid already."""
        raise ValueError("guided_obs is not offered on the single-agent env (VecSingleAgentReferenceModel): its observation "
                         "holds the whole grid already; use VecReferenceModel")

    guidance = guided_obs

    def poll_error(self):
        rc = self._poll()[0]
        if rc == L.MAPF_OK:
            return
        if rc == L.MAPF_ERR_BAD_ACTION:
            raise ValueError("Invalid action")  # SA-env:401-403
        raise RuntimeError(self._lib.mapf_last_error(self._h).decode())

    def get_state(self) -> dict:
        B, N = self.num_envs, self.num_agents
        out = {"positions": np.zeros((B, N, 2), np.int16), "goals": np.zeros((B, N, 2), np.int16),
               "starts": np.zeros((B, N, 2), np.int16), "reached": np.zeros((B, N), np.uint8),
               "counters": np.zeros((B, L.NUM_COUNTERS), np.int32), "rng_words": np.zeros((B, 6), np.uint64)}
        s = L.MapfState(**{k: v.ctypes.data_as(C.c_void_p) for k, v in out.items()})
        self._check(self._lib.mapf_get_state(self._h, C.byref(s)))
        return out
