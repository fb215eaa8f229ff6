"""Batched evaluation: the reference's test mode (main.py ``test_trained_model``) for B envs at once, on the device.

The reference runs ``num_episodes`` times ``reset()`` + ``step()`` until done with one env object, keeps one result row per
episode (main.py:286-324) and one visit count per cell (main.py:153-155, :262-267), and writes them as CSV and as a heatmap.
Here every env of a ``VecReferenceModel`` runs ``episodes_per_env`` episodes of its own and the bookkeeping is one small
launch per step (``mapf_eval_record``, include/mapf_step.h), so a checkpoint is evaluated over thousands of seeds with one
handle, three launches per step and no host round trip inside the loop:

    env = VecReferenceModel({..., "num_envs": 4096, "seed": 0})
    res, heat = evaluate(env, policy, episodes_per_env=4)        # policy(obs, first) -> int8 [B, N], or "random"
    table = results_table(res, lifelong=env.lifelong_mapf)
    write_results_csv("results.csv", table)

An env that has finished its episodes idles (it is masked out of the step and keeps its terminal state) while the others
run; episode boundaries are ``step(auto_reset=False)`` followed by ``reset`` of the finished envs, the reference's own
order of calls, so every env sees the placements its reference counterpart with the same seed sees.

The test mode's third output, the video of the first episodes (main.py ``SAVE_VIDEO``), and the per-agent paths the
reference's planner scripts report come from a trace: ``evaluate(..., trace=TraceSpec(env_ids, episodes))`` keeps one word
per agent and step of the named envs on the device (``mapf_eval_trace``, two more launches per step) and returns a
``Trace`` that redraws any frame (``mapf_render_words``), writes the GIF and the ``.npz``, and counts ``path_metrics``.

The single-agent (CTE) env, for which the reference has no test mode (main.py:37), is evaluated the same way: ``evaluate``
takes a ``VecSingleAgentReferenceModel`` too (``JointEvaluator``, ``mapf_cte_eval_record``: the same loop restated for a
gym.Env), and ``joint_neural_policy`` runs a trained ``JointActionPolicy`` in it.
"""

from __future__ import annotations

import csv

import numpy as np
import torch

from . import _lib as L
from .device_net import DeviceNet, ptr
from .engine_handle import config_seeds
from .vec_env import INFO_ALL_KEYS, VecReferenceModel
from .vec_env_single_agent import INFO_KEYS as SA_INFO_KEYS
from .vec_env_single_agent import VecSingleAgentReferenceModel

INFO_GOALS_REACHED_TOTAL = INFO_ALL_KEYS.index("goals_reached_total")
INFO_COMPLETION_RATIO = INFO_ALL_KEYS.index("completion_ratio")


class TraceSpec:
    """Which envs of an evaluation are traced and how many of their episodes (``evaluate(..., trace=TraceSpec(...))``):
    ``env_ids`` a non-empty sequence of env indices, any order, duplicates allowed; ``episodes`` the first so many episodes
    of each, at least 1 and clamped to the evaluation's ``episodes_per_env``.  ``resolve`` checks the ids against a batch."""

    def __init__(self, env_ids=(0,), episodes: int = 1):
        ids = np.atleast_1d(np.asarray(env_ids))
        if ids.ndim != 1 or ids.size == 0 or not np.issubdtype(ids.dtype, np.integer):
            raise ValueError("env_ids must be a non-empty 1-D sequence of integers")
        if ids.min() < 0:
            raise ValueError(f"env_ids must not be negative, got {int(ids.min())}")
        if int(episodes) != episodes or int(episodes) < 1:
            raise ValueError(f"episodes must be an integer >= 1, got {episodes!r}")
        self.env_ids = ids.astype(np.int32)
        self.episodes = int(episodes)

    def resolve(self, num_envs: int, episodes_per_env: int):
        """``(env_ids int32 [K], V)`` for a batch of ``num_envs`` envs that run ``episodes_per_env`` episodes each."""
        if int(self.env_ids.max()) >= num_envs:
            raise ValueError(f"env_ids must lie in [0, {num_envs}), got {int(self.env_ids.max())}")
        return self.env_ids, min(self.episodes, int(episodes_per_env))


class _Recorder:
    """What ``Evaluator`` and ``JointEvaluator`` share: the record buffers of one evaluation as torch tensors on the env's
    device, and the three-launch step (masked step, recorder, masked reset).  A subclass checks the class of its env, names
    the ``*_eval_begin`` entry point (``BEGIN``) and the widths of a record's float64 and info rows, makes the first two
    launches in ``_step`` and ``_record`` and turns the rows of finished episodes into its ``results()``.

    ``begin()`` starts the evaluation and returns the first observations; ``step(actions)`` returns ``(obs, first)``;
    ``done()`` reads back whether every env has finished (one host round trip: poll it rarely); ``results()`` and
    ``heatmap()`` copy the records to the host.

    ``trace(spec)``, called before ``begin()``, also keeps the per-step state of the envs a ``TraceSpec`` names
    (``mapf_eval_trace``): one more launch after ``begin()``'s reset, and a step becomes five launches -- masked step, trace
    STEP, recorder, masked reset, trace RESET.  ``get_trace()`` wraps the words as a ``Trace``."""

    BEGIN = None  # name of the library's begin call

    def __init__(self, env, episodes_per_env: int, f64_cols: int, info_cols: int):
        E = int(episodes_per_env)
        if E < 1:
            raise ValueError(f"episodes_per_env must be >= 1, got {episodes_per_env}")
        self.env = env
        self.episodes_per_env = E
        B, N = env.num_envs, env.num_agents
        H, W = env.grid_shape
        dev = env.device
        # (torch has no arithmetic on uint32: the counts are kept in int32 storage and read as uint32 on the host)
        self.heat = torch.zeros((B, H, W), dtype=torch.int32, device=dev)
        self.ep_i32 = torch.zeros((B, E, 2 + 4 * N), dtype=torch.int32, device=dev)
        self.ep_f64 = torch.zeros((B, E, f64_cols) if f64_cols > 1 else (B, E), dtype=torch.float64, device=dev)
        self.ep_info = torch.zeros((B, E, info_cols), dtype=torch.float32, device=dev)
        self.episodes_recorded = torch.zeros((B,), dtype=torch.int32, device=dev)
        self.active = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.reset_mask = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.max_steps = E * env.steps_per_episode  # every episode ends at the step limit at the latest
        self._act_shape = torch.Size((B, N))
        self._begun = False
        self._trace_ids = self._trace_words = None

    def trace(self, spec: TraceSpec) -> None:
        """Trace the envs of ``spec`` from ``begin()`` on.  Allocates the words, int32 storage of uint32
        [K, V, steps_per_episode + 1, N] on the env's device (zeroed; only slots up to an episode's length are written)."""
        if self._begun:
            raise RuntimeError("trace() must be called before begin()")
        e = self.env
        ids, V = spec.resolve(e.num_envs, self.episodes_per_env)
        self._trace_ids = torch.from_numpy(ids).to(e.device)
        self._trace_words = torch.zeros((len(ids), V, e.steps_per_episode + 1, e.num_agents), dtype=torch.int32, device=e.device)

    def begin(self) -> torch.Tensor:
        e = self.env
        e._check(getattr(e._lib, self.BEGIN)(e._h, self.episodes_per_env, ptr(self.heat), ptr(self.ep_i32), ptr(self.ep_f64),
                                             ptr(self.ep_info), ptr(self.episodes_recorded), ptr(self.active),
                                             ptr(self.reset_mask), e._stream()), ValueError)
        self._begun = True
        if self._trace_words is None:
            return e.reset()
        K, V = self._trace_words.shape[:2]
        e._check(e._lib.mapf_eval_trace_begin(e._h, K, ptr(self._trace_ids), V, ptr(self._trace_words), e._stream()), ValueError)
        obs = e.reset()
        e._check(e._lib.mapf_eval_trace(e._h, L.TRACE_START, e._stream()))
        return obs

    def step(self, actions: torch.Tensor):
        """One step of every env that still has episodes to run, its bookkeeping, and the reset of the envs whose episode
        just ended.  actions: int8 [B, N] on the device (rows of idle envs are ignored).  Returns ``obs`` (the env's
        observation tensor, overwritten by the next call) and ``first`` uint8 [B]: 1 where the row of ``obs`` is the
        first observation of a new episode (a recurrent policy clears its state there).  Nothing is synchronized and
        nothing is allocated when ``actions`` already is a contiguous int8 device tensor."""
        if not self._begun:
            raise RuntimeError(f"{type(self).__name__}.begin() must be called before step()")
        e = self.env
        if actions.dtype != torch.int8 or actions.device != e.device or not actions.is_contiguous():
            actions = actions.to(device=e.device, dtype=torch.int8).contiguous()
        if actions.shape != self._act_shape:
            raise ValueError(f"actions must have shape {tuple(self._act_shape)}")
        lib, h, s = e._lib, e._h, e._stream()
        traced = self._trace_words is not None
        rc = self._step(lib, h, ptr(actions), s)
        if traced and rc == L.MAPF_OK:  # before the recorder, which moves the episode and step counters on
            rc = lib.mapf_eval_trace(h, L.TRACE_STEP, s)
        if rc == L.MAPF_OK:
            rc = self._record(lib, h, s)
        if rc == L.MAPF_OK:
            rc = e._reset_fn(h, ptr(self.reset_mask), ptr(e._obs), s)
        if traced and rc == L.MAPF_OK:
            rc = lib.mapf_eval_trace(h, L.TRACE_RESET, s)
        if rc != L.MAPF_OK:
            e._check(rc)
        return e._obs, self.reset_mask

    def _step(self, lib, h, actions, s) -> int:
        """The masked step of the envs that still run (first launch of a step)."""
        raise NotImplementedError

    def _record(self, lib, h, s) -> int:
        """The recorder launch on the outputs of ``_step``."""
        raise NotImplementedError

    def get_trace(self, results: dict | None = None) -> "Trace":
        """The traced episodes as a ``Trace`` (after the evaluation has finished; ``results``: this recorder's, when the
        caller has them already)."""
        if self._trace_words is None:
            raise RuntimeError("nothing was traced: call trace(spec) before begin()")
        return Trace.from_results(self.env, self._trace_words, self._trace_ids.cpu().numpy(), results or self.results())

    def done(self) -> bool:
        return not bool(self.active.any().item())

    def end(self) -> None:
        if self._begun and getattr(self.env, "_h", None):
            self.env._check(self.env._lib.mapf_eval_end(self.env._h))
        self._begun = False

    def _rows(self):
        """``(env index, episode index, ep_i32 rows, ep_f64 rows, ep_info rows, episodes_recorded)`` of the finished
        episodes on the host, ordered by (env, episode of that env)."""
        self.env.poll_error()
        n = self.episodes_recorded.cpu().numpy()
        i32, f64, info = self.ep_i32.cpu().numpy(), self.ep_f64.cpu().numpy(), self.ep_info.cpu().numpy()
        keep = np.arange(self.episodes_per_env)[None, :] < n[:, None]
        b, k = np.nonzero(keep)
        return b, k, i32[b, k], f64[b, k], info[b, k], n

    def heatmap(self, per_env: bool = False) -> np.ndarray:
        """Number of visits per cell (main.py:262-267, "Number of visits" of the saved plot): int64 [H, W] summed over the
        envs, or [B, H, W]."""
        self.env.poll_error()
        h = self.heat.cpu().numpy().view(np.uint32).astype(np.int64)
        return h if per_env else h.sum(axis=0)


class Evaluator(_Recorder):
    """The recorder of a ``VecReferenceModel`` (``mapf_eval_record``); ``_Recorder`` states the methods."""

    BEGIN = "mapf_eval_begin"

    def __init__(self, env: VecReferenceModel, episodes_per_env: int):
        if not isinstance(env, VecReferenceModel):
            raise TypeError("Evaluator needs a VecReferenceModel (the reference's test mode is multi-agent only; "
                            "JointEvaluator takes a VecSingleAgentReferenceModel)")
        super().__init__(env, episodes_per_env, 1 + env.num_agents, L.INFO_ALL)

    def _step(self, lib, h, actions, s) -> int:
        e = self.env
        return lib.mapf_step_masked(h, actions, ptr(self.active), ptr(e._obs), ptr(e._rewards), ptr(e._terminated),
                                    ptr(e._truncated), ptr(e._info_all), ptr(e._info_agent), None, 0, s)

    def _record(self, lib, h, s) -> int:
        e = self.env
        return lib.mapf_eval_record(h, ptr(e._rewards), ptr(e._terminated), ptr(e._truncated), ptr(e._info_all), s)

    def results(self) -> dict:
        """The records of every finished episode as NumPy arrays, M rows ordered by (env, episode of that env):
        ``env`` / ``episode`` int32 [M] (episode counts from 0), ``timesteps`` int32 [M], ``terminated`` / ``truncated``
        bool [M], ``total_reward`` float64 [M], ``agent_reward`` float64 [M, N], ``starts`` / ``goals`` int32 [M, N, 2]
        (row, col), ``info_all`` float32 [M, 14] (the terminal step's, ``INFO_ALL_KEYS`` columns), plus
        ``episodes_recorded`` int32 [B] and ``seeds`` (one per env, None where the env was seeded from OS entropy)."""
        b, k, i32, f64, info, n = self._rows()
        sg = i32[:, 2:].reshape(-1, self.env.num_agents, 4)
        return {
            "env": b.astype(np.int32), "episode": k.astype(np.int32), "timesteps": i32[:, 0].copy(),
            "terminated": (i32[:, 1] & 1) != 0, "truncated": (i32[:, 1] & 2) != 0,
            "total_reward": f64[:, 0].copy(), "agent_reward": f64[:, 1:].copy(),
            "starts": sg[:, :, 0:2].copy(), "goals": sg[:, :, 2:4].copy(), "info_all": info,
            "episodes_recorded": n, "seeds": env_seeds(self.env),
        }


class JointEvaluator(_Recorder):
    """The recorder of a ``VecSingleAgentReferenceModel`` (``mapf_cte_eval_record``): main.py's test loop restated for the
    single-agent env, whose one policy moves all N agents.  ``_Recorder`` states the methods; ``step`` takes the joint
    actions int8 [B, N].  The env has one float64 reward: an episode's ``total_reward`` is the running sum of its step
    rewards in step order, Python's ``episode_reward += reward`` bit for bit."""

    BEGIN = "mapf_cte_eval_begin"

    def __init__(self, env: VecSingleAgentReferenceModel, episodes_per_env: int):
        if not isinstance(env, VecSingleAgentReferenceModel):
            raise TypeError("JointEvaluator needs a VecSingleAgentReferenceModel (Evaluator takes a VecReferenceModel)")
        super().__init__(env, episodes_per_env, 1, len(SA_INFO_KEYS))

    def _step(self, lib, h, actions, s) -> int:
        e = self.env
        return lib.mapf_cte_step_masked(h, actions, ptr(self.active), ptr(e._obs), ptr(e._reward), ptr(e._terminated),
                                        ptr(e._truncated), ptr(e._info), None, 0, s)

    def _record(self, lib, h, s) -> int:
        e = self.env
        return lib.mapf_cte_eval_record(h, ptr(e._reward), ptr(e._terminated), ptr(e._truncated), ptr(e._info), s)

    def results(self) -> dict:
        """The records of every finished episode as NumPy arrays, M rows ordered by (env, episode of that env):
        ``env`` / ``episode`` int32 [M] (episode counts from 0), ``timesteps`` int32 [M], ``terminated`` / ``truncated``
        bool [M] (an episode that ends at the step limit carries both, SA-env:347-348: success is terminated without
        truncated), ``total_reward`` float64 [M], ``starts`` / ``goals`` int32 [M, N, 2] (row, col), ``info`` float32
        [M, 4] (the terminal step's, ``vec_env_single_agent.INFO_KEYS`` columns), plus ``episodes_recorded`` int32 [B] and
        ``seeds``.  There is no ``agent_reward``: the env has one reward."""
        b, k, i32, f64, info, n = self._rows()
        sg = i32[:, 2:].reshape(-1, self.env.num_agents, 4)
        return {
            "env": b.astype(np.int32), "episode": k.astype(np.int32), "timesteps": i32[:, 0].copy(),
            "terminated": (i32[:, 1] & 1) != 0, "truncated": (i32[:, 1] & 2) != 0, "total_reward": f64.copy(),
            "starts": sg[:, :, 0:2].copy(), "goals": sg[:, :, 2:4].copy(), "info": info,
            "episodes_recorded": n, "seeds": env_seeds(self.env),
        }


class Trace:
    """The traced episodes of an evaluation (``evaluate(..., trace=TraceSpec(...))``): per step, the position and goal of
    every agent of K envs, V episodes each -- enough to redraw every frame bit for bit (``mapf_render_words``) and to
    measure every agent's path.

    ``words`` int32 storage of uint32 [K, V, S + 1, N] (``col | row << 8 | goal_col << 16 | goal_row << 24``,
    include/mapf_step.h), on the env's device, or a NumPy array after ``load``; ``env_ids`` int32 [K]; ``lengths`` int32
    [K, V], the recorder's ``timesteps`` of episode v of env ``env_ids[k]`` (slot t of an episode is valid for t <=
    length; 0 = the env recorded no such episode); ``seeds`` one per traced env; ``lifelong`` whether goals move.
    ``env`` draws the frames: the env the trace came from, or, for a loaded trace, any env of the same kind with the same
    grids (``attach``)."""

    def __init__(self, words, env_ids, lengths, seeds=None, lifelong: bool = False, env=None):
        self.words = words
        self.env_ids = np.asarray(env_ids, np.int32)
        self.lengths = np.asarray(lengths, np.int32)
        K, V = self.lengths.shape
        if tuple(words.shape[:2]) != (K, V) or len(words.shape) != 4 or len(self.env_ids) != K:
            raise ValueError("words must be [K, V, S + 1, N] with env_ids [K] and lengths [K, V]")
        if self.lengths.min(initial=0) < 0 or self.lengths.max(initial=0) > int(words.shape[2]) - 1:
            raise ValueError("lengths must lie in [0, S]")
        self.seeds = [None] * K if seeds is None else list(seeds)
        self.lifelong = bool(lifelong)
        self.env = env
        self._host = None
        self._dev = None

    @classmethod
    def from_results(cls, env, words, env_ids, results: dict) -> "Trace":
        """The trace of a finished evaluation: the lengths are the ``timesteps`` of ``results``."""
        K, V = int(words.shape[0]), int(words.shape[1])
        per_env = np.zeros((len(results["episodes_recorded"]), V), np.int32)
        m = np.asarray(results["episode"]) < V
        per_env[results["env"][m], results["episode"][m]] = results["timesteps"][m]
        seeds = [results["seeds"][int(b)] for b in env_ids]
        return cls(words, env_ids, per_env[np.asarray(env_ids)], seeds, bool(getattr(env, "lifelong_mapf", False)), env)

    @property
    def shape(self):
        return tuple(int(s) for s in self.words.shape)

    def attach(self, env) -> "Trace":
        """Draw frames with ``env``: its grid shape and agent count must be the trace's, its batch must hold ``env_ids``."""
        if env.num_agents != self.shape[3] or int(self.env_ids.max()) >= env.num_envs:
            raise ValueError("the env's agent count and batch must hold the trace's")
        self.env, self._dev = env, None
        return self

    def host_words(self) -> np.ndarray:
        """The words as uint32 [K, V, S + 1, N] on the host (one copy, kept)."""
        if self._host is None:
            w = self.words.cpu().numpy() if isinstance(self.words, torch.Tensor) else np.asarray(self.words)
            self._host = np.ascontiguousarray(w).view(np.uint32)
        return self._host

    def _episode(self, k: int, v: int) -> np.ndarray:
        K, V = self.lengths.shape
        if not (0 <= k < K and 0 <= v < V):
            raise IndexError(f"(k, v) = ({k}, {v}) outside the trace's [{K}, {V}]")
        return self.host_words()[k, v, :int(self.lengths[k, v]) + 1]

    def positions(self, k: int, v: int) -> np.ndarray:
        """int32 [len + 1, N, 2] (row, col) of every agent: the episode's placement, then the state after every step."""
        w = self._episode(k, v)
        return np.stack([(w >> 8) & 255, w & 255], axis=-1).astype(np.int32)

    def goals(self, k: int, v: int) -> np.ndarray:
        """int32 [len + 1, N, 2] (row, col): every agent's goal at the same moments (they move in lifelong mode only)."""
        w = self._episode(k, v)
        return np.stack([w >> 24, (w >> 16) & 255], axis=-1).astype(np.int32)

    def slot_rows(self, k: int, v: int) -> np.ndarray:
        """Rows of the words, viewed as [K * V * (S + 1), N], that hold episode (k, v): int32 [len + 1]."""
        _K, V, S1, _N = self.shape
        self._episode(k, v)
        return ((k * V + v) * S1 + np.arange(int(self.lengths[k, v]) + 1)).astype(np.int32)

    def render_rows(self, rows, env_ids, cell_px: int, out: torch.Tensor | None = None) -> torch.Tensor:
        """One ``mapf_render_words`` launch: uint8 [F, H*c, W*c, 3] on the env's device, frame f from row ``rows[f]`` of the
        words over the grid of env ``env_ids[f]``; enqueued on the current stream, no sync."""
        env = self.env
        if env is None:
            raise RuntimeError("this trace has no env to draw with: attach(env) first")
        c = int(cell_px)
        if not L.RENDER_MIN_CELL_PX <= c <= L.RENDER_MAX_CELL_PX:
            raise ValueError(f"cell_px must lie in [{L.RENDER_MIN_CELL_PX}, {L.RENDER_MAX_CELL_PX}], got {cell_px}")
        rows, ids = np.asarray(rows, np.int32), np.asarray(env_ids, np.int32)
        K, V, S1, _N = self.shape
        if rows.ndim != 1 or rows.size == 0 or rows.shape != ids.shape or rows.min() < 0 or rows.max() >= K * V * S1:
            raise ValueError("rows and env_ids must be equally long, non-empty, rows inside the words")
        if ids.min() < 0 or ids.max() >= env.num_envs:
            raise ValueError(f"env_ids must lie in [0, {env.num_envs})")
        if self._dev is None:
            w = self.words if isinstance(self.words, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(self.words).view(np.int32))
            self._dev = w.to(env.device).contiguous()
        H, W = env.grid_shape
        shape = (int(rows.size), H * c, W * c, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=env.device)
        elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != env.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on {env.device}")
        both = torch.from_numpy(np.stack([rows, ids])).to(env.device)
        env._check(env._lib.mapf_render_words(env._h, ptr(self._dev), ptr(both[0]), ptr(both[1]), shape[0], c, ptr(out),
                                              env._stream()), ValueError)
        return out

    def frames(self, k: int, v: int, cell_px: int = 32, out: torch.Tensor | None = None) -> torch.Tensor:
        """Every frame of episode (k, v), uint8 [len + 1, H*c, W*c, 3] on the device: one launch."""
        rows = self.slot_rows(k, v)
        return self.render_rows(rows, np.full(len(rows), self.env_ids[k], np.int32), cell_px, out)

    def video_rows(self, hold: int = 3):
        """``(rows, env_ids)`` of a video in main.py's order (main.py:188-194, :239-243, :269-274): the recorded episodes in
        sequence -- traced env after traced env, each env's episodes in order -- every episode's frames followed by its
        last frame ``hold`` more times."""
        rows, ids = [], []
        K, V = self.lengths.shape
        for k in range(K):
            for v in range(V):
                if self.lengths[k, v] < 1:
                    continue
                r = self.slot_rows(k, v)
                r = np.concatenate([r, np.repeat(r[-1:], max(int(hold), 0))])
                rows.append(r)
                ids.append(np.full(len(r), self.env_ids[k], np.int32))
        if not rows:
            return np.zeros(0, np.int32), np.zeros(0, np.int32)
        return np.concatenate(rows).astype(np.int32), np.concatenate(ids)

    def video_chunks(self, hold: int = 3, cell_px: int = 32, max_frames: int = 64):
        """Yields the video's frames as uint8 NumPy arrays [n, H*c, W*c, 3], n <= ``max_frames``, rendered chunk by chunk so
        that a long video is never resident at once (one launch and one copy to the host per chunk)."""
        rows, ids = self.video_rows(hold)
        step = max(1, int(max_frames))
        for i in range(0, len(rows), step):
            yield self.render_rows(rows[i:i + step], ids[i:i + step], cell_px).cpu().numpy()

    def write_gif(self, path, fps: int = 5, hold: int = 3, cell_px: int = 32, max_frames: int = 64) -> int:
        """The video as an animated GIF at ``fps`` frames per second, looping (what imageio.mimsave writes at main.py:346,
        through PIL).  Returns the number of frames of the video; the encoder stores a frame that repeats its predecessor
        (a held last frame, a step in which nobody moved) as a longer display time of that one, which plays the same."""
        try:
            from PIL import Image
        except ImportError as exc:
            raise ImportError("write_gif needs PIL (the Pillow package) to encode the GIF") from exc
        rows, ids = self.video_rows(hold)
        if len(rows) == 0:
            raise ValueError("the trace holds no recorded episode")
        # One palette for the whole file, from up to 32 frames spread over the video: the raster has few colours (exact when
        # the sample holds at most 256), and a palette per frame would let equal frames differ.
        pick = np.unique(np.linspace(0, len(rows) - 1, min(len(rows), 32)).astype(np.int64))
        sample = self.render_rows(rows[pick], ids[pick], cell_px).cpu().numpy().reshape(-1, 3).astype(np.uint32)
        colours = np.unique(sample[:, 0] << 16 | sample[:, 1] << 8 | sample[:, 2])
        rgb = np.stack([colours >> 16, (colours >> 8) & 255, colours & 255], axis=1).astype(np.uint8)
        if len(rgb) <= 256:
            palette = Image.new("P", (1, 1))
            palette.putpalette(np.concatenate([rgb, np.repeat(rgb[-1:], 256 - len(rgb), axis=0)]).reshape(-1).tolist())
        else:
            palette = Image.fromarray(rgb[None]).quantize(colors=256, method=Image.Quantize.MEDIANCUT)

        def images():  # (chunk by chunk: the encoder pulls the frames one at a time)
            for chunk in self.video_chunks(hold, cell_px, max_frames):
                for f in chunk:
                    yield Image.fromarray(f).quantize(palette=palette, dither=Image.Dither.NONE)

        it = images()
        next(it).save(path, format="GIF", save_all=True, append_images=it, duration=int(round(1000 / max(int(fps), 1))), loop=0,
                      optimize=False)
        return len(rows)

    def save(self, path) -> None:
        """The exact artefact as ``.npz``: words (uint32), lengths, env ids, seeds (-1 = none), lifelong."""
        seeds = np.array([-1 if s is None else int(s) for s in self.seeds], np.int64)
        with open(path, "wb") as f:
            np.savez_compressed(f, words=self.host_words(), lengths=self.lengths, env_ids=self.env_ids, seeds=seeds,
                                lifelong=np.array(self.lifelong))

    @classmethod
    def load(cls, path, env=None) -> "Trace":
        with np.load(path) as z:
            seeds = [None if s < 0 else int(s) for s in z["seeds"]]
            t = cls(z["words"].astype(np.uint32), z["env_ids"], z["lengths"], seeds, bool(z["lifelong"]))
        return t.attach(env) if env is not None else t

    def path_metrics(self) -> dict:
        """Per recorded episode, what scripts/a-star.py:204-239 counts on every agent's path (positions 0 .. len):
        ``steps`` int32 [K, V, N], the positions up to and including the first one on the agent's goal (1 for an agent that
        starts there, len + 1 for one that never arrives); ``total_distance`` int32 [K, V, N], the Manhattan distance
        between consecutive positions up to there; ``max_steps`` int32 [K, V], the largest ``steps`` of the episode.
        Episodes that were not recorded hold -1.  Finite mode only: in lifelong mode the goals move."""
        if self.lifelong:
            raise ValueError("path_metrics counts the way to one goal per agent: it does not apply to lifelong_mapf")
        K, V = self.lengths.shape
        N = self.shape[3]
        steps = np.full((K, V, N), -1, np.int32)
        dist = np.full((K, V, N), -1, np.int32)
        for k in range(K):
            for v in range(V):
                if self.lengths[k, v] < 1:
                    continue
                pos, goal = self.positions(k, v), self.goals(k, v)[0]
                at_goal = (pos == goal[None]).all(axis=2)  # [len + 1, N]
                n = np.where(at_goal.any(axis=0), at_goal.argmax(axis=0), len(pos) - 1) + 1
                moved = np.abs(np.diff(pos, axis=0)).sum(axis=2)  # [len, N]
                steps[k, v] = n
                dist[k, v] = [int(moved[:n[a] - 1, a].sum()) for a in range(N)]
        return {"steps": steps, "total_distance": dist, "max_steps": steps.max(axis=2, initial=-1).astype(np.int32)}


def env_seeds(env: VecReferenceModel) -> list:
    """The NumPy seed of every env as ``VecReferenceModel`` derives it from its config (None: not seeded by number)."""
    if env.env_config.get("rng_words", None) is not None:
        return [None] * env.num_envs
    return [None if s is None else int(s) for s in config_seeds(env.env_config, env.num_envs)]


def random_policy(env: VecReferenceModel, seed: int = 0):
    """main.py's ``ALGO_NAME = "RANDOM"``: uniform actions, here from one seeded device generator for all envs."""
    gen = torch.Generator(device=env.device)
    gen.manual_seed(int(seed))
    shape = (env.num_envs, env.num_agents)

    def policy(_obs, _first):
        return torch.randint(0, 5, shape, generator=gen, device=env.device, dtype=torch.int8)

    return policy


def shortest_path_policy(env: VecReferenceModel, yielding: bool = True):
    """The classical baseline next to a trained policy (the reference's scripts/a-star.py, per agent and without
    coordination): every agent takes a first move of a shortest path to its goal, searched on the device from the env's
    current state (``EngineHandle.expert_actions``).  yielding: an agent does not step onto a cell another agent stands
    on -- it takes another shortest move or waits; False: the agents ignore each other.  The callable ignores ``obs`` and
    ``first`` and writes into one action tensor of its own."""
    mode = "yielding" if yielding else "independent"
    out = torch.empty((env.num_envs, env.num_agents), dtype=torch.int8, device=env.device)

    def policy(_obs, _first):
        return env.expert_actions(mode, out=out)

    return policy


def _plan_player(plan: torch.Tensor):
    """``play(first)`` for a stored ``plan`` int8 [B, T, N] (read when called, so a planner may rewrite it in place): the
    next row of every env's plan, zeros (wait) past the horizon; an env's step cursor restarts where ``first`` is set."""
    B, T = int(plan.shape[0]), int(plan.shape[1])
    cursor = torch.zeros((B,), dtype=torch.int64, device=plan.device)
    rows = torch.arange(B, device=plan.device)

    def play(first):
        cursor.mul_((first == 0).to(torch.int64))
        acts = plan[rows, cursor.clamp(max=T - 1)] * (cursor < T).to(torch.int8)[:, None]
        cursor.add_(1)
        return acts

    return play


def prioritized_policy(env: VecReferenceModel, horizon: int | None = None):
    """The coordinated classical baseline (the reference's scripts/cbs.py plans the agents together; here prioritised
    planning in the env's move order, ``EngineHandle.plan_prioritized``): where ``first`` is set the env's episode is
    planned as a whole, then every step plays the next row of the plan, waits past the horizon.  A solved env executes its
    plan without a failed move and terminates after at most ``makespan`` steps; an unsolved env plays what was planned
    (agents without a path wait).  Plans, a step cursor per env and the action tensor stay on the device: no host round
    trip.  Finite mode only: in lifelong mode the goals change under the plan (``windowed_policy`` replans as it goes)."""
    if env.lifelong_mapf:
        raise ValueError("prioritized_policy plans an episode once: it does not apply to lifelong_mapf, where goals change "
                         '(use "windowed")')
    plan, arrival = env.plan_prioritized(horizon)  # (sizes the buffers and the handle's workspace)
    T = int(plan.shape[1])
    play = _plan_player(plan)

    def policy(_obs, first):
        env.plan_prioritized(T, mask=first, out=(plan, arrival))
        return play(first)

    return policy


def cbs_policy(env: VecReferenceModel, horizon: int | None = None, max_nodes: int = 256, fallback: str | None = "prioritized"):
    """The reference's own coordinated baseline (scripts/cbs.py), conflict-based search on the device
    (``EngineHandle.plan_cbs``): where ``first`` is set the env's episode is planned as a whole, then every step plays the
    next row of the plan, waits past the horizon.  A solved env plays the plan of least sum of costs.  Envs the search does
    not solve within ``max_nodes`` nodes are planned by one ``plan_prioritized`` call masked to them (``fallback=
    "prioritized"``), or wait out the episode (``fallback=None``).  Plans, the fallback mask, a step cursor per env and
    the action tensor stay on the device: no host round trip.  Finite mode only, as ``prioritized_policy``."""
    if env.lifelong_mapf:
        raise ValueError("cbs_policy plans an episode once: it does not apply to lifelong_mapf, where goals change "
                         '(use "windowed")')
    if fallback not in (None, "prioritized"):
        raise ValueError(f'fallback must be "prioritized" or None, got {fallback!r}')
    out = env.plan_cbs(horizon, max_nodes)  # (sizes the buffers and the handle's node store)
    plan, arrival = out["plan"], out["arrival"]
    T = int(plan.shape[1])
    if fallback:
        env.plan_prioritized(T)  # (sizes its workspace)
    unsolved = torch.zeros((env.num_envs,), dtype=torch.uint8, device=env.device)
    play = _plan_player(plan)

    def policy(_obs, first):
        env.plan_cbs(T, max_nodes, mask=first, out=out)
        if fallback:
            torch.mul(first != 0, out["status"] != L.CBS_SOLVED, out=unsolved)
            env.plan_prioritized(T, mask=unsolved, out=(plan, arrival))
        return play(first)

    policy.buffers = out  # plan, arrival (the fallback's where it ran), status and nodes of every env's last episode
    return policy


def cbs_summary(status, nodes) -> dict:
    """What a ``plan_cbs`` call achieved, from its ``status`` and ``nodes`` int32 [B] (tensors or arrays): the share of
    envs per status (``solved``, ``budget``, ``infeasible``, ``no_path``) and ``mean_nodes`` / ``max_nodes_created`` over
    all envs."""
    st, nd = (np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.int64) for x in (status, nodes))
    n = max(len(st), 1)
    res = {name: float((st == code).sum()) / n for code, name in enumerate(L.CBS_STATUS_NAMES)}
    res["mean_nodes"] = float(nd.mean()) if len(nd) else 0.0
    res["max_nodes_created"] = int(nd.max()) if len(nd) else 0
    return res


def windowed_policy(env: VecReferenceModel, window: int = 16, replan_every: int = 8, replan_on_arrival: bool = False):
    """The coordinated classical baseline for lifelong mode (and finite mode alike): rolling-horizon prioritised planning,
    ``EngineHandle.plan_windowed``.  An env's next ``window`` steps are planned together; it plays ``replan_every`` of them
    and is planned again -- also where ``first`` is set, and with ``replan_on_arrival`` after a step in which one of its
    agents arrived (``arrival[b, j] == cursor[b]``: the step in which a lifelong goal respawned), so that the agent does
    not wait out the rest of its window.  A consistent window executes without a failed move; an inconsistent one plays
    what was planned (agents without a window wait).  Plans, a step cursor per env and the replan mask stay on the device:
    one planner launch per step, masked to the envs that need it, and no host round trip.  A launch that replans nothing
    returns after one ballot per workgroup: 7.6 us from Python at 1 024 to 8 192 envs."""
    w, h = int(window), int(replan_every)
    if not 1 <= w <= L.PLAN_MAX_WINDOW:
        raise ValueError(f"window must lie in [1, {L.PLAN_MAX_WINDOW}], got {window}")
    if not 1 <= h <= w:
        raise ValueError(f"replan_every must lie in [1, window = {w}], got {replan_every}")
    B, N, dev = env.num_envs, env.num_agents, env.device
    plan = torch.zeros((B, w, N), dtype=torch.int8, device=dev)
    arrival = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    remaining = torch.full((B, N), -1, dtype=torch.int32, device=dev)
    cursor = torch.zeros((B,), dtype=torch.int64, device=dev)
    replan = torch.ones((B,), dtype=torch.uint8, device=dev)
    arrived = torch.zeros((B,), dtype=torch.bool, device=dev)
    rows = torch.arange(B, device=dev)

    def policy(_obs, first):
        need = (first != 0) | (cursor >= h)
        if replan_on_arrival:
            need |= arrived
        replan.copy_(need)
        env.plan_windowed(w, mask=replan, out=(plan, arrival, remaining))
        cursor.mul_((replan == 0).to(torch.int64))
        acts = plan[rows, cursor]  # (cursor < replan_every <= window)
        cursor.add_(1)
        if replan_on_arrival:
            torch.any(arrival == cursor[:, None], dim=1, out=arrived)
        return acts

    return policy


def neural_policy(env: VecReferenceModel, policy, sample: bool = False, seed: int = 0, guidance: bool = False):
    """A trained policy (main.py's test mode with a checkpoint) as one launch per step: ``policy`` is a
    ``policy.DevicePolicy`` on the env's B * N rows, or a ``policy.MaskedRecurrentPolicy`` / ``policy.PerAgentPolicy`` / the
    path of a saved one (the checkpoint's kind says which), for which a ``DevicePolicy`` is made here; one policy per agent
    (kind ``per_agent``) needs an env with as many agents as it has policies (ValueError otherwise).  The recurrent state is cleared where ``first`` is set, and the env's own action
    and reward tensors are the previous action and reward, so nothing but the act launch runs between two env steps.
    sample: draw from the policy's distribution (counter-based noise from ``seed``) instead of the greedy action.  Not in
    ``STRING_POLICIES``: it needs weights.  A ``dqn.QNetwork``, a ``dqn.DeviceQPolicy`` or a checkpoint of kind ``q_network`` acts
    greedily on its Q-values, and with ``sample`` epsilon-greedily at epsilon = 0.05.
    guidance: the policy was trained on guided observations (``Rollout(guidance=True)``; a checkpoint does not record it):
    one ``guided_obs`` launch into a buffer of this callable's precedes the act launch, and the policy's ``obs_len`` must be
    the env's + 6 (ValueError otherwise).  Not offered for a Q-network."""
    from .policy import DevicePolicy
    from .rollout import check_guidance_fits, check_guided_obs_len

    B, N = env.num_envs, env.num_agents
    qpolicy = _as_q_policy(env, policy)
    if qpolicy is not None:
        if guidance:
            raise ValueError("guidance is not offered for a Q-network (DQN trains on the plain observation)")
        return _q_policy_fn(env, qpolicy, sample, seed)
    if guidance:  # before a device policy is asked for a row no kernel takes
        check_guidance_fits(env.obs_len)
    if not isinstance(policy, DevicePolicy):
        policy = DevicePolicy(policy, B * N, N, env.device)
    if guidance:
        check_guided_obs_len(policy.obs_len, env.obs_len, True)
    if policy.rows != B * N or policy.agents_per_env != N or policy.obs_len != env.obs_len + (L.GUIDANCE_LEN if guidance else 0):
        raise ValueError("the policy's rows, agents_per_env and obs_len must be the env's")
    policy.reset_state()
    actions = policy.action.view(B, N)
    guided = torch.zeros((B, N, env.guided_obs_len), dtype=torch.float32, device=env.device) if guidance else None

    def fn(obs, first):
        if guidance:
            obs = env.guided_obs(obs, out=guided)
        policy.act(obs, prev_action=policy.action, prev_reward=env._rewards, start=(first, None), sample=sample, seed=seed)
        return actions

    fn.policy = policy
    return fn


def joint_neural_policy(env: VecSingleAgentReferenceModel, policy, sample: bool = False, seed: int = 0):
    """A trained joint-action policy on the single-agent env as one launch per step (``mapf_jpolicy_act``): ``policy`` is a
    ``policy.JointDevicePolicy`` on the env's B rows, a ``policy.JointActionPolicy``, or the path of a saved one (what
    ``scripts/train_single_agent_env.py`` writes), for which a ``JointDevicePolicy`` is made here.  The recurrent state is
    cleared where ``first`` is set; the previous action is the policy's own action tensor and the previous reward the env's
    float64 reward tensor, so nothing but the act launch runs between two env steps.  sample: draw from the policy's
    distribution (counter-based noise from ``seed``) instead of the greedy action.  A policy made for another grid size or
    agent count raises ValueError before anything touches the device."""
    from .policy import JointActionPolicy, JointDevicePolicy

    B, N = env.num_envs, env.num_agents
    H, W = env.grid_shape
    if not isinstance(policy, JointDevicePolicy):
        policy = DeviceNet._module(JointActionPolicy, policy, "joint_neural_policy needs a JointActionPolicy, a JointDevicePolicy "
                                   "or a checkpoint of kind 'joint_action' (neural_policy runs the multi-agent kinds)")
    if policy.grid_cells != H * W or policy.num_agents != N:
        raise ValueError(f"the policy was made for {policy.grid_cells} grid cells and {policy.num_agents} agents, the env has "
                         f"{H * W} cells ({H} x {W}) and {N} agents")
    if not isinstance(policy, JointDevicePolicy):
        policy = JointDevicePolicy(policy, B, env.device)
    if policy.rows != B:
        raise ValueError(f"the policy has {policy.rows} rows, the env {B} envs")
    policy.reset_state()

    def fn(obs, first):
        policy.act(obs, prev_action=policy.action, prev_reward=env._reward, start=(first, None), sample=sample, seed=seed)
        return policy.action

    fn.policy = policy
    return fn


Q_SAMPLE_EPSILON = 0.05  # what ``sample=True`` means for a Q-network: the final epsilon of training


def _as_q_policy(env, policy):
    """A ``dqn.DeviceQPolicy`` when ``policy`` is one, a ``dqn.QNetwork`` or a checkpoint of kind ``q_network``; else None."""
    from . import dqn

    if isinstance(policy, dqn.DeviceQPolicy):
        return policy
    if isinstance(policy, torch.nn.Module):
        return dqn.DeviceQPolicy(policy, env.num_envs * env.num_agents, env.device) if isinstance(policy, dqn.QNetwork) else None
    if isinstance(policy, (str, bytes)) or hasattr(policy, "__fspath__"):
        blob = torch.load(policy, map_location="cpu", weights_only=True)
        if isinstance(blob, dict) and blob.get("kind") == dqn.QNetwork.KIND:
            return dqn.DeviceQPolicy(dqn.QNetwork.load(policy), env.num_envs * env.num_agents, env.device)
    return None


def _q_policy_fn(env, policy, sample: bool, seed: int):
    """Greedy on the Q-values, or epsilon-greedy at ``Q_SAMPLE_EPSILON`` with ``sample``: one launch per step."""
    B, N = env.num_envs, env.num_agents
    if policy.rows != B * N or policy.obs_len != env.obs_len:
        raise ValueError("the policy's rows and obs_len must be the env's")
    policy.reset_state()
    actions = policy.action.view(B, N)
    eps = None
    if sample:
        policy.epsilon.fill_(Q_SAMPLE_EPSILON)
        eps = policy.epsilon

    def fn(obs, first):
        policy.act(obs, epsilon=eps, seed=seed)
        return actions

    fn.policy = policy
    return fn


STRING_POLICIES = {
    "random": lambda env, seed: random_policy(env, seed),
    "shortest_path": lambda env, seed: shortest_path_policy(env, yielding=True),
    "shortest_path_independent": lambda env, seed: shortest_path_policy(env, yielding=False),
    "prioritized": lambda env, seed: prioritized_policy(env),
    "windowed": lambda env, seed: windowed_policy(env),
    "cbs": lambda env, seed: cbs_policy(env),
}
# the coordinated planners: include/mapf_step.h claims their no-failed-move guarantee for multi-agent handles only
MULTI_AGENT_ONLY_POLICIES = ("prioritized", "windowed", "cbs")


def evaluate(env, policy, episodes_per_env: int, poll_every: int = 32, seed: int = 0, trace: TraceSpec | None = None):
    """Runs ``episodes_per_env`` episodes of every env of ``env`` under ``policy`` and returns
    ``(Evaluator.results(), Evaluator.heatmap())``; with ``trace`` (a ``TraceSpec``) the per-step state of the envs it
    names is kept as well -- two more small launches per step, the results and the heatmap are the same -- and the return
    is ``(results, heatmap, Trace)``.  A ``VecSingleAgentReferenceModel`` is evaluated by a
    ``JointEvaluator`` (obs float32 [B, H*W + 5N], the same actions int8 [B, N]); of the strings it takes ``"random"``,
    ``"shortest_path"`` and ``"shortest_path_independent"``, the coordinated planners raise ValueError
    (``joint_neural_policy`` makes the callable of a trained joint policy).

    policy: ``policy(obs, first) -> int8 [B, N]`` on the device (obs float32 [B, N, L]; first uint8 [B], 1 where the row
    starts an episode, all ones at the first call), or a string: ``"random"`` (``random_policy(env, seed)``),
    ``"shortest_path"`` or ``"shortest_path_independent"`` (``shortest_path_policy``, yielding or not),
    ``"prioritized"`` (``prioritized_policy``: a joint plan per episode, finite mode only), ``"windowed"``
    (``windowed_policy``: the next 16 steps planned together, replanned every 8; finite and lifelong mode), ``"cbs"``
    (``cbs_policy``: conflict-based search per episode with the prioritised planner as fallback; finite mode only).  This callable is where an RLlib connector pipeline (main.py:125-229) would plug in.  The loop needs at most
    ``episodes_per_env * steps_per_episode`` steps, so the host asks the device whether every env has finished only every
    ``poll_every`` steps; steps made after that are no-ops on the device."""
    if trace is not None and not isinstance(trace, TraceSpec):
        raise TypeError("trace must be a TraceSpec or None")
    single = isinstance(env, VecSingleAgentReferenceModel)
    if isinstance(policy, str):
        if policy.lower() not in STRING_POLICIES:
            raise ValueError(f"unknown policy {policy!r} (a callable, or one of {sorted(STRING_POLICIES)})")
        if single and policy.lower() in MULTI_AGENT_ONLY_POLICIES:
            raise ValueError(f"policy {policy!r} is not offered on the single-agent env: the planner's guarantee that its plan "
                             "executes without a failed move is stated for the multi-agent move rule only (on a single-agent "
                             f"env: a callable, or one of {sorted(set(STRING_POLICIES) - set(MULTI_AGENT_ONLY_POLICIES))})")
        policy = STRING_POLICIES[policy.lower()](env, seed)
    poll_every = max(1, int(poll_every))
    ev = (JointEvaluator if single else Evaluator)(env, episodes_per_env)
    if trace is not None:
        ev.trace(trace)
    try:
        obs = ev.begin()
        first = torch.ones((env.num_envs,), dtype=torch.uint8, device=env.device)
        for t in range(ev.max_steps):
            obs, first = ev.step(policy(obs, first))
            if (t + 1) % poll_every == 0 and ev.done():
                break
        if not ev.done():
            raise RuntimeError("evaluation did not finish within episodes_per_env * steps_per_episode steps")
        if trace is None:
            return ev.results(), ev.heatmap()
        results = ev.results()
        return results, ev.heatmap(), ev.get_trace(results)
    finally:
        ev.end()


def bounds_from_lengths(sp: np.ndarray) -> dict:
    """The two lower bounds classical MAPF results are reported against, from the agents' shortest-path lengths int32
    [M, N] (-1: no path): ``sum_of_costs_lower_bound`` and ``makespan_lower_bound`` int64 / int32 [M] -- no plan can have
    the agents arrive sooner in total, or the last of them sooner -- both -1 where an agent of the episode has no path."""
    sp = np.asarray(sp, dtype=np.int32)
    ok = (sp >= 0).all(axis=1)
    return {"shortest_path": sp,
            "sum_of_costs_lower_bound": np.where(ok, sp.astype(np.int64).sum(axis=1), -1),
            "makespan_lower_bound": np.where(ok, sp.max(axis=1), -1).astype(np.int32)}


def plan_costs(arrival) -> dict:
    """What a joint plan costs, from ``plan_prioritized``'s arrivals int32 [B, N] (a tensor or an array; -1: no path found):
    ``solved`` bool [B] (every agent arrives), ``sum_of_costs`` int64 [B] (the sum of the arrivals) and ``makespan`` int32
    [B] (the last arrival), both -1 where the env is unsolved -- the numbers to quote against ``bounds_from_lengths``."""
    a = np.asarray(arrival.cpu().numpy() if isinstance(arrival, torch.Tensor) else arrival, dtype=np.int32)
    solved = (a >= 0).all(axis=1)
    return {"solved": solved, "sum_of_costs": np.where(solved, a.astype(np.int64).sum(axis=1), -1),
            "makespan": np.where(solved, a.max(axis=1, initial=-1), -1).astype(np.int32)}


def window_costs(arrival, remaining) -> dict:
    """What a window achieves, from ``plan_windowed``'s arrivals and remaining distances int32 [B, N] (tensors or arrays):
    ``consistent`` bool [B] (no agent failed: no -1 in ``remaining``), ``arrived`` int32 [B] (agents that reach their goal
    within the window; -1 where the env is inconsistent) and ``remaining_sum`` int64 [B] (the path lengths still to go at
    the end of the window, summed; -1 where the env is inconsistent or a goal is unreachable)."""
    a, rem = (np.asarray(x.cpu().numpy() if isinstance(x, torch.Tensor) else x, dtype=np.int32) for x in (arrival, remaining))
    consistent = (rem != -1).all(axis=1)
    summable = consistent & (rem >= 0).all(axis=1)
    return {"consistent": consistent, "arrived": np.where(consistent, (a >= 0).sum(axis=1), -1).astype(np.int32),
            "remaining_sum": np.where(summable, rem.astype(np.int64).sum(axis=1), -1)}


def path_length_bounds(env, results: dict) -> dict:
    """``bounds_from_lengths`` of the M recorded episodes of ``results`` (``Evaluator.results()`` or
    ``JointEvaluator.results()``, with the env of either kind they came from): one ``path_lengths``
    launch over the recorded start and goal of every agent of every episode, on the grid of the episode's env.  In
    lifelong mode the recorded goal is the agent's last one, so the bound is that of its last leg from the start."""
    M, N = results["starts"].shape[:2]
    if M == 0:
        return bounds_from_lengths(np.zeros((0, N), np.int32))
    ids = np.repeat(np.asarray(results["env"], np.int32), N)
    sp = env.path_lengths(ids, results["starts"].reshape(M * N, 2), results["goals"].reshape(M * N, 2))
    return bounds_from_lengths(sp.cpu().numpy().reshape(M, N))


def table_columns(num_agents: int, lifelong: bool, single_agent: bool = False) -> list:
    """Column names of a result row in the reference's order (main.py:287-319, ``cpu_time`` left out), then ``env``.
    single_agent: the row of the single-agent env, which has one reward -- ``goals_reached_total`` and
    ``blocking_count_total`` (its terminal info) instead of the lifelong columns, no ``agent_i_reward``."""
    cols = ["episode", "seed", "total_reward", "timesteps"]
    if single_agent:
        cols += ["goals_reached_total", "blocking_count_total"]
    elif lifelong:
        cols += ["goals_reached_total", "throughput", "completion_ratio"]
    for i in range(num_agents):
        cols += ([] if single_agent else [f"agent_{i}_reward"]) + [f"agent_{i}_start_x", f"agent_{i}_start_y",
                                                                   f"agent_{i}_goal_x", f"agent_{i}_goal_y"]
    return cols + ["env"]


def results_columns(results: dict, lifelong: bool = False) -> list:
    """``table_columns`` of the table ``results_table(results, lifelong)`` gives: results without ``agent_reward`` are a
    ``JointEvaluator``'s."""
    return table_columns(results["starts"].shape[1], lifelong, single_agent="agent_reward" not in results)


def path_columns(num_agents: int) -> list:
    """The columns ``results_table(..., trace=...)`` appends: those of the reference's planner result files
    (experiments/results/A_star_*.csv, CBS_*.csv) that a path gives."""
    return ["max_steps"] + [f"agent_{i}_{what}" for i in range(num_agents) for what in ("steps", "total_distance")]


def results_table(results: dict, lifelong: bool = False, trace: "Trace | None" = None) -> list:
    """One dict per episode with the reference's column names in the reference's order (main.py:286-324): ``episode``
    (1-based, per env, as each reference run counts its own), ``seed``, ``total_reward``, ``timesteps``, in lifelong
    mode ``goals_reached_total``, ``throughput``, ``completion_ratio``, then per agent ``agent_i_reward``,
    ``agent_i_start_x``, ``agent_i_start_y``, ``agent_i_goal_x``, ``agent_i_goal_y`` -- the reference stores the ROW in
    ``_x`` and the column in ``_y`` (main.py:316-319), and so does this table -- plus ``env``, the index of the env in the
    batch.  ``throughput`` and ``completion_ratio`` are float64 quotients of the integers behind the float32 info columns
    (goals over steps, agents that completed over agents), as the reference computes them.  The reference's ``cpu_time``
    column is left out: it is the process time of the reference's own Python loop and has no meaning for a batched
    device run.  The rows of a single-agent env's results (``JointEvaluator.results()``; ``lifelong`` does not apply) are
    ``episode``, ``seed``, ``total_reward``, ``timesteps``, ``goals_reached_total``, ``blocking_count_total`` (the terminal
    step's info), then per agent the four start / goal columns, then ``env``.  trace: a ``Trace`` of the same evaluation
    (finite mode) -- every row then ends with ``path_columns``: ``max_steps``, and per agent ``agent_i_steps`` and
    ``agent_i_total_distance`` as ``Trace.path_metrics`` counts them, None (an empty CSV field) in the rows of episodes
    that were not traced."""
    single = "agent_reward" not in results
    N = results["starts"].shape[1]
    paths, slot = None, {}
    if trace is not None:
        paths = trace.path_metrics()
        slot = {int(b): k for k, b in reversed(list(enumerate(trace.env_ids)))}  # (a duplicate id: its first region)
    rows = []
    for m in range(len(results["env"])):
        b, steps = int(results["env"][m]), int(results["timesteps"][m])
        row = {"episode": int(results["episode"][m]) + 1, "seed": results["seeds"][b],
               "total_reward": float(results["total_reward"][m]), "timesteps": steps}
        if single:
            row["goals_reached_total"] = float(results["info"][m, SA_INFO_KEYS.index("goals_reached_total")])
            row["blocking_count_total"] = float(results["info"][m, SA_INFO_KEYS.index("blocking_count_total")])
        elif lifelong:
            goals = float(results["info_all"][m, INFO_GOALS_REACHED_TOTAL])
            completed = int(np.rint(float(results["info_all"][m, INFO_COMPLETION_RATIO]) * N))
            row["goals_reached_total"] = goals
            row["throughput"] = goals / float(max(steps, 1))
            row["completion_ratio"] = completed / float(N)
        for i in range(N):
            if not single:
                row[f"agent_{i}_reward"] = float(results["agent_reward"][m, i])
            row[f"agent_{i}_start_x"] = int(results["starts"][m, i, 0])
            row[f"agent_{i}_start_y"] = int(results["starts"][m, i, 1])
            row[f"agent_{i}_goal_x"] = int(results["goals"][m, i, 0])
            row[f"agent_{i}_goal_y"] = int(results["goals"][m, i, 1])
        row["env"] = b
        if paths is not None:
            k, v = slot.get(b), int(results["episode"][m])
            have = k is not None and v < paths["steps"].shape[1] and paths["max_steps"][k, v] >= 0
            row["max_steps"] = int(paths["max_steps"][k, v]) if have else None
            for i in range(N):
                row[f"agent_{i}_steps"] = int(paths["steps"][k, v, i]) if have else None
                row[f"agent_{i}_total_distance"] = int(paths["total_distance"][k, v, i]) if have else None
        rows.append(row)
    return rows


def summary(results: dict, lifelong: bool = False) -> dict:
    """What the reference prints after its loop (main.py:326-338): ``average reward``, ``average timesteps`` and
    ``success rate`` (finite mode: terminated and not truncated; lifelong mode: the mean completion ratio), in lifelong
    mode also the means of ``goals_reached_total``, ``throughput`` and ``completion_ratio``."""
    table = results_table(results, lifelong)
    n = len(table)
    if n == 0:
        return {"episodes": 0}
    out = {"episodes": n, "average reward": sum(r["total_reward"] for r in table) / n,
           "average timesteps": sum(r["timesteps"] for r in table) / n}
    if lifelong:
        out["success rate"] = float(np.mean([r["completion_ratio"] for r in table]))
        for k in ("goals_reached_total", "throughput", "completion_ratio"):
            out["average " + k] = float(np.mean([r[k] for r in table]))
    else:
        out["success rate"] = float(np.mean((results["terminated"] & ~results["truncated"]).astype(np.float64)))
    return out


def write_trace_outputs(trace: "Trace | None", output_dir, stem: str, video: bool = False, trajectories: bool = False,
                        fps: int = 5, hold: int = 3, cell_px: int = 32) -> dict:
    """What the evaluation scripts write of a trace next to their CSV: ``<stem>_trajectories.npz`` (``Trace.save``) and
    ``videos/<stem>.gif`` (``Trace.write_gif``; main.py:342-347 writes its GIF into a ``videos`` folder too).  Returns
    ``{"video": path or None, "trajectories": path or None}``."""
    from pathlib import Path

    out = {"video": None, "trajectories": None}
    if trace is None:
        return out
    output_dir = Path(output_dir)
    if trajectories:
        out["trajectories"] = output_dir / f"{stem}_trajectories.npz"
        trace.save(out["trajectories"])
        print(f"Trajectories saved to {out['trajectories']}")
    if video:
        out["video"] = output_dir / "videos" / f"{stem}.gif"
        out["video"].parent.mkdir(parents=True, exist_ok=True)
        n = trace.write_gif(out["video"], fps=fps, hold=hold, cell_px=cell_px)
        print(f"Saved evaluation video to {out['video']} ({n} frames)")
    return out


def write_results_csv(path, table: list) -> None:
    """The table as CSV, header = the keys of its rows in order (what ``DataFrame.to_csv(index=False)`` writes at
    main.py:362, without pandas).  Floats are written with ``repr``, so reading them back gives the same float64."""
    with open(path, "w", encoding="utf-8", newline="") as f:
        if not table:
            return
        w = csv.DictWriter(f, fieldnames=list(table[0].keys()))
        w.writeheader()
        for row in table:
            w.writerow({k: ("" if v is None else repr(v) if isinstance(v, float) else v) for k, v in row.items()})
