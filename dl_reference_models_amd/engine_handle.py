"""What the two batched wrappers of a ``mapf_*`` handle share (``VecReferenceModel``, ``VecSingleAgentReferenceModel``):
the rules that turn an ``env_config`` into what the C ABI takes (seeds, grids, fixed tables, the layout of the blob of small
outputs) as pure functions that need neither the native library nor a GPU, and ``EngineHandle``, the base class that owns
the handle itself."""

from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _lib as L
from . import get_grid as grid_tables


def pcg64_words(seed) -> np.ndarray:
    """uint64[6] PCG64 state of ``np.random.default_rng(seed)`` (SeedSequence expansion stays in NumPy)."""
    st = np.random.default_rng(seed).bit_generator.state
    s, inc = int(st["state"]["state"]), int(st["state"]["inc"])
    m = (1 << 64) - 1
    return np.array([s >> 64, s & m, inc >> 64, inc & m, int(st["has_uint32"]), int(st["uinteger"])], dtype=np.uint64)


def config_seeds(cfg: dict, num_envs: int) -> list:
    """The NumPy seed of every env: ``seeds`` as given, else ``seed + b``, else None (OS entropy) for each.  ``rng_words``
    is not looked at here: where it is given it replaces the streams these seeds would start (``config_rng_words``)."""
    seeds = cfg.get("seeds", None)
    if seeds is None:
        seed = cfg.get("seed", None)
        seeds = [None] * num_envs if seed is None else [int(seed) + b for b in range(num_envs)]
    if len(seeds) != num_envs:
        raise ValueError("need one seed per env")
    return list(seeds)


def config_rng_words(cfg: dict, num_envs: int) -> np.ndarray:
    """uint64 [B,6]: one NumPy PCG64 stream per env (MA-env:74-78), ``rng_words`` if given, else those of ``config_seeds``."""
    if cfg.get("rng_words", None) is not None:
        return np.ascontiguousarray(cfg["rng_words"], dtype=np.uint64).reshape(num_envs, 6)
    return np.stack([pcg64_words(s) for s in config_seeds(cfg, num_envs)])


def config_grids(cfg: dict, num_envs: int):
    """``(grids uint8 [K,H,W], shared)``: ``grid`` ([H,W]: K = 1, shared by every env; or [num_envs,H,W]), default the
    named grid ``env_name``."""
    grid = cfg.get("grid", None)
    if grid is None:
        grid = grid_tables.get_grid(cfg["env_name"])
    grid = np.ascontiguousarray(grid, dtype=np.uint8)
    if grid.ndim == 2:
        return grid[None], 1
    if grid.ndim == 3 and grid.shape[0] == num_envs:
        return grid, 0
    raise ValueError("grid must be [H,W] or [num_envs,H,W]")


def config_fixed_tables(cfg: dict, num_agents: int, num_envs: int):
    """``(starts, goals)`` int16 [B,N,2] of a ``deterministic`` env (MA-env:124-132, SA-env:109-112): ``fixed_starts`` /
    ``fixed_goals`` ([N,2] or [B,N,2]) or, without both, the tables of the named grid."""
    N = num_agents
    fs, fg = cfg.get("fixed_starts", None), cfg.get("fixed_goals", None)
    if fs is None or fg is None:
        s = grid_tables.get_start_positions(cfg["env_name"], N)
        g = grid_tables.get_goal_positions(cfg["env_name"], N)
        fs = np.array([s[f"agent_{i}"] for i in range(N)], dtype=np.int16)
        fg = np.array([g[f"agent_{i}"] for i in range(N)], dtype=np.int16)
    return tuple(np.ascontiguousarray(np.broadcast_to(np.asarray(t, np.int16).reshape(-1, N, 2), (num_envs, N, 2)))
                 for t in (fs, fg))


def section_layout(shapes):
    """``(offsets, sizes, total)`` in bytes of the sections ``(name, shape, torch dtype)`` packed into one allocation, each
    starting on a multiple of 256."""
    sizes = [int(np.prod(shape)) * torch.empty((), dtype=dt).element_size() for _, shape, dt in shapes]
    offs, total = [], 0
    for sz in sizes:
        offs.append(total)
        total += (sz + 255) & ~255
    return offs, sizes, total


def alloc_sections(shapes, device):
    """``(blob, {name: view})``: one zeroed uint8 allocation on ``device`` and a typed view of each section in it."""
    offs, sizes, total = section_layout(shapes)
    blob = torch.zeros((total,), dtype=torch.uint8, device=device)
    return blob, {name: blob[off:off + sz].view(dt).view(shape) for (name, shape, dt), off, sz in zip(shapes, offs, sizes)}


def metrics_from_sums(s, num_agents: int, lifelong: bool) -> dict:
    """Means over finished episodes from the int64 accumulator vector (exact rational arithmetic in float64)."""
    n = float(s[L.ACC_EPISODES])
    if n == 0:
        return {"episodes": 0}
    m = {
        "episodes": int(s[L.ACC_EPISODES]),
        "goals_reached": s[L.ACC_GOALS_REACHED] / n,
        "blocking_count": s[L.ACC_BLOCKING_COUNT] / n,
        "deadlock_count": s[L.ACC_DEADLOCK_COUNT] / n,
        "livelock_count": s[L.ACC_LIVELOCK_COUNT] / n,
        "deadlock_steps": s[L.ACC_DEADLOCK_STEPS] / n,
        "livelock_steps": s[L.ACC_LIVELOCK_STEPS] / n,
        "episode_len_mean": s[L.ACC_EPISODE_STEPS] / n,
    }
    completion = s[L.ACC_COMPLETED_AGENTS] / (n * num_agents)
    if lifelong:  # SuccessRateCallback logs the completion ratio as success in lifelong mode (callbacks.py:150-155)
        m["success_rate"] = completion
        m["completion_ratio"] = completion
        # every lifelong episode runs to the step limit, so the mean of goals/steps is the ratio of the sums
        m["throughput"] = s[L.ACC_GOALS_REACHED] / max(float(s[L.ACC_EPISODE_STEPS]), 1.0)
    else:
        m["success_rate"] = s[L.ACC_SUCCESSES] / n
    return m


# the current stream's raw handle without building a torch.cuda.Stream object per call (0.5 us of a 7 us Python step)
_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None) or (lambda idx: torch.cuda.current_stream(idx).cuda_stream)

# pixels per grid cell of an rgb_array frame wherever the caller passes no size (facades, rows, vector adapters)
RENDER_CELL_PX = 32


def render_frames(eng, env_ids=None, cell_px: int = RENDER_CELL_PX, out: torch.Tensor | None = None) -> torch.Tensor:
    """``EngineHandle.render``: uint8 [K, H*c, W*c, 3] frames of the envs ``env_ids`` (mapf_render; include/mapf_step.h
    states the raster rule), enqueued on the current stream, no sync.

    env_ids: None (every env), a host sequence / numpy array (checked here: ValueError), or a device int32 tensor (passed
    through as it is: an id outside [0, B) gives a zero frame and is reported by ``poll_error``).  out: a preallocated
    contiguous uint8 tensor of the frames' shape on the engine's device; with it and env_ids None or on the device the
    call allocates nothing and can be captured in a graph."""
    B = eng.num_envs
    H, W = eng.grid_shape
    c = int(cell_px)
    if not L.RENDER_MIN_CELL_PX <= c <= L.RENDER_MAX_CELL_PX:
        raise ValueError(f"cell_px must lie in [{L.RENDER_MIN_CELL_PX}, {L.RENDER_MAX_CELL_PX}], got {cell_px}")
    ids = None
    if env_ids is None:
        K = B
    elif isinstance(env_ids, torch.Tensor) and env_ids.device.type != "cpu":
        if env_ids.dtype != torch.int32 or env_ids.device != eng.device or env_ids.dim() != 1 or not env_ids.is_contiguous():
            raise ValueError(f"a device env_ids must be a contiguous 1-D int32 tensor on {eng.device}")
        ids, K = env_ids, int(env_ids.numel())
    else:
        a = np.asarray(env_ids.numpy() if isinstance(env_ids, torch.Tensor) else env_ids)
        if a.ndim != 1 or a.size == 0 or not np.issubdtype(a.dtype, np.integer):
            raise ValueError("env_ids must be a non-empty 1-D sequence of integers")
        if a.min() < 0 or a.max() >= B:
            raise ValueError(f"env_ids must lie in [0, {B})")
        ids, K = torch.from_numpy(a.astype(np.int32)).to(eng.device), int(a.size)
    if K < 1:
        raise ValueError("env_ids must not be empty")
    shape = (K, H * c, W * c, 3)
    if out is None:
        out = torch.empty(shape, dtype=torch.uint8, device=eng.device)
    elif tuple(out.shape) != shape or out.dtype != torch.uint8 or out.device != eng.device or not out.is_contiguous():
        raise ValueError(f"out must be a contiguous uint8 tensor of shape {shape} on {eng.device}")
    rc = eng._lib.mapf_render(eng._h, None if ids is None else C.c_void_p(ids.data_ptr()), K, c, C.c_void_p(out.data_ptr()),
                              eng._stream())
    eng._check(rc, ValueError)
    return out


class EngineHandle:
    """One ``mapf_*`` handle and what every wrapper of one does with it.  A subclass builds its ``MapfConfig`` and calls, in
    this order, ``_open``, ``_upload_config``, ``_alloc_outputs`` and ``_place``; it sets ``_reset_fn`` (its reset entry
    point) before ``_place`` and ``lifelong_mapf`` where its env has that mode."""

    lifelong_mapf = False

    def __init__(self, env_config: dict):
        cfg = dict(env_config)
        self.env_config = cfg
        self._lib = L.load()  # raises if the HIP library is not built: no CPU fallback
        self.device = torch.device(cfg.get("device", "cuda:0"))
        if self.device.type != "cuda":
            raise ValueError(f"{type(self).__name__} runs on a HIP device only (device='cuda:N')")
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self._dev_index = int(self.device.index)
        self.num_envs = int(cfg.get("num_envs", 1))
        self.num_agents = int(cfg.get("num_agents", 2))
        self.steps_per_episode = int(cfg.get("steps_per_episode", 100))
        self.deterministic = bool(cfg.get("deterministic", False))
        self.grids, self._shared_grid = config_grids(cfg, self.num_envs)
        self.grid_shape = (int(self.grids.shape[1]), int(self.grids.shape[2]))

    def _open(self, c: L.MapfConfig) -> None:
        self._cfg = c
        self.obs_len = int(self._lib.mapf_obs_len(C.byref(c)))
        h = C.c_void_p()
        rc = self._lib.mapf_create(C.byref(c), C.byref(h))
        if rc != L.MAPF_OK:
            raise ValueError(f"mapf_create failed ({rc}): {self._lib.mapf_last_error(None).decode()}")
        self._h = h

    def _upload_config(self) -> None:
        """The grids and one PCG64 stream per env."""
        self._check(self._lib.mapf_set_grids(self._h, self.grids.ctypes.data_as(C.c_void_p), self._shared_grid), ValueError)
        words = config_rng_words(self.env_config, self.num_envs)
        self._check(self._lib.mapf_set_rng_state(self._h, words.ctypes.data_as(C.c_void_p)))

    def _alloc_outputs(self, obs_shape, sections) -> None:
        """``_obs`` / ``_final_obs`` and, as attributes named by ``sections``, the small per-step outputs.  Those live in ONE
        allocation, ``_out_blob`` (256-byte aligned sections): a wave's stores to them then share address translations
        instead of touching separately mapped tensors, and a host mirror of them is one copy (host_mirror.HostMirror)."""
        with torch.cuda.device(self.device):
            self._obs = torch.zeros(obs_shape, dtype=torch.float32, device=self.device)
            self._final_obs = torch.zeros(obs_shape, dtype=torch.float32, device=self.device)
            self._out_blob, views = alloc_sections(sections, self.device)
        for name, t in views.items():
            setattr(self, name, t)

    def _place(self) -> None:
        """What the reference ctor does about positions: the fixed start/goal tables of a ``deterministic`` env, else one
        ``generate_starts_goals()`` draw (MA-env:124-134, SA-env:109-114: same RNG consumption)."""
        if self.deterministic:
            fs, fg = config_fixed_tables(self.env_config, self.num_agents, self.num_envs)
            self._check(self._lib.mapf_set_fixed_starts_goals(
                self._h, fs.ctypes.data_as(C.c_void_p), fg.ctypes.data_as(C.c_void_p)), ValueError)
        else:
            self._check(self._reset_fn(self._h, None, None, self._stream()))

    # ------------------------------------------------------------------------------------------
    def _stream(self):
        return C.c_void_p(_raw_stream(int(self.device.index)))

    def _check(self, rc: int, exc=RuntimeError):
        if rc != L.MAPF_OK:
            raise exc(f"{self._lib.mapf_last_error(self._h).decode()} (code {rc})")

    def close(self):
        if getattr(self, "_h", None):
            self._lib.mapf_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _launch_shape(self, fn):
        """``(fn's return value, blocks, threads, lds_bytes, lanes_per_env)`` of a ``mapf_*launch_info`` entry point."""
        out = [C.c_int32() for _ in range(4)]
        rv = fn(self._h, *(C.byref(v) for v in out))
        return (int(rv), *(v.value for v in out))

    def _int8_actions(self, actions: torch.Tensor, shape) -> torch.Tensor:
        """``actions`` as a contiguous int8 tensor on the handle's device, of ``shape`` (a leading None: any T)."""
        if actions.dtype != torch.int8 or actions.device != self.device or not actions.is_contiguous():
            actions = actions.to(device=self.device, dtype=torch.int8).contiguous()
        if actions.dim() != len(shape) or any(s is not None and s != a for s, a in zip(shape, actions.shape)):
            raise ValueError(f"actions must have shape ({', '.join('T' if s is None else str(s) for s in shape)})")
        return actions

    def _env_mask(self, env_mask: torch.Tensor) -> torch.Tensor:
        """``env_mask`` as a contiguous uint8 [B] tensor on the handle's device."""
        env_mask = env_mask.to(device=self.device, dtype=torch.uint8).contiguous()
        if tuple(env_mask.shape) != (self.num_envs,):
            raise ValueError(f"env_mask must have shape {(self.num_envs,)}")
        return env_mask

    # ------------------------------------------------------------------------------------------
    def reset(self, env_mask: torch.Tensor | None = None) -> torch.Tensor:
        """reset() of every env (or those with env_mask != 0).  Returns the observation tensor (device)."""
        mptr = None
        if env_mask is not None:
            env_mask = env_mask.to(device=self.device, dtype=torch.uint8).contiguous()
            mptr = C.c_void_p(env_mask.data_ptr())
        self._check(self._reset_fn(self._h, mptr, C.c_void_p(self._obs.data_ptr()), self._stream()))
        return self._obs

    def debug_hints(self) -> np.ndarray:
        """Diagnostic: the engine-internal "may finish in the next step" hint of every env, int32 [B] (``get_state`` reports
        0 for it).  Synchronizes the device."""
        out = np.zeros(self.num_envs, np.int32)
        self._check(self._lib.mapf_debug_hints(self._h, out.ctypes.data_as(C.c_void_p)))
        return out

    def render(self, env_ids=None, cell_px: int = RENDER_CELL_PX, out: torch.Tensor | None = None) -> torch.Tensor:
        """rgb_array frames uint8 [K, H*cell_px, W*cell_px, 3] of the envs ``env_ids`` (default all) from the current state,
        on the device, enqueued on the current stream (no sync); ``render_frames`` says what ``env_ids`` / ``out`` take.
        The single-agent env's frames have no sensor windows (SA-env draws none)."""
        return render_frames(self, env_ids, cell_px, out)

    # ---- shortest-path planner (mapf_expert_actions / mapf_path_lengths / mapf_distance_field: include/mapf_step.h
    # states the rule).  Device tensors in and out, one launch on the current stream each, nothing synchronized.
    def _device_array(self, x, dtype: torch.dtype, shape, name: str) -> torch.Tensor:
        """``x`` (a tensor, array or sequence) as a contiguous ``dtype`` tensor of ``shape`` on the handle's device."""
        t = torch.as_tensor(x).to(device=self.device, dtype=dtype).contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name} must have shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _plan_queries(self, env_ids, cells: dict):
        ids = torch.as_tensor(env_ids).to(device=self.device, dtype=torch.int32).contiguous()
        if ids.dim() != 1 or ids.numel() < 1:
            raise ValueError("env_ids must be a non-empty 1-D sequence")
        K = int(ids.numel())
        return ids, K, [self._device_array(v, torch.int16, (K, 2), k) for k, v in cells.items()]

    def expert_actions(self, mode: str = "yielding", out: torch.Tensor | None = None, return_distance: bool = False):
        """The shortest-path expert's action of every agent from the current state: int8 [B, N] (``out`` if given).
        ``"independent"``: the lowest action id that shortens the agent's path to its goal; ``"yielding"``: the same
        without the cells other agents stand on, 0 (wait) when none is left.  With ``return_distance`` also the agents'
        path lengths, int32 [B, N] (-1: goal unreachable), as ``(actions, distance)``."""
        modes = {"independent": 0, "yielding": 1}
        if mode not in modes:
            raise ValueError(f"mode must be one of {sorted(modes)}, got {mode!r}")
        shape = (self.num_envs, self.num_agents)
        if out is None:
            out = torch.empty(shape, dtype=torch.int8, device=self.device)
        elif tuple(out.shape) != shape or out.dtype != torch.int8 or out.device != self.device or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int8 tensor of shape {shape} on {self.device}")
        dist = torch.empty(shape, dtype=torch.int32, device=self.device) if return_distance else None
        self._check(self._lib.mapf_expert_actions(self._h, modes[mode], C.c_void_p(out.data_ptr()),
                                                  None if dist is None else C.c_void_p(dist.data_ptr()), self._stream()), ValueError)
        return (out, dist) if return_distance else out

    def path_lengths(self, env_ids, src, dst) -> torch.Tensor:
        """int32 [K]: the shortest-path length from ``src[k]`` to ``dst[k]`` ((row, col), [K, 2]) on the grid of env
        ``env_ids[k]``, -1 where there is no path or a cell is an obstacle or outside the grid.  An env id outside
        [0, B) leaves its element unwritten and is reported by ``poll_error``."""
        ids, K, (s, d) = self._plan_queries(env_ids, {"src": src, "dst": dst})
        out = torch.empty((K,), dtype=torch.int32, device=self.device)
        self._check(self._lib.mapf_path_lengths(self._h, K, C.c_void_p(ids.data_ptr()), C.c_void_p(s.data_ptr()),
                                                C.c_void_p(d.data_ptr()), C.c_void_p(out.data_ptr()), self._stream()), ValueError)
        return out

    def distance_field(self, env_ids, dst) -> torch.Tensor:
        """uint16 [K, H, W]: the path length of every cell of env ``env_ids[k]`` to ``dst[k]``, 0xFFFF where there is none
        (obstacles included): the heuristic channel of PRIMAL-style observations."""
        ids, K, (d,) = self._plan_queries(env_ids, {"dst": dst})
        out = torch.empty((K, *self.grid_shape), dtype=torch.uint16, device=self.device)
        self._check(self._lib.mapf_distance_field(self._h, K, C.c_void_p(ids.data_ptr()), C.c_void_p(d.data_ptr()),
                                                  C.c_void_p(out.data_ptr()), self._stream()), ValueError)
        return out

    def _plan_outputs(self, spec: dict, out, mask, keyed: bool = False):
        """What a joint planner's call writes and whom it plans: ``(tensors, mask pointer)``.  spec: name -> (shape, dtype)
        in the order of the call's arguments.  out: None (the tensors are allocated), or the caller's tensors -- a sequence
        in spec's order, with ``keyed`` a dict with spec's names -- each a contiguous tensor of its shape and dtype on the
        handle's device (ValueError otherwise).  mask: None or what ``_env_mask`` takes."""
        if out is None:
            tensors = [torch.empty(shape, dtype=dt, device=self.device) for shape, dt in spec.values()]
        elif keyed:
            if not isinstance(out, dict) or set(out) != set(spec):
                raise ValueError(f"out must be a dict with the keys {sorted(spec)}")
            tensors = [out[name] for name in spec]
        else:
            if not isinstance(out, (tuple, list)) or len(out) != len(spec):
                raise ValueError(f"out must be a {'pair' if len(spec) == 2 else 'triple'} ({', '.join(spec)})")
            tensors = list(out)
        for t, (name, (shape, dt)) in zip(tensors, spec.items()):
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != dt or t.device != self.device \
                    or not t.is_contiguous():
                raise ValueError(f"out's {name} must be a contiguous {dt} tensor of shape {shape} on {self.device}")
        self._plan_mask = None if mask is None else self._env_mask(mask)  # (kept: the launch reads it)
        return tensors, None if mask is None else C.c_void_p(self._plan_mask.data_ptr())

    # ---- prioritised planner (mapf_plan_prioritized: include/mapf_step.h states the rule)
    @property
    def plan_max_horizon(self) -> int:
        """The longest horizon ``plan_prioritized`` takes on this handle (MAPF_PLAN_MAX_HORIZON of its grid height)."""
        return int(self._lib.mapf_plan_max_horizon(self._h))

    def plan_prioritized(self, horizon: int | None = None, mask: torch.Tensor | None = None, out=None):
        """One collision-free joint plan per env from the current state, the agents planned one after another in the order
        the env moves them: ``(plan int8 [B, horizon, N], arrival int32 [B, N])`` on the device, one launch on the current
        stream, no sync.  ``plan[b, t]`` are the actions of step t; ``arrival[b, j]`` is the step after which agent j
        stands on its goal for good, -1 where the planner found no path for it within the horizon (its actions are all 0).
        An env whose arrivals are all >= 0 is solved: stepping it with ``plan[b, 0], plan[b, 1], ...`` no move fails
        (``evaluation.plan_costs`` gives solved, sum-of-costs and makespan).  horizon: default
        ``min(steps_per_episode, plan_max_horizon)``.  mask: uint8 [B], only envs with a non-zero byte are planned and
        written.  out: ``(plan, arrival)`` to write into; with it, and after a first call with the same horizon, the call
        allocates nothing and can be captured in a graph."""
        limit = self.plan_max_horizon
        T = min(self.steps_per_episode, limit) if horizon is None else int(horizon)
        if not 1 <= T <= limit:
            raise ValueError(f"horizon must lie in [1, {limit}], got {horizon}")
        B, N = self.num_envs, self.num_agents
        (plan, arrival), mptr = self._plan_outputs({"plan": ((B, T, N), torch.int8), "arrival": ((B, N), torch.int32)}, out, mask)
        self._check(self._lib.mapf_plan_prioritized(self._h, T, mptr, C.c_void_p(plan.data_ptr()),
                                                    C.c_void_p(arrival.data_ptr()), self._stream()), ValueError)
        return plan, arrival

    # ---- windowed prioritised planner (mapf_plan_windowed: include/mapf_step.h states the rule)
    @property
    def max_window(self) -> int:
        """The longest window ``plan_windowed`` takes (MAPF_PLAN_MAX_WINDOW)."""
        return int(self._lib.mapf_plan_max_window(self._h))

    def plan_windowed(self, window: int = 16, mask: torch.Tensor | None = None, out=None):
        """The next ``window`` steps of every env planned together from the current state, the agents one after another in
        the order the env moves them, each steering by the distance to its goal: ``(plan int8 [B, window, N], arrival
        int32 [B, N], remaining int32 [B, N])`` on the device, one launch on the current stream, no sync.  ``plan[b, t]``
        are the actions of step t; ``arrival[b, j]`` is the first step of the window after which agent j stands on its
        goal (-1: not within the window); ``remaining[b, j]`` is its path length to the goal at the end of the window, -2
        where the goal cannot be reached, -1 where the planner found no collision-free window for the agent (its actions
        are all 0).  An env without a -1 in ``remaining`` is consistent: stepping it with ``plan[b, 0], plan[b, 1], ...``
        no move fails, in finite and in lifelong mode (``evaluation.window_costs``).  The rolling-horizon planner for
        lifelong mode: play some of the window, call again.  mask: uint8 [B], only envs with a non-zero byte are planned
        and written.  out: ``(plan, arrival, remaining)`` to write into.  The call never allocates on the device and keeps
        nothing in the handle: it can be captured in a graph from the first call, and calls on different streams may
        overlap."""
        limit = self.max_window
        w = int(window)
        if not 1 <= w <= limit:
            raise ValueError(f"window must lie in [1, {limit}], got {window}")
        B, N = self.num_envs, self.num_agents
        spec = {"plan": ((B, w, N), torch.int8), "arrival": ((B, N), torch.int32), "remaining": ((B, N), torch.int32)}
        (plan, arrival, remaining), mptr = self._plan_outputs(spec, out, mask)
        self._check(self._lib.mapf_plan_windowed(self._h, w, mptr, C.c_void_p(plan.data_ptr()), C.c_void_p(arrival.data_ptr()),
                                                 C.c_void_p(remaining.data_ptr()), self._stream()), ValueError)
        return plan, arrival, remaining

    # ---- conflict-based search (mapf_plan_cbs: include/mapf_step.h states the rule)
    def plan_cbs_max_nodes(self) -> int:
        """The largest ``max_nodes`` ``plan_cbs`` takes on this handle at the longest horizon (mapf_plan_cbs_max_nodes)."""
        return int(self._lib.mapf_plan_cbs_max_nodes(self._h))

    def plan_cbs_workspace_bytes(self, horizon: int, max_nodes: int) -> int:
        """Bytes of the node store ``plan_cbs(horizon, max_nodes)`` keeps in the handle (0 for arguments it refuses)."""
        return int(self._lib.mapf_plan_cbs_workspace_bytes(self._h, int(horizon), int(max_nodes)))

    def plan_cbs(self, horizon: int | None = None, max_nodes: int = 256, mask: torch.Tensor | None = None, out=None):
        """Conflict-based search from the current state: per env the joint plan of least sum of costs within ``horizon``
        steps, if the search finds it within ``max_nodes`` nodes.  Returns a dict of device tensors -- ``plan`` int8 [B,
        horizon, N], ``arrival`` int32 [B, N], ``status`` int32 [B] (``_lib.CBS_SOLVED`` / ``CBS_BUDGET`` /
        ``CBS_INFEASIBLE`` / ``CBS_NO_PATH``) and ``nodes`` int32 [B] (nodes created, the root included) -- from one launch
        on the current stream, no sync.  A solved env executes ``plan[b, 0], plan[b, 1], ...`` without a failed move and
        ``arrival[b, j]`` is the step after which agent j stands on its goal for good; every other env has an all-zero
        plan and arrivals of -1 (``evaluation.plan_costs`` takes the arrivals, ``evaluation.cbs_summary`` status and
        nodes).  horizon: default ``min(steps_per_episode, 128)``.  mask: uint8 [B], only envs with a non-zero byte are
        planned and written.  out: a dict with the four tensors to write into; with it, and after a first call that needed
        no smaller node store, the call allocates nothing and can be captured in a graph."""
        T = min(self.steps_per_episode, L.CBS_MAX_HORIZON) if horizon is None else int(horizon)
        M = int(max_nodes)
        if not 1 <= T <= L.CBS_MAX_HORIZON:
            raise ValueError(f"horizon must lie in [1, {L.CBS_MAX_HORIZON}], got {horizon}")
        if not 1 <= M <= L.CBS_MAX_NODES:
            raise ValueError(f"max_nodes must lie in [1, {L.CBS_MAX_NODES}], got {max_nodes}")
        B, N = self.num_envs, self.num_agents
        spec = {"plan": ((B, T, N), torch.int8), "arrival": ((B, N), torch.int32), "status": ((B,), torch.int32),
                "nodes": ((B,), torch.int32)}
        tensors, mptr = self._plan_outputs(spec, out, mask, keyed=True)
        self._check(self._lib.mapf_plan_cbs(self._h, T, M, mptr, *(C.c_void_p(t.data_ptr()) for t in tensors), self._stream()),
                    ValueError)
        return dict(zip(spec, tensors)) if out is None else out

    def episode_sums(self, reset: bool = False) -> np.ndarray:
        """int64[12] sums over all finished episodes of all envs (columns: _lib.ACC_*; the single-agent env has no lock
        metrics, its deadlock / livelock columns stay 0).  Synchronizes the device; ``reset=True`` clears the sums
        afterwards."""
        out = np.zeros(L.NUM_EPISODE_ACC, dtype=np.int64)
        self._check(self._lib.mapf_get_episode_stats(self._h, out.ctypes.data_as(C.c_void_p), 1 if reset else 0))
        return out

    def episode_sums_device(self, out: torch.Tensor | None = None) -> torch.Tensor:
        """The same sums as a device tensor (int64[12]), added up by one small launch on the current stream: no host
        round trip, nothing synchronized, nothing cleared (mapf_episode_stats_async)."""
        if out is None:
            out = torch.empty(L.NUM_EPISODE_ACC, dtype=torch.int64, device=self.device)
        if out.dtype != torch.int64 or out.device != self.device or out.numel() != L.NUM_EPISODE_ACC or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous int64[{L.NUM_EPISODE_ACC}] tensor on {self.device}")
        self._check(self._lib.mapf_episode_stats_async(self._h, C.c_void_p(out.data_ptr()), self._stream()))
        return out

    def episode_metrics(self, reset: bool = False, sums: np.ndarray | None = None) -> dict:
        """Mean per-episode metrics under the names the reference's RLlib callbacks log
        (src/trainers/callbacks.py: success_rate :138-181, goals_reached ... livelock_steps :325-330,
        throughput / completion_ratio :331-335; for the single-agent env goals_reached counts goal_reached_once and the
        lock metrics are the callbacks' 0.0 defaults).  `sums` lets a multi-GPU job pass the all-reduced vector."""
        return metrics_from_sums(self.episode_sums(reset) if sums is None else sums, self.num_agents,
                                 self.lifelong_mapf)

    def _poll(self):
        """``(code, env, agent, value)`` of the latched error record (mapf_poll_error: synchronizes and clears it)."""
        env, agent, value = C.c_int32(-1), C.c_int32(-1), C.c_int32(0)
        rc = self._lib.mapf_poll_error(self._h, self._stream(), C.byref(env), C.byref(agent), C.byref(value))
        return rc, env.value, agent.value, value.value
