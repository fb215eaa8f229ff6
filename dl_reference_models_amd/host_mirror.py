"""What the two vector adapters share (``vector_env``, ``vector_env_single_agent``): the pinned host mirror of an engine's
per-step outputs, and the adapter base with the lazily fetched row state and the rgb_array frames."""

from __future__ import annotations

import numpy as np
import torch

from .engine_handle import RENDER_CELL_PX


class HostMirror:
    """Host copies of an engine's observations (``_obs``) and of its blob of small outputs (``_out_blob``), pinned where a
    GPU is present, and NumPy views of the blob's sections: a vector step costs two device->host copies and one sync."""

    def __init__(self, engine):
        self._engine = engine
        pin = (lambda t: t.pin_memory()) if torch.cuda.is_available() else (lambda t: t)
        self._h_obs = pin(torch.empty(tuple(engine._obs.shape), dtype=torch.float32))
        self._h_blob = pin(torch.empty(tuple(engine._out_blob.shape), dtype=torch.uint8))

    def view(self, device_tensor: torch.Tensor, dtype) -> np.ndarray:
        """The mirror's bytes of ``device_tensor`` (a section of the engine's blob) as a NumPy array of its shape."""
        off = device_tensor.data_ptr() - self._engine._out_blob.data_ptr()
        nbytes = device_tensor.numel() * device_tensor.element_size()
        return self._h_blob.numpy()[off:off + nbytes].view(dtype).reshape(tuple(device_tensor.shape))

    def fetch(self, want_small: bool = True) -> np.ndarray:
        """Device -> host: the observations (+ the blob of small outputs, which the views then show), one sync.  Returns
        the observations as a new array."""
        e = self._engine
        self._h_obs.copy_(e._obs, non_blocking=True)
        if want_small:
            self._h_blob.copy_(e._out_blob, non_blocking=True)
        torch.cuda.current_stream(e.device).synchronize()
        return self._h_obs.numpy().copy()


def render_vector_frames(vec) -> np.ndarray:
    """Frames of every row of a vector adapter: one launch into a device buffer, one copy into a pinned mirror (both made
    on first use and kept), then a new host array [num_envs, H*32, W*32, 3] for the caller."""
    eng = vec._engine
    if vec._render_bufs is None:
        H, W = eng.grid_shape
        shape = (vec.num_envs, H * RENDER_CELL_PX, W * RENDER_CELL_PX, 3)
        vec._render_bufs = (torch.empty(shape, dtype=torch.uint8, device=eng.device),
                            torch.empty(shape, dtype=torch.uint8).pin_memory())
    dev, host = vec._render_bufs
    eng.render(None, RENDER_CELL_PX, out=dev)
    host.copy_(dev, non_blocking=True)
    torch.cuda.current_stream(eng.device).synchronize()
    return host.numpy().copy()


class VectorAdapter:
    """Base of the vector adapters: ``num_envs`` rows (``envs``) of ONE engine handle (``_engine``, given to ``_attach``)."""

    def __init__(self, cfg: dict, num_envs: int):
        self.num_envs = int(num_envs)
        if self.num_envs < 1:
            raise ValueError("num_envs must be >= 1")
        self.render_mode = cfg.get("render_mode", None)
        if self.render_mode not in (None, "rgb_array"):
            raise ValueError(f"render_mode must be None or 'rgb_array', got {self.render_mode!r}")
        self._render_bufs = None
        self._state_cache = None  # set to None again by whatever changes the engine's state

    def _attach(self, engine) -> None:
        self._engine = engine
        self.device = engine.device
        self._mirror = HostMirror(engine)

    def _state(self):
        """One batched ``get_state``, fetched on first use, at most once per vector step."""
        if self._state_cache is None:
            self._state_cache = self._engine.get_state()
        return self._state_cache

    def get_sub_environments(self):
        return self.envs

    def render(self):
        """gymnasium ``VectorEnv.render``: None unless the env_config set ``render_mode`` to ``"rgb_array"``; then a tuple
        of ``num_envs`` new uint8 [H*32, W*32, 3] frames (one launch, one device->host copy into a pinned buffer).  A row
        that finished shows its terminal state until the ``step`` that resets it."""
        if self.render_mode is None:
            return None
        return tuple(render_vector_frames(self))
