"""What the device networks share on the Python side (policy.py, dqn.py, learner.py, rollout.py): the small ctypes
helpers, the checkpoint format of the torch modules, the base of the three device policies and the launch / capture /
replay of a rollout fragment.  csrc/mapf_nn.h is the same for the kernels.

A new network writes its own torch module (``Checkpoint`` + ``KIND``), its ``DeviceNet`` subclass (constructor, tensors,
``reset_state``, ``act_raw``, ``act``) and, for a rollout, a ``GraphedFragment`` with its slabs and its ``_launch``.
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .engine_handle import _raw_stream


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream_of(device) -> C.c_void_p:
    """The current stream of a cuda device, as the C ABI takes it."""
    return C.c_void_p(_raw_stream(int(device.index)))


def cuda_device(device, who: str) -> torch.device:
    device = torch.device(device)
    if device.type != "cuda":
        raise ValueError(f"{who} runs on the GPU only (there is no CPU path)")
    return torch.device("cuda", torch.cuda.current_device()) if device.index is None else device


def f32c(t):
    return t.detach().to(torch.float32).contiguous()


def check_rc(rc: int, what: str) -> None:
    if rc != L.MAPF_OK:
        raise (ValueError if rc == L.MAPF_ERR_CONFIG else RuntimeError)(f"{what} failed (code {rc})")


class Checkpoint:
    """Mixin of a torch module with ``config()``: the flat parameter vector its device handle takes and a checkpoint file
    that says its ``KIND``, so that ``load`` of another class names the class that reads it.  A class is entered into
    the table when it is defined; ``LOADER`` is how the message spells its ``load`` (default ``<class>.load``)."""

    KIND = None
    LOADER = None
    DEFAULT_KIND = "masked_recurrent"  # files from before the key existed are this kind
    _loaders: dict = {}                # kind -> the spelling of the class method that reads it

    def __init_subclass__(cls, **kwargs):
        super().__init_subclass__(**kwargs)
        if cls.__dict__.get("KIND"):
            Checkpoint._loaders[cls.KIND] = cls.__dict__.get("LOADER") or f"{cls.__name__}.load"

    def flat_params(self) -> torch.Tensor:
        """The parameter vector ``mapf_*_set_params`` takes: every tensor of ``state_dict()`` in its order, flattened."""
        return torch.cat([v.detach().reshape(-1).to(torch.float32) for v in self.state_dict().values()])

    def save(self, path) -> None:
        torch.save({"kind": self.KIND, "config": self.config(), "state_dict": self.state_dict()}, path)

    @classmethod
    def load(cls, path, map_location="cpu"):
        blob = torch.load(path, map_location=map_location, weights_only=True)
        cls._check_kind(blob, path)
        m = cls(**blob["config"])
        m.load_state_dict(blob["state_dict"])
        return m

    @classmethod
    def _check_kind(cls, blob, path) -> None:
        kind = blob.get("kind", Checkpoint.DEFAULT_KIND)
        if kind != cls.KIND:
            raise ValueError(f"{path} is a checkpoint of kind '{kind}'; {cls.__name__}.load reads kind '{cls.KIND}' "
                             f"(load it with {Checkpoint._loaders.get(kind, 'the class that wrote it')})")


class DeviceNet:
    """The base of ``DevicePolicy``, ``JointDevicePolicy`` and ``DeviceQPolicy``: one handle of the C ABI family ``prefix``
    (``mapf_policy``, ``mapf_jpolicy``, ``mapf_qnet``) on one device, its parameter staging vector and the pieces every
    ``act`` shares.  A subclass resolves its module (``_module``) and its shapes (``rows`` among them), calls ``_create``
    with its config struct, allocates its own tensors and calls ``load_params``."""

    @staticmethod
    def _module(module_cls, module_or_path, needs: str | None = None):
        module = module_cls.load(module_or_path) if not isinstance(module_or_path, torch.nn.Module) else module_or_path
        if needs is not None and not isinstance(module, module_cls):
            raise TypeError(needs)
        return module

    def __init__(self, prefix: str, device):
        self._prefix = prefix
        self.device = cuda_device(device, type(self).__name__)

    def _create(self, cfg, module, create: str | None = None, extra=()) -> None:
        """create: the symbol that makes the handle, default ``<prefix>_create``; extra: its arguments between the config and
        the handle."""
        create = create or self._prefix + "_create"
        self._lib = L.load()
        self._h = C.c_void_p()
        rc = getattr(self._lib, create)(C.byref(cfg), *extra, C.byref(self._h))
        if rc != L.MAPF_OK:
            raise ValueError(f"{create} refused the configuration {module.config()} (code {rc})")
        count = int(getattr(self._lib, self._prefix + "_param_count")(self._h))
        self._params = torch.zeros((count,), dtype=torch.float32, device=self.device)
        self._act_fn = getattr(self._lib, self._prefix + "_act")

    def _stream(self):
        return stream_of(self.device)

    def _check(self, rc: int, what: str):
        check_rc(rc, what)

    def load_params(self, module) -> None:
        """The module's current weights, asynchronously on the current stream: one copy into the policy's staging vector and
        one repacking launch."""
        flat = module.flat_params()
        if flat.numel() != self._params.numel():
            raise ValueError(f"the module has {flat.numel()} parameters, the policy handle takes {self._params.numel()}")
        self._params.copy_(flat, non_blocking=True)
        what = self._prefix + "_set_params"
        self._check(getattr(self._lib, what)(self._h, ptr(self._params), self._params.numel(), self._stream()), what)

    def _act(self, before_seed, seed: int, mode: int, after_mode, stream) -> None:
        """``<prefix>_act(handle, rows, *before_seed, seed, mode, *after_mode, stream)``, default the current stream."""
        rc = self._act_fn(self._h, self.rows, *before_seed, C.c_uint64(int(seed) & (2**64 - 1)), int(mode), *after_mode,
                          stream if stream is not None else self._stream())
        if rc != L.MAPF_OK:
            self._check(rc, self._prefix + "_act")

    def _input(self, t, dtype, n, name):
        if t is None:
            return None
        if t.dtype != dtype or t.device != self.device or not t.is_contiguous():
            t = t.to(device=self.device, dtype=dtype).contiguous()
        if t.numel() != n:
            raise ValueError(f"{name} must have {n} elements, got {tuple(t.shape)}")
        return t

    def close(self) -> None:
        if getattr(self, "_h", None):
            getattr(self._lib, self._prefix + "_destroy")(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class GraphedFragment:
    """``collect()`` of a rollout: the first call runs ``_launch()``, the second synchronises and captures it into a graph,
    every later one replays the graph.  The owner sets ``env``, ``_out`` (what ``collect`` returns), ``_graph = None`` and
    ``_calls = 0``."""

    def collect(self) -> dict:
        if self._calls == 0:
            self._launch()
        else:
            if self._graph is None:
                torch.cuda.synchronize(self.env.device)
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g):
                    self._launch()
                self._graph = g
            self._graph.replay()
        self._calls += 1
        return self._out
