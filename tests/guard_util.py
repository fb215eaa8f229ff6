"""Guarded, poisoned output buffers for the tests of the C ABI's WRITE contracts (include/mapf_step.h): where a launch
stores, not only what.

``GuardedBuffer`` is one byte arena laid out  guard | payload | guard.  The whole arena is filled with a poison byte
before a call; afterwards the guards must still hold it (a store outside the caller's buffer lands in memory this test
allocated and is reported, nothing can fault), every element the contract says is written must have lost it, and every
element the contract says is left alone must still hold it.

The poison byte is 0xA5: as float32 about -2.87e-16, as float64 about -1.4e-130, 165 as uint8, -91 as int8, negative as
int16 / int32 / int64 -- nothing an output of the engine can hold.  (Render frames are the exception, a blended channel
can be 165: ``two_fill`` runs such a call with 0xA5 and 0x5A and requires the same payload from both.)

``GuardedEngineStepper`` / ``GuardedCteEngineStepper`` put the raw ``mapf_*`` entry points behind the stepper interface
of trace_util with every output guarded, so compare_steppers / replay_* run through them unchanged, and ``CASES`` is the
table (kernel path -> smallest configuration that reaches it) the contract tests and their oracle-only coverage check
share.
"""

from __future__ import annotations

import ctypes as C
import functools

import numpy as np

from trace_util import CteEngineStepper, EngineStepper, synth_grid

POISON = 0xA5
POISON_ALT = 0x5A
MIN_GUARD = 4096
PAYLOAD_PHASE = 16  # the payload starts at an address that is 16 (mod 256): the ABI asks for 16-byte alignment, no more


def guard_bytes_for(slab_bytes: int) -> int:
    """Bytes of each guard: one whole [B]-slab of the output (a [T+1]-th slab, a workgroup of stray rows), at least 4 KiB,
    rounded up to 256."""
    return (max(MIN_GUARD, int(slab_bytes)) + 255) & ~255


class GuardedBuffer:
    """guard | payload | guard in one uint8 arena; the payload is a typed view of ``shape`` / ``dtype`` (a NumPy dtype).

    device: a torch device ("cuda:0", "cpu") for a torch arena, or "numpy" for a NumPy one (host-pointer outputs)."""

    def __init__(self, shape, dtype, device="cuda:0", guard_bytes: int = MIN_GUARD, fill: int = POISON, name: str = "buffer"):
        self.name = name
        self.shape = tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.fill = int(fill)
        self.guard_bytes = (int(guard_bytes) + 255) & ~255
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize
        total = self.guard_bytes + 256 + self.nbytes + self.guard_bytes
        self.numpy_backed = str(device) == "numpy"
        if self.numpy_backed:
            self.arena = np.empty(total, np.uint8)
            base = self.arena.ctypes.data
        else:
            import torch

            self.arena = torch.empty(total, dtype=torch.uint8, device=device)
            base = self.arena.data_ptr()
        # first address >= base + guard_bytes that is PAYLOAD_PHASE (mod 256)
        self.offset = self.guard_bytes + (PAYLOAD_PHASE - (base + self.guard_bytes)) % 256
        self.address = base + self.offset
        assert self.address % 256 == PAYLOAD_PHASE and self.offset + self.nbytes + self.guard_bytes <= total
        self.poison()

    @property
    def ptr(self) -> C.c_void_p:
        return C.c_void_p(self.address)

    def poison(self, fill: int | None = None) -> None:
        """Refill the whole arena, payload included."""
        if fill is not None:
            self.fill = int(fill)
        if self.numpy_backed:
            self.arena[:] = self.fill
        else:
            self.arena.fill_(self.fill)

    def _bytes(self) -> np.ndarray:
        return self.arena if self.numpy_backed else self.arena.cpu().numpy()

    def payload_view(self):
        """The payload as a typed view of the arena itself (torch tensor or NumPy array): writes go to the arena."""
        raw = self.arena[self.offset:self.offset + self.nbytes]
        if self.numpy_backed:
            return raw.view(self.dtype).reshape(self.shape)
        import torch

        return raw.view(getattr(torch, self.dtype.name)).view(self.shape)

    def snapshot(self):
        """(payload as a NumPy array (a copy), front guard bytes, back guard bytes) from ONE read of the arena."""
        b = self._bytes()
        pay = b[self.offset:self.offset + self.nbytes].copy().view(self.dtype).reshape(self.shape)
        return pay, b[:self.offset], b[self.offset + self.nbytes:]

    def array(self) -> np.ndarray:
        return self.snapshot()[0]

    def guard_damage(self, snap=None) -> str | None:
        """None when both guards still hold the fill, else where the first damaged byte of each lies."""
        _, front, back = snap or self.snapshot()
        msgs = []
        bad = np.flatnonzero(front != self.fill)
        if bad.size:
            msgs.append(f"{bad.size} byte(s) written BEFORE {self.name}, nearest {self.offset - int(bad[-1])} byte(s) in front of "
                        f"element 0 (value {int(front[bad[-1]]):#x})")
        bad = np.flatnonzero(back != self.fill)
        if bad.size:
            past = int(bad[0])
            msgs.append(f"{bad.size} byte(s) written AFTER {self.name}, first {past} byte(s) past its end = flat element "
                        f"{(self.nbytes + past) // self.dtype.itemsize} of {self.nbytes // self.dtype.itemsize} "
                        f"(value {int(back[bad[0]]):#x})")
        return "; ".join(msgs) if msgs else None

    def guards_intact(self) -> bool:
        return self.guard_damage() is None

    def unwritten(self, snap=None) -> np.ndarray:
        """Boolean mask over the payload's elements: True where every byte of the element still equals the fill."""
        pay = (snap or self.snapshot())[0]
        b = np.ascontiguousarray(pay).view(np.uint8).reshape(self.shape + (self.dtype.itemsize,))
        return (b == self.fill).all(axis=-1)

    def check(self, written=True, what: str = "") -> np.ndarray:
        """The three assertions of a guarded call, in their order: guards intact; no element of ``written`` still poison;
        every other element still poison.  written: True (all), False / None (none) or a boolean mask that broadcasts
        against the payload from the LEFT (a [B] mask selects whole rows).  Returns the payload (a NumPy copy)."""
        snap = self.snapshot()
        where = f" ({what})" if what else ""
        damage = self.guard_damage(snap)
        assert damage is None, f"{self.name}{where}: {damage}"
        if written is True or written is False or written is None:
            w = np.full(self.shape, bool(written), bool)
        else:
            w = np.asarray(written, bool)
            w = np.broadcast_to(w.reshape(w.shape + (1,) * (len(self.shape) - w.ndim)), self.shape)
        un = self.unwritten(snap)
        miss = np.argwhere(w & un)
        assert miss.size == 0, (f"{self.name}{where}: {len(miss)} element(s) the call must write are still poison, first index "
                                f"{miss[0].tolist()}")
        stray = np.argwhere(~w & ~un)
        assert stray.size == 0, (f"{self.name}{where}: {len(stray)} element(s) the call must leave alone were written, first "
                                 f"index {stray[0].tolist()} = {snap[0][tuple(stray[0])]!r}")
        return snap[0]


def two_fill(buf: GuardedBuffer, call, what: str = "") -> np.ndarray:
    """For payloads that can legitimately hold the poison byte (render frames): ``call()`` once on 0xA5 and once on 0x5A
    from the same state; guards intact both times and the two payloads identical, hence fully written."""
    got = []
    for fill in (POISON, POISON_ALT):
        buf.poison(fill)
        call()
        snap = buf.snapshot()
        damage = buf.guard_damage(snap)
        assert damage is None, f"{buf.name} ({what}, fill {fill:#x}): {damage}"
        got.append(snap[0])
    buf.poison(POISON)
    diff = np.argwhere(got[0] != got[1])
    assert diff.size == 0, (f"{buf.name} ({what}): {len(diff)} element(s) keep whatever the buffer held before the call, first "
                            f"index {diff[0].tolist()}")
    return got[0]


# ---------------------------------------------------------------------------------------------------------------------
# the engine's outputs behind guards
# ---------------------------------------------------------------------------------------------------------------------
MA_OUTPUTS = ("obs", "rewards", "terminated", "truncated", "info_all", "info_agent")
CTE_OUTPUTS = ("obs", "reward", "terminated", "truncated", "info")


def ma_output_specs(B: int, N: int, L: int) -> dict:
    """name -> (shape of one [B]-slab, dtype) of the outputs of mapf_step (final_obs included)."""
    return {"obs": ((B, N, L), np.float32), "rewards": ((B, N), np.float32), "terminated": ((B,), np.uint8),
            "truncated": ((B,), np.uint8), "info_all": ((B, 14), np.float32), "info_agent": ((B, N, 2), np.uint8),
            "final_obs": ((B, N, L), np.float32)}


def cte_output_specs(B: int, L: int) -> dict:
    return {"obs": ((B, L), np.float32), "reward": ((B,), np.float64), "terminated": ((B,), np.uint8),
            "truncated": ((B,), np.uint8), "info": ((B, 4), np.float32), "final_obs": ((B, L), np.float32)}


def guarded_outputs(specs: dict, device, lead=(), names=None, prefix: str = "") -> dict:
    """One GuardedBuffer per output of ``specs`` (``names``: a subset); ``lead`` = extra leading dimensions ([T] of the
    fused launches) -- the guard stays one [B]-slab, so a [T+1]-th slab lands in it."""
    out = {}
    for k, (shape, dt) in specs.items():
        if names is not None and k not in names:
            continue
        slab = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[k] = GuardedBuffer(tuple(lead) + tuple(shape), dt, device, guard_bytes_for(slab), name=prefix + k)
    return out


def _ptr(buf):
    return None if buf is None else buf.ptr


def _sync(env):
    import torch

    torch.cuda.synchronize(env.device)


def device_bytes(env, a, dtype):
    """A host array as a contiguous device tensor of the engine (inputs: actions, masks, ids)."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(env.device)


class _GuardedCalls:
    """What the two guarded steppers share: every output of the step entry points in a GuardedBuffer, poisoned before
    every call; ``reset`` / ``step`` check the write contract after the call, ``launch`` / ``reset_masked`` leave the
    checking of partial contracts (masked steps, latched errors) to the test."""

    OUTPUTS = ()

    def _init_guards(self, specs, call, only):
        env = self.env
        self.call = call
        self.specs = specs
        self.only = None if only is None else tuple(only)
        self.buf = guarded_outputs(specs, env.device, names=None if only is None else tuple(only) + ("obs",))  # reset() needs obs
        self.history = []  # the dict every step() returned
        self.reset_obs0 = None  # the observation of the first reset()
        self._ones = device_bytes(env, np.ones(self.B), np.uint8)

    def _passed(self, k):
        return self.buf.get(k) if (self.only is None or k in self.only) else None

    def poison(self):
        for b in self.buf.values():
            b.poison()

    def reset(self):
        obs = self.reset_masked(None)
        if self.reset_obs0 is None:
            self.reset_obs0 = obs
        return obs

    def reset_masked(self, mask, with_obs: bool = True):
        """mapf_reset / mapf_cte_reset of the envs with mask != 0 (None: all, mask pointer NULL).  Rows of selected envs
        are written, all others left alone; with_obs=False passes obs = NULL (state only).  Returns the payload."""
        env, obs = self.env, self.buf["obs"]
        obs.poison()
        m = None if mask is None else device_bytes(env, mask, np.uint8)
        env._check(self._reset_entry(env._h, None if m is None else C.c_void_p(m.data_ptr()), obs.ptr if with_obs else None,
                                     env._stream()))
        _sync(env)
        rows = True if mask is None else np.asarray(mask).astype(bool)
        return obs.check(rows if with_obs else False, f"reset, mask {'NULL' if mask is None else 'given'}, obs "
                                                      f"{'given' if with_obs else 'NULL'}")

    def launch(self, actions, auto_reset=True, mask_ptr=None, sync: bool = True) -> dict:
        """Poison every buffer, make the step call, wait.  mask_ptr: a device uint8 [B] pointer -> the masked entry point.
        Returns name -> pointer passed (None = NULL)."""
        env = self.env
        a = device_bytes(env, actions, np.int8)
        self.poison()
        p = {k: _ptr(self._passed(k)) for k in self.specs}
        if mask_ptr is None and self.call == "masked":
            mask_ptr = C.c_void_p(self._ones.data_ptr())
        env._check(self._step_entry(C.c_void_p(a.data_ptr()), p, 1 if auto_reset else 0, mask_ptr))
        if sync:
            _sync(env)
        return p

    def step(self, actions, auto_reset=True):
        p = self.launch(actions, auto_reset)
        what = f"step[{self.call}] auto_reset={int(bool(auto_reset))}"
        res = {"rc": 0}
        for k in self.OUTPUTS:
            res[k] = self.buf[k].check(True, what) if p[k] is not None else None
            if p[k] is None and k in self.buf:
                self.buf[k].check(False, what + ", pointer not passed")
        res["final_obs"] = None
        if "final_obs" in self.buf:
            if p["final_obs"] is None or not auto_reset:
                # mapf_step.h: final_obs is not written at all when auto_reset == 0
                self.buf["final_obs"].check(False, what)
            elif res["terminated"] is not None and res["truncated"] is not None:
                # rows of envs that finished hold the terminal observation, every other row is left alone
                res["final_obs"] = self.buf["final_obs"].check((res["terminated"] | res["truncated"]).astype(bool), what)
        self.history.append(res)
        return res


class GuardedEngineStepper(_GuardedCalls, EngineStepper):
    """EngineStepper whose reset / step go through the raw C ABI with every output in a GuardedBuffer, poisoned before
    every call and checked after it.  call: "step" (mapf_step, final_obs always passed), "bound" (mapf_bind_outputs once,
    then mapf_step_bound) or "masked" (mapf_step_masked with an all-one mask).  only: pass just these outputs, every
    other pointer NULL (the returned dict holds None for them)."""

    OUTPUTS = MA_OUTPUTS

    def __init__(self, *args, call: str = "step", only=None, **kw):
        EngineStepper.__init__(self, *args, **kw)
        self._init_guards(ma_output_specs(self.B, self.N, self.L), call, only)
        self._reset_entry = self.env._lib.mapf_reset
        if call == "bound":
            self.env._check(self.env._lib.mapf_bind_outputs(self.env._h, *(self.buf[k].ptr for k in MA_OUTPUTS)))

    def _step_entry(self, a, p, ar, mask_ptr):
        env = self.env
        if mask_ptr is not None:
            return env._lib.mapf_step_masked(env._h, a, mask_ptr, p["obs"], p["rewards"], p["terminated"], p["truncated"],
                                             p["info_all"], p["info_agent"], p["final_obs"], ar, env._stream())
        if self.call == "bound":
            p["final_obs"] = None
            return env._lib.mapf_step_bound(env._h, a, ar, env._stream())
        return env._lib.mapf_step(env._h, a, p["obs"], p["rewards"], p["terminated"], p["truncated"], p["info_all"],
                                  p["info_agent"], p["final_obs"], ar, env._stream())


class GuardedCteEngineStepper(_GuardedCalls, CteEngineStepper):
    """The single-agent counterpart: mapf_cte_reset / mapf_cte_step / mapf_cte_step_masked on guarded buffers."""

    OUTPUTS = CTE_OUTPUTS

    def __init__(self, *args, call: str = "step", only=None, **kw):
        CteEngineStepper.__init__(self, *args, **kw)
        self._init_guards(cte_output_specs(self.B, self.L), call, only)
        self._reset_entry = self.env._lib.mapf_cte_reset

    def _step_entry(self, a, p, ar, mask_ptr):
        env = self.env
        if mask_ptr is not None:
            return env._lib.mapf_cte_step_masked(env._h, a, mask_ptr, p["obs"], p["reward"], p["terminated"], p["truncated"],
                                                 p["info"], p["final_obs"], ar, env._stream())
        return env._lib.mapf_cte_step(env._h, a, p["obs"], p["reward"], p["terminated"], p["truncated"], p["info"],
                                      p["final_obs"], ar, env._stream())


# ---------------------------------------------------------------------------------------------------------------------
# the case table: kernel path -> smallest configuration that reaches it
# ---------------------------------------------------------------------------------------------------------------------
def _common(**over) -> dict:
    """workloads.COMMON (the flags the compile-time specialisations are matched on) with a short episode."""
    from dl_reference_models_amd.workloads import COMMON

    cfg = dict(COMMON)
    cfg.pop("info_mode", None)
    cfg.update(over)
    return cfg


STEPS = 40          # steps of every case
DENSITY = 0.15
DENSITY_WIDE = 0.04  # N = 33 / 64 need 2N free cells (and lifelong respawns a spare one) of at most 144


def _ma(cid, n, h, w, lanes, expect, spe=7, density=DENSITY, engine=None, **over):
    """lanes: the group width the case must land on (G = 64 / lanes envs per wave decides the batches); expect:
    (specialized_kernel, lanes_per_env, threads, jit) of launch_info()."""
    return {"id": cid, "kind": "ma", "N": n, "H": h, "W": w, "lanes": lanes, "expect": expect, "density": density,
            "cfg": dict(_common(steps_per_episode=spe, **over), num_agents=n), "engine": dict(engine or {})}


def _cte(cid, n, h, w, lanes, force, many_lanes=None, batches=None, spe=6, steps=STEPS, **over):
    """force: lanes_per_env passed to the engine (0 = its own choice, which must be ``lanes``)."""
    return {"id": cid, "kind": "cte", "N": n, "H": h, "W": w, "lanes": lanes, "many_lanes": many_lanes or lanes,
            "expect": (0, lanes, 128, False), "density": DENSITY, "batches": batches, "steps": steps,
            "cfg": dict({"num_agents": n, "steps_per_episode": spe}, **over), "engine": {"lanes_per_env": force} if force else {}}


_OFF = {"include_action_mask_in_obs": False}
_TRAIN = {"sensor_range": 3, "include_action_mask_in_obs": False}

CASES = [
    # compile-time specialisations of the small groups: k_step3 (three waves) and the two-wave 128-register build
    _ma("c3_three_wave", 8, 9, 11, 8, (1, 8, 192, False)),
    _ma("c3_dense_two_wave", 8, 9, 11, 8, (1, 8, 128, False), engine={"register_budget": "dense"}),
    _ma("c2", 4, 7, 10, 4, (2, 4, 192, False), spe=6),
    _ma("c3_L28", 8, 10, 9, 8, (4, 8, 192, False), **_OFF),
    _ma("c2_L28", 4, 6, 9, 4, (5, 4, 192, False), spe=5, **_OFF),
    _ma("c3_no_sentinel_columns_5x64", 8, 5, 64, 8, (1, 8, 192, False), spe=9),
    # the reference's training setup: 16-lane groups on bit rows, and the two older observation waves
    _ma("train16_bit_rows", 16, 11, 12, 16, (6, 16, 192, False), spe=8, **_TRAIN),
    _ma("train16_table_walk", 16, 11, 12, 16, (6, 16, 192, False), spe=8, engine={"small_group_observation": "table_walk"},
        **_TRAIN),
    _ma("train16_rows_off", 16, 11, 12, 16, (6, 16, 192, False), spe=8, engine={"small_group_rows": "off"}, **_TRAIN),
    _ma("train16_lifelong_generic", 16, 11, 12, 16, (0, 16, 128, False), spe=8, lifelong_mapf=True, **_TRAIN),
    # 64-lane groups: k_stepw (three waves, bit rows), the two-wave kernel with the word-per-cell map, idle lanes
    _ma("c5_stepw_lifelong", 64, 12, 12, 64, (3, 64, 192, False), spe=6, density=DENSITY_WIDE, lifelong_mapf=True),
    _ma("c5_two_wave_lifelong", 64, 12, 12, 64, (3, 64, 128, False), spe=6, density=DENSITY_WIDE, lifelong_mapf=True,
        engine={"wide_kernel": "two_wave"}),
    _ma("wide_n33_finite", 33, 11, 12, 64, (0, 64, 192, False), spe=6, density=DENSITY_WIDE),
    # runtime-config kernels: sliced draw, sampler workgroups, the generic kernel on the c3 configuration
    _ma("runtime_sliced_sr1", 8, 8, 11, 8, (0, 8, 192, False), sensor_range=1),
    _ma("runtime_sampler_workgroups", 8, 8, 11, 8, (0, 8, 128, False), sensor_range=1,
        engine={"background_draw": "sampler_workgroups"}),
    _ma("c3_forced_generic", 8, 9, 11, 8, (0, 8, 192, False), engine={"force_generic_kernel": True}),
    # partial groups (idle lanes inside a group), one of them deterministic
    _ma("partial_n3", 3, 6, 8, 4, (0, 4, 128, False), spe=5),
    _ma("partial_n5_deterministic", 5, 7, 9, 8, (0, 8, 128, False), spe=6, deterministic=True),
    _ma("partial_n12", 12, 10, 11, 16, (0, 16, 128, False), spe=8),
    _ma("partial_n20", 20, 11, 12, 32, (0, 32, 128, False), spe=8),
    _ma("partial_n6_on_64_lanes", 6, 7, 9, 64, (0, 64, 192, False), spe=6, engine={"lanes_per_env": 64}),
    # a configuration without a prebuilt specialisation, compiled at creation
    _ma("jit_n8_sr1", 8, 8, 11, 8, (0, 8, 192, True), sensor_range=1, engine={"jit_specialize": True}),
    # the single-agent env: the width it picks by itself, one forced width per kernel instantiation, and a batch at
    # which the fused launches pick another width than the single steps
    _cte("cte_n4_6x7_default", 4, 6, 7, 64, 0),
    _cte("cte_n4_6x7_lanes4", 4, 6, 7, 4, 4),
    _cte("cte_n4_6x7_lanes16", 4, 6, 7, 16, 16),
    _cte("cte_n8_9x11_default", 8, 9, 11, 64, 0, spe=8),
    _cte("cte_n8_9x11_lanes8", 8, 9, 11, 8, 8, spe=8),
    _cte("cte_n8_9x11_lanes32", 8, 9, 11, 32, 32, spe=8),
    _cte("cte_n4_6x7_fused_narrower", 4, 6, 7, 64, 0, many_lanes=32, batches=(512,), steps=30),
]
CASE_BY_ID = {c["id"]: c for c in CASES}
MA_CASES = [c for c in CASES if c["kind"] == "ma"]
CTE_CASES = [c for c in CASES if c["kind"] == "cte"]


def case_batches(case) -> tuple:
    """B in {1, G + 1, 3G - 1} with G = 64 / lanes envs per wave ({1, 3} for G = 1): every batch but 1 leaves a ragged
    last workgroup."""
    if case.get("batches"):
        return tuple(case["batches"])
    G = 64 // case["lanes"]
    return (1, 3) if G == 1 else (1, G + 1, 3 * G - 1)


def case_params(cases=None):
    """(case id, B) of every case and batch, for pytest.mark.parametrize."""
    return [(c["id"], B) for c in (CASES if cases is None else cases) for B in case_batches(c)]


def case_inputs(case, B: int) -> dict:
    """Everything a run of ``case`` at batch B is a function of (computed once per case and batch, shared by the tests:
    treat it as read-only): grids, one seed per env, the per-env step counter set after the first reset (staggered
    episode phases), fixed tables (deterministic) and the action stream.  The stream is the biased ('greedy') mix of the
    engine-vs-oracle parity tests, except that an agent steps along the larger axis of its goal delta three times out of
    four (positions and goals of the CPU oracle, which is stepped along): with 5-9 steps per episode the biased mix alone
    ends no episode in success."""
    return _case_inputs(case["id"], int(B))


@functools.lru_cache(maxsize=None)
def _case_inputs(cid: str, B: int) -> dict:
    case = CASE_BY_ID[cid]
    n, h, w = case["N"], case["H"], case["W"]
    spe = int(case["cfg"]["steps_per_episode"])
    steps = case.get("steps", STEPS)
    # every grid needs 2N free cells, a lifelong one spare cells for the respawns
    need = 2 * n + (8 if case["cfg"].get("lifelong_mapf") else 0)
    grids = np.stack([synth_grid(20_000 + b, h, w, case["density"], need) for b in range(B)])
    out = {"grids": grids, "seeds": [300 + b for b in range(B)], "actions": None,
           "step_counts": np.array([(3 * b + 1) % spe for b in range(B)], np.int32), "fixed_starts": None, "fixed_goals": None}
    if case["cfg"].get("deterministic"):
        fs, fg = [], []
        for b in range(B):
            free = np.argwhere(grids[b] == 0)
            pick = np.random.default_rng(500 + b).permutation(len(free))[:2 * n]
            fs.append(free[pick[:n]])
            fg.append(free[pick[n:]])
        out["fixed_starts"], out["fixed_goals"] = np.array(fs, np.int16), np.array(fg, np.int16)
    rng = np.random.default_rng(999)
    mix = rng.choice(5, size=(steps, B, n), p=[0.1, 0.1, 0.3, 0.4, 0.1])
    toward = rng.random((steps, B, n)) < 0.75
    st = make_oracle(case, out)
    st.reset()
    st.set_step_counts(out["step_counts"])
    actions = np.zeros((steps, B, n), np.int8)
    for t in range(steps):
        d = st.goals().astype(np.int64) - st.positions().astype(np.int64)
        dr, dc = d[..., 0], d[..., 1]
        greedy = np.where(np.abs(dr) >= np.abs(dc), np.where(dr > 0, 3, np.where(dr < 0, 1, 0)), np.where(dc > 0, 2, 4))
        actions[t] = np.where(toward[t], greedy, mix[t])
        assert st.step(actions[t], auto_reset=True)["rc"] == 0
    out["actions"] = actions
    return out


def make_oracle(case, inp):
    from trace_util import CteOracleStepper, OracleStepper

    cls = OracleStepper if case["kind"] == "ma" else CteOracleStepper
    return cls(inp["grids"], case["cfg"], seeds=inp["seeds"], fixed_starts=inp["fixed_starts"], fixed_goals=inp["fixed_goals"])


def make_engine(case, inp, cls=None, **kw):
    if cls is None:
        cls = GuardedEngineStepper if case["kind"] == "ma" else GuardedCteEngineStepper
    return cls(inp["grids"], case["cfg"], seeds=inp["seeds"], fixed_starts=inp["fixed_starts"], fixed_goals=inp["fixed_goals"],
               **case["engine"], **kw)


def coverage_of(case, B: int) -> dict:
    """What a run of the case at batch B exercises, from the CPU oracle alone: steps in which some envs finish and
    others do not, episode ends, ends by success, lifelong respawns."""
    inp = case_inputs(case, B)
    st = make_oracle(case, inp)
    st.reset()
    st.set_step_counts(inp["step_counts"])
    cov = {"mixed_steps": 0, "episode_ends": 0, "successes": 0, "respawns": 0.0}
    for a in inp["actions"]:
        out = st.step(a, auto_reset=True)
        assert out["rc"] == 0
        done = (out["terminated"] | out["truncated"]).astype(bool)
        cov["mixed_steps"] += int(done.any() and not done.all())
        cov["episode_ends"] += int(done.sum())
        cov["successes"] += int((out["terminated"].astype(bool) & ~out["truncated"].astype(bool)).sum())
        if case["kind"] == "ma" and case["cfg"].get("lifelong_mapf"):
            cov["respawns"] += float(out["info_all"][:, 0].sum())  # goals_reached_step: every one respawns the goal
    return cov
