"""The fused parameter gradients on the device through the raw C ABI (mapf_trunk_param_grad, mapf_lstm_seq_param_grad,
mapf_param_grad_workspace_bytes) against the float64 oracles of param_grad_util: every output and the workspace between
poisoned guards, every input at the front of an allocation that reads as NaN behind it, the mask columns of the observation
NaN, and prev_action / prev_reward of the rows that start an episode unreadable (a byte of 77, NaN).

Tolerances: ``dev`` is the deviation of the fp32 CPU computation from the float64 one (param_grad_util); the kernels may
deviate by a margin times dev.  Every ratio is printed before it is asserted."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import param_grad_util as pg
import trunk_util as tu
from guard_util import GuardedBuffer, guard_bytes_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BYTE = 0xFF
TRUNK_IN = {"obs": np.float32, "prev_action": np.int8, "prev_reward": np.float32, "first": np.uint8, "a1": np.float32,
            "a2": np.float32, "dpre1": np.float32, "dpre2": np.float32, "dxg": np.float32}
TRUNK_OUT = ("dw1", "db1", "dw2", "db2", "dwih", "dbl")
LSTM_IN = {"dxg": np.float32, "h": np.float32, "h0": np.float32, "reset": np.uint8}


def _lib():
    from dl_reference_models_amd import _lib as L

    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _guarded_inputs(arrays: dict, dtypes: dict) -> dict:
    """Every input in front of NaN bytes: one stray 32-row stage behind the last row lands in them."""
    buf = {}
    for k, dt in dtypes.items():
        if arrays.get(k) is None:
            continue
        a = np.ascontiguousarray(arrays[k], dtype=dt)
        row_bytes = a.nbytes // max(1, a.shape[0]) if a.ndim > 1 else a.itemsize
        b = GuardedBuffer(a.shape, dt, DEV, guard_bytes_for(32 * row_bytes), fill=NAN_BYTE, name=k)
        b.payload_view().copy_(torch.from_numpy(a))
        buf[k] = b
    return buf


class _Raw:
    def ptr(self, k):
        if isinstance(k, C.c_void_p):
            return k
        return self.buf[k].ptr if k is not None and k in self.buf else None

    def poison(self):
        for k in self.outs + ("ws",):
            self.buf[k].poison()

    def off4(self, k):
        return C.c_void_p(self.buf[k].address + 4)  # inside the payload, not 16-byte aligned


class RawTrunkGrad(_Raw):
    outs = TRUNK_OUT

    def __init__(self, case):
        self.L, self.lib = _lib()
        inp = case["inp"]
        self.M, self.F, self.Lo, self.rec = inp["M"], inp["F"], inp["L"], bool(inp["recurrent"])
        self.buf = _guarded_inputs(pg.trunk_kernel_inputs(case), TRUNK_IN)
        shapes = {"dw1": (64, self.F), "db1": (64,), "dw2": (64, 64), "db2": (64,), "dwih": (256, 70), "dbl": (256,)}
        for k, s in shapes.items():
            self.buf[k] = GuardedBuffer(s, np.float32, DEV, name=k)
        self.ws_bytes = int(self.lib.mapf_param_grad_workspace_bytes(self.M, self.F, int(self.rec), 0))
        tiles = 2 * ((self.F + 1 + 31) // 32) + 6 + (24 if self.rec else 0)
        assert self.ws_bytes == pg.slabs_of(self.M)[0] * tiles * 4096
        self.buf["ws"] = GuardedBuffer((self.ws_bytes,), np.uint8, DEV, name="workspace")
        self.asked = tuple(k for k in TRUNK_OUT if self.rec or k not in ("dwih", "dbl"))

    def call(self, M=None, F=None, L=None, recurrent=None, ws_bytes=None, **over):
        a = {k: k for k in ("obs", "prev_action", "prev_reward", "first", "a1", "a2", "dpre1", "dpre2", "dxg")}
        a.update({k: (k if k in self.asked else None) for k in TRUNK_OUT})
        a["ws"] = "ws"
        a.update(over)
        p = [self.ptr(a[k]) for k in ("obs", "prev_action", "prev_reward", "first", "a1", "a2", "dpre1", "dpre2", "dxg", *TRUNK_OUT, "ws")]
        return self.lib.mapf_trunk_param_grad(self.M if M is None else M, self.F if F is None else F, self.Lo if L is None else L,
                                              int(self.rec) if recurrent is None else recurrent, *p,
                                              self.ws_bytes if ws_bytes is None else ws_bytes, _stream())

    def run(self, what="", **over):
        """One call; the outputs asked for fully written, the others and every guard (the workspace's included) untouched."""
        self.poison()
        torch.cuda.synchronize()
        assert self.call(**over) == 0, what
        torch.cuda.synchronize()
        asked = tuple(k for k in self.asked if over.get(k, k) is not None)
        got = {k: self.buf[k].check(True, what) for k in asked}
        for k in TRUNK_OUT:
            if k not in asked:
                self.buf[k].check(False, what + ", not asked for")
        assert self.buf["ws"].guard_damage() is None, self.buf["ws"].guard_damage()
        for k in TRUNK_IN:
            assert k not in self.buf or self.buf[k].guards_intact(), k
        return got


def _check_trunk(got, case, what, lines=None):
    for q, v in got.items():
        assert np.isfinite(v).all(), (what, q, "a NaN or inf: a row past M, a mask column or a first row's action / reward was read")
        err, dev = float(np.abs(v - case["want"][q].reshape(v.shape)).max()), pg.trunk_dev(case, q)
        line = f"param_grad parity {what}: {q} {err:.3e} / {dev:.3e} = {tu.ratio(err, dev):.2f} (margin {pg.TRUNK_MARGIN})"
        print(line)
        if lines is not None:
            lines.append(line)
        assert err <= pg.TRUNK_MARGIN * dev, line


@pytest.mark.parametrize("M", pg.TRUNK_ROWS)
def test_trunk_gradients_write_contract_and_parity(M):
    for m, (F, L), rec in pg.trunk_pairs():
        if m == M:
            case = tu.trunk_case(M, F, L, rec)
            _check_trunk(RawTrunkGrad(case).run(f"M={M} F={F} L={L}"), case, f"fresh M={M} F={F} L={L} rec={int(rec)}")


def test_the_pruned_cross_product_keeps_every_shape_with_both_kinds():
    pairs = pg.trunk_pairs()
    for rec in (True, False):
        assert {m for m, _s, r in pairs if r == rec} == set(pg.TRUNK_ROWS)
        assert {s for _m, s, r in pairs if r == rec} == set(tu.FEATURE_SHAPES)


@pytest.mark.parametrize("recurrent", (True, False), ids=("recurrent", "feed_forward"))
@pytest.mark.parametrize("regime", tu.REGIMES[1:])
def test_trunk_gradients_beyond_a_fresh_net(regime, recurrent):
    M, (F, L) = pg.TRUNK_ROWS[-1], (53, 58)
    case = tu.trunk_case(M, F, L, recurrent, regime)
    _check_trunk(RawTrunkGrad(case).run(regime), case, f"{regime} M={M} F={F} L={L} rec={int(recurrent)}")


def test_trunk_gradients_on_the_capped_partition():
    """One row more than MAX_SLABS slabs of SLAB_ROWS rows: the slabs grow, their count stays within the cap."""
    slabs, per = pg.slabs_of(pg.CAPPED_ROWS)
    assert per > pg.S and per % 32 == 0 and slabs <= pg.MAX_SLABS
    case = tu.trunk_case(pg.CAPPED_ROWS, 2, 2, False)
    raw = RawTrunkGrad(case)
    assert raw.ws_bytes == slabs * 8 * 4096  # 2 tiles of dW1 | db1, 2 of db2, 4 of dW2
    _check_trunk(raw.run("capped"), case, f"capped M={pg.CAPPED_ROWS} F=2 L=2 rec=0")


@pytest.mark.parametrize("recurrent", (True, False), ids=("recurrent", "feed_forward"))
def test_a_null_output_is_skipped_and_two_calls_are_bitwise_equal(recurrent):
    case = tu.trunk_case(pg.S + 1, 53, 58, recurrent)
    raw = RawTrunkGrad(case)
    full = raw.run("all outputs")
    again = raw.run("all outputs, again")
    for k in full:
        assert np.array_equal(full[k].view(np.uint32), again[k].view(np.uint32)), k
    for left_out in (("dw1", "db2"), ("db1", "dw2", "dwih"), ("dbl",), ("dwih", "dbl")):
        part = raw.run(f"without {left_out}", **{k: None for k in left_out})
        assert set(part) == set(raw.asked) - set(left_out)
        for k in part:
            assert np.array_equal(full[k].view(np.uint32), part[k].view(np.uint32)), (left_out, k)
    if recurrent:  # nothing of the gates asked for: their inputs are not needed
        part = raw.run("trunk only", dwih=None, dbl=None, dxg=None, prev_action=None, prev_reward=None, first=None)
        assert set(part) == {"dw1", "db1", "dw2", "db2"}
    assert raw.call(**{k: None for k in TRUNK_OUT}) == 0  # nothing asked for: accepted, nothing to do


@pytest.mark.parametrize("byte", (5, -1))
def test_an_action_byte_outside_the_moves_adds_no_one_hot_entry(byte):
    base = tu.trunk_case(33, 11, 11, True)
    inp = dict(base["inp"], prev_action=np.full(33, byte, np.int8), first=np.zeros(33, np.uint8))
    want = tu.trunk_np(inp, np.float64)
    case = {"inp": inp, "want": want, "dev": {q: float(np.abs(tu.trunk_np(inp, np.float32)[q] - want[q]).max()) for q in tu.PARAM_GRADS}}
    got = RawTrunkGrad(case).run(f"byte {byte}")
    assert (got["dwih"][:, 64:69] == 0).all() and (got["dwih"][:, 69] != 0).any()
    _check_trunk(got, case, f"action byte {byte}")


def test_refused_trunk_arguments_launch_nothing():
    for recurrent in (True, False):
        case = tu.trunk_case(33, 53, 58, recurrent)
        raw = RawTrunkGrad(case)
        CFG = raw.L.MAPF_ERR_CONFIG
        raw.poison()
        torch.cuda.synchronize()
        bad = [{"M": 0}, {"M": -1}, {"F": 0}, {"F": -2}, {"F": 126, "L": 126}, {"L": 57}, {"L": 59}, {"L": 52}, {"recurrent": 2}, {"recurrent": -1},
               {"obs": None}, {"a1": None}, {"a2": None}, {"dpre1": None}, {"dpre2": None},
               {"ws": None}, {"ws_bytes": raw.ws_bytes - 1}, {"ws_bytes": 0}, {"ws": raw.off4("ws")},
               {"a1": raw.off4("a1")}, {"a2": raw.off4("a2")}, {"dpre1": raw.off4("dpre1")}, {"dpre2": raw.off4("dpre2")}]
        if recurrent:
            bad += [{k: None} for k in ("dxg", "prev_action", "prev_reward", "first")]
            bad += [{"dxg": None, "dwih": None}, {"first": None, "dbl": None}]  # (the other of the two is still asked for)
            bad += [{"dxg": raw.off4("dxg")}, {"recurrent": 0}]
        else:
            bad += [{"dwih": "dwih"}, {"dbl": "dbl"}, {"recurrent": 1, "dwih": "dwih"}]  # (recurrent without its inputs)
        for b in bad:
            assert raw.call(**b) == CFG, (recurrent, b)
        torch.cuda.synchronize()
        for k in TRUNK_OUT + ("ws",):
            raw.buf[k].check(False, "refused call")
        _check_trunk(raw.run("after the refusals"), case, "after the refusals")
    lib = raw.lib
    assert lib.mapf_param_grad_workspace_bytes(0, 53, 1, 0) == 0 and lib.mapf_param_grad_workspace_bytes(33, 126, 1, 0) == 0
    assert lib.mapf_param_grad_workspace_bytes(33, 53, 2, 0) == 0 and lib.mapf_param_grad_workspace_bytes(33, 0, 0, 2) == 0
    assert lib.mapf_param_grad_workspace_bytes(33, 53, 1, -1) == 0


# ---- dW_hh -------------------------------------------------------------------------------------------------------------------
class RawLstmGrad(_Raw):
    outs = ("dwhh",)

    def __init__(self, case):
        self.L, self.lib = _lib()
        inp = case["inp"]
        self.T, self.R, self.groups = inp["T"], inp["R"], inp["groups"]
        self.buf = _guarded_inputs(inp, LSTM_IN)
        self.buf["dwhh"] = GuardedBuffer((self.groups, 256, 64), np.float32, DEV, guard_bytes_for(256 * 64 * 4), name="dwhh")
        self.ws_bytes = int(self.lib.mapf_param_grad_workspace_bytes(self.T * self.R, 0, 0, self.groups))
        assert self.ws_bytes == self.groups * pg.slabs_of(self.T * self.R // self.groups)[0] * 65536
        self.buf["ws"] = GuardedBuffer((self.ws_bytes,), np.uint8, DEV, name="workspace")

    def call(self, T=None, R=None, groups=None, ws_bytes=None, **over):
        a = {k: k for k in ("dxg", "h", "h0", "reset", "dwhh", "ws")}
        a.update(over)
        p = [self.ptr(a[k]) for k in ("dxg", "h", "h0", "reset", "dwhh", "ws")]
        return self.lib.mapf_lstm_seq_param_grad(self.T if T is None else T, self.R if R is None else R,
                                                 self.groups if groups is None else groups, *p,
                                                 self.ws_bytes if ws_bytes is None else ws_bytes, _stream())

    def run(self, what=""):
        self.poison()
        torch.cuda.synchronize()
        assert self.call() == 0, what
        torch.cuda.synchronize()
        got = self.buf["dwhh"].check(True, what)
        assert self.buf["ws"].guard_damage() is None, self.buf["ws"].guard_damage()
        for k in LSTM_IN:
            assert k not in self.buf or self.buf[k].guards_intact(), k
        return got


def _check_dwhh(got, case, what):
    assert np.isfinite(got).all(), (what, "a NaN or inf: a row past T x R was read")
    err = float(np.abs(got - case["want"]).max())
    line = f"param_grad parity {what}: dwhh {err:.3e} / {case['dev']:.3e} = {tu.ratio(err, case['dev']):.2f} (margin {pg.DWHH_MARGIN})"
    print(line)
    assert err <= pg.DWHH_MARGIN * case["dev"], line


@pytest.mark.parametrize("reset", pg.RESETS)
@pytest.mark.parametrize("T,R,groups", pg.DWHH_SHAPES)
def test_dwhh_write_contract_and_parity(T, R, groups, reset):
    case = pg.dwhh_case(T, R, groups, reset)
    raw = RawLstmGrad(case)
    got = raw.run(f"T={T} R={R} groups={groups} reset={reset}")
    _check_dwhh(got, case, f"T={T} R={R} groups={groups} reset={reset}")
    if (T, R, groups) == (3, 66, 2):
        again = raw.run("again")
        assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


def test_a_missed_reset_would_show():
    """The oracle itself tells the reset variants apart (h0 is not zero), so parity above pins the reset rule."""
    a, b, c = (pg.dwhh_case(5, 64, 1, k) for k in ("null", "quarter", "step1"))
    assert np.abs(a["want"] - b["want"]).max() > 100 * a["dev"] and np.abs(a["want"] - c["want"]).max() > 100 * a["dev"]
    assert np.array_equal(a["want"], pg.dwhh_case(5, 64, 1, "zero")["want"])


def test_dwhh_on_the_capped_partition():
    T, R, groups = pg.DWHH_CAPPED
    slabs, per = pg.slabs_of(T * R)
    assert T * R > pg.S * pg.MAX_SLABS and per > pg.S and slabs <= pg.MAX_SLABS
    case = pg.dwhh_case(T, R, groups, "quarter")
    raw = RawLstmGrad(case)
    assert raw.ws_bytes == slabs * 65536
    _check_dwhh(raw.run("capped"), case, f"capped T={T} R={R} groups={groups} reset=quarter")


def test_refused_lstm_arguments_launch_nothing():
    case = pg.dwhh_case(3, 66, 2, "quarter")
    raw = RawLstmGrad(case)
    CFG = raw.L.MAPF_ERR_CONFIG
    raw.poison()
    torch.cuda.synchronize()
    bad = [{"T": 0}, {"T": -1}, {"R": 0}, {"R": -2}, {"groups": 0}, {"groups": -1}, {"groups": 4}, {"R": 65}, {"dxg": None}, {"h": None},
           {"h0": None}, {"dwhh": None}, {"ws": None}, {"ws_bytes": raw.ws_bytes - 1}, {"ws": raw.off4("ws")}, {"dxg": raw.off4("dxg")},
           {"h": raw.off4("h")}, {"h0": raw.off4("h0")}]
    for b in bad:
        assert raw.call(**b) == CFG, b
    torch.cuda.synchronize()
    raw.buf["dwhh"].check(False, "refused call")
    raw.buf["ws"].check(False, "refused call")
    _check_dwhh(raw.run("after the refusals"), case, "after the refusals")


# ---- graph capture as the first GPU work of a process ----------------------------------------------------------------------
def _first_call_capture():
    """Both calls captured as the very first GPU work of a process and replayed: bitwise what the direct calls give."""
    tcase, lcase = tu.trunk_case(pg.S + 1, 53, 58, True), pg.dwhh_case(3, 66, 2, "quarter")
    rt, rl = RawTrunkGrad(tcase), RawLstmGrad(lcase)
    rt.poison(), rl.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert rt.call() == 0
        assert rl.call() == 0
    rt.poison(), rl.poison()
    g.replay()
    torch.cuda.synchronize()
    replayed = {k: rt.buf[k].check(True, "replay") for k in rt.asked}
    replayed_l = rl.buf["dwhh"].check(True, "replay")
    direct, direct_l = rt.run("direct"), rl.run("direct")
    for k in direct:
        assert np.array_equal(direct[k].view(np.uint32), replayed[k].view(np.uint32)), k
    assert np.array_equal(direct_l.view(np.uint32), replayed_l.view(np.uint32))
    _check_trunk(direct, tcase, "after capture")  # (and it is the rule's result, not stale data)
    _check_dwhh(direct_l, lcase, "after capture")
    print("first-call capture ok")


def test_graph_capture_from_the_very_first_call():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first-call capture ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _first_call_capture()
