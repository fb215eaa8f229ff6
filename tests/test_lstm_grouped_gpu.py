"""The grouped LSTM sequence kernels on the device (mapf_lstm_seq_forward_grouped / _backward_grouped through the raw C ABI,
and learner.lstm_sequence with whh [G, 256, 64] over them): row r recurs through whh[r % G].  Every output is guarded and
poisoned, every input lies between guards that read as NaN.

What the kernels return is compared BIT FOR BIT with the existing ungrouped entry points on each group's rows gathered
contiguously with whh[g] (the ungrouped calls are the one-group case of the same kernels, and a row's arithmetic does not
depend on its neighbours); the ungrouped calls are pinned to the float64 loop by test_lstm_seq_gpu.  dW_hh, which a batched
GEMM after the backward kernel sums, is compared with the float64 loop within learner_util.GRAD_MARGIN x dev."""

import ctypes as C

import numpy as np
import pytest
import torch

import dte_util as du
import learner_util as lu
from guard_util import GuardedBuffer, guard_bytes_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BYTE = 0xFF
OUT_F = ("h", "c", "gates")
OUT_B = ("dxg", "dh0", "dc0")


def _lib():
    from dl_reference_models_amd import _lib as L

    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class RawGrouped:
    """Both calls on guarded buffers; groups = None: the existing ungrouped entry points (whh [256, 64])."""

    def __init__(self, inp, groups):
        self.L, self.lib = _lib()
        self.groups = groups
        self.T, self.R = inp["xg"].shape[:2]
        T, R = self.T, self.R
        sh = {"xg": (T, R, 256), "whh": inp["whh"].shape, "reset": (T, R), "h0": (R, 64), "c0": (R, 64), "h": (T, R, 64),
              "c": (T, R, 64), "gates": (T, R, 256), "dh": (T, R, 64), "dhT": (R, 64), "dcT": (R, 64), "dxg": (T, R, 256),
              "dh0": (R, 64), "dc0": (R, 64)}
        self.buf = {}
        for k in ("xg", "whh", "reset", "h0", "c0", "dh", "dhT", "dcT"):
            if inp.get(k) is None:
                continue
            dt = np.uint8 if k == "reset" else np.float32
            b = GuardedBuffer(sh[k], dt, DEV, fill=NAN_BYTE, name=k)
            b.payload_view().copy_(torch.from_numpy(np.ascontiguousarray(inp[k], dtype=dt)))
            self.buf[k] = b
        for k in OUT_F + OUT_B:
            slab = int(np.prod(sh[k][1:])) * 4
            self.buf[k] = GuardedBuffer(sh[k], np.float32, DEV, guard_bytes_for(min(slab, 1 << 20)), name=k)

    def ptr(self, k):
        return self.buf[k].ptr if k in self.buf else None

    def forward(self, rows=None, groups=None):
        p = self.ptr
        tail = (p("xg"), p("whh"), p("reset"), p("h0"), p("c0"), p("h"), p("c"), p("gates"), _stream())
        R = self.R if rows is None else rows
        if self.groups is None:
            return self.lib.mapf_lstm_seq_forward(self.T, R, *tail)
        return self.lib.mapf_lstm_seq_forward_grouped(self.T, R, self.groups if groups is None else groups, *tail)

    def backward(self, rows=None, groups=None):
        p = self.ptr
        tail = (p("whh"), p("reset"), p("c0"), p("c"), p("gates"), p("dh"), p("dhT"), p("dcT"), p("dxg"), p("dh0"), p("dc0"), _stream())
        R = self.R if rows is None else rows
        if self.groups is None:
            return self.lib.mapf_lstm_seq_backward(self.T, R, *tail)
        return self.lib.mapf_lstm_seq_backward_grouped(self.T, R, self.groups if groups is None else groups, *tail)

    def poison(self):
        for k in OUT_F + OUT_B:
            self.buf[k].poison()

    def run(self):
        """Forward then backward, every output checked as fully written and nothing else touched; returns the payloads."""
        self.poison()
        assert self.forward() == 0
        torch.cuda.synchronize()
        out = {k: self.buf[k].check(True, "forward") for k in OUT_F}
        for k in OUT_B:
            self.buf[k].check(False, "forward")
        assert self.backward() == 0
        torch.cuda.synchronize()
        out.update({k: self.buf[k].check(True, "backward") for k in OUT_B})
        for k in ("xg", "whh", "h0", "c0", "dh", "dhT", "dcT"):
            assert self.buf[k].guards_intact(), k
        return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


CASES = [(s, r) for s in du.LSTM_SHAPES for r in lu.RESETS]


@pytest.mark.parametrize("shape,reset_kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_a_groups_rows_get_the_bits_of_the_ungrouped_call(shape, reset_kind):
    T, per, G = shape
    c = du.lstm_case(shape, reset_kind)
    got = RawGrouped(c["inp"], G).run()
    for g in range(G):
        want = RawGrouped(du.group_inputs(c["inp"], g, G), None).run()
        for k in OUT_F + ("dxg",):
            assert np.array_equal(_bits(got[k][:, g::G]), _bits(want[k])), (k, g)
        for k in ("dh0", "dc0"):
            assert np.array_equal(_bits(got[k][g::G]), _bits(want[k])), (k, g)
    # the groups are not interchangeable: group 0's rows with the last group's matrix are something else
    if G > 1:
        other = du.group_inputs(c["inp"], 0, G)
        other["whh"] = np.ascontiguousarray(c["inp"]["whh"][G - 1])
        assert not np.array_equal(RawGrouped(other, None).run()["h"], got["h"][:, 0::G])


@pytest.mark.parametrize("shape,reset_kind", CASES, ids=lambda v: str(v).replace(" ", ""))
@pytest.mark.parametrize("fused", (True, False), ids=("fused", "torch_loop"))
def test_lstm_sequence_with_grouped_weights(shape, reset_kind, fused):
    """The autograd function is the two grouped calls and nothing else (bitwise), and dW_hh [G, 256, 64], one batched GEMM
    behind them, lies within GRAD_MARGIN x dev of the float64 loop on each group's rows."""
    from dl_reference_models_amd.learner import lstm_sequence

    T, per, G = shape
    c = du.lstm_case(shape, reset_kind)
    t = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in c["inp"].items()}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("xg", "whh", "h0", "c0")}
    h, (hT, cT) = lstm_sequence(leaf["xg"], leaf["whh"], t["reset"], leaf["h0"], leaf["c0"], fused=fused)
    loss = (h * t["dh"]).sum() + (hT * t["dhT"]).sum() + (cT * t["dcT"]).sum()
    dxg, dwhh, dh0, dc0 = torch.autograd.grad(loss, [leaf["xg"], leaf["whh"], leaf["h0"], leaf["c0"]])
    assert dwhh.shape == (G, 256, 64)
    if fused:
        raw = RawGrouped(c["inp"], G).run()
        for k, v in (("h", h.detach()), ("dxg", dxg), ("dh0", dh0), ("dc0", dc0)):
            assert np.array_equal(_bits(v.cpu().numpy()), _bits(raw[k])), k
    err, dev = float(np.abs(dwhh.cpu().numpy() - c["want_dwhh"]).max()), c["dev_dwhh"]
    print(f"grouped lstm T={T} rows/group={per} G={G} reset={reset_kind} fused={fused}: dwhh {err:.3e} / {dev:.3e}"
          + (f" = {err / dev:.2f}" if dev > 0 else ""))
    assert np.isfinite(dwhh.cpu().numpy()).all() and err <= lu.GRAD_MARGIN * dev, (err, dev)


def test_refused_arguments_launch_nothing():
    c = du.lstm_case((2, 33, 3), "none")
    raw = RawGrouped(c["inp"], 3)
    CFG = raw.L.MAPF_ERR_CONFIG
    raw.poison()
    torch.cuda.synchronize()
    for bad in ({"groups": 0}, {"groups": -1}, {"groups": 2}, {"rows": 98}, {"rows": 0}):  # 99 rows: 3 x 33
        assert raw.forward(**bad) == CFG, bad
        assert raw.backward(**bad) == CFG, bad
    torch.cuda.synchronize()
    for k in OUT_F + OUT_B:
        raw.buf[k].check(False, "refused call")
    raw.run()  # and the same object is accepted as it is
