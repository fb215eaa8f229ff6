"""The LSTM sequence kernels on the device (mapf_lstm_seq_forward / _backward through the raw C ABI, and the autograd function
learner.lstm_sequence over them) against the float64 loop of learner_util, with every output guarded and poisoned and every
input between guards that read as NaN.

Tolerances: ``dev`` is the deviation of the fp32 CPU loop from the float64 oracle for the case and quantity; the kernel may
deviate by a margin times dev (learner_util says where FORWARD_MARGIN, KERNEL_GRAD_MARGIN and GRAD_MARGIN come from)."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import learner_util as lu
import regime_util as ru
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


def _shapes(T, R):
    return {"xg": (T, R, 256), "whh": (256, 64), "reset": (T, R), "h0": (R, 64), "c0": (R, 64), "h": (T, R, 64), "c": (T, R, 64),
            "gates": (T, R, 256), "dh": (T, R, 64), "dhT": (R, 64), "dcT": (R, 64), "dxg": (T, R, 256), "dh0": (R, 64),
            "dc0": (R, 64)}


class RawLstm:
    """Both calls on guarded buffers: inputs between NaN guards, outputs poisoned before every call."""

    def __init__(self, inp):
        self.L, self.lib = _lib()
        self.T, self.R = inp["xg"].shape[:2]
        sh = _shapes(self.T, self.R)
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
        return self.buf[k].ptr if k is not None and k in self.buf else None

    def forward(self, gates="gates", T=None, rows=None, **over):
        a = {k: k for k in ("xg", "whh", "reset", "h0", "c0", "h", "c")}
        a.update(over)
        return self.lib.mapf_lstm_seq_forward(self.T if T is None else T, self.R if rows is None else rows, self.ptr(a["xg"]),
                                              self.ptr(a["whh"]), self.ptr(a["reset"]), self.ptr(a["h0"]), self.ptr(a["c0"]),
                                              self.ptr(a["h"]), self.ptr(a["c"]), self.ptr(gates), _stream())

    def backward(self, dhT="dhT", dcT="dcT", dh0="dh0", dc0="dc0", T=None, rows=None, **over):
        a = {k: k for k in ("whh", "reset", "c0", "c", "gates", "dh", "dxg")}
        a.update(over)
        return self.lib.mapf_lstm_seq_backward(self.T if T is None else T, self.R if rows is None else rows, self.ptr(a["whh"]),
                                               self.ptr(a["reset"]), self.ptr(a["c0"]), self.ptr(a["c"]), self.ptr(a["gates"]),
                                               self.ptr(a["dh"]), self.ptr(dhT), self.ptr(dcT), self.ptr(a["dxg"]), self.ptr(dh0),
                                               self.ptr(dc0), _stream())

    def poison(self, names):
        for k in names:
            self.buf[k].poison()

    def run(self):
        """Forward then backward, every output checked as fully written; returns the payloads."""
        self.poison(OUT_F + OUT_B)
        assert self.forward() == 0
        torch.cuda.synchronize()
        out = {k: self.buf[k].check(True, "forward") for k in OUT_F}
        for k in OUT_B:
            self.buf[k].check(False, "forward")
        assert self.backward() == 0
        torch.cuda.synchronize()
        out.update({k: self.buf[k].check(True, "backward") for k in OUT_B})
        for k in OUT_F:  # backward reads them and leaves them as they were
            assert np.array_equal(self.buf[k].check(True, "after backward").view(np.uint8), out[k].view(np.uint8)), k
        return out


def _autograd(inp, fused=True):
    """The same quantities through learner.lstm_sequence and torch's autograd on the device."""
    from dl_reference_models_amd.learner import lstm_sequence

    t = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in inp.items()}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("xg", "whh", "h0", "c0")}
    h, (hT, cT) = lstm_sequence(leaf["xg"], leaf["whh"], t["reset"], leaf["h0"], leaf["c0"], fused=fused)
    loss = (h * t["dh"]).sum() + (hT * t["dhT"]).sum() + (cT * t["dcT"]).sum()
    dxg, dwhh, dh0, dc0 = torch.autograd.grad(loss, [leaf["xg"], leaf["whh"], leaf["h0"], leaf["c0"]])
    return {"h": h.detach(), "dxg": dxg, "dwhh": dwhh, "dh0": dh0, "dc0": dc0}


CASES = [(s, r) for s in lu.SHAPES for r in lu.RESETS]


def _parity(c):
    """Raw calls on guarded, poisoned buffers; the autograd function bit-identical to them; every quantity finite and
    within its margin times dev of the float64 oracle.  Returns what the device computed."""
    shape, reset_kind = c["shape"], c["reset_kind"]
    got = RawLstm(c["inp"]).run()
    auto = _autograd(c["inp"])
    for k in ("h", "dxg", "dh0", "dc0"):  # the autograd function is the two calls and nothing else
        assert np.array_equal(auto[k].cpu().numpy().view(np.uint8), got[k].view(np.uint8)), k
    got["dwhh"] = auto["dwhh"].cpu().numpy()
    line = []
    for k in lu.QUANTITIES:
        assert np.isfinite(got[k]).all(), k
        err, dev = float(np.abs(got[k] - c["want"][k]).max()), c["dev"][k]
        line.append(f"{k} {err:.3e} / {dev:.3e}" + (f" = {err / dev:.2f}" if dev > 0 else ""))
    print(f"lstm parity T={shape[0]} rows={shape[1]} reset={reset_kind}: " + ", ".join(line))
    for k in lu.QUANTITIES:
        err, dev = float(np.abs(got[k] - c["want"][k]).max()), c["dev"][k]
        assert err <= lu.margin_of(k) * dev, (k, err, dev)
    return got


@pytest.mark.parametrize("shape,reset_kind", CASES, ids=lambda v: str(v).replace(" ", ""))
def test_parity_with_the_float64_loop(shape, reset_kind):
    _parity(lu.lstm_case(shape, reset_kind))


@pytest.mark.parametrize("name", list(ru.LSTM_REGIMES))
def test_parity_beyond_a_fresh_net(name):
    """The regime cases of regime_util: four times the longest sequence so far, saturating gates, and gate pre-activations
    at which expf overflows in the kernels' sigmoid (test_regimes_host shows that each case reaches its regime)."""
    c = ru.lstm_case(name)
    got = _parity(c)
    if name == "overflow":
        exact = (got["gates"] == 0.0) | (got["gates"] == 1.0)
        exact[:, :, 128:192] = False  # (the g quarter is a tanh)
        assert (exact & (c["G"] < -89)).any() and (got["gates"][exact & (c["G"] < -89)] == 0.0).all()
        assert np.isfinite(got["dxg"][exact]).all()


def test_a_reset_row_equals_two_separate_sequences():
    T, R, k = 5, 65, 2
    inp = dict(lu.lstm_case((T, R), "none")["inp"])
    reset = np.zeros((T, R), np.uint8)
    reset[k, 1::2] = 1
    odd = np.arange(R) % 2 == 1
    whole = RawLstm(dict(inp, reset=reset)).run()
    zeros = np.zeros((R, 64), np.float32)
    head = RawLstm(dict(inp, xg=inp["xg"][:k], dh=inp["dh"][:k], dhT=zeros, dcT=zeros)).run()
    tail = RawLstm(dict(inp, xg=inp["xg"][k:], dh=inp["dh"][k:], h0=zeros, c0=zeros)).run()

    def same(a, b, what):
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8)), what

    for q in ("h", "c", "gates", "dxg"):
        same(whole[q][:k, odd], head[q][:, odd], q + " before the reset")
        same(whole[q][k:, odd], tail[q][:, odd], q + " from the reset on")
    same(whole["dh0"][odd], head["dh0"][odd], "dh0")
    same(whole["dc0"][odd], head["dc0"][odd], "dc0")
    # the rows without a reset are one sequence: they differ from the cut ones
    assert not np.array_equal(whole["h"][k:, ~odd], tail["h"][:, ~odd])


def test_what_each_call_writes():
    c = lu.lstm_case((5, 65), "scattered")
    raw = RawLstm(c["inp"])
    full = raw.run()
    again = raw.run()
    for k, v in full.items():
        assert np.array_equal(again[k].view(np.uint8), v.view(np.uint8)), k  # bitwise repeatable
    # forward without gates
    raw.poison(OUT_F)
    assert raw.forward(gates=None) == 0
    torch.cuda.synchronize()
    for k in ("h", "c"):
        assert np.array_equal(raw.buf[k].check(True, "gates NULL").view(np.uint8), full[k].view(np.uint8)), k
    raw.buf["gates"].check(False, "pointer not passed")
    raw.buf["gates"].payload_view().copy_(torch.from_numpy(full["gates"]))
    # backward without dh0 / dc0
    raw.poison(OUT_B)
    assert raw.backward(dh0=None, dc0=None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(raw.buf["dxg"].check(True, "dh0 / dc0 NULL").view(np.uint8), full["dxg"].view(np.uint8))
    raw.buf["dh0"].check(False, "pointer not passed")
    raw.buf["dc0"].check(False, "pointer not passed")
    # NULL dhT / dcT mean zeros
    raw.poison(OUT_B)
    assert raw.backward(dhT=None, dcT=None) == 0
    torch.cuda.synchronize()
    null = {k: raw.buf[k].check(True, "dhT / dcT NULL") for k in OUT_B}
    raw.buf["dhT"].payload_view().zero_()
    raw.buf["dcT"].payload_view().zero_()
    raw.poison(OUT_B)
    assert raw.backward() == 0
    torch.cuda.synchronize()
    for k, v in null.items():
        assert np.array_equal(raw.buf[k].check(True, "dhT / dcT zero").view(np.uint8), v.view(np.uint8)), k
    assert not np.array_equal(null["dxg"], full["dxg"])


def test_refused_arguments_launch_nothing():
    c = lu.lstm_case((2, 33), "none")
    raw = RawLstm(c["inp"])
    CFG = raw.L.MAPF_ERR_CONFIG
    raw.poison(OUT_F + OUT_B)
    torch.cuda.synchronize()
    for bad in ({"T": 0}, {"T": -1}, {"rows": 0}, {"rows": -3}, {"xg": None}, {"whh": None}, {"h0": None}, {"c0": None},
                {"h": None}, {"c": None}):
        assert raw.forward(**bad) == CFG, bad
    for bad in ({"T": 0}, {"rows": 0}, {"rows": -1}, {"whh": None}, {"c0": None}, {"c": None}, {"gates": None}, {"dh": None},
                {"dxg": None}):
        assert raw.backward(**bad) == CFG, bad
    torch.cuda.synchronize()
    for k in OUT_F + OUT_B:
        raw.buf[k].check(False, "refused call")
    raw.run()  # and the same object is accepted as it is


def _first_call_capture():
    """Both calls captured as the very first calls of a process, replayed on changed inputs (run as a script, see below)."""
    c = lu.lstm_case((5, 65), "scattered")
    raw = RawLstm(c["inp"])
    raw.poison(OUT_F + OUT_B)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert raw.forward() == 0
        assert raw.backward() == 0
    for variant in ("as captured", "changed"):
        inp = dict(c["inp"])
        if variant == "changed":
            inp["xg"] = -inp["xg"]
            inp["reset"] = np.ascontiguousarray(inp["reset"][::-1])
        want, got32 = lu.loop_with_grads(inp, torch.float64), lu.loop_with_grads(inp, torch.float32)
        for k in ("xg", "reset"):
            raw.buf[k].payload_view().copy_(torch.from_numpy(np.ascontiguousarray(inp[k])))
        raw.poison(OUT_F + OUT_B)
        g.replay()
        torch.cuda.synchronize()
        got = {k: raw.buf[k].check(True, f"replay, inputs {variant}") for k in OUT_F + OUT_B}
        err = {k: float(np.abs(got[k] - want[k]).max()) for k in got}
        dev = {k: float(np.abs(got32[k] - want[k]).max()) for k in got}
        print(f"lstm replay, inputs {variant}: " + ", ".join(f"{k} {err[k]:.3e} / {dev[k]:.3e}" for k in got))
        for k in got:
            assert err[k] <= lu.margin_of(k) * dev[k], (variant, k, err[k], dev[k])
    print("first-call capture ok")


def test_graph_capture_from_the_very_first_call():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first-call capture ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _first_call_capture()
