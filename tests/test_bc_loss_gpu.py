"""The behaviour-cloning objective kernel on the device (mapf_bc_loss through the raw C ABI, and the autograd function of
learner.py over it) against the float64 oracle of bc_util, with every output guarded and poisoned and every input between
guards that read as NaN.

Tolerances: the hit counts are compared exactly.  For every other tensor ``dev`` is the deviation of the learner's fp32 torch
path on the CPU from the float64 oracle for the case and quantity, floored at half an ulp; the kernel may deviate by a margin
times dev (bc_util.MARGINS says where the margins come from).

Figures measured on the MI355X, kernel error over dev, largest over all cases of this file: see DESIGN.md 4z."""

import ctypes as C
import itertools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import bc_util as bu
from guard_util import GuardedBuffer, guard_bytes_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BYTE = 0xFF
INPUTS = {"logits": np.float32, "expert": np.int8, "values": np.float32, "targets": np.float32}
OUTPUTS = ("nll", "dlogits", "dvalues", "partials")
SCALARS = ("vf_coeff", "ent_coeff")
EPS = float(np.finfo(np.float32).eps)


def _ids(s):
    return s if isinstance(s, str) else "T%d_rows%d_heads%d_groups%d" % s


def _lib():
    from dl_reference_models_amd import _lib as L

    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


class RawBC:
    """The call on guarded buffers: inputs between NaN guards, outputs poisoned before every call.  A case without values has
    neither ``values`` nor ``targets`` (both pointers NULL), and ``dvalues`` is then not passed either."""

    def __init__(self, inp, hp, groups=1):
        self.L, self.lib = _lib()
        self.T, self.R, self.heads = inp["expert"].shape
        self.G = groups
        self.hp = dict(hp)
        self.has_values = inp["values"] is not None
        self.buf = {}
        for k, dt in INPUTS.items():
            if inp[k] is None:
                continue
            b = GuardedBuffer(inp[k].shape, dt, DEV, fill=NAN_BYTE, name=k)
            b.payload_view().copy_(torch.from_numpy(np.ascontiguousarray(inp[k], dtype=dt)))
            self.buf[k] = b
        self.parts = int(self.lib.mapf_bc_partials(self.R, self.G))
        shapes = {"nll": (self.T, self.R), "dvalues": (self.T, self.R), "dlogits": (self.T, self.R, self.heads * 5),
                  "partials": (self.parts, 5)}
        for k, sh in shapes.items():
            slab = int(np.prod(sh[1:])) * 4
            self.buf[k] = GuardedBuffer(sh, np.float32, DEV, guard_bytes_for(min(slab, 1 << 20)), name=k)

    def ptr(self, k):
        return self.buf[k].ptr if k is not None and k in self.buf else None

    def call(self, T=None, rows=None, heads=None, groups=None, **over):
        a = {k: k for k in tuple(INPUTS) + OUTPUTS}
        if not self.has_values:
            a["dvalues"] = None
        a.update({k: v for k, v in over.items() if k not in SCALARS})
        s = [C.c_float(over.get(k, self.hp[k])) for k in SCALARS]
        return self.lib.mapf_bc_loss(self.T if T is None else T, self.R if rows is None else rows,
                                     self.heads if heads is None else heads, self.G if groups is None else groups,
                                     *(self.ptr(a[k]) for k in INPUTS), *s, *(self.ptr(a[k]) for k in OUTPUTS), _stream())

    def poison(self):
        for k in OUTPUTS:
            self.buf[k].poison()

    def run(self, **null):
        """One call, every output passed checked as fully written and every other one as untouched; the payloads."""
        self.poison()
        assert self.call(**null) == 0
        torch.cuda.synchronize()
        out = {}
        for k in OUTPUTS:
            if k in null or (k == "dvalues" and not self.has_values):
                self.buf[k].check(False, "pointer not passed")
            else:
                out[k] = self.buf[k].check(True, "call")
        return out

    def quantities(self, out):
        """Every quantity of bc_util.QUANTITIES from the payloads (the first three columns of the partials), the hit count of
        every tile, and the loss terms per group: the partials added over a group's tiles (in float32, as the learner does)
        over its count."""
        q = {k: out[k].astype(np.float64) for k in bu.ELEMENTWISE if k in out}
        sums = torch.from_numpy(out["partials"]).view(self.G, -1, 5).sum(1).numpy().astype(np.float64) / (self.T * self.R // self.G)
        q.update(partials=out["partials"][:, :3].astype(np.float64), tile_hits=out["partials"][:, 3], nll_mean=sums[:, 0],
                 vf_loss=sums[:, 1], entropy=sums[:, 2], accuracy=sums[:, 3] / self.heads, total=sums[:, 4])
        return q


def _compare(c, q, what):
    line, worst = [], {}
    for k in bu.QUANTITIES:
        if k not in q:
            assert k == "dvalues" and not c["with_values"]
            continue
        assert np.isfinite(q[k]).all(), (what, k)
        err, dev = float(np.abs(q[k] - c["want"][k]).max()), c["dev"][k]
        worst[k] = (err, dev)
        line.append(f"{k} {err:.3e} / {dev:.3e}" + (f" = {err / dev:.2f}" if dev > 0 else ""))
    print(f"bc parity {what} T={c['T']} rows={c['rows']} heads={c['heads']} groups={c['groups']} {c['kind']}"
          + ("" if c["with_values"] else " no values") + ": " + ", ".join(line))
    # the hits: exactly the oracle's, tile by tile (integers in fp32)
    assert np.array_equal(q["tile_hits"].astype(np.int64), c["want"]["tile_hits"]) and np.array_equal(q["tile_hits"], np.floor(q["tile_hits"]))
    for k, (err, dev) in worst.items():
        assert err <= bu.MARGINS[k] * dev, (what, k, err, dev)
    # the loss terms are a group's partials added up and divided by its count: each partial within its bound, plus the fp32 sum
    G = c["groups"]
    n, count = q["partials"].shape[0] // G, c["T"] * c["rows"] // G
    for g in range(G):
        mine = q["partials"][g * n:(g + 1) * n]
        slack = (n * bu.MARGINS["partials"] * c["dev"]["partials"] + n * EPS * np.abs(mine).sum()) / count
        for k in bu.SUMMED:
            assert abs(q[k][g] - c["want"][k][g]) <= slack, (what, k, g, q[k][g], c["want"][k][g], slack)
        assert abs(q["accuracy"][g] - c["want"]["accuracy"][g]) <= 2 * EPS  # an exact count, one division


def _autograd(c):
    """The same quantities through learner._BCLoss and torch's autograd on the device."""
    from dl_reference_models_amd import learner as ln

    t = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in c["inp"].items()}
    logits = t["logits"].clone().requires_grad_(True)
    values = None if t["values"] is None else t["values"].clone().requires_grad_(True)
    terms = ln._BCLoss.apply(logits, values, t["expert"], t["targets"], c["heads"], c["groups"], tuple(c["hp"][k] for k in SCALARS))
    grads = torch.autograd.grad(terms[0].sum(), [logits] + ([] if values is None else [values]))
    out = dict(zip(("total", "nll_mean", "vf_loss", "entropy", "accuracy"), terms), dlogits=grads[0])
    if values is not None:
        out["dvalues"] = grads[1]
    return out


def _parity(c, what="kernel"):
    raw = RawBC(c["inp"], c["hp"], c["groups"])
    out = raw.run()
    q = raw.quantities(out)
    _compare(c, q, what)
    # the fifth column is the weighted sum of the first three per tile, rounded there
    hp, G = c["hp"], c["groups"]
    total = q["nll_mean"] + hp["vf_coeff"] * q["vf_loss"] - hp["ent_coeff"] * q["entropy"]
    mass = np.abs(out["partials"][:, :3]).reshape(G, -1).sum(1) / (c["T"] * c["rows"] // G)
    assert (np.abs(q["total"] - total) <= 8 * EPS * mass).all()
    auto = _autograd(c)  # the autograd function is the call, the sum of the partials and nothing else
    for k in ("dlogits", "dvalues"):
        if k in out:
            assert _same(auto[k].cpu().numpy(), out[k]), k
    n, count = out["partials"].shape[0] // G, c["T"] * c["rows"] // G
    for col, k in ((0, "nll_mean"), (1, "vf_loss"), (2, "entropy"), (3, "accuracy"), (4, "total")):
        mag = np.abs(out["partials"][:, col].astype(np.float64)).reshape(G, n).sum(1) / count / (c["heads"] if k == "accuracy" else 1)
        assert (np.abs(auto[k].detach().cpu().numpy() - q[k]) <= n * EPS * mag + 4 * EPS * np.abs(q[k])).all(), k
    return q, out


@pytest.mark.parametrize("kind", bu.KINDS)
@pytest.mark.parametrize("shape", bu.SHAPES + bu.LONG_SHAPES, ids=_ids)
def test_parity_with_the_float64_oracle(shape, kind):
    q, out = _parity(bu.case(*shape, kind))
    for k in OUTPUTS:
        assert np.isfinite(out[k]).all(), k


@pytest.mark.parametrize("shape", ((2, 63, 3, 1), (33, 65, 3, 1), (40, 130, 1, 2), (1, 1, 1, 1)), ids=_ids)
def test_parity_without_values(shape):
    c = bu.case(*shape, "plain", False)
    assert c["inp"]["values"] is None and c["inp"]["targets"] is None
    q, out = _parity(c, "kernel without values")
    assert "dvalues" not in out and not out["partials"][:, 1].any()
    full = RawBC(bu.case(*shape)["inp"], c["hp"], shape[3]).run()  # nll and the hits are those of the call with values
    assert _same(full["nll"], out["nll"]) and _same(full["partials"][:, 3], out["partials"][:, 3])


def test_saturated_heads_stay_finite():
    """A logit 200 above the rest: four probabilities are exactly 0 in fp32, a label off the top costs about 200, and the
    entropy and its gradient are finite and 0 there (never 0 x inf)."""
    c = bu.case(5, 65, 16, 1, "saturated")
    lg = c["inp"]["logits"].reshape(5, 65, 16, 5)[:, 1::2]
    p32 = np.exp((lg - lg.max(axis=3, keepdims=True)).astype(np.float32))
    assert ((p32 == 0).sum(axis=3) == 4).all()
    out = RawBC(c["inp"], dict(c["hp"], vf_coeff=0.0), 1).run(values=None, targets=None, dvalues=None)
    assert all(np.isfinite(v).all() for v in out.values())
    full = RawBC(c["inp"], c["hp"], 1).run()  # with the entropy coefficient on
    scale = np.float32(1.0) / (np.float32(5) * np.float32(65))  # the call's 1 / (T rows), as the launch rounds it
    onehot = np.arange(5) == np.clip(c["inp"]["expert"][:, 1::2], 0, 4)[..., None]
    want = (np.where(p32 == 1, np.float32(1), np.float32(0)) - np.where(onehot, np.float32(1), np.float32(0))) * scale
    assert np.array_equal(full["dlogits"].reshape(5, 65, 16, 5)[:, 1::2], want)  # c (p - 1[label]): the entropy term is exactly 0
    assert float(out["nll"][:, 1::2].max()) > 150 and (out["nll"][:, 1::2] >= 0).all()


def test_ties_take_the_lowest_index():
    """Five equal logits: the greedy action is 0, so label 0 is a hit and label 4 is none; equal top logits at 1 and 3: 1."""
    logits = np.zeros((1, 4, 1 * 5), np.float32)
    logits[0, 2] = logits[0, 3] = (-1.0, 2.5, 0.0, 2.5, 1.0)
    expert = np.array([0, 4, 1, 3], np.int8).reshape(1, 4, 1)
    out = RawBC({"logits": logits, "expert": expert, "values": None, "targets": None}, bu.SETTINGS).run()
    assert float(out["partials"][0, 3]) == 2.0
    assert np.allclose(out["nll"][0, :2], np.log(5.0), rtol=1e-6)
    for a, b in ((0, 1), (2, 3)):  # (the cross-entropy does not care which of the tied actions the label is)
        assert out["nll"][0, a] == out["nll"][0, b]
    c = bu.case(5, 65, 16, 1, "ties")
    assert c["shares"]["label_tied_not_lowest"] > 0.02 and c["shares"]["label_tied_lowest"] > 0.02


@pytest.mark.parametrize("shape", ((2, 63, 3, 1), (2, 130, 1, 2)), ids=_ids)
def test_a_label_byte_out_of_range_is_clamped(shape):
    c = bu.case(*shape, "bad_action")
    inp = c["inp"]
    assert ((inp["expert"] < 0) | (inp["expert"] > 4)).mean() > 0.2
    a = RawBC(inp, c["hp"], shape[3]).run()
    b = RawBC(dict(inp, expert=np.clip(inp["expert"], 0, 4)), c["hp"], shape[3]).run()
    for k in a:
        assert _same(a[k], b[k]), k


@pytest.mark.parametrize("shape", ((3, 96, 1, 3), (2, 130, 1, 2), (64, 96, 1, 3)), ids=_ids)
def test_a_group_equals_the_ungrouped_call_on_its_rows(shape):
    """Bitwise: what a tile computes does not depend on ``groups``, and both calls scale the gradients by 1 / (T rows of
    the group)."""
    c = bu.case(*shape)
    T, R, H, G = shape
    whole = RawBC(c["inp"], c["hp"], G).run()
    tiles = whole["partials"].shape[0] // G
    for g in range(G):
        sub = {k: np.ascontiguousarray(v[:, g::G]) for k, v in c["inp"].items()}
        alone = RawBC(sub, c["hp"], 1).run()
        for k in bu.ELEMENTWISE:
            assert _same(whole[k][:, g::G], alone[k]), (g, k)
        assert _same(whole["partials"][g * tiles:(g + 1) * tiles], alone["partials"]), g
    assert not _same(whole["partials"][:tiles], whole["partials"][tiles:2 * tiles])


@pytest.mark.parametrize("shape", ((33, 65, 3, 1), (33, 34, 64, 1), (33, 130, 1, 2)), ids=_ids)
def test_the_first_chunk_of_a_longer_call_is_the_call_on_it(shape):
    """Nothing is carried between the chunks and no output depends on where a chunk begins: the first 32 steps of a call on
    T = 33 give, bit for bit, the nll of the T = 32 call on them, the 33rd that of the call on it alone, and the hit counts
    add up exactly.  dlogits and dvalues carry the call's own 1 / (T rows), one rounding of the scale and
    one of the product: rescaled they agree within two ulps, and parity pins them."""
    T, R, H, G = shape
    c = bu.case(*shape)
    long = RawBC(c["inp"], c["hp"], G).run()
    first = RawBC(bu.time_slice(c["inp"], 0, 32), c["hp"], G).run()
    last = RawBC(bu.time_slice(c["inp"], 32, 33), c["hp"], G).run()
    assert _same(long["nll"][:32], first["nll"]) and _same(long["nll"][32:], last["nll"])
    assert np.array_equal(long["partials"][:, 3], first["partials"][:, 3] + last["partials"][:, 3])
    for k in ("dlogits", "dvalues"):
        a, b = long[k][:32].astype(np.float64) * 33.0, first[k].astype(np.float64) * 32.0
        assert (np.abs(a - b) <= 4 * EPS * np.abs(b)).all(), k
    added = first["partials"][:, :3].astype(np.float64) + last["partials"][:, :3]
    mass = np.array([[float(np.abs(c["want"]["el"][k][:, idx]).sum()) for k in bu.SUMMED] for idx in bu.tiles_of(R, G)])
    count = np.array([len(idx) for idx in bu.tiles_of(R, G)]) * 33
    assert (np.abs(long["partials"][:, :3] - added) <= count[:, None] * EPS * mass).all()


@pytest.mark.parametrize("shape", ((5, 65, 16, 1), (2, 130, 1, 2), (33, 65, 3, 1)), ids=_ids)
def test_what_the_call_writes(shape):
    """Two runs are bitwise equal; every combination of NULL outputs is accepted, writes what is left exactly as the full call
    does and leaves everything else, guards included, untouched; the inputs are read, never written."""
    c = bu.case(*shape)
    raw = RawBC(c["inp"], c["hp"], shape[3])
    full = raw.run()
    again = raw.run()
    for k, v in full.items():
        assert _same(again[k], v), k
    for n in range(1, len(OUTPUTS) + 1):
        for names in itertools.combinations(OUTPUTS, n):
            null = {k: None for k in names}
            got = raw.run(**null)  # (checks every buffer not passed as untouched)
            assert set(got) == set(OUTPUTS) - set(names)
            for k, v in got.items():
                assert _same(v, full[k]), (null, k)
    for k in INPUTS:
        assert raw.buf[k].guard_damage() is None and _same(raw.buf[k].array(), c["inp"][k]), k


def test_refused_arguments_launch_nothing():
    c = bu.case(3, 96, 1, 3)
    raw = RawBC(c["inp"], c["hp"], 3)
    CFG = raw.L.MAPF_ERR_CONFIG
    raw.poison()
    torch.cuda.synchronize()
    bad = [{"T": 0}, {"T": -1}, {"rows": 0}, {"rows": -3}, {"heads": 0}, {"heads": 65}, {"heads": -1}, {"groups": 0}, {"groups": -1},
           {"groups": 5}, {"rows": 95}]
    bad += [{"logits": None}, {"expert": None}]
    bad += [{"values": None}, {"targets": None}]  # only one of the two
    bad += [{"values": None, "targets": None}]  # neither, but dvalues asked for
    bad += [{k: v} for k in SCALARS for v in (float("nan"), float("inf"), -float("inf"), -0.5)]
    for b in bad:
        assert raw.call(**b) == CFG, b
    torch.cuda.synchronize()
    for k in OUTPUTS:
        raw.buf[k].check(False, "refused call")
    parts = raw.lib.mapf_bc_partials
    assert parts(0, 1) == 0 and parts(65, 1) == 3 and parts(96, 3) == 3 and parts(130, 2) == 6 and parts(1, 1) == 1
    raw.run()  # and the same object is accepted as it is
    got = raw.run(values=None, targets=None, dvalues=None)  # neither, and no dvalues: accepted
    assert not got["partials"][:, 1].any()


def test_the_autograd_function_refuses_what_the_kernel_cannot_walk():
    """A tensor on another device or of another shape is refused before any launch: the kernel takes raw pointers."""
    from dl_reference_models_amd import learner as ln

    c = bu.case(3, 96, 1, 3)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c["inp"].items()}
    order = ("logits", "values", "expert", "targets")
    scalars = tuple(c["hp"][k] for k in SCALARS)
    for k in order[1:]:
        with pytest.raises(ValueError, match=k):
            ln._BCLoss.apply(*(t[j].cpu() if j == k else t[j] for j in order), 1, 3, scalars)
    for k in order:
        with pytest.raises(ValueError, match="must be|groups"):
            ln._BCLoss.apply(*(t[j][:, :-1] if j == k else t[j] for j in order), 1, 3, scalars)
    with pytest.raises(ValueError, match="groups"):
        ln._BCLoss.apply(*(t[j] for j in order), 1, 5, scalars)
    with pytest.raises(ValueError, match="both or neither"):
        ln._BCLoss.apply(t["logits"], t["values"], t["expert"], None, 1, 3, scalars)
    total = ln._BCLoss.apply(*(t[j].double() if j in ("logits", "values") else t[j] for j in order), 1, 3, scalars)[0]
    assert tuple(total.shape) == (3,) and torch.isfinite(total).all()  # floating point of another width: cast to what the kernel takes


def _first_call_capture():
    """The call captured as the very first call of a process and replayed, on the captured inputs and on changed ones (run as
    a script, see below)."""
    c = bu.case(3, 96, 1, 3)
    raw = RawBC(c["inp"], c["hp"], 3)
    raw.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert raw.call() == 0
    other = bu.make_inputs(3, 96, 1, 3, seed=1)
    for variant, inp in (("as captured", c["inp"]), ("changed inputs", other)):
        want, got32 = bu.oracle(inp, c["hp"], 3), bu.torch_path32(inp, c["hp"], 3)
        want["partials"], got32["partials"] = bu._partials(bu.oracle, inp, c["hp"], 3), bu._partials(bu.torch_path32, inp, c["hp"], 3)
        want["tile_hits"] = bu.tile_hits(want["hits"], 3)
        cc = dict(c, inp=inp, want=want, got32=got32, kind=variant, dev=bu.deviation(got32, want))
        for k in INPUTS:
            raw.buf[k].payload_view().copy_(torch.from_numpy(np.ascontiguousarray(inp[k])))
        raw.poison()
        g.replay()
        torch.cuda.synchronize()
        q = raw.quantities({k: raw.buf[k].check(True, f"replay, {variant}") for k in OUTPUTS})
        _compare(cc, q, "replay " + variant)
        if variant == "as captured":
            first = q
    assert not _same(first["nll"], q["nll"])
    print("first-call capture ok")


def test_graph_capture_from_the_very_first_call():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:])
    assert r.returncode == 0 and "first-call capture ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _first_call_capture()
