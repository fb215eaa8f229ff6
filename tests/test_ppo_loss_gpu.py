"""The PPO objective kernel on the device (mapf_ppo_loss through the raw C ABI, and the autograd function of learner.py over
it) against the float64 oracle of ppo_loss_util, with every output guarded and poisoned and every input between guards that
read as NaN.

Tolerances: ``dev`` is the deviation of the learner's fp32 torch path on the CPU from the float64 oracle for the case and
quantity; the kernel may deviate by a margin times dev (ppo_loss_util.MARGINS says where the margins come from).

Figures measured on the MI355X, kernel error over dev, largest over all cases of this file: see DESIGN.md 4y."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppo_loss_util as plu
from guard_util import GuardedBuffer, guard_bytes_for

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
NAN_BYTE = 0xFF
INPUTS = {"logits": np.float32, "old_logits": np.float32, "actions": np.int8, "old_logp": np.float32, "adv": np.float32,
          "values": np.float32, "targets": np.float32}
OUTPUTS = ("logp", "kl", "dlogits", "dvalues", "partials")
SCALARS = ("clip", "vf_clip", "vf_coeff", "ent_coeff")
EPS = float(np.finfo(np.float32).eps)


def _ids(s):
    return "T%d_rows%d_heads%d_groups%d" % s


def _lib():
    from dl_reference_models_amd import _lib as L

    return L, L.load()


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))


class RawPPO:
    """The call on guarded buffers: inputs between NaN guards, outputs poisoned before every call.  A case without the KL
    term has neither ``old_logits`` nor ``kl_coeff``: both pointers are NULL."""

    def __init__(self, inp, hp, groups=1):
        self.L, self.lib = _lib()
        self.T, self.R = inp["values"].shape
        self.heads, self.G = inp["actions"].shape[2], groups
        self.hp = dict(hp)
        self.buf = {}
        for k, dt in tuple(INPUTS.items()) + (("kl_coeff", np.float32),):
            if inp[k] is None:
                continue
            b = GuardedBuffer(inp[k].shape, dt, DEV, fill=NAN_BYTE, name=k)
            b.payload_view().copy_(torch.from_numpy(np.ascontiguousarray(inp[k], dtype=dt)))
            self.buf[k] = b
        self.parts = int(self.lib.mapf_ppo_partials(self.R, self.G))
        shapes = {k: (self.T, self.R) for k in ("logp", "kl", "dvalues")}
        shapes.update(dlogits=(self.T, self.R, self.heads * 5), partials=(self.parts, 5))
        for k, sh in shapes.items():
            slab = int(np.prod(sh[1:])) * 4
            self.buf[k] = GuardedBuffer(sh, np.float32, DEV, guard_bytes_for(min(slab, 1 << 20)), name=k)

    def ptr(self, k):
        return self.buf[k].ptr if k is not None and k in self.buf else None

    def call(self, T=None, rows=None, heads=None, groups=None, **over):
        a = {k: k for k in tuple(INPUTS) + OUTPUTS + ("kl_coeff",)}
        a.update({k: v for k, v in over.items() if k not in SCALARS})
        s = [C.c_float(over.get(k, self.hp[k])) for k in SCALARS]
        return self.lib.mapf_ppo_loss(self.T if T is None else T, self.R if rows is None else rows,
                                      self.heads if heads is None else heads, self.G if groups is None else groups,
                                      *(self.ptr(a[k]) for k in INPUTS), *s, self.ptr(a["kl_coeff"]),
                                      *(self.ptr(a[k]) for k in OUTPUTS), _stream())

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
            if k in null:
                self.buf[k].check(False, "pointer not passed")
            else:
                out[k] = self.buf[k].check(True, "call")
        return out

    def quantities(self, out):
        """Every quantity of ppo_loss_util.QUANTITIES from the payloads (the first four columns of the partials), and the
        loss terms per group: the partials added over a group's tiles (in float32, as the learner does) over its count."""
        q = {k: out[k].astype(np.float64) for k in plu.ELEMENTWISE}
        sums = torch.from_numpy(out["partials"]).view(self.G, -1, 5).sum(1).numpy().astype(np.float64) / (self.T * self.R // self.G)
        q.update(partials=out["partials"][:, :4].astype(np.float64), policy_loss=sums[:, 0], vf_loss=sums[:, 1], entropy=sums[:, 2],
                 kl_mean=sums[:, 3], total=sums[:, 4])
        return q


def _compare(c, q, what):
    line, worst = [], {}
    for k in plu.QUANTITIES:
        assert np.isfinite(q[k]).all(), (what, k)
        err, dev = float(np.abs(q[k] - c["want"][k]).max()), c["dev"][k]
        worst[k] = (err, dev)
        line.append(f"{k} {err:.3e} / {dev:.3e}" + (f" = {err / dev:.2f}" if dev > 0 else ""))
    print(f"ppo parity {what} T={c['T']} rows={c['rows']} heads={c['heads']} groups={c['groups']} {c['kind']} {c['settings']}: "
          + ", ".join(line))
    for k, (err, dev) in worst.items():
        assert err <= plu.MARGINS[k] * dev, (what, k, err, dev)
    # the loss terms are a group's partials added up and divided by its count: each partial within its bound, plus the fp32 sum
    G = c["groups"]
    n, count = q["partials"].shape[0] // G, c["T"] * c["rows"] // G
    for g in range(G):
        mine = q["partials"][g * n:(g + 1) * n]
        slack = (n * plu.MARGINS["partials"] * c["dev"]["partials"] + n * EPS * np.abs(mine).sum()) / count
        for k in plu.SUMMED:
            assert abs(q[k][g] - c["want"][k][g]) <= slack, (what, k, g, q[k][g], c["want"][k][g], slack)


def _autograd(c):
    """The same quantities through learner._PPOLoss and torch's autograd on the device."""
    from dl_reference_models_amd import learner as ln

    t = {k: (None if v is None else torch.from_numpy(v).to(DEV)) for k, v in c["inp"].items()}
    logits, values = t["logits"].clone().requires_grad_(True), t["values"].clone().requires_grad_(True)
    terms = ln._PPOLoss.apply(logits, values, t["actions"], t["old_logp"], t["adv"], t["targets"], t["old_logits"], t["kl_coeff"],
                              c["heads"], c["groups"], tuple(c["hp"][k] for k in SCALARS))
    dlogits, dvalues = torch.autograd.grad(terms[0].sum(), [logits, values])
    return dict(zip(("total", "policy_loss", "vf_loss", "entropy", "kl_mean"), terms), dlogits=dlogits, dvalues=dvalues)


def _parity(c, what="kernel"):
    raw = RawPPO(c["inp"], c["hp"], c["groups"])
    out = raw.run()
    q = raw.quantities(out)
    _compare(c, q, what)
    # the fifth column is the weighted sum of the other four per tile, rounded there
    hp, G = c["hp"], c["groups"]
    coeff = np.zeros(G) if c["inp"]["kl_coeff"] is None else c["inp"]["kl_coeff"].astype(np.float64)
    total = q["policy_loss"] + hp["vf_coeff"] * q["vf_loss"] - hp["ent_coeff"] * q["entropy"] + coeff * q["kl_mean"]
    mass = np.abs(out["partials"][:, :4]).reshape(G, -1).sum(1) * max(1.0, float(coeff.max())) / (c["T"] * c["rows"] // G)
    assert (np.abs(q["total"] - total) <= 8 * EPS * mass).all()
    auto = _autograd(c)  # the autograd function is the call, the sum of the partials and nothing else
    for k in ("dlogits", "dvalues"):
        assert _same(auto[k].cpu().numpy(), out[k]), k
    # its terms are the same partials added on the device, in fp32 and in another order: n terms, each rounding within eps
    # of the sum of their magnitudes (a term like the policy loss is a small sum of large partials), and one scaling
    n, count = out["partials"].shape[0] // G, c["T"] * c["rows"] // G
    for col, k in enumerate(plu.SUMMED + ("total",)):
        mag = np.abs(out["partials"][:, col].astype(np.float64)).reshape(G, n).sum(1) / count
        assert (np.abs(auto[k].detach().cpu().numpy() - q[k]) <= n * EPS * mag + 4 * EPS * np.abs(q[k])).all(), k
    return q, out


@pytest.mark.parametrize("shape", plu.SHAPES, ids=lambda s: "T%d_rows%d_heads%d_groups%d" % s)
def test_parity_with_the_float64_oracle(shape):
    _parity(plu.case(*shape))


def test_parity_at_the_reference_settings():
    """clip 0.05, vf_clip 10, 0.5, 0.001 and a KL coefficient of 0.2: what the reference's PPO trains with."""
    _parity(plu.case(2, 63, 3, 1, "plain", "REFERENCE"))


@pytest.mark.parametrize("shape", ((3, 96, 1, 3), (2, 130, 1, 2)), ids=lambda s: "T%d_rows%d_heads%d_groups%d" % s)
def test_a_group_equals_the_ungrouped_call_on_its_rows(shape):
    """Bitwise: what a tile computes does not depend on ``groups``, and both calls scale the gradients by 1 / (T rows of
    the group)."""
    c = plu.case(*shape)
    T, R, H, G = shape
    whole = RawPPO(c["inp"], c["hp"], G).run()
    tiles = whole["partials"].shape[0] // G
    for g in range(G):
        sub = {k: (v[g:g + 1] if k == "kl_coeff" else np.ascontiguousarray(v[:, g::G])) for k, v in c["inp"].items()}
        alone = RawPPO(sub, c["hp"], 1).run()
        for k in ("logp", "kl", "dlogits", "dvalues"):
            assert _same(whole[k][:, g::G], alone[k]), (g, k)
        assert _same(whole["partials"][g * tiles:(g + 1) * tiles], alone["partials"]), g
    assert not _same(whole["partials"][:tiles], whole["partials"][tiles:2 * tiles])


def test_without_a_coefficient_there_is_no_kl_term():
    c = plu.case(3, 96, 1, 3, "plain", "SETTINGS", False)
    assert c["inp"]["old_logits"] is None and c["inp"]["kl_coeff"] is None
    q, out = _parity(c)  # both pointers NULL
    assert not out["kl"].any() and not out["partials"][:, 3].any()
    full = plu.case(3, 96, 1, 3)  # the behaviour logits passed, the coefficient not: they are not read (NaN would show)
    raw = RawPPO(dict(full["inp"], kl_coeff=None), c["hp"], 3)
    raw.buf["old_logits"].poison(NAN_BYTE)
    again = raw.run()
    for k in OUTPUTS:
        assert _same(again[k], out[k]), k


def test_an_overflowing_ratio_clips():
    c = plu.case(2, 63, 3, 1, "overflow")
    pos = c["inp"]["adv"] > 0
    with np.errstate(over="ignore"):
        assert np.isinf(np.exp((c["want"]["logp"] - c["inp"]["old_logp"]).astype(np.float32))[pos]).all()  # +inf in fp32 there
    q, out = _parity(c)
    assert np.isfinite(out["dlogits"]).all() and np.isfinite(out["partials"]).all()
    # there the surrogate is A (1 + clip) and no policy gradient flows: what is left is the entropy and the KL term's
    d_plain = RawPPO(dict(c["inp"], adv=np.where(pos, 0, c["inp"]["adv"]).astype(np.float32),
                          old_logp=np.where(pos, c["want"]["logp"], c["inp"]["old_logp"]).astype(np.float32)), c["hp"]).run()
    assert _same(out["dlogits"][pos], d_plain["dlogits"][pos])
    want_pol = -(c["inp"]["adv"].astype(np.float64) * (1.0 + c["hp"]["clip"]))[pos].sum()
    got_pol = float(q["partials"][:, 0].sum()) - float(c["want"]["el"]["policy_loss"][~pos].sum())
    assert abs(got_pol - want_pol) <= 1e-4 * abs(want_pol)


def test_a_head_with_one_action_left():
    c = plu.case(5, 65, 3, 1, "one_left")
    for key, rows in (("logits", slice(1, None, 3)), ("old_logits", slice(2, None, 3))):
        lg = c["inp"][key].reshape(5, 65, 3, 5)[:, rows, 0]
        p32 = np.exp((lg - lg.max(axis=2, keepdims=True)).astype(np.float32))
        assert (p32 == 0).sum() == 4 * p32[..., 0].size, key  # four probabilities of those heads are exactly 0 in fp32
    q, out = _parity(c)
    for k in OUTPUTS:
        assert np.isfinite(out[k]).all(), k
    # an action of probability 0 has no entropy gradient (and no policy gradient: it was not taken); without the KL term
    # nothing is left of it, and of the one action left (p = 1) neither
    nokl = RawPPO(dict(c["inp"], kl_coeff=None, old_logits=None), c["hp"]).run()
    d = nokl["dlogits"].reshape(5, 65, 3, 5)[:, 1::3, 0]
    assert ((d == 0).sum(axis=2) >= 4).all()
    # with it, exactly the KL term's share c kl_coeff (p - q) = -c kl_coeff q is
    dk = out["dlogits"].reshape(5, 65, 3, 5)[:, 1::3, 0].astype(np.float64)
    lq = c["inp"]["old_logits"].reshape(5, 65, 3, 5)[:, 1::3, 0].astype(np.float64)
    qq = np.exp(lq - lq.max(axis=2, keepdims=True))
    qq /= qq.sum(axis=2, keepdims=True)
    taken = np.arange(5)[None, None, :] == c["inp"]["actions"][:, 1::3, 0, None]
    want = -float(c["inp"]["kl_coeff"][0]) * qq / (5 * 65)
    assert (want[~taken] < 0).all() and (np.abs(dk - want)[~taken] <= 1e-4 * np.abs(want)[~taken]).all()


def test_what_the_call_writes():
    c = plu.case(5, 65, 16)
    raw = RawPPO(c["inp"], c["hp"])
    full = raw.run()
    again = raw.run()
    for k, v in full.items():
        assert _same(again[k], v), k  # bitwise repeatable
    for null in [{k: None} for k in OUTPUTS] + [{k: None for k in OUTPUTS}]:
        got = raw.run(**null)
        for k, v in got.items():
            assert _same(v, full[k]), (null, k)
    for k in tuple(INPUTS) + ("kl_coeff",):  # inputs are read, never written
        assert raw.buf[k].guard_damage() is None and _same(raw.buf[k].array(), c["inp"][k]), k
    one = plu.case(2, 130, 1, 2)  # and the one-head path, which writes dlogits from the first pass, on two groups
    raw = RawPPO(one["inp"], one["hp"], 2)
    full = raw.run()
    for null in [{k: None} for k in OUTPUTS] + [{k: None for k in OUTPUTS}]:
        got = raw.run(**null)
        for k, v in got.items():
            assert _same(v, full[k]), (null, k)


# Fragments of one chunk and beyond (ppo_loss_util.LONG_SHAPES).  The kernel walks t in chunks of 32 steps and keeps g_logp of a
# chunk in LDS (s_g), which the next chunk's pass A overwrites; with more than one head two barriers separate the two.


@pytest.mark.parametrize("shape", plu.LONG_SHAPES, ids=_ids)
def test_parity_beyond_one_chunk(shape):
    _parity(plu.case(*shape))


@pytest.mark.parametrize("kind", ("overflow", "one_left"))
@pytest.mark.parametrize("shape", ((33, 65, 3, 1), (65, 33, 16, 1)), ids=_ids)
def test_parity_of_the_other_kinds_beyond_one_chunk(shape, kind):
    q, out = _parity(plu.case(*shape, kind))
    for k in OUTPUTS:
        assert np.isfinite(out[k]).all(), k


def test_parity_of_one_full_chunk_at_the_reference_settings():
    """T = 32: what ``Trainer`` and both training scripts run."""
    _parity(plu.case(32, 33, 1, 1, "plain", "REFERENCE"))


def test_parity_without_a_coefficient_beyond_one_chunk():
    """Pass C without ``head_kl``."""
    c = plu.case(33, 65, 3, 1, "plain", "SETTINGS", False)
    assert c["inp"]["old_logits"] is None and c["inp"]["kl_coeff"] is None
    q, out = _parity(c, "kernel without a coefficient")
    assert not out["kl"].any() and not out["partials"][:, 3].any()


def _tile_mass(c, T0=0, T1=None):
    """[tiles, 4] sums of the magnitudes of what a tile's partials add up, over steps T0 .. T1 - 1, and the number of
    elements of every tile.  Two fp32 sums of the same n numbers in two orders each lie within (n - 1) eps / 2 of the sum
    of their magnitudes of the exact sum, so within n eps of it of each other."""
    tiles = plu.tiles_of(c["rows"], c["groups"])
    el = c["want"]["el"]
    mass = np.array([[float(np.abs(el[k][T0:T1][:, idx]).sum()) for k in plu.SUMMED] for idx in tiles])
    count = np.array([len(idx) for idx in tiles]) * len(el["entropy"][T0:T1])
    return mass, count


@pytest.mark.parametrize("shape", ((65, 33, 16, 1), (40, 130, 1, 2)), ids=_ids)
def test_reversed_in_time_the_outputs_are_the_same_reversed(shape):
    """Bitwise: every per-element output depends on its own (t, row) alone and on the call's scale, not on the chunk it falls
    into nor on its place in it.  Reversed, step t is element T - 1 - t: a chunk of one step or of eight becomes the first
    instead of the last, and g_logp of a step passes through another element of LDS behind another chunk's."""
    c = plu.case(*shape)
    T, G = shape[0], shape[3]
    fwd = RawPPO(c["inp"], c["hp"], G).run()
    bwd = RawPPO(plu.reversed_in_time(c["inp"]), c["hp"], G).run()
    for k in plu.ELEMENTWISE:
        assert _same(fwd[k][::-1], bwd[k]), k
        assert not _same(fwd[k], bwd[k]), k  # (and time was reversed)
    mass, count = _tile_mass(c)  # the partials are the same sums in another order
    diff = np.abs(fwd["partials"][:, :4].astype(np.float64) - bwd["partials"][:, :4])
    print(f"ppo reversed T={T} rows={shape[1]} heads={shape[2]} groups={G}: partials differ by at most "
          f"{float((diff / (count[:, None] * EPS * mass)).max()):.2e} of the bound")
    assert (diff <= count[:, None] * EPS * mass).all()


def test_a_long_call_is_its_chunks_called_alone():
    """Bitwise for logp and kl: three calls on steps [0, 32), [32, 64) and [64, 65) give what the one call on 65 steps gives
    (dlogits and dvalues carry the call's 1 / (T rows): parity pins them).  The four sums of a tile are the slices' added."""
    shape = (65, 33, 16, 1)
    c = plu.case(*shape)
    whole = RawPPO(c["inp"], c["hp"]).run()
    added = np.zeros((whole["partials"].shape[0], 4))
    for a, b in ((0, 32), (32, 64), (64, 65)):
        part = RawPPO(plu.time_slice(c["inp"], a, b), c["hp"]).run()
        for k in ("logp", "kl"):
            assert _same(whole[k][a:b], part[k]), (k, a, b)
        added += part["partials"][:, :4].astype(np.float64)
    mass, count = _tile_mass(c)
    assert (np.abs(whole["partials"][:, :4] - added) <= count[:, None] * EPS * mass).all()
    assert (added[:, 1:] > 0.5 * mass[:, 1:]).all()  # (the three columns of one sign are sums of something)


def test_what_the_call_writes_beyond_one_chunk():
    """Every output pointer alone and all of them NULL, multi-head across a chunk edge: without ``dlogits`` pass C and its
    barriers are skipped, and no other output may change; without ``partials`` likewise."""
    c = plu.case(33, 65, 3, 1)
    raw = RawPPO(c["inp"], c["hp"])
    full = raw.run()
    for null in [{k: None} for k in OUTPUTS] + [{k: None for k in OUTPUTS}]:
        got = raw.run(**null)  # (checks every buffer not passed as untouched, guards included)
        for k, v in got.items():
            assert _same(v, full[k]), (null, k)
    for k in tuple(INPUTS) + ("kl_coeff",):
        assert raw.buf[k].guard_damage() is None and _same(raw.buf[k].array(), c["inp"][k]), k


@pytest.mark.parametrize("shape", ((2, 63, 3, 1), (2, 130, 1, 2)), ids=lambda s: "T%d_rows%d_heads%d_groups%d" % s)
def test_an_action_byte_out_of_range_is_clamped(shape):
    c = plu.case(*shape)
    inp = dict(c["inp"])
    wild = inp["actions"].copy()
    wild[inp["actions"] == 0] = -128
    wild[inp["actions"] == 4] = 127
    a, b = RawPPO(inp, c["hp"], shape[3]).run(), RawPPO(dict(inp, actions=wild), c["hp"], shape[3]).run()
    for k in a:
        assert _same(a[k], b[k]), k


def test_refused_arguments_launch_nothing():
    c = plu.case(3, 96, 1, 3)
    raw = RawPPO(c["inp"], c["hp"], 3)
    CFG = raw.L.MAPF_ERR_CONFIG
    raw.poison()
    torch.cuda.synchronize()
    bad = [{"T": 0}, {"T": -1}, {"rows": 0}, {"rows": -3}, {"heads": 0}, {"heads": 65}, {"heads": -1}, {"groups": 0}, {"groups": -1},
           {"groups": 5}, {"rows": 95}]
    bad += [{k: None} for k in INPUTS]  # (old_logits: a coefficient without the behaviour logits)
    bad += [{k: v} for k in SCALARS for v in (float("nan"), float("inf"), -0.5)]
    bad += [{"clip": 1.0}, {"clip": 1.5}]
    for b in bad:
        assert raw.call(**b) == CFG, b
    torch.cuda.synchronize()
    for k in OUTPUTS:
        raw.buf[k].check(False, "refused call")
    parts = raw.lib.mapf_ppo_partials
    assert parts(0, 1) == 0 and parts(65, 1) == 3 and parts(96, 3) == 3 and parts(130, 2) == 6
    raw.run()  # and the same object is accepted as it is


def test_the_autograd_function_refuses_what_the_kernel_cannot_walk():
    """A tensor on another device or of another shape is refused before any launch: the kernel takes raw pointers."""
    from dl_reference_models_amd import learner as ln

    c = plu.case(3, 96, 1, 3)
    t = {k: torch.from_numpy(v).to(DEV) for k, v in c["inp"].items()}
    order = ("logits", "values", "actions", "old_logp", "adv", "targets", "old_logits", "kl_coeff")
    scalars = tuple(c["hp"][k] for k in SCALARS)
    for k in order[2:]:
        with pytest.raises(ValueError, match=k):
            ln._PPOLoss.apply(*(t[j].cpu() if j == k else t[j] for j in order), 1, 3, scalars)
    for k in order:
        with pytest.raises(ValueError, match=k if k != "values" else "must be|groups"):
            ln._PPOLoss.apply(*(t[j][..., :-1] if j == k else t[j] for j in order), 1, 3, scalars)
    with pytest.raises(ValueError, match="groups"):
        ln._PPOLoss.apply(*(t[j] for j in order), 1, 5, scalars)
    total = ln._PPOLoss.apply(*(t[j].double() if j in ("logits", "values") else t[j] for j in order), 1, 3, scalars)[0]
    assert tuple(total.shape) == (3,) and torch.isfinite(total).all()  # floating point of another width: cast to what the kernel takes


def _first_call_capture():
    """The call captured as the very first call of a process, replayed on changed inputs and on a changed coefficient buffer
    (run as a script, see below)."""
    c = plu.case(3, 96, 1, 3)
    raw = RawPPO(c["inp"], c["hp"], 3)
    raw.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert raw.call() == 0
    other = plu.make_inputs(3, 96, 1, 3, seed=1)
    other["kl_coeff"] = (other["kl_coeff"] * np.float32(1.5)).astype(np.float32)
    for variant, inp in (("as captured", c["inp"]), ("changed inputs", dict(other, kl_coeff=c["inp"]["kl_coeff"])),
                         ("changed coefficient", dict(c["inp"], kl_coeff=other["kl_coeff"]))):
        want, got32 = plu.oracle(inp, c["hp"], 3), plu.torch_path32(inp, c["hp"], 3)
        want["partials"], got32["partials"] = plu._partials(plu.oracle, inp, c["hp"], 3), plu._partials(plu.torch_path32, inp, c["hp"], 3)
        cc = dict(c, inp=inp, want=want, got32=got32, kind=variant,
                  dev=plu.deviation(got32, want))
        plu.check_conditions(dict(cc, kind="plain"))
        for k in tuple(INPUTS) + ("kl_coeff",):
            raw.buf[k].payload_view().copy_(torch.from_numpy(np.ascontiguousarray(inp[k])))
        raw.poison()
        g.replay()
        torch.cuda.synchronize()
        q = raw.quantities({k: raw.buf[k].check(True, f"replay, {variant}") for k in OUTPUTS})
        _compare(cc, q, "replay " + variant)
        if variant == "changed coefficient":  # and the term moved with it: the weighted total is not the captured one's
            assert np.abs(q["total"] - first["total"]).min() > 1e-3 and _same(q["partials"][:, :4], first["partials"][:, :4])
        elif variant == "as captured":
            first = q
    print("first-call capture ok")


def test_graph_capture_from_the_very_first_call():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first-call capture ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _first_call_capture()
