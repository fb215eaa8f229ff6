"""Both act kernels (mapf_policy_act, mapf_jpolicy_act, through the raw C ABI) beyond a freshly initialised net: the
regime cases of regime_util (scaled parameters until gates saturate and logits pass the range of fp32 exp, whole rows
masked 0 or 0.5, unchained state) and the paths the ABI states but no other parity case walks (both start arrays with
different flags, prev_action bytes outside 0..4, draw counters across the top of their range, seeds with the top bit set),
against the float64 restatement of the rule.  Buffers as in test_policy_gpu / test_joint_policy_gpu: the observation
between NaN guards, outputs poisoned, state guarded and loaded from the case before each call.

The assertions are regime_util.compare's, with the project's margins (16 x dev, 32 x dev_logp on every row against the
restatement's log-probability of the kernel's own action); test_regimes_host runs the same function on the float32
restatement and on four mutants of it.

One joint case more runs `hot`, recurrent and sampled, at regime_util.JOINT_SPLIT_SHAPE: of the shapes that walk the splits
of the joint kernel's schedule (joint_policy_util.SPLIT_SHAPES) the one with the most head tiles and a partly filled upper
quarter of fc1's K.

Kind "wide" runs the same cases on the 256-256 feed-forward net through the wide act kernel (RawWide of
test_wide_joint_gpu: h and c poisoned and checked untouched, since that net has no state); the recurrent inputs of a case
are passed all the same, a feed-forward handle must not read them."""

import numpy as np
import pytest
import torch

import regime_util as ru
from guard_util import GuardedBuffer
from test_joint_policy_gpu import RawJoint
from test_policy_gpu import DEV, NAN_BYTE, RawPolicy, _dev
from test_wide_joint_gpu import RawWide

pytestmark = pytest.mark.gpu

OUTPUTS = ("action", "logp", "value", "logits")


def _load(buf, a, dtype):
    """A guarded state buffer refilled with poison, then its payload loaded with ``a`` (bytes: torch has no uint32 copy)."""
    buf.poison()
    raw = np.ascontiguousarray(a, dtype=dtype).view(np.uint8).reshape(-1)
    buf.arena[buf.offset:buf.offset + buf.nbytes].copy_(torch.from_numpy(raw).to(DEV))
    return raw


def _run_case(c):
    """Every step of an unchained case on the device; returns per-step snapshots in the shape regime_util.compare takes."""
    kind = c["kind"]
    rows, _N, per, L = ru.geometry(kind, c["shape"])
    pol = {"agent": lambda: RawPolicy(c["module"], rows, per), "joint": lambda: RawJoint(c["module"], rows),
           "wide": lambda: RawWide(c["module"], rows)}[kind]()
    obs_buf = GuardedBuffer((rows, L), np.float32, DEV, fill=NAN_BYTE, name="obs")
    got = []
    for t, s in enumerate(c["steps"]):
        obs_buf.payload_view().copy_(_dev(s["obs"], np.float32))
        pa = _dev(s["prev_action"], np.int8)
        pr = _dev(s["prev_reward"], np.float32 if kind == "agent" else np.float64)
        sa, sb = (None if s[k] is None else _dev(s[k], np.uint8) for k in ("start_a", "start_b"))
        pol.poison_outputs()
        loaded = {}
        if c["recurrent"]:
            loaded["h"], loaded["c"] = _load(pol.buf["h"], s["h_in"], np.float32), _load(pol.buf["c"], s["c_in"], np.float32)
        if c["sample"]:
            loaded["draws"] = _load(pol.buf["draws"], s["draws_in"], np.uint32)
        else:
            pol.buf["draws"].poison()  # greedy mode neither reads nor writes draws
        mode = (1 if c["sample"] else 0) | (2 if s["peek"] else 0)
        if kind == "wide":
            assert pol.act(obs_buf.ptr, mode, s["seed"], unread=(pa, pr, sa, sb)) == 0
        else:
            assert pol.act(obs_buf.ptr, pa, pr, sa, sb, mode, s["seed"]) == 0
        torch.cuda.synchronize()
        what = f"step {t}"
        snap = {k: pol.buf[k].check(True, what) for k in OUTPUTS}
        if c["recurrent"]:
            snap["h"], snap["c"] = pol.buf["h"].check(True, what), pol.buf["c"].check(True, what)
        elif kind == "wide":  # h and c are still the poison RawWide filled them with
            pol.buf["h"].check(False, what), pol.buf["c"].check(False, what)
        else:  # a feed-forward policy has no state to write (the buffers were zeroed, so look at the bytes)
            assert not pol.buf["h"].array().any() and not pol.buf["c"].array().any()
            assert pol.buf["h"].guards_intact() and pol.buf["c"].guards_intact()
        if c["sample"]:
            snap["draws"] = pol.buf["draws"].check(True, what)
        else:
            snap["draws"] = None
            pol.buf["draws"].check(False, what + ", greedy")
        if s["peek"]:  # every output, no state and no draw counter
            for k, raw in loaded.items():
                assert np.array_equal(np.ascontiguousarray(snap[k]).view(np.uint8).reshape(-1), raw), (k, what, "PEEK wrote state")
        got.append(snap)
    pol.close()
    return got


def _check(c):
    got = _run_case(c)
    line, fails = ru.compare(c, got)
    print(line)
    assert not fails, fails
    return got


def _id(v):
    return str(v).replace(" ", "")


PARITY = ([("agent", s, r, m) for s in ru.AGENT_SHAPES for r in ru.NEW_REGIMES for m in (False, True)]
          + [("joint", s, r, m) for s in ru.JOINT_SHAPES for r in ru.NEW_REGIMES for m in (False, True)]
          + [ru.JOINT_SPLIT_CASE[:3] + (True,)]  # sampled; test_parity_in_the_regime runs kind "joint" recurrent
          + [("wide", s, r, m) for s in ru.WIDE_SHAPES for r in ru.NEW_REGIMES for m in (False, True)])


@pytest.mark.parametrize("kind,shape,regime,sample", PARITY, ids=_id)
def test_parity_in_the_regime(kind, shape, regime, sample):
    c = ru.case(kind, shape, regime, kind != "wide", sample)
    got = _check(c)
    for t, g in enumerate(got):
        if c["sample"]:
            assert (g["draws"] == t + 1).all()
        if kind != "agent" or shape[3]:  # the fully masked row 0 and the 0.5-mask row 1
            assert np.isfinite(g["logp"][:2]).all() and np.isfinite(g["logits"][:2]).all()


@pytest.mark.parametrize("kind", ("agent", "joint"))
@pytest.mark.parametrize("sample", (False, True))
def test_feed_forward_parity_when_peaked(kind, sample):
    _check(ru.case(kind, ru.FEED_FORWARD_SHAPE[kind], "peaked", False, sample))


@pytest.mark.parametrize("kind", ("agent", "joint"))
def test_both_start_arrays_are_ored(kind):
    c = ru.case(kind, ru.ABI_SHAPE[kind], "default", True, True, "both_starts")
    got = _check(c)
    # a row flagged in either array alone has left its state behind: h' is that of h = c = 0, far from the carried one's
    s = c["steps"][1]
    only_b = ru.start_rows(kind, c["shape"], None, s["start_b"]) & ~ru.start_rows(kind, c["shape"], s["start_a"], None)
    assert only_b.sum() >= 2 and np.abs(s["h_in"][only_b]).max() > 1e-2
    assert np.abs(got[1]["h"][only_b] - s["h"][only_b]).max() <= 16 * c["dev"]


@pytest.mark.parametrize("kind", ("agent", "joint"))
def test_prev_action_bytes_outside_0_to_4_give_no_one_hot_entry(kind):
    _check(ru.case(kind, ru.ABI_SHAPE[kind], "default", True, True, "bad_bytes"))


@pytest.mark.parametrize("kind", ru.KINDS)
def test_draw_counters_across_the_top_of_their_range(kind):
    c = ru.case(kind, ru.ABI_SHAPE[kind], "default", kind != "wide", True, "counters")
    got = _check(c)  # noise per the rule with that counter (the decided actions), counters afterwards as the rule leaves them
    for g, s in zip(got, c["steps"]):
        d = s["draws_in"].astype(np.uint64)
        want = d if s["peek"] else (d + 1) % (1 << 32)
        assert np.array_equal(g["draws"].astype(np.uint64), want)
        assert (g["draws"][s["draws_in"] == 0xFFFFFFFF] == (0xFFFFFFFF if s["peek"] else 0)).all()
    assert c["steps"][-1]["peek"] and not c["steps"][0]["peek"]


@pytest.mark.parametrize("kind", ru.KINDS)
def test_seeds_with_the_top_bit_set(kind):
    c = ru.case(kind, ru.ABI_SHAPE[kind], "default", kind != "wide", True, "seeds")
    assert {s["seed"] for s in c["steps"]} == set(ru.TOP_SEEDS)
    _check(c)
