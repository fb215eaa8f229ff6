"""The regime cases of regime_util without a GPU: the inputs are proved before any device sees them.  Every case used by
test_policy_regimes_gpu / test_lstm_seq_gpu has a finite positive ``dev`` and stays under the existing caps on undecided
decisions; every regime reaches what it is for; and four mutants of the float32 restatement, each a defect that every
parity case from before these regimes lets through, pass their ``default`` case and fail their new one under the very
assertions the GPU tests make (regime_util.compare)."""

import numpy as np
import pytest

import joint_policy_util as ju
import learner_util as lu
import policy_util as pu
import regime_util as ru

SHAPES = [("agent", s) for s in ru.AGENT_SHAPES] + [("joint", s) for s in ru.JOINT_SHAPES]
WIDE_VARIANTS = ("counters", "seeds")
# every (kind, shape, regime, recurrent, sample, variant) the GPU tests run
GPU_CASES = ([(k, s, r, True, m, None) for k, s in SHAPES for r in ru.NEW_REGIMES for m in (False, True)]
             + [ru.JOINT_SPLIT_CASE]
             + [(k, ru.FEED_FORWARD_SHAPE[k], "peaked", False, m, None) for k in ("agent", "joint") for m in (False, True)]
             + [(k, ru.ABI_SHAPE[k], "default", True, True, v) for k in ("agent", "joint") for v in ru.VARIANTS]
             # the wide net is feed-forward: the two variants that need no state (wide_joint_gpu pins what it must not read)
             + [("wide", s, r, False, m, None) for s in ru.WIDE_SHAPES for r in ru.NEW_REGIMES for m in (False, True)]
             + [("wide", ru.ABI_SHAPE["wide"], "default", False, True, v) for v in WIDE_VARIANTS])


def _id(v):
    return str(v).replace(" ", "")


@pytest.mark.parametrize("key", GPU_CASES, ids=_id)
def test_case_is_inside_the_caps_and_the_restatement_passes_it(key):
    """dev finite and positive, the undecided shares under the caps (conditions on the inputs, not measurements), and the
    float32 restatement itself inside every margin the kernels are held to."""
    c = ru.case(*key)
    assert np.isfinite(c["dev"]) and 0 < c["dev"] < 1e-2
    assert 0 < c["dev_module"] and 0 < c["dev_other"]
    und_dec, und_rows = ru.undecided(c)
    if key[0] != "agent":
        assert und_dec <= ju.MAX_UNDECIDED_DECISIONS and und_rows <= ju.MAX_UNDECIDED_ROWS, (und_dec, und_rows)
    else:
        assert und_rows <= ru.MAX_UNDECIDED_AGENT_ROWS, und_rows
    line, fails = ru.compare(c, ru.restate32(c))
    print(line + f"; other-order / module deviation {c['dev_other'] / c['dev_module']:.2f}, |logit| before the mask up to "
          f"{c['max_abs_logit']:.1f}, |h| up to {c['max_abs_h']:.4f}; undecided shares: decisions {und_dec:.4%}, rows {und_rows:.4%}")
    assert not fails, fails
    for s in c["steps"]:  # the whole-row masks: row 0 all 0, row 1 all 0.5; finite expectations throughout
        if key[0] != "agent" or key[1][3]:
            N = ru.geometry(key[0], key[1])[1]
            assert (s["obs"][0, -5 * N:] == 0).all() and (s["obs"][1, -5 * N:] == 0.5).all()
        assert np.isfinite(s["logits"]).all() and np.isfinite(s["logp"]).all()
        assert s["draws_out"].dtype == np.uint32


@pytest.mark.parametrize("kind,shape", SHAPES, ids=_id)
def test_regimes_reach_what_they_are_for(kind, shape):
    for sample in (False, True):
        peaked, saturated, hot, default = (ru.case(kind, shape, r, True, sample) for r in ("peaked", "saturated", "hot", "default"))
        assert all(np.abs(s["logits"]).max() > 100 for s in peaked["steps"]) and peaked["max_abs_logit"] > 100
        assert saturated["max_abs_h"] > 0.99
        assert default["max_abs_logit"] < 1 < hot["max_abs_logit"] < saturated["max_abs_logit"] < 88 < peaked["max_abs_logit"]
        assert default["dev"] < 1e-5  # the sanity bound of the existing parity tests holds in their regime only
    ff = ru.case(kind, ru.FEED_FORWARD_SHAPE[kind], "peaked", False, True)
    assert all(np.abs(s["logits"]).max() > 100 for s in ff["steps"])


def test_scale_params():
    a, b = pu.make_module(33, True, True), ru.scale_params(pu.make_module(33, True, True), 4, 16)
    for (name, v), w in zip(a.state_dict().items(), b.state_dict().values()):
        assert np.array_equal(w.numpy(), v.numpy() * (16 if name.split(".")[0] in ("pi", "vf") else 4)), name
    assert ru.REGIMES == {"default": (1, 1), "hot": (4, 16), "saturated": (8, 64), "peaked": (8, 256)}


def test_the_variants_carry_what_they_say():
    for kind in ("agent", "joint"):
        shape = ru.ABI_SHAPE[kind]
        rows, N, per, _L = ru.geometry(kind, shape)
        both = ru.case(kind, shape, "default", True, True, "both_starts")
        for s in both["steps"]:
            a, b = s["start_a"] != 0, s["start_b"] != 0
            assert (a & ~b).sum() >= 2 and (b & ~a).sum() >= 2 and (a & b).sum() == 1 and (a & b)[32 // per]
            assert np.array_equal(ru.start_rows(kind, shape, s["start_a"], s["start_b"]), np.repeat(a | b, per))
        bad = ru.case(kind, shape, "default", True, True, "bad_bytes")
        seen = set()
        for t, s in enumerate(bad["steps"]):
            pa = s["prev_action"].reshape(rows, N)
            seen |= set(np.unique(pa[(pa < 0) | (pa > 4)]).tolist())
            if t in ru.START_STEPS:
                srow = ru.start_rows(kind, shape, s["start_a"], s["start_b"])
                assert srow.any() and ((pa[srow] < 0) | (pa[srow] > 4)).all()
        assert seen == set(ru.BAD_BYTES)
        cnt = ru.case(kind, shape, "default", True, True, "counters")
        for t, s in enumerate(cnt["steps"]):
            for tile in (s["draws_in"][:32], s["draws_in"][32:]):
                assert set(ru.TOP_COUNTERS) <= set(tile.tolist())
            want = s["draws_in"] if s["peek"] else ((s["draws_in"].astype(np.uint64) + 1) % (1 << 32)).astype(np.uint32)
            assert np.array_equal(s["draws_out"], want) and s["peek"] == (t == ru.STEPS - 1)
            # the noise of the rule, once more in Python integers, on a row of each counter
            g = ru.noise(kind, s["seed"], rows, s["draws_in"], N)
            for row in (0, 2, 4, 6, 34):
                d = int(s["draws_in"][row])
                for k in range(5 * N):
                    ref = pu.gumbel_int(s["seed"], row, d, k) if kind == "agent" else ju.gumbel_int(s["seed"], row, d, k // 5, k % 5)
                    assert g[row, k] == pytest.approx(ref, rel=1e-15)
        seeds = ru.case(kind, shape, "default", True, True, "seeds")
        assert [s["seed"] for s in seeds["steps"]] == [ru.TOP_SEEDS[t % 2] for t in range(ru.STEPS)]
        s = seeds["steps"][1]
        g = ru.noise(kind, s["seed"], rows, s["draws_in"], N)
        ref = pu.gumbel_int(s["seed"], 33, 1, 3) if kind == "agent" else ju.gumbel_int(s["seed"], 33, 1, 0, 3)
        assert g[33, 3] == pytest.approx(ref, rel=1e-15)


# mutant -> (the case of today's regime it passes, the new case it fails): keys of regime_util.case after the kind and shape
MUTANTS = {"no_max": (("default", True, True, None), ("peaked", True, True, None)),
           "start_a_only": (("default", True, True, None), ("default", True, True, "both_starts")),
           "wrap_bytes": (("default", True, True, None), ("default", True, True, "bad_bytes")),
           "counter31": (("default", True, True, None), ("default", True, True, "counters"))}


@pytest.mark.parametrize("kind", ("agent", "joint"))
@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_mutant_passes_default_and_fails_its_new_case(kind, mutant):
    shape = ru.ABI_SHAPE[kind]
    old, new = (ru.case(kind, shape, *k) for k in MUTANTS[mutant])
    _line, fails = ru.compare(old, ru.restate32(old, mutant))
    assert not fails, fails
    # ... and the existing chained cases say nothing either: their inputs never reach the mutated path
    c = (pu.case(shape, True, True) if kind == "agent" else ju.case(shape, True, True))
    assert all(int(s["logits"].max()) < 15 for s in c["steps"]) and c["prev_action"].min() >= 0 and c["prev_action"].max() <= 4
    _line, fails = ru.compare(new, ru.restate32(new, mutant))
    print(f"{kind} {mutant}: {fails[:4]}")
    assert fails
    if mutant == "no_max":
        assert all("logp not finite" in f or f.startswith("logp") for f in fails), fails
        got = ru.restate32(old, mutant)
        assert all(np.isfinite(g["logp"]).all() for g in got)
    _line, fails = ru.compare(new, ru.restate32(new))
    assert not fails, fails


# ---- the wide net ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ru.WIDE_SHAPES, ids=_id)
def test_wide_regimes_reach_what_they_are_for(shape):
    import wide_joint_util as wu

    assert set(ru.JOINT_SHAPES) <= set(ru.WIDE_SHAPES) and all(s in wu.SHAPES for s in ru.WIDE_SHAPES)
    assert any(n % 2 and n >= 3 for s in ru.WIDE_SHAPES for n in wu.fc1_groups(s[1] * s[2]))  # one odd tail behind the loop
    for sample in (False, True):
        peaked, saturated, hot, default = (ru.case("wide", shape, r, False, sample) for r in ("peaked", "saturated", "hot", "default"))
        assert default["cfg"] == {"grid_cells": shape[1] * shape[2], "num_agents": shape[3], "recurrent": False, "hidden": 256}
        assert all(np.abs(s["logits"]).max() > 100 for s in peaked["steps"]) and peaked["max_abs_logit"] > 100
        # the heads sum 256 inputs and have no LSTM in front of them, so a regime's logits lie above the 64-wide net's:
        # already "saturated" is past the range of fp32 exp (88)
        assert default["max_abs_logit"] < 1.5 < hot["max_abs_logit"] < 88 < saturated["max_abs_logit"] < peaked["max_abs_logit"]
        assert default["dev"] < 1e-5 and max(np.abs(s["logits"]).max() for s in default["steps"]) < 15
        # the inputs are the wide kind's own, not the joint case's
        joint = ru.case("joint", shape, "hot", True, sample) if shape in ru.JOINT_SHAPES else None
        assert joint is None or not np.array_equal(joint["steps"][0]["obs"], hot["steps"][0]["obs"])


def test_a_recurrent_wide_case_is_refused():
    with pytest.raises(ValueError, match="feed-forward only"):
        ru.case("wide", ru.ABI_SHAPE["wide"], "hot", True, True)
    with pytest.raises(ValueError, match="feed-forward only"):
        ru.case("wide", ru.ABI_SHAPE["wide"])  # the default is recurrent


def test_the_wide_variants_carry_what_they_say():
    shape = ru.ABI_SHAPE["wide"]
    rows, N, _per, _L = ru.geometry("wide", shape)
    cnt = ru.case("wide", shape, "default", False, True, "counters")
    for t, s in enumerate(cnt["steps"]):
        for tile in (s["draws_in"][:32], s["draws_in"][32:64], s["draws_in"][64:]):
            assert set(tile.tolist()) & set(ru.TOP_COUNTERS)
        assert set(ru.TOP_COUNTERS) <= set(s["draws_in"][:32].tolist()) and set(ru.TOP_COUNTERS) <= set(s["draws_in"][32:].tolist())
        want = s["draws_in"] if s["peek"] else ((s["draws_in"].astype(np.uint64) + 1) % (1 << 32)).astype(np.uint32)
        assert np.array_equal(s["draws_out"], want) and s["peek"] == (t == ru.STEPS - 1)
        g = ru.noise("wide", s["seed"], rows, s["draws_in"], N)
        for row in (0, 2, 4, 6, 34):  # the noise of the rule, once more in Python integers, on a row of each counter
            for k in range(5 * N):
                assert g[row, k] == pytest.approx(ju.gumbel_int(s["seed"], row, int(s["draws_in"][row]), k // 5, k % 5), rel=1e-15)
    seeds = ru.case("wide", shape, "default", False, True, "seeds")
    assert [s["seed"] for s in seeds["steps"]] == [ru.TOP_SEEDS[t % 2] for t in range(ru.STEPS)]
    s = seeds["steps"][1]
    assert ru.noise("wide", s["seed"], rows, s["draws_in"], N)[33, 3] == pytest.approx(ju.gumbel_int(s["seed"], 33, 1, 0, 3), rel=1e-15)


@pytest.mark.parametrize("mutant", ("no_max", "counter31"))  # the two that apply to a feed-forward net
def test_wide_mutant_passes_default_and_fails_its_new_case(mutant):
    import wide_joint_util as wu

    shape = ru.ABI_SHAPE["wide"]
    old, new = (ru.case("wide", shape, *((k[0], False) + k[2:])) for k in MUTANTS[mutant])
    _line, fails = ru.compare(old, ru.restate32(old, mutant))
    assert not fails, fails
    # ... and the wide kernel's own parity cases say nothing either: a fresh net, counters below six
    c = wu.case(shape, True)
    assert all(np.abs(s["logits"]).max() < 15 for s in c["steps"])
    _line, fails = ru.compare(new, ru.restate32(new, mutant))
    print(f"wide {mutant}: {fails[:4]}")
    assert fails
    if mutant == "no_max":
        assert all("logp not finite" in f or f.startswith("logp") for f in fails), fails
    _line, fails = ru.compare(new, ru.restate32(new))
    assert not fails, fails


def _sha(a):
    import hashlib

    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


# (obs of all steps, the restatement's logits of all steps rounded to float32, draws_in of all steps) as the cases stood
# before the kind "wide" joined the rng key.  The float64 logits are hashed after rounding to float32: the order in which a
# BLAS sums a float64 product moves its last bits (some 1e-16 relative), which that rounding hides on all but one value in
# about 1e9 and any change of the inputs or the parameters does not.
CASES_BEFORE_WIDE = {
    ("agent", (65, 5, 33, True), "hot", True, True, None):
        ("105b2eadb47dc1dadcd18815d2bf18105aa8c88fae615b756efb549c56d0a861", "f8bc99b9f4e54d2c4fea259a8d0b7b0f3c6c2ab4d319368cf501640310bc573d",
         "4b374f4808334311f65c198da6a840c3bebfb5ee94eb76a884d793821d28ecef"),
    ("joint", (33, 5, 7, 3), "hot", True, True, None):
        ("25bcc532890274001f2e90769d43dc94ab98c6a4059ed2de0207ea1e69f77ce2", "fd2a3b214d2ca342f4b2144add8ec95a274af91edfefa48018f055353a22040d",
         "72f83af9276b576677c75a2e2b0a49619a34c9a6727043399dfe2052b4b7ca9b"),
    ("joint", (65, 16, 16, 4), "default", True, True, "counters"):
        ("4c579ba697f62273d91d2f75ca23bd8d9f4cb1e842acc39d1aefa7eafb0a0ee7", "8ea51031a26af1badb00f95af84f3f73a0dba383253ba6c8aadd7c3d319764d9",
         "26c63c9ac2d0e3101339df63b6ebb87e5f31a252b3f54450188abd1196567fc4")}


@pytest.mark.parametrize("key", list(CASES_BEFORE_WIDE), ids=_id)
def test_the_agent_and_joint_cases_are_what_they_were(key):
    c = ru.case(*key)
    got = (_sha(np.stack([s["obs"] for s in c["steps"]])), _sha(np.stack([s["logits"] for s in c["steps"]]).astype(np.float32)),
           _sha(np.stack([s["draws_in"] for s in c["steps"]])))
    assert got == CASES_BEFORE_WIDE[key]
    assert ru.KINDS[:2] == ("agent", "joint")  # their entries in the rng key


def test_forward64_drops_a_prev_action_byte_outside_0_to_4():
    m = pu.make_module(33, True, True)
    p, cfg = pu.params64(m), m.config()
    rng = np.random.default_rng(3)
    obs = rng.random((8, 33)).astype(np.float32)
    bad = np.array(ru.BAD_BYTES * 2, np.int8)
    h = rng.uniform(-1, 1, (8, 64))
    got = pu.forward64(p, cfg, obs, bad, None, None, (h, h))
    for k in range(5):  # none of the five one-hot columns: the same as a zero column, which no valid byte gives
        assert np.abs(got[0] - pu.forward64(p, cfg, obs, np.full(8, k, np.int8), None, None, (h, h))[0]).max() > 1e-3
    q = dict(p)
    q["lstm.weight_ih"] = p["lstm.weight_ih"].copy()
    q["lstm.weight_ih"][:, 64:69] = 0.0
    want = pu.forward64(q, cfg, obs, np.zeros(8, np.int8), None, None, (h, h))
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2][0], want[2][0])
    with pytest.raises(Exception):  # the torch module keeps raising on such input (its docstring says so)
        m(__import__("torch").from_numpy(obs), __import__("torch").from_numpy(bad))


# ---- the LSTM sequence cases ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ru.LSTM_REGIMES))
def test_lstm_case(name):
    c = ru.lstm_case(name)
    T, R, _sx, _sw, _fb = ru.LSTM_REGIMES[name]
    assert c["inp"]["xg"].shape == (T, R, 256) and T * R <= 128 * 33 and set(c["dev"]) == set(lu.QUANTITIES)
    assert 0.01 < (c["inp"]["reset"] != 0).mean() < 0.06
    line = []
    for k in lu.QUANTITIES:
        assert np.isfinite(c["want"][k]).all(), k
        assert np.isfinite(c["dev"][k]) and 0 < c["dev"][k] < 1e-3, (k, c["dev"][k])
        assert c["dev_loop"][k] > 0 and c["dev_perm"][k] > 0
        line.append(f"{k} dev {c['dev'][k]:.3e} (relabelled / loop {c['dev_perm'][k] / c['dev_loop'][k]:.2f})")
    gi = c["want"]["gates"][:, :, :64]
    sat = float(((gi < 1e-4) | (gi > 1 - 1e-4)).mean())
    print(f"lstm regime {name} T={T} rows={R}: G in [{c['G'].min():.1f}, {c['G'].max():.1f}], |c| up to {np.abs(c['want']['c']).max():.1f}, "
          f"input gate saturated on {100 * sat:.1f} %; " + ", ".join(line))
    if name == "overflow":
        assert c["G"].min() < -89  # expf(-x) overflows to +inf in the kernels' sigmoid
    if name == "saturated":
        assert sat >= 0.30
    if name == "long":
        assert np.abs(c["G"]).max() < 8  # today's regime, four times today's longest sequence


def test_the_stable_sigmoid_is_the_sigmoid_with_finite_gradients():
    import torch

    x = torch.tensor([-200.0, -89.0, -1.5, 0.0, 2.0, 95.0, 200.0], dtype=torch.float32, requires_grad=True)
    y = ru.stable_sig(x)
    (g,) = torch.autograd.grad(y.sum(), x)
    x64 = x.detach().double()
    assert torch.isfinite(g).all() and torch.allclose(y.double(), torch.sigmoid(x64), rtol=1e-6, atol=1e-45)
    assert torch.allclose(g.double(), torch.sigmoid(x64) * torch.sigmoid(-x64), rtol=1e-5, atol=1e-45) and g[3] == 0.25
    (g_plain,) = torch.autograd.grad(lu._sig(x).sum(), x)
    assert not torch.isfinite(g_plain).all()  # why the overflow case cannot take learner_util._sig behind dev
