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
# every (kind, shape, regime, recurrent, sample, variant) the GPU tests run
GPU_CASES = ([(k, s, r, True, m, None) for k, s in SHAPES for r in ru.NEW_REGIMES for m in (False, True)]
             + [(k, ru.FEED_FORWARD_SHAPE[k], "peaked", False, m, None) for k in ("agent", "joint") for m in (False, True)]
             + [(k, ru.ABI_SHAPE[k], "default", True, True, v) for k in ("agent", "joint") for v in ru.VARIANTS])


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
    if key[0] == "joint":
        assert und_dec <= ju.MAX_UNDECIDED_DECISIONS and und_rows <= ju.MAX_UNDECIDED_ROWS, (und_dec, und_rows)
    else:
        assert und_rows <= ru.MAX_UNDECIDED_AGENT_ROWS, und_rows
    line, fails = ru.compare(c, ru.restate32(c))
    print(line + f"; other-order / module deviation {c['dev_other'] / c['dev_module']:.2f}, |logit| before the mask up to "
          f"{c['max_abs_logit']:.1f}, |h| up to {c['max_abs_h']:.4f}")
    assert not fails, fails
    for s in c["steps"]:  # the whole-row masks: row 0 all 0, row 1 all 0.5; finite expectations throughout
        if key[0] == "joint" or key[1][3]:
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
