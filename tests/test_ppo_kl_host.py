"""PPO's adaptive KL penalty without a GPU: the torch statement of ``PPOLearner.losses`` with the KL term against
ppo_loss_util's float64 oracle on synthetic fragments (shared and one policy per agent), the adaptation rule, what a
learner built with defaults still returns, the error that names ``keep_logits``, the conditions of the case generator, and
the C ABI's bookkeeping (symbols, header, constants, the argument checks that need no device)."""

import copy
import os
import re

import numpy as np
import pytest
import torch

import dte_util as du
import learner_util as lu
import policy_util as pu
import ppo_loss_util as plu

T, B, N, L = 6, 4, 3, 16


def _fragment(seed=3):
    """A synthetic fragment with behaviour logits: recorded log-probabilities far enough from the module's that the ratio
    clip binds, value targets far enough that the value clip does."""
    frag = lu.synthetic_fragment(T, B, N, L, mask=True, seed=seed)
    rng = np.random.default_rng(seed + 100)
    frag["logits"] = torch.from_numpy((1.5 * rng.standard_normal((T, B, N, 5))).astype(np.float32))
    adv = torch.from_numpy(rng.standard_normal((T, B, N)))
    targets = torch.from_numpy(rng.standard_normal((T, B, N)))
    return frag, adv, targets


def _by_hand(module, frag64, adv, targets, hp, coeff, groups):
    """ppo_loss_util.ppo_terms on T chained ``module.forward`` calls, float64: the loss terms per group and the flat gradient."""
    module.zero_grad()
    logits, values = lu.chained_forward(module, frag64)
    R = B * N
    out = plu.ppo_terms(logits, values, frag64["logits"].reshape(T, R, 5), frag64["actions"].reshape(T, R, 1),
                        frag64["logp"].reshape(T, R), adv.reshape(T, R), targets.reshape(T, R), coeff, hp, groups)
    out["total_loss"].backward()
    out["gradient"] = torch.cat([p.grad.reshape(-1) for p in module.parameters()]).clone()
    return out


@pytest.mark.parametrize("per_agent", (False, True), ids=("shared", "per_agent"))
def test_torch_losses_with_kl_equal_the_float64_oracle(per_agent):
    from dl_reference_models_amd import learner as ln

    frag, adv, targets = _fragment()
    frag64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}
    module = (du.make_per_agent(N, L, True, True, seed=2) if per_agent else pu.make_module(L, True, True, seed=2)).double().train()
    G = N if per_agent else 1
    hp = {"clip": 0.2, "vf_clip": 0.8, "vf_coeff": 0.7, "ent_coeff": 0.03}
    learner = ln.PPOLearner(module, fused=False, kl_coeff=0.2, **hp)
    assert learner.kl_coeff.dtype == torch.float32 and tuple(learner.kl_coeff.shape) == (G,)  # (CPU tensors take the torch ops whatever fused_objective says)
    learner.kl_coeff.copy_(torch.from_numpy(plu.group_coeffs(G, 0.2)))
    want = _by_hand(copy.deepcopy(module), frag64, adv, targets, hp, learner.kl_coeff.double(), G)
    ratio, err = want["ratio"].detach(), want["err"].detach()
    assert ((ratio > 1.2) | (ratio < 0.8)).double().mean() > 0.2 and 0.1 < (err > 0.8).double().mean() < 0.9  # both clips bind
    assert float(want["kl_mean"].detach().min()) > 1e-2

    module.zero_grad()
    terms = learner.losses(frag64, adv, targets)
    terms["total_loss"].backward()
    grad = torch.cat([p.grad.reshape(-1) for p in module.parameters()])
    assert list(terms)[:5] == ["total_loss", "policy_loss", "vf_loss", "entropy", "kl"] if per_agent else \
        list(terms) == ["policy_loss", "vf_loss", "entropy", "kl", "total_loss"]
    assert abs(float(terms["total_loss"].detach()) - float(want["total_loss"].detach())) <= 1e-12
    for mine, theirs in (("policy_loss", "policy_loss"), ("vf_loss", "vf_loss"), ("entropy", "entropy"), ("kl", "kl_mean")):
        assert abs(float(terms[mine].detach()) - float(want[theirs].detach().mean())) <= 1e-12, mine
        if per_agent:
            assert (terms["per_policy"][mine] - want[theirs]).abs().max() <= 1e-12, mine
    assert (grad - want["gradient"]).abs().max() <= 1e-12 and want["gradient"].abs().max() > 1e-3
    # and the term is in it: without the coefficient the total and the gradient are other numbers
    plain = ln.PPOLearner(module, fused=False, **hp).losses({k: v for k, v in frag64.items() if k != "logits"}, adv, targets)
    assert abs(float(plain["total_loss"].detach()) - float(terms["total_loss"].detach())) > 1e-3


def test_the_adaptation_rule_at_its_three_regimes():
    from dl_reference_models_amd import learner as ln

    target = 0.01
    coeff = torch.tensor([0.2, 0.3, 0.4, 0.5, 0.6], dtype=torch.float32)
    kl = torch.tensor([0.0201, 0.0049, 0.01, 0.02, 0.005], dtype=torch.float32)  # above 2 x, below 0.5 x, inside, on both edges
    got = ln.adapted_kl_coeff(coeff, kl, target)
    assert torch.equal(got, coeff * torch.tensor([1.5, 0.5, 1.0, 1.0, 1.0]))
    assert got.dtype == torch.float32 and got.data_ptr() != coeff.data_ptr()


def test_update_adapts_every_policys_coefficient_by_its_own_kl():
    from dl_reference_models_amd import learner as ln

    frag, adv, targets = _fragment()
    module = du.make_per_agent(N, L, True, True, seed=2).train()
    learner = ln.PPOLearner(module, fused=False, kl_coeff=0.2, kl_target=0.01, epochs=1, minibatches=2)
    out = learner.update(frag, adv.float(), targets.float())
    kl = out["per_policy"]["kl"]
    assert torch.equal(learner.sampled_kl, kl) and tuple(kl.shape) == (N,) and (kl > 0.02).all()  # far from the behaviour logits
    assert torch.equal(learner.kl_coeff, torch.full((N,), 0.2) * 1.5) and torch.equal(out["per_policy"]["kl_coeff"], learner.kl_coeff)
    assert float(out["kl_coeff"]) == pytest.approx(0.3) and float(out["kl"]) == pytest.approx(float(kl.mean()))
    # a target far above what was sampled halves it; one the sample lies within leaves it
    shared = lambda target: ln.PPOLearner(pu.make_module(L, True, True, seed=2).train(), fused=False, kl_coeff=0.4,  # noqa: E731
                                          kl_target=target, epochs=1, minibatches=1, lr=0.0)
    kl0 = float(shared(0.01).update(frag, adv.float(), targets.float())["kl"])  # (lr 0: the same number whatever the target)
    for target, factor in ((10.0 * kl0, 0.5), (kl0, 1.0), (0.1 * kl0, 1.5)):
        ln2 = shared(target)
        res = ln2.update(frag, adv.float(), targets.float())
        assert float(res["kl"]) == kl0 and torch.equal(ln2.sampled_kl, res["kl"].reshape(1))
        assert torch.equal(ln2.kl_coeff, torch.full((1,), 0.4) * factor) and torch.equal(res["kl_coeff"], ln2.kl_coeff[0]), target


def test_a_learner_built_with_defaults_is_todays():
    from dl_reference_models_amd import learner as ln

    frag, adv, targets = _fragment()
    del frag["logits"]
    module = pu.make_module(L, True, True, seed=2).train()
    learner = ln.PPOLearner(module, fused=False, epochs=1, minibatches=2)
    assert learner.kl_coeff is None and learner.fused_objective is False and learner.sampled_kl is None
    assert list(learner.losses(frag, adv.float(), targets.float())) == ["policy_loss", "vf_loss", "entropy", "total_loss"]
    assert list(learner.update(frag, adv.float(), targets.float())) == ["policy_loss", "vf_loss", "entropy", "total_loss"]
    per = ln.PPOLearner(du.make_per_agent(N, L, True, True, seed=2), fused=False).losses(frag, adv.float(), targets.float())
    assert list(per) == ["total_loss", "policy_loss", "vf_loss", "entropy", "per_policy"]
    assert list(per["per_policy"]) == ["policy_loss", "vf_loss", "entropy", "total_loss"]
    with pytest.raises(ValueError, match="kl_coeff"):
        ln.PPOLearner(module, kl_coeff=-0.1)
    assert ln.PPO_FUSED_OBJECTIVE_DEFAULT in (True, False)
    assert ln.PPOLearner(module, kl_coeff=0.2).fused_objective is ln.PPO_FUSED_OBJECTIVE_DEFAULT
    assert ln.PPOLearner(module, fused_objective=True).fused_objective is True


def test_a_coefficient_without_logits_names_keep_logits():
    from dl_reference_models_amd import learner as ln

    frag, adv, targets = _fragment()
    module = pu.make_module(L, True, True, seed=2)
    learner = ln.PPOLearner(module, fused=False, kl_coeff=0.2)
    bare = {k: v for k, v in frag.items() if k != "logits"}
    with pytest.raises(ValueError, match="keep_logits"):
        learner.losses(bare, adv.float(), targets.float())
    with pytest.raises(ValueError, match="keep_logits"):
        learner.update(bare, adv.float(), targets.float())
    with pytest.raises(ValueError, match=r"fragment\['logits'\]"):
        learner.losses(dict(frag, logits=frag["logits"][..., :4]), adv.float(), targets.float())


@pytest.mark.parametrize("shape", plu.SHAPES + plu.LONG_SHAPES, ids=lambda s: "T%d_rows%d_heads%d_groups%d" % s)
def test_the_generators_conditions_hold(shape):
    c = plu.case(*shape)  # (asserts them)
    s = c["shares"]
    print("ppo case T=%d rows=%d heads=%d groups=%d: " % shape + ", ".join(f"{k} {v:.4f}" for k, v in s.items()))
    assert s["zero_grad"] >= 0.05 and s["above"] >= 0.05 and s["below"] >= 0.03 and 0.2 <= s["vclip"] <= 0.5
    assert all(c["dev"][k] > 0 for k in plu.QUANTITIES)
    tiles = plu.tiles_of(shape[1], shape[3])
    assert len(tiles) == shape[3] * -(-(shape[1] // shape[3]) // plu.TILE_ROWS) == c["want"]["partials"].shape[0]
    assert sorted(np.concatenate(tiles).tolist()) == list(range(shape[1]))


def test_the_other_cases_meet_their_conditions():
    for args in ((2, 63, 3, 1, "plain", "REFERENCE"), (2, 63, 3, 1, "overflow"), (5, 65, 3, 1, "one_left"),
                 (3, 96, 1, 3, "plain", "SETTINGS", False)):
        plu.case(*args)
    # and those of the fragments beyond one chunk (tests/test_ppo_loss_gpu.py)
    for args in ((33, 65, 3, 1, "overflow"), (33, 65, 3, 1, "one_left"), (65, 33, 16, 1, "overflow"), (65, 33, 16, 1, "one_left"),
                 (32, 33, 1, 1, "plain", "REFERENCE"), (33, 65, 3, 1, "plain", "SETTINGS", False)):
        plu.case(*args)
    c = plu.case(2, 63, 3, 1, "overflow")
    with np.errstate(over="ignore"):
        ratio32 = np.exp((c["want"]["logp"] - c["inp"]["old_logp"]).astype(np.float32))
    pos = c["inp"]["adv"] > 0
    assert np.isinf(ratio32[pos]).all() and (ratio32[~pos] < 3).all() and 0.3 < pos.mean() < 0.7


def test_abi_bookkeeping():
    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd import build

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mapf_step.h")).read()
    assert "mapf_ppo_loss" in L.EXPORTED_SYMBOLS and "mapf_ppo_partials" in L.EXPORTED_SYMBOLS
    assert re.search(r"^int mapf_ppo_loss\(", header, re.M) and re.search(r"^int32_t mapf_ppo_partials\(", header, re.M)
    rule = header[header.index("The PPO objective on a minibatch"):header.index("int mapf_ppo_loss(")]
    for word in ("kl_coeff", "DEVICE pointer", "groups", "bitwise equal", "MAPF_ERR_CONFIG", "clamp(ratio"):
        assert word in rule, word
    assert (L.PPO_MAX_HEADS, L.PPO_CHUNK, L.PPO_TILE_ROWS) == tuple(
        int(re.search(r"#define MAPF_PPO_" + n + r" (\d+)", header).group(1)) for n in ("MAX_HEADS", "CHUNK", "TILE_ROWS"))
    assert (plu.CHUNK, plu.TILE_ROWS) == (L.PPO_CHUNK, L.PPO_TILE_ROWS)
    assert "chunks of MAPF_PPO_CHUNK steps" in rule
    with open(os.path.join(root, "dl_reference_models_amd", "csrc", "mapf_ppo.hip"), encoding="utf-8") as f:
        assert "static_assert(kChunk == MAPF_PPO_CHUNK" in f.read()  # the kernel's chunk is the header's
    lengths = [s[0] for s in plu.LONG_SHAPES]  # whole chunks, a one-step and a short last chunk, three chunks
    assert min(lengths) == plu.CHUNK and {T % plu.CHUNK for T in lengths} == {0, 1, 8} and max(lengths) > 2 * plu.CHUNK
    assert build.PPO_SOURCE in build.SOURCES
    for name, (_so, _flags, units) in build.VARIANTS.items():
        assert [u for u in units if u[0] == "ppo" and u[1] == build.PPO_SOURCE], name
    lib = L.load()  # the checks that come before any launch need no device
    f = [0.2, 10.0, 0.5, 0.001]
    for shape in ((0, 1, 1, 1), (1, 1, 1, 1), (1, 1, 65, 1), (1, 3, 1, 2), (1, 1, 1, 0)):
        assert lib.mapf_ppo_loss(*shape, *([None] * 7), *f, *([None] * 7)) == L.MAPF_ERR_CONFIG, shape
    assert [lib.mapf_ppo_partials(*a) for a in ((0, 1), (65, 1), (96, 3), (130, 2), (5, 2), (4, 0))] == [0, 3, 3, 6, 0, 0]
