"""Behaviour cloning without a GPU: ``learner.bc_objective`` against bc_util's float64 NumPy restatement and its closed-form
gradients, the per-group means, a ``BCLearner`` that learns labels which are a function of the observation (shared, joint and
one policy per agent), the refusals by name, the DAgger draw and the beta schedule, the conditions of the case generator and
the C ABI's bookkeeping (symbols, header, constants, the argument checks that need no device)."""

import copy
import os
import re

import numpy as np
import pytest
import torch

import bc_util as bu
import dte_util as du
import joint_learner_util as jl
import joint_policy_util as ju
import learner_util as lu
import policy_util as pu

HOST_CASES = [(s, k) for s in ((2, 63, 3, 1), (3, 96, 1, 3), (2, 130, 1, 2), (1, 1, 1, 1)) for k in bu.KINDS]


def _objective64(c, per_group=True):
    from dl_reference_models_amd import learner as ln

    inp, hp = c["inp"], c["hp"]
    logits = torch.from_numpy(inp["logits"]).double().requires_grad_(True)
    values = None if inp["values"] is None else torch.from_numpy(inp["values"]).double().requires_grad_(True)
    targets = None if inp["targets"] is None else torch.from_numpy(inp["targets"]).double()
    per, extra = ln.bc_objective(logits, torch.from_numpy(inp["expert"]), values, targets, hp["vf_coeff"], hp["ent_coeff"],
                                 c["groups"], per_group)
    return logits, values, per, extra


@pytest.mark.parametrize("shape,kind", HOST_CASES, ids=lambda x: x if isinstance(x, str) else "T%d_rows%d_heads%d_groups%d" % x)
def test_the_objective_in_float64_equals_the_numpy_restatement(shape, kind):
    c = bu.case(*shape, kind)
    want = c["want"]
    logits, values, per, extra = _objective64(c)
    assert per["nll"].dtype == torch.float64 and tuple(per["nll"].shape) == (shape[3],)
    for mine, theirs in (("nll", "nll_mean"), ("vf_loss", "vf_loss"), ("entropy", "entropy"), ("accuracy", "accuracy"), ("total_loss", "total")):
        assert np.abs(per[mine].detach().numpy() - want[theirs]).max() <= 1e-12 * max(1.0, np.abs(want[theirs]).max()), mine
    assert np.abs(extra["nll"].detach().numpy() - want["nll"]).max() <= 1e-12 * max(1.0, np.abs(want["nll"]).max())
    assert np.array_equal(extra["hits"].numpy(), want["hits"])
    # and its autograd gradient is the closed form
    dlogits, dvalues = torch.autograd.grad(per["total_loss"].sum(), [logits, values])
    assert np.abs(dlogits.numpy() - want["dlogits"]).max() <= 1e-12
    assert np.abs(dvalues.numpy() - want["dvalues"]).max() <= 1e-12
    assert np.abs(want["dlogits"]).max() > 0 and np.isfinite(want["dlogits"]).all()


def test_the_objective_without_values_has_no_value_term():
    c = bu.case(2, 63, 3, 1, "plain", False)
    logits, values, per, _ = _objective64(c)
    assert values is None and float(per["vf_loss"].abs().max()) == 0.0
    assert np.abs(per["total_loss"].detach().numpy() - c["want"]["total"]).max() <= 1e-12
    full = bu.case(2, 63, 3, 1)
    assert np.abs(c["want"]["nll_mean"] - full["want"]["nll_mean"]).max() == 0 and c["want"]["total_loss"] != full["want"]["total_loss"]
    from dl_reference_models_amd import learner as ln

    with pytest.raises(ValueError, match="both or neither"):
        ln.bc_objective(logits, torch.from_numpy(c["inp"]["expert"]), torch.zeros(2, 63, dtype=torch.float64), None)


@pytest.mark.parametrize("shape", ((3, 96, 1, 3), (2, 130, 1, 2)), ids=lambda s: "T%d_rows%d_heads%d_groups%d" % s)
def test_the_per_group_means_are_the_ungrouped_call_on_a_groups_rows(shape):
    from dl_reference_models_amd import learner as ln

    c = bu.case(*shape)
    G, hp = shape[3], c["hp"]
    _, _, per, _ = _objective64(c)
    t = {k: torch.from_numpy(v) for k, v in c["inp"].items()}
    for g in range(G):
        alone, _ = ln.bc_objective(t["logits"][:, g::G].double(), t["expert"][:, g::G], t["values"][:, g::G].double(),
                                   t["targets"][:, g::G].double(), hp["vf_coeff"], hp["ent_coeff"])
        for k in ("nll", "vf_loss", "entropy", "accuracy", "total_loss"):
            assert abs(float(per[k][g].detach()) - float(alone[k].detach())) <= 1e-12 * max(1.0, abs(float(alone[k].detach()))), (g, k)
    _, _, whole, _ = _objective64(c, per_group=False)  # and the ungrouped means are the means of the groups' (equal counts)
    for k in ("nll", "vf_loss", "entropy", "accuracy"):
        assert abs(float(whole[k].detach()) - float(per[k].mean().detach())) <= 1e-12 * max(1.0, abs(float(whole[k].detach()))), k


# ---- the learner -----------------------------------------------------------------------------------------------------------
T, B, N, L = 8, 12, 2, 16


def _label_of(obs):
    """Labels that are a function of the observation alone: which of its first two features are positive, 0 .. 3."""
    return ((obs[..., 0] > 0).to(torch.int8) + 2 * (obs[..., 1] > 0).to(torch.int8))


def _labelled(layout, seed):
    if layout == "joint":
        frag = jl.synthetic_fragment(T, B, 4, 4, N, seed=seed)
        obs = frag["obs"]  # [T, B, 16 + 5 N]: head k is labelled by two of the env's cells
        frag["expert_actions"] = torch.stack([(obs[..., 2 * k] > 0).to(torch.int8) + 2 * (obs[..., 2 * k + 1] > 0).to(torch.int8)
                                              for k in range(N)], dim=2)
    else:
        frag = lu.synthetic_fragment(T, B, N, L, mask=True, seed=seed)
        frag["expert_actions"] = _label_of(frag["obs"])
    frag["followed"] = torch.zeros((T, B), dtype=torch.uint8)
    return frag


def _module(layout, seed=2):
    if layout == "joint":
        return ju.make_module(16, N, True, seed=seed).train()
    if layout == "per_agent":
        return du.make_per_agent(N, L, True, True, seed=seed).train()
    return pu.make_module(L, True, True, seed=seed).train()


@pytest.mark.parametrize("layout", ("shared", "joint", "per_agent"))
def test_the_learner_clones_labels_that_are_a_function_of_the_observation(layout):
    from dl_reference_models_amd import learner as ln

    train, held = _labelled(layout, 5), _labelled(layout, 6)
    assert len(torch.unique(held["expert_actions"])) >= 2
    module = _module(layout)
    learner = ln.BCLearner(module, lr=5e-3, epochs=12, minibatches=3, seed=1)
    assert not learner.needs_gae and learner.beta_schedule == [(0, 0.0)]
    with torch.no_grad():
        before = learner.losses(held)
    out = learner.update(train)  # 36 Adam steps
    with torch.no_grad():
        after = learner.losses(held)
    print(f"bc on the CPU, {layout}: held nll {float(before['nll']):.4f} -> {float(after['nll']):.4f}, accuracy "
          f"{float(before['accuracy']):.3f} -> {float(after['accuracy']):.3f}")
    assert float(after["nll"]) < float(before["nll"]) and float(after["accuracy"]) > float(before["accuracy"])
    want = {"nll", "accuracy", "vf_loss", "entropy", "total_loss"} | ({"per_policy"} if layout == "per_agent" else set())
    assert set(out) == want and float(out["vf_loss"]) == 0.0
    if layout == "per_agent":
        assert all(tuple(v.shape) == (N,) for v in out["per_policy"].values())


def test_with_a_value_coefficient_the_value_head_is_regressed_to_gaes_targets():
    from dl_reference_models_amd import learner as ln

    frag = _labelled("shared", 5)
    module = _module("shared")
    learner = ln.BCLearner(module, lr=5e-3, vf_coeff=0.5, ent_coeff=0.01, epochs=8, minibatches=2, seed=1)
    assert learner.needs_gae
    adv, targets = ln.gae(frag)
    with torch.no_grad():
        before = learner.losses(frag, targets)
    with pytest.raises(ValueError, match="targets"):
        learner.update(frag)
    learner.update(frag, adv, targets)
    with torch.no_grad():
        after = learner.losses(frag, targets)
    assert float(before["vf_loss"]) > 0 and float(after["vf_loss"]) < float(before["vf_loss"]) and float(after["nll"]) < float(before["nll"])
    total = after["nll"] + 0.5 * after["vf_loss"] - 0.01 * after["entropy"]
    assert abs(float(after["total_loss"]) - float(total)) <= 1e-6 * abs(float(total))
    # the value head of a learner without the coefficient does not move
    module = _module("shared")
    vf = copy.deepcopy(module.vf.state_dict())
    ln.BCLearner(module, epochs=1, minibatches=1).update(frag)
    assert all(torch.equal(v, module.vf.state_dict()[k]) for k, v in vf.items())


def test_the_torch_losses_equal_the_restatement_on_chained_forwards():
    """The learner's view, minibatch gather and objective on a fragment against bc_util.bc_terms on T chained module calls."""
    from dl_reference_models_amd import learner as ln

    for layout, G, heads in (("shared", 1, 1), ("joint", 1, N), ("per_agent", N, 1)):
        frag = _labelled(layout, 7)
        frag64 = {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}
        module = _module(layout).double()
        logits, values = (jl if layout == "joint" else lu).chained_forward(module, frag64)
        R = values.shape[1]
        adv, targets = ln.gae(frag)
        want = bu.bc_terms(logits.detach().numpy().reshape(T, R, 5 * heads), frag["expert_actions"].reshape(T, R, heads).numpy(),
                           values.detach().numpy(), targets.reshape(T, R).numpy(), 0.7, 0.03, G)
        got = ln.BCLearner(module, vf_coeff=0.7, ent_coeff=0.03, fused=False).losses(frag64, targets.double())
        per = got.get("per_policy", got)
        for mine, theirs in (("nll", "nll_mean"), ("vf_loss", "vf_loss"), ("entropy", "entropy"), ("accuracy", "accuracy")):
            assert np.abs(per[mine].detach().numpy().reshape(G) - want[theirs]).max() <= 1e-10, (layout, mine)
        assert abs(float(got["total_loss"].detach()) - want["total_loss"]) <= 1e-10, layout


def test_refusals_by_name():
    from dl_reference_models_amd import learner as ln
    from dl_reference_models_amd import rollout as ro

    frag = _labelled("shared", 5)
    bare = {k: v for k, v in frag.items() if k != "expert_actions"}
    learner = ln.BCLearner(_module("shared"))
    for call in (learner.update, learner.losses):
        with pytest.raises(ValueError, match=r"expert_actions.*Rollout\(expert="):
            call(bare)
    with pytest.raises(ValueError, match="expert_actions"):
        learner.losses(dict(frag, expert_actions=frag["expert_actions"][..., :1]))
    # the rollouts refuse their expert options before they look at the env
    with pytest.raises(ValueError, match="'windowed' is not offered on the single-agent env"):
        ro.JointRollout(None, None, 8, expert="windowed")
    for cls in (ro.Rollout, ro.JointRollout):
        with pytest.raises(ValueError, match="unknown expert 'prioritized'.*yielding"):
            cls(None, None, 8, expert="prioritized")
        with pytest.raises(ValueError, match="beta must lie in"):
            cls(None, None, 8, expert="yielding", beta=1.5)
        with pytest.raises(ValueError, match="needs an expert"):
            cls(None, None, 8, beta=0.5)
        with pytest.raises(TypeError):  # and with none of the options, what they refused before
            cls(None, None, 8)
    with pytest.raises(ValueError, match="expert_window must lie in"):
        ro.Rollout(None, None, 8, expert="windowed", expert_window=65)
    assert ro.MULTI_AGENT_ONLY_EXPERTS == ("windowed",)
    # and so does the learner that carries them to the Trainer
    with pytest.raises(ValueError, match="unknown expert"):
        ln.BCLearner(_module("shared"), expert="cbs")
    with pytest.raises(ValueError, match="single-agent env"):
        ln.BCLearner(_module("joint"), expert="windowed")
    with pytest.raises(ValueError, match="beta must lie in"):
        ln.BCLearner(_module("shared"), beta_schedule=[(0, 1.0), (5, -0.1)])
    for name in ("vf_coeff", "ent_coeff"):
        for bad in (-0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=name):
                ln.BCLearner(_module("shared"), **{name: bad})


def test_the_beta_schedule_and_the_seeded_draw():
    from dl_reference_models_amd import learner as ln
    from dl_reference_models_amd import rollout as ro
    from dl_reference_models_amd.dqn import epsilon_at

    learner = ln.BCLearner(_module("shared"), expert="windowed", expert_window=6, beta_schedule=[(0, 1.0), (4, 0.0)])
    assert [learner.beta_at(i) for i in range(6)] == [1.0, 0.75, 0.5, 0.25, 0.0, 0.0]
    assert all(learner.beta_at(i) == epsilon_at([(0, 1.0), (4, 0.0)], i) for i in range(-2, 8))
    assert learner.rollout_options() == {"expert": "windowed", "expert_window": 6, "beta": 1.0}
    assert ln.BCLearner(_module("shared"), beta_schedule=0.25).beta_at(100) == 0.25
    # the draw of the rollouts' ``followed`` slab: a host generator, so the same bytes everywhere; rand < beta
    gen = torch.Generator()
    gen.manual_seed(77)
    a = ro.followed_draw(gen, 8, 16, 0.5)
    gen.manual_seed(77)
    assert torch.equal(a, (torch.rand((8, 16), generator=gen) < 0.5).to(torch.uint8)) and a.dtype == torch.uint8
    assert not ro.followed_draw(gen, 8, 16, 0.0).any() and ro.followed_draw(gen, 8, 16, 1.0).all()
    # what tests/test_bc_rollout_gpu.py asks of the share of three fragments of 8 x 16 draws at its seed holds for the draw
    gen.manual_seed(11 ^ 0x5DA66E12)
    share = float(torch.stack([ro.followed_draw(gen, 8, 16, 0.5) for _ in range(3)]).float().mean())
    bound = bu.followed_share_bound(3 * 8 * 16, 0.5)
    assert abs(bound - 5 * 0.5 / np.sqrt(384)) < 1e-15 and abs(share - 0.5) <= bound, (share, bound)


@pytest.mark.parametrize("shape", bu.SHAPES + bu.LONG_SHAPES, ids=lambda s: "T%d_rows%d_heads%d_groups%d" % s)
def test_the_generators_conditions_hold(shape):
    for kind in bu.KINDS:
        c = bu.case(*shape, kind)  # (asserts them)
        print("bc case T=%d rows=%d heads=%d groups=%d " % shape + kind + ": " + ", ".join(f"{k} {v:.4f}" for k, v in c["shares"].items()))
        assert all(c["dev"][k] > 0 for k in bu.QUANTITIES) or shape == (1, 1, 1, 1)  # (one element can be exact: a bound of 0 then)
        tiles = bu.tiles_of(shape[1], shape[3])
        assert len(tiles) == c["want"]["partials"].shape[0] == len(c["want"]["tile_hits"])
        assert shape[0] * bu.TILE_ROWS * shape[2] < 2 ** 24  # where the fp32 hit count of a tile is exact


def test_abi_bookkeeping():
    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd import build

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mapf_step.h")).read()
    assert "mapf_bc_loss" in L.EXPORTED_SYMBOLS and "mapf_bc_partials" in L.EXPORTED_SYMBOLS
    assert re.search(r"^int mapf_bc_loss\(", header, re.M) and re.search(r"^int32_t mapf_bc_partials\(", header, re.M)
    rule = header[header.index("The behaviour-cloning objective on a minibatch"):header.index("int mapf_bc_loss(")]
    for word in ("clamped to 0 .. 4", "lowest j on ties", "groups", "bitwise equal", "MAPF_ERR_CONFIG", "2^24", "both or neither",
                 "chunks of MAPF_BC_CHUNK steps", "never 0 x inf"):
        assert word in rule, word
    assert (L.BC_MAX_HEADS, L.BC_CHUNK, L.BC_TILE_ROWS) == tuple(
        int(re.search(r"#define MAPF_BC_" + n + r" (\d+)", header).group(1)) for n in ("MAX_HEADS", "CHUNK", "TILE_ROWS"))
    assert (bu.CHUNK, bu.TILE_ROWS) == (L.BC_CHUNK, L.BC_TILE_ROWS)
    with open(os.path.join(root, "dl_reference_models_amd", "csrc", "mapf_bc.hip"), encoding="utf-8") as f:
        assert "static_assert(kChunk == MAPF_BC_CHUNK" in f.read()  # the kernel's chunk is the header's
    assert build.BC_SOURCE in build.SOURCES
    for name, (_so, _flags, units) in build.VARIANTS.items():
        assert [u for u in units if u[0] == "bc" and u[1] == build.BC_SOURCE], name
    lib = L.load()  # exported, and the checks that come before any launch need no device
    assert hasattr(lib, "mapf_bc_loss") and hasattr(lib, "mapf_bc_partials")
    for shape in ((0, 1, 1, 1), (1, 0, 1, 1), (1, 1, 0, 1), (1, 1, 65, 1), (1, 3, 1, 2), (1, 1, 1, 0), (1, 1, 1, 1)):
        assert lib.mapf_bc_loss(*shape, *([None] * 4), 0.0, 0.0, *([None] * 5)) == L.MAPF_ERR_CONFIG, shape
    parts = lib.mapf_bc_partials
    assert parts(0, 1) == 0 and parts(65, 1) == 3 and parts(96, 3) == 3 and parts(130, 2) == 6 and parts(5, 2) == 0 and parts(4, 0) == 0
