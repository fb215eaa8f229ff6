"""The wide joint-action policy (256-256 feed-forward, the reference's CTE IMPALA net) without a GPU: the module's config
and checkpoint, the layout of its parameter vector, the module against the float64 restatement, the property of the shared
cases that the GPU test relies on, the paths of fc1's K-walk that the shapes reach (and two faults of its odd tail that only
the shapes added for it can see), and the refusal of a recurrent wide module before the library is touched."""

import numpy as np
import pytest
import torch

import wide_joint_util as wu


def test_config_and_checkpoint_round_trip(tmp_path):
    from dl_reference_models_amd.policy import JointActionPolicy

    m = wu.make_module(35, 3, seed=3)
    want = {"grid_cells": 35, "num_agents": 3, "recurrent": False, "hidden": 256}
    assert m.config() == want
    m.save(tmp_path / "wide.pt")
    blob = torch.load(tmp_path / "wide.pt", weights_only=True)
    assert blob["kind"] == "joint_action" and blob["config"] == want
    back = JointActionPolicy.load(tmp_path / "wide.pt")
    assert back.config() == want and torch.equal(back.flat_params(), m.flat_params())
    assert back.fc1.weight.shape == (256, 35) and back.fc2.weight.shape == (256, 256) and not hasattr(back, "lstm")


def test_flat_params_are_the_state_dict_in_its_order():
    F, N = 35, 3
    m = wu.make_module(F, N)
    names = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "pi.weight", "pi.bias", "vf.weight", "vf.bias"]
    sizes = [256 * F, 256, 256 * 256, 256, 5 * N * 256, 5 * N, 256, 1]
    assert list(m.state_dict().keys()) == names
    assert [v.numel() for v in m.state_dict().values()] == sizes
    assert [tuple(v.shape) for v in m.state_dict().values()] == [(256, F), (256,), (256, 256), (256,), (5 * N, 256), (5 * N,), (1, 256), (1,)]
    with torch.no_grad():
        for i, v in enumerate(m.state_dict().values()):
            v.fill_(float(i))
    flat = m.flat_params().numpy()
    assert flat.dtype == np.float32 and flat.size == sum(sizes)
    assert np.array_equal(flat, np.concatenate([np.full(s, i, np.float32) for i, s in enumerate(sizes)]))


@pytest.mark.parametrize("shape", wu.SHAPES, ids=str)
def test_module_agrees_with_the_restatement_to_dev(shape):
    """``dev`` is the module's largest deviation on the case, so every step lies within it, and some step attains it."""
    c = wu.case(shape, False)
    assert 0 < c["dev"] < 1e-5
    worst = 0.0
    for s in c["steps"]:
        assert s["logits32"].dtype == np.float32 and s["logits32"].shape == s["logits"].shape
        worst = max(worst, float(np.abs(s["logits32"] - s["logits"]).max()), float(np.abs(s["value32"] - s["value"]).max()))
    assert worst == c["dev"]
    # the restatement is the module's rule: a float64 copy of the module gives the same numbers to float64 rounding
    m64 = wu.make_module(shape[1] * shape[2], shape[3]).double()
    with torch.no_grad():
        l64, v64, _ = m64(torch.from_numpy(c["obs"][0]).double())
    assert np.abs(l64.numpy() - c["steps"][0]["logits"]).max() < 1e-12 and np.abs(v64.numpy() - c["steps"][0]["value"]).max() < 1e-12


@pytest.mark.parametrize("shape,sample", wu.CASES, ids=lambda v: str(v).replace(" ", ""))
def test_case_inputs_leave_the_decisions_to_the_policy(shape, sample):
    """The share the restatement itself cannot decide (top-two gap within 32 x dev): at most 1 % of the decisions and 2 % of
    the rows of a case."""
    c = wu.case(shape, sample)
    assert 0 < c["dev"] < 1e-5
    dec, rows = wu.undecided(c)
    print(f"wide joint case {shape} sample={sample}: dev {c['dev']:.3e}, undecided decisions {dec:.4%}, rows {rows:.4%}")
    assert dec <= wu.MAX_UNDECIDED_DECISIONS and rows <= wu.MAX_UNDECIDED_ROWS
    assert c["cfg"] == {"grid_cells": shape[1] * shape[2], "num_agents": shape[3], "recurrent": False, "hidden": 256}


def test_fc1_groups_is_the_layout_rule():
    assert (wu.WALK, wu.CHUNK, wu.GC) == (16, 256, 8)
    want = {1: [1], 9: [1], 32: [1], 33: [2], 35: [2], 64: [2], 65: [3], 96: [3], 97: [4], 256: [8], 257: [8, 1], 261: [8, 1],
            340: [8, 3], 600: [8, 8, 3], 1024: [8] * 4, 4096: [8] * 16}
    assert {F: wu.fc1_groups(F) for F in want} == want
    for F in range(1, 4097):  # one count per chunk the kernel stages, every chunk but the last full, all k-steps covered
        g = wu.fc1_groups(F)
        assert len(g) == -(-F // wu.CHUNK) and all(n == wu.GC for n in g[:-1]) and 1 <= g[-1] <= wu.GC
        assert 2 * wu.WALK * (sum(g) - 1) < F <= 2 * wu.WALK * sum(g)
    assert [wu.walk_order(n) for n in (1, 2, 3, 8)] == [[0], [0, 1], [0, 1, 2], list(range(8))]
    assert [wu.walk_order(n, "stale_tail") for n in (1, 2, 3, 5)] == [[0], [0, 1], [0, 1, 1], [0, 1, 2, 3, 3]]
    assert [wu.walk_order(n, "drop_tail") for n in (1, 2, 3, 5)] == [[0], [0, 1], [0, 1], [0, 1, 2, 3]]


def _odd_tail(shape):
    return any(n % 2 and n >= 3 for n in wu.fc1_groups(shape[1] * shape[2]))


def test_the_shapes_walk_every_path_of_the_k_walk():
    """Conditions on the table, from the layout rule: an edit of SHAPES cannot silently lose a path of ``walk``."""
    per_shape = {s: wu.fc1_groups(s[1] * s[2]) for s in wu.SHAPES}
    assert set(wu.OLD_SHAPES) <= set(wu.SHAPES) and len(set(wu.SHAPES)) == len(wu.SHAPES)
    # what the seven shapes of the 64-wide kernel reach: the loop alone or the tail alone
    assert {n for s in wu.OLD_SHAPES for n in per_shape[s]} == {1, 2, 8}
    assert not any(_odd_tail(s) for s in wu.OLD_SHAPES)
    counts = list(per_shape.values())
    assert {n for g in counts for n in g} == set(range(1, 9))  # every count a chunk can have
    for n in (3, 5, 7):  # the loop, then the tail: as the only chunk, and behind full chunks
        assert [n] in counts, n
        assert any(len(g) > 1 and g[-1] == n for g in counts), n
    # an odd tail of at least 3 in either staging buffer: the chunk's index is even (first buffer) and odd (second)
    buffers = {(len(g) - 1) & 1 for g in counts if g[-1] % 2 and g[-1] >= 3}
    assert buffers == {0, 1}
    assert any(len(g) > 2 and g[-1] % 2 and g[-1] >= 3 for g in counts)  # ... the first buffer also after it was reused
    assert any(n in (4, 6) for g in counts for n in g)  # the clamp on a trip other than the first or the fourth
    assert all(s[0] <= 65 for s in wu.WALK_SHAPES)


def test_an_odd_tail_fault_passes_the_old_shapes_and_fails_the_new():
    """The float32 restatement whose fc1 accumulates K in the kernel's order, and two mutants of its tail, under the
    logits / value assertions of the GPU parity test: the seven shapes from before cannot see either fault, every shape
    with an odd group count of at least 3 sees both, and the unmutated restatement passes everywhere."""
    assert len(wu.OLD_SHAPES) == 7
    odd = [s for s in wu.SHAPES if _odd_tail(s)]
    assert len(odd) >= 7 and not set(odd) & set(wu.OLD_SHAPES)
    for shape in wu.SHAPES:
        c = wu.case(shape, False)
        assert not wu.parity_fails(c, wu.restate32(c)), shape
        for mutant in wu.WALK_MUTANTS:
            fails = wu.parity_fails(c, wu.restate32(c, mutant))
            if shape in odd:
                print(f"wide joint {shape} groups {wu.fc1_groups(shape[1] * shape[2])} {mutant}: {fails}")
                assert fails, (shape, mutant)
            else:
                assert not fails, (shape, mutant, fails)


def test_a_recurrent_wide_module_is_refused_by_name_before_the_library(monkeypatch):
    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd.policy import JointDevicePolicy

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "load", no_library)
    with pytest.raises(ValueError, match="hidden = 256.*feed-forward only"):
        JointDevicePolicy(wu.make_module(9, 1, recurrent=True), 4, device="cuda:0")
