"""The learner's rows view without a GPU: every chain of tests/golden/learner_parent_f64.npz (what the commit before the view
computed; tools/gen_learner_golden.py) recomputed on the CPU in float64, and the shared and the joint layout of the same
data against each other."""

import os

import numpy as np
import pytest
import torch

import learner_golden_util as gu
import policy_util as pu
from trace_util import ROOT


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(ROOT, "tests", "golden", gu.FIXTURE + ".npz"), allow_pickle=False) as z:
        return {k: z[k] for k in z.files}


def test_the_fixture_holds_every_chain_and_nothing_else(golden):
    assert {k.split("/")[0] for k in golden} == set(gu.CHAINS)
    assert all(v.dtype == np.float64 and np.isfinite(v).all() for v in golden.values())
    per = [k for k in golden if "/per_policy/" in k]
    assert per and all(k.startswith("ppo_per_agent") for k in per)  # present exactly with a PerAgentPolicy


@pytest.mark.parametrize("name", list(gu.CHAINS))
def test_the_chain_computes_what_the_commit_before_the_view_computed(golden, name):
    """In float64 a reordering of sums costs about 1e-15 and a wiring error O(1): every recorded quantity within 1e-9 x
    max(1, |recorded|), and the net moved."""
    got = gu.run_chain(name)
    want = {k: v for k, v in golden.items() if k.startswith(name + "/")}
    assert set(got) == set(want) and len(want) >= 12
    worst = 0.0
    for k, w in want.items():
        assert got[k].shape == w.shape, k
        err = np.abs(got[k] - w) / np.maximum(1.0, np.abs(w))
        worst = max(worst, float(err.max()))
        assert (err <= gu.MARGIN).all(), (k, float(err.max()))
    print(f"{name}: {sum(v.size for v in want.values())} doubles, largest relative difference {worst:.2e}")
    assert float(want[name + "/moved"][0]) > gu.MOVED and float(got[name + "/moved"][0]) > gu.MOVED


def _close(a, b, what):
    a, b = a.detach().double().reshape(-1), b.detach().double().reshape(-1)
    assert a.shape == b.shape and bool(((a - b).abs() <= 1e-12 * torch.clamp(b.abs(), min=1.0)).all()), (what, float((a - b).abs().max()))


def test_one_agent_per_env_is_the_same_thing_in_the_shared_and_in_the_joint_layout():
    """A ``JointActionPolicy`` of one agent and a ``MaskedRecurrentPolicy`` with a mask have the same ``state_dict``; on the same
    data laid out as [T, B, L] and as [T, B, 1, L] (rewards exactly representable in fp32, which the joint rule rounds to)
    ``gae``, ``sequence_forward``, the PPO loss and the parameters after ``update`` agree to float64 rounding."""
    from dl_reference_models_amd import learner as ln
    from dl_reference_models_amd.policy import JointActionPolicy

    T, B, F = 5, 8, 11
    shared = pu.make_module(F + 5, True, True, seed=2).double().train()
    joint = JointActionPolicy(F, 1).double().train()
    assert {k: tuple(v.shape) for k, v in joint.state_dict().items()} == {k: tuple(v.shape) for k, v in shared.state_dict().items()}
    joint.load_state_dict(shared.state_dict())
    import learner_util as lu

    frag = gu.f64(lu.synthetic_fragment(T, B, 1, F + 5, True, seed=9))
    assert torch.equal(frag["rewards"], frag["rewards"].float().double()) and torch.equal(frag["prev_rewards"], frag["prev_rewards"].float().double())
    as_joint = {k: (v if k in ("terminated", "truncated", "first", "h0", "c0", "actions", "prev_action0") else v.squeeze(2 if v.dim() > 2 else 1))
                for k, v in frag.items()}
    assert ln.is_joint(as_joint) and not ln.is_joint(frag) and ln.check_fragment(as_joint) == ln.check_fragment(frag) == (T, B, 1, F + 5)
    va, vb = ln.fragment_view(frag, shared), ln.fragment_view(as_joint, joint)
    assert (va.R, va.heads, va.groups, va.units) == (vb.R, vb.heads, vb.groups, vb.units) == (B, 1, 1, B)
    rows = torch.tensor([4, 0, 3])
    (adv, tgt), (jadv, jtgt) = ln.gae(frag), ln.gae(as_joint)
    assert adv.shape == (T, B, 1) and jadv.shape == (T, B)
    _close(jadv, adv, "adv"), _close(jtgt, tgt, "targets")
    with torch.no_grad():
        for r in (None, rows):
            for name, x, y in zip(("logits", "value"), ln.sequence_forward(joint, as_joint, r, fused=False),
                                  ln.sequence_forward(shared, frag, r, fused=False)):
                _close(x, y, name)
    kw = dict(epochs=2, minibatches=3, seed=4, grad_clip=0.5, fused=False)
    la, lb = ln.PPOLearner(shared, **kw), ln.PPOLearner(joint, **kw)
    ta, tb = la.losses(frag, adv, tgt, rows), lb.losses(as_joint, jadv, jtgt, rows)
    assert set(ta) == set(tb) == set(lu.LOSS_TERMS)
    for k in lu.LOSS_TERMS:
        _close(tb[k], ta[k], k)
    before = gu.params64(shared)
    ua, ub = la.update(frag, adv, tgt), lb.update(as_joint, jadv, jtgt)
    for k in lu.LOSS_TERMS:
        _close(ub[k], ua[k], "update " + k)
    _close(gu.params64(joint), gu.params64(shared), "parameters")
    assert float((gu.params64(shared) - before).norm()) > 1e-4
