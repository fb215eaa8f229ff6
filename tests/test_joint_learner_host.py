"""The learner on joint fragments without a GPU: ``PPOLearner.losses`` and its gradient against the objective written out
in joint_learner_util (which shares no code with learner.py), ``gae`` against a NumPy loop, ``sequence_forward`` against T
chained ``module.forward`` calls, and the fragment checks."""

import copy

import numpy as np
import pytest
import torch

import joint_learner_util as jl
import joint_policy_util as ju
import learner_util as lu
import policy_util as pu


def _learner():
    from dl_reference_models_amd import learner as ln

    return ln


def _f64(frag):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}


def _objective_case():
    """A synthetic joint fragment whose recorded logp are random, so the new policy's ratio is far from 1 on both sides, and
    settings that are none of the defaults and small enough that both clips bind on a part of the elements."""
    T, B, H, W, N = 6, 15, 5, 7, 3
    frag = jl.synthetic_fragment(T, B, H, W, N, seed=21)
    adv, targets = (torch.from_numpy(x) for x in jl.gae64(frag, 0.99, 0.95))
    settings = {"clip": 0.2, "vf_coeff": 0.7, "ent_coeff": 0.03, "vf_clip": 0.8}
    return frag, _f64(frag), jl.standardised(adv), targets, settings, ju.make_module(H * W, N, True, seed=4).train()


def test_losses_equal_the_objective_written_out():
    """Per-agent log-softmax, the summed log-probability of the N actions, the ratio against the recorded logp, the smaller
    of the clipped and the unclipped product, the squared error cut at vf_clip, the sum of the per-agent entropies and
    the weighted sum, all in float64: the same numbers up to the order of summation, 1e-12 of the largest term."""
    ln = _learner()
    frag, frag64, adv, targets, settings, m = _objective_case()
    m64 = copy.deepcopy(m).double()
    want = jl.ppo_by_hand(m64, frag64, adv, targets, **settings)
    assert 0.1 < want["ratio_binds"] < 0.9 and 0.1 < want["vf_binds"] < 0.9, want
    got64 = copy.deepcopy(m).double()
    terms = ln.PPOLearner(got64, fused=False, **settings).losses(frag64, adv, targets)
    terms["total_loss"].backward()
    loss = np.array([float(terms[k].detach()) for k in jl.LOSS_TERMS])
    grad = torch.cat([p.grad.reshape(-1) for p in got64.parameters()]).numpy()
    print(f"joint objective: {dict(zip(jl.LOSS_TERMS, loss))}, ratio clip binds on {want['ratio_binds']:.2f}, vf clip on "
          f"{want['vf_binds']:.2f}; largest difference {np.abs(loss - want['loss']).max():.2e}, gradient "
          f"{np.abs(grad - want['gradient']).max():.2e} of {np.abs(want['gradient']).max():.2e}")
    assert np.abs(loss - want["loss"]).max() <= 1e-12 * max(1.0, np.abs(want["loss"]).max())
    assert np.abs(want["gradient"]).max() > 1e-3
    assert np.abs(grad - want["gradient"]).max() <= 1e-12 * max(1.0, np.abs(want["gradient"]).max())
    assert abs(want["loss"][1]) > 1e-2 and want["loss"][2] > 1e-2
    # the entropy is the SUM over the agents: above what one five-way head can have, at most N log 5
    assert np.log(5) < want["loss"][3] <= 3 * np.log(5) + 1e-9
    # a subset of rows is the objective on those rows of the fragment
    rows = torch.tensor([7, 0, 14, 3, 9])
    sub = {k: (v[rows] if k in ("h0", "c0", "last_value", "prev_action0") else v[:, rows]) for k, v in frag64.items()}
    want_sub = jl.ppo_by_hand(m64, sub, adv[:, rows], targets[:, rows], **settings)
    got_sub = ln.PPOLearner(got64, fused=False, **settings).losses(frag64, adv, targets, rows)
    got_sub = np.array([float(got_sub[k].detach()) for k in jl.LOSS_TERMS])
    assert np.abs(got_sub - want_sub["loss"]).max() <= 1e-12 * max(1.0, np.abs(want_sub["loss"]).max())


def test_update_runs_on_a_joint_fragment_and_casts_the_rewards_once():
    ln = _learner()
    frag, frag64, _, targets, settings, m = _objective_case()
    adv = torch.from_numpy(jl.gae64(frag, 0.99, 0.95)[0])
    m64 = copy.deepcopy(m).double()
    want = jl.ppo_by_hand(m64, frag64, jl.standardised(adv), targets, **settings)["loss"]
    learner = ln.PPOLearner(copy.deepcopy(m64), lr=0.0, epochs=1, minibatches=1, fused=False, **settings)
    terms = learner.update(frag64, adv, targets)
    got = np.array([float(terms[k]) for k in jl.LOSS_TERMS])
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max()), (got, want)
    assert frag64["prev_rewards"].dtype == torch.float64  # the caller's fragment is left as it is
    mod = copy.deepcopy(m)
    learner = ln.PPOLearner(mod, epochs=2, minibatches=4, seed=5, fused=False, **settings)
    parts = learner.minibatch_rows(15)
    assert sorted(torch.cat(parts).tolist()) == list(range(15))  # the rows are the 15 envs
    out = learner.update(frag, adv.float(), targets.float())
    assert all(torch.isfinite(v) for v in out.values()) and (mod.flat_params() - m.flat_params()).abs().max() > 1e-4


@pytest.mark.parametrize("boot", (False, True))
def test_gae_equals_the_numpy_loop(boot):
    ln = _learner()
    T, B = 7, 9
    term = np.zeros((T, B), np.uint8)
    trunc = np.zeros((T, B), np.uint8)
    term[2, 1], term[6, 2] = 1, 1
    term[3, 4], trunc[3, 4] = 1, 1  # the time limit raises both
    trunc[6, 5], term[0, 6], term[1, 6] = 1, 1, 1
    frag = jl.synthetic_fragment(T, B, 3, 3, 2, seed=3, flags=(term, trunc))
    bv = torch.from_numpy(np.random.default_rng(1).standard_normal((T, B)).astype(np.float32)) if boot else None
    want_adv, want_tgt = jl.gae64(frag, 0.97, 0.9, None if bv is None else bv.numpy())
    adv, tgt = ln.gae(frag, 0.97, 0.9, boot_value=bv)
    assert adv.shape == (T, B) and adv.dtype == torch.float32 and tgt.dtype == torch.float32
    assert np.abs(adv.numpy() - want_adv).max() <= 32 * np.finfo(np.float32).eps * np.abs(want_adv).max()
    assert np.abs(tgt.numpy() - want_tgt).max() <= 32 * np.finfo(np.float32).eps * np.abs(want_tgt).max()
    out = (torch.empty(T, B), torch.empty(T, B))
    a2, t2 = ln.gae(frag, 0.97, 0.9, boot_value=bv, out=out)
    assert a2 is out[0] and torch.equal(a2, adv) and torch.equal(t2, tgt)
    # in float64 it is the loop's numbers
    f64 = dict(_f64(frag), rewards=frag["rewards"].float().double())
    adv64 = ln.gae(f64, 0.97, 0.9, boot_value=None if bv is None else bv.double())[0]
    assert np.abs(adv64.numpy() - want_adv).max() <= 1e-12
    with pytest.raises(ValueError, match="out must be two"):
        ln.gae(frag, out=(torch.empty(T, B, 1), torch.empty(T, B)))
    with pytest.raises(ValueError, match="boot_value"):
        ln.gae(frag, boot_value=torch.zeros(T, B, 2))


@pytest.mark.parametrize("recurrent", (True, False))
def test_sequence_forward_equals_chained_forward_calls(recurrent):
    ln = _learner()
    T, B, H, W, N = 6, 9, 5, 7, 3
    frag = jl.synthetic_fragment(T, B, H, W, N, seed=5)
    assert frag["first"][1:].any() and frag["first"][0].any() and not frag["first"][0].all()
    m = ju.make_module(H * W, N, recurrent, seed=7)
    m64 = copy.deepcopy(m).double()
    with torch.no_grad():
        want = jl.chained_forward(m64, _f64(frag))
        got64 = ln.sequence_forward(m64, _f64(frag), fused=False)
        got32 = ln.sequence_forward(m, frag, fused=True)  # CPU tensors always take the loop
        chained32 = jl.chained_forward(m, frag)
    assert got64[0].shape == (T, B, 5 * N) and got64[1].shape == (T, B)
    for g, w in zip(got64, want):
        assert np.abs(g.numpy() - w.numpy()).max() <= 1e-12
    dev = max(float(np.abs(c.double().numpy() - w.numpy()).max()) for c, w in zip(chained32, want))
    assert dev > 0
    for g, w in zip(got32, want):
        assert np.abs(g.double().numpy() - w.numpy()).max() <= 16 * dev
    rows = torch.tensor([7, 0, 3])
    with torch.no_grad():
        sub = ln.sequence_forward(m64, _f64(frag), rows, fused=False)
    assert sub[0].shape == (T, 3, 5 * N) and np.abs(sub[0].numpy() - want[0][:, rows].numpy()).max() <= 1e-12
    assert np.abs(sub[1].numpy() - want[1][:, rows].numpy()).max() <= 1e-12
    # the state before step 0 and the previous action count, where the row does not start an episode
    if recurrent:
        other = dict(_f64(frag), h0=torch.zeros(B, 64, dtype=torch.float64))
        with torch.no_grad():
            moved = (ln.sequence_forward(m64, other, fused=False)[0][0] - want[0][0]).abs().amax(dim=1)
        # (a started row ignores h0; the batched products may still sum its terms in another order: float64 rounding)
        assert (moved[frag["first"][0] == 0] > 1e-6).all() and (moved[frag["first"][0] != 0] <= 1e-12).all()


def test_fragment_keys_and_shapes_are_validated():
    ln = _learner()
    frag = jl.synthetic_fragment(4, 3, 3, 3, 2)
    m = ju.make_module(9, 2, True)
    assert ln.check_fragment(frag) == (4, 3, 2, 19) and ln.is_joint(frag)
    assert not ln.is_joint(lu.synthetic_fragment(4, 3, 2, 16, False))
    for key in ln.FRAGMENT_KEYS:
        with pytest.raises(ValueError, match=key):
            ln.sequence_forward(m, {k: v for k, v in frag.items() if k != key})
        with pytest.raises(ValueError, match=key):
            ln.gae({k: v for k, v in frag.items() if k != key})
    with pytest.raises(ValueError, match="h0"):
        ln.sequence_forward(m, dict(frag, h0=frag["h0"][:-1]))
    with pytest.raises(ValueError, match="terminated"):
        ln.gae(dict(frag, terminated=frag["terminated"][:, :-1]))
    with pytest.raises(ValueError, match="last_value"):
        ln.gae(dict(frag, last_value=frag["last_value"][:, None]))
    with pytest.raises(ValueError, match="actions"):
        ln.check_fragment(dict(frag, actions=frag["actions"][:, :, 0]))
    with pytest.raises(ValueError, match="prev_action0"):
        ln.check_fragment(dict(frag, prev_action0=frag["prev_action0"][:, :1]))
    with pytest.raises(ValueError, match="logp"):
        ln.PPOLearner(m).losses(dict(frag, logp=frag["logp"][:, :, None]), frag["value"], frag["value"])
    # each kind of fragment needs its kind of module
    with pytest.raises(ValueError, match="JointActionPolicy"):
        ln.sequence_forward(pu.make_module(19, True, True), frag)
    with pytest.raises(ValueError, match="joint fragment"):
        ln.sequence_forward(m, lu.synthetic_fragment(4, 3, 2, 19, True))
    with pytest.raises(ValueError, match="3 agents|takes 24"):
        ln.sequence_forward(ju.make_module(9, 3, True), frag)
