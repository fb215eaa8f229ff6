"""One policy per agent (DTE) without a GPU: the torch rule (``PerAgentPolicy``), its checkpoint, ``sequence_forward`` and the
PPO learner of N independent nets in torch ops on the CPU, and the argument errors of the scripts and the other learners."""

import copy
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import dte_util as du
import learner_util as lu
import policy_util as pu
from trace_util import ROOT


def _policy():
    from dl_reference_models_amd import policy

    return policy


def _learner():
    from dl_reference_models_amd import learner

    return learner


def _f64(frag):
    return {k: (v.double() if v.dtype == torch.float32 else v) for k, v in frag.items()}


@pytest.mark.parametrize("recurrent", (True, False))
@pytest.mark.parametrize("mask", (True, False))
def test_forward_is_each_agents_own_forward(recurrent, mask):
    N, B, L = 3, 4, 16
    m = du.make_per_agent(N, L, mask, recurrent)
    assert m.KIND == "per_agent" and len(m.agents) == N
    rng = np.random.default_rng(0)
    obs = torch.from_numpy(rng.uniform(0, 1, (B * N, L)).astype(np.float32))
    pa = torch.from_numpy(rng.integers(0, 5, B * N).astype(np.int8))
    pr = torch.from_numpy(rng.uniform(-1, 1, B * N).astype(np.float32))
    start = torch.from_numpy(np.repeat(np.array([1, 0, 0, 1], np.uint8), N))
    state = (torch.from_numpy(rng.uniform(-1, 1, (B * N, 64)).astype(np.float32)),
             torch.from_numpy(rng.uniform(-1, 1, (B * N, 64)).astype(np.float32))) if recurrent else None
    with torch.no_grad():
        logits, value, new = m(obs, pa, pr, start, state)
        assert logits.shape == (B * N, 5) and value.shape == (B * N,)
        for a in range(N):
            s = slice(a, None, N)
            lg, v, st = m.agents[a](obs[s], pa[s], pr[s], start[s], None if state is None else (state[0][s], state[1][s]))
            assert torch.equal(logits[s], lg) and torch.equal(value[s], v)
            if recurrent:
                assert torch.equal(new[0][s], st[0]) and torch.equal(new[1][s], st[1])
        # the nets differ: agent 0's rows through agent 1's net are something else
        assert not torch.equal(logits[0::N], m.agents[1](obs[0::N], pa[0::N], pr[0::N], start[0::N],
                                                         None if state is None else (state[0][0::N], state[1][0::N]))[0])
    with pytest.raises(ValueError, match="whole number of envs"):
        m(obs[:-1])


def test_flat_params_is_the_concatenation_and_the_state_dict_is_policy_major():
    m = du.make_per_agent(3, 11, False, True)
    assert torch.equal(m.flat_params(), torch.cat([a.flat_params() for a in m.agents]))
    names = list(m.state_dict())
    per = len(m.agents[0].state_dict())
    assert names[:per] == ["agents.0." + k for k in m.agents[0].state_dict()] and names[per].startswith("agents.1.")
    for bad in (0, 65):
        with pytest.raises(ValueError, match="num_agents"):
            _policy().PerAgentPolicy(bad, 11)
    shared = pu.make_module(11, False, True, seed=3)
    copies = _policy().PerAgentPolicy.from_shared(shared, 4)
    assert copies.num_agents == 4 and all(torch.equal(a.flat_params(), shared.flat_params()) for a in copies.agents)
    copies.agents[0].fc1.bias.data += 1  # copies, not views
    assert not torch.equal(copies.agents[0].flat_params(), copies.agents[1].flat_params())


def test_checkpoint_round_trip_and_the_wrong_kind_names_the_loader(tmp_path):
    P = _policy()
    m = du.make_per_agent(3, 16, True, True)
    path, shared_path = tmp_path / "dte.pt", tmp_path / "shared.pt"
    m.save(path)
    back = P.PerAgentPolicy.load(path)
    assert back.config() == m.config() == {"num_agents": 3, "obs_len": 16, "has_mask": True, "recurrent": True, "hidden": 64}
    assert torch.equal(back.flat_params(), m.flat_params())
    assert isinstance(P.load_policy(path), P.PerAgentPolicy)
    with pytest.raises(ValueError, match=re.escape("PerAgentPolicy.load")):
        P.MaskedRecurrentPolicy.load(path)
    # every agent is itself a loadable shared policy
    m.agents[1].save(shared_path)
    one = P.MaskedRecurrentPolicy.load(shared_path)
    assert torch.equal(one.flat_params(), m.agents[1].flat_params()) and isinstance(P.load_policy(shared_path), P.MaskedRecurrentPolicy)
    with pytest.raises(ValueError, match=re.escape("MaskedRecurrentPolicy.load")):
        P.PerAgentPolicy.load(shared_path)


@pytest.mark.parametrize("recurrent", (True, False))
def test_sequence_forward_equals_the_chained_forward_calls(recurrent):
    """To fp32 rounding: as far from the float64 run as the T chained fp32 ``forward`` calls are, within the margin
    test_learner_host uses for the shared module (learner_util.FORWARD_MARGIN x dev)."""
    T, B, N, L = 5, 6, 3, 16
    frag = lu.synthetic_fragment(T, B, N, L, True, seed=3)
    m = du.make_per_agent(N, L, True, recurrent)
    want = [x.detach().numpy() for x in lu.chained_forward(copy.deepcopy(m).double(), _f64(frag))]
    with torch.no_grad():
        chained = [x.double().numpy() for x in lu.chained_forward(m, frag)]
        got = [x.double().numpy() for x in _learner().sequence_forward(m, frag, fused=False)]
        rows = torch.tensor([4, 0, 3])
        sub = [x.double().numpy() for x in _learner().sequence_forward(m, frag, rows, fused=False)]
    assert got[0].shape == (T, B, N, 5) and got[1].shape == (T, B, N) and sub[0].shape == (T, 3, N, 5)
    for name, w, c32, g32, s32 in zip(("logits", "value"), want, chained, got, sub):
        dev = np.abs(c32 - w).max()
        g32 = g32.reshape(w.shape)
        assert 0 < dev < 1e-4 and np.abs(g32 - w).max() <= lu.FORWARD_MARGIN * dev, (name, dev, np.abs(g32 - w).max())
        # rows index the envs: a subset is the same envs of the whole
        whole = g32.reshape(T, B, N, -1)[:, rows.numpy()]
        assert np.abs(s32.reshape(whole.shape) - whole).max() <= lu.FORWARD_MARGIN * dev, name


@pytest.mark.parametrize("recurrent", (True, False), ids=("recurrent", "feed_forward"))
@pytest.mark.parametrize("mask", (True, False), ids=("mask", "no_mask"))
def test_the_learner_is_n_independent_learners(recurrent, mask):
    """In float64 a reordering of sums costs about 1e-15 and a wiring error (another agent's data, a wrong normaliser, a
    shared mean) O(1): the gradient of the summed loss on every agent's parameters must equal, within 1e-9 x the largest
    gradient entry, the gradient of the shared learner's loss on that agent's net alone, its slice of the fragment and
    its own standardised advantages."""
    ln = _learner()
    T, B, N, L = 5, 8, 3, 16
    frag = _f64(lu.synthetic_fragment(T, B, N, L, mask, seed=5))
    adv, targets = (x.double() for x in ln.gae({k: (v.float() if v.dtype == torch.float64 else v) for k, v in frag.items()}))
    adv = du.standardised_per_agent(adv)
    m = du.make_per_agent(N, L, mask, recurrent).double().train()
    learner = ln.PPOLearner(m, fused=False)
    terms = learner.losses(frag, adv, targets)
    terms["total_loss"].backward()
    assert set(terms["per_policy"]) == set(lu.LOSS_TERMS) and all(v.shape == (N,) for v in terms["per_policy"].values())
    assert torch.allclose(terms["total_loss"], terms["per_policy"]["total_loss"].sum(), rtol=1e-12, atol=0)
    for a in range(N):
        alone = copy.deepcopy(m.agents[a])
        alone.zero_grad()
        single = ln.PPOLearner(alone, fused=False).losses(du.agent_fragment(frag, a), adv[:, :, a:a + 1], targets[:, :, a:a + 1])
        single["total_loss"].backward()
        for k in lu.LOSS_TERMS:
            assert abs(float(single[k].detach()) - float(terms["per_policy"][k][a].detach())) <= 1e-9 * max(1.0, abs(float(single[k].detach()))), (a, k)
        want = torch.cat([p.grad.reshape(-1) for p in alone.parameters()])
        got = torch.cat([p.grad.reshape(-1) for p in m.agents[a].parameters()])
        big = float(want.abs().max())
        assert big > 1e-4 and float((got - want).abs().max()) <= 1e-9 * big, (a, float((got - want).abs().max()), big)


def test_update_reports_the_mean_over_the_policies_and_each_policy():
    ln = _learner()
    T, B, N, L = 5, 8, 3, 16
    frag = lu.synthetic_fragment(T, B, N, L, True, seed=6)
    adv, targets = ln.gae(frag)

    def run(grad_clip=None):
        m = du.make_per_agent(N, L, True, True).train()
        learner = ln.PPOLearner(m, epochs=2, minibatches=3, seed=4, fused=False, grad_clip=grad_clip)
        assert [len(r) for r in learner.minibatch_rows(B)] == [3, 3, 2]  # envs, not agent rows
        return m, learner.update(frag, adv, targets)

    (m1, out), (m2, again), (m3, _clipped) = run(), run(), run(grad_clip=1e-3)
    assert set(out) == set(lu.LOSS_TERMS) | {"per_policy"} and set(out["per_policy"]) == set(lu.LOSS_TERMS)
    for k in lu.LOSS_TERMS:
        assert out["per_policy"][k].shape == (N,) and torch.allclose(out[k], out["per_policy"][k].mean(), rtol=1e-6, atol=1e-8), k
        assert torch.equal(out[k], again[k])  # the same seed: the same minibatches
    assert torch.equal(m1.flat_params(), m2.flat_params()) and not torch.equal(m1.flat_params(), m3.flat_params())
    fresh = du.make_per_agent(N, L, True, True)
    for a in range(N):  # every policy moved, and no two are the same net
        assert not torch.equal(m1.agents[a].flat_params(), fresh.agents[a].flat_params())
        assert not torch.equal(m1.agents[a].flat_params(), m1.agents[(a + 1) % N].flat_params())


@pytest.mark.parametrize("grad_clip", (0.5, 1e-3), ids=("clip_0.5", "clip_1e-3"))
def test_update_with_clipping_is_n_independent_updates(grad_clip):
    """The argument of test_the_learner_is_n_independent_learners carried through ``update``: 2 epochs of 3 minibatches with
    ``grad_clip`` (0.5, and 1e-3, which clips every policy in every step) must leave every ``agents[a]`` within 1e-9 x the
    largest parameter change of a shared learner run alone on a copy of that agent, its slice of the fragment, its own
    standardised advantages and the same minibatches.  (Before the rows view both LSTM biases of an agent shared one gradient
    storage and were clipped twice: agent 0 then deviated by 1.7e-3 where its parameters change by 6.0e-3 at most at 0.5, and by 5.0e-3 of 6.0e-3 at 1e-3.)"""
    ln = _learner()
    T, B, N, L = 5, 8, 3, 16
    frag = _f64(lu.synthetic_fragment(T, B, N, L, True, seed=5))
    adv, targets = ln.gae(frag)
    kw = dict(epochs=2, minibatches=3, seed=4, fused=False)
    # one agent per env: the rows are the envs, so the same seed draws the same minibatches as the per-agent learner's
    a_draw, b_draw = (ln.PPOLearner(pu.make_module(L, True, True), **kw) for _ in range(2))
    for _ in range(kw["epochs"]):
        assert all(torch.equal(x, y) for x, y in zip(a_draw.minibatch_rows(B), b_draw.minibatch_rows(B * 1)))
    start = du.make_per_agent(N, L, True, True).double().train()
    clipped, free = copy.deepcopy(start), copy.deepcopy(start)
    ln.PPOLearner(clipped, grad_clip=grad_clip, **kw).update(frag, adv, targets)
    ln.PPOLearner(free, grad_clip=None, **kw).update(frag, adv, targets)
    flat = lambda net: torch.cat([p.detach().reshape(-1) for p in net.parameters()])  # noqa: E731
    for a in range(N):
        alone = copy.deepcopy(start.agents[a])
        ln.PPOLearner(alone, grad_clip=grad_clip, **kw).update(du.agent_fragment(frag, a), adv[:, :, a:a + 1], targets[:, :, a:a + 1])
        moved = float((flat(alone) - flat(start.agents[a])).abs().max())
        off = float((flat(clipped.agents[a]) - flat(alone)).abs().max())
        print(f"grad_clip {grad_clip}, agent {a}: largest parameter change {moved:.3e}, deviation from the agent alone {off:.3e}")
        assert moved > 1e-4 and off <= 1e-9 * moved, (a, off, moved)
        # the clip was at work for this policy: without it the net ends up somewhere else
        assert float((flat(free.agents[a]) - flat(alone)).abs().max()) > 1e-3 * moved, a


def test_no_two_parameters_share_a_gradient_after_backward():
    """``clip_grad_norm_`` scales every ``.grad`` in place, once per parameter: two parameters on one storage would be scaled
    twice (and counted twice in the norm)."""
    ln = _learner()
    T, B, N, L = 5, 8, 3, 16
    frag = lu.synthetic_fragment(T, B, N, L, True, seed=5)
    adv, targets = ln.gae(frag)
    m = du.make_per_agent(N, L, True, True).train()
    ln.PPOLearner(m, fused=False).losses(frag, adv, targets)["total_loss"].backward()
    ptrs = [p.grad.data_ptr() for p in m.parameters()]
    assert all(p.grad is not None for p in m.parameters()) and len(set(ptrs)) == len(ptrs) == N * 12


def test_lstm_sequence_on_the_cpu_takes_interleaved_groups():
    c = du.lstm_case((5, 65, 5), "scattered")
    G = 5
    t = {k: (None if v is None else torch.from_numpy(v)) for k, v in c["inp"].items()}
    h, (hT, cT) = _learner().lstm_sequence(t["xg"], t["whh"], t["reset"], t["h0"], t["c0"])
    for g in range(G):
        gi = {k: (None if v is None else torch.from_numpy(v)) for k, v in du.group_inputs(c["inp"], g, G).items()}
        hg, (hTg, cTg) = _learner().lstm_sequence(gi["xg"], gi["whh"], gi["reset"], gi["h0"], gi["c0"])
        assert torch.allclose(h[:, g::G], hg, rtol=0, atol=1e-6) and torch.allclose(cT[g::G], cTg, rtol=0, atol=1e-6)
    with pytest.raises(ValueError, match="interleaved groups"):
        _learner().lstm_sequence(t["xg"][:, :-1], t["whh"], None, t["h0"][:-1], t["c0"][:-1])


def test_dte_is_refused_by_name_where_it_is_out_of_scope(tmp_path):
    from dl_reference_models_amd import dqn

    m = du.make_per_agent(3, 16, True, True)
    with pytest.raises(ValueError, match="DTE"):
        _learner().IMPALALearner(m)
    with pytest.raises(ValueError, match="DTE"):
        dqn.DQNLearner(m)
    with pytest.raises(ValueError, match="DTE"):
        _policy().JointDevicePolicy(m, 4)
    # an env with another agent count: refused before anything touches the device (a stand-in env is all it reads)
    import types

    from dl_reference_models_amd import evaluation as ev

    env = types.SimpleNamespace(num_envs=2, num_agents=4, obs_len=16, device=torch.device("cuda:0"))
    path = tmp_path / "dte.pt"
    m.save(path)
    for policy in (m, str(path)):
        with pytest.raises(ValueError, match="one policy for each of 3 agents"):
            ev.neural_policy(env, policy)
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "scripts", "train_multi_agent_env.py"))
    train = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(train)
    for algo in ("IMPALA", "DQN"):
        with pytest.raises(SystemExit, match="DTE"):
            train.main(["--execution-mode", "DTE", "--algo", algo, "--iters", "1"])
    assert train.parse_args([]).execution_mode == "CTDE"


def test_abi_is_declared_and_exported():
    from dl_reference_models_amd import _lib as L

    header = open(os.path.join(ROOT, "include", "mapf_step.h")).read()
    for name in ("mapf_policy_create_per_agent", "mapf_lstm_seq_forward_grouped", "mapf_lstm_seq_backward_grouped"):
        assert name in L.EXPORTED_SYMBOLS and re.search(r"^int " + name + r"\(", header, re.M), name
