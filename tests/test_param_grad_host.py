"""The fused parameter gradients on the CPU: the ``fused_grads`` keyword changes nothing for CPU tensors, argument checks raise
what they raised, the header, the library table and the scripts know the new unit, and the NumPy restatement of dW_hh
(param_grad_util) agrees with torch autograd through the learner's own loop in float64."""

import copy
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

import learner_util as lu
import param_grad_util as pg
import trunk_util as tu
from policy_util import make_module
from trace_util import ROOT


def _ln():
    from dl_reference_models_amd import learner as ln

    return ln


@pytest.mark.parametrize("recurrent,mask", ((True, True), (False, False)))
def test_fused_grads_on_cpu_tensors_is_bit_for_bit_the_path_without_it(recurrent, mask):
    ln = _ln()
    T, B, N = 5, 6, 3
    L = 14 if mask else 9
    frag = lu.synthetic_fragment(T, B, N, L, mask, seed=3)
    module = make_module(L, mask, recurrent, seed=1).train()
    plain = ln.sequence_forward(module, frag, fused=False)
    for kw in ({"fused_grads": False}, {"fused_grads": True}, {"fused_grads": True, "fused_trunk": True}):
        for fused in (False, True):  # (CPU tensors take the loop whatever ``fused`` says)
            got = ln.sequence_forward(module, frag, fused=fused, **kw)
            assert all(torch.equal(x, y) for x, y in zip(got, plain)), (kw, fused)
    adv, tgt = ln.gae(frag)
    grads = []
    for cls, args in ((ln.PPOLearner, (frag, adv, tgt)), (ln.IMPALALearner, (frag,))):
        for kw in ({}, {"fused_grads": False}, {"fused_grads": True}, {"fused_grads": True, "fused_trunk": True}):
            m = copy.deepcopy(module)
            learner = cls(m, **kw)
            assert learner.fused_grads is bool(kw.get("fused_grads", False))
            terms = learner.losses(*args)
            terms["total_loss"].backward()
            grads.append((terms["total_loss"].detach(), torch.cat([p.grad.reshape(-1) for p in m.parameters()])))
        for total, flat in grads[-3:]:
            assert torch.equal(total, grads[-4][0]) and torch.equal(flat, grads[-4][1]), cls.__name__


def test_the_ops_on_cpu_tensors_ignore_the_keyword():
    ln = _ln()
    case = lu.lstm_case((2, 33), "scattered")
    t = {k: (None if v is None else torch.from_numpy(v)) for k, v in case["inp"].items()}
    res = []
    for kw in ({}, {"fused_grads": True}):
        whh = t["whh"].clone().requires_grad_(True)
        h, (hT, cT) = ln.lstm_sequence(t["xg"], whh, t["reset"], t["h0"], t["c0"], **kw)
        ((h * t["dh"]).sum() + (hT * t["dhT"]).sum()).backward()
        res.append((h.detach(), whh.grad))
    assert all(torch.equal(x, y) for x, y in zip(*res))
    T, R, L = 2, 3, 14
    module = make_module(L, True, True)
    obs, pa = torch.rand(T, R, L), torch.zeros(T, R, 1, dtype=torch.int8)
    pr, first = torch.rand(T, R), torch.zeros(T, R, dtype=torch.uint8)
    one, two = ln.dense_trunk(module, obs, pa, pr, first), ln.dense_trunk(module, obs, pa, pr, first, fused_grads=True)
    assert all(torch.equal(x, y) for x, y in zip(one, two))


def test_every_class_takes_the_keyword_and_argument_checks_raise_as_before():
    ln = _ln()
    from dl_reference_models_amd.policy import JointActionPolicy, PerAgentPolicy, PopulationPolicy
    import inspect

    from dl_reference_models_amd.population import PopulationTrainer

    module = make_module(14, True, True)
    for cls in (ln.PPOLearner, ln.IMPALALearner, ln.BCLearner):
        assert cls(module).fused_grads is False and cls(module, fused_grads=True).fused_grads is True
        assert cls(module, fused_grads=True).fused_trunk is False  # (the option does not imply the other one)
    # the option alone is taken with every module kind; together with fused_trunk the kind is refused as before
    for other in (JointActionPolicy(16, 2), PerAgentPolicy(2, 14, has_mask=True), PopulationPolicy(2, 2, 14, has_mask=True)):
        assert ln.PPOLearner(other, fused_grads=True).fused_grads is True
        with pytest.raises(ValueError, match="fused_trunk is not supported for a"):
            ln.PPOLearner(other, fused_trunk=True, fused_grads=True)
    for fn in (ln.lstm_sequence, ln.dense_trunk, ln.sequence_forward, ln._forward, ln.Trainer.__init__, PopulationTrainer.__init__):
        assert inspect.signature(fn).parameters["fused_grads"].default is False, fn
    T, R, L = 2, 3, 14
    obs, pa = torch.zeros(T, R, L), torch.zeros(T, R, 1, dtype=torch.int8)
    pr, first = torch.zeros(T, R), torch.zeros(T, R, dtype=torch.uint8)
    for bad, match in (({"obs": torch.zeros(T, R, L + 1)}, "obs must be"), ({"prev_actions": None}, "needs prev_actions"),
                       ({"first": torch.zeros(T, R)}, "first must be")):
        args = dict({"obs": obs, "prev_actions": pa, "prev_rewards": pr, "first": first}, **bad)
        with pytest.raises(ValueError, match=match):
            ln.dense_trunk(module, fused_grads=True, **args)
    xg, whh, h0 = torch.zeros(T, R, 256), torch.zeros(256, 64), torch.zeros(R, 64)
    for bad, match in (({"xg": torch.zeros(T, R, 255)}, "xg must be"), ({"whh": torch.zeros(2, 256, 64)}, "interleaved groups"),
                       ({"h0": torch.zeros(R + 1, 64)}, "h0 must be"), ({"reset": torch.zeros(T, R)}, "reset must be uint8")):
        args = dict({"xg": xg, "whh": whh, "reset": None, "h0": h0, "c0": h0}, **bad)
        with pytest.raises(ValueError, match=match):
            ln.lstm_sequence(fused_grads=True, **args)


def test_header_library_table_and_scripts_know_the_unit():
    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd import build

    header = open(os.path.join(ROOT, "include", "mapf_step.h")).read()
    for name in ("mapf_trunk_param_grad", "mapf_lstm_seq_param_grad"):
        assert name in L.EXPORTED_SYMBOLS and re.search(r"^int " + name + r"\(", header, re.M), name
    assert "mapf_param_grad_workspace_bytes" in L.EXPORTED_SYMBOLS and re.search(r"^int64_t mapf_param_grad_workspace_bytes\(", header, re.M)
    rows = int(re.search(r"^#define MAPF_PARAM_GRAD_SLAB_ROWS (\d+)", header, re.M).group(1))
    slabs = int(re.search(r"^#define MAPF_PARAM_GRAD_MAX_SLABS (\d+)", header, re.M).group(1))
    assert rows == L.PARAM_GRAD_SLAB_ROWS == pg.SLAB_ROWS and slabs == L.PARAM_GRAD_MAX_SLABS == pg.MAX_SLABS
    assert ("grad", "mapf_grad.hip") in [(n, s) for n, s, _w in build.UNITS]
    assert all("grad" in [n for n, _s, _d in build.VARIANTS[v][2]] for v in build.VARIANTS)

    def script(name):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, "scripts", name + ".py"))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod

    for mod in (script("train_multi_agent_env"), script("train_single_agent_env")):
        assert mod.parse_args([]).fused_grads is False and mod.parse_args(["--fused-grads"]).fused_grads is True


def test_the_shapes_the_gpu_tests_derive_from_the_partition():
    S, N = pg.SLAB_ROWS, pg.MAX_SLABS
    assert {S - 1, S, S + 1, 2 * S + 3} <= set(pg.TRUNK_ROWS) and pg.CAPPED_ROWS == S * N + 1
    sizes = sorted(T * R for T, R, G in pg.DWHH_SHAPES if G == 1)
    assert any(S < n <= S + 8 for n in sizes) and any(2 * S < n <= 2 * S + 8 for n in sizes)
    T, R, G = pg.DWHH_CAPPED
    assert (T, G) == (5, 1) and S * N < T * R <= S * N + 5


@pytest.mark.parametrize("reset", pg.RESETS)
@pytest.mark.parametrize("T,R,groups", pg.DWHH_SHAPES[:7])
def test_the_dwhh_restatement_agrees_with_autograd_through_the_loop(T, R, groups, reset):
    """dxg of a real recurrence (autograd through ``_lstm_loop`` in float64, a leaf added to xg) and its h into the NumPy formula:
    the result is autograd's own gradient with respect to whh."""
    ln = _ln()
    rng = np.random.default_rng(13 * T + R + groups)
    tt = lambda *s: torch.from_numpy(rng.standard_normal(s))  # noqa: E731
    xg, h0, c0, dh = tt(T, R, 256).requires_grad_(True), tt(R, 64) * 0.5, tt(R, 64), tt(T, R, 64)
    whh = (tt(groups, 256, 64) * 0.1 if groups > 1 else tt(256, 64) * 0.1).requires_grad_(True)
    reset_np = pg.reset_pattern(reset, T, R, rng)
    h, _hT, _cT = ln._lstm_loop(xg, whh, None if reset_np is None else torch.from_numpy(reset_np), h0, c0)
    (h * dh).sum().backward()
    got = pg.dwhh_np(xg.grad.numpy(), h.detach().numpy(), h0.numpy(), reset_np, groups, np.float64)
    want = whh.grad.numpy().reshape(groups, 256, 64)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, float(np.abs(want).max()))


def test_the_trunk_kernel_inputs_hide_what_must_not_be_read():
    case = tu.trunk_case(33, 53, 58, True)
    k = pg.trunk_kernel_inputs(case)
    started = case["inp"]["first"] != 0
    assert started.any() and (k["prev_action"][started] == 77).all() and np.isnan(k["prev_reward"][started]).all()
    assert np.isnan(k["obs"][:, 53:]).all() and all(k[q].dtype == np.float32 for q in ("a1", "a2", "dpre1", "dpre2"))
    assert all(pg.trunk_dev(case, q) > 0 for q in tu.PARAM_GRADS)
