"""The joint-action policy without a GPU: the torch module against the float64 restatement of the rule
(joint_policy_util), the layout of the parameter vector, the header and the symbol list, the counter-based noise, the
checkpoint round trip, the property of the shared cases that the GPU test relies on, and the splits of the kernel's schedule
(fc1's K over four waves, the head tiles, the extra k-steps of the gates) that the shapes reach, with two faults of a partly
filled upper quarter that only the shapes added for it can see."""

import os
import re

import numpy as np
import pytest
import torch

import joint_policy_util as ju
import policy_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = [(s, r, m) for s in ju.SHAPES for r in (True, False) for m in (False, True)]


@pytest.mark.parametrize("shape", ju.SHAPES[:5], ids=str)
@pytest.mark.parametrize("recurrent", (True, False))
def test_module_equals_the_restatement(shape, recurrent):
    """A second module and other inputs than the ones `dev` of the case was measured on: within 16 x dev."""
    c = ju.case(shape, recurrent, False)
    rows, H, W, N = shape
    rows = min(rows, 65)
    m = ju.make_module(H * W, N, recurrent, seed=1)
    p, cfg = ju.params64(m), m.config()
    rng = np.random.default_rng(5)
    state, state32, worst = None, None, 0.0
    with torch.no_grad():
        for t in range(ju.STEPS):
            obs = ju.draw_obs(rng, rows, H, W, N)
            pa = rng.integers(0, 5, size=(rows, N)).astype(np.int8)
            pr = rng.uniform(-1, 1, size=rows)
            start = rng.random(rows) < (0.3 if t else 1.0)
            logits, value, state = ju.forward64(p, cfg, obs, pa, pr, start, state)
            l32, v32, state32 = m(torch.from_numpy(obs), torch.from_numpy(pa), torch.from_numpy(pr), torch.from_numpy(start), state32)
            assert l32.shape == (rows, 5 * N) and v32.shape == (rows,) and l32.dtype == torch.float32
            worst = max(worst, np.abs(l32.numpy() - logits).max(), np.abs(v32.numpy() - value).max())
            if recurrent:
                worst = max(worst, np.abs(state32[0].numpy() - state[0]).max(), np.abs(state32[1].numpy() - state[1]).max())
    assert 0 < c["dev"] < 1e-5
    assert worst <= 16 * c["dev"], (worst, c["dev"])


@pytest.mark.parametrize("shape,recurrent,sample", ALL_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_case_inputs_leave_the_decisions_to_the_policy(shape, recurrent, sample):
    """dev > 0, and the share the restatement itself cannot decide (top-two gap within 32 x dev): at most 1 % of the
    decisions and 2 % of the rows of a case."""
    c = ju.case(shape, recurrent, sample)
    assert 0 < c["dev"] < 1e-5
    dec, rows = ju.undecided(c)
    print(f"joint case {shape} recurrent={recurrent} sample={sample}: dev {c['dev']:.3e}, undecided decisions {dec:.4%}, rows {rows:.4%}")
    assert dec <= ju.MAX_UNDECIDED_DECISIONS and rows <= ju.MAX_UNDECIDED_ROWS
    assert [t for t in range(ju.STEPS) if c["flags"][t].any()] == [2, 4]
    assert ju.start_rows(shape[0]) == sorted({0, min(32, shape[0] - 1), shape[0] - 1})
    # the observation is the env's: 0/1 cells, one cell per agent and goal code, a 0/1 mask that allows NO_OP
    H, W, N = shape[1:]
    grid, mask = c["obs"][..., :H * W], c["obs"][..., H * W:].reshape(ju.STEPS, shape[0], N, 5)
    for code in range(2, 2 + 2 * N):
        assert ((grid == code).sum(axis=-1) == 1).all()
    assert set(np.unique(mask)) <= {0.0, 1.0} and (mask[..., 0] == 1).all() and c["prev_reward"].dtype == np.float64


def test_module_is_differentiable_and_none_means_zeros():
    m = ju.make_module(35, 3, True)
    obs = torch.from_numpy(ju.draw_obs(np.random.default_rng(0), 7, 5, 7, 3))
    logits, value, (h, c) = m(obs)
    l2, v2, _ = m(obs, torch.zeros((7, 3), dtype=torch.int8), torch.zeros(7, dtype=torch.float64), torch.zeros(7, dtype=torch.uint8),
                  (torch.zeros(7, 64), torch.zeros(7, 64)))
    assert torch.equal(logits, l2) and torch.equal(value, v2)
    (logits[torch.isfinite(logits)].sum() + value.sum() + h.sum()).backward()
    assert all(q.grad is not None and torch.isfinite(q.grad).all() for q in m.parameters())
    assert m.config() == {"grid_cells": 35, "num_agents": 3, "recurrent": True, "hidden": 64}
    # a float64 previous reward is rounded to nearest fp32, as the kernel's load does
    pr = torch.tensor([1 / 3] * 7, dtype=torch.float64)
    a = m(obs, None, pr)[0]
    b = m(obs, None, pr.to(torch.float32))[0]
    assert torch.equal(a, b)


@pytest.mark.parametrize("recurrent", (True, False))
def test_flat_params_layout_is_the_headers(recurrent):
    F, N = 35, 3
    m = ju.make_module(F, N, recurrent)
    names = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias"]
    sizes = [64 * F, 64, 64 * 64, 64]
    if recurrent:
        names += ["lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih", "lstm.bias_hh"]
        sizes += [256 * (64 + 5 * N + 1), 256 * 64, 256, 256]
    names += ["pi.weight", "pi.bias", "vf.weight", "vf.bias"]
    sizes += [5 * N * 64, 5 * N, 64, 1]
    assert list(m.state_dict().keys()) == names
    assert [v.numel() for v in m.state_dict().values()] == sizes
    with torch.no_grad():
        for i, v in enumerate(m.state_dict().values()):
            v.fill_(float(i))
    flat = m.flat_params().numpy()
    assert flat.dtype == np.float32 and flat.size == sum(sizes)
    assert np.array_equal(flat, np.concatenate([np.full(s, i, np.float32) for i, s in enumerate(sizes)]))
    # the header names the same tensors in the same order
    text = open(os.path.join(ROOT, "include", "mapf_step.h")).read()
    block = text[text.index("state_dict order of policy.JointActionPolicy"):]
    block = block[:block.index("mapf_jpolicy_param_count returns")]
    found = re.findall(r"(fc1|fc2|lstm|pi|vf)\.(weight_ih|weight_hh|bias_ih|bias_hh|weight|bias)", block)
    all_names = ["fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "lstm.weight_ih", "lstm.weight_hh", "lstm.bias_ih",
                 "lstm.bias_hh", "pi.weight", "pi.bias", "vf.weight", "vf.bias"]
    assert [".".join(f) for f in found] == all_names


def test_header_and_exported_symbols_agree():
    from dl_reference_models_amd import _lib as L

    text = open(os.path.join(ROOT, "include", "mapf_step.h")).read()
    declared = set(re.findall(r"\b(mapf_jpolicy_\w+)\s*\(", text))
    want = {"mapf_jpolicy_create", "mapf_jpolicy_destroy", "mapf_jpolicy_param_count", "mapf_jpolicy_set_params", "mapf_jpolicy_act"}
    assert declared == want and want <= set(L.EXPORTED_SYMBOLS)
    assert f"#define MAPF_JPOLICY_MAX_CELLS {L.JPOLICY_MAX_CELLS}" in text and f"#define MAPF_JPOLICY_MAX_AGENTS {L.JPOLICY_MAX_AGENTS}" in text
    assert [f[0] for f in L.MapfJPolicyConfig._fields_] == re.findall(
        r"int32_t (\w+);", text[text.index("typedef struct mapf_jpolicy_config"):text.index("} mapf_jpolicy_config;")])
    lib = L.load()
    for s in want:
        assert hasattr(lib, s), s


def test_noise_in_python_integers_equals_the_numpy_one():
    rows, draws, N = np.array([0, 1, 31, 32, 2048, 2 ** 31 - 1]), np.array([0, 1, 2, 3, 4, 2 ** 32 - 1]), 64
    u = ju.uniform_np(12345, rows, draws, N)
    g = ju.gumbel_np(12345, rows, draws, N)
    assert u.shape == (6, 5 * N) and ((u > 0) & (u < 1)).all()
    for i, (r, d) in enumerate(zip(rows, draws)):
        for ag in (0, 1, 17, 63):
            for k in range(5):
                assert ju.uniform_int(12345, int(r), int(d), ag, k) == u[i, 5 * ag + k]
                assert abs(ju.gumbel_int(12345, int(r), int(d), ag, k) - g[i, 5 * ag + k]) <= 1e-12
    # for N = 1 it is the noise of the per-agent policy
    assert np.array_equal(ju.uniform_np(7, rows, draws, 1), pu.uniform_np(7, rows, draws))


def test_checkpoints_round_trip_and_refuse_the_other_kind(tmp_path):
    from dl_reference_models_amd.policy import JointActionPolicy, MaskedRecurrentPolicy

    j = ju.make_module(35, 3, True, seed=3)
    jp, mp = tmp_path / "joint.pt", tmp_path / "masked.pt"
    j.save(jp)
    back = JointActionPolicy.load(jp)
    assert back.config() == j.config() and torch.equal(back.flat_params(), j.flat_params())
    ff = ju.make_module(9, 1, False)
    ff.save(tmp_path / "ff.pt")
    assert JointActionPolicy.load(tmp_path / "ff.pt").recurrent is False
    m = pu.make_module(33, True, True)
    m.save(mp)
    assert torch.equal(MaskedRecurrentPolicy.load(mp).flat_params(), m.flat_params())
    with pytest.raises(ValueError, match="joint_action.*MaskedRecurrentPolicy.load reads kind 'masked_recurrent'"):
        MaskedRecurrentPolicy.load(jp)
    with pytest.raises(ValueError, match="masked_recurrent.*JointActionPolicy.load reads kind 'joint_action'"):
        JointActionPolicy.load(mp)
    # a checkpoint from before the key existed is the per-agent kind
    torch.save({"config": m.config(), "state_dict": m.state_dict()}, tmp_path / "old.pt")
    assert torch.equal(MaskedRecurrentPolicy.load(tmp_path / "old.pt").flat_params(), m.flat_params())
    with pytest.raises(ValueError, match="masked_recurrent"):
        JointActionPolicy.load(tmp_path / "old.pt")


def test_device_policy_has_no_cpu_path():
    from dl_reference_models_amd.policy import DevicePolicy, JointDevicePolicy

    with pytest.raises(ValueError, match="GPU only"):
        JointDevicePolicy(ju.make_module(9, 1, True), 4, device="cpu")
    with pytest.raises(TypeError, match="JointActionPolicy"):
        JointDevicePolicy(pu.make_module(33, True, True), 4, device="cpu")
    with pytest.raises(ValueError, match="GPU only"):
        DevicePolicy(pu.make_module(33, True, True), 5, 5, device="cpu")


# ---- the schedule of k_jpolicy_act that the shapes reach -------------------------------------------------------------------
def _splits(shape):
    return ju.fc1_split(shape[1] * shape[2])


def test_fc1_split_is_the_layout_rule():
    assert (ju.WAVES, ju.CHUNK, ju.QUARTER) == (4, 256, 32)
    full = [32, 32, 32, 32]
    want = {1: [[1, -31, -63, -95]], 9: [[5, -27, -59, -91]], 16: [[8, -24, -56, -88]], 35: [[18, -14, -46, -78]],
            63: [[32, 0, -32, -64]], 64: [[32, 0, -32, -64]], 65: [[32, 1, -31, -63]], 81: [[32, 9, -23, -55]],
            144: [[32, 32, 8, -24]], 196: [[32, 32, 32, 2]], 255: [full], 256: [full], 259: [full, [2, -30, -62, -94]],
            261: [full, [3, -29, -61, -93]], 340: [full, [32, 10, -22, -54]], 400: [full, [32, 32, 8, -24]],
            462: [full, [32, 32, 32, 7]], 600: [full, full, [32, 12, -20, -52]], 1024: [full] * 4, 4096: [full] * 16}
    assert {F: ju.fc1_split(F) for F in want} == want
    for F in range(1, 4097):
        split = ju.fc1_split(F)
        flat = [ns for per_wave in split for ns in per_wave]
        assert len(split) == -(-F // ju.CHUNK) and all(len(per_wave) == ju.WAVES for per_wave in split)  # one per chunk staged
        last = max(i for i, ns in enumerate(flat) if ns > 0)
        assert all(ns == ju.QUARTER for ns in flat[:last]) and all(ns <= 0 for ns in flat[last + 1:])
        assert sum(max(ns, 0) for ns in flat) == (F + 1) // 2  # every k-step walked once
        assert len(ju.partial_quarters(F)) <= 1
    assert ju.partial_quarters(400) == [(1, 2, 8)] and ju.partial_quarters(255) == [] and ju.partial_quarters(64) == []


def test_head_deal_and_extra_split_are_the_layout_rule():
    assert ju.head_deal(32) == (6, [[0, 4], [1, 5], [2], [3]])
    assert ju.head_deal(19) == (3, [[0], [1], [2], []]) and (5 * 19 + 1) % 32 == 0
    assert ju.head_deal(1) == (1, [[0], [], [], []]) and ju.head_deal(64) == (11, [[0, 4, 8], [1, 5, 9], [2, 6, 10], [3, 7]])
    assert ju.head_deal(26)[1] == [[0, 4], [1], [2], [3]] and ju.head_deal(51) == (8, [[0, 4], [1, 5], [2, 6], [3, 7]])
    for N in range(1, 65):
        HT, tiles = ju.head_deal(N)
        assert 32 * (HT - 1) < 5 * N + 1 <= 32 * HT and sorted(t for per_wave in tiles for t in per_wave) == list(range(HT))
        XS, lower, upper = ju.extra_split(N)
        assert 2 * (XS - 1) < 5 * N + 1 <= 2 * XS and lower == (0, XS // 2) and upper == (XS // 2, XS)
    assert ju.extra_split(2) == (6, (0, 3), (3, 6)) and ju.extra_split(25) == (63, (0, 31), (31, 63))
    assert ju.extra_split(64) == (161, (0, 80), (80, 161))


def test_the_shapes_walk_every_split_of_the_schedule():
    """Conditions on the table, from the layout rule: an edit of SHAPES cannot silently lose a path of the kernel."""
    assert ju.SHAPES == ju.OLD_SHAPES + ju.SPLIT_SHAPES and len(set(ju.SHAPES)) == len(ju.SHAPES) and len(ju.OLD_SHAPES) == 7
    # what the seven shapes from before reach: a partly filled quarter in wave 0 only, three tile counts
    old = [q for s in ju.OLD_SHAPES for q in ju.partial_quarters(s[1] * s[2])]
    assert sorted(old) == [(0, 0, 5), (0, 0, 8), (0, 0, 18), (1, 0, 3)]
    assert not any(ju.upper_partial(s) for s in ju.OLD_SHAPES)
    assert not any(ns == 0 for s in ju.OLD_SHAPES for per_wave in _splits(s) for ns in per_wave)
    assert {ju.head_deal(s[3])[0] for s in ju.OLD_SHAPES} == {1, 3, 11}
    # the whole table
    quarters = [q for s in ju.SHAPES for q in ju.partial_quarters(s[1] * s[2])]
    for wave in (1, 2, 3):
        assert any(c == 0 and w == wave for c, w, _ns in quarters), wave  # in the only chunk
        assert any(c % 2 == 1 and w == wave for c, w, _ns in quarters), wave  # in the second staging buffer
    assert any(c >= 2 and c % 2 == 0 and w > 0 for c, w, _ns in quarters)  # in the first staging buffer after it was reused
    assert any(ns == 0 for s in ju.SHAPES for per_wave in _splits(s) for ns in per_wave)
    # an odd K tail (the zero half of the last k-step) in a wave other than wave 0: in a partly filled quarter and in a full one
    def odd_tail(shapes):  # (wave, ns) of the quarter that holds the last k-step of an odd F
        return [((F // 2 % 128) // 32, ju.fc1_split(F)[-1][(F // 2 % 128) // 32]) for F in (s[1] * s[2] for s in shapes) if F % 2]

    assert odd_tail(ju.OLD_SHAPES) and all(w == 0 for w, _ns in odd_tail(ju.OLD_SHAPES))
    assert any(w > 0 and 0 < ns < 32 for w, ns in odd_tail(ju.SHAPES)) and (3, 32) in odd_tail(ju.SHAPES)
    assert {ju.head_deal(s[3])[0] for s in ju.SHAPES} == {1, 2, 3, 4, 5, 6, 8, 11}
    assert any((5 * s[3] + 1) % 32 == 0 for s in ju.SHAPES)  # a tile filled exactly: the value in row 31
    assert any((5 * s[3]) % 32 == 0 and ju.head_deal(s[3])[0] < 11 for s in ju.SHAPES)  # the value alone in a tile, not the eleventh
    assert len({ju.extra_split(s[3])[0] for s in ju.SHAPES}) >= 15 and any(ju.extra_split(s[3])[0] % 2 for s in ju.SPLIT_SHAPES)
    assert all(s[0] <= 65 for s in ju.SPLIT_SHAPES)
    # the table of joint_policy_util's comment
    table = {s[1] * s[2]: (_splits(s)[-1], ju.head_deal(s[3])[0], ju.extra_split(s[3])[0]) for s in ju.SPLIT_SHAPES}
    assert {F: (HT, XS) for F, (_q, HT, XS) in table.items()} == {64: (1, 6), 81: (2, 18), 144: (3, 48), 196: (4, 63), 255: (5, 66),
                                                                 259: (6, 81), 340: (3, 33), 400: (8, 128), 462: (2, 23), 600: (1, 16)}
    assert [[max(ns, -1) for ns in table[F][0]] for F in sorted(table)] == [
        [32, 0, -1, -1], [32, 9, -1, -1], [32, 32, 8, -1], [32, 32, 32, 2], [32, 32, 32, 32], [2, -1, -1, -1], [32, 10, -1, -1],
        [32, 32, 8, -1], [32, 32, 32, 7], [32, 12, -1, -1]]


def test_a_fault_of_an_upper_quarter_passes_the_old_shapes_and_fails_the_new():
    """The float32 restatement whose fc1 accumulates K in the kernel's order, and two mutants of a partly filled quarter of
    wave 1, 2 or 3, under the logits / value assertions of the GPU parity test: the seven shapes from before cannot see
    either fault, every shape with such a quarter sees both, and the unmutated restatement passes everywhere."""
    upper = [s for s in ju.SHAPES if ju.upper_partial(s)]
    assert len(upper) >= 7 and not set(upper) & set(ju.OLD_SHAPES)
    for shape in ju.SHAPES:
        c = ju.case(shape, False, False)
        assert not ju.parity_fails(c, ju.restate32(c)), shape
        for mutant in ju.SPLIT_MUTANTS:
            fails = ju.parity_fails(c, ju.restate32(c, mutant))
            if shape in upper:
                print(f"joint {shape} split {_splits(shape)[-1]} in chunk {len(_splits(shape)) - 1} {mutant}: {fails}")
                assert fails, (shape, mutant)
            else:
                assert not fails, (shape, mutant, fails)
