"""Per-group hyperparameters in the PPO objective kernel (mapf_ppo_loss_hp through the raw C ABI) on guarded, poisoned
buffers: hp rows equal to the scalars against the hp = NULL call and against mapf_ppo_loss, distinct rows per group against
the groups = 1 scalar call on every group's gathered rows (all bitwise), NULL outputs, a captured graph that follows an hp
overwritten on the device, and the float64 rule of ppo_loss_util with its quantities, kinds and margins as they are.

Shapes: T = 5 and T = 33 (a chunk edge); rows = groups x 33 (a full tile and a one-row tile per group) with groups 1, 2
and 6; heads 1 (dlogits from the first pass) and 3 (the second pass); with and without kl_coeff."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ppo_loss_util as plu
import population_util as popu
from population_util import PPO_OUTPUTS, RawPPO, same

pytestmark = pytest.mark.gpu

SHAPES = [(T, 33 * G, heads, G) for T in (5, 33) for G in (1, 2, 6) for heads in (1, 3)]
IDS = lambda s: "T%d_rows%d_heads%d_groups%d" % s  # noqa: E731


def _inputs(shape, kl, kind="plain"):
    inp = plu.make_inputs(*shape, kind)
    return inp if kl else dict(inp, kl_coeff=None, old_logits=None)


def _scalar_rows(G):
    return np.tile(np.array([[plu.SETTINGS[k] for k in popu.SCALARS]], np.float32), (G, 1))


@pytest.mark.parametrize("kl", (True, False), ids=("kl", "no_kl"))
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_rows_equal_to_the_scalars_give_the_scalar_call(shape, kl):
    inp, G = _inputs(shape, kl), shape[3]
    raw = RawPPO(inp, plu.SETTINGS, G, _scalar_rows(G))
    with_hp, null_hp, parent = raw.run(), raw.run(hp=None), raw.run("mapf_ppo_loss")
    for k in PPO_OUTPUTS:
        assert same(with_hp[k], null_hp[k]) and same(null_hp[k], parent[k]), k
        assert np.isfinite(with_hp[k]).all(), k
    if not kl:
        assert not with_hp["kl"].any() and not with_hp["partials"][:, 3].any()
    # with hp the scalars are not read: any other valid-or-not values change nothing
    junk = RawPPO(inp, {"clip": 7.0, "vf_clip": -1.0, "vf_coeff": float("nan"), "ent_coeff": float("inf")}, G, _scalar_rows(G))
    again = junk.run()
    for k in PPO_OUTPUTS:
        assert same(again[k], with_hp[k]), k
    assert junk.call(hp=None) == junk.L.MAPF_ERR_CONFIG  # (and without hp they are checked as ever)
    assert raw.buf["hp"].guard_damage() is None and same(raw.buf["hp"].array(), _scalar_rows(G))  # read, never written


@pytest.mark.parametrize("kl", (True, False), ids=("kl", "no_kl"))
@pytest.mark.parametrize("shape", [s for s in SHAPES if s[3] > 1], ids=IDS)
def test_distinct_rows_give_every_group_its_own_scalar_call(shape, kl):
    inp, G = _inputs(shape, kl), shape[3]
    hp = popu.hp_rows(G, plu.SETTINGS)
    whole = RawPPO(inp, plu.SETTINGS, G, hp).run()
    tiles = whole["partials"].shape[0] // G
    differs = 0
    for g in range(G):
        sub = {k: (v if v is None else v[g:g + 1] if k == "kl_coeff" else np.ascontiguousarray(v[:, g::G])) for k, v in inp.items()}
        scalars = {k: float(hp[g, i]) for i, k in enumerate(popu.SCALARS)}
        alone = RawPPO(sub, scalars, 1).run("mapf_ppo_loss")
        for k in ("logp", "kl", "dlogits", "dvalues"):
            assert same(whole[k][:, g::G], alone[k]), (g, k)
        assert same(whole["partials"][g * tiles:(g + 1) * tiles], alone["partials"]), g
        if g:  # and the group's own values were at work: with group 0's the gradients are others
            base = RawPPO(sub, {k: float(hp[0, i]) for i, k in enumerate(popu.SCALARS)}, 1).run("mapf_ppo_loss")
            differs += not same(base["dlogits"], alone["dlogits"]) and not same(base["dvalues"], alone["dvalues"])
    assert differs == G - 1


def test_null_outputs_are_honoured():
    for shape in ((33, 66, 3, 2), (5, 66, 1, 2)):
        inp = _inputs(shape, True)
        raw = RawPPO(inp, plu.SETTINGS, 2, popu.hp_rows(2, plu.SETTINGS))
        full = raw.run()
        for null in [{k: None} for k in PPO_OUTPUTS] + [{k: None for k in PPO_OUTPUTS}]:
            got = raw.run(**null)  # (checks every buffer not passed as untouched, guards included)
            for k, v in got.items():
                assert same(v, full[k]), (null, k)
        for k in tuple(popu.PPO_INPUTS) + ("kl_coeff", "hp"):  # inputs are read, never written
            assert raw.buf[k].guard_damage() is None, k


def _case_with(shape, kind, hp):
    """ppo_loss_util's oracle and fp32 statement for a case whose every group has its own hyperparameters: the groups = 1
    quantities of each group's gathered rows with its own values, put back in place."""
    T, R, heads, G = shape
    inp = plu.make_inputs(*shape, kind)
    shapes = {k: (inp["logits"] if k == "dlogits" else inp["values"]).shape for k in plu.ELEMENTWISE}
    want, got32 = ({k: np.zeros(s) for k, s in shapes.items()} for _ in range(2))
    parts_w, parts_32 = [], []
    for g in range(G):
        sub = {k: (v[g:g + 1] if k == "kl_coeff" else np.ascontiguousarray(v[:, g::G])) for k, v in inp.items()}
        hpg = {k: float(hp[g, i]) for i, k in enumerate(popu.SCALARS)}
        w, s = plu.oracle(sub, hpg, 1), plu.torch_path32(sub, hpg, 1)
        # no element so near a boundary of ITS group that fp32 and float64 could stand on different sides of it (the bands
        # ppo_loss_util draws its inputs around are those of the scalars' boundaries, which are group 0's here)
        finite = np.isfinite(np.log(w["ratio"]))
        gap_ratio = min(float(np.abs(np.log(w["ratio"][finite]) - np.log1p(sg * hpg["clip"])).min()) for sg in (1, -1))
        assert gap_ratio >= 1e-5 and float(np.abs(w["err"] - hpg["vf_clip"]).min()) >= 1e-5, (g, gap_ratio)
        parts_w.append(plu._partials(plu.oracle, sub, hpg, 1)), parts_32.append(plu._partials(plu.torch_path32, sub, hpg, 1))
        for k in plu.ELEMENTWISE:
            want[k][:, g::G], got32[k][:, g::G] = w[k], s[k]
    want["partials"], got32["partials"] = np.concatenate(parts_w), np.concatenate(parts_32)
    return inp, want, plu.deviation(got32, want)


@pytest.mark.parametrize("kind", plu.KINDS)
@pytest.mark.parametrize("shape", ((5, 66, 3, 2), (33, 198, 1, 6)), ids=IDS)
def test_parity_with_the_float64_rule(shape, kind):
    """In units of dev, the deviation of the learner's fp32 torch statement on the CPU from the float64 oracle: the
    quantities, kinds and margins of tests/test_ppo_loss_gpu.py."""
    G = shape[3]
    hp = popu.hp_rows(G, plu.SETTINGS)
    inp, want, dev = _case_with(shape, kind, hp)
    out = RawPPO(inp, plu.SETTINGS, G, hp).run()
    q = {k: out[k].astype(np.float64) for k in plu.ELEMENTWISE}
    q["partials"] = out["partials"][:, :4].astype(np.float64)
    line = []
    for k in plu.QUANTITIES:
        assert np.isfinite(q[k]).all(), k
        err = float(np.abs(q[k] - want[k]).max())
        line.append(f"{k} {err:.3e} / {dev[k]:.3e}" + (f" = {err / dev[k]:.2f}" if dev[k] > 0 else ""))
    print(f"ppo hp parity T={shape[0]} rows={shape[1]} heads={shape[2]} groups={G} {kind}: " + ", ".join(line))
    for k in plu.QUANTITIES:
        assert float(np.abs(q[k] - want[k]).max()) <= plu.MARGINS[k] * dev[k], (k, dev[k])


def test_the_autograd_function_and_the_learner_read_hp():
    """learner._PPOLoss with hp is the call, the sum of the partials and nothing else."""
    from dl_reference_models_amd import learner as ln

    shape = (5, 198, 1, 6)
    inp, G = _inputs(shape, True), 6
    hp = popu.hp_rows(G, plu.SETTINGS)
    out = RawPPO(inp, plu.SETTINGS, G, hp).run()
    t = {k: torch.from_numpy(v).to(popu.DEV) for k, v in inp.items()}
    logits, values = t["logits"].clone().requires_grad_(True), t["values"].clone().requires_grad_(True)
    terms = ln._PPOLoss.apply(logits, values, t["actions"], t["old_logp"], t["adv"], t["targets"], t["old_logits"], t["kl_coeff"],
                              1, G, (0.0, 0.0, 0.0, 0.0), torch.from_numpy(hp).to(popu.DEV))
    dlogits, dvalues = torch.autograd.grad(terms[0].sum(), [logits, values])
    assert same(dlogits.cpu().numpy(), out["dlogits"]) and same(dvalues.cpu().numpy(), out["dvalues"])
    sums = torch.from_numpy(out["partials"]).view(G, -1, 5).sum(1).numpy() * np.float32(G / (shape[0] * shape[1]))
    assert np.allclose(terms[0].detach().cpu().numpy(), sums[:, 4], rtol=1e-5, atol=1e-6)
    for bad in (torch.from_numpy(hp[:5]).to(popu.DEV), torch.from_numpy(hp).double().to(popu.DEV), torch.from_numpy(hp)):
        with pytest.raises(ValueError, match="hp"):
            ln._PPOLoss.apply(logits, values, t["actions"], t["old_logp"], t["adv"], t["targets"], t["old_logits"], t["kl_coeff"], 1, G,
                              (0.0, 0.0, 0.0, 0.0), bad)


def _first_call_capture():
    """One graph captured as the first call of a process, replayed after hp was overwritten on the device with no
    synchronisation in between: it gives the new values' results, bit for bit those of the scalar calls (run as a script)."""
    shape = (5, 66, 3, 2)
    inp, G = _inputs(shape, True), 2
    first, second = popu.hp_rows(G, plu.SETTINGS), popu.hp_rows(G, plu.REFERENCE)[::-1].copy()
    raw = RawPPO(inp, plu.SETTINGS, G, first)
    raw.poison()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert raw.call() == 0
    outs = []
    for i, hp in enumerate((first, second, first)):
        raw.set_hp(hp)  # (a device write on the stream the replay follows)
        raw.poison()
        g.replay()
        torch.cuda.synchronize()
        outs.append(raw.collect(f"replay {i}"))
        for grp in range(G):
            sub = {k: (v[grp:grp + 1] if k == "kl_coeff" else np.ascontiguousarray(v[:, grp::G])) for k, v in inp.items()}
            alone = RawPPO(sub, {k: float(hp[grp, j]) for j, k in enumerate(popu.SCALARS)}, 1).run("mapf_ppo_loss")
            for k in ("logp", "kl", "dlogits", "dvalues"):
                assert same(outs[-1][k][:, grp::G], alone[k]), (i, grp, k)
    assert not same(outs[0]["dlogits"], outs[1]["dlogits"]) and same(outs[0]["dlogits"], outs[2]["dlogits"])
    print("first-call capture ok")


def test_a_captured_graph_follows_hp_without_recapture():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first-call capture ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _first_call_capture()
