"""The mapped act launch on the device (mapf_policy_create_mapped, then the usual mapf_policy_* calls) through the raw C ABI
with every output and state buffer guarded and poisoned (guard_util).

Bitwise: row r of a mapped handle must equal, bit for bit, row r of a shared handle loaded with set set_of_group[r % groups]
and run on the same full inputs and state, noise included -- the launches differ in which rows share a tile, and a row's
arithmetic does not depend on its tile-mates.  For a population that is: the rows of member p's envs equal those of a shared
handle loaded with members[p]."""

import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import policy_util as pu
import population_util as popu
from population_util import DEV, OUTPUTS, STATE, RawPolicy

pytestmark = pytest.mark.gpu

CASES = [(s, r, m) for s in popu.ACT_SHAPES for r in (True, False) for m in (False, True)]
IDS = lambda v: str(v).replace(" ", "")  # noqa: E731


@pytest.mark.parametrize("shape,recurrent,sample", CASES, ids=IDS)
def test_a_members_rows_equal_its_shared_handle_bit_for_bit(shape, recurrent, sample):
    c = popu.act_case(shape, recurrent, sample)
    B, N, P, L, mask = shape
    rows = B * N
    module = c["module"]
    mapped = RawPolicy.of_population(module, rows)
    assert mapped.lib.mapf_policy_param_count(mapped.h_) == P * module.members[0].flat_params().numel()
    shared = [(RawPolicy(m, m.flat_params(), rows, N), popu.member_rows(B, N, P, p)) for p, m in enumerate(module.members)]
    assert sum(mask_.sum() for _s, mask_ in shared) == rows
    popu.chained_against_shared(mapped, shared, c, rows)


def test_a_general_map_through_the_raw_abi():
    """groups = 4, sets = 2, map [1, 0, 0, 1], N = 2: rows 0, 3 (mod 4) read set 1, rows 1, 2 set 0 -- no population's map."""
    B, N, L, mask = 70, 2, 33, True
    c = dict(popu.act_case((B, N, 1, L, mask), True, True))
    nets = [pu.make_module(L, mask, True, seed=s) for s in (31, 32)]
    rows = B * N
    mapped = RawPolicy(nets[0], torch.cat([n.flat_params() for n in nets]), rows, N, "mapped", 4, 2, [1, 0, 0, 1])
    sets = np.array([1, 0, 0, 1])[np.arange(rows) % 4]
    shared = [(RawPolicy(n, n.flat_params(), rows, N), sets == s) for s, n in enumerate(nets)]
    popu.chained_against_shared(mapped, shared, c, rows)


@pytest.mark.parametrize("sample", (False, True), ids=("greedy", "sampled"))
def test_the_identity_map_equals_the_per_agent_handle_on_every_row(sample):
    import dte_util as du

    B, N, L, mask = 35, 5, 11, False
    c = dict(popu.act_case((B, N, 1, L, mask), True, sample))
    module = du.make_per_agent(N, L, mask, True)
    rows = B * N
    mapped = RawPolicy(module, module.flat_params(), rows, N, "mapped", N, N, list(range(N)))
    per_agent = RawPolicy(module, module.flat_params(), rows, N, "per_agent")
    popu.chained_against_shared(mapped, [(per_agent, np.ones(rows, bool))], c, rows)


def _one(sample=True, set_params=True):
    c = popu.act_case((66, 3, 2, 33, True), True, sample)
    B, N, P, L, _ = c["shape"]
    return c, RawPolicy.of_population(c["module"], B * N, set_params=set_params), popu.step_inputs(c, 1)[:3]


def test_null_outputs_and_peek():
    c, pol, (obs, pa, pr) = _one()
    assert pol.act(popu.dev(c["obs"][0], np.float32), mode=1, seed=3) == 0  # a non-trivial state
    torch.cuda.synchronize()
    before = {k: pol.buf[k].array() for k in STATE}
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5) == 0
    torch.cuda.synchronize()
    full = {k: pol.buf[k].check(True, "peek") for k in OUTPUTS}
    for k in before:  # PEEK leaves h, c and draws untouched
        assert pol.buf[k].guards_intact() and popu.same(pol.buf[k].array(), before[k]), k
    pol.poison_outputs()
    assert pol.act(obs, pa, pr, mode=1 | 2, seed=5, outputs=()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(pol.buf["action"].check(True, "action only"), full["action"])
    for k in ("logp", "value", "logits"):
        pol.buf[k].check(False, "pointer not passed")
    pol.close()


def test_refused_arguments_launch_nothing():
    c, pol, (obs, pa, pr) = _one()
    _c, fresh, _ = _one(set_params=False)
    L, lib = pol.L, pol.lib
    for b in list(pol.buf.values()) + list(fresh.buf.values()):
        b.poison()
    torch.cuda.synchronize()
    CFG = L.MAPF_ERR_CONFIG
    assert pol.act(obs, rows=66 * 3 - 3) == CFG  # whole envs, but no whole number of the 6 groups: refused without start flags too
    assert pol.act(obs, rows=4) == CFG and pol.act(obs, rows=0) == CFG
    assert fresh.act(obs) == L.MAPF_ERR_STATE
    for count in (pol.flat.numel() - 1, pol.flat.numel() // 2, pol.flat.numel() + 1):  # one member's vector is not enough
        assert lib.mapf_policy_set_params(pol.h_, popu.p_(pol.flat), count, popu.stream()) == CFG

    def create(n, groups, sets, entries):
        h = C.c_void_p(1)
        cfg = L.MapfPolicyConfig(33, 28, 1, n, 64, 0)
        rc = lib.mapf_policy_create_mapped(C.byref(cfg), groups, sets, None if entries is None else (C.c_int32 * len(entries))(*entries), C.byref(h))
        assert rc != 0 or h.value
        if rc == 0:
            lib.mapf_policy_destroy(h)
        else:
            assert not h.value
        return rc

    assert create(3, 6, 2, [0, 0, 0, 1, 1, 1]) == 0
    assert create(3, 4, 2, [0, 0, 1, 1]) == CFG  # groups no multiple of N
    assert create(3, 0, 1, []) == CFG and create(3, -3, 1, []) == CFG
    assert create(3, 6, 2, [0, 0, 0, 1, 1, 2]) == CFG and create(3, 6, 2, [0, 0, -1, 1, 1, 1]) == CFG  # a map entry out of range
    assert create(3, 6, 0, [0] * 6) == CFG and create(3, 6, 7, [0] * 6) == CFG  # sets out of range
    assert create(3, 6, 2, None) == CFG
    big = L.POLICY_MAX_GROUPS
    assert create(1, big, 1, [0] * big) == 0 and create(1, big + 1, 1, [0] * (big + 1)) == CFG  # groups above the maximum
    torch.cuda.synchronize()
    for b in list(pol.buf.values()) + list(fresh.buf.values()):
        b.check(False, "refused call")
    pol.zero_state()
    assert pol.act(obs, rows=60) == 0  # a whole number of units is accepted
    torch.cuda.synchronize()
    assert pol.buf["h"].guards_intact() and pol.buf["logits"].guards_intact()
    pol.close(), fresh.close()


def test_device_policy_takes_a_population_and_a_checkpoint_of_that_kind(tmp_path):
    from dl_reference_models_amd.policy import DevicePolicy

    c = popu.act_case((66, 3, 2, 33, True), True, False)
    B, N, P, L, _ = c["shape"]
    module = c["module"]
    path = tmp_path / "pop.pt"
    module.save(path)
    obs, pa, pr = popu.step_inputs(c, 1)[:3]
    outs = []
    for source in (module, str(path)):
        pol = DevicePolicy(source, B * N, N, DEV)
        assert pol.population and not pol.per_agent
        outs.append({k: v.clone() for k, v in pol.act(obs, pa, pr).items()})
    for p, member in enumerate(module.members):
        want = DevicePolicy(member, B * N, N, DEV).act(obs, pa, pr)
        rows = torch.from_numpy(popu.member_rows(B, N, P, p)).to(DEV)
        for k in ("action", "logp", "value", "logits"):
            for out in outs:
                assert torch.equal(out[k][rows].view(torch.uint8), want[k][rows].view(torch.uint8)), (p, k)
    with pytest.raises(ValueError, match="multiple of 6"):
        DevicePolicy(module, B * N - N, N, DEV)
    with pytest.raises(ValueError, match="agents per env"):
        DevicePolicy(module, B * N, 2, DEV)


def _first_call_capture():
    """The mapped act captured as the very first calls of a process, replayed after set_params with other weights (run as a
    script, see below): the replay computes with the new weights, bit for bit what the shared handles of the new members
    give."""
    c = popu.act_case((66, 3, 2, 33, True), True, True)
    B, N, P, L, mask = c["shape"]
    rows = B * N
    module = c["module"]
    pol = RawPolicy.of_population(module, rows)
    obs, pa, pr = (popu.dev(c[k][0], dt) for k, dt in (("obs", np.float32), ("prev_action", np.int8), ("prev_reward", np.float32)))
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert pol.act(obs, pa, pr, mode=1, seed=c["seed"]) == 0  # the handle's first act ever
    other = popu.make_population(P, N, L, mask, True, seed=3)
    first = None
    for i, mod in enumerate((module, other)):
        pol.set_params(mod.flat_params().to(DEV))
        pol.zero_state()
        pol.poison_outputs()
        g.replay()
        torch.cuda.synchronize()
        got = popu.checked(pol, True, True, f"replay {i}")
        for p, member in enumerate(mod.members):
            sh = RawPolicy(member, member.flat_params(), rows, N)
            assert sh.act(obs, pa, pr, mode=1, seed=c["seed"]) == 0
            torch.cuda.synchronize()
            want, mask_ = popu.checked(sh, True, True, f"shared {i} {p}"), popu.member_rows(B, N, P, p)
            for k, v in want.items():
                assert popu.same(got[k][mask_], v[mask_]), (i, p, k)
            sh.close()
        if first is None:
            first = got
    assert not popu.same(first["logits"], got["logits"])
    print("first-call capture ok")


def test_graph_capture_from_the_very_first_act():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "first-call capture ok" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _first_call_capture()
