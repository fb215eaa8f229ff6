"""The windowed prioritised planner on the device (mapf_plan_windowed) against the bit-row restatement of its rule
(windowed_util), element for element, consistent and inconsistent envs alike; its windows executed by the engine's own step
in lifelong mode; its write contract on guarded, poisoned buffers; then the layers above: the tensor API, two calls in
flight, graph capture from the first call, the evaluation policy, the dict facade, the script and the checking build."""

import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

import eval_util as eu
import prioritized_util as pq
import windowed_util as wu
from guard_util import GuardedBuffer, device_bytes, guard_bytes_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOOP_WINDOW, LOOP_EVERY, LOOP_STEPS = 8, 4, 64  # the closed loop of tests/test_windowed_host.py
# 4 x 64 x 64 agents at the longest window: groups of 4 lanes, 16 to a wavefront, but the regions of only 15 envs fit a
# workgroup's LDS (4 288 bytes each with the occupancy as bit rows; as cells it would be 6), so the last group of every
# wavefront plans nothing and env 15 is the second workgroup's first
LDS_CAPPED_SHAPE, LDS_CAPPED_B = ("random", 4, 64, 64, 0.0, 0), 33
LDS_MAX_SHAPE = pq.SHAPES[5]  # 64 x 64 x 64: at window 64 the largest LDS region there is


def _vec(cfg):
    from dl_reference_models_amd.vec_env import VecReferenceModel

    return VecReferenceModel(dict({"device": DEV}, **cfg))


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _sync():
    torch.cuda.synchronize()


def _poll(eng):
    env, agent, value = C.c_int32(-1), C.c_int32(-1), C.c_int32(0)
    rc = eng._lib.mapf_poll_error(eng._h, eng._stream(), C.byref(env), C.byref(agent), C.byref(value))
    return rc, env.value, agent.value, value.value


def _engine(shape, B=None, **over):
    """A handle on the shape's instances, positions and goals set through set_state."""
    kind, H, W, N, density, _T = shape
    B = pq.batch_of(H) if B is None else B
    grids, pos, goals = pq.instances(kind, H, W, N, density, B)
    eng = _vec(dict({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 1, "steps_per_episode": 100,
                     "seeds": list(range(B))}, **over))
    eng.reset()
    eng.set_state(positions=np.array(pos), goals=np.array(goals), clear_episode=True)
    return eng, B


def _restated(shape, w, B):
    kind, H, W, N, density, _T = shape
    return wu.restated(kind, H, W, N, density, w, B)[:3]


def _assert_equal(got, want, what):
    for name, g, w in zip(("remaining", "arrival", "plan"), got[::-1], want[::-1]):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape, (what, name, g.shape, w.shape)
        bad = np.argwhere(g != w)
        assert bad.size == 0, f"{what}: {len(bad)} elements of {name} differ, first at {bad[0].tolist()}: " \
                              f"{g[tuple(bad[0])]} != {w[tuple(bad[0])]}"


def _guarded(B, w, N):
    return (GuardedBuffer((B, w, N), np.int8, DEV, guard_bytes_for(w * N), name="plan"),
            GuardedBuffer((B, N), np.int32, DEV, guard_bytes_for(4 * N), name="arrival"),
            GuardedBuffer((B, N), np.int32, DEV, guard_bytes_for(4 * N), name="remaining"))


def _call(eng, w, mask_ptr, bufs):
    return eng._lib.mapf_plan_windowed(eng._h, w, mask_ptr, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, eng._stream())


def _check(bufs, written, what):
    return tuple(b.check(written, what) for b in bufs)


def _poison(bufs):
    for b in bufs:
        b.poison()


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", [1, 16])
@pytest.mark.parametrize("shape", pq.SHAPES, ids=pq.SHAPE_IDS)
def test_parity_with_the_restatement(shape, w):
    eng, B = _engine(shape)
    want = _restated(shape, w, B)
    got = eng.plan_windowed(w)
    assert got[0].dtype == torch.int8 and tuple(got[0].shape) == want[0].shape and got[0].device == eng.device
    assert all(t.dtype == torch.int32 and tuple(t.shape) == (B, shape[3]) for t in got[1:])
    _assert_equal([t.cpu().numpy() for t in got], want, f"plan_windowed({w})")
    assert _poll(eng)[0] == 0
    eng.close()


def test_parity_at_the_lds_maximum():
    """64 x 64 x 64 agents at window 64: one env per workgroup, 41 728 bytes of LDS (the occupancy as cells: as bit rows
    it would not fit)."""
    eng, B = _engine(LDS_MAX_SHAPE, B=3)
    assert eng.max_window == 64
    bufs = _guarded(B, 64, 64)
    eng._check(_call(eng, 64, None, bufs))
    _sync()
    _assert_equal(_check(bufs, True, "LDS maximum"), _restated(LDS_MAX_SHAPE, 64, B), "window 64 at 64 x 64 x 64")
    assert _poll(eng)[0] == 0
    eng.close()


def test_parity_where_the_lds_limit_leaves_groups_of_the_wavefront_idle():
    shape, B = LDS_CAPPED_SHAPE, LDS_CAPPED_B
    eng, _ = _engine(shape, B=B)
    bufs = _guarded(B, 64, 64)
    eng._check(_call(eng, 64, None, bufs))
    _sync()
    _assert_equal(_check(bufs, True, "capped"), _restated(shape, 64, B), "LDS-capped workgroups")
    # one env of the second workgroup alone
    _poison(bufs)
    mask = np.zeros(B, np.uint8)
    mask[16] = 1
    eng._check(_call(eng, 64, _ptr(device_bytes(eng, mask, np.uint8)), bufs))
    _sync()
    got = _check(bufs, (mask != 0)[:, None], "capped, one env")
    _assert_equal([g[16] for g in got], [x[16] for x in _restated(shape, 64, B)], "LDS-capped, env 16 alone")
    assert _poll(eng)[0] == 0
    eng.close()


@pytest.mark.parametrize("case", wu.HAND_CASES, ids=lambda c: c["name"])
def test_hand_cases(case):
    N = len(case["positions"])
    grid = case["grid"]
    if int((grid == 0).sum()) < 2 * N:
        # the engine refuses a grid with fewer than 2 N free cells (starts and goals of a reset): a wall row and a free row
        # below the case's grid give it the cells; nothing of the case reaches them, so the rule decides the same
        W = grid.shape[1]
        grid = np.concatenate([grid, np.ones((1, W), np.uint8), np.zeros((1, W), np.uint8)])
        want = wu.plan_bit_rows(grid, case["positions"], case["goals"], case["w"])
        assert want[0].T.tolist() == case["plan"] and want[1].tolist() == case["arrival"] and want[2].tolist() == case["remaining"]
    eng = _vec({"grid": grid, "num_envs": 1, "num_agents": N, "sensor_range": 1, "seed": 1})
    eng.reset()
    eng.set_state(positions=case["positions"][None], goals=case["goals"][None], clear_episode=True)
    plan, arrival, remaining = (t.cpu().numpy() for t in eng.plan_windowed(case["w"]))
    assert plan[0].T.tolist() == case["plan"]
    assert arrival[0].tolist() == case["arrival"]
    assert remaining[0].tolist() == case["remaining"]
    assert _poll(eng)[0] == 0
    eng.close()


# ---- 2. closed loop, lifelong handle --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pq.CLOSED_LOOP_SHAPES, ids=[pq.SHAPE_IDS[pq.SHAPES.index(s)] for s in pq.CLOSED_LOOP_SHAPES])
def test_closed_loop_the_engine_executes_consistent_windows_in_lifelong_mode(shape):
    kind, H, W, N, density, _T = shape
    B = pq.batch_of(H)
    grids, _pos, _goals = pq.instances(kind, H, W, N, density, B)
    eng = _vec({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 1, "lifelong_mapf": True,
                "steps_per_episode": LOOP_STEPS + 8, "seeds": list(range(B))})
    eng.reset()
    windows = consistent_windows = 0
    goals_reached = np.zeros(B)
    for t in range(LOOP_STEPS):
        k = t % LOOP_EVERY
        if k == 0:  # replan from the engine's own state; the restatement on that state says what to expect
            st = eng.get_state()
            want = wu.plan_batch(wu.plan_bit_rows, grids, st["positions"], st["goals"], LOOP_WINDOW)
            plan, arrival, remaining = eng.plan_windowed(LOOP_WINDOW)
            _assert_equal([x.cpu().numpy() for x in (plan, arrival, remaining)], want[:3], f"step {t}")
            cells = want[3]
            consistent = wu.costs(want[1], want[2])[0]
            windows += B
            consistent_windows += int(consistent.sum())
        out = eng.step(plan[:, k].contiguous(), auto_reset=False)
        info = out["info_all"].cpu().numpy()
        assert not out["terminated"].any() and not out["truncated"].any()
        pos = eng.get_state()["positions"]
        for b in np.flatnonzero(consistent):
            assert info[b, 2] == 0, f"env {b}, step {t}: {info[b, 2]} failed moves"  # blocking_count_step
            assert np.array_equal(pos[b], cells[b, k + 1]), f"env {b}, step {t}"
        goals_reached = info[:, 1]  # goals_reached_total
    assert 2 * consistent_windows >= windows, f"only {consistent_windows} of {windows} windows consistent"
    assert goals_reached.sum() >= B, f"{goals_reached.sum()} goals reached in {B} envs"
    assert _poll(eng)[0] == 0
    eng.close()


# ---- 3. write contract ---------------------------------------------------------------------------------------------------
CONTRACT_SHAPE = pq.SHAPES[2]  # 12 x 12 x 8: groups of 16 lanes, four envs to a wavefront


@pytest.fixture(scope="module")
def contract_engine():
    eng, B = _engine(CONTRACT_SHAPE)
    yield eng, B
    eng.close()


def test_write_contract_masked_envs_keep_the_poison(contract_engine):
    shape, N, w = CONTRACT_SHAPE, CONTRACT_SHAPE[3], 16
    eng, B = contract_engine
    want = _restated(shape, w, B)
    bufs = _guarded(B, w, N)
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    eng._check(_call(eng, w, _ptr(device_bytes(eng, mask, np.uint8)), bufs))
    _sync()
    keep = mask != 0
    got = (bufs[0].check(keep[:, None, None], "masked"), bufs[1].check(keep[:, None], "masked"), bufs[2].check(keep[:, None], "masked"))
    _assert_equal([g[keep] for g in got], [x[keep] for x in want], "masked-in envs")
    # NULL mask: every env
    _poison(bufs)
    eng._check(_call(eng, w, None, bufs))
    _sync()
    _assert_equal(_check(bufs, True, "all"), want, "mask NULL")
    # an all-zero mask writes nothing: every workgroup leaves before the agent loop
    _poison(bufs)
    eng._check(_call(eng, w, _ptr(device_bytes(eng, np.zeros(B, np.uint8), np.uint8)), bufs))
    _sync()
    _check(bufs, False, "mask all zero")
    # exactly one env of a wavefront of four
    _poison(bufs)
    one = np.zeros(B, np.uint8)
    one[5] = 1
    eng._check(_call(eng, w, _ptr(device_bytes(eng, one, np.uint8)), bufs))
    _sync()
    keep = one != 0
    got = (bufs[0].check(keep[:, None, None], "one env"), bufs[1].check(keep[:, None], "one env"), bufs[2].check(keep[:, None], "one env"))
    _assert_equal([g[5] for g in got], [x[5] for x in want], "env 5 alone")
    assert _poll(eng)[0] == 0


@pytest.mark.parametrize("w", [1, 64])
def test_write_contract_at_the_ends_of_the_window_range(contract_engine, w):
    shape, N = CONTRACT_SHAPE, CONTRACT_SHAPE[3]
    eng, B = contract_engine
    bufs = _guarded(B, w, N)
    eng._check(_call(eng, w, None, bufs))
    _sync()
    _assert_equal(_check(bufs, True, f"window {w}"), _restated(shape, w, B), f"window {w}")
    assert _poll(eng)[0] == 0


# ---- 4. no side effects, no hidden state ------------------------------------------------------------------------------------
def _slots(eng):
    B, N = eng.num_envs, eng.num_agents
    slots, stage, vis = np.zeros(B * N, np.uint32), np.zeros(B * (4 * N + 4), np.uint32), np.zeros(B * 6, np.uint64)
    eng._check(eng._lib.mapf_debug_slots(eng._h, slots.ctypes.data_as(C.c_void_p), stage.ctypes.data_as(C.c_void_p),
                                         vis.ctypes.data_as(C.c_void_p)))
    return slots, stage, vis


def test_planning_changes_nothing():
    import plan_util as pu

    B, N = 40, 8
    grids = pu.random_grids(16, 16, B, pu.DENSITY_CONNECTED, 2 * N)
    cfg = {"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": 20,
           "lifelong_mapf": True, "seeds": list(range(B))}
    a, b = _vec(cfg), _vec(cfg)
    rng = np.random.default_rng(7)
    for _ in range(15):
        acts = torch.from_numpy(rng.integers(0, 5, size=(B, N)).astype(np.int8)).to(a.device)
        a.step(acts)
        b.step(acts)
    mask = torch.from_numpy((np.arange(B) % 2).astype(np.uint8)).to(a.device)
    calls = {"plan_windowed": lambda: a.plan_windowed(16), "plan_windowed(mask)": lambda: a.plan_windowed(33, mask=mask)}
    for name, call in calls.items():
        before, slots_before = a.get_state(), _slots(a)
        call()
        _sync()
        after, slots_after = a.get_state(), _slots(a)
        for k in before:  # agents, counters, generator words
            assert np.array_equal(before[k], after[k]), (name, k)
        for x, y in zip(slots_before, slots_after):
            assert np.array_equal(x, y), name
    # a step trace with the calls interleaved equals the trace without them
    names = list(calls)
    for t in range(24):
        acts = torch.from_numpy(rng.integers(0, 5, size=(B, N)).astype(np.int8)).to(a.device)
        calls[names[t % len(names)]]()
        oa = {k: v.clone() for k, v in a.step(acts).items() if v is not None}
        ob = b.step(acts)
        for k, v in oa.items():
            assert torch.equal(v, ob[k]), (t, k)
    sa, sb = a.get_state(), b.get_state()
    for k in sa:
        assert np.array_equal(sa[k], sb[k]), k
    assert _poll(a)[0] == 0
    a.close()
    b.close()


def test_two_calls_in_flight_on_two_streams():
    """Different windows on two streams, no event between them: nothing is shared, so both equal the restatement."""
    eng, B = _engine(LDS_MAX_SHAPE, B=3)
    s1, s2 = torch.cuda.Stream(eng.device), torch.cuda.Stream(eng.device)
    _sync()
    with torch.cuda.stream(s1):
        got64 = eng.plan_windowed(64)
    with torch.cuda.stream(s2):
        got16 = eng.plan_windowed(16)
    _sync()
    _assert_equal([t.cpu().numpy() for t in got64], _restated(LDS_MAX_SHAPE, 64, B), "window 64 on stream 1")
    _assert_equal([t.cpu().numpy() for t in got16], _restated(LDS_MAX_SHAPE, 16, B), "window 16 on stream 2")
    assert _poll(eng)[0] == 0
    eng.close()


# ---- 5. bad arguments ------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing(contract_engine):
    from dl_reference_models_amd import _lib as L

    N = CONTRACT_SHAPE[3]
    eng, B = contract_engine
    assert eng.max_window == 64 == L.PLAN_MAX_WINDOW
    assert eng._lib.mapf_plan_max_window(None) == 0
    bufs = _guarded(B, 65, N)
    for w in (0, -1, 65):
        assert _call(eng, w, None, bufs) == L.MAPF_ERR_CONFIG
        with pytest.raises(ValueError):
            eng.plan_windowed(w)
    s = eng._stream()
    assert eng._lib.mapf_plan_windowed(eng._h, 8, None, None, bufs[1].ptr, bufs[2].ptr, s) == L.MAPF_ERR_CONFIG
    assert eng._lib.mapf_plan_windowed(eng._h, 8, None, bufs[0].ptr, None, bufs[2].ptr, s) == L.MAPF_ERR_CONFIG
    assert eng._lib.mapf_plan_windowed(eng._h, 8, None, bufs[0].ptr, bufs[1].ptr, None, s) == L.MAPF_ERR_CONFIG
    assert eng._lib.mapf_plan_windowed(None, 8, None, bufs[0].ptr, bufs[1].ptr, bufs[2].ptr, s) == L.MAPF_ERR_CONFIG
    _sync()
    _check(bufs, False, "refused: nothing launched")
    i8, i32 = torch.int8, torch.int32
    good = (torch.empty((B, 8, N), dtype=i8, device=eng.device), torch.empty((B, N), dtype=i32, device=eng.device),
            torch.empty((B, N), dtype=i32, device=eng.device))
    eng.plan_windowed(8, out=good)
    bad_outs = [(torch.empty((B, 9, N), dtype=i8, device=eng.device), good[1], good[2]),     # shape
                (good[0].to(torch.int16), good[1], good[2]),                                # dtype
                (good[0], good[1], torch.empty((B, N), dtype=torch.int64, device=eng.device)),
                (good[0], good[1][:, :-1], good[2]),                                        # shape
                (good[0].cpu(), good[1], good[2]),                                          # host tensor
                good[:2]]                                                                   # not a triple
    for out in bad_outs:
        with pytest.raises(ValueError):
            eng.plan_windowed(8, out=out)
    with pytest.raises(ValueError):
        eng.plan_windowed(8, mask=torch.ones((B + 1,), dtype=torch.uint8))
    assert _poll(eng)[0] == 0


# ---- 6. capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_as_the_first_planner_call_of_the_handle():
    shape = CONTRACT_SHAPE
    N, w, K = shape[3], 16, 4
    eager, B = _engine(shape, lifelong_mapf=True)
    cap, _ = _engine(shape, lifelong_mapf=True)
    want = []
    for _ in range(K):
        plan, arrival, remaining = eager.plan_windowed(w)
        out = eager.step(plan[:, 0].contiguous())
        want.append((plan.cpu().numpy(), arrival.cpu().numpy(), remaining.cpu().numpy(), out["rewards"].cpu().numpy(),
                     eager.get_state()["positions"]))
    bufs = (torch.zeros((B, w, N), dtype=torch.int8, device=cap.device), torch.zeros((B, N), dtype=torch.int32, device=cap.device),
            torch.zeros((B, N), dtype=torch.int32, device=cap.device))
    a_buf = torch.zeros((B, N), dtype=torch.int8, device=cap.device)
    s = torch.cuda.Stream(cap.device)
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):  # one linear chain; no planner call of this handle was made before
        cap.plan_windowed(w, out=bufs)
        a_buf.copy_(bufs[0][:, 0])
        cap.step(a_buf)
    torch.cuda.synchronize()
    for k in range(K):
        g.replay()
        torch.cuda.synchronize()
        for i in range(3):
            assert np.array_equal(bufs[i].cpu().numpy(), want[k][i]), (k, i)
        assert np.array_equal(cap._rewards.cpu().numpy(), want[k][3]), k
        assert np.array_equal(cap.get_state()["positions"], want[k][4]), k
    assert _poll(cap)[0] == 0
    eager.close()
    cap.close()


# ---- 7. policy -------------------------------------------------------------------------------------------------------------
def test_evaluate_with_the_windowed_policy_on_the_lifelong_fixture():
    from dl_reference_models_amd import evaluation as evm

    fx = eu.load_eval_fixture("ge_eval_2_1_n4_lifelong")
    E = fx["E"]
    assert fx["config"].get("lifelong_mapf")
    env = _vec(eu.engine_config(fx))
    res, heat = evm.evaluate(env, "windowed", E, poll_every=8)
    env.close()
    B = len(fx["seeds"])
    assert len(res["env"]) == B * E
    # the same run with the actions kept: a host replay through the oracle gives the same records
    env = _vec(eu.engine_config(fx))
    inner, taken = evm.windowed_policy(env), []

    def policy(obs, first):
        acts = inner(obs, first)
        taken.append(acts.clone())
        return acts

    res2, heat2 = evm.evaluate(env, policy, E, poll_every=8)
    assert evm.results_table(res, lifelong=True) == evm.results_table(res2, lifelong=True) and np.array_equal(heat, heat2)
    actions = torch.stack(taken).cpu().numpy()
    want = eu.run_oracle_eval(fx["grids"], fx["config"], E, seeds=[int(s) for s in fx["seeds"]], actions=actions)
    got = eu.dense_from_results(res2, np.zeros_like(want["heat"]), E)
    for k in eu.RECORD_KEYS:
        if k != "heat":
            assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(heat2, want["heat"].sum(axis=0))
    assert evm.summary(res2, lifelong=True)["average goals_reached_total"] > 0
    # with replanning at arrivals, and in finite mode
    res3, _ = evm.evaluate(env, evm.windowed_policy(env, window=8, replan_every=4, replan_on_arrival=True), 1)
    assert len(res3["env"]) == B
    env.close()
    cfg = eu.engine_config(fx)
    cfg["lifelong_mapf"] = False
    finite = _vec(cfg)
    res4, _ = evm.evaluate(finite, "windowed", 1)
    assert len(res4["env"]) == B
    finite.close()


# ---- 8. facade, script, single-agent handle, checking build -------------------------------------------------------------------
def test_facade_dicts_equal_row_zero_of_the_tensor_call():
    from dl_reference_models_amd.reference_model_multi_agent import ReferenceModel

    env = ReferenceModel({"env_name": "ReferenceModel-2-1", "num_agents": 4, "seed": 5, "sensor_range": 2, "lifelong_mapf": True})
    env.reset()
    acts, arrival, remaining = env.plan_windowed(window=12)
    tens = [t[0].cpu().numpy() for t in env._engine.plan_windowed(12)]
    assert list(acts) == list(arrival) == list(remaining) == [f"agent_{i}" for i in range(4)]
    for i in range(4):
        assert acts[f"agent_{i}"] == tens[0][:, i].tolist() and all(type(v) is int for v in acts[f"agent_{i}"])
        assert arrival[f"agent_{i}"] == int(tens[1][i]) and type(arrival[f"agent_{i}"]) is int
        assert remaining[f"agent_{i}"] == int(tens[2][i]) and type(remaining[f"agent_{i}"]) is int
    st = env._engine.get_state()
    want = wu.plan_bit_rows(np.asarray(env.grid, np.uint8), st["positions"][0], st["goals"][0], 12)
    _assert_equal(tens, want[:3], "facade")
    assert len(env.plan_windowed()[0]["agent_0"]) == 16  # the default window
    env.close()


def test_script_runs_the_windowed_policy(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("eval_cli", os.path.join(ROOT, "scripts", "evaluate_multi_agent_env.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--policy", "WINDOWED", "--lifelong", "--window", "8", "--replan-every", "4", "--num-envs", "8",
                    "--episodes", "1", "--steps-per-episode", "40", "--output-dir", str(tmp_path / "WINDOWED")])
    assert len(out["table"]) == 8
    assert os.path.basename(out["csv"]).startswith("ReferenceModel-2-1_WINDOWED_4_agents_")
    assert out["summary"]["average goals_reached_total"] > 0
    assert "Success rate:" in capsys.readouterr().out


def test_single_agent_handle():
    import plan_util as pu
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    B, N, H, W, w = 7, 3, 12, 12, 16
    grids = pu.random_grids(H, W, B, pu.DENSITY_CONNECTED, 2 * N)
    eng = VecSingleAgentReferenceModel({"grid": np.array(grids), "num_envs": B, "num_agents": N, "seeds": list(range(B)),
                                        "device": DEV, "steps_per_episode": 20})
    eng.reset()
    st = eng.get_state()
    want = wu.plan_batch(wu.plan_bit_rows, grids, st["positions"], st["goals"], w)
    _assert_equal([t.cpu().numpy() for t in eng.plan_windowed(w)], want[:3], "single-agent handle")
    assert _poll(eng)[0] == 0
    eng.close()


CHECK_CAPPED_SHAPE, CHECK_CAPPED_B = ("random", 4, 16, 16, 0.0, 0), 33  # 15 of 16 groups per workgroup at window 64


@pytest.mark.parametrize("w", [1, 16, 64])
def test_checking_build_runs_the_parity_shapes_clean(monkeypatch, w):
    """-DMAPF_CHECK range-checks the LDS history and slot indices and the walk's predecessor (sites 18 - 20).  The checking
    build holds the step kernels of up to 16 lanes per env, i.e. up to 16 agents, so every parity shape but 64 x 64 x 64
    runs on it (33 x 12 with its 64-lane planner groups included), and an LDS-capped shape of 16 agents."""
    monkeypatch.setenv("MAPF_CHECK_BUILD", "1")
    from dl_reference_models_amd import _lib as L

    shapes = [s for s in pq.SHAPES if s[3] <= 16] + [CHECK_CAPPED_SHAPE]
    assert len(shapes) == len(pq.SHAPES) and pq.SHAPES[4] in shapes
    for shape in shapes:
        eng, B = _engine(shape, B=CHECK_CAPPED_B if shape is CHECK_CAPPED_SHAPE else None)
        assert eng._lib is L.load() and L.library_path().endswith("libmapfstep_check.so")
        got = eng.plan_windowed(w)
        rc, env, site, value = _poll(eng)
        assert rc == 0, f"{shape[:4]}: site {site}, env {env}, value {value}"  # no index left its region
        _assert_equal([t.cpu().numpy() for t in got], _restated(shape, w, B), f"checking build {shape[:4]}")
        eng.close()
