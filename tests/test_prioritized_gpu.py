"""The prioritised planner on the device (mapf_plan_prioritized) against the bit-row restatement of its rule
(prioritized_util), element for element, solved and unsolved envs alike; its plans executed by the engine's own step; its
write contract on guarded, poisoned buffers; then the layers above: the tensor API, graph capture, the evaluation policy,
the dict facade and the script."""

import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import prioritized_util as pq
from guard_util import GuardedBuffer, device_bytes, guard_bytes_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


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
    return rc, env.value, value.value


def _engine(shape, B=None, **over):
    """A handle on the shape's instances, positions and goals set through set_state."""
    kind, H, W, N, density, T = shape
    B = pq.batch_of(H) if B is None else B
    grids, pos, goals = pq.instances(kind, H, W, N, density, B)
    eng = _vec(dict({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 1,
                     "steps_per_episode": T + 8, "seeds": list(range(B))}, **over))
    eng.reset()
    eng.set_state(positions=np.array(pos), goals=np.array(goals), clear_episode=True)
    return eng, B


def _restated(shape, B):
    kind, H, W, N, density, T = shape
    return pq.restated(kind, H, W, N, density, T, B)


def _assert_equal(got_plan, got_arr, plan, arrival, what):
    bad = np.argwhere(got_arr != arrival)
    assert bad.size == 0, f"{what}: {len(bad)} arrivals differ, first (env, agent) {bad[0].tolist()}: " \
                          f"{got_arr[tuple(bad[0])]} != {arrival[tuple(bad[0])]}"
    bad = np.argwhere(got_plan != plan)
    assert bad.size == 0, f"{what}: {len(bad)} actions differ, first (env, step, agent) {bad[0].tolist()}: " \
                          f"{got_plan[tuple(bad[0])]} != {plan[tuple(bad[0])]}"


# ---- 1. parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pq.SHAPES, ids=pq.SHAPE_IDS)
def test_parity_with_the_restatement(shape):
    T = shape[5]
    eng, B = _engine(shape)
    plan, arrival, _cells = _restated(shape, B)
    got_plan, got_arr = eng.plan_prioritized(T)
    assert got_plan.dtype == torch.int8 and tuple(got_plan.shape) == plan.shape and got_plan.device == eng.device
    assert got_arr.dtype == torch.int32 and tuple(got_arr.shape) == arrival.shape
    _assert_equal(got_plan.cpu().numpy(), got_arr.cpu().numpy(), plan, arrival, "plan_prioritized")
    assert _poll(eng)[0] == 0
    eng.close()


def test_parity_where_the_lds_limit_leaves_groups_of_the_wavefront_idle():
    """4 x 8 x 8 agents at the longest horizon: groups of 4 lanes, 16 to a wavefront, but the slots of only 15 envs fit a
    workgroup's LDS, so the last group of every wavefront plans nothing and env 15 is the second workgroup's first."""
    shape = ("random", 4, 8, 8, 0.0, 256)
    B = 33
    eng, _ = _engine(shape, B=B)
    assert eng.plan_max_horizon == 256
    plan, arrival, _cells = _restated(shape, B)
    gp, ga = _guarded(B, 256, 8)
    eng._check(eng._lib.mapf_plan_prioritized(eng._h, 256, None, gp.ptr, ga.ptr, eng._stream()))
    _sync()
    _assert_equal(gp.check(True, "capped"), ga.check(True, "capped"), plan, arrival, "LDS-capped workgroups")
    assert _poll(eng)[0] == 0
    eng.close()


@pytest.mark.parametrize("case", pq.HAND_CASES, ids=lambda c: c["name"])
def test_hand_cases(case):
    eng = _vec({"grid": case["grid"], "num_envs": 1, "num_agents": 2, "sensor_range": 1, "seed": 1})
    eng.reset()
    eng.set_state(positions=case["positions"][None], goals=case["goals"][None], clear_episode=True)
    T = case["T"]
    plan, arrival = (t.cpu().numpy() for t in eng.plan_prioritized(T))
    assert arrival[0].tolist() == case["arrival"]
    for j, acts in case["plan"].items():
        assert plan[0, :, j].tolist() == list(acts) + [0] * (T - len(acts)), j
    eng.close()


# ---- 2. closed loop ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", pq.CLOSED_LOOP_SHAPES, ids=[pq.SHAPE_IDS[pq.SHAPES.index(s)] for s in pq.CLOSED_LOOP_SHAPES])
def test_closed_loop_the_engine_executes_solved_plans(shape):
    _kind, _H, _W, N, _density, T = shape
    eng, B = _engine(shape)
    _grids, _pos, goals = pq.instances(*shape[:5], B)
    _plan, arrival, cells = _restated(shape, B)
    solved, _soc, makespan = pq.costs(arrival)
    assert 2 * int(solved.sum()) >= B, f"only {int(solved.sum())} of {B} envs solved"
    plan, got_arr = eng.plan_prioritized(T)
    assert np.array_equal(got_arr.cpu().numpy(), arrival)
    want_done = np.array([pq.first_all_on_goal(cells[b], goals[b]) for b in range(B)])
    done_at = np.full(B, -1)
    for t in range(1, int(makespan.max()) + 1):
        out = eng.step(plan[:, t - 1].contiguous(), auto_reset=False)
        term, info = out["terminated"].cpu().numpy(), out["info_all"].cpu().numpy()
        pos = eng.get_state()["positions"]
        for b in np.flatnonzero(solved):
            if done_at[b] >= 0:  # (the env has ended: it is stepped on only because the batch is)
                continue
            assert info[b, 2] == 0, f"env {b}, step {t}: {info[b, 2]} failed moves"  # blocking_count_step
            assert np.array_equal(pos[b], cells[b, t]), f"env {b}, step {t}"
            if term[b]:
                done_at[b] = t
            assert (done_at[b] == t) == (want_done[b] == t), f"env {b}, step {t}: terminated {term[b]}, expected at {want_done[b]}"
    assert np.array_equal(done_at[solved], want_done[solved])
    assert (want_done[solved] <= np.maximum(makespan[solved], 1)).all()
    assert _poll(eng)[0] == 0
    eng.close()


# ---- 3. write contract ---------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _contract_engine():
    return _engine(pq.SHAPES[2])


def _guarded(B, T, N):
    return (GuardedBuffer((B, T, N), np.int8, DEV, guard_bytes_for(T * N), name="plan"),
            GuardedBuffer((B, N), np.int32, DEV, guard_bytes_for(4 * N), name="arrival"))


def test_write_contract_masked_envs_keep_the_poison():
    shape = pq.SHAPES[2]
    N, T = shape[3], shape[5]
    eng, B = _contract_engine()
    plan, arrival, _cells = _restated(shape, B)
    gp, ga = _guarded(B, T, N)
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)
    mask_d = device_bytes(eng, mask, np.uint8)
    eng._check(eng._lib.mapf_plan_prioritized(eng._h, T, _ptr(mask_d), gp.ptr, ga.ptr, eng._stream()))
    _sync()
    got_plan, got_arr = gp.check(mask != 0, "masked"), ga.check(mask != 0, "masked")
    keep = mask != 0
    _assert_equal(got_plan[keep], got_arr[keep], plan[keep], arrival[keep], "masked-in envs")
    # NULL mask: every env
    gp.poison()
    ga.poison()
    eng._check(eng._lib.mapf_plan_prioritized(eng._h, T, None, gp.ptr, ga.ptr, eng._stream()))
    _sync()
    _assert_equal(gp.check(True, "all"), ga.check(True, "all"), plan, arrival, "mask NULL")
    # an all-zero mask writes nothing
    gp.poison()
    ga.poison()
    zero_d = device_bytes(eng, np.zeros(B, np.uint8), np.uint8)
    eng._check(eng._lib.mapf_plan_prioritized(eng._h, T, _ptr(zero_d), gp.ptr, ga.ptr, eng._stream()))
    _sync()
    gp.check(False, "mask all zero")
    ga.check(False, "mask all zero")
    assert _poll(eng)[0] == 0


@pytest.mark.parametrize("which", ["one", "limit"])
def test_write_contract_at_the_ends_of_the_horizon_range(which):
    shape = pq.SHAPES[2]
    kind, H, W, N, density, _T = shape
    eng, B = _contract_engine()
    T = 1 if which == "one" else eng.plan_max_horizon
    assert eng.plan_max_horizon >= 256
    gp, ga = _guarded(B, T, N)
    eng._check(eng._lib.mapf_plan_prioritized(eng._h, T, None, gp.ptr, ga.ptr, eng._stream()))
    _sync()
    got_plan, got_arr = gp.check(True, f"horizon {T}"), ga.check(True, f"horizon {T}")
    plan, arrival, _cells = pq.restated(kind, H, W, N, density, T, B)
    _assert_equal(got_plan, got_arr, plan, arrival, f"horizon {T}")
    assert _poll(eng)[0] == 0


# ---- 4. no side effects --------------------------------------------------------------------------------------------------
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
           "seeds": list(range(B))}
    a, b = _vec(cfg), _vec(cfg)
    rng = np.random.default_rng(7)
    for _ in range(15):
        acts = torch.from_numpy(rng.integers(0, 5, size=(B, N)).astype(np.int8)).to(a.device)
        a.step(acts)
        b.step(acts)
    mask = torch.from_numpy((np.arange(B) % 2).astype(np.uint8)).to(a.device)
    calls = {"plan_prioritized": lambda: a.plan_prioritized(20), "plan_prioritized(mask)": lambda: a.plan_prioritized(33, mask=mask)}
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


# ---- 5. bad arguments ------------------------------------------------------------------------------------------------------
def test_bad_arguments_launch_nothing():
    from dl_reference_models_amd import _lib as L

    shape = pq.SHAPES[2]
    N = shape[3]
    eng, B = _contract_engine()
    limit = eng.plan_max_horizon
    gp, ga = _guarded(B, limit + 1, N)
    for T in (0, -1, limit + 1):
        assert eng._lib.mapf_plan_prioritized(eng._h, T, None, gp.ptr, ga.ptr, eng._stream()) == L.MAPF_ERR_CONFIG
        with pytest.raises(ValueError):
            eng.plan_prioritized(T)
    assert eng._lib.mapf_plan_prioritized(eng._h, 8, None, None, ga.ptr, eng._stream()) == L.MAPF_ERR_CONFIG
    assert eng._lib.mapf_plan_prioritized(eng._h, 8, None, gp.ptr, None, eng._stream()) == L.MAPF_ERR_CONFIG
    _sync()
    gp.check(False, "refused: nothing launched")
    ga.check(False, "refused: nothing launched")
    good = (torch.empty((B, 8, N), dtype=torch.int8, device=eng.device), torch.empty((B, N), dtype=torch.int32, device=eng.device))
    eng.plan_prioritized(8, out=good)
    bad_outs = [(torch.empty((B, 9, N), dtype=torch.int8, device=eng.device), good[1]),      # shape
                (good[0].to(torch.int16), good[1]),                                        # dtype
                (good[0], torch.empty((B, N), dtype=torch.int64, device=eng.device)),      # dtype
                (good[0], good[1][:, :-1]),                                                # shape
                (good[0].cpu(), good[1]),                                                  # host tensor
                good[0]]                                                                   # not a pair
    for out in bad_outs:
        with pytest.raises(ValueError):
            eng.plan_prioritized(8, out=out)
    with pytest.raises(ValueError):
        eng.plan_prioritized(8, mask=torch.ones((B + 1,), dtype=torch.uint8))
    assert _poll(eng)[0] == 0


# ---- 6. capture ----------------------------------------------------------------------------------------------------------
def test_graph_capture_of_plan_then_step():
    shape = pq.SHAPES[2]
    N, T, K = shape[3], 32, 4
    eager, B = _engine(shape)
    cap, _ = _engine(shape)
    want = []
    for _ in range(K):
        plan, arrival = eager.plan_prioritized(T)
        out = eager.step(plan[:, 0].contiguous())
        want.append((plan.cpu().numpy(), arrival.cpu().numpy(), out["rewards"].cpu().numpy(), eager.get_state()["positions"]))
    bufs = (torch.zeros((B, T, N), dtype=torch.int8, device=cap.device), torch.zeros((B, N), dtype=torch.int32, device=cap.device))
    a_buf = torch.zeros((B, N), dtype=torch.int8, device=cap.device)
    scratch = tuple(torch.zeros_like(t) for t in bufs)
    cap.plan_prioritized(T, out=scratch)  # the warm-up call sizes the handle's workspace
    s = torch.cuda.Stream(cap.device)
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):  # one linear chain: plan, pick the first step's actions, step
        cap.plan_prioritized(T, out=bufs)
        a_buf.copy_(bufs[0][:, 0])
        cap.step(a_buf)
    torch.cuda.synchronize()
    for k in range(K):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(bufs[0].cpu().numpy(), want[k][0]), k
        assert np.array_equal(bufs[1].cpu().numpy(), want[k][1]), k
        assert np.array_equal(cap._rewards.cpu().numpy(), want[k][2]), k
        assert np.array_equal(cap.get_state()["positions"], want[k][3]), k
    assert _poll(cap)[0] == 0
    eager.close()
    cap.close()


# ---- 7. policy -------------------------------------------------------------------------------------------------------------
def test_evaluate_with_the_prioritized_policy():
    import plan_util as pu
    from dl_reference_models_amd import evaluation as evm

    B, N, spe = 16, 4, 48
    grids = pu.random_grids(12, 12, B, pu.DENSITY_CONNECTED, 2 * N)
    cfg = {"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": spe,
           "seeds": list(range(B))}
    env = _vec(cfg)
    res, _heat = evm.evaluate(env, "prioritized", 2, poll_every=8)
    M = len(res["env"])
    assert M == 2 * B
    n_solved = 0
    for m in range(M):
        _plan, arrival, _cells = pq.plan_bit_rows(grids[res["env"][m]], res["starts"][m], res["goals"][m], spe)
        costs = evm.plan_costs(arrival[None])
        if costs["solved"][0]:
            n_solved += 1
            assert res["terminated"][m] and not res["truncated"][m], m
            assert res["timesteps"][m] <= max(int(costs["makespan"][0]), 1), (m, res["timesteps"][m], costs["makespan"][0])
    assert 2 * n_solved >= M
    assert len(set(res["timesteps"].tolist())) > 1  # the episodes end at different times
    # the callable form, with a shorter horizon: past it the agents wait
    res2, _ = evm.evaluate(env, evm.prioritized_policy(env, horizon=3), 1)
    assert len(res2["env"]) == B
    env.close()
    lifelong = _vec(dict(cfg, lifelong_mapf=True))
    with pytest.raises(ValueError):
        evm.evaluate(lifelong, "prioritized", 1)
    with pytest.raises(ValueError):
        evm.prioritized_policy(lifelong)
    lifelong.close()


# ---- 8. facade, script, single-agent handle ----------------------------------------------------------------------------------
def test_facade_dicts_equal_row_zero_of_the_tensor_call():
    from dl_reference_models_amd.reference_model_multi_agent import ReferenceModel

    env = ReferenceModel({"env_name": "ReferenceModel-2-1", "num_agents": 4, "seed": 5, "sensor_range": 2})
    env.reset()
    acts, arrival = env.plan_prioritized(horizon=40)
    plan_t, arr_t = env._engine.plan_prioritized(40)
    plan_t, arr_t = plan_t[0].cpu().numpy(), arr_t[0].cpu().numpy()
    assert list(acts) == list(arrival) == [f"agent_{i}" for i in range(4)]
    for i in range(4):
        assert acts[f"agent_{i}"] == plan_t[:, i].tolist() and all(type(v) is int for v in acts[f"agent_{i}"])
        assert arrival[f"agent_{i}"] == int(arr_t[i]) and type(arrival[f"agent_{i}"]) is int
    st = env._engine.get_state()
    want_plan, want_arr, _ = pq.plan_bit_rows(np.asarray(env.grid, np.uint8), st["positions"][0], st["goals"][0], 40)
    assert np.array_equal(plan_t, want_plan) and np.array_equal(arr_t, want_arr)
    # the default horizon
    acts, _ = env.plan_prioritized()
    assert len(acts["agent_0"]) == min(env._engine.steps_per_episode, env._engine.plan_max_horizon)
    env.close()


def test_script_runs_the_prioritized_policy(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("eval_cli", os.path.join(ROOT, "scripts", "evaluate_multi_agent_env.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--policy", "PRIORITIZED", "--num-envs", "8", "--episodes", "1", "--steps-per-episode", "40",
                    "--output-dir", str(tmp_path / "PRIORITIZED")])
    assert len(out["table"]) == 8
    assert os.path.basename(out["csv"]).startswith("ReferenceModel-2-1_PRIORITIZED_4_agents_")
    assert out["summary"]["average sum_of_costs_lower_bound"] >= out["summary"]["average makespan_lower_bound"] > 0
    assert "Average makespan_lower_bound:" in capsys.readouterr().out


def test_single_agent_handle():
    import plan_util as pu
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    B, N, H, W, T = 7, 3, 12, 12, 40
    grids = pu.random_grids(H, W, B, pu.DENSITY_CONNECTED, 2 * N)
    eng = VecSingleAgentReferenceModel({"grid": np.array(grids), "num_envs": B, "num_agents": N, "seeds": list(range(B)),
                                        "device": DEV, "steps_per_episode": 20})
    eng.reset()
    st = eng.get_state()
    plan, arrival, _cells = pq.plan_batch(pq.plan_bit_rows, grids, st["positions"], st["goals"], T)
    got_plan, got_arr = eng.plan_prioritized(T)
    _assert_equal(got_plan.cpu().numpy(), got_arr.cpu().numpy(), plan, arrival, "single-agent handle")
    assert tuple(eng.plan_prioritized()[0].shape) == (B, 20, N)  # the default horizon: steps_per_episode
    assert _poll(eng)[0] == 0
    eng.close()
