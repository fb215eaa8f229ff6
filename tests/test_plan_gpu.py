"""The shortest-path planner on the device (mapf_expert_actions, mapf_path_lengths, mapf_distance_field) against the NumPy
restatement of its rule (plan_util), element for element, with every output in a guarded, poisoned arena (guard_util):
guards intact, every element the contract names written, nothing else -- then the layers above: the tensor API, graph
capture, the evaluation loop and its bounds, the dict facade and the script."""

import ctypes as C
import functools
import importlib.util
import os

import numpy as np
import pytest
import torch

import plan_util as pu
from guard_util import GuardedBuffer, device_bytes, guard_bytes_for

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"


def _vec(cfg):
    from dl_reference_models_amd.vec_env import VecReferenceModel

    return VecReferenceModel(dict({"device": DEV}, **cfg))


def _group_width(H):
    return next(g for g in (4, 8, 16, 32, 64) if g >= H)


def _batches(H):
    """B in {1, G + 1, 3G - 1} for G searches per wavefront ({1, 3} when a search takes the whole wavefront)."""
    G = 64 // _group_width(H)
    return (1, 3) if G == 1 else (1, G + 1, 3 * G - 1)


def _grids(kind, H, W, B, density=pu.DENSITY, need_free=2):
    return pu.random_grids(H, W, B, density, need_free) if kind == "random" else pu.serpentine_grids(H, W, B)


@functools.lru_cache(maxsize=None)
def _query_engine(kind, H, W):
    """One handle per grid shape for the field and path-length tests: 5 envs with a grid each, one agent."""
    B = 5
    grids = _grids(kind, H, W, B)
    return _vec({"grid": np.array(grids), "num_envs": B, "num_agents": 1, "sensor_range": 1, "seeds": list(range(B))}), grids


GRID_PARAMS = [("random", H, W) for H, W in pu.SHAPES] + [("serpentine", H, W) for H, W in pu.SERPENTINES]
GRID_IDS = [f"{k}_{H}x{W}" for k, H, W in GRID_PARAMS]


def _sync():
    torch.cuda.synchronize()


def _poll(eng):
    env, agent, value = C.c_int32(-1), C.c_int32(-1), C.c_int32(0)
    rc = eng._lib.mapf_poll_error(eng._h, eng._stream(), C.byref(env), C.byref(agent), C.byref(value))
    return rc, env.value, value.value


def _ptr(t):
    return C.c_void_p(t.data_ptr())


# ---- 1. fields ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,W", GRID_PARAMS, ids=GRID_IDS)
def test_distance_fields(kind, H, W):
    eng, grids = _query_engine(kind, H, W)
    for K in (1, 5, 67):
        env_ids, _src, dst = pu.queries(grids, K, 100 + K)
        if K == 5 and (grids != 0).any():  # a destination on an obstacle: the whole field says "no path"
            b = int(np.argwhere((grids != 0).any(axis=(1, 2)))[0, 0])
            env_ids[2], dst[2] = b, np.argwhere(grids[b] != 0)[0]
        buf = GuardedBuffer((K, H, W), np.uint16, DEV, guard_bytes_for(H * W * 2), name="field")
        ids_d, dst_d = device_bytes(eng, env_ids, np.int32), device_bytes(eng, dst, np.int16)
        eng._check(eng._lib.mapf_distance_field(eng._h, K, _ptr(ids_d), _ptr(dst_d), buf.ptr, eng._stream()))
        _sync()
        got = buf.check(True, f"K = {K}")
        cache = {}
        for k in range(K):
            key = (int(env_ids[k]), int(dst[k, 0]), int(dst[k, 1]))
            if key not in cache:
                cache[key] = pu.field_u16(grids[key[0]], key[1:])
            bad = np.argwhere(got[k] != cache[key])
            assert bad.size == 0, f"K = {K}, query {k} {key}: {len(bad)} cells differ, first {bad[0].tolist()}: " \
                                  f"{got[k][tuple(bad[0])]} != {cache[key][tuple(bad[0])]}"
        if K == 5 and (grids != 0).any():
            assert (got[2] == pu.NO_PATH_U16).all()
    assert _poll(eng)[0] == 0


def test_distance_field_tensor_api_and_bad_arguments():
    from dl_reference_models_amd import _lib as L

    eng, grids = _query_engine("random", 12, 33)
    env_ids, _src, dst = pu.queries(grids, 9, 7)
    f = eng.distance_field(env_ids, dst)
    assert f.dtype == torch.uint16 and tuple(f.shape) == (9, 12, 33) and f.device == eng.device
    got = f.cpu().numpy()
    for k in range(9):
        assert np.array_equal(got[k], pu.field_u16(grids[env_ids[k]], dst[k])), k
    ids_d, dst_d = device_bytes(eng, env_ids, np.int32), device_bytes(eng, dst, np.int16)
    buf = GuardedBuffer((9, 12, 33), np.uint16, DEV, name="field")
    for K in (0, -3):
        assert eng._lib.mapf_distance_field(eng._h, K, _ptr(ids_d), _ptr(dst_d), buf.ptr, eng._stream()) == L.MAPF_ERR_CONFIG
        assert eng._lib.mapf_path_lengths(eng._h, K, _ptr(ids_d), _ptr(dst_d), _ptr(dst_d), buf.ptr, eng._stream()) == L.MAPF_ERR_CONFIG
    _sync()
    buf.check(False, "K <= 0: nothing launched")
    # a bad env id: the field of that query is not written, the others are, the error record names query and id
    bad_ids = env_ids.copy()
    bad_ids[4] = 5
    bad_d = device_bytes(eng, bad_ids, np.int32)
    eng._check(eng._lib.mapf_distance_field(eng._h, 9, _ptr(bad_d), _ptr(dst_d), buf.ptr, eng._stream()))
    _sync()
    buf.check(np.arange(9) != 4, "env id 5 of 5 envs in query 4")
    assert _poll(eng) == (L.MAPF_ERR_CONFIG, 4, 5)
    with pytest.raises(ValueError):
        eng.distance_field([], np.zeros((0, 2), np.int16))
    with pytest.raises(ValueError):
        eng.distance_field([0, 1], [[0, 0]])


# ---- 2. path lengths ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,H,W", GRID_PARAMS, ids=GRID_IDS)
def test_path_lengths(kind, H, W):
    eng, grids = _query_engine(kind, H, W)
    for K in (1, 67, 200):
        env_ids, src, dst = pu.queries(grids, K, 200 + K)
        if K > 2:  # a source and a destination outside the grid
            src[2] = (H, 0)
            dst[K - 1] = (0, -1)
        buf = GuardedBuffer((K,), np.int32, DEV, name="out")
        # (the inputs stay referenced until the launch has run: a temporary's block would be handed to the next one)
        ids_d, src_d, dst_d = device_bytes(eng, env_ids, np.int32), device_bytes(eng, src, np.int16), device_bytes(eng, dst, np.int16)
        eng._check(eng._lib.mapf_path_lengths(eng._h, K, _ptr(ids_d), _ptr(src_d), _ptr(dst_d), buf.ptr, eng._stream()))
        _sync()
        got = buf.check(True, f"K = {K}")
        cache, want = {}, np.zeros(K, np.int32)
        for k in range(K):
            key = (int(env_ids[k]), int(dst[k, 0]), int(dst[k, 1]))
            if key not in cache:
                cache[key] = pu.field(grids[key[0]], key[1:])
            want[k] = pu.distance(grids[key[0]], src[k], key[1:], cache[key])
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"K = {K}: {len(bad)} differ, first query {bad[0]}: {got[bad[0]]} != {want[bad[0]]}"
        assert got[0] == 0  # src = dst on a free cell
        if K == 200 and kind == "random" and (H, W) != (3, 3):
            assert (want == -1).any() and (want > 0).any()
    assert _poll(eng)[0] == 0
    # the tensor API gives the same numbers
    t = eng.path_lengths(env_ids, src, dst)
    assert t.dtype == torch.int32 and np.array_equal(t.cpu().numpy(), want)


def test_path_lengths_bad_env_id_leaves_its_row_alone():
    from dl_reference_models_amd import _lib as L

    eng, grids = _query_engine("random", 12, 12)
    K = 67
    env_ids, src, dst = pu.queries(grids, K, 31)
    env_ids[40] = -1
    buf = GuardedBuffer((K,), np.int32, DEV, name="out")
    ids_d, src_d, dst_d = device_bytes(eng, env_ids, np.int32), device_bytes(eng, src, np.int16), device_bytes(eng, dst, np.int16)
    eng._check(eng._lib.mapf_path_lengths(eng._h, K, _ptr(ids_d), _ptr(src_d), _ptr(dst_d), buf.ptr, eng._stream()))
    _sync()
    got = buf.check(np.arange(K) != 40, "env id -1 in query 40")
    assert _poll(eng) == (L.MAPF_ERR_CONFIG, 40, -1)
    for k in (0, 39, 41, K - 1):
        assert got[k] == pu.distance(grids[env_ids[k]], src[k], dst[k])


# ---- 3. expert actions -------------------------------------------------------------------------------------------------
def _check_expert(eng, grids, what):
    """Both modes, dist given and NULL, against the restatement on the state mapf_get_state reports."""
    st = eng.get_state()
    pos, goals = st["positions"], st["goals"]
    B, N = pos.shape[:2]
    fields = pu.goal_fields(grids, goals)
    acts = GuardedBuffer((B, N), np.int8, DEV, name="actions")
    dist = GuardedBuffer((B, N), np.int32, DEV, name="dist")
    out = {}
    for mode in (0, 1):
        want_a, want_d = pu.expert(grids, pos, goals, mode, fields)
        for with_dist in (True, False):
            acts.poison()
            dist.poison()
            eng._check(eng._lib.mapf_expert_actions(eng._h, mode, acts.ptr, dist.ptr if with_dist else None, eng._stream()))
            _sync()
            where = f"{what}, mode {mode}, dist {'given' if with_dist else 'NULL'}"
            got_a = acts.check(True, where)
            got_d = dist.check(with_dist, where)
            bad = np.argwhere(got_a != want_a)
            assert bad.size == 0, (f"{where}: {len(bad)} actions differ, first (env, agent) {bad[0].tolist()}: "
                                   f"{got_a[tuple(bad[0])]} != {want_a[tuple(bad[0])]}, at {pos[tuple(bad[0])]} -> {goals[tuple(bad[0])]}")
            if with_dist:
                bad = np.argwhere(got_d != want_d)
                assert bad.size == 0, f"{where}: {len(bad)} distances differ, first {bad[0].tolist()}: " \
                                      f"{got_d[tuple(bad[0])]} != {want_d[tuple(bad[0])]}"
        out[mode] = (want_a, want_d)
    return out


def _random_steps(eng, T, seed):
    rng = np.random.default_rng(seed)
    for _ in range(T):
        eng.step(torch.from_numpy(rng.integers(0, 5, size=(eng.num_envs, eng.num_agents)).astype(np.int8)).to(eng.device))


# (kind, H, W, N, density): N in {1, 4, 8, 9, 16, 33, 64} across the group widths of the step kernels and of the planner
EXPERT_CONFIGS = [("random", 3, 3, 1, 0.4), ("random", 12, 12, 4, 0.4), ("random", 12, 31, 8, 0.4), ("random", 12, 32, 9, 0.4),
                  ("random", 12, 33, 16, 0.4), ("random", 33, 12, 33, 0.4), ("random", 5, 64, 16, 0.4),
                  ("random", 64, 64, 64, 0.4), ("serpentine", 11, 12, 8, 0.0), ("serpentine", 13, 64, 4, 0.0)]
EXPERT_PARAMS = [(k, H, W, N, d, B) for k, H, W, N, d in EXPERT_CONFIGS for B in _batches(H)]


@pytest.mark.parametrize("kind,H,W,N,density,B", EXPERT_PARAMS, ids=[f"{k}_{H}x{W}_n{N}_b{B}" for k, H, W, N, _d, B in EXPERT_PARAMS])
def test_expert_actions(kind, H, W, N, density, B):
    grids = _grids(kind, H, W, B, density, 2 * N)
    eng = _vec({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": 30,
                "seeds": [50 + b for b in range(B)]})
    eng.reset()
    first = _check_expert(eng, grids, "after reset")
    _random_steps(eng, 5, N)
    _check_expert(eng, grids, "after five random steps")
    if kind == "random" and N >= 16 and B > 1:  # what the random grids give without looking for it
        _a0, d0 = first[0]  # (where the two modes part is pinned by the hand cases: a random placement need not hold one)
        assert (d0 == -1).any() and (d0 > 0).any()
    assert _poll(eng)[0] == 0
    eng.close()


@pytest.mark.parametrize("case", pu.RULE_CASES, ids=lambda c: c["name"])
def test_expert_hand_cases(case):
    g = case["grid"]
    eng = _vec({"grid": g, "num_envs": 1, "num_agents": 2, "sensor_range": 1, "seed": 1})
    eng.set_state(positions=case["positions"][None], goals=case["goals"][None], clear_episode=True)
    for mode in ("independent", "yielding"):
        a, d = eng.expert_actions(mode, return_distance=True)
        assert a.cpu().numpy()[0].tolist() == case[mode], mode
        assert d.cpu().numpy()[0].tolist() == case["dist"], mode
    eng.close()


def test_expert_lifelong_goals_change_under_the_planner():
    B, N, H, W = 5, 4, 12, 12
    grids = _grids("random", H, W, B, pu.DENSITY_CONNECTED, 2 * N + 8)
    eng = _vec({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": 40,
                "lifelong_mapf": True, "seeds": [70 + b for b in range(B)]})
    eng.reset()
    goals0 = eng.get_state()["goals"]
    for t in range(12):
        want = _check_expert(eng, grids, f"lifelong, step {t}")[1][0]
        eng.step(torch.from_numpy(want).to(eng.device))
    assert (eng.get_state()["goals"] != goals0).any()  # agents arrived and were handed new goals on the way
    assert _poll(eng)[0] == 0
    eng.close()


def test_expert_deterministic_config():
    B, N, H, W = 5, 4, 12, 12
    grids = _grids("random", H, W, B, pu.DENSITY, 2 * N)
    fs, fg = [], []
    for b in range(B):
        free = pu.free_cells(grids[b])
        pick = np.random.default_rng(600 + b).permutation(len(free))[:2 * N]
        fs.append(free[pick[:N]])
        fg.append(free[pick[N:]])
    fs, fg = np.array(fs, np.int16), np.array(fg, np.int16)
    eng = _vec({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": 30,
                "deterministic": True, "fixed_starts": fs, "fixed_goals": fg, "seeds": list(range(B))})
    eng.reset()
    st = eng.get_state()
    assert np.array_equal(st["positions"], fs) and np.array_equal(st["goals"], fg)
    _check_expert(eng, grids, "deterministic, after reset")
    _random_steps(eng, 5, 3)
    _check_expert(eng, grids, "deterministic, after five random steps")
    eng.close()


def test_single_agent_handle():
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    B, N, H, W = 7, 3, 12, 12
    grids = _grids("random", H, W, B, pu.DENSITY, 2 * N)
    eng = VecSingleAgentReferenceModel({"grid": np.array(grids), "num_envs": B, "num_agents": N, "seeds": list(range(B)),
                                        "device": DEV, "steps_per_episode": 20})
    eng.reset()
    _check_expert(eng, grids, "single-agent handle, after reset")
    _random_steps(eng, 5, 4)
    _check_expert(eng, grids, "single-agent handle, after five random steps")
    env_ids, src, dst = pu.queries(grids, 20, 5)
    want = [pu.distance(grids[e], s, d) for e, s, d in zip(env_ids, src, dst)]
    assert eng.path_lengths(env_ids, src, dst).cpu().numpy().tolist() == want
    assert np.array_equal(eng.distance_field(env_ids[:3], dst[:3]).cpu().numpy(),
                          np.stack([pu.field_u16(grids[e], d) for e, d in zip(env_ids[:3], dst[:3])]))
    eng.close()


def test_mode_two_is_refused():
    from dl_reference_models_amd import _lib as L

    eng, _ = _query_engine("random", 12, 12)
    acts = GuardedBuffer((5, 1), np.int8, DEV, name="actions")
    dist = GuardedBuffer((5, 1), np.int32, DEV, name="dist")
    for mode in (2, -1):
        assert eng._lib.mapf_expert_actions(eng._h, mode, acts.ptr, dist.ptr, eng._stream()) == L.MAPF_ERR_CONFIG
    assert eng._lib.mapf_expert_actions(eng._h, 0, None, dist.ptr, eng._stream()) == L.MAPF_ERR_CONFIG
    _sync()
    acts.check(False, "refused: nothing launched")
    dist.check(False, "refused: nothing launched")
    with pytest.raises(ValueError):
        eng.expert_actions("greedy")
    with pytest.raises(ValueError):
        eng.expert_actions("yielding", out=torch.empty((5, 1), dtype=torch.int8))  # host tensor


# ---- 4. untouched state ------------------------------------------------------------------------------------------------
def _slots(eng):
    B, N = eng.num_envs, eng.num_agents
    slots, stage, vis = np.zeros(B * N, np.uint32), np.zeros(B * (4 * N + 4), np.uint32), np.zeros(B * 6, np.uint64)
    eng._check(eng._lib.mapf_debug_slots(eng._h, slots.ctypes.data_as(C.c_void_p), stage.ctypes.data_as(C.c_void_p),
                                         vis.ctypes.data_as(C.c_void_p)))
    return slots, stage, vis


def test_planning_changes_nothing():
    B, N = 40, 8
    grids = _grids("random", 16, 16, B, pu.DENSITY_CONNECTED, 2 * N)
    cfg = {"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": 20,
           "seeds": list(range(B))}
    a, b = _vec(cfg), _vec(cfg)
    _random_steps(a, 15, 7)
    _random_steps(b, 15, 7)
    env_ids, src, dst = pu.queries(grids, 50, 9)
    calls = {"expert_actions(independent)": lambda: a.expert_actions("independent", return_distance=True),
             "expert_actions(yielding)": lambda: a.expert_actions("yielding"),
             "path_lengths": lambda: a.path_lengths(env_ids, src, dst),
             "distance_field": lambda: a.distance_field(env_ids, dst)}
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
    rng = np.random.default_rng(8)
    names = list(calls)
    for t in range(40):
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


# ---- 5. capture --------------------------------------------------------------------------------------------------------
def test_graph_capture_of_expert_then_step():
    B, N, T = 16, 4, 5
    grids = _grids("random", 10, 12, B, pu.DENSITY_CONNECTED, 2 * N)
    cfg = {"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 1, "steps_per_episode": 6,
           "seeds": list(range(B))}
    eager, cap = _vec(cfg), _vec(cfg)
    eager.reset()
    cap.reset()
    want = []
    for _ in range(T):
        acts = eager.expert_actions("yielding")
        out = eager.step(acts)
        want.append((acts.cpu().numpy(), out["rewards"].cpu().numpy(), eager.get_state()["positions"]))
    a_buf = torch.zeros((B, N), dtype=torch.int8, device=cap.device)
    s = torch.cuda.Stream(cap.device)
    s.wait_stream(torch.cuda.current_stream())
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        cap.expert_actions("yielding", out=a_buf)
        cap.step(a_buf)
    torch.cuda.synchronize()
    # capturing does not run the launches: the first replay is the first step
    for t in range(T):
        g.replay()
        torch.cuda.synchronize()
        assert np.array_equal(a_buf.cpu().numpy(), want[t][0]), t
        assert np.array_equal(cap._rewards.cpu().numpy(), want[t][1]), t
        assert np.array_equal(cap.get_state()["positions"], want[t][2]), t
    assert _poll(cap)[0] == 0


# ---- 6. closed loop ----------------------------------------------------------------------------------------------------
def _restated_lengths(grids, res):
    M, N = res["starts"].shape[:2]
    return np.array([[pu.distance(grids[res["env"][m]], res["starts"][m, i], res["goals"][m, i]) for i in range(N)]
                     for m in range(M)], np.int32).reshape(M, N)


def test_closed_loop_single_agent_walks_its_shortest_path():
    from dl_reference_models_amd import evaluation as evm

    B, spe = 64, 150  # (longer than any path of a 12 x 12 grid: only an unreachable goal runs into the limit)
    grids = _grids("random", 12, 12, B, pu.DENSITY_CONNECTED, 2)
    env = _vec({"grid": np.array(grids), "num_envs": B, "num_agents": 1, "sensor_range": 2, "steps_per_episode": spe,
                "seeds": list(range(B))})
    res, _heat = evm.evaluate(env, "shortest_path_independent", 2)
    assert len(res["env"]) == 2 * B
    bounds = evm.path_length_bounds(env, res)
    sp = bounds["shortest_path"]
    assert sp.dtype == np.int32 and sp.shape == (2 * B, 1)
    assert np.array_equal(sp, _restated_lengths(grids, res))
    reach = sp[:, 0] >= 0
    assert reach.any()
    # a single agent is never blocked: it arrives after exactly its shortest path
    assert np.array_equal(res["timesteps"][reach], sp[reach, 0])
    assert res["terminated"][reach].all() and not res["truncated"][reach].any()
    assert (res["timesteps"][~reach] == spe).all() and res["truncated"][~reach].all()
    assert np.array_equal(bounds["makespan_lower_bound"], sp[:, 0])
    assert np.array_equal(bounds["sum_of_costs_lower_bound"], sp[:, 0].astype(np.int64))
    env.close()


def test_closed_loop_four_agents_yielding():
    from dl_reference_models_amd import evaluation as evm

    B, N = 64, 4
    grids = _grids("random", 12, 12, B, pu.DENSITY_CONNECTED, 2 * N)
    env = _vec({"grid": np.array(grids), "num_envs": B, "num_agents": N, "sensor_range": 2, "steps_per_episode": 40,
                "seeds": list(range(B))})
    inner = evm.shortest_path_policy(env, yielding=True)
    seen = []

    def policy(obs, first):
        a = inner(obs, first)
        seen.append(a.clone())
        return a

    res, _heat = evm.evaluate(env, policy, 2)
    acts = torch.stack(seen).cpu().numpy()
    assert acts.dtype == np.int8 and acts.min() >= 0 and acts.max() <= 4 and (acts > 0).any()
    assert len(res["env"]) == 2 * B
    bounds = evm.path_length_bounds(env, res)
    assert np.array_equal(bounds["shortest_path"], _restated_lengths(grids, res))
    ok = res["terminated"] & ~res["truncated"]
    assert ok.any()
    # every agent needs at least its shortest path, and the episode lasts until the last one has arrived
    assert (bounds["sum_of_costs_lower_bound"][ok] >= 0).all()
    assert (N * res["timesteps"][ok].astype(np.int64) >= bounds["sum_of_costs_lower_bound"][ok]).all()
    assert (res["timesteps"][ok] >= bounds["makespan_lower_bound"][ok]).all()
    # the string form runs the same policy
    res2, _ = evm.evaluate(env, "shortest_path", 1)
    assert len(res2["env"]) == B
    with pytest.raises(ValueError):
        evm.evaluate(env, "astar", 1)
    env.close()


# ---- 7. facade and script ----------------------------------------------------------------------------------------------
def test_facade_dict_equals_row_zero_of_the_tensor_call():
    from dl_reference_models_amd.reference_model_multi_agent import ReferenceModel

    env = ReferenceModel({"env_name": "ReferenceModel-2-1", "num_agents": 4, "seed": 5, "sensor_range": 2})
    env.reset()
    for _ in range(3):
        for mode in ("yielding", "independent"):
            d = env.expert_actions(mode=mode)
            row = env._engine.expert_actions(mode)[0].cpu().numpy()
            assert list(d) == [f"agent_{i}" for i in range(4)]
            assert [d[f"agent_{i}"] for i in range(4)] == row.tolist() and all(type(v) is int for v in d.values())
        st = env._engine.get_state()
        want, _ = pu.expert(np.asarray(env.grid, np.uint8), st["positions"], st["goals"], 0)
        assert row.tolist() == want[0].tolist()
        env.step(d)
    env.close()


def test_script_runs_the_shortest_path_policies(tmp_path, capsys):
    spec = importlib.util.spec_from_file_location("eval_cli", os.path.join(ROOT, "scripts", "evaluate_multi_agent_env.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    for name in ("SHORTEST_PATH", "SHORTEST_PATH_INDEPENDENT"):
        out = mod.main(["--policy", name, "--num-envs", "8", "--episodes", "1", "--steps-per-episode", "40",
                        "--output-dir", str(tmp_path / name)])
        assert len(out["table"]) == 8
        assert os.path.basename(out["csv"]).startswith(f"ReferenceModel-2-1_{name}_4_agents_")
        s = out["summary"]
        assert s["average sum_of_costs_lower_bound"] >= s["average makespan_lower_bound"] > 0
        printed = capsys.readouterr().out
        assert "Average sum_of_costs_lower_bound:" in printed and "Average makespan_lower_bound:" in printed
