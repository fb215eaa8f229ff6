"""Single-agent (CTE) sibling env on the GPU: golden traces recorded from the reference, the oracle at size, the
drop-in gym.Env class, and the reference's own dtype/bounds test for this env."""

import numpy as np
import pytest

from trace_util import (CTE_FIXTURES, CteEngineStepper, CteOracleStepper, _eq, load_golden, replay_cte_trace, synth_grids)

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", CTE_FIXTURES)
def test_cte_engine_matches_golden_trace(name):
    fx = load_golden(name)
    replay_cte_trace(CteEngineStepper, fx)


@pytest.mark.parametrize("shape", [(512, 16, 16, 4, {}), (300, 32, 32, 8, {"blocking_penalty": -0.3}),
                                   (40, 64, 64, 64, {"steps_per_episode": 50}), (70, 5, 9, 7, {"steps_per_episode": 30})])
def test_cte_engine_vs_oracle(shape):
    B, H, W, N, extra = shape
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": 60}
    cfg.update(extra)
    grids = synth_grids(B, H, W, 0.2, N, base_seed=140_000)
    seeds = list(range(B))
    a, b = CteEngineStepper(grids, cfg, seeds=seeds), CteOracleStepper(grids, cfg, seeds=seeds)
    _eq("reset obs", a.reset(), b.reset())
    rng = np.random.default_rng(4)
    blocking = goals = 0.0
    for t in range(150):
        pos, gl = b.positions().astype(int), b.goals().astype(int)
        d = gl - pos
        greedy = np.where(np.abs(d[..., 0]) >= np.abs(d[..., 1]), np.where(d[..., 0] > 0, 3, np.where(d[..., 0] < 0, 1, 0)),
                          np.where(d[..., 1] > 0, 2, 4))
        acts = np.where(rng.random((B, N)) < 0.6, greedy, rng.integers(0, 5, size=(B, N))).astype(np.int8)
        ra, rb = a.step(acts), b.step(acts)
        for k in ("obs", "reward", "terminated", "truncated", "info"):
            _eq(k, ra[k], rb[k], t)
        blocking += rb["info"][:, 0].sum()
        goals += rb["info"][:, 1].sum()
    _eq("positions", a.positions(), b.positions())
    _eq("rng", a.rng_words(), b.rng_words())
    assert goals > 0


def test_single_agent_dropin_class_like_the_reference_dtype_test():
    """reference tests/test_reference_model_observation_dtypes.py:44-56 against the drop-in class."""
    from dl_reference_models_amd.reference_model_single_agent import ReferenceModel

    env = ReferenceModel({"env_name": "ReferenceModel-2-1", "seed": 123, "deterministic": True, "num_agents": 4,
                          "steps_per_episode": 20, "sensor_range": 2, "render_env": False,
                          "validate_observation_space": True})
    obs, info = env.reset()
    assert obs.dtype == np.float32 and env.observation_space.contains(obs)
    mask = obs[env._obs_slices["action_mask"]]
    assert np.all(np.isin(mask, np.array([0.0, 1.0], dtype=np.float32))) and np.array_equal(mask, info["action_mask"])
    nxt, reward, term, trunc, inf = env.step([0] * env.num_agents)
    assert nxt.dtype == np.float32 and env.observation_space.contains(nxt) and isinstance(reward, float)
    assert set(inf) == {"action_mask", "blocking_count_step", "goals_reached_step", "goals_reached_total",
                        "blocking_count_total"}
    split = env.split_flat_observation(nxt)
    assert split["observations"].shape == env.grid.shape
    # the deterministic fixture of the reference (gs_cte_named_2_1_det) through the dict-free gym API
    fx = load_golden("gs_cte_named_2_1_det")
    env2 = ReferenceModel(dict(fx["config"], seed=123))
    o, _ = env2.reset()
    assert np.array_equal(o, fx["reset0_obs"][0])
    for t in range(40):
        o, r, te, tr, _i = env2.step(fx["actions"][t, 0].tolist())
        assert np.array_equal(o, fx["obs"][t, 0]) and r == fx["reward"][t, 0] and te == bool(fx["terminated"][t, 0])
        if te or tr:
            break
    with pytest.raises(ValueError, match="Invalid action"):
        env.step([0, 9, 0, 0])


def test_cte_randomized_configuration_fuzz():
    rng = np.random.default_rng(77)
    for case in range(15):
        H, W = int(rng.integers(2, 65)), int(rng.integers(2, 65))
        N = int(rng.integers(1, min(64, max(1, (H * W) // 4)) + 1))
        cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": int(rng.integers(3, 50)),
               "blocking_penalty": float(rng.choice([-0.2, -0.3, -1.0])),
               "move_after_goal_penalty": float(rng.choice([-0.05, -0.07, 0.0]))}
        B = int(rng.integers(1, 30))
        grids = synth_grids(B, H, W, float(rng.choice([0.0, 0.2])), N, base_seed=int(rng.integers(0, 10**6)))
        seeds = [int(x) for x in rng.integers(0, 10**6, size=B)]
        a, b = CteEngineStepper(grids, cfg, seeds=seeds), CteOracleStepper(grids, cfg, seeds=seeds)
        _eq(f"case {case} reset", a.reset(), b.reset())
        p = rng.dirichlet(np.ones(5))
        for t in range(70):
            acts = rng.choice(5, size=(B, N), p=p).astype(np.int8)
            ra, rb = a.step(acts), b.step(acts)
            for k in ("obs", "reward", "terminated", "truncated", "info"):
                _eq(f"case {case} {cfg} {H}x{W} {k}", ra[k], rb[k], t)
        _eq(f"case {case} rng", a.rng_words(), b.rng_words())


@pytest.mark.parametrize("shape", [(130, 16, 16, 4, 23, 0), (65, 9, 7, 5, 6, 0), (40, 32, 32, 8, 31, 64), (24, 12, 12, 3, 1, 8),
                                   (20, 40, 37, 40, 17, 0),
                                   # fused and single-step launches of one handle on DIFFERENT group widths (lanes = 0: the
                                   # engine picks 32 / 8 and 8 / 4 lanes at these batch sizes), and the narrow widths by hand
                                   (2048, 32, 32, 8, 31, 0), (8192, 16, 16, 4, 23, 0), (130, 16, 16, 4, 23, 4), (70, 16, 16, 7, 9, 8),
                                   (33, 20, 20, 16, 12, 16)])
def test_cte_fused_launch_equals_single_steps_of_the_oracle(shape):
    """mapf_cte_step_many: T steps in one launch (positions in registers, the obstacle part of the observation row written
    once, the touched cells put back after every row) against the oracle stepped T times with reset-on-done; every
    observation mode, episode ends inside the launch (also episodes of ONE step), single steps in between."""
    import torch

    B, H, W, N, spe, lanes = shape
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": spe}
    grids = synth_grids(B, H, W, 0.2, N, base_seed=150_000)
    seeds = list(range(B))
    a = CteEngineStepper(grids, cfg, seeds=seeds, lanes_per_env=lanes)
    b = CteOracleStepper(grids, cfg, seeds=seeds)
    _eq("reset obs", a.reset(), b.reset())
    if lanes == 0 and B >= 2048:
        assert a.env.launch_info()["lanes_per_env"] != a.env.launch_info(fused=True)["lanes_per_env"]
    rng = np.random.default_rng(4)
    for rep, (T, mode) in enumerate(((37, 2), (5, 1), (11, 0), (1, 2), (19, 2), (1, 0), (26, 1))):
        acts = rng.integers(0, 5, size=(T, B, N)).astype(np.int8)
        out = a.env.step_many(torch.from_numpy(acts).to(a.env.device), obs_mode=mode)
        refs = [b.step(acts[t]) for t in range(T)]
        for k in ("reward", "terminated", "truncated", "info"):
            _eq(f"fused {k}", out[k].cpu().numpy(), np.stack([r[k] for r in refs]), rep)
        if mode == 2:
            _eq("fused obs", out["obs"].cpu().numpy(), np.stack([r["obs"] for r in refs]), rep)
        elif mode == 1:
            _eq("fused last obs", out["obs"].cpu().numpy(), refs[-1]["obs"], rep)
        _eq("positions", a.positions(), b.positions(), rep)
        _eq("rng", a.rng_words(), b.rng_words(), rep)
        acts1 = rng.integers(0, 5, size=(B, N)).astype(np.int8)  # a single step between fused launches
        ra, rb = a.step(acts1), b.step(acts1)
        for k in ("obs", "reward", "terminated", "truncated", "info"):
            _eq(f"single {k}", ra[k], rb[k], rep)
    a.env.poll_error()


def test_cte_ctor_refuses_a_seed_list_of_the_wrong_length():
    # (checked after mapf_create, as in VecReferenceModel: before, a short list reached mapf_set_rng_state mis-sized)
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

    cfg = {"grid": np.zeros((6, 6), dtype=np.uint8), "num_agents": 2, "num_envs": 3}
    with pytest.raises(ValueError, match="need one seed per env"):
        VecSingleAgentReferenceModel(dict(cfg, seeds=[1, 2]))
    env = VecSingleAgentReferenceModel(dict(cfg, seeds=[1, 2, 3]))
    assert env.get_state()["rng_words"].shape == (3, 6)
    env.close()
