"""The shortest-path guidance without a GPU: the C ABI declares, exports and binds mapf_observe_guided, the NumPy
restatement of its rule (guidance_util) agrees with the existing expert's restatement (plan_util) on every shared case and
gives what the hand cases state, the shared cases hold every class of the rule, and the Python layers refuse by name what
they do not offer."""

import ctypes as C
import importlib.util
import os
import re

import numpy as np
import pytest

import guidance_util as gu
import plan_util as pu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_call_is_declared_exported_and_bound():
    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd import build

    with open(os.path.join(ROOT, "include", "mapf_step.h"), encoding="utf-8") as f:
        header = f.read()
    assert re.search(r"^int mapf_observe_guided\(mapf_handle h, const float \*obs [^,]*, int32_t tail,\s*float \*out [^,]*, void \*stream\);",
                     header, re.M)
    assert re.search(r"^#define MAPF_GUIDANCE_LEN 6$", header, re.M) and L.GUIDANCE_LEN == gu.GUIDANCE_LEN == 6
    assert "mapf_observe_guided" in L.EXPORTED_SYMBOLS
    for path in (build.SO_PATH, build.CHECK_SO_PATH):  # (the checking build holds the kernel too)
        assert hasattr(C.CDLL(path), "mapf_observe_guided"), path
    fn = L.load().mapf_observe_guided
    assert fn.restype is C.c_int and len(fn.argtypes) == 5 and fn.argtypes[2] is C.c_int32


@pytest.mark.parametrize("case", gu.CASES, ids=gu.CASE_IDS)
def test_restatement_against_the_existing_expert(case):
    st = gu.case_state(case)
    H, W = case[1], case[2]
    q = st["q"]
    acts, dist = pu.expert(st["grids"], st["positions"], st["goals"], 0, st["fields"])
    assert np.array_equal(gu.decoded_action(q), acts)
    want5 = np.where(dist < 0, np.float32(-1.0), dist.astype(np.float32) / np.float32(H * W)).astype(np.float32)
    assert np.array_equal(q[..., 5].view(np.int32), want5.view(np.int32))
    assert np.array_equal(gu.decoded_distance(q, H * W), dist)
    assert np.array_equal(q[..., 0] == 1.0, dist == 0) and np.isin(q[..., :5], (0.0, 1.0)).all()
    assert not q[dist <= 0][:, 1:5].any()
    # no test on these cases passes on degenerate input: every class of the rule occurs
    got = gu.classes(q)
    if case[0] == "serpentine":  # (one corridor: a cell never has two ways on)
        assert got.pop("two_moves") == 0
    assert all(n >= 1 for n in got.values()), got
    # and the placements are what mapf_set_state accepts
    for b in range(case[5]):
        assert len({tuple(p) for p in st["positions"][b]}) == len({tuple(g) for g in st["goals"][b]}) == case[3]
        assert (st["grids"][b][tuple(st["positions"][b].T)] == 0).all()


@pytest.mark.parametrize("case", pu.RULE_CASES, ids=lambda c: c["name"])
def test_the_experts_rule_cases(case):
    H, W = case["grid"].shape
    q = gu.guidance_ref(case["grid"], case["positions"][None], case["goals"][None])[0]
    assert gu.decoded_action(q).tolist() == case["independent"]
    assert gu.decoded_distance(q, H * W).tolist() == case["dist"]


@pytest.mark.parametrize("case", gu.HAND_CASES, ids=gu.HAND_IDS)
def test_hand_cases(case):
    grid, pos, goals, want = gu.hand_state(case)
    q = gu.guidance_ref(grid, pos, goals)
    assert np.array_equal(q.view(np.int32), want.view(np.int32)), (q, want)


def test_rows_keep_the_tail_last():
    obs = np.arange(2 * 3 * 7, dtype=np.float32).reshape(2, 3, 7)
    q = -np.ones((2, 3, 6), np.float32)
    for tail in (0, 5, 7):
        rows = gu.guided_rows_ref(obs, q, tail)
        assert rows.shape == (2, 3, 13)
        assert np.array_equal(rows[..., :7 - tail], obs[..., :7 - tail]) and np.array_equal(rows[..., 7 - tail:13 - tail], q)
        assert np.array_equal(rows[..., 13 - tail:], obs[..., 7 - tail:])
    bits = np.array([[[0x7FC00001, -1, 3]]], np.int32)  # (words, not numbers: a NaN's payload stays)
    assert np.array_equal(gu.guided_rows_ref(bits, np.zeros((1, 1, 6), np.float32), 1)[0, 0], [0x7FC00001, -1, 0, 0, 0, 0, 0, 0, 3])


# ---- refusals that need no device ----------------------------------------------------------------------------------------
def test_joint_rollout_refuses_guidance_by_name():
    from dl_reference_models_amd.rollout import JointRollout

    with pytest.raises(ValueError, match="guidance is not offered on the single-agent env"):
        JointRollout(None, None, 4, guidance=True)


def _train_script():
    spec = importlib.util.spec_from_file_location("train_cli", os.path.join(ROOT, "scripts", "train_multi_agent_env.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("extra,what", ((["--algo", "DQN"], "--algo DQN"), (["--population", "2"], "--population")))
def test_script_refuses_guidance_with_dqn_and_with_a_population(extra, what):
    with pytest.raises(SystemExit, match="--guidance is offered with --algo PPO, IMPALA or BC only: " + what):
        _train_script().main(["--guidance", "--device", "cpu"] + extra)


def test_obs_len_check_names_both_numbers():
    from dl_reference_models_amd.rollout import check_guided_obs_len

    check_guided_obs_len(34, 28, True)
    check_guided_obs_len(28, 28, False)
    with pytest.raises(ValueError, match=r"guidance=True needs a policy with obs_len = env.obs_len \+ 6 = 34, got obs_len = 28"):
        check_guided_obs_len(28, 28, True)
    with pytest.raises(ValueError, match=r"obs_len = 34 is env.obs_len \+ 6 \(env.obs_len = 28\).*pass guidance=True"):
        check_guided_obs_len(34, 28, False)


def _widest_env(monkeypatch, obs_len=130):
    """What the three callers read of a VecReferenceModel at sensor range 5 with goal distance, pressure and mask (obs_len 130,
    guided 136), with no handle behind it; any call into the library from here on fails the test."""
    import torch

    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd.vec_env import VecReferenceModel

    env = VecReferenceModel.__new__(VecReferenceModel)
    env.num_envs, env.num_agents, env.obs_len, env.device = 2, 3, obs_len, torch.device("cpu")
    assert env.guided_obs_len == obs_len + 6

    def no_library(*a, **k):
        raise AssertionError("the library was touched")

    monkeypatch.setattr(L, "load", no_library)
    return env


def test_guidance_on_the_widest_observation_is_refused_by_name_before_the_library(monkeypatch):
    """A guided row of 136 floats is above the policy kernel's 130: Rollout, Trainer and neural_policy say so, with both
    numbers, instead of the refusal of mapf_policy_create."""
    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd.evaluation import neural_policy
    from dl_reference_models_amd.learner import Trainer
    from dl_reference_models_amd.policy import MaskedRecurrentPolicy
    from dl_reference_models_amd.rollout import Rollout, check_guidance_fits, check_guided_obs_len

    with open(os.path.join(ROOT, "include", "mapf_step.h"), encoding="utf-8") as f:
        assert "the longest observation mapf_obs_len can return = 130]" in f.read()
    assert L.POLICY_MAX_OBS_LEN == 130 == (2 * L.MAX_SENSOR_RANGE + 1) ** 2 + 9
    env = _widest_env(monkeypatch)
    module = MaskedRecurrentPolicy(130, has_mask=True)  # the longest a device policy takes; none takes the guided 136
    says = r"env\.obs_len \+ 6 = 136 floats, more than the 130 the policy kernel takes"
    with pytest.raises(ValueError, match=says):
        Rollout(env, None, 4, guidance=True)
    with pytest.raises(ValueError, match=says):
        Trainer(env, module, T=4, guidance=True)
    with pytest.raises(ValueError, match=says):
        neural_policy(env, module, guidance=True)
    with pytest.raises(ValueError, match=says):
        check_guided_obs_len(136, 130, True)
    # the longest guided row that fits, and everything without guidance, passes the check
    check_guidance_fits(124)
    check_guided_obs_len(130, 124, True)
    check_guided_obs_len(130, 130, False)
    with pytest.raises(ValueError, match=r"env\.obs_len \+ 6 = 131 floats, more than the 130"):
        check_guidance_fits(125)
