"""Evaluation records without a GPU: the NumPy restatement of the recorder kernel on top of the CPU oracle (eval_util)
against the fixtures recorded from the reference's own test-mode loop (tools/gen_eval_golden.py), every array, exactly;
and the host side of dl_reference_models_amd.evaluation -- the result table, its column order, the CSV."""

import csv

import numpy as np
import pytest

import eval_util as eu


@pytest.mark.parametrize("name", eu.EVAL_FIXTURES)
def test_oracle_recorder_reproduces_reference_fixture(name):
    fx = eu.load_eval_fixture(name)
    got = eu.run_oracle_eval(fx["grids"], fx["config"], fx["E"], rng_words=fx["rng_words"], actions=fx["actions"],
                             fixed_starts=fx["ctor_starts"], fixed_goals=fx["ctor_goals"])
    eu.assert_records_equal(got, fx, name)
    assert got["launches"] == int(fx["env_steps"].max()) == fx["actions"].shape[0]
    assert np.array_equal(fx["timesteps"].sum(axis=1), fx["env_steps"])
    # one visit per agent and step, nothing lost and nothing counted twice
    assert np.array_equal(got["heat"].sum(axis=(1, 2)), fx["env_steps"].astype(np.int64) * fx["config"]["num_agents"])


def test_first_fixture_has_both_endings_and_envs_that_idle():
    fx = eu.load_eval_fixture(eu.EVAL_FIXTURES[0])
    assert (fx["terminated"] & ~fx["truncated"]).any() and fx["truncated"].any()
    assert len(set(fx["env_steps"].tolist())) > 1  # envs finish at different launches


def test_greedy_stream_of_the_restatement_replays():
    fx = eu.load_eval_fixture(eu.EVAL_FIXTURES[0])
    a = eu.run_oracle_eval(fx["grids"], fx["config"], 3, seeds=fx["seeds"], greedy=0.9)
    b = eu.run_oracle_eval(fx["grids"], fx["config"], 3, seeds=fx["seeds"], actions=a["actions"])
    eu.assert_records_equal(a, b)
    for k in a["state"]:
        assert np.array_equal(a["state"][k], b["state"][k]), k


@pytest.mark.parametrize("name", eu.EVAL_FIXTURES)
def test_results_table_columns_and_values(name):
    from dl_reference_models_amd import evaluation as ev

    fx = eu.load_eval_fixture(name)
    lifelong = bool(fx["config"].get("lifelong_mapf", False))
    N, E = fx["config"]["num_agents"], fx["E"]
    table = ev.results_table(eu.results_from_dense(fx, fx["seeds"]), lifelong=lifelong)
    assert len(table) == fx["timesteps"].size
    for m, row in enumerate(table):
        b, k = divmod(m, E)
        assert list(row.keys()) == fx["columns"] == ev.table_columns(N, lifelong)
        assert (row["env"], row["episode"], row["seed"]) == (b, k + 1, int(fx["seeds"][b]))
        assert row["timesteps"] == fx["timesteps"][b, k] and row["total_reward"] == fx["total_reward"][b, k]
        if lifelong:
            for col in ("goals_reached_total", "throughput", "completion_ratio"):
                assert row[col] == fx[col][b, k], (col, b, k)  # float64, exactly
        for i in range(N):
            assert row[f"agent_{i}_reward"] == fx["agent_reward"][b, k, i]
            assert [row[f"agent_{i}_start_x"], row[f"agent_{i}_start_y"]] == fx["starts"][b, k, i].tolist()  # _x is the ROW
            assert [row[f"agent_{i}_goal_x"], row[f"agent_{i}_goal_y"]] == fx["goals"][b, k, i].tolist()
    s = ev.summary(eu.results_from_dense(fx, fx["seeds"]), lifelong=lifelong)
    assert s["average reward"] == fx["total_reward"].sum() / fx["timesteps"].size
    assert s["average timesteps"] == fx["timesteps"].sum() / fx["timesteps"].size
    if lifelong:
        assert s["success rate"] == float(np.mean(fx["completion_ratio"]))
    else:
        assert s["success rate"] == float(np.mean((fx["terminated"] & ~fx["truncated"]).astype(np.float64)))


def test_csv_round_trip(tmp_path):
    from dl_reference_models_amd import evaluation as ev

    fx = eu.load_eval_fixture("ge_eval_2_1_n4_lifelong")
    table = ev.results_table(eu.results_from_dense(fx, fx["seeds"]), lifelong=True)
    path = tmp_path / "results.csv"
    ev.write_results_csv(path, table)
    with open(path, newline="", encoding="utf-8") as f:
        rd = csv.DictReader(f)
        assert rd.fieldnames == fx["columns"]
        rows = list(rd)
    assert len(rows) == len(table)
    for got, want in zip(rows, table):
        for k, v in want.items():
            assert type(v)(got[k]) == v, (k, got[k], v)
    ev.write_results_csv(tmp_path / "empty.csv", [])
    assert (tmp_path / "empty.csv").read_text() == ""


def test_evaluator_rejects_what_it_cannot_run():
    from dl_reference_models_amd import evaluation as ev

    with pytest.raises(TypeError):
        ev.Evaluator(object(), 2)
