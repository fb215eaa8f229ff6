"""bench.py end to end: a plain run times the headline leg only, `--full` adds the secondary measurements, and
`--dump-outputs` writes what the headline leg's last timed step returned -- the same arrays whichever of the two runs."""

from __future__ import annotations

import json
import os
import subprocess
import sys

import numpy as np
import pytest

from trace_util import ROOT

pytestmark = pytest.mark.gpu


def _bench(out, *extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "c2_1024x16x16_n4",
                        "--steps", "30", "--warmup", "5", "--dump-outputs", str(out), *extra],
                       capture_output=True, text=True, timeout=600, env={k: v for k, v in os.environ.items() if k != "RANK"})
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0]), {f[:-4]: np.load(os.path.join(out, f)) for f in os.listdir(out)}


def test_plain_and_full_runs_dump_the_same_last_step(tmp_path):
    plain, dp = _bench(tmp_path / "plain")
    full, df = _bench(tmp_path / "full", "--full", "--cpu-seconds", "0.5")
    for d in (plain, full):
        assert d["steps"] == 30 and d["warmup"] == 5 and d["ms_per_step"] > 0
        assert d["value"] == pytest.approx(1024 * 4 * 1e3 / d["ms_per_step"])
        assert d["config"]["episode_phases"] == "staggered"
    assert "value_synchronised" not in plain and "cpu_baseline" not in plain and plain["per_call_ms"] is None
    assert full["value_synchronised"] > 0 and full["per_call_ms"] > 0 and full["cpu_baseline"]["value"] > 0
    assert sorted(dp) == ["info_agent", "info_all", "obs", "rewards", "terminated", "truncated"]
    assert dp["obs"].shape == (1024, 4, plain["config"]["obs_floats"]) and dp["info_all"].shape == (1024, 14)
    assert all(a.dtype in (np.float32, np.float64) for a in dp.values())
    assert sorted(df) == sorted(dp)
    for k in dp:
        np.testing.assert_array_equal(dp[k], df[k], err_msg=k)
