"""Time of the rgb_array frame rasteriser (mapf_render) on the device (not a test).  One JSON line per case:

  a  K = 2048 frames of 32x32 cells, 8 agents (the c3 grids), cell_px 8: 402 MB of frames, past the 256 MiB Infinity Cache
  b  K = 64 frames of the c5 shape (64x64 cells, 64 agents, sensor_range 5, lifelong), cell_px 8: the most per-cell work
  c  the drop-in facade's render("rgb_array") on ReferenceModel-2-1 (10x20 cells, 4 agents), end to end per call

    python tools/time_render.py [--cases a b c] [--reps 50] [--out FILE]

(a) and (b): us per launch from device events around `reps` back-to-back launches into one preallocated buffer after a
warm-up, bytes written, GB/s and the share of 8 TB/s.  (c): wall time per call (launch, device->host copy, new array),
median of 5 repetitions of `reps` calls.  MAPF_LIB=<path> times another build of the library (e.g. the nontemporal-store
build)."""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_BPS = 8e12


def time_launches(name, cfg, c, reps):
    import torch

    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd.vec_env import VecReferenceModel

    eng = VecReferenceModel(dict(cfg, device="cuda:0"))
    H, W = eng.grid_shape
    K = eng.num_envs
    out = torch.empty((K, H * c, W * c, 3), dtype=torch.uint8, device=eng.device)
    for _ in range(5):
        eng.render(None, c, out=out)
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        eng.render(None, c, out=out)
    t1.record()
    t1.synchronize()
    eng.poll_error()
    us = t0.elapsed_time(t1) * 1e3 / reps
    nbytes = out.numel()
    line = {"case": name, "shape": [K, H * c, W * c, 3], "K": K, "cell_px": c, "agents": eng.num_agents,
            "sensor_range": eng.sensor_range, "bytes_written": nbytes, "us_per_launch": round(us, 2),
            "GBps": round(nbytes / us * 1e-3, 1), "frac_of_8TBps": round(nbytes / (us * 1e-6) / PEAK_BPS, 3),
            "reps": reps, "timing": "device events around back-to-back launches", "lib": os.path.basename(L.library_path())}
    eng.close()
    return line


def time_facade(reps):
    import numpy as np

    from dl_reference_models_amd import _lib as L
    from dl_reference_models_amd.reference_model_multi_agent import ReferenceModel

    env = ReferenceModel({"env_name": "ReferenceModel-2-1", "num_agents": 4, "sensor_range": 2, "seed": 0})
    env.reset()
    for _ in range(20):
        env.render(mode="rgb_array")
    runs = []
    for _ in range(5):
        t = time.perf_counter()
        for _ in range(reps):
            f = env.render(mode="rgb_array")
        runs.append((time.perf_counter() - t) / reps * 1e3)
    assert f.dtype == np.uint8
    line = {"case": "c_facade_rgb_array", "shape": list(f.shape), "K": 1, "cell_px": 32, "agents": 4, "sensor_range": 2,
            "bytes_written": int(f.nbytes), "ms_per_call": round(statistics.median(runs), 4),
            "ms_per_call_min": round(min(runs), 4), "reps": reps,
            "timing": "host wall clock per call, median of 5 x reps calls (the call ends with the copy to a new array)",
            "lib": os.path.basename(L.library_path())}
    env.close()
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["a", "b", "c"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from dl_reference_models_amd.workloads import workload_config

    lines = []
    for case in args.cases:
        if case == "a":
            lines.append(time_launches("a_2048x32x32_n8_c8", workload_config("c3_8192x32x32_n8", range(2048)), 8, args.reps))
        elif case == "b":
            cfg = workload_config("c5_1024x64x64_n64_lifelong", range(64))
            cfg["sensor_range"] = 5
            lines.append(time_launches("b_64x64x64_n64_sr5_c8", cfg, 8, args.reps))
        elif case == "c":
            lines.append(time_facade(args.reps))
        else:
            raise SystemExit(f"unknown case {case!r}")
        print(json.dumps(lines[-1]), flush=True)
    if args.out:
        with open(args.out, "a") as fh:
            for ln in lines:
                fh.write(json.dumps(ln) + "\n")


if __name__ == "__main__":
    main()
