"""Time of the evaluation trace (mapf_eval_trace, mapf_render_words, evaluation.Trace) on the device (not a test).  One
JSON line per case:

  evaluate  evaluate(env, "random", 4) end to end (host wall clock, records copied back) on 8192 envs of the headline shape
            (32x32, 8 agents) and of the single-agent env (16x16, 4 agents): without a trace, with K = 8 traced envs and
            with K = B, `--rounds` alternating rounds in one process.  `--root DIR` imports the package from another
            checkout (the parent commit built next to this one: its evaluate in the same session is the baseline) and
            times the untraced case only.  Under `rocprofv3 --kernel-trace --stats` the same process gives k_eval_trace
            per launch next to k_eval_record, and the kernel count per step with and without a trace.
  render    2048 frames of 256 x 256 (32x32 cells, 8 agents, cell_px 8: the shape of DESIGN.md 4f): us per launch of
            mapf_render and of mapf_render_words over the same states, alternating rounds, device events around `reps`
            back-to-back launches into one preallocated buffer.
  video     a 5-episode video of ReferenceModel-2-1 (10x20 cells, 4 agents, 256-step episodes, cell_px 32: 640 x 320
            frames) end to end: traced evaluation, render chunks, GIF; next to the per-object facade loop that renders
            every frame as main.py does (frames kept in a list, not encoded).

    python tools/time_eval_trace.py [--cases evaluate render video] [--rounds 3] [--reps 50] [--root DIR] [--out FILE]
"""

from __future__ import annotations

import argparse
import json
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

WORKLOADS = (("c3_8192x32x32_n8", False), ("cte_8192x16x16_n4", True))


def _make(name, single, B):
    from dl_reference_models_amd.vec_env import VecReferenceModel
    from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel
    from dl_reference_models_amd.workloads import workload_config

    return (VecSingleAgentReferenceModel if single else VecReferenceModel)(dict(workload_config(name, range(B)), device="cuda:0"))


def time_evaluate(rounds, modes):
    import torch

    from dl_reference_models_amd import evaluation as evm

    lines = []
    for name, single in WORKLOADS:
        B, E = 8192, 4
        wall = {m: [] for m in modes}
        for _ in range(rounds):
            for m in modes:
                env = _make(name, single, B)
                kw = {} if m == "none" else {"trace": evm.TraceSpec(range(8) if m == "k8" else range(B), E)}
                torch.cuda.synchronize()
                t = time.perf_counter()
                out = evm.evaluate(env, "random", E, **kw)
                if m != "none":
                    out[2].host_words()  # (the trace copied back too)
                wall[m].append(round(time.perf_counter() - t, 4))
                env.close()
        res = out[0]
        lines.append({"case": "evaluate_" + name, "episodes": len(res["env"]), "env_steps": int(res["timesteps"].sum()),
                      "wall_s": wall, "wall_s_best": {m: min(v) for m, v in wall.items()}, "rounds": rounds,
                      "package": os.path.dirname(evm.__file__)})
    return lines


def time_render(rounds, reps):
    import torch

    from dl_reference_models_amd.device_net import ptr
    from dl_reference_models_amd.vec_env import VecReferenceModel
    from dl_reference_models_amd.workloads import workload_config

    K, c = 2048, 8
    eng = VecReferenceModel(dict(workload_config("c3_8192x32x32_n8", range(K)), device="cuda:0"))
    H, W = eng.grid_shape
    out = torch.empty((K, H * c, W * c, 3), dtype=torch.uint8, device=eng.device)
    st = eng.get_state()
    p, g = st["positions"].astype("uint32"), st["goals"].astype("uint32")
    words = torch.from_numpy((p[..., 1] | p[..., 0] << 8 | g[..., 1] << 16 | g[..., 0] << 24).astype("uint32").view("int32")).to(eng.device)
    ids = torch.arange(K, dtype=torch.int32, device=eng.device)

    def live():
        eng.render(None, c, out=out)

    def from_words():
        eng._check(eng._lib.mapf_render_words(eng._h, ptr(words), None, ptr(ids), K, c, ptr(out), eng._stream()))

    def events(fn):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for _ in range(reps):
            fn()
        t1.record()
        t1.synchronize()
        return round(t0.elapsed_time(t1) * 1e3 / reps, 2)

    live()
    want = out.clone()
    from_words()
    same = bool(torch.equal(out, want))
    for _ in range(5):
        live()
        from_words()
    torch.cuda.synchronize()
    us = {"mapf_render": [], "mapf_render_words": []}
    for _ in range(rounds):
        us["mapf_render"].append(events(live))
        us["mapf_render_words"].append(events(from_words))
    eng.poll_error()
    eng.close()
    return [{"case": "render_2048x256x256", "bytes_written": out.numel(), "us_per_launch": us, "frames_equal": same,
             "spread_us": {k: round(max(v) - min(v), 2) for k, v in us.items()}, "rounds": rounds, "reps": reps,
             "timing": "device events around back-to-back launches"}]


def time_video():
    import numpy as np
    import torch

    from dl_reference_models_amd import evaluation as evm
    from dl_reference_models_amd.reference_model_multi_agent import ReferenceModel
    from dl_reference_models_amd.vec_env import VecReferenceModel

    cfg = {"env_name": "ReferenceModel-2-1", "num_agents": 4, "sensor_range": 2, "steps_per_episode": 256, "seed": 0}
    E = 5
    with tempfile.TemporaryDirectory() as tmp:
        env = VecReferenceModel(dict(cfg, num_envs=1, device="cuda:0"))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res, _heat, trace = evm.evaluate(env, "random", E, trace=evm.TraceSpec([0], E))
        t1 = time.perf_counter()
        frames = sum(len(chunk) for chunk in trace.video_chunks(hold=3, cell_px=32))
        t2 = time.perf_counter()
        n = trace.write_gif(os.path.join(tmp, "v.gif"), fps=5, hold=3, cell_px=32)
        t3 = time.perf_counter()
        size = os.path.getsize(os.path.join(tmp, "v.gif"))
        env.close()
    # the per-object loop: main.py's, a frame after the reset and after every step
    rng = np.random.default_rng(0)
    fenv = ReferenceModel(dict(cfg))
    t4 = time.perf_counter()
    kept = []
    for _ep in range(E):
        obs, _ = fenv.reset()
        kept.append(fenv.render(mode="rgb_array"))
        done = False
        while not done:
            obs, _r, term, trunc, _i = fenv.step({a: int(rng.integers(0, 5)) for a in obs})
            done = bool(term["__all__"] or trunc["__all__"])
            kept.append(fenv.render(mode="rgb_array"))
    t5 = time.perf_counter()
    fenv.close()
    return [{"case": "video_2_1_n4_5x256", "frames": frames, "gif_frames": n, "gif_bytes": size, "frame_shape": list(kept[0].shape),
             "env_steps": int(res["timesteps"].sum()), "traced_evaluate_s": round(t1 - t0, 3), "render_chunks_to_host_s": round(t2 - t1, 3),
             "write_gif_s": round(t3 - t2, 3), "facade_loop_s": round(t5 - t4, 3), "facade_frames": len(kept)}]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="*", default=["evaluate", "render", "video"])
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--modes", nargs="*", default=["none", "k8", "kB"], help="evaluate: none (no trace), k8, kB")
    ap.add_argument("--root", default=None, help="import dl_reference_models_amd from this checkout (baseline: evaluate without a trace only)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root) if args.root else ROOT)
    for case in args.cases:
        if case == "evaluate":
            lines = time_evaluate(args.rounds, ["none"] if args.root else args.modes)
        elif case == "render":
            lines = time_render(args.rounds, args.reps)
        elif case == "video":
            lines = time_video()
        else:
            raise SystemExit(f"unknown case {case!r}")
        for line in lines:
            print(json.dumps(line), flush=True)
            if args.out:
                with open(args.out, "a") as fh:
                    fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
