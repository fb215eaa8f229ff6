#!/usr/bin/env python3
"""What a rollout step costs with the reference's policy between two env steps (a measurement, modelled on
tools/policy_loop.py): one graph of 20 x [mapf_step -> policy] at the headline shape and at the reference's training setup,
in three configurations, all in this process:

    fused     the policy as one launch (DevicePolicy.act: mapf_policy_act)
    torch     the same MaskedRecurrentPolicy composed of torch fp32 ops (greedy action, state carried in place)
    env_only  the env alone (the actions of the last policy run)

Three alternating rounds of the three graphs; then the same for the feed-forward variant; then Rollout.collect() per step.
One JSON object per line; the raw lines are kept under profiles/r11/policy/ when --out is given.

    python tools/time_policy.py [--out profiles/r11/policy/time_policy.jsonl] [workload ...]
"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import DevicePolicy, MaskedRecurrentPolicy
from dl_reference_models_amd.rollout import Rollout
from dl_reference_models_amd.vec_env import VecReferenceModel

K = 20  # env steps per graph
ROUNDS = 3


def timed(g, reps=30):
    for _ in range(3):
        g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        g.replay()
    e1.record()
    torch.cuda.synchronize()
    return 1e3 * e0.elapsed_time(e1) / (reps * K)  # us per env step


def make_env(name):
    b, h, w, n, density, _ = wl.WORKLOADS[name]
    cfg = wl.workload_config(name, list(range(b)))
    env = VecReferenceModel(cfg)
    env.reset()
    c = env.get_state()["counters"]
    c[:, 0] = np.arange(b) % int(cfg["steps_per_episode"])  # staggered episode phases, as in bench.py
    env.set_state(counters=c)
    return env, cfg, b, n


def run(name, recurrent, emit):
    env, cfg, b, n = make_env(name)
    dev, L = env.device, env.obs_len
    has_mask = bool(cfg.get("include_action_mask_in_obs", False))
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(L, has_mask=has_mask, recurrent=recurrent)
    fused = DevicePolicy(module, b * n, n, dev)
    mod = module.to(dev)
    R = b * n
    actions = torch.zeros((b, n), dtype=torch.int8, device=dev)
    state = list(mod.initial_state(R, dev))
    start = torch.zeros((R,), dtype=torch.uint8, device=dev)

    def fused_policy(o):
        fused.act_raw(o.data_ptr(), actions.data_ptr(), env._rewards.data_ptr(), env._terminated.data_ptr(),
                      env._truncated.data_ptr(), 0, 0, out=(actions.data_ptr(), fused.logp.data_ptr(), fused.value.data_ptr(), None))

    @torch.no_grad()
    def torch_policy(o):
        start.view(b, n).copy_((env._terminated | env._truncated)[:, None].expand(b, n))
        logits, value, st = mod(o.view(R, L), actions.view(R), env._rewards.view(R), start, tuple(state) if recurrent else None)
        if recurrent:
            state[0].copy_(st[0])
            state[1].copy_(st[1])
        act = torch.argmax(logits, dim=1)
        fused.logp.copy_(torch.log_softmax(logits, dim=1).gather(1, act[:, None])[:, 0])
        fused.value.copy_(value)
        actions.copy_(act.to(torch.int8).view(b, n))

    def env_step():
        return env.step(actions)["obs"]

    policies = {"fused": fused_policy, "torch": torch_policy, "env_only": None}
    for p in (fused_policy, torch_policy):  # warm up (rocBLAS picks its kernels outside the capture)
        for _ in range(3):
            p(env_step())
    torch.cuda.synchronize()
    graphs = {}
    for kind, p in policies.items():
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(K):
                o = env_step()
                if p is not None:
                    p(o)
        graphs[kind] = g
    out = {"workload": name, "envs": b, "agents": n, "rows": R, "obs_floats": L, "mask": has_mask, "recurrent": recurrent,
           "steps_per_graph": K, "params": int(module.flat_params().numel())}
    for r in range(ROUNDS):
        for kind, g in graphs.items():
            out[f"{kind}_us_per_step_round{r}"] = timed(g)
    env.poll_error()
    for kind in graphs:
        out[kind + "_us_per_step"] = float(np.median([out[f"{kind}_us_per_step_round{r}"] for r in range(ROUNDS)]))
    out["fused_policy_us"] = out["fused_us_per_step"] - out["env_only_us_per_step"]
    out["torch_policy_us"] = out["torch_us_per_step"] - out["env_only_us_per_step"]
    out["fused_faster_in_every_round"] = all(out[f"fused_us_per_step_round{r}"] < out[f"torch_us_per_step_round{r}"] for r in range(ROUNDS))
    out["env_share_of_fused_step"] = out["env_only_us_per_step"] / out["fused_us_per_step"]
    out["env_share_of_torch_step"] = out["env_only_us_per_step"] / out["torch_us_per_step"]
    emit(out)
    del graphs
    env.close()


def run_rollout(name, emit, T=K):
    env, cfg, b, n = make_env(name)
    torch.manual_seed(0)
    module = MaskedRecurrentPolicy(env.obs_len, has_mask=bool(cfg.get("include_action_mask_in_obs", False)), recurrent=True)
    ro = Rollout(env, DevicePolicy(module, b * n, n, env.device), T, sample=True, seed=1)
    for _ in range(4):
        ro.collect()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rounds = []
    for _ in range(ROUNDS):
        e0.record()
        for _ in range(30):
            ro.collect()
        e1.record()
        torch.cuda.synchronize()
        rounds.append(1e3 * e0.elapsed_time(e1) / (30 * T))
    env.poll_error()
    emit({"workload": name, "rollout_T": T, "sample": True, "collect_us_per_step_rounds": rounds,
          "collect_us_per_step": float(np.median(rounds)), "agent_steps_per_s": b * n / (float(np.median(rounds)) * 1e-6)})
    env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = None
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    sink = open(path, "w", encoding="utf-8") if path else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    names = argv or [wl.HEADLINE, "ref_training_4096x32x32_n16"]
    for rec in (True, False):
        for nm in names:
            run(nm, rec, emit)
    for nm in names:
        run_rollout(nm, emit)
