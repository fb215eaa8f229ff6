#!/usr/bin/env python3
"""What a rollout step of the single-agent env costs with the joint-action policy between two env steps (a measurement,
the method of tools/time_policy.py): one graph of 20 x [mapf_cte_step -> policy] in three configurations, all in this
process:

    fused     the policy as one launch (JointDevicePolicy.act_raw: mapf_jpolicy_act)
    torch     the same JointActionPolicy composed of torch fp32 ops (greedy action, state carried in place)
    env_only  the env alone (the actions of the last policy run)

Three alternating rounds of the three graphs, medians; then JointRollout.collect() per step; then, with --learner, one
Trainer.iterate() with the fused recurrence and with the torch loop.  A shape is a single-agent workload name or
BxHxWxN (synthetic grids at density 0.2).  One JSON object per line; the raw lines are kept when --out is given.

--hidden 256 times the wide feed-forward net (the reference's CTE IMPALA model) the same way, prints the matrix-rate floor
(the line's gflop at 157 TF, the f32-input MFMA) and the traffic floor (its obs_mbytes at 8 TB/s) with it, and ends with
one Trainer.iterate() under the reference's IMPALA settings instead of --learner's PPO pair.

    python tools/time_joint_policy.py [--out FILE] [--learner] [--hidden 256] [shape ...]
"""
import json, os, sys, time
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.learner import IMPALALearner, PPOLearner, Trainer
from dl_reference_models_amd.policy import JointActionPolicy, JointDevicePolicy
from dl_reference_models_amd.rollout import JointRollout
from dl_reference_models_amd.vec_env_single_agent import VecSingleAgentReferenceModel

K = 20  # env steps per graph
ROUNDS = 3
DEFAULT_SHAPES = ("cte_8192x16x16_n4", "cte_1024x32x32_n8", "8192x32x32x16")
WIDE = 256
MATRIX_TFLOPS, HBM_TBYTES = 157.0, 8.0  # the floors' rates: v_mfma_f32_32x32x2_f32, HBM


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
    if name in wl.WORKLOADS:
        b, h, w, n, density, _ = wl.WORKLOADS[name]
        cfg = wl.workload_config(name, list(range(b)))
    else:
        b, h, w, n = (int(x) for x in name.split("x"))
        cfg = dict(wl.workload_config("cte_8192x16x16_n4", [0]), num_agents=n, num_envs=b, seeds=list(range(b)),
                   grid=wl.synthetic_grids(range(b), h, w, 0.2, n))
    env = VecSingleAgentReferenceModel(cfg)
    env.reset()
    env.set_step_counts(np.arange(b) % int(env.steps_per_episode))  # staggered episode phases, as in bench.py
    return env, b, h, w, n


def run(name, emit, hidden=64):
    env, b, h, w, n = make_env(name)
    dev, L = env.device, env.obs_len
    torch.manual_seed(0)
    recurrent = hidden != WIDE  # the wide net is feed-forward
    module = JointActionPolicy(h * w, n, recurrent=recurrent, hidden=hidden)
    fused = JointDevicePolicy(module, b, dev)
    mod = module.to(dev)
    actions = torch.zeros((b, n), dtype=torch.int8, device=dev)
    state = list(mod.initial_state(b, dev))

    def fused_policy(o):
        fused.act_raw(o.data_ptr(), actions.data_ptr(), env._reward.data_ptr(), env._terminated.data_ptr(),
                      env._truncated.data_ptr(), 0, 0, out=(actions.data_ptr(), fused.logp.data_ptr(), fused.value.data_ptr(), None))

    @torch.no_grad()
    def torch_policy(o):
        if recurrent:
            logits, value, st = mod(o, actions, env._reward, env._terminated | env._truncated, tuple(state))
            state[0].copy_(st[0])
            state[1].copy_(st[1])
        else:
            logits, value, _ = mod(o)
        lg = logits.view(b, n, 5)
        act = torch.argmax(lg, dim=2)
        fused.logp.copy_(torch.log_softmax(lg, dim=2).gather(2, act[..., None])[..., 0].sum(dim=1))
        fused.value.copy_(value)
        actions.copy_(act.to(torch.int8))

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
    out = {"shape": name, "hidden": hidden, "recurrent": recurrent, "envs": b, "grid": [h, w], "agents": n, "obs_floats": L,
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
    out["obs_mbytes"] = 4e-6 * b * L
    if recurrent:
        out["gflop"] = 2e-9 * b * (64 * h * w + 64 * 64 + 256 * (64 + 5 * n + 1 + 64) + (5 * n + 1) * 64)
    else:
        out["gflop"] = 2e-9 * b * (hidden * h * w + hidden * hidden + (5 * n + 1) * hidden)
        out["matrix_floor_us"] = 1e-3 * out["gflop"] / MATRIX_TFLOPS * 1e6
        out["traffic_floor_us"] = out["obs_mbytes"] / HBM_TBYTES
    emit(out)
    del graphs
    # JointRollout.collect() per step, sampling
    env.reset()
    ro = JointRollout(env, fused, K, sample=True, seed=1)
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
        rounds.append(1e3 * e0.elapsed_time(e1) / (30 * K))
    env.poll_error()
    med = float(np.median(rounds))
    emit({"shape": name, "hidden": hidden, "rollout_T": K, "sample": True, "collect_us_per_step_rounds": rounds, "collect_us_per_step": med,
          "env_share_of_collect": out["env_only_us_per_step"] / med, "env_steps_per_s": b / (med * 1e-6)})
    env.close()


def run_learner(name, emit, T=32, iters=3):
    for fused in (True, False):
        env, b, h, w, n = make_env(name)
        torch.manual_seed(0)
        module = JointActionPolicy(h * w, n, recurrent=True).to(env.device)
        learner = PPOLearner(module, lr=1e-4, clip=0.2, vf_coeff=1.0, ent_coeff=0.01, epochs=10, minibatches=8, fused=fused)
        trainer = Trainer(env, module, T=T, learner=learner)
        secs = []
        for _ in range(iters + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            trainer.iterate()
            secs.append(time.perf_counter() - t0)
        emit({"shape": name, "learner_fused": fused, "T": T, "epochs": 10, "minibatches": 8, "iterate_seconds": secs[1:],
              "first_iterate_seconds": secs[0], "iterate_seconds_median": float(np.median(secs[1:]))})
        env.close()


def run_impala(name, emit, T=32, iters=3):
    """One Trainer.iterate() of the wide net under the reference's CTE IMPALA settings (src/agents/impala.py:16-51)."""
    env, b, h, w, n = make_env(name)
    torch.manual_seed(0)
    module = JointActionPolicy(h * w, n, recurrent=False, hidden=WIDE).to(env.device)
    learner = IMPALALearner(module, lr=1e-3, vf_coeff=0.3, ent_coeff=0.001, gamma=0.99)
    trainer = Trainer(env, module, T=T, learner=learner)
    secs = []
    for _ in range(iters + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        trainer.iterate()
        secs.append(time.perf_counter() - t0)
    emit({"shape": name, "hidden": WIDE, "learner": "IMPALA", "T": T, "epochs": 1, "minibatches": 8, "iterate_seconds": secs[1:],
          "first_iterate_seconds": secs[0], "iterate_seconds_median": float(np.median(secs[1:]))})
    env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path = None
    hidden = 64
    if "--hidden" in argv:
        i = argv.index("--hidden")
        hidden = int(argv[i + 1])
        del argv[i:i + 2]
        if hidden not in (64, WIDE):
            sys.exit(f"--hidden must be 64 or {WIDE}")
    if "--out" in argv:
        i = argv.index("--out")
        path = argv[i + 1]
        del argv[i:i + 2]
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    learner = "--learner" in argv
    argv = [a for a in argv if a != "--learner"]
    sink = open(path, "w", encoding="utf-8") if path else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    names = argv or list(DEFAULT_SHAPES)
    for nm in names:
        run(nm, emit, hidden)
    if hidden == WIDE:
        run_impala(names[0], emit)
    elif learner:
        run_learner(names[0], emit)
