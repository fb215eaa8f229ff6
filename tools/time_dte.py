#!/usr/bin/env python3
"""What one policy per agent (DTE) costs (a measurement, modelled on tools/time_policy.py and tools/time_learner.py), all in
this process, three alternating rounds each, medians:

    act       one graph of 20 x [mapf_step -> policy] at the headline shape and at the reference's training setup:
                per_agent    the PerAgentPolicy as one launch (a per-agent handle: mapf_policy_create_per_agent)
                other_order  the same launch with the other block order (--other-order-lib: a library built with
                             -DMAPF_POLICY_AGENT_FASTEST=1: agent-fastest; csrc/mapf_policy.hip), when given
                torch        the same PerAgentPolicy composed of torch fp32 ops, batched products over the agent axis
                shared       the shared-weights launch (one MaskedRecurrentPolicy for every row)
                env_only     the env alone
    lstm      learner.lstm_sequence forward plus backward with whh [G, 256, 64] (G = 16), T = 32 at 8 192 and 65 536 rows:
              the grouped kernels, the torch loop with a batched product, and the ungrouped call (whh [256, 64])
    iterate   one Trainer.iterate() in DTE at the training setup, fused against fused=False

One JSON object per line; the raw lines are kept when --out is given.

    python -m dl_reference_models_amd.build --variant full -DMAPF_POLICY_AGENT_FASTEST=1 --out build_diag/libagentfastest.so
    python tools/time_dte.py --other-order-lib build_diag/libagentfastest.so --out profiles/r17/dte/time_dte.jsonl
"""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
from dl_reference_models_amd import learner as ln
from dl_reference_models_amd import workloads as wl
from dl_reference_models_amd.policy import NUM_ACTIONS, DevicePolicy, MaskedRecurrentPolicy, PerAgentPolicy
from dl_reference_models_amd.vec_env import VecReferenceModel

K = 20  # env steps per graph
T = 32
ROUNDS = 3
SIZES = (8192, 65536)
GROUPS = 16
TRAINING = "ref_training_4096x32x32_n16"
DEV = "cuda:0"


def timed_graph(g, reps=30):
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


def timed(fn, reps):
    """ms per call: `reps` calls between two events, after two calls outside them."""
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def make_env(name):
    b, h, w, n, density, _ = wl.WORKLOADS[name]
    cfg = wl.workload_config(name, list(range(b)))
    env = VecReferenceModel(cfg)
    env.reset()
    c = env.get_state()["counters"]
    c[:, 0] = np.arange(b) % int(cfg["steps_per_episode"])  # staggered episode phases, as in bench.py
    env.set_state(counters=c)
    return env, cfg, b, n


@torch.no_grad()
def batched_step(m: PerAgentPolicy, obs, pa, pr, start, state):
    """``PerAgentPolicy.forward`` as batched products over the agent axis: obs [B, N, L], pa / pr / start [B, N], state
    [B, N, 64] each.  Returns logits [B, N, 5], value [B, N] and the new state."""
    def dense(x, name):
        return torch.einsum("bni,noi->bno", x, m.stacked(name + ".weight")) + m.stacked(name + ".bias")

    a2 = torch.tanh(dense(torch.tanh(dense(obs[..., :m.features], "fc1")), "fc2"))
    keep = (start == 0)
    h, c = state[0] * keep[..., None], state[1] * keep[..., None]
    z = torch.cat([a2, torch.nn.functional.one_hot(pa.to(torch.int64) * keep, NUM_ACTIONS).to(a2.dtype), (pr * keep)[..., None]], dim=2)
    g = (torch.einsum("bni,noi->bno", z, m.stacked("lstm.weight_ih")) + torch.einsum("bni,noi->bno", h, m.stacked("lstm.weight_hh"))
         + m.stacked("lstm.bias_ih") + m.stacked("lstm.bias_hh"))
    gi, gf, gg, go = g.split(64, dim=2)
    c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
    h = torch.sigmoid(go) * torch.tanh(c)
    logits = dense(h, "pi")
    if m.has_mask:
        logits = logits + torch.log(obs[..., m.features:] + 1e-6)
    return logits, dense(h, "vf")[..., 0], (h, c)


def run_act(name, other_lib, emit):
    env, cfg, b, n = make_env(name)
    dev, L = env.device, env.obs_len
    has_mask = bool(cfg.get("include_action_mask_in_obs", False))
    torch.manual_seed(0)
    module = PerAgentPolicy(n, L, has_mask=has_mask, recurrent=True)
    R = b * n
    handles = {"per_agent": DevicePolicy(module, R, n, dev), "shared": DevicePolicy(module.agents[0], R, n, dev)}
    if other_lib:
        os.environ["MAPF_LIB"] = os.path.abspath(other_lib)  # read when a handle is created (_lib.library_path)
        handles["other_order"] = DevicePolicy(module, R, n, dev)
        del os.environ["MAPF_LIB"]
    mod = module.to(dev)
    actions = torch.zeros((b, n), dtype=torch.int8, device=dev)
    state = [torch.zeros((b, n, 64), device=dev), torch.zeros((b, n, 64), device=dev)]
    logp, value = handles["per_agent"].logp, handles["per_agent"].value

    def fused(pol):
        def fn(o):
            pol.act_raw(o.data_ptr(), actions.data_ptr(), env._rewards.data_ptr(), env._terminated.data_ptr(),
                        env._truncated.data_ptr(), 0, 0, out=(actions.data_ptr(), logp.data_ptr(), value.data_ptr(), None))
        return fn

    def torch_policy(o):
        start = (env._terminated | env._truncated)[:, None].expand(b, n)
        logits, v, st = batched_step(mod, o.view(b, n, L), actions, env._rewards.view(b, n), start, state)
        state[0].copy_(st[0])
        state[1].copy_(st[1])
        act = torch.argmax(logits, dim=2)
        logp.view(b, n).copy_(torch.log_softmax(logits, dim=2).gather(2, act[..., None])[..., 0])
        value.view(b, n).copy_(v)
        actions.copy_(act.to(torch.int8))

    def env_step():
        return env.step(actions)["obs"]

    policies = {k: fused(p) for k, p in handles.items()}
    policies.update({"torch": torch_policy, "env_only": None})
    for p in policies.values():  # warm up (rocBLAS picks its kernels outside the capture)
        for _ in range(3):
            o = env_step()
            if p is not None:
                p(o)
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
    out = {"section": "act", "workload": name, "envs": b, "agents": n, "rows": R, "obs_floats": L, "steps_per_graph": K,
           "params_per_policy": int(module.agents[0].flat_params().numel())}
    for r in range(ROUNDS):
        for kind, g in graphs.items():
            out[f"{kind}_us_per_step_round{r}"] = timed_graph(g)
    env.poll_error()
    for kind in graphs:
        out[kind + "_us_per_step"] = float(np.median([out[f"{kind}_us_per_step_round{r}"] for r in range(ROUNDS)]))
    for kind in graphs:
        if kind != "env_only":
            out[kind + "_policy_us"] = out[kind + "_us_per_step"] - out["env_only_us_per_step"]
    out["fused_faster_in_every_round"] = all(out[f"per_agent_us_per_step_round{r}"] < out[f"torch_us_per_step_round{r}"] for r in range(ROUNDS))
    out["torch_over_per_agent_policy"] = out["torch_policy_us"] / out["per_agent_policy_us"]
    out["per_agent_over_shared_policy"] = out["per_agent_policy_us"] / out["shared_policy_us"]
    if other_lib:
        out["other_order_over_per_agent_policy"] = out["other_order_policy_us"] / out["per_agent_policy_us"]
    emit(out)
    del graphs
    env.close()


def run_lstm(rows, emit):
    g = torch.Generator(device=DEV).manual_seed(0)
    xg = torch.randn((T, rows, 256), device=DEV, generator=g).requires_grad_(True)
    whh = ((torch.rand((GROUPS, 256, 64), device=DEV, generator=g) - 0.5) / 4).requires_grad_(True)
    whh1 = whh[0].detach().clone().requires_grad_(True)
    reset = (torch.rand((T, rows), device=DEV, generator=g) < 0.05).to(torch.uint8)
    h0 = torch.zeros((rows, 64), device=DEV).requires_grad_(True)
    c0 = torch.zeros((rows, 64), device=DEV).requires_grad_(True)
    dh = torch.randn((T, rows, 64), device=DEV, generator=g)

    def both(w, fused):
        def fn():
            h, _ = ln.lstm_sequence(xg, w, reset, h0, c0, fused=fused)
            torch.autograd.grad((h * dh).sum(), [xg, w, h0, c0])
        return fn

    fns = {"fused": both(whh, True), "torch": both(whh, False), "ungrouped": both(whh1, True)}
    reps = {"fused": 10, "torch": 3, "ungrouped": 10}
    out = {"section": "lstm", "T": T, "rows": rows, "groups": GROUPS}
    for r in range(ROUNDS):
        for kind, fn in fns.items():
            out[f"{kind}_ms_round{r}"] = timed(fn, reps[kind])
    for kind in fns:
        out[kind + "_ms"] = float(np.median([out[f"{kind}_ms_round{r}"] for r in range(ROUNDS)]))
    out["fused_faster_in_every_round"] = all(out[f"fused_ms_round{r}"] < out[f"torch_ms_round{r}"] for r in range(ROUNDS))
    out["torch_over_fused"] = out["torch_ms"] / out["fused_ms"]
    out["grouped_over_ungrouped"] = out["fused_ms"] / out["ungrouped_ms"]
    emit(out)


def run_iterate(emit, iters=3):
    b = wl.WORKLOADS[TRAINING][0]
    cfg = wl.workload_config(TRAINING, list(range(b)))
    for fused in (True, False):
        env = VecReferenceModel(cfg)
        torch.manual_seed(0)
        module = PerAgentPolicy(env.num_agents, env.obs_len, has_mask=False, recurrent=True).to(env.device)
        tr = ln.Trainer(env, module, T=T, learner=ln.PPOLearner(module, fused=fused))
        for _ in range(2):  # the launch and the capture
            tr.iterate()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        ms = []
        for _ in range(iters):
            e0.record()
            tr.iterate()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        env.poll_error()
        emit({"section": "iterate", "workload": TRAINING, "rows": b * env.num_agents, "policies": env.num_agents, "T": T, "fused": fused,
              "epochs": 12, "minibatches": 8, "iterate_ms_rounds": ms, "iterate_ms": float(np.median(ms)),
              "agent_steps_per_s": b * env.num_agents * T / (float(np.median(ms)) * 1e-3)})
        env.close()


if __name__ == "__main__":
    argv = sys.argv[1:]
    path, other, sections = None, None, ("act", "lstm", "iterate")

    def take(flag):
        if flag not in argv:
            return None
        i = argv.index(flag)
        v = argv[i + 1]
        del argv[i:i + 2]
        return v

    path, other = take("--out"), take("--other-order-lib")
    sections = tuple((take("--sections") or "act,lstm,iterate").split(","))
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    sink = open(path, "w", encoding="utf-8") if path else None

    def emit(obj):
        line = json.dumps(obj)
        print(line, flush=True)
        if sink:
            sink.write(line + "\n")
            sink.flush()

    if "act" in sections:
        for nm in (wl.HEADLINE, TRAINING):
            run_act(nm, other, emit)
    if "lstm" in sections:
        for rows in SIZES:
            run_lstm(rows, emit)
    if "iterate" in sections:
        run_iterate(emit)
