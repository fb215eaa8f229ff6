"""The learners on the rollout slabs: ``Rollout.collect()`` -> ``gae`` -> ``PPOLearner.update`` -> ``DevicePolicy.load_params``.

    env = VecReferenceModel({..., "num_envs": 4096})
    module = MaskedRecurrentPolicy(env.obs_len, has_mask=..., recurrent=True).to(env.device)
    trainer = Trainer(env, module, T=32, learner=PPOLearner(module))
    for it in range(200):
        print(trainer.iterate())
    module.save("policy.pt")     # scripts/evaluate_multi_agent_env.py --policy NEURAL --checkpoint policy.pt

Everything here is written once, on ``fragment_view``: a fragment as R sequences of T steps (``obs`` [T, R, L], ``actions``
[T, R, heads], the per-step numbers [T, R], the state before step 0 [R, 64]), each row with ``heads`` five-way heads, the rows
dealt to ``groups`` independent nets, minibatches drawn over ``units``:

    fragment, module                                  R              heads   groups   units
    multi-agent [T, B, N, L], MaskedRecurrentPolicy   B N            1       1        the B N rows
    single-agent [T, B, L], JointActionPolicy         B              N       1        the B rows
    multi-agent [T, B, N, L], PerAgentPolicy          B N (b N + a)  1       N        the B envs (unit u: rows u N .. u N + N - 1)
    multi-agent [T, B, N, L], PopulationPolicy        B N (b N + a)  1       P N      B / P runs of P envs, one of every member

A row's log-probability is the sum over its heads and its entropy the sum of their entropies (RLlib's MultiCategorical).
With a ``PerAgentPolicy`` (the reference's DTE mode, src/agents/ppo.py:77-88) PPO is N independent learners in one: a
minibatch is whole envs, so every policy sees the same number of sequences; the dense layers are batched products over the
agent axis (``PerAgentPolicy.dense``), the recurrence one grouped launch; advantages are standardised, every loss term
averaged and the gradient clipped per policy, and the optimised scalar is the sum of the N totals -- the parameters are
disjoint and Adam is elementwise, so one optimizer over all of them is N optimizers.  IMPALA, DQN and the joint policy do
not take a ``PerAgentPolicy`` (DTE is out of scope there) and say so.  With a ``PopulationPolicy`` (P shared policies on one
env handle, env b with member b % P; population.py) PPO is P independent learners in one by the same rule, "policy" read as
"member" -- a member owns N of the P N groups -- and with per-member hyperparameters (``PPOLearner.set_hyper``).

Inside a learner only the LSTM recurrence is sequential in t.  ``sequence_forward`` evaluates fc1 / fc2, the input half of
the gates (W_ih z + b) and the heads for all T at once and leaves the recurrence to ``lstm_sequence``: on the GPU one launch
forward and one backward over the whole fragment (``mapf_lstm_seq_forward_grouped`` / ``_backward_grouped``; include/mapf_step.h
states the rule), or -- ``fused=False``, the baseline -- the same rule as a loop of torch ops.  The kernels are GPU kernels:
tensors on the CPU always take the loop.  On the GPU ``fused=True`` needs the built library; there is no fallback.
The part before the recurrence (fc1 / fc2, the one-hot, W_ih z + b) is ``dense_trunk``: torch ops by default, or --
``fused_trunk=True`` of the three learners and of ``sequence_forward``, opt-in, a ``MaskedRecurrentPolicy`` only -- one launch
forward and one backward over the minibatch's [T * R'] rows (``mapf_trunk_forward`` / ``mapf_trunk_backward``).
The sums over rows behind both -- dW_hh of the recurrence, the trunk's weight and bias gradients -- are GEMMs and column sums
by default, or -- ``fused_grads=True``, opt-in, wherever ``fused`` / ``fused_trunk`` are accepted -- one split-row reduction
each (``mapf_lstm_seq_param_grad`` with ``fused``, any module; ``mapf_trunk_param_grad`` with ``fused_trunk``).

PPO's defaults are the reference's multi-agent settings (src/agents/ppo.py:104-117): lr 1e-3, clip 0.05, vf_coeff 0.5,
ent_coeff 0.001, 12 epochs, gamma 0.99, lambda 0.95; vf_clip is RLlib's 10.  The reference also runs with RLlib's adaptive KL
penalty (kl_coeff 0.2, kl_target 0.01), which is opt-in here: ``PPOLearner(..., kl_coeff=0.2)`` adds ``kl_coeff *
KL(behaviour || current)`` to the loss, needs the behaviour logits in the fragment (``Rollout(..., keep_logits=True)``,
which ``Trainer`` sets) and adapts the coefficient on the device after every update; ``ppo_objective`` states the whole
objective in torch ops, ``mapf_ppo_loss`` evaluates it and its gradients with respect to logits and values in one launch
(``_PPOLoss``, ``fused_objective``).

IMPALA is the second chain: ``collect()`` -> ``IMPALALearner.update`` -> ``load_params`` every ``push_every`` iterations.
There is no ``gae`` step: the V-trace targets are recomputed from the current network in every minibatch (``vtrace`` states
the rule in torch ops; on the GPU ``mapf_vtrace_loss`` evaluates targets, loss terms and their gradients with respect to
logits and values in one launch, ``_VtraceLoss``).  Its defaults are the reference's multi-agent IMPALA settings
(src/agents/impala.py:94-108) over RLlib's: lr 1e-3, vf_coeff 0.5, ent_coeff 0, grad_clip 40, one epoch, gamma 0.99,
lambda 1, all three V-trace thresholds 1.

Behaviour cloning is the third: ``Rollout(expert=...).collect()`` -> ``BCLearner.update`` -> ``load_params``.  The rollout
labels every step with the action of one of the device planners (``expert_actions`` in the fragment) and the learner
minimises the negative log-likelihood of those labels under the current network (``bc_objective`` states the objective in
torch ops, ``mapf_bc_loss`` evaluates it and its gradients in one launch, ``_BCLoss``); with ``vf_coeff > 0`` the value head
is regressed to ``gae``'s targets as well, so that PPO can start from the cloned checkpoint.  ``Trainer`` walks the DAgger
mixing share ``beta`` (how many steps execute the expert's action instead of the policy's) along the learner's schedule.
"""

from __future__ import annotations

import dataclasses
import math

import torch

from . import _lib as L
from .device_net import f32c, ptr, stream_of
from .dqn import epsilon_at
from .policy import (HIDDEN, MASK_EPS, NUM_ACTIONS, DevicePolicy, JointDevicePolicy, MaskedRecurrentPolicy, PerAgentPolicy,
                     PopulationPolicy)
from .rollout import JointRollout, Rollout, check_expert, check_guidance_fits

GATES = 4 * HIDDEN
FRAGMENT_KEYS = ("obs", "actions", "logp", "value", "rewards", "terminated", "truncated", "first", "h0", "c0", "last_value",
                 "prev_action0", "prev_rewards")


# ---- the recurrence --------------------------------------------------------------------------------------------------------
def _lstm_loop(xg, whh, reset, h0, c0):
    """The rule of ``lstm_sequence`` in elementary torch ops, one step at a time."""
    h, c, hs = h0, c0, []
    grouped = whh.dim() == 3  # [G, 256, 64]: row r recurs through whh[r % G], one batched product per step
    wt = whh.transpose(1, 2) if grouped else whh.t()
    for t in range(xg.shape[0]):
        if reset is not None:
            keep = (reset[t] == 0).to(xg.dtype)[:, None]
            h, c = h * keep, c * keep
        if grouped:
            G = whh.shape[0]
            g = xg[t] + torch.bmm(h.reshape(-1, G, HIDDEN).transpose(0, 1), wt).transpose(0, 1).reshape(-1, GATES)
        else:
            g = xg[t] + h @ wt
        gi, gf, gg, go = g.split(HIDDEN, dim=1)
        c = torch.sigmoid(gf) * c + torch.sigmoid(gi) * torch.tanh(gg)
        h = torch.sigmoid(go) * torch.tanh(c)
        hs.append(h)
    return torch.stack(hs), h, c


class _LstmSequence(torch.autograd.Function):
    @staticmethod
    def forward(ctx, xg, whh, reset, h0, c0, fused_grads=False):
        lib = L.load()
        T, R = int(xg.shape[0]), int(xg.shape[1])
        xg, whh, h0, c0 = f32c(xg), f32c(whh), f32c(h0), f32c(c0)
        h = torch.empty((T, R, HIDDEN), dtype=torch.float32, device=xg.device)
        c = torch.empty_like(h)
        gates = torch.empty((T, R, GATES), dtype=torch.float32, device=xg.device)
        stream = stream_of(xg.device)
        groups = int(whh.shape[0]) if whh.dim() == 3 else 1  # (one matrix is the one-group case of the same kernels)
        rc = lib.mapf_lstm_seq_forward_grouped(T, R, groups, ptr(xg), ptr(whh), ptr(reset), ptr(h0), ptr(c0), ptr(h), ptr(c),
                                               ptr(gates), stream)
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_lstm_seq_forward_grouped failed (code {rc})")
        ctx.save_for_backward(whh, reset, h0, c0, h, c, gates)
        ctx.fused_grads = bool(fused_grads)
        ctx.set_materialize_grads(False)  # an unused final state arrives as None and is passed on as NULL (zeros)
        return h, h[-1].clone(), c[-1].clone()

    @staticmethod
    def backward(ctx, dh, dhT, dcT):
        whh, reset, h0, c0, h, c, gates = ctx.saved_tensors
        lib = L.load()
        T, R = int(h.shape[0]), int(h.shape[1])
        dh = torch.zeros_like(h) if dh is None else f32c(dh)
        dhT = None if dhT is None else f32c(dhT)
        dcT = None if dcT is None else f32c(dcT)
        need_xg, need_w, need_h0, need_c0 = (ctx.needs_input_grad[i] for i in (0, 1, 3, 4))
        dxg = torch.empty_like(gates)
        dh0 = torch.empty_like(h0) if need_h0 else None
        dc0 = torch.empty_like(c0) if need_c0 else None
        stream = stream_of(h.device)
        groups = int(whh.shape[0]) if whh.dim() == 3 else 1
        rc = lib.mapf_lstm_seq_backward_grouped(T, R, groups, ptr(whh), ptr(reset), ptr(c0), ptr(c), ptr(gates), ptr(dh), ptr(dhT),
                                                ptr(dcT), ptr(dxg), ptr(dh0), ptr(dc0), stream)
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_lstm_seq_backward_grouped failed (code {rc})")
        dwhh = None
        if need_w and ctx.fused_grads:
            # the same sum in one split-row reduction: hprev is formed in the kernel from h, h0 and reset
            dwhh = torch.empty((groups, GATES, HIDDEN), dtype=torch.float32, device=h.device)
            ws = _grad_workspace(lib, T * R, 0, 0, groups, h.device)
            rc = lib.mapf_lstm_seq_param_grad(T, R, groups, ptr(dxg), ptr(h), ptr(h0), ptr(reset), ptr(dwhh), ptr(ws), ws.numel(), stream)
            if rc != L.MAPF_OK:
                raise RuntimeError(f"mapf_lstm_seq_param_grad failed (code {rc})")
            dwhh = dwhh if whh.dim() == 3 else dwhh[0]
        elif need_w:
            # dW_hh = sum_t dxg_t^T hprev_t: one GEMM over [T * R]; hprev is h0 / h[:-1], zero where the step was reset
            hprev = torch.empty_like(h)
            hprev[0].copy_(h0)
            if T > 1:
                hprev[1:].copy_(h[:-1])
            if reset is not None:
                hprev.mul_((reset == 0).to(torch.float32)[:, :, None])
            if whh.dim() == 3:  # [T * R / G, G, .]: one batched GEMM, a group's rows with its own matrix
                dwhh = torch.bmm(dxg.view(-1, groups, GATES).permute(1, 2, 0), hprev.view(-1, groups, HIDDEN).transpose(0, 1))
            else:
                dwhh = dxg.view(T * R, GATES).t() @ hprev.view(T * R, HIDDEN)
        return (dxg if need_xg else None), dwhh, None, dh0, dc0, None


def _grad_workspace(lib, rows: int, F: int, recurrent: int, groups: int, device):
    """The workspace of ``mapf_trunk_param_grad`` (groups = 0) / ``mapf_lstm_seq_param_grad`` from torch's caching allocator
    (whose blocks are aligned far beyond the 16 bytes asked for)."""
    size = int(lib.mapf_param_grad_workspace_bytes(int(rows), int(F), int(recurrent), int(groups)))
    if size <= 0:
        raise RuntimeError(f"mapf_param_grad_workspace_bytes refused rows={rows}, F={F}, recurrent={recurrent}, groups={groups}")
    return torch.empty(size, dtype=torch.uint8, device=device)


def _check_sequence_args(xg, whh, reset, h0, c0):
    if xg.dim() != 3 or xg.shape[2] != GATES or xg.shape[0] < 1 or xg.shape[1] < 1:
        raise ValueError(f"xg must be [T >= 1, rows >= 1, {GATES}], got {tuple(xg.shape)}")
    T, R = xg.shape[0], xg.shape[1]
    if tuple(whh.shape[-2:]) != (GATES, HIDDEN) or whh.dim() not in (2, 3):
        raise ValueError(f"whh must be [{GATES}, {HIDDEN}] or [groups, {GATES}, {HIDDEN}], got {tuple(whh.shape)}")
    if whh.dim() == 3 and (whh.shape[0] < 1 or R % whh.shape[0]):
        raise ValueError(f"{R} rows are no whole number of {whh.shape[0]} interleaved groups")
    for name, s in (("h0", h0), ("c0", c0)):
        if tuple(s.shape) != (R, HIDDEN):
            raise ValueError(f"{name} must be [{R}, {HIDDEN}], got {tuple(s.shape)}")
    if reset is not None and (tuple(reset.shape) != (T, R) or reset.dtype != torch.uint8):
        raise ValueError(f"reset must be uint8 [{T}, {R}] or None, got {reset.dtype} {tuple(reset.shape)}")
    # the kernels take raw pointers: every tensor on xg's device, floating point (cast to float32 on the fused path)
    for name, s in (("xg", xg), ("whh", whh), ("h0", h0), ("c0", c0)):
        if not s.is_floating_point():
            raise ValueError(f"{name} must be floating point, got {s.dtype}")
    for name, s in (("whh", whh), ("reset", reset), ("h0", h0), ("c0", c0)):
        if s is not None and s.device != xg.device:
            raise ValueError(f"{name} is on {s.device}, xg on {xg.device}")


def lstm_sequence(xg, whh, reset, h0, c0, fused: bool = True, fused_grads: bool = False):
    """The LSTM recurrence over a fragment.  xg float32 [T, R, 256] = W_ih z_t + b_ih + b_hh for every step (gate order i, f,
    g, o); whh [256, 64] (``lstm.weight_hh``), or [G, 256, 64]: row r recurs through whh[r % G] (R a multiple of G: the
    interleaved agent rows of a ``PerAgentPolicy``); reset uint8 [T, R] or None -- non-zero: the row uses h = c = 0 in place of the
    previous step's state at step t, and no gradient flows into step t - 1; h0, c0 [R, 64].  Returns h [T, R, 64] and the
    final (h, c); differentiable with respect to xg, whh, h0 and c0.  fused (GPU tensors only): one launch forward, one
    backward plus one (batched) GEMM for dW_hh, computed in float32 whatever the floating-point dtype of the inputs; otherwise a
    loop of torch ops in the inputs' dtype, which is also what CPU tensors always take.  fused_grads (with fused, GPU tensors
    only; ignored otherwise): dW_hh comes from ``mapf_lstm_seq_param_grad`` instead of the GEMM, and hprev is never built.
    Every tensor must be on xg's device."""
    _check_sequence_args(xg, whh, reset, h0, c0)
    if fused and xg.is_cuda:
        reset_c = None if reset is None else reset.contiguous()
        h, hT, cT = _LstmSequence.apply(xg, whh, reset_c, h0, c0, bool(fused_grads))
        return h, (hT, cT)
    h, hT, cT = _lstm_loop(xg, whh, reset, h0, c0)
    return h, (hT, cT)


# ---- a fragment as rows ----------------------------------------------------------------------------------------------------
def is_joint(frag) -> bool:
    """A ``JointRollout.collect()``-shaped dict: one observation per env, [T, B, L]."""
    return "obs" in frag and frag["obs"].dim() == 3


def check_fragment(frag) -> tuple:
    """(T, B, N, L) of a ``Rollout.collect()``- or ``JointRollout.collect()``-shaped dict; ValueError naming the key that is
    missing or misshapen."""
    missing = [k for k in FRAGMENT_KEYS if k not in frag]
    if missing:
        raise ValueError(f"the fragment lacks {missing} (a Rollout.collect() dict has {list(FRAGMENT_KEYS)})")
    obs, actions = frag["obs"], frag["actions"]
    joint = obs.dim() == 3
    if not joint and obs.dim() != 4:
        raise ValueError(f"fragment['obs'] must be [T, B, N, L], got {tuple(obs.shape)}")
    T, B, Lo = int(obs.shape[0]), int(obs.shape[1]), int(obs.shape[-1])
    if joint and (actions.dim() != 3 or tuple(actions.shape[:2]) != (T, B)):
        raise ValueError(f"fragment['actions'] must be [{T}, {B}, N] for obs {[T, B, Lo]}, got {list(actions.shape)}")
    N = int(actions.shape[2]) if joint else int(obs.shape[2])
    layout = _layout(joint, None, B, N)
    want = {k: (T, *layout["per_row"]) for k in ("logp", "value", "rewards", "prev_rewards")}
    want.update({"actions": (T, B, N), "terminated": (T, B), "truncated": (T, B), "first": (T, B), "last_value": layout["per_row"],
                 "h0": (layout["R"], HIDDEN), "c0": (layout["R"], HIDDEN), "prev_action0": (B, N)})
    for k, shape in want.items():
        if tuple(frag[k].shape) != shape:
            raise ValueError(f"fragment['{k}'] must be {list(shape)} for obs {list(obs.shape)}" + (f" and {N} agents" if joint else "")
                             + f", got {list(frag[k].shape)}")
    return T, B, N, Lo


def _layout(joint: bool, module, B: int, N: int) -> dict:
    """The line of the module docstring's table for B envs of N agents, joint (a row is an env) or not, and ``module`` (None:
    one net), as the first fields of ``FragmentView``.  ``agent_axis``: the results keep the agent axis ([.., B', N]) and the loss
    terms come per policy as well."""
    groups = 1 if module is None else module.groups
    R = B if joint else B * N
    return {"R": R, "heads": N if joint else 1, "groups": groups, "units": R // groups, "per_row": (B,) if joint else (B, N),
            "agent_axis": module is not None and module.agent_axis}


@dataclasses.dataclass
class FragmentView:
    """A fragment as R rows of T steps.  Every tensor is a view of the fragment's, except ``first`` / ``ended`` of a multi-agent
    fragment (the env's flag once per agent row), ``prev_actions`` (``prev_action0`` before ``actions[:-1]``) and the
    ``prev_rewards`` of a joint fragment (float64; the joint policy's rule rounds the previous reward to fp32: here, once)."""
    T: int
    R: int
    heads: int
    groups: int
    units: int
    agent_axis: bool
    per_row: tuple              # the shape of one number per row as the fragment holds it: (B,) or (B, N)
    obs: torch.Tensor           # [T, R, L]
    actions: torch.Tensor       # [T, R, heads], as prev_actions
    prev_actions: torch.Tensor
    logp: torch.Tensor          # [T, R], as value, rewards and prev_rewards
    value: torch.Tensor
    rewards: torch.Tensor
    prev_rewards: torch.Tensor
    h0: torch.Tensor            # [R, 64], as c0
    c0: torch.Tensor
    last_value: torch.Tensor    # [R]
    prev_action0: torch.Tensor  # [R, heads]
    first: torch.Tensor = None  # uint8 [T, R], as ended (terminated or truncated)
    ended: torch.Tensor = None
    logits: torch.Tensor = None  # [T, R, 5 heads]: the behaviour policy's, where the rollout kept them (keep_logits)

    def spread(self, x):
        """A per-env [T, B] tensor as [T, R]: once per agent row."""
        return x if x.shape[1] == self.R else x[:, :, None].expand(self.T, x.shape[1], self.R // x.shape[1]).reshape(self.T, self.R)

    def take(self, x, units, dim: int = 1):
        """The rows of the units ``units`` (an index tensor; None: all of them) along ``dim`` of x: one gather."""
        if units is None:
            return x
        index = (slice(None),) * dim + (units,)
        if self.units == self.R:
            return x[index]
        return x.unflatten(dim, (self.units, self.groups))[index].flatten(dim, dim + 1)


def fragment_view(frag, module=None) -> FragmentView:
    """The rows view of a fragment for ``module`` (None: one net, as ``gae`` needs no more); ValueError where the fragment is
    misshapen or is not the module's kind."""
    T, B, N, Lo = check_fragment(frag)
    joint = is_joint(frag)
    if module is not None:
        if joint and isinstance(module, PopulationPolicy):
            raise ValueError("a PopulationPolicy is not supported on a joint fragment: it needs the multi-agent env's [T, B, N, L]")
        if joint and isinstance(module, PerAgentPolicy):
            raise ValueError("DTE (one policy per agent) is not supported on a joint fragment: it needs the multi-agent env's [T, B, N, L]")
        if joint != module.rows_are_envs:
            raise ValueError("a joint fragment (obs [T, B, L]) needs a JointActionPolicy" if joint else
                             "a JointActionPolicy needs a joint fragment (obs [T, B, L])")
        agents = getattr(module, "num_agents", N)  # (a shared policy takes any number of agents)
        if Lo != module.obs_len or N != agents:
            raise ValueError(f"the fragment has {Lo} floats per observation and {N} agents, the module takes {module.obs_len} and {agents}")
        if isinstance(module, PopulationPolicy) and B % module.num_members:
            raise ValueError(f"the fragment has {B} envs, no whole number of the population's {module.num_members} members")
    layout = _layout(joint, module, B, N)
    R, heads = layout["R"], layout["heads"]
    actions, prev_action0 = frag["actions"].reshape(T, R, heads), frag["prev_action0"].reshape(R, heads)
    view = FragmentView(T=T, **layout, obs=frag["obs"].reshape(T, R, Lo), actions=actions,
                        prev_actions=torch.cat([prev_action0[None], actions[:-1]]), prev_action0=prev_action0, h0=frag["h0"],
                        c0=frag["c0"], last_value=frag["last_value"].reshape(R),
                        **{k: frag[k].reshape(T, R) for k in ("logp", "value", "rewards", "prev_rewards")})
    if joint:  # (float64 there)
        view.prev_rewards = view.prev_rewards.to(torch.float32)
    view.first = view.spread(frag["first"])
    view.ended = view.spread(((frag["terminated"] != 0) | (frag["truncated"] != 0)).to(torch.uint8))
    if "logits" in frag:
        want = (T, *layout["per_row"], NUM_ACTIONS * (heads if joint else 1))
        if tuple(frag["logits"].shape) != want:
            raise ValueError(f"fragment['logits'] must be {list(want)} for obs {list(frag['obs'].shape)}, got {list(frag['logits'].shape)}")
        view.logits = frag["logits"].reshape(T, R, NUM_ACTIONS * heads)
    return view


# ---- the dense trunk -------------------------------------------------------------------------------------------------------
def check_trunk_module(module) -> None:
    """ValueError naming the module's kind where ``mapf_trunk_*`` do not cover it: they take one net with one head and
    hidden width 64 (a ``MaskedRecurrentPolicy``), at most ``TRUNK_MAX_FEATURES`` features."""
    kind = f"{type(module).__name__} ('{getattr(module, 'KIND', None)}')"
    if not isinstance(module, MaskedRecurrentPolicy):
        raise ValueError(f"fused_trunk is not supported for a {kind}: the trunk kernels take one shared net with one head "
                         "(a MaskedRecurrentPolicy)")
    if module.hidden != HIDDEN or module.features > L.TRUNK_MAX_FEATURES:
        raise ValueError(f"fused_trunk is not supported for a {kind} with hidden width {module.hidden} and {module.features} "
                         f"features: the trunk kernels take width {HIDDEN} and at most {L.TRUNK_MAX_FEATURES} features")


def _trunk_composition(module, obs, prev_actions, prev_rewards, first):
    """The rule of ``dense_trunk`` in torch ops on [T, R', .] rows: what ``fused=False`` and CPU tensors take."""
    a2 = torch.tanh(module.dense(torch.tanh(module.dense(obs[..., :module.features], "fc1")), "fc2"))
    if not module.recurrent:
        return a2, None
    keep = first == 0
    pa, pr = prev_actions.to(torch.int64) * keep[..., None].to(torch.int64), prev_rewards.to(a2.dtype) * keep.to(a2.dtype)
    z = torch.cat([a2, torch.nn.functional.one_hot(pa, NUM_ACTIONS).to(a2.dtype).flatten(2), pr[..., None]], dim=2)
    return a2, module.dense(z, "lstm")


class _DenseTrunk(torch.autograd.Function):
    """``mapf_trunk_forward`` / ``_backward`` as one differentiable op on M = T R' contiguous rows: (a2 [M, 64], xg [M, 256]) of
    a recurrent net, (a2,) of a feed-forward one.  Backward is the one launch for the pre-activation gradients plus the
    parameter gradients as GEMMs and column sums over the M rows; the six columns of z behind a2 (the one-hot and the
    previous reward) reach the W_ih GEMM as a [M, 6] side tensor built by torch ops in forward.  With ``fused_grads`` the
    parameter gradients are one ``mapf_trunk_param_grad`` call instead, which forms those six columns itself: no side tensor
    is built or saved (prev action, prev reward and first are).  A recurrent net's a2 is not differentiable on its own: it
    reaches the loss through xg alone."""

    @staticmethod
    def forward(ctx, obs, pa, pr, first, w1, b1, w2, b2, wih, bih, bhh, fused_grads=False):
        lib = L.load()
        M, Lo, F, rec = int(obs.shape[0]), int(obs.shape[1]), int(w1.shape[1]), wih is not None
        dev = obs.device
        w1, b1, w2, b2 = f32c(w1), f32c(b1), f32c(w2), f32c(b2)
        a1 = torch.empty((M, HIDDEN), dtype=torch.float32, device=dev)
        a2 = torch.empty_like(a1)
        xg = side = None
        if rec:
            wih, bih, bhh = f32c(wih), f32c(bih), f32c(bhh)
            xg = torch.empty((M, GATES), dtype=torch.float32, device=dev)
        if rec and not fused_grads:  # (mapf_trunk_param_grad forms these six columns itself)
            keep = first == 0
            kept = torch.where(keep, pa, torch.zeros_like(pa))  # (a byte outside 0 .. 4 equals no index below)
            side = torch.cat([(kept[:, None] == torch.arange(NUM_ACTIONS, dtype=torch.int8, device=dev)).to(torch.float32),
                              (pr * keep.to(torch.float32))[:, None]], dim=1)
        rc = lib.mapf_trunk_forward(M, F, Lo, int(rec), ptr(obs), ptr(pa), ptr(pr), ptr(first), ptr(w1), ptr(b1), ptr(w2), ptr(b2),
                                    ptr(wih), ptr(bih), ptr(bhh), ptr(a1), ptr(a2), ptr(xg), stream_of(dev))
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_trunk_forward failed (code {rc})")
        if fused_grads:
            ctx.save_for_backward(obs, a1, a2, w2, wih, pa, pr, first)
        else:
            ctx.save_for_backward(obs, a1, a2, w2, wih, side)
        ctx.features, ctx.fused_grads = F, bool(fused_grads)
        ctx.set_materialize_grads(False)
        if rec:
            ctx.mark_non_differentiable(a2)
            return a2, xg
        return a2, None

    @staticmethod
    def backward(ctx, da2, dxg):
        if ctx.fused_grads:
            obs, a1, a2, w2, wih, pa, pr, first = ctx.saved_tensors
        else:
            obs, a1, a2, w2, wih, side = ctx.saved_tensors
        rec = wih is not None
        g = dxg if rec else da2
        if g is None:
            return (None,) * 12
        lib = L.load()
        g = f32c(g)
        dpre2, dpre1 = torch.empty_like(a2), torch.empty_like(a1)
        rc = lib.mapf_trunk_backward(int(a1.shape[0]), int(rec), ptr(g) if rec else None, None if rec else ptr(g), ptr(a1), ptr(a2),
                                     ptr(wih), ptr(w2), ptr(dpre2), ptr(dpre1), stream_of(a1.device))
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_trunk_backward failed (code {rc})")
        need = ctx.needs_input_grad
        if ctx.fused_grads:
            return (None,) * 4 + _trunk_param_grads(lib, ctx.features, rec, obs, pa, pr, first, a1, a2, dpre1, dpre2, g, need) + (None,)
        dw1 = dpre1.t() @ obs[:, :ctx.features] if need[4] else None
        db1 = dpre1.sum(0) if need[5] else None
        dw2 = dpre2.t() @ a1 if need[6] else None
        db2 = dpre2.sum(0) if need[7] else None
        dwih = dbl = None
        if rec:
            dwih = g.t() @ torch.cat([a2, side], dim=1) if need[8] else None
            dbl = g.sum(0) if need[9] or need[10] else None
        return None, None, None, None, dw1, db1, dw2, db2, dwih, (dbl if need[9] else None), (dbl if need[10] else None), None


def _trunk_param_grads(lib, F, rec, obs, pa, pr, first, a1, a2, dpre1, dpre2, dxg, need) -> tuple:
    """(dw1, db1, dw2, db2, dwih, dbih, dbhh) by ``mapf_trunk_param_grad``: one reduction over the M rows in place of three
    GEMMs, three column sums and the [M, 70] operand; ``need`` is the wrapper's needs_input_grad (None where not needed)."""
    M, dev = int(a1.shape[0]), a1.device

    def out(i, *shape):
        return torch.empty(shape, dtype=torch.float32, device=dev) if need[i] else None

    dw1, db1, dw2, db2 = out(4, HIDDEN, F), out(5, HIDDEN), out(6, HIDDEN, HIDDEN), out(7, HIDDEN)
    dwih = out(8, GATES, HIDDEN + NUM_ACTIONS + 1) if rec else None
    dbl = torch.empty(GATES, dtype=torch.float32, device=dev) if rec and (need[9] or need[10]) else None
    ws = _grad_workspace(lib, M, F, int(rec), 0, dev)
    rc = lib.mapf_trunk_param_grad(M, F, int(obs.shape[1]), int(rec), ptr(obs), ptr(pa), ptr(pr), ptr(first), ptr(a1), ptr(a2), ptr(dpre1),
                                   ptr(dpre2), ptr(dxg) if rec else None, ptr(dw1), ptr(db1), ptr(dw2), ptr(db2), ptr(dwih), ptr(dbl),
                                   ptr(ws), ws.numel(), stream_of(dev))
    if rc != L.MAPF_OK:
        raise RuntimeError(f"mapf_trunk_param_grad failed (code {rc})")
    return dw1, db1, dw2, db2, dwih, (dbl if rec and need[9] else None), (dbl if rec and need[10] else None)


def _check_trunk_args(module, obs, prev_actions, prev_rewards, first):
    if obs.dim() != 3 or obs.shape[-1] != module.obs_len or obs.numel() == 0:
        raise ValueError(f"obs must be [T >= 1, rows >= 1, {module.obs_len}], got {list(obs.shape)}")
    if not obs.is_floating_point():
        raise ValueError(f"obs must be floating point, got {obs.dtype}")
    if not module.recurrent:
        return
    lead = tuple(obs.shape[:-1])
    for name, x in (("prev_actions", prev_actions), ("prev_rewards", prev_rewards), ("first", first)):
        if x is None:
            raise ValueError(f"a recurrent module needs {name}")
        if x.device != obs.device:
            raise ValueError(f"{name} is on {x.device}, obs on {obs.device}")
    if tuple(prev_actions.shape) != lead + (module.heads,) or prev_actions.is_floating_point() or prev_actions.dtype == torch.bool:
        raise ValueError(f"prev_actions must be integer {list(lead + (module.heads,))}, got {prev_actions.dtype} {list(prev_actions.shape)}")
    if tuple(prev_rewards.shape) != lead or not prev_rewards.is_floating_point():
        raise ValueError(f"prev_rewards must be floating point {list(lead)}, got {prev_rewards.dtype} {list(prev_rewards.shape)}")
    if tuple(first.shape) != lead or first.dtype not in (torch.uint8, torch.bool):
        raise ValueError(f"first must be uint8 or bool {list(lead)}, got {first.dtype} {list(first.shape)}")


def dense_trunk(module, obs, prev_actions=None, prev_rewards=None, first=None, fused: bool = True, fused_grads: bool = False):
    """The part of a learner's forward pass that does not depend on the recurrence, on all rows at once: ``(a2, xg)`` with

        a2 = tanh(fc2(tanh(fc1(obs[..., :features]))))                                       [T, R', 64]
        xg = W_ih [a2, onehot5(prev action), prev reward] + b_ih + b_hh                      [T, R', 256], None when feed-forward

    where a row with ``first`` set takes action 0 and reward 0.  obs [T, R', L]; prev_actions integer [T, R', heads],
    prev_rewards [T, R'] and first uint8 [T, R'] are needed by a recurrent module only.  fused (GPU tensors only, a module
    ``check_trunk_module`` accepts): one launch of ``mapf_trunk_forward``, and in the backward pass one of
    ``mapf_trunk_backward`` plus the parameter gradients as GEMMs, computed in float32; the results are differentiable
    with respect to the module's fc1, fc2 and lstm input parameters (a recurrent module's a2 only through xg), not with
    respect to obs.  It needs the built library; there is no fallback.  ``fused=False`` and CPU tensors take the
    composition of torch ops, in the module's dtype, with any module the learners take.  fused_grads (with fused, GPU
    tensors only; ignored otherwise): the parameter gradients come from one ``mapf_trunk_param_grad`` call instead of the
    GEMMs and column sums, and the [M, 6] side tensor of the W_ih operand is neither built nor saved."""
    _check_trunk_args(module, obs, prev_actions, prev_rewards, first)
    if not (fused and obs.is_cuda):
        return _trunk_composition(module, obs, prev_actions, prev_rewards, first)
    check_trunk_module(module)
    lead, M = tuple(obs.shape[:-1]), obs.numel() // obs.shape[-1]
    rows = f32c(obs).reshape(M, obs.shape[-1])
    fc1, fc2 = module.fc1, module.fc2
    if module.recurrent:
        pa, pr = prev_actions.reshape(M).to(torch.int8).contiguous(), f32c(prev_rewards).reshape(M)
        fs = first.reshape(M).to(torch.uint8).contiguous()
        lstm = module.lstm
        a2, xg = _DenseTrunk.apply(rows, pa, pr, fs, fc1.weight, fc1.bias, fc2.weight, fc2.bias, lstm.weight_ih, lstm.bias_ih, lstm.bias_hh,
                                    bool(fused_grads))
        return a2.view(*lead, HIDDEN), xg.view(*lead, GATES)
    a2, _none = _DenseTrunk.apply(rows, None, None, None, fc1.weight, fc1.bias, fc2.weight, fc2.bias, None, None, None, bool(fused_grads))
    return a2.view(*lead, HIDDEN), None


def _forward(module, view: FragmentView, units, fused: bool, fused_trunk: bool = False, fused_grads: bool = False):
    """``sequence_forward`` on a view: logits [T, R', 5 heads] and values [T, R'] on the rows of the units ``units``."""
    F = module.features
    obs = view.take(view.obs, units)
    if module.recurrent:
        first, pa, pr = (view.take(x, units) for x in (view.first, view.prev_actions, view.prev_rewards))
        _a2, xg = dense_trunk(module, obs, pa, pr, first, fused=fused_trunk, fused_grads=fused_grads)
        u, _ = lstm_sequence(xg, module.weight_hh(), first.contiguous(), view.take(view.h0, units, 0),
                             view.take(view.c0, units, 0), fused=fused, fused_grads=fused_grads)
    else:
        u, _xg = dense_trunk(module, obs, fused=fused_trunk, fused_grads=fused_grads)
    logits = module.dense(u, "pi")
    if module.has_mask:
        logits = logits + torch.log(obs[..., F:] + MASK_EPS)
    return logits, module.dense(u, "vf")[..., 0]


def sequence_forward(module, frag, rows=None, fused: bool = True, fused_trunk: bool = False, fused_grads: bool = False):
    """Logits [T, R', 5] and values [T, R'] of ``module`` on a fragment -- what T chained calls of ``module.forward`` on
    (obs[t], prev action, prev reward, first[t], state) return, the state starting from (h0, c0).  rows: an index tensor
    into the view's units (a minibatch of whole sequences), None: all of them.  fc1 / fc2 and W_ih z run once on [T * R']
    rows, the recurrence through ``lstm_sequence``, the heads and the mask term on the stacked h; a feed-forward module has no
    loop at all.  On a joint fragment (obs [T, B, L], a ``JointActionPolicy``) the rows are the B envs, the logits [T, R', 5N]
    and the previous action the N bytes of the env's agents.  With a ``PerAgentPolicy`` the rows are the B envs too (a
    minibatch is whole envs) and the results keep the agent axis: logits [T, B', N, 5], values [T, B', N]."""
    view = fragment_view(frag, module)
    logits, value = _forward(module, view, rows, fused, fused_trunk, fused_grads)
    return (logits.unflatten(1, (-1, view.groups)), value.unflatten(1, (-1, view.groups))) if view.agent_axis else (logits, value)


# ---- advantages ------------------------------------------------------------------------------------------------------------
def gae(frag, gamma=0.99, lam=0.95, boot_value=None, out=None):
    """Generalised advantage estimation on a fragment: (advantages, value targets), float32 [T, B, N] each, written into
    ``out = (adv, targets)`` (contiguous) when given.  No synchronisation.

        delta_t = r_t + gamma * nv_t - v_t;    adv_t = delta_t + gamma * lam * adv_{t+1};    target_t = adv_t + v_t

    Where ``truncated[t]``, nv_t is ``boot_value[t]`` ([T, B, N], the value of the episode's final observation) or 0 when
    boot_value is None; otherwise it is 0 where ``terminated[t]``; otherwise ``value[t + 1]`` (``last_value`` at T - 1).  The
    engine raises both flags at the time limit and ``terminated`` alone when every agent has reached its goal, so a step with
    both flags is a truncation.  The recursion is cut (adv_{t+1} does not enter adv_t) where either flag is set: step t + 1
    belongs to the next episode.

    Without a boot_value a time-limit truncation is treated as a termination.  ``Rollout`` does not evaluate ``final_obs``, so
    it has no such value to give; this deviates from RLlib, which bootstraps truncated episodes with the value function.

    On a joint fragment everything is per env: value, rewards (float64 there, cast to float32 once), boot_value and both
    results are [T, B].

    gamma and lam are floats, or tensors broadcastable to one number per row as the fragment holds it ([B, N], or [B] on a
    joint fragment): every row with its own discount and its own lambda, as the members of a population have them.  A tensor
    is read in float64 and gamma, gamma * lam are rounded to the values' dtype once, as a float is: rows whose entries are
    g and l get exactly what ``gae(frag, g, l)`` gives them."""
    view = fragment_view(frag)
    T, R, shape = view.T, view.R, (view.T, *view.per_row)
    value, rewards = view.value, view.rewards.to(view.value.dtype)
    if out is None:
        out = (torch.empty_like(frag["value"]), torch.empty_like(frag["value"]))
    if tuple(out[0].shape) != shape or tuple(out[1].shape) != shape:
        raise ValueError(f"out must be two {list(shape)} tensors")
    adv, targets = out[0].view(T, R), out[1].view(T, R)
    live = view.ended == 0
    nv = torch.empty_like(value)
    nv[:-1].copy_(value[1:])
    nv[-1].copy_(view.last_value)
    nv = nv * live.to(nv.dtype)
    if boot_value is not None:
        if tuple(boot_value.shape) != shape:
            raise ValueError(f"boot_value must be {list(shape)}, got {list(boot_value.shape)}")
        nv = torch.where(view.spread(frag["truncated"] != 0), boot_value.reshape(T, R).to(nv.dtype), nv)
    if torch.is_tensor(gamma) or torch.is_tensor(lam):
        g64, l64 = (torch.as_tensor(x, dtype=torch.float64, device=value.device).expand(view.per_row).reshape(R) for x in (gamma, lam))
        gamma, lam = g64.to(value.dtype), 1.0
        carry = (g64 * l64).to(value.dtype) * live.to(value.dtype)
    else:
        carry = (gamma * lam) * live.to(value.dtype)
    delta = rewards + gamma * nv - value
    adv[T - 1].copy_(delta[T - 1])
    for t in range(T - 2, -1, -1):
        torch.addcmul(delta[t], carry[t], adv[t + 1], out=adv[t])
    torch.add(adv, value, out=targets)
    return out[0], out[1]


# ---- the epoch / minibatch loop ----------------------------------------------------------------------------------------------
class _MinibatchLearner:
    """What ``PPOLearner`` and ``IMPALALearner`` share: Adam over the module's parameters, the seeded generator of the
    minibatch permutations and the epoch loop.  Minibatches are disjoint sets of the view's units (whole sequences of T steps,
    each starting from the fragment's h0 / c0); every unit is used exactly once per epoch."""

    needs_gae = False  # ``update`` takes (frag, adv, targets) instead of (frag)

    def __init__(self, module, lr: float, epochs: int, minibatches: int, grad_clip, seed: int, fused: bool, fused_trunk: bool = False,
                 fused_grads: bool = False):
        if epochs < 1 or minibatches < 1:
            raise ValueError("epochs and minibatches must be >= 1")
        if fused_trunk:  # (a module the trunk kernels do not cover is refused here, by kind, not in the first update)
            check_trunk_module(module)
        self.fused_trunk = bool(fused_trunk)
        self.fused_grads = bool(fused_grads)  # (any module: dW_hh with ``fused``, the trunk's with ``fused_trunk``)
        self.module, self.epochs, self.minibatches, self.grad_clip, self.fused = module, int(epochs), int(minibatches), grad_clip, bool(fused)
        self.optimizer = torch.optim.Adam(module.parameters(), lr=lr)
        self.device = next(module.parameters()).device
        self._gen = torch.Generator(device=self.device)
        self._gen.manual_seed(int(seed))

    def minibatch_rows(self, rows: int) -> list:
        """One epoch's minibatches: a fresh permutation of the rows in ``minibatches`` nearly equal parts (fewer when there
        are fewer rows than minibatches)."""
        perm = torch.randperm(int(rows), generator=self._gen, device=self.device)
        return [p for p in perm.tensor_split(min(self.minibatches, int(rows)))]

    def _epochs(self, view: FragmentView, terms_of) -> dict:
        """``epochs`` passes of Adam steps on ``terms_of(units)["total_loss"]``, the gradient norm of every net of the module
        bounded by ``grad_clip`` on its own; the terms averaged over the last epoch's minibatches (nothing is synchronised),
        with ``per_policy`` where ``terms_of`` gives it: then the four terms are the means over the policies."""
        last = None
        for _ in range(self.epochs):
            last = []
            for units in self.minibatch_rows(view.units):
                terms = terms_of(units)
                self.optimizer.zero_grad(set_to_none=True)
                terms["total_loss"].backward()
                if self.grad_clip is not None:
                    for net in self.module.nets():
                        torch.nn.utils.clip_grad_norm_(net.parameters(), float(self.grad_clip))
                self.optimizer.step()
                last.append({k: v.detach() for k, v in terms.get("per_policy", terms).items()})
        mean = {k: torch.stack([m[k] for m in last]).mean(dim=0) for k in last[0]}
        return {**{k: v.mean() for k, v in mean.items()}, "per_policy": mean} if view.agent_axis else mean


# ---- PPO -------------------------------------------------------------------------------------------------------------------
def ppo_objective(logits, values, actions, old_logp, adv, targets, clip=0.05, vf_clip=10.0, vf_coeff=0.5,
                  ent_coeff=0.001, old_logits=None, kl_coeff=None, groups: int = 1, per_group: bool = False):
    """The PPO loss terms of logits [T, R, 5 heads] and values [T, R] in torch ops, differentiable with respect to both:
    ({policy_loss, vf_loss, entropy, [kl,] total_loss}, {logp, kl}).  actions [T, R, heads]; old_logp, adv (standardised),
    targets [T, R].  kl_coeff: None, or a tensor [groups] -- then old_logits [T, R, 5 heads] are the behaviour policy's,
    ``kl`` is the mean of KL(behaviour || current) summed over a row's heads, and total_loss has kl_coeff * kl added.
    per_group: every term is a [groups] tensor, the mean over the rows r with r % groups = g; otherwise a mean over
    everything.  clip, vf_clip, vf_coeff and ent_coeff are floats, or (per_group only) tensors [groups]: row r is then judged
    with entry r % groups, as ``mapf_ppo_loss_hp`` reads its ``hp``.  What ``mapf_ppo_loss`` computes in one launch; the
    ``fused_objective=False`` baseline."""
    heads = int(actions.shape[2])
    if any(torch.is_tensor(x) for x in (clip, vf_clip, vf_coeff, ent_coeff)) and not per_group:
        raise ValueError("per-group clip, vf_clip, vf_coeff or ent_coeff need per_group=True")

    def rowwise(x):  # [groups] -> [1, R]: row r takes entry r % groups (a float stays a float)
        return x.to(logits.dtype).repeat(int(values.shape[1]) // groups)[None] if torch.is_tensor(x) else x

    def groupwise(x):
        return x.to(logits.dtype) if torch.is_tensor(x) else x

    clip_r, vf_clip_r, vf_coeff, ent_coeff = rowwise(clip), rowwise(vf_clip), groupwise(vf_coeff), groupwise(ent_coeff)
    logp_all = torch.log_softmax(logits.unflatten(2, (heads, NUM_ACTIONS)), dim=3)
    logp = logp_all.gather(3, actions.to(torch.int64)[..., None])[..., 0].sum(dim=2)
    ratio = torch.exp(logp - old_logp)
    if torch.is_tensor(clip_r):
        clamped = torch.minimum(torch.maximum(ratio, 1.0 - clip_r), 1.0 + clip_r)
    else:
        clamped = torch.clamp(ratio, 1.0 - clip, 1.0 + clip)
    surrogate = torch.minimum(adv * ratio, adv * clamped)

    def mean(x):  # [T, R'] -> one number, or one per policy
        return x.unflatten(1, (-1, groups)).mean(dim=(0, 1)) if per_group else x.mean()

    per = {"policy_loss": -mean(surrogate),
           "vf_loss": mean(torch.minimum((values - targets) ** 2, vf_clip_r) if torch.is_tensor(vf_clip_r)
                           else torch.clamp((values - targets) ** 2, max=vf_clip)),
           "entropy": mean(-(torch.exp(logp_all) * logp_all).flatten(2).sum(dim=2))}
    total = per["policy_loss"] + vf_coeff * per["vf_loss"] - ent_coeff * per["entropy"]
    kl = None
    if kl_coeff is not None:
        old = torch.log_softmax(old_logits.to(logp_all.dtype).unflatten(2, (heads, NUM_ACTIONS)), dim=3)
        kl = (torch.exp(old) * (old - logp_all)).flatten(2).sum(dim=2)
        coeff = kl_coeff.to(logp_all.dtype)
        per["kl"] = mean(kl)
        total = total + (coeff if per_group else coeff[0]) * per["kl"]
    per["total_loss"] = total
    return per, {"logp": logp, "kl": kl}


class _PPOLoss(torch.autograd.Function):
    """``mapf_ppo_loss`` as one differentiable op: (total_loss, policy_loss, vf_loss, entropy, kl) of logits [T, R, 5 heads]
    and values [T, R], each a [groups] tensor of per-policy means; forward is the one launch plus the sum of the tiles'
    partials, backward scales the gradients the launch left behind, every group's by its own total's.  Only total_loss is
    differentiable.  kl_coeff: a float32 device tensor [groups] the kernel reads, or None (no KL term; old_logits unused).
    hp: None, or a float32 device tensor [groups, 4] (clip, vf_clip, vf_coeff, ent_coeff per group) that the kernel reads in
    place of ``scalars`` (``mapf_ppo_loss_hp``); its owner has validated the values."""

    @staticmethod
    def forward(ctx, logits, values, actions, old_logp, adv, targets, old_logits, kl_coeff, heads, groups, scalars, hp=None):
        lib = L.load()
        T, R, heads, G = int(values.shape[0]), int(values.shape[1]), int(heads), int(groups)
        ctx.dtypes = (logits.dtype, values.dtype)
        lg, v, old_logp, adv, targets = f32c(logits), f32c(values), f32c(old_logp), f32c(adv), f32c(targets)
        actions = actions.to(torch.int8).contiguous()
        dev = lg.device
        if G < 1 or R % G:
            raise ValueError(f"{R} rows are no whole number of {G} interleaved groups")
        # the kernel takes raw pointers: every tensor on the logits' device, of the shape the launch walks
        checked = [("values", v, (T, R)), ("actions", actions, (T, R, heads)), ("old_logp", old_logp, (T, R)), ("adv", adv, (T, R)),
                   ("targets", targets, (T, R)), ("logits", lg, (T, R, NUM_ACTIONS * heads))]
        if kl_coeff is not None:
            if old_logits is None:
                raise ValueError("a KL coefficient needs the behaviour policy's logits")
            old_logits = f32c(old_logits)
            if kl_coeff.dtype != torch.float32 or not kl_coeff.is_contiguous():
                raise ValueError(f"kl_coeff must be a contiguous float32 tensor, got {kl_coeff.dtype}")
            checked += [("old_logits", old_logits, (T, R, NUM_ACTIONS * heads)), ("kl_coeff", kl_coeff, (G,))]
        else:
            old_logits = None
        if hp is not None:
            if hp.dtype != torch.float32 or not hp.is_contiguous():
                raise ValueError(f"hp must be a contiguous float32 tensor, got {hp.dtype}")
            checked.append(("hp", hp, (G, 4)))
        for name, x, shape in checked:
            if x.device != dev or tuple(x.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)} on {dev}, got {list(x.shape)} on {x.device}")
        dlogits = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        dvalues = torch.empty_like(v) if ctx.needs_input_grad[1] else None
        partials = torch.empty((int(lib.mapf_ppo_partials(R, G)), 5), dtype=torch.float32, device=dev)
        before = (T, R, heads, G, ptr(lg), ptr(old_logits), ptr(actions), ptr(old_logp), ptr(adv), ptr(v), ptr(targets), *scalars,
                  ptr(kl_coeff))
        after = (None, None, ptr(dlogits), ptr(dvalues), ptr(partials), stream_of(dev))
        rc = lib.mapf_ppo_loss(*before, *after) if hp is None else lib.mapf_ppo_loss_hp(*before, ptr(hp), *after)
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_ppo_loss failed (code {rc})")
        ctx.grads, ctx.groups, ctx.with_hp = (dlogits, dvalues), G, int(hp is not None)
        policy, vf, entropy, kl, total = (partials.view(G, -1, 5).sum(1) * (G / (T * R))).unbind(1)
        ctx.mark_non_differentiable(policy, vf, entropy, kl)
        return total, policy, vf, entropy, kl

    @staticmethod
    def backward(ctx, g, *_unused):
        dlogits, dvalues = ctx.grads
        G = ctx.groups
        if dlogits is not None:  # row r is group r % G: [T, R / G, G, .] times g [G]
            dlogits = (dlogits.unflatten(1, (-1, G)) * g[:, None]).flatten(1, 2).to(ctx.dtypes[0])
        if dvalues is not None:
            dvalues = (dvalues.unflatten(1, (-1, G)) * g).flatten(1, 2).to(ctx.dtypes[1])
        return (dlogits, dvalues) + (None,) * (9 + ctx.with_hp)  # (hp is passed only where there is one)


# tools/time_ppo.py: the objective forward + backward at T = 32 fused / torch ops 0.18 / 0.70 ms (11 / 86 kernels) at 8 192
# rows and 0.13 / 0.74 ms at 65 536, one update epoch 18.2 / 19.6 ms and 46.4 / 48.7 ms, the fused objective faster in every
# one of three alternating rounds at both sizes
PPO_FUSED_OBJECTIVE_DEFAULT = True


class PPOLearner(_MinibatchLearner):
    """Clipped-surrogate PPO with Adam on a ``MaskedRecurrentPolicy``, a ``JointActionPolicy`` or a ``PerAgentPolicy``.  With
    the last it is N independent learners in one: minibatches are sets of envs, advantages are standardised per policy,
    every loss term is a per-policy mean, ``grad_clip`` bounds each policy's own gradient norm and ``total_loss`` is the sum
    of the N per-policy totals.

    With a ``PopulationPolicy`` it is P independent learners in one by the same rule with "policy" read as "member": a unit
    of a minibatch is P consecutive envs, one of every member; advantages are standardised per member over its
    [T, B / P, N]; a member's loss term is the mean of its N agent groups' means; ``per_policy`` is per member.  ``clip``,
    ``vf_clip``, ``vf_coeff`` and ``ent_coeff`` are per member, in one float32 device tensor (``hp``, written through
    ``set_hyper``) that the fused objective reads (``mapf_ppo_loss_hp``: on the GPU it is the only path); ``kl_coeff`` is
    per member; Adam has one parameter group per member, so ``lr`` is per member too.  ``epochs`` and ``minibatches`` are
    one value for the whole population.

    kl_coeff (None: no such term, the default): RLlib's adaptive KL penalty, which the reference's PPO runs with at 0.2 /
    ``kl_target`` 0.01 -- ``kl_coeff * KL(behaviour || current)`` joins the loss, and after every ``update`` the
    coefficient grows by 1.5 where the last epoch's mean KL exceeds 2 kl_target and halves where it is below 0.5 kl_target.
    ``self.kl_coeff`` is then a float32 tensor [G] on the module's device (G = N policies of a ``PerAgentPolicy``, else 1),
    adapted there without a synchronisation, and the fragment must carry the behaviour ``logits`` (``keep_logits``).
    fused_objective (GPU only): the whole objective and its gradients with respect to logits and values in one launch of
    ``mapf_ppo_loss`` instead of elementary torch ops; None: off without a KL coefficient, ``PPO_FUSED_OBJECTIVE_DEFAULT``
    with one.  It needs the built library; there is no fallback.  CPU tensors always take the torch ops."""

    needs_gae = True

    def __init__(self, module, lr: float = 1e-3, clip: float = 0.05, vf_coeff: float = 0.5,
                 ent_coeff: float = 0.001, vf_clip: float = 10.0, epochs: int = 12, minibatches: int = 8, grad_clip=None,
                 seed: int = 0, fused: bool = True, kl_coeff: float | None = None, kl_target: float = 0.01,
                 fused_objective: bool | None = None, fused_trunk: bool = False, fused_grads: bool = False):
        super().__init__(module, lr, epochs, minibatches, grad_clip, seed, fused, fused_trunk, fused_grads)
        self.clip, self.vf_coeff, self.ent_coeff, self.vf_clip = float(clip), float(vf_coeff), float(ent_coeff), float(vf_clip)
        self.kl_coeff, self.kl_target, self.sampled_kl = None, float(kl_target), None
        self.population = isinstance(module, PopulationPolicy)
        policies = module.num_members if self.population else getattr(module, "groups", 1)
        if kl_coeff is not None:
            if not math.isfinite(float(kl_coeff)) or float(kl_coeff) < 0 or not self.kl_target > 0:
                raise ValueError(f"kl_coeff must be finite and >= 0 and kl_target > 0, got {kl_coeff} and {kl_target}")
            self.kl_coeff = torch.full((policies,), float(kl_coeff), dtype=torch.float32, device=self.device)
        self.kl_coeff0 = None if kl_coeff is None else float(kl_coeff)
        if self.population:
            if fused_objective is False:
                raise ValueError("with a PopulationPolicy the fused objective (mapf_ppo_loss_hp) is the only path on the GPU")
            fused_objective = True
            # one Adam with a parameter group per member (lr is per member); the hyperparameters of the objective as the
            # kernel reads them, [P N, 4]: a member's row once per agent group
            self.optimizer = torch.optim.Adam([{"params": list(m.parameters()), "lr": float(lr)} for m in module.members])
            self.hp_groups = torch.zeros((module.groups, 4), dtype=torch.float32, device=self.device)
            for p in range(policies):
                self.set_hyper(p, clip=clip, vf_clip=vf_clip, vf_coeff=vf_coeff, ent_coeff=ent_coeff)
        if fused_objective is None:
            fused_objective = PPO_FUSED_OBJECTIVE_DEFAULT if kl_coeff is not None else False
        self.fused_objective = bool(fused_objective)

    HP_COLUMNS = ("clip", "vf_clip", "vf_coeff", "ent_coeff")  # the columns of mapf_ppo_loss_hp's hp

    @property
    def hp(self) -> torch.Tensor:
        """[P, 4] float32 on the device: clip, vf_clip, vf_coeff, ent_coeff of every member (a view of what the kernel reads)."""
        return self.hp_groups.view(self.module.num_members, self.module.num_agents, 4)[:, 0]

    def set_hyper(self, member: int, lr=None, **values) -> None:
        """Member ``member``'s ``lr`` and / or columns of ``hp`` (``clip`` in [0, 1); ``vf_clip``, ``vf_coeff``, ``ent_coeff``
        finite and >= 0: the kernel cannot check them, so every value is checked here before it is written).  Device writes
        on the current stream, no synchronisation."""
        if not self.population or not 0 <= int(member) < self.module.num_members:
            raise ValueError(f"set_hyper needs a PopulationPolicy and a member in 0 .. its size - 1, got {member}")
        for name, x in values.items():
            if name not in self.HP_COLUMNS:
                raise ValueError(f"{name} is no per-member hyperparameter of the objective ({', '.join(self.HP_COLUMNS)}, lr)")
            if not math.isfinite(float(x)) or float(x) < 0 or (name == "clip" and float(x) >= 1):
                raise ValueError(f"{name} must be finite and >= 0" + (" and < 1" if name == "clip" else "") + f", got {x}")
        if lr is not None and not (math.isfinite(float(lr)) and float(lr) > 0):
            raise ValueError(f"lr must be finite and > 0, got {lr}")
        rows = self.hp_groups.view(self.module.num_members, self.module.num_agents, 4)[int(member)]
        for name, x in values.items():
            rows[:, self.HP_COLUMNS.index(name)] = float(x)
        if lr is not None:
            self.optimizer.param_groups[int(member)]["lr"] = float(lr)

    def reset_member(self, member: int) -> None:
        """What a rebuilt trial starts from: member ``member``'s Adam moments and step count are dropped (the next step
        starts them at zero) and its KL coefficient returns to the initial value."""
        for prm in self.module.members[int(member)].parameters():
            self.optimizer.state.pop(prm, None)
        if self.kl_coeff is not None:
            self.kl_coeff[int(member)] = self.kl_coeff0

    def losses(self, frag, adv, targets, rows=None, _view=None) -> dict:
        """The loss terms on the units ``rows`` (None: all), means over [T, R']: ``policy_loss`` (minus the clipped surrogate
        on exp(logp_new - logp_old)), ``vf_loss`` (the squared error clamped at vf_clip), ``entropy`` (of the masked
        logits) and ``total_loss`` = policy_loss + vf_coeff * vf_loss - ent_coeff * entropy.  adv: already standardised.
        A row's log-probability is the sum over its heads and its entropy the sum of their entropies.  With a
        ``PerAgentPolicy`` also ``per_policy``: the four terms as [N] tensors, each a mean over that agent's [T, B'];
        ``total_loss`` is then their totals' SUM (what is differentiated: policy a's parameters receive exactly the gradient
        of its own total), the other three are means over the policies.  With a KL coefficient also ``kl``, the mean
        KL(behaviour || current) summed over a row's heads, and ``total_loss`` has ``kl_coeff * kl`` added (per policy)."""
        view = fragment_view(frag, self.module) if _view is None else _view
        T, R = view.T, view.R
        with_kl = self.kl_coeff is not None
        if with_kl and view.logits is None:
            raise ValueError("a PPOLearner with a kl_coeff needs the behaviour policy's logits in the fragment: build the "
                             "rollout with keep_logits=True (Trainer does)")
        logits, value = _forward(self.module, view, rows, self.fused, self.fused_trunk, self.fused_grads)
        actions, old_logp = view.take(view.actions, rows), view.take(view.logp, rows)
        a, tg = view.take(adv.reshape(T, R), rows), view.take(targets.reshape(T, R), rows)
        old_logits = view.take(view.logits, rows) if with_kl else None
        names = ("policy_loss", "vf_loss", "entropy") + (("kl",) if with_kl else ()) + ("total_loss",)
        scalars, kl_coeff, hp = (self.clip, self.vf_clip, self.vf_coeff, self.ent_coeff), self.kl_coeff, None
        if self.population:  # per member -> per group: a member's number once per agent group
            N = self.module.num_agents
            kl_coeff, hp = (kl_coeff.repeat_interleave(N) if with_kl else None), self.hp_groups
        if self.fused_objective and logits.is_cuda:
            total, policy_loss, vf_loss, entropy, kl = _PPOLoss.apply(
                logits, value, actions, old_logp, a, tg, old_logits, kl_coeff, view.heads, view.groups, scalars,
                *(() if hp is None else (hp,)))
            per = {"policy_loss": policy_loss, "vf_loss": vf_loss, "entropy": entropy, "kl": kl, "total_loss": total}
            per = {k: per[k] if view.agent_axis else per[k][0] for k in names}
        else:
            if hp is not None:
                scalars = tuple(hp[:, i] for i in range(4))
            per = ppo_objective(logits, value, actions, old_logp, a, tg, *scalars, old_logits, kl_coeff, view.groups, view.agent_axis)[0]
        if not view.agent_axis:
            return per
        if self.population:  # a member's term is the mean of its N groups' means (its coefficients are the same in all of them)
            per = {k: v.unflatten(0, (-1, self.module.num_agents)).mean(dim=1) for k, v in per.items()}
        return {"total_loss": per["total_loss"].sum(), **{k: per[k].mean() for k in names[:-1]}, "per_policy": per}

    def update(self, frag, adv, targets) -> dict:
        """``epochs`` passes of ``minibatches`` Adam steps over the fragment.  Advantages are standardised first, over the
        whole fragment or, with a ``PerAgentPolicy``, over each agent's [T, B].  Returns the loss terms averaged over the last
        epoch's minibatches, as tensors on the module's device; nothing is synchronised.  With a ``PerAgentPolicy`` the terms
        are averaged over the policies as well, plus ``per_policy``, the same four terms as [N] tensors.  With a KL
        coefficient ``kl`` is among the terms (kept per policy as ``sampled_kl``), the coefficient is adapted by it on the
        device, and ``kl_coeff`` is the adapted one (the mean over the policies, and [N] under ``per_policy``)."""
        view = fragment_view(frag, self.module)
        over = (0, 1) if view.agent_axis else None  # adv [T, B, N]: per agent; otherwise everything
        shape = adv.shape
        if self.population:  # [T, B / P, P, N]: per member, over its envs and all their agents
            adv, over = adv.unflatten(1, (-1, self.module.num_members)), (0, 1, 3)
        adv = (adv - adv.mean(dim=over, keepdim=True)) / torch.clamp(adv.std(dim=over, unbiased=False, keepdim=True), min=1e-4)
        adv = adv.reshape(shape)
        out = self._epochs(view, lambda units: self.losses(frag, adv, targets, units, view))
        if self.kl_coeff is not None:
            self.sampled_kl = (out["per_policy"]["kl"] if view.agent_axis else out["kl"].reshape(1)).to(torch.float32)
            self.kl_coeff.copy_(adapted_kl_coeff(self.kl_coeff, self.sampled_kl, self.kl_target))
            out["kl_coeff"] = self.kl_coeff.mean()
            if view.agent_axis:
                out["per_policy"]["kl_coeff"] = self.kl_coeff.clone()
        return out


def adapted_kl_coeff(coeff, sampled_kl, kl_target: float):
    """RLlib's rule for PPO's KL coefficient, elementwise and without a synchronisation: x 1.5 where the sampled KL is above
    2 kl_target, x 0.5 where it is below 0.5 kl_target, unchanged in between."""
    return torch.where(sampled_kl > 2.0 * kl_target, coeff * 1.5, torch.where(sampled_kl < 0.5 * kl_target, coeff * 0.5, coeff))


# ---- IMPALA ----------------------------------------------------------------------------------------------------------------
def vtrace(behaviour_logp, target_logp, values, rewards, ended, bootstrap, gamma: float = 0.99, lam: float = 1.0,
           clip_rho: float = 1.0, clip_c: float = 1.0, clip_pg_rho: float = 1.0):
    """V-trace targets and policy-gradient advantages (Espeholt et al. 2018, as RLlib's torch IMPALA learner applies them):
    ``(vs, pg_adv)``, [T, R] each, in the dtype of ``values``; constants of the objective, so nothing here is differentiated.

        w = exp(target_logp - behaviour_logp);  rho, c, rho_pg = min(clip_rho, w), lam * min(clip_c, w), min(clip_pg_rho, w)
        disc = gamma * (ended ? 0 : 1);   delta_t = rho_t (r_t + disc_t V_{t+1} - V_t)            V_T = vs_T = bootstrap
        acc_t = delta_t + disc_t c_t acc_{t+1};   vs_t = V_t + acc_t;   pg_adv_t = rho_pg_t (r_t + disc_t vs_{t+1} - V_t)

    behaviour_logp, target_logp, values, rewards [T, R]; ended [T, R], non-zero where the episode ended at step t (terminated
    or truncated: a time-limit truncation counts as a termination, as in ``gae`` without a boot_value); bootstrap [R], the
    value after step T - 1.  Elementary torch ops, a loop over t: the readable statement of ``mapf_vtrace_loss``'s rule, the
    ``fused=False`` baseline, and what CPU tensors always take."""
    if values.dim() != 2 or values.shape[0] < 1 or values.shape[1] < 1:
        raise ValueError(f"values must be [T >= 1, rows >= 1], got {list(values.shape)}")
    T, R = (int(x) for x in values.shape)
    for name, x in (("behaviour_logp", behaviour_logp), ("target_logp", target_logp), ("rewards", rewards), ("ended", ended)):
        if tuple(x.shape) != (T, R):
            raise ValueError(f"{name} must be [{T}, {R}] like values, got {list(x.shape)}")
    if tuple(bootstrap.shape) != (R,):
        raise ValueError(f"bootstrap must be [{R}], got {list(bootstrap.shape)}")
    dt = values.dtype
    values, rewards, bootstrap = values.detach(), rewards.detach().to(dt), bootstrap.detach().to(dt)
    w = torch.exp(target_logp.detach().to(dt) - behaviour_logp.detach().to(dt))
    rho, c, rho_pg = torch.clamp(w, max=clip_rho), lam * torch.clamp(w, max=clip_c), torch.clamp(w, max=clip_pg_rho)
    disc = gamma * (ended == 0).to(dt)
    delta = rho * (rewards + disc * torch.cat([values[1:], bootstrap[None]]) - values)
    carry = disc * c
    acc, accs = torch.zeros_like(bootstrap), [None] * T
    for t in range(T - 1, -1, -1):
        acc = delta[t] + carry[t] * acc
        accs[t] = acc
    vs = values + torch.stack(accs)
    pg_adv = rho_pg * (rewards + disc * torch.cat([vs[1:], bootstrap[None]]) - values)
    return vs, pg_adv


def impala_objective(logits, values, actions, behaviour_logp, rewards, ended, bootstrap, gamma: float = 0.99, lam: float = 1.0,
                     clip_rho: float = 1.0, clip_c: float = 1.0, clip_pg_rho: float = 1.0, vf_coeff: float = 0.5,
                     ent_coeff: float = 0.0):
    """The IMPALA loss terms of logits [T, R, 5 heads] and values [T, R] in torch ops, differentiable with respect to both:
    ({total_loss, policy_loss, vf_loss, entropy}, {logp, vs, pg_adv}).  actions [T, R, heads]; the rest as ``vtrace`` takes
    them.  What ``mapf_vtrace_loss`` computes in one launch; the ``fused=False`` baseline."""
    T, heads = int(values.shape[0]), int(actions.shape[2])
    logp_all = torch.log_softmax(logits.reshape(T, -1, heads, NUM_ACTIONS), dim=3)
    logp = logp_all.gather(3, actions.to(torch.int64)[..., None])[..., 0].sum(dim=2)
    vs, pg_adv = vtrace(behaviour_logp, logp, values, rewards, ended, bootstrap, gamma, lam, clip_rho, clip_c, clip_pg_rho)
    policy_loss = -(pg_adv * logp).mean()
    vf_loss = 0.5 * ((values - vs) ** 2).mean()
    entropy = -(torch.exp(logp_all) * logp_all).sum(dim=(2, 3)).mean()
    terms = {"total_loss": policy_loss + vf_coeff * vf_loss - ent_coeff * entropy, "policy_loss": policy_loss, "vf_loss": vf_loss,
             "entropy": entropy}
    return terms, {"logp": logp, "vs": vs, "pg_adv": pg_adv}


class _VtraceLoss(torch.autograd.Function):
    """``mapf_vtrace_loss`` as one differentiable op: (total_loss, policy_loss, vf_loss, entropy) of logits [T, R, 5 heads]
    and values [T, R]; forward is the one launch plus the sum of the workgroups' partials, backward scales the gradients
    the launch left behind.  Only total_loss is differentiable."""

    @staticmethod
    def forward(ctx, logits, values, actions, mu, rewards, ended, boot, heads, scalars):
        lib = L.load()
        T, R = int(values.shape[0]), int(values.shape[1])
        ctx.dtypes = (logits.dtype, values.dtype)
        lg, v, mu, rewards, boot = f32c(logits), f32c(values), f32c(mu), f32c(rewards), f32c(boot)
        actions, ended = actions.to(torch.int8).contiguous(), ended.to(torch.uint8).contiguous()
        dev = lg.device
        # the kernel takes raw pointers: every tensor on the logits' device, of the shape the launch walks
        for name, x, shape in (("values", v, (T, R)), ("actions", actions, (T, R, int(heads))), ("behaviour_logp", mu, (T, R)),
                               ("rewards", rewards, (T, R)), ("ended", ended, (T, R)), ("bootstrap", boot, (R,)),
                               ("logits", lg, (T, R, NUM_ACTIONS * int(heads)))):
            if x.device != dev or tuple(x.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)} on {dev}, got {list(x.shape)} on {x.device}")
        vs = torch.empty((T, R), dtype=torch.float32, device=dev)
        pg = torch.empty_like(vs)
        dlogits = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        dvalues = torch.empty_like(v) if ctx.needs_input_grad[1] else None
        partials = torch.empty((int(lib.mapf_vtrace_partials(R)), 4), dtype=torch.float32, device=dev)
        stream = stream_of(dev)
        rc = lib.mapf_vtrace_loss(T, R, int(heads), ptr(lg), ptr(actions), ptr(mu), ptr(v), ptr(rewards), ptr(ended), ptr(boot),
                                  *scalars, ptr(vs), ptr(pg), None, ptr(dlogits), ptr(dvalues), ptr(partials), stream)
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_vtrace_loss failed (code {rc})")
        ctx.grads = (dlogits, dvalues)
        policy, vf, entropy, total = (partials.sum(0) * (1.0 / (T * R))).unbind(0)
        ctx.mark_non_differentiable(policy, vf, entropy)
        return total, policy, vf, entropy

    @staticmethod
    def backward(ctx, g, *_unused):
        dlogits, dvalues = ctx.grads
        return (None if dlogits is None else (dlogits * g).to(ctx.dtypes[0]),
                None if dvalues is None else (dvalues * g).to(ctx.dtypes[1]), None, None, None, None, None, None, None)


# tools/time_impala.py: losses + backward at T = 32 fused / torch ops 5.6 / 17.1 ms at 8 192 rows and 26.5 / 86.0 ms at 65 536, the
# fused path faster in every one of three alternating rounds at both sizes
IMPALA_FUSED_DEFAULT = True


class IMPALALearner(_MinibatchLearner):
    """IMPALA (V-trace actor-critic) with Adam on a ``MaskedRecurrentPolicy`` or a ``JointActionPolicy``: one pass per
    fragment by default, minibatches as in ``PPOLearner``, global-norm gradient clipping.  The targets come from the current
    network in every minibatch, bootstrapped with the fragment's ``last_value`` (the behaviour network's value: the fragment
    does not carry the observation after its last step, so the target network is not evaluated there).  fused (GPU only):
    the objective and its gradients in one launch of ``mapf_vtrace_loss`` and the recurrence on the sequence kernels; it
    needs the built library, there is no fallback.  ``fused=False`` is the same rule in torch ops, in the module's dtype, and
    what a module on the CPU always takes."""

    def __init__(self, module, lr: float = 1e-3, vf_coeff: float = 0.5, ent_coeff: float = 0.0, gamma: float = 0.99,
                 lam: float = 1.0, clip_rho: float = 1.0, clip_c: float = 1.0, clip_pg_rho: float = 1.0, epochs: int = 1,
                 minibatches: int = 8, grad_clip=40.0, seed: int = 0, fused: bool = IMPALA_FUSED_DEFAULT,
                 fused_trunk: bool = False, fused_grads: bool = False):
        super().__init__(module, lr, epochs, minibatches, grad_clip, seed, fused, fused_trunk, fused_grads)
        if isinstance(module, PerAgentPolicy):
            raise ValueError("DTE (one policy per agent) is not supported by IMPALALearner; PPOLearner takes a PerAgentPolicy")
        if isinstance(module, PopulationPolicy):
            raise ValueError("a PopulationPolicy is not supported by IMPALALearner; PPOLearner takes a PopulationPolicy")
        scalars = {"gamma": gamma, "lam": lam, "clip_rho": clip_rho, "clip_c": clip_c, "clip_pg_rho": clip_pg_rho,
                   "vf_coeff": vf_coeff, "ent_coeff": ent_coeff}
        for name, x in scalars.items():  # what mapf_vtrace_loss refuses, refused here by name
            if not math.isfinite(float(x)) or float(x) < 0 or (name in ("gamma", "lam") and float(x) > 1):
                raise ValueError(f"{name} must be finite and >= 0" + (" and <= 1" if name in ("gamma", "lam") else "") + f", got {x}")
        self.gamma, self.lam, self.clip_rho, self.clip_c, self.clip_pg_rho, self.vf_coeff, self.ent_coeff = \
            (float(x) for x in scalars.values())

    def losses(self, frag, rows=None, _view=None) -> dict:
        """The loss terms on the rows ``rows`` (None: all), means over [T, R']: ``policy_loss`` = -mean(pg_adv logp),
        ``vf_loss`` = 0.5 mean((V - vs)^2), ``entropy`` (of the masked logits) and ``total_loss`` = policy_loss + vf_coeff *
        vf_loss - ent_coeff * entropy, with (vs, pg_adv) = ``vtrace`` of the current network's logp and values against the
        fragment's recorded logp.  A row's log-probability is the sum over its heads and its entropy the sum of their
        entropies."""
        view = fragment_view(frag, self.module) if _view is None else _view
        actions, mu, rewards, ended = (view.take(x, rows) for x in (view.actions, view.logp, view.rewards, view.ended))
        boot = view.take(view.last_value, rows, 0)
        logits, value = _forward(self.module, view, rows, self.fused, self.fused_trunk, self.fused_grads)
        if self.fused and logits.is_cuda:
            scalars = (self.gamma, self.lam, self.clip_rho, self.clip_c, self.clip_pg_rho, self.vf_coeff, self.ent_coeff)
            total, policy_loss, vf_loss, entropy = _VtraceLoss.apply(logits, value, actions, mu, rewards, ended, boot, view.heads, scalars)
            return {"total_loss": total, "policy_loss": policy_loss, "vf_loss": vf_loss, "entropy": entropy}
        return impala_objective(logits, value, actions, mu, rewards, ended, boot, self.gamma, self.lam, self.clip_rho, self.clip_c,
                                self.clip_pg_rho, self.vf_coeff, self.ent_coeff)[0]

    def update(self, frag) -> dict:
        """``epochs`` passes of ``minibatches`` Adam steps over the fragment.  Returns the loss terms averaged over the last
        epoch's minibatches, as tensors on the module's device; nothing is synchronised."""
        view = fragment_view(frag, self.module)
        view.rewards = view.rewards.to(torch.float32)  # (float64 on a joint fragment) once, not in every minibatch
        return self._epochs(view, lambda units: self.losses(frag, units, view))



# ---- behaviour cloning -------------------------------------------------------------------------------------------------------
def bc_objective(logits, expert, values=None, targets=None, vf_coeff: float = 0.0, ent_coeff: float = 0.0, groups: int = 1,
                 per_group: bool = False):
    """The behaviour-cloning loss terms of logits [T, R, 5 heads] (and values [T, R]) in torch ops, in the dtype of the
    logits, differentiable with respect to both: ({nll, vf_loss, entropy, accuracy, total_loss}, {nll, hits}).  expert
    [T, R, heads]: the expert's actions, clamped to 0 .. 4; values and targets [T, R]: both or neither (without them
    vf_loss is 0).  nll is minus the log-probability of the expert's actions summed over a row's heads, entropy the sum of
    the heads' entropies, accuracy the share of heads whose largest logit (the lowest index on ties) is the expert's action,
    total_loss = nll + vf_coeff * vf_loss - ent_coeff * entropy with vf_loss = 0.5 (value - target)^2.  per_group: every
    term is a [groups] tensor, the mean over the rows r with r % groups = g; otherwise a mean over everything.  What
    ``mapf_bc_loss`` computes in one launch; the ``fused_objective=False`` baseline."""
    if (values is None) != (targets is None):
        raise ValueError("values and targets: both or neither")
    heads = int(expert.shape[2])
    x = logits.unflatten(2, (heads, NUM_ACTIONS))
    logp_all = torch.log_softmax(x, dim=3)
    e = expert.to(torch.int64).clamp(0, NUM_ACTIONS - 1)
    nll = -logp_all.gather(3, e[..., None])[..., 0].sum(dim=2)
    ids = torch.arange(NUM_ACTIONS, device=x.device)
    top = torch.where(x == x.max(dim=3, keepdim=True).values, ids, NUM_ACTIONS).min(dim=3).values  # the lowest index of the maximum
    hits = (top == e).sum(dim=2)

    def mean(v):  # [T, R'] -> one number, or one per policy
        return v.unflatten(1, (-1, groups)).mean(dim=(0, 1)) if per_group else v.mean()

    per = {"nll": mean(nll),
           "vf_loss": mean(0.5 * (values - targets.to(values.dtype)) ** 2).to(logits.dtype) if values is not None else mean(torch.zeros_like(nll)),
           "entropy": mean(-(torch.exp(logp_all) * logp_all).flatten(2).sum(dim=2)),
           "accuracy": mean(hits.to(logits.dtype)).detach() / heads}
    per["total_loss"] = per["nll"] + vf_coeff * per["vf_loss"] - ent_coeff * per["entropy"]
    return per, {"nll": nll, "hits": hits}


class _BCLoss(torch.autograd.Function):
    """``mapf_bc_loss`` as one differentiable op: (total_loss, nll, vf_loss, entropy, accuracy) of logits [T, R, 5 heads] and
    values [T, R] (or None, with targets None), each a [groups] tensor of per-policy means; forward is the one launch plus the
    sum of the tiles' partials, backward scales the gradients the launch left behind, every group's by its own total's.  Only
    total_loss is differentiable."""

    @staticmethod
    def forward(ctx, logits, values, expert, targets, heads, groups, scalars):
        lib = L.load()
        T, R, heads, G = int(logits.shape[0]), int(logits.shape[1]), int(heads), int(groups)
        ctx.dtypes = (logits.dtype, None if values is None else values.dtype)
        lg = f32c(logits)
        expert = expert.to(torch.int8).contiguous()
        dev = lg.device
        if G < 1 or R % G:
            raise ValueError(f"{R} rows are no whole number of {G} interleaved groups")
        if (values is None) != (targets is None):
            raise ValueError("values and targets: both or neither")
        # the kernel takes raw pointers: every tensor on the logits' device, of the shape the launch walks
        checked = [("expert", expert, (T, R, heads)), ("logits", lg, (T, R, NUM_ACTIONS * heads))]
        v = None
        if values is not None:
            v, targets = f32c(values), f32c(targets)
            checked += [("values", v, (T, R)), ("targets", targets, (T, R))]
        for name, x, shape in checked:
            if x.device != dev or tuple(x.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)} on {dev}, got {list(x.shape)} on {x.device}")
        dlogits = torch.empty_like(lg) if ctx.needs_input_grad[0] else None
        dvalues = torch.empty_like(v) if v is not None and ctx.needs_input_grad[1] else None
        partials = torch.empty((int(lib.mapf_bc_partials(R, G)), 5), dtype=torch.float32, device=dev)
        rc = lib.mapf_bc_loss(T, R, heads, G, ptr(lg), ptr(expert), ptr(v), ptr(targets), *scalars, None, ptr(dlogits), ptr(dvalues),
                              ptr(partials), stream_of(dev))
        if rc != L.MAPF_OK:
            raise RuntimeError(f"mapf_bc_loss failed (code {rc})")
        ctx.grads, ctx.groups = (dlogits, dvalues), G
        nll, vf, entropy, hits, total = (partials.view(G, -1, 5).sum(1) * (G / (T * R))).unbind(1)
        accuracy = hits / heads
        ctx.mark_non_differentiable(nll, vf, entropy, accuracy)
        return total, nll, vf, entropy, accuracy

    @staticmethod
    def backward(ctx, g, *_unused):
        dlogits, dvalues = ctx.grads
        G = ctx.groups
        if dlogits is not None:  # row r is group r % G: [T, R / G, G, .] times g [G]
            dlogits = (dlogits.unflatten(1, (-1, G)) * g[:, None]).flatten(1, 2).to(ctx.dtypes[0])
        if dvalues is not None:
            dvalues = (dvalues.unflatten(1, (-1, G)) * g).flatten(1, 2).to(ctx.dtypes[1])
        return (dlogits, dvalues) + (None,) * 5


# tools/time_bc.py: the objective forward + backward at T = 32 fused / torch ops 0.21 / 0.59 ms (12 / 59 kernels) at 8 192 rows
# and 0.22 / 0.62 ms at 65 536, the fused objective faster in every one of three alternating rounds at both sizes
BC_FUSED_DEFAULT = True


class BCLearner(_MinibatchLearner):
    """Behaviour cloning with Adam on a ``MaskedRecurrentPolicy``, a ``JointActionPolicy`` (the wide net included) or a
    ``PerAgentPolicy``: the fragment's ``expert_actions`` (``Rollout(expert=...)``) are the labels of a cross-entropy on the
    network's masked logits.  With a ``PerAgentPolicy`` it is N independent learners in one, as ``PPOLearner`` is: every term
    a per-policy mean, ``grad_clip`` on each policy's own gradient norm, ``total_loss`` the sum of the N totals.

    vf_coeff > 0: ``needs_gae`` is set and ``update(frag, adv, targets)`` also regresses the value head to ``gae``'s value
    targets (0.5 (value - target)^2), so that a cloned checkpoint carries a value function PPO can start from; with 0 the
    value head is left alone and ``update(frag)`` is the whole call.  ent_coeff: an entropy bonus, as in PPO.
    expert / expert_window / beta_schedule: what ``Trainer`` builds its rollout with -- the planner that labels the steps and
    the DAgger mixing share as (iteration, beta) points, piecewise linear between them and constant outside
    (``dqn.epsilon_at``'s rule); a number means that constant.
    fused_objective (GPU only): the objective and its gradients in one launch of ``mapf_bc_loss`` instead of elementary
    torch ops; None: ``BC_FUSED_DEFAULT``.  It needs the built library; there is no fallback.  CPU tensors always take the
    torch ops.  fused: the recurrence on the sequence kernels, as in ``PPOLearner``."""

    def __init__(self, module, lr: float = 1e-3, vf_coeff: float = 0.0, ent_coeff: float = 0.0, epochs: int = 1,
                 minibatches: int = 8, grad_clip=None, seed: int = 0, fused: bool = True, fused_objective: bool | None = None,
                 expert: str = "yielding", expert_window: int = 8, beta_schedule=0.0, fused_trunk: bool = False,
                 fused_grads: bool = False):
        if isinstance(module, PopulationPolicy):
            raise ValueError("a PopulationPolicy is not supported by BCLearner; PPOLearner takes a PopulationPolicy")
        super().__init__(module, lr, epochs, minibatches, grad_clip, seed, fused, fused_trunk, fused_grads)
        for name, x in (("vf_coeff", vf_coeff), ("ent_coeff", ent_coeff)):  # what mapf_bc_loss refuses, refused here by name
            if not math.isfinite(float(x)) or float(x) < 0:
                raise ValueError(f"{name} must be finite and >= 0, got {x}")
        self.vf_coeff, self.ent_coeff = float(vf_coeff), float(ent_coeff)
        self.needs_gae = self.vf_coeff > 0
        self.fused_objective = BC_FUSED_DEFAULT if fused_objective is None else bool(fused_objective)
        if isinstance(beta_schedule, (int, float)):
            beta_schedule = [(0, float(beta_schedule))]
        self.beta_schedule = [(int(i), float(b)) for i, b in beta_schedule]
        if not self.beta_schedule:
            raise ValueError("beta_schedule needs at least one (iteration, beta) point")
        self.expert, self.expert_window = expert, int(expert_window)
        for _i, b in self.beta_schedule:
            check_expert(expert, module.rows_are_envs, expert_window, b)

    def rollout_options(self) -> dict:
        """What ``Trainer`` passes to the rollout it builds: the expert and the schedule's first beta."""
        return {"expert": self.expert, "expert_window": self.expert_window, "beta": self.beta_at(0)}

    def beta_at(self, iteration: int) -> float:
        return epsilon_at(self.beta_schedule, int(iteration))

    def losses(self, frag, targets=None, rows=None, _view=None) -> dict:
        """The loss terms on the units ``rows`` (None: all), means over [T, R']: ``nll`` (minus the log-probability of the
        expert's actions, summed over a row's heads), ``accuracy`` (the share of heads whose greedy action is the expert's),
        ``vf_loss`` (0.5 (value - target)^2; 0 without ``targets``), ``entropy`` and ``total_loss`` = nll + vf_coeff * vf_loss
        - ent_coeff * entropy.  With a ``PerAgentPolicy`` also ``per_policy``, the terms as [N] tensors; ``total_loss`` is then
        their totals' SUM and the others are means over the policies."""
        if "expert_actions" not in frag:
            raise ValueError("the fragment has no 'expert_actions': build the rollout with an expert, Rollout(expert=...) or "
                             "JointRollout(expert=...) (Trainer does for a BCLearner)")
        view = fragment_view(frag, self.module) if _view is None else _view
        T, R = view.T, view.R
        if tuple(frag["expert_actions"].shape) != tuple(frag["actions"].shape):
            raise ValueError(f"fragment['expert_actions'] must be {list(frag['actions'].shape)} like the actions, got "
                             f"{list(frag['expert_actions'].shape)}")
        if self.needs_gae and targets is None:
            raise ValueError("a BCLearner with vf_coeff > 0 needs gae's value targets: update(frag, adv, targets)")
        logits, value = _forward(self.module, view, rows, self.fused, self.fused_trunk, self.fused_grads)
        expert = view.take(frag["expert_actions"].reshape(T, R, view.heads), rows)
        tg = view.take(targets.reshape(T, R), rows) if self.needs_gae else None
        value = value if self.needs_gae else None
        names = ("nll", "accuracy", "vf_loss", "entropy", "total_loss")
        if self.fused_objective and logits.is_cuda:
            total, nll, vf_loss, entropy, accuracy = _BCLoss.apply(logits, value, expert, tg, view.heads, view.groups,
                                                                   (self.vf_coeff, self.ent_coeff))
            per = {"nll": nll, "accuracy": accuracy, "vf_loss": vf_loss, "entropy": entropy, "total_loss": total}
            per = {k: per[k] if view.agent_axis else per[k][0] for k in names}
        else:
            per = bc_objective(logits, expert, value, tg, self.vf_coeff, self.ent_coeff, view.groups, view.agent_axis)[0]
            per = {k: per[k] for k in names}
        if not view.agent_axis:
            return per
        return {"total_loss": per["total_loss"].sum(), **{k: per[k].mean() for k in names[:-1]}, "per_policy": per}

    def update(self, frag, adv=None, targets=None) -> dict:
        """``epochs`` passes of ``minibatches`` Adam steps over the fragment.  adv is not used (the signature is
        ``PPOLearner.update``'s, for ``Trainer``); targets: ``gae``'s value targets, needed exactly when vf_coeff > 0.  Returns
        ``nll``, ``accuracy``, ``vf_loss``, ``entropy`` and ``total_loss`` averaged over the last epoch's minibatches, as
        tensors on the module's device; nothing is synchronised.  With a ``PerAgentPolicy`` they are averaged over the
        policies as well, plus ``per_policy``."""
        if "expert_actions" not in frag:
            raise ValueError("the fragment has no 'expert_actions': build the rollout with an expert, Rollout(expert=...) or "
                             "JointRollout(expert=...) (Trainer does for a BCLearner)")
        view = fragment_view(frag, self.module)
        return self._epochs(view, lambda units: self.losses(frag, targets, units, view))


class Trainer:
    """collect -> gae -> update -> load_params, one fragment of T steps per ``iterate()``.  The module must live on the env's
    device; the trainer owns the ``DevicePolicy`` and the ``Rollout`` that run it -- for a ``JointActionPolicy`` on a
    ``VecSingleAgentReferenceModel`` the ``JointDevicePolicy`` and the ``JointRollout``; a ``PerAgentPolicy`` (DTE, PPO only)
    is taken as it is, with one policy for each of the env's agents.  With an ``IMPALALearner`` there is
    no ``gae`` step (gamma and lam are the learner's).  push_every: the device policy takes the module's parameters every
    ``push_every`` iterations, so with more than 1 the behaviour policy lags the learner, which is what V-trace corrects.
    With a ``BCLearner`` the rollout is built with the learner's expert options, ``iterate()`` sets the rollout's ``beta`` to
    the learner's schedule at the iteration it starts and reports it, and ``gae`` runs only when the learner regresses the
    value head.  guidance: the rollout's option (``Rollout(guidance=True)``: the module's ``obs_len`` is then the env's + 6);
    the learners read ``frag["obs"]`` as they find it.  fused_grads: turns the learner's option of that name on (the
    parameter gradients from ``mapf_lstm_seq_param_grad`` / ``mapf_trunk_param_grad``)."""

    # rows are envs (a joint policy) or agents: what acts on them and what collects their fragment
    RUNNERS = {True: (lambda module, R, N, device: JointDevicePolicy(module, R, device), JointRollout), False: (DevicePolicy, Rollout)}

    def __init__(self, env, module, T: int = 32, learner: PPOLearner | IMPALALearner | BCLearner | None = None, gamma: float = 0.99,
                 lam: float = 0.95, sample_seed: int = 0, push_every: int = 1, guidance: bool = False, fused_grads: bool = False):
        if int(push_every) < 1:
            raise ValueError(f"push_every must be >= 1, got {push_every}")
        self.push_every = int(push_every)
        if guidance and not module.rows_are_envs:  # before a device policy is asked for a row no kernel takes
            check_guidance_fits(env.obs_len)
        dev = next(module.parameters()).device
        if dev != env.device:
            raise ValueError(f"the module is on {dev}, the env on {env.device}")
        self.env, self.module, self.gamma, self.lam = env, module, float(gamma), float(lam)
        self.learner = learner if learner is not None else PPOLearner(module)
        if self.learner.module is not module:
            raise ValueError("the learner optimises another module")
        if fused_grads:  # (a learner built with the option keeps it either way)
            self.learner.fused_grads = True
        layout = _layout(module.rows_are_envs, module, env.num_envs, env.num_agents)
        make_policy, make_rollout = self.RUNNERS[module.rows_are_envs]
        self.policy = make_policy(module, layout["R"], env.num_agents, env.device)
        keep = {"keep_logits": True} if getattr(self.learner, "kl_coeff", None) is not None else {}  # what its KL term reads
        if isinstance(self.learner, BCLearner):  # what its labels and its mixing need
            keep.update(self.learner.rollout_options())
        if guidance:  # (JointRollout refuses it by name)
            keep["guidance"] = True
        self.rollout = make_rollout(env, self.policy, T, sample=True, seed=sample_seed, **keep)
        self._adv = torch.empty((int(T), *layout["per_row"]), dtype=torch.float32, device=env.device)
        self._targets = torch.empty_like(self._adv)
        self.iterations = 0

    def iterate(self) -> dict:
        """One training iteration; synchronises once, at the end, to hand back Python numbers: ``reward_per_step`` (mean
        over agents and steps), ``episodes`` ended in the fragment, of which ``terminated`` (every agent reached its goal)
        and ``truncated`` (the time limit, at which the engine raises both flags), and the learner's loss terms; with a
        ``BCLearner`` also ``beta``, the mixing share the fragment was collected with."""
        beta = None
        if isinstance(self.learner, BCLearner):
            beta = self.rollout.beta = self.learner.beta_at(self.iterations)
        frag = self.rollout.collect()
        if self.learner.needs_gae:
            adv, targets = gae(frag, self.gamma, self.lam, out=(self._adv, self._targets))
            terms = self.learner.update(frag, adv, targets)
        else:
            terms = self.learner.update(frag)
        if (self.iterations + 1) % self.push_every == 0:
            self.policy.load_params(self.module)
        per_policy = terms.pop("per_policy", None)
        term, trunc = frag["terminated"] != 0, frag["truncated"] != 0
        names = ["reward_per_step", "episodes", "terminated", "truncated"] + list(terms)
        vals = [frag["rewards"].mean(), (term | trunc).sum(), (term & ~trunc).sum(), trunc.sum()] + list(terms.values())
        host = torch.stack([v.to(torch.float32) for v in vals]).cpu()  # the iteration's one synchronisation
        self.iterations += 1
        out = {k: float(v) for k, v in zip(names, host.tolist())}
        for k in ("episodes", "terminated", "truncated"):
            out[k] = int(out[k])
        out["iteration"] = self.iterations
        if beta is not None:
            out["beta"] = beta
        if per_policy is not None:  # (after the synchronisation above)
            out["per_policy"] = {k: v.tolist() for k, v in per_policy.items()}
        return out
