"""DQN on the device (the reference's ``ALGO_NAME = "DQN"``, src/agents/dqn.py; include/mapf_step.h, "DQN", states every rule).

``QNetwork`` is the dueling 32-32 feed-forward net in plain torch (differentiable: what the learner optimises and what the
act kernel is compared with); ``DeviceQPolicy`` runs it as ONE launch per step (``mapf_qnet_act``) with epsilon-greedy
exploration whose epsilon lies in device memory.  ``QRollout`` is the loop of ``rollout.Rollout`` on it, ``ReplayBuffer`` a
ring of time slots next to the rollout slabs with integer priorities, sampled by ``mapf_replay_sample``; ``td_objective`` is
the double-Q Huber objective in torch ops and ``_TDLoss`` the same as one launch of ``mapf_dqn_td_loss``.  ``DQNLearner`` and
``DQNTrainer`` put them together.  The kernels have no fallback: without the built library the device classes raise.

DTE (one net per agent) and CTE are out of scope: the reference refuses CTE for DQN, and so does ``DQNTrainer``.
"""

from __future__ import annotations

import copy
import ctypes as C

import torch

from . import _lib as L
from .device_net import Checkpoint, DeviceNet, GraphedFragment, check_rc, f32c, ptr, stream_of
from .policy import PerAgentPolicy, PopulationPolicy
from .vec_env import VecReferenceModel

HIDDEN = L.QNET_HIDDEN
NUM_ACTIONS = 5
W_ONE = 1 << 16  # the weight of |td| + 1e-6 = 1, and of a transition no priority update has seen yet (before any update)
W_MAX = 1 << 20
PRIORITY_EPS = 1e-6

# tools/time_dqn.py: the objective forward + backward at K = 4 000 fused / torch ops 0.111 / 0.407 ms, one iteration at the
# reference's training setup 5.59 / 6.48 ms, the fused path faster in every one of three alternating rounds
DQN_FUSED_DEFAULT = True


class QNetwork(Checkpoint, torch.nn.Module):
    """obs [R, L] -> q [R, 5]: a1 = tanh(fc1 obs), a2 = tanh(fc2 a1), q = val + adv - mean(adv).  The whole observation is
    the feature vector; mask floats, if the env emits them, are features."""

    KIND = "q_network"
    LOADER = "dqn.QNetwork.load"

    def __init__(self, obs_len: int, hidden: int = HIDDEN):
        super().__init__()
        self.obs_len, self.hidden = int(obs_len), int(hidden)
        if self.obs_len < 1:
            raise ValueError(f"obs_len {obs_len} leaves no feature")
        self.fc1 = torch.nn.Linear(self.obs_len, self.hidden)
        self.fc2 = torch.nn.Linear(self.hidden, self.hidden)
        self.adv = torch.nn.Linear(self.hidden, NUM_ACTIONS)
        self.val = torch.nn.Linear(self.hidden, 1)

    def config(self) -> dict:
        return {"obs_len": self.obs_len, "hidden": self.hidden}

    def forward(self, obs):
        a2 = torch.tanh(self.fc2(torch.tanh(self.fc1(obs))))
        adv = self.adv(a2)
        return self.val(a2) + adv - adv.mean(dim=-1, keepdim=True)


class DeviceQPolicy(DeviceNet):
    """``QNetwork`` as one launch per step (``mapf_qnet_act``) on ``rows`` agent rows.

    ``act`` returns the policy's own output tensors (overwritten by the next call): ``action`` int8 [rows] and ``q`` float32
    [rows, 5]; ``draws`` (uint32 counters in int32 storage) is its state.  Nothing is synchronised and nothing is allocated
    per call, so a loop of ``act`` and env steps can be captured into a graph from the first call."""

    def __init__(self, module_or_path, rows: int, device="cuda:0"):
        module = self._module(QNetwork, module_or_path, "DeviceQPolicy needs a QNetwork (DevicePolicy runs a MaskedRecurrentPolicy)")
        super().__init__("mapf_qnet", device)
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError(f"rows = {rows} must be positive")
        self.obs_len = module.obs_len
        self._create(L.MapfQnetConfig(self.obs_len, module.hidden, int(self.device.index)), module)
        dev, R = self.device, self.rows
        self.draws = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.action = torch.zeros((R,), dtype=torch.int8, device=dev)
        self.q = torch.zeros((R, NUM_ACTIONS), dtype=torch.float32, device=dev)
        self.epsilon = torch.zeros((1,), dtype=torch.float32, device=dev)  # what act(epsilon=<number>) writes and passes
        self.load_params(module)

    def reset_state(self) -> None:
        self.draws.zero_()

    def act_raw(self, obs_ptr, epsilon_ptr, mode: int, seed: int, out=None, stream=None) -> None:
        """``mapf_qnet_act`` on raw device pointers (ints or None) with the policy's own draw counters; out: (action, q)
        pointers, default the policy's own tensors."""
        if out is None:
            out = (self.action.data_ptr(), self.q.data_ptr())
        self._act((obs_ptr, epsilon_ptr, self.draws.data_ptr()), seed, mode, out, stream)

    def act(self, obs, epsilon=None, peek: bool = False, seed: int = 0) -> dict:
        """One step of every row.  obs float32 [rows, L] (or [B, N, L]); epsilon: None (greedy), a one-float tensor on the
        policy's device (read by the launch, so a captured graph follows it) or a number (written into ``self.epsilon``);
        peek: leave ``draws`` as it is."""
        obs = self._input(obs, torch.float32, self.rows * self.obs_len, "obs")
        if epsilon is not None and not isinstance(epsilon, torch.Tensor):
            self.epsilon.fill_(float(epsilon))
            epsilon = self.epsilon
        if epsilon is not None and (epsilon.dtype != torch.float32 or epsilon.device != self.device or epsilon.numel() != 1):
            raise ValueError("epsilon must be one float32 on the policy's device")
        self.act_raw(ptr(obs), ptr(epsilon), L.QNET_PEEK if peek else 0, seed)
        return {"action": self.action, "q": self.q}


class QRollout(GraphedFragment):
    """T x (``mapf_qnet_act`` -> ``mapf_step`` with auto-reset), two launches per step, written in place into [T + 1]-deep
    slabs.  ``epsilon`` is a one-float device tensor the act reads; whoever trains writes it.  The first ``collect()``
    launches, the second captures the fragment into a graph and every later one replays it."""

    def __init__(self, env: VecReferenceModel, policy: DeviceQPolicy, T: int, seed: int = 0):
        if not isinstance(env, VecReferenceModel):
            raise TypeError("QRollout needs a VecReferenceModel (DQN has no CTE mode)")
        if not isinstance(policy, DeviceQPolicy):
            raise TypeError("QRollout needs a DeviceQPolicy")
        B, N, Lo = env.num_envs, env.num_agents, env.obs_len
        if policy.rows != B * N or policy.obs_len != Lo or policy.device != env.device:
            raise ValueError("the policy's rows, obs_len and device must be the env's")
        self.env, self.policy, self.T, self.seed = env, policy, int(T), int(seed)
        if self.T < 1:
            raise ValueError(f"T must be >= 1, got {T}")
        T, dev = self.T, env.device
        f32, u8 = torch.float32, torch.uint8
        self._obs = torch.zeros((T + 1, B, N, Lo), dtype=f32, device=dev)
        self._rew = torch.zeros((T + 1, B, N), dtype=f32, device=dev)
        self._term = torch.zeros((T + 1, B), dtype=u8, device=dev)
        self._trunc = torch.zeros((T + 1, B), dtype=u8, device=dev)
        self._act = torch.zeros((T, B, N), dtype=torch.int8, device=dev)
        self.epsilon = torch.ones((1,), dtype=f32, device=dev)
        self._obs[T].copy_(env.reset())
        policy.reset_state()
        self._graph = None
        self._calls = 0
        self._out = {"obs": self._obs, "actions": self._act, "rewards": self._rew[1:], "terminated": self._term[1:],
                     "truncated": self._trunc[1:]}

    def _launch(self) -> None:
        env, pol, T = self.env, self.policy, self.T
        lib, h = env._lib, env._h
        self._obs[0].copy_(self._obs[T])
        stream = pol._stream()
        info_all, info_agent = env._info_all.data_ptr(), env._info_agent.data_ptr()
        eps = self.epsilon.data_ptr()
        for t in range(T):
            pol.act_raw(self._obs[t].data_ptr(), eps, 0, self.seed, out=(self._act[t].data_ptr(), None), stream=stream)
            rc = lib.mapf_step(h, self._act[t].data_ptr(), self._obs[t + 1].data_ptr(), self._rew[t + 1].data_ptr(),
                               self._term[t + 1].data_ptr(), self._trunc[t + 1].data_ptr(), info_all, info_agent, None, 1, stream)
            if rc != 0:
                env._check(rc)

    def collect(self) -> dict:
        """One fragment of T steps.  Returns views of the preallocated slabs (overwritten by the next call): ``obs``
        [T + 1, B, N, L] (``obs[t]`` is what act t saw, ``obs[T]`` the observation after the last step -- after an episode's
        end the next episode's first one), ``actions`` int8 [T, B, N], ``rewards`` [T, B, N], ``terminated`` and
        ``truncated`` uint8 [T, B]."""
        return super().collect()


def _segments(start: int, n: int, S: int):
    """[(first slot, first step, steps)]: the slots start .. start + n - 1 (mod S) as at most two contiguous runs."""
    start %= S
    first = min(n, S - start)
    return [(start, 0, first)] + ([(0, first, n - first)] if n > first else [])


class ReplayBuffer:
    """A ring of ``S = ceil(capacity / rows) + 1`` time slots (at least 2) of ``rows`` agent rows.  ``obs`` [S, R, L];
    ``action`` int8, ``reward`` float32, ``ended`` uint8 [S, R] stored at the slot of the observation the action was taken
    from; ``w`` [S, R] the integer weights (uint32 values in int32 storage).  Transition (g, row) is (obs[g], action[g],
    reward[g], ended[g], obs[(g + 1) % S]); its weight is non-zero exactly while both observations are in the ring, and the
    head slot (the latest observation, no action yet) has weight 0.  ``w_max`` (a device tensor) is the largest weight any
    priority update has written, 2^16 before the first.  Nothing here synchronises; ``append`` is a fixed number of copies
    (at most two runs per tensor) and allocates only in its first call (one [T, B] scratch for terminated | truncated)."""

    def __init__(self, rows: int, obs_len: int, capacity: int, device="cuda:0"):
        self.rows, self.obs_len, self.capacity = int(rows), int(obs_len), int(capacity)
        if self.rows < 1 or self.obs_len < 1 or self.capacity < 1:
            raise ValueError("rows, obs_len and capacity must be >= 1")
        self.device = torch.device(device)
        self.slots = max(2, -(-self.capacity // self.rows) + 1)
        S, R, dev = self.slots, self.rows, self.device
        self.count = S * R
        if self.count > L.REPLAY_MAX_COUNT:
            raise ValueError(f"{S} slots of {R} rows are {self.count} weights, more than {L.REPLAY_MAX_COUNT}")
        self.obs = torch.zeros((S, R, self.obs_len), dtype=torch.float32, device=dev)
        self.action = torch.zeros((S, R), dtype=torch.int8, device=dev)
        self.reward = torch.zeros((S, R), dtype=torch.float32, device=dev)
        self.ended = torch.zeros((S, R), dtype=torch.uint8, device=dev)
        self.w = torch.zeros((S, R), dtype=torch.int32, device=dev)
        self.w_max = torch.full((1,), W_ONE, dtype=torch.int32, device=dev)
        self._amax = torch.zeros((1,), dtype=torch.int32, device=dev)
        self.head = 0       # the slot of the latest observation
        self.steps = 0      # time steps appended so far
        self._ended_tb = None
        self._draws = torch.zeros((1,), dtype=torch.int32, device=dev)
        self._sample = {}   # K -> (idx, wk, stats, workspace)

    @property
    def stored(self) -> int:
        """Live transitions."""
        return min(self.steps, self.slots - 1) * self.rows

    def append(self, frag: dict) -> None:
        """The T steps of a ``QRollout`` fragment (T <= S - 1).  New transitions get weight ``w_max``; the new head's weights
        are 0.  The first append also stores ``obs[0]``; every later one relies on its ``obs[0]`` being the head's
        observation, as consecutive fragments of one rollout are."""
        S, R, Lo = self.slots, self.rows, self.obs_len
        obs, act, rew = frag["obs"], frag["actions"], frag["rewards"]
        T = int(act.shape[0])
        if T > S - 1:
            raise ValueError(f"a fragment of {T} steps does not fit a ring of {S} slots (T <= S - 1)")
        if obs.shape[0] != T + 1 or obs[0].numel() != R * Lo or act[0].numel() != R:
            raise ValueError("the fragment's shapes are not the buffer's")
        term, trunc = frag["terminated"], frag["truncated"]
        B = int(term.shape[1])
        if self._ended_tb is None or self._ended_tb.shape != term.shape:
            self._ended_tb = torch.zeros_like(term)
        torch.bitwise_or(term, trunc, out=self._ended_tb)
        ended = self._ended_tb[:, :, None].expand(T, B, R // B)
        obs, act, rew = obs.reshape(T + 1, R, Lo), act.reshape(T, R), rew.reshape(T, R)
        if self.steps == 0:
            self.obs[self.head].copy_(obs[0])
        for s0, t0, n in _segments(self.head, T, S):
            self.action[s0:s0 + n].copy_(act[t0:t0 + n])
            self.reward[s0:s0 + n].copy_(rew[t0:t0 + n])
            self.ended[s0:s0 + n].view(n, B, R // B).copy_(ended[t0:t0 + n])
            self.w[s0:s0 + n].copy_(self.w_max.expand(n, R))
        for s0, t0, n in _segments(self.head + 1, T, S):
            self.obs[s0:s0 + n].copy_(obs[t0 + 1:t0 + 1 + n])
        self.head = (self.head + T) % S
        self.w[self.head].zero_()
        self.steps += T

    def sample(self, K: int, seed: int = 0):
        """``mapf_replay_sample``: (idx int32 [K], wk int32 [K], stats int64 [2] = (W, n_valid)), the buffer's own tensors
        (overwritten by the next call with the same K); the buffer's draw counter advances by one."""
        if self.device.type != "cuda":
            raise ValueError("ReplayBuffer.sample runs on the GPU only (there is no CPU path)")
        K = int(K)
        if K not in self._sample:
            lib = L.load()
            nbytes = int(lib.mapf_replay_sample_workspace_bytes(self.count))
            self._sample[K] = (torch.zeros((K,), dtype=torch.int32, device=self.device),
                               torch.zeros((K,), dtype=torch.int32, device=self.device),
                               torch.zeros((2,), dtype=torch.int64, device=self.device),
                               torch.zeros((nbytes // 8 + 1,), dtype=torch.int64, device=self.device))
        idx, wk, stats, ws = self._sample[K]
        rc = L.load().mapf_replay_sample(ptr(self.w), self.count, K, ptr(self._draws), C.c_uint64(int(seed) & (2**64 - 1)),
                                         ptr(ws), ptr(idx), ptr(wk), ptr(stats), stream_of(self.device))
        check_rc(rc, "mapf_replay_sample")
        return idx, wk, stats

    def gather(self, idx):
        """(obs, next_obs, action, reward, ended) of the transitions ``idx`` (flat indices g * R + row)."""
        i = idx.to(torch.int64)
        nxt = (i + self.rows) % self.count
        flat = self.obs.view(self.count, self.obs_len)
        return flat[i], flat[nxt], self.action.view(-1)[i], self.reward.view(-1)[i], self.ended.view(-1)[i]

    def note_priorities(self, new_w) -> None:
        """``w_max`` after a priority update that wrote ``new_w``."""
        torch.amax(new_w, dim=0, keepdim=True, out=self._amax)
        torch.maximum(self.w_max, self._amax, out=self.w_max)

    def update_priorities(self, idx, new_w) -> None:
        """w[idx] = new_w in torch ops (the fused objective scatters them itself)."""
        self.w.view(-1).index_copy_(0, idx.to(torch.int64), new_w.to(torch.int32))
        self.note_priorities(new_w)


def importance_weights(wk, stats, beta: float):
    """isw = (n_valid * wk / W)^(-beta), divided by the batch's largest."""
    W, n_valid = stats[0].to(torch.float64), stats[1].to(torch.float64)
    isw = (n_valid * wk.to(torch.float64) / W) ** (-float(beta))
    return (isw / isw.max()).to(torch.float32)


def priority(td_abs64, alpha: float):
    """clamp(rint((|td| + 1e-6)^alpha * 2^16), 1, 2^20) of a float64 tensor, as int32."""
    p = torch.round((td_abs64 + PRIORITY_EPS) ** float(alpha) * float(W_ONE))  # half to even, as rint
    return torch.nan_to_num(p, nan=1.0).clamp(1.0, float(W_MAX)).to(torch.int32)


def td_objective(q, qn_online, qn_target, action, reward, ended, isw, gamma: float = 0.99, delta: float = 1.0,
                 alpha: float = 0.6) -> dict:
    """The rule of ``mapf_dqn_td_loss`` in torch ops, in q's dtype; differentiable with respect to q.  ``loss``, ``td`` [K],
    ``abs_td`` (its mean magnitude) and ``new_w`` int32 [K] (from |td| in float64 with gamma and alpha rounded to fp32, as
    the kernel takes them)."""
    a = action.to(torch.int64).clamp(0, NUM_ACTIONS - 1)
    done = ended != 0
    with torch.no_grad():
        best = qn_online.argmax(dim=-1, keepdim=True)  # the first of several maxima
        qt = qn_target.gather(-1, best)[:, 0]
        y = torch.where(done, reward.to(q.dtype), reward.to(q.dtype) + gamma * qt.to(q.dtype))
    qa = q.gather(-1, a[:, None])[:, 0]
    td = qa - y
    ad = td.abs()
    l = torch.where(ad <= delta, 0.5 * td * td, delta * (ad - 0.5 * delta))
    loss = (isw.to(q.dtype) * l).mean()
    with torch.no_grad():
        g32 = float(torch.tensor(gamma, dtype=torch.float32))
        a32 = float(torch.tensor(alpha, dtype=torch.float32))
        y64 = torch.where(done, reward.double(), reward.double() + g32 * qt.double())
        new_w = priority((qa.detach().double() - y64).abs(), a32)
    return {"loss": loss, "td": td, "abs_td": ad.detach().mean(), "new_w": new_w}


class _TDLoss(torch.autograd.Function):
    """``mapf_dqn_td_loss`` as one differentiable op: (loss, mean |td|, new_w) of q [K, 5]; forward is the one launch plus
    the sum of the workgroups' partials, backward scales the gradient the launch left behind.  With ``idx`` and ``weights``
    the launch also writes the new priorities into the ring.  Only loss is differentiable."""

    @staticmethod
    def forward(ctx, q, qn_online, qn_target, action, reward, ended, isw, scalars, idx, weights):
        lib = L.load()
        K = int(q.shape[0])
        ctx.dtype = q.dtype
        qf, on, tg, reward, isw = f32c(q), f32c(qn_online), f32c(qn_target), f32c(reward), f32c(isw)
        action, ended = action.to(torch.int8).contiguous(), ended.to(torch.uint8).contiguous()
        dev = qf.device
        if dev.type != "cuda":
            raise ValueError("the fused TD objective runs on the GPU only (td_objective is the CPU path)")
        for name, x, shape in (("q", qf, (K, NUM_ACTIONS)), ("qn_online", on, (K, NUM_ACTIONS)), ("qn_target", tg, (K, NUM_ACTIONS)),
                               ("action", action, (K,)), ("reward", reward, (K,)), ("ended", ended, (K,)), ("isw", isw, (K,))):
            if x.device != dev or tuple(x.shape) != shape:
                raise ValueError(f"{name} must be {list(shape)} on {dev}, got {list(x.shape)} on {x.device}")
        count = 0
        if idx is not None:
            if idx.dtype != torch.int32 or weights.dtype != torch.int32 or idx.device != dev or weights.device != dev \
                    or idx.numel() != K or not idx.is_contiguous() or not weights.is_contiguous():
                raise ValueError(f"idx must be int32 [{K}] and weights a contiguous int32 tensor on {dev}")
            count = weights.numel()
        dq = torch.empty_like(qf) if ctx.needs_input_grad[0] else None
        new_w = torch.empty((K,), dtype=torch.int32, device=dev)
        partials = torch.empty((int(lib.mapf_dqn_td_partials(K)), 2), dtype=torch.float32, device=dev)
        rc = lib.mapf_dqn_td_loss(K, ptr(qf), ptr(on), ptr(tg), ptr(action), ptr(reward), ptr(ended), ptr(isw), *scalars,
                                  ptr(idx), ptr(weights) if idx is not None else None, count, None, ptr(dq), ptr(new_w),
                                  ptr(partials), stream_of(dev))
        check_rc(rc, "mapf_dqn_td_loss")
        ctx.dq = dq
        loss, abs_td = (partials.sum(0) * (1.0 / K)).unbind(0)
        ctx.mark_non_differentiable(abs_td, new_w)
        return loss, abs_td, new_w

    @staticmethod
    def backward(ctx, g, *_unused):
        return (None if ctx.dq is None else (ctx.dq * g).to(ctx.dtype),) + (None,) * 9


class DQNLearner:
    """Double dueling DQN with Adam on a ``QNetwork``: prioritised batches of ``train_batch`` transitions from a
    ``ReplayBuffer``, Huber loss weighted by the importance weights, a target copy of the module that takes the module's
    weights every ``target_update_every`` updates, global-norm gradient clipping.  fused (GPU only): the objective, its
    gradient and the priority scatter in one launch of ``mapf_dqn_td_loss``; ``fused=False`` is ``td_objective``."""

    def __init__(self, module: QNetwork, lr: float = 3e-4, gamma: float = 0.99, train_batch: int = 4000, alpha: float = 0.6,
                 beta: float = 0.4, delta: float = 1.0, double_q: bool = True, target_update_every: int = 100, grad_clip=40.0,
                 seed: int = 0, fused: bool = DQN_FUSED_DEFAULT):
        if isinstance(module, PopulationPolicy):
            raise ValueError("a PopulationPolicy is not supported by DQNLearner: populations are PPO on the multi-agent env "
                             "(learner.PPOLearner takes a policy.PopulationPolicy)")
        if isinstance(module, PerAgentPolicy):
            raise ValueError("DTE (one policy per agent) is not supported by DQN: one QNetwork acts for every agent "
                             "(learner.PPOLearner takes a policy.PerAgentPolicy)")
        if not isinstance(module, QNetwork):
            raise TypeError("DQNLearner optimises a QNetwork")
        if not 1 <= int(train_batch) <= L.REPLAY_MAX_SAMPLES:
            raise ValueError(f"train_batch must lie in 1 .. {L.REPLAY_MAX_SAMPLES}, got {train_batch}")
        if not (0 <= gamma <= 1 and 0 <= alpha <= 1 and beta >= 0 and delta > 0 and int(target_update_every) >= 1):
            raise ValueError("gamma and alpha lie in [0, 1], beta >= 0, delta > 0, target_update_every >= 1")
        self.module = module
        self.device = next(module.parameters()).device
        self.target = copy.deepcopy(module).requires_grad_(False)
        self.gamma, self.alpha, self.beta, self.delta = float(gamma), float(alpha), float(beta), float(delta)
        self.train_batch, self.double_q, self.target_update_every = int(train_batch), bool(double_q), int(target_update_every)
        self.grad_clip, self.seed = grad_clip, int(seed)
        self.fused = bool(fused) and self.device.type == "cuda"
        self.optimizer = torch.optim.Adam(module.parameters(), lr=lr)
        self.updates = 0
        self.last_idx = None  # the indices of the latest batch (the sampler's own tensor)

    def _update(self, buffer: ReplayBuffer) -> tuple:
        K = self.train_batch
        idx, wk, stats = buffer.sample(K, self.seed)
        self.last_idx = idx
        isw = importance_weights(wk, stats, self.beta)
        obs, nxt, action, reward, ended = buffer.gather(idx)
        q_all = self.module(torch.cat([obs, nxt], dim=0))  # one online forward on the 2K rows
        q = q_all[:K]
        with torch.no_grad():
            qn_target = self.target(nxt)
        qn_online = q_all[K:].detach() if self.double_q else qn_target
        if self.fused:
            scalars = (C.c_float(self.gamma), C.c_float(self.delta), C.c_float(self.alpha))
            loss, abs_td, new_w = _TDLoss.apply(q, qn_online, qn_target, action, reward, ended, isw, scalars, idx, buffer.w)
            buffer.note_priorities(new_w)
        else:
            o = td_objective(q, qn_online, qn_target, action, reward, ended, isw, self.gamma, self.delta, self.alpha)
            loss, abs_td, new_w = o["loss"], o["abs_td"], o["new_w"]
            buffer.update_priorities(idx, new_w)
        self.optimizer.zero_grad(set_to_none=True)
        loss.backward()
        if self.grad_clip is not None:
            torch.nn.utils.clip_grad_norm_(self.module.parameters(), self.grad_clip)
        self.optimizer.step()
        self.updates += 1
        if self.updates % self.target_update_every == 0:
            self.target.load_state_dict(self.module.state_dict())
        return loss.detach(), abs_td, q.detach().mean()

    def update(self, buffer: ReplayBuffer, updates: int = 1) -> dict:
        """``updates`` times: sample -> gather obs and next obs -> forwards -> objective -> backward -> step -> priorities.
        Returns the means of ``loss``, ``abs_td`` and ``q`` over the updates as device tensors; synchronises nothing."""
        if buffer.device != self.device:
            raise ValueError(f"the buffer is on {buffer.device}, the module on {self.device}")
        out = [self._update(buffer) for _ in range(int(updates))]
        return {k: torch.stack([o[i] for o in out]).mean() for i, k in enumerate(("loss", "abs_td", "q"))}


def epsilon_at(schedule, step: int) -> float:
    """Piecewise linear in vector steps through the (step, epsilon) points of ``schedule``, constant outside them."""
    pts = sorted((int(s), float(e)) for s, e in schedule)
    if step <= pts[0][0]:
        return pts[0][1]
    for (s0, e0), (s1, e1) in zip(pts, pts[1:]):
        if step < s1:
            return e0 + (e1 - e0) * (step - s0) / (s1 - s0)
    return pts[-1][1]


class DQNTrainer:
    """collect -> append -> ``updates`` learner updates (once ``learning_starts`` transitions are stored) -> load_params,
    one fragment of T steps per ``iterate()``.  epsilon is linear in VECTOR steps (one step of every env) and constant
    within a fragment, at the value of the fragment's first step; 1 250 vector steps are RLlib's 10 000 timesteps spread over
    the reference's 8 runners.  The ring holds whole time slots, so its capacity is raised to one fragment where
    ``capacity`` is less (rows x T transitions)."""

    def __init__(self, env, module: QNetwork, T: int = 32, learner: DQNLearner | None = None, capacity: int = 50_000,
                 epsilon=((0, 1.0), (1250, 0.05)), learning_starts: int = 1000, updates: int = 4, seed: int = 0):
        if not isinstance(env, VecReferenceModel):
            raise TypeError("DQNTrainer needs a VecReferenceModel: the reference refuses CTE for DQN, and so does this")
        if isinstance(module, PerAgentPolicy):
            raise ValueError("DTE (one policy per agent) is not supported by DQN: one QNetwork acts for every agent "
                             "(learner.PPOLearner takes a policy.PerAgentPolicy)")
        dev = next(module.parameters()).device
        if dev != env.device:
            raise ValueError(f"the module is on {dev}, the env on {env.device}")
        self.env, self.module, self.T = env, module, int(T)
        self.learner = learner if learner is not None else DQNLearner(module, seed=seed)
        if self.learner.module is not module:
            raise ValueError("the learner optimises another module")
        rows = env.num_envs * env.num_agents
        self.policy = DeviceQPolicy(module, rows, env.device)
        self.rollout = QRollout(env, self.policy, self.T, seed=seed)
        self.buffer = ReplayBuffer(rows, env.obs_len, max(int(capacity), rows * self.T), env.device)
        self.schedule, self.learning_starts, self.updates = tuple(epsilon), int(learning_starts), int(updates)
        self.iterations = 0
        self.vector_steps = 0
        self._zero = torch.zeros((), dtype=torch.float32, device=env.device)

    def iterate(self) -> dict:
        """One training iteration; synchronises once, at the end, to hand back Python numbers: the keys of
        ``Trainer.iterate()`` (``reward_per_step``, ``episodes``, ``terminated``, ``truncated``, the learner's terms -- zeros
        before ``learning_starts`` -- and ``iteration``) plus ``epsilon`` and ``stored``."""
        eps = epsilon_at(self.schedule, self.vector_steps)
        self.rollout.epsilon.fill_(eps)
        frag = self.rollout.collect()
        self.buffer.append(frag)
        self.vector_steps += self.T
        if self.buffer.stored >= self.learning_starts:
            terms = self.learner.update(self.buffer, self.updates)
            self.policy.load_params(self.module)
        else:
            terms = {"loss": self._zero, "abs_td": self._zero, "q": self._zero}
        term, trunc = frag["terminated"] != 0, frag["truncated"] != 0
        names = ["reward_per_step", "episodes", "terminated", "truncated"] + list(terms)
        vals = [frag["rewards"].mean(), (term | trunc).sum(), (term & ~trunc).sum(), trunc.sum()] + list(terms.values())
        host = torch.stack([v.to(torch.float32) for v in vals]).cpu()  # the iteration's one synchronisation
        self.iterations += 1
        out = {k: float(v) for k, v in zip(names, host.tolist())}
        for k in ("episodes", "terminated", "truncated"):
            out[k] = int(out[k])
        out.update(iteration=self.iterations, epsilon=eps, stored=self.buffer.stored)
        return out
