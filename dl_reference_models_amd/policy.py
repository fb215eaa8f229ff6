"""The policies the reference trains (src/agents/ppo.py:67-75, impala.py:54-59: 64-64 dense plus an LSTM of 64 that also
sees the previous action and reward, behind models/action_mask_model.py), twice:

``MaskedRecurrentPolicy`` is the rule of include/mapf_step.h ("Fused recurrent policy") in plain torch: differentiable, so
it is what a learner optimises, and what the fused kernel is compared with.

``DevicePolicy`` runs the same rule as ONE launch per step for every agent of every env (``mapf_policy_act``): it owns the
LSTM state, the draw counters of the sampler and the output tensors, and takes its weights from a module
(``load_params``, one small launch, asynchronous -- a learner can push weights every iteration).  There is no fallback:
without the built library it raises.

``PerAgentPolicy`` is N ``MaskedRecurrentPolicy`` side by side, one per agent (the reference's DTE mode, src/agents/ppo.py:
77-88: ``policies = {agent_i: PolicySpec()}``, ``policy_mapping_fn = agent_id``): row ``b * N + a`` is agent a's.  A
``DevicePolicy`` takes it as it takes the shared module and runs the same launch with one weight set per agent
(``mapf_policy_create_per_agent``).

``PopulationPolicy`` is P ``MaskedRecurrentPolicy`` trained side by side on one env handle (the reference's tuner,
src/trainers/tuner.py, runs such a population as separate trials): env b is member ``b % P``'s.  A ``DevicePolicy`` runs it as
the same launch with one weight set per member and a group-to-set map (``mapf_policy_create_mapped``).

``JointActionPolicy`` / ``JointDevicePolicy`` are the same pair for the single-agent env (the reference's CTE mode,
src/agents/ppo.py:25-64 behind models/action_mask_model_single.py): one row per env, the full grid as features, N five-way
heads, one launch per step (``mapf_jpolicy_act``).
"""

from __future__ import annotations

import ctypes as C

import torch

from . import _lib as L
from .device_net import Checkpoint, DeviceNet, ptr

HIDDEN = L.POLICY_HIDDEN
NUM_ACTIONS = 5
MASK_EPS = 1e-6


class _OneNet(Checkpoint, torch.nn.Module):
    """One net of the rule of include/mapf_step.h, the base of ``MaskedRecurrentPolicy`` and ``JointActionPolicy``: 64-64 dense
    on the first ``features`` floats of a row, an LSTMCell on [a2, onehot5 of each of the ``heads`` previous actions,
    prev_reward] when ``recurrent``, ``heads`` five-way heads (plus log(mask + 1e-6) when ``has_mask``) and the value.  A
    subclass sets those four and ``hidden``, then calls ``_layers``.

    Also what the learner's rows view asks of a module (learner.fragment_view): ``heads``, ``groups`` independent nets
    (``nets()``), whether a row is an env (``rows_are_envs``), whether results keep an agent axis (``agent_axis``), and a
    layer on [T, R, in] rows (``dense``)."""

    heads, groups, rows_are_envs, agent_axis = 1, 1, False, False
    REWARD_DTYPE = None  # what prev_reward is rounded to before the cast to the observation's dtype (None: not rounded)

    def _layers(self) -> None:
        self.fc1 = torch.nn.Linear(self.features, self.hidden)
        self.fc2 = torch.nn.Linear(self.hidden, self.hidden)
        if self.recurrent:
            self.lstm = torch.nn.LSTMCell(self.hidden + NUM_ACTIONS * self.heads + 1, self.hidden)
        self.pi = torch.nn.Linear(self.hidden, NUM_ACTIONS * self.heads)
        self.vf = torch.nn.Linear(self.hidden, 1)

    def initial_state(self, rows: int, device=None):
        z = torch.zeros((int(rows), self.hidden), dtype=torch.float32, device=device)
        return z, z.clone()

    def forward(self, obs, prev_action=None, prev_reward=None, start=None, state=None):
        """obs float32 [R, L]; prev_action integer [R] ([R, N] with N heads) and prev_reward [R] (None: zeros); start bool /
        uint8 [R] (None: no row starts an episode): rows where it is set use h = c = 0, prev_action = 0, prev_reward = 0;
        state (h, c) float32 [R, 64] each (None: zeros).  Returns logits [R, 5 heads], value [R], (h', c').  prev_action must
        lie in 0 .. 4: the kernel drops any other byte (it contributes no one-hot entry, as the rule says), this module
        raises."""
        R = obs.shape[0]
        a2 = torch.tanh(self.fc2(torch.tanh(self.fc1(obs[:, :self.features]))))
        if self.recurrent:
            h, c = state if state is not None else self.initial_state(R, obs.device)
            pa = (torch.zeros((R, self.heads), dtype=torch.int64, device=obs.device) if prev_action is None
                  else prev_action.to(torch.int64).reshape(R, self.heads))
            pr = torch.zeros(R, dtype=obs.dtype, device=obs.device) if prev_reward is None else prev_reward.to(self.REWARD_DTYPE or obs.dtype).to(obs.dtype)
            if start is not None:
                keep = start == 0
                h, c = h * keep[:, None].to(h.dtype), c * keep[:, None].to(c.dtype)
                pa, pr = pa * keep[:, None].to(pa.dtype), pr * keep.to(pr.dtype)
            z = torch.cat([a2, torch.nn.functional.one_hot(pa, NUM_ACTIONS).to(a2.dtype).flatten(1), pr[:, None]], dim=1)
            h, c = self.lstm(z, (h, c))
            u, state = h, (h, c)
        else:
            u = a2
        logits = self.pi(u)
        if self.has_mask:
            logits = logits + torch.log(obs[:, self.features:] + MASK_EPS)
        return logits, self.vf(u)[:, 0], state

    def nets(self) -> list:
        return [self]

    def dense(self, x, name: str):
        """Layer ``name`` (fc1, fc2, pi, vf) on x, or, for ``lstm``, the input half of the gates, W_ih x + b_ih + b_hh."""
        if name == "lstm":
            return torch.nn.functional.linear(x, self.lstm.weight_ih, self.lstm.bias_ih + self.lstm.bias_hh)
        return getattr(self, name)(x)

    def weight_hh(self):
        return self.lstm.weight_hh


class MaskedRecurrentPolicy(_OneNet):
    """obs [R, L] -> logits [R, 5], value [R], state.  ``has_mask``: the observation ends in the 5-float action mask, which
    is no feature and is added to the logits as log(mask + 1e-6).  ``recurrent``: LSTMCell(64 + 5 + 1 -> 64) on
    [a2, onehot5(prev_action), prev_reward]; otherwise the heads read a2 and the state is passed through."""

    KIND = "masked_recurrent"  # what a checkpoint of this class says it is (device_net.Checkpoint)

    def __init__(self, obs_len: int, has_mask: bool = False, recurrent: bool = True, hidden: int = HIDDEN):
        super().__init__()
        self.obs_len, self.has_mask, self.recurrent, self.hidden = int(obs_len), bool(has_mask), bool(recurrent), int(hidden)
        self.features = self.obs_len - NUM_ACTIONS if self.has_mask else self.obs_len
        if self.features < 1:
            raise ValueError(f"obs_len {obs_len} leaves no feature")
        self._layers()

    @property
    def mask_off(self) -> int:
        return self.features if self.has_mask else -1

    def config(self) -> dict:
        return {"obs_len": self.obs_len, "has_mask": self.has_mask, "recurrent": self.recurrent, "hidden": self.hidden}


class PerAgentPolicy(Checkpoint, torch.nn.Module):
    """One ``MaskedRecurrentPolicy`` per agent: ``agents[a]`` acts on the rows ``a::N`` of the usual ``b * N + a`` row order.
    ``agents`` is a ``ModuleList``, so the ``state_dict`` is policy-major and ``flat_params()`` is the concatenation of the
    agents' vectors -- what a per-agent handle takes; every ``agents[a]`` is itself a shared policy that can be saved,
    loaded and run on its own."""

    KIND = "per_agent"
    heads, rows_are_envs, agent_axis = 1, False, True  # (the protocol of _OneNet, for N nets)

    def __init__(self, num_agents: int, obs_len: int, has_mask: bool = False, recurrent: bool = True, hidden: int = HIDDEN):
        super().__init__()
        self.num_agents = int(num_agents)
        if not 1 <= self.num_agents <= L.MAX_AGENTS:
            raise ValueError(f"num_agents {num_agents} must lie in 1 .. {L.MAX_AGENTS}")
        self.agents = torch.nn.ModuleList(MaskedRecurrentPolicy(obs_len, has_mask, recurrent, hidden) for _ in range(self.num_agents))
        first = self.agents[0]
        self.obs_len, self.has_mask, self.recurrent, self.hidden = first.obs_len, first.has_mask, first.recurrent, first.hidden
        self.features, self.mask_off, self.groups = first.features, first.mask_off, self.num_agents

    @classmethod
    def from_shared(cls, module: MaskedRecurrentPolicy, num_agents: int):
        """N copies of one shared policy (on its device, in its dtype)."""
        out = cls(num_agents, module.obs_len, module.has_mask, module.recurrent, module.hidden)
        ref = next(module.parameters())
        out.to(device=ref.device, dtype=ref.dtype)
        for agent in out.agents:
            agent.load_state_dict(module.state_dict())
        return out

    def config(self) -> dict:
        return {"num_agents": self.num_agents, "obs_len": self.obs_len, "has_mask": self.has_mask, "recurrent": self.recurrent,
                "hidden": self.hidden}

    def initial_state(self, rows: int, device=None):
        return self.agents[0].initial_state(rows, device)

    def stacked(self, name: str) -> torch.Tensor:
        """Parameter ``name`` (``fc1.weight``, ``lstm.bias_ih``, ...) of every agent as one [N, ...] tensor; differentiable,
        the gradient of slice a arrives at agent a's parameter."""
        return torch.stack([agent.get_parameter(name) for agent in self.agents])

    def nets(self) -> list:
        return list(self.agents)

    def dense(self, x, name: str):
        """``_OneNet.dense`` on [T, R, in] rows in ``b * N + a`` order, every row through its own agent's layer: one batched
        product over the agent axis.  The two LSTM biases are added per agent BEFORE they are stacked: the sum hands one
        gradient to two parameters, so each receives its own copy (stacked apart, both ``.grad`` would be the same slice of
        the stack's gradient, and an in-place clip of one would clip the other again)."""
        if name == "lstm":
            w, b = self.stacked("lstm.weight_ih"), torch.stack([a.lstm.bias_ih + a.lstm.bias_hh for a in self.agents])
        else:
            w, b = self.stacked(name + ".weight"), self.stacked(name + ".bias")
        return (torch.einsum("tbni,noi->tbno", x.unflatten(1, (-1, self.num_agents)), w) + b).flatten(1, 2)

    def weight_hh(self):
        return self.stacked("lstm.weight_hh")

    def forward(self, obs, prev_action=None, prev_reward=None, start=None, state=None):
        """As ``MaskedRecurrentPolicy.forward`` on rows in ``b * N + a`` order (R a multiple of N): row r goes through
        ``agents[r % N]``."""
        N, R = self.num_agents, obs.shape[0]
        if R % N:
            raise ValueError(f"{R} rows are no whole number of envs of {N} agents")
        outs = [self.agents[a](obs[a::N], None if prev_action is None else prev_action[a::N],
                               None if prev_reward is None else prev_reward[a::N], None if start is None else start[a::N],
                               None if state is None else (state[0][a::N], state[1][a::N])) for a in range(N)]

        def weave(xs):  # [N] x [B, ...] -> [B * N, ...]
            return torch.stack(xs, dim=1).reshape(R, *xs[0].shape[1:])

        new_state = state
        if self.recurrent:
            new_state = (weave([o[2][0] for o in outs]), weave([o[2][1] for o in outs]))
        return weave([o[0] for o in outs]), weave([o[1] for o in outs]), new_state


class PopulationPolicy(Checkpoint, torch.nn.Module):
    """P ``MaskedRecurrentPolicy`` trained side by side on one env handle (the reference's tuner runs such a population as
    separate trials, src/trainers/tuner.py): env b belongs to member ``b % P``, so with N agents per env row ``r = b N + a``
    is group ``r % (P N)`` of ``groups = P N`` and its weights are those of member ``(r % (P N)) // N``.  ``members`` is a
    ``ModuleList``, so the ``state_dict`` and ``flat_params()`` are member-major -- what a mapped handle takes
    (``mapf_policy_create_mapped``); every ``members[p]`` is itself a shared policy that can be saved, loaded and evaluated
    on its own.  It follows the protocol ``PerAgentPolicy`` gives the learner, with ``policies = P`` independent nets of
    ``num_agents`` groups each."""

    KIND = "population"
    heads, rows_are_envs, agent_axis = 1, False, True  # (the protocol of _OneNet, for P nets on P N groups)

    def __init__(self, members: int, num_agents: int, obs_len: int, has_mask: bool = False, recurrent: bool = True,
                 hidden: int = HIDDEN):
        super().__init__()
        self.num_members, self.num_agents = int(members), int(num_agents)
        if self.num_members < 1 or not 1 <= self.num_agents <= L.MAX_AGENTS:
            raise ValueError(f"members {members} must be >= 1 and num_agents {num_agents} in 1 .. {L.MAX_AGENTS}")
        self.groups = self.num_members * self.num_agents
        if self.groups > L.POLICY_MAX_GROUPS:
            raise ValueError(f"{members} members of {num_agents} agents are {self.groups} groups, more than the {L.POLICY_MAX_GROUPS} "
                             f"a mapped policy handle takes")
        self.members = torch.nn.ModuleList(MaskedRecurrentPolicy(obs_len, has_mask, recurrent, hidden) for _ in range(self.num_members))
        first = self.members[0]
        self.obs_len, self.has_mask, self.recurrent, self.hidden = first.obs_len, first.has_mask, first.recurrent, first.hidden
        self.features, self.mask_off = first.features, first.mask_off

    @property
    def policies(self) -> int:
        return self.num_members

    @classmethod
    def from_shared(cls, module: MaskedRecurrentPolicy, members: int, num_agents: int):
        """P copies of one shared policy (on its device, in its dtype)."""
        out = cls(members, num_agents, module.obs_len, module.has_mask, module.recurrent, module.hidden)
        ref = next(module.parameters())
        out.to(device=ref.device, dtype=ref.dtype)
        for member in out.members:
            member.load_state_dict(module.state_dict())
        return out

    def config(self) -> dict:
        return {"members": self.num_members, "num_agents": self.num_agents, "obs_len": self.obs_len, "has_mask": self.has_mask,
                "recurrent": self.recurrent, "hidden": self.hidden}

    def set_of_group(self) -> list:
        """The map a mapped handle takes: group g = p N + a reads set p."""
        return [g // self.num_agents for g in range(self.groups)]

    def initial_state(self, rows: int, device=None):
        return self.members[0].initial_state(rows, device)

    def stacked(self, name: str) -> torch.Tensor:
        """Parameter ``name`` of every member as one [P, ...] tensor; differentiable, slice p's gradient arrives at member p."""
        return torch.stack([m.get_parameter(name) for m in self.members])

    def nets(self) -> list:
        return list(self.members)

    def dense(self, x, name: str):
        """``_OneNet.dense`` on [T, R, in] rows in ``b * N + a`` order, every row through its own member's layer: one
        batched product over the member axis, rows unflattened to [.., P, N, in] against weights [P, out, in].  The two LSTM
        biases are added per member before they are stacked, as ``PerAgentPolicy.dense`` explains."""
        if name == "lstm":
            w, b = self.stacked("lstm.weight_ih"), torch.stack([m.lstm.bias_ih + m.lstm.bias_hh for m in self.members])
        else:
            w, b = self.stacked(name + ".weight"), self.stacked(name + ".bias")
        y = torch.einsum("tupni,poi->tupno", x.unflatten(1, (-1, self.num_members, self.num_agents)), w) + b[:, None]
        return y.flatten(1, 3)

    def weight_hh(self):
        """[P N, 256, 64]: each member's matrix once per agent group, as the grouped LSTM kernels take their groups (a copy
        of P N x 64 KB per call; the gradient of the N copies is summed back into the member's matrix)."""
        return self.stacked("lstm.weight_hh").repeat_interleave(self.num_agents, dim=0)

    def forward(self, obs, prev_action=None, prev_reward=None, start=None, state=None):
        """As ``MaskedRecurrentPolicy.forward`` on rows in ``b * N + a`` order (R a multiple of P N): the rows of env b go
        through ``members[b % P]``."""
        P, N, R = self.num_members, self.num_agents, obs.shape[0]
        if R % (P * N):
            raise ValueError(f"{R} rows are no whole number of {P} envs of {N} agents")

        def of(x, p):  # the rows of member p, in its own b' * N + a order
            return None if x is None else x.unflatten(0, (-1, P, N))[:, p].flatten(0, 1)

        outs = [self.members[p](of(obs, p), of(prev_action, p), of(prev_reward, p), of(start, p),
                                None if state is None else (of(state[0], p), of(state[1], p))) for p in range(P)]

        def weave(xs):  # [P] x [U * N, ...] -> [U * P * N, ...]
            return torch.stack([x.unflatten(0, (-1, N)) for x in xs], dim=1).reshape(R, *xs[0].shape[1:])

        new_state = state
        if self.recurrent:
            new_state = (weave([o[2][0] for o in outs]), weave([o[2][1] for o in outs]))
        return weave([o[0] for o in outs]), weave([o[1] for o in outs]), new_state


def load_policy(path, map_location="cpu"):
    """The module of a checkpoint written by ``MaskedRecurrentPolicy.save``, ``PerAgentPolicy.save`` or
    ``PopulationPolicy.save``, by its kind (any other kind: the ValueError of ``MaskedRecurrentPolicy.load``, which names the
    class that reads it)."""
    blob = torch.load(path, map_location=map_location, weights_only=True)
    kind = blob.get("kind", Checkpoint.DEFAULT_KIND) if isinstance(blob, dict) else None
    classes = {PerAgentPolicy.KIND: PerAgentPolicy, PopulationPolicy.KIND: PopulationPolicy}
    return classes.get(kind, MaskedRecurrentPolicy).load(path, map_location)


class JointActionPolicy(_OneNet):
    """The joint-action policy of the single-agent env (include/mapf_step.h, "Joint-action policy"): obs [R, F + 5N] ->
    logits [R, 5N], value [R], state.  One row is one env: the first F = grid_cells floats are the features, the last 5N
    the action mask of the N agents, added to the logits as log(mask + 1e-6).  ``recurrent``: LSTMCell(64 + 5N + 1 -> 64)
    on [a2, onehot5(prev_action[:, 0]), ..., onehot5(prev_action[:, N-1]), prev_reward]; prev_action integer [R, N],
    prev_reward float32 or float64 [R], rounded to nearest fp32 as the kernel's load does.  ``hidden=256`` with
    ``recurrent=False`` is the reference's CTE IMPALA net (fcnet_hiddens = [256, 256], the value head on the shared trunk);
    ``JointDevicePolicy`` runs these two widths."""

    KIND = "joint_action"
    rows_are_envs, has_mask, REWARD_DTYPE = True, True, torch.float32

    def __init__(self, grid_cells: int, num_agents: int, recurrent: bool = True, hidden: int = HIDDEN):
        super().__init__()
        self.grid_cells, self.num_agents, self.recurrent, self.hidden = int(grid_cells), int(num_agents), bool(recurrent), int(hidden)
        if self.grid_cells < 1 or self.num_agents < 1:
            raise ValueError(f"grid_cells {grid_cells} and num_agents {num_agents} must be >= 1")
        self.features, self.heads = self.grid_cells, self.num_agents
        self.num_logits = NUM_ACTIONS * self.num_agents
        self.obs_len = self.features + self.num_logits
        self._layers()

    def config(self) -> dict:
        return {"grid_cells": self.grid_cells, "num_agents": self.num_agents, "recurrent": self.recurrent, "hidden": self.hidden}


class _DeviceActor(DeviceNet):
    """What ``DevicePolicy`` and ``JointDevicePolicy`` share: the recurrent state, the sampler's draw counters and the output
    tensors of ``rows`` rows with ``heads`` five-way heads each, and ``<prefix>_act`` on them."""

    def _allocate(self, heads=None) -> None:
        """heads None: one head, and ``action`` is [rows] instead of [rows, heads]."""
        dev, R = self.device, self.rows
        self.h = torch.zeros((R, HIDDEN), dtype=torch.float32, device=dev)
        self.c = torch.zeros((R, HIDDEN), dtype=torch.float32, device=dev)
        self.draws = torch.zeros((R,), dtype=torch.int32, device=dev)
        self.action = torch.zeros((R,) if heads is None else (R, heads), dtype=torch.int8, device=dev)
        self.logp = torch.zeros((R,), dtype=torch.float32, device=dev)
        self.value = torch.zeros((R,), dtype=torch.float32, device=dev)
        self.logits = torch.zeros((R, NUM_ACTIONS * (heads or 1)), dtype=torch.float32, device=dev)

    def reset_state(self) -> None:
        self.h.zero_()
        self.c.zero_()
        self.draws.zero_()

    def act_raw(self, obs_ptr, prev_action_ptr, prev_reward_ptr, start_a_ptr, start_b_ptr, mode: int, seed: int,
                out=None, stream=None) -> None:
        """``mapf_policy_act`` / ``mapf_jpolicy_act`` on raw device pointers (ints or None) with the policy's own state
        (prev_reward points to float32, for the joint policy to float64); out: (action, logp, value, logits) pointers,
        default the policy's own tensors."""
        if out is None:
            out = (self.action.data_ptr(), self.logp.data_ptr(), self.value.data_ptr(), self.logits.data_ptr())
        self._act((obs_ptr, prev_action_ptr, prev_reward_ptr, start_a_ptr, start_b_ptr, self.h.data_ptr(), self.c.data_ptr(),
                   self.draws.data_ptr()), seed, mode, out, stream)

    def _step(self, obs, pa, pr, start, start_rows: int, sample: bool, peek: bool, seed: int) -> dict:
        """The tail of ``act``: the pair of start flags ([start_rows] each), the mode bits, the launch and what it returns."""
        if isinstance(start, torch.Tensor) or start is None:
            start = (start, None)
        sa, sb = (self._input(s, torch.uint8, start_rows, "start") for s in start)
        mode = (L.POLICY_SAMPLE if sample else 0) | (L.POLICY_PEEK if peek else 0)
        self.act_raw(ptr(obs), ptr(pa), ptr(pr), ptr(sa), ptr(sb), mode, seed)
        return {"action": self.action, "logp": self.logp, "value": self.value, "logits": self.logits}


class DevicePolicy(_DeviceActor):
    """``MaskedRecurrentPolicy`` as one launch per step (``mapf_policy_act``) on ``rows = B * agents_per_env`` agent rows;
    with a ``PerAgentPolicy`` (or a checkpoint of that kind) the same launch with one weight set per agent: ``per_agent``
    says which, and ``agents_per_env`` must then be the module's ``num_agents``.  With a ``PopulationPolicy`` (or a checkpoint
    of that kind) it is the launch of ``mapf_policy_create_mapped`` with one weight set per member: ``population`` says so,
    ``agents_per_env`` must be the module's ``num_agents`` and ``rows`` a multiple of its ``groups`` = P N.

    ``act`` returns the policy's own output tensors (overwritten by the next call): ``action`` int8 [rows], ``logp``,
    ``value`` float32 [rows], ``logits`` float32 [rows, 5]; ``h`` / ``c`` float32 [rows, 64] and ``draws`` (uint32 counters
    in int32 storage) are its state.  Nothing is synchronised and nothing is allocated per call, so a loop of ``act`` and
    env steps can be captured into a graph from the first call."""

    def __init__(self, module_or_path, rows: int, agents_per_env: int, device="cuda:0"):
        module = module_or_path if isinstance(module_or_path, torch.nn.Module) else load_policy(module_or_path)
        super().__init__("mapf_policy", device)
        self.rows, self.agents_per_env = int(rows), int(agents_per_env)
        if self.rows < 1 or self.agents_per_env < 1 or self.rows % self.agents_per_env:
            raise ValueError(f"rows = {rows} must be a positive multiple of agents_per_env = {agents_per_env}")
        self.per_agent = isinstance(module, PerAgentPolicy)
        if self.per_agent and module.num_agents != self.agents_per_env:
            raise ValueError(f"the checkpoint holds one policy for each of {module.num_agents} agents, the rows have "
                             f"{self.agents_per_env} agents per env")
        self.population = isinstance(module, PopulationPolicy)
        create, extra = "mapf_policy_create_per_agent" if self.per_agent else None, ()
        if self.population:
            if module.num_agents != self.agents_per_env or self.rows % module.groups:
                raise ValueError(f"a population of {module.num_members} members of {module.num_agents} agents needs rows = {rows} to "
                                 f"be a multiple of {module.groups} and {self.agents_per_env} agents per env to be {module.num_agents}")
            create = "mapf_policy_create_mapped"
            extra = (module.groups, module.num_members, (C.c_int32 * module.groups)(*module.set_of_group()))
        self.obs_len, self.mask_off, self.recurrent = module.obs_len, module.mask_off, module.recurrent
        self._create(L.MapfPolicyConfig(self.obs_len, self.mask_off, int(self.recurrent), self.agents_per_env, module.hidden,
                                        int(self.device.index)), module, create, extra)
        self._allocate()
        self.load_params(module)

    def act(self, obs, prev_action=None, prev_reward=None, start=(None, None), sample: bool = False, peek: bool = False,
            seed: int = 0) -> dict:
        """One policy step of every row.  obs float32 [rows, L] (or [B, N, L]); prev_action int8, prev_reward float32
        [rows] or None (zeros); start: a pair of uint8 [B] tensors (either may be None) -- a row whose env has a non-zero
        byte in either starts an episode; sample: Gumbel-max sampling instead of argmax; peek: leave h, c and draws as they
        are."""
        R, B = self.rows, self.rows // self.agents_per_env
        obs = self._input(obs, torch.float32, R * self.obs_len, "obs")
        pa = self._input(prev_action, torch.int8, R, "prev_action")
        pr = self._input(prev_reward, torch.float32, R, "prev_reward")
        return self._step(obs, pa, pr, start, B, sample, peek, seed)


class JointDevicePolicy(_DeviceActor):
    """``JointActionPolicy`` as one launch per step (``mapf_jpolicy_act``) on ``rows = B`` env rows.

    ``act`` returns the policy's own output tensors (overwritten by the next call): ``action`` int8 [rows, N], ``logp``,
    ``value`` float32 [rows], ``logits`` float32 [rows, 5N]; ``h`` / ``c`` float32 [rows, 64] and ``draws`` (uint32 counters
    in int32 storage) are its state.  Nothing is synchronised and nothing is allocated per call, so a loop of ``act`` and
    env steps can be captured into a graph from the first call.  There is no fallback: without the built library it raises.

    The module's ``hidden`` is 64, or 256 for the feed-forward 256-256 net of the reference's CTE IMPALA configuration
    (src/agents/impala.py:16-51), which runs on a kernel of its own behind the same calls; a feed-forward policy leaves
    ``h`` and ``c`` at zero."""

    def __init__(self, module_or_path, rows: int, device="cuda:0"):
        if isinstance(module_or_path, PopulationPolicy):
            raise ValueError("a PopulationPolicy is not supported on the single-agent env: populations are PPO on the multi-agent "
                             "env with shared-policy members (DevicePolicy runs a PopulationPolicy)")
        if isinstance(module_or_path, PerAgentPolicy):
            raise ValueError("DTE (one policy per agent) is not supported on the single-agent env: a JointActionPolicy moves all "
                             "agents of an env (DevicePolicy runs a PerAgentPolicy on the multi-agent env)")
        module = self._module(JointActionPolicy, module_or_path,
                              "JointDevicePolicy needs a JointActionPolicy (DevicePolicy runs a MaskedRecurrentPolicy)")
        if module.hidden == L.JPOLICY_HIDDEN_WIDE and module.recurrent:
            raise ValueError(f"the wide joint net (hidden = {L.JPOLICY_HIDDEN_WIDE}) runs on the device feed-forward only: a recurrent "
                             f"JointActionPolicy must have hidden = {HIDDEN} (mapf_jpolicy_create refuses any other combination)")
        super().__init__("mapf_jpolicy", device)
        self.rows = int(rows)
        if self.rows < 1:
            raise ValueError(f"rows = {rows} must be positive")
        self.grid_cells, self.num_agents, self.recurrent = module.grid_cells, module.num_agents, module.recurrent
        self.obs_len = module.obs_len
        self._create(L.MapfJPolicyConfig(self.grid_cells, self.num_agents, int(self.recurrent), module.hidden, int(self.device.index)),
                     module)
        self._allocate(self.num_agents)
        self.load_params(module)

    def act(self, obs, prev_action=None, prev_reward=None, start=(None, None), sample: bool = False, peek: bool = False,
            seed: int = 0) -> dict:
        """One policy step of every env row.  obs float32 [rows, L]; prev_action int8 [rows, N], prev_reward float64 [rows]
        or None (zeros); start: a pair of uint8 [rows] tensors (either may be None) -- a row with a non-zero byte in either
        starts an episode; sample: Gumbel-max sampling instead of argmax; peek: leave h, c and draws as they are."""
        R = self.rows
        obs = self._input(obs, torch.float32, R * self.obs_len, "obs")
        pa = self._input(prev_action, torch.int8, R * self.num_agents, "prev_action")
        pr = self._input(prev_reward, torch.float64, R, "prev_reward")
        return self._step(obs, pa, pr, start, R, sample, peek, seed)
