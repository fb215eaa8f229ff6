"""The rollout loop on the fused policy: T x (``mapf_policy_act`` -> ``mapf_step`` with auto-reset) plus one PEEK act for
the bootstrap value, two launches per step, everything written where a learner reads it.

    env = VecReferenceModel({..., "num_envs": 4096})
    pol = DevicePolicy(module, env.num_envs * env.num_agents, env.num_agents, env.device)
    ro = Rollout(env, pol, T=32)
    frag = ro.collect()          # the first call launches, every later call replays one captured graph

The slabs are allocated once, [T + 1] deep: the act of step t reads slab t (observation, reward and episode-end flags of
the step before; the previous action is row t - 1 of the action slab) and writes row t of ``actions`` / ``logp`` /
``value``; the env step writes slab t + 1 through the C ABI's output pointers, so there is no copy between the two
launches.  A fragment starts with the carry of the previous one (slab T -> slab 0, the last action and h, c -> h0, c0:
six small copies per fragment) and ends with the PEEK act and one OR launch for ``first``.  GAE and the learner are in
learner.py; they read the dict ``collect()`` returns.

Expert labels (opt-in, ``expert="yielding" | "independent" | "windowed"``): between the act of step t and the env step the
planner is evaluated on the state the step starts from and its actions go into row t of a slab ``expert_actions`` int8
[T, B, N] -- one more launch per step (``mapf_expert_actions`` writes the row itself; ``"windowed"`` is
``mapf_plan_windowed(expert_window)`` into the rollout's own buffers and a copy of the plan's first step).  ``beta`` is the
DAgger mixing share: a uint8 slab ``followed`` [T, B] is redrawn before every ``collect()`` from a seeded host generator
(``followed_draw``), outside the captured graph, and the envs with ``followed[t]`` set execute the expert's action at step t
in place of the policy's -- ``actions[t]`` holds what was executed, and so does the next act's previous action.  ``logp`` of
a followed step is still the log-probability of the action the policy drew, not of the executed one: fragments collected
with beta > 0 are for ``BCLearner``, not for PPO or V-trace.  Without ``expert`` there is no such slab, key or launch.

Shortest-path guidance (opt-in, ``Rollout(..., guidance=True)``): the policy sees ``env.guided_obs`` rows, the observation
with the six floats of ``mapf_observe_guided`` in it (include/mapf_step.h: which moves shorten the agent's path, whether it
stands on its goal, the path length).  The observation slab is then [T + 1, B, N, L + 6]; the env step writes its observation
into one staging buffer [B, N, L] and one ``mapf_observe_guided`` launch per step -- and one after the constructor's reset --
moves it into slab t + 1 with the guidance of the state the step left, inside the captured fragment.  It combines with
``keep_logits``, ``expert`` and ``beta`` as they are; without it there is no staging buffer, no launch and no new key.

``JointRollout`` is the same loop for the single-agent env: T x (``mapf_jpolicy_act`` -> ``mapf_cte_step`` with auto-reset)
plus the PEEK act, on ``VecSingleAgentReferenceModel`` and ``JointDevicePolicy``.  One row is one env, an action is the N
bytes of its agents, and the reward slab is the float64 one the step writes (the act reads it as it is).
"""

from __future__ import annotations

import torch

from . import _lib as L
from .device_net import GraphedFragment
from .policy import DevicePolicy, JointDevicePolicy
from .vec_env import VecReferenceModel
from .vec_env_single_agent import VecSingleAgentReferenceModel


EXPERTS = ("yielding", "independent", "windowed")
MULTI_AGENT_ONLY_EXPERTS = ("windowed",)  # as evaluation.MULTI_AGENT_ONLY_POLICIES: the planner's guarantee is the multi-agent move rule's
_EXPERT_MODE = {"independent": 0, "yielding": 1}  # mapf_expert_actions' mode


def check_expert(expert, joint: bool, expert_window: int = 8, beta: float = 0.0) -> None:
    """ValueError, by name, for what a rollout does not take as its expert options; needs no env."""
    if expert is None:
        if float(beta) != 0.0:
            raise ValueError(f"beta = {beta} needs an expert: one of {list(EXPERTS)}")
        return
    if expert not in EXPERTS:
        raise ValueError(f"unknown expert {expert!r} (None, or one of {list(EXPERTS)})")
    if joint and expert in MULTI_AGENT_ONLY_EXPERTS:
        raise ValueError(f"expert {expert!r} is not offered on the single-agent env (JointRollout): the planner's guarantee that "
                         "its plan executes without a failed move is stated for the multi-agent move rule only (there: one of "
                         f"{sorted(set(EXPERTS) - set(MULTI_AGENT_ONLY_EXPERTS))})")
    if expert == "windowed" and not 1 <= int(expert_window) <= L.PLAN_MAX_WINDOW:
        raise ValueError(f"expert_window must lie in [1, {L.PLAN_MAX_WINDOW}], got {expert_window}")
    if not 0.0 <= float(beta) <= 1.0:
        raise ValueError(f"beta must lie in [0, 1], got {beta}")


def check_guidance_fits(env_obs_len: int) -> None:
    """ValueError, naming both numbers, for an env whose guided observation is longer than the policy kernel's longest row
    (the widest observation, 130 floats, leaves no room for the six): no ``DevicePolicy`` can be made for it."""
    if env_obs_len + L.GUIDANCE_LEN > L.POLICY_MAX_OBS_LEN:
        raise ValueError(f"guidance=True gives this env guided observations of env.obs_len + {L.GUIDANCE_LEN} = "
                         f"{env_obs_len + L.GUIDANCE_LEN} floats, more than the {L.POLICY_MAX_OBS_LEN} the policy kernel takes "
                         "(mapf_policy_create): use a smaller sensor range or fewer observation extras, or leave the guidance out")


def check_guided_obs_len(policy_obs_len: int, env_obs_len: int, guidance: bool) -> None:
    """ValueError, naming both numbers, for a policy whose ``obs_len`` is the plain observation's where the guided one's is
    asked for, or the reverse; and for guidance on an env whose guided observation no policy can take
    (``check_guidance_fits``)."""
    if guidance:
        check_guidance_fits(env_obs_len)
    if guidance and policy_obs_len != env_obs_len + L.GUIDANCE_LEN:
        raise ValueError(f"guidance=True needs a policy with obs_len = env.obs_len + {L.GUIDANCE_LEN} = {env_obs_len + L.GUIDANCE_LEN}, "
                         f"got obs_len = {policy_obs_len}")
    if not guidance and policy_obs_len == env_obs_len + L.GUIDANCE_LEN:
        raise ValueError(f"the policy's obs_len = {policy_obs_len} is env.obs_len + {L.GUIDANCE_LEN} (env.obs_len = {env_obs_len}): "
                         "it was built for guided observations, pass guidance=True")


def followed_draw(generator: torch.Generator, T: int, B: int, beta: float) -> torch.Tensor:
    """The ``followed`` slab of one fragment, uint8 [T, B] on the host: ``rand(T, B) < beta`` from ``generator`` (a host
    generator, so the draw is the same on every machine; beta = 0 sets nothing, beta = 1 everything)."""
    return (torch.rand((int(T), int(B)), generator=generator) < float(beta)).to(torch.uint8)


class _PolicyRollout(GraphedFragment):
    """What ``Rollout`` and ``JointRollout`` share: the slabs, the carry, the T + 1 acts and T steps of a fragment and
    ``first = terminated | truncated``.  ``row``: the shape of a step's rows ((B, N) agent rows or (B,) env rows);
    ``reward_dtype``: what the env's step writes; ``_step(t, stream)``: the one env step from slab t into slab t + 1.
    ``guidance``: the module docstring's guided observations (``Rollout`` only).
    ``keep_logits``: the T acts also write the behaviour policy's (masked) logits, into a slab [T, *row, 5 heads] that the
    fragment hands out as ``logits`` -- what a KL term against the behaviour policy needs; without it there is no such slab
    and no such key, and the launches are the ones they were.
    ``expert`` / ``expert_window`` / ``beta``: the module docstring's expert labels and DAgger mixing; ``beta`` may be set
    between two ``collect()`` calls (a schedule needs no recapture; the first non-zero beta of a rollout built with beta = 0
    adds the replace op to the fragment and captures it again)."""

    def __init__(self, env, policy, T: int, sample: bool, seed: int, row: tuple, reward_dtype, keep_logits: bool = False,
                 expert=None, expert_window: int = 8, beta: float = 0.0, guidance: bool = False):
        B, N = env.num_envs, env.num_agents
        self.guidance = bool(guidance)
        Lo = env.guided_obs_len if self.guidance else env.obs_len
        self.env, self.policy, self.T, self.sample, self.seed = env, policy, int(T), bool(sample), int(seed)
        if self.T < 1:
            raise ValueError(f"T must be >= 1, got {T}")
        T, dev = self.T, env.device
        f32, u8 = torch.float32, torch.uint8
        self._obs = torch.zeros((T + 1, *row, Lo), dtype=f32, device=dev)
        self._rew = torch.zeros((T + 1, *row), dtype=reward_dtype, device=dev)
        self._term = torch.zeros((T + 1, B), dtype=u8, device=dev)
        self._trunc = torch.zeros((T + 1, B), dtype=u8, device=dev)
        self._act = torch.zeros((T, B, N), dtype=torch.int8, device=dev)
        self._logp = torch.zeros((T, *row), dtype=f32, device=dev)
        self._val = torch.zeros((T, *row), dtype=f32, device=dev)
        self._first = torch.zeros((T, B), dtype=u8, device=dev)
        self._pa0 = torch.zeros((B, N), dtype=torch.int8, device=dev)  # the action before the fragment's first step
        self._peek_act = torch.zeros((B, N), dtype=torch.int8, device=dev)
        self._h0 = torch.zeros_like(policy.h)
        self._c0 = torch.zeros_like(policy.c)
        self._last_value = torch.zeros(row, dtype=f32, device=dev)
        self.keep_logits = bool(keep_logits)
        self._logits = torch.zeros((T, *row, policy.logits.shape[-1]), dtype=f32, device=dev) if self.keep_logits else None
        # the first fragment starts every env's episode: what the carry finds in slab T is the reset observation and a set flag
        if self.guidance:
            self._stage = torch.zeros((*row, env.obs_len), dtype=f32, device=dev)  # what the env step writes
            env.reset()
            env.guided_obs(out=self._obs[T])
        else:
            self._obs[T].copy_(env.reset())
        self._term[T].fill_(1)
        policy.reset_state()
        self._graph = None
        self._calls = 0
        self._out = {"obs": self._obs[:T], "actions": self._act, "logp": self._logp, "value": self._val, "rewards": self._rew[1:],
                     "terminated": self._term[1:], "truncated": self._trunc[1:], "first": self._first, "h0": self._h0,
                     "c0": self._c0, "last_value": self._last_value, "prev_action0": self._pa0, "prev_rewards": self._rew[:T]}
        if self.keep_logits:
            self._out["logits"] = self._logits
        self.expert, self.expert_window = expert, int(expert_window)
        self._beta, self._mix = float(beta), float(beta) != 0.0
        if expert is not None:
            self._expert = torch.zeros((T, B, N), dtype=torch.int8, device=dev)
            self._followed = torch.zeros((T, B), dtype=u8, device=dev)
            self._followed_gen = torch.Generator()
            self._followed_gen.manual_seed(self.seed ^ 0x5DA66E12)
            if expert == "windowed":
                if self.expert_window > env.max_window:
                    raise ValueError(f"expert_window must lie in [1, {env.max_window}], got {expert_window}")
                W = self.expert_window
                self._plan = (torch.zeros((B, W, N), dtype=torch.int8, device=dev), torch.zeros((B, N), dtype=torch.int32, device=dev),
                              torch.zeros((B, N), dtype=torch.int32, device=dev))
            self._out["expert_actions"], self._out["followed"] = self._expert, self._followed

    @property
    def beta(self) -> float:
        return self._beta

    @beta.setter
    def beta(self, value: float) -> None:
        check_expert(self.expert, False, self.expert_window, value)
        self._beta = float(value)
        if self._beta != 0.0 and not self._mix:  # the fragment gets its replace op: whatever was captured lacks it
            self._mix, self._graph = True, None

    def collect(self) -> dict:
        if self.expert is not None and self._mix:  # outside the graph: a replay reads the slab it finds
            self._followed.copy_(followed_draw(self._followed_gen, self.T, self.env.num_envs, self._beta))
        return super().collect()

    def _label(self, t, stream) -> None:
        """The expert's actions on the state step t starts from into row t of the label slab, and the executed action of the
        envs that follow the expert."""
        env = self.env
        if self.expert == "windowed":
            plan, arrival, remaining = self._plan
            rc = env._lib.mapf_plan_windowed(env._h, self.expert_window, None, plan.data_ptr(), arrival.data_ptr(),
                                             remaining.data_ptr(), stream)
            if rc != 0:
                env._check(rc)
            self._expert[t].copy_(plan[:, 0, :])
        else:
            rc = env._lib.mapf_expert_actions(env._h, _EXPERT_MODE[self.expert], self._expert[t].data_ptr(), None, stream)
            if rc != 0:
                env._check(rc)
        if self._mix:
            torch.where(self._followed[t][:, None] != 0, self._expert[t], self._act[t], out=self._act[t])

    def _launch(self) -> None:
        pol, T = self.policy, self.T
        mode = 1 if self.sample else 0
        for dst, src in ((self._obs[0], self._obs[T]), (self._rew[0], self._rew[T]), (self._term[0], self._term[T]),
                         (self._trunc[0], self._trunc[T]), (self._h0, pol.h), (self._c0, pol.c)):
            dst.copy_(src)
        if self._calls:
            self._pa0.copy_(self._act[T - 1])
        stream = pol._stream()
        for t in range(T + 1):
            pa = self._pa0 if t == 0 else self._act[t - 1]
            last = t == T
            out = ((self._peek_act.data_ptr(), None, self._last_value.data_ptr(), None) if last else
                   (self._act[t].data_ptr(), self._logp[t].data_ptr(), self._val[t].data_ptr(),
                    self._logits[t].data_ptr() if self.keep_logits else None))
            pol.act_raw(self._obs[t].data_ptr(), pa.data_ptr(), self._rew[t].data_ptr(), self._term[t].data_ptr(),
                        self._trunc[t].data_ptr(), mode | (2 if last else 0), self.seed, out=out, stream=stream)
            if last:
                break
            if self.expert is not None:
                self._label(t, stream)
            rc = self._step(t, stream)
            if rc != 0:
                self.env._check(rc)
        torch.bitwise_or(self._term[:T], self._trunc[:T], out=self._first)


class Rollout(_PolicyRollout):
    def __init__(self, env: VecReferenceModel, policy: DevicePolicy, T: int, sample: bool = True, seed: int = 0,
                 keep_logits: bool = False, expert=None, expert_window: int = 8, beta: float = 0.0, guidance: bool = False):
        check_expert(expert, False, expert_window, beta)
        if not isinstance(env, VecReferenceModel):
            raise TypeError("Rollout needs a VecReferenceModel")
        B, N, Lo = env.num_envs, env.num_agents, env.obs_len
        if guidance:  # (no device policy exists for such an env, so none is looked at)
            check_guidance_fits(Lo)
        check_guided_obs_len(policy.obs_len, Lo, guidance)
        if policy.rows != B * N or policy.agents_per_env != N or policy.obs_len != Lo + (L.GUIDANCE_LEN if guidance else 0) \
                or policy.device != env.device:
            raise ValueError("the policy's rows, agents_per_env, obs_len and device must be the env's")
        super().__init__(env, policy, T, sample, seed, (B, N), torch.float32, keep_logits, expert, expert_window, beta, guidance)

    def _step(self, t, stream) -> int:
        env = self.env
        obs = self._stage if self.guidance else self._obs[t + 1]
        rc = env._lib.mapf_step(env._h, self._act[t].data_ptr(), obs.data_ptr(), self._rew[t + 1].data_ptr(),
                                self._term[t + 1].data_ptr(), self._trunc[t + 1].data_ptr(), env._info_all.data_ptr(),
                                env._info_agent.data_ptr(), None, 1, stream)
        if rc == 0 and self.guidance:  # the guidance of the state the step left, around the observation it wrote
            rc = env._lib.mapf_observe_guided(env._h, obs.data_ptr(), env.guidance_tail, self._obs[t + 1].data_ptr(), stream)
        return rc

    def collect(self) -> dict:
        """One fragment of T steps.  Returns views of the preallocated slabs (overwritten by the next call): ``obs``
        [T, B, N, L] (what the policy saw), ``actions`` int8, ``logp``, ``value``, ``rewards`` [T, B, N], ``terminated``,
        ``truncated``, ``first`` uint8 [T, B] (``first[t]``: ``obs[t]`` starts an episode, i.e. step t - 1 ended one -- the
        rows where the policy cleared its state), ``h0`` / ``c0`` [B * N, 64] (the LSTM state before step 0, before that
        clearing), ``last_value`` [B, N] (the value of the observation after step T - 1, state untouched), ``prev_action0``
        int8 [B, N] (the action before step 0; the one before step t > 0 is ``actions[t - 1]``) and ``prev_rewards`` [T, B, N]
        (the reward the act of step t read: ``rewards`` shifted by one step) -- with them a learner can rebuild the LSTM's
        input at every step.  With ``keep_logits`` also ``logits`` [T, B, N, 5], the masked logits the actions were drawn from.  With ``expert`` also
        ``expert_actions`` int8 [T, B, N] (the planner's action on the state step t starts from) and ``followed`` uint8 [T, B]
        (1: the env executed the expert's action at step t, and ``actions[t]`` holds it; ``logp[t]`` is then NOT the executed
        action's -- such fragments are for ``BCLearner``).  With ``guidance`` the rows of ``obs`` are [L + 6] long: what the policy
        saw.  The env's own observation tensor is not updated.  The first call launches; the second captures the fragment into a graph and every
        call from then on replays it."""
        return super().collect()


class JointRollout(_PolicyRollout):
    def __init__(self, env: VecSingleAgentReferenceModel, policy: JointDevicePolicy, T: int, sample: bool = True, seed: int = 0,
                 keep_logits: bool = False, expert=None, expert_window: int = 8, beta: float = 0.0, guidance: bool = False):
        if guidance:
            raise ValueError("guidance is not offered on the single-agent env (JointRollout): its full-grid observation holds "
                             "the grid already; use Rollout on a VecReferenceModel")
        check_expert(expert, True, expert_window, beta)
        if not isinstance(env, VecSingleAgentReferenceModel):
            raise TypeError("JointRollout needs a VecSingleAgentReferenceModel")
        if not isinstance(policy, JointDevicePolicy):
            raise TypeError("JointRollout needs a JointDevicePolicy")
        B, N, Lo = env.num_envs, env.num_agents, env.obs_len
        if policy.rows != B or policy.num_agents != N or policy.obs_len != Lo or policy.device != env.device:
            raise ValueError("the policy's rows, num_agents, obs_len and device must be the env's")
        super().__init__(env, policy, T, sample, seed, (B,), torch.float64, keep_logits, expert, expert_window,
                         beta)  # float64: what mapf_cte_step writes

    def _step(self, t, stream) -> int:
        env = self.env
        return env._lib.mapf_cte_step(env._h, self._act[t].data_ptr(), self._obs[t + 1].data_ptr(), self._rew[t + 1].data_ptr(),
                                      self._term[t + 1].data_ptr(), self._trunc[t + 1].data_ptr(), env._info.data_ptr(), None, 1,
                                      stream)

    def collect(self) -> dict:
        """One fragment of T steps.  Returns views of the preallocated slabs (overwritten by the next call), under the keys
        of ``Rollout.collect``: ``obs`` [T, B, L], ``actions`` int8 [T, B, N], ``logp``, ``value`` [T, B] (the summed
        log-probability of the N actions), ``rewards`` and ``prev_rewards`` float64 [T, B], ``terminated``, ``truncated``,
        ``first`` uint8 [T, B], ``h0`` / ``c0`` [B, 64], ``last_value`` [B], ``prev_action0`` int8 [B, N]; with ``keep_logits``
        also ``logits`` [T, B, 5N]; with ``expert`` (``"yielding"`` or ``"independent"``) also ``expert_actions`` int8 [T, B, N]
        and ``followed`` uint8 [T, B], as in ``Rollout.collect``.  The env's own
        observation tensor is not updated.  The first call launches; the second captures the fragment into a graph and
        every call from then on replays it."""
        return super().collect()
