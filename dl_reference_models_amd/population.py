"""Population-based training: P policies in one rollout and one learner.

    env = VecReferenceModel({..., "num_envs": 4096})
    module = PopulationPolicy(8, env.num_agents, env.obs_len, has_mask=..., recurrent=True).to(env.device)
    trainer = PopulationTrainer(env, module, T=32, hyper=Hyper(), pbt=PBT(perturb_every=10, seed=0))
    for it in range(400):
        print(trainer.iterate())
    trainer.best().save("policy.pt")     # scripts/evaluate_multi_agent_env.py --policy NEURAL --checkpoint policy.pt

The reference's training entry point hands its config to a tuner (src/trainers/tuner.py) that runs a population of trials
under a PB2 / ``PopulationBasedTraining`` scheduler, one process, one env and one learner per trial, and restores exploited
trials "weights only" (src/trainers/resettable_rllib_trainable.py:73-101).  Here the population shares ONE env handle, ONE
``DevicePolicy`` (``mapf_policy_create_mapped``: env b is member b % P's), ONE ``Rollout`` with its one captured graph and
ONE ``PPOLearner`` (P independent learners in one, per-member hyperparameters in device memory: ``mapf_ppo_loss_hp``).

``Hyper`` is one member's settings.  The searched ones and their default ranges are tuner.py:19-26's: ``lr`` [1e-5, 1e-3]
(log-uniform), ``ent_coeff`` (entropy_coeff) [0, 0.015], ``clip`` (clip_param) [0.05, 0.5], ``gamma`` [0.8, 0.999], ``lam``
(lambda) [0.8, 0.99].  ``num_epochs`` is NOT searched and is one value for the whole population (the learner's ``epochs``):
the members share one minibatch loop, and a member cannot skip an Adam step inside it without its moments still moving.

``PBT`` is Ray's ``PopulationBasedTraining`` rule with Ray's defaults (quantile 0.25, resample probability 0.25, factors 1.2
and 0.8), drawn from a seeded host generator, every ``perturb_every`` ITERATIONS (the reference's 600 s are wall clock;
iterations make a run repeatable).  PB2's Gaussian-process bandit is out of scope.

The score is the reference's PB2 metric, ``env_runners/episode_return_mean``: the mean return (the reward summed over the
agents and steps of an episode) of the member's episodes that ended since the last perturbation (``EpisodeScore``).
"""

from __future__ import annotations

import copy
import dataclasses
import math

import torch

from .learner import PPOLearner, Rollout, _layout, gae
from .policy import DevicePolicy, MaskedRecurrentPolicy, PopulationPolicy
from .vec_env import VecReferenceModel


@dataclasses.dataclass
class Hyper:
    """One member's hyperparameters; the defaults are ``PPOLearner``'s and ``Trainer``'s (the reference's multi-agent PPO)."""
    lr: float = 1e-3
    ent_coeff: float = 0.001
    clip: float = 0.05
    gamma: float = 0.99
    lam: float = 0.95
    vf_coeff: float = 0.5   # (not searched)
    vf_clip: float = 10.0   # (not searched)

    def check(self) -> "Hyper":
        for name, x in dataclasses.asdict(self).items():
            if not math.isfinite(float(x)) or float(x) < 0:
                raise ValueError(f"{name} must be finite and >= 0, got {x}")
        if not self.lr > 0 or not self.clip < 1 or self.gamma > 1 or self.lam > 1:
            raise ValueError(f"lr must be > 0, clip < 1, gamma and lam <= 1, got {self}")
        return self


# the searched hyperparameters and their bounds (tuner.py:19-26); lr is drawn log-uniformly, the others uniformly
DEFAULT_RANGES = {"lr": (1e-5, 1e-3), "ent_coeff": (0.0, 0.015), "clip": (0.05, 0.5), "gamma": (0.8, 0.999), "lam": (0.8, 0.99)}
LOG_UNIFORM = ("lr",)


class PBT:
    """Ray's truncation-and-perturb rule.  ``perturb(scores, hypers)`` ranks the members that have a score (None: no episode
    of the member ended in the window; it neither gives nor receives), lets each of the lower ``quantile`` (ceil(n / 4), at
    least 1 of n >= 2) clone a uniformly drawn member of the upper one, and explores from the donor's hyperparameters: each
    searched one is resampled from its range with probability ``resample_probability`` (``lr`` log-uniform, the others
    uniform), otherwise multiplied by 1.2 or 0.8 with equal chance, then clipped to the range.  All draws come from one
    seeded host generator whose state ``state()`` / ``load_state()`` carry, so a run is repeatable and continues after a
    reload with the same decisions."""

    def __init__(self, perturb_every: int = 10, seed: int = 0, ranges: dict | None = None, quantile: float = 0.25,
                 resample_probability: float = 0.25, factors=(1.2, 0.8)):
        if int(perturb_every) < 1 or not 0 < float(quantile) <= 0.5 or not 0 <= float(resample_probability) <= 1:
            raise ValueError("perturb_every must be >= 1, quantile in (0, 0.5] and resample_probability in [0, 1]")
        self.perturb_every, self.quantile, self.resample_probability = int(perturb_every), float(quantile), float(resample_probability)
        self.factors = tuple(float(f) for f in factors)
        self.ranges = dict(DEFAULT_RANGES if ranges is None else ranges)
        fields = {f.name for f in dataclasses.fields(Hyper)}
        for name, (lo, hi) in self.ranges.items():
            if name not in fields or not lo <= hi or (name in LOG_UNIFORM and not lo > 0):
                raise ValueError(f"range {name}: ({lo}, {hi}) names no hyperparameter or is empty")
        self._gen = torch.Generator()
        self._gen.manual_seed(int(seed))

    def _uniform(self) -> float:
        return float(torch.rand((), generator=self._gen, dtype=torch.float64))

    def _below(self, n: int) -> int:
        return int(torch.randint(int(n), (), generator=self._gen))

    def explore(self, hyper: Hyper) -> Hyper:
        new = dataclasses.asdict(hyper)
        for name, (lo, hi) in self.ranges.items():
            if self._uniform() < self.resample_probability:
                u = self._uniform()
                x = math.exp(math.log(lo) + u * (math.log(hi) - math.log(lo))) if name in LOG_UNIFORM else lo + u * (hi - lo)
            else:
                x = new[name] * self.factors[self._below(len(self.factors))]
            new[name] = min(max(x, lo), hi)
        return Hyper(**new).check()

    def perturb(self, scores, hypers) -> list:
        """scores: one float or None per member; hypers: their ``Hyper``.  Returns [(receiver, donor, the receiver's new
        Hyper)]; nothing is applied here."""
        ranked = sorted((p for p, s in enumerate(scores) if s is not None), key=lambda p: (scores[p], p))
        if len(ranked) < 2:
            return []
        n = min(max(1, math.ceil(len(ranked) * self.quantile)), len(ranked) // 2)
        lower, upper = ranked[:n], ranked[-n:]
        return [(p, donor, self.explore(hypers[donor])) for p in lower for donor in [upper[self._below(len(upper))]]]

    def state(self) -> torch.Tensor:
        return self._gen.get_state()

    def load_state(self, state) -> None:
        self._gen.set_state(state.to(torch.uint8).cpu())


def exploit(module: PopulationPolicy, learner: PPOLearner, receiver: int, donor: int) -> None:
    """The reference's "weights only" restore into a rebuilt trial, on the module's device: the receiver's parameters become
    the donor's, its Adam moments and step count are reset and its ``kl_coeff`` returns to the initial value."""
    with torch.no_grad():
        for dst, src in zip(module.members[receiver].parameters(), module.members[donor].parameters()):
            dst.copy_(src)
    learner.reset_member(receiver)


def apply_hyper(learner: PPOLearner, member: int, hyper: Hyper) -> None:
    """The learner's share of a member's ``Hyper`` (gamma and lam are ``gae``'s)."""
    hyper.check()
    learner.set_hyper(member, lr=hyper.lr, clip=hyper.clip, vf_clip=hyper.vf_clip, vf_coeff=hyper.vf_coeff, ent_coeff=hyper.ent_coeff)


class EpisodeScore:
    """The return of the episodes that ended, per env, accumulated on the device in torch ops over a fragment's [T, B]: no
    loop over steps and no synchronisation.  An episode's return is the reward summed over its agents and steps; episodes
    span fragments (``carry`` holds the running sum of the episode in progress).  ``skip``: the envs whose episode in
    progress is not to be counted (a member that just took over another's weights mid-episode)."""

    def __init__(self, num_envs: int, members: int, device):
        self.members = int(members)
        self.carry = torch.zeros(int(num_envs), dtype=torch.float64, device=device)
        self.total = torch.zeros_like(self.carry)
        self.count = torch.zeros(int(num_envs), dtype=torch.int64, device=device)
        self.skip = torch.zeros(int(num_envs), dtype=torch.bool, device=device)
        self.open = torch.zeros_like(self.skip)  # an episode is in progress: the last step seen did not end one

    def update(self, rewards, ended) -> None:
        """rewards [T, B, N] (or [T, B]); ended [T, B], non-zero where an episode ended at step t."""
        r = rewards.to(torch.float64)
        r = r.sum(dim=2) if r.dim() == 3 else r
        T = r.shape[0]
        e = ended != 0
        steps = torch.arange(T, device=r.device)[:, None]
        ends, any_end = e.sum(dim=0), e.any(dim=0)
        first = torch.where(e, steps, T).min(dim=0).values  # the first and the last step at which an episode ended
        last = torch.where(e, steps, -1).max(dim=0).values
        upto_first, upto_last = (r * (steps <= first)).sum(dim=0), (r * (steps <= last)).sum(dim=0)
        # the returns of the episodes that ended here add up to the running sum at the last end: every episode begins where
        # the one before it ended.  Where the episode in progress is not to be counted, the sum starts at the first end.
        dropped = self.skip & any_end
        self.total += torch.where(any_end, torch.where(dropped, upto_last - upto_first, self.carry + upto_last), 0.0)
        self.count += ends - dropped.to(ends.dtype)
        self.skip &= ~any_end
        self.open.copy_(last != T - 1)
        self.carry.copy_(torch.where(any_end, 0.0, self.carry) + (r.sum(dim=0) - upto_last))

    def per_member(self):
        """(sum of returns, episodes) per member, [P] each: env b is member b % P's."""
        return self.total.view(-1, self.members).sum(dim=0), self.count.view(-1, self.members).sum(dim=0)

    def new_window(self, receivers=()) -> None:
        """After a perturbation: every member's window starts again; the receivers' episodes in progress are not theirs (an
        env that has just ended an episode has none in progress and loses nothing)."""
        self.total.zero_()
        self.count.zero_()
        for p in receivers:
            self.skip[p::self.members] = self.open[p::self.members]

    def state(self) -> dict:
        return {"carry": self.carry, "total": self.total, "count": self.count, "skip": self.skip, "open": self.open}

    def load_state(self, state: dict) -> None:
        for k, v in self.state().items():
            v.copy_(state[k])


class PopulationTrainer:
    """collect -> per-member gae -> update -> load_params for a ``PopulationPolicy``: the one ``DevicePolicy``, the one
    ``Rollout`` and the one ``PPOLearner`` of P members on ``env`` (a ``VecReferenceModel`` whose ``num_envs`` is a multiple
    of P; env b is member b % P's).  hyper: one ``Hyper`` for every member or a list of P; pbt: a ``PBT`` (None: the members
    train side by side and nothing is ever perturbed).  The remaining arguments are ``PPOLearner``'s: ``epochs`` and
    ``minibatches`` are one value for the whole population."""

    def __init__(self, env, module: PopulationPolicy, T: int = 32, hyper=None, pbt: PBT | None = None, epochs: int = 12,
                 minibatches: int = 8, grad_clip=None, kl_coeff: float | None = None, kl_target: float = 0.01, seed: int = 0,
                 sample_seed: int = 0, fused: bool = True, fused_grads: bool = False):
        if not isinstance(module, PopulationPolicy):
            raise TypeError("PopulationTrainer needs a PopulationPolicy")
        if not isinstance(env, VecReferenceModel):
            raise TypeError("a PopulationPolicy is not supported on the single-agent env: PopulationTrainer needs a VecReferenceModel")
        P = module.num_members
        if env.num_envs % P:
            raise ValueError(f"num_envs = {env.num_envs} is no multiple of the population's {P} members")
        dev = next(module.parameters()).device
        if dev != env.device:
            raise ValueError(f"the module is on {dev}, the env on {env.device}")
        hypers = [hyper if hyper is not None else Hyper()] * P if not isinstance(hyper, (list, tuple)) else list(hyper)
        if len(hypers) != P:
            raise ValueError(f"{len(hypers)} Hyper for {P} members")
        self.env, self.module, self.pbt, self.T = env, module, pbt, int(T)
        self.hypers = [dataclasses.replace(h).check() for h in hypers]
        first = self.hypers[0]
        self.learner = PPOLearner(module, lr=first.lr, clip=first.clip, vf_coeff=first.vf_coeff, ent_coeff=first.ent_coeff,
                                  vf_clip=first.vf_clip, epochs=epochs, minibatches=minibatches, grad_clip=grad_clip, seed=seed,
                                  fused=fused, kl_coeff=kl_coeff, kl_target=kl_target, fused_grads=fused_grads)
        layout = _layout(False, module, env.num_envs, env.num_agents)
        self.policy = DevicePolicy(module, layout["R"], env.num_agents, env.device)
        self.rollout = Rollout(env, self.policy, self.T, sample=True, seed=sample_seed, keep_logits=kl_coeff is not None)
        self._adv = torch.empty((self.T, *layout["per_row"]), dtype=torch.float32, device=env.device)
        self._targets = torch.empty_like(self._adv)
        self._gamma = torch.empty((env.num_envs, 1), dtype=torch.float64, device=env.device)
        self._lam = torch.empty_like(self._gamma)
        self.score = EpisodeScore(env.num_envs, P, env.device)
        self.scores = [None] * P  # the members' scores at the last iteration (None: no episode ended in the window)
        self.iterations = 0
        self.perturbations = []  # [(iteration, receiver, donor)]
        for p in range(P):
            self._set_hyper(p, self.hypers[p])

    def _set_hyper(self, member: int, hyper: Hyper) -> None:
        self.hypers[member] = hyper
        apply_hyper(self.learner, member, hyper)
        self._gamma[member::self.module.num_members] = hyper.gamma
        self._lam[member::self.module.num_members] = hyper.lam

    def _exploit(self, receiver: int, donor: int, hyper: Hyper) -> None:
        """Everything on the device: weights, optimizer state, KL coefficient, hyperparameters, and the recurrent state of
        the receiver's rows (the env keeps running)."""
        exploit(self.module, self.learner, receiver, donor)
        self._set_hyper(receiver, hyper)
        P, N = self.module.num_members, self.module.num_agents
        for state in (self.policy.h, self.policy.c):
            state.view(-1, P, N, state.shape[-1])[:, receiver].zero_()

    def iterate(self) -> dict:
        """One training iteration; synchronises once, to hand back Python numbers: what ``Trainer.iterate()`` returns (the
        loss terms are means over the members) plus ``per_member`` (the loss terms, the current hyperparameters and the
        score of every member), ``best_score`` / ``mean_score`` (over the members that have one; None where none has) and
        ``perturbed``, the [(receiver, donor)] of this iteration.  The perturbation follows that one synchronisation."""
        P = self.module.num_members
        frag = self.rollout.collect()
        adv, targets = gae(frag, self._gamma, self._lam, out=(self._adv, self._targets))
        terms = self.learner.update(frag, adv, targets)
        ended = (frag["terminated"] != 0) | (frag["truncated"] != 0)
        self.score.update(frag["rewards"], ended)
        per_policy = terms.pop("per_policy")
        term, trunc = frag["terminated"] != 0, frag["truncated"] != 0
        names = ["reward_per_step", "episodes", "terminated", "truncated"] + list(terms)
        vals = [frag["rewards"].mean(), (term | trunc).sum(), (term & ~trunc).sum(), trunc.sum()] + list(terms.values())
        total, count = self.score.per_member()
        host = torch.cat([torch.stack([v.to(torch.float64) for v in vals]), total, count.to(torch.float64),
                          torch.stack([v.to(torch.float64) for v in per_policy.values()]).flatten()]).cpu()  # the one synchronisation
        self.iterations += 1
        out = {k: float(v) for k, v in zip(names, host[:len(names)].tolist())}
        for k in ("episodes", "terminated", "truncated"):
            out[k] = int(out[k])
        out["iteration"] = self.iterations
        o = len(names)
        totals, counts = host[o:o + P].tolist(), host[o + P:o + 2 * P].tolist()
        self.scores = [t / c if c > 0 else None for t, c in zip(totals, counts)]
        per = host[o + 2 * P:].view(len(per_policy), P)
        have = [s for s in self.scores if s is not None]
        out["best_score"], out["mean_score"] = (max(have), sum(have) / len(have)) if have else (None, None)
        out["perturbed"] = []
        if self.pbt is not None and self.iterations % self.pbt.perturb_every == 0:
            decisions = self.pbt.perturb(self.scores, self.hypers)
            for receiver, donor, hyper in decisions:
                self._exploit(receiver, donor, hyper)
                self.perturbations.append((self.iterations, receiver, donor))
            self.score.new_window([r for r, _d, _h in decisions])
            out["perturbed"] = [(r, d) for r, d, _h in decisions]
        self.policy.load_params(self.module)
        out["per_member"] = {**{k: per[i].tolist() for i, k in enumerate(per_policy)},
                             "hyper": [dataclasses.asdict(h) for h in self.hypers], "score": list(self.scores)}
        return out

    def best_member(self) -> int:
        """The member with the highest score at the last iteration (member 0 before any episode ended)."""
        have = [(s, -p) for p, s in enumerate(self.scores) if s is not None]
        return -max(have)[1] if have else 0

    def best(self) -> MaskedRecurrentPolicy:
        """A copy of the best member, an ordinary ``MaskedRecurrentPolicy``."""
        return copy.deepcopy(self.module.members[self.best_member()])

    def save(self, path) -> None:
        """The whole population: module, optimizer, hyperparameters, KL coefficients, score window, the generators' states
        and the iteration count."""
        torch.save({"kind": "population_trainer", "config": self.module.config(), "state_dict": self.module.state_dict(),
                    "optimizer": self.learner.optimizer.state_dict(), "hyper": [dataclasses.asdict(h) for h in self.hypers],
                    "kl_coeff": self.learner.kl_coeff, "pbt": None if self.pbt is None else self.pbt.state(),
                    "minibatch_generator": self.learner._gen.get_state(), "score": self.score.state(), "scores": self.scores,
                    "iterations": self.iterations, "perturbations": self.perturbations}, path)

    def load(self, path) -> None:
        blob = torch.load(path, map_location=self.env.device, weights_only=True)
        if not isinstance(blob, dict) or blob.get("kind") != "population_trainer":
            raise ValueError(f"{path} is no PopulationTrainer.save file (PopulationPolicy.load reads a population's checkpoint)")
        if blob["config"] != self.module.config():
            raise ValueError(f"{path} holds a population of {blob['config']}, this trainer one of {self.module.config()}")
        self.module.load_state_dict(blob["state_dict"])
        self.learner.optimizer.load_state_dict(blob["optimizer"])
        if self.learner.kl_coeff is not None and blob["kl_coeff"] is not None:
            self.learner.kl_coeff.copy_(blob["kl_coeff"])
        for p, h in enumerate(blob["hyper"]):
            self._set_hyper(p, Hyper(**h).check())
        if self.pbt is not None and blob["pbt"] is not None:
            self.pbt.load_state(blob["pbt"])
        self.learner._gen.set_state(blob["minibatch_generator"].cpu())
        self.score.load_state(blob["score"])
        self.scores, self.iterations = list(blob["scores"]), int(blob["iterations"])
        self.perturbations = [tuple(x) for x in blob["perturbations"]]
        self.policy.load_params(self.module)
