"""Single-agent (CTE) env: episode statistics booked by the step kernels, and the masked step (mapf_cte_step_masked).

Expected sums come from the oracle's outputs at every episode end, under the definitions of the reference's callbacks
(src/trainers/callbacks.py:138-181, :236-345): goals reached = agents with goal_reached_once (info[:, 2]), blocking count =
_episode_blocking_count (info[:, 3]), episode length = step_count at the finishing step."""

import numpy as np
import pytest

from trace_util import CteEngineStepper, CteOracleStepper, _eq, synth_grids

pytestmark = pytest.mark.gpu

ACC = dict(EPISODES=0, SUCCESSES=1, GOALS_REACHED=2, BLOCKING_COUNT=3, COMPLETED_AGENTS=8, EPISODE_STEPS=9)


class SumsFromOracle:
    """The accumulator vector the engine should hold, built from the oracle's per-step outputs."""

    def __init__(self, counts):
        self.want = np.zeros(12, dtype=np.int64)
        self.steps = np.asarray(counts, dtype=np.int64).copy()  # step_count of every env

    def book(self, out, rows=None, reset_done=True):
        """out: the oracle's outputs of one step for the envs `rows` (all when None)."""
        rows = np.arange(len(self.steps)) if rows is None else np.asarray(rows)
        self.steps[rows] += 1
        term, trunc = out["terminated"][rows].astype(bool), out["truncated"][rows].astype(bool)
        done = term | trunc
        w, info = self.want, out["info"][rows]
        w[ACC["EPISODES"]] += int(done.sum())
        w[ACC["SUCCESSES"]] += int((term & ~trunc).sum())
        w[ACC["GOALS_REACHED"]] += int(info[done, 2].sum())
        w[ACC["BLOCKING_COUNT"]] += int(info[done, 3].sum())
        w[ACC["COMPLETED_AGENTS"]] += int(info[done, 2].sum())
        w[ACC["EPISODE_STEPS"]] += int(self.steps[rows][done].sum())
        if reset_done:
            self.steps[rows[done]] = 0
        return rows[done]


def _actions(orc, rng, greedy_share=0.6):
    pos, gl = orc.positions().astype(int), orc.goals().astype(int)
    d = gl - pos
    greedy = np.where(np.abs(d[..., 0]) >= np.abs(d[..., 1]), np.where(d[..., 0] > 0, 3, np.where(d[..., 0] < 0, 1, 0)),
                      np.where(d[..., 1] > 0, 2, 4))
    B, N = greedy.shape
    return np.where(rng.random((B, N)) < greedy_share, greedy, rng.integers(0, 5, size=(B, N))).astype(np.int8)


def _staggered(a, b, spe, rng):
    counts = rng.integers(0, spe, size=a.B)
    a.env.set_step_counts(counts)
    for e, c in zip(b.envs, counts):
        e._step[0] = int(c)
    return counts


# ---- 1. sums against the oracle, single-step launches -----------------------------------------------------------------
@pytest.mark.parametrize("shape", [(512, 16, 16, 4, {}), (300, 32, 32, 8, {"blocking_penalty": -0.3}),
                                   (40, 64, 64, 64, {"steps_per_episode": 50}), (70, 5, 9, 7, {"steps_per_episode": 30})])
def test_cte_episode_sums_match_the_oracle(shape):
    import torch

    B, H, W, N, extra = shape
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": 60}
    cfg.update(extra)
    spe = cfg["steps_per_episode"]
    grids = synth_grids(B, H, W, 0.2, N, base_seed=140_000)
    seeds = list(range(B))
    a, b = CteEngineStepper(grids, cfg, seeds=seeds), CteOracleStepper(grids, cfg, seeds=seeds)
    _eq("reset obs", a.reset(), b.reset())
    rng = np.random.default_rng(4)
    sums = SumsFromOracle(_staggered(a, b, spe, rng))
    truncs = 0
    for t in range(150):
        acts = _actions(b, rng)
        ra, rb = a.step(acts), b.step(acts)
        for k in ("obs", "reward", "terminated", "truncated", "info"):
            _eq(k, ra[k], rb[k], t)
        sums.book(rb)
        truncs += int(rb["truncated"].sum())
        if t % 10 == 9:
            _eq("episode sums", a.env.episode_sums(), sums.want, t)
    want = sums.want
    assert truncs > 0 and want[ACC["EPISODES"]] > truncs - 1
    if N <= 7:  # (32x32 x 8 and 64x64 x 64 agents never all stand on their goals in 150 steps of this policy)
        assert want[ACC["SUCCESSES"]] > 0
    assert want[4:8].sum() == 0
    # the device-side sums: directly, and captured in a graph behind the steps
    dev = torch.full((12,), -1, dtype=torch.int64, device=a.env.device)
    assert a.env.episode_sums_device(dev) is dev
    _eq("device sums", dev.cpu().numpy(), a.env.episode_sums())
    K = 12
    acts = rng.integers(0, 5, size=(K, B, N)).astype(np.int8)
    dacts = torch.from_numpy(acts).to(a.env.device)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for t in range(K):
            a.env.step(dacts[t], auto_reset=True)
        a.env.episode_sums_device(dev)
    for rep in range(2):
        g.replay()
        for t in range(K):
            sums.book(b.step(acts[t]))
        torch.cuda.synchronize()
        a.env.poll_error()
        _eq("device sums after replay", dev.cpu().numpy(), sums.want, rep)
    _eq("host sums after replay", a.env.episode_sums(), sums.want)
    _eq("positions", a.positions(), b.positions())
    _eq("rng", a.rng_words(), b.rng_words())
    m = a.env.episode_metrics()
    n = sums.want[0]
    assert m["episodes"] == n and m["success_rate"] == sums.want[1] / n and m["goals_reached"] == sums.want[2] / n
    assert m["blocking_count"] == sums.want[3] / n and m["episode_len_mean"] == sums.want[9] / n
    assert m["deadlock_count"] == m["livelock_steps"] == 0.0
    _eq("sums (reset)", a.env.episode_sums(reset=True), sums.want)
    assert a.env.episode_sums().sum() == 0


# ---- 2. sums through fused launches -----------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2048, 32, 32, 8, 31), (8192, 16, 16, 4, 23), (130, 16, 16, 4, 9)])
def test_cte_episode_sums_through_fused_launches(shape):
    import torch

    B, H, W, N, spe = shape
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": spe}
    grids = synth_grids(B, H, W, 0.2, N, base_seed=150_000)
    seeds = list(range(B))
    a, b = CteEngineStepper(grids, cfg, seeds=seeds), CteOracleStepper(grids, cfg, seeds=seeds)
    _eq("reset obs", a.reset(), b.reset())
    if B >= 2048:  # single-step and fused launches of this handle run on different group widths
        assert a.env.launch_info()["lanes_per_env"] != a.env.launch_info(fused=True)["lanes_per_env"]
    rng = np.random.default_rng(9)
    sums = SumsFromOracle(_staggered(a, b, spe, rng))
    for rep, T in enumerate((13, 1, 1, 29, 1, 7, 40)):
        acts = rng.integers(0, 5, size=(T, B, N)).astype(np.int8)
        out = a.env.step_many(torch.from_numpy(acts).to(a.env.device), obs_mode=0)
        for t in range(T):
            rb = b.step(acts[t])
            sums.book(rb)
        _eq("fused terminated", out["terminated"][-1].cpu().numpy(), rb["terminated"], rep)
        _eq("episode sums", a.env.episode_sums(), sums.want, rep)
    assert sums.want[ACC["EPISODES"]] > B
    a.env.poll_error()


# ---- 3. a step that latches an invalid action books nothing -----------------------------------------------------------
def test_cte_bad_action_books_no_episode():
    import torch

    B, N, spe = 8, 4, 20
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": spe}
    a = CteEngineStepper(synth_grids(B, 16, 16, 0.2, N, base_seed=160_000), cfg, seeds=list(range(B)))
    a.reset()
    a.env.set_step_counts([spe - 1] * B)  # the next step ends every episode (step limit)
    acts = np.zeros((B, N), dtype=np.int8)
    acts[3, 1] = 9
    out = a.env.step(torch.from_numpy(acts).to(a.env.device), auto_reset=True)
    torch.cuda.synchronize()
    with pytest.raises(ValueError, match="Invalid action"):
        a.env.poll_error()
    s = a.env.episode_sums()
    assert s[ACC["EPISODES"]] == B - 1 and s[ACC["EPISODE_STEPS"]] == (B - 1) * spe
    assert s[ACC["SUCCESSES"]] == 0
    trunc = out["truncated"].cpu().numpy()
    assert trunc[3] == 0 and trunc[np.arange(B) != 3].all()


# ---- 4. the masked step -----------------------------------------------------------------------------------------------
SENTINEL = -7.0


def _fill_sentinel(env):
    env._obs.fill_(SENTINEL)
    env._reward.fill_(SENTINEL)
    env._info.fill_(SENTINEL)
    env._terminated.fill_(0xAB)
    env._truncated.fill_(0xCD)


def _outputs(env):
    return {"obs": env._obs.cpu().numpy(), "reward": env._reward.cpu().numpy(), "info": env._info.cpu().numpy(),
            "terminated": env._terminated.cpu().numpy(), "truncated": env._truncated.cpu().numpy()}


def _oracle_rows(orc, acts, rows, auto_reset):
    """The oracle stepping only the envs `rows` (the others are not touched)."""
    B, L = orc.B, orc.L
    out = {"obs": np.zeros((B, L), np.float32), "reward": np.zeros(B, np.float64), "terminated": np.zeros(B, np.uint8),
           "truncated": np.zeros(B, np.uint8), "info": np.zeros((B, 4), np.float32)}
    for r in rows:
        e = orc.envs[r]
        rc, obs, rew, term, trunc, info = e.step(acts[r])
        assert rc == 0
        out["obs"][r], out["reward"][r], out["terminated"][r], out["truncated"][r], out["info"][r] = obs, rew, term, trunc, info
        if auto_reset and (term or trunc):
            out["obs"][r] = e.reset()
    return out


STATE_KEYS = ("positions", "goals", "starts", "reached", "counters", "rng_words")


@pytest.mark.parametrize("shape", [(320, 16, 16, 4, 23), (301, 9, 7, 5, 11)])
def test_cte_masked_step_against_the_oracle(shape):
    import torch

    B, H, W, N, spe = shape
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": spe}
    grids = synth_grids(B, H, W, 0.2, N, base_seed=170_000)
    seeds = list(range(B))
    a, b = CteEngineStepper(grids, cfg, seeds=seeds), CteOracleStepper(grids, cfg, seeds=seeds)
    env = a.env
    _eq("reset obs", a.reset(), b.reset())
    rng = np.random.default_rng(31)
    sums = SumsFromOracle(_staggered(a, b, spe, rng))
    masked_launches = 0
    for it in range(90):
        acts = _actions(b, rng)
        dacts = torch.from_numpy(acts).to(env.device)
        kind = it % 3
        if kind == 0:  # an unmasked launch: its sampler workgroups pre-draw placements between the masked ones
            ra, rb = a.step(acts), b.step(acts)
            for k in ("obs", "reward", "terminated", "truncated", "info"):
                _eq(k, ra[k], rb[k], it)
            sums.book(rb)
            continue
        auto_reset = kind == 1
        p = rng.choice([0.1, 0.5, 0.9])
        sel = rng.random(B) < p
        rows = np.flatnonzero(sel)
        before = env.get_state()
        _fill_sentinel(env)
        env.step_masked(dacts, torch.from_numpy(sel.astype(np.uint8)).to(env.device), auto_reset=auto_reset)
        masked_launches += 1
        got = _outputs(env)
        rb = _oracle_rows(b, acts, rows, auto_reset)
        for k in ("obs", "reward", "terminated", "truncated", "info"):
            _eq(f"stepped rows {k}", got[k][sel], rb[k][sel], it)
        _eq("masked-off obs rows", got["obs"][~sel], np.full_like(got["obs"][~sel], SENTINEL), it)
        _eq("masked-off reward", got["reward"][~sel], np.full(int((~sel).sum()), SENTINEL), it)
        _eq("masked-off info", got["info"][~sel], np.full_like(got["info"][~sel], SENTINEL), it)
        assert (got["terminated"][~sel] == 0xAB).all() and (got["truncated"][~sel] == 0xCD).all()
        after = env.get_state()
        for k in STATE_KEYS:
            _eq(f"masked-off {k}", after[k][~sel], before[k][~sel], it)
        _eq("positions", after["positions"], b.positions(), it)
        _eq("goals", after["goals"], b.goals(), it)
        _eq("rng words", after["rng_words"], b.rng_words(), it)
        done_rows = sums.book(rb, rows, reset_done=auto_reset)
        if not auto_reset and len(done_rows):  # next-step autoreset: the finished rows are reset by a masked reset
            m = np.zeros(B, np.uint8)
            m[done_rows] = 1
            obs = env.reset(torch.from_numpy(m).to(env.device)).cpu().numpy()
            for r in done_rows:
                _eq("masked reset obs", obs[r], b.envs[r].reset(), it)
            sums.steps[done_rows] = 0
        _eq("episode sums", env.episode_sums(), sums.want, it)
    env.poll_error()
    assert masked_launches == 60 and sums.want[ACC["EPISODES"]] > 0
    # an all-zero mask changes nothing
    before, sums0 = env.get_state(), env.episode_sums()
    _fill_sentinel(env)
    env.step_masked(torch.zeros((B, N), dtype=torch.int8, device=env.device), torch.zeros(B, dtype=torch.uint8, device=env.device))
    got, after = _outputs(env), env.get_state()
    assert (got["obs"] == SENTINEL).all() and (got["reward"] == SENTINEL).all() and (got["info"] == SENTINEL).all()
    assert (got["terminated"] == 0xAB).all() and (got["truncated"] == 0xCD).all()
    for k in STATE_KEYS:
        _eq(f"all-zero mask {k}", after[k], before[k])
    _eq("all-zero mask sums", env.episode_sums(), sums0)


def test_cte_all_ones_mask_equals_the_unmasked_step():
    import torch

    B, H, W, N, spe = 300, 16, 16, 4, 17
    cfg = {"env_name": "synthetic", "num_agents": N, "steps_per_episode": spe}
    grids = synth_grids(B, H, W, 0.2, N, base_seed=180_000)
    a, c = (CteEngineStepper(grids, cfg, seeds=list(range(B))) for _ in range(2))
    _eq("reset", a.reset(), c.reset())
    counts = np.arange(B) % spe
    a.env.set_step_counts(counts)
    c.env.set_step_counts(counts)
    ones = torch.ones(B, dtype=torch.uint8, device=a.env.device)
    rng = np.random.default_rng(5)
    for t in range(60):
        acts = torch.from_numpy(rng.integers(0, 5, size=(B, N)).astype(np.int8)).to(a.env.device)
        auto_reset = t % 4 != 3
        ra = _outputs_of(a.env.step_masked(acts, ones, auto_reset=auto_reset))
        rc = _outputs_of(c.env.step(acts, auto_reset=auto_reset))
        for k in ra:
            _eq(f"all-ones {k}", ra[k], rc[k], t)
        sa, sc = a.env.get_state(), c.env.get_state()
        for k in STATE_KEYS:
            _eq(k, sa[k], sc[k], t)
    _eq("sums", a.env.episode_sums(), c.env.episode_sums())
    assert a.env.episode_sums()[0] > B


def _outputs_of(out):
    return {k: out[k].cpu().numpy() for k in ("obs", "reward", "terminated", "truncated", "info")}
