// mapf_eval.hip -- the evaluation recorders of libmapfstep.so (mapf_eval_record and, for the single-agent env,
// mapf_cte_eval_record; include/mapf_step.h), one launch unit.
//
// The reference's test mode (main.py: test_trained_model) keeps, per episode, the reward of every agent, the number of
// steps, how the episode ended, where every agent started and where its goal lies, and -- over all episodes -- how often
// each cell held an agent after a step.  k_eval_record books all of that on the device, once after every step of an
// evaluation and before the reset of the envs that finished:
//   lanes are agents, lpe consecutive lanes own one env (the engine's own grouping; a group never spans a wavefront), so
//   no two groups write the same address, and inside a group no two agents stand on the same cell: no atomics.
// It reads plane 0 of the agent state and the outputs of the step and writes the caller's record buffers, the handle's
// two running sums, `active` and `reset_mask`.  Nothing the step kernels read is touched.  Values that are one per env
// leave through lane 0 of the group as ordinary vector stores.

#include "mapf_engine.h"

namespace mapfk {

namespace {

__global__ __launch_bounds__(kEvalThreads) void k_eval_record(EvalArgs ea) {
    const Params &P = *ea.params;
    const int N = ea.N, lpe = ea.lpe, E = ea.E;
    const unsigned t = blockIdx.x * (unsigned)kEvalThreads + threadIdx.x;
    const int env = (int)(t / (unsigned)lpe), a = (int)(t - (unsigned)env * (unsigned)lpe);
    const bool env_ok = env < ea.B;
    // every read of what lane 0 rewrites below (active, episodes_recorded, run_steps) happens here, ahead of any store
    const bool on = env_ok && ea.active[env] != 0;
    const bool agent = on && a < N;
    uint32_t flags = 0;
    int k = 0, steps = 0;
    if (on) {
        flags = (ea.terminated[env] ? 1u : 0u) | (ea.truncated[env] ? 2u : 0u);
        k = ea.episodes_recorded[env];
        steps = ea.run_steps[env] + 1;
    }
    const bool done = flags != 0;
    // (a full table would have cleared `active`; the test only bounds the addresses below)
    const bool record = done && (unsigned)k < (unsigned)E;
    MAPF_CHK(P, !done || record, 13, env, k);

    double mine = 0.0;
    uint2 w = make_uint2(0u, 0u);
    const size_t ia = (size_t)env * N + a;
    if (agent) {
        w = ea.agents[ia];
        mine = ea.run_reward[ia] + (double)ea.rewards[ia];
        ea.run_reward[ia] = done ? 0.0 : mine;
        // the cell the agent stands on after the step (main.py:265-267, bounds test included)
        const int r = (int)((w.x >> 8) & 255u), c = (int)(w.x & 255u);
        MAPF_CHK(P, r < ea.H && c < ea.W, 14, env, w.x & 0xFFFFu);
        if (r < ea.H && c < ea.W) ea.heat[((size_t)env * ea.H + r) * ea.W + c] += 1u;
    }
    // total reward of the episode: the group's sum.  Rewards are multiples of 0.5, so every order of addition is exact.
    // Lanes outside the group's env, or of an env that idles, carry 0; no lane leaves before the exchange.
    double total = mine;
    for (int d = 1; d < lpe; d <<= 1) total += __shfl_xor(total, d);

    if (record) {
        const size_t rec = (size_t)env * E + k;
        if (agent) {
            int32_t *o = ea.ep_i32 + rec * (size_t)(2 + 4 * N) + 2 + 4 * a;
            const uint32_t start = w.y & 0xFFFFu, goal = w.x >> 16;
            o[0] = (int32_t)(start >> 8);
            o[1] = (int32_t)(start & 255u);
            o[2] = (int32_t)(goal >> 8);
            o[3] = (int32_t)(goal & 255u);
            ea.ep_f64[rec * (size_t)(1 + N) + 1 + a] = mine;
        }
        for (int j = a; j < MAPF_INFO_ALL; j += lpe) ea.ep_info[rec * MAPF_INFO_ALL + j] = ea.info_all[(size_t)env * MAPF_INFO_ALL + j];
    }
    if (on && a == 0) {
        if (record) {
            const size_t rec = (size_t)env * E + k;
            ea.ep_i32[rec * (size_t)(2 + 4 * N)] = steps;
            ea.ep_i32[rec * (size_t)(2 + 4 * N) + 1] = (int32_t)flags;
            ea.ep_f64[rec * (size_t)(1 + N)] = total;
            ea.episodes_recorded[env] = k + 1;
        }
        const bool more = done && k + 1 < E;
        ea.run_steps[env] = done ? 0 : steps;
        ea.reset_mask[env] = more ? 1 : 0;
        if (done && !more) ea.active[env] = 0;
    }
}

// The same bookkeeping for the single-agent (CTE) env: main.py's loop restated for a gym.Env (reset(), step() until
// terminated or truncated, episode_reward += reward).  The env has ONE float64 reward and one 4-float info row, so the
// running sum is one double per env, continued by lane 0 of the group in step order: run = run + reward[env] is Python's
// `episode_reward += reward` bit for bit (the step rewards carry -0.2 and -0.05 terms, so the order matters and no lanes'
// values are ever added up).  Lanes are agents, G consecutive lanes own one env (G a power of two <= 64: a group lies in
// one wavefront, and its lanes exchange nothing).  No atomics on the visit counts: no two groups share an env, and inside
// an env the sequential move rule of SA-env:259-274 lets an agent enter a cell only when no other agent stands on it, so
// after a step no two agents of an env hold the same cell.  Reads plane 0 of the agent state and the step's outputs;
// writes the record buffers, the two running sums, `active` and `reset_mask`.  Values that are one per env leave through
// lane 0 of the group as ordinary vector stores.
__global__ __launch_bounds__(kEvalThreads) void k_cte_eval_record(CteEvalArgs ea) {
    const Params &P = *ea.params;
    const int N = ea.N, G = ea.G, E = ea.E;
    const unsigned t = blockIdx.x * (unsigned)kEvalThreads + threadIdx.x;
    const int env = (int)(t / (unsigned)G), a = (int)(t - (unsigned)env * (unsigned)G);
    const bool env_ok = env < ea.B;
    // every read of what lane 0 rewrites below (active, episodes_recorded, the running sums) happens here, ahead of any store
    const bool on = env_ok && ea.active[env] != 0;
    const bool agent = on && a < N;
    uint32_t flags = 0;
    int k = 0, steps = 0;
    double run = 0.0;
    if (on) {
        flags = (ea.terminated[env] ? 1u : 0u) | (ea.truncated[env] ? 2u : 0u);  // (a time-limit end sets both, SA-env:347-348)
        k = ea.episodes_recorded[env];
        steps = ea.run_steps[env] + 1;
        if (a == 0) run = ea.run_reward[env] + ea.reward[env];
    }
    const bool done = flags != 0;
    // (a full table would have cleared `active`; the test only bounds the addresses below)
    const bool record = done && (unsigned)k < (unsigned)E;
    MAPF_CHK(P, !done || record, 24, env, k);

    uint2 w = make_uint2(0u, 0u);
    if (agent) {
        w = ea.agents[(size_t)env * N + a];
        const int r = (int)((w.x >> 8) & 255u), c = (int)(w.x & 255u);
        MAPF_CHK(P, r < ea.H && c < ea.W, 25, env, w.x & 0xFFFFu);
        if (r < ea.H && c < ea.W) ea.heat[((size_t)env * ea.H + r) * ea.W + c] += 1u;
    }
    if (record) {
        const size_t rec = (size_t)env * E + k;
        if (agent) {
            int32_t *o = ea.ep_i32 + rec * (size_t)(2 + 4 * N) + 2 + 4 * a;
            const uint32_t start = w.y & 0xFFFFu, goal = w.x >> 16;
            o[0] = (int32_t)(start >> 8);
            o[1] = (int32_t)(start & 255u);
            o[2] = (int32_t)(goal >> 8);
            o[3] = (int32_t)(goal & 255u);
        }
        for (int j = a; j < 4; j += G) ea.ep_info[rec * 4 + j] = ea.info[(size_t)env * 4 + j];
    }
    if (on && a == 0) {
        if (record) {
            const size_t rec = (size_t)env * E + k;
            ea.ep_i32[rec * (size_t)(2 + 4 * N)] = steps;
            ea.ep_i32[rec * (size_t)(2 + 4 * N) + 1] = (int32_t)flags;
            ea.ep_f64[rec] = run;
            ea.episodes_recorded[env] = k + 1;
        }
        const bool more = done && k + 1 < E;
        ea.run_reward[env] = done ? 0.0 : run;
        ea.run_steps[env] = done ? 0 : steps;
        ea.reset_mask[env] = more ? 1 : 0;
        if (done && !more) ea.active[env] = 0;
    }
}

}  // namespace

hipError_t launch_eval_record(const EvalArgs &ea, hipStream_t s) {
    const unsigned blocks = (unsigned)(((size_t)ea.B * ea.lpe + kEvalThreads - 1) / kEvalThreads);
    LAUNCH_CHECKED(k_eval_record, dim3(blocks), dim3(kEvalThreads), 0, s, ea);
}

hipError_t launch_cte_eval_record(const CteEvalArgs &ea, hipStream_t s) {
    const unsigned blocks = (unsigned)(((size_t)ea.B * ea.G + kEvalThreads - 1) / kEvalThreads);
    LAUNCH_CHECKED(k_cte_eval_record, dim3(blocks), dim3(kEvalThreads), 0, s, ea);
}

}  // namespace mapfk
