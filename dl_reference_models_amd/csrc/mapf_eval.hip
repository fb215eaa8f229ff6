// mapf_eval.hip -- the evaluation recorder of libmapfstep.so: kernel, launch and its part of the C ABI (mapf_eval_begin /
// _record for multi-agent handles, mapf_cte_eval_begin / _record for the single-agent env, mapf_eval_end;
// include/mapf_step.h).
//
// The reference's test mode (main.py: test_trained_model) keeps, per episode, the reward of every agent, the number of
// steps, how the episode ended, where every agent started and where its goal lies, and -- over all episodes -- how often
// each cell held an agent after a step.  k_eval_record books all of that on the device, once after every step of an
// evaluation and before the reset of the envs that finished.
// It reads plane 0 of the agent state and the outputs of the step and writes the caller's record buffers, the handle's
// two running sums, `active` and `reset_mask`.  Nothing the step kernels read is touched.
// k_eval_trace, optional, keeps the plane-0 words of chosen envs per step next to it (mapf_eval_trace_begin /
// mapf_eval_trace), so that every frame of an episode can be redrawn later (mapf_render_words).

#include "mapf_handle.h"

namespace mapfk {

namespace {

constexpr int kEvalThreads = 256;

// One recorder for both kinds of handle; lanes are agents and G consecutive lanes own one env (G a power of two <= 64, so
// a group lies in one wavefront).
//   multi-agent (SINGLE = false): G is the engine's own group width.  One float reward per agent and a 14-float info row;
//     every agent carries its own running sum and the episode's total is the group's sum.
//   single-agent (SINGLE = true): main.py's loop restated for a gym.Env (reset(), step() until terminated or truncated,
//     episode_reward += reward).  G is the smallest power of two that holds N (the step kernels' group width is chosen for
//     the observation row and would leave most lanes idle here).  The env has ONE float64 reward and a 4-float info row, so
//     the running sum is one double per env, continued by lane 0 of the group in step order: run = run + reward[env] is
//     Python's `episode_reward += reward` bit for bit (the step rewards carry -0.2 and -0.05 terms, so the order matters and
//     no lanes' values are ever added up).
// No atomics on the visit counts: no two groups share an env, and inside an env the sequential move rule (MA-env:502-526,
// SA-env:259-274) lets an agent enter a cell only when no other agent stands on it, so after a step no two agents of an
// env hold the same cell.
template <bool SINGLE>
__global__ __launch_bounds__(kEvalThreads) void k_eval_record(EvalArgs ea) {
    constexpr int kInfo = SINGLE ? 4 : MAPF_INFO_ALL;
    constexpr int kSiteTable = SINGLE ? 24 : 13, kSiteCell = SINGLE ? 25 : 14;  // MAPF_CHK sites
    const Params &P = *ea.params;
    const int N = ea.N, G = ea.G, E = ea.E;
    const size_t f64_row = SINGLE ? 1 : 1 + (size_t)N;  // doubles of an episode in ep_f64
    const unsigned t = blockIdx.x * (unsigned)kEvalThreads + threadIdx.x;
    const int env = (int)(t / (unsigned)G), a = (int)(t - (unsigned)env * (unsigned)G);
    const bool env_ok = env < ea.B;
    // every read of what lane 0 rewrites below (active, episodes_recorded, the running sums) happens here, ahead of any store
    const bool on = env_ok && ea.active[env] != 0;
    const bool agent = on && a < N;
    uint32_t flags = 0;
    int k = 0, steps = 0;
    double run = 0.0;  // the running reward with this step's: the env's on lane 0 (SINGLE), else this agent's
    if (on) {
        flags = (ea.terminated[env] ? 1u : 0u) | (ea.truncated[env] ? 2u : 0u);  // (a time-limit end sets both, SA-env:347-348)
        k = ea.episodes_recorded[env];
        steps = ea.run_steps[env] + 1;
        if constexpr (SINGLE)
            if (a == 0) run = ea.run_reward[env] + static_cast<const double *>(ea.reward)[env];
    }
    const bool done = flags != 0;
    // (a full table would have cleared `active`; the test only bounds the addresses below)
    const bool record = done && (unsigned)k < (unsigned)E;
    MAPF_CHK(P, !done || record, kSiteTable, env, k);

    uint2 w = make_uint2(0u, 0u);
    const size_t ia = (size_t)env * N + a;
    if (agent) {
        w = ea.agents[ia];
        if constexpr (!SINGLE) {
            run = ea.run_reward[ia] + (double)static_cast<const float *>(ea.reward)[ia];
            ea.run_reward[ia] = done ? 0.0 : run;
        }
        // the cell the agent stands on after the step (main.py:265-267, bounds test included)
        const int r = (int)((w.x >> 8) & 255u), c = (int)(w.x & 255u);
        MAPF_CHK(P, r < ea.H && c < ea.W, kSiteCell, env, w.x & 0xFFFFu);
        if (r < ea.H && c < ea.W) ea.heat[((size_t)env * ea.H + r) * ea.W + c] += 1u;
    }
    double total = run;
    if constexpr (!SINGLE) {
        // total reward of the episode: the group's sum.  Rewards are multiples of 0.5, so every order of addition is exact.
        // Lanes outside the group's env, or of an env that idles, carry 0; no lane leaves before the exchange.
        for (int d = 1; d < G; d <<= 1) total += __shfl_xor(total, d);
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
            if constexpr (!SINGLE) ea.ep_f64[rec * f64_row + 1 + a] = run;
        }
        for (int j = a; j < kInfo; j += G) ea.ep_info[rec * kInfo + j] = ea.info[(size_t)env * kInfo + j];
    }
    // values that are one per env leave through lane 0 of the group as ordinary vector stores
    if (on && a == 0) {
        if (record) {
            const size_t rec = (size_t)env * E + k;
            ea.ep_i32[rec * (size_t)(2 + 4 * N)] = steps;
            ea.ep_i32[rec * (size_t)(2 + 4 * N) + 1] = (int32_t)flags;
            ea.ep_f64[rec * f64_row] = total;
            ea.episodes_recorded[env] = k + 1;
        }
        const bool more = done && k + 1 < E;
        if constexpr (SINGLE) ea.run_reward[env] = done ? 0.0 : run;
        ea.run_steps[env] = done ? 0 : steps;
        ea.reset_mask[env] = more ? 1 : 0;
        if (done && !more) ea.active[env] = 0;
    }
}

// The trace of an evaluation: lanes are (traced env k, agent), K * N of them, and each copies one plane-0 word into the
// slot (k, episode v, step t) its phase names (include/mapf_step.h above mapf_eval_trace_begin).  v and t come from the
// recorder's own counters, read as the phase finds them: STEP runs before k_eval_record, RESET after it.  Every episode
// ends at the step limit S at the latest, so a slot is a fixed address: no cursor, no atomic, and no two lanes share one.
// It reads the recorder's buffers and writes `words` only.
__global__ __launch_bounds__(kEvalThreads) void k_eval_trace(TraceArgs ta) {
    const Params &P = *ta.params;
    const int N = ta.N;
    const unsigned t = blockIdx.x * (unsigned)kEvalThreads + threadIdx.x;
    const int k = (int)(t / (unsigned)N), a = (int)(t - (unsigned)k * (unsigned)N);
    if (k >= ta.K) return;
    const int env = ta.env_ids[k];
    if ((unsigned)env >= (unsigned)ta.B) {
        if (a == 0) raise_error(P, MAPF_ERR_CONFIG, k, 0, env);
        return;
    }
    const int v = ta.episodes_recorded[env];  // STEP: the running episode; RESET: the one that just started; START: 0
    if ((unsigned)v >= (unsigned)ta.V) return;
    int step = 0;
    if (ta.phase == MAPF_TRACE_STEP) {
        if (ta.active[env] == 0) return;
        step = ta.run_steps[env] + 1;
    } else if (ta.phase == MAPF_TRACE_RESET) {
        if (ta.reset_mask[env] == 0) return;
    }
    MAPF_CHK(P, (unsigned)step <= (unsigned)ta.S, 26, env, step);
    if ((unsigned)step > (unsigned)ta.S) return;  // (cannot happen: the step kernels truncate at S)
    const size_t slot = ((size_t)k * ta.V + (ta.phase == MAPF_TRACE_START ? 0 : v)) * (size_t)(ta.S + 1) + step;
    ta.words[slot * N + a] = ta.agents[(size_t)env * N + a].x;
}

hipError_t launch_eval_trace(const TraceArgs &ta, hipStream_t s) {
    const dim3 grid((unsigned)(((size_t)ta.K * ta.N + kEvalThreads - 1) / kEvalThreads));
    LAUNCH_CHECKED(k_eval_trace, grid, dim3(kEvalThreads), 0, s, ta);
}

constexpr int cte_eval_group_width(int N) { return N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : N <= 32 ? 32 : 64; }

hipError_t launch_eval_record(const EvalArgs &ea, bool single, hipStream_t s) {
    const dim3 grid((unsigned)(((size_t)ea.B * ea.G + kEvalThreads - 1) / kEvalThreads));
    if (single) LAUNCH_CHECKED(k_eval_record<true>, grid, dim3(kEvalThreads), 0, s, ea);
    LAUNCH_CHECKED(k_eval_record<false>, grid, dim3(kEvalThreads), 0, s, ea);
}

int eval_begin(mapf_engine *e, bool single, int32_t episodes_per_env, uint32_t *heat, int32_t *ep_i32, double *ep_f64, float *ep_info,
               int32_t *episodes_recorded, uint8_t *active, uint8_t *reset_mask, void *stream) {
    const std::string fn = single ? "mapf_cte_eval_begin" : "mapf_eval_begin";
    if (!e || !heat || !ep_i32 || !ep_f64 || !ep_info || !episodes_recorded || !active || !reset_mask)
        return fail(e, MAPF_ERR_CONFIG, fn + ": null argument");
    if (episodes_per_env < 1) return fail(e, MAPF_ERR_CONFIG, fn + ": episodes_per_env must be >= 1");
    if (e->cte != single)
        return fail(e, MAPF_ERR_STATE, single ? "mapf_cte_eval_begin: not a MAPF_FLAG_SINGLE_AGENT handle (use mapf_eval_begin)"
                                              : "mapf_eval_begin: handle was created with MAPF_FLAG_SINGLE_AGENT (the recorder is for multi-agent handles)");
    // a group of the recorder is a power of two of lanes inside one wavefront that holds every agent of its env
    const int G = single ? cte_eval_group_width(e->p.N) : e->lpe;
    if (G < e->p.N || G > 64 || (G & (G - 1)) != 0) return fail(e, MAPF_ERR_INTERNAL, fn + ": the handle's group width cannot hold its agents");
    const size_t B = (size_t)e->p.B, HW = (size_t)e->p.HW, sums = single ? B : B * (size_t)e->p.N;
    ON_DEVICE(e);
    if (!e->d_eval_reward) HIP_TRY(e, hipMalloc(&e->d_eval_reward, sums * sizeof(double)));
    if (!e->d_eval_steps) HIP_TRY(e, hipMalloc(&e->d_eval_steps, B * sizeof(int32_t)));
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(e, hipMemsetAsync(heat, 0, B * HW * sizeof(uint32_t), s));
    HIP_TRY(e, hipMemsetAsync(episodes_recorded, 0, B * sizeof(int32_t), s));
    HIP_TRY(e, hipMemsetAsync(reset_mask, 0, B, s));
    HIP_TRY(e, hipMemsetAsync(active, 1, B, s));
    HIP_TRY(e, hipMemsetAsync(e->d_eval_reward, 0, sums * sizeof(double), s));
    HIP_TRY(e, hipMemsetAsync(e->d_eval_steps, 0, B * sizeof(int32_t), s));
    e->eval = EvalArgs{env_view(e)};
    EvalArgs &ea = e->eval;
    ea.active = active;
    ea.reset_mask = reset_mask;
    ea.heat = heat;
    ea.ep_i32 = ep_i32;
    ea.ep_f64 = ep_f64;
    ea.ep_info = ep_info;
    ea.episodes_recorded = episodes_recorded;
    ea.run_reward = e->d_eval_reward;
    ea.run_steps = e->d_eval_steps;
    ea.E = episodes_per_env;
    ea.G = G;
    e->eval_on = true;
    e->trace_on = false;  // (a trace belongs to one evaluation: mapf_eval_trace_begin follows this call)
    return MAPF_OK;
}

int eval_record(mapf_engine *e, bool single, const void *reward, const uint8_t *terminated, const uint8_t *truncated, const float *info,
                void *stream) {
    const std::string fn = single ? "mapf_cte_eval_record" : "mapf_eval_record", begin = single ? "mapf_cte_eval_begin" : "mapf_eval_begin";
    if (!e || !reward || !terminated || !truncated || !info) return fail(e, MAPF_ERR_CONFIG, fn + ": null argument");
    if (e->cte != single)
        return fail(e, MAPF_ERR_STATE, single ? "mapf_cte_eval_record: not a MAPF_FLAG_SINGLE_AGENT handle (use mapf_eval_record)"
                                              : "mapf_eval_record: handle was created with MAPF_FLAG_SINGLE_AGENT");
    if (!e->grids_set) return fail(e, MAPF_ERR_STATE, "mapf_set_grids must be called before " + fn);
    if (!e->eval_on) return fail(e, MAPF_ERR_STATE, begin + " must be called before " + fn);
    EvalArgs ea = e->eval;
    ea.reward = reward;
    ea.terminated = terminated;
    ea.truncated = truncated;
    ea.info = info;
    ON_DEVICE(e);
    HIP_TRY(e, launch_eval_record(ea, single, (hipStream_t)stream));
    return MAPF_OK;
}

int eval_trace_begin(mapf_engine *e, int32_t K, const int32_t *env_ids, int32_t episodes, uint32_t *words) {
    if (!e || !env_ids || !words) return fail(e, MAPF_ERR_CONFIG, "mapf_eval_trace_begin: null argument");
    if (K < 1) return fail(e, MAPF_ERR_CONFIG, "mapf_eval_trace_begin: K must be >= 1");
    if (episodes < 1) return fail(e, MAPF_ERR_CONFIG, "mapf_eval_trace_begin: episodes must be >= 1");
    if ((uint64_t)K * (uint64_t)e->p.N > 0x7FFFFFFFull) return fail(e, MAPF_ERR_CONFIG, "mapf_eval_trace_begin: too many envs for one launch");
    if (!e->eval_on) return fail(e, MAPF_ERR_STATE, "mapf_eval_begin / mapf_cte_eval_begin must be called before mapf_eval_trace_begin");
    const EvalArgs &ea = e->eval;
    e->trace = TraceArgs{ea.params, ea.agents, ea.active, ea.reset_mask, ea.episodes_recorded, ea.run_steps, env_ids, words,
                         ea.B, ea.N, K, episodes, e->p.steps_per_episode, MAPF_TRACE_START};
    e->trace_on = true;
    return MAPF_OK;
}

int eval_trace(mapf_engine *e, int32_t phase, void *stream) {
    if (!e) return fail(e, MAPF_ERR_CONFIG, "mapf_eval_trace: null argument");
    if (phase != MAPF_TRACE_START && phase != MAPF_TRACE_STEP && phase != MAPF_TRACE_RESET)
        return fail(e, MAPF_ERR_CONFIG, "mapf_eval_trace: unknown phase");
    if (!e->eval_on) return fail(e, MAPF_ERR_STATE, "mapf_eval_begin / mapf_cte_eval_begin must be called before mapf_eval_trace");
    if (!e->trace_on) return fail(e, MAPF_ERR_STATE, "mapf_eval_trace_begin must be called before mapf_eval_trace");
    if (!e->grids_set) return fail(e, MAPF_ERR_STATE, "mapf_set_grids must be called before mapf_eval_trace");
    TraceArgs ta = e->trace;
    ta.phase = phase;
    ON_DEVICE(e);
    HIP_TRY(e, launch_eval_trace(ta, (hipStream_t)stream));
    return MAPF_OK;
}

}  // namespace

}  // namespace mapfk

using namespace mapfk;

extern "C" {

int mapf_eval_begin(mapf_handle e, int32_t episodes_per_env, uint32_t *heat, int32_t *ep_i32, double *ep_f64, float *ep_info,
                    int32_t *episodes_recorded, uint8_t *active, uint8_t *reset_mask, void *stream) {
    return eval_begin(e, false, episodes_per_env, heat, ep_i32, ep_f64, ep_info, episodes_recorded, active, reset_mask, stream);
}

int mapf_cte_eval_begin(mapf_handle e, int32_t episodes_per_env, uint32_t *heat, int32_t *ep_i32, double *ep_f64, float *ep_info,
                        int32_t *episodes_recorded, uint8_t *active, uint8_t *reset_mask, void *stream) {
    return eval_begin(e, true, episodes_per_env, heat, ep_i32, ep_f64, ep_info, episodes_recorded, active, reset_mask, stream);
}

int mapf_eval_record(mapf_handle e, const float *rewards, const uint8_t *terminated, const uint8_t *truncated,
                     const float *info_all, void *stream) {
    return eval_record(e, false, rewards, terminated, truncated, info_all, stream);
}

int mapf_cte_eval_record(mapf_handle e, const double *reward, const uint8_t *terminated, const uint8_t *truncated,
                         const float *info, void *stream) {
    return eval_record(e, true, reward, terminated, truncated, info, stream);
}

int mapf_eval_trace_begin(mapf_handle e, int32_t K, const int32_t *env_ids, int32_t episodes, uint32_t *words, void *stream) {
    (void)stream;  // (nothing is enqueued: the words need no clearing)
    return eval_trace_begin(e, K, env_ids, episodes, words);
}

int mapf_eval_trace(mapf_handle e, int32_t phase, void *stream) { return eval_trace(e, phase, stream); }

int mapf_eval_end(mapf_handle e) {
    if (!e) return MAPF_ERR_CONFIG;
    e->trace_on = false;
    if (!e->eval_on && !e->d_eval_reward && !e->d_eval_steps) return MAPF_OK;
    ON_DEVICE(e);
    e->eval_on = false;
    HIP_TRY(e, hipDeviceSynchronize());  // (no recorder launch may still be using the sums freed below)
    hipError_t first = hipFree(e->d_eval_reward);
    const hipError_t rc = hipFree(e->d_eval_steps);
    e->d_eval_reward = nullptr;
    e->d_eval_steps = nullptr;
    if (first == hipSuccess) first = rc;
    HIP_TRY(e, first);
    return MAPF_OK;
}

}  // extern "C"
