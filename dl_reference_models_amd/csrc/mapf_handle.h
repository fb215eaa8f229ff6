// mapf_handle.h -- internal to libmapfstep.so, host only: the engine handle and what the C ABI of any unit needs to work
// on one.
//
// mapf_step.hip (create, state, step) and the handle-bound side units (mapf_render.hip, mapf_eval.hip, mapf_plan.hip) each
// end with their own part of the C ABI of include/mapf_step.h.  They share the handle's definition, the error report
// (`fail`, defined once in mapf_step.hip), HIP_TRY / ON_DEVICE, the env view every side kernel's arguments start with and
// the workspace growth of the planners.  The launch units (mapf_launch.hip) see mapf_engine.h only.

#ifndef MAPF_HANDLE_H
#define MAPF_HANDLE_H

#include <string>
#include <vector>

#include "mapf_engine.h"

namespace mapfk {

// What every side kernel reads of a handle; its argument struct derives from this (a trivially copyable aggregate, passed
// by value) and the host fills it with env_view().
struct EnvView {
    const Params *params;  // the handle's Params: error record (bad env id, MAPF_CHK)
    const uint2 *agents;   // plane 0 of the agent state
    const uint64_t *rows;  // [B][H] obstacle rows, bit col + col_pad
    int B, H, W, N, col_pad;
};

// Evaluation recorder (mapf_eval.hip): one launch after every step of an evaluation.  Lanes are agents, G lanes own one
// env; the record layouts are in include/mapf_step.h above mapf_eval_begin and mapf_cte_eval_begin.  The handle keeps the
// record bound by begin, so the struct lives here; where the two kinds of handle differ the single-agent form is second.
struct EvalArgs : EnvView {
    const void *reward;          // of the step just made: float [B][N] | double [B]
    const uint8_t *terminated;   // [B]
    const uint8_t *truncated;    // [B]
    const float *info;           // [B][14] | [B][4]
    uint8_t *active;             // [B] the mask the step was launched with; cleared after an env's E-th episode
    uint8_t *reset_mask;         // [B] out: 1 = the env ended an episode and runs another
    uint32_t *heat;              // [B][H][W]
    int32_t *ep_i32;             // [B][E][2 + 4N]
    double *ep_f64;              // [B][E][1 + N] | [B][E]
    float *ep_info;              // [B][E][14] | [B][E][4]
    int32_t *episodes_recorded;  // [B]
    double *run_reward;          // reward of the running episode (handle-owned): [B][N] per agent | [B], added up in step order
    int32_t *run_steps;          // [B] steps of the running episode (handle-owned)
    int E, G;
};

// Evaluation trace (mapf_eval.hip: k_eval_trace): the plane-0 words of K chosen envs, one fixed slot per (k, episode, step).
// mapf_eval_trace_begin binds it to the handle next to the recorder's buffers, which the kernel reads; `phase` is set per call.
struct TraceArgs {
    const Params *params;              // error record (bad env id, MAPF_CHK)
    const uint2 *agents;               // plane 0 of the agent state
    const uint8_t *active;             // [B] the recorder's
    const uint8_t *reset_mask;         // [B] the recorder's
    const int32_t *episodes_recorded;  // [B] the recorder's
    const int32_t *run_steps;          // [B] the recorder's (handle-owned)
    const int32_t *env_ids;            // [K]
    uint32_t *words;                   // [K][V][S + 1][N]
    int B, N, K, V, S, phase;
};

}  // namespace mapfk

struct mapf_engine {
    mapf_config cfg;
    mapfk::Params p;
    int lpe = 0;
    int cus = 256;  // compute units of the device (mapf_plan_windowed: does a launch stay resident?)
    int mask_w = 32;
    int special = 0;  // id in MAPF_SPECIALIZATIONS, 0 = runtime-config kernel
    int dense = 0;    // the step grid has more than three waves per SIMD: the 128-register build of k_step (WPS = 4)
    int many_dense = 0;  // the fused launch has more than two waves per SIMD: the 128-register build of k_step_many
    int obs_prepared = 0;  // k_step3 with bit rows (goals / old cells / intents: obs3_wave_prepared, state3_outputs; Io::use_map bit 1)
    int three_wave = 0;  // k_step3 (state / observation / aux wave): specialised finite shapes with N = 4 or 8, not dense
    int rt_sliced = 0;   // runtime-config kernels with the sliced background draw (KRuntimeSliced): full groups of 4 / 8 agents
    int wide3 = 0;       // k_stepw: 64-lane groups with the cell-map conditions met step on the three-wave kernel with bit rows
    int wide_lds_bytes = 0;
    // step kernels compiled for exactly this configuration at mapf_create (MAPF_FLAG_JIT_SPECIALIZE), else null
    hipFunction_t jit_step = nullptr, jit_many = nullptr;
    std::string jit_note = "not requested (MAPF_FLAG_JIT_SPECIALIZE)";
    bool cte = false;  // single-agent (CTE) variant
    int col_pad = 0;   // kRowPad when W <= 64 - 2*kRowPad
    int use_map = 0, lds_map_off = 0;  // LDS cell-map path of wide groups
    double cte_blocking_penalty = -0.2, cte_move_after_goal_penalty = -0.05;  // SA-env:92-93
    // single-agent env, fused launches (mapf_cte_step_many, T > 1): their own group width and LDS layout (mapf_create)
    int cte_scratch2_off = 0;
    struct CteManyPlan { int lpe = 0, blocks = 0, lds_bytes = 0, tab_off = 0, stage_off = 0, scratch_off = 0; } cte_many;
    int blocks = 0;
    int sampler_blocks = 0;  // k_step only: workgroups appended to the grid that pre-draw next-episode placements
    int lds_bytes = 0;
    bool grids_set = false;
    std::vector<uint64_t> h_rows;  // host copy of the obstacle rows (mapf_set_state validates injected positions against it)
    std::string err;
    // device allocations
    uint2 *d_agents = nullptr;  // the planes of the agent state (mapf_kernels.inl: agent_plane_off)
    uint32_t bn8 = 0;           // agent_bn8(B, N, layout): the plane stride, bit 0 = compact history planes, bit 1 = derived distance
    uint2 *d_agents_derived = nullptr;  // the 16-byte planes a demoted handle left (demote_derived), freed with the handle
    int planned_sliced = 0;     // the launch shape was planned for a sliced background draw (what a demoted handle steps with)
    int *d_scal = nullptr;
    int16_t *d_ring = nullptr;
    uint64_t *d_rng = nullptr;
    uint64_t *d_rows = nullptr;
    uint16_t *d_free_cells = nullptr;
    uint16_t *d_free_rank = nullptr;
    int *d_n_free = nullptr;
    int *d_err = nullptr;
    int *d_ep_acc = nullptr;
    uint32_t *d_stage_vals = nullptr;  // [B][2N] bounded draws of a staged background draw (Params::stage_vals)
    uint64_t *d_jump_c = nullptr;   // [B][32][2] S_q * inc of every env's stream (Io::jump_c), rewritten whenever the streams are set
    uint64_t *d_vis_rng = nullptr;  // [B][6] visible stream state of envs whose placement slot is pending (Params::vis_rng)
    mapfk::Params *d_params = nullptr;  // device copy of `p`, read by the kernels through a pointer
    unsigned long long *d_dbg = nullptr;  // stamps buffer (diagnostic build only)
    // mapf_bind_outputs: the caller's output buffers for mapf_step_bound
    float *b_obs = nullptr, *b_rewards = nullptr, *b_info_all = nullptr;
    uint8_t *b_terminated = nullptr, *b_truncated = nullptr, *b_info_agent = nullptr;
    bool bound = false;
    // mapf_eval_begin / mapf_cte_eval_begin: the caller's record buffers and the running sums of the episodes in flight
    // (handle-owned)
    mapfk::EvalArgs eval;
    double *d_eval_reward = nullptr;  // [B][N]; single-agent handles: [B]
    int32_t *d_eval_steps = nullptr;  // [B]
    uint64_t *d_plan_hist = nullptr;  // mapf_plan_prioritized's workspace: [B][horizon + 1][G] reach rows
    size_t plan_hist_bytes = 0;
    uint8_t *d_cbs_ws = nullptr;  // mapf_plan_cbs's workspace: reach rows, root paths and node records of every env
    size_t cbs_ws_bytes = 0;
    bool eval_on = false;
    mapfk::TraceArgs trace;  // mapf_eval_trace_begin: the caller's words, bound until mapf_eval_end or the next *_eval_begin
    bool trace_on = false;
};

namespace mapfk {

// Records `msg` on the handle (on the calling thread's create error when there is none) and returns `code`.
int fail(mapf_engine *e, int code, const std::string &msg);

#define HIP_TRY(e, call)                                                                                  \
    do {                                                                                                  \
        hipError_t _s = (call);                                                                           \
        if (_s != hipSuccess)                                                                             \
            return fail((e), MAPF_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(_s));            \
    } while (0)

// Makes the handle's GPU current for the duration of an ABI call and puts the caller's device back on every exit
// path: a process that holds envs on several GPUs (or whose torch current device differs) must not find its
// thread's device switched by a step() or by a destructor run from the garbage collector.
struct DeviceScope {
    int prev = -1;
    hipError_t status = hipSuccess;
    explicit DeviceScope(int dev) {
        status = hipGetDevice(&prev);
        if (status != hipSuccess) { prev = -1; return; }
        if (prev != dev) status = hipSetDevice(dev); else prev = -1;  // hot path: nothing to do, nothing to undo
    }
    ~DeviceScope() { if (prev >= 0) (void)hipSetDevice(prev); }
    DeviceScope(const DeviceScope &) = delete;
    DeviceScope &operator=(const DeviceScope &) = delete;
};
#define ON_DEVICE(e)                                                                                       \
    DeviceScope _dev_scope((e)->cfg.device);                                                               \
    if (_dev_scope.status != hipSuccess)                                                                   \
        return fail((e), MAPF_ERR_HIP, std::string("selecting the handle's device: ") + hipGetErrorString(_dev_scope.status))

inline EnvView env_view(const mapf_engine *e) {
    return {e->d_params, e->d_agents, e->d_rows, e->p.B, e->p.H, e->p.W, e->p.N, e->col_pad};
}

// Grows a workspace of the handle to `need` bytes; one that is large enough already is left alone, so a call that needs
// no more than an earlier one allocates nothing.
template <typename T>
int grow_workspace(mapf_engine *e, T *&ptr, size_t &bytes, size_t need) {
    if (bytes >= need) return MAPF_OK;
    if (ptr) HIP_TRY(e, hipFree(ptr));  // (waits for the device: earlier launches are done with it)
    ptr = nullptr;
    bytes = 0;
    HIP_TRY(e, hipMalloc(&ptr, need));
    bytes = need;
    return MAPF_OK;
}

}  // namespace mapfk

#endif  // MAPF_HANDLE_H
