// mapf_engine.h -- internal to libmapfstep.so: what the translation units of the library share.
//
// The library is built from one host translation unit (mapf_step.hip: the C ABI of include/mapf_step.h) and a set of
// LAUNCH units (mapf_launch.hip compiled once per -DMAPF_TU_* selection), each of which instantiates the kernels of one
// group -- one prebuilt specialisation, the runtime-config kernels of one group width and window-mask width, the
// single-agent kernels of one group width -- behind plain functions declared here.  The units compile in parallel
// (dl_reference_models_amd/build.py); a cold build of the whole library is the longest unit, not the sum.
//
// Device code lives in mapf_kernels.inl, compiled under the named namespace `mapfk` so that the types the units
// exchange (Io, Params, ManyPolicy, ...) are the same types in every unit.

#ifndef MAPF_ENGINE_H
#define MAPF_ENGINE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapf_step.h"

#ifndef MAPF_NS
#define MAPF_NS mapfk
#endif
#include "mapf_kernels.inl"

namespace mapfk {

// Group widths and window-mask widths the library holds.  Reduced builds (development / checking: dl_reference_models_amd/
// build.py selects the launch units to match) cut them down; mapf_create refuses what a reduced build does not hold.
#if defined(MAPF_DEV_C3)  // the headline shape only
#define MAPF_FOR_LPE(X) X(8)
#define MAPF_FOR_MW(X, L) X(L, 32)
#elif defined(MAPF_DEV_CTE)  // the single-agent env at 8 and 64 lanes per env
#define MAPF_FOR_LPE(X) X(8) X(64)
#define MAPF_FOR_MW(X, L) X(L, 32)
#elif defined(MAPF_DEV_N16)  // groups of 16 lanes, 7 x 7 windows: the reference's training setup
#define MAPF_FOR_LPE(X) X(16)
#define MAPF_FOR_MW(X, L) X(L, 64)
#elif defined(MAPF_DEV_C5)  // the c5 shape only -- one wavefront per env, 5 x 5 windows
#define MAPF_FOR_LPE(X) X(64)
#define MAPF_FOR_MW(X, L) X(L, 32)
#elif defined(MAPF_SMALL_SHAPES)  // the checking build: groups of 4, 8 and 16 lanes (either env), windows up to 7 x 7
#define MAPF_FOR_LPE(X) X(4) X(8) X(16)
#define MAPF_FOR_MW(X, L) X(L, 32) X(L, 64)
#else
#define MAPF_FOR_LPE(X) X(4) X(8) X(16) X(32) X(64)
#define MAPF_FOR_MW(X, L) X(L, 32) X(L, 64) X(L, 128)
#endif
#if defined(MAPF_DEV_C3) || defined(MAPF_DEV_N16) || defined(MAPF_DEV_C5)
#define MAPF_NO_CTE_KERNELS 1
#endif

// What a launch unit needs to know about a handle (the host unit fills it from mapf_engine).
struct LaunchPlan {
    const Params *d_params;
    int blocks;          // env workgroups
    int sampler_blocks;  // k_step only: workgroups of the grid that pre-draw next-episode placements
    int lds_bytes;
    int dense;           // k_step: the 128-register build (more than three waves per SIMD in one launch)
    int many_dense;      // k_step_many: idem (more than two)
    int three_wave;      // k_step3
    int rt_sliced;       // runtime-config kernels with the sliced background draw (KRuntimeSliced)
    int wide3;           // k_stepw: the three-wave kernel of 64-lane groups (one env per workgroup, bit rows in LDS)
    int wide_lds_bytes;  // its dynamic LDS
};

enum { KIND_RESET = 0, KIND_STEP = 1, KIND_OBSERVE = 2 };

// observation-window mask width of a sensor range
constexpr int mask_width_for(int sr) {
    return (2 * sr + 1) * (2 * sr + 1) <= 32 ? 32 : ((2 * sr + 1) * (2 * sr + 1) <= 64 ? 64 : 128);
}

// ---- the launch units' entry points (mapf_launch.hip) ----------------------------------------------------------------
// prebuilt specialisations: one unit per id of MAPF_SPECIALIZATIONS
#define MAPF_DECLARE_SPECIAL(ID, N_, SR_, FLAGS_, DW_, LW_, NEARBY_, MINN_, LPE_)                            \
    hipError_t launch_special_step_##ID(const LaunchPlan &lp, const Io &io, hipStream_t s);                   \
    hipError_t launch_special_many_##ID(const LaunchPlan &lp, const Io &io, int T, int obs_mode, const ManyPolicy &pol, hipStream_t s);
MAPF_SPECIALIZATIONS(MAPF_DECLARE_SPECIAL)
#undef MAPF_DECLARE_SPECIAL
// runtime-config kernels: one unit per (lanes per env, window-mask width)
#define MAPF_DECLARE_RUNTIME(L, MW)                                                                           \
    hipError_t launch_runtime_##L##_##MW(int kind, const LaunchPlan &lp, const Io &io, hipStream_t s);        \
    hipError_t launch_runtime_many_##L##_##MW(const LaunchPlan &lp, const Io &io, int T, int obs_mode, const ManyPolicy &pol, hipStream_t s);
#define MAPF_DECLARE_RUNTIME_L(L) MAPF_FOR_MW(MAPF_DECLARE_RUNTIME, L)
MAPF_FOR_LPE(MAPF_DECLARE_RUNTIME_L)
#undef MAPF_DECLARE_RUNTIME_L
#undef MAPF_DECLARE_RUNTIME
// single-agent (CTE) kernels: one unit per lanes per env
#ifndef MAPF_NO_CTE_KERNELS
#define MAPF_DECLARE_CTE(L) hipError_t launch_cte_##L(const LaunchPlan &lp, const CteIo &io, bool step, hipStream_t s, CteMany many);
MAPF_FOR_LPE(MAPF_DECLARE_CTE)
#undef MAPF_DECLARE_CTE
#endif

// rgb_array frames (mapf_render.hip, its own launch unit).  A workgroup rasterises a band of rows_per_band cell rows of
// one frame; the host picks rows_per_band = ceil(kRenderBandPixels / (c * c * W)) (at most H), so a band holds at most
// 1024 + W - 1 < kRenderMaxBandCells cells and its five colours per cell fit the kernel's static LDS table.
#ifndef MAPF_RENDER_NT
#define MAPF_RENDER_NT 0  // 1: the frame stores carry the nontemporal hint (measured)
#endif
constexpr int kRenderThreads = 256;
constexpr int kRenderBandPixels = 16384;  // 48 KiB of output per workgroup when the cell rows allow it
constexpr int kRenderMaxBandCells = 1088;
struct RenderArgs {
    const Params *params;     // the handle's Params: error record (bad env id, MAPF_CHK)
    const uint2 *agents;      // plane 0 of the agent state
    const uint64_t *rows;     // [B][H] obstacle rows, bit col + col_pad
    const int32_t *env_ids;   // [K] or null (= 0 .. K-1)
    uint8_t *frames;          // [K][H*c][W*c][3]
    int B, H, W, N, col_pad;
    int sr;                   // sensor range; -1 on single-agent handles (no windows)
    int c, rows_per_band;
    int aligned;              // frames is 16-byte aligned: whole 16-pixel chunks leave as three 16-byte stores
};
hipError_t launch_render(const RenderArgs &ra, unsigned blocks, hipStream_t s);

// evaluation recorder (mapf_eval.hip, its own launch unit): one launch after every step of an evaluation.  Lanes are
// agents, lpe lanes own one env; the record layout is in include/mapf_step.h above mapf_eval_begin.
constexpr int kEvalThreads = 256;
struct EvalArgs {
    const Params *params;        // the handle's Params: error record (MAPF_CHK)
    const uint2 *agents;         // plane 0 of the agent state
    const float *rewards;        // [B][N] of the step just made
    const uint8_t *terminated;   // [B]
    const uint8_t *truncated;    // [B]
    const float *info_all;       // [B][14]
    uint8_t *active;             // [B] the mask the step was launched with; cleared after an env's E-th episode
    uint8_t *reset_mask;         // [B] out: 1 = the env ended an episode and runs another
    uint32_t *heat;              // [B][H][W]
    int32_t *ep_i32;             // [B][E][2 + 4N]
    double *ep_f64;              // [B][E][1 + N]
    float *ep_info;              // [B][E][14]
    int32_t *episodes_recorded;  // [B]
    double *run_reward;          // [B][N] reward of the running episode per agent (handle-owned)
    int32_t *run_steps;          // [B] steps of the running episode (handle-owned)
    int B, H, W, N, E, lpe;
};
hipError_t launch_eval_record(const EvalArgs &ea, hipStream_t s);

// the same for a single-agent handle (k_cte_eval_record, the same launch unit): one reward and one 4-float info row per env.
// Lanes are agents, G = the smallest power of two that holds N lanes own one env (the step kernels' group width is chosen
// for the observation row and would leave most lanes idle here); the record layout is above mapf_cte_eval_begin.
constexpr int cte_eval_group_width(int N) { return N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : N <= 16 ? 16 : N <= 32 ? 32 : 64; }
struct CteEvalArgs {
    const Params *params;        // the handle's Params: error record (MAPF_CHK)
    const uint2 *agents;         // plane 0 of the agent state
    const double *reward;        // [B] of the step just made
    const uint8_t *terminated;   // [B]
    const uint8_t *truncated;    // [B]
    const float *info;           // [B][4]
    uint8_t *active;             // [B] the mask the step was launched with; cleared after an env's E-th episode
    uint8_t *reset_mask;         // [B] out: 1 = the env ended an episode and runs another
    uint32_t *heat;              // [B][H][W]
    int32_t *ep_i32;             // [B][E][2 + 4N]
    double *ep_f64;              // [B][E]
    float *ep_info;              // [B][E][4]
    int32_t *episodes_recorded;  // [B]
    double *run_reward;          // [B] reward of the running episode, added up in step order (handle-owned)
    int32_t *run_steps;          // [B] steps of the running episode (handle-owned)
    int B, H, W, N, E, G;
};
hipError_t launch_cte_eval_record(const CteEvalArgs &ea, hipStream_t s);

// shortest-path planner (mapf_plan.hip, its own launch unit): G lanes of a wavefront own one search, lane r holds grid row
// r as a bit row.  The host picks G = plan_group_width(H); one struct serves the three kernels, each reads its own fields.
constexpr int kPlanThreads = 256;
constexpr int plan_group_width(int H) { return H <= 4 ? 4 : H <= 8 ? 8 : H <= 16 ? 16 : H <= 32 ? 32 : 64; }
struct PlanArgs {
    const Params *params;     // the handle's Params: error record (bad env id, MAPF_CHK site 15)
    const uint2 *agents;      // plane 0 of the agent state (expert actions)
    const uint64_t *rows;     // [B][H] obstacle rows, bit col + col_pad
    const int32_t *env_ids;   // [K] (path lengths, fields)
    const int16_t *src;       // [K][2] row, col (path lengths)
    const int16_t *dst;       // [K][2] row, col (path lengths, fields)
    int8_t *actions;          // [B][N] (expert actions)
    int32_t *dist;            // [B][N] or null (expert actions)
    int32_t *out;             // [K] (path lengths)
    uint16_t *field;          // [K][H][W] (fields)
    int B, H, W, N, col_pad;
    int K, G, mode;
};
hipError_t launch_plan_expert(const PlanArgs &pa, hipStream_t s);
hipError_t launch_plan_lengths(const PlanArgs &pa, hipStream_t s);
hipError_t launch_plan_field(const PlanArgs &pa, hipStream_t s);

// prioritised planner (the same launch unit): a group of G lanes owns one ENV and plans its agents one after another; a
// workgroup is one wavefront of epw <= 64 / G envs.  LDS: one 2-byte cell per planned agent and time step, T + 2 slots of
// NP = N rounded up to 4 cells per env; epw is the most envs whose slots fit kPrioMaxLds.  The reach sets of the agent
// being planned go to `hist`, the handle's workspace.
constexpr int kPrioThreads = 64;
constexpr int kPrioMaxLds = 64 * 1024;
constexpr int prio_lds_bytes(int epw, int T, int NP) { return epw * (T + 2) * NP * (int)sizeof(uint16_t); }
constexpr int prio_envs_per_workgroup(int G, int T, int NP) {
    return 64 / G < kPrioMaxLds / prio_lds_bytes(1, T, NP) ? 64 / G : kPrioMaxLds / prio_lds_bytes(1, T, NP);
}
struct PrioArgs {
    const Params *params;     // the handle's Params: error record (MAPF_CHK sites 16, 17)
    const uint2 *agents;      // plane 0 of the agent state
    const uint64_t *rows;     // [B][H] obstacle rows, bit col + col_pad
    const uint8_t *mask;      // [B] or null (= every env)
    int8_t *plan;             // [B][T][N]
    int32_t *arrival;         // [B][N]
    uint64_t *hist;           // [B][T + 1][G] workspace: row r of reach[t] of the agent being planned
    int B, H, W, N, col_pad;
    int G, T, NP, epw;
};
hipError_t launch_plan_prioritized(const PrioArgs &pa, hipStream_t s);

// windowed prioritised planner (the same launch unit, the same lane mapping): everything of an env lives in LDS -- the reach
// history of the agent being planned, (w + 1) x G 8-byte rows, then the cells of the planned agents, w + 2 slots of NP =
// N rounded up to 4 cells -- so the call has no workspace.  epw is the most envs whose regions fit kPrioMaxLds (>= 1: the
// largest region, w = G = N = 64, is 33 280 + 8 448 bytes).
// `rows`: the planned agents' cells as bit rows, (w + 1) x G more 8-byte rows and one slot of cells (the agents' cells now)
// instead of w + 2.  Taken (win_occ_rows) where it costs no env of the wavefront AND the whole launch stays resident on
// the device with the larger regions (kCuLdsBytes of LDS per compute unit); measured per shape and window in DESIGN.md 4j:
// bit rows win where the launch stays resident (0.59 of the cells' time at 1 024 x 64x64 x 64, window 16) and lose where
// it does not (1.27 at 8 192 x 32x32 x 8, window 16).
#ifndef MAPF_WIN_OCC_ROWS
#define MAPF_WIN_OCC_ROWS 2  // 0: cells everywhere, 1: bit rows wherever no env is lost (the A/B builds of DESIGN.md 4j)
#endif
constexpr int kCuLdsBytes = 160 * 1024;  // gfx950
constexpr int win_env_words(int G, int w, int NP, bool rows) {  // 8-byte words (NP % 4 == 0)
    return rows ? 2 * (w + 1) * G + NP / 4 : (w + 1) * G + (w + 2) * NP / 4;
}
constexpr int win_lds_bytes(int epw, int G, int w, int NP, bool rows) { return epw * win_env_words(G, w, NP, rows) * 8; }
constexpr int win_envs_per_workgroup(int G, int w, int NP, bool rows) {
    return 64 / G < kPrioMaxLds / win_lds_bytes(1, G, w, NP, rows) ? 64 / G : kPrioMaxLds / win_lds_bytes(1, G, w, NP, rows);
}
constexpr bool win_occ_rows(int G, int w, int NP, int B, int cus) {
    const int epw = win_envs_per_workgroup(G, w, NP, true);
    if (MAPF_WIN_OCC_ROWS == 0 || epw < 1 || epw < win_envs_per_workgroup(G, w, NP, false)) return false;
    if (MAPF_WIN_OCC_ROWS == 1) return true;
    const long long resident = (long long)cus * (kCuLdsBytes / win_lds_bytes(epw, G, w, NP, true));
    return (B + epw - 1) / epw <= resident;
}
struct WinArgs {
    const Params *params;     // the handle's Params: error record (MAPF_CHK sites 18 - 20)
    const uint2 *agents;      // plane 0 of the agent state
    const uint64_t *rows;     // [B][H] obstacle rows, bit col + col_pad
    const uint8_t *mask;      // [B] or null (= every env)
    int8_t *plan;             // [B][w][N]
    int32_t *arrival;         // [B][N]
    int32_t *remaining;       // [B][N]
    int B, H, W, N, col_pad;
    int G, w, NP, epw, occ_rows;
};
hipError_t launch_plan_windowed(const WinArgs &pa, hipStream_t s);

// conflict-based search (the same launch unit, the same lane mapping; mapf_plan.hip describes the tables).  A path is
// c_0 .. c_T and the arrival, 2 bytes each, rounded up to whole 8-byte words; an env's LDS region is the joint plan (N
// paths), 12 bytes per node (8 of parent / constraint / same-time ancestor, 4 of cost key) and 2 bytes per time step of
// constraint heads.  At the limits (N = 64, T = 128, M = 1 024) that is 16 896 + 12 288 + 264 = 29 448 bytes: every env
// fits kPrioMaxLds; epw is the most envs of a wavefront that fit together.
constexpr int cbs_path_cells(int T) { return (T + 2 + 3) & ~3; }
constexpr int cbs_record_bytes(int T) { return 16 + 2 * cbs_path_cells(T); }
constexpr int cbs_env_words(int N, int T, int M) {  // 8-byte words
    return N * cbs_path_cells(T) / 4 + ((M + 1) & ~1) + ((M + 1) & ~1) / 2 + ((T + 4) & ~3) / 4;
}
constexpr int cbs_lds_bytes(int epw, int N, int T, int M) { return epw * cbs_env_words(N, T, M) * 8; }
constexpr int cbs_envs_per_workgroup(int G, int N, int T, int M) {
    return 64 / G < kPrioMaxLds / cbs_lds_bytes(1, N, T, M) ? 64 / G : kPrioMaxLds / cbs_lds_bytes(1, N, T, M);
}
constexpr size_t cbs_env_workspace_bytes(int G, int N, int T, int M) {  // reach history, root paths, records
    return (size_t)(T + 1) * G * 8 + (size_t)N * cbs_path_cells(T) * 2 + (size_t)M * cbs_record_bytes(T);
}
struct CbsArgs {
    const Params *params;     // the handle's Params: error record (MAPF_CHK sites 21 - 23)
    const uint2 *agents;      // plane 0 of the agent state
    const uint64_t *rows;     // [B][H] obstacle rows, bit col + col_pad
    const uint8_t *mask;      // [B] or null (= every env)
    int8_t *plan;             // [B][T][N]
    int32_t *arrival;         // [B][N]
    int32_t *status;          // [B]
    int32_t *nodes;           // [B]
    uint64_t *hist;           // [B][T + 1][G] workspace: row r of reach[t] of the agent being planned
    uint16_t *root;           // [B][N][TP] workspace: the unconstrained paths
    uint8_t *recs;            // [B][M] records of cbs_record_bytes(T)
    int B, H, W, N, col_pad;
    int G, T, M, epw;
};
hipError_t launch_plan_cbs(const CbsArgs &pa, hipStream_t s);

// Status of the launch just made. hipGetLastError() also returns (and clears) an error some earlier, unrelated call
// left on this thread (torch, RCCL, an event query), so stale state is dropped right before the launch and only what
// the launch itself raised is reported.
#define LAUNCH_CHECKED(...)                          \
    do {                                             \
        (void)hipGetLastError();                     \
        hipLaunchKernelGGL(__VA_ARGS__);             \
        return hipGetLastError();                    \
    } while (0)

// the step kernels take the head of Io as individual (preloadable) arguments
#define IO_HEAD_ARGS(io) (io).agents, (io).scal, (io).grid_rows, (io).actions, (io).B, (io).H, (io).W, (io).bn8, \
                         static_cast<const IoTail &>(io)

}  // namespace mapfk

#endif  // MAPF_ENGINE_H
