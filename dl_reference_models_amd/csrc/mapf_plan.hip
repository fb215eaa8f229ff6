// mapf_plan.hip -- the planners of libmapfstep.so: the shortest-path planner (mapf_expert_actions, mapf_path_lengths,
// mapf_distance_field, and mapf_observe_guided: the expert's search as six floats of an observation row), the prioritised
// planner (mapf_plan_prioritized), its windowed form (mapf_plan_windowed) and conflict-based search (mapf_plan_cbs, the last kernel); include/mapf_step.h states their rules.  Kernels, launches and,
// at the end of the file, their part of the C ABI.
//
// A search is a breadth-first flood on the env's obstacle bit rows.  A GROUP of G lanes (the power of two >= H, at least
// 4, inside one wavefront) owns one search and lane r of the group holds grid row r as one 64-bit word, bit col + col_pad:
//     reach' = (reach | reach << 1 | reach >> 1 | row above | row below) & free
// The rows above and below arrive from the neighbouring lanes by a cross-lane move (DPP wave shift), never through memory; the bits the
// engine sets outside the grid (below col_pad, from W + col_pad up) read as obstacle, so a shift never leaks across the
// grid's edge, and rows r >= H hold free = 0.  The flood starts on the DESTINATION and stops when it reaches the source
// (k expansions = distance k), or when a ballot over the group says that it stopped growing (unreachable: -1).  The set
// before the last expansion is kept: it holds every cell nearer than D to the destination, so the neighbours of the
// source that lie in it are exactly the cells at distance D - 1 -- the expert's moves -- without a second search.
// Groups of one wave that finish early idle until the last one is done: no lane leaves before a cross-lane operation.
//
// The kernels read plane 0 of the agent state and the obstacle rows and write the caller's outputs, plus the error
// record for a bad env id (and the prioritised planner its workspace).  Nothing the step kernels read is touched, no
// generator is used.
//
// Stated once for all kernels: Agent, the state word taken apart; and for the three joint planners EnvFrame
// (which env a group owns), fill_now, flood_to_goal (prioritised and CBS; the windowed flood has no goal to stop at),
// walk_back (the tie-break of include/mapf_step.h: each kernel passes what one step emits), and on the host
// envs_per_workgroup, launch_per_env and the entry points' common openings (plan_refuses, shortest_path_entry, joint_entry).

#include "mapf_handle.h"

namespace mapfk {

namespace {

// shortest-path planner: G lanes of a wavefront own one search, lane r holds grid row
// r as a bit row.  The host picks G = plan_group_width(H); one struct serves the three kernels, each reads its own fields.
constexpr int kPlanThreads = 256;
constexpr int plan_group_width(int H) { return H <= 4 ? 4 : H <= 8 ? 8 : H <= 16 ? 16 : H <= 32 ? 32 : 64; }
struct PlanArgs : EnvView {
    const int32_t *env_ids;   // [K] (path lengths, fields)
    const int16_t *src;       // [K][2] row, col (path lengths)
    const int16_t *dst;       // [K][2] row, col (path lengths, fields)
    int8_t *actions;          // [B][N] (expert actions)
    int32_t *dist;            // [B][N] or null (expert actions)
    int32_t *out;             // [K] (path lengths)
    uint16_t *field;          // [K][H][W] (fields)
    int K, G, mode;
};

// prioritised planner (the same lane mapping): a group of G lanes owns one ENV and plans its agents one after another; a
// workgroup is one wavefront of epw <= 64 / G envs.  LDS: one 2-byte cell per planned agent and time step, T + 2 slots of
// NP = N rounded up to 4 cells per env; epw is the most envs whose slots fit kPrioMaxLds.  The reach sets of the agent
// being planned go to `hist`, the handle's workspace.
constexpr int kPrioThreads = 64;
constexpr int kPrioMaxLds = 64 * 1024;
constexpr int prio_lds_bytes(int epw, int T, int NP) { return epw * (T + 2) * NP * (int)sizeof(uint16_t); }
// the envs of one workgroup of a joint planner: as many groups as a wavefront holds, and no more than fit its LDS
constexpr int envs_per_workgroup(int G, int bytes_of_one_env) {
    return 64 / G < kPrioMaxLds / bytes_of_one_env ? 64 / G : kPrioMaxLds / bytes_of_one_env;
}
// what the three joint planners take alike (their structs go on from here, each in its own order)
struct JointArgs : EnvView {
    const uint8_t *mask;      // [B] or null (= every env)
    int8_t *plan;             // [B][steps][N]
    int32_t *arrival;         // [B][N]
};
struct PrioArgs : JointArgs {  // plan [B][T][N]
    uint64_t *hist;           // [B][T + 1][G] workspace: row r of reach[t] of the agent being planned
    int G, T, NP, epw;
};

// windowed prioritised planner (the same lane mapping): everything of an env lives in LDS -- the reach
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
    return envs_per_workgroup(G, win_lds_bytes(1, G, w, NP, rows));
}
constexpr bool win_occ_rows(int G, int w, int NP, int B, int cus) {
    const int epw = win_envs_per_workgroup(G, w, NP, true);
    if (MAPF_WIN_OCC_ROWS == 0 || epw < 1 || epw < win_envs_per_workgroup(G, w, NP, false)) return false;
    if (MAPF_WIN_OCC_ROWS == 1) return true;
    const long long resident = (long long)cus * (kCuLdsBytes / win_lds_bytes(epw, G, w, NP, true));
    return (B + epw - 1) / epw <= resident;
}
struct WinArgs : JointArgs {  // plan [B][w][N]
    int32_t *remaining;       // [B][N]
    int G, w, NP, epw, occ_rows;
};

// conflict-based search (the same lane mapping; the tables are described above k_plan_cbs).  A path is
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
constexpr int cbs_envs_per_workgroup(int G, int N, int T, int M) { return envs_per_workgroup(G, cbs_lds_bytes(1, N, T, M)); }
constexpr size_t cbs_env_workspace_bytes(int G, int N, int T, int M) {  // reach history, root paths, records
    return (size_t)(T + 1) * G * 8 + (size_t)N * cbs_path_cells(T) * 2 + (size_t)M * cbs_record_bytes(T);
}
struct CbsArgs : JointArgs {  // plan [B][T][N]
    int32_t *status;          // [B]
    int32_t *nodes;           // [B]
    uint64_t *hist;           // [B][T + 1][G] workspace: row r of reach[t] of the agent being planned
    uint16_t *root;           // [B][N][TP] workspace: the unconstrained paths
    uint8_t *recs;            // [B][M] records of cbs_record_bytes(T)
    int G, T, M, epw;
};

#ifndef MAPF_PLAN_DPP
#define MAPF_PLAN_DPP 1  // the neighbouring rows move by DPP wave shifts; 0: by __shfl (ds_bpermute), 10 % slower
#endif

// the value lane - 1 / lane + 1 of the wavefront holds (what the wave's first / last lane gets is never used: the caller
// masks the group's first / last row)
__device__ __forceinline__ uint64_t from_lane_below(uint64_t v) {
#if MAPF_PLAN_DPP
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138 /* wave_shr:1 */, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xF, 0xF, true);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
#else
    return __shfl_up((unsigned long long)v, 1);
#endif
}
__device__ __forceinline__ uint64_t from_lane_above(uint64_t v) {
#if MAPF_PLAN_DPP
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x130 /* wave_shl:1 */, 0xF, 0xF, true);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x130, 0xF, 0xF, true);
    return ((uint64_t)(uint32_t)hi << 32) | (uint32_t)lo;
#else
    return __shfl_down((unsigned long long)v, 1);
#endif
}

// where a lane sits: r = its row in the group, base = the group's first lane in the wavefront, gmask = G ones
struct Group {
    int r, base, G;
    uint64_t gmask;
    __device__ __forceinline__ explicit Group(int G_) : G(G_) {
        const int lane = (int)(threadIdx.x & 63u);
        r = lane & (G - 1);
        base = lane - r;
        gmask = G >= 64 ? ~0ull : ((1ull << G) - 1ull);
    }
    // the group's part of a wave-wide ballot, bit i = lane base + i
    __device__ __forceinline__ uint64_t ballot(bool p) const { return (__ballot(p) >> base) & gmask; }
    __device__ __forceinline__ bool any(bool p) const { return ballot(p) != 0ull; }
};

// one expansion of `reach` inside `free`
__device__ __forceinline__ uint64_t expand(const Group &g, uint64_t reach, uint64_t free) {
    uint64_t up = from_lane_below(reach), dn = from_lane_above(reach);
    up = g.r == 0 ? 0ull : up;
    dn = g.r == g.G - 1 ? 0ull : dn;
    return (reach | (reach << 1) | (reach >> 1) | up | dn) & free;
}

struct Found {
    int D;          // distance source -> destination, -1: none
    uint64_t prev;  // this lane's row of the set before the last expansion: the cells nearer than D to the destination
};

// The search of one group: `ok` (group-uniform) says that the query is valid (env in range, both cells inside the grid);
// (sr, sbit) / (dr, dbit) are the row and the bit index (col + col_pad) of source and destination.  Every lane of the
// wavefront calls this, whatever `ok` says.
__device__ __forceinline__ Found search(const Group &g, uint64_t free, bool ok, int sr, int sbit, int dr, int dbit, int HW) {
    uint64_t reach = (ok && g.r == dr) ? ((1ull << dbit) & free) : 0ull, prev = 0ull;
    const bool src_lane = ok && g.r == sr;
    // a source on an obstacle is never reached: do not flood for it
    // (every ballot is made by every lane: none sits behind a short-circuit)
    const bool seeded = g.any(reach != 0ull), src_free = g.any(src_lane && ((free >> sbit) & 1ull));
    const bool there = g.any(src_lane && ((reach >> sbit) & 1ull));
    bool active = seeded && src_free;
    int k = 0, D = -1;
    if (active && there) {
        D = 0;
        active = false;
    }
    // every expansion that keeps a group active adds a cell to its set, so HW bounds the loop whatever the rows hold
    for (int it = 0; it < HW && __ballot(active) != 0ull; it++) {
        const uint64_t nr = expand(g, reach, free);
        const bool grew = g.any(active && nr != reach);
        if (active && grew) {
            prev = reach;
            reach = nr;
            k++;
        } else {
            active = false;
        }
        const bool hit = g.any(active && src_lane && ((reach >> sbit) & 1ull));
        if (active && hit) {
            D = k;
            active = false;
        }
    }
    return {D, prev};
}

__device__ __forceinline__ uint64_t load_free(const uint64_t *rows, int H, const Group &g, bool env_ok, int env) {
    return (env_ok && g.r < H) ? ~rows[(size_t)env * H + g.r] : 0ull;
}
__device__ __forceinline__ uint64_t load_free(const PlanArgs &pa, const Group &g, bool env_ok, int env) {
    return load_free(pa.rows, pa.H, g, env_ok, env);
}

__device__ __forceinline__ bool in_grid(const EnvView &v, int r, int c) {
    return (unsigned)r < (unsigned)v.H && (unsigned)c < (unsigned)v.W;
}

// An agent's state word taken apart: where it stands (pr, pc), its goal (gr, gc), whether each lies inside the grid (false
// for an agent that is `off`: outside the batch, the mask or the env), and the bit index col + col_pad of each in a bit
// row, 0 where the cell is outside (W + col_pad <= 64: a shift by it is defined either way).
struct Agent {
    uint32_t w;
    int pr, pc, gr, gc, pbit, gbit;
    bool p_in, g_in;
    __device__ __forceinline__ Agent(const EnvView &v, bool on, uint32_t word) : w(on ? word : 0u) {
        pr = (int)((w >> 8) & 255u), pc = (int)(w & 255u), gr = (int)(w >> 24), gc = (int)((w >> 16) & 255u);
        p_in = on && in_grid(v, pr, pc);
        g_in = on && in_grid(v, gr, gc);
        pbit = p_in ? pc + v.col_pad : 0;
        gbit = g_in ? gc + v.col_pad : 0;
    }
    __device__ __forceinline__ bool valid() const { return p_in && g_in; }
    __device__ __forceinline__ uint32_t cell() const { return w & 0xFFFFu; }  // row << 8 | col, as the planners store it
    __device__ __forceinline__ uint32_t goal_cell() const { return w >> 16; }
};
// agent j of env `env`; nothing is read for one that is off
__device__ __forceinline__ Agent load_agent(const EnvView &v, bool on, int env, int j) {
    return Agent(v, on, on ? v.agents[(size_t)env * v.N + j].x : 0u);
}

// The moves that shorten the path, bit a = action a: 1 UP (row - 1), 2 RIGHT (col + 1), 3 DOWN (row + 1), 4 LEFT (col - 1),
// for a source at (row pr, bit sbit) whose search gave `f`; the rows next to the source's come out of a ballot over the
// group.  Every lane of the wavefront calls this.
__device__ __forceinline__ uint32_t shortening_moves(const Group &g, const Found &f, int pr, int sbit) {
    const uint64_t col_bits = g.ballot((f.prev >> sbit) & 1ull);
    const uint64_t right = g.ballot(g.r == pr && sbit + 1 < 64 && ((f.prev >> (sbit + 1)) & 1ull));
    const uint64_t left = g.ballot(g.r == pr && sbit >= 1 && ((f.prev >> (sbit - 1)) & 1ull));
    uint32_t cand = 0;
    if (f.D > 0) {
        if (pr >= 1 && ((col_bits >> (pr - 1)) & 1ull)) cand |= 1u << 1;
        if (right) cand |= 1u << 2;
        if (pr + 1 < g.G && ((col_bits >> (pr + 1)) & 1ull)) cand |= 1u << 3;
        if (left) cand |= 1u << 4;
    }
    return cand;
}

// ---- expert actions: search s = env * N + agent, source = the agent's cell, destination = its goal ------------------
// (the mode is a template parameter: two kernel names in a trace, no occupancy loop in the independent one)
template <bool YIELD>
__global__ __launch_bounds__(kPlanThreads) void k_plan_expert(PlanArgs pa) {
    const Group g(pa.G);
    const int N = pa.N;
    const size_t s = ((size_t)blockIdx.x * kPlanThreads + threadIdx.x) / (unsigned)pa.G;
    const bool ok = s < (size_t)pa.B * N;
    const int env = ok ? (int)(s / (unsigned)N) : 0;
    const Agent ag(pa, ok, ok ? pa.agents[s].x : 0u);
    const int pr = ag.pr, sbit = ag.pbit;
    const uint64_t free = load_free(pa, g, ok, env);
    const Found f = search(g, free, ag.valid(), pr, sbit, ag.gr, ag.gbit, pa.H * pa.W);

    uint32_t cand = shortening_moves(g, f, pr, sbit);
    if constexpr (YIELD) {
        // cells other agents of the env stand on (no agent stands on a neighbour of its own cell and on its own cell)
        const uint32_t cell = ag.cell();
        const uint32_t tgt[4] = {cell - 0x100u, cell + 1u, cell + 0x100u, cell - 1u};
        uint32_t mine = 0;
        for (int j0 = 0; j0 < N; j0 += pa.G) {  // (uniform trip count)
            const int j = j0 + g.r;
            if (ok && j < N) {
                const uint32_t o = pa.agents[(size_t)env * N + j].x & 0xFFFFu;
#pragma unroll
                for (int u = 0; u < 4; u++) mine |= (o == tgt[u]) ? (2u << u) : 0u;
            }
        }
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const bool taken = g.any((mine >> (u + 1)) & 1u);
            cand &= taken ? ~(2u << u) : ~0u;
        }
    }
    if (ok && g.r == 0) {
        pa.actions[s] = (int8_t)(cand ? __ffs((int)cand) - 1 : 0);
        if (pa.dist) pa.dist[s] = f.D;
    }
}

// ---- guided observations (mapf_observe_guided; include/mapf_step.h states the rule): the expert's search, then the G lanes
// of the group share the agent's output row -- the observation words around the six guidance floats, 4-byte words moved as
// they are -- lane i of the row taking words i, i + G, ...
struct GuidedArgs : EnvView {
    const uint32_t *obs;  // [B][N][L] or null
    uint32_t *out;        // [B][N][L + 6]; null obs: [B][N][6]
    int G, L, tail;       // L = 0 with a null obs
};

__global__ __launch_bounds__(kPlanThreads) void k_plan_guided(GuidedArgs pa) {
    const Group g(pa.G);
    const size_t s = ((size_t)blockIdx.x * kPlanThreads + threadIdx.x) / (unsigned)pa.G;
    const bool ok = s < (size_t)pa.B * pa.N;
    const int env = ok ? (int)(s / (unsigned)pa.N) : 0;
    const Agent ag(pa, ok, ok ? pa.agents[s].x : 0u);
    const uint64_t free = load_free(pa.rows, pa.H, g, ok, env);
    const Found f = search(g, free, ag.valid(), ag.pr, ag.pbit, ag.gr, ag.gbit, pa.H * pa.W);
    const uint32_t cand = shortening_moves(g, f, ag.pr, ag.pbit);
    if (!ok) return;  // (behind the last cross-lane operation)

    const int L = pa.L, head = L - pa.tail;
    uint32_t *o = pa.out + s * (size_t)(L + MAPF_GUIDANCE_LEN);
    const uint32_t *in = pa.obs + s * (size_t)L;  // (not read when L == 0)
    for (int i = g.r; i < L; i += pa.G) o[i < head ? i : i + MAPF_GUIDANCE_LEN] = in[i];
    const float far = f.D < 0 ? -1.0f : (float)f.D / (float)(pa.H * pa.W);  // (no fast-math: the correctly rounded quotient)
    for (int a = g.r; a < MAPF_GUIDANCE_LEN; a += pa.G) {
        const bool set = a == 0 ? f.D == 0 : ((cand >> a) & 1u) != 0u;
        o[head + a] = a == MAPF_GUIDANCE_LEN - 1 ? __float_as_uint(far) : set ? 0x3F800000u /* 1.0f */ : 0u;
    }
}

// ---- K independent queries ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPlanThreads) void k_plan_lengths(PlanArgs pa) {
    const Params &P = *pa.params;
    const Group g(pa.G);
    const size_t k = ((size_t)blockIdx.x * kPlanThreads + threadIdx.x) / (unsigned)pa.G;
    const bool in_k = k < (size_t)pa.K;
    const int env = in_k ? pa.env_ids[k] : 0;
    const bool ok = in_k && (unsigned)env < (unsigned)pa.B;
    if (in_k && !ok && g.r == 0) raise_error(P, MAPF_ERR_CONFIG, (int)k, 0, env);
    int sr = 0, sc = 0, dr = 0, dc = 0;
    if (ok) {
        sr = pa.src[2 * k];
        sc = pa.src[2 * k + 1];
        dr = pa.dst[2 * k];
        dc = pa.dst[2 * k + 1];
    }
    const bool valid = ok && in_grid(pa, sr, sc) && in_grid(pa, dr, dc);
    const uint64_t free = load_free(pa, g, ok, env);
    const Found f = search(g, free, valid, sr, valid ? sc + pa.col_pad : 0, dr, valid ? dc + pa.col_pad : 0, pa.H * pa.W);
    if (ok && g.r == 0) pa.out[k] = f.D;
}

// ---- distance fields: the flood runs until it stops growing; every expansion writes its number into the cells it
// reached first, in an LDS image of the field (lane r walks the set bits of its own row's new frontier), and the block
// then stores its images -- consecutive fields of the output -- as one contiguous stream
__global__ __launch_bounds__(kPlanThreads) void k_plan_field(PlanArgs pa) {
    extern __shared__ uint16_t s_img[];  // [groups per block][H * W]
    __shared__ uint8_t s_ok[kPlanThreads / 4];
    const Params &P = *pa.params;
    const Group g(pa.G);
    const int H = pa.H, W = pa.W, HW = H * W, pad = pa.col_pad;
    const int grp = (int)threadIdx.x / pa.G, groups = kPlanThreads / pa.G;
    const size_t k0 = (size_t)blockIdx.x * groups, k = k0 + grp;
    const bool in_k = k < (size_t)pa.K;
    const int env = in_k ? pa.env_ids[k] : 0;
    const bool ok = in_k && (unsigned)env < (unsigned)pa.B;
    if (in_k && !ok && g.r == 0) raise_error(P, MAPF_ERR_CONFIG, (int)k, 0, env);
    if (g.r == 0) s_ok[grp] = ok ? 1 : 0;
    uint16_t *img = s_img + (size_t)grp * HW;
    for (int i = g.r; i < HW; i += pa.G) img[i] = 0xFFFFu;
    __syncthreads();

    int dr = 0, dc = 0;
    if (ok) {
        dr = pa.dst[2 * k];
        dc = pa.dst[2 * k + 1];
    }
    const bool valid = ok && in_grid(pa, dr, dc);
    const uint64_t free = load_free(pa, g, ok, env);
    uint64_t reach = 0ull, fresh = (valid && g.r == dr) ? ((1ull << (dc + pad)) & free) : 0ull;
    bool active = g.any(fresh != 0ull);
    // (the same bound as in search(): an expansion that keeps the group active reaches at least one new cell)
    for (int d = 0; d <= HW && __ballot(active) != 0ull; d++) {
        for (uint64_t m = active ? fresh : 0ull; m != 0ull; m &= m - 1ull) {
            const int c = __ffsll((unsigned long long)m) - 1 - pad;
            MAPF_CHK(P, g.r < H && (unsigned)c < (unsigned)W, 15, env, c);
            if (g.r < H && (unsigned)c < (unsigned)W) img[g.r * W + c] = (uint16_t)d;
        }
        reach |= fresh;
        const uint64_t nr = expand(g, reach, free);
        fresh = nr & ~reach;
        const bool more = g.any(fresh != 0ull);
        active = active && more;
    }
    __syncthreads();
    for (int q = 0; q < groups && k0 + q < (size_t)pa.K; q++) {
        if (!s_ok[q]) continue;  // a bad env id: the row is not written
        uint16_t *o = pa.field + (k0 + q) * (size_t)HW;
        for (int i = (int)threadIdx.x; i < HW; i += kPlanThreads) o[i] = s_img[(size_t)q * HW + i];
    }
}

// ---- prioritised planning (mapf_plan_prioritized; include/mapf_step.h states the rule) ---------------------------------
// One group owns one ENV and plans its N agents one after another, in index order.  What the agents planned so far occupy
// is kept in LDS as one 2-byte cell (row << 8 | col, 0xFFFF: none) per agent and time step -- slot t of the env holds
// c_t of agents 0 .. j - 1 -- and is turned into this lane's row mask when the flood needs it; slot T + 1 holds the
// agents' cells now.  The sets reach[0 .. A] of the agent being planned go to the handle's workspace, lane r writes and
// later reads its own row, so the walk back needs no fence.  A workgroup is one wavefront: its barriers order the LDS
// writes of one agent's walk before the next agent's reads, and every loop bound is uniform over the wavefront.
constexpr uint32_t kNoCell = 0xFFFFu;

// this lane's row of the cells slot[0 .. n) (n rounded up to a whole pack of four: the rest of a pack holds kNoCell or,
// with `after` >= 0, is skipped up to and including agent `after`)
__device__ __forceinline__ uint64_t row_mask(const Params &P, const uint16_t *slot, int n, int after, int r, int pad, int env,
                                             int lds_left) {
    uint64_t m = 0ull;
    for (int k0 = after >= 0 ? ((after + 1) & ~3) : 0; k0 < n; k0 += 4) {
        MAPF_CHK(P, k0 + 4 <= lds_left, 16, env, k0);
        const uint64_t q = *reinterpret_cast<const uint64_t *>(slot + k0);
#pragma unroll
        for (int u = 0; u < 4; u++) {
            const uint32_t cell = (uint32_t)(q >> (16 * u)) & 0xFFFFu;
            const bool mine = (int)(cell >> 8) == r && k0 + u > after;
            m |= mine ? 1ull << (((cell & 255u) + pad) & 63u) : 0ull;  // (a stored cell lies inside the grid: col + col_pad <= 63)
        }
    }
    return m;
}

// ---- what the three joint planners share ------------------------------------------------------------------------------
// Where a group sits in a launch of one group per env: grp = its number in the workgroup (slot() = its LDS region), env =
// the env it owns (0 where it owns none), ok = it owns one and the mask selects it.  G and epw are passed because the three
// argument structs keep them at different places.
struct EnvFrame {
    int grp, epw, env;
    bool ok;
    __device__ __forceinline__ EnvFrame(const JointArgs &pa, int G, int epw_) : grp((int)threadIdx.x / G), epw(epw_) {
        const int env_raw = (int)blockIdx.x * epw + grp;
        const bool in_b = grp < epw && env_raw < pa.B;
        env = in_b ? env_raw : 0;
        ok = in_b && (!pa.mask || pa.mask[env] != 0);
    }
    __device__ __forceinline__ int slot() const { return grp < epw ? grp : 0; }  // (only `ok` groups write theirs)
    // no env of this wavefront is selected: every lane may leave (a workgroup is one wavefront)
    __device__ __forceinline__ bool none_selected() const { return __ballot(ok) == 0ull; }
};

// now[0 .. NP) = the cells the env's agents stand on, kNoCell for one outside the grid and for the padding behind agent N - 1
__device__ __forceinline__ void fill_now(const EnvView &v, const Group &g, int env, int NP, uint16_t *now) {
    for (int k = g.r; k < NP; k += g.G) {
        const Agent a = load_agent(v, k < v.N, env, k);
        now[k] = (uint16_t)(a.p_in ? a.cell() : kNoCell);
    }
}

// The flood in space-time that stops at the goal: reach[0] = the agent's cell, reach[t] = expand(reach[t - 1]) & free &
// ~blocked[t], every set stored as hist[t * G] (`hist` is this lane's column of the history; reach[0] is stored by every
// lane that is `on`).  Returns the arrival A: the first t > last at which the set holds the goal, 0 for an agent that stands
// on a goal nothing holds later (last < 0), -1 where the goal is held through T (last >= T), the set runs empty or T
// passes.  blocked_at(t, active) gives this lane's row of what is blocked at time t and is called once for t = 0, 1, ... in
// order; its value at t = 0 is not used (nothing moves before time 1): a callable that reads a step ahead starts there.
template <typename Blocked>
__device__ __forceinline__ int flood_to_goal(const Group &g, uint64_t *hist, uint64_t free, const Agent &a, bool on, int last, int T,
                                             Blocked blocked_at) {
    const bool valid = a.valid();
    uint64_t reach = (valid && g.r == a.pr) ? 1ull << a.pbit : 0ull;
    if (on) hist[0] = reach;
    int A = -1;
    bool active = valid && last < T;  // (the goal is held through time T: no arrival, and no flood for it)
    if (active && last < 0 && a.pr == a.gr && a.pc == a.gc) {
        A = 0;
        active = false;
    }
    (void)blocked_at(0, active);
    for (int t = 1; t <= T && __ballot(active) != 0ull; t++) {
        const uint64_t blocked = blocked_at(t, active);
        const uint64_t nr = expand(g, reach, free & ~blocked);
        if (active) {
            reach = nr;
            hist[(size_t)t * g.G] = nr;
        }
        const bool hit = g.any(active && g.r == a.gr && ((reach >> a.gbit) & 1ull));
        const bool some = g.any(active && reach != 0ull);
        if (active && hit && t > last) {
            A = t;
            active = false;
        } else if (active && !some) {
            active = false;
        }
    }
    return A;
}

// The walk back from the end cell (row cr, bit cb) at time t through the stored sets (include/mapf_step.h: the lowest
// action id whose source cell is in reach[t - 1]): while t > 0 the cell moves against that action and every walking lane
// calls step(t - 1, a, cr, cb) -- action a at step t - 1 leaves the cell (cr, cb) of time t - 1.  `hist` is this lane's
// column of the history, n_hist words long from the group's first lane; `walking` is group-uniform, every lane of the
// wavefront calls this.  site_hist / site_walk: the caller's MAPF_CHK sites for a read outside the history and for a cell
// that no action reaches.
template <typename Step>
__device__ __forceinline__ void walk_back(const Params &P, const Group &g, const uint64_t *hist, int n_hist, int cr, int cb, int t,
                                          bool walking, int site_hist, int site_walk, int env, Step step) {
    const int G = g.G, r = g.r;
    uint64_t wcur = walking ? hist[(size_t)(t - 1) * G] : 0ull;
    while (__ballot(walking) != 0ull) {
        MAPF_CHK(P, !walking || t < 2 || (t - 2) * G + r < n_hist, site_hist, env, t);
        const uint64_t wnext = (walking && t >= 2) ? hist[(size_t)(t - 2) * G] : 0ull;
        const uint64_t col = g.ballot(walking && ((wcur >> cb) & 1ull));
        const bool before = g.any(walking && r == cr && cb >= 1 && ((wcur >> (cb >= 1 ? cb - 1 : 0)) & 1ull));
        const bool after = g.any(walking && r == cr && cb + 1 < 64 && ((wcur >> (cb + 1 < 64 ? cb + 1 : 0)) & 1ull));
        if (walking) {
            const bool stay = (col >> cr) & 1ull;
            const bool below = cr + 1 < G && ((col >> (cr + 1 < G ? cr + 1 : 0)) & 1ull);
            const bool above = cr >= 1 && ((col >> (cr >= 1 ? cr - 1 : 0)) & 1ull);
            const int a = stay ? 0 : below ? 1 : before ? 2 : above ? 3 : after ? 4 : -1;
            MAPF_CHK(P, a >= 0, site_walk, env, t);
            cr += a == 1 ? 1 : a == 3 ? -1 : 0;
            cb += a == 2 ? -1 : a == 4 ? 1 : 0;
            step(t - 1, a, cr, cb);
            t--;
            walking = t > 0;
        }
        wcur = wnext;
    }
}

__global__ __launch_bounds__(kPrioThreads) void k_plan_prioritized(PrioArgs pa) {
    extern __shared__ __attribute__((aligned(8))) uint16_t s_cells[];  // [envs per workgroup][T + 2][NP], read in packs of four
    const Params &P = *pa.params;
    const Group g(pa.G);
    const int N = pa.N, NP = pa.NP, T = pa.T, pad = pa.col_pad, r = g.r;
    const EnvFrame f(pa, pa.G, pa.epw);  // (no early return here: DESIGN.md 4w)
    const int env = f.env;
    const bool ok = f.ok;
    const int per_env = (T + 2) * NP;  // cells of an env's LDS region
    uint16_t *cells = s_cells + (size_t)f.slot() * per_env;
    uint16_t *now = cells + (size_t)(T + 1) * NP;
    uint64_t *hist = pa.hist + (size_t)env * (T + 1) * pa.G + r;  // + t * G
    const uint64_t free = load_free(pa.rows, pa.H, g, ok, env);

    if (ok) {
        for (int i = r; i < (T + 1) * NP; i += pa.G) cells[i] = (uint16_t)kNoCell;
        fill_now(pa, g, env, NP, now);
    }
    __syncthreads();

    for (int j = 0; j < N; j++) {
        const Agent ag = load_agent(pa, ok, env, j);
        const bool valid = ag.valid();
        const int gr = ag.gr, gbit = ag.gbit;
        const uint32_t gcell = ag.goal_cell();
        const int packs = (j + 3) & ~3;  // agents 0 .. j - 1 in whole packs of four

        // the agents after j have not moved when j makes its first move: their cells are blocked at time 1
        const uint64_t later = ok ? row_mask(P, now, NP, j, r, pad, env, NP) : 0ull;
        // the last time an earlier plan holds the goal (the lanes share the time steps)
        int last = -1;
        if (valid) {
            for (int t = r; t <= T; t += pa.G) {
                for (int k0 = 0; k0 < packs; k0 += 4) {
                    MAPF_CHK(P, t * NP + k0 + 4 <= per_env, 16, env, t);
                    const uint64_t q = *reinterpret_cast<const uint64_t *>(cells + (size_t)t * NP + k0);
#pragma unroll
                    for (int u = 0; u < 4; u++) last = ((uint32_t)(q >> (16 * u)) & 0xFFFFu) == gcell ? t : last;
                }
            }
        }
        for (int m = 1; m < pa.G; m <<= 1) last = max(last, __shfl_xor(last, m));
        const bool goal_later = g.any(valid && r == gr && ((later >> gbit) & 1ull));
        if (goal_later) last = max(last, 1);

        // the flood: blocked[t] = what the earlier plans hold at t and at t + 1 (no swap with them), the row of t + 1 read a
        // step ahead of its use, and at time 1 the agents after j
        uint64_t m_next = 0ull;
        const int A = flood_to_goal(g, hist, free, ag, ok, last, T, [&](int t, bool active) {
            const uint64_t m_now = m_next;
            const int tn = t + 1 <= T ? t + 1 : T;  // occ[T + 1] = occ[T]
            m_next = active ? row_mask(P, cells + (size_t)tn * NP, packs, -1, r, pad, env, per_env - tn * NP) : 0ull;
            return m_now | m_next | (t == 1 ? later : 0ull);
        });

        // outputs of the steps the agent stands still in, and where it stands from then on
        if (ok) {
            const uint16_t parked = (uint16_t)(A >= 0 ? gcell : (ag.p_in ? ag.cell() : kNoCell));
            const int from = A >= 0 ? A : 0;
            for (int t = from + r; t <= T; t += pa.G) {
                MAPF_CHK(P, t * NP + j < per_env - NP, 16, env, t);
                cells[(size_t)t * NP + j] = parked;
                if (t < T) pa.plan[((size_t)env * T + t) * N + j] = 0;
            }
            if (r == 0) pa.arrival[(size_t)env * N + j] = A;
        }

        // the walk back from the goal: the plan's actions, and the agent's cells for the agents after it
        walk_back(P, g, hist, (T + 1) * pa.G, gr, gbit, A, ok && A > 0, 16, 17, env, [&](int t, int a, int cr, int cb) {
            if (r == 0) {
                MAPF_CHK(P, t * NP + j < per_env - NP, 16, env, t + 1);
                pa.plan[((size_t)env * T + t) * N + j] = (int8_t)(a > 0 ? a : 0);
                cells[(size_t)t * NP + j] = (uint16_t)(cr << 8 | (cb - pad));
            }
        });
        __syncthreads();
    }
}

// ---- windowed prioritised planning (mapf_plan_windowed; include/mapf_step.h states the rule) ---------------------------
// The same lane mapping and the same cells as above, w steps deep, but nothing leaves the workgroup's LDS: an env's region
// is the reach history of the agent being planned, hist[t][r] = row r of reach[t] (t = 0 .. w; lane r writes and reads its
// own row), followed by slots 0 .. w of the planned agents' cells and slot w + 1, the agents' cells now.  The flood always
// runs w steps (or until the set is empty: the agent fails); there is no arrival to stop at.  The end cell is found
// without a distance field: a second flood from the goal on `free` alone meets reach[w] at level k exactly in the cells
// of reach[w] at distance k, the nearest ones; lowest row by ballot, lowest column by ffs of that lane's word.  A
// workgroup none of whose envs the mask selects leaves before the agent loop (one wavefront: every lane leaves).
// ROWS: where it costs no env of the wavefront (win_occ_rows) the planned agents' cells are kept as BIT ROWS instead,
// occ[t][r] = row r of occ[t] (t = 0 .. w), so the flood's mask of a time step is one LDS read of the lane's own word
// instead of a walk over the cells of agents 0 .. j - 1; only slot `now` of the cells is kept, for the time-1 mask.
template <bool ROWS>
__global__ __launch_bounds__(kPrioThreads) void k_plan_windowed(WinArgs pa) {
    extern __shared__ __attribute__((aligned(8))) uint64_t s_win[];  // [envs per workgroup][win_env_words]
    const Params &P = *pa.params;
    const Group g(pa.G);
    const int N = pa.N, NP = pa.NP, w = pa.w, pad = pa.col_pad, r = g.r, G = pa.G;
    const EnvFrame f(pa, G, pa.epw);
    const int env = f.env;
    const bool ok = f.ok;
    if (f.none_selected()) return;  // (before any barrier)

    uint64_t *region = s_win + (size_t)f.slot() * win_env_words(G, w, NP, ROWS);
    uint64_t *hist = region + r;  // + t * G
    const int n_hist = (w + 1) * G, n_cells = ROWS ? NP : (w + 2) * NP;
    uint64_t *occ = region + n_hist;  // ROWS: [w + 1][G]
    uint16_t *cells = reinterpret_cast<uint16_t *>(region + (size_t)n_hist * (ROWS ? 2 : 1));
    uint16_t *now = ROWS ? cells : cells + (size_t)(w + 1) * NP;
    const uint64_t free = load_free(pa.rows, pa.H, g, ok, env);
    const int HW = pa.H * pa.W;

    if (ok) {
        if constexpr (ROWS) {
            for (int t = 0; t <= w; t++) occ[(size_t)t * G + r] = 0ull;
        } else {
            for (int i = r; i < (w + 1) * NP; i += G) cells[i] = (uint16_t)kNoCell;
        }
        fill_now(pa, g, env, NP, now);
    }
    __syncthreads();

    for (int j = 0; j < N; j++) {
        const Agent ag = load_agent(pa, ok, env, j);
        const int pr = ag.pr, gr = ag.gr, pbit = ag.pbit, gbit = ag.gbit;
        const bool p_in = ag.p_in, g_in = ag.g_in;
        const int packs = (j + 3) & ~3;  // agents 0 .. j - 1 in whole packs of four

        // the agents after j have not moved when j makes its first move: their cells are blocked at time 1
        const uint64_t later = ok ? row_mask(P, now, NP, j, r, pad, env, NP) : 0ull;

        // the flood in space-time, w steps: reach[t] = expand(reach[t - 1]) & free & ~blocked[t]
        uint64_t reach = (p_in && r == pr) ? 1ull << pbit : 0ull;
        if (ok) hist[0] = reach;
        bool alive = p_in;  // (group-uniform; false from the first empty set on: the agent fails)
        const auto occ_row = [&](int t) -> uint64_t {  // this lane's row of occ[t], t = 1 .. w
            if constexpr (ROWS) {
                MAPF_CHK(P, t * G + r < n_hist, 19, env, t);
                return occ[(size_t)t * G + r];
            } else {
                MAPF_CHK(P, t * NP + packs <= n_cells - NP, 19, env, t);
                return row_mask(P, cells + (size_t)t * NP, packs, -1, r, pad, env, n_cells - t * NP);
            }
        };
        uint64_t m_next = alive ? occ_row(1) : 0ull;
        for (int t = 1; t <= w && __ballot(alive) != 0ull; t++) {
            const uint64_t m_now = m_next;
            const int tn = t + 1 <= w ? t + 1 : w;  // occ[w + 1] = occ[w]
            m_next = alive ? occ_row(tn) : 0ull;
            const uint64_t blocked = m_now | m_next | (t == 1 ? later : 0ull);
            const uint64_t nr = expand(g, reach, free & ~blocked);
            if (alive) {
                MAPF_CHK(P, t * G + r < n_hist, 18, env, t);
                reach = nr;
                hist[(size_t)t * G] = nr;
            }
            alive = g.any(alive && reach != 0ull);
        }

        // the flood from the goal on `free` alone, until it meets reach[w] (every expansion that keeps a group seeking adds
        // a cell to its set, so HW bounds the loop)
        uint64_t gv = (alive && g_in && r == gr) ? ((1ull << gbit) & free) : 0ull;
        bool seeking = alive;
        int D = -2, k = 0;
        for (int it = 0; it <= HW && __ballot(seeking) != 0ull; it++) {
            const bool meet = g.any(seeking && (gv & reach) != 0ull);
            if (seeking && meet) {
                D = k;
                seeking = false;
            }
            const uint64_t nv = expand(g, gv, free);
            const bool grew = g.any(seeking && nv != gv);
            if (seeking && grew) {
                gv = nv;
                k++;
            } else {
                seeking = false;
            }
        }
        // the end cell: the lowest (row, col) of the meeting cells, or of reach[w] when the goal is out of reach
        const uint64_t cand = alive ? (D >= 0 ? (gv & reach) : reach) : 0ull;
        const uint64_t cand_rows = g.ballot(cand != 0ull);
        const int er = cand_rows ? __ffsll((unsigned long long)cand_rows) - 1 : 0;
        const int eb = __shfl(cand ? __ffsll((unsigned long long)cand) - 1 : 0, g.base + er);

        if (ok && !alive) {  // FAIL: stands still, for itself and for the agents after it
            const uint16_t parked = (uint16_t)(p_in ? ag.cell() : kNoCell);
            for (int t = r; t <= w; t += G) {  // (the lanes share the time steps: no two write the same word)
                if constexpr (ROWS) {
                    MAPF_CHK(P, t * G + pr < n_hist || !p_in, 19, env, t);
                    if (p_in) occ[(size_t)t * G + pr] |= 1ull << pbit;
                } else {
                    MAPF_CHK(P, t * NP + j < n_cells - NP, 19, env, t);
                    cells[(size_t)t * NP + j] = parked;
                }
                if (t < w) pa.plan[((size_t)env * w + t) * N + j] = 0;
            }
            if (r == 0) {
                pa.arrival[(size_t)env * N + j] = -1;
                pa.remaining[(size_t)env * N + j] = -1;
            }
        }

        // the walk back from the end cell: the plan's actions, the agent's cells for the agents after it (the group's first
        // lane writes them), and the first time it stands on its goal (the walk goes down in time: the last one is the first)
        int arr = -1;
        const auto on_goal = [&](int t, int cr, int cb) { arr = (g_in && cr == gr && cb == gbit) ? t : arr; };
        const auto occupy = [&](int t, int cr, int cb) {
            if constexpr (ROWS) {
                MAPF_CHK(P, t * G + cr < n_hist, 19, env, t);
                occ[(size_t)t * G + cr] |= 1ull << cb;
            } else {
                MAPF_CHK(P, t * NP + j < n_cells - NP, 19, env, t);
                cells[(size_t)t * NP + j] = (uint16_t)(cr << 8 | (cb - pad));
            }
        };
        if (alive) {
            on_goal(w, er, eb);
            if (r == 0) occupy(w, er, eb);
        }
        walk_back(P, g, hist, n_hist, er, eb, w, alive, 18, 20, env, [&](int t, int a, int cr, int cb) {
            on_goal(t, cr, cb);
            if (r == 0) {
                pa.plan[((size_t)env * w + t) * N + j] = (int8_t)(a > 0 ? a : 0);
                occupy(t, cr, cb);
            }
        });
        if (alive && r == 0) {
            pa.arrival[(size_t)env * N + j] = arr;
            pa.remaining[(size_t)env * N + j] = D;
        }
        __syncthreads();
    }
}

// ---- conflict-based search (mapf_plan_cbs; include/mapf_step.h states the rule) ----------------------------------------
// The same lane mapping: one group owns one ENV, a workgroup is one wavefront.  An env's LDS region holds
//   cells [N][TP]   the joint plan of the node being expanded: c_0 .. c_T of every agent, 2 bytes each, and its arrival in
//                   slot T + 1 (lane r works on time step t0 + r, so neighbouring lanes read neighbouring cells)
//   info  [MP]      per node: parent, constrained agent, time | cell, the nearest ancestor that constrains the same agent
//                   at the same time (node 0 has no constraint, so 0 ends both chains)
//   key   [MP]      per node: cost << 10 | id while the node is open, all ones once it is closed
//   head  [HP]      per time step: the deepest node of the chain that constrains the agent being replanned at that time;
//                   the flood of step t walks head[t] -> same-time ancestors and reads no other constraint
// and the node store in the handle's workspace holds the paths: `root` the N unconstrained ones, a record the path of the
// one agent its node replanned, behind a 16-byte header (parent, constraint, cost, arrival).
// Every group runs the same loop, one low-level search per turn: the N searches of the root first, then, whenever it has no
// child left to build, it takes the open node with the smallest key, assembles its plan by walking the parent chain, finds
// the first conflict, and queues the two child constraints.  Groups of a wavefront are at different points of that loop
// and finish at different turns: every cross-lane operation is made by every lane, every loop around one runs while a
// ballot says that some group needs it, and a finished group only keeps its `running` flag down.
constexpr uint32_t kCbsNone = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t group_min(uint32_t v, int G) {
    for (int m = 1; m < G; m <<= 1) v = min(v, (uint32_t)__shfl_xor((int)v, m));
    return v;
}

__global__ __launch_bounds__(kPrioThreads) void k_plan_cbs(CbsArgs pa) {
    extern __shared__ __attribute__((aligned(8))) uint64_t s_cbs[];  // [envs per workgroup][cbs_env_words]
    const Params &P = *pa.params;
    const Group g(pa.G);
    const int N = pa.N, T = pa.T, M = pa.M, pad = pa.col_pad, r = g.r, G = pa.G;
    const int TP = cbs_path_cells(T), MP = (M + 1) & ~1, HP = (T + 4) & ~3;
    const EnvFrame f(pa, G, pa.epw);
    const int env = f.env;
    const bool ok = f.ok;
    if (f.none_selected()) return;  // (before any barrier)

    uint64_t *region = s_cbs + (size_t)f.slot() * cbs_env_words(N, T, M);
    uint16_t *cells = reinterpret_cast<uint16_t *>(region);
    uint2 *info = reinterpret_cast<uint2 *>(region + N * TP / 4);
    uint32_t *key = reinterpret_cast<uint32_t *>(region + N * TP / 4 + MP);
    uint16_t *head = reinterpret_cast<uint16_t *>(region + N * TP / 4 + MP + MP / 2);
    const size_t rec_bytes = cbs_record_bytes(T);
    uint64_t *hist = pa.hist + (size_t)env * (T + 1) * G + r;  // + t * G
    uint16_t *root = pa.root + (size_t)env * N * TP;
    uint8_t *recs = pa.recs + (size_t)env * M * rec_bytes;
    const uint64_t free = load_free(pa.rows, pa.H, g, ok, env);

    // group-uniform state of the search
    bool running = ok;
    int status = MAPF_CBS_BUDGET, n_nodes = 0, root_j = 0, root_cost = 0, cur = 0, cur_cost = 0, pend_n = 0, pend_i = 0;
    uint32_t pend0 = 0, pend1 = 0;  // child constraints: agent | time << 8 | cell << 16

    // a turn is one low-level search, or the turn a group finishes in: N for the root, at most two per expanded node
    for (int turn = 0; turn < N + 2 * M + 2 && __ballot(running) != 0ull; turn++) {
        // ---- the open node with the smallest (cost, id), its joint plan and its first conflict
        const bool picking = running && root_j >= N && pend_i >= pend_n;
        if (__ballot(picking) != 0ull) {
            uint32_t m = kCbsNone;
            if (picking)
                for (int i = r; i < n_nodes; i += G) m = min(m, key[i]);
            m = group_min(m, G);
            const bool expanding = picking && m != kCbsNone;
            if (picking && !expanding) {
                status = MAPF_CBS_INFEASIBLE;
                running = false;
            }
            if (expanding) {
                cur = (int)(m & 1023u);
                cur_cost = (int)(m >> 10);
                MAPF_CHK(P, cur < n_nodes, 21, env, cur);
                if (r == 0) key[cur] = kCbsNone;
                // the plan: of every agent the path of the deepest node of the chain that replanned it, else the root's
                uint64_t filled = 0ull;
                int n = cur;
                for (int s = 0; s < M && n != 0; s++) {
                    const uint2 inf = info[n];
                    const int a = (int)((inf.x >> 10) & 63u);
                    if (!((filled >> a) & 1ull)) {
                        MAPF_CHK(P, n < M && a < N, 22, env, n);
                        const uint64_t *src = reinterpret_cast<const uint64_t *>(recs + (size_t)n * rec_bytes + 16);
                        uint64_t *dst = reinterpret_cast<uint64_t *>(cells + (size_t)a * TP);
                        for (int q = r; q < TP / 4; q += G) dst[q] = src[q];
                        filled |= 1ull << a;
                    }
                    n = (int)(inf.x & 1023u);
                }
                for (int j = 0; j < N; j++) {
                    if ((filled >> j) & 1ull) continue;
                    const uint64_t *src = reinterpret_cast<const uint64_t *>(root + (size_t)j * TP);
                    uint64_t *dst = reinterpret_cast<uint64_t *>(cells + (size_t)j * TP);
                    for (int q = r; q < TP / 4; q += G) dst[q] = src[q];
                }
            }
            __syncthreads();

            // first conflict: key = t << 13 | kind << 12 | i << 6 | k, lane r looks at time t0 + r, the group takes the minimum
            uint32_t conf = kCbsNone;
            bool searching = expanding;
            for (int t0 = 0; t0 <= T && __ballot(searching) != 0ull; t0 += G) {
                const int t = t0 + r;
                uint32_t best = kCbsNone;
                if (searching && t <= T) {
                    const bool do_v = t >= 1, do_o = t <= T - 1;
                    for (int i = 0; i + 1 < N; i++) {
                        MAPF_CHK(P, i * TP + t + 1 < N * TP, 21, env, t);
                        const uint32_t ci = cells[i * TP + t], ci1 = do_o ? cells[i * TP + t + 1] : kCbsNone;
                        for (int k = i + 1; k < N; k++) {
                            const uint32_t ck = cells[k * TP + t], ik = (uint32_t)(i << 6 | k);
                            best = (do_v && ci == ck) ? min(best, ik) : best;
                            best = ci1 == ck ? min(best, ik | 1u << 12) : best;
                        }
                    }
                    best = best != kCbsNone ? (best | (uint32_t)t << 13) : best;
                }
                best = group_min(best, G);
                if (searching && best != kCbsNone) {
                    conf = best;
                    searching = false;
                }
            }
            if (expanding && conf == kCbsNone) {  // (the region keeps this node's plan for the outputs)
                status = MAPF_CBS_SOLVED;
                running = false;
            } else if (expanding) {
                const int t = (int)(conf >> 13), kind = (int)((conf >> 12) & 1u), i = (int)((conf >> 6) & 63u), k = (int)(conf & 63u);
                const uint32_t x = cells[k * TP + t];
                pend0 = (uint32_t)i | (uint32_t)(t + kind) << 8 | x << 16;
                pend1 = (uint32_t)k | (uint32_t)t << 8 | x << 16;
                pend_n = t >= 1 ? 2 : 1;  // (a constraint at time 0 makes no child)
                pend_i = 0;
            }
        }

        // ---- this turn's search: root agent root_j without constraints, or the next child's agent under the chain's
        const bool rooting = running && root_j < N;
        bool job = running && (rooting || pend_i < pend_n);
        if (job && !rooting && n_nodes >= M) {
            status = MAPF_CBS_BUDGET;
            running = false;
            job = false;
        }
        const bool child = job && !rooting;
        const uint32_t pc = pend_i == 0 ? pend0 : pend1;
        const int a = job ? (rooting ? root_j : (int)(pc & 63u)) : 0;
        const int ct = (int)((pc >> 8) & 255u);
        const uint32_t cx = pc >> 16;
        const Agent ag = load_agent(pa, job, env, a);
        const uint32_t gcell = ag.goal_cell();

        // the agent's constraints, bucketed by time; `last` = the latest one that sits on its goal
        int last = -1;
        if (child)
            for (int t = r; t < HP; t += G) head[t] = 0;
        __syncthreads();
        if (child) {
            int n = cur;
            for (int s = 0; s < M && n != 0; s++) {
                const uint2 inf = info[n];
                if ((int)((inf.x >> 10) & 63u) == a) {
                    const int t = (int)((inf.x >> 16) & 255u);
                    MAPF_CHK(P, t >= 1 && t <= T, 21, env, t);
                    last = (inf.y & 0xFFFFu) == gcell ? max(last, t) : last;
                    if (r == 0 && head[t] == 0) head[t] = (uint16_t)n;
                }
                n = (int)(inf.x & 1023u);
            }
            last = cx == gcell ? max(last, ct) : last;
        }
        __syncthreads();
        const uint32_t same = child ? head[ct] : 0u;
        __syncthreads();
        if (child && r == 0) {  // the child's own entry, where the flood finds it; it counts once the search succeeds
            MAPF_CHK(P, n_nodes >= 1 && n_nodes < M && ct >= 1 && ct <= T, 21, env, n_nodes);
            info[n_nodes] = make_uint2((uint32_t)cur | (uint32_t)a << 10 | (uint32_t)ct << 16, cx | same << 16);
            head[ct] = (uint16_t)n_nodes;
        }
        __syncthreads();

        // the flood: blocked[t] = the cells the chain of head[t] constrains the agent at
        const int A = flood_to_goal(g, hist, free, ag, job, last, T, [&](int t, bool active) {
            uint64_t blocked = 0ull;
            if (active && child) {
                uint32_t e = head[t];
                for (int s = 0; s < M && e != 0u; s++) {
                    MAPF_CHK(P, e < (uint32_t)M, 21, env, e);
                    const uint2 inf = info[e];
                    blocked |= (int)((inf.y >> 8) & 255u) == r ? 1ull << (((inf.y & 255u) + pad) & 63u) : 0ull;
                    e = inf.y >> 16;
                }
            }
            return blocked;
        });

        // the path: the goal from A on, the arrival behind it, and the walk back by lowest action id
        uint16_t *path = rooting ? root + (size_t)a * TP : reinterpret_cast<uint16_t *>(recs + (size_t)(child ? n_nodes : 0) * rec_bytes + 16);
        if (job && A >= 0) {
            for (int t = A + r; t <= T; t += G) path[t] = (uint16_t)gcell;
            if (r == 0) path[T + 1] = (uint16_t)A;
        }
        walk_back(P, g, hist, (T + 1) * G, ag.gr, ag.gbit, A, job && A > 0, 21, 23, env, [&](int t, int, int cr, int cb) {
            MAPF_CHK(P, t < TP, 22, env, t + 1);
            if (r == 0) path[t] = (uint16_t)(cr << 8 | (cb - pad));
        });

        // what the search leaves: a root path, or a child node
        if (job && rooting) {
            if (A < 0) {
                status = MAPF_CBS_NO_PATH;
                running = false;
            } else {
                root_cost += A;
                root_j++;
                if (root_j == N) {
                    n_nodes = 1;
                    if (r == 0) {
                        key[0] = (uint32_t)root_cost << 10;
                        info[0] = make_uint2(0u, 0u);
                        int32_t *hdr = reinterpret_cast<int32_t *>(recs);
                        hdr[0] = -1;
                        hdr[1] = 0;
                        hdr[2] = root_cost;
                        hdr[3] = -1;
                    }
                }
            }
        } else if (job) {
            if (A >= 0) {
                const int cost = cur_cost - (int)cells[a * TP + T + 1] + A;
                if (r == 0) {
                    key[n_nodes] = (uint32_t)cost << 10 | (uint32_t)n_nodes;
                    int32_t *hdr = reinterpret_cast<int32_t *>(recs + (size_t)n_nodes * rec_bytes);
                    hdr[0] = cur;
                    hdr[1] = (int32_t)pc;
                    hdr[2] = cost;
                    hdr[3] = A;
                }
                n_nodes++;
            }
            pend_i++;
        }
        __syncthreads();
    }
    MAPF_CHK(P, !running, 21, env, n_nodes);

    // outputs: the actions are the differences of consecutive cells
    if (ok) {
        const bool solved = status == MAPF_CBS_SOLVED;
        for (int t = r; t < T; t += G) {
            for (int j = 0; j < N; j++) {
                const int d = solved ? (int)cells[j * TP + t + 1] - (int)cells[j * TP + t] : 0;
                pa.plan[((size_t)env * T + t) * N + j] = (int8_t)(d == -256 ? 1 : d == 1 ? 2 : d == 256 ? 3 : d == -1 ? 4 : 0);
            }
        }
        for (int j = r; j < N; j += G) pa.arrival[(size_t)env * N + j] = solved ? (int32_t)cells[j * TP + T + 1] : -1;
        if (r == 0) {
            pa.status[env] = status;
            pa.nodes[env] = n_nodes;
        }
    }
}

unsigned plan_blocks(size_t searches, int G) {
    const size_t per_block = (size_t)(kPlanThreads / G);
    return (unsigned)((searches + per_block - 1) / per_block);
}

hipError_t launch_plan_expert(const PlanArgs &pa, hipStream_t s) {
    const dim3 grid(plan_blocks((size_t)pa.B * pa.N, pa.G));
    if (pa.mode == 1) LAUNCH_CHECKED(k_plan_expert<true>, grid, dim3(kPlanThreads), 0, s, pa);
    LAUNCH_CHECKED(k_plan_expert<false>, grid, dim3(kPlanThreads), 0, s, pa);
}

hipError_t launch_plan_guided(const GuidedArgs &pa, hipStream_t s) {
    LAUNCH_CHECKED(k_plan_guided, dim3(plan_blocks((size_t)pa.B * pa.N, pa.G)), dim3(kPlanThreads), 0, s, pa);
}

hipError_t launch_plan_lengths(const PlanArgs &pa, hipStream_t s) {
    LAUNCH_CHECKED(k_plan_lengths, dim3(plan_blocks((size_t)pa.K, pa.G)), dim3(kPlanThreads), 0, s, pa);
}

hipError_t launch_plan_field(const PlanArgs &pa, hipStream_t s) {
    const size_t lds = (size_t)(kPlanThreads / pa.G) * pa.H * pa.W * sizeof(uint16_t);  // <= 32 KiB: H <= G, W <= 64
    LAUNCH_CHECKED(k_plan_field, dim3(plan_blocks((size_t)pa.K, pa.G)), dim3(kPlanThreads), lds, s, pa);
}

// a joint planner: one group per env, epw envs per one-wavefront workgroup, `lds` bytes for their regions
template <typename Args>
hipError_t launch_per_env(void (*kernel)(Args), const Args &pa, size_t lds, hipStream_t s) {
    LAUNCH_CHECKED(kernel, dim3((unsigned)((pa.B + pa.epw - 1) / pa.epw)), dim3(kPrioThreads), lds, s, pa);
}

// searches a launch may hold: its grid is searches / (kPlanThreads / G) workgroups
bool plan_fits(const PlanArgs &pa, uint64_t searches) { return searches * (uint64_t)pa.G / kPlanThreads < 0x7FFFFFFFull; }

// ---- what the entry points share.  Every one refuses in this order: a null handle or argument, its own argument check
// (`bad`: what is wrong, or null), grids that are not set; then it takes the env view and the group width.
int plan_refuses(mapf_handle e, const char *name, bool null_arg, const char *bad) {
    if (!e || null_arg) return fail(e, MAPF_ERR_CONFIG, std::string(name) + ": null argument");
    if (bad) return fail(e, MAPF_ERR_CONFIG, std::string(name) + ": " + bad);
    if (!e->grids_set) return fail(e, MAPF_ERR_STATE, std::string("mapf_set_grids must be called before ") + name);
    return MAPF_OK;
}

// the shortest-path entry points: `searches` (of `what`) must fit one launch; launch(pa) runs on the handle's device
template <typename Launch>
int shortest_path_entry(mapf_handle e, const char *name, bool null_arg, const char *bad, uint64_t searches, const char *what,
                        Launch launch) {
    if (const int rc = plan_refuses(e, name, null_arg, bad)) return rc;
    PlanArgs pa{env_view(e)};
    pa.G = plan_group_width(pa.H);
    if (!plan_fits(pa, searches)) return fail(e, MAPF_ERR_CONFIG, std::string(name) + ": too many " + what + " for one launch");
    ON_DEVICE(e);
    const hipError_t s = launch(pa);
    return s == hipSuccess ? MAPF_OK : fail(e, MAPF_ERR_HIP, std::string(name) + ": launch: " + hipGetErrorString(s));
}

// the joint planners: body(pa) sizes the call, grows its workspace and launches, on the handle's device
template <typename Args, typename Body>
int joint_entry(mapf_handle e, const char *name, bool null_arg, const char *bad, const uint8_t *mask, int8_t *plan, int32_t *arrival,
                Body body) {
    if (const int rc = plan_refuses(e, name, null_arg, bad)) return rc;
    Args pa{{env_view(e), mask, plan, arrival}};
    pa.G = plan_group_width(pa.H);
    ON_DEVICE(e);
    return body(pa);
}

}  // namespace

}  // namespace mapfk

using namespace mapfk;

extern "C" {

int mapf_expert_actions(mapf_handle e, int32_t mode, int8_t *actions, int32_t *dist, void *stream) {
    const char *bad = mode != 0 && mode != 1 ? "mode must be 0 (independent) or 1 (yielding)" : nullptr;
    const uint64_t searches = e ? (uint64_t)e->p.B * (uint64_t)e->p.N : 0;
    return shortest_path_entry(e, "mapf_expert_actions", !actions, bad, searches, "agents", [&](PlanArgs &pa) {
        pa.actions = actions;
        pa.dist = dist;
        pa.mode = mode;
        return launch_plan_expert(pa, (hipStream_t)stream);
    });
}

int mapf_observe_guided(mapf_handle e, const float *obs, int32_t tail, float *out, void *stream) {
    const int64_t L = e ? mapf_obs_len(&e->cfg) : 0, rows = e ? (int64_t)e->p.B * e->p.N : 0;
    const char *ob = reinterpret_cast<const char *>(obs), *ot = reinterpret_cast<const char *>(out);
    const bool overlap = obs && out && ob < ot + rows * (L + MAPF_GUIDANCE_LEN) * 4 && ot < ob + rows * L * 4;
    const char *bad = e && e->cte            ? "a MAPF_FLAG_SINGLE_AGENT handle's observation holds the whole grid already"
                      : tail < 0 || tail > L ? "tail must lie in [0, mapf_obs_len]"
                      : !obs && tail != 0    ? "tail must be 0 when obs is NULL"
                      : overlap              ? "out overlaps obs"
                                             : nullptr;
    return shortest_path_entry(e, "mapf_observe_guided", !out, bad, (uint64_t)rows, "agents", [&](PlanArgs &pa) {
        const int Lo = obs ? (int)L : 0;
        const GuidedArgs ga{static_cast<const EnvView &>(pa), reinterpret_cast<const uint32_t *>(obs), reinterpret_cast<uint32_t *>(out),
                            pa.G, Lo, tail};
        return launch_plan_guided(ga, (hipStream_t)stream);
    });
}

int mapf_path_lengths(mapf_handle e, int32_t K, const int32_t *env_ids, const int16_t *src, const int16_t *dst, int32_t *out,
                      void *stream) {
    const char *bad = K < 1 ? "K must be >= 1" : nullptr;
    return shortest_path_entry(e, "mapf_path_lengths", !env_ids || !src || !dst || !out, bad, (uint64_t)K, "queries", [&](PlanArgs &pa) {
        pa.K = K;
        pa.env_ids = env_ids;
        pa.src = src;
        pa.dst = dst;
        pa.out = out;
        return launch_plan_lengths(pa, (hipStream_t)stream);
    });
}

int mapf_distance_field(mapf_handle e, int32_t K, const int32_t *env_ids, const int16_t *dst, uint16_t *field, void *stream) {
    const char *bad = K < 1 ? "K must be >= 1" : nullptr;
    return shortest_path_entry(e, "mapf_distance_field", !env_ids || !dst || !field, bad, (uint64_t)K, "queries", [&](PlanArgs &pa) {
        pa.K = K;
        pa.env_ids = env_ids;
        pa.dst = dst;
        pa.field = field;
        return launch_plan_field(pa, (hipStream_t)stream);
    });
}

int mapf_plan_max_horizon(mapf_handle e) { return e ? MAPF_PLAN_MAX_HORIZON(e->p.H) : 0; }

int mapf_plan_prioritized(mapf_handle e, int32_t horizon, const uint8_t *mask, int8_t *plan, int32_t *arrival, void *stream) {
    const char *bad = e && (horizon < 1 || horizon > MAPF_PLAN_MAX_HORIZON(e->p.H)) ? "horizon must lie in [1, MAPF_PLAN_MAX_HORIZON(H)]" : nullptr;
    return joint_entry<PrioArgs>(e, "mapf_plan_prioritized", !plan || !arrival, bad, mask, plan, arrival, [&](PrioArgs &pa) {
        pa.T = horizon;
        pa.NP = (pa.N + 3) & ~3;
        pa.epw = envs_per_workgroup(pa.G, prio_lds_bytes(1, pa.T, pa.NP));  // >= 1: an env's slots are at most 258 x 64 x 2 bytes
        // the workspace grows with the longest horizon asked for: a call with a horizon seen before allocates nothing
        const size_t need = (size_t)pa.B * (size_t)(horizon + 1) * (size_t)pa.G * sizeof(uint64_t);
        if (const int rc = grow_workspace(e, e->d_plan_hist, e->plan_hist_bytes, need)) return rc;
        pa.hist = e->d_plan_hist;
        HIP_TRY(e, launch_per_env(k_plan_prioritized, pa, prio_lds_bytes(pa.epw, pa.T, pa.NP), (hipStream_t)stream));
        return (int)MAPF_OK;
    });
}

int mapf_plan_max_window(mapf_handle e) { return e ? MAPF_PLAN_MAX_WINDOW : 0; }

int mapf_plan_windowed(mapf_handle e, int32_t window, const uint8_t *mask, int8_t *plan, int32_t *arrival, int32_t *remaining,
                       void *stream) {
    const char *bad = window < 1 || window > MAPF_PLAN_MAX_WINDOW ? "window must lie in [1, MAPF_PLAN_MAX_WINDOW]" : nullptr;
    return joint_entry<WinArgs>(e, "mapf_plan_windowed", !plan || !arrival || !remaining, bad, mask, plan, arrival, [&](WinArgs &pa) {
        pa.remaining = remaining;
        pa.w = window;
        pa.NP = (pa.N + 3) & ~3;
        const bool rows = win_occ_rows(pa.G, pa.w, pa.NP, pa.B, e->cus);  // (the layout only: both give the same plans)
        pa.occ_rows = rows ? 1 : 0;
        pa.epw = win_envs_per_workgroup(pa.G, pa.w, pa.NP, rows);  // >= 1: an env's region is at most 41 728 bytes with cells
        // (no workspace, nothing of the handle is written)
        HIP_TRY(e, launch_per_env(rows ? k_plan_windowed<true> : k_plan_windowed<false>, pa,
                                  (size_t)win_lds_bytes(pa.epw, pa.G, pa.w, pa.NP, rows), (hipStream_t)stream));
        return (int)MAPF_OK;
    });
}

int mapf_plan_cbs_max_nodes(mapf_handle e) {
    if (!e) return 0;
    int m = MAPF_CBS_MAX_NODES;  // (every env fits at the limits; the loop guards a build that raises them)
    while (m > 0 && cbs_envs_per_workgroup(plan_group_width(e->p.H), e->p.N, MAPF_CBS_MAX_HORIZON, m) < 1) m--;
    return m;
}

int64_t mapf_plan_cbs_workspace_bytes(mapf_handle e, int32_t horizon, int32_t max_nodes) {
    if (!e || horizon < 1 || horizon > MAPF_CBS_MAX_HORIZON || max_nodes < 1 || max_nodes > MAPF_CBS_MAX_NODES) return 0;
    return (int64_t)((size_t)e->p.B * cbs_env_workspace_bytes(plan_group_width(e->p.H), e->p.N, horizon, max_nodes));
}

int mapf_plan_cbs(mapf_handle e, int32_t horizon, int32_t max_nodes, const uint8_t *mask, int8_t *plan, int32_t *arrival,
                  int32_t *status, int32_t *nodes, void *stream) {
    const char *bad = horizon < 1 || horizon > MAPF_CBS_MAX_HORIZON     ? "horizon must lie in [1, MAPF_CBS_MAX_HORIZON]"
                      : max_nodes < 1 || max_nodes > MAPF_CBS_MAX_NODES ? "max_nodes must lie in [1, MAPF_CBS_MAX_NODES]"
                      : e && cbs_envs_per_workgroup(plan_group_width(e->p.H), e->p.N, horizon, max_nodes) < 1
                          ? "the tables of one env exceed 64 KiB of LDS"
                          : nullptr;
    return joint_entry<CbsArgs>(e, "mapf_plan_cbs", !plan || !arrival || !status || !nodes, bad, mask, plan, arrival, [&](CbsArgs &pa) {
        pa.status = status;
        pa.nodes = nodes;
        pa.T = horizon;
        pa.M = max_nodes;
        pa.epw = cbs_envs_per_workgroup(pa.G, pa.N, horizon, max_nodes);
        // the workspace grows with the largest need asked for: a call that needs no more than an earlier one allocates nothing
        const size_t B = (size_t)pa.B, need = B * cbs_env_workspace_bytes(pa.G, pa.N, horizon, max_nodes);
        if (const int rc = grow_workspace(e, e->d_cbs_ws, e->cbs_ws_bytes, need)) return rc;
        const size_t hist_bytes = B * (size_t)(horizon + 1) * pa.G * 8, root_bytes = B * (size_t)pa.N * cbs_path_cells(horizon) * 2;
        pa.hist = reinterpret_cast<uint64_t *>(e->d_cbs_ws);
        pa.root = reinterpret_cast<uint16_t *>(e->d_cbs_ws + hist_bytes);
        pa.recs = e->d_cbs_ws + hist_bytes + root_bytes;
        HIP_TRY(e, launch_per_env(k_plan_cbs, pa, (size_t)cbs_lds_bytes(pa.epw, pa.N, pa.T, pa.M), (hipStream_t)stream));
        return (int)MAPF_OK;
    });
}

}  // extern "C"
