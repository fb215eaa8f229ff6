// mapf_grad.hip -- the parameter gradients of the learner as one split-row reduction (mapf_trunk_param_grad /
// mapf_lstm_seq_param_grad / mapf_param_grad_workspace_bytes; include/mapf_step.h states the rule).
//
// Every parameter gradient of the dense trunk and of the recurrence is a product with a tiny result and an enormous inner
// dimension, dW = P^T Q summed over the rows: P a gradient per row (dpre1, dpre2, dxg), Q what the layer read in that row
// (x, a1, [a2, onehot5, pr], hprev).  On v_mfma_f32_32x32x2_f32 the rows are K: in k-step s lane (h, j) = (lane >> 5, lane & 31)
// supplies P[row 2 s + h][32 p + j] as A and Q[row 2 s + h][32 q + j] as B, and accumulator register r of the lane then holds
//   dW[32 p + (r & 3) + 8 (r >> 2) + 4 h][32 q + j]                                     (mapf_nn.h: the accumulator layout)
// so both operands are the same fetch, "row 2 s + h, 32 consecutive columns", from a row-major image of the rows.
//   rows      a workgroup (eight wavefronts) reduces one contiguous slab of rows; slab_rows_of() / slabs_of() give the
//             partition from the row count alone (MAPF_PARAM_GRAD_SLAB_ROWS, MAPF_PARAM_GRAD_MAX_SLABS), never from the device.
//   staging   the slab is walked in stages of 16 (trunk) or 32 (recurrence) rows.  A thread owns a fixed part of one row of the
//             stage, fetches it with 16-byte global loads (obs, whose rows are L floats apart, with dword loads) into registers
//             two stages ahead of the products (two stages, about 75 KB per CU, are in flight while a third is multiplied; no
//             load's address waits for another load), and writes it to the other of two LDS images; one barrier per stage.
//             A row past the slab's end is a select of zeros, never a load.  The image of a trunk row, in floats:
//               0 dpre1 | 64 dpre2 | 128 dxg | 384 x[0 .. F), 1, 0 .. | 512 a1 | 576 a2 | 640 onehot5, pr, 1, 0 .. | 672
//             and of a recurrence row: 0 dxg | 256 hprev | 320.  The constant-one column behind x and behind pr makes db1 and
//             db_lstm columns of dW1 and dW_ih; db2 is dpre2 against the tile of x that holds the one.  hprev is formed in the
//             fetch (h one step back, h0 at t = 0, zero where reset) and the six columns behind a2 by the forward kernel's rule;
//             neither exists in memory.  The operand fetch is a ds_read_b32 of 32 consecutive dwords per lane group: no bank
//             conflict at any row stride.
//   tiles     output tile k belongs to wavefront k % 8, which keeps it in 16 accumulator registers for the whole slab: at most
//             38 tiles (2 ceil((F + 1) / 32) of dW1 | db1, 2 of db2, 4 of dW2, 24 of dW_ih | db_lstm), five per wavefront; the
//             recurrence has 16, two per wavefront.
//   partials  a workgroup stores its tiles raw, [tile][register][lane], into its own part of the workspace; k_param_grad_sum adds
//             the slabs in slab order and scatters the elements to the row-major outputs.  No atomics: bitwise repeatable.
// Vector stores and plain C++ only.  fp32 throughout, no fast-math (build.py).  Row and element indices are 64-bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;

constexpr int HID = MAPF_POLICY_HIDDEN;
constexpr int G4 = 4 * HID;
constexpr int ZIN = HID + kActions + 1;  // 70
constexpr int kWaves = 8;
constexpr int kThreads = 64 * kWaves;
constexpr int kTileFloats = 32 * 32;
constexpr int kSumThreads = 256;

// the trunk's row image
constexpr int T_P1 = 0, T_P2 = HID, T_P3 = 2 * HID, T_X = 2 * HID + G4, T_A1 = T_X + 128, T_A2 = T_A1 + HID, T_SIDE = T_A2 + HID;
constexpr int T_RS = T_SIDE + 32, T_ROWS = 16;
// the recurrence's
constexpr int S_P = 0, S_Q = G4, S_RS = G4 + HID, S_ROWS = 32;
constexpr int kLstmTiles = (G4 / 32) * (HID / 32);

static_assert(HID == 64 && ZIN == 70 && MAPF_TRUNK_MAX_FEATURES + 1 <= 128, "the row images are laid out for 64 hidden units and 125 features");
static_assert(T_ROWS * 32 == kThreads && S_ROWS * 16 == kThreads, "one thread owns a fixed part of one row of a stage");
static_assert(2 * T_ROWS * T_RS * sizeof(float) <= 160 * 1024 && T_RS % 4 == 0 && S_RS % 4 == 0, "LDS budget, 16-byte rows");
static_assert(kLstmTiles == 2 * kWaves, "two tiles per wavefront");

enum { FF = 0, REC = 1, LSTM = 2 };

struct GradArgs {
    const float *obs;
    const int8_t *prev_action;
    const float *prev_reward;
    const uint8_t *first;
    const float *a1, *a2, *dpre1, *dpre2, *dxg;
    const float *h, *h0;
    const uint8_t *reset;
    float *ws;
    int64_t rows;       // the rows one grid row reduces: M, or T * (R / groups) of one group
    int64_t slab_rows;
    int64_t R;          // the recurrence: rows per step
    int32_t Rg, groups;  // R / groups
    int32_t F, L, c1, ntiles, nslabs;
};

// the partition: a function of the row count alone
int64_t slab_rows_of(int64_t rows) {
    const int64_t S = MAPF_PARAM_GRAD_SLAB_ROWS, N = MAPF_PARAM_GRAD_MAX_SLABS;
    if ((rows + S - 1) / S <= N) return S;
    return ((rows + N - 1) / N + 31) / 32 * 32;  // capped: longer slabs, whole 32-row stages
}

int64_t slabs_of(int64_t rows) {
    const int64_t per = slab_rows_of(rows);
    return (rows + per - 1) / per;
}

int trunk_c1(int F) { return (F + 1 + 31) / 32; }
int trunk_tiles(int F, bool rec) { return 2 * trunk_c1(F) + 2 + 4 + (rec ? 24 : 0); }

// output tile k of the trunk: the column offsets of its A and B operands in the row image
__device__ __forceinline__ void trunk_tile(int k, int c1, int &a, int &b) {
    if (k < 2 * c1) {  // dW1 | db1
        a = T_P1 + 32 * (k / c1), b = T_X + 32 * (k % c1);
        return;
    }
    k -= 2 * c1;
    if (k < 2) {  // db2: dpre2 against the tile of x that holds the one
        a = T_P2 + 32 * k, b = T_X + 32 * (c1 - 1);
        return;
    }
    k -= 2;
    if (k < 4) {  // dW2
        a = T_P2 + 32 * (k >> 1), b = T_A1 + 32 * (k & 1);
        return;
    }
    k -= 4;  // dW_ih | db_lstm
    a = T_P3 + 32 * (k / 3), b = T_A2 + 32 * (k % 3);
}

__device__ __forceinline__ float4 zero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }
__device__ __forceinline__ float4 ld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ void st4(float *p, const float4 &v) { *reinterpret_cast<float4 *>(p) = v; }

// what one thread holds of the stage in flight
template <int MODE>
struct Stage {
    float4 v[MODE == FF ? 2 : MODE == REC ? 4 : 5];
    float x[4];
    float side;
};

template <int MODE>
__device__ __forceinline__ void fetch(Stage<MODE> &s, const GradArgs &a, int64_t begin, int64_t end, int stage, int g) {
    const int tid = threadIdx.x;
    if constexpr (MODE == LSTM) {
        const int l = tid & 15;
        const int64_t n = begin + (int64_t)stage * S_ROWS + (tid >> 4);
        if (n >= end) {
#pragma unroll
            for (int q = 0; q < 5; q++) s.v[q] = zero4();
            return;
        }
        int64_t t, r;  // row n of group g is row r = i * groups + g of step t
        if (a.groups == 1) t = n < a.R ? 0 : 1, r = n;  // (only "step 0 or later" is asked of t)
        else if (a.rows <= 0x7fffffff) t = (uint32_t)n / (uint32_t)a.Rg, r = (int64_t)((uint32_t)n % (uint32_t)a.Rg) * a.groups + g;
        else t = n / a.Rg, r = (n % a.Rg) * a.groups + g;
        const int64_t grow = a.groups == 1 ? n : t * a.R + r;
        // no load waits for another: the reset byte selects afterwards (h one step back, or h0, is always there to be read)
        const uint8_t cut = a.reset ? a.reset[grow] : (uint8_t)0;
        const float *dx = a.dxg + grow * G4 + 4 * l;
        const float *hp = t == 0 ? a.h0 + (a.groups == 1 ? n : r) * HID + 4 * l : a.h + (grow - a.R) * HID + 4 * l;
#pragma unroll
        for (int q = 0; q < 4; q++) s.v[q] = ld4(dx + 64 * q);
        s.v[4] = ld4(hp);
        if (cut) s.v[4] = zero4();
    } else {
        const int l = tid & 31;
        const int64_t row = begin + (int64_t)stage * T_ROWS + (tid >> 5);
        const bool valid = row < end;
        const int F = a.F;
        if (!valid) {
#pragma unroll
            for (int q = 0; q < (MODE == REC ? 4 : 2); q++) s.v[q] = zero4();
#pragma unroll
            for (int q = 0; q < 4; q++) s.x[q] = 0.f;
            s.side = 0.f;
            return;
        }
        s.v[0] = l < 16 ? ld4(a.dpre1 + row * HID + 4 * l) : ld4(a.dpre2 + row * HID + 4 * (l - 16));
        if constexpr (MODE == REC) {
            s.v[1] = l < 16 ? ld4(a.a1 + row * HID + 4 * l) : ld4(a.a2 + row * HID + 4 * (l - 16));
            s.v[2] = ld4(a.dxg + row * G4 + 4 * l);
            s.v[3] = ld4(a.dxg + row * G4 + 128 + 4 * l);
            // the six columns behind a2 by the forward kernel's rule, then the constant one; the three loads do not wait for
            // each other: on a row that starts an episode the action and the reward are selected away, whatever they hold
            const uint8_t started = a.first[row];
            const int8_t pa_read = a.prev_action[row];
            const float pr_read = a.prev_reward[row];
            const int pa = started ? 0 : (int)pa_read;
            const float pr = started ? 0.f : pr_read;
            s.side = l < kActions ? (pa == l ? 1.f : 0.f) : l == kActions ? pr : l == kActions + 1 ? 1.f : 0.f;
        } else {
            s.v[1] = l < 16 ? ld4(a.a1 + row * HID + 4 * l) : zero4();
        }
        const float *x = a.obs + row * a.L;  // columns F .. L (the mask) are never read
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int c = l + 32 * q;
            s.x[q] = c < F ? x[c] : c == F ? 1.f : 0.f;
        }
    }
}

template <int MODE>
__device__ __forceinline__ void stash(const Stage<MODE> &s, float *img) {
    const int tid = threadIdx.x;
    if constexpr (MODE == LSTM) {
        const int l = tid & 15;
        float *p = img + (tid >> 4) * S_RS;
#pragma unroll
        for (int q = 0; q < 4; q++) st4(p + S_P + 64 * q + 4 * l, s.v[q]);
        st4(p + S_Q + 4 * l, s.v[4]);
    } else {
        const int l = tid & 31;
        float *p = img + (tid >> 5) * T_RS;
        st4(p + T_P1 + 4 * l, s.v[0]);  // dpre1 | dpre2
        if (MODE == REC || l < 16) st4(p + T_A1 + 4 * l, s.v[1]);  // a1 | a2
        if constexpr (MODE == REC) {
            st4(p + T_P3 + 4 * l, s.v[2]);
            st4(p + T_P3 + 128 + 4 * l, s.v[3]);
            p[T_SIDE + l] = s.side;
        }
#pragma unroll
        for (int q = 0; q < 4; q++) p[T_X + l + 32 * q] = s.x[q];
    }
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void k_param_grad(GradArgs a) {
    constexpr int RS = MODE == LSTM ? S_RS : T_RS, ROWS = MODE == LSTM ? S_ROWS : T_ROWS;
    constexpr int SLOTS = MODE == REC ? 5 : 2;  // tiles per wavefront: 38, 14 and 16 tiles at most
    __shared__ __attribute__((aligned(16))) float img[2][ROWS * RS];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;
    const int g = blockIdx.y;
    const int64_t begin = (int64_t)blockIdx.x * a.slab_rows;
    const int64_t end = begin + a.slab_rows < a.rows ? begin + a.slab_rows : a.rows;
    const int nstages = (int)((end - begin + ROWS - 1) / ROWS);  // >= 1: every slab of the partition holds a row

    int aoff[SLOTS], boff[SLOTS], nslots = 0;
#pragma unroll
    for (int t = 0; t < SLOTS; t++) {
        const int k = wave + kWaves * t;
        aoff[t] = boff[t] = 0;
        if (k < a.ntiles) {
            nslots = t + 1;
            if constexpr (MODE == LSTM) aoff[t] = S_P + 32 * (k >> 1), boff[t] = S_Q + 32 * (k & 1);
            else trunk_tile(k, a.c1, aoff[t], boff[t]);
        }
    }
    f32x16 acc[SLOTS];
#pragma unroll
    for (int t = 0; t < SLOTS; t++) acc[t] = zero_tile();

    // Two stages are in flight in registers while a third is multiplied: stage i runs from image i & 1, stage i + 1 waits in
    // `one` (odd stages) or `two` (even stages) and is written to the other image behind the products, stage i + 2 is fetched.
    // A stage past the slab's end fetches nothing and holds zeros, so the walk may run one stage over an odd count.
    auto products = [&](const float *image) {
        const float *base = image + h * RS + j;
#pragma unroll
        for (int s = 0; s < ROWS / 2; s++) {
#pragma unroll
            for (int t = 0; t < SLOTS; t++) {
                if (t < nslots)  // (uniform)
                    acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(base[2 * s * RS + aoff[t]], base[2 * s * RS + boff[t]], acc[t], 0, 0, 0);
            }
        }
    };
    Stage<MODE> one, two;
    fetch<MODE>(two, a, begin, end, 0, g);
    fetch<MODE>(one, a, begin, end, 1, g);
    stash<MODE>(two, img[0]);
    fetch<MODE>(two, a, begin, end, 2, g);
    __syncthreads();
    for (int sidx = 0; sidx < nstages; sidx += 2) {
        products(img[0]);
        stash<MODE>(one, img[1]);  // (read last in stage sidx - 1, behind the barrier that ended it)
        fetch<MODE>(one, a, begin, end, sidx + 3, g);
        __syncthreads();
        if (sidx + 1 < nstages) products(img[1]);  // (uniform)
        stash<MODE>(two, img[0]);
        fetch<MODE>(two, a, begin, end, sidx + 4, g);
        __syncthreads();
    }

    // the partial: [group][slab][tile][register][lane]
    float *out = a.ws + ((int64_t)g * a.nslabs + blockIdx.x) * a.ntiles * kTileFloats;
#pragma unroll
    for (int t = 0; t < SLOTS; t++) {
        if (t < nslots) {
            float *o = out + (int64_t)(wave + kWaves * t) * kTileFloats + lane;
#pragma unroll
            for (int r = 0; r < 16; r++) o[64 * r] = acc[t][r];
        }
    }
}

struct SumArgs {
    const float *ws;
    float *dw1, *db1, *dw2, *db2, *dwih, *dbl, *dwhh;
    int32_t F, c1, ntiles, nslabs, lstm;
};

// adds the slabs' partials in slab order, one thread per tile element, and scatters to the row-major outputs
__global__ __launch_bounds__(kSumThreads) void k_param_grad_sum(SumArgs a) {
    const int e = blockIdx.x * kSumThreads + threadIdx.x;  // < ntiles * 1024 (a whole number of blocks)
    const int g = blockIdx.y;
    const float *p = a.ws + (int64_t)g * a.nslabs * a.ntiles * kTileFloats + e;
    const int64_t stride = (int64_t)a.ntiles * kTileFloats;
    float sum = 0.f;
#pragma unroll 8
    for (int s = 0; s < a.nslabs; s++) sum += p[s * stride];
    int k = e >> 10;
    const int r = (e >> 6) & 15, lane = e & 63;
    const int i = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5), j = lane & 31;
    if (a.lstm) {
        a.dwhh[((int64_t)g * G4 + 32 * (k >> 1) + i) * HID + 32 * (k & 1) + j] = sum;
        return;
    }
    const int F = a.F, c1 = a.c1;
    if (k < 2 * c1) {
        const int row = 32 * (k / c1) + i, c = 32 * (k % c1) + j;
        if (c < F) {
            if (a.dw1) a.dw1[row * F + c] = sum;
        } else if (c == F && a.db1) a.db1[row] = sum;
        return;
    }
    k -= 2 * c1;
    if (k < 2) {
        if (32 * (c1 - 1) + j == F && a.db2) a.db2[32 * k + i] = sum;
        return;
    }
    k -= 2;
    if (k < 4) {
        if (a.dw2) a.dw2[(32 * (k >> 1) + i) * HID + 32 * (k & 1) + j] = sum;
        return;
    }
    k -= 4;
    const int row = 32 * (k / 3) + i, c = 32 * (k % 3) + j;
    if (c < ZIN) {
        if (a.dwih) a.dwih[row * ZIN + c] = sum;
    } else if (c == ZIN && a.dbl) a.dbl[row] = sum;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

int64_t mapf_param_grad_workspace_bytes(int64_t rows, int32_t F, int32_t recurrent, int32_t groups) {
    if (rows < 1 || groups < 0) return 0;
    if (groups == 0) {  // the trunk on M = rows
        if (F < 1 || F > MAPF_TRUNK_MAX_FEATURES || (recurrent != 0 && recurrent != 1)) return 0;
        return slabs_of(rows) * trunk_tiles(F, recurrent != 0) * kTileFloats * (int64_t)sizeof(float);
    }
    if (rows % groups) return 0;
    return (int64_t)groups * slabs_of(rows / groups) * kLstmTiles * kTileFloats * (int64_t)sizeof(float);
}

int mapf_trunk_param_grad(int64_t M, int32_t F, int32_t L, int32_t recurrent, const float *obs, const int8_t *prev_action,
                          const float *prev_reward, const uint8_t *first, const float *a1, const float *a2, const float *dpre1,
                          const float *dpre2, const float *dxg, float *dw1, float *db1, float *dw2, float *db2, float *dwih,
                          float *dbl, void *workspace, int64_t workspace_bytes, void *stream) {
    if (M < 1 || F < 1 || F > MAPF_TRUNK_MAX_FEATURES || (L != F && L != F + kActions) || (recurrent != 0 && recurrent != 1)) return MAPF_ERR_CONFIG;
    if (!obs || !a1 || !a2 || !dpre1 || !dpre2) return MAPF_ERR_CONFIG;
    const bool gates = dwih || dbl;
    if (!recurrent && gates) return MAPF_ERR_CONFIG;
    if (gates && (!dxg || !prev_action || !prev_reward || !first)) return MAPF_ERR_CONFIG;
    if (!aligned16(a1) || !aligned16(a2) || !aligned16(dpre1) || !aligned16(dpre2) || !aligned16(dxg)) return MAPF_ERR_CONFIG;
    if (!workspace || !aligned16(workspace) || workspace_bytes < mapf_param_grad_workspace_bytes(M, F, recurrent, 0)) return MAPF_ERR_CONFIG;
    if (!dw1 && !db1 && !dw2 && !db2 && !gates) return MAPF_OK;  // nothing is asked for
    GradArgs a{};
    a.obs = obs, a.prev_action = prev_action, a.prev_reward = prev_reward, a.first = first;
    a.a1 = a1, a.a2 = a2, a.dpre1 = dpre1, a.dpre2 = dpre2, a.dxg = dxg, a.ws = (float *)workspace;
    a.rows = M, a.slab_rows = slab_rows_of(M), a.nslabs = (int32_t)slabs_of(M), a.groups = 1;
    a.F = F, a.L = L, a.c1 = trunk_c1(F), a.ntiles = trunk_tiles(F, gates);
    const dim3 grid((uint32_t)a.nslabs);
    if (gates) hipLaunchKernelGGL(k_param_grad<REC>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_param_grad<FF>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return MAPF_ERR_HIP;
    SumArgs s{};
    s.ws = a.ws, s.dw1 = dw1, s.db1 = db1, s.dw2 = dw2, s.db2 = db2, s.dwih = dwih, s.dbl = dbl;
    s.F = F, s.c1 = a.c1, s.ntiles = a.ntiles, s.nslabs = a.nslabs;
    hipLaunchKernelGGL(k_param_grad_sum, dim3(a.ntiles * kTileFloats / kSumThreads), dim3(kSumThreads), 0, (hipStream_t)stream, s);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int mapf_lstm_seq_param_grad(int32_t T, int32_t R, int32_t groups, const float *dxg, const float *h, const float *h0,
                             const uint8_t *reset, float *dwhh, void *workspace, int64_t workspace_bytes, void *stream) {
    if (T < 1 || R < 1 || groups < 1 || groups > 65535 || R % groups) return MAPF_ERR_CONFIG;
    if (!dxg || !h || !h0 || !dwhh) return MAPF_ERR_CONFIG;
    if (!aligned16(dxg) || !aligned16(h) || !aligned16(h0)) return MAPF_ERR_CONFIG;
    const int64_t rows = (int64_t)T * R;
    if (!workspace || !aligned16(workspace) || workspace_bytes < mapf_param_grad_workspace_bytes(rows, 0, 0, groups)) return MAPF_ERR_CONFIG;
    GradArgs a{};
    a.dxg = dxg, a.h = h, a.h0 = h0, a.reset = reset, a.ws = (float *)workspace;
    a.rows = rows / groups, a.slab_rows = slab_rows_of(a.rows), a.nslabs = (int32_t)slabs_of(a.rows);
    a.R = R, a.Rg = R / groups, a.groups = groups, a.ntiles = kLstmTiles;
    hipLaunchKernelGGL(k_param_grad<LSTM>, dim3((uint32_t)a.nslabs, (uint32_t)groups), dim3(kThreads), 0, (hipStream_t)stream, a);
    if (hipGetLastError() != hipSuccess) return MAPF_ERR_HIP;
    SumArgs s{};
    s.ws = a.ws, s.dwhh = dwhh, s.ntiles = kLstmTiles, s.nslabs = a.nslabs, s.lstm = 1;
    hipLaunchKernelGGL(k_param_grad_sum, dim3(kLstmTiles * kTileFloats / kSumThreads, (uint32_t)groups), dim3(kSumThreads), 0,
                       (hipStream_t)stream, s);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
