// mapf_lstm.hip -- the LSTM recurrence of the learner over a whole fragment, forward and backward (mapf_lstm_seq_*;
// include/mapf_step.h states the rule).
//
// Only the recurrence is sequential in t: the caller evaluates the input half of the gates (xg = W_ih z + b) for all T at
// once, and these two kernels walk t inside ONE launch each.  The layout is k_policy_act's (mapf_policy.hip): a wavefront
// owns 32 rows for all T and computes every product transposed on v_mfma_f32_32x32x2_f32, so a result tile has the row on
// the lane (j = lane & 31) and feature (r & 3) + 8 (r >> 2) + 4 (lane >> 5) of its 32-feature tile in accumulator register
// r -- which is the B-operand layout of the next product when its k-steps are taken register by register.
//   forward:   G_t = xg_t + W_hh h_{t-1}      h_t leaves the cell update in the layout the next step's product reads
//   backward:  dh_{t-1} += W_hh^T dG_t        dG_t is formed lane-locally from gates / c / dh and is the B operand as it is
// W_hh (64 KB) is staged once per workgroup in LDS, in the order the A operand is read: forward 16 bytes per lane per
// k-step (the four gates of one hidden unit), backward 16 bytes per lane per pair of k-steps (two steps x two output tiles);
// a wavefront's read is one contiguous 1 KB block.  The backward image is the same matrix transposed.  A workgroup is four
// wavefronts (128 rows): two workgroups share a CU's LDS, two wavefronts a SIMD's matrix pipe.
// Vector stores and plain C++ only.  fp32 throughout, libm-grade tanh / exp, no fast-math (build.py); no atomics: a row's
// results depend on that row's inputs alone, so both calls are bitwise repeatable and a row does not see its neighbours.
// GROUPS (mapf_lstm_seq_*_grouped): `groups` weight matrices, row r recurring through W_hh[r % groups] (one policy per
// agent on interleaved agent rows).  A workgroup stages the image of ONE group and its lanes own rows g + groups * i of it,
// i = 0 .. rows / groups - 1; the grid is groups * ceil(rows / groups / 128).  The ungrouped entry points are groups = 1 of
// the same kernels (row = i, one image), so a group's rows get the bits the ungrouped call gives them gathered contiguously.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // the accumulator layout: load_tile / store_tile / zero_tile, reg_of / half_of, sigmoidf

constexpr int HID = MAPF_POLICY_HIDDEN;
constexpr int kTile = 32;      // rows per wavefront (the MFMA's N)
constexpr int kWaves = 4;      // wavefronts per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int NT = HID / 32;   // 32-feature accumulator tiles of h
constexpr int G4 = 4 * HID;    // gate features per row
constexpr int kWhhFloats = G4 * HID;

static_assert(HID == 64, "the LDS images below are laid out for 64 hidden units");
static_assert(kWhhFloats * sizeof(float) == 65536, "W_hh fills 64 KB of LDS");

// Forward image: k-step st = 16 m + r of hidden tile q reads float4 fw[(q * 32 + st) * 64 + lane] = gates i, f, g, o of
// W_hh[64 g + 32 q + (lane & 31)][feature 32 m + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)].  Read coalesced, scattered into LDS.
__device__ __forceinline__ void stage_forward(float *img, const float *__restrict__ whh) {
    for (int e = threadIdx.x; e < kWhhFloats; e += blockDim.x) {
        const int row = e >> 6, k = e & 63;
        const int g = row >> 6, q = (row >> 5) & 1, i = row & 31;
        const int st = 16 * (k >> 5) + reg_of(k & 31), lane = i + 32 * half_of(k & 31);
        img[((q * 32 + st) * 64 + lane) * 4 + g] = whh[e];
    }
}

// Backward image: k-step s = (4 q + g) * 16 + r (gate feature 64 g + 32 q + (r & 3) + 8 (r >> 2) + 4 (lane >> 5)) of output
// tile m reads bw[((s >> 1) * 64 + lane) * 4 + 2 (s & 1) + m] = W_hh[that gate feature][32 m + (lane & 31)].
__device__ __forceinline__ void stage_backward(float *img, const float *__restrict__ whh) {
    for (int e = threadIdx.x; e < kWhhFloats; e += blockDim.x) {
        const int row = e >> 6, k = e & 63;
        const int g = row >> 6, q = (row >> 5) & 1, kk = row & 31;
        const int s = (4 * q + g) * 16 + reg_of(kk), lane = (k & 31) + 32 * half_of(kk), m = k >> 5;
        img[((s >> 1) * 64 + lane) * 4 + 2 * (s & 1) + m] = whh[e];
    }
}

struct FwdArgs {
    const float *xg, *whh;
    const uint8_t *reset;
    const float *h0, *c0;
    float *h, *c, *gates;
    int32_t T, rows, groups, per_group, group_blocks;  // per_group = rows / groups, group_blocks = ceil(per_group / 128)
};

// blocks are group-major (the blocks of a group are neighbours): the workgroup's group, and a lane's index inside it
__device__ __forceinline__ int group_of_block(int group_blocks) { return (int)(blockIdx.x / (uint32_t)group_blocks); }
__device__ __forceinline__ int64_t index_in_group(int group_blocks, int wave, int j) {
    return ((int64_t)(blockIdx.x % (uint32_t)group_blocks) * kWaves + wave) * kTile + j;
}

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_lstm_seq_forward(FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float img[kWhhFloats];
    stage_forward(img, a.whh + (int64_t)group_of_block(a.group_blocks) * kWhhFloats);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
    const int64_t idx = index_in_group(a.group_blocks, wave, j);
    const int64_t row = group_of_block(a.group_blocks) + (int64_t)a.groups * idx;
    const bool valid = idx < a.per_group;  // a lane past the last row computes on zeros and stores nothing
    if (idx - j >= a.per_group) return;  // (a whole wavefront past it has nothing to do; no barrier follows)
    const float4 *fw = reinterpret_cast<const float4 *>(img) + lane;

    f32x16 hold[NT], cold[NT], hnew[NT];
#pragma unroll
    for (int q = 0; q < NT; q++) {
        hold[q] = valid ? load_tile(a.h0 + row * HID + 32 * q, hh) : zero_tile();
        cold[q] = valid ? load_tile(a.c0 + row * HID + 32 * q, hh) : zero_tile();
    }
    for (int t = 0; t < a.T; t++) {
        const int64_t at = (int64_t)t * a.rows + row;
        if (valid && a.reset && a.reset[at]) {
#pragma unroll
            for (int q = 0; q < NT; q++) hold[q] = zero_tile(), cold[q] = zero_tile();
        }
#pragma unroll
        for (int q = 0; q < NT; q++) {  // hidden units 32 q .. 32 q + 31: gate tiles i, f, g, o
            f32x16 gate[4];
#pragma unroll
            for (int g = 0; g < 4; g++) gate[g] = valid ? load_tile(a.xg + at * G4 + HID * g + 32 * q, hh) : zero_tile();
#pragma unroll
            for (int st = 0; st < 16 * NT; st++) {
                const float4 w = fw[(q * 16 * NT + st) * 64];
                const float b = hold[st >> 4][st & 15];
                gate[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, b, gate[0], 0, 0, 0);
                gate[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, b, gate[1], 0, 0, 0);
                gate[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, b, gate[2], 0, 0, 0);
                gate[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, b, gate[3], 0, 0, 0);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float gi = sigmoidf(gate[0][r]), gf = sigmoidf(gate[1][r]), gg = tanhf(gate[2][r]), go = sigmoidf(gate[3][r]);
                const float c1 = gf * cold[q][r] + gi * gg;
                gate[0][r] = gi, gate[1][r] = gf, gate[2][r] = gg, gate[3][r] = go;
                cold[q][r] = c1;
                hnew[q][r] = go * tanhf(c1);
            }
            if (valid) {
                if (a.gates) {
#pragma unroll
                    for (int g = 0; g < 4; g++) store_tile(a.gates + at * G4 + HID * g + 32 * q, hh, gate[g]);
                }
                store_tile(a.c + at * HID + 32 * q, hh, cold[q]);
                store_tile(a.h + at * HID + 32 * q, hh, hnew[q]);
            }
        }
#pragma unroll
        for (int q = 0; q < NT; q++) hold[q] = hnew[q];
    }
}

struct BwdArgs {
    const float *whh;
    const uint8_t *reset;
    const float *c0, *c, *gates, *dh, *dhT, *dcT;
    float *dxg, *dh0, *dc0;
    int32_t T, rows, groups, per_group, group_blocks;
};

__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_lstm_seq_backward(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float img[kWhhFloats];
    stage_backward(img, a.whh + (int64_t)group_of_block(a.group_blocks) * kWhhFloats);
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, hh = lane >> 5;
    const int64_t idx = index_in_group(a.group_blocks, wave, j);
    const int64_t row = group_of_block(a.group_blocks) + (int64_t)a.groups * idx;
    const bool valid = idx < a.per_group;  // a lane past the last row computes on zeros and stores nothing
    if (idx - j >= a.per_group) return;
    const float4 *bw = reinterpret_cast<const float4 *>(img) + lane;

    // the gradient that arrives from step t + 1 (dhT / dcT at the last step)
    f32x16 dhr[NT], dcr[NT], acc[NT];
#pragma unroll
    for (int q = 0; q < NT; q++) {
        dhr[q] = valid && a.dhT ? load_tile(a.dhT + row * HID + 32 * q, hh) : zero_tile();
        dcr[q] = valid && a.dcT ? load_tile(a.dcT + row * HID + 32 * q, hh) : zero_tile();
    }
    for (int t = a.T - 1; t >= 0; t--) {
        const int64_t at = (int64_t)t * a.rows + row;
        const bool cut = valid && a.reset && a.reset[at];  // step t started from zeros: nothing flows into step t - 1
        const float *cprev = t > 0 ? a.c + (at - a.rows) * HID : a.c0 + row * HID;
#pragma unroll
        for (int m = 0; m < NT; m++) acc[m] = zero_tile();
#pragma unroll
        for (int q = 0; q < NT; q++) {
            f32x16 dg[4];
            {
                f32x16 ct = zero_tile(), cp = zero_tile(), dht = zero_tile();
#pragma unroll
                for (int g = 0; g < 4; g++) dg[g] = valid ? load_tile(a.gates + at * G4 + HID * g + 32 * q, hh) : zero_tile();
                if (valid) {
                    ct = load_tile(a.c + at * HID + 32 * q, hh);
                    dht = load_tile(a.dh + at * HID + 32 * q, hh);
                    if (!cut) cp = load_tile(cprev + 32 * q, hh);
                }
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const float gi = dg[0][r], gf = dg[1][r], gg = dg[2][r], go = dg[3][r];
                    const float tc = tanhf(ct[r]);
                    const float dhv = dht[r] + dhr[q][r];
                    const float dcv = dcr[q][r] + dhv * go * (1.0f - tc * tc);
                    dg[0][r] = dcv * gg * gi * (1.0f - gi);
                    dg[1][r] = dcv * cp[r] * gf * (1.0f - gf);
                    dg[2][r] = dcv * gi * (1.0f - gg * gg);
                    dg[3][r] = dhv * tc * go * (1.0f - go);
                    dcr[q][r] = cut ? 0.f : dcv * gf;
                }
            }
            if (valid) {
#pragma unroll
                for (int g = 0; g < 4; g++) store_tile(a.dxg + at * G4 + HID * g + 32 * q, hh, dg[g]);
            }
#pragma unroll
            for (int g = 0; g < 4; g++) {
#pragma unroll
                for (int r = 0; r < 16; r += 2) {
                    const int s = (4 * q + g) * 16 + r;
                    const float4 w = bw[(s >> 1) * 64];
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.x, dg[g][r], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.y, dg[g][r], acc[1], 0, 0, 0);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.z, dg[g][r + 1], acc[0], 0, 0, 0);
                    acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(w.w, dg[g][r + 1], acc[1], 0, 0, 0);
                }
            }
        }
#pragma unroll
        for (int m = 0; m < NT; m++) dhr[m] = cut ? zero_tile() : acc[m];
    }
    if (valid) {
#pragma unroll
        for (int q = 0; q < NT; q++) {
            if (a.dh0) store_tile(a.dh0 + row * HID + 32 * q, hh, dhr[q]);
            if (a.dc0) store_tile(a.dc0 + row * HID + 32 * q, hh, dcr[q]);
        }
    }
}

int blocks_of(int32_t per_group) { return (int)(((int64_t)per_group + kTile * kWaves - 1) / (kTile * kWaves)); }

}  // namespace

extern "C" {

int mapf_lstm_seq_forward_grouped(int32_t T, int32_t rows, int32_t groups, const float *xg, const float *whh, const uint8_t *reset,
                                  const float *h0, const float *c0, float *h, float *c, float *gates, void *stream) {
    if (T < 1 || rows < 1 || groups < 1 || rows % groups != 0 || !xg || !whh || !h0 || !c0 || !h || !c) return MAPF_ERR_CONFIG;
    FwdArgs a{};
    a.xg = xg, a.whh = whh, a.reset = reset, a.h0 = h0, a.c0 = c0, a.h = h, a.c = c, a.gates = gates, a.T = T, a.rows = rows;
    a.groups = groups, a.per_group = rows / groups, a.group_blocks = blocks_of(a.per_group);
    const dim3 grid((uint32_t)((int64_t)groups * a.group_blocks));
    hipLaunchKernelGGL(k_lstm_seq_forward, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int mapf_lstm_seq_backward_grouped(int32_t T, int32_t rows, int32_t groups, const float *whh, const uint8_t *reset, const float *c0,
                                   const float *c, const float *gates, const float *dh, const float *dhT, const float *dcT,
                                   float *dxg, float *dh0, float *dc0, void *stream) {
    if (T < 1 || rows < 1 || groups < 1 || rows % groups != 0 || !whh || !c0 || !c || !gates || !dh || !dxg) return MAPF_ERR_CONFIG;
    BwdArgs a{};
    a.whh = whh, a.reset = reset, a.c0 = c0, a.c = c, a.gates = gates, a.dh = dh, a.dhT = dhT, a.dcT = dcT;
    a.dxg = dxg, a.dh0 = dh0, a.dc0 = dc0, a.T = T, a.rows = rows;
    a.groups = groups, a.per_group = rows / groups, a.group_blocks = blocks_of(a.per_group);
    const dim3 grid((uint32_t)((int64_t)groups * a.group_blocks));
    hipLaunchKernelGGL(k_lstm_seq_backward, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int mapf_lstm_seq_forward(int32_t T, int32_t rows, const float *xg, const float *whh, const uint8_t *reset, const float *h0,
                          const float *c0, float *h, float *c, float *gates, void *stream) {
    return mapf_lstm_seq_forward_grouped(T, rows, 1, xg, whh, reset, h0, c0, h, c, gates, stream);
}

int mapf_lstm_seq_backward(int32_t T, int32_t rows, const float *whh, const uint8_t *reset, const float *c0, const float *c,
                           const float *gates, const float *dh, const float *dhT, const float *dcT, float *dxg, float *dh0,
                           float *dc0, void *stream) {
    return mapf_lstm_seq_backward_grouped(T, rows, 1, whh, reset, c0, c, gates, dh, dhT, dcT, dxg, dh0, dc0, stream);
}

}  // extern "C"
