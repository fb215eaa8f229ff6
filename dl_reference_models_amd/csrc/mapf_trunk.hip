// mapf_trunk.hip -- the dense trunk of the learner over a whole minibatch, forward and backward (mapf_trunk_forward /
// mapf_trunk_backward; include/mapf_step.h states the rule).
//
// The trunk is the first half of k_policy_act (mapf_policy.hip) on M = T * R' gathered rows instead of one step's: fc1 ->
// tanh -> fc2 -> tanh and, for a recurrent net, the input half of the LSTM gates, xg = W_ih [a2, onehot5, prev_reward] + b,
// the array mapf_lstm_seq_forward reads.  The layout is mapf_nn.h's: a wavefront owns a 32-row tile, every product is
// computed transposed on v_mfma_f32_32x32x2_f32, a result tile is the B operand of the next product register by register,
// so a1 and a2 never leave the registers between the products; they are stored once because the backward pass needs them.
//   forward:   the module's own row-major tensors (they change every Adam step, so there is no packed handle) are staged
//              once per workgroup in LDS in the order the A operand is read -- the index maps are pack_fc1 / pack_chained /
//              pack_wih of mapf_nn.h, the images those of the act kernel's packed buffer: W1 [S1][2][64] (at most 63 k-steps,
//              32 256 bytes), W2 [32][2][64] (16 KB), W_ih [2][35][4][64] (71 680 bytes), the biases (b_ih + b_hh summed) 1.5 KB.
//   backward:  dpre2 = (W_ih[:, :64]^T dxg) (1 - a2^2), dpre1 = (W2^T dpre2) (1 - a1^2): dxg is loaded tile by tile in
//              accumulator layout and is the B operand as it is; the images are the same matrices transposed, W_ih^T
//              [128][2][64] (64 KB) and W2^T [32][2][64] (16 KB).
// A workgroup is eight wavefronts (two per SIMD: one's tanh and stores overlap the other's products) and holds the whole
// LDS budget of its CU's share, so one workgroup is resident per CU; it walks its tiles with the grid's stride, and the grid
// is the number of 8-tile groups capped at the CU count, so a small launch stages the weights in few workgroups.
// Vector stores and plain C++ only.  fp32 throughout, libm-grade tanh, no fast-math (build.py); no atomics, no reduction
// over rows: a row's results depend on that row's inputs alone (an MFMA column depends on its own B column), so both calls
// are bitwise repeatable and a row does not see its neighbours or its place in the launch.  Row and element indices are
// 64-bit.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // the accumulator layout: load_tile / store_tile / chain, the pack_* index maps

constexpr int HID = MAPF_POLICY_HIDDEN;
constexpr int NT = HID / 32;          // 32-feature accumulator tiles of a1 / a2
constexpr int CH = HID / 2;           // chained k-steps over a 64-feature input
constexpr int G4 = 4 * HID;           // gate features per row
constexpr int ZIN = HID + kActions + 1;  // 70: [a2, onehot5(prev_action), prev_reward]
constexpr int kExtraSteps = 3;        // k-steps of the LSTM input past a2
constexpr int KS = CH + kExtraSteps;  // k-steps of one hidden tile's gate products
constexpr int kTile = 32;             // rows per wavefront (the MFMA's N)
constexpr int kWaves = 8;             // wavefronts per workgroup
constexpr int kThreads = 64 * kWaves;
constexpr int kMaxF = MAPF_TRUNK_MAX_FEATURES;
constexpr int kMaxS1 = (kMaxF + 1) / 2;
constexpr int kChunk = 8;            // k-steps of fc1 whose features are loaded together

constexpr int kW1Floats = kMaxS1 * NT * 64;    // 8 064
constexpr int kW2Floats = CH * NT * 64;        // 4 096
constexpr int kWihFloats = NT * KS * 4 * 64;   // 17 920
constexpr int kWihTFloats = (G4 / 2) * NT * 64;  // 16 384: W_ih[:, :64]^T, 128 chained k-steps

static_assert(kW2Floats % kThreads == 0 && kWihFloats % kThreads == 0 && kWihTFloats % kThreads == 0, "whole staging trips");
static_assert(HID == 64 && ZIN == 70, "the LDS images below are laid out for 64 hidden units");
static_assert(2 * kExtraSteps >= kActions + 1, "the extra k-steps hold the one-hot and the reward");
static_assert((kW1Floats + kW2Floats + kWihFloats + HID + HID + G4) * sizeof(float) <= 128 * 1024, "forward LDS budget");

struct FwdArgs {
    const float *obs;
    const int8_t *prev_action;
    const float *prev_reward;
    const uint8_t *first;
    const float *w1, *b1, *w2, *b2, *wih, *bih, *bhh;
    float *a1, *a2, *xg;
    int64_t M, groups;  // groups = ceil(M / (32 * 8)): the 8-tile groups the workgroups share out
    int32_t F, L;
};

__device__ __forceinline__ void tanh_tiles(f32x16 (&v)[NT]) {
#pragma unroll
    for (int m = 0; m < NT; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) v[m][r] = tanhf(v[m][r]);
}

template <bool REC>
__global__ __launch_bounds__(kThreads) void k_trunk_forward(FwdArgs a) {
    __shared__ __attribute__((aligned(16))) float w1img[kW1Floats];
    __shared__ __attribute__((aligned(16))) float w2img[kW2Floats];
    __shared__ __attribute__((aligned(16))) float wihimg[REC ? kWihFloats : 64];
    __shared__ __attribute__((aligned(16))) float b1s[HID], b2s[HID], bls[REC ? G4 : 4];
    const int F = a.F, L = a.L, S1 = (F + 1) / 2;
    // the images, in the order the A operand is read (a padding element of fc1's odd tail is 0); the loops are unrolled so that
    // a thread's loads are in flight together instead of one round trip each
#pragma unroll 4
    for (int e = threadIdx.x; e < S1 * NT * 64; e += kThreads) w1img[e] = pack_read(a.w1, 0, pack_fc1(e, NT, F));
#pragma unroll
    for (int e = threadIdx.x; e < kW2Floats; e += kThreads) w2img[e] = a.w2[pack_chained(e, NT)];
    if (threadIdx.x < HID) b1s[threadIdx.x] = a.b1[threadIdx.x], b2s[threadIdx.x] = a.b2[threadIdx.x];
    if constexpr (REC) {
#pragma unroll 7
        for (int e = threadIdx.x; e < kWihFloats; e += kThreads) wihimg[e] = pack_read(a.wih, 0, pack_wih(e, NT, KS, ZIN));
        if (threadIdx.x < G4) bls[threadIdx.x] = a.bih[threadIdx.x] + a.bhh[threadIdx.x];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;

    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {  // (no barrier inside: the waves walk on their own)
        const int64_t row0 = (grp * kWaves + wave) * kTile;
        if (row0 >= a.M) break;  // a whole wavefront past the last row has nothing to do (its later tiles lie further out)
        const int64_t row = row0 + j;
        const bool valid = row < a.M;  // a lane past the last row computes on zeros and stores nothing

        // a1 = tanh(W1 x + b1): k-steps in natural order, lane half h supplies obs[row][2 s + h]; 0 past F, so the tail of
        // the last step at odd F never comes from memory and the mask columns F .. L are never read
        f32x16 a1[NT], a2[NT];
#pragma unroll
        for (int m = 0; m < NT; m++) a1[m] = load_tile(b1s + 32 * m, h);
        {
            // the row's features are fetched kChunk k-steps ahead of the products that take them: a lane's loads of one
            // chunk are independent, and the next chunk's are in flight while this one's products run
            const float *x = a.obs + row * L;  // (dereferenced for valid rows only)
            const float *w1 = w1img + lane;
            float cur[kChunk], nxt[kChunk];
#pragma unroll
            for (int e = 0; e < kChunk; e++) {
                const int k = 2 * e + h;
                cur[e] = valid && k < F ? x[k] : 0.f;
            }
            for (int s0 = 0; s0 < S1; s0 += kChunk) {
#pragma unroll
                for (int e = 0; e < kChunk; e++) {
                    const int k = 2 * (s0 + kChunk + e) + h;
                    nxt[e] = valid && k < F ? x[k] : 0.f;
                }
#pragma unroll
                for (int e = 0; e < kChunk; e++) {
                    const int s = s0 + e;
                    if (s < S1) {  // (uniform; the image holds S1 k-steps)
#pragma unroll
                        for (int m = 0; m < NT; m++) a1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[(s * NT + m) * 64], cur[e], a1[m], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int e = 0; e < kChunk; e++) cur[e] = nxt[e];
            }
        }
        tanh_tiles(a1);
        if (valid) {
#pragma unroll
            for (int m = 0; m < NT; m++) store_tile(a.a1 + row * HID + 32 * m, h, a1[m]);
        }

        // a2 = tanh(W2 a1 + b2)
#pragma unroll
        for (int m = 0; m < NT; m++) a2[m] = load_tile(b2s + 32 * m, h);
        chain<NT, NT>(a2, a1, w2img, lane);
        tanh_tiles(a2);
        if (valid) {
#pragma unroll
            for (int m = 0; m < NT; m++) store_tile(a.a2 + row * HID + 32 * m, h, a2[m]);
        }

        if constexpr (REC) {
            // z = [a2, onehot5(prev_action), prev_reward]; a row that starts an episode takes action 0 and reward 0, a byte
            // outside 0 .. 4 matches no one-hot index
            int pa = 0;
            float pr = 0.f;
            if (valid && !a.first[row]) pa = a.prev_action[row], pr = a.prev_reward[row];
            float zx[kExtraSteps];
#pragma unroll
            for (int e = 0; e < kExtraSteps; e++) {
                const int idx = 2 * e + h;
                zx[e] = idx < kActions ? (pa == idx ? 1.f : 0.f) : (idx == kActions ? pr : 0.f);
            }
#pragma unroll
            for (int q = 0; q < NT; q++) {  // hidden units 32 q .. 32 q + 31: gate tiles i, f, g, o
                f32x16 gate[4];
#pragma unroll
                for (int g = 0; g < 4; g++) gate[g] = load_tile(bls + HID * g + 32 * q, h);
                const float *wih = wihimg + q * KS * 256;
                chain<4, NT>(gate, a2, wih, lane);
#pragma unroll
                for (int e = 0; e < kExtraSteps; e++)
#pragma unroll
                    for (int g = 0; g < 4; g++)
                        gate[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(wih[((CH + e) * 4 + g) * 64 + lane], zx[e], gate[g], 0, 0, 0);
                if (valid) {
#pragma unroll
                    for (int g = 0; g < 4; g++) store_tile(a.xg + row * G4 + HID * g + 32 * q, h, gate[g]);
                }
            }
        }
    }
}

struct BwdArgs {
    const float *dxg, *da2, *a1, *a2, *wih, *w2;
    float *dpre2, *dpre1;
    int64_t M, groups;
};

// v = v (1 - a^2), a the saved activation of the same rows in the same layout
__device__ __forceinline__ void tanh_backward(f32x16 (&v)[NT], const float *act, int h, bool valid) {
#pragma unroll
    for (int m = 0; m < NT; m++) {
        const f32x16 s = valid ? load_tile(act + 32 * m, h) : zero_tile();
#pragma unroll
        for (int r = 0; r < 16; r++) v[m][r] = v[m][r] * (1.0f - s[r] * s[r]);
    }
}

template <bool REC>
__global__ __launch_bounds__(kThreads) void k_trunk_backward(BwdArgs a) {
    __shared__ __attribute__((aligned(16))) float wihT[REC ? kWihTFloats : 64];
    __shared__ __attribute__((aligned(16))) float w2T[kW2Floats];
    // transposed images: chained k-step st of output tile m reads W[k = chained_feature(st, lane >> 5)][32 m + (lane & 31)]
    if constexpr (REC) {
#pragma unroll 8
        for (int e = threadIdx.x; e < kWihTFloats; e += kThreads) {
            const int lane = e & 63, m = (e >> 6) % NT, st = (e >> 6) / NT;
            wihT[e] = a.wih[chained_feature(st, lane >> 5) * ZIN + 32 * m + (lane & 31)];
        }
    }
#pragma unroll
    for (int e = threadIdx.x; e < kW2Floats; e += kThreads) {
        const int lane = e & 63, m = (e >> 6) % NT, st = (e >> 6) / NT;
        w2T[e] = a.w2[chained_feature(st, lane >> 5) * HID + 32 * m + (lane & 31)];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, j = lane & 31, h = lane >> 5;

    for (int64_t grp = blockIdx.x; grp < a.groups; grp += gridDim.x) {
        const int64_t row0 = (grp * kWaves + wave) * kTile;
        if (row0 >= a.M) break;
        const int64_t row = row0 + j;
        const bool valid = row < a.M;

        f32x16 d2[NT], d1[NT];
        if constexpr (REC) {
            // da2 = W_ih[:, :64]^T dxg: the eight 32-feature tiles of a row's dxg, each the B operand as it is loaded
#pragma unroll
            for (int m = 0; m < NT; m++) d2[m] = zero_tile();
            f32x16 in[2][1];  // (double-buffered: tile c + 1 is in flight while tile c's products run)
            in[0][0] = valid ? load_tile(a.dxg + row * G4, h) : zero_tile();
#pragma unroll
            for (int c = 0; c < G4 / 32; c++) {
                if (c + 1 < G4 / 32) in[(c + 1) & 1][0] = valid ? load_tile(a.dxg + row * G4 + 32 * (c + 1), h) : zero_tile();
                chain<NT, 1>(d2, in[c & 1], wihT + c * 16 * NT * 64, lane);
            }
        } else {
#pragma unroll
            for (int m = 0; m < NT; m++) d2[m] = valid ? load_tile(a.da2 + row * HID + 32 * m, h) : zero_tile();
        }
        tanh_backward(d2, a.a2 + row * HID, h, valid);
        if (valid) {
#pragma unroll
            for (int m = 0; m < NT; m++) store_tile(a.dpre2 + row * HID + 32 * m, h, d2[m]);
        }
#pragma unroll
        for (int m = 0; m < NT; m++) d1[m] = zero_tile();
        chain<NT, NT>(d1, d2, w2T, lane);
        tanh_backward(d1, a.a1 + row * HID, h, valid);
        if (valid) {
#pragma unroll
            for (int m = 0; m < NT; m++) store_tile(a.dpre1 + row * HID + 32 * m, h, d1[m]);
        }
    }
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

// the 8-tile groups of M rows and the grid that shares them out: one workgroup per group, capped at the workgroups that
// stay resident (one per CU: a workgroup holds more than half of a CU's LDS)
int64_t groups_of(int64_t M) { return (M + kTile * kWaves - 1) / (kTile * kWaves); }

uint32_t grid_of(int64_t groups) {
    static int cus[64] = {};  // per device, asked once (a host-side query: no stream operation, so capture is not disturbed)
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
    if (cus[dev] <= 0) {
        int n = 0;
        if (hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n <= 0) n = 256;
        cus[dev] = n;
    }
    return (uint32_t)(groups < cus[dev] ? groups : cus[dev]);
}

}  // namespace

extern "C" {

int mapf_trunk_forward(int64_t M, int32_t F, int32_t L, int32_t recurrent, const float *obs, const int8_t *prev_action,
                       const float *prev_reward, const uint8_t *first, const float *w1, const float *b1, const float *w2,
                       const float *b2, const float *wih, const float *bih, const float *bhh, float *a1, float *a2, float *xg,
                       void *stream) {
    if (M < 1 || F < 1 || F > kMaxF || (L != F && L != F + kActions) || (recurrent != 0 && recurrent != 1)) return MAPF_ERR_CONFIG;
    if (!obs || !w1 || !b1 || !w2 || !b2 || !a1 || !a2) return MAPF_ERR_CONFIG;
    if (recurrent ? (!prev_action || !prev_reward || !first || !wih || !bih || !bhh || !xg) : (xg != nullptr)) return MAPF_ERR_CONFIG;
    if (!aligned16(a1) || !aligned16(a2) || !aligned16(xg)) return MAPF_ERR_CONFIG;  // (the 16-byte stores)
    FwdArgs a{};
    a.obs = obs, a.prev_action = prev_action, a.prev_reward = prev_reward, a.first = first;
    a.w1 = w1, a.b1 = b1, a.w2 = w2, a.b2 = b2, a.wih = wih, a.bih = bih, a.bhh = bhh, a.a1 = a1, a.a2 = a2, a.xg = xg;
    a.M = M, a.groups = groups_of(M), a.F = F, a.L = L;
    const dim3 grid(grid_of(a.groups));
    if (recurrent) hipLaunchKernelGGL(k_trunk_forward<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_trunk_forward<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int mapf_trunk_backward(int64_t M, int32_t recurrent, const float *dxg, const float *da2, const float *a1, const float *a2,
                        const float *wih, const float *w2, float *dpre2, float *dpre1, void *stream) {
    if (M < 1 || (recurrent != 0 && recurrent != 1) || !a1 || !a2 || !w2 || !dpre2 || !dpre1) return MAPF_ERR_CONFIG;
    if (recurrent ? (!dxg || !wih || da2 != nullptr) : (!da2 || dxg != nullptr)) return MAPF_ERR_CONFIG;
    if (!aligned16(dxg) || !aligned16(da2) || !aligned16(a1) || !aligned16(a2) || !aligned16(dpre2) || !aligned16(dpre1)) return MAPF_ERR_CONFIG;
    BwdArgs a{};
    a.dxg = dxg, a.da2 = da2, a.a1 = a1, a.a2 = a2, a.wih = wih, a.w2 = w2, a.dpre2 = dpre2, a.dpre1 = dpre1;
    a.M = M, a.groups = groups_of(M);
    const dim3 grid(grid_of(a.groups));
    if (recurrent) hipLaunchKernelGGL(k_trunk_backward<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(k_trunk_backward<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
