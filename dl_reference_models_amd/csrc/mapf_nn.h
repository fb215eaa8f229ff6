// mapf_nn.h -- what the neural units of libmapfstep.so share (mapf_policy.hip, mapf_policy_joint.hip, mapf_lstm.hip,
// mapf_dqn.hip, mapf_vtrace.hip): the accumulator layout and the helpers that rest on it, the random-number pieces, the
// small reductions, the index maps of the packed weight buffer and the host side of a network handle.  Helpers only: the
// fc1 front ends, the LSTM cell bodies, the epilogues and the layout structs belong to the units, where they differ.
//
// THE ACCUMULATOR LAYOUT.  Every product is computed transposed on v_mfma_f32_32x32x2_f32,
//   D[out feature i][row j] = sum_k W[i][k] * X^T[k][j]        A = W (one dword per lane), B = X^T (one dword per lane)
// so a 32-feature result tile has the row on the lane (j = lane & 31) and, in accumulator register r of lane half
// h = lane >> 5, feature
//   (r & 3) + 8 * (r >> 2) + 4 * h                              (chained_feature; reg_of / half_of are the inverse)
// That IS the B-operand layout of the next product when its k-steps are taken in the order "register r of tile m": in
// chained k-step st = 16 m + r lane half h supplies feature 32 m + (r & 3) + 8 (r >> 2) + 4 h, and the packing index maps
// below place the weight of exactly that feature in the A dword of the same lane in the same step.  Registers 4g .. 4g + 3
// of a lane half are four consecutive features, so a tile moves to and from a row of memory in 16-byte accesses.
// Everything in this file, and every kernel that includes it, rests on this one fact: a change to it is made here.
//
// Vector stores and plain C++ only; no fast-math (build.py).

#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <new>

#include "mapf_step.h"

namespace mapf_nn {

constexpr int kActions = 5;  // moves per agent: every head, one-hot and action clamp
// the longest per-agent observation row: the widest sensor window, goal delta, two flags, the action mask
constexpr int kMaxObsLen = (2 * MAPF_MAX_SENSOR_RANGE + 1) * (2 * MAPF_MAX_SENSOR_RANGE + 1) + 2 + 1 + 1 + 5;

typedef float f32x16 __attribute__((ext_vector_type(16)));

// the feature a lane half supplies in chained k-step `st` (register st & 15 of accumulator tile st >> 4)
__device__ __forceinline__ int chained_feature(int st, int h) {
    const int r = st & 15;
    return 32 * (st >> 4) + (r & 3) + 8 * (r >> 2) + 4 * h;
}

// the inverse: accumulator register and lane half of feature kk (0 .. 31) of a tile
__device__ __forceinline__ int reg_of(int kk) { return (kk & 3) + 4 * (kk >> 3); }
__device__ __forceinline__ int half_of(int kk) { return (kk >> 2) & 1; }

// accumulator tile <-> 32 consecutive floats (a bias vector, a row of h or c): one 16-byte access per register group
__device__ __forceinline__ f32x16 load_tile(const float *p, int h) {
    f32x16 v;
#pragma unroll
    for (int g = 0; g < 4; g++) {
        const float4 x = *reinterpret_cast<const float4 *>(p + 8 * g + 4 * h);
        v[4 * g + 0] = x.x, v[4 * g + 1] = x.y, v[4 * g + 2] = x.z, v[4 * g + 3] = x.w;
    }
    return v;
}

__device__ __forceinline__ void store_tile(float *p, int h, const f32x16 &v) {
#pragma unroll
    for (int g = 0; g < 4; g++)
        *reinterpret_cast<float4 *>(p + 8 * g + 4 * h) = make_float4(v[4 * g + 0], v[4 * g + 1], v[4 * g + 2], v[4 * g + 3]);
}

__device__ __forceinline__ f32x16 zero_tile() {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = 0.f;
    return v;
}

// out[t] += W_t * in for NO output tiles; in = NI accumulator tiles taken as the B operand register by register.
// w: [16 * NI steps][NO][64 lanes]
template <int NO, int NI>
__device__ __forceinline__ void chain(f32x16 (&out)[NO], const f32x16 (&in)[NI], const float *__restrict__ w, int lane) {
#pragma unroll
    for (int st = 0; st < 16 * NI; st++) {
        const float b = in[st >> 4][st & 15];
#pragma unroll
        for (int t = 0; t < NO; t++) out[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[(st * NO + t) * 64 + lane], b, out[t], 0, 0, 0);
    }
}

__device__ __forceinline__ float sigmoidf(float x) { return 1.0f / (1.0f + expf(-x)); }

// ---- random numbers: splitmix64 ----------------------------------------------------------------------------------------
constexpr uint64_t kGolden = 0x9E3779B97F4A7C15ull;  // the stream's increment

__device__ __forceinline__ uint64_t mix64(uint64_t x) {  // the finalizer
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

// the top 24 bits as a uniform in (0, 1): 25 significant bits, so it is a double
__device__ __forceinline__ double uniform24(uint64_t x) { return ((double)(x >> 40) + 0.5) * (1.0 / 16777216.0); }

// ---- small reductions and selects ----------------------------------------------------------------------------------------
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

__device__ __forceinline__ uint64_t wave_sum(uint64_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o, 64);
    return v;
}

// x[a] as a chain of selects (an indexed read would put the array into scratch memory)
__device__ __forceinline__ float pick(const float x[kActions], int a) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < kActions; j++) r = a == j ? x[j] : r;
    return r;
}

__device__ __forceinline__ int clamp_action(int8_t a) { return a < 0 ? 0 : a > kActions - 1 ? kActions - 1 : (int)a; }

// ---- the packed weight buffer ------------------------------------------------------------------------------------------
// Each map takes the element index `e` inside its segment of the packed buffer (one dword per lane per k-step, as the A
// operand is read) and the tile count NT = hidden / 32, and returns the index inside the source matrix (row-major, as in
// the state_dict), or -1 where the packed element is zero padding.  The pack kernels of the units dispatch over their own
// layout structs and call these.

// P[base + i], or the zero of a padding element (i < 0)
__device__ __forceinline__ float pack_read(const float *__restrict__ P, int base, int i) { return i < 0 ? 0.f : P[base + i]; }

// fc1 [k-step][NT][lane] of W1[32 NT][F]: k-steps in natural order, lane half h takes input 2 s + h (padding past F)
__device__ __forceinline__ int pack_fc1(int e, int NT, int F) {
    const int lane = e & 63, mo = (e >> 6) % NT, s = (e >> 6) / NT, k = 2 * s + (lane >> 5);
    return k < F ? (32 * mo + (lane & 31)) * F + k : -1;
}

// a chained square product (fc2) [chained k-step][NT][lane] of W[32 NT][32 NT]
__device__ __forceinline__ int pack_chained(int e, int NT) {
    const int lane = e & 63, mo = (e >> 6) % NT, st = (e >> 6) / NT;
    return (32 * mo + (lane & 31)) * (32 * NT) + chained_feature(st, lane >> 5);
}

// LSTM input weights [hidden tile q][KS k-steps][gate][lane] of Wih[4 * 32 NT][ZIN]: 16 NT chained k-steps over a2, then
// the extra inputs in natural order (padding past ZIN)
__device__ __forceinline__ int pack_wih(int e, int NT, int KS, int ZIN) {
    const int HID = 32 * NT, CH = 16 * NT;
    const int lane = e & 63, g = (e >> 6) & 3, rest = e >> 8, s = rest % KS, q = rest / KS;
    const int row = HID * g + 32 * q + (lane & 31);
    const int k = s < CH ? chained_feature(s, lane >> 5) : HID + 2 * (s - CH) + (lane >> 5);
    return k < ZIN ? row * ZIN + k : -1;
}

// LSTM recurrent weights [hidden tile q][16 NT chained k-steps][gate][lane] of Whh[4 * 32 NT][32 NT]
__device__ __forceinline__ int pack_whh(int e, int NT) {
    const int HID = 32 * NT, CH = 16 * NT;
    const int lane = e & 63, g = (e >> 6) & 3, rest = e >> 8, s = rest % CH, q = rest / CH;
    return (HID * g + 32 * q + (lane & 31)) * HID + chained_feature(s, lane >> 5);
}

// head tiles [head tile][16 NT chained k-steps][lane]: outputs 0 .. A - 1 are rows of the [A][32 NT] matrix at `src_w`,
// output A is the [32 NT] vector at `src_v`, the rest of the last tile is padding.  Returns the index in the flat
// parameter vector (the two sources are different tensors).
__device__ __forceinline__ int pack_head(int e, int NT, int A, int src_w, int src_v) {
    const int CH = 16 * NT;
    const int lane = e & 63, st = (e >> 6) % CH, ht = (e >> 6) / CH;
    const int i = 32 * ht + (lane & 31), f = chained_feature(st, lane >> 5);
    return i < A ? src_w + i * (32 * NT) + f : i == A ? src_v + f : -1;
}

// the head biases, padded to whole tiles: outputs 0 .. A - 1 from `src_b`, output A from `src_vb`
__device__ __forceinline__ int pack_head_bias(int e, int A, int src_b, int src_vb) { return e < A ? src_b + e : e == A ? src_vb : -1; }

// ---- the host side of a network handle ---------------------------------------------------------------------------------
// A handle H is { cfg; l (the unit's layout: src_count, total); float *packed; bool params_set; }.  These are the bodies
// of mapf_<net>_create / _destroy / _param_count / _set_params after the unit's own checks of its config.

// the packed buffer on cfg.device (the caller's current device is left as it was): `sets` packed images of l.total floats,
// one behind the other (a handle with one weight set per agent; 1 everywhere else)
template <class H, class Cfg, class Layout>
int handle_create(const Cfg &cfg, const Layout &l, H **out, int sets = 1) {
    if (cfg.device < 0) return MAPF_ERR_CONFIG;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess) return MAPF_ERR_HIP;
    if (cfg.device >= ndev) return MAPF_ERR_CONFIG;
    H *p = new (std::nothrow) H;
    if (!p) return MAPF_ERR_HIP;
    p->cfg = cfg;
    p->l = l;
    int prev = 0;
    (void)hipGetDevice(&prev);
    const bool ok = hipSetDevice(cfg.device) == hipSuccess && hipMalloc((void **)&p->packed, (size_t)sets * (size_t)l.total * sizeof(float)) == hipSuccess;
    (void)hipSetDevice(prev);
    if (!ok) {
        delete p;
        return MAPF_ERR_HIP;
    }
    *out = p;
    return MAPF_OK;
}

template <class H>
int handle_destroy(H *p) {
    if (!p) return MAPF_ERR_CONFIG;
    if (p->packed) (void)hipFree(p->packed);
    delete p;
    return MAPF_OK;
}

template <class H>
int64_t handle_param_count(const H *p) {
    return p ? (int64_t)p->l.src_count : 0;
}

// pack: the unit's kernel (const float *params, float *packed, Layout), one thread per packed float; with `sets` > 1 the
// grid's y index is the weight set, params is [sets][src_count] and a kernel that supports it offsets both by blockIdx.y
template <class H, class Kernel>
int handle_set_params(H *p, const float *params, int64_t count, void *stream, Kernel pack, int sets = 1) {
    if (!p || !params || count != (int64_t)sets * (int64_t)p->l.src_count) return MAPF_ERR_CONFIG;
    const int threads = 256, blocks = (p->l.total + threads - 1) / threads;
    hipLaunchKernelGGL(pack, dim3(blocks, sets), dim3(threads), 0, (hipStream_t)stream, params, p->packed, p->l);
    if (hipGetLastError() != hipSuccess) return MAPF_ERR_HIP;
    p->params_set = true;
    return MAPF_OK;
}

}  // namespace mapf_nn
