// mapf_bc.hip -- the behaviour-cloning objective of the learner on a minibatch: the negative log-likelihood of the expert's
// actions, an optional value regression, an optional entropy bonus, the share of heads whose argmax is the expert's action,
// and the closed-form gradients with respect to the logits and the values in ONE launch (mapf_bc_loss; include/mapf_step.h
// states the rule).
//
// The layout is k_ppo_loss's (csrc/mapf_ppo.hip): a workgroup of four wavefronts owns a tile of 32 rows OF ONE GROUP (rows
// g + groups * i: the interleaved agent rows of one policy) and walks t in chunks of 32 steps with nothing carried between
// the chunks.  Unlike PPO's, the gradient of a head needs no number of the rest of its row, so nothing goes through LDS
// between the passes:
//   pass A  one thread per (t, row) of the chunk (1024 elements, four per thread): log-softmax of the row's heads, nll,
//           entropy, hits and the value error; nll and dvalues go to memory; with ONE head the thread writes dlogits too
//   pass C  (more than one head) one thread per (t, row, head) -- consecutive threads write consecutive 20-byte groups of
//           dlogits: the head's softmax again (the logits are in L2 from pass A)
// What a thread computes and the order in which it sums depend on (t, row in tile) alone, never on `groups`: a group's
// outputs equal the groups = 1 call on its rows bit for bit.  No atomics: every thread sums the elements it owns in a fixed
// order, a wavefront reduces by shuffles, thread 0 adds the four wavefronts, and the sums leave as one partial per
// workgroup.  Vector stores and plain C++ only, fp32 throughout, libm-grade exp / log, no fast-math (build.py).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // kActions, clamp_action, wave_sum

constexpr int kRows = 32;   // rows per workgroup
constexpr int kChunk = 32;  // steps per chunk (MAPF_BC_CHUNK)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int NA = kActions;  // actions per head

static_assert(kRows == MAPF_BC_TILE_ROWS, "mapf_step.h states the tile");
static_assert(kChunk == MAPF_BC_CHUNK, "mapf_step.h states the chunk");
static_assert(kRows == 32, "element index = 32 * step + row below");

struct Args {
    const float *logits;
    const int8_t *expert;
    const float *values, *targets;
    float *nll, *dlogits, *dvalues, *partials;
    float vf_coeff, ent_coeff, scale;
    int32_t T, rows, heads, groups, tiles;  // tiles: per group
};

// log-softmax of one head; returns the head's entropy (a probability that underflowed to 0 contributes 0, never 0 * inf)
// and the index of its largest logit, the lowest on ties: a comparison of the inputs, no arithmetic
__device__ __forceinline__ float head_log_softmax(const float *__restrict__ x, float lp[NA], int &top) {
    float v[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) v[j] = x[j];
    float m = v[0];
    top = 0;
#pragma unroll
    for (int j = 1; j < NA; j++) {
        top = v[j] > m ? j : top;
        m = v[j] > m ? v[j] : m;
    }
    float s = 0.f;
#pragma unroll
    for (int j = 0; j < NA; j++) s += expf(v[j] - m);
    const float ls = logf(s);
    float H = 0.f;
#pragma unroll
    for (int j = 0; j < NA; j++) {
        lp[j] = (v[j] - m) - ls;
        const float p = expf(lp[j]);
        H -= p > 0.f ? p * lp[j] : 0.f;
    }
    return H;
}

// lp[a] as a sum of selects (an indexed read of lp would put the array into scratch memory), as k_vtrace_loss has it
__device__ __forceinline__ float pick_sum(const float lp[NA], int a) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < NA; j++) r += a == j ? lp[j] : 0.f;
    return r;
}

// the gradient of one head: c [ (p - 1[j = e]) + ent_coeff p (lp + H) ]
__device__ __forceinline__ void head_grad(const Args &a, float *__restrict__ out, const float lp[NA], float H, int e) {
#pragma unroll
    for (int j = 0; j < NA; j++) {
        const float p = expf(lp[j]);
        const float ent = p > 0.f ? a.ent_coeff * p * (lp[j] + H) : 0.f;
        out[j] = ((p - (e == j ? 1.f : 0.f)) + ent) * a.scale;
    }
}

__global__ __launch_bounds__(kThreads) void k_bc_loss(Args a) {
    __shared__ float s_part[kWaves][4];

    const int tid = threadIdx.x;
    const int g = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - g * a.tiles;
    const int64_t rows = a.rows, heads = a.heads, G = a.groups;
    const int r0 = tile * kRows, grows = a.rows / a.groups;    // the tile's first row IN its group, the group's rows
    const int vrows = grows - r0 < kRows ? grows - r0 : kRows;  // >= 1: tiles = ceil(grows / kRows)
    const bool has_v = a.values != nullptr;
    const bool one_head = a.heads == 1;

    float sum_nll = 0.f, sum_vf = 0.f, sum_ent = 0.f, sum_hit = 0.f;

    for (int t0 = 0; t0 < a.T; t0 += kChunk) {
        const int nT = a.T - t0 < kChunk ? a.T - t0 : kChunk;

        // pass A
        for (int e = tid; e < nT * kRows; e += kThreads) {
            const int rl = e & (kRows - 1);
            if (rl >= vrows) continue;
            const int64_t at = (int64_t)(t0 + (e >> 5)) * rows + g + G * (r0 + rl);
            const float *x = a.logits + at * heads * NA;
            const int8_t *ex = a.expert + at * heads;
            float lp[NA];
            float nll = 0.f, H = 0.f, Hk = 0.f;
            int hits = 0, act = 0, top = 0;
            for (int k = 0; k < a.heads; k++) {
                Hk = head_log_softmax(x + k * NA, lp, top);
                act = clamp_action(ex[k]);
                H += Hk;
                nll -= pick_sum(lp, act);
                hits += top == act ? 1 : 0;
            }
            float v = 0.f;
            if (has_v) {
                const float d = a.values[at] - a.targets[at];
                v = 0.5f * d * d;
                if (a.dvalues) a.dvalues[at] = (a.vf_coeff * d) * a.scale;
            }
            if (a.nll) a.nll[at] = nll;
            if (one_head && a.dlogits) head_grad(a, a.dlogits + at * NA, lp, Hk, act);
            sum_nll += nll;
            sum_vf += v;
            sum_ent += H;
            sum_hit += (float)hits;
        }

        // pass C
        if (!one_head && a.dlogits) {
            const int per = vrows * a.heads, total = nT * per;
            for (int e = tid; e < total; e += kThreads) {
                const int tl = e / per, qq = e - tl * per;
                const int rl = qq / a.heads, k = qq - rl * a.heads;
                const int64_t at = (int64_t)(t0 + tl) * rows + g + G * (r0 + rl);
                const int64_t hd = at * heads + k;
                float lp[NA];
                int top;
                const float H = head_log_softmax(a.logits + hd * NA, lp, top);
                head_grad(a, a.dlogits + hd * NA, lp, H, clamp_action(a.expert[hd]));
            }
        }
    }

    if (!a.partials) return;
    sum_nll = wave_sum(sum_nll), sum_vf = wave_sum(sum_vf), sum_ent = wave_sum(sum_ent), sum_hit = wave_sum(sum_hit);
    if ((tid & 63) == 0) {
        float *w = s_part[tid >> 6];
        w[0] = sum_nll, w[1] = sum_vf, w[2] = sum_ent, w[3] = sum_hit;
    }
    __syncthreads();
    if (tid == 0) {
        float n = s_part[0][0], v = s_part[0][1], h = s_part[0][2], c = s_part[0][3];
        for (int w = 1; w < kWaves; w++) n += s_part[w][0], v += s_part[w][1], h += s_part[w][2], c += s_part[w][3];
        float *out = a.partials + (int64_t)blockIdx.x * 5;
        out[0] = n, out[1] = v, out[2] = h, out[3] = c;
        out[4] = n + a.vf_coeff * v - a.ent_coeff * h;  // this tile's share of its group's total * (T rows / groups)
    }
}

bool scalar_ok(float x) { return isfinite(x) && x >= 0.f; }

}  // namespace

extern "C" {

int32_t mapf_bc_partials(int32_t rows, int32_t groups) {
    if (rows < 1 || groups < 1 || rows % groups) return 0;
    return (int32_t)((int64_t)groups * ((rows / groups + kRows - 1) / kRows));
}

int mapf_bc_loss(int32_t T, int32_t rows, int32_t heads, int32_t groups, const float *logits, const int8_t *expert,
                 const float *values, const float *targets, float vf_coeff, float ent_coeff, float *nll, float *dlogits,
                 float *dvalues, float *partials, void *stream) {
    if (T < 1 || rows < 1 || heads < 1 || heads > MAPF_BC_MAX_HEADS || groups < 1 || rows % groups) return MAPF_ERR_CONFIG;
    if (!logits || !expert || (values == nullptr) != (targets == nullptr) || (dvalues && !values)) return MAPF_ERR_CONFIG;
    if (!scalar_ok(vf_coeff) || !scalar_ok(ent_coeff)) return MAPF_ERR_CONFIG;
    Args a{};
    a.logits = logits, a.expert = expert, a.values = values, a.targets = targets;
    a.nll = nll, a.dlogits = dlogits, a.dvalues = dvalues, a.partials = partials;
    a.vf_coeff = vf_coeff, a.ent_coeff = ent_coeff;
    a.scale = 1.0f / ((float)T * (float)(rows / groups));  // = groups / (T rows): every group has the same count
    a.T = T, a.rows = rows, a.heads = heads, a.groups = groups, a.tiles = (rows / groups + kRows - 1) / kRows;
    hipLaunchKernelGGL(k_bc_loss, dim3((uint32_t)mapf_bc_partials(rows, groups)), dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
