// mapf_vtrace.hip -- the IMPALA objective of the learner on a fragment: V-trace targets, the three loss terms and their
// closed-form gradients with respect to the logits and the values in ONE launch (mapf_vtrace_loss; include/mapf_step.h
// states the rule).
//
// Only the V-trace recursion is sequential in t; the log-softmax, the taken log-probability, the entropy, the importance
// weight and the gradient of every (t, row, head) do not depend on it.  A workgroup of four wavefronts owns a tile of 32
// rows and walks t from the end in chunks of 32 steps:
//   pass A  all waves, one thread per (t, row) of the chunk (1024 elements, four per thread): log-softmax of the row's
//           heads, logp, entropy, w and the three clipped weights; the per-(t, row) scalars go to LDS (25 KB)
//   scan    lanes 0 .. 31 of wave 0, one row each: the backward recursion over the chunk out of LDS, acc / V[t+1] / vs[t+1]
//           carried in registers from chunk to chunk (so LDS does not grow with T); vs and pg_adv go back to LDS
//   pass B  all waves, one thread per (t, row): vs, pg_adv, logp, dvalues to memory, the policy and value sums
//   pass C  all waves, one thread per (t, row, head) -- consecutive threads write consecutive 20-byte groups of dlogits:
//           the head's softmax again (its logits are in L2 from pass A) with pg_adv read back from LDS
// A tile of 32 rows rather than 64 puts a minibatch of 1 024 rows on 32 workgroups (128 wavefronts) instead of 16, and a
// 32-step chunk takes the reference's max_seq_len in one piece; a [t][rows] access of a tile is one 128-byte segment.
// No atomics: every thread sums the elements it owns in a fixed order, a wavefront reduces by shuffles, thread 0 adds the
// four wavefronts, and the sums leave as one partial per workgroup.  Vector stores and plain C++ only, fp32 throughout,
// libm-grade exp / log, no fast-math (build.py).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // kActions, clamp_action, wave_sum

constexpr int kRows = 32;    // rows per workgroup
constexpr int kChunk = 32;   // steps per chunk (MAPF_VTRACE_CHUNK)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kElems = kRows * kChunk;
constexpr int NA = kActions;  // actions per head

static_assert(kChunk == MAPF_VTRACE_CHUNK && kRows == MAPF_VTRACE_TILE_ROWS, "mapf_step.h states the tile");
static_assert(kRows == 32, "element index = 32 * step + row below");

struct Args {
    const float *logits;
    const int8_t *actions;
    const float *mu, *values, *rewards;
    const uint8_t *ended;
    const float *boot;
    float *vs, *pg_adv, *logp, *dlogits, *dvalues, *partials;
    float gamma, lam, clip_rho, clip_c, clip_pg_rho, vf_coeff, ent_coeff, inv_count;
    int32_t T, rows, heads;
};

// log-softmax of one head; returns the head's entropy (a probability that underflowed to 0 contributes 0, never 0 * inf)
__device__ __forceinline__ float head_log_softmax(const float *__restrict__ x, float lp[NA]) {
    float v[NA];
#pragma unroll
    for (int j = 0; j < NA; j++) v[j] = x[j];
    float m = v[0];
#pragma unroll
    for (int j = 1; j < NA; j++) m = fmaxf(m, v[j]);
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

// lp[a] as a SUM of selects (an indexed read of lp would put the array into scratch memory).  mapf_nn.h's pick is a chain
// of selects: other instructions (and -0 where this sum gives +0), so this kernel keeps the form it was measured with
__device__ __forceinline__ float pick_sum(const float lp[NA], int a) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < NA; j++) r += a == j ? lp[j] : 0.f;
    return r;
}

__global__ __launch_bounds__(kThreads) void k_vtrace_loss(Args a) {
    __shared__ float s_rho[kElems];   // rho, after the scan vs
    __shared__ float s_rpg[kElems];   // rho_pg, after the scan pg_adv
    __shared__ float s_c[kElems], s_r[kElems], s_v[kElems], s_logp[kElems];
    __shared__ uint8_t s_end[kElems];
    __shared__ float s_part[kWaves][3];

    const int tid = threadIdx.x;
    const int64_t rows = a.rows, heads = a.heads;
    const int64_t row0 = (int64_t)blockIdx.x * kRows;
    const int vrows = rows - row0 < kRows ? (int)(rows - row0) : kRows;  // >= 1: the grid is ceil(rows / kRows)

    float sum_pol = 0.f, sum_vf = 0.f, sum_ent = 0.f;
    float acc = 0.f, next_v = 0.f, next_vs = 0.f;  // the scan's carry (threads 0 .. vrows - 1)
    if (tid < vrows) next_v = next_vs = a.boot[row0 + tid];

    for (int t1 = a.T; t1 > 0; t1 -= kChunk) {
        const int t0 = t1 > kChunk ? t1 - kChunk : 0, nT = t1 - t0;

        // pass A
        for (int e = tid; e < nT * kRows; e += kThreads) {
            const int rl = e & (kRows - 1);
            if (rl >= vrows) continue;
            const int64_t at = (int64_t)(t0 + (e >> 5)) * rows + row0 + rl;
            const float *x = a.logits + at * heads * NA;
            const int8_t *ac = a.actions + at * heads;
            float logp = 0.f, H = 0.f;
            for (int k = 0; k < a.heads; k++) {
                float lp[NA];
                H += head_log_softmax(x + k * NA, lp);
                logp += pick_sum(lp, clamp_action(ac[k]));
            }
            const float w = expf(logp - a.mu[at]);  // +inf when it overflows: min() then gives the threshold
            s_rho[e] = fminf(a.clip_rho, w);
            s_c[e] = a.lam * fminf(a.clip_c, w);
            s_rpg[e] = fminf(a.clip_pg_rho, w);
            s_r[e] = a.rewards[at];
            s_v[e] = a.values[at];
            s_end[e] = a.ended[at];
            s_logp[e] = logp;
            sum_ent += H;
        }
        __syncthreads();

        // scan: an episode end cuts the bootstrap and the recursion (selected, not multiplied by 0)
        if (tid < vrows) {
            for (int tl = nT - 1; tl >= 0; tl--) {
                const int e = tl * kRows + tid;
                const float v = s_v[e], r = s_r[e];
                const bool end = s_end[e] != 0;
                const float delta = s_rho[e] * ((end ? r : r + a.gamma * next_v) - v);
                acc = end ? delta : delta + a.gamma * s_c[e] * acc;
                const float vs = v + acc;
                s_rpg[e] = s_rpg[e] * ((end ? r : r + a.gamma * next_vs) - v);
                s_rho[e] = vs;
                next_v = v, next_vs = vs;
            }
        }
        __syncthreads();

        // pass B
        for (int e = tid; e < nT * kRows; e += kThreads) {
            const int rl = e & (kRows - 1);
            if (rl >= vrows) continue;
            const int64_t at = (int64_t)(t0 + (e >> 5)) * rows + row0 + rl;
            const float vs = s_rho[e], pg = s_rpg[e], lp = s_logp[e], d = s_v[e] - vs;
            a.vs[at] = vs;
            a.pg_adv[at] = pg;
            if (a.logp) a.logp[at] = lp;
            if (a.dvalues) a.dvalues[at] = a.vf_coeff * d * a.inv_count;
            sum_pol -= pg * lp;
            sum_vf += 0.5f * d * d;
        }

        // pass C
        if (a.dlogits) {
            const int per = vrows * a.heads, total = nT * per;
            for (int e = tid; e < total; e += kThreads) {
                const int tl = e / per, q = e - tl * per;
                const int rl = q / a.heads;
                const int64_t at = (int64_t)(t0 + tl) * rows + row0;  // the tile's first row at this step
                const int64_t hd = at * heads + q;                     // = (at + rl) * heads + head
                float lp[NA];
                const float H = head_log_softmax(a.logits + hd * NA, lp);
                const int act = clamp_action(a.actions[hd]);
                const float pg = s_rpg[tl * kRows + rl];
                float *out = a.dlogits + hd * NA;
#pragma unroll
                for (int j = 0; j < NA; j++) {
                    const float p = expf(lp[j]);
                    const float ent = p > 0.f ? a.ent_coeff * p * (lp[j] + H) : 0.f;
                    out[j] = (ent - pg * ((act == j ? 1.f : 0.f) - p)) * a.inv_count;
                }
            }
        }
        __syncthreads();  // the next chunk's pass A overwrites what passes B and C read
    }

    if (!a.partials) return;
    sum_pol = wave_sum(sum_pol), sum_vf = wave_sum(sum_vf), sum_ent = wave_sum(sum_ent);
    if ((tid & 63) == 0) s_part[tid >> 6][0] = sum_pol, s_part[tid >> 6][1] = sum_vf, s_part[tid >> 6][2] = sum_ent;
    __syncthreads();
    if (tid == 0) {
        float p = s_part[0][0], v = s_part[0][1], h = s_part[0][2];
        for (int w = 1; w < kWaves; w++) p += s_part[w][0], v += s_part[w][1], h += s_part[w][2];
        float *out = a.partials + (int64_t)blockIdx.x * 4;
        out[0] = p, out[1] = v, out[2] = h;
        out[3] = p + a.vf_coeff * v - a.ent_coeff * h;  // this workgroup's share of total_loss * (T rows)
    }
}

bool scalar_ok(float x) { return isfinite(x) && x >= 0.f; }

}  // namespace

extern "C" {

int32_t mapf_vtrace_partials(int32_t rows) { return rows < 1 ? 0 : (int32_t)(((int64_t)rows + kRows - 1) / kRows); }

int mapf_vtrace_loss(int32_t T, int32_t rows, int32_t heads, const float *logits, const int8_t *actions,
                     const float *behaviour_logp, const float *values, const float *rewards, const uint8_t *ended,
                     const float *bootstrap, float gamma, float lam, float clip_rho, float clip_c, float clip_pg_rho,
                     float vf_coeff, float ent_coeff, float *vs, float *pg_adv, float *logp, float *dlogits, float *dvalues,
                     float *partials, void *stream) {
    if (T < 1 || rows < 1 || heads < 1 || heads > MAPF_VTRACE_MAX_HEADS) return MAPF_ERR_CONFIG;
    if (!logits || !actions || !behaviour_logp || !values || !rewards || !ended || !bootstrap || !vs || !pg_adv) return MAPF_ERR_CONFIG;
    if (!scalar_ok(gamma) || !scalar_ok(lam) || !scalar_ok(clip_rho) || !scalar_ok(clip_c) || !scalar_ok(clip_pg_rho) ||
        !scalar_ok(vf_coeff) || !scalar_ok(ent_coeff) || gamma > 1.f || lam > 1.f)
        return MAPF_ERR_CONFIG;
    Args a{};
    a.logits = logits, a.actions = actions, a.mu = behaviour_logp, a.values = values, a.rewards = rewards, a.ended = ended;
    a.boot = bootstrap, a.vs = vs, a.pg_adv = pg_adv, a.logp = logp, a.dlogits = dlogits, a.dvalues = dvalues, a.partials = partials;
    a.gamma = gamma, a.lam = lam, a.clip_rho = clip_rho, a.clip_c = clip_c, a.clip_pg_rho = clip_pg_rho;
    a.vf_coeff = vf_coeff, a.ent_coeff = ent_coeff, a.inv_count = 1.0f / ((float)T * (float)rows);
    a.T = T, a.rows = rows, a.heads = heads;
    hipLaunchKernelGGL(k_vtrace_loss, dim3((uint32_t)mapf_vtrace_partials(rows)), dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
