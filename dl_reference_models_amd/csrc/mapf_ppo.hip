// mapf_ppo.hip -- the PPO objective of the learner on a minibatch: clipped surrogate, clipped value error, entropy, the
// KL penalty against the behaviour policy's logits, and their closed-form gradients with respect to the logits and the
// values in ONE launch (mapf_ppo_loss; include/mapf_step.h states the rule).
//
// Nothing here is sequential in t: every (t, row) is on its own, and only the gradient of a head needs a number of its whole
// row (g_logp, which hangs on the log-probability summed over the row's heads).  A workgroup of four wavefronts owns a tile
// of 32 rows OF ONE GROUP (rows g + groups * i: the interleaved agent rows of one policy) and walks t in chunks of 32 steps:
//   pass A  one thread per (t, row) of the chunk (1024 elements, four per thread): log-softmax of the row's heads in the
//           new and in the behaviour logits, logp, entropy, KL, ratio, the two clipped terms; logp, kl and dvalues go to
//           memory, g_logp to LDS (4 KB); with ONE head the thread has all its head's gradient needs and writes dlogits too
//   pass C  (more than one head) one thread per (t, row, head) -- consecutive threads write consecutive 20-byte groups of
//           dlogits: the head's two softmaxes again (the logits are in L2 from pass A) with g_logp read back from LDS
// What a thread computes and the order in which it sums depend on (t, row in tile) alone, never on `groups`: a group's
// outputs equal the groups = 1 call on its rows bit for bit.  No atomics: every thread sums the elements it owns in a fixed
// order, a wavefront reduces by shuffles, thread 0 adds the four wavefronts, and the sums leave as one partial per
// workgroup.  kl_coeff is read from device memory, and so are, through mapf_ppo_loss_hp, the clip bounds and coefficients of
// the workgroup's group.  Vector stores and plain C++ only, fp32 throughout, libm-grade exp / log,
// no fast-math (build.py).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // kActions, clamp_action, wave_sum

constexpr int kRows = 32;   // rows per workgroup
constexpr int kChunk = 32;  // steps per chunk (MAPF_PPO_CHUNK)
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kElems = kRows * kChunk;
constexpr int NA = kActions;  // actions per head

static_assert(kRows == MAPF_PPO_TILE_ROWS, "mapf_step.h states the tile");
static_assert(kChunk == MAPF_PPO_CHUNK, "mapf_step.h states the chunk");
static_assert(kRows == 32, "element index = 32 * step + row below");

struct Args {
    const float *logits, *old_logits;
    const int8_t *actions;
    const float *old_logp, *adv, *values, *targets, *kl_coeff;
    float *logp, *kl, *dlogits, *dvalues, *partials;
    float lo, hi, vf_clip, vf_coeff, ent_coeff, scale;
    int32_t T, rows, heads, groups, tiles;  // tiles: per group
    const float *hp;  // mapf_ppo_loss_hp: [groups][4] clip, vf_clip, vf_coeff, ent_coeff in place of the scalars above
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

// log-softmax of one head of the behaviour logits and its KL to the head lp: sum_j q (lq - lp), 0 where q underflowed to 0
__device__ __forceinline__ float head_kl(const float *__restrict__ x, const float lp[NA], float q[NA]) {
    float lq[NA];
    (void)head_log_softmax(x, lq);
    float kl = 0.f;
#pragma unroll
    for (int j = 0; j < NA; j++) {
        q[j] = expf(lq[j]);
        kl += q[j] > 0.f ? q[j] * (lq[j] - lp[j]) : 0.f;
    }
    return kl;
}

// lp[a] as a sum of selects (an indexed read of lp would put the array into scratch memory), as k_vtrace_loss has it
__device__ __forceinline__ float pick_sum(const float lp[NA], int a) {
    float r = 0.f;
#pragma unroll
    for (int j = 0; j < NA; j++) r += a == j ? lp[j] : 0.f;
    return r;
}

// the gradient of one head: c [ -g_logp (1[j = a] - p) + ent_coeff p (lp + H) + kl_coeff (p - q) ]
__device__ __forceinline__ void head_grad(float ent_coeff, float scale, float *__restrict__ out, const float lp[NA], float H,
                                          const float q[NA], int act, float gl, float klc, bool has_kl) {
#pragma unroll
    for (int j = 0; j < NA; j++) {
        const float p = expf(lp[j]);
        const float ent = p > 0.f ? ent_coeff * p * (lp[j] + H) : 0.f;
        float d = ent - gl * ((act == j ? 1.f : 0.f) - p);
        if (has_kl) d += klc * (p - q[j]);
        out[j] = d * scale;
    }
}

// HP = false: clip bounds and coefficients are the launch's scalars (mapf_ppo_loss: the code of the kernel before the
// per-group values existed).  HP = true: the workgroup reads its group's four values where it reads kl_coeff[g] and forms
// lo / hi as the host does for the scalars; below that the two are the same code on the same values, so a group's results
// are those of the scalar call with its values, bit for bit.
template <bool HP>
__global__ __launch_bounds__(kThreads) void k_ppo_loss(Args a) {
    __shared__ float s_g[kElems];  // g_logp of the chunk
    __shared__ float s_part[kWaves][4];

    const int tid = threadIdx.x;
    const int g = (int)blockIdx.x / a.tiles, tile = (int)blockIdx.x - g * a.tiles;
    const int64_t rows = a.rows, heads = a.heads, G = a.groups;
    const int r0 = tile * kRows, grows = a.rows / a.groups;               // the tile's first row IN its group, the group's rows
    const int vrows = grows - r0 < kRows ? grows - r0 : kRows;             // >= 1: tiles = ceil(grows / kRows)
    const bool has_kl = a.kl_coeff != nullptr;
    const float klc = has_kl ? a.kl_coeff[g] : 0.f;
    const bool one_head = a.heads == 1;
    float lo = a.lo, hi = a.hi, vf_clip = a.vf_clip, vf_coeff = a.vf_coeff, ent_coeff = a.ent_coeff;
    if constexpr (HP) {
        const float *hp = a.hp + 4 * g;  // uniform over the workgroup
        const float clip = hp[0];
        lo = (float)(1.0 - (double)clip), hi = (float)(1.0 + (double)clip);
        vf_clip = hp[1], vf_coeff = hp[2], ent_coeff = hp[3];
    }

    float sum_pol = 0.f, sum_vf = 0.f, sum_ent = 0.f, sum_kl = 0.f;

    for (int t0 = 0; t0 < a.T; t0 += kChunk) {
        const int nT = a.T - t0 < kChunk ? a.T - t0 : kChunk;

        // pass A
        for (int e = tid; e < nT * kRows; e += kThreads) {
            const int rl = e & (kRows - 1);
            if (rl >= vrows) continue;
            const int64_t at = (int64_t)(t0 + (e >> 5)) * rows + g + G * (r0 + rl);
            const float *x = a.logits + at * heads * NA;
            const float *xo = has_kl ? a.old_logits + at * heads * NA : nullptr;  // (not read without a coefficient)
            const int8_t *ac = a.actions + at * heads;
            float lp[NA], q[NA];
            float logp = 0.f, H = 0.f, KL = 0.f, Hk = 0.f;
            int act = 0;
            for (int k = 0; k < a.heads; k++) {
                Hk = head_log_softmax(x + k * NA, lp);
                act = clamp_action(ac[k]);
                H += Hk;
                logp += pick_sum(lp, act);
                if (has_kl) KL += head_kl(xo + k * NA, lp, q);
            }
            const float A = a.adv[at];
            const float w = expf(logp - a.old_logp[at]);  // +inf when it overflows: the clamp then gives 1 + clip
            const float ar = A * w, acl = A * fminf(fmaxf(w, lo), hi);
            const bool open = ar <= acl;  // the unclipped term is the minimum (a tie included): the gradient flows
            const float s = open ? ar : acl, gl = open ? ar : 0.f;
            const float d = a.values[at] - a.targets[at], err = d * d;
            const bool vopen = err <= vf_clip;
            s_g[e] = gl;
            if (a.logp) a.logp[at] = logp;
            if (a.kl) a.kl[at] = KL;
            if (a.dvalues) a.dvalues[at] = vopen ? (vf_coeff * 2.f * d) * a.scale : 0.f;
            if (one_head && a.dlogits) head_grad(ent_coeff, a.scale, a.dlogits + at * NA, lp, Hk, q, act, gl, klc, has_kl);
            sum_pol -= s;
            sum_vf += vopen ? err : vf_clip;
            sum_ent += H;
            sum_kl += KL;
        }

        // pass C
        if (!one_head && a.dlogits) {
            __syncthreads();
            const int per = vrows * a.heads, total = nT * per;
            for (int e = tid; e < total; e += kThreads) {
                const int tl = e / per, qq = e - tl * per;
                const int rl = qq / a.heads, k = qq - rl * a.heads;
                const int64_t at = (int64_t)(t0 + tl) * rows + g + G * (r0 + rl);
                const int64_t hd = at * heads + k;
                float lp[NA], q[NA];
                const float H = head_log_softmax(a.logits + hd * NA, lp);
                if (has_kl) (void)head_kl(a.old_logits + hd * NA, lp, q);
                head_grad(ent_coeff, a.scale, a.dlogits + hd * NA, lp, H, q, clamp_action(a.actions[hd]), s_g[tl * kRows + rl], klc,
                          has_kl);
            }
            __syncthreads();  // the next chunk's pass A overwrites what pass C read
        }
    }

    if (!a.partials) return;
    sum_pol = wave_sum(sum_pol), sum_vf = wave_sum(sum_vf), sum_ent = wave_sum(sum_ent), sum_kl = wave_sum(sum_kl);
    if ((tid & 63) == 0) {
        float *w = s_part[tid >> 6];
        w[0] = sum_pol, w[1] = sum_vf, w[2] = sum_ent, w[3] = sum_kl;
    }
    __syncthreads();
    if (tid == 0) {
        float p = s_part[0][0], v = s_part[0][1], h = s_part[0][2], k = s_part[0][3];
        for (int w = 1; w < kWaves; w++) p += s_part[w][0], v += s_part[w][1], h += s_part[w][2], k += s_part[w][3];
        float *out = a.partials + (int64_t)blockIdx.x * 5;
        out[0] = p, out[1] = v, out[2] = h, out[3] = k;
        out[4] = p + vf_coeff * v - ent_coeff * h + klc * k;  // this tile's share of its group's total * (T rows / groups)
    }
}

bool scalar_ok(float x) { return isfinite(x) && x >= 0.f; }

}  // namespace

extern "C" {

int32_t mapf_ppo_partials(int32_t rows, int32_t groups) {
    if (rows < 1 || groups < 1 || rows % groups) return 0;
    return (int32_t)((int64_t)groups * ((rows / groups + kRows - 1) / kRows));
}

int mapf_ppo_loss_hp(int32_t T, int32_t rows, int32_t heads, int32_t groups, const float *logits, const float *old_logits,
                     const int8_t *actions, const float *old_logp, const float *adv, const float *values, const float *targets,
                     float clip, float vf_clip, float vf_coeff, float ent_coeff, const float *kl_coeff, const float *hp, float *logp,
                     float *kl, float *dlogits, float *dvalues, float *partials, void *stream) {
    if (T < 1 || rows < 1 || heads < 1 || heads > MAPF_PPO_MAX_HEADS || groups < 1 || rows % groups) return MAPF_ERR_CONFIG;
    if (!logits || !actions || !old_logp || !adv || !values || !targets || (kl_coeff && !old_logits)) return MAPF_ERR_CONFIG;
    // (with hp the scalars are not read, and the host cannot see hp: its ranges are the caller's duty)
    if (!hp && (!scalar_ok(clip) || !scalar_ok(vf_clip) || !scalar_ok(vf_coeff) || !scalar_ok(ent_coeff) || clip >= 1.f)) return MAPF_ERR_CONFIG;
    Args a{};
    a.logits = logits, a.old_logits = kl_coeff ? old_logits : nullptr, a.actions = actions, a.old_logp = old_logp, a.adv = adv;
    a.values = values, a.targets = targets, a.kl_coeff = kl_coeff;
    a.logp = logp, a.kl = kl, a.dlogits = dlogits, a.dvalues = dvalues, a.partials = partials;
    a.lo = (float)(1.0 - (double)clip), a.hi = (float)(1.0 + (double)clip);
    a.vf_clip = vf_clip, a.vf_coeff = vf_coeff, a.ent_coeff = ent_coeff;
    a.scale = 1.0f / ((float)T * (float)(rows / groups));  // = groups / (T rows): every group has the same count
    a.T = T, a.rows = rows, a.heads = heads, a.groups = groups, a.tiles = (rows / groups + kRows - 1) / kRows;
    a.hp = hp;
    const dim3 grid((uint32_t)mapf_ppo_partials(rows, groups));
    if (hp)
        hipLaunchKernelGGL(k_ppo_loss<true>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k_ppo_loss<false>, grid, dim3(kThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int mapf_ppo_loss(int32_t T, int32_t rows, int32_t heads, int32_t groups, const float *logits, const float *old_logits,
                  const int8_t *actions, const float *old_logp, const float *adv, const float *values, const float *targets,
                  float clip, float vf_clip, float vf_coeff, float ent_coeff, const float *kl_coeff, float *logp, float *kl,
                  float *dlogits, float *dvalues, float *partials, void *stream) {
    return mapf_ppo_loss_hp(T, rows, heads, groups, logits, old_logits, actions, old_logp, adv, values, targets, clip, vf_clip,
                            vf_coeff, ent_coeff, kl_coeff, nullptr, logp, kl, dlogits, dvalues, partials, stream);
}

}  // extern "C"
