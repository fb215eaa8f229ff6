// mapf_policy_joint.hip -- the joint-action policy of libmapfstep.so (mapf_jpolicy_*; include/mapf_step.h states the rule).
//
// One launch takes every env row of the single-agent env from its full-grid observation to the N actions of its agents,
// their summed log-probability, the value and the new LSTM state.  The products are those of mapf_policy.hip: TRANSPOSED
// on the f32-input MFMA (v_mfma_f32_32x32x2_f32), D[out feature][row] = sum_k W[out][k] X^T[k][row], with the row on the
// lane and the output features in the 16 accumulator registers, so that an accumulator tile IS the B operand of the next
// product when its k-steps are taken register by register (chained_feature), and mapf_jpolicy_set_params packs every
// matrix as the A operand is read.  What differs from mapf_policy.hip is the size of three of the products: fc1 has up to
// 4 096 inputs, the LSTM input up to 321 extra entries, the heads up to 321 outputs.  So a 32-row tile belongs to a
// WORKGROUP of four wavefronts, one per SIMD, and the work of the tile is spread over them:
//   fc1    the observation tile is staged through LDS in chunks of 256 floats (two buffers, and the loads of chunk c + 1
//          are in flight in registers while chunk c is multiplied); each wave takes a quarter of a chunk's k-steps, and
//          the four partial accumulators are summed through LDS in wave order by every wave (all then hold the same a1)
//   fc2    64 MFMAs, in every wave (a split would need a second reduction for 48 MFMAs saved)
//   gates  wave w owns hidden-unit tile q = w & 1 and one half of the K range: w < 2 the a2 part and the first half of
//          the extra k-steps, w >= 2 the h part and the rest; the upper pair hands its four gate tiles over through LDS.
//          The B operand of an extra k-step is formed in registers from the row's previous-action bytes (kept in LDS)
//   heads  ceil((5N + 1) / 32) output tiles, dealt round-robin to the waves, written to LDS as [row][output]
//   epilogue  one thread per (row, agent) decision: mask, argmax / Gumbel-max, log-softmax; a row's log-probability is
//          summed in agent order by one thread, so the result does not depend on the schedule
// THE WIDE NET (hidden = MAPF_JPOLICY_HIDDEN_WIDE = 256, feed-forward: the reference's CTE IMPALA model) has a kernel of its
// own, k_jpolicy_act_wide, behind the same entry points.  256 outputs are eight accumulator tiles, too many to keep whole
// in every wave and to sum through LDS, so there the OUTPUT FEATURES are split and nothing is reduced across waves:
//   fc1    wave w owns output tiles 2 w and 2 w + 1; the observation chunks are staged as above and every wave walks all
//          k-steps of a chunk against its own quarter of W1; bias (the accumulator's start) and tanh in registers; the two
//          tiles go to LDS as a1[k][row], so that the B operand of k-step s of the next product is 64 consecutive floats
//   fc2    128 k-steps x 2 tiles per wave from a1 in LDS, a2 to LDS the same way
//   heads  output tiles round-robin over the waves, K = 256 from a2 in LDS; the epilogue is the one above
// The weights of 16 k-steps are loaded into registers while the 16 before them are multiplied (walk).  The K orders are
// natural (k-step s holds inputs 2 s and 2 s + 1), and fc1's k-steps are padded with zero weights to whole groups of 16.
// Every reduction has a fixed order: two calls on the same input are bitwise equal.
// Vector stores and plain C++ only.  fp32 operands, fp32 accumulation, correctly rounded division, libm-grade tanh / exp /
// log: no fast-math (build.py).  The Gumbel noise is evaluated in double, as in mapf_policy.hip.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // the accumulator layout and its helpers, the packing index maps, the handle's host side

constexpr int kTile = 32;      // env rows per workgroup (the MFMA's N)
constexpr int kWaves = 4;      // one per SIMD
constexpr int kThreads = 64 * kWaves;
constexpr int HID = MAPF_POLICY_HIDDEN;
constexpr int NT = HID / 32, CH = HID / 2;
constexpr int kChunk = 256;                     // floats of a row staged per fc1 chunk
constexpr int kChunkStride = kChunk + 1;        // odd: lanes of different rows read different banks
constexpr int kStageFloats = kTile * kChunkStride;
constexpr int kMaxHeadTiles = (kActions * MAPF_JPOLICY_MAX_AGENTS + 1 + 31) / 32;  // 11
constexpr int kPaStride = MAPF_JPOLICY_MAX_AGENTS + 4;                            // bytes; 17 dwords: odd
constexpr int kLpStride = MAPF_JPOLICY_MAX_AGENTS + 1;

static_assert(HID == 64, "the wave roles below are written for two hidden-unit tiles");
static_assert(kTile * (32 * kMaxHeadTiles + 1) <= 2 * kStageFloats, "the head outputs reuse the staging buffers");
static_assert(kWaves * NT * 16 * 64 <= kStageFloats && NT * 4 * 16 * 64 <= kStageFloats, "so do the two hand-overs");

// the wide net: 8 output tiles, 2 per wave; k-steps are walked in groups of 16
constexpr int WHID = MAPF_JPOLICY_HIDDEN_WIDE;
constexpr int WNT = WHID / 32, WCH = WHID / 2, kOwn = WNT / kWaves, kWalk = 16;
constexpr int kActFloats = WHID * kTile;                    // a1 or a2 of a tile as [k][row]
constexpr int kHeadFloats = kTile * (32 * kMaxHeadTiles + 1);
// one LDS array (floats): [0, 2 kStageFloats) the fc1 chunks, then a1.  a2 takes the place of the first chunk buffer once
// fc1 is done; the head outputs and the per-decision log-probabilities follow a2, over the second chunk buffer and a1,
// which are both dead by then.
constexpr int kWideA1 = 2 * kStageFloats, kWideA2 = 0, kWideHead = kWideA2 + kActFloats, kWideLp = kWideHead + kHeadFloats;
constexpr int kWideFloats = kWideA1 + kActFloats;
static_assert(WNT == kOwn * kWaves && WCH % kWalk == 0 && (kChunk / 2) % kWalk == 0, "whole tiles per wave, whole groups per chunk");
static_assert(kActFloats <= kStageFloats, "a2 lies inside the first chunk buffer");
static_assert(kWideLp + kTile * kLpStride <= kWideFloats, "the heads and the log-probabilities fit behind a2");
static_assert(kWideFloats * sizeof(float) <= 160 * 1024, "the LDS of a gfx950 CU");

// where everything lies: `src_*` in the flat parameter vector (state_dict order), the rest in the packed buffer (floats)
struct JointLayout {
    int32_t F, S1;   // grid cells, k-steps of fc1
    int32_t N, A;    // agents, A = 5 N logits
    int32_t XS, HT;  // extra k-steps of the LSTM input ([onehot5 x N, prev_reward], padded to K = 2), head output tiles
    int32_t recurrent;
    int32_t src_fc1w, src_fc1b, src_fc2w, src_fc2b, src_wih, src_whh, src_bih, src_bhh, src_piw, src_pib, src_vfw, src_vfb;
    int32_t src_count;
    int32_t w1, b1, w2, b2, wih, whh, bl, wh, bh, total;
};

// hidden: MAPF_POLICY_HIDDEN, or WHID (feed-forward only), where fc1's k-steps are padded to whole groups of kWalk
JointLayout make_layout(int F, int N, int recurrent, int hidden) {
    const int H = hidden, T = H / 32, C = H / 2, G = 4 * H;
    JointLayout l{};
    l.F = F, l.S1 = (F + 1) / 2;
    if (H == WHID) l.S1 = (l.S1 + kWalk - 1) / kWalk * kWalk;
    l.N = N, l.A = kActions * N;
    l.XS = (l.A + 1 + 1) / 2, l.HT = (l.A + 1 + 31) / 32;
    l.recurrent = recurrent;
    const int ZIN = H + l.A + 1;
    int o = 0;
    l.src_fc1w = o, o += H * F;
    l.src_fc1b = o, o += H;
    l.src_fc2w = o, o += H * H;
    l.src_fc2b = o, o += H;
    if (recurrent) {
        l.src_wih = o, o += G * ZIN;
        l.src_whh = o, o += G * H;
        l.src_bih = o, o += G;
        l.src_bhh = o, o += G;
    }
    l.src_piw = o, o += l.A * H;
    l.src_pib = o, o += l.A;
    l.src_vfw = o, o += H;
    l.src_vfb = o, o += 1;
    l.src_count = o;
    o = 0;
    l.w1 = o, o += l.S1 * T * 64;
    l.b1 = o, o += H;
    l.w2 = o, o += C * T * 64;
    l.b2 = o, o += H;
    if (recurrent) {
        l.wih = o, o += T * (C + l.XS) * 4 * 64;
        l.whh = o, o += T * C * 4 * 64;
        l.bl = o, o += G;
    }
    l.wh = o, o += l.HT * C * 64;
    l.bh = o, o += l.HT * 32;
    l.total = o;
    return l;
}

// one thread per packed float: zero-padded to the MFMA's K and to whole output tiles, gate biases summed (bih + bhh)
__global__ __launch_bounds__(256) void k_jpolicy_pack(const float *__restrict__ P, float *__restrict__ out, JointLayout l) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= l.total) return;
    const int ZIN = HID + l.A + 1, KS = CH + l.XS;
    float v;
    if (t < l.b1) v = pack_read(P, l.src_fc1w, pack_fc1(t - l.w1, NT, l.F));
    else if (t < l.w2) v = P[l.src_fc1b + (t - l.b1)];
    else if (t < l.b2) v = pack_read(P, l.src_fc2w, pack_chained(t - l.w2, NT));
    else if (t < (l.recurrent ? l.wih : l.wh)) v = P[l.src_fc2b + (t - l.b2)];
    else if (l.recurrent && t < l.whh) v = pack_read(P, l.src_wih, pack_wih(t - l.wih, NT, KS, ZIN));
    else if (l.recurrent && t < l.bl) v = pack_read(P, l.src_whh, pack_whh(t - l.whh, NT));
    else if (l.recurrent && t < l.wh) v = P[l.src_bih + (t - l.bl)] + P[l.src_bhh + (t - l.bl)];
    else if (t < l.bh) v = pack_read(P, 0, pack_head(t - l.wh, NT, l.A, l.src_piw, l.src_vfw));  // output 5N is the value
    else v = pack_read(P, 0, pack_head_bias(t - l.bh, l.A, l.src_pib, l.src_vfb));
    out[t] = v;
}

// head tiles of the wide net [head tile][k-step][lane] in natural K order (pack_head's is the chained one): lane half h
// takes input 2 s + h of output 32 ht + (lane & 31); the index in the flat parameter vector, -1 for padding
__device__ __forceinline__ int pack_head_natural(int e, int H, int A, int src_w, int src_v) {
    const int lane = e & 63, s = (e >> 6) % (H / 2), ht = (e >> 6) / (H / 2);
    const int i = 32 * ht + (lane & 31), k = 2 * s + (lane >> 5);
    return i < A ? src_w + i * H + k : i == A ? src_v + k : -1;
}

// the same for the wide net: fc1 [S1 padded k-steps][8][lane], fc2 [128 k-steps][8][lane] (pack_fc1 with F = 256: fc2 reads
// a1 from LDS in natural order), the heads as above
__global__ __launch_bounds__(256) void k_jpolicy_pack_wide(const float *__restrict__ P, float *__restrict__ out, JointLayout l) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= l.total) return;
    float v;
    if (t < l.b1) v = pack_read(P, l.src_fc1w, pack_fc1(t - l.w1, WNT, l.F));
    else if (t < l.w2) v = P[l.src_fc1b + (t - l.b1)];
    else if (t < l.b2) v = pack_read(P, l.src_fc2w, pack_fc1(t - l.w2, WNT, WHID));
    else if (t < l.wh) v = P[l.src_fc2b + (t - l.b2)];
    else if (t < l.bh) v = pack_read(P, 0, pack_head_natural(t - l.wh, WHID, l.A, l.src_piw, l.src_vfw));
    else v = pack_read(P, 0, pack_head_bias(t - l.bh, l.A, l.src_pib, l.src_vfb));
    out[t] = v;
}

struct JointArgs {
    const float *packed;
    const float *obs;
    const int8_t *prev_action;
    const double *prev_reward;
    const uint8_t *start_a, *start_b;
    float *hstate, *cstate;
    uint32_t *draws;
    uint64_t seed;
    int8_t *action;
    float *logp, *value, *logits;
    int32_t rows, mode;
    JointLayout l;
};

// accumulator tiles through LDS, register-major: p[r * 64 + lane] (conflict-free)
__device__ __forceinline__ void lds_put(float *p, int lane, const f32x16 &v) {
#pragma unroll
    for (int r = 0; r < 16; r++) p[r * 64 + lane] = v[r];
}

__device__ __forceinline__ f32x16 lds_get(const float *p, int lane) {
    f32x16 v;
#pragma unroll
    for (int r = 0; r < 16; r++) v[r] = p[r * 64 + lane];
    return v;
}

// chunk c of the tile's observation rows, in two halves so that the loads are in flight while the chunk before is
// multiplied: wave w fetches rows 8 w .. 8 w + 7, a lane columns lane, lane + 64, ... of the chunk (256 bytes per load
// instruction), into registers, and puts them into a staging buffer afterwards.  Zero past F and past the last row, so
// nothing outside obs[rows][L] is read and the K tail of fc1 never comes from memory.
constexpr int kFetchRows = kTile / kWaves, kFetchCols = kChunk / 64;
static_assert(kFetchRows * kFetchCols == kTile, "32 floats per thread and chunk");

__device__ __forceinline__ void fetch_chunk(float (&v)[kTile], const float *__restrict__ src, int L, int F, int nrow, int c, int w, int lane) {
#pragma unroll
    for (int rr = 0; rr < kFetchRows; rr++) {
        const int r = w * kFetchRows + rr;
#pragma unroll
        for (int i = 0; i < kFetchCols; i++) {
            const int k = c * kChunk + 64 * i + lane;
            v[rr * kFetchCols + i] = (k < F && r < nrow) ? src[r * L + k] : 0.f;  // (32 rows of at most 4 416 floats)
        }
    }
}

__device__ __forceinline__ void put_chunk(float *buf, const float (&v)[kTile], int w, int lane) {
#pragma unroll
    for (int rr = 0; rr < kFetchRows; rr++)
#pragma unroll
        for (int i = 0; i < kFetchCols; i++) buf[(w * kFetchRows + rr) * kChunkStride + 64 * i + lane] = v[rr * kFetchCols + i];
}

// ---- epilogue: one thread per (row, agent) decision -------------------------------------------------------------------
// hd: the head outputs of the tile in LDS as [row][HS]; lp_s: kTile * kLpStride floats of LDS.  Every wave has arrived.
__device__ __forceinline__ void decide(const JointArgs &a, const float *hd, int HS, float *lp_s, int64_t row0, int nrow, int tid) {
    const int F = a.l.F, N = a.l.N, A = a.l.A, L = F + A;
    const bool sample = a.mode & MAPF_POLICY_SAMPLE;
    for (int d = tid; d < nrow * N; d += kThreads) {
        const int r = d / N, ag = d - r * N;
        const int64_t rr = row0 + r;
        const float *m = a.obs + rr * L + F + ag * kActions;
        float lg[kActions];
#pragma unroll
        for (int k = 0; k < kActions; k++) lg[k] = hd[r * HS + ag * kActions + k] + logf(m[k] + 1e-6f);
        int act = 0;
        if (sample) {
            const uint64_t x = mix64(a.seed ^ (((uint64_t)rr << 32) | a.draws[rr]));
            double best = 0.0;
#pragma unroll
            for (int k = 0; k < kActions; k++) {
                const uint64_t xk = mix64(x + (uint64_t)(ag * kActions + k + 1) * kGolden);
                const double uk = uniform24(xk);
                const double s = (double)lg[k] - log(-log(uk));
                if (k == 0 || s > best) best = s, act = k;
            }
        } else {
#pragma unroll
            for (int k = 1; k < kActions; k++)
                if (lg[k] > lg[act]) act = k;
        }
        a.action[rr * N + ag] = (int8_t)act;
        if (a.logp) {
            float mx = lg[0];
#pragma unroll
            for (int k = 1; k < kActions; k++) mx = fmaxf(mx, lg[k]);
            float sum = 0.f;
#pragma unroll
            for (int k = 0; k < kActions; k++) sum += expf(lg[k] - mx);
            lp_s[r * kLpStride + ag] = lg[act] - (mx + logf(sum));
        }
        if (a.logits) {
#pragma unroll
            for (int k = 0; k < kActions; k++) a.logits[rr * A + ag * kActions + k] = lg[k];
        }
    }
    __syncthreads();  // every decision of a row has read its draw counter and left its log-probability
    if (tid < nrow) {
        const int64_t rr = row0 + tid;
        if (a.logp) {
            float s = 0.f;
            for (int ag = 0; ag < N; ag++) s += lp_s[tid * kLpStride + ag];
            a.logp[rr] = s;
        }
        if (a.value) a.value[rr] = hd[tid * HS + A];
        if (sample && !(a.mode & MAPF_POLICY_PEEK)) a.draws[rr] = a.draws[rr] + 1u;
    }
}

template <bool REC>
__global__ __launch_bounds__(kThreads) void k_jpolicy_act(JointArgs a) {
    __shared__ __attribute__((aligned(16))) float stage[2 * kStageFloats];  // fc1 chunks; later the hand-overs and the heads
    __shared__ __attribute__((aligned(16))) float u_s[NT * 16 * 64];          // h' in accumulator layout, for the heads
    __shared__ float lp_s[kTile * kLpStride];                                 // per-decision log-probabilities
    __shared__ int8_t pa_s[kTile * kPaStride];                                // previous actions of the tile's rows

    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = a.l.F, N = a.l.N, A = a.l.A, L = F + A;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    const int nrow = (int)min((int64_t)kTile, (int64_t)a.rows - row0);
    const int64_t row = row0 + j;
    const bool valid = j < nrow;
    const float *P = a.packed;
    const float *src = a.obs + row0 * L;

    bool keep = false;  // the row exists and carries its state over
    if constexpr (REC) {
        if (valid) keep = !((a.start_a && a.start_a[row]) || (a.start_b && a.start_b[row]));
        // previous actions of the tile: 0 where the row starts an episode, where there is no row, and without prev_action
        for (int i = tid; i < kTile * N; i += kThreads) {
            const int r = i / N, ag = i - r * N;
            int8_t v = 0;
            if (r < nrow && a.prev_action) {
                const int64_t rr = row0 + r;
                const bool st = (a.start_a && a.start_a[rr]) || (a.start_b && a.start_b[rr]);
                if (!st) v = a.prev_action[rr * N + ag];
            }
            pa_s[r * kPaStride + ag] = v;
        }
    }

    // ---- a1 = tanh(W1 x + b1): split K over the waves, chunk by chunk ----------------------------------------------
    f32x16 a1[NT], a2[NT];
#pragma unroll
    for (int m = 0; m < NT; m++) a1[m] = zero_tile();
    const int nchunk = (F + kChunk - 1) / kChunk;
    float pre[kTile];
    fetch_chunk(pre, src, L, F, nrow, 0, w, lane);
    put_chunk(stage, pre, w, lane);
    __syncthreads();
    for (int c = 0; c < nchunk; c++) {
        const float *buf = stage + (c & 1) * kStageFloats;
        const bool more = c + 1 < nchunk;
        if (more) fetch_chunk(pre, src, L, F, nrow, c + 1, w, lane);
        constexpr int SW = kChunk / 2 / kWaves;  // k-steps of a chunk per wave
        const int s0 = c * (kChunk / 2) + w * SW;
        const int ns = min(SW, a.l.S1 - s0);
        const float *w1 = P + a.l.w1 + (int64_t)s0 * NT * 64 + lane;
        const float *x = buf + j * kChunkStride + 2 * w * SW + h;
        if (ns == SW) {  // a whole quarter: unrolled, so that the weight loads run ahead of the products
#pragma unroll
            for (int s = 0; s < SW; s++) {
                const float b = x[2 * s];
#pragma unroll
                for (int m = 0; m < NT; m++) a1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[(s * NT + m) * 64], b, a1[m], 0, 0, 0);
            }
        } else {
            for (int s = 0; s < ns; s++) {
                const float b = x[2 * s];
#pragma unroll
                for (int m = 0; m < NT; m++) a1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[(s * NT + m) * 64], b, a1[m], 0, 0, 0);
            }
        }
        if (more) put_chunk(stage + ((c + 1) & 1) * kStageFloats, pre, w, lane);
        __syncthreads();  // chunk c is consumed, chunk c + 1 is staged
    }
    {
        float *red = stage;  // [wave][tile][register][lane]
#pragma unroll
        for (int m = 0; m < NT; m++) lds_put(red + (w * NT + m) * 1024, lane, a1[m]);
        __syncthreads();
#pragma unroll
        for (int m = 0; m < NT; m++) {
            a1[m] = load_tile(P + a.l.b1 + 32 * m, h);
#pragma unroll
            for (int ww = 0; ww < kWaves; ww++) {
                const f32x16 part = lds_get(red + (ww * NT + m) * 1024, lane);
#pragma unroll
                for (int r = 0; r < 16; r++) a1[m][r] += part[r];
            }
#pragma unroll
            for (int r = 0; r < 16; r++) a1[m][r] = tanhf(a1[m][r]);
        }
    }

    // ---- a2 = tanh(W2 a1 + b2), in every wave -------------------------------------------------------------------------
#pragma unroll
    for (int m = 0; m < NT; m++) a2[m] = load_tile(P + a.l.b2 + 32 * m, h);
    chain<NT, NT>(a2, a1, P + a.l.w2, lane);
#pragma unroll
    for (int m = 0; m < NT; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) a2[m][r] = tanhf(a2[m][r]);

    f32x16 u[NT];
    if constexpr (REC) {
        // ---- gates of hidden-unit tile q: the lower wave pair takes [a2, first extras], the upper pair [h, the rest] ----
        const int q = w & 1, upper = w >> 1;
        const int KS = CH + a.l.XS;
        const float *wih = P + a.l.wih + (int64_t)q * KS * 256;
        float *hand = stage + kStageFloats;  // [q][gate][register][lane]; the a1 partials are still being read in stage[0]
        f32x16 gate[4];
        const int xmid = a.l.XS / 2;
        int e0, e1;
        if (upper) {
            f32x16 hold[NT];
#pragma unroll
            for (int m = 0; m < NT; m++) hold[m] = keep ? load_tile(a.hstate + row * HID + 32 * m, h) : zero_tile();
#pragma unroll
            for (int g = 0; g < 4; g++) gate[g] = zero_tile();
            chain<4, NT>(gate, hold, P + a.l.whh + (int64_t)q * CH * 256, lane);
            e0 = xmid, e1 = a.l.XS;
        } else {
#pragma unroll
            for (int g = 0; g < 4; g++) gate[g] = load_tile(P + a.l.bl + HID * g + 32 * q, h);
            chain<4, NT>(gate, a2, wih, lane);
            e0 = 0, e1 = xmid;
        }
        float pr = 0.f;
        if (keep && a.prev_reward) pr = (float)a.prev_reward[row];  // round to nearest
        const int8_t *pa = pa_s + j * kPaStride;
#pragma unroll 4
        for (int e = e0; e < e1; e++) {
            // entry 2 e + h of [onehot5(prev_action[0]), ..., onehot5(prev_action[N - 1]), prev_reward]
            const int idx = 2 * e + h;
            float b = 0.f;
            if (idx < A) {
                const int ag = idx / kActions;
                b = (int)pa[ag] == idx - ag * kActions ? 1.f : 0.f;
            } else if (idx == A) {
                b = pr;
            }
            const float *wx = wih + (int64_t)(CH + e) * 256 + lane;
#pragma unroll
            for (int g = 0; g < 4; g++) gate[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(wx[g * 64], b, gate[g], 0, 0, 0);
        }
        if (upper) {
#pragma unroll
            for (int g = 0; g < 4; g++) lds_put(hand + (q * 4 + g) * 1024, lane, gate[g]);
        }
        __syncthreads();
        if (!upper) {
            const f32x16 cold = keep ? load_tile(a.cstate + row * HID + 32 * q, h) : zero_tile();
#pragma unroll
            for (int g = 0; g < 4; g++) {
                const f32x16 part = lds_get(hand + (q * 4 + g) * 1024, lane);
#pragma unroll
                for (int r = 0; r < 16; r++) gate[g][r] += part[r];
            }
            f32x16 cnew, hnew;
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float c1 = sigmoidf(gate[1][r]) * cold[r] + sigmoidf(gate[0][r]) * tanhf(gate[2][r]);
                cnew[r] = c1;
                hnew[r] = sigmoidf(gate[3][r]) * tanhf(c1);
            }
            lds_put(u_s + q * 1024, lane, hnew);
            if (valid && !(a.mode & MAPF_POLICY_PEEK)) {
                store_tile(a.hstate + row * HID + 32 * q, h, hnew);
                store_tile(a.cstate + row * HID + 32 * q, h, cnew);
            }
        }
        __syncthreads();
#pragma unroll
        for (int m = 0; m < NT; m++) u[m] = lds_get(u_s + m * 1024, lane);
    } else {
#pragma unroll
        for (int m = 0; m < NT; m++) u[m] = a2[m];
        __syncthreads();  // every wave has read the a1 partials: the staging buffers are free for the heads
    }

    // ---- heads: output tiles round-robin over the waves, into LDS as [row][output] ---------------------------------
    const int HS = 32 * a.l.HT + 1;
    float *hd = stage;
    for (int ht = w; ht < a.l.HT; ht += kWaves) {
        f32x16 head[1];
        head[0] = load_tile(P + a.l.bh + 32 * ht, h);
        chain<1, NT>(head, u, P + a.l.wh + (int64_t)ht * CH * 64, lane);
#pragma unroll
        for (int r = 0; r < 16; r++) hd[j * HS + 32 * ht + (r & 3) + 8 * (r >> 2) + 4 * h] = head[0][r];
    }
    __syncthreads();

    decide(a, hd, HS, lp_s, row0, nrow, tid);
}

// ---- the wide net ---------------------------------------------------------------------------------------------------------
// acc[t] += W_s b_s over `groups` groups of kWalk k-steps.  The A dword of step s and tile t is wp[(s * WS + t) * 64] (wp
// already points at the lane's dword), the B dword x[s * XS] (LDS).  The operands of group g + 1 are loaded while group g
// is multiplied, in two register sets that change roles (no copy, so no product waits for the loads of the next group);
// behind the last group the last one is loaded once more, which keeps the loop free of a branch and stays inside the matrix.
template <int NO>
struct WalkGroup {
    float w[kWalk * NO], b[kWalk];
};

template <int NO, int WS, int XS>
__device__ __forceinline__ void load_group(WalkGroup<NO> &v, const float *__restrict__ wp, const float *x, int g) {
    const float *wg = wp + (int64_t)g * kWalk * WS * 64, *xg = x + g * kWalk * XS;
#pragma unroll
    for (int i = 0; i < kWalk; i++)
#pragma unroll
        for (int t = 0; t < NO; t++) v.w[i * NO + t] = wg[(i * WS + t) * 64];
#pragma unroll
    for (int i = 0; i < kWalk; i++) v.b[i] = xg[i * XS];
    __builtin_amdgcn_sched_barrier(0);  // issued here: before the products that follow, not behind them
}

template <int NO>
__device__ __forceinline__ void mult_group(f32x16 (&acc)[NO], const WalkGroup<NO> &v) {
#pragma unroll
    for (int i = 0; i < kWalk; i++)
#pragma unroll
        for (int t = 0; t < NO; t++) acc[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(v.w[i * NO + t], v.b[i], acc[t], 0, 0, 0);
    __builtin_amdgcn_sched_barrier(0);
}

template <int NO, int WS, int XS>
__device__ __forceinline__ void walk(f32x16 (&acc)[NO], const float *__restrict__ wp, const float *x, int groups) {
    WalkGroup<NO> even, odd;
    load_group<NO, WS, XS>(even, wp, x, 0);
    int g = 0;
    for (; g + 2 <= groups; g += 2) {
        load_group<NO, WS, XS>(odd, wp, x, g + 1);
        mult_group<NO>(acc, even);
        load_group<NO, WS, XS>(even, wp, x, min(g + 2, groups - 1));
        mult_group<NO>(acc, odd);
    }
    if (g < groups) mult_group<NO>(acc, even);
}

// tanh of the wave's tiles, then into LDS as act[feature][row]: the B operand of k-step s of the next product is then
// act[64 s + lane]
__device__ __forceinline__ void put_activation(float *act, f32x16 (&v)[kOwn], int w, int j, int h) {
#pragma unroll
    for (int t = 0; t < kOwn; t++)
#pragma unroll
        for (int r = 0; r < 16; r++) act[(32 * (kOwn * w + t) + (r & 3) + 8 * (r >> 2) + 4 * h) * kTile + j] = tanhf(v[t][r]);
}

__global__ __launch_bounds__(kThreads) void k_jpolicy_act_wide(JointArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[kWideFloats];
    float *stage = lds, *a1 = lds + kWideA1, *a2 = lds + kWideA2, *hd = lds + kWideHead, *lp_s = lds + kWideLp;

    const int tid = threadIdx.x, lane = tid & 63, j = lane & 31, h = lane >> 5;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int F = a.l.F, L = F + a.l.A;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    const int nrow = (int)min((int64_t)kTile, (int64_t)a.rows - row0);
    const float *P = a.packed;
    const float *src = a.obs + row0 * L;

    // ---- a1 = tanh(W1 x + b1): the wave's two output tiles over all of K, chunk by chunk ------------------------------
    f32x16 acc[kOwn];
#pragma unroll
    for (int t = 0; t < kOwn; t++) acc[t] = load_tile(P + a.l.b1 + 32 * (kOwn * w + t), h);
    const int nchunk = (F + kChunk - 1) / kChunk;
    constexpr int GC = kChunk / 2 / kWalk;  // groups of k-steps per chunk
    const int groups = a.l.S1 / kWalk;
    float pre[kTile];
    fetch_chunk(pre, src, L, F, nrow, 0, w, lane);
    put_chunk(stage, pre, w, lane);
    __syncthreads();
    for (int c = 0; c < nchunk; c++) {
        const float *buf = stage + (c & 1) * kStageFloats;
        const bool more = c + 1 < nchunk;
        if (more) fetch_chunk(pre, src, L, F, nrow, c + 1, w, lane);
        walk<kOwn, WNT, 2>(acc, P + a.l.w1 + ((int64_t)c * (kChunk / 2) * WNT + kOwn * w) * 64 + lane, buf + j * kChunkStride + h,
                           min(GC, groups - c * GC));
        if (more) put_chunk(stage + ((c + 1) & 1) * kStageFloats, pre, w, lane);
        __syncthreads();  // chunk c is consumed, chunk c + 1 is staged
    }
    put_activation(a1, acc, w, j, h);
    __syncthreads();

    // ---- a2 = tanh(W2 a1 + b2); it overwrites the first chunk buffer, which every wave has left ---------------------
#pragma unroll
    for (int t = 0; t < kOwn; t++) acc[t] = load_tile(P + a.l.b2 + 32 * (kOwn * w + t), h);
    walk<kOwn, WNT, 64>(acc, P + a.l.w2 + kOwn * w * 64 + lane, a1 + lane, WCH / kWalk);
    put_activation(a2, acc, w, j, h);
    __syncthreads();  // a2 is whole, and a1 and the second chunk buffer are free for the heads

    // ---- heads: output tiles round-robin over the waves, into LDS as [row][output] ---------------------------------
    const int HS = 32 * a.l.HT + 1;
    for (int ht = w; ht < a.l.HT; ht += kWaves) {
        f32x16 head[1];
        head[0] = load_tile(P + a.l.bh + 32 * ht, h);
        walk<1, 1, 64>(head, P + a.l.wh + (int64_t)ht * WCH * 64 + lane, a2 + lane, WCH / kWalk);
#pragma unroll
        for (int r = 0; r < 16; r++) hd[j * HS + 32 * ht + (r & 3) + 8 * (r >> 2) + 4 * h] = head[0][r];
    }
    __syncthreads();

    decide(a, hd, HS, lp_s, row0, nrow, tid);
}

}  // namespace

struct mapf_jpolicy {
    mapf_jpolicy_config cfg;
    JointLayout l;
    float *packed = nullptr;
    bool params_set = false;
};

extern "C" {

int mapf_jpolicy_create(const mapf_jpolicy_config *cfg, mapf_jpolicy_handle *out) {
    if (!cfg || !out) return MAPF_ERR_CONFIG;
    *out = nullptr;
    if (cfg->hidden != MAPF_POLICY_HIDDEN && cfg->hidden != WHID) return MAPF_ERR_CONFIG;
    if (cfg->grid_cells < 1 || cfg->grid_cells > MAPF_JPOLICY_MAX_CELLS) return MAPF_ERR_CONFIG;
    if (cfg->num_agents < 1 || cfg->num_agents > MAPF_JPOLICY_MAX_AGENTS) return MAPF_ERR_CONFIG;
    if (cfg->recurrent != 0 && cfg->recurrent != 1) return MAPF_ERR_CONFIG;
    if (cfg->hidden == WHID && cfg->recurrent) return MAPF_ERR_CONFIG;  // the wide net is feed-forward only
    return handle_create(*cfg, make_layout(cfg->grid_cells, cfg->num_agents, cfg->recurrent, cfg->hidden), out);
}

int mapf_jpolicy_destroy(mapf_jpolicy_handle p) { return handle_destroy(p); }

int64_t mapf_jpolicy_param_count(mapf_jpolicy_handle p) { return handle_param_count(p); }

int mapf_jpolicy_set_params(mapf_jpolicy_handle p, const float *params, int64_t count, void *stream) {
    return handle_set_params(p, params, count, stream, p && p->cfg.hidden == WHID ? k_jpolicy_pack_wide : k_jpolicy_pack);
}

int mapf_jpolicy_act(mapf_jpolicy_handle p, int32_t rows, const float *obs, const int8_t *prev_action, const double *prev_reward,
                     const uint8_t *start_a, const uint8_t *start_b, float *hstate, float *cstate, uint32_t *draws, uint64_t seed,
                     int32_t mode, int8_t *action, float *logp, float *value, float *logits, void *stream) {
    if (!p || !obs || !action) return MAPF_ERR_CONFIG;
    if (p->cfg.recurrent && (!hstate || !cstate)) return MAPF_ERR_CONFIG;
    if (mode & ~(MAPF_POLICY_SAMPLE | MAPF_POLICY_PEEK)) return MAPF_ERR_CONFIG;
    if ((mode & MAPF_POLICY_SAMPLE) && !draws) return MAPF_ERR_CONFIG;
    if (rows < 1) return MAPF_ERR_CONFIG;
    if (!p->params_set) return MAPF_ERR_STATE;
    JointArgs a{};
    a.packed = p->packed, a.obs = obs, a.prev_action = prev_action, a.prev_reward = prev_reward;
    a.start_a = start_a, a.start_b = start_b, a.hstate = hstate, a.cstate = cstate, a.draws = draws, a.seed = seed;
    a.action = action, a.logp = logp, a.value = value, a.logits = logits;
    a.rows = rows, a.mode = mode;
    a.l = p->l;
    const dim3 grid((uint32_t)(((int64_t)rows + kTile - 1) / kTile)), block(kThreads);
    if (p->cfg.hidden == WHID)
        hipLaunchKernelGGL(k_jpolicy_act_wide, grid, block, 0, (hipStream_t)stream, a);
    else if (p->cfg.recurrent)
        hipLaunchKernelGGL((k_jpolicy_act<true>), grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL((k_jpolicy_act<false>), grid, block, 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
