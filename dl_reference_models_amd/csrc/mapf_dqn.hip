// mapf_dqn.hip -- what DQN needs on the device (include/mapf_step.h, "DQN", states the rules):
//   mapf_qnet_*          the dueling 32-32 Q-network, observation to epsilon-greedy action in one launch per step
//   mapf_replay_sample   stratified prioritised sampling from integer weights, three launches
//   mapf_dqn_td_loss     the double-Q Huber objective, its gradient and the new priorities in one launch
//
// k_qnet_act is the feed-forward half of mapf_policy.hip at a hidden width of 32: a wavefront owns a tile of 32 rows and
// computes every product transposed on v_mfma_f32_32x32x2_f32, D[out feature][row] = sum_k W[out][k] X^T[k][row].  With 32
// hidden units every layer is ONE accumulator tile, whose register r of lane half h holds feature (r & 3) + 8 (r >> 2) + 4 h;
// taken register by register that is the B operand of the next product, and mapf_qnet_set_params packs the weights so that
// the A dword of the same lane in the same k-step is the weight of exactly that feature: fc1 -> fc2 -> heads chain in
// registers.  The five advantages and the value are rows 0 .. 5 of one head tile.  LDS holds the wave's 32 x L observation
// tile; the packed weights (at most 25 KB) are read as 256-byte rows, one dword per lane per MFMA, each exactly once per
// wavefront, so staging them in LDS would add a copy without a second reader.
//
// The sampler works on chunks of 256 weights: k_replay_sums (a wavefront per chunk: its sum and its count of non-zero
// weights), k_replay_scan (one workgroup: inclusive prefix over the chunk sums, W, n_valid, the draw counter), and
// k_replay_search (a wavefront per sample: binary search over the chunk prefix, then a wave scan inside the chunk).  All
// sums are 64-bit integers, so the result does not depend on the order of summation.
//
// k_dqn_td owns one sample per thread; a wavefront reduces by shuffles, thread 0 adds the four wavefronts: no atomics, a
// fixed order, one partial per workgroup.  Vector stores and plain C++ only, no fast-math (build.py).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // the accumulator layout and its helpers, the packing index maps, the handle's host side

constexpr int kTile = 32;     // rows per wavefront (the MFMA's N)
constexpr int kWave = 64;
constexpr int kAhead = 8;     // k-steps of fc1 whose operands are in flight together
constexpr int HID = MAPF_QNET_HIDDEN;
constexpr int NA = kActions;
static_assert(HID == 32, "one accumulator tile per layer");

// ---------------------------------------------------------------------------------------------------------------------
// Q-network
// ---------------------------------------------------------------------------------------------------------------------

// where everything lies: `src_*` in the flat parameter vector (state_dict order), the rest in the packed buffer (floats)
struct QLayout {
    int32_t L, S1;  // features, k-steps of fc1 (L rounded up to the MFMA's K = 2)
    int32_t src_fc1w, src_fc1b, src_fc2w, src_fc2b, src_advw, src_advb, src_valw, src_valb, src_count;
    int32_t w1, b1, w2, b2, wh, bh, total;
};

QLayout make_layout(int L) {
    QLayout l{};
    l.L = L;
    l.S1 = (L + 1) / 2;
    int o = 0;
    l.src_fc1w = o, o += HID * L;
    l.src_fc1b = o, o += HID;
    l.src_fc2w = o, o += HID * HID;
    l.src_fc2b = o, o += HID;
    l.src_advw = o, o += NA * HID;
    l.src_advb = o, o += NA;
    l.src_valw = o, o += HID;
    l.src_valb = o, o += 1;
    l.src_count = o;
    o = 0;
    l.w1 = o, o += l.S1 * kWave;
    l.b1 = o, o += HID;
    l.w2 = o, o += (HID / 2) * kWave;
    l.b2 = o, o += HID;
    l.wh = o, o += (HID / 2) * kWave;
    l.bh = o, o += 32;
    l.total = o;
    return l;
}

// one thread per packed float, zero-padded to the MFMA's K
__global__ __launch_bounds__(256) void k_qnet_pack(const float *__restrict__ P, float *__restrict__ out, QLayout l) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= l.total) return;
    float v;
    if (t < l.b1) v = pack_read(P, l.src_fc1w, pack_fc1(t - l.w1, 1, l.L));
    else if (t < l.w2) v = P[l.src_fc1b + (t - l.b1)];
    else if (t < l.b2) v = pack_read(P, l.src_fc2w, pack_chained(t - l.w2, 1));
    else if (t < l.wh) v = P[l.src_fc2b + (t - l.b2)];
    else if (t < l.bh) v = pack_read(P, 0, pack_head(t - l.wh, 1, NA, l.src_advw, l.src_valw));  // output 5 is the value
    else v = pack_read(P, 0, pack_head_bias(t - l.bh, NA, l.src_advb, l.src_valb));
    out[t] = v;
}

struct QActArgs {
    const float *packed;
    const float *obs;
    const float *epsilon;
    uint32_t *draws;
    uint64_t seed;
    int8_t *action;
    float *q;
    int32_t rows, mode;
    QLayout l;
};

__global__ __launch_bounds__(kWave) void k_qnet_act(QActArgs a) {
    extern __shared__ __attribute__((aligned(16))) float tile[];  // [kTile][L]: the wave's observation rows
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int L = a.l.L;
    const int64_t row0 = (int64_t)blockIdx.x * kTile;
    const int nrow = (int)min((int64_t)kTile, (int64_t)a.rows - row0);
    {
        // rows row0 .. row0 + nrow - 1 are one contiguous block of obs; nothing past obs[rows][L] is read
        const float *src = a.obs + row0 * L;
        const int n = nrow * L;
        for (int i = lane; i < kTile * L; i += kWave) tile[i] = i < n ? src[i] : 0.f;
    }
    __syncthreads();
    const int64_t row = row0 + j;
    const bool valid = j < nrow;
    const float *trow = tile + j * L;
    const float *P = a.packed;

    // a1 = tanh(W1 x + b1): lane half h supplies obs[row][2 s + h] (0 past L: the tail of the last step is not from memory)
    // kAhead k-steps at a time, their operands loaded before the first product: a loop of load, wait, product spends one
    // L2 round trip per k-step (65 of them at L = 130) on a chain whose products take 64 cycles each
    f32x16 a1[1], a2[1], head[1];  // one tile per layer: chain<1, 1>
    a1[0] = load_tile(P + a.l.b1, h);
    {
        const float *w1 = P + a.l.w1 + lane;
        for (int s0 = 0; s0 < a.l.S1; s0 += kAhead) {
            float wv[kAhead], bv[kAhead];
#pragma unroll
            for (int u = 0; u < kAhead; u++) {
                const int s = s0 + u, k = 2 * s + h;
                wv[u] = s < a.l.S1 ? w1[s * 64] : 0.f;  // nothing past the packed fc1 rows is read
                bv[u] = k < L ? trow[k] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < kAhead; u++)
                if (s0 + u < a.l.S1) a1[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(wv[u], bv[u], a1[0], 0, 0, 0);
        }
    }
#pragma unroll
    for (int r = 0; r < 16; r++) a1[0][r] = tanhf(a1[0][r]);

    a2[0] = load_tile(P + a.l.b2, h);
    chain<1, 1>(a2, a1, P + a.l.w2, lane);
#pragma unroll
    for (int r = 0; r < 16; r++) a2[0][r] = tanhf(a2[0][r]);

    // heads: rows 0 .. 4 of the tile are the advantages, row 5 the value: lane half 0 holds adv 0 .. 3 in registers 0 .. 3,
    // lane half 1 holds adv 4 and the value in registers 0 and 1
    head[0] = load_tile(P + a.l.bh, h);
    chain<1, 1>(head, a2, P + a.l.wh, lane);
    const float adv4 = __shfl(head[0][0], j + 32), val = __shfl(head[0][1], j + 32);
    if (h != 0 || !valid) return;

    const float adv[NA] = {head[0][0], head[0][1], head[0][2], head[0][3], adv4};
    const float mean = ((((adv[0] + adv[1]) + adv[2]) + adv[3]) + adv[4]) / 5.0f;
    float qv[NA];
#pragma unroll
    for (int k = 0; k < NA; k++) qv[k] = val + adv[k] - mean;
    int act = 0;
#pragma unroll
    for (int k = 1; k < NA; k++)
        if (qv[k] > qv[act]) act = k;
    if (a.epsilon) {
        const double eps = (double)a.epsilon[0];
        const uint32_t d = a.draws[row];
        const uint64_t x = mix64(a.seed ^ (((uint64_t)row << 32) | d));
        const double u = uniform24(x);
        if (u < eps) act = (int)((mix64(x + kGolden) >> 40) % 5u);
        if (!(a.mode & MAPF_QNET_PEEK)) a.draws[row] = d + 1u;
    }
    a.action[row] = (int8_t)act;
    if (a.q) {
#pragma unroll
        for (int k = 0; k < NA; k++) a.q[row * NA + k] = qv[k];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// prioritised sampling
// ---------------------------------------------------------------------------------------------------------------------

constexpr int kChunk = MAPF_REPLAY_CHUNK;  // weights per chunk: four per lane of one wavefront
constexpr int kScanThreads = 1024;
static_assert(kChunk == 4 * kWave, "a lane owns four consecutive weights of its chunk");

// the workspace: [0] W, [1] the draw counter this call uses, then the inclusive prefix of the chunk sums, then the counts
struct ReplayWs {
    uint64_t *head;    // [2]
    uint64_t *prefix;  // [nchunks]
    uint32_t *count;   // [nchunks]
};

__host__ __device__ inline int64_t replay_chunks(int64_t C) { return (C + kChunk - 1) / kChunk; }

__host__ __device__ inline ReplayWs carve(void *ws, int64_t nchunks) {
    ReplayWs r;
    r.head = (uint64_t *)ws;
    r.prefix = r.head + 2;
    r.count = (uint32_t *)(r.prefix + nchunks);
    return r;
}

// a lane's four weights of chunk `chunk` (0 past the end: nothing outside w[C] is read)
__device__ __forceinline__ void lane_weights(const uint32_t *__restrict__ w, int64_t C, int64_t chunk, int lane, uint32_t v[4]) {
    const int64_t base = chunk * kChunk + 4 * lane;
#pragma unroll
    for (int i = 0; i < 4; i++) v[i] = base + i < C ? w[base + i] : 0u;
}

__global__ __launch_bounds__(256) void k_replay_sums(const uint32_t *__restrict__ w, int64_t C, int64_t nchunks, void *ws) {
    const int lane = threadIdx.x & 63;
    const int64_t chunk = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (chunk >= nchunks) return;
    const ReplayWs r = carve(ws, nchunks);
    uint32_t v[4];
    lane_weights(w, C, chunk, lane, v);
    uint64_t s = (uint64_t)v[0] + v[1] + v[2] + v[3];
    uint64_t n = (uint64_t)((v[0] != 0) + (v[1] != 0) + (v[2] != 0) + (v[3] != 0));
    s = wave_sum(s), n = wave_sum(n);
    if (lane == 0) r.prefix[chunk] = s, r.count[chunk] = (uint32_t)n;
}

// one workgroup: thread t owns chunks [t per, (t + 1) per)
__global__ __launch_bounds__(kScanThreads) void k_replay_scan(int64_t nchunks, void *ws, uint32_t *draws, int64_t *stats) {
    __shared__ uint64_t s_sum[kScanThreads];
    __shared__ uint64_t s_cnt[kScanThreads];
    const ReplayWs r = carve(ws, nchunks);
    const int t = threadIdx.x;
    const int64_t per = (nchunks + kScanThreads - 1) / kScanThreads;
    const int64_t c0 = min(nchunks, (int64_t)t * per), c1 = min(nchunks, c0 + per);
    uint64_t s = 0, n = 0;
    for (int64_t c = c0; c < c1; c++) s += r.prefix[c], n += r.count[c];
    s_sum[t] = s, s_cnt[t] = n;
    __syncthreads();
    for (int o = 1; o < kScanThreads; o <<= 1) {  // inclusive scan of the per-thread sums
        const uint64_t a = t >= o ? s_sum[t - o] : 0, b = t >= o ? s_cnt[t - o] : 0;
        __syncthreads();
        s_sum[t] += a, s_cnt[t] += b;
        __syncthreads();
    }
    uint64_t run = t > 0 ? s_sum[t - 1] : 0;
    for (int64_t c = c0; c < c1; c++) run += r.prefix[c], r.prefix[c] = run;
    if (t == 0) {
        const uint32_t d = draws[0];
        r.head[0] = s_sum[kScanThreads - 1];
        r.head[1] = d;
        draws[0] = d + 1u;
        if (stats) stats[0] = (int64_t)s_sum[kScanThreads - 1], stats[1] = (int64_t)s_cnt[kScanThreads - 1];
    }
}

// a wavefront per sample
__global__ __launch_bounds__(256) void k_replay_search(const uint32_t *__restrict__ w, int64_t C, int64_t nchunks, const void *ws,
                                                       int32_t K, uint64_t seed, int32_t *idx, uint32_t *wk) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (k >= K) return;
    const ReplayWs r = carve(const_cast<void *>(ws), nchunks);
    const uint64_t W = r.head[0];
    if (W == 0) {
        if (lane == 0) {
            idx[k] = -1;
            if (wk) wk[k] = 0u;
        }
        return;
    }
    const uint64_t lo = (uint64_t)k * W / (uint64_t)K, hi = ((uint64_t)k + 1) * W / (uint64_t)K;  // (k + 1) W < 2^62
    const uint64_t x = mix64(seed ^ ((r.head[1] << 32) | (uint64_t)(uint32_t)k));
    const uint64_t span = hi > lo ? hi - lo : 1;
    const uint64_t target = lo + x % span;  // < W
    // the first chunk whose inclusive prefix exceeds the target
    int64_t a = 0, b = nchunks - 1;
    while (a < b) {
        const int64_t m = (a + b) >> 1;
        if (r.prefix[m] > target) b = m; else a = m + 1;
    }
    const uint64_t before = a > 0 ? r.prefix[a - 1] : 0;
    uint32_t v[4];
    lane_weights(w, C, a, lane, v);
    const uint64_t own = (uint64_t)v[0] + v[1] + v[2] + v[3];
    uint64_t incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const uint64_t up = __shfl_up(incl, o, 64);
        if (lane >= o) incl += up;
    }
    const bool hit = before + incl > target;
    const uint64_t ballot = __ballot(hit);  // never 0: the chunk's inclusive prefix exceeds the target
    const int first = __ffsll((unsigned long long)ballot) - 1;
    if (lane == first) {
        uint64_t run = before + incl - own;
        int i = 0;
#pragma unroll
        for (int e = 0; e < 3; e++) {
            if (i == e && run + v[e] <= target) run += v[e], i = e + 1;
        }
        const int64_t at = a * kChunk + 4 * lane + i;
        idx[k] = (int32_t)at;
        if (wk) wk[k] = i == 0 ? v[0] : i == 1 ? v[1] : i == 2 ? v[2] : v[3];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// TD objective
// ---------------------------------------------------------------------------------------------------------------------

constexpr int kTdThreads = MAPF_DQN_TD_TILE;
static_assert(kTdThreads == 256, "four wavefronts per workgroup below");

struct TdArgs {
    const float *q, *qn_online, *qn_target;
    const int8_t *action;
    const float *reward;
    const uint8_t *ended;
    const float *isw;
    const int32_t *idx;
    uint32_t *weights;
    int64_t count;
    float *td, *dq;
    uint32_t *new_w;
    float *partials;
    float gamma, delta, alpha, inv_k;
    int32_t K;
};

__global__ __launch_bounds__(kTdThreads) void k_dqn_td(TdArgs a) {
    __shared__ float s_part[kTdThreads / 64][2];
    const int tid = threadIdx.x;
    const int64_t k = (int64_t)blockIdx.x * kTdThreads + tid;
    float sum_l = 0.f, sum_abs = 0.f;
    if (k < a.K) {
        float qv[NA];
#pragma unroll
        for (int j = 0; j < NA; j++) qv[j] = a.q[k * NA + j];
        const int8_t ab = a.action[k];
        const int act = clamp_action(ab);
        const float r = a.reward[k], qa = pick(qv, act);
        float y = r;
        double yd = (double)r;
        if (!a.ended[k]) {  // an ended step reads nothing of the next observation
            float on[NA], tg[NA];
#pragma unroll
            for (int j = 0; j < NA; j++) on[j] = a.qn_online[k * NA + j], tg[j] = a.qn_target[k * NA + j];
            int best = 0;
#pragma unroll
            for (int j = 1; j < NA; j++)
                if (on[j] > on[best]) best = j;
            const float qt = pick(tg, best);
            y = r + a.gamma * qt;
            yd = (double)r + (double)a.gamma * (double)qt;
        }
        const float td = qa - y, ad = fabsf(td), w = a.isw[k];
        const float l = ad <= a.delta ? 0.5f * td * td : a.delta * (ad - 0.5f * a.delta);
        sum_l = w * l, sum_abs = ad;
        if (a.td) a.td[k] = td;
        if (a.dq) {
            const float g = w * fminf(fmaxf(td, -a.delta), a.delta) * a.inv_k;
#pragma unroll
            for (int j = 0; j < NA; j++) a.dq[k * NA + j] = j == act ? g : 0.f;
        }
        if (a.new_w || (a.idx && a.weights)) {
            // the priority in double from the fp32 inputs: 2^16 (|td| + 1e-6)^alpha has 21 bits in front of the point
            const double p = pow(fabs((double)qa - yd) + 1e-6, (double)a.alpha) * 65536.0;
            const double c = fmin(fmax(rint(p), 1.0), 1048576.0);  // a NaN gives 1
            const uint32_t nw = (uint32_t)c;
            if (a.new_w) a.new_w[k] = nw;
            if (a.idx && a.weights) {
                const int32_t at = a.idx[k];
                if (at >= 0 && at < a.count) a.weights[at] = nw;
            }
        }
    }
    if (!a.partials) return;
    sum_l = wave_sum(sum_l), sum_abs = wave_sum(sum_abs);
    if ((tid & 63) == 0) s_part[tid >> 6][0] = sum_l, s_part[tid >> 6][1] = sum_abs;
    __syncthreads();
    if (tid == 0) {
        float l = s_part[0][0], d = s_part[0][1];
        for (int w = 1; w < kTdThreads / 64; w++) l += s_part[w][0], d += s_part[w][1];
        a.partials[(int64_t)blockIdx.x * 2 + 0] = l;
        a.partials[(int64_t)blockIdx.x * 2 + 1] = d;
    }
}

}  // namespace

struct mapf_qnet {
    mapf_qnet_config cfg;
    QLayout l;
    float *packed = nullptr;
    bool params_set = false;
};

extern "C" {

int mapf_qnet_create(const mapf_qnet_config *cfg, mapf_qnet_handle *out) {
    if (!cfg || !out) return MAPF_ERR_CONFIG;
    *out = nullptr;
    if (cfg->hidden != MAPF_QNET_HIDDEN) return MAPF_ERR_CONFIG;
    if (cfg->obs_len < 1 || cfg->obs_len > kMaxObsLen) return MAPF_ERR_CONFIG;
    return handle_create(*cfg, make_layout(cfg->obs_len), out);
}

int mapf_qnet_destroy(mapf_qnet_handle p) { return handle_destroy(p); }

int64_t mapf_qnet_param_count(mapf_qnet_handle p) { return handle_param_count(p); }

int mapf_qnet_set_params(mapf_qnet_handle p, const float *params, int64_t count, void *stream) {
    return handle_set_params(p, params, count, stream, k_qnet_pack);
}

int mapf_qnet_act(mapf_qnet_handle p, int32_t rows, const float *obs, const float *epsilon, uint32_t *draws, uint64_t seed,
                  int32_t mode, int8_t *action, float *q, void *stream) {
    if (!p || !obs || !action) return MAPF_ERR_CONFIG;
    if (mode & ~MAPF_QNET_PEEK) return MAPF_ERR_CONFIG;
    if (epsilon && !draws) return MAPF_ERR_CONFIG;
    if (rows < 1) return MAPF_ERR_CONFIG;
    if (!p->params_set) return MAPF_ERR_STATE;
    QActArgs a{};
    a.packed = p->packed, a.obs = obs, a.epsilon = epsilon, a.draws = draws, a.seed = seed, a.action = action, a.q = q;
    a.rows = rows, a.mode = mode, a.l = p->l;
    const dim3 grid((uint32_t)(((int64_t)rows + kTile - 1) / kTile)), block(kWave);
    const size_t lds = (size_t)kTile * (size_t)a.l.L * sizeof(float);
    hipLaunchKernelGGL(k_qnet_act, grid, block, lds, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int64_t mapf_replay_sample_workspace_bytes(int64_t count) {
    if (count < 1 || count > MAPF_REPLAY_MAX_COUNT) return 0;
    return 16 + 12 * replay_chunks(count);
}

int mapf_replay_sample(const uint32_t *weights, int64_t count, int32_t K, uint32_t *draws, uint64_t seed, void *workspace,
                       int32_t *idx, uint32_t *wk, int64_t *stats, void *stream) {
    if (!weights || !draws || !workspace || !idx) return MAPF_ERR_CONFIG;
    if (count < 1 || count > MAPF_REPLAY_MAX_COUNT || K < 1 || K > MAPF_REPLAY_MAX_SAMPLES) return MAPF_ERR_CONFIG;
    if ((uintptr_t)workspace & 7) return MAPF_ERR_CONFIG;
    const int64_t nchunks = replay_chunks(count);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(k_replay_sums, dim3((uint32_t)((nchunks + 3) / 4)), dim3(256), 0, s, weights, count, nchunks, workspace);
    hipLaunchKernelGGL(k_replay_scan, dim3(1), dim3(kScanThreads), 0, s, nchunks, workspace, draws, stats);
    hipLaunchKernelGGL(k_replay_search, dim3((uint32_t)((K + 3) / 4)), dim3(256), 0, s, weights, count, nchunks,
                       (const void *)workspace, K, seed, idx, wk);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

int32_t mapf_dqn_td_partials(int32_t K) { return K < 1 ? 0 : (int32_t)(((int64_t)K + kTdThreads - 1) / kTdThreads); }

int mapf_dqn_td_loss(int32_t K, const float *q, const float *qn_online, const float *qn_target, const int8_t *action,
                     const float *reward, const uint8_t *ended, const float *isw, float gamma, float delta, float alpha,
                     const int32_t *idx, uint32_t *weights, int64_t count, float *td, float *dq, uint32_t *new_w, float *partials,
                     void *stream) {
    if (K < 1 || K > MAPF_REPLAY_MAX_SAMPLES) return MAPF_ERR_CONFIG;
    if (!q || !qn_online || !qn_target || !action || !reward || !ended || !isw) return MAPF_ERR_CONFIG;
    if ((idx == nullptr) != (weights == nullptr) || (weights && (count < 1 || count > MAPF_REPLAY_MAX_COUNT))) return MAPF_ERR_CONFIG;
    if (!isfinite(gamma) || gamma < 0.f || gamma > 1.f || !isfinite(delta) || !(delta > 0.f) || !isfinite(alpha) || alpha < 0.f ||
        alpha > 1.f)
        return MAPF_ERR_CONFIG;
    TdArgs a{};
    a.q = q, a.qn_online = qn_online, a.qn_target = qn_target, a.action = action, a.reward = reward, a.ended = ended, a.isw = isw;
    a.idx = idx, a.weights = weights, a.count = count, a.td = td, a.dq = dq, a.new_w = new_w, a.partials = partials;
    a.gamma = gamma, a.delta = delta, a.alpha = alpha, a.inv_k = 1.0f / (float)K, a.K = K;
    hipLaunchKernelGGL(k_dqn_td, dim3((uint32_t)mapf_dqn_td_partials(K)), dim3(kTdThreads), 0, (hipStream_t)stream, a);
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
