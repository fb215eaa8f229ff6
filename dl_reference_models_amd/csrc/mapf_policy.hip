// mapf_policy.hip -- the fused recurrent policy of libmapfstep.so (mapf_policy_*; include/mapf_step.h states the rule).
//
// One launch takes every agent row from its observation to action, log-probability, value and new LSTM state.  A
// wavefront owns a tile of 32 rows and computes every product TRANSPOSED on the f32-input MFMA (v_mfma_f32_32x32x2_f32):
//   D[out feature i][row j] = sum_k W[i][k] * X^T[k][j]        A = W (one dword per lane), B = X^T (one dword per lane)
// The result tile has the agent row on the lane (j = lane & 31) and the output features in the 16 accumulator registers
// (feature = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) of its 32-feature tile), and that IS the B-operand layout of the
// next product when its k-steps are taken in the order "register r of tile m": lane half h then supplies feature
// 32 m + (r & 3) + 8 (r >> 2) + 4 h, and mapf_policy_set_params packs every weight matrix so that the A dword of the same
// lane in the same step is the weight of exactly that feature.  So fc1 -> fc2 -> LSTM gates -> heads chain in registers:
// no LDS between the products, no lane movement (two shuffles in the epilogue bring logit 4 and the value to the lane
// that owns the row).  h and c live in the same layout, so the state loads and stores are 16-byte accesses per lane.
// LDS holds only the wave's 32 x L observation tile (a contiguous block of global memory, copied coalesced).  The packed
// weights (162 KB for the recurrent policy at F = 28) do not fit next to it and are read through L2 as 256-byte rows, one
// dword per lane per MFMA.
// Vector stores and plain C++ only.  fp32 operands, fp32 accumulation, correctly rounded division, libm-grade tanh / exp
// / log: no fast-math (build.py).  The Gumbel noise is evaluated in double, since u = (n + 0.5) * 2^-24 has 25 bits.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "mapf_nn.h"
#include "mapf_step.h"

namespace {

using namespace mapf_nn;  // the accumulator layout and its helpers, the packing index maps, the handle's host side

constexpr int kTile = 32;     // agent rows per wavefront (the MFMA's N)
constexpr int kThreads = 64;  // one wavefront per workgroup: nothing is shared between tiles but the weights in L2
constexpr int kExtraSteps = 3;  // k-steps of the LSTM input past a2: onehot5(prev_action), prev_reward

// where everything lies: `src_*` in the flat parameter vector (state_dict order), the rest in the packed buffer (floats)
struct PolicyLayout {
    int32_t F, S1;  // features, k-steps of fc1 (F rounded up to the MFMA's K = 2)
    int32_t recurrent;
    int32_t src_fc1w, src_fc1b, src_fc2w, src_fc2b, src_wih, src_whh, src_bih, src_bhh, src_piw, src_pib, src_vfw, src_vfb;
    int32_t src_count;
    int32_t w1, b1, w2, b2, wih, whh, bl, wh, bh, total;
};

template <int HID>
PolicyLayout make_layout(int F, int recurrent) {
    constexpr int G = 4 * HID, ZIN = HID + kActions + 1;
    PolicyLayout l{};
    l.F = F;
    l.S1 = (F + 1) / 2;
    l.recurrent = recurrent;
    int o = 0;
    l.src_fc1w = o, o += HID * F;
    l.src_fc1b = o, o += HID;
    l.src_fc2w = o, o += HID * HID;
    l.src_fc2b = o, o += HID;
    if (recurrent) {
        l.src_wih = o, o += G * ZIN;
        l.src_whh = o, o += G * HID;
        l.src_bih = o, o += G;
        l.src_bhh = o, o += G;
    }
    l.src_piw = o, o += kActions * HID;
    l.src_pib = o, o += kActions;
    l.src_vfw = o, o += HID;
    l.src_vfb = o, o += 1;
    l.src_count = o;
    o = 0;
    l.w1 = o, o += l.S1 * (HID / 32) * 64;
    l.b1 = o, o += HID;
    l.w2 = o, o += (HID / 2) * (HID / 32) * 64;
    l.b2 = o, o += HID;
    if (recurrent) {
        l.wih = o, o += (HID / 32) * (HID / 2 + kExtraSteps) * 4 * 64;
        l.whh = o, o += (HID / 32) * (HID / 2) * 4 * 64;
        l.bl = o, o += G;
    }
    l.wh = o, o += (HID / 2) * 64;
    l.bh = o, o += 32;
    l.total = o;
    return l;
}

// one thread per packed float: zero-padded to the MFMA's K, gate biases summed (bih + bhh, one fp32 addition)
template <int HID>
__global__ __launch_bounds__(256) void k_policy_pack(const float *__restrict__ P, float *__restrict__ out, PolicyLayout l) {
    constexpr int ZIN = HID + kActions + 1, NT = HID / 32, KS = HID / 2 + kExtraSteps;
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= l.total) return;
    P += (int64_t)blockIdx.y * l.src_count, out += (int64_t)blockIdx.y * l.total;  // weight set blockIdx.y (per-agent handle)
    float v;
    if (t < l.b1) v = pack_read(P, l.src_fc1w, pack_fc1(t - l.w1, NT, l.F));
    else if (t < l.w2) v = P[l.src_fc1b + (t - l.b1)];
    else if (t < l.b2) v = pack_read(P, l.src_fc2w, pack_chained(t - l.w2, NT));
    else if (t < (l.recurrent ? l.wih : l.wh)) v = P[l.src_fc2b + (t - l.b2)];
    else if (l.recurrent && t < l.whh) v = pack_read(P, l.src_wih, pack_wih(t - l.wih, NT, KS, ZIN));
    else if (l.recurrent && t < l.bl) v = pack_read(P, l.src_whh, pack_whh(t - l.whh, NT));
    else if (l.recurrent && t < l.wh) v = P[l.src_bih + (t - l.bl)] + P[l.src_bhh + (t - l.bl)];
    else if (t < l.bh) v = pack_read(P, 0, pack_head(t - l.wh, NT, kActions, l.src_piw, l.src_vfw));
    else v = pack_read(P, 0, pack_head_bias(t - l.bh, kActions, l.src_pib, l.src_vfb));
    out[t] = v;
}

struct ActArgs {
    const float *packed;
    const float *obs;
    const int8_t *prev_action;
    const float *prev_reward;
    const uint8_t *start_a, *start_b;
    float *hstate, *cstate;
    uint32_t *draws;
    uint64_t seed;
    int8_t *action;
    float *logp, *value, *logits;
    int32_t rows, L, mask_off, agents_per_env, mode;
    PolicyLayout l;
    // mapped handles only (behind l: the shared kernel's offsets stay): the groups, U = rows / groups units per group,
    // ceil(U / 32), and the handle's device copy of the group-to-set map
    int32_t groups, units, unit_tiles;
    const int32_t *set_of_group;
};

// The block order of the mapped launch (G * ceil(U / 32) one-wave workgroups; a per-agent handle is G = N groups with the
// identity map, group = agent).  Group-major (kept): group = block / ceil(U / 32), neighbouring blocks share a weight set
// and every XCD's L2 sees every set over the launch.  Group-fastest: group = block % G, so with workgroups dealt round-robin
// over the 8 XCDs an XCD's L2 sees the weights of only G / 8 groups when 8 divides G.  Measured (tools/time_dte.py): agent-major is 1.4 to 1.8 % faster at 8 agents in every
// round of two runs; at 16 agents the two lie within 1.3 % of each other and the sign follows the handle's place in the
// measurement, not the order.  Results do not depend on it.  -DMAPF_POLICY_AGENT_FASTEST=1 builds the other one.
#ifndef MAPF_POLICY_AGENT_FASTEST
#define MAPF_POLICY_AGENT_FASTEST 0
#endif
constexpr bool kAgentFastest = MAPF_POLICY_AGENT_FASTEST != 0;

// MAPPED = false: a tile is 32 consecutive rows and every row reads the one packed weight set.  MAPPED = true: a tile is
// 32 UNITS of one group g of the handle's G (lane j of tile (g, ub) owns row (32 ub + j) G + g, the row's env is row / N),
// and the weights are set set_of_group[g] of the handle's: one uniform load per workgroup.  A per-agent handle is G = N
// with the identity map, a population of P members P N groups with set g / N.  Only the addressing differs: which rows,
// which start flag, which weight base; the body below it is the same code, and the arithmetic of a row does not depend on
// its tile-mates, so both give a row the same bits.
template <int HID, bool REC, bool MAPPED>
__global__ __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(2))) void k_policy_act(ActArgs a) {
    static_assert(HID % 32 == 0, "the hidden width is a whole number of 32-feature accumulator tiles");
    constexpr int NT = HID / 32, CH = HID / 2;
    extern __shared__ __attribute__((aligned(16))) float tile[];  // [kTile][L]: the wave's observation rows
    const int lane = threadIdx.x, j = lane & 31, h = lane >> 5;
    const int L = a.L, F = a.l.F;
    int64_t row;
    bool valid, start = false;
    const float *P = a.packed;
    if constexpr (MAPPED) {
        const int G = a.groups;
        const int g = kAgentFastest ? (int)(blockIdx.x % (uint32_t)G) : (int)(blockIdx.x / (uint32_t)a.unit_tiles);
        const int ub = kAgentFastest ? (int)(blockIdx.x / (uint32_t)G) : (int)(blockIdx.x % (uint32_t)a.unit_tiles);
        const int unit0 = ub * kTile, nunit = min(kTile, a.units - unit0);
        // 32 rows of L floats at a stride of G L: a half-wave copies a row; nothing outside obs[rows][L] is read
        for (int r = h; r < kTile; r += 2) {
            const float *src = a.obs + ((int64_t)(unit0 + r) * G + g) * L;
            for (int k = j; k < L; k += 32) tile[r * L + k] = r < nunit ? src[k] : 0.f;
        }
        row = (int64_t)(unit0 + j) * G + g;
        valid = j < nunit;
        if (valid && (a.start_a || a.start_b)) {
            const int env = (int)row / a.agents_per_env;  // (rows is an int32)
            start = (a.start_a && a.start_a[env]) || (a.start_b && a.start_b[env]);
        }
        P += (int64_t)a.set_of_group[g] * a.l.total;  // (checked against the handle's sets at creation)
    } else {
        const int64_t row0 = (int64_t)blockIdx.x * kTile;
        const int nrow = (int)min((int64_t)kTile, (int64_t)a.rows - row0);
        {
            // rows row0 .. row0 + nrow - 1 are one contiguous block of obs; nothing past obs[rows][L] is read
            const float *src = a.obs + row0 * L;
            const int n = nrow * L;
            for (int i = lane; i < kTile * L; i += kThreads) tile[i] = i < n ? src[i] : 0.f;
        }
        row = row0 + j;
        valid = j < nrow;
        if (valid && (a.start_a || a.start_b)) {
            const int env = (int)row / a.agents_per_env;  // (rows is an int32)
            start = (a.start_a && a.start_a[env]) || (a.start_b && a.start_b[env]);
        }
    }
    __syncthreads();
    const float *trow = tile + j * L;

    // a1 = tanh(W1 x + b1): k-steps in natural order, lane half h supplies obs[row][2 s + h] (0 past F: the tail of the
    // last step never comes from memory)
    f32x16 a1[NT], a2[NT];
#pragma unroll
    for (int m = 0; m < NT; m++) a1[m] = load_tile(P + a.l.b1 + 32 * m, h);
    {
        const float *w1 = P + a.l.w1 + lane;
        for (int s = 0; s < a.l.S1; s++) {
            const int k = 2 * s + h;
            const float b = k < F ? trow[k] : 0.f;
#pragma unroll
            for (int m = 0; m < NT; m++) a1[m] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[(s * NT + m) * 64], b, a1[m], 0, 0, 0);
        }
    }
#pragma unroll
    for (int m = 0; m < NT; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) a1[m][r] = tanhf(a1[m][r]);

    // a2 = tanh(W2 a1 + b2)
#pragma unroll
    for (int m = 0; m < NT; m++) a2[m] = load_tile(P + a.l.b2 + 32 * m, h);
    chain<NT, NT>(a2, a1, P + a.l.w2, lane);
#pragma unroll
    for (int m = 0; m < NT; m++)
#pragma unroll
        for (int r = 0; r < 16; r++) a2[m][r] = tanhf(a2[m][r]);

    f32x16 u[NT];
    if constexpr (REC) {
        // z = [a2, onehot5(prev_action), prev_reward]; h and c in accumulator layout
        int pa = 0;
        float pr = 0.f;
        f32x16 hold[NT], cold[NT];
        const bool keep = valid && !start;
        if (keep && a.prev_action) pa = a.prev_action[row];
        if (keep && a.prev_reward) pr = a.prev_reward[row];
#pragma unroll
        for (int q = 0; q < NT; q++) {
            if (keep) {
                hold[q] = load_tile(a.hstate + row * HID + 32 * q, h);
                cold[q] = load_tile(a.cstate + row * HID + 32 * q, h);
            } else {
#pragma unroll
                for (int r = 0; r < 16; r++) hold[q][r] = 0.f, cold[q][r] = 0.f;
            }
        }
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
            for (int g = 0; g < 4; g++) gate[g] = load_tile(P + a.l.bl + HID * g + 32 * q, h);
            const float *wih = P + a.l.wih + q * (CH + kExtraSteps) * 256;
            chain<4, NT>(gate, a2, wih, lane);
#pragma unroll
            for (int e = 0; e < kExtraSteps; e++)
#pragma unroll
                for (int g = 0; g < 4; g++)
                    gate[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(wih[((CH + e) * 4 + g) * 64 + lane], zx[e], gate[g], 0, 0, 0);
            chain<4, NT>(gate, hold, P + a.l.whh + q * CH * 256, lane);
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float c1 = sigmoidf(gate[1][r]) * cold[q][r] + sigmoidf(gate[0][r]) * tanhf(gate[2][r]);
                cold[q][r] = c1;
                u[q][r] = sigmoidf(gate[3][r]) * tanhf(c1);
            }
        }
        if (valid && !(a.mode & MAPF_POLICY_PEEK)) {
#pragma unroll
            for (int q = 0; q < NT; q++) {
                store_tile(a.hstate + row * HID + 32 * q, h, u[q]);
                store_tile(a.cstate + row * HID + 32 * q, h, cold[q]);
            }
        }
    } else {
#pragma unroll
        for (int m = 0; m < NT; m++) u[m] = a2[m];
    }

    // heads: rows 0 .. 4 of one tile are the logits, row 5 the value: lane half 0 holds logits 0 .. 3 in registers 0 .. 3,
    // lane half 1 holds logit 4 and the value in registers 0 and 1
    f32x16 head[1];
    head[0] = load_tile(P + a.l.bh, h);
    chain<1, NT>(head, u, P + a.l.wh, lane);
    const float l4 = __shfl(head[0][0], j + 32), val = __shfl(head[0][1], j + 32);
    if (h != 0 || !valid) return;

    float lg[kActions] = {head[0][0], head[0][1], head[0][2], head[0][3], l4};
    if (a.mask_off >= 0) {
#pragma unroll
        for (int k = 0; k < kActions; k++) lg[k] += logf(trow[a.mask_off + k] + 1e-6f);
    }
    int act = 0;
    if (a.mode & MAPF_POLICY_SAMPLE) {
        const uint32_t d = a.draws[row];
        const uint64_t x = mix64(a.seed ^ (((uint64_t)row << 32) | d));
        double best = 0.0;
#pragma unroll
        for (int k = 0; k < kActions; k++) {
            const uint64_t xk = mix64(x + (uint64_t)(k + 1) * kGolden);
            const double uk = uniform24(xk);
            const double s = (double)lg[k] - log(-log(uk));
            if (k == 0 || s > best) best = s, act = k;
        }
        if (!(a.mode & MAPF_POLICY_PEEK)) a.draws[row] = d + 1u;
    } else {
#pragma unroll
        for (int k = 1; k < kActions; k++)
            if (lg[k] > lg[act]) act = k;
    }
    a.action[row] = (int8_t)act;
    if (a.logp) {
        float mx = lg[0];
#pragma unroll
        for (int k = 1; k < kActions; k++) mx = fmaxf(mx, lg[k]);
        float sum = 0.f;
#pragma unroll
        for (int k = 0; k < kActions; k++) sum += expf(lg[k] - mx);
        a.logp[row] = lg[act] - (mx + logf(sum));
    }
    if (a.value) a.value[row] = val;
    if (a.logits) {
#pragma unroll
        for (int k = 0; k < kActions; k++) a.logits[row * kActions + k] = lg[k];
    }
}

}  // namespace

struct mapf_policy {
    mapf_policy_config cfg;
    PolicyLayout l;
    float *packed = nullptr;  // `sets` packed images of l.total floats
    bool params_set = false;
    int sets = 1;             // 1: one policy for every row; otherwise row r reads set set_of_group[r % groups]
    int groups = 0;           // 0: a shared handle
    int32_t *set_of_group = nullptr;  // device [groups], owned
};

namespace {

// what both kinds of handle require of a config
bool config_ok(const mapf_policy_config *cfg) {
    if (cfg->hidden != MAPF_POLICY_HIDDEN) return false;
    if (cfg->obs_len < 1 || cfg->obs_len > kMaxObsLen) return false;
    if (cfg->mask_off != -1 && cfg->mask_off != cfg->obs_len - kActions) return false;
    if (cfg->mask_off == 0) return false;  // a mask and no feature
    if (cfg->recurrent != 0 && cfg->recurrent != 1) return false;
    return cfg->agents_per_env >= 1;
}

PolicyLayout layout_of(const mapf_policy_config *cfg) {
    return make_layout<MAPF_POLICY_HIDDEN>(cfg->mask_off >= 0 ? cfg->mask_off : cfg->obs_len, cfg->recurrent);
}

// a handle of `sets` weight sets whose row r reads set map[r % groups]; the arguments are checked by the callers
int create_mapped(const mapf_policy_config *cfg, int groups, int sets, const int32_t *map, mapf_policy_handle *out) {
    const int rc = handle_create(*cfg, layout_of(cfg), out, sets);
    if (rc != MAPF_OK) return rc;
    mapf_policy *p = *out;
    p->sets = sets, p->groups = groups;
    int prev = 0;
    (void)hipGetDevice(&prev);
    // (a blocking copy from pageable memory: the map may be the caller's stack)
    const bool ok = hipSetDevice(cfg->device) == hipSuccess &&
                    hipMalloc((void **)&p->set_of_group, (size_t)groups * sizeof(int32_t)) == hipSuccess &&
                    hipMemcpy(p->set_of_group, map, (size_t)groups * sizeof(int32_t), hipMemcpyHostToDevice) == hipSuccess;
    (void)hipSetDevice(prev);
    if (!ok) {
        if (p->set_of_group) (void)hipFree(p->set_of_group);
        p->set_of_group = nullptr;
        (void)handle_destroy(p);
        *out = nullptr;
        return MAPF_ERR_HIP;
    }
    return MAPF_OK;
}

}  // namespace

extern "C" {

int mapf_policy_create(const mapf_policy_config *cfg, mapf_policy_handle *out) {
    if (!cfg || !out) return MAPF_ERR_CONFIG;
    *out = nullptr;
    if (!config_ok(cfg)) return MAPF_ERR_CONFIG;
    return handle_create(*cfg, layout_of(cfg), out);
}

int mapf_policy_create_per_agent(const mapf_policy_config *cfg, mapf_policy_handle *out) {
    if (!cfg || !out) return MAPF_ERR_CONFIG;
    *out = nullptr;
    if (!config_ok(cfg) || cfg->agents_per_env > MAPF_MAX_AGENTS) return MAPF_ERR_CONFIG;
    int32_t identity[MAPF_MAX_AGENTS];
    for (int a = 0; a < cfg->agents_per_env; a++) identity[a] = a;
    return create_mapped(cfg, cfg->agents_per_env, cfg->agents_per_env, identity, out);
}

int mapf_policy_create_mapped(const mapf_policy_config *cfg, int32_t groups, int32_t sets, const int32_t *set_of_group,
                              mapf_policy_handle *out) {
    if (!cfg || !out) return MAPF_ERR_CONFIG;
    *out = nullptr;
    if (!config_ok(cfg) || !set_of_group) return MAPF_ERR_CONFIG;
    if (groups < 1 || groups > MAPF_POLICY_MAX_GROUPS || groups % cfg->agents_per_env != 0) return MAPF_ERR_CONFIG;
    if (sets < 1 || sets > groups) return MAPF_ERR_CONFIG;
    for (int g = 0; g < groups; g++)
        if (set_of_group[g] < 0 || set_of_group[g] >= sets) return MAPF_ERR_CONFIG;
    return create_mapped(cfg, groups, sets, set_of_group, out);
}

int mapf_policy_destroy(mapf_policy_handle p) {
    if (p && p->set_of_group) (void)hipFree(p->set_of_group);
    return handle_destroy(p);
}

int64_t mapf_policy_param_count(mapf_policy_handle p) { return p ? (int64_t)p->sets * handle_param_count(p) : 0; }

int mapf_policy_set_params(mapf_policy_handle p, const float *params, int64_t count, void *stream) {
    return handle_set_params(p, params, count, stream, k_policy_pack<MAPF_POLICY_HIDDEN>, p ? p->sets : 1);
}

int mapf_policy_act(mapf_policy_handle p, int32_t rows, const float *obs, const int8_t *prev_action, const float *prev_reward,
                    const uint8_t *start_a, const uint8_t *start_b, float *hstate, float *cstate, uint32_t *draws, uint64_t seed,
                    int32_t mode, int8_t *action, float *logp, float *value, float *logits, void *stream) {
    if (!p || !obs || !action) return MAPF_ERR_CONFIG;
    if (p->cfg.recurrent && (!hstate || !cstate)) return MAPF_ERR_CONFIG;
    if (mode & ~(MAPF_POLICY_SAMPLE | MAPF_POLICY_PEEK)) return MAPF_ERR_CONFIG;
    if ((mode & MAPF_POLICY_SAMPLE) && !draws) return MAPF_ERR_CONFIG;
    if (rows < 1) return MAPF_ERR_CONFIG;
    if ((start_a || start_b) && rows % p->cfg.agents_per_env != 0) return MAPF_ERR_CONFIG;
    if (p->groups && rows % p->groups != 0) return MAPF_ERR_CONFIG;
    if (!p->params_set) return MAPF_ERR_STATE;
    ActArgs a{};
    a.packed = p->packed, a.obs = obs, a.prev_action = prev_action, a.prev_reward = prev_reward;
    a.start_a = start_a, a.start_b = start_b, a.hstate = hstate, a.cstate = cstate, a.draws = draws, a.seed = seed;
    a.action = action, a.logp = logp, a.value = value, a.logits = logits;
    a.rows = rows, a.L = p->cfg.obs_len, a.mask_off = p->cfg.mask_off, a.agents_per_env = p->cfg.agents_per_env, a.mode = mode;
    a.l = p->l;
    const dim3 block(kThreads);
    const size_t lds = (size_t)kTile * (size_t)a.L * sizeof(float);
    if (p->groups) {
        a.groups = p->groups, a.units = rows / p->groups, a.unit_tiles = (a.units + kTile - 1) / kTile;
        a.set_of_group = p->set_of_group;
        const dim3 grid((uint32_t)((int64_t)p->groups * a.unit_tiles));
        if (p->cfg.recurrent)
            hipLaunchKernelGGL((k_policy_act<MAPF_POLICY_HIDDEN, true, true>), grid, block, lds, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL((k_policy_act<MAPF_POLICY_HIDDEN, false, true>), grid, block, lds, (hipStream_t)stream, a);
    } else {
        const dim3 grid((uint32_t)(((int64_t)rows + kTile - 1) / kTile));
        if (p->cfg.recurrent)
            hipLaunchKernelGGL((k_policy_act<MAPF_POLICY_HIDDEN, true, false>), grid, block, lds, (hipStream_t)stream, a);
        else
            hipLaunchKernelGGL((k_policy_act<MAPF_POLICY_HIDDEN, false, false>), grid, block, lds, (hipStream_t)stream, a);
    }
    return hipGetLastError() == hipSuccess ? MAPF_OK : MAPF_ERR_HIP;
}

}  // extern "C"
