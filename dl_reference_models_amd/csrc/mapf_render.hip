// mapf_render.hip -- the rgb_array frame rasteriser of libmapfstep.so: kernel, launch and its part of the C ABI
// (mapf_render, include/mapf_step.h).
//
// A frame is an exact integer raster of one env's state (the rule is in include/mapf_step.h above mapf_render).  Every
// pixel of a cell takes one of five colours -- plain, grid line, goal diamond, line inside the diamond, agent disc -- and
// which one depends only on the pixel's offset inside the cell.  So a workgroup takes a BAND of cell rows of one frame:
//   1. LDS: the agents' plane-0 words (pos | goal << 16), the class of every offset in a cell (c x c bytes);
//   2. one thread per cell composes the cell's five colours, agents in index order (disc, then sensor window);
//   3. the band's pixels -- contiguous bytes of the output -- are written as a flat stream: each lane turns 16
//      consecutive pixels into 48 bytes and stores them as three 16-byte vector stores, so a wave writes 3 KiB of
//      contiguous output per instruction triple.  A pixel costs two LDS reads (its class, its cell's colour) and a few
//      ALU operations.  Only chunks that straddle an end of the band (at most two; the neighbouring band writes the
//      rest of such a chunk) or a pixel row (when W * c is not a multiple of 16) are written pixel by pixel.
// The kernel reads plane 0 of the agent state and the obstacle rows and writes the frames, plus the error record when
// an env id is out of range.  Nothing else: no stream, slot, counter or pass bit is touched.

#include <algorithm>
#include <type_traits>

#include "mapf_handle.h"

namespace mapfk {

namespace {

// A workgroup rasterises a band of rows_per_band cell rows of one frame; the host picks rows_per_band =
// ceil(kRenderBandPixels / (c * c * W)) (at most H), so a band holds at most 1024 + W - 1 < kRenderMaxBandCells cells and
// its five colours per cell fit the kernel's static LDS table.
#ifndef MAPF_RENDER_NT
#define MAPF_RENDER_NT 0  // 1: the frame stores carry the nontemporal hint (measured)
#endif
constexpr int kRenderThreads = 256;
constexpr int kRenderBandPixels = 16384;  // 48 KiB of output per workgroup when the cell rows allow it
constexpr int kRenderMaxBandCells = 1088;
struct RenderArgs : EnvView {
    const int32_t *env_ids;   // [K] or null (= 0 .. K-1)
    uint8_t *frames;          // [K][H*c][W*c][3]
    int sr;                   // sensor range; -1 on single-agent handles (no windows)
    int c, rows_per_band;
    int aligned;              // frames is 16-byte aligned: whole 16-pixel chunks leave as three 16-byte stores
};
// mapf_render_words: the agent words come from the caller instead of plane 0.  The fields are appended, so what the live
// instantiation reads of its argument sits where it always sat.
struct RenderWordsArgs : RenderArgs {
    const uint32_t *words;     // [M][N] pos | goal << 16 (an evaluation trace)
    const int32_t *word_rows;  // [K] row of `words` frame k is drawn from, or null (= 0 .. K-1)
};

// the reference's 16 agent colours in its order, CSS RGB (red, blue, green, purple, orange, cyan, magenta, yellow, brown,
// pink, olive, teal, navy, gold, lime, gray), as 0x00BBGGRR: byte 0 is R, the first byte of a pixel in memory
__device__ __forceinline__ uint32_t palette(int a) {
    constexpr uint32_t rgb[16] = {0xFF0000, 0x0000FF, 0x008000, 0x800080, 0xFFA500, 0x00FFFF, 0xFF00FF, 0xFFFF00,
                                  0xA52A2A, 0xFFC0CB, 0x808000, 0x008080, 0x000080, 0xFFD700, 0x00FF00, 0x808080};
    const uint32_t v = rgb[a & 15];
    return (v >> 16) | (v & 0xFF00u) | ((v & 0xFFu) << 16);
}

// blend(d, s, alpha) = (s * alpha + d * (255 - alpha) + 127) // 255 per channel
__device__ __forceinline__ uint32_t blend(uint32_t d, uint32_t s, uint32_t alpha) {
    uint32_t out = 0;
#pragma unroll
    for (int sh = 0; sh < 24; sh += 8) {
        const uint32_t dc = (d >> sh) & 255u, sc = (s >> sh) & 255u;
        out |= ((sc * alpha + dc * (255u - alpha) + 127u) / 255u) << sh;
    }
    return out;
}

enum { kClsPlain = 0, kClsLine = 1, kClsDiamond = 2, kClsLineDiamond = 3, kClsDisc = 4, kNumCls = 5 };
constexpr uint32_t kWhite = 0xFFFFFFu, kBlack = 0u, kGray = 0x808080u;

// 16 pixels (0x00BBGGRR) -> 48 bytes as 12 dwords, 4 pixels per 3 dwords
__device__ __forceinline__ void pack4(const uint32_t *px, uint32_t *d) {
    d[0] = px[0] | (px[1] << 24);
    d[1] = (px[1] >> 8) | (px[2] << 16);
    d[2] = (px[2] >> 16) | (px[3] << 8);
}

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

template <bool NT>
__device__ __forceinline__ void store16(uint8_t *dst, uint32_t a, uint32_t b, uint32_t c, uint32_t d) {
    const u32x4 v = {a, b, c, d};
    if constexpr (NT)
        __builtin_nontemporal_store(v, reinterpret_cast<u32x4 *>(dst));
    else
        *reinterpret_cast<u32x4 *>(dst) = v;
}

// Walks the pixels of a band in memory order from band-local pixel index l (y = l / Wp, x = l % Wp); the colour of a
// pixel is tab[cell][cls[offset in the cell]].
struct PixelWalk {
    int xm, ym, j, cb, mrow;  // offset in the cell (x, y), cell column, cell base in tab, row base in cls
    __device__ __forceinline__ PixelWalk(int l, int Wp, int W, int c) {
        const int y = l / Wp, x = l - y * Wp;
        const int i = y / c;
        ym = y - i * c;
        j = x / c;
        xm = x - j * c;
        cb = (i * W + j) * kNumCls;
        mrow = ym * c;
    }
    __device__ __forceinline__ void next(int W, int c) {
        if (++xm == c) {
            xm = 0;
            cb += kNumCls;
            if (++j == W) {  // next pixel row
                j = 0;
                cb -= W * kNumCls;
                mrow += c;
                if (++ym == c) {  // next cell row
                    ym = 0;
                    mrow = 0;
                    cb += W * kNumCls;
                }
            }
        }
    }
};

// WORDS: where s_agent comes from -- false: plane 0 of env env_ids[k] (mapf_render); true: row word_rows[k] of the caller's
// words (mapf_render_words).  Everything after that load is the same code.
template <bool NT, bool WORDS>
__global__ __launch_bounds__(kRenderThreads) void k_render(std::conditional_t<WORDS, RenderWordsArgs, RenderArgs> ra) {
    __shared__ uint32_t s_tab[kRenderMaxBandCells * kNumCls];  // five colours per cell of the band
    __shared__ __attribute__((aligned(16))) uint32_t s_agent[MAPF_MAX_AGENTS];  // pos | goal << 16
    __shared__ uint8_t s_cls[MAPF_RENDER_MAX_CELL_PX * MAPF_RENDER_MAX_CELL_PX];
    const Params &P = *ra.params;
    const int tid = (int)threadIdx.x;
    const int bands = (ra.H + ra.rows_per_band - 1) / ra.rows_per_band;
    const int k = (int)(blockIdx.x / (unsigned)bands), band = (int)(blockIdx.x - (unsigned)k * (unsigned)bands);
    const int H = ra.H, W = ra.W, N = ra.N, c = ra.c;
    const int i0 = band * ra.rows_per_band, nrows = min(ra.rows_per_band, H - i0);
    const int env = ra.env_ids ? ra.env_ids[k] : k;
    bool ok = (unsigned)env < (unsigned)ra.B;
    if constexpr (WORDS) {
        const int row = ra.word_rows ? ra.word_rows[k] : k;
        if (!ok && tid == 0 && band == 0) raise_error(P, MAPF_ERR_CONFIG, k, 0, env);
        if (ok && row < 0 && tid == 0 && band == 0) raise_error(P, MAPF_ERR_CONFIG, k, 0, row);
        ok = ok && row >= 0;
        if (ok && tid < N) s_agent[tid] = ra.words[(size_t)row * N + tid];
    } else {
        if (!ok && tid == 0 && band == 0) raise_error(P, MAPF_ERR_CONFIG, k, 0, env);
        if (ok && tid < N) s_agent[tid] = ra.agents[(size_t)env * N + tid].x;
    }
    for (int o = tid; o < c * c; o += kRenderThreads) {
        const int ym = o / c, xm = o - ym * c;
        const int dx = 2 * xm + 1 - c, dy = 2 * ym + 1 - c;
        const bool line = ym == 0 || xm == 0;
        const bool diamond = abs(dx) + abs(dy) <= c;
        // radius 0.3 cell; for c >= 4 the disc lies inside the diamond and off the grid lines, so its pixels show the
        // diamond colour until an agent stands on the cell
        const bool disc = 25 * (dx * dx + dy * dy) <= 9 * c * c;
        s_cls[o] = (uint8_t)(disc ? kClsDisc : (line ? kClsLine : kClsPlain) + (diamond ? kClsDiamond : 0));
    }
    __syncthreads();

    // compose: one thread per cell of the band
    const int ncell = nrows * W;
    for (int q = tid; q < ncell; q += kRenderThreads) {
        uint32_t col[kNumCls] = {0, 0, 0, 0, 0};
        if (ok) {
            const int ib = q / W, j = q - ib * W, i = i0 + ib;
            const uint32_t cell = ((uint32_t)i << 8) | (uint32_t)j;
            const bool obst = (ra.rows[(size_t)env * H + i] >> (j + ra.col_pad)) & 1ull;
            col[kClsPlain] = obst ? kBlack : kWhite;
            col[kClsLine] = kGray;
            col[kClsDiamond] = col[kClsPlain];
            col[kClsLineDiamond] = kGray;
            // (the agent words are read four at a time: one 16-byte LDS broadcast instead of four dependent reads)
            const uint4 *s_agent4 = reinterpret_cast<const uint4 *>(s_agent);
            for (int g0 = 0; g0 < N; g0 += 4) {
                const uint4 w4 = s_agent4[g0 >> 2];
                const uint32_t ws[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (g0 + u < N && (ws[u] >> 16) == cell) {
                        col[kClsDiamond] = blend(col[kClsDiamond], palette(g0 + u), 128u);
                        col[kClsLineDiamond] = blend(col[kClsLineDiamond], palette(g0 + u), 128u);
                    }
                }
            }
            col[kClsDisc] = col[kClsDiamond];
            for (int a0 = 0; a0 < N; a0 += 4) {
                const uint4 w4 = s_agent4[a0 >> 2];
                const uint32_t ws[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int a = a0 + u;
                    const uint32_t w = ws[u];
                    const int r = (int)((w >> 8) & 255u), cc = (int)(w & 255u);
                    if (a < N) {
                        const uint32_t pal = palette(a);
                        if ((w & 0xFFFFu) == cell) col[kClsDisc] = pal;
                        if (abs(i - r) <= ra.sr && abs(j - cc) <= ra.sr) {  // sr < 0: a single-agent handle draws no windows
#pragma unroll
                            for (int s = 0; s < kNumCls; s++) col[s] = blend(col[s], pal, 51u);
                        }
                    }
                }
            }
        }
        MAPF_CHK(P, (q + 1) * kNumCls <= kRenderMaxBandCells * kNumCls, 12, env, q);
#pragma unroll
        for (int s = 0; s < kNumCls; s++) s_tab[q * kNumCls + s] = col[s];
    }
    __syncthreads();

    // pixels: the band is the byte range [3 * p0, 3 * p1) of the output, p = pixel index over all frames.  Thread tid takes
    // the 16-pixel chunks q0 + tid, q0 + tid + kRenderThreads, ...; the band-local position of its chunk's first pixel,
    // l = y * Wp + x with y = i * c + ym and x = j * c + xm, advances by kStride pixels per iteration without a division.
    const int Wp = W * c;
    const int band_px = nrows * c * Wp;
    const size_t p0 = ((size_t)k * H + i0) * (size_t)c * Wp, p1 = p0 + band_px;
    const size_t q0 = p0 >> 4, q1 = (p1 + 15) >> 4;  // 16-pixel chunks overlapping the band
    const int tab_end = ncell * kNumCls;
    constexpr int kStride = kRenderThreads * 16;
    const int sy = kStride / Wp, sx = kStride - sy * Wp;
    const int syi = sy / c, sym = sy - syi * c, sxj = sx / c, sxm = sx - sxj * c;
    int l = (int)(((q0 + tid) << 4) - p0);  // >= -15: only chunk q0 can start before the band
    int i, ym, j, xm;
    {
        const int y = l >= 0 ? l / Wp : -1, x = l - y * Wp;
        i = y >= 0 ? y / c : -1;
        ym = y - i * c;
        j = x / c;
        xm = x - j * c;
    }
    for (size_t qc = q0 + tid; qc < q1; qc += kRenderThreads) {
        const size_t first = qc << 4;
        uint8_t *dst = ra.frames + first * 3;
        if (ra.aligned && l >= 0 && l + 16 <= band_px && j * c + xm + 16 <= Wp) {
            // the common chunk: inside the band and inside one pixel row, so only the cell column moves
            int cb = (i * W + j) * kNumCls, m = xm;
            const int mrow = ym * c;
            uint32_t px[16];
#pragma unroll
            for (int t = 0; t < 16; t++) {
                MAPF_CHK(P, mrow + m < c * c && cb + kNumCls <= tab_end, 12, env, cb);
                px[t] = s_tab[cb + s_cls[mrow + m]];
                const bool wrap = ++m == c;
                m = wrap ? 0 : m;
                cb += wrap ? kNumCls : 0;
            }
            uint32_t d[12];
#pragma unroll
            for (int t = 0; t < 4; t++) pack4(px + 4 * t, d + 3 * t);
            store16<NT>(dst, d[0], d[1], d[2], d[3]);
            store16<NT>(dst + 16, d[4], d[5], d[6], d[7]);
            store16<NT>(dst + 32, d[8], d[9], d[10], d[11]);
        } else {  // a chunk across a pixel row, across an end of the band, or an output not 16-byte aligned: byte stores
            const size_t lo = first > p0 ? first : p0, hi = first + 16 < p1 ? first + 16 : p1;
            if (lo < hi) {
                PixelWalk pw((int)(lo - p0), Wp, W, c);
                for (size_t p = lo; p < hi; p++) {
                    MAPF_CHK(P, pw.mrow + pw.xm < c * c && pw.cb + kNumCls <= tab_end, 12, env, pw.cb);
                    const uint32_t v = s_tab[pw.cb + s_cls[pw.mrow + pw.xm]];
                    uint8_t *o = ra.frames + p * 3;
                    o[0] = (uint8_t)v;
                    o[1] = (uint8_t)(v >> 8);
                    o[2] = (uint8_t)(v >> 16);
                    pw.next(W, c);
                }
            }
        }
        l += kStride;
        xm += sxm;
        j += sxj;
        if (xm >= c) { xm -= c; j++; }
        if (j >= W) { j -= W; ym++; }  // (a pixel row is exactly W cells: xm stays)
        ym += sym;
        i += syi;
        if (ym >= c) { ym -= c; i++; }
    }
}

hipError_t launch_render(const RenderArgs &ra, unsigned blocks, hipStream_t s) {
    LAUNCH_CHECKED((k_render<MAPF_RENDER_NT != 0, false>), dim3(blocks), dim3(kRenderThreads), 0, s, ra);
}

hipError_t launch_render_words(const RenderWordsArgs &ra, unsigned blocks, hipStream_t s) {
    LAUNCH_CHECKED((k_render<MAPF_RENDER_NT != 0, true>), dim3(blocks), dim3(kRenderThreads), 0, s, ra);
}

// What both entry points check and plan: the arguments of the launch in `ra` and its workgroups in `blocks`.
int plan_render(mapf_engine *e, const std::string &fn, const int32_t *env_ids, int32_t K, int32_t cell_px, uint8_t *frames,
                RenderArgs &ra, unsigned &blocks) {
    if (!e || !frames) return fail(e, MAPF_ERR_CONFIG, "null argument");
    if (K < 1) return fail(e, MAPF_ERR_CONFIG, fn + ": K must be >= 1");
    if (cell_px < MAPF_RENDER_MIN_CELL_PX || cell_px > MAPF_RENDER_MAX_CELL_PX)
        return fail(e, MAPF_ERR_CONFIG, fn + ": cell_px must lie in [4, 64]");
    if (!env_ids && K > e->p.B) return fail(e, MAPF_ERR_CONFIG, fn + ": K exceeds the number of envs (env_ids NULL)");
    if (!e->grids_set) return fail(e, MAPF_ERR_STATE, "mapf_set_grids must be called before " + fn);
    const int H = e->p.H, W = e->p.W, c = cell_px;
    const int R = std::min(H, std::max(1, (kRenderBandPixels + c * c * W - 1) / (c * c * W)));
    if (R * W > kRenderMaxBandCells) return fail(e, MAPF_ERR_INTERNAL, fn + ": band plan exceeds the LDS table");
    const uint64_t nb = (uint64_t)K * (uint64_t)((H + R - 1) / R);
    if (nb > 0x7FFFFFFFull) return fail(e, MAPF_ERR_CONFIG, fn + ": too many frames for one launch");
    ra = RenderArgs{env_view(e)};
    ra.env_ids = env_ids;
    ra.frames = frames;
    ra.sr = e->cte ? -1 : e->p.sr;
    ra.c = c;
    ra.rows_per_band = R;
    ra.aligned = (reinterpret_cast<uintptr_t>(frames) & 15u) == 0;
    blocks = (unsigned)nb;
    return MAPF_OK;
}

}  // namespace

}  // namespace mapfk

using namespace mapfk;

extern "C" int mapf_render(mapf_handle e, const int32_t *env_ids, int32_t K, int32_t cell_px, uint8_t *frames, void *stream) {
    RenderArgs ra;
    unsigned blocks = 0;
    const int rc = plan_render(e, "mapf_render", env_ids, K, cell_px, frames, ra, blocks);
    if (rc != MAPF_OK) return rc;
    ON_DEVICE(e);
    HIP_TRY(e, launch_render(ra, blocks, (hipStream_t)stream));
    return MAPF_OK;
}

extern "C" int mapf_render_words(mapf_handle e, const uint32_t *words, const int32_t *rows, const int32_t *env_ids, int32_t F,
                                 int32_t cell_px, uint8_t *frames, void *stream) {
    if (!e || !words || !env_ids || !frames) return fail(e, MAPF_ERR_CONFIG, "null argument");
    RenderWordsArgs ra;
    unsigned blocks = 0;
    const int rc = plan_render(e, "mapf_render_words", env_ids, F, cell_px, frames, ra, blocks);
    if (rc != MAPF_OK) return rc;
    ra.words = words;
    ra.word_rows = rows;
    ON_DEVICE(e);
    HIP_TRY(e, launch_render_words(ra, blocks, (hipStream_t)stream));
    return MAPF_OK;
}
