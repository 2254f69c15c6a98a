// slide.hip — sliding-window evaluation (evaluate.py:145-227, whole=False) without the full-resolution logits.
//
// gather_tiles_kernel: every zero-padded tile of an image (optionally of its mirror image, which is never formed) in one
// launch, [N,ch,h,w] -> [T,N,ch,th,tw].  Pure data movement; one lane owns four consecutive output floats (one 16-byte
// store), the last total % 4 floats go out one by one.
//
// slide_vote_kernel: the multi-scale + flip vote over the tiles' low-resolution logits.  The reference, per pass: every
// tile's logits are upsampled to the tile (th x tw), cropped to the part of the tile inside the image, summed into an
// N x C x hs x ws accumulator, divided by the number of tiles per pixel, flipped back, resized to H x W, summed.  All of it
// is linear in the low-resolution logits:
//
//   score[n,c,y,x] = sum_k weight_k * sum_{(Y,a) in lerp(y: hs_k -> H)} sum_{(X,b) in lerp(x: ws_k -> W)}
//                    a * b * S_k(n, c, Y, flip_k ? ws_k-1-X : X)
//   S_k(n,c,Y,X)   = 1/cnt_k(Y,X) * sum_{tiles t covering (Y,X)} U_kt(n, c, Y - y1_t, X - x1_t)
//   U_kt           = logits_k[t,n,c] resized bilinearly (lh, lw) -> (th, tw)
//
// The tile grid is separable (rows x cols origins), so is cnt_k.  One lane owns one output pixel and walks the origin
// tables of a pass (any number of tiles may cover a pixel); per covering tile it has 2 x 2 taps that are reused over the
// classes.  The summation order (passes, the two rows Y, tile rows, the two columns X, tile columns, classes) is fixed
// and there are no float atomics: two calls give the same bits.  The pixel loop, the argmax and the confusion count
// around that sum are vote_core.h's, shared with vote.hip.
//
// The origins (up to 16 passes x (32 + 32)) do not fit the kernel arguments beside the descriptors: the kernel reads
// them from a device table that the caller keeps (a copy of the host table that is validated here) and stages them in
// LDS.  Whatever the device table holds, no access leaves a tile: a tile takes part only where
// origin <= Y < origin + th, and the taps inside it are clamped by lerp_of.
//
// Coordinate rule of all index computations: bilinear.h (lerp_of / host_scale).
#include "common.h"
#include "bilinear.h"
#include "vote_core.h"

namespace {

using namespace dcfp_bilinear;
using namespace dcfp_vote;

constexpr int kMaxPasses = DCFP_SLIDE_MAX_PASSES;
constexpr int kMaxAxis = DCFP_SLIDE_MAX_TILES_PER_AXIS;
constexpr int kTabStride = 2 * kMaxAxis;          // per pass: kMaxAxis row origins, then kMaxAxis column origins

struct GatherArgs {
    int ys[kMaxAxis], xs[kMaxAxis];
};

// position of one output float: tile, image, channel, row and column inside the tile
struct TilePos {
    int t, n, c, i, j;
};

__device__ __forceinline__ TilePos tile_pos(long long o, int N, int ch, int th, int tw) {
    TilePos p;
    p.j = (int)(o % tw);
    long long r = o / tw;
    p.i = (int)(r % th);
    r /= th;
    p.c = (int)(r % ch);
    r /= ch;
    p.n = (int)(r % N);
    p.t = (int)(r / N);
    return p;
}

// the next output float (the output is dense, so the carries run through all five indices)
__device__ __forceinline__ void tile_next(TilePos& p, int N, int ch, int th, int tw) {
    if (++p.j < tw) return;
    p.j = 0;
    if (++p.i < th) return;
    p.i = 0;
    if (++p.c < ch) return;
    p.c = 0;
    if (++p.n < N) return;
    p.n = 0;
    ++p.t;
}

template <bool FLIP>
__device__ __forceinline__ float gather_one(const float* __restrict__ image, const GatherArgs& g, const TilePos& p,
                                            int ch, int h, int w, int cols) {
    const int y = g.ys[p.t / cols] + p.i, x = g.xs[p.t % cols] + p.j;
    if (y >= h || x >= w) return 0.f;
    return image[(((long long)p.n * ch + p.c) * h + y) * w + (FLIP ? w - 1 - x : x)];
}

// The four floats of a quad are loaded one by one: a tile row starts at any column of the image (and runs backwards
// under FLIP), so no 16-byte alignment of the source can be relied on; lanes of a wave still read neighbouring
// addresses.  The index decomposition is done once per quad.
template <bool FLIP>
__global__ void __launch_bounds__(kThreads)
gather_tiles_kernel(const float* __restrict__ image, const GatherArgs g, int N, int ch, int h, int w, int cols, int th,
                    int tw, long long total, float* __restrict__ tiles) {
    const long long quads = total / 4;
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < quads; q += (long long)gridDim.x * kThreads) {
        TilePos p = tile_pos(4 * q, N, ch, th, tw);
        float4 v;
        v.x = gather_one<FLIP>(image, g, p, ch, h, w, cols);
        tile_next(p, N, ch, th, tw);
        v.y = gather_one<FLIP>(image, g, p, ch, h, w, cols);
        tile_next(p, N, ch, th, tw);
        v.z = gather_one<FLIP>(image, g, p, ch, h, w, cols);
        tile_next(p, N, ch, th, tw);
        v.w = gather_one<FLIP>(image, g, p, ch, h, w, cols);
        reinterpret_cast<float4*>(tiles)[q] = v;       // tiles is 16-byte aligned (checked by the entry point)
    }
    if (blockIdx.x == 0 && threadIdx.x < (int)(total - 4 * quads)) {
        const long long o = 4 * quads + threadIdx.x;
        tiles[o] = gather_one<FLIP>(image, g, tile_pos(o, N, ch, th, tw), ch, h, w, cols);
    }
}

struct SlidePass {
    const float* p;
    int lh, lw, hs, ws, th, tw, rows, cols, flip;
    float weight;
    float sY, sX;   // hs -> H, ws -> W
    float sh, sw;   // lh -> th, lw -> tw
};
struct SlideBatch {
    SlidePass m[kMaxPasses];
};

// number of tiles along one axis that cover position v: origin <= v < origin + extent
__device__ __forceinline__ int cover_count(const int* org, int n, int extent, int v) {
    int cnt = 0;
    for (int i = 0; i < n; ++i) cnt += (org[i] <= v && v < org[i] + extent) ? 1 : 0;
    return cnt;
}

// the taps of a pass are recomputed per chunk of classes (19 classes: once); pixel loop and epilogue: vote_core.h
template <bool ALIGN, int CHUNK>
__global__ void __launch_bounds__(kThreads)
slide_vote_kernel(const SlideBatch batch, int n_passes, const int* __restrict__ table, const VoteOut out) {
    extern __shared__ unsigned int slide_lds[];
    int* org = reinterpret_cast<int*>(slide_lds);                 // [n_passes][kTabStride]
    unsigned int* hist = slide_lds + kMaxPasses * kTabStride;     // [lds_bins]
    for (int i = threadIdx.x; i < n_passes * kTabStride; i += kThreads) org[i] = table[i];
    bins_clear(hist, out.lds_bins);
    __syncthreads();
    const int N = out.N, C = out.C;
    vote_pixels<CHUNK>(out, hist, [&](float (&acc)[CHUNK], int n, int y, int x, int c0) {
        for (int k = 0; k < n_passes; ++k) {
            const SlidePass& m = batch.m[k];
            const int* ys = org + k * kTabStride;
            const int* xs = ys + kMaxAxis;
            const Lerp LY = lerp_of<ALIGN>(y, m.sY, m.hs), LX = lerp_of<ALIGN>(x, m.sX, m.ws);
            const long long plane = (long long)m.lh * m.lw;
            for (int a = 0; a < 2; ++a) {
                const float wy = a ? LY.l1 : LY.l0;
                // a tap of weight exactly 0 adds exact zeros for finite logits and is skipped; with an Inf or NaN
                // logit under such a tap the chain gives NaN (0 * Inf) where this kernel gives a finite score
                if (wy == 0.f) continue;
                const int Y = a ? LY.i1 : LY.i0;
                const int cnt_r = cover_count(ys, m.rows, m.th, Y);
                if (cnt_r == 0) continue;                    // (cannot happen with a validated table)
                const float wrow = m.weight * wy / (float)cnt_r;
                for (int r = 0; r < m.rows; ++r) {
                    const int oy = ys[r];
                    if (!(oy <= Y && Y < oy + m.th)) continue;
                    const Lerp R = lerp_of<ALIGN>(Y - oy, m.sh, m.lh);
                    const int ro0 = R.i0 * m.lw, ro1 = R.i1 * m.lw;
                    const float wr0 = wrow * R.l0, wr1 = wrow * R.l1;
                    for (int b = 0; b < 2; ++b) {
                        const float wx = b ? LX.l1 : LX.l0;
                        if (wx == 0.f) continue;
                        const int X0 = b ? LX.i1 : LX.i0;
                        const int X = m.flip ? m.ws - 1 - X0 : X0;
                        const int cnt_c = cover_count(xs, m.cols, m.tw, X);
                        if (cnt_c == 0) continue;
                        const float wcol = wx / (float)cnt_c;
                        for (int c = 0; c < m.cols; ++c) {
                            const int ox = xs[c];
                            if (!(ox <= X && X < ox + m.tw)) continue;
                            const Lerp Cl = lerp_of<ALIGN>(X - ox, m.sw, m.lw);
                            const float cw0 = wcol * Cl.l0, cw1 = wcol * Cl.l1;
                            const long long tile = (long long)r * m.cols + c;
                            const float* base = m.p + ((tile * N + n) * C + c0) * plane;
                            const float* r0 = base + ro0;
                            const float* r1 = base + ro1;
#pragma unroll
                            for (int j = 0; j < CHUNK; ++j) {
                                if (c0 + j < C) {
                                    const float* q0 = r0 + j * plane;
                                    const float* q1 = r1 + j * plane;
                                    acc[j] += wr0 * (cw0 * q0[Cl.i0] + cw1 * q0[Cl.i1]) +
                                              wr1 * (cw0 * q1[Cl.i0] + cw1 * q1[Cl.i1]);
                                }
                            }
                        }
                    }
                }
            }
        }
    });
}

// origins of one axis: 1 .. kMaxAxis of them, sorted, inside [0, size), every position of [0, size) under a tile
bool origins_ok(const int32_t* o, int n, int extent, int size) {
    if (n < 1 || n > kMaxAxis || extent <= 0 || size <= 0) return false;
    if (o[0] != 0) return false;
    for (int i = 0; i < n; ++i) {
        if (o[i] < 0 || o[i] >= size) return false;
        if (i && (o[i] < o[i - 1] || (long long)o[i] > (long long)o[i - 1] + extent)) return false;
    }
    return (long long)o[n - 1] + extent >= size;
}

}  // namespace

extern "C" int dcfp_gather_tiles_f32(const float* image, int N, int channels, int h, int w, const int32_t* ys, int rows,
                                     const int32_t* xs, int cols, int th, int tw, int flip, float* tiles,
                                     dcfp_stream_t stream) {
    if (!image || !tiles || !ys || !xs || N <= 0 || channels <= 0 || h <= 0 || w <= 0 || th <= 0 || tw <= 0 ||
        rows < 1 || rows > kMaxAxis || cols < 1 || cols > kMaxAxis || (flip != 0 && flip != 1) || !dcfp_aligned16(tiles))
        return DCFP_E_BADDESC;
    GatherArgs g;
    for (int i = 0; i < kMaxAxis; ++i) {
        g.ys[i] = ys[i < rows ? i : 0];
        g.xs[i] = xs[i < cols ? i : 0];
    }
    for (int i = 0; i < rows; ++i)
        if (ys[i] < 0 || ys[i] >= h) return DCFP_E_BADDESC;
    for (int i = 0; i < cols; ++i)
        if (xs[i] < 0 || xs[i] >= w) return DCFP_E_BADDESC;
    const long long total = (long long)rows * cols * N * channels * th * tw;
    long long blocks = (total / 4 + kThreads - 1) / kThreads;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    if (blocks < 1) blocks = 1;
    hipStream_t st = dcfp_s(stream);
    if (flip)
        hipLaunchKernelGGL((gather_tiles_kernel<true>), dim3((unsigned)blocks), dim3(kThreads), 0, st, image, g, N,
                           channels, h, w, cols, th, tw, total, tiles);
    else
        hipLaunchKernelGGL((gather_tiles_kernel<false>), dim3((unsigned)blocks), dim3(kThreads), 0, st, image, g, N,
                           channels, h, w, cols, th, tw, total, tiles);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_vote_sliding_f32(const DcfpSlidePass* passes, int n_passes, const int32_t* origins_host,
                                     const int32_t* origins_dev, int N, int C, int H, int W, int out_h, int out_w,
                                     int align_corners, float* scores, int32_t* pred, const int64_t* gt,
                                     int ignore_index, int64_t* conf, dcfp_stream_t stream) {
    if (!passes || !origins_host || !origins_dev || n_passes <= 0 || n_passes > kMaxPasses ||
        !vote_args_ok(N, C, H, W, out_h, out_w, scores, pred, gt, conf))
        return DCFP_E_BADDESC;
    SlideBatch batch;
    for (int k = 0; k < kMaxPasses; ++k) {
        const DcfpSlidePass& s = passes[k < n_passes ? k : 0];
        if (k < n_passes) {
            if (!s.logits || s.lh <= 0 || s.lw <= 0 || s.hs <= 0 || s.ws <= 0 || s.th <= 0 || s.tw <= 0 ||
                (s.flip != 0 && s.flip != 1) || !(s.weight == s.weight) || (long long)s.lh * s.lw > 0x7fffffffLL)
                return DCFP_E_BADDESC;
            const int32_t* o = origins_host + (long long)k * kTabStride;
            if (!origins_ok(o, s.rows, s.th, s.hs) || !origins_ok(o + kMaxAxis, s.cols, s.tw, s.ws))
                return DCFP_E_BADDESC;
        }
        SlidePass& m = batch.m[k];
        m.p = s.logits;
        m.lh = s.lh; m.lw = s.lw; m.hs = s.hs; m.ws = s.ws; m.th = s.th; m.tw = s.tw;
        m.rows = s.rows; m.cols = s.cols; m.flip = s.flip;
        m.weight = s.weight;
        m.sY = host_scale(s.hs, H, align_corners);
        m.sX = host_scale(s.ws, W, align_corners);
        m.sh = host_scale(s.lh, s.th, align_corners);
        m.sw = host_scale(s.lw, s.tw, align_corners);
    }
    const VoteLaunch L = vote_launch(N, C, out_h, out_w, scores, pred, gt, ignore_index, conf, kMaxPasses * kTabStride);
    vote_dispatch(align_corners, C, [&](auto align, auto chunk) {
        hipLaunchKernelGGL((slide_vote_kernel<decltype(align)::value, decltype(chunk)::value>), dim3(L.blocks),
                           dim3(kThreads), L.lds_bytes, dcfp_s(stream), batch, n_passes, origins_dev, L.out);
    });
    DCFP_RETURN_LAUNCH();
}
