// resize.hip — bilinear resize (F.interpolate, mode='bilinear') into / out of a channel slice of a batch-strided,
// row-pitched tensor: the DeepLabv3+ decoder (networks/deeplabv3p.py:31-40) resizes the ASPP output to the layer1
// resolution straight into channels [0, 512) of the pitched concat buffer that its first 3x3 conv reads.
//
// Forward: one thread per output column, kFwdRows output rows per block, the interpolation of upsample_fwd_kernel
// (upsample_ce.hip) with its roundings spelled out.  Dense operands go to upsample_fwd_kernel itself: the same bits as
// dcfp_upsample_bilinear_fwd_f32 (whose grid-stride loop rounds its vectorised body and its scalar tail differently).
// Only the W live floats of a row are written: the pitch tail and the channels outside the slice are untouched.
//
// Adjoint (dx (+)= interpolate^T(dy)), separable and gathered: a block owns BR rows x up to 256 columns of one dx
// plane.  It streams the dy rows that touch its band in chunks: each chunk is staged in LDS (read from global memory
// once), every thread reduces the columns of its dx column j (sum over X ascending of wx(X, j) * dy[Y, X]), then adds
// wy(Y, i) times that into its BR row accumulators (Y ascending).  Fixed order, no atomics: every run gives the same
// bits.  dy rows whose taps straddle two bands are read by both blocks (at a x2 ratio, 1-2 rows of ~34 per band).
#include "common.h"
#include "bilinear.h"

namespace {

using namespace dcfp_bilinear;

constexpr int kThreads = 256;
constexpr int kFwdRows = 8;          // output rows per forward block
constexpr int kBandRows = 16;        // dx rows per adjoint block
constexpr int kSegFloats = 8192;     // LDS floats for the staged dy rows of an adjoint chunk (32 KB)
constexpr int kMaxChunkRows = 16;

template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
resize_fwd_kernel(const float* __restrict__ x, long long x_nstride, int C, int h, int w, float* __restrict__ y,
                  long long y_nstride, int y_pitch, int H, int W, float sh, float sw) {
    const int plane = blockIdx.y;
    const int n = plane / C, c = plane - n * C;
    const float* p = x + (long long)n * x_nstride + (long long)c * h * w;
    float* q = y + (long long)n * y_nstride + (long long)c * H * y_pitch;
    const int Y0 = blockIdx.x * kFwdRows;
    for (int X = threadIdx.x; X < W; X += kThreads) {
        const Lerp Lw = lerp_of<ALIGN>(X, sw, w);
#pragma unroll
        for (int r = 0; r < kFwdRows; ++r) {
            const int Y = Y0 + r;
            if (Y >= H) break;
            const Lerp Lh = lerp_of<ALIGN>(Y, sh, h);
            // (the roundings the compiler chose for upsample_fwd_kernel's vectorised body, spelled out)
            const float top = __builtin_fmaf(Lw.l1, p[Lh.i0 * w + Lw.i1], Lw.l0 * p[Lh.i0 * w + Lw.i0]);
            const float bot = __builtin_fmaf(Lw.l1, p[Lh.i1 * w + Lw.i1], Lw.l0 * p[Lh.i1 * w + Lw.i0]);
            q[(long long)Y * y_pitch + X] = __builtin_fmaf(Lh.l0, top, Lh.l1 * bot);
        }
    }
}

// true when the taps of L put a non-zero weight on a source index in [a, b)
__device__ __forceinline__ bool touches(const Lerp& L, int a, int b) {
    return (L.i0 >= a && L.i0 < b && L.l0 != 0.f) || (L.i1 >= a && L.i1 < b && L.l1 != 0.f);
}

template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
resize_adjoint_kernel(const float* __restrict__ dy, long long dy_nstride, int dy_pitch, int C, int H, int W,
                      float* __restrict__ dx, long long dx_nstride, int h, int w, float sh, float sw, int tile_w,
                      int chunk_rows, int accumulate) {
    __shared__ float seg[kSegFloats];
    const int plane = blockIdx.z;
    const int n = plane / C, c = plane - n * C;
    const float* g = dy + (long long)n * dy_nstride + (long long)c * H * dy_pitch;
    float* o = dx + (long long)n * dx_nstride + (long long)c * h * w;
    const int ia = blockIdx.y * kBandRows;
    const int ib = min(ia + kBandRows, h);            // dx rows [ia, ib)
    const int ja = blockIdx.x * tile_w;
    const int jb = min(ja + tile_w, w);               // dx columns [ja, jb)
    const int j = ja + (int)threadIdx.x;
    const bool live = threadIdx.x < (unsigned)tile_w && j < jb;

    // dy rows / columns with a non-zero weight on the band / the tile: dst_range's conservative span, trimmed
    int ylo, yhi, t0, t1, xlo, xhi;
    dst_range<ALIGN>(ia, sh, H, ylo, t0);
    dst_range<ALIGN>(ib - 1, sh, H, t1, yhi);
    dst_range<ALIGN>(ja, sw, W, xlo, t0);
    dst_range<ALIGN>(jb - 1, sw, W, t1, xhi);
    while (ylo < yhi && !touches(lerp_of<ALIGN>(ylo, sh, h), ia, ib)) ++ylo;
    while (yhi > ylo && !touches(lerp_of<ALIGN>(yhi, sh, h), ia, ib)) --yhi;
    while (xlo < xhi && !touches(lerp_of<ALIGN>(xlo, sw, w), ja, jb)) ++xlo;
    while (xhi > xlo && !touches(lerp_of<ALIGN>(xhi, sw, w), ja, jb)) --xhi;
    int segw = xhi - xlo + 1;
    if (segw * chunk_rows > kSegFloats) segw = kSegFloats / chunk_rows;   // (the host's bound keeps this from happening)
    // this thread's dx column: the dy columns with a non-zero weight on it, relative to xlo
    int ja_x = 0, jb_x = -1;
    if (live) {
        int lo, hi;
        dst_range<ALIGN>(j, sw, W, lo, hi);
        lo = max(lo, xlo); hi = min(hi, xlo + segw - 1);
        ja_x = hi + 1;
        for (int X = lo; X <= hi; ++X)
            if (tap_weight(lerp_of<ALIGN>(X, sw, w), j) != 0.f) { ja_x = min(ja_x, X); jb_x = X; }
        ja_x -= xlo; jb_x -= xlo;
    }

    float acc[kBandRows];
#pragma unroll
    for (int k = 0; k < kBandRows; ++k) acc[k] = 0.f;

    for (int y0 = ylo; y0 <= yhi; y0 += chunk_rows) {
        const int rows = min(chunk_rows, yhi - y0 + 1);
        const int cnt = rows * segw;
        __syncthreads();                              // the previous chunk has been consumed
        for (int e = threadIdx.x; e < cnt; e += kThreads) {
            const int r = e / segw, col = e - r * segw;
            seg[e] = g[(long long)(y0 + r) * dy_pitch + xlo + col];
        }
        __syncthreads();
        for (int r = 0; r < rows; ++r) {
            const int Y = y0 + r;
            const Lerp Lh = lerp_of<ALIGN>(Y, sh, h);
            if (Lh.i1 < ia || Lh.i0 >= ib) continue;
            float s = 0.f;                            // column reduction, X ascending
            for (int xc = ja_x; xc <= jb_x; ++xc)
                s += tap_weight(lerp_of<ALIGN>(xlo + xc, sw, w), j) * seg[r * segw + xc];
#pragma unroll
            for (int k = 0; k < kBandRows; ++k) {
                const float wy = tap_weight(Lh, ia + k);
                if (wy != 0.f) acc[k] += wy * s;
            }
        }
    }
    if (!live) return;
#pragma unroll
    for (int k = 0; k < kBandRows; ++k) {
        const int i = ia + k;
        if (i >= ib) break;
        float* d = o + (long long)i * w + j;
        *d = accumulate ? *d + acc[k] : acc[k];
    }
}

// Upper bound of the staged dy columns of a tile of `tw` dx columns (dst_range's span plus its margins).
inline long long seg_bound(int tw, int W, float sw) {
    if (!(sw > 0.f)) return W;
    const long long b = (long long)((double)(tw + 1) / (double)sw) + 8;
    return b < W ? b : W;
}

}  // namespace

extern "C" int dcfp_resize_bilinear_into_f32(const float* x, int64_t x_nstride, int N, int C, int h, int w,
                                             float* y, int64_t y_nstride, int y_pitch, int H, int W,
                                             int align_corners, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    if (N > 65535 || (long long)N * C > 65535) return DCFP_E_UNSUPPORTED;
    const int pitch = y_pitch ? y_pitch : W;
    if (pitch < W) return DCFP_E_BADDESC;
    if (x_nstride == 0) x_nstride = (int64_t)C * h * w;
    if (y_nstride == 0) y_nstride = (int64_t)C * H * pitch;
    if (x_nstride < (int64_t)C * h * w || y_nstride < (int64_t)C * H * pitch) return DCFP_E_BADDESC;
    if (pitch == W && x_nstride == (int64_t)C * h * w && y_nstride == (int64_t)C * H * W)   // dense: the same kernel, the same bits
        return dcfp_upsample_bilinear_fwd_f32(x, y, N, C, h, w, H, W, align_corners, stream);
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const dim3 grid((H + kFwdRows - 1) / kFwdRows, N * C);
    if (align_corners)
        hipLaunchKernelGGL(resize_fwd_kernel<true>, grid, dim3(kThreads), 0, dcfp_s(stream), x, (long long)x_nstride, C,
                           h, w, y, (long long)y_nstride, pitch, H, W, sh, sw);
    else
        hipLaunchKernelGGL(resize_fwd_kernel<false>, grid, dim3(kThreads), 0, dcfp_s(stream), x, (long long)x_nstride, C,
                           h, w, y, (long long)y_nstride, pitch, H, W, sh, sw);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_resize_bilinear_adjoint_f32(const float* dy, int64_t dy_nstride, int dy_pitch, int N, int C, int H,
                                                int W, float* dx, int64_t dx_nstride, int h, int w, int align_corners,
                                                int accumulate, dcfp_stream_t stream) {
    if (!dy || !dx || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    if ((long long)N * C > 65535) return DCFP_E_UNSUPPORTED;
    const int pitch = dy_pitch ? dy_pitch : W;
    if (pitch < W) return DCFP_E_BADDESC;
    if (dy_nstride == 0) dy_nstride = (int64_t)C * H * pitch;
    if (dx_nstride == 0) dx_nstride = (int64_t)C * h * w;
    if (dy_nstride < (int64_t)C * H * pitch || dx_nstride < (int64_t)C * h * w) return DCFP_E_BADDESC;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    // columns per block: up to 256, fewer where the dy columns they need would not fit the LDS chunk
    int tw = w < kThreads ? w : kThreads;
    while (tw > 1 && seg_bound(tw, W, sw) > kSegFloats) tw = (tw + 1) / 2;
    const long long sb = seg_bound(tw, W, sw);
    if (sb > kSegFloats) return DCFP_E_UNSUPPORTED;
    int rows = (int)(kSegFloats / sb);
    rows = rows < 1 ? 1 : (rows > kMaxChunkRows ? kMaxChunkRows : rows);
    const dim3 grid((w + tw - 1) / tw, (h + kBandRows - 1) / kBandRows, N * C);
    if (align_corners)
        hipLaunchKernelGGL(resize_adjoint_kernel<true>, grid, dim3(kThreads), 0, dcfp_s(stream), dy,
                           (long long)dy_nstride, pitch, C, H, W, dx, (long long)dx_nstride, h, w, sh, sw, tw, rows,
                           accumulate);
    else
        hipLaunchKernelGGL(resize_adjoint_kernel<false>, grid, dim3(kThreads), 0, dcfp_s(stream), dy,
                           (long long)dy_nstride, pitch, C, H, W, dx, (long long)dx_nstride, h, w, sh, sw, tw, rows,
                           accumulate);
    DCFP_RETURN_LAUNCH();
}
