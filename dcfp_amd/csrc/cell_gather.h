// cell_gather.h — the adjoint of the bilinear upsample organised by interpolation CELLS: the one gather behind the
// backward of every full-resolution loss (CE, weighted CE: upsample_ce.hip; Lovasz: lovasz.hip).
//
// The cell of a destination pixel is the low-resolution position (i0, j0) its stencil starts at; every destination pixel
// lies in exactly one cell and touches only that cell's four corners (i0|i1, j0|j1).  A per-output gather visits every
// destination pixel once per corner it touches - four evaluations of the loss per pixel and class; here a lane pair owns
// a cell and a window of CT classes [c0, c0 + CT), holds the four corner logit vectors in registers, evaluates each of
// its ~8 x 8 destination pixels ONCE (label, LSE, weight and the stencils once per pixel, not once per class and corner)
// and accumulates the four corner sums (4 x CT registers).  A workgroup covers a 7 x 15 tile of low-resolution outputs =
// 8 x 16 cells (one halo row / column above and left is recomputed by the neighbour: 1.2x instead of 4x), parks the
// corner sums in LDS and gathers, per output and class, the <= 4 (cell, corner) terms that land on it in a fixed order -
// no atomics, run-to-run bit-identical, and a window's result does not depend on any other window's logits.
//
// The tail window of a class count that is no multiple of CT holds nc < CT real classes: a phantom class is never
// loaded, never evaluated and never stored.  Full windows run without any of those guards (TAIL = false); the branch
// between the two is block-uniform.
//
// What a destination pixel contributes per class is the loss's, a functor:
//     struct Loss {
//         struct Pixel { float pw; ... };                 // pw: the pixel's factor on its four corner weights
//         bool pixel(long long q, Pixel& px) const;       // q = Y * W + X of the image; false: the pixel contributes nothing
//         float grad(const Pixel& px, int c, float v00, float v01, float v10, float v11, const Lerp& Lh,
//                    const Lerp& Lw) const;                // d loss / d z of class c0 + c from its four corner logits
//     };
// Everything inlines.  Floating-point contraction is fixed where an expression is parsed, so a file that turns it off
// (lovasz.hip) includes this header after its pragma and gets the accumulates below as separate multiplies and adds.
#pragma once
#include "bilinear.h"

namespace dcfp_cells {

using dcfp_bilinear::dst_range;
using dcfp_bilinear::Lerp;
using dcfp_bilinear::lerp_of;

constexpr int kCellTH = 7, kCellTW = 15, kCellThreads = 256;      // 8 x 16 cells x 2 lanes: four full waves, two
                                                                   // workgroups per CU at 219 registers (an 8 x 16 tile
                                                                   // with 320 threads left 3 of 8 wave slots empty)
constexpr int kCellCount = (kCellTH + 1) * (kCellTW + 1);

inline int cell_tiles_h(int h) { return (h + kCellTH - 1) / kCellTH; }
inline int cell_tiles_w(int w) { return (w + kCellTW - 1) / kCellTW; }

// block <-> (image, tile row, tile column, class window); the window varies fastest, so the blocks that read the same
// tile's labels and per-pixel maps are neighbours in dispatch order
struct CellBlock {
    int n, I0, J0, c0, nc;
};

// WHOLE: the class count is CT, so every block has the one full window (chunks == 1)
template <int CT, bool WHOLE>
__device__ __forceinline__ CellBlock cell_block(int C, int tiles_w, int tiles_h, int chunks) {
    int b = blockIdx.x;
    const int chunk = WHOLE ? 0 : b % chunks;
    if (!WHOLE) b /= chunks;
    const int tw = b % tiles_w;
    b /= tiles_w;
    CellBlock r;
    r.I0 = (b % tiles_h) * kCellTH;
    r.J0 = tw * kCellTW;
    r.n = b / tiles_h;
    r.c0 = chunk * CT;
    r.nc = WHOLE || C - r.c0 >= CT ? CT : C - r.c0;
    return r;
}

// base / out: logits / dlogits of (n, c0); corner: the workgroup's LDS; gs scales every stored value
template <bool ALIGN, int CT, bool TAIL, class Loss>
__device__ __forceinline__ void cell_gather_body(float (*corner)[4][CT + 1], const float* __restrict__ base,
                                                 const Loss& loss, int nc, int h, int w, int H, int W, float sh,
                                                 float sw, float gs, float* __restrict__ out, int I0, int J0) {
    const int tid = threadIdx.x;
    const long long plane = (long long)h * w;
    const int cell = tid >> 1, part = tid & 1;
    if (cell < kCellCount) {
        const int ci = I0 - 1 + cell / (kCellTW + 1), cj = J0 - 1 + cell % (kCellTW + 1);
        float a00[CT], a01[CT], a10[CT], a11[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) a00[c] = a01[c] = a10[c] = a11[c] = 0.f;
        if (ci >= 0 && ci < h && cj >= 0 && cj < w) {
            const int i1 = ci + (ci < h - 1 ? 1 : 0), j1 = cj + (cj < w - 1 ? 1 : 0);
            float p00[CT], p01[CT], p10[CT], p11[CT];
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                p00[c] = p01[c] = p10[c] = p11[c] = 0.f;
                if (TAIL && c >= nc) continue;
                const float* p = base + c * plane;
                p00[c] = p[ci * w + cj]; p01[c] = p[ci * w + j1];
                p10[c] = p[i1 * w + cj]; p11[c] = p[i1 * w + j1];
            }
            int ylo, yhi, xlo, xhi;
            dst_range<ALIGN>(ci, sh, H, ylo, yhi);
            dst_range<ALIGN>(cj, sw, W, xlo, xhi);
            for (int Y = ylo + part; Y <= yhi; Y += 2) {
                const Lerp Lh = lerp_of<ALIGN>(Y, sh, h);
                if (Lh.i0 != ci) continue;
                for (int X = xlo; X <= xhi; ++X) {
                    const Lerp Lw = lerp_of<ALIGN>(X, sw, w);
                    if (Lw.i0 != cj) continue;
                    typename Loss::Pixel px;
                    if (!loss.pixel((long long)Y * W + X, px)) continue;
                    const float w00 = Lh.l0 * Lw.l0 * px.pw, w01 = Lh.l0 * Lw.l1 * px.pw;
                    const float w10 = Lh.l1 * Lw.l0 * px.pw, w11 = Lh.l1 * Lw.l1 * px.pw;
#pragma unroll
                    for (int c = 0; c < CT; ++c) {
                        if (TAIL && c >= nc) continue;
                        const float g = loss.grad(px, c, p00[c], p01[c], p10[c], p11[c], Lh, Lw);
                        a00[c] += w00 * g; a01[c] += w01 * g;
                        a10[c] += w10 * g; a11[c] += w11 * g;
                    }
                }
            }
        }
        // the two lanes of a cell: even rows + odd rows, always in that order
#pragma unroll
        for (int c = 0; c < CT; ++c) {
            a00[c] += __shfl_xor(a00[c], 1, 64); a01[c] += __shfl_xor(a01[c], 1, 64);
            a10[c] += __shfl_xor(a10[c], 1, 64); a11[c] += __shfl_xor(a11[c], 1, 64);
        }
        if (part == 0) {
#pragma unroll
            for (int c = 0; c < CT; ++c) {
                corner[cell][0][c] = a00[c]; corner[cell][1][c] = a01[c];
                corner[cell][2][c] = a10[c]; corner[cell][3][c] = a11[c];
            }
        }
    }
    __syncthreads();
    // gather over the nc real classes of the window: output (i, j) collects corner (a, b) of cell (ci, cj) wherever
    // ci + (a && ci < h-1) == i and cj + (b && cj < w-1) == j; candidates are ci in {i-1, i}, cj in {j-1, j}; fixed
    // visiting order
    for (int o = tid; o < kCellTH * kCellTW * nc; o += kCellThreads) {
        const int c = o / (kCellTH * kCellTW);
        const int r = o - c * (kCellTH * kCellTW);
        const int li = r / kCellTW, lj = r - li * kCellTW;
        const int i = I0 + li, j = J0 + lj;
        if (i >= h || j >= w) continue;
        float acc = 0.f;
#pragma unroll
        for (int di = 0; di < 2; ++di) {
            const int ci = i - 1 + di;
            if (ci < 0) continue;
#pragma unroll
            for (int a = 0; a < 2; ++a) {
                if (ci + ((a && ci < h - 1) ? 1 : 0) != i) continue;
#pragma unroll
                for (int dj = 0; dj < 2; ++dj) {
                    const int cj = j - 1 + dj;
                    if (cj < 0) continue;
#pragma unroll
                    for (int bb = 0; bb < 2; ++bb) {
                        if (cj + ((bb && cj < w - 1) ? 1 : 0) != j) continue;
                        acc += corner[(li + di) * (kCellTW + 1) + (lj + dj)][a * 2 + bb][c];
                    }
                }
            }
        }
        out[c * plane + (long long)i * w + j] = acc * gs;
    }
}

// the block's window: full windows without the tail guards
template <bool ALIGN, int CT, bool WHOLE, class Loss>
__device__ __forceinline__ void cell_gather(float (*corner)[4][CT + 1], const float* __restrict__ base,
                                            const Loss& loss, const CellBlock& blk, int h, int w, int H, int W,
                                            float sh, float sw, float gs, float* __restrict__ out) {
    if (WHOLE || blk.nc == CT)
        cell_gather_body<ALIGN, CT, false>(corner, base, loss, blk.nc, h, w, H, W, sh, sw, gs, out, blk.I0, blk.J0);
    else
        cell_gather_body<ALIGN, CT, true>(corner, base, loss, blk.nc, h, w, H, W, sh, sw, gs, out, blk.I0, blk.J0);
}

}  // namespace dcfp_cells
