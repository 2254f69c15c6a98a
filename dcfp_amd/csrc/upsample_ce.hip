// upsample_ce.hip — bilinear upsample (F.interpolate, networks/deeplabv3.py:47,50) and its
// fusion with nn.CrossEntropyLoss(ignore_index, 'mean') (loss/criterion.py:60,65-67).
//
// The fused pair never materialises the N x C x H x W logits (637 MB per head at
// 4x19x1024x2048): forward reads the low-resolution logits (L1/L2 resident) and the
// labels, and keeps one float per pixel (log-sum-exp); backward GATHERS, per
// low-resolution cell and class, the contributions of the <= ~16x16 full-resolution
// pixels that touch that cell, so there are no float atomics and the result is
// run-to-run deterministic.
//
// Coordinate rules: bilinear.h (ATen's area_pixel_compute_scale / _source_index).
#include "common.h"
#include "bilinear.h"
#include "cell_gather.h"
#include "upsample_logits.h"
#include "vote_core.h"
#include <math.h>
#include <stdlib.h>

namespace {

constexpr int kThreads = dcfp_vote::kThreads;   // 256; the confusion kernels share vote_core.h's bin loops
constexpr int kLossBlocks = 2048;

using namespace dcfp_bilinear;   // Lerp, lerp_of, host_scale, with_align, dst_range, tap_weight (bilinear.h);
                                 // Pix, pix_of, Tap, tap_of, logit_of, logit_at, lse_step (upsample_logits.h)
using namespace dcfp_cells;      // the cell gather and its tile constants (cell_gather.h)

// ------------------------------------------------------------ plain upsample
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_fwd_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int h,
                    int w, int H, int W, float sh, float sw) {
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * kThreads) {
        const int X = (int)(idx % W);
        const long long t = idx / W;
        const int Y = (int)(t % H);
        const long long plane = t / H;
        const Lerp Lh = lerp_of<ALIGN>(Y, sh, h), Lw = lerp_of<ALIGN>(X, sw, w);
        const float* p = x + plane * (long long)h * w;
        const float top = Lw.l0 * p[Lh.i0 * w + Lw.i0] + Lw.l1 * p[Lh.i0 * w + Lw.i1];
        const float bot = Lw.l0 * p[Lh.i1 * w + Lw.i0] + Lw.l1 * p[Lh.i1 * w + Lw.i1];
        y[idx] = Lh.l0 * top + Lh.l1 * bot;
    }
}

template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_bwd_kernel(const float* __restrict__ dy, float* __restrict__ dx, long long total, int h,
                    int w, int H, int W, float sh, float sw) {
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * kThreads) {
        const int j = (int)(idx % w);
        const long long t = idx / w;
        const int i = (int)(t % h);
        const long long plane = t / h;
        const float* g = dy + plane * (long long)H * W;
        int ylo, yhi, xlo, xhi;
        dst_range<ALIGN>(i, sh, H, ylo, yhi);
        dst_range<ALIGN>(j, sw, W, xlo, xhi);
        float acc = 0.f;
        for (int Y = ylo; Y <= yhi; ++Y) {
            const float wy = tap_weight(lerp_of<ALIGN>(Y, sh, h), i);
            if (wy == 0.f) continue;
            float row = 0.f;
            for (int X = xlo; X <= xhi; ++X) {
                const float wx = tap_weight(lerp_of<ALIGN>(X, sw, w), j);
                if (wx != 0.f) row += wx * g[(long long)Y * W + X];
            }
            acc += wy * row;
        }
        dx[idx] = acc;
    }
}

// ------------------------------------------------------- fused upsample + CE
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_ce_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                       const uint8_t* __restrict__ keep, int ignore_index, int N, int C, int h,
                       int w, int H, int W, float sh, float sw, float* __restrict__ lse_out,
                       float* __restrict__ gt_prob, float* __restrict__ part) {
    __shared__ float red[4];
    const long long total = (long long)N * H * W;
    const long long plane = (long long)h * w;
    float loss = 0.f, cnt = 0.f;
    for (long long pix = (long long)blockIdx.x * kThreads + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * kThreads) {
        const Pix P = pix_of(pix, H, W);
        const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
        const float* base = logits + (long long)P.n * C * plane;
        const long long label = labels[pix];
        float m = -INFINITY, s = 0.f, zl = 0.f;
        for (int c = 0; c < C; ++c) {
            const float z = logit_at(base + c * plane, t);
            lse_step(z, m, s);
            if (c == label) zl = z;
        }
        const float lse = m + logf(s);
        const bool labelled = label != ignore_index;
        const bool valid = labelled && (!keep || keep[pix]);
        if (lse_out) lse_out[pix] = lse;
        if (gt_prob) gt_prob[pix] = labelled ? expf(zl - lse) : 1.f;
        if (valid) {
            loss += lse - zl;
            cnt += 1.f;
        }
    }
    const float t1 = block_sum_256(loss, red);
    const float t2 = block_sum_256(cnt, red);
    if (threadIdx.x == 0) {
        part[blockIdx.x * 2 + 0] = t1;
        part[blockIdx.x * 2 + 1] = t2;
    }
}

// One 256-thread block: thread t sums the partials t, t + 256, ... in fp64, then a fixed-order tree over the 256
// sums (deterministic; the single-thread loop this replaces took 134 us for 32 k partials).
__global__ void __launch_bounds__(256) loss_final_kernel(const float* __restrict__ part, int nblocks,
                                                         float* __restrict__ out2) {
    __shared__ double sa[256], sb[256];
    double a = 0.0, b = 0.0;
    for (int k = threadIdx.x; k < nblocks; k += 256) {
        const float2 v = *reinterpret_cast<const float2*>(part + 2 * k);
        a += (double)v.x;
        b += (double)v.y;
    }
    sa[threadIdx.x] = a; sb[threadIdx.x] = b;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { sa[threadIdx.x] += sa[threadIdx.x + s]; sb[threadIdx.x] += sb[threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out2[0] = (float)sa[0];
        out2[1] = (float)sb[0];
    }
}

// dlogits[n,c,i,j] = gs * sum_pix wy wx [pw] (softmax - onehot)   (gather form), thread <-> one element of dlogits.
// Plain CE: a nullable keep mask and grad_scale[0]; weighted CE: a weight map pw (0 where a pixel does not count) and
// grad_scale[n].  A pixel's factor is wx for plain and (wx * pw) for weighted: with an all-ones map the two are the
// same bits.
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_ce_bwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                       const uint8_t* __restrict__ keep /* nullable */, const float* __restrict__ pix_weight /* nullable */,
                       int ignore_index, int N, int C, int h, int w, int H, int W, float sh, float sw,
                       const float* __restrict__ lse, const float* __restrict__ grad_scale,
                       int scale_per_image /* grad_scale[n] instead of grad_scale[0] */, float* __restrict__ dlogits) {
    const long long total = (long long)N * C * h * w;
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * kThreads) {
        const int j = (int)(idx % w);
        long long t = idx / w;
        const int i = (int)(t % h);
        t /= h;
        const int c = (int)(t % C);
        const int n = (int)(t / C);
        const float* p = logits + ((long long)n * C + c) * h * w;
        const long long* lab = labels + (long long)n * H * W;
        const float* ls = lse + (long long)n * H * W;
        const uint8_t* kp = keep ? keep + (long long)n * H * W : nullptr;
        const float* wp = pix_weight ? pix_weight + (long long)n * H * W : nullptr;
        int ylo, yhi, xlo, xhi;
        dst_range<ALIGN>(i, sh, H, ylo, yhi);
        dst_range<ALIGN>(j, sw, W, xlo, xhi);
        float acc = 0.f;
        for (int Y = ylo; Y <= yhi; ++Y) {
            const Lerp Lh = lerp_of<ALIGN>(Y, sh, h);
            const float wy = tap_weight(Lh, i);
            if (wy == 0.f) continue;
            float row = 0.f;
            for (int X = xlo; X <= xhi; ++X) {
                const Lerp Lw = lerp_of<ALIGN>(X, sw, w);
                float wx = tap_weight(Lw, j);
                if (wx == 0.f) continue;
                const long long q = (long long)Y * W + X;
                const long long label = lab[q];
                if (label == ignore_index || (kp && !kp[q])) continue;
                if (wp) {
                    const float pwq = wp[q];
                    if (pwq == 0.f) continue;
                    wx *= pwq;
                }
                const float z = logit_at(p, tap_of(Lh, Lw, w));
                row += wx * (expf(z - ls[q]) - (label == c ? 1.f : 0.f));
            }
            acc += wy * row;
        }
        dlogits[idx] = acc * grad_scale[scale_per_image ? n : 0];
    }
}

// Same gradient, thread <-> one low-resolution pixel (n,i,j) with ALL classes in registers (CT of
// them, compile-time): the per-destination-pixel work that does not depend on the class — the two
// interpolation stencils, the tap weights, label, LSE — is done once instead of once per class
// (3.0 -> ~1 ms per head at 19 classes).  The logit interpolation keeps the forward's expression.
template <bool ALIGN, int CT>
__global__ void __launch_bounds__(kThreads)
upsample_ce_bwd_classes_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                               const uint8_t* __restrict__ keep, int ignore_index, int N, int h, int w,
                               int H, int W, float sh, float sw, const float* __restrict__ lse,
                               const float* __restrict__ grad_scale, float* __restrict__ dlogits,
                               const float* __restrict__ pix_weight /* GSRL weights, nullable */,
                               int scale_per_image /* grad_scale[n] instead of grad_scale[0] */) {
    // four lanes share one low-resolution pixel (destination rows Y = ylo + part, +4, ...) and
    // combine their partial sums with two butterfly shuffles: 4x the waves for latency hiding
    const long long total = (long long)N * h * w * 4;
    const long long plane = (long long)h * w;
    for (long long idx4 = (long long)blockIdx.x * kThreads + threadIdx.x; idx4 < total;
         idx4 += (long long)gridDim.x * kThreads) {
        const int part = (int)(idx4 & 3);
        const long long idx = idx4 >> 2;
        const int j = (int)(idx % w);
        const long long t = idx / w;
        const int i = (int)(t % h);
        const int n = (int)(t / h);
        const float* base = logits + (long long)n * CT * plane;
        const long long* lab = labels + (long long)n * H * W;
        const float* ls = lse + (long long)n * H * W;
        const uint8_t* kp = keep ? keep + (long long)n * H * W : nullptr;
        const float* wp = pix_weight ? pix_weight + (long long)n * H * W : nullptr;
        const float gs = grad_scale[scale_per_image ? n : 0];
        int ylo, yhi, xlo, xhi;
        dst_range<ALIGN>(i, sh, H, ylo, yhi);
        dst_range<ALIGN>(j, sw, W, xlo, xhi);
        float acc[CT];
#pragma unroll
        for (int c = 0; c < CT; ++c) acc[c] = 0.f;
        for (int Y = ylo + part; Y <= yhi; Y += 4) {
            const Lerp Lh = lerp_of<ALIGN>(Y, sh, h);
            const float wy = tap_weight(Lh, i);
            if (wy == 0.f) continue;
            for (int X = xlo; X <= xhi; ++X) {
                const Lerp Lw = lerp_of<ALIGN>(X, sw, w);
                float wgt = wy * tap_weight(Lw, j);
                if (wgt == 0.f) continue;
                const long long q = (long long)Y * W + X;
                const long long label = lab[q];
                if (label == ignore_index || (kp && !kp[q])) continue;
                if (wp) {
                    const float pwq = wp[q];
                    if (pwq == 0.f) continue;
                    wgt *= pwq;
                }
                const Tap t = tap_of(Lh, Lw, w);
                const float lq = ls[q];
#pragma unroll
                for (int c = 0; c < CT; ++c)
                    acc[c] += wgt * (expf(logit_at(base + c * plane, t) - lq) - (label == c ? 1.f : 0.f));
            }
        }
#pragma unroll
        for (int c = 0; c < CT; ++c) {   // fixed combination order: (p0+p1)+(p2+p3)
            acc[c] += __shfl_xor(acc[c], 1, 64);
            acc[c] += __shfl_xor(acc[c], 2, 64);
        }
        if (part == 0) {
            float* o = dlogits + (long long)n * CT * plane + (long long)i * w + j;
#pragma unroll
            for (int c = 0; c < CT; ++c) o[c * plane] = acc[c] * gs;
        }
    }
}

// The same gradient organised by interpolation CELLS (cell_gather.h): each destination pixel is evaluated once per
// window of CT classes instead of once per class and corner (four softmax evaluations), and the class-independent work
// of a pixel - stencils, label, LSE, weight - is repeated ceil(C / CT) times instead of C times.  Once the per-pixel LSE
// is known the softmax factorises over classes, so a workgroup works on the window [c0, c0 + CT) of the C-class tensor
// alone; one launch covers every window.  Interpolation and softmax expressions are the forward's.
//
// Two instantiations: CT = kCeChunk for any class count (Pascal-Context 59, ADE 150, COCO-Stuff 171), and CT = 19 with
// WHOLE set, where Cityscapes' classes are the one full window (the "cells19" route of the training path: no chunk
// decode, never a tail).  Times of both against the separate 19-class kernel this replaced: DESIGN §13a.
//
// Budget: 8 x CT corner / accumulator registers per lane (216 VGPRs at 19, 211 at 20, of the 256 that two workgroups
// of four waves per CU leave each lane), LDS 128 x 4 x (CT + 1) x 4 B = 40 KB at 19, 42 KB at 20 per workgroup.
#ifndef DCFP_CE_CHUNK
#define DCFP_CE_CHUNK 20          // the chunk width; the candidates' times are in DESIGN §13a
#endif
constexpr int kCeChunk = DCFP_CE_CHUNK;
constexpr int kCeChunkMinC = 2;   // the smallest class count timed; faster than the per-output kernels from there on
                                  // (DESIGN §13a).  C == 1 (gradient identically zero) stays where it was

// what a destination pixel contributes to class c0 + c: pw * (softmax - onehot).
//
// ROUNDING19 spells out how z is rounded in the 19-class instantiation.  With contraction left to the compiler, which of
// the two products of a row w0 * v00 + w1 * v01 is fused into the add depends on the code around the expression, and
// the 19-class kernel, when it was a kernel of its own, came out as fma(w0, v00, w1 * v01) per row and an unfused
// h0 * top + h1 * bot, while the chunked kernel, through logit_of(), comes out as fma(w1, v01, w0 * v00) per row.  The
// training path's gradients keep their bits, so that choice is written down here instead of being left to chance.
template <bool ROUNDING19>
struct CeCellLoss {
    const long long* __restrict__ lab;      // of the image
    const uint8_t* __restrict__ kp;         // nullable
    const float* __restrict__ wp;           // GSRL weights, nullable
    const float* __restrict__ ls;
    int ignore_index, c0;

    struct Pixel {
        float pw, lq;
        long long lrel;                     // the label's position in this window, if it is in it
    };

    __device__ __forceinline__ bool pixel(long long q, Pixel& px) const {
        const long long label = lab[q];
        if (label == ignore_index || (kp && !kp[q])) return false;
        px.pw = 1.f;
        if (wp) {
            px.pw = wp[q];
            if (px.pw == 0.f) return false;
        }
        px.lq = ls[q];
        px.lrel = label - c0;
        return true;
    }

    __device__ __forceinline__ float grad(const Pixel& px, int c, float v00, float v01, float v10, float v11,
                                          const Lerp& Lh, const Lerp& Lw) const {
        float z;
        if (ROUNDING19) {
#pragma clang fp contract(off)
            const float top = __builtin_fmaf(Lw.l0, v00, Lw.l1 * v01), bot = __builtin_fmaf(Lw.l0, v10, Lw.l1 * v11);
            z = Lh.l0 * top + Lh.l1 * bot;
        } else {
            z = logit_of(v00, v01, v10, v11, Lh.l0, Lh.l1, Lw.l0, Lw.l1);
        }
        return expf(z - px.lq) - (px.lrel == c ? 1.f : 0.f);
    }
};

template <bool ALIGN, int CT, bool WHOLE /* C == CT: the cells19 route */>
__global__ void __launch_bounds__(kCellThreads, 2)
ce_bwd_cells_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                    const uint8_t* __restrict__ keep, int ignore_index, int C, int h, int w, int H, int W, float sh,
                    float sw, const float* __restrict__ lse, const float* __restrict__ grad_scale,
                    float* __restrict__ dlogits, const float* __restrict__ pix_weight, int scale_per_image,
                    int tiles_w, int tiles_h, int chunks) {
    __shared__ float corner[kCellCount][4][CT + 1];
    const CellBlock blk = cell_block<CT, WHOLE>(C, tiles_w, tiles_h, chunks);
    const long long img = (long long)blk.n * H * W;
    const long long first = ((long long)blk.n * C + blk.c0) * h * w;      // (n, c0): batch stride C * plane, not CT
    const CeCellLoss<WHOLE> loss{labels + img, keep ? keep + img : nullptr, pix_weight ? pix_weight + img : nullptr,
                          lse + img,    ignore_index,                blk.c0};
    cell_gather<ALIGN, CT, WHOLE>(corner, logits + first, loss, blk, h, w, H, W, sh, sw,
                           grad_scale[scale_per_image ? blk.n : 0], dlogits + first);
}

// OHEM threshold search input (loss/ohem.py:20-33): the reference zooms the full-resolution
// softmax to 1/factor with scipy.ndimage.zoom(order=1) and the labels with order=0, then
// gathers the zoomed probability of the zoomed label.  Per zoomed position that is a bilinear
// blend of prob_L at four full-resolution pixels, L = nearest label — computed here from the
// low-resolution logits and the per-pixel LSE without ever forming the probability tensor.
// scipy's coordinate rule (grid_mode=False): src = o * (in-1)/(out-1), evaluated in double.
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
ohem_zoom_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                 const float* __restrict__ lse, int N, int C, int h, int w, int H, int W,
                 float sh, float sw, int H8, int W8, float* __restrict__ pred8,
                 int* __restrict__ lab8) {
    const long long total = (long long)N * H8 * W8;
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * kThreads) {
        const int ox = (int)(idx % W8);
        const long long t = idx / W8;
        const int oy = (int)(t % H8);
        const int n = (int)(t / H8);
        const double cy = H8 > 1 ? (double)oy * (double)(H - 1) / (double)(H8 - 1) : 0.0;
        const double cx = W8 > 1 ? (double)ox * (double)(W - 1) / (double)(W8 - 1) : 0.0;
        int ny = (int)floor(cy + 0.5), nx = (int)floor(cx + 0.5);
        ny = ny > H - 1 ? H - 1 : ny; nx = nx > W - 1 ? W - 1 : nx;
        const long long L = labels[((long long)n * H + ny) * W + nx];
        lab8[idx] = (int)L;
        float out = 0.f;
        if (L >= 0 && L < C) {
            const int y0 = (int)floor(cy), x0 = (int)floor(cx);
            const double ty = cy - y0, tx = cx - x0;
            const float* p = logits + ((long long)n * C + L) * h * w;
            double acc = 0.0;
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx) {
                    const int Y = y0 + dy, X = x0 + dx;
                    const double wgt = (dy ? ty : 1.0 - ty) * (dx ? tx : 1.0 - tx);
                    if (Y > H - 1 || X > W - 1 || wgt == 0.0) continue;   // mode='constant', cval=0
                    const float z = logit_at(p, tap_of(lerp_of<ALIGN>(Y, sh, h), lerp_of<ALIGN>(X, sw, w), w));
                    acc += wgt * (double)expf(z - lse[((long long)n * H + Y) * W + X]);
                }
            }
            out = (float)acc;
        }
        pred8[idx] = out;
    }
}

// ---- GSRL (loss/criterion.py:77-101): margin map, k x k stride-1 max filter, per-pixel-weighted CE
// margin[pix] = p1 - p2 (two largest softmax probabilities of the interpolated logits)
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_margin_kernel(const float* __restrict__ logits, int N, int C, int h, int w, int H, int W,
                       float sh, float sw, float* __restrict__ margin) {
    const long long total = (long long)N * H * W;
    const long long plane = (long long)h * w;
    for (long long pix = (long long)blockIdx.x * kThreads + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * kThreads) {
        const Pix P = pix_of(pix, H, W);
        const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
        const float* base = logits + (long long)P.n * C * plane;
        float m1 = -INFINITY, m2 = -INFINITY, s = 0.f;      // the running log-sum-exp, and the runner-up m2
        for (int c = 0; c < C; ++c) {
            const float z = logit_at(base + c * plane, t);
            const float lower = z > m1 ? m1 : z;            // whichever of (z, m1) is not the maximum after this step
            lse_step(z, m1, s);
            m2 = lower > m2 ? lower : m2;
        }
        // p1 = exp(m1 - lse) = 1/s ; p2 = exp(m2 - m1)/s
        margin[pix] = (1.f - (C > 1 ? expf(m2 - m1) : 0.f)) / s;
    }
}

// y = max over the k x k window (stride 1, pad k/2, -inf padding) of a [planes,H,W] map
__global__ void __launch_bounds__(kThreads)
maxfilter_kernel(const float* __restrict__ x, float* __restrict__ y, long long total, int H, int W,
                 int k) {
    const int r = k / 2;
    for (long long idx = (long long)blockIdx.x * kThreads + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * kThreads) {
        const int X = (int)(idx % W);
        const long long t = idx / W;
        const int Y = (int)(t % H);
        const float* xp = x + (t / H) * (long long)H * W;
        const int y0 = Y - r < 0 ? 0 : Y - r, y1 = Y + (k - 1 - r) > H - 1 ? H - 1 : Y + (k - 1 - r);
        const int x0 = X - r < 0 ? 0 : X - r, x1 = X + (k - 1 - r) > W - 1 ? W - 1 : X + (k - 1 - r);
        float best = -INFINITY;
        for (int yy = y0; yy <= y1; ++yy)
            for (int xx = x0; xx <= x1; ++xx) {
                const float v = xp[yy * W + xx];
                best = (v > best || v != v) ? v : best;
            }
        y[idx] = best;
    }
}

// per-image sums  out[n] = (sum_pix w*ce, sum_pix w)  with w = pix_weight (0 where ignored)
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_wce_fwd_kernel(const float* __restrict__ logits, const long long* __restrict__ labels,
                        const float* __restrict__ pw, int ignore_index, int C, int h, int w, int H,
                        int W, float sh, float sw, float* __restrict__ lse_out,
                        float* __restrict__ part /* [N][gridDim.x][2] */) {
    __shared__ float red[4];
    const int n = blockIdx.y;
    const long long HWl = (long long)H * W;
    const long long plane = (long long)h * w;
    const float* base = logits + (long long)n * C * plane;
    float a = 0.f, b = 0.f;
    for (long long q = (long long)blockIdx.x * kThreads + threadIdx.x; q < HWl;
         q += (long long)gridDim.x * kThreads) {
        const int X = (int)(q % W), Y = (int)(q / W);
        const long long pix = n * HWl + q;
        const Tap t = tap_of(lerp_of<ALIGN>(Y, sh, h), lerp_of<ALIGN>(X, sw, w), w);
        const long long label = labels[pix];
        float m = -INFINITY, s = 0.f, zl = 0.f;
        for (int c = 0; c < C; ++c) {
            const float z = logit_at(base + c * plane, t);
            lse_step(z, m, s);
            if (c == label) zl = z;
        }
        const float lse = m + logf(s);
        if (lse_out) lse_out[pix] = lse;
        const float wgt = pw[pix];
        if (label != ignore_index) a += wgt * (lse - zl);   // CE(reduction='none') is 0 where ignored
        b += wgt;
    }
    const float t1 = block_sum_256(a, red);
    const float t2 = block_sum_256(b, red);
    if (threadIdx.x == 0) {
        part[((long long)n * gridDim.x + blockIdx.x) * 2 + 0] = t1;
        part[((long long)n * gridDim.x + blockIdx.x) * 2 + 1] = t2;
    }
}

__global__ void wce_final_kernel(const float* __restrict__ part, int nblocks, float* __restrict__ out) {
    const int n = blockIdx.x;
    if (threadIdx.x != 0) return;
    double a = 0.0, b = 0.0;
    for (int k = 0; k < nblocks; ++k) {
        a += (double)part[((long long)n * nblocks + k) * 2];
        b += (double)part[((long long)n * nblocks + k) * 2 + 1];
    }
    out[2 * n] = (float)a;
    out[2 * n + 1] = (float)b;
}

template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
upsample_argmax_kernel(const float* __restrict__ logits, int N, int C, int h, int w, int H, int W,
                       float sh, float sw, int* __restrict__ pred) {
    const long long total = (long long)N * H * W;
    const long long plane = (long long)h * w;
    for (long long pix = (long long)blockIdx.x * kThreads + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * kThreads) {
        const Pix P = pix_of(pix, H, W);
        const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
        const float* base = logits + (long long)P.n * C * plane;
        float best = -INFINITY;
        int bi = 0;
        for (int c = 0; c < C; ++c) {
            const float z = logit_at(base + c * plane, t);
            if (z > best) { best = z; bi = c; }     // first maximum wins, like torch.argmax / np.argmax
        }
        pred[pix] = bi;
    }
}

// per-block LDS histogram (C*C <= 4096 bins), then one integer atomic per non-empty bin; the bins, and the rule for a
// label outside the classes, are vote_core.h's.  pred comes from outside: a prediction that is no class is skipped too.
__global__ void __launch_bounds__(kThreads)
confusion_kernel(const int* __restrict__ pred, const long long* __restrict__ gt, int ignore_index,
                 long long n, int C, unsigned long long* __restrict__ conf) {
    extern __shared__ unsigned int hist[];
    const int bins = C * C;
    dcfp_vote::bins_clear(hist, bins);
    __syncthreads();
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n;
         i += (long long)gridDim.x * kThreads) {
        const int p = pred[i];
        if (p >= 0 && p < C) dcfp_vote::bins_count(hist, bins, conf, gt[i], p, C, ignore_index);
    }
    dcfp_vote::bins_flush(hist, bins, conf);
}

__global__ void __launch_bounds__(kThreads)
confusion_global_kernel(const int* __restrict__ pred, const long long* __restrict__ gt, int ignore_index,
                        long long n, int C, unsigned long long* __restrict__ conf) {
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n;
         i += (long long)gridDim.x * kThreads) {
        const int p = pred[i];
        if (p >= 0 && p < C) dcfp_vote::bins_count(nullptr, 0, conf, gt[i], p, C, ignore_index);
    }
}

inline unsigned stream_grid(long long total) {
    long long b = (total + kThreads - 1) / kThreads;
    if (b > 256 * 16) b = 256 * 16;
    if (b < 1) b = 1;
    return (unsigned)b;
}

}  // namespace

extern "C" int dcfp_upsample_bilinear_fwd_f32(const float* x, float* y, int N, int C, int h, int w,
                                              int H, int W, int align_corners,
                                              dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    const long long total = (long long)N * C * H * W;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(upsample_fwd_kernel<A.value>, dim3(stream_grid(total)), dim3(kThreads), 0,
                           dcfp_s(stream), x, y, total, h, w, H, W, sh, sw);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_upsample_bilinear_bwd_f32(const float* dy, float* dx, int N, int C, int h,
                                              int w, int H, int W, int align_corners,
                                              dcfp_stream_t stream) {
    if (!dy || !dx || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    const long long total = (long long)N * C * h * w;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(upsample_bwd_kernel<A.value>, dim3(stream_grid(total)), dim3(kThreads), 0,
                           dcfp_s(stream), dy, dx, total, h, w, H, W, sh, sw);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" size_t dcfp_upsample_ce_workspace_bytes(int N, int H, int W) {
    (void)N; (void)H; (void)W;
    return (size_t)kLossBlocks * 2 * sizeof(float);
}

extern "C" int dcfp_upsample_ce_fwd_f32(const float* logits, const int64_t* labels,
                                        const uint8_t* pixel_keep, int ignore_index, int N, int C,
                                        int h, int w, int H, int W, int align_corners, float* lse,
                                        float* gt_prob, float* out2, void* workspace,
                                        size_t workspace_bytes, dcfp_stream_t stream) {
    if (!logits || !labels || !out2 || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return DCFP_E_BADDESC;
    if (!workspace || workspace_bytes < (size_t)kLossBlocks * 2 * sizeof(float))
        return DCFP_E_WORKSPACE;
    const long long total = (long long)N * H * W;
    long long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > kLossBlocks) blocks = kLossBlocks;
    float* part = static_cast<float*>(workspace);
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(upsample_ce_fwd_kernel<A.value>, dim3((unsigned)blocks), dim3(kThreads), 0,
                           dcfp_s(stream), logits, lab, pixel_keep, ignore_index, N, C, h, w, H, W,
                           sh, sw, lse, gt_prob, part);
    });
    hipLaunchKernelGGL(loss_final_kernel, dim3(1), dim3(256), 0, dcfp_s(stream), part, (int)blocks,
                       out2);
    DCFP_RETURN_LAUNCH();
}

// Which backward kernel a shape gets: the one decision launch_ce_bwd and dcfp_upsample_ce_bwd_plan make.
enum { kCePlanCells19 = 0, kCePlanCellsChunked = 1, kCePlanPerOutput = 2 };
struct CeBwdPlan { int variant, chunk_width, chunks; };

static CeBwdPlan ce_bwd_plan(int N, int C, int h, int w) {
    static const bool cells = [] { const char* e = getenv("DCFP_CE_BWD_CELLS"); return !e || atoi(e) != 0; }();
    const int CT = C == 19 ? 19 : kCeChunk;   // Cityscapes (datasets/CSdatasets.py:13): all classes in one window
    const int chunks = (C + CT - 1) / CT;
    const long long tiles = (long long)N * cell_tiles_h(h) * cell_tiles_w(w);
    if (cells && C >= kCeChunkMinC && tiles * chunks <= 0x7fffffffLL)     // the cell kernels' 32-bit block count
        return CeBwdPlan{C == 19 ? kCePlanCells19 : kCePlanCellsChunked, CT, chunks};
    return CeBwdPlan{kCePlanPerOutput, 0, 0};
}

extern "C" int dcfp_upsample_ce_bwd_plan(int N, int C, int h, int w, int H, int W, int* variant, int* chunk_width,
                                         int* chunks) {
    if (!variant || !chunk_width || !chunks || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return DCFP_E_BADDESC;
    if (((long long)N * C * h * w + kThreads - 1) / kThreads > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    const CeBwdPlan plan = ce_bwd_plan(N, C, h, w);
    *variant = plan.variant;
    *chunk_width = plan.chunk_width;
    *chunks = plan.chunks;
    return DCFP_OK;
}

// The backward of plain CE (nullable keep mask, grad_scale[0]) and of weighted CE (weight map, grad_scale[n]), on the
// route ce_bwd_plan names.  The per-output route at 19 classes is upsample_ce_bwd_classes_kernel, the A/B partner of
// the cell kernel under DCFP_CE_BWD_CELLS=0.
static int launch_ce_bwd(const float* logits, const int64_t* labels, const uint8_t* keep, const float* pix_weight,
                         int per_image, int ignore_index, int N, int C, int h, int w, int H, int W, int align_corners,
                         const float* lse, const float* gscale, float* dlogits, hipStream_t st) {
    const long long blocks = ((long long)N * C * h * w + kThreads - 1) / kThreads;
    if (blocks > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    const CeBwdPlan plan = ce_bwd_plan(N, C, h, w);
    const int tiles_w = cell_tiles_w(w), tiles_h = cell_tiles_h(h);
    const dim3 cell_grid((unsigned)((long long)N * tiles_h * tiles_w * plan.chunks));
    with_align(align_corners, [&](auto A) {
        if (plan.variant == kCePlanCells19)
            hipLaunchKernelGGL((ce_bwd_cells_kernel<A.value, 19, true>), cell_grid, dim3(kCellThreads), 0, st, logits, lab, keep,
                               ignore_index, C, h, w, H, W, sh, sw, lse, gscale, dlogits, pix_weight, per_image, tiles_w,
                               tiles_h, plan.chunks);
        else if (plan.variant == kCePlanCellsChunked)
            hipLaunchKernelGGL((ce_bwd_cells_kernel<A.value, kCeChunk, false>), cell_grid, dim3(kCellThreads), 0, st, logits, lab,
                               keep, ignore_index, C, h, w, H, W, sh, sw, lse, gscale, dlogits, pix_weight, per_image,
                               tiles_w, tiles_h, plan.chunks);
        else if (C == 19)   // 4 lanes per low-resolution pixel
            hipLaunchKernelGGL((upsample_ce_bwd_classes_kernel<A.value, 19>),
                               dim3((unsigned)(((long long)N * h * w * 4 + kThreads - 1) / kThreads)), dim3(kThreads), 0,
                               st, logits, lab, keep, ignore_index, N, h, w, H, W, sh, sw, lse, gscale, dlogits,
                               pix_weight, per_image);
        else
            hipLaunchKernelGGL(upsample_ce_bwd_kernel<A.value>, dim3((unsigned)blocks), dim3(kThreads), 0, st, logits, lab,
                               keep, pix_weight, ignore_index, N, C, h, w, H, W, sh, sw, lse, gscale, per_image, dlogits);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_upsample_ce_bwd_f32(const float* logits, const int64_t* labels,
                                        const uint8_t* pixel_keep, int ignore_index, int N, int C,
                                        int h, int w, int H, int W, int align_corners,
                                        const float* lse, const float* grad_scale, float* dlogits,
                                        dcfp_stream_t stream) {
    if (!logits || !labels || !lse || !grad_scale || !dlogits || N <= 0 || C <= 0 || h <= 0 ||
        w <= 0 || H <= 0 || W <= 0)
        return DCFP_E_BADDESC;
    return launch_ce_bwd(logits, labels, pixel_keep, nullptr, 0, ignore_index, N, C, h, w, H, W, align_corners, lse,
                         grad_scale, dlogits, dcfp_s(stream));
}

extern "C" int dcfp_ohem_zoom_gt_prob_f32(const float* logits, const int64_t* labels, const float* lse,
                                          int N, int C, int h, int w, int H, int W,
                                          int align_corners, int H8, int W8, float* pred8,
                                          int32_t* lab8, dcfp_stream_t stream) {
    if (!logits || !labels || !lse || !pred8 || !lab8 || N <= 0 || C <= 0 || h <= 0 || w <= 0 ||
        H <= 0 || W <= 0 || H8 <= 0 || W8 <= 0)
        return DCFP_E_BADDESC;
    const long long total = (long long)N * H8 * W8;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(ohem_zoom_kernel<A.value>, dim3(stream_grid(total)), dim3(kThreads), 0,
                           dcfp_s(stream), logits, lab, lse, N, C, h, w, H, W, sh, sw, H8, W8, pred8, lab8);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_upsample_margin_f32(const float* logits, int N, int C, int h, int w, int H, int W,
                                        int align_corners, float* margin, dcfp_stream_t stream) {
    if (!logits || !margin || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    const long long total = (long long)N * H * W;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(upsample_margin_kernel<A.value>, dim3(stream_grid(total)), dim3(kThreads), 0,
                           dcfp_s(stream), logits, N, C, h, w, H, W, sh, sw, margin);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_maxfilter2d_s1_f32(const float* x, float* y, int planes, int H, int W, int k,
                                       dcfp_stream_t stream) {
    if (!x || !y || planes <= 0 || H <= 0 || W <= 0 || k <= 0 || (k & 1) == 0) return DCFP_E_BADDESC;
    const long long total = (long long)planes * H * W;
    hipLaunchKernelGGL(maxfilter_kernel, dim3(stream_grid(total)), dim3(kThreads), 0, dcfp_s(stream), x, y,
                       total, H, W, k);
    DCFP_RETURN_LAUNCH();
}

constexpr int kWceBlocks = 512;   // per image

extern "C" size_t dcfp_upsample_wce_workspace_bytes(int N, int H, int W) {
    (void)H; (void)W;
    return (size_t)(N > 0 ? N : 0) * kWceBlocks * 2 * sizeof(float);
}

extern "C" int dcfp_upsample_wce_fwd_f32(const float* logits, const int64_t* labels,
                                         const float* pix_weight, int ignore_index, int N, int C, int h,
                                         int w, int H, int W, int align_corners, float* lse,
                                         float* out_per_image, void* workspace, size_t workspace_bytes,
                                         dcfp_stream_t stream) {
    if (!logits || !labels || !pix_weight || !out_per_image || N <= 0 || C <= 0 || h <= 0 || w <= 0 ||
        H <= 0 || W <= 0 || N > 65535)
        return DCFP_E_BADDESC;
    if (!workspace || workspace_bytes < (size_t)N * kWceBlocks * 2 * sizeof(float)) return DCFP_E_WORKSPACE;
    long long blocks = ((long long)H * W + kThreads - 1) / kThreads;
    if (blocks > kWceBlocks) blocks = kWceBlocks;
    float* part = static_cast<float*>(workspace);
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    dim3 grid((unsigned)blocks, (unsigned)N);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(upsample_wce_fwd_kernel<A.value>, grid, dim3(kThreads), 0, dcfp_s(stream), logits, lab,
                           pix_weight, ignore_index, C, h, w, H, W, sh, sw, lse, part);
    });
    hipLaunchKernelGGL(wce_final_kernel, dim3((unsigned)N), dim3(64), 0, dcfp_s(stream), part, (int)blocks,
                       out_per_image);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_upsample_wce_bwd_f32(const float* logits, const int64_t* labels,
                                         const float* pix_weight, int ignore_index, int N, int C, int h,
                                         int w, int H, int W, int align_corners, const float* lse,
                                         const float* grad_scale_per_image, float* dlogits,
                                         dcfp_stream_t stream) {
    if (!logits || !labels || !pix_weight || !lse || !grad_scale_per_image || !dlogits || N <= 0 ||
        C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0)
        return DCFP_E_BADDESC;
    return launch_ce_bwd(logits, labels, nullptr, pix_weight, 1, ignore_index, N, C, h, w, H, W, align_corners, lse,
                         grad_scale_per_image, dlogits, dcfp_s(stream));
}

extern "C" int dcfp_upsample_argmax_f32(const float* logits, int N, int C, int h, int w, int H, int W,
                                        int align_corners, int32_t* pred, dcfp_stream_t stream) {
    if (!logits || !pred || N <= 0 || C <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0) return DCFP_E_BADDESC;
    const long long total = (long long)N * H * W;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(upsample_argmax_kernel<A.value>, dim3(stream_grid(total)), dim3(kThreads), 0,
                           dcfp_s(stream), logits, N, C, h, w, H, W, sh, sw, pred);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_confusion_matrix_i64(const int32_t* pred, const int64_t* gt, int ignore_index,
                                         int64_t n_pixels, int C, int64_t* conf, dcfp_stream_t stream) {
    if (!conf || n_pixels < 0 || C <= 0 || C > 1024) return DCFP_E_BADDESC;
    if (n_pixels == 0) return DCFP_OK;     // an empty tensor has no storage: its pointers are null
    if (!pred || !gt) return DCFP_E_BADDESC;
    long long b = (n_pixels + kThreads - 1) / kThreads;
    if (b > 1024) b = 1024;
    if (C <= 64)
        hipLaunchKernelGGL(confusion_kernel, dim3((unsigned)b), dim3(kThreads), (size_t)C * C * sizeof(unsigned),
                           dcfp_s(stream), pred, reinterpret_cast<const long long*>(gt), ignore_index,
                           (long long)n_pixels, C, reinterpret_cast<unsigned long long*>(conf));
    else   // ADE (150) / COCO-Stuff (171): the histogram does not fit LDS, count in global memory
        hipLaunchKernelGGL(confusion_global_kernel, dim3((unsigned)b), dim3(kThreads), 0, dcfp_s(stream), pred,
                           reinterpret_cast<const long long*>(gt), ignore_index, (long long)n_pixels, C,
                           reinterpret_cast<unsigned long long*>(conf));
    DCFP_RETURN_LAUNCH();
}
