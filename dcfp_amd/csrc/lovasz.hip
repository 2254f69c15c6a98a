// lovasz.hip — Lovasz-Softmax loss (Berman, Triki, Blaschko, CVPR 2018; classes = 'present') of the bilinearly
// upsampled low-resolution logits, without a sort and without the N x C x H x W probabilities.
//
// Per valid pixel (label in [0, C), not ignore_index) and class c:  z = bilinear upsample of the logits (bilinear.h,
// logit_of() of upsample_logits.h),  p = exp(z - lse),  e = (label == c) ? 1 - p : p,
//     q = min(2^20, floor(e * 2^20 + 0.5)),      b = min(B - 1, q >> (20 - log2 B)),       B = bins.
// Per class and bin four integers: nF / nB count the foreground (label == c) / background pixels of the bin, SF / SB
// add their q.  With G = sum_b nF[b] (> 0: the class is present) and F_above / G_above the foreground / background
// counts of all higher bins,
//     I0 = G - F_above,  U0 = G + G_above,  I1 = I0 - nF[b],  U1 = U0 + nB[b],
//     wF[b] = (1/U0 + 1/U1) / 2,     wB[b] = (I0 + I1) / (2 U0 U1)
// - the mean of the exact Lovasz gradients of the two sort orders of a tied bin (foreground first, background first) -
//     loss_c = 2^-20 * sum_b (wF[b] SF[b] + wB[b] SB[b]),        loss = mean of loss_c over the present classes.
// The weights are locally constant in the logits:  dloss/dz_k = p_k (a_k - sum_c a_c p_c),  a_c = -wF[b]/P for the
// label's class, +wB[b]/P for any other present class, 0 for an absent one; then the bilinear adjoint.
//
// Kernels.  lovasz_term() below is the only place that computes z, p, q and b; every kernel calls it, and fp contraction
// is off in this file, so forward and backward put every (pixel, class) into the same bin bit for bit.
//   histogram  a workgroup owns a tile of pixels: writes their log-sum-exp, then loops over chunks of classes whose
//              accumulators fit its 64 KiB of LDS (4096 / B classes): zero, one 64-bit LDS add per (pixel, class)
//              (count in the high word, the sum of q - (b << shift) in the low word: at most 2^14 per pixel and 2^16
//              pixels per tile), then one integer atomic per non-empty accumulator into the global table.  Integer
//              adds only: the table does not depend on the order of arrival.
//   scan       one workgroup per class: suffix sums over the bins, the weights and loss_c in fp64 in a fixed order;
//              a last kernel counts the present classes P, writes the loss and the fp32 table [C][B][2] = (wF, wB) / P.
//   backward   one pass writes A = sum_c a_c p_c per pixel; the gather organised by cells that the CE backward
//              uses (cell_gather.h) adds wy wx p_c (a_c - A) over the destination pixels of every
//              low-resolution element, each pixel evaluated once per window of 20 classes.  No atomics.
//   errors     q of every (n, c, Y, X) as uint32, 0xFFFFFFFF at invalid pixels: for tests and for looking at the
//              error distribution, never part of a training step.
#include <math.h>

#include "bilinear.h"
#include "common.h"

// From here on every expression compiles without FMAs, those of the two headers below included: contraction is fixed
// where an expression is parsed, not where a template is instantiated.  bilinear.h stays above the pragma - lerp_of and
// dst_range are the coordinate rules of every file and keep the contraction they have everywhere else - while the
// per-pixel helpers (logit_of, lse_at) and the cell gather's accumulates must be this file's: uncontracted, like
// lovasz_term(), so that the histogram and the backward see the same z, p, q and b.
#pragma clang fp contract(off)

#include "cell_gather.h"
#include "upsample_logits.h"

namespace {

using namespace dcfp_bilinear;   // Lerp, lerp_of, host_scale, with_align; Tap, tap_of, logit_of, lse_at, Pix, pix_of
using namespace dcfp_cells;      // kCellTH, kCellTW, kCellThreads, kCellCount, cell_block, cell_gather

constexpr int kQ = 20;                       // q = e * 2^20, rounded
constexpr int kThreads = 256;
constexpr int kHistThreads = 512;
constexpr int kHistSlots = 4096;             // (class, bin) pairs of a chunk: 4096 x 2 x 8 B = 64 KiB of LDS
constexpr long long kTileMin = 2048, kTileMax = 65536;      // pixels per histogram workgroup (low word: 2^16 * 2^14)
constexpr int kMaxBlocks = 1 << 16;

struct Term {
    float z, p;
    unsigned q;
    int b;
};

// (pixel, class) -> z, p, q, b from the class's four stencil values; shift = 20 - log2 B
__device__ __forceinline__ Term lovasz_term(float v00, float v01, float v10, float v11, float h0, float h1, float w0,
                                            float w1, float lse, bool fg, int shift, int last_bin) {
    Term r;
    r.z = logit_of(v00, v01, v10, v11, h0, h1, w0, w1);
    r.p = expf(r.z - lse);
    const float e = fg ? 1.0f - r.p : r.p;
    const float s = floorf(e * (float)(1 << kQ) + 0.5f);          // exact: a power-of-two scale, then |x| < 2^23
    r.q = s <= 0.0f ? 0u : (s >= (float)(1 << kQ) ? (1u << kQ) : (unsigned)s);
    const int b = (int)(r.q >> shift);
    r.b = b > last_bin ? last_bin : b;
    return r;
}

// the same from the class's low-resolution plane
__device__ __forceinline__ Term lovasz_term(const float* __restrict__ plane, const Tap& t, float lse, bool fg,
                                            int shift, int last_bin) {
    return lovasz_term(plane[t.o00], plane[t.o01], plane[t.o10], plane[t.o11], t.h0, t.h1, t.w0, t.w1, lse, fg, shift,
                       last_bin);
}

__device__ __forceinline__ bool label_valid(long long label, int C, int ignore_index) {
    return label >= 0 && label < C && label != ignore_index;
}

// ------------------------------------------------------------------------------------------------ histogram
template <bool ALIGN>
__global__ void __launch_bounds__(kHistThreads)
lovasz_hist_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, int ignore_index, int N, int C,
                   int h, int w, int H, int W, float sh, float sw, int log2B, int chunk, long long tile,
                   float* lse_out, unsigned long long* __restrict__ SF, unsigned long long* __restrict__ SB,
                   unsigned int* __restrict__ nF, unsigned int* __restrict__ nB) {
    __shared__ unsigned long long acc[kHistSlots][2];       // [class of the chunk * B + bin][foreground, background]
    const int B = 1 << log2B, shift = kQ - log2B;
    const long long total = (long long)N * H * W, plane = (long long)h * w;
    const long long start = (long long)blockIdx.x * tile;
    const long long end = start + tile < total ? start + tile : total;
    const int tid = threadIdx.x;

    for (long long pix = start + tid; pix < end; pix += kHistThreads) {
        const Pix P = pix_of(pix, H, W);
        const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
        lse_out[pix] = lse_at(logits + (long long)P.n * C * plane, plane, C, t);
    }
    for (int c0 = 0; c0 < C; c0 += chunk) {
        const int nc = C - c0 < chunk ? C - c0 : chunk;
        for (int i = tid; i < nc * B; i += kHistThreads) acc[i][0] = acc[i][1] = 0ull;
        __syncthreads();
        for (long long pix = start + tid; pix < end; pix += kHistThreads) {       // the pixels this thread wrote lse for
            const long long label = labels[pix];
            if (!label_valid(label, C, ignore_index)) continue;
            const Pix P = pix_of(pix, H, W);
            const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
            const float lse = lse_out[pix];
            const float* base = logits + ((long long)P.n * C + c0) * plane;
            for (int k = 0; k < nc; ++k) {
                const bool fg = label == c0 + k;
                const Term r = lovasz_term(base + k * plane, t, lse, fg, shift, B - 1);
                const unsigned low = r.q - ((unsigned)r.b << shift);              // <= 2^shift <= 2^14
                atomicAdd(&acc[k * B + r.b][fg ? 0 : 1], (1ull << 32) | low);
            }
        }
        __syncthreads();
        for (int i = tid; i < nc * B; i += kHistThreads) {
            const unsigned long long base_q = (unsigned long long)(i & (B - 1)) << shift;
            const long long g = (long long)c0 * B + i;
            const unsigned long long f = acc[i][0], bk = acc[i][1];
            if (f) {
                atomicAdd(&nF[g], (unsigned)(f >> 32));
                atomicAdd(&SF[g], (f & 0xffffffffull) + (f >> 32) * base_q);
            }
            if (bk) {
                atomicAdd(&nB[g], (unsigned)(bk >> 32));
                atomicAdd(&SB[g], (bk & 0xffffffffull) + (bk >> 32) * base_q);
            }
        }
        __syncthreads();
    }
}

// ------------------------------------------------------------------------------------------------ scan
// One workgroup per class.  Thread t owns the B / nthr bins from t * per; wraw[c][b] = (wF, wB) in fp64.
__global__ void __launch_bounds__(kThreads)
lovasz_scan_kernel(const unsigned int* __restrict__ nF, const unsigned int* __restrict__ nB,
                   const unsigned long long* __restrict__ SF, const unsigned long long* __restrict__ SB, int log2B,
                   double* __restrict__ wraw, double* __restrict__ loss_c, long long* __restrict__ fg_count) {
    __shared__ long long tF[kThreads], tB[kThreads];
    __shared__ double part[kThreads];
    const int B = 1 << log2B, c = blockIdx.x, t = threadIdx.x;
    const int per = B > kThreads ? B / kThreads : 1, nthr = B / per;
    const long long row = (long long)c * B;
    long long f = 0, g = 0;
    if (t < nthr)
        for (int b = t * per; b < (t + 1) * per; ++b) {
            f += nF[row + b];
            g += nB[row + b];
        }
    tF[t] = f; tB[t] = g;
    __syncthreads();
    long long G = 0, Fa = 0, Ga = 0;            // G: the class's foreground pixels; Fa / Ga: counts of the bins above mine
    for (int u = 0; u < nthr; ++u) {
        G += tF[u];
        if (u > t) { Fa += tF[u]; Ga += tB[u]; }
    }
    double acc = 0.0;
    if (t < nthr) {
        for (int b = (t + 1) * per - 1; b >= t * per; --b) {
            double wf = 0.0, wb = 0.0;
            const long long cf = nF[row + b], cb = nB[row + b];
            if (G > 0) {
                const long long I0 = G - Fa, U0 = G + Ga, I1 = I0 - cf, U1 = U0 + cb;
                wf = (1.0 / (double)U0 + 1.0 / (double)U1) / 2.0;
                wb = (double)(I0 + I1) / (2.0 * (double)U0 * (double)U1);
                acc += wf * (double)SF[row + b] + wb * (double)SB[row + b];
            }
            wraw[(row + b) * 2 + 0] = wf;
            wraw[(row + b) * 2 + 1] = wb;
            Fa += cf; Ga += cb;
        }
    }
    part[t] = acc;
    __syncthreads();
    if (t == 0) {
        double s = 0.0;
        for (int u = nthr - 1; u >= 0; --u) s += part[u];        // from the highest bins down, always in this order
        loss_c[c] = s * (1.0 / (double)(1 << kQ));
        fg_count[c] = G;
    }
}

// P = present classes; loss = sum_c loss_c / P (block 0); table = (float)(wraw / P), zeros where P == 0
__global__ void __launch_bounds__(kThreads)
lovasz_final_kernel(const double* __restrict__ wraw, const double* __restrict__ loss_c,
                    const long long* __restrict__ fg_count, int C, long long n_table, float* __restrict__ table,
                    float* __restrict__ loss_out) {
    __shared__ int present;
    if (threadIdx.x == 0) {
        int P = 0;
        for (int c = 0; c < C; ++c) P += fg_count[c] > 0 ? 1 : 0;
        present = P;
        if (blockIdx.x == 0) {
            double s = 0.0;
            for (int c = 0; c < C; ++c)
                if (fg_count[c] > 0) s += loss_c[c];
            loss_out[0] = P > 0 ? (float)(s / (double)P) : 0.0f;
        }
    }
    __syncthreads();
    const int P = present;
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < n_table; i += (long long)gridDim.x * kThreads)
        table[i] = P > 0 ? (float)(wraw[i] / (double)P) : 0.0f;
}

// ------------------------------------------------------------------------------------------------ backward
// a_c of a (pixel, class): -wF[b] for the label's class, +wB[b] otherwise (the table is divided by P, 0 when absent)
__device__ __forceinline__ float coeff_of(const float* __restrict__ table, int c, int B, const Term& r, bool fg) {
    const float v = table[((long long)c * B + r.b) * 2 + (fg ? 0 : 1)];
    return fg ? -v : v;
}

template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
lovasz_asum_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, int ignore_index, int N, int C,
                   int h, int w, int H, int W, float sh, float sw, int log2B, const float* __restrict__ lse,
                   const float* __restrict__ table, float* __restrict__ asum) {
    const int B = 1 << log2B, shift = kQ - log2B;
    const long long total = (long long)N * H * W, plane = (long long)h * w;
    for (long long pix = (long long)blockIdx.x * kThreads + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * kThreads) {
        const long long label = labels[pix];
        float A = 0.f;
        if (label_valid(label, C, ignore_index)) {
            const Pix P = pix_of(pix, H, W);
            const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
            const float* base = logits + (long long)P.n * C * plane;
            const float ls = lse[pix];
            for (int c = 0; c < C; ++c) {
                const bool fg = label == c;
                const Term r = lovasz_term(base + c * plane, t, ls, fg, shift, B - 1);
                A += coeff_of(table, c, B, r, fg) * r.p;
            }
        }
        asum[pix] = A;
    }
}

// The gather is cell_gather.h's, in windows of kCellCT classes; what a destination pixel contributes per class is here.
constexpr int kCellCT = 20;            // classes per window: 19 in one, 4 x 20 accumulators and corners per lane

struct LovaszCellLoss {
    const long long* __restrict__ lab;      // of the image
    const float* __restrict__ ls;
    const float* __restrict__ as;
    const float* __restrict__ table;        // of class c0
    int ignore_index, C, c0, shift, B;

    struct Pixel {
        float pw, lq, Aq;
        long long lrel;                     // the label's position in this window, if it is in it
    };

    __device__ __forceinline__ bool pixel(long long q, Pixel& px) const {
        const long long label = lab[q];
        if (!label_valid(label, C, ignore_index)) return false;
        px.pw = 1.f;
        px.lq = ls[q];
        px.Aq = as[q];
        px.lrel = label - c0;
        return true;
    }

    __device__ __forceinline__ float grad(const Pixel& px, int c, float v00, float v01, float v10, float v11,
                                          const Lerp& Lh, const Lerp& Lw) const {
        const bool fg = px.lrel == c;
        const Term r = lovasz_term(v00, v01, v10, v11, Lh.l0, Lh.l1, Lw.l0, Lw.l1, px.lq, fg, shift, B - 1);
        return r.p * (coeff_of(table, c, B, r, fg) - px.Aq);
    }
};

template <bool ALIGN, int CT>
__global__ void __launch_bounds__(kCellThreads, 2)
lovasz_bwd_cells_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, int ignore_index, int C,
                        int h, int w, int H, int W, float sh, float sw, int log2B, const float* __restrict__ lse,
                        const float* __restrict__ table, const float* __restrict__ asum,
                        const float* __restrict__ grad_scale, float* __restrict__ dlogits, int tiles_w, int tiles_h,
                        int chunks) {
    __shared__ float corner[kCellCount][4][CT + 1];
    const int B = 1 << log2B;
    const CellBlock blk = cell_block<CT, false>(C, tiles_w, tiles_h, chunks);
    const long long img = (long long)blk.n * H * W;
    const long long first = ((long long)blk.n * C + blk.c0) * h * w;      // (n, c0) of logits and dlogits
    const LovaszCellLoss loss{labels + img, lse + img, asum + img, table + (long long)blk.c0 * B * 2,
                              ignore_index,  C,         blk.c0,     kQ - log2B,
                              B};
    cell_gather<ALIGN, CT, false>(corner, logits + first, loss, blk, h, w, H, W, sh, sw, grad_scale[0], dlogits + first);
}

// ------------------------------------------------------------------------------------------------ error dump
template <bool ALIGN>
__global__ void __launch_bounds__(kThreads)
lovasz_errors_kernel(const float* __restrict__ logits, const long long* __restrict__ labels, int ignore_index, int N,
                     int C, int h, int w, int H, int W, float sh, float sw, unsigned int* __restrict__ out) {
    const long long total = (long long)N * H * W, plane = (long long)h * w, HW = (long long)H * W;
    for (long long pix = (long long)blockIdx.x * kThreads + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * kThreads) {
        const long long label = labels[pix];
        const Pix P = pix_of(pix, H, W);
        unsigned int* o = out + (long long)P.n * C * HW + (pix - (long long)P.n * HW);
        if (!label_valid(label, C, ignore_index)) {
            for (int c = 0; c < C; ++c) o[c * HW] = 0xFFFFFFFFu;
            continue;
        }
        const Tap t = tap_of(lerp_of<ALIGN>(P.Y, sh, h), lerp_of<ALIGN>(P.X, sw, w), w);
        const float* base = logits + (long long)P.n * C * plane;
        const float ls = lse_at(base, plane, C, t);
        for (int c = 0; c < C; ++c) o[c * HW] = lovasz_term(base + c * plane, t, ls, label == c, 0, 1 << kQ).q;
    }
}

// ------------------------------------------------------------------------------------------------ host side
int log2_bins(int bins) {        // log2 B for a power of two in [64, 4096], else -1
    for (int k = 6; k <= 12; ++k)
        if (bins == (1 << k)) return k;
    return -1;
}

// workspace: SF, SB (uint64 [C*B] each), nF, nB (uint32 [C*B] each), wraw (fp64 [C*B*2]), loss_c (fp64 [C]),
// fg_count (int64 [C]); every part starts 8-byte aligned
struct Workspace {
    unsigned long long *SF, *SB;
    unsigned int *nF, *nB;
    double *wraw, *loss_c;
    long long* fg_count;
    size_t bytes, hist_bytes;
};

Workspace carve(void* ws, int C, int bins) {
    const size_t cb = (size_t)C * bins;
    char* p = static_cast<char*>(ws);
    Workspace r;
    r.SF = reinterpret_cast<unsigned long long*>(p);
    r.SB = r.SF + cb;
    r.nF = reinterpret_cast<unsigned int*>(r.SB + cb);
    r.nB = r.nF + cb;
    r.hist_bytes = cb * 24;
    r.wraw = reinterpret_cast<double*>(p + r.hist_bytes);
    r.loss_c = r.wraw + cb * 2;
    r.fg_count = reinterpret_cast<long long*>(r.loss_c + C);
    r.bytes = r.hist_bytes + cb * 16 + (size_t)C * 16;
    return r;
}

int check_shape(int N, int C, int h, int w, int H, int W) {
    if (N < 1 || C < 1 || h < 1 || w < 1 || H < 1 || W < 1) return DCFP_E_BADDESC;
    if (C > 255 || (long long)N * H * W >= (1LL << 31)) return DCFP_E_UNSUPPORTED;
    return DCFP_OK;
}

unsigned grid_for(long long items) {
    const long long blocks = (items + kThreads - 1) / kThreads;
    return (unsigned)(blocks < 1 ? 1 : (blocks > kMaxBlocks ? kMaxBlocks : blocks));
}

}  // namespace

extern "C" size_t dcfp_lovasz_workspace_bytes(int C, int bins) {
    if (C < 1 || C > 255 || log2_bins(bins) < 0) return 0;
    return carve(nullptr, C, bins).bytes;
}

extern "C" int dcfp_lovasz_hist_f32(const float* logits, const int64_t* labels, int ignore_index, int N, int C, int h,
                                    int w, int H, int W, int align_corners, int bins, float* lse, void* workspace,
                                    size_t workspace_bytes, dcfp_stream_t stream) {
    const int log2B = log2_bins(bins);
    if (!logits || !labels || !lse || log2B < 0) return DCFP_E_BADDESC;
    if (const int e = check_shape(N, C, h, w, H, W)) return e;
    if (!workspace || workspace_bytes < dcfp_lovasz_workspace_bytes(C, bins)) return DCFP_E_WORKSPACE;
    const Workspace ws = carve(workspace, C, bins);
    hipStream_t st = dcfp_s(stream);
    if (hipMemsetAsync(workspace, 0, ws.hist_bytes, st) != hipSuccess) DCFP_RETURN_LAUNCH();
    const long long total = (long long)N * H * W;
    const long long want = 4LL * dcfp_num_cus();
    long long tile = (total + want - 1) / want;
    tile = (tile + kHistThreads - 1) / kHistThreads * kHistThreads;
    tile = tile < kTileMin ? kTileMin : (tile > kTileMax ? kTileMax : tile);
    const unsigned blocks = (unsigned)((total + tile - 1) / tile);
    const int chunk = kHistSlots / bins;                   // classes whose accumulators share the LDS: 64 ... 1
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(lovasz_hist_kernel<A.value>, dim3(blocks), dim3(kHistThreads), 0, st, logits, lab,
                           ignore_index, N, C, h, w, H, W, sh, sw, log2B, chunk, tile, lse, ws.SF, ws.SB, ws.nF, ws.nB);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_lovasz_scan_f32(int C, int bins, void* workspace, size_t workspace_bytes, float* loss_out,
                                    float* weights, dcfp_stream_t stream) {
    const int log2B = log2_bins(bins);
    if (!loss_out || !weights || C < 1 || log2B < 0) return DCFP_E_BADDESC;
    if (C > 255) return DCFP_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < dcfp_lovasz_workspace_bytes(C, bins)) return DCFP_E_WORKSPACE;
    const Workspace ws = carve(workspace, C, bins);
    hipStream_t st = dcfp_s(stream);
    hipLaunchKernelGGL(lovasz_scan_kernel, dim3(C), dim3(kThreads), 0, st, ws.nF, ws.nB, ws.SF, ws.SB, log2B, ws.wraw,
                       ws.loss_c, ws.fg_count);
    const long long n_table = (long long)C * bins * 2;
    hipLaunchKernelGGL(lovasz_final_kernel, dim3(grid_for((n_table + 3) / 4)), dim3(kThreads), 0, st, ws.wraw, ws.loss_c,
                       ws.fg_count, C, n_table, weights, loss_out);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_lovasz_bwd_f32(const float* logits, const int64_t* labels, int ignore_index, int N, int C, int h,
                                   int w, int H, int W, int align_corners, int bins, const float* lse,
                                   const float* weights, const float* grad_scale, float* asum, float* dlogits,
                                   dcfp_stream_t stream) {
    const int log2B = log2_bins(bins);
    if (!logits || !labels || !lse || !weights || !grad_scale || !asum || !dlogits || log2B < 0) return DCFP_E_BADDESC;
    if (const int e = check_shape(N, C, h, w, H, W)) return e;
    const int tiles_h = cell_tiles_h(h), tiles_w = cell_tiles_w(w), chunks = (C + kCellCT - 1) / kCellCT;
    const long long cell_blocks = (long long)N * tiles_h * tiles_w * chunks;
    if (cell_blocks > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    hipStream_t st = dcfp_s(stream);
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(lovasz_asum_kernel<A.value>, dim3(grid_for((long long)N * H * W)), dim3(kThreads), 0, st,
                           logits, lab, ignore_index, N, C, h, w, H, W, sh, sw, log2B, lse, weights, asum);
        hipLaunchKernelGGL((lovasz_bwd_cells_kernel<A.value, kCellCT>), dim3((unsigned)cell_blocks), dim3(kCellThreads),
                           0, st, logits, lab, ignore_index, C, h, w, H, W, sh, sw, log2B, lse, weights, asum,
                           grad_scale, dlogits, tiles_w, tiles_h, chunks);
    });
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_lovasz_errors_u32(const float* logits, const int64_t* labels, int ignore_index, int N, int C, int h,
                                      int w, int H, int W, int align_corners, uint32_t* errors, dcfp_stream_t stream) {
    if (!logits || !labels || !errors) return DCFP_E_BADDESC;
    if (const int e = check_shape(N, C, h, w, H, W)) return e;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
    const long long* lab = reinterpret_cast<const long long*>(labels);
    with_align(align_corners, [&](auto A) {
        hipLaunchKernelGGL(lovasz_errors_kernel<A.value>, dim3(grid_for((long long)N * H * W)), dim3(kThreads), 0,
                           dcfp_s(stream), logits, lab, ignore_index, N, C, h, w, H, W, sh, sw, errors);
    });
    DCFP_RETURN_LAUNCH();
}
