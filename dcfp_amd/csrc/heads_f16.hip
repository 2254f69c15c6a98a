// heads_f16.hip — the two NHWC fp16 nodes that the DeepLabv3+ decoder and the PSPNet pyramid add to the frozen fp16
// engine (dcfp_amd/deploy.py).  Conventions of conv_f16.hip: activations NHWC fp16 with channel pitches
// that are multiples of 8, a lane owns one 16-byte chunk (8 channels) per access, fp32 arithmetic with one rounding to
// fp16 at the store, vector stores only, no atomics (two runs give the same bits), every launcher validates on the
// host before any HIP call.
//
// Bilinear resize (resize_bilinear_kernel): F.interpolate(mode='bilinear') with the index math of bilinear.h (its
//   products rounded one by one, see lerp_rounded) and the fused-multiply-add order of resize.hip (top = fma(l1x, b, l0x * a), bot likewise, out = fma(l0y, top, l1y * bot)):
//   one lane per (output pixel, chunk), chunk fastest, so a wave stores 1 KiB of consecutive channels.  The four source
//   chunks come from a map that is small next to the destination and stays in cache; the kernel is store-bound.  A 1x1
//   source gives l0 = 1, l1 = 0 on both axes: the value itself, bit for bit what dcfp_broadcast_nhwc_f16 writes.
//
// Pyramid pool (pyramid_partial_kernel + pyramid_final_kernel): all levels of nn.AdaptiveAvgPool2d(s) in ONE sweep over
//   the features.  PyTorch's windows (rows floor(i*H/s) .. ceil((i+1)*H/s) - 1) overlap where s does not divide H, so
//   the map is cut into "atoms", the cells between all the levels' window boundaries (ppm.hip does the same in fp32);
//   long gaps are cut further so that large maps spread over the CUs.  Pass 1: one block per (atom, group of 16 chunks,
//   image) sums the atom's pixels in fp32 - 16 pixel lanes stride the atom row-major, then lane 0 .. 15 are added in
//   that order - and writes the sum to the caller's workspace [N][atom][C8] (no exchange between blocks in a launch).
//   Pass 2: one lane per (image, bin, chunk) adds the atoms of its window (row atom ascending, then column atom
//   ascending), multiplies by 1 / area and rounds once.
#include "common.h"
#include "bilinear.h"

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

namespace {

using namespace dcfp_bilinear;

constexpr int kMaxLevels = 4;
constexpr int kMaxS = 8;
constexpr int kBaseCuts = 2 * kMaxLevels * kMaxS;   // window boundaries of all levels along one axis, before unique
constexpr int kSplit = 32;                          // an atom spans at most max(kSplit, len / kSplit) rows / columns
constexpr int kMaxCuts = kBaseCuts + kSplit + 2;
constexpr int kChunks = 16, kPixLanes = 16;         // pass 1 block: 16 chunks x 16 pixel lanes

bool mult8(int v) { return v > 0 && (v & 7) == 0; }

// ------------------------------------------------------------------------------------------------ bilinear resize
// lerp_of of bilinear.h with every product rounded before it is used, which is ATen's arithmetic.  hipcc contracts by
// default, and fma(scale, dst, -i0) keeps the unrounded product: where the two grids coincide but the scale is inexact
// (5 -> 13 rows under align_corners, scale 4/12) l1 then comes out as 2^-24 instead of 0 and leaks 2^-24 |neighbour|
// into a pixel that F.interpolate copies exactly - more than the rounding of a pixel that is itself near zero.
template <bool ALIGN>
__device__ __forceinline__ Lerp lerp_rounded(int dst, float scale, int in_size) {
#pragma clang fp contract(off)
    float src;
    if (ALIGN) {
        src = scale * (float)dst;
    } else {
        src = scale * ((float)dst + 0.5f) - 0.5f;
        src = src < 0.f ? 0.f : src;
    }
    Lerp r;
    int i0 = (int)src;
    if (i0 > in_size - 1) i0 = in_size - 1;
    r.i0 = i0;
    r.i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
    float l1 = src - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    r.l1 = l1;
    r.l0 = 1.f - l1;
    return r;
}

template <bool ALIGN>
__global__ __launch_bounds__(256) void resize_bilinear_kernel(const h8_t* __restrict__ x, h8_t* __restrict__ y,
                                                              long total, int h, int w, int c8n, int xp8, int H, int W,
                                                              int yp8, int yo8, float scale_h, float scale_w) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c8n);
    long pix = idx / c8n;                              // (n * H + Y) * W + X
    const int X = (int)(pix % W);
    const long nY = pix / W;
    const int Y = (int)(nY % H);
    const long n = nY / H;
    const Lerp Lh = lerp_rounded<ALIGN>(Y, scale_h, h), Lw = lerp_rounded<ALIGN>(X, scale_w, w);
    const h8_t* p = x + n * h * w * xp8 + ch;
    const h8_t a = p[((long)Lh.i0 * w + Lw.i0) * xp8], b = p[((long)Lh.i0 * w + Lw.i1) * xp8];
    const h8_t c = p[((long)Lh.i1 * w + Lw.i0) * xp8], d = p[((long)Lh.i1 * w + Lw.i1) * xp8];
    h8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const float top = __builtin_fmaf(Lw.l1, (float)b[e], Lw.l0 * (float)a[e]);
        const float bot = __builtin_fmaf(Lw.l1, (float)d[e], Lw.l0 * (float)c[e]);
        o[e] = (_Float16)__builtin_fmaf(Lh.l0, top, Lh.l1 * bot);
    }
    y[pix * yp8 + yo8 + ch] = o;
}

// --------------------------------------------------------------------------------------------------- pyramid pool
struct PyrGeom {
    int nlev;
    int s[kMaxLevels];
    int nra, nca;                                       // row / column atoms
    short rcut[kMaxCuts], ccut[kMaxCuts];               // atom a: rows [rcut[a], rcut[a + 1])
    unsigned char ra[kMaxLevels][kMaxS][2], ca[kMaxLevels][kMaxS][2];   // atoms [lo, hi) of bin row i / column j
};

struct PyrOut {
    _Float16* y[kMaxLevels];
    int pitch[kMaxLevels];
};

__global__ __launch_bounds__(256) void pyramid_partial_kernel(const h8_t* __restrict__ x, float* __restrict__ part,
                                                              int H, int W, int c8n, int xp8, int xo8, const PyrGeom G) {
    __shared__ float red[kPixLanes][kChunks][8];
    const int cl = threadIdx.x & (kChunks - 1), pl = threadIdx.x / kChunks;
    const int atom = blockIdx.x, ar = atom / G.nca, ac = atom - ar * G.nca;
    const int ch = blockIdx.y * kChunks + cl;
    const long n = blockIdx.z;
    const int y0 = G.rcut[ar], x0 = G.ccut[ac], aw = G.ccut[ac + 1] - x0;
    const int npix = (G.rcut[ar + 1] - y0) * aw;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ch < c8n)
        for (int q = pl; q < npix; q += kPixLanes) {
            const int r = q / aw, c = q - r * aw;
            const h8_t v = x[((n * H + y0 + r) * W + x0 + c) * xp8 + xo8 + ch];
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pl][cl][e] = a[e];
    __syncthreads();
    if (threadIdx.x < kChunks * 2) {                    // lane (chunk, half): four of the chunk's eight channels
        const int c2 = threadIdx.x >> 1, hf = threadIdx.x & 1, cc = blockIdx.y * kChunks + c2;
        if (cc < c8n) {
            float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
            for (int q = 0; q < kPixLanes; ++q) {
                t.x += red[q][c2][4 * hf]; t.y += red[q][c2][4 * hf + 1];
                t.z += red[q][c2][4 * hf + 2]; t.w += red[q][c2][4 * hf + 3];
            }
            const long natoms = (long)G.nra * G.nca;
            *reinterpret_cast<float4*>(part + ((n * natoms + atom) * c8n + cc) * 8 + 4 * hf) = t;
        }
    }
}

__global__ __launch_bounds__(256) void pyramid_final_kernel(const float* __restrict__ part, const PyrOut out, int c8n,
                                                            int nbins, long total, const PyrGeom G) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c8n);
    const long nb = idx / c8n;
    int b = (int)(nb % nbins);
    const long n = nb / nbins;
    int l = 0;
    while (b >= G.s[l] * G.s[l]) { b -= G.s[l] * G.s[l]; ++l; }
    const int s = G.s[l], i = b / s, j = b - i * s;
    const int r0 = G.ra[l][i][0], r1 = G.ra[l][i][1], c0 = G.ca[l][j][0], c1 = G.ca[l][j][1];
    const long natoms = (long)G.nra * G.nca;
    const float* p = part + (n * natoms * c8n + ch) * 8;
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int ar = r0; ar < r1; ++ar)
        for (int ac = c0; ac < c1; ++ac) {
            const float4* v = reinterpret_cast<const float4*>(p + (long)(ar * G.nca + ac) * c8n * 8);
            const float4 lo = v[0], hi = v[1];
            acc[0] += lo.x; acc[1] += lo.y; acc[2] += lo.z; acc[3] += lo.w;
            acc[4] += hi.x; acc[5] += hi.y; acc[6] += hi.z; acc[7] += hi.w;
        }
    const float area = (float)((G.rcut[r1] - G.rcut[r0]) * (G.ccut[c1] - G.ccut[c0]));
    h8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) o[e] = (_Float16)(acc[e] / area);
    *reinterpret_cast<h8_t*>(out.y[l] + ((n * s + i) * s + j) * out.pitch[l] + ch * 8) = o;
}

// PyTorch's adaptive-pool windows of every level along one axis as atoms, gaps longer than max(kSplit, len / kSplit) cut
void axis_atoms(int len, int nlev, const int* s, short* cut, int& natoms, unsigned char (*bins)[kMaxS][2]) {
    int pts[kMaxCuts];
    int np = 0;
    for (int l = 0; l < nlev; ++l)
        for (int i = 0; i < s[l]; ++i) {
            pts[np++] = (int)(((long long)i * len) / s[l]);
            pts[np++] = (int)(((long long)(i + 1) * len + s[l] - 1) / s[l]);
        }
    const int step = len / kSplit > kSplit ? (len + kSplit - 1) / kSplit : kSplit;
    for (int v = step; v < len; v += step) pts[np++] = v;       // at most kSplit - 1 of them
    for (int a = 1; a < np; ++a)                                // insertion sort, then unique
        for (int b = a; b > 0 && pts[b - 1] > pts[b]; --b) { const int t = pts[b]; pts[b] = pts[b - 1]; pts[b - 1] = t; }
    int ncut = 0;
    for (int a = 0; a < np; ++a)
        if (ncut == 0 || cut[ncut - 1] != pts[a]) cut[ncut++] = (short)pts[a];
    for (int l = 0; l < nlev; ++l)
        for (int i = 0; i < s[l]; ++i) {
            const int st = (int)(((long long)i * len) / s[l]), en = (int)(((long long)(i + 1) * len + s[l] - 1) / s[l]);
            for (int a = 0; a < ncut; ++a) {
                if (cut[a] == st) bins[l][i][0] = (unsigned char)a;
                if (cut[a] == en) bins[l][i][1] = (unsigned char)a;
            }
        }
    natoms = ncut - 1;
}

int pyr_geom(int N, int H, int W, int C8, int nlev, const int* sizes, PyrGeom& G) {
    if (N <= 0 || H <= 0 || W <= 0 || !mult8(C8) || !sizes) return DCFP_E_BADDESC;
    if (nlev < 1) return DCFP_E_BADDESC;
    if (nlev > kMaxLevels || N > 65535 || H > 32767 || W > 32767 || C8 / 8 > 65535 * kChunks) return DCFP_E_UNSUPPORTED;
    for (int l = 0; l < nlev; ++l) {
        if (sizes[l] <= 0) return DCFP_E_BADDESC;
        if (sizes[l] > kMaxS) return DCFP_E_UNSUPPORTED;
    }
    G = PyrGeom{};
    G.nlev = nlev;
    for (int l = 0; l < nlev; ++l) G.s[l] = sizes[l];
    axis_atoms(H, nlev, G.s, G.rcut, G.nra, G.ra);
    axis_atoms(W, nlev, G.s, G.ccut, G.nca, G.ca);
    return DCFP_OK;
}

unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" {

int dcfp_resize_bilinear_nhwc_f16(const void* x, int N, int h, int w, int C8, int x_pitch, void* y, int H, int W,
                                  int y_pitch, int y_off, int align_corners, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || h <= 0 || w <= 0 || H <= 0 || W <= 0 || !mult8(C8) || !mult8(x_pitch) || !mult8(y_pitch) ||
        x_pitch < C8 || y_off < 0 || (y_off & 7) || y_off + C8 > y_pitch || !dcfp_aligned16(x) || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    if (h > 32768 || w > 32768 || H > 32768 || W > 32768) return DCFP_E_UNSUPPORTED;
    const long total = (long)N * H * W * (C8 / 8);
    if (total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    const float sh = host_scale(h, H, align_corners), sw = host_scale(w, W, align_corners);
#define DCFP_RESIZE_F16(A)                                                                                         \
    hipLaunchKernelGGL(resize_bilinear_kernel<A>, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream),            \
                       reinterpret_cast<const h8_t*>(x), reinterpret_cast<h8_t*>(y), total, h, w, C8 / 8, x_pitch / 8, \
                       H, W, y_pitch / 8, y_off / 8, sh, sw)
    if (align_corners) DCFP_RESIZE_F16(true); else DCFP_RESIZE_F16(false);
#undef DCFP_RESIZE_F16
    DCFP_RETURN_LAUNCH();
}

size_t dcfp_pyramid_pool_nhwc_f16_workspace_bytes(int N, int H, int W, int C8, int nlev, const int* sizes) {
    PyrGeom G;
    if (pyr_geom(N, H, W, C8, nlev, sizes, G) != DCFP_OK) return 0;
    return (size_t)N * G.nra * G.nca * C8 * sizeof(float);
}

int dcfp_pyramid_pool_nhwc_f16(const void* x, int N, int H, int W, int C8, int x_pitch, int x_off, int nlev,
                               const int* sizes, void* const* y, const int* y_pitch, void* workspace,
                               size_t workspace_bytes, dcfp_stream_t stream) {
    if (!x || !y || !y_pitch || !dcfp_aligned16(x) || !mult8(x_pitch) || x_off < 0 || (x_off & 7) ||
        (long)x_off + C8 > x_pitch)
        return DCFP_E_BADDESC;
    PyrGeom G;
    const int st = pyr_geom(N, H, W, C8, nlev, sizes, G);
    if (st != DCFP_OK) return st;
    PyrOut out{};
    int nbins = 0;
    for (int l = 0; l < nlev; ++l) {
        if (!y[l] || !dcfp_aligned16(y[l]) || !mult8(y_pitch[l]) || y_pitch[l] < C8) return DCFP_E_BADDESC;
        out.y[l] = reinterpret_cast<_Float16*>(y[l]);
        out.pitch[l] = y_pitch[l];
        nbins += sizes[l] * sizes[l];
    }
    if (!workspace || !dcfp_aligned16(workspace) ||
        workspace_bytes < dcfp_pyramid_pool_nhwc_f16_workspace_bytes(N, H, W, C8, nlev, sizes))
        return DCFP_E_WORKSPACE;
    const int c8n = C8 / 8;
    float* part = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(pyramid_partial_kernel, dim3(G.nra * G.nca, (c8n + kChunks - 1) / kChunks, N), dim3(256), 0,
                       dcfp_s(stream), reinterpret_cast<const h8_t*>(x), part, H, W, c8n, x_pitch / 8, x_off / 8, G);
    const long total = (long)N * nbins * c8n;
    hipLaunchKernelGGL(pyramid_final_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream), part, out, c8n,
                       nbins, total, G);
    DCFP_RETURN_LAUNCH();
}

}  // extern "C"
