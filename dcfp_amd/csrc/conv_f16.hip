// conv_f16.hip — the kernels of the frozen fp16 inference engine (dcfp_amd/deploy.py).
//
// Implicit-GEMM forward conv on the fp16 matrix cores: D[co][pixel] = sum_k W[co][k] * X[k][pixel] with
// k = (tap, ci) and v_mfma_f32_32x32x16_f16.  Both operands of that instruction take 8 consecutive k per lane
// (A: row = lane & 31, k = 8 (lane >> 5) + j; B: col = lane & 31, same k), so with NHWC fp16 activations (channels
// padded to 8) and weights packed [Cout8][kh][kw][Cin8] every lane's fragment is one 16-byte chunk of one pixel /
// one filter row.  The weights are the A operand: the accumulator then has the pixel on the lane and four consecutive
// output channels in each group of four registers: 8 bytes of an NHWC pixel, staged through LDS into 16-byte stores
// that cover a pixel's channels contiguously (or, for the classifier, 32 lanes on 32 consecutive pixels of an NCHW
// plane, stored directly).
//
// Block: 256 threads = 4 waves, BM output channels x 128 pixels x 64 k per step; BM = 128 / 64 / 32 by Cout.
// Global -> registers -> LDS, two LDS stages, one barrier per step: the loads of step t+1 are issued before the
// MFMAs of step t and written to the other stage after them.  LDS rows are 128 B (64 k); the 16-byte chunk c of row r
// sits at chunk c ^ ((r >> 1) & 7), which makes the ds_read_b128 of a fragment (32 rows, one chunk) and the
// ds_write_b128 of the staging pass (8 lanes per row) conflict free.
#include "common.h"

typedef _Float16 h8_t __attribute__((ext_vector_type(8)));
typedef _Float16 h4_t __attribute__((ext_vector_type(4)));
typedef float f16x_t __attribute__((ext_vector_type(16)));

namespace {

struct ConvF16Params {
    const uint4* x;       // NHWC fp16, in 16-byte chunks
    const uint4* w;       // [rows][taps][Cin8]
    const float* shift;
    const _Float16* res;
    void* y;
    int P, HoWo, Wo, H, W;
    int x_pitch8;         // chunks per pixel of x
    int cpt;              // chunks per tap = Cin8 / 8
    int KC;               // chunks per filter row = taps * cpt
    int wrows;            // rows of w (Cout rounded up to 8)
    int Cout;
    int KW, stride, pad, dil;
    int y_pitch, y_off, res_pitch, res_off, relu;
    int n_co_tiles;
};

constexpr int BN = 128, BK8 = 8;   // pixels per block; 16-byte chunks (8 k each) per row and step

__device__ __forceinline__ int lds_slot(int row, int c) { return row * BK8 + (c ^ ((row >> 1) & 7)); }

template <int BM, int WM, bool F32OUT>
__global__ __launch_bounds__(256) void conv_f16_kernel(ConvF16Params p) {
    constexpr int WN = 4 / WM;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int A_LOADS = BM * BK8 / 256, B_LOADS = BN * BK8 / 256;
    constexpr int STAGE = (BM + BN) * BK8;
    __shared__ uint4 lds[2 * STAGE];

    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const int co_base = (blockIdx.x % p.n_co_tiles) * BM;
    const int pix_base = (blockIdx.x / p.n_co_tiles) * BN;
    const int c = t & 7, r0 = t >> 3;

    // the B_LOADS pixels this thread stages: top-left input coordinate and image base (in pixels)
    int iy0[B_LOADS], ix0[B_LOADS], nb[B_LOADS];
#pragma unroll
    for (int i = 0; i < B_LOADS; ++i) {
        const int pix = pix_base + r0 + 32 * i;
        if (pix < p.P) {
            const int n = pix / p.HoWo, rem = pix - n * p.HoWo;
            const int oy = rem / p.Wo, ox = rem - oy * p.Wo;
            iy0[i] = oy * p.stride - p.pad;
            ix0[i] = ox * p.stride - p.pad;
            nb[i] = n * p.H * p.W;
        } else {
            iy0[i] = -(1 << 28); ix0[i] = -(1 << 28); nb[i] = 0;   // every tap lands outside: zeros
        }
    }

    uint4 ra[A_LOADS], rb[B_LOADS];
    auto load_global = [&](int kt) {
        const int kc = kt * BK8 + c;
        const bool kin = kc < p.KC;
        int dy = 0, dx = 0, ci = 0;
        if (kin) {
            const int tap = kc / p.cpt;
            ci = kc - tap * p.cpt;
            const int ky = tap / p.KW, kx = tap - ky * p.KW;
            dy = ky * p.dil; dx = kx * p.dil;
        }
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) {
            const int row = co_base + r0 + 32 * i;
            ra[i] = (kin && row < p.wrows) ? p.w[(size_t)row * p.KC + kc] : make_uint4(0, 0, 0, 0);
        }
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) {
            const int iy = iy0[i] + dy, ix = ix0[i] + dx;
            const bool in = kin && iy >= 0 && iy < p.H && ix >= 0 && ix < p.W;
            rb[i] = in ? p.x[(size_t)(nb[i] + iy * p.W + ix) * p.x_pitch8 + ci] : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_lds = [&](int buf) {
        uint4* a = lds + buf * STAGE;
        uint4* b = a + BM * BK8;
#pragma unroll
        for (int i = 0; i < A_LOADS; ++i) a[lds_slot(r0 + 32 * i, c)] = ra[i];
#pragma unroll
        for (int i = 0; i < B_LOADS; ++i) b[lds_slot(r0 + 32 * i, c)] = rb[i];
    };

    f16x_t acc[TM][TN];
#pragma unroll
    for (int i = 0; i < TM; ++i)
#pragma unroll
        for (int j = 0; j < TN; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    const int KT = (p.KC + BK8 - 1) / BK8;
    const int fr = lane & 31, fh = lane >> 5;
    load_global(0);
    store_lds(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const bool more = kt + 1 < KT;
        if (more) load_global(kt + 1);
        const h8_t* a = reinterpret_cast<const h8_t*>(lds + (kt & 1) * STAGE);
        const h8_t* b = a + BM * BK8;
#pragma unroll
        for (int ks = 0; ks < BK8 / 2; ++ks) {
            const int cc = ks * 2 + fh;
            h8_t fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) fa[i] = a[lds_slot(wm * (BM / WM) + i * 32 + fr, cc)];
#pragma unroll
            for (int j = 0; j < TN; ++j) fb[j] = b[lds_slot(wn * (BN / WN) + j * 32 + fr, cc)];
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_32x32x16_f16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        if (more) store_lds((kt + 1) & 1);
        __syncthreads();
    }

    // epilogue: register group g of a 32x32 tile = output channels 8g + 4 fh .. + 3 of pixel fr
    if constexpr (F32OUT) {
        float* y = reinterpret_cast<float*>(p.y);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int pix = pix_base + wn * (BN / WN) + j * 32 + fr;
            if (pix >= p.P) continue;
            const int n = pix / p.HoWo, rem = pix - n * p.HoWo;
            const size_t ybase = (size_t)n * p.Cout * p.HoWo + rem;      // 32 lanes = 32 consecutive pixels of a plane
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int co = co_base + wm * (BM / WM) + i * 32 + 8 * g + 4 * fh;
                    if (co >= p.Cout) continue;
                    const float4 sh = *reinterpret_cast<const float4*>(p.shift + co);
                    const float v[4] = {acc[i][j][4 * g] + sh.x, acc[i][j][4 * g + 1] + sh.y,
                                        acc[i][j][4 * g + 2] + sh.z, acc[i][j][4 * g + 3] + sh.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cout) y[ybase + (size_t)(co + e) * p.HoWo] = v[e];
                }
        }
    } else {
        // shift, residual, ReLU and the one rounding in registers; the fp16 tile then goes through LDS (free after the
        // last barrier of the K loop) as [pixel][channel] rows, so that the global stores are 16 bytes per lane with
        // BM / 8 consecutive lanes on one pixel's contiguous channels, instead of 8 bytes per lane on 32 pixels
        constexpr int ROWB = BM * 2 + 16;   // bytes per staged pixel row; BN * ROWB <= the K loop's LDS
        static_assert(BN * ROWB <= 2 * STAGE * 16, "staged output tile must fit");
        char* stg = reinterpret_cast<char*>(lds);
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const int pl = wn * (BN / WN) + j * 32 + fr;
            const int pix = pix_base + pl;
            if (pix >= p.P) continue;
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int cl = wm * (BM / WM) + i * 32 + 8 * g + 4 * fh;
                    const int co = co_base + cl;
                    if (co >= p.Cout) continue;
                    const float4 sh = *reinterpret_cast<const float4*>(p.shift + co);
                    float v[4] = {acc[i][j][4 * g] + sh.x, acc[i][j][4 * g + 1] + sh.y, acc[i][j][4 * g + 2] + sh.z,
                                  acc[i][j][4 * g + 3] + sh.w};
                    if (p.res) {
                        const h4_t rv = *reinterpret_cast<const h4_t*>(p.res + (size_t)pix * p.res_pitch + p.res_off + co);
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] += (float)rv[e];
                    }
                    h4_t o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = (_Float16)((p.relu && v[e] < 0.f) ? 0.f : v[e]);
                    *reinterpret_cast<h4_t*>(stg + pl * ROWB + cl * 2) = o;
                }
        }
        __syncthreads();
        constexpr int CPR = BM / 8;         // 16-byte chunks per pixel row
        _Float16* y = reinterpret_cast<_Float16*>(p.y);
#pragma unroll
        for (int idx = t; idx < BN * CPR; idx += 256) {
            const int pl = idx / CPR, ch = idx - pl * CPR;
            const int pix = pix_base + pl, co = co_base + ch * 8;
            if (pix < p.P && co < p.Cout)   // (Cout is a multiple of 8: a chunk is written whole or not at all)
                *reinterpret_cast<uint4*>(y + (size_t)pix * p.y_pitch + p.y_off + co) =
                    *reinterpret_cast<const uint4*>(stg + pl * ROWB + ch * 16);
        }
    }
}

bool mult8(int v) { return v > 0 && (v & 7) == 0; }

int check_desc(const DcfpConvF16Desc* d, bool f32out) {
    if (!d) return DCFP_E_BADDESC;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 || d->Hout <= 0 || d->Wout <= 0) return DCFP_E_BADDESC;
    if (!mult8(d->Cin8) || !mult8(d->x_pitch) || d->x_pitch < d->Cin8) return DCFP_E_BADDESC;
    if (d->K != 1 && d->K != 3) return DCFP_E_UNSUPPORTED;
    if (d->stride != 1 && d->stride != 2) return DCFP_E_UNSUPPORTED;
    if (d->dil < 1 || d->dil > 4096 || d->pad < 0 || d->pad > 8192) return DCFP_E_UNSUPPORTED;
    if (d->H > 32768 || d->W > 32768) return DCFP_E_UNSUPPORTED;
    const int ext = d->dil * (d->K - 1) + 1;
    if (d->H + 2 * d->pad < ext || d->W + 2 * d->pad < ext) return DCFP_E_BADDESC;
    if (d->Hout != (d->H + 2 * d->pad - ext) / d->stride + 1 || d->Wout != (d->W + 2 * d->pad - ext) / d->stride + 1)
        return DCFP_E_BADDESC;
    if ((int64_t)d->N * d->H * d->W >= (1ll << 31) || (int64_t)d->N * d->Hout * d->Wout >= (1ll << 31) - BN)
        return DCFP_E_UNSUPPORTED;
    if (!f32out) {
        if (!mult8(d->Cout) || !mult8(d->y_pitch) || d->y_off < 0 || (d->y_off & 7) || d->y_off + d->Cout > d->y_pitch)
            return DCFP_E_BADDESC;
    }
    return DCFP_OK;
}

template <bool F32OUT>
int launch_conv(const DcfpConvF16Desc* d, ConvF16Params& p, hipStream_t s) {
    // the block height that pads Cout least, the tallest within 15 % of that (a taller block re-reads x less)
    int bm = 32;
    const long need32 = (d->Cout + 31) / 32 * 32;
    if ((d->Cout + 127) / 128 * 128 * 100L <= need32 * 115) bm = 128;
    else if ((d->Cout + 63) / 64 * 64 * 100L <= need32 * 115) bm = 64;
    p.n_co_tiles = (d->Cout + bm - 1) / bm;
    const long grid = (long)p.n_co_tiles * ((p.P + BN - 1) / BN);
    if (grid >= (1l << 31)) return DCFP_E_UNSUPPORTED;
    if (bm == 128) hipLaunchKernelGGL((conv_f16_kernel<128, 2, F32OUT>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else if (bm == 64) hipLaunchKernelGGL((conv_f16_kernel<64, 2, F32OUT>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv_f16_kernel<32, 1, F32OUT>), dim3((unsigned)grid), dim3(256), 0, s, p);
    DCFP_RETURN_LAUNCH();
}

ConvF16Params make_params(const DcfpConvF16Desc* d, const void* x, const void* w, const float* shift) {
    ConvF16Params p{};
    p.x = reinterpret_cast<const uint4*>(x);
    p.w = reinterpret_cast<const uint4*>(w);
    p.shift = shift;
    p.P = d->N * d->Hout * d->Wout; p.HoWo = d->Hout * d->Wout; p.Wo = d->Wout; p.H = d->H; p.W = d->W;
    p.x_pitch8 = d->x_pitch / 8; p.cpt = d->Cin8 / 8; p.KC = d->K * d->K * p.cpt;
    p.wrows = (d->Cout + 7) / 8 * 8; p.Cout = d->Cout;
    p.KW = d->K; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    return p;
}

// ---------------------------------------------------------------- small NHWC fp16 kernels
__global__ __launch_bounds__(256) void maxpool_nhwc_f16_kernel(const h8_t* __restrict__ x, h8_t* __restrict__ y,
                                                               long total, int H, int W, int c8n, int xp8, int Ho,
                                                               int Wo, int yp8) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c8n);
    long pix = idx / c8n;
    const int ox = (int)(pix % Wo); pix /= Wo;
    const int oy = (int)(pix % Ho);
    const long n = pix / Ho;
    h8_t m;
#pragma unroll
    for (int e = 0; e < 8; ++e) m[e] = (_Float16)(-65504.f);   // every window of a 3x3 / 2 / 1 pool holds a pixel
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const h8_t v = x[((n * H + iy) * W + ix) * xp8 + ch];
#pragma unroll
            for (int e = 0; e < 8; ++e) m[e] = v[e] > m[e] ? v[e] : m[e];
        }
    }
    y[((n * Ho + oy) * (long)Wo + ox) * yp8 + ch] = m;
}

constexpr int AVG_PIX_LANES = 8;   // pixel slices per block of 32 channel chunks
__global__ __launch_bounds__(256) void avgpool_partial_kernel(const h8_t* __restrict__ x, float* __restrict__ part,
                                                              long HW, int c8n, int xp8, int S) {
    // block: 32 chunks x 8 pixel lanes; grid (chunk groups, S pixel splits, N); part [N][S][c8n * 8]
    __shared__ float red[AVG_PIX_LANES][32][8];
    const int cl = threadIdx.x & 31, pl = threadIdx.x >> 5;
    const int ch = blockIdx.x * 32 + cl, s = blockIdx.y;
    const long n = blockIdx.z;
    const long per = (HW + S - 1) / S, lo = s * per, hi = (lo + per < HW) ? lo + per : HW;
    float a[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    if (ch < c8n)
        for (long q = lo + pl; q < hi; q += AVG_PIX_LANES) {
            const h8_t v = x[(n * HW + q) * xp8 + ch];
#pragma unroll
            for (int e = 0; e < 8; ++e) a[e] += (float)v[e];
        }
#pragma unroll
    for (int e = 0; e < 8; ++e) red[pl][cl][e] = a[e];
    __syncthreads();
    if (pl == 0 && ch < c8n) {
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float t = 0.f;
#pragma unroll
            for (int q = 0; q < AVG_PIX_LANES; ++q) t += red[q][cl][e];
            part[((n * S + s) * c8n + ch) * 8 + e] = t;
        }
    }
}

__global__ __launch_bounds__(256) void avgpool_final_kernel(const float* __restrict__ part, _Float16* __restrict__ y,
                                                            int C8, int S, int y_pitch, float inv, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % C8);
    const long n = idx / C8;
    float t = 0.f;
    for (int s = 0; s < S; ++s) t += part[(n * S + s) * C8 + ch];
    y[n * y_pitch + ch] = (_Float16)(t * inv);
}

int avg_splits(int64_t HW) {
    const int64_t s = (HW + 255) / 256;
    return (int)(s < 1 ? 1 : (s > 64 ? 64 : s));
}

__global__ __launch_bounds__(256) void broadcast_nhwc_f16_kernel(const h8_t* __restrict__ v, int vp8,
                                                                 h8_t* __restrict__ y, long HW, int c8n, int yp8,
                                                                 int yo8, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c8n);
    const long pix = idx / c8n;   // n * HW + p
    const long n = pix / HW;
    y[pix * yp8 + yo8 + ch] = v[n * vp8 + ch];
}

__global__ __launch_bounds__(256) void nchw_f32_to_nhwc_f16_kernel(const float* __restrict__ x, h8_t* __restrict__ y,
                                                                   int C, long HW, int c8n, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;   // (chunk, pixel): pixel fastest, coalesced plane reads
    if (idx >= total) return;
    const long NHW = total / c8n;
    const int ch = (int)(idx / NHW);
    const long pix = idx - ch * NHW;
    const long n = pix / HW, q = pix - n * HW;
    h8_t o;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int cc = ch * 8 + e;
        o[e] = cc < C ? (_Float16)x[(n * C + cc) * HW + q] : (_Float16)0.f;
    }
    y[pix * c8n + ch] = o;
}

unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" {

int dcfp_conv2d_fwd_f16_nhwc(const DcfpConvF16Desc* d, const void* x, const void* w_packed, const float* shift,
                             const void* residual, void* y, dcfp_stream_t stream) {
    const int st = check_desc(d, false);
    if (st != DCFP_OK) return st;
    if (!x || !w_packed || !shift || !y) return DCFP_E_BADDESC;
    if (!dcfp_aligned16(x) || !dcfp_aligned16(w_packed) || !dcfp_aligned16(shift) || !dcfp_aligned16(y) ||
        !dcfp_aligned16(residual))
        return DCFP_E_BADDESC;
    if (residual && (!mult8(d->res_pitch) || d->res_off < 0 || (d->res_off & 7) || d->res_off + d->Cout > d->res_pitch))
        return DCFP_E_BADDESC;
    ConvF16Params p = make_params(d, x, w_packed, shift);
    p.res = reinterpret_cast<const _Float16*>(residual);
    p.y = y;
    p.y_pitch = d->y_pitch; p.y_off = d->y_off; p.res_pitch = d->res_pitch; p.res_off = d->res_off;
    p.relu = d->relu != 0;
    return launch_conv<false>(d, p, dcfp_s(stream));
}

int dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw(const DcfpConvF16Desc* d, const void* x, const void* w_packed,
                                         const float* bias, float* y, dcfp_stream_t stream) {
    const int st = check_desc(d, true);
    if (st != DCFP_OK) return st;
    if (!x || !w_packed || !bias || !y) return DCFP_E_BADDESC;
    if (!dcfp_aligned16(x) || !dcfp_aligned16(w_packed) || !dcfp_aligned16(bias)) return DCFP_E_BADDESC;
    ConvF16Params p = make_params(d, x, w_packed, bias);
    p.y = y;
    return launch_conv<true>(d, p, dcfp_s(stream));
}

int dcfp_maxpool3x3s2_nhwc_f16(const void* x, void* y, int N, int H, int W, int C8, int x_pitch, int Ho, int Wo,
                               int y_pitch, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || !mult8(C8) || !mult8(x_pitch) || !mult8(y_pitch) || x_pitch < C8 ||
        y_pitch < C8 || !dcfp_aligned16(x) || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    if (Ho != (H - 1) / 2 + 1 || Wo != (W - 1) / 2 + 1) return DCFP_E_BADDESC;
    const long total = (long)N * Ho * Wo * (C8 / 8);
    if (total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(maxpool_nhwc_f16_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const h8_t*>(x), reinterpret_cast<h8_t*>(y), total, H, W, C8 / 8, x_pitch / 8,
                       Ho, Wo, y_pitch / 8);
    DCFP_RETURN_LAUNCH();
}

size_t dcfp_avgpool_nhwc_f16_workspace_bytes(int N, int C8, int64_t HW) {
    if (N <= 0 || C8 <= 0 || HW <= 0) return 0;
    return (size_t)N * avg_splits(HW) * C8 * sizeof(float);
}

int dcfp_avgpool_nhwc_f16(const void* x, void* y, int N, int64_t HW, int C8, int x_pitch, int y_pitch,
                          void* workspace, size_t workspace_bytes, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || N > 65535 || HW <= 0 || !mult8(C8) || !mult8(x_pitch) || x_pitch < C8 || y_pitch < C8 ||
        !dcfp_aligned16(x))
        return DCFP_E_BADDESC;
    if (!workspace || workspace_bytes < dcfp_avgpool_nhwc_f16_workspace_bytes(N, C8, HW)) return DCFP_E_WORKSPACE;
    const int S = avg_splits(HW), c8n = C8 / 8;
    float* part = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(avgpool_partial_kernel, dim3((c8n + 31) / 32, S, N), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const h8_t*>(x), part, (long)HW, c8n, x_pitch / 8, S);
    const long total = (long)N * C8;
    hipLaunchKernelGGL(avgpool_final_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream), part,
                       reinterpret_cast<_Float16*>(y), C8, S, y_pitch, 1.0f / (float)HW, total);
    DCFP_RETURN_LAUNCH();
}

int dcfp_broadcast_nhwc_f16(const void* v, int v_pitch, void* y, int N, int64_t HW, int C8, int y_pitch, int y_off,
                            dcfp_stream_t stream) {
    if (!v || !y || N <= 0 || HW <= 0 || !mult8(C8) || !mult8(v_pitch) || !mult8(y_pitch) || v_pitch < C8 ||
        y_off < 0 || (y_off & 7) || y_off + C8 > y_pitch || !dcfp_aligned16(v) || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    const long total = (long)N * HW * (C8 / 8);
    if (total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(broadcast_nhwc_f16_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const h8_t*>(v), v_pitch / 8, reinterpret_cast<h8_t*>(y), (long)HW, C8 / 8,
                       y_pitch / 8, y_off / 8, total);
    DCFP_RETURN_LAUNCH();
}

int dcfp_nchw_f32_to_nhwc_f16(const float* x, void* y, int N, int C, int H, int W, int C8, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || C <= 0 || H <= 0 || W <= 0 || !mult8(C8) || C8 < C || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    const long total = (long)N * H * W * (C8 / 8);
    if (total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(nchw_f32_to_nhwc_f16_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream), x,
                       reinterpret_cast<h8_t*>(y), C, (long)H * W, C8 / 8, total);
    DCFP_RETURN_LAUNCH();
}

}  // extern "C"
