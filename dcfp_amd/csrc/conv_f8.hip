// conv_f8.hip — the kernels of the calibrated fp8 inference engine (dcfp_amd/deploy.py).
//
// Every 8-bit value is OCP e4m3fn (bias 7, largest finite 448, no infinities).  Every conversion to it follows one
// rule: clamp the fp32 value to [-448, 448], then round to nearest even (v_cvt_pk_fp8_f32); subnormals are kept.
//
// The conv is conv_f16.hip's implicit GEMM with 16 k per 16-byte chunk instead of 8: D[co][pixel] = sum_k W[co][k] *
// X[k][pixel], k = (tap, ci), activations NHWC fp8 with channels padded to 16, weights [Cout8][kh][kw][Cin16] fp8.  Both
// operands of an fp8 MFMA take the same k in the same byte of the same lane, so a product over a 32x32 tile is
// sum over (lane half h, byte b) of A[row][h][b] * B[col][h][b], whatever k a byte holds: any chunk-to-lane assignment
// that is the same for A and B is correct.  The instruction is v_mfma_scale_f32_32x32x64_f8f6f4 with unit (0x7f = 2^0)
// block scales: lane half h takes chunks 4s + 2h and 4s + 2h + 1 of a 128-k LDS row in step s = 0, 1 (32 bytes per lane
// and operand).  The unscaled v_mfma_f32_32x32x16_fp8_fp8 (chunk 2s + h, its low and high 8 bytes in two instructions)
// was built in the same loop and measured 9 - 11 % slower end to end, so it is not kept.
// The weights are the A operand, so the accumulator has the pixel on the lane and four consecutive output channels in
// each group of four registers: 4 bytes of an NHWC pixel after the epilogue
//     v = acc * mul[co] + add[co] (+ res_mul * float(res)) -> ReLU? -> clamp -> fp8,
// staged through LDS as [pixel][channel] rows so that the global stores are 16 bytes per lane.  The classifier form
// stores acc * mul + add as fp32 NCHW directly.
//
// Block: 256 threads = 4 waves, BM output channels x 128 pixels x 128 k per step, global -> registers -> LDS, two
// stages, one barrier per step, the LDS swizzle of conv_f16.hip (rows are 128 bytes there too).
#include "common.h"

typedef float f16x_t __attribute__((ext_vector_type(16)));
typedef int i8x_t __attribute__((ext_vector_type(8)));
typedef _Float16 h8_t __attribute__((ext_vector_type(8)));

namespace {

struct ConvF8Params {
    const uint4* x;       // NHWC fp8, in 16-byte chunks
    const uint4* w;       // [rows][taps][Cin16]
    const float* mul;
    const float* add;
    const unsigned char* res;
    void* y;
    int P, HoWo, Wo, H, W;
    int x_pitch16;        // chunks per pixel of x
    int cpt;              // chunks per tap = Cin16 / 16
    int KC;               // chunks per filter row = taps * cpt
    int wrows;            // rows of w (Cout rounded up to 8)
    int Cout, Cout16;     // true output channels; channels written by the fp8 form (Cout rounded up to 16)
    int KW, stride, pad, dil;
    int y_pitch, y_off, res_pitch, res_off, relu;
    float res_mul;
    int n_co_tiles;
};

constexpr int BN = 128, BKC = 8;   // pixels per block; 16-byte chunks (16 k each) per row and step
constexpr float F8_MAX = 448.f;

__device__ __forceinline__ int lds_slot(int row, int c) { return row * BKC + (c ^ ((row >> 1) & 7)); }

__device__ __forceinline__ float clamp_f8(float v) { return __builtin_amdgcn_fmed3f(v, -F8_MAX, F8_MAX); }

// four fp32 values -> four e4m3 bytes (byte e = value e), clamped, round to nearest even
__device__ __forceinline__ unsigned pack4_f8(float a, float b, float c, float d) {
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_f8(a), clamp_f8(b), 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(clamp_f8(c), clamp_f8(d), w, true);
    return (unsigned)w;
}

template <int E>
__device__ __forceinline__ float f8_byte(unsigned w) { return __builtin_amdgcn_cvt_f32_fp8((int)w, E); }

__device__ __forceinline__ void decode4(unsigned w, float* f) {
    f[0] = f8_byte<0>(w); f[1] = f8_byte<1>(w); f[2] = f8_byte<2>(w); f[3] = f8_byte<3>(w);
}

template <int BM, int WM, bool F32OUT>
__global__ __launch_bounds__(256) void conv_f8_kernel(ConvF8Params p) {
    constexpr int WN = 4 / WM;
    constexpr int TM = BM / WM / 32, TN = BN / WN / 32;
    constexpr int A_LOADS = BM * BKC / 256, B_LOADS = BN * BKC / 256;
    constexpr int STAGE = (BM + BN) * BKC;
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
        const int kc = kt * BKC + c;
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
            rb[i] = in ? p.x[(size_t)(nb[i] + iy * p.W + ix) * p.x_pitch16 + ci] : make_uint4(0, 0, 0, 0);
        }
    };
    auto store_lds = [&](int buf) {
        uint4* a = lds + buf * STAGE;
        uint4* b = a + BM * BKC;
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

    const int KT = (p.KC + BKC - 1) / BKC;
    const int fr = lane & 31, fh = lane >> 5;
    load_global(0);
    store_lds(0);
    __syncthreads();
    for (int kt = 0; kt < KT; ++kt) {
        const bool more = kt + 1 < KT;
        if (more) load_global(kt + 1);
        const uint4* a = lds + (kt & 1) * STAGE;
        const uint4* b = a + BM * BKC;
#pragma unroll
        for (int ks = 0; ks < BKC / 4; ++ks) {
            const int cc = ks * 4 + fh * 2;
            i8x_t fa[TM], fb[TN];
#pragma unroll
            for (int i = 0; i < TM; ++i) {
                const int row = wm * (BM / WM) + i * 32 + fr;
                const uint4 lo = a[lds_slot(row, cc)], hi = a[lds_slot(row, cc + 1)];
                fa[i] = i8x_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const int row = wn * (BN / WN) + j * 32 + fr;
                const uint4 lo = b[lds_slot(row, cc)], hi = b[lds_slot(row, cc + 1)];
                fb[j] = i8x_t{(int)lo.x, (int)lo.y, (int)lo.z, (int)lo.w, (int)hi.x, (int)hi.y, (int)hi.z, (int)hi.w};
            }
#pragma unroll
            for (int i = 0; i < TM; ++i)
#pragma unroll
                for (int j = 0; j < TN; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(
                        fa[i], fb[j], acc[i][j], 0 /* A: e4m3 */, 0 /* B: e4m3 */, 0, 0x7f7f7f7f, 0, 0x7f7f7f7f);
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
                    const float4 m4 = *reinterpret_cast<const float4*>(p.mul + co);
                    const float4 a4 = *reinterpret_cast<const float4*>(p.add + co);
                    const float v[4] = {acc[i][j][4 * g] * m4.x + a4.x, acc[i][j][4 * g + 1] * m4.y + a4.y,
                                        acc[i][j][4 * g + 2] * m4.z + a4.z, acc[i][j][4 * g + 3] * m4.w + a4.w};
#pragma unroll
                    for (int e = 0; e < 4; ++e)
                        if (co + e < p.Cout) y[ybase + (size_t)(co + e) * p.HoWo] = v[e];
                }
        }
    } else {
        // scale, shift, residual, ReLU, clamp and the one rounding in registers; the fp8 tile then goes through LDS
        // (free after the last barrier of the K loop) as [pixel][channel] rows: 16-byte global stores, BM / 16
        // consecutive lanes on one pixel's contiguous channels
        constexpr int ROWB = BM + 16;   // bytes per staged pixel row
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
                    if (co >= p.Cout16) continue;
                    unsigned out = 0;                 // channels Cout .. Cout16 - 1: exact zeros
                    if (co < p.Cout) {
                        const float4 m4 = *reinterpret_cast<const float4*>(p.mul + co);
                        const float4 a4 = *reinterpret_cast<const float4*>(p.add + co);
                        float v[4] = {acc[i][j][4 * g] * m4.x + a4.x, acc[i][j][4 * g + 1] * m4.y + a4.y,
                                      acc[i][j][4 * g + 2] * m4.z + a4.z, acc[i][j][4 * g + 3] * m4.w + a4.w};
                        if (p.res) {
                            float rv[4];
                            decode4(*reinterpret_cast<const unsigned*>(p.res + (size_t)pix * p.res_pitch + p.res_off + co), rv);
#pragma unroll
                            for (int e = 0; e < 4; ++e) v[e] += p.res_mul * rv[e];
                        }
#pragma unroll
                        for (int e = 0; e < 4; ++e) v[e] = ((p.relu && v[e] < 0.f) || co + e >= p.Cout) ? 0.f : v[e];
                        out = pack4_f8(v[0], v[1], v[2], v[3]);
                    }
                    *reinterpret_cast<unsigned*>(stg + pl * ROWB + cl) = out;
                }
        }
        __syncthreads();
        constexpr int CPR = BM / 16;        // 16-byte chunks per pixel row
        unsigned char* y = reinterpret_cast<unsigned char*>(p.y);
#pragma unroll
        for (int idx = t; idx < BN * CPR; idx += 256) {
            const int pl = idx / CPR, ch = idx - pl * CPR;
            const int pix = pix_base + pl, co = co_base + ch * 16;
            if (pix < p.P && co < p.Cout16)   // (Cout16 is a multiple of 16: a chunk is written whole or not at all)
                *reinterpret_cast<uint4*>(y + (size_t)pix * p.y_pitch + p.y_off + co) =
                    *reinterpret_cast<const uint4*>(stg + pl * ROWB + ch * 16);
        }
    }
}

bool mult16(int v) { return v > 0 && (v & 15) == 0; }
bool mult8(int v) { return v > 0 && (v & 7) == 0; }
int r16(int v) { return (v + 15) / 16 * 16; }

int check_desc(const DcfpConvF8Desc* d, bool f32out) {
    if (!d) return DCFP_E_BADDESC;
    if (d->N <= 0 || d->H <= 0 || d->W <= 0 || d->Cout <= 0 || d->Hout <= 0 || d->Wout <= 0) return DCFP_E_BADDESC;
    if (d->Cout > (1 << 24)) return DCFP_E_UNSUPPORTED;
    if (!mult16(d->Cin16) || !mult16(d->x_pitch) || d->x_pitch < d->Cin16) return DCFP_E_BADDESC;
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
        if (!mult16(d->y_pitch) || d->y_off < 0 || (d->y_off & 15) || d->y_off + r16(d->Cout) > d->y_pitch)
            return DCFP_E_BADDESC;
    }
    return DCFP_OK;
}

template <bool F32OUT>
int launch_conv(const DcfpConvF8Desc* d, ConvF8Params& p, hipStream_t s) {
    // the block height that pads Cout least, the tallest within 15 % of that (a taller block re-reads x less)
    int bm = 32;
    const long need32 = (d->Cout + 31) / 32 * 32;
    if ((d->Cout + 127) / 128 * 128 * 100L <= need32 * 115) bm = 128;
    else if ((d->Cout + 63) / 64 * 64 * 100L <= need32 * 115) bm = 64;
    p.n_co_tiles = (d->Cout + bm - 1) / bm;
    const long grid = (long)p.n_co_tiles * ((p.P + BN - 1) / BN);
    if (grid >= (1l << 31)) return DCFP_E_UNSUPPORTED;
    if (bm == 128) hipLaunchKernelGGL((conv_f8_kernel<128, 2, F32OUT>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else if (bm == 64) hipLaunchKernelGGL((conv_f8_kernel<64, 2, F32OUT>), dim3((unsigned)grid), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((conv_f8_kernel<32, 1, F32OUT>), dim3((unsigned)grid), dim3(256), 0, s, p);
    DCFP_RETURN_LAUNCH();
}

ConvF8Params make_params(const DcfpConvF8Desc* d, const void* x, const void* w, const float* mul, const float* add) {
    ConvF8Params p{};
    p.x = reinterpret_cast<const uint4*>(x);
    p.w = reinterpret_cast<const uint4*>(w);
    p.mul = mul; p.add = add;
    p.P = d->N * d->Hout * d->Wout; p.HoWo = d->Hout * d->Wout; p.Wo = d->Wout; p.H = d->H; p.W = d->W;
    p.x_pitch16 = d->x_pitch / 16; p.cpt = d->Cin16 / 16; p.KC = d->K * d->K * p.cpt;
    p.wrows = (d->Cout + 7) / 8 * 8; p.Cout = d->Cout; p.Cout16 = r16(d->Cout);
    p.KW = d->K; p.stride = d->stride; p.pad = d->pad; p.dil = d->dil;
    return p;
}

// ---------------------------------------------------------------- small NHWC fp8 kernels
// 16 fp32 values -> one 16-byte chunk of e4m3
__device__ __forceinline__ uint4 pack16_f8(const float* v) {
    return make_uint4(pack4_f8(v[0], v[1], v[2], v[3]), pack4_f8(v[4], v[5], v[6], v[7]),
                      pack4_f8(v[8], v[9], v[10], v[11]), pack4_f8(v[12], v[13], v[14], v[15]));
}

// channels 16 ch .. 16 ch + 15 of an fp16 row (x8: its 8-channel chunks), times scale; channels >= C are zero
__device__ __forceinline__ uint4 row16_f16_to_f8(const h8_t* x8, int ch, int C, float scale) {
    float v[16];
#pragma unroll
    for (int half = 0; half < 2; ++half) {
        const int c0 = ch * 16 + half * 8;
        h8_t h;
#pragma unroll
        for (int e = 0; e < 8; ++e) h[e] = (_Float16)0.f;
        if (c0 < C) h = x8[ch * 2 + half];     // (the chunk lies inside the C rounded up to 8 the caller vouches for)
#pragma unroll
        for (int e = 0; e < 8; ++e) v[half * 8 + e] = (c0 + e < C) ? (float)h[e] * scale : 0.f;
    }
    return pack16_f8(v);
}

__global__ __launch_bounds__(256) void cast_nhwc_f16_to_f8_kernel(const h8_t* __restrict__ x, int xp8,
                                                                  uint4* __restrict__ y, int yp16, int yo16, int C,
                                                                  int c16n, float scale, long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c16n);
    const long pix = idx / c16n;
    y[pix * yp16 + yo16 + ch] = row16_f16_to_f8(x + pix * xp8, ch, C, scale);
}

__global__ __launch_bounds__(256) void broadcast_nhwc_f16_to_f8_kernel(const h8_t* __restrict__ v, int vp8,
                                                                       uint4* __restrict__ y, long HW, int yp16,
                                                                       int yo16, int C, int c16n, float scale,
                                                                       long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c16n);
    const long pix = idx / c16n;   // n * HW + p
    const long n = pix / HW;
    y[pix * yp16 + yo16 + ch] = row16_f16_to_f8(v + n * vp8, ch, C, scale);
}

__global__ __launch_bounds__(256) void maxpool_nhwc_f8_kernel(const uint4* __restrict__ x, uint4* __restrict__ y,
                                                              long total, int H, int W, int c16n, int xp16, int Ho,
                                                              int Wo, int yp16) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % c16n);
    long pix = idx / c16n;
    const int ox = (int)(pix % Wo); pix /= Wo;
    const int oy = (int)(pix % Ho);
    const long n = pix / Ho;
    float m[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) m[e] = -F8_MAX;   // every window of a 3x3 / 2 / 1 pool holds a pixel
#pragma unroll
    for (int ky = 0; ky < 3; ++ky) {
        const int iy = oy * 2 - 1 + ky;
        if (iy < 0 || iy >= H) continue;
#pragma unroll
        for (int kx = 0; kx < 3; ++kx) {
            const int ix = ox * 2 - 1 + kx;
            if (ix < 0 || ix >= W) continue;
            const uint4 q = x[((n * H + iy) * W + ix) * xp16 + ch];
            float f[16];
            decode4(q.x, f); decode4(q.y, f + 4); decode4(q.z, f + 8); decode4(q.w, f + 12);
#pragma unroll
            for (int e = 0; e < 16; ++e) m[e] = f[e] > m[e] ? f[e] : m[e];
        }
    }
    y[((n * Ho + oy) * (long)Wo + ox) * yp16 + ch] = pack16_f8(m);   // (a decoded e4m3 value converts back exactly)
}

constexpr int AVG_PIX_LANES = 16;   // pixel slices per block of 16 channel chunks
__global__ __launch_bounds__(256) void avgpool_f8_partial_kernel(const uint4* __restrict__ x, float* __restrict__ part,
                                                                 long HW, int c16n, int xp16, int S) {
    // block: 16 chunks x 16 pixel lanes; grid (chunk groups, S pixel splits, N); part [N][S][c16n * 16]
    __shared__ float red[AVG_PIX_LANES][16][17];
    const int cl = threadIdx.x & 15, pl = threadIdx.x >> 4;
    const int ch = blockIdx.x * 16 + cl, s = blockIdx.y;
    const long n = blockIdx.z;
    const long per = (HW + S - 1) / S, lo = s * per, hi = (lo + per < HW) ? lo + per : HW;
    float a[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = 0.f;
    if (ch < c16n)
        for (long q = lo + pl; q < hi; q += AVG_PIX_LANES) {
            const uint4 v = x[(n * HW + q) * xp16 + ch];
            float f[16];
            decode4(v.x, f); decode4(v.y, f + 4); decode4(v.z, f + 8); decode4(v.w, f + 12);
#pragma unroll
            for (int e = 0; e < 16; ++e) a[e] += f[e];
        }
#pragma unroll
    for (int e = 0; e < 16; ++e) red[pl][cl][e] = a[e];
    __syncthreads();
    // thread (cl, e = pl) adds the 16 pixel lanes of channel 16 ch + e in ascending order
    if (ch < c16n) {
        float t = 0.f;
#pragma unroll
        for (int q = 0; q < AVG_PIX_LANES; ++q) t += red[q][cl][pl];
        part[((n * S + s) * c16n + ch) * 16 + pl] = t;
    }
}

__global__ __launch_bounds__(256) void avgpool_f8_final_kernel(const float* __restrict__ part, _Float16* __restrict__ y,
                                                               int C16, int S, int y_pitch, float inv, float scale,
                                                               long total) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int ch = (int)(idx % C16);
    const long n = idx / C16;
    float t = 0.f;
    for (int s = 0; s < S; ++s) t += part[(n * S + s) * C16 + ch];
    y[n * y_pitch + ch] = (_Float16)(t * inv * scale);
}

unsigned blocks_of(long total) { return (unsigned)((total + 255) / 256); }

}  // namespace

extern "C" {

int dcfp_conv2d_fwd_f8_nhwc(const DcfpConvF8Desc* d, const void* x, const void* w_packed, const float* mul,
                            const float* add, const void* residual, void* y, dcfp_stream_t stream) {
    const int st = check_desc(d, false);
    if (st != DCFP_OK) return st;
    if (!x || !w_packed || !mul || !add || !y) return DCFP_E_BADDESC;
    if (!dcfp_aligned16(x) || !dcfp_aligned16(w_packed) || !dcfp_aligned16(mul) || !dcfp_aligned16(add) ||
        !dcfp_aligned16(y) || !dcfp_aligned16(residual))
        return DCFP_E_BADDESC;
    if (residual && (!mult16(d->res_pitch) || d->res_off < 0 || (d->res_off & 15) ||
                     d->res_off + r16(d->Cout) > d->res_pitch))
        return DCFP_E_BADDESC;
    ConvF8Params p = make_params(d, x, w_packed, mul, add);
    p.res = reinterpret_cast<const unsigned char*>(residual);
    p.y = y;
    p.y_pitch = d->y_pitch; p.y_off = d->y_off; p.res_pitch = d->res_pitch; p.res_off = d->res_off;
    p.relu = d->relu != 0;
    p.res_mul = d->res_mul;
    return launch_conv<false>(d, p, dcfp_s(stream));
}

int dcfp_conv2d_fwd_f8_nhwc_to_f32_nchw(const DcfpConvF8Desc* d, const void* x, const void* w_packed, const float* mul,
                                        const float* add, float* y, dcfp_stream_t stream) {
    const int st = check_desc(d, true);
    if (st != DCFP_OK) return st;
    if (!x || !w_packed || !mul || !add || !y) return DCFP_E_BADDESC;
    if (!dcfp_aligned16(x) || !dcfp_aligned16(w_packed) || !dcfp_aligned16(mul) || !dcfp_aligned16(add))
        return DCFP_E_BADDESC;
    ConvF8Params p = make_params(d, x, w_packed, mul, add);
    p.y = y;
    return launch_conv<true>(d, p, dcfp_s(stream));
}

int dcfp_cast_nhwc_f16_to_f8(const void* x, int x_pitch, void* y, int y_pitch, int y_off, int64_t P, int C,
                             float scale, dcfp_stream_t stream) {
    if (!x || !y || P <= 0 || C <= 0 || !mult8(x_pitch) || x_pitch < (C + 7) / 8 * 8 || !mult16(y_pitch) || y_off < 0 ||
        (y_off & 15) || y_off + r16(C) > y_pitch || !dcfp_aligned16(x) || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    const int c16n = r16(C) / 16;
    const long total = (long)P * c16n;
    if (P >= (1ll << 31) || total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(cast_nhwc_f16_to_f8_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const h8_t*>(x), x_pitch / 8, reinterpret_cast<uint4*>(y), y_pitch / 16,
                       y_off / 16, C, c16n, scale, total);
    DCFP_RETURN_LAUNCH();
}

int dcfp_maxpool3x3s2_nhwc_f8(const void* x, void* y, int N, int H, int W, int C16, int x_pitch, int Ho, int Wo,
                              int y_pitch, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || H <= 0 || W <= 0 || !mult16(C16) || !mult16(x_pitch) || !mult16(y_pitch) ||
        x_pitch < C16 || y_pitch < C16 || !dcfp_aligned16(x) || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    if (Ho != (H - 1) / 2 + 1 || Wo != (W - 1) / 2 + 1) return DCFP_E_BADDESC;
    const long total = (long)N * Ho * Wo * (C16 / 16);
    if (total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(maxpool_nhwc_f8_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const uint4*>(x), reinterpret_cast<uint4*>(y), total, H, W, C16 / 16,
                       x_pitch / 16, Ho, Wo, y_pitch / 16);
    DCFP_RETURN_LAUNCH();
}

int dcfp_avgpool_nhwc_f8_to_f16(const void* x, void* y, int N, int64_t HW, int C16, int x_pitch, int y_pitch,
                                float scale, void* workspace, size_t workspace_bytes, dcfp_stream_t stream) {
    if (!x || !y || N <= 0 || N > 65535 || HW <= 0 || !mult16(C16) || !mult16(x_pitch) || x_pitch < C16 ||
        y_pitch < C16 || !dcfp_aligned16(x))
        return DCFP_E_BADDESC;
    // the workspace protocol of the fp16 pool: [N][S][C16] fp32 partial sums
    const size_t need = dcfp_avgpool_nhwc_f16_workspace_bytes(N, C16, HW);
    if (!workspace || need == 0 || workspace_bytes < need) return DCFP_E_WORKSPACE;
    const int S = (int)(need / ((size_t)N * C16 * sizeof(float))), c16n = C16 / 16;
    if (S < 1 || S > 65535) return DCFP_E_UNSUPPORTED;
    float* part = reinterpret_cast<float*>(workspace);
    hipLaunchKernelGGL(avgpool_f8_partial_kernel, dim3((c16n + 15) / 16, S, N), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const uint4*>(x), part, (long)HW, c16n, x_pitch / 16, S);
    const long total = (long)N * C16;
    hipLaunchKernelGGL(avgpool_f8_final_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream), part,
                       reinterpret_cast<_Float16*>(y), C16, S, y_pitch, 1.0f / (float)HW, scale, total);
    DCFP_RETURN_LAUNCH();
}

int dcfp_broadcast_nhwc_f16_to_f8(const void* v, int v_pitch, void* y, int N, int64_t HW, int C, int y_pitch,
                                  int y_off, float scale, dcfp_stream_t stream) {
    if (!v || !y || N <= 0 || HW <= 0 || C <= 0 || !mult8(v_pitch) || v_pitch < (C + 7) / 8 * 8 || !mult16(y_pitch) ||
        y_off < 0 || (y_off & 15) || y_off + r16(C) > y_pitch || !dcfp_aligned16(v) || !dcfp_aligned16(y))
        return DCFP_E_BADDESC;
    const int c16n = r16(C) / 16;
    const long total = (long)N * HW * c16n;
    if ((int64_t)N * HW >= (1ll << 31) || total >= (1l << 31) * 256) return DCFP_E_UNSUPPORTED;
    hipLaunchKernelGGL(broadcast_nhwc_f16_to_f8_kernel, dim3(blocks_of(total)), dim3(256), 0, dcfp_s(stream),
                       reinterpret_cast<const h8_t*>(v), v_pitch / 8, reinterpret_cast<uint4*>(y), (long)HW,
                       y_pitch / 16, y_off / 16, C, c16n, scale, total);
    DCFP_RETURN_LAUNCH();
}

}  // extern "C"
