// kd.hip — knowledge-distillation losses between the low-resolution logits of a student and a frozen teacher
// (DESIGN §16).  s, t: fp32 NCHW [N,C,h,w], contiguous; T > 0 the temperature; x' = x / T.
//
//   pixel   (Hinton et al.; the pixel-wise term of Liu et al., structured KD for segmentation): KL over the classes at
//           every pixel,   L = T^2/(N h w) * sum_pix KL(p_t || p_s),   dL/ds = T/(N h w) * (p_s - p_t)
//   channel (CWD, Shu et al. 2021): every (n, c) plane is a distribution over its h*w positions,
//                          L = T^2/(N C)   * sum_rows KL(q_t || q_s),  dL/ds = T/(N C)   * (q_s - q_t)
//
// One launch computes the per-block (pixel: per 64 pixels; channel: per row) sums of KL and, when a dlogits
// pointer is given, the gradient; a one-block kernel then adds the partials in fp64 in a fixed order.  No atomics: two
// calls leave the same bits.  Per distribution
//   KL = A / Z_t + ((M_s - M_t) + (log Z_s - log Z_t)),   A = sum e^(t' - M_t) (t' - s'),  Z_x = sum e^(x' - M_x),
// with M_x the maximum of x' (every exponent is <= 0).  Written this way a one-element distribution and t == s give
// exactly 0: A and M_s - M_t cancel bit for bit, and the gradient is the difference of two identically rounded terms
// (fp contraction is off in this file so that no product is fused into that difference).
//
// Layout.  pixel: a lane owns a pixel and walks classes at stride h*w, so a wave reads 256 contiguous bytes per class.
// A block is 64 pixels x K waves; wave y takes the classes y, y + K, ... of its 64 pixels, and the K partial softmax
// states of a pixel are combined through LDS in the order of the waves.  Up to K*R classes (32 with K = 4, 192 with
// K = 8: every dataset's count) a wave keeps its classes in registers, so s and t are read once and dlogits is written
// once; beyond that a wave runs an online softmax over its classes and reads them a second time for the gradient.
// channel: a 1024-thread workgroup owns a row of h*w contiguous floats; rows are too long for LDS next to the
// teacher's (129 x 257 floats = 130 KB each), so the block makes an online pass over the row and a second pass for the
// gradient that finds the row in L2 / Infinity Cache.
//
// Exponentials are the hardware's exp2 of x * log2(e) (__expf): every argument is <= 0, and its error, relative
// |x| * 2^-24, weighs on a term of size e^x - 1e-7 of the sum at worst.  The two logarithms per distribution are logf.
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kPixLanes = 64;          // pixels of a block: one wave wide
constexpr int kPixSmallK = 4, kPixSmallR = 8;      // C <= 32:  4 waves x 8 classes in registers
constexpr int kPixLargeK = 8, kPixLargeR = 24;     // C <= 192: 8 waves x 24 classes in registers; above: 8 waves, online
constexpr int kRowThreads = 1024;
constexpr int kRowWaves = kRowThreads / 64;

// online softmax step: (m, z) = running maximum and sum of e^(x - m); m = -inf, z = 0 at the start (0 * e^-inf = 0)
__device__ __forceinline__ void online_step(float x, float& m, float& z) {
    const float mn = fmaxf(m, x);
    z = z * __expf(m - mn) + __expf(x - mn);
    m = mn;
}

// the teacher's step carries A = sum e^(t' - m) (t' - s') along
__device__ __forceinline__ void online_step_a(float x, float d, float& m, float& z, float& a) {
    const float mn = fmaxf(m, x);
    const float r = __expf(m - mn), e = __expf(x - mn);
    z = z * r + e;
    a = a * r + e * d;
    m = mn;
}

__device__ __forceinline__ float kl_of(float ms, float zs, float mt, float zt, float a) {
    return a / zt + ((ms - mt) + (logf(zs) - logf(zt)));
}

// ---------------------------------------------------------------------------------------------- pixel mode
// blockDim = (64, K).  CACHED: wave y holds its classes y + r*K, r < R, in registers (the host guarantees C <= K*R).
template <int K, int R, bool CACHED>
__global__ void __launch_bounds__(kPixLanes * K)
kd_pixel_kernel(const float* __restrict__ s, const float* __restrict__ t, long long npix, int C, long long hw,
                float invT, float gscale, float* __restrict__ part, float* __restrict__ dl) {
    __shared__ float sm[5][K][kPixLanes];
    const int lane = threadIdx.x, y = threadIdx.y;
    const long long pix = (long long)blockIdx.x * kPixLanes + lane;
    const bool valid = pix < npix;
    long long base = 0;
    float ms = -INFINITY, mt = -INFINITY, zs = 0.f, zt = 0.f, a = 0.f;
    float vs[R], vt[R];
    if (valid) {
        const long long n = pix / hw;
        base = n * C * hw + (pix - n * hw);
        if (CACHED) {
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int c = y + r * K;
                if (c < C) {
                    vs[r] = s[base + c * hw] * invT;
                    vt[r] = t[base + c * hw] * invT;
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (y + r * K < C) {
                    ms = fmaxf(ms, vs[r]);
                    mt = fmaxf(mt, vt[r]);
                }
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                if (y + r * K < C) {
                    const float d = vt[r] - vs[r];
                    const float es = __expf(vs[r] - ms), et = __expf(vt[r] - mt);
                    zs += es;
                    zt += et;
                    a += et * d;
                    vs[r] = es;
                    vt[r] = et;
                }
            }
        } else {
#pragma unroll 4
            for (int c = y; c < C; c += K) {
                const float xs = s[base + c * hw] * invT, xt = t[base + c * hw] * invT;
                online_step(xs, ms, zs);
                online_step_a(xt, xt - xs, mt, zt, a);
            }
        }
    }
    sm[0][y][lane] = ms; sm[1][y][lane] = zs; sm[2][y][lane] = mt; sm[3][y][lane] = zt; sm[4][y][lane] = a;
    __syncthreads();
    // the pixel's state from its K slices, in the order of the waves (a wave without classes holds m = -inf, z = 0)
    float Ms = -INFINITY, Mt = -INFINITY;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        Ms = fmaxf(Ms, sm[0][k][lane]);
        Mt = fmaxf(Mt, sm[2][k][lane]);
    }
    float Zs = 0.f, Zt = 0.f, A = 0.f;
#pragma unroll
    for (int k = 0; k < K; ++k) {
        const float ft = __expf(sm[2][k][lane] - Mt);
        Zs += sm[1][k][lane] * __expf(sm[0][k][lane] - Ms);
        Zt += sm[3][k][lane] * ft;
        A += sm[4][k][lane] * ft;
    }
    if (y == 0) {
        const float kl = wave_sum(valid ? kl_of(Ms, Zs, Mt, Zt, A) : 0.f);
        if (lane == 0) part[blockIdx.x] = kl;
    }
    if (dl && valid) {
        if (CACHED) {
            const float fs = __expf(ms - Ms) * (1.0f / Zs), ft = __expf(mt - Mt) * (1.0f / Zt);
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const int c = y + r * K;
                if (c < C) {
                    const float ps = vs[r] * fs, pt = vt[r] * ft;
                    dl[base + c * hw] = (ps - pt) * gscale;
                }
            }
        } else {
            const float rs = 1.0f / Zs, rt = 1.0f / Zt;
#pragma unroll 4
            for (int c = y; c < C; c += K) {
                const float xs = s[base + c * hw] * invT, xt = t[base + c * hw] * invT;
                const float ps = __expf(xs - Ms) * rs, pt = __expf(xt - Mt) * rt;
                dl[base + c * hw] = (ps - pt) * gscale;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------- channel mode
// Block-wide maximum / sum over kRowThreads threads in a fixed order; every thread gets the result.
__device__ __forceinline__ float row_block_max(float v, float* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off, 64));
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
#pragma unroll
    for (int k = 1; k < kRowWaves; ++k) r = fmaxf(r, sm[k]);
    __syncthreads();
    return r;
}

__device__ __forceinline__ float row_block_sum(float v, float* sm) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
#pragma unroll
    for (int k = 1; k < kRowWaves; ++k) r += sm[k];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kRowThreads)
kd_channel_kernel(const float* __restrict__ s, const float* __restrict__ t, long long L, float invT, float gscale,
                  float* __restrict__ part, float* __restrict__ dl) {
    __shared__ float sm[kRowWaves];
    const long long base = (long long)blockIdx.x * L;
    const float* __restrict__ sr = s + base;
    const float* __restrict__ tr = t + base;
    float ms = -INFINITY, mt = -INFINITY, zs = 0.f, zt = 0.f, a = 0.f;
#pragma unroll 4
    for (long long i = threadIdx.x; i < L; i += kRowThreads) {
        const float xs = sr[i] * invT, xt = tr[i] * invT;
        online_step(xs, ms, zs);
        online_step_a(xt, xt - xs, mt, zt, a);
    }
    // the threads' (m, z, a) to the row's: rescale to the row maximum (a thread without elements has m = -inf, z = 0)
    const float Ms = row_block_max(ms, sm), Mt = row_block_max(mt, sm);
    const float fs = __expf(ms - Ms), ft = __expf(mt - Mt);
    const float Zs = row_block_sum(zs * fs, sm);
    const float Zt = row_block_sum(zt * ft, sm);
    const float A = row_block_sum(a * ft, sm);
    if (threadIdx.x == 0) part[blockIdx.x] = kl_of(Ms, Zs, Mt, Zt, A);
    if (dl) {
        float* __restrict__ dr = dl + base;
        const float rs = 1.0f / Zs, rt = 1.0f / Zt;
#pragma unroll 4
        for (long long i = threadIdx.x; i < L; i += kRowThreads) {
            const float xs = sr[i] * invT, xt = tr[i] * invT;
            const float qs = __expf(xs - Ms) * rs, qt = __expf(xt - Mt) * rt;
            dr[i] = (qs - qt) * gscale;
        }
    }
}

// One 256-thread block: thread k adds the partials k, k + 256, ... in fp64, then a fixed-order tree over the 256 sums.
__global__ void __launch_bounds__(256)
kd_final_kernel(const float* __restrict__ part, long long n, double scale, float* __restrict__ out) {
    __shared__ double sa[256];
    double acc = 0.0;
    for (long long k = threadIdx.x; k < n; k += 256) acc += (double)part[k];
    sa[threadIdx.x] = acc;
    __syncthreads();
    for (int st = 128; st > 0; st >>= 1) {
        if ((int)threadIdx.x < st) sa[threadIdx.x] += sa[threadIdx.x + st];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(sa[0] * scale);
}

// number of loss partials (= blocks of the forward launch); 0 for arguments the entry points refuse
long long kd_partials(int mode, int N, int C, int h, int w) {
    if (N < 1 || C < 1 || h < 1 || w < 1) return 0;
    if (mode == DCFP_KD_PIXEL) return ((long long)N * h * w + kPixLanes - 1) / kPixLanes;
    if (mode == DCFP_KD_CHANNEL) return (long long)N * C;
    return 0;
}

}  // namespace

extern "C" size_t dcfp_kd_workspace_bytes(int mode, int N, int C, int h, int w) {
    return (size_t)kd_partials(mode, N, C, h, w) * sizeof(float);
}

extern "C" int dcfp_kd_fwd_f32(const float* s, const float* t, int mode, int N, int C, int h, int w, float T,
                               void* workspace, size_t workspace_bytes, float* loss_out, float* dlogits,
                               dcfp_stream_t stream) {
    if (!s || !t || !loss_out || N < 1 || C < 1 || h < 1 || w < 1) return DCFP_E_BADDESC;
    if (!(T > 0.0f) || !isfinite(T)) return DCFP_E_BADDESC;
    if (mode != DCFP_KD_PIXEL && mode != DCFP_KD_CHANNEL) return DCFP_E_BADDESC;
    const long long blocks = kd_partials(mode, N, C, h, w);
    if (blocks > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < (size_t)blocks * sizeof(float)) return DCFP_E_WORKSPACE;
    float* part = static_cast<float*>(workspace);
    const long long hw = (long long)h * w;
    const double dT = (double)T;
    const float invT = (float)(1.0 / dT);
    hipStream_t st = dcfp_s(stream);
    double count;
    if (mode == DCFP_KD_PIXEL) {
        const long long npix = (long long)N * hw;
        count = (double)npix;
        const float gscale = (float)(dT / count);
        const dim3 grid((unsigned)blocks);
        if (C <= kPixSmallK * kPixSmallR)
            hipLaunchKernelGGL((kd_pixel_kernel<kPixSmallK, kPixSmallR, true>), grid, dim3(kPixLanes, kPixSmallK), 0, st, s,
                               t, npix, C, hw, invT, gscale, part, dlogits);
        else if (C <= kPixLargeK * kPixLargeR)
            hipLaunchKernelGGL((kd_pixel_kernel<kPixLargeK, kPixLargeR, true>), grid, dim3(kPixLanes, kPixLargeK), 0, st, s,
                               t, npix, C, hw, invT, gscale, part, dlogits);
        else
            hipLaunchKernelGGL((kd_pixel_kernel<kPixLargeK, 1, false>), grid, dim3(kPixLanes, kPixLargeK), 0, st, s, t,
                               npix, C, hw, invT, gscale, part, dlogits);
    } else {
        count = (double)N * C;
        const float gscale = (float)(dT / count);
        hipLaunchKernelGGL(kd_channel_kernel, dim3((unsigned)blocks), dim3(kRowThreads), 0, st, s, t, hw, invT, gscale,
                           part, dlogits);
    }
    hipLaunchKernelGGL(kd_final_kernel, dim3(1), dim3(256), 0, st, part, blocks, dT * dT / count, loss_out);
    DCFP_RETURN_LAUNCH();
}
