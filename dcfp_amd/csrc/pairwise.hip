// pairwise.hip — pair-wise similarity distillation between a feature map of the student and of a frozen teacher
// (the second term of Liu et al., structured KD for segmentation).
//
//   nodes     u_p[c]  = mean of the in-range elements of the b x b window p of channel c   (avg_pool2d, ceil_mode,
//                       count_include_pad = False);  P = ceil(h/b) * ceil(w/b) nodes per image
//   scale     s_p     = 1 / r_p,  r_p^2 = sum_c u_p[c]^2,  and s_p = 0 where r_p^2 <= 1e-12 (a dead node);  f_p = u_p s_p
//   loss      A^x_pq  = f^x_p . f^x_q,  D = A^S - A^T,  L = 1/(N P^2) * sum_n sum_pq D_pq^2
//   gradient  g_p     = 4/(N P^2) * sum_q D_pq f^S_q,   du_p = (g_p - f_p (f_p . g_p)) s_p,
//             dS[n,c,y,x] = du_{p(y,x)}[c] / |window_p|
//
// Workspace images (all fp32, zero-padded so that no matrix kernel checks a bound):
//   U  [N][Cpad][Ppad]   node matrix, CHANNEL-major: row c holds channel c of every node; Cpad = C rounded up to 32 (the
//                        K loop's block), Ppad = P rounded up to 128 (the block tile); rows >= C and columns >= P are 0
//   s  [N][Ppad]         the scales, 0 for columns >= P
//   D  [N][Ppad][Ppad]   only when a gradient is wanted;  GT [N][CsPad][Ppad] = (D F^S)^T;  dot [N][Ppad] = f_p . g_p
// The forward call (dcfp_pairwise_fwd_f32) leaves US, sS and D in the workspace; the backward call
// (dcfp_pairwise_bwd_f32) on the same workspace makes GT, the dot and dS, scaled by autograd's grad_output in its last
// multiplication - so the caller keeps one workspace per graph and no gradient tensor waits from forward to backward.
//
// Kernels.  pa_nodes_nchw / pa_nodes_nhwc read a feature map once (fp32 NCHW; fp16 NHWC with a pixel pitch, only the C
// channels of the slice are read) and write U and, per chunk of 64 channels, a share of r^2 that pa_reduce_kernel adds
// up in order and turns into s.  pa_gram_kernel: one 256-thread block per image and pair of
// 128-node tiles (ti <= tj) runs the two K loops - over the student's and the teacher's channels - on
// v_mfma_f32_32x32x2_f32 into two sets of accumulators, scales them in the epilogue (A_pq = (u_p . u_q)(s_p s_q)), forms
// the D tile, writes it and (ti != tj) its mirror, and one partial sum of D^2 per block, counted twice off the diagonal.
// A^S and A^T never reach memory and the lower triangle is never computed.  pa_final_kernel adds the partials in fp64
// in a fixed order.  pa_grad_gemm_kernel is GT = F^S^T D on the same MFMA (D is symmetric bit for bit, so its rows serve
// as the k-major operand), pa_dot_kernel (+ pa_reduce_kernel) the dot over channels, pa_scatter_kernel du and the un-pooled dS: every
// element of dS is written exactly once.  No atomics anywhere: two calls leave the same bits.
//
// Student and teacher being the same tensor give exactly 0: both Grams run the same instruction sequence over the same
// values, and fp contraction is off in this file so that neither product of the difference is fused into it.
#include <hip/hip_fp16.h>
#include <math.h>

#include "common.h"

#pragma clang fp contract(off)

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kTile = 128;             // nodes per side of a block tile (2 x 2 waves of 64 x 64, each 2 x 2 MFMA tiles)
constexpr int kBK = 32;                // k rows staged per step: 16 MFMAs of k = 2
constexpr int kNodeLanes = 64;         // nodes of a pa_nodes_nchw / pa_dot block: one wave wide
constexpr int kNodeWaves = 8;          // ... and the waves that share their channels
constexpr int kHwcNodes = 32;          // nodes of a pa_nodes_nhwc block
constexpr int kChunk = 64;             // channels of a node / dot block: its partial sums are added by pa_reduce_kernel
constexpr float kDead = 1e-12f;        // r^2 at or below this: a dead node

__host__ __device__ inline long long round_up(long long v, long long m) { return (v + m - 1) / m * m; }

__device__ __forceinline__ float scale_of(float r2) { return r2 > kDead ? 1.0f / sqrtf(r2) : 0.0f; }

struct PaGeom {
    int C, h, w, b, wp, P;             // wp = ceil(w / b)
    int Cpad, Ppad;
};

// window p of an h x w map: [y0, y1) x [x0, x1) and 1 / its in-range size
__device__ __forceinline__ void window_of(const PaGeom& g, int p, int& y0, int& y1, int& x0, int& x1, float& inv) {
    const int i = p / g.wp, j = p - i * g.wp;
    y0 = i * g.b; x0 = j * g.b;
    y1 = min(g.h, y0 + g.b); x1 = min(g.w, x0 + g.b);
    inv = 1.0f / (float)((y1 - y0) * (x1 - x0));
}

// ------------------------------------------------------------------------------------------ nodes, fp32 NCHW
// grid (Ppad / 64, Cpad / 64 rounded up, N), block (64, 8): a lane owns a node, the block a chunk of 64 channels, wave y
// the channels y, y + 8, ... of the chunk.  The chunk's share of r^2 goes to rpart[n][chunk][p]; pa_reduce_kernel adds
// the chunks in their order.
__global__ void __launch_bounds__(kNodeLanes * kNodeWaves)
pa_nodes_nchw_kernel(const float* __restrict__ x, PaGeom g, float* __restrict__ U, float* __restrict__ rpart) {
    __shared__ float sm[kNodeWaves][kNodeLanes];
    const int lane = threadIdx.x, y = threadIdx.y, n = blockIdx.z;
    const int p = blockIdx.x * kNodeLanes + lane;
    const bool valid = p < g.P;
    int y0 = 0, y1 = 0, x0 = 0, x1 = 0;
    float inv = 0.f;
    if (valid) window_of(g, p, y0, y1, x0, x1, inv);
    const long long plane = (long long)g.h * g.w;
    const float* __restrict__ xn = x + (long long)n * g.C * plane;
    float* __restrict__ Un = U + (long long)n * g.Cpad * g.Ppad + p;
    const int cend = min(g.Cpad, ((int)blockIdx.y + 1) * kChunk);
    float sq = 0.f;
    for (int c = blockIdx.y * kChunk + y; c < cend; c += kNodeWaves) {
        float u = 0.f;
        if (valid && c < g.C) {
            const float* __restrict__ xc = xn + c * plane;
            float acc = 0.f;
            for (int yy = y0; yy < y1; ++yy)
                for (int xx = x0; xx < x1; ++xx) acc += xc[(long long)yy * g.w + xx];
            u = acc * inv;
            sq += u * u;
        }
        Un[(long long)c * g.Ppad] = u;
    }
    sm[y][lane] = sq;
    __syncthreads();
    if (y == 0) {
        float r2 = 0.f;
#pragma unroll
        for (int k = 0; k < kNodeWaves; ++k) r2 += sm[k][lane];
        rpart[((long long)n * gridDim.y + blockIdx.y) * g.Ppad + p] = r2;
    }
}

// ------------------------------------------------------------------------------------------ nodes, fp16 NHWC
// grid (Ppad / 32, Cpad / 64 rounded up, N), block 256: wave v owns the nodes 8v .. 8v + 7 of the block's 32, a lane a
// channel of the block's chunk of 64; the 64 x 32 tile goes through LDS so that U's rows are written 128 bytes at a time
__global__ void __launch_bounds__(256)
pa_nodes_nhwc_kernel(const __half* __restrict__ x, long long pitch, PaGeom g, float* __restrict__ U,
                     float* __restrict__ rpart) {
    __shared__ float tile[kChunk][kHwcNodes + 1];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, n = blockIdx.z;
    const int p0 = blockIdx.x * kHwcNodes, c0 = blockIdx.y * kChunk;
    constexpr int kPer = kHwcNodes / 4;
    const __half* __restrict__ xn = x + (long long)n * g.h * g.w * pitch;
    float* __restrict__ Un = U + (long long)n * g.Cpad * g.Ppad;
    float* __restrict__ rp = rpart + ((long long)n * gridDim.y + blockIdx.y) * g.Ppad;
    const int c = c0 + lane;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int p = p0 + wv * kPer + j;
        float u = 0.f;
        if (p < g.P && c < g.C) {
            int y0, y1, x0, x1;
            float inv;
            window_of(g, p, y0, y1, x0, x1, inv);
            float acc = 0.f;
            for (int yy = y0; yy < y1; ++yy)
                for (int xx = x0; xx < x1; ++xx) acc += __half2float(xn[((long long)yy * g.w + xx) * pitch + c]);
            u = acc * inv;
        }
        tile[lane][wv * kPer + j] = u;
        const float r2 = wave_sum(u * u);
        if (lane == 0) rp[p] = r2;
    }
    __syncthreads();
    const int node = threadIdx.x & 31;
#pragma unroll
    for (int i = 0; i < kChunk / 8; ++i) {
        const int row = (threadIdx.x >> 5) + 8 * i;
        if (c0 + row < g.Cpad) Un[(long long)(c0 + row) * g.Ppad + p0 + node] = tile[row][node];
    }
}

// out[n][p] = sum over the Z chunk partials part[n][z][p], z in order; SCALE: the node's scale of that r^2
template <bool SCALE>
__global__ void __launch_bounds__(256)
pa_reduce_kernel(const float* __restrict__ part, int Z, int Ppad, float* __restrict__ out) {
    const int p = blockIdx.x * 256 + threadIdx.x, n = blockIdx.y;
    if (p >= Ppad) return;
    const float* __restrict__ src = part + (long long)n * Z * Ppad + p;
    float acc = 0.f;
    for (int z = 0; z < Z; ++z) acc += src[(long long)z * Ppad];
    out[(long long)n * Ppad + p] = SCALE ? scale_of(acc) : acc;
}

// ------------------------------------------------------------------------------------------ MFMA tiles
// a 32 x 128 row-major image (k rows, 128 columns) from global rows of pitch ld: 4 float4 per thread
struct RowTile {
    float4 v[4];
    __device__ __forceinline__ void load(const float* __restrict__ src, long long ld) {
        const int t = threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            v[j] = *reinterpret_cast<const float4*>(src + (long long)((t >> 5) + 8 * j) * ld + (t & 31) * 4);
    }
    __device__ __forceinline__ void store(float* lds) const {
        const int t = threadIdx.x;
#pragma unroll
        for (int j = 0; j < 4; ++j) *reinterpret_cast<float4*>(lds + ((t >> 5) + 8 * j) * kTile + (t & 31) * 4) = v[j];
    }
};

// acc[m][n] += A^T B over one staged step: As, Bs are [kBK][128] k-major images, the wave's 64 x 64 corner at (am, bn)
__device__ __forceinline__ void mfma_step_kk(const float* As, const float* Bs, int am, int bn, f32x16 (&acc)[2][2]) {
    const int lane = threadIdx.x & 63, r = lane & 31, kh = lane >> 5;
#pragma unroll
    for (int kk = 0; kk < kBK / 2; ++kk) {
        const int k = 2 * kk + kh;
        const float a0 = As[k * kTile + am + r], a1 = As[k * kTile + am + 32 + r];
        const float b0 = Bs[k * kTile + bn + r], b1 = Bs[k * kTile + bn + 32 + r];
        acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
        acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
        acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
        acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
    }
}

// one Gram K loop: acc += U[:, rows]^T U[:, cols] over Cpad channels; the next step's tiles wait in registers
__device__ __forceinline__ void gram_loop(const float* __restrict__ Ua, const float* __restrict__ Ub, int Cpad,
                                          long long Ppad, float* As, float* Bs, int am, int bn, f32x16 (&acc)[2][2]) {
    RowTile ta, tb;
    ta.load(Ua, Ppad);
    tb.load(Ub, Ppad);
    for (int c0 = 0; c0 < Cpad; c0 += kBK) {
        __syncthreads();                           // (the previous step's reads of As / Bs are done)
        ta.store(As);
        tb.store(Bs);
        __syncthreads();
        if (c0 + kBK < Cpad) {
            ta.load(Ua + (long long)(c0 + kBK) * Ppad, Ppad);
            tb.load(Ub + (long long)(c0 + kBK) * Ppad, Ppad);
        }
        mfma_step_kk(As, Bs, am, bn, acc);
    }
}

__device__ __forceinline__ void zero_acc(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < 2; ++n)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[m][n][r] = 0.f;
}

// grid (nt (nt + 1) / 2, N), block 256.  D may be null (loss only).
__global__ void __launch_bounds__(256)
pa_gram_kernel(const float* __restrict__ US, const float* __restrict__ sS, int CsPad, const float* __restrict__ UT,
               const float* __restrict__ sT, int CtPad, int Ppad, float* __restrict__ D, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float As[kBK * kTile];
    __shared__ __attribute__((aligned(16))) float Bs[kBK * kTile];
    __shared__ float red[4];
    const int nt = Ppad / kTile, n = blockIdx.y;
    int ti = 0, rem = blockIdx.x;
    while (rem >= nt - ti) { rem -= nt - ti; ++ti; }
    const int tj = ti + rem;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int am = (wave >> 1) * 64, bn = (wave & 1) * 64;
    const long long P = Ppad;
    f32x16 accS[2][2], accT[2][2];
    zero_acc(accS);
    zero_acc(accT);
    const float* __restrict__ USn = US + (long long)n * CsPad * P;
    const float* __restrict__ UTn = UT + (long long)n * CtPad * P;
    gram_loop(USn + ti * kTile, USn + tj * kTile, CsPad, P, As, Bs, am, bn, accS);
    gram_loop(UTn + ti * kTile, UTn + tj * kTile, CtPad, P, As, Bs, am, bn, accT);
    const float* __restrict__ sSn = sS + (long long)n * P;
    const float* __restrict__ sTn = sT + (long long)n * P;
    float* __restrict__ Dn = D ? D + (long long)n * P * P : nullptr;
    float sum = 0.f;
#pragma unroll
    for (int m = 0; m < 2; ++m) {
#pragma unroll
        for (int nn = 0; nn < 2; ++nn) {
            const int q = tj * kTile + bn + nn * 32 + (lane & 31);
            const float sq = sSn[q], tq = sTn[q];
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int pb = ti * kTile + am + m * 32 + 8 * g4 + 4 * (lane >> 5);
                float d[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int p = pb + e;
                    const float a_s = accS[m][nn][4 * g4 + e] * (sSn[p] * sq);
                    const float a_t = accT[m][nn][4 * g4 + e] * (sTn[p] * tq);
                    d[e] = a_s - a_t;
                    sum += d[e] * d[e];
                    if (Dn) Dn[(long long)p * P + q] = d[e];
                }
                if (Dn && ti != tj) *reinterpret_cast<float4*>(Dn + (long long)q * P + pb) = make_float4(d[0], d[1], d[2], d[3]);
            }
        }
    }
    const float tot = block_sum_256(sum, red);
    if (threadIdx.x == 0) part[(long long)n * gridDim.x + blockIdx.x] = ti == tj ? tot : 2.0f * tot;
}

// GT[n][c][p] = sum_q (U[c][q] s_q) D[q][p]:  grid (Ppad / 128, ceil(Cpad / 128), N), block 256
__global__ void __launch_bounds__(256)
pa_grad_gemm_kernel(const float* __restrict__ U, const float* __restrict__ sc, int Cpad, int Ppad,
                    const float* __restrict__ D, float* __restrict__ GT) {
    constexpr int kAP = kBK + 1;
    __shared__ float As[kTile * kAP];              // [c][k], pitch 33: a lane group reads 32 rows of one k
    __shared__ __attribute__((aligned(16))) float Bs[kBK * kTile];
    const int n = blockIdx.z, c0 = blockIdx.y * kTile, p0 = blockIdx.x * kTile;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, r = lane & 31, kh = lane >> 5;
    const int am = (wave >> 1) * 64, bn = (wave & 1) * 64;
    const long long P = Ppad;
    const float* __restrict__ Un = U + (long long)n * Cpad * P;
    const float* __restrict__ sn = sc + (long long)n * P;
    const float* __restrict__ Dn = D + (long long)n * P * P + p0;
    f32x16 acc[2][2];
    zero_acc(acc);
    float4 va[4];
    RowTile tb;
    const int arow = t >> 3, acol = (t & 7) * 4;
    auto load_a = [&](int q0) {
        const float4 s4 = *reinterpret_cast<const float4*>(sn + q0 + acol);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int c = c0 + arow + 32 * j;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (c < Cpad) v = *reinterpret_cast<const float4*>(Un + (long long)c * P + q0 + acol);
            va[j] = make_float4(v.x * s4.x, v.y * s4.y, v.z * s4.z, v.w * s4.w);
        }
    };
    load_a(0);
    tb.load(Dn, P);
    for (int q0 = 0; q0 < Ppad; q0 += kBK) {
        __syncthreads();
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float* dst = As + (arow + 32 * j) * kAP + acol;
            dst[0] = va[j].x; dst[1] = va[j].y; dst[2] = va[j].z; dst[3] = va[j].w;
        }
        tb.store(Bs);
        __syncthreads();
        if (q0 + kBK < Ppad) {
            load_a(q0 + kBK);
            tb.load(Dn + (long long)(q0 + kBK) * P, P);
        }
#pragma unroll
        for (int kk = 0; kk < kBK / 2; ++kk) {
            const int k = 2 * kk + kh;
            const float a0 = As[(am + r) * kAP + k], a1 = As[(am + 32 + r) * kAP + k];
            const float b0 = Bs[k * kTile + bn + r], b1 = Bs[k * kTile + bn + 32 + r];
            acc[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, acc[0][0], 0, 0, 0);
            acc[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, acc[0][1], 0, 0, 0);
            acc[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, acc[1][0], 0, 0, 0);
            acc[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, acc[1][1], 0, 0, 0);
        }
    }
    float* __restrict__ Gn = GT + (long long)n * Cpad * P;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int nn = 0; nn < 2; ++nn)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int c = c0 + am + m * 32 + (e & 3) + 8 * (e >> 2) + 4 * kh;
                if (c < Cpad) Gn[(long long)c * P + p0 + bn + nn * 32 + r] = acc[m][nn][e];
            }
}

// dpart[n][chunk][p] = sum over the chunk's channels of (U[c][p] s_p) (gs GT[c][p]):  grid (Ppad / 64, chunks, N),
// block (64, 8); pa_reduce_kernel adds the chunks
__global__ void __launch_bounds__(kNodeLanes * kNodeWaves)
pa_dot_kernel(const float* __restrict__ U, const float* __restrict__ sc, const float* __restrict__ GT, int Cpad,
              int Ppad, float gs, float* __restrict__ dpart) {
    __shared__ float sm[kNodeWaves][kNodeLanes];
    const int lane = threadIdx.x, y = threadIdx.y, n = blockIdx.z;
    const int p = blockIdx.x * kNodeLanes + lane;
    const long long base = (long long)n * Cpad * Ppad + p;
    const float s = sc[(long long)n * Ppad + p];
    const int cend = min(Cpad, ((int)blockIdx.y + 1) * kChunk);
    float acc = 0.f;
#pragma unroll 4
    for (int c = blockIdx.y * kChunk + y; c < cend; c += kNodeWaves) {
        const long long o = base + (long long)c * Ppad;
        acc += (U[o] * s) * (GT[o] * gs);
    }
    sm[y][lane] = acc;
    __syncthreads();
    if (y == 0) {
        float r = 0.f;
#pragma unroll
        for (int k = 0; k < kNodeWaves; ++k) r += sm[k][lane];
        dpart[((long long)n * gridDim.y + blockIdx.y) * Ppad + p] = r;
    }
}

// dS[n,c,y,x] = ((g - f (f . g)) s / |window|) * grad_output, f = U s, g = gs GT:  grid (N * C, ceil(h w / 256)),
// block 256.  gout: the device scalar autograd hands to backward (null: 1); it is the last factor, so a call with it is
// the call without it times that scalar, bit for bit.
__global__ void __launch_bounds__(256)
pa_scatter_kernel(const float* __restrict__ U, const float* __restrict__ sc, const float* __restrict__ GT,
                  const float* __restrict__ dot, PaGeom g, float gs, const float* __restrict__ gout,
                  float* __restrict__ dS) {
    const long long nc = blockIdx.x;
    const int n = (int)(nc / g.C), c = (int)(nc - (long long)n * g.C);
    const int i = blockIdx.y * 256 + threadIdx.x;
    if (i >= g.h * g.w) return;
    const int y = i / g.w, x = i - y * g.w;
    const int pi = y / g.b, pj = x / g.b, p = pi * g.wp + pj;
    const int cnt = (min(g.h, (pi + 1) * g.b) - pi * g.b) * (min(g.w, (pj + 1) * g.b) - pj * g.b);
    const long long o = ((long long)n * g.Cpad + c) * g.Ppad + p;
    const float s = sc[(long long)n * g.Ppad + p];
    const float f = U[o] * s, gg = GT[o] * gs;
    const float du = (gg - f * dot[(long long)n * g.Ppad + p]) * s;
    const float v = du * (1.0f / (float)cnt);
    dS[nc * g.h * g.w + i] = gout ? v * gout[0] : v;
}

// One 256-thread block: thread k adds the partials k, k + 256, ... in fp64, then a fixed-order tree over the 256 sums.
__global__ void __launch_bounds__(256)
pa_final_kernel(const float* __restrict__ part, long long n, double scale, float* __restrict__ out) {
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

// ------------------------------------------------------------------------------------------ host
// The workspace's segments, each 256-byte aligned; ok = false for arguments the entry points refuse.  The forward call
// fills US, sS, UT, sT (through the chunk partials cp) and part, and with a gradient wanted D; the backward call reads
// US, sS and D and needs GT, the dot's chunk partials and the dot.  By then the teacher's images are dead: the dot takes
// sT's place, its partials take cp's, and GT takes UT's where the teacher is at least as wide as the student.
struct PaPlan {
    bool ok = false, fits = false;
    PaGeom gs{}, gt{};
    long long pairs = 0;
    int zs = 0, zt = 0;                    // channel chunks of the student's and the teacher's node kernels
    size_t oUS = 0, oSS = 0, oUT = 0, oST = 0, oCp = 0, oPart = 0, oD = 0, oGT = 0, fwd_bytes = 0, all_bytes = 0;
};

PaPlan pa_plan(int N, int Cs, int Ct, int h, int w, int pool) {
    PaPlan pl;
    if (N < 1 || Cs < 1 || Ct < 1 || h < 1 || w < 1 || pool < 1) return pl;
    pl.ok = true;
    const long long hp = ((long long)h + pool - 1) / pool, wp = ((long long)w + pool - 1) / pool, P = hp * wp;
    const long long Ppad = round_up(P, kTile), nt = Ppad / kTile;
    pl.pairs = nt * (nt + 1) / 2;
    // grids: pairs, N * Cs and node blocks in x, chunks / row tiles / ceil(h w / 256) in y, N in y or z (all <= 65535
    // beyond x); element counts fit 63 bits
    pl.fits = Ppad <= 0x7fffffffLL && pl.pairs <= 0x7fffffffLL && N <= 65535 && (long long)N * Cs <= 0x7fffffffLL &&
              ((long long)h * w + 255) / 256 <= 65535 && (long long)h * w <= 0x7fffffffLL &&
              round_up(Cs, kChunk) / kChunk <= 65535 && round_up(Ct, kChunk) / kChunk <= 65535 &&
              (double)N * Ppad * Ppad * 4.0 < 9.0e18;
    if (!pl.fits) return pl;
    PaGeom g{};
    g.h = h; g.w = w; g.b = pool; g.wp = (int)wp; g.P = (int)P; g.Ppad = (int)Ppad;
    pl.gs = g; pl.gs.C = Cs; pl.gs.Cpad = (int)round_up(Cs, kBK);
    pl.gt = g; pl.gt.C = Ct; pl.gt.Cpad = (int)round_up(Ct, kBK);
    pl.zs = (pl.gs.Cpad + kChunk - 1) / kChunk;
    pl.zt = (pl.gt.Cpad + kChunk - 1) / kChunk;
    size_t off = 0;
    auto seg = [&](size_t floats) { const size_t o = off; off += (size_t)round_up((long long)floats * 4, 256); return o; };
    pl.oUS = seg((size_t)N * pl.gs.Cpad * Ppad);
    pl.oSS = seg((size_t)N * Ppad);
    pl.oUT = seg((size_t)N * pl.gt.Cpad * Ppad);
    pl.oST = seg((size_t)N * Ppad);
    pl.oCp = seg((size_t)N * (pl.zs > pl.zt ? pl.zs : pl.zt) * Ppad);
    pl.oPart = seg((size_t)N * pl.pairs);
    pl.fwd_bytes = off;
    pl.oD = seg((size_t)N * Ppad * Ppad);
    pl.oGT = pl.gt.Cpad >= pl.gs.Cpad ? pl.oUT : seg((size_t)N * pl.gs.Cpad * Ppad);
    pl.all_bytes = off;
    return pl;
}

int pa_check(const PaPlan& pl, const void* workspace, size_t workspace_bytes, bool grad) {
    if (!pl.ok) return DCFP_E_BADDESC;
    if (!pl.fits) return DCFP_E_UNSUPPORTED;
    if (!workspace || workspace_bytes < (grad ? pl.all_bytes : pl.fwd_bytes)) return DCFP_E_WORKSPACE;
    if ((reinterpret_cast<uintptr_t>(workspace) & 15u) != 0) return DCFP_E_WORKSPACE;
    return DCFP_OK;
}

inline float* pa_at(void* ws, size_t off) { return reinterpret_cast<float*>(static_cast<char*>(ws) + off); }

}  // namespace

extern "C" size_t dcfp_pairwise_workspace_bytes(int N, int Cs, int Ct, int h, int w, int pool, int with_grad) {
    const PaPlan pl = pa_plan(N, Cs, Ct, h, w, pool);
    if (!pl.ok || !pl.fits) return 0;
    return with_grad ? pl.all_bytes : pl.fwd_bytes;
}

extern "C" int dcfp_pairwise_fwd_f32(const float* s, const void* t, int t_layout, long long t_pitch, int N, int Cs,
                                     int Ct, int h, int w, int pool, void* workspace, size_t workspace_bytes,
                                     float* loss_out, int with_grad, dcfp_stream_t stream) {
    if (!s || !t || !loss_out) return DCFP_E_BADDESC;
    if (t_layout != DCFP_PA_F32_NCHW && t_layout != DCFP_PA_F16_NHWC) return DCFP_E_BADDESC;
    const PaPlan pl = pa_plan(N, Cs, Ct, h, w, pool);
    if (pl.ok && t_layout == DCFP_PA_F16_NHWC && t_pitch < Ct) return DCFP_E_BADDESC;
    if (const int rc = pa_check(pl, workspace, workspace_bytes, with_grad != 0)) return rc;
    float* US = pa_at(workspace, pl.oUS);
    float* sS = pa_at(workspace, pl.oSS);
    float* UT = pa_at(workspace, pl.oUT);
    float* sT = pa_at(workspace, pl.oST);
    float* cp = pa_at(workspace, pl.oCp);
    float* part = pa_at(workspace, pl.oPart);
    float* D = with_grad ? pa_at(workspace, pl.oD) : nullptr;
    hipStream_t st = dcfp_s(stream);
    const int Ppad = pl.gs.Ppad;
    const dim3 node_block(kNodeLanes, kNodeWaves), red_grid((Ppad + 255) / 256, N);
    hipLaunchKernelGGL(pa_nodes_nchw_kernel, dim3(Ppad / kNodeLanes, pl.zs, N), node_block, 0, st, s, pl.gs, US, cp);
    hipLaunchKernelGGL(pa_reduce_kernel<true>, red_grid, dim3(256), 0, st, cp, pl.zs, Ppad, sS);
    if (t_layout == DCFP_PA_F32_NCHW)
        hipLaunchKernelGGL(pa_nodes_nchw_kernel, dim3(Ppad / kNodeLanes, pl.zt, N), node_block, 0, st,
                           static_cast<const float*>(t), pl.gt, UT, cp);
    else
        hipLaunchKernelGGL(pa_nodes_nhwc_kernel, dim3(Ppad / kHwcNodes, pl.zt, N), dim3(256), 0, st,
                           static_cast<const __half*>(t), t_pitch, pl.gt, UT, cp);
    hipLaunchKernelGGL(pa_reduce_kernel<true>, red_grid, dim3(256), 0, st, cp, pl.zt, Ppad, sT);
    hipLaunchKernelGGL(pa_gram_kernel, dim3((unsigned)pl.pairs, N), dim3(256), 0, st, US, sS, pl.gs.Cpad, UT, sT,
                       pl.gt.Cpad, Ppad, D, part);
    const double count = (double)N * (double)pl.gs.P * (double)pl.gs.P;
    hipLaunchKernelGGL(pa_final_kernel, dim3(1), dim3(256), 0, st, part, (long long)N * pl.pairs, 1.0 / count, loss_out);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_pairwise_bwd_f32(int N, int Cs, int Ct, int h, int w, int pool, void* workspace,
                                     size_t workspace_bytes, const float* grad_out, float* dstudent,
                                     dcfp_stream_t stream) {
    if (!dstudent) return DCFP_E_BADDESC;
    const PaPlan pl = pa_plan(N, Cs, Ct, h, w, pool);
    if (const int rc = pa_check(pl, workspace, workspace_bytes, true)) return rc;
    float* US = pa_at(workspace, pl.oUS);
    float* sS = pa_at(workspace, pl.oSS);
    float* D = pa_at(workspace, pl.oD);
    float* GT = pa_at(workspace, pl.oGT);
    float* dpart = pa_at(workspace, pl.oCp);
    float* dot = pa_at(workspace, pl.oST);
    hipStream_t st = dcfp_s(stream);
    const int Ppad = pl.gs.Ppad;
    const double count = (double)N * (double)pl.gs.P * (double)pl.gs.P;
    const float gscale = (float)(4.0 / count);
    hipLaunchKernelGGL(pa_grad_gemm_kernel, dim3(Ppad / kTile, (pl.gs.Cpad + kTile - 1) / kTile, N), dim3(256), 0, st, US,
                       sS, pl.gs.Cpad, Ppad, D, GT);
    hipLaunchKernelGGL(pa_dot_kernel, dim3(Ppad / kNodeLanes, pl.zs, N), dim3(kNodeLanes, kNodeWaves), 0, st, US, sS, GT,
                       pl.gs.Cpad, Ppad, gscale, dpart);
    hipLaunchKernelGGL(pa_reduce_kernel<false>, dim3((Ppad + 255) / 256, N), dim3(256), 0, st, dpart, pl.zs, Ppad, dot);
    hipLaunchKernelGGL(pa_scatter_kernel, dim3((unsigned)((long long)N * Cs), (unsigned)(((long long)h * w + 255) / 256)),
                       dim3(256), 0, st, US, sS, GT, dot, pl.gs, gscale, grad_out, dstudent);
    DCFP_RETURN_LAUNCH();
}
