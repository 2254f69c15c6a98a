// score.hip — the baseline pruning criteria next to the EIC score of eic_sgd.hip:
//   gate kernels     first-order Taylor on the BN gate, the Network Slimming L1 term     (per step, all layers, 1 launch)
//   filter_reduce    sum|w|, sqrt(sum w^2), (sum w*g)^2 per filter of every conv          (1 launch for the model)
//   fpgm             sum_j ||w_i - w_j|| per filter of every conv                        (2 launches for the model)
// All of them read a device-resident table of records, use no atomics and add in a fixed order.
#include "common.h"

namespace {

// ------------------------------------------------------------------------------------------------ gate kernels
// One block per scored BN layer (C <= 2048 floats each: latency-bound, as eic_update_kernel).  Every product and sum is
// rounded on its own, so a float32 restatement one operation at a time gives the same bits and exact zeros stay exact.
// That is fmul / fadd in round-to-nearest, written with plain operators under `fp contract(off)`: the products of the
// __fmul_rn / __fadd_rn intrinsics are inlined with the header's contraction setting, and hipcc then fuses
// score + t*t into an FMA (one ulp off the restatement; see also running_update in common.h).
__global__ void __launch_bounds__(256)
gate_taylor_kernel(const DcfpGateEntry* __restrict__ table) {
#pragma clang fp contract(off)
    const DcfpGateEntry e = table[blockIdx.x];
    for (int i = threadIdx.x; i < e.n; i += 256) {
        const float a = e.gamma[i] * e.ggrad[i];
        const float b = e.beta[i] * e.bgrad[i];
        const float t = a + b;
        const float tt = t * t;
        e.score[i] = e.score[i] + tt;
    }
}

__global__ void __launch_bounds__(256)
gate_l1reg_kernel(const DcfpGateEntry* __restrict__ table, float lambda) {
#pragma clang fp contract(off)
    const DcfpGateEntry e = table[blockIdx.x];
    for (int i = threadIdx.x; i < e.n; i += 256) {
        const float w = e.gamma[i];
        const float s = (w > 0.f) ? 1.f : ((w < 0.f) ? -1.f : 0.f);
        if (s != 0.f) {                               // sign(0) = 0: the gradient keeps its bits (a -0 included)
            const float p = lambda * s;
            e.ggrad[i] = e.ggrad[i] + p;
        }
    }
}

// ----------------------------------------------------------------------------------------------- filter_reduce
// The split rule (restated in include/dcfp_hip.h): a row of K floats is summed by a group of G lanes,
//   K <= 32: G = 8     K <= 128: G = 16     K <= 1024: G = 64     above: G = 256,
// and a block (one unit) takes 256/G rows, so the 27-float stem rows fill a block 32 at a time and an 18432-float ASPP
// row is spread over all 256 threads.  G <= 16: lane l adds elements l, l+G, ... in order (<= 8 of them).  G >= 64: the
// row is cut at its 16-byte boundaries into <= 3 head floats, float4s and <= 3 tail floats; lane l takes float4s l,
// l+G, ... into one accumulator per component, adds them as (x+y)+(z+w), then its head or tail float.  The lanes of a
// group are added by a butterfly (xor 32 ... 1 inside a wave), the four waves of G = 256 as (s0+s1)+(s2+s3).  Longest
// chain of additions: ceil(K/G) + log2(G) for G <= 16; ceil(K/(4G)) + 4 + log2(min(G,64)) (+ 2 for G = 256) above.
__host__ __device__ inline int filter_group(int K) { return K <= 32 ? 8 : K <= 128 ? 16 : K <= 1024 ? 64 : 256; }

template <int OP>
__device__ __forceinline__ float filter_term(float w, float g, float acc) {
    if (OP == DCFP_FILTER_ABS_SUM) return acc + fabsf(w);
    if (OP == DCFP_FILTER_L2) return fmaf(w, w, acc);
    return fmaf(w, g, acc);
}

template <int OP>
__device__ __forceinline__ float filter_row_wide(const float* __restrict__ w, const float* __restrict__ g, int K, int lane,
                                                 int G) {
    constexpr bool DOT = OP == DCFP_FILTER_DOT_SQ_ACC;
    int head = (int)((16u - (unsigned)(reinterpret_cast<uintptr_t>(w) & 15u)) & 15u) >> 2;   // floats up to a 16-byte boundary
    if (head > K) head = K;
    const int nvec = (K - head) >> 2;
    const int tail0 = head + (nvec << 2);
    const float4* wv = reinterpret_cast<const float4*>(w + head);
    const bool g_vec = DOT && ((reinterpret_cast<uintptr_t>(g + head) & 15u) == 0);           // same for the whole row
    float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
    for (int i = lane; i < nvec; i += G) {
        const float4 x = wv[i];
        float4 y = make_float4(0.f, 0.f, 0.f, 0.f);
        if (DOT) {
            if (g_vec) {
                y = reinterpret_cast<const float4*>(g + head)[i];
            } else {
                const float* gp = g + head + 4 * (size_t)i;
                y = make_float4(gp[0], gp[1], gp[2], gp[3]);
            }
        }
        a0 = filter_term<OP>(x.x, y.x, a0);
        a1 = filter_term<OP>(x.y, y.y, a1);
        a2 = filter_term<OP>(x.z, y.z, a2);
        a3 = filter_term<OP>(x.w, y.w, a3);
    }
    float acc = (a0 + a1) + (a2 + a3);
    if (lane < head) acc = filter_term<OP>(w[lane], DOT ? g[lane] : 0.f, acc);
    const int t = tail0 + (lane - head);               // the tail floats go to the lanes behind the head's (G >= 64 > 6)
    if (lane >= head && t < K) acc = filter_term<OP>(w[t], DOT ? g[t] : 0.f, acc);
    return acc;
}

template <int OP>
__device__ __forceinline__ void filter_store(float* out, float s) {
    if (OP == DCFP_FILTER_ABS_SUM) *out = s;
    else if (OP == DCFP_FILTER_L2) *out = sqrtf(s);
    else *out = *out + s * s;
}

template <int OP>
__global__ void __launch_bounds__(256)
filter_reduce_kernel(const DcfpFilterEntry* __restrict__ table, int n_entries) {
    __shared__ float smem[4];
    const long long unit = blockIdx.x;
    int lo = 0, hi = n_entries - 1;                     // last entry with first_unit <= unit
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_unit <= unit) lo = mid; else hi = mid - 1;
    }
    const DcfpFilterEntry e = table[lo];
    const int K = e.K, G = filter_group(K);
    const long long u = unit - e.first_unit;
    if (u < 0 || K < 1) return;
    const int tid = threadIdx.x;
    if (G == 256) {                                     // one row per block (block-uniform branch)
        if (u >= e.rows) return;
        const size_t off = (size_t)u * (size_t)K;
        const float acc = filter_row_wide<OP>(e.w + off, e.g ? e.g + off : nullptr, K, tid, 256);
        const float s = block_sum_256(acc, smem);
        if (tid == 0) filter_store<OP>(e.out + u, s);
        return;
    }
    const int per_unit = 256 / G;
    const long long row = u * per_unit + tid / G;
    const int lane = tid % G;
    const bool live = row < e.rows;
    float acc = 0.f;
    if (live) {
        const size_t off = (size_t)row * (size_t)K;
        const float* w = e.w + off;
        const float* g = e.g ? e.g + off : nullptr;
        if (G == 64) {
            acc = filter_row_wide<OP>(w, g, K, lane, 64);
        } else {
            for (int k = lane; k < K; k += G)
                acc = filter_term<OP>(w[k], OP == DCFP_FILTER_DOT_SQ_ACC ? g[k] : 0.f, acc);
        }
    }
    // butterfly over the G lanes of a group (groups are aligned runs of lanes inside a wave): every lane ends with the sum
    for (int m = G >> 1; m > 0; m >>= 1) acc += __shfl_xor(acc, m, 64);
    if (live && lane == 0) filter_store<OP>(e.out + row, acc);
}

// ------------------------------------------------------------------------------------------------------- fpgm
// Launch 1: block = (i tile, j tile) of 64 x 64 filter pairs, 256 threads, thread (ti, tj) = (tid / 16, tid % 16) owns the
// 4 x 4 pairs (ti + 16 a, tj + 16 b).  K goes through LDS in chunks of 32 floats (rows and chunk ends past the matrix are
// zero-filled: they add (0 - 0)^2); the squared differences of a chunk are summed from zero, k ascending, and the chunk's
// sum is then added to the pair's total: the longest chain of a distance is 32 + ceil(K/32) additions, not K.  The thread
// adds the sqrt of its 4 pairs of a row i (b ascending, pairs with j >= C left out), the 16 threads of the row are added
// by a butterfly, and the sum over the j tile goes to the workspace at [j tile][i].  Launch 2 adds the j tiles in
// ascending order: 3 + 4 + ceil(C/64) additions per row sum.
constexpr int FP_T = DCFP_FPGM_TILE, FP_KC = 32, FP_LD = FP_KC + 4;     // rows 144 B apart: float4 reads, 16 rows on 16 slots

__device__ __forceinline__ void fpgm_stage(float (*dst)[FP_LD], const float* __restrict__ w, int row0, int C, int K, int k0) {
    // 64 rows x 32 floats: thread t takes column t % 32 of rows t / 32, + 8, ... (128 contiguous bytes per row)
    const int c = threadIdx.x & 31, k = k0 + c;
    for (int r = threadIdx.x >> 5; r < FP_T; r += 8) {
        const int row = row0 + r;
        dst[r][c] = (row < C && k < K) ? w[(size_t)row * (size_t)K + k] : 0.f;
    }
}

__global__ void __launch_bounds__(256)
fpgm_tile_kernel(const DcfpFpgmEntry* __restrict__ table, int n_entries, float* __restrict__ ws, long long ws_floats) {
    __shared__ __attribute__((aligned(16))) float A[FP_T][FP_LD];
    __shared__ __attribute__((aligned(16))) float B[FP_T][FP_LD];
    const long long tile = blockIdx.x;
    int lo = 0, hi = n_entries - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_tile <= tile) lo = mid; else hi = mid - 1;
    }
    const DcfpFpgmEntry e = table[lo];
    const int C = e.C, K = e.K;
    if (C < 1 || K < 1) return;
    const long long nt = (C + FP_T - 1) / FP_T, t = tile - e.first_tile;
    if (t < 0 || t >= nt * nt) return;
    if (e.ws_off < 0 || e.ws_off + nt * (long long)C > ws_floats) return;     // a table that does not fit its workspace
    const int it = (int)(t / nt), jt = (int)(t % nt);
    const int i0 = it * FP_T, j0 = jt * FP_T;
    const int ti = threadIdx.x >> 4, tj = threadIdx.x & 15;
    float tot[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) tot[a][b] = 0.f;
    for (int k0 = 0; k0 < K; k0 += FP_KC) {
        __syncthreads();                                // the chunk before is read
        fpgm_stage(A, e.w, i0, C, K, k0);
        fpgm_stage(B, e.w, j0, C, K, k0);
        __syncthreads();
        float part[4][4];
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) part[a][b] = 0.f;
#pragma unroll 2
        for (int k = 0; k < FP_KC; k += 4) {
            float4 x[4], y[4];
#pragma unroll
            for (int a = 0; a < 4; ++a) x[a] = *reinterpret_cast<const float4*>(&A[ti + 16 * a][k]);
#pragma unroll
            for (int b = 0; b < 4; ++b) y[b] = *reinterpret_cast<const float4*>(&B[tj + 16 * b][k]);
#pragma unroll
            for (int a = 0; a < 4; ++a)
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    float d, p = part[a][b];
                    d = x[a].x - y[b].x; p = fmaf(d, d, p);
                    d = x[a].y - y[b].y; p = fmaf(d, d, p);
                    d = x[a].z - y[b].z; p = fmaf(d, d, p);
                    d = x[a].w - y[b].w; p = fmaf(d, d, p);
                    part[a][b] = p;
                }
        }
#pragma unroll
        for (int a = 0; a < 4; ++a)
#pragma unroll
            for (int b = 0; b < 4; ++b) tot[a][b] += part[a][b];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        float s = 0.f;
#pragma unroll
        for (int b = 0; b < 4; ++b) s += (j0 + tj + 16 * b < C) ? sqrtf(tot[a][b]) : 0.f;
        for (int m = 8; m > 0; m >>= 1) s += __shfl_xor(s, m, 64);           // the 16 lanes tj of this ti
        const int i = i0 + ti + 16 * a;
        if (tj == 0 && i < C) ws[e.ws_off + (long long)jt * C + i] = s;
    }
}

__global__ void __launch_bounds__(256)
fpgm_rows_kernel(const DcfpFpgmEntry* __restrict__ table, const float* __restrict__ ws, long long ws_floats) {
    const DcfpFpgmEntry e = table[blockIdx.x];
    const int C = e.C;
    if (C < 1 || e.K < 1) return;
    const long long nt = (C + FP_T - 1) / FP_T;
    if (e.ws_off < 0 || e.ws_off + nt * (long long)C > ws_floats) return;
    for (int i = threadIdx.x; i < C; i += 256) {
        float s = 0.f;
        for (long long j = 0; j < nt; ++j) s += ws[e.ws_off + j * C + i];
        e.out[i] = s;
    }
}

}  // namespace

extern "C" int dcfp_gate_taylor_f32(const DcfpGateEntry* table, int n_layers, dcfp_stream_t stream) {
    if (n_layers == 0) return DCFP_OK;
    if (!table || n_layers < 0) return DCFP_E_BADDESC;
    hipLaunchKernelGGL(gate_taylor_kernel, dim3((unsigned)n_layers), dim3(256), 0, dcfp_s(stream), table);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_gate_l1reg_f32(const DcfpGateEntry* table, int n_layers, float lambda, dcfp_stream_t stream) {
    if (n_layers == 0) return DCFP_OK;
    if (!table || n_layers < 0) return DCFP_E_BADDESC;
    hipLaunchKernelGGL(gate_l1reg_kernel, dim3((unsigned)n_layers), dim3(256), 0, dcfp_s(stream), table, lambda);
    DCFP_RETURN_LAUNCH();
}

extern "C" int64_t dcfp_filter_reduce_units(int rows, int K) {
    if (rows < 1 || K < 1) return 0;
    const int per_unit = 256 / filter_group(K);
    return ((int64_t)rows + per_unit - 1) / per_unit;
}

extern "C" int dcfp_filter_reduce_f32(const DcfpFilterEntry* table, int n_entries, int64_t total_units, int op,
                                      dcfp_stream_t stream) {
    if (n_entries == 0 || total_units == 0) return DCFP_OK;
    if (!table || n_entries < 0 || total_units < 0 || op < DCFP_FILTER_ABS_SUM || op > DCFP_FILTER_DOT_SQ_ACC)
        return DCFP_E_BADDESC;
    if (total_units > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    const dim3 grid((unsigned)total_units), block(256);
    if (op == DCFP_FILTER_ABS_SUM)
        hipLaunchKernelGGL(filter_reduce_kernel<DCFP_FILTER_ABS_SUM>, grid, block, 0, dcfp_s(stream), table, n_entries);
    else if (op == DCFP_FILTER_L2)
        hipLaunchKernelGGL(filter_reduce_kernel<DCFP_FILTER_L2>, grid, block, 0, dcfp_s(stream), table, n_entries);
    else
        hipLaunchKernelGGL(filter_reduce_kernel<DCFP_FILTER_DOT_SQ_ACC>, grid, block, 0, dcfp_s(stream), table, n_entries);
    DCFP_RETURN_LAUNCH();
}

extern "C" size_t dcfp_fpgm_workspace_bytes(int C) {
    if (C < 1) return 0;
    const size_t nt = ((size_t)C + FP_T - 1) / FP_T;
    return ((nt * (size_t)C * sizeof(float) + 255) / 256) * 256;
}

extern "C" int dcfp_fpgm_f32(const DcfpFpgmEntry* table, int n_entries, int64_t total_tiles, void* workspace,
                             size_t workspace_bytes, dcfp_stream_t stream) {
    if (n_entries == 0 || total_tiles == 0) return DCFP_OK;
    if (!table || n_entries < 0 || total_tiles < 0) return DCFP_E_BADDESC;
    if (!workspace || workspace_bytes < sizeof(float) || (reinterpret_cast<uintptr_t>(workspace) & 3u))
        return DCFP_E_WORKSPACE;
    if (total_tiles > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    float* ws = static_cast<float*>(workspace);
    const long long ws_floats = (long long)(workspace_bytes / sizeof(float));
    hipLaunchKernelGGL(fpgm_tile_kernel, dim3((unsigned)total_tiles), dim3(256), 0, dcfp_s(stream), table, n_entries, ws,
                       ws_floats);
    hipError_t err = hipGetLastError();
    if (err != hipSuccess) return (int)err;
    hipLaunchKernelGGL(fpgm_rows_kernel, dim3((unsigned)n_entries), dim3(256), 0, dcfp_s(stream), table, ws, ws_floats);
    DCFP_RETURN_LAUNCH();
}
