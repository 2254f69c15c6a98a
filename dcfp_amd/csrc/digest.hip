// digest.hip — a 128-bit digest of a buffer of 32-bit words at the rate of a read-only pass:
//   d0 = sum_i w_i          d1 = sum_i (b + i + 1) * w_i          (mod 2^64, b = index_base)
// Integer sums are associative: no reduction order matters, so the kernel needs neither atomics nor a fixed order and
// two calls give the same pair.  The buffer is read as bits (-0.0 != 0.0, NaN payloads and denormals count).
//
// Layout of a call over n words at a 4-byte aligned address:
//   head   0..3 words up to the first 16-byte boundary            \  summed by the finalize block
//   tail   0..3 words after the last whole 16-byte vector         /
//   body   nvec uint4 vectors in CHUNKS of DCFP_DIGEST_CHUNK words; block k takes chunks k, k + grid, ...
// Inside a chunk a lane keeps s0 = sum w and s1 = sum j*w with the 32-bit chunk-local word index j, one
// 32x32->64 multiply-add per word; the chunk's first index is folded in once per chunk (c * s0), the rest once per lane.
#include "common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kVecPerLane = DCFP_DIGEST_CHUNK / 4 / kThreads;      // 4 uint4 per lane and chunk
constexpr long long kMaxBlocks = DCFP_DIGEST_MAX_BLOCKS;
static_assert(kVecPerLane * 4 * kThreads == DCFP_DIGEST_CHUNK, "a chunk is a whole number of 16-byte loads per lane");

typedef unsigned long long u64;

__device__ __forceinline__ u64 wave_sum_u64(u64 v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ void take(const uint4 v, uint32_t j, u64& s0, u64& s1) {
    s0 += (u64)v.x + (u64)v.y;
    s0 += (u64)v.z + (u64)v.w;
    s1 += (u64)j * v.x;
    s1 += (u64)(j + 1) * v.y;
    s1 += (u64)(j + 2) * v.z;
    s1 += (u64)(j + 3) * v.w;
}

// body: vectors [0, nvec) at `vec` (16-byte aligned); first: b + 1 + the word index of the body's first word.
// part[2*block] = the block's share of d0, part[2*block + 1] of d1.
__global__ void __launch_bounds__(kThreads)
digest_body_kernel(const uint4* __restrict__ vec, long long nvec, u64 first, u64* __restrict__ part) {
    constexpr long long kChunkVec = DCFP_DIGEST_CHUNK / 4;
    const long long nchunks = (nvec + kChunkVec - 1) / kChunkVec;
    const uint32_t t = threadIdx.x;
    u64 a0 = 0;          // sum of w over this lane's words
    u64 a1 = 0;          // sum of j * w, j chunk-local
    u64 ac = 0;          // sum over chunks of c * (the lane's s0 in chunk c)
    for (long long c = blockIdx.x; c < nchunks; c += gridDim.x) {
        const uint4* p = vec + c * kChunkVec;
        u64 s0 = 0;
        if ((c + 1) * kChunkVec <= nvec) {
            uint4 v[kVecPerLane];
#pragma unroll
            for (int u = 0; u < kVecPerLane; ++u) v[u] = p[t + u * kThreads];
#pragma unroll
            for (int u = 0; u < kVecPerLane; ++u) take(v[u], 4u * (t + u * kThreads), s0, a1);
        } else {
            const long long left = nvec - c * kChunkVec;
#pragma unroll
            for (int u = 0; u < kVecPerLane; ++u) {
                const uint32_t i = t + u * kThreads;
                if ((long long)i < left) take(p[i], 4u * i, s0, a1);
            }
        }
        a0 += s0;
        ac += (u64)c * s0;
    }
    // word index of (chunk c, local j) within the body is c*CHUNK + j
    u64 d0 = a0;
    u64 d1 = first * a0 + (u64)DCFP_DIGEST_CHUNK * ac + a1;
    __shared__ u64 sm[2 * (kThreads / 64)];
    d0 = wave_sum_u64(d0);
    d1 = wave_sum_u64(d1);
    const int lane = t & 63, wid = t >> 6;
    if (lane == 0) { sm[2 * wid] = d0; sm[2 * wid + 1] = d1; }
    __syncthreads();
    if (t == 0) {
        u64 r0 = 0, r1 = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) { r0 += sm[2 * w]; r1 += sm[2 * w + 1]; }
        part[2 * blockIdx.x] = r0;
        part[2 * blockIdx.x + 1] = r1;
    }
}

// one block: the per-block partials plus the head and tail words
__global__ void __launch_bounds__(kThreads)
digest_final_kernel(const u64* __restrict__ part, int nparts, const uint32_t* __restrict__ words, long long n, int head,
                    int tail, u64 base, u64* __restrict__ out2) {
    const int t = threadIdx.x;
    u64 d0 = 0, d1 = 0;
    for (int i = t; i < nparts; i += kThreads) { d0 += part[2 * i]; d1 += part[2 * i + 1]; }
    if (t < head) {
        const u64 w = words[t];
        d0 += w; d1 += (base + (u64)t + 1) * w;
    } else if (t >= 64 && t - 64 < tail) {
        const long long i = n - tail + (t - 64);
        const u64 w = words[i];
        d0 += w; d1 += (base + (u64)i + 1) * w;
    }
    __shared__ u64 sm[2 * (kThreads / 64)];
    d0 = wave_sum_u64(d0);
    d1 = wave_sum_u64(d1);
    const int lane = t & 63, wid = t >> 6;
    if (lane == 0) { sm[2 * wid] = d0; sm[2 * wid + 1] = d1; }
    __syncthreads();
    if (t == 0) {
        u64 r0 = 0, r1 = 0;
#pragma unroll
        for (int w = 0; w < kThreads / 64; ++w) { r0 += sm[2 * w]; r1 += sm[2 * w + 1]; }
        out2[0] = r0;
        out2[1] = r1;
    }
}

// blocks of the body pass for n words at ANY alignment (the head takes at most 3 words away from the body)
long long body_blocks_upper(size_t n_words) {
    const size_t chunks = (n_words / 4 + DCFP_DIGEST_CHUNK / 4 - 1) / (DCFP_DIGEST_CHUNK / 4);
    return chunks < (size_t)kMaxBlocks ? (long long)chunks : kMaxBlocks;
}

}  // namespace

extern "C" size_t dcfp_state_digest_workspace_bytes(size_t n_words) {
    return (size_t)body_blocks_upper(n_words) * 2 * sizeof(u64);
}

extern "C" int dcfp_state_digest_u64(const void* data, size_t n_words, uint64_t index_base, void* workspace,
                                     size_t workspace_bytes, uint64_t* out2, dcfp_stream_t stream) {
    if (!out2 || (reinterpret_cast<uintptr_t>(out2) & 7u)) return DCFP_E_BADDESC;
    if (n_words > 0 && (!data || (reinterpret_cast<uintptr_t>(data) & 3u))) return DCFP_E_BADDESC;
    if (n_words > ((size_t)1 << 60)) return DCFP_E_UNSUPPORTED;
    const uintptr_t addr = reinterpret_cast<uintptr_t>(data);
    size_t head = n_words ? ((16u - (addr & 15u)) & 15u) / 4u : 0;
    if (head > n_words) head = n_words;
    const size_t nvec = (n_words - head) / 4;
    const int tail = (int)(n_words - head - 4 * nvec);
    const long long blocks = body_blocks_upper(4 * nvec);
    if (blocks > 0) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) ||
            workspace_bytes < dcfp_state_digest_workspace_bytes(n_words))
            return DCFP_E_WORKSPACE;
        const uint4* vec = reinterpret_cast<const uint4*>(static_cast<const uint32_t*>(data) + head);
        hipLaunchKernelGGL(digest_body_kernel, dim3((unsigned)blocks), dim3(kThreads), 0, dcfp_s(stream), vec,
                           (long long)nvec, (u64)index_base + 1 + (u64)head, static_cast<u64*>(workspace));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(digest_final_kernel, dim3(1), dim3(kThreads), 0, dcfp_s(stream),
                       static_cast<const u64*>(workspace), (int)blocks, static_cast<const uint32_t*>(data),
                       (long long)n_words, (int)head, tail, (u64)index_base, reinterpret_cast<u64*>(out2));
    DCFP_RETURN_LAUNCH();
}
