// adamw.hip — torch.optim.AdamW.step (optimizer.py:26-31, the reference's `--optim adamw`) over a list of
// tensors as ONE launch over a device-resident pointer table, in the manner of sgd_momentum_kernel.
// Streaming: 16 B read and 12 B written per element; one block per DCFP_SGD_CHUNK elements of one tensor.
#include "common.h"
#include "optim_step.h"

namespace {

using namespace dcfp_optim;      // AdamK, adamw_one: shared with clip_ema.hip

__device__ __forceinline__ void adamw_four(f32x4& p, const f32x4 g, f32x4& m, f32x4& v, const AdamK k) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float pc = p[c], mc = m[c], vc = v[c];
        adamw_one(pc, g[c], mc, vc, k);
        p[c] = pc; m[c] = mc; v[c] = vc;
    }
}

__global__ void __launch_bounds__(256)
adamw_kernel(const DcfpAdamEntry* __restrict__ table, int n_tensors, const AdamK k) {
    // binary search: last entry with first_chunk <= blockIdx.x
    const long long chunk = blockIdx.x;
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    const DcfpAdamEntry e = table[lo];
    const long long base = (chunk - e.first_chunk) * (long long)DCFP_SGD_CHUNK;
    if (base >= e.n) return;                      // (a table whose first_chunk leaves a gap: nothing to do)
    long long end = base + DCFP_SGD_CHUNK;
    if (end > e.n) end = e.n;
    const int len = (int)(end - base);
    // The pointers come out of the table, so the compiler only knows them as generic: say that they are global memory
    // (global_load / global_store instead of flat instructions)
    gfloat* P = (gfloat*)(e.param + base);
    const gfloat* G = (const gfloat*)(e.grad + base);
    gfloat* M = (gfloat*)(e.exp_avg + base);
    gfloat* V = (gfloat*)(e.exp_avg_sq + base);
    // base is a multiple of 16384 floats: the chunk is 16-byte aligned exactly when the entry's pointers are
    const bool vec = ((reinterpret_cast<uintptr_t>(e.param) | reinterpret_cast<uintptr_t>(e.grad) |
                       reinterpret_cast<uintptr_t>(e.exp_avg) | reinterpret_cast<uintptr_t>(e.exp_avg_sq)) & 15u) == 0;
    int done = 0;
    if (vec) {
        const int n4 = len >> 2;                  // <= 4096: at most 16 float4 per thread
        gfloat4* P4 = (gfloat4*)P;
        const gfloat4* G4 = (const gfloat4*)G;
        gfloat4* M4 = (gfloat4*)M;
        gfloat4* V4 = (gfloat4*)V;
        // two float4 per operand in flight per thread (128 B of loads, 32 KiB per block) before the first is used:
        // the stores of one iteration may alias the loads of the next as far as the compiler knows, so it would not
        // hoist them itself
        for (int i = threadIdx.x; i < n4; i += 512) {
            const int j = i + 256;
            const bool two = j < n4;
            f32x4 p0 = P4[i], m0 = M4[i], v0 = V4[i];
            const f32x4 g0 = G4[i];
            f32x4 p1 = 0.f, m1 = 0.f, v1 = 0.f, g1 = 0.f;
            if (two) { p1 = P4[j]; m1 = M4[j]; v1 = V4[j]; g1 = G4[j]; }
            adamw_four(p0, g0, m0, v0, k);
            P4[i] = p0; M4[i] = m0; V4[i] = v0;
            if (two) {
                adamw_four(p1, g1, m1, v1, k);
                P4[j] = p1; M4[j] = m1; V4[j] = v1;
            }
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += 256) {      // the tail (< 4 elements), or an unaligned entry
        float p = P[i], m = M[i], v = V[i];
        adamw_one(p, G[i], m, v, k);
        P[i] = p; M[i] = m; V[i] = v;
    }
}

}  // namespace

extern "C" int dcfp_adamw_f32(const DcfpAdamEntry* table, int n_tensors, int64_t total_chunks,
                              float lr, float beta1, float beta2, float eps, float weight_decay,
                              float bias_correction1, float bias_correction2_sqrt, dcfp_stream_t stream) {
    if (n_tensors < 0 || total_chunks < 0 || total_chunks > 0x7fffffffLL) return DCFP_E_BADDESC;
    if (n_tensors == 0 || total_chunks == 0) return DCFP_OK;
    if (!table) return DCFP_E_BADDESC;
    AdamK k;
    k.decay = (float)(1.0 - (double)lr * (double)weight_decay);     // in double, as torch's Python scalars are
    k.step = (float)((double)lr / (double)bias_correction1);
    k.w1 = (float)(1.0 - (double)beta1);
    k.beta2 = beta2;
    k.omb2 = (float)(1.0 - (double)beta2);
    k.bc2_sqrt = bias_correction2_sqrt;
    k.eps = eps;
    hipLaunchKernelGGL(adamw_kernel, dim3((unsigned)total_chunks), dim3(256), 0, dcfp_s(stream),
                       table, n_tensors, k);
    DCFP_RETURN_LAUNCH();
}
