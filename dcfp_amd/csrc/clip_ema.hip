// clip_ema.hip — global gradient-norm clipping and a weight EMA on the multi-tensor optimizer steps.
//   dcfp_grad_norm_f32          L2 norm of a list of gradient tensors in fp64 and torch's clip coefficient, two launches,
//                               no atomics: a read-only pass of 4 B per element plus one block over the partials
//   dcfp_sgd_momentum_ex_f32    the SGD / AdamW steps of eic_sgd.hip / adamw.hip (the same per-element bodies,
//   dcfp_adamw_ex_f32           optim_step.h) with the gradient entering as g * *coef and ema = lerp(ema, p_new, ema_w)
//                               in the epilogue: no pass that rewrites the gradients, no second pass over the weights
#include "common.h"
#include "optim_step.h"

namespace {

using namespace dcfp_optim;

constexpr int kThreads = 256;

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    return v;
}

__device__ __forceinline__ double sq(const float x) {
    const double d = (double)x;
    return d * d;                                   // exact: 48 significant bits at most
}

// ---------------------------------------------------------------------------------------------------------- the norm
// One block per DCFP_SGD_CHUNK elements of one tensor: part[blockIdx.x] = the chunk's sum of squares.  The chunk starts
// a multiple of 16384 floats behind the tensor, so it has the tensor's residue on the 16-byte grid: 0..3 head elements
// up to the first boundary, whole 16-byte vectors, 0..3 tail elements.  A lane adds its values in a fixed order and the
// block's lanes are combined in a fixed order, so the partial depends on the data alone.
__global__ void __launch_bounds__(kThreads)
grad_norm_part_kernel(const DcfpNormEntry* __restrict__ table, int n_tensors, double* __restrict__ part) {
    const long long chunk = blockIdx.x;
    const DcfpNormEntry e = table[find_entry(table, n_tensors, chunk)];
    const long long base = (chunk - e.first_chunk) * (long long)DCFP_SGD_CHUNK;
    const int t = threadIdx.x;
    double acc = 0.0;
    if (base < e.n) {
        long long end = base + DCFP_SGD_CHUNK;
        if (end > e.n) end = e.n;
        const int len = (int)(end - base);
        const gfloat* X = (const gfloat*)(e.data + base);
        int head = (int)(((16u - (unsigned)(reinterpret_cast<uintptr_t>(e.data) & 15u)) & 15u) >> 2);
        if (head > len) head = len;
        const int n4 = (len - head) >> 2;             // <= 4096: at most 16 vectors per lane
        const int tail = len - head - (n4 << 2);
        const gfloat4* X4 = (const gfloat4*)(X + head);
        for (int i0 = 0; i0 < n4; i0 += 4 * kThreads) {      // four 16-byte loads in flight per lane
            f32x4 v[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int i = i0 + u * kThreads + t;
                v[u] = 0.f;
                if (i < n4) v[u] = X4[i];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc += (sq(v[u][0]) + sq(v[u][1])) + (sq(v[u][2]) + sq(v[u][3]));
        }
        if (t < head) acc += sq(X[t]);
        else if (t >= 64 && t - 64 < tail) acc += sq(X[head + (n4 << 2) + (t - 64)]);
    }
    __shared__ double sm[kThreads / 64];
    acc = wave_sum_f64(acc);
    if ((t & 63) == 0) sm[t >> 6] = acc;
    __syncthreads();
    if (t == 0) part[chunk] = (sm[0] + sm[1]) + (sm[2] + sm[3]);
}

// One block.  Lane t adds the chunk partials of tensors t, t + 256, ... in ascending chunk order (the tensor's squared
// norm, left in the tensor's first partial); lane 0 then adds the tensors in ascending order and writes the record.
__global__ void __launch_bounds__(kThreads)
grad_norm_final_kernel(const DcfpNormEntry* __restrict__ table, int n_tensors, long long total_chunks,
                       double* __restrict__ part, float max_norm, double* __restrict__ tensor_sq,
                       DcfpGradNorm* __restrict__ result) {
    for (int i = threadIdx.x; i < n_tensors; i += kThreads) {
        const DcfpNormEntry e = table[i];
        const long long nc = (e.n + DCFP_SGD_CHUNK - 1) / DCFP_SGD_CHUNK;
        double s = 0.0;
        for (long long c = 0; c < nc; ++c) {
            const long long j = e.first_chunk + c;
            if (j >= 0 && j < total_chunks) s += part[j];
        }
        if (nc > 0 && e.first_chunk >= 0 && e.first_chunk < total_chunks) part[e.first_chunk] = s;
        if (tensor_sq) tensor_sq[i] = s;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    double total = 0.0;
#pragma unroll 8
    for (int i = 0; i < n_tensors; ++i) {
        const long long f = table[i].first_chunk;
        if (table[i].n > 0 && f >= 0 && f < total_chunks) total += part[f];
    }
    const float norm = (float)sqrt(total);
    // torch.nn.utils.clip_grad_norm_: clip_coef = max_norm / (total_norm + 1e-6), clamped to 1 (a NaN stays a NaN)
    const float c = __fdiv_rn(max_norm, __fadd_rn(norm, 1e-6f));
    result->sqnorm = total;
    result->norm = norm;
    result->coef = (n_tensors == 0 || c > 1.f) ? 1.f : c;
}

// ---------------------------------------------------------------------------------------------------------- the steps
// The walk over one chunk, shared by the two optimizers.  Op holds the chunk's pointers and scalars:
//   Op::vec()            every pointer of the entry on the 16-byte grid
//   Op::four(i)/one(i)   load, update and store vector i / element i
//   Op::two(i, j)        the same for two vectors with all loads issued before the first store (the stores of one may
//                        alias the loads of the other as far as the compiler knows)
template <class Op>
__device__ __forceinline__ void walk_chunk(const Op& op, const int len) {
    int done = 0;
    if (op.vec()) {
        const int n4 = len >> 2;                  // <= 4096: at most 16 float4 per thread
        for (int i = threadIdx.x; i < n4; i += 2 * kThreads) {
            const int j = i + kThreads;
            if (j < n4) op.two(i, j); else op.four(i);
        }
        done = n4 << 2;
    }
    for (int i = done + threadIdx.x; i < len; i += kThreads) op.one(i);     // the tail, or an unaligned entry
}

template <bool kClip>
struct SgdOp {
    gfloat* P; const gfloat* G; gfloat* B; gfloat* E;      // E null: no EMA for this entry
    bool aligned;
    float wd, lr, momentum, coef, ema_w;
    int first_step;

    __device__ __forceinline__ bool vec() const { return aligned; }
    __device__ __forceinline__ void elem(float& p, float g, float& b, float& e) const {
        if (kClip) g = mul_once(g, coef);                   // g.mul_(clip_coef)
        b = sgd_one(p, g, b, wd, lr, momentum, first_step);
        e = lerp_small(e, p, ema_w);
    }
    __device__ __forceinline__ void one(const int i) const {
        float p = P[i], b = first_step ? 0.f : B[i], e = E ? E[i] : 0.f;
        elem(p, G[i], b, e);
        P[i] = p; B[i] = b;
        if (E) E[i] = e;
    }
    struct Q { f32x4 p, g, b, e; };
    __device__ __forceinline__ Q load(const int i) const {
        Q q;
        q.p = ((gfloat4*)P)[i];
        q.g = ((const gfloat4*)G)[i];
        q.b = 0.f;
        if (!first_step) q.b = ((gfloat4*)B)[i];
        q.e = 0.f;
        if (E) q.e = ((gfloat4*)E)[i];
        return q;
    }
    __device__ __forceinline__ void finish(Q& q, const int i) const {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float p = q.p[c], b = q.b[c], e = q.e[c];
            elem(p, q.g[c], b, e);
            q.p[c] = p; q.b[c] = b; q.e[c] = e;
        }
        ((gfloat4*)P)[i] = q.p;
        ((gfloat4*)B)[i] = q.b;
        if (E) ((gfloat4*)E)[i] = q.e;
    }
    __device__ __forceinline__ void four(const int i) const { Q q = load(i); finish(q, i); }
    __device__ __forceinline__ void two(const int i, const int j) const {
        Q a = load(i), b = load(j);
        finish(a, i);
        finish(b, j);
    }
};

template <bool kClip>
struct AdamOp {
    gfloat* P; const gfloat* G; gfloat* M; gfloat* V; gfloat* E;
    bool aligned;
    AdamK k;
    float coef, ema_w;

    __device__ __forceinline__ bool vec() const { return aligned; }
    __device__ __forceinline__ void elem(float& p, float g, float& m, float& v, float& e) const {
        if (kClip) g = mul_once(g, coef);                   // g.mul_(clip_coef)
        adamw_one(p, g, m, v, k);
        e = lerp_small(e, p, ema_w);
    }
    __device__ __forceinline__ void one(const int i) const {
        float p = P[i], m = M[i], v = V[i], e = E ? E[i] : 0.f;
        elem(p, G[i], m, v, e);
        P[i] = p; M[i] = m; V[i] = v;
        if (E) E[i] = e;
    }
    struct Q { f32x4 p, g, m, v, e; };
    __device__ __forceinline__ Q load(const int i) const {
        Q q;
        q.p = ((gfloat4*)P)[i];
        q.g = ((const gfloat4*)G)[i];
        q.m = ((gfloat4*)M)[i];
        q.v = ((gfloat4*)V)[i];
        q.e = 0.f;
        if (E) q.e = ((gfloat4*)E)[i];
        return q;
    }
    __device__ __forceinline__ void finish(Q& q, const int i) const {
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            float p = q.p[c], m = q.m[c], v = q.v[c], e = q.e[c];
            elem(p, q.g[c], m, v, e);
            q.p[c] = p; q.m[c] = m; q.v[c] = v; q.e[c] = e;
        }
        ((gfloat4*)P)[i] = q.p;
        ((gfloat4*)M)[i] = q.m;
        ((gfloat4*)V)[i] = q.v;
        if (E) ((gfloat4*)E)[i] = q.e;
    }
    __device__ __forceinline__ void four(const int i) const { Q q = load(i); finish(q, i); }
    __device__ __forceinline__ void two(const int i, const int j) const {
        Q a = load(i), b = load(j);
        finish(a, i);
        finish(b, j);
    }
};

__device__ __forceinline__ bool on_grid(const void* a, const void* b, const void* c, const void* d, const void* e) {
    return ((reinterpret_cast<uintptr_t>(a) | reinterpret_cast<uintptr_t>(b) | reinterpret_cast<uintptr_t>(c) |
             reinterpret_cast<uintptr_t>(d) | reinterpret_cast<uintptr_t>(e)) & 15u) == 0;      // null counts as aligned
}

template <bool kClip>
__global__ void __launch_bounds__(kThreads)
sgd_ex_kernel(const DcfpSgdExEntry* __restrict__ table, int n_tensors, float lr, float momentum, int first_step,
              const float* __restrict__ coef, float ema_w) {
    const long long chunk = blockIdx.x;
    const DcfpSgdExEntry e = table[find_entry(table, n_tensors, chunk)];
    const long long base = (chunk - e.first_chunk) * (long long)DCFP_SGD_CHUNK;
    if (base >= e.n) return;
    long long end = base + DCFP_SGD_CHUNK;
    if (end > e.n) end = e.n;
    SgdOp<kClip> op;
    op.P = (gfloat*)(e.param + base);
    op.G = (const gfloat*)(e.grad + base);
    op.B = (gfloat*)(e.momentum_buf + base);
    op.E = e.ema ? (gfloat*)(e.ema + base) : nullptr;
    // base is a multiple of 16384 floats: the chunk is 16-byte aligned exactly when the entry's pointers are
    op.aligned = on_grid(e.param, e.grad, e.momentum_buf, e.ema, nullptr);
    op.wd = e.weight_decay; op.lr = lr; op.momentum = momentum; op.first_step = first_step;
    op.coef = kClip ? *coef : 1.f;
    op.ema_w = ema_w;
    walk_chunk(op, (int)(end - base));
}

template <bool kClip>
__global__ void __launch_bounds__(kThreads)
adamw_ex_kernel(const DcfpAdamExEntry* __restrict__ table, int n_tensors, const AdamK k,
                const float* __restrict__ coef, float ema_w) {
    const long long chunk = blockIdx.x;
    const DcfpAdamExEntry e = table[find_entry(table, n_tensors, chunk)];
    const long long base = (chunk - e.first_chunk) * (long long)DCFP_SGD_CHUNK;
    if (base >= e.n) return;
    long long end = base + DCFP_SGD_CHUNK;
    if (end > e.n) end = e.n;
    AdamOp<kClip> op;
    op.P = (gfloat*)(e.param + base);
    op.G = (const gfloat*)(e.grad + base);
    op.M = (gfloat*)(e.exp_avg + base);
    op.V = (gfloat*)(e.exp_avg_sq + base);
    op.E = e.ema ? (gfloat*)(e.ema + base) : nullptr;
    op.aligned = on_grid(e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.ema);
    op.k = k;
    op.coef = kClip ? *coef : 1.f;
    op.ema_w = ema_w;
    walk_chunk(op, (int)(end - base));
}

bool bad_step_args(const void* table, int n_tensors, int64_t total_chunks, float ema_w) {
    return n_tensors < 0 || total_chunks < 0 || total_chunks > 0x7fffffffLL || !(ema_w >= 0.f && ema_w < 0.5f) ||
           (n_tensors > 0 && total_chunks > 0 && !table);
}

}  // namespace

extern "C" size_t dcfp_grad_norm_workspace_bytes(int64_t total_chunks) {
    return total_chunks > 0 ? (size_t)total_chunks * sizeof(double) : 0;
}

extern "C" int dcfp_grad_norm_f32(const DcfpNormEntry* table, int n_tensors, int64_t total_chunks, float max_norm,
                                  void* workspace, size_t workspace_bytes, double* tensor_sq, DcfpGradNorm* result,
                                  dcfp_stream_t stream) {
    if (n_tensors < 0 || total_chunks < 0 || total_chunks > 0x7fffffffLL || !(max_norm > 0.f) || !result ||
        (reinterpret_cast<uintptr_t>(result) & 7u) || (reinterpret_cast<uintptr_t>(tensor_sq) & 7u))
        return DCFP_E_BADDESC;
    if (n_tensors > 0 && !table) return DCFP_E_BADDESC;
    if (n_tensors == 0) total_chunks = 0;
    if (total_chunks > 0) {
        if (!workspace || (reinterpret_cast<uintptr_t>(workspace) & 7u) ||
            workspace_bytes < dcfp_grad_norm_workspace_bytes(total_chunks))
            return DCFP_E_WORKSPACE;
        hipLaunchKernelGGL(grad_norm_part_kernel, dim3((unsigned)total_chunks), dim3(kThreads), 0, dcfp_s(stream),
                           table, n_tensors, static_cast<double*>(workspace));
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(grad_norm_final_kernel, dim3(1), dim3(kThreads), 0, dcfp_s(stream), table, n_tensors,
                       (long long)total_chunks, static_cast<double*>(workspace), max_norm, tensor_sq, result);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_sgd_momentum_ex_f32(const DcfpSgdExEntry* table, int n_tensors, int64_t total_chunks, float lr,
                                        float momentum, int first_step, const float* coef, float ema_w,
                                        dcfp_stream_t stream) {
    if (bad_step_args(table, n_tensors, total_chunks, ema_w)) return DCFP_E_BADDESC;
    if (n_tensors == 0 || total_chunks == 0) return DCFP_OK;
    if (coef)
        hipLaunchKernelGGL(sgd_ex_kernel<true>, dim3((unsigned)total_chunks), dim3(kThreads), 0, dcfp_s(stream), table,
                           n_tensors, lr, momentum, first_step, coef, ema_w);
    else
        hipLaunchKernelGGL(sgd_ex_kernel<false>, dim3((unsigned)total_chunks), dim3(kThreads), 0, dcfp_s(stream), table,
                           n_tensors, lr, momentum, first_step, coef, ema_w);
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_adamw_ex_f32(const DcfpAdamExEntry* table, int n_tensors, int64_t total_chunks, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, float bias_correction1,
                                 float bias_correction2_sqrt, const float* coef, float ema_w, dcfp_stream_t stream) {
    if (bad_step_args(table, n_tensors, total_chunks, ema_w)) return DCFP_E_BADDESC;
    if (n_tensors == 0 || total_chunks == 0) return DCFP_OK;
    AdamK k;
    k.decay = (float)(1.0 - (double)lr * (double)weight_decay);     // in double, as torch's Python scalars are
    k.step = (float)((double)lr / (double)bias_correction1);
    k.w1 = (float)(1.0 - (double)beta1);
    k.beta2 = beta2;
    k.omb2 = (float)(1.0 - (double)beta2);
    k.bc2_sqrt = bias_correction2_sqrt;
    k.eps = eps;
    if (coef)
        hipLaunchKernelGGL(adamw_ex_kernel<true>, dim3((unsigned)total_chunks), dim3(kThreads), 0, dcfp_s(stream), table,
                           n_tensors, k, coef, ema_w);
    else
        hipLaunchKernelGGL(adamw_ex_kernel<false>, dim3((unsigned)total_chunks), dim3(kThreads), 0, dcfp_s(stream),
                           table, n_tensors, k, coef, ema_w);
    DCFP_RETURN_LAUNCH();
}
