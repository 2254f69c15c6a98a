// optim_step.h — the per-element bodies of the optimizer steps, shared by the plain kernels (eic_sgd.hip, adamw.hip)
// and the clipped / EMA ones (clip_ema.hip): one statement of each update, so the entry points cannot drift apart.
#pragma once
#include "common.h"

namespace dcfp_optim {

typedef __attribute__((address_space(1))) float gfloat;
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(1))) f32x4 gfloat4;

struct AdamK {
    float decay;     // float(1 - lr*wd)
    float step;      // float(lr / bias_correction1)
    float w1;        // float(1 - beta1): the lerp weight
    float beta2;
    float omb2;      // float(1 - beta2)
    float bc2_sqrt;
    float eps;
};

// a * b rounded on its own whatever consumes it: the product carries no contract flag, so a following add or
// subtract cannot be fused with it (torch's g.mul_(clip_coef) is a pass of its own)
__device__ __forceinline__ float mul_once(const float a, const float b) {
#pragma clang fp contract(off)
    const float r = a * b;
    return r;
}

// torch.optim.SGD (momentum, weight decay, dampening 0, no nesterov) for one element; bprev is not used on the first
// step.  Returns the new momentum buffer value.
__device__ __forceinline__ float sgd_one(float& p, float g, const float bprev, const float wd, const float lr,
                                         const float momentum, const int first_step) {
    if (wd != 0.f) g = fmaf(wd, p, g);          // grad.add(param, alpha=wd)
    float b;
    if (first_step) b = g;                        // buf = clone(grad)
    // buf.mul_(m).add_(g).  The compiler has always contracted this product and sum of dcfp_sgd_momentum_f32 into one
    // fma (the __f*_rn intrinsics do not stop it); spelled out, so that every kernel that shares the body has its bits
    else b = fmaf(bprev, momentum, g);
    p = fmaf(-lr, b, p);                          // param.add_(buf, alpha=-lr)
    return b;
}

// One element, in the order of torch's _single_tensor_adam (decoupled decay).  Every operation is spelled as an
// intrinsic with one rounding (no contraction left to the compiler), so the float4 body and the scalar body give
// the same bits for the same element.
__device__ __forceinline__ void adamw_one(float& p, const float g, float& m, float& v, const AdamK k) {
    const float p1 = __fmul_rn(p, k.decay);                                  // p.mul_(1 - lr*wd)
    const float diff = __fsub_rn(g, m);                                      // m.lerp_(g, 1 - beta1), ATen's two forms
    const float m1 = (k.w1 < 0.5f) ? fmaf(k.w1, diff, m) : fmaf(-__fsub_rn(1.f, k.w1), diff, g);
    const float v1 = fmaf(k.omb2, __fmul_rn(g, g), __fmul_rn(k.beta2, v));   // v.mul_(beta2).addcmul_(g, g, 1 - beta2)
    const float denom = __fadd_rn(__fdiv_rn(__fsqrt_rn(v1), k.bc2_sqrt), k.eps);
    p = fmaf(-k.step, __fdiv_rn(m1, denom), p1);                             // p.addcdiv_(m, denom, value=-step)
    m = m1;
    v = v1;
}

// torch.lerp(a, b, w) for w < 0.5 (ATen's first form), the only one an EMA with 0.5 < decay < 1 can take
__device__ __forceinline__ float lerp_small(const float a, const float b, const float w) {
    return fmaf(w, __fsub_rn(b, a), a);
}

// binary search: last entry with first_chunk <= chunk
template <class Entry>
__device__ __forceinline__ int find_entry(const Entry* __restrict__ table, const int n_tensors, const long long chunk) {
    int lo = 0, hi = n_tensors - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if (table[mid].first_chunk <= chunk) lo = mid; else hi = mid - 1;
    }
    return lo;
}

}  // namespace dcfp_optim
