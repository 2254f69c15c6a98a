// upsample_logits.h — one destination pixel of the bilinearly upsampled logits: its stencil, a class's interpolated
// logit and the running log-sum-exp over the classes.  Shared by upsample_ce.hip and lovasz.hip, so the losses, their
// backwards and the evaluation kernels all form z and lse with the same expressions.
//
// Floating-point contraction is fixed where an expression is parsed: a file that turns it off (lovasz.hip) includes this
// header after its pragma, and every expression below then compiles without FMAs there.
#pragma once
#include "bilinear.h"

namespace dcfp_bilinear {

// (image, row, column) of a full-resolution pixel index
struct Pix {
    int n, Y, X;
};

__device__ __forceinline__ Pix pix_of(long long pix, int H, int W) {
    Pix r;
    r.X = (int)(pix % W);
    const long long t = pix / W;
    r.Y = (int)(t % H);
    r.n = (int)(t / H);
    return r;
}

// the stencil of a destination pixel: four offsets into a class plane and the four lerp factors
struct Tap {
    int o00, o01, o10, o11;
    float h0, h1, w0, w1;
};

__device__ __forceinline__ Tap tap_of(const Lerp& Lh, const Lerp& Lw, int w) {
    Tap t;
    t.o00 = Lh.i0 * w + Lw.i0; t.o01 = Lh.i0 * w + Lw.i1;
    t.o10 = Lh.i1 * w + Lw.i0; t.o11 = Lh.i1 * w + Lw.i1;
    t.h0 = Lh.l0; t.h1 = Lh.l1; t.w0 = Lw.l0; t.w1 = Lw.l1;
    return t;
}

// THE interpolation expression, from the four stencil values of a class: it does not matter whether a kernel reads
// them from the class plane or holds them in registers
__device__ __forceinline__ float logit_of(float v00, float v01, float v10, float v11, float h0, float h1, float w0,
                                          float w1) {
    return h0 * (w0 * v00 + w1 * v01) + h1 * (w0 * v10 + w1 * v11);
}

__device__ __forceinline__ float logit_at(const float* __restrict__ p, const Tap& t) {
    return logit_of(p[t.o00], p[t.o01], p[t.o10], p[t.o11], t.h0, t.h1, t.w0, t.w1);
}

// one step of the running log-sum-exp: m is the largest logit so far, s the sum of exp(z - m); lse = m + logf(s)
__device__ __forceinline__ void lse_step(float z, float& m, float& s) {
    if (z > m) {
        s = s * expf(m - z) + 1.f;
        m = z;
    } else {
        s += expf(z - m);
    }
}

// log-sum-exp of the pixel's C interpolated logits
__device__ __forceinline__ float lse_at(const float* __restrict__ base, long long plane, int C, const Tap& t) {
    float m = -INFINITY, s = 0.f;
    for (int c = 0; c < C; ++c) lse_step(logit_at(base + c * plane, t), m, s);
    return m + logf(s);
}

}  // namespace dcfp_bilinear
