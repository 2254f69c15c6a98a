// bilinear.h — PyTorch's bilinear index math (F.interpolate, mode='bilinear'), shared by upsample_ce.hip and resize.hip.
//
// Coordinate rules follow ATen's area_pixel_compute_scale / _source_index:
//   align_corners: scale = (in-1)/(out-1) (0 if out==1), src = scale*dst
//   otherwise    : scale = in/out,        src = max(scale*(dst+0.5)-0.5, 0)
//   i0 = (int)src, i1 = i0 + (i0 < in-1), l1 = src - i0, l0 = 1 - l1
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include <type_traits>

namespace dcfp_bilinear {

struct Lerp {
    int i0, i1;
    float l0, l1;
};

template <bool ALIGN>
__device__ __forceinline__ Lerp lerp_of(int dst, float scale, int in_size) {
    float src;
    if (ALIGN) {
        src = scale * (float)dst;
    } else {
        src = scale * ((float)dst + 0.5f) - 0.5f;
        src = src < 0.f ? 0.f : src;
    }
    Lerp r;
    int i0 = (int)src;
    if (i0 > in_size - 1) i0 = in_size - 1;
    r.i0 = i0;
    r.i1 = i0 + ((i0 < in_size - 1) ? 1 : 0);
    float l1 = src - (float)i0;
    l1 = l1 < 0.f ? 0.f : (l1 > 1.f ? 1.f : l1);
    r.l1 = l1;
    r.l0 = 1.f - l1;
    return r;
}

inline float host_scale(int in, int out, int align) {
    if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
    return (float)in / (float)out;
}

// The host's align_corners flag as the kernels' ALIGN template argument: f(std::true_type{}) or f(std::false_type{}),
//     with_align(align_corners, [&](auto A) { hipLaunchKernelGGL(kernel<A.value>, ...); });
template <class F>
inline void with_align(int align_corners, F&& f) {
    if (align_corners)
        f(std::true_type{});
    else
        f(std::false_type{});
}

// Conservative [lo, hi] range of destination indices whose taps may include source cell i.
template <bool ALIGN>
__device__ __forceinline__ void dst_range(int i, float scale, int out_size, int& lo, int& hi) {
    if (!(scale > 0.f)) {  // out_size == 1 under align_corners
        lo = 0;
        hi = out_size - 1;
        return;
    }
    float a, b;
    if (ALIGN) {
        a = ((float)i - 1.f) / scale;
        b = ((float)i + 1.f) / scale;
    } else {
        a = ((float)i - 0.5f) / scale - 0.5f;
        b = ((float)i + 1.5f) / scale - 0.5f;
    }
    int l = (int)floorf(a) - 1, h = (int)ceilf(b) + 1;
    lo = l < 0 ? 0 : l;
    hi = h > out_size - 1 ? out_size - 1 : h;
}

__device__ __forceinline__ float tap_weight(const Lerp& L, int i) {
    return (L.i0 == i ? L.l0 : 0.f) + (L.i1 == i ? L.l1 : 0.f);
}

}  // namespace dcfp_bilinear
