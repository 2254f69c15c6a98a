// augment.hip — the training-time data augmentation of the reference's datasets/Base.py:224-261 on the device
// (DESIGN §13): uint8 BGR sources + uint8 raw-id label maps -> normalised fp32 NCHW crops, int64 trainId crops, a
// per-sample class histogram and (second kernel) the per-crop class-balance weight of get_label.
//
// The geometry (random scale, pad, crop, mirror) never reaches the device as coordinates: the host folds it into one
// column table [crop_w] and one row table [crop_h] per sample (DcfpAugTap: source index or -1 for padding, the two
// 11-bit interpolation coefficients, the nearest-neighbour label index).  The image path of one output pixel is
//   u8   = (((b0*(h0>>4))>>16) + ((b1*(h1>>4))>>16) + 2) >> 2,   h = S[sx]*a0 + S[sx+1]*a1 on the two source rows
//   u8   = LUT A[u8]                              brightness (+ contrast when it runs before the HSV block)
//   bgr  = HSV block(bgr)                          only when saturation or hue fired: fp32, one rounding per operation
//   f32  = LUT B[c][u8]                            (contrast when it runs last +) BGR->RGB, /255, -mean, /std
// so everything but the HSV block is integer arithmetic and table lookups, and the HSV block is written one IEEE
// operation per statement with contraction off: the result is defined bit for bit.
//
// One launch covers up to kMaxSamples samples of different source sizes (records by value in the kernel argument);
// blockIdx.z picks the sample.  A lane produces 4 adjacent pixels of one output row: three 16-byte fp32 stores and two
// 16-byte int64 stores.  Source reads are bytes (the gather is irregular by construction; the L1 absorbs the re-reads
// of neighbouring taps).  The histogram is 256 LDS bins per block, one global atomic per non-empty bin and block.
#include "common.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxSamples = 16;                  // records per launch: 16 x 64 bytes of kernel argument
constexpr int kPix = 4;                          // output pixels per lane
constexpr int kRows = 4;                         // output rows per block (blockDim = 64 x kRows)

struct AugBatch { DcfpAugSample s[kMaxSamples]; };

__device__ __forceinline__ float clip_u8(float v) { return fminf(fmaxf(v, 0.0f), 255.0f); }

// BGR -> HSV (H in 0..179, S and V in 0..255, all integers held in fp32), the two jitters, HSV -> BGR.  Every line is
// one correctly rounded fp32 operation; tests/_augment_ref.py states the same lines in numpy float32.
__device__ __forceinline__ void hsv_block(int& b8, int& g8, int& r8, int flags, float sat_alpha, int hue_delta) {
#pragma clang fp contract(off)
    const float b = (float)b8, g = (float)g8, r = (float)r8;
    const float V = fmaxf(fmaxf(r, g), b);
    const float m = fminf(fminf(r, g), b);
    const float d = V - m;
    float S = 0.0f;
    if (V != 0.0f) {
        const float n = 255.0f * d;
        const float q = n / V;
        S = rintf(q);
    }
    float H = 0.0f;
    if (d != 0.0f) {
        if (V == r) {
            const float n = 30.0f * (g - b);
            H = n / d;
        } else if (V == g) {
            const float n = 30.0f * (b - r);
            const float q = n / d;
            H = 60.0f + q;
        } else {
            const float n = 30.0f * (r - g);
            const float q = n / d;
            H = 120.0f + q;
        }
        if (H < 0.0f) H = H + 180.0f;
        H = rintf(H);
        if (H == 180.0f) H = 0.0f;
    }
    if (flags & DCFP_AUG_SATURATION) {
        const float t = S * sat_alpha;
        S = clip_u8(rintf(t));
    }
    if (flags & DCFP_AUG_HUE) {
        H = H + (float)hue_delta;               // integers of magnitude < 256: exact
        if (H < 0.0f) H = H + 180.0f;
        if (H >= 180.0f) H = H - 180.0f;
    }
    const float s = S / 255.0f;
    const float h6 = H / 30.0f;
    const float fi = floorf(h6);
    const float f = h6 - fi;
    const float oms = 1.0f - s;
    const float p = V * oms;
    const float sf = s * f;
    const float omsf = 1.0f - sf;
    const float q = V * omsf;
    const float omf = 1.0f - f;
    const float st = s * omf;
    const float omst = 1.0f - st;
    const float t = V * omst;
    const int i = (int)fi;
    float R, G, B;
    switch (i) {
        case 0: R = V; G = t; B = p; break;
        case 1: R = q; G = V; B = p; break;
        case 2: R = p; G = V; B = t; break;
        case 3: R = p; G = q; B = V; break;
        case 4: R = t; G = p; B = V; break;
        default: R = V; G = p; B = q; break;
    }
    b8 = (int)clip_u8(rintf(B));
    g8 = (int)clip_u8(rintf(G));
    r8 = (int)clip_u8(rintf(R));
}

template <bool VEC>
__global__ __launch_bounds__(64 * kRows) void augment_kernel(AugBatch batch, const int4* __restrict__ taps,
                                                            const uint8_t* __restrict__ lut_a,
                                                            const float* __restrict__ lut_b,
                                                            const uint8_t* __restrict__ id_table, int n0, int ch, int cw,
                                                            int ignore_label, float* __restrict__ images,
                                                            int64_t* __restrict__ labels, int* __restrict__ hist) {
    __shared__ float sB[3 * 256];
    __shared__ int bins[256];
    __shared__ uint8_t sA[256];
    __shared__ uint8_t sId[256];
    const DcfpAugSample& s = batch.s[blockIdx.z];
    const int n = n0 + (int)blockIdx.z;
    const int tid = (int)(threadIdx.y * 64 + threadIdx.x);
    {
        const float* lb = lut_b + s.lut_b_off;
        sB[tid] = lb[tid];
        sB[256 + tid] = lb[256 + tid];
        sB[512 + tid] = lb[512 + tid];
        sA[tid] = s.lut_a_off >= 0 ? lut_a[s.lut_a_off + tid] : (uint8_t)tid;
        sId[tid] = id_table ? id_table[tid] : (uint8_t)tid;
        bins[tid] = 0;
    }
    __syncthreads();

    const int x0 = ((int)blockIdx.x * 64 + (int)threadIdx.x) * kPix;
    const int y = (int)blockIdx.y * kRows + (int)threadIdx.y;
    if (x0 < cw && y < ch) {
        const int W = s.src_w, H = s.src_h;
        const int4 row = taps[s.row_off + y];          // .x source row or -1, .y / .z coefficients, .w label row
        const int sy0 = min(row.x, H - 1), sy1 = min(sy0 + 1, H - 1);
        const int ly = min(max(row.w, 0), H - 1);
        float o[3][kPix];
        int64_t lab[kPix];
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            const int x = x0 + i;
            o[0][i] = o[1][i] = o[2][i] = 0.0f;      // padding: zeros after normalisation (Base.py:184-201)
            lab[i] = ignore_label;
            if (x >= cw) continue;
            const int4 col = taps[s.col_off + x];
            if (col.x < 0 || row.x < 0) continue;
            const int sx0 = min(col.x, W - 1), sx1 = min(sx0 + 1, W - 1);
            const uint8_t* p00 = s.image + ((long long)sy0 * W + sx0) * 3;
            const uint8_t* p01 = s.image + ((long long)sy0 * W + sx1) * 3;
            const uint8_t* p10 = s.image + ((long long)sy1 * W + sx0) * 3;
            const uint8_t* p11 = s.image + ((long long)sy1 * W + sx1) * 3;
            int px[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int h0 = (int)p00[c] * col.y + (int)p01[c] * col.z;
                const int h1 = (int)p10[c] * col.y + (int)p11[c] * col.z;
                const int v = (((row.y * (h0 >> 4)) >> 16) + ((row.z * (h1 >> 4)) >> 16) + 2) >> 2;
                px[c] = (int)sA[min(max(v, 0), 255)];
            }
            if (s.hsv_flags) hsv_block(px[0], px[1], px[2], s.hsv_flags, s.sat_alpha, s.hue_delta);
            o[0][i] = sB[px[2]];                     // plane 0 = R
            o[1][i] = sB[256 + px[1]];
            o[2][i] = sB[512 + px[0]];
            if (labels) {
                const int lx = min(max(col.w, 0), W - 1);
                lab[i] = (int64_t)sId[s.label[(long long)ly * W + lx]];
            }
        }
        const long long plane = (long long)ch * cw;
        const long long at = (long long)y * cw + x0;
        float* img = images + (long long)n * 3 * plane + at;
        if (VEC) {
#pragma unroll
            for (int c = 0; c < 3; ++c)
                *reinterpret_cast<float4*>(img + c * plane) = make_float4(o[c][0], o[c][1], o[c][2], o[c][3]);
        } else {
#pragma unroll
            for (int c = 0; c < 3; ++c)
#pragma unroll
                for (int i = 0; i < kPix; ++i)
                    if (x0 + i < cw) img[c * plane + i] = o[c][i];
        }
        if (labels) {
            int64_t* lp = labels + (long long)n * plane + at;
            if (VEC) {
                *reinterpret_cast<longlong2*>(lp) = make_longlong2(lab[0], lab[1]);
                *reinterpret_cast<longlong2*>(lp + 2) = make_longlong2(lab[2], lab[3]);
            } else {
#pragma unroll
                for (int i = 0; i < kPix; ++i)
                    if (x0 + i < cw) lp[i] = lab[i];
            }
            // label maps are piecewise constant: one LDS atomic per run of equal labels among the lane's pixels
            int run = 0, cur = -1;
#pragma unroll
            for (int i = 0; i < kPix; ++i) {
                if (x0 + i >= cw) break;
                const int l = (int)lab[i] & 255;
                if (l != cur) {
                    if (run) atomicAdd(&bins[cur], run);
                    cur = l;
                    run = 0;
                }
                ++run;
            }
            if (run) atomicAdd(&bins[cur], run);
        }
    }
    if (hist) {
        __syncthreads();
        const int c = bins[tid];
        if (c) atomicAdd(&hist[(long long)n * 256 + tid], c);
    }
}

// get_label (Base.py:73-89): the class weights of one sample from its histogram in fp64, then weight = w[label]
template <bool VEC>
__global__ __launch_bounds__(256) void balance_weight_kernel(const int64_t* __restrict__ labels,
                                                             const int* __restrict__ hist,
                                                             const int* __restrict__ target, int balance, int C,
                                                             int ignore_label, double beta, long long P,
                                                             float* __restrict__ weight) {
    __shared__ float w[256];
    const int n = (int)blockIdx.y, tid = (int)threadIdx.x;
    {
        const int* h = hist + (long long)n * 256;
        double wd = 0.0;
        if (tid < C && tid != ignore_label) {
            const double nc = (double)h[tid];
            if (balance == 1) {
                wd = 1.0 / (nc + 1.0);
            } else {
                const int t = target[n];
                if (t >= 0 && t < C && t != ignore_label) {   // (no target class: the sample gets weight 0)
                    const double num = (1.0 + 1e-8) - pow(beta, (double)h[t]);
                    const double den = (1.0 + 1e-8) - pow(beta, nc);
                    wd = num / den;
                }
            }
            wd = fmin(fmax(wd, 0.0), 1.0);
        }
        w[tid] = (float)wd;
    }
    __syncthreads();
    const int64_t* lab = labels + (long long)n * P;
    float* out = weight + (long long)n * P;
    const long long stride = (long long)gridDim.x * 256;
    if (VEC) {
        for (long long i = (long long)blockIdx.x * 256 + tid; i < P / 4; i += stride) {
            const longlong2 a = *reinterpret_cast<const longlong2*>(lab + 4 * i);
            const longlong2 b = *reinterpret_cast<const longlong2*>(lab + 4 * i + 2);
            const long long l[4] = {a.x, a.y, b.x, b.y};
            float v[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = (l[k] >= 0 && l[k] < 256) ? w[l[k]] : 0.0f;
            *reinterpret_cast<float4*>(out + 4 * i) = make_float4(v[0], v[1], v[2], v[3]);
        }
    } else {
        for (long long i = (long long)blockIdx.x * 256 + tid; i < P; i += stride) {
            const long long l = lab[i];
            out[i] = (l >= 0 && l < 256) ? w[l] : 0.0f;
        }
    }
}

}  // namespace

extern "C" int dcfp_augment_u8_to_f32_nchw(const DcfpAugSample* samples, int N, int crop_h, int crop_w,
                                           const DcfpAugTap* taps, int64_t n_taps, const uint8_t* lut_a,
                                           int64_t lut_a_bytes, const float* lut_b, int64_t lut_b_floats,
                                           const uint8_t* id_table, int ignore_label, float* images, int64_t* labels,
                                           int32_t* hist, dcfp_stream_t stream) {
    if (!samples || N <= 0 || crop_h <= 0 || crop_w <= 0 || !taps || !lut_b || !images || (hist && !labels) ||
        ignore_label < 0 || ignore_label > 255 || (reinterpret_cast<uintptr_t>(taps) & 15u) ||
        (reinterpret_cast<uintptr_t>(images) & 3u) || (labels && (reinterpret_cast<uintptr_t>(labels) & 7u)))
        return DCFP_E_BADDESC;
    for (int i = 0; i < N; ++i) {
        const DcfpAugSample& s = samples[i];
        if (!s.image || (labels && !s.label) || s.src_h <= 0 || s.src_w <= 0 ||
            (long long)s.src_h * s.src_w > 0x7fffffffLL / 3 ||
            s.col_off < 0 || (long long)s.col_off + crop_w > n_taps ||
            s.row_off < 0 || (long long)s.row_off + crop_h > n_taps ||
            s.lut_b_off < 0 || (long long)s.lut_b_off + 768 > lut_b_floats ||
            (s.lut_a_off >= 0 && (!lut_a || (long long)s.lut_a_off + 256 > lut_a_bytes)) ||
            (s.hsv_flags & ~(DCFP_AUG_SATURATION | DCFP_AUG_HUE)) || s.hue_delta < -180 || s.hue_delta > 180)
            return DCFP_E_BADDESC;
    }
    const long long gx = ((long long)crop_w + 64 * kPix - 1) / (64 * kPix), gy = ((long long)crop_h + kRows - 1) / kRows;
    if (gy > 65535 || (long long)N * 3 * crop_h * crop_w > (1LL << 40)) return DCFP_E_UNSUPPORTED;
    if (hist) {
        hipError_t e = hipMemsetAsync(hist, 0, (size_t)N * 256 * sizeof(int32_t), dcfp_s(stream));
        if (e != hipSuccess) return (int)e;
    }
    const bool vec = crop_w % kPix == 0 && dcfp_aligned16(images) && (!labels || dcfp_aligned16(labels));
    for (int n0 = 0; n0 < N; n0 += kMaxSamples) {
        const int cnt = N - n0 < kMaxSamples ? N - n0 : kMaxSamples;
        AugBatch batch;
        for (int i = 0; i < kMaxSamples; ++i) batch.s[i] = samples[n0 + (i < cnt ? i : 0)];
        const dim3 grid((unsigned)gx, (unsigned)gy, (unsigned)cnt), block(64, kRows);
        if (vec)
            hipLaunchKernelGGL((augment_kernel<true>), grid, block, 0, dcfp_s(stream), batch,
                               reinterpret_cast<const int4*>(taps), lut_a, lut_b, id_table, n0, crop_h, crop_w,
                               ignore_label, images, labels, hist);
        else
            hipLaunchKernelGGL((augment_kernel<false>), grid, block, 0, dcfp_s(stream), batch,
                               reinterpret_cast<const int4*>(taps), lut_a, lut_b, id_table, n0, crop_h, crop_w,
                               ignore_label, images, labels, hist);
    }
    DCFP_RETURN_LAUNCH();
}

extern "C" int dcfp_balance_weight_f32(const int64_t* labels, const int32_t* hist, const int32_t* target_class, int N,
                                       int64_t pixels, int num_classes, int ignore_label, int balance, double beta,
                                       float* weight, dcfp_stream_t stream) {
    if (balance < 0 || balance > 2 || N <= 0 || pixels <= 0 || num_classes < 1 || num_classes > 256) return DCFP_E_BADDESC;
    if (balance == 0) return DCFP_OK;              // get_label returns the plain label: nothing to compute
    if (!labels || !hist || !weight || (balance == 2 && (!target_class || !(beta > 0.0 && beta < 1.0))) || N > 65535 ||
        (reinterpret_cast<uintptr_t>(labels) & 7u) || (reinterpret_cast<uintptr_t>(weight) & 3u))
        return DCFP_E_BADDESC;
    const bool vec = pixels % 4 == 0 && dcfp_aligned16(labels) && dcfp_aligned16(weight);
    const long long items = vec ? pixels / 4 : pixels;
    long long gx = (items + 255) / 256;
    const long long cap = (long long)dcfp_num_cus() * 8;
    if (gx > cap) gx = cap;
    const dim3 grid((unsigned)gx, (unsigned)N);
    if (vec)
        hipLaunchKernelGGL((balance_weight_kernel<true>), grid, dim3(256), 0, dcfp_s(stream), labels, hist,
                           target_class, balance, num_classes, ignore_label, beta, (long long)pixels, weight);
    else
        hipLaunchKernelGGL((balance_weight_kernel<false>), grid, dim3(256), 0, dcfp_s(stream), labels, hist,
                           target_class, balance, num_classes, ignore_label, beta, (long long)pixels, weight);
    DCFP_RETURN_LAUNCH();
}
