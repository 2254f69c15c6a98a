// boundary.hip — label-map boundary transform of the Boundary-IoU metric.
//
//   valid(p)    : 0 <= L[p] < C
//   interior(p) : valid(p) and every pixel of the (2d+1)x(2d+1) window centred on p is inside the image
//                 and carries L[p]
//   out[p]      = valid(p) && !interior(p) ? L[p] : background
//
// Two launches; no window walk, no d sweeps over the image and no per-class pass.  Labels are read twice and the output
// written once whatever d and C are; the one term that grows with d is the column pass's warm-up over one-byte keys:
//   row pass    : one workgroup per image row.  A forward sweep over 1024-pixel chunks finds the start of the run
//                 of equal valid labels through every pixel (prefix maximum of change positions: serial over a
//                 lane's 4 pixels, cross-lane over the wave, one LDS step over the 4 waves, a register carried from
//                 chunk to chunk) and writes the one-byte key "label if the run reaches d to the left, else 255".
//                 Filtering only ever shortens a run at its left end, so the backward sweep can find the run end on
//                 the filtered keys; it writes key = label if the run reaches d to both sides (rowok), else 255.
//   column pass : one wave per (128 columns, 16 rows); a lane owns 2 adjacent columns, i.e. one 16-bit word of
//                 keys per row.  The band's own key words are loaded once and stay in registers.  The wave walks down
//                 from min(d, y0) rows above its band with the length of the vertical run of equal keys in a register
//                 and keeps "reaches d up" as one bit per row, walks up from min(d, ..) rows below the band for
//                 "reaches d down", and emits the band's rows on the way.  The warm-up rows read keys only.  Band and
//                 columns per lane are the fastest of {16, 32} x {2, 4} at 4 x 1024 x 2048, d = 46.
// No atomics, every output element is stored once, images never share a row or a band.
#include "common.h"

namespace {

constexpr int kRowThreads = 256;
constexpr int kPix = 4;                          // pixels per lane and step: 16 bytes of int32, 32 of int64
constexpr int kChunk = kRowThreads * kPix;
constexpr int kBand = 16;                        // rows per column-pass wave: one bit per row in a register
constexpr int kColPix = 2;                       // columns per lane of the column pass
constexpr unsigned kNoKey = 255u;

__host__ __device__ inline long long pitch_of(int W) { return ((long long)W + 3) & ~3LL; }

template <typename T, int P> struct Vec;          // P adjacent labels, moved as 8- or 16-byte vectors
template <> struct Vec<int32_t, 4> {
    int32_t v[4];
    __device__ void load(const int32_t* p) {
        const int4 t = *reinterpret_cast<const int4*>(p);
        v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w;
    }
    __device__ void store(int32_t* p) const { *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]); }
};
template <> struct Vec<int64_t, 4> {
    int64_t v[4];
    __device__ void load(const int64_t* p) {
        const longlong2 a = *reinterpret_cast<const longlong2*>(p), b = *reinterpret_cast<const longlong2*>(p + 2);
        v[0] = a.x; v[1] = a.y; v[2] = b.x; v[3] = b.y;
    }
    __device__ void store(int64_t* p) const {
        *reinterpret_cast<longlong2*>(p) = make_longlong2(v[0], v[1]);
        *reinterpret_cast<longlong2*>(p + 2) = make_longlong2(v[2], v[3]);
    }
};
template <> struct Vec<int32_t, 2> {
    int32_t v[2];
    __device__ void load(const int32_t* p) {
        const int2 t = *reinterpret_cast<const int2*>(p);
        v[0] = t.x; v[1] = t.y;
    }
    __device__ void store(int32_t* p) const { *reinterpret_cast<int2*>(p) = make_int2(v[0], v[1]); }
};
template <> struct Vec<int64_t, 2> {
    int64_t v[2];
    __device__ void load(const int64_t* p) {
        const longlong2 t = *reinterpret_cast<const longlong2*>(p);
        v[0] = t.x; v[1] = t.y;
    }
    __device__ void store(int64_t* p) const { *reinterpret_cast<longlong2*>(p) = make_longlong2(v[0], v[1]); }
};

template <typename T> __device__ __forceinline__ unsigned key_of(T l, int C) {
    return (l >= (T)0 && l < (T)C) ? (unsigned)l : kNoKey;
}

// the P labels of a row from column x0 on (x0 a multiple of P); columns >= W read as -1 (invalid)
template <typename T, int P, bool ALIGNED>
__device__ __forceinline__ void load_labels(const T* row, int x0, int W, Vec<T, P>& r) {
    if (ALIGNED && x0 < W) {                      // W % 4 == 0: the P are inside together
        r.load(row + x0);
    } else {
#pragma unroll
        for (int i = 0; i < P; ++i) r.v[i] = (!ALIGNED && x0 + i < W) ? row[x0 + i] : (T)-1;
    }
}

__device__ __forceinline__ int wave_prefix_max(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_up(v, off, 64);
        if (lane >= off) v = max(v, t);
    }
    return v;
}
__device__ __forceinline__ int wave_suffix_min(int v, int lane) {
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int t = __shfl_down(v, off, 64);
        if (lane + off < 64) v = min(v, t);
    }
    return v;
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(kRowThreads) void boundary_row_kernel(const T* __restrict__ labels, uint8_t* half,
                                                                   uint8_t* __restrict__ keys, int W, int C, int d) {
    __shared__ int sm[2][4];
    const long long r = blockIdx.x;               // n*H + y: every row stands alone, so images never mix
    const long long Wp = pitch_of(W);
    const T* row = labels + r * W;
    uint8_t* hrow = half + r * Wp;
    uint8_t* krow = keys + r * Wp;
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int nchunks = (W + kChunk - 1) / kChunk;

    // ---- forward: start of the run through every pixel
    int carry = -1;
    for (int j = 0; j < nchunks; ++j) {
        const int x0 = j * kChunk + tid * kPix;
        Vec<T, kPix> l;
        load_labels<T, kPix, ALIGNED>(row, x0, W, l);
        unsigned k[kPix];
#pragma unroll
        for (int i = 0; i < kPix; ++i) k[i] = key_of<T>(l.v[i], C);
        unsigned prev = (x0 > 0 && x0 <= W) ? key_of<T>(row[x0 - 1], C) : kNoKey;
        int s[kPix], run = -1;
#pragma unroll
        for (int i = 0; i < kPix; ++i) {          // a pixel opens a run if it differs from its left neighbour
            if (k[i] == kNoKey || k[i] != prev) run = x0 + i;
            s[i] = run;
            prev = k[i];
        }
        const int incl = wave_prefix_max(run, lane);
        int excl = __shfl_up(incl, 1, 64);
        if (lane == 0) excl = -1;
        if (lane == 63) sm[j & 1][wid] = incl;
        __syncthreads();
        int before = carry;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = sm[j & 1][w];
            if (w < wid) before = max(before, t);
            carry = max(carry, t);
        }
        before = max(before, excl);
        unsigned word = 0;
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            const int start = max(s[i], before);
            const bool ok = k[i] != kNoKey && (x0 + i) - start >= d;
            word |= (ok ? k[i] : kNoKey) << (8 * i);
        }
        if (x0 < W) *reinterpret_cast<uint32_t*>(hrow + x0) = word;
    }
    __syncthreads();                               // the half-filtered row is read back by other lanes below

    // ---- backward: end of the run, on the keys the forward sweep left
    carry = 0x7fffffff;
    for (int j = nchunks - 1; j >= 0; --j) {
        const int x0 = j * kChunk + tid * kPix;
        const unsigned word = (x0 < W) ? *reinterpret_cast<const uint32_t*>(hrow + x0) : 0xffffffffu;
        unsigned next = (x0 + kPix < W) ? (unsigned)hrow[x0 + kPix] : kNoKey;
        unsigned k[kPix];
        int e[kPix], run = 0x7fffffff;
#pragma unroll
        for (int i = kPix - 1; i >= 0; --i) {      // a pixel closes a run if it differs from its right neighbour
            k[i] = (word >> (8 * i)) & 0xffu;
            if (k[i] == kNoKey || k[i] != next) run = x0 + i;
            e[i] = run;
            next = k[i];
        }
        const int incl = wave_suffix_min(run, lane);
        int excl = __shfl_down(incl, 1, 64);
        if (lane == 63) excl = 0x7fffffff;
        const int slot = (nchunks - 1 - j) & 1;
        if (lane == 0) sm[slot][wid] = incl;
        __syncthreads();
        int after = carry;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int t = sm[slot][w];
            if (w > wid) after = min(after, t);
            carry = min(carry, t);
        }
        after = min(after, excl);
        unsigned out = 0;
#pragma unroll
        for (int i = 0; i < kPix; ++i) {
            const int end = min(e[i], after);
            const bool ok = k[i] != kNoKey && end - (x0 + i) >= d;
            out |= (ok ? k[i] : kNoKey) << (8 * i);
        }
        if (x0 < W) *reinterpret_cast<uint32_t*>(krow + x0) = out;
    }
}

// the keys of kColPix adjacent columns of one row (columns past W, inside the pitch, hold no key)
__device__ __forceinline__ unsigned load_keys(const uint8_t* p) {
    if (kColPix == 4) return *reinterpret_cast<const uint32_t*>(p);
    return *reinterpret_cast<const uint16_t*>(p);
}

// one row further along a column walk: cnt = length of the run of equal keys that ends at this row (this row included)
__device__ __forceinline__ void col_step(unsigned word, unsigned (&prev)[kColPix], int (&cnt)[kColPix]) {
#pragma unroll
    for (int i = 0; i < kColPix; ++i) {
        const unsigned k = (word >> (8 * i)) & 0xffu;
        cnt[i] = (k == prev[i]) ? cnt[i] + 1 : 1;   // at most d + kBand rows are walked: no cap needed
        prev[i] = k;
    }
}

template <typename T, bool ALIGNED>
__global__ __launch_bounds__(64) void boundary_col_kernel(const T* __restrict__ labels, const uint8_t* __restrict__ keys,
                                                          T* __restrict__ out, int H, int W, int C, int d,
                                                          int background, int colgroups, int bands) {
    constexpr int kGroup = 8;                       // label rows loaded together on the way up
    const long long Wp = pitch_of(W);
    long long b = blockIdx.x;
    const int cg = (int)(b % colgroups); b /= colgroups;
    const int band = (int)(b % bands);
    const long long n = b / bands;
    const int x0 = (cg * 64 + (int)threadIdx.x) * kColPix;
    if (x0 >= W) return;
    const int y0 = band * kBand, y1 = min(y0 + kBand, H);
    const uint8_t* kcol = keys + n * H * Wp + x0;
    const int need = d + 1;                         // run length, the pixel included, that reaches d rows away

    // the band's own keys stay in registers for both walks: one word per row, all loads in flight together
    unsigned kw[kBand];
#pragma unroll
    for (int j = 0; j < kBand; ++j)
        kw[j] = (y0 + j < H) ? load_keys(kcol + (y0 + j) * Wp) : ~0u;

    // ---- down: bit j of up[i] = the run of equal keys through (y0+j, x0+i) reaches d rows up
    unsigned up[kColPix], prev[kColPix];
    int cnt[kColPix];
#pragma unroll
    for (int i = 0; i < kColPix; ++i) { up[i] = 0u; prev[i] = kNoKey; cnt[i] = 0; }
#pragma unroll 8
    for (int y = max(0, y0 - d); y < y0; ++y)       // warm-up: keys only
        col_step(load_keys(kcol + y * Wp), prev, cnt);
#pragma unroll
    for (int j = 0; j < kBand; ++j) {               // (rows past the image carry no key: their bits stay 0)
        col_step(kw[j], prev, cnt);
#pragma unroll
        for (int i = 0; i < kColPix; ++i)
            if (prev[i] != kNoKey && cnt[i] >= need) up[i] |= 1u << j;
    }
    // ---- up: the same towards the bottom; the band's rows are emitted as they are passed
#pragma unroll
    for (int i = 0; i < kColPix; ++i) { prev[i] = kNoKey; cnt[i] = 0; }
#pragma unroll 8
    for (int y = (int)min((long long)H - 1, (long long)y1 - 1 + d); y >= y1; --y)
        col_step(load_keys(kcol + y * Wp), prev, cnt);
    const T* lrow = labels + n * H * W;             // row pointers: load4 adds x0
    T* ocol = out + n * H * W + x0;
#pragma unroll
    for (int g = kBand / kGroup - 1; g >= 0; --g) {
        if (y0 + g * kGroup >= H) continue;         // the same in every lane
        Vec<T, kColPix> l[kGroup];
#pragma unroll
        for (int r = 0; r < kGroup; ++r) {
            const int y = y0 + g * kGroup + r;
            if (y < H) load_labels<T, kColPix, ALIGNED>(lrow + (long long)y * W, x0, W, l[r]);
        }
#pragma unroll
        for (int r = kGroup - 1; r >= 0; --r) {
            const int j = g * kGroup + r, y = y0 + j;
            if (y >= H) continue;
            col_step(kw[j], prev, cnt);
#pragma unroll
            for (int i = 0; i < kColPix; ++i) {
                const bool interior = prev[i] != kNoKey && cnt[i] >= need && ((up[i] >> j) & 1u);
                const T v = l[r].v[i];
                l[r].v[i] = (v >= (T)0 && v < (T)C && !interior) ? v : (T)background;
            }
            const long long off = (long long)y * W;
            if (ALIGNED) {
                l[r].store(ocol + off);
            } else {
#pragma unroll
                for (int i = 0; i < kColPix; ++i)
                    if (x0 + i < W) ocol[off + i] = l[r].v[i];
            }
        }
    }
}

template <typename T>
int label_boundary(const T* labels, T* out, int N, int H, int W, int num_classes, int d, int background, void* ws,
                   size_t ws_bytes, dcfp_stream_t stream) {
    if (!labels || !out || !ws || N <= 0 || H <= 0 || W <= 0 || d < 1 || num_classes < 1 ||
        static_cast<const void*>(labels) == static_cast<const void*>(out) || (reinterpret_cast<uintptr_t>(ws) & 3u) ||
        ws_bytes < dcfp_label_boundary_workspace_bytes(N, H, W))
        return DCFP_E_BADDESC;
    if (num_classes > 255) return DCFP_E_UNSUPPORTED;
    const long long rows = (long long)N * H, Wp = pitch_of(W);
    const int colgroups = (int)((Wp / kColPix + 63) / 64), bands = (H + kBand - 1) / kBand;
    const long long colblocks = (long long)N * bands * colgroups;
    if (rows > 0x7fffffffLL || colblocks > 0x7fffffffLL) return DCFP_E_UNSUPPORTED;
    // no window reaches further than the image: a larger d marks every valid pixel, as max(H, W) already does
    const int dd = d < (H > W ? H : W) ? d : (H > W ? H : W);
    uint8_t* half = static_cast<uint8_t*>(ws);
    uint8_t* keys = half + rows * Wp;
    const bool aligned = W % kPix == 0 && dcfp_aligned16(labels) && dcfp_aligned16(out);
    if (aligned) {
        hipLaunchKernelGGL((boundary_row_kernel<T, true>), dim3((unsigned)rows), dim3(kRowThreads), 0, dcfp_s(stream),
                           labels, half, keys, W, num_classes, dd);
        hipLaunchKernelGGL((boundary_col_kernel<T, true>), dim3((unsigned)colblocks), dim3(64), 0, dcfp_s(stream),
                           labels, keys, out, H, W, num_classes, dd, background, colgroups, bands);
    } else {
        hipLaunchKernelGGL((boundary_row_kernel<T, false>), dim3((unsigned)rows), dim3(kRowThreads), 0, dcfp_s(stream),
                           labels, half, keys, W, num_classes, dd);
        hipLaunchKernelGGL((boundary_col_kernel<T, false>), dim3((unsigned)colblocks), dim3(64), 0, dcfp_s(stream),
                           labels, keys, out, H, W, num_classes, dd, background, colgroups, bands);
    }
    DCFP_RETURN_LAUNCH();
}

}  // namespace

extern "C" size_t dcfp_label_boundary_workspace_bytes(int N, int H, int W) {
    if (N <= 0 || H <= 0 || W <= 0) return 0;
    return (size_t)2 * (size_t)N * (size_t)H * (size_t)pitch_of(W);   // the half-filtered keys and the key map
}

extern "C" int dcfp_label_boundary_i32(const int32_t* labels, int32_t* out, int N, int H, int W, int num_classes,
                                       int d, int background, void* ws, size_t ws_bytes, dcfp_stream_t stream) {
    return label_boundary<int32_t>(labels, out, N, H, W, num_classes, d, background, ws, ws_bytes, stream);
}

extern "C" int dcfp_label_boundary_i64(const int64_t* labels, int64_t* out, int N, int H, int W, int num_classes,
                                       int d, int background, void* ws, size_t ws_bytes, dcfp_stream_t stream) {
    return label_boundary<int64_t>(labels, out, N, H, W, num_classes, d, background, ws, ws_bytes, stream);
}
