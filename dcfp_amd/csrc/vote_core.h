// vote_core.h — what the fused evaluation votes (vote.hip, slide.hip) share: everything around "add the passes'
// contributions to a pixel's class scores".  One lane owns one output pixel; CHUNK classes are accumulated in registers
// at a time by the vote's own code, then stored (scores), compared (first maximum wins, like upsample_argmax_kernel)
// and, with labels, counted into the confusion matrix: per-block LDS bins while C*C <= kLdsBins, global 64-bit integer
// atomics above that.  The bin helpers also serve confusion_kernel / confusion_global_kernel (upsample_ce.hip), so the
// rule for a label outside the classes exists once.
#pragma once
#include "common.h"
#include <math.h>
#include <type_traits>

namespace dcfp_vote {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 256 * 8;
constexpr int kLdsBins = 4096;

// ---- confusion bins: hist holds lds_bins = C*C counters of the block, or lds_bins is 0 and conf is counted directly
__device__ __forceinline__ void bins_clear(unsigned int* hist, int lds_bins) {
    for (int i = threadIdx.x; i < lds_bins; i += kThreads) hist[i] = 0;
}

// one pixel of label g predicted as p (0 <= p < C); a label that is ignore_index or no class is skipped
__device__ __forceinline__ void bins_count(unsigned int* hist, int lds_bins, unsigned long long* conf, long long g, int p,
                                           int C, int ignore_index) {
    if (g != ignore_index && g >= 0 && g < C) {
        if (lds_bins) atomicAdd(&hist[(int)g * C + p], 1u);
        else atomicAdd(&conf[g * C + p], 1ull);
    }
}

// the block's bins into conf: one integer atomic per non-empty bin (every lane of the block arrives here)
__device__ __forceinline__ void bins_flush(const unsigned int* hist, int lds_bins, unsigned long long* conf) {
    if (!lds_bins) return;
    __syncthreads();
    for (int i = threadIdx.x; i < lds_bins; i += kThreads)
        if (hist[i]) atomicAdd(&conf[i], (unsigned long long)hist[i]);
}

// ---- the outputs of a vote: the top-left out_h x out_w crop of the voting grid; scores, pred and conf may be null
struct VoteOut {
    int N, C, out_h, out_w;
    float* scores;                  // [N,C,out_h,out_w]
    int* pred;                      // [N,out_h,out_w]
    const long long* gt;            // [N,out_h,out_w], read when conf is given
    int ignore_index;
    unsigned long long* conf;       // [C,C], accumulated
    int lds_bins;
};

// The pixel loop of a vote kernel.  acc_fn(float (&acc)[CHUNK], n, y, x, c0) adds every pass's contribution to the scores
// of classes c0 .. c0+CHUNK-1 (those below C) of pixel (n, y, x); acc comes zeroed.  hist: the block's cleared bins.
template <int CHUNK, class Accumulate>
__device__ __forceinline__ void vote_pixels(const VoteOut& o, unsigned int* hist, Accumulate acc_fn) {
    const int C = o.C, out_h = o.out_h, out_w = o.out_w;
    float* __restrict__ scores = o.scores;
    int* __restrict__ pred = o.pred;
    const long long total = (long long)o.N * out_h * out_w;
    const long long out_plane = (long long)out_h * out_w;
    for (long long pix = (long long)blockIdx.x * kThreads + threadIdx.x; pix < total;
         pix += (long long)gridDim.x * kThreads) {
        const int x = (int)(pix % out_w);
        const long long t = pix / out_w;
        const int y = (int)(t % out_h);
        const int n = (int)(t / out_h);
        float best = -INFINITY;
        int bi = 0;
        for (int c0 = 0; c0 < C; c0 += CHUNK) {
            float acc[CHUNK];
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) acc[j] = 0.f;
            acc_fn(acc, n, y, x, c0);
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) {
                if (c0 + j < C) {
                    if (scores) scores[((long long)n * C + c0 + j) * out_plane + (long long)y * out_w + x] = acc[j];
                    if (acc[j] > best) { best = acc[j]; bi = c0 + j; }     // first maximum wins
                }
            }
        }
        if (pred) pred[pix] = bi;
        if (o.conf) bins_count(hist, o.lds_bins, o.conf, o.gt[pix], bi, C, o.ignore_index);
    }
    bins_flush(hist, o.lds_bins, o.conf);
}

// ---- host side
// the checks of a vote's entry point on everything but its pass descriptors
inline bool vote_args_ok(int N, int C, int H, int W, int out_h, int out_w, const float* scores, const int32_t* pred,
                         const int64_t* gt, const int64_t* conf) {
    if (N <= 0 || C <= 0 || H <= 0 || W <= 0 || out_h <= 0 || out_w <= 0 || out_h > H || out_w > W) return false;
    if ((conf && !gt) || (!scores && !pred && !conf)) return false;
    return !(conf && C > 1024);         // as dcfp_confusion_matrix_i64
}

struct VoteLaunch {
    VoteOut out;
    unsigned blocks;
    size_t lds_bytes;       // dynamic LDS: extra_words in front, then the bins
};

inline VoteLaunch vote_launch(int N, int C, int out_h, int out_w, float* scores, int32_t* pred, const int64_t* gt,
                              int ignore_index, int64_t* conf, int extra_words) {
    const long long total = (long long)N * out_h * out_w;
    long long blocks = (total + kThreads - 1) / kThreads;
    if (blocks > kMaxBlocks) blocks = kMaxBlocks;
    const int lds_bins = (conf && (long long)C * C <= kLdsBins) ? C * C : 0;
    return {{N, C, out_h, out_w, scores, pred, reinterpret_cast<const long long*>(gt), ignore_index,
             reinterpret_cast<unsigned long long*>(conf), lds_bins},
            (unsigned)blocks, (size_t)(extra_words + lds_bins) * sizeof(unsigned)};
}

// launch(align, chunk) with the kernel's template arguments as integral constants.  19 classes (Cityscapes): every
// class in registers, the taps of a pass computed once; otherwise chunks of 16.
template <class Launch>
inline void vote_dispatch(int align_corners, int C, Launch launch) {
    using std::integral_constant;
    if (C == 19) {
        if (align_corners) launch(std::true_type(), integral_constant<int, 19>());
        else launch(std::false_type(), integral_constant<int, 19>());
    } else {
        if (align_corners) launch(std::true_type(), integral_constant<int, 16>());
        else launch(std::false_type(), integral_constant<int, 16>());
    }
}

}  // namespace dcfp_vote
