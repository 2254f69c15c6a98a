// vote.hip — the multi-scale + flip vote of evaluate.py:198-227 (whole=True) in one launch.
//
// The reference, per scale: the network's low-resolution logits are upsampled to the size the network saw (hs x ws),
// averaged with the mirrored pass flipped back, resized to the image (H x W) and added up; argmax and confusion matrix
// follow.  Everything after the network is linear interpolation, so a pixel's score is a fixed weighted sum of 16
// low-resolution values per map and class:
//
//   score[n,c,y,x] = sum_k weight_k * sum_{(Y,wY) in lerp(y: hs_k -> H)} sum_{(X,wX) in lerp(x: ws_k -> W)}
//                    wY * wX * U_k(c, Y, flip_k ? ws_k-1-X : X)
//
// with U_k the bilinear value of logits_k[n,c] resized (h_k, w_k) -> (hs_k, ws_k).  One lane owns one output pixel,
// computes the 4 row and 4 column taps of a map once and reuses them over the classes; the maps are small beside L2.
// The full-resolution logits never exist.  The summation order (maps, then rows, then columns) is fixed and there are
// no float atomics: two calls give the same bits.  The pixel loop, the argmax and the confusion count around that sum
// are vote_core.h's, shared with slide.hip.
//
// Coordinate rule of all four index computations: bilinear.h (lerp_of / host_scale).
#include "common.h"
#include "bilinear.h"
#include "vote_core.h"

namespace {

using namespace dcfp_bilinear;
using namespace dcfp_vote;

constexpr int kMaxMaps = 16;

struct VoteMap {
    const float* p;
    int h, w, hs, ws, flip;
    float weight;
    float sY, sX;   // hs -> H, ws -> W
    float sh, sw;   // h -> hs, w -> ws
};
struct VoteBatch {
    VoteMap m[kMaxMaps];
};

// the taps of a map are recomputed per chunk of classes (19 classes: once); pixel loop and epilogue: vote_core.h
template <bool ALIGN, int CHUNK>
__global__ void __launch_bounds__(kThreads)
vote_kernel(const VoteBatch batch, int n_maps, const VoteOut out) {
    extern __shared__ unsigned int vote_hist[];
    bins_clear(vote_hist, out.lds_bins);
    __syncthreads();
    const int C = out.C;
    vote_pixels<CHUNK>(out, vote_hist, [&](float (&acc)[CHUNK], int n, int y, int x, int c0) {
        for (int k = 0; k < n_maps; ++k) {
            const VoteMap& m = batch.m[k];
            const Lerp LY = lerp_of<ALIGN>(y, m.sY, m.hs), LX = lerp_of<ALIGN>(x, m.sX, m.ws);
            const Lerp R0 = lerp_of<ALIGN>(LY.i0, m.sh, m.h), R1 = lerp_of<ALIGN>(LY.i1, m.sh, m.h);
            const int x0 = m.flip ? m.ws - 1 - LX.i0 : LX.i0, x1 = m.flip ? m.ws - 1 - LX.i1 : LX.i1;
            const Lerp C0 = lerp_of<ALIGN>(x0, m.sw, m.w), C1 = lerp_of<ALIGN>(x1, m.sw, m.w);
            const int ro[4] = {R0.i0 * m.w, R0.i1 * m.w, R1.i0 * m.w, R1.i1 * m.w};
            const float wy0 = m.weight * LY.l0, wy1 = m.weight * LY.l1;
            const float rw[4] = {wy0 * R0.l0, wy0 * R0.l1, wy1 * R1.l0, wy1 * R1.l1};
            const int co[4] = {C0.i0, C0.i1, C1.i0, C1.i1};
            const float cw[4] = {LX.l0 * C0.l0, LX.l0 * C0.l1, LX.l1 * C1.l0, LX.l1 * C1.l1};
            const long long plane = (long long)m.h * m.w;
            const float* base = m.p + ((long long)n * C + c0) * plane;
#pragma unroll
            for (int j = 0; j < CHUNK; ++j) {
                if (c0 + j < C) {
                    const float* p = base + j * plane;
                    float s = 0.f;
#pragma unroll
                    for (int a = 0; a < 4; ++a) {
                        const float* r = p + ro[a];
                        const float row = (cw[0] * r[co[0]] + cw[1] * r[co[1]]) + (cw[2] * r[co[2]] + cw[3] * r[co[3]]);
                        s += rw[a] * row;
                    }
                    acc[j] += s;
                }
            }
        }
    });
}

}  // namespace

extern "C" int dcfp_vote_multiscale_f32(const DcfpVoteMap* maps, int n_maps, int N, int C, int H, int W, int out_h,
                                        int out_w, int align_corners, float* scores, int32_t* pred, const int64_t* gt,
                                        int ignore_index, int64_t* conf, dcfp_stream_t stream) {
    if (!maps || n_maps <= 0 || n_maps > kMaxMaps || !vote_args_ok(N, C, H, W, out_h, out_w, scores, pred, gt, conf))
        return DCFP_E_BADDESC;
    VoteBatch batch;
    for (int k = 0; k < kMaxMaps; ++k) {
        const DcfpVoteMap& s = maps[k < n_maps ? k : 0];
        if (k < n_maps) {
            if (!s.logits || s.h <= 0 || s.w <= 0 || s.hs <= 0 || s.ws <= 0 || (s.flip != 0 && s.flip != 1) ||
                !(s.weight == s.weight) || (long long)s.h * s.w > 0x7fffffffLL)
                return DCFP_E_BADDESC;
        }
        VoteMap& m = batch.m[k];
        m.p = s.logits;
        m.h = s.h; m.w = s.w; m.hs = s.hs; m.ws = s.ws; m.flip = s.flip;
        m.weight = s.weight;
        m.sY = host_scale(s.hs, H, align_corners);
        m.sX = host_scale(s.ws, W, align_corners);
        m.sh = host_scale(s.h, s.hs, align_corners);
        m.sw = host_scale(s.w, s.ws, align_corners);
    }
    const VoteLaunch L = vote_launch(N, C, out_h, out_w, scores, pred, gt, ignore_index, conf, 0);
    vote_dispatch(align_corners, C, [&](auto align, auto chunk) {
        hipLaunchKernelGGL((vote_kernel<decltype(align)::value, decltype(chunk)::value>), dim3(L.blocks), dim3(kThreads),
                           L.lds_bytes, dcfp_s(stream), batch, n_maps, L.out);
    });
    DCFP_RETURN_LAUNCH();
}
