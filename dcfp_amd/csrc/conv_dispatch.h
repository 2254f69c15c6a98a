// conv_dispatch.h — the one internal header of the fp32 conv_*.hip family: the problem view the dispatch works on, the
// named options of the run functions, the environment knobs read by more than one file, and every function one of
// these files calls in another - declared once, so the compiler holds definition and callers to the same signature.
// (conv_f16.hip / conv_f8.hip have their own descriptors and stay out.)
#pragma once
#include "common.h"
#include <stdlib.h>
#include <string.h>

struct Igemm2Params;    // igemm2_common.h

// ---------------------------------------------------------------- descriptor checks
inline int check_desc(const DcfpConvDesc* d) {
    if (!d) return DCFP_E_BADDESC;
    if (d->N <= 0 || d->Cin <= 0 || d->Cout <= 0 || d->H <= 0 || d->W <= 0 || d->stride <= 0 ||
        d->dil <= 0 || d->pad < 0)
        return DCFP_E_BADDESC;
    if (d->KH != d->KW || (d->KH != 1 && d->KH != 3)) return DCFP_E_UNSUPPORTED;
    const int ho = (d->H + 2 * d->pad - d->dil * (d->KH - 1) - 1) / d->stride + 1;
    const int wo = (d->W + 2 * d->pad - d->dil * (d->KW - 1) - 1) / d->stride + 1;
    if (ho != d->Hout || wo != d->Wout || ho <= 0 || wo <= 0) return DCFP_E_BADDESC;
    if ((d->x_pitch != 0 && (d->x_pitch < d->W || (d->x_pitch & 3))) ||
        (d->dy_pitch != 0 && (d->dy_pitch < d->Wout || (d->dy_pitch & 3))))
        return DCFP_E_BADDESC;
    // buffer descriptors address one image / the weight tensor with 31-bit byte offsets
    if ((long long)d->Cin * d->H * (d->x_pitch ? d->x_pitch : d->W) >= (1LL << 29) ||
        (long long)d->Cout * d->Hout * (d->dy_pitch ? d->dy_pitch : d->Wout) >= (1LL << 29) ||
        (long long)d->Cout * d->Cin * d->KH * d->KW >= (1LL << 29))
        return DCFP_E_UNSUPPORTED;
    return DCFP_OK;
}

// the shape every Winograd path takes: 3x3, stride 1, pad == dilation, output the size of the input
inline bool same_size_3x3(const DcfpConvDesc* d) {
    return d->KH == 3 && d->KW == 3 && d->stride == 1 && d->pad == d->dil && d->Hout == d->H && d->Wout == d->W;
}

// ---------------------------------------------------------------- environment knobs read in more than one place
// (each latches on first use)
// EXPERIMENTAL opt-in DCFP_CONV_MATH=bf16x3: fp32 operands as three bf16 planes (conv_igemm3.hip, conv_wgrad3.hip)
inline bool math_bf16x3() {
    static const bool v = [] { const char* e = getenv("DCFP_CONV_MATH"); return e && !strcmp(e, "bf16x3"); }();
    return v;
}
// DCFP_CONV_WINOGRAD: 0 off, 1 the cost models decide (default), 2 wherever eligible (A/B)
inline int conv_winograd_mode() {
    static const int v = [] { const char* e = getenv("DCFP_CONV_WINOGRAD"); return e ? atoi(e) : 1; }();
    return v;
}
// DCFP_IGEMM_DMA=0: no LDS-DMA forward / dgrad kernels
inline bool igemm_dma_on() {
    static const bool v = [] { const char* e = getenv("DCFP_IGEMM_DMA"); return !e || atoi(e) != 0; }();
    return v;
}
// DCFP_IGEMM_2D: 2-D pixel tiles of igemm2_dma_kernel<9, true>: 0 off; 4 / 5 (default): 16 / 32 columns
inline int igemm_2d_mode() {
    static const int v = [] { const char* e = getenv("DCFP_IGEMM_2D"); return e ? atoi(e) : 5; }();
    return v;
}
// DCFP_WINO_FUSED: 0 the three passes of conv_winograd.hip only, 1 the fused kernel where it measures faster
// (default), 2 wherever it applies (tests)
inline int wino_fused_mode() {
    static const int v = [] { const char* e = getenv("DCFP_WINO_FUSED"); return e ? atoi(e) : 1; }();
    return v;
}
// DCFP_WINO_WGRAD_FUSED: 0 the batched path of conv_winograd.hip with the kept transform, 1 the fused weight-gradient
// kernel where the cost model prefers it (default), 2 wherever it applies and beats the direct kernel
inline int wino_wgrad_fused_mode() {
    static const int v = [] { const char* e = getenv("DCFP_WINO_WGRAD_FUSED"); return e ? atoi(e) : 1; }();
    return v;
}
// DCFP_WGRAD_DMA=0: no LDS-DMA weight-gradient kernels
inline bool wgrad_dma_on() {
    static const bool v = [] { const char* e = getenv("DCFP_WGRAD_DMA"); return !e || atoi(e) != 0; }();
    return v;
}

// An operand the 16-byte paths may read or write: on the 16-byte grid, images a whole number of quads apart
inline bool dcfp_quad_operand(const void* p, long long nstride) { return dcfp_aligned16(p) && nstride % 4 == 0; }

// ---------------------------------------------------------------- the problem view
// A forward or data-gradient pass as the implicit GEMM the kernels run (the table at the top of conv_igemm.hip):
//   Out[m][p] = sum over (tap, c) of A[m][tap, c] * B[c][pixel p shifted by the tap]
// (Hi, Wi): the B source's map, (Ho, Wo): the output's; the source pixel of output (oh, ow) for tap (kh, kw) is
// ((oh * sn + off0 + kh * offstep) / sd, likewise for columns); A[m][tap, c] = w[m * sAm + c * sAc + tap].
struct GemmProblem {
    int T, M, Ck, N, Hi, Wi, Ho, Wo, sn, sd, off0, offstep;
    int in_pitch;       // row pitch (floats) of the B source, 0: dense
    int sAm, sAc;
    long long in_nstride, out_nstride;
    int P() const { return Ho * Wo; }
    long long px() const { return (long long)N * Ho * Wo; }
    int HiWi() const { return Hi * Wi; }
    bool pitched() const { return in_pitch > 0 && in_pitch != Wi; }
};

// `nstride_override`: the caller's image stride of the Cout-side tensor (y of a forward, dy of a dgrad), 0: dense
inline GemmProblem gemm_problem(const DcfpConvDesc* d, int pass, long long nstride_override) {
    GemmProblem g;
    g.T = d->KH * d->KW; g.N = d->N;
    if (pass == DCFP_CONV_FWD) {
        g.M = d->Cout; g.Ck = d->Cin; g.Hi = d->H; g.Wi = d->W; g.Ho = d->Hout; g.Wo = d->Wout;
        g.sn = d->stride; g.sd = 1; g.off0 = -d->pad; g.offstep = d->dil;
        g.in_pitch = d->x_pitch; g.sAm = d->Cin * g.T; g.sAc = g.T;
        g.in_nstride = (long long)d->Cin * d->H * (d->x_pitch ? d->x_pitch : d->W);
        g.out_nstride = nstride_override ? nstride_override : (long long)d->Cout * d->Hout * d->Wout;
    } else {
        g.M = d->Cin; g.Ck = d->Cout; g.Hi = d->Hout; g.Wi = d->Wout; g.Ho = d->H; g.Wo = d->W;
        g.sn = 1; g.sd = d->stride; g.off0 = d->pad; g.offstep = -d->dil;
        g.in_pitch = d->dy_pitch; g.sAm = g.T; g.sAc = d->Cin * g.T;
        g.in_nstride = nstride_override ? nstride_override
                                        : (long long)d->Cout * d->Hout * (d->dy_pitch ? d->dy_pitch : d->Wout);
        g.out_nstride = (long long)d->Cin * d->H * d->W;
    }
    return g;
}

// What the Winograd paths ask about a same_size_3x3 problem: N x H x W maps, dilation d, M output and Ck reduced channels
struct WinoProblem {
    int N, H, W, d, M, Ck;
    long long in_nstride;
    int in_pitch;       // 0: dense
};
inline WinoProblem wino_problem(const GemmProblem& g) {
    return {g.N, g.Ho, g.Wo, g.offstep < 0 ? -g.offstep : g.offstep, g.M, g.Ck, g.in_nstride, g.in_pitch};
}

// ---------------------------------------------------------------- named options of the run functions
struct GemmExtras {
    const float* bias = nullptr;
    const float* scale = nullptr;       // inference epilogue: y = act(acc * scale[m] + shift[m] (+ residual))
    const float* shift = nullptr;
    const float* residual = nullptr;    // laid out as out
    int relu = 0;
    float* stat_part = nullptr;         // BatchNorm batch-statistics partials of the output
    int accumulate = 0;                 // out += result
    int wp_valid = 0;                   // the workspace already holds the permuted / transformed weights
    long long wp_nstride = 0;           // floats between the weight copies of consecutive images (the batched Winograd GEMM)
    const float* fan_src = nullptr;     // gradient fan-in of a residual block: out = result + fan_src where fan_mask is set
    const unsigned long long* fan_mask = nullptr;
    const Igemm2Red* red = nullptr;     // ... with the previous block's BatchNorm-backward sums as a side output
    float* xform_out = nullptr;         // Winograd forward: receives the transformed input V for the weight gradient
};

// ---------------------------------------------------------------- conv_igemm2.hip
enum Igemm2Family { IGEMM2_TILE, IGEMM2_DMA, IGEMM2_DMA1P, IGEMM2_DMA8 };
// The kernel dcfp_igemm2_run launches for (problem, options, operand alignment), and its tiling.  vec_store: the output
// takes 16-byte stores; vec_load: the B source is 16-byte aligned with an image stride of whole quads - what every LDS-DMA
// family needs of the address it copies from (the register-staged tile family takes any 4-byte aligned address)
struct Igemm2Route {
    int family;             // Igemm2Family
    int cfg, bm, bn;        // tile configuration (0: 32x512  1: 64x512  2: 128x256  3: 128x128  4: 256x256  5: 128x256
                            // strided dgrad) and the tile the launch counts in (256 x 256 on the LDS-DMA families)
    bool dma_shape;         // the shape qualifies for the 256 x 256 LDS-DMA kernels (whatever the options then allow)
    bool mixed;             // igemm2_dma_kernel<9, MIXED>: tap shifts off the 16-byte grid on dense rows
    int Mpad, CkP, tile2d;
    int tiles_per_img, tiles_n_total, tiles_m;
    int Hc, Wc, tiles_per_phase, zfold;     // strided dgrad (Igemm2Params)
};
Igemm2Route igemm2_route(const GemmProblem& g, const GemmExtras& x, bool vec_store, bool vec_load = true);
int dcfp_igemm2_run(const GemmProblem& g, const float* in, const float* w, float* out, void* workspace, size_t workspace_bytes,
                    const GemmExtras& x, hipStream_t stream);
size_t dcfp_igemm2_workspace_bytes(const GemmProblem& g);
int dcfp_igemm2_cfg_id(const GemmProblem& g);
const char* dcfp_igemm2_cfg_args(const GemmProblem& g);
bool dcfp_igemm2_dma_shape(const GemmProblem& g);
bool dcfp_igemm2_use_dma8(const GemmProblem& g);
double dcfp_igemm2_exec_fraction(const GemmProblem& g);
void dcfp_igemm2_wp_layout(const GemmProblem& g, DcfpWpEntry* e);
long long dcfp_igemm2_stat_slots(const GemmProblem& g, const float* out);
bool dcfp_igemm2_persist();
int dcfp_igemm2_ck_pad();
int dcfp_igemm2_permute_multi(const DcfpWpEntry* table, int n, long long total_blocks, hipStream_t stream);
int dcfp_igemm2n_launch(const Igemm2Params& p, int T, hipStream_t stream);     // conv_igemm2n.hip: 8 x 2 wave tiles, ragged M
int dcfp_igemm2p_launch(const Igemm2Params& p, hipStream_t stream);            // conv_igemm2p.hip: the persistent 1x1 LDS-DMA kernel
bool dcfp_igemm2p_fan_red_ok(int Mpad, int CkP);

// ---------------------------------------------------------------- conv_igemm3.hip (DCFP_CONV_MATH=bf16x3)
size_t dcfp_igemm3_workspace_bytes(int T, int M, int Ck);
int dcfp_igemm3_run(const GemmProblem& g, const float* in, const float* w, float* out, void* workspace, size_t workspace_bytes,
                    const GemmExtras& x, hipStream_t stream);

// ---------------------------------------------------------------- conv_winograd.hip / conv_winograd2.hip / conv_winograd3.hip
bool dcfp_wino_ok(const WinoProblem& q);
size_t dcfp_wino_workspace_bytes(const WinoProblem& q);
double dcfp_wino_exec_fraction(const WinoProblem& q);
double dcfp_wino_grid_fraction(const WinoProblem& q);
long long dcfp_wino_stat_slots(const WinoProblem& q);
size_t dcfp_wino_xform_bytes(const WinoProblem& q);
int dcfp_wino_run(const GemmProblem& g, const float* in, const float* w, float* out, void* workspace, size_t workspace_bytes,
                  const GemmExtras& x, hipStream_t stream);
bool dcfp_wino_fused_ok(const WinoProblem& q);
size_t dcfp_wino_fused_workspace_bytes(const WinoProblem& q);
void dcfp_wino_fused_pads(const WinoProblem& q, int* CkP, int* Mpad);
int dcfp_wino_fused_run(const GemmProblem& g, const float* in, const float* w, float* out, void* workspace,
                        size_t workspace_bytes, const GemmExtras& x, hipStream_t stream);
bool dcfp_wino_wgrad_ok(int N, int H, int W, int d, int M, int C);
size_t dcfp_wino_wgrad_workspace_bytes(int N, int H, int W, int d, int M, int C);
int dcfp_wino_wgrad_run(const float* dy, long long dy_nstride, int dy_pitch, const float* x, long long x_nstride,
                        int x_pitch, float* dw, int N, int M, int C, int H, int W, int d, void* workspace,
                        size_t workspace_bytes, hipStream_t stream, const float* xform_in);
bool dcfp_wino_wgrad_fused_ok(int N, int H, int W, int d, int M, int C, long long x_nstride, int x_pitch,
                              long long dy_nstride, int dy_pitch);
size_t dcfp_wino_wgrad_fused_workspace_bytes(int N, int H, int W, int d, int M, int C);
int dcfp_wino_wgrad_fused_run(const float* dy, long long dy_nstride, int dy_pitch, const float* x, long long x_nstride,
                              int x_pitch, float* dw, int N, int M, int C, int H, int W, int d, void* workspace,
                              size_t workspace_bytes, hipStream_t stream);

// ---------------------------------------------------------------- conv_stem.hip / conv_gemv.hip
bool dcfp_stem_shape(const DcfpConvDesc* d);
long long dcfp_stem_stat_slots(const DcfpConvDesc* d, const float* y, long long y_nstride);
int dcfp_stem_fwd(const DcfpConvDesc* d, const float* x, const float* w, float* y, long long y_nstride, const GemmExtras& ex,
                  hipStream_t stream);      // reads ex.bias, ex.stat_part
size_t dcfp_stem_wgrad_workspace_bytes(const DcfpConvDesc* d);
int dcfp_stem_wgrad(const DcfpConvDesc* d, const float* dy, long long dy_nstride, const float* x, float* dw, void* workspace,
                    size_t workspace_bytes, hipStream_t stream);
bool dcfp_gemv_shape(const DcfpConvDesc* d);
int dcfp_gemv_fwd(const DcfpConvDesc* d, const float* x, const float* w, const float* bias, float* y, long long y_nstride,
                  hipStream_t stream);
int dcfp_gemv_dgrad(const DcfpConvDesc* d, const float* dy, long long dy_nstride, const float* w, float* dx, int accumulate,
                    hipStream_t stream);
int dcfp_gemv_wgrad(const DcfpConvDesc* d, const float* dy, long long dy_nstride, const float* x, float* dw, hipStream_t stream);

// ---------------------------------------------------------------- conv_wgrad.hip / conv_wgrad3.hip / conv_igemm.hip
int dcfp_wgrad_kernel_name(const DcfpConvDesc* d, char* buf, int buf_len);
double dcfp_wgrad_exec_fraction(const DcfpConvDesc* d);
bool dcfp_wgrad_is_winograd(const DcfpConvDesc* d);
bool dcfp_wgrad_wants_xform(const DcfpConvDesc* d);
bool dcfp_wgrad_pitch_ok(const DcfpConvDesc* d);
size_t dcfp_wgrad_batched_workspace_bytes(int batch, int M, int C, long long K, int* splits_out);
int dcfp_wgrad_batched_run(const float* a, const float* bmat, float* out, int batch, int M, int C, long long K,
                           void* workspace, size_t workspace_bytes, hipStream_t stream);
int dcfp_wgrad3_launch(const float* dy, long long dy_nstride, const float* x, long long x_nstride,
                       float* out, int N, int M, int Cin, int T, int H, int W, int Ho, int Wo, int pad,
                       int dil, int Kpix, int kchunk, int splits, int tiles_m, int tiles_n,
                       hipStream_t stream);
size_t dcfp_conv2d_fwd_dgrad_workspace_bytes_(const DcfpConvDesc* d, int pass);
