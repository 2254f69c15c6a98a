// conv_igemm.hip — C-ABI entry points of conv2d forward / data gradient (include/dcfp_hip.h) and
// their dispatch to the implicit-GEMM kernels.  Replaces nn.Conv2d fwd/dgrad reached from
// networks/backbone/resnet.py:25-30,88-96,110-114, networks/tools/aspp.py:13-14,57,63 and
// networks/deeplabv3.py:25-33,37-41.
//
// Per image:   Out[m][p] = sum_k A[m][k] * B[k][p]     k = (tap, c)
//   forward :  m = co, c = ci,  A = w[co][ci][tap],  B = x [ci][ (oh*s - pad + kh*d, ow*s - pad + kw*d) ]
//   dgrad   :  m = ci, c = co,  A = w[co][ci][tap],  B = dy[co][ ((h + pad - kh*d)/s, (w + pad - kw*d)/s) ]
// i.e. a 3x3 (dilated) conv is nine shifted 1x1 GEMM slabs accumulated in one MFMA accumulator;
// large dilations (12/24/36) make halo reuse worthless, so every slab is fetched with border
// predication (L2/MALL absorb the 9x re-read of the same rows).
//   conv_igemm2.hip  exact fp32 MFMA (v_mfma_f32_32x32x2_f32, 157.3 TFLOP/s) - the default
//   conv_igemm3.hip  opt-in DCFP_CONV_MATH=bf16x3: fp32 operands as three bf16 planes
// gemm_problem (conv_dispatch.h) is the one place that writes this table out; every entry point and query below works on
// the GemmProblem it returns.
#include "conv_dispatch.h"
#include "wino_plan.h"
#include <stdio.h>

extern "C" int dcfp_abi_version(void) { return 2; }

// the shapes the bf16x3 split kernel takes: unit sampling strides and the 256 x 256 tile of the fp32 path
static bool igemm3_ok(const GemmProblem& g) {
    return math_bf16x3() && g.sn == 1 && g.sd == 1 && dcfp_igemm2_cfg_id(g) == 4;
}

// Winograd F(2x2, 3x3) (conv_winograd.hip) takes a wide 3x3 stride-1 pad == dil conv, forward or dgrad, where a
// cost model calibrated on this chip says it is faster than the direct LDS-DMA kernel (same-box measurements,
// profiles/r02_winograd_ab.txt): direct = nominal FLOPs x executed share (dead kernel rows) at 143 TF; Winograd =
// 16/36 of the nominal FLOPs x tile padding at 118 ... 135 TF (by GEMM shape) plus the two transform passes
// at 4.2 / 5.4 TB/s.  DCFP_CONV_WINOGRAD: 0 off, 1 model (default), 2 wherever eligible (A/B).
// which Winograd path a pass would take: 0 none (direct kernels), 1 the three passes of conv_winograd.hip, 2 the fused kernel
// of conv_winograd2.hip (the only one for fewer than 129 / 128 channels; needs a row-pitched operand for dilation 1 / 2)
static int wino_kind(const DcfpConvDesc* d, int pass) {
    const int mode = conv_winograd_mode();
    if (mode == 0 || !same_size_3x3(d) || math_bf16x3()) return 0;
    const bool fwd = pass == DCFP_CONV_FWD;
    const GemmProblem g = gemm_problem(d, pass, 0);
    const WinoProblem q = wino_problem(g);
    const int M = g.M, Ck = g.Ck;
    const bool three = dcfp_wino_ok(q), fused = dcfp_wino_fused_ok(q);
    if (!three && !fused) return 0;
    if (mode == 2) return three ? 1 : 2;
    const double nominal = 2.0 * d->N * (double)d->H * d->W * (double)M * Ck * 9.0;
    const double f_direct = dcfp_igemm2_exec_fraction(g);
    // (channel counts off the 256 grid - pruned models, the narrow layers - run the ragged-M / register-staged direct
    //  kernels: 100...127 TF measured)
    const double t_direct = nominal * f_direct / (M % 256 != 0 ? 115e12 : 143e12);
    const double f_wino = dcfp_wino_grid_fraction(q);
    double t_wino = 1e30;
    if (three) {
        const double tiles = f_wino * 9.0 / 16.0 * d->N * (double)d->H * d->W;          // T
        // batched GEMM rate by shape class (measured): K = 256 is store-bound (118 TF at M = 256, 130 at M >= 1024),
        // deeper K runs at 127 TF with one row of M tiles and 135 TF with several
        const double rate = Ck <= 256 ? (M >= 1024 ? 130e12 : 118e12) : (M <= 256 ? 127e12 : 135e12);
        const double pix = (double)d->N * d->H * d->W;
        const double t_in = (4.0 * pix * Ck + 64.0 * tiles * Ck) / 4.2e12;
        const double t_out = (64.0 * tiles * M + 4.0 * pix * M * (fwd ? 1.0 : 2.0)) / 5.4e12;
        const double mpad = (double)((M + 255) / 256 * 256) / M;      // the GEMM's tiles are 256 (128) rows: ragged M pays for the padding
        t_wino = nominal * f_wino * mpad / rate + t_in + t_out + 20e-6;
    }
    if (fused) {
        // the fused kernel (what dcfp_wino_run takes wherever it applies, except where the forward must leave V behind):
        // 125 TF of executed MFMA work in its K loop since round 4 (one ALU burst per slot), about four K-steps' worth of
        // prologue + epilogue per block (measured executed rates, profiles/r04_wino_fused_burst_ab.txt: 87 TF at 64 input
        // channels, 110 at 256, 122 at 512, 118 at 2048 with 16 % tile padding); blocks are 64 output channels - off the 256
        // grid (narrow layers, pruned widths) it pads M to 64 instead of 256
        const double nk = (double)((Ck + 15) / 16 * 2);
        const double mpad = (double)((M + 63) / 64 * 64) / M;
        const double t_f = nominal * f_wino * mpad / (125e12 * nk / (nk + 4.0)) + 10e-6;
        if (t_f < t_wino) t_wino = t_f;
    }
    if (!(t_wino < 0.97 * t_direct)) return 0;
    return three ? 1 : 2;
}
static bool wino_pass(const DcfpConvDesc* d, int pass) { return wino_kind(d, pass) != 0; }

// A Winograd pass that ALWAYS runs the fused kernel (conv_winograd2.hip) needs nothing in its workspace but the transformed
// filters U (16/9 of the weights): like the permuted copies of the direct kernels they can be kept per conv, rebuilt for the
// whole model by the multi-tensor refresh after an optimizer step and passed back with wp_valid = 1 - 86 filter-transform
// launches of ~10 us per step otherwise (round 4).  Not the forward that leaves its transformed INPUT behind for a batched
// weight gradient with more than 256 input channels (three passes, all scratch).  DCFP_WINO_KEEP_U=0: off.
static bool wino_keeps_u(const DcfpConvDesc* d, int pass) {
    static const bool on = [] { const char* e = getenv("DCFP_WINO_KEEP_U"); return !e || atoi(e) != 0; }();
    if (!on || (pass != DCFP_CONV_FWD && pass != DCFP_CONV_DGRAD) || !wino_pass(d, pass)) return false;
    const WinoProblem q = wino_problem(gemm_problem(d, pass, 0));
    if (!dcfp_wino_fused_ok(q)) return false;
    if (pass == DCFP_CONV_FWD && q.Ck > 256 && dcfp_wino_ok(q) && dcfp_conv2d_xform_bytes(d) > 0) return false;
    return true;
}

extern "C" int dcfp_conv2d_workspace_is_scratch(const DcfpConvDesc* d, int pass) {
    if (check_desc(d) != DCFP_OK || pass == DCFP_CONV_WGRAD) return 0;
    return (wino_pass(d, pass) && !wino_keeps_u(d, pass)) ? 1 : 0;
}

size_t dcfp_conv2d_fwd_dgrad_workspace_bytes_(const DcfpConvDesc* d, int pass) {
    if (check_desc(d) != DCFP_OK) return 0;
    const GemmProblem g = gemm_problem(d, pass, 0);
    if (const int wk = wino_kind(d, pass)) {
        const WinoProblem q = wino_problem(g);
        if (wino_keeps_u(d, pass)) {
            // (a forward WITH bias of the same descriptor runs a direct kernel - dcfp_conv2d_fwd_f32_nchw - and builds its
            //  permuted copy in whatever workspace it is handed: large enough for either)
            const size_t u = dcfp_wino_fused_workspace_bytes(q), direct = dcfp_igemm2_workspace_bytes(g);
            return u > direct ? u : direct;
        }
        if (wk == 1) return dcfp_wino_workspace_bytes(q);
        // (the fused kernel only: a source off the 16-byte grid runs the direct kernel in the same workspace)
        const size_t u = dcfp_wino_fused_workspace_bytes(q), direct = dcfp_igemm2_workspace_bytes(g);
        return u > direct ? u : direct;
    }
    const size_t b2 = dcfp_igemm2_workspace_bytes(g);
    const size_t b3 = igemm3_ok(g) ? dcfp_igemm3_workspace_bytes(g.T, g.M, g.Ck) : 0;
    return b2 > b3 ? b2 : b3;
}

// The kernel of a PLAIN call - no bias, no epilogue, no statistics, no accumulate or fan-in - whose output is dense and
// 16-byte aligned: dcfp_igemm2_run reads the same igemm2_route, with the call's own options and output alignment.
extern "C" int dcfp_conv2d_kernel_name(const DcfpConvDesc* d, int pass, char* buf, int buf_len) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!buf || buf_len <= 0) return DCFP_E_BADDESC;
    if (dcfp_gemv_shape(d)) return snprintf(buf, buf_len, "gemv_1x1_map_kernel");
    if (pass == DCFP_CONV_WGRAD) return dcfp_wgrad_kernel_name(d, buf, buf_len);
    if (pass == DCFP_CONV_FWD && dcfp_stem_shape(d)) return snprintf(buf, buf_len, "stem_fwd_kernel");
    if (const int wk = wino_kind(d, pass))
        return wk == 1 ? snprintf(buf, buf_len, "winograd_f2x2_3x3 (igemm2_dma1p_kernel<false,true>)")
                       : snprintf(buf, buf_len, "winograd_f2x2_3x3 fused (wino_fused_kernel)");
    const GemmProblem g = gemm_problem(d, pass, 0);
    if (igemm3_ok(g)) return snprintf(buf, buf_len, "igemm3_kernel<%d>", g.T);
    const Igemm2Route r = igemm2_route(g, GemmExtras(), true);
    switch (r.family) {
        case IGEMM2_DMA8: return snprintf(buf, buf_len, "igemm2_dma8_kernel<%d>", g.T);
        case IGEMM2_DMA1P: return snprintf(buf, buf_len, "igemm2_dma1p_kernel");   // <ACC>
        case IGEMM2_DMA: return snprintf(buf, buf_len, "igemm2_dma_kernel<%d,%s>", g.T, r.mixed ? "true" : "false");   // <TAPS, MIXED>
        default: return snprintf(buf, buf_len, "igemm2_kernel<%d,%s>", g.T, dcfp_igemm2_cfg_args(g));
    }
}

extern "C" double dcfp_conv2d_executed_fraction(const DcfpConvDesc* d, int pass) {
    if (check_desc(d) != DCFP_OK) return 1.0;
    if (pass == DCFP_CONV_WGRAD) return dcfp_wgrad_exec_fraction(d);
    const GemmProblem g = gemm_problem(d, pass, 0);
    // (Winograd: the enumerated tiles at 16 components each.  The 12- and 9-component classes of the fused forward / dgrad
    //  kernel are not subtracted - dcfp_wino_tile_plan reports the issued components exactly)
    if (wino_pass(d, pass)) return dcfp_wino_exec_fraction(wino_problem(g));
    if (igemm3_ok(g)) return 1.0;
    return dcfp_igemm2_exec_fraction(g);
}

// The tile plan of the Winograd paths (wino_plan.h) for an N x H x W map with dilation d.  ragged: 0 the full grid of
// super-blocks, 1 the valid tiles only, -1 as DCFP_WINO_RAGGED selects; classes: cut the grid into component classes
// (the fused forward / dgrad kernel).  out[0..5] = TH, TW, T, T16, regions, 64-tile blocks; then 8 values per region
// (four slots): r0, nr, c0, nc, rows3, cols3, first block, blocks; out[38] = components issued over all tiles.
extern "C" int dcfp_wino_tile_plan(int N, int H, int W, int d, int ragged, int classes, int64_t* out) {
    if (N <= 0 || H <= 0 || W <= 0 || d <= 0 || !out) return DCFP_E_BADDESC;
    const WinoTilePlan pl = wino_tile_plan(N, H, W, d, ragged < 0 ? wino_ragged_on() : ragged != 0, classes != 0);
    out[0] = pl.TH; out[1] = pl.TW; out[2] = pl.T; out[3] = pl.T16; out[4] = pl.nreg; out[5] = pl.tblocks;
    for (int i = 0; i < pl.nreg; ++i) {
        const WinoRegion& r = pl.reg[i];
        int64_t* o = out + 6 + 8 * i;
        o[0] = r.r0; o[1] = r.nr; o[2] = r.c0; o[3] = r.nc; o[4] = r.rows3; o[5] = r.cols3; o[6] = r.tb0; o[7] = r.nblocks;
    }
    out[38] = pl.issued;
    return DCFP_OK;
}

// Bytes of the transformed input (Winograd V, conv_winograd.hip) that the forward pass of this conv can write into a
// caller-owned buffer (dcfp_conv2d_fwd_keep_f32_nchw) for its weight gradient to take over
// (dcfp_conv2d_wgrad_kept_f32_nchw) instead of transforming x again; 0 where either pass is not Winograd.
extern "C" size_t dcfp_conv2d_xform_bytes(const DcfpConvDesc* d) {
    if (check_desc(d) != DCFP_OK) return 0;
    if (!wino_pass(d, DCFP_CONV_FWD) || !dcfp_wgrad_wants_xform(d)) return 0;
    return dcfp_wino_xform_bytes(wino_problem(gemm_problem(d, DCFP_CONV_FWD, 0)));
}

// wp_valid as a Winograd pass takes it: only the kept transformed filters are worth anything to it
static int wino_wp_valid(const DcfpConvDesc* d, int pass, int wp_valid) { return (wp_valid && wino_keeps_u(d, pass)) ? 1 : 0; }

extern "C" int dcfp_conv2d_fwd_keep_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w, float* y,
                                             int64_t y_nstride, float* xform_out, size_t xform_bytes,
                                             float* stat_partials, void* workspace, size_t workspace_bytes,
                                             dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!x || !w || !y || !xform_out) return DCFP_E_BADDESC;
    const size_t need = dcfp_conv2d_xform_bytes(d);
    if (need == 0) return DCFP_E_UNSUPPORTED;
    if (xform_bytes < need) return DCFP_E_WORKSPACE;
    GemmExtras ex;
    ex.xform_out = xform_out;
    if (stat_partials && dcfp_conv2d_fwd_stat_slots(d, y, y_nstride) > 0) ex.stat_part = stat_partials;
    return dcfp_wino_run(gemm_problem(d, DCFP_CONV_FWD, y_nstride), x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
}

extern "C" int dcfp_conv2d_fwd_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w,
                                        const float* bias, float* y, int64_t y_nstride,
                                        void* workspace, size_t workspace_bytes, int wp_valid,
                                        dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!x || !w || !y) return DCFP_E_BADDESC;
    const GemmProblem g = gemm_problem(d, DCFP_CONV_FWD, y_nstride);
    if (g.pitched() && math_bf16x3()) return DCFP_E_UNSUPPORTED;
    GemmExtras ex;
    ex.bias = bias; ex.wp_valid = wp_valid;
    if (dcfp_gemv_shape(d)) return dcfp_gemv_fwd(d, x, w, bias, y, y_nstride, dcfp_s(stream));
    // Cin = 3, stride 2: conv_stem.hip (16-byte stores only: an output off that grid takes the strided tile kernel below)
    if (dcfp_stem_shape(d) && dcfp_quad_operand(y, g.out_nstride)) return dcfp_stem_fwd(d, x, w, y, y_nstride, ex, dcfp_s(stream));
    if (!bias && wino_pass(d, DCFP_CONV_FWD)) {
        ex.wp_valid = wino_wp_valid(d, DCFP_CONV_FWD, wp_valid);
        return dcfp_wino_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
    }
    if (!bias && igemm3_ok(g)) return dcfp_igemm3_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
    return dcfp_igemm2_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
}

// Forward conv that also emits BatchNorm batch-statistics partials of its output (see
// dcfp_bn_stats_from_partials_f32).  slots == 0: this shape / math mode has no fused statistics.
extern "C" int64_t dcfp_conv2d_fwd_stat_slots(const DcfpConvDesc* d, const float* y, int64_t y_nstride) {
    if (check_desc(d) != DCFP_OK) return 0;
    if (dcfp_stem_shape(d)) return dcfp_stem_stat_slots(d, y, y_nstride);
    const GemmProblem g = gemm_problem(d, DCFP_CONV_FWD, y_nstride);
    if (wino_pass(d, DCFP_CONV_FWD))                // (the output transform emits them where every tile is interior)
        return (y_nstride % 4 == 0 && dcfp_aligned16(y)) ? dcfp_wino_stat_slots(wino_problem(g)) : 0;
    if (igemm3_ok(g)) return 0;
    return dcfp_igemm2_stat_slots(g, y);
}

extern "C" int dcfp_conv2d_fwd_stats_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w,
                                              float* y, int64_t y_nstride, float* stat_partials,
                                              void* workspace, size_t workspace_bytes, int wp_valid,
                                              dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!x || !w || !y || !stat_partials) return DCFP_E_BADDESC;
    if (dcfp_conv2d_fwd_stat_slots(d, y, y_nstride) <= 0) return DCFP_E_UNSUPPORTED;
    const GemmProblem g = gemm_problem(d, DCFP_CONV_FWD, y_nstride);
    GemmExtras ex;
    ex.stat_part = stat_partials; ex.wp_valid = wp_valid;
    if (dcfp_stem_shape(d)) return dcfp_stem_fwd(d, x, w, y, y_nstride, ex, dcfp_s(stream));
    if (wino_pass(d, DCFP_CONV_FWD)) {
        ex.wp_valid = wino_wp_valid(d, DCFP_CONV_FWD, wp_valid);
        return dcfp_wino_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
    }
    return dcfp_igemm2_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
}

extern "C" int dcfp_conv2d_dgrad_f32_nchw(const DcfpConvDesc* d, const float* dy,
                                          int64_t dy_nstride, const float* w, float* dx,
                                          int accumulate, void* workspace, size_t workspace_bytes,
                                          int wp_valid, dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!dy || !w || !dx) return DCFP_E_BADDESC;
    const GemmProblem g = gemm_problem(d, DCFP_CONV_DGRAD, dy_nstride);
    if (g.pitched() && math_bf16x3()) return DCFP_E_UNSUPPORTED;
    GemmExtras ex;
    ex.accumulate = accumulate ? 1 : 0; ex.wp_valid = wp_valid;
    if (dcfp_gemv_shape(d)) return dcfp_gemv_dgrad(d, dy, dy_nstride, w, dx, ex.accumulate, dcfp_s(stream));
    if (wino_pass(d, DCFP_CONV_DGRAD)) {    // dx = conv(dy, w') with w'[ci][co] = w[co][ci] rotated by 180 degrees
        ex.wp_valid = wino_wp_valid(d, DCFP_CONV_DGRAD, wp_valid);
        return dcfp_wino_run(g, dy, w, dx, workspace, workspace_bytes, ex, dcfp_s(stream));
    }
    if (igemm3_ok(g)) return dcfp_igemm3_run(g, dy, w, dx, workspace, workspace_bytes, ex, dcfp_s(stream));
    return dcfp_igemm2_run(g, dy, w, dx, workspace, workspace_bytes, ex, dcfp_s(stream));
}

// Gradient fan-in of a residual block (resnet.py:52-56 backward): dx = dgrad(dy) + fan_src * mask, where mask is the 1-bit
// ReLU mask of dcfp_bn_apply_relu_mask_f32 and fan_src the gradient that arrived at the block's output - the residual
// branch's gradient is never written.  1x1 stride-1 convs on the persistent LDS-DMA kernel, Cin % 256 == 0,
// H * W % 256 == 0 (dcfp_conv2d_dgrad_fanin_supported); fan_src has dx's layout.
extern "C" int dcfp_conv2d_dgrad_fanin_supported(const DcfpConvDesc* d) {
    if (check_desc(d) != DCFP_OK || d->KH != 1 || d->stride != 1 || d->pad != 0 || math_bf16x3()) return 0;
    const GemmProblem g = gemm_problem(d, DCFP_CONV_DGRAD, 0);
    if (g.M % 256 != 0 || g.P() % 256 != 0 || !dcfp_igemm2_persist()) return 0;
    if (igemm3_ok(g)) return 0;
    return dcfp_igemm2_dma_shape(g) ? 1 : 0;
}

extern "C" int dcfp_conv2d_dgrad_fanin_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride, const float* w,
                                                float* dx, const float* fan_src, const void* fan_mask, void* workspace,
                                                size_t workspace_bytes, int wp_valid, dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!dy || !w || !dx || !fan_src || !fan_mask) return DCFP_E_BADDESC;
    if (!dcfp_conv2d_dgrad_fanin_supported(d)) return DCFP_E_UNSUPPORTED;
    GemmExtras ex;
    ex.wp_valid = wp_valid; ex.fan_src = fan_src; ex.fan_mask = static_cast<const unsigned long long*>(fan_mask);
    return dcfp_igemm2_run(gemm_problem(d, DCFP_CONV_DGRAD, dy_nstride), dy, w, dx, workspace, workspace_bytes, ex, dcfp_s(stream));
}

// The fan-in with the PREVIOUS residual block's BatchNorm-backward sums as a side output: dx (this call's result) is the
// gradient arriving at that block's output; with its bn3 input `red_x`, its ReLU bit mask `red_mask` and batch mean
// `red_mean` the epilogue emits red_part[slot][Cin][2] = (sum g, sum g*(x - mean)) per 128 pixels, g = dx * mask -
// dcfp_bn_bwd_sums_from_partials_f32 turns them into what dcfp_bn_bwd_reduce_f32 returns, and that block's backward skips
// its reduce kernel (which would re-read dx and x: 8 B/element).  dcfp_conv2d_dgrad_fanin_red_slots: the slot count
// (N*H*W/128) where this form exists (fan-in supported and the launch takes 128-row tiles), else 0.
extern "C" int64_t dcfp_conv2d_dgrad_fanin_red_slots(const DcfpConvDesc* d) {
    if (!dcfp_conv2d_dgrad_fanin_supported(d)) return 0;
    const GemmProblem g = gemm_problem(d, DCFP_CONV_DGRAD, 0);
    const Igemm2Route r = igemm2_route(g, GemmExtras(), true);
    if (!dcfp_igemm2p_fan_red_ok(r.Mpad, r.CkP)) return 0;
    return g.px() / 128;
}

extern "C" int dcfp_conv2d_dgrad_fanin_red_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride,
                                                    const float* w, float* dx, const float* fan_src, const void* fan_mask,
                                                    const float* red_x, const void* red_mask, const float* red_mean,
                                                    float* red_part, void* workspace, size_t workspace_bytes, int wp_valid,
                                                    dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!dy || !w || !dx || !fan_src || !fan_mask || !red_x || !red_mask || !red_mean || !red_part) return DCFP_E_BADDESC;
    if (dcfp_conv2d_dgrad_fanin_red_slots(d) <= 0) return DCFP_E_UNSUPPORTED;
    if (reinterpret_cast<uintptr_t>(red_part) & 7u) return DCFP_E_BADDESC;
    const Igemm2Red red = {red_x, static_cast<const unsigned long long*>(red_mask), red_mean, red_part};
    GemmExtras ex;
    ex.wp_valid = wp_valid; ex.fan_src = fan_src; ex.fan_mask = static_cast<const unsigned long long*>(fan_mask);
    ex.red = &red;
    return dcfp_igemm2_run(gemm_problem(d, DCFP_CONV_DGRAD, dy_nstride), dy, w, dx, workspace, workspace_bytes, ex, dcfp_s(stream));
}

// Inference: conv + folded eval-mode BatchNorm (+residual) (+ReLU) in the conv epilogue.
extern "C" int dcfp_conv2d_fwd_fused_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w,
                                              const float* scale, const float* shift,
                                              const float* residual, int relu, float* y,
                                              void* workspace, size_t workspace_bytes, int wp_valid,
                                              dcfp_stream_t stream) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!x || !w || !y || !scale || !shift) return DCFP_E_BADDESC;
    const GemmProblem g = gemm_problem(d, DCFP_CONV_FWD, 0);
    GemmExtras ex;
    ex.scale = scale; ex.shift = shift; ex.residual = residual; ex.relu = relu ? 1 : 0;
    if (wino_pass(d, DCFP_CONV_FWD))      // the folded BatchNorm (+residual) (+ReLU) rides on the Winograd output transform
        return dcfp_wino_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));    // (U rebuilt per call)
    ex.wp_valid = wp_valid;
    if (igemm3_ok(g)) return dcfp_igemm3_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));   // opt-in bf16x3 inference
    return dcfp_igemm2_run(g, x, w, y, workspace, workspace_bytes, ex, dcfp_s(stream));
}

// Wp layout of (descriptor, pass) for a caller that refreshes the permuted copies of many convs in one
// launch after an optimizer step (dcfp_conv2d_permute_weights_multi_f32) and then passes wp_valid = 1.
extern "C" int dcfp_conv2d_wp_layout(const DcfpConvDesc* d, int pass, DcfpWpEntry* e) {
    int rc = check_desc(d);
    if (rc) return rc;
    if (!e || (pass != DCFP_CONV_FWD && pass != DCFP_CONV_DGRAD)) return DCFP_E_BADDESC;
    const GemmProblem g = gemm_problem(d, pass, 0);
    if (wino_pass(d, pass)) {
        if (!wino_keeps_u(d, pass)) return DCFP_E_UNSUPPORTED;            // all scratch: nothing to keep
        // the fused Winograd kernel's transformed filters: perm8 = 2 (forward) / 3 (dgrad: taps rotated by 180 degrees, the
        // roles of the channel strides swapped) - one (c, m) pair per element of the refresh kernel
        e->T = 16; e->M = g.M; e->Ck = g.Ck;
        dcfp_wino_fused_pads(wino_problem(g), &e->CkP, &e->Mpad);
        e->sAm = g.sAm; e->sAc = g.sAc; e->perm8 = pass == DCFP_CONV_FWD ? 2 : 3;
        const long long pairs = (long long)e->CkP * e->Mpad;
        e->n_blocks = (pairs + DCFP_WP_BLOCK_ELEMS - 1) / DCFP_WP_BLOCK_ELEMS;
        return DCFP_OK;
    }
    if (igemm3_ok(g)) return DCFP_E_UNSUPPORTED;     // bf16x3 keeps its own split copy
    dcfp_igemm2_wp_layout(g, e);
    const long long total = (long long)e->T * e->CkP * e->Mpad;
    e->n_blocks = (total + DCFP_WP_BLOCK_ELEMS - 1) / DCFP_WP_BLOCK_ELEMS;
    return DCFP_OK;
}

extern "C" int dcfp_conv2d_permute_weights_multi_f32(const DcfpWpEntry* table, int n, int64_t total_blocks,
                                                     dcfp_stream_t stream) {
    if (n == 0 || total_blocks == 0) return DCFP_OK;
    if (!table || n < 0 || total_blocks < 0 || total_blocks > 0x7fffffffLL) return DCFP_E_BADDESC;
    return dcfp_igemm2_permute_multi(table, n, total_blocks, dcfp_s(stream));
}

extern "C" int dcfp_conv2d_pitch_supported(const DcfpConvDesc* d) {
    if (check_desc(d) != DCFP_OK || math_bf16x3() || !same_size_3x3(d)) return 0;
    const int xp = d->x_pitch ? d->x_pitch : d->W, dp = d->dy_pitch ? d->dy_pitch : d->Wout;
    if (xp < d->W + d->pad && xp != d->W) return 0;
    if (dp < d->Wout + d->pad && dp != d->Wout) return 0;
    // forward and dgrad on the fused Winograd kernel (it is what makes the narrow layers Winograd at all - it reads the
    // shifted operand through 16-byte loads that rely on the zero tail), weight gradient on a kernel that takes the pitch
    if (xp != d->W && dp != d->Wout && wino_kind(d, DCFP_CONV_FWD) == 2 && wino_kind(d, DCFP_CONV_DGRAD) == 2)
        return dcfp_wgrad_pitch_ok(d) ? 1 : 0;
    // each of forward / dgrad on an LDS-DMA kernel: the 256 x 256 one or the ragged-M one (conv_igemm2n.hip).  The question
    // is about the pitched layout, so an operand the descriptor leaves dense is asked about as if it carried a tail.
    for (const int pass : {DCFP_CONV_FWD, DCFP_CONV_DGRAD}) {
        GemmProblem g = gemm_problem(d, pass, 0);
        if (!g.pitched()) g.in_pitch = g.Wi + 4;
        if (igemm2_route(g, GemmExtras(), true).family == IGEMM2_TILE) return 0;
    }
    return dcfp_wgrad_pitch_ok(d) ? 1 : 0;
}
