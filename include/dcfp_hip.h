/*
 * dcfp_hip.h — C-ABI of libdcfp_hip.so: the MI355X (gfx950) kernels under the DCFP
 * segmentation-training hot path.
 *
 * The reference (wzx99/DCFP) has no native ABI: every op below is reached through a
 * stock torch.nn module (cuDNN / ATen).  Each entry point cites the reference call
 * site it replaces (file:line into the reference tree) — SURVEY.md §8(a)/(b).
 *
 * Conventions
 *   - every buffer (including workspace) is owned by the caller; the library
 *     allocates nothing (one exception, on request: dcfp_p2p_alloc, because the SyncBN mailbox needs a fine-grained
 *     allocation and an IPC handle torch cannot give) and keeps no state between calls; all launches are
 *     stream-ordered on `stream` (a hipStream_t passed as void*; NULL = default).
 *     The only process-wide state is a set of tuning switches read ONCE from the
 *     environment into function-local statics on first use: DCFP_CONV_MATH (bf16x3 opt-in),
 *     DCFP_CONV_WINOGRAD (0 direct kernels only / 1 cost model, default / 2 wherever eligible),
 *     DCFP_IGEMM_{DMA,DMA9,DMA8,2D,BK32,PERSIST,P128,P128_STATS,TAPSKIP} (P128: 128-row tiles with two workgroups per CU for
 *     the 1x1 forward / dgrad - 0 off / 1 K <= 256 / 2 every K, default; P128_STATS: the same for launches with the statistics
 *     epilogue), DCFP_WGRAD_{DMA,DMA_MIXED,WIDE,LOPSIDED,T192,HALF} (HALF = 0: 1x1 weight gradients on 256-row tiles),
 *     DCFP_WINO_KEEP_U (0: the fused Winograd kernels' transformed filters are scratch again, rebuilt in every call),
 *     DCFP_WINO_VEC, DCFP_WINO_FUSED (0 three-pass Winograd only / 1 fused kernel where it wins, default / 2 wherever it
 *     applies), DCFP_WINO_WGRAD_FUSED (0 batched Winograd weight gradient on the kept transform only / 1 the fused
 *     weight-gradient kernel where the cost model prefers it, default / 2 wherever it applies and beats the direct
 *     kernel), DCFP_WINO_RAGGED (0: every Winograd path enumerates the full grid of 2d x 2d super-blocks and the fused
 *     kernel runs all 16 components of every tile; 1, default: tiles without an output inside the image are not enumerated
 *     and tiles whose second output row / column lies outside run 12 or 9 components - forward and dgrad results are
 *     bit-identical either way), DCFP_WINO_WGRAD_RATE (TF the cost model prices that kernel at), DCFP_CONV_STEM (0: the Cin = 3 stem conv
 *     through the general kernels), DCFP_IGEMM_NT (1 / 2: nt / sc1 output stores of the 1x1 kernel, A/B), DCFP_WF_SCALAR_EPI, DCFP_CONV_GEMV (0: 1x1 convs on a 1 x 1 map through the general kernels),
 *     DCFP_CE_BWD_CELLS (0: the per-output fused upsample + CE backward instead of the cell-organised one, at every
 *     class count) -
 *     kernel / algorithm selection A/B knobs, results are identical up to the documented
 *     fp32 tolerances; changing them after the first call has no effect.  (A thread_local 16-entry cache
 *     of dispatch decisions for dilated convs is the only other state.)
 *     The second object that keeps state is an engine handle (dcfp_engine_t, the last section): it owns HOST memory
 *     only - the parsed engine file and the cached per-shape launch lists - from dcfp_engine_open to dcfp_engine_close;
 *     the device weights, workspace, input and output stay the caller's.
 *   - tensors are fp32, NCHW, dense unless a *_nstride (batch stride, in elements)
 *     argument says otherwise.
 *   - return value: 0 ok; <0 bad descriptor / unsupported shape (DCFP_E_*);
 *     >0 a hipError_t from the launch.  Nothing throws across the ABI.
 */
#ifndef DCFP_HIP_H
#define DCFP_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DCFP_OK 0
#define DCFP_E_BADDESC (-1)     /* inconsistent sizes / null pointer            */
#define DCFP_E_UNSUPPORTED (-2) /* kernel size other than 1x1 / 3x3, groups...  */
#define DCFP_E_WORKSPACE (-3)   /* workspace too small                          */

typedef void* dcfp_stream_t; /* hipStream_t */

/* ABI version of this header (bumped on any signature change). */
int dcfp_abi_version(void);

/* ------------------------------------------------------------------ conv2d
 * Replaces nn.Conv2d fwd + autograd dgrad/wgrad:
 *   networks/backbone/resnet.py:25-30 (Bottleneck), :88-96 (deep stem),
 *   :110-114,127-131 (downsample), networks/tools/aspp.py:13-14,57,63,
 *   networks/deeplabv3.py:25-33,37-41 (heads).
 * Cross-correlation, zero padding, groups=1, square kernel 1x1 or 3x3.
 * Hout = (H + 2*pad - dil*(K-1) - 1)/stride + 1 must match the descriptor.
 */
typedef struct DcfpConvDesc {
    int32_t N, Cin, H, W;       /* input  [N,Cin,H,W]                  */
    int32_t Cout, KH, KW;       /* weight [Cout,Cin,KH,KW]             */
    int32_t stride, pad, dil;   /* same in h and w                     */
    int32_t Hout, Wout;         /* output [N,Cout,Hout,Wout]           */
    /* Row-pitched operands (0 = dense rows).  x_pitch: rows of x are x_pitch >= W floats apart and the
     * x_pitch - W floats behind each row are ZERO (images x_pitch*H*Cin apart); dy_pitch likewise for dy
     * (rows of Wout).  A 3x3 conv with pad = dil whose taps shift columns by a non-multiple of 4 (dilation
     * 1, 2) can then copy every shifted 16-byte quad as is - what hangs over a row end reads the zero tail -
     * instead of falling back to 4-byte copies at the image borders (dcfp_conv2d_pitch_supported tells
     * whether all three passes of a descriptor take pitched operands; the BatchNorm kernels that produce
     * x / dy write pitched outputs: dcfp_bn_apply_f32 / dcfp_bn_bwd_apply_f32 `*_pitch`).
     * fwd reads x pitched, dgrad reads dy pitched, wgrad reads both; outputs are always dense.
     * Contract for a pitched tensor: besides the zero tails, the (pitch - W) floats in FRONT of its first
     * element must be readable zeros too (a leading margin of the allocation): the quad that hangs over the
     * left end of the very first row reads them. */
    int32_t x_pitch, dy_pitch;
} DcfpConvDesc;

enum { DCFP_CONV_FWD = 0, DCFP_CONV_DGRAD = 1, DCFP_CONV_WGRAD = 2 };

/* Bytes of workspace a pass needs: fwd/dgrad — the permuted, zero-padded weight copy
 * Wp[tap][c][m] the kernel streams its A operand from; wgrad — the split-K slabs.
 * fwd/dgrad take `wp_valid`: 0 => the call (re)builds Wp in `workspace` first; != 0 => the caller
 * vouches that `workspace` still holds the Wp an earlier call with the SAME descriptor, pass and
 * weight values left there (weights change once per optimizer step, so a training loop keeps one
 * buffer per conv and pass and permutes at most once per step). */
size_t dcfp_conv2d_workspace_bytes(const DcfpConvDesc* d, int pass);

/* One launch for the Wp copies of MANY convs (a model's forward and dgrad layouts after an optimizer
 * step: optimizer.py:24-25 changes every weight once per iteration).  dcfp_conv2d_wp_layout fills the
 * layout fields and n_blocks of an entry for (descriptor, pass) (DCFP_E_UNSUPPORTED where the pass keeps
 * another kind of copy, e.g. DCFP_CONV_MATH=bf16x3); the caller sets w (reference-layout weights), wp
 * (its persistent buffer of dcfp_conv2d_workspace_bytes) and first_block = prefix sum of n_blocks, uploads
 * the table once, and after every weight update launches dcfp_conv2d_permute_weights_multi_f32 and passes
 * wp_valid = 1 to the conv calls. */
#define DCFP_WP_BLOCK_ELEMS 2048
typedef struct DcfpWpEntry {
    const float* w;
    float* wp;
    int64_t first_block;
    int64_t n_blocks;
    int32_t T, Ck, CkP, M, Mpad, sAm, sAc;
    int32_t perm8;   /* 1: rows of every 256-row tile permuted for the ragged-M kernel (position 8l+i <- channel 32i+l);
                        2 / 3: not a permutation but the transformed filters G g G^T of a fused Winograd conv (forward /
                        dgrad: T = 16, one (channel, filter) pair per element - dcfp_conv2d_workspace_is_scratch) */
} DcfpWpEntry;
int dcfp_conv2d_wp_layout(const DcfpConvDesc* d, int pass, DcfpWpEntry* entry);
int dcfp_conv2d_permute_weights_multi_f32(const DcfpWpEntry* table, int n_entries, int64_t total_blocks,
                                          dcfp_stream_t stream);

/* 1 when forward, dgrad and wgrad of this descriptor all accept the row-pitched operands it names
 * (x_pitch / dy_pitch > 0): 3x3, stride 1, pad = dil, the 256 x 256 LDS-DMA tiles; else 0. */
int dcfp_conv2d_pitch_supported(const DcfpConvDesc* d);

/* 1 when the pass's workspace is pure scratch (the Winograd path of conv_winograd.hip: transformed filters,
 * transformed input and the batched GEMM's output - up to a few GB for the ASPP branches): nothing in it survives
 * the call, `wp_valid` is ignored, and a caller should hand every such conv the SAME buffer instead of keeping one
 * per conv.  0: the workspace holds the permuted weight copy described under `wp_valid` - or, for a Winograd pass
 * that always runs the fused kernel (round 4), nothing but its transformed filters (16/9 of the weights), kept, refreshed
 * by dcfp_conv2d_permute_weights_multi_f32 and validated through `wp_valid` the same way. */
int dcfp_conv2d_workspace_is_scratch(const DcfpConvDesc* d, int pass);

/* Winograd convs (see dcfp_conv2d_workspace_is_scratch): forward and weight gradient transform the same input x
 * the same way.  dcfp_conv2d_xform_bytes > 0: the forward call may write that transform (16 x Cin x tiles floats, 4x
 * the size of x) into a caller-owned buffer, and the weight gradient takes it instead of x - a fifth to a quarter of
 * its time - at the price of keeping the buffer alive between the two (the way autograd keeps x).  Same results
 * either way (the same kernels produce the same values).  0: not available for this descriptor - or not wanted: since
 * round 4 the weight gradient of most Winograd convs is ONE kernel that transforms x and dy inside the GEMM
 * (conv_winograd3.hip; dilation 1 / 2 on row-pitched operands with W % 4 == 0, even dilations >= 4 with W even), needs no
 * kept transform and is what dcfp_conv2d_wgrad_f32_nchw dispatches to; the kept transform remains for the convs that
 * kernel does not take (dense dilation-1 / 2 operands: conv_deepsup.0 reading layer3's output). */
size_t dcfp_conv2d_xform_bytes(const DcfpConvDesc* d);
int dcfp_conv2d_fwd_keep_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w, float* y, int64_t y_nstride,
                                  float* xform_out, size_t xform_bytes,
                                  float* stat_partials /* nullable: as dcfp_conv2d_fwd_stats_f32_nchw, where
                                                          dcfp_conv2d_fwd_stat_slots > 0 */,
                                  void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
int dcfp_conv2d_wgrad_kept_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride, const float* xform,
                                    size_t xform_bytes, float* dw, void* workspace, size_t workspace_bytes,
                                    dcfp_stream_t stream);

/* Gradient fan-in of a residual block (networks/backbone/resnet.py:52-56, backward): dx = dgrad(dy) + fan_src * mask,
 * mask = the 1-bit ReLU mask written by dcfp_bn_apply_relu_mask_f32, fan_src = the gradient that arrived at the block's
 * output (layout of dx).  The residual branch's gradient dy * mask is then never materialised (the BatchNorm backward
 * is called without its residual output).  Same workspace / wp_valid contract as dcfp_conv2d_dgrad_f32_nchw. */
int dcfp_conv2d_dgrad_fanin_supported(const DcfpConvDesc* d);
int dcfp_conv2d_dgrad_fanin_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride, const float* w, float* dx,
                                     const float* fan_src, const void* fan_mask, void* workspace, size_t workspace_bytes,
                                     int wp_valid, dcfp_stream_t stream);
/* The same fan-in that ALSO emits the BatchNorm-backward sums of the PREVIOUS residual block (resnet.py:41-56 backward):
 * dx, this call's result, is the gradient arriving at that block's output; with that block's bn3 input `red_x` (laid
 * out as dx), its ReLU bit mask `red_mask` (layout of dcfp_bn_apply_relu_mask_f32) and batch mean `red_mean[Cin]` the
 * epilogue writes red_part[slot][Cin][2] = (sum g, sum g*(x - mean)) over 128 pixels each, g = dx * mask bit;
 * dcfp_bn_bwd_sums_from_partials_f32 reduces the slots in a fixed order in fp64 to exactly the outputs of
 * dcfp_bn_bwd_reduce_f32 (sum_dy, sum_dy_xmu, dgamma, dbeta) - that block's backward then skips its reduce kernel and
 * never re-reads dx (8 B/element less).  dcfp_conv2d_dgrad_fanin_red_slots: the slot count N*H*W/128 where this form
 * exists (fan-in supported AND the launch takes the 128-row tiles, Cout <= 256), else 0. */
int64_t dcfp_conv2d_dgrad_fanin_red_slots(const DcfpConvDesc* d);
int dcfp_conv2d_dgrad_fanin_red_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride, const float* w,
                                         float* dx, const float* fan_src, const void* fan_mask, const float* red_x,
                                         const void* red_mask, const float* red_mean, float* red_part, void* workspace,
                                         size_t workspace_bytes, int wp_valid, dcfp_stream_t stream);
int dcfp_bn_bwd_sums_from_partials_f32(const float* partials, int64_t slots, int C, const float* var, float eps,
                                       float* sum_dy, float* sum_dy_xmu, float* dgamma /* nullable */,
                                       float* dbeta /* nullable */, dcfp_stream_t stream);

/* Name of the kernel instance a pass dispatches for this descriptor, e.g.
 * "igemm_kernel<9,4,4,2,2,0>" (template args: taps, TM, TN, WM, WN[, strided-dgrad]) — the
 * string rocprofv3 shows (demangled) for the launch; used by bench.py to label rooflines.
 * Returns the length written (excluding NUL), or <0 on a bad descriptor. */
int dcfp_conv2d_kernel_name(const DcfpConvDesc* d, int pass, char* buf, int buf_len);

/* Fraction (0 < f <= 1) of the pass's nominal multiply-adds - 2*N*Cout*Hout*Wout*Cin*KH*KW, padded taps included,
 * the usual convention and the one bench.py's `roofline.achieved` uses - that the dispatched kernel really issues.
 * < 1 for dilated 3x3 convs whose dilation is comparable to the image height (ASPP 12 / 24 / 36 on 128 rows,
 * networks/tools/aspp.py:37-39): the 9-tap LDS-DMA kernels skip, per pixel tile, the kernel rows that lie
 * wholly in the zero padding (x + 0*w == x: same bits for finite weights).  Accounting only (bench.py reports
 * `executed_frac` beside `frac`); DCFP_IGEMM_TAPSKIP=0 disables the skipping.  A Winograd pass counts the tiles its
 * plan enumerates at 16 components each (16/36 x tile padding; ragged maps: dcfp_wino_tile_plan). */
double dcfp_conv2d_executed_fraction(const DcfpConvDesc* d, int pass);

/* The tile plan the Winograd F(2x2, 3x3) paths share for an N x H x W map with dilation d (tests, tools).
 * ragged: 0 the full grid of super-blocks, 1 only tile rows / columns with an output inside the image, -1 what
 * DCFP_WINO_RAGGED selects; classes != 0: the grid cut into the component classes of the fused forward / dgrad kernel.
 * out (39 values): TH, TW, T, T16, regions, 64-tile blocks, then per region (four slots) r0, nr, c0, nc, rows3, cols3,
 * first block, blocks - tile rows r0 .. r0 + nr - 1 x tile columns c0 .. c0 + nc - 1 of every image; rows3 / cols3 = 0: the
 * tiles' second output row / column lies outside the image and the components r = 3 / s = 3 are not computed; out[38]:
 * the components issued over all tiles (dcfp_conv2d_executed_fraction counts 16 per enumerated tile). */
int dcfp_wino_tile_plan(int N, int H, int W, int d, int ragged, int classes, int64_t* out);

/* Alignment contract of the fp32 conv entry points (dcfp_conv2d_*_f32_nchw): x, w, bias, y, dy, dx, dw, db, residual,
 * scale and shift may be ANY 4-byte aligned address, and every image stride any count of floats.  16-byte alignment (with
 * an image stride that is a multiple of 4 floats) only selects faster kernels: the LDS-DMA families (igemm2_dma*,
 * the fused Winograd kernels, wgrad_dma_kernel) copy 16 bytes at a time from x / dy and are taken only when that source is
 * 16-byte aligned; the 16-byte epilogues, the stem kernels and the fused BatchNorm statistics only when y (dy for the
 * stem's weight gradient, residual for the inference epilogue) is.  Anything else runs the register-staged kernels,
 * within the same error bounds but - on a shape that would have taken an LDS-DMA kernel - with another summation order.
 * dcfp_conv2d_kernel_name names the kernel of the call whose operands are all 16-byte aligned.  Consequences and exceptions:
 *  - `workspace`, `xform` / `xform_out` and `red_part` keep the alignment stated with them (16 / 16 / 8 bytes).
 *  - wp_valid != 0 vouches for a copy built by a call with the same descriptor, pass AND the same two answers to "is the
 *    source 16-byte aligned / is the output": a call off the grid may run a kernel with another layout of the copy, so a
 *    caller keeps one buffer per such class (or passes 0).
 *  - a row-pitched x / dy (x_pitch / dy_pitch) is read by LDS-DMA kernels only: it and the call's output must be 16-byte
 *    aligned, else DCFP_E_UNSUPPORTED (nothing is launched).
 *  - dcfp_conv2d_fwd_stats_f32_nchw / dcfp_conv2d_fwd_keep_f32_nchw on a Winograd descriptor, and the dgrad fan-in
 *    (dy, fan_src, red_x): the statistics, the kept transform and the fan-in epilogue exist on the LDS-DMA kernels only, so
 *    x / dy / fan_src / red_x must be 16-byte aligned, else DCFP_E_UNSUPPORTED (nothing is launched);
 *    dcfp_conv2d_fwd_stat_slots answers 0 for a y the statistics epilogue cannot take.
 * No call launches anything before it is refused.
 *
 * y = conv(x, w) (+ bias[co] when bias != NULL).  y_nstride: batch stride of y in
 * elements (0 => Cout*Hout*Wout), lets a branch write into a channel slice of a
 * wider tensor (ASPP concat, aspp.py:77). */
int dcfp_conv2d_fwd_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w,
                             const float* bias, float* y, int64_t y_nstride,
                             void* workspace, size_t workspace_bytes, int wp_valid,
                             dcfp_stream_t stream);
/* Inference path (evaluate.py:186-196 predict_whole): conv with the eval-mode BatchNorm folded
 * into the epilogue: y = act( conv(x,w)[co]*scale[co] + shift[co] (+ residual) ), act = ReLU if relu
 * (scale = gamma*rsqrt(running_var+eps), shift = beta - running_mean*scale).  Dense y / residual. */
int dcfp_conv2d_fwd_fused_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w,
                                   const float* scale, const float* shift, const float* residual,
                                   int relu, float* y, void* workspace, size_t workspace_bytes,
                                   int wp_valid, dcfp_stream_t stream);
/* dx = conv_transpose(dy, w); accumulate != 0 => dx += (fan-out gradients).
 * dy_nstride: batch stride of dy in elements (0 => dense). */
int dcfp_conv2d_dgrad_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride,
                               const float* w, float* dx, int accumulate,
                               void* workspace, size_t workspace_bytes, int wp_valid,
                               dcfp_stream_t stream);
/* dw[co,ci,kh,kw] = sum_{n,p} dy[n,co,p] * x[n,ci,src(p,kh,kw)]; deterministic
 * two-stage split-K (no float atomics).  db (nullable) = sum_{n,p} dy. */
int dcfp_conv2d_wgrad_f32_nchw(const DcfpConvDesc* d, const float* dy, int64_t dy_nstride,
                               const float* x, float* dw, float* db,
                               void* workspace, size_t workspace_bytes,
                               dcfp_stream_t stream);

/* ------------------------------------------------------------- batch norm
 * Replaces nn.BatchNorm2d(+ReLU inplace)(+residual add) train fwd/bwd:
 *   resnet.py:9,26-33,41-56; aspp.py:15-16,22-24; deeplabv3.py:26-31,38-39.
 * Statistics over (N,H,W) per channel; biased variance for normalisation.
 * Alignment: every float tensor (x, y, dy, dx, residual, d_residual, the per-channel vectors) may be any 4-byte aligned
 * address with any image stride; 16-byte alignment with HW % 4 == 0 and strides of whole quads only selects the 16-byte
 * kernels (same values: the kernels are per element or add in an order that does not depend on the vector width, except
 * dcfp_bn_stats_f32 / dcfp_bn_bwd_reduce_f32, whose sums are chunked by the access width).  Exceptions: the bit mask of
 * dcfp_bn_apply_relu_mask_f32 is 8-byte aligned, workspaces as stated, and dcfp_bn_apply_relu_mask_f32 and
 * dcfp_bn_bwd_fused_f32 take 16-byte aligned tensors only (DCFP_E_UNSUPPORTED otherwise, nothing launched: run
 * dcfp_bn_apply_f32 / the two backward kernels).
 */
/* Module-side bookkeeping of a training-mode nn.BatchNorm2d forward, folded into the kernel that
 * finalises the statistics (resnet.py:9: momentum 0.1): when running_mean != NULL,
 *   running = (1-momentum)*running + momentum*stat   (variance unbiased by count/(count-1)),
 * and when num_batches_tracked != NULL (one int64) it is incremented by one. */
typedef struct DcfpBnRunning {
    float* running_mean;          /* nullable: no running-statistics update            */
    float* running_var;
    int64_t* num_batches_tracked; /* nullable                                          */
    float momentum;
    int32_t pad_;
} DcfpBnRunning;
/* Per-channel batch mean and biased variance of x[N,C,HW] (x_nstride elements
 * between images; 0 => C*HW).  workspace: dcfp_bn_workspace_bytes(N,C,HW).  run: nullable. */
size_t dcfp_bn_workspace_bytes(int N, int C, int HW);
int dcfp_bn_stats_f32(const float* x, int64_t x_nstride, int N, int C, int HW,
                      float* mean, float* var, const DcfpBnRunning* run,
                      void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
/* y = act( (x-mean)*rsqrt(var+eps)*gamma + beta (+ residual) ), act = ReLU if relu.
 * y_nstride: batch stride of y (0 => dense).  y_pitch != 0 (with W, the row length): the rows of y are
 * written y_pitch >= W floats apart (DcfpConvDesc.x_pitch of the conv that reads y); the tail behind each
 * row is the caller's zero padding and is not written. */
int dcfp_bn_apply_f32(const float* x, const float* mean, const float* var,
                      const float* gamma, const float* beta, float eps,
                      const float* residual, int relu, float* y, int64_t y_nstride,
                      int N, int C, int HW, int W, int y_pitch, dcfp_stream_t stream);
/* Backward stage 1: with g = dy * mask:
 *   sum_dy[c] = sum g ;  sum_dy_xmu[c] = sum g*(x-mean[c])
 * (dbeta = sum_dy; dgamma = sum_dy_xmu * rsqrt(var+eps): the per-filter statistic
 * that feeds the EIC score, pruners/dcfp_pruner.py:18).
 * relu: 0 no ReLU (mask = 1); 1 mask = (y > 0) read from the saved output y; 3 `y` is the bit mask
 *       written by dcfp_bn_apply_relu_mask_f32;
 *       2 mask re-derived from x with the forward's own expression (only valid when the
 *         forward had no residual input; needs var/gamma/beta, y may be NULL). */
int dcfp_bn_bwd_reduce_f32(const float* dy, int64_t dy_nstride, const float* x,
                           const float* y, int64_t y_nstride, const float* mean,
                           const float* var, const float* gamma, const float* beta, float eps,
                           int relu, int N, int C, int HW,
                           float* sum_dy, float* sum_dy_xmu, float* dgamma /* nullable: sum_dy_xmu*istd */,
                           float* dbeta /* nullable: a second copy of sum_dy (the caller's gradient slot; sum_dy
                                           itself may then be all-reduced in place under SyncBN) */,
                           void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
/* Conv forward that also emits the BatchNorm batch statistics of its OUTPUT as partials
 * (resnet.py:25-33: every conv is followed by a BatchNorm that needs mean/var over N,H,W):
 * stat_partials[slot][Cout][2] = (mean, sum of squared deviations) over 128 output pixels each.
 * dcfp_conv2d_fwd_stat_slots() gives the slot count for a shape (0: not available - tiles off
 * the channel/pixel grid, bias, or DCFP_CONV_MATH=bf16x3 - use dcfp_bn_stats_f32 then);
 * dcfp_bn_stats_from_partials_f32 merges them in a fixed order in fp64 (biased variance). */
int64_t dcfp_conv2d_fwd_stat_slots(const DcfpConvDesc* d, const float* y, int64_t y_nstride);
int dcfp_conv2d_fwd_stats_f32_nchw(const DcfpConvDesc* d, const float* x, const float* w, float* y,
                                   int64_t y_nstride, float* stat_partials, void* workspace,
                                   size_t workspace_bytes, int wp_valid, dcfp_stream_t stream);
int dcfp_bn_stats_from_partials_f32(const float* partials, int64_t slots, int slot_count, int C,
                                    float* mean, float* var, const DcfpBnRunning* run /* nullable; count =
                                    slots*slot_count */, dcfp_stream_t stream);
/* SyncBatchNorm (engine.py:65) forward exchange, device side: `gathered` = world rows of
 * (mean[C], var[C], count) as all-gathered from the ranks -> pooled mean, biased variance over all
 * ranks' pixels and the total count (one float, stays on the device). */
int dcfp_syncbn_combine_f32(const float* gathered, int world, int C, float* mean, float* var,
                            float* total_count, const DcfpBnRunning* run /* nullable; pooled statistics and
                            count */, dcfp_stream_t stream);
/* SyncBatchNorm exchange without a collective library call (engine.py:65; SURVEY C2: 115 all-gathers + 115
 * all-reduces of <= 4097 floats per step, all latency-bound): each rank owns a MAILBOX in its HBM that its peers map
 * (dcfp_p2p_export -> the 64-byte handle travels over the host-side process group -> dcfp_p2p_import), and ONE
 * single-workgroup kernel per BatchNorm layer and direction writes this rank's row into every rank's mailbox over
 * xGMI, waits for the others' rows in its own, and reduces them in rank order (bit-identical on all ranks).
 *   mailboxes[r]  rank r's mailbox as mapped in THIS process (the local allocation for r == rank), world <= 8;
 *   seq           1, 2, 3, ... - the same on all ranks for the same exchange (never 0);
 *   cap_floats    payload capacity the mailboxes were sized for (multiple of 32); n <= cap_floats;
 *   mode 0        out[world][n] = the rows (all-gather);
 *   mode 1        out[n] = sum over ranks, rank order (backward: [sum g, sum g*(x-mean)] adjacent, n = 2C);
 *   mode 2        rows = (mean[C], var[C], count), n = 2C+1: out = (pooled mean[C], pooled biased var[C], total count)
 *                 as dcfp_syncbn_combine_f32 computes them, and `run` (nullable) is updated from the pooled values;
 *   spin_limit    polling rounds (~0.55 us each) after which the kernel gives up: outputs = NaN, *status = seq
 *                 (a device int32 the caller zeroed once; it is never written otherwise).
 * dcfp_p2p_alloc kind: 0 fine-grained device memory (the default), 1 uncached, 2 plain hipMalloc; zero-filled.
 * All ranks must have imported every mailbox before the first exchange, and unmap before the owner frees. */
#define DCFP_P2P_HANDLE_BYTES 64
size_t dcfp_syncbn_p2p_mailbox_bytes(int world, int cap_floats);
int dcfp_p2p_alloc(size_t bytes, int kind, void** ptr);
int dcfp_p2p_free(void* ptr);
int dcfp_p2p_export(void* ptr, void* handle64);
int dcfp_p2p_import(const void* handle64, void** ptr);
int dcfp_p2p_unmap(void* ptr);
int dcfp_syncbn_p2p_exchange_f32(void* const* mailboxes, int world, int rank, uint32_t seq, int cap_floats,
                                 const float* local, int n, int mode, float* out, const DcfpBnRunning* run,
                                 uint32_t spin_limit, int32_t* status, dcfp_stream_t stream);
/* Running statistics of nn.BatchNorm2d in training mode (resnet.py:9, momentum 0.1):
 * running = (1-momentum)*running + momentum*stat, the variance unbiased by count/(count-1);
 * count_dev (nullable, one float) overrides `count` (SyncBN: global count on the device). */
int dcfp_bn_update_running_f32(const float* mean, const float* var, int C, float momentum,
                               float count, const float* count_dev, float* running_mean,
                               float* running_var, dcfp_stream_t stream);
/* Forward of a BatchNorm + ReLU with a residual input that ALSO writes the ReLU mask as one bit per
 * element (N*C*HW/8 bytes, 8-byte aligned; needs HW % 256 == 0).  The backward kernels take the mask
 * through their `y` argument with relu == 3 instead of re-reading the 4-byte output (resnet.py:52-56). */
int dcfp_bn_apply_relu_mask_f32(const float* x, const float* mean, const float* var,
                                const float* gamma, const float* beta, float eps,
                                const float* residual, float* y, void* relu_mask,
                                int N, int C, int HW, dcfp_stream_t stream);
/* Backward stage 2: dx = gamma*istd*( g - sum_dy/M - (x-mean)*istd^2*sum_dy_xmu/M ),
 * M = count (N*HW); under SyncBN the global count lives on the device: count_dev (nullable,
 * one float) then overrides `count` without a host round trip.  d_residual (nullable) = g. */
int dcfp_bn_bwd_apply_f32(const float* dy, int64_t dy_nstride, const float* x,
                          const float* y, int64_t y_nstride, const float* mean,
                          const float* var, const float* gamma, const float* beta, float eps,
                          const float* sum_dy, const float* sum_dy_xmu, float count,
                          const float* count_dev,
                          int relu, float* dx, float* d_residual,
                          int N, int C, int HW, int W, int dx_pitch /* as y_pitch above, for dx */,
                          dcfp_stream_t stream);

/* Backward stages 1 + 2 in ONE launch, for a BatchNorm whose sums need no exchange between ranks (plain
 * nn.BatchNorm2d, or SyncBatchNorm at world size 1): a block keeps its <= 8192 elements of dy and x in registers
 * between the two stages, so both tensors are read once (12 B/element instead of 20).  Outputs are the same bits as
 * dcfp_bn_bwd_reduce_f32 followed by dcfp_bn_bwd_apply_f32 (same plan, same summation order).  Arguments as there;
 * `count` = N*HW.  The blocks of a channel meet through `sync` (dcfp_bn_bwd_fused_sync_bytes(N,C,HW) bytes, 8-byte
 * aligned; 0 = shape not supported, the call then returns DCFP_E_UNSUPPORTED and the two-kernel path applies):
 *   - the CALLER zero-fills `sync` once (it may serve every later call on the same stream, any shape that fits) and
 *     passes a strictly increasing `epoch` >= 1 with every call on it (re-zero before wrapping to 1);
 *   - spin_limit: polls (~0.3 us each) after which a block gives up waiting for its channel's other blocks
 *     (0 = default 2^18, ~0.1 s): its dx and the channel's sums become NaN and *status (nullable device int32, zeroed once by
 *     the caller, never written otherwise) = epoch.  Needs 16-byte aligned tensors, HW % 4 == 0. */
size_t dcfp_bn_bwd_fused_sync_bytes(int N, int C, int HW);
int dcfp_bn_bwd_fused_f32(const float* dy, int64_t dy_nstride, const float* x, const float* y,
                          int64_t y_nstride, const float* mean, const float* var, const float* gamma,
                          const float* beta, float eps, float count, int relu, float* dx, float* d_residual,
                          int N, int C, int HW, int W, int dx_pitch, float* sum_dy, float* sum_dy_xmu,
                          float* dgamma, float* dbeta, void* sync, size_t sync_bytes, uint32_t epoch,
                          uint32_t spin_limit, int32_t* status, dcfp_stream_t stream);

/* ------------------------------------------------- element-wise / pooling
 * Alignment of the entry points of this section and of the pyramid pooling below: any 4-byte aligned float tensor, any
 * image stride; 16-byte alignment (with W % 8 == 0 for the max pool, W % 4 == 0 / HW % 4 == 0 / pitches and strides of
 * whole quads elsewhere) only selects the 16-byte kernels, which give the same values - the same bits, except the row
 * sums of dcfp_rowsum_f32, whose order follows the access width.
 * MaxPool2d(3,2,1) (resnet.py:100,149): -inf padding, first-max index. */
int dcfp_maxpool3x3s2_fwd_f32(const float* x, float* y, int32_t* argmax,
                              int N, int C, int H, int W, int Hout, int Wout,
                              dcfp_stream_t stream);
int dcfp_maxpool3x3s2_bwd_f32(const float* dy, const int32_t* argmax, float* dx,
                              int N, int C, int H, int W, int Hout, int Wout,
                              dcfp_stream_t stream);
/* AdaptiveAvgPool2d(1) (aspp.py:56): y[n,c] = scale * sum_hw x[n,c,:]. */
int dcfp_rowsum_f32(const float* x, int64_t x_nstride, float* y, float scale,
                    int N, int C, int HW, dcfp_stream_t stream);
/* bilinear 1x1 -> HxW (aspp.py:76) = broadcast: y[n,c,:] (+)= scale*v[n,c]. */
int dcfp_broadcast_hw_f32(const float* v, float scale, float* y, int64_t y_nstride,
                          int accumulate, int N, int C, int HW, dcfp_stream_t stream);
/* out = a + b (gradient fan-in); out may alias a. */
int dcfp_add_f32(const float* a, const float* b, float* out, int64_t n,
                 dcfp_stream_t stream);
/* Dropout2d (deeplabv3.py:40) with a host-drawn keep mask: y = x*mask[n,c]. */
int dcfp_channel_scale_f32(const float* x, const float* mask, float* y,
                           int N, int C, int HW, dcfp_stream_t stream);

/* --------------------------------------- bilinear upsample (+) cross-entropy
 * F.interpolate(bilinear, align_corners) (deeplabv3.py:47,50). */
int dcfp_upsample_bilinear_fwd_f32(const float* x, float* y, int N, int C,
                                   int h, int w, int H, int W, int align_corners,
                                   dcfp_stream_t stream);
int dcfp_upsample_bilinear_bwd_f32(const float* dy, float* dx, int N, int C,
                                   int h, int w, int H, int W, int align_corners,
                                   dcfp_stream_t stream);
/* y[:, c, :H, :W] = F.interpolate(x, (H, W), mode='bilinear', align_corners) into a channel slice of a
 * batch-strided, row-pitched destination (y_pitch 0: dense rows).  Writes only the W live floats of a row.
 * x: [N, C, h, w] with dense images, x_nstride elements apart (0: C*h*w); y_nstride 0: C*H*pitch.  On dense
 * operands the same bits as dcfp_upsample_bilinear_fwd_f32 (networks/deeplabv3p.py:37, the DeepLabv3+ decoder). */
int dcfp_resize_bilinear_into_f32(const float* x, int64_t x_nstride, int N, int C, int h, int w,
                                  float* y, int64_t y_nstride, int y_pitch, int H, int W,
                                  int align_corners, dcfp_stream_t stream);
/* dx (+)= interpolate^T(dy): dy is a channel slice of a batch-strided (optionally row-pitched) tensor.
 * Gather form, fixed summation order, no atomics; accumulate = 1 adds into dx.  dx: [N, C, h, w] with dense
 * images, dx_nstride elements apart (0: C*h*w). */
int dcfp_resize_bilinear_adjoint_f32(const float* dy, int64_t dy_nstride, int dy_pitch, int N, int C, int H, int W,
                                     float* dx, int64_t dx_nstride, int h, int w, int align_corners,
                                     int accumulate, dcfp_stream_t stream);
/* ------------------------------------------------ pyramid pooling (PSPNet, networks/tools/ppm.py)
 * Levels: nlev (1..4) pairs (sh, sw), 1 <= sh, sw <= 8, in host memory (level_hw).  The pooled maps / their
 * gradients are one buffer of level-major blocks [N, C, sh, sw].  Windows are PyTorch's adaptive ones
 * (start = floor(i*H/s), end = ceil((i+1)*H/s)): they overlap where s does not divide H, s > H included.
 * Fixed summation orders, no atomics: every run gives the same bits.
 *
 * out = the sums (mean = 0) or means (mean = 1) of every level of x [N, C, H, W] (dense), and, with dst,
 * dst[:, c, :H, :W] = x: a copy into a channel slice of a batch-strided, row-pitched destination (dst_pitch 0:
 * dense rows; dst_nstride 0: C*H*pitch) that writes only the W live floats of a row.  x is read once. */
int dcfp_ppm_pool_f32(const float* x, int N, int C, int H, int W, int nlev, const int* level_hw,
                      float* out, int mean, float* dst, int64_t dst_nstride, int dst_pitch,
                      dcfp_stream_t stream);
/* dx = g + sum over levels (as given), bins i ascending, j ascending of dp[bin] / area[bin] over the bins whose
 * window holds (y, x).  g (nullable: zero) is read in place, dense or row-pitched (g_nstride 0: C*H*pitch);
 * dx [N, C, H, W] is dense. */
int dcfp_ppm_pool_adjoint_f32(const float* dp, int N, int C, int H, int W, int nlev, const int* level_hw,
                              const float* g, int64_t g_nstride, int g_pitch, float* dx, dcfp_stream_t stream);
/* The adjoint of F.interpolate(bilinear, align_corners) from small grids: dp[n, c, i, j] =
 * sum_Y sum_X wy(Y, i) * wx(X, j) * g[n, c, Y, X] (Y ascending, X ascending) for nlev levels of level_chw
 * triples (C_l, sh, sw), 1 <= sh, sw <= 8.  g: the sum C_l channels of the levels, in order, read in place from a
 * batch-strided (g_nstride 0: sum C_l * H * pitch), optionally row-pitched tensor; W <= 2048.  dp: level-major
 * blocks [N, C_l, sh, sw]. */
int dcfp_ppm_resize_adjoint_f32(const float* g, int64_t g_nstride, int g_pitch, int N, int H, int W,
                                int nlev, const int* level_chw, float* dp, int align_corners,
                                dcfp_stream_t stream);
/* Fused  F.interpolate -> nn.CrossEntropyLoss(ignore_index, 'mean')
 * (deeplabv3.py:47,50 + loss/criterion.py:60,65-67): never materialises the
 * full-resolution logits.  labels: int64 [N,H,W].
 *   fwd: out[0] = sum over valid pixels of -log_softmax(z)[label];
 *        out[1] = number of valid pixels (as float).
 *   bwd: dlogits[n,c,i,j] = grad_scale * sum_pixels weight*(softmax - onehot),
 *        gathered per low-res cell (deterministic, no atomics).
 * pixel_keep (nullable, uint8 [N,H,W]): 0 => pixel treated as ignored (OHEM). */
size_t dcfp_upsample_ce_workspace_bytes(int N, int H, int W);
/* lse (nullable on fwd): [N,H,W] log-sum-exp of the interpolated logits per pixel,
 * written by fwd and consumed by bwd (33.5 MB at 4x1024x2048 instead of 637 MB of
 * full-resolution logits).  gt_prob (nullable): softmax probability of the label
 * class per pixel (1.0 where the label is ignore_index) — feeds OHEM. */
int dcfp_upsample_ce_fwd_f32(const float* logits, const int64_t* labels,
                             const uint8_t* pixel_keep, int ignore_index,
                             int N, int C, int h, int w, int H, int W, int align_corners,
                             float* lse, float* gt_prob, float* out2,
                             void* workspace, size_t workspace_bytes,
                             dcfp_stream_t stream);
int dcfp_upsample_ce_bwd_f32(const float* logits, const int64_t* labels,
                             const uint8_t* pixel_keep, int ignore_index,
                             int N, int C, int h, int w, int H, int W, int align_corners,
                             const float* lse, const float* grad_scale /* device scalar */,
                             float* dlogits, dcfp_stream_t stream);
/* Which kernel dcfp_upsample_ce_bwd_f32 and dcfp_upsample_wce_bwd_f32 launch at this shape (both make this decision):
 *   variant 0 "cells19"        C == 19: the cell-organised kernel with all 19 classes in registers; 19, 1
 *           1 "cells_chunked"  the same kernel per class window of chunk_width classes, chunks = ceil(C / chunk_width)
 *                              windows in one launch
 *           2 "per_output"     one thread per dlogits element (DCFP_CE_BWD_CELLS=0, C == 1, or a block count
 *                              beyond 32 bits); chunk_width = chunks = 0. */
int dcfp_upsample_ce_bwd_plan(int N, int C, int h, int w, int H, int W, int* variant, int* chunk_width, int* chunks);

/* OHEM threshold input (loss/ohem.py:20-33): per position of the 1/factor-zoomed grid
 * (H8 x W8 = round(H/factor) x round(W/factor), scipy.ndimage.zoom coordinates) the nearest
 * label (lab8) and the order-1-zoomed softmax probability of that label (pred8), computed from
 * the low-resolution logits and the LSE map of dcfp_upsample_ce_fwd_f32. */
int dcfp_ohem_zoom_gt_prob_f32(const float* logits, const int64_t* labels, const float* lse,
                               int N, int C, int h, int w, int H, int W, int align_corners,
                               int H8, int W8, float* pred8, int32_t* lab8,
                               dcfp_stream_t stream);

/* OHEM threshold (loss/ohem.py:34-48, np.partition on the host in the reference) on the device:
 *   num_valid = #(lab8 != ignore_label) over the n zoomed positions;
 *   min_kept >= num_valid -> 1.0;  min_kept <= 0 -> thresh;  otherwise
 *   kth = the (min(num_valid, min_kept)-1)-th smallest pred8 among valid positions (exact radix
 *   select), *threshold = kth > thresh ? kth : thresh.  min_kept is the reference's
 *   `self.min_kept // (factor*factor)`.  threshold: ONE float in device memory, consumed by
 *   dcfp_ohem_keep_mask_u8 without a host round trip. */
int dcfp_ohem_threshold_f32(const float* pred8, const int32_t* lab8, int64_t n, int ignore_label,
                            float thresh, int64_t min_kept, float* threshold /* device scalar */,
                            dcfp_stream_t stream);
/* keep[i] = gt_prob[i] <= *threshold (loss/ohem.py:69 kept_flag) over the n full-resolution pixels:
 * the pixel_keep mask of dcfp_upsample_ce_{fwd,bwd}_f32.  gt_prob 16-byte, keep 4-byte aligned. */
int dcfp_ohem_keep_mask_u8(const float* gt_prob, const float* threshold /* device scalar */, int64_t n,
                           uint8_t* keep, dcfp_stream_t stream);

/* GSRL fine-tune loss (loss/criterion.py:77-101), fused the same way as the CE above:
 *   margin[pix]  = p1 - p2, the two largest softmax probabilities of the interpolated logits
 *                  (replaces softmax + sort over the full-resolution tensor, :89-91);
 *   maxfilter    = F.max_pool2d(weight, k, stride=1, padding=k/2) of the balance weights (:88);
 *   wce fwd/bwd  = CE(reduction='none') * pix_weight, summed per image:
 *                  out_per_image[n] = (sum w*ce, sum w); bwd scales image n by
 *                  grad_scale_per_image[n] (:94-99: per-image normalisation, mean over images). */
int dcfp_upsample_margin_f32(const float* logits, int N, int C, int h, int w, int H, int W,
                             int align_corners, float* margin, dcfp_stream_t stream);
int dcfp_maxfilter2d_s1_f32(const float* x, float* y, int planes, int H, int W, int k,
                            dcfp_stream_t stream);
size_t dcfp_upsample_wce_workspace_bytes(int N, int H, int W);
int dcfp_upsample_wce_fwd_f32(const float* logits, const int64_t* labels, const float* pix_weight,
                              int ignore_index, int N, int C, int h, int w, int H, int W,
                              int align_corners, float* lse, float* out_per_image,
                              void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
int dcfp_upsample_wce_bwd_f32(const float* logits, const int64_t* labels, const float* pix_weight,
                              int ignore_index, int N, int C, int h, int w, int H, int W,
                              int align_corners, const float* lse,
                              const float* grad_scale_per_image, float* dlogits,
                              dcfp_stream_t stream);

/* Evaluation (evaluate.py:229-247,340-372): pred = argmax_c F.interpolate(logits)[c] per pixel
 * (never materialising the full-resolution logits) and the class confusion matrix
 * conf[gt*C + pred] += 1 over pixels with gt != ignore_index (int64, integer atomics: exact). */
int dcfp_upsample_argmax_f32(const float* logits, int N, int C, int h, int w, int H, int W,
                             int align_corners, int32_t* pred, dcfp_stream_t stream);
int dcfp_confusion_matrix_i64(const int32_t* pred, const int64_t* gt, int ignore_index,
                              int64_t n_pixels, int C, int64_t* conf /* [C*C], accumulated */,
                              dcfp_stream_t stream);

/* The multi-scale + flip vote of evaluate.py:198-227 with whole=True, fused with the argmax and the confusion matrix
 * above into one launch (vote.hip).  Every map is the network's low-resolution logits of one (scale, flip)
 * pass.  For y < out_h, x < out_w:
 *   score[n,c,y,x] = sum_k weight_k * sum_{(Y,wY) in lerp(y: hs_k -> H)} sum_{(X,wX) in lerp(x: ws_k -> W)}
 *                    wY * wX * U_k(c, Y, flip_k ? ws_k-1-X : X)
 * where U_k(c, Y, X') is the bilinear value of logits_k[n,c] resized from (h_k, w_k) to (hs_k, ws_k) at (Y, X'); all
 * four index computations follow the coordinate rule of the upsample kernels.  pred = the first maximum of score over
 * c; conf[gt*C + pred] += 1 where gt != ignore_index and 0 <= gt < C (C <= 1024 with conf).  scores
 * [N,C,out_h,out_w], pred [N,out_h,out_w] and conf [C*C] (accumulated; needs gt [N,out_h,out_w]) are optional, at
 * least one of them is asked for.  The N x C x hs x ws logits never exist.  No float atomics, a fixed summation
 * order: two calls give the same bits.  `maps` is a HOST array of n_maps <= 16 records (logits: device pointer),
 * validated here before the launch (DCFP_E_BADDESC) and passed by value. */
typedef struct DcfpVoteMap {
    const float* logits;   /* [N, C, h, w] dense fp32: net.lowres_logits of the resized (and maybe mirrored) image */
    int h, w;              /* its size */
    int hs, ws;            /* size of the image the network saw = size its logits are upsampled to */
    int flip;              /* 1: the network saw the image mirrored along x */
    float weight;          /* 1/len(scales), or 0.5/len(scales) for each map of a flip pair */
} DcfpVoteMap;
int dcfp_vote_multiscale_f32(const DcfpVoteMap* maps, int n_maps, int N, int C,
                             int H, int W,          /* the grid the reference votes on (image size after pad_inf) */
                             int out_h, int out_w,  /* top-left crop that is produced, <= H, W */
                             int align_corners,
                             float* scores,         /* optional [N, C, out_h, out_w] */
                             int32_t* pred,         /* optional [N, out_h, out_w] */
                             const int64_t* gt, int ignore_index,   /* optional [N, out_h, out_w] */
                             int64_t* conf,         /* optional [C*C], accumulated; needs gt */
                             dcfp_stream_t stream);

/* Sliding-window evaluation (evaluate.py:145-184 under evaluate.py:198-227, whole=False; slide.hip).
 *
 * The tile grid is separable: tile t = r * cols + c has its origin at (ys[r], xs[c]) and covers
 * [ys[r], min(ys[r] + th, h)) x [xs[c], min(xs[c] + tw, w)); at most 32 origins per axis.
 *
 * dcfp_gather_tiles_f32: all rows * cols zero-padded tiles of image [N,channels,h,w] in one launch, tiles
 * [rows*cols, N, channels, th, tw]; with flip != 0 the tiles of the image mirrored along x (which is never formed).
 * ys / xs are HOST arrays, checked (0 <= origin < size) and passed by value.  `tiles` must be 16-byte aligned (it is
 * written in 16-byte stores), DCFP_E_BADDESC otherwise. */
#define DCFP_SLIDE_MAX_PASSES 16
#define DCFP_SLIDE_MAX_TILES_PER_AXIS 32
int dcfp_gather_tiles_f32(const float* image, int N, int channels, int h, int w,
                          const int32_t* ys, int rows, const int32_t* xs, int cols,
                          int th, int tw, int flip, float* tiles, dcfp_stream_t stream);

/* dcfp_vote_sliding_f32: the vote of dcfp_vote_multiscale_f32 over sliding-window passes, one launch.  A pass holds
 * the network's low-resolution logits on every padded tile of the image resized to hs x ws (mirrored along x when
 * flip).  For y < out_h, x < out_w:
 *   score[n,c,y,x] = sum_k weight_k * sum_{(Y,a) in lerp(y: hs_k -> H)} sum_{(X,b) in lerp(x: ws_k -> W)}
 *                    a * b * S_k(n, c, Y, flip_k ? ws_k-1-X : X)
 *   S_k(n,c,Y,X)   = 1/cnt_k(Y,X) * sum_{tiles t covering (Y,X)} U_kt(n, c, Y - y1_t, X - x1_t)
 *   U_kt           = logits_k[t,n,c] resized bilinearly (lh, lw) -> (th, tw), always the full padded tile size
 * with cnt_k the number of covering tiles (any number per axis).  scores / pred / gt / conf, the first-maximum rule,
 * the limits on C and the bit-for-bit repeatability are those of dcfp_vote_multiscale_f32.
 * The origins travel apart from the records: origins_host and origins_dev are the same table of n_passes x 64 int32
 * (per pass 32 row origins, then 32 column origins, unused entries 0), once in host memory - validated here before
 * the launch: sorted, inside the image, no pixel of [0,hs) x [0,ws) uncovered - and once in device memory, which the
 * kernel reads.  `passes` is a HOST array of n_passes <= 16 records, passed by value.  DCFP_E_BADDESC otherwise. */
typedef struct DcfpSlidePass {
    const float* logits;   /* [rows*cols, N, C, lh, lw] dense fp32 */
    int lh, lw;            /* size of one tile's logits */
    int hs, ws;            /* size of the resized image the tiles were cut from */
    int th, tw;            /* the (padded) tile size the network saw */
    int rows, cols;        /* tile grid, 1 .. 32 each */
    int flip;              /* 1: the tiles were cut from the image mirrored along x */
    float weight;          /* 1/len(scales), or 0.5/len(scales) for each pass of a flip pair */
} DcfpSlidePass;
int dcfp_vote_sliding_f32(const DcfpSlidePass* passes, int n_passes,
                          const int32_t* origins_host, const int32_t* origins_dev,
                          int N, int C,
                          int H, int W,          /* the grid the reference votes on */
                          int out_h, int out_w,  /* top-left crop that is produced, <= H, W */
                          int align_corners,
                          float* scores,         /* optional [N, C, out_h, out_w] */
                          int32_t* pred,         /* optional [N, out_h, out_w] */
                          const int64_t* gt, int ignore_index,   /* optional [N, out_h, out_w] */
                          int64_t* conf,         /* optional [C*C], accumulated; needs gt */
                          dcfp_stream_t stream);

/* Boundary IoU (evaluate.py:352-357, utils/edge_utils.py:98-127): the label map with everything but the class
 * boundaries set to `background`.  A pixel is valid if 0 <= label < num_classes; a valid pixel is interior if
 * the whole (2d+1)x(2d+1) window centred on it lies inside the image and carries its label;
 * out = label where valid and not interior, else background.  [N,H,W] dense, images independent, out != labels.
 * Work per pixel does not depend on d or num_classes (boundary.hip); num_classes <= 255 (one-byte keys). */
size_t dcfp_label_boundary_workspace_bytes(int N, int H, int W);
int dcfp_label_boundary_i32(const int32_t* labels, int32_t* out, int N, int H, int W, int num_classes, int d,
                            int background, void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
int dcfp_label_boundary_i64(const int64_t* labels, int64_t* out, int N, int H, int W, int num_classes, int d,
                            int background, void* workspace, size_t workspace_bytes, dcfp_stream_t stream);

/* ------------------------------------------------- training augmentation
 * The train-split chain of datasets/Base.py:224-261 (id -> trainId, random scale, photometric jitter,
 * input_transform, pad + random crop, mirror, get_label) on the device; DESIGN §13 states the arithmetic.  The host
 * draws the random parameters and folds the geometry into tables; the device gathers.
 *   taps   : device array of records, 16-byte aligned.  A sample's column table is taps[col_off .. col_off+crop_w),
 *            its row table taps[row_off .. row_off+crop_h).  src = source column / row of the left / upper tap, or -1
 *            where the output pixel is padding; c0 + c1 = 2048 weigh src and src + 1 (clamped to the last one);
 *            lsrc = nearest-neighbour source column / row of the label.
 *   lut_a  : device bytes; 256 per sample at lut_a_off (u8 -> u8 before the HSV block), lut_a_off = -1: identity.
 *   lut_b  : device floats; 3 x 256 per sample at lut_b_off: output plane c (R, G, B) of a pixel is
 *            lut_b[lut_b_off + 256*c + u8 of source channel 2 - c].
 *   HSV    : hsv_flags != 0 runs the BGR -> HSV -> BGR round trip between the two tables: saturation S =
 *            clip(rint(S * sat_alpha)) and / or hue H = (H + hue_delta) mod 180.
 *   output : images fp32 [N,3,crop_h,crop_w] (0.0 in the padding); labels int64 [N,crop_h,crop_w] =
 *            id_table[raw id] (id_table: 256 device bytes, NULL = identity; ignore_label, 0 .. 255, in the padding);
 *            hist int32 [N,256] = per-sample count of every label value of the crop, padding included (zeroed here).
 *            labels and hist may be NULL together (test split); hist alone may be NULL.
 * `samples` is a HOST array of N records (their pointers are device pointers): it is validated here, before any
 * launch, and travels by value in the kernel argument, 16 records per launch.  16-byte stores are used when crop_w is
 * a multiple of 4 and images / labels are 16-byte aligned; any source address and size works. */
#define DCFP_AUG_SATURATION 1
#define DCFP_AUG_HUE 2
typedef struct DcfpAugTap {
    int32_t src, c0, c1, lsrc;
} DcfpAugTap;
typedef struct DcfpAugSample {
    const uint8_t* image;       /* BGR uint8 [src_h, src_w, 3], dense                          */
    const uint8_t* label;       /* raw ids uint8 [src_h, src_w], dense; NULL without labels     */
    int32_t src_h, src_w;
    int32_t col_off, row_off;   /* first record of the column / row table in taps              */
    int32_t lut_a_off;          /* bytes into lut_a, or -1                                     */
    int32_t lut_b_off;          /* floats into lut_b                                           */
    int32_t hsv_flags;          /* DCFP_AUG_SATURATION | DCFP_AUG_HUE                          */
    int32_t hue_delta;
    float sat_alpha;
    int32_t pad_;
} DcfpAugSample;
int dcfp_augment_u8_to_f32_nchw(const DcfpAugSample* samples, int N, int crop_h, int crop_w, const DcfpAugTap* taps,
                                int64_t n_taps, const uint8_t* lut_a, int64_t lut_a_bytes, const float* lut_b,
                                int64_t lut_b_floats, const uint8_t* id_table, int ignore_label, float* images,
                                int64_t* labels, int32_t* hist, dcfp_stream_t stream);
/* get_label (Base.py:73-89) from the histogram above: per sample, with n_c = hist[n][c] for c < num_classes,
 *   balance 1: w_c = clip(1 / (n_c + 1), 0, 1)
 *   balance 2: w_c = clip((1 + 1e-8 - beta^n_t) / (1 + 1e-8 - beta^n_c), 0, 1), t = target_class[n] (device int32 [N];
 *              a target outside 0 .. num_classes-1 gives the sample weight 0)
 * in fp64, rounded once; weight fp32 [N, pixels] = w[label], 0 where the label is ignore_label or no class.
 * balance 0 computes nothing (the reference returns the plain label); balance outside 0 .. 2 is DCFP_E_BADDESC. */
int dcfp_balance_weight_f32(const int64_t* labels, const int32_t* hist, const int32_t* target_class, int N,
                            int64_t pixels, int num_classes, int ignore_label, int balance, double beta, float* weight,
                            dcfp_stream_t stream);

/* ------------------------------------------ connected components (resample sampler)
 * The crop location of the `resample` sampler (Base.py:203-222): the 8-connected components of one class
 * on the scaled, padded label grid, and the k-th pixel of a chosen component.  For a sample the grid is Hp x Wp
 * (Hp >= dst_h, Wp >= dst_w); pixel (y, x) is foreground iff y < dst_h, x < dst_w and
 *   id_table[label[maps[row_off + y] * src_w + maps[col_off + x]]] == cls
 * (maps: device int32, the nearest-neighbour source row / column of every destination row / column, clamped to the
 * source; id_table: 256 device bytes, NULL = identity).  Everything outside dst_h x dst_w is background.
 * The label of a component is the smallest linear index y*Wp + x among its pixels; components are numbered 1 .. C in
 * ascending order of that label; the pixels of a component are ordered by linear index.  Integer arithmetic only: the
 * result is defined bit for bit and does not depend on the order in which blocks run.
 * A sample owns the slice [work_off, work_off + dcfp_components_workspace_bytes(Hp, Wp)) of the work buffer (work_off a
 * multiple of 16); as int32 it holds, each region starting on a multiple of 4 entries, with P = Hp*Wp, P8 = P rounded up
 * to 8, cap = ceil(Hp/2)*ceil(Wp/2) (the most components 8-connectivity allows), nblk = ceil(P/2048):
 *   [0, P)                    the label map (-1 background)
 *   [P8, P8 + P)              scratch; at a component's label, its pixel count
 *   [2*P8, +cap)              the labels of components 1 .. C, ascending
 *   [2*P8 + up4(cap), +cap)   their pixel counts
 *   then 2 * up4(nblk)        scan scratch
 * `samples` is a HOST array of N records (label: device pointer), validated here before any launch
 * (DCFP_E_BADDESC) and passed by value, 16 records per launch; samples may differ in every field.  counts: device
 * int32 [N], the component count of every sample.  No host synchronisation inside either entry point. */
typedef struct DcfpCcSample {
    const uint8_t* label;       /* raw ids uint8 [src_h, src_w], dense                          */
    int32_t src_h, src_w;
    int32_t dst_h, dst_w;       /* the scaled size                                             */
    int32_t Hp, Wp;             /* max(dst, crop): the padded grid                             */
    int32_t row_off, col_off;   /* first entry of the row / column map in maps                 */
    int32_t cls;                /* 0 .. 255                                                    */
    int32_t pad_;
    int64_t work_off;           /* bytes into the work buffer                                  */
} DcfpCcSample;
size_t dcfp_components_workspace_bytes(int Hp, int Wp);
int dcfp_label_components_u8(const DcfpCcSample* samples, int N, const int32_t* maps, int64_t n_maps,
                             const uint8_t* id_table, void* work, size_t work_bytes, int32_t* counts,
                             dcfp_stream_t stream);
/* yx int32 [N,2] = (y, x) of the k[s]-th pixel (0-based, linear-index order) of component n[s] (1-based) of a labelled
 * batch; (-1, -1) where n[s] == 0 (skipped), n[s] > counts[s] or k[s] is not below the component's size.  n, k, counts:
 * device int32 [N].  Reads the label map once plus one 2048-pixel segment per sample. */
int dcfp_component_pixel_i32(const DcfpCcSample* samples, int N, void* work, size_t work_bytes, const int32_t* counts,
                             const int32_t* n, const int32_t* k, int32_t* yx, dcfp_stream_t stream);

/* ------------------------------------------------------------- EIC score
 * dcfp_pruning.step (pruners/dcfp_pruner.py:15-20), all scored BN layers in one
 * launch.  table: device array of n_layers records; eic is updated in place:
 *   flag = (g*gamma > 0); t = flag ? |g| : eic; eic = eic*r + t*(1-r)
 * evaluated exactly in the reference's operation order (two roundings). */
typedef struct DcfpEicEntry {
    const float* gamma;
    const float* grad;
    float* eic;
    int32_t n;
    int32_t pad_;
} DcfpEicEntry;
int dcfp_eic_update_f32(const DcfpEicEntry* table, int n_layers, float r,
                        float one_minus_r /* float(1.0 - double(r)), as torch casts it */,
                        dcfp_stream_t stream);

/* --------------------------------------------------------- SGD (momentum)
 * torch.optim.SGD step as built by optimizer.py:24-25 over a list of tensors:
 *   g' = g + wd*p ; buf = first ? g' : mom*buf + g' ; p -= lr*buf. */
typedef struct DcfpSgdEntry {
    float* param;
    const float* grad;
    float* momentum_buf;
    int64_t n;
    int64_t first_chunk; /* prefix sum of ceil(n / DCFP_SGD_CHUNK) over earlier entries */
    float weight_decay;
    int32_t pad_;
} DcfpSgdEntry;
#define DCFP_SGD_CHUNK 16384
int dcfp_sgd_momentum_f32(const DcfpSgdEntry* table, int n_tensors, int64_t total_chunks,
                          float lr, float momentum, int first_step, dcfp_stream_t stream);

/* ------------------------------------------------------------------ AdamW
 * torch.optim.AdamW step (decoupled weight decay, no amsgrad, no maximize) over a list of tensors that share one
 * step count, in the order of torch's single-tensor implementation:
 *   p *= 1 - lr*wd ; m = lerp(m, g, 1-beta1) ; v = beta2*v + (1-beta2)*g*g ;
 *   denom = sqrt(v)/bias_correction2_sqrt + eps ; p -= (lr/bias_correction1) * m/denom
 * One launch over the device table, one block per DCFP_SGD_CHUNK elements of one tensor.  1 - lr*wd, lr/bc1,
 * 1 - beta1 and 1 - beta2 are formed in double here and rounded once; every scalar is passed by value, so a
 * learning rate or weight decay that changes every step needs no new table.  Entries whose four pointers are all
 * 16-byte aligned take 16-byte loads and stores, the others (and the last n % 4 elements) a scalar path with the
 * same bits per element.  grad is only read; nothing is written past n.  DCFP_E_BADDESC: negative counts,
 * total_chunks > 2^31-1, null table; n_tensors == 0 or total_chunks == 0: DCFP_OK, no launch. */
typedef struct DcfpAdamEntry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t n;
    int64_t first_chunk; /* prefix sum of ceil(n / DCFP_SGD_CHUNK) over earlier entries */
} DcfpAdamEntry;
int dcfp_adamw_f32(const DcfpAdamEntry* table, int n_tensors, int64_t total_chunks,
                   float lr, float beta1, float beta2, float eps, float weight_decay,
                   float bias_correction1, float bias_correction2_sqrt, dcfp_stream_t stream);

/* ------------------------------------- gradient-norm clipping and weight EMA (csrc/clip_ema.hip)
 * dcfp_grad_norm_f32: the global L2 norm of n_tensors gradient tensors and torch.nn.utils.clip_grad_norm_'s
 * coefficient, on the device.  table: DEVICE array of records, first_chunk the prefix sum of ceil(n / DCFP_SGD_CHUNK)
 * as in the step tables; data at any 4-byte aligned address (16-byte loads from the first 16-byte boundary on).
 * Every element is converted to double, squared (exact) and accumulated in double: launch 1 leaves one partial per
 * chunk in the workspace (dcfp_grad_norm_workspace_bytes(total_chunks) bytes, 8-byte aligned), launch 2 - one block -
 * adds each tensor's partials in ascending chunk order (tensor_sq[i], device, nullable; the workspace is scratch and
 * is overwritten), then the tensors in ascending order, and writes
 *   result->sqnorm ; result->norm = (float)sqrt(sqnorm) ;
 *   c = max_norm / (norm + 1e-6f), each operation rounded once ; result->coef = c > 1 ? 1 : c
 * so a NaN norm gives a NaN coefficient and an infinite one 0 (error_if_nonfinite=False).  No atomics: two calls on
 * the same inputs leave the same bits.  n_tensors == 0 writes {0, 0, 1}.  DCFP_E_BADDESC: null table with a positive
 * count, negative counts, total_chunks > 2^31-1, max_norm not > 0 (NaN included), result null or result / tensor_sq
 * not 8-byte aligned; DCFP_E_WORKSPACE: a workspace that is needed and null, not 8-byte aligned or too small.  All of
 * it is checked before any HIP call.
 *
 * dcfp_sgd_momentum_ex_f32 / dcfp_adamw_ex_f32: dcfp_sgd_momentum_f32 / dcfp_adamw_f32 (the same per-element code)
 * with two optional additions in the same launch:
 *   coef (device, nullable): the gradient enters as g * *coef, rounded once - torch's g.mul_(clip_coef); grad itself
 *     is only read;
 *   ema (per entry, nullable) and ema_w = float(1.0 - double(decay)), 0 <= ema_w < 0.5: after the new parameter value
 *     is formed, ema = ema + ema_w * (p_new - ema) with torch.lerp's bits (one subtraction, one fma).
 * Entries whose pointers (ema included) are all 16-byte aligned take 16-byte loads and stores, the others (and the
 * last n % 4 elements) a scalar path with the same bits per element; nothing is written past n.  With coef null and
 * no ema pointers the results equal the plain entry points' bit for bit.  DCFP_E_BADDESC: negative counts,
 * total_chunks > 2^31-1, ema_w outside [0, 0.5), null table; n_tensors == 0 or total_chunks == 0: DCFP_OK, no launch. */
typedef struct DcfpNormEntry {
    const float* data;
    int64_t n;
    int64_t first_chunk; /* prefix sum of ceil(n / DCFP_SGD_CHUNK) over earlier entries */
} DcfpNormEntry;
typedef struct DcfpGradNorm {
    double sqnorm;
    float norm;
    float coef;
} DcfpGradNorm;
size_t dcfp_grad_norm_workspace_bytes(int64_t total_chunks);
int dcfp_grad_norm_f32(const DcfpNormEntry* table, int n_tensors, int64_t total_chunks, float max_norm,
                       void* workspace, size_t workspace_bytes, double* tensor_sq, DcfpGradNorm* result,
                       dcfp_stream_t stream);
typedef struct DcfpSgdExEntry {
    float* param;
    const float* grad;
    float* momentum_buf;
    float* ema;          /* nullable */
    int64_t n;
    int64_t first_chunk;
    float weight_decay;
    int32_t pad_;
} DcfpSgdExEntry;
int dcfp_sgd_momentum_ex_f32(const DcfpSgdExEntry* table, int n_tensors, int64_t total_chunks, float lr,
                             float momentum, int first_step, const float* coef, float ema_w, dcfp_stream_t stream);
typedef struct DcfpAdamExEntry {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    float* ema;          /* nullable */
    int64_t n;
    int64_t first_chunk;
} DcfpAdamExEntry;
int dcfp_adamw_ex_f32(const DcfpAdamExEntry* table, int n_tensors, int64_t total_chunks, float lr, float beta1,
                      float beta2, float eps, float weight_decay, float bias_correction1,
                      float bias_correction2_sqrt, const float* coef, float ema_w, dcfp_stream_t stream);

/* ------------------------------------------------- fp16 deployment engine
 * The frozen half-precision inference path (dcfp_amd/deploy.py; the reference's totrt.py stage).  Activations are
 * NHWC fp16 with a channel pitch that is a multiple of 8; weights are packed once as [Cout8][KH][KW][Cin8] fp16 with
 * the eval-mode BatchNorm scale folded in (zero rows / columns in the padding); accumulation is fp32 on the fp16
 * matrix cores (v_mfma_f32_32x32x16_f16), one rounding to fp16 in the epilogue.
 *   y[n, oy, ox, y_off + co] = relu?(sum_k x * w + shift[co] (+ residual[n, oy, ox, res_off + co]))
 * Cross-correlation, zero padding, square 1x1 or 3x3 filter, stride 1 or 2, any dilation.  Every pointer is 16-byte
 * aligned; x must hold Cin8 valid channels per pixel (x_pitch >= Cin8 apart); N*H*W and N*Hout*Wout < 2^31. */
typedef struct DcfpConvF16Desc {
    int32_t N, H, W;            /* input  [N,H,W,x_pitch], channels 0 .. Cin8-1 read                    */
    int32_t Cin8, x_pitch;      /* multiples of 8                                                      */
    int32_t Cout;               /* output channels written: a multiple of 8 for the fp16 output (the
                                   padded count), the true class count for the fp32 NCHW output; the
                                   packed weight and shift always hold Cout rounded up to 8 rows       */
    int32_t K, stride, pad, dil;/* K = 1 or 3; stride 1 or 2; same in h and w                           */
    int32_t Hout, Wout;         /* (H + 2*pad - dil*(K-1) - 1)/stride + 1                               */
    int32_t y_pitch, y_off;     /* fp16 output: channel pitch and first channel (multiples of 8)        */
    int32_t res_pitch, res_off; /* residual (fp16 NHWC at the output's resolution), when given          */
    int32_t relu;
} DcfpConvF16Desc;
int dcfp_conv2d_fwd_f16_nhwc(const DcfpConvF16Desc* d, const void* x, const void* w_packed, const float* shift,
                             const void* residual /* nullable */, void* y, dcfp_stream_t stream);
/* The classifier's epilogue: y fp32 NCHW dense [N, Cout, Hout, Wout] = acc + bias (no ReLU, no residual; y_*, res_*
 * and relu of the descriptor are ignored), what dcfp_upsample_argmax_f32 / dcfp_upsample_bilinear_fwd_f32 read. */
int dcfp_conv2d_fwd_f16_nhwc_to_f32_nchw(const DcfpConvF16Desc* d, const void* x, const void* w_packed,
                                         const float* bias, float* y, dcfp_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC fp16 (resnet.py:98): C8 channels of x [N,H,W,x_pitch] -> y [N,Ho,Wo,y_pitch]. */
int dcfp_maxpool3x3s2_nhwc_f16(const void* x, void* y, int N, int H, int W, int C8, int x_pitch, int Ho, int Wo,
                               int y_pitch, dcfp_stream_t stream);
/* nn.AdaptiveAvgPool2d(1) on NHWC fp16 (aspp.py:60): y[n, c] = fp16(mean over the HW pixels of x[n, :, c]), summed
 * in fp32 in a fixed order (deterministic).  workspace: dcfp_avgpool_nhwc_f16_workspace_bytes(N, C8, HW). */
size_t dcfp_avgpool_nhwc_f16_workspace_bytes(int N, int C8, int64_t HW);
int dcfp_avgpool_nhwc_f16(const void* x, void* y, int N, int64_t HW, int C8, int x_pitch, int y_pitch,
                          void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
/* Bilinear resize from a 1x1 map = broadcast (aspp.py:76): y[n, p, y_off + c] = v[n, c] for the HW pixels p and
 * c < C8; v rows v_pitch apart.  Channels of y outside the slice are not touched. */
int dcfp_broadcast_nhwc_f16(const void* v, int v_pitch, void* y, int N, int64_t HW, int C8, int y_pitch, int y_off,
                            dcfp_stream_t stream);
/* The engine's input converter: x fp32 NCHW dense [N,C,H,W] -> y fp16 NHWC [N,H,W,C8], channels C .. C8-1 zero. */
int dcfp_nchw_f32_to_nhwc_f16(const float* x, void* y, int N, int C, int H, int W, int C8, dcfp_stream_t stream);
/* F.interpolate(mode='bilinear'), both align_corners modes, on NHWC fp16 (the DeepLabv3+ decoder's resize of the ASPP
 * output, deeplabv3p.py:31, and the PSPNet priors, ppm.py:36): channels 0 .. C8-1 of x [N,h,w,x_pitch] ->
 * y[n, Y, X, y_off + c] of y [N,H,W,y_pitch]; channels of y outside the slice are not touched.  Any h x w -> H x W.
 * PyTorch's index math in fp32 (the weights of dcfp_upsample_bilinear_fwd_f32), fp32 interpolation, one rounding.
 * A 1x1 source gives the bits of dcfp_broadcast_nhwc_f16. */
int dcfp_resize_bilinear_nhwc_f16(const void* x, int N, int h, int w, int C8, int x_pitch, void* y, int H, int W,
                                  int y_pitch, int y_off, int align_corners, dcfp_stream_t stream);
/* nn.AdaptiveAvgPool2d(sizes[k]) for nlev <= 4 levels (sizes 1 .. 8) in one sweep (ppm.py:29): channels
 * x_off .. x_off+C8-1 of x [N,H,W,x_pitch] -> y[k] dense [N, sizes[k], sizes[k], y_pitch[k]], channels 0 .. C8-1.
 * PyTorch's windows (rows floor(i*H/s) .. ceil((i+1)*H/s)-1).  x is read once: pass 1 sums the cells between all the
 * levels' window boundaries in fp32 into the workspace, pass 2 adds a window's cells (rows, then columns, ascending),
 * divides by the area and rounds once.  Fixed order, no atomics.  workspace (16-byte aligned):
 * dcfp_pyramid_pool_nhwc_f16_workspace_bytes(N, H, W, C8, nlev, sizes), 0 for arguments the kernel refuses. */
size_t dcfp_pyramid_pool_nhwc_f16_workspace_bytes(int N, int H, int W, int C8, int nlev, const int* sizes);
int dcfp_pyramid_pool_nhwc_f16(const void* x, int N, int H, int W, int C8, int x_pitch, int x_off, int nlev,
                               const int* sizes, void* const* y, const int* y_pitch, void* workspace,
                               size_t workspace_bytes, dcfp_stream_t stream);

/* ------------------------------------------------- fp8 deployment engine (conv_f8.hip)
 * The calibrated 8-bit inference path of dcfp_amd/deploy.py (build_engine(precision="fp8")).  Every 8-bit value is OCP
 * e4m3fn; every conversion to it clamps the fp32 value to [-448, 448] and rounds to nearest even (subnormals kept).
 * Activations are NHWC fp8 with a channel pitch that is a multiple of 16; weights are packed once as
 * [Cout8][KH][KW][Cin16] fp8 (zero rows / columns in the padding); accumulation is fp32 on the fp8 matrix cores.
 *   y[n, oy, ox, y_off + co] = fp8(relu?(acc * mul[co] + add[co] (+ res_mul * residual[n, oy, ox, res_off + co])))
 * for co < Cout, and exact zeros for co = Cout .. Cout16-1 (Cout16 = Cout rounded up to 16).  mul and add hold Cout
 * rounded up to 8 floats.  Geometry, alignment and size limits are those of DcfpConvF16Desc. */
typedef struct DcfpConvF8Desc {
    int32_t N, H, W;            /* input  [N,H,W,x_pitch], channels 0 .. Cin16-1 read                   */
    int32_t Cin16, x_pitch;     /* multiples of 16                                                     */
    int32_t Cout;               /* the true output channel count (w_packed has Cout rounded up to 8 rows) */
    int32_t K, stride, pad, dil;
    int32_t Hout, Wout;         /* (H + 2*pad - dil*(K-1) - 1)/stride + 1                               */
    int32_t y_pitch, y_off;     /* fp8 output: channel pitch and first channel (multiples of 16)        */
    int32_t res_pitch, res_off; /* residual (fp8 NHWC at the output's resolution), when given           */
    int32_t relu;
    float res_mul;              /* residual scale / output scale                                        */
} DcfpConvF8Desc;
int dcfp_conv2d_fwd_f8_nhwc(const DcfpConvF8Desc* d, const void* x, const void* w_packed, const float* mul,
                            const float* add, const void* residual /* nullable */, void* y, dcfp_stream_t stream);
/* The classifier's epilogue: y fp32 NCHW dense [N, Cout, Hout, Wout] = acc * mul + add (no clamp, ReLU or residual;
 * y_*, res_* and relu of the descriptor are ignored). */
int dcfp_conv2d_fwd_f8_nhwc_to_f32_nchw(const DcfpConvF8Desc* d, const void* x, const void* w_packed, const float* mul,
                                        const float* add, float* y, dcfp_stream_t stream);
/* y[p, y_off + c] = fp8(x[p, c] * scale) for the P pixels of an fp16 NHWC buffer and c < C; channels C .. C16-1 of the
 * slice are zero, bytes of y outside it are not touched.  x_pitch: a multiple of 8, >= C rounded up to 8. */
int dcfp_cast_nhwc_f16_to_f8(const void* x, int x_pitch, void* y, int y_pitch, int y_off, int64_t P, int C,
                             float scale, dcfp_stream_t stream);
/* nn.MaxPool2d(3, 2, 1) on NHWC fp8: compares the decoded values, exact. */
int dcfp_maxpool3x3s2_nhwc_f8(const void* x, void* y, int N, int H, int W, int C16, int x_pitch, int Ho, int Wo,
                              int y_pitch, dcfp_stream_t stream);
/* nn.AdaptiveAvgPool2d(1) from NHWC fp8 to an fp16 vector: y[n, c] = fp16(mean over the HW pixels of x[n, :, c] * scale),
 * summed in fp32 in a fixed order.  workspace: dcfp_avgpool_nhwc_f16_workspace_bytes(N, C16, HW). */
int dcfp_avgpool_nhwc_f8_to_f16(const void* x, void* y, int N, int64_t HW, int C16, int x_pitch, int y_pitch,
                                float scale, void* workspace, size_t workspace_bytes, dcfp_stream_t stream);
/* y[n, p, y_off + c] = fp8(v[n, c] * scale) for the HW pixels p and c < C of an fp16 vector v (rows v_pitch apart, a
 * multiple of 8); channels C .. C16-1 of the slice are zero, bytes of y outside it are not touched. */
int dcfp_broadcast_nhwc_f16_to_f8(const void* v, int v_pitch, void* y, int N, int64_t HW, int C, int y_pitch,
                                  int y_off, float scale, dcfp_stream_t stream);

/* ------------------------------------------------- label maps as PNG streams (png.hip)
 * pred int32 [N,H,W] and P lookup tables uint8 [P][256] (1 <= P <= 4) -> N*P finished zlib streams, stream n*P + p
 * holding the 8-bit image lut[p][pred[n] & 255]: filter type Up on every row, one fixed-Huffman deflate block and an
 * empty stored block per row (every row's piece is whole bytes), run-length matches at distance 1 by a closed-form
 * rule per run, header 78 01, trailer 03 00 + Adler-32.  The uint8 image is never stored.  The streams lie one after
 * the other in `out` (stream s at offsets[s], lengths[s] bytes; both device int64 [N*P]).  Integer arithmetic only,
 * byte-identical between two calls.  H <= 4096, W <= 8192, N*P*H < 2^31, else DCFP_E_UNSUPPORTED.
 *   dcfp_png_deflate_bound(H, W): the largest size of one stream, 2 + H * ((9*(W+1) + 13 + 7)/8 + 4) + 2 + 4
 *       (0 for sizes the encoder refuses); out_bytes >= N*P times it, else DCFP_E_BADDESC.
 *   dcfp_png_deflate_workspace_bytes(N, H, W, P): the workspace (4-byte aligned; 0 for arguments the encoder refuses);
 *       a smaller one is DCFP_E_WORKSPACE.
 * Null pointers, sizes < 1 and P outside 1 .. 4 are DCFP_E_BADDESC; all of it is checked before any HIP call. */
size_t dcfp_png_deflate_bound(int H, int W);
size_t dcfp_png_deflate_workspace_bytes(int N, int H, int W, int P);
int dcfp_png_deflate_labels_i32(const int32_t* pred, int N, int H, int W, const uint8_t* luts, int P, uint8_t* out,
                                size_t out_bytes, int64_t* offsets, int64_t* lengths, void* workspace,
                                size_t workspace_bytes, dcfp_stream_t stream);

/* ------------------------------------------------- knowledge-distillation losses (kd.hip)
 * s (student), t (teacher): fp32 NCHW [N,C,h,w], contiguous, finite; T > 0 the temperature, x' = x / T.
 *   DCFP_KD_PIXEL    L = T^2/(N h w) * sum over pixels of KL(softmax_c(t') || softmax_c(s'))
 *                    dL/ds = T/(N h w) * (softmax_c(s') - softmax_c(t'))
 *   DCFP_KD_CHANNEL  L = T^2/(N C) * sum over (n, c) planes of KL(softmax_yx(t') || softmax_yx(s'))
 *                    dL/ds = T/(N C) * (softmax_yx(s') - softmax_yx(t'))
 * fp32 with the maximum subtracted before every exponential.  One launch writes the per-block sums of KL to the
 * workspace and, when dlogits (nullable, [N,C,h,w]) is given, the gradient; a second adds the partials in fp64 in a
 * fixed order into *loss_out.  No atomics: two calls on the same inputs leave the same bits.  C == 1 (pixel) and
 * h*w == 1 (channel) give loss 0 and gradient 0 exactly, and so does t == s.
 *   dcfp_kd_workspace_bytes: the workspace of a call (4-byte aligned; 0 for arguments the call refuses).
 * Null s / t / loss_out, sizes < 1, T <= 0 or not finite and an unknown mode are DCFP_E_BADDESC; a workspace that is
 * null or too small is DCFP_E_WORKSPACE; more than 2^31 - 1 blocks DCFP_E_UNSUPPORTED.  All of it is checked before
 * any HIP call. */
#define DCFP_KD_PIXEL 0
#define DCFP_KD_CHANNEL 1
size_t dcfp_kd_workspace_bytes(int mode, int N, int C, int h, int w);
int dcfp_kd_fwd_f32(const float* s, const float* t, int mode, int N, int C, int h, int w, float T, void* workspace,
                    size_t workspace_bytes, float* loss_out /* device scalar */, float* dlogits /* may be null */,
                    dcfp_stream_t stream);

/* ------------------------------------------- pair-wise similarity distillation (pairwise.hip)
 * s (student): fp32 NCHW [N,Cs,h,w], contiguous.  t (teacher) over the same N, h, w with Ct channels (Ct != Cs allowed):
 *   DCFP_PA_F32_NCHW  fp32 NCHW [N,Ct,h,w], contiguous (t_pitch is not read)
 *   DCFP_PA_F16_NHWC  fp16 NHWC, pixel (n,y,x) at t + ((n h + y) w + x) * t_pitch halves, t_pitch >= Ct; only the Ct
 *                     channels from t on are read (a channel offset is part of the pointer)
 * Nodes: the mean of every pool x pool window (the last ones clipped to the map; P = ceil(h/pool) ceil(w/pool)),
 * normalised over the channels, f_p = u_p / r_p, and f_p = 0 where r_p^2 <= 1e-12 (a dead node: no gradient).
 *   L = 1/(N P^2) * sum_n sum_pq (f^S_p . f^S_q - f^T_p . f^T_q)^2,  diagonal included
 * fp32 on the f32-input matrix cores; the loss partials are added in fp64 in a fixed order.  No atomics: two calls leave
 * the same bits.  t == s (the same fp32 tensor) gives loss 0 and gradient 0 exactly.
 *   dcfp_pairwise_fwd_f32: the loss into *loss_out.  with_grad != 0 also leaves in the workspace what the backward call
 *     reads (the node matrix, its scales and the N x Ppad x Ppad difference matrix, Ppad = P rounded up to 128).
 *   dcfp_pairwise_bwd_f32: on the workspace of a with_grad forward call with the same sizes, untouched since:
 *     dstudent [N,Cs,h,w] = dL/ds * grad_out[0] (grad_out: device scalar, null = 1), every element written once; the
 *     scalar is the last factor, so the result is the unscaled one times it, bit for bit.
 *   dcfp_pairwise_workspace_bytes: the workspace of a forward call (with_grad != 0: of a forward + backward pair); 0
 *     for arguments the calls refuse.
 * Null s / t / loss_out / dstudent, sizes or pool < 1, an unknown layout and t_pitch < Ct are DCFP_E_BADDESC; a workspace
 * that is null, too small or not 16-byte aligned DCFP_E_WORKSPACE; N > 65535, h w or a launch grid beyond 2^31 - 1
 * DCFP_E_UNSUPPORTED.  All of it is checked before any HIP call. */
#define DCFP_PA_F32_NCHW 0
#define DCFP_PA_F16_NHWC 1
size_t dcfp_pairwise_workspace_bytes(int N, int Cs, int Ct, int h, int w, int pool, int with_grad);
int dcfp_pairwise_fwd_f32(const float* s, const void* t, int t_layout, long long t_pitch, int N, int Cs, int Ct, int h,
                          int w, int pool, void* workspace, size_t workspace_bytes, float* loss_out /* device scalar */,
                          int with_grad, dcfp_stream_t stream);
int dcfp_pairwise_bwd_f32(int N, int Cs, int Ct, int h, int w, int pool, void* workspace, size_t workspace_bytes,
                          const float* grad_out /* device scalar, may be null */, float* dstudent, dcfp_stream_t stream);

/* ------------------------------------------------ baseline pruning criteria (csrc/score.hip)
 * One fp32 score per output channel of every scored BatchNorm layer; larger means keep.  Every entry point takes a
 * DEVICE array of records (built on the host, uploaded once), returns DCFP_OK for a count of 0 and DCFP_E_BADDESC for a
 * null table with a positive count or a negative count (checked before any HIP call), uses no atomics and combines in
 * a fixed order: two calls on the same inputs leave the same bits.
 *
 * Gate kernels: one launch for all layers, one block per layer, n floats each.
 *   dcfp_gate_taylor_f32   t = fadd(fmul(gamma, ggrad), fmul(beta, bgrad)); score = fadd(score, fmul(t, t))
 *                          (Molchanov et al. 2019 on the BN gate; the caller divides by its step count)
 *   dcfp_gate_l1reg_f32    ggrad = fadd(ggrad, fmul(lambda, sign(gamma))), sign(0) = 0 and ggrad then stays as it is
 *                          (the sparsity term of Liu et al. 2017, added to the gradient before the optimizer step)
 * Every product and sum is rounded on its own, in this order: a float32 restatement done one operation at a time gives
 * the same bits, and exact zeros stay exact (the contract of dcfp_eic_update_f32). */
typedef struct DcfpGateEntry {
    const float* gamma;
    const float* beta;
    float* ggrad; /* written by dcfp_gate_l1reg_f32 only */
    const float* bgrad;
    float* score; /* dcfp_gate_taylor_f32 only; dcfp_gate_l1reg_f32 reads gamma and ggrad alone */
    int32_t n;
    int32_t pad_;
} DcfpGateEntry;
int dcfp_gate_taylor_f32(const DcfpGateEntry* table, int n_layers, dcfp_stream_t stream);
int dcfp_gate_l1reg_f32(const DcfpGateEntry* table, int n_layers, float lambda, dcfp_stream_t stream);

/* Row reductions over MANY matrices in one launch: entry = `rows` rows of K contiguous floats (a conv weight
 * [C, Cin, kh, kw] is C rows of K = Cin*kh*kw), any 4-byte aligned base, any K >= 1.
 *   DCFP_FILTER_ABS_SUM     out[r]  = sum_k |w[r,k]|            (g unused, may be null)
 *   DCFP_FILTER_L2          out[r]  = sqrt(sum_k w[r,k]^2)      (g unused, may be null)
 *   DCFP_FILTER_DOT_SQ_ACC  out[r] += (sum_k w[r,k]*g[r,k])^2   (first-order Taylor on the filter)
 * The split rule: a row is summed by a GROUP of G lanes, G = 8 for K <= 32, 16 for K <= 128, 64 for K <= 1024 and 256
 * above; a block of 256 threads is one UNIT of 256/G rows.  dcfp_filter_reduce_units(rows, K) is the unit count of an
 * entry (0 for sizes < 1); first_unit is the prefix sum of it over the earlier entries and total_units the sum over
 * all.  Units past an entry's rows do nothing, so a wrong prefix gives wrong sums but touches no other memory. */
#define DCFP_FILTER_ABS_SUM 0
#define DCFP_FILTER_L2 1
#define DCFP_FILTER_DOT_SQ_ACC 2
typedef struct DcfpFilterEntry {
    const float* w;
    const float* g;
    float* out;
    int32_t rows;
    int32_t K;
    int64_t first_unit;
} DcfpFilterEntry;
int64_t dcfp_filter_reduce_units(int rows, int K);
int dcfp_filter_reduce_f32(const DcfpFilterEntry* table, int n_entries, int64_t total_units, int op,
                           dcfp_stream_t stream);

/* FPGM (He et al. 2019): out[i] = sum_j sqrt(sum_k (w[i,k] - w[j,k])^2) for MANY matrices [C, K] in two launches.
 * Distances are sums of squared DIFFERENCES (never n_i + n_j - 2 G_ij): equal rows are at distance exactly 0, no
 * distance is NaN for finite input, C = 1 gives 0.  Launch 1: one block per (i tile, j tile) of DCFP_FPGM_TILE rows
 * each, K in LDS chunks, writes the row sums over its j tile to the workspace; launch 2: one block per matrix adds
 * them, j tiles ascending.  An entry's tiles number ceil(C/TILE)^2: first_tile is the prefix sum over the earlier
 * entries, total_tiles the sum.  ws_off: the entry's offset into the workspace in floats, the prefix sum of
 * dcfp_fpgm_workspace_bytes(C) / 4 (a multiple of 64 floats; 0 bytes for C < 1). */
#define DCFP_FPGM_TILE 64
typedef struct DcfpFpgmEntry {
    const float* w;
    float* out;
    int32_t C;
    int32_t K;
    int64_t first_tile;
    int64_t ws_off;
} DcfpFpgmEntry;
size_t dcfp_fpgm_workspace_bytes(int C);
int dcfp_fpgm_f32(const DcfpFpgmEntry* table, int n_entries, int64_t total_tiles, void* workspace,
                  size_t workspace_bytes, dcfp_stream_t stream);

/* ------------------------------------------------ state digest (csrc/digest.hip)
 * A 128-bit digest of a device buffer viewed as n_words 32-bit words w_0 .. w_{n-1}, all arithmetic mod 2^64:
 *   out2[0] = sum_i w_i          out2[1] = sum_i (index_base + i + 1) * w_i
 * Integer sums: the result does not depend on any reduction order (no atomics, the same pair from every call), the
 * words are read as bits (-0.0 and 0.0 differ), a swap of two different words changes out2[1], and a buffer digested
 * in pieces gives the whole's digest as the sum of digest(piece, index_base + the piece's first index).
 * data: any 4-byte aligned device address (16-byte loads from the first 16-byte boundary on).  The body is cut into
 * chunks of DCFP_DIGEST_CHUNK words, at most DCFP_DIGEST_MAX_BLOCKS blocks stride over them and leave 16 bytes each in
 * the workspace; a second one-block launch adds those and the up to 3 + 3 words outside the 16-byte vectors.
 * dcfp_state_digest_workspace_bytes(n_words) is enough at every alignment (0 for n_words < 4).  out2: device, 2 values,
 * 8-byte aligned, written by the second launch on `stream`.
 * n_words == 0 gives (0, 0) and reads nothing.  Null or misaligned data with n_words > 0 and a null or misaligned out2
 * are DCFP_E_BADDESC; a workspace that is needed and null, not 8-byte aligned or too small DCFP_E_WORKSPACE; n_words
 * above 2^60 DCFP_E_UNSUPPORTED.  All of it is checked before any HIP call. */
#define DCFP_DIGEST_CHUNK 4096
#define DCFP_DIGEST_MAX_BLOCKS 2048
size_t dcfp_state_digest_workspace_bytes(size_t n_words);
int dcfp_state_digest_u64(const void* data, size_t n_words, uint64_t index_base, void* workspace,
                          size_t workspace_bytes, uint64_t* out2 /* device, 2 values */, dcfp_stream_t stream);

/* ------------------------------------------------ Lovasz-Softmax loss (csrc/lovasz.hip)
 * The Lovasz-Softmax loss (Berman et al. 2018, classes = 'present') of the bilinearly upsampled logits, with the sort
 * replaced by an integer histogram of quantised errors.  Arguments as dcfp_upsample_ce_*: logits fp32 [N,C,h,w], labels
 * int64 [N,H,W]; a pixel counts when its label lies in [0, C) and is not ignore_index.  bins = B, a power of two in
 * 64 .. 4096.  Per valid pixel and class, with p = exp(z - lse) of the interpolated logits z:
 *     e = (label == c) ? 1 - p : p,   q = min(2^20, floor(e * 2^20 + 0.5)),   b = min(B - 1, q >> (20 - log2 B)).
 *   dcfp_lovasz_hist_f32    writes lse [N,H,W] and, into the workspace, per (class, bin) the counts nF / nB of the
 *                           foreground / background pixels and the sums SF / SB of their q.  Integer atomics only: two
 *                           calls leave the same bits.
 *   dcfp_lovasz_scan_f32    from that workspace: the loss (device scalar) and the weight table fp32 [C][B][2] =
 *                           (wF, wB) / P, P the number of present classes (zeros for an absent class; P == 0 gives
 *                           loss 0 and a zero table); fp64 in a fixed order.
 *   dcfp_lovasz_bwd_f32     dlogits [N,C,h,w] = *grad_scale x dloss/dlogits from logits, labels, lse and the table;
 *                           asum: fp32 [N,H,W] scratch (sum_c a_c p_c per pixel).  A gather, no atomics.
 *   dcfp_lovasz_errors_u32  q of every (n, c, Y, X) as uint32 [N,C,H,W], 0xFFFFFFFF at pixels that do not count.
 * Workspace of dcfp_lovasz_workspace_bytes(C, bins) bytes (0 for arguments the calls refuse), 8-byte aligned, with
 * CB = C * bins:   SF uint64 [CB] | SB uint64 [CB] | nF uint32 [CB] | nB uint32 [CB] | fp64 [CB][2] raw weights |
 * fp64 [C] loss per class | int64 [C] foreground pixels per class.  hist zero-fills and fills the first four, scan
 * reads them and fills the rest.
 * Null pointers, sizes < 1 and bins that are no power of two in 64 .. 4096 are DCFP_E_BADDESC; C > 255 or
 * N*H*W >= 2^31 DCFP_E_UNSUPPORTED; a workspace that is null or too small DCFP_E_WORKSPACE.  All of it is checked before
 * any HIP call. */
size_t dcfp_lovasz_workspace_bytes(int C, int bins);
int dcfp_lovasz_hist_f32(const float* logits, const int64_t* labels, int ignore_index, int N, int C, int h, int w, int H,
                         int W, int align_corners, int bins, float* lse, void* workspace, size_t workspace_bytes,
                         dcfp_stream_t stream);
int dcfp_lovasz_scan_f32(int C, int bins, void* workspace, size_t workspace_bytes, float* loss_out /* device scalar */,
                         float* weights, dcfp_stream_t stream);
int dcfp_lovasz_bwd_f32(const float* logits, const int64_t* labels, int ignore_index, int N, int C, int h, int w, int H,
                        int W, int align_corners, int bins, const float* lse, const float* weights,
                        const float* grad_scale /* device scalar */, float* asum, float* dlogits, dcfp_stream_t stream);
int dcfp_lovasz_errors_u32(const float* logits, const int64_t* labels, int ignore_index, int N, int C, int h, int w,
                           int H, int W, int align_corners, uint32_t* errors, dcfp_stream_t stream);

/* ------------------------------------------------- the C engine runtime (engine_rt.hip, image_u8.hip)
 * A deployment engine as a file a C program loads and runs: deploy.save_flat writes the plan, the tables and one weight
 * blob in a flat little-endian layout; the calls below parse it (trusting nothing in it), size the workspace for an
 * input shape and run the plan through the entry points of the two sections above, in plan order, on `stream` - the
 * same kernels with the same arguments as dcfp_amd.deploy.Engine, hence the same bits.
 *
 * The caller owns every device buffer: the weights (dcfp_engine_weight_bytes, filled by dcfp_engine_upload), the
 * workspace (dcfp_engine_workspace_bytes for the shape; activation slots - buffers with disjoint lifetimes share one,
 * each rounded up to 256 bytes - followed by the pools' partial sums; no byte of it needs initialising), the image
 * and the logits, all 16-byte aligned.  The handle owns host memory only.  A handle is NOT thread-safe: calls on one
 * handle (they update its cache of launch lists) must not overlap; different handles are independent.
 *
 * Errors: a file the parser rejects is DCFP_E_BADDESC with a one-line message in err (errlen bytes, may be null);
 * an input too small for a layer DCFP_E_BADDESC, a size no kernel takes DCFP_E_UNSUPPORTED, a workspace too small
 * DCFP_E_WORKSPACE - each before anything is launched; dcfp_engine_run_u8 on a file without an input table
 * DCFP_E_UNSUPPORTED.  A failing launch returns that kernel's status and nothing further is launched.
 * The full-resolution steps stay separate calls: dcfp_upsample_bilinear_fwd_f32 / dcfp_upsample_argmax_f32 on the
 * logits with dcfp_engine_info_t.align_corner. */
typedef struct dcfp_engine* dcfp_engine_t;
typedef struct dcfp_engine_info_t {
    int32_t format;          /* 1: fp16 engine, 2: fp8 engine                                   */
    int32_t num_classes, in_channels, align_corner;
    int32_t model;           /* 0 simple, 1 deeplabv3, 2 deeplabv3p, 3 psp                      */
    int32_t n_records, n_buffers, n_slots;
    int32_t has_input_table; /* the file carries the uint8 lookup table: dcfp_engine_run_u8 works */
} dcfp_engine_info_t;
/* Host only, no GPU call. */
int dcfp_engine_open(const char* path, dcfp_engine_t* out, char* err, size_t errlen);
int dcfp_engine_open_memory(const void* bytes, size_t n, dcfp_engine_t* out, char* err, size_t errlen);
void dcfp_engine_close(dcfp_engine_t e);
int dcfp_engine_info(dcfp_engine_t e, dcfp_engine_info_t* out);
size_t dcfp_engine_weight_bytes(dcfp_engine_t e);
/* One host-to-device copy of the weight blob (and the input table behind it) on `stream`. */
int dcfp_engine_upload(dcfp_engine_t e, void* dev_weights, dcfp_stream_t stream);
/* The logits of an N x in_channels x H x W input: fp32 NCHW dense [N, *C, *h, *w]. */
int dcfp_engine_output_shape(dcfp_engine_t e, int N, int H, int W, int* C, int* h, int* w);
/* hw_pairs[2b], hw_pairs[2b+1] = height and width of activation buffer b for an H x W input (0, 0: no record writes
 * it); n_pairs >= n_buffers. */
int dcfp_engine_buffer_shapes(dcfp_engine_t e, int H, int W, int* hw_pairs, int n_pairs);
/* 0: the shape is not supported (too small for a layer, or beyond a kernel's limits). */
size_t dcfp_engine_workspace_bytes(dcfp_engine_t e, int N, int H, int W);
/* image_nchw: fp32 [N, in_channels, H, W] dense on the device. */
int dcfp_engine_run_f32(dcfp_engine_t e, const void* dev_weights, const float* image_nchw, int N, int H, int W,
                        void* workspace, size_t workspace_bytes, float* logits_nchw, dcfp_stream_t stream);
/* image_hwc: uint8 [N][H][W][3] on the device, rows row_pitch_bytes >= 3 W apart (images H * row_pitch_bytes apart),
 * normalised by the file's table. */
int dcfp_engine_run_u8(dcfp_engine_t e, const void* dev_weights, const uint8_t* image_hwc, size_t row_pitch_bytes,
                       int N, int H, int W, void* workspace, size_t workspace_bytes, float* logits_nchw,
                       dcfp_stream_t stream);
/* The uint8 input converter: dst[n][y][x][c] = table[c * 256 + src[n][y][x][order[c]]] for c < 3 and exact zeros for
 * c = 3 .. C8-1; src uint8 [N][H][W][3], rows row_pitch_bytes >= 3 W apart, any alignment; table 3 x 256 fp16 on the
 * device (deploy.input_table: fp16((v / 255 - mean[c]) / std[c]), rounded once from fp64), order a HOST array of 3
 * source byte indices (BGR -> RGB is {2, 1, 0}); dst fp16 NHWC [N,H,W,C8], C8 a multiple of 8.  A pure lookup: the
 * result is exact.  3 bytes read and 2 C8 written per pixel. */
int dcfp_image_u8_hwc_to_nhwc_f16(const uint8_t* src, size_t row_pitch_bytes, int N, int H, int W, const void* table,
                                  const int* order, void* dst, int C8, dcfp_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* DCFP_HIP_H */
