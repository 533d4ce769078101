/* utv2.h - C ABI of the MI355X (gfx950) kernels behind the Unbiased-Teacher-v2 training step.
 *
 * The reference (facebookresearch/unbiased-teacher-v2) is pure Python and has no FFI of its own;
 * every entry point below replaces the native op the reference reaches through PyTorch /
 * Detectron2 / fvcore / torchvision at the cited call site (paths relative to the reference
 * root).  Conventions:
 *   - every pointer is a DEVICE pointer owned by the caller unless the name ends in _host;
 *     tensors are contiguous fp32 / int32 / int64 / uint8 as declared;
 *   - activations are NHWC ([N][H][W][C]); conv weights are [Cout][KH][KW][Cin];
 *   - the last argument is the hipStream_t to launch on; nothing synchronises the stream,
 *     nothing allocates; scratch memory is passed in (size from the *_workspace_* twin);
 *   - return 0 on success, -(hipError_t) on a launch failure, -1000 on a bad argument.
 *   - re-entrant; no mutable global state (the A/B environment switches and two one-time kernel attributes are read / set once per
 *     process, thread-safely, and never change a result).
 */
#ifndef UTV2_H
#define UTV2_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

typedef struct ihipStream_t* utv2_stream_t; /* == hipStream_t */

/* ---- convolution (implicit GEMM on v_mfma_f32_32x32x2_f32) ------------------------------------
 * Replaces ATen conv2d fwd / dgrad / wgrad reached from D2 ResNet/FPN, fcos/fcos.py:252-304
 * (towers + prediction convs), backbone/fpn.py:21-22 (P6/P7) and the RCNN heads.
 * y = relu?(conv(x,w) * scale[co] + bias[co] + residual) (+ y when accumulate).
 * Kred = length of one weight row (KH*KW*C, or the 16-padded 208 for the C==4 stem image).
 * in_dil > 1: transposed gather (dgrad of a strided conv) - see ubteacher/hip.py:conv2d_dgrad. */
int utv2_conv2d_nhwc_fwd(const float* x, const float* w, float* y, const float* scale, const float* bias,
                         const float* residual, int N, int H, int W, int C, int K, int KH, int KW, int stride, int pad,
                         int in_dil, int OH, int OW, int relu, int accumulate, int Kred, utv2_stream_t stream);
/* D2 BasicStem conv1 on the zero-padded NHWC4 image (C == 4, weight rows padded to Kred % 16 == 0); y_dtype selects
 * the output element type (UTV2_F32 / UTV2_BF16, defined below) */
int utv2_conv2d_stem_fwd(const float* x, const float* w, void* y, int y_dtype, const float* scale, const float* bias, int N,
                         int H, int W, int K, int KH, int KW, int stride, int pad, int OH, int OW, int relu, int Kred,
                         utv2_stream_t stream);
int utv2_conv2d_wgrad_splits(int N, int OH, int OW, int K, int Kred);
int64_t utv2_conv2d_wgrad_workspace_floats(int N, int OH, int OW, int K, int Kred);
/* dw[K][KH*KW*C] (+)= sum_m dy[m][k] * im2col(x)[m][:]; deterministic split reduction through ws. */
int utv2_conv2d_nhwc_wgrad(const float* x, const float* dy, float* dw, float* ws, int N, int H, int W, int C, int K,
                           int KH, int KW, int stride, int pad, int OH, int OW, int accumulate, utv2_stream_t stream);
/* db[C] (+)= column sums of g[M][C] (conv bias gradient).  ws >= 1024*C floats. */
int utv2_colsum(const float* g, float* db, float* ws, int M, int C, int accumulate, utv2_stream_t stream);
/* wt[ci][KH-1-kh][KW-1-kw][co] = w[co][kh][kw][ci]  (weight image consumed by dgrad) */
int utv2_weight_flip_transpose(const float* w, float* wt, int K, int KH, int KW, int C, utv2_stream_t stream);

/* Multi-level "same" conv on a level-first [sum_l N*H_l*W_l][C] buffer: ONE launch for every FPN level of a
 * shared head (fcos/fcos.py:338-376 loops the towers over the levels; D2 StandardRPNHead likewise).
 * Doubles as its own dgrad (flipped/transposed weights, pad = k-1-pad).  H_host/W_host: host int[nlev]. */
int utv2_conv2d_ml_fwd(const float* x, const float* w, float* y, const float* scale, const float* bias,
                       const float* residual, int nlev, const int* H_host, const int* W_host, int N, int C, int K, int KH,
                       int KW, int pad, int relu, int accumulate, utv2_stream_t stream);
int utv2_conv2d_ml_wgrad(const float* x, const float* dy, float* dw, float* ws, int nlev, const int* H_host,
                         const int* W_host, int N, int C, int K, int KH, int KW, int pad, int accumulate,
                         utv2_stream_t stream);

/* ---- mixed precision (the reference's SOLVER.AMP.ENABLED configs: autocast at engine/trainer.py:194-198,318-349):
 * bf16 operands on v_mfma_f32_32x32x16_bf16, fp32 accumulate, weights from a bf16 mirror of the fp32 master arena.
 * Activations and activation gradients are bf16 in HBM (autocast stores conv outputs in 16 bit too); every tensor
 * argument carries its element type (`*_dtype`: UTV2_F32 or UTV2_BF16) so fp32 tensors - the loss-side head outputs,
 * their gradients, RoIAlign output - enter and leave without a cast pass.  `residual` has y's type.
 * Same contracts as the fp32 entry points otherwise. */
#define UTV2_F32 0
#define UTV2_BF16 1   /* the library's 16-bit float type: bfloat16 in libutv2_hip.so, IEEE fp16 in libutv2_hip_f16.so (the same sources built
                       * with -DUTV2_H16=_Float16; csrc/common.h h16_t) - "bf16" in the names below reads "the 16-bit type" there */
int utv2_conv2d_bf16_supported(int C, int KH, int KW);

/* Measurement aid (bench.py roofline.sustained_clock_ghz; synchronises the device, never on the training path): the shader clock in GHz
 * that workgroup 0 of the LAST persistent-grid multi-level launch (FCOS tower / RPN head) of the 256 x 256 forward / dgrad conv tile ran at (s_memtime ticks per 10 ns
 * s_memrealtime tick over that workgroup's lifetime) and the lifetime in microseconds; 0 / 0 before the first such launch.  The MFMA peak
 * is quoted at 2.4 GHz; under full-chip MFMA load the board's power limit holds the clock at 1.45-1.9 GHz.  No reference counterpart. */
int utv2_conv_clock_probe(double* ghz, double* lifetime_us);
/* NHWC conv on the 16-bit MFMA kernels (a dgrad is the same call over dy with the flipped weights).  w16 = bf16 [K][KH*KW*C], C % 8 == 0.
 * mask (optional, y's type and shape): y = mask > 0 ? conv*scale+bias : 0, before the residual add - the ReLU backward of the
 * layer that produced the input, fused into the dgrad launch that computes its gradient; post_mask (optional, same type and shape):
 * y = post_mask > 0 ? y : 0 AFTER the residual add - the ReLU whose OUTPUT this gradient flows into (a bottleneck's input), so the
 * block that produced that output needs no separate mask pass.
 * rowinfo (optional; in_dil == 1): the per-output-pixel geometry table of utv2_rowinfo_nhwc for this conv, device int32[N*OH*OW][2] - the
 * tile prologues of the bf16-input kernels load their rows' geometry instead of decoding it (2 us of a 70 us tile on the 256-tile kernel).
 * ReLU masks as BIT planes (all optional; 16-bit y, K % 8 == 0): uint8 [N*OH*OW][K / 8], bit q of byte c = channel 8c + q.
 * relu_bits (WRITTEN): bit = the stored output is > 0 - all the backward of the ReLU needs of it; mask_bits / post_mask_bits
 * (read) take the place of mask / post_mask (one form per mask).  The dgrads of a bottleneck (engine/trainer.py's backward
 * through D2 BottleneckBlock) then read K / 8 bytes per pixel for a sign instead of re-reading 2 K bytes of forward activation. */
int utv2_conv2d_nhwc_fwd_bf16_bits(const void* x, int x_dtype, const void* w16, void* y, int y_dtype, const float* scale,
                                   const float* bias, const void* residual, const void* mask, const void* post_mask, int N, int H, int W,
                                   int C, int K, int KH, int KW, int stride, int pad, int in_dil, int OH, int OW, int relu, int accumulate,
                                   const int* rowinfo, void* relu_bits, const void* mask_bits, const void* post_mask_bits,
                                   utv2_stream_t stream);
/* Multi-level KH x KW 'same' conv over a level-first [P][x_pitch] matrix (P = N * sum of H*W over the nlev levels; H_host / W_host: host
 * arrays), optionally over column slices and / or GROUPED (the paired FCOS towers - cls | bbox, two independent 256 -> 256 chains of
 * fcos/fcos.py:252-304 - run as ONE launch per depth): x has row pitch x_pitch elements and group g reads its channels
 * [g*C, (g+1)*C) (C = input channels PER GROUP, C % 8 == 0), w16 = bf16 [K][KH*KW*C], y / residual have row pitch y_pitch >= K.
 * Anything but (groups 1, x_pitch C, y_pitch K, no gn_part, no rowinfo) needs bf16 x, C % 32 == 0, K % 4 == 0, pitches % 8 == 0,
 * (K / groups) % 128 == 0.
 * gn_part (optional; bf16 y, K % 8 == 0): fp32 [ceil(P / 32)][K / 8][2] - per 32-row block and 8-channel group the sum and the sum of
 * squares of y as stored: the statistics pass of the GroupNorm that consumes y (fcos/fcos.py:263-264), see ..._seg_fwd_p32.
 * rowinfo (optional): device int32[P][2], the geometry table of utv2_rowinfo_nhwc for this conv (same k and pad, one call per level). */
int utv2_conv2d_ml_fwd_bf16_g(const void* x, int x_dtype, int x_pitch, const void* w16, void* y, int y_dtype, int y_pitch,
                              const float* scale, const float* bias, const void* residual, int nlev, const int* H_host,
                              const int* W_host, int N, int C, int K, int KH, int KW, int pad, int relu, int accumulate, int groups,
                              float* gn_part, const int* rowinfo, utv2_stream_t stream);
/* The dgrad that produces the gradient of a GroupNorm + ReLU OUTPUT (the FCOS towers' conv -> GN -> ReLU chain, fcos/fcos.py:252-304,
 * in backward): a 16-bit level-first conv as ..._g with dense y (pitch K) whose epilogue applies the ReLU mask - mask_bits: [P * K / 8]
 * bytes, the plane utv2_groupnorm_relu_seg_fwd_p32 wrote - and leaves GroupNorm backward's first reduction, taken while the rows are in
 * registers: gnb_part fp32 [ceil(P / 64)][K][2] = {sum y, sum y * gnb_x} per 64-row block and channel over the rows as stored
 * (gnb_x: [P][K], the GroupNorm's input, 16-bit).  utv2_groupnorm_seg_bwd_p64 finishes the backward from them.
 * C % 64 == 0, KH * KW * C >= 1024, (K / groups) % 128 == 0. */
int utv2_conv2d_ml_fwd_bf16_gnb(const void* x, int x_pitch, const void* w16, void* y, int nlev, const int* H_host, const int* W_host, int N,
                                int C, int K, int KH, int KW, int pad, int groups, const int* rowinfo, const void* mask_bits,
                                const void* gnb_x, float* gnb_part, utv2_stream_t stream);
/* bf16 wgrad (+ fused bias gradient); rowinfo = device int32[M][2] per OUTPUT pixel:
 * {input pixel index of tap (0,0), (W << 16) | mask of the taps that fall inside the image}; KH*KW <= 16 */
int utv2_conv2d_wgrad_bf16_splits(int M, int K, int Kred);
int64_t utv2_conv2d_wgrad_bf16_workspace_floats(int M, int K, int Kred);
/* dw [K][KH*KW*C] (+)= the weight gradient of a conv from x (`x_dtype`, C % 8 == 0) and dy (`dy_dtype`, [M][K], K % 8 == 0); db (optional,
 * [K]) (+)= the column sums of dy; ws: utv2_conv2d_wgrad_bf16_workspace_floats floats of scratch.
 * rowscale (optional, [K]): per-output-channel multiplier of the result (the folded FrozenBN scale: the kernels then
 * consume the gradient of the BN OUTPUT directly); the dgrad weight image takes the same multiplier at flip time.
 * x has pixel pitch x_pitch (C, or wider: a channel slice of a wider matrix), dy row pitch dy_pitch >= K (the first K columns of a
 * zero-padded matrix); groups > 1: dw rows [g*K/groups, (g+1)*K/groups) correlate dy with input channels [g*C, (g+1)*C)
 * (C per group); (K / groups) % 128 == 0, x_pitch >= groups * C */
int utv2_conv2d_wgrad_bf16_g(const void* x, int x_dtype, int x_pitch, const void* dy, int dy_dtype, int dy_pitch, float* dw, float* db,
                             float* ws, const int* rowinfo, const float* rowscale, int M, int C, int K, int KH, int KW, int accumulate,
                             int groups, utv2_stream_t stream);
/* utv2_conv2d_wgrad_bf16_g with its split-K tail (slab reduction, bias reduction) RECORDED in a caller-owned pending table - host memory of
 * utv2_wgrad_fold_table_bytes() bytes, zero-initialised - instead of launched: utv2_wgrad_fold_flush runs the recorded tails of up to 8
 * launches as ONE kernel, with the arithmetic of the separate kernels (bit-identical gradients).  dw / db are valid after the flush on the
 * same stream; every recorded launch needs its own ws until then; two recorded launches must not share dw or db (EARG: flush first).
 * utv2_wgrad_fold_pending: recorded tails (0 = nothing to flush).  The per-layer tails of a backward are 60-70 dispatches of 5-25 us. */
int utv2_conv2d_wgrad_bf16_d(const void* x, int x_dtype, int x_pitch, const void* dy, int dy_dtype, int dy_pitch, float* dw, float* db,
                             float* ws, const int* rowinfo, const float* rowscale, int M, int C, int K, int KH, int KW, int accumulate,
                             int groups, void* pending, utv2_stream_t stream);
int64_t utv2_wgrad_fold_table_bytes(void);
int utv2_wgrad_fold_pending(const void* pending);
int utv2_wgrad_fold_flush(void* pending, utv2_stream_t stream);
/* D2 BasicStem conv1 on bf16 MFMA: xpad16 = bf16 [N][H+6][W+8][4], the normalised NHWC4 image inside a zero border
 * (written by utv2_preprocess_image_bf16pad); w16s = bf16 [K][7][32] (7 taps x 4 channels + 4 zeros per kernel row) */
int utv2_conv2d_stem_fwd_bf16(const void* xpad16, const void* w16s, void* y, int y_dtype, const float* scale,
                              const float* bias, int N, int H, int W, int K, int OH, int OW, int relu, utv2_stream_t stream);
/* the geometry table above, built on the device: out = int32 [N*OH*OW][2] for an [N, OH, OW] output over an [N, H, W] input whose first
 * pixel has index `start` (level-concatenated inputs: one call per level with the running pixel offset); replaces a host-side build + copy
 * per new canvas (Detectron2 ImageList.from_tensors pads every batch to its own canvas: reference data/dataset_mapper.py, INPUT.MIN_SIZE_TRAIN) */
int utv2_rowinfo_nhwc(int* out, int N, int H, int W, int OH, int OW, int stride, int pad, int KH, int KW, int64_t start,
                      utv2_stream_t stream);
int utv2_f32_to_bf16(const float* src, void* dst16, int64_t n, utv2_stream_t stream);
int utv2_weight_flip_transpose_bf16(const float* w, void* wt16, const float* scale, int K, int KH, int KW, int C,
                                    utv2_stream_t stream);
/* dst16 bf16 [rows][cpad] = src [rows][c] (UTV2_F32 / UTV2_BF16) rounded to nearest even, columns [c, cpad) zero; c, cpad % 8 == 0.
 * The output gradient of a layer whose channel count is no multiple of 32 (the 80-channel FCOS prediction convs, fcos.py:283-307),
 * padded for the LDS-DMA dgrad kernel. */
int utv2_pad_cols_bf16(const void* src, int src_dtype, void* dst16, int64_t rows, int c, int cpad, utv2_stream_t stream);
/* every dgrad weight image of a model in one launch; table = device array of nlayers 48-byte records
 * {int64 w_off (elements into arena), int64 dst_off (into bank), int64 scale_off (into scales, -1 = none), int32 K, KH, KW, C,
 *  int32 Kpad (>= K: pitch of the image's output-channel axis, channels [K, Kpad) zero), int32 0} */
int utv2_weight_flip_transpose_bf16_batched(const float* arena, const float* scales, void* bank, const void* table, int nlayers,
                                            utv2_stream_t stream);

/* ---- teacher EMA: engine/trainer.py:468-486 (FCOS), :950-968 (RCNN) --------------------------
 * teacher = student*(1-keep) + teacher*keep, evaluated with the reference's three roundings.
 * mirror16 (optional; here 8-byte aligned, and in the two SGD updates below): the 16-bit mirror of the arena range that is updated -
 * mirror16[i] = the library's 16-bit rounding of the new value, the copy the mixed-precision convs read: the weights are not re-read by a
 * conversion pass before the next forward */
int utv2_ema_axpby(float* teacher, const float* student, void* mirror16, int64_t n, double keep_rate, utv2_stream_t stream);
/* ---- SGD+momentum+weight-decay on a flat arena: torch.optim.SGD via D2 build_optimizer
 * (engine/trainer.py:50,625; optimizer.step at :425-429,:912). */
int utv2_sgd_momentum(float* param, float* grad, float* mom_buf, void* mirror16, int64_t n, float lr, float momentum, float weight_decay,
                      float grad_scale, int zero_grad, utv2_stream_t stream);
/* Dynamic loss scaling of the fp16 AMP mode with torch.cuda.amp.GradScaler's semantics (reference engine/trainer.py:207,424-426),
 * on the device: state = fp32 {loss scale, found_inf flag, growth tracker}.  utv2_amp_found_inf sets the flag when the (scaled)
 * gradient arena holds a non-finite value; utv2_sgd_momentum_amp applies the SGD step to grad / scale (* grad_scale), or nothing at
 * all when the flag is set; utv2_amp_update_scale: flag ? scale *= backoff : (every growth_interval clean steps scale *= growth),
 * then clears the flag. */
int utv2_amp_found_inf(const float* grad, int64_t n, float* state, utv2_stream_t stream);
int utv2_sgd_momentum_amp(float* param, const float* grad, float* mom_buf, void* mirror16, int64_t n, float lr, float momentum,
                          float weight_decay, float grad_scale, const float* state, utv2_stream_t stream);
int utv2_amp_update_scale(float* state, float growth_factor, float backoff_factor, int growth_interval, utv2_stream_t stream);
/* Per-tensor gradient clipping and Nesterov momentum inside the SGD update (SOLVER.CLIP_GRADIENTS.*, SOLVER.NESTEROV; Detectron2's
 * maybe_add_gradient_clipping: clip_grad_value_ / clip_grad_norm_ on every parameter tensor inside optimizer.step(), then
 * torch.optim.SGD [D2-recall]).  The updated arena range [0, chunk_start[nchunks]) is described by a device work list the caller builds
 * once: chunk c = elements [chunk_start[c], chunk_start[c+1]) (int64, increasing, chunk_start[0] = 0), chunk_seg[c] = the reference
 * tensor ("segment", 0 <= s < nseg) it lies in or -1 for elements of no tensor (padding), chunk_wd[c] its weight decay; seg_chunks =
 * nseg pairs {first chunk, chunk count}: the chunks of a segment are consecutive.  The entry points cannot read the list; the caller
 * vouches for it.  grad / param / mom_buf are 16-byte aligned, mirror16 8-byte.
 * utv2_grad_clip_coef: coef[s] = min(1, clip_value / (mult * ||grad[segment s]||_p + 1e-6)), p = 2 / 1 / inf for norm_kind 0 / 1 / 2,
 *   mult = grad_scale (/ amp_state[0], the loss scale, when amp_state is given).  Sums in fp64, two stages, no atomics: the result is
 *   bit-reproducible.  partial: nchunks doubles of scratch.
 * utv2_sgd_segmented: g = grad * mult; clip_mode 1: g = clamp(g, -clip_value, clip_value), 2: g *= coef[segment] (1 outside every
 *   segment), 0: nothing; g += wd*p; buf = momentum*buf + g; p -= lr * (nesterov ? g + momentum*buf : buf); mirror16 as above.  With
 *   amp_state the step is skipped when its found_inf flag is set.  The clipped gradient is not written back. */
int utv2_grad_clip_coef(const float* grad, const int64_t* chunk_start, const int32_t* chunk_seg, int nchunks, const int32_t* seg_chunks,
                        int nseg, int norm_kind, double clip_value, float grad_scale, const float* amp_state, double* partial, float* coef,
                        utv2_stream_t stream);
int utv2_sgd_segmented(float* param, const float* grad, float* mom_buf, void* mirror16, const int64_t* chunk_start,
                       const int32_t* chunk_seg, const float* chunk_wd, int nchunks, const float* coef, int clip_mode, float clip_value,
                       float lr, float momentum, float grad_scale, int nesterov, const float* amp_state, utv2_stream_t stream);

/* ---- elementwise pieces of ResNet / FPN ([D2-recall]) ------------------ */
int utv2_relu_bwd_scale(const void* dy, const void* y, const float* scale, void* out, int64_t M, int C, int dtype,
                        utv2_stream_t stream);
int utv2_add(const float* a, const float* b, float* out, int64_t n, utv2_stream_t stream);
int utv2_maxpool3x3s2_nhwc(const void* x, int x_dtype, void* y, int y_dtype, int N, int H, int W, int C, int OH, int OW,
                           utv2_stream_t stream);
/* its backward (a trainable stem, MODEL.BACKBONE.FREEZE_AT < 1; ATen max_pool2d_with_indices_backward): dx = the sum of dpool over the
 * windows whose FIRST maximum (kh, kw scan order) the pixel is; relu != 0: times (x > 0), the ReLU in front of the pool.  x = the
 * pool's input (x_dtype); dpool, dx: g_dtype (f32 / f32, 16-bit / 16-bit, 16-bit x with f32 gradients) */
int utv2_maxpool3x3s2_bwd_nhwc(const void* x, int x_dtype, const void* dpool, void* dx, int g_dtype, int N, int H, int W, int C, int OH,
                               int OW, int relu, utv2_stream_t stream);
int utv2_upsample2x_add_nhwc(const void* lateral, const void* top, void* out, int N, int H, int W, int C, int dtype,
                             utv2_stream_t stream);
int utv2_downsample2x_sum_nhwc(const void* g, void* dtop, int N, int TH, int TW, int C, int accumulate, int dtype,
                               utv2_stream_t stream);
/* dgrad of a stride-2 1x1 conv (D2 STRIDE_IN_1X1 bottlenecks): dst[n,2i,2j,:] = src[n,i,j,:], zeros elsewhere;
 * src is [N][(H+1)/2][(W+1)/2][C] - the compact gradient comes from a plain GEMM instead of a 4x larger masked one */
int utv2_zero_interleave2x_nhwc(const void* src, const void* mask, void* dst, int N, int H, int W, int C, int dtype, utv2_stream_t stream);
/* the same on 16-bit tensors (C % 8 == 0) with the fusions of the stride-2 bottlenecks' backward: dst = add + (even pixel ? masked src : 0);
 * the mask as a 16-bit tensor or as a bit plane (utv2_conv2d_nhwc_fwd_bf16_bits); `add` = the gradient another consumer of the same
 * activation produced (already masked by its producer) - no elementwise add pass.  mask, mask_bits, add optional. */
int utv2_zero_interleave2x_add_nhwc(const void* src, const void* mask, const void* mask_bits, const void* add, void* dst, int N, int H, int W,
                                    int C, utv2_stream_t stream);
/* modeling/one_stage_detector.py:88-90 / meta_arch/rcnn.py:18 (preprocess_image + ImageList pad) */
int utv2_preprocess_image(const void* src, int is_u8, float* dst, int H, int W, int Hp, int Wp,
                          const float* mean3_host, const float* std3_host, utv2_stream_t stream);
/* same, as bf16 at pixel offset (3,3) of one [Hp+6][Wp+8][4] slot of the zero-bordered bf16 stem input */
int utv2_preprocess_image_bf16pad(const void* src, int is_u8, void* dst16, int H, int W, int Hp, int Wp,
                                  const float* mean3_host, const float* std3_host, utv2_stream_t stream);
/* the whole batch in one launch: src_host = host array of N <= 32 device pointers ([3][H_i][W_i] images, all uint8 or all fp32),
 * dst16 = the N slots bf16 [N][Hp+6][Wp+8][4] */
int utv2_preprocess_images_bf16pad(const void* const* src_host, int is_u8, void* dst16, const int* H_host, const int* W_host, int N,
                                   int Hp, int Wp, const float* mean3_host, const float* std3_host, utv2_stream_t stream);
/* D2 FrozenBatchNorm2d.forward: scale = w*rsqrt(var+eps), shift = b - mean*scale, all layers at once */
int utv2_frozenbn_fold(const float* w, const float* b, const float* mean, const float* var, float* scale, float* shift,
                       int n, float eps, utv2_stream_t stream);
/* GroupNorm(32)+ReLU of the FCOS towers: fcos/fcos.py:263-264,283.  Every entry normalises all the (image, FPN level) segments of a
 * level-first [rows][C] buffer in one launch chain (seg_rows_host: host int[nseg], 1 <= nseg <= 160, rows of each segment >= 0; a dense
 * [N][HW][C] tensor is N segments of HW rows).  ws: utv2_groupnorm_seg_workspace_floats() floats, for the forward and both backwards. */
int64_t utv2_groupnorm_seg_workspace_floats(int nseg, const int* seg_rows_host, int C);
int utv2_groupnorm_relu_seg_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                float* ws, int nseg, const int* seg_rows_host, int C, int G, float eps, int relu, int dtype,
                                utv2_stream_t stream);
/* the same for bf16 x with 8 channels per group when the conv that produced x left the statistics partials in part32
 * (utv2_conv2d_ml_fwd_bf16_g gn_part: fp32 [ceil(rows / 32)][G][2]): one tensor pass less.
 * relu_bits (optional; C % 32 == 0): also writes the ReLU mask as a bit plane, [rows * C / 8] bytes, bit (row * C + c) = y > 0 in fp32,
 * before the 16-bit rounding (the reference's ReLU follows an fp32 GroupNorm under autocast): the mask ..._seg_bwd recomputes from x */
int utv2_groupnorm_relu_seg_fwd_p32(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                                    const float* part32, int nseg, const int* seg_rows_host, int C, int G, float eps, int relu,
                                    void* relu_bits, utv2_stream_t stream);
/* beta (optional): the ReLU mask is recomputed from x with the forward expression instead of read from y (y may be null).
 * colsum_part (optional, fp32 [utv2_groupnorm_seg_chunks(...)][C]) = per-chunk column sums of dx as stored: summed over the chunks
 * (utv2_colsum_partials) they are the bias gradient of the convolution in front of the GroupNorm (fcos.py:263: conv -> GN -> ReLU), whose
 * dY is this dx - no separate pass over dY */
int64_t utv2_groupnorm_seg_chunks(int nseg, const int* seg_rows_host);
int utv2_groupnorm_relu_seg_bwd(const void* dy, const void* y, const void* x, const float* mean, const float* rstd,
                                const float* gamma, const float* beta, void* dx, float* dgamma, float* dbeta, float* ws,
                                int nseg, const int* seg_rows_host, int C, int G, int relu, int dtype, float* colsum_part,
                                utv2_stream_t stream);
/* GroupNorm (+ ReLU) backward from the partial sums of utv2_conv2d_ml_fwd_bf16_gnb: g = the incoming gradient with the ReLU mask already
 * applied (16-bit [rows][C]), part64 = that conv's gnb_part.  dx / dgamma / dbeta / colsum_part / ws as utv2_groupnorm_relu_seg_bwd. */
int utv2_groupnorm_seg_bwd_p64(const void* g, const void* x, const float* mean, const float* rstd, const float* gamma, void* dx,
                               float* dgamma, float* dbeta, float* ws, int nseg, const int* seg_rows_host, int C, int G,
                               const float* part64, float* colsum_part, utv2_stream_t stream);
/* GroupNorm (+ ReLU) over ROIS (csrc/groupnorm_roi.hip; the conv box head, Detectron2 FastRCNNConvFCHead with NORM "GN"): x, y dense
 * [R][HW][C] of `dtype`, statistics per (ROI, group) into mean, rstd fp32 [R][G]; one workgroup per ROI, one pass over the tensor.
 * 1 <= HW <= 196, C % 4 == 0, C <= 1024, C % G == 0, (C / G) % 4 == 0, every pointer 16-byte aligned; R == 0: nothing is launched.
 * The mean, then the sum of squares of x - mean (centred; biased variance, eps inside the square root), all fp32; the ReLU acts on the
 * fp32 value before the rounding to `dtype`. */
int utv2_groupnorm_roi_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, int R, int HW, int C,
                           int G, float eps, int relu, int dtype, utv2_stream_t stream);
/* dx written; dgamma / dbeta (fp32 [C]) accumulated (+=) from per-workgroup column sums by a second launch in a fixed order (no
 * atomics: bit-identical from run to run).  The ReLU mask is recomputed from x with the forward's expression.
 * ws: utv2_groupnorm_roi_workspace_floats(R, C) floats. */
int64_t utv2_groupnorm_roi_workspace_floats(int R, int C);
int utv2_groupnorm_roi_bwd(const void* dy, const void* x, const float* mean, const float* rstd, const float* gamma, const float* beta,
                           void* dx, float* dgamma, float* dbeta, float* ws, int R, int HW, int C, int G, int relu, int dtype,
                           utv2_stream_t stream);
/* db[c] (+)= sum_b partial[b][c], partial fp32 [nb][K] (the colsum_part above; fixed summation order) */
int utv2_colsum_partials(const float* partial, float* db, int nb, int K, int accumulate, utv2_stream_t stream);

/* ---- FCOS targets / losses / decode: modeling/fcos/fcos_outputs.py --------------------------- */
/* :649-698,:772-906; center_radius > 0 = CENTER_SAMPLE with POS_RADIUS (get_sample_region :700-770), 0 = plain in-box test.
 * drop_empty: bit 0 = images without gt drop all their locations (label -1; keep_locations of :804-815,310-311), bit 1 = ignore_near
 * (:841-848): a location inside some box but inside no box's centre-sampling region is dropped.
 * H,W,strides,soi are HOST arrays.  img_active (optional, device uint8[N]):
 * images flagged 0 get label -1 everywhere (ignored by the loss kernels) - the two student passes of one iteration
 * (trainer.py:396-411) run as one batch and each loss branch sees only its own images. */
int utv2_fcos_targets(int num_levels, const int* H_host, const int* W_host, const int* strides_host,
                      const float* soi_host, int N, int MAXG, const float* gt_boxes, const int* gt_classes,
                      const unsigned char* gt_valid, const float* gt_std, int num_classes, int drop_empty,
                      float center_radius, const unsigned char* img_active, int* labels, float* reg_targets, float* bvars,
                      int* gt_inds, utv2_stream_t stream);
/* the same for a batch of N images of which only [gt_img0, gt_img0 + gt_imgs) carry this loss branch's ground truth (the gt arrays
 * hold gt_imgs images); every other image gets label -1 - no padded copies of the gt arrays, no activity mask */
int utv2_fcos_targets_range(int num_levels, const int* H_host, const int* W_host, const int* strides_host, const float* soi_host, int N,
                            int MAXG, const float* gt_boxes, const int* gt_classes, const unsigned char* gt_valid, const float* gt_std,
                            int gt_img0, int gt_imgs, int num_classes, int drop_empty, float center_radius,
                            const unsigned char* img_active, int* labels, float* reg_targets, float* bvars, int* gt_inds,
                            utv2_stream_t stream);
/* fvcore sigmoid_focal_loss_jit at :329-338,:619-628 with on-the-fly one-hot.  ws >= 1024 floats.
 * Checked (UTV2_EARG otherwise): non-null pointers, P >= 0, C >= 1 (any C; C % 4 == 0 with P * C < 2^32 takes the vector path).
 * The caller's contract, NOT checked (device data / no defined error): labels in [-1, C] (-1 = row skipped, C = background; any other
 * value is a row without a positive), gamma >= 0 (2 is a fast path); alpha < 0 = no class weighting (fvcore's rule). */
int utv2_sigmoid_focal_fwd(const float* logits, const int* labels, int64_t P, int C, float alpha, float gamma,
                           float* loss_sum, float* ws, utv2_stream_t stream);
int utv2_sigmoid_focal_bwd(const float* logits, const int* labels, int64_t P, int C, float alpha, float gamma,
                           const float* coef, float* dlogits, utv2_stream_t stream);
/* :340-416 / :514-590 fused over positive locations: Integral(:44-77), centerness target + BCE,
 * GIoU (layers/iou_loss.py:26-76), NLL (layers/kl_loss.py:69-105), TS-better L1 (:552-569).
 * sums[8] = {n_pos, sum ctr_t, sum bce, sum giou*ctr_t, sum nll*iou, n_sel, sum_sel|d-t|, 0}
 * ws >= 4096 floats.
 * Accepted: reg_max == 16, box_stride >= 73 and % 4 == 0, P >= 0, flags = quality-iou (1) | klloss (2) | loc type 0..2 << 2 | kl-weight-ctr (16),
 * bvars NULL = no teacher-better term; all of these are checked, anything else: UTV2_EARG.  P == 0: the forward writes sums = 0, the
 * backward entries write nothing.  Not checked (device data): labels (< 0 or == num_classes: no gradient), targets > 0. */
int utv2_fcos_loc_terms_fwd(const int* labels, const float* box, int box_stride, const float* reg_targets,
                            const float* bvars, int64_t P, int num_classes, int reg_max, float ts_better, float ts_cert,
                            int flags, float* sums, float* ws, utv2_stream_t stream);
int utv2_fcos_loc_terms_bwd(const int* labels, const float* box, int box_stride, const float* reg_targets,
                            const float* bvars, int64_t P, int num_classes, int reg_max, float ts_better, float ts_cert,
                            int flags, const float* coef, float* dbox, utv2_stream_t stream);
/* The backward launches of SEVERAL loss branches of one fused student pass into ONE gradient tensor per head output (the supervised,
 * pseudo-classification and pseudo-regression target sets of engine/trainer.py:396-411 all differentiate the same logits / box
 * buffers): coef = the d total / d sum vector of utv2_fcos_loss_combine for this branch (focal: 1 float; loc terms: the 8 floats of
 * d total / d sums[8], read at [2], [3], [4], [6]), gscale = optional device scalar multiplied in (the node's upstream gradient).
 * accumulate 0: writes every row (zeros where the branch has no gradient); 1: rows without a gradient (label < 0; for the location
 * terms also background) are left untouched, the others ADDED - no per-branch gradient tensors, no elementwise add passes. */
int utv2_sigmoid_focal_bwd_acc(const float* logits, const int* labels, int64_t P, int C, float alpha, float gamma, const float* coef,
                               const float* gscale, float* dlogits, int accumulate, utv2_stream_t stream);
int utv2_fcos_loc_terms_bwd_acc(const int* labels, const float* box, int box_stride, const float* reg_targets, const float* bvars,
                                int64_t P, int num_classes, int reg_max, float ts_better, float ts_cert, int flags, const float* coef8,
                                const float* gscale, float* dbox, int accumulate, utv2_stream_t stream);
/* scalar tail of the FCOS losses of a fused student pass (normalisation fcos_outputs.py:317-321,361-362,381-416; pseudo branch
 * :504-585; loss weighting engine/trainer.py:396-417): the raw sums of utv2_sigmoid_focal_fwd / utv2_fcos_loc_terms_fwd of the
 * supervised, pseudo-cls and pseudo-reg target sets -> rec[8] = {cls, loc, ctr, cls_pseudo, ctr_pseudo, loc_pseudo,
 * teacher_better_student, weighted total} and coef[26] = d total / d {focal_sup[1], sums_sup[8], focal_cls[1], sums_cls[8], sums_reg[8]}.
 * norm: optional [6] all-reduced (n_pos, sum ctrness) per branch (NULL: the local sums); world = data-parallel world size;
 * flags 1 KL_LOSS, 2 KL type "klloss", 4 UNIFY_CTRCLS, 8 tsbetter; loss k (order cls, loc, ctr, cls_p, ctr_p, loc_p) enters the total
 * as value * wmul_host[k] / wdiv_host[k]. */
int utv2_fcos_loss_combine(const float* focal_sup, const float* sums_sup, const float* focal_cls, const float* sums_cls,
                           const float* sums_reg, const float* norm, float world, int flags, float kl_weight, const float* wmul_host,
                           const float* wdiv_host, float* rec, float* coef, utv2_stream_t stream);
/* :1146-1195 ranking score -> sortable int64 key (method 0 cls, 1 cls_n_ctr, 2 ctr, 3 cls_n_loc); image n's HW*C keys
 * start at keys + n*key_row_stride (>= HW*C: rows of a wider matrix shared by all FPN levels).  = utv2_fcos_rank_keys_f with flags 0. */
int utv2_fcos_rank_keys(const float* logits, const float* box, int box_stride, int reg_max, int N, int HW, int C,
                        float thr, int method, long long* keys, int64_t key_row_stride, utv2_stream_t stream);
/* MODEL.FCOS.THRESH_WITH_CTR (fcos_outputs.py:148,1172-1195,1270-1275): the ranking / decode entry points with a further `flags`
 * argument, 0 or UTV2_FCOS_THRESH_WITH_CTR; utv2_fcos_rank_keys, utv2_fcos_decode and utv2_fcos_decode_cont forward to them with
 * flags 0 (one kernel per op, the flag is a uniform branch in it), every other argument and check as there.  With the flag,
 * s = sigmoid(logit) * sigmoid(ctrness) (both sigmoids first, one fp32 product) is what the threshold tests, s is the ranking score
 * the key carries for EVERY criterion (the cls / cls_n_ctr / ctr / cls_n_loc switch is skipped; ctrness is read at column
 * 4 * (reg_max + 1) + 4: the discrete rows and, with reg_max = 0, the continuous ones) and the decode writes oconf = s; oscores
 * still follows the criterion's name: sqrt(s) for cls_n_ctr / cls_n_loc, s for cls / ctr; octr (the plain sigmoid), ostd, boxes and
 * locations do not depend on the flag.  The keys a decode is given must come from utv2_fcos_rank_keys_f with the same flags.
 * UTV2_EARG, nothing launched: method outside 0..3, any flag bit other than UTV2_FCOS_THRESH_WITH_CTR. */
#define UTV2_FCOS_THRESH_WITH_CTR 1
int utv2_fcos_rank_keys_f(const float* logits, const float* box, int box_stride, int reg_max, int N, int HW, int C,
                          float thr, int method, int flags, long long* keys, int64_t key_row_stride, utv2_stream_t stream);
int utv2_fcos_decode_f(const long long* topkeys, int K, const float* logits, const float* box, int box_stride, int reg_max,
                       int N, int HW, int Wl, int C, int stride, int level, int method, int flags, int MAXC, int slot0, float* oboxes,
                       float* oscores, int* ocls, float* oloc, float* octr, float* oconf, float* ostd, int* olevel,
                       unsigned char* ovalid, utv2_stream_t stream);
int utv2_fcos_decode_cont_f(const long long* topkeys, int K, const float* logits, const float* box, int box_stride, int N, int HW, int Wl,
                            int C, int stride, int level, int method, int flags, int MAXC, int slot0, float* oboxes, float* oscores,
                            int* ocls, float* oloc, float* octr, float* oconf, float* ostd, int* olevel, unsigned char* ovalid,
                            utv2_stream_t stream);
/* :1238-1241 `topk(pre_nms_top_n)` for every (image, level) row at once: exact MSD radix select over ragged rows
 * (row r = keys[row_off[r] .. row_off[r+1]), row_off device int64[rows+1]); out[rows][k] descending, -1 padded; k <= 8192 */
int64_t utv2_topk_rows_workspace_bytes(int rows, int k);
int utv2_topk_rows_i64(const long long* keys, const long long* row_off, int rows, int64_t max_width, int k, long long* out,
                       void* ws, utv2_stream_t stream);
/* :1093-1104,:1258-1296 decode of the selected candidates of one level into padded slots (method 0..3, as utv2_fcos_rank_keys; this
 * entry point does not check it: any other value writes what 0 writes, as it always did).  = utv2_fcos_decode_f with flags 0. */
int utv2_fcos_decode(const long long* topkeys, int K, const float* logits, const float* box, int box_stride, int reg_max,
                     int N, int HW, int Wl, int C, int stride, int level, int method, int MAXC, int slot0, float* oboxes,
                     float* oscores, int* ocls, float* oloc, float* octr, float* oconf, float* ostd, int* olevel,
                     unsigned char* ovalid, utv2_stream_t stream);
/* ---- the same for the CONTINUOUS regression head (MODEL.FCOS.REG_DISCRETE False: plain FCOS, fcos/fcos.py:294-297,363-364) ----
 * box rows: [ltrb 4 | std 4 | ctr 1 | pad], the ltrb columns hold the Scale layer's output BEFORE the ReLU: every kernel here uses
 * d = max(box[0:4], 0) (fcos_outputs.py:349-350,545-546,1107-1108) and the backward writes 0 where the stored value is <= 0 (torch's
 * ReLU gradient at exactly 0 and at -0.0).  sums[8], flags, bvars / ts_better / ts_cert, coef / coef8 / gscale / accumulate and the row
 * rules are those of utv2_fcos_loc_terms_fwd / _bwd / _bwd_acc above; the reduction is per-block partials summed in a fixed order.
 * ws >= 4096 floats.
 * Checked (UTV2_EARG otherwise, nothing is launched): non-null labels / box / reg_targets / sums / ws / coef / dbox, P >= 0,
 * box_stride >= 9 and % 4 == 0, 0 <= flags < 32 with loc type 0..2.  P == 0: the forward writes sums = 0, the backward entries write
 * nothing.  Rows are indexed in 64 bits.  Not checked (device data): labels (< 0 or == num_classes: no gradient), targets > 0. */
int utv2_fcos_loc_terms_cont_fwd(const int* labels, const float* box, int box_stride, const float* reg_targets, const float* bvars,
                                 int64_t P, int num_classes, float ts_better, float ts_cert, int flags, float* sums, float* ws,
                                 utv2_stream_t stream);
int utv2_fcos_loc_terms_cont_bwd(const int* labels, const float* box, int box_stride, const float* reg_targets, const float* bvars,
                                 int64_t P, int num_classes, float ts_better, float ts_cert, int flags, const float* coef, float* dbox,
                                 utv2_stream_t stream);
int utv2_fcos_loc_terms_cont_bwd_acc(const int* labels, const float* box, int box_stride, const float* reg_targets, const float* bvars,
                                     int64_t P, int num_classes, float ts_better, float ts_cert, int flags, const float* coef8,
                                     const float* gscale, float* dbox, int accumulate, utv2_stream_t stream);
/* utv2_fcos_decode for those rows: ltrb = max(r, 0) * stride, every other output as there.  The ranking keys come from
 * utv2_fcos_rank_keys with reg_max = 0 (it finds std / ctr at 4 * (reg_max + 1) = 4: this layout).
 * Checked: non-null pointers (outputs included), box_stride >= 9 and % 4 == 0, K >= 0, 1 <= N <= 65535, HW, Wl, C, stride >= 1,
 * Wl <= HW, HW * C < 2^32, method 0..3, slot0 >= 0, slot0 + K <= MAXC.  K == 0 writes nothing.  A key >= 0 whose index lies outside
 * HW * C (no utv2_fcos_rank_keys output) becomes an empty slot.  = utv2_fcos_decode_cont_f with flags 0. */
int utv2_fcos_decode_cont(const long long* topkeys, int K, const float* logits, const float* box, int box_stride, int N, int HW, int Wl,
                          int C, int stride, int level, int method, int MAXC, int slot0, float* oboxes, float* oscores, int* ocls,
                          float* oloc, float* octr, float* oconf, float* ostd, int* olevel, unsigned char* ovalid,
                          utv2_stream_t stream);
/* Scale layers fcos/fcos.py:22-28,356-357 (one learnable scalar per level on the first ncols columns of strided rows) of ALL levels of a
 * level-first matrix at once (one launch forward, two backward): row0_host = host int64[nlev + 1] (first row of each level, then the end), s_host / sgrad_host = host arrays of nlev DEVICE pointers
 * (the per-level scalar and its gradient, accumulated: sgrad_l += sum(g_in * ypost) / s_l).  nlev <= 8; ws >= nlev * 1024 floats */
int utv2_scale_cols_ml(float* y, int nlev, const int64_t* row0_host, int row_stride, int ncols, const float* const* s_host,
                       utv2_stream_t stream);
int utv2_scale_cols_bwd_ml(float* g, const float* ypost, int nlev, const int64_t* row0_host, int row_stride, int ncols,
                           const float* const* s_host, float* const* sgrad_host, float* ws, utv2_stream_t stream);
/* the same backward, out of place, straight into the zero-padded 16-bit matrix the prediction conv's dgrad / weight gradient read:
 * out16 = 16-bit [rows][cpad] (cpad >= row_stride, % 4 == 0): [:, :ncols] = g * s_l, [:, ncols:row_stride] = g, [:, row_stride:] = 0; g is
 * not modified (no clone of the incoming gradient, no separate utv2_pad_cols_bf16 pass).  ws >= nlev * 1024 floats */
int utv2_scale_cols_bwd_ml_pad16(const float* g, const float* ypost, int nlev, const int64_t* row0_host, int row_stride, int ncols,
                                 const float* const* s_host, float* const* sgrad_host, float* ws, void* out16, int cpad, utv2_stream_t stream);

/* ---- NMS / IoU: layers/ml_nms.py:27, D2 batched_nms / pairwise_iou ---------------------------- */
int utv2_nms_mpad(int M);
int64_t utv2_nms_workspace_bytes(int N, int M);
int utv2_nms_batched(const float* boxes, const float* scores, const int* cls, const unsigned char* valid, int N, int M,
                     float iou_thr, int class_aware, int post_topk, int max_out, int* keep, int* keep_count, void* ws,
                     utv2_stream_t stream);
int utv2_box_iou(const float* a, const float* b, int A, int B, float* out, utv2_stream_t stream);

/* ---- Faster-RCNN path ----------------------------------------------------------------------- */
/* D2 pairwise_iou + Matcher (proposal_generator/rpn.py:112-148, roi_heads/roi_heads.py:213-231):
 * per candidate box the max IoU over the image's valid gts and its (first) argmax; optionally the
 * per-gt max over boxes (uint32 float bits, caller zero-fills) for the low-quality pass. */
int utv2_match_boxes(const float* boxes, int64_t box_img_stride, int N, int P, const float* gt_boxes,
                     const unsigned char* gt_valid, int G, float* max_iou, int* arg, unsigned* gt_max_bits,
                     utv2_stream_t stream);
int utv2_match_lowq(const float* boxes, int64_t box_img_stride, int N, int P, const float* gt_boxes,
                    const unsigned char* gt_valid, int G, const unsigned* gt_max_bits, unsigned char* lowq,
                    utv2_stream_t stream);
/* The ROI pooler (D2 ROIPooler, roi_heads/roi_heads.py:28-45,118: level assignment with canonical size 224 at level 4) in the three
 * forms of MODEL.ROI_BOX_HEAD.POOLER_TYPE.  feats_host / dfeats_host: HOST arrays of device pointers.
 *   UTV2_POOLER_ALIGN_V2  "ROIAlignV2": torchvision roi_align, aligned=True (half-pixel shift, empty boxes pool nothing)
 *   UTV2_POOLER_ALIGN     "ROIAlign":   torchvision roi_align, aligned=False (no shift, sides floored at one pixel)
 *   UTV2_POOLER_MAX       "ROIPool":    torchvision roi_pool (rounded corners, maximum per bin)
 * sampling_ratio (RoIAlign only; ignored by UTV2_POOLER_MAX): samples per bin and axis, 0 = ceil(bin size in pixels).
 * argmax (UTV2_POOLER_MAX only, otherwise NULL) [R][PH][PW][C] int32: written by fwd, read by bwd - per output element the index
 * y * W + x of its maximum inside the ROI's (level, image) map, -1 where the bin's window is empty or the slot invalid.
 * fwd: features / out are `dtype`.  bwd: fp32 atomic scatter into zero-filled dfeats, any ROI order.  bwd_tiled: deterministic gather
 * over 8 x 8 pixel tiles, the ROIs of image n are rois[n*rois_per_image .. (n+1)*rois_per_image), C <= 256, PH, PW <= 7; every element
 * of every dfeats[l] ([N][H_l][W_l][C], element type out_dtype) is written - no zero-fill, no atomics. */
#define UTV2_POOLER_ALIGN_V2 0
#define UTV2_POOLER_ALIGN 1
#define UTV2_POOLER_MAX 2
int utv2_roi_pooler_fwd(int pooler, int sampling_ratio, int num_levels, int min_level, const void* const* feats_host,
                        const int* H_host, const int* W_host, const float* scales_host, const float* rois, const int* roi_batch,
                        const unsigned char* roi_valid, int R, int C, int PH, int PW, void* out, int* argmax, int dtype,
                        utv2_stream_t stream);
int utv2_roi_pooler_bwd(int pooler, int sampling_ratio, int num_levels, int min_level, float* const* dfeats_host, const int* H_host,
                        const int* W_host, const float* scales_host, const float* rois, const int* roi_batch,
                        const unsigned char* roi_valid, int R, int C, int PH, int PW, const void* dy, const int* argmax, int dtype,
                        utv2_stream_t stream);
int utv2_roi_pooler_bwd_tiled(int pooler, int sampling_ratio, int num_levels, int min_level, void* const* dfeats_host,
                              const int* H_host, const int* W_host, const float* scales_host, const float* rois,
                              const unsigned char* roi_valid, int N, int rois_per_image, int C, int PH, int PW, const void* dy,
                              const int* argmax, int dy_dtype, int out_dtype, utv2_stream_t stream);
/* RPN proposal decoding, the part of detectron2's RPN.predict_proposals / find_top_rpn_proposals in front of the NMS that
 * proposal_generator/rpn.py:60-76 inherits.  head: level-first RPN head output, rows (level, image, pixel) x ch floats = A objectness
 * logits then 4A anchor-major deltas; hw_host[l] = pixels of level l.
 * rank_keys: keys[t] for every logit in memory order (rows x A), 63-bit, descending key order == (logit desc, anchor index asc) within
 * the logit's (level, image) row - the input of utv2_topk_rows_i64.
 * decode: top = [num_levels * N][maxk] selected keys (-1 = empty), k_host[l] candidates kept per image on level l; writes, per image,
 * the K = sum k_l candidates in level order: boxes [N][K][4] (apply_deltas with weights_host[4], clipped to image_hw[n] = (h, w)),
 * scores (0 where non-finite), lvls, keep (finite and both sides > min_size). */
int utv2_rpn_rank_keys(const float* head, int num_levels, const int* hw_host, int N, int A, int ch, int64_t* keys, utv2_stream_t stream);
int utv2_rpn_decode(const int64_t* top, int maxk, const float* head, const float* anchors, const float* image_hw, int num_levels,
                    const int* hw_host, const int* k_host, int N, int A, int ch, const float* weights_host, float scale_clamp,
                    float min_size, float* boxes, float* scores, int* lvls, unsigned char* keep, utv2_stream_t stream);
/* the survivors of utv2_nms_batched (kidx [N][D], -1 padded; cnt [N]) gathered into padded outputs: oboxes [N][D][4], oscores [N][D],
 * ovalid [N][D] = slot < cnt (slots beyond the count repeat candidate 0) - the tail of D2 find_top_rpn_proposals in one launch */
int utv2_nms_pack(const int* kidx, const int* cnt, const float* boxes, const float* scores, int N, int M, int D, float* oboxes, float* oscores,
                  unsigned char* ovalid, utv2_stream_t stream);
/* The predictor's inference (roi_heads/fast_rcnn.py:1094-1125,1162-1225; D2 fast_rcnn_inference) around the top-k and the NMS.
 * nbox = 1 (class-agnostic regression: one box per proposal) or K (MODEL.ROI_BOX_HEAD.CLS_AGNOSTIC_BBOX_REG False, fast_rcnn.py:1162-1185:
 * one box per (proposal, class)).
 * keys:   probs [N*P][K+1] (softmax), deltas [N*P][4*nbox], prop [N][P][4], valid [N][P], whwh [N][4] = (w, h, w, h) of the image ->
 *         boxes [N][P][nbox][4] = Box2BoxXYXYTransform.apply_deltas (weights wx, wy; clamp +-scale_clamp) clipped to the image, and
 *         keys [N][P*K]: per foreground class (order-preserving bits of its probability) << 32 | (2^32 - 1 - (p*K + c)), the key of
 *         -1 when prob <= thr / the slot is invalid / ANY decoded box or foreground probability of the proposal is not finite (D2
 *         fast_rcnn_inference_single_image filters rows).  Descending key order = (prob desc, index asc).
 * gather: top [N][k] (the k largest keys of each image, descending; keys that `keys` wrote: flat index < P*K) -> sc, rows (proposal
 *         index, int64), cls, cb [N][k][4] = boxes[n][row][nbox == 1 ? 0 : cls], valid (sc > thr)
 * pack:   kidx [N][D] / cnt [N] of utv2_nms_batched on (cb, sc, cls, valid) -> the padded detections + ostd [N][D][4*nbox], the kept
 *         rows' std logits of stdl [N*P][4*nbox] (fast_rcnn.py:1118-1123); slots beyond the count repeat candidate 0
 * Accepted: N, P, K, k, D >= 1, nbox == K or nbox == 1 (keys, gather), P*K < 2^32 (keys, gather), nbox >= 1 (pack); anything else:
 * UTV2_EARG.  Layout contract, NOT checked: every array is dense (no row pitch) and deltas, prop, whwh, boxes, cb, stdl, oboxes, ostd are
 * 16-byte aligned - the kernels move them as float4. */
int utv2_roi_infer_keys(const float* probs, const float* deltas, const float* prop, const unsigned char* valid, const float* whwh, int N, int P,
                        int K, int nbox, float wx, float wy, float scale_clamp, float thr, float* boxes, int64_t* keys, utv2_stream_t stream);
int utv2_roi_infer_gather(const int64_t* top, const float* boxes, int N, int P, int K, int nbox, int k, float thr, float* sc, int64_t* rows,
                          int* cls, float* cb, unsigned char* valid, utv2_stream_t stream);
int utv2_roi_infer_pack(const int* kidx, const int* cnt, const float* cb, const float* sc, const int* cls, const int64_t* rows, const float* stdl,
                        int N, int P, int k, int D, int nbox, float* oboxes, float* oscores, int* ocls, float* ostd, int64_t* orows,
                        unsigned char* ovalid, utv2_stream_t stream);
/* PseudoLabRPN.losses on the sampled anchors (proposal_generator/rpn.py:153-225): sums[0] = sum of BCE-with-logits over the sampled
 * positives (pos_idx [N][npos], int64 anchor indices, pos_valid) and negatives (neg_idx [N][nneg]) - every term times the score of the
 * anchor's matched pseudo box when gt_scores is given, zero when the image has no gt (has_gt [N]) -, sums[1] = sum over the valid
 * positives of |delta - Box2BoxTransform.get_deltas(anchor, matched gt, weights_host[4])|; gobj [N][npos+nneg] / gdl [N][npos][4] =
 * the derivatives of the two sums.  head = 0: obj [N][R], deltas [N][R][4]; head = 1: obj = deltas = the level-first RPN head output
 * (utv2_rpn_decode's layout).  matched [N][R] int32 (utv2_match_boxes' argmax), gt_boxes [N][G][4], gt_scores [N][G] or NULL.
 * bwd: scatters gout_cls[0] * gobj and gout_loc[0] * gdl (device scalars) to the sampled anchors of zero-filled grad_obj / grad_deltas
 * (same layouts; head = 1: both = the head-output gradient). */
int utv2_rpn_loss_fwd(const float* obj, const float* deltas, int head, int num_levels, const int* hw_host, int N, int A, int ch, int R,
                      const float* anchors, const int64_t* pos_idx, const unsigned char* pos_valid, int npos, const int64_t* neg_idx,
                      const unsigned char* neg_valid, int nneg, const int* matched, const unsigned char* has_gt, const float* gt_boxes,
                      const float* gt_scores, int G, const float* weights_host, float* sums, float* gobj, float* gdl, utv2_stream_t stream);
int utv2_rpn_loss_bwd(const float* gobj, const float* gdl, const float* gout_cls, const float* gout_loc, int head, int num_levels,
                      const int* hw_host, int N, int A, int ch, int R, const int64_t* pos_idx, const unsigned char* pos_valid, int npos,
                      const int64_t* neg_idx, const unsigned char* neg_valid, int nneg, float* grad_obj, float* grad_deltas,
                      utv2_stream_t stream);
/* _range (head = 1 only): the head output holds `batch` images per level and the N images of this call - the sampler arrays, gt and
 * has_gt are theirs alone - are images [img0, img0 + N) of it: one loss branch of a student pass that ran the labeled and the
 * pseudo-labeled images (reference trainer.py:838-866) as one batch.  The plain entries are batch = N, img0 = 0. */
int utv2_rpn_loss_fwd_range(const float* obj, const float* deltas, int head, int num_levels, const int* hw_host, int N, int batch, int img0,
                            int A, int ch, int R, const float* anchors, const int64_t* pos_idx, const unsigned char* pos_valid, int npos,
                            const int64_t* neg_idx, const unsigned char* neg_valid, int nneg, const int* matched,
                            const unsigned char* has_gt, const float* gt_boxes, const float* gt_scores, int G, const float* weights_host,
                            float* sums, float* gobj, float* gdl, utv2_stream_t stream);
int utv2_rpn_loss_bwd_range(const float* gobj, const float* gdl, const float* gout_cls, const float* gout_loc, int head, int num_levels,
                            const int* hw_host, int N, int batch, int img0, int A, int ch, int R, const int64_t* pos_idx,
                            const unsigned char* pos_valid, int npos, const int64_t* neg_idx, const unsigned char* neg_valid, int nneg,
                            float* grad_obj, float* grad_deltas, utv2_stream_t stream);
/* _f: the same with MODEL.RPN.SMOOTH_L1_BETA and BBOX_REG_LOSS_TYPE "giou" (D2 _dense_box_regression_loss [D2-recall], rpn.py:194-202).
 * loc_mode 0, "smooth_l1": sums[1] / gdl are fvcore's smooth_l1_loss of (delta - target) at `beta` - beta < 1e-5: |d| (derivative
 * sign(d)); else 0.5 d^2 / beta where |d| < beta (derivative d / beta) and |d| - 0.5 beta from |d| == beta on (derivative sign(d)).  At
 * beta 0 the arithmetic and the order of the additions are utv2_rpn_loss_fwd's: nothing divides by beta there.  scale_clamp is not read.
 * loc_mode 1, "giou": the positive's deltas decoded on its anchor by Box2BoxTransform.apply_deltas (divide by weights_host, dw / dh
 * clamped from above at scale_clamp, exp - utv2_rpn_decode's arithmetic without the clip to the image), fvcore's giou_loss (eps 1e-7)
 * of that box against the matched gt box, summed; gdl = its derivative through the decode, 0 through a clamped dw / dh.  beta is not
 * read (it must still be valid).  The BCE sum, gobj, the layouts, the one-workgroup fixed summation order and "every element of gobj /
 * gdl is written; a slot without weight contributes nothing" are as above; utv2_rpn_loss_bwd(_range) serves both modes.
 * Accepted: what the plain entries accept, loc_mode 0 or 1, beta >= 0 (+inf included), scale_clamp not NaN; loc_mode outside {0, 1}, a
 * negative or NaN beta, a NaN scale_clamp: UTV2_EARG, nothing is launched.  utv2_rpn_loss_fwd(_range) = _f at (0, 0.f). */
int utv2_rpn_loss_fwd_f(const float* obj, const float* deltas, int head, int num_levels, const int* hw_host, int N, int A, int ch, int R,
                        const float* anchors, const int64_t* pos_idx, const unsigned char* pos_valid, int npos, const int64_t* neg_idx,
                        const unsigned char* neg_valid, int nneg, const int* matched, const unsigned char* has_gt, const float* gt_boxes,
                        const float* gt_scores, int G, const float* weights_host, int loc_mode, float beta, float scale_clamp, float* sums,
                        float* gobj, float* gdl, utv2_stream_t stream);
int utv2_rpn_loss_fwd_range_f(const float* obj, const float* deltas, int head, int num_levels, const int* hw_host, int N, int batch, int img0,
                              int A, int ch, int R, const float* anchors, const int64_t* pos_idx, const unsigned char* pos_valid, int npos,
                              const int64_t* neg_idx, const unsigned char* neg_valid, int nneg, const int* matched,
                              const unsigned char* has_gt, const float* gt_boxes, const float* gt_scores, int G, const float* weights_host,
                              int loc_mode, float beta, float scale_clamp, float* sums, float* gobj, float* gdl, utv2_stream_t stream);
/* Labelling + random subsampling of anchors / proposals (rpn.py:112-148 -> D2 label_and_sample_anchors + subsample_labels;
 * roi_heads.py:141-270 -> D2 Matcher + _sample_proposals).  Random choice = the k smallest of one uniform key in [0, 1) per slot (keys
 * from the caller); equal keys are taken in slot order.
 * rpn_sample_keys: max_iou / lowq [N][R] (utv2_match_boxes / utv2_match_lowq), labels: IoU < lo negative, >= hi or lowq positive, image
 * without gt all negative; out [2N][R]: row n = positives of image n, row N + n its negatives, -1 = not a candidate, else a sortable key
 * (input of utv2_topk_rows_i64 with k = max(npos_max, nneg_max)).  rpn_sample_unpack: top [2N][k] selected keys -> pos_idx [N][npos_max]
 * / neg_idx [N][nneg_max] (ascending key order) and their valid flags; negatives are valid up to nneg_max - #positives; has_gt [N].
 * roi_sample: boxes [N][P][4] (proposals ++ gt, P <= 4096), valid [N][P], max_iou / argmax [N][P] against gt_* [N][G]; foreground = matched
 * IoU >= iou_thr in an image with gt; per image <= nfg_max foreground then background up to `batch` slots: out_boxes [N][batch][4],
 * out_classes (int64: gt class, num_classes = background, -1 = empty slot), out_gt_boxes, out_valid, out_idx (slot in [0, P)), and - when
 * gt_scores / gt_std [N][G] / [N][G][4] and the outputs are given - the matched pseudo box's score and std logits. */
int utv2_rpn_sample_keys(const float* max_iou, const unsigned char* lowq, const unsigned char* gt_valid, int G, const float* keys, int N,
                         int R, float lo, float hi, int64_t* out, utv2_stream_t stream);
/* _b: rpn_sample_keys with MODEL.RPN.BOUNDARY_THRESH (rpn.py:125-131).  boundary_thresh >= 0: once an anchor's label is final - after the
 * IoU thresholds, the low-quality matches and the all-negative labels of an image without gt - D2's Boxes.inside_box decides: anchors
 * [R][4] row r is inside image n (image_hw [N][2]: its own height and width, not the padded canvas) if x1 >= -t && y1 >= -t &&
 * x2 < W + t && y2 < H + t; an anchor that is not inside is a candidate for neither row.  boundary_thresh < 0: anchors / image_hw are
 * not read (NULL allowed) and the output is utv2_rpn_sample_keys', which forwards here with (NULL, NULL, -1).
 * boundary_thresh >= 0 with anchors or image_hw NULL, a NaN boundary_thresh: UTV2_EARG, nothing is launched. */
int utv2_rpn_sample_keys_b(const float* max_iou, const unsigned char* lowq, const unsigned char* gt_valid, int G, const float* keys, int N,
                           int R, float lo, float hi, const float* anchors, const float* image_hw, float boundary_thresh, int64_t* out,
                           utv2_stream_t stream);
int utv2_rpn_sample_unpack(const int64_t* top, int k, int N, int npos_max, int nneg_max, const unsigned char* gt_valid, int G,
                           int64_t* pos_idx, unsigned char* pos_valid, int64_t* neg_idx, unsigned char* neg_valid, unsigned char* has_gt,
                           utv2_stream_t stream);
int utv2_roi_sample(const float* boxes, const unsigned char* valid, const float* max_iou, const int* argmax, const float* keys, int N, int P,
                    const float* gt_boxes, const int* gt_classes, const unsigned char* gt_valid, const float* gt_scores, const float* gt_std,
                    int G, float iou_thr, int num_classes, int batch, int nfg_max, float* out_boxes, int64_t* out_classes,
                    float* out_gt_boxes, unsigned char* out_valid, int64_t* out_idx, float* out_conf, float* out_std, utv2_stream_t stream);
/* box_reg_loss / box_reg_pseudo_loss of the boundary-variance predictor (roi_heads/fast_rcnn.py:938-1090) on R sampled ROIs, summed:
 * deltas / stdl = the predicted boundary deltas and std logits, 4 * nbox columns per row (row pitch ld floats): nbox = 1 (class-agnostic)
 * or num_classes (CLS_AGNOSTIC_BBOX_REG False: a foreground row reads columns 4*cls .. 4*cls+3 of both, fast_rcnn.py:950-959,
 * :1036-1045); cls [R] int64 (-1 = empty slot, foreground = [0, num_classes)), prop / gtb [R][4] proposal and matched gt boxes, gstd
 * [R][4] the pseudo boxes' std logits or NULL (read in mode 2 only, like ts_better and t_cert).
 * mode 0: nlloss (L1 + 0.05 sum NLL * IoU, gradient through the IoU), 1: smooth_l1 at beta 0, 2: tsbetter, 3: pseudo smooth_l1.
 * Writes sum[0] and gdeltas / gstd_out [R][4*nbox] (Box2BoxXYXYTransform weights wx, wy and clamp): the derivatives in the selected four
 * columns, 0 everywhere else (background and empty rows: all 0) - every element is written by this launch.  One workgroup sums in a
 * fixed order, the same for both layouts: nbox = num_classes on the full matrix and nbox = 1 on the pre-gathered four columns give the
 * same bits in the sum and on every foreground row (a background row's zeros are signed, sign(d - t) * 0, when nbox == 1).
 * Accepted: R >= 0 (R == 0: sum 0), num_classes >= 1, nbox == num_classes or nbox == 1, ld >= 4*nbox (the pitch of deltas and of stdl),
 * mode 0..3, and mode 2 with nbox == 1 only (tsbetter has no per-class form in the reference); anything else: UTV2_EARG.
 * The caller's contract, NOT checked: cls (device data) in [-1, num_classes] (a value outside is treated as background); prop, gtb,
 * gdeltas and gstd_out are dense and 16-byte aligned (float4 accesses) - deltas / stdl are read as scalars: any 4-byte aligned
 * address and any pitch ld >= 4*nbox.
 * _f: the same with MODEL.ROI_BOX_HEAD.SMOOTH_L1_BETA and BBOX_REG_LOSS_TYPE "giou".  smooth_l1_beta: the L1 terms of modes 0, 1 and 3
 * become fvcore's smooth_l1_loss - beta < 1e-5: |d| (derivative sign(d)); else 0.5 d^2 / beta where |d| < beta (derivative d / beta) and
 * |d| - 0.5 beta from |d| == beta on (derivative sign(d)).  Mode 0's NLL term does not depend on it: the reference's nl_loss takes
 * `beta` and never reads it (fast_rcnn.py:1228-1292).  Mode 2 ignores it (the reference calls its smooth-L1 at 0.0, :1070-1075).
 * mode 4: "giou" (fast_rcnn.py:998-1002) - the foreground row's deltas of its class decoded by Box2BoxXYXYTransform.apply_deltas
 * (wx, wy, scale_clamp), fvcore's giou_loss (eps 1e-7) against the matched gt box, summed; gdeltas = its derivative through the decode
 * (0 where the clamp cuts), gstd_out all 0 (the std head has no part in it); stdl and smooth_l1_beta have no effect.
 * Accepted: what utv2_roi_box_loss accepts, mode 0..4, smooth_l1_beta >= 0 (+inf included); a negative or NaN beta, mode 5..: UTV2_EARG.
 * utv2_roi_box_loss = _f at beta 0 (the same arithmetic as ever: nothing divides by beta there) with mode 0..3; its mode 4: UTV2_EARG. */
int utv2_roi_box_loss_f(const float* deltas, const float* stdl, int64_t ld, const int64_t* cls, const float* prop, const float* gtb,
                        const float* gstd, int R, int num_classes, int nbox, int mode, float wx, float wy, float scale_clamp,
                        float ts_better, float t_cert, float smooth_l1_beta, float* sum, float* gdeltas, float* gstd_out,
                        utv2_stream_t stream);
int utv2_roi_box_loss(const float* deltas, const float* stdl, int64_t ld, const int64_t* cls, const float* prop, const float* gtb,
                      const float* gstd, int R, int num_classes, int nbox, int mode, float wx, float wy, float scale_clamp, float ts_better,
                      float t_cert, float* sum, float* gdeltas, float* gstd_out, utv2_stream_t stream);
/* roi_heads/fast_rcnn.py:925-936 + FocalLoss :1405-1429 (softmax CE focal, gamma 1.5), summed.  Accepted: R >= 0, any C >= 1 (one wave
 * strides over the row); R < 0 or C < 1: UTV2_EARG.  The caller's contract, NOT checked (device data): target in [-1, C) (-1 = row
 * skipped) - a target >= C reads past the row. */
int utv2_softmax_focal_fwd(const float* logits, const int* target, int R, int C, float gamma, float* loss_sum, float* ws,
                           utv2_stream_t stream);
int utv2_softmax_focal_bwd(const float* logits, const int* target, int R, int C, float gamma, const float* coef,
                           float* dlogits, utv2_stream_t stream);
/* The scalar tail of the Faster-RCNN UTv2 losses in one launch (roi_heads/fast_rcnn.py:925-936 normalisation by the number of sampled
 * ROIs, proposal_generator/rpn.py:214-224 normalisation + loss weights, engine/trainer.py:880-893 weighting and sum): raw kernel sums of
 * the supervised and the pseudo branch -> rec[9] = {loss_cls, loss_box_reg, loss_rpn_cls, loss_rpn_loc} x {supervised, pseudo}, total;
 * coef[8] = d total / d raw sum.  wt_host: host float[8], the trainer's weight per loss in rec order.  tgt_* may be null when its n is 0. */
int utv2_rcnn_loss_combine(const float* rpn_sup, const float* rpn_uns, const float* focal_sup, const float* focal_uns, const float* box_sup,
                           const float* box_uns, const int* tgt_sup, int n_sup, const int* tgt_uns, int n_uns, float rpn_norm_sup,
                           float rpn_norm_uns, float w_rpn_cls, float w_rpn_loc, float w_box, const float* wt_host, float* rec, float* coef,
                           utv2_stream_t stream);

/* ---- the frozen ResNet stem as ONE kernel (csrc/stem_pool.hip): D2 BasicStem conv1 (7x7 stride 2 pad 3, 3 -> 64, FrozenBN as scale /
 * shift, ReLU) + max_pool2d(3, 2, 1), the first two layers of the R-50 the reference builds (backbone/fpn.py:21-22).  xpad16 / w16s as
 * for utv2_conv2d_stem_fwd_bf16 (W even); y: 16-bit [N][PH][PW][64], OH = (H - 1) / 2 + 1, PH = (OH - 1) / 2 + 1 (same for W).  The conv
 * output never leaves LDS. */
int utv2_stem_pool_fwd_bf16(const void* xpad16, const void* w16s, void* y, const float* scale, const float* shift, int N, int H, int W,
                            int K, utv2_stream_t stream);

/* ---- one frozen ResNet bottleneck as ONE kernel (csrc/bottleneck.hip): D2 BottleneckBlock conv1 1x1 -> conv2 3x3 -> conv3 1x1 + identity
 * (or + the 1x1 shortcut conv of a stage's first block), FrozenBN folded to scale / shift, of the R-50 the reference builds through
 * build_fcos_resnet_fpn_backbone (ubteacher/modeling/backbone/fpn.py:21-22; res2 under MODEL.BACKBONE.FREEZE_AT 2).
 * x: [N, H, W, C], y: [N, H, W, 256] of the library's 16-bit type, y != x; w1 [MID = 64][C], w2 [MID][3][3][MID], w3 [256][MID] 16-bit;
 * s* / b*: fp32 per output channel.  wsc NULL (C = 256): y = relu(conv3(relu(conv2(relu(conv1(x) s1 + b1)) s2 + b2)) s3 + b3 + x);
 * wsc [256][C] (C = 64): ... + h16(shortcut(x) ssc + bsc) instead of + x.  The 64-channel intermediates never leave LDS. */
int utv2_bottleneck_supported(int C, int MID, int has_shortcut);
int utv2_bottleneck_fwd_bf16(const void* x, void* y, const void* w1, const void* w2, const void* w3, const void* wsc, const float* s1,
                             const float* b1, const float* s2, const float* b2, const float* s3, const float* b3, const float* ssc,
                             const float* bsc, int N, int H, int W, int C, int MID, utv2_stream_t stream);

/* ---- one frozen identity BasicBlock as ONE kernel (csrc/basicblock.hip): D2 BasicBlock conv1 3x3 -> conv2 3x3 + identity, both stride 1
 * pad 1 and 64 -> 64 channels, FrozenBN folded to scale / shift - every res2 block of R-18 / R-34 (MODEL.RESNETS.DEPTH 18 / 34 with
 * RES2_OUT_CHANNELS 64) under MODEL.BACKBONE.FREEZE_AT 2.
 * x, y: [N, H, W, C = 64] of the library's 16-bit type, y != x; w1, w2: [64][3][3][64] 16-bit (tap-major, channel-minor: the layout
 * utv2_conv2d_nhwc_fwd_bf16_bits reads); s* / b*: fp32 per output channel.
 * c1 = h16(relu(conv1(x) s1 + b1)), zero outside the image; y = h16(relu(conv2(c1) s2 + b2 + x)): fp32 accumulation and the roundings of the
 * two-launch chain (conv, ReLU; conv, residual x, ReLU).  c1 never leaves LDS.  C != 64, y == x, a null operand or an image of more than
 * 2^31 - 1 elements: UTV2_EARG.
 * utv2_basicblock_supported: 1 when the kernel takes a block of C channels whose conv1 has this stride, with / without a shortcut conv
 * ((64, 1, 0) only). */
int utv2_basicblock_supported(int C, int stride, int has_shortcut);
int utv2_basicblock_fwd_bf16(const void* x, void* y, const void* w1, const void* w2, const float* s1, const float* b1, const float* s2,
                             const float* b2, int N, int H, int W, int C, utv2_stream_t stream);

/* ---- two-crop data path: the pixel arithmetic of the reference's weak / strong views, on uint8 [H][W][3] images
 * in HBM, bit-exact to Pillow (which Detectron2 / torchvision / the reference call on the CPU) ------------------------------------- */
/* detectron2 ResizeTransform.apply_image (used by ubteacher/data/dataset_mapper.py:97-99) = PIL.Image.resize(BILINEAR): Resample.c
 * two-pass 8.22 fixed-point convolution; flip != 0 also applies HFlipTransform.  ws >= utv2_aug_resize_workspace_bytes bytes */
int64_t utv2_aug_resize_workspace_bytes(int H, int W, int OH, int OW);
int utv2_aug_resize_bilinear_u8(const unsigned char* src, int H, int W, unsigned char* dst, int OH, int OW, int flip, void* ws,
                                utv2_stream_t stream);
/* ubteacher/data/detection_utils.py:20-23 ColorJitter on PIL images = ImageEnhance.{Brightness,Contrast,Color} = Blend.c ImagingBlend
 * against a degenerate image: mode 0 black, 1 the constant *mean (from utv2_aug_gray_mean_u8: int(mean(L) + 0.5)), 2 the L image */
int utv2_aug_gray_mean_u8(const unsigned char* img, int64_t npix, void* sum_ws, int* mean_out, utv2_stream_t stream);
int utv2_aug_blend_u8(unsigned char* img, int64_t npix, int mode, float alpha, const int* mean, utv2_stream_t stream);
/* torchvision F_pil.adjust_hue: Convert.c rgb2hsv, H += shift (uint8 wrap), hsv2rgb */
int utv2_aug_hue_u8(unsigned char* img, int64_t npix, int shift, utv2_stream_t stream);
/* detection_utils.py:24 RandomGrayscale: convert("L") replicated to 3 channels */
int utv2_aug_grayscale_u8(unsigned char* img, int64_t npix, utv2_stream_t stream);
/* data/transforms/augmentation_impl.py:7-22 GaussianBlur = PIL.ImageFilter.GaussianBlur = 3 + 3 passes of BoxBlur.c; one pass per call
 * (radius / ww / fw = the pass constants of ImagingHorizontalBoxBlur), src != dst */
int utv2_aug_box_blur_u8(const unsigned char* src, unsigned char* dst, int H, int W, int vertical, int radius, int ww, int fw,
                         utv2_stream_t stream);
/* detection_utils.py:27-41 ToTensor -> RandomErasing(value="random") -> ToPILImage: rectangle <- (noise[3][h][w] * 255).byte() */
int utv2_aug_erase_u8(unsigned char* img, int H, int W, int i, int j, int h, int w, const float* noise, utv2_stream_t stream);
/* dataset_mapper.py:139-147 image_strong_aug.transpose(2, 0, 1) */
int utv2_aug_hwc_to_chw_u8(const unsigned char* src, unsigned char* dst, int64_t npix, utv2_stream_t stream);

/* ---- COCO box evaluation (evaluation/coco_eval_device.py; the metric of Detectron2's COCOEvaluator behind the reference's
 * build_evaluator), bit-identical to evaluation/coco_eval.py.  Detections / ground truth are CSR by image (off: device int64[N+1]) in the
 * evaluator's image order; an (image, class) pair has the id image * (K + 1) + class, class K standing for every class outside [0, K).
 * ubteacher/hip.py:coco_box_eval chains these with three stable sorts (torch.sort) of the keys - see csrc/coco_eval.hip. */
/* keys[i] = pid << 32 | descending-score bits of scores[i] (scores NULL: 0) */
int utv2_coco_pair_keys(const float* scores, const int* cls, const long long* off, int N, int K, long long* keys, utv2_stream_t stream);
/* keys ascending: off[s] = first i with (keys[i] >> 32) >= s for s in [0, nseg] (ids above nseg count as nseg) */
int utv2_coco_seg_offsets(const long long* keys, int64_t n, int64_t nseg, long long* off, utv2_stream_t stream);
/* key1 sorted, pair_off its pair offsets: key2[p] = class << 32 | score bits when the class is < K and the rank of p inside its pair is
 * < max_dets (else K << 32), rank[p] = that rank (255 when excluded); max_dets <= 254 */
int utv2_coco_rank_keys(const long long* key1, const long long* pair_off, int64_t D, int K, int max_dets, long long* key2,
                        unsigned char* rank, utv2_stream_t stream);
/* the matched / ignored bits of every (sorted detection, area, IoU threshold) + the non-ignored ground-truth counts per (class, area),
 * written by utv2_coco_match into ws and read by utv2_coco_accumulate */
int64_t utv2_coco_eval_workspace_bytes(int64_t D, int K);
/* dbox fp32 [D][4] xyxy, dperm: sorted position -> detection; gbox fp64 [G][4], gcrowd uint8, garea fp64 (NULL: box areas), gperm: sorted
 * position -> ground truth; *_pair_off int64[N*(K+1)+1].  max_gt >= the ground-truth count of any pair (<= 12800);
 * iou_thrs_host[10], area_rng_host[4][2] (lo, hi of all / small / medium / large) */
int utv2_coco_match(const float* dbox, const long long* dperm, const long long* dpair_off, const double* gbox, const unsigned char* gcrowd,
                    const double* garea, const long long* gperm, const long long* gpair_off, int N, int K, int64_t D, int max_dets,
                    int max_gt, const double* iou_thrs_host, const double* area_rng_host, void* ws, utv2_stream_t stream);
/* perm2: position in the class-merged order -> sorted position; cat_off int64[K+1]; rec_thrs_host[101].
 * precision fp64 [10][101][K][4], recall fp64 [10][K][4][3] (maxDets 1, 10, max_dets); -1 where the class has no ground truth */
int utv2_coco_accumulate(const long long* perm2, const long long* cat_off, const unsigned char* rank, int K, int64_t D,
                         const double* rec_thrs_host, const void* ws, double* precision, double* recall, utv2_stream_t stream);

/* ---- grouped 3x3 convolution (ResNeXt conv2, modeling/backbone.py; D2 BottleneckBlock with num_groups > 1) -----------------------
 * NHWC, pad 1, stride 1 or 2, C input = C output channels in G groups of g = C / G (g % 4 == 0); OH = (H - 1) / stride + 1.
 * w = the arena matrix [C][3][3][g], element type op_dtype like the activation operand (UTV2_F32: exact fp32 mode; UTV2_BF16: the
 * library's 16-bit type); fp32 accumulation; one launch for all groups (csrc/conv_grouped.hip).
 * fwd:   y = relu?(conv(x, w) * scale[k] + shift[k]) (scale / shift NULL: 1 / 0); y_dtype UTV2_F32 or op_dtype.
 * dgrad: dx = dgrad(dy) with scale[k] (NULL: 1) folded into the weights; then dx = mask > 0 ? dx : 0 (mask NULL: none), dx += residual;
 *        mask / residual have dx's element type.
 * wgrad: dw[k][kh][kw][c] (+)= scale[k] * sum_m dy[m][k] * x[...]: split over output pixels into ws, the splits added in a fixed order by
 *        a second launch (deterministic, no atomics). */
int utv2_gconv3x3_supported(int C, int G);
int utv2_gconv3x3_fwd(const void* x, const void* w, int op_dtype, void* y, int y_dtype, const float* scale, const float* shift, int N,
                      int H, int W, int C, int G, int stride, int OH, int OW, int relu, utv2_stream_t stream);
int utv2_gconv3x3_dgrad(const void* dy, const void* w, int op_dtype, void* dx, int dx_dtype, const float* scale, const void* mask,
                        const void* residual, int N, int H, int W, int C, int G, int stride, int OH, int OW, utv2_stream_t stream);
int utv2_gconv3x3_wgrad_splits(int N, int OH, int OW, int C, int G);
int64_t utv2_gconv3x3_wgrad_workspace_floats(int N, int OH, int OW, int C, int G);
int utv2_gconv3x3_wgrad(const void* x, const void* dy, int op_dtype, float* dw, float* ws, const float* scale, int N, int H, int W,
                        int C, int G, int stride, int OH, int OW, int accumulate, utv2_stream_t stream);

/* ---- BatchNorm2d + ReLU of the FCOS towers (MODEL.FCOS.NORM "BN" / "SyncBN", fcos/fcos.py:262-281; csrc/batchnorm.hip) --------------
 * x, y, dy, dx: level-first [P, C] matrices of one element type (`dtype`: UTV2_F32 or UTV2_BF16), C % 4 == 0.  Per-channel coefficients
 * and the per-element arithmetic are fp64, every output is rounded once (16-bit outputs through fp32); a NaN in x is a NaN in y (torch's
 * ReLU) and its gradient is masked like any y that is not > 0.
 * A STATISTIC SET s = rows [set_row0[s], set_row0[s] + set_rows[s]) = the rows of FPN level set_level[s] that one forward call of the
 * reference hands its BatchNorm2d; gamma / beta / running_* / dgamma / dbeta are [nlevels, C] fp32, mean / rstd / scale [nsets, C] fp64.  The set
 * tables are HOST arrays (at most 16 sets, from the canvas geometry), passed on by value: nothing depends on device data.
 * All sums are carried in fp64 and reduced in two stages of fixed order without atomics (bit-reproducible):
 *   stats_partial  partial[chunk][0 | 1][C] = sum x | sum x^2 over chunks of 64 rows (utv2_bn_chunks of them)
 *   reduce         out[s][0 | 1][C] = the set's chunks added up, divided by set_rows[s] when `divide` (-> [mean, mean of squares])
 *   finalize       mode 0: mean, var = moments[s][1] - moments[s][0]^2 (in fp64), rstd = 1 / sqrt(var + eps), scale = gamma * rstd; then
 *                  running_mean += momentum * (mean - running_mean), running_var likewise with var * n / (n - 1), n = set_rows[s] *
 *                  count_mul (biased_running: with var itself), the sets in order (two sets of a level: two sequential updates);
 *                  mode 1 (eval): mean / var = the level's running statistics, which are not written.  `moments` may be the mean of
 *                  several ranks' reduce outputs (count_mul = their number, equal set sizes).  n < 2 in mode 0: UTV2_EARG.
 *   apply_relu     y = relu(x * scale + shift), shift = beta - mean * scale, evaluated as (x - mean) * scale + beta; one rounding
 *   bwd_partial    partial[chunk][0 | 1][C] = sum g | sum g * xhat; g = dy * [y > 0], xhat = (x - mean) * rstd; then `reduce`, divide 0
 *   bwd_apply      dx = gamma * rstd * (g - sums[s][0] / n - xhat * sums[s][1] / n); dgamma[level] += sums[s][1] / count_mul,
 *                  dbeta[level] += sums[s][0] / count_mul, the sets in order.  `sums` may be the SUM over count_mul ranks. */
int utv2_bn_chunks(int nsets, const int* set_rows_host);
int utv2_bn_stats_partial(const void* x, int dtype, double* partial, int64_t P, int C, int nsets, const int* set_row0_host,
                          const int* set_rows_host, utv2_stream_t stream);
int utv2_bn_reduce(const double* partial, double* out, int C, int nsets, const int* set_rows_host, int divide, utv2_stream_t stream);
int utv2_bn_finalize(const double* moments, const float* gamma, float* running_mean, float* running_var, double* mean, double* rstd,
                     double* scale, int C, int nlevels, int nsets, const int* set_rows_host, const int* set_level_host, double eps,
                     double momentum, int mode, int count_mul, int biased_running, utv2_stream_t stream);
int utv2_bn_apply_relu(const void* x, void* y, int dtype, const double* mean, const double* scale, const float* beta, int64_t P, int C,
                       int nlevels, int nsets, const int* set_row0_host, const int* set_rows_host, const int* set_level_host,
                       utv2_stream_t stream);
int utv2_bn_bwd_partial(const void* dy, const void* y, const void* x, int dtype, const double* mean, const double* rstd, double* partial,
                        int64_t P, int C, int nsets, const int* set_row0_host, const int* set_rows_host, utv2_stream_t stream);
int utv2_bn_bwd_apply(const void* dy, const void* y, const void* x, void* dx, int dtype, const double* mean, const double* rstd,
                      const float* gamma, const double* sums, float* dgamma, float* dbeta, int64_t P, int C, int nlevels, int nsets,
                      const int* set_row0_host, const int* set_rows_host, const int* set_level_host, int count_mul, utv2_stream_t stream);

/* ---- TEST.PRECISE_BN for the BatchNorm towers (csrc/bn_precise.hip): population statistics estimated on the device --------------------
 * state: fp64 [nlevels][3][C] per layer = pop_mean | pop_sq (population mean of squares) | num (images seen, carried per channel);
 * zero-initialised by the caller.  The set tables are those of the section above; set_images_host[s] = B, the images of set s's call.
 *   precise_update  for the sets in order, from moments[s] = [mean, mean of squares] (utv2_bn_reduce with divide, or the mean of
 *                   count_mul ranks' outputs): var = max(moments[s][1] - mean^2, 0), v = var * n / (n - 1) with n = set_rows[s] *
 *                   count_mul (biased_running: v = var) - what utv2_bn_finalize mode 0 moves the running variance by - then
 *                   [fvcore-recall]  num += B; q = mean^2 + v * (B - 1) / B; pop_mean += (mean - pop_mean) * (B / num);
 *                   pop_sq += (q - pop_sq) * (B / num).  Also writes mean / rstd / scale [nsets][C] exactly as utv2_bn_finalize mode 0
 *                   does (bit for bit), for utv2_bn_apply_relu.  No running buffer is read or written.  One thread per channel, no atomics.
 *                   UTV2_EARG: C % 4 != 0, n < 2, B < 1, a bad set table, a null pointer.
 *   precise_commit  state: [nlayers][nlevels][3][C]; running_mean_host / running_var_host: HOST arrays of nlayers device pointers to
 *                   [nlevels][C] fp32.  running_mean = fp32(pop_mean), running_var = fp32(pop_sq - pop_mean^2), one rounding each; a
 *                   level whose num is 0 keeps its buffers. */
int utv2_bn_precise_update(const double* moments, const float* gamma, double* state, double* mean, double* rstd, double* scale, int C,
                           int nlevels, int nsets, const int* set_rows_host, const int* set_level_host, const int* set_images_host,
                           double eps, int count_mul, int biased_running, utv2_stream_t stream);
int utv2_bn_precise_commit(const double* state, float* const* running_mean_host, float* const* running_var_host, int nlayers, int nlevels,
                           int C, utv2_stream_t stream);

/* ---- test-time augmentation (TEST.AUG; Detectron2 GeneralizedRCNNWithTTA._inverse_augmented_boxes and the head of _merge_detections
 * [D2-recall]): the detections of the V views of ONE image, each in its view's pixel frame, brought back to the original image and
 * packed view-major into one candidate set for utv2_nms_batched.
 * boxes_host / scores_host / classes_host / valid_host: HOST arrays of V device pointers - view v's padded detections as the inference
 * chains leave them (boxes fp32 [D][4] xyxy, 16-byte aligned; scores fp32 [D]; classes int32 [D]; valid u8 [D]).
 * table: DEVICE fp32 [V][UTV2_TTA_STRIDE], the view's inverse transform chain: FLIP (0 / 1), WVIEW (the view's width, read when FLIP),
 * RX_VIEW / RY_VIEW = fp32(w_loader / w_view) / fp32(h_loader / h_view), RX_LEAD / RY_LEAD = fp32(w_orig / w_loader) /
 * fp32(h_orig / h_loader) (1 when the loader image is the original), ORIG_H / ORIG_W.
 * Per slot, in fp32 with one rounding per operation: x <- WVIEW - x when FLIP, (x1, x2) <- (min, max), x *= RX_VIEW, x *= RX_LEAD (y
 * likewise), clip to [0, ORIG_W] x [0, ORIG_H]; ovalid = valid && score > 1e-8f.  Outputs [V * D] (oboxes [V * D][4], 16-byte aligned);
 * a slot that is not valid is written as zeros.  One thread per (view, slot), one launch per UTV2_TTA_MAX_VIEWS views, no atomics.
 * Checked (UTV2_EARG, nothing launched): non-null pointers (each view's included), the alignment, V >= 1, D >= 1, V * D < 2^31. */
#define UTV2_TTA_MAX_VIEWS 32
#define UTV2_TTA_STRIDE 8
#define UTV2_TTA_FLIP 0
#define UTV2_TTA_WVIEW 1
#define UTV2_TTA_RX_VIEW 2
#define UTV2_TTA_RY_VIEW 3
#define UTV2_TTA_RX_LEAD 4
#define UTV2_TTA_RY_LEAD 5
#define UTV2_TTA_ORIG_H 6
#define UTV2_TTA_ORIG_W 7
int utv2_tta_collect(const void* const* boxes_host, const void* const* scores_host, const void* const* classes_host,
                     const void* const* valid_host, const float* table, int V, int D, float* oboxes, float* oscores, int* oclasses,
                     unsigned char* ovalid, utv2_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif
