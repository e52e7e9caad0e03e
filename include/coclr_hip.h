/*
 * coclr_hip.h -- C ABI of libcoclr_hip.so, the gfx950 (MI355X / CDNA4) kernel
 * library under the CoCLR training hot path.
 *
 * The reference (TengdaHan/CoCLR) has no FFI of its own: every FLOP of
 * model/pretrain.py and backbone/{s3dg,resnet_2d3d}.py is an implicit call
 * into ATen/cuDNN/NCCL.  Each entry point below therefore cites the ATen op
 * *call site* in the reference that it replaces (file:line under the
 * reference root).  The Python host (coclr_amd/) binds these with ctypes;
 * INTEGRATION.md shows the stub.
 *
 * Conventions
 *   - all tensors are device pointers to contiguous fp32 unless noted,
 *     NCDHW for activations, [Cout][Cin][kt][kh][kw] for conv weights
 *   - every function enqueues work on `stream` (a hipStream_t passed as
 *     void*; NULL = the legacy default stream), never synchronises, never
 *     allocates device memory and keeps no pointer after returning
 *   - return value: 0 on success, otherwise a hipError_t value
 *     (1 == hipErrorInvalidValue is also used for rejected arguments)
 *   - "nstride" arguments are the distance in floats between consecutive
 *     samples, so a tensor may be a channel slice of a wider buffer
 */
#ifndef COCLR_HIP_H_
#define COCLR_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ------------------------------------------------------------------------ */
/* Convolution (backbone/s3dg.py:11-13,25,39-42,59,62;                      */
/*              backbone/resnet_2d3d.py:53-59,67-79,138,192; head convs      */
/*              model/pretrain.py:52,54 when applied to un-pooled maps)      */
/* ------------------------------------------------------------------------ */

typedef struct coclr_conv_desc {
  int32_t N, Cin, Cout;
  int32_t Ti, Hi, Wi;      /* input extent  */
  int32_t To, Ho, Wo;      /* output extent */
  int32_t kt, kh, kw;      /* stencil       */
  int32_t st, sh, sw;      /* stride        */
  int32_t pt, ph, pw;      /* zero padding  */
  int32_t dt, dh, dw;      /* input dilation (zero insertion); 1 for a forward conv,
                              = forward stride when the call computes a data gradient */
  int64_t x_nstride;       /* floats between input samples  (>= Cin*Ti*Hi*Wi)  */
  int64_t y_nstride;       /* floats between output samples (>= Cout*To*Ho*Wo) */
  /* Destination lattice (phase-decomposed data gradient of a strided conv): output
   * position o of this launch is element o*ys + yo of a (yT, yH, yW) tensor.
   * ys_t == 0 selects the dense case (ys = 1, yo = 0, extent = To/Ho/Wo). */
  int32_t ys_t, ys_h, ys_w;
  int32_t yo_t, yo_h, yo_w;
  int32_t yT, yH, yW;
  int32_t Nx;              /* samples addressable through n_index (0: N) */
  int32_t algo;            /* 0: direct; 1: Winograd, w_packed must then be the transform-domain
                              operand made by coclr_conv_pack_weights(transpose | 2):
                              (3,1,1) stencil, stride 1, pad (1,0,0), no n_index: F(2,3) along T, taps = 4;
                              (1,3,3) stencil, stride 1, pad (0,1,1), even Ho/Wo >= 4, dense
                              destination, no n_index: F(2x2,3x3), taps = 16;
                              (7,1,1) stencil, stride (2,1,1), pad (3,0,0), Ti = 2 To, >= 8 output
                              frames, dense destination, no n_index: polyphase form of the temporal stem
                              conv (backbone/s3dg.py:41,145) -- F(2,3) on the odd taps + F(2,4) on the even
                              ones, taps = 9 (forward operand only);
                              2: (3,1,1) stencil, stride 1, pad (1,0,0), no n_index: F(4,3) along T,
                              taps = 6 (six contractions per quad of output frames);
                              (4,1,1) stencil, stride 1, pad (1,0,0), To = Ti: F(2,4) along T, taps = 5.
                              The algo = 2 kernels also write through a destination lattice along T
                              (ys_t > 0, ys_h = ys_w = 1): the two phases of a strided temporal data gradient */
} coclr_conv_desc;

/* Number of fp32 elements of the packed-weight buffer for one conv. */
int coclr_conv_packed_size(int cin, int cout, int taps, int transpose, int64_t* elems);

/* Re-lay [Cout][Cin][taps] weights as [taps][R'][C'] (zero padded: reduction
 * channels R to x32, produced channels C to x128).
 * transpose=0: operand of the forward conv (R = Cin, C = Cout); transpose=1: operand of
 * the data gradient (R = Cout, C = Cin, stencil flipped); transpose | 2: Winograd operand
 * (coclr_conv_desc.algo >= 1) -- taps = 4: the four F(2,3) matrices of a 3-tap temporal stencil,
 * taps = 6: its six F(4,3) matrices (algo = 2), taps = 5: the five F(2,4) matrices of a 4-tap temporal stencil,
 * taps = 9: the 4 + 5 polyphase matrices of the 7-tap stride-2 stem conv (the source taps are then tap_base +
 * t*tap_step, t = 0..6; transpose = 0 only),
 * taps = 16: the sixteen F(2x2,3x3) matrices U = G g G^T of a 9-tap spatial stencil, laid out
 * [R'][C'][16] (stand-alone operands only).  co/ci strides, tap_base and
 * tap_step address a sub-stencil: source tap of packed tap t is tap_base + t*tap_step
 * (one kt-slice of a (5,7,7) stem; the taps of one phase of a strided data gradient).
 * rows_total/cols_total > 0 place this tensor at (row0, col0) of a WIDER packed operand
 * [taps][pad32(rows_total)][pad128(cols_total)] that the caller has zero-filled: several
 * convs that read the same input (the three 1x1x1 heads of an inception block,
 * backbone/s3dg.py:97-112) then run as one convolution over concatenated channels. */
int coclr_conv_pack_weights(const float* w, float* packed, int cout, int cin, int taps,
                            int64_t co_stride, int64_t ci_stride, int tap_base, int tap_step,
                            int transpose, int row0, int rows_total, int col0, int cols_total,
                            void* stream);

/* The same re-layouts, many at once (every operand of an encoder: ~80 tiny launches per pass
 * otherwise).  coclr_conv_pack_describe validates one request exactly as
 * coclr_conv_pack_weights would and writes it as a 16-word table row plus the number of
 * 1024-element blocks it needs; the caller uploads the rows and a block map
 * int32[nblocks][2] = {row, block index within the row} and launches them all with
 * coclr_conv_pack_batch.  The pointers in a row must stay valid for every replay. */
int coclr_conv_pack_describe(const float* w, float* packed, int cout, int cin, int taps,
                             int64_t co_stride, int64_t ci_stride, int tap_base, int tap_step,
                             int transpose, int row0, int rows_total, int col0, int cols_total,
                             int64_t* entry, int32_t* nblocks);
int coclr_conv_pack_batch(const int64_t* table, const int32_t* blockmap, int nblocks,
                          void* stream);

/* Number of per-workgroup BatchNorm partial sums coclr_conv3d_fwd will emit
 * per channel for this geometry (stats buffer = 2 * Cout * ntiles floats). */
int coclr_conv3d_ntiles(const coclr_conv_desc* d, int* ntiles);

/* y (+)= act(affine(conv(x, w) + bias)).  Replaces aten::conv3d forward and,
 * with transposed weights + input dilation, the dgrad half of
 * aten::convolution_backward.  stats (optional): [2][Cout][ntiles] partial
 * sum / sum-of-squares of the raw conv output for train-mode BatchNorm
 * (backbone/s3dg.py:16,46-47).  n_index (optional): x sample n is read from
 * sample n_index[n] -- the shuffle-BN row gather of model/pretrain.py:124
 * folded into the first conv.  Only the direct kernels gather: COCLR_EINVAL with
 * algo >= 1. */
int coclr_conv3d_fwd(const coclr_conv_desc* d, const float* x, const float* w_packed, float* y,
                     float* stats, const float* bias, const float* ep_scale,
                     const float* ep_shift, const int64_t* n_index, int relu, int accumulate,
                     void* stream);

/* Several INDEPENDENT convolutions in one call; consecutive pairs (0,1), (2,3), ... that resolve to the
 * same kernel variant run as ONE launch whose grid holds the tiles of both problems.  Replaces two
 * aten::conv3d calls of sibling branches: the (1,3,3) / (3,1,1) convolutions of branch1 and branch2 of an
 * inception block (backbone/s3dg.py:100-118), forward and data gradient -- on the 8x8x8 / 4x4x4 maps each
 * of them alone is a 10-40 us launch that leaves most of the chip idle.  Per-problem arguments are those
 * of coclr_conv3d_fwd.  Every problem keeps the plan it would have alone (same tiles, same statistics
 * layout: coclr_conv3d_ntiles), so outputs and statistics are bit-identical to separate calls.
 * COCLR_PAIR=0 in the environment launches every problem on its own. */
typedef struct coclr_conv_call {
  const coclr_conv_desc* d;
  const float* x;
  const float* w_packed;
  float* y;
  float* stats;
  const float* bias;
  const float* ep_scale;
  const float* ep_shift;
  const int64_t* n_index;
  int32_t relu, accumulate;
  /* Data gradient whose destination y is the dz of a BatchNorm(+ReLU) unit (the producer of the tensor
   * this convolution read in forward): bwd_y = that unit's convolution output, laid out exactly like y,
   * bwd_scale / bwd_shift / bwd_mean / bwd_invstd its per-channel coefficients.  The kernel then also
   * forms the unit's backward sums while dz is in registers -- g = dz where bwd_relu == 0 or
   * bwd_y*scale + shift > 0; stats[0][c][tile] = sum g, stats[1][c][tile] = sum g*(bwd_y - mean)*invstd --
   * and coclr_bn_act_backward_multi takes them as `part` instead of running its reduction pass over dz
   * and y (aten::native_batch_norm_backward's sums + threshold_backward; backbone/s3dg.py:46-48,60-64).
   * Requires stats, no accumulate / bias / ep_* / relu / n_index, and a kernel that has the epilogue
   * (coclr_conv3d_bwd_sums_ok; COCLR_EINVAL otherwise).  All NULL / 0: a plain call. */
  const float* bwd_y;
  const float* bwd_scale;
  const float* bwd_shift;
  const float* bwd_mean;
  const float* bwd_invstd;
  int32_t bwd_relu;
  /* The input x is the RAW convolution output of a BatchNorm(+ReLU) unit whose apply pass has not run:
   * the kernel applies x' = x * in_scale[ci] + in_shift[ci] (max(., 0) when in_relu) to every element it
   * reads, zero padding staying zero -- the normalised tensor is never written or re-read (the apply pass
   * of backbone/s3dg.py:46-48 fused into the NEXT convolution of the separable unit, :49).  Only the
   * kernels that move their B operand through registers support it (the polyphase temporal stem conv);
   * COCLR_EINVAL otherwise.  NULL: a plain call. */
  int32_t in_relu;
  const float* in_scale;
  const float* in_shift;
} coclr_conv_call;
int coclr_conv3d_fwd_multi(const coclr_conv_call* calls, int n, void* stream);
int coclr_conv3d_bwd_sums_ok(const coclr_conv_desc* d, int* ok);

/* What coclr_conv3d_fwd / coclr_conv3d_fwd_multi would launch for this descriptor (x_nstride, y_nstride and Nx
 * filled in as for the launch); launches nothing (ABI 24).  Comes from the launcher's own planner and kernel
 * selection, so a test can assert which instantiation a geometry reaches.  Returns what the launch would return
 * before launching (COCLR_EINVAL for a refused combination).
 * flags: 1 x is 16-byte aligned, 2 y is 8-byte aligned, 4 an n_index is given, 8 an in-affine (in_scale) is given,
 *        16 the call sits in a pair slot of coclr_conv3d_fwd_multi, 32 backward sums (bwd_y) are asked for.
 * out:
 *   [0]  planner variant
 *   [1]  kernel family: 0 conv_igemm_kernel, 1 conv_wino_tf_kernel<WinoF23> (F(2,3); reported as a family of
 *        its own, as when it had a kernel of its own), 2 conv_wino_tf_kernel in its other forms,
 *        3 conv_wino_hw_kernel, 4 conv_wino_hw8_kernel, 5 conv_stem_kernel
 *   [2]  family 2: matrices of the form (6: F(4,3), 5: F(2,4), 9: polyphase stem); 0 otherwise
 *   [3..10]  template numbers KT KH KW CC BM BN PCH OCC (0: the kernel has none)
 *   [11..16] XV4, XG, X16, INAFF, destination lattice, pairable (a two-problem kernel exists and would be used)
 *   [17..20] log2 box extents lTW lTH lTT lTN
 *   [21..24] window WT WH WW (floats; widened to whole granules by XG / X16) and plane (floats; granules with
 *            XG / X16)
 *   [25..28] ntiles, mtiles, nchunks, planeS (LDS pitch of a staged channel)
 *   [29..31] dynamic LDS bytes, workgroups, threads per workgroup
 *   [32] 1 if this call would fill its pair slot instead of launching
 *   [33..37] boxes covering the output and their count per axis (w, h, t, n)
 *   [38] 1 if the kernel can form backward sums (coclr_conv3d_bwd_sums_ok) */
int coclr_conv3d_fwd_plan(const coclr_conv_desc* d, int flags, int32_t out[40]);

/* Split-K workspace (fp32 elements) for coclr_conv3d_wgrad. */
int coclr_conv3d_wgrad_workspace(const coclr_conv_desc* d, int64_t* elems);

/* What coclr_conv3d_wgrad would launch for this descriptor; launches nothing.  Comes from the launcher's own
 * planner and kernel selection, so a test can assert which instantiation a geometry reaches.
 * operands_16B_aligned: whether x and dy will both be 16-byte aligned (the launcher checks the pointers; the
 * 16-byte-DMA pointwise kernels need it).  out:
 *   [0] family: 0 first-generation kernel, 1 wave-specialised kernel, 2 (1,7,7) stem kernel,
 *               3 16-byte-DMA pointwise kernel
 *   [1] id: wave-specialised 1 (1,3,3), 2 (3,1,1), 3 (7,1,1), 4 / 5 pointwise 128 x 128 / 64 x 64 tile,
 *           6 (3,1,1) in the F(2,3) domain, 7 (1,3,3) in the F(2x2,3x3) domain; pointwise-DMA 4 big / 5 small;
 *           stem 9; first generation 0
 *   [2] template PCH (64-element window chunks per channel; 0: the kernel has none)
 *   [3] template BJ (first generation only, else 0)
 *   [4] split count   [5] workspace slices per split (1, 2 or 4)
 *   [6] ct: input-channel (first generation: j) tiles   [7] mt: output-channel tiles
 *   [8..11] box log2 extents lTW, lTH, lTT, lTN   [12] ntiles (boxes)
 *   [13] workgroup order of the default rule: 1 tile-fastest, 0 split-fastest (COCLR_WGRAD_ORDER=split|tile
 *        overrides it per call; only families 1 and 3 have an order)
 *   [14] 1 if coclr_conv3d_wgrad_bn has a kernel for it (the rule of coclr_conv3d_wgrad_bn_ok)
 *   [15] 1 if id 7 re-cut its 32 x 2 boxes (34 x 4 windows) to 16 x 4 (18 x 6) */
int coclr_conv3d_wgrad_plan(const coclr_conv_desc* d, int operands_16B_aligned, int32_t out[16]);

/* dw[co][ci][tap] (+)= sum_{n,o} dy[n][co][o] * x[n][ci][o*s - p + tap]: the wgrad
 * half of aten::convolution_backward.  dw is addressed as
 * dw[co*w_co_stride + ci*w_ci_stride + tap_base + tap]. */
int coclr_conv3d_wgrad(const coclr_conv_desc* d, const float* x, const float* dy, float* dw,
                       float* workspace, int64_t w_co_stride, int64_t w_ci_stride, int tap_base,
                       int accumulate, void* stream);

/* The weight gradient of a convolution whose BatchNorm(+ReLU) backward apply pass has NOT run: `dz` is
 * d(activation) of the unit behind the convolution (backbone/s3dg.py:24-28: conv -> bn -> relu), `y` the
 * convolution's own output, coef[5][Cout] what coclr_bn_act_backward_coeffs left.  The kernel forms
 *   dy = A[co] * g + B[co] * y + D[co],   g = relu ? (y * scale[co] + shift[co] > 0 ? dz : 0) : dz
 * -- the expression of coclr_bn_act_backward's second pass, bit for bit -- between LDS and the matrix
 * pipe, so d(conv output) is never written or re-read.  For units whose data gradient nobody needs (the
 * (1,7,7) stem over the clip: 1 GB per pass at B = 32); coclr_conv3d_wgrad_bn_ok says whether the geometry
 * has such a kernel, COCLR_EINVAL otherwise.  Replaces the native_batch_norm_backward +
 * convolution_backward pair autograd runs for backbone/s3dg.py:145 (Conv_1a.conv1 / bn1). */
int coclr_conv3d_wgrad_bn_ok(const coclr_conv_desc* d, int* ok);
int coclr_conv3d_wgrad_bn(const coclr_conv_desc* d, const float* x, const float* dz, const float* y,
                          int64_t y_nstride, const float* coef, int relu, float* dw, float* workspace,
                          int64_t w_co_stride, int64_t w_ci_stride, int tap_base, int accumulate,
                          void* stream);

/* The same gradient delivered to up to four destinations: output-channel rows
 * [row_end[i-1], row_end[i]) go to dw_list[i] (row index local to the destination;
 * row_end[nseg-1] == d->Cout).  For convolutions that stand for several parameters at once --
 * the three 1x1x1 heads of an inception block run as one convolution over concatenated output
 * channels (backbone/s3dg.py:97-104,119-123) -- whose gradients live at unrelated addresses
 * (views of DistributedDataParallel's buckets, main_nce.py:172).  dw_list / row_end are HOST
 * arrays read during the call. */
int coclr_conv3d_wgrad_multi(const coclr_conv_desc* d, const float* x, const float* dy,
                             float* const* dw_list, const int32_t* row_end, int nseg,
                             float* workspace, int64_t w_co_stride, int64_t w_ci_stride,
                             int tap_base, int accumulate, void* stream);

/* ------------------------------------------------------------------------ */
/* BatchNorm3d + ReLU (+ residual)  (backbone/s3dg.py:16-17,26-27,46-48,     */
/*                                   60-64; backbone/resnet_2d3d.py:54-83)   */
/* ------------------------------------------------------------------------ */

/* Fold the conv partial sums (sum[c][ntiles], sumsq[c][ntiles]; two pointers so a channel
 * range of a concatenated convolution can be finalised on its own): batch mean / invstd,
 * fused scale = gamma*invstd and shift = beta - mean*scale; momentum update of
 * running_mean / running_var (unbiased) and num_batches_tracked += 1 (aten::batch_norm,
 * training=True). */
int coclr_bn_finalize(const float* sum, const float* sumsq, int C, int ntiles, double count,
                      const float* gamma, const float* beta, float* running_mean,
                      float* running_var, int64_t* num_batches_tracked, float momentum, float eps,
                      float* mean, float* invstd, float* scale, float* shift, void* stream);

/* coclr_bn_finalize followed by coclr_bn_act_apply (no residual) as ONE call: for layers whose
 * channels hold few values (N*S <= 32768: the 8x8x8 and 4x4x4 maps of S3D's last two stages) both
 * run in a single launch, one workgroup per channel; larger layers take the two launches. */
int coclr_bn_finalize_apply(const float* sum, const float* sumsq, int C, int ntiles, double count,
                            const float* gamma, const float* beta, float* running_mean,
                            float* running_var, int64_t* num_batches_tracked, float momentum,
                            float eps, float* mean, float* invstd, float* scale, float* shift,
                            const float* y, float* z, int N, int64_t S, int64_t y_nstride,
                            int64_t z_nstride, int relu, void* stream);

/* Eval-mode coefficients from the running statistics (main_coclr.py:363). */
int coclr_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean,
                         const float* running_var, float eps, int C, float* mean, float* invstd,
                         float* scale, float* shift, void* stream);

/* z = act(y*scale[c] + shift[c] (+ residual)); every tensor is [N][C][S] with its own
 * sample stride (channel slices of wider buffers). */
int coclr_bn_act_apply(const float* y, const float* scale, const float* shift,
                       const float* residual, float* z, int N, int C, int64_t S, int64_t y_nstride,
                       int64_t z_nstride, int64_t res_nstride, int relu, void* stream);

/* Backward of the above (aten::threshold_backward + native_batch_norm_backward):
 * dy, dgamma, dbeta and, for residual units, dres (+)= masked dz.
 * z may be NULL (ReLU mask is then recomputed from y).  sums_ws: fp64 partial sums, one
 * pair per (channel, sample) -- coclr_bn_backward_workspace doubles; no zero-fill needed,
 * no atomics (run-to-run deterministic). */
int coclr_bn_backward_workspace(int N, int C, int64_t* doubles);
/* The routes of one BatchNorm unit; launches nothing and needs no device (ABI 25).  Answered by the route struct
 * the launchers switch on.  Forward: coclr_bn_finalize_apply with y / z at y_nstride / z_nstride.  Backward:
 * coclr_bn_act_backward with dz, y, dy (and z / dres when has_z / has_dres) at their strides, or the
 * from-partials form of coclr_bn_act_backward_multi when has_partials.
 *  out[0] forward one workgroup per channel    out[1] forward 16-byte    out[2] forward non-temporal
 *  out[3], out[4] forward plane grid x, y (0 for the one-workgroup form)
 *  out[5] backward one workgroup per channel   out[6] backward 16-byte   out[7] backward non-temporal
 *  out[8] sample groups of the reduce pass (0: none)    out[9], out[10] backward plane grid x, y
 *  out[11] from partials */
int coclr_bn_plan(int N, int C, int64_t S, int64_t y_nstride, int64_t z_nstride, int64_t dz_nstride,
                  int64_t dy_nstride, int64_t dres_nstride, int has_z, int has_dres, int has_partials,
                  int32_t out[16]);
int coclr_bn_act_backward(const float* dz, const float* y, const float* z, const float* scale,
                          const float* shift, const float* mean, const float* invstd,
                          double* sums_ws, float* dy, float* dres, float* dgamma, float* dbeta,
                          int N, int C, int64_t S, int64_t dz_nstride, int64_t y_nstride,
                          int64_t dy_nstride, int64_t z_nstride, int64_t dres_nstride, int relu,
                          int training, int dres_accumulate, void* stream);

/* The first pass of the above plus the coefficients of its second, for a unit whose d(conv output) is
 * applied by its one reader (coclr_conv3d_wgrad_bn): coef[5][C] = A, B, D, scale, shift with
 * dy = A*g + B*y + D (training: A = scale, B = -scale*invstd*mean(g*xhat),
 * D = scale*(mean*invstd*mean(g*xhat) - mean(g)); frozen statistics: dy = scale*g); dgamma / dbeta as
 * above.  Two launches, no pass that writes dy. */
int coclr_bn_act_backward_coeffs(const float* dz, const float* y, const float* scale, const float* shift,
                                 const float* mean, const float* invstd, double* sums_ws, float* coef,
                                 float* dgamma, float* dbeta, int N, int C, int64_t S,
                                 int64_t dz_nstride, int64_t y_nstride, int relu, int training,
                                 void* stream);

/* ------------------------------------------------------------------------ */
/* Pooling (backbone/s3dg.py:105,151,162,173,190; resnet_2d3d.py:141;        */
/*          model/pretrain.py:51)                                            */
/* ------------------------------------------------------------------------ */

typedef struct coclr_pool_desc {
  int32_t N, C;
  int32_t Ti, Hi, Wi, To, Ho, Wo;
  int32_t kt, kh, kw, st, sh, sw, pt, ph, pw;
  int64_t x_nstride, y_nstride;
} coclr_pool_desc;

/* aten::max_pool3d_with_indices (floor mode, -inf padding, first max wins);
 * indices (optional, [N][C][To*Ho*Wo] int32) = flat offset inside the input plane.
 * in_scale / in_shift (optional, [C]): the input is read as x*in_scale[c] + in_shift[c], clamped at 0
 * when in_relu -- the BatchNorm3d + ReLU in front of the pool (backbone/s3dg.py:60-64 before
 * :151,:162) applied on the fly, so that the normalised activation is never written to HBM. */
int coclr_maxpool3d_fwd(const coclr_pool_desc* d, const float* x, float* y, int32_t* indices,
                        const float* in_scale, const float* in_shift, int in_relu, void* stream);
/* aten::max_pool3d_with_indices_backward, gather form (deterministic). */
int coclr_maxpool3d_bwd(const coclr_pool_desc* d, const float* dy, const int32_t* indices, float* dx,
                        int64_t dy_nstride, int64_t dx_nstride, int accumulate, void* stream);

/* Several BatchNorm units in one call: runs of up to four units that are small enough for the
 * one-workgroup-per-channel form (N*S <= 32768, the last two stages of S3D) and share a vector width run
 * as ONE launch whose grid is their channels back to back; everything else goes through the single-unit
 * entry points, in order.  Fields as the arguments of coclr_bn_finalize_apply / coclr_bn_act_backward
 * (no residual).  The three 1x1x1 heads of an inception block and the two separable branches side by
 * side (backbone/s3dg.py:97-118): 10 us launches of 16-384 workgroups each. */
typedef struct coclr_bn_fwd_call {
  const float* sum; const float* sumsq; const float* gamma; const float* beta;
  float* running_mean; float* running_var; int64_t* num_batches_tracked;
  float* mean; float* invstd; float* scale; float* shift;
  const float* y; float* z;
  double count;
  int64_t S, y_nstride, z_nstride;
  int32_t C, ntiles, N, relu;
  float momentum, eps;
} coclr_bn_fwd_call;
typedef struct coclr_bn_bwd_call {
  const float* dz; const float* y; const float* scale; const float* shift; const float* mean;
  const float* invstd;
  double* sums_ws; float* dy; float* dgamma; float* dbeta;
  int64_t S, dz_nstride, y_nstride, dy_nstride;
  int32_t N, C, relu, training;
  /* Backward sums already formed by the data gradient(s) that wrote dz (coclr_conv_call.bwd_y): up to two
   * [2][C][part_ntiles[i]] arrays (a strided convolution's data gradient is one launch per residue class).
   * part[0] != NULL: the reduction pass is replaced by a fold of these partials (fp64, fixed order). */
  const float* part[2];
  int32_t part_ntiles[2];
} coclr_bn_bwd_call;
int coclr_bn_finalize_apply_multi(const coclr_bn_fwd_call* calls, int n, void* stream);
int coclr_bn_act_backward_multi(const coclr_bn_bwd_call* calls, int n, void* stream);
/* The launches the two entry points above would make for these n units (exactly one of fwd / bwd given); launches
 * nothing and needs no device (ABI 25).  Answered by the run-cutting function the launchers themselves call: a run
 * is up to four consecutive units that take the one-workgroup route, share a vector width and (backward) carry no
 * partial sums; COCLR_PAIR=0 keeps every unit alone.  run_len[k] = units of launch k (>= 2: one fused launch, 1: the
 * unit goes alone), terminated by 0: n + 1 entries.  Reads only shapes, strides, part[0] and whether the operand
 * pointers are null (COCLR_EINVAL as the launch). */
int coclr_bn_multi_plan(const coclr_bn_fwd_call* fwd, const coclr_bn_bwd_call* bwd, int n, int32_t* run_len);

/* BatchNorm(+ReLU) backward of a unit whose only consumer is the max-pool described by `d` that
 * applied the unit's affine + ReLU while reading (coclr_maxpool3d_fwd with in_scale / in_shift): the
 * gradient of the normalised activation is the pool's dy at the arg-max positions and is never
 * written.  Replaces aten::max_pool3d_with_indices_backward + aten::native_batch_norm_backward +
 * threshold_backward (backbone/s3dg.py:151,162 behind :60-64).  y: the unit's convolution output
 * [N][C][Ti][Hi][Wi]; pool_dy / pool_idx: [N][C][To][Ho][Wo]; sums: workspace of
 * coclr_bn_backward_workspace(N, C) doubles.  Only for pools whose (time-folded) input plane fits the
 * kernel's LDS tile: coclr_bn_act_backward_pooled_fits answers that from the same tiling constants;
 * a pool that does not fit is rejected with COCLR_EINVAL (1) and the caller runs
 * coclr_maxpool3d_bwd + coclr_bn_act_backward instead. */
int coclr_bn_act_backward_pooled(const coclr_pool_desc* d, const float* pool_dy,
                                 const int32_t* pool_idx, const float* y, const float* scale,
                                 const float* shift, const float* mean, const float* invstd,
                                 double* sums, float* dy, float* dgamma, float* dbeta,
                                 int64_t pool_dy_nstride, int64_t y_nstride, int64_t dy_nstride,
                                 int relu, int training, void* stream);
int coclr_bn_act_backward_pooled_fits(const coclr_pool_desc* d, int* fits);

/* What coclr_maxpool3d_fwd, coclr_maxpool3d_bwd and coclr_bn_act_backward_pooled would launch for this descriptor
 * (x_nstride / y_nstride filled in as for the launch); launches nothing and needs no device (ABI 25).  Answered
 * by the plan structs the launchers themselves switch on.  with_indices: the forward writes arg-max indices.
 * dy_nstride / dx_nstride: sample strides of the backward's operands, 0: dense.  The pooled BatchNorm backward
 * is planned with y at x_nstride and its dy at dx_nstride.  The 16-byte flags (out[6], out[18], out[29]) are the
 * values the launchers pass to the kernels, which branch on nothing else.
 *  out[0]  forward family: 0 generic, 1 separable 3x3x3/1/1, 2 LDS-tiled
 *  out[1]  forward template: separable TT (0: run-time frame count); tiled row 0 (1,3,3)/(1,2,2) WPT 2,
 *          1 (3,3,3)/(1,1,1) WPT 4, 2 (3,3,3)/(2,2,2) WPT 2, 3 (2,2,2)/(2,2,2) WPT 2
 *  out[2]  volumes per workgroup (PG / G)    out[3], out[4] grid x, y    out[5] tfold
 *  out[6]  16-byte staging of x              out[7] dynamic LDS bytes
 *  out[8]  backward family: 0 generic gather, 1 3x3x3/1/1 gather, 2 colour-class tiled
 *  out[9..12] colour-class template PT, PH, PW, KQ (all 0: the generic form)
 *  out[13] G    out[14] outputs per thread and class for that G (kq)    out[15], out[16] grid x, y
 *  out[17] tfold    out[18] 16-byte staging of dy / indices (gather) or stores of dx (tiled)    out[19] LDS bytes
 *  out[20] pooled BatchNorm backward fits    out[21] G    out[22..25] template PT, PH, PW, KQ (0: generic form)
 *  out[26] kq    out[27] workgroups    out[28] tfold    out[29] 16-byte apply pass    out[30] LDS bytes
 *  out[31] non-temporal streaming (COCLR_BN_NT_MB)
 * COCLR_EINVAL for a null argument or a descriptor the forward refuses. */
int coclr_pool_plan(const coclr_pool_desc* d, int with_indices, int64_t dy_nstride, int64_t dx_nstride,
                    int32_t out[32]);
/* aten::adaptive_avg_pool3d(x, (1,1,1)) and its backward; planes = N*C. */
int coclr_global_avgpool_fwd(const float* x, float* y, int64_t planes, int64_t S, void* stream);
int coclr_global_avgpool_bwd(const float* dy, float* dx, int64_t planes, int64_t S, void* stream);

/* ------------------------------------------------------------------------ */
/* Contrastive head (model/pretrain.py)                                      */
/* ------------------------------------------------------------------------ */

/* C[m][n] (+)= act(alpha * sum_k A(m,k)*B(k,n) + bias[n]) on the fp32 MFMA;
 * A(m,k) = a[m*sam + k*sak], B(k,n) = b[k*sbk + n*sbn].  splits > 1 selects
 * split-K through `workspace` (coclr_gemm_workspace elements).  Used for the
 * projection-head 1x1x1 convs on pooled features (pretrain.py:52,54), their
 * backward, and the similarity products below. */
int coclr_gemm_workspace(int M, int N, int K, int splits, int64_t* elems);
int coclr_gemm(const float* a, int64_t sam, int64_t sak, const float* b, int64_t sbk, int64_t sbn,
               float* c, int64_t ldc, const float* bias, int M, int N, int K, float alpha, int relu,
               int accumulate, int splits, float* workspace, void* stream);

/* The products of an encoder's projection head and of its backward, each with the row-level operation
 * that FOLLOWS it in the reference applied by the kernel that folds the split-K partials
 * (pretrain.py:49-54: AdaptiveAvgPool3d -> Conv3d 1x1x1 -> ReLU -> Conv3d 1x1x1; :153-154 / :166-167
 * F.normalize; :175-182 the logits whose gradient arrives here).  Two launches per product instead of three
 * or four, same fold order as coclr_gemm (k = 0 .. splits-1: bit-identical to the unfused sequence):
 *   mode 0  none (with splits == 1: the plain product in one launch, optionally + rowsum)
 *   mode 1  aten::threshold_backward: c = a[m][n] > 0 ? v : 0            (nn.ReLU backward, pretrain.py:53)
 *   mode 2  F.normalize rows: c = v / max(||v||, f), out2[m] = 1 / max(||v||, f)              (N <= 512)
 *   mode 3  v += a[m*lda] * f * b[m][n]  (the l_pos term of pretrain.py:175, f = 1/T), then the backward of
 *           F.normalize: c = (v - y <y, v>) * inv_norm[m]                                      (N <= 512)
 *   mode 4  aten::adaptive_avg_pool3d backward: c is dense [M][N][S], c[m][n][:] = v / S
 * rowsum (splits == 1): rowsum[m] = sum_k A(m,k) -- the bias gradient of a weight-gradient product.
 * workspace: max(splits, 1) * M * N elements (always used unless mode 0 with splits == 1). */
typedef struct coclr_gemm_epilogue {
  int32_t mode;
  int32_t S;
  const float* a;
  int64_t lda;
  const float* b;
  const float* y;
  const float* inv_norm;
  float* out2;
  float f;
  float* rowsum;
} coclr_gemm_epilogue;
int coclr_gemm_fused(const float* a, int64_t sam, int64_t sak, const float* b, int64_t sbk, int64_t sbn,
                     float* c, int64_t ldc, const float* bias, int M, int N, int K, float alpha, int relu,
                     int splits, float* workspace, const coclr_gemm_epilogue* ep, void* stream);

/* F.normalize(x, dim=1) over rows of D (pretrain.py:154,167,380) and backward. */
int coclr_l2norm_fwd(const float* x, float* y, float* inv_norm, int rows, int D, float eps,
                     void* stream);
int coclr_l2norm_bwd(const float* dy, const float* y, const float* inv_norm, float* dx, int rows,
                     int D, void* stream);

/* logits[B][1+K] = [ <q_b,k_b> | q . queue ] / T  (pretrain.py:175-182: two einsums,
 * queue.clone(), cat and the in-place divide in one pass). queue is [D][K]. */
int coclr_nce_logits_fwd(const float* q, const float* k, const float* queue, float* logits, int B,
                         int D, int K, float T, void* stream);
/* dq = (dlogits[:,1:] . queue^T + dlogits[:,0] * k) / T ; workspace as coclr_gemm(B, D, K, splits). */
int coclr_nce_logits_bwd(const float* dlogits, const float* k, const float* queue, float* dq,
                         float* workspace, int B, int D, int K, float T, int splits, void* stream);

/* p_k = p_k*m + p_q*(1-m) over many tensors in one launch (pretrain.py:76-80).
 * table: int64[3*nchunks] on device = {dst ptr, src ptr, count<=65536} per chunk. */
int coclr_momentum_update(const int64_t* table, int nchunks, float m, float one_minus_m,
                          void* stream);

/* queue[:, ptr:ptr+BW] = keys^T with ptr read on device (pretrain.py:89-93 without the
 * int(queue_ptr) host sync); int64 side queues (pretrain.py:217,337-338); ptr=(ptr+BW)%K. */
int coclr_queue_enqueue(float* queue, const float* keys, int D, int K, int BW, const int64_t* ptr,
                        void* stream);
int coclr_queue_fill_i64(int64_t* queue, const int64_t* vals, int64_t const_val, int K, int BW,
                         const int64_t* ptr, void* stream);
int coclr_queue_advance(int64_t* ptr, int BW, int K, void* stream);

/* mask[B][1+K] (bytes): col 0 = 1; col 1+j = (src[b]==names[j]) or j among the topk
 * largest sim[b][:] after same-source columns are set to -inf
 * (pretrain.py:397-413; with topk=0 also UberNCE's label mask, pretrain.py:267-269). */
int coclr_positive_mask(const float* sim, const int64_t* src, const int64_t* names, uint8_t* mask,
                        int B, int K, int topk, void* stream);

/* The same mask with the similarity product folded in and no (B, K) similarity tensor
 * (pretrain.py:405-410: `sim = kf.matmul(queue_second)`, siblings to -inf, topk, scatter): ONE launch,
 * sim tiles on the MFMA pipe, a running top-k per row across tiles.  kf [B][D] unit rows, queue_second
 * [D][K]; D must be 128, topk <= 16.  Workspaces: cand_val / cand_idx [B][ceil(K/64)][topk];
 * counters [ceil(B/32)] int32, ZERO before the first call (every call leaves them zero again).
 * sim_out (optional, [B][K]) receives the similarities, for tests. */
int coclr_mine_positives(const float* kf, const float* queue_second, const int64_t* src,
                         const int64_t* names, uint8_t* mask, float* cand_val, int32_t* cand_idx,
                         int32_t* counters, float* sim_out, int B, int D, int K, int topk,
                         void* stream);

/* out[i][:] = in[idx[i]][:] (pretrain.py:124,143); rows of `row_elems` floats, source rows
 * `in_row_stride` floats apart (>= row_elems: the second clip of a (B,2,...) pair is a
 * strided view). */
int coclr_gather_rows(const float* in, const int64_t* idx, float* out, int rows, int64_t row_elems,
                      int64_t in_row_stride, void* stream);

/* out[i][:] = the `row_elems` floats at device address row_ptrs[i] (int64[rows] on the device): the
 * shuffle-BN exchange of pretrain.py:98-124 as a ROW PULL -- each rank reads the B key clips it will
 * encode straight out of its peers' staging buffers (hipIpc-mapped, over xGMI) instead of all-gathering
 * B*world clips; local rows are ordinary addresses. */
int coclr_pull_rows(const int64_t* row_ptrs, float* out, int rows, int64_t row_elems, void* stream);

/* nn.ReLU of the projection head (pretrain.py:53) and small helpers. */
int coclr_relu_fwd(const float* x, float* y, int64_t n, void* stream);
int coclr_relu_bwd(const float* dy, const float* y, float* dx, int64_t n, void* stream);
int coclr_colsum(const float* x, float* out, int rows, int cols, void* stream);

/* S3D-G self gating (backbone/s3dg.py:68-78): out = x * sigmoid(fc(mean_{T,H,W} x)).
 * The mean is coclr_global_avgpool_fwd, fc is coclr_gemm; these supply the rest:
 * w = sigmoid(s) and ds = dw*w*(1-w); out[n][c][:] (+)= a[n][c][:]*gain[n*C+c] + bias[n*C+c]
 * (forward scaling, and dx = dout*w + (ds.W)/S in the backward); out[n*C+c] = <a, b> per
 * (n, c) plane (dw of the backward). */
int coclr_sigmoid_fwd(const float* s, float* w, int64_t n, void* stream);
int coclr_sigmoid_bwd(const float* dw, const float* w, float* ds, int64_t n, void* stream);
int coclr_plane_scale(const float* a, const float* gain, const float* bias, float* out, int N, int C,
                      int64_t S, int64_t a_nstride, int64_t out_nstride, int accumulate,
                      void* stream);
int coclr_plane_dot(const float* a, const float* b, float* out, int N, int C, int64_t S,
                    int64_t a_nstride, int64_t b_nstride, void* stream);

/* ------------------------------------------------------------------------ */
/* Training-loop neighbours of the model: optimiser step,     */
/* loss + accuracy epilogue, input staging                                   */
/* ------------------------------------------------------------------------ */

/* torch.optim.Adam.step() over the launch scripts' one-group-per-tensor parameter list
 * (main_nce.py:190-200,331; main_coclr.py:213,406) as ONE launch, operation-for-operation the
 * arithmetic of torch.optim.Adam (amsgrad=False, maximize=False, L2 weight decay).
 *   table  int64[nchunks][8] on device: {param, grad, exp_avg, exp_avg_sq, key_param or 0,
 *          count (<= 65536 elements of the tensor), group index, 0}
 *   hyper  double[.][8] on device, one row per group: {lr, beta1, beta2, eps, weight_decay, 0,0,0}
 *          (doubles: torch forms 1-beta and beta**t from Python floats)
 *   steps  float[.] on device, one per group: number of steps taken so far; read as t = steps+1
 *          for the bias corrections, then incremented for the `ngroups` groups listed in `groups`
 * key_param != 0 folds the momentum-encoder update of model/pretrain.py:76-80 into the pass:
 *   key = key*mom_m + param_new*mom_1m  (exactly what the next forward would compute). */
int coclr_adam_step(const int64_t* table, int nchunks, const double* hyper, float* steps,
                    const int32_t* groups, int ngroups, float mom_m, float mom_1m, void* stream);

/* torch.optim.SGD.step() over a one-group-per-tensor parameter list as ONE launch: the classifier
 * fine-tuning loop's optimizer (eval/main_classifier.py:159, `optim.SGD(params, lr, weight_decay,
 * momentum=0.9)`; eval/feature_linear_probe.py:121 constructs the same class), operation for operation
 * torch.optim.SGD's foreach arithmetic (momentum, dampening, nesterov, weight_decay, maximize).
 *   table  int64[nchunks][8] on device: {param, grad, momentum_buffer or 0 (momentum == 0), count
 *          (<= 32768 elements of the tensor), slot, first, 0, 0}; first != 0: the parameter's first
 *          step with momentum (torch's momentum_buffer is None): buffer = d_p, not read
 *   hyper  double[.][8] on device, one row per slot: {lr, momentum, dampening, weight_decay,
 *          nesterov (0/1), maximize (0/1), 0, 0} (doubles: torch forms 1-dampening from Python floats)
 * No step counter: nothing is written but the parameters and their momentum buffers. */
int coclr_sgd_step(const int64_t* table, int nchunks, const double* hyper, void* stream);

/* Loss + accuracy over logits[B][N1] in one pass, results as device scalars:
 *   mode 0  nn.CrossEntropyLoss(logits, target)                         (main_nce.py:315)
 *   mode 1  multi_nce_loss: -log(sum_j softmax_j*mask_j)                (main_coclr.py:343-346);
 *           drop_self: column 0 is left out of a row's positives when the row has others
 *           (the mask_clone[mask_sum!=1, 0] = 0 branch, main_coclr.py:384-389)
 *   mode 2  -(sum_j log_softmax_j*mask_j) / sum_j mask_j                (main_nce.py:322)
 * scalars[5] = batch means of {loss, hit@k1, hit@k2, self-hit@k1, self-hit@k2}: hit@k = one of the
 * row's positives is among its k largest logits (calc_topk_accuracy / calc_mask_accuracy,
 * utils/utils.py:52-85), self-hit@k the same for column 0 alone (main_coclr.py:392).
 * rowstats float[B][8] and flags uint8[B] carry what the backward needs.  mask: bytes, [B][N1]. */
int coclr_nce_loss_fwd(const float* logits, const uint8_t* mask, const int64_t* target,
                       float* rowstats, uint8_t* flags, float* scalars, int B, int N1, int mode,
                       int drop_self, int k1, int k2, void* stream);
/* dlogits = dloss[0]/B * (softmax - positives' weights); dloss is a DEVICE scalar. */
int coclr_nce_loss_bwd(const float* logits, const uint8_t* mask, const int64_t* target,
                       const float* rowstats, const uint8_t* flags, const float* dloss,
                       float* dlogits, int B, int N1, int mode, void* stream);

/* Loader frames -> model input in one pass (main_nce.py:207-209,299-302; utils/transforms.py:57-63;
 * model/pretrain.py:149-150): frames[B][C][S][THW] (uint8 when from_u8, else fp32 in [0,1]) ->
 * out[B][S][C][THW] fp32 = ((x / 255 if uint8) - mean[c]) / std[c].  THW = seq_len*H*W; mean / std
 * are HOST arrays of C floats read at call time. */
int coclr_stage_clips(const void* frames, int from_u8, float* out, int B, int C, int S, int64_t THW,
                      const float* mean, const float* std, void* stream);

/* Five/ten-crop test clips of ONE video from its raw frames in one launch (eval/main_classifier.py:453-469;
 * utils/augmentation.py:21-43,61-88,149-177,347-350): for every crop k = {x0, y0, flip} and slot (clip, t),
 *   flip the frame (flip = 1) -> crop the cw x ch box at (x0, y0) OF THE FLIPPED FRAME -> PIL's
 *   Image.resize((S, S), BICUBIC) on 8-bit pixels -> / 255 -> (x - mean[c]) / std[c]
 * into out[n_crops][n_clips][3][T][S][S] fp32, bit-identical to that chain.  The random test-time ColorJitter
 * of the reference is not part of it: coclr_resize_crops_u8 + coclr_color_jitter_clips below are.
 * frames: uint8 [F][H][W][3] (interleaved RGB), device.  slot_frame: int32 [n_clips*T], device: the frame of
 * every (clip, t); frames may repeat.  crops: HOST int32 [n_crops][3], read at call time.  The resampling
 * tables (device, int32) are PIL's precomputed coefficients per axis, in its 22-bit fixed point:
 * xmin[Sp], xk[xtaps][Sp] with Sp = S rounded up to a multiple of 4 (tap-major; rows shorter than xtaps and
 * the columns past S are zero); the same for y.  A flipped crop uses the same tables on mirrored columns.
 * COCLR_EINVAL before any launch: a null pointer; F, H, W, T, n_clips, S, cw, ch < 1; S > 512; n_crops
 * outside 1..16; taps outside 1..64; a box that leaves the frame; flip not 0/1; std == 0; n_clips*T > 65535
 * or a grid over the launch limits; an output row whose ytaps source rows (3*Sp bytes each) exceed 64 KiB.
 * Frame indices outside [0, F) are the CALLER's to refuse (they live on the device). */
int coclr_stage_crops(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame, int n_clips,
                      int T, const int32_t* crops, int n_crops, int cw, int ch, int S, const int32_t* xmin,
                      const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                      const float* mean, const float* std, float* out, void* stream);

/* The resize of coclr_stage_crops alone: same arguments without mean / std, same flip, box, tables, integer
 * passes and clamps, but the resized BYTES go out as uint8 out[n_crops][n_clips*T][S][S][3] (one image per slot,
 * interleaved RGB like `frames`) -- the input of coclr_color_jitter_clips.  Same refusals. */
int coclr_resize_crops_u8(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame, int n_clips,
                          int T, const int32_t* crops, int n_crops, int cw, int ch, int S, const int32_t* xmin,
                          const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                          uint8_t* out, void* stream);

/* The reference's ColorJitter / RandomGray (utils/augmentation.py:179-320, i.e. torchvision 0.5's functional on
 * PIL images) on uint8 frames, then / 255 and (x - mean[c]) / std[c], in one launch: frames uint8 [N][H][W][3]
 * (device) -> out fp32 [N/T][3][T][H][W], frame n at clip n / T, position n % T.  Frame n runs program
 * n / group_size of kinds int32 [G][P] and params fp32 [G][P] (DEVICE tables, P <= 8), its ops in order on the
 * frame's RGB bytes, bit-identical to PIL:
 *   0 nothing (padding)
 *   1 brightness  ImageEnhance.Brightness(img).enhance(param)
 *   2 contrast    ImageEnhance.Contrast(img).enhance(param); the mean of L is that of THIS frame at this point
 *   3 saturation  ImageEnhance.Color(img).enhance(param)
 *   4 hue         convert('HSV'), h = (h + param) & 255, convert('RGB'); param an integer 0..255
 *   5 gray        all three channels = channel param (0..2) (RandomGray.grayscale)
 * An all-zero program gives coclr_stage_clips' arithmetic on the bytes.  kinds_host / params_host are the SAME
 * tables on the HOST, read at call time: the entry point validates them, the kernel reads the device copies
 * (and stays in bounds whatever those hold).  mean / std: HOST arrays of 3 floats.
 * COCLR_EINVAL before any launch: a null pointer; N, H, W, T, G, group_size < 1; P outside 1..8; N % T != 0;
 * G * group_size < N; H * W > 224 * 224 (one workgroup holds the frame in LDS); std == 0; a kind outside 0..5;
 * a non-finite factor; a hue shift that is no integer in 0..255; a gray channel outside 0..2. */
int coclr_color_jitter_clips(const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                             const float* params, const int32_t* kinds_host, const float* params_host, int G,
                             int P, int group_size, const float* mean, const float* std, float* out,
                             void* stream);

/* The training transform's ops on uint8 frames (main_nce.py:366-392; utils/augmentation.py:149-216,357-369): a
 * superset of coclr_color_jitter_clips -- same arguments, same layouts, same validated host copies, kinds 0..5 as
 * there -- with the two ops the pretraining chain adds:
 *   6 blur  img.filter(ImageFilter.GaussianBlur(sigma)) on 8-bit pixels, bit-identical to PIL: three box blurs
 *           along x, three along y, rounded to bytes after each.  param = r_f, PIL's fp32 box radius for sigma
 *           (computed on the host in PIL's own float arithmetic: staging.blur_box_radius), 0 <= r_f <= 16; r_f = 0 is the identity.
 *   7 flip  transpose(FLIP_LEFT_RIGHT); param unused.
 * COCLR_EINVAL as coclr_color_jitter_clips, with kinds 0..7 admitted, and for a blur radius outside [0, 16] or NaN.
 * Additive: coclr_color_jitter_clips keeps refusing kinds 6 and 7, and the ABI number stays 24 -- no existing
 * signature or behaviour changed. */
int coclr_augment_clips(const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                        const float* params, const int32_t* kinds_host, const float* params_host, int G, int P,
                        int group_size, const float* mean, const float* std, float* out, void* stream);

/* RandomSizedCrop's boxes of a whole batch in one launch (utils/augmentation.py:90-138): for output clip k and
 * t < T, crop the w x h box at (x0, y0) of frame first + t and Image.resize((S, S), BICUBIC) it on 8-bit pixels,
 * as coclr_resize_crops_u8 does for one box size, into uint8 out[n_clips*T][S][S][3] -- the input of
 * coclr_augment_clips.  No flip (the reference flips after the resize: kind 7 above).
 * frames: uint8 [F][H][W][3], device.  desc: int32 [n_clips][10], DEVICE:
 *   {first frame, frames (= T), x0, y0, w, h, x-table offset, y-table offset, xtaps, ytaps};
 * desc_host: the same on the HOST, read at call time and validated (the kernel reads the device copy and stays in
 * bounds whatever that holds).  xtab / ytab: int32 device buffers of xlen / ylen elements, 16-byte aligned, the
 * per-box tables of each axis one after the other: at a box's offset (a multiple of 4) min[Sp] then k[taps][Sp],
 * laid out as coclr_stage_crops takes them (Sp = S rounded up to a multiple of 4).  Boxes may share tables.
 * COCLR_EINVAL before any launch: a null or misaligned pointer; F, H, W, T, n_clips, S < 1; S > 512; a descriptor
 * whose frames != T, whose frames leave [0, F), whose box leaves the frame, whose taps are outside 1..64 or whose
 * tables leave their buffer; n_clips*T > 65535 or a grid over the launch limits; an output row of the tallest
 * box whose source rows (3*Sp bytes each) exceed 64 KiB. */
int coclr_resize_boxes_u8(const uint8_t* frames, int F, int H, int W, const int32_t* desc,
                          const int32_t* desc_host, int n_clips, int T, int S, const int32_t* xtab, int64_t xlen,
                          const int32_t* ytab, int64_t ylen, uint8_t* out, void* stream);

/* The crop chain of the classifier's fine-tuning / linear-probe loop in one launch (eval/main_classifier.py:729-744:
 * A.RandomSizedCrop(size=224, consistent=True, bottom_area=0.2) then A.Scale(args.img_dim); utils/augmentation.py:
 * 21-58 Scale and CenterCrop, 90-146 RandomSizedCrop with its ten attempts and its Scale + CenterCrop fallback): per
 * output clip k and t < T, resample the w x h region at (x0, y0) of frame first + t to (ow, oh) with
 * Image.resize(BICUBIC) on 8-bit pixels, keep the size x size window at (cx, cy) of that, and Image.resize it to
 * S x S -- four 8-bit passes, each rounded and clamped on its own, the size x size image in LDS only.
 * A drawn box is ow = oh = size, cx = cy = 0; the fallback is the whole frame with Scale's (ow, oh) and
 * CenterCrop's window.
 * desc: int32 [n_clips][14], DEVICE: {first frame, frames (= T), x0, y0, w, h, ow, oh, cx, cy, x-table offset,
 *   y-table offset, xtaps, ytaps}; desc_host: the same on the HOST, read at call time and validated (the kernel
 *   reads the device copy and stays in bounds whatever that holds).
 * xtab / ytab: int32 device buffers of xlen / ylen elements, 16-byte aligned, the clips' stage-1 tables one after
 *   the other: at a clip's offset (a multiple of 4) min[P] then k[taps][P], P = size rounded up to a multiple of 4,
 *   holding columns cx .. cx+size-1 of the w -> ow tables (rows cy .. of the h -> oh tables).  Clips may share.
 * tab2: int32 device buffer of len2 elements, 16-byte aligned: min[Sp] then k[taps2][Sp] of size -> S, used on
 *   both axes of every clip (Sp = S rounded up to a multiple of 4).  size == S makes it PIL's identity.
 * Exactly one output: out8 uint8 [n_clips*T][S][S][3] (the input of coclr_augment_clips), or out fp32
 *   [n_clips][3][T][S][S] = (byte / 255 - mean[c]) / std[c] with mean / std host arrays of 3, as coclr_stage_crops.
 * COCLR_EINVAL before any launch: a null or misaligned pointer, both or neither output, out without mean / std or
 * with a zero std; F, H, W, T, n_clips, S, size < 1; S or size > 224; a descriptor whose frames != T, whose
 * frames leave [0, F), whose region leaves the frame, whose window leaves (ow, oh), whose taps are outside 1..64 or
 * whose tables leave their buffer; taps2 outside 1..64 or len2 < Sp (1 + taps2); n_clips*T > 65535; one output
 * row whose halo of intermediate and source rows exceeds the CU's LDS.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_resize2_boxes(const uint8_t* frames, int F, int H, int W, const int32_t* desc, const int32_t* desc_host,
                        int n_clips, int T, int size, int S, const int32_t* xtab, int64_t xlen, const int32_t* ytab,
                        int64_t ylen, const int32_t* tab2, int64_t len2, int taps2, const float* mean,
                        const float* std, uint8_t* out8, float* out, void* stream);

/* Baseline JPEG frames -> the uint8 [F][H][W][3] frames the staging entry points above take, bit-identical to
 * Image.open(BytesIO(raw)).convert('RGB') with libjpeg-turbo (dataset/lmdb_dataset.py:37-38): Huffman decoding,
 * libjpeg's "islow" inverse DCT, "fancy" chroma upsampling, 16-bit fixed-point YCbCr -> RGB.  All frames of a call
 * share (H, W), the component count (1, or 3 = YCbCr) and the luma sampling hs x vs in {1x1, 2x1, 2x2} (chroma 1x1;
 * one component: 1x1); tables, restart interval and byte counts are per frame.  The headers are parsed on the host
 * (coclr_amd/jpeg.py: parse / pack), which refuses every other kind of file.
 * Workspace, answered without a device: bytes PER FRAME of `coefs` (int16, 64 per 8x8 block) and `planes` (uint8). */
int coclr_jpeg_workspace(int H, int W, int ncomp, int hs, int vs, int64_t* coef_bytes, int64_t* plane_bytes);
/* data: the frames' entropy-coded bytes one after the other, data_len of them (< 2^31), device.
 * meta: int32 [F][width], DEVICE, one descriptor per frame (word offsets as in csrc/jpeg_core.h):
 *   0 offset of the frame's bytes in data, 1 their count, 2 restart interval in MCUs (0 = none), 3 restart segments,
 *   16 [3][64] quantisers per component, natural order; 208 six Huffman tables of 96 words (DC of component 0..2,
 *   AC of component 0..2: limit[16], valoff[16], 256 values in 64 words); 784 [segments] first byte of every restart
 *   segment relative to word 0.  width >= 784 + the most segments of any frame.
 * meta_host: the same on the HOST, read at call time and validated; the kernels read the device copy and stay in
 *   bounds -- reads inside data, stores inside the frame's own storage, loops bounded by the block count -- whatever
 *   the device copy and the bytes hold.  Past the end of its bytes a frame reads zero bits, as libjpeg pads.
 * stages: bit mask of what to launch, in order: 1 entropy (zero-fills coefs and status, then one lane per (frame,
 *   restart segment): here a frame without restart markers is one lane; coclr_jpeg_decode_split below gives it a
 *   workgroup), 2 inverse DCT (one lane per block, coefs -> planes), 4 upsampling + colour + crop (planes -> out).
 *   7 decodes; the parts exist to be timed.
 * coefs / planes: F times the workspace sizes, 16-byte aligned.  out: uint8 [F][H][W][3].
 * status: int32 [F], 0 = clean; bit 0 a bit pattern that is no Huffman code (decoded as 0), bit 1 a zero run past
 *   the 64th coefficient.
 * COCLR_EINVAL before any launch: a null or misaligned pointer; F < 1; H or W outside 1..8192; another component
 * count or sampling; stages outside 1..7; data_len outside 0..2^31-1; a descriptor whose bytes leave data, whose
 * segment count is not ceil(MCUs / interval) or exceeds width - 784, whose segment offsets decrease or leave its
 * bytes, whose quantisers leave 0..255 or whose code limits decrease or leave 0..65536.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_jpeg_decode(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host, int F,
                      int width, int H, int W, int ncomp, int hs, int vs, int stages, int16_t* coefs,
                      uint8_t* planes, uint8_t* out, int32_t* status, void* stream);
/* coclr_jpeg_decode with intra-frame parallel Huffman decoding for the frames of ONE restart segment (no restart
 * markers: what ffmpeg, cv2.imwrite and PIL write by default).  chunk_bytes == 0 is exactly coclr_jpeg_decode.
 * 8 <= chunk_bytes <= 65536: such a frame is one workgroup, one lane per chunk of chunk_bytes raw bytes (up to 1024
 * lanes, sized by the call's longest frame; longer frames take several windows of chunks in order).  Every chunk is
 * decoded from a guessed state, each chunk's exit state becomes the next chunk's entry, and chunks whose entry
 * changed are decoded again until nothing changes: chunk 0 starts from the true state, so this reaches the serial
 * decoder's states for ANY bytes in at most as many rounds as there are chunks, and coefs, out and status are
 * bit for bit those of coclr_jpeg_decode.  Frames WITH restart markers keep the lane per segment of
 * coclr_jpeg_decode in the same call.  No workspace beyond coclr_jpeg_decode's; the same bounds hold.
 * COCLR_EINVAL before any launch: everything coclr_jpeg_decode refuses; chunk_bytes other than 0 or 8..65536.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_jpeg_decode_split(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host,
                            int F, int width, int H, int W, int ncomp, int hs, int vs, int stages, int16_t* coefs,
                            uint8_t* planes, uint8_t* out, int32_t* status, int chunk_bytes, void* stream);

/* coclr_jpeg_decode_split for a batch whose frames DIFFER in geometry (a loader batch of videos that keep their own
 * aspect ratio: kinetics400-256): the same stages, still one launch each for the whole batch, with (H, W, components,
 * hs, vs), the place of the coefficients and the place of the output per frame.
 * data, meta, meta_host, width, stages, status, chunk_bytes: as coclr_jpeg_decode_split; every descriptor is held
 *   against its OWN frame's geometry.
 * geom: int64 [F][8], DEVICE: {H, W, components, hs, vs, first coefficient block, first output byte, 0} (csrc/
 *   jpeg_core.h: JR_*); geom_host: the same on the HOST, read at call time and validated.
 * prefix: int64 [2][F + 1], DEVICE, and prefix_host: the blocks, then the row groups (H * ceil(W / 16)) of all frames
 *   before each one, [0] = 0 and [F] the total.  A lane of the inverse DCT (one per block) and of the colour stage (one
 *   per 16 pixels of a row) finds its frame by binary search in it.
 * coefs / planes: workspaces of coef_blocks blocks (128 / 64 bytes each), 16-byte aligned; frame f uses blocks
 *   [first block, first block + its block count) of both.  out: out_bytes bytes, 16-byte aligned; frame f is
 *   uint8 [H][W][3] at its first output byte.  Bytes between frames are not written.
 * The kernels read the device copies and stay in bounds whatever those hold: a frame whose geometry is not one of the
 * above, or whose blocks or bytes leave coef_blocks / out_bytes, is skipped, and a lane outside its frame's own count
 * does nothing.
 * COCLR_EINVAL before any launch: everything coclr_jpeg_decode_split refuses, per frame against its own geometry; a
 * frame whose first block or first byte is below the end of the frame before it (overlapping or decreasing) or whose
 * range leaves its buffer; a first output byte that is not a multiple of 16; prefix arrays that do not start at 0 or
 * whose steps are not the frames' block and row-group counts.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_jpeg_decode_ragged(const uint8_t* data, int64_t data_len, const int32_t* meta, const int32_t* meta_host,
                             int F, int width, const int64_t* geom, const int64_t* geom_host, const int64_t* prefix,
                             const int64_t* prefix_host, int stages, int16_t* coefs, uint8_t* planes,
                             int64_t coef_blocks, uint8_t* out, int64_t out_bytes, int32_t* status, int chunk_bytes,
                             void* stream);

/* A dataset's compressed frames kept on the device, parsed and validated once, and decoded by frame index
 * (coclr_amd/jpeg.py: class Store).  What a frame's Huffman decoder needs to start in the middle of its bytes is a
 * property of the file, so it is found once (coclr_jpeg_store_index) and every later decode of a restart-less frame
 * is ONE pass, a lane per chunk, with no rounds (coclr_jpeg_decode_store).
 * data: every frame's entropy-coded bytes, data_bytes of them, DEVICE; data_bytes may exceed 2^31, one frame's count
 *   may not.
 * frames: int64 [nframes][8], DEVICE, and frames_host, the same on the HOST (csrc/jpeg_core.h: JS_*): {first byte
 *   (64 bits), byte count, restart interval, restart segments, table set, first word in segs, first row in rows,
 *   H | W << 16 | components << 32 | hs << 36 | vs << 40}.
 * tables: int32 [16 + table_sets * 768], DEVICE, and tables_host: set i holds words 16 .. 783 of coclr_jpeg_decode's
 *   descriptor (quantisers, Huffman tables) at word 16 + i * 768, once per distinct set.
 * segs: int32 [nsegs], DEVICE, and segs_host: for every frame of more than one restart segment the first byte of each,
 *   relative to the frame's first byte.  May be null when nsegs is 0.
 * rows: uint32 [nrows][4], DEVICE: for every frame of ONE restart segment a row per chunk of chunk_bytes raw bytes
 *   (at least one), the serial decoder at the first symbol that starts in the chunk (csrc/jpeg_core.h: jc_row_pack):
 *   bit, block of the MCU and zigzag index (14 bits), position relative to the chunk (17), "only zero bits are left"
 *   (1); the frame's blocks completed before it (32); the three DC predictors (3 x 16).  16 bytes per chunk_bytes
 *   compressed bytes.
 * chunk_bytes: 8..65536, fixed for the life of the store. */
typedef struct {
  const uint8_t* data;
  int64_t data_bytes;
  const int64_t* frames;
  const int64_t* frames_host;
  int64_t nframes;
  const int32_t* tables;
  const int32_t* tables_host;
  int64_t table_sets;
  const int32_t* segs;
  const int32_t* segs_host;
  int64_t nsegs;
  uint32_t* rows;
  int64_t nrows;
  int32_t chunk_bytes;
} coclr_jpeg_store;

/* Writes the rows of the restart-less frames among frames [f0, f1) of `st`, whose bytes, records, tables and segment
 * words are in place: one workgroup per frame runs the scan rounds of coclr_jpeg_decode_split to their fixed point
 * (in windows of up to 1024 chunks) and stores per chunk the entry state, block count and predictors that its write
 * pass would start from.  No coefficients are written.  Frames with restart markers get no rows: their segment
 * offsets are their index.  The kernel reads the device copies and stays inside data, tables and rows whatever they
 * hold.
 * COCLR_EINVAL before any launch: a null pointer; chunk_bytes outside 8..65536; f0 < 0, f1 <= f0 or f1 > nframes; a
 * frame of [f0, f1) whose bytes leave data or number 2^31 or more, whose geometry is not one coclr_jpeg_decode takes,
 * whose table set does not exist or holds what coclr_jpeg_decode refuses, whose segment count is not ceil(MCUs /
 * interval), whose segment words leave segs, decrease or leave its bytes, or whose rows leave `rows`.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_jpeg_store_index(const coclr_jpeg_store* st, int64_t f0, int64_t f1, void* stream);

/* coclr_jpeg_decode_ragged for F frames of a store named by a selection: frame i of the call is store frame sel[i];
 * repeats are allowed.  Bytes, tables, segment words and rows are reached through the selection, bytes with 64-bit
 * addresses.
 * sel: int64 [F], DEVICE, and sel_host.
 * geom, geom_host, coefs, planes, coef_blocks, out, out_bytes, stages, status: as coclr_jpeg_decode_ragged.
 * prefix: int64 [3][F + 1], DEVICE, and prefix_host: blocks and row groups as there, then the entropy lanes of all
 *   frames before each one: a frame of one restart segment has a lane per chunk, any other a lane per segment.
 * Entropy stage: one launch, one pass.  A lane finds its frame by binary search in the third prefix; a chunk's lane
 * loads its row and decodes the chunk from it (jc_chunk_write), a segment's lane decodes its segment.  Status bits of
 * a frame's lanes are OR-ed.  A row is the serial decoder's state for those bytes, so coefs, out and status are bit
 * for bit those of coclr_jpeg_decode on the same bytes, whatever chunk_bytes the store was built with.
 * The kernels stay in bounds whatever the device copies hold, rows included: a selection outside the store names
 * frame 0, a record is clamped to the buffers, and a row of any words decodes to garbage inside the frame's own
 * coefficient blocks (the guarantee jc_chunk_write gives for guessed states).
 * COCLR_EINVAL before any launch: what coclr_jpeg_decode_ragged refuses of geom, prefix, the workspaces and out; a
 * selection outside [0, nframes); a selected frame whose recorded geometry is not its row of geom, whose bytes leave
 * data, whose rows or segment words leave their arrays, or whose third prefix step is not its lane count.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_jpeg_decode_store(const coclr_jpeg_store* st, const int64_t* sel, const int64_t* sel_host, int F,
                            const int64_t* geom, const int64_t* geom_host, const int64_t* prefix,
                            const int64_t* prefix_host, int stages, int16_t* coefs, uint8_t* planes,
                            int64_t coef_blocks, uint8_t* out, int64_t out_bytes, int32_t* status, void* stream);

/* coclr_jpeg_decode_store for ONE pixel box of every selected frame (what nvJPEG calls a ROI decode): the training
 * transform crops before it resizes, so no pixel outside a clip's RandomSizedCrop box reaches the model.
 * window: int64 [F][4], DEVICE, and window_host: {x0, y0, w, h} of frame i's box inside the frame (csrc/jpeg_core.h:
 *   JW_*).
 * out: frame i is its box alone, h x w x 3 bytes at geom[i][6], rows w * 3 bytes apart; offsets in frame order,
 *   16-byte aligned, the frames neither overlapping nor leaving out_bytes.
 * prefix: int64 [3][F + 1] as coclr_jpeg_decode_store, with the first two rows counted for the window: the blocks of the
 *   box's MCU rectangle, and the box's row groups h * ceil(w / 16).  The third row is unchanged: every chunk and
 *   segment keeps its lane, and a lane that has nothing to do returns.
 * coefs, planes, coef_blocks, geom[i][5]: the FULL-frame layout of coclr_jpeg_decode_store, so every block and sample
 *   lies where a whole decode puts it and the arithmetic is the same at the same addresses, on fewer lanes.  The entry
 *   derives the MCU rectangle [mx0, mx1) x [my0, my1) itself, from the box and the store's host record: the MCUs of
 *   the box's luma samples and of the chroma samples the fancy upsampling reads for them (on an axis subsampled by 2,
 *   columns or rows (p >> 1) - 1 .. (p >> 1) + 1 clamped to the plane's real size).  With first = my0 * mcux + mx0 and
 *   last = (my1 - 1) * mcux + mx1:
 *   entropy   a chunk's lane reads its row and the next row's block count and returns when the blocks it touches lie
 *             wholly before MCU `first` or start at or after MCU `last`; else it decodes its chunk, up to `last`.  A
 *             segment's lane returns when its MCUs miss [first, last).  Blocks of MCUs at or after `last` stay zero.
 *   idct      a lane per block of the MCU rectangle.     colour   a lane per 16 pixels of a row of the box.
 * The bytes of `out` are bit for bit the box cut from coclr_jpeg_decode_store's frame.  status holds the bits met in
 * the chunks and segments that WERE decoded: damage outside them goes unreported; a clean file gives 0 either way.
 * Sample planes outside the MCU rectangle are not written and not read.  The bounds of coclr_jpeg_decode_store hold.
 * COCLR_EINVAL before any launch: what coclr_jpeg_decode_store refuses (output frames and the first two prefix rows
 * measured for the window); a null window table; w < 1, h < 1, or a box that leaves its frame.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_jpeg_decode_store_window(const coclr_jpeg_store* st, const int64_t* sel, const int64_t* sel_host, int F,
                                   const int64_t* geom, const int64_t* geom_host, const int64_t* window,
                                   const int64_t* window_host, const int64_t* prefix, const int64_t* prefix_host,
                                   int stages, int16_t* coefs, uint8_t* planes, int64_t coef_blocks, uint8_t* out,
                                   int64_t out_bytes, int32_t* status, void* stream);

/* Copies the bytes and rows of m distinct frames of a store to a device arena, one launch, so that a store whose
 * `data` and `rows` lie in PINNED HOST memory (a dataset larger than the device's memory) is decoded by
 * coclr_jpeg_decode_store / _window from the arena: a coclr_jpeg_store whose data / rows are the arena's, whose frames
 * are the rebased records and whose tables / segs are the source store's own, with the selection 0 .. n-1.  `st` with
 * device data and rows is taken alike (compaction).
 * st: the source.  data and rows: device memory, or host memory registered with the runtime (hipHostMalloc,
 *   hipHostRegister), 16-byte aligned, allocated with 16 bytes of room behind data_bytes.  Only frames_host is read of
 *   its tables.
 * plan: int64 [m][8], DEVICE, and plan_host (csrc/jpeg_core.h: JG_*): per distinct frame {store frame, first byte and
 *   byte count in the store, first byte in the arena, first row and row count in the store, first row in the arena,
 *   lanes of all frames before it}.  A frame's lanes are the 16-byte words of its hull [base & ~15, (base + len + 15)
 *   & ~15) -- none for an empty frame -- and then its rows.  Its first arena byte is congruent to its first store byte
 *   mod 16; hulls follow each other in the arena from byte 0 without a gap, rows likewise from row 0.  What a hull
 *   holds outside its frame is copied too and is never read.
 * slot_host: int64 [n], HOST: the plan entry of each of the n frames of the decode call (repeats share one).
 * frames_host: int64 [n][8], HOST: the rebased records the decode call will be given: the store's own with the first
 *   byte and the first row replaced by the arena's (jc_gather_rebase).
 * arena: arena_bytes bytes, arena_rows: uint32 [arena_nrows][4], both DEVICE and 16-byte aligned.
 * The kernel reads the device plan and holds every word it touches against the four buffer sizes, which it is given
 * by value: whatever the plan holds, nothing outside the 16-byte words of data, rows, arena and arena_rows is touched.
 * COCLR_EINVAL before any launch: a null or misaligned pointer; m < 1 or n < m; a plan frame outside [0, nframes),
 * whose record is not one coclr_jpeg_decode_store takes, whose bytes or rows leave the source arrays or are not what
 * the plan says; an arena byte that breaks the congruence or a hull that does not start where the one before it ends;
 * a hull or rows that leave the arena; a lane prefix that is not the frames' lane counts; a slot outside [0, m); a
 * rebased record that is not the store's record moved to the plan's place; and a source data or rows pointer whose
 * first or last byte hipPointerGetAttributes does not report as device memory or registered host memory (pageable and
 * managed memory are refused, and the runtime's last-error state is left clean).
 * Additive: the ABI number stays 26 -- no existing signature or behaviour changed. */
int coclr_jpeg_store_gather(const coclr_jpeg_store* st, const int64_t* plan, const int64_t* plan_host, int64_t m,
                            const int64_t* slot_host, const int64_t* frames_host, int64_t n, uint8_t* arena,
                            int64_t arena_bytes, uint32_t* arena_rows, int64_t arena_nrows, void* stream);

/* coclr_jpeg_store_gather with a SOURCE per plan row: the shards of one dataset lie in different buffers -- stores of
 * this process, device or pinned host, or the device memory of another rank of the node mapped through hipIpc
 * (coclr_amd/jpeg.py: class ShardedStore) -- and one launch copies the selection's distinct frames from whichever
 * shard holds them into the arena, which is then decoded exactly as there.
 * shards: nshards (1..8, JG_MAX_SHARDS: one per GPU of a node) sources.  Of each only data, data_bytes, rows, nrows,
 *   chunk_bytes and the HOST tables are read: frames_host (its own nframes records, bytes and rows counted inside the
 *   shard; may be null when nframes is 0: a shard may be empty), tables_host / table_sets and segs_host / nsegs as the
 *   records name them.  frames, tables and segs (DEVICE) may be null.  data and rows as coclr_jpeg_store_gather's.
 * plan, plan_host: as coclr_jpeg_store_gather, with {frame, first byte, first row} counted inside the row's own shard
 *   and the congruence held to the frame's first SHARD byte.
 * shard: int64 [m], DEVICE, and shard_host: the source of every plan row.  Rows are ordered by (shard, frame), strictly.
 * slot_host, frames_host, arena, arena_rows: as coclr_jpeg_store_gather; a rebased record is its shard's record moved.
 * The kernel is coclr_jpeg_store_gather's with a by-value table {data, words, rows, nrows} per source: a lane reads its
 * row's shard from the device column, returns when that lies outside [0, nshards), and holds its word against THAT
 * source's sizes and the arena's.  Whatever the device plan and shard column hold, nothing outside the buffers is
 * touched.
 * COCLR_EINVAL before any launch: what coclr_jpeg_store_gather refuses, per row against the row's own shard; nshards
 * outside 1..8; a null shard (or one without data, rows or host tables); shards that differ in chunk_bytes; a shard
 * index outside [0, nshards); rows not ordered by (shard, frame); and ANY shard's data or rows pointer -- read by a
 * row or not -- whose first or last byte hipPointerGetAttributes does not report as device memory or registered host
 * memory (the runtime's last-error state is left clean).  A buffer opened from a hipIpc handle has to pass that same
 * query: no launch on an address the runtime has not vouched for.
 * Additive: the ABI number stays 26 -- no existing signature or behaviour changed. */
int coclr_jpeg_store_gather_shards(const coclr_jpeg_store* const* shards, int nshards, const int64_t* plan,
                                   const int64_t* plan_host, const int64_t* shard, const int64_t* shard_host,
                                   int64_t m, const int64_t* slot_host, const int64_t* frames_host, int64_t n,
                                   uint8_t* arena, int64_t arena_bytes, uint32_t* arena_rows, int64_t arena_nrows,
                                   void* stream);

/* coclr_resize_boxes_u8 for frames that differ in size from clip to clip: `frames` is ONE flat byte buffer of nbytes
 * bytes, 16-byte aligned, and a descriptor is int32 [14]: the ten words of coclr_resize_boxes_u8 ({first frame} is
 * not read) followed by {byte offset of the clip's first frame, low word; high word; W; H} of the clip's T frames,
 * which follow each other at W * H * 3 bytes rounded up to 16.  The same kernel body; the box is clamped to, and checked against, the
 * clip's OWN frame.  Clips may share frames.  The LDS band is sized by the tallest box of the launch, as there.
 * COCLR_EINVAL before any launch: what coclr_resize_boxes_u8 refuses; nbytes < 1; an offset that is negative, not a
 * multiple of 16 or whose T frames leave the buffer; W or H < 1; a box that leaves its own W x H frame (whether or not
 * it would fit a larger frame of the batch).
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_resize_boxes_ragged_u8(const uint8_t* frames, int64_t nbytes, const int32_t* desc, const int32_t* desc_host,
                                 int n_clips, int T, int S, const int32_t* xtab, int64_t xlen, const int32_t* ytab,
                                 int64_t ylen, uint8_t* out, void* stream);

/* coclr_resize2_boxes for frames that differ in size from clip to clip: `frames` and the four trailing descriptor
 * words as coclr_resize_boxes_ragged_u8 (a descriptor is int32 [18]); everything else as coclr_resize2_boxes, the
 * region clamped to and checked against the clip's own frame.
 * COCLR_EINVAL before any launch: what coclr_resize2_boxes refuses, and what coclr_resize_boxes_ragged_u8 refuses of
 * the buffer, the offsets and the frame sizes.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_resize2_boxes_ragged(const uint8_t* frames, int64_t nbytes, const int32_t* desc, const int32_t* desc_host,
                               int n_clips, int T, int size, int S, const int32_t* xtab, int64_t xlen,
                               const int32_t* ytab, int64_t ylen, const int32_t* tab2, int64_t len2, int taps2,
                               const float* mean, const float* std, uint8_t* out8, float* out, void* stream);

/* Five/ten-crop test clips of MANY videos, of differing frame sizes, in one launch (eval/main_classifier.py:425-521,
 * 548-684: the test modes and the retrieval feature extraction): the chain of coclr_stage_crops /
 * coclr_resize_crops_u8 -- flip the frame -> crop the cw x ch box at (x0, y0) OF THE FLIPPED FRAME -> PIL's
 * Image.resize((S, S), BICUBIC) on 8-bit pixels -> bytes, or / 255 -> (x - mean[c]) / std[c] -- with the geometry per
 * output clip.  It is the same kernel body, the geometry read from a descriptor instead of the arguments.
 * frames: ONE flat byte buffer of nbytes bytes, 16-byte aligned (a staging.RaggedFrames).  An output clip is one
 * (video, crop, clip) triple, one row of the model's batch.  desc: int32 [n_clips][5] = {x0, y0, flip, W, H}, W x H
 * the size of the clip's frames, on the device, and desc_host, the same on the host.  slot_off: int64 [n_clips*T],
 * the byte offset of the frame every (clip, t) reads, device and host: per slot, because test clips are strided
 * (ds > 1), left-padded with frame 0 when the video is shorter than a clip, and overlap; slots may repeat and clips
 * may share frames.  cw, ch, S and the four tables are those of coclr_stage_crops, one set for the launch.
 * Exactly one output: out fp32 [n_clips][3][T][S][S], normalised (mean / std HOST arrays read at call time), or out8
 * uint8 [n_clips*T][S][S][3], the input of coclr_color_jitter_clips with group_size = T (one program per clip).
 * The descriptors and offsets are device data: the kernel clamps W, H and the box into range and skips a slot whose
 * frame would not lie inside [0, nbytes) or is smaller than the crop, so nothing is read or written out of bounds
 * whatever the device copies hold.
 * COCLR_EINVAL before any launch: a null pointer; frames, xmin or xk not 16-byte aligned, slot_off not 8-byte, desc,
 * ymin, yk or out not 4-byte; both outputs or neither; out without mean / std; std == 0; nbytes, n_clips, T, S, cw,
 * ch < 1; S > 512; taps outside 1..64; W or H outside 1..32768; a box that leaves its OWN W x H frame (whether or not
 * it would fit a larger frame of the batch); flip not 0/1; a slot offset that is negative, not a multiple of 16 or
 * whose 3 * W * H bytes leave the buffer; n_clips*T > 65535 or a grid over the launch limits; an output row whose
 * ytaps source rows (3*Sp bytes each) exceed 64 KiB.
 * Additive: the ABI number stays 25 -- no existing signature or behaviour changed. */
int coclr_stage_crops_ragged(const uint8_t* frames, int64_t nbytes, const int32_t* desc, const int32_t* desc_host,
                             int n_clips, int T, const int64_t* slot_off, const int64_t* slot_off_host, int cw, int ch,
                             int S, const int32_t* xmin, const int32_t* xk, int xtaps, const int32_t* ymin,
                             const int32_t* yk, int ytaps, const float* mean, const float* std, uint8_t* out8,
                             float* out, void* stream);

/* What the staging launchers above would do (ABI 26): each query takes the arguments of its launcher without the
 * stream, runs the launcher's own validation and planning function -- the launcher launches from the struct this
 * reports -- and launches nothing.  No device is needed and no DEVICE pointer is read: of those only whether they
 * are null and how they are aligned matters, so any address with the alignment in question will do.  HOST arrays
 * (crops, desc_host, slot_off_host, kinds_host, params_host, mean, std) are read as the launcher reads them.
 * Each returns what its launcher would return before launching: COCLR_EINVAL for everything the launcher refuses,
 * and for a null `plan`.
 *
 * Crop form (coclr_stage_crops with `out`, coclr_resize_crops_u8 with `out8`; exactly one of the two),
 * coclr_stage_crops_ragged, and the box form (ragged = 0 coclr_resize_boxes_u8, 1 coclr_resize_boxes_ragged_u8):
 *  plan[0] R, output rows per band      plan[1] bands (grid x)     plan[2] cap_rows, source rows a band may stage
 *  plan[3] dynamic LDS bytes            plan[4] cap_rows is the box height, not the bound (clipped)
 *  plan[5] U8OUT instantiation          plan[6] RAGGED instantiation
 *  plan[7] 16-byte stores (fp32 forms: S % 4 == 0 and `out` 16-byte aligned).  Unlike the other fields this one is a
 *          RESTATEMENT: the crop kernels evaluate the same predicate themselves from S and `out` and are not handed
 *          the flag (their bodies are as they were before ABI 26); tests/test_gpu_stage_exact.py holds the rows on
 *          either side of it to the exact result.  The same holds for plan[9] of the two-stage form below.
 *          coclr_stage_clips_plan's plan[1] and coclr_jitter_plan's plan[5] ARE the values their kernels branch on. */
int coclr_stage_crops_plan(const uint8_t* frames, int F, int H, int W, const int32_t* slot_frame, int n_clips,
                           int T, const int32_t* crops, int n_crops, int cw, int ch, int S, const int32_t* xmin,
                           const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                           const float* mean, const float* std, uint8_t* out8, float* out, int32_t plan[8]);
int coclr_stage_crops_ragged_plan(const uint8_t* frames, int64_t nbytes, const int32_t* desc,
                                  const int32_t* desc_host, int n_clips, int T, const int64_t* slot_off,
                                  const int64_t* slot_off_host, int cw, int ch, int S, const int32_t* xmin,
                                  const int32_t* xk, int xtaps, const int32_t* ymin, const int32_t* yk, int ytaps,
                                  const float* mean, const float* std, uint8_t* out8, float* out, int32_t plan[8]);
int coclr_resize_boxes_plan(int ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W,
                            const int32_t* desc, const int32_t* desc_host, int n_clips, int T, int S,
                            const int32_t* xtab, int64_t xlen, const int32_t* ytab, int64_t ylen, uint8_t* out,
                            int32_t plan[8]);
/* Two-stage form (ragged = 0 coclr_resize2_boxes, 1 coclr_resize2_boxes_ragged):
 *  plan[0] R    plan[1] bands    plan[2] cap1, source rows    plan[3] capA, rows of the size x size image
 *  plan[4] dynamic LDS bytes     plan[5] `one` is sized by H1's rows (cap1 * 3 * P), not H2's (capA * 3 * Sp)
 *  plan[6] more than 64 KiB: the instantiation's dynamic-LDS limit is raised
 *  plan[7] U8OUT    plan[8] RAGGED    plan[9] 16-byte stores (as above: a restatement of the kernel's own test) */
int coclr_resize2_boxes_plan(int ragged, const uint8_t* frames, int64_t nbytes, int F, int H, int W,
                             const int32_t* desc, const int32_t* desc_host, int n_clips, int T, int size, int S,
                             const int32_t* xtab, int64_t xlen, const int32_t* ytab, int64_t ylen,
                             const int32_t* tab2, int64_t len2, int taps2, const float* mean, const float* std,
                             uint8_t* out8, float* out, int32_t plan[10]);
/* coclr_stage_clips:  plan[0] uint8 source instantiation    plan[1] 16-byte loads and stores: THW a multiple of 16
 * (uint8) / 4 (fp32) elements and BOTH `frames` and `out` 16-byte aligned; the kernel branches on this value and
 * nothing else    plan[2] grid x */
int coclr_stage_clips_plan(const void* frames, int from_u8, float* out, int B, int C, int S, int64_t THW,
                           const float* mean, const float* std, int32_t plan[3]);
/* Program form (aug = 0 coclr_color_jitter_clips, 1 coclr_augment_clips):
 *  plan[0] AUG instantiation    plan[1] use_lds (a program has a contrast or a blur)    plan[2] dynamic LDS bytes
 *  plan[3] items (four pixels each)    plan[4] items per lane    plan[5] 16-byte stores (W % 4 == 0, `out` aligned)
 *  plan[6] contrast and blur ops of the longest program: the passes it is cut into, less one */
int coclr_jitter_plan(int aug, const uint8_t* frames, int N, int H, int W, int T, const int32_t* kinds,
                      const float* params, const int32_t* kinds_host, const float* params_host, int G, int P,
                      int group_size, const float* mean, const float* std, float* out, int32_t plan[7]);

/* ------------------------------------------------------------------------ */
/* Evaluation consumers (model/classifier.py:47-61; eval/main_classifier.py) */
/* ------------------------------------------------------------------------ */

/* fp32 workspace elements for the two column-statistics entry points below. */
int coclr_colstats_workspace(int rows, int cols, int64_t* elems);
/* BatchNorm1d batch statistics of pooled features x[rows][cols] (final_bn, classifier.py:34,56)
 * as stats[2][cols] = {sum, sum of squares}: the layout coclr_bn_finalize takes with ntiles=1. */
int coclr_bn1d_stats(const float* x, float* stats, float* workspace, int rows, int cols,
                     void* stream);
/* out = x - x.mean(0) (eval/main_classifier.py:690-691). */
int coclr_center_rows(const float* x, float* out, float* workspace, int rows, int cols,
                      void* stream);
/* Nearest-neighbour retrieval (eval/main_classifier.py:699-703): for every row of sim[B][N] the
 * kmax most similar columns in order (value descending, column ascending on ties);
 * hits[b][i] = 1.0 if any(train_label[top ks[i] columns] == test_label[b]) else 0.0 (fp32, so
 * coclr_colsum gives the accuracies); ks ascending, ks[nk-1] ==
 * kmax.  topidx (optional) int32[B][kmax] receives the selected columns. */
int coclr_retrieval_hits(const float* sim, const int64_t* train_label, const int64_t* test_label,
                         const int32_t* ks, int nk, float* hits, int32_t* topidx, int B, int N,
                         int kmax, void* stream);

/* Two-stream score fusion (eval/merge_2stream_prob.py:80-98): for every video v of p1[V][C] and p2[V][C]
 * (dense fp32 rows), fused[v][c] = ((double)p1 + (double)p2) * 0.5 as float64, and argmax[v][0..2] = the
 * first maximum (value descending, column ascending: np.argmax) of p1[v], of p2[v] and of fused[v];
 * hits[v][i] = 1.0 if argmax[v][i] == label[v] else 0.0 (fp32, so coclr_colsum gives the three
 * accuracies).  C has no upper limit.  A NaN leaves the arg-maxima in [0, C) and deterministic, no more. */
int coclr_fuse_scores(const float* p1, const float* p2, const int64_t* label, double* fused,
                      int32_t* argmax, float* hits, int V, int C, void* stream);

/* Video-level scores of the test modes (eval/main_classifier.py:488,533): for every segment s = {first row,
 * rows, out row} of logits[R][C],  out[out row][:] += weight[s] * sum over its rows of softmax(row), rows
 * added in ascending order in fp32 (no atomics: results are run-to-run identical).  `segs` (S x 3 int32) and
 * `weight` (S floats) are HOST arrays read at call time; out is [V][C] on the device and is accumulated
 * into.  Segments naming the same out row are applied in the order given.  1 <= C <= 4096;
 * COCLR_EINVAL for an empty or out-of-range segment (nothing is launched then). */
int coclr_segment_softmax_accum(const float* logits, const int32_t* segs, const float* weight, float* out,
                                int R, int C, int S, int V, void* stream);
/* The same without the softmax: per-video feature sums (eval/main_classifier.py:637,673). */
int coclr_segment_accum(const float* x, const int32_t* segs, const float* weight, float* out, int R, int C,
                        int S, int V, void* stream);

/* Library/ABI version, bumped when a signature changes. */
int coclr_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* COCLR_HIP_H_ */
