/*
 * robosat_hip.h -- C ABI of librobosat_hip.so: the MI355X (gfx950) implementation of the RoboSat U-Net hot path.
 *
 * The reference (mapbox/robosat v1.2.0) has no FFI of its own: its hot path is Python calling torch ops
 * (SURVEY.md section 0.1).  This header is therefore the boundary a maintainer binds *beneath* the reference's
 * Python operator surface; every entry point names the reference call it replaces (file:line under
 * /root/reference).  INTEGRATION.md shows the ctypes stub.
 *
 * Conventions
 *   - plain device pointers + sizes, no torch types; `stream` is a hipStream_t passed as void*.
 *   - every function only ENQUEUES work on `stream` (no allocation, no implicit sync) and returns a hipError_t
 *     as int (0 = success); argument errors return RS_EINVAL (-22) before anything is enqueued.
 *   - activations are NHWC fp32 ("channels last"): x[n][y][x][c].  Convolution weights are KRSC fp32
 *     (w[cout][ky][kx][cin]) == a torch [Cout,Cin,kh,kw] tensor in channels_last memory format.
 *   - logits / probabilities / loss inputs are NCHW fp32, label maps are [N][H][W] int64: exactly the tensors the
 *     reference's losses and predict tool see (robosat/losses.py, robosat/tools/predict.py:87).
 */
#ifndef ROBOSAT_HIP_H
#define ROBOSAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RS_EINVAL (-22)

typedef void* rs_stream_t;

/* Activation storage types of the *_dt / *_bf16 entry points (the bf16 training path, BASELINE configs[2]).
 * bf16 tensors are passed as raw 16-bit words (torch.bfloat16 storage); arithmetic and accumulation stay fp32. */
typedef uint16_t rs_bf16;
#define RS_F32 0
#define RS_BF16 1

/* Version of this ABI (bumped on any signature change). */
int rs_abi_version(void);

/* ------------------------------------------------------------------------------------------------------------
 * Convolution (implicit GEMM on v_mfma_f32_32x32x2_f32; exact fp32).
 *
 * One descriptor covers every convolution in UNet.forward (robosat/unet.py:122-141):
 *   - resnet.conv1 7x7/2 stem                      (unet.py:122)   stem = 1
 *   - Bottleneck 1x1, 3x3 (stride 1|2), downsample (unet.py:127-130; torchvision 0.3.0 resnet50)
 *   - ConvRelu 3x3 + ReLU                          (unet.py:32,44)
 *   - DecoderBlock = interpolate(nearest, x2) then ConvRelu (unet.py:73), with the torch.cat of the skip tensor
 *     (unet.py:134-137) folded in: src1 = skip (first C1 channels), src2 = previous decoder output (next C2).
 *     Neither the upsampled nor the concatenated tensor is ever materialised.
 * and, by symmetry, every data-gradient convolution of loss.backward() (robosat/tools/train.py:186):
 *   ups = 2 reads the source through a zero-inserted x2 grid (the adjoint of a stride-2 convolution).
 *
 * out[n][oy][ox][co] = epilogue( sum_{ky,kx,ci} in[n][oy*stride-pad+ky][ox*stride-pad+kx][ci] * w[co][ky][kx][ci] )
 * epilogue(v) = relu?( v * scale[co] + shift[co] + residual[n][oy][ox][co] )   (each part optional / NULL)
 * and, when relu_mask != NULL, the result is zeroed wherever relu_mask[n][oy][ox][co] <= 0 (the ReLU backward of the
 * layer whose output `relu_mask` is, fused into the data-gradient convolution that produces its gradient).
 * ---------------------------------------------------------------------------------------------------------- */
typedef struct rs_conv_desc {
  int32_t N;          /* batch */
  int32_t Hs, Ws;     /* spatial size of the source tensor(s) as stored */
  int32_t C1, C2;     /* channels of src1 / src2 (C2 = 0: single source); C1, C2 multiples of 32 unless stem */
  int32_t ups;        /* 0: none; 1: nearest x2 upsample fused into the gather; 2: zero-insert x2 (stride-2 dgrad) */
  int32_t kh, kw, stride, pad;
  int32_t Ho, Wo;     /* output spatial size */
  int32_t Cout;       /* multiple of 32 */
  int32_t relu;       /* 1: ReLU in the epilogue */
  int32_t stem;       /* 1: src1 is NHWC with 4 channels, weights packed [Cout][kh][8][4] (see rs_pack_stem_weight): resnet.conv1,
                         7x7 / stride 2 / pad 3 -> 64 (stem_f32.hip); 3: ... and the 4th channel of src1 and the filter's c = 3
                         entries are zeros (an RGB image through rs_nchw_to_nhwc4): they are skipped, not multiplied */
} rs_conv_desc;

int rs_conv2d_fwd(const rs_conv_desc* d, const float* src1, const float* src2, const float* weight,
                  const float* scale, const float* shift, const float* residual, const float* relu_mask, float* out,
                  rs_stream_t stream);

/* Which tile configuration rs_conv2d_fwd picks for `d` (index into rs_conv2d_tile_name); for the roofline report. */
int rs_conv2d_tile(const rs_conv_desc* d);
const char* rs_conv2d_tile_name(int tile);

/* resnet.conv1 weight [Cout][kh][kw][Cin<=4] (KRSC) -> [Cout][kh][8][4], zero padded (unet.py:122). */
int rs_pack_stem_weight(const float* w_krsc, float* packed, int Cout, int kh, int kw, int Cin, rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Layout / elementwise / pooling
 * ---------------------------------------------------------------------------------------------------------- */

/* images.to(device) as UNet.forward receives them (train.py:172, predict.py:83): NCHW [N][C<=4][H][W] -> NHWC4,
 * channel 3 zero-filled when C == 3. */
int rs_nchw_to_nhwc4(const float* x, float* y, int N, int C, int H, int W, rs_stream_t stream);

/* F.max_pool2d on NHWC: resnet.maxpool 3x3/2 pad 1 (unet.py:125) and the 2x2/2 before `center` (unet.py:132).
 * Padding behaves as -inf (torch semantics).  C multiple of 4.  `argmax` (optional, uint8 [N][Ho][Wo][C]) receives
 * the winning tap ky*k+kx (first maximum in row-major window order, as torch picks) for the backward pass. */
int rs_maxpool2d_fwd(const float* x, float* y, uint8_t* argmax, int N, int H, int W, int C, int k, int stride, int pad,
                     int Ho, int Wo, rs_stream_t stream);

/* Eval-mode BatchNorm2d folded to per-channel scale/shift for the conv epilogue (resnet bn*, eps as torch):
 * scale = gamma / sqrt(var + eps), shift = beta - mean * scale. */
int rs_bn_fold(const float* gamma, const float* beta, const float* mean, const float* var, float eps, float* scale,
               float* shift, int C, rs_stream_t stream);

/* self.final (unet.py:108,141): 1x1 conv Cin=32..128 (multiple of 4, <= 128) -> C classes (<= 8) with bias, reading
 * NHWC and writing NCHW.  softmax = 1 additionally applies nn.functional.softmax(dim=1) (predict.py:87). */
int rs_final_conv1x1(const float* x, const float* w, const float* bias, float* out, int N, int H, int W, int Cin,
                     int C, int softmax, rs_stream_t stream);


/* ------------------------------------------------------------------------------------------------------------
 * Training path: what autograd synthesises for loss.backward() (robosat/tools/train.py:186) and train-mode
 * BatchNorm (net.train(), tools/train.py:169).  Workspaces are caller-provided; query sizes with *_workspace_bytes.
 * ---------------------------------------------------------------------------------------------------------- */

/* Filter gradient of the convolution described by `d` (same descriptor as the forward call; `relu` is ignored):
 *   dw[co][ky][kx][ci] = sum_{n,oy,ox} dy[n][oy][ox][co] * in[n][oy*stride-pad+ky][ox*stride-pad+kx][ci]
 * with `in` read through the forward gather (upsample / concat / stem packing).  dw is KRSC (packed [Cout][kh][8][4]
 * for the stem -> rs_unpack_stem_weight).  Split-P partials live in `workspace`; deterministic (no atomics). */
long rs_conv2d_wgrad_workspace_bytes(const rs_conv_desc* d);
/* Which form rs_conv2d_wgrad runs this fp32 launch in (a pure host decision on the geometry and the knobs): 0 the direct form,
 * 2 the phase form of DecoderBlock (unet.py:63-73; 4/9 of the multiply-adds), 3 the same in the Winograd domain of the forward's
 * F(2x2, 2x2) form (1/4; conv_wgrad_wino_f32.hip, round 6), 4 a stride-1 3x3 / pad-1 convolution (torchvision Bottleneck.conv2) in the
 * Winograd domain of F(2x2, 3x3) (16/36; conv_wgrad_wino33_f32.hip, round 6); RS_EINVAL for a descriptor rs_conv2d_wgrad refuses. */
int rs_conv2d_wgrad_form(const rs_conv_desc* d);
int rs_conv2d_wgrad(const rs_conv_desc* d, const float* dy, const float* src1, const float* src2, float* dw,
                    void* workspace, rs_stream_t stream);
int rs_unpack_stem_weight(const float* packed, float* w_krsc, int Cout, int kh, int kw, int Cin, rs_stream_t stream);

/* Forward KRSC weights [Cout][kh][kw][Cin] -> data-gradient weights [Cin][kh][kw][Cout] with flipped taps.  The data
 * gradient of a convolution is rs_conv2d_fwd on dy with these weights, pad' = k-1-pad, and ups = 2 when the forward
 * stride was 2. */
int rs_pack_dgrad_weight(const float* w_krsc, float* out, int Cout, int kh, int kw, int Cin, rs_stream_t stream);

/* Train-mode BatchNorm2d over y [M = N*H*W][C] (torchvision resnet50 bn*, eps 1e-5, momentum 0.1):
 * rs_bn_train_stats: batch mean / biased variance -> mean, invstd = 1/sqrt(var+eps), scale = gamma*invstd,
 *   shift = beta - mean*scale; running_mean/var (optional, both or neither) updated with the UNBIASED variance;
 *   *num_batches_tracked (optional, int64) += 1.
 * rs_bn_apply: out = relu?( y*scale + shift (+ residual) ).
 * rs_bn_bwd: g = dz * (zmask > 0) (zmask optional = the ReLU output); dgamma = sum g*xhat, dbeta = sum g,
 *   dy = gamma*invstd*(g - dbeta/M - xhat*dgamma/M); dmasked (optional) receives g (gradient of the residual branch).
 * workspace: rs_bn_workspace_bytes(M, C) + 3*C*sizeof(float) bytes. */
long rs_bn_workspace_bytes(long M, int C);
int rs_bn_train_stats(const float* y, long M, int C, float eps, float momentum, const float* gamma, const float* beta,
                      float* mean, float* invstd, float* scale, float* shift, float* running_mean, float* running_var,
                      long long* num_batches_tracked, void* workspace, rs_stream_t stream);
int rs_bn_apply(const float* y, const float* scale, const float* shift, const float* residual, float* out, long M, int C,
                int relu, rs_stream_t stream);
int rs_bn_bwd(const float* dz, const float* zmask, const float* y, const float* mean, const float* invstd,
              const float* gamma, float* dy, float* dmasked, float* dgamma, float* dbeta, long M, int C, void* workspace,
              rs_stream_t stream);

/* Backward of F.max_pool2d given the argmax taps recorded by rs_maxpool2d_fwd; accumulate = 1 adds into dx. */
int rs_maxpool2d_bwd(const float* dy, const uint8_t* argmax, float* dx, int N, int H, int W, int C, int k, int stride,
                     int pad, int Ho, int Wo, int accumulate, rs_stream_t stream);

/* Backward of interpolate(nearest, x2) + torch.cat split: dup [N][2H][2W][C1+C2] -> d1 [N][H][W][C1] (+= when
 * accumulate1), d2 [N][H][W][C2]; mask1/mask2 (optional): ReLU outputs whose backward is fused (zero where <= 0). */
int rs_upsample2x_bwd(const float* dup, float* d1, float* d2, const float* mask1, const float* mask2, int N, int H, int W,
                      int C1, int C2, int accumulate1, rs_stream_t stream);

/* Backward of self.final (unet.py:108,141): x NHWC [N][H][W][Cin<=64], dlogits NCHW -> dx (zeroed where x <= 0 when
 * relu_mask: x is the ReLU output dec5), dw [C][Cin], db [C]. */
long rs_final_conv1x1_bwd_workspace_bytes(int Cin, int C);
int rs_final_conv1x1_bwd(const float* x, const float* w, const float* dlogits, float* dx, float* dw, float* db, int N, int H,
                         int W, int Cin, int C, int relu_mask, void* workspace, rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Losses (robosat/losses.py) and metrics (robosat/metrics.py) on NCHW logits + int64 [N][H][W] targets
 * ---------------------------------------------------------------------------------------------------------- */

/* mode 0: CrossEntropyLoss2d (losses.py:8-25); mode 1: FocalLoss2d with `gamma` (losses.py:28-50).  `weight` [C]
 * optional.  loss[0] = sum w*l / sum w; stats[0..1] = (loss, sum w) is consumed by the backward:
 * dlogits = grad_out[0] * w[t] * dl/dx / sum w  (grad_out NULL = 1). */
long rs_nll_loss_workspace_bytes(void);
int rs_nll_loss_fwd(const float* logits, const long long* targets, const float* weight, float* loss, float* stats, int N,
                    int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream);
int rs_nll_loss_bwd(const float* logits, const long long* targets, const float* weight, const float* stats,
                    const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                    rs_stream_t stream);

/* mIoULoss2d (losses.py:53-83): max(1 - mean_{c,n} softIoU, weighted NLL), gradient through the larger branch.
 * stats needs 5 + 2*N*C floats: loss, sum w, chosen branch (0 miou / 1 nll), per-(n,c) gradient coefficients, then the
 * miou branch's value and the nll branch's numerator sum_i w_i l_i.  rs_miou_loss_bwd reads [1] (the NLL denominator) and
 * [2] (the branch) back: data-parallel ranks overwrite them with the global batch's (the reference evaluates
 * max(miou, nll) ONCE over the gathered batch, losses.py:83 under tools/train.py:69). */
long rs_miou_loss_workspace_bytes(int N, int C);
int rs_miou_loss_fwd(const float* logits, const long long* targets, const float* weight, float* loss, float* stats, int N,
                     int C, int H, int W, void* workspace, rs_stream_t stream);
int rs_miou_loss_bwd(const float* logits, const long long* targets, const float* weight, const float* stats,
                     const float* grad_out, float* dlogits, int N, int C, int H, int W, rs_stream_t stream);

/* LovaszLoss2d (losses.py:86-119): batched radix sort + scans.  loss[0] = mean over images; grad_unit (optional,
 * NCHW like logits) receives d loss / d logits for grad_out = 1 (multiply with rs_scale_by_scalar). */
long rs_lovasz_workspace_bytes(int N, int C, int H, int W);
int rs_lovasz_fwd(const float* logits, const long long* targets, float* loss, float* grad_unit, int N, int C, int H, int W,
                  void* workspace, rs_stream_t stream);
int rs_scale_by_scalar(const float* src, const float* scalar, float* dst, long n, rs_stream_t stream);

/* Lovasz-Softmax (Berman et al. 2018, arXiv 1705.08790), the multi-class loss of the paper.  logits [N,C,H,W] fp32 (C >= 2),
 * targets [N,H,W] int64 in [0, C).  p = softmax(logits) over C; per segment s -- (image n, class c) when per_image, class c
 * over the whole batch otherwise -- the errors e_i = |1[y_i = c] - p_{c,i}| (fp32) are sorted descending, EQUAL ERRORS IN
 * ASCENDING PIXEL INDEX (n, h, w): this tie order makes the gradient a defined function of the input.  With g = sum 1[y = c]
 * and k_r the labels among the first r + 1: I_r = g - k_r, U_r = g + r + 1 - k_r, delta_0 = 1 / U_0,
 * delta_r = (I_{r-1} U_r - I_r U_{r-1}) / (U_r U_{r-1}) (integer numerator), L_s = sum_r e_{pi(r)} delta_r (fp64).
 * loss[0] = mean_n mean_{c in P_n} L_{n,c} (per_image) or mean_{c in P} L_c, P = the classes with g > 0 or, with
 * all_classes, every class.  grad_unit (optional, NCHW) = d loss / d logits for grad_out = 1 (autograd of this definition
 * through the softmax; multiply with rs_scale_by_scalar); probs_out (optional, NCHW) receives the fp32 p the keys were made
 * from.  Deterministic (no float atomics): bit-identical run to run.  RS_EINVAL for C < 2, a non-positive size,
 * N*C*H*W >= 2^31 or more than 65535 segments. */
long rs_lovasz_softmax_workspace_bytes(int N, int C, int H, int W, int per_image);
int rs_lovasz_softmax_fwd(const float* logits, const long long* targets, float* loss, float* grad_unit, float* probs_out, int N,
                          int C, int H, int W, int per_image, int all_classes, void* workspace, rs_stream_t stream);

/* The five losses above with an IGNORE LABEL: `ignore` is a label value that is no class, C <= ignore <= 255 (RS_EINVAL otherwise;
 * the label rasters are bytes).  Each entry point is its base signature plus `int ignore`, with the base call's workspace.  The loss
 * is the base definition evaluated on the VALID pixels only (targets != ignore): as if the ignored pixels had been cut out of every
 * image and the rest packed together in their (n, h, w) order.  Labels >= C other than `ignore` are undefined, as in the base calls.
 *   - rs_nll_loss_*_ig: loss = sum_valid w l / sum_valid w; stats[1] is that denominator.  A denominator of 0 (no valid pixel, or
 *     only classes of weight 0) gives loss 0 and gradient 0, not NaN.
 *   - rs_miou_loss_*_ig: the soft-IoU sums of each (class, image) run over the valid pixels; an image with no valid pixel has ratio 1
 *     in every class (no loss, no gradient) and the mean stays over C*N terms.  The NLL term is as above; the max(miou, nll) branch
 *     and the stats layout are the base call's.
 *   - rs_lovasz_fwd_ig: per image the sort runs over the C*K entries of its K valid pixels with gts = K; an image with K = 0
 *     contributes 0; the divisor stays N.
 *   - rs_lovasz_softmax_fwd_ig: a segment holds valid pixels only and the present classes are judged on them; per image, an image
 *     with no valid pixel contributes 0 and the divisor stays N; flattened, no valid pixel at all gives 0.  Equal errors stay in
 *     ascending pixel index.  probs_out still receives the softmax of every pixel.
 * In all of them d loss / d logits is exactly +0.0f in every class plane of an ignored pixel, the label of an ignored pixel never
 * indexes `weight`, and for finite logits neither loss nor gradient depends on the logits at ignored pixels (non-finite logits
 * under ignored pixels are not shielded in the two Lovasz forms, whose softmax / sort still see them).  With no pixel ignored the
 * results are the base calls' bit for bit.  The fixed divisors (N, C*N) and the exchanged normaliser stats[1] are what the
 * data-parallel exchange of robosat_amd/losses.py rests on: it is unchanged.
 * In the two Lovasz forms an ignored pixel's entries get a key behind every valid key (error -inf / -1) and label bit 0: the stable
 * sort puts them in the tail of their segment, where they change no prefix count, add 0 to the loss and get gradient 0; each
 * segment's gts is counted from its label bits.  No host synchronisation: every call can be captured into a graph. */
int rs_nll_loss_fwd_ig(const float* logits, const long long* targets, const float* weight, float* loss, float* stats, int N,
                       int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream, int ignore);
int rs_nll_loss_bwd_ig(const float* logits, const long long* targets, const float* weight, const float* stats,
                       const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                       rs_stream_t stream, int ignore);
int rs_miou_loss_fwd_ig(const float* logits, const long long* targets, const float* weight, float* loss, float* stats, int N,
                        int C, int H, int W, void* workspace, rs_stream_t stream, int ignore);
int rs_miou_loss_bwd_ig(const float* logits, const long long* targets, const float* weight, const float* stats,
                        const float* grad_out, float* dlogits, int N, int C, int H, int W, rs_stream_t stream, int ignore);
int rs_lovasz_fwd_ig(const float* logits, const long long* targets, float* loss, float* grad_unit, int N, int C, int H, int W,
                     void* workspace, rs_stream_t stream, int ignore);
int rs_lovasz_softmax_fwd_ig(const float* logits, const long long* targets, float* loss, float* grad_unit, float* probs_out, int N,
                             int C, int H, int W, int per_image, int all_classes, void* workspace, rs_stream_t stream, int ignore);

/* BOUNDARY-WEIGHTED CrossEntropy / Focal (`rs train`: `[opt] boundary_weight`, `boundary_sigma`): the border weight map of the U-Net
 * paper (Ronneberger et al. 2015, its first term), a per-pixel weight that decays with the distance from the nearest label boundary,
 * made from the label raster on the device at every step.
 *
 * Inputs:
 * - targets: int64 [N][H][W]
 * - C classes
 * - an optional ignore label
 * - w0 > 0
 * - sigma > 0, with R = ceil(3*sigma) and 1 <= R <= 128
 *
 * Rules:
 * - A pixel is *valid* if its label is not the ignore label.
 * - A *boundary pixel* is a valid pixel with a 4-neighbour inside the same image that is valid and has another label.
 *   - The edge of the image is no boundary.
 *   - The edge of an ignored region is no boundary.
 *   - This is the rule rs_features_edt and rs_eval_boundary already follow: nothing is known there.
 *   - Images never see each other.
 * - d2(p) = min(R^2, squared centre-to-centre distance from p to the nearest boundary pixel of its image).
 *   - This is rs_features_edt(complement of the boundary set, R), which gives 0 on a boundary pixel.
 *   - An image without a boundary has R^2 everywhere.
 * - The host makes a table in float64 and rounds it once to float32: table[k] = float32(1 + w0*exp(-k / (2*sigma^2))), k = 0 .. R^2-1.
 * - The weight plane m is float32 [N][H][W]:
 *   - m(p) = table[d2(p)] where d2(p) < R^2
 *   - exactly 1.0f where d2(p) == R^2
 *   - exactly 0.0f at an ignored pixel
 *   - Because d2 is an integer and the table comes from the host, the plane is defined bit for bit.
 * - Loss, for CrossEntropy and Focal alike:
 *   - loss = sum_valid m_p*w[t_p]*l_p / sum_valid m_p*w[t_p]
 *   - stats[1] is that denominator.
 *   - A denominator of 0 gives loss 0 and gradient 0.
 *   - dlogits = grad_out * m_p*w[t_p] * dl/dx / stats[1]
 *   - The gradient is exactly +0.0f in every class plane of an ignored pixel.
 *   - Sums are accumulated in double, as in nll_fwd_kernel.
 *   - There are no float atomics.  The same input gives the same bits in every run.
 *   - There is no host synchronisation.  Every call can be captured into a graph.
 *
 * The paper's second term (d1 + d2 to the two nearest OBJECTS, which opens gaps between touching cells) is the SEPARATION WEIGHT
 * further down (rs_separation_weight_plane), which adds onto this plane.
 *
 * rs_boundary_weight_plane: targets, table [R*R] (device), R, ignore (-1 for none) -> plane m.  Four launches: the uint8 complement
 * of the boundary set (0 = boundary pixel, 1 = any other valid pixel, 2 = ignored; non-zero = set) from the int64 labels, the two
 * passes of rs_features_edt on it (called as it is), the lookup d2 -> m.  The mask, g and d2 planes live in `workspace`
 * (rs_boundary_weight_plane_workspace_bytes(N, H, W) = 6 bytes per pixel; RS_EINVAL for sizes rs_features_edt refuses: N > 65535,
 * H or W > 4096, N*H*W >= 2^29).  Labels >= C other than `ignore` are undefined, as in the losses.
 * rs_nll_loss_fwd_pw / rs_nll_loss_bwd_pw: the base signature plus `pixel_weight` [N][H][W] (ANY non-negative finite plane, not only
 * one made above) plus `ignore` (-1 for none), with the base call's workspace: the sums above with m = pixel_weight.  They are the
 * `_ig` kernels with one more load and one more multiply per pixel (an ignored pixel's weight is never read); with a plane of 1.0f
 * they do the base call's arithmetic in its order.
 * RS_EINVAL: R outside 1..128, C outside 1..8, an ignore label that is neither -1 nor in C..255, a non-positive size. */
long rs_boundary_weight_plane_workspace_bytes(int N, int H, int W);
int rs_boundary_weight_plane(const long long* targets, const float* table, float* plane, int N, int C, int H, int W, int R, int ignore,
                             void* workspace, rs_stream_t stream);
int rs_nll_loss_fwd_pw(const float* logits, const long long* targets, const float* weight, float* loss, float* stats, int N,
                       int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream, const float* pixel_weight,
                       int ignore);
int rs_nll_loss_bwd_pw(const float* logits, const long long* targets, const float* weight, const float* stats,
                       const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                       rs_stream_t stream, const float* pixel_weight, int ignore);

/* SEPARATION WEIGHT for CrossEntropy / Focal (`rs train`: `[opt] separation_weight`, `separation_sigma`): the second term of the U-Net
 * paper's weight map (Ronneberger et al. 2015, eq. 2), ws*exp(-(d1 + d2)^2 / (2*sigma^2)) with d1 and d2 the distances to the nearest
 * and the second-nearest OBJECT.  It is large only in a narrow background corridor between two different objects.  DESIGN.md section 7i.
 *
 * Per image n of the int64 label raster [N][H][W] with C classes and an optional ignore label:
 * - A pixel is *valid* if its label is not the ignore label (tested first).  An *object pixel* is a valid pixel whose label is one of
 *   1 .. C-1; class 0 is the background.  Any other valid pixel counts as background.
 * - The *objects* are the 4-connected components of the object pixels inside the image (rs_features_label on the object mask).
 *   - Two touching objects of different classes are one object: there is no gap between them to keep open.
 *   - An ignored pixel belongs to no object and is no background.  Distances pass over it.
 *   - Nothing lies beyond the image's edge.  Images never see each other.
 * - For a valid background pixel p and an object k: delta_k(p) = min over the pixels q of k of |p - q|^2, an integer >= 1.
 *   - a <= b are the two smallest of the per-object values (a == b where two objects tie for nearest).
 *   - With fewer than two objects in the image the term is 0.
 * - s2 = a + b + isqrt(4*a*b), isqrt the exact integer floor square root: s2 = floor((sqrt a + sqrt b)^2), the paper's (d1 + d2)^2
 *   rounded down to an integer, so the exponent is off by less than 1 / (2*sigma^2).
 * - Reach D = ceil(3*sigma), 1 <= D <= 32.  term(p) = table[s2] if s2 < D^2, else 0; 0 at every pixel that is no valid background.
 *   - The host makes the table in float64 and rounds it once: table[k] = float32(ws*exp(-k / (2*sigma^2))), k = 0 .. D^2-1.
 *   - s2 > b, so only objects with delta < D^2 matter: nothing further than D-1 pixels in x or y is looked at.
 * - plane[p] = base[p] + term(p), one fp32 addition; without `base`, base is exactly 1.0f at a valid pixel and 0.0f at an ignored one.
 *   Where the term is 0 the plane is the base to the bit (the base is copied, nothing is added).
 *
 * rs_separation_weight_plane: one memset and six launches on `stream`: the class bytes (0 background, 1 object, 2 ignored) and the
 * object mask; the three launches of rs_features_label (called as it is; labels = root pixel index + 1, so they depend on no
 * scheduling); a row pass that gives every pixel the two nearest DISTINCT labels of its row within |dx| < D, each with its |dx| (left
 * before right at equal |dx|; a candidate is (label << 5) | |dx| in one int32, 0 = none); a column pass that merges both candidates
 * of every row |dy| < D into a running best two by distinct label (value dy^2 + dx^2), walking outward until dy^2 >= the second best,
 * then makes s2, looks the table up, adds the base and writes the plane -- exactly once per pixel, by one thread.  Two candidates per row
 * suffice: an object that is third or later in a row stands behind two distinct objects that are at most as far through that row.
 * No atomics of its own, integer arithmetic up to the lookup: the same input gives the same bits in every run.  No allocation and no
 * host synchronisation: the call can be captured into a graph.
 * `workspace`: rs_separation_weight_plane_workspace_bytes(N, H, W) = 16 + 14 bytes per pixel, 16-byte aligned.  Its first int32 is the
 * labelling's `err` word (rs_features_label), zeroed on the stream in every call and left there for the caller to read if it wants to.
 * `base` may be null.
 * RS_EINVAL: a null pointer that may not be null, a misaligned workspace, D outside 1..32, C outside 1..256, an ignore label that is
 * neither -1 nor in 1..255, the sizes rs_features_label refuses (N > 65535, H or W > 4096, N*H*W >= 2^29, a non-positive size). */
long rs_separation_weight_plane_workspace_bytes(int N, int H, int W);
int rs_separation_weight_plane(const long long* targets, const float* table, const float* base, float* plane, int N, int C, int H, int W,
                               int D, int ignore, void* workspace, rs_stream_t stream);

/* BOUNDARY LABEL RELAXATION for CrossEntropy / Focal (`rs train`: `[opt] relax`): near an outline either neighbouring class is
 * acceptable (Zhu et al., CVPR 2019, "Improving Semantic Segmentation via Video Propagation and Label Relaxation").  At a pixel whose
 * neighbourhood holds several classes the loss maximises the probability of their union, -log sum_{c in S} p_c instead of -log p_t.
 * DESIGN.md section 7k.
 *
 * Inputs:
 * - the int64 label raster [N][H][W] with C <= 8 classes, so a set of classes fits a byte
 * - an optional ignore label
 * - the relaxation radius R in pixels, 1 <= R <= 16
 *
 * Rules:
 * - A pixel is *valid* if its label is not the ignore label.
 * - The label set plane `sets` is uint8 [N][H][W]:
 *   - For a valid pixel p, bit c of sets(p) is set iff some valid pixel q of the same image has |qx - px| <= R, |qy - py| <= R and
 *     label c.  The window is a square: it covers every translation of the label layer by up to R pixels per axis.
 *   - Nothing lies beyond the image's edge.  Images never see each other.  Ignored pixels add no bit.
 *   - sets(p) = 0 at an ignored pixel.  A valid pixel always holds its own bit.
 *   - The plane is integers only, so it is defined bit for bit.
 * - Pixel term, with S = sets(p):
 *   - lse = logsumexp_c x_c over all classes; lse_S = logsumexp_{c in S} x_c, with its own maximum taken over S
 *   - log q = lse_S - lse;  r_c = exp(x_c - lse_S) for c in S, 0 otherwise (computed as exp(x_c - max_S) / sum_S)
 *   - CrossEntropy: l = -log q, dl/dx_c = p_c - r_c
 *   - Focal: l = -(1 - q)^gamma * log q, dl/dx_c = k*(r_c - p_c), k = gamma*(1 - q)^(gamma-1) * q * log q - (1 - q)^gamma
 *   - A pixel whose set is its own label alone has lse_S = x_t and r_t = 1 exactly, and does the arithmetic of the `_pw` kernels in
 *     their order: on such an input loss, stats and gradient are theirs bit for bit.
 *   - A pixel whose set is all C classes has log q = 0 and a CrossEntropy gradient of exactly 0.
 * - Loss: loss = sum_valid m_p*w[t_p]*l_p / sum_valid m_p*w[t_p].
 *   - The class weight is that of the pixel's OWN label, and m is the optional pixel-weight plane.
 *   - So stats[1] is exactly the `_pw` call's and does not depend on the sets.
 *   - A denominator of 0 gives loss 0 and gradient 0.
 *   - The gradient is exactly +0.0f in every class plane of an ignored pixel and of a pixel of weight 0.
 *   - Sums are accumulated in double in a fixed order.  There are no float atomics: the same input gives the same bits in every run.
 *   - There is no host synchronisation.  Every call can be captured into a graph.
 *
 * rs_label_set_plane: targets, R, ignore (-1 for none) -> sets.  One launch that reads the labels once and writes one byte per pixel: a
 * block stages a 64 x 64 tile plus an apron of R as class bits in LDS, four pixels per dword, ORs along the rows, then along the
 * columns, and stores.  A window of 2R+1 is built by doubling, w_2k(i) = w_k(i) | w_k(i+k), and one OR of two overlapping
 * power-of-two windows: about log2(2R+1) + 1 ORs per pass.  No workspace.  Labels >= C other than `ignore` are undefined, as in
 * the losses.
 * rs_nll_loss_fwd_rx / rs_nll_loss_bwd_rx: the `_pw` signatures plus `sets` [N][H][W] (ANY plane of class sets, not only one made
 * above; a valid pixel's own bit is taken as set), with the base call's workspace and the `_pw` launch geometry.  `pixel_weight`
 * may be null: every valid pixel then weighs 1.
 * RS_EINVAL: a null pointer that may not be null, R outside 1..16, C outside 1..8, an ignore label that is neither -1 nor in
 * C..255, a non-positive size, the sizes the boundary and separation planes refuse (N > 65535, H or W > 4096, N*H*W >= 2^29; the
 * plane only), a mode that is neither CrossEntropy nor Focal. */
int rs_label_set_plane(const long long* targets, uint8_t* sets, int N, int C, int H, int W, int R, int ignore, rs_stream_t stream);
int rs_nll_loss_fwd_rx(const float* logits, const long long* targets, const float* weight, float* loss, float* stats, int N,
                       int C, int H, int W, int mode, float gamma, void* workspace, rs_stream_t stream, const float* pixel_weight,
                       int ignore, const uint8_t* sets);
int rs_nll_loss_bwd_rx(const float* logits, const long long* targets, const float* weight, const float* stats,
                       const float* grad_out, float* dlogits, int N, int C, int H, int W, int mode, float gamma,
                       rs_stream_t stream, const float* pixel_weight, int ignore, const uint8_t* sets);

/* HARD-PIXEL MINING for CrossEntropy / Focal (`rs train`: `[opt] hard_fraction`, `hard_below`): online hard example mining, also
 * called bootstrapped cross-entropy or top-k pixel loss.  Per image, only the hardest share of the pixels keeps its weight; the others
 * get weight 0 in the `_pw` loss above.  DESIGN.md section 7e.
 *
 * For every image n of the batch, independently:
 * - Key.  A pixel whose label is not the ignore label is *valid*.  Its key is its unweighted cross-entropy l = lse - x_t, computed in
 *   fp32 by the function the loss kernels use (pixel_loss, mode 0), whatever the loss's own mode.
 *   - Focal is monotone in the true class's probability, so the ranking by cross-entropy is the ranking by Focal.
 *   - The ranking does not depend on the class weights.
 *   - As a uint32 the key is bits(l) if l > 0, else 0: -0.0f, a tiny negative rounding result and NaN become 0.
 *   - The bit patterns of non-negative floats order like the floats.
 * - Count.  V_n is the number of valid pixels.
 *   - k_n = 0 if V_n = 0.
 *   - Otherwise k_n = min(V_n, max(1, (int64) ceil(fraction * (double) V_n))).
 *   - `fraction` is a double and the product one IEEE double multiply: the same integer on the host and on the device.
 * - Threshold.  tau_n is the k_n-th largest key among the valid pixels of image n (0 where V_n = 0).
 *   - tau_n = min(tau_n, cap); cap = bits(float32(-ln m)) for a probability bound m in (0, 1), made by the host in float64 and rounded
 *     once.  0xFFFFFFFF means "no cap".
 *   - So a pixel whose true class has a probability below m is always kept, and `fraction` reads "at least this share".
 * - Plane: float32 [N][H][W].
 *   - A valid pixel with key >= tau_n is *kept* and gets base[p], or exactly 1.0f without a base plane.
 *   - Every other pixel gets exactly +0.0f.
 *   - Ties at tau_n are all kept: kept_n >= k_n, and the set depends on no traversal order.
 *   - V_n = 0 keeps nothing.
 * - Loss: rs_nll_loss_fwd_pw / bwd_pw with that plane, sum_kept base*w[t]*l / sum_kept base*w[t].  The selection is piecewise
 *   constant: no gradient flows through it, and a dropped pixel's gradient is +0.0f in every class plane.
 * - Per image, not per batch: an image's selection depends neither on its companions in the batch nor on how the batch is split over
 *   ranks.
 *
 * info: int64 [N][4] = (V_n, k_n, tau_n, kept_n).
 * rs_hard_pixel_select: the selection and the plane on a key plane the caller supplies (any uint32 values): the histograms zeroed on
 * the stream, then an exact radix select over the 32 key bits in three rounds of 11 / 11 / 10 bits from the top -- a histogram of the
 * round's digit over the valid keys that carry the prefix found so far (per block in LDS, the lanes of a wave that hold one digit
 * added as one, one integer atomic per non-empty bin into the image's histogram), then one block per image that walks the bins from
 * the top, finds the digit that holds the k_n-th largest and writes the longer prefix and the remaining rank (the first round's also
 * makes V_n and k_n) -- then the plane and kept_n.  Eight launches for every shape, the first of which zeroes the histograms; integer
 * sums only, so the same input gives the same bits in every run; no allocation, no host synchronisation: the call can be captured
 * into a graph.
 * rs_hard_pixel_plane: the key kernel (one thread per pixel, an ignored pixel's logits are not read; into `keys_out` where that is
 * given, else into the workspace) followed by exactly those stages.
 * `targets` of rs_hard_pixel_select may be null iff ignore < 0; `base` and `keys_out` may be null.  `workspace`:
 * rs_hard_pixel_workspace_bytes(N, H, W) bytes, 16-byte aligned.
 * The scalar arguments of this ABI are int, long and float (tests/test_host_logic.py binds them by class), so the double `fraction`
 * travels as `fraction_bits`, the 64 bits of the IEEE double in a long -- exactly, no float in between -- and the uint32 `cap` as a
 * long in 0..0xFFFFFFFF.
 * RS_EINVAL: a null pointer that may not be null, a misaligned workspace, C outside 1..8, a fraction that is not finite or not in
 * (0, 1], a cap outside 0..0xFFFFFFFF, an ignore label that is neither -1 nor in C..255 (select: 0..255), a non-positive size, H*W >= 2^31. */
long rs_hard_pixel_workspace_bytes(int N, int H, int W);
int rs_hard_pixel_plane(const float* logits, const long long* targets, const float* base, float* plane, unsigned* keys_out,
                        long long* info, int N, int C, int H, int W, long fraction_bits, long cap, int ignore, void* workspace,
                        rs_stream_t stream);
int rs_hard_pixel_select(const unsigned* keys, const long long* targets, const float* base, float* plane, long long* info, int N,
                         int H, int W, long fraction_bits, long cap, int ignore, void* workspace, rs_stream_t stream);

/* THE TVERSKY LOSS FAMILY with a fused cross-entropy term (`rs train`: `[opt] loss = "Tversky"`): Dice, the Tversky index (Salehi et
 * al. 2017), the focal Tversky loss (Abraham & Khan 2019) and "that term plus cross-entropy".  DESIGN.md section 7g.
 *
 * Inputs: logits [N][C][H][W] fp32 with 2 <= C <= 8, targets int64 [N][H][W], an optional `weight` [C] (it weighs the cross-entropy
 * term only) and `ignore`, -1 for none or a label value with C <= ignore <= 255.  A pixel is *valid* if its label is not `ignore`; an
 * ignored pixel enters no sum, its gradient is exactly +0.0f in every class plane and its logits are never read.  With p = softmax
 * over C:
 * - Segment.  s = (image n, class c) when per_image, class c over the whole batch otherwise.
 * - Sums over the valid pixels of a segment: TP = sum_{t=c} p_c, SP = sum p_c, cnt = #{t=c}; FP = SP - TP, FN = cnt - TP.
 * - Tversky index: TI_s = (TP + eps) / (TP + alpha*FP + beta*FN + eps), and TI_s = 1 where the denominator is 0.
 * - Segment loss: l_s = max(1 - TI_s, 0)^gamma.  Where 1 - TI_s <= 0, d l_s / d TI_s is -1 for gamma == 1 and 0 otherwise; a segment
 *   whose denominator is 0 has no gradient.
 * - Segments that count.  Without all_classes those with cnt > 0; with it every segment of an image that has a valid pixel (batch
 *   form: every class, if the batch has a valid pixel).
 * - Tversky term.  Per image T = (1/N) sum_n mean_{c in P_n} l_{n,c}: an image with empty P_n contributes 0 and the divisor stays N.
 *   Batch form T = mean_{c in P} l_c, 0 for empty P.
 * - Pixel term.  CE = sum_valid w[t] (-log p_t) / sum_valid w[t]; a zero denominator gives 0 and no gradient, as in rs_nll_loss_fwd_ig.
 * - loss = T + lambda*CE.  With lambda == 0 the pixel term adds nothing to loss or gradient.
 * alpha = beta = 0.5 is Dice; alpha = beta = 1 the soft Jaccard, which with eps = 0, gamma = 1, all_classes and per_image is the
 * soft-IoU term of rs_miou_loss_fwd.  beta > alpha favours recall.  alpha, beta >= 0 and not both 0, gamma > 0, eps >= 0, lambda >= 0,
 * all finite: float32 values, used as the doubles they convert to.
 *
 * The forward is two calls, so that data-parallel ranks can exchange the sums between them:
 * rs_tversky_sums: one pass over logits and targets (one thread per pixel, at most 64 blocks per image; fp64 partial sums per block),
 * then one block that adds them in a fixed order.  sums (fp64) per image: [N][C][3] = (TP, SP, cnt), then the CE numerator and
 * denominator (3*N*C + 2 doubles); batch form: [C][3], the images added in ascending order, then the same two (3*C + 2 doubles).
 * `workspace`: rs_tversky_workspace_bytes(N, C) bytes, 8-byte aligned; every word the call reads was written by the same call.
 * rs_tversky_finalize: one launch, from `sums` to loss[0] and stats [4 + 2*S] floats, S = N*C per image and C otherwise:
 * [0] the loss, [1] T, [2] the CE numerator, [3] the CE denominator / world (what the backward divides by), [4 + s] d loss / d p_c
 * for a pixel with t == c of segment s, [4 + S + s] for a valid pixel with t != c.  `world` >= 1 is the number of data-parallel ranks
 * whose sums were added into `sums` before the call (1: none).  Per image only the CE denominator is exchanged, and
 * loss = T + lambda * numerator / (denominator / world): the mean of the ranks' losses is the global batch's.  In the batch form the
 * whole block is exchanged, every rank's loss is the global one and its coefficients are multiplied by world, so that the mean of the
 * ranks' gradients is the gradient of the one evaluation over the concatenated batch.
 * rs_tversky_bwd: one pass, dlogits_c = grad_out[0] * ( p_c (g_c - sum_j p_j g_j) + lambda * w[t] (p_c - 1[c == t]) / stats[3] ), g_c
 * the coefficient of the pixel's segment of class c; grad_out NULL = 1; per_image, lambda and ignore as given to the forward.
 * Every reduction is fp64 in a fixed order, without float atomics: the same input gives the same bits in every run, with `ignore`
 * = -1 and with an ignore label that no pixel carries alike.  No host synchronisation: every call can be captured into a graph.
 * RS_EINVAL: a null pointer other than weight and grad_out, C outside 2..8, a non-positive size, N > 65535, N*C*H*W >= 2^31, an ignore
 * label that is neither -1 nor in C..255, a misaligned workspace, world < 1, a parameter out of range or not finite. */
long rs_tversky_workspace_bytes(int N, int C);
int rs_tversky_sums(const float* logits, const long long* targets, const float* weight, double* sums, int N, int C, int H, int W,
                    int per_image, int ignore, void* workspace, rs_stream_t stream);
int rs_tversky_finalize(const double* sums, float* loss, float* stats, int N, int C, float alpha, float beta, float gamma, float eps,
                        float lambda, int all_classes, int per_image, int world, rs_stream_t stream);
int rs_tversky_bwd(const float* logits, const long long* targets, const float* weight, const float* stats, const float* grad_out,
                   float* dlogits, int N, int C, int H, int W, int per_image, float lambda, int ignore, rs_stream_t stream);

/* THE clDice TOPOLOGY LOSS (`rs train`: `[opt] cldice`, `cldice_iters`, `cldice_smooth`, `cldice_classes`) of Shit et al., "clDice -- a
 * Novel Topology-Preserving Loss Function for Tubular Structure Segmentation", CVPR 2021: a Dice-like score between each side's soft
 * skeleton and the other side's mask, added to a region loss.  DESIGN.md section 7j.
 *
 * SOFT SKELETON of fp32 planes X [M][H][W] with values in [0, 1], S = skel(X, iters), 0 <= iters <= 64 (the paper's soft_skel):
 * - E_0 = X, E_{k+1} = erode(E_k), O_k = dilate(E_{k+1}), D_k = relu(E_k - O_k) for k = 0 .. iters.
 * - S_0 = D_0, S_k = S_{k-1} + relu(D_k - S_{k-1}*D_k), S = S_iters.
 * - erode(x) = min(v, h), v the minimum over (N, C, S), h the minimum over (W, C, E); dilate = the maximum over the 3x3 square.
 *   Nothing lies beyond a plane's edge: a cell outside it is never a candidate of a min or a max.  Planes never see each other.
 * - The paper's code recomputes the erosion inside every opening; this shared form gives the same bits with iters + 1 erosions.
 * - Forward arithmetic: every subtraction, product and sum is one separately rounded fp32 operation (no FMA contraction), so the
 *   forward equals the op-by-op fp32 evaluation bit for bit.
 * - Backward tie rules (what torch's CPU autograd does with the paper's code):
 *   - v: the gradient goes to the first cell attaining it in the order N, C, S; h: in the order W, C, E.
 *   - erode: v < h, all through v; h < v, all through h; v == h, half through each, even when both halves land on the same cell.
 *   - dilate: to the first maximum in row-major order of the 3x3 window.
 *   - relu'(0) = 0.
 * rs_soft_skeleton_fwd: iters + 2 launches; launch j reads E_j and writes E_{j+1} and S_{j-1}, so no launch reads a neighbour that a
 * block of the same launch writes.  `state` holds rs_soft_skeleton_state_floats(M, H, W, iters, save) floats: with `save` the planes
 * E_1 .. E_{iters+1} then S_0 .. S_{iters-1} (2*iters + 1 planes of M*H*W floats, what the backward reads besides X itself); without
 * it five planes that the levels use in turn, and the call leaves nothing to keep.  `skel` receives S.
 * rs_soft_skeleton_bwd: `grad` = dL/dS -> `dplanes` = dL/dX from X and the saved `state`.  One launch for the pixel-local chain through
 * the S updates, then iters + 2 launches in gather form: every cell of E_k collects from the at most 9 dilation windows and the at
 * most 5 erosions that selected it, the selections recomputed from E_k by the tie rules.  `workspace`:
 * rs_soft_skeleton_bwd_workspace_bytes(M, H, W, iters) = (iters + 3) planes, 4-byte aligned.
 * No atomics: the same input gives the same bits in every run.  No host synchronisation, no allocation: both can be captured.
 * RS_EINVAL: a null pointer, a non-positive size, iters outside 0..64, M*H*W >= 2^31, a misaligned workspace.
 *
 * THE LOSS.  K = the classes of `class_mask` (bit c set = class c; only classes 1 .. C-1), pairs = N*|K| planes in the order
 * [n][class ascending].  Per pair: P = softmax(logits)[n][c] in fp32, Y = (target == c) as 0/1; both are 0 at a pixel whose label is
 * `ignore`, and the gradient under such a pixel is exactly 0.  With S_P = skel(P), S_Y = skel(Y) (no gradient through Y):
 *   Tprec = (sum S_P*Y + smooth) / (sum S_P + smooth), Tsens = (sum S_Y*P + smooth) / (sum S_Y + smooth),
 *   term = 1 - 2*Tprec*Tsens / (Tprec + Tsens); loss = the mean of the term over ALL pairs (an absent class is not skipped).
 * A ratio whose denominator is 0 counts as 0 and has no gradient; Tprec + Tsens = 0 gives the term 1 and no gradient (smooth = 0 only).
 * The divisor depends on the batch size alone: the mean of data-parallel ranks' losses over equal batches is the global value.
 * rs_cldice_planes: logits [N][C][H][W] fp32 (2 <= C <= 8), targets int64 -> P and Y [pairs][H][W].
 * rs_cldice_sums: sums[pair][4] = (sum S_P*Y, sum S_P, sum S_Y*P, sum S_Y) in fp64, at most 64 blocks per plane, their partial sums
 * added in ascending block order; `workspace`: rs_cldice_workspace_bytes(pairs), 8-byte aligned.
 * rs_cldice_finalize: one block: loss[0] and coef[pair][3] = (alpha, beta, gamma) with dL/dS_P = alpha*Y + beta per pixel and
 * dL/dP through Tsens = gamma*S_Y.
 * rs_cldice_skel_grad: grad = alpha*Y + beta, the `grad` of rs_soft_skeleton_bwd.
 * rs_cldice_bwd: g_c = dP[c] + gamma_c*S_Y[c] for the classes of the mask, 0 for the others and the background;
 * dlogits_k = grad_out[0] * p_k * (g_k - sum_c g_c*p_c); grad_out NULL = 1; +0.0f in every class plane under an ignored pixel.
 * Every reduction is fp64 in a fixed order without float atomics; no host synchronisation.
 * RS_EINVAL: a null pointer other than grad_out, C outside 2..8, an empty mask or one with bit 0 or a bit >= C, a non-positive size,
 * N or pairs > 65535, N*C*H*W >= 2^31, an ignore label that is neither -1 nor in C..255, a misaligned workspace, smooth < 0 or not finite. */
long rs_soft_skeleton_state_floats(int M, int H, int W, int iters, int save);
int rs_soft_skeleton_fwd(const float* planes, float* skel, float* state, int M, int H, int W, int iters, int save, rs_stream_t stream);
long rs_soft_skeleton_bwd_workspace_bytes(int M, int H, int W, int iters);
int rs_soft_skeleton_bwd(const float* planes, const float* state, const float* grad, float* dplanes, int M, int H, int W, int iters,
                         void* workspace, rs_stream_t stream);
int rs_cldice_planes(const float* logits, const long long* targets, float* P, float* Y, int N, int C, int H, int W, int class_mask,
                     int ignore, rs_stream_t stream);
long rs_cldice_workspace_bytes(int pairs);
int rs_cldice_sums(const float* P, const float* Y, const float* SP, const float* SY, double* sums, int pairs, int H, int W,
                   void* workspace, rs_stream_t stream);
int rs_cldice_finalize(const double* sums, float* loss, float* coef, int pairs, float smooth, rs_stream_t stream);
int rs_cldice_skel_grad(const float* Y, const float* coef, float* grad, int pairs, int H, int W, rs_stream_t stream);
int rs_cldice_bwd(const float* logits, const long long* targets, const float* dP, const float* SY, const float* coef,
                  const float* grad_out, float* dlogits, int N, int C, int H, int W, int class_mask, int ignore, rs_stream_t stream);

/* Metrics.add over a whole batch (metrics.py:27-41): counts[0..3] += (tn, fn, fp, tp) in the reference's naming. */
int rs_confusion_counts(const float* scores, const long long* targets, unsigned long long* counts, int N, int C, int H,
                        int W, rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * bf16 path (BASELINE configs[2]: rs train bf16): the same operators with activations stored as bf16 NHWC, fp32
 * master weights cast per step, fp32 accumulation (v_mfma_f32_32x32x16_bf16), fp32 statistics / gradients of
 * parameters / logits / losses.  The image is cast to bf16 on upload (rs_nchw_to_nhwc4_bf16); the 7x7 stem has its own
 * bf16 kernels (rs_stem_conv_*_bf16).
 *
 * `_dt` variants: same contract as the fp32 entry point of the same name, activations typed by `dtype`
 * (RS_F32 | RS_BF16); per-channel vectors, parameter gradients, logits and workspaces are always fp32.
 * ---------------------------------------------------------------------------------------------------------- */

/* rs_conv2d_fwd with bf16 sources / weights (KRSC bf16) / residual / relu_mask / output; scale, shift fp32.
 * stem = 1 is not supported here.  Same fused gather (ups, concat) and epilogue. */
int rs_conv2d_fwd_bf16(const rs_conv_desc* d, const rs_bf16* src1, const rs_bf16* src2, const rs_bf16* weight,
                       const float* scale, const float* shift, const rs_bf16* residual, const rs_bf16* relu_mask,
                       rs_bf16* out, rs_stream_t stream);
int rs_conv2d_tile_bf16(const rs_conv_desc* d);
/* Tile index (rs_conv2d_tile_name order) and K-chunk row size (64 | 128 bytes) the dispatcher picks for `d` with `es`-byte
 * activations, direct (phase4 = 0) or phase form: kernel names in reports then map 1:1 to the launched symbols. */
int rs_conv2d_config(const rs_conv_desc* d, int es, int form, int* tile, int* rowb);
/* (`form`: bit 0 = phase form; bit 1 = a launch with a fused epilogue beyond scale / shift / residual / ReLU -- BatchNorm statistics,
 * a ReLU mask, two destinations -- which never takes the plain-epilogue fp32 1x1 kernel.) */
/* Dispatcher override for the parity tests and A/B measurements (process-global; not a tuning API for callers): force the
 * tile (index as above; honoured for every launch that tile can run, -1 = the measured heuristics) and the K-chunk row
 * size (64 | 128; 0 = heuristics).  rs_conv2d_config reports what a launch will then use, so a test can assert that the
 * symbol it means to cover is the one that ran.  The reference has no counterpart: cuDNN's autotuner
 * (torch.backends.cudnn.benchmark, tools/train.py:72-73) is its equivalent of the heuristics this overrides.
 * Tile 8 = the bf16 HALO-ONCE forms (3x3 / stride 1 / pad 1; DecoderBlock phase form; its 4x4 / stride-2 data gradient):
 * the block's rows are a 2-D patch of the output grid (8 x 32 pixels; rowb = 64: 16 x 32 pixels with 32-channel chunks),
 * its source halo is copied to LDS once per channel chunk and every filter tap reads it at a row offset.  rs_conv2d_config
 * reports them as tile 8 with the N tile (128 | 64, + 0x1000 for the 512-pixel patch) in *rowb. */
int rs_conv2d_set_tuning(int tile, int rowb);
/* The library's measurement / A-B switches by name (process-global; robosat_amd/csrc/knobs.hip lists them with the environment
 * variable that seeds each ONCE, at the first use: "conv1x1_ew" <- RS_CONV1X1_EW, "conv_halo" <- RS_CONV_HALO,
 * "wgrad_f32_phase" <- RS_WGRAD_F32_PHASE, ...).  No dispatcher reads the environment per launch: a workspace query and the
 * launch it sizes always see the same settings.  rs_set_knob returns 0, or RS_EINVAL for an unknown name; rs_get_knob writes
 * the current value.  No reference counterpart (torch.backends.cudnn.* flags are the closest). */
int rs_set_knob(const char* name, int value);
int rs_get_knob(const char* name, int* value);
const char* rs_conv2d_tile_name_bf16(int tile);

/* rs_conv2d_wgrad with bf16 dy / sources; dw is fp32 KRSC (the optimizer's master gradient). */
long rs_conv2d_wgrad_bf16_workspace_bytes(const rs_conv_desc* d);
int rs_conv2d_wgrad_bf16_form(const rs_conv_desc* d); /* 0 tap-per-block, 1 all-taps thin kernel, 2 phase form (4/9 MACs) */
int rs_conv2d_wgrad_bf16_tile(const rs_conv_desc* d); /* (couts << 16) | (cins of a second per-source launch << 8) | cins of the tile; 0 = thin kernel */
int rs_conv2d_wgrad_bf16(const rs_conv_desc* d, const rs_bf16* dy, const rs_bf16* src1, const rs_bf16* src2, float* dw,
                         void* workspace, rs_stream_t stream);

/* fp32 master weights -> bf16 compute copies: plain cast (KRSC stays KRSC), and the data-gradient packing of
 * rs_pack_dgrad_weight with a bf16 result. */
int rs_cast_f32_to_bf16(const float* src, rs_bf16* dst, long n, rs_stream_t stream);
/* dst = (float)src * scale.  The gradient exchange of robosat/tools/train.py:69 (DataParallel's reduce-add of 149.4 MB
 * fp32 onto device 0) done in bf16 on the wire (`[model] grad_dtype = "bf16"`, 74.7 MB): the bucket is cast with
 * rs_cast_f32_to_bf16, summed by RCCL, and comes back through this call with scale = 1 / world into the fp32 arena the
 * optimizer reads.  src / dst 16-byte aligned. */
int rs_cast_bf16_to_f32_scaled(const rs_bf16* src, float* dst, long n, float scale, rs_stream_t stream);
/* dst = bf16(src * scale): the way OUT of the same exchange with scale = 1 / world, so that every rank puts an already
 * averaged contribution on the wire and the ring's bf16 partial sums stay at the magnitude of one gradient (summing WORLD
 * unscaled values and dividing afterwards loses mantissa and overflows earlier).  src / dst 16-byte aligned. */
int rs_cast_f32_to_bf16_scaled(const float* src, rs_bf16* dst, long n, float scale, rs_stream_t stream);
int rs_pack_dgrad_weight_bf16(const float* w_krsc, rs_bf16* out, int Cout, int kh, int kw, int Cin, rs_stream_t stream);

/* The 7x7/2 stem (resnet.conv1, unet.py:122) in bf16: x NHWC4 bf16 [N][H][W][4] (rs_nchw_to_nhwc4_bf16), weights packed
 * bf16 [64][7][8][4] (rs_pack_stem_weight_bf16 from the fp32 KRSC master), out [N][H/2][W/2][64] bf16 with the optional
 * eval-BatchNorm scale/shift + ReLU epilogue; rs_stem_conv_wgrad_bf16 returns the PACKED fp32 gradient [64][7][8][4]
 * (-> rs_unpack_stem_weight).  H, W multiples of 32.  One block owns an output patch and all 49 taps (stem_bf16.hip). */
int rs_nchw_to_nhwc4_bf16(const float* x, rs_bf16* y, int N, int C, int H, int W, rs_stream_t stream);
int rs_pack_stem_weight_bf16(const float* w_krsc, rs_bf16* packed, int Cout, int kh, int kw, int Cin, rs_stream_t stream);
int rs_stem_conv_fwd_bf16(const rs_bf16* x, const rs_bf16* w_packed, const float* scale, const float* shift, rs_bf16* out,
                          int N, int H, int W, int relu, rs_stream_t stream);
long rs_stem_conv_wgrad_bf16_workspace_bytes(int N, int H, int W);
int rs_stem_conv_wgrad_bf16(const rs_bf16* dy, const rs_bf16* x, float* dw_packed, int N, int H, int W, void* workspace,
                            rs_stream_t stream);

int rs_maxpool2d_fwd_dt(const void* x, int x_dtype, void* y, int y_dtype, uint8_t* argmax, int N, int H, int W, int C, int k,
                        int stride, int pad, int Ho, int Wo, rs_stream_t stream);
int rs_maxpool2d_bwd_dt(const void* dy, int dy_dtype, const uint8_t* argmax, void* dx, int dx_dtype, int N, int H, int W,
                        int C, int k, int stride, int pad, int Ho, int Wo, int accumulate, rs_stream_t stream);
int rs_final_conv1x1_dt(const void* x, int x_dtype, const float* w, const float* bias, float* out, int N, int H, int W,
                        int Cin, int C, int softmax, rs_stream_t stream);
int rs_final_conv1x1_bwd_dt(const void* x, const float* w, const float* dlogits, void* dx, float* dw, float* db, int dtype,
                            int N, int H, int W, int Cin, int C, int relu_mask, void* workspace, rs_stream_t stream);
int rs_bn_train_stats_dt(const void* y, int dtype, long M, int C, float eps, float momentum, const float* gamma,
                         const float* beta, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                         float* running_var, long long* num_batches_tracked, void* workspace, rs_stream_t stream);
int rs_bn_apply_dt(const void* y, const float* scale, const float* shift, const void* residual, void* out, int dtype, long M,
                   int C, int relu, rs_stream_t stream);
int rs_bn_bwd_dt(const void* dz, const void* zmask, const void* y, const float* mean, const float* invstd, const float* gamma,
                 void* dy, void* dmasked, float* dgamma, float* dbeta, int dtype, long M, int C, void* workspace,
                 rs_stream_t stream);
int rs_upsample2x_bwd_dt(const void* dup, void* d1, void* d2, const void* mask1, const void* mask2, int dtype, int N, int H,
                         int W, int C1, int C2, int accumulate1, rs_stream_t stream);

/* Train-mode convolution that also produces the BatchNorm forward statistics of its output (the conv -> bn pairs of
 * torchvision's Bottleneck, unet.py:127-130): out = conv(gather(src1|src2)) with NO epilogue, plus per-M-tile partial
 * sums stats_partial[tile][0][co] = sum, [tile][1][co] = sum of squares of the values as stored (tiles =
 * rs_conv2d_bnstats_rows(d)); rs_bn_finalize_stats turns them into what rs_bn_train_stats returns, saving that
 * kernel's read pass over the activation.  Not for the stem. */
long rs_conv2d_bnstats_rows(const rs_conv_desc* d);
/* ... for activations of `dtype` (RS_F32 | RS_BF16): the bf16 halo-once forms of the kernel tile the output into 8 x 32
 * pixel patches (one partial row per patch) where they run; rs_conv2d_bnstats_rows is the fp32 answer. */
long rs_conv2d_bnstats_rows_dt(const rs_conv_desc* d, int dtype);
int rs_conv2d_fwd_bnstats_dt(const rs_conv_desc* d, int dtype, const void* src1, const void* src2, const void* weight,
                             void* out, float* stats_partial, rs_stream_t stream);
int rs_bn_finalize_stats(const float* partial, long rows, long M, int C, float eps, float momentum, const float* gamma,
                         const float* beta, float* mean, float* invstd, float* scale, float* shift, float* running_mean,
                         float* running_var, long long* num_batches_tracked, void* workspace, rs_stream_t stream);
/* (workspace: 64 * 2 * C doubles, optional -- enables the parallel first-level reduction when rows > 256) */

/* Phase form of DecoderBlock (unet.py:73: conv3x3(pad 1) over interpolate(nearest, x2)): each output parity (oy&1, ox&1)
 * sees a 2x2 convolution on the SOURCE grid whose taps are sums of the 3x3 taps that fall on the same source pixel, so
 * the layer is four 2x2 convolutions with 4/9 of the multiply-adds and no duplicated gathers -- same result up to fp32
 * summation order.  `d` describes the original layer (ups = 1, 3x3, stride 1, pad 1, Ho = 2*Hs); `weight_phase` is
 * [4][Cout][2][2][C1+C2] from rs_pack_phase_weight_dt (fp32 KRSC master in, `dtype` out).  Epilogue as rs_conv2d_fwd. */
int rs_pack_phase_weight_dt(const float* w_krsc, void* out, int dtype, int Cout, int Cin, rs_stream_t stream);
/* The DATA gradient of a 3x3 / stride-2 / pad-1 convolution (torchvision Bottleneck.conv2 of layer2..layer4's first block, under
 * loss.backward(), tools/train.py:186) in the same form (round 6): rs_conv2d_fwd_phase_dt over dy [N][Hs][Ws][Cout] with this pack
 * [4][Cin][2][2][Cout] (fp32 KRSC master [Cout][3][3][Cin] in) gives d input [N][2 Hs][2 Ws][Cin] -- on each input parity the gradient
 * is a 2x2 convolution over dy with at most four of the nine taps (zeros elsewhere): 16 multiply-adds per four pixels (9 in the
 * Winograd form of rs_conv2d_fwd_phase_wino) instead of the 36 of the zero-insertion launch (ups = 2) it replaces. */
int rs_pack_s2_dgrad_phase_weight_dt(const float* w_krsc, void* out, int dtype, int Cout, int Cin, rs_stream_t stream);
int rs_conv2d_fwd_phase_dt(const rs_conv_desc* d, int dtype, const void* src1, const void* src2, const void* weight_phase,
                           const float* scale, const float* shift, const void* residual, const void* relu_mask, void* out,
                           rs_stream_t stream);

/* Split K (fp32, the 64x64 tile of the implicit-GEMM kernel, direct or phase form): a launch whose grid cannot fill the chip but
 * whose K loop is long -- the 16x16 stage of the network -- runs as S slices of the K loop per output tile, S x the blocks; each block
 * stores its raw fp32 accumulators to `ws` [S][rows][Cout] (rows = N*Ho*Wo; phase form: [4 parities][N*Hs*Ws]) and a second kernel,
 * splitk_reduce_f32, sums the partials in the fixed order s = 0 .. S-1 and applies the epilogue of rs_conv2d_fwd (scale / shift,
 * residual, ReLU; phase form: the scatter of parity rows to output pixels).  No atomics: bit-reproducible.  The slice bounds fall on
 * 32-channel groups, so the sums do not depend on the K-chunk row size either.
 * rs_conv2d_splitk: the S the dispatcher picks for `d` (`form` as for rs_conv2d_config: bit 0 = phase form, bit 1 = a launch with a
 * ReLU mask / fused statistics, which never splits) and the K-chunk row size in *rowb: 0 = the launch stays unsplit (call
 * rs_conv2d_fwd / rs_conv2d_fwd_phase_dt), S >= 1 = call rs_conv2d_fwd_splitk with a workspace of S * rows * Cout floats.  By rule S
 * is a function of the layer's GEOMETRY only (Hs, Ws, channels, filter, stride), never of N: splitting changes the fp32 summation
 * order, and a tile's output must not depend on the batch it travels in.  Knob "conv_splitk" (RS_CONV_SPLITK): -1 the rule, 0 never,
 * S >= 1 every launch that can (1: one slice through the split path, bit-identical to the unsplit launch), for tests and A/B runs.
 * rs_conv2d_fwd_splitk: `splits` must be what rs_conv2d_splitk answers for the same `d` and `form` (bit 0 only). */
int rs_conv2d_splitk(const rs_conv_desc* d, int form, int* rowb);
int rs_conv2d_fwd_splitk(const rs_conv_desc* d, int form, const float* src1, const float* src2, const float* weight,
                         const float* scale, const float* shift, const float* residual, float* out, float* ws, int splits,
                         rs_stream_t stream);

/* DecoderBlock (unet.py:63-73) in fp32 as a Winograd F(2x2, 2x2) convolution on the phase form: each parity's 2x2
 * convolution on the source grid produces 2x2 blocks of outputs from 3x3 blocks of inputs with 9 multiplies instead of 16
 * (transforms with 0 / +-1 coefficients only): 9/16 of the phase form's MFMA work, 1/4 of the reference-shape count -- for
 * the fp32 path, whose matrix cores (157 TFLOP/s) are the bottleneck of these layers (conv_wino_f32.hip).  `d` describes the
 * layer like rs_conv2d_fwd_phase_dt (ups = 1, 3x3, pad 1, Ho = 2 Hs); the epilogue is the model's: optional ReLU (d->relu).
 * `u` = [4][9][Cout][C1+C2] from rs_pack_wino_phase_weight(phase pack [4][Cout][2][2][Cin] of rs_pack_phase_weight_dt).
 * rs_conv2d_fwd_phase_wino takes ANY phase pack's four 2x2 parity filter sets (also rs_pack_s2_dgrad_phase_weight_dt's: the 3x3 /
 * stride-2 data gradient over dy) and runs one parity per work item (the tile form).  rs_conv2d_fwd_upsampled_wino, same arguments,
 * is for the DecoderBlock alone: `u` MUST come from one 3x3 filter over the upsample (rs_pack_phase_weight_dt), whose parity filters
 * are sums of the same three taps along each axis -- then the p8 blocks compute all four parities per SOURCE PIXEL from nine of the
 * 36 filter slabs (the pixel form; knob "wino_pixel", ROBOSAT_WINO_PIXEL=0: the tile form).  Other filters give wrong results there.
 * The two entry points differ in fp32 summation order; _ok and _name hold for both.
 * rs_conv2d_phase_wino_ok: 0 if this form cannot run `d` (needs >= 4 tiles per image side, channel counts % 16, Cout % 32,
 * 32-bit offsets): use rs_conv2d_fwd_phase_dt; 1 if it can and should; 2 if it can but should not (fewer than 8 tiles per image
 * side: the generic kernel is faster).  The answer depends on the layer's geometry only, never on N: the two forms differ in
 * summation order, and a tile's output must not depend on the size of the batch it travels in.  rs_conv2d_phase_wino_name: the launched instantiation, for reports. */
int rs_conv2d_phase_wino_ok(const rs_conv_desc* d);
const char* rs_conv2d_phase_wino_name(const rs_conv_desc* d);
int rs_pack_wino_phase_weight(const float* w_phase, float* u, int Cout, int Cin, rs_stream_t stream);
int rs_conv2d_fwd_phase_wino(const rs_conv_desc* d, const float* src1, const float* src2, const float* u, float* out,
                             rs_stream_t stream);
int rs_conv2d_fwd_upsampled_wino(const rs_conv_desc* d, const float* src1, const float* src2, const float* u, float* out,
                                 rs_stream_t stream);
/* The DATA gradient of that DecoderBlock (autograd of unet.py:63-73 under tools/train.py:186) in the same Winograd machinery: the
 * 4x4 / stride-2 convolution over dz is four 2x2 correlations over dz's parity planes that accumulate into one source-resolution
 * tile, each of them the forward's parity item on its plane -- 9/16 of rs_conv2d_fwd_dt's multiply-adds on that launch.
 * `d` = the FORWARD layer's descriptor (as for rs_conv2d_fwd_phase_wino); dz [N][2 Hs][2 Ws][Cout] fp32; `u` = [4][9][C1+C2][Cout]
 * from rs_pack_wino_dgrad_weight(wd = [C1+C2][4][4][Cout] of rs_combine_dgrad_phase_weight_dt); result d cat[skip, prev]
 * [N][Hs][Ws][C1+C2] in `out`, or split at channel `csplit` (% 64 == 0) into `out` [..][csplit] and `out2` [..][C1+C2-csplit]
 * (torch.cat's backward fused into the store; out2 = NULL, csplit = 0: one tensor); `mask` / `mask2`: optional tensors shaped like
 * their destination, the result is zeroed where they are <= 0 (the ReLU of the layer that produced skip / prev).
 * rs_conv2d_dgrad_phase_wino_ok: 1 if this form runs the layer's gradient (>= 8 tiles per image side, C1 + C2 a multiple of 64,
 * Cout % 16 == 0, 32-bit offsets) -- geometry only, never N; else use rs_conv2d_fwd_split_dt / rs_conv2d_fwd_dt on the 4x4 form. */
int rs_conv2d_dgrad_phase_wino_ok(const rs_conv_desc* d);
const char* rs_conv2d_dgrad_phase_wino_name(const rs_conv_desc* d);
int rs_pack_wino_dgrad_weight(const float* wd4x4, float* u, int Cin, int Cout, rs_stream_t stream);
int rs_conv2d_dgrad_phase_wino(const rs_conv_desc* d, const float* dz, const float* u, float* out, const float* mask, float* out2,
                               const float* mask2, int csplit, rs_stream_t stream);

/* The stride-1 3x3 / pad-1 convolutions of the fp32 predict path -- Bottleneck.conv2 (torchvision resnet50 via unet.py:94,
 * 122-130) with its eval-mode BatchNorm folded into scale / shift, and dec5's ConvRelu (unet.py:32-44,139) -- as a Winograd
 * F(2x2, 3x3) convolution: 16 multiplies per 2x2 outputs instead of 36 (conv_wino33_f32.hip).  `d`: kh = kw = 3, stride 1,
 * pad 1, ups 0, C2 = 0, Ho = Hs, Wo = Ws; out = relu?(conv(src) * scale + shift), scale / shift optional.  `u` = [16][Cout][Cin]
 * from rs_pack_wino33_weight(KRSC fp32 weight).  rs_conv2d_wino33_ok: 1 if this form runs `d` (H, W >= 15, Cin % 16 == 0 and
 * >= 32, Cout % 16 == 0): a function of the layer's geometry only, never of N (see rs_conv2d_phase_wino_ok). */
int rs_conv2d_wino33_ok(const rs_conv_desc* d);
const char* rs_conv2d_wino33_name(const rs_conv_desc* d);
int rs_pack_wino33_weight(const float* w_krsc, float* u, int Cout, int Cin, rs_stream_t stream);
int rs_conv2d_fwd_wino33(const rs_conv_desc* d, const float* src, const float* u, const float* scale, const float* shift, float* out,
                         rs_stream_t stream);
/* dec5 + self.final (+ softmax / quantise / argmax) of the fp32 predict path in ONE launch (reference unet.py:139-141:
 * `dec5 = self.dec5(dec4); return self.final(dec5)`; tools/predict.py:87-103; tools/serve.py:160-164): rs_conv2d_fwd_wino33 on
 * a 32-cout layer whose block keeps its 32 channels on the CU, applies the 1x1 convolution final_w [C][32] + final_b [C] (C <= 8)
 * and then does what rs_final_conv1x1_dt (mode 0 logits / 1 softmax -> `out` fp32 NCHW [N][C][H][W]),
 * rs_final_conv1x1_quantize_dt (mode 2 -> `qout`, needs `anchors` and `overlap`) or rs_final_conv1x1_argmax_dt (mode 3 ->
 * `qout` [N][H][W]) do with a pixel's logits -- same operations in the same order; the logits themselves differ from the
 * two-launch form by fp32 summation order over the 32 channels.  The layer's own output is never written (537 MB per
 * bs-16 512^2 batch that the two-launch form writes and reads back).  rs_conv2d_wino33_head_ok: 1 if this form runs `d`
 * with C classes (rs_conv2d_wino33_ok, Cout == 32, 1 <= C <= 8). */
int rs_conv2d_wino33_head_ok(const rs_conv_desc* d, int C);
const char* rs_conv2d_wino33_head_name(void);
int rs_conv2d_fwd_wino33_head(const rs_conv_desc* d, const float* src, const float* u, const float* scale, const float* shift,
                              const float* final_w, const float* final_b, int C, int mode, const double* anchors, int overlap,
                              float* out, uint8_t* qout, rs_stream_t stream);
/* The tail of a layer1 Bottleneck and the head of the next one in ONE launch, fp32 eval mode (torchvision Bottleneck.forward under
 * reference unet.py:127; round 6, bottleneck_tail_f32.hip):
 *     out = relu(conv1x1(x; w3) * scale3 + shift3 + identity)     x [M][C1], w3 [Cmid][C1], identity / out [M][Cmid]
 *     z   = relu(conv1x1(out; w1) * scale1 + shift1)              w1 [C2][Cmid], z [M][C2]
 * (the folded BatchNorms of rs_bn_fold).  The second product reads the first one's accumulator registers: `out` is written once and
 * never read back.  C1 = 64, Cmid = 256, C2 = 64 (layer1's widths), M % 32 == 0; anything else: RS_EINVAL (the caller then runs the two
 * rs_conv2d_fwd launches). */
int rs_bottleneck_tail_f32(const float* x, const float* w3, const float* scale3, const float* shift3, const float* identity,
                           const float* w1, const float* scale1, const float* shift1, float* out, float* z, long M, int C1, int Cmid,
                           int C2, rs_stream_t stream);
/* The same kernel's first stage alone: out = [relu](conv1x1(x; w) * scale + shift [+ residual]), C1 = 64 -> Cout = 256, M % 32 == 0 -- layer1's
 * downsample convolution (97 against 109 us at bs 16 / 512^2; with a residual the generic launch is the faster one); `residual` may be NULL.  Same sums in
 * the same order as the chained form's `out`. */
int rs_conv1x1_wave_f32(const float* x, const float* w, const float* scale, const float* shift, const float* residual, int relu, float* out,
                        long M, int C1, int Cout, rs_stream_t stream);
/* The same layers in the TRAIN-mode forward (torchvision Bottleneck.conv2 -> BatchNorm2d under tools/train.py:169, fp32): the raw
 * convolution output plus the per-block partial sums of the BatchNorm statistics (sum y, sum y^2 over the block's pixels, in a fixed
 * order), `stats` [rs_conv2d_wino33_stats_rows(d)][2][Cout] fp32 -- the input of rs_bn_finalize_stats, as rs_conv2d_fwd_bnstats_dt's
 * rows are.  `d` / `u` as for rs_conv2d_fwd_wino33 (rs_conv2d_wino33_ok decides; d->relu ignored). */
long rs_conv2d_wino33_stats_rows(const rs_conv_desc* d);
int rs_conv2d_fwd_wino33_stats(const rs_conv_desc* d, const float* src, const float* u, float* out, float* stats, rs_stream_t stream);
/* The DATA gradient of such a layer in the same form (round 6): `d` describes the gradient's convolution (3x3 / stride 1 / pad 1 over
 * dy; C1 = dy's channels, Cout = the gradient's, Cout % 32 == 0), `u` = rs_pack_wino33_weight of rs_pack_dgrad_weight's filters.  The
 * gradient arrives at a ReLU output -- `mask` (the forward activation) or `mask_bits` (rs_bn_apply_bits_dt's; Cout % 8 == 0) or
 * neither -- and, with `stats` [rs_conv2d_wino33_stats_rows(d)][2][Cout], at a BatchNorm output: the per-block partial sums
 * (sum g, sum g * (bn_y - bn_mean) * bn_invstd) of the masked gradient g, rs_bn_bwd_from_partials_dt's input.  Replaces
 * rs_conv2d_dgrad_bnstats[_bits]_dt / rs_conv2d_fwd(relu_mask) on these layers in fp32 (autograd of torchvision Bottleneck.conv2 and of
 * ConvRelu, robosat/unet.py:28-41, under tools/train.py:186) at 4/9 of the multiply-adds. */
int rs_conv2d_dgrad_wino33(const rs_conv_desc* d, const float* dy, const float* u, const float* mask, const uint8_t* mask_bits,
                           const float* bn_y, const float* bn_mean, const float* bn_invstd, float* out, float* stats,
                           rs_stream_t stream);

/* ... and its data gradient: d loss / d (pre-upsample input) is ONE 4x4 / stride-2 / pad-1 convolution over dz with
 * pre-summed taps (rs_conv2d_fwd[_bf16] with kh = kw = 4 and these weights, [Cin][4][4][Cout]): the gradient lands at
 * the source resolution with 4/9 of the multiply-adds and the 2x2 sum of interpolate's backward already inside;
 * rs_cat_split_bwd_dt then only splits torch.cat's channels, applies the ReLU masks and accumulates (rs_upsample2x_bwd
 * without the 2x2 sum). */
int rs_pack_dgrad_phase_weight_dt(const float* w_krsc, void* out, int dtype, int Cout, int Cin, rs_stream_t stream);
/* bf16 compute copies of MANY convolution weights in one launch -- what rs_cast_f32_to_bf16 + rs_pack_dgrad_weight_bf16
 * produce per tensor, bit for bit (the per-step re-cast of the fp32 master weights after Adam.step, robosat/tools/
 * train.py:188; the reference has no counterpart: it computes in fp32).  `items_dev` is a DEVICE array of n items ordered
 * by tile_begin; item i covers tiles [tile_begin_i, tile_begin_i + taps * ceil(Cin/32) * ceil(Cout/32)); total_tiles = their
 * sum.  cast / dgrad may be NULL. */
typedef struct rs_wprep_item {
  const float* w; /* fp32 KRSC [Cout][taps][Cin] */
  rs_bf16* cast;  /* bf16 KRSC copy, or NULL */
  rs_bf16* dgrad; /* bf16 [Cin][taps, flipped][Cout] (the layout of rs_pack_dgrad_weight_bf16), or NULL */
  int Cout, taps, Cin;
  int tile_begin;
} rs_wprep_item;
int rs_weight_prep_bf16(const rs_wprep_item* items_dev, int n, int total_tiles, rs_stream_t stream);
/* The fp32 twin: every item's `dgrad` points at a FLOAT buffer [Cin][taps, flipped][Cout] (the layout of rs_pack_dgrad_weight),
 * `cast` must be NULL (the fp32 KRSC master is its own compute copy): the data-gradient weights of a whole fp32 training step
 * (tools/train.py:180-188 in the reference's arithmetic) in one launch instead of one per convolution. */
int rs_weight_prep_f32(const rs_wprep_item* items_dev, int n, int total_tiles, rs_stream_t stream);
/* The same weights from the already transposed, tap-flipped fp32 weights of rs_pack_dgrad_weight ([Cin][3][3][Cout]):
 * both sides contiguous along Cout (the one-step pack reads with a 9*Cin stride). */
int rs_combine_dgrad_phase_weight_dt(const float* w_dgrad, void* out, int dtype, int Cout, int Cin, rs_stream_t stream);
/* rs_conv2d_fwd with torch.cat's backward fused into the store: output channels [0, csplit) -> out1 (row stride csplit,
 * zeroed where mask1 <= 0 if mask1 != NULL), [csplit, Cout) -> out2 (row stride Cout - csplit, mask2); csplit must be a
 * multiple of the tile's cout width (64 | 128 for these layers). */
int rs_conv2d_fwd_split_dt(const rs_conv_desc* d, int dtype, const void* src1, const void* weight, void* out1, const void* mask1,
                           void* out2, const void* mask2, int csplit, rs_stream_t stream);
int rs_cat_split_bwd_dt(const void* dcat, void* d1, void* d2, const void* mask1, const void* mask2, int dtype, int N, int H,
                        int W, int C1, int C2, int accumulate1, rs_stream_t stream);
/* out[n][2a][2b][:] += t[n][a][b][:] (t [N][Hs][Ws][C], out [N][Ho][Wo][C], Ho >= 2 Hs - 1; fp32: C % 4 == 0, bf16: C % 8 == 0): the
 * data gradient of a 1x1 / stride-2 convolution -- torchvision Bottleneck.downsample[0] of layer2..layer4 under loss.backward(),
 * tools/train.py:186 -- is rs_conv2d_fwd of its transposed filters on the low-resolution grid, added here onto the even positions
 * of the gradient the tensor already has (round 6; replaces the zero-insertion form, ups = 2, of that launch). */
int rs_scatter_add_stride2_dt(const void* t, void* out, int dtype, int N, int Hs, int Ws, int Ho, int Wo, int C, rs_stream_t stream);

/* The same fusion for BatchNorm's BACKWARD (conv -> bn -> relu read right to left): the data-gradient convolution that
 * produces g = d loss / d z (rs_conv2d_fwd semantics on `dy` with rs_pack_dgrad_weight weights, optional residual,
 * relu_mask = z) also accumulates, per M tile, sum g and sum g * xhat with xhat = (bn_y - bn_mean) * bn_invstd;
 * rs_bn_bwd_from_partials_dt then needs one streaming pass (dy = gamma*invstd*(g - mean(g) - xhat*mean(g*xhat)))
 * instead of rs_bn_bwd's two.  workspace: 64*2*C doubles + 3*C floats. */
int rs_conv2d_dgrad_bnstats_dt(const rs_conv_desc* d, int dtype, const void* dy, const void* weight, const void* residual,
                               const void* relu_mask, const void* bn_y, const float* bn_mean, const float* bn_invstd,
                               void* out, float* stats_partial, rs_stream_t stream);
int rs_bn_bwd_from_partials_dt(const void* g, const void* y, const float* mean, const float* invstd, const float* gamma,
                               void* dy, float* dgamma, float* dbeta, const float* partial, long rows, int dtype, long M,
                               int C, void* workspace, rs_stream_t stream);
/* The ReLU mask as one bit per element (round 2).  autograd's ReLU backward (threshold_backward on the block output of
 * torchvision's Bottleneck, `out = relu(bn3(...) + identity)`) only needs the SIGN of z; the data-gradient epilogue of a
 * bottleneck's conv1 moves four Cout-wide operands (g out, residual gradient, bn_y, z) and is HBM-bound.
 * rs_bn_apply_bits_dt = rs_bn_apply_dt that also writes `bits` (M*C/8 bytes; bit e of byte i: element 8*i + e of `out` is > 0;
 * C must divide 2048, else RS_EINVAL); rs_conv2d_dgrad_bnstats_bits_dt = rs_conv2d_dgrad_bnstats_dt reading those bits
 * instead of z (Cout % 8 == 0).  Same results bit for bit. */
int rs_bn_apply_bits_dt(const void* y, const float* scale, const float* shift, const void* residual, void* out,
                        unsigned char* bits, int dtype, long M, int C, int relu, rs_stream_t stream);
int rs_conv2d_dgrad_bnstats_bits_dt(const rs_conv_desc* d, int dtype, const void* dy, const void* weight, const void* residual,
                                    const unsigned char* relu_mask_bits, const void* bn_y, const float* bn_mean,
                                    const float* bn_invstd, void* out, float* stats_partial, rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * Device-side input / output of `rs predict`: only bytes cross PCIe.
 * ---------------------------------------------------------------------------------------------------------- */

/* Decoded tiles as uint8 HWC [N][H][W][C<=4] -> normalised NHWC4 fp32, i.e. ToTensor + Normalize of the reference's
 * transform chain (tools/predict.py:71: x/255 then (x - mean[c])/std[c], fp32, IEEE division: bit-identical to the
 * host ops) + the stem's layout.  `mean`, `std`: HOST arrays of C floats. */
int rs_u8_to_nhwc4_norm(const uint8_t* img, float* out, const float* mean, const float* std, int N, int H, int W, int C,
                        rs_stream_t stream);

/* self.final + softmax + un-buffer crop + 8-bit quantisation in one pass (tools/predict.py:87,96-103):
 * out[n][y][x][c-1] = uint8(np.digitize(p_c, anchors)) for every non-background class c = 1..C-1 over the central
 * (H-2*overlap) x (W-2*overlap) window, with `anchors` = the 256 float64 values of np.linspace(0, 1, 256) in device memory
 * (1-based bins, 256 wraps to 0 -- the reference's behaviour).  C = 2 is the reference's single-channel PNG payload, byte for
 * byte; C > 2 (the reference asserts a binary model, predict.py:98) stores the same encoding per foreground class,
 * interleaved.  x: NHWC [N][H][W][Cin] of `x_dtype`; w [C][Cin], bias [C]. */
int rs_final_conv1x1_quantize_dt(const void* x, int x_dtype, const float* w, const float* bias, const double* anchors,
                                 uint8_t* out, int N, int H, int W, int Cin, int C, int overlap, rs_stream_t stream);

/* self.final + argmax over the classes -> one byte per pixel: Predictor.segment of `rs serve`
 * (tools/serve.py:160-164: output.argmax(axis=0).astype(np.uint8); first maximum on ties). */
int rs_final_conv1x1_argmax_dt(const void* x, int x_dtype, const float* w, const float* bias, uint8_t* out, int N, int H,
                               int W, int Cin, int C, rs_stream_t stream);

/* Dihedral test-time augmentation (csrc/tta.hip; an extension, the reference has none).  A mode is an ordered list of V ops
 * ops[v] in the encoding of rs_augment_tiles, op = f + 2*k: FLIP_LEFT_RIGHT when f, then k counter-clockwise 90-degree
 * rotations (np.rot90).  g_v maps tile pixel p to its position in view v; view v of tile n sits at batch index n*V + v.
 * V is 1, 2, 4 or 8; `ops` is a HOST array of V ints; H, W are multiples of 32; ops with odd k need H == W.
 *
 * rs_tta_fan_out: view_v[q] = tile[g_v^-1(q)] -> out [N*V][H][W][4] NHWC4 of `out_dtype` (RS_F32 or RS_BF16, round to nearest
 * even), channels >= C zero.  x_kind RS_TTA_IN_U8: x = uint8 HWC [N][H][W][C<=4] normalised as rs_u8_to_nhwc4_norm (mean,
 * std: HOST arrays of C floats); RS_TTA_IN_F32: x = fp32 NCHW [N][C][H][W] taken as it is (rs_nchw_to_nhwc4; mean, std
 * unused).  Bit-identical to transforming the tile first and then calling those ops.
 *
 * rs_tta_merge: probs = the N*V views' fp32 NCHW [N*V][C][H][W] probabilities (16-byte aligned).  For each output pixel p and class c the V
 * values probs_v[c][g_v(p)] are sorted ascending, added in fp32 one after another from the smallest, and multiplied by 1/V
 * (exact).  The summands of g(x) at g(p) are the same multiset as those of x at p for every g of a mode that is a group, so
 * the merge is exactly equivariant: tta(g.x) == g.tta(x) bit for bit, given a batch-independent network.  Then by `mode`:
 *   RS_TTA_PROBS     out = fp32 [N][C][H][W], uncropped;
 *   RS_TTA_QUANTIZE  out = uint8 of rs_final_conv1x1_quantize_dt's layout and encoding ([N][H'][W'] for C = 2,
 *                    [N][H'][W'][C-1] for C > 2, H' = H - 2*overlap; `anchors` = np.linspace(0, 1, 256) in device memory);
 *   RS_TTA_ARGMAX    out = uint8 [N][H][W], the first maximum over the classes of the merged probabilities.
 * Neither kernel uses atomics; the results are deterministic. */
#define RS_TTA_IN_U8 0
#define RS_TTA_IN_F32 1
#define RS_TTA_PROBS 0
#define RS_TTA_QUANTIZE 1
#define RS_TTA_ARGMAX 2
int rs_tta_fan_out(const void* x, int x_kind, const float* mean, const float* std, void* out, int out_dtype, const int* ops,
                   int V, int N, int H, int W, int C, rs_stream_t stream);
int rs_tta_merge(const float* probs, const int* ops, int V, int mode, const double* anchors, int overlap, void* out, int N,
                 int C, int H, int W, rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The callers either side of the network, on the device (csrc/postproc.hip)
 * ---------------------------------------------------------------------------------------------------------- */

/* Metrics.add generalised to C classes (robosat/metrics.py:27-41; its Todo at :87-88): counts[actual * C + predicted] += 1
 * per pixel, predicted = argmax over the C scores (first maximum).  counts: int64 [C*C] in device memory, accumulated.
 * For C = 2 the reference's counters are tn = counts[0], "fn" = counts[1], "fp" = counts[2], tp = counts[3].  C <= 8. */
int rs_confusion_matrix(const float* scores, const int64_t* targets, int64_t* counts, int N, int C, int H, int W,
                        rs_stream_t stream);

/* np.bincount over label tiles (robosat/tools/weights.py:41-47): counts256[v] += number of labels equal to v.
 * labels: n bytes in device memory, 16-byte aligned; counts256: int64 [256], accumulated. */
int rs_label_histogram_u8(const uint8_t* labels, long n, int64_t* counts256, rs_stream_t stream);

/* `rs masks` (robosat/tools/masks.py:42-84): K models' quantised probabilities q [K][P][C-1] (the bytes rs predict writes)
 * -> class index per pixel: np.argmax(np.average(probs, axis=0, weights), axis=0) with probs_k = [1 - sum_c f_c, f_1, ..],
 * f_c = anchors[q]; float64, models accumulated in order, first maximum.  weights: K doubles in device memory or NULL. */
int rs_softvote_masks(const uint8_t* q, const double* weights, const double* anchors, uint8_t* out, int K, long P, int C,
                      rs_stream_t stream);

/* `rs masks --threshold T`, binary models only: q [K][P], the same un-quantisation and weighted average as rs_softvote_masks
 * (float64, models accumulated in order), then out[p] = voted foreground >= T in place of the argmax:
 * np.average(anchors[q], axis=0, weights) >= T.  threshold: T, one double in HOST memory, read before the call returns (every
 * value the ABI passes by value is an int, a long or a float, and T must arrive as the float64 it is); 0 < T <= 1, RS_EINVAL
 * otherwise.  With one model and T = anchors[k] the mask is `byte >= k`, the operating point k of `rs evaluate --probs`. */
int rs_softvote_masks_threshold(const uint8_t* q, const double* weights, const double* anchors, uint8_t* out, int K, long P,
                                const double* threshold, rs_stream_t stream);

/* Training-set augmentation from a cache of decoded tiles in HBM (robosat/tools/train.py:248-260,
 * robosat/transforms.py:127-221): for batch item n take tile index[n] of images [T][S][S][C] (uint8 HWC) / masks [T][S][S],
 * apply op[n] = f + 2*k (PIL FLIP_LEFT_RIGHT when f, then k x ROTATE_90), ToTensor + Normalize ((v/255 - mean)/std, fp32),
 * and write what the reference's loader yields: images NCHW fp32 [N][C][S][S], masks int64 [N][S][S].
 * mean / std: HOST arrays of C floats.  masks / out_masks may be NULL together. */
int rs_augment_tiles(const uint8_t* images, const uint8_t* masks, const int32_t* index, const int32_t* op, const float* mean,
                     const float* std, float* out_images, int64_t* out_masks, int N, int S, int C, rs_stream_t stream);

/* Zoom and colour jitter on top of the eight views (csrc/augment.hip; an extension, the `[augment]` table of `rs train`).
 *
 * rs_tile_band_sums: sums[t][c] = the sum of band c of tile t of images [T][S][S][C] (uint8 HWC, C <= 4, any base address),
 * int64 [T][C], overwritten.  Integer arithmetic only: every run gives the same bits.
 *
 * rs_augment_tiles_jitter: rs_augment_tiles with, per batch item n, a square window geom[n] = (w, x0, y0) of the source tile
 * that is enlarged to the S x S frame, and the colour factors color[n] = (brightness, contrast, saturation, gamma).  geom and
 * color are HOST arrays like mean / std ([N][3] and [N][4]); index, op and band_sums (the sums above, of the same `images`)
 * are device arrays.  op[n] is undone first, as in rs_augment_tiles, giving (y, x) in the frame; per axis, frame index j reads
 *   mask (nearest):   source index x0 + ((2j+1)*w) / (2S), integer division;
 *   image (bilinear, half-pixel centres): t = max((2j+1)*w - S, 0), i0 = t / (2S), f = float(t % (2S)) / float(2S),
 *                     i1 = min(i0 + 1, w - 1), taps x0 + i0 and x0 + i1; per band on the bytes as floats
 *                     top = a + fx*(b - a), bot likewise, v = top + fy*(bot - top)   (w = S: i0 = j, f = 0, the byte itself).
 * Then v = v / 255 and, in fp32, each stage whose factor is not exactly 1.0f, each followed by a clamp to [0, 1]:
 *   brightness v*b;  contrast m_c + k*(v - m_c), m_c = sums[tile][c] / (S*S*255) (float64 quotient rounded to fp32);
 *   saturation g + s*(v - g) on bands 0..2 with g = 0.299f*R + 0.587f*G + 0.114f*B, only when `rgb` is set;  gamma powf(v, gamma).
 * Then (v - mean[c]) / std[c].  All factors 1.0f and w = S: the bits of rs_augment_tiles.
 * RS_EINVAL: C > 4, S > 16384, w outside [1, S], a window that leaves the tile (x0, y0 outside [0, S - w]), `rgb` with C < 3,
 * a contrast factor other than 1.0f without band_sums.  masks / out_masks may be NULL together. */
int rs_tile_band_sums(const uint8_t* images, int64_t* sums, int T, int S, int C, rs_stream_t stream);
int rs_augment_tiles_jitter(const uint8_t* images, const uint8_t* masks, const int32_t* index, const int32_t* op,
                            const int32_t* geom, const float* color, const int64_t* band_sums, const float* mean,
                            const float* std, float* out_images, int64_t* out_masks, int N, int S, int C, int rgb,
                            rs_stream_t stream);

/* Free rotation on top of the zoom (`[augment] rotate`): rs_augment_tiles_jitter with the window of item n turned about its
 * centre by the angle whose cosine and sine are rot[n] = (c, s) in units of 2^-16 (HOST array [N][2], like geom), the content
 * counter-clockwise as displayed for a positive angle (the sense of np.rot90).  op[n] is undone first, giving (x, y) in the
 * frame, so the rotation acts on the window and the flip and quarter turns come last.  All in 64-bit integers:
 *   A  = floor((2*c*w + S) / (2*S))        B = floor((2*s*w + S) / (2*S))      (once per item, on the host)
 *   dx = 2x + 1 - S                        dy = 2y + 1 - S
 *   Ux = A*dx - B*dy + (2*x0 + w)*65536    Uy = B*dx + A*dy + (2*y0 + w)*65536
 * (Ux, Uy) is where the pixel's centre falls in the source tile, in units of 2^-17 pixels.  With >> the arithmetic shift:
 *   mask:   the label at (fold(Ux >> 17), fold(Uy >> 17));
 *   image:  per axis i0 = (U - 65536) >> 17, i1 = i0 + 1, weight of the second tap f = float((U - 65536) & 131071) / 131072
 *           (exact), taps fold(i0) and fold(i1), interpolated as above: top = a + fx*(b - a), v = top + fy*(bot - top);
 *   fold(i) = -1 - i for i < 0, 2S - 1 - i for i >= S, i otherwise: the tile mirrored about its edges, the edge pixel repeated.
 * The taps are NOT clamped to the window: a turned window reads its true neighbours in the tile, and past the tile the mirror,
 * image and mask alike.  One fold is enough: the window lies in the tile, so no sample is further than 0.21 S outside.  The
 * colour stages and the normalisation are rs_augment_tiles_jitter's, on the interpolated value; the contrast stage's band means
 * stay those of the whole source tile.  A and B are rounded to 2^-16, so a sample sits at most S * 2^-17 pixels from the ideal
 * rotation; the quantised map is the definition.  (c, s) = (65536, 0) with w = S reads every byte itself (f = 0), and the quarter
 * turns (0, +-65536), (-65536, 0) are np.rot90 exactly.
 * RS_EINVAL: as rs_augment_tiles_jitter, and |c| or |s| above 65536, or |c*c + s*s - 2^32| above 2^17 (the two roundings move the
 * sum by 92 700 at the most): a pair that is no rotation is refused before it can address memory. */
int rs_augment_tiles_rotate(const uint8_t* images, const uint8_t* masks, const int32_t* index, const int32_t* op,
                            const int32_t* geom, const int32_t* rot, const float* color, const int64_t* band_sums,
                            const float* mean, const float* std, float* out_images, int64_t* out_masks, int N, int S, int C,
                            int rgb, rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * `rs features` (robosat/tools/features.py, robosat/features/core.py): the raster stages on the device
 * (csrc/features.hip).  Batched over B tiles of equal H x W, 1 <= H, W <= 4096, B <= 65535,
 * B*H*W < 2^29 (so the edge count, at most 4 per pixel, fits the int32 counter); RS_EINVAL otherwise.
 * ---------------------------------------------------------------------------------------------------------- */

/* disc(eps): eps x eps 0/1 matrix, r = c = eps / 2; row i (dy = i - r) has dx = rint(c * sqrt((r*r - dy*dy) / (r*r))) and
 * columns max(c - dx, 0) .. min(c + dx + 1, eps) - 1 set (OpenCV's documented MORPH_ELLIPSE); S = {(i - r, j - c)} its offsets.
 * erode(m)[p] = AND over s in S of m[p + s], outside the tile 1; dilate(m)[p] = OR over s in S of m[p - s], outside 0 (the
 * reflected set: open(m) <= m <= close(m) and both idempotent for even eps too, where OpenCV anchors both at the same corner).
 * rs_features_clean: out = close(open(images == index)) as 0/1 bytes [B][H][W]; open = dilate(erode) with disc(eps_open),
 * close = erode(dilate) with disc(eps_close); eps 0 or 1 = identity, eps <= 64.  dx_open / dx_close: HOST arrays of eps ints, the
 * rows' dx above.  form 1: bit-planes resident in LDS, one workgroup per tile (needs rs_features_clean_form(H, W) == 1, i.e. two
 * planes of H * ceil(W/32) words within 160 KB); form 2: planes in `workspace` (rs_features_clean_workspace_bytes; may be NULL
 * for form 1), one launch per pass; form 0: the library's choice (form 2: profiles/features).  Both forms give the same bytes. */
int rs_features_clean_form(int H, int W);
long rs_features_clean_workspace_bytes(int B, int H, int W);
int rs_features_clean(const uint8_t* images, uint8_t* out, void* workspace, int B, int H, int W, int index, int eps_open,
                      const int32_t* dx_open, int eps_close, const int32_t* dx_close, int form, rs_stream_t stream);

/* 4-connected components of masks != 0: labels [B][H][W] int32, background 0, a component's label = 1 + min(y * W + x) over its
 * pixels (canonical: independent of the order the device worked in).  Lock-free union-find; no workgroup waits for another and
 * every loop is bounded by H*W.  *err (int32 in device memory, zeroed by the caller) is set non-zero should a bound run out. */
int rs_features_label(const uint8_t* masks, int32_t* labels, int32_t* err, int B, int H, int W, rs_stream_t stream);

/* Component table: one row [tile, label, area, x0, y0, x1, y1] (pixel count, inclusive bounding box) per component with
 * area >= min_area, in no particular order.  counters (int32 [2], device): [0] = components found, [1] = rows kept; rows are
 * written only below `capacity` (call again with capacity >= counters[0] if it was exceeded).  slotmap: int32 [B][H][W]
 * scratch; raw: int32 [capacity][6] scratch; table: int32 [capacity][7]. */
int rs_features_components(const int32_t* labels, int32_t* slotmap, int32_t* raw, int32_t* table, int32_t* counters,
                           long capacity, int B, int H, int W, int min_area, rs_stream_t stream);

/* Boundary edges of the components listed in `table` (`rows` rows as above): a pixel (x, y) of label L emits one directed unit
 * edge per 4-neighbour whose label is not L (outside the tile counts), walking round the pixel with the pixel on the right --
 * dir 0 top (x,y)->(x+1,y), 1 right (x+1,y)->(x+1,y+1), 2 bottom (x+1,y+1)->(x,y+1), 3 left (x,y+1)->(x,y).  Rows
 * [tile, label, x, y, dir] int32 in no particular order; *counter (int32, device) = number of edges, rows written only below
 * `capacity` (capacity 0, edges NULL: count only).  keep: B*H*W bytes of scratch. */
int rs_features_edges(const int32_t* labels, const int32_t* table, long rows, uint8_t* keep, int32_t* edges, long capacity,
                      int32_t* counter, int B, int H, int W, rs_stream_t stream);

/* ---- stitched form: every tile of a call is part of one sparse raster (`rs features --stitch`) ----
 * A call holds T tiles of equal H x W in slot order (the host sorts them by z, x, y); tile (x, y) covers mosaic pixels
 * [x*W, (x+1)*W) x [y*H, (y+1)*H), and every pixel no present tile covers is "not the class" for every stage.  Two host tables
 * describe the layout: nbr int32 [T][8], the slot of the neighbour to the NW, N, NE, W, E, SW, S, SE or -1 (an entry outside
 * 0..T-1 reads as -1); origin int32 [T][2], the tile's (X, Y) offset in mosaic pixels from the call's smallest x and y.  The
 * stages then give what the per-tile stages above give on that one large raster:
 *
 * halo (crop = 0): dst [T][H+2A][W+2A] = the tile with an apron of A pixels taken from its 8 neighbours, `fill` (0..255, a byte that
 * is not the class) where a neighbour is absent; run the unchanged clean on it as T tiles of (H+2A) x (W+2A), then
 * halo (crop = 1): dst [T][H][W] = the centres of src [T][H+2A][W+2A] (nbr may be NULL).  A = eps_open + eps_close (an eps of 0 or 1
 * counting 0) is enough: an erode or dilate with disc(eps) reads at most eps/2 pixels away, so open then close reads at most
 * 2*(eps_open/2) + 2*(eps_close/2) <= A pixels away, and the clean's "outside the tile = 1" rule, which is wrong only at the
 * padded border, spoils apron pixels only.  RS_EINVAL for A > min(H, W) (one step in nbr must reach the whole apron), for H+2A or
 * W+2A above 4096 and for T*(H+2A)*(W+2A) >= 2^29.
 *
 * stitch_labels: labels [T][H][W] as the per-tile labeller left them -> in place, the labels of the large raster in the global
 * index space g = slot*H*W + y*W + x: components are joined across every right and down seam whose two tiles are present (never
 * across a corner), and every pixel gets 1 + min(g) over its whole component: canonical, whatever order the device worked in.
 * Same union-find as the labeller (lock-free, no workgroup waits, loops bounded by T*H*W, *err as there).
 *
 * components_stitched: rows [label, area, X0, Y0, X1, Y1], the area of the whole component against min_area, the box in mosaic
 * pixels (inclusive); counters, capacity and scratch as in the per-tile call (slotmap int32 [T][H][W], raw [capacity][6],
 * table [capacity][6]).
 *
 * edges_stitched: rows [label, X, Y, dir] in mosaic pixels of the components listed in `table` (rows of 6 as above).  The
 * 4-neighbour across a seam is the facing pixel of the neighbour tile; an absent tile counts as outside; two pixels of one
 * component either side of a seam emit nothing.  counter, capacity and keep as in the per-tile call. */
int rs_features_halo(const uint8_t* src, uint8_t* dst, const int32_t* nbr, int T, int H, int W, int A, int fill, int crop,
                     rs_stream_t stream);
int rs_features_stitch_labels(int32_t* labels, const int32_t* nbr, int32_t* err, int T, int H, int W, rs_stream_t stream);
int rs_features_components_stitched(const int32_t* labels, const int32_t* origin, int32_t* slotmap, int32_t* raw, int32_t* table,
                                    int32_t* counters, long capacity, int T, int H, int W, int min_area, rs_stream_t stream);
int rs_features_edges_stitched(const int32_t* labels, const int32_t* nbr, const int32_t* origin, const int32_t* table, long rows,
                               uint8_t* keep, int32_t* edges, long capacity, int32_t* counter, int T, int H, int W,
                               rs_stream_t stream);

/* ---- overlap table of two label rasters (`rs features --dedupe`) ----
 * labels_a, labels_b: int32 [pixels] each, canonical labels as rs_features_label or rs_features_stitch_labels write them, 0 =
 * background.  `group` = pixels per independent raster (H*W for per-tile labels, T*H*W for stitched ones; pixels % group == 0),
 * raster = p / group.  One row [raster, label_a, label_b, count] int32 per distinct triple with at least one pixel p where
 * labels_a[p] != 0 && labels_b[p] != 0; count = the number of such pixels; rows in no particular order, and, counts being
 * integers, a pure function of the inputs once sorted.  The pairs are summed in an open-addressing hash table of
 * S = max(16, the power of two >= 2 * capacity) slots in `workspace` (rs_features_overlaps_workspace_bytes(capacity) = 12 * S
 * bytes, 8-byte aligned, zeroed by the call).  counters (int32 [2], device): [0] = distinct triples in the table, counted past
 * `capacity`, rows written only below it; [1] != 0: a probe sequence ran out (the table is full, or 1024 slots in a row are) and
 * pairs were left out.  The rows are complete iff counters[1] == 0 && counters[0] <= capacity.  With counters[1] == 0 alone
 * counters[0] is the exact number of rows: call again with capacity >= counters[0]; with counters[1] != 0 call again with a several
 * times larger capacity.  capacity 0 (rows may be NULL) only counts, in a table of 16 slots.  capacity <= 2^29, pixels < 2^29;
 * RS_EINVAL otherwise.  No workgroup waits for another; the probe loop is bounded by min(S, 1024). */
long rs_features_overlaps_workspace_bytes(long capacity);
int rs_features_overlaps(const int32_t* labels_a, const int32_t* labels_b, void* workspace, int32_t* rows, long capacity,
                         int32_t* counters, long pixels, long group, rs_stream_t stream);

/* ---- per-component sums of probability bytes (`rs features --score`) ----
 * labels: int32 [pixels] as rs_features_label, rs_features_stitch_labels or the instances stage leave them; `group` = pixels per
 * independent raster as in rs_features_overlaps (pixels % group == 0), raster = p / group.  q: uint8 [K][pixels], model k's
 * quantised probability of the one class under extraction at every pixel (the host picks the class's channel), 1 <= K <= 8.
 * table / rows: the components wanted, rows of 7 [tile, label, ...] (stitched == 0) or of 6 [label, ...] (stitched != 0, raster 0),
 * no component twice.  For the component c of row i -- the pixels p of raster tile_i with labels[p] == label_i, i.e. the pixels
 * rs_features_edges draws the polygon around -- and every model k
 *   sums[i][k] = sum over p in c of q[k][p]          (uint64 [rows][K], zeroed by the call, 8-byte aligned)
 * exactly: integers, so the same bits whatever order the device worked in, and for the same raster per tile or stitched.  A sum is
 * at most 2^29 * 255 < 2^37.  The host makes the score of it: sum_k w_k sums[i][k] / (255 * area_i * sum_k w_k), the mean over the
 * component of the probability `rs masks` votes with.  Pixels of components the table does not list add nothing.
 * rowmap: int32 [pixels] scratch: the call fills it with -1 and writes rowmap[raster * group + label - 1] = i for every row (a
 * component's label is 1 + the index of one of its pixels in its raster: so is an instance's, whose core's root keeps
 * L[root] == root + 1); a row whose tile lies outside 0 .. pixels / group - 1 or whose label lies outside 1 .. group is skipped and
 * its sums stay 0.  Two launches; per wave a segmented sum over its 64 consecutive pixels (a run ends where the label changes or a
 * raster begins: two tiles may both hold label 1 either side of that border), the block's four waves merged in LDS, then one 64-bit
 * atomic add per run and model.  No workgroup waits for another; every loop is bounded.  rows == 0 returns at once (table and sums
 * may be NULL).  pixels < 2^29, rows <= pixels; RS_EINVAL otherwise. */
int rs_features_scores(const int32_t* labels, const uint8_t* q, const int32_t* table, long rows, int stitched, int32_t* rowmap,
                       uint64_t* sums, long pixels, long group, int K, rs_stream_t stream);

/* ---- centerlines: skeleton and links (`rs features --geometry centerline`) ----
 * Thinning is the Guo-Hall two-subiteration parallel algorithm (CACM 32(3), 1989).  With p2..p9 = the N, NE, E, SE, S, SW, W, NW
 * neighbours of a set pixel p, a pixel outside the raster reading 0:
 *   C  = (!p2 & (p3|p4)) + (!p4 & (p5|p6)) + (!p6 & (p7|p8)) + (!p8 & (p9|p2))
 *   N1 = (p9|p2) + (p3|p4) + (p5|p6) + (p7|p8),  N2 = (p2|p3) + (p4|p5) + (p6|p7) + (p8|p9),  N = min(N1, N2)
 *   m  = (p2|p3|!p5) & p4 in the first sub-iteration of a pair, (p6|p7|!p9) & p8 in the second
 * and p is deleted iff C == 1, 2 <= N <= 3 and m == 0.  Every pixel of a sub-iteration is judged on the raster as it stood before
 * that sub-iteration (two bit-planes, ping-pong; one launch per sub-iteration over all tiles, no workgroup waits for another), and
 * pairs repeat until a whole pair deletes nothing: the skeleton is a pure function of the mask.  A pair on a converged raster is the
 * identity.
 *
 * rs_features_thin: masks [B][H][W] (non-zero = set) -> `pairs` (1 .. 2^20) pairs of sub-iterations -> out [B][H][W] 0/1 bytes.
 * workspace: rs_features_clean_workspace_bytes(B, H, W) bytes holding the two planes; with resume != 0 the call goes on from the
 * planes an earlier call with the same workspace and shape left (masks is not read and may be NULL).  counters (int32 [2], device):
 * [0] = pixels deleted since the last call with resume == 0, [1] = pixels deleted by this call's last pair: the host enqueues pairs
 * in chunks and stops at counters[1] == 0, whatever the chunk size.  nbr NULL: each of the B tiles is a raster of its own.  nbr
 * int32 [B][8] (the table of rs_features_halo): the tiles are one sparse raster -- the 8-neighbour of a border pixel across a seam or
 * a corner is the facing pixel of the neighbouring tile, 0 where that tile is absent; the result is the definition above applied to
 * that raster (read through nbr at every sub-iteration: thinning has no bounded reach, so no apron would do).  Any W works.
 *
 * rs_features_skeleton_links: the links of skeleton s [B][H][W] (0/1) under `labels` and `table` as rs_features_edges takes them
 * (nbr and origin NULL: per tile, table rows of 7) or as rs_features_edges_stitched does (both given: table rows of 6).  From a
 * set pixel (x, y): dir 0 E to (x+1, y) where set; dir 2 S to (x, y+1) where set; dir 1 SE to (x+1, y+1) where set and neither
 * (x+1, y) nor (x, y+1) is; dir 3 SW to (x-1, y+1) where set and neither (x-1, y) nor (x, y+1) is (a diagonal link only where no
 * orthogonal detour exists: staircase corners stay at degree 2).  The links' connected components are the skeleton's 8-connected
 * components.  A link is emitted, once, by its first pixel where the component of either end is listed in `table`, under the first
 * pixel's label where that is listed and the other's otherwise; a set pixel of a listed component with no set 8-neighbour (no link at
 * either end) emits one row with dir -1.  Rows [tile, label, x, y, dir] (per tile) or [label, X, Y, dir] in mosaic pixels
 * (stitched; a link across a seam is emitted by its first pixel like any other), at most 4 per pixel, in no particular order;
 * counter, capacity and keep as in rs_features_edges. */
int rs_features_thin(const uint8_t* masks, uint8_t* out, void* workspace, const int32_t* nbr, int32_t* counters, int B, int H, int W,
                     int pairs, int resume, rs_stream_t stream);
int rs_features_skeleton_links(const uint8_t* skeleton, const int32_t* labels, const int32_t* nbr, const int32_t* origin,
                               const int32_t* table, long rows, uint8_t* keep, int32_t* links, long capacity, int32_t* counter, int B,
                               int H, int W, rs_stream_t stream);

/* ---- road widths: capped squared Euclidean distance transform (`rs features --width`) ----
 * rs_features_edt: masks m [B][H][W] (non-zero = set), a radius R in 1 .. 128 -> d2 [B][H][W] int32:
 *   an unset pixel gives 0;
 *   a set pixel p gives min(R*R, min over the unset pixels q of the same raster of |p - q|^2), in integer pixel units.
 * Pixels outside the raster are NOT background: nothing is known there, so they are ignored, and a road that runs off the edge keeps
 * its width up to the edge.  A set pixel with no unset pixel within R gives exactly R*R, which reads as "capped".  The cap bounds the
 * reach, which is what makes the stitched form exact.
 *
 * nbr NULL: each of the B tiles is a raster of its own.  nbr int32 [B][8] (the table of rs_features_halo and rs_features_thin): the
 * tiles are one sparse raster -- the result is the definition above on the tiles pasted into a canvas whose other pixels are
 * "unknown" (neither set nor unset): unset pixels of present neighbour tiles count across seams and corners, absent tiles are ignored
 * like the outside.  This needs R <= min(H, W), so that only the 8 neighbours matter: RS_EINVAL otherwise.
 *
 * Two launches over the decomposition
 *   g(x, y)  = the horizontal distance from (x, y) to the nearest unset pixel of row y, capped at R (R where the row has none within
 *              reach; unknown pixels are passed over; g <= 128 fits a byte),
 *   d2(x, y) = min(R*R, min over |dy| <= R of g(x, y + dy)^2 + dy^2), rows outside the canvas skipped,
 * which is exact because of the cap.  The row pass writes g [B][H][W] (a caller-provided byte plane) and looks into the W and E tiles;
 * the column pass reads the N and S tiles' g.  g is only kept for the tiles that are there: column x of a row in an ABSENT N (S) tile is
 * x + 1 + g of the last column of that row in the NW (SW) tile, or W - x + g of the first column in the NE (SE) tile, whichever is
 * present and smaller -- unset pixels of a corner tile count although the tile between is unknown.  Integer only, no atomics, every
 * output written by one thread: bit-reproducible.  Any W and H work (W not a multiple of 32 or 64, H < R and W < R per tile). */
int rs_features_edt(const uint8_t* masks, const int32_t* nbr, uint8_t* g, int32_t* d2, int B, int H, int W, int R, rs_stream_t stream);

/* Width of a line (host, robosat_amd/features.py: line_width): over the line's pixel chain after pruning and before simplification,
 * the per-pixel width is 2*sqrt(d2) - 1; width_px = the median, width_min_px / width_max_px the extremes, rounded to 3 decimals;
 * width_capped = true where any pixel of the chain has d2 == R*R (absent otherwise).  An axis-parallel road of odd width w gives
 * exactly w, one of even width w - 1 (the skeleton runs on one of the two middle rows). */

/* ---- instances: touching objects split by the influence zones of their cores (`rs features --split R`) ----
 * Given a cleaned mask m (non-zero = set), its canonical labels Lm (rs_features_label, or rs_features_stitch_labels for the one raster
 * the tiles form) and a radius R:
 *   seeds  a pixel is a seed pixel iff d2 == R*R in rs_features_edt(m, R): a disc of radius R around it meets no unset pixel.  Pixels
 *          outside the raster and absent tiles are unknown, as the transform defines them: an object cut by the raster's edge is not
 *          eroded from that edge.  The seed mask is labelled the way m is (per tile, or stitched): Ls, 4-connected, a core named
 *          1 + the index of its smallest pixel.
 *   start  L0 = Ls where Ls != 0; on a component of m that holds no seed pixel L0 = Lm (a thin component keeps its label and is never
 *          lost); on the other set pixels L0 = -1 (unassigned); on unset pixels 0.
 *   step   every pixel with L == -1 looks at its 4-neighbours AS THEY STOOD BEFORE THE STEP (Jacobi) in the fixed order N (y - 1),
 *          W (x - 1), E (x + 1), S (y + 1) and takes the label of the first one with L > 0; with none it stays -1.  Nothing else
 *          changes.  A pixel outside the raster reads 0.
 * Steps repeat until no -1 is left.  That always happens: a -1 pixel is 4-connected through m to a seed pixel of its own component,
 * and the frontier comes one pixel nearer with every step.  A pixel takes the label of the core that reaches it first (geodesic
 * influence zones), and a tie is broken by where the neighbours lie, never by the labels' values: stitched labels are numbered
 * differently from the labels of the same pixels on one large raster, and the partition must be the same in both.  The result is a pure
 * function of the mask.  A core's root keeps L[root] == root + 1 and so does a thin component's, and a root belongs to one of them
 * only: rs_features_components*, rs_features_edges* and rs_features_overlaps take the result as it is (rs_features_edges emits an
 * edge wherever the neighbour's label differs, so two instances that touch each get their side of the shared border).
 *
 * rs_features_split_cores: d2 int32 [pixels] (rs_features_edt with radius R, 1 .. 128) -> cores uint8 [pixels] = (d2 == R*R).
 *
 * rs_features_split_seeds: labels = Lm, seed_labels = Ls, both int32 [pixels]; `group` = pixels per independent raster as in
 * rs_features_overlaps (H*W per tile, T*H*W stitched; pixels % group == 0; pixels < 2^29) -> out int32 [pixels] = L0 (out may be
 * labels or seed_labels themselves).  has: `pixels` bytes of scratch, zeroed by the call.  Two launches: the first sets
 * has[raster * group + Lm[p] - 1] = 1 for every seed pixel p (the Lm root of its component; the only racing store, and every racer
 * stores the same byte), the second writes L0, every output by one thread.
 *
 * rs_features_grow: labels int32 [B][H][W] holding L0 or any later state -> `steps` (1 .. 2^20) steps further, in place.
 * workspace: rs_features_grow_workspace_bytes(B, H, W) bytes.  nbr NULL: each of the B tiles is a raster of its own.  nbr int32
 * [B][8] (the table of rs_features_halo): the tiles are one sparse raster -- the 4-neighbour across a seam is the facing pixel of the
 * neighbouring tile and an absent tile reads 0, as in rs_features_edges_stitched.  counters (int32 [2], device, zeroed by the call):
 * [0] = pixels assigned by this call, [1] = pixels still -1 after it.  The host enqueues chunks of steps and stops at
 * counters[1] == 0; the result does not depend on the chunks.  counters[0] == 0 with counters[1] != 0 means the -1 pixels left can
 * never be reached (no raster that rs_features_split_seeds wrote has such pixels): an error for the host to raise, not to spin on.
 *
 * A step reaches one pixel, so K steps on a block of pixels are exact when it is loaded with an apron of K pixels.  A launch takes
 * K steps (the last launch of a call what is left of `steps`): a workgroup loads its 32 x 64 block of a tile with an apron of K
 * pixels into LDS (through nbr, corners included, in the stitched form), leaves at once if the block holds no -1, takes the steps
 * there (a barrier between reading the neighbours and writing the new labels: Jacobi) and writes the block back.  What a step makes
 * of an apron pixel within s pixels of the loaded region's edge after s steps may be wrong; it cannot reach the block within K steps.
 * Launches ping-pong between `labels` and the workspace: an apron is read from the launch's input, which no workgroup of that launch
 * writes (a workgroup that has nothing left to do copies its block across once, and remembers it in a byte of its own in the
 * workspace).  After an odd number of launches the call copies the workspace back.  K = rs_features_grow_config's `fused` (12:
 * profiles/features_split, against the same kernel at K = 1; the knob grow_fused, 1 .. 16, overrides it for measurements), clamped to
 * min(H, W) so that one step in nbr reaches the whole apron.  No workgroup waits for another, every loop is bounded, integers only:
 * bit-identical for every K and every `steps`.  rs_features_grow_config: the block's rows and columns and the K in force. */
int rs_features_split_cores(const int32_t* d2, uint8_t* cores, long pixels, int R, rs_stream_t stream);
int rs_features_split_seeds(const int32_t* labels, const int32_t* seed_labels, uint8_t* has, int32_t* out, long pixels, long group,
                            rs_stream_t stream);
long rs_features_grow_workspace_bytes(int B, int H, int W);
int rs_features_grow_config(int* block_h, int* block_w, int* fused);
int rs_features_grow(int32_t* labels, void* workspace, const int32_t* nbr, int32_t* counters, int B, int H, int W, int steps,
                     rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * `rs evaluate` (robosat_amd/tools/evaluate.py): the counting passes over two rasters (csrc/evaluate.hip).
 * Pixels come in groups of `group` consecutive ones as in rs_features_scores (H*W: one group per tile; the whole call: one group for
 * stitched tiles); pixels % group == 0, 0 < pixels < 2^31, RS_EINVAL otherwise.  G = pixels / group.  All counting is in integers:
 * the same bits in every run, whatever order the device worked in.
 * ---------------------------------------------------------------------------------------------------------- */

/* rs_eval_confusion: predicted, actual: uint8 [pixels] class indices (any address: no alignment is asked for), 2 <= C <= 8.
 *   counts[g][a][p] = the number of pixels of group g with actual == a and predicted == p, for a, p < C   (int64 [G][C][C])
 *   bad[g]          = the number of pixels of group g where either value is >= C; they are counted in no cell   (int64 [G])
 * both set by the call, not added to, 8-byte aligned.  The orientation is M[actual][predicted], as rs_confusion_matrix and
 * robosat_amd/metrics.py have it.
 *
 * rs_eval_boundary: d2_a, d2_b: int32 [pixels], rs_features_edt(m, R) of the two masks with R = D + 1, 1 <= D <= 127 (so that R stays
 * within the transform's 128).  The band of a mask is X_D = { pixel : 1 <= d2 <= D*D }: its set pixels within D pixels, centre to
 * centre, of an unset pixel of the same raster (R = D + 1 keeps the cap (D+1)^2 above D*D: a capped pixel is never in the band).
 *   counts[g] = (|A_D|, |B_D|, |A_D and B_D|) over the pixels of group g   (int64 [G][3], set by the call, 8-byte aligned)
 * from which the host makes the Boundary IoU of Cheng et al. (CVPR 2021), shared / (|A_D| + |B_D| - shared).  One departure from the
 * paper's code, which pads the mask with zeros before it erodes: rs_features_edt lets no distance come from outside the raster or
 * from an absent tile, so a raster edge is NOT a boundary here -- an object cut by the edge has no band along the cut (nothing is
 * known beyond it), and a mask that fills its raster has an empty band.  With stitched transforms (nbr given to rs_features_edt) a
 * seam between two present tiles is interior.
 *
 * One launch each behind the fill of the outputs (one fill for rs_eval_confusion where bad == counts + G*C*C, two otherwise).  A workgroup of 256 threads covers rs_eval_config's block_pixels (4096)
 * consecutive pixels of the call, a thread 16 consecutive ones (16-byte loads where its first address is 16-byte aligned and its run
 * ends within `pixels`, single checked loads otherwise), and walks the groups those pixels lie in: a block may straddle two groups,
 * or hold many small ones.  Per group the counts are merged on chip -- confusion: runs of equal cells within a thread, then one
 * histogram per wave in LDS, then the four waves' sum; boundary: bit counts within a thread, a sum over the wave's lanes, then over
 * the waves -- and one 64-bit atomic add goes out per block, group and non-empty cell: at most C*C + 1, or 3.  No workgroup waits for
 * another; every loop is bounded. */
int rs_eval_config(int* block_pixels);
int rs_eval_confusion(const uint8_t* predicted, const uint8_t* actual, int64_t* counts, int64_t* bad, long pixels, long group, int C,
                      rs_stream_t stream);
int rs_eval_boundary(const int32_t* d2_a, const int32_t* d2_b, int64_t* counts, long pixels, long group, int D, rs_stream_t stream);

/* rs_eval_confusion with an ignore label, C <= ignore <= 255: a pixel whose ACTUAL byte equals `ignore` over a predicted byte that
 * is a class lies in no cell and is counted in ignored[g] (int64 [G], set by the call, 8-byte aligned) instead of bad[g].  A
 * predicted byte >= C is bad whatever lies under it; so is an actual byte >= C other than `ignore`.  One fill where
 * bad == counts + G*C*C and ignored == bad + G, three otherwise. */
int rs_eval_confusion_ig(const uint8_t* predicted, const uint8_t* actual, int64_t* counts, int64_t* bad, int64_t* ignored, long pixels,
                         long group, int C, rs_stream_t stream, int ignore);

/* rs_eval_prob_hist (`rs evaluate --probs`): prob: uint8 [pixels], the probability bytes of ONE class as `rs predict` stores them;
 * actual: uint8 [pixels] labels (any address for both); 2 <= C <= 8, 1 <= cls <= C - 1, ignore = -1 for none, else C <= ignore <= 255.
 * A byte q stands for q / 255 = np.linspace(0, 1, 256)[q], the value `rs masks` and `rs features --score` un-quantise it to.
 * Byte 0 is read as probability 0, as those tools read it: that includes the reference's wrap of p == 1.0 to byte 0
 * (robosat/tools/predict.py quantises with np.digitize, which puts exactly 1.0 behind the last anchor, and the uint8 cast wraps it).
 * This view describes the files as the other tools read them, not what the network meant.
 *   hist[g][pos][q] = the number of pixels of group g with prob == q and (actual == cls) == pos, among the pixels whose label is a
 *                     class (actual < C)                                                                   (int64 [G][2][256])
 *   skipped[g][0]   = the pixels of group g whose label is >= C and not `ignore` (the bad ones)
 *   skipped[g][1]   = the pixels of group g whose label equals `ignore`; neither kind is in a hist cell        (int64 [G][2])
 * both set by the call, not added to, 8-byte aligned; one fill where skipped == hist + G*512, two otherwise.  The shape is
 * rs_eval_confusion's (4096 pixels per workgroup, 16 per thread, the block walks its groups).  Per group: a wave whose pixels all
 * lie in one cell sums its count over the lanes and sends one LDS add; otherwise runs of equal cells within a thread go to the
 * wave's own histogram (32-bit counters: a block holds 4096 pixels) one LDS atomic per run; the four copies are summed per cell
 * and put back to zero by the thread that sums them, and one 64-bit atomic add goes out per block, group and non-empty cell: at
 * most 514.  No workgroup waits for another; every loop is bounded. */
int rs_eval_prob_hist(const uint8_t* prob, const uint8_t* actual, int64_t* hist, int64_t* skipped, long pixels, long group, int C,
                      int cls, int ignore, rs_stream_t stream);

/* rs_eval_centerline (`rs evaluate --centerline RHO`): the buffer method of Wiedemann and Heipke (1998) for road centre lines, on
 * rasters.  skel_p, skel_g: uint8 [B][H][W] skeletons (non-zero = set; rs_features_thin's 0/1 bytes) of the predicted and the actual
 * mask of one class.  nbr NULL: each of the B tiles is a raster and a group of its own, G = B.  nbr int32 [B][8] (the table of
 * rs_features_halo): the tiles are one sparse raster and one group, G = 1.
 *   links    those of rs_features_skeleton_links without its labels and table; every link counts.  From a set pixel (x, y): E to
 *            (x+1, y) where set; S to (x, y+1) where set; SE to (x+1, y+1) where set and neither (x+1, y) nor (x, y+1) is; SW to
 *            (x-1, y+1) where set and neither (x-1, y) nor (x, y+1) is.  A pixel outside the raster or in an absent tile reads 0;
 *            across a seam or a corner the neighbour is the facing pixel of the neighbouring tile.  A link belongs to its first pixel,
 *            and so to that pixel's tile.  E and S links are straight (length 1), SE and SW links diagonal (length sqrt 2); a
 *            skeleton pixel without links has no length.
 *   reach    for a skeleton S and a tolerance rho, 1 <= rho <= 127: near_S(q) = rs_features_edt(complement of S, R = rho + 1)[q]
 *            <= rho*rho: q lies within rho pixels, centre to centre, of a pixel of S on the same raster (0 on S itself; R = rho + 1
 *            keeps the cap above rho*rho, as for the boundary band).  The transform's rules hold as they stand: nothing is known
 *            outside the raster or in an absent tile, so a line beyond the edge matches nothing; with nbr a seam is interior.
 *            d2_to_g is that transform for skel_g, d2_to_p the one for skel_p, both int32 [B][H][W], with the same nbr.
 *   matched  a link of skel_p is matched iff near_{skel_g} holds at both of its end pixels, a link of skel_g iff near_{skel_p}
 *            does; the second end is read through nbr like the skeleton.
 *   counts[g] = (p_straight, p_diag, p_straight_matched, p_diag_matched, g_straight, g_diag, g_straight_matched, g_diag_matched)
 *            over the links of group g   (int64 [G][8], set by the call, not added to, 8-byte aligned)
 * from which the host makes, with len(s, d) = s + d * sqrt 2 in float64 over the sums of all groups, P and G the two lengths and
 * Pm and Gm their matched parts: correctness = Pm / P, completeness = Gm / G, quality = Pm / (P + G - Gm), f1 = their harmonic
 * mean.  The paper measures vector lengths after matching; here both sides are rasters, length is counted in links and matching is
 * judged at link ends.
 *
 * One launch behind the fill of counts.  A thread owns a run of up to 16 consecutive pixels of one ROW (a row is cdiv(W, 16) runs; a
 * workgroup of 256 threads takes 256 consecutive runs of the call, so it may straddle tiles or hold many small ones) and reads the
 * bytes beside and below them, beyond the tile through nbr; the transforms are read only by threads whose run starts a link (its four
 * rows whole where W is a multiple of 4, else link end by link end).  Per group: bit
 * counts within a thread, a sum over the wave's lanes, the four waves merged in LDS, one 64-bit atomic add per block, group and
 * non-zero counter: at most 8.  No workgroup waits for another; every loop is bounded; integers only.  Any H and W work.
 * RS_EINVAL for rho outside 1..127, B*H*W outside 1 .. 2^31 - 1, a null pointer other than nbr. */
int rs_eval_centerline(const uint8_t* skel_p, const uint8_t* skel_g, const int32_t* d2_to_g, const int32_t* d2_to_p,
                       const int32_t* nbr, int64_t* counts, int B, int H, int W, int rho, rs_stream_t stream);

/* `rs evaluate --type T --ignored unknown`: the typed views beside ignored label pixels.  a is the label raster, p the mask raster,
 * t the class index of --type, I the dataset's ignore value (C <= I <= 255).
 *   U  = {a == I}           the unknown pixels: nothing is known there on either side
 *   P  = {p == t} \ U       the prediction under an ignored label cannot be judged, so it is no part of P
 *   G  = {a == t}
 *   cP = 2 on U, 1 on P, 0 elsewhere; cG likewise with G: the rasters coded UNSET / SET / UNKNOWN.
 * An ignored pixel is what a pixel outside the raster or in an absent tile already is to rs_features_edt, at pixel granularity.
 *   outlines      a side's band is its SET pixels with 1 <= d2 <= D*D, d2 the transform of the coded raster with R = D + 1:
 *                 distances come from UNSET pixels only and pass over unknown ones, and an unknown pixel is in no band.  The edge of
 *                 an ignored region is no boundary, as the raster's edge is none (and as in rs_boundary_weight_plane).  On the device
 *                 the transform is rs_features_edt of the coded plane as it stands (non-zero = set): at a SET pixel its value is the
 *                 definition's; at an unknown pixel it writes a distance where the definition has none, so the count leaves U out
 *                 (rs_eval_boundary_coded).
 *   objects       the 4-connected components of P and of G.  An object that an unknown region cuts is cut on both sides alike, the
 *                 rule that holds at a tile border without --stitch; a predicted object wholly inside U does not exist.  Areas count
 *                 known pixels; --min_area, the overlap table and the matching are as they are.
 *   centre lines  P and G are thinned and rs_eval_centerline counts as it stands.  Both skeletons stop about half a road's width
 *                 short of an unknown region, on both sides alike, and a line beyond it matches nothing.  No pixel of a skeleton
 *                 lies in U, and the reach is looked at at skeleton pixels only, where the transform of the skeleton's complement
 *                 has the same value whether U is coded unknown or "not skeleton" (both are passed over).
 *   probabilities rs_eval_prob_hist leaves ignored labels out already.
 *
 * rs_eval_select: predicted, actual: uint8 [pixels] (any address), 0 < pixels < 2^31, 2 <= C <= 8, 1 <= cls <= C - 1,
 * C <= ignore <= 255 (RS_EINVAL otherwise).  Writes coded_p = cP, coded_g = cG, mask_p = (cP == 1), mask_g = (cG == 1), uint8 [pixels]
 * each (any address).  A byte that is no class and not the ignore value is set on neither side (rs_eval_confusion_ig counts it as
 * bad).  One launch of the shape above, without groups: 16 consecutive pixels per thread, 16-byte loads and stores where the run's
 * first address in that plane is 16-byte aligned and the run ends within `pixels`, single checked accesses otherwise; every output
 * byte has one writer: no atomic, no LDS.  Each input is read once.
 *
 * rs_eval_boundary_coded: rs_eval_boundary over the known pixels.  coded: uint8 [pixels] (any address), cP or cG: U is the same in both.
 *   counts[g] = (|A_D|, |B_D|, |A_D and B_D|) over the pixels of group g whose coded byte is not 2
 * Group walk, merge and atomics are rs_eval_boundary's (the kernels are one template); on a plane without a 2 so are the counts. */
int rs_eval_select(const uint8_t* predicted, const uint8_t* actual, uint8_t* coded_p, uint8_t* coded_g, uint8_t* mask_p, uint8_t* mask_g,
                   long pixels, int C, int cls, int ignore, rs_stream_t stream);
int rs_eval_boundary_coded(const int32_t* d2_a, const int32_t* d2_b, const uint8_t* coded, int64_t* counts, long pixels, long group, int D,
                           rs_stream_t stream);

/* ------------------------------------------------------------------------------------------------------------
 * The optimiser step of `rs train` (csrc/optim.hip; an extension: the `[opt] weight_decay / schedule / clip_norm / ema` keys,
 * robosat_amd/optim.py).  torch.optim.AdamW's update -- Adam's with wd = 0 -- with the learning-rate schedule, gradient clipping by
 * the global norm and an exponential moving average (EMA) of the weights in the one pass that reads and writes every parameter.
 *
 * items   a HOST array of n items, read before the call returns: one per parameter tensor with a gradient.  p, g, m, v and the
 *         optional shadow s (NULL: none) are fp32 device arrays of numel elements in the same memory order, 4-byte aligned (16-byte
 *         aligned items take 16-byte accesses); decay != 0 applies the weight decay to the item.  The items travel by value in
 *         launch-argument blocks of at most RS_OPTIM_ITEMS; one workgroup walks RS_OPTIM_CHUNK elements of one item
 *         (rs_optim_limits exports both).  No device-side table, no allocation, no synchronisation: every call can be captured.
 * ctl     32 bytes of device memory, 8-byte aligned: int64 step (the number of steps taken) at 0, double sumsq at 8, float coef
 *         at 16.
 * table   fp32 [T][4], 16-byte aligned: row t = (a_t, b_t, c_t, d_t) = (lr_t / (1 - beta1^(t+1)), 1 / sqrt(1 - beta2^(t+1)),
 *         1 - lr_t wd, the EMA decay of step t), made by the host in float64 and rounded once.  Step t uses row min(t, T - 1).
 *
 * rs_optim_grad_norm: sumsq = the sum of g^2 over all items in float64 and coef = min(1, clip / (sqrt(sumsq) + 1e-6)) as a float
 * (torch.nn.utils.clip_grad_norm_ with error_if_nonfinite=False; a NaN norm gives a NaN coef), written to ctl.  Per item range,
 * never across the padding between items.  One fp64 partial per chunk in `workspace` (rs_optim_workspace_bytes(total chunks),
 * 8-byte aligned; chunks of an item = ceil(numel / RS_OPTIM_CHUNK)), summed by one block in a fixed order: no float atomics, the
 * same input gives the same bits.  Only g and numel of an item are read.
 *
 * rs_optim_step: with the row of ctl.step and g^ = coef g (use_coef != 0: ctl.coef as rs_optim_grad_norm left it) or g, per element
 *   m' = beta1 m + (1 - beta1) g^,  v' = beta2 v + (1 - beta2) g^ g^,  u = a_t m' / (sqrt(v') b_t + eps),
 *   p' = (decay ? c_t p : p) - u,   s' = d_t s + (1 - d_t) p' where s is given.
 * g is read only.  A one-thread launch behind the element pass then adds 1 to ctl.step.
 *
 * RS_EINVAL: a null (other than s) or misaligned pointer, n <= 0, numel <= 0, T <= 0, a beta outside [0, 1), a non-finite or negative
 * eps or clip. */
typedef struct rs_optim_item {
  float* p;
  const float* g;
  float* m; /* exp_avg */
  float* v; /* exp_avg_sq */
  float* s; /* EMA shadow, or NULL */
  long numel;
  int decay;
  int reserved;
} rs_optim_item;
int rs_optim_limits(int* chunk, int* items);
long rs_optim_workspace_bytes(long total_chunks);
int rs_optim_grad_norm(const rs_optim_item* items, int n, float clip, void* ctl, void* workspace, rs_stream_t stream);
int rs_optim_step(const rs_optim_item* items, int n, const float* table, int T, void* ctl, float beta1, float beta2, float eps,
                  int use_coef, rs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* ROBOSAT_HIP_H */
