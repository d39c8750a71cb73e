/* instageo_hip.h -- C ABI of libinstageo_hip.so: the MI355X (gfx950) hot path of InstaGeo's Prithvi
 * segmentation model (instageo/model).  Plain pointers and sizes only; every pointer is a DEVICE pointer
 * unless stated otherwise; `stream` is a hipStream_t (NULL = default stream).  All functions return 0 on
 * success or a negative IG_ERR_* code and set a thread-local message readable through ig_last_error().
 *
 * The reference has no native interface: the seam is the Python symbol instageo.model.base.PrithviSeg
 * (base.py:28,69-77).  Each entry point below replaces the ATen op(s) that the reference module calls at the
 * cited file:line (paths relative to the reference root); INTEGRATION.md shows the ctypes binding.
 *
 * bf16 tensors: raw uint16 storage.  Every bf16 tensor argument is a pair (x_hi, x_lo): x_lo == NULL selects
 * plain bf16; non-NULL selects the split "bf16x3" precision mode (value = hi + lo, products hi*hi+hi*lo+lo*hi).
 * Either all bf16 operands of a call are split or none.  Activations in the decode head are NHWC.
 * Placement of a split pair (performance only, results are the same up to fp32 summation order): when x_lo lies ABOVE x_hi, 16-byte aligned
 * and less than 4 GiB minus the tensor away -- e.g. both halves of one allocation, which is how the Python host allocates them -- the
 * linear and wide-convolution engines fetch hi and lo with ONE LDS-DMA stream ("paired" K-tiles, 5-35 % faster); any other placement runs
 * the three-pass form of the same products.
 * Conv weights (3x3 and transposed) are stored Wc[Cout][9][Cin], tap = ky*3+kx.
 * Dropout is a counter-based hash of (drop_seed + *drop_seed_dev, element index): backward regenerates the mask;
 * drop_seed_dev (device uint32, may be NULL) lets a captured graph advance the seed without new host arguments.
 */
#ifndef INSTAGEO_HIP_H
#define INSTAGEO_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define IG_OK 0
#define IG_ERR_ARG (-1)
#define IG_ERR_HIP (-2)
#define IG_ERR_UNSUPPORTED (-3)

/* ---- runtime ---------------------------------------------------------------------------------------- */
const char* ig_last_error(void);
/* name of the (last) kernel the most recent MFMA entry point of this thread launched, as rocprofv3 prints it minus
 * "(anonymous namespace)::" and blanks -- bench.py keys its per-kernel roofline table by it */
const char* ig_last_kernel(void);
int ig_note_reset(void); /* forget the name (an entry point without a named kernel then reports "") */
int ig_last_grid(void);  /* workgroups of the last persistent GEMM launch of this thread (see ig_set_reserved_cus) */
int ig_version(void);
/* first 32 bits of the MD5 of this header as the library was built against it: the host mirror refuses a library whose
 * entry points were compiled from a different revision of the declarations (stale .so next to a newer header) */
int ig_header_stamp(void);
int ig_device_info(int device, char* name, int name_len, int* cu_count, int* lds_per_block, long* hbm_bytes);
/* Compute units the persistent kernels (one workgroup per CU) leave free.  Data-parallel training (Lightning DDP in the
 * reference, pipeline_utils.py:368-374) launches RCCL all-reduce kernels beside the backward GEMMs: a grid that pins all
 * 256 CUs serialises them behind a whole GEMM.  Default 0, or the IG_RESERVED_CUS environment variable. */
int ig_set_reserved_cus(int n);
int ig_get_reserved_cus(void);
/* Run-to-run deterministic reductions (the reference's Trainer runs with deterministic=True, pipeline_utils.py:373; float atomics
 * make the bias / norm / head gradients depend on arrival order).  shadow: zeroed int64[n] on the device, paralleling the flat fp32
 * gradient buffer grad_base[n]; while registered, every multi-contributor reduction into that buffer is an INTEGER add of the
 * 2^44-scaled contribution into the shadow (order-independent; one gradient element must stay below 5.2e5 in magnitude), and the
 * BatchNorm statistics are folded from per-workgroup partials in index order; call ig_det_fold(lo, hi) once the gradients of flat
 * range [lo, hi) are complete to add the shadow into them (and clear it).  shadow = NULL switches the mode off.  Not
 * stream-concurrent: call with no kernel of the library in flight, outside captures.  The cross-entropy statistics of ig_ce_loss
 * and the weight gradients of the linears (ordered split-K folds) are order-independent in both modes. */
int ig_set_deterministic(void* shadow, const void* grad_base, long n, void* stream);
int ig_get_deterministic(void);
int ig_det_fold(long lo, long hi, void* stream);
/* the same over n ranges in ONE launch: ranges_dev = DEVICE int64 [n][2] (lo, hi), longest = the longest range (sizes the grid) */
int ig_det_fold_ranges(int n, const long* ranges_dev, long longest, void* stream);

/* ---- dataset side: normalise + layout (instageo/model/dataloader.py:495-524, 707-750) ---------------- */
/* src (B, T*C, H, W) band = t*C+c, src_dtype 0=int16 1=float32 -> dst (B, C, T, H, W) f32 = (src*mult-mean_c)/std_c */
int ig_normalize_chips(const void* src, int src_dtype, const float* mean, const float* stdv, double mult, int mult_enabled,
                       float* dst, int B, int T, int C, int H, int W, void* stream);
/* On-device input pipeline.
 * RandomCrop(im) + hflip/vflip + per-band normalise in one pass (dataloader.py:58-141, 495-585): src (B, T*C, Hs, Ws)
 * int16|f32, params[b] = {top, left, hflip, vflip} (host-drawn, so the reference's RNG stream can be replayed);
 * labels (optional, f32 (B, Hs, Ws) -> (B, im, im)) get the same crop and flips. */
int ig_crop_flip_normalize(const void* src, int src_dtype, const float* mean, const float* stdv, double mult, int mult_enabled,
                           const int* params, float* dst, const float* labels_in, float* labels_out, int B, int T, int C, int Hs,
                           int Ws, int im, void* stream);
/* Sliding-window gather + normalise (process_test / crop_array, dataloader.py:588-669; chip_inference over a tile,
 * BASELINE configs[3]): tile (T*C, Hs, Ws) int16|f32 and origins[i] = {top, left} -> dst (n, C, T, crop, crop) f32 normalised,
 * optionally the same windows of a label tile (Hs, Ws) f32 -> (n, crop, crop).  One launch for all n windows. */
int ig_normalize_windows(const void* tile, int src_dtype, const float* mean, const float* stdv, double mult, int mult_enabled,
                         const int* origins, float* dst, const float* labels_tile, float* labels_out, int n, int T, int C, int Hs,
                         int Ws, int crop, void* stream);
/* Photometric / resampling augmentations of the training pipeline (dataloader.py:144-386) on a raw-domain float32 batch
 * (B, T*C, S, S) -- the output of ig_crop_flip_normalize with identity statistics -- one launch per augmentation and batch.
 * Every random decision is drawn on the host, per chip, like the crop origins.
 * ig_aug_rotate: RandomRotation (dataloader.py:144-187) = Pillow's nearest-neighbour Image.rotate with constant fill;
 *   params[b] = {apply, a0, a1, a2, a3, a4, a5, 0}: the 16.16 fixed-point inverse affine of the drawn angle (host mirror:
 *   dataloader.rotate_coeffs); labels (B, S, S) follow with their own fill.  src != dst.
 * ig_aug_brightness_contrast: RandomBrightnessContrast (dataloader.py:190-260), in place; params[b] = {apply, bright, contrast, 0}.
 * ig_aug_blur: RandomGaussianBlur (dataloader.py:263-333): clip/scale to [0,1], ksize x ksize kernel2d (outer product of the
 *   two normalised 1-D Gaussians) with reflect padding, clamp, * max_pixel, truncate to uint16; apply[b] in {0,1}.  src != dst.
 * ig_aug_noise: RandomGaussianNoise (dataloader.py:336-386), in place; params[b] = {apply, seed}; noise = optional standard-normal
 *   field of buf's shape (else a counter hash + Box-Muller seeded per chip). */
int ig_aug_rotate(const float* src, float* dst, const float* labels_in, float* labels_out, const int* params, float fill,
                  float label_fill, int B, int CT, int S, void* stream);
int ig_aug_brightness_contrast(float* buf, const float* params, float max_pixel, int B, int CT, int S, void* stream);
int ig_aug_blur(const float* src, float* dst, const int* apply, const float* kernel2d, int ksize, float max_pixel, int B, int CT,
                int S, void* stream);
int ig_aug_noise(float* buf, const int* params, const float* noise, float noise_std, float max_pixel, int B, int CT, int S,
                 void* stream);
/* mode=stats reduction (pipeline_utils.py:207-254): sums[c] += mean_bc, sums[C+c] += biased var_bc over (T,H,W) for every
 * chip b of x (B, C, T, H, W) f32; counts[v - lo] += 1 per label value (counts[nbins] = everything else) */
int ig_chip_stats(const float* x, double* sums, int B, int C, long n_per_channel, void* stream);
int ig_label_hist(const float* labels, unsigned long long* counts, long n, int lo, int nbins, void* stream);

/* ---- encoder (instageo/model/pritvhi.py) ------------------------------------------------------------- */
/* Conv3d(k=s=(1,p,p)) im2col: img (B,C,T,H,W) f32 -> patches [B*T*gh*gw][C*p*p], token order (t,row,col)  :243-268 */
int ig_patchify(const float* img, void* out_hi, void* out_lo, int B, int C, int T, int H, int W, int p, void* stream);
/* x[b][0][:] = cls_token + pos_embed[0]                                                        :520-522 */
int ig_cls_rows(float* x, const float* cls, const float* pos, int B, int ntok, int D, void* stream);
/* x[b][1+tp][:] = patches[b*TP+tp] @ w^T + bias + pos_embed[1+tp]                               :266-268,513-517 */
int ig_patch_embed_fwd(const void* p_hi, const void* p_lo, const void* w_hi, const void* w_lo, const float* bias,
                       const float* pos, float* x, int batch, int tokens_per_chip, int D, int K, void* stream);
/* nn.LayerNorm(eps) over D; feat_T>=1 writes the model.py:406-413 feature-image layout [B][G][D*T] (c = d*T+t) */
int ig_layernorm_fwd(const float* x, const float* gamma, const float* beta, void* out_hi, void* out_lo, float* mean,
                     float* rstd, int M, int D, float eps, int feat_T, int feat_G, int ntok, void* stream);
int ig_layernorm_bwd(const void* dy_hi, const void* dy_lo, const float* x, const float* mean, const float* rstd,
                     const float* gamma, float* dx, int accumulate, void* dxb_hi, void* dxb_lo, float* dgamma, float* dbeta,
                     float* dcol, int M, int D, int feat_T, int feat_G, int ntok, void* stream);
/* timm Block linears (qkv / fc1 [+GELU]) : y = act(x @ w^T + b), act 0 none, 1 exact GELU            :446-456
 * act 1 with dact != NULL (training) also stores dact = gelu'(x @ w^T + b), the factor ig_linear_dgrad mode 1 applies */
int ig_linear_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, void* y_hi,
                  void* y_lo, void* dact_hi, void* dact_lo, int M, int N, int K, int act, void* stream);
/* timm Block residual linears (proj / fc2): out = resid + x @ w^T + b (fp32 residual stream)          :446-456 */
int ig_linear_residual_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias,
                           const float* resid, float* out, int M, int N, int K, void* stream);
/* dx = dy @ w  (mode 1: * dact elementwise, the saved gelu'); optional dx_colsum[k] += sum_m dx[m][k] (bias grad of the producing layer);
 * dw += dy^T @ x (fp32 atomics) */
int ig_linear_dgrad(const void* dy_hi, const void* dy_lo, const void* w_hi, const void* w_lo, void* dx_hi, void* dx_lo,
                    const void* dact_hi, const void* dact_lo, float* dx_colsum, int M, int N, int K, int mode, void* stream);
int ig_linear_wgrad(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, float* dw, int M, int N, int K,
                    void* stream);
/* n weight gradients sharing the token count M in ONE launch (the four linears of a timm Block, pritvhi.py:446-456:
 * autograd's grad_weight of F.linear for qkv / proj / fc1 / fc2): dw[g] += dy[g]^T @ x[g].  All array arguments are HOST arrays
 * of n entries; dy_lo / x_lo may be NULL (plain bf16).  Bit-reproducible (ordered split-K fold).  overwrite != 0: dw[g] = dy[g]^T @
 * x[g] -- the first backward of a step then needs neither a zeroed dw nor reads its old contents (4 + 4 bytes per weight less). */
int ig_linear_wgrad_group(int n, const void* const* dy_hi, const void* const* dy_lo, const void* const* x_hi,
                          const void* const* x_lo, float* const* dw, const int* N, const int* K, int M, int overwrite, void* stream);
/* base[lo .. hi) = 0 for n flat ranges in ONE launch: ranges_dev = DEVICE int64 [n][2], longest = the longest range */
int ig_zero_ranges(float* base, int n, const long* ranges_dev, long longest, void* stream);
/* ig_linear_dgrad with the weight handed over TRANSPOSED (wt [K][N] = w^T, see ig_transpose_bf16): same result, but both
 * operands are contiguous in the reduce dimension, the form of the forward linears (dx = dy @ w is autograd's grad_input of
 * F.linear, pritvhi.py:446-456) */
int ig_linear_dgrad_wt(const void* dy_hi, const void* dy_lo, const void* wt_hi, const void* wt_lo, void* dx_hi, void* dx_lo,
                       const void* dact_hi, const void* dact_lo, float* dx_colsum, int M, int N, int K, int mode, void* stream);
/* dst[b][c][r] = src[b][r][c] for b < batch: bf16 matrix transposes (R, C multiples of 64; strides in elements).  The engine
 * keeps a transposed operand copy of the Block linears' weights next to the bf16 shadow and refreshes it once per step. */
int ig_transpose_bf16(const void* src_hi, const void* src_lo, void* dst_hi, void* dst_lo, int R, int C, int batch, long src_stride,
                      long dst_stride, void* stream);
/* F.scaled_dot_product_attention of timm Attention: qkv [B][N][3][H][hd] -> out [B][N][H*hd], lse [B][H][N]; head_dim 64 or 80.
 * ig_attention_bwd: dqkv_colsum (optional, fp32 [3*H*hd]) += column sums of dqkv over the B*N tokens = the bias gradient of the
 * fused qkv Linear (pritvhi.py:446-456 -> timm Attention.qkv); fused into the single-pass backward kernel where that runs. */
int ig_attention_fwd(const void* qkv_hi, const void* qkv_lo, void* out_hi, void* out_lo, float* lse, int B, int N, int H,
                     int head_dim, void* stream);
int ig_attention_bwd(const void* qkv_hi, const void* qkv_lo, const void* out_hi, const void* out_lo, const void* dout_hi,
                     const void* dout_lo, const float* lse, float* delta, void* dqkv_hi, void* dqkv_lo, float* dqkv_colsum, int B,
                     int N, int H, int head_dim, void* stream);
/* gradient plumbing: column sums (bias grads), patch-embed grad prep (cls_token / conv bias grads) */
int ig_colsum(const void* hi, const void* lo, float* out, long M, int C, void* stream);
int ig_patch_grad_prep(const float* dx, void* hi, void* lo, float* dcls, float* dbias, int B, int ntok, int D, void* stream);
int ig_split_bf16(const float* src, void* hi, void* lo, long n, void* stream);
int ig_merge_bf16(const void* hi, const void* lo, float* dst, long n, void* stream);

/* ---- decode head (instageo/model/model.py:349-390) --------------------------------------------------- */
/* nn.ConvTranspose2d(k=3,s=2,p=1,op=1) + nn.Dropout(p): x (B,H,W,Cin) -> y (B,2H,2W,Cout)             :361-369 */
int ig_convT_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, void* y_hi,
                 void* y_lo, int B, int H, int W, int Cin, int Cout, unsigned drop_seed, const unsigned* drop_seed_dev, float drop_p,
                 void* stream);
int ig_convT_dgrad(const void* dy_hi, const void* dy_lo, const void* w_hi, const void* w_lo, void* dx_hi, void* dx_lo, int B,
                   int H, int W, int Cin, int Cout, void* stream);
/* dbias (optional): dbias[co] += sum over the output pixels of dy (the ConvTranspose2d bias gradient); fused into the direct
 * kernel of the 96 -> 48 stage, one column-sum pass otherwise */
int ig_convT_wgrad(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, float* dw, float* dbias, int B, int H,
                   int W, int Cin, int Cout, void* stream);
/* nn.Conv2d(k=3,padding=1)                                                                           :370-375 */
/* bn_scale/bn_shift (may be NULL): eval-mode BatchNorm2d + ReLU folded into the epilogue, y = relu((conv+bias)*s + t) */
int ig_conv3x3_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias,
                   const float* bn_scale, const float* bn_shift, void* y_hi, void* y_lo, int B, int H, int W, int Cin, int Cout,
                   void* stream);
/* the same in front of a training-mode nn.BatchNorm2d (:376): where a direct kernel runs (48 / 96 channels), the convolution also leaves
 * sums[2 Cout] (per-channel sum / sum of squares of the stored outputs) and sets *fused = 1 (HOST int); else *fused = 0 */
int ig_conv3x3_fwd_stats(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, void* y_hi,
                         void* y_lo, double* sums, int* fused, int B, int H, int W, int Cin, int Cout, void* stream);
/* inference tail: the last nn.Conv2d(k=3, padding=1) (:370-375, + eval-mode BatchNorm + ReLU) and the nn.Conv2d(k=1) classifier (:389;
 * dropout is the identity in eval mode) in ONE kernel where the direct 48-channel kernel runs and ncls <= 2: *fused = 1 (HOST int), y_hi
 * may be NULL (the activation is then not stored).  *fused = 0: nothing was computed, run ig_conv3x3_fwd + ig_classifier_fwd. */
int ig_conv3x3_cls_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, const float* bn_scale,
                       const float* bn_shift, void* y_hi, const float* cls_w, const float* cls_b, float* logits, int* fused, int B, int H,
                       int W, int Cin, int Cout, int ncls, void* stream);
/* batch statistics -> scale / shift / mean / rstd (+ running update) from sums a producer filled (finalize step of ig_bn_relu_fwd) */
int ig_bn_finalize(const double* sums, const float* gamma, const float* beta, float* running_mean, float* running_var, float* scale,
                   float* shift, float* mean, float* rstd, long M, int C, float eps, float momentum, int update_running, void* stream);
int ig_bn_eval_affine(const float* gamma, const float* beta, const float* running_mean, const float* running_var, float* scale,
                      float* shift, int C, float eps, void* stream);
int ig_conv3x3_dgrad(const void* dy_hi, const void* dy_lo, const void* w_hi, const void* w_lo, void* dx_hi, void* dx_lo, int B,
                     int H, int W, int Cin, int Cout, unsigned drop_seed, const unsigned* drop_seed_dev, float drop_p, void* stream);
/* dbias (optional): dbias[co] += sum_pixels dy[p][co] (the Conv2d bias gradient); fused into the direct kernels (48 / 96 / 192
 * input channels: an all-ones MFMA operand against the dy fragments), one column-sum pass otherwise */
int ig_conv3x3_wgrad(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, float* dw, float* dbias, int B, int H,
                     int W, int Cin, int Cout, void* stream);
/* nn.Conv2d(kernel_size=KS, padding=1) for odd KS in 3..9: the 5 x 5 / 7 x 7 convolutions of the 600M variants' decode head
 * (model.py:169-177 seg_head_kernel_sizes, :370-375).  NHWC, weights Wc[Cout][KS*KS][Cin]; x is (B,H,W,Cin), y / dy are
 * (B,Ho,Wo,Cout) with Ho = H + 3 - KS, Wo = W + 3 - KS.  bn_scale / bn_shift as in ig_conv3x3_fwd. */
int ig_convk_fwd(const void* x_hi, const void* x_lo, const void* w_hi, const void* w_lo, const float* bias, const float* bn_scale,
                 const float* bn_shift, void* y_hi, void* y_lo, int B, int H, int W, int Cin, int Cout, int KS, void* stream);
int ig_convk_dgrad(const void* dy_hi, const void* dy_lo, const void* w_hi, const void* w_lo, void* dx_hi, void* dx_lo, int B,
                   int H, int W, int Cin, int Cout, int KS, unsigned drop_seed, const unsigned* drop_seed_dev, float drop_p,
                   void* stream);
int ig_convk_wgrad(const void* dy_hi, const void* dy_lo, const void* x_hi, const void* x_lo, float* dw, float* dbias, int B, int H,
                   int W, int Cin, int Cout, int KS, void* stream);
/* nn.BatchNorm2d + nn.ReLU on [M][C] (M = B*H*W)                                                      :376-377 */
int ig_bn_relu_fwd(const void* x_hi, const void* x_lo, const float* gamma, const float* beta, float* running_mean,
                   float* running_var, void* y_hi, void* y_lo, float* scale, float* shift, float* mean, float* rstd,
                   double* sums, long M, int C, float eps, float momentum, int training, int update_running, void* stream);
int ig_bn_relu_bwd(const void* x_hi, const void* x_lo, const void* dy_hi, const void* dy_lo, const float* scale,
                   const float* shift, const float* mean, const float* rstd, void* dx_hi, void* dx_lo, float* dgamma,
                   float* dbeta, double* sums, long M, int C, void* stream);
/* y_hi == NULL: batch statistics + scale / shift / mean / rstd (+ running update) only, no apply pass (ig_classifier_bn_fwd applies);
 * training == 2: batch statistics that a producer has already left in sums (ig_conv3x3_fwd_stats with *fused == 1): no statistics pass */
/* nn.Dropout(p) + nn.Conv2d(k=1): f (B,HW,C) -> logits (B,ncls,HW) f32                                 :388-389 */
int ig_classifier_fwd(const void* f_hi, const void* f_lo, const float* w, const float* bias, float* logits, int B, long HW, int C,
                      int ncls, unsigned drop_seed, const unsigned* drop_seed_dev, float drop_p, void* stream);
int ig_classifier_bwd(const float* dlogits, const void* f_hi, const void* f_lo, const float* w, void* df_hi, void* df_lo,
                      float* dw, float* db, const double* count, int B, long HW, int C, int ncls, unsigned drop_seed,
                      const unsigned* drop_seed_dev, float drop_p, void* stream);
/* training-mode tail of the head in fused passes: the last stage's nn.BatchNorm2d + nn.ReLU (:376-377) applied inside the
 * nn.Dropout + nn.Conv2d(k=1) kernels (:388-389); x = that stage's Conv2d output.  The activation between them and its gradient
 * are recomputed, never stored.  Backward: classifier dW / db + the BatchNorm sums in one pass over x, dx + dgamma / dbeta in a second. */
int ig_classifier_bn_fwd(const void* x_hi, const void* x_lo, const float* scale, const float* shift, const float* w, const float* bias,
                         float* logits, int B, long HW, int C, int ncls, unsigned drop_seed, const unsigned* drop_seed_dev, float drop_p,
                         void* stream);
int ig_classifier_bn_bwd(const float* dlogits, const void* x_hi, const void* x_lo, const float* scale, const float* shift,
                         const float* mean, const float* rstd, const float* w, void* dx_hi, void* dx_lo, float* dw, float* db,
                         float* dgamma, float* dbeta, double* sums, const double* count, int B, long HW, int C, int ncls,
                         unsigned drop_seed, const unsigned* drop_seed_dev, float drop_p, void* stream);

/* ---- task module (instageo/model/segmentation.py, metrics.py, infer_utils.py, base.py) --------------- */
/* CE(weight, ignore_index,'none') + masked mean pieces, argmax, int64 confusion matrix   segmentation.py:85-87,117-151 */
int ig_ce_loss(const float* logits, const void* labels, int label_dtype, const float* class_weights, long ignore_index,
               double* stats, float* dlogits, long long* preds, signed char* preds_i8, unsigned long long* confusion, int B,
               long HW, int ncls, void* stream);
/* Focal + region (Dice / Tversky) segmentation loss for class-imbalanced maps (not in the reference).  Same inputs, outputs and validity
 * predicate (label != ignore_index and 0 <= label < ncls) as ig_ce_loss; p = softmax(logits), pt = p[y]:
 *   pixel term  sum_valid w_y (1 - pt)^gamma (-log pt); focal_gamma = 0 is the cross-entropy of ig_ce_loss (bit for bit when
 *               region_weight = 0 as well), otherwise 1 <= focal_gamma <= 8; pixel_term = 0 drops the term (loss = region term alone)
 *               while the count, argmax and confusion matrix still run
 *   region term region_weight * (1 / K_p) sum_{c present} (1 - T_c),  T_c = (I_c + s) / (I_c + alpha (P_c - I_c) + beta (G_c - I_c) + s)
 *               over the valid pixels of the whole launch (I_c = sum p_c [y == c], P_c = sum p_c, G_c = #{y == c}, K_p = classes present,
 *               s = region_smooth >= 0; alpha = beta = 0.5 is Dice); class weights do not enter it; off when region_weight = 0
 * stats double[2] += (pixel-term sum + #valid * region term, #valid): loss = stats[0] / stats[1] (NaN when nothing is valid); dlogits is the
 * gradient of stats[0], UN-normalised like ig_ce_loss's (divide by stats[1] downstream; ig_kd_loss stacks on top unchanged).  parts
 * (optional, needs stats) double[2] += (pixel-term sum, #valid * region term) for logging.  All sums are folded in a fixed order or as
 * integers: results are bit-identical from run to run.  The region term costs a second pass over logits, labels and dlogits. */
int ig_seg_loss(const float* logits, const void* labels, int label_dtype, const float* class_weights, long ignore_index, float focal_gamma,
                int pixel_term, float region_weight, float region_smooth, float tversky_alpha, float tversky_beta, double* stats, double* parts,
                float* dlogits, long long* preds, signed char* preds_i8, unsigned long long* confusion, int B, long HW, int ncls, void* stream);
/* torch.argmax(dim=1) -> int8                                                           infer_utils.py:99-101 */
int ig_argmax_i8(const float* logits, signed char* out, int B, long HW, int ncls, void* stream);
/* RunningConfusionMatrix.update                                                         metrics.py:86-108 */
/* knowledge distillation (segmentation.py:352-378): KLDivLoss(batchmean)(log_softmax(student),
 * softmax(teacher)) over the valid pixels: *kl_sum += KL sum, dlogits += softmax(student) - softmax(teacher) (un-normalised,
 * on top of the cross-entropy gradient written by ig_ce_loss) */
int ig_kd_loss(const float* student_logits, const float* teacher_logits, const void* labels, int label_dtype, long ignore_index,
               double* kl_sum, float* dlogits, int B, long HW, int ncls, void* stream);
/* regression head (regression.py:141-191, metrics.py:330-352): masked MSE (+ log1p label scale) of the
 * single-channel output: stats double[2] += (sum sq. err, #valid), dpred = 2 (pred - label') un-normalised, msums double[9] =
 * streaming sums of RunningRegressionMetrics on the de-scaled values {n, Sx, Sy, Sxy, Sxx, Syy, S|e|, See, #within EE} */
int ig_mse_loss(const float* pred, const float* labels, float ignore_value, int use_log_scale, double* stats, float* dpred,
                double* msums, float ee_bias, float ee_coef, int include_ee, long n, void* stream);
/* distillation of the regression task (regression.py:345-534): sum[0] += sum over valid pixels (labels != ignore_value) of
 * (pred - teacher')^2, teacher' = log1p(teacher) under use_log_scale (regression.py:527-529); dpred += 2 (pred - teacher') on
 * top of the gradient ig_mse_loss wrote (both terms are means over the same valid count, regression.py:496-503) */
int ig_kd_mse_loss(const float* pred, const float* teacher, const float* labels, float ignore_value, int use_log_scale, double* sum,
                   float* dpred, long n, void* stream);
/* test-time metrics on the device: RunningAUC histograms of softmax(logits) (metrics.py:214-256 via
 * segmentation.py:153-156; hist = uint64 [2][ncls][nbins], 0 = positives / 1 = negatives of each class, ignored pixels
 * skipped) and predict_step's softmax(logits, 1)[:, cls] (segmentation.py:202-213) */
int ig_auc_update(const float* logits, const void* labels, int label_dtype, long ignore_index, unsigned long long* hist, int B,
                  long HW, int ncls, int nbins, float min_score, float max_score, void* stream);
int ig_softmax_prob(const float* logits, float* out, int B, long HW, int ncls, int cls, void* stream);
/* Probability-blended tile inference (tile_blend.hip).  The windows of a tile form the row-major grid tops[n_rows] x lefts[n_cols]
 * (DEVICE int32, each ascending: process_test's rule, dataloader.py:655-664, optionally with a last origin at size - crop).
 * ig_window_blend_accumulate adds windows [w0, w0 + n) of that grid, logits (n, ncls, crop, crop) f32, to a canvas band:
 * acc (ncls, Hb, W) and wsum (Hb, W) hold canvas rows [y0, y0 + Hb) of the H x W tile; only rows [ylo, yhi) of it are visited (the
 * rows the batch covers).  Per covered pixel and window, w = wvec[y - top] * wvec[x - left]: wsum += w, acc[c] += w * softmax(logits)[c]
 * (max-subtracted, as predict_step's probability, segmentation.py:202-213; the raw value when ncls == 1).  No atomics: a pixel's terms
 * are added in row-major window order, so the canvas is bit-identical however the windows are split into batches.
 * ig_window_blend_finalize, per pixel of the full canvas (HW = H * W): where wsum == 0 or (nodata_enabled) any band of tile
 * (TC, H, W), tile_dtype 0 = int16 / 1 = f32, equals no_data_value: classmap = fill, prob = NaN; else p_c = acc_c / wsum, classmap =
 * the first argmax (ig_argmax_i8), prob (ncls, H, W) optional.  ncls == 1: classmap NULL, prob = the blended regression value. */
int ig_window_blend_accumulate(const float* logits, const int* tops, const int* lefts, int n_rows, int n_cols, long w0, int n,
                               const float* wvec, float* acc, float* wsum, int ncls, int crop, int H, int W, int y0, int Hb, int ylo,
                               int yhi, void* stream);
int ig_window_blend_finalize(const float* acc, const float* wsum, const void* tile, int tile_dtype, int TC, double no_data_value,
                             int nodata_enabled, signed char* classmap, float* prob, int ncls, long HW, int fill, void* stream);
/* D4 test-time augmentation and uncertainty rasters on the blend canvas (tile_blend.hip).
 * The eight transforms of an S x S plane a: code k in 0..7 has bits h = k & 1, v = (k >> 1) & 1, t = (k >> 2) & 1 and
 *   G_k(a)[y][x] = a[sy][sx],  (y1, x1) = t ? (x, y) : (y, x),  sy = v ? S-1-y1 : y1,  sx = h ? S-1-x1 : x1
 * (0 identity, 1 fliplr, 2 flipud, 3 rot180, 4 transpose, 5 rot90 counter-clockwise, 6 rot90 clockwise, 7 anti-transpose; the inverse of k
 * is k when t = 0, else 4 | v | (h << 1): dataloader.d4_inverse).
 * ig_d4_apply: codes = HOST array of K codes (1 <= K <= 8), f32 planes, src != dst, bits are copied.  expand = 1: src (m, P, S, S) ->
 * dst (m*K, P, S, S), dst[i*K + j] = G_codes[j](src[i]); expand = 0: both (m*K, P, S, S), dst[i*K + j] = G_codes[j](src[i*K + j]).
 * ig_window_blend_accumulate_tta: ig_window_blend_accumulate with K (1 <= K <= 8) logit sets per window, logits (n, K, ncls, crop, crop)
 * already in the canvas frame; a pixel's terms are added in row-major window order and, inside a window, in order j = 0..K-1 (for K > 1
 * a window's K fp32 terms are summed in fp64 and added to the fp32 canvas with one rounding, acc[c] += w * sum_j softmax(logits[j])[c],
 * wsum += K * w), so the canvas is bit-identical for any split of the windows into batches; K = 1 is ig_window_blend_accumulate bit
 * for bit.
 * ig_window_blend_uncertainty, per pixel of the finished canvas with ig_window_blend_finalize's validity rule (NaN where wsum == 0 or a
 * band is NODATA): p_c = acc_c / wsum, entropy = -sum_c p_c ln p_c / ln(ncls) (0 ln 0 = 0), margin = largest p - second largest p;
 * entropy or margin may be NULL (not both); 2 <= ncls <= 127. */
int ig_d4_apply(const float* src, float* dst, const int* codes, int K, int m, int P, int S, int expand, void* stream);
int ig_window_blend_accumulate_tta(const float* logits, const int* tops, const int* lefts, int n_rows, int n_cols, long w0, int n, int K,
                                   const float* wvec, float* acc, float* wsum, int ncls, int crop, int H, int W, int y0, int Hb, int ylo,
                                   int yhi, void* stream);
int ig_window_blend_uncertainty(const float* acc, const float* wsum, const void* tile, int tile_dtype, int TC, double no_data_value,
                                int nodata_enabled, float* entropy, float* margin, int ncls, long HW, void* stream);
/* Region post-processing of class maps (regions.hip; not in the reference).  A class map is (n, H, W) int8, contiguous; `fill` (any int8
 * value) marks invalid pixels, every other value is a class; H * W <= 2^31 - 1; images are independent; connectivity is 4 or 8.  All
 * results are integers and unique: bit-identical from run to run.  n = 0 returns IG_OK without touching a pointer.
 * ig_ccl_label: labels (n, H, W) int32 = the smallest row-major index y * W + x among the pixels of the pixel's component (same class,
 *   connected under `connectivity`), -1 at fill pixels.  status: device int, zeroed by the caller; nonzero afterwards means a capped
 *   union-find loop gave up (the labels are then not valid): the caller must check it.
 * ig_region_area: area (n, HW) int32 = the pixel count at root positions (labels[p] == p), 0 elsewhere.
 * ig_sieve_pass: one pass of the minimum-mapping-unit sieve on cls, IN PLACE, given its labels and areas.  Regions with area <
 *   min_region are small, the others kept.  A small region R takes the class of the kept region S that shares a 4-neighbour edge with
 *   it and has the largest area (ties: the smaller label): best (n, HW) uint64 scratch receives max((area(S) << 32) | (0xFFFFFFFF - S))
 *   at R.  Small regions without a kept neighbour stay; fill never counts.  *changed (device int) += the small regions reassigned.
 * ig_region_stats: stats (n_regions, 7) int64 = {area, row_min, row_max, col_min, col_max, row_sum, col_sum} of every region;
 *   rid (n, HW) int32 holds at root positions the region's row in stats (dense, from area != 0; other positions are not read). */
int ig_ccl_label(const signed char* cls, int* labels, int n, int H, int W, int connectivity, int fill, int* status, void* stream);
int ig_region_area(const int* labels, int* area, int n, long HW, void* stream);
int ig_sieve_pass(signed char* cls, const int* labels, const int* area, int min_region, int n, int H, int W, int fill,
                  unsigned long long* best, int* changed, void* stream);
int ig_region_stats(const int* labels, const int* rid, long long* stats, long n_regions, int n, int H, int W, void* stream);
/* Post-hoc calibration of the class probabilities (calibrate.hip; not in the reference).  Inputs and validity predicate of ig_ce_loss /
 * ig_auc_update: logits (B, ncls, HW) f32 planar, labels with label_dtype 0 = int64 / 1 = int32 / 2 = f32, a pixel is valid iff
 * label != ignore_index and 0 <= label < ncls; 2 <= ncls <= 127.  B == 0 or HW == 0 returns IG_OK without touching a pointer.
 * ig_calib_nll_grid: inv_temps = HOST array of K values beta_k = 1 / T_k, 1 <= K <= 32, each finite and > 0.  For every valid pixel and k:
 *   nll[k] += logsumexp_c(beta_k z_c) - beta_k z_y, evaluated max-subtracted (exponents beta_k (z_c - max_c z_c) <= 0).  nll = DEVICE
 *   double[K], accumulated; count = DEVICE uint64, += #valid.  A thread sums its pixels in double, workgroup partials are folded in
 *   workgroup order by a second launch, the count is an integer add: bit-identical from run to run, no float atomics.  Uses a per
 *   (device, stream) scratch buffer: the first call on a stream must not happen during a graph capture.
 * ig_reliability_update: hist = DEVICE uint64 [ncls][3][nbins], accumulated, indexed by the PREDICTED class.  Per valid pixel:
 *   p = softmax(inv_temp * z) max-subtracted, pred = the first argmax (ig_argmax_i8's rule), conf = p[pred], bin = min(nbins - 1,
 *   floor(conf * nbins)); hist[pred][0][bin] += 1, hist[pred][1][bin] += (pred == label), hist[pred][2][bin] += floor(conf * 2^24 + 0.5).
 *   1 <= nbins <= 64 and ncls * nbins <= 4096 (the workgroup-local LDS histogram); B * HW <= 2^40 per call.  Integer sums only: the
 *   result does not depend on any order and adds across ranks; the confidence sum cannot overflow below 2^40 pixels in total. */
int ig_calib_nll_grid(const float* logits, const void* labels, int label_dtype, long ignore_index, const float* inv_temps, int K, double* nll,
                      unsigned long long* count, int B, long HW, int ncls, void* stream);
int ig_reliability_update(const float* logits, const void* labels, int label_dtype, long ignore_index, float inv_temp,
                          unsigned long long* hist, int B, long HW, int ncls, int nbins, void* stream);
/* Boundary-quality primitives on class maps (boundary.hip; not in the reference).  Class maps as above: (n, H, W) int8, contiguous, `fill`
 * (any int8 value) marks invalid pixels, images are independent, H * W <= 2^31 - 1.  All results are integers and unique: bit-identical
 * from run to run.  n = 0 returns IG_OK without touching a device pointer.
 * ig_boundary_dist2: dist2 (n, H, W) int32, 1 <= rmax <= 32.  For a pixel p with cls[p] != fill,
 *   dist2[p] = min{ (py - qy)^2 + (px - qx)^2 : q inside the image, cls[q] != fill, cls[q] != cls[p] }
 *   when that minimum is <= rmax^2, else IG_BOUNDARY_FAR; dist2[p] = -1 at fill pixels.  Fill is transparent (never a source, distances
 *   pass through it) and the image border is no boundary.
 * ig_boundary_update: gt, pred (n, HW) int8 with their dist2 rasters gt_d2, pred_d2 (n, HW) int32; thresholds = HOST array of K squared
 *   distances t_k, 1 <= K <= 8, strictly ascending, each in [1, 1024].  A pixel counts iff gt != fill, pred != fill and both classes lie
 *   in [0, ncls), 2 <= ncls <= 127.  Accumulated (the caller zeroes) into DEVICE uint64 tables:
 *     band[K][ncls][3]:       band[k][c][0] += (gt == c and gt_d2 <= t_k), band[k][c][1] += (pred == c and pred_d2 <= t_k),
 *                             band[k][c][2] += (gt == pred == c and gt_d2 <= t_k and pred_d2 <= t_k)
 *     trimap[K][ncls][ncls]:  trimap[k][gt][pred] += (gt_d2 <= t_k)
 *   Integer sums only: the result does not depend on any order and adds across calls and ranks.  Tables of K * ncls * (ncls + 3) <= 8192
 *   cells are aggregated per workgroup in LDS (32-bit cells, hence n * HW <= 2^40 per call) and reach memory as one 64-bit add per
 *   non-empty cell and workgroup; larger tables (e.g. K = 8 beyond 30 classes, K = 1 beyond 89) take one 64-bit global atomic per
 *   pixel, table and k. */
#define IG_BOUNDARY_FAR 0x7fffffff
int ig_boundary_dist2(const signed char* cls, int* dist2, int n, int H, int W, int rmax, int fill, void* stream);
int ig_boundary_update(const signed char* gt, const signed char* pred, const int* gt_d2, const int* pred_d2, const int* thresholds, int K,
                       unsigned long long* band, unsigned long long* trimap, int n, long HW, int ncls, int fill, void* stream);
/* Vectorisation of labelled class maps into polygon rings (vectorize.hip; not in the reference).  labels (n, H, W) int32 are those of
 * ig_ccl_label (a component's smallest pixel index, -1 at fill; fill and the outside of the image count as label -1); images are
 * independent; H * W <= 2^31 - 1.  Pixel (r, c) covers [c, c+1] x [r, r+1] in (x, y), y down.  A valid pixel p owns four directed unit
 * edges with p on their right-hand side: side 0 top (c,r)->(c+1,r) heading E, 1 right (c+1,r)->(c+1,r+1) S, 2 bottom (c+1,r+1)->(c,r+1) W,
 * 3 left (c,r+1)->(c,r) N; d[0..3] = E, S, W, N as (dr, dc) = (0,1), (1,0), (0,-1), (-1,0).  Side s of p is LIVE iff the pixel across it,
 * p + d[(s+3)%4], has another label.  The successor of the live edge (p, s), with me = label(p), A = p + d[s], B = A + d[(s+3)%4]:
 * (B, (s+3)%4) if label(B) == me (left turn), else (A, s) if label(A) == me (straight), else (p, (s+1)%4) (right turn); it is always
 * live, and the successor map is a permutation of the live edges whose cycles are the rings.  Live edges are numbered 0..E-1 in the
 * order of (image * HW + pixel) * 4 + side ("compact ids"); E <= 2^31 - 1.  A ring's root is its smallest compact id.  Its vertices are
 * the tails of the edges whose predecessor has another heading ("turn" edges), in ring order from the root.  Twice its signed area is
 * sum (x1 y2 - x2 y1) over its edges in lattice coordinates: positive for a region's exterior ring (one per region), negative for a hole.
 * Under 8-connectivity a ring may touch itself at a vertex.  All results are integers and unique: bit-identical from run to run.  Every
 * launch does a fixed amount of work; no kernel waits on another workgroup.  n = 0 or E = 0 returns IG_OK without touching a pointer.
 * ig_edge_mask: mask (n, H, W) uint8: bits 0-3 = the live sides of the pixel, bits 4-6 = their number (0 at fill pixels); *total (device
 *   uint64) += the live edges of all images.  The exclusive scan of (mask >> 4) over image * HW + pixel is the caller's: off (n, HW)
 *   int32 = the compact id of the pixel's first live edge, so edge (p, s) has id off[p] + popcount(mask[p] & ((1 << s) - 1)).
 * ig_edge_link: for every live edge e with successor f: succ[e] = f (E int32), tail[e] = the (x, y) of e's tail vertex ((E, 2) int32),
 *   flag[f] = heading(f) | (heading(f) != heading(e)) << 2 (E uint8; every f is written once because succ is a permutation).  status:
 *   device int, zeroed by the caller; nonzero afterwards means a successor was not live (labels and mask do not belong together).
 * ig_ring_jump: ONE round of pointer jumping over the E edges; the caller loops it, at most ceil(log2 E) rounds per phase, reading one
 *   buffer pair and writing another (val_in / ptr_in -> val_out / ptr_out, never in place), and may stop when *changed (device int,
 *   zeroed by the caller before the round) stays 0.
 *   phase 0, ring root by min-propagation: val_out[e] = min(val_in[e], val_in[ptr_in[e]]), ptr_out[e] = ptr_in[ptr_in[e]]; first round:
 *     val_in = NULL stands for val_in[e] = e, and ptr_in = succ.  *changed is set when a value fell.  At the end val = the ring's root.
 *   phase 1, vertex ranking with the cycle cut at the root (a pointer of -1 is the end of the list): val_out[e] = val_in[e] +
 *     (ptr_in[e] >= 0 ? val_in[ptr_in[e]] : 0), ptr_out[e] = ptr_in[e] >= 0 ? ptr_in[ptr_in[e]] : -1; first round: val_in = NULL stands for
 *     val_in[e] = flag[e] >> 2 & 1 and ptr_in = succ stands for (succ[e] == root[e] ? -1 : succ[e]); root and flag are read in that
 *     round only.  *changed is set while a pointer is still >= 0.  At the end val[e] = the turn edges from e to the end of its ring, so
 *     val[root] = the ring's vertices and val[root[e]] - val[e] = the position of turn edge e among them.
 * ig_ring_sums: sums (n_rings, 2) int64 += {vertices, twice the signed area} of every ring (the caller zeroes); ring_id (E int32) holds
 *   at root positions the ring's row in sums (dense; other positions are not read).  Integer atomics, one per run of adjacent edges of
 *   one ring in a wave.
 * ig_ring_emit: vertices (n_vertices, 2) int32: for every turn edge e, vertices[first[ring_id[root[e]]] + rank[root[e]] - rank[e]] =
 *   tail[e]; rank = the result of phase 1, first (n_rings int64) = where the ring's vertices start.  status: device int, zeroed by the
 *   caller; nonzero afterwards means a destination lay outside [0, n_vertices) (nothing is written there). */
int ig_edge_mask(const int* labels, unsigned char* mask, unsigned long long* total, int n, int H, int W, void* stream);
int ig_edge_link(const int* labels, const unsigned char* mask, const int* off, int* succ, int* tail, unsigned char* flag, int n, int H,
                 int W, long E, int* status, void* stream);
int ig_ring_jump(int phase, const int* val_in, const int* ptr_in, int* val_out, int* ptr_out, const int* root, const unsigned char* flag,
                 long E, int* changed, void* stream);
int ig_ring_sums(const int* root, const int* ring_id, const int* tail, const unsigned char* flag, long long* sums, long E, long n_rings,
                 void* stream);
int ig_ring_emit(const int* root, const int* ring_id, const int* rank, const int* tail, const unsigned char* flag, const long long* first,
                 int* vertices, long E, long n_rings, long n_vertices, int* status, void* stream);
/* Zonal statistics: polygon zones rasterised onto a class map and tallied per zone and class (zonal.hip; not in the reference).  The
 * inverse of the vectorisation above, in its coordinates: the raster is one (H, W) int8 class map, `fill` marks invalid pixels,
 * H * W <= 2^31 - 1, pixel (r, c) covers [c, c+1] x [r, r+1] in lattice (x, y), y down.  Zone vertices arrive in fixed point with Q = 256
 * units per pixel, X = floor(x * 256 + 0.5) and the same for Y, computed by the host in float64 as int32 with |X|, |Y| <= 2^29 (an edge
 * with a coordinate beyond that crosses nothing); the centre of pixel (r, c) is (Xc, Yc) = (256 c + 128, 256 r + 128).  A zone is a set
 * of closed rings (exteriors and holes of a Polygon or MultiPolygon; orientation is irrelevant) given as directed edges
 * (x0, y0) -> (x1, y1).  An edge CROSSES row r iff (y0 <= Yc) != (y1 <= Yc) (half-open: a horizontal edge crosses nothing, a vertex on
 * the centre line belongs to the edge that goes down from it); its crossing abscissa is the rational xc = x0 + (x1 - x0)(Yc - y0)/(y1 - y0).
 * Pixel (r, c) is INSIDE the zone iff an odd number of the zone's edges cross row r with xc <= Xc: the even-odd rule on pixel centres
 * (GDAL / rasterio without all_touched); ties at vertices and centres are decided by these two inequalities and nothing else.  Every
 * quantity is an integer: differences stay below 2^31, sums of products below 2^62 (int64), no floating point.  Zones are independent:
 * a pixel inside several zones counts in each.  Up to 64 zones go through one pass over a (H, W) uint64 canvas, one bit per zone; all
 * results are unique: bit-identical from run to run.  Every launch does a fixed amount of work; no kernel waits on another workgroup.
 * E = 0, T = 0 or H * W = 0 returns IG_OK without touching a pointer.
 * ig_zone_edge_rows: edges (E, 4) int32 {x0, y0, x1, y1}, 16-byte aligned; rows[e] (E int32) = the number of rows in [0, H) that edge e
 *   crosses under (y0 <= Yc) != (y1 <= Yc), Q = 256.  The exclusive scan of rows is the caller's: first (E int64) = the number of the
 *   edge's first (edge, crossed row) pair, with total T <= 2^38.
 * ig_zone_toggle: one work item per (edge, crossed row) pair 0..T-1; the edge is found by binary search in first, so the work is
 *   balanced whatever the spread of edge lengths (an edge may span every row).  The item computes c* = max(0, ceil((xc - 128)/256)), the
 *   first column with xc <= Xc (Q = 256: Xc = 256 c + 128), exactly: int64 floor division with the denominator made positive.  If c* < W it
 *   flips bit bit[e] (E uint8, 0..63: the zone's bit in this pass) of canvas[r][c*] with a 64-bit atomic XOR, which is order-independent;
 *   the caller zeroes the canvas.  The rows are those of ig_zone_edge_rows ((y0 <= Yc) != (y1 <= Yc)); items that first places outside
 *   their edge's rows are dropped.
 * ig_zone_tally: the inclusive prefix XOR along each row of canvas turns the toggles into inside masks (bit z of pixel (r, c) = an odd
 *   number of zone z's crossings of row r, (y0 <= Yc) != (y1 <= Yc), have c* <= c, i.e. xc <= Xc at Q = 256), and in the same pass
 *   counts (64, ncls + 1) uint64 += for every set bit z: counts[z][k] with k = cls[r][c] when that is a class in [0, ncls), else
 *   k = ncls (fill, or a value outside [0, ncls)); 2 <= ncls <= 127.  counts is accumulated (the caller zeroes it): per workgroup in an LDS
 *   table of 32-bit cells, then one 64-bit atomic add per non-empty cell.  write_mask != 0 leaves the inside masks in canvas, 0 leaves
 *   the toggles.  cls = NULL (with write_mask != 0) computes the masks only: counts is not touched. */
int ig_zone_edge_rows(const int* edges, int* rows, long E, int H, void* stream);
int ig_zone_toggle(const int* edges, const unsigned char* bit, const long long* first, unsigned long long* canvas, long E, long T, int H,
                   int W, void* stream);
int ig_zone_tally(unsigned long long* canvas, const signed char* cls, unsigned long long* counts, int H, int W, int ncls, int fill,
                  int write_mask, void* stream);
/* all_touched rasterisation (zonal.hip; not in the reference): a second rule on the grid, fixed point and limits of the block above
 * (Q = 256, |X|, |Y| <= 2^29, H * W <= 2^31 - 1), for features that are small next to a pixel.  The default stays the centre rule.
 * THE RULE.  Pixel (r, c) is the square 256 c <= X <= 256 c + 256, 256 r <= Y <= 256 r + 256.  An edge TOUCHES pixel (r, c) iff the closed
 *   segment (x0, y0)-(x1, y1) meets the OPEN square (256 c, 256 c + 256) x (256 r, 256 r + 256).  Under all_touched a pixel belongs to a
 *   zone or feature iff its centre is inside by the rule above OR one of the zone's edges touches it.  The square is open on purpose: an
 *   edge that runs along a pixel border touches neither side, so a polygon whose vertices sit on the pixel lattice selects the same pixels
 *   under both rules (a closed square would grow it by a ring).  This is not GDAL's line walker; for vertices in general position it is
 *   expected to select the pixels of rasterio's all_touched=True, which has not been verified.
 * ROWS.  With ymin = min(y0, y1), ymax = max(y0, y1) an edge touches exactly the rows floor(ymin / 256) <= r <= ceil(ymax / 256) - 1,
 *   clamped to [0, H): none when ymin = ymax lies on a row border.
 * COLUMNS of row r.  A non-horizontal edge: ya = max(ymin, 256 r), yb = min(ymax, 256 r + 256) and the abscissae x(ya), x(yb) as exact
 *   rationals N / |y1 - y0|, N = x0 (y1 - y0) + (x1 - x0)(y - y0) negated when y1 < y0, |N| < 2^61 (int64).  A horizontal edge: its two x
 *   coordinates.  With lo the smaller and hi the larger, the touched columns are exactly floor(lo / 256) <= c <= ceil(hi / 256) - 1,
 *   clamped to [0, W): none for a vertical edge on a column border or a span outside the raster.  Nothing is clamped ONTO column 0,
 *   unlike the toggle.  Floor and ceiling division on int64 with the denominator made positive; no floating point anywhere.
 * ig_zone_touch_rows: edges (E, 4) int32, 16-byte aligned; rows[e] (E int32) = the number of rows in [0, H) edge e touches (ROWS).  The
 *   exclusive scan is the caller's: first (E int64), total T <= 2^38.  An edge with a coordinate beyond 2^29 touches nothing.
 * ig_zone_touch: one work item per (edge, touched row) pair 0..T-1, the edge found by binary search in first.  The item sets bit bit[e]
 *   (E uint8, 0..63) of touch[r][c] for every column c of the span (COLUMNS) with 64-bit atomic ORs, which are order-independent: two
 *   runs give the same bits.  touch is a (H, W) uint64 canvas the caller zeroes.  A lane writes a span of up to 4 columns itself; longer
 *   spans (a near-horizontal edge can span the row) are written by the item's whole wave, one span after the other, 64 adjacent columns
 *   per step.  Items that first places outside their edge's rows, and bits outside 0..63, are dropped.
 * ig_zone_touch_merge: canvas (H, W) uint64 holds the toggles of the pass (ig_zone_toggle).  Per row m = (inclusive prefix XOR of the
 *   toggles, by the device function ig_zone_tally scans with (one rule, one scan)) | touch, and canvas[r][c] = m[c] ^ m[c - 1] with m[-1] = 0 is
 *   written back in place: the canvas is a toggle canvas again whose prefix XOR is the all_touched mask, and ig_zone_tally,
 *   ig_zone_value_tally, ig_zone_quantile_hist and ig_burn_resolve take it as it is (the last feature that contains or touches a pixel
 *   is the highest set bit).  touch is only read.  A workgroup owns whole rows and reads each chunk of 1024 columns before it writes it;
 *   no kernel waits on another workgroup; every launch does a fixed amount of work.
 * E = 0, T = 0 or H * W = 0 returns IG_OK without touching a pointer.  canvas, touch and first are 8-byte aligned. */
int ig_zone_touch_rows(const int* edges, int* rows, long E, int H, void* stream);
int ig_zone_touch(const int* edges, const unsigned char* bit, const long long* first, unsigned long long* touch, long E, long T, int H,
                  int W, void* stream);
int ig_zone_touch_merge(unsigned long long* canvas, const unsigned long long* touch, int H, int W, void* stream);
/* Zonal statistics of float rasters (zonal.hip; not in the reference): per zone and band the count, mean, sum of squared deviations,
 * minimum and maximum of a band-major float32 raster (B, H, W) under the inside masks of the block above.  canvas (H, W) uint64 holds the
 * TOGGLES of one pass as ig_zone_toggle leaves them; it is read, never written, so one canvas serves any number of calls (band groups).
 * The masks are the inclusive prefix XOR along each row, by the same device function as ig_zone_tally (one rule, one scan).
 * VALIDITY.  A pixel's value v is VALID iff it is finite (not NaN, not +-Inf) and, when has_nodata != 0, v != nodata (compared as
 *   float32).  An invalid value counts in `pixels` and in nothing else.
 * ARITHMETIC.  Every partial result is a triple (n, T, M2): the number of valid values, their sum and the sum of their squared deviations
 *   from their own mean T / n, all float64 (n is an integer below 2^31, exact).  A thread forms the triple of its run of 4 pixels by the
 *   two-pass formula; from there on triples are only ever MERGED, by the pairwise update of Chan, Golub and LeVeque in its (T, M2) form:
 *     n = na + nb,  T = Ta + Tb,  M2 = M2a + M2b + (Tb / nb - Ta / na)^2 * (na * nb / n),   an empty side contributes nothing,
 *   through the wave (a fixed 6-step butterfly, the lower lane always the left operand), the wave's own accumulator over the chunks and
 *   rows it owns (in the order it meets them), the workgroup (waves 0..3 in order) and the grid (ig_zone_value_reduce, workgroups in
 *   order).  No sum of squares, no pivot, no floating-point atomic.  T is a plain float64 sum: exact for integer-valued data below 2^53
 *   in total, within n * 2^-53 * sum|v| otherwise.  min and max are those of the valid float32 values.
 * DETERMINISM.  The grid is G = ig_zone_value_grid(H) = min(H, 512) workgroups whatever the device; workgroup g owns rows g, g + G, ...;
 *   the order of every merge is fixed by (H, W) alone and each band goes through the same instructions whatever B is: two runs give the
 *   same bits, and a band gives the same bits in any band group.
 * ig_zone_value_tally: raster (B, H, W) float32, contiguous, 1 <= B <= 8 (IG_ZONE_VALUE_BANDS; the caller loops over groups of bands).
 *   Writes, for its workgroup g, EVERY cell of partials (G, B, 64, 4) float64 {n, T, M2, the float32 pair (min, max) in one 8-byte
 *   word} and of pix_partials (G, 64) uint64 = the inside pixels per zone bit (band-independent): the caller need not zero them.  Empty
 *   cells hold n = 0, T = M2 = 0, min = +Inf, max = -Inf.  There are 64 bits per pixel and nothing is written for any other bit.
 * ig_zone_value_reduce: partials and pix_partials of G workgroups, merged in workgroup order, -> valid (64, B) int64, stats (64, B, 4)
 *   float64 {mean = T / n, M2, min, max} and pixels (64) int64 (NULL: not wanted).  A zone bit without a valid value reports valid = 0,
 *   mean = M2 = 0, min = +Inf, max = -Inf; population variance is M2 / valid.
 * H * W = 0 or B = 0 returns IG_OK before a pointer is looked at (ig_zone_value_reduce: G = 0 or B = 0).  Pointers are 8-byte aligned,
 * partials 16-byte, raster 4-byte. */
int ig_zone_value_grid(int H);
int ig_zone_value_tally(const unsigned long long* canvas, const float* raster, double* partials, unsigned long long* pix_partials, int H,
                        int W, int B, int has_nodata, float nodata, void* stream);
int ig_zone_value_reduce(const double* partials, const unsigned long long* pix_partials, long long* valid, double* stats,
                         long long* pixels, int G, int B, void* stream);
/* Order statistics of float rasters per zone and band: the median and percentiles (zonal.hip; not in the reference).  canvas, raster,
 * has_nodata and nodata are those of ig_zone_value_tally; the canvas is read, never written.
 * THE RULE.  The VALID values of zone z and band b are exactly those ig_zone_value_tally counts: inside the mask, finite, and != nodata
 *   as float32 when has_nodata != 0.  Zeros are canonical: a value enters as v + 0.0f, so -0.0 counts and comes out as +0.0.  Sorted
 *   ascending they are v(0) <= ... <= v(n-1), n = valid[z][b].  For a fraction f in [0, 1] (float64; the host forms f = q / 100.0 once)
 *     h = (double)(n - 1) * f,   lo = floor(h),   hi = min(lo + 1, n - 1)      (one float64 multiply and a floor, no contraction)
 *   and the device delivers the pair (v(lo), v(hi)) as float32, exactly: order statistics are members of the data, so the result is
 *   unique.  n = 0 delivers (NaN, NaN).  The host interpolates in float64 by numpy's `linear` method: g = h - lo,
 *   p = a + (b - a) * g for g > 0, else p = a, with (a, b) the pair widened to float64.  f = 0 is the minimum, 1 the maximum, 0.5 the median.
 * METHOD.  Most-significant-digit radix selection on order-preserving keys: u = bits(v + 0.0f), key = u ^ (u >> 31 ? 0xFFFFFFFF :
 *   0x80000000); IG_ZONE_QUANTILE_ROUNDS = 4 rounds of 8 bits, round r deciding key bits 31 - 8r .. 24 - 8r.  A selection of Q fractions
 *   has S = 2 Q rank slots (slot 2 i = lo, slot 2 i + 1 = hi of fraction i); 1 <= B <= 8 bands and 1 <= Q <= 8 fractions per selection
 *   (the caller loops over groups).  One selection is rounds 0, 1, 2, 3 of (ig_zone_quantile_hist, ig_zone_quantile_pick) on one stream
 *   with the same B, Q, state and hist: 8 launches, no host round trip, no wait between workgroups.  All additions are unsigned 32-bit
 *   integer atomics (a counter holds at most H * W <= 2^31 - 1), so the result does not depend on arrival order: the same bits from run
 *   to run.  Before an add reaches memory a wave merges its lanes' equal (band, zone bit, slot, digit) targets into one add of their count.
 * BUFFERS.  hist (B, 64, S, 256) uint32, zeroed by the caller before round 0 (ig_zone_quantile_pick clears what it has read); state
 *   (B, 64, S, 4) uint32 {key prefix, remaining 0-based rank (0xFFFFFFFF: n = 0), leader, unused}, 16-byte aligned, written by round 0
 *   (the caller need not initialise it).  Slots of one (band, zone bit) whose prefixes are equal share the bins of the first of them, their
 *   leader: in round 0 (empty prefix) that is slot 0 for all.
 * ig_zone_quantile_hist: round r.  The rows, the scan and the validity test of ig_zone_value_tally; for every valid pixel, zone bit z of
 *   its mask, band b and leader slot s whose prefix equals the key's bits above the round's digit d: hist[b][z][s][d] += 1.
 * ig_zone_quantile_pick: round r.  Per (band, zone bit, slot) the first digit d, ascending, whose cumulative count exceeds the slot's
 *   remaining rank; the count below d is subtracted from the rank, d is appended to the prefix, the bins read are cleared and the leaders
 *   of the next round are found.  Round 0 first forms n (the sum of the bins) -> valid (64, B) int64, and lo, hi from fractions (Q
 *   float64 in HOST memory, read during the call in every round; each in [0, 1]).  Round 3 inverts the key transform -> order (64, B, Q, 2) float32.
 * H * W = 0, B = 0 or Q = 0 returns IG_OK before a pointer is looked at (ig_zone_quantile_pick: B = 0 or Q = 0).  canvas, valid: 8-byte
 * aligned; state, hist: 16-byte; raster, order: 4-byte.  A fraction outside [0, 1] (or NaN), B > 8, Q > 8 or a round outside 0..3 is an
 * argument error. */
int ig_zone_quantile_hist(const unsigned long long* canvas, const float* raster, const unsigned* state, unsigned* hist, int H, int W,
                          int B, int Q, int round, int has_nodata, float nodata, void* stream);
int ig_zone_quantile_pick(unsigned* hist, unsigned* state, const double* fractions, long long* valid, float* order, int B, int Q,
                          int round, void* stream);
/* Polygon labels burned into label rasters (burn.hip; the reference assumes its label rasters were made with gdal_rasterize beforehand).
 * THE RULE:
 * Grid and inside test.  Those of the zonal block above, unchanged: Q = 256 fixed point, X = floor(x * 256 + 0.5), the centre of pixel
 *   (r, c) at (256 c + 128, 256 r + 128), an edge crosses row r iff (y0 <= Yc) != (y1 <= Yc), and the pixel is inside a feature iff an odd
 *   number of the feature's edges cross its row with xc <= Xc.
 * Features.  An ordered list, in file order; feature i carries one burn value v_i: an int8 in [-1, 127] for segmentation (-1 burns the
 *   ignore value), a float32 for regression (copied bit for bit).
 * Which feature wins.  A pixel takes the value of the LAST feature, in order, that contains its centre (gdal_rasterize burning the
 *   features one after the other).  A pixel in no feature keeps what the raster held before: the host initialises the raster (to the
 *   background, or to the ignore value -1 / NaN when a labelled area is given, whose polygons are then burned FIRST with the background
 *   value by the same machinery).
 * Exactness.  Everything on the device is integer work or a copy of a caller-supplied value: two runs give the same bytes, and so does
 *   the numpy host path.
 * Passes.  Features go through a canvas 64 at a time in file order: bit b of a pass is its b-th feature, so inside one pass the last
 *   containing feature is the HIGHEST set bit of the pixel's inside mask; later passes overwrite earlier ones (the host launches them in
 *   order on one stream).  The canvas of a pass is not the whole raster but an Hp x Wp rectangle with its top-left pixel at (r0, c0) of
 *   the raster: ig_zone_edge_rows and ig_zone_toggle are called as they are on that canvas with the edges shifted by (-256 c0, -256 r0),
 *   whole pixels, which is exact: the toggle clamps crossings left of column 0 to column 0 and drops rows outside [0, Hp) and columns
 *   >= Wp.
 * ig_burn_resolve: canvas (Hp, Wp) uint64 holds the TOGGLES of one pass (it is read, not written).  The inclusive prefix XOR along each
 *   canvas row (thread runs of 4, wave scan, workgroup scan, a carry in a register over the chunks of 1024 columns: the scan of
 *   ig_zone_tally) is the inside mask m of 64 features; for m != 0 the pixel is written: out[(r0 + r) * pitch + c0 + c] =
 *   table[63 - clz(m)], table = 64 values of the element type ON THE DEVICE (int8 for elem_size 1, float32 for 4).  Pixels with m == 0
 *   are NOT written.  out is a raster of H rows of W pixels with a row pitch of `pitch` elements (pitch >= W); the rectangle lies inside
 *   it: 0 <= r0, r0 + Hp <= H, 0 <= c0, c0 + Wp <= W.  int8 pixels are stored as single bytes, except that a thread whose four
 *   consecutive pixels are all written and start at a 4-byte aligned address stores them as one 32-bit word (the word is then private to
 *   that thread): no two lanes ever read-modify-write one word, whatever pitch and c0 are.  written (uint64, or NULL) += the number of
 *   pixels stored: summed per thread, wave and workgroup, one 64-bit atomic add per workgroup.  A workgroup owns whole rows; no kernel
 *   waits on another workgroup; every launch does a fixed amount of work.  Hp * Wp <= 2^31 - 1, H * pitch < 2^40; canvas and written
 *   8-byte aligned, float32 table / out 4-byte aligned.  Hp * Wp = 0 returns IG_OK without touching a pointer.
 * ig_label_cells: raster (ny * S, nx * S), int8 (elem_size 1) or float32 (4), contiguous, is cut into ny x nx cells of S x S pixels, cell
 *   (cy, cx) numbered cy * nx + cx.  valid (ny * nx uint64) += the cell's VALID pixels: != ignore for int8, not NaN for float32 (ignore is
 *   not read).  hist (ny * nx, K) uint64 += for int8 with K > 0 the valid pixels per value in [0, K); a value outside [0, K) counts as
 *   valid but goes in no histogram cell.  The caller zeroes both.  One workgroup owns up to 64 rows of one cell; lanes of a wave that
 *   hold the same value add once to an LDS table of 32-bit cells, which reaches memory as one 64-bit atomic add per non-empty cell;
 *   integer sums, bit-identical from run to run.  1 <= S <= 2^15, ny * nx <= 2^31 - 1, ny * S * nx * S < 2^40, 0 <= K <= 128 (K > 0 needs
 *   elem_size 1), ignore fits int8.  ny * nx = 0 returns IG_OK without touching a pointer. */
int ig_burn_resolve(const unsigned long long* canvas, int Hp, int Wp, const void* table, int elem_size, void* out, int H, int W, long pitch,
                    int r0, int c0, unsigned long long* written, void* stream);
int ig_label_cells(const void* raster, int ny, int nx, int S, int elem_size, int ignore, int K, unsigned long long* valid,
                   unsigned long long* hist, void* stream);
/* Overview pyramids and tile layout for Cloud Optimized GeoTIFF output (cog.hip; the reference calls gdal_translate -of COG instead).
 * Level 0 is the raster itself, H_0 x W_0; level k has H_k = ceil(H_{k-1} / 2) rows and W_k = ceil(W_{k-1} / 2) columns.  Pixel (r, c) of
 * level k has as CHILDREN the pixels (2r..2r+1, 2c..2c+1) of level k-1 that lie inside that level: 1, 2 or 4 of them, in row-major order.
 * Levels cascade: level k is computed from level k-1, never from level 0.  H * W <= 2^31 - 1, 1 <= levels <= 12.
 * MODE rule (int8 class maps with a fill value): children equal to fill are ignored; if none is left the result is fill; otherwise the
 *   result is the value with the most children, ties go to the smallest value (as signed int8).  The rule does not depend on child order,
 *   so it commutes with the eight D4 maps of the square whenever H and W are multiples of 2^levels.  It makes no claim of equality with
 *   GDAL's MODE resampling, which decides ties by position.
 * MEAN rule (float32 rasters with NaN as NODATA, band by band): the valid children are those that are not NaN; the result is their float32
 *   sum taken in row-major child order (the first valid child, then one IEEE addition per further one), divided by their count as float32
 *   with IEEE round-to-nearest division; NaN (the quiet NaN 0x7fc00000) if there are none.  Bit-reproducible and equal to numpy float32
 *   arithmetic in the same order.
 * One workgroup owns a 64 x 64 block of the source with its origin at multiples of 64, so every 2 x 2 group of every level nests in one
 * block: the block is read from memory once (16-byte loads where the row pitch and the pointer allow, single elements elsewhere) and
 * levels 1..6 come out of LDS; for more than six levels the entry point launches again on level 6.  Every output element is written
 * exactly once; no kernel waits on another workgroup; results are bit-identical from run to run.  H * W = 0 (or bands = 0) returns IG_OK
 * without touching a pointer.
 * ig_overview_mode: src (H, W) int8 -> dst int8: levels 1..levels by the MODE rule back to back in level order (sum of H_k * W_k bytes).
 *   counts, when not NULL, is (ncls + 1) uint64 and accumulates (the caller zeroes it) the class histogram of src: counts[v] += 1 for a
 *   pixel whose value v is a class in [0, ncls) and is not fill, counts[ncls] += 1 for fill or any value that is not a class;
 *   1 <= ncls <= 127.  Integer sums: runs of equal classes are merged per thread and wave, counted per workgroup in LDS and added with one
 *   64-bit atomic per non-empty cell and workgroup.
 * ig_overview_mean: src (bands, H, W) float32 -> dst float32: levels 1..levels by the MEAN rule, level-major, each level (bands, H_k, W_k).
 * ig_cog_tiles: src (bands, H, W) of elem_size = 1, 2 or 4 bytes -> dst (bands, ny, nx, tile, tile) with ny = ceil(H / tile),
 *   nx = ceil(W / tile), tile a multiple of 16; dst 16-byte aligned.  The part of the edge tiles outside the raster holds the low elem_size
 *   bytes of pad (the fill value, or the NaN bit pattern).  predictor 1 copies; predictor 2 (integers only: is_float must be 0) applies
 *   TIFF horizontal differencing along each tile row of the padded tile, out[x] = v[x] - v[x-1] for x > 0, with wrap-around arithmetic in
 *   the element's width.  A gather: every output element is written exactly once. */
int ig_overview_mode(const signed char* src, int H, int W, int fill, int ncls, int levels, signed char* dst, unsigned long long* counts,
                     void* stream);
int ig_overview_mean(const float* src, int bands, int H, int W, int levels, float* dst, void* stream);
int ig_cog_tiles(const void* src, int bands, int H, int W, int elem_size, int is_float, int tile, unsigned pad, int predictor, void* dst,
                 void* stream);
/* Mosaic of per-chip rasters on one canvas (mosaic.hip; the reference runs gdal_merge.py over the prediction folder instead).  nchips
 * rectangles lie on an H x W canvas, H * W <= 2^31 - 1.  Chip i has rects[i] = (row0, col0, h, w) (int32; h, w in [1, 2^30], row0 and col0
 * in [-2^30, 2^30]) and its h * w pixels row-major at element offset starts[i] (int64, >= 0) of one packed buffer `chips`; pixel (r, c) of
 * the chip lies on canvas pixel (row0 + r, col0 + c).  A rectangle may hang over the canvas edge, negative row0 / col0 included: only the
 * part inside the canvas counts.  Chip i CONTRIBUTES to a canvas pixel when it covers the pixel and its value there is not transparent:
 * for int8 class maps (elem_size 1) transparent means == fill, for float32 rasters (elem_size 4) it means NaN.  The contributors of a
 * pixel are ordered by chip index.  The value of a canvas pixel by rule:
 *   0 LAST: the value of the contributor with the largest index (gdal_merge -n fill: later files win);
 *   1 FIRST: the value of the contributor with the smallest index;
 *   2 MODE (int8 only): the value that the most contributors have, ties go to the smallest value (as signed int8): the tie rule of
 *     ig_overview_mode.  It does not depend on the order of the chips;
 *   3 MEAN (float32 only): the float32 sum of the contributors in index order (the first, then one IEEE addition per further one),
 *     divided by their count as float32 with IEEE round-to-nearest division: equal to numpy float32 arithmetic in the same order;
 *   no contributor: fill for int8, the quiet NaN 0x7fc00000 for float32.
 * LAST and FIRST copy bits: a float keeps its sign of zero.  cover (H, W) uint8, when not NULL, receives the number of contributors of
 * every pixel, saturating at 255.
 * ig_mosaic_paste: a gather.  One workgroup owns one 64 x 64 block of the canvas with its origin at multiples of 64 (the blocking of
 *   ig_overview_mode, which may read the canvas next); blocks are numbered row-major, ceil(W / 64) to a row.  bin_ptr (blocks + 1 int32,
 *   ascending from 0) and bin_idx are a CSR list made by the caller: bin_idx[bin_ptr[b] .. bin_ptr[b + 1]) holds, in ASCENDING order, the
 *   indices of all chips whose rectangle intersects block b (more are harmless, fewer lose contributors).  A list may have any length; it is
 *   staged through LDS 256 entries at a time.  A block with an empty list is written as fill / NaN.  Every pixel of dst (and cover) is
 *   written exactly once, by the thread that computed it; no atomics, no kernel waits on another workgroup; results are bit-identical
 *   from run to run.  A chip index outside [0, nchips), a rectangle outside the bounds above or a negative start contributes nothing;
 *   the caller guarantees that starts[i] + h * w lies inside chips.  dst 16-byte aligned, rects 16-byte aligned.  fill must fit int8 (for
 *   float32 it is ignored).  H * W = 0 returns IG_OK without touching a pointer; nchips = 0 writes fill / NaN everywhere and reads none
 *   of chips, starts, rects, bin_ptr, bin_idx.  ceil(H / 64) <= 65535. */
int ig_mosaic_paste(const void* chips, const long long* starts, const int* rects, int nchips, const int* bin_ptr, const int* bin_idx, int H,
                    int W, int elem_size, int rule, int fill, void* dst, unsigned char* cover, void* stream);
/* Reprojection and resampling of north-up rasters between grids (warp.hip; the reference's viewer reprojects with rasterio before display,
 * apps/viz.py).  A COORDINATE SYSTEM is five doubles (kind, lon0, k0, FE, FN): kind 0 geographic WGS84 (x = longitude, y = latitude, degrees;
 * the other four are ignored but compared), kind 1 transverse Mercator on WGS84 (a = 6378137, 1/f = 298.257223563) with central meridian
 * lon0 (degrees), scale k0, false easting FE and false northing FN (metres; UTM north: 0.9996, 500000, 0; south: FN = 1e7), kind 2
 * spherical web Mercator EPSG:3857 (R = 6378137; the other four ignored).  Transverse Mercator is the Krueger series in the third
 * flattening n to n^6, forward and inverse, in float64: xi + i eta = xi' + i eta' + sum_j alpha_j sin(2j (xi' + i eta')), j = 1..6, summed
 * by the angle-addition recurrence from one sincos and one sinh / cosh pair; the geographic latitude comes from the conformal one by
 * three Newton steps on tan(latitude) from tau'/(1 - e^2) (no data-dependent loop).
 * ACCURACY of that rule, measured against a 50-digit reference that shares nothing with the series (tests/projection_truth.py: the
 * conformal map from its definition, by complex Newton and quadrature; fixture tests/golden/projection_truth.npz), as |float64 evaluation
 * of the rule (tests/warp_reference.py) - truth| on the ground.  Within 40 degrees of the central meridian, latitudes to 89.9: forward
 * <= 3.8e-9 m, inverse (E - FE within 4800 km) <= 7.5e-8 m, and <= 4.1e-7 m within 0.6 degrees of a pole, which is the rounding of that
 * evaluation (instageo_amd/crs.py stays within 2e-9 m there); web Mercator and the chains between systems <= 5.8e-8 m.  The device is
 * held to 1e-6 m on all of these (tests/test_gpu_projection_truth.py).  The PICKS of the value kernels (ig_warp, ig_chip_warp,
 * ig_s1_chip_warp, ig_s2_chip_warp, ig_tile_render) are held to the same truth at 10 to 30 m pixels: outside 1e-6 m + 4 ulp of a pixel
 * boundary the pixel read must equal the true pick (tests/test_cpu_warp_picks.py, tests/test_gpu_warp_picks.py, on
 * tests/warp_pick_reference.py and tests/golden/warp_pick_truth.npz).  BEYOND 40 degrees the truncated series itself is off, forward,
 * worst per band of |longitude - lon0|:
 *     latitude    (40, 50]    (50, 60]    (60, 70]    (70, 79.9]
 *        0        1.3e-7 m    1.1e-5 m    4.8e-3 m    118 m      (4.7 m at 77.5 degrees)
 *       20        3.8e-8 m    1.1e-6 m    3.9e-5 m    1.1e-3 m
 *       45        2.1e-9 m    5.7e-9 m    1.3e-8 m    3.5e-8 m
 * and <= 3.5e-8 m everywhere from 45 degrees of latitude up.  So the domain declared below (|longitude - lon0| < 80 degrees) reaches into
 * a region where, near the equator, the coordinates are wrong by centimetres from 70 degrees on and by about 100 m at its edge; the
 * kernels are exact evaluations of the series there (within twice its own error), not of the projection.  Sources that far from their
 * meridian are off-raster in every caller.  A GRID is four doubles (X0, Y0, sx, sy), the outer
 * corner of the top-left pixel and the positive pixel sizes, with its size (h, w): the centre of pixel (r, c) lies at x = X0 + (c + 0.5) sx,
 * y = Y0 - (r + 0.5) sy, and the point (x, y) has the pixel coordinates u = (x - X0) / sx, v = (Y0 - y) / sy, so that pixel (r, c) covers
 * [c, c + 1) x [r, r + 1).
 * The source coordinates (u, v) of a destination pixel: its centre (x, y) -> (longitude, latitude) by the inverse projection of the
 * destination system -> (x', y') by the forward projection of the source system -> (u, v) on the source grid.  (NaN, NaN) OUTSIDE THE
 * DOMAIN: a longitude or latitude that is not finite, |latitude| > 89.9 degrees, for a transverse Mercator destination |xi'| > pi / 2, and
 * for a transverse Mercator source |longitude - lon0| >= 80 degrees (the difference taken into [-180, 180] by IEEE remainder).  Where the
 * five doubles of the two systems are equal (compared as doubles) no projection is evaluated: (u, v) is the affine arithmetic above.
 * ig_warp_coords: uv (2, H, W) float64 = the u plane, then the v plane, of the H x W destination grid in the one source grid; dst_crs and
 *   src_crs point to 5, dst_grid and src_grid to 4 doubles ON THE DEVICE.  H * W = 0 returns IG_OK without touching a pointer.
 * ig_warp: resamples nsrc <= 8 sources onto the destination in one launch.  Source i has src_crs[5 i ..], src_grid[4 i ..], src_size[2 i ..]
 *   = (h, w) (int32, in [1, 2^30]) and its h * w pixels row-major at element offset starts[i] (int64, >= 0) of the packed buffer src.
 *   A value is TRANSPARENT as in the mosaic paste: int8 (elem_size 1) == fill, float32 (elem_size 4) NaN.
 *   resampling 0 NEAREST (int8, float32): c = floor(u), r = floor(v); the source contributes its pixel (r, c) when 0 <= r < h, 0 <= c < w
 *     and the value is not transparent; bits are copied.
 *   resampling 1 BILINEAR (float32 only): c0 = floor(u - 0.5), r0 = floor(v - 0.5), wx = u - 0.5 - c0, wy = v - 0.5 - r0; the neighbours
 *     (r0, c0), (r0, c0 + 1), (r0 + 1, c0), (r0 + 1, c0 + 1) have the float64 weights (1 - wx)(1 - wy), wx (1 - wy), (1 - wx) wy, wx wy.  A
 *     neighbour counts when it lies inside the source, is not NaN and has a weight > 0; the value is sum(weight * value) / sum(weight)
 *     over those that count, both sums in float64 in the order above, rounded once to float32.  None counts: no contribution.
 *   (u, v) = (NaN, NaN) never contributes.  rule 0 LAST: the contributing source with the largest index gives the value; 1 FIRST: the
 *   smallest; no contributor: fill (int8) or the quiet NaN 0x7fc00000.  src_id (H, W) uint8, when not NULL, receives that index, 255 for
 *   none.  One workgroup owns one 64 x 64 block of the destination with its origin at multiples of 64 (the blocking of ig_mosaic_paste and
 *   ig_overview_mode), blocks numbered row-major; bin_ptr (blocks + 1 int32, ascending from 0) / bin_idx is the caller's CSR list of the
 *   sources that can reach each block, in ASCENDING order (more are harmless, fewer lose contributors).  The longitude and latitude of
 *   a pixel are computed once and reused for every source, and sources of one coordinate system share the forward projection.  Every
 *   pixel of dst (and src_id) is written exactly once by the thread that computed it, a wave stores 64 consecutive pixels of a row; no
 *   atomics, no kernel waits on another workgroup; results are bit-identical from run to run.  A source index outside [0, nsrc), a size
 *   outside the bounds, a grid whose pixel sizes are not finite and positive or a negative start contributes nothing; the caller guarantees that
 *   starts[i] + h * w lies inside src.  H * W <= 2^31 - 1, ceil(H / 64) <= 65535; H * W = 0 returns IG_OK without touching a pointer;
 *   nsrc = 0 writes fill / NaN everywhere and reads none of the source arguments. */
int ig_warp_coords(const double* dst_crs, const double* dst_grid, int H, int W, const double* src_crs, const double* src_grid, double* uv,
                   void* stream);
int ig_warp(const void* src, const long long* starts, const double* src_crs, const double* src_grid, const int* src_size, int nsrc,
            const int* bin_ptr, const int* bin_idx, const double* dst_crs, const double* dst_grid, int H, int W, int elem_size, int resampling,
            int rule, int fill, void* dst, unsigned char* src_id, void* stream);
/* Chips and label maps cut from a satellite tile (chips.hip; the reference's instageo/data chip creator: apply_mask, decode_fmask_value,
 * create_segmentation_map, mask_segmentation_map, get_chip_coords and the loop of create_and_save_chips_with_seg_maps).  THE RULE:
 * tile (T * C, H, W) int16: band b belongs to date b / C.  fmask (T, H, W) uint8, or NULL (no masking).  origins (n, 2) int32 = (row0, col0):
 *   chip i is the S x S window of the tile with its top-left pixel at (row0, col0); it lies wholly inside the tile, 0 <= row0 <= H - S,
 *   0 <= col0 <= W - S.  Origins need not be multiples of anything and chips may overlap.
 * mask_bits: the OR of 1 << position over the requested mask types, positions cloud 1, near_cloud_or_shadow 2, cloud_shadow 3, water 5
 *   (decode_fmask_value(v, p) = (v >> p) & 1).  Date t is MASKED at a pixel when fmask[t] & mask_bits != 0.
 *   strategy 0 EACH: the C bands of date t become no_data where date t is masked.  strategy 1 ANY: all T * C bands become no_data where
 *   any date is masked.  With clip != 0 every value v then becomes min(max(v, clip_lo), clip_hi): clipping comes after masking.
 * Per chip: chips (n, T * C, S, S) int16, the values by the rule above; valid_values[i] int32 += the number of its values that differ from
 *   no_data (the caller zeroes it); validity (n, S, S) uint8, or NULL: bit 0 is set when all T * C values of the pixel differ from
 *   no_data, bit 1 when at least one differs (the reference's `any` and `each` rules of mask_segmentation_map).
 * Label maps.  A point is (row, col, index) int32: its pixel on the TILE and its original index in the table of P points, whose labels
 *   (P elements, int16 when elem_size = 2, float32 when 4) are looked up by that index.  The points are grouped by chip in CSR form:
 *   pts[ptr[i] .. ptr[i + 1]) are those of chip i (ptr: n + 1 int32, ascending from 0); a point that falls in two overlapping chips is
 *   listed under both.  With (pr, pc) = (row - row0, col - col0), pixel (r, c) of the chip is COVERED by the point when |r - pr| <= w
 *   and |c - pc| <= w: the window is intersected with the chip and never spills into a neighbouring one.  Among the covering points the one
 *   with the largest original index WINS (numpy's repeated-index assignment in the reference, made explicit) and the pixel gets its
 *   label; a pixel with no covering point gets -1; a pixel whose validity bit (valid_bit 1: bit 0, `any`; 2: bit 1, `each`; 0: no
 *   validity plane) is clear gets -1.  maps (n, S, S) int16 or float32: float labels are copied bit for bit.  valid_labels[i] int32 += the
 *   pixels != -1; hist (n, K) int32 += for int16 maps the pixels per label in [0, K), K <= 256 (labels outside are not counted); K = 0 or
 *   hist NULL: no histogram.  The caller zeroes valid_labels and hist.
 * All results are integers or copies, and unique: the same bits for any launch geometry, run after run.
 * ig_chip_cut: a gather.  One workgroup of 256 threads owns a block of 16 rows x 128 columns of one chip, a thread 8 consecutive pixels of
 *   a row.  It reads the T fmask bytes of its pixels once and forms the per-date masks, then streams the T * C values through and stores
 *   each once; the validity plane comes from the same pass.  The access width is chosen per row segment from the address (16, 8, 4 or 2
 *   bytes: the row pitch of a 3660-pixel tile is 8 mod 16, so alignment alternates from row to row); a segment that crosses the chip edge
 *   goes element by element.  valid_values is reduced in the wave and the workgroup and added with one integer atomic per workgroup.
 *   T <= 32, 1 <= S <= min(H, W), no_data and the clip range fit int16, T * C * S * S <= 2^31 - 1 (valid_values is int32),
 *   n * T * C * S * S and T * C * H * W below 2^40.  The origins are on
 *   the device: the caller guarantees them (ops.chip_cut checks them on the host before the upload); a chip whose origin breaks the bounds
 *   is left unwritten and nothing is read for it, so no read leaves the tile.  n = 0 returns IG_OK without touching a pointer.
 * ig_chip_labels: one workgroup owns a 64 x 64 block of one chip's label map with an int32 winner plane in LDS (16 KiB) set to -1; its
 *   threads walk the chip's points, skip those whose window misses the block, and apply an LDS atomic max of the original index over the
 *   window pixels inside the block; after a barrier each thread resolves winner -> label, applies the validity bit and stores its pixels
 *   once; valid_labels and the histogram are tallied in LDS and added with integer atomics.  Atomic max and integer adds commute; no
 *   workgroup waits on another.  0 <= w <= 2^20, 0 <= K <= 256 (K > 0 needs elem_size 2).  A point outside its chip or with an index
 *   outside [0, P) paints nothing (ops.chip_labels refuses both on the host). */
int ig_chip_cut(const short* tile, const unsigned char* fmask, const int* origins, int n, int T, int C, int H, int W, int S, int mask_bits,
                int strategy, int no_data, int clip, int clip_lo, int clip_hi, short* chips, int* valid_values, unsigned char* validity,
                void* stream);
int ig_chip_labels(const int* origins, int n, int S, const int* ptr, const int* pts, const void* labels, long P, int elem_size, int w,
                   const unsigned char* validity, int valid_bit, int K, void* maps, int* valid_labels, int* hist, void* stream);
/* Chips cut from Sentinel-2 L2A planes of several resolutions under the scene classification (s2_chips.hip; the reference's
 * instageo/data/s2_utils.py: S2PointsPipeline on a stack that stackstac has resampled onto one resolution, create_mask_from_scl,
 * MASK_DECODING_POS["S2"], apply_mask).  THE RULE:
 * Planes.  T * C band planes, uint16, band b of date b / C, and T SCL planes, uint8, or none (scl NULL: no masking).  Plane k has its own
 *   size H_k x W_k and its own square pixel size p_k, a positive integer (metres).  All planes and the output grid SHARE THE TOP-LEFT
 *   CORNER (Sentinel-2 resolutions do; the host checks the tiepoints, the coordinate system and that every pixel scale is an integer).
 * Packing.  The band planes lie row-major in one uint16 buffer `bands`, plane k at element offset starts[k] (int64, >= 0), as ig_warp packs
 *   its sources; the SCL planes in one uint8 buffer `scl`, plane t at scl_starts[t].  geom holds (H_k, W_k, p_k) as int32, 3 per plane, the
 *   T * C bands first and then, when scl is not NULL, the T SCL planes.  starts, scl_starts and geom are ON THE DEVICE.
 * Output grid.  Pixel size p_o (integer metres), H_o x W_o pixels.  origins (n, 2) int32 = (row0, col0) on the OUTPUT grid: chip i is its
 *   S x S window, wholly inside, 0 <= row0 <= H_o - S, 0 <= col0 <= W_o - S.
 * Source pixel.  Output pixel (r, c) reads plane k at rs = ((2 r + 1) p_o) div (2 p_k), cs = ((2 c + 1) p_o) div (2 p_k), floor division in
 *   exact integers: the NEAREST rule of ig_warp (the floor of the centre's source coordinate) without float64.  With p_k = 2 p_o a source
 *   pixel fans out into 2 x 2 output pixels (rs = r div 2); with p_o = 2 p_k the output picks source pixel (2 r + 1, 2 c + 1).  An (rs, cs)
 *   outside the plane gives the band value 0 and the SCL class 0 (stackstac's fill_value).
 * Value chain of a band value v (an integer in [0, 65535]):
 *   1. boa_offset > 0 and v != 0: v = max(v - boa_offset, 0) (the +1000 BOA_ADD_OFFSET of processing baseline >= 04.00; 0, the default,
 *      is the reference, which does not subtract);
 *   2. date t is MASKED at the pixel when scl_t < 32 and (class_bits >> scl_t) & 1 (class_bits: the OR of 1 << class over the requested
 *      SCL classes, cloud 8 and 9, water 6, ...).  strategy 0 EACH / 1 ANY exactly as in ig_chip_cut; a masked value becomes no_data;
 *   3. range != 0: a value outside [range_lo, range_hi] becomes no_data (the reference's chip.where((chip >= 0) & (chip <= 10000), 0): it
 *      REPLACES the value, it does not clip, unlike the HLS rule).
 * Per chip: chips (n, T * C, S, S) uint16; valid_values[i] int32 += the values that differ from no_data (the caller zeroes it); validity
 *   (n, S, S) uint8, or NULL, with the bits of ig_chip_cut (bit 0: all values of the pixel differ from no_data, bit 1: at least one
 *   does): it feeds ig_chip_labels unchanged.
 * All results are integers or copies, and unique: the same bits for any launch geometry, run after run.
 * ig_s2_chip_cut: a gather in the blocking of ig_chip_cut.  One workgroup of 256 threads owns 16 rows x 128 columns of one chip, a thread 8
 *   consecutive output pixels of a row.  The SCL bytes are read once into a per-pixel date mask, then the T * C bands stream through (gather,
 *   offset, mask, range, count, one 16-byte store); the validity byte comes from the same pass.  The read side is chosen per plane,
 *   uniformly for the workgroup: p_k = p_o reads the 8 pixels in the widest units the address allows; p_k = 2 p_o reads the 4 or 5 source
 *   pixels (odd first column: 5) the 8 outputs come from, 8 / 4 / 2 bytes at a time, and expands them in registers; any other ratio, and
 *   any segment that crosses the chip's or the plane's edge, goes element by element: one 64-bit division for the thread's first pixel,
 *   then quotient-and-remainder steps.  valid_values is reduced in the wave and the workgroup and added with one integer atomic per
 *   workgroup; no workgroup waits on another.
 *   1 <= T <= 32, C >= 1, S >= 1, S <= min(H_o, W_o), 1 <= p_o <= 2^15, H_o * W_o <= 2^31 - 1, T * C * S * S <= 2^31 - 1 (valid_values is
 *   int32), n * T * C * S * S < 2^40, no_data, boa_offset and the range inside [0, 65535] with range_lo <= range_hi; these are refused
 *   before any launch.  Per plane 1 <= p_k <= 2^15, H_k, W_k >= 1, H_k * W_k <= 2^31 - 1, 0 <= starts[k] and the packed totals below
 *   2^40: the tables are on the device, so ops.s2_chip_cut checks them (and the origins) on the host before the upload, and the kernel is
 *   the second fence: a plane whose entry breaks these bounds reads nothing and gives the fill, a chip whose origin breaks its bounds is
 *   left unwritten and nothing is read for it.  The caller guarantees that starts[k] + H_k * W_k lies inside its buffer; no read leaves a
 *   plane.  bands, chips 2-byte, the int32 arrays 4-byte, the int64 arrays 8-byte aligned.  n = 0 returns IG_OK without touching a pointer. */
int ig_s2_chip_cut(const unsigned short* bands, const long long* starts, const unsigned char* scl, const long long* scl_starts,
                   const int* geom, const int* origins, int n, int T, int C, int Ho, int Wo, int po, int S, unsigned class_bits, int strategy,
                   int no_data, int boa_offset, int range, int range_lo, int range_hi, unsigned short* chips, int* valid_values,
                   unsigned char* validity, void* stream);
/* Chips warped onto label grids (raster_chips.hip; the reference's instageo/data/raster_chip_creator.py: HLSRasterPipeline.process_row on
 * a stack that stackstac has resampled onto the label's coordinate system and resolution, geo_utils.slice_xr_dataset, apply_mask,
 * mask_segmentation_map).  THE RULE:
 * tile (T * C, H, W) int16 and fmask (T, H, W) uint8 or NULL as for ig_chip_cut.  src_crs (5 doubles) and src_grid (4 doubles) describe
 *   the stack, dst_crs (5 doubles) the one coordinate system of the n chips, dst_grids (n, 4) doubles the grid of every chip, all ON THE
 *   DEVICE and exactly as ig_warp defines coordinate systems and grids.  Every chip is S x S.
 * The centre of pixel (r, c) of chip i has the source coordinates (u, v) by the chain of ig_warp / ig_warp_coords: where the five doubles
 *   of the two systems are equal the affine arithmetic alone, otherwise inverse projection of dst_crs and forward projection of src_crs,
 *   (NaN, NaN) outside the domain.  NEAREST: cs = floor(u), rs = floor(v), tested on the float64 values.  When 0 <= rs < H and
 *   0 <= cs < W the pixel takes the T * C values and the T Fmask bytes of source pixel (rs, cs); otherwise (NaN included) it takes no_data
 *   in every band and Fmask 0 (stackstac's fill_value).  A destination grid, or a source grid, whose values are not finite or whose pixel
 *   sizes are not positive gives a chip that is no_data everywhere; no read leaves the tile.
 * Then the rule of ig_chip_cut applies unchanged: date t is masked where fmask[t] & mask_bits != 0, strategy 0 EACH / 1 ANY, the clip
 *   after the masking, chips (n, T * C, S, S) int16, valid_values[i] += the values that differ from no_data, validity (n, S, S) uint8 or
 *   NULL with bit 0 = all values of the pixel differ from no_data, bit 1 = at least one does.
 * Label maps go through the same pass.  labels (n, S, S), int8 (elem_size 1) or float32 (elem_size 4), or NULL (then maps, valid_labels
 *   and hist are not touched).  The output pixel is the input pixel, bit for bit, except that it becomes -1 when valid_bit != 0 and the
 *   pixel's validity bit is clear (valid_bit 1: bit 0, `any`; 2: bit 1, `each`; 0: no label masking, the reference's qa_check = false),
 *   or when it is a float32 NaN (the reference's where(~isnan, -1)).  valid_labels[i] int32 += the output pixels != -1; hist (n, K) int32
 *   += for int8 maps the output pixels per value in [0, K), K <= 128 (values outside are not counted); K = 0: no histogram, hist may be
 *   NULL.  The caller zeroes valid_values, valid_labels and hist.
 * All results are integers or copies, and unique: the same bits for any launch geometry, run after run.
 * ig_chip_warp: a gather, one launch for all n chips.  One workgroup of 256 threads owns a 64 x 64 block of one chip (the blocking of
 *   ig_warp and ig_chip_labels); a wave owns 64 consecutive pixels of a row and stores them with one instruction, a thread takes 16 rows.
 *   A thread evaluates the float64 chain ONCE per pixel and keeps the source offset rs * W + cs (int32, -1 for none) of its 16 pixels in
 *   registers, gathers their T Fmask bytes into one 32-bit date mask per pixel, then streams the T * C bands: gather, mask, clip, one
 *   store.  The validity byte and the label pixel come from the same registers.  valid_values and valid_labels are summed in the wave
 *   and the workgroup, the histogram in LDS, and added with integer atomics, one set per workgroup; no workgroup waits on another.
 *   1 <= T <= 32, C >= 1, 1 <= S <= 2^15, H * W <= 2^31 - 1, T * C * S * S <= 2^31 - 1 (valid_values is int32), n * T * C * S * S < 2^40,
 *   no_data and the clip range fit int16, elem_size 1 or 4 (also without labels), 0 <= K <= 128 and K > 0 needs elem_size 1 and labels,
 *   valid_bit 0, 1 or 2.  tile, chips 2-byte, the int32 arrays and float32 labels / maps 4-byte, the float64 arrays 8-byte aligned.
 *   n = 0 returns IG_OK without touching a pointer. */
int ig_chip_warp(const short* tile, const unsigned char* fmask, const double* src_crs, const double* src_grid, const double* dst_crs,
                 const double* dst_grids, int n, int T, int C, int H, int W, int S, int mask_bits, int strategy, int no_data, int clip,
                 int clip_lo, int clip_hi, const void* labels, int elem_size, int valid_bit, int K, short* chips, int* valid_values,
                 unsigned char* validity, void* maps, int* valid_labels, int* hist, void* stream);
/* Sentinel-2 chips warped onto label grids (s2_raster_chips.hip; the reference's instageo/data/raster_chip_creator.py:
 * S2RasterPipeline.process_row on a stack that stackstac has resampled onto the label's coordinate system and resolution, then
 * create_mask_from_scl, apply_mask, the range replacement and mask_segmentation_map).  THE RULE:
 * Sources.  T * C band planes, uint16, band b of date b / C, and T SCL planes, uint8, or none (scl NULL: no masking), packed exactly as
 *   ig_s2_chip_cut packs them: `bands` with starts[k] (int64 element offsets, >= 0), `scl` with scl_starts[t].  All planes are in ONE
 *   coordinate system src_crs (5 doubles, as ig_warp defines them) but need not share a lattice, nor a corner: every plane belongs to
 *   one of G geometry classes, 1 <= G <= 8.  plane_class int32, one entry per band plane and then, when scl is not NULL, one per SCL
 *   plane, in [0, G); class_grid (G, 4) doubles = (X0, Y0, sx, sy) as ig_warp defines a grid; class_size (G, 2) int32 = (H, W).  A real
 *   product has 2 or 3 classes (10 m, 20 m, 60 m).  All tables are ON THE DEVICE.
 * Destination.  dst_crs (5 doubles) the one coordinate system of the n chips, dst_grids (n, 4) doubles the grid of every chip, ON THE
 *   DEVICE; every chip is S x S: exactly as ig_chip_warp.
 * Coordinates.  The centre of pixel (r, c) of chip i is taken to source map coordinates (x, y) ONCE, by the chain of ig_warp /
 *   ig_chip_warp: where the five doubles of the two systems are equal the affine arithmetic alone, otherwise inverse projection of
 *   dst_crs and forward projection of src_crs, (NaN, NaN) outside the domain.  For class g: u_g = (x - X0_g) / sx_g,
 *   v_g = (Y0_g - y) / sy_g, the arithmetic of ig_chip_warp for its single grid, so with one class the source offsets are
 *   ig_chip_warp's bit for bit.  NEAREST: cs = floor(u_g), rs = floor(v_g), tested on the float64 values.  When 0 <= rs < H_g and
 *   0 <= cs < W_g the pixel reads source pixel (rs, cs) of every plane of class g; otherwise (NaN included) it takes no_data in every
 *   band of class g and SCL class 0 in every SCL plane of class g; the other classes are unaffected.  A destination grid, or ANY of the
 *   G class grids, whose values are not finite or whose pixel sizes are not positive gives a chip that is no_data everywhere (and
 *   SCL class 0).  No read leaves a plane.
 * Value chain of a band value v that was READ (a fill stays no_data), that of ig_s2_chip_cut unchanged:
 *   1. boa_offset > 0 and v != 0: v = max(v - boa_offset, 0);
 *   2. date t is MASKED at the pixel when scl_t < 32 and (class_bits >> scl_t) & 1; strategy 0 EACH / 1 ANY as in ig_chip_cut; a masked
 *      value becomes no_data;
 *   3. range != 0: a value outside [range_lo, range_hi] becomes no_data (replaced, not clipped).
 * chips (n, T * C, S, S) uint16; valid_values[i] int32 += the values that differ from no_data; validity (n, S, S) uint8 or NULL with
 *   the bits of ig_chip_cut (bit 0: all values of the pixel differ from no_data, bit 1: at least one does).
 * Label maps: labels, elem_size, valid_bit, K, maps, valid_labels and hist exactly as in ig_chip_warp (int8 or float32, NaN -> -1,
 *   -1 where the validity bit of valid_bit is clear, the histogram of int8 values in [0, K)).  The caller zeroes valid_values,
 *   valid_labels and hist.
 * All results are integers or copies, and unique: the same bits for any launch geometry, run after run.
 * ig_s2_chip_warp: a gather in the blocking of ig_chip_warp, one launch for all n chips.  One workgroup of 256 threads owns a 64 x 64
 *   block of one chip; a wave owns 64 consecutive pixels of a row and stores them with one instruction, a thread takes 16 rows.  A
 *   thread evaluates the float64 chain ONCE per pixel and keeps (x, y) of its 16 pixels in registers.  The int32 source offsets
 *   rs * W_g + cs (-1 for none) are held for ONE class at a time: class by class the thread derives its 16 offsets (two divisions per
 *   pixel), gathers the SCL bytes of that class's SCL planes into the 32-bit date mask per pixel, and in a second sweep over the classes
 *   derives the offsets again and streams that class's bands: gather, offset, mask, range, count, one store.  (16 x G offsets do not fit
 *   the register file for G = 8; the affine step is cheap next to the projection.)  The validity byte and the label pixel come from
 *   the same registers; valid_values and valid_labels are summed in the wave and the workgroup, the histogram in LDS, and added with
 *   integer atomics, one set per workgroup; no workgroup waits on another.
 *   1 <= T <= 32, C >= 1, 1 <= S <= 2^15, 1 <= G <= 8, T * C * S * S <= 2^31 - 1 (valid_values is int32), n * T * C * S * S < 2^40,
 *   no_data, boa_offset and the range inside [0, 65535] with range_lo <= range_hi, elem_size 1 or 4 (also without labels),
 *   0 <= K <= 128 and K > 0 needs elem_size 1 and labels, valid_bit 0, 1 or 2; these are refused before any launch.  Per table entry
 *   0 <= plane_class < G, H_g, W_g >= 1, H_g * W_g <= 2^31 - 1, 0 <= starts[k]: the tables are on the device, so ops.s2_chip_warp checks
 *   them on the host before the upload, and the kernel is the second fence: a plane whose class index or start breaks these bounds,
 *   and every plane of a class whose size does, reads nothing and gives the fill (no_data, SCL class 0).  The caller guarantees that
 *   starts[k] + H_g * W_g lies inside its buffer.  bands, chips 2-byte, the int32 arrays and float32 labels / maps 4-byte, the int64
 *   and float64 arrays 8-byte aligned.  n = 0 returns IG_OK without touching a pointer. */
int ig_s2_chip_warp(const unsigned short* bands, const long long* starts, const unsigned char* scl, const long long* scl_starts,
                    const int* plane_class, const double* class_grid, const int* class_size, int G, const double* src_crs,
                    const double* dst_crs, const double* dst_grids, int n, int T, int C, int S, unsigned class_bits, int strategy, int no_data,
                    int boa_offset, int range, int range_lo, int range_hi, const void* labels, int elem_size, int valid_bit, int K,
                    unsigned short* chips, int* valid_values, unsigned char* validity, void* maps, int* valid_labels, int* hist,
                    void* stream);
/* Sentinel-1 chips cut from float32 RTC scenes stacked per date (s1_chips.hip; the reference's instageo/data/s1_utils.py:
 * S1PointsPipeline on what stackstac.stack(..., epsg, resolution, fill_value = -1) has resampled, nearest, onto one lattice over the union
 * of the scenes' bounds; NO_DATA_VALUES.S1 = -1, no mask band).  THE RULE:
 * Sources.  T dates, 1 <= T <= 32, C >= 1 bands per date (a real product: vv, vh).  Date t has n_t >= 1 SCENES, the slices of its orbit,
 *   listed date after date; N = the sum of the n_t <= 32.  first_bits marks where the dates begin: bit s is set when scene s is the first
 *   scene of a date (so bit 0 is set, T bits are set in all and none at or above N).  Scene s has its own coordinate system
 *   scene_crs[5 s ..] (5 doubles), its own grid scene_grid[4 s ..] = (X0, Y0, sx, sy) and its own size scene_size[2 s ..] = (H_s, W_s)
 *   int32, all as ig_warp defines them, and C float32 planes, row-major in the one buffer `planes`, band b at the int64 element offset
 *   starts[s C + b] >= 0.  All tables are ON THE DEVICE.
 * Destination.  One coordinate system dst_crs (5 doubles) and one grid dst_grid (4 doubles), the STACK lattice, ON THE DEVICE; n chips of
 *   S x S pixels; origins (n, 2) int32 = (row0, col0) of chip i's top-left pixel on the stack lattice, ON THE DEVICE.  An origin may be
 *   negative or beyond every scene.
 * Coordinates.  Pixel (r, c) of chip i has the centre x = X0 + (col0 + c + 0.5) sx, y = Y0 - (row0 + r + 0.5) sy on the stack's map.  For
 *   scene s it has (u, v) by the chain of ig_warp / ig_chip_warp: where the five doubles of dst_crs and the scene's system are equal the
 *   affine arithmetic alone, u = (x - X0_s) / sx_s, v = (Y0_s - y) / sy_s (the common case: every scene in the stack's UTM zone);
 *   otherwise the inverse projection of dst_crs, evaluated ONCE per pixel and not once per scene, then the forward projection of the
 *   scene's system, (NaN, NaN) outside the domain.  NEAREST: cs = floor(u), rs = floor(v), tested on the float64 values; the pixel lies
 *   INSIDE scene s when 0 <= rs < H_s and 0 <= cs < W_s (NaN fails).  A stack grid whose values are not finite or whose pixel sizes are
 *   not positive gives chips that are no_data everywhere; a scene whose grid is such, or whose size breaks 1 <= H_s, W_s,
 *   H_s * W_s <= 2^31 - 1, reads nothing, and so does a plane with a negative start.  No read leaves a plane.
 * Value of band b of date t at a pixel.  A value v is PRESENT when it is not NaN and, with has_src_nodata != 0, v != src_nodata (float32
 *   comparison: the source's own no-data, e.g. -32768).  Walk the scenes of date t in list order: the first scene the pixel lies inside
 *   and whose value of band b is present gives the value, its 32 bits copied (-0.0, denormals and infinities included).  If no scene
 *   does, the value is no_data (float32; -1: stackstac's fill_value).  Presence is decided per value and not per scene: vv and vh of one
 *   pixel may come from different slices.  With clip != 0 a present value v then becomes clip_lo where v < clip_lo and clip_hi where
 *   v > clip_hi (the bits of the bound); a fill is not clipped.  A value that equals no_data counts as no-data wherever it came from (the
 *   reference's chip != NO_DATA_VALUES.S1).
 * Per chip: chips (n, T * C, S, S) float32, band b of date t in plane t C + b; valid_values[i] int32 += the values that differ from
 *   no_data (float32 comparison; the caller zeroes it); validity (n, S, S) uint8, or NULL, with the bits of ig_chip_cut (bit 0: all
 *   T * C values of the pixel differ from no_data, bit 1: at least one does): it feeds ig_chip_labels unchanged, which then reproduces
 *   create_segmentation_map + mask_segmentation_map(chip, seg_map, -1, strategy): `any` reads bit 0, `each` bit 1.
 * All results are copies or integers, and unique: the same bits for any launch geometry, run after run.
 * ig_s1_chip_cut: a gather in the blocking of ig_chip_warp, one launch for all n chips.  One workgroup of 256 threads owns a 64 x 64
 *   block of one chip; a wave owns 64 consecutive float32 of a row (256 bytes per store instruction), a thread takes 16 rows, 4 at a
 *   time.  Only when some scene lives in another system a thread first keeps (lon, lat) of those pixels.  Then date by date, and within a
 *   date slice by slice: the thread derives the slice's int32 source offsets rs * W_s + cs (-1 for none) and streams the C bands: a
 *   4-byte gather, the presence test, clip, count, one store.  One 32-bit mask per pixel (a bit per band; C > 32 goes in groups of 32
 *   bands) holds the values still pending: a present value is stored at once, the date's last slice stores whatever is still pending,
 *   and a later slice is neither projected nor read for a pixel with nothing pending.  The offsets are held for ONE slice at a time
 *   (16 x 32 do not fit the register file).  The validity byte comes from two per-pixel flags kept across the dates; valid_values is
 *   summed in the wave and the workgroup and added with one integer atomic per workgroup; no workgroup waits on another.
 *   1 <= T <= 32, C >= 1, 1 <= N <= 32 with first_bits as above (every n_t >= 1), 1 <= S <= 2^15, T * C * S * S <= 2^31 - 1
 *   (valid_values is int32), n * T * C * S * S < 2^40, no_data and (when given) src_nodata not NaN, clip_lo <= clip_hi; these are refused
 *   before any launch.  Per table entry H_s, W_s >= 1, H_s * W_s <= 2^31 - 1, 0 <= starts[k]: the tables are on the device, so
 *   ops.s1_chip_cut checks them on the host before the upload, and the kernel is the second fence (above).  The caller guarantees that
 *   starts[s C + b] + H_s * W_s lies inside the buffer.  planes, chips and the int32 arrays 4-byte, starts and the float64 arrays 8-byte
 *   aligned.  n = 0 returns IG_OK without touching a pointer. */
int ig_s1_chip_cut(const float* planes, const long long* starts, const double* scene_crs, const double* scene_grid, const int* scene_size,
                   int N, unsigned first_bits, const double* dst_crs, const double* dst_grid, const int* origins, int n, int T, int C, int S,
                   float no_data, int has_src_nodata, float src_nodata, int clip, float clip_lo, float clip_hi, float* chips,
                   int* valid_values, unsigned char* validity, void* stream);
/* Sentinel-1 chips warped onto label grids (s1_raster_chips.hip; not in the reference, which has no label-raster pipeline for Sentinel-1:
 * the sources and the value rule of ig_s1_chip_cut on the destination and with the label maps of ig_chip_warp).  THE RULE:
 * Sources.  Exactly those of ig_s1_chip_cut: T <= 32 dates of C >= 1 float32 bands, date t with n_t >= 1 scenes, N <= 32 in all, marked
 *   by first_bits; scene s with its own scene_crs (5 doubles), scene_grid, scene_size and its planes at starts[s C + b] in the one
 *   buffer `planes`.  All tables are ON THE DEVICE.
 * Destination.  Exactly that of ig_chip_warp: dst_crs (5 doubles) the one coordinate system of the n chips, dst_grids (n, 4) doubles the
 *   grid of every chip, ON THE DEVICE; every chip is S x S.
 * Coordinates.  The centre of pixel (r, c) of chip i comes from the arithmetic of ig_chip_warp on dst_grids[i],
 *   x = X0_i + (c + 0.5) sx_i, y = Y0_i - (r + 0.5) sy_i, and goes to every scene by the chain of ig_s1_chip_cut: where the five doubles
 *   of dst_crs equal the scene's, the affine arithmetic alone; otherwise the inverse projection of dst_crs ONCE per pixel and not once
 *   per scene, then the forward projection of the scene's system, (NaN, NaN) outside the domain.  NEAREST: floor, tested on the float64
 *   values; INSIDE as in ig_s1_chip_cut.  A destination grid whose values are not finite or whose pixel sizes are not positive gives a
 *   chip that is no_data everywhere; a scene with such a grid, or whose size breaks 1 <= H_s, W_s, H_s * W_s <= 2^31 - 1, reads nothing,
 *   and so does a plane with a negative start.  No read leaves a plane.
 * Value of band b of date t at a pixel: the rule of ig_s1_chip_cut unchanged (presence per value: not NaN and, with has_src_nodata,
 *   != src_nodata; the first scene of the date in list order that the pixel lies inside and whose value is present gives its 32 bits;
 *   otherwise no_data, float32; clip on present values only).  chips (n, T * C, S, S) float32; valid_values and validity (or NULL) with
 *   the bits of ig_chip_cut, as in ig_s1_chip_cut.
 * Label maps: labels, elem_size, valid_bit, K, maps, valid_labels and hist exactly as in ig_chip_warp (int8 or float32, NaN -> -1,
 *   -1 where the validity bit of valid_bit is clear, valid_bit 0: no masking, the histogram of int8 values in [0, K), K <= 128).  The
 *   caller zeroes valid_values, valid_labels and hist.
 * All results are copies or integers, and unique: the same bits for any launch geometry, run after run.
 * ig_s1_chip_warp: a gather in the blocking of ig_chip_warp, one launch for all n chips, with the inner loop of ig_s1_chip_cut: a thread
 *   takes its 16 rows 4 at a time, keeps (lon, lat) of those pixels when some scene lives in another system than the chips (label grids
 *   in EPSG:4326 or 3857: the common case here), holds the int32 source offsets of ONE slice at a time and the 32-bit pending mask per
 *   pixel; the validity byte, the label pixel and the tallies come from the epilogue of ig_chip_warp (the histogram in LDS; integer
 *   atomics, one set per workgroup; no workgroup waits on another).
 *   The limits are the union of the two parents': 1 <= T <= 32, C >= 1, 1 <= N <= 32 with first_bits as in ig_s1_chip_cut,
 *   1 <= S <= 2^15, T * C * S * S <= 2^31 - 1, n * T * C * S * S < 2^40, no_data and (when given) src_nodata not NaN,
 *   clip_lo <= clip_hi, elem_size 1 or 4 (also without labels), 0 <= K <= 128 and K > 0 needs elem_size 1 and labels, valid_bit 0, 1 or
 *   2; these are refused before any launch.  Per table entry H_s, W_s >= 1, H_s * W_s <= 2^31 - 1, 0 <= starts[k]: the tables are on the
 *   device, so ops.s1_chip_warp checks them on the host before the upload, and the kernel is the second fence (above).  The caller
 *   guarantees that starts[s C + b] + H_s * W_s lies inside the buffer.  planes, chips, the int32 arrays and float32 labels / maps
 *   4-byte, starts and the float64 arrays 8-byte aligned.  n = 0 returns IG_OK without touching a pointer. */
int ig_s1_chip_warp(const float* planes, const long long* starts, const double* scene_crs, const double* scene_grid, const int* scene_size,
                    int N, unsigned first_bits, const double* dst_crs, const double* dst_grids, int n, int T, int C, int S, float no_data,
                    int has_src_nodata, float src_nodata, int clip, float clip_lo, float clip_hi, const void* labels, int elem_size,
                    int valid_bit, int K, float* chips, int* valid_values, unsigned char* validity, void* maps, int* valid_labels, int* hist,
                    void* stream);
/* Cloud-free temporal composites of HLS scenes (composite.hip; not in the reference, whose add_hls_stac_items takes the single least
 * cloudy granule near a step's date and loses what Fmask flags in it).  THE RULE:
 * Inputs.  N scenes of one MGRS tile on ONE grid of H x W pixels (the host checks size, tiepoint, pixel scale and GeoKeys).  Scene n has C
 *   int16 band planes and one uint8 Fmask plane, each row-major and whole, packed in the one int16 buffer `bands` and the one uint8 buffer
 *   `fmasks`: band c of scene n at the int64 element offset starts[n C + c], its Fmask at fmask_starts[n]; both tables ON THE DEVICE, as
 *   ig_warp and ig_s2_chip_cut pack theirs.  fmasks NULL (then fmask_starts NULL): no scene has an Fmask.  The scenes are grouped into T
 *   temporal steps: step_ptr, T + 1 ascending int32 values from 0 to N ON THE DEVICE, lists the CANDIDATES of step t as the scenes
 *   step_ptr[t] .. step_ptr[t + 1] - 1, in the order the host gives them; a step has 0 <= m <= 16 candidates, T <= 32.  max_m is the
 *   largest m, which the caller states (the table is on the device): it sizes the kernel's registers and sorting network.
 * Clear observations.  Candidate n is CLEAR at a pixel when fmask_n & mask_bits == 0 and every one of its C values differs from no_data.
 *   mask_bits has the bit positions of ig_chip_cut (cloud 1, near_cloud_or_shadow 2, cloud_shadow 3, water 5); an Fmask of 255 (fill) is
 *   masked by any non-zero mask_bits.
 * Count.  count is the number of clear candidates at the pixel.  A pixel with count < min_clear (min_clear >= 1) gets no_data in all C
 *   bands and source = 255.  Otherwise, by method:
 *   0 NEAREST: the first clear candidate in list order gives all C values; its position in the step's list goes to source.  The host
 *     orders candidates by |acquisition date - the step's target date|, the earlier date on a tie, so this is the nearest clear date: the
 *     rule ig_s1_chip_cut has for orbit slices.
 *   1 MEDIAN: per band the LOWER MEDIAN of the clear values, the floor((count - 1) / 2)-th smallest, 0-based: an observed value, nothing
 *     is rounded.  source = 255.
 *   2 MEDOID: with med_c the MEDIAN of band c, the clear candidate with the smallest sum over c of |v_{n,c} - med_c| gives all C values,
 *     so the output is a spectrum that was observed; the EARLIEST IN LIST ORDER wins a tie.  The differences are formed in 32 bits and the
 *     sum is exact in int32 (C <= 32767).  The candidate's position goes to source.
 * Outputs.  composite (T, C, H, W) int16, count (T, H, W) uint8, source (T, H, W) uint8; hist (T, 17) int32 += the number of pixels of
 *   step t per count value 0 .. 16 (the caller zeroes it).  Every output pixel is WRITTEN EXACTLY ONCE.  A step with m = 0 writes no_data,
 *   count 0 and source 255 everywhere.  All results are integers or copies, and unique: the same bits for any launch geometry, run after
 *   run.
 * ig_composite: a streaming read bound by HBM, m (2 C + 1) bytes in and 2 C + 2 bytes out per pixel, all T steps in one launch.  Every
 *   plane is a whole grid, so pixels are taken in plane order (the row pitch never enters); one workgroup of 256 threads owns 512
 *   consecutive pixels of one step, a thread two of them, kept as the two 16-bit halves of one register.  The access width is chosen per
 *   plane from its address (4 bytes, or 2 + 2 for a plane that starts at an odd element); the workgroup at the end of a plane goes element
 *   by element.  For C in {1, 2, 3, 4, 6} every value is read ONCE and stays in registers: first the clear masks, then band by band the
 *   keys (a candidate that is not clear becomes 32767, which sorts behind every clear value and equals what it may tie with) go through
 *   Batcher's odd-even merge network on packed 16-bit minima and maxima (63 comparators at 16 keys, both pixels per instruction); MEDOID
 *   accumulates the distances while the band is in registers and copies the winner out of them.  For any other C the register file cannot
 *   hold the stack: the no_data test takes a pass of its own, the bands are read again and the winner's values a third time.  hist is
 *   tallied in LDS and added with at most 17 integer atomics per workgroup; no workgroup waits on another.
 *   Refused before any launch: T > 32, max_m > 16 (a step with more candidates), N > T * max_m, C outside [1, 32767], no_data outside
 *   int16, mask_bits outside a byte, min_clear outside [1, 16], a method outside 0..2, H * W > 2^31 - 1, T * C * H * W >= 2^40, null
 *   pointers, bands / composite not 2-byte, step_ptr / hist not 4-byte, starts / fmask_starts not 8-byte aligned.  H * W = 0 or T = 0
 *   returns IG_OK without touching a pointer.  The tables are on the device, so ops.composite checks them on the host before the upload
 *   (every plane inside its buffer, step_ptr ascending, m <= max_m); the kernel is the second fence: a step whose bounds break
 *   0 <= step_ptr[t] <= step_ptr[t + 1] <= N has no candidates and one longer than max_m is cut.  The caller guarantees that
 *   starts[k] + H * W and fmask_starts[n] + H * W lie inside the buffers. */
int ig_composite(const short* bands, const long long* starts, const unsigned char* fmasks, const long long* fmask_starts,
                 const int* step_ptr, int T, int N, int max_m, int C, int H, int W, int mask_bits, int no_data, int min_clear, int method,
                 short* composite, unsigned char* count, unsigned char* source, int* hist, void* stream);
/* Speckle filtering and dB scaling of Sentinel-1 RTC planes (s1_filter.hip; not in the reference, whose S1PointsPipeline copies linear
 * gamma0 into the chips as it comes).  THE RULE:
 * Inputs.  N float32 planes, each row-major and whole, packed in the one float32 buffer `planes` of `total` elements: plane p has the size
 *   sizes[2 p ..] = (H, W) int32 and starts at the int64 element offset starts[p]; both tables ON THE DEVICE, the packing of
 *   ig_s1_chip_cut and ig_composite.  h in 1..7 gives the window w = 2 h + 1 of 3..15; method is 0 BOXCAR, 1 LEE or 2 GAMMA_MAP; looks is
 *   a float32 > 0, the equivalent number of looks (a user setting, 4.4 for IW GRD); has_src_nodata / src_nodata as in ig_s1_chip_cut;
 *   to_db is 0 or 1.
 * Presence.  A value is PRESENT when it is finite (NaN and +-inf are absent) and, with has_src_nodata != 0, differs from src_nodata.
 * Window moments.  For pixel (r, c) the window is rows r - h .. r + h and columns c - h .. c + h, clipped to the plane.  All arithmetic is
 *   in FLOAT64 WITH CONTRACTION OFF, in this order: per window row, left to right over the present values, starting from +0.0:
 *   A_i += x, Q_i += x x, K_i += 1 (x the float32 widened, so x x is exact); then top to bottom, starting from +0.0: A += A_i, Q += Q_i,
 *   n += K_i.  The order is part of the rule.
 * Centre absent: the output is the quiet NaN 0x7FC00000; absent stays absent, nothing is filled in.
 * Centre present (then n >= 1): m = A / n, v = Q / n - m m with each operation rounded once, v = 0 where v < 0; s = 1 / (double)looks.
 *   0 BOXCAR: y = m.
 *   1 LEE (Lee 1980, MMSE form): t = (m m) s, vx = (v - t) / (1 + s), b = vx / v when v > 0 and vx > 0, else 0, y = m + b (x - m).
 *   2 GAMMA_MAP (Lopes 1990): if m <= 0, y = m.  Otherwise ci2 = v / (m m); if ci2 <= s, y = m; if ci2 >= 2 s, y = x; otherwise
 *     a = (1 + s) / (ci2 - s), B = a - (double)looks - 1, D = (m m)(B B) + ((4 a)(double)looks)(m x), y = (B m + sqrt(D)) / (2 a) when
 *     D >= 0, else m.
 * Scale.  to_db = 0: out = (float)y, rounded to nearest.  to_db = 1: out = (float)(10 log10(y)) when y > 0, else the quiet NaN and the
 *   pixel is counted as DROPPED.
 * Outputs.  out float32 with the layout and starts of planes (`total` elements; it must not overlap planes); every element of every
 *   plane is WRITTEN EXACTLY ONCE, elements between planes are left alone.  counts (N, 2) int32 (the caller zeroes it): counts[p][0] +=
 *   the outputs of plane p that are present (centre present and not dropped), counts[p][1] += the pixels dropped by the dB step.
 *   Add, multiply, divide, compare and convert are correctly rounded, so BOXCAR and LEE in linear scale are the same bits on any
 *   IEEE-754 machine; sqrt and log10 are the library's.  Each result depends on its window alone: the same bits for any launch geometry.
 * ig_s1_speckle: one launch for all planes.  One workgroup of 256 threads owns a tile of 64 columns x 32 rows of one plane; tile_ptr
 *   (N + 1 ascending int64 from 0, ON THE DEVICE, built by the host: plane p has ceil(H / 32) ceil(W / 64) tiles) lets workgroup b find
 *   its plane by binary search, `tiles` = tile_ptr[N] is the grid.  The tile and its halo of h pixels are staged in LDS once as float32,
 *   absent values (and what lies outside the plane) as NaN; then the row moments of the 32 + 2 h staged rows go to LDS as float64,
 *   float64, int32 and are summed down the columns.  Each value comes from HBM once plus the halo; a wave stores 64 consecutive float32
 *   of a row, 4 bytes per lane, which any W and any 4-byte-aligned start allow; borders and ragged last tiles are bounds tests, no
 *   padding is read; LDS 73 232 bytes at h = 7: two workgroups per CU.  The counts are summed in the wave and the workgroup and added
 *   with one integer atomic each per workgroup; no workgroup waits on another.
 *   Refused before any launch: h outside 1..7, method outside 0..2, looks not > 0 or not finite, has_src_nodata or to_db outside 0..1,
 *   src_nodata NaN, N < 0, total < 0 or >= 2^40, tiles < 0 or > 2^31 - 1, null pointers, planes / out / sizes / counts not 4-byte,
 *   starts / tile_ptr not 8-byte aligned, out overlapping planes.  N = 0 returns IG_OK without touching a pointer.  Per table entry
 *   1 <= H W <= 2^31 - 1, starts >= 0 and starts + H W <= total: the tables are on the device, so ops.s1_speckle checks them on the host
 *   before the upload, and the kernel is the second fence: a plane whose stated size is not positive (or that breaks the other bounds) is
 *   skipped, as is a workgroup beyond its plane's own number of tiles. */
int ig_s1_speckle(const float* planes, const long long* starts, const int* sizes, const long long* tile_ptr, int N, long total, long tiles,
                  int h, int method, float looks, int has_src_nodata, float src_nodata, int to_db, float* out, int* counts, void* stream);
/* Refined Lee speckle filtering of Sentinel-1 RTC planes (s1_filter.hip; Lee 1981, the edge-aligned window that is the default speckle
 * filter of ESA's SNAP toolbox; not in the reference).  The square window of ig_s1_speckle straddles both sides of an edge; this filter
 * estimates from the half of a 7 x 7 window that lies on the pixel's own side of the local edge.  THE RULE:
 * Exactly ig_s1_speckle's: presence, the packed planes and starts / sizes / tile_ptr, an absent centre stays absent (the quiet NaN
 *   0x7FC00000), the dB step and the two counts per plane.  The window is 7 x 7 (h = 3), clipped to the plane.  All arithmetic is FLOAT64
 *   WITH CONTRACTION OFF, every operation rounded on its own; an absent or outside value adds +0.0 and counts 0; s = 1 / (double)looks.
 *   For a present centre x at (r, c):
 * 1 Full window.  A, Q and n as in ig_s1_speckle at h = 3 (row moments left to right, rows top to bottom).  m = A / n,
 *   v = max(Q / n - m m, 0), t = (m m) s, vx = (v - t) / (1 + s).  If not (v > 0 and vx > 0) the window is HOMOGENEOUS: y = m, which is
 *   what LEE at h = 3 returns there, and steps 2 to 4 are skipped.
 * 2 Sub-window means.  For i, j in {0, 1, 2} the 3 x 3 window centred at (r + 2 (i - 1), c + 2 (j - 1)), clipped to the plane: A3 is
 *   summed per row left to right from +0.0, then the rows top to bottom from +0.0, n3 is its number of present values, M[i][j] = A3 / n3
 *   (Mij below).  If any of the nine has n3 = 0, y is the LEE value of the full window from step 1's sums, y = m + (vx / v)(x - m), and
 *   steps 3 and 4 are skipped (the FALLBACK: the outermost ring of a plane and pixels next to large holes).
 * 3 Direction.  With c0 = M11, the four gradients, each evaluated as written, left to right:
 *     g_d1 = |(M12 + M21 + M22) - (M00 + M01 + M10)|   halves SE / NW
 *     g_d2 = |(M01 + M02 + M12) - (M10 + M20 + M21)|   halves NE / SW
 *     g_h  = |(M02 + M12 + M22) - (M00 + M10 + M20)|   halves E / W
 *     g_v  = |(M20 + M21 + M22) - (M00 + M01 + M02)|   halves S / N
 *   The largest gradient wins; on a tie the first in the order d1, d2, h, v.  Inside the winning pair the first-named half wins if its
 *   sub-window is at least as close to the centre mean as the other's: SE if |M22 - c0| <= |M00 - c0|, else NW; NE if
 *   |M02 - c0| <= |M20 - c0|, else SW; E if |M12 - c0| <= |M10 - c0|, else W; S if |M21 - c0| <= |M01 - c0|, else N.
 * 4 Half window.  With offsets (dy, dx) in [-3, 3]^2, dy down and dx right, the masks are E: dx >= 0, W: dx <= 0, S: dy >= 0,
 *   N: dy <= 0, SE: dx + dy >= 0, NW: dx + dy <= 0, NE: dx - dy >= 0, SW: dx - dy <= 0; each holds 28 pixels and always the centre.  The
 *   sums A', Q', n' run over the mask's present pixels inside the plane: per mask row left to right from +0.0, then the row sums top to
 *   bottom from +0.0 over all seven rows (a pixel outside the mask adds +0.0, so a predicated 7 x 7 loop and a 28-term loop give the
 *   same bits).  Then LEE on (A', Q', n', x): m' = A' / n', v' = max(Q' / n' - m' m', 0), t' = (m' m') s, vx' = (v' - t') / (1 + s),
 *   b' = vx' / v' when v' > 0 and vx' > 0, else 0, y = m' + b' (x - m').
 * 5 Scale and outputs as in ig_s1_speckle: to_db = 0 stores (float)y, to_db = 1 stores (float)(10 log10(y)) when y > 0, else the quiet
 *   NaN and a DROPPED count; every element of every plane is written exactly once, counts (N, 2) int32 is zeroed by the caller.
 *   Only correctly rounded operations occur before the dB step, so the linear scale is the same bits on any IEEE-754 machine and for any
 *   launch geometry; dB goes through each side's log10.
 * ig_s1_refined_lee: one launch for all planes with the tile of ig_s1_speckle (64 columns x 32 rows, 256 threads, the plane found by
 *   binary search in tile_ptr, so one tile table serves both).  The tile and its halo of 3 pixels are staged in LDS as float32, absent
 *   values and what lies outside the plane as NaN; the row moments of the full window go to LDS and are summed down the columns as in
 *   ig_s1_speckle; the sub-window means of the (32 + 4) x (64 + 4) centres a tile can ask for go to LDS once as float64 (NaN where
 *   n3 = 0), so a pixel reads nine of them; the half window is one uniform 7 x 7 loop over the staged tile under the chosen direction's
 *   49-bit mask, taken only by the lanes that reach step 4.  Less than 80 KB of LDS: two workgroups per CU.  Stores and counts as in
 *   ig_s1_speckle.
 *   Refused before any launch: looks not > 0 or not finite, has_src_nodata or to_db outside 0..1, src_nodata NaN, N < 0, total < 0 or
 *   >= 2^40, tiles < 0 or > 2^31 - 1, null pointers, planes / out / sizes / counts not 4-byte, starts / tile_ptr not 8-byte aligned, out
 *   overlapping planes.  N = 0 returns IG_OK without touching a pointer.  The tables are on the device, so ops.s1_refined_lee checks them
 *   on the host before the upload, and the kernel is the second fence, exactly as in ig_s1_speckle. */
int ig_s1_refined_lee(const float* planes, const long long* starts, const int* sizes, const long long* tile_ptr, int N, long total,
                      long tiles, float looks, int has_src_nodata, float src_nodata, int to_db, float* out, int* counts, void* stream);
/* Multi-temporal speckle filtering of Sentinel-1 RTC planes (s1_temporal.hip; Quegan and Yu 2001 with the boxcar local mean; not in the
 * reference).  Every date of a stack is filtered by borrowing the other dates at the same pixel, at the input's resolution.  THE RULE:
 * Inputs.  N float32 planes packed in `planes` with starts / sizes exactly as for ig_s1_speckle.  Every plane belongs to one GROUP (the
 *   planes of one band on one pixel lattice of H_g x W_g pixels, lattice[2 g ..] = (H_g, W_g) int32) and one DATE (an index >= 0) and sits
 *   at an integer offset on its group's lattice: place[3 p ..] = (row0, col0, date) int32 with row0, col0 >= 0, row0 + H <= H_g and
 *   col0 + W <= W_g.  The members of group g are members[member_ptr[g] .. member_ptr[g + 1]) (plane indices; member_ptr: G + 1 ascending
 *   int32 from 0 to M), ORDERED BY DATE, THEN BY THE ORDER GIVEN: the order in which orbit slices are tried, the slice order of
 *   ig_s1_chip_cut.  All tables ON THE DEVICE.  h, has_src_nodata / src_nodata and to_db as in ig_s1_speckle.
 * Presence and local mean.  A value is PRESENT by ig_s1_speckle's definition (finite and, with has_src_nodata != 0, not src_nodata).  The
 *   local mean of plane p at one of its pixels whose value is present is m_p = A / (double)n, with A and n exactly ig_s1_speckle's first
 *   moment and count: the window of w = 2 h + 1 around the pixel CLIPPED TO THE PLANE p (not to the lattice), present values only, FLOAT64
 *   WITH CONTRACTION OFF, per window row left to right from +0.0, then the rows top to bottom from +0.0.  No second moment.
 * Ratio sum at lattice pixel x.  Walk the group's members in order.  The value of a date is that of the FIRST member of the date that
 *   covers x and is present there; later members of that date are not looked at for x.  The date CONTRIBUTES when that member's m > 0: it
 *   adds r = x_p / m_p to R (float64, from +0.0, in date order) and 1 to c (int).  A date with no present member at x, or whose first
 *   present member has m <= 0, contributes nothing.
 * Output of plane k at x, for every element of every plane, WRITTEN EXACTLY ONCE (elements between planes are left alone).
 *   Centre absent: the quiet NaN 0x7FC00000.  Centre present with m_k > 0 and c >= 1: y = m_k * (R / (double)c), each operation rounded
 *   once.  Any other present centre: y = x_k, counted as PASSED THROUGH.  to_db = 0 stores (float)y; to_db = 1 stores
 *   (float)(10 log10(y)) when y > 0, else the quiet NaN and the pixel is counted as DROPPED (a passed-through pixel can be dropped too, and
 *   is then counted as both).  Overflow of the float conversion to +-inf is IEEE's and not special-cased.
 * Counts.  counts (N, 4) int32 (the caller zeroes it), per plane: [0] += the present outputs (centre present and not dropped), [1] +=
 *   the pixels dropped by the dB step, [2] += the pixels passed through, [3] += the present outputs at pixels with c == 1 (no temporal
 *   gain there: with m_k > 0 the output is m_k (x_p / m_p), which for the date's own value is x_k up to rounding).
 * Bits.  Each output depends on its pixel's windows and the member order alone: the same bits for any launch geometry, run after run.
 *   Add, multiply, divide, compare and convert are correctly rounded, so the linear scale is the same bits on any IEEE-754 machine; dB goes
 *   through each side's log10.
 * ig_s1_temporal: one launch for all groups.  One workgroup of 256 threads owns a tile of 64 columns x 32 rows of one group's LATTICE;
 *   tile_ptr (G + 1 ascending int64 from 0, built by the host: group g has ceil(H_g / 32) ceil(W_g / 64) tiles) lets workgroup b find its
 *   group by binary search, `tiles` = tile_ptr[G] is the grid.  Two sweeps over the group's members inside the workgroup; a member whose
 *   extent misses the tile is passed over.  Sweep 1 stages the member's part of the tile and a halo of h pixels in LDS as float32 (absent
 *   values and what lies outside the plane as NaN, bounds tests at the load, no padding read), forms the row moments (A float64, K int32) and
 *   the column sums as ig_s1_speckle does, and keeps R, c and the last date taken of a thread's 8 pixels in registers.  Sweep 2 stages
 *   every member again (a cache hit), forms m_k and stores y: a wave writes 64 consecutive float32 of a row, 4 bytes per lane, which any
 *   W and any 4-byte-aligned start allow.  LDS 49 680 bytes at h = 7: three workgroups per CU.  The counts are summed in the wave and the
 *   workgroup and added with integer atomics per workgroup and touched plane; no workgroup waits on another.
 *   Refused before any launch: h outside 1..7, has_src_nodata or to_db outside 0..1, src_nodata NaN, N < 0, G outside [1, N], M outside
 *   [0, N], total < 0 or >= 2^40, tiles < 0 or > 2^31 - 1, null pointers, planes / out / sizes / place / lattice / member_ptr / members /
 *   counts not 4-byte, starts / tile_ptr not 8-byte aligned, out overlapping planes.  N = 0 returns IG_OK without touching a pointer.  The
 *   tables are on the device, so ops.s1_temporal checks them on the host before the upload (planes inside the buffer and not overlapping,
 *   every plane inside its group's lattice, H_g W_g <= 2^31 - 1, the member lists consistent with the planes' groups and dates, at most 64
 *   planes per group and 32 dates: the kernel's loop is a runtime loop, these bounds only size tables), and the kernel is the second fence:
 *   a group whose lattice is not positive or whose member range breaks 0 <= begin <= end <= M is skipped, as is a workgroup beyond its
 *   group's own number of tiles, a member entry outside [0, N) and a plane that breaks the bounds of ig_s1_speckle, has a negative offset
 *   or date, or leaves its lattice. */
int ig_s1_temporal(const float* planes, const long long* starts, const int* sizes, const int* place, const int* lattice,
                   const int* member_ptr, const int* members, const long long* tile_ptr, int N, int G, int M, long total, long tiles, int h,
                   int has_src_nodata, float src_nodata, int to_db, float* out, int* counts, void* stream);
/* Web Mercator map tiles rendered from an overview pyramid (maptiles.hip; the reference's new_apps/backend/app/tiler_service.py answers
 * tiles/WebMercatorQuad/{z}/{x}/{y}@1x.png through TiTiler: a warp into EPSG:3857, an overview level, nearest sampling and a colormap or
 * rescale per request).  THE RULE:
 * Source.  One raster in one coordinate system src_crs (5 doubles) on one grid src_grid = (X0, Y0, sx, sy) (4 doubles), both ON THE DEVICE
 *   and exactly as ig_warp defines them, given as a pyramid of nlevels levels in the level geometry of ig_overview_mode / ig_overview_mean:
 *   level 0 is H x W, level k has H_k = ceil(H_{k-1} / 2) rows and W_k = ceil(W_{k-1} / 2) columns (= ceil(H / 2^k), ceil(W / 2^k)) and
 *   the grid (X0, Y0, sx 2^k, sy 2^k).  Elements are int8 with 1 band (elem_size 1) or float32 with 1 or 3 bands (elem_size 4); level k is
 *   laid out (bands, H_k, W_k).  levels is a table ON THE DEVICE of nlevels pointers, one per level: every level stays where it is (level 0
 *   is never copied; levels 1.. may be the views of the one buffer ig_overview_* filled, or separate allocations).
 * Tiles.  One launch renders n tiles of tile x tile pixels, tile a multiple of 64 from 64 to 1024.  Tile i has the destination grid
 *   tile_grids[4 i ..] (4 doubles) in EPSG:3857, the coordinate system (2, 0, 0, 0, 0) of ig_warp, and reads pyramid level tile_level[i]
 *   (int32); the host chooses both.  A level outside [0, nlevels), a tile grid or a source grid whose values are not finite or whose pixel
 *   sizes are not positive gives a fully transparent tile and reads nothing.
 * Sampling.  The source coordinates (u, v) of a pixel centre come from the chain of ig_warp_coords, unchanged (the affine arithmetic alone
 *   where src_crs equals (2, 0, 0, 0, 0) as doubles, otherwise inverse web Mercator and the forward projection of src_crs, (NaN, NaN)
 *   outside the domain).  Both are then divided by 2^level, which is exact.  NEAREST: c = floor(u), r = floor(v), tested on the float64
 *   values; a pixel with r outside [0, H_k), c outside [0, W_k) or NaN coordinates is TRANSPARENT.
 * Output.  rgba (n, tile, tile, 4) uint8, the bytes R, G, B, A in memory order; a transparent pixel is four zero bytes.  opaque[i] (int32,
 *   the caller zeroes it) += the pixels of tile i with A != 0.
 * Styles.  lut is (256, 4) uint8 ON THE DEVICE (R, G, B, A per entry; style 2 does not read it and takes NULL).
 *   0 PALETTE (int8): a value v with 0 <= v < ncolors (ncolors <= 256) and v != fill gives the four bytes of lut[v]; any other is transparent.
 *   1 RAMP (float32, 1 band): NaN is transparent; otherwise t = ((double)v - lo) / span, clamped to [0, 1] (below 0 -> 0, above 1 -> 1:
 *     infinities clamp), idx = (int)rint(t * 255) with ties to even, and the pixel is lut[idx].  span = hi - lo is formed by the caller;
 *     lo and span are finite, span > 0.
 *   2 RGB (float32, 3 bands): output channel j comes from plane order[j] (each in 0..2); if any of the three values is NaN the pixel is
 *     transparent, otherwise each channel is idx as above and A = 255.
 *   The index is one float64 subtraction, one division, one multiplication and one rint, each rounded on its own (nothing is contracted):
 *   numpy float64 arithmetic with np.rint gives the same integer.
 * ig_tile_render: a gather.  One workgroup of 256 threads owns one 64 x 64 block of one tile (the blocking of ig_chip_warp), blocks
 *   numbered tile-major, then row-major; a wave owns 64 consecutive pixels of a row and stores them as one 32-bit value per lane, 256
 *   contiguous bytes per instruction; a thread takes 16 rows in turn and evaluates the float64 chain ONCE per pixel.  Every pixel of rgba
 *   is written exactly once by the thread that computed it.  opaque is summed in the wave and the workgroup (the only LDS) and added with
 *   one integer atomic per workgroup; no workgroup waits on another; all results are integers or table entries: the same bits for any
 *   launch geometry, run after run.  1 <= nlevels <= 13, H * W <= 2^31 - 1 (so every level's offsets fit int32), n * tile * tile < 2^31,
 *   fill fits int8.  The level table and the float64 arrays 8-byte, tile_level, lut, rgba and opaque 4-byte aligned; a level's pointer is
 *   aligned to its elements (int8 levels may start at any byte).  The caller guarantees that levels[k] holds bands * H_k * W_k elements.
 *   n = 0 returns IG_OK without touching a pointer. */
int ig_tile_render(const void* const* levels, int nlevels, int elem_size, int bands, int H, int W, const double* src_crs,
                   const double* src_grid, const double* tile_grids, const int* tile_level, int n, int tile, int style,
                   const unsigned char* lut, int ncolors, int fill, double lo, double span, int order0, int order1, int order2,
                   unsigned char* rgba, int* opaque, void* stream);
/* Dataset cleaning (clean.hip; the reference's instageo/data/data_cleaner.py: should_drop_chip, buffer_observation_pixels,
 * limit_seg_map_to_observation_pixels).  All results are integers or bit copies, and unique: the same bits for any launch geometry, run
 * after run.  THE RULE:
 * No-data planes and counts.  chips (n, B, H, W), 16-bit (int16 or uint16: the comparison is on the 16-bit pattern of no_data, which the
 *   caller has checked to be representable in the chips' type).  Pixel p of chip i is ANY-no-data when at least one of its B values equals
 *   no_data, ALL-no-data when all B do.  plane (n, H, W) uint8: bit 0 = any, bit 1 = all.  counts (n, 2) int32 += the chip's any pixels
 *   (counts[2 i]) and all pixels (counts[2 i + 1]); the caller zeroes it.  A chip is DROPPED when count[strategy] / float(H * W) >
 *   no_data_threshold, evaluated on the host in float64 (np.mean(mask) > threshold).
 * Buffer.  labels (n, H, W), int16 (elem_size 2) or float32 (4).  A pixel is a SOURCE when its value != ignore_index, compared in the
 *   map's type: for float32 a NaN is a source, as in numpy.  Output pixel (r, c) takes the value of the source with the LARGEST ROW-MAJOR
 *   INDEX r' * W + c' among the sources of the INPUT map with |r - r'| <= w and |c - c'| <= w inside the map; with no such source it keeps
 *   its input value (which is then ignore_index).  Afterwards a pixel whose plane byte has bit 1 set (all-no-data; plane NULL: no masking)
 *   becomes ignore_index.  This is the reference's numpy repeated-index assignment made explicit: sources go in np.where order, the later
 *   assignment wins, and clipping the window to the border only repeats a pixel with the same value.  A source is itself overwritten by a
 *   later source in its window, and running the buffer twice buffers twice.  Values are copied bit for bit.
 * Limit.  The points of map i are pts[ptr[i] .. ptr[i + 1]) (ptr: n + 1 int32, ascending from 0 to P; pts (P, 2) int32 = (row, col) on
 *   the map).  An output pixel keeps its input value where at least one point lies on it and becomes ignore_index elsewhere.  Duplicates
 *   are harmless; a point outside the map paints nothing.
 * Both label entry points: out (n, H, W) of the labels' type, distinct from labels; valid_labels[i] int32 += the output pixels !=
 *   ignore_index; hist (n, K) int32 += for int16 maps the output pixels per value in [0, K), K <= 256 (values outside are not counted);
 *   K = 0: no histogram, hist may be NULL.  The caller zeroes valid_labels and hist.  ignore_index must be representable in the map's
 *   type (int16 range; for float32 |ignore_index| <= 2^24).
 * ig_chip_nodata: a streaming read.  A thread owns 8 consecutive pixels of one chip's plane and walks the B bands: load, compare, OR into
 *   any, AND into all; it writes its 8 plane bytes once.  The access width of every 8-pixel segment is chosen from its address (16, 8, 4
 *   or 2 bytes: with H * W odd every second band starts 2-byte aligned); the tail of a plane goes element by element.  The counts are
 *   summed in the wave and the workgroup and added with one integer atomic pair per workgroup; no workgroup waits on another.  B >= 1,
 *   H * W <= 2^31 - 1, n * B * H * W < 2^40, -32768 <= no_data <= 65535.  n = 0 returns IG_OK without touching a pointer.
 * ig_label_buffer: a gather.  One workgroup owns a 64 x 64 block of one map.  It stages the source flags of the block plus a halo of w
 *   into LDS (outside the map: no source), a row pass gives every staged row and block column the right-most source column within +-w
 *   (or -1), and the column pass takes the bottom-most staged row within +-w that has a hit: the largest row-major index.  A thread
 *   resolves 16 pixels: the winner's value from global memory, the plane's bit 1, one store, valid_labels and the histogram tallied in LDS
 *   and added with integer atomics.  0 <= w <= 32 (w = 0 is only the masking), H, W <= 2^30, n * H * W < 2^40.
 * ig_label_limit: the same block ownership with a 4096-bit mask in LDS: a thread takes every 256th point of the map's list and sets the
 *   bit of a point inside the block with an LDS atomic OR; after the barrier the pixels are resolved and tallied as above.  The caller
 *   guarantees ptr (ops.label_limit checks it on the host); list bounds are clamped to [0, P] all the same, so no read leaves pts. */
int ig_chip_nodata(const void* chips, int n, int B, int H, int W, int no_data, unsigned char* plane, int* counts, void* stream);
int ig_label_buffer(const void* labels, int n, int H, int W, int elem_size, int w, int ignore_index, const unsigned char* plane, int K,
                    void* out, int* valid_labels, int* hist, void* stream);
int ig_label_limit(const void* labels, int n, int H, int W, int elem_size, const int* ptr, const int* pts, long P, int ignore_index, int K,
                   void* out, int* valid_labels, int* hist, void* stream);
/* Spatially blocked train / val / test splitting of a chip dataset (split.hip; the step of the reference's instageo/data/data_splitter.py,
 * under a rule of this project's own: DESIGN.md 3.34).  Everything the kernels compute is integer, so every result is unique: the same
 * bits for any launch geometry and any order of arrival, run after run.  THE RULE:
 * Location.  The location of a dataset row is the centre of the grid of its Input GeoTIFF, taken from the file's profile (the pixels are
 *   never read) and brought to longitude / latitude in float64 (crs.inverse).  A row whose file has no georeferencing is dropped
 *   (reason no_location).
 * Position.  p = (cos(lat) cos(lon), cos(lat) sin(lon), sin(lat)) in float64; every component is multiplied by 2^29 and rounded half to
 *   even to int32: |p_i| <= 2^29, one unit is about 1.2 cm on the ground.  This is done on the host; the kernels only see int32 (N, 3).
 * Distance.  d2(p, q) = sum_i (p_i - q_i)^2 as an unsigned 64-bit integer: |p_i - q_i| <= 2^30, so d2 <= 3 * 2^60.  Kilometres, for the
 *   buffer test and the report only, are 2 * 6371.0088 * asin(sqrt(d2) / 2^30), clipped at the antipode, in float64 on the host.  The
 *   antimeridian and the poles are no special case.
 * Spherical k-means.  Initial centres (host): the first is the point at index numpy.random.default_rng(random_state).integers(N); each
 *   further one is the point with the largest d2 to its nearest chosen centre, ties to the smallest index; with fewer than n_clusters
 *   distinct positions K becomes their number.  One Lloyd round is one launch of ig_split_assign: every point takes the centre with the
 *   smallest d2, ties to the smallest centre index; per centre the int64 sums of x, y, z and the count; the number of points whose
 *   assignment changed (assignments start at -1).  The host then divides the sums by the count in float64, normalises to unit length and
 *   quantises as above; an empty centre, or one whose mean vector is zero, keeps its position.  Rounds stop when nothing changed or after
 *   max_iter.
 * Clusters to sets (host, K items).  Targets are floor(N * test_ratio) and floor(N * val_ratio) rows.  Test: the seed is the cluster
 *   with the highest mean year when every row has a year (the first of 19xx | 20xx in the file name), ties to the smallest index, else
 *   cluster 0; then the untaken cluster whose centre is nearest (d2) to any taken test centre is added, ties to the smallest index,
 *   until the target is reached.  Val: the same among the remaining clusters, seeded by the remaining cluster at position
 *   rng.integers(number remaining) of the same generator.  Train is the rest.  A set that would take every cluster raises.
 * Audit and guard band.  The nearest-row search (ig_split_nearest) runs train -> (val u test) and val -> test: per row the smallest d2 to
 *   a row of the other side and the SMALLEST INDEX that attains it.  With buffer_km > 0 the train rows nearer than that to any val or
 *   test row are removed, then the val rows nearer than that to any test row (reason buffer).
 * ig_split_assign: pts (N, 3) int32, centres (K, 3) int32, |coordinate| <= 2^29 (the caller guarantees it; differences are taken modulo
 *   2^32, so any input is memory-safe).  assign (N) int32 is read (the previous assignment) and written; sums (K, 4) int64 += (sum x,
 *   sum y, sum z, count) and changed (1) int32 += the points whose assignment differs from the one read; the caller zeroes both.  The
 *   centres live in LDS; a thread owns 8 points, keeps the sums of a run of points with one centre in registers, adds them to per-centre
 *   64-bit cells in LDS with integer atomics, and the workgroup adds its non-zero cells to sums with 64-bit integer atomics.
 *   0 <= N < 2^30, 1 <= K <= 256; N = 0 returns IG_OK without touching a pointer.
 * ig_split_nearest: a (Na, 3), b (Nb, 3) int32 as above -> d2 (Na) uint64 and idx (Na) int32, every element written exactly once.  A
 *   thread owns 4 rows of a (1 when Na < 1024) in registers; b is staged through LDS in tiles of 1024 points and read as a broadcast; a
 *   pair costs three subtractions and three 32 x 32 + 64 multiply-adds.  b is walked in ascending index with a strict comparison, so
 *   the first minimum is the smallest index.  When the blocks of a alone do not fill the device b is cut into contiguous ranges, one
 *   workgroup each, whose results go to a scratch buffer and are merged by a second kernel in ascending range order (smaller d2, then
 *   smaller index: associative, so the result does not depend on the cut).  No floating point, no workgroup waits on another.
 *   0 <= Na < 2^30, 1 <= Nb < 2^30; Na = 0 returns IG_OK without touching a pointer.  pts, centres, assign, changed, a, b and idx 4-byte,
 *   sums and d2 8-byte aligned. */
int ig_split_assign(const int* pts, int N, const int* centres, int K, int* assign, long long* sums, int* changed, void* stream);
int ig_split_nearest(const int* a, int Na, const int* b, int Nb, unsigned long long* d2, int* idx, void* stream);
int ig_confusion_update(const long long* y_true, const long long* y_pred, unsigned long long* confusion, long n, int k,
                        long ignore_index, int has_ignore, void* stream);
/* torch.optim.AdamW step on a flat buffer (+ clip_weights, + bf16 shadow refresh)        base.py:103-126 */
int ig_adamw_advance(float* hyper, void* stream);
int ig_adamw_step(float* p, const float* g, float* m, float* v, void* shadow_hi, void* shadow_lo, const float* hyper, long n,
                  void* stream);

#ifdef __cplusplus
}
#endif
#endif /* INSTAGEO_HIP_H */
