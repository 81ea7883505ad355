/* cvae_hip.h — C ABI of libcvae_hip.so: the MI355X (gfx950) kernels behind the CausalVAE train step.
 *
 * Boundary contract (SURVEY.md §8(b) "lower boundary"):
 *   - extern "C", plain device pointers + sizes; no torch / C++ types.
 *   - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*); it never allocates or
 *     frees device memory, never synchronises, never throws.  All buffers (inputs, outputs, workspace)
 *     are owned by the caller (the torch caching allocator on the Python side).
 *   - return 0 (CVAE_OK) or a negative CVAE_E_* code; cvae_strerror() names it.
 *
 * Tensor conventions
 *   - conv activations are CHANNELS-LAST: [B, D, H, W, C] (D == 1 for 2D), dtype = CVAE_F32 or CVAE_BF16.
 *   - every k4/s2/p1 convolution pair is described by its SMALL tensor S [B, sd, sh, sw, Cs] and its LARGE
 *     tensor L [B, ld, lh, lw, Cl] with l = 2*s - 1 + k (k = 0..3) per strided dim; nd = 2 keeps D unstrided
 *     (sd == ld == 1, one depth tap).  The weight W is fp32 [Cs][Cl][taps] — exactly nn.Conv{2,3}d.weight
 *     ([C_out][C_in][k..], S = output) and nn.ConvTranspose{2,3}d.weight ([C_in][C_out][k..], S = input).
 *       down : S = act(gather(L, W) + bias)   = Conv forward            = ConvTranspose backward-data
 *       up   : L = act(scatter(S, W) + bias)  = ConvTranspose forward   = Conv backward-data
 *       wgrad: dW[cs][cl][k] = sum S[.., cs] * L[2s-1+k, cl]            = both weight gradients
 *   - linear layers, losses, BN, reparameterisation and Adam are fp32.
 *
 * Reference interfaces replaced (file:line in /root/reference):
 *   conv_down/up/wgrad ........ nn.Conv2d / nn.ConvTranspose2d fwd+bwd   causal_cascade/models.py:12-16,50-55;
 *                                                                        mnist_test/01_baseline_causal_vae/models.py:19-23,45-48
 *   adaptive_avgpool .......... nn.AdaptiveAvgPool2d((4,4)) + Flatten    causal_cascade/models.py:18-19
 *   upsample_linear ........... F.interpolate(bilinear, align_corners=False)  causal_cascade/models.py:87
 *   linear_* .................. nn.Linear (+ReLU/LeakyReLU)              causal_cascade/models.py:24-31,35-44
 *   bn1d_* .................... nn.BatchNorm1d(64)                       causal_cascade/models.py:36
 *   reparam_kld_* ............. reparameterize + KLD term                causal_cascade/models.py:65-68, train.py:13
 *   sse / bce / wmse_sparsity / gauss_nll .. loss terms                  causal_cascade/train.py:7,10;
 *                                            mnist_test/01_baseline_causal_vae/train.py:70; vessel_analysis/01_train/train.py:27-58
 *   softmax_ce / uniform_kl ... F.cross_entropy, F.kl_div(log_softmax)   mnist_test/01_baseline_causal_vae/train.py:56,82-85
 *   adam_step / sqnorm ........ optim.Adam.step, clip_grad_norm_         causal_cascade/main.py:50, train.py:34;
 *                                                                        vessel_analysis/01_train/train.py:85-86
 */
#ifndef CVAE_HIP_H
#define CVAE_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CVAE_OK             0
#define CVAE_E_BADSHAPE    (-1)
#define CVAE_E_DTYPE       (-2)
#define CVAE_E_UNSUPPORTED (-3)
#define CVAE_E_WORKSPACE   (-4)
#define CVAE_E_LAUNCH      (-5)
#define CVAE_E_NULLPTR     (-6)

#define CVAE_F32  0
#define CVAE_BF16 1
#define CVAE_FP8  2          /* OCP e4m3 codes with a per-tensor scale kept by the caller (cvae_conv_fp8 ...) */

#define CVAE_ACT_NONE    0
#define CVAE_ACT_RELU    1
#define CVAE_ACT_SIGMOID 2
#define CVAE_ACT_LEAKY02 3   /* LeakyReLU(0.2) */
#define CVAE_ACT_LEAKY001 4  /* LeakyReLU() with torch's default slope 0.01 */

int         cvae_version(void);
const char* cvae_strerror(int code);

/* ---- layout / precision plumbing -------------------------------------------------------------- */
/* [B, C, S] (torch NC(D)HW, S = spatial voxels) -> channels-last [B, S, C], converting dtype on the way. */
int cvae_ncs_to_nsc(const void* src, void* dst, int64_t B, int64_t C, int64_t S, int src_dtype, int dst_dtype, void* stream);
int cvae_nsc_to_ncs(const void* src, void* dst, int64_t B, int64_t C, int64_t S, int src_dtype, int dst_dtype, void* stream);
int cvae_cast(const void* src, void* dst, int64_t n, int src_dtype, int dst_dtype, void* stream);
/* Up to 8 panels in one launch (host arrays of device pointers / widths / row strides): gather == 0: wide[b][col0 + off_i + j] = panels[i][b * strides[i] + j]
 * with off_i = widths[0] + .. + widths[i-1] (torch.cat(dim=1)); gather != 0: the reverse copy (the column ranges of `wide` out into the panels: cat's backward). */
int cvae_copy_panels(float* const* panels, const int64_t* widths, const int64_t* strides, int count, float* wide, int64_t B, int64_t wide_stride, int64_t col0,
                     int gather, void* stream);
/* dst[b, col0 + t[b]] = 1, other columns of the panel 0 (F.one_hot(t, n).float() into a concat panel). */
int cvae_onehot_panel(const int64_t* t, float* dst, int64_t B, int64_t n_classes, int64_t dst_stride, int64_t col0, void* stream);

/* ---- k4 s2 p1 convolution family ---------------------------------------------------------------- */
/* fp32 W [Cs][Cl][taps] -> MFMA operand panels in the compute dtype.
 *   for_up == 0: [tap][Cl/16][Cs][16]   (down: N = Cs, K = (tap, cl))
 *   for_up == 1: [tap][Cs/16][Cl][16]   (up  : N = Cl, K = (tap, cs))
 * Not needed (pass the fp32 W itself as `w`) when Cl == 1. */
int cvae_conv_pack_weight(const float* w, void* packed, int64_t Cs, int64_t Cl, int nd, int for_up, int dtype, void* stream);

/* Both packings (for_up = 0 and 1) of a LIST of weights in one launch through an LDS transpose (Cs and Cl multiples of 16).
 * For a training step with fp8 forward products: f8dir[i] = 1 / 2 writes the `down` / `up` panel of weight i as fp8 codes of w * *inv_scale_dev[i] into
 * f8out[i] (layout of cvae_conv_pack_weight_fp8) INSTEAD of its bf16 panel (packed_down[i] / packed_up[i] may then be NULL), and records max |w| in
 * amax_slots[i] (optional); f8dir[i] = 0 (or f8dir == NULL, f8out / inv_scale_dev / amax_slots then unused): both bf16 / fp32 panels. */
int cvae_conv_pack_weight_pairs(const float* const* w, void* const* packed_down, void* const* packed_up, const int64_t* Cs, const int64_t* Cl,
                                const int* f8dir, void* const* f8out, const float* const* inv_scale_dev, void* const* amax_slots,
                                int count, int nd, int dtype, void* stream);

/* Optional scratch for cvae_conv_down (for_up = 0) / cvae_conv_up (for_up = 1): layers whose output grid is too small to fill
 * the chip (8^3, 4^3 volumes) split the input-channel loop over workgroups and sum fp32 partial tiles from this buffer.
 * Returns 0 when the launch needs none.  Passing NULL / a smaller buffer is always valid: the launch then runs unsplit. */
size_t cvae_conv_data_workspace_bytes(int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                                      int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int for_up);
/* cvae_conv_down: S = act(gather(L, w) + bias) [then * (mask > 0) if mask != NULL].  bias fp32 [Cs] or NULL; mask has S's shape/dtype.
 * cvae_conv_up:   L = act(scatter(S, w) + bias) [then * (mask > 0) if mask != NULL].  bias fp32 [Cl] or NULL; mask has L's shape/dtype.
 * ReLU masks as BITS.  The backward-data launch of a layer whose input was a ReLU output zeroes its result where that activation was not positive
 * (`mask` = the saved activation, read in full: 67 MB for enc_conv[2]'s backward at 4 x 128^3).  In the bit form the PRODUCING forward launch leaves
 * one bit per element of its result — dword i covers elements 32 i .. 32 i + 31 in memory order (a position's 32-channel block; channel counts % 32 == 0),
 * bit set <=> element > 0 — and the backward launch reads those (1/16 of the bf16 bytes).
 *   relu_bits_out (optional): numel / 32 dwords that receive the mask of THIS launch's result;  mask_bits (optional): the mask to apply, in place of
 *                 `mask` (passing both is CVAE_E_BADSHAPE).  Either bit pointer needs the result's channel count % 32 == 0 and, in `up`, Cl > 1;
 *                 `down` with Cl == 1 reads mask_bits in bf16 only (CVAE_E_UNSUPPORTED otherwise).
 * Kernel forms, chosen by launch size unless the CALLER forces one for this call (the library keeps no process-wide tuning state).  Every form computes
 * the same products in the same order (bit-identical results; the tests run each narrow case through both):
 *   xpair         -1 automatic; 0 / 1: one sample per tile / two side by side — layers at most half a tile wide: 2D grids up to 8 wide (the 7 x 7 maps
 *                 of the MNIST model; automatic from 512 workgroups up) and, in `up`, 3D layers at most 4 source voxels wide (the decoder's 4^3 input;
 *                 automatic from 2048 workgroups up);
 *   upfull        -1 automatic; 0 / 1: never / whenever it fits — the whole-K `up` kernel (bf16, 64 / 128 / 256 input channels, 32 output channels).
 *                 It has no bit form: with mask_bits or relu_bits_out the launch takes the bit form and upfull has no effect;
 *   c1_walk_units  0 automatic; > 0: the single-channel output layer (bf16, 3D) walks z columns when the launch has at least 2 x this many tiles. */
int cvae_conv_down(const void* L, const void* w, const float* bias, const void* mask, const void* mask_bits, void* S, void* relu_bits_out,
                   int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                   int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int dtype, int act,
                   void* workspace, size_t workspace_bytes, int xpair, void* stream);
int cvae_conv_up(const void* S, const void* w, const float* bias, const void* mask, const void* mask_bits, void* L, void* relu_bits_out,
                 int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                 int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int dtype, int act,
                 void* workspace, size_t workspace_bytes, int upfull, int xpair, int64_t c1_walk_units, void* stream);
/* The input gradient of cvae_conv_down (2D, k4/s2/p1) with the derivative of the PRODUCING activation in its epilogue:
 *   dx = scatter(g, w) * act'(gate), the multiplication on the fp32 accumulator before the one rounding to `dtype`; gate (NULL with CVAE_ACT_NONE) of dx's
 *   shape and dtype; act'(gate) = gate > 0 ? 1 : slope of gate_act (CVAE_ACT_NONE / RELU / LEAKY02 / LEAKY001), read off the activation's OUTPUT.
 * g [B][sh][sw][Cs], dx [B][lh][lw][Cl], w the packed `up` weight of cvae_conv_pack_weight(for_up = 1).  cvae_conv_up's tiles, dispatch, workspace and per-call
 * form overrides (upfull, xpair): NONE and RELU ARE cvae_conv_up launches (without / with `mask`: the same bits); a LeakyReLU slope runs second instances of
 * the same kernel text that multiply where the first ones zero (the data kernel, the split-K finish, the whole-K parity kernel).  nd = 2, Cs % 16 == 0 and
 * Cl % 32 == 0, else CVAE_E_UNSUPPORTED (nothing is launched).  The ViT-VAE stem's backward: one launch per layer, no cvae_act_bwd pass. */
int cvae_conv_down_bwd_data(const void* g, const void* w, const void* gate, void* dx, int64_t B, int64_t sh, int64_t sw, int64_t Cs, int64_t lh, int64_t lw,
                            int64_t Cl, int nd, int dtype, int gate_act, void* workspace, size_t workspace_bytes, int upfull, int xpair, void* stream);
/* The first conv of the encoder (Cl == 1) with the IMAGE read in the dtype it is stored in (l_dtype) while S is written in the compute
 * dtype (`dtype`): the fp32 input volume of a bf16 model feeds the kernels directly — no cast pass, no bf16 copy of the batch
 * (causal_cascade/models.py:13: nn.Conv2d(img_channels, 32, 4, 2, 1) on the fp32 batch).  cvae_conv_down_image = cvae_conv_down with
 * Cl == 1 (w = the fp32 master weight); cvae_conv_wgrad_image = cvae_conv_wgrad with Cl == 1 and the S-side bias sum.  The mixed
 * (fp32 image, bf16 S) forward reads 16-byte rows: it needs lw % 4 == 0 and a 16-byte aligned image (cvae_conv_image_supported == 1),
 * otherwise cast the image and use the plain entry points. */
int cvae_conv_image_supported(const void* L, int64_t lw, int l_dtype, int dtype);
int cvae_conv_down_image(const void* L, int l_dtype, const float* w, const float* bias, const void* mask, void* S,
                         int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, int act, void* stream);
int cvae_conv_wgrad_image(const void* S, const void* L, int l_dtype, float* dW, float* dbias, void* workspace, size_t workspace_bytes,
                          int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int dtype, void* stream);
/* The input gradient of that first conv: the gradient with respect to the IMAGE, as an fp32 result whatever the operand dtype (csrc/conv_c1.hip).
 *   g   channels-last [B][sh][sw][32], `dtype` CVAE_F32 or CVAE_BF16: the gradient of the layer's pre-activation;
 *   w   the fp32 k4 weight [32][1][4][4] as cvae_fold_bn_conv leaves it.  It is NOT rounded in bf16 mode: a bf16 g is widened exactly and every product and
 *       sum is fp32, so the result's error is fp32 rounding alone in both modes;
 *   dx  fp32 [B][1][2 sh][2 sw]:  s[b][y][x] = sum_{c, ky, kx} g[b][sy][sx][c] w[c][0][ky][kx] over the positions with 2 sy - 1 + ky = y and 2 sx - 1 + kx = x
 *       (at most 2 x 2 source positions x 32 channels);  accumulate == 0: dx = alpha * s;  accumulate != 0: dx = fma(alpha, s, dx).
 * Every element of dx is written by exactly one thread: no atomics, no workspace.  The order of an element's sum depends on (sh, sw) and its position only — per
 * neighbouring source position (row-major) a 16-term fma chain per channel half started at 0, added to the element's partial, the two halves added last — so the
 * result is bit-reproducible and a batch row's bits do not depend on B.
 * Any sh, sw >= 1 (no tile multiple is asked for).  Every check precedes the launch: negative B or a size < 1: CVAE_E_BADSHAPE; a dtype code other than the two:
 * CVAE_E_DTYPE; nd != 2, Cs != 32, (lh, lw) != (2 sh, 2 sw) or B sh sw >= 2^30: CVAE_E_UNSUPPORTED; then B == 0 is CVAE_OK (nothing is launched); a null pointer:
 * CVAE_E_NULLPTR; g not 16-byte aligned, w or dx not 4-byte aligned, or dx overlapping g or w: CVAE_E_UNSUPPORTED. */
int cvae_conv_down_image_bwd_data(const void* g, const float* w, float* dx, int64_t B, int64_t sh, int64_t sw, int64_t Cs, int64_t lh, int64_t lw, int nd, int dtype,
                                  float alpha, int accumulate, void* stream);
/* ---- fp8 (OCP e4m3) products (BASELINE.json configs[4]): the batched counterfactual decode (replaces the per-value decode loop of
 * vessel_analysis/04_generate_counterfactual/generate_counterfactual.py:77-99) and the forward convolutions of the train step
 * (causal_cascade/train.py:19-39 with fp8 conv inputs; the backward pass stays bf16) ----
 * A tensor x is held as fp8 codes q with a per-tensor scale s kept by the caller: x ~ s * q.  Products accumulate in fp32 on the block-scaled
 * CDNA4 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, unit block scales): twice the bf16 FLOPs per clock.  Channel counts: C_in % 32 == 0,
 * C_out % 64 == 0 (conv) / C_out % 32 == 0, C_out > 1 (ConvTranspose).
 *   cvae_quantize_fp8           dst[i] = fp8(src[i] * inv_scale)               (src fp32 or bf16; saturating); inv_scale_dev (optional): 1 / s read from
 *                               DEVICE memory instead of the by-value inv_scale; amax_slots (optional): records max |src| (see below)
 *   cvae_absmax                 max |src| into amax_slots (calibration of the first step)
 *   cvae_conv_pack_weight_fp8   fp32 [Cs][Cl][taps] -> operand panels [tap][C_in / 32][C_out][32] of fp8(w * inv_scale)
 *   cvae_conv_pack_weights_fp8  the same for a list of layers in one launch, 1 / s_w read from device memory, max |w| recorded
 *   cvae_conv_fp8               up = 0: S = act(conv(L_q, w_q) * acc_scale + bias); up = 1: L = act(scatter(S_q, w_q) * acc_scale + bias), acc_scale =
 *                               s_in * s_w.  out_dtype CVAE_BF16: `out` bf16, and `out8` (optional) a second copy as codes fp8(out * out8_inv_scale) for
 *                               the next fp8 layer; out_dtype CVAE_FP8: `out` holds the codes only.  dscale (optional, device): {acc_scale,
 *                               out8_inv_scale} read at run time instead of the two by-value arguments (delayed scaling under graph replay).
 *                               amax_slots (optional): records max |out|.  workspace: cvae_conv_data_workspace_bytes of the same geometry (split-K
 *                               of the small `down` grids; NULL = unsplit).  xpair: as in cvae_conv_down / cvae_conv_up (-1 = automatic).  relu_bits_out
 *                               (optional): the ReLU mask of `out` as bits (as in cvae_conv_down / cvae_conv_up).
 *   cvae_fp8_scale_update       once per step: for each of n tracked tensors, scale[i] = headroom * amax_i / 448 (amax_i = the largest value
 *                               recorded in its CVAE_AMAX_SLOTS words since the last call; the words are cleared; nothing recorded = scale kept),
 *                               inv_scale[i] = 1 / scale[i]; then for each fp8 layer l: dscale[2l] = scale[layer_in[l]] * scale[layer_w[l]],
 *                               dscale[2l + 1] = 1 / scale[layer_out[l]] (0 when layer_out[l] < 0).  layer_* are HOST arrays; `ticket` is one device
 *                               word, zero before the first call (the kernel's workgroups count themselves in on it and the last one resets it).
 * An amax record is CVAE_AMAX_SLOTS unsigned words holding float bits (non-negative floats order like unsigned integers; atomicMax, so the
 * result does not depend on the order of arrival; one word per workgroup of the producing launch, modulo the slot count); the caller zero-fills it once. */
#define CVAE_AMAX_SLOTS 4096
int cvae_quantize_fp8(const void* src, int src_dtype, void* dst, int64_t n, float inv_scale, const float* inv_scale_dev, void* amax_slots, void* stream);
int cvae_absmax(const void* src, int dtype, int64_t n, void* amax_slots, void* stream);
int cvae_conv_pack_weight_fp8(const float* w, void* packed, int64_t Cs, int64_t Cl, int nd, int for_up, float inv_scale, void* stream);
int cvae_conv_pack_weights_fp8(const float* const* w, void* const* packed, const int64_t* Cs, const int64_t* Cl, const int* for_up,
                               const float* const* inv_scale_dev, void* const* amax_slots, int count, int nd, void* stream);
int cvae_conv_fp8(int up, const void* in8, const void* w8, const float* bias, void* out, int out_dtype, void* out8, const float* dscale, float acc_scale,
                  float out8_inv_scale, void* amax_slots, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int64_t Cl,
                  int nd, int act, void* workspace, size_t workspace_bytes, int xpair, void* relu_bits_out, void* stream);
/* The decode sweep's last layer fed by the fp8 layer before it: nn.ConvTranspose3d(32, 1, 4, 2, 1) (causal_cascade/models.py:54 lifted to 3D) of S8 [B][sd][sh][sw][32] e4m3
 * codes (activation / in_scale, e.g. the codes cvae_conv_fp8 leaves with out_dtype CVAE_FP8), fp32 master weight w [32][1][64] and bias as they are: L [B][2sd][2sh][2sw][1] bf16 =
 * act(in_scale * (S8 (*) w) + bias).  The 32-channel tensor between the last two layers travels at one byte per element and is never widened in memory.  3D, Cs == 32 only. */
int cvae_conv_up_c1_fp8in(const void* S8, const float* w, const float* bias, void* L, float in_scale, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int nd, int act,
                          void* stream);
/* cvae_conv_down_image with bf16 S and the fp8 side channel of a training forward whose next conv runs on fp8 operands: S8 (optional) = fp8(S * *inv_scale_dev),
 * amax_slots (optional) records max |S|, relu_bits_out (optional) receives the ReLU mask of S as bits (as in cvae_conv_down; this entry point also serves a
 * bf16 step that only wants the bits: S8 = NULL).  Needs the 16-byte-row form (cvae_conv_image_supported). */
int cvae_conv_down_image_f8(const void* L, int l_dtype, const float* w, const float* bias, void* S, void* S8, const float* inv_scale_dev, void* amax_slots,
                            void* relu_bits_out, int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs, int64_t ld, int64_t lh, int64_t lw, int nd, int act,
                            void* stream);
int cvae_fp8_scale_update(void* amax_slots, float* scale, float* inv_scale, int n, float headroom, const int* layer_in, const int* layer_w, const int* layer_out,
                          int n_layers, float* dscale, void* ticket, void* stream);
/* ---- Exact-2x linear resize (decoder output d x h x w, one channel -> 2d x 2h x 2w; D == d == 1 for 2D) fused with the ELBO ----
 * causal_cascade/models.py:84-87 + train.py:5-17: the resized volume is recomputed from the small tensor wherever it is needed
 * instead of being written and re-read (csrc/recon_loss.hip).  cvae_up2x_supported: 1 when the shapes qualify (w % 4 == 0). */
int cvae_up2x_supported(int64_t B, int64_t d, int64_t h, int64_t w, int64_t D, int64_t H, int64_t W);
/* dst fp32 [B][D][H][W] = F.interpolate(src, (D, H, W), 'trilinear' | 'bilinear', align_corners=False) */
int cvae_up2x_fwd(const void* src, float* dst, int64_t B, int64_t d, int64_t h, int64_t w, int64_t D, int64_t H, int64_t W, int dtype, void* stream);
/* out4 = {loss, recon, m_loss, kld}: recon = sum (up(src) - x)^2, m_loss = sum (m_hat - m)^2 (n_m elements),
 * kld = -0.5 sum (1 + logvar - mu^2 - exp(logvar)) (n_z elements), loss = recon + gamma * m_loss + kld.
 * partial: scratch of cvae_elbo_up2x_partials(B, d, h, w) floats (per-workgroup sums, added in a fixed order: no atomics). */
#define CVAE_ELBO_TICKET_WORDS (33 * 32)
int64_t cvae_elbo_up2x_partials(int64_t B, int64_t d, int64_t h, int64_t w);
int cvae_elbo_up2x_fwd(const void* src, const float* x, const float* m_hat, const float* m, const float* mu, const float* logvar, float gamma,
                       float* out4, float* partial, float* t1, void* ticket, int* bump, int64_t B, int64_t d, int64_t h, int64_t w, int64_t D, int64_t H, int64_t W,
                       int64_t n_m, int64_t n_z, int dtype, void* stream);
/* ticket (optional): CVAE_ELBO_TICKET_WORDS device words, zero before the first call — the launch then finishes the sums itself (the workgroup that arrives
 * last, found by a two-level arrival count, adds the partials in index order: same bits as the two-launch form, one dependent launch fewer; the words are
 * zero again when the launch ends).  bump (optional,
 * needs ticket): a device int incremented once by that last workgroup — the optimizer's device step counter rides along (cvae_adam_multi's step_dev). */
/* t1 (B*D*H*w floats, or NULL when no backward follows): the same launch also leaves U_w^T (up(src) - x), the part of the backward that needs x,
 * so that a training step reads x once.  cvae_elbo_up2x_bwd turns it into the gradients of `loss` scaled by the device scalar *g_loss (NULL = 1):
 * dsrc (dtype), d_mhat, dmu, dlv. */
int cvae_elbo_up2x_bwd(const float* t1, const float* m_hat, const float* m, const float* mu, const float* logvar, float gamma, const float* g_loss,
                       void* dsrc, float* d_mhat, float* dmu, float* dlv, int64_t B, int64_t d, int64_t h, int64_t w, int64_t D, int64_t H, int64_t W,
                       int64_t n_m, int64_t n_z, int dtype, void* stream);

/* ---- CausalVesselVAE extras (vessel_analysis/00_core/models.py:9-166): BatchNorm2d, clamp, Upsample(nearest x2) + Conv2d(k3, s1, p1) ----
 * nn.Upsample(scale_factor=2, 'nearest') followed by nn.Conv2d(Cin, Cout, 3, 1, 1) equals the transposed k4/s2/p1 product of
 * cvae_conv_up with K4[cin][cout] = A W3[cout][cin] A^T, A = [[0,0,1],[0,1,1],[1,1,0],[1,0,0]] (csrc/vessel2d.hip): the layer runs on
 * cvae_conv_up / cvae_conv_down / cvae_conv_wgrad with the transformed weight; its gradient maps back with A^T . A. */
int cvae_conv3_to_k4(const float* w3 /* [Cout][Cin][3][3] */, float* k4 /* [Cin][Cout][4][4] */, int64_t Cout, int64_t Cin, void* stream);
int cvae_k4_to_conv3_grad(const float* dk4, float* dw3, int64_t Cout, int64_t Cin, void* stream);
/* torch.clamp(x, lo, hi) and its backward (the gradient passes where lo <= x <= hi); fp32 */
int cvae_clamp_fwd(const float* x, float* y, float lo, float hi, int64_t n, void* stream);
int cvae_clamp_bwd(const float* x, const float* g, float* dx, float lo, float hi, int64_t n, void* stream);
/* nn.BatchNorm2d (+ fused activation `act`) on a channels-last tensor [P = B*H*W][C], P >= 1 (training: P >= 2), 8 <= C <= 2048 and
 * C % 8 == 0, else CVAE_E_BADSHAPE; x, dy, y, dx 16-byte aligned (16-byte loads and stores without a fallback).  training: two-pass batch
 * statistics (mean, then sum of squared deviations) into mean / rstd, running_mean / running_var updated with the unbiased variance
 * (either may be NULL, each on its own); otherwise mean / rstd are inputs (running mean, 1/sqrt(running_var + eps)) and the running
 * statistics and the workspace are not touched.  y = act((x - mean) rstd gamma + beta). */
/* workspace: cvae_bn2d_workspace_bytes(P, C) (0 for a shape the entries refuse) — per-workgroup partial rows of the channel statistics,
 * added in index order by the finalize launches (no float atomics; required in training mode and by the backward: NULL is
 * CVAE_E_NULLPTR, too small CVAE_E_WORKSPACE, both before any launch; the forward uses one set of rows and is satisfied with half of
 * cvae_bn2d_workspace_bytes, the backward needs all of it). */
size_t cvae_bn2d_workspace_bytes(int64_t P, int64_t C);
int cvae_bn2d_fwd(const void* x, const float* gamma, const float* beta, void* y, float* mean, float* rstd, float* running_mean, float* running_var,
                  int64_t P, int64_t C, float momentum, float eps, int training, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* training-mode backward through the activation and the normalisation: dx, dgamma, dbeta (y = the forward's output, for act') */
int cvae_bn2d_bwd(const void* x, const void* dy, const void* y, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                  float* dbeta, int64_t P, int64_t C, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* Batch-statistics BatchNorm2d forward that reads its input twice (csrc/bn2d_batch.hip): the ViT-VAE stem's training walk.
 *   y channels-last [P][C] in `dtype` (CVAE_F32 / CVAE_BF16): the conv output; a = act((y - mean) rstd gamma + beta), same shape and dtype; mean, rstd fp32 [C]
 *   are OUTPUTS (the batch's mean and 1 / sqrt(biased variance + eps)): with (x = y, y = a) they are what cvae_bn2d_bwd reads.  running_mean / running_var
 *   (both or neither): updated in place as torch does, r = (1 - momentum) r + momentum * (mean | unbiased variance).
 * Three launches: per-chunk (mean, M2) from sums shifted by the chunk's first row (one read of y), the chunks merged in index order with the pairwise
 * update, then the apply pass (one read of y, one write of a).  The chunking is a function of P alone; no float atomics: bit-reproducible on every device.
 * workspace: cvae_bn2d_batch_workspace_bytes(P, C) (0 for a shape the entry refuses), 4-byte aligned.
 * Every check precedes the first launch: P < 2 (torch: "Expected more than 1 value per channel"), P > 2^40, C < 8, C % 8 != 0, C > 2048, momentum outside
 * [0, 1] or NaN, eps <= 0 or NaN: CVAE_E_BADSHAPE; an act code that is no CVAE_ACT_*: CVAE_E_UNSUPPORTED; a null pointer (the workspace included, or one
 * running buffer without the other): CVAE_E_NULLPTR; y or a not 16-byte aligned, a float array not 4-byte aligned: CVAE_E_UNSUPPORTED; a workspace below the
 * query: CVAE_E_WORKSPACE; a dtype code other than the two: CVAE_E_DTYPE. */
size_t cvae_bn2d_batch_workspace_bytes(int64_t P, int64_t C);
int cvae_bn2d_batch_fwd(const void* y, const float* gamma, const float* beta, void* a, float* mean, float* rstd, float* running_mean, float* running_var,
                        int64_t P, int64_t C, float momentum, float eps, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* The forward with a residual (the BatchNorm that ends a ResBlock): cvae_bn2d_batch_fwd's arguments plus `resid`, of y's shape and dtype,
 * 16-byte aligned.  a = resid + ((y - mean) rstd gamma + beta), the sum formed in fp32 and rounded once; the same moments and finish launches, an apply
 * instance that reads y and resid once and writes a once.  resid with act != CVAE_ACT_NONE: CVAE_E_UNSUPPORTED (behind an activation `a` would no longer
 * carry the sign the backward reads).  resid == NULL: cvae_bn2d_batch_fwd.  Every other check and code as there. */
int cvae_bn2d_batch_fwd_res(const void* y, const float* gamma, const float* beta, void* a, float* mean, float* rstd, float* running_mean, float* running_var,
                            int64_t P, int64_t C, float momentum, float eps, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream,
                            const void* resid);
/* The backward of a = act((y - mean) rstd gamma + beta) with batch statistics, on the forward's chunking: y, dy, a, dx channels-last [P][C]
 * in `dtype`; gamma, mean, rstd fp32 [C] (mean / rstd as the forward left them); dgamma, dbeta fp32 [C].  With g = dy act'(a) (act' read off the activation's
 * output a; a may be NULL when act == CVAE_ACT_NONE and is then not read) and xh = (y - mean) rstd: dbeta = sum g, dgamma = sum g xh,
 * dx = gamma rstd (g - dbeta / P - xh dgamma / P).  Three launches: per-chunk sums (one workgroup per chunk, the chunk read once), the partials added in an
 * order set by the chunk count alone, the apply pass (y, dy, a read once, dx written once).  No float atomics: bit-reproducible on every device.
 * workspace: cvae_bn2d_batch_bwd_workspace_bytes(P, C) (0 for a shape the entry refuses), 4-byte aligned.  Checks, all before the first launch, with the
 * forward's codes: shape CVAE_E_BADSHAPE; act code CVAE_E_UNSUPPORTED; a null pointer CVAE_E_NULLPTR; y, dy, a, dx not 16-byte aligned or a float array not
 * 4-byte aligned CVAE_E_UNSUPPORTED; a short workspace CVAE_E_WORKSPACE; a dtype code other than the two CVAE_E_DTYPE. */
size_t cvae_bn2d_batch_bwd_workspace_bytes(int64_t P, int64_t C);
int cvae_bn2d_batch_bwd(const void* y, const void* dy, const void* a, const float* gamma, const float* mean, const float* rstd, void* dx, float* dgamma,
                        float* dbeta, int64_t P, int64_t C, int act, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- CausalVesselVAE inference (csrc/vessel_infer.hip): eval-mode BatchNorm2d folded into the convs, sweep reductions ---------------------
 * Fold a table of `count` (1..16, else CVAE_E_UNSUPPORTED) conv layers with the eval-mode BatchNorm2d behind them in ONE launch (host arrays
 * of device pointers, dims = count rows of {Cout, Cin}).  Per output channel c: s = gamma[c] rsqrt(var[c] + eps[k]),
 * w_out[c] = w[c] s, b_out[c] = (bias[c] - mean[c]) s + beta[c] — the conv then runs with the activation in its epilogue and no BatchNorm pass.
 *   kind CVAE_FOLD_CONV_K4:   w = nn.Conv2d(k4) weight [Cout][Cin][4][4], w_out in the same layout;
 *   kind CVAE_FOLD_UPCONV_K3: w = the Conv2d(k3) of an Upsample(x2, nearest) + Conv2d pair [Cout][Cin][3][3], w_out the transposed k4 weight
 *                             [Cin][Cout][4][4] = A W3 A^T of cvae_conv3_to_k4 (same sums, same order);
 *   kind CVAE_FOLD_CONV_K3S2: w = nn.Conv2d(k3, s2, p1) weight [Cout][Cin][3][3] (the ViT-VAE stem), w_out the k4/s2/p1 weight [Cout][Cin][4][4] with
 *                             w_out[..][kh][kw] = w[..][kh][kw] s for kh, kw < 3 and a zero fourth row and column: both kernels read in[2 o - 1 + k] and
 *                             give equal output extents on even inputs, so cvae_conv_down with w_out computes the k3 layer (16 taps issued for 9).
 * gamma NULL (the array, or its entry k): no BatchNorm — the plain transform, bias copied (a NULL bias entry counts as zeros); otherwise beta /
 * mean / var entries are required.  w and w_out 16-byte aligned (an UpConv2dK3 with Cin % 4 != 0: w_out only), else CVAE_E_UNSUPPORTED.
 * Outputs fp32. */
#define CVAE_FOLD_CONV_K4   0
#define CVAE_FOLD_UPCONV_K3 1
#define CVAE_FOLD_CONV_K3S2 3   /* 2 stays unassigned */
/* The ViT-VAE decoder's kinds (dims rows stay {Cout, Cin} with Cout the BatchNorm's channel count; outputs fp32):
 *   kind CVAE_FOLD_CONVT_K3S2:          w = nn.ConvTranspose2d(k3, s2, p1, output_padding 1) weight [Cin][Cout][3][3], w_out the transposed k4/s2/p1 weight
 *                                       [Cin][Cout][4][4] of cvae_conv_up with w_out[..][kh][kw] = w[..][kh][kw] s[cout] for kh, kw < 3 and a zero fourth row and
 *                                       column: both scatter in[i] to out[2 i - 1 + k], and the k4 extent 2 n is the k3 extent with output_padding 1;
 *   kind CVAE_FOLD_CONV_K3S1:           w = nn.Conv2d(k3, s1, p1) weight [Cout][Cin][3][3], w_out the GEMM matrix [Cout][KT] of cvae_conv_s1 (form
 *                                       CVAE_CONV_S1_K3): w_out[co][(ky 3 + kx) Cin + ci] = w[co][ci][ky][kx] s[co], KT = 9 Cin rounded up to 64, zero columns behind;
 *   kind CVAE_FOLD_CONVT_K3S2_SUBPIXEL: w as CVAE_FOLD_CONVT_K3S2, w_out the GEMM matrix [4 Cout][KT] of cvae_conv_s1 (form CVAE_CONV_S1_SUBPIXEL): row
 *                                       (py 2 + px) Cout + co, column (dy 2 + dx) Cin + ci holds w[ci][co][ky][kx] s[co] with, per direction, parity 0: {d 0 -> k 1},
 *                                       parity 1: {d 0 -> k 2, d 1 -> k 0} and zero elsewhere; KT = 4 Cin rounded up to 64.
 * The two GEMM kinds need Cin % 4 == 0 (else CVAE_E_UNSUPPORTED). */
#define CVAE_FOLD_CONVT_K3S2          4
#define CVAE_FOLD_CONV_K3S1           5
#define CVAE_FOLD_CONVT_K3S2_SUBPIXEL 6
/* The same two GEMM kinds with the matrix of the layer's INPUT GRADIENT (cvae_conv_s1_bwd_data) written behind the forward matrix, w_out = [forward | backward]
 * (the forward part bit for bit what kinds 5 / 6 write; the BatchNorm scale s[co] sits on the backward matrix's K side):
 *   kind CVAE_FOLD_CONV_K3S1_GRAD:           + [Cin][KT]: column (ky 3 + kx) Cout + co of row ci holds w[co][ci][2 - ky][2 - kx] s[co] (taps flipped, channels
 *                                            transposed), KT = 9 Cout rounded up to 64;
 *   kind CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD: + [32][256]: column (dy 2 + dx) 64 + (py 2 + px) 16 + co of row ci holds w[ci][co][2 dy + py - 1][2 dx + px - 1] s[co]
 *                                            where both tap indices are >= 0, zero elsewhere and in rows ci >= Cin (Cout = 16 only, else CVAE_E_UNSUPPORTED). */
#define CVAE_FOLD_CONV_K3S1_GRAD           7
#define CVAE_FOLD_CONVT_K3S2_SUBPIXEL_GRAD 8
int cvae_fold_bn_conv(int count, const float* const* w, const int* kind, const int64_t* dims, const float* const* bias, const float* const* gamma,
                      const float* const* beta, const float* const* mean, const float* const* var, const float* eps, float* const* w_out,
                      float* const* b_out, void* stream);
/* The way back through the fold, for `count` (1..16) layers in ONE launch: from the gradient of the FOLDED weight dwf and bias dbf [Cout] to the gradients of
 * the module's parameters, with s = gamma rsqrt(var + eps) per BatchNorm channel (running statistics: constants):
 *   dw = s dwf,  db = s dbf,  dgamma = rsqrt(var + eps) (sum dwf w + dbf (bias - mean)),  dbeta = dbf.
 * kind CVAE_FOLD_CONVT_K3S2: dwf is the gradient of the k4 weight [Cin][Cout][4][4], of which the 3 x 3 taps are read; CVAE_FOLD_CONV_K3S2 (the ViT-VAE stem): the
 * gradient of the k4 weight [Cout][Cin][4][4] as cvae_conv_wgrad writes it, read the same way (the fourth row and column are ignored); CVAE_FOLD_CONV_K3S1: dwf [Cout][Cin][3][3];
 * CVAE_FOLD_CONVT_K3S2_SUBPIXEL: dwf [Cin][Cout][3][3] — both as cvae_conv_s1_wgrad writes them.  dw in w's layout.  One workgroup per (layer, channel): a
 * thread's ordered chain, then a fixed tree.  bias entries may be NULL (zeros; db then too); gamma NULL: no BatchNorm (dw = dwf, db = dbf, nothing else). */
int cvae_fold_bn_conv_bwd(int count, const float* const* w, const int* kind, const int64_t* dims, const float* const* bias, const float* const* gamma,
                          const float* const* mean, const float* const* var, const float* eps, const float* const* dwf, const float* const* dbf,
                          float* const* dw, float* const* db, float* const* dgamma, float* const* dbeta, void* stream);
/* l2[r] = ||a[r] - b[ref[r]]||_2 and (mean_abs != NULL) mean_abs[r] = mean |a[r] - b[ref[r]]| over rows of n elements; a holds `rows` rows,
 * b holds b_rows rows; ref: device int64[rows] (NULL: ref[r] = r, needs b_rows >= rows); a ref outside [0, b_rows) gives NaN for that row,
 * nothing is read.  dtype CVAE_F32 or CVAE_BF16 (a and b alike); sums in fp32.  workspace: cvae_row_diff_norms_workspace_bytes(rows, n, dtype) —
 * per-(row, chunk) partial sums, added by a second launch in a fixed order (no float atomics: the bits do not change from run to run, nor with
 * the number of rows in the call). */
size_t cvae_row_diff_norms_workspace_bytes(int64_t rows, int64_t n, int dtype);
int cvae_row_diff_norms(const void* a, const void* b, const int64_t* ref, float* l2, float* mean_abs, int64_t rows, int64_t b_rows, int64_t n,
                        int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* Element-wise over `count` (1..16, else CVAE_E_UNSUPPORTED) fp32 tensors of n elements (host array of device pointers):
 * mean = (x_0 + .. + x_{K-1}) / K, std = sqrt(sum_k (x_k - mean)^2 / (K - 1)) — torch.stack(x).mean(0) / .std(0) in the two-pass form;
 * K = 1 gives NaN std, as torch does.  Fixed order, no reductions across elements. */
int cvae_stack_mean_std(const float* const* x, int count, float* mean, float* std, int64_t n, void* stream);

/* ---- ViT-VAE encoder, eval mode (csrc/vit.hip; vessel_analysis/00_core/vit_backbone.py:158-179, latent_translator/models.py:95-110) ----------------
 * Transformer width 256, 8 heads x 32.  dtype CVAE_F32 (exact fp32 MFMA) or CVAE_BF16 (bf16 operands); accumulation, softmax, LayerNorm statistics and the
 * residual stream are fp32 in both.  No atomics: fixed-order sums, bit-reproducible, and a row's bits do not depend on the other rows of the launch.
 * Pointers 16-byte aligned, strides (in elements) multiples of 16 bytes, else CVAE_E_UNSUPPORTED.
 *   cvae_vit_tokens     tokens fp32 [B][n_patches + 1][256]: row 0 = cls + pos[0], row 1 + i = stem[b][i] + pos[1 + i]; stem [B][n_patches][256] (the channels-last
 *                       output of the last stem conv, stem_dtype fp32 or bf16), cls [256], pos [n_patches + 1][256]
 *   cvae_layernorm256   y[r] = (x[r] - mean) / sqrt(var + eps) * gamma + beta over 256 columns (biased variance, two-pass); x fp32 with row stride x_stride,
 *                       y [rows][256] in out_dtype
 *   cvae_token_gemm     y[M][N] = epi(x[M][K] W[N][K]^T + bias), (K, N) in {(256, 768), (256, 256), (256, 512), (512, 256)}; x in `dtype`, W / bias the fp32
 *                       nn.Linear tensors (W is rounded to bf16 on its way into LDS in bf16 mode).  epilogue NONE / GELU (exact erf): y in `dtype`;
 *                       RESIDUAL: y fp32 = resid + (x W^T + bias), resid fp32 with row stride resid_stride (y == resid: the residual stream in place)
 *   cvae_mhsa_fwd       out [B][n_query_rows][256] = softmax(q k^T / sqrt(32)) v per head, for the FIRST n_query_rows tokens as queries against all n_tokens
 *                       keys (n_query_rows = n_tokens: plain self-attention; 1: the CLS row of the last block).  q / k / v: row strides and batch strides in
 *                       elements, head h in columns 32 h .. 32 h + 31 (the packed in-projection output [B][n_tokens][768]: q, q + 256, q + 512, strides 768).
 *                       Online softmax over 64-key tiles; in bf16 mode P is rounded to bf16 for the P V product while its row sum stays fp32. */
#define CVAE_GEMM_EPI_NONE     0
#define CVAE_GEMM_EPI_GELU     1
#define CVAE_GEMM_EPI_RESIDUAL 2
int cvae_vit_tokens(const void* stem, int stem_dtype, const float* cls, const float* pos, float* tokens, int64_t B, int64_t n_patches, void* stream);
int cvae_layernorm256(const float* x, int64_t x_stride, const float* gamma, const float* beta, void* y, int64_t rows, float eps, int out_dtype, void* stream);
int cvae_token_gemm(const void* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, void* y, int64_t y_stride,
                    int64_t M, int64_t K, int64_t N, int epilogue, int dtype, void* stream);
int cvae_mhsa_fwd(const void* q, const void* k, const void* v, void* out, int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride,
                  int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype, void* stream);

/* ---- ViT-VAE encoder, training the transformer (csrc/vit.hip) ---------------------------------------------------------------------
 * The backward of the entries above, in both arithmetic modes, under the same contract: fp32 accumulation, no atomics, every cross-row or cross-workgroup
 * sum in a fixed order (slabs that depend on the row count only, then an ordered finish launch), bit-reproducible; every check precedes the first launch;
 * workspaces belong to the caller (*_workspace_bytes).  The residual-stream gradient is fp32 in both modes, cotangents of tensors the forward stores in
 * bf16 are bf16, every parameter gradient is fp32.
 *   cvae_mhsa_fwd_train         cvae_mhsa_fwd (the same `out`, bit for bit) that also leaves lse fp32 [B][8][n_query_rows]: log2 of the row's sum of
 *                               2^(score log2(e) / sqrt(32)), the one statistic the backward needs
 *   cvae_mhsa_bwd               dq [.][n_query_rows][256], dk / dv [.][n_tokens][256] (each with its own row and batch stride: the packed [B][N][768]
 *                               cotangent of the in-projection is written in place) from q, k, v, out, lse and dout [B][n_query_rows][256] (contiguous, as out).
 *                               Recompute-style: P = 2^(s - lse), delta = rowsum(dout * out) in fp32, dS = P (dP - delta) / sqrt(32); two launches (query
 *                               tiles walk the keys for dq and leave delta in the workspace; key tiles walk the queries for dk, dv).  bf16: P and dS are
 *                               rounded to bf16 for their MFMA products.
 *   cvae_token_gemm_gelu_train  cvae_token_gemm's GELU epilogue (the same y, bit for bit) that also stores the pre-activation x W^T + bias in `dtype`
 *   cvae_token_gemm_bwd_data    dx[M][K] = (g[M][N] W[N][K]) * gelu'(pre) + resid.  W is the fp32 nn.Linear tensor (or a row slice of it: N rows),
 *                               transposed and rounded on its way into LDS; g in g_dtype (fp32 g in bf16 mode: the stream gradient, rounded on its way
 *                               into LDS), dx in dx_dtype; pre (optional, `dtype`): exact-erf GELU derivative; resid (optional, fp32, needs fp32 dx; may be dx)
 *   cvae_token_gemm_wgrad       dW[N][K] = sum_m g[m][n] x[m][k], db[n] = sum_m g[m][n] (compensated), fp32, nn.Linear layout; slabs of 512 rows (M <= 65535 x 512)
 *   cvae_layernorm256_bwd       dx = rstd (gamma g - mean(gamma g) - xh mean(gamma g xh)) written or (accumulate != 0) added to dx (row stride dx_stride);
 *                               statistics recomputed two-pass from the saved fp32 input x (nothing but x is saved); dgamma = sum_rows g xh, dbeta = sum_rows g
 *                               over slabs of 32 rows, then in slab order
 *   cvae_vit_tokens_bwd         dpos[i] = sum_b dtokens[b][i], dcls = sum_b dtokens[b][0] (b in order), dstem[b][i] = dtokens[b][1 + i] in stem_dtype; with a gate
 *                               (optional: the stem output [B][n][256] in stem_dtype, a LeakyReLU output) dstem[b][i] = dtokens[b][1 + i] * act'(gate[b][i]),
 *                               act'(gate) = gate > 0 ? 1 : slope of gate_act, the product in fp32, then one rounding; gate NULL / CVAE_ACT_NONE: as without;
 *                               dpos and dcls are never gated */
int cvae_mhsa_fwd_train(const void* q, const void* k, const void* v, void* out, float* lse, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                        int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int dtype,
                        void* stream);
size_t cvae_mhsa_bwd_workspace_bytes(int64_t B, int64_t n_query_rows);
int cvae_mhsa_bwd(const void* q, const void* k, const void* v, const void* out, const float* lse, const void* dout, void* dq, void* dk, void* dv, int64_t q_stride,
                  int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t dq_stride, int64_t dk_stride,
                  int64_t dv_stride, int64_t dq_batch_stride, int64_t dk_batch_stride, int64_t dv_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows,
                  int dtype, void* workspace, size_t workspace_bytes, void* stream);
int cvae_token_gemm_gelu_train(const void* x, int64_t x_stride, const float* W, const float* bias, void* pre, int64_t pre_stride, void* y, int64_t y_stride, int64_t M,
                               int64_t K, int64_t N, int dtype, void* stream);
int cvae_token_gemm_bwd_data(const void* g, int64_t g_stride, int g_dtype, const float* W, const void* pre, int64_t pre_stride, const float* resid,
                             int64_t resid_stride, void* dx, int64_t dx_stride, int dx_dtype, int64_t M, int64_t K, int64_t N, int dtype, void* stream);
size_t cvae_token_gemm_wgrad_workspace_bytes(int64_t M, int64_t K, int64_t N);
int cvae_token_gemm_wgrad(const void* g, int64_t g_stride, int g_dtype, const void* x, int64_t x_stride, float* dW, float* db, int64_t M, int64_t K, int64_t N,
                          int dtype, void* workspace, size_t workspace_bytes, void* stream);
size_t cvae_layernorm256_bwd_workspace_bytes(int64_t rows);
int cvae_layernorm256_bwd(const void* g, int64_t g_stride, int g_dtype, const float* x, int64_t x_stride, const float* gamma, float* dx, int64_t dx_stride,
                          int accumulate, float* dgamma, float* dbeta, int64_t rows, float eps, void* workspace, size_t workspace_bytes, void* stream);
int cvae_vit_tokens_bwd(const float* dtokens, float* dpos, float* dcls, void* dstem, int stem_dtype, const void* gate, int gate_act, int64_t B, int64_t n_patches,
                        void* stream);

/* ---- ViT-VAE encoder, dropout when training the transformer (csrc/vit.hip) -------------------------------------------------------
 * The training entries above with a dropout mask that is never stored: every kernel recomputes it in registers from a counter-based generator, the forward
 * and the backward alike.  fp32 only: these entries take no dtype code (every tensor is fp32).  Otherwise the contract of their siblings: every check precedes
 * the first launch, the workspace is the caller's, no atomics, fixed-order sums, pointers and strides multiples of 16 bytes.
 *
 * THE MASK.  One Philox4x32-10 call (counter c0..c3, key k0 = low word of `key`, k1 = high word) yields four 32-bit words w[0..3].
 *   row site        an fp32 matrix [rows][N], N % 4 == 0.  Element (r, c): counter = (c >> 2, low 32 bits of R, high 32 bits of R, 0), word c & 3, where
 *                   R = mask_row0 + r * mask_row_step is the element's LOGICAL row (0 <= mask_row0 <= 2^40, 1 <= mask_row_step <= 2^30): the rows
 *                   0, n, 2 n, ... of a [B n][N] site are the [B][N] site with (mask_row0, mask_row_step) = (0, n).
 *   attention site  element (batch b, head h, query i, key j): counter = (j >> 2, i, b * 8 + h, 0), word j & 3.  i and j are token indices: they do not
 *                   depend on n_query_rows or on any tile size.
 *   keep rule       an element is kept iff (w >> 8) >= T, T = (uint32_t)((double)p * 16777216.0); kept values are multiplied by the fp32 constant
 *                   s = 1.0f / (1.0f - p), dropped ones are 0.  0 <= p < 1, anything else is CVAE_E_BADSHAPE.
 *   p = 0           T = 0, s = 1: nothing is dropped and every entry below produces the bits of its sibling without dropout.
 *
 *   cvae_mhsa_fwd_train_dropout       cvae_mhsa_fwd_train with Pd = softmax(S) keep s in place of P in the P V product.  Row max, row sum and lse are those of
 *                                     the undropped row (lse: cvae_mhsa_fwd_train's bits); s multiplies the output row once, next to 1 / (row sum).
 *   cvae_mhsa_bwd_dropout             cvae_mhsa_bwd for that forward (the same p and key): dV = Pd^T dO, dP = (dO V^T) keep s, dS = P (dP - delta) / sqrt(32)
 *                                     with delta = rowsum(dout * out) of the dropped out.  Workspace: cvae_mhsa_bwd_workspace_bytes.
 *   cvae_token_gemm_dropout           cvae_token_gemm on fp32 x with a row-site mask over (logical row, output column).  epilogue CVAE_GEMM_EPI_GELU: stores the
 *                                     pre-activation in `pre` (row stride pre_stride) and y = gelu(pre) keep s; CVAE_GEMM_EPI_RESIDUAL: y = resid +
 *                                     (x W^T + bias) keep s (y == resid allowed; pre is not read).  Any other epilogue is CVAE_E_BADSHAPE.
 *   cvae_token_gemm_bwd_data_dropout  dx[M][K] = (g[M][N] W[N][K]) keep s * gelu'(pre), the mask over (logical row, column of dx); pre optional
 *   cvae_dropout_rows                 y = x keep s on fp32 [M][N] with row strides (y == x allowed; N % 4 == 0, M and N at most 2^30); on an all-ones x it
 *                                     is the mask itself (times s) */
int cvae_mhsa_fwd_train_dropout(const float* q, const float* k, const float* v, float* out, float* lse, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, float p,
                                uint64_t key, void* stream);
int cvae_mhsa_bwd_dropout(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* dout, float* dq, float* dk, float* dv,
                          int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride,
                          int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int64_t dq_batch_stride, int64_t dk_batch_stride, int64_t dv_batch_stride,
                          int64_t B, int64_t n_tokens, int64_t n_query_rows, float p, uint64_t key, void* workspace, size_t workspace_bytes, void* stream);
int cvae_token_gemm_dropout(const float* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, float* pre,
                            int64_t pre_stride, float* y, int64_t y_stride, int64_t M, int64_t K, int64_t N, int epilogue, float p, uint64_t key, int64_t mask_row0,
                            int64_t mask_row_step, void* stream);
int cvae_token_gemm_bwd_data_dropout(const float* g, int64_t g_stride, const float* W, const float* pre, int64_t pre_stride, float* dx, int64_t dx_stride, int64_t M,
                                     int64_t K, int64_t N, float p, uint64_t key, int64_t mask_row0, int64_t mask_row_step, void* stream);
int cvae_dropout_rows(const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t M, int64_t N, float p, uint64_t key, int64_t mask_row0,
                      int64_t mask_row_step, void* stream);

/* ---- device-resident dropout keys (csrc/vit.hip) -----------------------------------------------------------------------------------
 * What a captured training step needs: keys that are not launch arguments.  A graph bakes every by-value argument in, so the five entries above would
 * replay one mask for ever; the forms below read the key from device memory when the kernel runs, and one more entry derives a step's keys on the device.
 *
 * THE KEY OF A SITE (normative; the host's ops.DropoutKeys.key computes the same integers).  With splitmix64(z): z += 0x9E3779B97F4A7C15;
 * z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB; return z ^ (z >> 31), all mod 2^64:
 *   key(seed, step, block, site) = splitmix64(splitmix64(seed) + (step << 20 | block << 4 | site)),   step < 2^44, block < 2^16, site < 16.
 *
 *   cvae_dropout_keys_step   base = splitmix64(seed), computed by the caller.  One workgroup reads s = *step mod 2^44, writes
 *                            table[4 b + site] = splitmix64(base + (s << 20 | b << 4 | site)) for b < n_blocks, site < 4, and — after a workgroup barrier
 *                            that follows every thread's read — stores s + 1 to *step.  1 <= n_blocks <= 65536, else CVAE_E_BADSHAPE; step and table are
 *                            8-byte-aligned device pointers (null: CVAE_E_NULLPTR), table holds 4 n_blocks words.
 *   cvae_*_devkey            the five entries above with `uint64_t key` replaced by `const uint64_t* key`: an 8-byte-aligned device pointer to the key
 *                            (null: CVAE_E_NULLPTR; misaligned: CVAE_E_UNSUPPORTED), read by the kernel when it runs — low word k0, high word k1.  Every
 *                            other argument, check and output bit is the sibling's: the same key gives the same bits through either form. */
int cvae_dropout_keys_step(uint64_t base, int64_t* step, uint64_t* table, int n_blocks, void* stream);
int cvae_mhsa_fwd_train_dropout_devkey(const float* q, const float* k, const float* v, float* out, float* lse, int64_t q_stride, int64_t k_stride, int64_t v_stride,
                                       int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows,
                                       float p, const uint64_t* key, void* stream);
int cvae_mhsa_bwd_dropout_devkey(const float* q, const float* k, const float* v, const float* out, const float* lse, const float* dout, float* dq, float* dk, float* dv,
                                 int64_t q_stride, int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride,
                                 int64_t dq_stride, int64_t dk_stride, int64_t dv_stride, int64_t dq_batch_stride, int64_t dk_batch_stride, int64_t dv_batch_stride,
                                 int64_t B, int64_t n_tokens, int64_t n_query_rows, float p, const uint64_t* key, void* workspace, size_t workspace_bytes,
                                 void* stream);
int cvae_token_gemm_dropout_devkey(const float* x, int64_t x_stride, const float* W, const float* bias, const float* resid, int64_t resid_stride, float* pre,
                                   int64_t pre_stride, float* y, int64_t y_stride, int64_t M, int64_t K, int64_t N, int epilogue, float p, const uint64_t* key,
                                   int64_t mask_row0, int64_t mask_row_step, void* stream);
int cvae_token_gemm_bwd_data_dropout_devkey(const float* g, int64_t g_stride, const float* W, const float* pre, int64_t pre_stride, float* dx, int64_t dx_stride,
                                            int64_t M, int64_t K, int64_t N, float p, const uint64_t* key, int64_t mask_row0, int64_t mask_row_step, void* stream);
int cvae_dropout_rows_devkey(const float* x, int64_t x_stride, float* y, int64_t y_stride, int64_t M, int64_t N, float p, const uint64_t* key, int64_t mask_row0,
                             int64_t mask_row_step, void* stream);

/* ---- ViT-VAE encoder, attention weights and attention rollout (csrc/vit.hip) ----------------------------------------------------
 * What nn.MultiheadAttention returns next to its output and vit_backbone.py:43 drops: the attention probabilities, which cvae_mhsa_fwd never writes.
 * Both entries recompute them from q, k and the row statistic lse that cvae_mhsa_fwd_train leaves (fp32 [B][8][n_query_rows], log2 of the row sum):
 *   P[b][h][i][j] = 2^(s - lse[b][h][i]),  s = (q_i . k_j) log2(e) / sqrt(32)  over head h's 32 columns — the expression cvae_mhsa_bwd uses; no max or sum pass.
 * q / k follow cvae_mhsa_fwd: views into the packed in-projection output, row and batch strides in elements, head h in columns 32 h .. 32 h + 31, the
 * queries are the FIRST n_query_rows tokens; dtype CVAE_F32 (v_mfma_f32_32x32x2_f32) or CVAE_BF16 (bf16 MFMA); everything after the product is fp32.
 * Contract: enqueue-only; every check precedes the launch; B == 0 is CVAE_OK (nothing is launched); no atomics; every sum in an order that depends on
 * n_tokens and n_query_rows only (not on B, not on the run): bit-reproducible, and a batch row's bits do not depend on the other rows of the launch.
 * q, k 16-byte aligned with strides multiples of 16 bytes (else CVAE_E_UNSUPPORTED), strides at least 256 and batch strides non-negative (else
 * CVAE_E_BADSHAPE), 1 <= n_query_rows <= n_tokens <= 2^24, B <= 65535.
 *   cvae_mhsa_weights       average_heads = 0: w fp32 [B][8][n_query_rows][n_tokens] = P.  average_heads != 0: w fp32 [B][n_query_rows][n_tokens] =
 *                           ((((P_0 + P_1) + P_2) + ... ) + P_7) * 0.125f, plain fp32 adds in head order: what nn.MultiheadAttention(need_weights=True)
 *                           returns in eval mode.  Rows of w are DENSE: n_tokens floats, no padding, so a row start is in general not 16-byte aligned
 *                           (n_tokens = 961, 7, 65) and the kernel stores 4-byte elements.  Only the base of w (16-byte aligned, else CVAE_E_UNSUPPORTED)
 *                           and w_batch_stride (in floats, at least one batch's extent, else CVAE_E_BADSHAPE) are constrained.
 *   cvae_mhsa_rollout_step  one factor of attention rollout (Abnar & Zuidema 2020) applied to a row vector, the N x N matrix never formed:
 *                             out[b][j] = residual r[b][j] + (1 - residual) 0.125 sum_{h < 8} sum_{i < n_query_rows} r[b][i] P[b][h][i][j]
 *                           r, out fp32 [B][n_tokens], contiguous.  The double sum is one fp32 chain per key and lane half in the order (64-query tile,
 *                           head, query), the two halves (queries 8 g + 0..3 and 8 g + 4..7 of every 32) added at the end.  0 <= residual <= 1, else
 *                           CVAE_E_BADSHAPE; residual = 1 returns r.  out == r (any overlap) is refused: CVAE_E_UNSUPPORTED.  n_query_rows < n_tokens
 *                           serves the CLS-only last block: only the first rows of the matrix exist; the residual term still covers all n_tokens. */
int cvae_mhsa_weights(const void* q, const void* k, const float* lse, float* w, int64_t q_stride, int64_t k_stride, int64_t q_batch_stride,
                      int64_t k_batch_stride, int64_t w_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, int average_heads, int dtype,
                      void* stream);
int cvae_mhsa_rollout_step(const void* q, const void* k, const float* lse, const float* r, float* out, int64_t q_stride, int64_t k_stride,
                           int64_t q_batch_stride, int64_t k_batch_stride, int64_t B, int64_t n_tokens, int64_t n_query_rows, float residual, int dtype,
                           void* stream);

/* ---- ViT-VAE encoder, attention gradients and gradient-weighted attention relevance (csrc/vit_attention_grad_probe.inc) ------------
 * The counterpart of the two entries above on the backward's side: the gradient of a target with respect to the attention probabilities, which never exist in
 * memory, and one step of the relevance rule of Chefer, Gur & Wolf (ICCV 2021, "Generic Attention-model Explainability ...", self-attention).  Per block, for
 * batch row b and head h of 8 (head h reads feature columns 32 h .. 32 h + 31):
 *   P[b][h][i][j]  = 2^(q_i . k_j  log2(e) / sqrt(32) - lse[b][h][i])      as above: recomputed, never stored
 *   dO             = the cotangent of the attention output [B][n_query_rows][256] (before out_proj), in the compute dtype
 *   gA[b][h][i][j] = sum_{d < 32} dO[b][i][32 h + d] V[b][j][32 h + d]      the gradient with respect to the probabilities taken as a free variable (out = A V):
 *                                                                          what a hook on the softmax output receives; it needs neither q, k nor lse
 *   Abar[b][i][j]  = 0.125 ((((t_0 + t_1) + t_2) + ...) + t_7),  t_h = max(0, gA[b][h][i][j] P[b][h][i][j])       heads summed in order 0..7, plain fp32 adds
 *   relevance:       R = I, then R <- R + Abar_l R for l = first .. last block; the map is R's CLS row.  As a row vector: r = e_cls, then for l = last .. first
 *                    r <- r + r Abar_l — the left-multiplication of the rollout, so no N x N object is formed.  In the last block only the CLS output reaches a
 *                    target, so only row 0 of its Abar is non-zero (exactly): that step runs with n_query_rows = 1 on the CLS-only record.
 * dout is dense [B][n_query_rows][256] as cvae_mhsa_bwd takes it; q, k, v are views as cvae_mhsa_fwd takes them (row and batch strides in elements); dtype
 * CVAE_F32 (v_mfma_f32_32x32x2_f32) or CVAE_BF16 (bf16 MFMA) for q, k, v and dout alike; everything after the two products is fp32.
 * Contract, as above: enqueue-only; every check precedes the first launch; B == 0 is CVAE_OK (nothing is launched); no atomics and no "last workgroup"
 * ticket; every sum in an order that depends on n_tokens and n_query_rows only, so a batch row's bits do not depend on B or on the run, and
 * n_query_rows = 1 gives the bits that row 0 contributes in a full call.  1 <= n_query_rows <= n_tokens <= 2^24, 0 <= B <= 65535, strides at least 256 and
 * batch strides non-negative (else CVAE_E_BADSHAPE); an unknown dtype code: CVAE_E_DTYPE; a null pointer: CVAE_E_NULLPTR; q, k, v, dout not 16-byte aligned
 * or a stride not a multiple of 16 bytes, lse / r / out / workspace not 4-byte aligned: CVAE_E_UNSUPPORTED.
 *   cvae_mhsa_weight_grads    w fp32 [B][8][n_query_rows][n_tokens] = gA.  Rows of w are dense (n_tokens floats), stored 4 bytes at a time; only w's base
 *                             (16-byte aligned, else CVAE_E_UNSUPPORTED) and w_batch_stride (in floats, at least 8 n_query_rows n_tokens, else
 *                             CVAE_E_BADSHAPE) are constrained.  One launch, grid (ceil(n_tokens / 128), 8, B).
 *   cvae_mhsa_relevance_step  out[b][j] = r[b][j] + sum_{i < n_query_rows} r[b][i] Abar[b][i][j];  r, out fp32 [B][n_tokens], contiguous; out == r (any overlap)
 *                             is refused: CVAE_E_UNSUPPORTED.  The query rows are split into S = ceil(n_query_rows / 64) chunks (a function of n_query_rows
 *                             alone), one workgroup per (128 keys, chunk, batch row).  Within a chunk the sum is one fp32 chain per key and lane half,
 *                             col += r[i] * (Abar[i][j]) in query order (queries 8 g + 0..3 and 8 g + 4..7 of every 32), the halves added once.  S > 1: the
 *                             chunk sums go to `workspace` as fp32 [B][S][n_tokens] (cvae_mhsa_relevance_step_workspace_bytes; CVAE_E_WORKSPACE below
 *                             it, CVAE_E_NULLPTR without one) and a second small launch computes out = r + (((c_0 + c_1) + ...) + c_{S-1}).  S == 1 (at most
 *                             64 query rows: the CLS-only last block): one launch writes out = r + c_0 itself, no workspace is read (0 bytes asked).
 *                             S > 65535: CVAE_E_UNSUPPORTED.  dout == 0 returns r bit for bit. */
int cvae_mhsa_weight_grads(const void* dout, const void* v, float* w, int64_t v_stride, int64_t v_batch_stride, int64_t w_batch_stride, int64_t B,
                           int64_t n_tokens, int64_t n_query_rows, int dtype, void* stream);
size_t cvae_mhsa_relevance_step_workspace_bytes(int64_t B, int64_t n_tokens, int64_t n_query_rows);
int cvae_mhsa_relevance_step(const void* q, const void* k, const void* v, const float* lse, const void* dout, const float* r, float* out, int64_t q_stride,
                             int64_t k_stride, int64_t v_stride, int64_t q_batch_stride, int64_t k_batch_stride, int64_t v_batch_stride, int64_t B,
                             int64_t n_tokens, int64_t n_query_rows, int dtype, void* workspace, size_t workspace_bytes, void* stream);

/* ---- ViT-VAE encoder, Grad-CAM on the stem output (csrc/vit_gradcam.inc) ---------------------------------------------------------
 * The arithmetic of the reference's GradCAM.__call__ (mnist_test/02_mechanism_analysis/analyze_gradcam.py:56-73) without its resize, on the channels-last stem
 * output A and its gradient dA, both [B][n][256] contiguous in `dtype` (CVAE_F32 or CVAE_BF16); cam fp32 [B][n]:
 *   w[b][c]   = (((dA[b][0][c] + dA[b][1][c]) + ...) + dA[b][n-1][c]) * (1.0f / n)          one fp32 chain per channel, rows in index order
 *   m[b][i]   = max(0, sum_c w[b][c] A[b][i][c])        per 4 consecutive channels an fma chain started at 0 (64 of them per row), then the xor-shuffle sum
 *                                                       of the 64 partials (lane offsets 32, 16, 8, 4, 2, 1)
 *   cam[b][i] = normalize != 0 ? (m[b][i] - min_i m[b]) / (max_i m[b] - min_i m[b] + 1e-8f) : m[b][i]
 * One launch, one workgroup per image, no workspace, no atomics; an image's bits do not depend on B or on the run.  1 <= n <= 4096 (the map of an image lives in
 * LDS; the encoder has n <= 961), else CVAE_E_BADSHAPE (n < 1, B < 0) / CVAE_E_UNSUPPORTED (n > 4096); a dtype code other than the two: CVAE_E_DTYPE; then
 * B == 0 is CVAE_OK; a null pointer: CVAE_E_NULLPTR; A or dA not 16-byte aligned, cam not 4-byte aligned or cam overlapping an input: CVAE_E_UNSUPPORTED. */
int cvae_gradcam256(const void* A, const void* dA, float* cam, int64_t B, int64_t n, int normalize, int dtype, void* stream);

/* ---- ViT-VAE decoder, eval mode (csrc/conv_s1.hip; vessel_analysis/00_core/vit_backbone.py:7-19, 115-156, 186-193) -------------------------------------
 * Stride-1 window convolutions on channels-last [B][H][W][C] tensors, dtype CVAE_F32 (exact fp32 MFMA) or CVAE_BF16; fp32 accumulation in a fixed order
 * (no atomics, no split-K): bit-reproducible, and a sample's bits do not depend on the batch it travels in.  Pointers 16-byte aligned, else CVAE_E_UNSUPPORTED;
 * channel counts outside the lists are CVAE_E_UNSUPPORTED; B == 0 is CVAE_OK (nothing is launched).
 *   cvae_conv_s1         y = act(conv(x, w) + bias + resid), everything after the products in fp32 before the one rounding to `dtype`.
 *                        form CVAE_CONV_S1_K3:       nn.Conv2d(C, C, 3, 1, 1), Cin == Cout in {32, 64, 128}; x, y, resid [B][H][W][C];
 *                        form CVAE_CONV_S1_SUBPIXEL: nn.ConvTranspose2d(Cin, 16, 3, 2, 1, output_padding 1), Cin in {32, 16}, as a 2 x 2 forward-window conv
 *                                                    to 64 channels with a pixel-shuffle store; x [B][H][W][Cin], y and resid [B][2H][2W][16].
 *                        w: the GEMM matrix in `dtype` (cvae_conv_s1_weight_elems elements; fp32: what cvae_fold_bn_conv's kinds CVAE_FOLD_CONV_K3S1 /
 *                        CVAE_FOLD_CONVT_K3S2_SUBPIXEL write; bf16: that, through cvae_conv_s1_pack_weights); bias fp32 [Cout] (required); resid optional (NULL);
 *                        act CVAE_ACT_NONE / RELU / LEAKY02 / LEAKY001.
 *   cvae_conv_s1_weight_elems   elements of that matrix, 0 for an unsupported (Cin, Cout, form)
 *   cvae_conv_s1_pack_weights   fp32 -> bf16 for `count` (1..16) matrices of n[i] elements (n[i] % 4 == 0) in ONE launch (host arrays of device pointers)
 *   cvae_conv_s1_c1      nn.Conv2d(16, 1, 3, 1, 1): x [B][H][W][16] in `dtype`, w the fp32 weight [1][16][3][3] as it is (rounded to bf16 on its way into LDS
 *                        in bf16 mode), bias fp32 [1] or NULL; y fp32 [B][1][H][W] = act(conv + bias).  Cin != 16: CVAE_E_UNSUPPORTED.
 *   cvae_latent_to_grid  out[b][p][c] = sum_k W[c P + p][k] z[b][k] + bias[c P + p]: nn.Linear(K, C P) followed by view(B, C, gh, gw), written channels-last
 *                        [B][P][C] in `dtype`.  z fp32 [B][K], W / bias the fp32 nn.Linear tensors, read once per launch with 16-byte loads and never cast;
 *                        products and sums fp32.  B <= 16 per launch (the caller chunks larger batches), K <= 512 and K % 4 == 0, C % 32 == 0, else
 *                        CVAE_E_UNSUPPORTED. */
#define CVAE_CONV_S1_K3       0
#define CVAE_CONV_S1_SUBPIXEL 1
#define CVAE_CONV_S1_SUBPIXEL_T 2   /* cvae_conv_s1_bwd_data only */
int64_t cvae_conv_s1_weight_elems(int64_t Cin, int64_t Cout, int form);
int cvae_conv_s1_pack_weights(int count, const float* const* w, void* const* packed, const int64_t* n, void* stream);
int cvae_conv_s1(const void* x, const void* w, const float* bias, const void* resid, void* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int64_t Cout,
                 int form, int dtype, int act, void* stream);
int cvae_conv_s1_c1(const void* x, const float* w, const float* bias, float* y, int64_t B, int64_t H, int64_t W, int64_t Cin, int dtype, int act, void* stream);
int cvae_latent_to_grid(const float* z, const float* W, const float* bias, void* out, int64_t B, int64_t K, int64_t P, int64_t C, int dtype, void* stream);
/* The decoder's input-gradient path (frozen weights, eval-mode BatchNorm; the same tiling, fixed summation order and batch-independent bits as the forward):
 *   cvae_conv_s1_bwd_data     dx = (conv(g, w^T) + resid) * act'(gate), epilogue in fp32 before the one rounding; resid and gate optional (NULL), both of dx's
 *                             shape and dtype; act'(gate) = gate > 0 ? 1 : slope of gate_act (CVAE_ACT_NONE / RELU / LEAKY02 / LEAKY001), read off the
 *                             activation's OUTPUT.  dx [B][H][W][C].
 *                             form CVAE_CONV_S1_K3:         input gradient of nn.Conv2d(C, C, 3, 1, 1), C in {32, 64, 128}; g [B][H][W][C];
 *                             form CVAE_CONV_S1_SUBPIXEL_T: input gradient of nn.ConvTranspose2d(C, 16, 3, 2, 1, output_padding 1), C in {32, 16}; g [B][2H][2W][16].
 *                             w: the backward matrix of cvae_fold_bn_conv's kinds CVAE_FOLD_*_GRAD in `dtype` (cvae_conv_s1_weight_elems(C, C, K3) resp.
 *                             cvae_conv_s1_weight_elems(C, 16, SUBPIXEL_T) = 32 x 256 elements).
 *   cvae_conv_s1_c1_bwd_data  input gradient of nn.Conv2d(16, 1, 3, 1, 1): g fp32 [B][1][H][W], w the fp32 weight [1][16][3][3] (rounded to bf16 in bf16 mode, as
 *                             the forward reads it), dx [B][H][W][16] in `dtype` = conv^T(g) * act'(gate), gate optional, of dx's shape and dtype.
 *   cvae_latent_to_grid_bwd   dz[b][k] = sum_{p, c} g[b][p][c] W[c P + p][k], fp32: g [B][P][C] in `dtype`, W the fp32 nn.Linear tensor, read ONCE per launch
 *                             with 16-byte loads for B <= 16 rows.  Slabs of 256 rows of W per workgroup (a split that depends on C and P only), per-slab partial
 *                             sums in `workspace` (cvae_latent_to_grid_bwd_workspace_bytes; CVAE_E_WORKSPACE below it), added in slab order by a second launch:
 *                             no float atomics, and a row's bits do not depend on B.  Limits as cvae_latent_to_grid. */
int cvae_conv_s1_bwd_data(const void* g, const void* w, const void* resid, const void* gate, void* dx, int64_t B, int64_t H, int64_t W, int64_t C, int form,
                          int dtype, int gate_act, void* stream);
int cvae_conv_s1_c1_bwd_data(const float* g, const float* w, const void* gate, void* dx, int64_t B, int64_t H, int64_t W, int64_t Cin, int dtype, int gate_act,
                             void* stream);
size_t cvae_latent_to_grid_bwd_workspace_bytes(int64_t B, int64_t K, int64_t P, int64_t C);
int cvae_latent_to_grid_bwd(const void* g, const float* W, float* dz, int64_t B, int64_t K, int64_t P, int64_t C, int dtype, void* workspace, size_t workspace_bytes,
                            void* stream);
/* The decoder's weight-gradient path (eval-mode BatchNorm: running statistics, not updated).  Activations and cotangents in `dtype`, every gradient fp32;
 * fp32 sums in a fixed order, no float atomics: two runs give the same bits.  B >= 1; all checks come before the first launch.
 *   cvae_conv_s1_wgrad        dW and dbias = sum g of the layer's FOLDED weight, in the torch layout, from the layer's input x [B][H][W][C] and the gated
 *                             cotangent g of its pre-activation.  A GEMM over the B H W pixels on the MFMA: 8 x 16 pixel tiles with the halo staged once,
 *                             a workgroup walks tiles s, s + slabs, .. and leaves its partial sums in slab s of `workspace`
 *                             (cvae_conv_s1_wgrad_workspace_bytes; CVAE_E_WORKSPACE below it); a second launch adds the slabs in slab order.
 *                             form CVAE_CONV_S1_K3:       nn.Conv2d(C, C, 3, 1, 1), C in {16, 32, 64, 128}; g [B][H][W][C]; dW [C][C][3][3], dbias [C];
 *                             form CVAE_CONV_S1_SUBPIXEL: nn.ConvTranspose2d(C, 16, 3, 2, 1, output_padding 1), C in {32, 16}; g [B][2H][2W][16], read in the
 *                                                         forward's sub-pixel form; dW [C][16][3][3] (the 9 real taps per (ci, co)), dbias [16].
 *   cvae_conv_s1_c1_wgrad     nn.Conv2d(16, 1, 3, 1, 1): x [B][H][W][16] in `dtype`, g fp32 [B][1][H][W]; dW [1][16][3][3], dbias [1]; per-workgroup partial
 *                             sums in `workspace` (cvae_conv_s1_c1_wgrad_workspace_bytes), added in workgroup order by a second launch.
 *   cvae_latent_to_grid_wgrad dW[c P + p][k] = sum_b g[b][p][c] z[b][k] (rows b in order), dbias[c P + p] = sum_b g[b][p][c]: g [B][P][C] in `dtype`, z fp32
 *                             [B][K]; dW [C P][K] written once with 16-byte stores; any B >= 1, K <= 512 and K % 4 == 0, C % 32 == 0. */
size_t cvae_conv_s1_wgrad_workspace_bytes(int64_t B, int64_t H, int64_t W, int64_t C, int form);
int cvae_conv_s1_wgrad(const void* x, const void* g, float* dW, float* dbias, int64_t B, int64_t H, int64_t W, int64_t C, int form, int dtype, void* workspace,
                       size_t workspace_bytes, void* stream);
size_t cvae_conv_s1_c1_wgrad_workspace_bytes(int64_t B, int64_t H, int64_t W);
int cvae_conv_s1_c1_wgrad(const void* x, const float* g, float* dW, float* dbias, int64_t B, int64_t H, int64_t W, int64_t Cin, int dtype, void* workspace,
                          size_t workspace_bytes, void* stream);
int cvae_latent_to_grid_wgrad(const void* g, const float* z, float* dW, float* dbias, int64_t B, int64_t K, int64_t P, int64_t C, int dtype, void* stream);

/* ---- The dense heads of CausalViTVAE, eval mode (csrc/heads.hip; vessel_analysis/00_core/models.py:225-250, 281-302) ------------------------------------------
 * One launch = one whole head: the logical concatenation of n_panels (1..3) fp32 row panels {ptr, width, row stride in elements} (torch.cat(dim=1), never
 * materialised) through n_layers (1..3) fp32 nn.Linear layers (W [out][in], b [out] as they are; hidden rows stay in LDS), then per layer and in this order:
 *   eval-mode BatchNorm1d  when bn_var != NULL: y = (v - bn_mean) * (bn_weight / sqrt(bn_var + bn_eps)) + bn_bias, computed from the LIVE tensors on every
 *                          call (nothing is cached across calls: parameters may be rewritten through raw pointers);
 *   LeakyReLU(slope)       when leaky != 0.
 * The LAST layer may be held by two weight tensors: rows 0 .. out_first - 1 in (W, b), rows out_first .. out - 1 in (W2 [out - out_first][in], b2)
 * (morph_predictor_mu / morph_predictor_logvar: no stacked copy); other layers have out_first == out.  Epilogue: output columns 0 .. split - 1 go to out0
 * [B][split], columns split .. out - 1 to out1 [B][out - split] (split == out: out1 unused); clamp0 / clamp1: NULL, or HOST {lo, hi} of torch.clamp for that
 * panel; z (optional, needs out == 2 split and eps [B][split]): z = out0 + eps * exp(0.5 * out1) from the clamped values.  All strides in elements.
 * fp32 throughout; every output value is one fmaf chain over the inputs in index order (no atomics, no split sums): a row's bits do not depend on B nor on the
 * row's position in the batch.  Limits: the concatenated input width and every layer's `out` at most CVAE_HEADS_MAX_WIDTH, else CVAE_E_UNSUPPORTED (the heads
 * served: 287 -> 512 -> 256, 140 -> 256 -> 512, 19 -> 64 -> 64 -> 12 + 12).  B == 0 is CVAE_OK (nothing is launched).  Shape and limit errors are reported
 * before that return, NULL pointers after it; the training entries below are checked by the same code. */
#define CVAE_HEADS_MAX_PANELS 3
#define CVAE_HEADS_MAX_LAYERS 3
#define CVAE_HEADS_MAX_WIDTH  512
typedef struct { const float* ptr; int64_t width, stride; } cvae_heads_panel;
typedef struct {
    const float *W, *b, *W2, *b2;
    int64_t out, out_first;
    const float *bn_weight, *bn_bias, *bn_mean, *bn_var;
    float bn_eps;
    int leaky;
    float slope;
} cvae_heads_layer;
int cvae_mlp_heads_fwd(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t split,
                       const float* clamp0, const float* clamp1, const float* eps, int64_t eps_stride, float* out0, int64_t out0_stride,
                       float* out1, int64_t out1_stride, float* z, int64_t z_stride, int64_t B, void* stream);

/* ---- The same heads in TRAINING mode, and their backward (csrc/heads.hip) ---------------------------------------------------------------
 * cvae_mlp_heads_train_fwd: cvae_mlp_heads_fwd's arguments, limits and checks (the same code) with training-mode semantics.  A hidden layer is a BatchNorm1d layer when its
 * bn_weight != NULL (bn_bias required; the layer's bn_mean / bn_var are NOT read): it normalises with the statistics of the B rows of this call, mean first,
 * then sum (v - mean)^2 (two passes, one thread per column walking the rows in order), the biased variance, rstd = 1 / sqrt(var + bn_eps), and updates
 * bn[l] as torch does: running = (1 - momentum) running + momentum batch with the UNBIASED variance, *num_batches_tracked += 1 (each of the three pointers
 * may be NULL: not tracked).  B < 2 with a BatchNorm layer is CVAE_E_BADSHAPE.  The last layer is a plain Linear (BatchNorm or LeakyReLU there:
 * CVAE_E_UNSUPPORTED).  `bn` [n_layers] is read for BatchNorm layers only and may be NULL without one.
 * `saved` (cvae_mlp_heads_train_workspace_bytes; below it CVAE_E_WORKSPACE) receives what the backward reads, fp32, in this order: for every hidden layer l
 * of width N_l: { mean [N_l], rstd [N_l], the normalised pre-activation x^ [B][N_l] } when it is a BatchNorm layer, then the pre-LeakyReLU value [B][N_l]
 * (gamma x^ + beta, or the Linear output), then the activation [B][N_l]; after the hidden layers the PRE-CLAMP last-layer output [B][out].
 * One launch per stretch of layers between BatchNorm layers plus one statistics launch per BatchNorm layer (an adapter: 3, the morph predictor: 1).
 *
 * cvae_mlp_heads_bwd: cotangents g0 [B][split], g1 [B][out - split], gz [B][split] of the first result, the second result and z (each may be NULL = zero;
 * gz needs eps and out == 2 split) -> grads[l] for every layer (dW, db as the weights are laid out; dW2, db2 for the last layer's second tensor; dgamma,
 * dbeta for a BatchNorm layer: all required) and, for every panel p with panel_grads[p] != NULL, the input gradient [B][width_p] at row stride
 * panel_grad_strides[p] (panel_grads NULL: none).  Chain: g_mu += g_z, g_lv += g_z eps 0.5 exp(lv / 2) from the clamped lv; the clamp passes where
 * lo <= pre-clamp <= hi; Linear dW = g^T a, db = sum_rows g, da = g W; LeakyReLU y > 0 ? 1 : slope from the saved activation (exact zero: slope);
 * BatchNorm dbeta = sum dy, dgamma = sum dy x^, dv = gamma rstd (dy - dbeta / B - x^ dgamma / B).  Every cross-row sum is ONE chain over rows 0 .. B-1 in one
 * thread (dW: fmaf): no atomics, two runs give identical bits.  `saved` as the forward wrote it; `workspace` (cvae_mlp_heads_bwd_workspace_bytes) holds
 * the per-layer output gradients.  Launches: an adapter 3, the morph predictor 2.  Rows >= B are never read or written.  Both workspace queries return 0
 * for a head the entries refuse. */
typedef struct { float *running_mean, *running_var; int64_t* num_batches_tracked; float momentum; } cvae_heads_bn_train;
typedef struct { float *dW, *db, *dW2, *db2, *dgamma, *dbeta; } cvae_heads_layer_grad;
size_t cvae_mlp_heads_train_workspace_bytes(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t B);
size_t cvae_mlp_heads_bwd_workspace_bytes(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, int64_t B);
int cvae_mlp_heads_train_fwd(const cvae_heads_panel* panels, int n_panels, const cvae_heads_layer* layers, int n_layers, const cvae_heads_bn_train* bn,
                             int64_t split, const float* clamp0, const float* clamp1, const float* eps, int64_t eps_stride, float* out0,
                             int64_t out0_stride, float* out1, int64_t out1_stride, float* z, int64_t z_stride, int64_t B, void* saved,
                             size_t saved_bytes, void* stream);
int cvae_mlp_heads_bwd(const cvae_heads_panel* panels, int n_panels, float* const* panel_grads, const int64_t* panel_grad_strides,
                       const cvae_heads_layer* layers, int n_layers, const cvae_heads_layer_grad* grads, int64_t split, const float* clamp0,
                       const float* clamp1, const float* eps, int64_t eps_stride, const float* g0, int64_t g0_stride, const float* g1,
                       int64_t g1_stride, const float* gz, int64_t gz_stride, int64_t B, const void* saved, size_t saved_bytes, void* workspace,
                       size_t workspace_bytes, void* stream);

/* ---- The dense bottleneck of CausalBioVAE in 5 + 5 launches (batch M <= 16, fp32 arithmetic) --------------------------------
 * Replaces, between the last encoder conv and the first decoder conv (causal_cascade/models.py:57-79):
 *   AdaptiveAvgPool + Flatten, cat([x_feat, m, t]), enc_fc (Linear-ReLU-Linear-ReLU), fc_mu, fc_logvar, reparameterize,
 *   mechanism_net (Linear, BatchNorm1d, ReLU, Linear, ReLU, Linear), cat([z, m_hat]), dec_input (+ the NC(D)HW -> channels-last
 *   move into the decoder).  All pointers are device pointers; weights are the nn.Linear / BatchNorm1d tensors as they are.
 * y_cl: last encoder activation [M][D][H][W][C] (conv dtype), pooled to OD x OH x OW windows (D % OD == 0 etc.).
 * N1 / N2: widths of enc_fc.0 / enc_fc.2; Z: latent; HM: mechanism_net width; K1 = C*OD*OH*OW + m_dim + t_dim; K4 = Z + m_dim.
 * Accepted: 1 <= M <= 16, C % 64 == 0, non-overlapping windows, 4 <= N1 <= 4096, N2 <= 2048, Z + m_dim <= 128, HM <= 1024, t_dim <= 65536, and
 * every level launch's LDS within a workgroup's 160 KiB — about 4 M N1, 4 M (t_dim + 2 HM) and 4 M (Z + 2 m_dim + 5 HM + t_dim) bytes (so N1 = 4096
 * needs M <= 10, HM = 1024 M <= 7).  Anything else is CVAE_E_BADSHAPE from every entry, before any launch. */
typedef struct { int64_t M, D, H, W, C, OD, OH, OW, m_dim, t_dim, N1, N2, Z, HM; } cvae_bottleneck_dims;
typedef struct {                 /* parameters (fp32, torch layouts [out][in]) */
    const float *W1, *b1, *W2, *b2, *Wmu, *bmu, *Wlv, *blv, *Wm0, *bm0, *gamma, *beta, *Wm3, *bm3, *Wm5, *bm5, *Wd, *bd;
} cvae_bottleneck_params;
typedef struct {                 /* their gradients (overwritten), same order and shapes */
    float *dW1, *db1, *dW2, *db2, *dWmu, *dbmu, *dWlv, *dblv, *dWm0, *dbm0, *dgamma, *dbeta, *dWm3, *dbm3, *dWm5, *dbm5, *dWd, *dbd;
} cvae_bottleneck_grads;
typedef struct {                 /* activations kept for backward, all [M][dim] fp32: h1 [N1], h2 [N2], mu / logvar [Z],
                                    xhat / a1n / a2 [HM], invstd [HM] (one row), m_hat [m_dim], zm [K4] = cat(z, m_hat) */
    float *h1, *h2, *mu, *logvar, *xhat, *invstd, *a1n, *a2, *m_hat, *zm;
} cvae_bottleneck_saved;
/* Scratch sizes (in floats) for the given dims: xcat needs M*K1; the three partial buffers as returned. */
int cvae_bottleneck_sizes(const cvae_bottleneck_dims* dims, int64_t* K1, int64_t* K4, int64_t* fwd_partial_floats, int64_t* dzm_partial_floats,
                          int64_t* dx_partial_floats);
/* Forward.  t_onehot [M][t_dim] (F.one_hot(t).float(): an INPUT when t_labels is NULL; with t_labels [M] (int64 class indices) the call
 * writes it itself, saving the caller's one-hot launch), eps [M][Z] (the reparameterisation noise).  bn_training: batch statistics + running-stat /
 * num_batches_tracked update (running_* may be NULL), else running statistics.  Outputs: saved->mu / logvar / m_hat (the
 * model's outputs) and dec_cl [M][OD][OH][OW][C] (conv dtype) = dec_input(cat(z, m_hat)) viewed [M, C, 4..] channels-last.
 * dzm_acc: scratch of dzm_partial_floats (cvae_bottleneck_sizes) the BACKWARD fills with per-workgroup partials of d(zm) (one slot per
 * workgroup, plain stores, summed in index order: no float atomics); the forward does not touch it (kept in the signature so one
 * buffer can serve the pair).  bn_rank_stats (optional): mechanism_net's BatchNorm1d over the global batch of bn_ranks ranks (SyncBatchNorm, below).
 * noise (optional): the reparameterisation noise drawn by the first launch: eps [M][Z] becomes an OUTPUT holding exactly the numbers
 * cvae_philox_normal_advance(eps, M * Z, seed, 0, subsequence, call_counter) would have written, and *call_counter is incremented the same way (one
 * launch fewer per step; the reference draws torch.randn_like in reparameterize, causal_cascade/models.py:65-68). */
typedef struct { uint64_t seed, subsequence; int* call_counter; } cvae_bottleneck_noise;
int cvae_bottleneck_fwd(const cvae_bottleneck_dims* dims, const cvae_bottleneck_params* params, const void* y_cl, const float* m, float* t_onehot,
                        const int64_t* t_labels, float* eps, float* running_mean, float* running_var, long long* num_batches_tracked, float momentum,
                        float bn_eps, int bn_training, float* xcat, float* fwd_partial, float* dzm_acc, const cvae_bottleneck_saved* saved, void* dec_cl, int dtype,
                        const float* bn_rank_stats, int bn_ranks, const cvae_bottleneck_noise* noise, void* stream);
/* Backward (training-mode BatchNorm only).  g_dec_cl: gradient of dec_cl; g_mu / g_logvar / g_mhat: gradients arriving at the
 * three outputs (NULL = zero).  Writes every parameter gradient and dy_cl, the gradient of y_cl (zeroed where y_cl <= 0 when
 * relu_mask).  g1 is scratch of M*(N1+N2) floats; dzm_partial: dzm_partial_floats of scratch (any contents on entry).
 * bn_dy / bn_local_sums (both or neither): SyncBatchNorm, below. */
int cvae_bottleneck_bwd(const cvae_bottleneck_dims* dims, const cvae_bottleneck_params* params, const cvae_bottleneck_grads* grads,
                        const cvae_bottleneck_saved* saved, const void* g_dec_cl, const float* g_mu, const float* g_logvar, const float* g_mhat,
                        const float* t_onehot, const float* eps, const float* xcat, const void* y_cl, int relu_mask, float* dzm_partial, float* g1,
                        float* dx_partial, void* dy_cl, int dtype, float* bn_dy, float* bn_local_sums, void* stream);

/* ---- The same pair with mechanism_net's BatchNorm1d normalising over the GLOBAL batch of `bn_ranks` data-parallel ranks (SyncBatchNorm; replaces what
 * nn.SyncBatchNorm.convert_sync_batchnorm does to causal_cascade/models.py:36 under DDP).  The library runs no collective itself; the caller moves
 * 2 * HM floats per rank twice per step:
 *   1. cvae_bottleneck_bn_local_stats: local_stats [2][HM] = this rank's (sum, squared deviations from its own mean) of mechanism_net.0's output
 *      (it depends on t only, so it can run — and the all-gather can travel — before the encoder).  Wm0 [HM][t_dim], bm0 [HM]; t_onehot [M][t_dim] or t_labels [M]
 *      (either may be NULL);
 *   2. all-gather -> bn_rank_stats [bn_ranks][2][HM]; cvae_bottleneck_fwd combines them in rank order (Chan's update: identical bits on every rank),
 *      normalises with the global mean / variance and updates the running statistics with the global unbiased variance;
 *   3. cvae_bottleneck_bwd with bn_dy / bn_local_sums: mechanism_net's backward stops at the BatchNorm: bn_dy [M][HM] = the masked gradient at its output,
 *      bn_local_sums [2][HM] = this rank's (sum dy, sum dy * xhat) (also written to dbeta / dgamma: the rank's share, summed by the gradient exchange);
 *   4. all-reduce (sum) of bn_local_sums -> bn_sums; cvae_bottleneck_bn_bwd_finish writes dWm0 / dbm0 from bn_dy and the global sums (one small launch). */
int cvae_bottleneck_bn_local_stats(const float* Wm0, const float* bm0, const float* t_onehot, const int64_t* t_labels, float* local_stats, int64_t M, int64_t t_dim,
                                   int64_t HM, void* stream);
int cvae_bottleneck_bn_bwd_finish(const cvae_bottleneck_dims* dims, const cvae_bottleneck_params* params, const cvae_bottleneck_grads* grads,
                                  const cvae_bottleneck_saved* saved, const float* t_onehot, const float* bn_dy, const float* bn_sums, int bn_ranks, void* stream);

/* dW fp32 [Cs][Cl][taps] (overwritten) = sum over batch and positions.  workspace: cvae_conv_wgrad_workspace_bytes().
 * dbias (optional, overwritten) rides along in the same pass, where both tensors are read anyway:
 *   dbias_side 0: fp32 [Cs] = sum over batch and positions of S — the bias gradient of a Conv layer (S = output gradient);
 *   dbias_side 1: fp32 [Cl] = the same sum of L — the bias gradient of a ConvTranspose layer (L = output gradient). */
size_t cvae_conv_wgrad_workspace_bytes(int64_t Cs, int64_t Cl, int nd);
int cvae_conv_wgrad(const void* S, const void* L, float* dW, float* dbias, int dbias_side, void* workspace, size_t workspace_bytes,
                    int64_t B, int64_t sd, int64_t sh, int64_t sw, int64_t Cs,
                    int64_t ld, int64_t lh, int64_t lw, int64_t Cl, int nd, int dtype, void* stream);
/* The weight gradients of `count` (<= 8) layers in ONE main launch and ONE reduce launch: what a backward pass defers to its end, so
 * that the small layers (a few tiles each, launch- and latency-bound alone) run in the shadow of the large ones.  Arrays of `count`
 * entries; dims: count rows of 9 int64 {B, sd, sh, sw, Cs, ld, lh, lw, Cl}; every layer needs its OWN workspace
 * (cvae_conv_wgrad_workspace_bytes) because they run concurrently.  All layers share nd and dtype; Cl != 1, Cs % 64 == 0,
 * Cl % 32 == 0; an entry with dbias_side 1 needs L == 2 S (otherwise use cvae_conv_wgrad for that layer).  The partial sums of a layer
 * are split over fewer workgroups than in its own launch (the layers share the chip), so the results equal those of `count` calls of
 * cvae_conv_wgrad up to the fp32 summation order; they are reproducible bit for bit from run to run (no atomics). */
int cvae_conv_wgrad_multi(int count, const void* const* S, const void* const* L, float* const* dW, float* const* dbias, const int* dbias_side,
                          void* const* workspace, const size_t* workspace_bytes, const int64_t* dims, int nd, int dtype, void* stream);
/* out[c] = sum_p x[p, c] over a channels-last [P, C] tensor (bias gradients). out is overwritten.  workspace (optional,
 * cvae_channel_sum_workspace_bytes): partial rows of a multi-workgroup pass, added in index order (no float atomics); without it
 * the rows of one channel group are summed by ONE workgroup (same result bits for a given geometry, slower for large P). */
size_t cvae_channel_sum_workspace_bytes(int64_t P, int64_t C, int dtype);
int cvae_channel_sum(const void* x, float* out, int64_t P, int64_t C, int dtype, void* workspace, size_t workspace_bytes, void* stream);
/* y = act(x) elementwise (nn.ReLU / nn.Sigmoid / nn.LeakyReLU(0.2) / nn.LeakyReLU() when not fused into a producer). */
int cvae_act_fwd(const void* x, void* y, int64_t n, int act, int dtype, void* stream);
/* dx = dy * act'(y) elementwise (y = saved activation OUTPUT); dtype applies to all three. */
int cvae_act_bwd(const void* dy, const void* y, void* dx, int64_t n, int act, int dtype, void* stream);

/* ---- pooling / resize ----------------------------------------------------------------------------- */
/* x channels-last [B, D, H, W, C] -> out fp32 [B, out_stride], columns (c, od, oh, ow) flattened like
 * nn.AdaptiveAvgPool(d)+Flatten on NC(D)HW; adaptive windows [floor(i*I/O), ceil((i+1)*I/O)). */
int cvae_adaptive_avgpool_fwd(const void* x, float* out, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                              int64_t OD, int64_t OH, int64_t OW, int64_t out_stride, int dtype, void* stream);
/* dx[b, d, h, w, c] = sum over windows containing (d, h, w) of dout / |window|, times (x > 0) when relu_mask_x != NULL. */
int cvae_adaptive_avgpool_bwd(const float* dout, const void* relu_mask_x, void* dx, int64_t B, int64_t D, int64_t H, int64_t W, int64_t C,
                              int64_t OD, int64_t OH, int64_t OW, int64_t dout_stride, int dtype, void* stream);
/* (bi|tri)linear resize, align_corners = False, channels-last C channels; src dtype `dtype`, dst fp32. */
int cvae_upsample_linear_fwd(const void* src, float* dst, int64_t B, int64_t d, int64_t h, int64_t w,
                             int64_t D, int64_t H, int64_t W, int64_t C, int dtype, void* stream);
/* transpose of the above: dsrc (dtype `dtype`) = A^T ddst (fp32). */
int cvae_upsample_linear_bwd(const float* ddst, void* dsrc, int64_t B, int64_t d, int64_t h, int64_t w,
                             int64_t D, int64_t H, int64_t W, int64_t C, int dtype, void* stream);

/* ---- fp32 linear layers ------------------------------------------------------------------------------ */
/* Long reductions over few output tiles (the 16415-wide encoder layer at batch 4) are split across workgroups; each split leaves its
 * partial tile in a slab of `workspace` (cvae_linear_workspace_bytes(M, K, N, op); op 0 = fwd, 1 = bwd_data, 2 = bwd_weight) and a finish
 * launch adds the slabs in index order — no float atomics.  workspace may be NULL / smaller: the product then runs unsplit.
 * bf16_math != 0: bf16 MFMA operands (fp32 tensors in memory, rounded to bf16 on the way into LDS, fp32 accumulate and output): 16x the matrix rate of
 * the exact-fp32 form, relative error ~2^-9 per operand.  M > 16 only (smaller batches are HBM-bound skinny kernels: CVAE_E_UNSUPPORTED).
 * Row strides are in elements; one below its row length, or K, N <= 0, M < 0 is CVAE_E_BADSHAPE.  M == 0 is CVAE_OK from fwd and bwd_data (nothing is
 * launched) and CVAE_E_BADSHAPE from bwd_weight (dW of an empty batch is not written as zeros).  Every refusal comes before any launch. */
size_t cvae_linear_workspace_bytes(int64_t M, int64_t K, int64_t N, int op);
/* y[M, N] = act(x[M, K] @ W[N, K]^T + b). */
int cvae_linear_fwd(const float* x, const float* W, const float* b, float* y, int64_t M, int64_t K, int64_t N,
                    int64_t x_stride, int64_t y_stride, int act, int bf16_math, void* workspace, size_t workspace_bytes, void* stream);
/* dx[M, K] = (g[M, N] @ W[N, K]) * in_act'(x_in) with g = dy * act'(y_act) (y_act = the layer's saved OUTPUT, same shape/stride as dy; pass
 * NULL / CVAE_ACT_NONE for g = dy).  The fused activation gradient is available for M <= 16 (the model's batch sizes; CVAE_E_UNSUPPORTED above).
 * x_in [M][K] (row stride x_stride) / in_act: the derivative of the activation that produced this layer's INPUT (taken from its output, i.e. from x_in:
 * ReLU / LeakyReLU / Sigmoid) applied in the GEMM's epilogue (or its split-K slab sum) — in an MLP the previous layer then needs no activation-gradient
 * pass of its own (causal_cascade/models.py:24-31's Linear-ReLU-Linear chains).  M > 16 only (CVAE_E_UNSUPPORTED below); NULL / CVAE_ACT_NONE: none. */
int cvae_linear_bwd_data(const float* dy, const float* W, float* dx, int64_t M, int64_t K, int64_t N, int64_t dy_stride, int64_t dx_stride,
                         const float* y_act, int act, const float* x_in, int64_t x_stride, int in_act, int bf16_math,
                         void* workspace, size_t workspace_bytes, void* stream);
/* dW[N, K] = g^T x ; db[N] = column sums of g (db may be NULL).  Both overwritten.  g as above (y_act on dy's stride, M <= 16 only).
 * M > 16 with db needs dense dy rows, dy_stride == N (the column sums are a cvae_channel_sum pass): otherwise CVAE_E_UNSUPPORTED before any launch. */
int cvae_linear_bwd_weight(const float* dy, const float* x, float* dW, float* db, int64_t M, int64_t K, int64_t N,
                           int64_t dy_stride, int64_t x_stride, const float* y_act, int act, int bf16_math, void* workspace, size_t workspace_bytes,
                           void* stream);

/* ---- BatchNorm1d --------------------------------------------------------------------------------------- */
/* train: batch statistics (biased var) normalise; running stats updated with momentum (unbiased var). B >= 2. */
int cvae_bn1d_train_fwd(const float* x, const float* w, const float* b, float* y, float* save_mean, float* save_rstd,
                        float* running_mean, float* running_var, int64_t B, int64_t F, float momentum, float eps, void* stream);
int cvae_bn1d_train_bwd(const float* dy, const float* x, const float* w, const float* save_mean, const float* save_rstd,
                        float* dx, float* dw, float* db, int64_t B, int64_t F, void* stream);
int cvae_bn1d_eval_fwd(const float* x, const float* w, const float* b, const float* running_mean, const float* running_var,
                       float* y, int64_t B, int64_t F, float eps, void* stream);
/* The same BatchNorm1d cut where its batch sums appear, for statistics that span data-parallel ranks (SyncBN; the host all-reduces
 * the F-float sum vectors between the calls: a per-rank batch of 4 then normalises like the reference's single-process batch of 32,
 * causal_cascade/models.py:36 at the global batch):
 *   cvae_bn1d_stats        out[f] = sum_b x[b][f] (mean_sum NULL), else sum_b (x[b][f] - mean_sum[f] * inv_n)^2
 *   cvae_bn1d_apply_stats  y, save_mean, save_rstd, running stats from the reduced sums; inv_n = 1 / global batch
 *   cvae_bn1d_bwd_sums     sums[0:F] = sum_b dy (this rank's d beta), sums[F:2F] = sum_b dy * xhat (this rank's d gamma)
 *   cvae_bn1d_bwd_apply    dx from the REDUCED sums
 * The global batch holds at least 2 samples: inv_n outside (0, 0.5] is CVAE_E_BADSHAPE from cvae_bn1d_apply_stats and cvae_bn1d_bwd_apply. */
int cvae_bn1d_stats(const float* x, const float* mean_sum, float inv_n, float* out, int64_t B, int64_t F, void* stream);
int cvae_bn1d_apply_stats(const float* x, const float* w, const float* b, const float* mean_sum, const float* sqdev_sum, float inv_n, float* y,
                          float* save_mean, float* save_rstd, float* running_mean, float* running_var, int64_t B, int64_t F, float momentum,
                          float eps, void* stream);
int cvae_bn1d_bwd_sums(const float* dy, const float* x, const float* save_mean, const float* save_rstd, float* sums, int64_t B, int64_t F, void* stream);
int cvae_bn1d_bwd_apply(const float* dy, const float* x, const float* w, const float* save_mean, const float* save_rstd, const float* sums, float inv_n,
                        float* dx, int64_t B, int64_t F, void* stream);

/* ---- sampling + losses (all reductions accumulate into a caller-zeroed fp32 scalar) -------------------------
 * Every reduction takes (workspace, workspace_bytes): cvae_reduce_workspace_bytes() of scratch for the per-workgroup partial sums, which a
 * one-block finish launch adds in index order — no float atomics, the sums are bit-reproducible.  NULL / too small: the reduction runs
 * as a single workgroup (same contract, slower for large n). */
size_t cvae_reduce_workspace_bytes(void);
/* eps ~ N(0,1): Philox4x32-10 + Box-Muller, counter-based (seed = key, offset = counter words 0-1, subsequence = counter words 2-3)
 * -> reproducible per launch; different subsequences are independent streams of one seed (the Python side passes
 * (rank << 32) | model instance, so data-parallel ranks that share torch.manual_seed(42) still draw different noise).  call_counter
 * (optional device int): offset += *call_counter << 24, so a captured HIP graph draws fresh numbers on every replay. */
int cvae_philox_normal(float* out, int64_t n, uint64_t seed, uint64_t offset, uint64_t subsequence, const int* call_counter, void* stream);
/* The same draw followed by *call_counter += 1 (one launch for n <= 16384): what EpsSource issues once per forward pass. */
int cvae_philox_normal_advance(float* out, int64_t n, uint64_t seed, uint64_t offset, uint64_t subsequence, int* call_counter, void* stream);
/* z = mu + eps*exp(logvar/2) (if z != NULL);  *kld += -0.5*sum(1 + logvar - mu^2 - exp(logvar)) (if kld != NULL). */
int cvae_reparam_kld_fwd(const float* mu, const float* logvar, const float* eps, float* z, float* kld, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
/* dmu = dz + gk*mu ; dlogvar = dz*eps*0.5*exp(logvar/2) + gk*0.5*(exp(logvar) - 1), gk = *gkld * gk_scale;
 * dz / gkld (device scalar) may be NULL. */
int cvae_reparam_kld_bwd(const float* dz, const float* gkld, float gk_scale, const float* mu, const float* logvar, const float* eps,
                         float* dmu, float* dlogvar, int64_t n, void* stream);
/* The same head on the encoder's [B][2 Z] output rows (mu | logvar) without splitting them: z1 = mu + eps1 exp(logvar / 2), an optional second sample z2
 * from eps2, and *kld = the KLD sum (assigned; any of z1 / z2 / kld may be NULL).  One launch; B * Z <= 2^24.  The backward writes d h [B][2 Z] from
 * d z1, d z2 (either may be NULL) and the KLD's incoming gradient *gkld (NULL: 0). */
int cvae_latent_head_fwd(const float* h, const float* eps1, const float* eps2, float* z1, float* z2, float* kld, int64_t B, int64_t Z, void* stream);
int cvae_latent_head_bwd(const float* dz1, const float* dz2, const float* gkld, const float* h, const float* eps1, const float* eps2, float* dh,
                         int64_t B, int64_t Z, void* stream);
/* *out += sum (a - b)^2 */
int cvae_sse_fwd(const float* a, const float* b, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
/* da = 2*(a - b) * (*gout) * scale   (db = -da is formed by the caller when needed) */
int cvae_sse_bwd(const float* a, const float* b, const float* gout, float scale, float* da, int64_t n, void* stream);
/* out4[0] = out4[1] + wb*out4[2] + wc*out4[3]: total loss from its three terms, on the device */
int cvae_combine3(float* out4, float wb, float wc, void* stream);
/* F.binary_cross_entropy(p, x, reduction='sum') with torch's log clamp at -100 */
int cvae_bce_fwd(const float* p, const float* x, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int cvae_bce_bwd(const float* p, const float* x, const float* gout, float* dp, int64_t n, void* stream);
/* vessel recon terms (vessel_analysis/01_train/train.py:27-46): stats[0] = sum(x) must be produced first by
 * cvae_sum_fwd; then out[0] += sum (r-x)^2 (1 + (pw-1) x), out[1] += sum |r| [x < 0.1], pw = clamp((1-pf)/(pf+1e-6), 1, 50),
 * pf = *sum_x / (n_pos + 1e-6).  n_pos = the element count sum_x was taken over: n for a single process; under data parallelism the
 * caller all-reduces sum_x and passes the GLOBAL count, which reproduces the reference's batch-global pos_weight (:30-36). */
int cvae_sum_fwd(const float* x, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int cvae_wmse_sparsity_fwd(const float* r, const float* x, const float* sum_x, float* out2, int64_t n, int64_t n_pos, void* workspace, size_t workspace_bytes, void* stream);
int cvae_wmse_sparsity_bwd(const float* r, const float* x, const float* sum_x, const float* g_recon, const float* g_sparsity,
                           float* dr, int64_t n, int64_t n_pos, void* stream);
/* *out += 0.5 * sum(logvar + (m - mu)^2 / exp(logvar)) */
int cvae_gauss_nll_fwd(const float* m, const float* mu, const float* logvar, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
int cvae_gauss_nll_bwd(const float* m, const float* mu, const float* logvar, const float* gout, float* dmu, float* dlogvar, int64_t n, void* stream);
/* *out += mean_b CE(logits[b, :], target[b])  (F.cross_entropy, reduction='mean'); dlogits = (softmax - onehot)/B * gout */
int cvae_softmax_ce_fwd(const float* logits, const int64_t* target, float* out, int64_t B, int64_t C, void* workspace, size_t workspace_bytes, void* stream);
int cvae_softmax_ce_bwd(const float* logits, const int64_t* target, const float* gout, float* dlogits, int64_t B, int64_t C, void* stream);
/* *out += F.kl_div(log_softmax(logits), full(1/C), reduction='batchmean'); dlogits = (softmax - 1/C)/B * gout */
int cvae_uniform_kl_fwd(const float* logits, float* out, int64_t B, int64_t C, void* workspace, size_t workspace_bytes, void* stream);
int cvae_uniform_kl_bwd(const float* logits, const float* gout, float* dlogits, int64_t B, int64_t C, void* stream);

/* ---- nn.Linear (+ activation) for SMALL layers at LARGE batch (csrc/small_dense.hip): M > 16 rows (below 2^30), 1 <= K, N <= 128 and N * K <= 12288 weights — the MLP heads of
 * mnist_test/01_baseline_causal_vae/models.py:24-37, 93-111 at batch 1024.  The weight lives in LDS; one launch forward, one for the data gradient, two for the
 * weight + bias gradient (per-workgroup partials in `workspace`, summed in index order: no atomics).  fp32 throughout.
 *   fwd         y = act(x W^T + b)
 *   bwd_data    dx = ((dy * act'(y_act)) W) * in_act'(x_in)     y_act / x_in may be NULL (ACT_NONE): both activation gradients ride in this launch
 *   bwd_weight  dW = (dy * act'(y_act))^T x,  db = column sums of (dy * act'(y_act))  (db may be NULL)
 * act and in_act: every CVAE_ACT_* code (NONE, RELU, SIGMOID, LEAKY02, LEAKY001).  cvae_small_dense_supported answers 1 for a shape inside the limits and
 * cvae_small_dense_workspace_bytes gives what bwd_weight needs (0 outside the limits; CVAE_E_WORKSPACE below it, CVAE_E_NULLPTR without a workspace).  A shape
 * outside the limits, a row stride below the row length (y_stride / x_stride: only where y_act / x_in is read) or another activation code is CVAE_E_BADSHAPE,
 * before any launch. */
int cvae_small_dense_supported(int64_t M, int64_t K, int64_t N);
size_t cvae_small_dense_workspace_bytes(int64_t M, int64_t K, int64_t N);
int cvae_small_dense_fwd(const float* x, const float* W, const float* b, float* y, int64_t M, int64_t K, int64_t N, int64_t x_stride, int64_t y_stride, int act, void* stream);
int cvae_small_dense_bwd_data(const float* dy, const float* W, float* dx, const float* y_act, int act, const float* x_in, int in_act, int64_t M, int64_t K, int64_t N,
                              int64_t dy_stride, int64_t dx_stride, int64_t y_stride, int64_t x_stride, void* stream);
int cvae_small_dense_bwd_weight(const float* dy, const float* x, float* dW, float* db, const float* y_act, int act, int64_t M, int64_t K, int64_t N, int64_t dy_stride,
                                int64_t x_stride, int64_t y_stride, void* workspace, size_t workspace_bytes, void* stream);

/* ---- optimiser ---------------------------------------------------------------------------------------------- */
/* torch.optim.Adam (no weight decay / amsgrad) on flat fp32 buffers; bias corrections bc1 = 1-b1^t, bc2 = 1-b2^t
 * computed by the caller.  grad_scale: optional device scalar multiplied into g first (gradient clipping). */
int cvae_adam_step(float* p, const float* g, float* m, float* v, int64_t n, float lr, float beta1, float beta2, float eps,
                   float bc1, float bc2, const float* grad_scale, void* stream);
/* The same update for a LIST of tensors in one launch (host arrays of `count` device pointers / sizes).  step_dev: optional
 * device int holding the step number t; when non-NULL the kernel derives bc1/bc2 from it (HIP-graph replay safe). */
int cvae_adam_multi(float* const* p, const float* const* g, float* const* m, float* const* v, const int64_t* n, int count,
                    float lr, float beta1, float beta2, float eps, float bc1, float bc2, const int* step_dev,
                    const float* grad_scale, void* stream);
/* dst[i][0..n[i]) = src[i][0..n[i]) for a LIST of fp32 tensors in one launch (gradient bucket pack / unpack). */
int cvae_multi_copy(const float* const* src, float* const* dst, const int64_t* n, int count, void* stream);
/* *counter += delta (device int; step counters that must advance inside a captured graph) */
int cvae_counter_add(int* counter, int delta, void* stream);
/* *out += sum g^2 */
int cvae_sqnorm(const float* g, float* out, int64_t n, void* workspace, size_t workspace_bytes, void* stream);
/* Weighted sum of up to 8 scalar (0-dim, device) loss terms: backward == 0: out[0] = sum_i weights[i] * *terms[i] and out[1 + i] = weights[i] * *terms[i]
 * (host arrays of device pointers / host floats; `out` holds count + 1 floats); backward != 0: out[i] = weights[i] * *g (g NULL = 1) for i < count —
 * the gradient of every term. */
int cvae_weighted_sum(const float* const* terms, const float* weights, int count, const float* g, float* out, int backward, void* stream);
/* The same sum over a LIST of tensors (host arrays of `count` device pointers / sizes) in one launch + one finish; workspace: cvae_reduce_workspace_bytes()
 * (one block per tensor at least: CVAE_E_WORKSPACE below min(count, 64) + 1 floats, 64 being the tensors of one launch's table; a NULL workspace too). */
int cvae_sqnorm_multi(const float* const* g, const int64_t* n, int count, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* g *= *scale  (in place; scale is a device scalar) */
int cvae_scale(float* g, int64_t n, const float* scale, void* stream);
/* *scale = min(1, max_norm / (sqrt(*sqnorm) + 1e-6))   (clip_grad_norm_ coefficient, on device) */
int cvae_clip_coef(const float* sqnorm, float* scale, float max_norm, void* stream);

/* ---- The latent translator (csrc/ridge.hip): the reference's latent_translator/analysis.py:11-82 (a Ridge regression from the latents
 * Z [N][d] to the morphology table M [N][F], its leave-one-out ranking) and the group means of :91-165 (the group-contrast bootstrap).  FLOAT64 ONLY: every
 * array below is double, row-major, 8-byte aligned (else CVAE_E_UNSUPPORTED); row strides are in elements and at least the row length (else CVAE_E_BADSHAPE).
 * Contract, as everywhere: enqueue-only on `stream`; the caller owns every buffer and workspace; every check precedes the first launch; no float atomics, no
 * workgroup waits on another, every sum in one fixed order, every grid a function of the shape alone: two runs give equal bits.
 * Limits: 2 <= N < 2^31, 1 <= d <= 1024, 1 <= F < 2^21, N F < 2^38 (else CVAE_E_BADSHAPE); a null pointer: CVAE_E_NULLPTR; a workspace below its query:
 * CVAE_E_WORKSPACE.
 * The leave-one-out prediction of a ridge with an unpenalised intercept is exact in closed form: with Xc = Z - zbar, A = Xc^T Xc + alpha I = L L^T,
 * W = A^-1 Xc^T (M - mbar), Yhat = mbar + Xc W and h_i = 1 / N + xc_i^T A^-1 xc_i = 1 / N + |L^-1 xc_i|^2, the fit without row i predicts
 * p_i = y_i - (y_i - yhat_i) / (1 - h_i).  One Gram matrix, one factorisation and three triangular solves replace the reference's N fits.
 *   cvae_col_means_f64       mean[c] = (sum over rows, chunk by chunk in row order, the chunks in order) / N of x [N][C] (1 <= N, C < 2^31).
 *   cvae_ridge_gram_f64      A [d][d] = Xc^T Xc + alpha I (both triangles written, bitwise symmetric) and R [d][F] = Xc^T (M - mbar) on v_mfma_f64_16x16x4_f64.  The
 *                            means are subtracted on load (mean first, then centred products).  The rows are split into ceil(N / chunk) <= 16 chunks, chunk the
 *                            smallest multiple of 256 that allows it; the chunks' partial products [chunks][d][d + F] go to `workspace` and a finish launch adds
 *                            them in chunk order.  alpha <= 0, NaN or infinite: CVAE_E_BADSHAPE (the centred Gram matrix is singular without it).
 *   cvae_chol_f64            A = L L^T in place, lower triangle (the strict upper triangle is left as it was), 1 <= d <= 1024, in blocks of 64 columns: the
 *                            panel (one workgroup), the rows below it, the trailing update — three launches per block and nothing that waits across workgroups.
 *                            *info (device int) = 0, or column + 1 of the first pivot that is <= 0 or NaN; the entry then still runs to its end without
 *                            faulting and that column and every later one are NaN.
 *   cvae_trsm_f64            transpose == 0: L T = B by forward substitution; transpose == 1: L^T W = B by back substitution; L [d][>= d] lower triangular (its
 *                            upper triangle is not read), B and the result [d][n], 1 <= n < 2^31, one thread per column.  B is read as
 *                            in[k * in_row_stride + c * in_col_stride] - row_shift[k] (row_shift may be NULL), so the right-hand side Xc^T is Z itself with
 *                            strides (1, z_stride) and row_shift = zbar.  in == out is allowed element for element only (in_row_stride == ldo, in_col_stride == 1).
 *   cvae_ridge_loo_f64       from W [d][F] (the solution) and T [d][N] = L^-1 Xc^T: leverage [N] = 1 / N + sum_k T[k][i]^2, fitted [N][F] = mbar + Xc W,
 *                            loo [N][F] = M - (M - fitted) / (1 - leverage), coef [F][d] = W^T, intercept [F] = mbar - zbar^T W.  Three launches.
 *   cvae_ridge_predict_f64   out [N][F] = intercept + Z coef^T (N == 0 is CVAE_OK, nothing is launched).
 *   cvae_ranking_stats_f64   per feature j of Y (the truth) and P (the leave-one-out predictions), both [N][F], the rules of analysis.py:55-68:
 *                            r2 = 1 - sum (y - p)^2 / sum (y - ybar)^2, and where that denominator is 0 sklearn's value (1 if the numerator is 0 too, else 0);
 *                            corr = the Pearson correlation, clipped to [-1, 1] as numpy.corrcoef does, and 0 where the population standard deviation of either
 *                            side is below 1e-12.  One workgroup per feature, 1 <= N.
 *   cvae_group_means_resampled_f64   out [n_boot][G][d] = the mean over i, in index order, of Z[idx[b][i]] whose codes[idx[b][i]] == g, counts [n_boot][G] (int)
 *                            how many there were; an empty group gives a zero row and count 0.  codes [N] and idx [n_boot][N] are int (4-byte aligned); an index
 *                            outside [0, N) or a code outside [0, G) belongs to no group.  1 <= d <= 65536, 1 <= G <= 65535, n_boot <= 65535 (0: CVAE_OK, nothing
 *                            is launched). */
size_t cvae_col_means_f64_workspace_bytes(int64_t N, int64_t C);
int cvae_col_means_f64(const double* x, int64_t N, int64_t C, int64_t stride, double* mean, void* workspace, size_t workspace_bytes, void* stream);
size_t cvae_ridge_gram_f64_workspace_bytes(int64_t N, int64_t d, int64_t F);
int cvae_ridge_gram_f64(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, int64_t N, int64_t d,
                        int64_t F, double alpha, double* A, double* R, void* workspace, size_t workspace_bytes, void* stream);
int cvae_chol_f64(double* A, int64_t d, int* info, void* stream);
int cvae_trsm_f64(const double* L, int64_t ldl, const double* in, int64_t in_row_stride, int64_t in_col_stride, const double* row_shift, double* out, int64_t ldo,
                  int64_t d, int64_t n, int transpose, void* stream);
int cvae_ridge_loo_f64(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, const double* W,
                       const double* T, int64_t N, int64_t d, int64_t F, double* leverage, double* fitted, double* loo, double* coef, double* intercept, void* stream);
int cvae_ridge_predict_f64(const double* Z, int64_t z_stride, const double* coef, const double* intercept, int64_t N, int64_t d, int64_t F, double* out, void* stream);
int cvae_ranking_stats_f64(const double* Y, int64_t y_stride, const double* P, int64_t p_stride, int64_t N, int64_t F, double* r2, double* corr, void* stream);
int cvae_group_means_resampled_f64(const double* Z, int64_t z_stride, const int* codes, const int* idx, int64_t N, int64_t d, int64_t G, int64_t n_boot, double* out,
                                   int* counts, void* stream);

/* ---- The symmetric eigensolver, the ridge alpha path and the latent PCA (csrc/eigh.hip, csrc/ridge.hip).  FLOAT64 ONLY, with the conventions
 * of the section above (8-byte aligned row-major doubles, strides in elements, every check before the first launch, no float atomics, fixed orders, equal bits).
 *   cvae_eigh_f64            A [n][>= lda] symmetric (the lower triangle is read), 1 <= n <= 1024: w [n] ascending (ties by original index) and V [n][>= ldv] with
 *                            column k the eigenvector of w[k] (numpy.linalg.eigh's convention).  A two-sided Jacobi method in round-robin order: n - 1 (n even) or
 *                            n (n odd, one pair a bye) rounds per sweep, one launch per round in which all the round's disjoint pairs rotate, between two buffers
 *                            of `workspace` (cvae_eigh_f64_workspace_bytes: 4 n^2 doubles and a little).  A sweep in which no rotated |a_pq| exceeded
 *                            2^-53 max |A| is the last.  NOT enqueue-only: the host reads one word from the device before the first sweep and after every sweep
 *                            (a stream synchronisation each; the entry cannot be captured into a graph) and stops launching when it is set; at most
 *                            cvae_eigh_max_sweeps() sweeps.  info (device int [2], 4-byte aligned): info[0] = 0 converged, 1 the sweep cap was reached, 2 a
 *                            non-finite entry was met (in A, or on the diagonal after a sweep; w and V are then unspecified); info[1] = the sweeps used (the
 *                            last one, which only confirms, included).  No loop in any kernel has a trip count that depends on data: the entry returns for
 *                            every input.  Eigenvalues are not clamped.
 *   cvae_centered_gram_f64   cvae_ridge_gram_f64 without the shift and with F >= 0: G [d][d] = Xc^T Xc, R [d][F] = Xc^T (M - mbar), the same two launches; with
 *                            F == 0, M, m_mean and R are not read and may be NULL.  1 <= N.
 *   cvae_centered_matmul_f64 out [R][>= ldo] = (X - mean) B on v_mfma_f64_16x16x4_f64, X read as x[i x_row_stride + k x_col_stride] - mean[k] (mean [K] may be
 *                            NULL: nothing is subtracted), B as b[k b_row_stride + j b_col_stride]: either operand may be a transpose in place.  The mean is
 *                            subtracted on load.  1 <= K <= 1024, 1 <= R < 2^31, 1 <= C < 2^21; out must not be x or b.  One launch, K walked in order.
 *   cvae_ridge_path_f64      with P [N][d] = Xc V, Q [d][F] = V^T Xc^T Yc, lambda [d] the eigenvalues of Xc^T Xc (clamped at 0 from below here, and written so to
 *                            eigenvalues [d], which must not be lambda) and alphas [G] in device memory, 1 <= G <= 64:
 *                            leverage [G][N] = 1 / N + sum_k P[i][k]^2 / (lambda_k + alpha_g), loo [G][N][F] = M - (M - Yhat) / (1 - leverage) with
 *                            Yhat = mbar + sum_k P[i][k] Q[k][j] / (lambda_k + alpha_g), sse [G][F] = sum_i (M - loo)^2 (a thread's rows in row order, the 256
 *                            partial sums in a fixed tree).  Three launches.  The alphas are not checked on the device.
 *   cvae_pca_components_f64  from cvae_eigh_f64's w [d] and V of the centred Gram matrix of N rows: components [k][d] = the k last columns of V in descending
 *                            order of eigenvalue, each signed so that its entry of largest |value| (lowest index on a tie) is positive; explained_variance [k] =
 *                            w / (N - 1), explained_variance_ratio [k] = w / (the sum of all d, in index order), singular_values [k] = sqrt(w), w clamped at 0.
 *                            1 <= k <= min(N - 1, d). */
int cvae_eigh_max_sweeps(void);
size_t cvae_eigh_f64_workspace_bytes(int64_t n);
int cvae_eigh_f64(const double* A, int64_t lda, int64_t n, double* w, double* V, int64_t ldv, int* info, void* workspace, size_t workspace_bytes, void* stream);
size_t cvae_centered_gram_f64_workspace_bytes(int64_t N, int64_t d, int64_t F);
int cvae_centered_gram_f64(const double* Z, int64_t z_stride, const double* z_mean, const double* M, int64_t m_stride, const double* m_mean, int64_t N, int64_t d,
                           int64_t F, double* G, double* R, void* workspace, size_t workspace_bytes, void* stream);
int cvae_centered_matmul_f64(const double* x, int64_t x_row_stride, int64_t x_col_stride, const double* mean, const double* b, int64_t b_row_stride,
                             int64_t b_col_stride, int64_t R, int64_t K, int64_t C, double* out, int64_t ldo, void* stream);
int cvae_ridge_path_f64(const double* P, const double* Q, const double* lambda, const double* alphas, const double* M, int64_t m_stride, const double* m_mean,
                        int64_t N, int64_t d, int64_t F, int64_t G, double* eigenvalues, double* leverage, double* loo, double* sse, void* stream);
int cvae_pca_components_f64(const double* w, const double* V, int64_t ldv, int64_t d, int64_t k, int64_t N, double* components, double* explained_variance,
                            double* explained_variance_ratio, double* singular_values, void* stream);

/* ---- Exact t-SNE of the latents (csrc/tsne.hip): sklearn's method="exact" pipeline, two components, one degree of freedom.  FLOAT64 ONLY, with
 * the conventions of the two sections above (8-byte aligned row-major doubles, every check before the first launch, no float atomics, fixed orders, equal bits).
 * 3 <= N <= 4096 everywhere; square matrices are dense [N][N]; Y, update, gains, A, R and grad are [N][2].
 *   cvae_tsne_sqdist_f64     Z [N][>= z_stride] float64, or float32 with z_is_f32 (converted on load), d >= 1: D[i][j] = sum_k (z_ik - z_jk)^2 from differences,
 *                            k in index order, one fma per term; D is bitwise symmetric and its diagonal is 0.  32 x 32 tiles, the rows staged in LDS 32 columns
 *                            at a time.
 *   cvae_tsne_affinities_f64 per row i over j != i with d' = D[i][j] - min_j D[i][j]: e_j = exp(-beta d'_j), S = sum e_j, H = log S + beta (sum d'_j e_j) / S;
 *                            beta by sklearn's search (from 1; while H > log perplexity the lower bound moves up and beta doubles until an upper bound exists, then
 *                            takes midpoints; the mirror image below), at most 100 steps, the first step with |H - log perplexity| <= tol the last (tol = 0: all
 *                            100 unless H hits the target).  Pc[i][j] = e_j / S at the last beta evaluated, Pc[i][i] = 0; beta [N]; steps [N] (int) = the steps
 *                            taken.  0 < perplexity < N, tol >= 0.  One workgroup per row, the shifted row in LDS; the trip count is at most 100 for every
 *                            input, non-finite ones included.  Pc must not be D.
 *   cvae_tsne_joint_f64      P = max((Pc + Pc^T) / s, 2^-52) off the diagonal, 0 on it, s = the sum of all entries of Pc + Pc^T (32 x 32 tile sums, added in
 *                            order by one workgroup); P is bitwise symmetric.  info (device int [1]): 0, or 2 if an entry of D, Pc or the sum is not finite (P is
 *                            then unspecified).  workspace: cvae_tsne_joint_f64_workspace_bytes(N).  Three launches.  P must be neither Pc nor D.
 *   cvae_tsne_forces_f64     the pair pass: per row i over j != i, w = 1 / (1 + |y_i - y_j|^2): S [N] = sum w, A = sum P w (y_i - y_j), R = sum w^2 (y_i - y_j)
 *                            and, unless kl_partials is NULL, kl_partials [3][N] = (sum P log P, sum P log w, sum P).  P must be positive off the diagonal for the
 *                            partials (cvae_tsne_joint_f64's is).  A few rows per workgroup, the columns strided over its threads, Y in LDS.
 *   cvae_tsne_grad_f64       Zs = sum S in a fixed order, grad = 4 (exaggeration A - R / Zs) and, unless kl is NULL, kl [1] = the KL divergence of
 *                            exaggeration P from Q = w / Zs: exaggeration (sum P log P + (log exaggeration + log Zs) sum P - sum P log w).  sklearn's clamp of Q
 *                            at 2^-52 is not applied.
 *   cvae_tsne_update_f64     one iteration of sklearn's _gradient_descent on every element: with grad as above, gains = (update grad < 0) ? gains + 0.2 :
 *                            0.8 gains, at least 0.01; update = momentum update - learning_rate gains grad; Y += update; written to Y_out, update_out, gains_out
 *                            (which must not be the inputs: nothing is updated in place).  Unless record is NULL, record [4] = (that KL, |gains grad|^2, 1.0 if
 *                            a new position, the KL or the norm is not finite else 0.0, Zs).
 *   cvae_tsne_fit_f64        TSNE._tsne from P and Y (in: the start, out: the embedding): min(250, max_iter) iterations at early_exaggeration and momentum 0.5,
 *                            then up to max_iter at 1 and 0.8, two launches per iteration (forces, update) between two sets of buffers in `workspace`
 *                            (cvae_tsne_fit_f64_workspace_bytes).  NOT enqueue-only: after every iteration i with (i + 1) % 50 == 0 the host reads the record
 *                            (a stream synchronisation each; the entry cannot be captured into a graph) and applies sklearn's tests in sklearn's order: a KL that
 *                            is not a new best for more than 250 (first phase) or n_iter_without_progress (second) iterations ends the phase; a |gains grad| <=
 *                            min_grad_norm ends the fit (sklearn would go on to the second phase and stop at its first check).  kl [1] = the KL of P
 *                            (exaggeration 1) at the returned Y, from one more pair pass (sklearn reports the KL before the last update); max_iter = 0 returns Y
 *                            unchanged with its KL.  info (device int [4]): info[0] = 0, or 2 if a position, the KL or the norm stopped being finite (seen at a
 *                            check or at the end); info[1] = the index of the last iteration run (sklearn's n_iter_; 0 if none ran); info[2] = why the descent
 *                            ended: 0 the iterations ran out, 1 the gradient norm, 2 no progress in the second phase; info[3] = the records read. */
int cvae_tsne_sqdist_f64(const void* Z, int z_is_f32, int64_t z_stride, int64_t N, int64_t d, double* D, void* stream);
int cvae_tsne_affinities_f64(const double* D, int64_t N, double perplexity, double tol, double* Pc, double* beta, int* steps, void* stream);
size_t cvae_tsne_joint_f64_workspace_bytes(int64_t N);
int cvae_tsne_joint_f64(const double* D, const double* Pc, int64_t N, double* P, int* info, void* workspace, size_t workspace_bytes, void* stream);
int cvae_tsne_forces_f64(const double* Y, const double* P, int64_t N, double* A, double* R, double* S, double* kl_partials, void* stream);
int cvae_tsne_grad_f64(const double* A, const double* R, const double* S, const double* kl_partials, int64_t N, double exaggeration, double* grad, double* kl,
                       void* stream);
int cvae_tsne_update_f64(const double* Y, const double* update, const double* gains, const double* A, const double* R, const double* S, const double* kl_partials,
                         int64_t N, double exaggeration, double momentum, double learning_rate, double* Y_out, double* update_out, double* gains_out, double* record,
                         void* stream);
size_t cvae_tsne_fit_f64_workspace_bytes(int64_t N);
int cvae_tsne_fit_f64(const double* P, double* Y, int64_t N, double early_exaggeration, double learning_rate, int64_t max_iter, int64_t n_iter_without_progress,
                      double min_grad_norm, double* kl, int* info, void* workspace, size_t workspace_bytes, void* stream);

/* ---- Morphology of small grey images (csrc/morphology.hip): the 12 features of the reference's extract_refined_features
 * (mnist_test/01_baseline_causal_vae/dataset.py:11-99) for a batch, ONE launch, one workgroup per image, everything in LDS; enqueue-only (no host read, no
 * allocation: the call can be captured into a graph).  x [B][H][W] fp32 contiguous, 1 <= H, W <= CVAE_MORPH_MAX_SIDE, B >= 1; feats [B][12] fp32; raw NULL or
 * int [B][CVAE_MORPH_RAW_WORDS].  Coordinates are (r, c).  Per image, in integers: mask = x > threshold (fp32; a NaN is background); 8-connected components,
 * labelled in raster order of their first pixel; the measured component is the one of largest area, ties to the lowest label; its area, bounding box and raw
 * sums; its perimeter histogram (border = component minus its erosion by the 4-neighbour cross, outside = background; code = 1 + 2 (4-neighbours in border) +
 * 10 (diagonal neighbours in border)); the largest squared Euclidean distance from a pixel of the WHOLE mask to the nearest background pixel of the image;
 * the number of pixel centres inside or on the convex hull of the points (r +- 1/2, c), (r, c +- 1/2) of the component's pixels; the bit-quad counts of the
 * zero-padded component.  The features, formed in fp64 and rounded once, in the reference's order:
 *   A / area_norm;  (n[5,7,15,17,25,27] + sqrt 2 n[21,33] + (1 + sqrt 2) / 2 n[13,23]) / perimeter_norm;  sqrt(max d^2) / thickness_norm;
 *   4 sqrt(lambda1) / axis_norm;  sqrt(disc / lambda1) (0 if lambda1 = 0);  (orientation + pi / 2) / pi;  A / convex;  A / (h w);  (w / h) / 3;  (euler + 2) / 4;
 *   1 - mean |x - fliplr x|;  1 - mean |x - flipud x|   (over the whole grey image, fp32 differences added in fp64 in a fixed order)
 * with a = mu02 / A, c = mu20 / A, b = -mu11 / A, disc = sqrt((a - c)^2 + 4 b^2), lambda1 = (a + c + disc) / 2, orientation = atan2(-2 b, c - a) / 2, or
 * -pi / 4 (b < 0) / +pi / 4 when a == c exactly.  An empty mask gives twelve zeros; a mask without a background pixel gives a NaN thickness.  An image's output
 * bits depend on the image alone.  Codes: B, H or W < 1, a norm that is not positive, a NaN threshold: CVAE_E_BADSHAPE; H or W above the limit, B >= 2^31:
 * CVAE_E_UNSUPPORTED; x or feats NULL: CVAE_E_NULLPTR.  cvae_morph12_threads: the threads per image this build uses for a shape (CVAE_MORPH_THREADS up to
 * CVAE_MORPH_SMALL_PIXELS pixels, CVAE_MORPH_THREADS_LARGE above); the output does not depend on it. */
#define CVAE_MORPH_MAX_SIDE 64
#define CVAE_MORPH_RAW_WORDS 32
#define CVAE_MORPH_RAW_STATUS 0      /* bits: CVAE_MORPH_EMPTY, CVAE_MORPH_NO_BACKGROUND */
#define CVAE_MORPH_RAW_COMPONENTS 1  /* 8-connected components of the mask */
#define CVAE_MORPH_RAW_FIRST 2       /* raster index r W + c of the measured component's first pixel; -1 for an empty mask */
#define CVAE_MORPH_RAW_AREA 3
#define CVAE_MORPH_RAW_MINR 4        /* the bounding box as skimage gives it: min row, min column, max row + 1, max column + 1 */
#define CVAE_MORPH_RAW_MINC 5
#define CVAE_MORPH_RAW_MAXR 6
#define CVAE_MORPH_RAW_MAXC 7
#define CVAE_MORPH_RAW_SR 8          /* sum r, sum c, sum r^2, sum c^2, sum r c over the component */
#define CVAE_MORPH_RAW_SC 9
#define CVAE_MORPH_RAW_SRR 10
#define CVAE_MORPH_RAW_SCC 11
#define CVAE_MORPH_RAW_SRC 12
#define CVAE_MORPH_RAW_PERIM 13      /* ten counts, of the codes 5, 7, 15, 17, 25, 27 (weight 1), 21, 33 (sqrt 2), 13, 23 ((1 + sqrt 2) / 2) */
#define CVAE_MORPH_RAW_MAXD2 23      /* -1 without a background pixel */
#define CVAE_MORPH_RAW_CONVEX 24
#define CVAE_MORPH_RAW_Q1 25         /* bit-quads with one, three, two diagonal pixels set; euler = (Q1 - Q3 - 2 QD) / 4 */
#define CVAE_MORPH_RAW_Q3 26
#define CVAE_MORPH_RAW_QD 27
#define CVAE_MORPH_RAW_EULER 28      /* words 29 .. 31 are 0; an empty mask leaves every word but STATUS and FIRST 0 */
#define CVAE_MORPH_EMPTY 1
#define CVAE_MORPH_NO_BACKGROUND 2
int cvae_morph12_threads(int64_t H, int64_t W);
int cvae_morph12_f32(const float* x, int64_t B, int64_t H, int64_t W, float threshold, double area_norm, double perimeter_norm, double thickness_norm,
                     double axis_norm, float* feats, int* raw, void* stream);

/* ---- Vessel image preparation (csrc/image_prep.hip): the reference's two image transforms (vessel_analysis/00_core/dataset.py:192-237,
 * latent_translator/utils.py:18-60) for a batch.  Every entry is enqueue-only (no host read, no allocation).  Grids depend on the shapes alone, there is no float
 * atomic, and every sum that crosses workgroups is merged in a fixed order: an image's output bits depend on the image alone, not on B or its place in the batch.
 * Common codes: a size < 1: CVAE_E_BADSHAPE; a dtype code the entry does not take: CVAE_E_DTYPE; B > 65535 or an image of 2^31 pixels or more:
 * CVAE_E_UNSUPPORTED; a NULL pointer: CVAE_E_NULLPTR; a workspace that is NULL or too small: CVAE_E_WORKSPACE.  Nothing is launched on a refusal.
 *
 * cvae_mip_max: src [B][D][Hs][Ws] of uint16 (CVAE_U16) or fp32 (CVAE_F32) -> dst fp32 [B][Hs][Ws] = the maximum over D; a NaN propagates (np.max).
 *
 * cvae_resize_bilinear_aa_f32: torch's F.interpolate(mode="bilinear", antialias=True, align_corners=False) of src fp32 [B][Hs][Ws] -> dst fp32 [B][H][W], ONE
 * launch: a workgroup owns an output tile, filters the source rows its tile needs along W into LDS and then along H from LDS.  Per axis n_in -> n_out, in fp64:
 * scale = n_in / n_out, support = max(scale, 1), c = scale (i + 1/2), xmin = max(0, (int)(c - support + 1/2)), xmax = min((int)(c + support + 1/2), n_in),
 * w_j = max(0, 1 - |(j - c + 1/2) / support|) over xmin <= j < xmax divided by their sum and rounded to fp32; the products are added in fp32 in ascending j.
 * Equal sizes copy the bits.  A shape whose tile needs more source rows than LDS holds (a height ratio above about 50) is CVAE_E_UNSUPPORTED.
 *
 * cvae_minmax_binarise: y fp32 [B][H][W] -> out [B A][H][W] of 0 / 1 in fp32 or bf16 (out_dtype), A = 1 or 4 (image b's variants at b A + a: a = 0 as it is,
 * 1 flipped along W, 2 along H, 3 both), and rec[b].  mn, mx = the image's extremes; v = fl32((y - mn) / fl32(mx - mn)) (two correctly rounded fp32
 * operations); thr = (the fp64 sum of v in a fixed order) / (H W) in fp64; pixel = (double)v > thr.  mx == mn: zeros and CVAE_PREP_CONSTANT; a NaN or an
 * infinity anywhere in the image: zeros and CVAE_PREP_NONFINITE.  Three launches (extremes, sum, apply); the statistics are formed once per source image.
 *
 * cvae_percentile_clip_scale: x fp32 [B][N] -> out fp32 [B][N] and rec[b].  ranks[4] = the 0-based order statistics (lo, lo', hi, hi') and t[2] the two
 * fractions of numpy's "linear" percentile pair, computed by the caller; a radix select (4 passes of 8 bits over the order-preserving uint32 image of the
 * floats, per-workgroup LDS histograms merged in order) finds the four values exactly; vmin = lerp(x_lo, x_lo', t[0]), vmax = lerp(x_hi, x_hi', t[1]) with
 * numpy's lerp(a, b, t) = a + d t, or b - d (1 - t) when t >= 1/2, d = (double)fl32(b - a), in fp64 without contraction; denom = vmax - vmin, 1e-5 when 0;
 * out = fl32((min(max((double)x, vmin), vmax) - vmin) / denom).  A NaN or an infinity in the image sets CVAE_PREP_NONFINITE (its output is unspecified).
 * A rank outside [0, N): CVAE_E_BADSHAPE. */
#define CVAE_U16 3                   /* dtype code of cvae_mip_max's source only */
#define CVAE_PREP_CONSTANT 1
#define CVAE_PREP_NONFINITE 2
typedef struct { double thr; int64_t ones; float mn, mx; int32_t flags, reserved; } cvae_binarise_record;          /* 32 bytes; ones counts variant 0 */
typedef struct { double vmin, vmax; int32_t flags, reserved; } cvae_clip_record;                                   /* 24 bytes */
int cvae_mip_max(const void* src, float* dst, int64_t B, int64_t D, int64_t Hs, int64_t Ws, int src_dtype, void* stream);
int cvae_resize_bilinear_aa_f32(const float* src, float* dst, int64_t B, int64_t Hs, int64_t Ws, int64_t H, int64_t W, void* stream);
size_t cvae_minmax_binarise_workspace_bytes(int64_t B, int64_t H, int64_t W);
int cvae_minmax_binarise(const float* y, void* out, cvae_binarise_record* rec, int64_t B, int64_t H, int64_t W, int augment4, int out_dtype, void* workspace,
                         size_t workspace_bytes, void* stream);
size_t cvae_percentile_clip_scale_workspace_bytes(int64_t B, int64_t N);
int cvae_percentile_clip_scale(const float* x, float* out, cvae_clip_record* rec, int64_t B, int64_t N, const int64_t* ranks, const double* t, void* workspace,
                               size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CVAE_HIP_H */
