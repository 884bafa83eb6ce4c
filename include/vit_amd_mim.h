/* vit_amd_mim.h -- masked spectrum modelling: self-supervised pre-training in SimMIM's form, restated for 1-D signals
 * (included by vit_amd.h; conventions as stated there).
 *
 * What it stands for: HF `ViTForMaskedImageModeling` ("SimMIM: A Simple Framework for Masked Image Modeling").  A masked
 * patch's projected token is replaced by a learned `mask_token` [D] before the position embedding and the embedding dropout;
 * CLS stays; the encoder runs unchanged over all T = 1 + N rows; one Linear decodes token 1 + n into the P samples of window n:
 *     pred[b, n, :] = last[b, 1 + n, :] W_dec^T + b_dec                      (W_dec [P, D]; a vit_gemm, not declared here)
 * The reference's model has no such head: `model.task_type: mim` is this build's key.
 *
 * mask int32 [B, N]: non-zero = masked.  No kernel below forms an address from a mask value.
 * Masks are drawn in blocks of `span` consecutive patches: Nb = ceil(N / span) blocks, of which vit_patch_select(B, Nb, Kb)
 * keeps Kb = max(1, int(Nb * (1 - mask_ratio))) visible (the double-precision expression of patch dropout's K), and
 *     mask[b, n] = slot_blocks[b, n / span] < 0.
 * A short last block makes m = sum(mask) vary per sample: m is counted on the device.
 *
 * vit_mim_mask: the expansion above.  Nb must equal ceil(N / span), span >= 1.
 * vit_embed_finish_masked: vit_embed_finish over tokens [B, T, D] (T = N + 1) with
 *     row(b, t) = cls if t == 0;  mask_token if mask[b, t - 1];  tokens[b, t] otherwise
 *     tokens[b, t] = dropout(row(b, t) + pos[t])                              (pos [T, D] or NULL; mask keyed by row b * T + t)
 *   The projected token of a masked patch is not loaded.  With an all-zero mask it stores vit_embed_finish's bits.
 * vit_embed_finish_masked_bwd: with g[b, t] = dropout_multiplier(b, t) * dtokens[b, t]:
 *     dpatch[b * N + n] = mask[b, n] ? 0 : g[b, 1 + n]                        (bf16 / f32; masked rows are exact zeros)
 *     dmask_token = sum over masked (b, n) of g[b, 1 + n];  dcls = sum_b g[b, 0];  dpos[t] = sum_b g[b, t] (optional)
 *   Every sum is taken as vit_embed_finish_bwd takes its own: per (t, 4 columns) over min(B, 16) batch chunks in ascending b,
 *   then the deterministic reduce over the partial rows (for dmask_token: the chunks' T rows each, in row order) -- no float
 *   atomics, bit-identical from call to call, and dcls / dpos are vit_embed_finish_bwd's bit for bit when the mask is all
 *   zero.  `accumulate` (OR the handle's "grad_accumulate"): dcls / dpos / dmask_token store old + new.
 *   Workspace: 2 * min(B, 16) * T * D floats, claimed before the first launch.
 * vit_mim_loss_fwd: target window n of sample b is t[p] = x[b, n * S + p], p < P; a window that does not fit inside the signal
 *   is all zero (vit_unfold_cast's rule).  It is the signal as given: no gradient flows into it.  norm_target != 0 replaces it
 *   by (t - mean) / sqrt(var + 1e-6), mean and the UNBIASED var over the window's P samples (MAE's norm_pix_loss; needs P >= 2).
 *     m = #{mask != 0} (int32, to count_out);  loss = sum_{masked b, n} sum_p l(pred[b * T + 1 + n, p] - t[p]) / (max(1, m) * P)
 *   with l = |.| (VIT_LOSS_L1) or (.)^2 (VIT_LOSS_MSE); pred [B * T, P] f32 or bf16 (row b * T is the CLS row: ignored).
 *   One wave per window: a masked window reduces its P terms across the 64 lanes, an unmasked one loads nothing; the
 *   per-window partials go to the workspace (B * N floats) and a single-block second stage sums them and counts the mask in
 *   a fixed order.  With S == P and L1 this is HF's SimMIM loss without its 1e-5.  m == 0: loss 0.
 * vit_mim_loss_bwd: dpred [B * T, P] (bf16 / f32): CLS rows and rows of unmasked windows are exact zeros; a masked row holds
 *     sign(d) (L1; sign(0) = 0) or 2 d (MSE), times dloss[0] / (max(1, m) * P),  d = pred - t
 *   with t re-normalised in the kernel under norm_target, and m read from `count` (vit_mim_loss_fwd's count_out).
 * Bad arguments -- span < 1, T != N + 1, a kind other than L1 / MSE, P not a multiple of 4, a window start past the signal,
 * null pointers -- return VIT_ERR_ARG with a message and launch nothing. */
#ifndef VIT_AMD_MIM_H_
#define VIT_AMD_MIM_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_mim_mask(vit_handle h, const int32_t* slot_blocks, int32_t* mask, int B, int N, int Nb, int span, vit_stream stream);
int vit_embed_finish_masked(vit_handle h, float* tokens, const float* cls, const float* pos, const int32_t* mask,
                            const float* mask_token, int B, int T, int D, float dropout_p, uint64_t seed, uint64_t site,
                            vit_stream stream);
int vit_embed_finish_masked_bwd(vit_handle h, const float* dtokens, const int32_t* mask, void* dpatch_out, int dpatch_dtype,
                                float* dcls, float* dpos, float* dmask_token, int B, int T, int D, float dropout_p,
                                uint64_t seed, uint64_t site, int accumulate, vit_stream stream);
int vit_mim_loss_fwd(vit_handle h, const float* x, const void* pred, int pred_dtype, const int32_t* mask, float* loss_out,
                     int32_t* count_out, int B, int L, int P, int S, int N, int T, int kind, int norm_target,
                     vit_stream stream);
int vit_mim_loss_bwd(vit_handle h, const float* x, const void* pred, int pred_dtype, const int32_t* mask, const int32_t* count,
                     const float* dloss, void* dpred, int dpred_dtype, int B, int L, int P, int S, int N, int T, int kind,
                     int norm_target, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_MIM_H_ */
