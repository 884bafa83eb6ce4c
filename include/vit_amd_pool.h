/* vit_amd_pool.h -- global average pooling of the token rows (`model.global_pool: avg`; included by vit_amd.h; conventions as
 * stated there).
 *
 * What it stands for: timm's `global_pool='avg', fc_norm=False` and big_vision's plain-ViT head -- the classifier reads the
 * mean of the patch tokens of the final LayerNorm's output instead of its CLS row:
 *     logits = head(mean_{t = first .. T-1} LayerNorm_final(x_L)[b, t, :])          (first = 1 in the engine: CLS excluded)
 * The reference's model has no such head: `model.global_pool` is this build's key.
 *
 * vit_token_pool_fwd: x f32 [B, T, D] contiguous, pooled f32 [B, D] contiguous, n = T - first:
 *     pooled[b, d] = (sum_{t = first}^{T-1} x[b, t, d]) * inv,   inv = (float)(1.0 / (double)n)   (numpy: np.float32(1 / n))
 *   THE ORDER OF THE SUM, a function of (T, first) alone -- not of B, D, the grid or the number of compute units: with
 *   W = min(8, n), partial w (0 <= w < W) takes the rows t = first + w, first + w + 8, first + w + 16, ... in ascending order,
 *       p_w = (..((x[first + w] + x[first + w + 8]) + x[first + w + 16]) + ..)           (f32 adds; p_w STARTS as its first row)
 *   and the partials are combined in ascending w,
 *       pooled = ((..((p_0 + p_1) + p_2) + ..) + p_{W-1}) * inv                          (f32 adds, one f32 multiply)
 *   One workgroup of 8 waves serves a (sample, 256-column chunk) pair (64 columns where D is no multiple of 4): wave w forms
 *   p_w in registers, the partials meet in the LDS, wave 0 adds them in the order above and stores.  No atomics, no workspace:
 *   the result is bit-identical from call to call.
 * vit_token_pool_bwd: dpooled f32 [B, D], dx f32 [B, T, D], both contiguous:
 *     dx[b, t, :] = t < first ? 0 : dpooled[b, :] * inv                                  (the same inv; one f32 multiply)
 *   EVERY element of dx is written, the exact zeros of the rows t < first included; nothing is accumulated.
 * Both: 16-byte accesses where D % 4 == 0 (every row is then 16-byte aligned, given 16-byte aligned base pointers), a scalar
 * path otherwise.  Neither touches the handle's workspace.
 * Bad arguments -- a null pointer, B, T or D < 1, first outside [0, T) -- return VIT_ERR_ARG with a message and launch
 * nothing. */
#ifndef VIT_AMD_POOL_H_
#define VIT_AMD_POOL_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_token_pool_fwd(vit_handle h, const float* x, float* pooled, int B, int T, int D, int first, vit_stream stream);
int vit_token_pool_bwd(vit_handle h, const float* dpooled, float* dx, int B, int T, int D, int first, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_POOL_H_ */
