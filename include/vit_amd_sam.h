/* vit_amd_sam.h -- sharpness-aware minimisation (SAM, Foret et al. 2021; the adaptive form ASAM, Kwon et al. 2021) as streaming
 * passes over the flat f32 parameter buffer (included by vit_amd.h; conventions as stated there).
 *
 * One optimisation step with `train.sam_rho` runs forward + backward twice on the same batch with the same random draws: at the
 * weights w (gradient g), then at the perturbed weights
 *     plain:     w'_i = w_i + rho * g_i / (||g|| + 1e-12)
 *     adaptive:  w'_i = w_i + rho * w_i^2 * g_i / (|| |w| (.) g || + 1e-12)
 * (the formulas of the widely used davda54/sam: e_w = (w^2 if adaptive else 1) * g * rho / (grad_norm + 1e-12), grad_norm the
 * L2 norm of (|w| if adaptive else 1) * g over every perturbed element), after which w is restored bit for bit and the optimizer
 * steps with the second gradient.  The three entry points below are the norm, the ascent and the descent.  All kernels: 16 bytes
 * per lane, grid-stride, scalar tail for n & 3, no atomics, deterministic; a call on a 16-byte-aligned slice gives there the bits
 * the whole-buffer call gives, so the caller may cover the perturbed runs of the buffer one by one.
 *
 * vit_sam_sqnorm: out[0] = sum_i (a_i g_i)^2 over i in [0, n), a_i = |p_i| if `adaptive` else 1; `accumulate` != 0 adds to out[0]
 *   instead (the runs of a buffer in ascending order).  Deterministic two-stage reduction through the handle's workspace.  With
 *   adaptive == 0, p is not read (may be NULL) and the result has the bits of vit_grad_sqnorm / vit_grad_sqnorm_acc: the same two
 *   launches.  Reads 4 B per parameter, 8 B in the adaptive form.
 * vit_sam_ascend: for i in [0, n): backup[i] = p[i]; p[i] = p[i] + (c_i g_i) s, one fused multiply-add, with c_i = p[i]^2 if
 *   `adaptive` else 1 and s = rho / (sqrtf(sqnorm_dev[0]) + 1e-12f).  sqnorm_dev is DEVICE memory (one f32, what vit_sam_sqnorm
 *   wrote): there is no host synchronisation, and inside a captured step the frozen argument is an address whose content is the
 *   replay's own.  p_bf16[i] = bf16(the new p[i]) in the same pass (may be NULL: f32 mode; the rounding is vit_cast_f32_bf16's and
 *   the step kernels').  An element with c_i g_i == 0 keeps every bit of p[i], so a zero gradient leaves p unchanged.
 *   Non-finite norm: sqnorm = +Inf gives s = 0 and every finite g_i leaves p[i] unchanged (an infinite g_i gives NaN);
 *   sqnorm = NaN gives s = NaN and every perturbed p[i] with c_i g_i != 0 becomes NaN -- for the second pass only: backup holds
 *   the finite weights and vit_sam_descend restores them, so the step ends with a NaN gradient, which the optimizer's clip
 *   coefficient then meets exactly as it meets one from a plain step.
 *   Moves 16 (+2) B per parameter (reads p and g, writes backup and p, and the shadow): the bytes of vit_ema_swap.
 * vit_sam_descend: p[i] = backup[i], p_bf16[i] = bf16(backup[i]) for i in [0, n).  Moves 8 (+2) B per parameter.  After
 *   vit_sam_ascend then vit_sam_descend over the same run, p holds its earlier bits (NaN payloads, infinities and -0.0
 *   included: the copy is bitwise), and p_bf16 its earlier bits provided it was bf16(p) before.
 * VIT_ERR_ARG, before anything is launched: a NULL p (where it is read), g, backup, out or sqnorm_dev; n <= 0; p, g or backup not
 *   16-byte aligned (p_bf16 not 8-byte, out / sqnorm_dev not 4-byte aligned); rho not finite or <= 0. */
#ifndef VIT_AMD_SAM_H_
#define VIT_AMD_SAM_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_sam_sqnorm(vit_handle h, const float* p, const float* g, int64_t n, int adaptive, int accumulate, float* out,
                   vit_stream stream);
int vit_sam_ascend(vit_handle h, float* p, const float* g, float* backup, void* p_bf16, int64_t n, float rho, int adaptive,
                   const float* sqnorm_dev, vit_stream stream);
int vit_sam_descend(vit_handle h, float* p, const float* backup, void* p_bf16, int64_t n, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_SAM_H_ */
