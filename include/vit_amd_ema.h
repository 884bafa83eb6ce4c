/* vit_amd_ema.h -- exponential moving average of the weights, kept on the GPU (included by vit_amd.h; conventions as stated
 * there).
 *
 * The averaging is torch.optim.swa_utils.AveragedModel's with get_ema_multi_avg_fn(decay): after an optimizer step,
 * ema <- torch.lerp(ema, p, 1 - decay), and the first update copies p.  The trainer keeps one flat f32 buffer shaped like the
 * flat parameter buffer, so the average is one more streaming pass behind the optimizer step (a launch of its own: the step
 * kernels and their entry points are untouched), rides in a captured step, and is evaluated by exchanging the two buffers in
 * place.  Both kernels: 16 bytes per lane, grid-stride, scalar tail for n & 3, no atomics, deterministic; a call on a
 * 16-byte-aligned slice gives there the bits the whole-buffer call gives.
 *
 * vit_ema_update: ema[i] <- lerp(ema[i], p[i], w) for i in [0, n):
 *     w <  0.5:  ema + w * (p - ema)
 *     w >= 0.5:  p - (p - ema) * (1 - w)
 *   each line one subtraction and one fused multiply-add.  `weight` is w = 1 - decay, ALREADY SUBTRACTED: the caller forms
 *   1 - decay in double and rounds once, as torch does (float(1 - 0.999) = 0.001f where 1.f - 0.999f = 0.00099998713; see the
 *   same note on Adam's betas in vit_amd_optim.h).  w == 1 (the first update) is a plain copy, bit for bit, and does not read
 *   ema.  w == 0 (a step the averaging schedule skips) leaves every bit of ema alone: the kernel returns before it loads
 *   anything.  p == ema gives ema in both branches, so a frozen parameter averages to itself.
 *   weight_dev != NULL: w is read from device memory instead (one f32, 16-byte aligned, only ever read) and `weight` is
 *   ignored.  This is the form for a step captured as a hipGraph, whose kernel arguments are frozen: the host rewrites the
 *   value ahead of a replay with a by-value kernel write on the same stream -- vit_optim_groups_write on a one-row table is
 *   such a write -- so there is no staging buffer the host could overwrite under a running step.
 *   Moves 12 B per parameter (reads p, reads and writes ema); 8 B for w == 1, nothing for w == 0.
 * vit_ema_swap: exchanges p[i] and ema[i] for i in [0, n) and writes p_bf16[i] = bf16(the new p[i]) in the same pass (p_bf16 may
 *   be NULL; the rounding is vit_cast_f32_bf16's and the step kernels').  Data moves, addresses stay.  A second call restores
 *   all three buffers bit for bit.  Moves 16 (+2) B per parameter.
 * VIT_ERR_ARG, before anything is launched: ema or p NULL; n <= 0; ema or p not 16-byte aligned (p_bf16 not 8-byte aligned;
 *   weight_dev not 16-byte aligned); a by-value weight outside [0, 1] or not finite. */
#ifndef VIT_AMD_EMA_H_
#define VIT_AMD_EMA_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_ema_update(vit_handle h, float* ema, const float* p, int64_t n, float weight, const float* weight_dev,
                   vit_stream stream);
int vit_ema_swap(vit_handle h, float* p, float* ema, void* p_bf16, int64_t n, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_EMA_H_ */
