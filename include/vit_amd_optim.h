/* vit_amd_optim.h -- optimizer steps of libvit_amd.so beside vit_adamw_step (included by vit_amd.h; conventions as stated there).
 *
 * The reference builds its optimizer as torch.optim.<type>(model.parameters(), lr=, weight_decay=) (src/opt/optimizer.py:14-26,108)
 * and documents three choices of `opt.type`: 'Adam', 'AdamW', 'SGD' (configs/config.yaml).  vit_adamw_step (vit_amd.h) is AdamW;
 * here are the other two, in the same form: one pass over a flat f32 parameter buffer, the clip coefficient
 * min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) applied to g on the fly (sqnorm may be NULL: no clipping), the bf16 shadow of p written
 * in the same pass (p_bf16 may be NULL), no atomics, deterministic.  Clipping comes first, as Lightning clips .grad before
 * optimizer.step().
 *
 * vit_sgd_step: torch.optim.SGD, single-tensor form, maximize = False, dampening = 0:
 *     g' = g * clip + weight_decay * p
 *     momentum != 0:  buf = momentum * buf + g';  d = nesterov ? g' + momentum * buf : buf
 *     momentum == 0:  d = g'   (buf is neither read nor written and may be NULL)
 *     p -= lr * d;  p_bf16 = bf16(p)
 *   A zero-filled buf reproduces torch's first step (buf = clone(g')) exactly, so there is no first-step flag.  Moves 14 B per
 *   parameter without momentum, 22 B with it (shadow included).  VIT_ERR_ARG: p or g NULL, n <= 0, momentum < 0, momentum != 0
 *   (or nesterov) with buf == NULL.
 * vit_adam_l2_step: torch.optim.Adam with weight_decay as L2 in the gradient: g' = g * clip + weight_decay * p, no decoupled
 *   decay, otherwise vit_adamw_step's arithmetic and arguments (`step` is 1-based; VIT_ERR_ARG below 1) -- with one difference:
 *   the moments' weights 1 - beta are torch's.  torch's caller holds the betas as doubles and torch rounds 1 - beta to f32
 *   after the subtraction (float(1 - 0.999) = 0.001f; 1.f - 0.999f = 0.00099998713 would leave exp_avg_sq 1.3e-5 off).  The
 *   f32 arguments have lost those bits, so each beta is read back as the shortest decimal that names it (0.999f -> 0.999),
 *   which is the caller's own number for any beta of up to 7 significant digits.  vit_adamw_step keeps 1.f - beta.
 * vit_sgd_step_dyn / vit_adam_l2_step_dyn: the forms for a captured step (vit_step_state_bind): lr and momentum, or lr and the
 *   bias corrections, are read from the bound record at kernel entry.  vit_sgd_step_dyn with buf == NULL is the momentum-free
 *   update whatever the record holds.  VIT_ERR_ARG when no record is bound. */
#ifndef VIT_AMD_OPTIM_H_
#define VIT_AMD_OPTIM_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_sgd_step(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, float lr, float momentum,
                 float weight_decay, int nesterov, const float* sqnorm, float max_norm, vit_stream stream);
int vit_sgd_step_dyn(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, float weight_decay,
                     int nesterov, const float* sqnorm, float max_norm, vit_stream stream);
int vit_adam_l2_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                     float max_norm, vit_stream stream);
int vit_adam_l2_step_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float beta1,
                         float beta2, float eps, float weight_decay, const float* sqnorm, float max_norm,
                         vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_OPTIM_H_ */
