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
 *
 * Parameter groups (torch.optim's param_groups: no-decay sets, layer-wise learning rates) in ONE launch: vit_*_step_groups.
 *   The flat buffer alternates decaying and non-decaying parameters (8 runs per encoder layer), so a launch per run would be
 *   ~100 launches at ViT-B; instead one kernel walks the buffer once and looks up each element's lr / weight_decay / momentum.
 *   Two caller-owned tables in device memory, only ever READ by the step kernels:
 *     segment table: seg_end[n_segments], ascending end offsets in elements; segment s covers [seg_end[s-1], seg_end[s]) (from 0
 *       for s = 0) and belongs to group seg_group[s].  Every end is a multiple of 4 except the last, which may equal the buffer's
 *       length.  A segment may be as short as 8 elements; there is no cap on n_segments or n_groups.
 *     group table: groups[n_groups][VIT_OPTIM_GROUP_STRIDE] f32 rows {lr, weight_decay, momentum, 0}, 16-byte aligned; momentum
 *       is SGD's and is ignored by Adam.
 *   `base` is the absolute element offset of p[0] in the segment table's coordinates (a multiple of 4, as the 16-byte accesses
 *   need anyway): the call updates [base, base + n).  A sub-run of the buffer (the active runs when parameters are frozen, a
 *   rank's shard) gives the bits the whole-buffer call gives there, wherever it starts and ends.
 *   Arithmetic: the by-value entry point's, with the element's group's numbers in place of the scalar arguments -- on any
 *   segment bit-identical to that entry point called on the slice: each family is ONE kernel, and the by-value entry points
 *   launch it without tables, their scalars as its only row.  Without tables, or with a table of one segment, the row is taken
 *   once per kernel and the loop is the plain grid-stride loop: a one-group optimizer is a one-row table at no cost.
 *   beta1, beta2, eps, nesterov, `step` and the clip coefficient stay call-wide.  vit_sgd_step_groups: a group whose momentum is 0 neither reads nor writes its part of buf
 *   (vit_sgd_step with momentum 0); buf == NULL is the momentum-free update whatever the table holds.  No atomics,
 *   deterministic.  Offsets past the last end count to the last segment and a group index past the table to the last group,
 *   so a malformed table cannot make a kernel read outside the tables; beyond that the tables' contents are the caller's job
 *   (vit_amd.functional.optim_group_tables checks them where they are built).
 *   The `_dyn` forms (a captured step, vit_step_state_bind) take the bias corrections, and nothing else, from the bound record;
 *   learning rates and momenta come from the group table in both forms (vit_sgd_step_groups_dyn only insists on the bound
 *   record).  They are the only forms for a captured step, for one group or many.
 *   VIT_ERR_ARG, before anything is launched: a NULL p, g, state buffer or table; n <= 0; n_segments <= 0; n_groups <= 0;
 *   base < 0 or not a multiple of 4; step < 1; nesterov with buf == NULL; no record bound (`_dyn`).
 * vit_optim_groups_write: writes groups[0 .. n_groups) from `values`, n_groups HOST rows of {lr, weight_decay, momentum}.  The
 *   numbers travel by value in kernel arguments (64 rows per launch) and are stored with 16-byte vector stores, so there is no
 *   staging buffer the host could overwrite under a running step.  The caller launches it only when a scheduler changed a
 *   number, ahead of the step -- or ahead of the replay of a captured step -- on the same stream: per-step schedules stay
 *   correct under a hipGraph although kernel arguments are frozen at capture. */
#ifndef VIT_AMD_OPTIM_H_
#define VIT_AMD_OPTIM_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_sgd_step(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, float lr, float momentum,
                 float weight_decay, int nesterov, const float* sqnorm, float max_norm, vit_stream stream);
int vit_adam_l2_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                     float max_norm, vit_stream stream);

#define VIT_OPTIM_GROUP_STRIDE 4 /* f32 per group-table row: lr, weight_decay, momentum, 0 */

int vit_adamw_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                          const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                          float beta1, float beta2, float eps, int step, const float* sqnorm, float max_norm,
                          vit_stream stream);
int vit_adamw_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                              int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                              const float* groups, int n_groups, float beta1, float beta2, float eps, const float* sqnorm,
                              float max_norm, vit_stream stream);
int vit_adam_l2_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                            const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                            int n_groups, float beta1, float beta2, float eps, int step, const float* sqnorm, float max_norm,
                            vit_stream stream);
int vit_adam_l2_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                                int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                                const float* groups, int n_groups, float beta1, float beta2, float eps, const float* sqnorm,
                                float max_norm, vit_stream stream);
int vit_sgd_step_groups(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, int64_t base,
                        const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                        int nesterov, const float* sqnorm, float max_norm, vit_stream stream);
int vit_sgd_step_groups_dyn(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, int64_t base,
                            const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                            int n_groups, int nesterov, const float* sqnorm, float max_norm, vit_stream stream);
int vit_optim_groups_write(vit_handle h, float* groups, int n_groups, const float* values, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_OPTIM_H_ */
