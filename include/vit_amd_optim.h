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
 *   correct under a hipGraph although kernel arguments are frozen at capture.
 *
 * vit_lamb_step*: LAMB as timm's `Lamb` states it (the implementation DeiT-III trains with), the fused clip in the place of timm's
 *   max_grad_norm.  Here a SEGMENT IS ONE PARAMETER TENSOR together with its alignment pad (zero in every buffer): the trust
 *   ratio is a norm over exactly that tensor, so the segment table is the per-parameter one
 *   (vit_amd.functional.optim_param_tables), never the merged runs the other families may be given.  Per segment, with the
 *   call-wide clip as above:
 *     g' = g * clip
 *     m  = beta1 * m + (1 - beta1) * g'          v = beta2 * v + (1 - beta2) * g'^2
 *     u  = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps)   [+ weight_decay * p   if weight_decay != 0]
 *     adapt = (weight_decay != 0) or always_adapt
 *     r  = adapt and ||p|| > 0 and ||u|| > 0 ? ||p|| / ||u|| : 1        (L2 norms over the segment)
 *     r  = trust_clip ? min(r, 1) : r
 *     p -= lr * r * u;  p_bf16 = bf16(p)
 *   lr and weight_decay are the segment's group row's; beta1, beta2, eps, always_adapt, trust_clip and `step` (1-based) are
 *   call-wide; 1 - beta is 1.f - beta as in vit_adamw_step; g is only read.  Defaults of the Python layer: betas (0.9, 0.999),
 *   eps 1e-6, always_adapt and trust_clip off.
 *   Three launches per call, their dependencies kernel boundaries (no atomics, no block waits for another): (1) m and v are
 *   updated and every TILE writes one (sum p^2, sum u^2) pair into the handle's workspace; (2) one wave per segment sums its
 *   tiles' pairs in a fixed order and writes trust[s]; (3) u is recomputed from the stored m, v and the untouched p by the same
 *   device function -- bit for bit what entered the norm -- and p and the shadow are written.  42 B per parameter (24 + 18)
 *   against AdamW's 30; storing u instead would take 4 B of scratch per parameter.  Tiles are VIT_LAMB_TILE elements cut from
 *   each segment's start (the last one short; none straddles a segment), a function of the segment table alone -- not of the
 *   grid, of `base` or of a handle option -- and all sums are f64 in one fixed order: deterministic, and a call over a sub-run
 *   [base, base + n) of WHOLE segments gives on those segments the bits the whole-buffer call gives, trust[] included.  A run
 *   that cuts a segment is the caller's error (vit_amd.functional refuses it); the kernels then cut the segment to the run and
 *   still read nothing outside the run or the tables.  A segment whose group index is negative (a parameter no group owns,
 *   which the per-parameter table keeps as a segment of its own so that it enters no neighbour's norm) is neither read nor
 *   written, and neither is its trust entry.
 *   `trust`: f32, caller-owned, n_segments entries indexed by the table's segment number; the by-value form (one tensor = one
 *   segment, for parameters outside the flat buffer) takes one entry, or NULL.  Workspace: 16 + 16 B per tile slot,
 *   n / VIT_LAMB_TILE + n_segments + 1 slots (by value: ceil(n / VIT_LAMB_TILE)), stated through vit_workspace_needed.
 *   `_dyn`: bc1 and sqrt(bc2) from the bound record, as for the other families.
 *   VIT_ERR_ARG, before anything is launched: a NULL p, g, m, v or table; a NULL trust with a table; n <= 0; n_segments <= 0;
 *   n_groups <= 0; base < 0 or not a multiple of 4; step < 1; no record bound (`_dyn`). */
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

#define VIT_LAMB_TILE 4096 /* elements per tile of the LAMB norms, cut from each segment's start */

int vit_lamb_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int always_adapt, int trust_clip, int step, const float* sqnorm,
                  float max_norm, float* trust, vit_stream stream);
int vit_lamb_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                         const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                         float beta1, float beta2, float eps, int always_adapt, int trust_clip, int step, const float* sqnorm,
                         float max_norm, float* trust, vit_stream stream);
int vit_lamb_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                             const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                             int n_groups, float beta1, float beta2, float eps, int always_adapt, int trust_clip,
                             const float* sqnorm, float max_norm, float* trust, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_OPTIM_H_ */
