/* vit_amd_mix.h -- Mixup / CutMix of a batch of spectra and of its labels, on the GPU (included by vit_amd.h; conventions as
 * stated there).
 *
 * The semantics are timm's `Mixup` (timm/data/mixup.py) restated for a 1-D signal: Mixup is a convex combination of two
 * spectra, CutMix replaces a contiguous wavelength span, regression labels mix linearly and class labels become soft targets
 * (optionally label-smoothed).  The partner of sample b in a batch of B is p = B - 1 - b (timm's x.flip(0)).  What is mixed is
 * decided on the host (vit_amd/mix.py) and reaches the kernels as a PLAN: one row per sample, or one row for the whole batch,
 *
 *     vit_mix_row { f32 w, u;  i32 lo, hi;  f32 wy, uy;  i32 reserved[2] }      32 bytes
 *
 *     out[b, i] = x[p, i]                         if lo <= i < hi              (bit copy)
 *               = x[b, i]                         else if u == 0 or p == b     (bit copy; x[p] is NOT read for it)
 *               = fma(w, x[b, i], u * x[p, i])    otherwise                    (f32: one product rounded, one fused multiply-add)
 *     regression labels  yout[b, :] = fma(wy, y[b, :], uy * y[p, :])           (uy == 0: bit copy of y[b, :])
 *     class labels       tout[b, c] = fma(wy, oh(y[b])[c], uy * oh(y[p])[c])   (uy == 0: oh(y[b])[c] itself)
 *                        oh(k)[c] = (c == k ? on : off);  off = s / C, on = 1 - s + off for label smoothing s, formed in double
 *                        by the caller and rounded once.  A label outside [0, C) selects no `on` entry (nothing is indexed by it).
 *   The identity row is {1, 0, 0, 0, 1, 0}; with s > 0 it is plain label smoothing.  lo / hi are clamped to [0, L] in the kernel:
 *   whatever a plan holds, no row is read or written outside the tensor.  The reserved words are neither read nor interpreted.
 *
 * vit_mix_plan_write: rows [0, n_rows) of the device plan <- host_rows.  The rows travel BY VALUE in kernel arguments, 64 per
 *   launch, and are stored with two 16-byte vector stores each: vit_optim_groups_write's pattern -- there is no staging buffer
 *   the host could overwrite under a running step, and the write is ordered on `stream` like every other launch.
 * vit_mix_signal: x, out: f32 [B, L]; n_rows = 1 (every sample uses row 0) or B (row b for sample b).
 *   out == x is the in-place form, any other out must not overlap x (the copy form).  One work item owns elements [i, i + 4) of
 *   BOTH rows of a pair (b, p) and loads what it needs of both before it stores either, so the in-place form has no hazard and
 *   the copy form reads every element of x once.  16 bytes per lane for any L: the vectors of a pair are laid on the 16-byte
 *   grid of row b (its up to 3 + 3 edge elements go one by one), row p is accessed at that offset with 4-byte-aligned 16-byte
 *   accesses.  Whether a 256-element chunk of a row needs its partner's chunk -- it is mixed, or its span reaches into the chunk
 *   -- is decided per wave from the plan alone (wave-uniform).  No atomics; deterministic.
 *   Bytes moved, copy form: 2 x B x L x 4, those of the plain copy it replaces, whatever the plan holds.  In place: 4 x L x 4
 *   per pair with a Mixup row (both rows read and written), 4 x span x 4 (to the chunk) per CutMix pair, nothing for a pair of
 *   identity rows.
 * vit_mix_targets: label_kind VIT_MIX_LABELS_F32: labels f32 [B, C] (regression, C = the number of targets; on / off ignored),
 *   VIT_MIX_LABELS_I64: labels int64 [B] (classes); out: f32 [B, C], not overlapping labels.
 * VIT_ERR_ARG, before anything is launched: a null pointer; n_rows <= 0 (plan_write) or not in {1, B}; B <= 0, L <= 0, C <= 0;
 *   plan_dev, x or out not 16-byte aligned (labels: their element size); x and out overlapping partially (out and labels at
 *   all); an unknown label_kind; a non-finite on / off with class labels.
 *
 * The soft-target kinds of vit_loss that the mixed class targets need -- VIT_LOSS_SOFT_CE, VIT_LOSS_BCE: labels are f32 [B, C]
 * targets t -- are described at vit_head_loss_fwd in vit_amd.h. */
#ifndef VIT_AMD_MIX_H_
#define VIT_AMD_MIX_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vit_mix_row {
  float w, u;       /* signal: weight of the sample itself / of its partner outside the span (u == 0: plain copy) */
  int32_t lo, hi;   /* signal: elements [lo, hi) are the partner's (CutMix); lo >= hi: no span */
  float wy, uy;     /* labels: weight of the sample's own label / of its partner's */
  int32_t reserved[2];
} vit_mix_row;

typedef enum { VIT_MIX_LABELS_F32 = 0, VIT_MIX_LABELS_I64 = 1 } vit_mix_labels;

int vit_mix_plan_write(vit_handle h, void* plan_dev, int n_rows, const vit_mix_row* host_rows, vit_stream stream);
int vit_mix_signal(vit_handle h, const float* x, float* out, const void* plan_dev, int n_rows, int B, int L,
                   vit_stream stream);
int vit_mix_targets(vit_handle h, const void* labels, int label_kind, float* out, const void* plan_dev, int n_rows, int B,
                    int C, float on, float off, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_MIX_H_ */
