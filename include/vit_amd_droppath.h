/* vit_amd_droppath.h -- stochastic depth ("drop path"): a per-sample gate on each residual branch (included by vit_amd.h;
 * conventions as stated there).
 *
 * What it stands for: timm.layers.DropPath(p, scale_by_keep=True) = torchvision.ops.StochasticDepth(p, mode="row") around the
 * attention branch and around the MLP branch of an encoder layer, as DeiT / BEiT-style ViT training applies it (HF
 * BeitLayer.drop_path) with the rate growing linearly with depth.  The reference's HF ViTLayer has no such module:
 * `model.drop_path_rate` is this build's key and its default 0 is the reference's arithmetic.  For layer i, sample b:
 *     x1 = x  + m(b, i, 0) * dropout(ctx Wo^T + bo)
 *     x2 = x1 + m(b, i, 1) * dropout(g W2^T + b2)
 * m = 0 with probability p_i, 1 / (1 - p_i) otherwise, one value for all token rows of the sample, the two branches drawn
 * independently.
 *
 * Where it lives: both sums are formed by vit_layernorm_fwd_residual(_rows) and differentiated by vit_layernorm_bwd_rows, HBM-bound
 * row kernels in which one wave owns one row; the sample index, the draw and the row's multiplier are wave-uniform and are kept
 * in scalar registers.  The GEMMs, their descriptor and the attention kernels do not know about the gate.
 *
 * The draw reuses the dropout machinery (vit_amd/csrc/common.h; host restatement: oracle/dropmask.py drop_cfg, drop_hash):
 *     (thr, scale, k0, k1) = make_drop(path_p, seed, path_site);  a bound per-step record (vit_step_state_bind) XORs its keys
 *         into (k0, k1) when thr != 0, so a captured hipGraph draws a fresh gate on every replay, as for dropout;
 *     r16 = drop_hash(k0, k1, 2 * b + branch) & 0xFFFF;  the branch is kept iff r16 >= thr;  kept branches are scaled by
 *         scale = 65536 / (65536 - thr)  (thr = round(path_p * 65536): exactly unbiased, not exactly 1 / (1 - path_p));
 *     b = original_row / rows_per_sample.  Forward: the original row of compact row r is r * x_row_stride.  Backward: the row
 *         index of the full row space that the pass walks anyway (row_stride > 1: only its multiples exist).  The CLS rows
 *         (stride T, rows_per_sample T) therefore draw what the pass over all token rows draws.
 * The engine passes seed = the step's seed (shared with the layer's dropout sites), path_site = 4 + 4 * layer -- the slot of
 * each layer's four that dropout leaves free -- rows_per_sample = T, branch 0 for the attention branch, 1 for the MLP branch.
 * The CLS tail's second forward sum reads a compact stream of one row per sample (x_row_stride 1): rows_per_sample = 1 there.
 *
 * vit_layernorm_fwd_residual_path: vit_layernorm_fwd_residual_rows with the gate.  A row of a kept sample computes
 *   xsum = x + scale * delta (one fused multiply-add per element); a row of a dropped sample computes xsum = x and its delta
 *   is NOT READ (it may hold anything).  Statistics, normalisation and outputs behind xsum are those of vit_layernorm_fwd on it.
 * vit_layernorm_bwd_path: vit_layernorm_bwd_rows (fused form: dyn and dbias are required) with the gate on what it emits
 *   for the Linear underneath the sum: dyn = dx * k * dropout_mask, k ONE f32 per row: drop_scale * path_scale (the product
 *   rounded once; drop_scale = 1 with dropout_p = 0) for a kept sample, 0 for a dropped one.  dx, dgamma and dbeta are the
 *   plain form's bit for bit; dbias sums what was stored.  Rows of dropped samples are walked like any other, so the order of
 *   the partial sums -- and with it the "CLS rows give the full pass's bits" property of row_stride > 1 -- is unchanged.
 * path_p = 0 (thr = 0) launches the plain kernels: the bits and the launches of the _rows forms.
 * VIT_ERR_ARG, before anything is launched: a NULL pointer (dyn and dbias included); path_p outside [0, 1);
 *   rows_per_sample <= 0; branch not 0 or 1; the stride errors of the _rows forms; forward: rows * x_row_stride >= 2^31. */
#ifndef VIT_AMD_DROPPATH_H_
#define VIT_AMD_DROPPATH_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_layernorm_fwd_residual_path(vit_handle h, const float* x, int64_t x_row_stride, const void* delta, int delta_dtype,
                                    float* xsum, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                                    float* rstd, int rows, int D, float eps, float path_p, uint64_t seed, uint64_t path_site,
                                    int rows_per_sample, int branch, vit_stream stream);
int vit_layernorm_bwd_path(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const float* dres, int64_t dres_row_stride, float* dx, float* dgamma,
                           float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, float dropout_p,
                           uint64_t seed, uint64_t site, int64_t row_stride, float path_p, uint64_t path_site,
                           int rows_per_sample, int branch, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_DROPPATH_H_ */
