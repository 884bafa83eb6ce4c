/* vit_amd_cov.h -- covariance statistics entry points of libvit_amd.so (included by vit_amd.h; conventions as stated there).
 *
 * The statistics file behind `warmup.cov_path` (mean / cov / eigvals / eigvecs of the training spectra): the reference's
 * compute_covariance_stats (src/prepca/preprocessor_utils.py:399-475: `mean = data.mean(0)`, `centered = data - mean`,
 * `cov = centered.t().matmul(centered) / (n - 1)`, then _sorted_eigh_sym :44-62, which stays on the host).
 *
 * vit_cov_accumulate: acc[L, L] (f32, dense, ld = L) += (x - mean)^T (x - mean) over the n rows of x (f32, row stride
 * ldx >= L), on exact-f32 MFMA (v_mfma_f32_32x32x2_f32, f32 accumulate: bit for bit a k-ordered fmaf chain -- not the
 * split-bf16 x3 products of vit_gemm's VIT_F32 mode, whose 2^-16 relative error is above the tail eigenvalues a ZCA front
 * divides by).  The centring is fused on the operand load; only the 128 x 128 tiles on or above the diagonal are computed,
 * everything of acc below them is left untouched.  Any n >= 1, L >= 1 (ragged edges are masked inside); x and mean need no
 * alignment (16-byte aligned x with ldx % 4 == 0 and L % 4 == 0 takes the vector loads).  Below 2048 tiles the rows are split into slices
 * through the workspace and reduced in slice order; the plan is a function of (n, L) alone and there are no floating-point
 * atomics: the result is a deterministic function of (x, mean, n, L).  Call once per row chunk of a split larger than
 * memory; mean is the mean over ALL rows (vit_colsum(..., accumulate) per chunk, then vit_cov_mean_finish).
 * vit_cov_mean_finish: colsum[L] /= n_total, in place.
 * vit_cov_finish: cov[i][j] = cov[j][i] = acc[min(i, j)][max(i, j)] / (n_total - 1): the lower triangle is mirrored from the
 * upper, so cov is bitwise symmetric (what the reference's 0.5 * (cov + cov^T) amounts to).  cov must not alias acc. */
#ifndef VIT_AMD_COV_H_
#define VIT_AMD_COV_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_cov_accumulate(vit_handle h, const float* x, int64_t ldx, const float* mean, float* acc, int n, int L,
                       vit_stream stream);
int vit_cov_mean_finish(vit_handle h, float* colsum, int L, int64_t n_total, vit_stream stream);
int vit_cov_finish(vit_handle h, const float* acc, float* cov, int L, int64_t n_total, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_COV_H_ */
