/* vit_amd_muon.h -- the Muon optimizer's kernels of libvit_amd.so (includes vit_amd.h, never the reverse: these entry points are
 * bound from their own table, vit_amd._cabi._PROTOS_MUON; conventions as stated in vit_amd.h).
 *
 * Muon (torch.optim.Muon, torch 2.10) keeps SGD momentum for a weight MATRIX and applies only its orthogonalisation, a quintic
 * Newton-Schulz iteration run in bf16.  For every Muon matrix W [rows, cols] with gradient g, f32 momentum buffer buf and the
 * call-wide clip coefficient min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) (sqnorm may be NULL: no clipping; Lightning clips before
 * the step):
 *     g'  = g * clip
 *     buf = buf + (1 - momentum) * (g' - buf)              (torch's lerp_, f32; 1 - momentum formed in double, rounded to f32)
 *     u   = nesterov ? g' + momentum * (buf - g') : buf    (f32, one fma)
 *     X0  = bf16(u), transposed if rows > cols  ->  [m, n] with m <= n
 *     X0  = bf16(X0 * (1 / max(||X0||_F, eps)))            (the norm: f64 sums of the bf16 values' squares in one fixed order,
 *                                                            as LAMB's; the reciprocal rounded once to f32)
 *     repeat ns_steps times (a, b, c = ns_coefficients):
 *         A = bf16(X X^T)                 f32 accumulate
 *         B = bf16(b*A + c*(A A))         f32 accumulate, one rounding      (A A is computed as A A^T: A is symmetric bit for bit,
 *                                                                            both halves sum the same products in the same order)
 *         X = bf16(a*X + B X)             f32 accumulate, one rounding
 *     O   = X, transposed back
 *     W   = fma(-(lr * ratio), O, W * fma(-lr, weight_decay, 1));  shadow = bf16(W)
 *   ratio is torch's _adjust_lr, a per-matrix constant the host builds: 'original' sqrt(max(1, rows / cols)), 'match_rms_adamw'
 *   0.2 * sqrt(max(rows, cols)), 'none' 1.  lr and weight_decay are the matrix's group row's (vit_amd_optim.h's group table,
 *   {lr, weight_decay, momentum, 0}; the row's momentum is not read here).
 *
 * Two device tables, caller-owned and only ever READ:
 *   vit_muon_mat[n_mats]: one entry per matrix, ascending in tile0 and ttile0.  `off`: the element offset of W in the flat buffers
 *     (p, g, the bf16 shadow); `xoff`: the element offset of the matrix in the compact buffers (buf, and the bf16 workspaces u / x);
 *     both multiples of 8.  rows and cols are multiples of 16, at least 16.  `tile0`: the number of streaming tiles
 *     (VIT_MUON_TILE elements, cut from each matrix's start, the last one short) of the matrices in front; `ttile0`: likewise of
 *     32 x 32 transposing tiles, ceil(rows / 32) * ceil(cols / 32) per matrix.  A matrix that is frozen is simply not in the table:
 *     neither it nor its buffer is read or written.
 *   vit_muon_problem[n_problems] + tiles[n_tiles] (int32 x 4: problem, tile row, tile column, 0) for vit_muon_gemm_grouped.
 *
 * vit_muon_momentum: buf and u (bf16, [rows, cols] as W lies) are written, and every streaming tile writes its f64 sum of
 *   bf16(u)^2 to part[tile]; n_tiles = the table's total.  g is only read.
 * vit_muon_norms: one wave per matrix sums its tiles' partials in a fixed order; norms[i] = ||X0||_F (f32, for reporting) and
 *   inv_norm[i] = 1 / max(norm, eps).
 * vit_muon_normalize: x (bf16, [m, n], m <= n) = bf16(u * inv_norm), transposed when rows > cols; n_ttiles = the table's total.
 * vit_muon_gemm_grouped: C_i = bf16(alpha_i * A_i op(B_i) + beta_i * R_i) for every problem of the table in ONE launch,
 *   v_mfma_f32_16x16x32_bf16 with f32 accumulation, operands staged through the LDS.  All four matrices bf16, row-major with
 *   leading dimensions lda / ldb / ldr / ldc (elements, multiples of 8; pointers 16-byte aligned); A is [m, k].  b_trans != 0:
 *   op(B) = B^T with B [n, k], both operands K-contiguous (X X^T, and A A through A's symmetry); b_trans == 0: B is [k, n],
 *   strided along K (B X).  m, n, k are multiples of 16, at least 16; a workgroup computes one VIT_MUON_GEMM_TILE-square tile of
 *   one C_i, edge tiles cut to the matrix.  beta_i == 0: R_i is not read and may be NULL.  C_i must not alias an operand of any
 *   problem of the launch (X therefore ping-pongs between two buffers).  Every element of every C_i is written, nothing else.
 * vit_muon_apply: W and (p_bf16 != NULL) the shadow from o (bf16, [m, n] as the iteration left it), transposing back.
 * One Newton-Schulz iteration is three vit_muon_gemm_grouped launches for the whole model; a step is 4 + 3 * ns_steps launches.
 * No atomics, no host synchronisation, deterministic; every scale lives in device memory, so a step is capturable as it is.
 * VIT_ERR_ARG, before anything is launched: a NULL pointer (p_bf16, sqnorm and a problem's R excepted), a count <= 0,
 * momentum outside [0, 1), eps <= 0. */
#ifndef VIT_AMD_MUON_H_
#define VIT_AMD_MUON_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIT_MUON_TILE 4096     /* elements per streaming tile of the norm's partial sums */
#define VIT_MUON_GEMM_TILE 64  /* rows and columns of C per workgroup of the grouped product */

typedef struct vit_muon_mat { /* 48 bytes */
  int64_t off, xoff;
  int32_t rows, cols;
  int32_t group;
  float ratio;
  int32_t tile0, ttile0;
  int64_t reserved;
} vit_muon_mat;

typedef struct vit_muon_problem { /* 72 bytes */
  const void* A;
  const void* B;
  const void* R;
  void* C;
  int32_t m, n, k;
  int32_t lda, ldb, ldr, ldc;
  float alpha, beta;
  int32_t reserved;
} vit_muon_problem;

int vit_muon_momentum(vit_handle h, const float* g, float* buf, void* u, const vit_muon_mat* mats, int n_mats, int n_tiles,
                      double momentum, int nesterov, const float* sqnorm, float max_norm, double* part, vit_stream stream);
int vit_muon_norms(vit_handle h, const vit_muon_mat* mats, int n_mats, const double* part, float eps, float* inv_norm,
                   float* norms, vit_stream stream);
int vit_muon_normalize(vit_handle h, const void* u, void* x, const vit_muon_mat* mats, int n_mats, int n_ttiles,
                       const float* inv_norm, vit_stream stream);
int vit_muon_gemm_grouped(vit_handle h, const vit_muon_problem* problems, int n_problems, const int32_t* tiles, int n_tiles,
                          int b_trans, vit_stream stream);
int vit_muon_apply(vit_handle h, float* p, void* p_bf16, const void* o, const vit_muon_mat* mats, int n_mats, int n_ttiles,
                   const float* groups, int n_groups, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_MUON_H_ */
