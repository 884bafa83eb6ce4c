/* vit_amd_registers.h -- register tokens (`model.num_register_tokens`; included by vit_amd.h; conventions as stated there).
 *
 * What it stands for: Darcet et al., "Vision Transformers Need Registers"; timm `VisionTransformer(reg_tokens=R)` and HF
 * `Dinov2WithRegisters`.  R learned tokens join the sequence behind CLS:
 *     [CLS, reg_0 .. reg_{R-1}, patch_0 .. patch_{N-1}],   T = 1 + R + N
 * They take no position information, every layer attends to them and every head ignores them.  The reference's model has no
 * such tokens: `model.num_register_tokens` is this build's key.  Everything behind the embedding runs unchanged at that T; the
 * two entry points below are vit_embed_finish / vit_embed_finish_masked and their backwards with the R rows in between.
 *
 * vit_embed_finish_reg: tokens f32 [B, T, D], whose patch rows 1 + R + n already hold the projection (vit_gemm with
 *   out_row_offset = 1 + R), finished in place:
 *     row(b, 0) = cls;  row(b, 1 + r) = reg[r];  row(b, 1 + R + n) = mask[b, n] ? mask_token : tokens[b, 1 + R + n]
 *     tokens[b, t] = dropout(row(b, t) + p(t)),   p(0) = pos[0],  p(1 + r) = 0 (nothing is added),  p(1 + R + n) = pos[1 + n]
 *   pos: f32 [1 + N, D] or NULL (none).  mask: int32 [B, N] or NULL (none masked; non-zero = masked, only ever compared with
 *   zero); mask_token [D] must be given exactly when mask is.  The projected token of a masked patch is not loaded.  The
 *   dropout multiplier of an element is keyed by (row b * T + t, column), registers included.  16-byte accesses: D % 4 == 0.
 * vit_embed_finish_reg_bwd: with g[b, t] = dropout_multiplier(b, t) * dtokens[b, t]:
 *     dpatch[b * N + n] = mask[b, n] ? 0 : g[b, 1 + R + n]              (bf16 / f32; every patch row is written)
 *     dcls = sum_b g[b, 0];   dreg[r] = sum_b g[b, 1 + r];   dmask_token = sum over masked (b, n) of g[b, 1 + R + n]
 *     dpos[0] = sum_b g[b, 0];   dpos[1 + n] = sum_b g[b, 1 + R + n]    (dpos f32 [1 + N, D] or NULL)
 *   dmask_token must be given exactly when mask is.
 *   THE ORDER OF EVERY SUM, a function of (B, R, N) alone -- not of D, the grid or the number of compute units; no float
 *   atomics, bit-identical from call to call.  The batch falls into Y = ceil(B / c) chunks of c = ceil(B / min(B, 16))
 *   consecutive samples.  For chunk y and token t
 *       q[y][t] = (..((0 + g[y c, t]) + g[y c + 1, t]) + ..)            (ascending b inside the chunk; f32 adds from +0)
 *   and m[y][t] likewise over the masked samples of a patch row alone (+0 for CLS and register rows).  Then
 *       dcls = S(q[0][0], q[1][0], .., q[Y-1][0]),  dreg[r] = S(q[.][1 + r]),  dpos[0] = dcls's sum,  dpos[1 + n] = S(q[.][1 + R + n])
 *       dmask_token = S over the Y * T rows m[y][t] in the order y-major, and inside a chunk: CLS, patch 0 .. N-1, register 0 .. R-1
 *   where S(x_0 .. x_{n-1}) is the library's partial-row reducer:
 *       n > 512 first folds groups of G = ceil(n / min(32, floor(n / 32))) consecutive rows into one row each,
 *           row' = ((0 + u_0) + u_1 .. + u_15),  u_j = ((0 + x_{r0 + j}) + x_{r0 + j + 16}) + ..   (ascending, inside the group)
 *       and continues with those ceil(n / G) rows;
 *       then strand j (0 <= j < 16) takes the rows j, j + 16, j + 32, ..: the even-numbered of them (counting from 0) are
 *       added in ascending order to a0 (from +0), the odd-numbered to a1 (from +0), s_j = a0 + a1, and
 *           S = ((..((0 + s_0) + s_1) + ..) + s_15)                      (n <= 16: the plain ascending sum from +0)
 *   `accumulate` (OR the handle's "grad_accumulate"): dcls / dreg / dpos / dmask_token store S + old, one more f32 add.
 *   Workspace: Y * T * D floats, twice that with a mask; claimed before the first launch (vit_workspace_needed()).
 * R = 0 is legal in both (reg / dreg are then ignored and may be NULL) and gives, bit for bit, what vit_embed_finish /
 * vit_embed_finish_masked and their backwards give: the same selects, the same add and multiply, the same sums.
 * Bad arguments -- a null required pointer, mask without mask_token (or the reverse), B, N or D < 1, R < 0, D % 4 != 0,
 * dropout_p outside [0, 1), a dtype that is neither VIT_BF16 nor VIT_F32 -- return VIT_ERR_ARG with a message and launch
 * nothing. */
#ifndef VIT_AMD_REGISTERS_H_
#define VIT_AMD_REGISTERS_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

int vit_embed_finish_reg(vit_handle h, float* tokens, const float* cls, const float* reg, const float* pos, const int32_t* mask,
                         const float* mask_token, int B, int R, int N, int D, float dropout_p, uint64_t seed, uint64_t site,
                         vit_stream stream);
int vit_embed_finish_reg_bwd(vit_handle h, const float* dtokens, const int32_t* mask, void* dpatch_out, int dpatch_dtype,
                             float* dcls, float* dreg, float* dpos, float* dmask_token, int B, int R, int N, int D,
                             float dropout_p, uint64_t seed, uint64_t site, int accumulate, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_REGISTERS_H_ */
