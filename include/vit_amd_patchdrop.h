/* vit_amd_patchdrop.h -- patch dropout: a training forward keeps a random K of each sample's N patch tokens (plus CLS) and
 * the encoder runs at T' = 1 + K (included by vit_amd.h; conventions as stated there).
 *
 * What it stands for: timm's `patch_drop_rate` (timm.layers.PatchDropout, "PatchDropout: Economizing Vision Transformers
 * Using Patch Dropout"; FLIP and MAE's encoder select tokens the same way).  The reference's model has no such module:
 * `model.patch_drop_rate` is this build's key and its default 0 is the reference's arithmetic.
 *
 * Past the embedding a step with patch dropout is a step of a model with sequence length T'; what is new sits in front:
 * the selection, gather forms of the four embedding-side kernels, and the backward of those.  Two index tensors tie them:
 *     idx  int32 [B, K]   the kept patches of sample b, strictly ascending in [0, N)
 *     slot int32 [B, N]   the inverse map: slot[b, n] = k where idx[b, k] = n, -1 for a dropped patch.  Every backward
 *                         reduction reads through it and therefore stays a gather: no scatter, no float atomics.
 * The position of compact token t of sample b is pos(b, t) = 0 for t = 0 (CLS), 1 + idx[b, t - 1] otherwise.
 * An index outside [0, N) never addresses memory: such a patch reads as a zero window / position row 0 (the engine
 * validates what a caller hands it; the kernels only stay inside their buffers).
 *
 * vit_patch_select: one workgroup per sample.  key(b, n) = drop_hash(k0, k1, b * N + n) with (k0, k1) the keys make_drop
 *   derives from (seed, site) (vit_amd/csrc/common.h; host restatement: oracle/dropmask.py drop_cfg, drop_hash).  A bound
 *   per-step record (vit_step_state_bind) XORs its keys into (k0, k1) at kernel entry ALWAYS -- the selection has no
 *   threshold that could be zero -- so a captured hipGraph draws a fresh subset on every replay.  The sample keeps the K
 *   patches that are smallest under (key ascending, then n ascending): the keys are staged in the LDS, every patch is ranked
 *   by counting, rank < K is kept (exactly K of them: the order is total), and a block scan compacts the kept patches in
 *   ascending n.  With iid keys that is a uniform K-subset.  1 <= K <= N <= VIT_PATCH_SELECT_MAX_N, else VIT_ERR_ARG.
 * vit_patch_slot: slot from a caller's idx (the engine's `patch_keep`): -1 everywhere, then slot[b, idx[b, k]] = k.
 * vit_unfold_gather_cast: patches[b * K + k, :] = cast(x[b, idx[b, k] * S : + P]); a window that does not fit inside the
 *   signal is all zero (vit_unfold_cast's rule).  Rows are those of vit_unfold_cast's output at b * N + idx[b, k], bit for bit.
 * vit_embed_finish_gather: vit_embed_finish over tokens [B, Tc, D] (Tc = 1 + K): CLS into row 0, + pos[pos(b, t), :] (pos:
 *   [T_full, D] or NULL), dropout keyed by the COMPACT row b * Tc + t -- the mask of a model of sequence length Tc.
 * vit_embed_finish_gather_bwd: the backward of that.  dpatch [B * K, D] (bf16 / f32) = mask * dtokens rows t >= 1;
 *   dcls [D] = the batch sum of row 0; dpos [T_full, D] (optional): row 0 = the CLS sum, row 1 + n = the sum over the samples
 *   b with slot[b, n] >= 0 of mask * dtokens[b, 1 + slot[b, n]], zero where no sample kept patch n.  The sums walk the batch
 *   in vit_embed_finish_bwd's chunks and order (fixed-order partials, then the deterministic reduce): with idx the identity
 *   (K = N) every output is vit_embed_finish_bwd's bit for bit.  `accumulate` (OR the handle's "grad_accumulate"): dcls /
 *   dpos store old + new.  Workspace: min(B, 16) * T_full * D floats, claimed before the first launch.
 * vit_rows_gather: out[b * Tc + t, :] = table[pos(b, t), :] for an f32 table [T_full, W], W a multiple of 4.  The engine
 *   builds per-step RoPE tables [B * Tc, head_dim / 2] with it; vit_rope_qk(rows = B * Tc, T = B * Tc) then rotates every token
 *   by its ORIGINAL position.  (The rotating GEMM epilogue takes linear positions only and is not used when dropping.)
 * vit_fold_add_gather: vit_fold_add reading dpatches [B * K, P] through slot: dropped windows contribute nothing, kept ones
 *   are added in ascending n -- the value of vit_fold_add over the zero-scattered [B * N, P] gradient. */
#ifndef VIT_AMD_PATCHDROP_H_
#define VIT_AMD_PATCHDROP_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

#define VIT_PATCH_SELECT_MAX_N 8192

int vit_patch_select(vit_handle h, int32_t* idx, int32_t* slot, int B, int N, int K, uint64_t seed, uint64_t site,
                     vit_stream stream);
int vit_patch_slot(vit_handle h, const int32_t* idx, int32_t* slot, int B, int N, int K, vit_stream stream);
int vit_unfold_gather_cast(vit_handle h, const float* x, const int32_t* idx, void* patches, int out_dtype, int B, int L, int P,
                           int S, int N, int K, vit_stream stream);
int vit_embed_finish_gather(vit_handle h, float* tokens, const float* cls, const float* pos, const int32_t* idx, int B, int Tc,
                            int T_full, int D, float dropout_p, uint64_t seed, uint64_t site, vit_stream stream);
int vit_embed_finish_gather_bwd(vit_handle h, const float* dtokens, const int32_t* slot, void* dpatch_out, int dpatch_dtype,
                                float* dcls, float* dpos, int B, int Tc, int T_full, int D, float dropout_p, uint64_t seed,
                                uint64_t site, int accumulate, vit_stream stream);
int vit_rows_gather(vit_handle h, const float* table, const int32_t* idx, float* out, int B, int Tc, int T_full, int W,
                    vit_stream stream);
int vit_fold_add_gather(vit_handle h, const float* dpatches, const int32_t* slot, float* dx, int B, int L, int P, int S, int N,
                        int K, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_PATCHDROP_H_ */
