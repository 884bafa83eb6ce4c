/* vit_amd_layerscale.h -- LayerScale (`model.layer_scale_init`) as an exact reparametrisation at weight size (included by
 * vit_amd.h; conventions as stated there).
 *
 * LayerScale multiplies each of a layer's two residual branches by a learnable per-channel factor lambda.  The branch is
 * dropout(W x + b) behind a per-sample gate, and both the mask and the gate commute with a per-channel factor, so
 *     lambda (.) dropout(W x + b) = dropout((diag(lambda) W) x + lambda (.) b):
 * the out-projection / FC2 GEMMs read the FOLDED operands W' = diag(lambda) W, b' = lambda (.) b, and the gradients those
 * GEMMs and the LayerNorm backward produce are the RAW gradients dW', db' of the folded operands, from which
 *     dW = diag(lambda) dW',   db = lambda (.) db',   dlambda[c] = sum_k dW'[c, k] W[c, k] + db'[c] b[c].
 * No GEMM, LayerNorm or attention kernel changes and no activation-sized byte is added: the feature is the two streaming
 * kernels below over a TABLE of matrices in device memory (the two Linears of a layer have different K, so every entry
 * carries its own rows and cols).  One wave owns a row; 16 bytes per lane; plain vector stores; no atomics, no workspace;
 * the row sum of dlambda is a fixed-order wave reduction, so results are deterministic.  Kernel arguments hold nothing that
 * changes from step to step: both launches may be captured in a hipGraph.
 *
 * vit_layer_scale_table_write: checks `count` entries on the host and writes them to table[0 .. count) on `stream`; the
 *   entries travel by value in kernel arguments (as vit_optim_groups_write's rows do), so there is no staging buffer.  An
 *   entry needs W, b, lambda and at least one complete output set: {Wf, bf} (what the fold writes) and / or {dW_raw, db_raw,
 *   dW, db, dlambda} (what the gradient pass reads and writes); a launch skips entries that lack its set.  `table` holds 96
 *   bytes per entry, 16-byte aligned.
 * vit_layer_scale_fold: for entries [0, n_entries) of `table`:  Wf[c, k] = lambda[c] * W[c, k], stored as bf16 (round to
 *   nearest even of the f32 product: vit_cast_f32_bf16's rounding) or f32 per `out_dtype`; bf[c] = lambda[c] * b[c] in f32.
 *   `max_rows`: the largest `rows` among those entries (the launch geometry; rows past an entry's own are not touched).
 *   Moves 4 + 2 (4) bytes per weight.
 * vit_layer_scale_grad: for entries [0, n_entries):  dW (+)= lambda[c] * dW_raw[c, k];  db (+)= lambda[c] * db_raw[c];
 *   dlambda[c] (+)= sum_k dW_raw[c, k] * W[c, k] + db_raw[c] * b[c].  accumulate = 0 stores, 1 adds to what is there (dW: one
 *   fused multiply-add per element; db, dlambda: one add).  db_raw is ZEROED behind the read: the fused LayerNorm backward adds
 *   into its dbias output under the handle's "grad_accumulate" option, so the raw bias gradient of an accumulating backward has
 *   to start from zero.  Moves 12 (accumulate: 16) bytes per weight.
 * VIT_ERR_ARG, before anything is launched: table NULL or not 16-byte aligned; n_entries / count <= 0; max_rows <= 0; out_dtype
 *   not VIT_F32 / VIT_BF16; accumulate not 0 / 1; an entry with a NULL W, b or lambda, without a complete output set, with
 *   rows <= 0, cols <= 0 or cols % 4 != 0, or with a matrix that is not 16-byte aligned. */
#ifndef VIT_AMD_LAYERSCALE_H_
#define VIT_AMD_LAYERSCALE_H_

#include "vit_amd.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct vit_layer_scale_entry {
  const float* W;      /* [rows, cols] f32: the parameter (rows = output channels, cols = K) */
  const float* b;      /* [rows] */
  const float* lambda; /* [rows] */
  void* Wf;            /* fold: [rows, cols] bf16 / f32 */
  float* bf;           /* fold: [rows] */
  const float* dW_raw; /* grad: [rows, cols], the gradient of Wf */
  float* db_raw;       /* grad: [rows], the gradient of bf; zeroed by the pass */
  float* dW;           /* grad: [rows, cols] */
  float* db;           /* grad: [rows] */
  float* dlambda;      /* grad: [rows] */
  int32_t rows, cols;
  int64_t reserved;    /* 96 bytes */
} vit_layer_scale_entry;

int vit_layer_scale_table_write(vit_handle h, void* table, const vit_layer_scale_entry* entries, int count, vit_stream stream);
int vit_layer_scale_fold(vit_handle h, const void* table, int n_entries, int max_rows, int out_dtype, vit_stream stream);
int vit_layer_scale_grad(vit_handle h, const void* table, int n_entries, int max_rows, int accumulate, vit_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* VIT_AMD_LAYERSCALE_H_ */
