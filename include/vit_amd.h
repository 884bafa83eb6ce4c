/* vit_amd.h -- C ABI of libvit_amd.so: the MI355X (gfx950) kernels behind the ViT training hot path of ViskaWei/VIT.
 *
 * The reference has no FFI layer: its boundary is the Python object surface that Lightning calls
 * (SURVEY.md section 8b).  This header is therefore the boundary the build's own host side (the vit_amd Python package, which
 * mirrors that surface) binds through ctypes; INTEGRATION.md shows the stub a maintainer of the reference would add.
 * Each entry point cites the reference code whose arithmetic it replaces (paths relative to the reference root).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (torch); nothing is allocated inside except the handle;
 *   - every call is asynchronous on `stream` (a hipStream_t passed as void*); no call synchronises the device;
 *   - return value: VIT_OK or a negative vit_status; vit_last_error() returns a thread-local message;
 *   - `dtype` arguments are vit_dtype codes; row-major tensors; "ld*" = leading dimension in ELEMENTS;
 *   - alignment: every base pointer 16-byte aligned, every leading/inner dimension of a bf16 GEMM operand a multiple
 *     of 8 elements (of an f32 one: 4), checked on the host before any launch (VIT_ERR_ARG otherwise);
 *   - dropout masks are a pure function of (seed, site, row, col): forward and backward regenerate them, nothing is
 *     stored;
 *   - state: the handle (workspace pointer, optional per-step state pointer, launch geometry: vit_handle_set_option) and
 *     the process-wide kernel-selection knobs of vit_set_option (A/B switches between bit-identical kernel forms); nothing
 *     else persists between calls.
 */
#ifndef VIT_AMD_H_
#define VIT_AMD_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VIT_AMD_VERSION 100

typedef struct vit_ctx* vit_handle;
typedef void* vit_stream; /* hipStream_t */

typedef enum { VIT_OK = 0, VIT_ERR_ARG = -1, VIT_ERR_HIP = -2, VIT_ERR_UNSUPPORTED = -3, VIT_ERR_WORKSPACE = -4 } vit_status;
typedef enum { VIT_F32 = 0, VIT_BF16 = 1 } vit_dtype;
/* GELU: C = gelu(acc + bias), aux_out (optional) = the pre-activation.  DGELU: C = acc * gelu'(aux_in).
 * GELU_GRAD: as GELU but aux_out = gelu'(pre-activation) -- the forward already holds Phi and exp(-x^2/2), so saving the
 * derivative costs two FMAs there and the backward GEMM (MUL_AUX: C = acc * aux_in) needs no transcendental at all. */
typedef enum { VIT_ACT_NONE = 0, VIT_ACT_GELU = 1, VIT_ACT_DGELU = 2, VIT_ACT_GELU_GRAD = 3, VIT_ACT_MUL_AUX = 4 } vit_act;
typedef enum { VIT_LOSS_MSE = 0, VIT_LOSS_L1 = 1, VIT_LOSS_CE = 2, VIT_LOSS_SOFT_CE = 3, VIT_LOSS_BCE = 4 } vit_loss;

int vit_version(void);
const char* vit_last_error(void);

/* Handle: device id + a workspace (split-K slabs, reduction partials).  The workspace is caller-owned device memory of any
 * size (256-byte aligned; none until vit_set_workspace).  Each call states what it needs: one that needs more than the handle
 * holds returns VIT_ERR_WORKSPACE BEFORE launching anything -- nothing was written, and the call may simply be repeated with a
 * larger workspace, also under "grad_accumulate" -- and vit_workspace_needed() then returns the bytes that whole call needs
 * (thread-local, like vit_last_error).  The need depends on the call's arguments and the handle's options alone, and no call
 * chooses its kernels or its summation order by the size of the workspace.  vit_gemm's need is exact: the maximum over the stages
 * the call really runs (its split-K slabs; the column sums' partials of the one route it takes), plus the scratch matrix below
 * where there is one; and every argument error of a vit_gemm is reported before its workspace is asked for. */
int vit_create(vit_handle* out, int device);
int vit_destroy(vit_handle h);
int vit_set_workspace(vit_handle h, void* ws, size_t bytes);
size_t vit_workspace_needed(void);
/* Process-wide options (none changes results beyond rounding order):
 *   "gemm_core": 0 = generic 128x128 core only, 1 = automatic (default): tile-aligned problems (M, N multiples of 256, K of
 *                64) run the 256x256x64 ping-pong core (wave halves one barrier out of phase: LOAD segment beside MFMA
 *                segment, ring of 8 half-tiles, 4 in flight); 5 = the same choice named explicitly.
 *   "attn_split": workgroups per (batch, head) in the resident attention kernels (T <= 592 at head_dim 64), default 2.
 *   "attn_bwd_fused": attention backward form: non-zero (default 4) = the pair-pipelined single kernel where it fits (head_dim
 *                64, 64 <= T <= 208), the dQ + dK/dV pair elsewhere; 0 = the dQ + dK/dV pair everywhere.  (The values 1 .. 3
 *                named the single-kernel forms of round 2, removed in round 4; they are accepted and mean the default.)
 *   "reserve_cus": 0 (default) .. 128 = the one-workgroup-per-CU kernels (ping-pong GEMMs, pair-pipelined attention backward) size
 *                their grids for that many fewer CUs, leaving room for a collective's kernels that overlap them (data-parallel
 *                runs; bench.py --reserve-cus).
 * The first three select the reference paths the tests compare against.  Returns VIT_ERR_ARG for an unknown name. */
int vit_set_option(const char* name, int value);
/* Per-handle launch geometry: what changes HOW MANY workgroups a call through this handle launches belongs to the handle, so
 * that two engines of one process (training + evaluation, an engine's second-stream handle) do not depend on the order
 * in which they were configured.  "reserve_cus": -1 (default) = follow the process-wide value above, 0 .. 128 = this handle's
 * own.  The remaining vit_set_option options select kernel forms and stay process-wide.
 * Reference: none (Lightning's 'ddp' overlaps NCCL with kernels that do not own whole SMs, src/hardware_utils.py:86-95).
 * "grad_accumulate": 0 (default) | 1.  While it is 1, every PARAMETER-GRADIENT output of a call through this handle stores
 * old + new where it stores new at 0: gradient accumulation over micro-batches, in place in the caller's gradient buffer
 * (Lightning's accumulate_grad_batches; autograd's `p.grad +=` for a buffer the kernels own).  `new` is bit for bit the value
 * overwrite mode stores, and the add is ONE f32 add in the producer's final write or reduce stage: no float atomics, no second
 * buffer, no extra pass over a weight matrix, deterministic (a second run from the same old values is bit-identical).
 * The outputs it covers: vit_gemm's colsum_out always, and its C when the product has the weight-gradient form dW = dY^T X
 * (a_trans != 0 and an f32 C; OR-ed with vit_gemm_desc.accumulate -- forward products and the dX products of the fp32 path
 * also write an f32 C and are never touched); vit_linear_bwd_dw / _dw_rows' dW; vit_colsum_rows' out; dgamma / dbeta / dbias
 * of the three vit_layernorm_bwd* forms; vit_attention_bwd's dqkv_colsum; vit_embed_finish_bwd's dcls / dpos and
 * vit_head_loss_bwd's dW / db (OR-ed with their `accumulate` argument).  vit_colsum keeps its own `accumulate` argument alone.
 * Activation gradients (dx, dyn, dqkv, dlast_hidden, ...) are always overwritten.
 * Where each add sits: split-K products -- in the slab reduction (slab 0 + slab 1 + ... in slice order, times alpha, THEN
 * + old C); single-slice products -- the epilogue's residual port reads old C; vit_linear_bwd_dw_rows -- the final store of
 * the slice total; every vector output -- the last stage of the partial-row reducer.  A vit_gemm whose C accumulates AND that
 * carries colsum_out (two parameter gradients from one descriptor; no training step issues it) runs the product into a
 * scratch matrix in the workspace, behind what its stages use (part of what the call needs of it), sums its columns and adds it
 * into C.
 * "lamb_passes": 7 (default) | a mask of 1 (moments + partial norms), 2 (ratios), 4 (apply): the launches a vit_lamb_step*
 * call makes (vit_amd_optim.h).  For measurement only -- tools/lamb_bench.py times each pass alone with it; a pass alone reads
 * what an earlier full call left in the workspace and in `trust`, so anything but 7 computes no optimizer step. */
int vit_handle_set_option(vit_handle h, const char* name, int value);

/* Per-step state in device memory, for a training step captured as a hipGraph (HIP streams and graphs instead of a tracing
 * compiler: kernel arguments are frozen at capture, so what changes from step to step must be read from memory).
 * `state`: 32 bytes, 16-byte aligned: { u32 key0, key1; u32 reserved; f32 bc1, rsqrt_bc2; u32 step; u32 reserved[2] },
 * caller-owned.
 * While bound (NULL unbinds), every call through this handle that takes (dropout_p, seed, site) XORs the state's keys
 * into its dropout keys at kernel entry: the masks of a replay are those of (seed, site, step).  vit_step_advance (one
 * tiny kernel, first node of the captured step) does step += 1, derives the keys from (base_seed, step) and AdamW's
 * bias corrections from step.  The reserved words are neither written nor read: what a scheduler changes between replays
 * (learning rates, SGD's momentum; one-cycle cycles both on every step) lives in the optimizer's group table
 * (vit_optim_groups_write, vit_amd_optim.h), and the vit_*_step_groups_dyn forms take only the bias corrections from here.
 * Replaces what Lightning's loop hands torch per step: the generator advance behind nn.Dropout and optimizer.step()'s
 * step count (basemodule.py:230-251). */
int vit_step_state_bind(vit_handle h, void* state);
int vit_step_advance(vit_handle h, uint64_t base_seed, float beta1, float beta2, vit_stream stream);

/* ------------------------------------------------------------------------------------------------ GEMM
 * C = epilogue(alpha * op(A) * op(B)), bf16 MFMA (v_mfma_f32_16x16x32_bf16), fp32 accumulate.
 * Replaces every nn.Linear on the path: tokenization.py:41,50 (patch projection); HF ViTSelfAttention
 * query/key/value (restated at vit_with_rope.py:54-56), ViTSelfOutput.dense, ViTIntermediate.dense, ViTOutput.dense
 * and their autograd backward (dX = dY*W, dW = dY^T*X).
 *   a_trans = 0: A stored [M][K] (lda >= K)      a_trans = 1: A stored [K][M] (lda >= M)
 *   b_trans = 0: B stored [N][K] (ldb >= K; the nn.Linear weight layout)   b_trans = 1: B stored [K][N]
 * Epilogue, in this order, on the fp32 accumulator v of element (m, n):
 *   v = alpha*v + bias[n];  ACT_GELU: (aux_out[m,n] = bf16(v) if aux_out), v = gelu_erf(v);
 *   ACT_DGELU: v *= gelu_erf'(aux_in[m,n]);  dropout(p, seed, site) as a function of (out_row, n);
 *   v += residual[out_row, n];  C[out_row, n] = (c_dtype) v
 * with out_row = (m / rows_per_batch) * out_batch_rows + (m % rows_per_batch) + out_row_offset when
 * rows_per_batch > 0 (patch-embed writes token rows 1..N of each sample, embedding.py:87-88), else out_row = m.
 * split_k > 1 accumulates partial products in the handle's workspace and reduces them deterministically (no float
 * atomics: the reference runs with deterministic=True, basemodule.py:250); only alpha and C (f32) apply then.
 */
typedef struct vit_gemm_desc {
  int M, N, K;
  int a_trans, b_trans;
  int ab_dtype;            /* VIT_BF16 (VIT_F32 operands: split-bf16 "x3" mode) */
  const void* A; int64_t lda;
  const void* B; int64_t ldb;
  void* C; int64_t ldc; int c_dtype;
  float alpha;
  const float* bias;       /* [N] or NULL */
  int act;                 /* vit_act */
  void* aux_out;           /* ACT_GELU: optional bf16 [M,N] pre-activation (ld = ldaux) */
  const void* aux_in;      /* ACT_DGELU: bf16 [M,N] pre-activation (ld = ldaux) */
  int64_t ldaux;
  float dropout_p; uint64_t seed; uint64_t site;
  const float* residual; int64_t ldres;   /* f32, indexed by out_row */
  int rows_per_batch, out_batch_rows, out_row_offset;
  int split_k;             /* 0/1 = off; >1 = that many K slices; -1 = choose */
  int accumulate;          /* C (f32) += result instead of C = result: in the split-K slab reduction (slabs summed in slice
                            * order, scaled by alpha, old C added last), else through the epilogue's residual port (no residual
                            * then); OR-ed with the handle's "grad_accumulate" for products of the weight-gradient form */
  float* colsum_out;       /* optional f32 [N]: column sums of C as stored (a Linear's bias gradient when C is the gradient
                            * of its output); summed inside the epilogue by the kernels that have such an epilogue, else by a
                            * vit_colsum pass behind the product: the shape and the options decide, never the workspace */
  /* Rotary position embedding of the fused QKV projection's output (src/models/vit_with_rope.py:58-60, rope.py:116-131):
   * columns [0, rope_cols) of C are heads of rope_dh columns whose element i pairs with element i + rope_dh / 2, row m is token
   * m % rope_T; cos / sin: f32 [rope_T, rope_dh / 2] (vit_rope_qk's tables).  NULL = off.  The ping-pong core rotates in its
   * epilogue, on the f32 values before the one rounding to bf16 (rope_dh 16 / 32 / 64, rope_cols a multiple of 64); every
   * other case runs vit_rope_qk on C right after the product -- same contract either way, PROVIDED the tables are the
   * reference's: row t holds the angles t * theta_i, linear in t and zero-based (rope.py:36-56).  The rotating epilogue reads
   * eight table rows per tile and steps a lane's later rows by the angle-addition recurrence over table row 8, so a table of
   * other positions (offset, scaled, learned) is NOT supported through this descriptor: rotate with vit_rope_qk, which reads
   * the table per row.  dropout_p must be 0 with rope (the reference rotates before any dropout). */
  const float* rope_cos; const float* rope_sin;
  int rope_T, rope_dh, rope_cols;
  /* Row stride of the dropout key: 0 / 1 = the mask of element (out_row, n) is keyed by out_row (above); s > 1 = by out_row * s.
   * For a product over a strided subset of a larger problem's rows (A read in place with lda = s * K, compact C: the CLS rows of
   * the last encoder layer, s = T): the mask of compact row r is then bit for bit the one the full problem draws for its row
   * r * s.  Such a launch runs the generic epilogue. */
  int drop_row_stride;
} vit_gemm_desc;
int vit_gemm(vit_handle h, const vit_gemm_desc* d, vit_stream stream);
/* Symbol (as rocprofv3 prints it, without the "void vit::" prefix and argument list) of the kernel of the calling thread's
 * last vit_gemm that passed its argument checks: written when the call is planned, before its workspace is claimed, so a call
 * refused with VIT_ERR_WORKSPACE (or one that cannot launch) still names the kernel it would run.  Lets a benchmark attribute
 * its per-call timings to the kernels a profiler lists. */
const char* vit_last_gemm_kernel(void);

/* Convenience forms named after SURVEY.md section 8b.  x:[M,K] bf16, W:[N,K] bf16 (nn.Linear layout), y:[M,N]. */
int vit_linear_fwd(vit_handle h, const void* x, const void* W, const float* bias, void* y, int y_dtype, int M, int N,
                   int K, int act, void* aux_out, float dropout_p, uint64_t seed, uint64_t site,
                   const float* residual, vit_stream stream);
/* dX[M,K] = dY[M,N] * W[N,K]  (optionally *= gelu'(aux_in)) */
int vit_linear_bwd_dx(vit_handle h, const void* dy, const void* W, void* dx, int dx_dtype, int M, int N, int K,
                      const void* dgelu_aux_in, vit_stream stream);
/* dW[N,K] (f32) (+)= dY[M,N]^T * X[M,K], deterministic split-K over M */
int vit_linear_bwd_dw(vit_handle h, const void* dy, const void* x, float* dW, int M, int N, int K, int accumulate,
                      vit_stream stream);

/* Weight gradient and column sums over a strided subset of rows (the CLS rows of the last encoder layer: row_stride = T,
 * full_rows = the padded B*T of the full tensors).  dy: [rows, N] (ld = ldy), x: [rows, K] (ld = ldx), both `dtype`; compact
 * row b stands for row b * row_stride of full tensors whose other rows are zero (dy) / irrelevant (x).
 * dW[N, K] (f32, dense) = sum_b dy[b]^T x[b].  Where the product over the full tensors would run the ping-pong core with
 * split-K, the B terms are summed in that product's order (K slices, rows within a slice, then the slices), so with
 * row_stride >= 64 the result is bit for bit the full product's (zero terms leave an f32 sum unchanged); any other shape runs
 * the compact product through vit_gemm -- except f32 operands (precision '32'), which run the full product's own kernel, split-K
 * plan and MFMA sequence with the absent rows read as zero: bit for bit the full product wherever rows x max(ldy, ldx) x 4 bytes stay below 2 GiB (beyond that: the compact product).  vit_colsum_rows: out[cols] = column sums of a ([rows, cols], ld = lda), likewise in
 * the order of the column sums that ride in the ping-pong epilogue of the product that would write the full tensor (f32: in
 * the order of vit_colsum over the full tensor). */
int vit_linear_bwd_dw_rows(vit_handle h, const void* dy, int64_t ldy, const void* x, int64_t ldx, int dtype, float* dW,
                           int rows, int N, int K, int64_t row_stride, int64_t full_rows, vit_stream stream);
int vit_colsum_rows(vit_handle h, const void* a, int a_dtype, int64_t lda, float* out, int rows, int cols, int64_t row_stride,
                    int64_t full_rows, vit_stream stream);

/* ------------------------------------------------------------------------------------------- LayerNorm
 * HF nn.LayerNorm(hidden, eps=layer_norm_eps=1e-12) (builder.py:250): layernorm_before/after and vit.layernorm.
 * x: f32 [rows, D] (the residual stream is kept in fp32); y: y_dtype [rows, D]; mean/rstd: f32 [rows] (saved for bwd).
 */
int vit_layernorm_fwd(vit_handle h, const float* x, const float* gamma, const float* beta, void* y, int y_dtype,
                      float* mean, float* rstd, int rows, int D, float eps, vit_stream stream);
/* The same LayerNorm over x + delta, where delta (delta_dtype [rows, D]) is the output of the Linear underneath a
 * "dropout(Linear(.)) + residual" (HF ViTLayer: attention_output + hidden_states; ViTOutput: hidden_states + input_tensor),
 * and xsum (f32 [rows, D]) receives the sum: the residual add rides on the pass that reads the stream anyway, so the
 * projection GEMMs write bf16 and never load. */
int vit_layernorm_fwd_residual(vit_handle h, const float* x, const void* delta, int delta_dtype, float* xsum,
                               const float* gamma, const float* beta, void* y, int y_dtype, float* mean, float* rstd,
                               int rows, int D, float eps, vit_stream stream);
/* vit_layernorm_fwd_residual over a strided subset of the stream's rows: row r of x is row r * x_row_stride of the tensor x
 * points into (x_row_stride >= 1); delta, xsum, y, mean, rstd are compact [rows, .].  The last encoder layer's LayerNorm-after
 * when only the CLS rows are consumed (x_row_stride = T): the head reads last_hidden[:, 0, :] alone (specvit.py:78-81). */
int vit_layernorm_fwd_residual_rows(vit_handle h, const float* x, int64_t x_row_stride, const void* delta, int delta_dtype,
                                    float* xsum, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                                    float* rstd, int rows, int D, float eps, vit_stream stream);
/* dx[rows,D] (f32) = LN'(dy) (+ dres if not NULL: the residual branch's gradient); dgamma/dbeta (f32 [D]) are
 * reduced deterministically through the workspace; the handle's "grad_accumulate" option (vit_handle_set_option) adds into
 * them -- and into dbias of the fused / rows forms below -- instead of overwriting. dy: dy_dtype [rows, D]. */
int vit_layernorm_bwd(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma,
                      const float* mean, const float* rstd, const float* dres, float* dx, float* dgamma,
                      float* dbeta, int rows, int D, vit_stream stream);

/* Same, fused with what always follows it in this path: also writes dyn (bf16 [rows, D]) = dropout_mask(seed, site) *
 * dx -- the gradient wrt the output of the Linear under "dropout(Linear(.)) + residual" -- and dbias (f32 [D]) = its
 * column sums (that Linear's bias gradient): one pass instead of vit_dropout_bwd_cast + vit_colsum re-reading dx. */
int vit_layernorm_bwd_fused(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma,
                            const float* mean, const float* rstd, const float* dres, float* dx, float* dgamma,
                            float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, float dropout_p,
                            uint64_t seed, uint64_t site, vit_stream stream);

/* vit_layernorm_bwd (dyn == NULL: dyn_dtype, dbias and the dropout arguments are ignored) / vit_layernorm_bwd_fused for the
 * two ends of a compact run of rows.  `rows` is always the row count of the FULL tensor.
 *   row_stride s > 1: of those rows only the rows r with r % s == 0 exist; dy, x, mean, rstd, dx, dyn and dres hold them
 *     compactly at r / s (ceil(rows / s) rows).  The dropout mask of dyn is keyed by r, and dgamma / dbeta / dbias are summed
 *     in the order the pass over the full tensor (its other rows exact zeros) sums them: bit for bit its results.
 *   dres_row_stride s > 0 (with row_stride 1): dres alone is compact, [ceil(rows / s), D]; row j of it is the residual
 *     gradient of row j * s, every other row has none (nothing is read for it).  This is where the gradient of the CLS rows
 *     re-enters the full token stream, without a zero-filled [rows, D] tensor in between. */
int vit_layernorm_bwd_rows(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const float* dres, int64_t dres_row_stride, float* dx, float* dgamma,
                           float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, float dropout_p,
                           uint64_t seed, uint64_t site, int64_t row_stride, vit_stream stream);

/* ------------------------------------------------------------------------------------------- Attention
 * softmax(Q K^T * scale) -> dropout -> * V, per (batch, head); flash-style (scores never reach HBM).
 * Replaces HF ViTSelfAttention's eager arithmetic as restated in vit_with_rope.py:63-81 (no logit clamp exists in
 * the reference: SURVEY.md section 0.4).  qkv: bf16 [B*T, 3*H*dh] token-major, columns [q | k | v], head h at
 * columns h*dh (the fused QKV projection's natural output; equals view(B,T,H,dh).transpose(1,2) of each third).
 * ctx: bf16 [B*T, H*dh] (= context_layer after transpose+view, vit_with_rope.py:75-78); lse: f32 [B*H, T]
 * (log-sum-exp of the scaled scores, saved for backward).
 * io_dtype = VIT_BF16: the MFMA flash kernels (qkv / ctx / dctx / dqkv bf16).  io_dtype = VIT_F32: the same tensors in
 * f32 and exact fp32 arithmetic (the precision='32' path; T <= 4096).
 */
/* ctx_lo (bf16 [B*T, H*dh], may be NULL): the forward also stores the rounding residual ctx_exact - bf16(ctx_exact), so that
 * the backward can form delta = rowsum(dctx * (ctx + ctx_lo)) with the context kept to ~16 mantissa bits.  Why: the softmax
 * backward is dS = P o (dP - delta); the reference (autocast, vit_with_rope.py:63-81 under basemodule.py:233) takes
 * delta = sum_j P_j dP_j in fp32, which cancels exactly against dP.  rowsum(dctx * ctx) with an 8-bit ctx is off by an amount
 * COMMON to a score row, which survives the sum over keys in dQ / dK once token representations share a large common
 * component (deep layers): 5e-2 on ViT-L's late query weights against the reference's own bf16 1.1e-2; with the residual 1e-2
 * or better (tests/test_parity_deep_gpu.py).  io_dtype = VIT_F32 ignores ctx_lo. */
int vit_attention_fwd(vit_handle h, const void* qkv, void* ctx, void* ctx_lo, float* lse, int io_dtype, int B, int H, int T,
                      int dh, float scale, float dropout_p, uint64_t seed, uint64_t site, vit_stream stream);
/* dqkv: bf16 [B*T, 3*H*dh] from dctx: bf16 [B*T, H*dh]; recomputes probabilities from lse. delta: f32 [B*H, T]
 * scratch (rowsum(dctx * (ctx + ctx_lo)); ctx_lo may be NULL: rowsum(dctx * ctx)), written by this call.
 * dqkv_colsum (f32 [3*H*dh], may be NULL) = the column sums of dqkv as stored: the bias gradient of the fused QKV projection
 * (without RoPE; with it the sums must be taken after the inverse rotation).  The resident and pipelined bf16 kernels sum
 * their own rows on the way out (one partial row per wave through the workspace); the tiled and f32 forms run vit_colsum
 * afterwards.  Which of the two is a function of the shape and the options alone. */
int vit_attention_bwd(vit_handle h, const void* qkv, const void* ctx, const void* ctx_lo, const void* dctx, const float* lse,
                      float* delta, void* dqkv, int io_dtype, int B, int H, int T, int dh, float scale, float dropout_p,
                      uint64_t seed, uint64_t site, float* dqkv_colsum, vit_stream stream);
/* Attention probabilities [B, H, T, T] f32 (eval-mode, for output_attentions=True: specvit.py:92-93). */
int vit_attention_probs(vit_handle h, const void* qkv, float* probs, int io_dtype, int B, int H, int T, int dh,
                        float scale, vit_stream stream);

/* ------------------------------------------------------------------------------- Embedding-side kernels
 * x.unfold(1,P,S) (+ zero pad of the ragged tail patch) -> patches [B*N, P] (bf16 or f32)   (tokenization.py:45-49) */
int vit_unfold_cast(vit_handle h, const float* x, void* patches, int out_dtype, int B, int L, int P, int S, int N,
                    vit_stream stream);
/* Backward of vit_unfold_cast wrt the signal, for a trainable input preprocessor (src/models/preprocessor.py:96-111 in
 * front of src/models/tokenization.py:43-69): dx[B, L] (f32) = overlap-add of dpatches[B*N, P] (f32) over the windows that
 * lie inside the signal.  Gather form, no atomics. */
int vit_fold_add(vit_handle h, const float* dpatches, float* dx, int B, int L, int P, int S, int N, vit_stream stream);

/* Training-time noise injection of ViTLModule.training_step (src/vit.py:86-88): out = flux + randn_like(flux) * error *
 * noise_level over n f32 elements (n % 4 == 0; out may alias flux).  The normal variates come from a counter-based
 * generator keyed on (seed, element index); the reference's come from torch's generator, whose stream is
 * implementation-defined, so only the distribution is contractual. */
int vit_add_noise(vit_handle h, const float* flux, const float* error, float* out, long n, float noise_level,
                  uint64_t seed, vit_stream stream);

/* Rotary position embedding of ViTSelfAttentionWithRoPE (src/models/vit_with_rope.py:58-60 -> src/models/rope.py:66-131,
 * model.pos_encoding_type: 'rope'): rotates the query and key thirds of the token-major qkv buffer ([rows, ld >= 2*H*dh]:
 * only columns [0, 2*H*dh) are touched, so a q / k-only buffer is legal; rows = B*T, position = row % T) in place, pairing
 * element i of a head with element i + dh/2 (_rotate_half).
 * cos_half / sin_half: f32 [T, dh/2] -- the first half of the reference's cached tables (rope.py:44-56), built on the
 * host by the reference's own formula.  inverse != 0 rotates by the negative angle: the backward of the rotation,
 * applied to dq / dk before the projection's weight and input gradients. */
int vit_rope_qk(vit_handle h, void* qkv, int dtype, const float* cos_half, const float* sin_half, long rows, int T,
                int H, int dh, long ld, int inverse, vit_stream stream);

/* rows 0 of every sample <- cls_token (embedding.py:87-88); optional "+ position_embeddings" (embedding.py:95-97)
 * and the embedding dropout (embedding.py:100) over the whole [B, T, D] f32 token tensor, in place. */
int vit_embed_finish(vit_handle h, float* tokens, const float* cls, const float* pos, int B, int T, int D,
                     float dropout_p, uint64_t seed, uint64_t site, vit_stream stream);
/* backward of the two above: dtokens [B,T,D] f32 -> dpatch_out bf16 [B*N, D] (dropout mask applied), dcls [D],
 * dpos [T,D] or NULL. */
int vit_embed_finish_bwd(vit_handle h, const float* dtokens, void* dpatch_out, int dpatch_dtype, float* dcls, float* dpos,
                         int B, int T, int D, float dropout_p, uint64_t seed, uint64_t site, int accumulate,
                         vit_stream stream);

/* ------------------------------------------------------------------------------- Elementwise / reductions
 * dy ([rows, cols], bf16 or f32) = dropout_mask(seed,site) * dx (f32): the gradient of "dropout(y) + residual" wrt y */
int vit_dropout_bwd_cast(vit_handle h, const float* dx, void* dy, int dy_dtype, int rows, int cols, float dropout_p,
                         uint64_t seed, uint64_t site, vit_stream stream);
/* out[cols] (f32) (+)= column sums of a [rows, cols] tensor (bias gradients), deterministic two-stage */
int vit_colsum(vit_handle h, const void* a, int a_dtype, int64_t lda, float* out, int rows, int cols, int accumulate,
               vit_stream stream);
/* f32 -> bf16 copy (weights after an optimizer step, inputs) */
int vit_cast_f32_bf16(vit_handle h, const float* src, void* dst, int64_t n, vit_stream stream);
/* dst (f32) = scale * src (bf16): the receive side of the optional bf16 gradient exchange (`train.ddp_grad_dtype: bf16`;
 * the reference's DDP exchanges fp32 gradients, src/hardware_utils.py:86-95 -- SURVEY.md section 5 prices the halved bytes) */
int vit_cast_bf16_f32(vit_handle h, const void* src, float* dst, int64_t n, float scale, vit_stream stream);

/* ------------------------------------------------------------------------------------- Head + loss
 * logits[B, C] = cls_rows * W^T + b, cls_rows = last_hidden[:, 0, :] (specvit.py:78-81); loss (specvit.py:83-89):
 * MSE / L1 over logits.view(-1) vs labels.view(-1) (mean), or cross-entropy over int64 labels (mean).
 * last_hidden: f32 [B, T, D]; loss_out: f32 [1]. labels may be NULL (loss_out untouched).
 * The soft-target kinds (the targets vit_mix_targets writes, vit_amd_mix.h; torch's F.cross_entropy with probability targets and
 * F.binary_cross_entropy_with_logits): labels are f32 [B, C] targets t,
 *   VIT_LOSS_SOFT_CE: loss = (1/B) sum_b sum_c -t[b,c] log_softmax(z[b])[c];  dz = (softmax(z) * sum_c t - t) * up / B
 *   VIT_LOSS_BCE:     loss = mean over B*C of max(z, 0) - z t + log1p(exp(-|z|));  dz = (sigmoid(z) - t) * up / (B*C)
 * C is 10 .. 1000 there, so their forward runs one wave per sample (lanes stride over C, wave max / sum), leaves the row losses
 * in the workspace (B floats: the call's need, claimed before the first launch) and a second single-block stage forms the
 * mean in a fixed order: deterministic.  MSE / L1 / CE keep their single-block kernel and need no workspace. */
int vit_head_loss_fwd(vit_handle h, const float* last_hidden, const float* W, const float* b, const void* labels,
                      float* logits, float* loss_out, int B, int T, int D, int C, int loss_kind, vit_stream stream);
/* d(last_hidden) (zero except the CLS rows), dW [C,D], db [C] given dloss (f32 [1], the upstream scalar gradient).  The
 * soft-target kinds form dz with one wave per sample, then d(last_hidden) with one lane per column; dW / db as for every kind
 * (`accumulate` / "grad_accumulate" included).  Workspace: B*C floats (dz), every kind. */
int vit_head_loss_bwd(vit_handle h, const float* last_hidden, const float* W, const float* logits, const void* labels,
                      const float* dloss, float* dlast_hidden, float* dW, float* db, int B, int T, int D, int C,
                      int loss_kind, int accumulate, vit_stream stream);

/* ------------------------------------------------------------------------------------- Optimizer
 * Global L2 norm (squared) of a flat f32 gradient buffer -> out[0] (Lightning gradient_clip_val=0.5, norm clipping:
 * basemodule.py:244). Deterministic two-stage reduction. */
int vit_grad_sqnorm(vit_handle h, const float* g, int64_t n, float* out, vit_stream stream);
/* out[0] += the squared norm of g: parameters that live outside the model's flat buffer (a trainable input
 * preprocessor) join the same global clipping norm. */
int vit_grad_sqnorm_acc(vit_handle h, const float* g, int64_t n, float* out, vit_stream stream);
/* torch.optim.AdamW step (opt/optimizer.py:16,108: lr, weight_decay=0 by default) over a flat parameter buffer, with
 * the clip coefficient min(1, max_norm / (sqrt(*sqnorm) + 1e-6)) applied to g on the fly (sqnorm may be NULL).
 * Also refreshes the bf16 shadow copy used by the GEMMs (p_bf16 may be NULL). bias_correction uses `step` (1-based). */
int vit_adamw_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                   float max_norm, vit_stream stream);

#ifdef __cplusplus
}
#endif

/* Covariance statistics of the training spectra (the file behind `warmup.cov_path`): vit_cov_accumulate, vit_cov_mean_finish,
 * vit_cov_finish.  Set-up time entry points, outside the training step: declared in their own header, part of this ABI. */
#include "vit_amd_cov.h"
/* The optimizer steps beside vit_adamw_step -- Adam with L2 decay and SGD, eager and captured (opt/optimizer.py:14-26,108;
 * `opt.type` in configs/config.yaml) -- are declared in their own header, part of this ABI. */
#include "vit_amd_optim.h"
/* The exponential moving average of the weights (`train.ema_decay`): vit_ema_update behind the optimizer step, vit_ema_swap
 * around an evaluation.  Declared in their own header, part of this ABI. */
#include "vit_amd_ema.h"
/* Stochastic depth (`model.drop_path_rate`): the path forms of the two LayerNorm passes that form and differentiate the
 * residual sums.  Declared in their own header, part of this ABI. */
#include "vit_amd_droppath.h"
/* LayerScale (`model.layer_scale_init`) as a reparametrisation at weight size: the fold of lambda into the out-projection /
 * FC2 operands and the pass that unfolds their raw gradients.  Declared in their own header, part of this ABI. */
#include "vit_amd_layerscale.h"
/* Mixup / CutMix of the batch and its labels (`augment:`): vit_mix_plan_write, vit_mix_signal, vit_mix_targets.  Declared in
 * their own header, part of this ABI. */
#include "vit_amd_mix.h"
/* Patch dropout (`model.patch_drop_rate`): the per-sample token selection and the gather forms of the embedding-side kernels
 * behind which the encoder runs at 1 + K tokens.  Declared in their own header, part of this ABI. */
#include "vit_amd_patchdrop.h"
/* Masked spectrum modelling (`model.task_type: mim`): the block mask, the embedding finish that substitutes the mask token and
 * its backward, and the reconstruction loss that reads its target from the signal.  Declared in their own header, part of
 * this ABI. */
#include "vit_amd_mim.h"
/* Global average pooling (`model.global_pool: avg`): the mean of the patch rows of the final LayerNorm's output, which the
 * head then reads in place of the CLS row, and its backward.  Declared in their own header, part of this ABI. */
#include "vit_amd_pool.h"
/* Sharpness-aware minimisation (`train.sam_rho`): the norm of the first gradient, the ascent that perturbs the flat parameter
 * buffer and keeps a backup, and the descent that restores it.  Declared in their own header, part of this ABI. */
#include "vit_amd_sam.h"
/* Register tokens (`model.num_register_tokens`): the embedding finish over [CLS, R registers, N patches] and its backward, for
 * the plain and the masked model.  Declared in their own header, part of this ABI. */
#include "vit_amd_registers.h"

#endif /* VIT_AMD_H_ */
