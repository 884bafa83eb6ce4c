// LayerScale as a reparametrisation at weight size for gfx950 (include/vit_amd_layerscale.h): the fold W' = diag(lambda) W,
// b' = lambda (.) b that the out-projection / FC2 GEMMs read, and the pass that turns the raw gradients of the folded operands
// into those of W, b and lambda.  HBM-bound (6 / 8 and 12 / 16 B per weight).  One launch serves a table of matrices in device
// memory: blockIdx.y is the entry, a wave owns a row (64 lanes x 16 B per trip), rows are grid-strided in x.  Plain vector
// stores, no atomics, no workspace; the row sum of dlambda is a per-lane chain in column order and one xor butterfly:
// deterministic.
#include <string.h>

#include "common.h"

// as in optim.hip: every multiply-add that is fused is written as one (fma_)
#pragma clang fp contract(off)

namespace vit {

constexpr int LS_WAVES = STEP_BLOCK / 64;  // rows a block covers per trip
constexpr int LS_DEPTH = 3;                // 16-byte vectors per operand a lane of the gradient pass requests ahead
typedef vit_layer_scale_entry LsEntry;
static_assert(sizeof(LsEntry) == 96, "vit_layer_scale_entry is 96 bytes (six 16-byte pieces)");

__global__ __launch_bounds__(STEP_BLOCK) void layer_scale_fold_kernel(const LsEntry* __restrict__ table, int bf16_out) {
  const LsEntry e = table[blockIdx.y];  // block-uniform
  if (!e.Wf || !e.bf) return;
  const int lane = threadIdx.x & 63, nv = e.cols >> 2;
  for (long row = blockIdx.x * (long)LS_WAVES + (threadIdx.x >> 6); row < e.rows; row += (long)gridDim.x * LS_WAVES) {
    const float lam = e.lambda[row];
    const float* __restrict__ w = e.W + row * e.cols;
    for (int v = lane; v < nv; v += 64) {
      const f32x4 p = *(const f32x4*)(w + 4 * v) * lam;
      if (bf16_out) store_shadow((short*)e.Wf + row * e.cols, 4L * v, p);
      else *(f32x4*)((float*)e.Wf + row * e.cols + 4 * v) = p;
    }
    if (lane == 0) e.bf[row] = lam * e.b[row];
  }
}

template <bool ACC>
__global__ __launch_bounds__(STEP_BLOCK) void layer_scale_grad_kernel(const LsEntry* __restrict__ table) {
  const LsEntry e = table[blockIdx.y];  // block-uniform
  if (!e.dW_raw || !e.db_raw || !e.dW || !e.db || !e.dlambda) return;
  const int lane = threadIdx.x & 63, nv = e.cols >> 2;
  for (long row = blockIdx.x * (long)LS_WAVES + (threadIdx.x >> 6); row < e.rows; row += (long)gridDim.x * LS_WAVES) {
    const float lam = e.lambda[row];
    const float* __restrict__ w = e.W + row * e.cols;
    const float* __restrict__ g = e.dW_raw + row * e.cols;
    float* __restrict__ d = e.dW + row * e.cols;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    // a layer's launch has one wave or two per SIMD, so the loads in flight are the lane's own: LS_DEPTH trips' worth are
    // requested before the first is used (the chain's order, hence dlambda's bits, is that of the plain loop)
    int v = lane;
    for (; v + 64 * (LS_DEPTH - 1) < nv; v += 64 * LS_DEPTH) {
      f32x4 gg[LS_DEPTH], ww[LS_DEPTH], dd[LS_DEPTH];
#pragma unroll
      for (int u = 0; u < LS_DEPTH; ++u) {
        gg[u] = *(const f32x4*)(g + 4 * (v + 64 * u));
        ww[u] = *(const f32x4*)(w + 4 * (v + 64 * u));
        if (ACC) dd[u] = *(const f32x4*)(d + 4 * (v + 64 * u));
      }
#pragma unroll
      for (int u = 0; u < LS_DEPTH; ++u) {
#pragma unroll
        for (int k = 0; k < 4; ++k) acc[k] = fma_(gg[u][k], ww[u][k], acc[k]);
        *(f32x4*)(d + 4 * (v + 64 * u)) = ACC ? fma_(gg[u], lam, dd[u]) : gg[u] * lam;
      }
    }
    for (; v < nv; v += 64) {
      const f32x4 gg = *(const f32x4*)(g + 4 * v);
      const f32x4 ww = *(const f32x4*)(w + 4 * v);
#pragma unroll
      for (int k = 0; k < 4; ++k) acc[k] = fma_(gg[k], ww[k], acc[k]);
      *(f32x4*)(d + 4 * v) = ACC ? fma_(gg, lam, *(const f32x4*)(d + 4 * v)) : gg * lam;
    }
    const float dot = wave_sum((acc[0] + acc[1]) + (acc[2] + acc[3]));
    if (lane == 0) {
      const float gb = e.db_raw[row];
      const float dl = fma_(gb, e.b[row], dot), dbv = lam * gb;
      e.dlambda[row] = ACC ? e.dlambda[row] + dl : dl;
      e.db[row] = ACC ? e.db[row] + dbv : dbv;
      e.db_raw[row] = 0.f;  // the LayerNorm reducer ADDS into it in an accumulating backward
    }
  }
}

// The table is written from kernel arguments (no staging buffer the host could overwrite under a running step): up to
// LS_PER_WRITE entries by value, one 16-byte vector store per piece.
constexpr int LS_PER_WRITE = 32;
struct LsValues { u32x4 piece[LS_PER_WRITE * 6]; };
__global__ __launch_bounds__(LS_PER_WRITE * 6) void layer_scale_table_kernel(u32x4* __restrict__ table, int pieces, LsValues vals) {
  const int t = threadIdx.x;
  if (t < pieces) table[t] = vals.piece[t];
}

static bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// what both passes check of their launch, before anything goes out (the table's contents were checked when it was written)
static int ls_check(const char* who, const void* table, int n_entries, int max_rows) {
  VIT_CHECK(table, VIT_ERR_ARG, "%s: null pointer (table)", who);
  VIT_CHECK(aligned16(table), VIT_ERR_ARG, "%s: table must be 16-byte aligned", who);
  VIT_CHECK(n_entries > 0 && n_entries <= 65535, VIT_ERR_ARG, "%s: n_entries = %d must lie in [1, 65535]", who, n_entries);
  VIT_CHECK(max_rows > 0, VIT_ERR_ARG, "%s: max_rows = %d must be positive", who, max_rows);
  return VIT_OK;
}

static dim3 ls_grid(int n_entries, int max_rows) { return dim3(grid_for(max_rows, LS_WAVES, 1024), n_entries); }

}  // namespace vit

using namespace vit;

extern "C" {

int vit_layer_scale_table_write(vit_handle h, void* table, const vit_layer_scale_entry* entries, int count, vit_stream stream) {
  (void)h;
  const char* who = "vit_layer_scale_table_write";
  VIT_CHECK(table && entries, VIT_ERR_ARG, "%s: null pointer (table, entries)", who);
  VIT_CHECK(aligned16(table), VIT_ERR_ARG, "%s: table must be 16-byte aligned", who);
  VIT_CHECK(count > 0, VIT_ERR_ARG, "%s: count = %d must be positive", who, count);
  for (int i = 0; i < count; ++i) {
    const vit_layer_scale_entry& e = entries[i];
    VIT_CHECK(e.W && e.b && e.lambda, VIT_ERR_ARG, "%s: entry %d: null pointer (W, b, lambda)", who, i);
    const bool fold = e.Wf && e.bf, no_fold = !e.Wf && !e.bf;
    const bool grad = e.dW_raw && e.db_raw && e.dW && e.db && e.dlambda;
    const bool no_grad = !e.dW_raw && !e.db_raw && !e.dW && !e.db && !e.dlambda;
    VIT_CHECK((fold || no_fold) && (grad || no_grad) && (fold || grad), VIT_ERR_ARG,
              "%s: entry %d: null pointer in an output set ({Wf, bf} and / or {dW_raw, db_raw, dW, db, dlambda}, each complete)",
              who, i);
    VIT_CHECK(e.rows > 0, VIT_ERR_ARG, "%s: entry %d: rows = %d must be positive", who, i, e.rows);
    VIT_CHECK(e.cols > 0, VIT_ERR_ARG, "%s: entry %d: cols = %d must be positive", who, i, e.cols);
    VIT_CHECK(e.cols % 4 == 0, VIT_ERR_ARG, "%s: entry %d: cols = %d must be a multiple of 4", who, i, e.cols);
    VIT_CHECK(aligned16(e.W) && aligned16(e.Wf) && aligned16(e.dW_raw) && aligned16(e.dW), VIT_ERR_ARG,
              "%s: entry %d: W, Wf, dW_raw and dW must be 16-byte aligned", who, i);
  }
  for (int first = 0; first < count; first += LS_PER_WRITE) {
    const int n = count - first < LS_PER_WRITE ? count - first : LS_PER_WRITE;
    LsValues vals;
    memset(&vals, 0, sizeof vals);
    memcpy(vals.piece, entries + first, sizeof(vit_layer_scale_entry) * n);
    hipLaunchKernelGGL(layer_scale_table_kernel, dim3(1), dim3(LS_PER_WRITE * 6), 0, (hipStream_t)stream,
                       (u32x4*)table + 6 * (size_t)first, 6 * n, vals);
    VIT_LAUNCH_CHECK();
  }
  return VIT_OK;
}

int vit_layer_scale_fold(vit_handle h, const void* table, int n_entries, int max_rows, int out_dtype, vit_stream stream) {
  (void)h;
  if (int rc = ls_check("vit_layer_scale_fold", table, n_entries, max_rows)) return rc;
  VIT_CHECK(out_dtype == VIT_F32 || out_dtype == VIT_BF16, VIT_ERR_ARG, "vit_layer_scale_fold: bad out_dtype %d", out_dtype);
  hipLaunchKernelGGL(layer_scale_fold_kernel, ls_grid(n_entries, max_rows), dim3(STEP_BLOCK), 0, (hipStream_t)stream,
                     (const LsEntry*)table, out_dtype == VIT_BF16 ? 1 : 0);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_layer_scale_grad(vit_handle h, const void* table, int n_entries, int max_rows, int accumulate, vit_stream stream) {
  (void)h;
  if (int rc = ls_check("vit_layer_scale_grad", table, n_entries, max_rows)) return rc;
  VIT_CHECK(accumulate == 0 || accumulate == 1, VIT_ERR_ARG, "vit_layer_scale_grad: accumulate = %d must be 0 or 1", accumulate);
  const dim3 grid = ls_grid(n_entries, max_rows);
  if (accumulate)
    hipLaunchKernelGGL(layer_scale_grad_kernel<true>, grid, dim3(STEP_BLOCK), 0, (hipStream_t)stream, (const LsEntry*)table);
  else
    hipLaunchKernelGGL(layer_scale_grad_kernel<false>, grid, dim3(STEP_BLOCK), 0, (hipStream_t)stream, (const LsEntry*)table);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
