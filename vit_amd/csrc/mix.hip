// Mixup / CutMix of a batch of spectra [B, L] and of its labels for gfx950 (include/vit_amd_mix.h): the plan write, the signal
// pass and the target pass.  The signal pass is HBM-bound: one work item owns four elements of BOTH rows of a pair (b, B-1-b),
// 16 bytes per lane, and moves the bytes of a plain copy (copy form) or only what the plan changes (in place).  No atomics.
#include <math.h>
#include <string.h>

#include <algorithm>

#include "common.h"

// every multiply-add that is fused is written as one (fma_), as in optim.hip / ema.hip: the header states the rounding
#pragma clang fp contract(off)

namespace vit {

struct MixRow { float w, u; int lo, hi; float wy, uy; int r0, r1; };  // vit_mix_row
static_assert(sizeof(MixRow) == 32 && sizeof(vit_mix_row) == 32, "a plan row is two 16-byte vectors");

// ---- plan write: up to MIX_ROWS_PER_WRITE rows by value in the kernel arguments (2 KiB), two 16-byte stores per row
constexpr int MIX_ROWS_PER_WRITE = 64;
struct MixRowValues { MixRow r[MIX_ROWS_PER_WRITE]; };
__global__ __launch_bounds__(MIX_ROWS_PER_WRITE) void mix_plan_write_kernel(MixRow* __restrict__ rows, int count, MixRowValues vals) {
  const int t = threadIdx.x;
  if (t >= count) return;
  const MixRow r = vals.r[t];
  i32x4* o = (i32x4*)(rows + t);
  o[0] = (i32x4){__builtin_bit_cast(int, r.w), __builtin_bit_cast(int, r.u), r.lo, r.hi};
  o[1] = (i32x4){__builtin_bit_cast(int, r.wy), __builtin_bit_cast(int, r.uy), 0, 0};
}

// ---- signal
// 16 bytes at a 4-byte-aligned address (row p on row b's vector grid); ALIGNED: at a 16-byte-aligned one
template <bool ALIGNED>
__device__ __forceinline__ void load_elems(f32x4& v, const float* p) {
  if (ALIGNED) v = *(const f32x4*)p;
  else __builtin_memcpy(&v, p, 16);
}
template <bool ALIGNED>
__device__ __forceinline__ void load_elems(float& v, const float* p) { v = *p; }
template <bool ALIGNED>
__device__ __forceinline__ void store_elems(float* p, f32x4 v) {
  if (ALIGNED) *(f32x4*)p = v;
  else __builtin_memcpy(p, &v, 16);
}
template <bool ALIGNED>
__device__ __forceinline__ void store_elems(float* p, float v) { *p = v; }

// elements [i, i + 4) / element i of one output row: the partner's inside the span; outside it the row's own, or the mix
__device__ __forceinline__ f32x4 mix_vals(f32x4 own, f32x4 par, int i, const MixRow& r, bool mix) {
  f32x4 o;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const bool in = i + k >= r.lo && i + k < r.hi;
    const float m = mix ? fma_(r.w, own[k], r.u * par[k]) : own[k];
    o[k] = in ? par[k] : m;
  }
  return o;
}
__device__ __forceinline__ float mix_vals(float own, float par, int i, const MixRow& r, bool mix) {
  const float m = mix ? fma_(r.w, own, r.u * par) : own;
  return (i >= r.lo && i < r.hi) ? par : m;
}

// what elements [e0, e1) of one row of a pair need, from the plan alone (wave-uniform where e0, e1 are):
//   mix: outside the span the row is w * own + u * partner;  par: the partner's elements are read for it;
//   write: the row's elements are stored (copy form: always; in place: only where something changes);
//   own: the row's own elements are read for it (not where the span covers them all)
struct RowNeeds { bool mix, par, write, own; };
template <bool INPLACE>
__device__ __forceinline__ RowNeeds row_needs(const MixRow& r, int e0, int e1, bool paired) {
  RowNeeds n;
  n.mix = paired && r.u != 0.f;
  const bool span_hit = (r.lo > e0 ? r.lo : e0) < (r.hi < e1 ? r.hi : e1);
  n.par = paired && (n.mix || span_hit);
  n.write = INPLACE ? n.par : true;
  n.own = n.write && !(paired && r.lo <= e0 && r.hi >= e1);
  return n;
}

// one work item: V = f32x4 (elements [i, i + 4), row b's accesses 16-byte aligned) or float (element i)
template <typename V>
__device__ __forceinline__ void mix_pair(const float* xb, const float* xp, float* ob, float* op, int i,
                                         const MixRow& rb, const MixRow& rp, RowNeeds nb, RowNeeds np, bool paired) {
  V vb = {}, vp = {};
  if (nb.own || (paired && np.par)) load_elems<true>(vb, xb + i);
  if (paired && (np.own || nb.par)) load_elems<false>(vp, xp + i);
  // both rows are in registers before either is stored: the in-place form (ob == xb, op == xp) has no hazard
  if (nb.write) store_elems<true>(ob + i, mix_vals(vb, vp, i, rb, nb.mix));
  if (paired && np.write) store_elems<false>(op + i, mix_vals(vp, vb, i, rp, np.mix));
}

// grid: x = chunks of 4 waves x 256 elements along the row, y = pairs (b, B - 1 - b); the middle row of an odd B is its own
// partner and stays what it is.  x and out may be the same buffer (no __restrict__); both are 16-byte aligned, so row b's 16-byte grid starts `head` elements into the row.
template <bool INPLACE>
__global__ __launch_bounds__(256) void mix_signal_kernel(const float* x, float* out, const MixRow* __restrict__ plan,
                                                         int per_sample, int B, int L) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
  const int pairs = (B + 1) >> 1;
  for (int b = blockIdx.y; b < pairs; b += gridDim.y) {
    const int p = B - 1 - b;
    const bool paired = p != b;
    MixRow rb = plan[per_sample ? b : 0], rp = plan[per_sample ? p : 0];
    rb.lo = min(max(rb.lo, 0), L); rb.hi = min(max(rb.hi, 0), L);
    rp.lo = min(max(rp.lo, 0), L); rp.hi = min(max(rp.hi, 0), L);
    if (!paired) rb.lo = rb.hi = 0;  // its span would be its own elements
    const float* xb = x + (long)b * L;
    const float* xp = x + (long)p * L;
    float* ob = out + (long)b * L;
    float* op = out + (long)p * L;
    const int head = min((int)((4 - (((long)b * L) & 3)) & 3), L);
    const int nv = (L - head) >> 2, tail0 = head + 4 * nv;
    for (int c = blockIdx.x * 4 + wave; c * 64 < nv; c += gridDim.x * 4) {
      const int e0 = head + c * 256, e1 = min(e0 + 256, tail0);
      const RowNeeds nb = row_needs<INPLACE>(rb, e0, e1, paired), np = row_needs<INPLACE>(rp, e0, e1, paired);
      if (!(nb.write || (paired && np.write))) continue;  // in place: nothing of this chunk changes
      const int k = c * 64 + lane;
      if (k < nv) mix_pair<f32x4>(xb, xp, ob, op, head + 4 * k, rb, rp, nb, np, paired);
    }
    if (blockIdx.x == 0 && wave == 0) {  // the up to 3 elements in front of and behind the vectors, one lane each
      int i = -1;
      if (lane < head) i = lane;
      else if (lane >= 32 && lane - 32 < L - tail0) i = tail0 + (lane - 32);
      if (i >= 0) {
        const RowNeeds nb = row_needs<INPLACE>(rb, i, i + 1, paired), np = row_needs<INPLACE>(rp, i, i + 1, paired);
        mix_pair<float>(xb, xp, ob, op, i, rb, rp, nb, np, paired);
      }
    }
  }
}

// ---- targets: one element of out [B, C] per work item
template <bool CLASSES>
__global__ __launch_bounds__(256) void mix_targets_kernel(const void* __restrict__ labels, float* __restrict__ out,
                                                          const MixRow* __restrict__ plan, int per_sample, int B, int C, float on,
                                                          float off) {
  const long total = (long)B * C;
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / C), c = (int)(i - (long)b * C), p = B - 1 - b;
    const MixRow r = plan[per_sample ? b : 0];
    float own, par = 0.f;
    if (CLASSES) {
      const long long* y = (const long long*)labels;
      own = y[b] == c ? on : off;
      if (r.uy != 0.f) par = y[p] == c ? on : off;
    } else {
      const float* y = (const float*)labels;
      own = y[i];
      if (r.uy != 0.f) par = y[(long)p * C + c];
    }
    out[i] = r.uy != 0.f ? fma_(r.wy, own, r.uy * par) : own;
  }
}

static bool overlap(const void* a, size_t na, const void* b, size_t nb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + nb && b0 < a0 + na;
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_mix_plan_write(vit_handle h, void* plan_dev, int n_rows, const vit_mix_row* host_rows, vit_stream stream) {
  (void)h;
  VIT_CHECK(plan_dev && host_rows, VIT_ERR_ARG, "vit_mix_plan_write: null pointer (plan_dev, host_rows)");
  VIT_CHECK(n_rows > 0, VIT_ERR_ARG, "vit_mix_plan_write: n_rows = %d must be positive", n_rows);
  VIT_CHECK(((uintptr_t)plan_dev & 15) == 0, VIT_ERR_ARG, "vit_mix_plan_write: plan_dev must be 16-byte aligned");
  for (int first = 0; first < n_rows; first += MIX_ROWS_PER_WRITE) {
    const int count = n_rows - first < MIX_ROWS_PER_WRITE ? n_rows - first : MIX_ROWS_PER_WRITE;
    MixRowValues vals;
    memset(&vals, 0, sizeof vals);
    memcpy(vals.r, host_rows + first, sizeof(MixRow) * count);
    hipLaunchKernelGGL(mix_plan_write_kernel, dim3(1), dim3(MIX_ROWS_PER_WRITE), 0, (hipStream_t)stream,
                       (MixRow*)plan_dev + first, count, vals);
    VIT_LAUNCH_CHECK();
  }
  return VIT_OK;
}

int vit_mix_signal(vit_handle h, const float* x, float* out, const void* plan_dev, int n_rows, int B, int L,
                   vit_stream stream) {
  (void)h;
  VIT_CHECK(x && out && plan_dev, VIT_ERR_ARG, "vit_mix_signal: null pointer (x, out, plan_dev)");
  VIT_CHECK(B > 0 && L > 0, VIT_ERR_ARG, "vit_mix_signal: B = %d, L = %d must be positive", B, L);
  VIT_CHECK(n_rows == 1 || n_rows == B, VIT_ERR_ARG, "vit_mix_signal: n_rows = %d must be 1 or B = %d", n_rows, B);
  VIT_CHECK((((uintptr_t)x | (uintptr_t)out | (uintptr_t)plan_dev) & 15) == 0, VIT_ERR_ARG,
            "vit_mix_signal: x, out and plan_dev must be 16-byte aligned");
  const size_t bytes = (size_t)B * L * sizeof(float);
  VIT_CHECK(x == out || !overlap(x, bytes, out, bytes), VIT_ERR_ARG,
            "vit_mix_signal: x and out overlap partially (out == x is the in-place form)");
  const int pairs = (B + 1) / 2;
  const dim3 grid(std::min(cdiv(cdiv(L, 4), 256), 1024), std::min(pairs, 32768));
  if (x == out)
    hipLaunchKernelGGL(mix_signal_kernel<true>, grid, dim3(256), 0, (hipStream_t)stream, x, out, (const MixRow*)plan_dev,
                       n_rows > 1 || B == 1 ? 1 : 0, B, L);
  else
    hipLaunchKernelGGL(mix_signal_kernel<false>, grid, dim3(256), 0, (hipStream_t)stream, x, out, (const MixRow*)plan_dev,
                       n_rows > 1 || B == 1 ? 1 : 0, B, L);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_mix_targets(vit_handle h, const void* labels, int label_kind, float* out, const void* plan_dev, int n_rows, int B,
                    int C, float on, float off, vit_stream stream) {
  (void)h;
  VIT_CHECK(labels && out && plan_dev, VIT_ERR_ARG, "vit_mix_targets: null pointer (labels, out, plan_dev)");
  VIT_CHECK(label_kind == VIT_MIX_LABELS_F32 || label_kind == VIT_MIX_LABELS_I64, VIT_ERR_ARG,
            "vit_mix_targets: label_kind = %d is neither VIT_MIX_LABELS_F32 nor VIT_MIX_LABELS_I64", label_kind);
  VIT_CHECK(B > 0, VIT_ERR_ARG, "vit_mix_targets: B = %d must be positive", B);
  VIT_CHECK(C > 0, VIT_ERR_ARG, "vit_mix_targets: C = %d must be positive", C);
  VIT_CHECK(n_rows == 1 || n_rows == B, VIT_ERR_ARG, "vit_mix_targets: n_rows = %d must be 1 or B = %d", n_rows, B);
  const bool classes = label_kind == VIT_MIX_LABELS_I64;
  VIT_CHECK((((uintptr_t)out | (uintptr_t)plan_dev) & 15) == 0 && ((uintptr_t)labels & (classes ? 7 : 3)) == 0, VIT_ERR_ARG,
            "vit_mix_targets: out and plan_dev must be 16-byte aligned, labels to their element size");
  VIT_CHECK(!overlap(labels, classes ? (size_t)B * 8 : (size_t)B * C * 4, out, (size_t)B * C * 4), VIT_ERR_ARG,
            "vit_mix_targets: out overlaps labels");
  if (classes) VIT_CHECK(isfinite(on) && isfinite(off), VIT_ERR_ARG, "vit_mix_targets: on = %g, off = %g must be finite", (double)on, (double)off);
  const int per_sample = n_rows > 1 || B == 1 ? 1 : 0;
  const int blocks = grid_for((long)B * C);
  if (classes)
    hipLaunchKernelGGL(mix_targets_kernel<true>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, labels, out,
                       (const MixRow*)plan_dev, per_sample, B, C, on, off);
  else
    hipLaunchKernelGGL(mix_targets_kernel<false>, dim3(blocks), dim3(256), 0, (hipStream_t)stream, labels, out,
                       (const MixRow*)plan_dev, per_sample, B, C, on, off);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
