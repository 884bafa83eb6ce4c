// Optimizer steps over a flat f32 parameter buffer for gfx950: AdamW, Adam with L2 decay, SGD (momentum / Nesterov).
// One pass each: the global-norm clip coefficient is applied to g on the fly, the bf16 shadow of p is written beside p.
// HBM-bound (14 / 22 / 30 B per parameter), 16 B per lane, grid-stride, scalar tail for n & 3, no atomics: deterministic.
// The `_dyn` forms (a step captured as a hipGraph) read what changes between replays from the handle's bound StepState.
// The `_groups` forms take lr / weight_decay / momentum per element from a segment table and a group table in device memory
// (torch.optim's param_groups in one launch); the update itself is stated once, below, for both.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace vit {

__device__ __forceinline__ float clip_coef(const float* __restrict__ sqnorm, float max_norm) {
  return sqnorm ? fminf(1.f, max_norm / (sqrtf(sqnorm[0]) + 1e-6f)) : 1.f;
}

// ---- the updates, stated once: T is f32x4 (the 16-byte body) or float (the n & 3 tail) ------------------------------------
__device__ __forceinline__ void store_shadow(short* __restrict__ pb, long at, f32x4 pp) {
  u32x2 pk = {pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3])};
  *(u32x2*)(pb + at) = pk;
}
__device__ __forceinline__ void store_shadow(short* __restrict__ pb, long at, float pp) { pb[at] = f2bf(pp); }

__device__ __forceinline__ f32x4 adam_descend(f32x4 pp, f32x4 mm, f32x4 vv, float decay, float step, float rsqrt_bc2, float eps) {
#pragma unroll
  for (int k = 0; k < 4; ++k) pp[k] = pp[k] * decay - step * mm[k] / (sqrtf(vv[k]) * rsqrt_bc2 + eps);
  return pp;
}
__device__ __forceinline__ float adam_descend(float pp, float mm, float vv, float decay, float step, float rsqrt_bc2, float eps) {
  return pp * decay - step * mm / (sqrtf(vv) * rsqrt_bc2 + eps);
}

// what Adam shares across a call (and across groups): the EMA weights, eps, the second bias correction
struct AdamShared { float b1, b2, omb1, omb2, eps, rsqrt_bc2; };

// torch.optim.AdamW (single-tensor form): p *= 1 - lr*wd; m,v EMA; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// L2 = torch.optim.Adam: weight_decay enters the gradient (g += wd * p, after the clip) and nothing decays p directly.
// omb1 / omb2: the EMA weights 1 - beta, formed on the host (one_minus): 1.f - beta for AdamW, torch's own for Adam.
// `at`: the element offset of this vector / element; step = lr / bc1, decay = L2 ? 1 : 1 - lr * wd.
template <bool L2, typename T>
__device__ __forceinline__ void adam_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, short* __restrict__ pb, long at, float clip,
                                            const AdamShared a, float step, float decay, float wd) {
  T pp = *(const T*)(p + at);
  T gg = *(const T*)(g + at) * clip;
  if (L2) gg = gg + pp * wd;
  T mm = *(const T*)(m + at);
  T vv = *(const T*)(v + at);
  mm = mm * a.b1 + gg * a.omb1;
  vv = vv * a.b2 + gg * gg * a.omb2;
  pp = adam_descend(pp, mm, vv, decay, step, a.rsqrt_bc2, a.eps);
  *(T*)(p + at) = pp;
  *(T*)(m + at) = mm;
  *(T*)(v + at) = vv;
  if (pb) store_shadow(pb, at, pp);
}

// torch.optim.SGD (single-tensor form, dampening 0): g' = g*clip + wd*p; buf = mu*buf + g'; d = nesterov ? g' + mu*buf : buf;
// p -= lr*d.  A zero-filled buf gives torch's first step (buf = g') without a flag.  MOM = false: d = g', buf is not touched.
template <bool MOM, typename T>
__device__ __forceinline__ void sgd_update(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                           short* __restrict__ pb, long at, float clip, float lr, float mu, float wd,
                                           int nesterov) {
  T pp = *(const T*)(p + at);
  T d = *(const T*)(g + at) * clip;
  if (wd != 0.f) d = d + pp * wd;
  if (MOM) {
    const T bb = *(const T*)(buf + at) * mu + d;
    *(T*)(buf + at) = bb;
    d = nesterov ? d + bb * mu : bb;
  }
  pp = pp - d * lr;
  *(T*)(p + at) = pp;
  if (pb) store_shadow(pb, at, pp);
}

// DYN: lr, bc1, rsqrt_bc2 come from the step record instead of the arguments.
template <bool L2, bool DYN>
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                    float* __restrict__ m, float* __restrict__ v,
                                                    short* __restrict__ pb, long n, float lr, float b1, float b2,
                                                    float omb1, float omb2, float eps, float wd, float bc1,
                                                    float rsqrt_bc2, const StepState* __restrict__ st,
                                                    const float* __restrict__ sqnorm, float max_norm) {
  const float clip = clip_coef(sqnorm, max_norm);
  if (DYN) {
    lr = st->lr; bc1 = st->bc1; rsqrt_bc2 = st->rsqrt_bc2;
  }
  const float step = lr / bc1, decay = L2 ? 1.f : 1.f - lr * wd;
  const AdamShared a = {b1, b2, omb1, omb2, eps, rsqrt_bc2};
  const long nv = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x)
    adam_update<L2, f32x4>(p, g, m, v, pb, 4 * i, clip, a, step, decay, wd);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) adam_update<L2, float>(p, g, m, v, pb, (nv << 2) + threadIdx.x, clip, a, step, decay, wd);
}

// DYN: lr and mu come from the step record.
template <bool MOM, bool DYN>
__global__ __launch_bounds__(256) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  short* __restrict__ pb, long n, float lr, float mu, float wd, int nesterov,
                                                  const StepState* __restrict__ st, const float* __restrict__ sqnorm,
                                                  float max_norm) {
  const float clip = clip_coef(sqnorm, max_norm);
  if (DYN) {
    lr = st->lr; mu = st->momentum;
  }
  const long nv = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x)
    sgd_update<MOM, f32x4>(p, g, buf, pb, 4 * i, clip, lr, mu, wd, nesterov);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) sgd_update<MOM, float>(p, g, buf, pb, (nv << 2) + threadIdx.x, clip, lr, mu, wd, nesterov);
}

// ---- parameter groups ------------------------------------------------------------------------------------------------------
// seg_end[n_seg]: ascending end offsets (elements, in the table's coordinates: p[0] sits at `base`); segment s covers
// [seg_end[s-1], seg_end[s]) and belongs to group seg_group[s]; every end but the last is a multiple of 4 and so is base, so a
// 16-byte vector never straddles a boundary.  rows[n_groups]: {lr, weight_decay, momentum, 0}.  Both tables are only read.
// Lookup: a block's 256 lanes cover one tile of 1024 consecutive elements per trip of the grid-stride loop.  The tile's first
// segment is found by one binary search on block-uniform values (scalar loads).  A tile that ends inside that segment -- all
// but ~n_seg of them -- takes the group's numbers from scalar registers and runs the plain kernel's body; a tile that crosses
// a boundary lets each lane walk on from the tile's first segment.  Offsets past the last end and group indices past the
// table are clamped, so a malformed table cannot make the kernel read outside it.
struct alignas(16) GroupRow { float lr, wd, mu, pad; };

__device__ __forceinline__ int seg_find(const long* __restrict__ seg_end, int n_seg, long off) {
  int lo = 0, hi = n_seg - 1;  // the first s with seg_end[s] > off, or the last segment
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (seg_end[mid] > off) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ GroupRow seg_row(const int* __restrict__ seg_group, const GroupRow* __restrict__ rows, int n_groups,
                                            int s) {
  const unsigned gi = (unsigned)seg_group[s];
  return rows[gi < (unsigned)n_groups ? gi : (unsigned)n_groups - 1u];
}

// calls body(at, row) for every 16-byte vector of [0, 4 * (n >> 2)) and tail(at, row) for the n & 3 elements behind them
template <typename Body, typename Tail>
__device__ __forceinline__ void for_each_grouped(long n, long base, const long* __restrict__ seg_end,
                                                 const int* __restrict__ seg_group, int n_seg,
                                                 const GroupRow* __restrict__ rows, int n_groups, Body body, Tail tail) {
  const long nv = n >> 2;
  for (long v0 = blockIdx.x * (long)blockDim.x; v0 < nv; v0 += (long)gridDim.x * blockDim.x) {  // block-uniform
    const long v1 = v0 + blockDim.x < nv ? v0 + blockDim.x : nv;
    const int s0 = seg_find(seg_end, n_seg, base + 4 * v0);
    const long i = v0 + threadIdx.x;
    if (s0 == n_seg - 1 || seg_end[s0] >= base + 4 * v1) {  // the whole tile lies in segment s0
      const GroupRow r = seg_row(seg_group, rows, n_groups, s0);
      if (i < v1) body(4 * i, r);
    } else if (i < v1) {
      int s = s0;
      while (s < n_seg - 1 && seg_end[s] <= base + 4 * i) ++s;
      body(4 * i, seg_row(seg_group, rows, n_groups, s));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (nv << 2) + threadIdx.x;
    tail(i, seg_row(seg_group, rows, n_groups, seg_find(seg_end, n_seg, base + i)));
  }
}

// DYN: bc1 and rsqrt_bc2 come from the step record; the learning rates are the table's in both forms.
template <bool L2, bool DYN>
__global__ __launch_bounds__(256) void adamw_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v,
                                                           short* __restrict__ pb, long n, long base,
                                                           const long* __restrict__ seg_end, const int* __restrict__ seg_group,
                                                           int n_seg, const GroupRow* __restrict__ rows, int n_groups, float b1,
                                                           float b2, float omb1, float omb2, float eps, float bc1,
                                                           float rsqrt_bc2, const StepState* __restrict__ st,
                                                           const float* __restrict__ sqnorm, float max_norm) {
  const float clip = clip_coef(sqnorm, max_norm);
  if (DYN) {
    bc1 = st->bc1; rsqrt_bc2 = st->rsqrt_bc2;
  }
  const AdamShared a = {b1, b2, omb1, omb2, eps, rsqrt_bc2};
  for_each_grouped(
      n, base, seg_end, seg_group, n_seg, rows, n_groups,
      [&](long at, GroupRow r) {
        adam_update<L2, f32x4>(p, g, m, v, pb, at, clip, a, r.lr / bc1, L2 ? 1.f : 1.f - r.lr * r.wd, r.wd);
      },
      [&](long at, GroupRow r) {
        adam_update<L2, float>(p, g, m, v, pb, at, clip, a, r.lr / bc1, L2 ? 1.f : 1.f - r.lr * r.wd, r.wd);
      });
}

// MOM: there is a momentum buffer; a group whose momentum is 0 still neither reads nor writes its part of it (vit_sgd_step
// with momentum 0 on that slice).
template <bool MOM>
__global__ __launch_bounds__(256) void sgd_groups_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                         float* __restrict__ buf, short* __restrict__ pb, long n, long base,
                                                         const long* __restrict__ seg_end, const int* __restrict__ seg_group,
                                                         int n_seg, const GroupRow* __restrict__ rows, int n_groups,
                                                         int nesterov, const float* __restrict__ sqnorm, float max_norm) {
  const float clip = clip_coef(sqnorm, max_norm);
  for_each_grouped(
      n, base, seg_end, seg_group, n_seg, rows, n_groups,
      [&](long at, GroupRow r) {
        if (MOM && r.mu != 0.f) sgd_update<true, f32x4>(p, g, buf, pb, at, clip, r.lr, r.mu, r.wd, nesterov);
        else sgd_update<false, f32x4>(p, g, buf, pb, at, clip, r.lr, r.mu, r.wd, 0);
      },
      [&](long at, GroupRow r) {
        if (MOM && r.mu != 0.f) sgd_update<true, float>(p, g, buf, pb, at, clip, r.lr, r.mu, r.wd, nesterov);
        else sgd_update<false, float>(p, g, buf, pb, at, clip, r.lr, r.mu, r.wd, 0);
      });
}

// The group table is written from kernel arguments (no staging buffer the host could overwrite under a running step): up to
// GROUPS_PER_WRITE rows of {lr, weight_decay, momentum} by value, one 16-byte vector store per row.
constexpr int GROUPS_PER_WRITE = 64;
struct GroupValues { float v[GROUPS_PER_WRITE * 3]; };
__global__ __launch_bounds__(GROUPS_PER_WRITE) void groups_write_kernel(GroupRow* __restrict__ rows, int count, GroupValues vals) {
  const int t = threadIdx.x;
  if (t >= count) return;
  const f32x4 row = {vals.v[3 * t], vals.v[3 * t + 1], vals.v[3 * t + 2], 0.f};
  *(f32x4*)(rows + t) = row;
}

// The EMA weight 1 - beta.  AdamW keeps 1.f - beta (the value its kernel always formed).  torch.optim.Adam's caller holds beta
// as a double and torch rounds 1 - beta to f32 AFTER the subtraction: float(1 - 0.999) = 0.001f, where 1.f - 0.999f =
// 0.00099998713 -- 1.3e-5 off, and exp_avg_sq with it.  The f32 that crosses the C ABI has lost those bits, so the double is
// read back from the shortest decimal that names this f32 (0.999f -> "0.999"; what the caller wrote, for every beta of up to
// 7 significant digits; otherwise the f32's own 9 digits, i.e. 1 - (double)beta).
template <bool L2>
static float one_minus(float beta) {
  if (!L2) return 1.f - beta;
  char text[32];
  for (int digits = 1; digits <= 9; ++digits) {
    snprintf(text, sizeof text, "%.*g", digits, (double)beta);
    if (strtof(text, nullptr) == beta) return (float)(1.0 - strtod(text, nullptr));
  }
  return (float)(1.0 - (double)beta);
}

template <bool L2>
static int adam_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* m, float* v, void* p_bf16,
                       int64_t n, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                       const float* sqnorm, float max_norm, vit_stream stream) {
  const StepState* st = dyn ? ctx_step_state(h) : nullptr;
  VIT_CHECK(!dyn || st, VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g && m && v && n > 0 && (dyn || step >= 1), VIT_ERR_ARG, "%s: bad arguments", who);
  const dim3 grid(grid_for(n / 4 + 1)), block(256);
  const float omb1 = one_minus<L2>(beta1), omb2 = one_minus<L2>(beta2);
  if (dyn) {
    hipLaunchKernelGGL((adamw_kernel<L2, true>), grid, block, 0, (hipStream_t)stream, p, g, m, v, (short*)p_bf16, (long)n, 0.f,
                       beta1, beta2, omb1, omb2, eps, weight_decay, 1.f, 1.f, st, sqnorm, max_norm);
  } else {
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    hipLaunchKernelGGL((adamw_kernel<L2, false>), grid, block, 0, (hipStream_t)stream, p, g, m, v, (short*)p_bf16, (long)n, lr,
                       beta1, beta2, omb1, omb2, eps, weight_decay, (float)bc1, (float)(1.0 / sqrt(bc2)), st, sqnorm, max_norm);
  }
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

static int sgd_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* buf, void* p_bf16, int64_t n,
                      float lr, float momentum, float weight_decay, int nesterov, const float* sqnorm, float max_norm,
                      vit_stream stream) {
  const StepState* st = dyn ? ctx_step_state(h) : nullptr;
  VIT_CHECK(!dyn || st, VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g, VIT_ERR_ARG, "%s: null pointer (p, g)", who);
  VIT_CHECK(n > 0, VIT_ERR_ARG, "%s: n = %lld must be positive", who, (long long)n);
  if (!dyn) {
    VIT_CHECK(momentum >= 0.f, VIT_ERR_ARG, "%s: momentum = %g is negative", who, (double)momentum);
    VIT_CHECK(momentum == 0.f || buf, VIT_ERR_ARG, "%s: momentum = %g needs a momentum buffer (buf is NULL)", who,
              (double)momentum);
    if (momentum == 0.f) buf = nullptr;  // torch.optim.SGD keeps no buffer then: neither read nor written
  }
  VIT_CHECK(!nesterov || buf, VIT_ERR_ARG, "%s: nesterov needs a momentum and its buffer", who);
  const dim3 grid(grid_for(n / 4 + 1)), block(256);
  hipStream_t s = (hipStream_t)stream;
  short* pb = (short*)p_bf16;
#define VIT_SGD(MOM, DYN)                                                                                              \
  hipLaunchKernelGGL((sgd_kernel<MOM, DYN>), grid, block, 0, s, p, g, buf, pb, (long)n, lr, momentum, weight_decay, nesterov, \
                     st, sqnorm, max_norm)
  if (buf) {
    if (dyn) VIT_SGD(true, true); else VIT_SGD(true, false);
  } else {
    if (dyn) VIT_SGD(false, true); else VIT_SGD(false, false);
  }
#undef VIT_SGD
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

// what every grouped entry point checks of its tables' description (their contents live on the device: the caller's job)
static int groups_check(const char* who, int64_t n, int64_t base, const int64_t* seg_end, const int32_t* seg_group,
                        int n_segments, const float* groups, int n_groups) {
  VIT_CHECK(n > 0, VIT_ERR_ARG, "%s: n = %lld must be positive", who, (long long)n);
  VIT_CHECK(seg_end && seg_group && groups, VIT_ERR_ARG, "%s: null table (seg_end, seg_group, groups)", who);
  VIT_CHECK(n_segments > 0 && n_groups > 0, VIT_ERR_ARG, "%s: n_segments = %d and n_groups = %d must be positive", who,
            n_segments, n_groups);
  VIT_CHECK(base >= 0 && base % 4 == 0, VIT_ERR_ARG, "%s: base = %lld must be a non-negative multiple of 4", who,
            (long long)base);
  return VIT_OK;
}

template <bool L2>
static int adam_groups_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* m, float* v,
                              void* p_bf16, int64_t n, int64_t base, const int64_t* seg_end, const int32_t* seg_group,
                              int n_segments, const float* groups, int n_groups, float beta1, float beta2, float eps, int step,
                              const float* sqnorm, float max_norm, vit_stream stream) {
  const StepState* st = dyn ? ctx_step_state(h) : nullptr;
  VIT_CHECK(!dyn || st, VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g && m && v && (dyn || step >= 1), VIT_ERR_ARG, "%s: bad arguments", who);
  if (int rc = groups_check(who, n, base, seg_end, seg_group, n_segments, groups, n_groups)) return rc;
  const dim3 grid(grid_for(n / 4 + 1)), block(256);
  const float omb1 = one_minus<L2>(beta1), omb2 = one_minus<L2>(beta2);
  const double bc1 = dyn ? 1.0 : 1.0 - pow((double)beta1, step), bc2 = dyn ? 1.0 : 1.0 - pow((double)beta2, step);
#define VIT_ADAM_GROUPS(DYN)                                                                                                  \
  hipLaunchKernelGGL((adamw_groups_kernel<L2, DYN>), grid, block, 0, (hipStream_t)stream, p, g, m, v, (short*)p_bf16, (long)n, \
                     (long)base, (const long*)seg_end, (const int*)seg_group, n_segments, (const GroupRow*)groups, n_groups,   \
                     beta1, beta2, omb1, omb2, eps, (float)bc1, (float)(1.0 / sqrt(bc2)), st, sqnorm, max_norm)
  if (dyn) VIT_ADAM_GROUPS(true); else VIT_ADAM_GROUPS(false);
#undef VIT_ADAM_GROUPS
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

static int sgd_groups_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* buf, void* p_bf16,
                             int64_t n, int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                             const float* groups, int n_groups, int nesterov, const float* sqnorm, float max_norm,
                             vit_stream stream) {
  VIT_CHECK(!dyn || ctx_step_state(h), VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g, VIT_ERR_ARG, "%s: null pointer (p, g)", who);
  if (int rc = groups_check(who, n, base, seg_end, seg_group, n_segments, groups, n_groups)) return rc;
  VIT_CHECK(!nesterov || buf, VIT_ERR_ARG, "%s: nesterov needs a momentum and its buffer", who);
  const dim3 grid(grid_for(n / 4 + 1)), block(256);
#define VIT_SGD_GROUPS(MOM)                                                                                                   \
  hipLaunchKernelGGL((sgd_groups_kernel<MOM>), grid, block, 0, (hipStream_t)stream, p, g, buf, (short*)p_bf16, (long)n,         \
                     (long)base, (const long*)seg_end, (const int*)seg_group, n_segments, (const GroupRow*)groups, n_groups,   \
                     nesterov, sqnorm, max_norm)
  if (buf) VIT_SGD_GROUPS(true); else VIT_SGD_GROUPS(false);
#undef VIT_SGD_GROUPS
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_adamw_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                   float max_norm, vit_stream stream) {
  return adam_launch<false>("vit_adamw_step", h, false, p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, step,
                            sqnorm, max_norm, stream);
}
int vit_adamw_step_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float beta1,
                       float beta2, float eps, float weight_decay, const float* sqnorm, float max_norm, vit_stream stream) {
  return adam_launch<false>("vit_adamw_step_dyn", h, true, p, g, m, v, p_bf16, n, 0.f, beta1, beta2, eps, weight_decay, 0,
                            sqnorm, max_norm, stream);
}
int vit_adam_l2_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                     float max_norm, vit_stream stream) {
  return adam_launch<true>("vit_adam_l2_step", h, false, p, g, m, v, p_bf16, n, lr, beta1, beta2, eps, weight_decay, step,
                           sqnorm, max_norm, stream);
}
int vit_adam_l2_step_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float beta1,
                         float beta2, float eps, float weight_decay, const float* sqnorm, float max_norm,
                         vit_stream stream) {
  return adam_launch<true>("vit_adam_l2_step_dyn", h, true, p, g, m, v, p_bf16, n, 0.f, beta1, beta2, eps, weight_decay, 0,
                           sqnorm, max_norm, stream);
}

int vit_sgd_step(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, float lr, float momentum,
                 float weight_decay, int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  return sgd_launch("vit_sgd_step", h, false, p, g, buf, p_bf16, n, lr, momentum, weight_decay, nesterov, sqnorm, max_norm,
                    stream);
}
int vit_sgd_step_dyn(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, float weight_decay,
                     int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  return sgd_launch("vit_sgd_step_dyn", h, true, p, g, buf, p_bf16, n, 0.f, 0.f, weight_decay, nesterov, sqnorm, max_norm,
                    stream);
}

int vit_adamw_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                          const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                          float beta1, float beta2, float eps, int step, const float* sqnorm, float max_norm,
                          vit_stream stream) {
  return adam_groups_launch<false>("vit_adamw_step_groups", h, false, p, g, m, v, p_bf16, n, base, seg_end, seg_group,
                                   n_segments, groups, n_groups, beta1, beta2, eps, step, sqnorm, max_norm, stream);
}
int vit_adamw_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                              int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                              const float* groups, int n_groups, float beta1, float beta2, float eps, const float* sqnorm,
                              float max_norm, vit_stream stream) {
  return adam_groups_launch<false>("vit_adamw_step_groups_dyn", h, true, p, g, m, v, p_bf16, n, base, seg_end, seg_group,
                                   n_segments, groups, n_groups, beta1, beta2, eps, 0, sqnorm, max_norm, stream);
}
int vit_adam_l2_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                            const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                            int n_groups, float beta1, float beta2, float eps, int step, const float* sqnorm, float max_norm,
                            vit_stream stream) {
  return adam_groups_launch<true>("vit_adam_l2_step_groups", h, false, p, g, m, v, p_bf16, n, base, seg_end, seg_group,
                                  n_segments, groups, n_groups, beta1, beta2, eps, step, sqnorm, max_norm, stream);
}
int vit_adam_l2_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                                int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                                const float* groups, int n_groups, float beta1, float beta2, float eps, const float* sqnorm,
                                float max_norm, vit_stream stream) {
  return adam_groups_launch<true>("vit_adam_l2_step_groups_dyn", h, true, p, g, m, v, p_bf16, n, base, seg_end, seg_group,
                                  n_segments, groups, n_groups, beta1, beta2, eps, 0, sqnorm, max_norm, stream);
}
int vit_sgd_step_groups(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, int64_t base,
                        const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                        int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  return sgd_groups_launch("vit_sgd_step_groups", h, false, p, g, buf, p_bf16, n, base, seg_end, seg_group, n_segments, groups,
                           n_groups, nesterov, sqnorm, max_norm, stream);
}
int vit_sgd_step_groups_dyn(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, int64_t base,
                            const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                            int n_groups, int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  return sgd_groups_launch("vit_sgd_step_groups_dyn", h, true, p, g, buf, p_bf16, n, base, seg_end, seg_group, n_segments,
                           groups, n_groups, nesterov, sqnorm, max_norm, stream);
}

int vit_optim_groups_write(vit_handle h, float* groups, int n_groups, const float* values, vit_stream stream) {
  (void)h;
  VIT_CHECK(groups && values, VIT_ERR_ARG, "vit_optim_groups_write: null pointer (groups, values)");
  VIT_CHECK(n_groups > 0, VIT_ERR_ARG, "vit_optim_groups_write: n_groups = %d must be positive", n_groups);
  for (int first = 0; first < n_groups; first += GROUPS_PER_WRITE) {
    const int count = n_groups - first < GROUPS_PER_WRITE ? n_groups - first : GROUPS_PER_WRITE;
    GroupValues vals;
    memset(&vals, 0, sizeof vals);
    memcpy(vals.v, values + 3 * (size_t)first, sizeof(float) * 3 * count);
    hipLaunchKernelGGL(groups_write_kernel, dim3(1), dim3(GROUPS_PER_WRITE), 0, (hipStream_t)stream,
                       (GroupRow*)groups + first, count, vals);
    VIT_LAUNCH_CHECK();
  }
  return VIT_OK;
}

}  // extern "C"
