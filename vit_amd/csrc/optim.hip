// Optimizer steps over a flat f32 parameter buffer for gfx950: AdamW, Adam with L2 decay, SGD (momentum / Nesterov).
// One pass each: the global-norm clip coefficient is applied to g on the fly, the bf16 shadow of p is written beside p.
// HBM-bound (14 / 22 / 30 B per parameter), 16 B per lane, grid-stride, scalar tail for n & 3, no atomics: deterministic.
// One kernel per family.  The `_groups` forms take lr / weight_decay / momentum per element from a segment table and a group
// table in device memory (torch.optim's param_groups in one launch); the by-value forms are that kernel without a table, their
// scalars as its one row.  The `_groups_dyn` forms (a step captured as a hipGraph) read the bias corrections from the handle's
// bound StepState; what a scheduler changes between replays lives in the group table.
// LAMB (further down) is the one family that cannot be one pass: its per-tensor trust ratio needs two norms over the whole
// tensor before p may be written -- three launches, 42 B per parameter, a deterministic segmented reduction in between.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

// Every multiply-add that is fused is written as one (fma_): left to the compiler's contraction, the same source rounded
// differently in different kernels (fused in one loop, a packed multiply and a separate add in another), and the contract
// "bit-identical on any segment, through any entry point" held only by luck.
#pragma clang fp contract(off)

namespace vit {

__device__ __forceinline__ float clip_coef(const float* __restrict__ sqnorm, float max_norm) {
  return sqnorm ? fminf(1.f, max_norm / (sqrtf(sqnorm[0]) + 1e-6f)) : 1.f;
}

// ---- the updates, stated once: T is f32x4 (the 16-byte body) or float (the n & 3 tail) ------------------------------------
__device__ __forceinline__ f32x4 adam_descend(f32x4 pp, f32x4 mm, f32x4 vv, float decay, float step, float rsqrt_bc2, float eps) {
#pragma unroll
  for (int k = 0; k < 4; ++k) pp[k] = fma_(pp[k], decay, -(step * mm[k] / fma_(sqrtf(vv[k]), rsqrt_bc2, eps)));
  return pp;
}
__device__ __forceinline__ float adam_descend(float pp, float mm, float vv, float decay, float step, float rsqrt_bc2, float eps) {
  return fma_(pp, decay, -(step * mm / fma_(sqrtf(vv), rsqrt_bc2, eps)));
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
  if (L2) gg = fma_(pp, wd, gg);
  T mm = *(const T*)(m + at);
  T vv = *(const T*)(v + at);
  mm = fma_(mm, a.b1, gg * a.omb1);
  vv = fma_(vv, a.b2, gg * gg * a.omb2);
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
  if (wd != 0.f) d = fma_(pp, wd, d);
  if (MOM) {
    const T bb = fma_(*(const T*)(buf + at), mu, d);
    *(T*)(buf + at) = bb;
    d = nesterov ? fma_(bb, mu, d) : bb;
  }
  pp = fma_(d, -lr, pp);
  *(T*)(p + at) = pp;
  if (pb) store_shadow(pb, at, pp);
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

// calls body(at, prep(row)) for every 16-byte vector of [0, 4 * (n >> 2)) and tail(at, prep(row)) for the n & 3 elements behind
// them.  n_seg <= 1 is kernel-uniform: the row -- `row` itself without a table (n_seg == 0: the by-value entry points), the one
// segment's otherwise -- is taken and prepared once, and the body runs in the plain grid-stride loop.
template <typename Prep, typename Body, typename Tail>
__device__ __forceinline__ void for_each_grouped(long n, long base, const long* __restrict__ seg_end,
                                                 const int* __restrict__ seg_group, int n_seg,
                                                 const GroupRow* __restrict__ rows, int n_groups, GroupRow row, Prep prep,
                                                 Body body, Tail tail) {
  const long nv = n >> 2;
  if (n_seg <= 1) {
    if (n_seg == 1) row = seg_row(seg_group, rows, n_groups, 0);
    const auto k = prep(row);
    for (long i = blockIdx.x * (long)STEP_BLOCK + threadIdx.x; i < nv; i += (long)gridDim.x * STEP_BLOCK) body(4 * i, k);
    if (blockIdx.x == 0 && threadIdx.x < (n & 3)) tail((nv << 2) + threadIdx.x, k);
    return;
  }
  for (long v0 = blockIdx.x * (long)STEP_BLOCK; v0 < nv; v0 += (long)gridDim.x * STEP_BLOCK) {  // block-uniform
    const long v1 = v0 + STEP_BLOCK < nv ? v0 + STEP_BLOCK : nv;
    const int s0 = seg_find(seg_end, n_seg, base + 4 * v0);
    const long i = v0 + threadIdx.x;
    if (s0 == n_seg - 1 || seg_end[s0] >= base + 4 * v1) {  // the whole tile lies in segment s0
      const GroupRow r = seg_row(seg_group, rows, n_groups, s0);
      if (i < v1) body(4 * i, prep(r));
    } else if (i < v1) {
      int s = s0;
      while (s < n_seg - 1 && seg_end[s] <= base + 4 * i) ++s;
      body(4 * i, prep(seg_row(seg_group, rows, n_groups, s)));
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (nv << 2) + threadIdx.x;
    tail(i, prep(seg_row(seg_group, rows, n_groups, seg_find(seg_end, n_seg, base + i))));
  }
}

// One kernel per family.  `st` (a captured step) supplies the bias corrections and nothing else; learning rates, weight decays
// and momenta are the row's: the by-value `row` (n_seg == 0) or the group table's.
struct AdamRow { float step, decay, wd; };  // step = lr / bc1, decay = L2 ? 1 : 1 - lr * wd
template <bool L2>
__global__ __launch_bounds__(STEP_BLOCK) void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, short* __restrict__ pb, long n, long base,
                                                   const long* __restrict__ seg_end, const int* __restrict__ seg_group,
                                                   int n_seg, const GroupRow* __restrict__ rows, int n_groups, GroupRow row,
                                                   float b1, float b2, float omb1, float omb2, float eps, float bc1,
                                                   float rsqrt_bc2, const StepState* __restrict__ st,
                                                   const float* __restrict__ sqnorm, float max_norm) {
  const float clip = clip_coef(sqnorm, max_norm);
  if (st) {
    bc1 = st->bc1; rsqrt_bc2 = st->rsqrt_bc2;
  }
  const AdamShared a = {b1, b2, omb1, omb2, eps, rsqrt_bc2};
  for_each_grouped(
      n, base, seg_end, seg_group, n_seg, rows, n_groups, row,
      [&](GroupRow r) { return AdamRow{r.lr / bc1, L2 ? 1.f : fma_(-r.lr, r.wd, 1.f), r.wd}; },
      [&](long at, AdamRow k) { adam_update<L2, f32x4>(p, g, m, v, pb, at, clip, a, k.step, k.decay, k.wd); },
      [&](long at, AdamRow k) { adam_update<L2, float>(p, g, m, v, pb, at, clip, a, k.step, k.decay, k.wd); });
}

// MOM: there is a momentum buffer; a row whose momentum is 0 still neither reads nor writes its part of it.
template <bool MOM>
__global__ __launch_bounds__(STEP_BLOCK) void sgd_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ buf,
                                                  short* __restrict__ pb, long n, long base, const long* __restrict__ seg_end,
                                                  const int* __restrict__ seg_group, int n_seg,
                                                  const GroupRow* __restrict__ rows, int n_groups, GroupRow row, int nesterov,
                                                  const float* __restrict__ sqnorm, float max_norm) {
  const float clip = clip_coef(sqnorm, max_norm);
  for_each_grouped(
      n, base, seg_end, seg_group, n_seg, rows, n_groups, row, [](GroupRow r) { return r; },
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

// a grouped call's tables as its entry point received them; the by-value entry points pass none, and their scalars as `row`
struct GroupTable {
  int64_t base;
  const int64_t* seg_end;
  const int32_t* seg_group;
  int n_segments;
  const float* groups;
  int n_groups;
};

// what every grouped entry point checks of its tables' description (their contents live on the device: the caller's job)
static int groups_check(const char* who, int64_t n, const GroupTable& t) {
  VIT_CHECK(n > 0, VIT_ERR_ARG, "%s: n = %lld must be positive", who, (long long)n);
  VIT_CHECK(t.seg_end && t.seg_group && t.groups, VIT_ERR_ARG, "%s: null table (seg_end, seg_group, groups)", who);
  VIT_CHECK(t.n_segments > 0 && t.n_groups > 0, VIT_ERR_ARG, "%s: n_segments = %d and n_groups = %d must be positive", who,
            t.n_segments, t.n_groups);
  VIT_CHECK(t.base >= 0 && t.base % 4 == 0, VIT_ERR_ARG, "%s: base = %lld must be a non-negative multiple of 4", who,
            (long long)t.base);
  return VIT_OK;
}

template <bool L2>
static int adam_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* m, float* v, void* p_bf16,
                       int64_t n, const GroupTable* table, GroupRow row, float beta1, float beta2, float eps, int step,
                       const float* sqnorm, float max_norm, vit_stream stream) {
  const StepState* st = dyn ? ctx_step_state(h) : nullptr;
  VIT_CHECK(!dyn || st, VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g && m && v && (table || n > 0) && (dyn || step >= 1), VIT_ERR_ARG, "%s: bad arguments", who);
  if (table)
    if (int rc = groups_check(who, n, *table)) return rc;
  const GroupTable t = table ? *table : GroupTable{};
  const float omb1 = one_minus<L2>(beta1), omb2 = one_minus<L2>(beta2);
  const double bc1 = dyn ? 1.0 : 1.0 - pow((double)beta1, step), bc2 = dyn ? 1.0 : 1.0 - pow((double)beta2, step);
  hipLaunchKernelGGL((adam_kernel<L2>), dim3(grid_for(n / 4 + 1)), dim3(STEP_BLOCK), 0, (hipStream_t)stream, p, g, m, v,
                     (short*)p_bf16, (long)n, (long)t.base, (const long*)t.seg_end, (const int*)t.seg_group, t.n_segments,
                     (const GroupRow*)t.groups, t.n_groups, row, beta1, beta2, omb1, omb2, eps, (float)bc1,
                     (float)(1.0 / sqrt(bc2)), st, sqnorm, max_norm);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

static int sgd_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* buf, void* p_bf16, int64_t n,
                      const GroupTable* table, GroupRow row, int nesterov, const float* sqnorm, float max_norm,
                      vit_stream stream) {
  VIT_CHECK(!dyn || ctx_step_state(h), VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g, VIT_ERR_ARG, "%s: null pointer (p, g)", who);
  if (table) {
    if (int rc = groups_check(who, n, *table)) return rc;
  } else {
    VIT_CHECK(n > 0, VIT_ERR_ARG, "%s: n = %lld must be positive", who, (long long)n);
    VIT_CHECK(row.mu >= 0.f, VIT_ERR_ARG, "%s: momentum = %g is negative", who, (double)row.mu);
    VIT_CHECK(row.mu == 0.f || buf, VIT_ERR_ARG, "%s: momentum = %g needs a momentum buffer (buf is NULL)", who,
              (double)row.mu);
    if (row.mu == 0.f) buf = nullptr;  // torch.optim.SGD keeps no buffer then: neither read nor written
  }
  VIT_CHECK(!nesterov || buf, VIT_ERR_ARG, "%s: nesterov needs a momentum and its buffer", who);
  const GroupTable t = table ? *table : GroupTable{};
  const dim3 grid(grid_for(n / 4 + 1)), block(STEP_BLOCK);
#define VIT_SGD(MOM)                                                                                                          \
  hipLaunchKernelGGL((sgd_kernel<MOM>), grid, block, 0, (hipStream_t)stream, p, g, buf, (short*)p_bf16, (long)n, (long)t.base, \
                     (const long*)t.seg_end, (const int*)t.seg_group, t.n_segments, (const GroupRow*)t.groups, t.n_groups,     \
                     row, nesterov, sqnorm, max_norm)
  if (buf) VIT_SGD(true); else VIT_SGD(false);
#undef VIT_SGD
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

// ---- LAMB: per-tensor trust ratios over the flat buffer (include/vit_amd_optim.h) ---------------------------------------------
// One segment is one parameter tensor.  Three launches: (1) moments + one (sum p^2, sum u^2) pair per tile, (2) one wave per
// segment sums its tiles' pairs and writes trust[s], (3) u is recomputed -- lamb_u, the same function on the same stored m, v and
// the still untouched p, so bit for bit -- and p and the shadow are written.  Tiles: LAMB_TILE elements, cut from each segment's
// start, the last one short; a tile never straddles a segment, and which block works on it changes nothing it computes.
// Tile k of segment s owns slot (a_s - lo) / LAMB_TILE + (s - s_first) + k of the partial buffer ([lo, hi) the run, a_s the
// segment's start, s_first the run's first segment): strictly ascending over (s, k), computable from the table alone, below
// n / LAMB_TILE + n_segments + 1 -- which the host can size without reading the table.  Slots no tile owns are never read.
// Sums are f64 throughout (a lane's, a wave's butterfly, the block's four waves in order, a segment's tiles strided over one
// wave): cheap beside 24 B of traffic per element, and it leaves the norms' error to the f32 elements alone.
constexpr int LAMB_TILE = VIT_LAMB_TILE;

struct LambShared { float b1, b2, omb1, omb2, eps, bc1, rsqrt_bc2; };

// u = (m / bc1) / (sqrt(v) / sqrt(bc2) + eps) [+ wd * p]: the ONE statement of it, for pass 1's norm and pass 3's update
__device__ __forceinline__ float lamb_u(float pp, float mm, float vv, float wd, const LambShared a) {
  const float u = (mm / a.bc1) / fma_(sqrtf(vv), a.rsqrt_bc2, a.eps);
  return wd != 0.f ? fma_(pp, wd, u) : u;
}
__device__ __forceinline__ f32x4 lamb_u(f32x4 pp, f32x4 mm, f32x4 vv, float wd, const LambShared a) {
  f32x4 u;
#pragma unroll
  for (int k = 0; k < 4; ++k) u[k] = lamb_u(pp[k], mm[k], vv[k], wd, a);
  return u;
}
__device__ __forceinline__ void lamb_sq(double& acc, float x) { acc = __builtin_fma((double)x, (double)x, acc); }
__device__ __forceinline__ void lamb_sq(double& acc, f32x4 x) {
#pragma unroll
  for (int k = 0; k < 4; ++k) lamb_sq(acc, x[k]);
}
__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// pass 1 on one vector / element: the moments are stored, p and u enter the tile's sums
template <typename T>
__device__ __forceinline__ void lamb_moments(const float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                             float* __restrict__ v, long at, float clip, const LambShared a, float wd,
                                             double& sp, double& su) {
  const T pp = *(const T*)(p + at);
  const T gg = *(const T*)(g + at) * clip;
  T mm = *(const T*)(m + at);
  T vv = *(const T*)(v + at);
  mm = fma_(mm, a.b1, gg * a.omb1);
  vv = fma_(vv, a.b2, gg * gg * a.omb2);
  *(T*)(m + at) = mm;
  *(T*)(v + at) = vv;
  lamb_sq(sp, pp);
  lamb_sq(su, lamb_u(pp, mm, vv, wd, a));
}
// pass 3: p -= (lr * r) * u
template <typename T>
__device__ __forceinline__ void lamb_apply(float* __restrict__ p, const float* __restrict__ m, const float* __restrict__ v,
                                           short* __restrict__ pb, long at, const LambShared a, float wd, float step) {
  T pp = *(const T*)(p + at);
  pp = fma_(lamb_u(pp, *(const T*)(m + at), *(const T*)(v + at), wd, a), -step, pp);
  *(T*)(p + at) = pp;
  if (pb) store_shadow(pb, at, pp);
}

// the run [lo, hi) in the table's coordinates with its first and last segment; without a table one segment, [0, n)
struct LambRun { long lo, hi; int s_first, s_last; };
__device__ __forceinline__ LambRun lamb_run(long n, long base, const long* __restrict__ seg_end, int n_seg) {
  if (n_seg == 0) return {0, n, 0, 0};
  return {base, base + n, seg_find(seg_end, n_seg, base), seg_find(seg_end, n_seg, base + n - 1)};
}
__device__ __forceinline__ long lamb_clamp(const LambRun& r, long x) { return x < r.lo ? r.lo : x > r.hi ? r.hi : x; }
// segment s of the run, cut to the run (a run of whole segments cuts nothing), and its first slot
struct LambSeg { long a, b, slot0; };
__device__ __forceinline__ long lamb_seg_start(const LambRun& r, const long* __restrict__ seg_end, int s) {
  return s > r.s_first ? lamb_clamp(r, seg_end[s - 1]) : r.lo;
}
__device__ __forceinline__ long lamb_slot0(const LambRun& r, long a, int s) { return (a - r.lo) / LAMB_TILE + (s - r.s_first); }
__device__ __forceinline__ LambSeg lamb_seg(const LambRun& r, const long* __restrict__ seg_end, int s) {
  const long a = lamb_seg_start(r, seg_end, s);
  const long b = s < r.s_last ? lamb_clamp(r, seg_end[s]) : r.hi;
  return {a, b, lamb_slot0(r, a, s)};
}
// the tile that owns slot w: its segment and [lo, hi) (hi <= lo: no tile owns the slot)
struct LambTile { int s; long lo, hi; };
__device__ __forceinline__ LambTile lamb_tile(const LambRun& r, const long* __restrict__ seg_end, long w) {
  int lo = r.s_first, hi = r.s_last;  // the last s whose first slot is <= w (slot0 ascends strictly; s_first's is 0)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (lamb_slot0(r, lamb_seg_start(r, seg_end, mid), mid) <= w) lo = mid; else hi = mid - 1;
  }
  const LambSeg sg = lamb_seg(r, seg_end, lo);
  const long t0 = sg.a + (w - sg.slot0) * LAMB_TILE;
  return {lo, t0, t0 + LAMB_TILE < sg.b ? t0 + LAMB_TILE : sg.b};
}
// the group's row of a tile / segment; false: a segment no group owns (group index < 0), which no pass touches
__device__ __forceinline__ bool lamb_row(const int* __restrict__ seg_group, const GroupRow* __restrict__ rows, int n_groups,
                                         int n_seg, int s, GroupRow& row) {
  if (n_seg == 0) return true;
  if (seg_group[s] < 0) return false;
  row = seg_row(seg_group, rows, n_groups, s);
  return true;
}

__global__ __launch_bounds__(STEP_BLOCK) void lamb_moments_kernel(const float* __restrict__ p, const float* __restrict__ g,
                                                           float* __restrict__ m, float* __restrict__ v, long n, long base,
                                                           const long* __restrict__ seg_end, const int* __restrict__ seg_group,
                                                           int n_seg, const GroupRow* __restrict__ rows, int n_groups,
                                                           GroupRow row, LambShared a, const StepState* __restrict__ st,
                                                           const float* __restrict__ sqnorm, float max_norm,
                                                           double* __restrict__ part, long n_slots) {
  __shared__ double red[2 * (STEP_BLOCK / 64)];
  const float clip = clip_coef(sqnorm, max_norm);
  if (st) {
    a.bc1 = st->bc1; a.rsqrt_bc2 = st->rsqrt_bc2;
  }
  const LambRun r = lamb_run(n, base, seg_end, n_seg);
  for (long w = blockIdx.x; w < n_slots; w += gridDim.x) {  // block-uniform
    const LambTile t = lamb_tile(r, seg_end, w);
    if (t.hi <= t.lo || !lamb_row(seg_group, rows, n_groups, n_seg, t.s, row)) continue;
    const long at0 = t.lo - r.lo, len = t.hi - t.lo, nv = len >> 2;
    double sp = 0.0, su = 0.0;
    for (long i = threadIdx.x; i < nv; i += STEP_BLOCK) lamb_moments<f32x4>(p, g, m, v, at0 + 4 * i, clip, a, row.wd, sp, su);
    if (threadIdx.x < (len & 3)) lamb_moments<float>(p, g, m, v, at0 + (nv << 2) + threadIdx.x, clip, a, row.wd, sp, su);
    sp = wave_sum_f64(sp);
    su = wave_sum_f64(su);
    if ((threadIdx.x & 63) == 0) {
      red[2 * (threadIdx.x >> 6)] = sp;
      red[2 * (threadIdx.x >> 6) + 1] = su;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      double tp = red[0], tu = red[1];
      for (int k = 1; k < STEP_BLOCK / 64; ++k) { tp += red[2 * k]; tu += red[2 * k + 1]; }
      part[2 * w] = tp;
      part[2 * w + 1] = tu;
    }
    __syncthreads();  // `red` is free for the next tile
  }
}

// one wave per segment: r = adapt and ||p|| > 0 and ||u|| > 0 ? ||p|| / ||u|| : 1, min(r, 1) under trust_clip
__global__ __launch_bounds__(64) void lamb_ratio_kernel(long n, long base, const long* __restrict__ seg_end,
                                                      const int* __restrict__ seg_group, int n_seg,
                                                      const GroupRow* __restrict__ rows, int n_groups, GroupRow row,
                                                      int always_adapt, int trust_clip, const double* __restrict__ part,
                                                      float* __restrict__ trust) {
  const LambRun r = lamb_run(n, base, seg_end, n_seg);
  for (long s = (long)r.s_first + blockIdx.x; s <= r.s_last; s += gridDim.x) {
    if (!lamb_row(seg_group, rows, n_groups, n_seg, (int)s, row)) continue;
    const LambSeg sg = lamb_seg(r, seg_end, (int)s);
    if (sg.b <= sg.a) continue;
    const long tiles = (sg.b - sg.a + LAMB_TILE - 1) / LAMB_TILE;
    double sp = 0.0, su = 0.0;
    for (long k = threadIdx.x; k < tiles; k += 64) {
      sp += part[2 * (sg.slot0 + k)];
      su += part[2 * (sg.slot0 + k) + 1];
    }
    sp = wave_sum_f64(sp);
    su = wave_sum_f64(su);
    if (threadIdx.x == 0) {
      float ratio = 1.f;
      if ((row.wd != 0.f || always_adapt) && sp > 0.0 && su > 0.0) ratio = (float)(sqrt(sp) / sqrt(su));
      trust[s] = trust_clip ? fminf(ratio, 1.f) : ratio;
    }
  }
}

__global__ __launch_bounds__(STEP_BLOCK) void lamb_apply_kernel(float* __restrict__ p, const float* __restrict__ m,
                                                         const float* __restrict__ v, short* __restrict__ pb, long n, long base,
                                                         const long* __restrict__ seg_end, const int* __restrict__ seg_group,
                                                         int n_seg, const GroupRow* __restrict__ rows, int n_groups, GroupRow row,
                                                         LambShared a, const StepState* __restrict__ st,
                                                         const float* __restrict__ trust, long n_slots) {
  if (st) {
    a.bc1 = st->bc1; a.rsqrt_bc2 = st->rsqrt_bc2;
  }
  const LambRun r = lamb_run(n, base, seg_end, n_seg);
  for (long w = blockIdx.x; w < n_slots; w += gridDim.x) {  // block-uniform
    const LambTile t = lamb_tile(r, seg_end, w);
    if (t.hi <= t.lo || !lamb_row(seg_group, rows, n_groups, n_seg, t.s, row)) continue;
    const float step = row.lr * trust[t.s];
    const long at0 = t.lo - r.lo, len = t.hi - t.lo, nv = len >> 2;
    for (long i = threadIdx.x; i < nv; i += STEP_BLOCK) lamb_apply<f32x4>(p, m, v, pb, at0 + 4 * i, a, row.wd, step);
    if (threadIdx.x < (len & 3)) lamb_apply<float>(p, m, v, pb, at0 + (nv << 2) + threadIdx.x, a, row.wd, step);
  }
}

static int lamb_launch(const char* who, vit_handle h, bool dyn, float* p, const float* g, float* m, float* v, void* p_bf16,
                       int64_t n, const GroupTable* table, GroupRow row, float beta1, float beta2, float eps, int always_adapt,
                       int trust_clip, int step, const float* sqnorm, float max_norm, float* trust, vit_stream stream) {
  const StepState* st = dyn ? ctx_step_state(h) : nullptr;
  VIT_CHECK(!dyn || st, VIT_ERR_ARG, "%s: no step state bound (vit_step_state_bind)", who);
  VIT_CHECK(p && g && m && v && (table || n > 0) && (dyn || step >= 1), VIT_ERR_ARG, "%s: bad arguments", who);
  if (table) {
    if (int rc = groups_check(who, n, *table)) return rc;
    VIT_CHECK(trust, VIT_ERR_ARG, "%s: null trust (one f32 per segment of the table)", who);
  }
  const GroupTable t = table ? *table : GroupTable{};
  // slots of the partial buffer: what the tiles of ANY table of n_segments segments over n elements stay below
  const long n_slots = table ? (long)(n / LAMB_TILE) + t.n_segments + 1 : (long)((n + LAMB_TILE - 1) / LAMB_TILE);
  char* ws = (char*)ctx_claim(h, 16 + (size_t)n_slots * 2 * sizeof(double), who);
  if (!ws) return VIT_ERR_WORKSPACE;
  if (!trust) trust = (float*)ws;  // by value: the one ratio nobody asked for
  double* part = (double*)(ws + 16);
  const double bc1 = dyn ? 1.0 : 1.0 - pow((double)beta1, step), bc2 = dyn ? 1.0 : 1.0 - pow((double)beta2, step);
  const LambShared a = {beta1, beta2, 1.f - beta1, 1.f - beta2, eps, (float)bc1, (float)(1.0 / sqrt(bc2))};
  const dim3 grid(grid_for(n_slots, 1, 8192));
  hipStream_t s = (hipStream_t)stream;
  const int passes = ctx_lamb_passes(h);  // 7 unless a measurement asked for single passes (vit_handle_set_option)
  if (passes & 1) {
    hipLaunchKernelGGL(lamb_moments_kernel, grid, dim3(STEP_BLOCK), 0, s, p, g, m, v, (long)n, (long)t.base,
                       (const long*)t.seg_end, (const int*)t.seg_group, t.n_segments, (const GroupRow*)t.groups, t.n_groups, row,
                       a, st, sqnorm, max_norm, part, n_slots);
    VIT_LAUNCH_CHECK();
  }
  if (passes & 2) {
    hipLaunchKernelGGL(lamb_ratio_kernel, dim3(grid_for(table ? t.n_segments : 1, 1, 4096)), dim3(64), 0, s, (long)n,
                       (long)t.base, (const long*)t.seg_end, (const int*)t.seg_group, t.n_segments, (const GroupRow*)t.groups,
                       t.n_groups, row, always_adapt, trust_clip, part, trust);
    VIT_LAUNCH_CHECK();
  }
  if (passes & 4) {
    hipLaunchKernelGGL(lamb_apply_kernel, grid, dim3(STEP_BLOCK), 0, s, p, m, v, (short*)p_bf16, (long)n, (long)t.base,
                       (const long*)t.seg_end, (const int*)t.seg_group, t.n_segments, (const GroupRow*)t.groups, t.n_groups, row,
                       a, st, trust, n_slots);
    VIT_LAUNCH_CHECK();
  }
  return VIT_OK;
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_adamw_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                   float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                   float max_norm, vit_stream stream) {
  return adam_launch<false>("vit_adamw_step", h, false, p, g, m, v, p_bf16, n, nullptr, {lr, weight_decay, 0.f, 0.f}, beta1,
                            beta2, eps, step, sqnorm, max_norm, stream);
}
int vit_adam_l2_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr,
                     float beta1, float beta2, float eps, float weight_decay, int step, const float* sqnorm,
                     float max_norm, vit_stream stream) {
  return adam_launch<true>("vit_adam_l2_step", h, false, p, g, m, v, p_bf16, n, nullptr, {lr, weight_decay, 0.f, 0.f}, beta1,
                           beta2, eps, step, sqnorm, max_norm, stream);
}
int vit_sgd_step(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, float lr, float momentum,
                 float weight_decay, int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  return sgd_launch("vit_sgd_step", h, false, p, g, buf, p_bf16, n, nullptr, {lr, weight_decay, momentum, 0.f}, nesterov,
                    sqnorm, max_norm, stream);
}

int vit_adamw_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                          const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                          float beta1, float beta2, float eps, int step, const float* sqnorm, float max_norm,
                          vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return adam_launch<false>("vit_adamw_step_groups", h, false, p, g, m, v, p_bf16, n, &t, {}, beta1, beta2, eps, step, sqnorm,
                            max_norm, stream);
}
int vit_adamw_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                              int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                              const float* groups, int n_groups, float beta1, float beta2, float eps, const float* sqnorm,
                              float max_norm, vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return adam_launch<false>("vit_adamw_step_groups_dyn", h, true, p, g, m, v, p_bf16, n, &t, {}, beta1, beta2, eps, 0, sqnorm,
                            max_norm, stream);
}
int vit_adam_l2_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                            const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                            int n_groups, float beta1, float beta2, float eps, int step, const float* sqnorm, float max_norm,
                            vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return adam_launch<true>("vit_adam_l2_step_groups", h, false, p, g, m, v, p_bf16, n, &t, {}, beta1, beta2, eps, step, sqnorm,
                           max_norm, stream);
}
int vit_adam_l2_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n,
                                int64_t base, const int64_t* seg_end, const int32_t* seg_group, int n_segments,
                                const float* groups, int n_groups, float beta1, float beta2, float eps, const float* sqnorm,
                                float max_norm, vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return adam_launch<true>("vit_adam_l2_step_groups_dyn", h, true, p, g, m, v, p_bf16, n, &t, {}, beta1, beta2, eps, 0, sqnorm,
                           max_norm, stream);
}
int vit_sgd_step_groups(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, int64_t base,
                        const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                        int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return sgd_launch("vit_sgd_step_groups", h, false, p, g, buf, p_bf16, n, &t, {}, nesterov, sqnorm, max_norm, stream);
}
int vit_sgd_step_groups_dyn(vit_handle h, float* p, const float* g, float* buf, void* p_bf16, int64_t n, int64_t base,
                            const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                            int n_groups, int nesterov, const float* sqnorm, float max_norm, vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return sgd_launch("vit_sgd_step_groups_dyn", h, true, p, g, buf, p_bf16, n, &t, {}, nesterov, sqnorm, max_norm, stream);
}

int vit_lamb_step(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, float lr, float beta1,
                  float beta2, float eps, float weight_decay, int always_adapt, int trust_clip, int step, const float* sqnorm,
                  float max_norm, float* trust, vit_stream stream) {
  return lamb_launch("vit_lamb_step", h, false, p, g, m, v, p_bf16, n, nullptr, {lr, weight_decay, 0.f, 0.f}, beta1, beta2, eps,
                     always_adapt, trust_clip, step, sqnorm, max_norm, trust, stream);
}
int vit_lamb_step_groups(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                         const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups, int n_groups,
                         float beta1, float beta2, float eps, int always_adapt, int trust_clip, int step, const float* sqnorm,
                         float max_norm, float* trust, vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return lamb_launch("vit_lamb_step_groups", h, false, p, g, m, v, p_bf16, n, &t, {}, beta1, beta2, eps, always_adapt,
                     trust_clip, step, sqnorm, max_norm, trust, stream);
}
int vit_lamb_step_groups_dyn(vit_handle h, float* p, const float* g, float* m, float* v, void* p_bf16, int64_t n, int64_t base,
                             const int64_t* seg_end, const int32_t* seg_group, int n_segments, const float* groups,
                             int n_groups, float beta1, float beta2, float eps, int always_adapt, int trust_clip,
                             const float* sqnorm, float max_norm, float* trust, vit_stream stream) {
  const GroupTable t = {base, seg_end, seg_group, n_segments, groups, n_groups};
  return lamb_launch("vit_lamb_step_groups_dyn", h, true, p, g, m, v, p_bf16, n, &t, {}, beta1, beta2, eps, always_adapt,
                     trust_clip, 0, sqnorm, max_norm, trust, stream);
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
