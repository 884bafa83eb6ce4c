// Global average pooling of the token rows for gfx950 (include/vit_amd_pool.h): the mean of rows first .. T-1 of every sample
// and its backward.  Streaming kernels: 16 B per lane where D % 4 == 0, free of atomics, no workspace.  The forward's order of
// summation is the header's, a function of (T, first) alone.
#include <climits>

#include "common.h"

namespace vit {

constexpr int POOL_WAVES = 8;  // partial sums per (sample, column chunk): wave w takes rows first + w, first + w + 8, ...

template <int VEC> struct PoolVec;
template <> struct PoolVec<4> { typedef f32x4 type; };
template <> struct PoolVec<1> { typedef float type; };

// one workgroup per (b, chunk of 64 * VEC columns); wave w forms p_w in registers, wave 0 adds p_0 .. p_{W-1} in that order
template <int VEC>
__global__ __launch_bounds__(POOL_WAVES * 64) void token_pool_fwd_kernel(const float* __restrict__ x, float* __restrict__ pooled,
                                                                         int T, int D, int first, int nchunk, float inv) {
  typedef typename PoolVec<VEC>::type vec;
  __shared__ vec part[POOL_WAVES][64];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long b = blockIdx.x / nchunk;
  const int d = ((int)(blockIdx.x - b * nchunk) * 64 + lane) * VEC;  // D % VEC == 0: d < D means d + VEC <= D
  const int n = T - first, nw = min(POOL_WAVES, n);
  const bool live = d < D;
  if (live && w < nw) {
    const long step = (long)POOL_WAVES * D;
    const float* p = x + (b * T + first + w) * (long)D + d;
    const int cnt = (n - w + POOL_WAVES - 1) / POOL_WAVES;  // this wave's rows, >= 1
    vec acc = *(const vec*)p;
    int k = 1;
    for (; k + 4 <= cnt; k += 4) {  // four loads in flight, added in ascending row order
      const vec v0 = *(const vec*)(p + (k + 0) * step), v1 = *(const vec*)(p + (k + 1) * step);
      const vec v2 = *(const vec*)(p + (k + 2) * step), v3 = *(const vec*)(p + (k + 3) * step);
      acc += v0;
      acc += v1;
      acc += v2;
      acc += v3;
    }
    for (; k < cnt; ++k) acc += *(const vec*)(p + k * step);
    part[w][lane] = acc;
  }
  __syncthreads();
  if (live && w == 0) {
    vec s = part[0][lane];
    for (int k = 1; k < nw; ++k) s += part[k][lane];
    *(vec*)(pooled + b * D + d) = s * inv;
  }
}

// one wave per row r = b * T + t of dx: zeros in front of `first`, the sample's scaled dpooled row behind it
template <int VEC>
__global__ __launch_bounds__(256) void token_pool_bwd_kernel(const float* __restrict__ dpooled, float* __restrict__ dx, long rows,
                                                             int T, int D, int first, float inv) {
  typedef typename PoolVec<VEC>::type vec;
  const int lane = threadIdx.x & 63;
  for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < rows; r += gridDim.x * 4L) {
    const long b = r / T;
    const bool live = (int)(r - b * T) >= first;  // wave-uniform
    const float* g = dpooled + b * D;
    float* o = dx + r * D;
    for (int d = lane * VEC; d < D; d += 64 * VEC) {
      vec v = {};
      if (live) v = *(const vec*)(g + d) * inv;
      *(vec*)(o + d) = v;
    }
  }
}

static int pool_args_ok(const char* who, const void* a, const void* b, int B, int T, int D, int first) {
  VIT_CHECK(a && b, VIT_ERR_ARG, "%s: null pointer", who);
  VIT_CHECK(B >= 1 && T >= 1 && D >= 1, VIT_ERR_ARG, "%s: B=%d T=%d D=%d (each must be >= 1)", who, B, T, D);
  VIT_CHECK(first >= 0 && first < T, VIT_ERR_ARG, "%s: first=%d outside [0, T=%d)", who, first, T);
  return VIT_OK;
}

}  // namespace vit

extern "C" {
using namespace vit;

int vit_token_pool_fwd(vit_handle h, const float* x, float* pooled, int B, int T, int D, int first, vit_stream stream) {
  (void)h;
  const int rc = pool_args_ok("vit_token_pool_fwd", x, pooled, B, T, D, first);
  if (rc != VIT_OK) return rc;
  const int vec = (D % 4) == 0 ? 4 : 1;
  const int nchunk = cdiv(D, 64 * vec);
  VIT_CHECK((long)B * nchunk <= INT_MAX, VIT_ERR_ARG, "vit_token_pool_fwd: B=%d x %d column chunks exceed the grid", B, nchunk);
  const float inv = (float)(1.0 / (double)(T - first));
  const dim3 grid((unsigned)((long)B * nchunk)), block(POOL_WAVES * 64);
  if (vec == 4)
    hipLaunchKernelGGL(token_pool_fwd_kernel<4>, grid, block, 0, (hipStream_t)stream, x, pooled, T, D, first, nchunk, inv);
  else
    hipLaunchKernelGGL(token_pool_fwd_kernel<1>, grid, block, 0, (hipStream_t)stream, x, pooled, T, D, first, nchunk, inv);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_token_pool_bwd(vit_handle h, const float* dpooled, float* dx, int B, int T, int D, int first, vit_stream stream) {
  (void)h;
  const int rc = pool_args_ok("vit_token_pool_bwd", dpooled, dx, B, T, D, first);
  if (rc != VIT_OK) return rc;
  const long rows = (long)B * T;
  const float inv = (float)(1.0 / (double)(T - first));
  const dim3 grid(grid_for(rows, 4)), block(256);
  if ((D % 4) == 0)
    hipLaunchKernelGGL(token_pool_bwd_kernel<4>, grid, block, 0, (hipStream_t)stream, dpooled, dx, rows, T, D, first, inv);
  else
    hipLaunchKernelGGL(token_pool_bwd_kernel<1>, grid, block, 0, (hipStream_t)stream, dpooled, dx, rows, T, D, first, inv);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
