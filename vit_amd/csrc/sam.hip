// Sharpness-aware minimisation over the flat f32 parameter buffer for gfx950 (include/vit_amd_sam.h): the norm of the first
// gradient, the ascent w' = w + rho * c * g / (norm + 1e-12) that keeps w in a backup buffer, and the descent that puts w back.
// HBM-bound (8 / 4, 16 (+2) and 8 (+2) B per parameter), 16 B per lane, grid-stride, scalar tail for n & 3, no atomics:
// deterministic, and on any 16-byte-aligned slice bit-identical to the whole-buffer call.
#include <math.h>

#include "common.h"

// as in optim.hip: every multiply-add that is fused is written as one (fma_)
#pragma clang fp contract(off)

namespace vit {

// one element: the step e = c * g * s is formed as (c * g) * s inside one fused multiply-add onto p; an element whose c * g is
// zero keeps p's bits (also the sign of a -0.0, which p + 0 would lose)
template <bool ADAPTIVE>
__device__ __forceinline__ float ascend_one(float p, float g, float s) {
  const float u = ADAPTIVE ? (p * p) * g : g;
  return u == 0.f ? p : fma_(u, s, p);
}

// g is read once and backup written once per step, neither is touched again before the second backward has streamed through
// every cache: both carry the non-temporal hint (measured: 284 -> 274 us over ViT-B's buffer, profiles/sam_bench.json)
template <bool ADAPTIVE>
__device__ __forceinline__ void ascend_vec(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                           short* __restrict__ pb, long at, float s) {
  const f32x4 pp = *(const f32x4*)(p + at);
  const f32x4 gg = __builtin_nontemporal_load((const f32x4*)(g + at));
  __builtin_nontemporal_store(pp, (f32x4*)(backup + at));
  f32x4 pn;
#pragma unroll
  for (int k = 0; k < 4; ++k) pn[k] = ascend_one<ADAPTIVE>(pp[k], gg[k], s);
  *(f32x4*)(p + at) = pn;
  if (pb) store_shadow(pb, at, pn);
}

template <bool ADAPTIVE>
__device__ __forceinline__ void ascend_scalar(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ backup,
                                              short* __restrict__ pb, long at, float s) {
  const float pp = p[at];
  backup[at] = pp;
  const float pn = ascend_one<ADAPTIVE>(pp, g[at], s);
  p[at] = pn;
  if (pb) store_shadow(pb, at, pn);
}

// s = rho / (sqrt(sqnorm[0]) + 1e-12) is read from device memory by every lane (a captured step freezes kernel arguments; the
// norm of the replay is whatever the reduction in front of this node left there)
template <bool ADAPTIVE>
__global__ __launch_bounds__(STEP_BLOCK) void sam_ascend_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                float* __restrict__ backup, short* __restrict__ pb, long n,
                                                                float rho, const float* __restrict__ sqnorm) {
  const float s = rho / (sqrtf(sqnorm[0]) + 1e-12f);
  const long nv = n >> 2;
  for (long i = blockIdx.x * (long)STEP_BLOCK + threadIdx.x; i < nv; i += (long)gridDim.x * STEP_BLOCK)
    ascend_vec<ADAPTIVE>(p, g, backup, pb, 4 * i, s);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) ascend_scalar<ADAPTIVE>(p, g, backup, pb, (nv << 2) + threadIdx.x, s);
}

template <typename T>
__device__ __forceinline__ void descend_one(float* __restrict__ p, const float* __restrict__ backup, short* __restrict__ pb,
                                            long at) {
  const T bb = *(const T*)(backup + at);
  *(T*)(p + at) = bb;
  if (pb) store_shadow(pb, at, bb);
}

__global__ __launch_bounds__(STEP_BLOCK) void sam_descend_kernel(float* __restrict__ p, const float* __restrict__ backup,
                                                                 short* __restrict__ pb, long n) {
  const long nv = n >> 2;
  for (long i = blockIdx.x * (long)STEP_BLOCK + threadIdx.x; i < nv; i += (long)gridDim.x * STEP_BLOCK)
    descend_one<f32x4>(p, backup, pb, 4 * i);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) descend_one<float>(p, backup, pb, (nv << 2) + threadIdx.x);
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_sam_sqnorm(vit_handle h, const float* p, const float* g, int64_t n, int adaptive, int accumulate, float* out,
                   vit_stream stream) {
  VIT_CHECK(g && out, VIT_ERR_ARG, "vit_sam_sqnorm: null pointer (g, out)");
  VIT_CHECK(n > 0, VIT_ERR_ARG, "vit_sam_sqnorm: n = %lld must be positive", (long long)n);
  VIT_CHECK(!adaptive || p, VIT_ERR_ARG, "vit_sam_sqnorm: the adaptive form needs p");
  VIT_CHECK((((uintptr_t)g | (uintptr_t)(adaptive ? p : nullptr)) & 15) == 0, VIT_ERR_ARG,
            "vit_sam_sqnorm: p and g must be 16-byte aligned");
  VIT_CHECK(((uintptr_t)out & 3) == 0, VIT_ERR_ARG, "vit_sam_sqnorm: out must be 4-byte aligned");
  return sqnorm_launch("vit_sam_sqnorm", h, adaptive ? p : nullptr, g, n, out, accumulate != 0, stream);
}

int vit_sam_ascend(vit_handle h, float* p, const float* g, float* backup, void* p_bf16, int64_t n, float rho, int adaptive,
                   const float* sqnorm_dev, vit_stream stream) {
  (void)h;
  VIT_CHECK(p && g && backup && sqnorm_dev, VIT_ERR_ARG, "vit_sam_ascend: null pointer (p, g, backup, sqnorm_dev)");
  VIT_CHECK(n > 0, VIT_ERR_ARG, "vit_sam_ascend: n = %lld must be positive", (long long)n);
  VIT_CHECK((((uintptr_t)p | (uintptr_t)g | (uintptr_t)backup) & 15) == 0, VIT_ERR_ARG,
            "vit_sam_ascend: p, g and backup must be 16-byte aligned");
  VIT_CHECK(((uintptr_t)p_bf16 & 7) == 0, VIT_ERR_ARG, "vit_sam_ascend: p_bf16 must be 8-byte aligned");
  VIT_CHECK(((uintptr_t)sqnorm_dev & 3) == 0, VIT_ERR_ARG, "vit_sam_ascend: sqnorm_dev must be 4-byte aligned");
  VIT_CHECK(isfinite(rho) && rho > 0.f, VIT_ERR_ARG, "vit_sam_ascend: rho = %g must be finite and positive", (double)rho);
  const dim3 grid(grid_for(n / 4 + 1)), block(STEP_BLOCK);
  if (adaptive)
    hipLaunchKernelGGL(sam_ascend_kernel<true>, grid, block, 0, (hipStream_t)stream, p, g, backup, (short*)p_bf16, (long)n, rho,
                       sqnorm_dev);
  else
    hipLaunchKernelGGL(sam_ascend_kernel<false>, grid, block, 0, (hipStream_t)stream, p, g, backup, (short*)p_bf16, (long)n, rho,
                       sqnorm_dev);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_sam_descend(vit_handle h, float* p, const float* backup, void* p_bf16, int64_t n, vit_stream stream) {
  (void)h;
  VIT_CHECK(p && backup, VIT_ERR_ARG, "vit_sam_descend: null pointer (p, backup)");
  VIT_CHECK(n > 0, VIT_ERR_ARG, "vit_sam_descend: n = %lld must be positive", (long long)n);
  VIT_CHECK((((uintptr_t)p | (uintptr_t)backup) & 15) == 0, VIT_ERR_ARG, "vit_sam_descend: p and backup must be 16-byte aligned");
  VIT_CHECK(((uintptr_t)p_bf16 & 7) == 0, VIT_ERR_ARG, "vit_sam_descend: p_bf16 must be 8-byte aligned");
  hipLaunchKernelGGL(sam_descend_kernel, dim3(grid_for(n / 4 + 1)), dim3(STEP_BLOCK), 0, (hipStream_t)stream, p, backup,
                     (short*)p_bf16, (long)n);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
