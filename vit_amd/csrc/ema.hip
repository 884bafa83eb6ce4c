// Exponential moving average of the flat f32 parameter buffer for gfx950: the update ema <- lerp(ema, p, w) and the exchange
// of the two buffers (evaluation on the average, in place: parameters are views of the flat buffer and captured graphs hold
// raw addresses, so data moves and addresses stay).  HBM-bound (12 and 16 (+2) B per parameter), 16 B per lane, grid-stride,
// scalar tail for n & 3, no atomics: deterministic, and on any 16-byte-aligned slice bit-identical to the whole-buffer call.
#include <math.h>

#include "common.h"

// as in optim.hip: every multiply-add that is fused is written as one (fma_)
#pragma clang fp contract(off)

namespace vit {

// torch.lerp(ema, p, w): w < 0.5 ? ema + w * (p - ema) : p - (p - ema) * (1 - w).  T is f32x4 (the 16-byte body) or float (the
// n & 3 tail).  COPY (w == 1, the first update): ema is not read -- p - (p - ema) * 0 is p only while p - ema is finite.
template <bool COPY, typename T>
__device__ __forceinline__ void ema_update(float* __restrict__ ema, const float* __restrict__ p, long at, float w, float omw) {
  const T pp = *(const T*)(p + at);
  if (COPY) {
    *(T*)(ema + at) = pp;
    return;
  }
  const T ee = *(const T*)(ema + at);
  const T d = pp - ee;
  *(T*)(ema + at) = w < 0.5f ? fma_(d, w, ee) : fma_(d, -omw, pp);
}

template <bool COPY>
__device__ __forceinline__ void ema_pass(float* __restrict__ ema, const float* __restrict__ p, long n, float w) {
  const long nv = n >> 2;
  const float omw = 1.f - w;
  for (long i = blockIdx.x * (long)STEP_BLOCK + threadIdx.x; i < nv; i += (long)gridDim.x * STEP_BLOCK)
    ema_update<COPY, f32x4>(ema, p, 4 * i, w, omw);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) ema_update<COPY, float>(ema, p, (nv << 2) + threadIdx.x, w, omw);
}

// wdev (a captured step: kernel arguments are frozen, the weight of this replay is in device memory) overrides w.  w == 0 -- a
// step the schedule skips -- returns before anything is loaded; the branch is kernel-uniform.
__global__ __launch_bounds__(STEP_BLOCK) void ema_update_kernel(float* __restrict__ ema, const float* __restrict__ p, long n,
                                                                float w, const float* __restrict__ wdev) {
  if (wdev) w = wdev[0];
  if (w == 0.f) return;
  if (w == 1.f) ema_pass<true>(ema, p, n, w);
  else ema_pass<false>(ema, p, n, w);
}

template <typename T>
__device__ __forceinline__ void swap_one(float* __restrict__ p, float* __restrict__ ema, short* __restrict__ pb, long at) {
  const T pp = *(const T*)(p + at);
  const T ee = *(const T*)(ema + at);
  *(T*)(p + at) = ee;
  *(T*)(ema + at) = pp;
  if (pb) store_shadow(pb, at, ee);
}

__global__ __launch_bounds__(STEP_BLOCK) void ema_swap_kernel(float* __restrict__ p, float* __restrict__ ema,
                                                              short* __restrict__ pb, long n) {
  const long nv = n >> 2;
  for (long i = blockIdx.x * (long)STEP_BLOCK + threadIdx.x; i < nv; i += (long)gridDim.x * STEP_BLOCK)
    swap_one<f32x4>(p, ema, pb, 4 * i);
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) swap_one<float>(p, ema, pb, (nv << 2) + threadIdx.x);
}

// what both entry points check of their buffers, before anything is launched
static int ema_check(const char* who, const float* a, const float* b, const void* shadow, int64_t n) {
  VIT_CHECK(a && b, VIT_ERR_ARG, "%s: null pointer (ema, p)", who);
  VIT_CHECK(n > 0, VIT_ERR_ARG, "%s: n = %lld must be positive", who, (long long)n);
  VIT_CHECK((((uintptr_t)a | (uintptr_t)b) & 15) == 0, VIT_ERR_ARG, "%s: ema and p must be 16-byte aligned", who);
  VIT_CHECK(((uintptr_t)shadow & 7) == 0, VIT_ERR_ARG, "%s: p_bf16 must be 8-byte aligned", who);
  return VIT_OK;
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_ema_update(vit_handle h, float* ema, const float* p, int64_t n, float weight, const float* weight_dev,
                   vit_stream stream) {
  (void)h;
  if (int rc = ema_check("vit_ema_update", ema, p, nullptr, n)) return rc;
  if (weight_dev)
    VIT_CHECK(((uintptr_t)weight_dev & 15) == 0, VIT_ERR_ARG, "vit_ema_update: weight_dev must be 16-byte aligned");
  else
    VIT_CHECK(isfinite(weight) && weight >= 0.f && weight <= 1.f, VIT_ERR_ARG,
              "vit_ema_update: weight = %g must lie in [0, 1] (1 - decay, subtracted by the caller)", (double)weight);
  hipLaunchKernelGGL(ema_update_kernel, dim3(grid_for(n / 4 + 1)), dim3(STEP_BLOCK), 0, (hipStream_t)stream, ema, p, (long)n,
                     weight, weight_dev);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_ema_swap(vit_handle h, float* p, float* ema, void* p_bf16, int64_t n, vit_stream stream) {
  (void)h;
  if (int rc = ema_check("vit_ema_swap", ema, p, p_bf16, n)) return rc;
  hipLaunchKernelGGL(ema_swap_kernel, dim3(grid_for(n / 4 + 1)), dim3(STEP_BLOCK), 0, (hipStream_t)stream, p, ema,
                     (short*)p_bf16, (long)n);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
