// Optimizer steps over a flat f32 parameter buffer for gfx950: AdamW, Adam with L2 decay, SGD (momentum / Nesterov).
// One pass each: the global-norm clip coefficient is applied to g on the fly, the bf16 shadow of p is written beside p.
// HBM-bound (14 / 22 / 30 B per parameter), 16 B per lane, grid-stride, scalar tail for n & 3, no atomics: deterministic.
// The `_dyn` forms (a step captured as a hipGraph) read what changes between replays from the handle's bound StepState.
#include <stdio.h>
#include <stdlib.h>

#include "common.h"

namespace vit {

__device__ __forceinline__ float clip_coef(const float* __restrict__ sqnorm, float max_norm) {
  return sqnorm ? fminf(1.f, max_norm / (sqrtf(sqnorm[0]) + 1e-6f)) : 1.f;
}

// torch.optim.AdamW (single-tensor form): p *= 1 - lr*wd; m,v EMA; p -= (lr/bc1) * m / (sqrt(v)/sqrt(bc2) + eps)
// L2 = torch.optim.Adam: weight_decay enters the gradient (g += wd * p, after the clip) and nothing decays p directly.
// DYN: lr, bc1, rsqrt_bc2 come from the step record instead of the arguments.
// omb1 / omb2: the EMA weights 1 - beta, formed on the host (one_minus): 1.f - beta for AdamW, torch's own for Adam.
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
  const long nv = n >> 2;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    f32x4 pp = *(const f32x4*)(p + 4 * i);
    f32x4 gg = *(const f32x4*)(g + 4 * i) * clip;
    if (L2) gg = gg + pp * wd;
    f32x4 mm = *(const f32x4*)(m + 4 * i);
    f32x4 vv = *(const f32x4*)(v + 4 * i);
    mm = mm * b1 + gg * omb1;
    vv = vv * b2 + gg * gg * omb2;
#pragma unroll
    for (int k = 0; k < 4; ++k) pp[k] = pp[k] * decay - step * mm[k] / (sqrtf(vv[k]) * rsqrt_bc2 + eps);
    *(f32x4*)(p + 4 * i) = pp;
    *(f32x4*)(m + 4 * i) = mm;
    *(f32x4*)(v + 4 * i) = vv;
    if (pb) {
      u32x2 pk = {pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3])};
      *(u32x2*)(pb + 4 * i) = pk;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (nv << 2) + threadIdx.x;
    float gg = g[i] * clip;
    if (L2) gg = gg + p[i] * wd;
    const float mm = m[i] * b1 + gg * omb1;
    const float vv = v[i] * b2 + gg * gg * omb2;
    const float pp = p[i] * decay - step * mm / (sqrtf(vv) * rsqrt_bc2 + eps);
    p[i] = pp; m[i] = mm; v[i] = vv;
    if (pb) pb[i] = f2bf(pp);
  }
}

// torch.optim.SGD (single-tensor form, dampening 0): g' = g*clip + wd*p; buf = mu*buf + g'; d = nesterov ? g' + mu*buf : buf;
// p -= lr*d.  A zero-filled buf gives torch's first step (buf = g') without a flag.  MOM = false: d = g', buf is not touched.
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
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < nv; i += (long)gridDim.x * blockDim.x) {
    f32x4 pp = *(const f32x4*)(p + 4 * i);
    f32x4 d = *(const f32x4*)(g + 4 * i) * clip;
    if (wd != 0.f) d = d + pp * wd;
    if (MOM) {
      const f32x4 bb = *(const f32x4*)(buf + 4 * i) * mu + d;
      *(f32x4*)(buf + 4 * i) = bb;
      d = nesterov ? d + bb * mu : bb;
    }
    pp = pp - d * lr;
    *(f32x4*)(p + 4 * i) = pp;
    if (pb) {
      u32x2 pk = {pack2bf(pp[0], pp[1]), pack2bf(pp[2], pp[3])};
      *(u32x2*)(pb + 4 * i) = pk;
    }
  }
  if (blockIdx.x == 0 && threadIdx.x < (n & 3)) {
    const long i = (nv << 2) + threadIdx.x;
    float pp = p[i];
    float d = g[i] * clip;
    if (wd != 0.f) d = d + pp * wd;
    if (MOM) {
      const float bb = buf[i] * mu + d;
      buf[i] = bb;
      d = nesterov ? d + bb * mu : bb;
    }
    pp = pp - d * lr;
    p[i] = pp;
    if (pb) pb[i] = f2bf(pp);
  }
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

}  // extern "C"
