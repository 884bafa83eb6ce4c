// Masked spectrum modelling for gfx950 (include/vit_amd_mim.h): the block mask, the embedding finish that substitutes the mask
// token and its backward -- twins of embed_finish_kernel / embed_finish_bwd_kernel of elementwise.hip, same walk, same sums --
// and the reconstruction loss that reads its target windows straight from the signal.
// Like their plain twins: vectorised (8-16 B per lane), free of float atomics; a mask value is only ever compared with zero,
// never turned into an address.
#include <algorithm>

#include "common.h"

namespace vit {

// ------------------------------------------------------------------------------------------ block selection -> patch mask
__global__ void mim_mask_kernel(const int* __restrict__ slot_blocks, int* __restrict__ mask, int B, int N, int Nb, int span) {
  const long total = (long)B * N;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const long b = i / N;
    const int n = (int)(i - b * N);
    mask[i] = slot_blocks[b * Nb + n / span] < 0 ? 1 : 0;  // n / span < Nb: the host checked Nb = ceil(N / span)
  }
}

// ------------------------------------------------------------------------------------------ embedding finish, masked
// embed_finish_kernel; the row of a masked patch is the mask token and its projected token is not loaded
__global__ void embed_finish_masked_kernel(float* __restrict__ tok, const float* __restrict__ cls, const float* __restrict__ pos,
                                           const int* __restrict__ mask, const float* __restrict__ mtok, int B, int T, int D,
                                           DropCfg drop) {
  resolve_drop(drop);
  const int dv = D >> 2, N = T - 1;
  const long total = (long)B * T * dv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i % dv) << 2;
    const long row = i / dv;  // b*T + t
    const int t = (int)(row % T);
    const long b = row / T;
    float* p = tok + row * D + d;
    f32x4 v;
    if (t == 0)
      v = *(const f32x4*)(cls + d);
    else if (mask[b * N + (t - 1)] != 0)
      v = *(const f32x4*)(mtok + d);
    else
      v = *(const f32x4*)p;
    if (pos) v += *(const f32x4*)(pos + (long)t * D + d);
    if (drop.thr) {
      float k0, k1, k2, k3;
      drop_pair(drop, (unsigned long long)row, (unsigned)d, k0, k1);
      drop_pair(drop, (unsigned long long)row, (unsigned)d + 2, k2, k3);
      v[0] *= k0; v[1] *= k1; v[2] *= k2; v[3] *= k3;
    }
    *(f32x4*)p = v;
  }
}

// embed_finish_bwd_kernel: one thread per (t, 4 columns) walks its batch chunk in ascending b.  acc (every row: dcls / dpos)
// is the plain kernel's sum, term for term; macc takes the masked rows' terms alone, and those rows store a zero dpatch.
template <int OUT_BF16>
__global__ void embed_finish_masked_bwd_kernel(const float* __restrict__ dtok, const int* __restrict__ mask,
                                               void* __restrict__ dpatch, float* __restrict__ part, float* __restrict__ mpart,
                                               int B, int T, int D, DropCfg drop, int bchunk) {
  resolve_drop(drop);
  const int dv = D >> 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * dv) return;
  const int d = (i % dv) << 2;
  const int t = i / dv;
  const int N = T - 1;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f}, macc = {0.f, 0.f, 0.f, 0.f};
  for (int b = b0; b < b1; ++b) {
    const long row = (long)b * T + t;
    f32x4 v = *(const f32x4*)(dtok + row * D + d);
    if (drop.thr) {
      float k0, k1, k2, k3;
      drop_pair(drop, (unsigned long long)row, (unsigned)d, k0, k1);
      drop_pair(drop, (unsigned long long)row, (unsigned)d + 2, k2, k3);
      v[0] *= k0; v[1] *= k1; v[2] *= k2; v[3] *= k3;
    }
    acc += v;
    if (t > 0) {
      if (mask[(long)b * N + (t - 1)] != 0) {
        macc += v;
        v = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      if (OUT_BF16) {
        u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)((short*)dpatch + ((long)b * N + (t - 1)) * D + d) = pk;
      } else {
        *(f32x4*)((float*)dpatch + ((long)b * N + (t - 1)) * D + d) = v;
      }
    }
  }
  *(f32x4*)(part + ((long)blockIdx.y * T + t) * D + d) = acc;
  *(f32x4*)(mpart + ((long)blockIdx.y * T + t) * D + d) = macc;
}

// ------------------------------------------------------------------------------------------ reconstruction loss
template <int BF16>
__device__ __forceinline__ f32x4 load_pred4(const void* __restrict__ pred, long at) {
  if (BF16) return bf_round4(*(const u32x2*)((const short*)pred + at));
  return *(const f32x4*)((const float*)pred + at);
}

// mean and 1 / sqrt(unbiased var + 1e-6) of one target window, by the whole wave (every lane ends with both)
__device__ __forceinline__ void window_stats(const float* __restrict__ xw, bool fits, int P, int lane, float& mean, float& rinv) {
  float s = 0.f, q = 0.f;
  if (fits) {
    for (int p = lane * 4; p < P; p += 256) s += (xw[p] + xw[p + 1]) + (xw[p + 2] + xw[p + 3]);
  }
  mean = wave_sum(s) / (float)P;
  if (fits) {
    for (int p = lane * 4; p < P; p += 256) {
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const float c = xw[p + k] - mean;
        q += c * c;
      }
    }
  }
  rinv = 1.0f / sqrtf(wave_sum(q) / (float)(P - 1) + 1e-6f);
}

// one wave per window w = b * N + n; part[w] = the window's sum of l(pred - target), 0 for an unmasked one (which loads nothing)
template <int PRED_BF16>
__global__ __launch_bounds__(256) void mim_loss_fwd_kernel(const float* __restrict__ x, const void* __restrict__ pred,
                                                           const int* __restrict__ mask, float* __restrict__ part, int B, int L,
                                                           int P, int S, int N, int T, int l1, int norm) {
  const int lane = threadIdx.x & 63;
  const long nwin = (long)B * N;
  for (long w = blockIdx.x * 4L + (threadIdx.x >> 6); w < nwin; w += gridDim.x * 4L) {
    if (mask[w] == 0) {  // wave-uniform
      if (lane == 0) part[w] = 0.f;
      continue;
    }
    const long b = w / N;
    const int n = (int)(w - b * N);
    const bool fits = (long)n * S + P <= L;  // a window that does not fit is all zero and never read
    const float* xw = x + b * L + (fits ? (long)n * S : 0);
    float mean = 0.f, rinv = 1.f;
    if (norm) window_stats(xw, fits, P, lane, mean, rinv);
    const long prow = (b * T + 1 + n) * (long)P;
    float acc = 0.f;
    for (int p = lane * 4; p < P; p += 256) {
      const f32x4 pv = load_pred4<PRED_BF16>(pred, prow + p);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        float tg = fits ? xw[p + k] : 0.f;
        if (norm) tg = (tg - mean) * rinv;
        const float dd = pv[k] - tg;
        acc += l1 ? fabsf(dd) : dd * dd;
      }
    }
    acc = wave_sum(acc);
    if (lane == 0) part[w] = acc;
  }
}

// second stage, one block: thread i sums windows i, i + 1024, ... in ascending order, then a fixed tree over the LDS
__global__ __launch_bounds__(1024) void mim_loss_finish_kernel(const float* __restrict__ part, const int* __restrict__ mask,
                                                               long nwin, int P, float* __restrict__ loss_out,
                                                               int* __restrict__ count_out) {
  __shared__ float sred[1024];
  __shared__ int cred[1024];
  const int tid = threadIdx.x;
  float s = 0.f;
  int c = 0;
  for (long i = tid; i < nwin; i += 1024) {
    s += part[i];
    c += mask[i] != 0;
  }
  sred[tid] = s;
  cred[tid] = c;
  __syncthreads();
  for (int o = 512; o > 0; o >>= 1) {
    if (tid < o) {
      sred[tid] += sred[tid + o];
      cred[tid] += cred[tid + o];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const int m = cred[0];
    *loss_out = sred[0] / ((float)max(1, m) * (float)P);
    *count_out = m;
  }
}

// one wave per row r = b * T + t of dpred: zeros for CLS and unmasked windows, the loss gradient for masked ones
template <int PRED_BF16, int OUT_BF16>
__global__ __launch_bounds__(256) void mim_loss_bwd_kernel(const float* __restrict__ x, const void* __restrict__ pred,
                                                           const int* __restrict__ mask, const int* __restrict__ count,
                                                           const float* __restrict__ dloss, void* __restrict__ dpred, int B,
                                                           int L, int P, int S, int N, int T, int l1, int norm) {
  const int lane = threadIdx.x & 63;
  const long nrow = (long)B * T;
  const float up = dloss[0] / ((float)max(1, count[0]) * (float)P);
  for (long r = blockIdx.x * 4L + (threadIdx.x >> 6); r < nrow; r += gridDim.x * 4L) {
    const long b = r / T;
    const int n = (int)(r - b * T) - 1;
    const bool masked = n >= 0 && mask[b * N + n] != 0;  // wave-uniform
    const bool fits = masked && (long)n * S + P <= L;
    const float* xw = x + b * L + (fits ? (long)n * S : 0);
    float mean = 0.f, rinv = 1.f;
    if (masked && norm) window_stats(xw, fits, P, lane, mean, rinv);
    for (int p = lane * 4; p < P; p += 256) {
      f32x4 g = {0.f, 0.f, 0.f, 0.f};
      if (masked) {
        const f32x4 pv = load_pred4<PRED_BF16>(pred, r * P + p);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          float tg = fits ? xw[p + k] : 0.f;
          if (norm) tg = (tg - mean) * rinv;
          const float dd = pv[k] - tg;
          g[k] = l1 ? (dd > 0.f ? up : (dd < 0.f ? -up : 0.f)) : 2.f * dd * up;
        }
      }
      if (OUT_BF16) {
        u32x2 pk = {pack2bf(g[0], g[1]), pack2bf(g[2], g[3])};
        *(u32x2*)((short*)dpred + r * P + p) = pk;
      } else {
        *(f32x4*)((float*)dpred + r * P + p) = g;
      }
    }
  }
}

static int loss_args_ok(const char* who, int B, int L, int P, int S, int N, int T, int kind, int norm_target) {
  VIT_CHECK(B > 0 && L > 0 && P > 0 && S > 0 && N > 0 && (P % 4) == 0, VIT_ERR_ARG,
            "%s: B=%d L=%d P=%d S=%d N=%d (P must be a multiple of 4)", who, B, L, P, S, N);
  VIT_CHECK(T == N + 1, VIT_ERR_ARG, "%s: T=%d must be N + 1 = %d", who, T, N + 1);
  VIT_CHECK((long)(N - 1) * S < L, VIT_ERR_ARG, "%s: window %d starts past the signal", who, N - 1);
  VIT_CHECK(kind == VIT_LOSS_L1 || kind == VIT_LOSS_MSE, VIT_ERR_ARG, "%s: kind %d is neither VIT_LOSS_L1 nor VIT_LOSS_MSE", who,
            kind);
  VIT_CHECK(!norm_target || P >= 2, VIT_ERR_ARG, "%s: norm_target needs P >= 2", who);
  return VIT_OK;
}

}  // namespace vit

extern "C" {
using namespace vit;

int vit_mim_mask(vit_handle h, const int32_t* slot_blocks, int32_t* mask, int B, int N, int Nb, int span, vit_stream stream) {
  (void)h;
  VIT_CHECK(slot_blocks && mask, VIT_ERR_ARG, "vit_mim_mask: null pointer");
  VIT_CHECK(span >= 1, VIT_ERR_ARG, "vit_mim_mask: span=%d (need span >= 1)", span);
  VIT_CHECK(B > 0 && N > 0 && Nb == cdiv(N, span), VIT_ERR_ARG, "vit_mim_mask: B=%d N=%d Nb=%d span=%d (need Nb = ceil(N / span))",
            B, N, Nb, span);
  hipLaunchKernelGGL(mim_mask_kernel, dim3(grid_for((long)B * N)), dim3(256), 0, (hipStream_t)stream, slot_blocks, mask, B, N, Nb,
                     span);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_embed_finish_masked(vit_handle h, float* tokens, const float* cls, const float* pos, const int32_t* mask,
                            const float* mask_token, int B, int T, int D, float dropout_p, uint64_t seed, uint64_t site,
                            vit_stream stream) {
  VIT_CHECK(tokens && cls && mask && mask_token, VIT_ERR_ARG, "vit_embed_finish_masked: null pointer");
  VIT_CHECK(B > 0 && T > 1 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_embed_finish_masked: B=%d T=%d D=%d", B, T, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_embed_finish_masked: dropout_p out of [0,1)");
  const long total = (long)B * T * (D / 4);
  hipLaunchKernelGGL(embed_finish_masked_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, tokens, cls, pos, mask,
                     mask_token, B, T, D, make_drop_h(h, dropout_p, seed, site));
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_embed_finish_masked_bwd(vit_handle h, const float* dtokens, const int32_t* mask, void* dpatch_out, int dpatch_dtype,
                                float* dcls, float* dpos, float* dmask_token, int B, int T, int D, float dropout_p,
                                uint64_t seed, uint64_t site, int accumulate, vit_stream stream) {
  VIT_CHECK(dtokens && mask && dpatch_out && dcls && dmask_token, VIT_ERR_ARG, "vit_embed_finish_masked_bwd: null pointer");
  VIT_CHECK(B > 0 && T > 1 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_embed_finish_masked_bwd: B=%d T=%d D=%d", B, T, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_embed_finish_masked_bwd: dropout_p out of [0,1)");
  VIT_CHECK(dpatch_dtype == VIT_BF16 || dpatch_dtype == VIT_F32, VIT_ERR_ARG, "vit_embed_finish_masked_bwd: bad dtype");
  const int nchunk = std::min(B, 16), bchunk = cdiv(B, nchunk), ny = cdiv(B, bchunk);  // vit_embed_finish_bwd's chunks
  const size_t plane = (size_t)ny * T * D;
  float* part = (float*)ctx_claim(h, 2 * plane * sizeof(float), "vit_embed_finish_masked_bwd");
  if (!part) return VIT_ERR_WORKSPACE;
  float* mpart = part + plane;
  hipStream_t st = (hipStream_t)stream;
  accumulate = accumulate || ctx_grad_accumulate(h);
  const dim3 grid(cdiv((long)T * (D / 4), 256), ny);
  const DropCfg drop = make_drop_h(h, dropout_p, seed, site);
  if (dpatch_dtype == VIT_BF16)
    hipLaunchKernelGGL(embed_finish_masked_bwd_kernel<1>, grid, dim3(256), 0, st, dtokens, mask, dpatch_out, part, mpart, B, T, D,
                       drop, bchunk);
  else
    hipLaunchKernelGGL(embed_finish_masked_bwd_kernel<0>, grid, dim3(256), 0, st, dtokens, mask, dpatch_out, part, mpart, B, T, D,
                       drop, bchunk);
  VIT_LAUNCH_CHECK();
  // dcls / dpos as vit_embed_finish_bwd reduces them; dmask_token = the sum of all ny * T partial rows, in row order
  int rc = launch_reduce_partials(part, ny, D, dcls, D, dcls, accumulate, st, T * D);
  if (rc == VIT_OK && dpos) rc = launch_reduce_partials(part, ny, T * D, dpos, T * D, dpos, accumulate, st, T * D);
  if (rc != VIT_OK) return rc;
  return launch_reduce_partials(mpart, ny * T, D, dmask_token, D, dmask_token, accumulate, st, D);
}

int vit_mim_loss_fwd(vit_handle h, const float* x, const void* pred, int pred_dtype, const int32_t* mask, float* loss_out,
                     int32_t* count_out, int B, int L, int P, int S, int N, int T, int kind, int norm_target,
                     vit_stream stream) {
  VIT_CHECK(x && pred && mask && loss_out && count_out, VIT_ERR_ARG, "vit_mim_loss_fwd: null pointer");
  VIT_CHECK(pred_dtype == VIT_BF16 || pred_dtype == VIT_F32, VIT_ERR_ARG, "vit_mim_loss_fwd: bad dtype");
  const int rc = loss_args_ok("vit_mim_loss_fwd", B, L, P, S, N, T, kind, norm_target);
  if (rc != VIT_OK) return rc;
  const long nwin = (long)B * N;
  float* part = (float*)ctx_claim(h, (size_t)nwin * sizeof(float), "vit_mim_loss_fwd");
  if (!part) return VIT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(grid_for(nwin, 4));
  const int l1 = kind == VIT_LOSS_L1, norm = norm_target != 0;
  if (pred_dtype == VIT_BF16)
    hipLaunchKernelGGL(mim_loss_fwd_kernel<1>, grid, dim3(256), 0, st, x, pred, mask, part, B, L, P, S, N, T, l1, norm);
  else
    hipLaunchKernelGGL(mim_loss_fwd_kernel<0>, grid, dim3(256), 0, st, x, pred, mask, part, B, L, P, S, N, T, l1, norm);
  VIT_LAUNCH_CHECK();
  hipLaunchKernelGGL(mim_loss_finish_kernel, dim3(1), dim3(1024), 0, st, part, mask, nwin, P, loss_out, count_out);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_mim_loss_bwd(vit_handle h, const float* x, const void* pred, int pred_dtype, const int32_t* mask, const int32_t* count,
                     const float* dloss, void* dpred, int dpred_dtype, int B, int L, int P, int S, int N, int T, int kind,
                     int norm_target, vit_stream stream) {
  (void)h;
  VIT_CHECK(x && pred && mask && count && dloss && dpred, VIT_ERR_ARG, "vit_mim_loss_bwd: null pointer");
  VIT_CHECK((pred_dtype == VIT_BF16 || pred_dtype == VIT_F32) && (dpred_dtype == VIT_BF16 || dpred_dtype == VIT_F32), VIT_ERR_ARG,
            "vit_mim_loss_bwd: bad dtype");
  const int rc = loss_args_ok("vit_mim_loss_bwd", B, L, P, S, N, T, kind, norm_target);
  if (rc != VIT_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid(grid_for((long)B * T, 4));
  const int l1 = kind == VIT_LOSS_L1, norm = norm_target != 0;
#define MIM_BWD(PB, OB)                                                                                                    \
  hipLaunchKernelGGL((mim_loss_bwd_kernel<PB, OB>), grid, dim3(256), 0, st, x, pred, mask, count, dloss, dpred, B, L, P, S, N, T, \
                     l1, norm)
  if (pred_dtype == VIT_BF16) {
    if (dpred_dtype == VIT_BF16) MIM_BWD(1, 1); else MIM_BWD(1, 0);
  } else {
    if (dpred_dtype == VIT_BF16) MIM_BWD(0, 1); else MIM_BWD(0, 0);
  }
#undef MIM_BWD
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
