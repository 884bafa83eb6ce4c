// Patch dropout for gfx950 (include/vit_amd_patchdrop.h): the per-sample token selection and the gather forms of the
// embedding-side kernels of elementwise.hip -- unfold + cast, embedding finish and its backward, the overlap-add -- plus the
// row gather that builds per-step RoPE tables.  Behind them the encoder runs at Tc = 1 + K tokens and knows nothing of this.
// Like their plain twins: vectorised (8-16 B per lane), grid-stride, free of float atomics; every index read from idx / slot
// is range-checked before it addresses memory.
#include <algorithm>

#include "common.h"

namespace vit {

// ------------------------------------------------------------------------------------------ selection
// One workgroup per sample: keys in the LDS, rank by counting (the order (key, n) is total, so exactly K patches have
// rank < K), then a block scan over ascending n compacts the kept ones.  N^2 / 256 LDS reads per lane, all broadcasts: 150
// per lane at N = 196, 262 k at the N = 8192 limit (a fraction of a millisecond, once per step).
__global__ __launch_bounds__(256) void patch_select_kernel(int* __restrict__ idx, int* __restrict__ slot, int N, int K, unsigned k0,
                                                           unsigned k1, const unsigned* __restrict__ dyn) {
  __shared__ unsigned keys[VIT_PATCH_SELECT_MAX_N];
  __shared__ unsigned char keep[VIT_PATCH_SELECT_MAX_N];
  __shared__ int wsum[4];
  const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (dyn) {  // a bound step record: always consulted -- there is no threshold whose zero would mean "off" (resolve_drop)
    k0 ^= dyn[0];
    k1 ^= dyn[1];
  }
  for (int n = tid; n < N; n += 256) keys[n] = drop_hash(k0, k1, (unsigned long long)b * N + n);
  __syncthreads();
  for (int n = tid; n < N; n += 256) {
    const unsigned kn = keys[n];
    int r = 0;
#pragma unroll 4
    for (int m = 0; m < N; ++m) {
      const unsigned km = keys[m];
      r += (km < kn) | ((km == kn) & (m < n));
    }
    keep[n] = r < K;
  }
  __syncthreads();
  int base = 0;
  for (int n0 = 0; n0 < N; n0 += 256) {
    const int n = n0 + tid;
    const int f = n < N ? keep[n] : 0;
    const unsigned long long bal = __ballot(f);
    const int pre = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wsum[w] = __popcll(bal);
    __syncthreads();
    int off = base;
    for (int i = 0; i < w; ++i) off += wsum[i];
    base += (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]);
    if (n < N) {
      const int s = off + pre;
      slot[(long)b * N + n] = f ? s : -1;
      if (f && s < K) idx[(long)b * K + s] = n;
    }
    __syncthreads();
  }
}

// slot from a caller's idx (ViTEngine.patch_keep): one workgroup per sample fills its row with -1, then places the kept ones
__global__ __launch_bounds__(256) void patch_slot_kernel(const int* __restrict__ idx, int* __restrict__ slot, int N, int K) {
  const long b = blockIdx.x;
  for (int n = threadIdx.x; n < N; n += 256) slot[b * N + n] = -1;
  __syncthreads();  // the block's own global stores, ordered for its own later stores to the same addresses
  for (int k = threadIdx.x; k < K; k += 256) {
    const int n = idx[b * K + k];
    if (n >= 0 && n < N) slot[b * N + n] = k;
  }
}

// ------------------------------------------------------------------------------------------ unfold + cast, gathered
// unfold_cast_kernel with n = idx[b, k]
template <int OUT_BF16>
__global__ void unfold_gather_cast_kernel(const float* __restrict__ x, const int* __restrict__ idx, void* __restrict__ out, int B,
                                          int L, int P, int S, int N, int K) {
  const long total = (long)B * K * (P >> 2);
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int pv = (int)(i % (P >> 2)) << 2;
    const long bk = i / (P >> 2);
    const long b = bk / K;
    const int n = idx[bk];
    const bool fits = n >= 0 && n < N && (long)n * S + P <= L;
    const float* src = x + b * L + (fits ? (long)n * S + pv : 0);
    float v[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) v[k] = fits ? src[k] : 0.f;
    if (OUT_BF16) {
      u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
      *(u32x2*)((short*)out + bk * P + pv) = pk;
    } else {
      *(f32x4*)((float*)out + bk * P + pv) = (f32x4){v[0], v[1], v[2], v[3]};
    }
  }
}

// position row of compact token t of the sample whose kept patches start at `idx_b`
__device__ __forceinline__ int pos_row(const int* __restrict__ idx_b, int t, int T_full) {
  if (t == 0) return 0;
  const int p = 1 + idx_b[t - 1];
  return (p >= 1 && p < T_full) ? p : 0;
}

// ------------------------------------------------------------------------------------------ embedding finish, gathered
// embed_finish_kernel over [B, Tc, D]; the position row is pos(b, t), the mask is keyed by the compact row
__global__ void embed_finish_gather_kernel(float* __restrict__ tok, const float* __restrict__ cls, const float* __restrict__ pos,
                                           const int* __restrict__ idx, int B, int Tc, int T_full, int D, DropCfg drop) {
  resolve_drop(drop);
  const int dv = D >> 2, K = Tc - 1;
  const long total = (long)B * Tc * dv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int d = (int)(i % dv) << 2;
    const long row = i / dv;  // b*Tc + t
    const int t = (int)(row % Tc);
    const long b = row / Tc;
    float* p = tok + row * D + d;
    f32x4 v = (t == 0) ? *(const f32x4*)(cls + d) : *(const f32x4*)p;
    if (pos) v += *(const f32x4*)(pos + (long)pos_row(idx + b * K, t, T_full) * D + d);
    if (drop.thr) {
      float k0, k1, k2, k3;
      drop_pair(drop, (unsigned long long)row, (unsigned)d, k0, k1);
      drop_pair(drop, (unsigned long long)row, (unsigned)d + 2, k2, k3);
      v[0] *= k0; v[1] *= k1; v[2] *= k2; v[3] *= k3;
    }
    *(f32x4*)p = v;
  }
}

// embed_finish_bwd_kernel walked over the FULL (t, 4 columns) space: thread (t, d) visits, for every sample of its batch chunk,
// the compact row that holds full token t (through slot; none for a dropped patch), applies that row's mask, stores the
// patch-projection gradient at its compact place and sums into part[blockIdx.y][T_full * D].  Every kept (b, k) has exactly
// one visitor; a token nobody kept sums to zero.  Same chunks, same order as the plain kernel: slot = identity gives its bits.
template <int OUT_BF16>
__global__ void embed_finish_gather_bwd_kernel(const float* __restrict__ dtok, const int* __restrict__ slot,
                                               void* __restrict__ dpatch, float* __restrict__ part, int B, int Tc, int T_full,
                                               int D, DropCfg drop, int bchunk) {
  resolve_drop(drop);
  const int dv = D >> 2;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T_full * dv) return;
  const int d = (i % dv) << 2;
  const int t = i / dv;
  const int N = T_full - 1, K = Tc - 1;
  const int b0 = blockIdx.y * bchunk, b1 = min(B, b0 + bchunk);
  f32x4 acc = {0.f, 0.f, 0.f, 0.f};
  for (int b = b0; b < b1; ++b) {
    int tc = 0;
    if (t > 0) {
      const int s = slot[(long)b * N + (t - 1)];
      if (s < 0 || s >= K) continue;
      tc = 1 + s;
    }
    const long row = (long)b * Tc + tc;
    f32x4 v = *(const f32x4*)(dtok + row * D + d);
    if (drop.thr) {
      float k0, k1, k2, k3;
      drop_pair(drop, (unsigned long long)row, (unsigned)d, k0, k1);
      drop_pair(drop, (unsigned long long)row, (unsigned)d + 2, k2, k3);
      v[0] *= k0; v[1] *= k1; v[2] *= k2; v[3] *= k3;
    }
    acc += v;
    if (t > 0) {
      if (OUT_BF16) {
        u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)((short*)dpatch + ((long)b * K + (tc - 1)) * D + d) = pk;
      } else {
        *(f32x4*)((float*)dpatch + ((long)b * K + (tc - 1)) * D + d) = v;
      }
    }
  }
  *(f32x4*)(part + ((long)blockIdx.y * T_full + t) * D + d) = acc;
}

// ------------------------------------------------------------------------------------------ table rows by position
__global__ void rows_gather_kernel(const float* __restrict__ table, const int* __restrict__ idx, float* __restrict__ out, int B,
                                   int Tc, int T_full, int W) {
  const int wv = W >> 2, K = Tc - 1;
  const long total = (long)B * Tc * wv;
  for (long i = blockIdx.x * (long)blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int c = (int)(i % wv) << 2;
    const long row = i / wv;
    const int t = (int)(row % Tc);
    const long b = row / Tc;
    *(f32x4*)(out + row * W + c) = *(const f32x4*)(table + (long)pos_row(idx + b * K, t, T_full) * W + c);
  }
}

// ------------------------------------------------------------------------------------------ overlap-add through slot
// fold_add_kernel reading the compact dpatches [B*K, P]: dropped windows are skipped, kept ones added in ascending n
__global__ __launch_bounds__(256) void fold_add_gather_kernel(const float* __restrict__ dp, const int* __restrict__ slot,
                                                              float* __restrict__ dx, int B, int L, int P, int S, int N, int K) {
  const long total = (long)B * L;
  const int nvalid = min(N, (L - P) / S + 1);  // windows that fit
  for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long)gridDim.x * blockDim.x) {
    const int b = (int)(i / L), l = (int)(i - (long)b * L);
    const int n_hi = min(nvalid - 1, l / S);
    const int n_lo = max(0, (l - P + S) / S);
    float acc = 0.f;
    for (int n = n_lo; n <= n_hi; ++n) {
      const int s = slot[(long)b * N + n];
      if (s >= 0 && s < K) acc += dp[((long)b * K + s) * P + (l - n * S)];
    }
    dx[i] = acc;
  }
}

}  // namespace vit

extern "C" {
using namespace vit;

int vit_patch_select(vit_handle h, int32_t* idx, int32_t* slot, int B, int N, int K, uint64_t seed, uint64_t site,
                     vit_stream stream) {
  VIT_CHECK(idx && slot, VIT_ERR_ARG, "vit_patch_select: null pointer");
  VIT_CHECK(B > 0 && N > 0 && K > 0 && K <= N, VIT_ERR_ARG, "vit_patch_select: B=%d N=%d K=%d (need 1 <= K <= N)", B, N, K);
  VIT_CHECK(N <= VIT_PATCH_SELECT_MAX_N, VIT_ERR_ARG, "vit_patch_select: N=%d exceeds the supported %d patches per sample", N,
            VIT_PATCH_SELECT_MAX_N);
  const DropCfg d = make_drop_h(h, 0.f, seed, site);
  hipLaunchKernelGGL(patch_select_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, idx, slot, N, K, d.k0, d.k1, d.dyn);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_patch_slot(vit_handle h, const int32_t* idx, int32_t* slot, int B, int N, int K, vit_stream stream) {
  (void)h;
  VIT_CHECK(idx && slot, VIT_ERR_ARG, "vit_patch_slot: null pointer");
  VIT_CHECK(B > 0 && N > 0 && K > 0 && K <= N, VIT_ERR_ARG, "vit_patch_slot: B=%d N=%d K=%d (need 1 <= K <= N)", B, N, K);
  hipLaunchKernelGGL(patch_slot_kernel, dim3(B), dim3(256), 0, (hipStream_t)stream, idx, slot, N, K);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_unfold_gather_cast(vit_handle h, const float* x, const int32_t* idx, void* patches, int out_dtype, int B, int L, int P,
                           int S, int N, int K, vit_stream stream) {
  (void)h;
  VIT_CHECK(x && idx && patches, VIT_ERR_ARG, "vit_unfold_gather_cast: null pointer");
  VIT_CHECK(B > 0 && L > 0 && P > 0 && S > 0 && N > 0 && K > 0 && K <= N && (P % 4) == 0, VIT_ERR_ARG,
            "vit_unfold_gather_cast: B=%d L=%d P=%d S=%d N=%d K=%d (P must be a multiple of 4, 1 <= K <= N)", B, L, P, S, N, K);
  VIT_CHECK((long)(N - 1) * S < L, VIT_ERR_ARG, "vit_unfold_gather_cast: patch %d starts past the signal", N - 1);
  VIT_CHECK(out_dtype == VIT_BF16 || out_dtype == VIT_F32, VIT_ERR_ARG, "vit_unfold_gather_cast: bad dtype");
  const long total = (long)B * K * (P / 4);
  if (out_dtype == VIT_BF16)
    hipLaunchKernelGGL(unfold_gather_cast_kernel<1>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, idx, patches, B,
                       L, P, S, N, K);
  else
    hipLaunchKernelGGL(unfold_gather_cast_kernel<0>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, x, idx, patches, B,
                       L, P, S, N, K);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_embed_finish_gather(vit_handle h, float* tokens, const float* cls, const float* pos, const int32_t* idx, int B, int Tc,
                            int T_full, int D, float dropout_p, uint64_t seed, uint64_t site, vit_stream stream) {
  VIT_CHECK(tokens && cls && idx, VIT_ERR_ARG, "vit_embed_finish_gather: null pointer");
  VIT_CHECK(B > 0 && Tc > 1 && Tc <= T_full && D > 0 && (D % 4) == 0, VIT_ERR_ARG,
            "vit_embed_finish_gather: B=%d Tc=%d T_full=%d D=%d (need 1 < Tc <= T_full, D a multiple of 4)", B, Tc, T_full, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_embed_finish_gather: dropout_p out of [0,1)");
  const long total = (long)B * Tc * (D / 4);
  hipLaunchKernelGGL(embed_finish_gather_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, tokens, cls, pos, idx,
                     B, Tc, T_full, D, make_drop_h(h, dropout_p, seed, site));
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_embed_finish_gather_bwd(vit_handle h, const float* dtokens, const int32_t* slot, void* dpatch_out, int dpatch_dtype,
                                float* dcls, float* dpos, int B, int Tc, int T_full, int D, float dropout_p, uint64_t seed,
                                uint64_t site, int accumulate, vit_stream stream) {
  VIT_CHECK(dtokens && slot && dpatch_out && dcls, VIT_ERR_ARG, "vit_embed_finish_gather_bwd: null pointer");
  VIT_CHECK(B > 0 && Tc > 1 && Tc <= T_full && D > 0 && (D % 4) == 0, VIT_ERR_ARG,
            "vit_embed_finish_gather_bwd: B=%d Tc=%d T_full=%d D=%d (need 1 < Tc <= T_full, D a multiple of 4)", B, Tc, T_full, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_embed_finish_gather_bwd: dropout_p out of [0,1)");
  VIT_CHECK(dpatch_dtype == VIT_BF16 || dpatch_dtype == VIT_F32, VIT_ERR_ARG, "vit_embed_finish_gather_bwd: bad dtype");
  const int nchunk = std::min(B, 16), bchunk = cdiv(B, nchunk), ny = cdiv(B, bchunk);  // vit_embed_finish_bwd's chunks
  float* part = (float*)ctx_claim(h, (size_t)ny * T_full * D * sizeof(float), "vit_embed_finish_gather_bwd");
  if (!part) return VIT_ERR_WORKSPACE;
  hipStream_t st = (hipStream_t)stream;
  accumulate = accumulate || ctx_grad_accumulate(h);
  const dim3 grid(cdiv((long)T_full * (D / 4), 256), ny);
  const DropCfg drop = make_drop_h(h, dropout_p, seed, site);
  if (dpatch_dtype == VIT_BF16)
    hipLaunchKernelGGL(embed_finish_gather_bwd_kernel<1>, grid, dim3(256), 0, st, dtokens, slot, dpatch_out, part, B, Tc, T_full,
                       D, drop, bchunk);
  else
    hipLaunchKernelGGL(embed_finish_gather_bwd_kernel<0>, grid, dim3(256), 0, st, dtokens, slot, dpatch_out, part, B, Tc, T_full,
                       D, drop, bchunk);
  VIT_LAUNCH_CHECK();
  // dcls = sum over the batch of row t = 0; dpos (if any) = the sums of every full row
  int rc = launch_reduce_partials(part, ny, D, dcls, D, dcls, accumulate, st, T_full * D);
  if (rc != VIT_OK || !dpos) return rc;
  return launch_reduce_partials(part, ny, T_full * D, dpos, T_full * D, dpos, accumulate, st, T_full * D);
}

int vit_rows_gather(vit_handle h, const float* table, const int32_t* idx, float* out, int B, int Tc, int T_full, int W,
                    vit_stream stream) {
  (void)h;
  VIT_CHECK(table && idx && out, VIT_ERR_ARG, "vit_rows_gather: null pointer");
  VIT_CHECK(B > 0 && Tc > 1 && Tc <= T_full && W > 0 && (W % 4) == 0, VIT_ERR_ARG,
            "vit_rows_gather: B=%d Tc=%d T_full=%d W=%d (need 1 < Tc <= T_full, W a multiple of 4)", B, Tc, T_full, W);
  const long total = (long)B * Tc * (W / 4);
  hipLaunchKernelGGL(rows_gather_kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, table, idx, out, B, Tc, T_full,
                     W);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_fold_add_gather(vit_handle h, const float* dpatches, const int32_t* slot, float* dx, int B, int L, int P, int S, int N,
                        int K, vit_stream stream) {
  (void)h;
  VIT_CHECK(dpatches && slot && dx, VIT_ERR_ARG, "vit_fold_add_gather: null pointer");
  VIT_CHECK(B > 0 && L > 0 && P > 0 && S > 0 && N > 0 && K > 0 && K <= N && P <= L, VIT_ERR_ARG,
            "vit_fold_add_gather: B=%d L=%d P=%d S=%d N=%d K=%d", B, L, P, S, N, K);
  hipLaunchKernelGGL(fold_add_gather_kernel, dim3(grid_for((long)B * L)), dim3(256), 0, (hipStream_t)stream, dpatches, slot, dx,
                     B, L, P, S, N, K);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
