// Muon for gfx950 (include/vit_amd_muon.h): SGD momentum per weight matrix, its orthogonalisation by a quintic Newton-Schulz
// iteration in bf16, and only that applied to the weights.  Unlike every other optimizer family here the hot path is matrix
// products: 3 per iteration per matrix, 1,080 small ones per step at ViT-B.  Issued one by one they would be bound by launches and
// occupancy, so ONE launch computes one product of one iteration for ALL matrices: a host-built tile table maps each workgroup
// to (problem, tile row, tile column), 64 x 64 of C per workgroup, v_mfma_f32_16x16x32_bf16, operands through the LDS.
// Around the products four streaming launches over a per-matrix table: momentum + u + per-tile f64 sums of squares, one wave per
// matrix for 1 / max(norm, eps), normalise into the wide orientation, and the apply that transposes back.  No atomics.
#include "common.h"
#include "../../include/vit_amd_muon.h"

// as optim.hip: every fused multiply-add is written as one (fma_), so the same source rounds the same way everywhere
#pragma clang fp contract(off)

namespace vit {

constexpr int MUON_TILE = VIT_MUON_TILE;
constexpr int GT = VIT_MUON_GEMM_TILE;  // C tile per workgroup
constexpr int GK = 64;                  // K per LDS stage
constexpr int GLD = GK + 8;             // LDS row stride in bf16: 144 B, 16-byte aligned fragments, rows spread over the banks
constexpr int TT = 32;                  // transposing tile

struct alignas(16) MuonRow { float lr, wd, mu, pad; };

// the last matrix whose first tile (field F) is <= w; tables ascend
template <int vit_muon_mat::*F>
__device__ __forceinline__ int mat_of(const vit_muon_mat* __restrict__ mats, int n_mats, int w) {
  int lo = 0, hi = n_mats - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (mats[mid].*F <= w) lo = mid; else hi = mid - 1;
  }
  return lo;
}

__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// ---- 1. momentum, u, partial sums ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(STEP_BLOCK) void muon_momentum_kernel(const float* __restrict__ g, float* __restrict__ buf,
                                                                   short* __restrict__ u, const vit_muon_mat* __restrict__ mats,
                                                                   int n_mats, int n_tiles, float omm, float mom, int nesterov,
                                                                   const float* __restrict__ sqnorm, float max_norm,
                                                                   double* __restrict__ part) {
  __shared__ double red[STEP_BLOCK / 64];
  const float clip = sqnorm ? fminf(1.f, max_norm / (sqrtf(sqnorm[0]) + 1e-6f)) : 1.f;
  for (int w = blockIdx.x; w < n_tiles; w += gridDim.x) {  // block-uniform
    const vit_muon_mat M = mats[mat_of<&vit_muon_mat::tile0>(mats, n_mats, w)];
    const long total = (long)M.rows * M.cols;  // a multiple of 256
    const long e0 = (long)(w - M.tile0) * MUON_TILE;
    const long e1 = e0 + MUON_TILE < total ? e0 + MUON_TILE : total;
    double sum = 0.0;
    for (long e = e0 + 4 * threadIdx.x; e < e1; e += 4 * STEP_BLOCK) {
      const f32x4 gg = *(const f32x4*)(g + M.off + e) * clip;
      f32x4 bb = *(const f32x4*)(buf + M.xoff + e);
      u32x2 pk;
      float uu[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        bb[k] = fma_(gg[k] - bb[k], omm, bb[k]);
        uu[k] = nesterov ? fma_(bb[k] - gg[k], mom, gg[k]) : bb[k];
      }
      pk[0] = pack2bf(uu[0], uu[1]);
      pk[1] = pack2bf(uu[2], uu[3]);
      *(f32x4*)(buf + M.xoff + e) = bb;
      *(u32x2*)(u + M.xoff + e) = pk;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const double r = (double)bf2f((short)((pk[k >> 1] >> (16 * (k & 1))) & 0xffffu));
        sum = __builtin_fma(r, r, sum);
      }
    }
    sum = wave_sum_d(sum);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
      double t = red[0];
      for (int k = 1; k < STEP_BLOCK / 64; ++k) t += red[k];
      part[w] = t;
    }
    __syncthreads();
  }
}

// ---- 2. one wave per matrix: 1 / max(norm, eps) ---------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void muon_norms_kernel(const vit_muon_mat* __restrict__ mats, int n_mats,
                                                        const double* __restrict__ part, float eps, float* __restrict__ inv_norm,
                                                        float* __restrict__ norms) {
  for (int i = blockIdx.x; i < n_mats; i += gridDim.x) {
    const vit_muon_mat M = mats[i];
    const long total = (long)M.rows * M.cols;
    const int tiles = (int)((total + MUON_TILE - 1) / MUON_TILE);
    double s = 0.0;
    for (int k = threadIdx.x; k < tiles; k += 64) s += part[M.tile0 + k];
    s = wave_sum_d(s);
    if (threadIdx.x == 0) {
      const double nrm = sqrt(s);
      norms[i] = (float)nrm;
      inv_norm[i] = (float)(1.0 / fmax(nrm, (double)eps));
    }
  }
}

// ---- 3. / 5. the transposing tile passes -----------------------------------------------------------------------------------------
// A workgroup owns one 32 x 32 tile of W's [rows, cols] grid.  The wide image x is [m, n] = [rows, cols], or [cols, rows] when
// rows > cols; both sides are read and written along their rows, the transposition happens in the LDS tile.
struct TTile { vit_muon_mat M; int i, r0, c0; bool tr; };
__device__ __forceinline__ TTile ttile_of(const vit_muon_mat* __restrict__ mats, int n_mats, int w) {
  TTile t;
  t.i = mat_of<&vit_muon_mat::ttile0>(mats, n_mats, w);
  t.M = mats[t.i];
  const int tc = (t.M.cols + TT - 1) / TT, local = w - t.M.ttile0;
  t.r0 = (local / tc) * TT;
  t.c0 = (local % tc) * TT;
  t.tr = t.M.rows > t.M.cols;
  return t;
}

__global__ __launch_bounds__(STEP_BLOCK) void muon_normalize_kernel(const short* __restrict__ u, short* __restrict__ x,
                                                                    const vit_muon_mat* __restrict__ mats, int n_mats,
                                                                    int n_ttiles, const float* __restrict__ inv_norm) {
  __shared__ short tile[TT][TT + 2];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int w = blockIdx.x; w < n_ttiles; w += gridDim.x) {
    const TTile t = ttile_of(mats, n_mats, w);
    const float inv = inv_norm[t.i];
    const long rows = t.M.rows, cols = t.M.cols;
    for (int rr = ty; rr < TT; rr += 8) {
      const long r = t.r0 + rr, c = t.c0 + tx;
      if (r < rows && c < cols) tile[rr][tx] = f2bf(bf2f(u[t.M.xoff + r * cols + c]) * inv);
    }
    __syncthreads();
    if (!t.tr) {
      for (int rr = ty; rr < TT; rr += 8) {
        const long r = t.r0 + rr, c = t.c0 + tx;
        if (r < rows && c < cols) x[t.M.xoff + r * cols + c] = tile[rr][tx];
      }
    } else {
      for (int cc = ty; cc < TT; cc += 8) {
        const long c = t.c0 + cc, r = t.r0 + tx;
        if (r < rows && c < cols) x[t.M.xoff + c * rows + r] = tile[tx][cc];
      }
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(STEP_BLOCK) void muon_apply_kernel(float* __restrict__ p, short* __restrict__ pb,
                                                                const short* __restrict__ o, const vit_muon_mat* __restrict__ mats,
                                                                int n_mats, int n_ttiles, const MuonRow* __restrict__ rowsT,
                                                                int n_groups) {
  __shared__ short tile[TT][TT + 2];
  const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
  for (int w = blockIdx.x; w < n_ttiles; w += gridDim.x) {
    const TTile t = ttile_of(mats, n_mats, w);
    const unsigned gi = (unsigned)t.M.group;
    const MuonRow row = rowsT[gi < (unsigned)n_groups ? gi : (unsigned)n_groups - 1u];
    const float decay = fma_(-row.lr, row.wd, 1.f), step = row.lr * t.M.ratio;
    const long rows = t.M.rows, cols = t.M.cols;
    if (!t.tr) {
      for (int rr = ty; rr < TT; rr += 8) {
        const long r = t.r0 + rr, c = t.c0 + tx;
        if (r < rows && c < cols) tile[rr][tx] = o[t.M.xoff + r * cols + c];
      }
    } else {
      for (int cc = ty; cc < TT; cc += 8) {
        const long c = t.c0 + cc, r = t.r0 + tx;
        if (r < rows && c < cols) tile[tx][cc] = o[t.M.xoff + c * rows + r];
      }
    }
    __syncthreads();
    for (int rr = ty; rr < TT; rr += 8) {
      const long r = t.r0 + rr, c = t.c0 + tx;
      if (r < rows && c < cols) {
        const long at = t.M.off + r * cols + c;
        const float pp = fma_(bf2f(tile[rr][tx]), -step, p[at] * decay);
        p[at] = pp;
        if (pb) pb[at] = f2bf(pp);
      }
    }
    __syncthreads();
  }
}

// ---- 4. the grouped product ----------------------------------------------------------------------------------------------------------
// 256 lanes = 4 waves as 2 x 2, each wave 32 x 32 of the 64 x 64 tile: 2 x 2 accumulators of v_mfma_f32_16x16x32_bf16.  Per
// 64-deep K stage both operands go through the LDS as [row or column of C][k] images, rows padded to 144 B, so every fragment
// is one 16-byte read: lane l takes k = 8 (l >> 4) .. + 7 of row (l & 15) (the instruction's A and B lane maps).  BT (A B^T, B
// [n, k]): B is staged exactly as A is.  !BT (A B, B [k, n]): a lane loads 8 consecutive n of one k and scatters them into the
// [n][k] image.  Rows, columns and k past the matrix are staged as zeros; the epilogue stores only what lies inside C.
template <bool BT>
__global__ __launch_bounds__(256) void muon_gemm_kernel(const vit_muon_problem* __restrict__ probs, int n_problems,
                                                        const i32x4* __restrict__ tiles) {
  __shared__ __attribute__((aligned(16))) short sA[GT][GLD];
  __shared__ __attribute__((aligned(16))) short sB[GT][GLD];
  const i32x4 t = tiles[blockIdx.x];
  if ((unsigned)t[0] >= (unsigned)n_problems) return;  // block-uniform: a malformed table computes nothing
  const vit_muon_problem P = probs[t[0]];
  const int row0 = t[1] * GT, col0 = t[2] * GT;
  if (row0 < 0 || col0 < 0 || row0 >= P.m || col0 >= P.n) return;
  const short* __restrict__ A = (const short*)P.A;
  const short* __restrict__ B = (const short*)P.B;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, wr = wave >> 1, wc = wave & 1;
  const int fr = lane & 15, fq = lane >> 4;
  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
  const bf16x8 zero = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int k0 = 0; k0 < P.k; k0 += GK) {
#pragma unroll
    for (int s = 0; s < 2; ++s) {  // 64 rows x 8 chunks of 8 k: two chunks per lane
      const int ch = tid + 256 * s, r = ch >> 3, c = (ch & 7) * 8;
      bf16x8 va = zero;
      if (row0 + r < P.m && k0 + c < P.k) va = *(const bf16x8*)(A + (long)(row0 + r) * P.lda + k0 + c);
      *(bf16x8*)&sA[r][c] = va;
      if (BT) {
        bf16x8 vb = zero;
        if (col0 + r < P.n && k0 + c < P.k) vb = *(const bf16x8*)(B + (long)(col0 + r) * P.ldb + k0 + c);
        *(bf16x8*)&sB[r][c] = vb;
      } else {  // 64 k x 8 chunks of 8 n
        const int kk = ch >> 3, nn = (ch & 7) * 8;
        bf16x8 vb = zero;
        if (k0 + kk < P.k && col0 + nn < P.n) vb = *(const bf16x8*)(B + (long)(k0 + kk) * P.ldb + col0 + nn);
#pragma unroll
        for (int j = 0; j < 8; ++j) sB[nn + j][kk] = vb[j];
      }
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < GK; ks += 32) {
      bf16x8 a[2], b[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        a[i] = *(const bf16x8*)&sA[wr * 32 + i * 16 + fr][ks + 8 * fq];
        b[i] = *(const bf16x8*)&sB[wc * 32 + i * 16 + fr][ks + 8 * fq];
      }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    __syncthreads();
  }
  const short* __restrict__ R = (const short*)P.R;
  short* __restrict__ C = (short*)P.C;
  const bool with_r = P.beta != 0.f && R != nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int col = col0 + wc * 32 + j * 16 + fr;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int row = row0 + wr * 32 + i * 16 + fq * 4 + q;
        if (row < P.m && col < P.n) {
          float v = P.alpha * acc[i][j][q];
          if (with_r) v = fma_(P.beta, bf2f(R[(long)row * P.ldr + col]), v);
          C[(long)row * P.ldc + col] = f2bf(v);
        }
      }
    }
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_muon_momentum(vit_handle h, const float* g, float* buf, void* u, const vit_muon_mat* mats, int n_mats, int n_tiles,
                      double momentum, int nesterov, const float* sqnorm, float max_norm, double* part, vit_stream stream) {
  (void)h;
  VIT_CHECK(g && buf && u && mats && part, VIT_ERR_ARG, "vit_muon_momentum: null pointer (g, buf, u, mats, part)");
  VIT_CHECK(n_mats > 0 && n_tiles > 0, VIT_ERR_ARG, "vit_muon_momentum: n_mats = %d and n_tiles = %d must be positive", n_mats,
            n_tiles);
  VIT_CHECK(momentum >= 0.0 && momentum < 1.0, VIT_ERR_ARG, "vit_muon_momentum: momentum = %g outside [0, 1)", momentum);
  hipLaunchKernelGGL(muon_momentum_kernel, dim3(grid_for(n_tiles, 1, 8192)), dim3(STEP_BLOCK), 0, (hipStream_t)stream, g, buf,
                     (short*)u, mats, n_mats, n_tiles, (float)(1.0 - momentum), (float)momentum, nesterov, sqnorm, max_norm, part);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_muon_norms(vit_handle h, const vit_muon_mat* mats, int n_mats, const double* part, float eps, float* inv_norm,
                   float* norms, vit_stream stream) {
  (void)h;
  VIT_CHECK(mats && part && inv_norm && norms, VIT_ERR_ARG, "vit_muon_norms: null pointer (mats, part, inv_norm, norms)");
  VIT_CHECK(n_mats > 0, VIT_ERR_ARG, "vit_muon_norms: n_mats = %d must be positive", n_mats);
  VIT_CHECK(eps > 0.f, VIT_ERR_ARG, "vit_muon_norms: eps = %g must be positive", (double)eps);
  hipLaunchKernelGGL(muon_norms_kernel, dim3(grid_for(n_mats, 1, 4096)), dim3(64), 0, (hipStream_t)stream, mats, n_mats, part, eps,
                     inv_norm, norms);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_muon_normalize(vit_handle h, const void* u, void* x, const vit_muon_mat* mats, int n_mats, int n_ttiles,
                       const float* inv_norm, vit_stream stream) {
  (void)h;
  VIT_CHECK(u && x && mats && inv_norm, VIT_ERR_ARG, "vit_muon_normalize: null pointer (u, x, mats, inv_norm)");
  VIT_CHECK(u != x, VIT_ERR_ARG, "vit_muon_normalize: x must not alias u (other tiles still read u)");
  VIT_CHECK(n_mats > 0 && n_ttiles > 0, VIT_ERR_ARG, "vit_muon_normalize: n_mats = %d and n_ttiles = %d must be positive", n_mats,
            n_ttiles);
  hipLaunchKernelGGL(muon_normalize_kernel, dim3(grid_for(n_ttiles, 1, 16384)), dim3(STEP_BLOCK), 0, (hipStream_t)stream,
                     (const short*)u, (short*)x, mats, n_mats, n_ttiles, inv_norm);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_muon_gemm_grouped(vit_handle h, const vit_muon_problem* problems, int n_problems, const int32_t* tiles, int n_tiles,
                          int b_trans, vit_stream stream) {
  (void)h;
  VIT_CHECK(problems && tiles, VIT_ERR_ARG, "vit_muon_gemm_grouped: null pointer (problems, tiles)");
  VIT_CHECK(n_problems > 0 && n_tiles > 0, VIT_ERR_ARG, "vit_muon_gemm_grouped: n_problems = %d and n_tiles = %d must be positive",
            n_problems, n_tiles);
  if (b_trans)
    hipLaunchKernelGGL((muon_gemm_kernel<true>), dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, problems, n_problems,
                       (const i32x4*)tiles);
  else
    hipLaunchKernelGGL((muon_gemm_kernel<false>), dim3(n_tiles), dim3(256), 0, (hipStream_t)stream, problems, n_problems,
                       (const i32x4*)tiles);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_muon_apply(vit_handle h, float* p, void* p_bf16, const void* o, const vit_muon_mat* mats, int n_mats, int n_ttiles,
                   const float* groups, int n_groups, vit_stream stream) {
  (void)h;
  VIT_CHECK(p && o && mats && groups, VIT_ERR_ARG, "vit_muon_apply: null pointer (p, o, mats, groups)");
  VIT_CHECK(n_mats > 0 && n_ttiles > 0 && n_groups > 0, VIT_ERR_ARG,
            "vit_muon_apply: n_mats = %d, n_ttiles = %d and n_groups = %d must be positive", n_mats, n_ttiles, n_groups);
  hipLaunchKernelGGL(muon_apply_kernel, dim3(grid_for(n_ttiles, 1, 16384)), dim3(STEP_BLOCK), 0, (hipStream_t)stream, p,
                     (short*)p_bf16, (const short*)o, mats, n_mats, n_ttiles, (const MuonRow*)groups, n_groups);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
