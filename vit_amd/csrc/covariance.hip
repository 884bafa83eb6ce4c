// Covariance statistics of [n, L] f32 spectra on exact-f32 MFMA (v_mfma_f32_32x32x2_f32): the arithmetic behind
// `warmup.cov_path` (reference: src/prepca/preprocessor_utils.py:426-430, `centered.t().matmul(centered) / (n - 1)`).
//
// vit_cov_accumulate is a symmetric rank-k update: acc[L, L] += (x - mean)^T (x - mean), only the 128 x 128 tiles on or above
// the diagonal.  The centring rides on the operand load (global -> registers -> LDS); no centred copy of x exists.  The f32
// MFMA is bit for bit a k-ordered fmaf chain, so an entry's error is an f32 chain's: the split-bf16 x3 products of the '32'
// GEMMs (~2^-16 relative) would drown the tail eigenvalues a ZCA front divides by.
//
// One workgroup = 4 waves = one 128 x 128 tile; a wave owns 64 x 64 of it as 2 x 2 MFMA tiles of 32 x 32: four independent
// 16-register accumulators, which is what the instruction's 64-cycle dependent latency needs at its 64-cycle issue interval.
// K (the row index of x) advances 16 rows per stage; the stage's two panels [16][128] sit in the LDS with a row stride of 160
// floats, so that the two lane halves of an operand read (rows k and k + 1) fall into disjoint banks.  The next stage's rows
// are loaded into registers before the current stage's MFMAs and written to the other LDS buffer after them: one barrier per
// stage.
//
// Fewer than 2048 upper tiles (L < 8192): the rows are split into S slices (at least 256 rows each) so that the device is filled
// and the grid's last round is short, slice s writes its tiles densely into
// workspace slab s, and cov_reduce_kernel adds the slabs to acc in slice order.  The plan depends on (n, L) alone -- not on
// the device's CU count, not on the workspace size -- and nothing uses a floating-point atomic: the result is a deterministic
// function of (x, mean, n, L).
#include <algorithm>

#include "common.h"

namespace vit {

typedef __attribute__((ext_vector_type(16))) float f32x16;

constexpr int COV_T = 128;         // tile edge
constexpr int COV_K = 16;          // rows of x per stage
constexpr int COV_LD = 160;        // LDS row stride in floats (128 + 32: rows k, k + 1 in disjoint bank halves)
constexpr int COV_FILL = 2048;     // workgroups wanted per launch: 8 per CU of a 256-CU device, so that the last round of a grid
                                   // that is no multiple of the resident workgroups (528 tiles at L = 4096) costs a few per cent
constexpr int COV_MIN_ROWS = 256;  // a slice shorter than this costs more in its slab traffic than it gains

// Four consecutive columns of one row, RAW: the address is clamped to a valid one (row r_safe / column 0) where the element is
// masked, so the load is unconditional -- no branch, and no use of the value until cov_centre at the LDS write, which is what
// lets the loads of stage k + 1 stay in flight under the MFMAs of stage k.  VEC: every base 16-byte aligned and L % 4 == 0, so
// a group of four columns is inside [0, L) or outside it as a whole.
template <bool VEC>
__device__ __forceinline__ f32x4 cov_load4(const float* __restrict__ x, long ldx, long row, int col, int L) {
  const float* p = x + row * ldx;
  if (VEC) return *(const f32x4*)(p + (col < L ? col : 0));
  f32x4 v;
#pragma unroll
  for (int e = 0; e < 4; ++e) v[e] = p[col + e < L ? col + e : 0];
  return v;
}

// centre, then mask: rows past the slice and columns past L are 0 AFTER the centring (a masked element must not become -mean)
__device__ __forceinline__ f32x4 cov_centre(f32x4 v, f32x4 mu, bool row_ok, int col, int L) {
  v -= mu;
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (!row_ok || col + e >= L) v[e] = 0.f;
  return v;
}

__device__ __forceinline__ f32x4 cov_mean4(const float* __restrict__ mean, int col, int L) {
  f32x4 mu = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e)
    if (col + e < L) mu[e] = mean[col + e];
  return mu;
}

// grid: (upper tiles, row slices).  slab == nullptr: acc += tile (every tile has one owner); else slab[slice][tile] = tile.
template <bool VEC>
__global__ __launch_bounds__(256) void cov_accumulate_kernel(const float* __restrict__ x, long ldx, const float* __restrict__ mean,
                                                             float* __restrict__ acc, float* __restrict__ slab, long n, int L, int nt,
                                                             long rows_per) {
  __shared__ float lds[2][2][COV_K * COV_LD];  // [stage][panel A (rows of the tile) / B (its columns)]
  int t = blockIdx.x, ti = 0, rowlen = nt;
  while (t >= rowlen) {  // tile row ti holds the nt - ti tiles (ti, ti) .. (ti, nt - 1)
    t -= rowlen;
    ++ti;
    --rowlen;
  }
  const int tj = ti + t;
  const bool diag = ti == tj;  // the two panels are the same columns: one is loaded
  const int i0 = ti * COV_T, j0 = tj * COV_T;
  const long r0 = (long)blockIdx.y * rows_per;
  const long r1 = r0 + rows_per < n ? r0 + rows_per : n;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wm = w >> 1, wn = w & 1, l31 = lane & 31, lh = lane >> 5;

  // loads: thread -> (row tid / 32 and that + 8 of the stage, 4 columns at (tid % 32) * 4): the columns are fixed, so is the mean
  const int lr = tid >> 5, lc = (tid & 31) * 4;
  const int ca = i0 + lc, cb = j0 + lc;
  const f32x4 mua = cov_mean4(mean, ca, L), mub = cov_mean4(mean, cb, L);
  f32x4 ga[2], gb[2];
  auto fetch = [&](long k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const long row = k0 + lr + 8 * r < r1 ? k0 + lr + 8 * r : r0;  // r0 < n: always a row of x
      ga[r] = cov_load4<VEC>(x, ldx, row, ca, L);
      if (!diag) gb[r] = cov_load4<VEC>(x, ldx, row, cb, L);
    }
  };
  auto commit = [&](int st, long k0) {
#pragma unroll
    for (int r = 0; r < 2; ++r) {
      const bool ok = k0 + lr + 8 * r < r1;
      *(f32x4*)&lds[st][0][(lr + 8 * r) * COV_LD + lc] = cov_centre(ga[r], mua, ok, ca, L);
      if (!diag) *(f32x4*)&lds[st][1][(lr + 8 * r) * COV_LD + lc] = cov_centre(gb[r], mub, ok, cb, L);
    }
  };

  f32x16 c[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) c[i][j][e] = 0.f;

  const long nk = (r1 - r0 + COV_K - 1) / COV_K;
  if (nk > 0) {
    fetch(r0);
    commit(0, r0);
  }
  __syncthreads();
  for (long kt = 0; kt < nk; ++kt) {
    const int cur = (int)(kt & 1);
    if (kt + 1 < nk) fetch(r0 + (kt + 1) * COV_K);
    const float* pa = &lds[cur][0][lh * COV_LD + wm * 64 + l31];
    const float* pb = &lds[cur][diag ? 0 : 1][lh * COV_LD + wn * 64 + l31];
    // lane l: A[i = l & 31][k = l >> 5] = xc[k][i0 + i], B[k = l >> 5][j = l & 31] = xc[k][j0 + j]; the whole stage's operands are
    // read first (32 registers), so no MFMA waits on the LDS
    float a[COV_K / 2][2], b[COV_K / 2][2];
#pragma unroll
    for (int s = 0; s < COV_K / 2; ++s) {
      a[s][0] = pa[2 * s * COV_LD], a[s][1] = pa[2 * s * COV_LD + 32];
      b[s][0] = pb[2 * s * COV_LD], b[s][1] = pb[2 * s * COV_LD + 32];
    }
    __builtin_amdgcn_sched_barrier(0);  // keep the reads above the MFMAs (the scheduler otherwise pairs each read with its use)
#pragma unroll
    for (int s = 0; s < COV_K / 2; ++s) {
      c[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][0], b[s][0], c[0][0], 0, 0, 0);
      c[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][0], b[s][1], c[0][1], 0, 0, 0);
      c[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][1], b[s][0], c[1][0], 0, 0, 0);
      c[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[s][1], b[s][1], c[1][1], 0, 0, 0);
    }
    if (kt + 1 < nk) commit(cur ^ 1, r0 + (kt + 1) * COV_K);
    __syncthreads();
  }

  // C/D map of the 32 x 32 forms: column = lane & 31, row = (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5)
  float* tile = slab ? slab + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * (size_t)(COV_T * COV_T) : nullptr;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int e = 0; e < 16; ++e) {
        const int r = wm * 64 + i * 32 + (e & 3) + 8 * (e >> 2) + 4 * lh;
        const int q = wn * 64 + j * 32 + l31;
        if (tile) {
          tile[r * COV_T + q] = c[i][j][e];
        } else if (i0 + r < L && j0 + q < L) {
          float* o = acc + (size_t)(i0 + r) * L + (j0 + q);
          *o += c[i][j][e];
        }
      }
}

// acc += slab[0] + slab[1] + ... in slice order (splitk_reduce_kernel's rule); grid (tiles, 8), 2048 elements of a tile each
__global__ __launch_bounds__(256) void cov_reduce_kernel(const float* __restrict__ slab, float* __restrict__ acc, int L, int nt,
                                                         int slices) {
  int t = blockIdx.x, ti = 0, rowlen = nt;
  while (t >= rowlen) {
    t -= rowlen;
    ++ti;
    --rowlen;
  }
  const int i0 = ti * COV_T, j0 = (ti + t) * COV_T;
  const size_t stride = (size_t)gridDim.x * (COV_T * COV_T);
  const float* s0 = slab + (size_t)blockIdx.x * (COV_T * COV_T);
  for (int e = blockIdx.y * 2048 + threadIdx.x; e < (int)(blockIdx.y + 1) * 2048; e += 256) {
    const int r = e >> 7, q = e & 127;
    if (i0 + r >= L || j0 + q >= L) continue;
    float a = s0[e];
    for (int s = 1; s < slices; ++s) a += s0[s * stride + e];
    acc[(size_t)(i0 + r) * L + (j0 + q)] += a;
  }
}

// cov[i][j] = cov[j][i] = acc[min(i, j)][max(i, j)] / denom: both halves are the SAME quotient, hence bitwise symmetric
__global__ __launch_bounds__(256) void cov_finish_kernel(const float* __restrict__ acc, float* __restrict__ cov, int L, float denom) {
  const size_t total = (size_t)L * L;
  for (size_t e = (size_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (size_t)gridDim.x * 256) {
    const size_t i = e / L, j = e - i * L;
    cov[e] = acc[i <= j ? e : j * L + i] / denom;
  }
}

__global__ __launch_bounds__(256) void cov_mean_finish_kernel(float* __restrict__ v, int L, float denom) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < L) v[c] = v[c] / denom;
}

// the launch plan of (n, L): row slices and rows per slice
static void cov_plan(long n, int L, int* slices, long* rows_per) {
  const long nt = cdiv(L, COV_T), tiles = nt * (nt + 1) / 2;
  long s = 1;
  if (tiles < COV_FILL) s = std::max(1L, std::min((COV_FILL + tiles - 1) / tiles, (n + COV_MIN_ROWS - 1) / COV_MIN_ROWS));
  long rp = (n + s - 1) / s;
  rp = (rp + COV_K - 1) / COV_K * COV_K;
  *rows_per = rp;
  *slices = (int)((n + rp - 1) / rp);
}

}  // namespace vit

using namespace vit;

extern "C" {

int vit_cov_accumulate(vit_handle h, const float* x, int64_t ldx, const float* mean, float* acc, int n, int L, vit_stream stream) {
  VIT_CHECK(x && mean && acc, VIT_ERR_ARG, "vit_cov_accumulate: null pointer");
  VIT_CHECK(n >= 1 && L >= 1 && ldx >= L, VIT_ERR_ARG, "vit_cov_accumulate: n=%d L=%d ldx=%ld (need n >= 1, L >= 1, ldx >= L)", n, L,
            (long)ldx);
  const int nt = cdiv(L, COV_T);
  const long tiles = (long)nt * (nt + 1) / 2;
  VIT_CHECK(tiles <= 0x7FFFFFFF, VIT_ERR_UNSUPPORTED, "vit_cov_accumulate: L=%d has too many tiles for one grid", L);
  int slices = 1;
  long rows_per = 0;
  cov_plan(n, L, &slices, &rows_per);
  VIT_CHECK(slices <= 65535, VIT_ERR_UNSUPPORTED, "vit_cov_accumulate: %d row slices", slices);
  hipStream_t st = (hipStream_t)stream;
  const bool vec = (ldx % 4) == 0 && (L % 4) == 0 && ((uintptr_t)x & 15) == 0;
  float* slab = nullptr;
  if (slices > 1) {
    slab = (float*)ctx_claim(h, (size_t)slices * tiles * COV_T * COV_T * sizeof(float), "vit_cov_accumulate");
    if (!slab) return VIT_ERR_WORKSPACE;
  }
  if (vec)
    hipLaunchKernelGGL(cov_accumulate_kernel<true>, dim3((unsigned)tiles, slices), dim3(256), 0, st, x, (long)ldx, mean, acc, slab,
                       (long)n, L, nt, rows_per);
  else
    hipLaunchKernelGGL(cov_accumulate_kernel<false>, dim3((unsigned)tiles, slices), dim3(256), 0, st, x, (long)ldx, mean, acc, slab,
                       (long)n, L, nt, rows_per);
  VIT_LAUNCH_CHECK();
  if (slab) {
    hipLaunchKernelGGL(cov_reduce_kernel, dim3((unsigned)tiles, 8), dim3(256), 0, st, slab, acc, L, nt, slices);
    VIT_LAUNCH_CHECK();
  }
  return VIT_OK;
}

int vit_cov_finish(vit_handle h, const float* acc, float* cov, int L, int64_t n_total, vit_stream stream) {
  (void)h;
  VIT_CHECK(acc && cov && acc != cov, VIT_ERR_ARG, "vit_cov_finish: null or aliased pointers");
  VIT_CHECK(L >= 1 && n_total >= 2, VIT_ERR_ARG, "vit_cov_finish: L=%d n_total=%ld (need L >= 1, n_total >= 2)", L, (long)n_total);
  const size_t total = (size_t)L * L;
  const int blocks = (int)std::min<size_t>((total + 255) / 256, 8192);
  hipLaunchKernelGGL(cov_finish_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, acc, cov, L, (float)(n_total - 1));
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_cov_mean_finish(vit_handle h, float* colsum, int L, int64_t n_total, vit_stream stream) {
  (void)h;
  VIT_CHECK(colsum && L >= 1 && n_total >= 1, VIT_ERR_ARG, "vit_cov_mean_finish: bad arguments (L=%d n_total=%ld)", L, (long)n_total);
  hipLaunchKernelGGL(cov_mean_finish_kernel, dim3(cdiv(L, 256)), dim3(256), 0, (hipStream_t)stream, colsum, L, (float)n_total);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // extern "C"
