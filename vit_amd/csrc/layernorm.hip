// LayerNorm forward / backward for gfx950: HBM-bound row kernels, one wave (64 lanes) per row.
// x is the fp32 residual stream; statistics, affine and the backward sums are fp32 (eps = 1e-12 is far below bf16
// resolution: SURVEY.md section 7).  Rows stay in registers between the statistics and the normalisation, so x is
// read from HBM exactly once per pass.  Cross-lane sums use wave shuffles (DPP/permute), no LDS.
#include <algorithm>

#include "common.h"

namespace vit {


// Stochastic depth ("drop path", include/vit_amd_droppath.h): a per-SAMPLE gate on the branch underneath a residual sum.  One
// wave owns one row, so the sample of a row, its draw and the multiplier that follows from it are wave-uniform: they are
// derived from the readfirstlane'd row index and stay in scalar registers.
struct PathCfg {
  DropCfg d;    // make_drop(path_p, seed, path_site): thr != 0 in every launch of a path form
  int rps;      // rows per sample, in the ORIGINAL row space
  int branch;   // 0 = attention branch, 1 = MLP branch: the two draw independently
  int xrs;      // forward: compact row r is original row r * xrs
};
// the multiplier of the branch for original row `orig`: draw index 2 * sample + branch, low 16 bits against thr; 0 = dropped.
// (k0, k1): the site's keys with the bound record's XORed in (resolve_drop)
__device__ __forceinline__ float path_mult(const PathCfg& p, unsigned k0, unsigned k1, int orig) {
  const unsigned b = __builtin_amdgcn_readfirstlane((unsigned)orig / (unsigned)p.rps);
  return (drop_hash(k0, k1, 2ull * b + (unsigned)p.branch) & 0xFFFFu) >= p.d.thr ? p.d.scale : 0.f;
}
__device__ __forceinline__ PathCfg path_of() { return PathCfg{}; }
__device__ __forceinline__ PathCfg path_of(const PathCfg& p) { return p; }

// NV = float4 chunks per lane held in registers; supports D <= 256*NV
// RES: 0 = plain; 1 / 2 = the row normalised is x + delta (delta bf16 / f32: the projection underneath a
// "dropout(Linear(.)) + residual"), and the sum is also written to xsum -- the new residual stream.
// Path: nothing (the plain forms: their instantiations, signatures and code are what they were without the pack), or one
// PathCfg (with RES): the sum is x + scale * delta for the rows of a kept sample and x for those of a dropped one, whose
// delta is not loaded.
template <int NV, int OUT_BF16, int RES, class... Path>
__global__ __launch_bounds__(256) void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ gamma,
                                                     const float* __restrict__ beta, void* __restrict__ y,
                                                     float* __restrict__ mean, float* __restrict__ rstd, int rows,
                                                     int D, float eps, const void* __restrict__ delta,
                                                     float* __restrict__ xsum, long x_ld, Path... path_arg) {
  constexpr bool PATH = sizeof...(Path) != 0;
  const PathCfg path = path_of(path_arg...);
  const int lane = threadIdx.x & 63;
  const int wave = PATH ? __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6)
                        : (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int nvec = D >> 2;
  const float invD = 1.0f / (float)D;
  unsigned pk0 = path.d.k0, pk1 = path.d.k1;  // resolve_drop: the bound record's keys
  if (PATH && path.d.dyn) {
    pk0 ^= path.d.dyn[0];
    pk1 ^= path.d.dyn[1];
  }
  for (int row = wave; row < rows; row += nwaves) {
    const float* xr = x + (long)row * x_ld;  // x_ld = D, or a multiple of it: a strided subset of the stream's rows
    f32x4 v[NV];
    float s = 0.f;
    // PATH: 0 for the rows of a dropped sample, the kept-branch scale otherwise -- wave-uniform, in a scalar register
    const float pm = PATH ? path_mult(path, pk0, pk1, row * path.xrs) : 1.f;
    if (PATH && pm == 0.f) {  // a dropped sample: the stream passes through, its delta is never loaded
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = (c < nvec) ? *(const f32x4*)(xr + 4 * c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (c < nvec) *(f32x4*)(xsum + (long)row * D + 4 * c) = v[i];
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      }
    } else {
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        v[i] = (c < nvec) ? *(const f32x4*)(xr + 4 * c) : (f32x4){0.f, 0.f, 0.f, 0.f};
        if (RES && c < nvec) {
          f32x4 dl;
          if (RES == 1) {
            const bf16x4 t = *(const bf16x4*)((const short*)delta + (long)row * D + 4 * c);
            dl = (f32x4){bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3])};
          } else {
            dl = *(const f32x4*)((const float*)delta + (long)row * D + 4 * c);
          }
          if (PATH) v[i] += dl * pm;
          else v[i] += dl;
          *(f32x4*)(xsum + (long)row * D + 4 * c) = v[i];
        }
        s += (v[i][0] + v[i][1]) + (v[i][2] + v[i][3]);
      }
    }
    const float mu = wave_sum(s) * invD;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        f32x4 d = v[i] - mu;
        q += (d[0] * d[0] + d[1] * d[1]) + (d[2] * d[2] + d[3] * d[3]);
      }
    }
    const float rs = rsqrtf(wave_sum(q) * invD + eps);
    if (lane == 0) {
      if (mean) mean[row] = mu;
      if (rstd) rstd[row] = rs;
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        const f32x4 g = *(const f32x4*)(gamma + 4 * c);
        const f32x4 b = *(const f32x4*)(beta + 4 * c);
        const f32x4 o = (v[i] - mu) * rs * g + b;
        if (OUT_BF16) {
          u32x2 pk = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
          *(u32x2*)((short*)y + (long)row * D + 4 * c) = pk;
        } else {
          *(f32x4*)((float*)y + (long)row * D + 4 * c) = o;
        }
      }
    }
  }
}

// Row maps of the backward at the two ends of a compact run of rows (vit_layernorm_bwd_rows); {0, 0} = none.
// compact_stride s > 0: `rows` counts the rows of the FULL tensor, of which only the rows r with r % s == 0 exist; dy, x, mean,
// rstd, dx, dyn (and dres, unless dres_stride says otherwise) hold them compactly at r / s.  The kernel walks the full row
// space with the full tensor's grid and skips the absent rows, so every wave meets its rows in the order it would meet them
// in the full tensor (whose other rows contribute exact zeros) and the partial sums -- dgamma, dbeta, dbias -- come out bit for
// bit the full pass's; the dropout key row is r itself.
struct RowMap {
  int compact_stride;
  int dres_stride;  // 0 = dres is laid out like dx; s > 0 = dres is compact while dx is full: row j of it belongs to row j * s
};

// backward: dx = rstd * (g - mean(g) - xhat * mean(g*xhat)) + dres,  g = dy*gamma, xhat = (x-mean)*rstd
// per-wave running sums of dy*xhat (dgamma) and dy (dbeta) over the rows the wave visits; block-combined through LDS
// and written as one partial row per block: part[blk][0][D] (dgamma), part[blk][1][D] (dbeta).
// FUSE: additionally emit dyn = dropout_mask(drop) * dx as bf16 (the gradient wrt the Linear output that sits under the
// "dropout(.) + residual" this LayerNorm's input came from) and its column sums (that Linear's bias gradient) as a
// third partial row -- what vit_dropout_bwd_cast + vit_colsum would otherwise re-read dx for.
// FUSE: 0 = plain, 1 = + bf16 dyn, 2 = + f32 dyn
// PATH (with FUSE): the Linear under the sum sits in a drop-path branch, dyn = k * mask * dx with ONE multiplier per row: the
// f32 product drop.scale * path.scale for a kept sample, 0 for a dropped one (whose rows still run, in their place in the
// order of the partial sums).  dx, dgamma and dbeta do not see the gate.
template <int NV, int DY_BF16, int FUSE, class... Path>
__global__ __launch_bounds__(1024) void ln_bwd_kernel(const void* __restrict__ dy, const float* __restrict__ x,
                                                     const float* __restrict__ gamma, const float* __restrict__ mean,
                                                     const float* __restrict__ rstd, const float* __restrict__ dres,
                                                     float* __restrict__ dx, float* __restrict__ part, int rows, int D,
                                                     void* __restrict__ dyn, DropCfg drop, RowMap rm, Path... path_arg) {
  constexpr bool PATH = sizeof...(Path) != 0;
  const PathCfg path = path_of(path_arg...);
  resolve_drop(drop);
  unsigned pk0 = path.d.k0, pk1 = path.d.k1;
  if (PATH && path.d.dyn) {
    pk0 ^= path.d.dyn[0];
    pk1 ^= path.d.dyn[1];
  }
  constexpr int NP = FUSE ? 3 : 2;
  extern __shared__ __attribute__((aligned(16))) float red[];  // [4 waves][NP][D], used by four waves at a time
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  // the same in every lane of a wave, and said so: the row index and what is derived from it (row base offsets, the row's
  // statistics, the compact-dres row, the dropout key row) stay in scalar registers
  const int wave = __builtin_amdgcn_readfirstlane((blockIdx.x * blockDim.x + threadIdx.x) >> 6);
  const int nwaves = (gridDim.x * blockDim.x) >> 6;
  const int nvec = D >> 2;
  const float invD = 1.0f / (float)D;
  // gamma: in registers up to D = 768; from D = 1024 (NV = 4, ViT-L) in the LDS behind the reduction buffer -- with three
  // accumulator sets of NV x 4 registers the fused form spilled 14 registers per lane at 128 VGPRs (4 waves per SIMD) and its
  // scratch traffic sat inside the row loop (r03: 4.2 TB/s at ViT-L against 6.0 TB/s at ViT-B)
  constexpr bool GAM_LDS = NV >= 4 && FUSE != 0;
  float* gam_s = red + 4 * NP * D;
  f32x4 gam[GAM_LDS ? 1 : NV], dg[NV], db[NV], dbias[FUSE ? NV : 1];
  if (GAM_LDS) {
    for (int i = threadIdx.x; i < nvec; i += blockDim.x) *(f32x4*)(gam_s + 4 * i) = *(const f32x4*)(gamma + 4 * i);
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int c = lane + 64 * i;
    if (!GAM_LDS) gam[i] = (c < nvec) ? *(const f32x4*)(gamma + 4 * c) : (f32x4){0.f, 0.f, 0.f, 0.f};
    dg[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    db[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
    if (FUSE) dbias[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
  }
  const float drop_scale = drop.scale;  // 1 with the hidden dropout off
  for (int row = wave; row < rows; row += nwaves) {
    int idx = row;  // where the row lives in the tensors
    if (rm.compact_stride) {
      idx = row / rm.compact_stride;
      if (idx * rm.compact_stride != row) continue;
    }
    const float mu = mean[idx], rs = rstd[idx];
    // the residual gradient of this row: laid out like dx, or compact and present for every dres_stride-th row only
    const float* dr = dres ? dres + (long)idx * D : nullptr;
    if (rm.dres_stride) {
      const int j = row / rm.dres_stride;
      dr = (dres && j * rm.dres_stride == row) ? dres + (long)j * D : nullptr;
    }
    if (PATH) drop.scale = drop_scale * path_mult(path, pk0, pk1, row);  // the row's multiplier, a scalar
    f32x4 xh[NV], g[NV];
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        f32x4 d;
        if (DY_BF16) {
          bf16x4 t = *(const bf16x4*)((const short*)dy + (long)idx * D + 4 * c);
          d = (f32x4){bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3])};
        } else {
          d = *(const f32x4*)((const float*)dy + (long)idx * D + 4 * c);
        }
        xh[i] = (*(const f32x4*)(x + (long)idx * D + 4 * c) - mu) * rs;
        g[i] = d * (GAM_LDS ? *(const f32x4*)(gam_s + 4 * c) : gam[GAM_LDS ? 0 : i]);
        dg[i] += d * xh[i];
        db[i] += d;
        s1 += (g[i][0] + g[i][1]) + (g[i][2] + g[i][3]);
        const f32x4 t2 = g[i] * xh[i];
        s2 += (t2[0] + t2[1]) + (t2[2] + t2[3]);
      } else {
        xh[i] = g[i] = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
    }
    const float c1 = wave_sum(s1) * invD, c2 = wave_sum(s2) * invD;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
      const int c = lane + 64 * i;
      if (c < nvec) {
        f32x4 o = (g[i] - c1 - xh[i] * c2) * rs;
        if (dr) o += *(const f32x4*)(dr + 4 * c);
        *(f32x4*)(dx + (long)idx * D + 4 * c) = o;
        if (FUSE) {
          if (drop.thr && (!PATH || drop.scale != 0.f)) {
            float k0, k1, k2, k3;
            drop_pair(drop, (unsigned long long)row, (unsigned)(4 * c), k0, k1);
            drop_pair(drop, (unsigned long long)row, (unsigned)(4 * c) + 2, k2, k3);
            o[0] *= k0; o[1] *= k1; o[2] *= k2; o[3] *= k3;
          } else if (PATH) {
            o *= drop.scale;
          }
          if (FUSE == 1) {
            u32x2 pk = {pack2bf(o[0], o[1]), pack2bf(o[2], o[3])};
            *(u32x2*)((short*)dyn + (long)idx * D + 4 * c) = pk;
            // sum what was stored (bf16-rounded), exactly like colsum over the bf16 tensor would
            dbias[i] += (f32x4){bf2f((short)(pk[0] & 0xFFFF)), bf2f((short)(pk[0] >> 16)), bf2f((short)(pk[1] & 0xFFFF)),
                                bf2f((short)(pk[1] >> 16))};
          } else {
            *(f32x4*)((float*)dyn + (long)idx * D + 4 * c) = o;
            dbias[i] += o;
          }
        }
      }
    }
  }
  // block combine, four waves at a time through the same 4 x NP x D floats (a 16-wave block = one partial row per CU: 256
  // rows for the reducer instead of 1024, no first reduction stage); each thread owns the columns tid, tid + blockDim, ...
  const int nw = blockDim.x >> 6, ngrp = (nw + 3) >> 2;
  constexpr int KMAX = 16;  // columns per thread: NP * D <= 4096 = 16 * 256 at every shape the dispatch accepts
  float tot[KMAX];
#pragma unroll
  for (int k = 0; k < KMAX; ++k) tot[k] = 0.f;
  for (int gq = 0; gq < ngrp; ++gq) {
    if ((wib >> 2) == gq) {
      const int w4 = wib & 3;
#pragma unroll
      for (int i = 0; i < NV; ++i) {
        const int c = lane + 64 * i;
        if (c < nvec) {
          *(f32x4*)(red + (w4 * NP + 0) * D + 4 * c) = dg[i];
          *(f32x4*)(red + (w4 * NP + 1) * D + 4 * c) = db[i];
          if (FUSE) *(f32x4*)(red + (w4 * NP + 2) * D + 4 * c) = dbias[i];
        }
      }
    }
    __syncthreads();
    const int nw4 = min(4, nw - gq * 4);
#pragma unroll
    for (int k = 0; k < KMAX; ++k) {
      const int i = threadIdx.x + k * blockDim.x;
      if (i < NP * D) {
        float a = 0.f;
        for (int w = 0; w < nw4; ++w) a += red[w * NP * D + i];
        tot[k] += a;
      }
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < KMAX; ++k) {
    const int i = threadIdx.x + k * blockDim.x;
    if (i < NP * D) part[(long)blockIdx.x * NP * D + i] = tot[k];
  }
}

template <int OUT_BF16, int RES>
static int ln_fwd_dispatch(const float* x, const float* g, const float* b, void* y, float* mean, float* rstd, int rows,
                           int D, float eps, hipStream_t st, const void* delta = nullptr, float* xsum = nullptr,
                           long x_ld = 0, const PathCfg* path = nullptr) {
  if (x_ld == 0) x_ld = D;
  const int nv = cdiv(D, 256);
  // one round of resident 4-wave blocks over 256 CUs: 8 per CU up to D = 768 (<= 64 VGPRs), 7 at D = 1024 (72 VGPRs)
  constexpr int BLOCKS_NARROW = 2048, BLOCKS_WIDE = 1792;
  const int blocks = std::min(cdiv(rows, 4), nv >= 4 ? BLOCKS_WIDE : BLOCKS_NARROW);
  // the path form runs the plain form's grid: it needs no more registers at any NV (profiles/droppath_resources.txt)
#define LAUNCH(NV)                                                                                                           \
  do {                                                                                                                       \
    if constexpr (RES != 0) {                                                                                                \
      if (path) {                                                                                                            \
        hipLaunchKernelGGL((ln_fwd_kernel<NV, OUT_BF16, RES, PathCfg>), dim3(blocks), dim3(256), 0, st, x, g, b, y, mean, rstd, \
                           rows, D, eps, delta, xsum, x_ld, *path);                                                          \
        break;                                                                                                               \
      }                                                                                                                      \
    }                                                                                                                        \
    hipLaunchKernelGGL((ln_fwd_kernel<NV, OUT_BF16, RES>), dim3(blocks), dim3(256), 0, st, x, g, b, y, mean, rstd, rows, D, \
                       eps, delta, xsum, x_ld);                                                                              \
  } while (0)
  if (nv <= 1) LAUNCH(1);
  else if (nv <= 2) LAUNCH(2);
  else if (nv <= 3) LAUNCH(3);
  else if (nv <= 4) LAUNCH(4);
  else if (nv <= 8) LAUNCH(8);
  else { set_error("vit_layernorm_fwd: D=%d > 2048 not supported", D); return VIT_ERR_UNSUPPORTED; }
#undef LAUNCH
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

template <int DY_BF16, int FUSE>
static int ln_bwd_dispatch(const void* dy, const float* x, const float* g, const float* mean, const float* rstd,
                           const float* dres, float* dx, float* part, int rows, int D, int blocks, int threads,
                           void* dyn, DropCfg drop, RowMap rm, hipStream_t st, const PathCfg* path) {
  const int nv = cdiv(D, 256);
  const size_t sh = (size_t)4 * (FUSE ? 3 : 2) * D * sizeof(float) + (FUSE && nv >= 4 ? (size_t)D * sizeof(float) : 0);
  if (sh > 64 * 1024) { set_error("vit_layernorm_bwd: D=%d needs %zu bytes of LDS", D, sh); return VIT_ERR_UNSUPPORTED; }
#define LAUNCH(NV)                                                                                                           \
  do {                                                                                                                       \
    if constexpr (FUSE != 0 && NV <= 4) {                                                                                    \
      if (path) {                                                                                                            \
        hipLaunchKernelGGL((ln_bwd_kernel<NV, DY_BF16, FUSE, PathCfg>), dim3(blocks), dim3(threads), sh, st, dy, x, g, mean,    \
                           rstd, dres, dx, part, rows, D, dyn, drop, rm, *path);                                             \
        break;                                                                                                               \
      }                                                                                                                      \
    }                                                                                                                        \
    hipLaunchKernelGGL((ln_bwd_kernel<NV, DY_BF16, FUSE>), dim3(blocks), dim3(threads), sh, st, dy, x, g, mean, rstd, dres, \
                       dx, part, rows, D, dyn, drop, rm);                                                                    \
  } while (0)
  if (nv <= 1) LAUNCH(1);
  else if (nv <= 2) LAUNCH(2);
  else if (nv <= 3) LAUNCH(3);
  else if (nv <= 4) LAUNCH(4);
  else if (nv <= 8 && !FUSE) LAUNCH(8);
  else { set_error("vit_layernorm_bwd: D=%d not supported (max 2048, 1024 for the fused form)", D); return VIT_ERR_UNSUPPORTED; }
#undef LAUNCH
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

static int ln_bwd_common(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma,
                         const float* mean, const float* rstd, const float* dres, float* dx, float* dgamma,
                         float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, DropCfg drop,
                         hipStream_t st, RowMap rm = {0, 0}, const PathCfg* path = nullptr) {
  // 16 waves per CU: with only two waves per SIMD the pass was latency-bound at 4.3 TB/s (bytes in flight / HBM latency).
  // They are TWO blocks of 512 threads per CU when there are rows for it: a block's waves combine through the LDS four at a
  // time (36 KiB at D = 768), so the pass leaves 512 partial rows instead of 1024 and the reducer needs no first stage (25
  // launches of 7 us per step).  Pass + reducers on one box: 4-wave blocks and two reducer stages ~123 us, one 16-wave block
  // per CU 126.1 us (the pass itself got 5 % slower), 8-wave blocks 122.0 us.  Small inputs keep 4-wave blocks.
  const int np = dyn ? 3 : 2;
  const bool big = rows >= 256 * 16;
  const int threads = big ? 512 : 256;
  const int blocks = big ? 512 : std::min(cdiv(rows, 16), 1024);
  float* part = (float*)ctx_claim(h, (size_t)blocks * np * D * sizeof(float), "vit_layernorm_bwd");
  if (!part) return VIT_ERR_WORKSPACE;
  int rc;
  if (dyn && dyn_dtype == VIT_BF16)
    rc = dy_dtype == VIT_BF16 ? ln_bwd_dispatch<1, 1>(dy, x, gamma, mean, rstd, dres, dx, part, rows, D, blocks, threads, dyn, drop, rm, st, path)
                              : ln_bwd_dispatch<0, 1>(dy, x, gamma, mean, rstd, dres, dx, part, rows, D, blocks, threads, dyn, drop, rm, st, path);
  else if (dyn)
    rc = dy_dtype == VIT_BF16 ? ln_bwd_dispatch<1, 2>(dy, x, gamma, mean, rstd, dres, dx, part, rows, D, blocks, threads, dyn, drop, rm, st, path)
                              : ln_bwd_dispatch<0, 2>(dy, x, gamma, mean, rstd, dres, dx, part, rows, D, blocks, threads, dyn, drop, rm, st, path);
  else rc = dy_dtype == VIT_BF16 ? ln_bwd_dispatch<1, 0>(dy, x, gamma, mean, rstd, dres, dx, part, rows, D, blocks, threads, dyn, drop, rm, st, path)
                                 : ln_bwd_dispatch<0, 0>(dy, x, gamma, mean, rstd, dres, dx, part, rows, D, blocks, threads, dyn, drop, rm, st, path);
  if (rc != VIT_OK) return rc;
  const int accum = ctx_grad_accumulate(h);  // dgamma / dbeta / dbias += : the add sits in the reducer's one store per column
  if (!dyn) return launch_reduce_partials(part, blocks, 2 * D, dgamma, D, dbeta, accum, st, np * D);
  return launch_reduce_partials(part, blocks, 3 * D, dgamma, D, dbeta, accum, st, np * D, 2 * D, dbias);  // one launch for all three
}

}  // namespace vit

extern "C" {

int vit_layernorm_fwd(vit_handle h, const float* x, const float* gamma, const float* beta, void* y, int y_dtype,
                      float* mean, float* rstd, int rows, int D, float eps, vit_stream stream) {
  using namespace vit;
  (void)h;
  VIT_CHECK(x && gamma && beta && y, VIT_ERR_ARG, "vit_layernorm_fwd: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_fwd: rows=%d D=%d (D must be a multiple of 4)", rows, D);
  VIT_CHECK(y_dtype == VIT_BF16 || y_dtype == VIT_F32, VIT_ERR_ARG, "vit_layernorm_fwd: bad y_dtype");
  hipStream_t st = (hipStream_t)stream;
  return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 0>(x, gamma, beta, y, mean, rstd, rows, D, eps, st)
                             : ln_fwd_dispatch<0, 0>(x, gamma, beta, y, mean, rstd, rows, D, eps, st);
}

int vit_layernorm_fwd_residual(vit_handle h, const float* x, const void* delta, int delta_dtype, float* xsum,
                               const float* gamma, const float* beta, void* y, int y_dtype, float* mean, float* rstd,
                               int rows, int D, float eps, vit_stream stream) {
  using namespace vit;
  (void)h;
  VIT_CHECK(x && delta && xsum && gamma && beta && y, VIT_ERR_ARG, "vit_layernorm_fwd_residual: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_fwd_residual: rows=%d D=%d (D must be a multiple of 4)", rows, D);
  VIT_CHECK((y_dtype == VIT_BF16 || y_dtype == VIT_F32) && (delta_dtype == VIT_BF16 || delta_dtype == VIT_F32), VIT_ERR_ARG,
            "vit_layernorm_fwd_residual: bad dtype");
  hipStream_t st = (hipStream_t)stream;
  if (delta_dtype == VIT_BF16)
    return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 1>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum)
                               : ln_fwd_dispatch<0, 1>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum);
  return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 2>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum)
                             : ln_fwd_dispatch<0, 2>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum);
}

int vit_layernorm_fwd_residual_rows(vit_handle h, const float* x, int64_t x_row_stride, const void* delta, int delta_dtype,
                                    float* xsum, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                                    float* rstd, int rows, int D, float eps, vit_stream stream) {
  using namespace vit;
  (void)h;
  VIT_CHECK(x && delta && xsum && gamma && beta && y, VIT_ERR_ARG, "vit_layernorm_fwd_residual_rows: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_fwd_residual_rows: rows=%d D=%d (D must be a multiple of 4)", rows, D);
  VIT_CHECK(x_row_stride >= 1, VIT_ERR_ARG, "vit_layernorm_fwd_residual_rows: x_row_stride=%lld", (long long)x_row_stride);
  VIT_CHECK((y_dtype == VIT_BF16 || y_dtype == VIT_F32) && (delta_dtype == VIT_BF16 || delta_dtype == VIT_F32), VIT_ERR_ARG,
            "vit_layernorm_fwd_residual_rows: bad dtype");
  hipStream_t st = (hipStream_t)stream;
  const long x_ld = (long)x_row_stride * D;
  if (delta_dtype == VIT_BF16)
    return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 1>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld)
                               : ln_fwd_dispatch<0, 1>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld);
  return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 2>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld)
                             : ln_fwd_dispatch<0, 2>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld);
}

int vit_layernorm_bwd(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma,
                      const float* mean, const float* rstd, const float* dres, float* dx, float* dgamma,
                      float* dbeta, int rows, int D, vit_stream stream) {
  using namespace vit;
  VIT_CHECK(dy && x && gamma && mean && rstd && dx && dgamma && dbeta, VIT_ERR_ARG, "vit_layernorm_bwd: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_bwd: rows=%d D=%d", rows, D);
  return ln_bwd_common(h, dy, dy_dtype, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, D, nullptr, VIT_BF16, nullptr,
                       make_drop(0.f, 0, 0), (hipStream_t)stream);
}

int vit_layernorm_bwd_fused(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma,
                            const float* mean, const float* rstd, const float* dres, float* dx, float* dgamma,
                            float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, float dropout_p,
                            uint64_t seed, uint64_t site, vit_stream stream) {
  using namespace vit;
  VIT_CHECK(dy && x && gamma && mean && rstd && dx && dgamma && dbeta && dyn && dbias, VIT_ERR_ARG,
            "vit_layernorm_bwd_fused: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_bwd_fused: rows=%d D=%d", rows, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_layernorm_bwd_fused: dropout_p out of [0,1)");
  return ln_bwd_common(h, dy, dy_dtype, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, D, dyn, dyn_dtype, dbias,
                       make_drop_h(h, dropout_p, seed, site), (hipStream_t)stream);
}

int vit_layernorm_bwd_rows(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const float* dres, int64_t dres_row_stride, float* dx, float* dgamma,
                           float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, float dropout_p,
                           uint64_t seed, uint64_t site, int64_t row_stride, vit_stream stream) {
  using namespace vit;
  VIT_CHECK(dy && x && gamma && mean && rstd && dx && dgamma && dbeta && (!dyn || dbias), VIT_ERR_ARG,
            "vit_layernorm_bwd_rows: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_bwd_rows: rows=%d D=%d", rows, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_layernorm_bwd_rows: dropout_p out of [0,1)");
  VIT_CHECK(dres_row_stride >= 0 && dres_row_stride <= 0x7FFFFFFF && row_stride >= 1 && row_stride <= 0x7FFFFFFF,
            VIT_ERR_ARG, "vit_layernorm_bwd_rows: dres_row_stride=%lld row_stride=%lld", (long long)dres_row_stride,
            (long long)row_stride);
  VIT_CHECK(!(row_stride > 1 && dres_row_stride > 0), VIT_ERR_ARG, "vit_layernorm_bwd_rows: a compact dres needs full rows");
  const RowMap rm = {row_stride > 1 ? (int)row_stride : 0, (int)dres_row_stride};
  if (!dyn)
    return ln_bwd_common(h, dy, dy_dtype, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, D, nullptr, VIT_BF16, nullptr,
                         make_drop(0.f, 0, 0), (hipStream_t)stream, rm);
  return ln_bwd_common(h, dy, dy_dtype, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, D, dyn, dyn_dtype, dbias,
                       make_drop_h(h, dropout_p, seed, site), (hipStream_t)stream, rm);
}

// ---- stochastic depth (include/vit_amd_droppath.h) ------------------------------------------------------------------
int vit_layernorm_fwd_residual_path(vit_handle h, const float* x, int64_t x_row_stride, const void* delta, int delta_dtype,
                                    float* xsum, const float* gamma, const float* beta, void* y, int y_dtype, float* mean,
                                    float* rstd, int rows, int D, float eps, float path_p, uint64_t seed, uint64_t path_site,
                                    int rows_per_sample, int branch, vit_stream stream) {
  using namespace vit;
  VIT_CHECK(x && delta && xsum && gamma && beta && y, VIT_ERR_ARG, "vit_layernorm_fwd_residual_path: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_fwd_residual_path: rows=%d D=%d (D must be a multiple of 4)", rows, D);
  VIT_CHECK(x_row_stride >= 1 && (int64_t)rows * x_row_stride <= 0x7FFFFFFF, VIT_ERR_ARG,
            "vit_layernorm_fwd_residual_path: x_row_stride=%lld (rows * x_row_stride must stay below 2^31)", (long long)x_row_stride);
  VIT_CHECK((y_dtype == VIT_BF16 || y_dtype == VIT_F32) && (delta_dtype == VIT_BF16 || delta_dtype == VIT_F32), VIT_ERR_ARG,
            "vit_layernorm_fwd_residual_path: bad dtype");
  VIT_CHECK(path_p >= 0.f && path_p < 1.f, VIT_ERR_ARG, "vit_layernorm_fwd_residual_path: path_p out of [0,1)");
  VIT_CHECK(rows_per_sample > 0 && (branch == 0 || branch == 1), VIT_ERR_ARG,
            "vit_layernorm_fwd_residual_path: rows_per_sample=%d branch=%d", rows_per_sample, branch);
  hipStream_t st = (hipStream_t)stream;
  const long x_ld = (long)x_row_stride * D;
  const PathCfg pc = {make_drop_h(h, path_p, seed, path_site), rows_per_sample, branch, (int)x_row_stride};
  const PathCfg* path = pc.d.thr ? &pc : nullptr;  // rate 0: the plain form, its launch and its bits
  if (delta_dtype == VIT_BF16)
    return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 1>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld, path)
                               : ln_fwd_dispatch<0, 1>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld, path);
  return y_dtype == VIT_BF16 ? ln_fwd_dispatch<1, 2>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld, path)
                             : ln_fwd_dispatch<0, 2>(x, gamma, beta, y, mean, rstd, rows, D, eps, st, delta, xsum, x_ld, path);
}

int vit_layernorm_bwd_path(vit_handle h, const void* dy, int dy_dtype, const float* x, const float* gamma, const float* mean,
                           const float* rstd, const float* dres, int64_t dres_row_stride, float* dx, float* dgamma,
                           float* dbeta, int rows, int D, void* dyn, int dyn_dtype, float* dbias, float dropout_p,
                           uint64_t seed, uint64_t site, int64_t row_stride, float path_p, uint64_t path_site,
                           int rows_per_sample, int branch, vit_stream stream) {
  using namespace vit;
  VIT_CHECK(dy && x && gamma && mean && rstd && dx && dgamma && dbeta && dyn && dbias, VIT_ERR_ARG,
            "vit_layernorm_bwd_path: null pointer");
  VIT_CHECK(rows > 0 && D > 0 && (D % 4) == 0, VIT_ERR_ARG, "vit_layernorm_bwd_path: rows=%d D=%d", rows, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "vit_layernorm_bwd_path: dropout_p out of [0,1)");
  VIT_CHECK(dres_row_stride >= 0 && dres_row_stride <= 0x7FFFFFFF && row_stride >= 1 && row_stride <= 0x7FFFFFFF,
            VIT_ERR_ARG, "vit_layernorm_bwd_path: dres_row_stride=%lld row_stride=%lld", (long long)dres_row_stride,
            (long long)row_stride);
  VIT_CHECK(!(row_stride > 1 && dres_row_stride > 0), VIT_ERR_ARG, "vit_layernorm_bwd_path: a compact dres needs full rows");
  VIT_CHECK(path_p >= 0.f && path_p < 1.f, VIT_ERR_ARG, "vit_layernorm_bwd_path: path_p out of [0,1)");
  VIT_CHECK(rows_per_sample > 0 && (branch == 0 || branch == 1), VIT_ERR_ARG,
            "vit_layernorm_bwd_path: rows_per_sample=%d branch=%d", rows_per_sample, branch);
  const RowMap rm = {row_stride > 1 ? (int)row_stride : 0, (int)dres_row_stride};
  const PathCfg pc = {make_drop_h(h, path_p, seed, path_site), rows_per_sample, branch, 1};
  return ln_bwd_common(h, dy, dy_dtype, x, gamma, mean, rstd, dres, dx, dgamma, dbeta, rows, D, dyn, dyn_dtype, dbias,
                       make_drop_h(h, dropout_p, seed, site), (hipStream_t)stream, rm, pc.d.thr ? &pc : nullptr);
}

}  // extern "C"
