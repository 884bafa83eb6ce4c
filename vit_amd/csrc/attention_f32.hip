#include "attention.h"

namespace vit {

// ======================================================================================= fp32 attention (precision '32')
// Exact-arithmetic path behind the reference's default precision: fp32 in, fp32 FMAs, fp32 out; one wave per query row
// (forward, dQ) or key row (dK/dV); scores / probabilities of the row live in the wave's LDS slice.  The fp32 matrix
// instructions run at the vector rate on gfx950, so nothing is lost by using the vector units; this path is for
// parity-grade runs, the bf16 kernels are the throughput path.  qkv: f32 [B*T, 3*H*dh].
__device__ __forceinline__ float drop_mult(const DropCfg& d, unsigned long long row, unsigned col) {
  if (!d.thr) return 1.f;
  const unsigned h = drop_bits(drop_rowkey(d, row), col >> 1);
  const unsigned r16 = (col & 1) ? (h >> 16) : (h & 0xFFFFu);
  return r16 >= d.thr ? d.scale : 0.f;
}
__device__ __forceinline__ float dot_row(const float* __restrict__ a_lds, const float* __restrict__ g, int dh) {
  float s = 0.f;
  for (int d = 0; d < dh; d += 4) {
    const f32x4 x = *(const f32x4*)(a_lds + d), y = *(const f32x4*)(g + d);
    s = fmaf(x[0], y[0], s); s = fmaf(x[1], y[1], s); s = fmaf(x[2], y[2], s); s = fmaf(x[3], y[3], s);
  }
  return s;
}

// MODE 0: forward (ctx, lse, optional probs)   MODE 1: dQ (+ delta)
template <int MODE>
__global__ __launch_bounds__(256) void attn32_row_kernel(Attn32Args p) {
  resolve_drop(p.drop);
  extern __shared__ __attribute__((aligned(16))) float sm32[];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wib;  // (b*H + h)*T + q
  if (row >= (long)p.B * p.H * p.T) return;      // whole waves only; no block barrier is used below
  const int T = p.T, dh = p.dh, H = p.H;
  const int q = (int)(row % T);
  const long bh = row / T;
  const int h = (int)(bh % H);
  const long b = bh / H;
  const long ld = 3L * H * dh, ldc = (long)H * dh;
  float* pr = sm32 + wib * (2 * p.Tp + 2 * 128);  // [Tp] p or p*mask, [Tp] ds, [128] q row, [128] dO row
  float* ds = pr + p.Tp;
  float* qrow = ds + p.Tp;
  float* dorow = qrow + 128;
  const float* qp = p.qkv + (b * T + q) * ld + h * dh;
  const float* kbase = p.qkv + b * T * ld + H * dh + h * dh;
  const float* vbase = kbase + H * dh;
  for (int d = lane; d < dh; d += 64) {
    qrow[d] = qp[d];
    if (MODE == 1) dorow[d] = p.dctx[(b * T + q) * ldc + h * dh + d];
  }
  __builtin_amdgcn_wave_barrier();  // LDS ops of one wave execute in order; this only pins the compiler's schedule
  const unsigned long long drow = (unsigned long long)row;
  if (MODE == 0) {
    float mx = -INFINITY;
    for (int k = lane; k < T; k += 64) {
      const float sc = dot_row(qrow, kbase + (long)k * ld, dh) * p.scale;
      pr[k] = sc;
      mx = fmaxf(mx, sc);
    }
    __builtin_amdgcn_wave_barrier();
    mx = wave_max(mx);
    float sum = 0.f;
    for (int k = lane; k < T; k += 64) {
      const float e = expf(pr[k] - mx);
      pr[k] = e;
      sum += e;
    }
    sum = wave_sum(sum);
    const float inv = 1.f / sum;
    for (int k = lane; k < T; k += 64) {
      const float pk = pr[k] * inv;
      if (p.probs) p.probs[row * T + k] = pk;
      pr[k] = pk * drop_mult(p.drop, drow, (unsigned)k);
    }
    __builtin_amdgcn_wave_barrier();
    if (p.lse && lane == 0) p.lse[row] = mx + logf(sum);
    if (p.ctx) {
      for (int d = lane; d < dh; d += 64) {
        float acc = 0.f;
        for (int k = 0; k < T; ++k) acc = fmaf(pr[k], vbase[(long)k * ld + d], acc);
        p.ctx[(b * T + q) * ldc + h * dh + d] = acc;
      }
    }
  } else {
    const float lse = p.lse[row];
    float dl = 0.f;
    for (int d = lane; d < dh; d += 64) dl = fmaf(dorow[d], p.ctx[(b * T + q) * ldc + h * dh + d], dl);
    dl = wave_sum(dl);
    if (lane == 0) p.delta[row] = dl;
    for (int k = lane; k < T; k += 64) {
      const float sc = dot_row(qrow, kbase + (long)k * ld, dh) * p.scale;
      const float pk = expf(sc - lse);
      const float dp = dot_row(dorow, vbase + (long)k * ld, dh);
      ds[k] = pk * (dp * drop_mult(p.drop, drow, (unsigned)k) - dl);
    }
    __builtin_amdgcn_wave_barrier();
    for (int d = lane; d < dh; d += 64) {
      float acc = 0.f;
      for (int k = 0; k < T; ++k) acc = fmaf(ds[k], kbase[(long)k * ld + d], acc);
      p.dqkv[(b * T + q) * ld + h * dh + d] = acc * p.scale;
    }
  }
}

// dK, dV: one wave per key row
__global__ __launch_bounds__(256) void attn32_dkv_kernel(Attn32Args p) {
  resolve_drop(p.drop);
  extern __shared__ __attribute__((aligned(16))) float sm32[];
  const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
  const long row = (long)blockIdx.x * 4 + wib;  // (b*H + h)*T + key
  if (row >= (long)p.B * p.H * p.T) return;
  const int T = p.T, dh = p.dh, H = p.H;
  const int key = (int)(row % T);
  const long bh = row / T;
  const int h = (int)(bh % H);
  const long b = bh / H;
  const long ld = 3L * H * dh, ldc = (long)H * dh;
  float* pd = sm32 + wib * (2 * p.Tp + 2 * 128);
  float* ds = pd + p.Tp;
  float* krow = ds + p.Tp;
  float* vrow = krow + 128;
  const float* qbase = p.qkv + b * T * ld + h * dh;
  const float* kp = qbase + (long)key * ld + H * dh;
  const float* dobase = p.dctx + b * T * ldc + h * dh;
  for (int d = lane; d < dh; d += 64) {
    krow[d] = kp[d];
    vrow[d] = kp[H * dh + d];
  }
  __builtin_amdgcn_wave_barrier();
  for (int q = lane; q < T; q += 64) {
    const float sc = dot_row(krow, qbase + (long)q * ld, dh) * p.scale;
    const float pk = expf(sc - p.lse[bh * T + q]);
    const float dp = dot_row(vrow, dobase + (long)q * ldc, dh);
    const float m = drop_mult(p.drop, (unsigned long long)(bh * T + q), (unsigned)key);
    pd[q] = pk * m;
    ds[q] = pk * (dp * m - p.delta[bh * T + q]);
  }
  __builtin_amdgcn_wave_barrier();
  for (int d = lane; d < dh; d += 64) {
    float av = 0.f, ak = 0.f;
    for (int q = 0; q < T; ++q) {
      av = fmaf(pd[q], dobase[(long)q * ldc + d], av);
      ak = fmaf(ds[q], qbase[(long)q * ld + d], ak);
    }
    float* o = p.dqkv + (b * T + key) * ld + H * dh + h * dh + d;
    o[0] = ak * p.scale;
    o[H * dh] = av;
  }
}

// ------------------------------------------------------------------------------------------------ fp32 attention on MFMA (r03)
// The one-wave-per-row kernels above are exact but slow: 258 of the 368 ms of a ViT-B step in precision '32' (r03 profile).
// gfx950 has f32-input matrix instructions (v_mfma_f32_16x16x4_f32: exact f32 products and f32 accumulation, bit for bit
// a k-ordered fmaf chain, at the f32 vector rate per instruction but 64 lanes x 16 results each), so the same flash-style
// tiling as the bf16 kernels runs on them: 4 waves x 16 rows, 64-row K / V (or Q / dO) tiles of f32 in the LDS, the swapped
// orientation that keeps the softmax statistics lane-local, and the accumulator tile of one product being the B operand of
// the next (a lane's register r IS the k-slot (lane >> 4) of MFMA step r: no lane movement).  head_dim 64 only (ViT-B / -L);
// other head sizes and the attention-map output stay on the kernels above.
// Operand maps of v_mfma_f32_16x16x4_f32: A[row = l & 15][k = l >> 4], B[k = l >> 4][col = l & 15] (one float per lane each),
// C / D as for every 16x16 MFMA.  The contraction over d (64) takes 16 steps; step s uses d = 16 g + s for lane group g, so a
// lane's 16 operand values are 64 CONTIGUOUS bytes of its row (4 x ds_read_b128).
// LDS tile [64 rows][64 f32]: row r at r * 256, 16-byte chunk c at ((c ^ sw(r)) << 4), sw(r) = (r & 3) | ((r & 8) ? 12 : 0):
// the row reads (a 16-lane group = 8 rows at chunk i of one lane group and 8 rows at chunk i + 4 of the next) tile the
// 256-byte bank row; the per-element reads of the third product are 2-way at worst, one per 32-cycle MFMA.
__device__ __forceinline__ int t32_off(int r, int c) { return r * 256 + ((c ^ ((r & 3) | ((r & 8) ? 12 : 0))) << 4); }
__device__ __forceinline__ void load_tile32(char* img, const float* g, long ld, int row0, int nrows, int tid) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int q = tid + 256 * i, r = q >> 4, c = q & 15;
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row0 + r < nrows) v = *(const f32x4*)(g + (long)(row0 + r) * ld + c * 4);
    *(f32x4*)(img + t32_off(r, c)) = v;
  }
}
// the 16 operand values of row (rb + l15) for the 16 contraction steps: d = 16 g + s
__device__ __forceinline__ void frag32_rows(float (&f)[16], const char* img, int rb, int l15, int lg) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const f32x4 v = *(const f32x4*)(img + t32_off(rb + l15, 4 * lg + i));
    f[4 * i] = v[0]; f[4 * i + 1] = v[1]; f[4 * i + 2] = v[2]; f[4 * i + 3] = v[3];
  }
}
__device__ __forceinline__ void load_own32(float (&f)[16], const float* g, long ld, int row, int nrows, int lg) {
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    if (row < nrows) v = *(const f32x4*)(g + (long)row * ld + 16 * lg + 4 * i);
    f[4 * i] = v[0]; f[4 * i + 1] = v[1]; f[4 * i + 2] = v[2]; f[4 * i + 3] = v[3];
  }
}
__device__ __forceinline__ float t32_elem(const char* img, int r, int col) {
  return *(const float*)(img + t32_off(r, col >> 2) + (col & 3) * 4);
}
#define MFMA32(a, b, c) __builtin_amdgcn_mfma_f32_16x16x4f32((a), (b), (c), 0, 0, 0)

__global__ __launch_bounds__(256) void attn32m_fwd_kernel(Attn32Args p) {
  resolve_drop(p.drop);
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * 256];
  char* Kimg = smem;
  char* Vimg = smem + 64 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T;
  const long ld = 3L * p.H * 64, ldc = (long)p.H * 64;
  const float* qb = p.qkv + (long)b * T * ld + h * 64;
  const float* kb_ = qb + p.H * 64;
  const float* vb = kb_ + p.H * 64;
  const int q0 = (blockIdx.x * 4 + wave) * 16, q = q0 + l15;
  float qf[16];
  load_own32(qf, qb, ld, q, T, lg);
  const float c = p.scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x4 ot[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) ot[i] = zero4();
  const unsigned long long drow = (unsigned long long)bh * T + q;
  for (int kb = 0; kb < T; kb += 64) {
    if (kb) __syncthreads();
    load_tile32(Kimg, kb_, ld, kb, T, tid);
    load_tile32(Vimg, vb, ld, kb, T, tid);
    __syncthreads();
    f32x4 st[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (kb + j * 16 < T) {
        float kf[16];
        frag32_rows(kf, Kimg, j * 16, l15, lg);
        f32x4 a = zero4();
#pragma unroll
        for (int s = 0; s < 16; ++s) a = MFMA32(kf[s], qf[s], a);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          a[r] = (kb + j * 16 + lg * 4 + r < T) ? a[r] * c : -INFINITY;
          mx = fmaxf(mx, a[r]);
        }
        st[j] = a;
      } else {
        st[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
    }
    mx = grp4_max(mx);
    const float mn = fmaxf(m, mx);
    const float alpha = exp2f(m - mn);
    m = mn;
    float ls = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        st[j][r] = exp2f(st[j][r] - mn);
        ls += st[j][r];
      }
    l = l * alpha + ls;
#pragma unroll
    for (int i = 0; i < 4; ++i) ot[i] *= alpha;
    if (p.drop.thr) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const unsigned key = kb + j * 16 + lg * 4;
        float k0, k1, k2, k3;
        drop_pair(p.drop, drow, key, k0, k1);
        drop_pair(p.drop, drow, key + 2, k2, k3);
        st[j][0] *= k0; st[j][1] *= k1; st[j][2] *= k2; st[j][3] *= k3;
      }
    }
    // O^T[d][q] += sum over keys V^T[d][key] P^T[key][q]: MFMA step (j, r) has k-slot g = key 16 j + 4 g + r, whose
    // probability is this lane's register st[j][r]; the A operand is V[that key][dt * 16 + l15]
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (kb + j * 16 < T) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int kr = j * 16 + lg * 4 + r;
#pragma unroll
          for (int dt = 0; dt < 4; ++dt) ot[dt] = MFMA32(t32_elem(Vimg, kr, dt * 16 + l15), st[j][r], ot[dt]);
        }
      }
    }
  }
  l = grp4_sum(l);
  if (q < T) {
    const float inv = 1.0f / l;
    float* o = p.ctx + ((long)b * T + q) * ldc + h * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *(f32x4*)(o + dt * 16 + lg * 4) = ot[dt] * inv;
    if (lg == 0 && p.lse) p.lse[(long)bh * T + q] = (m + log2f(l)) * LN2;
  }
}

__global__ __launch_bounds__(256) void attn32m_dq_kernel(Attn32Args p) {
  resolve_drop(p.drop);
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * 256];
  char* Kimg = smem;
  char* Vimg = smem + 64 * 256;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T;
  const long ld = 3L * p.H * 64, ldc = (long)p.H * 64;
  const float* qb = p.qkv + (long)b * T * ld + h * 64;
  const float* kb_ = qb + p.H * 64;
  const float* vb = kb_ + p.H * 64;
  const float* dob = p.dctx + (long)b * T * ldc + h * 64;
  const float* ob = p.ctx + (long)b * T * ldc + h * 64;
  const int q0 = (blockIdx.x * 4 + wave) * 16, q = q0 + l15;
  float qf[16], dof[16];
  load_own32(qf, qb, ld, q, T, lg);
  load_own32(dof, dob, ldc, q, T, lg);
  const float c = p.scale * LOG2E;
  const float lse2 = q < T ? p.lse[(long)bh * T + q] * LOG2E : INFINITY;
  float del = 0.f;  // delta[q] = rowsum(dO o O): this lane's 16 columns, then the 4 lane groups
  {
    float of[16];
    load_own32(of, ob, ldc, q, T, lg);
#pragma unroll
    for (int s = 0; s < 16; ++s) del = fmaf(of[s], dof[s], del);
    del = grp4_sum(del);
    if (q < T && lg == 0) p.delta[(long)bh * T + q] = del;
  }
  f32x4 dqt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dqt[i] = zero4();
  const unsigned long long drow = (unsigned long long)bh * T + q;
  for (int kb = 0; kb < T; kb += 64) {
    if (kb) __syncthreads();
    load_tile32(Kimg, kb_, ld, kb, T, tid);
    load_tile32(Vimg, vb, ld, kb, T, tid);
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (kb + j * 16 >= T) continue;
      float kf[16], vf[16];
      frag32_rows(kf, Kimg, j * 16, l15, lg);
      frag32_rows(vf, Vimg, j * 16, l15, lg);
      f32x4 s_ = zero4(), dp = zero4();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        s_ = MFMA32(kf[s], qf[s], s_);
        dp = MFMA32(vf[s], dof[s], dp);
      }
      const unsigned key0 = kb + j * 16 + lg * 4;
      float k[4] = {1.f, 1.f, 1.f, 1.f};
      if (p.drop.thr) {
        drop_pair(p.drop, drow, key0, k[0], k[1]);
        drop_pair(p.drop, drow, key0 + 2, k[2], k[3]);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = ((int)key0 + r < T) ? exp2f(s_[r] * c - lse2) : 0.f;
        const float ds = pr * (dp[r] * k[r] - del);
        const int kr = j * 16 + lg * 4 + r;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) dqt[dt] = MFMA32(t32_elem(Kimg, kr, dt * 16 + l15), ds, dqt[dt]);
      }
    }
  }
  if (q < T) {
    float* o = p.dqkv + ((long)b * T + q) * ld + h * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) *(f32x4*)(o + dt * 16 + lg * 4) = dqt[dt] * p.scale;
  }
}

__global__ __launch_bounds__(256) void attn32m_dkv_kernel(Attn32Args p) {
  resolve_drop(p.drop);
  __shared__ __attribute__((aligned(16))) char smem[2 * 64 * 256 + 2 * 64 * 4];
  char* Qimg = smem;
  char* Oimg = smem + 64 * 256;
  float* lse_s = (float*)(smem + 2 * 64 * 256);
  float* del_s = lse_s + 64;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T;
  const long ld = 3L * p.H * 64, ldc = (long)p.H * 64;
  const float* qb = p.qkv + (long)b * T * ld + h * 64;
  const float* kb_ = qb + p.H * 64;
  const float* vb = kb_ + p.H * 64;
  const float* dob = p.dctx + (long)b * T * ldc + h * 64;
  const int key = (blockIdx.x * 4 + wave) * 16 + l15;
  float kf[16], vf[16];
  load_own32(kf, kb_, ld, key, T, lg);
  load_own32(vf, vb, ld, key, T, lg);
  const float c = p.scale * LOG2E;
  f32x4 dkt[4], dvt[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) dkt[i] = dvt[i] = zero4();
  for (int qb0 = 0; qb0 < T; qb0 += 64) {
    if (qb0) __syncthreads();
    load_tile32(Qimg, qb, ld, qb0, T, tid);
    load_tile32(Oimg, dob, ldc, qb0, T, tid);
    if (tid < 64) {
      const int qq = qb0 + tid;
      lse_s[tid] = qq < T ? p.lse[(long)bh * T + qq] * LOG2E : INFINITY;
      del_s[tid] = qq < T ? p.delta[(long)bh * T + qq] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (qb0 + j * 16 >= T) continue;
      float qfr[16], ofr[16];
      frag32_rows(qfr, Qimg, j * 16, l15, lg);
      frag32_rows(ofr, Oimg, j * 16, l15, lg);
      f32x4 s_ = zero4(), dp = zero4();
#pragma unroll
      for (int s = 0; s < 16; ++s) {
        s_ = MFMA32(qfr[s], kf[s], s_);
        dp = MFMA32(ofr[s], vf[s], dp);
      }
      const f32x4 l4 = *(const f32x4*)(lse_s + j * 16 + lg * 4);
      const f32x4 d4 = *(const f32x4*)(del_s + j * 16 + lg * 4);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float pr = exp2f(s_[r] * c - l4[r]);  // rows past T carry lse = +inf -> 0
        float mk = 1.f;
        if (p.drop.thr) {
          const unsigned long long row = (unsigned long long)bh * T + (qb0 + j * 16 + lg * 4 + r);
          const unsigned hsh = drop_bits(drop_rowkey(p.drop, row), (unsigned)key >> 1);
          const unsigned r16 = (key & 1) ? (hsh >> 16) : (hsh & 0xFFFFu);
          mk = r16 >= p.drop.thr ? p.drop.scale : 0.f;
        }
        const float pd = pr * mk, ds = pr * (dp[r] * mk - d4[r]);
        const int qr = j * 16 + lg * 4 + r;
#pragma unroll
        for (int dt = 0; dt < 4; ++dt) {
          dvt[dt] = MFMA32(t32_elem(Oimg, qr, dt * 16 + l15), pd, dvt[dt]);
          dkt[dt] = MFMA32(t32_elem(Qimg, qr, dt * 16 + l15), ds, dkt[dt]);
        }
      }
    }
  }
  if (key < T) {
    float* ok = p.dqkv + ((long)b * T + key) * ld + p.H * 64 + h * 64;
    float* ov = ok + p.H * 64;
#pragma unroll
    for (int dt = 0; dt < 4; ++dt) {
      *(f32x4*)(ok + dt * 16 + lg * 4) = dkt[dt] * p.scale;
      *(f32x4*)(ov + dt * 16 + lg * 4) = dvt[dt];
    }
  }
}
#undef MFMA32

// which: 0 forward (+ optional attention maps), 1 dQ (+ delta), 2 dK/dV
static int launch_attn32(int which, Attn32Args& a, const AttnPlan& pl, hipStream_t st) {
  if (pl.form == ATTN_F32_MFMA) {  // head_dim 64, no attention-map output: the f32-MFMA kernels
    dim3 grid(cdiv(cdiv(a.T, 16), 4), a.B * a.H);
    if (which == 0) hipLaunchKernelGGL(attn32m_fwd_kernel, grid, dim3(256), 0, st, a);
    else if (which == 1) hipLaunchKernelGGL(attn32m_dq_kernel, grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL(attn32m_dkv_kernel, grid, dim3(256), 0, st, a);
    VIT_LAUNCH_CHECK();
    return VIT_OK;
  }
  a.Tp = (a.T + 63) & ~63;
  const size_t smem = (size_t)4 * (2 * a.Tp + 256) * sizeof(float);
  const long rows = (long)a.B * a.H * a.T;
  dim3 grid((unsigned)((rows + 3) / 4)), block(256);
  if (which == 0) return launch_lds160<attn32_row_kernel<0>>(grid, block, smem, st, a);
  if (which == 1) return launch_lds160<attn32_row_kernel<1>>(grid, block, smem, st, a);
  return launch_lds160<attn32_dkv_kernel>(grid, block, smem, st, a);
}

int launch_attn_f32(Attn32Args& a, const AttnPlan& pl, hipStream_t st) {
  VIT_CHECK(a.T <= 4096 && a.dh <= 128 && (a.dh % 4) == 0, VIT_ERR_UNSUPPORTED,
            "fp32 attention supports T <= 4096 and dh <= 128 (multiple of 4); got T=%d dh=%d", a.T, a.dh);
  if (!pl.bwd) return launch_attn32(0, a, pl, st);
  const int rc = launch_attn32(1, a, pl, st);
  if (rc != VIT_OK) return rc;
  return launch_attn32(2, a, pl, st);
}

}  // namespace vit
