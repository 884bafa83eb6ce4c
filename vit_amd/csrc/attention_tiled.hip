// Tiled attention kernels: 4 waves share 64-row K / V (or Q / dO) tiles staged in LDS, any sequence length and head_dim up
// to 128; and the eval-time attention-map kernel.  The shapes the LDS can hold whole take the resident kernels instead.
#include "attention.h"

namespace vit {

// ------------------------------------------------------------------------------------------------ forward
template <int DH>
__global__ __launch_bounds__(AW * 64) void attn_fwd_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  __shared__ __attribute__((aligned(16))) char smem[2 * RT * DH * 2];
  char* Kimg = smem;
  char* Vimg = smem + RT * DH * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T, dh = p.dh;
  const long ld = 3L * p.H * dh;
  const short* qb = p.qkv + (long)b * T * ld + h * dh;
  const short* kb_ = qb + p.H * dh;
  const short* vb = kb_ + p.H * dh;
  const int q0 = (blockIdx.x * AW + wave) * 16;

  bf16x8 qf[DH / 32];
  load_own<DH>(qf, qb, ld, q0, T, dh, l15, lg);
  const float c = p.scale * LOG2E;
  float m = -INFINITY, l = 0.f;
  f32x4 ot[DH / 16];
#pragma unroll
  for (int i = 0; i < DH / 16; ++i) ot[i] = zero4();
  const unsigned long long drow = (unsigned long long)bh * T + (q0 + l15);

  for (int kb = 0; kb < T; kb += RT) {
    if (kb) __syncthreads();
    load_tile<DH>(Kimg, kb_, ld, kb, T, dh, tid);
    load_tile<DH>(Vimg, vb, ld, kb, T, dh, tid);
    __syncthreads();
    f32x4 st[4];
    float mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (kb + j * 16 < T) {
        f32x4 a = zero4();
#pragma unroll
        for (int s = 0; s < DH / 32; ++s)
          a = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<DH>(Kimg, j * 16, s, l15, lg), qf[s], a, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int key = kb + j * 16 + lg * 4 + r;
          a[r] = key < T ? a[r] * c : -INFINITY;
          mx = fmaxf(mx, a[r]);
        }
        st[j] = a;
      } else {
        st[j] = (f32x4){-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      }
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
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
    for (int i = 0; i < DH / 16; ++i) ot[i] *= alpha;
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
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (kb + u * 32 < T) {
        const bf16x8 pf = pack8(st[2 * u], st[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DH / 16; ++dt)
          ot[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols<DH>(Vimg, u * 32, u * 32 + 16, dt * 16, l15, lg),
                                                           pf, ot[dt], 0, 0, 0);
      }
    }
  }
  l += __shfl_xor(l, 16, 64);
  l += __shfl_xor(l, 32, 64);
  const int q = q0 + l15;
  if (q < T) {
    const float inv = 1.0f / l;
    short* o = p.ctx + ((long)b * T + q) * (p.H * dh) + h * dh;
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      const int d = dt * 16 + lg * 4;
      if (d < dh) {
        const f32x4 v = ot[dt] * inv;
        u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)(o + d) = pk;
        if (p.ctx_lo) store_lo(p.ctx_lo + (o - p.ctx) + d, v, pk);
      }
    }
    if (lg == 0) p.lse[(long)bh * T + q] = (m + log2f(l)) * LN2;
  }
}

// ------------------------------------------------------------------------------------------------ dQ
template <int DH>
__global__ __launch_bounds__(AW * 64) void attn_bwd_dq_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  __shared__ __attribute__((aligned(16))) char smem[2 * RT * DH * 2];
  char* Kimg = smem;
  char* Vimg = smem + RT * DH * 2;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T, dh = p.dh;
  const long ld = 3L * p.H * dh, ldc = (long)p.H * dh;
  const short* qb = p.qkv + (long)b * T * ld + h * dh;
  const short* kb_ = qb + p.H * dh;
  const short* vb = kb_ + p.H * dh;
  const short* dob = p.dctx + (long)b * T * ldc + h * dh;
  const int q0 = (blockIdx.x * AW + wave) * 16;
  const int q = q0 + l15;

  bf16x8 qf[DH / 32], dof[DH / 32];
  load_own<DH>(qf, qb, ld, q0, T, dh, l15, lg);
  load_own<DH>(dof, dob, ldc, q0, T, dh, l15, lg);
  const float c = p.scale * LOG2E;
  const float lse2 = q < T ? p.lse[(long)bh * T + q] * LOG2E : INFINITY;
  // delta[q] = rowsum(dO * O): this lane holds 8 columns per 32-column step of its row; the 4 lane groups complete the
  // row with two xor-shuffles.  Written out for the dK/dV kernel that runs next on the stream.
  float del = 0.f;
  {
    const short* ob = p.ctx + (long)b * T * ldc + h * dh;
#pragma unroll
    for (int s = 0; s < DH / 32; ++s) {
      const int col = s * 32 + lg * 8;
      if (q < T && col < dh) {
        const bf16x8 o = __builtin_bit_cast(bf16x8, ld_head8(ob + (long)q * ldc, col, dh));
#pragma unroll
        for (int e = 0; e < 8; ++e) del += bf2f(o[e]) * bf2f(dof[s][e]);
        if (p.ctx_lo) {
          const bf16x8 ol = __builtin_bit_cast(bf16x8, ld_head8(p.ctx_lo + (ob - p.ctx) + (long)q * ldc, col, dh));
#pragma unroll
          for (int e = 0; e < 8; ++e) del += bf2f(ol[e]) * bf2f(dof[s][e]);
        }
      }
    }
    del += __shfl_xor(del, 16, 64);
    del += __shfl_xor(del, 32, 64);
    if (q < T && lg == 0) p.delta[(long)bh * T + q] = del;
  }
  f32x4 dqt[DH / 16];
#pragma unroll
  for (int i = 0; i < DH / 16; ++i) dqt[i] = zero4();
  const unsigned long long drow = (unsigned long long)bh * T + q;

  for (int kb = 0; kb < T; kb += RT) {
    if (kb) __syncthreads();
    load_tile<DH>(Kimg, kb_, ld, kb, T, dh, tid);
    load_tile<DH>(Vimg, vb, ld, kb, T, dh, tid);
    __syncthreads();
    f32x4 ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      ds[j] = zero4();
      if (kb + j * 16 < T) {
        f32x4 s_ = zero4(), dp = zero4();
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
          s_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<DH>(Kimg, j * 16, s, l15, lg), qf[s], s_, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<DH>(Vimg, j * 16, s, l15, lg), dof[s], dp, 0, 0, 0);
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
          ds[j][r] = pr * (dp[r] * k[r] - del);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (kb + u * 32 < T) {
        const bf16x8 df = pack8(ds[2 * u], ds[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DH / 16; ++dt)
          dqt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols<DH>(Kimg, u * 32, u * 32 + 16, dt * 16, l15, lg),
                                                            df, dqt[dt], 0, 0, 0);
      }
    }
  }
  if (q < T) {
    short* o = p.dqkv + ((long)b * T + q) * ld + h * dh;
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      const int d = dt * 16 + lg * 4;
      if (d < dh) {
        const f32x4 v = dqt[dt] * p.scale;
        u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)(o + d) = pk;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ dK, dV
template <int DH>
__global__ __launch_bounds__(AW * 64) void attn_bwd_dkv_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  __shared__ __attribute__((aligned(16))) char smem[2 * RT * DH * 2 + 2 * RT * 4];
  char* Qimg = smem;
  char* Oimg = smem + RT * DH * 2;
  float* lse_s = (float*)(smem + 2 * RT * DH * 2);
  float* del_s = lse_s + RT;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, l15 = lane & 15, lg = lane >> 4;
  const int bh = blockIdx.y, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T, dh = p.dh;
  const long ld = 3L * p.H * dh, ldc = (long)p.H * dh;
  const short* qb = p.qkv + (long)b * T * ld + h * dh;
  const short* kb_ = qb + p.H * dh;
  const short* vb = kb_ + p.H * dh;
  const short* dob = p.dctx + (long)b * T * ldc + h * dh;
  const int k0w = (blockIdx.x * AW + wave) * 16;
  const int key = k0w + l15;

  bf16x8 kf[DH / 32], vf[DH / 32];
  load_own<DH>(kf, kb_, ld, k0w, T, dh, l15, lg);
  load_own<DH>(vf, vb, ld, k0w, T, dh, l15, lg);
  const float c = p.scale * LOG2E;
  f32x4 dkt[DH / 16], dvt[DH / 16];
#pragma unroll
  for (int i = 0; i < DH / 16; ++i) dkt[i] = dvt[i] = zero4();

  for (int qb0 = 0; qb0 < T; qb0 += RT) {
    if (qb0) __syncthreads();
    load_tile<DH>(Qimg, qb, ld, qb0, T, dh, tid);
    load_tile<DH>(Oimg, dob, ldc, qb0, T, dh, tid);
    if (tid < RT) {
      const int qq = qb0 + tid;
      lse_s[tid] = qq < T ? p.lse[(long)bh * T + qq] * LOG2E : INFINITY;
      del_s[tid] = qq < T ? p.delta[(long)bh * T + qq] : 0.f;
    }
    __syncthreads();
    f32x4 pd[4], ds[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      pd[j] = ds[j] = zero4();
      if (qb0 + j * 16 < T) {
        f32x4 s_ = zero4(), dp = zero4();
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
          s_ = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<DH>(Qimg, j * 16, s, l15, lg), kf[s], s_, 0, 0, 0);
          dp = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_rows<DH>(Oimg, j * 16, s, l15, lg), vf[s], dp, 0, 0, 0);
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
          pd[j][r] = pr * mk;
          ds[j][r] = pr * (dp[r] * mk - d4[r]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (qb0 + u * 32 < T) {
        const bf16x8 pf = pack8(pd[2 * u], pd[2 * u + 1]);
        const bf16x8 df = pack8(ds[2 * u], ds[2 * u + 1]);
#pragma unroll
        for (int dt = 0; dt < DH / 16; ++dt) {
          dvt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols<DH>(Oimg, u * 32, u * 32 + 16, dt * 16, l15, lg),
                                                            pf, dvt[dt], 0, 0, 0);
          dkt[dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(frag_cols<DH>(Qimg, u * 32, u * 32 + 16, dt * 16, l15, lg),
                                                            df, dkt[dt], 0, 0, 0);
        }
      }
    }
  }
  if (key < T) {
    short* ok = p.dqkv + ((long)b * T + key) * ld + p.H * dh + h * dh;
    short* ov = ok + p.H * dh;
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      const int d = dt * 16 + lg * 4;
      if (d < dh) {
        const f32x4 a = dkt[dt] * p.scale, v = dvt[dt];
        u32x2 pk = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3])};
        u32x2 pv = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)(ok + d) = pk;
        *(u32x2*)(ov + d) = pv;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ probabilities
// eval-time attention maps [B,H,T,T] f32 (output_attentions=True, consumed by the reference's viz callbacks);
// a plain VALU kernel off the training path: one wave per (b, h, q) row.
__global__ __launch_bounds__(256) void attn_probs_kernel(const short* __restrict__ qkv, float* __restrict__ probs, int B,
                                                         int H, int T, int dh, float scale) {
  const int lane = threadIdx.x & 63;
  const long row = ((long)blockIdx.x * blockDim.x + threadIdx.x) >> 6;  // (b*H + h)*T + q
  if (row >= (long)B * H * T) return;
  const int q = (int)(row % T);
  const long bh = row / T;
  const int h = (int)(bh % H);
  const long b = bh / H;
  const long ld = 3L * H * dh;
  const short* qp = qkv + (b * T + q) * ld + h * dh;
  const short* kp = qkv + b * T * ld + H * dh + h * dh;
  float* out = probs + row * T;
  float mx = -INFINITY;
  for (int k = lane; k < T; k += 64) {
    float s = 0.f;
    for (int d = 0; d < dh; d += 8) {
      const bf16x8 x = __builtin_bit_cast(bf16x8, ld_head8(qp, d, dh)), y = __builtin_bit_cast(bf16x8, ld_head8(kp + (long)k * ld, d, dh));
#pragma unroll
      for (int e = 0; e < 8; ++e) s += bf2f(x[e]) * bf2f(y[e]);
    }
    s *= scale;
    out[k] = s;
    mx = fmaxf(mx, s);
  }
  mx = wave_max(mx);
  float sum = 0.f;
  for (int k = lane; k < T; k += 64) {
    const float e = __expf(out[k] - mx);
    out[k] = e;
    sum += e;
  }
  sum = wave_sum(sum);
  const float inv = 1.f / sum;
  for (int k = lane; k < T; k += 64) out[k] *= inv;
}

#define DISPATCH_DH(KERNEL, grid, st, a)                                                         \
  do {                                                                                           \
    if (pl.dhp == 32) hipLaunchKernelGGL((KERNEL<32>), grid, dim3(AW * 64), 0, st, a);            \
    else if (pl.dhp == 64) hipLaunchKernelGGL((KERNEL<64>), grid, dim3(AW * 64), 0, st, a);       \
    else hipLaunchKernelGGL((KERNEL<128>), grid, dim3(AW * 64), 0, st, a);                        \
  } while (0)

int launch_attn_tiled(const AttnArgs& a, const AttnPlan& pl, hipStream_t st) {
  dim3 grid(cdiv(cdiv(a.T, 16), AW), a.B * a.H);
  if (pl.bwd) {
    DISPATCH_DH(attn_bwd_dq_kernel, grid, st, a);
    VIT_LAUNCH_CHECK();
    DISPATCH_DH(attn_bwd_dkv_kernel, grid, st, a);
  } else {
    DISPATCH_DH(attn_fwd_kernel, grid, st, a);
  }
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int launch_attn_probs(const short* qkv, float* probs, int B, int H, int T, int dh, float scale, hipStream_t st) {
  const long rows = (long)B * H * T;
  hipLaunchKernelGGL(attn_probs_kernel, dim3((int)((rows + 3) / 4)), dim3(256), 0, st, qkv, probs, B, H, T, dh, scale);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

}  // namespace vit
