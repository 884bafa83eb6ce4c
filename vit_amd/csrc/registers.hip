// Register tokens for gfx950 (include/vit_amd_registers.h): the embedding finish over [CLS, R registers, N patches] and its
// backward -- embed_finish_kernel / embed_finish_masked_kernel of elementwise.hip / mim.hip and their backwards with R rows in
// between: same walk, same selects, same sums, so R = 0 stores their bits.  One forward and one backward kernel; the mask is
// optional (NULL: the plain model) and only ever compared with zero, never turned into an address.
// Vectorised (8-16 B per lane), free of float atomics.
#include <algorithm>

#include "common.h"

namespace vit {

// token t of a sample: 0 = CLS, 1 .. R = registers, 1 + R + n = patch n.  n = t - 1 - R is negative in front of the patches.
// I: the type of the element index -- unsigned where B * T * D / 4 stays below 2^30 (its divisions are a fraction of the 64-bit
// ones' instructions, and this kernel runs from the Infinity Cache at ViT-B, where they show), long beyond.
template <typename I>
__global__ void embed_finish_reg_kernel(float* __restrict__ tok, const float* __restrict__ cls, const float* __restrict__ reg,
                                        const float* __restrict__ pos, const int* __restrict__ mask,
                                        const float* __restrict__ mtok, int B, int R, int N, int D, DropCfg drop) {
  resolve_drop(drop);
  const int dv = D >> 2, T = 1 + R + N;
  const I total = (I)B * T * dv;
  for (I i = blockIdx.x * (I)blockDim.x + threadIdx.x; i < total; i += (I)gridDim.x * blockDim.x) {
    const int d = (int)(i % (I)dv) << 2;
    const I row = i / (I)dv;  // b*T + t
    const int t = (int)(row % (I)T);
    const long b = (long)(row / (I)T);
    const int n = t - 1 - R;
    float* p = tok + (long)row * D + d;
    f32x4 v;
    if (t == 0)
      v = *(const f32x4*)(cls + d);
    else if (n < 0)
      v = *(const f32x4*)(reg + (long)(t - 1) * D + d);
    else if (mask && mask[b * N + n] != 0)
      v = *(const f32x4*)(mtok + d);
    else
      v = *(const f32x4*)p;
    // position row 0 for CLS, 1 + n for patch n, none for a register
    if (pos && (t == 0 || n >= 0)) v += *(const f32x4*)(pos + (long)(n + 1 > 0 ? n + 1 : 0) * D + d);
    if (drop.thr) {
      float k0, k1, k2, k3;
      drop_pair(drop, (unsigned long long)row, (unsigned)d, k0, k1);
      drop_pair(drop, (unsigned long long)row, (unsigned)d + 2, k2, k3);
      v[0] *= k0; v[1] *= k1; v[2] *= k2; v[3] *= k3;
    }
    *(f32x4*)p = v;
  }
}

// embed_finish_bwd_kernel: one thread per (t, 4 columns) walks its batch chunk in ascending b.  The chunk's sum of token t goes
// to partial row `slot` = 0 (CLS), 1 + n (patch n), 1 + N + r (register r): the rows dpos takes are contiguous, and with R = 0
// the slot is t, the plain kernels' layout.  With a mask, macc takes the masked rows' terms alone (those rows store a zero
// dpatch) and goes to the second plane.
template <int OUT_BF16>
__global__ void embed_finish_reg_bwd_kernel(const float* __restrict__ dtok, const int* __restrict__ mask, void* __restrict__ dpatch,
                                            float* __restrict__ part, float* __restrict__ mpart, int B, int R, int N, int D,
                                            DropCfg drop, int bchunk) {
  resolve_drop(drop);
  const int dv = D >> 2, T = 1 + R + N;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= T * dv) return;
  const int d = (i % dv) << 2;
  const int t = i / dv;
  const int n = t - 1 - R;
  const int slot = t == 0 ? 0 : (n >= 0 ? 1 + n : N + t);
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
    if (n >= 0) {
      if (mask && mask[(long)b * N + n] != 0) {
        macc += v;
        v = (f32x4){0.f, 0.f, 0.f, 0.f};
      }
      if (OUT_BF16) {
        u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
        *(u32x2*)((short*)dpatch + ((long)b * N + n) * D + d) = pk;
      } else {
        *(f32x4*)((float*)dpatch + ((long)b * N + n) * D + d) = v;
      }
    }
  }
  *(f32x4*)(part + ((long)blockIdx.y * T + slot) * D + d) = acc;
  if (mask) *(f32x4*)(mpart + ((long)blockIdx.y * T + slot) * D + d) = macc;
}

static int reg_args_ok(const char* who, int B, int R, int N, int D, float dropout_p) {
  VIT_CHECK(B > 0 && N > 0 && D > 0 && R >= 0 && (D % 4) == 0, VIT_ERR_ARG, "%s: B=%d R=%d N=%d D=%d (D must be a multiple of 4)",
            who, B, R, N, D);
  VIT_CHECK((long)(1 + R + N) * (D / 4) < (1L << 31), VIT_ERR_ARG, "%s: R=%d N=%d D=%d: a sample's tokens exceed 2^31 vectors", who, R,
            N, D);
  VIT_CHECK(dropout_p >= 0.f && dropout_p < 1.f, VIT_ERR_ARG, "%s: dropout_p out of [0,1)", who);
  return VIT_OK;
}

}  // namespace vit

extern "C" {
using namespace vit;

int vit_embed_finish_reg(vit_handle h, float* tokens, const float* cls, const float* reg, const float* pos, const int32_t* mask,
                         const float* mask_token, int B, int R, int N, int D, float dropout_p, uint64_t seed, uint64_t site,
                         vit_stream stream) {
  VIT_CHECK(tokens && cls && (reg || R <= 0), VIT_ERR_ARG, "vit_embed_finish_reg: null pointer");
  VIT_CHECK((mask != nullptr) == (mask_token != nullptr), VIT_ERR_ARG, "vit_embed_finish_reg: mask and mask_token go together");
  const int rc = reg_args_ok("vit_embed_finish_reg", B, R, N, D, dropout_p);
  if (rc != VIT_OK) return rc;
  const long total = (long)B * (1 + R + N) * (D / 4);
  const DropCfg drop = make_drop_h(h, dropout_p, seed, site);
  // the stride is at most 4096 * 256 = 2^20 elements: below 2^30 elements i + stride cannot wrap in the narrow form
  if (total < (1L << 30))
    hipLaunchKernelGGL(embed_finish_reg_kernel<unsigned>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, tokens, cls, reg,
                       pos, mask, mask_token, B, R, N, D, drop);
  else
    hipLaunchKernelGGL(embed_finish_reg_kernel<long>, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, tokens, cls, reg, pos,
                       mask, mask_token, B, R, N, D, drop);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

int vit_embed_finish_reg_bwd(vit_handle h, const float* dtokens, const int32_t* mask, void* dpatch_out, int dpatch_dtype,
                             float* dcls, float* dreg, float* dpos, float* dmask_token, int B, int R, int N, int D,
                             float dropout_p, uint64_t seed, uint64_t site, int accumulate, vit_stream stream) {
  VIT_CHECK(dtokens && dpatch_out && dcls && (dreg || R <= 0), VIT_ERR_ARG, "vit_embed_finish_reg_bwd: null pointer");
  VIT_CHECK((mask != nullptr) == (dmask_token != nullptr), VIT_ERR_ARG,
            "vit_embed_finish_reg_bwd: mask and dmask_token go together");
  const int rc = reg_args_ok("vit_embed_finish_reg_bwd", B, R, N, D, dropout_p);
  if (rc != VIT_OK) return rc;
  VIT_CHECK(dpatch_dtype == VIT_BF16 || dpatch_dtype == VIT_F32, VIT_ERR_ARG, "vit_embed_finish_reg_bwd: bad dtype");
  const int T = 1 + R + N;
  const int nchunk = std::min(B, 16), bchunk = cdiv(B, nchunk), ny = cdiv(B, bchunk);  // vit_embed_finish_bwd's chunks
  const size_t plane = (size_t)ny * T * D;
  float* part = (float*)ctx_claim(h, (mask ? 2 : 1) * plane * sizeof(float), "vit_embed_finish_reg_bwd");
  if (!part) return VIT_ERR_WORKSPACE;
  float* mpart = part + plane;  // read and written with a mask only
  hipStream_t st = (hipStream_t)stream;
  accumulate = accumulate || ctx_grad_accumulate(h);
  const dim3 grid(cdiv((long)T * (D / 4), 256), ny);
  const DropCfg drop = make_drop_h(h, dropout_p, seed, site);
  if (dpatch_dtype == VIT_BF16)
    hipLaunchKernelGGL(embed_finish_reg_bwd_kernel<1>, grid, dim3(256), 0, st, dtokens, mask, dpatch_out, part, mpart, B, R, N, D,
                       drop, bchunk);
  else
    hipLaunchKernelGGL(embed_finish_reg_bwd_kernel<0>, grid, dim3(256), 0, st, dtokens, mask, dpatch_out, part, mpart, B, R, N, D,
                       drop, bchunk);
  VIT_LAUNCH_CHECK();
  // partial row of a chunk: [CLS | patches 0 .. N-1 | registers 0 .. R-1].  dcls = the sums of row 0; dpos = of rows 0 .. N;
  // dreg = of rows 1 + N ..; dmask_token = the sum of all ny * T rows of the second plane, in row order.  dpos and dreg share
  // one launch over the whole row (columns behind (1 + N) * D go to dreg): a column's sum does not depend on its neighbours,
  // and with R = 0 it is vit_embed_finish_bwd's call
  const int PD = (1 + N) * D;
  int rc2 = launch_reduce_partials(part, ny, D, dcls, D, dcls, accumulate, st, T * D);
  if (rc2 == VIT_OK && dpos) rc2 = launch_reduce_partials(part, ny, T * D, dpos, PD, dreg, accumulate, st, T * D);
  if (rc2 == VIT_OK && !dpos && R > 0) rc2 = launch_reduce_partials(part + PD, ny, R * D, dreg, R * D, dreg, accumulate, st, T * D);
  if (rc2 != VIT_OK || !mask) return rc2;
  return launch_reduce_partials(mpart, ny * T, D, dmask_token, D, dmask_token, accumulate, st, D);
}

}  // extern "C"
