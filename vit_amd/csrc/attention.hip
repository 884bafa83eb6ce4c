// Attention entry points of include/vit_amd.h: the launch plan and the three extern "C" functions.  Host code only; kernels
// and their launchers live one family per file (attention_tiled / _resident / _pipe / _f32.hip; shared pieces: attention.h).
#include "attention.h"

namespace vit {

// vit_set_option("attn_bwd_fused"): 0 = two-kernel backward everywhere; non-zero (default 4; 1 .. 3 named forms that no longer
// exist and mean the same) = the pair-pipelined single kernel where it fits (dh 64, 64 <= T <= 208), the two-kernel path elsewhere
int g_attn_bwd_fused = 4;
int g_attn_split = 2;  // vit_set_option("attn_split"): workgroups per (batch, head) in the resident kernels

// The one place that decides what an attention call launches: form, geometry, LDS bytes, template instantiation and the
// partial column-sum rows a backward leaves.  ctx_lo: the residual is passed; probs: the f32 forward also writes attention maps.
static AttnPlan attn_plan(vit_handle h, int io_dtype, bool bwd, int B, int H, int T, int dh, bool ctx_lo, bool probs) {
  AttnPlan pl = {};
  pl.bwd = bwd;
  if (io_dtype == VIT_F32) {  // head_dim 64, no attention-map output: the f32-MFMA kernels; else one wave per row
    pl.form = (dh == 64 && !probs) ? ATTN_F32_MFMA : ATTN_F32_ROW;
    return pl;
  }
  if (bwd && g_attn_bwd_fused && pipe_fits(T, dh)) {
    pl.form = ATTN_PIPE;
    pl.dhp = 64;
    pl.full7 = T > 192;
    pl.vitb = pl.full7 && H == 12 && ctx_lo;
    pl.grid = (unsigned)std::min(B * H, ctx_num_cus(h));
    pl.smem = pipe_smem(T);
    pl.csum_rows = B * 8;  // per batch: one per wave of the pipelined kernel
    return pl;
  }
  if (res_fits(T, dh)) {
    pl.form = ATTN_RESIDENT;
    pl.dhp = dh <= 32 ? 32 : 64;
    pl.dma = dh == 64;
    res_geometry(T, bwd, &pl.nsplit, &pl.wpw);
    pl.vitb = !bwd && pl.dma && T > 192 && T <= 208 && H == 12 && pl.nsplit == 2 && pl.wpw == 4;
    pl.grid = (unsigned)(B * H * pl.nsplit);
    pl.smem = res_smem(T, pl.dhp, false);
    if (bwd) {
      pl.smem_dkv = res_smem(T, pl.dhp, true);
      pl.csum_rows = B * pl.nsplit * pl.wpw;  // one per wave
    }
    return pl;
  }
  pl.form = ATTN_TILED;
  pl.dhp = dh <= 32 ? 32 : (dh <= 64 ? 64 : 128);
  return pl;
}

static int check_attn(const char* fn, int B, int H, int T, int dh, float p) {
  VIT_CHECK(B > 0 && H > 0 && T > 0 && dh > 0, VIT_ERR_ARG, "%s: B=%d H=%d T=%d dh=%d", fn, B, H, T, dh);
  VIT_CHECK((dh % 4) == 0 && dh <= 128, VIT_ERR_UNSUPPORTED, "%s: head dim %d (need a multiple of 4, <= 128)", fn, dh);
  VIT_CHECK(p >= 0.f && p < 1.f, VIT_ERR_ARG, "%s: dropout_p out of [0,1)", fn);
  return VIT_OK;
}

}  // namespace vit

extern "C" {
using namespace vit;

int vit_attention_fwd(vit_handle h, const void* qkv, void* ctx, void* ctx_lo, float* lse, int io_dtype, int B, int H, int T,
                      int dh, float scale, float dropout_p, uint64_t seed, uint64_t site, vit_stream stream) {
  VIT_CHECK(qkv && ctx && lse, VIT_ERR_ARG, "vit_attention_fwd: null pointer");
  int rc = check_attn("vit_attention_fwd", B, H, T, dh, dropout_p);
  if (rc != VIT_OK) return rc;
  const AttnPlan pl = attn_plan(h, io_dtype, false, B, H, T, dh, ctx_lo != nullptr, false);
  hipStream_t st = (hipStream_t)stream;
  if (io_dtype == VIT_F32) {
    Attn32Args a32 = {};
    a32.qkv = (const float*)qkv; a32.ctx = (float*)ctx; a32.lse = lse;
    a32.B = B; a32.H = H; a32.T = T; a32.dh = dh; a32.scale = scale;
    a32.drop = make_drop_h(h, dropout_p, seed, site);
    return launch_attn_f32(a32, pl, st);
  }
  AttnArgs a = {};
  a.qkv = (const short*)qkv; a.ctx = (short*)ctx; a.ctx_lo = (short*)ctx_lo; a.lse = lse;
  a.B = B; a.H = H; a.T = T; a.dh = dh; a.scale = scale;
  a.drop = make_drop_h(h, dropout_p, seed, site);
  return pl.form == ATTN_RESIDENT ? launch_attn_resident(a, pl, st) : launch_attn_tiled(a, pl, st);
}

int vit_attention_bwd(vit_handle h, const void* qkv, const void* ctx, const void* ctx_lo, const void* dctx, const float* lse,
                      float* delta, void* dqkv, int io_dtype, int B, int H, int T, int dh, float scale, float dropout_p,
                      uint64_t seed, uint64_t site, float* dqkv_colsum, vit_stream stream) {
  VIT_CHECK(qkv && ctx && dctx && lse && delta && dqkv, VIT_ERR_ARG, "vit_attention_bwd: null pointer");
  int rc = check_attn("vit_attention_bwd", B, H, T, dh, dropout_p);
  if (rc != VIT_OK) return rc;
  const AttnPlan pl = attn_plan(h, io_dtype, true, B, H, T, dh, ctx_lo != nullptr, false);
  hipStream_t st = (hipStream_t)stream;
  const int D3 = 3 * H * dh;
  // column sums: the resident and pipelined kernels leave one partial row per wave (the sums as stored), the f32 and tiled
  // forms run vit_colsum over the stored dqkv -- either way through the workspace, claimed before anything is launched
  float* part = nullptr;
  if (dqkv_colsum) {
    part = (float*)ctx_claim(h, pl.csum_rows ? (size_t)pl.csum_rows * D3 * sizeof(float) : colsum_ws_bytes(B * T, D3),
                             "vit_attention_bwd");
    if (!part) return VIT_ERR_WORKSPACE;
  }
  if (io_dtype == VIT_F32) {
    Attn32Args a32 = {};
    a32.qkv = (const float*)qkv; a32.ctx = (float*)const_cast<void*>(ctx); a32.lse = const_cast<float*>(lse);
    a32.dctx = (const float*)dctx; a32.delta = delta; a32.dqkv = (float*)dqkv;
    a32.B = B; a32.H = H; a32.T = T; a32.dh = dh; a32.scale = scale;
    a32.drop = make_drop_h(h, dropout_p, seed, site);
    rc = launch_attn_f32(a32, pl, st);
  } else {
    AttnArgs a = {};
    a.qkv = (const short*)qkv; a.lse = const_cast<float*>(lse); a.ctx = (short*)const_cast<void*>(ctx);
    a.ctx_lo = (short*)const_cast<void*>(ctx_lo);
    a.dctx = (const short*)dctx; a.delta = delta; a.dqkv = (short*)dqkv;
    a.B = B; a.H = H; a.T = T; a.dh = dh; a.scale = scale;
    a.drop = make_drop_h(h, dropout_p, seed, site);
    if (pl.csum_rows) a.csum_part = part;
    rc = pl.form == ATTN_PIPE ? launch_attn_pipe(a, pl, st)
         : pl.form == ATTN_RESIDENT ? launch_attn_resident(a, pl, st) : launch_attn_tiled(a, pl, st);
    if (rc == VIT_OK && a.csum_part)
      return launch_reduce_partials(a.csum_part, pl.csum_rows, D3, dqkv_colsum, D3, dqkv_colsum, ctx_grad_accumulate(h), st);
  }
  // no kernel partials (f32, tiled form): column sums over the stored dqkv
  if (rc != VIT_OK || !dqkv_colsum) return rc;
  return vit_colsum(h, dqkv, io_dtype, D3, dqkv_colsum, B * T, D3, ctx_grad_accumulate(h), stream);
}

int vit_attention_probs(vit_handle h, const void* qkv, float* probs, int io_dtype, int B, int H, int T, int dh,
                        float scale, vit_stream stream) {
  VIT_CHECK(qkv && probs, VIT_ERR_ARG, "vit_attention_probs: null pointer");
  int rc = check_attn("vit_attention_probs", B, H, T, dh, 0.f);
  if (rc != VIT_OK) return rc;
  if (io_dtype == VIT_F32) {
    Attn32Args a32 = {};
    a32.qkv = (const float*)qkv; a32.probs = probs;
    a32.B = B; a32.H = H; a32.T = T; a32.dh = dh; a32.scale = scale;
    a32.drop = make_drop(0.f, 0, 0);
    return launch_attn_f32(a32, attn_plan(h, io_dtype, false, B, H, T, dh, false, true), (hipStream_t)stream);
  }
  return launch_attn_probs((const short*)qkv, probs, B, H, T, dh, scale, (hipStream_t)stream);
}

}  // extern "C"
