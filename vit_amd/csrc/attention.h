// Internal header of the attention sources: what the kernel families share.
// Fused softmax attention (forward + backward) for gfx950, flash-style: scores / probabilities never reach HBM.
//
// Reads Q, K, V straight out of the fused QKV projection's output [B*T, 3*H*dh] (token-major, head h at columns
// h*dh of each third) and writes the merged-head context [B*T, H*dh], so no head split / merge copies exist.
//
// One wave owns 16 query rows (forward, dQ) or 16 keys (dK/dV); 4 waves share the 64-row K/V (or Q/dO) tiles staged
// in LDS.  All MFMAs (v_mfma_f32_16x16x32_bf16) are issued "swapped" so the 16 owned rows sit on lane&15:
//     S^T = K * Q^T,   O^T = V^T * P^T,   dP^T = V * dO^T,   dQ^T = K^T * dS^T          (owner = query)
//     S   = Q * K^T,   dP  = dO * V^T,    dV^T = dO^T * P,   dK^T = Q^T * dS            (owner = key)
// With that orientation (a) the softmax statistics m, l, lse, delta of a row live in the lane that owns the row
// (only the 4 lane groups lane>>4 have to be combined: two xor-shuffles), (b) the P / dS accumulator tile is already
// the B operand of the next MFMA (4 consecutive reduction indices per 16-tile per lane: k-slot j<4 -> tile 2u,
// j>=4 -> tile 2u+1), and (c) the other operand of that product is a transposed read of the row-major LDS tile
// (ds_read_b64_tr_b16) with the same slot order.  No P round trip through LDS, no permutes.
//
// LDS tile image: [64 rows][DH] bf16, 16-byte chunk c of row r at r*2*DH + ((c ^ swz(r)) << 4); row fragments by
// ds_read_b128, transposed fragments by ds_read_b64_tr_b16 inside the chunks.
#pragma once
#include <algorithm>
#include <math.h>

#include <type_traits>
#include "common.h"

namespace vit {

constexpr int AW = 4;    // waves per workgroup
constexpr int RT = 64;   // rows per LDS tile
constexpr float LOG2E = 1.4426950408889634f;
constexpr float LN2 = 0.6931471805599453f;

struct AttnArgs {
  const short* qkv; short* ctx; float* lse;
  short* ctx_lo;  // optional bf16 [B*T, H*dh]: the rounding residual ctx_exact - bf16(ctx_exact), so that the backward's
                  // delta = rowsum(dO * O) sees O to ~16 mantissa bits (with the 8-bit O its error is common to a whole
                  // score row and survives the sum over keys in dQ / dK: measured 5e-2 on ViT-L's deep query weights)
  const short* dctx; float* delta; short* dqkv;
  int B, H, T, dh;
  float scale;
  DropCfg drop;
  int nsplit, wpw;  // resident kernels: workgroups per (batch, head) and waves per workgroup (row tiles are dealt in order)
  float* csum_part;  // resident backward kernels: [B * nsplit * wpw][3 * H * dh] per-wave column sums of dqkv as stored, or NULL
};

// XOR applied to the 16-byte chunk index of row r.  Two kinds of read share an image and both must be free of bank conflicts
// (r03: the earlier swizzles served the row reads only; SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE read 0.27 / 0.43 in the
// forward / backward kernels while the GEMM images read 0.00):
//  * row fragments, ds_read_b128: a 16-lane group = 8 rows of lane group lg at chunk c0 and 8 rows of lg ^ 1 at chunk c0 ^ 1
//    (rows r and r ^ 8 never share a chunk) -> the 16 (row, chunk) slots must tile the 256-byte bank row;
//  * transposed fragments, ds_read_b64_tr_b16: a 32-lane half = 8 consecutive rows x one 32-byte chunk PAIR {2dt, 2dt + 1}
//    -> the 8 rows must land on 8 different 32-byte regions of the bank row, so the pair index (chunk >> 1) has to be
//    XORed with something that differs between rows that share their position (r mod rows-per-bank-row).
// DH = 64 (128-byte rows, 2 per bank row): (r & 6) -- pair index ^ ((r >> 1) & 3), the row's parity picks the half.
// DH = 32 (64-byte rows, 4 per bank row): rows r and r + 4 share a quarter -> pair index ^ ((r >> 2) & 1).
// DH = 128 (256-byte rows): pair index ^ (r & 7).
template <int DH>
__device__ __forceinline__ int swz(int r) {
  return DH == 32 ? ((r >> 1) & 2) : (DH == 64 ? (r & 6) : ((r & 7) << 1));
}
template <int DH>
__device__ __forceinline__ int tile_off(int r, int c) {
  return r * (DH * 2) + ((c ^ swz<DH>(r)) << 4);
}

// 8 bf16 of a head's row from column `col` (a multiple of 8), zero past the head size.  A head size that is a multiple of 4
// but not of 8 (the reference's sweep reaches hidden 32 / 8 heads = 4, configs/sweep.yaml:13-18) puts heads at 8-byte offsets
// and ends them in half a chunk: those take 8-byte loads; every other shape keeps its single 16-byte load.
__device__ __forceinline__ i32x4 ld_head8(const short* p, int col, int dh) {
  i32x4 v = {0, 0, 0, 0};
  if ((dh & 7) == 0) {
    if (col < dh) v = *(const i32x4*)(p + col);
    return v;
  }
  if (col < dh) {
    const i32x2 h = *(const i32x2*)(p + col);
    v[0] = h[0]; v[1] = h[1];
  }
  if (col + 4 < dh) {
    const i32x2 h = *(const i32x2*)(p + col + 4);
    v[2] = h[0]; v[3] = h[1];
  }
  return v;
}

// cooperative load of rows [row0, row0+64) x [0, DH) of a strided bf16 matrix into an LDS image (zero fill outside)
template <int DH>
__device__ __forceinline__ void load_tile(char* img, const short* g, long ld, int row0, int nrows, int dh, int tid) {
  constexpr int CPR = DH / 8;
#pragma unroll
  for (int i = 0; i < (RT * CPR) / (AW * 64); ++i) {
    const int q = tid + AW * 64 * i;
    const int r = q / CPR, c = q % CPR;
    const int row = row0 + r;
    i32x4 v = {0, 0, 0, 0};
    if (row < nrows) v = ld_head8(g + (long)row * ld, c * 8, dh);
    *(i32x4*)(img + tile_off<DH>(r, c)) = v;
  }
}

// 16 rows starting at rb (tile-local), reduction index = columns s*32 + 8*(lane>>4) + j
template <int DH>
__device__ __forceinline__ bf16x8 frag_rows(const char* img, int rb, int s, int l15, int lg) {
  return *(const bf16x8*)(img + tile_off<DH>(rb + l15, s * 4 + lg));
}
// transposed: MFMA rows = columns cb..cb+15 of the tile, reduction slots j<4 -> row rb0 + 4*lg + j, j>=4 -> rb1 + ...
template <int DH>
__device__ __forceinline__ bf16x8 frag_cols(const char* img, int rb0, int rb1, int cb, int l15, int lg) {
  const int tq = l15 >> 2, tp = l15 & 3;
  const int col = cb + 4 * tp;
  const int c = col >> 3, half = (col >> 2) & 1;
  const int r0 = rb0 + 4 * lg + tq, r1 = rb1 + 4 * lg + tq;
  bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(img + tile_off<DH>(r0, c) + half * 8));
  bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(img + tile_off<DH>(r1, c) + half * 8));
  return (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
}
// the 16 rows a wave owns, straight from global memory into fragment registers (row = r0 + lane&15)
template <int DH>
__device__ __forceinline__ void load_own(bf16x8 (&f)[DH / 32], const short* g, long ld, int r0, int nrows, int dh,
                                         int l15, int lg) {
#pragma unroll
  for (int s = 0; s < DH / 32; ++s) {
    const int col = s * 32 + lg * 8;
    i32x4 v = {0, 0, 0, 0};
    if (r0 + l15 < nrows) v = ld_head8(g + (long)(r0 + l15) * ld, col, dh);
    f[s] = __builtin_bit_cast(bf16x8, v);
  }
}
__device__ __forceinline__ bf16x8 pack8(const f32x4& a, const f32x4& b) {
  u32x4 r = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3]), pack2bf(b[0], b[1]), pack2bf(b[2], b[3])};
  return __builtin_bit_cast(bf16x8, r);
}
__device__ __forceinline__ f32x4 zero4() { return (f32x4){0.f, 0.f, 0.f, 0.f}; }
// lo = bf16(v - bf16(v)) for 4 values already packed as pk (the context residual), returned packed
__device__ __forceinline__ u32x2 pack_lo(const f32x4& v, const u32x2& pk) {
  const float h0 = __builtin_bit_cast(float, pk[0] << 16), h1 = __builtin_bit_cast(float, pk[0] & 0xFFFF0000u);
  const float h2 = __builtin_bit_cast(float, pk[1] << 16), h3 = __builtin_bit_cast(float, pk[1] & 0xFFFF0000u);
  return (u32x2){pack2bf(v[0] - h0, v[1] - h1), pack2bf(v[2] - h2, v[3] - h3)};
}
// (a function of its own: written out at its call sites, the forward kernels come out with other register numbers)
__device__ __forceinline__ void store_lo(short* dst, const f32x4& v, const u32x2& pk) { *(u32x2*)dst = pack_lo(v, pk); }
__device__ __forceinline__ void wait_vmcnt_dyn(int n) {  // n is wave-uniform; a smaller count than asked for is always safe
#define VIT_WAIT_(k) case k: asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory"); break;
#define VIT_WAIT10_(d) VIT_WAIT_(d##0) VIT_WAIT_(d##1) VIT_WAIT_(d##2) VIT_WAIT_(d##3) VIT_WAIT_(d##4) \
                       VIT_WAIT_(d##5) VIT_WAIT_(d##6) VIT_WAIT_(d##7) VIT_WAIT_(d##8) VIT_WAIT_(d##9)
  switch (n) {
    VIT_WAIT_(0) VIT_WAIT_(1) VIT_WAIT_(2) VIT_WAIT_(3) VIT_WAIT_(4) VIT_WAIT_(5) VIT_WAIT_(6) VIT_WAIT_(7) VIT_WAIT_(8) VIT_WAIT_(9)
    VIT_WAIT10_(1) VIT_WAIT10_(2) VIT_WAIT10_(3)
    default: asm volatile("s_waitcnt vmcnt(40)" ::: "memory"); break;
  }
#undef VIT_WAIT10_
#undef VIT_WAIT_
}

// Dropout keep FLAGS of 4 consecutive query rows at ONE key for the key-owner orientation of the backward kernels, from the
// rows' keys `rk`.  The mask word belongs to a (row, key pair): lanes l15 and l15 ^ 1 hold the two keys of a pair; the even lane
// evaluates rows 0, 1, the odd lane rows 2, 3, and they trade results across the lane pair by DPP (2 words + 2 moves per 4
// elements).  Flags, not multipliers (r03): the draw of (row r, this lane's key) sits in the low or high half of the pair's word by
// the key's parity (= the lane's); shifting the word left by 16 for even keys puts it in the high half either way, and
// "draw >= thr" becomes ONE unsigned compare against thr << 16.  The caller selects with the flags and applies the kept
// elements' 1 / (1 - p) where it is cheapest (an FMA operand, the dV accumulator at the end): 3 VALU per element less than
// building {0, scale} multipliers.
__device__ __forceinline__ void drop_keep4_keyowner(const DropCfg& d, const u32x4& rk, unsigned key, int l15, bool (&keep)[4]) {
  const unsigned odd = (unsigned)l15 & 1u;
  // dropout off: thr << 16 = 0 and every compare below is true -- the flags are formed OUTSIDE the uniform branch, so they are
  // plain compare results (inside it the compiler merged them with the "off" default through a dozen scalar mask instructions
  // per tile: ISA of the A stage, 90 of 586 instructions)
  unsigned h[4] = {~0u, ~0u, ~0u, ~0u};
  if (d.thr) {
    const unsigned ha = drop_bits(odd ? rk[2] : rk[0], key >> 1);
    const unsigned hb = drop_bits(odd ? rk[3] : rk[1], key >> 1);
    const unsigned oa = (unsigned)__builtin_amdgcn_update_dpp(0, (int)ha, 0xB1, 0xF, 0xF, false);
    const unsigned ob = (unsigned)__builtin_amdgcn_update_dpp(0, (int)hb, 0xB1, 0xF, 0xF, false);
    h[0] = odd ? oa : ha; h[1] = odd ? ob : hb; h[2] = odd ? ha : oa; h[3] = odd ? hb : ob;
  }
  const unsigned sh = odd ? 0u : 16u, thr16 = d.thr << 16;
#pragma unroll
  for (int r = 0; r < 4; ++r) keep[r] = (h[r] << sh) >= thr16;
}

// fp32 attention (precision '32'): qkv f32 [B*T, 3*H*dh]
struct Attn32Args {
  const float* qkv; float* ctx; float* lse; float* probs;
  const float* dctx; float* delta; float* dqkv;
  int B, H, T, dh, Tp;
  float scale;
  DropCfg drop;
};

// ------------------------------------------------------------------------------------------------ host: plan and launchers
// What one attention call launches.  attn_plan (attention.hip) is the only place that decides it; the family launchers below
// and the column-sum logic of vit_attention_bwd read it and decide nothing.
enum AttnForm { ATTN_F32_MFMA, ATTN_F32_ROW, ATTN_PIPE, ATTN_RESIDENT, ATTN_TILED };
struct AttnPlan {
  AttnForm form;
  bool bwd;          // backward pass (dQ, then dK/dV; one kernel in the pipelined form)
  int dhp;           // head_dim the bf16 kernels are instantiated for: 32 or 64 (resident), 32, 64 or 128 (tiled)
  bool dma;          // resident: head_dim exactly 64 -> the LDS-DMA prologue
  bool full7;        // pipelined: 192 < T <= 208, the padded length is the compile-time 208
  bool vitb;         // the ViT-B compile-time instantiation: resident forward <64, 2, true, 208, 12, 2, 4>, pipelined <true, 12, true>
  int nsplit, wpw;   // resident: workgroups per (batch, head), waves per workgroup
  unsigned grid;     // resident, pipelined: workgroups
  size_t smem;       // resident, pipelined: dynamic LDS bytes (resident backward: of the dQ kernel)
  size_t smem_dkv;   // resident backward: dynamic LDS bytes of the dK/dV kernel
  int csum_rows;     // backward: partial rows [csum_rows][3 * H * dh] the kernels leave when AttnArgs::csum_part is given; 0 = none
};

// Dynamic LDS above 64 KiB needs the attribute; it is set to the CU's 160 KiB once per KERNEL (the template parameter is the
// kernel itself, not its type: all kernels of a family share one function-pointer type), then the kernel is launched.
template <auto FN, class Args>
static int launch_lds160(dim3 grid, dim3 block, size_t smem, hipStream_t st, const Args& a) {
  static bool done = false;
  if (!done) {
    VIT_HIP(hipFuncSetAttribute((const void*)FN, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    done = true;
  }
  hipLaunchKernelGGL(FN, grid, block, smem, st, a);
  VIT_LAUNCH_CHECK();
  return VIT_OK;
}

// one launcher per family file (attention_tiled / _resident / _pipe / _f32.hip) and what the plan asks each family
int launch_attn_tiled(const AttnArgs& a, const AttnPlan& pl, hipStream_t st);
int launch_attn_probs(const short* qkv, float* probs, int B, int H, int T, int dh, float scale, hipStream_t st);
int launch_attn_resident(const AttnArgs& a, const AttnPlan& pl, hipStream_t st);
int launch_attn_pipe(const AttnArgs& a, const AttnPlan& pl, hipStream_t st);
int launch_attn_f32(Attn32Args& a, const AttnPlan& pl, hipStream_t st);
bool res_fits(int T, int dh);
void res_geometry(int T, bool bwd, int* nsplit, int* wpw);
size_t res_smem(int T, int dhp, bool stats);
bool pipe_fits(int T, int dh);
size_t pipe_smem(int T);
extern int g_attn_split, g_attn_bwd_fused;  // vit_set_option values (attention.hip)

}  // namespace vit
