#include "attention.h"

namespace vit {

// ======================================================================================= resident kernels (T <= RES_MAX_T = 592)
// When a (batch, head)'s whole K and V (or Q and dO) fit the LDS -- at head_dim 64 up to T = 592: every config of
// BASELINE.json's bench line and ViT-L/16 at 384^2 -- one workgroup owns the (batch, head): the tiles are staged ONCE, there
// is a single barrier, and every wave then runs its key loop without any synchronisation.  Each wave owns RQ = 2 sixteen-row
// tiles and feeds both from every K / V fragment it reads, which halves the LDS read traffic per MFMA (the 4-wave tiled
// kernels of attention_tiled.hip were LDS-read and barrier bound at ~135 TFLOP/s).
// Stage two [T, dh] matrices (all their 64-row tiles) at once: every global load of a thread is issued before its first
// LDS store, so a workgroup pays ONE memory latency for its whole working set (a load->store loop paid ten).
template <int DH>
__device__ __forceinline__ void load_all_tiles2(char* imgA, const short* ga, long lda, char* imgB, const short* gb,
                                                long ldb, int T, int dh, int rows_alloc, int tid, int nthr) {
  constexpr int CPR = DH / 8, MAXI = 8;
  const int total = rows_alloc * CPR;  // rows staged (zero beyond T): a multiple of 16, not necessarily of the 64-row tile
  for (int base = 0; base < total; base += MAXI * nthr) {
    i32x4 va[MAXI], vb[MAXI];
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int q = base + tid + i * nthr;
      const int r = q / CPR, c = q % CPR;
      va[i] = vb[i] = (i32x4){0, 0, 0, 0};
      if (q < total && r < T && c * 8 < dh) {
        va[i] = *(const i32x4*)(ga + (long)r * lda + c * 8);
        vb[i] = *(const i32x4*)(gb + (long)r * ldb + c * 8);
      }
    }
#pragma unroll
    for (int i = 0; i < MAXI; ++i) {
      const int q = base + tid + i * nthr;
      if (q < total) {
        const int r = q / CPR, c = q % CPR;
        const int off = (r >> 6) * (RT * DH * 2) + tile_off<DH>(r & 63, c);
        *(i32x4*)(imgA + off) = va[i];
        *(i32x4*)(imgB + off) = vb[i];
      }
    }
  }
}

// LDS-DMA staging of a [rows x 128 B] tile image (head_dim 64): 1 KiB of consecutive LDS per wave-instruction, the XOR
// swizzle applied to the GLOBAL address of each lane; rows past T are clamped to row T - 1 (a DMA has no bounds check).
__device__ __forceinline__ void dma_rows64(char* img, const short* g, long ld, int row0, int nrows_img, int T, int wave,
                                           int lane, int nwaves = 8) {
  // image = nrows_img rows of 128 B, tile layout (row r at r * 128, chunk c at ((c ^ swz(r)) << 4))
  const int p = lane & 7;
  const unsigned img_a = lds_addr_of(img);
  for (int j = wave; j < (nrows_img >> 3); j += nwaves) {
    const int r = (j << 3) + (lane >> 3);
    const int c = p ^ swz<64>(r & 63);
    const int grow = min(row0 + r, T - 1);
    // uniform base + 32-bit lane offset (rows x row stride x 2 B stays far below 2^32 inside one head's rows), raw LDS address
    lds_dma16_s(g, __umul24((unsigned)grow, (unsigned)(ld * 2)) + (unsigned)(c * 16), img_a + j * 1024);
  }
}

// The key loop of one wave: RQ 16-row query tiles (fragments qf) against the staged K / V images of a head; running max m,
// row sums l and the transposed output accumulators ot are the caller's.  pre_pv() runs once, before the first V fragment read.
template <int DH, int RQ, int TPC, class PrePV>  // TPC: the padded length 64 n + 16 when TPC - 16 < T <= TPC is known at compile time (208: ViT-B, 592: ViT-L), else 0
__device__ __forceinline__ void fwd_keyloop(const char* Kimg, const char* Vimg, const bf16x8 (&qf)[RQ][DH / 32], float (&m)[RQ],
                                            float (&l)[RQ], f32x4 (&ot)[RQ][DH / 16], int T, float c, const DropCfg& drop, int bh,
                                            int q00, int l15, int lg, PrePV&& pre_pv) {
  constexpr int TILE = RT * DH * 2;
  // One 64-key tile.  NJ = its 16-key blocks that hold keys (compile-time: the full tiles run a body with no validity test,
  // no -inf fills and no edge select at all; the LAST tile runs the body for its own block count, so a T = 197 head does
  // 3 x 4 + 1 blocks of softmax / dropout work instead of 4 x 4), EDGE = the last block straddles T (per-key select).
  // Blocks that are left out would have contributed exp(-inf) = 0 to the row sums and zero rows to P V: same results.
  // HOOK (compile-time): the caller's pre_pv() runs between this tile's scores and its first V fragment read.
  auto tile = [&](auto njc, auto edgec, auto hookc, int kt) {
    constexpr int NJ = decltype(njc)::value;
    constexpr bool EDGE = decltype(edgec)::value;
    const int kb = kt * RT;
    const char* Kt = Kimg + kt * TILE;
    const char* Vt = Vimg + kt * TILE;
    f32x4 st[RQ][NJ];
    float mx[RQ];
#pragma unroll
    for (int rq = 0; rq < RQ; ++rq) mx[rq] = -INFINITY;
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
      f32x4 a[RQ];
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) a[rq] = zero4();
#pragma unroll
      for (int s = 0; s < DH / 32; ++s) {
        const bf16x8 kf = frag_rows<DH>(Kt, j * 16, s, l15, lg);
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq) a[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[rq][s], a[rq], 0, 0, 0);
      }
      // raw scores: the scale rides in the exp2's FMA below (max(c s) = c max(s), c > 0)
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if (EDGE && j == NJ - 1 && kb + j * 16 + lg * 4 + r >= T) a[rq][r] = -INFINITY;
          mx[rq] = fmaxf(mx[rq], a[rq][r]);
        }
        st[rq][j] = a[rq];
      }
    }
#pragma unroll
    for (int rq = 0; rq < RQ; ++rq) {
      const float mn = fmaxf(m[rq], grp4_max(mx[rq]));  // running max of the RAW scores
      const float alpha = fast_exp2((m[rq] - mn) * c);
      m[rq] = mn;
      const float mnc = mn * c;
      float ls = 0.f;
#pragma unroll
      for (int j = 0; j < NJ; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          st[rq][j][r] = fast_exp2(fmaf(st[rq][j][r], c, -mnc));
          ls += st[rq][j][r];
        }
      l[rq] = l[rq] * alpha + ls;
#pragma unroll
      for (int i = 0; i < DH / 16; ++i) ot[rq][i] *= alpha;
      if (drop.thr) {
        // keep <=> the element's 16-bit draw >= thr: the high draw by ONE unsigned compare of the whole word against thr << 16,
        // the low draw after one shift; dropped probabilities become 0 by a select, and the 1 / (1 - p) of the kept ones is
        // applied once per row at the end (it rides in `inv`): 2.5 instead of 4 VALU per element in this VALU-bound kernel
        const unsigned rkey = drop_rowkey(drop, (unsigned long long)bh * T + (q00 + rq * 16 + l15));
        const unsigned thr16 = drop.thr << 16;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
          const unsigned key = kb + j * 16 + lg * 4;
          const unsigned ha = drop_bits(rkey, key >> 1), hb = drop_bits(rkey, (key >> 1) + 1);
          st[rq][j][0] = (ha << 16) >= thr16 ? st[rq][j][0] : 0.f;
          st[rq][j][1] = ha >= thr16 ? st[rq][j][1] : 0.f;
          st[rq][j][2] = (hb << 16) >= thr16 ? st[rq][j][2] : 0.f;
          st[rq][j][3] = hb >= thr16 ? st[rq][j][3] : 0.f;
        }
      }
    }
    if constexpr (decltype(hookc)::value) pre_pv();
#pragma unroll
    for (int u = 0; u < (NJ + 1) / 2; ++u) {
      const bool two = 2 * u + 1 < NJ;  // compile-time after unrolling
      bf16x8 pf[RQ];
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) pf[rq] = two ? pack8(st[rq][2 * u], st[rq][2 * u + 1 < NJ ? 2 * u + 1 : 2 * u]) : pack8(st[rq][2 * u], zero4());
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) {
        // a 16-row block with no key in it is not staged: point its half of the fragment at the first block (its P is 0)
        const bf16x8 vf = frag_cols<DH>(Vt, u * 32, two ? u * 32 + 16 : u * 32, dt * 16, l15, lg);
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq)
          ot[rq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, pf[rq], ot[rq][dt], 0, 0, 0);
      }
    }
  };
  using std::integral_constant;
  using no = integral_constant<bool, false>;
  using yes = integral_constant<bool, true>;
  if constexpr (TPC != 0) {  // TPC = 64 n + 16: n full tiles and one 16-key block
    static_assert(TPC % 64 == 16, "compile-time sequence lengths end in one 16-key block");
    constexpr int NFULL = TPC / 64;
    tile(integral_constant<int, 4>{}, no{}, yes{}, 0);
#pragma clang loop unroll(disable)  // unrolled, the scheduler overlaps the tiles and spills 50 registers per lane
    for (int kt = 1; kt < NFULL; ++kt) tile(integral_constant<int, 4>{}, no{}, no{}, kt);
    tile(integral_constant<int, 1>{}, yes{}, no{}, NFULL);
    return;
  }
  const int nfull = T / RT;
  // the first tile is peeled (the hook sits inside it); a sequence shorter than one full tile runs the hook before its only tile
  if (nfull > 0) tile(integral_constant<int, 4>{}, no{}, yes{}, 0);
  else pre_pv();
  for (int kt = 1; kt < nfull; ++kt) tile(integral_constant<int, 4>{}, no{}, no{}, kt);
  const int rem = T - nfull * RT;
  if (rem > 0) {
    const int nj = (rem + 15) >> 4;
    if (nj == 1) tile(integral_constant<int, 1>{}, yes{}, no{}, nfull);
    else if (nj == 2) tile(integral_constant<int, 2>{}, yes{}, no{}, nfull);
    else if (nj == 3) tile(integral_constant<int, 3>{}, yes{}, no{}, nfull);
    else tile(integral_constant<int, 4>{}, yes{}, no{}, nfull);
  }
}

// Normalise, store the context rows (+ their rounding residual) and the row statistics of one wave's query tiles.
template <int DH, int RQ, bool FULL = false, int HC = 0>  // FULL: dh == DH is known at compile time (no row-per-lane store path compiled); HC: head count, if known
__device__ __forceinline__ void fwd_finish(const AttnArgs& p, const float (&m)[RQ], const float (&l)[RQ], f32x4 (&ot)[RQ][DH / 16], int b,
                                           int h, int bh, int q00, float c, int l15, int lg) {
  const int T = p.T, dh = FULL ? DH : p.dh, NH = HC ? HC : p.H;
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq) {
    if (q00 + rq * 16 >= T) continue;  // uniform: a tile with no row below T has nothing to store
    const float lt = grp4_sum(l[rq]);
    const int q = q00 + rq * 16 + l15;
    const float inv = (p.drop.thr ? p.drop.scale : 1.0f) / lt;  // the kept probabilities' 1 / (1 - p) rides here
    short* o = p.ctx + ((long)b * T + q) * (NH * dh) + h * dh;
    if ((FULL || dh == DH) && (DH % 32) == 0) {
      // 16-byte stores: two adjacent 16-column tiles per instruction (row-per-lane stores are issue-bound)
#pragma unroll
      for (int dp = 0; dp < DH / 32; ++dp) {
        const f32x4 v0 = ot[rq][dp * 2] * inv, v1 = ot[rq][dp * 2 + 1] * inv;
        u32x2 p0 = {pack2bf(v0[0], v0[1]), pack2bf(v0[2], v0[3])}, p1 = {pack2bf(v1[0], v1[1]), pack2bf(v1[2], v1[3])};
        u32x2 l0 = pack_lo(v0, p0), l1 = pack_lo(v1, p1);
        const int col = widen_pair(p0, p1, lg);
        widen_pair(l0, l1, lg);
        if (q < T) {
          *(u32x4*)(o + dp * 32 + col) = (u32x4){p0[0], p0[1], p1[0], p1[1]};
          if (p.ctx_lo) *(u32x4*)(p.ctx_lo + (o - p.ctx) + dp * 32 + col) = (u32x4){l0[0], l0[1], l1[0], l1[1]};
        }
      }
    } else if (q < T) {
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) {
        const int d = dt * 16 + lg * 4;
        if (d < dh) {
          const f32x4 v = ot[rq][dt] * inv;
          u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *(u32x2*)(o + d) = pk;
          if (p.ctx_lo) store_lo(p.ctx_lo + (o - p.ctx) + d, v, pk);
        }
      }
    }
    if (q < T && lg == 0) p.lse[(long)bh * T + q] = (m[rq] * c + log2f(lt)) * LN2;
  }
}

// DMA: dh == DH == 64 (compile-time, so that the untracked-load prologue below shares no control flow with tracked loads: the
// compiler waits vmcnt(0) wherever a tracked load MIGHT be pending, and would drain the V image with it)
// TPC / HC / NSP / WPWC: a shape known at compile time (TPC = 208: 192 < T <= 208, 12 heads, 2 workgroups x 4 waves per head:
// ViT-B): piece counts, waits, row strides and the tile sequence are constants.  (The same for ViT-L -- 592, 16 heads, 2 x 10
// waves -- measured no gain: its nine-tile key loop dominates and is the same code.) (r03: the same specialisation took 7 %
// off the pair-pipelined backward)
template <int DH, int RQ, bool DMA, int TPC = 0, int HC = 0, int NSP = 0, int WPWC = 0>
__global__ __launch_bounds__(768, 3) void attn_fwd_res_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // workgroups go to the XCDs round-robin (blockIdx % 8): deal each XCD a contiguous run of logical ids, so the nsplit
  // workgroups that stage the SAME head's K / V sit on one XCD, back to back, and the second one finds them in that L2
  const int wg = (gridDim.x % 8 == 0) ? (blockIdx.x % 8) * (gridDim.x / 8) + blockIdx.x / 8 : blockIdx.x;
  const int NH = HC ? HC : p.H, NSPLIT = TPC ? NSP : p.nsplit, WPW = TPC ? WPWC : p.wpw;
  const int bh = wg / NSPLIT, part = wg - bh * NSPLIT, b = bh / NH, h = bh - b * NH;
  const int T = p.T, dh = DMA ? DH : p.dh, ntl = (T + RT - 1) / RT;
  const long ld = 3L * NH * dh;
  const short* qb = p.qkv + (long)b * T * ld + h * dh;
  const short* kb_ = qb + NH * dh;
  const short* vb = kb_ + NH * dh;
  char* Kimg = smem;
  // only the 16-row blocks that hold keys are staged: 208 rows at T = 197 -> 52 KiB per workgroup, so THREE workgroups
  // share a CU's 160 KiB (whole 64-row tiles took 64 KiB: two)
  const int rows_alloc = TPC ? TPC : ((T + 15) & ~15);
  char* Vimg = smem + rows_alloc * (DH * 2);
  const int q00 = (part * WPW + wave) * RQ * 16;
  bf16x8 qf[RQ][DH / 32];
  float m[RQ], l[RQ];
  f32x4 ot[RQ][DH / 16];
  // The wave's Q rows first (plain loads, oldest in the vmcnt order), then K, then V: the waits below are counted, so that
  // the three latencies overlap and the first tile's scores start when K is in (stamps, r03: a wave spent 30 % of its life
  // waiting for K + V together and another 10 % for Q fragments requested only after that)
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq) {
    if constexpr (DMA) {
      // loads the compiler does not track (it would wait vmcnt(0) at their first use and drain V with them): rows past T read
      // the last row again (never stored); the counted wait below covers them -- they are the oldest operations in flight
#pragma unroll
      for (int s = 0; s < DH / 32; ++s) {
        i32x4 v;
        const short* src = qb + (long)min(q00 + rq * 16 + l15, T - 1) * ld + s * 32 + lg * 8;
        asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(src) : "memory");
        qf[rq][s] = __builtin_bit_cast(bf16x8, v);
      }
    } else {
      load_own<DH>(qf[rq], qb, ld, q00 + rq * 16, T, dh, l15, lg);
    }
  }
  bool v_pending = false;
  if constexpr (DMA) {
    // no registers, no zero-fill moves, no address arithmetic per chunk: this kernel saturates the VALU (PMC: 3 waves x 33 %
    // VALU-active per SIMD) and the register-staged form spent ~300 VALU instructions per wave here.  Keys past T are
    // masked to -inf in the edge tile, so the clamped duplicate rows are never used.
    const int nwv = TPC ? WPWC : (int)(blockDim.x >> 6), npc = rows_alloc >> 3;
    dma_rows64(Kimg, kb_, ld, 0, rows_alloc, T, wave, lane, nwv);
    dma_rows64(Vimg, vb, ld, 0, rows_alloc, T, wave, lane, nwv);
    wait_vmcnt_dyn(wave < npc ? (npc - wave + nwv - 1) / nwv : 0);  // all but this wave's V pieces: Q and K are in
#pragma unroll
    for (int rq = 0; rq < RQ; ++rq)
#pragma unroll
      for (int s = 0; s < DH / 32; ++s) asm volatile("" : "+v"(qf[rq][s]));  // uses of Q stay behind the wait
    __builtin_amdgcn_sched_barrier(0);
    v_pending = true;
  } else {
    load_all_tiles2<DH>(Kimg, kb_, ld, Vimg, vb, ld, T, dh, rows_alloc, tid, blockDim.x);
  }
  __syncthreads();
  if (q00 >= T) {  // a wave with no query rows: it still owes the workgroup its V pieces and the barrier that publishes them
    if (v_pending) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
    return;
  }
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq) {
    m[rq] = -INFINITY;
    l[rq] = 0.f;
#pragma unroll
    for (int i = 0; i < DH / 16; ++i) ot[rq][i] = zero4();
  }
  const float c = p.scale * LOG2E;

  fwd_keyloop<DH, RQ, TPC>(Kimg, Vimg, qf, m, l, ot, T, c, p.drop, bh, q00, l15, lg, [&]() {
    if (v_pending) {  // V in and published before its first fragment read
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
    }
  });
  fwd_finish<DH, RQ, DMA, HC>(p, m, l, ot, b, h, bh, q00, c, l15, lg);
}

// The staged-image prologue of the two resident backward kernels, DMA form (dh == DH == 64).  One workgroup per CU at
// T = 577 (148 KiB of images), six of them one after the other: the register-staged prologue (global -> registers -> LDS, two
// or three full round trips for 148 KiB) sat in the open in front of each one's loop, ~6 of its ~35 us.  Here every piece
// of the two images is requested up front by LDS-DMA IN THE ORDER THE LOOP READS THEM (tile 0 of both images, tile 1, ...),
// the wave's own rows before them by loads the compiler does not track (it would wait vmcnt(0) at their first use and drain
// the images with them), and the loop waits, tile by tile, with a COUNTED vmcnt for this wave's pieces of that tile and a
// barrier that publishes everybody's: the first tile's arithmetic starts when 16 KiB have landed, the other 130 KiB arrive
// underneath it.  Piece jg (8 rows x 128 B) of an image belongs to wave jg % nwaves; vmcnt retires in order, so "all but my
// pieces of later tiles" is one number per tile.
struct ImgDma {
  int nwv, npc, wave, tot;
  __device__ __forceinline__ int mine_below(int lim) const { return lim > wave ? (lim - wave + nwv - 1) / nwv : 0; }
  // outstanding operations this wave may leave when tile kt (pieces < 8 (kt + 1)) is about to be read; PER = DMA instructions per piece
  __device__ __forceinline__ int allowed(int kt, int per) const { return tot - per * mine_below(min(8 * (kt + 1), npc)); }
};
__device__ __forceinline__ void dma_piece64(unsigned img_a, const short* g, long ld, int jg, int T, int lane) {
  const int r = (jg << 3) + (lane >> 3);
  const int c = (lane & 7) ^ swz<64>(r & 63);
  lds_dma16_s(g, __umul24((unsigned)min(r, T - 1), (unsigned)(ld * 2)) + (unsigned)(c * 16), img_a + jg * 1024);
}
__device__ __forceinline__ i32x4 load16_untracked(const short* src) {
  i32x4 v;
  asm volatile("global_load_dwordx4 %0, %1, off" : "=v"(v) : "v"(src) : "memory");
  return v;
}

template <int DH, int RQ, bool DMA = false>
__global__ __launch_bounds__(512) void attn_bwd_dq_res_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = RT * DH * 2;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int wave = DMA ? __builtin_amdgcn_readfirstlane(tid >> 6) : (tid >> 6);
  const int bh = blockIdx.x / p.nsplit, part = blockIdx.x - bh * p.nsplit, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T, dh = DMA ? DH : p.dh, ntl = (T + RT - 1) / RT;
  const long ld = 3L * p.H * dh, ldc = (long)p.H * dh;
  const short* qb = p.qkv + (long)b * T * ld + h * dh;
  const short* kb_ = qb + p.H * dh;
  const short* vb = kb_ + p.H * dh;
  const short* dob = p.dctx + (long)b * T * ldc + h * dh;
  const short* ob = p.ctx + (long)b * T * ldc + h * dh;
  char* Kimg = smem;
  // only the 16-row blocks that hold keys are staged: 208 rows at T = 197 -> 52 KiB per workgroup, so THREE workgroups
  // share a CU's 160 KiB (whole 64-row tiles took 64 KiB: two)
  const int rows_alloc = (T + 15) & ~15;
  char* Vimg = smem + rows_alloc * (DH * 2);
  const int q00 = (part * p.wpw + wave) * RQ * 16;
  float* csum = p.csum_part ? p.csum_part + ((long)(bh / p.H) * p.nsplit * p.wpw + part * p.wpw + wave) * ld + h * dh : nullptr;
  const bool idle = q00 >= T;  // a wave with no query rows (the last workgroup of a head): DMA form, it still owes its pieces and barriers

  bf16x8 qf[RQ][DH / 32], dof[RQ][DH / 32];
  float lse2[RQ], del[RQ];
  f32x4 dqt[RQ][DH / 16];
  ImgDma dm = {(int)(blockDim.x >> 6), rows_alloc >> 3, wave, 0};
  if constexpr (DMA) {
    i32x4 ov[RQ][DH / 32], lv[RQ][DH / 32];
    float lraw[RQ];
    const bool has_lo = p.ctx_lo != nullptr;
    if (!idle) {
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) {
        const long row = min(q00 + rq * 16 + l15, T - 1);  // rows past T read the last row again (masked through lse = +inf)
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
          const int col = s * 32 + lg * 8;
          qf[rq][s] = __builtin_bit_cast(bf16x8, load16_untracked(qb + row * ld + col));
          dof[rq][s] = __builtin_bit_cast(bf16x8, load16_untracked(dob + row * ldc + col));
          ov[rq][s] = load16_untracked(ob + row * ldc + col);
          if (has_lo) lv[rq][s] = load16_untracked(p.ctx_lo + (ob - p.ctx) + row * ldc + col);
        }
        asm volatile("global_load_dword %0, %1, off" : "=v"(lraw[rq]) : "v"(p.lse + (long)bh * T + row) : "memory");
      }
    }
    const unsigned Ka = lds_addr_of(Kimg), Va = lds_addr_of(Vimg);
    for (int jg = wave; jg < dm.npc; jg += dm.nwv) {  // ascending piece index = tile order
      dma_piece64(Ka, kb_, ld, jg, T, lane);
      dma_piece64(Va, vb, ld, jg, T, lane);
      dm.tot += 2;
    }
    wait_vmcnt_dyn(dm.allowed(0, 2));  // my own rows (older than every piece) and my pieces of tile 0
    __builtin_amdgcn_sched_barrier(0);
    if (!idle) {
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) {
        asm volatile("" : "+v"(lraw[rq]));
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
          asm volatile("" : "+v"(qf[rq][s]), "+v"(dof[rq][s]), "+v"(ov[rq][s]));  // their uses stay behind the wait
          if (has_lo) asm volatile("" : "+v"(lv[rq][s]));
        }
        const int q = q00 + rq * 16 + l15;
        lse2[rq] = q < T ? lraw[rq] * LOG2E : INFINITY;
        float d_ = 0.f;
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
          const bf16x8 o = __builtin_bit_cast(bf16x8, ov[rq][s]);
#pragma unroll
          for (int e = 0; e < 8; ++e) d_ += bf2f(o[e]) * bf2f(dof[rq][s][e]);
          if (has_lo) {
            const bf16x8 ol = __builtin_bit_cast(bf16x8, lv[rq][s]);
#pragma unroll
            for (int e = 0; e < 8; ++e) d_ += bf2f(ol[e]) * bf2f(dof[rq][s][e]);
          }
        }
        d_ = grp4_sum(d_);
        if (q < T && lg == 0) p.delta[(long)bh * T + q] = d_;
        del[rq] = q < T ? d_ : 0.f;
#pragma unroll
        for (int i = 0; i < DH / 16; ++i) dqt[rq][i] = zero4();
      }
    }
  } else {
    load_all_tiles2<DH>(Kimg, kb_, ld, Vimg, vb, ld, T, dh, rows_alloc, tid, blockDim.x);
    __syncthreads();
    if (idle) {
      if (csum && lane < DH / 4 && lane * 4 < dh) *(f32x4*)(csum + lane * 4) = zero4();  // an idle wave's partial row
      return;
    }
#pragma unroll
    for (int rq = 0; rq < RQ; ++rq) {
      const int q = q00 + rq * 16 + l15;
      load_own<DH>(qf[rq], qb, ld, q00 + rq * 16, T, dh, l15, lg);
      load_own<DH>(dof[rq], dob, ldc, q00 + rq * 16, T, dh, l15, lg);
      lse2[rq] = q < T ? p.lse[(long)bh * T + q] * LOG2E : INFINITY;
      float d_ = 0.f;
#pragma unroll
      for (int s = 0; s < DH / 32; ++s) {
        const int col = s * 32 + lg * 8;
        if (q < T && col < dh) {
          const bf16x8 o = *(const bf16x8*)(ob + (long)q * ldc + col);
#pragma unroll
          for (int e = 0; e < 8; ++e) d_ += bf2f(o[e]) * bf2f(dof[rq][s][e]);
          if (p.ctx_lo) {
            const bf16x8 ol = *(const bf16x8*)(p.ctx_lo + (ob - p.ctx) + (long)q * ldc + col);
#pragma unroll
            for (int e = 0; e < 8; ++e) d_ += bf2f(ol[e]) * bf2f(dof[rq][s][e]);
          }
        }
      }
      d_ = grp4_sum(d_);
      if (q < T && lg == 0) p.delta[(long)bh * T + q] = d_;
      del[rq] = d_;
#pragma unroll
      for (int i = 0; i < DH / 16; ++i) dqt[rq][i] = zero4();
    }
  }
  const float c = p.scale * LOG2E;

  // dropout row keys of this wave's rows; keep flags by compares against thr << 16 (high draw: the word itself, low draw: the
  // word shifted up), the kept elements' 1 / (1 - p) as the FMA's multiplier (r03: 3 VALU per element less than multipliers)
  unsigned rkey[RQ];
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq)
    rkey[rq] = p.drop.thr ? drop_rowkey(p.drop, (unsigned long long)bh * T + (q00 + rq * 16 + l15)) : 0u;
  const unsigned thr16 = p.drop.thr << 16;
  const float dscale = p.drop.thr ? p.drop.scale : 1.0f;
  // One 64-key tile; EDGE = the tile straddles T (per-key validity select).  Full tiles run the body without it (r03: the
  // forward's peeling applied here -- ViT-L's T = 577 walks nine full tiles and one edge tile).
  auto tile = [&](auto edgec, int kt) {
    constexpr bool EDGE = decltype(edgec)::value;
    const int kb = kt * RT;
    const char* Kt = Kimg + kt * TILE;
    const char* Vt = Vimg + kt * TILE;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (EDGE && kb + u * 32 >= T) continue;
      f32x4 ds[RQ][2];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * u + jj;
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq) ds[rq][jj] = zero4();
        if (!EDGE || kb + j * 16 < T) {
          f32x4 s_[RQ], dp[RQ];
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) s_[rq] = dp[rq] = zero4();
#pragma unroll
          for (int s = 0; s < DH / 32; ++s) {
            const bf16x8 kf = frag_rows<DH>(Kt, j * 16, s, l15, lg);
            const bf16x8 vf = frag_rows<DH>(Vt, j * 16, s, l15, lg);
#pragma unroll
            for (int rq = 0; rq < RQ; ++rq) {
              s_[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(kf, qf[rq][s], s_[rq], 0, 0, 0);
              dp[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(vf, dof[rq][s], dp[rq], 0, 0, 0);
            }
          }
          const unsigned key0 = kb + j * 16 + lg * 4;
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) {
            unsigned ha = ~0u, hb = ~0u;  // dropout off: thr16 = 0, every compare true
            if (p.drop.thr) {
              ha = drop_bits(rkey[rq], key0 >> 1);
              hb = drop_bits(rkey[rq], (key0 >> 1) + 1);
            }
            const bool keep[4] = {(ha << 16) >= thr16, ha >= thr16, (hb << 16) >= thr16, hb >= thr16};
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              float pr = fast_exp2(s_[rq][r] * c - lse2[rq]);
              if (EDGE) pr = ((int)key0 + r < T) ? pr : 0.f;
              ds[rq][jj][r] = pr * fmaf(keep[r] ? dp[rq][r] : 0.f, dscale, -del[rq]);
            }
          }
        }
      }
      bf16x8 df[RQ];
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) df[rq] = pack8(ds[rq][0], ds[rq][1]);
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) {
        const bf16x8 ktf = frag_cols<DH>(Kt, u * 32, (!EDGE || kb + u * 32 + 16 < T) ? u * 32 + 16 : u * 32, dt * 16, l15, lg);
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq)
          dqt[rq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ktf, df[rq], dqt[rq][dt], 0, 0, 0);
      }
    }
  };
  // DMA form: before a tile is read, this wave's pieces of it have landed (counted wait) and everybody's are published
  // (barrier).  Three rendezvous only -- tile 0; tiles 1-2; everything else -- all while the waves are still in step anyway:
  // a barrier in front of EVERY tile kept the seven waves in lock-step through the whole loop (all of them in their MFMA
  // chains, then all in their exp / dropout arithmetic) and cost more than the prologue it hid (T = 577: 418 -> 434 us).
  auto arrive = [&](int kt) {
    if constexpr (DMA) {
      if (kt == 0) {
        __builtin_amdgcn_s_barrier();  // the wait for tile 0 was the prologue's
      } else if (kt == 1) {
        wait_vmcnt_dyn(dm.allowed(2, 2));
        __builtin_amdgcn_s_barrier();
      } else if (kt == 3) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
    }
  };
  {
    using std::integral_constant;
    const int nfull = T / RT;
    for (int kt = 0; kt < nfull; ++kt) {
      arrive(kt);
      if (!DMA || !idle) tile(integral_constant<bool, false>{}, kt);
    }
    if (nfull * RT < T) {
      arrive(nfull);
      if (!DMA || !idle) tile(integral_constant<bool, true>{}, nfull);
    }
  }
  if (DMA && idle) {
    if (csum && lane < DH / 4) *(f32x4*)(csum + lane * 4) = zero4();  // an idle wave's partial row
    return;
  }
  f32x4 cs[DH / 16];
#pragma unroll
  for (int dt = 0; dt < DH / 16; ++dt) cs[dt] = zero4();
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq) {
    const int q = q00 + rq * 16 + l15;
    if (q < T) {
      short* o = p.dqkv + ((long)b * T + q) * ld + h * dh;
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) {
        const int d = dt * 16 + lg * 4;
        if (d < dh) {
          const f32x4 v = dqt[rq][dt] * p.scale;
          u32x2 pk = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *(u32x2*)(o + d) = pk;
          cs[dt] += bf_round4(pk);
        }
      }
    }
  }
  if (csum) {  // the query third's bias gradient: this wave's rows, reduced over the batch afterwards
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      const f32x4 t = rows16_sum(cs[dt]);
      const int d = dt * 16 + lg * 4;
      if (l15 == 0 && d < dh) *(f32x4*)(csum + d) = t;
    }
  }
}

template <int DH, int RQ, bool DMA = false>
__global__ __launch_bounds__(512) void attn_bwd_dkv_res_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int TILE = RT * DH * 2;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int wave = DMA ? __builtin_amdgcn_readfirstlane(tid >> 6) : (tid >> 6);
  const int bh = blockIdx.x / p.nsplit, part = blockIdx.x - bh * p.nsplit, b = bh / p.H, h = bh - b * p.H;
  const int T = p.T, dh = DMA ? DH : p.dh, ntl = (T + RT - 1) / RT;
  const long ld = 3L * p.H * dh, ldc = (long)p.H * dh;
  const short* qb = p.qkv + (long)b * T * ld + h * dh;
  const short* kb_ = qb + p.H * dh;
  const short* vb = kb_ + p.H * dh;
  const short* dob = p.dctx + (long)b * T * ldc + h * dh;
  // only the 16-row blocks that hold queries are staged (like K / V in the other two kernels): T = 577 -> 592 rows,
  // 2 x 74 KiB + 7.5 KiB of row statistics (each array padded to whole 64-row DMA pieces) fit the CU's 160 KiB
  const int rows_alloc = (T + 15) & ~15, rows_st = (T + 63) & ~63;
  char* Qimg = smem;
  char* Oimg = smem + rows_alloc * (DH * 2);
  float* lse_s = (float*)(smem + 2 * rows_alloc * (DH * 2));
  float* del_s = lse_s + rows_st;
  unsigned* rk_s = (unsigned*)(del_s + rows_st);  // dropout row keys of the head's query rows
  const int k00 = (part * p.wpw + wave) * RQ * 16;
  float* csum = p.csum_part ? p.csum_part + ((long)(bh / p.H) * p.nsplit * p.wpw + part * p.wpw + wave) * ld + p.H * dh + h * dh
                            : nullptr;
  const bool idle = k00 >= T;  // DMA form: an idle wave still owes the workgroup its pieces and barriers
  bf16x8 kf[RQ][DH / 32], vf[RQ][DH / 32];
  f32x4 dkt[RQ][DH / 16], dvt[RQ][DH / 16];
  ImgDma dm = {(int)(blockDim.x >> 6), rows_alloc >> 3, wave, 0};
  if constexpr (DMA) {
    // see the dQ kernel: own rows (untracked), then the raw row statistics (64 rows x 4 B per piece), then the Q / dO images in
    // the order the query loop reads them
    if (!idle) {
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) {
        const long row = min(k00 + rq * 16 + l15, T - 1);  // keys past T: nothing of theirs is stored
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) {
          kf[rq][s] = __builtin_bit_cast(bf16x8, load16_untracked(kb_ + row * ld + s * 32 + lg * 8));
          vf[rq][s] = __builtin_bit_cast(bf16x8, load16_untracked(vb + row * ld + s * 32 + lg * 8));
        }
      }
    }
    const unsigned La = lds_addr_of(lse_s), Da = lds_addr_of(del_s);
    for (int jp = wave; jp < (rows_st >> 6); jp += dm.nwv) {
      const unsigned off = (unsigned)min(jp * 64 + lane, T - 1) * 4u;
      lds_dma4_s(p.lse + (long)bh * T, off, La + jp * 256);
      lds_dma4_s(p.delta + (long)bh * T, off, Da + jp * 256);
    }
    const unsigned Qa = lds_addr_of(Qimg), Oa = lds_addr_of(Oimg);
    for (int jg = wave; jg < dm.npc; jg += dm.nwv) {
      dma_piece64(Qa, qb, ld, jg, T, lane);
      dma_piece64(Oa, dob, ldc, jg, T, lane);
      dm.tot += 2;
    }
    wait_vmcnt_dyn(dm.tot);  // everything older than the image pieces: my own rows and my statistics pieces
    __builtin_amdgcn_sched_barrier(0);
    if (!idle) {
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq)
#pragma unroll
        for (int s = 0; s < DH / 32; ++s) asm volatile("" : "+v"(kf[rq][s]), "+v"(vf[rq][s]));  // uses stay behind the wait
    }
    __builtin_amdgcn_s_barrier();  // everybody's statistics pieces are in
    for (int i = tid; i < rows_alloc; i += blockDim.x) {
      const float lr = lse_s[i], dr = del_s[i];
      lse_s[i] = i < T ? lr * LOG2E : INFINITY;
      del_s[i] = i < T ? dr : 0.f;
      rk_s[i] = p.drop.thr ? drop_rowkey(p.drop, (unsigned long long)bh * T + i) : 0u;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // published by the first tile's barrier below
  } else {
    load_all_tiles2<DH>(Qimg, qb, ld, Oimg, dob, ldc, T, dh, rows_alloc, tid, blockDim.x);
    for (int i = tid; i < rows_alloc; i += blockDim.x) {
      lse_s[i] = i < T ? p.lse[(long)bh * T + i] * LOG2E : INFINITY;
      del_s[i] = i < T ? p.delta[(long)bh * T + i] : 0.f;
      rk_s[i] = p.drop.thr ? drop_rowkey(p.drop, (unsigned long long)bh * T + i) : 0u;
    }
    __syncthreads();
    if (idle) {
      if (csum && lane < DH / 4 && lane * 4 < dh) {
        *(f32x4*)(csum + lane * 4) = zero4();
        *(f32x4*)(csum + p.H * dh + lane * 4) = zero4();
      }
      return;
    }
#pragma unroll
    for (int rq = 0; rq < RQ; ++rq) {
      load_own<DH>(kf[rq], kb_, ld, k00 + rq * 16, T, dh, l15, lg);
      load_own<DH>(vf[rq], vb, ld, k00 + rq * 16, T, dh, l15, lg);
    }
  }
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq)
#pragma unroll
    for (int i = 0; i < DH / 16; ++i) dkt[rq][i] = dvt[rq][i] = zero4();
  const float c = p.scale * LOG2E;
  const float dscale = p.drop.thr ? p.drop.scale : 1.0f;

  for (int qt = 0; qt < ntl; ++qt) {
    const int qb0 = qt * RT;
    if constexpr (DMA) {  // three rendezvous, as in the dQ kernel: tile 0; tiles 1-2; the rest
      if (qt == 0 || qt == 1) {
        wait_vmcnt_dyn(dm.allowed(qt ? 2 : 0, 2));
        __builtin_amdgcn_s_barrier();
      } else if (qt == 3) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __builtin_amdgcn_s_barrier();
      }
      if (idle) continue;
    }
    const char* Qt = Qimg + qt * TILE;
    const char* Ot = Oimg + qt * TILE;
#pragma unroll
    for (int u = 0; u < 2; ++u) {
      if (qb0 + u * 32 >= T) continue;
      u32x2 pdh[RQ][2], dsh[RQ][2];  // P*mask and dS, packed to bf16 as soon as they exist (register pressure)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        const int j = 2 * u + jj;
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq) pdh[rq][jj] = dsh[rq][jj] = (u32x2){0u, 0u};
        if (qb0 + j * 16 < T) {
          f32x4 s_[RQ], dp[RQ];
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) s_[rq] = dp[rq] = zero4();
#pragma unroll
          for (int s = 0; s < DH / 32; ++s) {
            const bf16x8 qfr = frag_rows<DH>(Qt, j * 16, s, l15, lg);
            const bf16x8 ofr = frag_rows<DH>(Ot, j * 16, s, l15, lg);
#pragma unroll
            for (int rq = 0; rq < RQ; ++rq) {
              s_[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfr, kf[rq][s], s_[rq], 0, 0, 0);
              dp[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ofr, vf[rq][s], dp[rq], 0, 0, 0);
            }
          }
          const f32x4 l4 = *(const f32x4*)(lse_s + qb0 + j * 16 + lg * 4);
          const f32x4 d4 = *(const f32x4*)(del_s + qb0 + j * 16 + lg * 4);
          const u32x4 rk4 = *(const u32x4*)(rk_s + qb0 + j * 16 + lg * 4);
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) {
            const unsigned key = k00 + rq * 16 + l15;
            float pdv[4], dsv[4];
            bool keep[4];
            // the lane pair (l15, l15 ^ 1) holds the two keys of a mask word: two hashes per four elements, traded by DPP, and
            // compare-only flags (key tiles start at even keys: key parity == lane parity)
            drop_keep4_keyowner(p.drop, rk4, key, l15, keep);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const float pr = fast_exp2(s_[rq][r] * c - l4[r]);  // rows past T carry lse = +inf -> 0
              pdv[r] = keep[r] ? pr : 0.f;  // 1 / (1 - p) goes onto dV once, at the end
              dsv[r] = pr * fmaf(keep[r] ? dp[rq][r] : 0.f, dscale, -d4[r]);
            }
            pdh[rq][jj] = (u32x2){pack2bf(pdv[0], pdv[1]), pack2bf(pdv[2], pdv[3])};
            dsh[rq][jj] = (u32x2){pack2bf(dsv[0], dsv[1]), pack2bf(dsv[2], dsv[3])};
          }
        }
      }
      bf16x8 pf[RQ], df[RQ];
#pragma unroll
      for (int rq = 0; rq < RQ; ++rq) {
        pf[rq] = __builtin_bit_cast(bf16x8, (u32x4){pdh[rq][0][0], pdh[rq][0][1], pdh[rq][1][0], pdh[rq][1][1]});
        df[rq] = __builtin_bit_cast(bf16x8, (u32x4){dsh[rq][0][0], dsh[rq][0][1], dsh[rq][1][0], dsh[rq][1][1]});
      }
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) {
        const int rb1 = (qb0 + u * 32 + 16 < T) ? u * 32 + 16 : u * 32;  // an un-staged block: its P and dS are 0
        const bf16x8 otf = frag_cols<DH>(Ot, u * 32, rb1, dt * 16, l15, lg);
        const bf16x8 qtf = frag_cols<DH>(Qt, u * 32, rb1, dt * 16, l15, lg);
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq) {
          dvt[rq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(otf, pf[rq], dvt[rq][dt], 0, 0, 0);
          dkt[rq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qtf, df[rq], dkt[rq][dt], 0, 0, 0);
        }
      }
    }
  }
  if (DMA && idle) {
    if (csum && lane < DH / 4) {
      *(f32x4*)(csum + lane * 4) = zero4();
      *(f32x4*)(csum + p.H * dh + lane * 4) = zero4();
    }
    return;
  }
  f32x4 csk[DH / 16], csv[DH / 16];
#pragma unroll
  for (int dt = 0; dt < DH / 16; ++dt) csk[dt] = csv[dt] = zero4();
#pragma unroll
  for (int rq = 0; rq < RQ; ++rq) {
    const int key = k00 + rq * 16 + l15;
    if (key < T) {
      short* ok = p.dqkv + ((long)b * T + key) * ld + p.H * dh + h * dh;
      short* ov = ok + p.H * dh;
#pragma unroll
      for (int dt = 0; dt < DH / 16; ++dt) {
        const int d = dt * 16 + lg * 4;
        if (d < dh) {
          const f32x4 a = dkt[rq][dt] * p.scale, v = dvt[rq][dt] * dscale;
          u32x2 pk = {pack2bf(a[0], a[1]), pack2bf(a[2], a[3])};
          u32x2 pv = {pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
          *(u32x2*)(ok + d) = pk;
          *(u32x2*)(ov + d) = pv;
          csk[dt] += bf_round4(pk);
          csv[dt] += bf_round4(pv);
        }
      }
    }
  }
  if (csum) {  // the key and value thirds' bias gradients
#pragma unroll
    for (int dt = 0; dt < DH / 16; ++dt) {
      const f32x4 tk = rows16_sum(csk[dt]), tv = rows16_sum(csv[dt]);
      const int d = dt * 16 + lg * 4;
      if (l15 == 0 && d < dh) {
        *(f32x4*)(csum + d) = tk;
        *(f32x4*)(csum + p.H * dh + d) = tv;
      }
    }
  }
}

// resident kernels: a (batch, head)'s whole K/V (or Q/dO) in the LDS -- at head_dim 64 up to T = 592 rows (2 x 74 KiB; the
// backward adds 4.6 KiB of row statistics): ViT-L/16 384^2 (T = 577) fits, one workgroup per CU, three workgroups of 7
// waves per head
constexpr int RES_MAX_T = 592, RES_MAX_DH = 64, RES_RQ = 2;
constexpr int RES_FWD_WAVES = 12, RES_BWD_WAVES = 8;  // most waves per workgroup (res_geometry)

// dynamic LDS of a resident kernel: the staged rows of two [T, dhp] images; stats: + three f32 rows of statistics (dK/dV)
size_t res_smem(int T, int dhp, bool stats) {
  const size_t rows = (T + 15) & ~15, rows_st = (T + 63) & ~63;
  return 2 * rows * dhp * 2 + (stats ? 3 * rows_st * 4 : 0);
}
bool res_fits(int T, int dh) {  // by the dK/dV kernel's LDS, the largest of the three
  if (T > RES_MAX_T || dh > RES_MAX_DH) return false;
  if (dh & 7) return false;  // 8-byte head offsets: the tiled kernels (ld_head8); the resident ones stage 16-byte pieces
  return res_smem(T, dh <= 32 ? 32 : 64, true) <= 160 * 1024;
}

// Most waves per workgroup: 8 for the backward kernels (their csum partial rows share one geometry; dK/dV needs 216 VGPRs = 2
// waves per SIMD), 12 for the forward (166 VGPRs = 3 per SIMD).  It matters where ONE workgroup fills the LDS (T = 577: 148 KiB of
// K / V): 19 waves' worth of query tiles as 3 x 7 waves left a CU with 1.75 waves per SIMD in an issue-bound kernel; 2 x 10 is
// 2.5 per SIMD and stages K / V twice per head instead of three times (r03).
void res_geometry(int T, bool bwd, int* nsplit, int* wpw) {
  const int max_waves = bwd ? RES_BWD_WAVES : RES_FWD_WAVES;
  const int nq = cdiv(T, 16), nw = cdiv(nq, RES_RQ);
  *nsplit = std::max(1, std::min(std::max(g_attn_split, cdiv(nw, max_waves)), nw));
  *wpw = cdiv(nw, *nsplit);
  *nsplit = cdiv(nw, *wpw);
}

// several workgroups per (batch, head), each staging the whole K / V (or Q / dO) but owning a share of the row tiles:
// with 4-wave workgroups three of them fit a CU (150 KiB of LDS, 12 of the 12 wave slots 152 VGPRs leave), so the
// staging latency of one hides behind the key loops of the others; one 7-wave workgroup per CU paid it in the open.
template <void (*FN)(AttnArgs)>
static int launch_res(const AttnArgs& a, const AttnPlan& pl, size_t smem, hipStream_t st) {
  AttnArgs b = a;
  b.nsplit = pl.nsplit;
  b.wpw = pl.wpw;
  return launch_lds160<FN>(dim3(pl.grid), dim3(pl.wpw * 64), smem, st, b);
}

// the two resident backward kernels: head_dim exactly 64 takes the DMA prologue (images requested in reading order, per-tile
// counted waits); head_dim 40 - 56 keeps the register-staged form
#define DISPATCH_RES_BWD(KERNEL, smem)                                                           \
  (pl.dma ? launch_res<KERNEL<64, RES_RQ, true>>(a, pl, smem, st)                                \
          : pl.dhp == 32 ? launch_res<KERNEL<32, RES_RQ, false>>(a, pl, smem, st)                \
                         : launch_res<KERNEL<64, RES_RQ, false>>(a, pl, smem, st))

int launch_attn_resident(const AttnArgs& a, const AttnPlan& pl, hipStream_t st) {
  if (!pl.bwd) {
    if (pl.vitb) return launch_res<attn_fwd_res_kernel<64, RES_RQ, true, 208, 12, 2, 4>>(a, pl, pl.smem, st);
    if (pl.dma) return launch_res<attn_fwd_res_kernel<64, RES_RQ, true>>(a, pl, pl.smem, st);
    if (pl.dhp == 32) return launch_res<attn_fwd_res_kernel<32, RES_RQ, false>>(a, pl, pl.smem, st);
    return launch_res<attn_fwd_res_kernel<64, RES_RQ, false>>(a, pl, pl.smem, st);
  }
  const int rc = DISPATCH_RES_BWD(attn_bwd_dq_res_kernel, pl.smem);
  if (rc != VIT_OK) return rc;
  return DISPATCH_RES_BWD(attn_bwd_dkv_res_kernel, pl.smem_dkv);
}

}  // namespace vit
