#include "attention.h"

namespace vit {

// ======================================================================================= pipelined fused backward (r03)
// The single-kernel backward (one pass, dS through the LDS, five products instead of the two-kernel path's seven).  Its two
// predecessors -- attn_bwd_fused_kernel<DH, NW> (one workgroup per head, r02) and attn_bwd_persist_kernel (one workgroup per CU
// walking heads, r02) -- ran their pieces one after the other: per (head, half) a phase A, a barrier, global loads for the next
// head, a phase B far too short to cover them, another barrier (140 of the persistent form's 364 us were that exposed chain).
// They were removed in r04 once this form had carried the benchmarked shape for a round: what they still served (dh 64 with
// T < 64 or 209 .. 240, dh 32) now takes the two-kernel resident path, which every test also covers.  This form removes every
// global -> register load and every phase boundary from the critical path: the unit of work is a PAIR of query tiles (32 rows), one barrier per pair,
// and in each barrier interval every stage of the backward runs for a DIFFERENT pair, on different waves:
//
//   iteration g:  top      B(g-1)   waves 4-7: dQ of pair g-1 (wave 4 + j: query tile j >> 1, 16-column tiles 2 (j & 1), + 1)
//                                   = dS(g-1) K over all keys (dS image
//                                   [key][32 q] written by A(g-1), K^T by transposing reads of the head's K image); stores
//                          E        every wave, when pair g-1 ended its head: dK / dV of its key tiles + bias-gradient sums
//                 issue    L(g+2)   LDS-DMA of pair g+2's rows into ring slot (g+2) % 3: Q, dO, O, O_lo, lse of 8 rows per wave,
//                                   ALL issued by waves 0-3 (waves 4-7 issue nothing: they carry B); KV(h+1): the next head's
//                                   K and V images, a few pieces per issuing wave per iteration (pairs 1 .. np-1 of head h)
//                 A(g)              every wave, owner = key (tiles w and w + 8): S = Q K^T, dP = dO V^T, P, dS; dV += P^T dO,
//                                   dK += dS^T Q in registers; dS (bf16) -> dS image g % 2.  K / V fragments are read from the
//                                   LDS images when a head starts.  This is the VALU-bound stage; all else hides under it.
//                 wait              s_waitcnt vmcnt(n): n = what THIS iteration issued, so L(g+1) (one iteration old) is in; in a
//                                   head's last iteration n excludes the K / V pieces issued in it (issued first: they are
//                                   read at the top of the next iteration's A stage, before that iteration's wait)
//                 D(g+1)   waves 0-3: delta = rowsum(dO (O + O_lo)), lse * log2 e, dropout row keys of the 8 rows whose
//                                   data the wave loaded ITSELF (its own vmcnt wait orders them: no barrier needed)
//                 barrier           publishes dS(g), statistics(g+1), the landed rows of pair g+1
//
// Nothing younger than an iteration's DMA is a store (stores sit at the top of the next iteration), so the counted wait
// never drains a store or a prefetch.  13 key tiles at T = 197: waves 0-3 and wave 7 own two, waves 4-6 one -- waves 0-3 carry
// the DMA issue and D, waves 4-7 the B stage, so the four SIMDs (waves w and w + 4) are loaded about evenly.  Rows past T: DMA sources are clamped to row
// T - 1, their probabilities are zero through lse = +inf (queries) / +inf added on the key side.
// LDS: ring 3 x 16 KiB + lse staging 3 KiB + 2 K images + V image + 2 dS images [R][32] + statistics = 156 KiB at R = 208.
// dh = 64, 64 <= T <= 208.  Deterministic, no atomics (basemodule.py:250).
// one LDS-DMA piece: 8 rows x 128 B (image rows row_img .. + 7 of a [rows][64] bf16 matrix whose image row 0 is global row
// grow0) into 1 KiB of consecutive LDS; SWZ: the tile image's XOR swizzle, applied to the lane's GLOBAL chunk
template <bool SWZ>
__device__ __forceinline__ void dma_piece(char* dst, const short* g, long ld, int row_img, int grow0, int T, int lane) {
  const int r = row_img + (lane >> 3), pc = lane & 7;
  const int c = SWZ ? (pc ^ swz<64>(r & 63)) : pc;
  const int grow = min(grow0 + r, T - 1);
  lds_dma16_s(g, __umul24((unsigned)grow, (unsigned)(ld * 2)) + (unsigned)(c * 16), lds_addr_of(dst));
}
// dS image of one pair: [key][32 queries] bf16, 64 B per key row, 8-byte slots (4 queries of one key) XOR-swizzled so that the
// phase-A store (16 consecutive keys at one slot, banks mod 32) and the transposing read (8 consecutive keys x 4 adjacent
// slots, banks mod 64) are both conflict-free: rows k and k + 2 share a 128-byte bank row half, rows k and k + 4 a quarter
// of the 256-byte bank row -> slot ^ bits (k2, k3, k1)
__device__ __forceinline__ int ds2_swz(int key) { return (((key >> 2) & 1) << 2) | (((key >> 3) & 1) << 1) | ((key >> 1) & 1); }
__device__ __forceinline__ int ds2_off(int key, int slot) { return key * 64 + ((slot ^ ds2_swz(key)) << 3); }

constexpr int PIPE_SLOT = 16384, PIPE_NS = 3;
size_t pipe_smem(int T) {
  const size_t R = (T + 15) & ~15;
  return PIPE_NS * PIPE_SLOT + PIPE_NS * 4 * 256 + 2 * R * 128 + R * 128 + 2 * R * 64 + 2 * 96 * 4;
}

struct PipeHead { int bh, b, hh; };

// HC: the head count when it is known at compile time (12: ViT-B -- row strides and head divisions become constants), else 0;
// LOC: the context residual is present (the bf16 training path always passes it)
template <bool FULL7, int HC, bool LOC>
__global__ __launch_bounds__(512) void attn_bwd_pipe_kernel(AttnArgs p) {
  resolve_drop(p.drop);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  constexpr int DH = 64, TILE = RT * DH * 2, RQ = 2, ND = DH / 16;
  const int tid = threadIdx.x, lane = tid & 63, l15 = lane & 15, lg = lane >> 4;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NH = HC ? HC : p.H;
  const int T = p.T, BH = p.B * NH;
  const long ld = 3L * NH * DH, ldc = (long)NH * DH, HD = (long)NH * DH;
  // FULL7: 192 < T <= 208 -- every quantity derived from the padded length is a compile-time constant (LDS offsets become
  // immediates, the key-step and tile loops lose their bounds tests)
  const int R = FULL7 ? 208 : ((T + 15) & ~15), nq = R >> 4, np = (nq + 1) >> 1, nks = FULL7 ? 7 : ((T + 31) >> 5);
  char* ring = smem;
  const unsigned ring_a = lds_addr_of(smem);   // DMA destinations are raw LDS addresses
  char* lse_raw = ring + PIPE_NS * PIPE_SLOT;  // [slot][row group][64 words]: raw lse, word l = lse of row (l >> 3) of the group
  char* Kimg0 = lse_raw + PIPE_NS * 4 * 256;   // two K images (heads alternate)
  char* Vimg = Kimg0 + 2 * R * 128;
  char* dSb = Vimg + R * 128;                  // two dS images
  float* stats = (float*)(dSb + 2 * R * 64);   // two sets of [lse 32 | delta 32 | dropout row key 32]
  if ((int)blockIdx.x >= BH) return;
  const int nheads = (BH - (int)blockIdx.x + (int)gridDim.x - 1) / (int)gridDim.x;
  const int G = nheads * np;  // pairs this workgroup walks
  const float c = p.scale * LOG2E;
  const bool has_lo = LOC || p.ctx_lo != nullptr;
  const float dscale = p.drop.thr ? p.drop.scale : 1.0f;  // 1 / (1 - p) of the kept probabilities
  // roles: waves 0-3 issue EVERY DMA piece (Q / dO / O / O_lo / lse of 8 rows each, and the next head's K / V) and derive the
  // statistics of the rows they loaded (D); waves 4-7 issue nothing and run the dQ stage (B): wave 4 + j takes query tile j >> 1 of the pair and the two 16-column tiles 2 (j & 1), 2 (j & 1) + 1 of dQ
  const bool is_d = wave < 4, is_b = wave >= 4;
  const int grp = wave & 3;
  // this wave's key tiles: tile w, and of the tiles past 8 first the four for waves 0-3, then wave 7, 6, 5, 4 -- waves 4-7 carry
  // the dQ stage, the heavier extra (stamps), and the second query tile's pair (6, 7) is idle in a head's last iteration
  const int kt0 = wave, kt1 = wave < 4 ? 8 + wave : 19 - wave;
  const bool own0 = kt0 * 16 < R, own1 = kt1 * 16 < R;
  const float kinf[RQ] = {(kt0 * 16 + l15 < T) ? 0.f : INFINITY, (kt1 * 16 + l15 < T) ? 0.f : INFINITY};
  // Lane constants of the stages OUTSIDE the A stage are derived from an opaque copy of the lane id inside each iteration
  // (`ln` below): hoisted out of the loop they stayed live across the A stage, whose registers then spilled to scratch --
  // and a scratch reload is a vector-memory load the compiler waits for with vmcnt(0), draining the LDS-DMA just issued.
  // A DMA piece is 8 rows x 128 B: lane -> (row rl8 of the piece, 16-byte chunk); the image swizzle of rows 8 j + rl8
  // depends on rl8 only.
  int rl8, csw8, clin8;

  auto head_of = [&](int hidx) -> PipeHead {  // the integer division happens here, once per head and pipeline position
    PipeHead h;
    h.bh = (int)blockIdx.x + hidx * (int)gridDim.x;
    h.b = h.bh / NH;
    h.hh = h.bh - h.b * NH;
    return h;
  };
  auto qoff_of = [&](const PipeHead& h) -> long { return (long)h.b * T * ld + (long)h.hh * DH; };
  auto coff_of = [&](const PipeHead& h) -> long { return (long)h.b * T * ldc + (long)h.hh * DH; };

  // byte offsets of the LDS regions (integers: DMA destinations are raw LDS addresses, see lds_dma16_s)
  const int off_lse = PIPE_NS * PIPE_SLOT, off_K = off_lse + PIPE_NS * 4 * 256, off_V = off_K + 2 * R * 128;
  auto issue_L = [&](int bh, long qo, long co, int pp, int s) -> int {
    // waves 0-3 issue every piece of their 8 rows (Q too), waves 4-7 carry the dQ stage -- they issue nothing.  Uniform 64-bit
    // bases (qo, co: element offsets of the head, computed once per head) + 32-bit lane offsets (bytes inside the head's rows:
    // < 208 rows x 3 D x 2 B): the first form spent ~180 cycles per piece, most of it 64-bit address arithmetic (stamps)
    if (is_b) return 0;
    const unsigned slot = ring_a + s * PIPE_SLOT + grp * 1024;
    const unsigned row = (unsigned)min(pp * 32 + grp * 8 + rl8, T - 1);
    const unsigned oq = __umul24(row, (unsigned)(ld * 2)) + (unsigned)csw8 * 2, oc = __umul24(row, (unsigned)(ldc * 2));
    lds_dma16_s(p.qkv + qo, oq, slot);
    lds_dma16_s(p.dctx + co, oc + (unsigned)csw8 * 2, slot + 4096);
    lds_dma16_s(p.ctx + co, oc + (unsigned)clin8 * 2, slot + 8192);
    if (has_lo) lds_dma16_s(p.ctx_lo + co, oc + (unsigned)clin8 * 2, slot + 12288);
    lds_dma4_s(p.lse + (long)bh * T, row * 4u, ring_a + off_lse + (s * 4 + grp) * 256);
    return has_lo ? 5 : 4;
  };
  // ---- KV: pieces [j0, j0 + n) of a head's K image (buffer kbuf) and V image; piece j < R/8: K rows 8j.., else V
  auto issue_KV = [&](long qo, int kbuf, int j0, int n) -> int {
    const int nk = R >> 3;
    const short* kb_ = p.qkv + qo + HD;
    const unsigned Kd = ring_a + off_K + kbuf * (R * 128), Vd = ring_a + off_V;
    int cnt = 0;
    for (int j = j0; j < j0 + n && j < 2 * nk; ++j) {
      const bool isk = j < nk;
      const int jj = isk ? j : j - nk;
      const unsigned row = (unsigned)min(jj * 8 + rl8, T - 1);
      lds_dma16_s(isk ? kb_ : kb_ + HD, __umul24(row, (unsigned)(ld * 2)) + (unsigned)csw8 * 2, (isk ? Kd : Vd) + jj * 1024);
      ++cnt;
    }
    return cnt;
  };
  const int kv_total = 2 * (R >> 3);
  const int kvp = (kv_total + 4 * (np - 1) - 1) / (4 * (np - 1));  // pieces per issuing wave (0-3) per iteration pp = 1 .. np - 1

  bf16x8 kf[RQ][DH / 32], vf[RQ][DH / 32];
  f32x4 dkt[RQ][ND], dvt[RQ][ND], csq[2];
  csq[0] = csq[1] = zero4();
#pragma unroll
  for (int i = 0; i < ND; ++i) {
#pragma unroll
    for (int rq = 0; rq < RQ; ++rq) dkt[rq][i] = dvt[rq][i] = zero4();
  }
  const int bq = (wave >> 1) & 1, bd = wave & 1;  // B stage: query tile of the pair, dt pair (waves 4-7)

  // (head ordinal, pair) of g - 1, g, g + 1, g + 2; g runs from -2
  int hm = 0, pm = -3, h0 = 0, p0 = -2, h1 = 0, p1 = -1, h2 = 0, p2 = 0;
  PipeHead Hm = head_of(0), H0 = Hm, H1 = Hm, H2 = Hm, Hn = Hm;
  long q2 = qoff_of(H2), c2 = coff_of(H2), qn = q2;  // element offsets of heads H2 / Hn: 64-bit products, once per head
  for (int g = -2; g <= G; ++g) {
    const bool vm = g - 1 >= 0 && g - 1 < G, v0 = g >= 0 && g < G, v1 = g + 1 >= 0 && g + 1 < G, v2 = g + 2 < G;
    int ln = lane;
    asm volatile("" : "+v"(ln));  // opaque: what derives from it is recomputed per iteration, not kept across the A stage
    const int l15o = ln & 15, lgo = ln >> 4;
    rl8 = ln >> 3;
    csw8 = ((ln & 7) ^ (rl8 & 6)) * 8;
    clin8 = (ln & 7) * 8;
    // ------------------------------------------------------------------ top: B(g-1), head-end epilogue (stores)
    if (vm) {
      const bool head_done = pm == np - 1;
      if (is_b) {
        const int qt = pm * 2 + bq;
        if (qt < nq) {
          f32x4 dq0 = zero4(), dq1 = zero4();
          // the transposing reads of the dS image (keys kb + 4 lg + tq (+ 16), this wave's query tile) and of the K image
          // (same keys, the wave's two 16-column tiles); kb is a multiple of 32, which leaves both swizzles alone
          const int tq = l15o >> 2, tp = l15o & 3, krow = 4 * lgo + tq;
          int k_lane[2];
#pragma unroll
          for (int i = 0; i < 2; ++i) {
            const int col = (bd * 2 + i) * 16 + 4 * tp;
            k_lane[i] = krow * 128 + ((((col >> 3)) ^ (krow & 6)) << 4) + ((col >> 2) & 1) * 8;
          }
          const char* dcol = dSb + ((g - 1) & 1) * (R * 64) + ds2_off(krow, bq * 4 + tp);
          const char* Kh = Kimg0 + (hm & 1) * (R * 128);
          const char* ka = Kh + k_lane[0];
          const char* kb2 = Kh + k_lane[1];
          // T <= 208: at most 7 key steps of 32.  Branch-free (a step past the last reads step 0 again and its dS fragment is
          // zeroed; a 16-key block that is not staged reads the block before it, zeroed likewise), so that the fragment reads
          // of two steps are in flight while the MFMAs of the two steps before them run: as one basic block per step the
          // stage was a chain of 7 LDS round trips (3 900 cycles per pair in the stamps, the critical path of the iteration).
          struct BFrag { bf16x8 ds, a, b; };
          auto bload = [&](int ks) -> BFrag {
            // FULL7 (192 < T <= 208, the ViT-B sequence): 7 key steps, the last one half full -- known at compile time, so the
            // offsets are immediates and nothing is selected (70 of the stage's 118 VALU instructions were these adds / selects)
            const bool on = FULL7 || ks < nks, hi_ok = FULL7 ? ks < 6 : (on && ks * 32 + 16 < R);
            const int od = on ? ks * 2048 : 0, okk = on ? ks * 4096 : 0, oh = hi_ok ? 1 : 0;
            bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(dcol + od));
            bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(dcol + od + oh * 1024));
            const bf16x4 a0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(ka + okk));
            const bf16x4 a1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(ka + okk + oh * 2048));
            const bf16x4 b0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(kb2 + okk));
            const bf16x4 b1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((LDS_AS bf16x4*)(kb2 + okk + oh * 2048));
            const bf16x4 z = {0, 0, 0, 0};
            lo = on ? lo : z;
            hi = hi_ok ? hi : z;
            BFrag f;
            f.ds = (bf16x8){lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
            f.a = (bf16x8){a0[0], a0[1], a0[2], a0[3], a1[0], a1[1], a1[2], a1[3]};
            f.b = (bf16x8){b0[0], b0[1], b0[2], b0[3], b1[0], b1[1], b1[2], b1[3]};
            return f;
          };
          auto bmma = [&](const BFrag& f) {
            dq0 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.a, f.ds, dq0, 0, 0, 0);
            dq1 = __builtin_amdgcn_mfma_f32_16x16x32_bf16(f.b, f.ds, dq1, 0, 0, 0);
          };
          {  // BD steps of fragments in flight (12 VGPRs each); 3 and 4 measured the same as 2 (r03: 307 us each)
            constexpr int BD = 2;
            BFrag f[BD];
#pragma unroll
            for (int i = 0; i < BD; ++i) f[i] = bload(i);
#pragma unroll
            for (int ks = 0; ks < 7; ++ks) {
              bmma(f[ks % BD]);
              if (ks + BD < 7) f[ks % BD] = bload(ks + BD);
            }
          }
          const int q = qt * 16 + l15o;
          const f32x4 v0_ = dq0 * p.scale, v1_ = dq1 * p.scale;
          u32x2 pa = {pack2bf(v0_[0], v0_[1]), pack2bf(v0_[2], v0_[3])};
          u32x2 pb = {pack2bf(v1_[0], v1_[1]), pack2bf(v1_[2], v1_[3])};
          if (q < T) {
            csq[0] += bf_round4(pa);
            csq[1] += bf_round4(pb);
          }
          const int col = widen_pair(pa, pb, lgo);
          if (q < T)
            *(u32x4*)(p.dqkv + ((long)Hm.b * T + q) * ld + Hm.hh * DH + bd * 32 + col) = (u32x4){pa[0], pa[1], pb[0], pb[1]};
        }
      }
      if (head_done) {  // dK, dV of this wave's key tiles of head hm; per-wave column sums of everything this wave stored
        f32x4 csk[ND], csv[ND];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) csk[dt] = csv[dt] = zero4();
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq) {
          const int key = (rq ? kt1 : kt0) * 16 + l15o;
          const bool okk = key < T;
          short* ok = p.dqkv + ((long)Hm.b * T + key) * ld + HD + Hm.hh * DH;
#pragma unroll
          for (int dp = 0; dp < 2; ++dp) {
            u32x2 pk[2], pv[2];
#pragma unroll
            for (int i = 0; i < 2; ++i) {
              const f32x4 a = dkt[rq][dp * 2 + i] * p.scale, v = dvt[rq][dp * 2 + i] * dscale;
              pk[i] = (u32x2){pack2bf(a[0], a[1]), pack2bf(a[2], a[3])};
              pv[i] = (u32x2){pack2bf(v[0], v[1]), pack2bf(v[2], v[3])};
              if (okk) {
                csk[dp * 2 + i] += bf_round4(pk[i]);
                csv[dp * 2 + i] += bf_round4(pv[i]);
              }
            }
            const int col = widen_pair(pk[0], pk[1], lgo);
            widen_pair(pv[0], pv[1], lgo);
            if (okk) {
              *(u32x4*)(ok + dp * 32 + col) = (u32x4){pk[0][0], pk[0][1], pk[1][0], pk[1][1]};
              *(u32x4*)(ok + HD + dp * 32 + col) = (u32x4){pv[0][0], pv[0][1], pv[1][0], pv[1][1]};
            }
          }
        }
        if (p.csum_part) {  // one partial row per (batch, wave): [q third | k third | v third], this head's 64 columns of each
          float* csum = p.csum_part + ((long)Hm.b * 8 + wave) * ld + Hm.hh * DH;
#pragma unroll
          for (int dt = 0; dt < ND; ++dt) {
            f32x4 tq_ = zero4();  // a B wave summed dQ over its two 16-column tiles only
            if (is_b && (dt >> 1) == bd) tq_ = rows16_sum(csq[dt & 1]);
            const f32x4 tk = rows16_sum(csk[dt]), tv = rows16_sum(csv[dt]);
            const int d = dt * 16 + lgo * 4;
            if (l15o == 0) {
              *(f32x4*)(csum + d) = tq_;
              *(f32x4*)(csum + HD + d) = tk;
              *(f32x4*)(csum + 2 * HD + d) = tv;
            }
          }
        }
        csq[0] = csq[1] = zero4();
#pragma unroll
        for (int i = 0; i < ND; ++i) {
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) dkt[rq][i] = dvt[rq][i] = zero4();
        }
      }
    }
    // ------------------------------------------------------------------ issue: next head's K / V images, pair g + 2
    // INVARIANT of every hand-counted wait below: a DMA piece may be read only after a wait of the wave that issued it AND a
    // barrier, both at least one iteration newer than its issue.  L pieces: issued in iteration g for pair g + 2, covered by
    // the wait of iteration g + 1 (which leaves only ITS OWN issues in flight), read from iteration g + 2 on.  K / V pieces of
    // the next head are read at the TOP of that head's first A stage, i.e. before that iteration's wait: the ones issued in a
    // head's LAST iteration are therefore waited for in that same iteration (they are issued before the L pieces and vmcnt
    // retires in order, so the wait leaves only the L pieces in flight; the whole A stage lies between issue and wait).
    int nissued = 0, nkv_now = 0;
    if (g == -2) {  // prologue: the first head's images, spread over the waves
      const int per = (kv_total + 7) >> 3;
      nissued += issue_KV(q2, 0, wave * per, per);
    } else if (is_d && v0 && p0 >= 1 && h0 + 1 < nheads) {
      if (p0 == 1) {
        Hn = head_of(h0 + 1);
        qn = qoff_of(Hn);
      }
      const int n_ = issue_KV(qn, (h0 + 1) & 1, ((p0 - 1) * 4 + wave) * kvp, kvp);
      nissued += n_;
      if (p0 == np - 1) nkv_now = n_;  // the head's last iteration: these must have landed before its closing barrier
    }
    if (v2) nissued += issue_L(H2.bh, q2, c2, p2, (g + 2) % PIPE_NS);
    // ------------------------------------------------------------------ A(g)
    if (v0) {
      if (p0 == 0) {  // a head starts: this wave's K / V rows out of the images (landed and published an iteration ago or more)
        const char* Kh = Kimg0 + (h0 & 1) * (R * 128);
#pragma unroll
        for (int rq = 0; rq < RQ; ++rq) {
          const int k0 = (rq ? kt1 : kt0) * 16;
          const bool ex = rq ? own1 : own0;
#pragma unroll
          for (int s = 0; s < DH / 32; ++s) {
            kf[rq][s] = ex ? frag_rows<DH>(Kh + (k0 >> 6) * TILE, k0 & 63, s, l15, lg) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
            vf[rq][s] = ex ? frag_rows<DH>(Vimg + (k0 >> 6) * TILE, k0 & 63, s, l15, lg) : (bf16x8){0, 0, 0, 0, 0, 0, 0, 0};
          }
        }
      }
      if (own0) {
        const char* Qt = ring + (g % PIPE_NS) * PIPE_SLOT;
        const char* Ot = Qt + 4096;
        const float* lse_s = stats + (g & 1) * 96;
        const float* del_s = lse_s + 32;
        const unsigned* rk_s = (const unsigned*)(del_s + 32);
        char* dSw = dSb + (g & 1) * (R * 64);
        u32x2 pdh[RQ][2], dsh[RQ][2];
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) pdh[rq][jj] = dsh[rq][jj] = (u32x2){0u, 0u};
          if (p0 * 32 + jj * 16 < R) {
            f32x4 s_[RQ], dp[RQ];
#pragma unroll
            for (int rq = 0; rq < RQ; ++rq) s_[rq] = dp[rq] = zero4();
#pragma unroll
            for (int s = 0; s < DH / 32; ++s) {
              const bf16x8 qfr = frag_rows<DH>(Qt, jj * 16, s, l15, lg);
              const bf16x8 ofr = frag_rows<DH>(Ot, jj * 16, s, l15, lg);
#pragma unroll
              for (int rq = 0; rq < RQ; ++rq) {
                s_[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qfr, kf[rq][s], s_[rq], 0, 0, 0);
                dp[rq] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ofr, vf[rq][s], dp[rq], 0, 0, 0);
              }
            }
            const f32x4 l4 = *(const f32x4*)(lse_s + jj * 16 + lg * 4);
            const f32x4 d4 = *(const f32x4*)(del_s + jj * 16 + lg * 4);
            const u32x4 rk4 = *(const u32x4*)(rk_s + jj * 16 + lg * 4);
#pragma unroll
            for (int rq = 0; rq < RQ; ++rq) {
              if (rq == 1 && !own1) continue;
              const unsigned key = (rq ? kt1 : kt0) * 16 + l15;
              float pdv[4], dsv[4];
              bool keep[4];
              drop_keep4_keyowner(p.drop, rk4, key, l15, keep);
#pragma unroll
              for (int r = 0; r < 4; ++r) {
                // queries past T carry lse = +inf, keys past T add +inf: probability 0 either way
                const float pr = fast_exp2(s_[rq][r] * c - (l4[r] + kinf[rq]));
                pdv[r] = keep[r] ? pr : 0.f;  // the kept elements' 1 / (1 - p) is applied to dV once, when the head ends
                dsv[r] = pr * fmaf(keep[r] ? dp[rq][r] : 0.f, dscale, -d4[r]);
              }
              pdh[rq][jj] = (u32x2){pack2bf(pdv[0], pdv[1]), pack2bf(pdv[2], pdv[3])};
              dsh[rq][jj] = (u32x2){pack2bf(dsv[0], dsv[1]), pack2bf(dsv[2], dsv[3])};
              *(u32x2*)(dSw + ds2_off((int)key, jj * 4 + lg)) = dsh[rq][jj];
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
        for (int dt = 0; dt < ND; ++dt) {
          // rows 16..31 of the slot always hold rows (clamped duplicates past T; their P and dS are 0)
          const bf16x8 otf = frag_cols<DH>(Ot, 0, 16, dt * 16, l15, lg);
          const bf16x8 qtf = frag_cols<DH>(Qt, 0, 16, dt * 16, l15, lg);
#pragma unroll
          for (int rq = 0; rq < RQ; ++rq) {
            if (rq == 1 && !own1) continue;
            dvt[rq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(otf, pf[rq], dvt[rq][dt], 0, 0, 0);
            dkt[rq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(qtf, df[rq], dkt[rq][dt], 0, 0, 0);
          }
        }
      }
    }
    // ------------------------------------------------------------------ my pieces of pair g + 1 (one iteration old) are in
    wait_vmcnt_dyn(nissued - nkv_now);
    // ------------------------------------------------------------------ D(g+1): statistics of the 8 rows this wave loaded
    if (v1 && is_d) {
      const int s1 = (g + 1) % PIPE_NS;
      const char* slot = ring + s1 * PIPE_SLOT;
      const int rl = grp * 8 + rl8, ch = ln & 7;
      const bf16x8 d8 = *(const bf16x8*)(slot + 4096 + tile_off<DH>(rl, ch));
      const bf16x8 o8 = *(const bf16x8*)(slot + 8192 + rl * 128 + ch * 16);
      bf16x8 l8 = {0, 0, 0, 0, 0, 0, 0, 0};
      if (has_lo) l8 = *(const bf16x8*)(slot + 12288 + rl * 128 + ch * 16);
      const float lraw = *(const float*)(lse_raw + (s1 * 4 + grp) * 256 + ln * 4);
      float d_ = 0.f;
#pragma unroll
      for (int e = 0; e < 8; ++e) d_ += (bf2f(o8[e]) + bf2f(l8[e])) * bf2f(d8[e]);
      d_ = sum_lanes_cpr<8>(d_);
      const int grow = p1 * 32 + rl;
      if (ch == 0) {
        float* st = stats + ((g + 1) & 1) * 96;
        st[rl] = grow < T ? lraw * LOG2E : INFINITY;
        st[32 + rl] = grow < T ? d_ : 0.f;
        ((unsigned*)st)[64 + rl] = p.drop.thr ? drop_rowkey(p.drop, (unsigned long long)H1.bh * T + min(grow, T - 1)) : 0u;
        if (grow < T) p.delta[(long)H1.bh * T + grow] = d_;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    hm = h0; pm = p0; h0 = h1; p0 = p1; h1 = h2; p1 = p2;
    Hm = H0; H0 = H1; H1 = H2;
    if (++p2 == np) {
      p2 = 0;
      ++h2;
      if (h2 < nheads) {
        H2 = head_of(h2);
        q2 = qoff_of(H2);
        c2 = coff_of(H2);
      }
    }
  }
}

bool pipe_fits(int T, int dh) { return dh == 64 && T >= 64 && T <= 208 && pipe_smem(T) <= 160 * 1024; }

int launch_attn_pipe(const AttnArgs& a, const AttnPlan& pl, hipStream_t st) {
  const dim3 grid(pl.grid), block(512);
  if (pl.vitb)  // the ViT-B shape: everything the padded length and the head count determine is constant
    return launch_lds160<attn_bwd_pipe_kernel<true, 12, true>>(grid, block, pl.smem, st, a);
  if (pl.full7) return launch_lds160<attn_bwd_pipe_kernel<true, 0, false>>(grid, block, pl.smem, st, a);
  return launch_lds160<attn_bwd_pipe_kernel<false, 0, false>>(grid, block, pl.smem, st, a);
}

}  // namespace vit
