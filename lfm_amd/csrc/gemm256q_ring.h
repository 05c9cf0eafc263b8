// The quadrant-phased operand ring and K loop of the 256-row MFMA kernels on v_mfma_f32_16x16x32_f16: everything that does not depend on who runs it.
// Users: gemm256h_tn_kernel (gemm256h_kernel.h, a 256 x 256 tile) and qkv_attention_kernel (qkv_attention_kernel.h, a 256 x 192 tile = one image x one head).
// A user brings its DMA sources, the pieces each LOAD part issues with the vmcnt counts behind them, its MFMA issue, its prologue and what follows the loop.
//
// LDS image.  A 64-deep K-tile = 128-byte rows, staged in four 16-KiB PIECES: A0 / A1 = rows {0..63} / {64..127} of both wave groups' 128-row halves, B0 / B1
// = the two halves of every wave's columns (GEMM: columns {0..31} / {32..63} of its 64; fused kernel: B0 = its 32 Q or K dims, B1 = its 16 V dims, 8 KiB of the
// slot).  Two K-tiles = 128 KiB; K-tile t lives in half t & 1.  Chunk c (16 bytes) of row r sits at c ^ ((r >> 1) & 7), applied to the DMA source address
// (g256q_cswz) and to the fragment read (g256q_frag_addr).  A piece is 1024 chunks: thread tid stages chunks tid and 512 + tid, i.e. one LDS-DMA per 8 KiB.
//
// Phases.  A K-tile is consumed in four phases, one quadrant of the wave's accumulator block each.  Each phase has a LOAD part (fragment reads in the order the
// MFMAs consume them, then LDS-DMA issues, then one counted vmcnt wait) and an MFMA part (every group of MFMAs behind its own counted lgkmcnt, g256q_lgkm_ladder).
//
//   phase   reads (ds_read_b128)        MFMAs, GEMM | fused       accumulators      GEMM stages      fused kernel stages
//   0 (t)   B0 (4) + A0 (8)             16 | 16                   A0 x B0           B1 (t+1)         -
//   1 (t)   B1 (GEMM 4, fused 2)        16 |  8                   A0 x B1           A1 (t+1)         B1 (t+1), A1 (t+1)
//   2 (t)   A1 (8)                      16 |  8                   A1 x B1           A0 (t+2)         A0 (t+2), its first LDS-DMA
//   3 (t)   -                           16 | 16                   A1 x B0           B0 (t+2)         A0 (t+2), its second; B0 (t+2)
//
// (t+1) goes to the other ring half, (t+2) to this one.  The fused kernel's placement 0 | 3 | 1 | 3 balances the LDS-DMAs against the parts' reads; the GEMM has
// the same placement as a measured, not shipped, variant (OPT & 4).
//
// Ping-pong (g256q_run).  The two wave groups (rows 0..127 / 128..255, one wave per SIMD each) alternate LOAD and MFMA parts so that a SIMD's matrix pipe always
// has a wave feeding it, with ONE barrier per phase: between two barriers group 0 runs MFMA(p), LOAD(p+1) and group 1 runs LOAD(p), MFMA(p).
//
// Hazard rule.  (1) A piece is read only behind EVERY wave's counted wait for it AND a barrier.  The wait that ends LOAD(p) covers what LOAD(p+2) reads: group
// 1's LOAD(p) and group 0's LOAD(p+1) share a barrier interval, so by the barrier that ends it both groups have waited for the pieces of LOAD(p+2), which group
// 0 starts in the next interval.  (2) A piece read in LOAD(r) is retired by the counted lgkmcnt waits of MFMA(r) and is re-staged in LOAD(r+2) or later: group 1
// runs LOAD(r) and MFMA(r) one interval before group 0 runs LOAD(r+2), with a barrier in between.  A0 / B0 of K-tile t are read in LOAD 0 and re-staged in LOAD
// 2 / 3 of the same K-tile; B1 / A1 of the other half were read in LOAD 1 / 2 of K-tile t-1 and are re-staged in LOAD 0 / 1 of K-tile t at the earliest.
//
// How a vmcnt number follows from an issue order.  vmcnt counts a wave's outstanding VMEM instructions, which retire in issue order: vmcnt(n) returns once all
// but the newest n have.  The rule: the wait that ends a LOAD part guarantees that what the LOAD part AFTER NEXT reads -- across the K-tile boundary: after LOAD
// 2 / 3 (t) come LOAD 0 / 1 (t+1) -- has landed.  Write down the wave's LDS-DMAs in issue order up to and including this part's own; n = how many of them lie
// behind the last LDS-DMA of the newest piece the part after next reads.  A part after next that reads nothing asks for nothing new: its wait repeats what the
// previous part's guarantee already implies, counted over the longer list.
//   GEMM, two LDS-DMAs per piece, issued  LOAD 0: B1(t+1) | LOAD 1: A1(t+1) | LOAD 2: A0(t+2) | LOAD 3: B0(t+2):
//     LOAD 0 (t)  LOAD 2 (t) reads A1(t);        behind it: A0(t+1) B0(t+1) B1(t+1)             -> vmcnt(6)
//     LOAD 1 (t)  LOAD 3 (t) reads nothing;      A0(t+1) stays landed; behind it: B0 B1 A1(t+1) -> vmcnt(6)
//     LOAD 2 (t)  LOAD 0 (t+1) reads A0 B0(t+1); behind B0(t+1): B1(t+1) A1(t+1) A0(t+2)        -> vmcnt(6)   last-but-one K-tile (no t+2): B1 A1(t+1) -> 4
//     LOAD 3 (t)  LOAD 1 (t+1) reads B1(t+1);    behind it: A1(t+1) A0(t+2) B0(t+2)             -> vmcnt(6)   last-but-one K-tile: A1(t+1)            -> 2
//   Fused kernel, B1 is ONE LDS-DMA, issued  LOAD 0: - | LOAD 1: B1 A1 A1 (t+1) | LOAD 2: A0 (t+2) | LOAD 3: A0 B0 B0 (t+2):
//     LOAD 0 (t)  LOAD 2 (t) reads A1(t);        behind it: A0 A0 B0 B0 (t+1)                   -> vmcnt(4)
//     LOAD 1 (t)  LOAD 3 (t) reads nothing;      A0(t+1) stays landed; behind it: B0 B0 B1 A1 A1 (t+1) -> vmcnt(5)
//     LOAD 2 (t)  LOAD 0 (t+1) reads A0 B0(t+1); behind B0(t+1): B1 A1 A1 (t+1), A0 (t+2)       -> vmcnt(4)   last-but-one K-tile: B1 A1 A1 -> 3
//     LOAD 3 (t)  LOAD 1 (t+1) reads B1(t+1);    behind it: A1 A1 (t+1), A0 A0 B0 B0 (t+2)      -> vmcnt(6)   last-but-one K-tile: A1 A1    -> 2
//   In the last K-tile nothing is in flight that is not read: vmcnt(0).  Prologues issue A0(0) B0(0) B1(0) A1(0) A0(1) B0(1) and wait for all but the newest 6
//   (GEMM) -- B1(0) landed, which LOAD 1 (0) reads one barrier later; LOAD 0 (0) of group 0 runs behind that wait and its own covers A1(0).
#pragma once
#include "gemm256_common.h"

#define G256Q_BK 64
#define G256Q_PIECE 16384
#define G256Q_SLOT_A0 0
#define G256Q_SLOT_B0 (1 * G256Q_PIECE)
#define G256Q_SLOT_B1 (2 * G256Q_PIECE)
#define G256Q_SLOT_A1 (3 * G256Q_PIECE)
#define G256Q_BUF_BYTES (4 * G256Q_PIECE)
#define G256Q_LDS_BYTES (2 * G256Q_BUF_BYTES)

template <int V>
struct g256q_ic {
  static constexpr int value = V;
};

// counted waits (n: a literal or a constant expression)
#define G256Q_VMCNT(n) asm volatile("s_waitcnt vmcnt(%0)" ::"n"(n) : "memory")
#define G256Q_LGKM(n) asm volatile("s_waitcnt lgkmcnt(%0)" ::"n"(n) : "memory")

// ---- LDS-DMA side: thread tid stages 16-byte chunk tid of an 8-KiB issue = physical chunk tid & 7 of LDS row tid >> 3, which holds logical chunk
// (tid & 7) ^ key(row), key = (row >> 1) & 7 = (tid >> 4) & 7.  -> the source column (in halves) of this thread's chunk
__device__ __forceinline__ int g256q_cswz(int tid) { return ((tid & 7) ^ ((tid >> 4) & 7)) * 8; }
// wave-uniform LDS destination of a wave's 1 KiB of an issue (the hardware adds lane * 16)
__device__ __forceinline__ int g256q_dma_off(int wave) { return wave * 1024; }

// ---- fragment side: lane (r = lane & 15, q = lane >> 4) reads logical chunk 4 ks + q of LDS row row0 + r (+ 16 rows per 2048 bytes of offset); row0 and the
// 16-row tile bases are multiples of 16, so the swizzle key depends on the lane only
__device__ __forceinline__ void g256q_frag_addr(int (&addr)[2], int row0, int lane) {
  const int rkey = ((lane & 15) >> 1) & 7, q4 = lane >> 4;
#pragma unroll
  for (int ks = 0; ks < 2; ++ks) addr[ks] = (row0 + (lane & 15)) * 128 + (((ks * 4 + q4) ^ rkey) << 4);
}
// Inline asm: invisible to the compiler's wait insertion, which would otherwise put a full lgkmcnt(0) in front of a phase's first MFMA.  (LIVE = false, main-loop
// ablations of measurement builds: no read, the fragment keeps whatever it held.)
template <int OFF, bool LIVE = true>
__device__ __forceinline__ void g256q_lds_read(half8_t& dst, int addr) {
  if constexpr (LIVE) asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(dst) : "v"(addr), "n"(OFF) : "memory");
  else asm volatile("" : "+v"(dst));
}
// the four 16-row A tiles of piece SLOT (A0 in phase 0, A1 in phase 2) for k32 step ks; addr = the step's fragment address + the ring half
template <int SLOT, bool LIVE = true>
__device__ __forceinline__ void g256q_read_a(half8_t (&af)[4][2], int addr, int ks) {
  g256q_lds_read<SLOT, LIVE>(af[0][ks], addr);
  g256q_lds_read<SLOT + 2048, LIVE>(af[1][ks], addr);
  g256q_lds_read<SLOT + 4096, LIVE>(af[2][ks], addr);
  g256q_lds_read<SLOT + 6144, LIVE>(af[3][ks], addr);
}

// The counted lgkmcnt in front of MFMA group (ks, i4) of phase PH = the reads of the phase's LOAD part that the group does not need yet.  Per k32 step the parts
// read  phase 0: W0 W1 A0 A1 A2 A3 (12 in all; group i4 needs up to A_i4),  phase 1: R1 / 2 W fragments (R1 = 4 in the GEMM, 2 in the fused kernel; all needed by
// the step's first group),  phase 2: A0 A1 A2 A3 (8),  phase 3: nothing.
template <int PH, int R1>
__device__ __forceinline__ void g256q_lgkm_ladder(int ks, int i4) {
  int n = -1;
  if constexpr (PH == 0) n = 9 - 6 * ks - i4;
  else if constexpr (PH == 1) n = i4 == 0 ? (1 - ks) * (R1 / 2) : -1;
  else if constexpr (PH == 2) n = 7 - 4 * ks - i4;
  switch (n) {
    case 0: G256Q_LGKM(0); break;
    case 1: G256Q_LGKM(1); break;
    case 2: G256Q_LGKM(2); break;
    case 3: G256Q_LGKM(3); break;
    case 4: G256Q_LGKM(4); break;
    case 5: G256Q_LGKM(5); break;
    case 6: G256Q_LGKM(6); break;
    case 7: G256Q_LGKM(7); break;
    case 8: G256Q_LGKM(8); break;
    case 9: G256Q_LGKM(9); break;
    default: break;
  }
}

// The counted vmcnt that ends a LOAD part: S2 while K-tile t + 2 is still staged, S1 in the last-but-one K-tile, everything in the last.
template <int S2, int S1>
__device__ __forceinline__ void g256q_load_wait(bool s1, bool s2) {
  if (s2) G256Q_VMCNT(S2);
  else if (s1) G256Q_VMCNT(S1);
  else G256Q_VMCNT(0);
}

// The K loop of wave group G over nk K-tiles, entered behind the barrier that follows the prologue's wait.
//   load_part(PHC, BUFC, t, s1, s2)  LOAD part of phase PH of K-tile t in ring half BUF; s1 / s2: K-tiles t + 1 / t + 2 exist
//   mfma_part(PHC)                   MFMA part of phase PH
//   end_phase(PHC)                   G256_BARRIER() in every shipped kernel (g256q_phase_barrier); measurement variants pass their own
struct g256q_phase_barrier {
  template <class PHC>
  __device__ __forceinline__ void operator()(PHC) const {
    G256_BARRIER();
  }
};
template <int G, class Load, class Mfma, class End = g256q_phase_barrier>
__device__ __forceinline__ void g256q_run(int nk, Load&& load_part, Mfma&& mfma_part, End&& end_phase = End{}) {
  if constexpr (G == 0) load_part(g256q_ic<0>{}, g256q_ic<0>{}, 0, 1 < nk, 2 < nk);
  G256_BARRIER();
  auto tile = [&](auto BUFC, int t) {
    constexpr int BUF = decltype(BUFC)::value;
    const bool s1 = t + 1 < nk, s2 = t + 2 < nk, s3 = t + 3 < nk;
    auto phase = [&](auto PHC) {
      constexpr int PH = decltype(PHC)::value;
      if constexpr (G == 0) {
        mfma_part(PHC);
        if constexpr (PH < 3) load_part(g256q_ic<PH + 1>{}, BUFC, t, s1, s2);
        else if (s1) load_part(g256q_ic<0>{}, g256q_ic<(BUF ^ 1)>{}, t + 1, s2, s3);
      } else {
        load_part(PHC, BUFC, t, s1, s2);
        mfma_part(PHC);
      }
      end_phase(PHC);
    };
    phase(g256q_ic<0>{});
    phase(g256q_ic<1>{});
    phase(g256q_ic<2>{});
    phase(g256q_ic<3>{});
  };
  int t = 0;
  for (; t + 1 < nk; t += 2) {
    tile(g256q_ic<0>{}, t);
    tile(g256q_ic<1>{}, t + 1);
  }
  if (t < nk) tile(g256q_ic<0>{}, t);
}

// ---- row statistics of the folded LayerNorm-modulate consumers.  A row's partials (sum X, sum (X - c)^2 per producer tile) and centring constant c, in
// registers: loaded ahead of the first LDS-DMAs, finished while they fly.
// (The g256h_ names: these are gemm256h_kernel.h's, which keeps the loader and the finisher; the type and the arithmetic live here because the fused kernel
// shares them.)
#define G256H_MAX_PARTS 5  // residual width <= 1280
struct G256hRowStatRegs {
  f32x2 p[G256H_MAX_PARTS];
  float c;
};
// -> (a, b) = (rstd, -rstd (mu - c)) and the row mean.  THE arithmetic: every consumer must agree bit for bit.
__device__ __forceinline__ f32x2 g256h_rowstat(const G256hRowStatRegs& r, float inv_n, float eps, float& mu) {
  float sx = 0.f, sq = 0.f;
#pragma unroll
  for (int t = 0; t < G256H_MAX_PARTS; ++t) {  // fixed order
    sx += r.p[t].x;
    sq += r.p[t].y;
  }
  mu = sx * inv_n;
  const float dl = mu - r.c;
  const float var = fmaxf(sq * inv_n - dl * dl, 0.f);
  const float rstd = rsqrtf(var + eps);
  return (f32x2){rstd, -rstd * dl};
}
