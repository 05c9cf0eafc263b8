// 256x256 quadrant-phased MFMA GEMM on v_mfma_f32_16x16x32_f16 (v5):  C[m][n] = sum_k A[m][k] * W[n][k]  (+ fused epilogue).
//
// Why (tools/ubench/mfma_shape.hip, profiles/r02_mfma_shape.txt): the GEMMs of this path run under the board POWER cap, not under an
// issue or bandwidth limit -- and on random fp16 operands a pure stream of 16x16x32 MFMAs sustains 1930 TFLOP/s where the 32x32x16
// stream that v1-v4 use sustains 1660 (both 2450 on zeros): the small shape moves 20 % fewer register-file bytes per flop (4
// accumulator registers per instruction instead of 16).  Energy per flop is the lever under a power cap, so this generation keeps
// v3's structure unchanged -- LDS image, piece-granular LDS-DMA ring, quadrant phases, one barrier per phase, counted waits,
// ping-pong wave groups (all of it in gemm256q_ring.h, with the phase table and the hazard rule), tile order -- and changes
// only the instruction and what follows from its fragment maps:
//
//   operand fragments  lane l holds 8 consecutive k of row (l & 15) at k-group (l >> 4): one ds_read_b128 of logical chunk
//                      4*ks + (l >> 4) of a 128-byte LDS row (ks = 0, 1 per 64-deep K-tile); the same 12 / 4 / 8 / 0 reads per phase as v3;
//   accumulators       a wave's 128 x 64 block = 8 (m) x 4 (n) tiles of f32x4; issued with W as the A operand, so lane l owns
//                      C[m = 16 i + (l & 15)][n = 16 j + 4 (l >> 4) + r], r = 0..3: four consecutive n per lane as before;
//   epilogue           the LDS-transposed hand-over of epilogue_handover.h with the scratch filled from this map (HoMap16); this file keeps the
//                      8-wave schedule of the folded LayerNorm's producer epilogue and its consumer prologue.
#pragma once
#include "gemm256n_kernel.h"
#include "gemm256q_ring.h"

// Producer epilogue of the folded LayerNorm-modulate, 8-wave form (the arithmetic and the LDS areas: epilogue_handover.h): wave (g, wn) owns rows
// g * 128 .., column quarter wn of the tile; all eight X rows of a 32-row pass are requested before the pass's first store.
template <class Epi>
__device__ __forceinline__ void g256h_epilogue_mod(f32x4_t (&acc)[8][4], char* smem, const Epi& epi, int m0, int n0, int tile_n, int N, int g, int wn,
                                                   int lane, int wave) {
  char* scr = ho_slot(smem, wave);
  float* cen_s = (float*)(smem + HO_CEN_OFF);
  const int rrow = lane >> 4, rcol = lane & 15;
  const int n = n0 + wn * 64 + rcol * 4;
  if (threadIdx.x < 256) cen_s[threadIdx.x] = epi.cen[m0 + threadIdx.x];
  const HoModCols k = HoModCols::load(epi, m0 / epi.tokens, n);
  __syncthreads();
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    HoMap16::fill_rows(acc, i, scr, lane);
    HO_LGKM0();
    const int rl = g * 128 + i * 32 + rrow;  // + 4 ps: row inside the tile
    f32x4 xo[8];
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) xo[ps] = *(const f32x4*)(epi.X + (long)(m0 + rl + ps * 4) * epi.ldx + n);
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) ho_mod_row(epi, scr, lane, ps, xo[ps], cen_s, k, m0, rl, n, N, ho_red_pass(smem, g, wn, i));
    HO_LGKM0();
  }
  __syncthreads();
  if (wn == 0) ho_mod_tile_sums(epi, smem, g, lane, m0, tile_n);
}

// Consumer prologue of the folded LayerNorm-modulate: (a, b) = (rstd, -rstd (mu - c)) of the tile's 256 rows -> LDS rs[256][2] (above the operand
// ring); tile column 0 publishes mu[m] as the next producer's centring constant.  Two halves around the K loop's first DMAs: the loads are issued
// BEFORE them (vmcnt returns in order: a load issued behind the twelve prologue DMAs would make its consumer wait for all of them -- measured
// +1.3 us per tile), the arithmetic (g256h_rowstat, gemm256q_ring.h) runs while they fly.
template <class Epi>
__device__ __forceinline__ G256hRowStatRegs g256h_rowstat_load(const Epi& epi, int m0, int M) {
  G256hRowStatRegs r;
  const int m = m0 + (int)threadIdx.x < M ? m0 + (int)threadIdx.x : M - 1;
  if (threadIdx.x < 256) {
    const f32x2* pp = (const f32x2*)(epi.st.part + (long)m * epi.st.tiles_p * 2);
#pragma unroll
    for (int t = 0; t < G256H_MAX_PARTS; ++t) r.p[t] = t < epi.st.tiles_p ? pp[t] : (f32x2){0.f, 0.f};
    r.c = epi.st.cen_in[m];
  }
  return r;
}
template <class Epi>
__device__ __forceinline__ void g256h_rowstat_finish(Epi& epi, const G256hRowStatRegs& r, char* smem, int m0, int M, int tile_n) {
  float* rs = (float*)(smem + G256Q_LDS_BYTES);
  if (threadIdx.x < 256) {
    float mu;
    *(f32x2*)(rs + 2 * threadIdx.x) = g256h_rowstat(r, epi.st.inv_n, epi.st.eps, mu);
    if (tile_n == 0 && m0 + (int)threadIdx.x < M) epi.st.cen_out[m0 + threadIdx.x] = mu;
  }
  epi.rs = rs;
  epi.m0 = m0;
}

template <int BN, bool TRACE = false, class Epi>
__device__ __forceinline__ void g256h_epilogue(f32x4_t (&acc)[8][4], char* smem, Epi& epi, int m0, int n0, int M, int N, int g, int wn, int lane,
                                               int wave, int bz, long bsC, int dbg, bool swapped) {
  const bool tr = TRACE && m0 == 0 && n0 == ((dbg >> LFM_DBG_TRACE_COL_SHIFT) & LFM_DBG_TRACE_COL_MASK) * BN && bz == 0;  // the stamped tile: row 0, column TRACE_COL
  epi_batch(epi, bz, bsC, 0);
  g256h_stamp<TRACE>(tr, g, wn, lane, 0);
  if (dbg & LFM_DBG_GEMM_NO_EPILOGUE) return;  // ablation: no epilogue
  if constexpr (epi_is_producer_mod<Epi>::value) {
    g256h_epilogue_mod(acc, smem, epi, m0, n0, n0 / BN, N, g, wn, lane, wave);
    return;
  }
  ho_block<HoMap16, BN, TRACE>(acc, smem, epi, m0, n0, M, N, g, wn, lane, wave, dbg, swapped, tr);
}

// Round 3, where the main loop goes (tools/mainloop_ablation.py on an LFM_MEASURE build, profiles/r03_mainloop_ablation.txt; epilogue off, fc2 shape
// M 16384 x N 1024 x K 4096): full loop 97.5 us (1410 TFLOP/s); without the LDS-DMA issues 82.4; without the fragment reads 69.9; with neither 60.6
// (2267 TFLOP/s, constant operands); barriers: free (60.0 without them, 60.1 with one per K-tile); static priority for the second wave group: WORSE
// (110 us); accumulators pinned to D = C registers through inline-asm MFMAs: nothing (the compiler rotates them through D != C register tuples, which
// costs nothing).  So the LOAD part of a phase (~450-600 cycles: six fragment reads on average + two LDS-DMA issues of 60-185 cycles each) is what
// keeps the matrix pipe at 62 % -- a phase is 256 + L, not 512.  Tried on that evidence and NOT kept: a software-pipelined loop in which every wave
// issues the next step's six reads and its two LDS-DMAs between its own MFMAs (in-place refill of the A fragments, one counted lgkmcnt(5) per group
// of four MFMAs; bit-identical results).  With both wave groups on the same instruction stream all eight waves hit the LDS-DMA issue together and
// the pipe starved (fc2 122 vs 116 us); staggering the groups with two copies of the loop did not fit the register allocator's 256 VGPRs (136-168 B
// of scratch, 180+ us); staggering only the LDS-DMA issue behind a uniform branch (one loop copy, 44 B of scratch) was as slow as un-staggered.  The
// same ablation on the pipelined loop (profiles/r03_mainloop_ablation_incl_pipelined.txt) settles it: its bare MFMA + waits + barriers skeleton runs
// in 69.6 us, the loop in 116.3, without the LDS-DMAs in 92.4 -- reads and DMAs cost as much BETWEEN the MFMAs as they do in a LOAD part of their
// own (~30 cycles of the issuing wave per ds_read_b128, 60-185 per LDS-DMA, and the partner wave does not win that time back).  With a 128x64 wave
// tile the loop needs 0.375 fragment reads and 0.125 LDS-DMAs per MFMA; only a larger wave tile (fewer operand bytes per MFMA) changes that.  Kept from it: ASrcRowMajor rows as 32-bit
// offsets from a uniform base (SGPR base + VGPR offset LDS-DMAs), which took this kernel from 256 VGPRs + 12 B of scratch to 252 VGPRs and none.
// ABL (LFM_MEASURE builds only; results are garbage, timings are the point): 1 = no LDS-DMA after the prologue, 2 = no fragment reads,
// 3 = neither (the bare MFMA stream + barriers), 4 = static priority (s_setprio 1 for the second wave group, no per-phase flips),
// 5 = 3 without the per-phase barriers (the bare MFMA stream), 6 = 3 with one barrier per K-tile instead of per phase,
// 7 = 5 with the accumulators pinned (inline-asm MFMA, D = C), 8 = the full kernel with pinned accumulators
// OPT (round 4): bit 0 = LDS-DMAs through buffer resources (ASrc::buffer_form sources; byte offsets < 2^31, checked at launch).
// Measured (tools/dma_opt_probe.py, profiles/r04_dma_opt_probe.txt; bit-identical results): -0.6 .. -2.1 us on the main loops of both 256x256 kernels
// (252 -> 218 VGPRs in this one) = the default.  (Bit 1 of that round -- a LOAD part's first LDS-DMA ahead of its fragment reads -- cost +1.5 .. +3 us and is gone.)
// OPT bit 2 (round 6): the pieces' LDS-DMAs placed against the LOAD parts' fragment reads (none | B1 | A1 | A0 B0 instead of B1 | A1 | A0 | B0; counted vmcnt 4 4 4 6):
// -0.2 % per DiT-L/2 forward, bit-identical (profiles/r06_dma_phase_balance.txt) -- not the default.
#ifndef G256H_DEFAULT_OPT
#define G256H_DEFAULT_OPT 1
#endif
template <class ASrc, class Epi, bool TRACE = false, int ABL = 0, int OPT = G256H_DEFAULT_OPT>
__global__ __launch_bounds__(512) void gemm256h_tn_kernel(ASrc asrc, const half_t* __restrict__ W, long ldw, int M, int N, int K, int tiles_n,
                                                           Epi epi, long bsA, long bsW, long bsC, int dbg) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int g = wave >> 2, wn = wave & 3;
  static_assert((OPT & 2) == 0, "OPT bit 1 (a LOAD part's first LDS-DMA ahead of its fragment reads, round 4: rejected) no longer exists");
  constexpr bool NO_DMA = ABL == 1 || ABL == 3 || (ABL >= 5 && ABL <= 7);  // (no LDS-DMA after the prologue)
  constexpr bool READS = !(ABL == 2 || ABL == 3 || (ABL >= 5 && ABL <= 7));

  int tile_m, tile_n;
  g256_tile_order(blockIdx.x, gridDim.x, tiles_n, dbg, tile_m, tile_n);
  const int m0 = tile_m * G256_BM, n0 = tile_n * G256_BN;
  bool swapped = false;
  if constexpr (epi_has_transposed<Epi>::value) swapped = epi.transposed(n0);
  const int bz = blockIdx.y;
  asrc.init(bz, bsA);
  W += (long)bz * bsW;

  // ---- DMA sources.  A.sub_s local row lr -> tile row (lr >> 6) * 128 + s * 64 + (lr & 63), B.sub_s local row lr -> tile column (lr >> 5) * 64 + s * 32 + (lr & 31)
  typename ASrc::Row arow[2][2];  // [sub][pass]
  const half_t* wrow[2][2];
  const int cswz = g256q_cswz(tid);
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int p = 0; p < 2; ++p) {
      arow[s][p] = asrc.row(m0 + p * 128 + s * 64 + (tid >> 3));
      const int n = n0 + (p * 2 + (tid >> 8)) * 64 + s * 32 + ((tid >> 3) & 31);
      wrow[s][p] = W + (long)(n < N ? n : N - 1) * ldw + cswz;
    }
  const int nk = K / G256Q_BK;
  const int dma_off = g256q_dma_off(wave);
  bool dma_on = true;  // (ABL 1 / 3 turn it off after the prologue)
  constexpr bool BUFDMA = (OPT & 1) != 0 && asrc_has_buffer<ASrc>::value;
  __amdgpu_buffer_rsrc_t rsa, rsw;
  unsigned avoff[2][2], wvoff[2][2];
  if constexpr (BUFDMA) {
    rsa = asrc.rsrc();
    rsw = __builtin_amdgcn_make_buffer_rsrc((void*)W, 0, -1, 0x00020000);
#pragma unroll
    for (int s = 0; s < 2; ++s)
#pragma unroll
      for (int p = 0; p < 2; ++p) {
        avoff[s][p] = asrc.voff(arow[s][p], cswz);
        const int n = n0 + (p * 2 + (tid >> 8)) * 64 + s * 32 + ((tid >> 3) & 31);
        wvoff[s][p] = ((unsigned)(n < N ? n : N - 1) * (unsigned)ldw + (unsigned)cswz) * 2u;
      }
  }
  // the two LDS-DMAs of a piece (A: of the A-source's current K-tile, begin_tile)
  auto issue_a = [&](int s, char* slot) {
    if (NO_DMA && !dma_on) return;
    if constexpr (BUFDMA) {
      glds16_buf(rsa, avoff[s][0], asrc.soff(), slot + dma_off);
      glds16_buf(rsa, avoff[s][1], asrc.soff(), slot + 8192 + dma_off);
    } else {
      glds16(asrc.ptr(arow[s][0], cswz), slot + dma_off);
      glds16(asrc.ptr(arow[s][1], cswz), slot + 8192 + dma_off);
    }
  };
  auto issue_b = [&](int s, int kt, char* slot) {
    if (NO_DMA && !dma_on) return;
    if constexpr (BUFDMA) {
      glds16_buf(rsw, wvoff[s][0], (unsigned)kt * (G256Q_BK * 2), slot + dma_off);
      glds16_buf(rsw, wvoff[s][1], (unsigned)kt * (G256Q_BK * 2), slot + 8192 + dma_off);
    } else {
      glds16(wrow[s][0] + kt * G256Q_BK, slot + dma_off);
      glds16(wrow[s][1] + kt * G256Q_BK, slot + 8192 + dma_off);
    }
  };

  f32x4_t acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (f32x4_t){0.f, 0.f, 0.f, 0.f};

  int a_addr[2], w_addr[2];  // + i4 * 2048 (16 rows) / + j2 * 2048
  g256q_frag_addr(a_addr, g * 64, lane);
  g256q_frag_addr(w_addr, wn * 32, lane);
  half8_t af[4][2], wf[4][2];  // A: [16-row tile of the current sub][k32 step];  W: [16-column tile 0..3 (sub0: 0,1; sub1: 2,3)][k32 step]

  // LOAD part of phase PH of K-tile t: fragment reads in consumption order (k32-step major), one piece staged, counted wait
  // pieces per part, and the waits behind them (gemm256q_ring.h):  B1(t+1) | A1(t+1) | A0(t+2) | B0(t+2),  in flight 3 3 3 3 | 3 3 2 1 | 0 0 0 0 pieces
  constexpr int VM_S2[4] = {6, 6, 6, 6}, VM_S1[4] = {6, 6, 4, 2};
  // (round 6 experiment, OPT & 4) placed against the parts' fragment reads (12 | 4 | 8 | 0):  none | B1(t+1) | A1(t+1) | A0(t+2) B0(t+2)
  constexpr int VM4_S2[4] = {4, 4, 4, 6}, VM4_S1[4] = {4, 4, 4, 2};
  auto load_part = [&](auto PHC, auto BUFC, int t, bool s1, bool s2) {
    constexpr int PH = decltype(PHC)::value, BUF = decltype(BUFC)::value, HI = BUF * G256Q_BUF_BYTES;
    char* cur = smem + BUF * G256Q_BUF_BYTES;
    char* oth = smem + (BUF ^ 1) * G256Q_BUF_BYTES;
    if constexpr (PH == 0) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        g256q_lds_read<G256Q_SLOT_B0, READS>(wf[0][ks], w_addr[ks] + HI);
        g256q_lds_read<G256Q_SLOT_B0 + 2048, READS>(wf[1][ks], w_addr[ks] + HI);
        g256q_read_a<G256Q_SLOT_A0, READS>(af, a_addr[ks] + HI, ks);
      }
    } else if constexpr (PH == 1) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        g256q_lds_read<G256Q_SLOT_B1, READS>(wf[2][ks], w_addr[ks] + HI);
        g256q_lds_read<G256Q_SLOT_B1 + 2048, READS>(wf[3][ks], w_addr[ks] + HI);
      }
    } else if constexpr (PH == 2) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) g256q_read_a<G256Q_SLOT_A1, READS>(af, a_addr[ks] + HI, ks);
    }
    __builtin_amdgcn_sched_barrier(0);
    constexpr bool BAL = (OPT & 4) != 0;  // the experiment's placement: every piece one part later, A0 and B0 together
    if constexpr (PH == (BAL ? 1 : 0)) {
      if (s1) issue_b(1, t + 1, oth + G256Q_SLOT_B1);
    } else if constexpr (PH == (BAL ? 2 : 1)) {
      if (s1) issue_a(1, oth + G256Q_SLOT_A1);
    } else if (s2) {
      if constexpr (PH == (BAL ? 3 : 2)) {
        asrc.begin_tile(t + 2, G256Q_BK);
        issue_a(0, cur + G256Q_SLOT_A0);
      }
      if constexpr (PH == 3) issue_b(0, t + 2, cur + G256Q_SLOT_B0);
    }
    if constexpr (NO_DMA) G256Q_VMCNT(0);
    else if constexpr (BAL) g256q_load_wait<VM4_S2[PH], VM4_S1[PH]>(s1, s2);
    else g256q_load_wait<VM_S2[PH], VM_S1[PH]>(s1, s2);
  };
  // MFMA part of phase PH: one 64 x 32 quadrant x K = 64 = 16 MFMAs of 16x16x32, every group of 2 behind a counted lgkmcnt.  SW: operands swapped (tiles an
  // epilogue wants transposed -- EpiQKV's V third -- come out as C^T blocks for free)
  auto mfma_part = [&](auto PHC, auto SWC) {
    constexpr int PH = decltype(PHC)::value;
    constexpr bool SW = decltype(SWC)::value != 0;
    constexpr int I0 = (PH >= 2) ? 4 : 0, J0 = (PH == 1 || PH == 2) ? 2 : 0;
    if constexpr (ABL != 4) __builtin_amdgcn_s_setprio(1);
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4) {
        g256q_lgkm_ladder<PH, 4>(ks, i4);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j2 = 0; j2 < 2; ++j2) {
          if constexpr (ABL == 7 || ABL == 8) {  // (experiment) the accumulator pinned: D and C the SAME registers
            if constexpr (SW) asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[I0 + i4][J0 + j2]) : "v"(af[i4][ks]), "v"(wf[J0 + j2][ks]));
            else asm volatile("v_mfma_f32_16x16x32_f16 %0, %1, %2, %0" : "+v"(acc[I0 + i4][J0 + j2]) : "v"(wf[J0 + j2][ks]), "v"(af[i4][ks]));
          } else if constexpr (SW) acc[I0 + i4][J0 + j2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(af[i4][ks], wf[J0 + j2][ks], acc[I0 + i4][J0 + j2], 0, 0, 0);
          else acc[I0 + i4][J0 + j2] = __builtin_amdgcn_mfma_f32_16x16x32_f16(wf[J0 + j2][ks], af[i4][ks], acc[I0 + i4][J0 + j2], 0, 0, 0);
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    if constexpr (ABL != 4) __builtin_amdgcn_s_setprio(0);
  };

  // ---- prologue: pieces A0(0) B0(0) B1(0) A1(0) [A0(1) B0(1)]
  G256hRowStatRegs rsr;
  if constexpr (epi_has_rowstat<Epi>::value) {
    rsr = g256h_rowstat_load(epi, m0, M);
    __builtin_amdgcn_sched_barrier(0);
  }
  asrc.begin_tile(0, G256Q_BK);
  issue_a(0, smem + G256Q_SLOT_A0);
  issue_b(0, 0, smem + G256Q_SLOT_B0);
  issue_b(1, 0, smem + G256Q_SLOT_B1);
  issue_a(1, smem + G256Q_SLOT_A1);
  if (nk > 1) {
    asrc.begin_tile(1, G256Q_BK);
    issue_a(0, smem + G256Q_BUF_BYTES + G256Q_SLOT_A0);
    issue_b(0, 1, smem + G256Q_BUF_BYTES + G256Q_SLOT_B0);
  }
  if constexpr (epi_has_rowstat<Epi>::value) g256h_rowstat_finish(epi, rsr, smem, m0, M, tile_n);
  if (nk > 1) G256Q_VMCNT(6);
  else G256Q_VMCNT(2);
  if constexpr (NO_DMA) {
    G256Q_VMCNT(0);
    dma_on = false;
  }
  if constexpr (!READS) {  // defined fragment contents for the ablated reads
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        af[i][ks] = (half8_t){1, 2, 3, 4, 5, 6, 7, 8};
        wf[i][ks] = (half8_t){1, -1, 1, -1, 1, -1, 1, -1};
      }
  }
  if constexpr (ABL == 4) {
    if (g == 1) __builtin_amdgcn_s_setprio(1);
  }
  G256_BARRIER();
  // the ping-pong K loop (gemm256q_ring.h); one barrier per phase, except in the barrier ablations
  auto end_phase = [&](auto PHC) {
    if constexpr (ABL == 5 || ABL == 7) {
    } else if constexpr (ABL == 6) {
      if constexpr (decltype(PHC)::value == 3) G256_BARRIER();
    } else {
      G256_BARRIER();
    }
  };
  // (the calls are written out: wrapped in one more lambda over SW, the ASrcConv instantiations -- 256 VGPRs -- spill 14 registers instead of 8)
  auto mfma_n = [&](auto PHC) { mfma_part(PHC, g256q_ic<0>{}); };
  auto mfma_s = [&](auto PHC) { mfma_part(PHC, g256q_ic<1>{}); };
  if constexpr (epi_has_transposed<Epi>::value) {
    if (swapped) {
      if (g == 0) g256q_run<0>(nk, load_part, mfma_s, end_phase);
      else g256q_run<1>(nk, load_part, mfma_s, end_phase);
    } else {
      if (g == 0) g256q_run<0>(nk, load_part, mfma_n, end_phase);
      else g256q_run<1>(nk, load_part, mfma_n, end_phase);
    }
  } else {
    if (g == 0) g256q_run<0>(nk, load_part, mfma_n, end_phase);
    else g256q_run<1>(nk, load_part, mfma_n, end_phase);
  }
  if constexpr (ABL == 7 || ABL == 8) asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");  // inline-asm MFMAs: their results must have landed
  g256h_epilogue<G256_BN, TRACE>(acc, smem, epi, m0, n0, M, N, g, wn, lane, wave, bz, bsC, dbg, swapped);
}

template <class ASrc, class Epi, bool TRACE = false, int ABL = 0, int OPT = G256H_DEFAULT_OPT>
static inline int launch_gemm256h_tn(const ASrc& asrc, const half_t* W, long ldw, int M, int N, int K, const Epi& epi, hipStream_t stream,
                                     int batch = 1, long bsA = 0, long bsW = 0, long bsC = 0) {
  if (!asrc_fits(asrc, 0)) return LFM_ERR_SHAPE;
  if constexpr ((OPT & 1) != 0 && asrc_has_buffer<ASrc>::value) {  // byte offsets of the buffer-addressed LDS-DMAs (batched operands: per batch element)
    if (!asrc_fits_buffer(asrc, 0) || (long)N * ldw >= (1L << 31)) return LFM_ERR_SHAPE;
  }
  if (M <= 0 || N <= 0 || K <= 0 || (K % G256Q_BK) != 0 || (N % 4) != 0) return LFM_ERR_SHAPE;
  if ((ldw % 8) != 0 || ((uintptr_t)W & 15)) return LFM_ERR_ALIGN;
  const int tm = cdiv(M, G256_BM), tn = cdiv(N, G256_BN);
  constexpr int LDS = G256Q_LDS_BYTES + (epi_has_rowstat<Epi>::value ? 2048 : 0);  // + rs[256][2] of the folded LayerNorm consumers
  if (!lfm_kernel_lds<&gemm256h_tn_kernel<ASrc, Epi, TRACE, ABL, OPT>>(LDS)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL((gemm256h_tn_kernel<ASrc, Epi, TRACE, ABL, OPT>), dim3(tm * tn, batch), dim3(512), LDS, stream, asrc, W, ldw, M, N, K, tn, epi, bsA,
                     bsW, bsC, lfm_gemm_debug_flags());
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
