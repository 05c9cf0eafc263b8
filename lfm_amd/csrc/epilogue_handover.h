// The epilogue hand-over of the 256-row kernels, once: the per-wave LDS transpose between the MFMA accumulator maps and row-major global stores.
// Users: gemm256n_kernel.h (256x128, 32x32x16 map), gemm256h_kernel.h and gemm256w_kernel.h (256x256, 16x16x32 map: one and two blocks per wave),
// conv_halo_kernel.h (fill + 8-column read-back under its own pixel addressing), the producer epilogues of the folded LayerNorm (fill + 4-column
// read-back + the shared row arithmetic below).
//
// Why a hand-over.  The MFMA leaves a lane with 4 consecutive n of ONE row m per register group: storing that directly makes every store instruction
// touch 16-32 different 128-B lines with 16-32 B each (measured: ~12 us per tile, L2-request-bound).  Instead a wave writes a 32-row x 64-column
// slice of its 128 x 64 accumulator block into a PRIVATE fp32 scratch [32][64 + pad] (row stride 272 B: conflict-free ds_write_b128) and reads it back
// row-major, so that the lanes of a store instruction cover whole rows: 8 lanes x 16 B of fp16 (store8: one instruction = 8 rows x one full 128-B
// line; the fp16 epilogues were store-ISSUE bound -- 3.8 TB/s ~ 7 B/cycle/CU with 8-byte stores, the guide's T21 case) or 16 lanes x 4 columns.
//
// The scratch image and the read-backs are the same for every kernel; only the map from accumulator registers to scratch differs (HoMap32, HoMap16).
//
// CONTRACTS of the row-major driver (ho_rows) that epilogues rely on -- EpiConvStatsF16 (nhwc_common.h) on the first two:
//   * a lane owns columns n0 + 64 wn + 8 (lane & 7) .. + 7 for EVERY store8 of a tile (4-column form: n0 + 64 wn + 4 (lane & 15) .. + 3);
//   * rows come in the order pass i = 0..3 (32 rows each), then ps = 0..3 (rows (lane >> 3) + 8 ps of the pass; 4-column form: ps = 0..7, rows
//     (lane >> 4) + 4 ps): store8 is called in that order, so the first call of a tile is the lane's lowest row;
//   * all auxiliary loads of a pass are issued before its first store (vmcnt counts stores too and returns in order: a load issued behind a pass's
//     stores waits for their round trip); column-only operands (column_aux) once per tile, ahead of the first pass.
#pragma once
#include "gemm_kernel.h"

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// ---- scratch geometry
#define HO_ROW_BYTES 272                         // 64 fp32 + 16 B of padding
#define HO_ROWS 32                               // rows per fill
#define HO_SLOT_BYTES (HO_ROWS * HO_ROW_BYTES)   // 8704: one wave's scratch; slot w starts at w * HO_SLOT_BYTES
#define HO_SLOTS 8                               // the producer epilogues' areas sit behind eight slots (four-wave kernels use slots 0..3)
#define HO_RED_OFF (HO_SLOTS * HO_SLOT_BYTES)    // red[128-row half][column quarter][128 rows][2]: per-row partial sums of a quarter, 8 KiB
#define HO_RED_BYTES 8192
#define HO_CEN_OFF (HO_RED_OFF + HO_RED_BYTES)   // cen_s[256]: centring constants of the tile's rows
#define HO_TILE_ROWS 256                         // a tile = two 128-row halves
#define HO_LGKM0() asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory")

__device__ __forceinline__ char* ho_slot(char* smem, int wave) { return smem + wave * HO_SLOT_BYTES; }

// ---- the two accumulator maps.  fill_rows(acc, I, scr, lane): rows 32 I .. 32 I + 31 of the wave's 128 x 64 block -> scratch[row][column];
// fill_cols(acc, J, ih, scr, lane): of a tile computed with the MFMA operands SWAPPED (a lane holds four consecutive m of one n), columns
// 32 J .. 32 J + 31 x rows 64 ih .. 64 ih + 63 -> scratch[column][row]; for_each_frag: f(row, column, C[row][column .. column + 3]) straight from
// the registers (epilogues that want the fragment layout).  Callers wait (HO_LGKM0) between a fill and its read-back and after the read-back.
// hoist_column_aux: ho_rows loads column-only auxiliary operands once per tile.
struct HoMap32 {  // v_mfma_f32_32x32x16: acc[i][j] = 32 x 32 block; lane l owns row (l & 31), columns 8 q + 4 (l >> 5) + r of register group q
  typedef f32x16 Acc[4][2];
  static constexpr bool hoist_column_aux = true;
  static __device__ __forceinline__ f32x4 group(const f32x16& a, int q) { return (f32x4){a[4 * q], a[4 * q + 1], a[4 * q + 2], a[4 * q + 3]}; }
  static __device__ __forceinline__ void fill_rows(const Acc& acc, int I, char* scr, int lane) {
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int q = 0; q < 4; ++q) *(f32x4*)(scr + (lane & 31) * HO_ROW_BYTES + (j * 32 + 8 * q + 4 * (lane >> 5)) * 4) = group(acc[I][j], q);
  }
  static __device__ __forceinline__ void fill_cols(const Acc& acc, int J, int ih, char* scr, int lane) {
#pragma unroll
    for (int ii = 0; ii < 2; ++ii)
#pragma unroll
      for (int q = 0; q < 4; ++q) *(f32x4*)(scr + (lane & 31) * HO_ROW_BYTES + (ii * 32 + 8 * q + 4 * (lane >> 5)) * 4) = group(acc[2 * ih + ii][J], q);
  }
  template <class F>
  static __device__ __forceinline__ void for_each_frag(const Acc& acc, int lane, F&& f) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int q = 0; q < 4; ++q) f(i * 32 + (lane & 31), j * 32 + 8 * q + 4 * (lane >> 5), group(acc[i][j], q));
  }
};
struct HoMap16 {  // v_mfma_f32_16x16x32: acc[i][j] = 16 x 16 tile; lane l owns row (l & 15), columns 4 (l >> 4) + r
  typedef f32x4_t Acc[8][4];
  static constexpr bool hoist_column_aux = true;
  static __device__ __forceinline__ void fill_rows(const Acc& acc, int I, char* scr, int lane) {
#pragma unroll
    for (int h2 = 0; h2 < 2; ++h2)
#pragma unroll
      for (int j = 0; j < 4; ++j) *(f32x4_t*)(scr + (h2 * 16 + (lane & 15)) * HO_ROW_BYTES + (j * 16 + (lane >> 4) * 4) * 4) = acc[2 * I + h2][j];
  }
  static __device__ __forceinline__ void fill_cols(const Acc& acc, int J, int ih, char* scr, int lane) {
#pragma unroll
    for (int j2 = 0; j2 < 2; ++j2)
#pragma unroll
      for (int i4 = 0; i4 < 4; ++i4)
        *(f32x4_t*)(scr + (j2 * 16 + (lane & 15)) * HO_ROW_BYTES + (i4 * 16 + (lane >> 4) * 4) * 4) = acc[4 * ih + i4][2 * J + j2];
  }
  template <class F>
  static __device__ __forceinline__ void for_each_frag(const Acc& acc, int lane, F&& f) {
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j) f(i * 16 + (lane & 15), j * 16 + (lane >> 4) * 4, (f32x4){acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]});
  }
};

// ---- the read-backs, one step `ps` of a pass each (callers unroll over ps).
// 8 columns: lane = (rrow = lane >> 3, rcol = lane & 7) gets columns 8 rcol .. + 7 of scratch row rrow + 8 ps, ps = 0..3
__device__ __forceinline__ void ho_read8(const char* scr, int lane, int ps, f32x4& lo, f32x4& hi) {
  lo = *(const f32x4*)(scr + (ps * 8 + (lane >> 3)) * HO_ROW_BYTES + (lane & 7) * 32);
  hi = *(const f32x4*)(scr + (ps * 8 + (lane >> 3)) * HO_ROW_BYTES + (lane & 7) * 32 + 16);
}
// 4 columns: lane = (lane >> 4, lane & 15) gets columns 4 (lane & 15) .. + 3 of scratch row (lane >> 4) + 4 ps, ps = 0..7.  After fill_cols this is
// also the 4-row transposed form: four consecutive m of column (lane >> 4) + 4 ps
__device__ __forceinline__ f32x4 ho_read4(const char* scr, int lane, int ps) {
  return *(const f32x4*)(scr + (ps * 4 + (lane >> 4)) * HO_ROW_BYTES + (lane & 15) * 16);
}
// wide transposed form (after fill_cols): lane = (column (lane >> 3) + 8 ps, tokens ml .. ml + 3 and ml + 8 .. ml + 11 of the 64) -- one 16-byte
// chunk of the permuted V^T row (vt_pos, gemm_epilogues.h)
__device__ __forceinline__ int ho_ml(int lane) { return 16 * ((lane & 7) >> 1) + 4 * (lane & 1); }
__device__ __forceinline__ void ho_read8_t(const char* scr, int lane, int ps, f32x4& lo, f32x4& hi) {
  lo = *(const f32x4*)(scr + (ps * 8 + (lane >> 3)) * HO_ROW_BYTES + ho_ml(lane) * 4);
  hi = *(const f32x4*)(scr + (ps * 8 + (lane >> 3)) * HO_ROW_BYTES + ho_ml(lane) * 4 + 32);
}

// ---- measurement only (lfm_gemm_select flag TRACE_GEMM with kernel 5): waves 0 and 4 of the tile at row 0, column TRACE_COL stamp s_memtime at the end
// of the K loop (slot 0) and after the scratch fill / read-back / auxiliary loads / store issue (slots 1 + 4 i .. 4 + 4 i) of each of the four passes i of
// a block, 17 = end; parked in g256q_trace and read back with lfm_gemm_trace_read().  One copy per translation unit; dit.hip's is read back.
#define G256Q_TRACE_MAX 2048
static __device__ unsigned long long g256q_trace[2][G256Q_TRACE_MAX];
template <bool TRACE>
__device__ __forceinline__ void g256h_stamp(bool tr, int g, int wn, int lane, int slot) {
  if constexpr (TRACE) {
    if (tr && wn == 0 && lane == 0) {
      unsigned long long t;
      asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
      g256q_trace[g][slot] = t;
    }
  }
}

// ---- the row-major driver: one 128 x 64 accumulator block (rows g * 128 .., columns wn * 64 .. of the tile at m0, n0; BN = the tile's width) through
// `epi`, scratch slot `wave`.  narrow: the 4-column form although the epilogue has store8 (A/B flag).  See the contracts at the top.
template <class Map, int BN, bool TRACE = false, class Epi>
__device__ __forceinline__ void ho_rows(const typename Map::Acc& acc, char* smem, const Epi& epi, int m0, int n0, int M, int N, int g, int wn, int lane,
                                        int wave, bool narrow, bool tr = false) {
  char* scr = ho_slot(smem, wave);
  const bool interior = (m0 + HO_TILE_ROWS <= M) && (n0 + BN <= N);
  constexpr bool COL = epi_column_aux<Epi>::value && Map::hoist_column_aux;  // bias-only auxiliary operand: loaded once per tile, ahead of the first store
  if constexpr (epi_has_store8<Epi>::value) {
    if (!narrow && epi.wide_ok()) {
      const int rrow = lane >> 3, rcol = lane & 7;
      typename Epi::Aux cl, ch;
      if constexpr (COL) {
        if (interior) {
          cl = epi.load(m0, n0 + wn * 64 + rcol * 8);
          ch = epi.load(m0, n0 + wn * 64 + rcol * 8 + 4);
        }
      }
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        Map::fill_rows(acc, i, scr, lane);
        HO_LGKM0();
        g256h_stamp<TRACE>(tr, g, wn, lane, 1 + 4 * i);
        f32x4 lo[4], hi[4];
        const int mb = m0 + g * 128 + i * 32 + rrow, n = n0 + wn * 64 + rcol * 8;
#pragma unroll
        for (int ps = 0; ps < 4; ++ps) {
          ho_read8(scr, lane, ps, lo[ps], hi[ps]);
        }
        if constexpr (epi_has_row_aux<Epi>::value) {  // per-row operands of the epilogue (LDS), fetched with the read-back: one wait covers both
          if (COL && interior) {
            f32x2 ra[4];
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) ra[ps] = epi.row_aux(mb + ps * 8);
#ifdef LFM_EXP_WAIT_ALL  // (experiment build) every LDS read of the pass has landed, plus 16 idle cycles, before the first VALU instruction that consumes one
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_nop 7\n\ts_nop 7" ::: "memory");
            __builtin_amdgcn_sched_barrier(0);
#endif
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) epi.store8r(mb + ps * 8, n, lo[ps], hi[ps], cl, ch, ra[ps]);
            HO_LGKM0();
            continue;
          }
        }
        if constexpr (TRACE) {
          HO_LGKM0();
          g256h_stamp<TRACE>(tr, g, wn, lane, 2 + 4 * i);
        }
        if (COL && interior) {
          if constexpr (COL) {
            g256h_stamp<TRACE>(tr, g, wn, lane, 3 + 4 * i);
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) epi.store8(mb + ps * 8, n, lo[ps], hi[ps], cl, ch);
            g256h_stamp<TRACE>(tr, g, wn, lane, 4 + 4 * i);
          }
        } else if (interior) {
          typename Epi::Aux al[4], ah[4];
#pragma unroll
          for (int ps = 0; ps < 4; ++ps) {
            al[ps] = epi.load(mb + ps * 8, n);
            ah[ps] = epi.load(mb + ps * 8, n + 4);
          }
          if constexpr (TRACE) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // (trace build only) the auxiliary loads have returned
            g256h_stamp<TRACE>(tr, g, wn, lane, 3 + 4 * i);
          }
#pragma unroll
          for (int ps = 0; ps < 4; ++ps) epi.store8(mb + ps * 8, n, lo[ps], hi[ps], al[ps], ah[ps]);
          g256h_stamp<TRACE>(tr, g, wn, lane, 4 + 4 * i);
        } else {
#pragma unroll
          for (int ps = 0; ps < 4; ++ps) {
            const int m = mb + ps * 8;
            if (m >= M) continue;
            if (n + 7 < N) epi.store8(m, n, lo[ps], hi[ps], epi.load(m, n), epi.load(m, n + 4));
            else if (n + 3 < N) epi.store(m, n, lo[ps], epi.load(m, n));  // N % 4 == 0: a ragged edge ends on a 4-column boundary
          }
        }
        HO_LGKM0();
      }
      return;
    }
  }
  const int rrow = lane >> 4, rcol = lane & 15;
  typename Epi::Aux cx;
  if constexpr (COL) {
    if (interior) cx = epi.load(m0, n0 + wn * 64 + rcol * 4);
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    Map::fill_rows(acc, i, scr, lane);
    HO_LGKM0();
    g256h_stamp<TRACE>(tr, g, wn, lane, 1 + 4 * i);
    f32x4 v[8];
#pragma unroll
    for (int ps = 0; ps < 8; ++ps) v[ps] = ho_read4(scr, lane, ps);
    if constexpr (TRACE) {
      HO_LGKM0();
      g256h_stamp<TRACE>(tr, g, wn, lane, 2 + 4 * i);
    }
    const int mb = m0 + g * 128 + i * 32 + rrow, n = n0 + wn * 64 + rcol * 4;
    if (COL && interior) {
      if constexpr (COL) {
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) epi.store(mb + ps * 4, n, v[ps], cx);
        g256h_stamp<TRACE>(tr, g, wn, lane, 4 + 4 * i);
      }
    } else if (interior) {
      typename Epi::Aux aux[8];
#pragma unroll
      for (int ps = 0; ps < 8; ++ps) aux[ps] = epi.load(mb + ps * 4, n);
      if constexpr (TRACE) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        g256h_stamp<TRACE>(tr, g, wn, lane, 3 + 4 * i);
      }
#pragma unroll
      for (int ps = 0; ps < 8; ++ps) epi.store(mb + ps * 4, n, v[ps], aux[ps]);
      g256h_stamp<TRACE>(tr, g, wn, lane, 4 + 4 * i);
    } else if (n + 3 < N) {
#pragma unroll
      for (int ps = 0; ps < 8; ++ps)
        if (mb + ps * 4 < M) epi.store(mb + ps * 4, n, v[ps], epi.load(mb + ps * 4, n));
    }
    HO_LGKM0();
  }
}

// ---- the transposed driver: the K loop ran this tile with the MFMA operands swapped, so a lane holds FOUR CONSECUTIVE m of one n.  Same scratch,
// roles exchanged (fill_cols): scratch rows = 32 columns n, scratch columns = 64 rows m; read back row-major, a lane gets 8 (wide: one 16-byte chunk
// of a V^T row) or 4 consecutive m of one n -> epi.store_t8 / store_t.
template <class Map, int BN, bool TRACE = false, class Epi>
__device__ __forceinline__ void ho_transposed(const typename Map::Acc& acc, char* smem, const Epi& epi, int m0, int n0, int M, int N, int g, int wn,
                                              int lane, int wave, int dbg, bool tr) {
  char* scr = ho_slot(smem, wave);
  const bool wide = !(dbg & LFM_DBG_GEMM_STORE8) && epi.wide_t_ok();
  // the per-column constants of every pass, loaded ahead of the first store (a load issued after stores waits for them: vmcnt is in order)
  typedef decltype(epi.load_t(0)) AuxT;  // float (a bias) or (u, v) of the folded path
  AuxT bt[2][4];
  if (wide) {
#pragma unroll
    for (int J = 0; J < 2; ++J)
#pragma unroll
      for (int ps = 0; ps < 4; ++ps) {
        const int n = n0 + wn * 64 + J * 32 + (lane >> 3) + ps * 8;
        bt[J][ps] = n < N ? epi.load_t(n) : AuxT{};
      }
  }
#pragma unroll
  for (int J = 0; J < 2; ++J) {
#pragma unroll
    for (int ih = 0; ih < 2; ++ih) {
      Map::fill_cols(acc, J, ih, scr, lane);
      HO_LGKM0();
      g256h_stamp<TRACE>(tr, g, wn, lane, 1 + 4 * (2 * J + ih));
      if (wide) {
        const int nb = n0 + wn * 64 + J * 32 + (lane >> 3), m = m0 + g * 128 + ih * 64 + ho_ml(lane);
        if (m0 + HO_TILE_ROWS <= M && n0 + BN <= N) {  // interior tile: no per-store bounds checks
          f32x4 lo[4], hi[4];
#pragma unroll
          for (int ps = 0; ps < 4; ++ps) ho_read8_t(scr, lane, ps, lo[ps], hi[ps]);
          if constexpr (TRACE) {
            HO_LGKM0();
            g256h_stamp<TRACE>(tr, g, wn, lane, 2 + 4 * (2 * J + ih));
          }
          if (!(TRACE && (dbg & LFM_DBG_TRACE_NO_STORES))) {  // (trace build: the pass without its stores)
#pragma unroll
            for (int ps = 0; ps < 4; ++ps) epi.store_t8(nb + ps * 8, m, lo[ps], hi[ps], bt[J][ps]);
          }
        } else {
#pragma unroll
          for (int ps = 0; ps < 4; ++ps) {
            f32x4 lo, hi;
            ho_read8_t(scr, lane, ps, lo, hi);
            const int n = nb + ps * 8;
            if (n >= N) continue;
            const AuxT b = bt[J][ps];
            if (m + 11 < M) epi.store_t8(n, m, lo, hi, b);
            else {
              if (m + 3 < M) epi.store_t(n, m, lo, b);
              // (the hi half -- tokens m + 8 .. m + 11 -- lies beyond M here; wide_t_ok() implies M % 16 == 0, so this branch only trims whole tails)
            }
          }
        }
      } else {
        const int nb = n0 + wn * 64 + J * 32 + (lane >> 4), m = m0 + g * 128 + ih * 64 + (lane & 15) * 4;
#pragma unroll
        for (int ps = 0; ps < 8; ++ps) {
          const f32x4 v = ho_read4(scr, lane, ps);
          const int n = nb + ps * 4;
          if (n < N && m + 3 < M) epi.store_t(n, m, v, epi.load_t(n));
        }
      }
      HO_LGKM0();
      g256h_stamp<TRACE>(tr, g, wn, lane, 4 + 4 * (2 * J + ih));
    }
  }
  g256h_stamp<TRACE>(tr, g, wn, lane, 17);
}

// ---- the dispatcher: one 128 x 64 accumulator block through the epilogue `epi` -- transposed tiles, fragment-direct column ranges, tiles that reduce to a
// plainer epilogue, else the row-major driver and the epilogue's finish_tile.  Shared by the 256x128 kernel, the 8-wave 256x256 kernel (one block per
// wave) and the 4-wave one (two blocks per wave).
template <class Map, int BN, bool TRACE = false, class Epi>
__device__ __forceinline__ void ho_block(const typename Map::Acc& acc, char* smem, Epi& epi, int m0, int n0, int M, int N, int g, int wn, int lane,
                                         int wave, int dbg, bool swapped, bool tr = false) {
  if constexpr (epi_has_transposed<Epi>::value) {
    if (swapped) {
      ho_transposed<Map, BN, TRACE>(acc, smem, epi, m0, n0, M, N, g, wn, lane, wave, dbg, tr);
      return;
    }
  }
  if (epi_direct(epi, n0, 0)) {  // epilogues that want the fragment layout: (m, n..n+3) per lane straight from the accumulators
    Map::for_each_frag(acc, lane, [&](int r, int c, f32x4 v) {
      const int m = m0 + g * 128 + r, n = n0 + wn * 64 + c;
      if (m < M && n + 3 < N) epi.store(m, n, v, epi.load(m, n));
    });
    return;
  }
  const bool narrow = (dbg & LFM_DBG_GEMM_STORE8) != 0;  // the 8-byte-store epilogue (A/B)
  if constexpr (epi_has_plain<Epi>::value) {
    if (epi.plain_tile(n0, BN)) {
      auto pe = epi.plain(n0);
      ho_rows<Map, BN, TRACE>(acc, smem, pe, m0, n0, M, N, g, wn, lane, wave, narrow, tr);
      return;
    }
  }
  ho_rows<Map, BN, TRACE>(acc, smem, epi, m0, n0, M, N, g, wn, lane, wave, narrow, tr);
  if constexpr (epi_has_finish_tile<Epi>::value) epi.finish_tile(m0, n0, g, wn, lane);
  g256h_stamp<TRACE>(tr, g, wn, lane, 17);
}

// ---- producer epilogues of the folded LayerNorm-modulate (EpiGateResidMod, gemm_epilogues.h): the gated-residual read-modify-write of X, plus the
// consumer GEMM's A operand A' = fp16((X' - c)(1 + scale)) and this tile's per-row partials (sum X', sum (X' - c)^2).  Interior tiles of ONE image
// only (the host guarantees it).  HoMap16 fill and the 4-column read-back: per pass a lane owns rows rl + 4 ps (ps = 0..7) of the tile, columns
// n .. n + 3; the 16 lanes that share a row are one DPP row, so a row's sums over a 64-column quarter cost four DPP adds each.  The kernels keep
// their own schedule of the X loads and their own wave -> quarter map (gemm256h_kernel.h, gemm256w_kernel.h); the arithmetic is here.
// sum over the 16 lanes of a DPP row (every lane of the row receives it): quad swaps, then two row rotations
__device__ __forceinline__ float ho_row16_sum(float v) {
  v = dpp_add<0xB1>(v);
  v = dpp_add<0x4E>(v);
  v = dpp_add<0x124>(v);
  v = dpp_add<0x128>(v);
  return v;
}
struct HoModCols {  // the column constants of a lane's four columns n .. n + 3
  f32x4 bias, gate, sc1;
  template <class Epi>
  static __device__ __forceinline__ HoModCols load(const Epi& epi, int img, int n) {
    return HoModCols{*(const f32x4*)(epi.bias + n), *(const f32x4*)(epi.gate + (long)img * epi.gate_stride + n),
                     *(const f32x4*)(epi.scale + (long)img * epi.mod_stride + n) + 1.0f};
  }
};
// step ps of a pass: tile row rl + 4 ps (rl = the lane's row at ps = 0), X row already in xo; red_pass = the quarter's partials at the pass's first row
template <class Epi>
__device__ __forceinline__ void ho_mod_row(const Epi& epi, const char* scr, int lane, int ps, f32x4 xo, const float* cen_s, const HoModCols& k, int m0,
                                           int rl, int n, int N, float* red_pass) {
  const f32x4 v = ho_read4(scr, lane, ps);
  const float c = cen_s[rl + ps * 4];
  const f32x4 xn = xo + k.gate * (v + k.bias);
  *(f32x4*)(epi.X + (long)(m0 + rl + ps * 4) * epi.ldx + n) = xn;
  const f32x4 d = xn - c;
  const f32x4 ap = d * k.sc1;
  *(half4_t*)(epi.A + (long)(m0 + rl + ps * 4) * N + n) = f16x4(ap);
  const float sx = ho_row16_sum((xn.x + xn.y) + (xn.z + xn.w));
  const float sq = ho_row16_sum((d.x * d.x + d.y * d.y) + (d.z * d.z + d.w * d.w));
  if ((lane & 15) == 0) {
    float* dst = red_pass + (ps * 4 + (lane >> 4)) * 2;
    dst[0] = sx;
    dst[1] = sq;
  }
}
__device__ __forceinline__ float* ho_red_pass(char* smem, int g, int quarter, int i) { return (float*)(smem + HO_RED_OFF) + ((g * 4 + quarter) * 128 + i * 32) * 2; }
// tile-level row sums of the 128-row half g (fixed order over the four column quarters) -> this tile's slot of the rows' partials; one wave per half
template <class Epi>
__device__ __forceinline__ void ho_mod_tile_sums(const Epi& epi, const char* smem, int g, int lane, int m0, int tile_n) {
  const float* red = (const float*)(smem + HO_RED_OFF);
#pragma unroll
  for (int rr = 0; rr < 2; ++rr) {
    const int r = lane + 64 * rr;
    float sx = 0.f, sq = 0.f;
#pragma unroll
    for (int w4 = 0; w4 < 4; ++w4) {
      sx += red[((g * 4 + w4) * 128 + r) * 2];
      sq += red[((g * 4 + w4) * 128 + r) * 2 + 1];
    }
    *(f32x2*)(epi.part + ((long)(m0 + g * 128 + r) * epi.tiles_n + tile_n) * 2) = (f32x2){sx, sq};
  }
}
