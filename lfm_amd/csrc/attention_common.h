// What the four MFMA attention kernels of the DiT side share (attention_kernel.h: one workgroup per item; attention_stream_kernel.h: persistent, streamed;
// attention_tiled_kernel.h: any token count, 128 queries per workgroup; qkv_attention_kernel.h: fused with the QKV projection).  Every piece of the arithmetic is ONE
// text here, so the four are bit-identical per query: att_load_q (Q fragments), att_qk_block (S^T = K Q^T), att_softmax_block (online softmax), att_pv_block
// (O^T += V^T P^T), att_normalised (O / l as fp16 pieces) and the two output staging layouts (att_ostage_*: padded rows, att_oswz_*: swizzled rows).  Where an
// operand lies in the LDS, when it is there (DMA issue, rings, counted waits, barriers) and in which order the blocks are issued stays with each kernel: a kernel
// hands its addresses in as a functor, which folds away once inlined.  Also here: the counted-wait / barrier macros and the trace stamps of the measurement variants.
#pragma once
#include "gemm_kernel.h"

#define ATS_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define ATS_BARRIER()                              \
  do {                                             \
    __builtin_amdgcn_s_barrier();                  \
    asm volatile("" ::: "memory");                 \
  } while (0)

// Operand mapping (v_mfma_f32_32x32x16_f16, hsel = lane >> 5, l31 = lane & 31): S^T = K Q^T -- the A operand is K row (lane & 31) of the 32-key block, the B operand
// Q row (lane & 31), both dims 16 ks + 8 hsel .. + 7 -- so a lane then holds, for ONE query, the scores of keys 8 g + 4 hsel + r of the block in register 4 g + r.
// hd 72 = 4.5 k-slots: the fifth slot's upper half (dims 72 .. 79) does not exist and is fed ZEROS on both operands (LDS past a row end is another row or stale
// bytes, possibly NaN patterns); its lanes read chunk 2 ks like the lower half (att_k_chunk), never past the row.
template <int HD>
__device__ __forceinline__ constexpr bool att_half_slot(int ks) { return ks * 16 + 16 > HD; }
// 16-byte chunk of a K / Q row that holds the lane's fragment of k-slot ks
template <int HD>
__device__ __forceinline__ int att_k_chunk(int ks, int hsel) { return att_half_slot<HD>(ks) ? ks * 2 : ks * 2 + hsel; }
// Q row qp (global memory) as the B operand of every k-slot
template <int HD>
__device__ __forceinline__ void att_load_q(half8_t (&qf)[(HD + 15) / 16], const half_t* qp, int hsel) {
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int ks = 0; ks < (HD + 15) / 16; ++ks) {
    if (!att_half_slot<HD>(ks)) qf[ks] = *(const half8_t*)(qp + ks * 16 + hsel * 8);
    else qf[ks] = hsel ? zero8 : *(const half8_t*)(qp + ks * 16);
  }
}
// One 32-key block of S^T for JQ blocks of 32 queries (every K fragment feeds JQ MFMAs; the first MFMA takes a shared all-zero C: no accumulator clears).
// kfrag(ks) = the lane's 16-byte K fragment of k-slot ks in the kernel's LDS image.  S: JQ accumulators, qf: [JQ][KS] (a kernel with one query block passes &S, &qf).
template <int HD, int JQ, class KF>
__device__ __forceinline__ void att_qk_block(f32x16* S, const half8_t (*qf)[(HD + 15) / 16], int hsel, KF&& kfrag) {
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  f32x16 zero16;
#pragma unroll
  for (int e = 0; e < 16; ++e) zero16[e] = 0.f;
#pragma unroll
  for (int ks = 0; ks < (HD + 15) / 16; ++ks) {
    half8_t kf = *(const half8_t*)kfrag(ks);
    if (att_half_slot<HD>(ks)) kf = hsel ? zero8 : kf;
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq) S[jq] = __builtin_amdgcn_mfma_f32_32x32x16_f16(kf, qf[jq][ks], ks == 0 ? zero16 : S[jq], 0, 0, 0);
  }
}
// O^T[d][q] += sum_key V^T[d][key] P[q][key] for the block whose packed P (k-slots 0 and 1) att_softmax_block returned: the A operand of k-slot s is V^T row
// att_v_row(db, l31) at the block's keys {4 hsel + r} and {8 + 4 hsel + r} of the slot's 16 -- ONE 16-byte chunk of the row in the vt_pos token order (gemm_epilogues.h),
// chunk 2 s + hsel of the block.  vfrag(s, db) = that chunk in the kernel's LDS image.  Oa: [JQ][NDB], P: [JQ][2].
template <int NDB, int JQ, class VF>
__device__ __forceinline__ void att_pv_block(f32x16 (*Oa)[NDB], const half8_t (*P)[2], VF&& vfrag) {
#pragma unroll
  for (int s = 0; s < 2; ++s)
#pragma unroll
    for (int db = 0; db < NDB; ++db) {
      const half8_t vf = *(const half8_t*)vfrag(s, db);
#pragma unroll
      for (int jq = 0; jq < JQ; ++jq) Oa[jq][db] = __builtin_amdgcn_mfma_f32_32x32x16_f16(vf, P[jq][s], Oa[jq][db], 0, 0, 0);
    }
}
// V^T row of the lane in 32-row block db: rows past HD (third block of hd 72) re-read row HD - 1 -- finite values into accumulator rows nobody stores
template <int HD>
__device__ __forceinline__ int att_v_row(int db, int l31) {
  return (db * 32 + 32 <= HD) ? db * 32 + l31 : (db * 32 + l31 < HD ? db * 32 + l31 : HD - 1);
}

// One 32-key block of the online softmax for the query a lane owns (S: its 16 scores of the block, the other 16 live in lane ^ 32), shared by all
// four kernels (same arithmetic in the same order => bit-identical results whichever kernel evaluates an item).  Round 6: the key loop is bound by instruction
// ISSUE, not by a pipe -- per SIMD, whether it holds two or four waves, one 32-key block of one wave goes through in ~850 cycles while its 8 MFMAs occupy the matrix
// pipe for 256 and ~5 single-issue instructions hide under each of them (profiles/r06_attention_stream.txt) -- so the block is written for instruction count:
//   * OPTIMISTIC exponentials: p = 2^((s - mrun) scale) is taken against the running reference mrun WITHOUT first looking for the block's maximum; the lane's own sum of
//     its 16 p (needed anyway) tells whether that was safe -- every p <= sum <= 2^14 stays far inside fp16 (P is the fp16 operand of the P V MFMA; row sums and O are
//     fp32).  Only when some lane's sum exceeds 2^14 (or is not a number), and for the first block of an item, the block takes the FULL path: row maximum (3-input
//     maxima + one lane ^ 32 exchange), mrun <- max, O and l rescaled by 2^((old - new) scale), exponentials again.  The reference follows the maximum lazily, as
//     before (rounds 3-5 moved it when the maximum had grown by more than 2^8); fp16 rounds P relative to its size, so the result does not depend on where in
//     [2^-14 .. 2^14] the block's largest p lands.
//   * row sum as a TREE of packed adds (8 issue slots; the serial chain of rounds 1-5 drew a wait state per link: 18).
// `first` is wave-uniform.  Returns the packed P of the block (k-slots 0 and 1) in P.
template <int NDB>
__device__ __forceinline__ void att_softmax_block(const f32x16& S, bool first, float& mrun, float& lrun, f32x16 (&Oa)[NDB], float scale_log2e, half8_t (&P)[2]) {
  f32x2 p[8];
  const f32x2 sc2 = {scale_log2e, scale_log2e};
  auto expo = [&]() {
    const float mbs = mrun * scale_log2e;
    const f32x2 nmb2 = {-mbs, -mbs};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const f32x2 s2 = {S[2 * e], S[2 * e + 1]};
      const f32x2 a2 = __builtin_elementwise_fma(s2, sc2, nmb2);  // ONE fused multiply-add on every path and in every kernel that inlines this (v_pk_fma_f32 / v_fma_f32)
      p[e] = (f32x2){__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
    }
  };
  auto lane_sum = [&]() {
    const f32x2 t = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));  // v_pk_add_f32 x 7
    return t.x + t.y;
  };
  float ls = 0.f;
  bool full = first;
  if (!first) {
    expo();
    ls = lane_sum();
    full = !__all(ls <= 16384.0f);
  }
  if (full) {  // wave-uniform
    float mx = fmaxf(fmaxf(S[0], S[1]), S[2]);
#pragma unroll
    for (int e = 3; e < 15; e += 2) mx = fmaxf(fmaxf(mx, S[e]), S[e + 1]);
    mx = fmaxf(mx, S[15]);
    mx = fmaxf(mx, xhalf(mx));
    const float mnew = fmaxf(mrun, mx);
    const float alpha = __builtin_amdgcn_exp2f((mrun - mnew) * scale_log2e);
    mrun = mnew;
    lrun *= alpha;
#pragma unroll
    for (int db = 0; db < NDB; ++db) Oa[db] *= alpha;
    expo();
    ls = lane_sum();
  }
  lrun += ls;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    P[e >> 2][(e & 3) * 2] = (half_t)p[e].x;
    P[e >> 2][(e & 3) * 2 + 1] = (half_t)p[e].y;
  }
}

// Normalise: the lane owns one query and holds O^T rows d = 32 db + 8 g + 4 hsel + r in Oa[db][4 g + r]; l is the lane's row sum plus lane ^ 32's (att_inv_l: every
// lane of the wave calls it).  sink(db, g, h) places the four fp16 values of rows 32 db + 8 g + 4 hsel .. + 3 (HD % 8 == 0: an 8-row group is live or dead as a
// whole; dead ones are skipped).
__device__ __forceinline__ float att_inv_l(float lrun) { return 1.0f / (lrun + xhalf(lrun)); }
template <int HD, class SINK>
__device__ __forceinline__ void att_normalised(const f32x16 (&Oa)[(HD + 31) / 32], float inv, SINK&& sink) {
#pragma unroll
  for (int db = 0; db < (HD + 31) / 32; ++db)
#pragma unroll
    for (int g = 0; g < 4; ++g) {
      if (db * 32 + 8 * g >= HD) continue;
      const half4_t h = {(half_t)(Oa[db][4 * g] * inv), (half_t)(Oa[db][4 * g + 1] * inv), (half_t)(Oa[db][4 * g + 2] * inv), (half_t)(Oa[db][4 * g + 3] * inv)};
      sink(db, g, h);
    }
}
// Output staging: O rows leave through the LDS (K / V^T are dead by then) so that a store instruction covers whole 16-byte chunks of whole rows instead of 64
// scattered 8-byte pieces.  Both layouts are wave-private: between a wave's writes and its reads stands `s_waitcnt lgkmcnt(0)` (asm: also the compiler barrier), no s_barrier.
// (a) padded rows, any HD: row r of the wave at r * ATT_OSTR (HD * 2 bytes of data; the 36- / 40-dword stride keeps the 16 lanes of a ds_write_b64 group on distinct banks)
template <int HD>
static constexpr int ATT_OSTR = HD * 2 + 16;
template <int HD>
__device__ __forceinline__ void att_ostage_put(char* ob, int row, int hsel, int db, int g, half4_t h) {
  *(half4_t*)(ob + row * ATT_OSTR<HD> + (db * 32 + 8 * g + 4 * hsel) * 2) = h;
}
// ... and the ROWS staged rows out to obase (row stride D halves), the first `live` of them
template <int HD, int ROWS>
__device__ __forceinline__ void att_ostage_store(const char* ob, half_t* obase, int D, int lane, int live) {
  constexpr int KCH = HD / 8, OCH = ROWS * KCH;  // 16-byte chunks per row / of all rows
#pragma unroll
  for (int i = 0; i < (OCH + 63) / 64; ++i) {
    const int c = i * 64 + lane, row = c / KCH, ch = c - row * KCH;
    if ((OCH % 64 == 0 || c < OCH) && row < live) {
      const half8_t v = *(const half8_t*)(ob + row * ATT_OSTR<HD> + ch * 16);
      *(half8_t*)(obase + (long)row * D + ch * 8) = v;
    }
  }
}
// (b) hd 64, 128-byte rows without padding: 8-byte position p of staged row r at p ^ ((r & 7) << 1).  att_oswz_put = byte offset of the lane's piece (db, g) of row r;
// att_oswz_get = byte offset of the lane's 16-byte read inside a pass of eight rows (row lane >> 3, chunk lane & 7): a store instruction covers eight whole rows.
__device__ __forceinline__ unsigned att_oswz_put(int row, int hsel, int db, int g) {
  return (unsigned)(row * 128) + ((((unsigned)(db * 8 + 2 * g + hsel)) ^ (unsigned)((row & 7) << 1)) << 3);
}
__device__ __forceinline__ unsigned att_oswz_get(int lane) {
  const int orow = lane >> 3, och = lane & 7;
  return (unsigned)(orow * 128 + ((och ^ orow) << 4));
}

// s_memtime stamps of the measurement variants (MODE 3 of the per-item and the streamed kernel, flag QKV_TRACE of the fused one; the slot maps are next to each
// kernel), read back with lfm_attention_trace_read / lfm_attention_wg_trace_read
#define ATT_TRACE_SLOTS 64
#define ATT_WG_TRACE 2048
static __device__ unsigned long long att_trace[ATT_TRACE_SLOTS];
static __device__ unsigned long long att_wg_trace[ATT_WG_TRACE][4];
// One stamp: the calling wave's lane 0 writes s_memtime to att_trace[idx].  Which wave of which workgroup stamps which slot is the kernel's (behind its
// `if constexpr (MODE == 3)` / `#ifdef LFM_MEASURE`: a product build holds no trace code).
__device__ __forceinline__ unsigned long long att_memtime() {
  unsigned long long t;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t)::"memory");
  return t;
}
__device__ __forceinline__ void att_stamp(int idx, int lane) {
  const unsigned long long t = att_memtime();
  if (lane == 0) att_trace[idx] = t;
}
// Per-workgroup record att_wg_trace[wg] = {HW_ID | XCC_ID << 32, stamp 0, stamp 1, stamp 2}: which CU the workgroup ran on and when
__device__ __forceinline__ void att_wg_stamp(int wg, int slot, int lane) {
  if (wg >= ATT_WG_TRACE) return;
  const unsigned long long t = att_memtime();
  if (slot == 0) {
    const unsigned hw = __builtin_amdgcn_s_getreg((31 << 11) | 4), xcc = __builtin_amdgcn_s_getreg((31 << 11) | 20);
    if (lane == 0) att_wg_trace[wg][0] = (unsigned long long)hw | ((unsigned long long)xcc << 32);
  }
  if (lane == 0) att_wg_trace[wg][slot + 1] = t;
}
