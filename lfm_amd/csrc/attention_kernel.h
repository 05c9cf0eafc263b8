// Attention core of a DiT block (timm Attention as called at /root/reference/models/DiT.py:120): O = softmax(Q K^T * hd^-0.5) V
// per (image, head), head_dim HD = 64 (DiT-S / B / L) or 72 (DiT-XL: 1152 / 16).
//
// One workgroup per (head, image); T / (32 JQ) waves, each owning JQ blocks of 32 queries (processed together so every K / V^T
// fragment read from LDS feeds JQ MFMAs).
// K [T][HD] and V^T [HD][T] of the head are staged once into LDS by LDS-DMA.  K rows are HD * 2 bytes: 128-B rows (hd 64) are
// XOR-swizzled at the DMA source (chunk' = chunk ^ ((row>>1)&7)); 144-B rows (hd 72) need no swizzle -- 36 dwords per row put 16
// consecutive rows on 16 disjoint groups of four banks.  V^T rows (2T bytes) are swizzled by row (chunk' = chunk ^ (row & VKEY)).
// The arithmetic is attention_common.h's, one text for all four MFMA kernels: S^T = K Q^T on v_mfma_f32_32x32x16_f16 (att_qk_block: a lane then holds the scores
// of ONE query, so row max / row sum are in-lane plus one lane^32 exchange, and the fp32->fp16 packed P registers are directly the B-operand of O^T = V^T P^T,
// att_pv_block: the key order inside an MFMA k-slot is the same permutation on both operands, so no shuffle is needed), the zero-fed half k-slot of hd 72
// (O^T has 2.25 blocks of 32 rows: the third block computes 8 live rows), V^T rows in the vt_pos token order (gemm_epilogues.h), which makes a lane's P V operand
// one 16-byte read.  This file owns the LDS image, the staging and the schedule.
// Keys are consumed in 32-key blocks with an online softmax (running max m, running sum l), which keeps
// the live state at S 32 + P 16 + O 64 + Q 32 registers for hd 64, JQ 2 (2 waves / SIMD).
#pragma once
#include "attention_common.h"

// MODE 3 (measurement only): s_memtime stamps of wave 0 of the first workgroup (slots 0..31) and of the last one (32..63), read back with
// lfm_attention_trace_read.  Slots: 0 start, 1 all DMAs / Q loads issued, 2 K and Q landed (first barrier), 3 + 4 k + {0: S(next) issued,
// 1: softmax + PV of the even block done, 2: S(next even) issued, 3: softmax + PV of the odd block done} for the k-th loop iteration,
// 19 stores issued, 20 stores acknowledged; inside the first softmax_pv: 21 softmax VALU done, 22 V^T landed (barrier), 23 PV MFMAs issued.
// MODE 3 also records, per workgroup (linear id < 2048): {HW_ID | XCC_ID << 32, start, loads landed, end} -- which CU it ran on and when

// MODE (measurement only, tools/r2_probe3.py): 0 = the kernel; 1 = memory phases only (stage K / V^T, fetch Q, store a row per query, no
// S / softmax / PV); 2 = compute only (K / V^T are never fetched: the loop runs on whatever the LDS holds).  Round 2, 64 images x 16 heads x 256
// tokens (profiles/r02_probe3_attention_phases_ln_rows.txt): whole kernel 40-41 us, memory phases 22-23 us, compute (with its Q / O traffic) 33-36 us
// -- the kernel is bound by the instruction stream of its two waves per SIMD, and the memory phases already hide behind the co-resident workgroup.
// Round 3 (profiles/r03_attention_*.txt): the per-workgroup timeline (MODE 3: HW_ID + s_memtime per workgroup) shows every CU holding two workgroups
// that de-phase by themselves (the second of a pair lags by ~14k cycles), a workgroup living ~33k cycles of which the loads take ~11k, the key-block
// loop ~15.5k and the store drain ~5k: the kernel is bound by memory LATENCY at an occupancy of two workgroups per CU (64 KiB of LDS each), not by
// its instruction streams.  Measured and not kept: sleeping one workgroup of every first-round pair (37.7-43 us vs 38.5), and a one-basic-block
// step with sched_group_barrier interleaving every MFMA with the VALU that covers its 32 pipe cycles (ISA as prescribed, 40.4 vs 39.5 us) -- the
// partner wave already fills those gaps.  Kept: the lazy rescale (below).
// Measured and NOT kept on that evidence (round 2): a streamed schedule (DMAs issued key block by key block, V^T slices as 64-byte pieces, the online-softmax
// loop started after block 0 behind one counted vmcnt + barrier per block): correct, 40.8-41.7 us vs 40.1-42.8 us.
// (Round 4, tried and dropped: the row maxima as inline-asm v_max3_f32 to skip the few canonicalising v_max_f32 x, x that IEEE fmaxf puts in front of MFMA
// results -- the compiler's hazard recogniser does not see an asm reading MFMA accumulators, and the hd-72 runs stopped being bit-repeatable.)
// NCH > 1 (round 4: DiT at 1024 tokens, models/DiT.py:179-182 with --image_size 512): the sequence has NCH * T tokens.  A workgroup owns T QUERIES
// (blockIdx.z = which block of T) and walks the keys in NCH chunks of T through the same LDS image -- the online softmax state carries over; a chunk
// is re-staged behind a barrier (no cross-chunk prefetch: this shape is off the benchmarked path).
// QS > 1 (round 5, latency mode: one image = `heads` workgroups for 256 CUs): the queries of an (image, head) item are split over QS workgroups (blockIdx.z) that
// each stage ALL keys; T / (32 JQ QS) waves, one per SIMD instead of two for QS = 2 -- the softmax VALU stream of a wave no longer shares its SIMD.  Same
// arithmetic per query, same key order: bit-identical to QS = 1 (tests/test_gpu_dit.py::test_attention_query_split_matches).
template <int T, int JQ, int HD, int MODE = 0, int NCH = 1, int QS = 1>
__global__ __launch_bounds__((T / (32 * JQ * QS)) * 64, HD == 64 && QS == 1 ? (T / (32 * JQ)) / 2 : 2) void dit_attention_kernel(
    const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ Vt, half_t* __restrict__ O, int D, int heads,
    float scale_log2e, int stag) {
  constexpr int TT = T * NCH;  // tokens of the sequence
#ifdef LFM_MEASURE
  if (stag > 0) {  // measurement (tools/stagger_probe.py): the second residents of the first wave of workgroups start late
    const int lin = blockIdx.x + blockIdx.y * gridDim.x;
    if (lin >= 256 && lin < 512) {
      const unsigned long long t0 = __builtin_amdgcn_s_memtime();
      while ((long long)(__builtin_amdgcn_s_memtime() - t0) < (long long)stag) __builtin_amdgcn_s_sleep(16);
    }
  }
#endif
  static_assert(NCH == 1 || MODE == 0, "measurement variants are single-chunk");
  static_assert(QS == 1 || (NCH == 1 && MODE == 0 && T % (32 * JQ * QS) == 0), "the query split is for the single-chunk product kernel");
  static_assert(HD % 8 == 0 && HD >= 32 && HD <= 128, "head_dim: whole 16-byte chunks");
  constexpr int NKB = T / 32;         // 32-key blocks
  constexpr int NW = T / (32 * JQ * QS);  // waves: each owns JQ blocks of 32 queries
  constexpr int NTHR = NW * 64;
  constexpr int KS = (HD + 15) / 16;  // k-slots of the S MFMAs (the last one half empty when HD % 16 == 8)
  constexpr int NDB = (HD + 31) / 32; // 32-row blocks of O^T
  constexpr int KCH = HD / 8;         // 16-B chunks per K row
  constexpr int KROW = KCH * 16;      // bytes per K row in LDS
  constexpr bool KSWZ = HD == 64;     // 128-B rows: XOR swizzle; rows of an odd number of chunks are conflict-free as they are
  constexpr int VKEY = (T / 8 - 1) < 15 ? (T / 8 - 1) : 15;  // V^T swizzle key mask (stays inside the row)
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* Ks = smem;             // [T][HD] halves
  char* Vs = smem + T * KROW;  // [HD][T] halves, 2T-B rows
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int head = blockIdx.x, img = blockIdx.y;
  const bool tr_first = blockIdx.x == 0 && blockIdx.y == 0, tr_last = blockIdx.x == gridDim.x - 1 && blockIdx.y == gridDim.y - 1;
  auto stamp = [&](int slot) {
    if constexpr (MODE == 3)
      if (wave == 0 && (tr_first || tr_last)) att_stamp((tr_first ? 0 : 32) + slot, lane);
  };
  stamp(0);
  auto wg_stamp = [&](int slot) {
    if constexpr (MODE == 3)
      if (wave == 0) att_wg_stamp(blockIdx.y * gridDim.x + blockIdx.x, slot, lane);
  };
  wg_stamp(0);
  const int qblk = NCH > 1 ? (int)blockIdx.z : 0;
  const half_t* Kg = K + (long)img * TT * D + head * HD;
  const half_t* Vg = Vt + ((long)img * heads + head) * HD * TT;
  // buffer-addressed LDS-DMA (SGPR resource + 32-bit VGPR byte offset: +13 % LDS-DMA throughput per CU over 64-bit VGPR addresses,
  // tools/ubench/ldsdma_rate.hip -- the load phase is a third of a workgroup's life)
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)Kg, 0, -1, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)Vg, 0, -1, 0x00020000);

  // ---- stage K, fetch this wave's Q fragments, then stage V^T.  Issue order = completion order for loads, so
  // vmcnt(VMIN) below means "K and Q are here, V^T may still be flying"; V^T is awaited before the first PV.
  // T * HD / 8 slots of 16 B over NTHR lanes: 8 or 4 full passes for hd 64, 4.5 for hd 72 (the last pass is issued by the lower
  // half of the waves only: whole waves, so the DMA's implicit lane*16 destination stays dense).
  constexpr int SLOTS = T * KCH;
  constexpr int NPASS = (SLOTS + NTHR - 1) / NTHR;
  constexpr int VMIN = SLOTS / NTHR;  // V^T DMAs every wave issues
  static_assert(VMIN == 8 || VMIN == 4, "the counted wait below is vmcnt(VMIN)");
  static_assert(SLOTS % NTHR == 0 || (SLOTS % NTHR) % 64 == 0, "a partial pass is made of whole waves");
  // (the chunk loop of the hd-64 kernel passes a laundered copy of tid: the 2 * NPASS per-lane offsets and LDS destinations are recomputed at every re-stage
  // instead of living -- spilled, 19 dwords under the 128-VGPR budget of two workgroups per CU -- across the key-block loop: 8 x 16 x 1024 x 64 59-62 -> 53-55 us,
  // tools/attn_1024_time.py; the NCH = 1 kernels issue both stages once, before anything else is live)
  auto stage_k = [&](int chunk, unsigned tid_) {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const unsigned s = p * NTHR + tid_, wave_ = tid_ >> 6;
      if (SLOTS % NTHR == 0 || p + 1 < NPASS || s < SLOTS) {
        const int row = s / KCH, ch = s - row * KCH;
        const int c = KSWZ ? (ch ^ ((row >> 1) & 7)) : ch;
        if (MODE != 2) glds16_buf(rs_k, (unsigned)((chunk * T + row) * D + c * 8) * 2u, 0u, Ks + (p * NTHR + wave_ * 64) * 16);
      }
    }
  };
  auto stage_v = [&](int chunk, unsigned tid_) {
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const unsigned s = p * NTHR + tid_, wave_ = tid_ >> 6;
      if (SLOTS % NTHR == 0 || p + 1 < NPASS || s < SLOTS) {
        constexpr int CPR = T / 8;  // 16-B chunks per V^T row of the staged key chunk
        const int row = s / CPR, c = (s % CPR) ^ (row & VKEY);
        if (MODE != 2) glds16_buf(rs_v, (unsigned)(row * TT + chunk * T + c * 8) * 2u, 0u, Vs + (p * NTHR + wave_ * 64) * 16);
      }
    }
  };
  stage_k(0, tid);
  const int q0 = ((QS > 1 ? (int)blockIdx.z * NW : 0) + wave) * 32 * JQ;
  const int hsel = lane >> 5, l31 = lane & 31;
  half8_t qf[JQ][KS];
#pragma unroll
  for (int jq = 0; jq < JQ; ++jq) att_load_q<HD>(qf[jq], Q + ((long)img * TT + qblk * T + q0 + jq * 32 + l31) * D + head * HD, hsel);
  stage_v(0, tid);

  if constexpr (MODE == 1) {  // everything has landed -> one output row per query, straight from the Q registers
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq)
#pragma unroll
      for (int ks = 0; ks < HD / 16; ++ks)
        *(half8_t*)(O + ((long)img * TT + qblk * T + q0 + jq * 32 + l31) * D + head * HD + ks * 16 + hsel * 8) = qf[jq][ks];
    return;
  }
  stamp(1);
  f32x16 Oa[JQ][NDB];  // [jq][db]
#pragma unroll
  for (int jq = 0; jq < JQ; ++jq)
#pragma unroll
    for (int db = 0; db < NDB; ++db)
#pragma unroll
      for (int e = 0; e < 16; ++e) Oa[jq][db][e] = 0.f;
  float mrun[JQ], lrun[JQ];
#pragma unroll
  for (int jq = 0; jq < JQ; ++jq) {
    mrun[jq] = -3.0e38f;
    lrun[jq] = 0.f;
  }

  if (VMIN == 8) asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
  else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
  __builtin_amdgcn_s_barrier();  // raw barrier: __syncthreads() would drain the in-flight V^T DMAs
  asm volatile("" ::: "memory");
  stamp(2);
  wg_stamp(1);

  // S^T block kb: 32 keys x 32 JQ queries (att_qk_block, attention_common.h)
  auto qk = [&](f32x16 (&S)[JQ], int kb) {
    const int row = kb * 32 + l31;
    const int key = KSWZ ? ((row >> 1) & 7) : 0;
    const char* kp = Ks + row * KROW;
    att_qk_block<HD, JQ>(S, qf, hsel, [&](int ks) { return kp + ((att_k_chunk<HD>(ks, hsel) ^ key) << 4); });
  };
  // online softmax update for the queries this lane owns, then O^T[d][q] += sum_key V^T[d][key] P[q][key].
  // VALU diet (the kernel is VALU-issue-bound: ~1.9k VALU per wave vs 128 MFMAs): 3-input max, packed fp32 FMA / ADD on
  // register pairs, one v_permlane32_swap instead of a ds_bpermute round trip for the lane^32 exchange.
  bool first_chunk = true;
  auto softmax_pv = [&](f32x16 (&S)[JQ], int kb) {
    half8_t P[JQ][2];
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq)  // attention_common.h: optimistic exponentials against the running reference, full path for the first block / on overflow risk
      att_softmax_block<NDB>(S[jq], kb == 0 && first_chunk, mrun[jq], lrun[jq], Oa[jq], scale_log2e, P[jq]);
    if (kb == 0 && first_chunk) {  // V^T was issued after K and Q: only now must it have landed (every wave's share)
      stamp(21);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      stamp(22);
    }
    att_pv_block<NDB, JQ>(Oa, P, [&](int s, int db) {  // chunk 4 kb + 2 s + hsel of the lane's V^T row
      const int d = att_v_row<HD>(db, l31);
      return Vs + d * (2 * T) + (((kb * 4 + 2 * s + hsel) ^ (d & VKEY)) << 4);
    });
    if (kb == 0) stamp(23);
  };
  // software pipeline over the key blocks: the S MFMAs of block kb+1 are issued BEFORE the softmax VALU of block kb, so
  // the matrix pipe works underneath the VALU-heavy part instead of the wave idling on the MFMA -> max -> exp -> MFMA chain
  f32x16 Sa[JQ], Sb[JQ];
#pragma unroll 1
  for (int chunk = 0; chunk < NCH; ++chunk) {
    if (NCH > 1 && chunk > 0) {  // every wave is done with the previous chunk of keys: stage the next one, wait for all of it
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      unsigned tid_l = threadIdx.x;
      if constexpr (HD == 64) asm volatile("" : "+v"(tid_l));  // hd 72 runs one workgroup per CU under 256 VGPRs: hoisted offsets cost nothing there
      stage_k(chunk, tid_l);
      stage_v(chunk, tid_l);
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();
      asm volatile("" ::: "memory");
      first_chunk = false;
    }
    qk(Sa, 0);
#pragma unroll 1
    for (int kb = 0; kb < NKB; kb += 2) {
      qk(Sb, kb + 1);
      stamp(3 + 2 * kb);
      softmax_pv(Sa, kb);
      stamp(4 + 2 * kb);
      if (kb + 2 < NKB) qk(Sa, kb + 2);
      stamp(5 + 2 * kb);
      softmax_pv(Sb, kb + 1);
      stamp(6 + 2 * kb);
    }
  }
  // ---- normalise and store (att_normalised, attention_common.h)
  if constexpr (HD == 64 && MODE == 0) {
    // Round 4: through the LDS (K / V^T are dead) so that a store instruction covers eight whole 128-byte output rows instead of 64 scattered 8-byte
    // pieces (the store drain was ~5k of a workgroup's ~33k cycles, profiles/r03_attention_wg_timeline.txt; MI355X guide T21).  Per-wave region of
    // 32 JQ padded rows (att_ostage_*, attention_common.h).
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // every wave has finished reading K / V^T
    asm volatile("" ::: "memory");
    unsigned tid_l = threadIdx.x;  // laundered: the staging addresses are functions of the thread id that the compiler would otherwise compute up front and keep
    asm volatile("" : "+v"(tid_l));  // -- spilled, in the chunked kernel -- across the key loop
    const int ln = tid_l & 63;
    char* ob = smem + (tid_l >> 6) * (32 * JQ * ATT_OSTR<HD>);
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq)
      att_normalised<HD>(Oa[jq], att_inv_l(lrun[jq]), [&](int db, int g, half4_t h) { att_ostage_put<HD>(ob, jq * 32 + (ln & 31), ln >> 5, db, g, h); });
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private region: no barrier
    att_ostage_store<HD, 32 * JQ>(ob, O + ((long)img * TT + qblk * T + q0) * D + head * HD, D, ln, 32 * JQ);
    stamp(19);
    return;
  }
#pragma unroll
  for (int jq = 0; jq < JQ; ++jq) {  // straight from the registers, 8-byte pieces
    half_t* orow = O + ((long)img * TT + qblk * T + q0 + jq * 32 + l31) * D + head * HD;
    att_normalised<HD>(Oa[jq], att_inv_l(lrun[jq]), [&](int db, int g, half4_t h) { *(half4_t*)(orow + db * 32 + 8 * g + 4 * hsel) = h; });
  }
  stamp(19);
  if constexpr (MODE == 3) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    stamp(20);
    wg_stamp(2);
  }
}

// 16 tokens (the DiT-x/8 family on 32x32 latents, models/DiT.py:362-415): 256 scores per (image, head) -- no MFMA tile to fill, and
// 16 rows of hd halves are served by the L1/L2 as they are.  One lane per query, four (image, head) items per wave; the lanes of an item
// read the same K row / V^T row at the same time (one broadcast fetch).  Same arithmetic as the tiled kernel: fp32 scores, exp2 of the
// scaled difference to the row maximum, P rounded to fp16 before P V, the row sum taken from the unrounded values, fp32 accumulation.
template <int HD>
__global__ __launch_bounds__(64) void dit_attention_t16_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ Vt,
                                                               half_t* __restrict__ O, int D, int heads, int items, float scale_log2e) {
  constexpr int T = 16, NC = HD / 8;
  const int item = blockIdx.x * 4 + (threadIdx.x >> 4), q = threadIdx.x & 15;
  if (item >= items) return;
  const int img = item / heads, head = item - img * heads;
  const half_t* qp = Q + ((long)img * T + q) * D + head * HD;
  const half_t* kp = K + (long)img * T * D + head * HD;
  const half_t* vp = Vt + ((long)img * heads + head) * HD * T;
  half8_t qf[NC];
#pragma unroll
  for (int c = 0; c < NC; ++c) qf[c] = *(const half8_t*)(qp + c * 8);
  float s[T];
  float mx = -3.0e38f;
#pragma unroll
  for (int k = 0; k < T; ++k) {
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
      const half8_t kf = *(const half8_t*)(kp + (long)k * D + c * 8);
#pragma unroll
      for (int e = 0; e < 8; ++e) acc += (float)qf[c][e] * (float)kf[e];
    }
    s[k] = acc;
    mx = fmaxf(mx, acc);
  }
  float l = 0.f;
  half_t ph[T];
#pragma unroll
  for (int k = 0; k < T; ++k) {
    const float p = __builtin_amdgcn_exp2f((s[k] - mx) * scale_log2e);
    l += p;
    ph[k] = (half_t)p;
  }
  const float inv = 1.0f / l;
  half_t* op = O + ((long)img * T + q) * D + head * HD;
#pragma unroll
  for (int c = 0; c < NC; ++c) {
    half8_t o8;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const half8_t v0 = *(const half8_t*)(vp + (c * 8 + e) * T);
      const half8_t v1 = *(const half8_t*)(vp + (c * 8 + e) * T + 8);
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) acc += (float)ph[vt_pos(k)] * (float)v0[k] + (float)ph[vt_pos(k + 8)] * (float)v1[k];  // memory position -> token (vt_pos)
      o8[e] = (half_t)(acc * inv);
    }
    *(half8_t*)(op + c * 8) = o8;
  }
}
