// Tiled attention core of a DiT block for ANY token count T with T % 16 == 0 (timm Attention as called at models/DiT.py:120 of the reference):
// O = softmax(Q K^T * hd^-0.5) V per (image, head) item, head_dim 64 or 72, T a RUNTIME argument.
//
// Why another kernel: every kernel behind attention_choose (attention_dispatch.h) has its token count as a template argument and the whole K / V^T of an item
// (or a 256-key chunk of it) resident in the LDS -- 16 / 64 / 128 / 256 / 1024 tokens, the grids of 256^2 and 512^2 images.  This one serves the other grids
// (--image_size 384 = 576 tokens, 192 = 144, 320 = 400, 768 = 2304): only a 64-key STAGE is resident, T is an argument.  Same operands as the other kernels, so
// the QKV epilogue is unchanged: Q, K, O fp16 [batch * T, D] with head-major columns, V^T fp16 [batch, heads, hd, T] in the vt_pos token order (gemm_epilogues.h).
//
// Shape.  A workgroup owns 128 QUERIES of one item (four waves x 32; blockIdx.x = item * qblocks + query block, so the workgroups that read the same K / V^T
// are neighbours) and walks ALL keys of the item in stages of 64 through a three-slot LDS ring.
//   * 128 queries, not 64: every staged byte then feeds four waves' MFMAs -- the L2 -> LDS traffic per query is half that of a two-wave workgroup, and four
//     waves are one per SIMD, so two or three co-resident workgroups give each SIMD independent instruction streams (the key loop is issue-bound, attention_common.h).
//     The price is the ragged last query block (576 tokens = 4.5 blocks: 10 % idle waves; 144 = 1.125: a tiny launch either way).  Waves whose 32 queries are
//     all >= T take part in the staging and reach every barrier, but run no MFMA.
//   * a stage = {K [64][hd] | V^T [hd][64]} as 16-byte LDS-DMA slots, lane-linear: 1024 slots = four passes of the 256 lanes for hd 64 (16 KiB), 1152 = four and a
//     half for hd 72 -- rounded up to five passes (20 KiB) whose dead slots are issued out of range, so that EVERY wave issues the same number of DMAs per
//     stage and one counted wait serves all.  128-byte K rows (hd 64) are XOR-swizzled at the DMA source (chunk ^ ((row >> 1) & 7)), 144-byte rows (hd 72)
//     need none; V^T stage rows are 128 bytes for both head sizes and swizzled by row with the same key.
//   * schedule: stage s + 2 is issued BEFORE the MFMAs of stage s (prologue: stages 0 and 1); top of iteration s: s_waitcnt vmcnt(passes) = "everything but
//     stage s + 1 has landed", one barrier (which also says that every wave is past its reads of stage s - 1, the slot stage s + 2 overwrites), the DMAs of
//     stage s + 2, then the two 32-key blocks of stage s.  No vmcnt(0) inside the loop; stages past the item's end are issued out of range (no traffic, but
//     they COUNT), so the wait is the same to the end.
//   * the arithmetic is attention_common.h's, one text for all kernels (att_load_q, att_qk_block, att_softmax_block, att_pv_block, att_normalised, att_ostage_*:
//     a lane owns ONE query, lane & 31, and holds its scores at keys 32 block + 8 g + 4 (lane >> 5) + r in register 4 g + r); the S MFMAs of both blocks of a
//     stage are issued before the softmax arithmetic of the first.  Same key order as the kernels that own 64 / 128 / 256 / 1024 tokens => bit-identical to them
//     (tests/test_gpu_dit_attention_tiled.py::test_tiled_kernel_on_the_shapes_other_kernels_own).
//   * every item is addressed through buffer resources of its own -- base = the item's K / V^T block, num_records = its extent, 32-bit offsets inside it (at most
//     T * D * 2 bytes) -- so no tensor-size limit appears; Q and O rows go through 64-bit pointers.
// The two tails.  T % 64 is 0 / 16 / 32 / 48, and for a grid side of 4 x odd T % 32 is 16: half a softmax block.
//   * keys >= T: their DMA slots are issued out of range, K rows and V^T 16-byte chunks alike (T % 16 == 0 and the vt_pos permutation stays inside a 16-group, so
//     a chunk is live or dead as a whole) -- the LDS image holds ZEROS there, whatever lies behind the item in memory (the next image's rows, the end of the
//     tensor) is never fetched.  Their scores are REPLACED by -inf before att_softmax_block sees them (a select: in the S layout a lane's registers split by
//     key group, so the dead half of a block is registers 8 .. 15 in every lane) -> P = 0 exactly, and 0 x 0 in the P V MFMA.  A block with no live key is skipped.
//   * queries >= T: the lane loads row T - 1 instead (finite scores, no special case in the loop) and stores nothing.
// O rows leave through the LDS (the ring is dead by then): a wave writes its 32 rows as 8-byte pieces and stores them as whole 16-byte chunks of whole rows.
// Served by default (attention_choose): T a perfect square of a grid side that is a multiple of 4, 144 <= T <= 3600, where no other kernel serves the shape.
// The upper end is NOT this kernel's limit (offsets and grid allow far more): tests/test_host_logic.py pins 4096 tokens as refused, and lifting that is a
// follow-up that edits those rows.  LFM_OPT_ATTENTION_TILED = 2 runs every T % 16 == 0, 16 <= T < 4096 here (parity tests, A/B).
// Build (gfx950, -O3): hd 64: 133 VGPRs, no scratch, 48 KiB of LDS -- three workgroups (three waves per SIMD) per CU; hd 72: 170 VGPRs, no scratch, 60 KiB -- two.
// Timings: profiles/dit_attention_tiled.txt.
#pragma once
#include "attention_common.h"

template <int HD>
__global__ __launch_bounds__(256, 2) void dit_attention_tiled_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ Vt,
                                                                     half_t* __restrict__ O, int T, int D, int heads, int qblocks, float scale_log2e) {
  static_assert(HD == 64 || HD == 72, "head_dim 64 / 72");
  constexpr int NTHR = 256, QB = 128, KST = 64;  // lanes, queries per workgroup, keys per stage
  constexpr int KS = (HD + 15) / 16;             // k-slots of the S MFMAs (hd 72: the fifth is half empty)
  constexpr int NDB = (HD + 31) / 32;            // 32-row blocks of O^T
  constexpr int KCH = HD / 8, KROW = KCH * 16;   // 16-byte chunks / bytes per K row
  constexpr bool KSWZ = HD == 64;
  constexpr int KSLOTS = KST * KCH, VSLOTS = HD * 8, SLOTS = KSLOTS + VSLOTS;  // 16-byte DMA slots of a stage: K rows, then V^T rows
  constexpr int NPASS = (SLOTS + NTHR - 1) / NTHR;                            // DMAs per lane and stage: 4 / 5
  constexpr int STAGE = NPASS * NTHR * 16, VOFF = KSLOTS * 16;
  static_assert(NPASS == 4 || NPASS == 5, "the counted wait below");
  static_assert(KSLOTS % 64 == 0 && SLOTS % 64 == 0, "K / V^T / dead slots change at wave boundaries");
  static_assert(4 * 32 * ATT_OSTR<HD> <= 3 * STAGE, "output staging (padded rows, attention_common.h) inside the ring");
  constexpr unsigned POISON = 0x80000000u;  // beyond every num_records below: the DMA fetches nothing and writes zeros
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hsel = lane >> 5, l31 = lane & 31;
  const int qb = blockIdx.x % qblocks, item = blockIdx.x / qblocks;
  const int img = item / heads, head = item - img * heads;
  const half_t* Kg = K + (long)img * T * D + head * HD;
  const half_t* Vg = Vt + (long)item * HD * T;
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)Kg, 0, ((T - 1) * D + HD) * 2, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)Vg, 0, HD * T * 2, 0x00020000);

  // ---- this lane's DMA slots: pass p fills 16-byte slot p * 256 + tid of the stage.  Byte offset at stage 0, the first key the slot holds (-> live while
  // key + 64 stage < T), and whether it is a K slot (wave-uniform: the offset advances by 64 K rows, else by 64 keys of a V^T row).
  unsigned off0[NPASS];
  int key0[NPASS];
  bool is_k[NPASS];
#pragma unroll
  for (int p = 0; p < NPASS; ++p) {
    const int s = p * NTHR + tid;
    is_k[p] = p * NTHR + wave * 64 < KSLOTS;
    if (is_k[p]) {
      const int row = s / KCH, ch = s - row * KCH;
      const int c = KSWZ ? (ch ^ ((row >> 1) & 7)) : ch;
      off0[p] = (unsigned)(row * D + c * 8) * 2u;
      key0[p] = row;
    } else if (p * NTHR + wave * 64 < SLOTS) {
      const int v = s - KSLOTS, row = v >> 3, c = (v & 7) ^ ((row >> 1) & 7);
      off0[p] = (unsigned)(row * T + c * 8) * 2u;
      key0[p] = c * 8;
    } else {  // the padding of the last pass (hd 72)
      off0[p] = POISON;
      key0[p] = 1 << 30;
    }
  }
  const unsigned kstep = (unsigned)(KST * D) * 2u;
  auto issue = [&](int st, int slot) {
    const int k0 = st * KST;
    char* dst = smem + slot * STAGE + wave * 1024;
#pragma unroll
    for (int p = 0; p < NPASS; ++p) {
      const bool live = key0[p] + k0 < T;
      if (is_k[p]) glds16_buf(rs_k, live ? off0[p] + (unsigned)st * kstep : POISON, 0u, dst + p * (NTHR * 16));
      else glds16_buf(rs_v, live ? off0[p] + (unsigned)k0 * 2u : POISON, 0u, dst + p * (NTHR * 16));
    }
  };

  // ---- this wave's 32 queries as the B operand of S^T (rows >= T: row T - 1, never stored).  Requested BEFORE the first DMAs: the compiler's own wait for the
  // fragments (in front of the loop) then leaves the two stages behind them in flight.
  const int q0 = qb * QB + wave * 32;
  const bool wave_live = q0 < T;  // wave-uniform
  half8_t qf[KS];
  att_load_q<HD>(qf, Q + ((long)img * T + (q0 + l31 < T ? q0 + l31 : T - 1)) * D + head * HD, hsel);
  issue(0, 0);
  issue(1, 1);
#pragma unroll
  for (int ks = 0; ks < KS; ++ks) asm volatile("" : "+v"(qf[ks]));  // the compiler's wait for the fragments goes HERE, counted (in front of a loop it drains everything)

  f32x16 Oa[NDB];
#pragma unroll
  for (int db = 0; db < NDB; ++db)
#pragma unroll
    for (int e = 0; e < 16; ++e) Oa[db][e] = 0.f;
  float mrun = -3.0e38f, lrun = 0.f;

  // S^T block kbl of the stage at Ks: 32 keys x the wave's 32 queries
  const int kkey = KSWZ ? ((l31 >> 1) & 7) : 0;
  auto qk = [&](f32x16& S, const char* Ks, int kbl) {
    const char* kp = Ks + (kbl * 32 + l31) * KROW;
    att_qk_block<HD, 1>(&S, &qf, hsel, [&](int ks) { return kp + ((att_k_chunk<HD>(ks, hsel) ^ kkey) << 4); });
  };
  // online softmax of the block for the query this lane owns, then O^T += V^T P^T.  `half_blk`: only the block's first 16 keys exist.
  auto softmax_pv = [&](f32x16& S, const char* Ks, int kbl, bool first, bool half_blk) {
#pragma unroll
    for (int e = 8; e < 16; ++e)
      if (half_blk) S[e] = -__builtin_inff();
    half8_t P[2];
    att_softmax_block<NDB>(S, first, mrun, lrun, Oa, scale_log2e, P);
    att_pv_block<NDB, 1>(&Oa, &P, [&](int s, int db) {  // chunk 4 kbl + 2 s + hsel of the lane's V^T row of the stage
      const int d = att_v_row<HD>(db, l31);
      return Ks + VOFF + d * 128 + (((kbl * 4 + 2 * s + hsel) ^ ((d >> 1) & 7)) << 4);
    });
  };

  // top of stage st: stage st (first time also Q) has landed -- only the DMAs of stage st + 1 may still fly --, every wave's share of it is in the LDS and every
  // wave is past its reads of stage st - 1, whose slot the DMAs of stage st + 2 overwrite
  int cur = 0;  // ring slot of the current stage
  auto begin_stage = [&](int st) {
    if constexpr (NPASS == 4) ATS_VMCNT(4);
    else ATS_VMCNT(5);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    ATS_BARRIER();
    issue(st + 2, cur == 0 ? 2 : cur - 1);  // slot (cur + 2) % 3
  };
  const int nfull = T / KST;  // whole stages: the loop body has no tail case
#pragma unroll 1
  for (int st = 0; st < nfull; ++st) {
    begin_stage(st);
    if (wave_live) {
      const char* Ks = smem + cur * STAGE;
      f32x16 Sa, Sb;
      qk(Sa, Ks, 0);
      qk(Sb, Ks, 1);
      softmax_pv(Sa, Ks, 0, st == 0, false);
      softmax_pv(Sb, Ks, 1, false, false);
    }
    cur = cur == 2 ? 0 : cur + 1;
  }
  const int rem = T - nfull * KST;  // keys of the ragged last stage: 0 / 16 / 32 / 48
  if (rem) {
    begin_stage(nfull);
    if (wave_live) {
      const char* Ks = smem + cur * STAGE;
      f32x16 Sa, Sb;
      qk(Sa, Ks, 0);
      if (rem > 32) {
        qk(Sb, Ks, 1);
        softmax_pv(Sa, Ks, 0, nfull == 0, false);
        softmax_pv(Sb, Ks, 1, false, true);
      } else {
        softmax_pv(Sa, Ks, 0, nfull == 0, rem < 32);
      }
    }
  }

  // ---- normalise and store: lane owns query q0 + l31, d = 32 db + 8 g + 4 hsel + r.  The ring is dead: the (out-of-range, zero-writing) DMAs of the two stages past
  // the end have landed and every wave is past its last reads before a wave's staging rows overwrite it.
  ATS_VMCNT(0);
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
  ATS_BARRIER();
  if (!wave_live) return;
  char* ob = smem + wave * (32 * ATT_OSTR<HD>);
  att_normalised<HD>(Oa, att_inv_l(lrun), [&](int db, int g, half4_t h) { att_ostage_put<HD>(ob, l31, hsel, db, g, h); });
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private rows: no barrier
  att_ostage_store<HD, 32>(ob, O + ((long)img * T + q0) * D + head * HD, D, lane, T - q0);
}
