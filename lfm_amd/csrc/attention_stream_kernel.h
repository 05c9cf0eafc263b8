// Streamed, persistent attention core for the benchmarked DiT shape: 256 tokens x head_dim 64 (timm Attention as called at
// /root/reference/models/DiT.py:120): O = softmax(Q K^T * hd^-0.5) V per (image, head) item.  Round 6.
//
// Why a second kernel (the per-item one stays for every other shape, attention_kernel.h): with one workgroup per item, 1024 items on 256 CUs x 2 resident
// workgroups are exactly TWO rounds, and a round is load-everything (96 KiB per workgroup, ~11k cycles with all 512 workgroups bursting at once), then
// compute (~15k), then drain the stores (~5k) -- the memory system idles while the matrix pipe works and the other way round (profiles/r03_attention_wg_timeline.txt,
// r04_attention_narrow_timeline.txt: memory-only 22.6 us, compute-only 28.5 us, whole kernel 33.4 us).  Here a workgroup is PERSISTENT (grid = two per CU, items
// strided over the grid) and K / V^T never stop streaming: the LDS holds a four-slot ring of 64-key STAGES (K rows 64 x 128 B + V^T rows 64 dims x 128 B = 16 KiB per
// slot, whole 128-byte lines on both operands), slot s always carries stage s of whatever item is current, and the LDS-DMA of a slot's next tenant is issued at
// the first barrier after its last reader: K runs three stages ahead of the MFMAs that consume it, V^T two -- across item boundaries, so only the first stage of a
// workgroup's first item is ever waited for with nothing else to do.
//
// Same arithmetic as dit_attention_kernel<256, 1, 64>, eight waves x 32 queries: the S^T block, the online softmax over 32-key blocks, the P V block, the
// normalisation and the swizzled output staging are attention_common.h's (att_qk_block, att_softmax_block, att_pv_block, att_normalised, att_oswz_*), the one
// text every MFMA attention kernel inlines -- the results are BIT-IDENTICAL to that kernel's (tests/test_gpu_dit.py::test_attention_stream_matches_per_item).
//   * every LDS address of the key loop is one of four per-lane registers + an immediate (slot, key block and k-slot are compile-time: the item body is fully unrolled);
//     K and V^T stages share the swizzle (16-byte chunk c of row r stored at c ^ ((r >> 1) & 7): conflict-free for the 16-lane groups of ds_read_b128), so the SAME
//     four registers address both;
//   * Q fragments and O rows go through buffer instructions: per item only two SGPR offsets change.
// VMEM bookkeeping (vmcnt counts loads, LDS-DMAs and stores alike and retires in issue order).  Per wave and item: 8 LDS-DMAs (one per stage and operand), 4 Q loads,
// 4 O stores.  Issue order, g = 4 item + stage: prologue K0 Q Q Q Q V0 K1 V1 K2 (four operations behind the
// Q loads, as in the steady state: the compiler's own wait for the fragments is vmcnt(4) on both paths); after barrier b: K(b+3), V(b+2); behind barrier 4i+3 also Q(i+1) x 4 (once the last
// S MFMAs of item i have consumed the old fragments) and O(i) x 4.  Barrier b needs K(b) and V(b) (and Q for b = 4i): the counted waits are 4 / 10 / 2 / 2 for stage
// 0 / 1 / 2 / 3 (first item: 3 / 3 / 2 / 2).  Stages past the workgroup's last item are issued with an out-of-range buffer offset (no memory traffic, zeros, but they
// COUNT), so the waits are the same to the end.
// LDS: 4 x 16 KiB ring + 8 x 1 KiB output staging (a wave's 8 rows x 128 B per pass, four passes: a store instruction covers eight whole 128-byte rows) = 72 KiB: two
// workgroups per CU, four waves per SIMD, <= 128 VGPRs.  (80 KiB -- 2 KiB of staging per wave, two passes -- measured the same time; the occupancy query answers two workgroups per CU for both sizes and the
// per-workgroup trace shows both resident from the start: profiles/r06_attention_stream.txt.)
#pragma once
#include <stdlib.h>
#include "attention_common.h"

// MODE (measurement builds only, the ATT_MODE field of the flags, like the per-item kernel): 1 = memory only (LDS-DMA ring, waits, barriers, Q loads, O stores; no MFMA / softmax),
// 2 = compute only (every LDS-DMA and Q load out of range: no operand traffic), 3 = s_memtime trace (att_trace = wave 0 of the first / last
// workgroup: slot 0 start, 1 prologue issued, 2 + 14 i + 3 j + {0 before the wait, 1 after the wait, 2 after the barrier} for stage j of the workgroup's item i < 2,
// 14 + 14 i key loop done, 15 + 14 i stores issued; att_wg_trace = {HW_ID | XCC_ID << 32, start, first barrier passed, end} per workgroup)
template <int MODE = 0>
__global__ __launch_bounds__(512, 4) void dit_attention_stream_kernel(const half_t* __restrict__ Q, const half_t* __restrict__ K, const half_t* __restrict__ Vt,
                                                                      half_t* __restrict__ O, int D, int heads, int items, int gq, int gr, unsigned kbytes,
                                                                      float scale_log2e) {
  constexpr int T = 256, HD = 64;
  constexpr int SLOT = 16384, VOFF = 8192, OSTG = 4 * SLOT;  // ring slot (K stage | V^T stage), V^T inside a slot, output staging
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int hsel = lane >> 5, l31 = lane & 31;
  const int G = gridDim.x;
  [[maybe_unused]] const bool tr_first = blockIdx.x == 0, tr_last = blockIdx.x == gridDim.x - 1;
  [[maybe_unused]] int tr_item = 0;
  auto stamp = [&](int slot) {
    if constexpr (MODE == 3)
      if (wave == 0 && (tr_first || tr_last) && slot < 32) att_stamp((tr_first ? 0 : 32) + slot, lane);
  };
  auto wg_stamp = [&](int slot) {
    if constexpr (MODE == 3)
      if (wave == 0) att_wg_stamp(blockIdx.x, slot, lane);
  };
  stamp(0);
  wg_stamp(0);
  int item = blockIdx.x;
  int img = item / heads, head = item - img * heads;

  // resources over the whole tensors (num_records = their size: an offset >= 2^31 is out of range -> the tail stages fetch nothing)
  const __amdgpu_buffer_rsrc_t rs_k = __builtin_amdgcn_make_buffer_rsrc((void*)K, 0, (int)kbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_v = __builtin_amdgcn_make_buffer_rsrc((void*)Vt, 0, (int)kbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_q = __builtin_amdgcn_make_buffer_rsrc((void*)Q, 0, (int)kbytes, 0x00020000);
  const __amdgpu_buffer_rsrc_t rs_o = __builtin_amdgcn_make_buffer_rsrc((void*)O, 0, (int)kbytes, 0x00020000);
  // LDS-DMA: lane i of the workgroup fills 16-byte position (i & 7) of stage row (i >> 3) with the row's chunk (i & 7) ^ key
  const int srow = tid >> 3, sch = (tid & 7) ^ ((srow >> 1) & 7);
  const unsigned koff = (unsigned)(srow * D + sch * 8) * 2u;  // K rows: tokens, D halves apart
  const unsigned voff = (unsigned)(srow * T + sch * 8) * 2u;  // V^T rows: head dims, T halves apart
  constexpr unsigned POISON = 0x80000000u;
  char* const dma_dst = smem + wave * 1024;  // + slot * SLOT (+ VOFF): lane-linear 1 KiB per wave
  // fragment reads: row (lane & 31) of a 32-row block, chunk ((2 j + hsel) ^ key) = one of four per-lane offsets
  unsigned fa[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) fa[j] = (unsigned)(l31 * 128 + ((((j * 2 + hsel) ^ ((l31 >> 1) & 7))) << 4));
  const unsigned qoff = (unsigned)((wave * 32 + l31) * D + hsel * 8) * 2u;
  // output staging, per wave: pass h holds rows 8 h .. 8 h + 7 of the wave's 32 queries as swizzled 128-byte rows (att_oswz_*, attention_common.h)
  char* const ob = smem + OSTG + wave * 1024;
  const unsigned ord0 = att_oswz_get(lane);
  const unsigned ooff = (unsigned)((wave * 32 + (lane >> 3)) * D + (lane & 7) * 8) * 2u;

  auto item_k = [&](int im, int hd) { return (unsigned)((im * T) * D + hd * HD) * 2u; };   // byte offset of the item's K / Q / O block (row 0, head column 0)
  auto item_v = [&](int im, int hd) { return (unsigned)((im * heads + hd) * HD * T) * 2u; };
  auto dma_k = [&](unsigned base, bool live, int stage) {
    glds16_buf(rs_k, live && MODE < 2 ? koff : POISON, base + (unsigned)(stage * 64 * D) * 2u, dma_dst + stage * SLOT);
  };
  auto dma_v = [&](unsigned base, bool live, int stage) {
    glds16_buf(rs_v, live && MODE < 2 ? voff : POISON, base + (unsigned)(stage * 64) * 2u, dma_dst + stage * SLOT + VOFF);
  };
  half8_t qf[4];
  auto load_q = [&](unsigned base) {
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      const f32x4 r = __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(rs_q, (int)((MODE < 2 ? qoff : POISON) + ks * 32), (int)base, 0));
      qf[ks] = __builtin_bit_cast(half8_t, r);
    }
  };

  unsigned kb_cur = item_k(img, head), vb_cur = item_v(img, head);
  // ---- prologue: the first three K stages and two V^T stages of the first item, its Q fragments
  dma_k(kb_cur, true, 0);
  load_q(kb_cur);
  dma_v(vb_cur, true, 0);
  dma_k(kb_cur, true, 1);
  dma_v(vb_cur, true, 1);
  dma_k(kb_cur, true, 2);
  stamp(1);

  f32x16 Oa[2];
  float mrun, lrun;

  // S^T block: 32 keys (block kbl of the stage in `slot`) x the wave's 32 queries
  auto qk = [&](f32x16& S, int slot, int kbl) {
    if constexpr (MODE == 1) return;
    att_qk_block<HD, 1>(&S, &qf, hsel, [&](int ks) { return smem + slot * SLOT + kbl * 4096 + fa[ks]; });
  };
  // online softmax of one 32-key block for the query this lane owns, then O^T += V^T P^T (chunk 4 kbl + 2 s + hsel of the stage's V^T row)
  auto softmax_pv = [&](f32x16& S, int slot, int kbl, bool first_block) {
    if constexpr (MODE == 1) return;
    half8_t P[2];
    att_softmax_block<2>(S, first_block, mrun, lrun, Oa, scale_log2e, P);
    att_pv_block<2, 1>(&Oa, &P, [&](int s, int db) { return smem + slot * SLOT + VOFF + db * 4096 + fa[kbl * 2 + s]; });
  };

  bool first = true;
#pragma unroll 1
  for (;;) {
    // the next item of this workgroup (strided by the grid); past the end its stages are issued out of range
    int nimg = img + gq, nhead = head + gr;
    if (nhead >= heads) {
      nhead -= heads;
      ++nimg;
    }
    const bool has_next = item + G < items;
    const unsigned kb_next = has_next ? item_k(nimg, nhead) : 0u, vb_next = has_next ? item_v(nimg, nhead) : 0u;

#pragma unroll
    for (int e = 0; e < 16; ++e) Oa[0][e] = 0.f, Oa[1][e] = 0.f;
    mrun = -3.0e38f;
    lrun = 0.f;

    // ---- stage 0 landed (and this item's Q): everything older than the previous item's four output stores
    if (tr_item < 2) stamp(2 + 14 * tr_item);
    if (first) ATS_VMCNT(3);
    else ATS_VMCNT(4);
    if (tr_item < 2) stamp(3 + 14 * tr_item);
    ATS_BARRIER();
    if (tr_item < 2) stamp(4 + 14 * tr_item);
    if (first) wg_stamp(1);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(qf[ks]));  // the compiler's own wait for the Q loads goes HERE, before the next LDS-DMAs are issued
    dma_k(kb_cur, true, 3);
    dma_v(vb_cur, true, 2);
    // ---- stage j + 1 landed; every wave is past its reads of K stage j and V^T stage j - 1: counted wait, barrier, the next two LDS-DMAs
    auto next_stage = [&](int j) {
      if (tr_item < 2) stamp(2 + 14 * tr_item + 3 * (j + 1));
      if (j == 0) {
        if (first) ATS_VMCNT(3);
        else ATS_VMCNT(10);
      } else {
        ATS_VMCNT(2);
      }
      if (tr_item < 2) stamp(3 + 14 * tr_item + 3 * (j + 1));
      ATS_BARRIER();
      if (tr_item < 2) stamp(4 + 14 * tr_item + 3 * (j + 1));
      if (j == 0) {
        dma_k(kb_next, has_next, 0);
        dma_v(vb_cur, true, 3);
      } else if (j == 1) {
        dma_k(kb_next, has_next, 1);
        dma_v(vb_next, has_next, 0);
      } else {
        dma_k(kb_next, has_next, 2);
        dma_v(vb_next, has_next, 1);
      }
    };
    // The eight key blocks of the item, MFMA-first: the S MFMAs of block b + 1 are issued before the softmax arithmetic of block b, so the matrix pipe works under the
    // VALU-heavy part.  (Measured and not kept, round 6: waves 4-7 in VALU-first order so that a SIMD's two waves of this workgroup want the pipe and the issue port
    // at different times -- 33.4 vs 31.8 us, 6144 items 180.7 vs 170.0: the VALU-first half loses its software pipeline, and the second code path costs 8 spilled
    // dwords under the 128-register budget.)
    f32x16 Sa, Sb;
    qk(Sa, 0, 0);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      qk(Sb, j, 1);
      if (j == 3 && has_next) load_q(kb_next);  // the old fragments are dead: the next item's arrive under the last two softmax blocks and the output pass
      softmax_pv(Sa, j, 0, j == 0);
      if (j < 3) {
        next_stage(j);
        qk(Sa, j + 1, 0);
      }
      softmax_pv(Sb, j, 1, false);
    }
    // ---- normalise and store: lane owns query (lane & 31), d = db * 32 + 8 g + 4 hsel + r.  Four passes of 8 rows through the wave's staging rows.
    if (tr_item < 2) stamp(14 + 14 * tr_item);
    {
      const float inv = att_inv_l(lrun);
      const unsigned obase = kb_cur;
#pragma unroll
      for (int h = 0; h < 4; ++h) {
        if ((l31 >> 3) == h) att_normalised<HD>(Oa, inv, [&](int db, int g, half4_t hv) { *(half4_t*)(ob + att_oswz_put(l31 & 7, hsel, db, g)) = hv; });
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // wave-private rows: no barrier (the asm is also the COMPILER barrier between the half4 writes and the
                                                            // f32x4 read of the same bytes: without it type-based alias analysis lets the read move up -- measured: wrong rows)
        const f32x4 v = *(const f32x4*)(ob + ord0);
        __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(__attribute__((ext_vector_type(4))) unsigned, v), rs_o, (int)ooff,
                                               (int)(obase + (unsigned)(h * 8 * D) * 2u), 0);
        if (h < 3) asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the rows of pass h are in registers before pass h + 1 overwrites them
      }
    }
    if (tr_item < 2) stamp(15 + 14 * tr_item);
    ++tr_item;
    if (!has_next) break;
    first = false;
    item += G;
    img = nimg;
    head = nhead;
    kb_cur = kb_next;
    vb_cur = vb_next;
  }
  if constexpr (MODE == 3) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wg_stamp(2);
  }
}

// grid = min(items, 2 x CUs): two resident workgroups per CU (72 KiB of LDS, <= 128 VGPRs).  MODE: the measurement variants (attention_launch picks one).
template <int MODE = 0>
static int attention_stream_launch(const half_t* Q, const half_t* K, const half_t* Vt, half_t* O, int batch, int heads, hipStream_t st) {
  constexpr int T = 256, HD = 64, LDS = 4 * 16384 + 8 * 1024;
  const long items = (long)batch * heads;
  const long bytes = items * T * HD * 2;  // = batch * T * D * 2: each of Q, K, V^T, O
  if (items <= 0 || bytes >= (1L << 31)) return LFM_ERR_SHAPE;  // 32-bit buffer offsets, bit 31 = the out-of-range mark: attention_choose never sends such tensors here
  if (!lfm_kernel_lds<&dit_attention_stream_kernel<MODE>>(LDS)) return LFM_ERR_LAUNCH;
  long per_cu = 2;
#ifdef LFM_MEASURE
  if (const char* e = getenv("LFM_ATS_WG_PER_CU")) per_cu = atoi(e) == 1 ? 1 : 2;  // measurement: one persistent workgroup per CU (twice the items each)
#endif
  const long resident = per_cu * lfm_cu_count();
  const int G = (int)(items < resident ? items : resident);
  const float sl2 = 0.125f * 1.4426950408889634f;  // hd^-0.5 * log2(e)
  hipLaunchKernelGGL(dit_attention_stream_kernel<MODE>, dim3(G), dim3(512), LDS, st, Q, K, Vt, O, heads * HD, heads, (int)items, G / heads, G % heads, (unsigned)bytes, sl2);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
