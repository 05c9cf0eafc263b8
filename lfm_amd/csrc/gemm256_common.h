// Shared pieces of the 256-row MFMA GEMM kernels (256x128 "two workgroups per CU", gemm256n_kernel.h; 256x256 quadrant-phased on
// v_mfma_f32_16x16x32_f16, gemm256h_kernel.h): tile order, the barrier macro.  (The quadrant-phased operand ring and its K loop: gemm256q_ring.h;
// the LDS-transposed epilogue hand-over of both accumulator maps: epilogue_handover.h; the epilogue structs and the Epi interface: gemm_epilogues.h.)
// History (DESIGN.md section 3 keeps the measurements): the first two 256x256 generations -- a four-stage ping-pong ring of 32-deep K-tiles
// (round 1) and its quadrant-phased successor on 32x32x16 MFMAs with 64-deep K-tiles (round 1 / 2) -- were superseded by the 16x16x32 kernel
// and removed in round 3; no reference shape dispatched to them (every K on the path is a multiple of 64).
#pragma once
#include "gemm_kernel.h"

#ifdef LFM_MEASURE
// Two workgroups share a CU in the 256x128 GEMM and the halo convolution; dispatched together they run in lockstep (both in their main loops, then both in
// their epilogues).  The experiment: delay the second resident of every CU in the FIRST wave of workgroups (ids 256..511: consecutive ids go round the
// XCDs and then the CUs, so id + 256 is the partner of id); later workgroups inherit the offset because a slot frees when its predecessor ends.
__device__ __forceinline__ void lfm_stagger_start(int ticks) {
  if (ticks > 0 && blockIdx.x >= 256 && blockIdx.x < 512) {
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    while ((long long)(__builtin_amdgcn_s_memtime() - t0) < (long long)ticks) __builtin_amdgcn_s_sleep(16);
  }
}
#endif

#include "epilogue_handover.h"

#define G256_BM 256
#define G256_BN 256
static_assert(G256_BM == HO_TILE_ROWS, "the hand-over's interior test is written for 256-row tiles");

// Tile order.  Block b runs on XCD b%8: give each XCD a contiguous range of tile ids, and inside a range walk groups of
// GM = 4 M-panels column-major, so the ~32 tiles an XCD runs concurrently form a 4 x 8 patch (12 operand panels in its
// L2) instead of a 1 x 32 / 2 x 16 strip (33 / 18 panels).
__device__ __forceinline__ void g256_tile_order(int bid, int nb, int tiles_n, int dbg, int& tile_m, int& tile_n) {
  if ((nb & 7) == 0 && !(dbg & LFM_DBG_GEMM_NO_XCD_REMAP)) bid = (bid & 7) * (nb >> 3) + (bid >> 3);
  // GM x tiles_n should be a multiple of the ~32 tiles an XCD runs at once: 8 for 12 tile columns (QKV, measured -3 %), else 4
  const int tiles_m = nb / tiles_n, GM = (dbg & LFM_DBG_GEMM_GM8) ? 8 : ((dbg & LFM_DBG_GEMM_GM2) ? 2 : ((dbg & LFM_DBG_GEMM_GM4) ? 4 : ((tiles_n & 7) && tiles_n > 8 ? 8 : 4)));
  const int grp = bid / (GM * tiles_n), within = bid - grp * (GM * tiles_n);
  const int gm = (tiles_m - grp * GM) < GM ? (tiles_m - grp * GM) : GM;  // last group may be short
  tile_m = grp * GM + within % gm;
  tile_n = within / gm;
}

#define G256_BARRIER()                  \
  do {                                  \
    asm volatile("" ::: "memory");      \
    __builtin_amdgcn_s_barrier();       \
    asm volatile("" ::: "memory");      \
    __builtin_amdgcn_sched_barrier(0);  \
  } while (0)
