// The UNets' GroupNorm behind lfm_groupnorm_f16 / lfm_groupnorm2_f16: which kernels serve a shape, and the launch.  gn_choose is the ONE place that knows
// (lfm_groupnorm_plan returns its answer without a launch: the truth table of tests/test_host_logic.py); with cpg = C / groups channels per group:
//   refused    N, HW, C or groups <= 0, groups > 32, C % groups, C % 8
//   statistics FUSED    cpg % 8 == 0, cpg <= 2048, HW <= 1024, flag UNET_GN_ROWS not set: one kernel for statistics and apply (one block's 256 threads cover the
//                       gpb cpg / 8 channel octets of its groups, so a group is at most 2048 channels wide); measured on the celeb512 UNet: at 64x64 maps its
//                       256 blocks are too few -- 300 us against ~35 us for the three kernels
//              ROWS     else cpg % 4 == 0 and C / 8 <= 256: gn_stats_rows_kernel, slots per half-octet
//              GROUPS4  else cpg % 4 == 0 (C / 8 > 256): gn_stats_general_kernel<4>, slots per group, 2048 pixels per block
//              GROUPS1  else: gn_stats_general_kernel<1>
//              at most GN_MAX_SLABS slabs per image on the three; then gn_coef_kernel
//   apply      FUSED    with the fused statistics
//              OCTET    else C / 8 <= 256 and 256 % (C / 8) == 0: gn_affine_rows_kernel, a thread per channel octet, at least four pixel rows per block
//              CHUNK    else: gn_affine_kernel, a thread per 16-byte chunk; refused at HW (C / 8) >= 2^31 (its 32-bit index)
#pragma once
#include "debug_flags.h"
#include "groupnorm_kernels.h"

enum { GN_STATS_FUSED = 1, GN_STATS_ROWS = 2, GN_STATS_GROUPS4 = 3, GN_STATS_GROUPS1 = 4 };
enum { GN_APPLY_FUSED = 1, GN_APPLY_OCTET = 2, GN_APPLY_CHUNK = 3 };
struct GnPlan {
  int err;           // LFM_OK, or the refusal (the other fields mean nothing then)
  int stats, apply;  // GN_STATS_*, GN_APPLY_*
  int gpb;           // FUSED: groups per block
  int ppb, slabs;    // ROWS, GROUPS4, GROUPS1: pixels per statistics block, slabs per image
  int app;           // OCTET: pixels per apply block
};

static inline GnPlan gn_choose(int N, int HW, int C, int groups) {
  GnPlan p{LFM_ERR_SHAPE, 0, 0, 0, 0, 0, 0};
  if (N <= 0 || HW <= 0 || C <= 0 || groups <= 0 || groups > 32 || C % groups || C % 8) return p;
  const int G = groups, cpg = C / G, c8n = C / 8;
  if (cpg % 8 == 0 && cpg <= 2048 && HW <= 1024 && !(lfm_gemm_debug_flags() & LFM_DBG_UNET_GN_ROWS)) {  // flag: the three-kernel path (A/B)
    p.stats = GN_STATS_FUSED;
    p.apply = GN_APPLY_FUSED;
    p.gpb = 1;
    while (p.gpb * 2 <= G && G % (p.gpb * 2) == 0 && (long)N * (G / (p.gpb * 2)) >= 256 && p.gpb * 2 * cpg <= 2048) p.gpb *= 2;
    p.err = LFM_OK;
    return p;
  }
  if (cpg % 4 == 0 && c8n <= 256) {
    p.stats = GN_STATS_ROWS;
    p.ppb = gn_pixels_per_block(HW);
  } else {
    p.stats = cpg % 4 == 0 ? GN_STATS_GROUPS4 : GN_STATS_GROUPS1;
    p.ppb = 2048;
  }
  if (cdiv(HW, p.ppb) > GN_MAX_SLABS) p.ppb = cdiv(HW, GN_MAX_SLABS);
  p.slabs = cdiv(HW, p.ppb);
  if (c8n <= 256 && 256 % c8n == 0) {
    const int pstride = 256 / c8n;  // pixel rows per block
    p.apply = GN_APPLY_OCTET;
    p.app = gn_pixels_per_block(HW);
    if (p.app < 4 * pstride) p.app = 4 * pstride < HW ? 4 * pstride : HW;
  } else {
    p.apply = GN_APPLY_CHUNK;
    if ((long)HW * c8n >= (1L << 31)) return p;
  }
  p.err = LFM_OK;
  return p;
}
extern "C" int lfm_groupnorm_plan(int N, int HW, int C, int groups) {
  const GnPlan p = gn_choose(N, HW, C, groups);
  return p.err ? p.err : p.stats | p.apply << 4;
}

// partials [N][GN_MAX_SLABS][max of the two slot layouts: C / 4 half-octets, 32 groups][2], then the coefficients {a, b} [N][C]
static inline size_t gn_part_bytes(int N, int C) {
  const size_t per_slab = (size_t)(C / 4 > 32 ? C / 4 : 32) * 2 * 4;
  return (((size_t)N * GN_MAX_SLABS * per_slab) + 255) / 256 * 256;
}
extern "C" size_t lfm_groupnorm_scratch_bytes(int N, int C) { return gn_part_bytes(N, C) + (size_t)N * C * 8 + 256; }

static int groupnorm_launch(const GnIn& in, void* y, const float* gamma, const float* beta, const float* film, long film_stride, void* scratch, int N,
                            int HW, int C, int groups, float eps, int silu, lfm_stream_t stream) {
  if (!in.a || !y || !gamma || !beta || !scratch) return LFM_ERR_ARG;
  const GnPlan p = gn_choose(N, HW, C, groups);
  if (p.err) return p.err;
  hipStream_t st = (hipStream_t)stream;
  const int G = groups, cpg = C / G;
  float* part = (float*)scratch;
  float* ab = (float*)((char*)scratch + gn_part_bytes(N, C));
  switch (p.stats) {
    case GN_STATS_FUSED:
      GN_LAUNCH_SILU(gn_fused_kernel, silu, dim3(G / p.gpb, N), st, in, (half_t*)y, gamma, beta, film, film_stride, HW, C, cpg, p.gpb, eps);
      LFM_CHECK_LAUNCH();
      return LFM_OK;
    case GN_STATS_ROWS: hipLaunchKernelGGL(gn_stats_rows_kernel, dim3(p.slabs, N), dim3(256), 0, st, in, part, HW, C, p.ppb); break;
    case GN_STATS_GROUPS4: hipLaunchKernelGGL(gn_stats_general_kernel<4>, dim3(G, N, p.slabs), dim3(256), 0, st, in, part, HW, C, cpg, p.ppb, G); break;
    default: hipLaunchKernelGGL(gn_stats_general_kernel<1>, dim3(G, N, p.slabs), dim3(256), 0, st, in, part, HW, C, cpg, p.ppb, G);
  }
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(gn_coef_kernel, dim3(cdiv((long)N * C, 256)), dim3(256), 0, st, part, p.slabs, p.stats == GN_STATS_ROWS, gamma, beta, film,
                     film_stride, ab, N, C, cpg, HW, p.ppb, eps, G);
  LFM_CHECK_LAUNCH();
  if (p.apply == GN_APPLY_OCTET)
    GN_LAUNCH_SILU(gn_affine_rows_kernel, silu, dim3(cdiv(HW, p.app), N), st, in, (half_t*)y, ab, HW, C, p.app);
  else
    GN_LAUNCH_SILU(gn_affine_kernel, silu, dim3(cdiv((long)HW * (C / 8), 256), N), st, in, (half_t*)y, ab, HW, C, (long)N * HW * C / 8);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_groupnorm_f16(const void* x, void* y, const float* gamma, const float* beta, const float* film, long film_stride, void* scratch,
                                 int N, int HW, int C, int groups, float eps, int silu, lfm_stream_t stream) {
  return groupnorm_launch(GnIn{(const half_t*)x, nullptr, C, 0}, y, gamma, beta, film, film_stride, scratch, N, HW, C, groups, eps, silu, stream);
}
// GroupNorm of the channel concat [xa (Ca channels) | xb (Cb channels)] without materialising it; y is dense [N*HW, Ca + Cb]; the plan is that of C = Ca + Cb
extern "C" int lfm_groupnorm2_f16(const void* xa, int Ca, const void* xb, int Cb, void* y, const float* gamma, const float* beta, const float* film,
                                  long film_stride, void* scratch, int N, int HW, int groups, float eps, int silu, lfm_stream_t stream) {
  if (!xa || !xb) return LFM_ERR_ARG;
  if (Ca <= 0 || Cb <= 0 || (Ca % 8) || (Cb % 8)) return LFM_ERR_SHAPE;
  if (((uintptr_t)xa | (uintptr_t)xb) & 15) return LFM_ERR_ALIGN;
  return groupnorm_launch(GnIn{(const half_t*)xa, (const half_t*)xb, Ca, Cb}, y, gamma, beta, film, film_stride, scratch, N, HW, Ca + Cb, groups, eps, silu,
                          stream);
}
