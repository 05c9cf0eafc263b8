// Kernel selection for the attention core of a DiT block (as gemm_dispatch.h for the GEMMs).  attention_choose is the ONE place that knows which kernel serves
// a shape (lfm_attention_plan returns its answer without a launch: tests/test_host_logic.py pins the table); attention_launch runs that answer.
#pragma once
#include <type_traits>
#include "attention_kernel.h"
#include "attention_stream_kernel.h"
#include "attention_tiled_kernel.h"

enum {
  ATT_KERN_T16 = 1,     // dit_attention_t16_kernel
  ATT_KERN_ITEM = 2,    // one workgroup per (image, head): 64 / 128 / 256 tokens
  ATT_KERN_WIDE = 3,    // the same with four waves x 64 queries (flag ATT_WIDE; hd 64, 256 tokens)
  ATT_KERN_CHUNKS = 4,  // 1024 tokens: four key chunks of 256 through the LDS, one workgroup per 256 queries
  ATT_KERN_QSPLIT = 5,  // latency mode (hd 64, 256 tokens, at most 64 items): two workgroups of four waves per item
  ATT_KERN_STREAM = 6,  // attention_stream_kernel.h (hd 64, 256 tokens, more than 64 items): persistent workgroups, K / V^T streamed through an LDS ring
  ATT_KERN_TILED = 7,   // attention_tiled_kernel.h: any T % 16 == 0 as a runtime argument, 128 queries per workgroup, keys in 64-key stages through an LDS ring
};
// the measurement-only variants MODE 1 / 2 / 3 of the hd-64, 256-token kernels (product builds have none)
static inline int att_measure_mode() {
#ifdef LFM_MEASURE
  return (lfm_gemm_debug_flags() >> LFM_DBG_ATT_MODE_SHIFT) & LFM_DBG_ATT_MODE_MASK;
#else
  return 0;
#endif
}
// Shapes the tiled kernel takes (LFM_OPT_ATTENTION_TILED = 2 sends all of them there) and the ones it serves by default: square grids of a side that is a multiple
// of 4 which no other kernel serves -- attention_choose asks the other kernels first.  T >= 4096 stays refused (tests/test_host_logic.py pins it), not a kernel limit.
static inline bool attention_tiled_takes(int hd, int T) { return (hd == 64 || hd == 72) && T >= 16 && T < 4096 && T % 16 == 0; }
static inline bool attention_tiled_default(int hd, int T) {
  if (!attention_tiled_takes(hd, T) || T < 144 || T > 3600) return false;
  int g = 12;
  while (g * g < T) g += 4;
  return g * g == T;
}
// Kernel for `batch` images x `heads` heads of `hd` dims x T tokens under the calling thread's flags and the library options, or LFM_ERR_SHAPE.  Pure host code.
static inline int attention_choose(int batch, int heads, int hd, int T) {
  if (hd != 64 && hd != 72) return LFM_ERR_SHAPE;
  const int tiled = lfm_attention_tiled_mode();  // LFM_OPT_ATTENTION_TILED: 0 = its shapes refused, 1 = the shapes no other kernel serves, 2 = every shape it takes (parity, A/B)
  if (tiled == 2 && attention_tiled_takes(hd, T)) return ATT_KERN_TILED;
  if (hd == 64 && T == 256) {  // the benchmarked shape
    // Rounds 1-3: 8 waves x 32 queries (4 waves/SIMD) measured 44.3 us vs 40.2 us for 4 waves x 64 queries (two 8-byte V^T reads per fragment then).
    // Round 4: with the V^T operand a single conflict-free ds_read_b128 (vt_pos) the balance flipped -- 8 waves x 32 queries (126 VGPRs: four waves per
    // SIMD) 35.7 us, 4 waves x 64 queries (228 VGPRs: two) 38.9 us -- so the narrow shape is the default; flag ATT_WIDE selects the wide one (A/B)
    if (lfm_gemm_debug_flags() & LFM_DBG_ATT_WIDE) return ATT_KERN_WIDE;
    const int items = batch * heads;
    if (items <= 64 && !att_measure_mode()) return ATT_KERN_QSPLIT;  // (it has no measurement variants: a mode runs the per-item kernel's)
    // the streamed kernel addresses each of Q, K, V^T, O with 32-bit buffer offsets whose bit 31 is its out-of-range mark: tensors below 2 GiB only
    if (items > 64 && lfm_attention_stream_enabled() && (long)items * 256 * 64 * 2 < (1L << 31)) return ATT_KERN_STREAM;
    return ATT_KERN_ITEM;
  }
  if (T == 16) return ATT_KERN_T16;
  if (T == 1024) return ATT_KERN_CHUNKS;
  if (T == 64 || T == 128 || T == 256) return ATT_KERN_ITEM;
  if (tiled && attention_tiled_default(hd, T)) return ATT_KERN_TILED;  // the other square grids of a side that is a multiple of 4, 144 .. 3600 tokens
  return LFM_ERR_SHAPE;
}

struct AttArgs {  // what every launch below passes on
  const half_t *Q, *K, *Vt;
  half_t* O;
  int batch, heads;
  float sl2;  // hd^-0.5 * log2(e)
  int stag;   // measurement builds: start offset of the second resident workgroups
  hipStream_t st;
};
// One instantiation of dit_attention_kernel: grid, block and LDS size are what its template arguments say.
template <int T, int JQ, int HD, int MODE = 0, int NCH = 1, int QS = 1>
static int att_run(const AttArgs& a) {
  constexpr int LDS = T * HD * 4;  // K + V^T, 2 bytes each (hd 72: 72 KiB, above the 64-KiB default)
  if (!lfm_kernel_lds<&dit_attention_kernel<T, JQ, HD, MODE, NCH, QS>>(LDS)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL((dit_attention_kernel<T, JQ, HD, MODE, NCH, QS>), dim3(a.heads, a.batch, NCH * QS), dim3(T / (32 * JQ * QS) * 64), LDS, a.st, a.Q, a.K, a.Vt,
                     a.O, a.heads * HD, a.heads, a.sl2, a.stag);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
// The tiled kernel: 128 queries per workgroup, a three-slot ring of 64-key stages (48 / 60 KiB of LDS).
template <int HD>
static int attention_tiled_run(const AttArgs& a, int T) {
  constexpr int SLOTS = 64 * (HD / 8) + HD * 8, LDS = 3 * ((SLOTS + 255) / 256) * 256 * 16;
  if (!attention_tiled_takes(HD, T)) return LFM_ERR_SHAPE;
  const int qblocks = (T + 127) / 128;
  const long grid = (long)a.batch * a.heads * qblocks;
  if (grid <= 0 || grid >= (1L << 31) || (long)T * a.heads * HD * 2 >= (1L << 31)) return LFM_ERR_SHAPE;  // (32-bit offsets inside ONE item's K rows)
  if (!lfm_kernel_lds<&dit_attention_tiled_kernel<HD>>(LDS)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL(dit_attention_tiled_kernel<HD>, dim3((unsigned)grid), dim3(256), LDS, a.st, a.Q, a.K, a.Vt, a.O, T, a.heads * HD, a.heads, qblocks, a.sl2);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
// f(std::integral_constant<int, MODE>) for the calling thread's measurement mode
template <class F>
static int att_with_mode(F&& f) {
#ifdef LFM_MEASURE
  switch (att_measure_mode()) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
  }
#endif
  return f(std::integral_constant<int, 0>{});
}

// Q, K: [batch*T, heads*hd] token-major; Vt: [batch][heads*hd][T]; O: [batch*T, heads*hd].  hd 64 / 72; T in {16, 64, 128, 256, 1024} or what attention_tiled_default says.
static int attention_launch(const half_t* Q, const half_t* K, const half_t* Vt, half_t* O, int batch, int heads, int hd, int T, hipStream_t st) {
  const int kern = attention_choose(batch, heads, hd, T);
  if (kern < 0) return kern;
  AttArgs a{Q, K, Vt, O, batch, heads, (hd == 64 ? 0.125f : 0.11785113019775793f) * 1.4426950408889634f, lfm_stagger_ticks(), st};
  switch (kern) {
    case ATT_KERN_T16: {
      const int items = batch * heads, D = heads * hd;
      if (hd == 64) hipLaunchKernelGGL(dit_attention_t16_kernel<64>, dim3((items + 3) / 4), dim3(64), 0, st, Q, K, Vt, O, D, heads, items, a.sl2);
      else hipLaunchKernelGGL(dit_attention_t16_kernel<72>, dim3((items + 3) / 4), dim3(64), 0, st, Q, K, Vt, O, D, heads, items, a.sl2);
      LFM_CHECK_LAUNCH();
      return LFM_OK;
    }
    case ATT_KERN_CHUNKS: return hd == 64 ? att_run<256, 1, 64, 0, 4>(a) : att_run<256, 1, 72, 0, 4>(a);
    case ATT_KERN_QSPLIT: a.stag = 0; return att_run<256, 1, 64, 0, 1, 2>(a);
    case ATT_KERN_STREAM: return att_with_mode([&](auto m) { return attention_stream_launch<decltype(m)::value>(Q, K, Vt, O, batch, heads, st); });
    case ATT_KERN_WIDE: return att_with_mode([&](auto m) { return att_run<256, 2, 64, decltype(m)::value>(a); });
    case ATT_KERN_TILED: return hd == 64 ? attention_tiled_run<64>(a, T) : attention_tiled_run<72>(a, T);
  }
  // ATT_KERN_ITEM.  hd 72: one query block per wave (48 accumulator + 20 Q registers per block)
  if (hd == 72) return T == 64 ? att_run<64, 1, 72>(a) : T == 128 ? att_run<128, 1, 72>(a) : att_run<256, 1, 72>(a);
  if (T == 256) return att_with_mode([&](auto m) { return att_run<256, 1, 64, decltype(m)::value>(a); });
  return T == 64 ? att_run<64, 2, 64>(a) : att_run<128, 2, 64>(a);
}
