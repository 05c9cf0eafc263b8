// Kernel selection for every GEMM of the library (all generations share the operand / A-source / epilogue interfaces).
#pragma once
#include <type_traits>
#include "gemm256w_kernel.h"

// v6 (gemm256w_kernel.h, one wave per SIMD) serves row-major A operands and epilogues without per-lane tile accumulators
template <class ASrc, class Epi>
struct gemm_v6_ok {
  static constexpr bool value = std::is_same<ASrc, ASrcRowMajor>::value && !epi_has_finish_tile<Epi>::value;
};

// What an instantiation can take (the caps argument of lfm_gemm_plan): GEMM_CAP_V6 = gemm_v6_ok<ASrc, Epi>; GEMM_CAP_FITS = the 256x256 kernels address
// row-major operands through buffer resources (unsigned 32-bit byte offsets: operands below 2^31 elements, like the 32-bit row offsets of every kernel)
enum { GEMM_CAP_V6 = 1, GEMM_CAP_FITS = 2 };
template <class ASrc>
static inline bool gemm_fits256(const ASrc& asrc, int N, long ldw) {
  bool fits = (long)N * ldw < (1L << 31);
  if constexpr (asrc_has_buffer<ASrc>::value) fits = fits && asrc_fits_buffer(asrc, 0);
  return fits;
}
template <class ASrc, class Epi>
static inline int gemm_caps(const ASrc& asrc, int N, long ldw) {
  return (gemm_v6_ok<ASrc, Epi>::value ? GEMM_CAP_V6 : 0) | (gemm_fits256(asrc, N, ldw) ? GEMM_CAP_FITS : 0);
}

// THE choice, under the calling thread's selection: the 256x256 kernel (16x16x32 MFMAs, gemm256h_kernel.h; 5, or 6 = its one-wave-per-SIMD form) when the
// problem fills the chip with such tiles and K % 64 == 0, the 256x128 two-per-CU kernel (gemm256n_kernel.h; 4) for chip-filling problems that are only 128
// columns wide (or where it measured faster, see lfm_gemm_prefers_v4), the 128x128 kernel (1) otherwise.  lfm_gemm_select() (0 auto, 1 / 4 / 5 / 6 force a
// kernel) exists for A/B measurements and for parity tests of all kernels.  Returns the kernel that launch_gemm_kernel then runs: callers that depend on
// the epilogue's lane mapping (vae.hip: conv3) ask first and launch that id.
static inline int gemm_choose(int M, int N, int K, int batch, int caps) {
  const long tiles256 = (long)cdiv(M, 256) * cdiv(N, 256) * batch;
  const int sel = lfm_gemm_selected();
  const bool big = tiles256 >= 192 && N >= 256 && M >= 256;
  if ((K % G256N_BK) == 0) {
    const long tiles128 = (long)cdiv(M, 256) * cdiv(N, G256N_BN) * batch;
    const bool narrow = N > 64 && N < 256 && tiles128 >= 256;  // e.g. the 128-channel convolutions at 256^2 / 512^2
    // Round 6: problems too small for the 256x256 tiling (< 192 such tiles) but with >= 192 tiles of 256x128 -- the UNets' 1x1 convolutions / attention
    // projections at 16 384 x 384 .. 512, 4096 x 1536, 32 768 x 256 -- ran on the 128x128 kernel: 14.4 vs 17.2, 18.0 vs 20.2, 16.8 vs 19.3, 18.6 vs 20.4 us here
    // (tools/linear_shapes_probe.py, profiles/r06_linear_shapes_probe.txt; below 192 tiles the 128x128 kernel wins: 4096 x 512 11.0 vs 13.8 us).  Bit-identical.
    const bool mid = !big && N >= 256 && tiles128 >= 192;
    if (sel == 4 || (sel == 0 && (narrow || mid || (big && lfm_gemm_prefers_v4(M, N, K))))) return 4;
  }
  if ((K % G256Q_BK) != 0 || !(caps & GEMM_CAP_FITS)) return 1;
  if ((caps & GEMM_CAP_V6) && (sel == 6 || (sel == 0 && big && lfm_gemm_v6_default()))) return 6;
  if (sel == 5 || sel == 6 || (sel == 0 && big)) return 5;
  return 1;
}

// runs kernel `kern` (an answer of gemm_choose for these types and this shape)
template <class ASrc, class Epi>
static inline int launch_gemm_kernel(int kern, const ASrc& asrc, const half_t* W, long ldw, int M, int N, int K, const Epi& epi, hipStream_t stream,
                                     int batch = 1, long bsA = 0, long bsW = 0, long bsC = 0) {
  switch (kern) {
    case 4: return launch_gemm256n_tn(asrc, W, ldw, M, N, K, epi, stream, batch, bsA, bsW, bsC);
    case 5: return launch_gemm256h_tn(asrc, W, ldw, M, N, K, epi, stream, batch, bsA, bsW, bsC);
    case 6:
      if constexpr (gemm_v6_ok<ASrc, Epi>::value) return launch_gemm256w_tn(asrc, W, ldw, M, N, K, epi, stream, batch, bsA, bsW, bsC);
      else return LFM_ERR_ARG;
    default: return launch_gemm_tn(asrc, W, ldw, M, N, K, epi, stream, batch, bsA, bsW, bsC);
  }
}

template <class ASrc, class Epi>
static inline int launch_gemm_auto(const ASrc& asrc, const half_t* W, long ldw, int M, int N, int K, const Epi& epi, hipStream_t stream,
                                   int batch = 1, long bsA = 0, long bsW = 0, long bsC = 0) {
  return launch_gemm_kernel(gemm_choose(M, N, K, batch, gemm_caps<ASrc, Epi>(asrc, N, ldw)), asrc, W, ldw, M, N, K, epi, stream, batch, bsA, bsW, bsC);
}

// slices of a deep small-map problem on the 256x256 kernel (declared in gemm_kernel.h, which the 256x256 kernels include): slice bz = K range
// [bz ks, (bz + 1) ks) through the batch index, fp32 partial tile into slab[bz].  Returns 1 when the A source cannot take the kernel.
template <class ASrc, class Epi>
static inline int launch_gemm_splitk256(const ASrc& asrc, const half_t* W, long ldw, int M, int N, int ks, const EpiSlabF32& e, hipStream_t stream, int S) {
  if (!gemm_fits256(asrc, N, ldw)) return 1;
  return launch_gemm256h_tn(asrc, W, ldw, M, N, ks, e, stream, S, ks, ks, 0);
}
