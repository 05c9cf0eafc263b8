// UNet attention behind lfm_attention_small_f16: the launch, and which kernel (VALU, resident MFMA, streamed MFMA) serves a shape.  unet_attention_choose is the ONE place
// that knows (lfm_unet_attention_plan returns its answer for 16-byte-aligned operands without a launch: the truth table of tests/test_unet_attention_ref.py): flag
// UNET_ATT_VALU decides first, then the four resident shapes, then whatever the VALU kernel's LDS admits; only the rest is streamed, so nothing served before it existed moved.
#pragma once
#include "debug_flags.h"
#include "unet_attention_kernel.h"
#include "unet_attention_stream_kernel.h"

enum { UNET_ATT_VALU = 1, UNET_ATT_RESIDENT = 2, UNET_ATT_STREAM = 3 };
static inline size_t unet_attention_valu_lds(int T, int ch) {  // S fp32 [min(T, 64)][T + 1], then K, V fp16 [T][ch + 2]
  return (size_t)(T < 64 ? T : 64) * ((size_t)T + 1) * 4 + (size_t)4 * T * ((size_t)ch + 2);
}
// aligned: qkv and out on 16-byte boundaries.  The MFMA kernels read and write 16-byte chunks; other operands get the VALU kernel where it fits.
static inline int unet_attention_choose(int T, int heads, int ch, bool aligned) {
  if (T <= 0 || heads <= 0 || ch <= 0) return LFM_ERR_SHAPE;
  const bool valu_fits = unet_attention_valu_lds(T, ch) <= 160 * 1024;
  const bool stream_fits = aligned && ch % 16 == 0 && ch <= 256;
  const int stream = lfm_unet_attention_stream_mode();
  if (lfm_gemm_debug_flags() & LFM_DBG_UNET_ATT_VALU) return valu_fits ? UNET_ATT_VALU : LFM_ERR_SHAPE;  // flag: the VALU kernel or nothing (A/B)
  if (stream == 2 && stream_fits) return UNET_ATT_STREAM;  // parity tests and A/B: every shape the streamed kernel takes
  if (aligned && (T == 64 || T == 256) && (ch == 64 || ch == 128)) return UNET_ATT_RESIDENT;
  if (valu_fits) return UNET_ATT_VALU;
  if (stream && stream_fits) return UNET_ATT_STREAM;
  return LFM_ERR_SHAPE;
}
extern "C" int lfm_unet_attention_plan(int N, int T, int heads, int ch) {
  return N <= 0 ? LFM_ERR_SHAPE : unet_attention_choose(T, heads, ch, true);
}

static int launch_attention_unet_valu(const half_t* qkv, half_t* out, int N, int T, int heads, int ch, hipStream_t st) {
  const int QB = T < 64 ? T : 64;  // queries per workgroup
  if (!lfm_kernel_lds<&attention_small_kernel>(160 * 1024)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL(attention_small_kernel, dim3(heads, N, cdiv(T, QB)), dim3(256), unet_attention_valu_lds(T, ch), st, qkv, out, T, heads, ch, QB);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_attention_small_f16(const void* qkv, void* out, int N, int T, int heads, int ch, lfm_stream_t stream) {
  if (!qkv || !out) return LFM_ERR_ARG;
  if (N <= 0 || T <= 0 || heads <= 0 || ch <= 0) return LFM_ERR_SHAPE;
  const half_t* qi = (const half_t*)qkv;
  half_t* oi = (half_t*)out;
  hipStream_t st = (hipStream_t)stream;
  switch (unet_attention_choose(T, heads, ch, !(((uintptr_t)qkv | (uintptr_t)out) & 15))) {
    case UNET_ATT_RESIDENT:
      if (T == 256 && ch == 128) return launch_attention_unet_mfma<128, 256>(qi, oi, N, heads, st);
      if (T == 256 && ch == 64) return launch_attention_unet_mfma<64, 256>(qi, oi, N, heads, st);
      if (T == 64 && ch == 128) return launch_attention_unet_mfma<128, 64>(qi, oi, N, heads, st);
      return launch_attention_unet_mfma<64, 64>(qi, oi, N, heads, st);
    case UNET_ATT_STREAM: return attention_unet_stream_launch(qi, oi, N, T, heads, ch, st);
    case UNET_ATT_VALU: return launch_attention_unet_valu(qi, oi, N, T, heads, ch, st);
    default: return LFM_ERR_SHAPE;
  }
}
