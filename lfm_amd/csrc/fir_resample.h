// The [1,3,3,1] FIR resampling of EDM's Conv2d (reference models/EDM.py:96-132) for NCSN++ (SongUNet with resample_filter = [1,3,3,1]), and the zero-border
// copy that turns the existing pad-1 3x3 convolutions into the pad-2 convolution of the fused "convolve, then filter down" path (:116-118).
// Included from ops.hip.  NHWC fp16, C % 8 == 0, 16 bytes per thread along the channels, fp32 arithmetic, ONE rounding to fp16; one thread per
// (output pixel, channel octet), as lfm_avgpool2_f16 / lfm_upsample2_f16: stream-ordered, no workspace, graph-capturable.
//
// The filter is separable, f2 = outer(f, f) / 64 with f = [1,3,3,1], and is applied as such: a row sum (x0 + x3) + 3 (x1 + x2) per input row, the same over
// the four row sums, one multiplication by 1/64 (a power of two: exact).  On integer-valued inputs every step is exact, and at most nine fp32 roundings lie
// between the fp16 inputs and the one fp16 rounding of the output (the Gaussian-input test's accumulation term).
//
// The border of the first aux_residual's fp32 NCHW input is made by a kernel as well (lfm_zero_border_f32), not by a slice copy into a zeroed buffer: a
// zero-fill inside a captured graph would be a memset node, which the host-sequenced UNets keep out of their graphs (common.h: lfm_zero_async).
#pragma once
#include "common.h"

__device__ __forceinline__ float fir4(float a, float b, float c, float d) { return (a + d) + 3.0f * (b + c); }

// y[n, oy, ox, :] = ((sum_{a,b<4} f[a] f[b] x[n, 2 oy - PAD + a, 2 ox - PAD + b, :]) / 64 (+ bias) (+ resid[n, oy, ox, :])) * scale, zeros outside the
// Hi x Wi input; Hi = 2 Ho + 2 - 2 PAD (PAD 1: every row / column index is checked; PAD 0: all 16 taps are inside by construction)
template <int PAD, bool EPI>
__global__ __launch_bounds__(256) void fir_down2_kernel(const half8_t* __restrict__ x, half8_t* __restrict__ y, const float* __restrict__ bias,
                                                        const half8_t* __restrict__ resid, float scale, int Ho, int Wo, int C8, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C8);
  const long p = i / C8;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const long n = p / ((long)Wo * Ho);
  const int Hi = 2 * Ho + 2 - 2 * PAD, Wi = 2 * Wo + 2 - 2 * PAD;
  const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  float rows[4][8];
#pragma unroll
  for (int a = 0; a < 4; ++a) {
    const int iy = 2 * oy - PAD + a;
    const bool yin = PAD == 0 || (unsigned)iy < (unsigned)Hi;
    half8_t v[4];
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int ix = 2 * ox - PAD + b;
      const bool in = yin && (PAD == 0 || (unsigned)ix < (unsigned)Wi);
      v[b] = in ? x[((n * Hi + iy) * Wi + ix) * C8 + c] : zero;
    }
#pragma unroll
    for (int j = 0; j < 8; ++j) rows[a][j] = fir4((float)v[0][j], (float)v[1][j], (float)v[2][j], (float)v[3][j]);
  }
  half8_t r = zero;
  float bv[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
  if (EPI) {
    if (resid) r = resid[i];
    if (bias) {
#pragma unroll
      for (int j = 0; j < 8; ++j) bv[j] = bias[c * 8 + j];
    }
  }
  half8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float s = fir4(rows[0][j], rows[1][j], rows[2][j], rows[3][j]) * 0.015625f;
    if (EPI) s = ((s + bv[j]) + (float)r[j]) * scale;
    o[j] = (half_t)s;
  }
  y[i] = o;
}

// y[n, oy, ox, :] of the transposed filter 4 f2 at stride 2, pad 1 (models/EDM.py:120-123): per axis y[2i] = (3 x[i] + x[i-1]) / 4, y[2i+1] = (3 x[i] + x[i+1]) / 4,
// zeros outside the Ho/2 x Wo/2 input -- four taps with the weights {9, 3, 3, 1} / 16
__global__ __launch_bounds__(256) void fir_up2_kernel(const half8_t* __restrict__ x, half8_t* __restrict__ y, int Ho, int Wo, int C8, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C8);
  const long p = i / C8;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const long n = p / ((long)Wo * Ho);
  const int Hi = Ho / 2, Wi = Wo / 2;
  const int y0 = oy >> 1, x0 = ox >> 1;                        // the near input row / column (weight 3)
  const int y1 = y0 + ((oy & 1) ? 1 : -1), x1 = x0 + ((ox & 1) ? 1 : -1);  // the far one (weight 1): may lie outside
  const bool yin = (unsigned)y1 < (unsigned)Hi, xin = (unsigned)x1 < (unsigned)Wi;
  const half8_t zero = {0, 0, 0, 0, 0, 0, 0, 0};
  const half8_t* b = x + n * Hi * Wi * C8 + c;
  const half8_t nn = b[((long)y0 * Wi + x0) * C8];
  const half8_t nf = xin ? b[((long)y0 * Wi + x1) * C8] : zero;
  const half8_t fn = yin ? b[((long)y1 * Wi + x0) * C8] : zero;
  const half8_t ff = (yin && xin) ? b[((long)y1 * Wi + x1) * C8] : zero;
  half8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const float near = 3.0f * (float)nn[j] + (float)nf[j], far = 3.0f * (float)fn[j] + (float)ff[j];
    o[j] = (half_t)((3.0f * near + far) * 0.0625f);
  }
  y[i] = o;
}

// y [planes][H + 2][W + 2][inner] = x [planes][H][W][inner] inside a one-pixel border of zeros; T = half8_t with inner = C / 8 (NHWC fp16, planes = N) or
// float with inner = 1 (NCHW fp32, planes = N * C)
template <typename T>
__global__ __launch_bounds__(256) void zero_border_kernel(const T* __restrict__ x, T* __restrict__ y, int H, int W, int inner, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % inner);
  const long p = i / inner;
  const int ox = (int)(p % (W + 2)), oy = (int)((p / (W + 2)) % (H + 2));
  const long n = p / ((long)(W + 2) * (H + 2));
  T v = {};
  if (ox >= 1 && ox <= W && oy >= 1 && oy <= H) v = x[((n * H + (oy - 1)) * W + (ox - 1)) * inner + c];
  y[i] = v;
}

static inline bool fir_grid_ok(long total) { return total > 0 && (total + 255) / 256 < (1L << 31); }  // one thread per 16 bytes of output: the grid's x limit

extern "C" int lfm_fir_down2_f16(const void* x, void* y, const float* bias, const void* resid, float scale, int N, int Ho, int Wo, int C, int pad,
                                 lfm_stream_t stream) {
  if (!x || !y) return LFM_ERR_ARG;
  if (N <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || C % 8 || (pad != 0 && pad != 1)) return LFM_ERR_SHAPE;
  if ((((uintptr_t)x | (uintptr_t)y | (uintptr_t)resid) & 15) || ((uintptr_t)bias & 3)) return LFM_ERR_ALIGN;
  const long total = (long)N * Ho * Wo * (C / 8);
  if (!fir_grid_ok(total)) return LFM_ERR_SHAPE;
  const dim3 grid((unsigned)((total + 255) / 256));
  const bool epi = bias || resid || scale != 1.0f;
  hipStream_t st = (hipStream_t)stream;
#define FIR_DOWN(PAD, EPI)                                                                                                                     \
  hipLaunchKernelGGL((fir_down2_kernel<PAD, EPI>), grid, dim3(256), 0, st, (const half8_t*)x, (half8_t*)y, bias, (const half8_t*)resid, scale, Ho, Wo, \
                     C / 8, total)
  if (pad && epi) FIR_DOWN(1, true);
  else if (pad) FIR_DOWN(1, false);
  else if (epi) FIR_DOWN(0, true);
  else FIR_DOWN(0, false);
#undef FIR_DOWN
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_fir_up2_f16(const void* x, void* y, int N, int Ho, int Wo, int C, lfm_stream_t stream) {
  if (!x || !y) return LFM_ERR_ARG;
  if (N <= 0 || Ho <= 0 || Wo <= 0 || ((Ho | Wo) & 1) || C <= 0 || C % 8) return LFM_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return LFM_ERR_ALIGN;
  const long total = (long)N * Ho * Wo * (C / 8);
  if (!fir_grid_ok(total)) return LFM_ERR_SHAPE;
  hipLaunchKernelGGL(fir_up2_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half8_t*)x, (half8_t*)y, Ho, Wo, C / 8,
                     total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_zero_border_f16(const void* x, void* y, int N, int H, int W, int C, lfm_stream_t stream) {
  if (!x || !y) return LFM_ERR_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || C <= 0 || C % 8) return LFM_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)y) & 15) return LFM_ERR_ALIGN;
  const long total = (long)N * (H + 2) * (W + 2) * (C / 8);
  if (!fir_grid_ok(total)) return LFM_ERR_SHAPE;
  hipLaunchKernelGGL(zero_border_kernel<half8_t>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half8_t*)x, (half8_t*)y, H,
                     W, C / 8, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_zero_border_f32(const float* x, float* y, int planes, int H, int W, lfm_stream_t stream) {
  if (!x || !y) return LFM_ERR_ARG;
  if (planes <= 0 || H <= 0 || W <= 0) return LFM_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)y) & 3) return LFM_ERR_ALIGN;
  const long total = (long)planes * (H + 2) * (W + 2);
  if (!fir_grid_ok(total)) return LFM_ERR_SHAPE;
  hipLaunchKernelGGL(zero_border_kernel<float>, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, x, y, H, W, 1, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
