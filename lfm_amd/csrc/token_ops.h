// The two token-row ops of the SpatialTransformer's BasicTransformerBlock (attention.py:85-105, 218-240) that are no GEMM: lfm_layernorm_f16, lfm_geglu_f16.
// Both are memory-bound, keep nothing in the LDS, move 16-byte chunks, compute in fp32 and round to fp16 once; 64-bit offsets, no workspace, graph-capturable.
//
// LayerNorm (nn.LayerNorm(C), biased variance): ONE WAVE PER ROW, four rows per 256-thread workgroup; lane l takes the chunks l, l + 64, ... of the row.
// Statistics in fp32 in two passes -- the mean first, then the sum of (x - mean)^2 -- never E[x^2] - E[x]^2, which loses every digit of the variance once
// |mean| >> spread (rows offset by +200: tests/test_layout_ref.py shows that form outside the bound).  The row is read three times (mean, centred squares,
// apply); it is at most a few KiB and the second and third reads come from the cache of the CU that made the first, so no register image bounds C.
//
// GEGLU: y[m][i] = h[m][i] * gelu(h[m][I + i]) with the EXACT GELU g Phi(g) of F.gelu's default, written 0.5 g erfc(-g / sqrt 2): erfc keeps its relative
// accuracy where 1 + erf(g / sqrt 2) cancels (negative gates): gelu_erf_f of common.h, shared with the GEMM epilogue ActGeluErf.  The library's gelu_tanh_f is
// the tanh form of another model and is not this function.
//
// Token + position embedding of the layout encoder (x_transformer.py:586-587, TransformerWrapper: token_emb(ids) + pos_emb(arange(L))): lfm_token_embed_f16,
// one 8-column chunk per thread, fp32 tables, one fp32 add, one rounding to fp16.  The ids are read on the device (no readback: a captured replay follows ids
// rewritten in place); an id outside the table poisons its row with NaN and reads nothing.
#pragma once
#include "common.h"

__global__ __launch_bounds__(256) void layernorm_rows_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, const float* __restrict__ gamma,
                                                             const float* __restrict__ beta, long M, int C8, float eps) {
  const int lane = threadIdx.x & 63;
  const long row = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= M) return;  // wave-uniform
  const half8_t* xr = (const half8_t*)x + row * C8;
  const float inv_c = 1.0f / (float)(C8 * 8);
  float s = 0.f;
  for (int c = lane; c < C8; c += 64) {
    const half8_t v = xr[c];
#pragma unroll
    for (int i = 0; i < 8; ++i) s += (float)v[i];
  }
  const float mean = wave_sum(s) * inv_c;
  float ss = 0.f;
  for (int c = lane; c < C8; c += 64) {
    const half8_t v = xr[c];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float d = (float)v[i] - mean;
      ss += d * d;
    }
  }
  const float rstd = 1.0f / sqrtf(wave_sum(ss) * inv_c + eps);
  half8_t* yr = (half8_t*)y + row * C8;
  for (int c = lane; c < C8; c += 64) {
    const half8_t v = xr[c];
    const f32x4 g0 = *(const f32x4*)(gamma + c * 8), g1 = *(const f32x4*)(gamma + c * 8 + 4);
    const f32x4 b0 = *(const f32x4*)(beta + c * 8), b1 = *(const f32x4*)(beta + c * 8 + 4);
    half8_t o;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = (half_t)(((float)v[i] - mean) * rstd * g0[i] + b0[i]);
      o[4 + i] = (half_t)(((float)v[4 + i] - mean) * rstd * g1[i] + b1[i]);
    }
    yr[c] = o;
  }
}

extern "C" int lfm_layernorm_f16(const void* x, void* y, const float* gamma, const float* beta, long M, int C, float eps, lfm_stream_t stream) {
  if (!x || !y || !gamma || !beta) return LFM_ERR_ARG;
  if (M <= 0 || C <= 0 || C % 8 || (M + 3) / 4 >= (1L << 31)) return LFM_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)gamma | (uintptr_t)beta) & 15) return LFM_ERR_ALIGN;
  hipLaunchKernelGGL(layernorm_rows_kernel, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, (hipStream_t)stream, (const half_t*)x, (half_t*)y, gamma, beta, M,
                     C / 8, eps);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

__global__ __launch_bounds__(256) void geglu_kernel(const half_t* __restrict__ h, long ldh, half8_t* __restrict__ y, int I8, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long m = e / I8;
  const int c = (int)(e - m * I8);
  const half_t* hr = h + m * ldh + c * 8;
  const half8_t a = *(const half8_t*)hr, g = *(const half8_t*)(hr + (long)I8 * 8);
  half8_t o;
#pragma unroll
  for (int i = 0; i < 8; ++i) o[i] = (half_t)((float)a[i] * gelu_erf_f((float)g[i]));
  y[e] = o;
}

extern "C" int lfm_geglu_f16(const void* h, long ldh, void* y, long M, int I, lfm_stream_t stream) {
  if (!h || !y) return LFM_ERR_ARG;
  if (M <= 0 || I <= 0 || I % 8 || ldh < 2L * I) return LFM_ERR_SHAPE;
  if ((ldh % 8) || (((uintptr_t)h | (uintptr_t)y) & 15)) return LFM_ERR_ALIGN;
  const long total = M * (I / 8);
  if ((total + 255) / 256 >= (1L << 31)) return LFM_ERR_SHAPE;
  hipLaunchKernelGGL(geglu_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (const half_t*)h, ldh, (half8_t*)y, I / 8, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

__global__ __launch_bounds__(256) void token_embed_kernel(const float* __restrict__ tok, int vocab, const float* __restrict__ pos, const long long* __restrict__ ids,
                                                          half8_t* __restrict__ out, int L, int D8, long total) {
  const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  const long m = e / D8;  // row n * L + p
  const int c = (int)(e - m * D8);
  const int p = (int)(m % L);
  const long long id = ids[m];
  half8_t o;
  if (id < 0 || id >= vocab) {  // nn.Embedding raises in the reference; poison instead of reading out of bounds
    const half_t nan = (half_t)__builtin_nanf("");
#pragma unroll
    for (int i = 0; i < 8; ++i) o[i] = nan;
  } else {
    const float* tr = tok + (id * D8 + c) * 8;
    const float* pr = pos + ((long)p * D8 + c) * 8;
    const f32x4 t0 = *(const f32x4*)tr, t1 = *(const f32x4*)(tr + 4), p0 = *(const f32x4*)pr, p1 = *(const f32x4*)(pr + 4);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      o[i] = (half_t)(t0[i] + p0[i]);
      o[4 + i] = (half_t)(t1[i] + p1[i]);
    }
  }
  out[e] = o;
}

extern "C" int lfm_token_embed_f16(const float* tok_emb, int vocab, const float* pos_emb, int pos_rows, const void* ids_int64, void* out, int N, int L, int D,
                                   lfm_stream_t stream) {
  if (!tok_emb || !pos_emb || !ids_int64 || !out) return LFM_ERR_ARG;
  if (vocab <= 0 || pos_rows <= 0 || N <= 0 || L <= 0 || D <= 0 || D % 8 || L > pos_rows) return LFM_ERR_SHAPE;
  if ((((uintptr_t)tok_emb | (uintptr_t)pos_emb | (uintptr_t)ids_int64 | (uintptr_t)out) & 15)) return LFM_ERR_ALIGN;
  const long total = (long)N * L * (D / 8);
  if ((total + 255) / 256 >= (1L << 31)) return LFM_ERR_SHAPE;
  hipLaunchKernelGGL(token_embed_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, (hipStream_t)stream, tok_emb, vocab, pos_emb,
                     (const long long*)ids_int64, (half8_t*)out, L, D / 8, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
