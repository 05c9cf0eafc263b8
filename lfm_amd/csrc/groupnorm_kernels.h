// ------------------------------------------------------------------ general GroupNorm(32 groups) on NHWC fp16
// 1) stats: one block per (image, pixel-slab) [fast path] or (group, image, pixel-slab) -> per-block PARTIAL {mean, M2} slots; the block's sums
//           are of x - k, k = the slab's first value of the half-octet / group (read by every thread), so offset data (|mean| >> std) keeps its
//           variance instead of losing it to the fp32 cancellation of sum(x^2) / n - mean^2
// 2) coef : per (n, c): merges the partials of its group in a FIXED order (deterministic: the reference is; atomics are not), shifted by the
//           group's first slot mean, then
//           a = rstd*gamma*(1+scale),  b = (beta - mean*rstd*gamma)*(1+scale) + shift     (FiLM optional)
// 3) apply: y = silu?(x*a + b), 8 channels per thread
// GnIn (one tensor, or the channel concat of two read in place), the row-wise statistics kernel gn_stats_rows_kernel (cpg % 4 == 0, C / 8 <= 256),
// the pixel walk gn_walk and the slot / merge / closing arithmetic gn_slot, gn_merge, gn_mean_rstd: groupnorm_common.h.  Which kernels serve a
// shape: groupnorm_dispatch.h.
#pragma once
#include "groupnorm_common.h"

template <int VEC>
__global__ __launch_bounds__(256) void gn_stats_general_kernel(GnIn in, float* __restrict__ part, int HW, int C, int cpg,
                                                               int pix_per_block, int G) {
  const int g = blockIdx.x, n = blockIdx.y;
  const int p0 = blockIdx.z * pix_per_block, p1 = min(p0 + pix_per_block, HW);
  const int vpp = cpg / VEC;  // vectors per pixel in this group
  const long total = (long)(p1 - p0) * vpp;
  const float k = (float)*in.at((long)n * HW + p0, g * cpg);  // the shift: the slab's first value of the group
  float s = 0.f, q = 0.f;
  for (long e = threadIdx.x; e < total; e += 256) {
    const int p = p0 + (int)(e / vpp), v = (int)(e % vpp);
    const half_t* ptr = in.at((long)n * HW + p, g * cpg + v * VEC);
    if (VEC == 4) {
      const half4_t h = *(const half4_t*)ptr;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const float f = (float)h[j] - k;
        s += f;
        q += f * f;
      }
    } else {
      const float f = (float)ptr[0] - k;
      s += f;
      q += f * f;
    }
  }
  __shared__ float rs[4], rq[4];
  s = wave_sum(s);
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0) {
    rs[threadIdx.x >> 6] = s;
    rq[threadIdx.x >> 6] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {  // slot [n][slab][g] = {mean, M2}
    float* o = part + (((long)n * gridDim.z + blockIdx.z) * G + g) * 2;
    const float ss = rs[0] + rs[1] + rs[2] + rs[3], qq = rq[0] + rq[1] + rq[2] + rq[3], rc = 1.f / (float)total / (float)VEC;
    gn_slot(o, k, ss, qq, rc);
  }
}

// rows != 0: partials are [n][slab][C/4 half-octets] (fast path);  rows == 0: [n][slab][G].  Slot {mean m, M2} of slab b holds
// c = min(ppb, HW - b ppb) x (4 | cpg) values; merged shifted by the group's first slot mean K: sum (x - K) = sum c (m - K), sum (x - K)^2 = sum M2 + c (m - K)^2
__global__ void gn_coef_kernel(const float* __restrict__ part, int slabs, int rows, const float* __restrict__ gamma, const float* __restrict__ beta,
                               const float* __restrict__ film, long film_stride, float* __restrict__ ab, int N, int C, int cpg, int HW, int ppb,
                               float eps, int G) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= N * C) return;
  const int n = i / C, c = i - n * C, g = c / cpg;
  float sum = 0.f, sq = 0.f, K;  // every channel of a group folds the same slots in the same order: identical, deterministic statistics
  if (rows) {
    const int h0 = g * (cpg / 4), h1 = h0 + cpg / 4, Q = C / 4;
    K = part[((long)n * slabs * Q + h0) * 2];
#pragma unroll 4
    for (int b = 0; b < slabs; ++b) {
      const float* p = part + ((long)n * slabs + b) * Q * 2;
      const float cb = (float)(4 * min(ppb, HW - b * ppb));
      for (int h = h0; h < h1; ++h) gn_merge(sum, sq, p + 2 * h, cb, K);
    }
  } else {
    K = part[((long)n * slabs * G + g) * 2];
    for (int b = 0; b < slabs; ++b) {
      const float* p = part + (((long)n * slabs + b) * G + g) * 2;
      gn_merge(sum, sq, p, (float)(cpg * min(ppb, HW - b * ppb)), K);
    }
  }
  float mean, rstd;
  gn_mean_rstd(K, sum, sq, (float)HW * (float)cpg, eps, mean, rstd);
  float a = rstd * gamma[c], b = beta[c] - mean * rstd * gamma[c];
  if (film) {  // h = norm(h) * (1 + scale) + shift   (unet.py:229-232; film row = [scale(C) | shift(C)])
    const float sc = 1.0f + film[(long)n * film_stride + c], sh = film[(long)n * film_stride + C + c];
    a *= sc;
    b = b * sc + sh;
  }
  ab[(long)i * 2] = a;
  ab[(long)i * 2 + 1] = b;
}

template <bool SILU>
__global__ __launch_bounds__(256) void gn_affine_kernel(GnIn in, half_t* __restrict__ y, const float* __restrict__ ab,
                                                        int HW, int C, long total8) {
  // grid (chunks of one image / 256, images): 32-bit index arithmetic only (HW * C / 8 < 2^31 per image)
  const int c8n = C / 8, n = blockIdx.y;
  const unsigned j = blockIdx.x * 256u + threadIdx.x;
  if (j >= (unsigned)HW * (unsigned)c8n) return;
  const unsigned pix = j / (unsigned)c8n;
  const int c0 = (int)(j - pix * (unsigned)c8n) * 8;
  const long i = (long)n * HW * c8n + j;
  (void)total8;
  const half8_t v = *(const half8_t*)in.at((long)n * HW + pix, c0);
  const f32x4* p = (const f32x4*)(ab + ((long)n * C + c0) * 2);
  half8_t o;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const f32x4 t = p[j];  // a0 b0 a1 b1
    float f0 = (float)v[2 * j] * t.x + t.y, f1 = (float)v[2 * j + 1] * t.z + t.w;
    if (SILU) {
      f0 = silu_f(f0);
      f1 = silu_f(f1);
    }
    o[2 * j] = (half_t)f0;
    o[2 * j + 1] = (half_t)f1;
  }
  ((half8_t*)y)[i] = o;
}
// The same apply for channel counts whose octets divide the block (256 % (C / 8) == 0: 256 / 512 / 1024 / 2048 channels, every large map of the
// UNets): a thread owns ONE channel octet -- its 16 coefficients stay in registers -- and walks the pixels of its block's slab, four 16-byte
// chunks in flight; no per-chunk 64-bit div / mod, no 64 bytes of coefficient loads per 16 bytes of data (round 4; same arithmetic per element).
template <bool SILU>
__global__ __launch_bounds__(256) void gn_affine_rows_kernel(GnIn in, half_t* __restrict__ y, const float* __restrict__ ab, int HW, int C,
                                                             int pix_per_block) {
  const int n = blockIdx.y, c8n = C / 8, tid = threadIdx.x;
  const int oct = tid % c8n, prow = tid / c8n, pstride = 256 / c8n;
  const f32x4* cp = (const f32x4*)(ab + ((long)n * C + oct * 8) * 2);
  f32x4 t[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) t[j] = cp[j];  // a0 b0 a1 b1
  long XS;
  const half_t* xb = in.column((long)n * HW, oct * 8, XS);
  half_t* yb = y + ((long)n * HW) * C + oct * 8;
  auto one = [&](const half8_t v) {
    half8_t o;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float f0 = (float)v[2 * j] * t[j].x + t[j].y, f1 = (float)v[2 * j + 1] * t[j].z + t[j].w;
      if (SILU) {
        f0 = silu_f(f0);
        f1 = silu_f(f1);
      }
      o[2 * j] = (half_t)f0;
      o[2 * j + 1] = (half_t)f1;
    }
    return o;
  };
  const int p0 = blockIdx.x * pix_per_block, p1 = min(p0 + pix_per_block, HW);
  int p = p0 + prow;
  for (; p + 3 * pstride < p1; p += 4 * pstride) {  // (gn_walk's loop in its own text: see there)
    half8_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const half8_t*)(xb + (long)(p + u * pstride) * XS);
#pragma unroll
    for (int u = 0; u < 4; ++u) *(half8_t*)(yb + (long)(p + u * pstride) * C) = one(v[u]);
  }
  for (; p < p1; p += pstride) *(half8_t*)(yb + (long)p * C) = one(*(const half8_t*)(xb + (long)p * XS));
}

// Fused small-tensor path (one launch instead of three): one block per (image, chunk of GPB groups) streams its channels of every pixel twice
// (the second pass hits the L2): pass 1 per-group {sum, sumsq} with a fixed-order block reduction, pass 2 y = silu?(x*a + b) with the
// per-channel a, b (FiLM folded) held in registers.  cpg % 8 == 0, HW <= 1024: the GroupNorms of the UNets' lower resolutions, where the
// three-kernel path is launch-bound.
template <bool SILU>
__global__ __launch_bounds__(256) void gn_fused_kernel(GnIn in, half_t* __restrict__ y, const float* __restrict__ gamma,
                                                       const float* __restrict__ beta, const float* __restrict__ film, long film_stride, int HW,
                                                       int C, int cpg, int gpb, float eps) {
  __shared__ float red[2][256];
  __shared__ float mr[2][32];
  __shared__ float ks[32];  // the shift of every group of the block
  const int n = blockIdx.y, tid = threadIdx.x;
  const int CW = gpb * cpg, o8 = CW >> 3;          // channels / octets of this block
  const int oct = tid % o8, prow = tid / o8, rows = 256 / o8;
  const int c0 = blockIdx.x * CW + oct * 8;         // first channel of this thread's octet
  long XS;  // row stride of the tensor that holds this thread's octet
  const half_t* xb = in.column((long)n * HW, c0, XS);
  const int gl = (oct * 8) / cpg;  // this thread's group within the block
  // the shift: pixel 0, first channel of the group (every thread of the group reads the same value, so the partial sums below add linearly)
  const float k = (float)*in.at((long)n * HW, blockIdx.x * CW + gl * cpg);
  if (tid == gl * (cpg >> 3)) ks[gl] = k;  // (prow 0, the group's first octet)
  float s = 0.f, q = 0.f;
  if (prow < rows)  // (the block is alone on its CU: latency, not bandwidth, bound it)
    gn_walk(xb, XS, prow, HW, rows, [&](const half8_t& v, int) {
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[j] - k;
        s += f;
        q += f * f;
      }
    });
  red[0][tid] = s;
  red[1][tid] = q;
  __syncthreads();
  if (tid < gpb) {  // group tid of this block: octets [tid*cpg/8, (tid+1)*cpg/8) of every pixel row, folded in a fixed order
    const int ob = tid * (cpg >> 3), oe = ob + (cpg >> 3);
    float ss = 0.f, qq = 0.f;
    for (int r = 0; r < rows; ++r)
      for (int o = ob; o < oe; ++o) {
        ss += red[0][r * o8 + o];
        qq += red[1][r * o8 + o];
      }
    gn_mean_rstd(ks[tid], ss, qq, (float)HW * (float)cpg, eps, mr[0][tid], mr[1][tid]);  // the group's shift + the mean of x - shift
  }
  __syncthreads();
  if (prow >= rows) return;
  const float mean = mr[0][gl], rstd = mr[1][gl];
  float a[8], b[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const int c = c0 + j;
    a[j] = rstd * gamma[c];
    b[j] = beta[c] - mean * a[j];
    if (film) {
      const float sc = 1.0f + film[(long)n * film_stride + c], sh = film[(long)n * film_stride + C + c];
      a[j] *= sc;
      b[j] = b[j] * sc + sh;
    }
  }
  half_t* yb = y + (long)n * HW * C + c0;
  gn_walk(xb, XS, prow, HW, rows, [&](const half8_t& v, int p) {
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = (float)v[j] * a[j] + b[j];
      if (SILU) f = silu_f(f);
      o[j] = (half_t)f;
    }
    *(half8_t*)(yb + (long)p * C) = o;
  });
}
