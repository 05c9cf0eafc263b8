// GroupNorm on NHWC fp16: what the UNets' kernels (groupnorm_kernels.h, groupnorm_dispatch.h, ops.hip) and the VAE's (vae.hip) share -- the {mean, M2}
// slot arithmetic of the two-stage statistics, the closing mean / rstd step, the input view GnIn, the pixel walk of a thread that owns one channel
// octet, the row-wise statistics kernel, and the host constants of both launch policies.
#pragma once
#include "common.h"

// ------------------------------------------------------------------ GroupNorm statistics: {mean, M2} slots
// Deterministic two-stage statistics (the reference is deterministic; float atomics are not): every producer folds a slab of pixels into partial
// {mean, M2} slots, a second kernel merges the slots of a group in a fixed order.  Both stages are shifted, so that offset data (|mean| >> std)
// keeps its variance instead of losing it to the fp32 cancellation of sum(x^2) / n - mean^2.
// The slot of sums taken around the shift k: s = sum (x - k), q = sum (x - k)^2 over 1 / rc values.
__device__ __forceinline__ void gn_slot(float* o, float k, float s, float q, float rc) {
  o[0] = k + s * rc;
  o[1] = fmaxf(q - s * s * rc, 0.f);
}
// One step of the merge, shifted by K (the group's first slot mean): slot {mean m, M2} of c values adds
// sum (x - K) += c (m - K),  sum (x - K)^2 += M2 + c (m - K)^2 -- linear, so lanes and trees add as before.
__device__ __forceinline__ void gn_merge(float& sum, float& sq, const float* slot, float c, float K) {
  const float d = slot[0] - K;
  sum += c * d;
  sq += slot[1] + c * d * d;
}
// The closing step: sum = sum (x - K), sq = sum (x - K)^2 over cnt values -> the group's mean and 1 / sqrt(var + eps).
__device__ __forceinline__ void gn_mean_rstd(float K, float sum, float sq, float cnt, float eps, float& mean, float& rstd) {
  const float dl = sum / cnt;
  mean = K + dl;
  rstd = rsqrtf(fmaxf(sq / cnt - dl * dl, 0.f) + eps);
}

// GroupNorm input = the channel concat [a | b] of two NHWC tensors read in place (th.cat([h, hs.pop()], dim=1) feeding a ResBlock's first
// GroupNorm, unet.py:649 + :171: the concatenated tensor is never materialised); b == nullptr: a alone (Ca == C).  Ca % 8 == 0.
struct GnIn {
  const half_t* a;
  const half_t* b;
  int Ca, Cb;
  __device__ __forceinline__ const half_t* at(long pix, int c) const { return c < Ca ? a + pix * Ca + c : b + pix * Cb + (c - Ca); }
  // a thread that owns channel c of every pixel of image n: first pixel's address and the row stride of the tensor that holds c
  __device__ __forceinline__ const half_t* column(long pix0, int c, long& stride) const {
    const bool fa = c < Ca;
    stride = fa ? Ca : Cb;
    return fa ? a + pix0 * Ca + c : b + pix0 * Cb + (c - Ca);
  }
};

// The pixel walk of a thread that owns one channel octet: pixels p, p + step, ... below p1 of the column at `base` (rows `stride` halves apart), four
// independent 16-byte loads in flight (one per iteration ran at 1.5 TB/s), handed to f(v, pixel) in pixel order, then a tail of single loads.
// Used by gn_stats_rows_kernel and both passes of gn_fused_kernel.  The two apply kernels gn_affine_rows_kernel and gn_apply_kernel keep their own
// text of this loop: through this function each compiled to one or two more VGPRs than before (profiles/groupnorm_refactor.txt).
template <class F>
__device__ __forceinline__ void gn_walk(const half_t* base, long stride, int p, int p1, int step, F&& f) {
  for (; p + 3 * step < p1; p += 4 * step) {
    const half8_t v0 = *(const half8_t*)(base + (long)p * stride), v1 = *(const half8_t*)(base + (long)(p + step) * stride);
    const half8_t v2 = *(const half8_t*)(base + (long)(p + 2 * step) * stride), v3 = *(const half8_t*)(base + (long)(p + 3 * step) * stride);
    f(v0, p);
    f(v1, p + step);
    f(v2, p + 2 * step);
    f(v3, p + 3 * step);
  }
  for (; p < p1; p += step) f(*(const half8_t*)(base + (long)p * stride), p);
}

// Row-wise statistics (channels per group % 4 == 0, C / 8 <= 256): grid (slabs, images); a block reads a slab of pixels with FULL rows (coalesced);
// thread = channel octet x pixel row; the sums are of x - k, k = the slab's first value of the half-octet (every thread of the octet reads the same
// k); per half-octet partial sums are folded through LDS (fixed order) and leave as slot part[n][slab][C / 4 half-octets].
inline __global__ __launch_bounds__(256) void gn_stats_rows_kernel(GnIn in, float* __restrict__ part, int HW, int C, int pix_per_block) {
  __shared__ float red[4][256];
  const int n = blockIdx.y, c8n = C / 8, tid = threadIdx.x;
  const int rows = 256 / c8n;
  const int oct = tid % c8n, prow = tid / c8n;
  const int p0 = blockIdx.x * pix_per_block;
  const int p1 = min(p0 + pix_per_block, HW);
  float s[2] = {0.f, 0.f}, q[2] = {0.f, 0.f};  // per half-octet (4 channels): a group is >= 4 channels wide
  long XS;  // row stride of the tensor that holds this thread's octet
  const half_t* base = in.column((long)n * HW, oct * 8, XS);
  const float k[2] = {(float)base[(long)p0 * XS], (float)base[(long)p0 * XS + 4]};  // the shifts: pixel p0 of this slab, per half-octet
  if (prow < rows)
    gn_walk(base, XS, p0 + prow, p1, rows, [&](const half8_t& v, int) {  // summed in pixel order
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const float f = (float)v[j] - k[j >> 2];
        s[j >> 2] += f;
        q[j >> 2] += f * f;
      }
    });
  red[0][tid] = s[0];
  red[1][tid] = s[1];
  red[2][tid] = q[0];
  red[3][tid] = q[1];
  __syncthreads();
  if (tid < c8n) {  // fold the pixel-rows of this channel octet, then one {mean, M2} slot per half-octet
    for (int r = 1; r < rows; ++r) {
      s[0] += red[0][tid + r * c8n];
      s[1] += red[1][tid + r * c8n];
      q[0] += red[2][tid + r * c8n];
      q[1] += red[3][tid + r * c8n];
    }
    const float rc = 1.f / (float)((p1 - p0) * 4);
    float* o = part + (((long)n * gridDim.x + blockIdx.x) * (C / 4) + tid * 2) * 2;
    gn_slot(o, k[0], s[0], q[0], rc);
    gn_slot(o + 2, k[1], s[1], q[1], rc);
  }
}

// ------------------------------------------------------------------ host side
#define GN_MAX_SLABS 64  // statistics slabs per image of a full chip (UNets and VAE alike): bounds the partial buffer independently of HW
// Pixels per block of the row-walking kernels (statistics and apply): 16 .. 4 chunks per thread at 128 .. 512 channels.  (512 pixels per block at
// 64x64 maps left 256 blocks: one per CU; 128 made gn_coef's serial slab walk the longer kernel.)
static inline int gn_pixels_per_block(int HW) { return HW >= 4096 ? 256 : (HW >= 256 ? 64 : HW); }
// Launch the <true> or the <false> instantiation of a kernel templated on SiLU, 256 threads per block.
#define GN_LAUNCH_SILU(kernel, silu, grid, st, ...)                                    \
  do {                                                                                 \
    if (silu) hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, st, __VA_ARGS__);   \
    else hipLaunchKernelGGL(kernel<false>, grid, dim3(256), 0, st, __VA_ARGS__);       \
  } while (0)
