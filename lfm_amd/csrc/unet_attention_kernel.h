// Attention of the UNets with every key of a head in the LDS (QKVAttentionLegacy, unet.py:310-334): the VALU kernel and the resident MFMA kernel; which shapes they
// and the streamed kernel serve: unet_attention_dispatch.h.  qkv: fp16 [N*T, 3*C], column layout [head][q | k | v][ch] (what reshape(bs*heads, 3*ch, T).split(ch) means
// for a token-major tensor); out: fp16 [N*T, C] with columns [head][ch].  softmax((q*s)(k*s)^T) v with s = ch^-1/4, fp32 softmax.  The VALU kernel: any ch; K, V of a head
// as fp16 rows plus a 64-query fp32 score block in the LDS, which bounds T (314 tokens at ch = 64, 127 at ch = 256); one workgroup per (head, image, 64 queries).
#pragma once
#include "unet_attention_common.h"

__global__ __launch_bounds__(256) void attention_small_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out, int T, int heads, int ch, int QB) {
  extern __shared__ __attribute__((aligned(16))) char smraw[];  // S fp32 [QB][T+1], then K, V fp16 [T][ch+2]: unet_attention_valu_lds (unet_attention_dispatch.h)
  const int head = blockIdx.x, n = blockIdx.y, q0 = blockIdx.z * QB, tid = threadIdx.x;
  const int nq = min(QB, T - q0);
  const int C = heads * ch, ldq = 3 * C, ks = ch + 2;
  float* S = (float*)smraw;
  half_t* Ks = (half_t*)(S + QB * (T + 1));
  half_t* Vs = Ks + T * ks;
  const half_t* base = qkv + (long)n * T * ldq + head * 3 * ch;
  for (int e = tid; e < T * ch; e += 256) {
    const int t = e / ch, c = e - t * ch;
    Ks[t * ks + c] = base[(long)t * ldq + ch + c];
    Vs[t * ks + c] = base[(long)t * ldq + 2 * ch + c];
  }
  __syncthreads();
  const float scale = rsqrtf((float)ch);  // (ch^-1/4)^2
  for (int e = tid; e < nq * T; e += 256) {
    const int t = e / T, s = e - t * T;
    const half_t* q = base + (long)(q0 + t) * ldq;
    float a = 0.f;
    for (int c = 0; c < ch; ++c) a += (float)q[c] * (float)Ks[s * ks + c];
    S[t * (T + 1) + s] = a * scale;
  }
  __syncthreads();
  for (int t = tid; t < nq; t += 256) {
    float* r = S + t * (T + 1);
    float mx = r[0];
    for (int s = 1; s < T; ++s) mx = fmaxf(mx, r[s]);
    float sum = 0.f;
    for (int s = 0; s < T; ++s) {
      r[s] = __expf(r[s] - mx);
      sum += r[s];
    }
    const float inv = 1.0f / sum;
    for (int s = 0; s < T; ++s) r[s] *= inv;
  }
  __syncthreads();
  half_t* ob = out + ((long)n * T + q0) * C + head * ch;
  for (int e = tid; e < nq * ch; e += 256) {
    const int t = e / ch, c = e - t * ch;
    const float* r = S + t * (T + 1);
    float a = 0.f;
    for (int s = 0; s < T; ++s) a += r[s] * (float)Vs[s * ks + c];
    ob[(long)t * C + c] = (half_t)a;
  }
}

// MFMA path for the shapes the big UNets use (T = 64 / 256 tokens = 8x8 / 16x16 maps, ch = 64 / 128 per head): the VALU kernel above was written for "T <= 64, FLOPs
// negligible", and the celeb512 UNet spent 5 % of an evaluation in it (T = 256, ch = 128: 4.3 GFLOP per call at batch 32 at 45 TFLOP/s).  One workgroup = 64 queries of
// one (image, head), a wave = 16 queries; ONE LDS image, every score of a query in registers; image, operand mapping and arithmetic: unet_attention_common.h.
template <int CH, int T>
__global__ __launch_bounds__(256) void attention_unet_mfma_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out, int heads, float scale) {
  using L = UattLayout<CH, T>;
  extern __shared__ __attribute__((aligned(16))) char smraw[];
  char *Ks = smraw, *Vt = smraw + L::VT;
  const int head = blockIdx.x, n = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int C = heads * CH, ldq = 3 * C;
  const half_t* base = qkv + (long)n * T * ldq + head * 3 * CH;
  // ---- stage K (16-byte chunks) and V^T (two keys x 8 channels per item)
  for (int e = tid; e < T * (CH / 8); e += 256) {
    const int t = e / (CH / 8), c8 = e - t * (CH / 8);
    *(half8_t*)(Ks + t * L::KS + c8 * 16) = *(const half8_t*)(base + (long)t * ldq + CH + c8 * 8);
  }
  for (int e = tid; e < (T / 2) * (CH / 8); e += 256) {
    const int tp = e % (T / 2), c8 = e / (T / 2);
    const half8_t v0 = *(const half8_t*)(base + (long)(2 * tp) * ldq + 2 * CH + c8 * 8);
    const half8_t v1 = *(const half8_t*)(base + (long)(2 * tp + 1) * ldq + 2 * CH + c8 * 8);
#pragma unroll
    for (int i = 0; i < 8; ++i) uatt_store_vt<L>(Vt, tp, c8 * 8 + i, v0[i], v1[i]);
  }
  const int j = lane & 15, q = lane >> 4, q0 = blockIdx.z * 64 + wave * 16;
  half8_t qf[CH / 32];
#pragma unroll
  for (int ks = 0; ks < CH / 32; ++ks) qf[ks] = uatt_q_frag(base + (long)(q0 + j) * ldq, ks, q);
  __syncthreads();
  f32x4 st[L::NTILE];
#pragma unroll
  for (int tile = 0; tile < L::NTILE; ++tile) {
    f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int ks = 0; ks < CH / 32; ++ks) a = uatt_qk_step<L>(a, Ks, tile, ks, qf[ks], j, q);
    st[tile] = a;
  }
  float mx = -3.0e38f;
#pragma unroll
  for (int tile = 0; tile < L::NTILE; ++tile) mx = fmaxf(uatt_max4(st[tile]), mx);
  mx = uatt_quad_max(mx);
  const float sl = scale * 1.4426950408889634f, mo = mx * sl;
  float sum = 0.f;
  half4_t pf[L::NTILE];
#pragma unroll
  for (int tile = 0; tile < L::NTILE; ++tile) pf[tile] = uatt_exp2_tile(sum, st[tile], sl, mo);
  sum += __shfl_xor(sum, 16, 64);
  sum += __shfl_xor(sum, 32, 64);
  const float inv = 1.0f / sum;
  half_t* ob = out + ((long)n * T + q0 + j) * C + head * CH;
#pragma unroll
  for (int ct = 0; ct < CH / 16; ++ct) {  // ONE live accumulator, stored at once
    f32x4 o = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int kt = 0; kt < L::NKT; ++kt) o = uatt_pv_step<L>(o, Vt, ct, kt, pf, j, q);
    uatt_store_o(ob, ct, q, o, inv);
  }
}

template <int CH, int T>
static int launch_attention_unet_mfma(const half_t* qkv, half_t* out, int N, int heads, hipStream_t st) {
  constexpr int LDS = UattLayout<CH, T>::BYTES;
  if (!lfm_kernel_lds<&attention_unet_mfma_kernel<CH, T>>(LDS)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL((attention_unet_mfma_kernel<CH, T>), dim3(heads, N, T / 64), dim3(256), LDS, st, qkv, out, heads, 1.0f / sqrtf((float)CH));
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
