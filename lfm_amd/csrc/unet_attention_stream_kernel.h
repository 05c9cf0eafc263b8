// Streamed attention of the UNets (QKVAttentionLegacy, unet.py:310-334; models/EDM.py UNetBlock) for ANY token count.  qkv layout: unet_attention_kernel.h; LDS image,
// operand mapping and arithmetic: unet_attention_common.h, one text with the resident kernel, whose token count is a template argument and ends at 256.  Here a
// workgroup (NW waves x 16 queries of one (image, head)) walks the keys in blocks of 64 and only a block is resident:
//   * two LDS stages (UattStage<CHP>): 36 KiB at CHP = 64 (four workgroups per CU), 138 KiB at CHP = 256 (one).  The global loads of block i + 1 are issued into
//     registers BEFORE the MFMAs of block i and written to the other stage after them; one barrier per block (the stage written in iteration i was last read in
//     iteration i - 1, which ended with a barrier).  V^T is built while staging, not with the LDS transpose reads of gfx950.
//   * online softmax per query in fp32: when the maximum of ANY query of the wave rises, l and the O accumulators are scaled by 2^((m_old - m_new) scale) (wave-uniform
//     branch).  The four lanes of a query agree on m, so each keeps a PARTIAL sum and the two xor-shuffles of the sum happen once, after the last block.
//   * any T >= 1: keys >= T of the ragged last block are never loaded (zeros in the LDS image) and their scores are set to -inf before the maximum; queries >= T are
//     neither loaded nor stored.  ch % 16 == 0, 16 <= ch <= 256: CHP = ch rounded up to a multiple of 32 (the k extent of the MFMA), channels [ch, CHP) are zeros in
//     the LDS image and in the Q fragments and their output tile is not stored -- nf = 192 models (heads of 48 and of 3 x 48 channels) are served.
//   * every global offset is 64-bit; no workspace, no allocation, no synchronisation: graph-capturable.  Variants tried: profiles/unet_attention_stream.txt.
#pragma once
#include "unet_attention_common.h"
template <int CHP>
using UattStage = UattLayout<CHP, 64>;  // one LDS stage: a block of 64 keys (kernel and launcher)

template <int CHP, int NW>
__global__ __launch_bounds__(NW * 64) void attention_unet_stream_kernel(const half_t* __restrict__ qkv, half_t* __restrict__ out, int T, int heads, int ch,
                                                                        int qblocks, float scale) {
  using L = UattStage<CHP>;
  constexpr int KB = L::KEYS, NT = NW * 64, C8 = CHP / 8;
  constexpr int KITEMS = KB * C8, VITEMS = (KB / 2) * C8;  // 16-byte chunks of a K block; (key pair, channel octet) items of a V block
  constexpr int KIT = (KITEMS + NT - 1) / NT, VIT = (VITEMS + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) char smraw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // blockIdx.x = (image * heads + head) * qblocks + query block: the workgroups that read the same K / V are neighbours
  const int qb = blockIdx.x % qblocks, item = blockIdx.x / qblocks;
  const int n = item / heads, head = item - n * heads;
  const int C = heads * ch;
  const long ldq = 3L * C;
  const half_t* base = qkv + (long)n * T * ldq + (long)head * 3 * ch;
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // ---- a key block: global -> registers (issued a block ahead) -> LDS stage.  Keys >= T and channels >= ch are zeros and never read.
  half8_t kr[KIT], va[VIT], vb[VIT];
  auto load_block = [&](int k0) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int e = tid + it * NT, t = e / C8, c8 = e - t * C8;
      const bool live = (KITEMS % NT == 0 || e < KITEMS) && k0 + t < T && c8 * 8 < ch;
      kr[it] = live ? *(const half8_t*)(base + (long)(k0 + t) * ldq + ch + c8 * 8) : zero8;
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int e = tid + it * NT, tp = e % (KB / 2), c8 = e / (KB / 2);
      const bool live = (VITEMS % NT == 0 || e < VITEMS) && c8 * 8 < ch;
      const int t0 = k0 + 2 * tp;
      va[it] = live && t0 < T ? *(const half8_t*)(base + (long)t0 * ldq + 2 * ch + c8 * 8) : zero8;
      vb[it] = live && t0 + 1 < T ? *(const half8_t*)(base + (long)(t0 + 1) * ldq + 2 * ch + c8 * 8) : zero8;
    }
  };
  auto store_block = [&](char* Ks) {
    char* Vt = Ks + L::VT;
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int e = tid + it * NT, t = e / C8, c8 = e - t * C8;
      if (KITEMS % NT == 0 || e < KITEMS) *(half8_t*)(Ks + t * L::KS + c8 * 16) = kr[it];
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int e = tid + it * NT, tp = e % (KB / 2), c8 = e / (KB / 2);
      if (VITEMS % NT == 0 || e < VITEMS) {
#pragma unroll
        for (int i = 0; i < 8; ++i) uatt_store_vt<L>(Vt, tp, c8 * 8 + i, va[it][i], vb[it][i]);
      }
    }
  };
  load_block(0);
  const int j = lane & 15, q = lane >> 4;
  const int q0 = qb * (NW * 16) + wave * 16;
  const bool q_live = q0 + j < T;
  half8_t qf[CHP / 32];
#pragma unroll
  for (int ks = 0; ks < CHP / 32; ++ks) qf[ks] = uatt_q_frag(base + (long)(q0 + j) * ldq, ks, q, q_live, ch);
  store_block(smraw);
  __syncthreads();
  const float sl = scale * 1.4426950408889634f;
  float mrun = -3.0e38f, lsum = 0.f;  // running maximum of query j (the same in its four lanes), this lane's part of the running sum
  f32x4 o[CHP / 16];
#pragma unroll
  for (int ct = 0; ct < CHP / 16; ++ct) o[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nblk = (T + KB - 1) / KB;
#pragma unroll 1
  for (int b = 0; b < nblk; ++b) {
    const char *Ks = smraw + (b & 1) * L::BYTES, *Vt = Ks + L::VT;
    const int k0 = b * KB;
    const bool more = b + 1 < nblk;
    if (more) load_block(k0 + KB);
    f32x4 st[L::NTILE];  // st[tile][r] = score of query j at key k0 + 16 tile + 4 q + r
#pragma unroll
    for (int tile = 0; tile < L::NTILE; ++tile) {
      f32x4 a = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int ks = 0; ks < CHP / 32; ++ks) a = uatt_qk_step<L>(a, Ks, tile, ks, qf[ks], j, q);
      st[tile] = a;
    }
    if (k0 + KB > T) {  // the ragged last block: its zero padding must not take part in the maximum or the sum
#pragma unroll
      for (int tile = 0; tile < L::NTILE; ++tile)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (k0 + tile * 16 + q * 4 + r >= T) st[tile][r] = -__builtin_inff();
    }
    float mx = uatt_max4(st[0]);
#pragma unroll
    for (int tile = 1; tile < L::NTILE; ++tile) mx = fmaxf(uatt_max4(st[tile]), mx);
    const float mnew = fmaxf(mrun, uatt_quad_max(mx));
    if (!__all(mnew == mrun)) {  // wave-uniform: some query's maximum rose (always in the first block)
      const float alpha = __builtin_amdgcn_exp2f((mrun - mnew) * sl);
      lsum *= alpha;
#pragma unroll
      for (int ct = 0; ct < CHP / 16; ++ct) {
        o[ct].x *= alpha;
        o[ct].y *= alpha;
        o[ct].z *= alpha;
        o[ct].w *= alpha;
      }
      mrun = mnew;
    }
    half4_t pf[L::NTILE];
    const float mo = mrun * sl;
#pragma unroll
    for (int tile = 0; tile < L::NTILE; ++tile) pf[tile] = uatt_exp2_tile(lsum, st[tile], sl, mo);
    // all CHP / 16 channel tiles, branch-free: the tile of channels [ch, CHP) multiplies zeros and is never stored
#pragma unroll
    for (int ct = 0; ct < CHP / 16; ++ct)
#pragma unroll
      for (int kt = 0; kt < L::NKT; ++kt) o[ct] = uatt_pv_step<L>(o[ct], Vt, ct, kt, pf, j, q);
    if (more) store_block(smraw + ((b + 1) & 1) * L::BYTES);
    __syncthreads();
  }
  lsum += __shfl_xor(lsum, 16, 64);
  lsum += __shfl_xor(lsum, 32, 64);
  const float inv = 1.0f / lsum;
  if (q_live) {
    half_t* ob = out + ((long)n * T + q0 + j) * C + (long)head * ch;
#pragma unroll
    for (int ct = 0; ct < CHP / 16; ++ct)
      if (ct * 16 < ch) uatt_store_o(ob, ct, q, o[ct], inv);
  }
}

// NW waves = NW x 16 queries per workgroup.  Grid: one workgroup per (image, head, query block), all in x (N is not bound by the 65535 of y / z).
template <int CHP, int NW>
static int launch_attention_unet_stream(const half_t* qkv, half_t* out, int N, int T, int heads, int ch, hipStream_t st) {
  constexpr int LDS = 2 * UattStage<CHP>::BYTES;
  static_assert(LDS <= 160 * 1024, "two stages must fit the LDS");
  const int qblocks = (T + NW * 16 - 1) / (NW * 16);
  const long grid = (long)N * heads * qblocks;
  if (grid >= (1L << 31)) return LFM_ERR_SHAPE;
  if (!lfm_kernel_lds<&attention_unet_stream_kernel<CHP, NW>>(LDS)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL((attention_unet_stream_kernel<CHP, NW>), dim3((unsigned)grid), dim3(NW * 64), LDS, st, qkv, out, T, heads, ch, qblocks,
                     1.0f / sqrtf((float)ch));
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

#ifndef LFM_UNET_ATT_STREAM_WAVES
#define LFM_UNET_ATT_STREAM_WAVES 4  // 64 queries per workgroup, as the resident kernel (8 = 128 queries, the A/B: profiles/unet_attention_stream.txt)
#endif
static int attention_unet_stream_launch(const half_t* qkv, half_t* out, int N, int T, int heads, int ch, hipStream_t st) {
  constexpr int NW = LFM_UNET_ATT_STREAM_WAVES;
  switch ((ch + 31) / 32) {
    case 1: return launch_attention_unet_stream<32, NW>(qkv, out, N, T, heads, ch, st);
    case 2: return launch_attention_unet_stream<64, NW>(qkv, out, N, T, heads, ch, st);
    case 3: return launch_attention_unet_stream<96, NW>(qkv, out, N, T, heads, ch, st);
    case 4: return launch_attention_unet_stream<128, NW>(qkv, out, N, T, heads, ch, st);
    case 5: return launch_attention_unet_stream<160, NW>(qkv, out, N, T, heads, ch, st);
    case 6: return launch_attention_unet_stream<192, NW>(qkv, out, N, T, heads, ch, st);
    case 7: return launch_attention_unet_stream<224, NW>(qkv, out, N, T, heads, ch, st);
    case 8: return launch_attention_unet_stream<256, NW>(qkv, out, N, T, heads, ch, st);
  }
  return LFM_ERR_SHAPE;
}
