// Cross-attention of the SpatialTransformer (attention.py:177-215, CrossAttention with a context): queries from one row-major buffer, keys and values from
// another with a token count of its own.  out[n Tq + i][head ch + c] = softmax_j(q_i . k_j / sqrt(ch)) v_j over the Tk keys of image n.
//   Q  fp16 rows [N * Tq], ldq apart;  K, V fp16 rows [N * Tk], ldkv apart (two column slices of one projection buffer, hence one ld);  out rows ldo apart;
//   columns [head][ch] in all four.
// The schedule is the streamed self-attention kernel's (unet_attention_stream_kernel.h) and the steps are the text of unet_attention_common.h, inlined here as
// there: a workgroup (NW waves x 16 queries of one (image, head)) walks the keys in blocks of 64 through two LDS stages (UattLayout<CHP, 64>: 36 KiB at CHP = 64,
// 138 KiB at CHP = 256), the global loads of block i + 1 issued into registers before the MFMAs of block i and written to the other stage after them, one barrier
// per block; online softmax per query in fp32, l and O scaled when any query's maximum rises (wave-uniform branch), the four lanes of a query keep partial sums.
// A short context (Tk <= 64) is the same loop with one trip: no second stage is written, no second kernel text.  What differs from the self-attention kernel:
//   * K and V^T are staged from K / V at row n * Tk, the queries come from Q at row n * Tq;
//   * the key loop, the load predicates and the -inf mask of the ragged last block are bounded by Tk; the query blocks, q_live and the stores by Tq.
// With Tq == Tk and K, V slices of a packed qkv this is the same arithmetic in the same order: bit-identical to that kernel (tests/test_gpu_layout_kernels.py).
// Any Tq >= 1, Tk >= 1; ch % 16 == 0, ch <= 256 (CHP = ch rounded up to 32: channels [ch, CHP) are zeros in the LDS image and in the Q fragments and their output
// tile is not stored).  Keys >= Tk are never loaded, queries >= Tq neither loaded nor stored.  Every global offset is 64-bit; no workspace, no allocation, no
// synchronisation: graph-capturable.
#pragma once
#include "unet_attention_common.h"

template <int CHP, int NW>
__global__ __launch_bounds__(NW * 64) void cross_attention_unet_kernel(const half_t* __restrict__ Q, long ldq, const half_t* __restrict__ K,
                                                                       const half_t* __restrict__ V, long ldkv, half_t* __restrict__ out, long ldo, int Tq,
                                                                       int Tk, int heads, int ch, int qblocks, float scale) {
  using L = UattLayout<CHP, 64>;
  constexpr int KB = L::KEYS, NT = NW * 64, C8 = CHP / 8;
  constexpr int KITEMS = KB * C8, VITEMS = (KB / 2) * C8;  // 16-byte chunks of a K block; (key pair, channel octet) items of a V block
  constexpr int KIT = (KITEMS + NT - 1) / NT, VIT = (VITEMS + NT - 1) / NT;
  extern __shared__ __attribute__((aligned(16))) char smraw[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  // blockIdx.x = (image * heads + head) * qblocks + query block: the workgroups that read the same K / V are neighbours
  const int qb = blockIdx.x % qblocks, item = blockIdx.x / qblocks;
  const int n = item / heads, head = item - n * heads;
  const half_t* kbase = K + (long)n * Tk * ldkv + (long)head * ch;
  const half_t* vbase = V + (long)n * Tk * ldkv + (long)head * ch;
  const half_t* qbase = Q + (long)n * Tq * ldq + (long)head * ch;
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  // ---- a key block: global -> registers (issued a block ahead) -> LDS stage.  Keys >= Tk and channels >= ch are zeros and never read.
  half8_t kr[KIT], va[VIT], vb[VIT];
  auto load_block = [&](int k0) {
#pragma unroll
    for (int it = 0; it < KIT; ++it) {
      const int e = tid + it * NT, t = e / C8, c8 = e - t * C8;
      const bool live = (KITEMS % NT == 0 || e < KITEMS) && k0 + t < Tk && c8 * 8 < ch;
      kr[it] = live ? *(const half8_t*)(kbase + (long)(k0 + t) * ldkv + c8 * 8) : zero8;
    }
#pragma unroll
    for (int it = 0; it < VIT; ++it) {
      const int e = tid + it * NT, tp = e % (KB / 2), c8 = e / (KB / 2);
      const bool live = (VITEMS % NT == 0 || e < VITEMS) && c8 * 8 < ch;
      const int t0 = k0 + 2 * tp;
      va[it] = live && t0 < Tk ? *(const half8_t*)(vbase + (long)t0 * ldkv + c8 * 8) : zero8;
      vb[it] = live && t0 + 1 < Tk ? *(const half8_t*)(vbase + (long)(t0 + 1) * ldkv + c8 * 8) : zero8;
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
  const bool q_live = q0 + j < Tq;
  half8_t qf[CHP / 32];
#pragma unroll
  for (int ks = 0; ks < CHP / 32; ++ks) qf[ks] = uatt_q_frag(qbase + (long)(q0 + j) * ldq, ks, q, q_live, ch);
  store_block(smraw);
  __syncthreads();
  const float sl = scale * 1.4426950408889634f;
  float mrun = -3.0e38f, lsum = 0.f;  // running maximum of query j (the same in its four lanes), this lane's part of the running sum
  f32x4 o[CHP / 16];
#pragma unroll
  for (int ct = 0; ct < CHP / 16; ++ct) o[ct] = (f32x4){0.f, 0.f, 0.f, 0.f};
  const int nblk = (Tk + KB - 1) / KB;
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
    if (k0 + KB > Tk) {  // the ragged last block: its zero padding must not take part in the maximum or the sum
#pragma unroll
      for (int tile = 0; tile < L::NTILE; ++tile)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          if (k0 + tile * 16 + q * 4 + r >= Tk) st[tile][r] = -__builtin_inff();
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
    half_t* ob = out + ((long)n * Tq + q0 + j) * ldo + (long)head * ch;
#pragma unroll
    for (int ct = 0; ct < CHP / 16; ++ct)
      if (ct * 16 < ch) uatt_store_o(ob, ct, q, o[ct], inv);
  }
}

static constexpr int CROSS_ATT_WAVES = 4;  // 64 queries per workgroup, as the self-attention kernels

// the shapes served, without a launch: any Tq, Tk >= 1; ch % 16 == 0, ch <= 256; the grid within 2^31 workgroups
static inline int cross_attention_served(int N, int Tq, int Tk, int heads, int ch) {
  if (N <= 0 || Tq <= 0 || Tk <= 0 || heads <= 0 || ch <= 0 || ch % 16 || ch > 256) return LFM_ERR_SHAPE;
  const long qblocks = ((long)Tq + CROSS_ATT_WAVES * 16 - 1) / (CROSS_ATT_WAVES * 16);
  if ((long)N * heads >= (1L << 31) / qblocks) return LFM_ERR_SHAPE;
  return 1;
}
extern "C" int lfm_cross_attention_plan(int N, int Tq, int Tk, int heads, int ch) { return cross_attention_served(N, Tq, Tk, heads, ch); }

// One workgroup per (image, head, query block), all in x (N is not bound by the 65535 of y / z).
template <int CHP>
static int launch_cross_attention_unet(const half_t* Q, long ldq, const half_t* K, const half_t* V, long ldkv, half_t* out, long ldo, int N, int Tq, int Tk,
                                       int heads, int ch, hipStream_t st) {
  constexpr int NW = CROSS_ATT_WAVES, LDS = 2 * UattLayout<CHP, 64>::BYTES;
  static_assert(LDS <= 160 * 1024, "two stages must fit the LDS");
  const int qblocks = (Tq + NW * 16 - 1) / (NW * 16);
  const long grid = (long)N * heads * qblocks;
  if (!lfm_kernel_lds<&cross_attention_unet_kernel<CHP, NW>>(LDS)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL((cross_attention_unet_kernel<CHP, NW>), dim3((unsigned)grid), dim3(NW * 64), LDS, st, Q, ldq, K, V, ldkv, out, ldo, Tq, Tk, heads, ch,
                     qblocks, 1.0f / sqrtf((float)ch));
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_cross_attention_f16(const void* Q, long ldq, const void* K, const void* V, long ldkv, void* out, long ldo, int N, int Tq, int Tk,
                                       int heads, int ch, lfm_stream_t stream) {
  if (!Q || !K || !V || !out) return LFM_ERR_ARG;
  if (cross_attention_served(N, Tq, Tk, heads, ch) < 0) return LFM_ERR_SHAPE;
  const long C = (long)heads * ch;
  if (ldq < C || ldkv < C || ldo < C) return LFM_ERR_SHAPE;
  if ((ldq % 8) || (ldkv % 8) || (ldo % 8) || (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)V | (uintptr_t)out) & 15)) return LFM_ERR_ALIGN;
  const half_t *q = (const half_t*)Q, *k = (const half_t*)K, *v = (const half_t*)V;
  half_t* o = (half_t*)out;
  hipStream_t st = (hipStream_t)stream;
  switch ((ch + 31) / 32) {
    case 1: return launch_cross_attention_unet<32>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 2: return launch_cross_attention_unet<64>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 3: return launch_cross_attention_unet<96>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 4: return launch_cross_attention_unet<128>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 5: return launch_cross_attention_unet<160>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 6: return launch_cross_attention_unet<192>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 7: return launch_cross_attention_unet<224>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
    case 8: return launch_cross_attention_unet<256>(q, ldq, k, v, ldkv, o, ldo, N, Tq, Tk, heads, ch, st);
  }
  return LFM_ERR_SHAPE;
}
