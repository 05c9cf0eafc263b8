// What the three DiT attention kernels share (attention_kernel.h: one workgroup per item; attention_stream_kernel.h: persistent, streamed; qkv_attention_kernel.h:
// fused with the QKV projection): the online-softmax block -- one text, so the three are bit-identical --, the counted-wait / barrier macros and the trace arrays
// of the measurement variants.
#pragma once
#include "gemm_kernel.h"

#define ATS_VMCNT(n) asm volatile("s_waitcnt vmcnt(" #n ")" ::: "memory")
#define ATS_BARRIER()                              \
  do {                                             \
    __builtin_amdgcn_s_barrier();                  \
    asm volatile("" ::: "memory");                 \
  } while (0)

// One 32-key block of the online softmax for the query a lane owns (S: its 16 scores of the block, the other 16 live in lane ^ 32), shared by the streamed and the
// per-item kernels (same arithmetic in the same order => bit-identical results whichever kernel evaluates an item).  Round 6: the key loop is bound by instruction
// ISSUE, not by a pipe -- per SIMD, whether it holds two or four waves, one 32-key block of one wave goes through in ~850 cycles while its 8 MFMAs occupy the matrix
// pipe for 256 and ~5 single-issue instructions hide under each of them (profiles/r06_attention_stream.txt) -- so the block is written for instruction count:
//   * OPTIMISTIC exponentials: p = 2^((s - mrun) scale) is taken against the running reference mrun WITHOUT first looking for the block's maximum; the lane's own sum of
//     its 16 p (needed anyway) tells whether that was safe -- every p <= sum <= 2^14 stays far inside fp16 (P is the fp16 operand of the P V MFMA; row sums and O are
//     fp32).  Only when some lane's sum exceeds 2^14 (or is not a number), and for the first block of an item, the block takes the FULL path: row maximum (3-input
//     maxima + one lane ^ 32 exchange), mrun <- max, O and l rescaled by 2^((old - new) scale), exponentials again.  The reference follows the maximum lazily, as
//     before (rounds 3-5 moved it when the maximum had grown by more than 2^8); fp16 rounds P relative to its size, so the result does not depend on where in
//     [2^-14 .. 2^14] the block's largest p lands.
//   * row sum as a TREE of packed adds (8 issue slots; the serial chain of rounds 1-5 drew a wait state per link: 18).
// `first` is wave-uniform.  Returns the packed P of the block (k-slots 0 and 1) in P.
template <int NDB>
__device__ __forceinline__ void att_softmax_block(const f32x16& S, bool first, float& mrun, float& lrun, f32x16 (&Oa)[NDB], float scale_log2e, half8_t (&P)[2]) {
  f32x2 p[8];
  const f32x2 sc2 = {scale_log2e, scale_log2e};
  auto expo = [&]() {
    const float mbs = mrun * scale_log2e;
    const f32x2 nmb2 = {-mbs, -mbs};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const f32x2 s2 = {S[2 * e], S[2 * e + 1]};
      const f32x2 a2 = __builtin_elementwise_fma(s2, sc2, nmb2);  // ONE fused multiply-add on every path and in every kernel that inlines this (v_pk_fma_f32 / v_fma_f32)
      p[e] = (f32x2){__builtin_amdgcn_exp2f(a2.x), __builtin_amdgcn_exp2f(a2.y)};
    }
  };
  auto lane_sum = [&]() {
    const f32x2 t = ((p[0] + p[1]) + (p[2] + p[3])) + ((p[4] + p[5]) + (p[6] + p[7]));  // v_pk_add_f32 x 7
    return t.x + t.y;
  };
  float ls = 0.f;
  bool full = first;
  if (!first) {
    expo();
    ls = lane_sum();
    full = !__all(ls <= 16384.0f);
  }
  if (full) {  // wave-uniform
    float mx = fmaxf(fmaxf(S[0], S[1]), S[2]);
#pragma unroll
    for (int e = 3; e < 15; e += 2) mx = fmaxf(fmaxf(mx, S[e]), S[e + 1]);
    mx = fmaxf(mx, S[15]);
    mx = fmaxf(mx, xhalf(mx));
    const float mnew = fmaxf(mrun, mx);
    const float alpha = __builtin_amdgcn_exp2f((mrun - mnew) * scale_log2e);
    mrun = mnew;
    lrun *= alpha;
#pragma unroll
    for (int db = 0; db < NDB; ++db) Oa[db] *= alpha;
    expo();
    ls = lane_sum();
  }
  lrun += ls;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    P[e >> 2][(e & 3) * 2] = (half_t)p[e].x;
    P[e >> 2][(e & 3) * 2 + 1] = (half_t)p[e].y;
  }
}

// s_memtime stamps of the measurement variants (MODE 3 of the per-item and the streamed kernel, flag QKV_TRACE of the fused one; the slot maps are next to each
// kernel), read back with lfm_attention_trace_read / lfm_attention_wg_trace_read
#define ATT_TRACE_SLOTS 64
#define ATT_WG_TRACE 2048
static __device__ unsigned long long att_trace[ATT_TRACE_SLOTS];
static __device__ unsigned long long att_wg_trace[ATT_WG_TRACE][4];
