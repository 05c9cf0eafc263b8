// What the resident and the streamed MFMA attention kernel of the UNets share (unet_attention_kernel.h, unet_attention_stream_kernel.h): the LDS image, the operand
// mapping and every piece of the arithmetic are ONE text here.  The schedule, the load predicates, the ragged-block masking and the rescale stay with each kernel -- and
// so do the loops around the steps below: a loop inside one of these functions is unrolled BEFORE the function is inlined, and the kernel's registers and issue order change.
//   S^T = K Q^T on v_mfma_f32_16x16x32_f16 with K as the A operand: lane (q = lane >> 4, j = lane & 15) ends up with the scores of ONE query j at keys
//   16 tile + 4 q + r -- the softmax row of a query lives in four lanes (two xor-shuffles per reduction) -- and O^T = V^T P^T takes P straight from those registers as
//   the B operand: the 8 k-slots of lane q in key step kt are keys 32 kt + 4 q + r and 32 kt + 16 + 4 q + r, which is what the two 8-byte V^T reads of the A operand
//   fetch.  No transposition of P, no cross-lane traffic for O; fp32 scores / softmax, P and V in fp16, 1 / sum applied to the fp32 accumulators.
#pragma once
#include "common.h"
// LDS image of KEYS keys x CHP channels: K [KEYS][CHP] fp16, then V^T [CHP][KEYS] fp16; rows padded by 16 bytes, so consecutive rows start 4 banks apart
template <int CHP_, int KEYS_>
struct UattLayout {
  static constexpr int CHP = CHP_, KEYS = KEYS_, NTILE = KEYS / 16, NKT = KEYS / 32;  // 16-key score tiles; 32-key steps of O^T
  static constexpr int KS = CHP * 2 + 16, VS = KEYS * 2 + 16;                         // row strides of K and V^T in bytes
  static constexpr int VT = KEYS * KS, BYTES = VT + CHP * VS;                         // byte offset of V^T; one {K | V^T} image
};
// ---- staging, the LDS writes.  The 16-byte chunk c8 of key t goes to Ks + t * KS + c8 * 16: an assignment in each kernel (behind a function the compiler folds the
// address with t = e / C8, c8 = e % C8 otherwise and orders the resident kernel's prologue otherwise).  V^T: keys 2 tp, 2 tp + 1 of channel c are one dword; an item
// is a channel octet, eight of these, and consecutive lanes take consecutive key pairs (conflict-free)
template <class L>
__device__ __forceinline__ void uatt_store_vt(char* Vt, int tp, int c, half_t v0, half_t v1) { *(half2_t*)(Vt + c * L::VS + tp * 4) = (half2_t){v0, v1}; }
// ---- k-step ks of the B operand of S^T: lane (q, j) holds Q[q0 + j][32 ks + 8 q .. + 7]; qrow = row q0 + j ...
__device__ __forceinline__ half8_t uatt_q_frag(const half_t* qrow, int ks, int q) { return *(const half8_t*)(qrow + ks * 32 + q * 8); }
// ... and with the streamed kernel's predicates: dead queries and channels >= ch are zeros and not read
__device__ __forceinline__ half8_t uatt_q_frag(const half_t* qrow, int ks, int q, bool q_live, int ch) {
  const half8_t zero8 = {0, 0, 0, 0, 0, 0, 0, 0};
  return q_live && ks * 32 + q * 8 < ch ? uatt_q_frag(qrow, ks, q) : zero8;
}
// ---- S^T: a += K[16 tile ..][32 ks ..] Q^T; over all ks, a[r] = score of query j at key 16 tile + 4 q + r of the image
template <class L>
__device__ __forceinline__ f32x4 uatt_qk_step(f32x4 a, const char* Ks, int tile, int ks, half8_t qf, int j, int q) {
  const half8_t kf = *(const half8_t*)(Ks + (tile * 16 + j) * L::KS + (ks * 4 + q) * 16);
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(kf, qf, a, 0, 0, 0);
}
// ---- row maximum of query j: the four keys of a score tile; then, over the lane's tiles (the kernel's loop), the four lanes of the query
__device__ __forceinline__ float uatt_max4(f32x4 s) { return fmaxf(fmaxf(s.x, s.y), fmaxf(s.z, s.w)); }
__device__ __forceinline__ float uatt_quad_max(float mx) {
  mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
  return fmaxf(mx, __shfl_xor(mx, 32, 64));
}
// ---- one score tile: p = 2^(s sl - mo) as the fp16 B operand of O^T; the lane's part of the row sum grows tile by tile (in / out: the streamed kernel's running sum)
__device__ __forceinline__ half4_t uatt_exp2_tile(float& sum, f32x4 st, float sl, float mo) {
  const float e0 = __builtin_amdgcn_exp2f(st.x * sl - mo), e1 = __builtin_amdgcn_exp2f(st.y * sl - mo);
  const float e2 = __builtin_amdgcn_exp2f(st.z * sl - mo), e3 = __builtin_amdgcn_exp2f(st.w * sl - mo);
  sum += (e0 + e1) + (e2 + e3);
  return (half4_t){(half_t)e0, (half_t)e1, (half_t)e2, (half_t)e3};
}
// ---- O^T: o += V^T[16 ct ..][32 kt ..] P^T; a channel tile is this step for kt = 0 .. L::NKT - 1, key step kt = 32 keys = score tiles 2 kt, 2 kt + 1
template <class L>
__device__ __forceinline__ f32x4 uatt_pv_step(f32x4 o, const char* Vt, int ct, int kt, const half4_t (&pf)[L::NTILE], int j, int q) {
  const char* vr = Vt + (ct * 16 + j) * L::VS + (kt * 32 + q * 4) * 2;
  const half4_t va = *(const half4_t*)vr, vb = *(const half4_t*)(vr + 32);
  const half8_t vf = {va[0], va[1], va[2], va[3], vb[0], vb[1], vb[2], vb[3]};
  const half4_t pa = pf[2 * kt], pb = pf[2 * kt + 1];
  const half8_t pp = {pa[0], pa[1], pa[2], pa[3], pb[0], pb[1], pb[2], pb[3]};
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(vf, pp, o, 0, 0, 0);
}
// ---- the lane holds O[query j][channels 16 ct + 4 q .. + 3]; orow = the query's output row
__device__ __forceinline__ void uatt_store_o(half_t* orow, int ct, int q, f32x4 o, float inv) {
  *(half4_t*)(orow + ct * 16 + q * 4) = (half4_t){(half_t)(o.x * inv), (half_t)(o.y * inv), (half_t)(o.z * inv), (half_t)(o.w * inv)};
}
