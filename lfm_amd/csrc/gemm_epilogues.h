// The epilogues of the MFMA GEMM kernels and the `Epi` interface they are written against (included by gemm_kernel.h).
//
// An epilogue is a small struct passed to a GEMM kernel by value.  It MUST provide
//   typedef / struct Aux;  Aux load(m, n) const;  void store(m, n, f32x4 v, const Aux&) const
// two-phase, so that an interior tile can issue ALL its loads before the first store (the compiler will not move a load above a possibly-aliasing
// store): v = C[m][n .. n + 3] (fp32 accumulators); m < M and n + 3 < N are guaranteed by the caller.  It MAY provide (detected by the traits at the
// end of this file; "256-row" = the hand-over of epilogue_handover.h, used by the 256x128, both 256x256 kernels and the halo convolution):
//   batch(bz, stride)                  batched problems: advance the bases by the batch index                       every GEMM kernel
//   wide_ok(), store8(m, n, lo, hi, aux_lo, aux_hi)
//                                      fp16 outputs: EIGHT consecutive columns = one 16-byte store                 256-row, halo convolution
//   static constexpr column_aux        load(m, n) depends on n only (a bias row): loaded once per tile              256-row
//   row_aux(m) -> f32x2, store8r(.., row_aux)
//                                      per-row operands in LDS, fetched with the scratch read-back                  256-row
//   finish_tile(m0, n0, g, wn, lane)   per-lane sums across the store8 calls of a tile (GroupNorm partials)        256x128, 256x256 eight-wave
//   finish_slab(img, slab, ncol0, lane) the same for the halo convolution's pixel tiles                             halo convolution
//   direct(n0)                         column ranges that want the raw MFMA fragment layout                         256-row, skinny / sq64
//   plain_tile(n0, bn), plain(n0)      tiles that reduce to a simpler epilogue (EpiQKV: Q or K tiles)                256-row
//   transposed(n0), load_t(n), store_t(n, m, v, aux_t), wide_t_ok(), store_t8(n, m, lo, hi, aux_t)
//                                      tiles the K loop computes with the MFMA operands swapped: C^T rows            256-row
//   static constexpr rowstat, RowStatSrc st, rs, m0
//                                      consumer of the folded LayerNorm: row statistics reduced before the K loop   256x256 (both)
//   static constexpr producer_mod      producer of the folded LayerNorm: the kernel runs its own epilogue           256x256 (both)
#pragma once
#include "common.h"

// ------------------------------------------------------------------ fp16 packing, activations
// (written  *(half4_t*)(dst) = f16x4(v);  the conversion is then sequenced before the address arithmetic, as in every epilogue so far)
__device__ __forceinline__ half4_t f16x4(f32x4 v) { return (half4_t){(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w}; }
__device__ __forceinline__ half8_t f16x8(f32x4 lo, f32x4 hi) {
  return (half8_t){(half_t)lo.x, (half_t)lo.y, (half_t)lo.z, (half_t)lo.w, (half_t)hi.x, (half_t)hi.y, (half_t)hi.z, (half_t)hi.w};
}
struct ActIdentity {
  static __device__ __forceinline__ f32x4 apply(f32x4 v) { return v; }
};
struct ActGeluTanh {  // two elements at a time on the packed-fp32 VALU (common.h)
  static __device__ __forceinline__ f32x4 apply(f32x4 v) {
    const f32x2_t a = gelu_tanh_pk((f32x2_t){v.x, v.y}), c = gelu_tanh_pk((f32x2_t){v.z, v.w});
    return (f32x4){a.x, a.y, c.x, c.y};
  }
};
struct ActSilu {  // x * sigmoid(x) in fp32 on the accumulator (silu_f, common.h: v_exp_f32 + v_rcp_f32), element by element: EDM FeedForward (models/EDM.py:438)
  static __device__ __forceinline__ f32x4 apply(f32x4 v) { return (f32x4){silu_f(v.x), silu_f(v.y), silu_f(v.z), silu_f(v.w)}; }
};
struct ActGeluErf {  // the exact GELU of nn.GELU() in fp32 on the accumulator (gelu_erf_f, common.h: 0.5 g erfc(-g / sqrt 2)), element by element: x_transformer FeedForward (models/encoder.py)
  static __device__ __forceinline__ f32x4 apply(f32x4 v) { return (f32x4){gelu_erf_f(v.x), gelu_erf_f(v.y), gelu_erf_f(v.z), gelu_erf_f(v.w)}; }
};

// ------------------------------------------------------------------ bias epilogues
template <class Act>
struct EpiBiasActF16 {  // C = act(acc + bias) -> fp16
  half_t* C;
  long ldc;
  const float* bias;
  typedef f32x4 Aux;
  static constexpr bool column_aux = true;
  __device__ __forceinline__ Aux load(int, int n) const { return *(const f32x4*)(bias + n); }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const {
    const f32x4 o = Act::apply(v + b);
    *(half4_t*)(C + (long)m * ldc + n) = f16x4(o);
  }
  __device__ __forceinline__ bool wide_ok() const { return (ldc & 7) == 0 && ((uintptr_t)C & 15) == 0; }  // 16-byte stores are aligned
  __device__ __forceinline__ void store8(int m, int n, f32x4 lo, f32x4 hi, const Aux& bl, const Aux& bh) const {
    const f32x4 ol = Act::apply(lo + bl), oh = Act::apply(hi + bh);
    *(half8_t*)(C + (long)m * ldc + n) = f16x8(ol, oh);
  }
};
struct EpiBiasF16 : EpiBiasActF16<ActIdentity> {  // C = acc + bias -> fp16; bias may be null
  __device__ __forceinline__ Aux load(int, int n) const { return bias ? *(const f32x4*)(bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f}; }
};
struct EpiBiasGeluF16 : EpiBiasActF16<ActGeluTanh> {};  // C = gelu_tanh(acc + bias) -> fp16   (timm Mlp fc1, DiT.py:123-124)
struct EpiBiasSiluF16 : EpiBiasActF16<ActSilu> {};      // C = silu(acc + bias) -> fp16   (EDM FeedForward.layer0, models/EDM.py:438)
struct EpiBiasGeluErfF16 : EpiBiasActF16<ActGeluErf> {};  // C = gelu_erf(acc + bias) -> fp16   (x_transformer FeedForward net.0, models/encoder.py)

struct EpiBiasF32 {  // C = acc + bias -> fp32   (adaLN modulation table)
  float* C;
  long ldc;
  const float* bias;
  typedef f32x4 Aux;
  static constexpr bool column_aux = true;
  __device__ __forceinline__ Aux load(int, int n) const { return bias ? *(const f32x4*)(bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const { *(f32x4*)(C + (long)m * ldc + n) = v + b; }
};

// X[m][n] += gate[img(m)][n] * (acc + bias[n]);  fp32 residual stream (DiT.py:129-130)
struct EpiGateResid {
  float* X;
  long ldx;
  const float* bias;
  const float* gate;  // gate + img*gate_stride + n
  long gate_stride;   // floats between images' modulation rows (0 => one shared row)
  int tokens;         // rows per image
  struct Aux {
    f32x4 b, g, x;
  };
  __device__ __forceinline__ Aux load(int m, int n) const {
    Aux a;
    a.b = *(const f32x4*)(bias + n);
    a.g = *(const f32x4*)(gate + (long)(m / tokens) * gate_stride + n);
    a.x = *(const f32x4*)(X + (long)m * ldx + n);
    return a;
  }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& a) const {
    *(f32x4*)(X + (long)m * ldx + n) = a.x + a.g * (v + a.b);
  }
};
struct EpiGateResidF32 : EpiGateResid {};

// ------------------------------------------------------------------ adaLN LayerNorm-modulate FOLDED into the GEMM epilogues (round 3)
// modulate(LayerNorm(x), shift, scale) (DiT.py:20-21, 129-130) feeds a Linear, so with mu, rstd the row statistics of x and c any per-row constant
//   (LN(x) (1 + s) + sh) W^T  =  rstd * [ ((x - c)(1 + s)) W^T  -  (mu - c) * u ]  +  v,     u[n] = sum_k (1 + s[k]) W[n][k],  v[n] = sum_k sh[k] W[n][k] + bias[n].
// PRODUCER = the gated-residual GEMM that updates x (proj, fc2; EpiGateResidMod): its epilogue already holds the new x in registers, so it also
//   writes A' = fp16((x - c)(1 + s)) -- the consumer's A operand -- and per-row partials (sum x, sum (x - c)^2) of its 256 columns into a fixed slot
//   part[m][tile_n] (plain stores, deterministic).  c = cen[m] = the row mean BEFORE this update (written by the previous consumer), so x - c is
//   centred up to the mean shift of one residual update: no cancellation in the fp16 rounding of A' or in the one-pass variance -- while that shift
//   r = |mu - c| / std stays below ~1.  The operand error grows like r 2^-11 (measured: the fc1 activation leaves the per-forward budget at r = 6 .. 8;
//   DESIGN.md, "Folded LayerNorm-modulate"; tests/test_gpu_dit_ln.py holds every piece to a bound that grows with the row's own r).
// CONSUMER = the GEMM that reads A' (qkv, fc1; rowstat epilogues below): before its K loop every tile reduces its 256 rows' partials to
//   a = rstd, b = -rstd (mu - c) in LDS (and tile column 0 publishes mu as the next producer's c); its epilogue evaluates a * acc + (b * u + v).
// No inter-workgroup synchronisation, no second pass over x: both LN-modulate launches of a block (2 x 100 MB of HBM traffic) disappear for
// 33.5 MB of extra stores in each producer epilogue.  u, v: one small batched GEMM per forward over all blocks (lfm_dit_forward).
// (Rejected first, measured in round 3: normalising inside the producer epilogue behind an inter-workgroup panel counter -- correct, bit-stable,
// but 12.03 vs 11.92 ms per DiT-L/2 evaluation: the wait for the three sibling tiles cost more than the two launches it saved.)
struct RowStatSrc {
  const float* part;    // [M][tiles_p][2]
  const float* cen_in;  // [M] the c the producer used
  float* cen_out;       // [M] <- mu (written by tile column 0 only)
  int tiles_p;          // partial slots per row (the producer's column tiles)
  float inv_n, eps;     // 1 / row length, LayerNorm eps
};

// X[m][n] += gate * (acc + bias)  AND  A'[m][n] = fp16((X[m][n] - c[m]) (1 + scale[n])),  part[m][tile_n] = (sum X, sum (X - c)^2): the producer
// epilogues of epilogue_handover.h / the 256x256 kernels do the work; load / store (EpiGateResid) serve the kernels without one.
// (Round 4, measured and removed: a variant whose epilogue requested the X rows of the next 32-row pass before the stores of the current one --
// bit-identical, 10.97 vs 10.95 ms per DiT-L/2 forward.  The four-wave kernel's own producer epilogue keeps that order: it costs nothing there.)
struct EpiGateResidMod : EpiGateResid {
  half_t* A;           // [M][N], leading dimension N
  const float* scale;  // the consumer LayerNorm's scale row (+ img * mod_stride)
  long mod_stride;
  const float* cen;    // [M]
  float* part;         // [M][tiles_n][2]
  int tiles_n;
  static constexpr bool producer_mod = true;
};

// C = act(a[m] * acc + (b[m] * u[n] + v[n])) -> fp16;  (a, b) of the tile's rows sit in LDS at rs[2 (m - m0)] (filled by the kernel's prologue).
// Cols = the column side (C, u, v), Rows = the row side: rs and m0, behind the row-statistic source where the kernel reduces it itself.
struct EpiModCols {
  half_t* C;
  long ldc;
  const float* u;  // + img * uv_stride + n
  const float* v;
  long uv_stride;
  int tokens;
  struct Aux {
    f32x4 u, v;
  };
  static constexpr bool column_aux = true;
  __device__ __forceinline__ Aux load(int m, int n) const {
    const long o = (long)(m / tokens) * uv_stride + n;
    Aux a;
    a.u = *(const f32x4*)(u + o);
    a.v = *(const f32x4*)(v + o);
    return a;
  }
  __device__ __forceinline__ bool wide_ok() const { return (ldc & 7) == 0 && ((uintptr_t)C & 15) == 0; }
};
struct EpiModRows {
  const float* rs;
  int m0;
#if defined(LFM_MEASURE) && defined(LFM_EXP_DUMP)
  float* dbg;
#endif
};
struct EpiModRowsStat {
  RowStatSrc st;
  const float* rs;
  int m0;
  static constexpr bool rowstat = true;
#if defined(LFM_MEASURE) && defined(LFM_EXP_DUMP)
  float* dbg;  // [M][N / 8][16] or null
#endif
};
template <class Act, class Rows>
struct EpiModActF16 : EpiModCols, Rows {
  using Rows::m0;
  using Rows::rs;
  __device__ __forceinline__ f32x2 row_aux(int m) const { return *(const f32x2*)(rs + 2 * (m - m0)); }
  __device__ __forceinline__ void store(int m, int n, f32x4 acc, const Aux& c) const {
    const f32x2 ab = *(const f32x2*)(rs + 2 * (m - m0));
    const f32x4 x = row_affine4(ab.x, ab.y, acc, c.u, c.v);  // plain FMAs, not the packed form: common.h fma_v
    const f32x4 o = Act::apply(x);
    *(half4_t*)(C + (long)m * ldc + n) = f16x4(o);
  }
  __device__ __forceinline__ void store8(int m, int n, f32x4 lo, f32x4 hi, const Aux& cl, const Aux& ch) const {
    store8r(m, n, lo, hi, cl, ch, row_aux(m));
  }
  __device__ __forceinline__ void store8r(int m, int n, f32x4 lo, f32x4 hi, const Aux& cl, const Aux& ch, f32x2 ab) const {
#if defined(LFM_MEASURE) && defined(LFM_EXP_DUMP)
    // (experiment build, tools/cosched_dump.py) every operand of the affine as THIS lane saw it, 16 floats per (row, 8-column group):
    // acc lo | acc hi | t = b u + v for columns 0, 2, 4, 6 | (a, b) | x for columns 0, 2
    const f32x4 acc_lo = lo, acc_hi = hi;
    const f32x4 tl = ab.y * cl.u + cl.v, th = ab.y * ch.u + ch.v;
    lo = ab.x * lo + tl;
    hi = ab.x * hi + th;
    if (this->dbg && (m & 7) >= 6) {  // lanes 48-63 of the hand-over
      f32x4* d = (f32x4*)(this->dbg + ((long)m * (ldc / 8) + n / 8) * 16);
      d[0] = acc_lo;
      d[1] = acc_hi;
      d[2] = (f32x4){tl.x, tl.z, th.x, th.z};
      d[3] = (f32x4){ab.x, ab.y, lo.x, lo.z};
    }
#elif defined(LFM_EXP_AFFINE_PACKED)
    // (experiment build) the vector expression: v_pk_fma_f32 with op_sel -- the form that leaves the solo result under co-scheduling
    lo = ab.x * lo + (ab.y * cl.u + cl.v);
    hi = ab.x * hi + (ab.y * ch.u + ch.v);
#else
    lo = row_affine4(ab.x, ab.y, lo, cl.u, cl.v);
    hi = row_affine4(ab.x, ab.y, hi, ch.u, ch.v);
#endif
    const f32x4 ol = Act::apply(lo), oh = Act::apply(hi);
    *(half8_t*)(C + (long)m * ldc + n) = f16x8(ol, oh);
  }
};
struct EpiModF16 : EpiModActF16<ActIdentity, EpiModRows> {};
// fc1 of the folded path: C = gelu_tanh(a[m] * acc + (b[m] * u[n] + v[n])) -> fp16   (v carries the fc1 bias)
struct EpiModGeluF16 : EpiModActF16<ActGeluTanh, EpiModRowsStat> {};

// u / v rows of the folded path (lfm_dit_forward): rows [0, R) = (1 + scale) W^T, rows [R, 2R) = shift W^T + bias; batched over the blocks
struct EpiUV {
  float* C;
  long ldc;
  const float* bias;
  int R;
  long bs_bias;
  typedef f32x4 Aux;
  __device__ __forceinline__ void batch(int bz, long bs) {
    C += (long)bz * bs;
    bias += (long)bz * bs_bias;
  }
  __device__ __forceinline__ Aux load(int m, int n) const { return m >= R ? *(const f32x4*)(bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const { *(f32x4*)(C + (long)m * ldc + n) = v + b; }
};

// Split-K partial tile: slice bz of the K range writes its fp32 partial product to slab[bz][M][N] (see launch_gemm_splitk).
struct EpiSlabF32 {
  float* slab;
  long ldn, slice_stride;
  typedef int Aux;
  __device__ __forceinline__ void batch(int bz, long) { slab += (long)bz * slice_stride; }
  __device__ __forceinline__ Aux load(int, int) const { return 0; }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux&) const { *(f32x4*)(slab + (long)m * ldn + n) = v; }
};

// ------------------------------------------------------------------ QKV projection
// V^T token order (round 4).  Inside every group of 16 tokens a V^T row stores the tokens in the order 0 1 2 3 8 9 10 11 | 4 5 6 7 12 13 14 15 (bits 2 and
// 3 of the token index exchanged: an involution).  Why: the attention kernel's P V MFMA takes, per k-slot of 16 keys, keys {4 h + r} and {8 + 4 h + r}
// (h = lane >> 5) from one lane -- the order its S^T = K Q^T accumulators already hold P in -- so with plain token order a lane needed TWO 8-byte LDS reads
// per fragment, and the 32 lanes of a half-wave could only reach 16 of the 32 eight-byte slots of a bank row (2-way conflicts by construction: 40 % of the
// kernel's LDS cycles, profiles/r03_final_pmc_in_situ.txt).  In this order the lane's eight keys are ONE 16-byte chunk: one conflict-free ds_read_b128.
// V^T is private to the QKV projection (writer) and the attention kernels (readers).
__host__ __device__ __forceinline__ int vt_pos(int tok) { return (tok & ~12) | ((tok & 4) << 1) | ((tok & 8) >> 1); }

// QKV projection of timm Attention (DiT.py:120): columns [q | k | v], each [head][hd].
// Q,K are stored token-major [M, D]; V is stored TRANSPOSED per (image, head): Vt[img][head][d][token],
// which is the key-contiguous layout the attention kernel's P*V MFMA operand wants.
// The layout, for the epilogues E that hold  half_t *Q, *K, *Vt;  int D, tokens, tok_sh  (tok_sh = log2(tokens) when tokens is a power of two --
// every DiT configuration --, else -1: no integer division per store):
template <class E>
struct QKVLayout {
  __device__ __forceinline__ const E& e() const { return *static_cast<const E*>(this); }
  static __host__ __device__ int log2_or_neg(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return (1 << s) == v ? s : -1;
  }
  __device__ __forceinline__ half_t* vt_ptr(int n, int m) const {  // &Vt[img][head][d][tok] for column n (>= 2D) and row m
    // ((img * heads + head) * hd + d) * tokens + tok  with  head * hd + d = c  and  heads * hd = D:  no head / d split is needed
    const int c = n - 2 * e().D;
    const int img = e().tok_sh >= 0 ? (m >> e().tok_sh) : m / e().tokens, tok = m - img * e().tokens;
    return e().Vt + ((long)img * e().D + c) * e().tokens + vt_pos(tok);
  }
  // generic path: C[m][n .. n + 3] (epilogue arithmetic applied) to its place in Q, K or V^T
  __device__ __forceinline__ void store_qkv(int m, int n, f32x4 v) const {
    const int D = e().D, tokens = e().tokens;
    if (n < 2 * D) {
      half_t* dst = (n < D) ? (e().Q + (long)m * D + n) : (e().K + (long)m * D + (n - D));
      *(half4_t*)dst = f16x4(v);
    } else {
      half_t* dst = vt_ptr(n, m);  // n..n+3 stay inside one head (hd % 4 == 0)
      dst[0] = (half_t)v.x;
      dst[tokens] = (half_t)v.y;
      dst[2 * tokens] = (half_t)v.z;
      dst[3 * tokens] = (half_t)v.w;
    }
  }
  // A 256-column tile that lies inside Q or inside K is a plain "-> fp16" tile of a [M, D] matrix: kernels that
  // ask get that epilogue (no per-store Q/K/V case distinction), with C shifted so that C[m*D + n] is the right element: plain_c(n0).
  __device__ __forceinline__ bool plain_tile(int n0, int bn) const { return n0 + bn <= e().D || (n0 >= e().D && n0 + bn <= 2 * e().D); }
  __device__ __forceinline__ half_t* plain_c(int n0) const { return n0 < e().D ? e().Q : e().K - e().D; }
  // Kernels that can compute a tile TRANSPOSED (operands swapped in the MFMA) hand V tiles over as rows of V^T:
  // v = C[m..m+3][n], four consecutive tokens of one (head, d) column -> one 8-byte store (store_t).  tokens % 4 == 0.
  // store_t8: one 16-byte chunk of a V^T row: lo = tokens m .. m + 3, hi = tokens m + 8 .. m + 11 (m % 16 == 0 or 4: see vt_pos)
  __device__ __forceinline__ bool transposed(int n0) const { return n0 >= 2 * e().D; }
  __device__ __forceinline__ bool wide_t_ok() const { return (e().tokens & 15) == 0 && ((uintptr_t)e().Vt & 15) == 0; }
};

struct EpiQKV : QKVLayout<EpiQKV> {
  half_t* Q;
  half_t* K;
  half_t* Vt;
  const float* bias;
  int D, hd, tokens;
  int hd_sh, tok_sh;
  static EpiQKV make(half_t* Q, half_t* K, half_t* Vt, const float* bias, int D, int hd, int tokens) {
    return EpiQKV{{}, Q, K, Vt, bias, D, hd, tokens, log2_or_neg(hd), log2_or_neg(tokens)};
  }
  typedef f32x4 Aux;
  __device__ __forceinline__ bool direct(int n0) const { return n0 >= 2 * D; }  // V tiles: 32 consecutive tokens per lane group
  __device__ __forceinline__ Aux load(int, int n) const { return *(const f32x4*)(bias + n); }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const { store_qkv(m, n, v + b); }
  __device__ __forceinline__ EpiBiasF16 plain(int n0) const { return EpiBiasF16{plain_c(n0), (long)D, bias}; }
  __device__ __forceinline__ float load_t(int n) const { return bias[n]; }
  __device__ __forceinline__ void store_t(int n, int m, f32x4 v, float b) const {
    const f32x4 o = {v.x + b, v.y + b, v.z + b, v.w + b};
    *(half4_t*)vt_ptr(n, m) = f16x4(o);
  }
  __device__ __forceinline__ void store_t8(int n, int m, f32x4 lo, f32x4 hi, float b) const {
    const f32x4 ol = {lo.x + b, lo.y + b, lo.z + b, lo.w + b}, oh = {hi.x + b, hi.y + b, hi.z + b, hi.w + b};
    *(half8_t*)vt_ptr(n, m) = f16x8(ol, oh);
  }
};

// QKV projection of the folded path: EpiQKV's layout with the row-affine correction instead of the bias (v carries the qkv bias)
struct EpiQKVMod : QKVLayout<EpiQKVMod> {
  half_t* Q;
  half_t* K;
  half_t* Vt;
  const float* u;  // [rows][3D] (+ img * uv_stride)
  const float* v;
  long uv_stride;
  int D, hd, tokens;
  int tok_sh;
  RowStatSrc st;
  const float* rs;
  int m0;
  static constexpr bool rowstat = true;
  typedef EpiModF16::Aux Aux;
  __device__ __forceinline__ Aux load(int m, int n) const {
    const long o = (long)(m / tokens) * uv_stride + n;
    Aux a;
    a.u = *(const f32x4*)(u + o);
    a.v = *(const f32x4*)(v + o);
    return a;
  }
  __device__ __forceinline__ void store(int m, int n, f32x4 acc, const Aux& c) const {  // generic path (edge tiles of odd shapes only)
    const f32x2 ab = *(const f32x2*)(rs + 2 * (m - m0));
    const f32x4 o = row_affine4(ab.x, ab.y, acc, c.u, c.v);
    store_qkv(m, n, o);
  }
  __device__ __forceinline__ EpiModF16 plain(int n0) const { return EpiModF16{plain_c(n0), (long)D, u, v, uv_stride, tokens, rs, m0}; }
  // column constants of a V^T row: (u[n], v[n]) of the tile's image
  __device__ __forceinline__ f32x2 load_t(int n) const {
    const long o = (long)(m0 / tokens) * uv_stride + n;
    return (f32x2){u[o], v[o]};
  }
  __device__ __forceinline__ void store_t(int n, int m, f32x4 acc, f32x2 c) const {  // four consecutive tokens m .. m + 3 of column n
    const f32x4 r0 = *(const f32x4*)(rs + 2 * (m - m0)), r1 = *(const f32x4*)(rs + 2 * (m - m0) + 4);  // (a, b) x 4 rows
    half4_t h = {(half_t)fma_v(r0.x, acc.x, fma_v(r0.y, c.x, c.y)), (half_t)fma_v(r0.z, acc.y, fma_v(r0.w, c.x, c.y)),
                 (half_t)fma_v(r1.x, acc.z, fma_v(r1.y, c.x, c.y)), (half_t)fma_v(r1.z, acc.w, fma_v(r1.w, c.x, c.y))};
    *(half4_t*)vt_ptr(n, m) = h;
  }
  __device__ __forceinline__ void store_t8(int n, int m, f32x4 lo, f32x4 hi, f32x2 c) const {  // lo = tokens m .. m + 3, hi = tokens m + 8 .. m + 11
    const float* r = rs + 2 * (m - m0);
    const f32x4 r0 = *(const f32x4*)r, r1 = *(const f32x4*)(r + 4), r2 = *(const f32x4*)(r + 16), r3 = *(const f32x4*)(r + 20);
    half8_t h = {(half_t)fma_v(r0.x, lo.x, fma_v(r0.y, c.x, c.y)), (half_t)fma_v(r0.z, lo.y, fma_v(r0.w, c.x, c.y)),
                 (half_t)fma_v(r1.x, lo.z, fma_v(r1.y, c.x, c.y)), (half_t)fma_v(r1.z, lo.w, fma_v(r1.w, c.x, c.y)),
                 (half_t)fma_v(r2.x, hi.x, fma_v(r2.y, c.x, c.y)), (half_t)fma_v(r2.z, hi.y, fma_v(r2.w, c.x, c.y)),
                 (half_t)fma_v(r3.x, hi.z, fma_v(r3.y, c.x, c.y)), (half_t)fma_v(r3.z, hi.w, fma_v(r3.w, c.x, c.y))};
    *(half8_t*)vt_ptr(n, m) = h;
  }
};

// ------------------------------------------------------------------ detection of the optional parts of the interface
// batched epilogues provide a member batch(bz, stride); the default ignores the batch index
template <class Epi>
__device__ __forceinline__ auto epi_batch(Epi& e, int bz, long bs, int) -> decltype(e.batch(bz, bs), void()) {
  e.batch(bz, bs);
}
template <class Epi>
__device__ __forceinline__ void epi_batch(Epi&, int, long, long) {}

// epilogues that need the raw MFMA fragment layout (lane = consecutive m) for some column range provide direct(n0)
template <class Epi>
__device__ __forceinline__ auto epi_direct(const Epi& e, int n0, int) -> decltype(e.direct(n0)) {
  return e.direct(n0);
}
template <class Epi>
__device__ __forceinline__ bool epi_direct(const Epi&, int, long) {
  return false;
}

#define LFM_EPI_TRAIT(name, expr, val)                      \
  template <class Epi, class = void>                        \
  struct name {                                             \
    static constexpr bool value = false;                    \
  };                                                        \
  template <class Epi>                                      \
  struct name<Epi, decltype((void)(expr))> {                \
    static constexpr bool value = val;                      \
  }
LFM_EPI_TRAIT(epi_has_store8, &Epi::store8, true);
// kernels may load a column-only auxiliary operand once per tile, AHEAD of the first store (vmcnt counts stores too and returns in order, so a bias load
// issued after a block's stores waits for those stores to drain -- profiles/r02_epilogue_trace.txt, the "aux" column of the bias epilogues)
LFM_EPI_TRAIT(epi_column_aux, Epi::column_aux, Epi::column_aux);
// in the row-major hand-over a lane always owns the SAME eight columns n0 + 64 wn + 8 (lane & 7) and rows of the 128-row half g
LFM_EPI_TRAIT(epi_has_finish_tile, &Epi::finish_tile, true);
LFM_EPI_TRAIT(epi_has_finish_slab, &Epi::finish_slab, true);
LFM_EPI_TRAIT(epi_has_row_aux, &Epi::row_aux, true);
LFM_EPI_TRAIT(epi_has_rowstat, Epi::rowstat, Epi::rowstat);
LFM_EPI_TRAIT(epi_is_producer_mod, Epi::producer_mod, Epi::producer_mod);
LFM_EPI_TRAIT(epi_has_transposed, ((const Epi*)nullptr)->transposed(0), true);
LFM_EPI_TRAIT(epi_has_plain, ((const Epi*)nullptr)->plain(0), true);
#undef LFM_EPI_TRAIT
