// NHWC-fp16 pieces that the VAE (vae.hip) and the UNet building blocks (ops.hip) share: the implicit-GEMM A source of a 3x3 convolution, the
// "acc + bias (+ residual)" epilogues (one of which leaves GroupNorm statistics: the slot arithmetic, the row-wise statistics kernel and the rest
// of what the two GroupNorms share are groupnorm_common.h, included here), and the gate in front of the halo-tiled convolution kernels.
#pragma once
#include "gemm_dispatch.h"
#include "conv_halo_kernel.h"
#include "groupnorm_common.h"  // gn_slot (EpiConvStatsF16), gn_merge, gn_mean_rstd, GnIn, gn_walk, gn_stats_rows_kernel, GN_MAX_SLABS

// ------------------------------------------------------------------ implicit-GEMM A source, NHWC fp16, 3x3
// M = N*H*W output pixels, K = 9*Cin with k = tap*Cin + ci; the gather (shifted pixel rows, zero padding) is the per-lane source address.
// MODE 0: same size, pad 1.  MODE 1: pad 1 on the nearest-2x upsampled input, never materialised (unet.py Upsample, diffusers Upsample2D).
// MODE 2: stride 2, pad 1 (ADM Downsample, unet.py:103-128): output (oy, ox) reads input (2oy + ky - 1, 2ox + kx - 1).
// MODE 3: stride 2 on the input padded (0,1,0,1) (diffusers Downsample2D, padding=0): reads (2oy + ky, 2ox + kx), zero beyond the bottom / right edge.
template <int MODE>
struct ASrcConv {
  const half_t* in;     // [N, Hi, Wi, Cin]: Hi = H (mode 0), H / 2 (mode 1), 2 H (modes 2, 3)
  const half_t* zeros;  // >= 64 halves of zeros (padding rows)
  int H, W, Cin, M;     // OUTPUT spatial size; M = N*H*W
  int tap, ci0;         // k-tile state: k0 = tap*Cin + ci0 (a 64-wide k tile never straddles a tap: Cin % 64 == 0)
  int tap_begin, ci_begin;  // split-K: slice bz starts at k = bz * bs (init), a multiple of 64 <= Cin granularity; batch 1, bs 0: tap 0
  __device__ __forceinline__ void init(int bz, long bs) {
    const long k = (long)bz * bs;
    tap_begin = (int)(k / Cin);
    ci_begin = (int)(k - (long)tap_begin * Cin);
  }
  struct Row {
    int n, y, x;
  };
  __device__ __forceinline__ Row row(int m) const {
    if (m >= M) m = M - 1;
    Row r;
    r.x = m % W;
    const int t = m / W;
    r.y = t % H;
    r.n = t / H;
    return r;
  }
  __device__ __forceinline__ void begin_tile(int kt, int bk) {  // called with kt = 0, 1, 2, ... in order
    if (kt == 0) {
      tap = tap_begin;
      ci0 = ci_begin;
    } else {
      ci0 += bk;
      if (ci0 >= Cin) {
        ci0 = 0;
        ++tap;
      }
    }
  }
  __device__ __forceinline__ const half_t* ptr(const Row& r, int koff) const {
    constexpr int PAD = MODE == 3 ? 0 : 1;
    const int dy = tap / 3 - PAD, dx = tap % 3 - PAD;
    if (MODE >= 2) {
      const int Hi = H * 2, Wi = W * 2;
      const int iy = 2 * r.y + dy, ix = 2 * r.x + dx;
      if ((unsigned)iy >= (unsigned)Hi || (unsigned)ix >= (unsigned)Wi) return zeros + koff;
      return in + (((long)r.n * Hi + iy) * Wi + ix) * Cin + ci0 + koff;
    }
    const int iy = r.y + dy, ix = r.x + dx;
    if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) return zeros + koff;
    const int Hs = H >> (MODE == 1), Ws = W >> (MODE == 1);
    return in + (((long)r.n * Hs + (iy >> (MODE == 1))) * Ws + (ix >> (MODE == 1))) * Cin + ci0 + koff;
  }
};

// ------------------------------------------------------------------ epilogues
struct EpiResidF16 {  // out = (acc + bias (+ residual)) * scale -> fp16
  half_t* C;
  long ldc;
  const float* bias;    // may be null
  const half_t* resid;  // may be null; same layout as C
  float scale = 1.0f;   // applied in fp32 to the finished sum (EDM UNetBlock skip_scale, models/EDM.py:272-274,290-291); x * 1.0f is exact: the default changes no bit
  struct Aux {
    f32x4 b;
    half4_t r;
  };
  __device__ __forceinline__ Aux load(int m, int n) const {
    Aux a;
    a.b = bias ? *(const f32x4*)(bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f};
    a.r = resid ? *(const half4_t*)(resid + (long)m * ldc + n) : (half4_t){0, 0, 0, 0};
    return a;
  }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& a) const {
    v += a.b;
    half4_t h = {(half_t)((v.x + (float)a.r.x) * scale), (half_t)((v.y + (float)a.r.y) * scale), (half_t)((v.z + (float)a.r.z) * scale),
                 (half_t)((v.w + (float)a.r.w) * scale)};
    *(half4_t*)(C + (long)m * ldc + n) = h;
  }
  __device__ __forceinline__ bool wide_ok() const { return (ldc & 7) == 0 && ((uintptr_t)C & 15) == 0 && (!resid || ((uintptr_t)resid & 15) == 0); }
  __device__ __forceinline__ half8_t round8(f32x4 lo, f32x4 hi, const Aux& al, const Aux& ah) const {  // eight columns of one row, as stored
    lo += al.b;
    hi += ah.b;
    return (half8_t){(half_t)((lo.x + (float)al.r.x) * scale), (half_t)((lo.y + (float)al.r.y) * scale), (half_t)((lo.z + (float)al.r.z) * scale),
                     (half_t)((lo.w + (float)al.r.w) * scale), (half_t)((hi.x + (float)ah.r.x) * scale), (half_t)((hi.y + (float)ah.r.y) * scale),
                     (half_t)((hi.z + (float)ah.r.z) * scale), (half_t)((hi.w + (float)ah.r.w) * scale)};
  }
  __device__ __forceinline__ void store8(int m, int n, f32x4 lo, f32x4 hi, const Aux& al, const Aux& ah) const {
    *(half8_t*)(C + (long)m * ldc + n) = round8(lo, hi, al, ah);
  }
};

// EpiResidF16 with a per-image fp32 row added to the sum: out = (acc + bias + resid + vec[m / tokens][n]) * scale -> fp16.  The `attn1.proj` linear of EDM's
// TransformerBlock (models/EDM.py:477-483) under a one-key context: attn2(norm2(x), context) is the same vector u[label] at every pixel, so this one
// epilogue performs x = attn1(norm1(x)) + x and x = attn2(..) + x (UNet section).  The row joins the bias in load(), in fp32 (bias + 0 is the
// bias: a null or all-zero `vec` changes no bit of EpiResidF16's result); everything after load() IS EpiResidF16 -- same Aux, same rounding, same
// 16-byte-store path, so the 256-row hand-over (epilogue_handover.h: per-(row, column) auxiliary loads ahead of a pass's stores) serves it unchanged.
struct EpiResidVecF16 {
  EpiResidF16 e;
  const float* vec;  // may be null; rows vec_stride apart, vec_stride % 4 == 0 and 16-byte aligned (f32x4 loads)
  long vec_stride;
  int tokens;        // rows of C per row of vec
  typedef EpiResidF16::Aux Aux;
  __device__ __forceinline__ Aux load(int m, int n) const {
    Aux a = e.load(m, n);
    if (vec) a.b += *(const f32x4*)(vec + (long)(m / tokens) * vec_stride + n);
    return a;
  }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& a) const { e.store(m, n, v, a); }
  __device__ __forceinline__ bool wide_ok() const { return e.wide_ok(); }
  __device__ __forceinline__ half8_t round8(f32x4 lo, f32x4 hi, const Aux& al, const Aux& ah) const { return e.round8(lo, hi, al, ah); }
  __device__ __forceinline__ void store8(int m, int n, f32x4 lo, f32x4 hi, const Aux& al, const Aux& ah) const { e.store8(m, n, lo, hi, al, ah); }
};

struct EpiNCHWF32 {  // Cout <= 4 output conv (the VAE decoder's `.sample` image, the UNets' out conv): fp32 NCHW, channels beyond nch are padding
  float* out;
  const float* bias;  // [4]
  int HW, nch;
  typedef f32x4 Aux;
  __device__ __forceinline__ Aux load(int, int n) const { return *(const f32x4*)(bias + n); }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const {
    if (n != 0) return;
    v += b;
    const int img = m / HW, pix = m - img * HW;
    float* o = out + (long)img * nch * HW + pix;
    o[0] = v.x;
    if (nch > 1) o[HW] = v.y;
    if (nch > 2) o[2 * HW] = v.z;
    if (nch > 3) o[3 * HW] = v.w;
  }
};

// EpiResidF16 that also leaves the GroupNorm statistics of what it stores (round 3): the next layer of every VAE resnet is a GroupNorm over exactly
// this tensor, and its statistics pass (gn_stats_rows_kernel) re-read it from HBM just to add it up.  In the row-major hand-over of the 256-row kernels
// a lane owns the same eight output columns for all of its rows, so it keeps shifted sums of the ROUNDED fp16 values per half-octet (a group is >= 4
// channels wide) in registers, folds the eight lanes that share its columns at the end of the tile, and writes one fixed slot per (image, 128-row
// slab, half-octet): part[n][slab][C / 4] = {mean, M2} of its 512 values, the layout gn_finish_kernel merges in a fixed order -- deterministic, no
// atomics.  Shifted: a lane's sums are of x - k with k its own first value of the half-octet; the finish re-shifts the eight lanes to one pivot
// before they are added.  Host-side preconditions (vae.hip: conv3): HW % 256 == 0 (a tile lies in one image), the halo kernel or the 256x128 /
// 256x256 implicit GEMM, 16-byte-store path.
struct EpiConvStatsF16 {
  EpiResidF16 e;
  float* part;  // [n][slabs][ldc / 4][2]
  int HW, slabs;
  mutable float s0 = 0.f, q0 = 0.f, s1 = 0.f, q1 = 0.f;  // sums of (x - k0), (x - k0)^2 over half-octet 0, the same for half-octet 1 around k1
  mutable float k0 = 0.f, k1 = 0.f, cnt = 0.f;           // shifts (set by the first store8) and values per half-octet so far
  typedef EpiResidF16::Aux Aux;
  __device__ __forceinline__ Aux load(int m, int n) const { return e.load(m, n); }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& a) const { e.store(m, n, v, a); }  // (4-column path: not used with statistics, kept for the interface)
  __device__ __forceinline__ bool wide_ok() const { return true; }  // checked on the host
  __device__ __forceinline__ void store8(int m, int n, f32x4 lo, f32x4 hi, const Aux& al, const Aux& ah) const {
    const half8_t h = e.round8(lo, hi, al, ah);
    *(half8_t*)(e.C + (long)m * e.ldc + n) = h;
    if (cnt == 0.f) {
      k0 = (float)h[0];
      k1 = (float)h[4];
    }
    cnt += 4.f;
    const float f0 = (float)h[0] - k0, f1 = (float)h[1] - k0, f2 = (float)h[2] - k0, f3 = (float)h[3] - k0;
    const float f4 = (float)h[4] - k1, f5 = (float)h[5] - k1, f6 = (float)h[6] - k1, f7 = (float)h[7] - k1;
    s0 += (f0 + f1) + (f2 + f3);
    q0 += (f0 * f0 + f1 * f1) + (f2 * f2 + f3 * f3);
    s1 += (f4 + f5) + (f6 + f7);
    q1 += (f4 * f4 + f5 * f5) + (f6 * f6 + f7 * f7);
  }
  // fold the eight lanes that own the same columns and write the wave's slot: columns ncol0 + 8 (lane & 7) .. + 7 of slab `slab` of image `img`
  __device__ __forceinline__ void finish_slab(int img, int slab, int ncol0, int lane) const {
    // re-shift every lane's sums to the shifts of lane (lane & 7): sum (x - p) = s + c d, sum (x - p)^2 = q + d (2 s + c d) with d = k - p
    const float p0 = __shfl(k0, lane & 7, 64), p1 = __shfl(k1, lane & 7, 64);
    const float d0 = k0 - p0, d1 = k1 - p1;
    float a = s0 + cnt * d0, b = q0 + d0 * (2.f * s0 + cnt * d0), c = s1 + cnt * d1, d = q1 + d1 * (2.f * s1 + cnt * d1), t = cnt;
#pragma unroll
    for (int o = 8; o < 64; o <<= 1) {  // the eight lanes lane & 7, + 8, .., + 56 own the same columns
      a += __shfl_xor(a, o, 64);
      b += __shfl_xor(b, o, 64);
      c += __shfl_xor(c, o, 64);
      d += __shfl_xor(d, o, 64);
      t += __shfl_xor(t, o, 64);
    }
    if (lane < 8) {  // {mean, M2} per half-octet
      float* o = part + (((long)img * slabs + slab) * (e.ldc >> 2) + ((ncol0 + lane * 8) >> 2)) * 2;
      const float r = 1.f / t;
      gn_slot(o, p0, a, b, r);
      gn_slot(o + 2, p1, c, d, r);
    }
  }
  __device__ __forceinline__ void finish_tile(int m0, int n0, int g, int wn, int lane) const {
    const int img = m0 / HW;
    finish_slab(img, ((m0 - img * HW) >> 8) * 2 + g, n0 + wn * 64, lane);
  }
};

// ------------------------------------------------------------------ halo kernel or implicit GEMM
// May the halo-tiled kernels (conv_halo_kernel.h) be tried for this output / residual: the automatic kernel choice, 16-byte stores, and
// CONV_IMPLICIT_GEMM (the implicit GEMM instead: A/B and parity tests) not set.  The launchers still answer 1 for shapes that are not theirs.
static inline bool conv_halo_allowed(const void* out = nullptr, const void* resid = nullptr) {
  return lfm_gemm_selected() == 0 && !(lfm_gemm_debug_flags() & LFM_DBG_CONV_IMPLICIT_GEMM) && !(((uintptr_t)out | (uintptr_t)resid) & 15);
}

// The <= 4-channel output convolution (fp16 NHWC -> fp32 NCHW; w4 fp16 [4][9][Cin]) of the UNets and the VAE decoder: the halo-tiled kernel, or the
// implicit GEMM on four columns where that one declines.  zeros: the caller's zero page.  (fp32 scalar stores: no alignment term in the gate.)
static inline int launch_conv3x3_out(const half_t* in, const half_t* zeros, const half_t* w4, int N, int H, int W, int Cin, const EpiNCHWF32& eo,
                                     hipStream_t st) {
  if (conv_halo_allowed()) {
    const int rc = launch_conv3x3_halo_out(in, zeros, w4, N, H, W, Cin, eo, st);
    if (rc != 1) return rc;
  }
  const int M = N * H * W;
  return launch_gemm_tn(ASrcConv<0>{in, zeros, H, W, Cin, M}, w4, 9L * Cin, M, 4, 9 * Cin, eo, st);
}
