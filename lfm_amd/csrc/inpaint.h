// The elementwise work around the three heavy steps of an inpainting batch (downstream_tasks/test_flow_latent_inpainting.py: the dataset class :36-55, the
// loop :147-150 and :157-160, torchvision.utils.save_image's quantisation), from the bytes the files hold: uint8 NHWC images and the mask PNG's bytes
// (255 = keep, 0 = hole).  Three launches replace about twenty torch ops over seven full-resolution fp32 tensors, and 4 bytes per pixel cross to the device
// where 28 did:
//   lfm_inpaint_prepare_u8    bytes -> the VAE encoder's input (masked image, NCHW in [-1,1]), optionally the image itself, and the mask on the latent grid
//   lfm_inpaint_cond_f32      the encoder's moments (+ noise) -> channels 0..3 of the conditioning tensor: the scaled posterior sample or mode
//   lfm_inpaint_composite_u8  decoded sample + bytes -> the composite's uint8 NHWC bytes, as save_image quantises them
//
// Bit for bit.  prepare and composite restate the reference's fp32 operation sequence with every operation rounded on its own.  hipcc contracts a * b + c
// into one FMA by default (-ffp-contract=fast-honor-pragmas), and the header's __fmul_rn / __fadd_rn are plain operators that contract like any other once
// inlined; so every function below that does arithmetic switches contraction off for its own body (#pragma clang fp contract(off)), which that default
// honours.  The pragma stands inside the functions: at file scope it would reach the code included after this header.  The division of a byte by 255 is
// the correctly rounded quotient (inp_unit below); (x + 1) / 2 is exact as a product with 0.5.  The LFM_FAST_MATH=1 A/B build (-ffast-math) is NOT covered: it may
// contract, reassociate and replace the division and expf, and the bit-for-bit tests are not expected to pass on it.
//
// Work split (HBM-bound streaming kernels, no LDS: a lane's pixels are adjacent in both layouts, so nothing needs transposing between lanes).  A lane owns P
// adjacent pixels of one image row (W % 8 == 0 keeps a group of 8 inside its row, W % 16 == 0 a group of 16): 3P image bytes and P mask bytes on the NHWC side,
// P floats per channel plane on the NCHW side; consecutive lanes take consecutive groups, so a wave's accesses are contiguous runs in every tensor.
//   P = 16: W % 16 == 0 and every pointer 16-byte aligned -- 16-byte loads (3 + 1 per lane) and 16-byte stores
//   P = 8 : every byte pointer 8-byte and every float pointer 16-byte aligned -- 8-byte loads of the bytes (a group's 24 image bytes are only 8-byte
//           aligned), 16-byte accesses of the floats
//   P = 8, scalar: any other alignment the element types allow (a float pointer must be 4-byte aligned: LFM_ERR_ALIGN otherwise) -- written one element
//           per access and assuming the element's own alignment only (the compiler may merge neighbours into wider unaligned accesses, which global
//           memory serves)
// The three variants compute the same bits.  The mask on the latent grid is one 4-byte store per 8 x 8 pixels (mask_latent needs 4-byte alignment only).
#pragma once
#include "common.h"

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef float inp_f32x4 __attribute__((ext_vector_type(4)));

// NB bytes at p (NB % 8 == 0) as little-endian words: 16-byte loads (WIDE), 8-byte loads (VEC) or byte loads.
template <int NB, bool VEC, bool WIDE>
__device__ __forceinline__ void inp_load_bytes(const uint8_t* __restrict__ p, unsigned (&w)[NB / 4]) {
  if constexpr (VEC && WIDE) {
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) {
      const u32x4 v = ((const u32x4*)p)[k];
      w[4 * k] = v[0], w[4 * k + 1] = v[1], w[4 * k + 2] = v[2], w[4 * k + 3] = v[3];
    }
  } else if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < NB / 8; ++k) {
      const u32x2 v = ((const u32x2*)p)[k];
      w[2 * k] = v[0], w[2 * k + 1] = v[1];
    }
  } else {
#pragma unroll
    for (int k = 0; k < NB / 4; ++k) w[k] = p[4 * k] | (unsigned)p[4 * k + 1] << 8 | (unsigned)p[4 * k + 2] << 16 | (unsigned)p[4 * k + 3] << 24;
  }
}
template <int NB, bool VEC, bool WIDE>
__device__ __forceinline__ void inp_store_bytes(uint8_t* __restrict__ p, const unsigned (&w)[NB / 4]) {
  if constexpr (VEC && WIDE) {
#pragma unroll
    for (int k = 0; k < NB / 16; ++k) ((u32x4*)p)[k] = u32x4{w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]};
  } else if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < NB / 8; ++k) ((u32x2*)p)[k] = u32x2{w[2 * k], w[2 * k + 1]};
  } else {
#pragma unroll
    for (int k = 0; k < NB; ++k) p[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}
template <int NW>
__device__ __forceinline__ unsigned inp_byte(const unsigned (&w)[NW], int k) { return (w[k >> 2] >> (8 * (k & 3))) & 255u; }

template <int P, bool VEC>
__device__ __forceinline__ void inp_load_floats(const float* __restrict__ p, float (&v)[P]) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < P / 4; ++k) {
      const inp_f32x4 q = ((const inp_f32x4*)p)[k];
      v[4 * k] = q[0], v[4 * k + 1] = q[1], v[4 * k + 2] = q[2], v[4 * k + 3] = q[3];
    }
  } else {
#pragma unroll
    for (int k = 0; k < P; ++k) v[k] = p[k];
  }
}
template <int P, bool VEC>
__device__ __forceinline__ void inp_store_floats(float* __restrict__ p, const float (&v)[P]) {
  if constexpr (VEC) {
#pragma unroll
    for (int k = 0; k < P / 4; ++k) ((inp_f32x4*)p)[k] = inp_f32x4{v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]};
  } else {
#pragma unroll
    for (int k = 0; k < P; ++k) p[k] = v[k];
  }
}

// The dataset's values of one byte (reference :42-47, :51-53), each operation rounded on its own.
// img.astype(np.float32) / 255.0, mask / 255.0: the correctly rounded quotient, as the IEEE division gives it, in three instructions instead of the
// division's ten (its scaling and fix-up steps serve denormal and huge operands, and a byte over 255 is neither).  With y = RN(1 / 255) and q = RN(x y), the
// residual r = x - 255 q is exact in one FMA and RN(q + r y) is the correctly rounded x / 255 (Markstein); tests/test_inpaint_ref.py checks all 256 bytes
// in exact rational arithmetic, the all-pairs GPU test checks them on the device.  The two FMAs here are written, not contracted.
__device__ __forceinline__ float inp_unit(unsigned b) {
#pragma clang fp contract(off)
  const float x = (float)b, y = 1.0f / 255.0f;
  const float q = x * y;
  const float r = __builtin_fmaf(-q, 255.0f, x);
  return __builtin_fmaf(r, y, q);
}
__device__ __forceinline__ float inp_pm1(float v) {  // v * 2.0 - 1.0
#pragma clang fp contract(off)
  const float d = v * 2.0f;
  return d - 1.0f;
}
__device__ __forceinline__ float inp_01(float v) {  // to_range_0_1 (:98): (v + 1.0) / 2.0
#pragma clang fp contract(off)
  const float s = v + 1.0f;
  return s / 2.0f;
}

template <int P, bool VEC>
__global__ __launch_bounds__(256) void inpaint_prepare_kernel(const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask, float* __restrict__ masked,
                                                              float* __restrict__ image, float* __restrict__ mlat, long mlat_stride, int H, int W,
                                                              long groups) {
#pragma clang fp contract(off)
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const long HW = (long)H * W, p0 = g * P, n = p0 / HW, rem = p0 - n * HW;
  const int y = (int)(rem / W), x = (int)(rem - (long)y * W);
  unsigned iw[3 * P / 4], mw[P / 4];
  inp_load_bytes<3 * P, VEC, P == 16>(img + 3 * p0, iw);
  inp_load_bytes<P, VEC, P == 16>(mask + p0, mw);
  float m[P], keep[P];
#pragma unroll
  for (int k = 0; k < P; ++k) {
    m[k] = 1.0f - inp_unit(inp_byte(mw, k));  // mask = 1 - mask / 255: 1 = hole
    keep[k] = 1.0f - m[k];
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float a[P], b[P];
#pragma unroll
    for (int k = 0; k < P; ++k) {
      const float i = inp_unit(inp_byte(iw, 3 * k + c));
      const float mi = keep[k] * i;  // masked_img = (1 - mask) * img
      a[k] = inp_pm1(mi);
      b[k] = inp_pm1(i);
    }
    inp_store_floats<P, VEC>(masked + (n * 3 + c) * HW + rem, a);
    if (image) inp_store_floats<P, VEC>(image + (n * 3 + c) * HW + rem, b);
  }
  if ((y & 7) == 0) {  // F.interpolate(mask, size=(H/8, W/8)), nearest: the pick [::8, ::8]
#pragma unroll
    for (int k = 0; k < P; k += 8) mlat[n * mlat_stride + (long)(y >> 3) * (W >> 3) + ((x + k) >> 3)] = inp_pm1(m[k]);
  }
}

template <int P, bool VEC>
__global__ __launch_bounds__(256) void inpaint_composite_kernel(const float* __restrict__ fake, const uint8_t* __restrict__ img, const uint8_t* __restrict__ mask,
                                                                uint8_t* __restrict__ out, int H, int W, long groups) {
#pragma clang fp contract(off)
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= groups) return;
  const long HW = (long)H * W, p0 = g * P, n = p0 / HW, rem = p0 - n * HW;
  unsigned iw[3 * P / 4], mw[P / 4], ow[3 * P / 4];
  float f[3][P];
#pragma unroll
  for (int c = 0; c < 3; ++c) inp_load_floats<P, VEC>(fake + (n * 3 + c) * HW + rem, f[c]);
  inp_load_bytes<3 * P, VEC, P == 16>(img + 3 * p0, iw);
  inp_load_bytes<P, VEC, P == 16>(mask + p0, mw);
#pragma unroll
  for (int k = 0; k < 3 * P / 4; ++k) ow[k] = 0;
#pragma unroll
  for (int k = 0; k < P; ++k) {
    const float mm = inp_01(inp_pm1(1.0f - inp_unit(inp_byte(mw, k))));  // the dataset's mask in {-1..1}, then to_range_0_1 (:158)
    const float keep = 1.0f - mm;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float i01 = inp_01(inp_pm1(inp_unit(inp_byte(iw, 3 * k + c))));  // the dataset's image in [-1,1], then to_range_0_1 (:159)
      const float f01 = inp_01(f[c][k]);                                     // :157
      const float t0 = f01 * mm, t1 = keep * i01;
      const float o = t0 + t1;  // :160
      // save_image: mul(255).add_(0.5).clamp_(0, 255).to(uint8).  fmaxf / fminf drop a NaN: NaN -> 0, +inf -> 255, -inf -> 0
      const float q = o * 255.0f;
      const float r = fminf(fmaxf(q + 0.5f, 0.0f), 255.0f);
      ow[(3 * k + c) >> 2] |= (unsigned)r << (8 * ((3 * k + c) & 3));
    }
  }
  inp_store_bytes<3 * P, VEC, P == 16>(out + 3 * p0, ow);
}

// out[n][c][:] = (mean + expf(0.5f * clamp(logvar, -30, 20)) * eps) * scale, c < 4: diffusers' DiagonalGaussianDistribution.sample() and the loop's
// .mul_(scale_factor) (:147).  expf is the library's accurate one (no -ffast-math: the OCML routine, documented at 1 ulp), not the v_exp_f32 approximation.
template <bool VEC>
__global__ __launch_bounds__(256) void inpaint_cond_kernel(const float* __restrict__ moments, const float* __restrict__ eps, float scale,
                                                           float* __restrict__ out, long out_stride, long per_image, long total) {
#pragma clang fp contract(off)
  constexpr int V = VEC ? 4 : 1;
  const long t = ((long)blockIdx.x * 256 + threadIdx.x) * V;
  if (t >= total) return;
  const long n = t / per_image, r = t - n * per_image;  // per_image = 4 * hw
  float mean[V], lv[V], e[V], o[V];
  inp_load_floats<V, VEC>(moments + n * 2 * per_image + r, mean);
  if (eps) {
    inp_load_floats<V, VEC>(moments + n * 2 * per_image + per_image + r, lv);
    inp_load_floats<V, VEC>(eps + t, e);
  }
#pragma unroll
  for (int k = 0; k < V; ++k) {
    if (eps) {
      const float l = lv[k] < -30.0f ? -30.0f : (lv[k] > 20.0f ? 20.0f : lv[k]);  // torch.clamp: a NaN stays a NaN
      const float sd = expf(0.5f * l);
      const float se = sd * e[k];
      const float s = mean[k] + se;
      o[k] = s * scale;
    } else {
      o[k] = mean[k] * scale;  // dist.mode() * scale_factor: exact
    }
  }
  inp_store_floats<V, VEC>(out + n * out_stride + r, o);
}

static inline bool inp_aligned(const void* p, int a) { return !((uintptr_t)p & (uintptr_t)(a - 1)); }

// 16: P = 16 vector, 8: P = 8 vector, 1: P = 8 scalar, 0: refused (a float pointer that is not 4-byte aligned).  floats[i] may be NULL.
static int inp_variant(const void* const* bytes, int nbytes, const void* const* floats, int nfloats, int W) {
  bool a16 = W % 16 == 0, a8 = true, f16 = true;
  for (int i = 0; i < nbytes; ++i) a16 = a16 && inp_aligned(bytes[i], 16), a8 = a8 && inp_aligned(bytes[i], 8);
  for (int i = 0; i < nfloats; ++i) {
    if (!inp_aligned(floats[i], 4)) return 0;
    f16 = f16 && inp_aligned(floats[i], 16);
  }
  return a16 && f16 ? 16 : (a8 && f16 ? 8 : 1);
}

extern "C" int lfm_inpaint_prepare_u8(const uint8_t* img_nhwc, const uint8_t* mask, float* masked_nchw, float* image_nchw, float* mask_latent,
                                      long mask_latent_image_stride, int N, int H, int W, lfm_stream_t stream) {
  if (!img_nhwc || !mask || !masked_nchw || !mask_latent) return LFM_ERR_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8 || mask_latent_image_stride < (long)(H / 8) * (W / 8)) return LFM_ERR_SHAPE;
  if (!inp_aligned(mask_latent, 4)) return LFM_ERR_ALIGN;
  const void* bytes[2] = {img_nhwc, mask};
  const void* floats[2] = {masked_nchw, image_nchw};
  const int v = inp_variant(bytes, 2, floats, 2, W);
  if (!v) return LFM_ERR_ALIGN;
  const long pixels = (long)N * H * W, groups = pixels / (v == 16 ? 16 : 8);
  if (groups + 255 > 0x7fffffffL * 256) return LFM_ERR_SHAPE;
  const dim3 grid((unsigned)((groups + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
#define LFM_INP_PREPARE(P, VEC) \
  hipLaunchKernelGGL((inpaint_prepare_kernel<P, VEC>), grid, dim3(256), 0, st, img_nhwc, mask, masked_nchw, image_nchw, mask_latent, \
                     mask_latent_image_stride, H, W, groups)
  if (v == 16) LFM_INP_PREPARE(16, true);
  else if (v == 8) LFM_INP_PREPARE(8, true);
  else LFM_INP_PREPARE(8, false);
#undef LFM_INP_PREPARE
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_inpaint_composite_u8(const float* fake_nchw, const uint8_t* img_nhwc, const uint8_t* mask, uint8_t* out_nhwc, int N, int H, int W,
                                        lfm_stream_t stream) {
  if (!fake_nchw || !img_nhwc || !mask || !out_nhwc) return LFM_ERR_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || H % 8 || W % 8) return LFM_ERR_SHAPE;
  const void* bytes[3] = {img_nhwc, mask, out_nhwc};
  const void* floats[1] = {fake_nchw};
  const int v = inp_variant(bytes, 3, floats, 1, W);
  if (!v) return LFM_ERR_ALIGN;
  const long pixels = (long)N * H * W, groups = pixels / (v == 16 ? 16 : 8);
  if (groups + 255 > 0x7fffffffL * 256) return LFM_ERR_SHAPE;
  const dim3 grid((unsigned)((groups + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
#define LFM_INP_COMPOSITE(P, VEC) \
  hipLaunchKernelGGL((inpaint_composite_kernel<P, VEC>), grid, dim3(256), 0, st, fake_nchw, img_nhwc, mask, out_nhwc, H, W, groups)
  if (v == 16) LFM_INP_COMPOSITE(16, true);
  else if (v == 8) LFM_INP_COMPOSITE(8, true);
  else LFM_INP_COMPOSITE(8, false);
#undef LFM_INP_COMPOSITE
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_inpaint_cond_f32(const float* moments, const float* eps, float scale, float* out, long out_image_stride, int N, int hw,
                                    lfm_stream_t stream) {
  if (!moments || !out) return LFM_ERR_ARG;
  if (N <= 0 || hw <= 0 || out_image_stride < 4L * hw) return LFM_ERR_SHAPE;
  if (!inp_aligned(moments, 4) || !inp_aligned(eps, 4) || !inp_aligned(out, 4)) return LFM_ERR_ALIGN;
  const long per_image = 4L * hw, total = per_image * N;
  // four elements per lane where no group of four is split or misaligned: hw % 4 == 0 keeps both halves of the moments and every image's eps on a 16-byte
  // boundary when the bases are
  const bool vec = inp_aligned(moments, 16) && inp_aligned(eps, 16) && inp_aligned(out, 16) && out_image_stride % 4 == 0 && hw % 4 == 0;
  const long lanes = vec ? total / 4 : total;
  const dim3 grid((unsigned)((lanes + 255) / 256));
  hipStream_t st = (hipStream_t)stream;
  if (vec) hipLaunchKernelGGL(inpaint_cond_kernel<true>, grid, dim3(256), 0, st, moments, eps, scale, out, out_image_stride, per_image, total);
  else hipLaunchKernelGGL(inpaint_cond_kernel<false>, grid, dim3(256), 0, st, moments, eps, scale, out, out_image_stride, per_image, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
