// Per-image SSIM of two image batches, and the per-image sum of a mask's bytes, in one tile kernel and one small reduce kernel: the arithmetic of the
// reference's datasets_prep/inpaint_preprocess/losses/ssim.py (SSIM._ssim :47-67 with size_average=False, the window of _gaussian / _create_window :36-45)
// as the inpainting evaluator uses it (losses/base_loss.py: SSIMScore; evaluator.py: the mask's area per image).  The reference runs five depthwise
// window_size x window_size F.conv2d calls and about fifteen elementwise ops over full-resolution fp32 tensors; here an image pair is read once, 6 bytes
// per pixel from uint8 NHWC (7 with the mask) or 8 * C from fp32 NCHW, and one float per image is written.
//
//   lfm_ssim_u8    uint8 NHWC [N,H,W,3] pairs, each byte / 255 as inp_unit (inpaint.h) gives it: what the evaluator's dataset makes of a file
//   lfm_ssim_f32   fp32 NCHW [N,C,H,W] pairs, 1 <= C <= 4, used as they are
//
// Operation order (tests/ssim_cases.py restates it in numpy and derives the error bound from it).  x, y the two images' values of one channel, 0 outside the
// image (zero padding, window_size / 2 wide); w the 1-D window the caller passes (window_size floats; the reference's 2-D window is its fp32 outer
// product, so the separable form differs from it by rounding only).  Every product below is rounded on its own (contraction is off in the kernel's body);
// the window sums are explicit FMAs, taps in ascending order from an accumulator of 0:
//   q in {x, y, x*x, y*y, x*y}                          the three products rounded to fp32
//   h_q[r][c] = sum_k w[k] * q[r][c + k]                horizontal pass, acc = fmaf(w[k], q, acc)
//   v_q[r][c] = sum_k w[k] * h_q[r + k][c]              vertical pass, the same
//   mu1 = v_x, mu2 = v_y, m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2
//   s11 = v_xx - m11, s22 = v_yy - m22, s12 = v_xy - m12
//   map = ((2 * m12 + C1) * (2 * s12 + C2)) / ((m11 + m22 + C1) * (s11 + s22 + C2))      C1 = (float)0.01**2, C2 = (float)0.03**2, IEEE division
// For identical images m11 == m22 == m12 and s11 == s22 == s12 bit for bit (the same operations on the same operands), 2 * m12 == m11 + m22 exactly, so
// numerator and denominator are the same float and the map is exactly 1.0f.  With contraction on, 2 * m12 + C1 could become one FMA of mu1 * mu2 while
// m11 + m22 + C1 cannot, and identical images would stop scoring exactly 1.
//
// Work split.  One workgroup of 256 lanes (4 waves) per (image, 32 x 32 tile of outputs); the channels are a loop inside the workgroup.  Per channel the tile
// and its halo of r = window_size / 2 pixels (at most 42 x 42) are staged in the LDS as fp32 for both images, the horizontal pass writes the five quantities
// for 42 rows x 32 columns back to the LDS (a lane per (row, column), five accumulators), and the vertical pass leaves four outputs per lane ((lane / 32
// + 8 j, lane % 32), j < 4) in registers, where the map is evaluated and added to the lane's running sum (channel-major, j ascending).  Consecutive lanes
// take consecutive columns in every LDS access, so a 32-lane group of a ds_read_b32 / ds_write_b32 touches 32 different banks.  The tile's sum: a
// butterfly over each wave's 64 lanes (__shfl_xor 32, 16, .. 1), then ((w0 + w1) + w2) + w3 through the LDS -- a fixed order, no float atomics.  One fp32
// partial per (image, tile) goes to the workspace; the reduce kernel (one workgroup per image) adds an image's partials in fp64 (lane t takes tiles t, t +
// 256, ..; then a fixed tree), divides by C*H*W and rounds once to fp32.  Nothing depends on N or on the image's place in the batch.
//
// The bytes.  The uint8 kernel first copies the tile's rows of both images, all three channels, into the LDS as the 4-byte words that hold them (at most 33
// words per row: 42 pixels * 3 bytes and up to 3 bytes of misalignment), once for the three channels.  Where W % 4 == 0 and the image (and mask) pointers
// are 4-byte aligned every row starts on a word and a lane loads whole aligned words, which never reach past the row's end (VEC); otherwise a word is put
// together from four byte loads, each checked against the end of the staged range.  Both leave the same bytes in the LDS, so both give the same bits.  The
// mask: lane t adds the 4 bytes at row t / 8, columns 4 (t % 8) .. + 3 of the tile (one word, or four checked byte loads); wave and workgroup integer
// sums (exact), one uint32 partial per (image, tile) (at most 1024 * 255), added into int64 by the reduce kernel.
//
// LDS per workgroup (static): staged tiles 2 * 42 * 42 * 4 = 14 112 B, horizontal results 5 * 42 * 32 * 4 = 26 880 B, the byte words 2 * 42 * 33 * 4 =
// 11 088 B (uint8 kernel only), window and reduction slots 76 B: 52 160 B as compiled (41 072 B for fp32 input), 70 VGPRs, no scratch.  Three workgroups of the uint8 kernel fit the CU's
// 160 KiB, that is 12 waves per CU; the kernel is bound by LDS traffic and VALU work (per channel and output ~2 * 11 * 5 FMAs), not by its 6 B per pixel.
// Workspace: 8 bytes per (image, tile), fp32 partials first, then the uint32 mask partials; every slot that is read is written by the same call.
#pragma once
#include "inpaint.h"

constexpr int SSIM_T = 32;                       // outputs per tile side
constexpr int SSIM_MAX_WS = 11;                  // largest window
constexpr int SSIM_I = SSIM_T + SSIM_MAX_WS - 1;  // staged tile side with halo: 42
constexpr int SSIM_RW = 33;                      // words per staged row of bytes: ceil((42 * 3 + 3) / 4)
constexpr int SSIM_MAX_DIM = 4096;

// The little-endian word at p: one aligned load, or four byte loads of which only the first `valid` are inside the staged range (the rest read as 0).
template <bool VEC>
__device__ __forceinline__ unsigned ssim_word(const uint8_t* __restrict__ p, int valid) {
  if constexpr (VEC) {
    return *(const unsigned*)p;
  } else {
    unsigned w = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < valid) w |= (unsigned)p[j] << (8 * j);
    return w;
  }
}

template <bool U8, bool VEC>
__global__ __launch_bounds__(256) void ssim_tile_kernel(const void* __restrict__ a_, const void* __restrict__ b_, const uint8_t* __restrict__ mask,
                                                        const float* __restrict__ window, int ws, int C, int H, int W, int tiles_x, int tiles,
                                                        float* __restrict__ part, unsigned* __restrict__ mpart) {
#pragma clang fp contract(off)
  __shared__ float sa[SSIM_I * SSIM_I], sb[SSIM_I * SSIM_I], sh[5][SSIM_I * SSIM_T], sw[SSIM_MAX_WS], sred[4];
  __shared__ unsigned sraw[U8 ? 2 * SSIM_I * SSIM_RW : 1], smred[4];
  const int tid = threadIdx.x, r = ws >> 1;
  const int n = blockIdx.x / tiles, t = blockIdx.x - n * tiles, ty = t / tiles_x, tx = t - ty * tiles_x;
  const int oh = min(SSIM_T, H - ty * SSIM_T), ow = min(SSIM_T, W - tx * SSIM_T);  // the tile's outputs inside the image
  const int y0 = ty * SSIM_T - r, x0 = tx * SSIM_T - r, ih = oh + 2 * r, iw = ow + 2 * r;  // the staged rectangle, halo included
  if (tid < ws) sw[tid] = window[tid];

  if (mask) {  // wave-uniform
    const int row = tid >> 3, gy = ty * SSIM_T + row, gx = tx * SSIM_T + 4 * (tid & 7);
    unsigned m = 0;
    if (gy < H && gx < W) {
      const unsigned w4 = ssim_word<VEC>(mask + ((long)n * H + gy) * W + gx, W - gx);
      m = (w4 & 255u) + ((w4 >> 8) & 255u) + ((w4 >> 16) & 255u) + (w4 >> 24);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m += (unsigned)__shfl_xor((int)m, o, 64);
    if ((tid & 63) == 0) smred[tid >> 6] = m;
  }

  int wb0 = 0;  // the byte offset inside an image row of the first staged word
  if constexpr (U8) {
    const int gx_lo = max(x0, 0), gx_hi = min(x0 + iw, W);  // the staged columns inside the image
    wb0 = (3 * gx_lo) & ~3;
    const int end = 3 * gx_hi, nw = (end - wb0 + 3) >> 2;  // nw <= SSIM_RW
    const uint8_t *a = (const uint8_t*)a_, *b = (const uint8_t*)b_;
    for (int i = tid; i < ih * SSIM_RW; i += 256) {
      const int row = i / SSIM_RW, k = i - row * SSIM_RW, gy = y0 + row;
      if (k < nw && gy >= 0 && gy < H) {
        const long off = ((long)n * H + gy) * 3L * W + wb0 + 4 * k;
        sraw[row * SSIM_RW + k] = ssim_word<VEC>(a + off, end - (wb0 + 4 * k));
        sraw[(SSIM_I + row) * SSIM_RW + k] = ssim_word<VEC>(b + off, end - (wb0 + 4 * k));
      }
    }
  }

  float acc = 0.0f;
  for (int c = 0; c < C; ++c) {
    __syncthreads();  // the byte words are there; the previous channel's vertical pass has read sh
    for (int i = tid; i < ih * iw; i += 256) {
      const int row = i / iw, col = i - row * iw, gy = y0 + row, gx = x0 + col;
      float va = 0.0f, vb = 0.0f;  // zero padding
      if (gy >= 0 && gy < H && gx >= 0 && gx < W) {
        if constexpr (U8) {
          const int bo = 3 * gx + c - wb0;
          va = inp_unit((sraw[row * SSIM_RW + (bo >> 2)] >> (8 * (bo & 3))) & 255u);
          vb = inp_unit((sraw[(SSIM_I + row) * SSIM_RW + (bo >> 2)] >> (8 * (bo & 3))) & 255u);
        } else {
          const long off = (((long)n * C + c) * H + gy) * W + gx;
          va = ((const float*)a_)[off];
          vb = ((const float*)b_)[off];
        }
      }
      sa[row * SSIM_I + col] = va;
      sb[row * SSIM_I + col] = vb;
    }
    __syncthreads();
    for (int i = tid; i < ih * SSIM_T; i += 256) {  // horizontal pass
      const int row = i >> 5, col = i & 31;
      if (col < ow) {
        float hx = 0.0f, hy = 0.0f, hxx = 0.0f, hyy = 0.0f, hxy = 0.0f;
        for (int k = 0; k < ws; ++k) {
          const float w = sw[k], x = sa[row * SSIM_I + col + k], y = sb[row * SSIM_I + col + k];
          const float xx = x * x, yy = y * y, xy = x * y;
          hx = __builtin_fmaf(w, x, hx);
          hy = __builtin_fmaf(w, y, hy);
          hxx = __builtin_fmaf(w, xx, hxx);
          hyy = __builtin_fmaf(w, yy, hyy);
          hxy = __builtin_fmaf(w, xy, hxy);
        }
        sh[0][i] = hx, sh[1][i] = hy, sh[2][i] = hxx, sh[3][i] = hyy, sh[4][i] = hxy;
      }
    }
    __syncthreads();
    const int ox = tid & 31;
    for (int j = 0; j < 4; ++j) {  // vertical pass and the map
      const int oy = (tid >> 5) + 8 * j;
      if (oy < oh && ox < ow) {
        float v[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
        for (int k = 0; k < ws; ++k) {
          const float w = sw[k];
#pragma unroll
          for (int q = 0; q < 5; ++q) v[q] = __builtin_fmaf(w, sh[q][(oy + k) * SSIM_T + ox], v[q]);
        }
        const float C1 = 1e-4f, C2 = 9e-4f;  // (float)(0.01 ** 2), (float)(0.03 ** 2)
        const float m11 = v[0] * v[0], m22 = v[1] * v[1], m12 = v[0] * v[1];
        const float s11 = v[2] - m11, s22 = v[3] - m22, s12 = v[4] - m12;
        const float t12 = 2.0f * m12, u12 = 2.0f * s12;
        const float na = t12 + C1, nb = u12 + C2;
        const float ms = m11 + m22, ss = s11 + s22;
        const float da = ms + C1, db = ss + C2;
        const float num = na * nb, den = da * db;
        const float val = num / den;
        acc = acc + val;
      }
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) acc = acc + __shfl_xor(acc, o, 64);
  if ((tid & 63) == 0) sred[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    const float s01 = sred[0] + sred[1], s012 = s01 + sred[2];
    part[blockIdx.x] = s012 + sred[3];
    if (mask) mpart[blockIdx.x] = smred[0] + smred[1] + smred[2] + smred[3];
  }
}

// out[n] = (float)(sum of image n's tile partials in fp64 / count); mask_sum[n] = the sum of its mask partials.  A fixed order: lane t adds tiles t, t + 256,
// .. in ascending order, then a binary tree over the 256 lanes.
__global__ __launch_bounds__(256) void ssim_reduce_kernel(const float* __restrict__ part, const unsigned* __restrict__ mpart, int tiles, double count,
                                                          float* __restrict__ out, long long* __restrict__ mask_sum) {
  __shared__ double sd[256];
  __shared__ unsigned long long sm[256];
  const int tid = threadIdx.x;
  const long base = (long)blockIdx.x * tiles;
  double s = 0.0;
  unsigned long long m = 0;
  for (int i = tid; i < tiles; i += 256) {
    s += (double)part[base + i];
    if (mask_sum) m += mpart[base + i];
  }
  sd[tid] = s, sm[tid] = m;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sd[tid] += sd[tid + o], sm[tid] += sm[tid + o];
    __syncthreads();
  }
  if (tid == 0) {
    out[blockIdx.x] = (float)(sd[0] / count);
    if (mask_sum) mask_sum[blockIdx.x] = (long long)sm[0];
  }
}

static inline long ssim_tiles(int H, int W) { return (long)cdiv(H, SSIM_T) * cdiv(W, SSIM_T); }
static inline bool ssim_shape_ok(int N, int H, int W) {
  return N >= 1 && H >= 1 && W >= 1 && H <= SSIM_MAX_DIM && W <= SSIM_MAX_DIM && (long)N * ssim_tiles(H, W) <= 0x7fffffffL;
}

extern "C" size_t lfm_ssim_workspace_bytes(int N, int H, int W) {
  if (!ssim_shape_ok(N, H, W)) return 0;
  return ((size_t)N * (size_t)ssim_tiles(H, W) * 8 + 15) & ~(size_t)15;
}

// The checks both entry points share, then the two launches.  u8: uint8 NHWC (C = 3), else fp32 NCHW.
static int ssim_run(bool u8, const void* a, const void* b, const uint8_t* mask, int N, int C, int H, int W, const float* window, int window_size,
                    void* workspace, size_t workspace_bytes, float* out, long long* mask_sum, lfm_stream_t stream) {
  if (!a || !b || !window || !workspace || !out || (mask != nullptr) != (mask_sum != nullptr)) return LFM_ERR_ARG;
  if (!ssim_shape_ok(N, H, W) || C < 1 || C > 4 || window_size < 3 || window_size > SSIM_MAX_WS || !(window_size & 1)) return LFM_ERR_SHAPE;
  if (workspace_bytes < lfm_ssim_workspace_bytes(N, H, W)) return LFM_ERR_SHAPE;
  if (!inp_aligned(window, 4) || !inp_aligned(out, 4) || !inp_aligned(mask_sum, 8) || !inp_aligned(workspace, 16)) return LFM_ERR_ALIGN;
  if (!u8 && (!inp_aligned(a, 4) || !inp_aligned(b, 4))) return LFM_ERR_ALIGN;
  const int tiles = (int)ssim_tiles(H, W), tiles_x = cdiv(W, SSIM_T);
  float* part = (float*)workspace;
  unsigned* mpart = (unsigned*)workspace + (size_t)N * tiles;
  const dim3 grid((unsigned)((long)N * tiles));
  hipStream_t st = (hipStream_t)stream;
#define LFM_SSIM_TILE(U8, VEC) \
  hipLaunchKernelGGL((ssim_tile_kernel<U8, VEC>), grid, dim3(256), 0, st, a, b, mask, window, window_size, C, H, W, tiles_x, tiles, part, mpart)
  if (!u8) LFM_SSIM_TILE(false, false);
  else if (W % 4 == 0 && inp_aligned(a, 4) && inp_aligned(b, 4) && inp_aligned(mask, 4)) LFM_SSIM_TILE(true, true);
  else LFM_SSIM_TILE(true, false);
#undef LFM_SSIM_TILE
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(ssim_reduce_kernel, dim3((unsigned)N), dim3(256), 0, st, part, mpart, tiles, (double)C * H * W, out, mask_sum);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_ssim_u8(const uint8_t* a_nhwc, const uint8_t* b_nhwc, const uint8_t* mask, int N, int H, int W, const float* window, int window_size,
                           void* workspace, size_t workspace_bytes, float* out, long long* mask_sum, lfm_stream_t stream) {
  return ssim_run(true, a_nhwc, b_nhwc, mask, N, 3, H, W, window, window_size, workspace, workspace_bytes, out, mask_sum, stream);
}

extern "C" int lfm_ssim_f32(const float* a_nchw, const float* b_nchw, int N, int C, int H, int W, const float* window, int window_size, void* workspace,
                            size_t workspace_bytes, float* out, lfm_stream_t stream) {
  return ssim_run(false, a_nchw, b_nchw, nullptr, N, C, H, W, window, window_size, workspace, workspace_bytes, out, nullptr, stream);
}
