// Generic NHWC-fp16 building blocks behind the C ABI, used by the origin-ADM UNet (reference
// models/guided_diffusion/unet.py) whose layer sequence is data-dependent and therefore driven from the host side:
// implicit-GEMM 3x3 convolution (same / nearest-2x-upsampled input / stride 2), 1x1 convolution / linear with residual,
// general GroupNorm(32) with optional FiLM scale-shift and SiLU (groupnorm_dispatch.h), channel concat, small-T attention
// (unet_attention_dispatch.h), timestep embedding.
#include "../../include/lfm_hip.h"
#include "nhwc_common.h"  // ASrcConv<MODE>, EpiResidF16, EpiNCHWF32, conv_halo_allowed

static __device__ half_t g_zero_page[64];  // zero padding rows for the conv gathers (zero-initialised device global)

static const half_t* zero_page() {  // the symbol's address is per DEVICE (one slot per device, written once; racing threads write the same value)
  static std::atomic<const half_t*> p[64];
  const int dev = lfm_device_index();
  const half_t* v = p[dev].load(std::memory_order_acquire);
  if (!v) {
    void* d = nullptr;
    if (hipGetSymbolAddress(&d, HIP_SYMBOL(g_zero_page)) != hipSuccess) return nullptr;
    v = (const half_t*)d;
    p[dev].store(v, std::memory_order_release);
  }
  return v;
}

// Low-resolution levels of a UNet are small-M, huge-K problems (celeb512 at batch 32: 4x4 maps = 512 rows x 1024 columns x K 9216..18432):
// 32 tiles of 128x128 on 256 CUs, hundreds of K-tiles in sequence.  With a caller-provided workspace the K range is sliced over
// blockIdx.y (fp32 slabs, summed in a fixed order by a finish kernel that applies the real epilogue -- deterministic), as for the
// batch-1 DiT GEMMs.  workspace may be NULL (no split-K).
#define CONV_SPLITK_MAX_TILES 256  // 16x16 maps at batch 32 x 512 channels = 256 tiles of 128x128: two slices = two workgroups per CU
#define CONV_SPLITK_MAX_WG 512
extern "C" size_t lfm_conv3x3_workspace_bytes(int N, int H, int W, int Cin, int Cout) {
  const long M = (long)N * H * W;
  if (M <= 0 || Cout <= 0 || Cin <= 0) return 0;
  const long tiles = (long)cdiv(M, 128) * cdiv(Cout, 128);
  const int s256 = M < (1L << 30) ? splitk256_slices((int)M, Cout, 9 * Cin, (size_t)-1) : 0;  // slices on the 256x256 kernel (gemm_kernel.h), if the shape takes it
  int s = 1;
  if (tiles <= CONV_SPLITK_MAX_TILES)
    while (tiles * (s * 2) <= CONV_SPLITK_MAX_WG && (9L * Cin) / (s * 2) >= 128 && ((9L * Cin) / (s * 2)) % 64 == 0) s *= 2;
  if (s256 > s) s = s256;
  return s < 2 ? 0 : (size_t)s * M * Cout * 4;
}

template <int MODE>
static int conv3x3_mode(const half_t* xi, const half_t* z, const half_t* wi, const EpiResidF16& epi, int H, int W, int Cin, int Cout, int M, float* ws,
                        size_t ws_bytes, hipStream_t st) {
  ASrcConv<MODE> a{xi, z, H, W, Cin, M};
  const int rc = launch_gemm_splitk_src(a, wi, 9L * Cin, M, Cout, 9 * Cin, epi, ws, ws_bytes, st, CONV_SPLITK_MAX_TILES, CONV_SPLITK_MAX_WG);
  if (rc != 1) return rc;
  return launch_gemm_auto(a, wi, 9L * Cin, M, Cout, 9 * Cin, epi, st);
}

static int conv3x3_f16_impl(const void* in, const void* w, const float* bias, const void* resid, float scale, void* out, int N, int H, int W, int Cin,
                            int Cout, int mode, void* workspace, size_t workspace_bytes, lfm_stream_t stream) {
  if (!in || !w || !out) return LFM_ERR_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || Cin % 64 || Cout % 4 || mode < 0 || mode > 2) return LFM_ERR_SHAPE;
  if (mode == 1 && ((H | W) & 1)) return LFM_ERR_SHAPE;
  if (workspace && ((uintptr_t)workspace & 15)) return LFM_ERR_ALIGN;
  const half_t* z = zero_page();
  if (!z) return LFM_ERR_LAUNCH;
  const int M = N * H * W;
  EpiResidF16 epi{(half_t*)out, Cout, bias, (const half_t*)resid, scale};
  hipStream_t st = (hipStream_t)stream;
  const half_t* wi = (const half_t*)w;
  const half_t* xi = (const half_t*)in;
  float* ws = (float*)workspace;
  // plain and upsample-fused 3x3 convolutions on 16-aligned maps that fill the chip: the halo-tiled direct kernel (conv_halo_kernel.h);
  // CONV_IMPLICIT_GEMM: the implicit GEMM instead (A/B and parity tests)
  if (mode != 2 && conv_halo_allowed(out, resid)) {
    const int rc = mode == 1 ? launch_conv3x3_halo<1>(xi, z, wi, N, H, W, Cin, Cout, epi, st) : launch_conv3x3_halo<0>(xi, z, wi, N, H, W, Cin, Cout, epi, st);
    if (rc != 1) return rc;
  }
  if (mode == 0) return conv3x3_mode<0>(xi, z, wi, epi, H, W, Cin, Cout, M, ws, workspace_bytes, st);
  if (mode == 1) return conv3x3_mode<1>(xi, z, wi, epi, H, W, Cin, Cout, M, ws, workspace_bytes, st);
  return conv3x3_mode<2>(xi, z, wi, epi, H, W, Cin, Cout, M, ws, workspace_bytes, st);
}

extern "C" int lfm_conv3x3_f16_ws(const void* in, const void* w, const float* bias, const void* resid, void* out, int N, int H, int W, int Cin,
                                  int Cout, int mode, void* workspace, size_t workspace_bytes, lfm_stream_t stream) {
  return conv3x3_f16_impl(in, w, bias, resid, 1.0f, out, N, H, W, Cin, Cout, mode, workspace, workspace_bytes, stream);
}
// out = (conv + bias (+ resid)) * scale: the residual epilogue of EDM's UNetBlock with skip_scale = sqrt(0.5) (SongUNet, models/EDM.py:272-274).  The scale
// rides in the epilogue struct, so the halo kernel, the implicit GEMM and the split-K finish kernel all apply it to the fp32 sum before the fp16 store.
extern "C" int lfm_conv3x3_scaled_f16_ws(const void* in, const void* w, const float* bias, const void* resid, float scale, void* out, int N, int H, int W,
                                         int Cin, int Cout, int mode, void* workspace, size_t workspace_bytes, lfm_stream_t stream) {
  return conv3x3_f16_impl(in, w, bias, resid, scale, out, N, H, W, Cin, Cout, mode, workspace, workspace_bytes, stream);
}

// Which path lfm_conv3x3_f16_ws takes for this shape with 16-byte-aligned operands and a workspace of `workspace_bytes`: the same questions in the same order
extern "C" int lfm_conv3x3_plan(int N, int H, int W, int Cin, int Cout, int mode, size_t workspace_bytes) {
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin % 64 || Cout <= 0 || Cout % 4 || mode < 0 || mode > 2) return LFM_ERR_SHAPE;
  if (mode == 1 && ((H | W) & 1)) return LFM_ERR_SHAPE;
  if (mode != 2 && conv_halo_allowed() && conv3x3_halo_takes(N, H, W, Cin, Cout)) return 1;
  const int M = N * H * W, K = 9 * Cin;
  if (workspace_bytes && lfm_gemm_selected_v1_ok() != 0 &&
      (splitk256_slices(M, Cout, K, workspace_bytes) || splitk_slices(M, Cout, K, workspace_bytes, CONV_SPLITK_MAX_TILES, CONV_SPLITK_MAX_WG) >= 2))
    return 2;
  return 3;
}

extern "C" int lfm_conv3x3_f16(const void* in, const void* w, const float* bias, const void* resid, void* out, int N, int H, int W, int Cin,
                               int Cout, int mode, lfm_stream_t stream) {
  return lfm_conv3x3_f16_ws(in, w, bias, resid, out, N, H, W, Cin, Cout, mode, nullptr, 0, stream);
}

extern "C" int lfm_conv3x3_out_f32(const void* in, const void* w4, const float* bias4, float* out_nchw, int N, int H, int W, int Cin, int nch,
                                   lfm_stream_t stream) {
  if (!in || !w4 || !bias4 || !out_nchw) return LFM_ERR_ARG;
  if (N <= 0 || Cin % 64 || nch < 1 || nch > 4) return LFM_ERR_SHAPE;
  const half_t* z = zero_page();
  if (!z) return LFM_ERR_LAUNCH;
  return launch_conv3x3_out((const half_t*)in, z, (const half_t*)w4, N, H, W, Cin, EpiNCHWF32{out_nchw, bias4, H * W, nch}, (hipStream_t)stream);
}

static int linear_f16_impl(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias, const void* resid,
                           float scale, lfm_stream_t stream) {
  if (!A || !W || !C) return LFM_ERR_ARG;
  // 16-byte operand chunks; the epilogue stores (and reads the residual) four columns at a time at m * ldc + n
  if ((lda % 8) || (ldw % 8) || (ldc % 4) || (((uintptr_t)A | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  return launch_gemm_auto(ASrcRowMajor{(const half_t*)A, lda, M, 0}, (const half_t*)W, ldw, M, N, K,
                          EpiResidF16{(half_t*)C, ldc, bias, (const half_t*)resid, scale}, (hipStream_t)stream);
}
extern "C" int lfm_linear_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                              const void* resid, lfm_stream_t stream) {
  return linear_f16_impl(A, lda, W, ldw, C, ldc, M, N, K, bias, resid, 1.0f, stream);
}
// C = (A W^T + bias (+ resid)) * scale: the attention projection of EDM's UNetBlock with skip_scale != 1 (models/EDM.py:290-291) and its 1x1 skip
extern "C" int lfm_linear_scaled_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                                     const void* resid, float scale, lfm_stream_t stream) {
  return linear_f16_impl(A, lda, W, ldw, C, ldc, M, N, K, bias, resid, scale, stream);
}

// C = [A1 | A2] W^T + bias (+ resid): the 1x1 skip convolution of a ResBlock whose input is the channel concat of two tensors (unet.py:649 + :236),
// read in place: the K range [0, K1) comes from A1 [M, K1], [K1, K1 + K2) from A2 [M, K2].  K1 % 64 == 0 (a K-tile never straddles the seam).
static int linear2_f16_impl(const void* A1, int K1, const void* A2, int K2, const void* W, long ldw, void* C, long ldc, int M, int N, const float* bias,
                            const void* resid, float scale, lfm_stream_t stream) {
  if (!A1 || !A2 || !W || !C) return LFM_ERR_ARG;
  if (K1 <= 0 || K2 <= 0 || (K1 % 64) || (K2 % 8)) return LFM_ERR_SHAPE;
  if ((ldw % 8) || (ldc % 4) || (((uintptr_t)A1 | (uintptr_t)A2 | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  return launch_gemm_auto(ASrcRowMajor2{(const half_t*)A1, (const half_t*)A2, K1, K2, M, 0}, (const half_t*)W, ldw, M, N, K1 + K2,
                          EpiResidF16{(half_t*)C, ldc, bias, (const half_t*)resid, scale}, (hipStream_t)stream);
}
extern "C" int lfm_linear2_f16(const void* A1, int K1, const void* A2, int K2, const void* W, long ldw, void* C, long ldc, int M, int N,
                               const float* bias, const void* resid, lfm_stream_t stream) {
  return linear2_f16_impl(A1, K1, A2, K2, W, ldw, C, ldc, M, N, bias, resid, 1.0f, stream);
}
extern "C" int lfm_linear2_scaled_f16(const void* A1, int K1, const void* A2, int K2, const void* W, long ldw, void* C, long ldc, int M, int N,
                                      const float* bias, const void* resid, float scale, lfm_stream_t stream) {
  return linear2_f16_impl(A1, K1, A2, K2, W, ldw, C, ldc, M, N, bias, resid, scale, stream);
}

// ------------------------------------------------------------------ the linears of EDM's TransformerBlock (models/EDM.py:427-483, `adm_context`)
// C = (A W^T + bias (+ resid) (+ vec[m / tokens])) * scale: attn1.proj with both residual sums of the block's first two lines in one epilogue (EpiResidVecF16)
extern "C" int lfm_linear_resid_vec_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                                        const void* resid, const float* vec, long vec_stride, int tokens, float scale, lfm_stream_t stream) {
  if (!A || !W || !C) return LFM_ERR_ARG;
  if ((lda % 8) || (ldw % 8) || (ldc % 4) || (((uintptr_t)A | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  if (vec && ((vec_stride % 4) || ((uintptr_t)vec & 15))) return LFM_ERR_ALIGN;  // four columns of a row of `vec` are one 16-byte load
  if (tokens <= 0 || M <= 0 || (M % tokens)) return LFM_ERR_SHAPE;
  return launch_gemm_auto(ASrcRowMajor{(const half_t*)A, lda, M, 0}, (const half_t*)W, ldw, M, N, K,
                          EpiResidVecF16{EpiResidF16{(half_t*)C, ldc, bias, (const half_t*)resid, scale}, vec, vec_stride, tokens}, (hipStream_t)stream);
}
// C = silu(A W^T + bias): ff.layer0; SiLU in fp32 on the accumulator, one rounding to fp16
extern "C" int lfm_linear_silu_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                                   lfm_stream_t stream) {
  if (!A || !W || !C || !bias) return LFM_ERR_ARG;
  if ((lda % 8) || (ldw % 8) || (ldc % 4) || (((uintptr_t)A | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  return launch_gemm_auto(ASrcRowMajor{(const half_t*)A, lda, M, 0}, (const half_t*)W, ldw, M, N, K, EpiBiasSiluF16{{(half_t*)C, ldc, bias}},
                          (hipStream_t)stream);
}
// C = gelu_erf(A W^T + bias): net.0 of the layout encoder's FeedForward (nn.Linear + nn.GELU(), the exact form); in fp32 on the accumulator, one rounding to fp16
extern "C" int lfm_linear_gelu_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                                   lfm_stream_t stream) {
  if (!A || !W || !C || !bias) return LFM_ERR_ARG;
  if ((lda % 8) || (ldw % 8) || (ldc % 4) || (((uintptr_t)A | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  return launch_gemm_auto(ASrcRowMajor{(const half_t*)A, lda, M, 0}, (const half_t*)W, ldw, M, N, K, EpiBiasGeluErfF16{{(half_t*)C, ldc, bias}},
                          (hipStream_t)stream);
}

// out[r][0 .. cols) = table[y[r]][0 .. cols): the rows of the stacked context table (one per TransformerBlock, column-wise) that this batch's labels name.
// Plain 16-byte loads and stores, no host readback: safe under capture, and a replay follows labels rewritten in place.  A label outside [0, rows) is
// the host's to refuse (hip.check_labels, before anything is enqueued); a replay cannot ask, so the kernel clamps instead of reading beyond the table.
__global__ void gather_rows_f32_kernel(const f32x4* __restrict__ table, int rows, int cols4, const long long* __restrict__ y, f32x4* __restrict__ out,
                                       long out_stride4, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const long r = i / cols4;
  const int c = (int)(i - r * cols4);
  long long l = y[r];
  l = l < 0 ? 0 : (l >= rows ? rows - 1 : l);
  out[r * out_stride4 + c] = table[l * cols4 + c];
}
extern "C" int lfm_gather_rows_f32(const float* table, int rows, int cols, const void* y_int64, int N, float* out, long out_stride, lfm_stream_t stream) {
  if (!table || !y_int64 || !out) return LFM_ERR_ARG;
  if (rows <= 0 || cols <= 0 || N <= 0 || (cols % 4) || out_stride < cols) return LFM_ERR_SHAPE;
  if ((out_stride % 4) || (((uintptr_t)table | (uintptr_t)out) & 15) || ((uintptr_t)y_int64 & 7)) return LFM_ERR_ALIGN;
  const long total = (long)N * (cols / 4);
  hipLaunchKernelGGL(gather_rows_f32_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const f32x4*)table, rows, cols / 4,
                     (const long long*)y_int64, (f32x4*)out, out_stride / 4, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ first conv: fp32 NCHW (Cin <= 16) -> fp16 NHWC
// Weights are transposed into LDS as [k = (c,ky,kx)][Cout] so the 8 output channels of a thread are two float4 reads per tap;
// a block walks CI_PIX pixels (threads = Cout/8 channel-octets x pixel rows), input taps are L1-served broadcast loads.
// blockIdx.y: the slice [blockIdx.y Cs, + Cs) of the output channels (Cs % 8 == 0) -- one slice, unless the weights of all of them exceed the LDS
// (Cin 16 with Cout 320: 180 KiB).
#define CI_PIX 256
__global__ __launch_bounds__(256) void conv_in_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                      half_t* __restrict__ out, int N, int H, int W, int Cin, int Cout, int Cs) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // [Cin*9][Cl]
  const int KK = Cin * 9, cs0 = blockIdx.y * Cs, Cl = Cout - cs0 < Cs ? Cout - cs0 : Cs, c8n = Cl / 8;
  w += (long)cs0 * KK;
  b += cs0;
  out += cs0;
  for (int e = threadIdx.x; e < KK * Cl; e += 256) {
    const int co = e / KK, k = e - co * KK;  // w is [Cout][Cin][3][3] = [Cout][KK]
    wl[k * Cl + co] = w[e];
  }
  __syncthreads();
  const int oct = threadIdx.x % c8n, prow = threadIdx.x / c8n, rows = 256 / c8n;
  if (prow >= rows) return;
  const int co = oct * 8;
  const long total = (long)N * H * W;
  const long p0 = (long)blockIdx.x * CI_PIX;
  for (long pix = p0 + prow; pix < p0 + CI_PIX && pix < total; pix += rows) {
    const int xx = (int)(pix % W), yy = (int)((pix / W) % H), n = (int)(pix / ((long)H * W));
    f32x4 a0 = *(const f32x4*)(b + co), a1 = *(const f32x4*)(b + co + 4);
    for (int c = 0; c < Cin; ++c)
#pragma unroll
      for (int t = 0; t < 9; ++t) {
        const int iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
        if ((unsigned)iy >= (unsigned)H || (unsigned)ix >= (unsigned)W) continue;
        const float v = x[(((long)n * Cin + c) * H + iy) * W + ix];
        const float* wr = wl + (c * 9 + t) * Cl + co;
        a0 += v * *(const f32x4*)wr;
        a1 += v * *(const f32x4*)(wr + 4);
      }
    half8_t h = {(half_t)a0.x, (half_t)a0.y, (half_t)a0.z, (half_t)a0.w, (half_t)a1.x, (half_t)a1.y, (half_t)a1.z, (half_t)a1.w};
    *(half8_t*)(out + pix * Cout + co) = h;
  }
}

// The same on the matrix cores (Cout % 64 == 0): the scalar kernel above runs at 16 TFLOP/s and had become 1.5 % of a celeb512 UNet evaluation.
// A workgroup walks chunks of 64 pixels: its 256 threads gather the im2col rows (k = c * 9 + tap, zero beyond the border and beyond Cin * 9) once into
// the LDS, split hi / lo into two fp16 planes (x = hi + lo to 2^-22: three MFMAs -- w_hi x_hi + w_hi x_lo + w_lo x_hi -- are the fp32 dot product to
// ~2^-21, the fp32 arithmetic of the scalar kernel and of the reference's conv at TF32-or-better); the fp32 weights are split the same way once per
// workgroup.  Wave w owns output channels [w Cout / 4, (w + 1) Cout / 4): D[channel][pixel] on v_mfma_f32_16x16x16_f16 with the weights as the A
// operand, so a lane ends up with four consecutive channels of one pixel: 8-byte NHWC stores.  Bound: the fp16 output write.
#define CIM_PIX 64
template <int NT>  // 16-channel tiles per wave = Cout / 64
__global__ __launch_bounds__(256) void conv_in_mfma_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                           half_t* __restrict__ out, int N, int H, int W, int Cin, int Cout, int KS) {
  extern __shared__ __attribute__((aligned(16))) char smraw[];
  const int Kp = KS * 16, LD = Kp + 8, KK = Cin * 9;  // LDS row stride (halves): + 8 keeps 16 consecutive rows on distinct banks for the 8-byte reads
  half_t* wh = (half_t*)smraw;                  // [Cout][LD]
  half_t* wl = wh + (size_t)Cout * LD;
  half_t* xh = wl + (size_t)Cout * LD;          // [CIM_PIX][LD]
  half_t* xl = xh + CIM_PIX * LD;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 15, q = lane >> 4;
  for (int e = tid; e < Cout * Kp; e += 256) {
    const int co = e / Kp, k = e - co * Kp;
    const float v = k < KK ? w[(long)co * KK + k] : 0.f;
    const half_t h = (half_t)v;
    wh[co * LD + k] = h;
    wl[co * LD + k] = (half_t)(v - (float)h);
  }
  const long total = (long)N * H * W;
  const int c0 = wave * NT * 16;
  f32x4 bias4[NT];
#pragma unroll
  for (int nt = 0; nt < NT; ++nt) bias4[nt] = *(const f32x4*)(b + c0 + nt * 16 + q * 4);
  for (long p0 = (long)blockIdx.x * CIM_PIX; p0 < total; p0 += (long)gridDim.x * CIM_PIX) {
    __syncthreads();  // the previous chunk's fragment reads are done (and, first time round, the weights are in place)
    {
      const long pix = p0 + (tid & 63);
      const bool live = pix < total;
      const int xx = live ? (int)(pix % W) : 0, yy = live ? (int)((pix / W) % H) : 0, n = live ? (int)(pix / ((long)H * W)) : 0;
      for (int k = tid >> 6; k < Kp; k += 4) {
        float v = 0.f;
        if (live && k < KK) {
          const int c = k / 9, t = k - c * 9, iy = yy + t / 3 - 1, ix = xx + t % 3 - 1;
          if ((unsigned)iy < (unsigned)H && (unsigned)ix < (unsigned)W) v = x[(((long)n * Cin + c) * H + iy) * W + ix];
        }
        const half_t h = (half_t)v;
        xh[(tid & 63) * LD + k] = h;
        xl[(tid & 63) * LD + k] = (half_t)(v - (float)h);
      }
    }
    __syncthreads();
#pragma unroll
    for (int pt = 0; pt < CIM_PIX / 16; ++pt) {
      f32x4 acc[NT];
#pragma unroll
      for (int nt = 0; nt < NT; ++nt) acc[nt] = bias4[nt];
      for (int s = 0; s < KS; ++s) {
        const half4_t bh = *(const half4_t*)(xh + (pt * 16 + r) * LD + s * 16 + q * 4), bl = *(const half4_t*)(xl + (pt * 16 + r) * LD + s * 16 + q * 4);
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
          const half4_t ah = *(const half4_t*)(wh + (c0 + nt * 16 + r) * LD + s * 16 + q * 4), al = *(const half4_t*)(wl + (c0 + nt * 16 + r) * LD + s * 16 + q * 4);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, bh, acc[nt], 0, 0, 0);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x16f16(ah, bl, acc[nt], 0, 0, 0);
          acc[nt] = __builtin_amdgcn_mfma_f32_16x16x16f16(al, bh, acc[nt], 0, 0, 0);
        }
      }
      const long pix = p0 + pt * 16 + r;  // lane holds channels c0 + 16 nt + 4 q .. + 3 of this pixel
      if (pix < total) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
          *(half4_t*)(out + pix * Cout + c0 + nt * 16 + q * 4) = (half4_t){(half_t)acc[nt].x, (half_t)acc[nt].y, (half_t)acc[nt].z, (half_t)acc[nt].w};
      }
    }
  }
}

template <int NT>
static int launch_conv_in_mfma(const float* x, const float* w, const float* b, half_t* out, int N, int H, int W, int Cin, int Cout, hipStream_t st) {
  const int KS = cdiv(Cin * 9, 16), LD = KS * 16 + 8;
  const size_t lds = ((size_t)2 * Cout + 2 * CIM_PIX) * LD * 2;
  if (lds > 160 * 1024) return 1;
  if (!lfm_kernel_lds<&conv_in_mfma_kernel<NT>>(160 * 1024)) return LFM_ERR_LAUNCH;
  const long chunks = cdiv((long)N * H * W, CIM_PIX);
  const int grid = (int)(chunks < 1024 ? chunks : 1024);  // a workgroup pays the weight split once and then walks its chunks
  hipLaunchKernelGGL(conv_in_mfma_kernel<NT>, dim3(grid), dim3(256), lds, st, x, w, b, out, N, H, W, Cin, Cout, KS);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_conv3x3_in_f32(const float* x_nchw, const float* w, const float* bias, void* out_nhwc, int N, int H, int W, int Cin,
                                  int Cout, lfm_stream_t stream) {
  if (!x_nchw || !w || !bias || !out_nhwc) return LFM_ERR_ARG;
  if (N <= 0 || H <= 0 || W <= 0 || Cin <= 0 || Cin > 16 || Cout <= 0 || Cout % 8 || Cout / 8 > 256) return LFM_ERR_SHAPE;
  if ((Cout == 64 || Cout == 128 || Cout == 192 || Cout == 256) && !((uintptr_t)out_nhwc & 7) && !((uintptr_t)bias & 15) &&
      !(lfm_gemm_debug_flags() & LFM_DBG_UNET_CONV_IN_SCALAR)) {  // flag: the scalar kernel (A/B)
    int rc;
    if (Cout == 64) rc = launch_conv_in_mfma<1>(x_nchw, w, bias, (half_t*)out_nhwc, N, H, W, Cin, Cout, (hipStream_t)stream);
    else if (Cout == 128) rc = launch_conv_in_mfma<2>(x_nchw, w, bias, (half_t*)out_nhwc, N, H, W, Cin, Cout, (hipStream_t)stream);
    else if (Cout == 192) rc = launch_conv_in_mfma<3>(x_nchw, w, bias, (half_t*)out_nhwc, N, H, W, Cin, Cout, (hipStream_t)stream);
    else rc = launch_conv_in_mfma<4>(x_nchw, w, bias, (half_t*)out_nhwc, N, H, W, Cin, Cout, (hipStream_t)stream);
    if (rc != 1) return rc;
  }
  if (((uintptr_t)out_nhwc | (uintptr_t)bias) & 15) return LFM_ERR_ALIGN;  // the scalar kernel: 16-byte stores of eight channels, 16-byte bias loads
  // output channels per slice: all of them, or the fewest equal slices of whole octets whose weights fit the LDS (Cin <= 16: 8 channels are 4.5 KiB at most)
  const int fit = (int)(160 * 1024 / ((size_t)Cin * 9 * 4)) & ~7, slices = cdiv(Cout, fit), Cs = cdiv(cdiv(Cout, slices), 8) * 8;
  const size_t lds = (size_t)Cin * 9 * Cs * 4;
  if (!lfm_kernel_lds<&conv_in_kernel>(160 * 1024)) return LFM_ERR_LAUNCH;
  hipLaunchKernelGGL(conv_in_kernel, dim3(cdiv((long)N * H * W, CI_PIX), slices), dim3(256), lds, (hipStream_t)stream, x_nchw, w, bias,
                     (half_t*)out_nhwc, N, H, W, Cin, Cout, Cs);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ general GroupNorm(32 groups) on NHWC fp16: lfm_groupnorm_f16, lfm_groupnorm2_f16, lfm_groupnorm_plan
#include "groupnorm_dispatch.h"

// ------------------------------------------------------------------ 2x2 average pooling, stride 2 (EDM Conv2d(down=True) with
// resample_filter [1,1]: conv2d with the 2x2 box filter / 4, models/EDM.py:96-98,122-125)
__global__ void avgpool2_kernel(const half8_t* __restrict__ x, half8_t* __restrict__ y, int Ho, int Wo, int C8, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C8);
  const long p = i / C8;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const long n = p / ((long)Wo * Ho);
  const long Wi = 2L * Wo;
  const half8_t* b = x + ((n * 2 * Ho + 2 * oy) * Wi + 2 * ox) * C8 + c;
  const half8_t a0 = b[0], a1 = b[C8], a2 = b[Wi * C8], a3 = b[Wi * C8 + C8];
  half8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)(0.25f * ((float)a0[j] + (float)a1[j] + (float)a2[j] + (float)a3[j]));
  y[i] = o;
}
extern "C" int lfm_avgpool2_f16(const void* x, void* y, int N, int Ho, int Wo, int C, lfm_stream_t stream) {
  if (!x || !y) return LFM_ERR_ARG;
  if (N <= 0 || Ho <= 0 || Wo <= 0 || C % 8) return LFM_ERR_SHAPE;
  const long total = (long)N * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(avgpool2_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const half8_t*)x, (half8_t*)y, Ho, Wo, C / 8, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ nearest-neighbour 2x upsample (EDM Conv2d(up=True, kernel=0) skip path:
// conv_transpose2d with the all-ones 2x2 filter, models/EDM.py:117-121)
__global__ void upsample2_kernel(const half8_t* __restrict__ x, half8_t* __restrict__ y, int Ho, int Wo, int C8, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C8);
  const long p = i / C8;
  const int ox = (int)(p % Wo), oy = (int)((p / Wo) % Ho);
  const long n = p / ((long)Wo * Ho);
  y[i] = x[((n * (Ho / 2) + oy / 2) * (Wo / 2) + ox / 2) * C8 + c];
}
extern "C" int lfm_upsample2_f16(const void* x, void* y, int N, int Ho, int Wo, int C, lfm_stream_t stream) {
  if (!x || !y) return LFM_ERR_ARG;
  if (N <= 0 || Ho <= 0 || Wo <= 0 || ((Ho | Wo) & 1) || C % 8) return LFM_ERR_SHAPE;
  const long total = (long)N * Ho * Wo * (C / 8);
  hipLaunchKernelGGL(upsample2_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const half8_t*)x, (half8_t*)y, Ho, Wo, C / 8, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ [1,3,3,1] FIR resampling and the zero-border copy (EDM Conv2d with the NCSN++ filter,
// models/EDM.py:96-132): lfm_fir_down2_f16, lfm_fir_up2_f16, lfm_zero_border_f16, lfm_zero_border_f32
#include "fir_resample.h"

// ------------------------------------------------------------------ h + emb_out[..., None, None] (ResBlock without scale-shift norm, unet.py:233-235)
__global__ void add_image_vec_kernel(const half8_t* __restrict__ x, const float* __restrict__ e, long e_stride, half8_t* __restrict__ y, int HW,
                                     int C8, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int c = (int)(i % C8);
  const long n = i / ((long)C8 * HW);
  const half8_t v = x[i];
  const float* ev = e + n * e_stride + c * 8;
  half8_t o;
#pragma unroll
  for (int j = 0; j < 8; ++j) o[j] = (half_t)((float)v[j] + ev[j]);
  y[i] = o;
}
extern "C" int lfm_add_image_vec_f16(const void* x, const float* e, long e_stride, void* y, int N, int HW, int C, lfm_stream_t stream) {
  if (!x || !e || !y) return LFM_ERR_ARG;
  if (N <= 0 || HW <= 0 || C % 8) return LFM_ERR_SHAPE;
  const long total = (long)N * HW * (C / 8);
  hipLaunchKernelGGL(add_image_vec_kernel, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, (const half8_t*)x, e, e_stride, (half8_t*)y, HW,
                     C / 8, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ channel concat (th.cat([h, skip], dim=1), unet.py:649)
__global__ void concat_c_kernel(const half8_t* __restrict__ a, const half8_t* __restrict__ b, half8_t* __restrict__ o, long pixels, int Ca8, int Cb8) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  const int Co8 = Ca8 + Cb8;
  if (i >= pixels * Co8) return;
  const long p = i / Co8;
  const int c = (int)(i - p * Co8);
  o[i] = c < Ca8 ? a[p * Ca8 + c] : b[p * Cb8 + (c - Ca8)];
}
extern "C" int lfm_concat_channels_f16(const void* a, const void* b, void* out, long pixels, int Ca, int Cb, lfm_stream_t stream) {
  if (!a || !b || !out) return LFM_ERR_ARG;
  if (Ca % 8 || Cb % 8 || pixels <= 0) return LFM_ERR_SHAPE;
  hipLaunchKernelGGL(concat_c_kernel, dim3(cdiv(pixels * ((Ca + Cb) / 8), 256)), dim3(256), 0, (hipStream_t)stream, (const half8_t*)a,
                     (const half8_t*)b, (half8_t*)out, pixels, Ca / 8, Cb / 8);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ attention (QKVAttentionLegacy, unet.py:310-334): lfm_attention_small_f16, lfm_unet_attention_plan
#include "unet_attention_dispatch.h"

// ------------------------------------------------------------------ SpatialTransformer (attention.py:85-280): lfm_cross_attention_f16, lfm_cross_attention_plan;
// lfm_layernorm_f16, lfm_geglu_f16
#include "unet_cross_attention_kernel.h"
#include "token_ops.h"

// ------------------------------------------------------------------ label-map conditioning of mask-to-image synthesis (encoder.py:90-112): lfm_label_rescale_f32
#include "label_rescale.h"

// ------------------------------------------------------------------ the sample writers' JPEGs, byte-identical to PIL.Image.save: lfm_jpeg_encode_rgb8,
// lfm_jpeg_encode_workspace_bytes
#include "jpeg_encode.h"

// ------------------------------------------------------------------ inpainting's elementwise stages from the image and mask bytes (test_flow_latent_inpainting.py
// :36-55, :147-150, :157-160): lfm_inpaint_prepare_u8, lfm_inpaint_cond_f32, lfm_inpaint_composite_u8
#include "inpaint.h"

// ------------------------------------------------------------------ the inpainting evaluator's SSIM per image and the masks' byte sums (losses/ssim.py :36-67):
// lfm_ssim_u8, lfm_ssim_f32, lfm_ssim_workspace_bytes
#include "ssim.h"

// ------------------------------------------------------------------ timestep embedding MLP (nn.py:103-121 + unet.py:633-641)
// emb[r] = W2 silu(W0 [cos(t f) | sin(t f)] + b0) + b2 (+ label_emb[y[r]]);  also emits fp16 silu(emb) for the ResBlock emb_layers
__global__ __launch_bounds__(256) void time_embed1_kernel(const float* __restrict__ t, int t_len, const float* __restrict__ w0,
                                                          const float* __restrict__ b0, float* __restrict__ h1, int F, int E) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= E) return;
  const float tv = t[t_len == 1 ? 0 : r];
  const int half = F / 2;
  const float* w = w0 + (long)j * F;
  float s = 0.f;
  for (int k = lane; k < 2 * half; k += 64) {
    const int i = k < half ? k : k - half;
    const float a = tv * expf(-9.210340371976184f * (float)i / (float)half);
    s += w[k] * (k < half ? cosf(a) : sinf(a));
  }
  s = wave_sum(s);
  if (lane == 0) h1[(long)r * E + j] = silu_f(s + b0[j]);
}
__global__ __launch_bounds__(256) void time_embed2_kernel(const float* __restrict__ h1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                          const float* __restrict__ label_table, const int64_t* __restrict__ y,
                                                          int label_rows, float* __restrict__ emb, half_t* __restrict__ emb_silu, int E) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= E) return;
  const float* w = w2 + (long)j * E;
  const float* h = h1 + (long)r * E;
  float s = 0.f;
  for (int k = lane; k < E; k += 64) s += w[k] * h[k];
  s = wave_sum(s);
  if (lane == 0) {
    float v = s + b2[j];
    if (label_table) {  // out-of-range label: nn.Embedding raises in the reference; poison instead of reading out of bounds
      const long yr = (long)y[r];
      v = (yr >= 0 && yr < label_rows) ? v + label_table[yr * E + j] : __builtin_nanf("");
    }
    emb[(long)r * E + j] = v;
    emb_silu[(long)r * E + j] = (half_t)silu_f(v);
  }
}

extern "C" int lfm_time_embed(const float* t, int t_len, const float* w0, const float* b0, const float* w2, const float* b2,
                              const float* label_table, const int64_t* y, int label_rows, float* scratch_h1, float* emb, void* emb_silu_f16, int N, int F,
                              int E, lfm_stream_t stream) {
  if (!t || !w0 || !b0 || !w2 || !b2 || !scratch_h1 || !emb || !emb_silu_f16) return LFM_ERR_ARG;
  if ((label_table != nullptr) != (y != nullptr)) return LFM_ERR_ARG;
  if (label_table && label_rows <= 0) return LFM_ERR_SHAPE;
  if (N <= 0 || F <= 0 || (F & 1) || E <= 0 || (t_len != 1 && t_len != N)) return LFM_ERR_SHAPE;
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(time_embed1_kernel, dim3(cdiv(E, 4), N), dim3(256), 0, st, t, t_len, w0, b0, scratch_h1, F, E);
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(time_embed2_kernel, dim3(cdiv(E, 4), N), dim3(256), 0, st, scratch_h1, w2, b2, label_table, y, label_rows, emb, (half_t*)emb_silu_f16, E);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ------------------------------------------------------------------ DDPM++ mapping network (SongUNet, models/EDM.py:663-675 + PositionalEmbedding :490-505)
// in[k]  = pe[k] (+ sqrt(L) W_label[:, y][k] + b_label[k]),  pe = [sin(t f) | cos(t f)],  f_i = 10000^(-i / (F / 2 - 1))   (endpoint = True; the reference
//          computes [cos | sin] and flips the halves);  emb = silu(W1 silu(W0 in + b0) + b1): fp32 and its fp16 copy, which the blocks' `affine` GEMM reads
//          as it is (already SiLU'd).  All fp32.  label_table is W_label^T [label_rows][F]; a label outside [0, label_rows) poisons its row with NaN.
// N x E values per evaluation: the correctly-rounded exp and a true division (silu_f's v_exp_f32 / v_rcp_f32 are ~2 ulp each, and this network has two
// SiLUs in sequence where lfm_time_embed has one)
__device__ __forceinline__ float silu_exact_f(float x) { return x / (1.0f + expf(-x)); }
// FOURIER (NCSN++, FourierEmbedding models/EDM.py:512-522): the argument is t * (fl32(2 pi) * freqs[i]) with the reference's two fp32 roundings -- the table
// in fp32 first, then the product with t -- instead of t * f_i; freqs ~ 16 N(0, 1), so the arguments reach several hundred radians: sinf / cosf reduce the
// full range (the fast intrinsics do not)
template <bool FOURIER>
__global__ __launch_bounds__(256) void song_embed1_kernel(const float* __restrict__ t, int t_len, const float* __restrict__ freqs,
                                                          const float* __restrict__ w0, const float* __restrict__ b0,
                                                          const float* __restrict__ label_table, const float* __restrict__ label_bias, float label_scale,
                                                          const int64_t* __restrict__ y, int label_rows, float* __restrict__ h1, int F, int E) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= E) return;
  const float tv = t[t_len == 1 ? 0 : r];
  const int half = F / 2;
  const float* w = w0 + (long)j * F;
  const float* lab = nullptr;
  bool poison = false;
  if (label_table) {
    const long yr = (long)y[r];
    if (yr >= 0 && yr < label_rows) lab = label_table + yr * F;
    else poison = true;
  }
  float s = 0.f;
  for (int k = lane; k < 2 * half; k += 64) {
    const int i = k < half ? k : k - half;
    float a;
    if (FOURIER) {
      const float f2pi = 6.2831855f * freqs[i];  // rounded to fp32 before the product with t, as (2 * np.pi * self.freqs).to(x.dtype) is
      a = tv * f2pi;
    } else {
      a = tv * expf(-9.210340371976184f * (float)i / (float)(half - 1));
    }
    float v = k < half ? sinf(a) : cosf(a);
    if (lab) v += label_scale * lab[k] + label_bias[k];
    s += w[k] * v;
  }
  s = wave_sum(s);
  if (lane == 0) h1[(long)r * E + j] = poison ? __builtin_nanf("") : silu_exact_f(s + b0[j]);
}
__global__ __launch_bounds__(256) void song_embed2_kernel(const float* __restrict__ h1, const float* __restrict__ w1, const float* __restrict__ b1,
                                                          float* __restrict__ emb, half_t* __restrict__ emb_f16, int E) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= E) return;
  const float* w = w1 + (long)j * E;
  const float* h = h1 + (long)r * E;
  float s = 0.f;
  for (int k = lane; k < E; k += 64) s += w[k] * h[k];
  s = wave_sum(s);
  if (lane == 0) {
    const float v = silu_exact_f(s + b1[j]);
    emb[(long)r * E + j] = v;
    emb_f16[(long)r * E + j] = (half_t)v;
  }
}

static int song_embed_impl(const float* t, int t_len, const float* freqs, const float* w0, const float* b0, const float* w1, const float* b1,
                           const float* label_table, const float* label_bias, float label_scale, const int64_t* y, int label_rows, float* scratch_h1,
                           float* emb, void* emb_f16, int N, int F, int E, lfm_stream_t stream) {
  if (!t || !w0 || !b0 || !w1 || !b1 || !scratch_h1 || !emb || !emb_f16) return LFM_ERR_ARG;
  if ((label_table != nullptr) != (y != nullptr) || (label_table != nullptr) != (label_bias != nullptr)) return LFM_ERR_ARG;
  if (label_table && label_rows <= 0) return LFM_ERR_SHAPE;
  if (N <= 0 || F < 4 || (F & 1) || E <= 0 || (t_len != 1 && t_len != N)) return LFM_ERR_SHAPE;  // F >= 4: the endpoint table divides by F / 2 - 1
  hipStream_t st = (hipStream_t)stream;
  if (freqs)
    hipLaunchKernelGGL(song_embed1_kernel<true>, dim3(cdiv(E, 4), N), dim3(256), 0, st, t, t_len, freqs, w0, b0, label_table, label_bias, label_scale, y,
                       label_rows, scratch_h1, F, E);
  else
    hipLaunchKernelGGL(song_embed1_kernel<false>, dim3(cdiv(E, 4), N), dim3(256), 0, st, t, t_len, freqs, w0, b0, label_table, label_bias, label_scale, y,
                       label_rows, scratch_h1, F, E);
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(song_embed2_kernel, dim3(cdiv(E, 4), N), dim3(256), 0, st, scratch_h1, w1, b1, emb, (half_t*)emb_f16, E);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
extern "C" int lfm_song_embed(const float* t, int t_len, const float* w0, const float* b0, const float* w1, const float* b1, const float* label_table,
                              const float* label_bias, float label_scale, const int64_t* y, int label_rows, float* scratch_h1, float* emb,
                              void* emb_f16, int N, int F, int E, lfm_stream_t stream) {
  return song_embed_impl(t, t_len, nullptr, w0, b0, w1, b1, label_table, label_bias, label_scale, y, label_rows, scratch_h1, emb, emb_f16, N, F, E, stream);
}
// NCSN++ mapping network: the same with the Fourier features [sin(t g) | cos(t g)], g_i = fl32(2 pi) freqs[i], freqs fp32 [F / 2] (map_noise.freqs)
extern "C" int lfm_fourier_embed(const float* t, int t_len, const float* freqs, const float* w0, const float* b0, const float* w1, const float* b1,
                                 const float* label_table, const float* label_bias, float label_scale, const int64_t* y, int label_rows,
                                 float* scratch_h1, float* emb, void* emb_f16, int N, int F, int E, lfm_stream_t stream) {
  if (!freqs) return LFM_ERR_ARG;
  return song_embed_impl(t, t_len, freqs, w0, b0, w1, b1, label_table, label_bias, label_scale, y, label_rows, scratch_h1, emb, emb_f16, N, F, E, stream);
}
