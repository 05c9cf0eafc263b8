// SD f8 KL-VAE decoder on gfx950 (decode half of diffusers AutoencoderKL, sd-vae-ft-mse config).
// Reference call site: /root/reference/test_flow_latent.py:193  first_stage_model.decode(z / scale_factor).sample
// Activations are NHWC fp16 ([pixels, C] row-major == the GEMM "A" operand), so every 3x3 convolution is an
// implicit GEMM on the same MFMA kernel as the DiT linears: M = N*H*W pixels, N = Cout, K = 9*Cin with
// k = tap*Cin + ci; the A-tile gather (shifted pixel rows, zero padding, optional nearest-2x upsample) is done
// by the per-lane LDS-DMA source address.  GroupNorm statistics / apply+SiLU are bandwidth-bound side kernels.
#include "../../include/lfm_hip.h"
#include "nhwc_common.h"  // ASrcConv<MODE>, EpiResidF16, EpiConvStatsF16, EpiNCHWF32, conv_halo_allowed; groupnorm_common.h

// ------------------------------------------------------------------ epilogues (EpiResidF16, EpiConvStatsF16, EpiNCHWF32: nhwc_common.h)
struct EpiTransposeF16 {  // per image: Ct[img][n][m % T] = acc + bias[n]   (V^T for the mid attention)
  half_t* Ct;
  const float* bias;
  int T, N;
  typedef f32x4 Aux;
  __device__ __forceinline__ bool direct(int) const { return true; }
  __device__ __forceinline__ Aux load(int, int n) const { return *(const f32x4*)(bias + n); }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const {
    v += b;
    const int img = m / T, tok = m - img * T;
    half_t* d = Ct + ((long)img * N + n) * T + tok;
    d[0] = (half_t)v.x;
    d[T] = (half_t)v.y;
    d[2 * T] = (half_t)v.z;
    d[3 * T] = (half_t)v.w;
  }
};

struct EpiBatchF32 {  // batched scores: S[bz][m][n] = acc
  float* C;
  long ldc;
  typedef int Aux;
  __device__ __forceinline__ void batch(int bz, long bs) { C += (long)bz * bs; }
  __device__ __forceinline__ Aux load(int, int) const { return 0; }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux&) const { *(f32x4*)(C + (long)m * ldc + n) = v; }
};

struct EpiBatchF16 {  // batched: O[bz][m][n] = acc -> fp16
  half_t* C;
  long ldc;
  typedef int Aux;
  __device__ __forceinline__ void batch(int bz, long bs) { C += (long)bz * bs; }
  __device__ __forceinline__ Aux load(int, int) const { return 0; }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux&) const {
    half4_t h = {(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
    *(half4_t*)(C + (long)m * ldc + n) = h;
  }
};

struct EpiMomentsNCHW {  // encoder conv_out (+ folded quant_conv): fp32 NCHW [img][nch][pix], nch a multiple of 4
  float* out;
  const float* bias;
  int HW, nch;
  typedef f32x4 Aux;
  __device__ __forceinline__ Aux load(int, int n) const { return n < nch ? *(const f32x4*)(bias + n) : (f32x4){0.f, 0.f, 0.f, 0.f}; }
  __device__ __forceinline__ void store(int m, int n, f32x4 v, const Aux& b) const {
    if (n >= nch) return;
    v += b;
    const int img = m / HW, pix = m - img * HW;
    float* o = out + ((long)img * nch + n) * HW + pix;
    o[0] = v.x;
    o[HW] = v.y;
    o[2 * HW] = v.z;
    o[3 * HW] = v.w;
  }
};

// ------------------------------------------------------------------ post_quant_conv (1x1, 4->4) + conv_in (3x3, 4->Cout)
// z fp32 NCHW [N,4,R,R] -> fp16 NHWC [N,R,R,Cout].  conv_in sees post_quant(z) zero-padded, so the 1x1 is
// evaluated per tap and skipped (=0) outside the image.  One thread = one pixel x 8 output channels.
#define VCI_PIX 256
__global__ __launch_bounds__(256) void vae_conv_in_kernel(const float* __restrict__ z, const float* __restrict__ pq_w,
                                                          const float* __restrict__ pq_b, const float* __restrict__ w,
                                                          const float* __restrict__ b, half_t* __restrict__ out, int N, int R, int Cout, int ppb) {
  extern __shared__ __attribute__((aligned(16))) float wl[];  // conv_in weights transposed to [k = (c,ky,kx)][Cout]
  for (int e = threadIdx.x; e < 36 * Cout; e += 256) {
    const int co = e / 36, k = e - co * 36;
    wl[k * Cout + co] = w[e];
  }
  __syncthreads();
  const int c8n = Cout / 8, rows = 256 / c8n;
  const int oct = threadIdx.x % c8n, prow = threadIdx.x / c8n;
  if (prow >= rows) return;
  const int co = oct * 8;
  const long total = (long)N * R * R, p0 = (long)blockIdx.x * ppb;  // ppb = VCI_PIX pixels per block, fewer when the batch alone cannot fill the chip
  for (long pix = p0 + prow; pix < p0 + ppb && pix < total; pix += rows) {
    const int x = (int)(pix % R), y = (int)((pix / R) % R), n = (int)(pix / ((long)R * R));
    f32x4 a0 = *(const f32x4*)(b + co), a1 = *(const f32x4*)(b + co + 4);
#pragma unroll
    for (int t = 0; t < 9; ++t) {
      const int iy = y + t / 3 - 1, ix = x + t % 3 - 1;
      if ((unsigned)iy >= (unsigned)R || (unsigned)ix >= (unsigned)R) continue;
      float zi[4];
#pragma unroll
      for (int c = 0; c < 4; ++c) zi[c] = z[(((long)n * 4 + c) * R + iy) * R + ix];
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const float pq = pq_b[c] + pq_w[c * 4 + 0] * zi[0] + pq_w[c * 4 + 1] * zi[1] + pq_w[c * 4 + 2] * zi[2] + pq_w[c * 4 + 3] * zi[3];
        const float* wr = wl + (c * 9 + t) * Cout + co;
        a0 += pq * *(const f32x4*)wr;
        a1 += pq * *(const f32x4*)(wr + 4);
      }
    }
    half8_t h = {(half_t)a0.x, (half_t)a0.y, (half_t)a0.z, (half_t)a0.w, (half_t)a1.x, (half_t)a1.y, (half_t)a1.z, (half_t)a1.w};
    *(half8_t*)(out + pix * Cout + co) = h;
  }
}

// ------------------------------------------------------------------ GroupNorm(32 groups, eps 1e-6) on NHWC fp16
// Two-stage, deterministic statistics: the producing convolution's epilogue (EpiConvStatsF16) or a pass of its own (gn_stats_rows_kernel) folds
// slabs of pixels into per-half-octet partial {mean, M2} slots part[n][slab][C/4] (groupnorm_common.h: both shifted, so a group whose mean is hundreds
// of standard deviations keeps its variance); a small second kernel merges the slabs and the half-octets of a group in a fixed order into
// stats[n][g] = {mean, rstd}; apply fuses SiLU.  The apply is ((x - mean) rstd) gamma + beta, the decoder's own rounding (constant groups come out
// as exactly beta), which is why these two kernels are not the UNets' (groupnorm_kernels.h: x a + b); the slot arithmetic, the closing step, the
// statistics kernel and the host constants are shared.
// one WAVE per (image, group): lane l folds slabs l, l + 64, ... in order, then a fixed-tree wave sum (deterministic).  (One thread per
// (image, group) walking all slabs serially took 75 us once the convolution epilogues started to deliver 512 slabs per image.)
// Slot {mean m, M2} of slab b holds c = 4 min(ppb, HW - b ppb) values; the merge is shifted by the group's first slot mean K (gn_merge).
__global__ __launch_bounds__(256) void gn_finish_kernel(const float* __restrict__ part, float* __restrict__ stats, int slabs, int ppb, int HW, int C,
                                                        int total) {
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;  // (n, g)
  if (i >= total) return;
  const int n = i >> 5, g = i & 31, hpg = C / 128;  // half-octets per group = (C/32)/4
  const float K = part[((long)n * slabs * (C / 4) + g * hpg) * 2];
  float sum = 0.f, sq = 0.f;
  for (int b = lane; b < slabs; b += 64) {
    const float* p = part + (((long)n * slabs + b) * (C / 4) + g * hpg) * 2;
    const float c = (float)(4 * min(ppb, HW - b * ppb));
    for (int h = 0; h < hpg; ++h) gn_merge(sum, sq, p + 2 * h, c, K);
  }
  sum = wave_sum(sum);
  sq = wave_sum(sq);
  if (lane == 0) gn_mean_rstd(K, sum, sq, (float)HW * (float)(C / 32), 1e-6f, stats[(long)i * 2], stats[(long)i * 2 + 1]);
}

// apply: y = silu?((x - mean) rstd gamma + beta).  Round 4: a thread OWNS one channel octet (256 % (C / 8) == 0) and walks the pixels of its block's
// slab, so the statistics, gamma and beta are read once per thread and there is no per-element 64-bit index arithmetic (the first version -- one
// 16-byte chunk per thread, four divisions and two 64-bit div / mod per chunk -- ran at 2.3 TB/s on the 2.15 GB full-resolution tensors:
// profiles/r03_final_bench_kernel_stats.csv, 6.2 ms of a 39.6 ms decode).  Same arithmetic per element.
template <bool SILU>
__global__ __launch_bounds__(256) void gn_apply_kernel(const half_t* __restrict__ x, half_t* __restrict__ y, const float* __restrict__ stats,
                                                       const float* __restrict__ gamma, const float* __restrict__ beta, int HW, int C,
                                                       int pix_per_block) {
  const int n = blockIdx.y, c8n = C / 8, cpg = C / 32, tid = threadIdx.x;
  const int oct = tid % c8n, prow = tid / c8n, pstride = 256 / c8n;
  float mean[2], rstd[2];
#pragma unroll
  for (int hh = 0; hh < 2; ++hh) {  // stats[n][g] = {mean, rstd} (gn_finish_kernel)
    const int g = (oct * 8 + hh * 4) / cpg;
    mean[hh] = stats[((long)n * 32 + g) * 2];
    rstd[hh] = stats[((long)n * 32 + g) * 2 + 1];
  }
  const f32x4 g0 = *(const f32x4*)(gamma + oct * 8), g1 = *(const f32x4*)(gamma + oct * 8 + 4);
  const f32x4 b0 = *(const f32x4*)(beta + oct * 8), b1 = *(const f32x4*)(beta + oct * 8 + 4);
  const float gm[8] = {g0.x, g0.y, g0.z, g0.w, g1.x, g1.y, g1.z, g1.w}, bt[8] = {b0.x, b0.y, b0.z, b0.w, b1.x, b1.y, b1.z, b1.w};
  const int p0 = blockIdx.x * pix_per_block, p1 = min(p0 + pix_per_block, HW);
  const long base = ((long)n * HW) * C + oct * 8;
  auto one = [&](const half8_t v) {
    half8_t o;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      float f = ((float)v[j] - mean[j >> 2]) * rstd[j >> 2] * gm[j] + bt[j];
      if (SILU) f = silu_f(f);
      o[j] = (half_t)f;
    }
    return o;
  };
  int p = p0 + prow;
  for (; p + 3 * pstride < p1; p += 4 * pstride) {  // four chunks in flight per thread (gn_walk's loop in its own text: see there)
    half8_t v[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) v[u] = *(const half8_t*)(x + base + (long)(p + u * pstride) * C);
#pragma unroll
    for (int u = 0; u < 4; ++u) *(half8_t*)(y + base + (long)(p + u * pstride) * C) = one(v[u]);
  }
  for (; p < p1; p += pstride) *(half8_t*)(y + base + (long)p * C) = one(*(const half8_t*)(x + base + (long)p * C));
}

// rows of S [rows, T] fp32 -> P fp16 = softmax(S * scale); one wave per row.
__global__ __launch_bounds__(256) void softmax_rows_kernel(const float* __restrict__ S, half_t* __restrict__ P, long rows, int T, float scale_log2e) {
  const int lane = threadIdx.x & 63;
  const long r = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (r >= rows) return;
  const float* s = S + r * T;
  float mx = -3.0e38f;
  for (int i = lane; i < T; i += 64) mx = fmaxf(mx, s[i]);
  mx = wave_max(mx) * scale_log2e;
  float sum = 0.f;
  for (int i = lane; i < T; i += 64) sum += __builtin_amdgcn_exp2f(s[i] * scale_log2e - mx);
  const float inv = 1.0f / wave_sum(sum);
  half_t* p = P + r * T;
  for (int i = lane; i < T; i += 64) p[i] = (half_t)(__builtin_amdgcn_exp2f(s[i] * scale_log2e - mx) * inv);
}

// ------------------------------------------------------------------ host side
static inline size_t a256(size_t v) { return (v + 255) / 256 * 256; }

struct VaeWs {
  half_t* b[4];       // four rotating activation buffers of the largest size
  float* stats;       // [images, 32, 2] {mean, rstd}
  float* part;        // [images, slabs, C / 4, 2] partial {mean, M2} of the two-stage GroupNorm statistics
  half_t* zeros;      // 256 B
  float* S;           // [images, T, T] scores
  size_t part_pairs;  // capacity of `part` in {mean, M2} pairs
};

// What one call needs of its workspace.  Every entry point describes itself with one of these, vae_carve lays it out, and gn reads part_pairs from
// it: the description alone decides how many statistics slabs a GroupNorm picks, so a stage entry point that gives part_pairs the decoder's value
// sums in the decoder's order.
struct VaeNeed {
  size_t buf_bytes;    // each of the four rotating buffers (0: none)
  size_t images;       // stats holds {mean, rstd} of 32 groups for this many images (0: none)
  size_t part_pairs;   // room for partial statistics in {mean, M2} pairs (0: none, ws.part stays null and no convolution leaves statistics)
  size_t score_bytes;  // the mid attention's fp32 scores (0: none)
};

static inline size_t max_sz(size_t a, size_t b) { return a > b ? a : b; }

// lfm_vae_decode / lfm_vae_encode, `chunk` images per pass.  The largest activation is the upsample convolution's 256 channels at 8R x 8R.  part: per image
// the larger of the convolution epilogues' 128-row slabs (2 HW / 256 x C / 4 half-octets, at most (8R)^2 x 256 / 512) and the statistics pass's
// GN_MAX_SLABS x 128.  A last, shorter pass keeps the room of `chunk` images (gn may then pick more slabs per image).
static VaeNeed vae_need_coder(int R, int chunk) {
  const size_t px = (size_t)(8 * R) * (8 * R), T = (size_t)R * R, c = (size_t)chunk;
  return {c * px * 256 * 2, c, c * max_sz(px * 256 / 512, (size_t)GN_MAX_SLABS * 128), c * T * T * 4};
}
// The mid-block attention alone: the buffers hold Q | K and V^T | P (n T (512 + max(512, T)) halves), part is the decoder's share per image at R^2 = T.
static VaeNeed vae_need_attention(int n, int T) {
  const size_t M = (size_t)n * T;
  return {M * (512 + max_sz(T, 512)) * 2, (size_t)n, n * max_sz(32 * (size_t)T, (size_t)GN_MAX_SLABS * 128), M * T * 4};
}
// A run of resnets up to 512 channels wide: part as in the decoder, with the epilogue slabs of a ragged map rounded up.
static VaeNeed vae_need_resnets(int n, int HW) {
  return {(size_t)n * HW * 512 * 2, (size_t)n, n * max_sz(2 * (size_t)cdiv(HW, 256) * 128, (size_t)GN_MAX_SLABS * 128), 0};
}
// The two GroupNorm entry points: part is what the caller's bytes leave after stats and the zero page, in whole 256-byte pieces (32 pairs: every
// count gn compares it with or divides it by is a multiple of 32).  Below `least_pairs` the description asks for that much, which no longer fits
// into the caller's bytes: vae_setup answers LFM_ERR_WORKSPACE.
static VaeNeed vae_need_gn(int n, size_t bytes, size_t least_pairs) {
  const size_t fixed = 256 + a256((size_t)n * 256), room = bytes > fixed ? (bytes - fixed) / 256 * 32 : 0;
  return {0, (size_t)n, max_sz(room, least_pairs), 0};
}
static const VaeNeed VAE_NEED_ZEROS{0, 0, 0, 0};  // the two bare convolutions: the zero page alone

// The one layout: [four buffers][stats][part][zeros 256 B][scores], every piece rounded up to 256 bytes, an empty piece null.  Returns the total;
// base null: sizes only.
static size_t vae_carve(const VaeNeed& d, void* base, VaeWs* w) {
  size_t off = 0;
  auto take = [&](size_t bytes) {
    char* p = base && bytes ? (char*)base + off : nullptr;
    off += a256(bytes);
    return p;
  };
  VaeWs o{};
  for (half_t*& b : o.b) b = (half_t*)take(d.buf_bytes);
  o.stats = (float*)take(d.images * 64 * 4);
  o.part = (float*)take(d.part_pairs * 2 * 4);
  o.part_pairs = d.part_pairs;
  o.zeros = (half_t*)take(256);
  o.S = (float*)take(d.score_bytes);
  if (w) *w = o;
  return off;
}

extern "C" size_t lfm_vae_workspace_bytes(int R, int chunk) {
  if (R <= 0 || chunk <= 0 || (R % 8)) return 0;
  return vae_carve(vae_need_coder(R, chunk), nullptr, nullptr);
}

#define RC(x)            \
  do {                   \
    int _rc = (x);       \
    if (_rc) return _rc; \
  } while (0)

struct VaeConv {  // a 3x3 convolution layer: w fp16 [Cout][9][Cin], b fp32 [Cout]; ups: on the nearest-2x upsampled input
  const void* w;
  const float* b;
  int Cin, Cout;
  bool ups;
};

struct VaeAttn {  // the mid-block attention's parameters, as lfm_vae_weights and lfm_vae_enc_weights hold them
  const float *at_g, *at_b;
  const void* q_w;
  const float* q_b;
  const void* k_w;
  const float* k_b;
  const void* v_w;
  const float* v_b;
  const void* o_w;
  const float* o_b;
};

// The host driver's state for n images: the carve, the stream, the four rotating activation buffers (x holds the current tensor) and what is known
// about x.  vae_setup makes it; the entry points whose description has no buffers call gn and conv3 with the caller's tensors.
struct VaeCtx {
  VaeWs ws;
  int n;
  hipStream_t st;
  half_t *x, *t1, *t2, *t3;
  int x_slabs;       // partial-sum slabs per image that the producer of x left in ws.part (0 = none: the GroupNorm runs its own statistics pass)
  bool chain_stats;  // decoder: the last convolution of a resnet leaves the statistics of its output for the GroupNorm that follows
  void rotate(half_t*& t) {  // the result was written to t: it becomes x, the old x becomes scratch
    half_t* o = t;
    t = x;
    x = o;
  }
  int gn(const half_t* in, half_t* y, const float* g, const float* b, int HW, int C, bool silu, int ready_slabs) const;
  int conv3(const half_t* in, half_t* out, const half_t* resid, int H, int W, const VaeConv& c, int* stat_slabs, int* stat_kernel = nullptr) const;
  int conv_down(const void* w, const float* b, int Ho, int Wo, int C);
  int resnet(const lfm_vae_resnet* r, int H, int W);
  int mid_attention(const VaeAttn& w, int T);
};

// The set-up of every entry point with a workspace, after its own argument checks: refuse a misaligned workspace, then one too short for `need`; carve; zero
// the zero page (once per call, the first thing enqueued); hand back the state for n images.  Nothing is enqueued before the last refusal.
static int vae_setup(const VaeNeed& need, void* workspace, size_t bytes, int n, lfm_stream_t stream, bool chain_stats, VaeCtx& c) {
  if ((uintptr_t)workspace & 255) return LFM_ERR_ALIGN;
  if (vae_carve(need, nullptr, nullptr) > bytes) return LFM_ERR_WORKSPACE;
  VaeWs ws;
  vae_carve(need, workspace, &ws);
  c = VaeCtx{ws, n, (hipStream_t)stream, ws.b[0], ws.b[1], ws.b[2], ws.b[3], 0, chain_stats};
  return lfm_zero_async(ws.zeros, 256, c.st) ? LFM_ERR_LAUNCH : LFM_OK;
}

// The decoder's slab policy: {slabs per image, pixels per slab} of the statistics a GroupNorm of n images merges.  ready_slabs > 0: the convolution that
// produced the tensor left that many (the epilogues: 128 pixels each).  Else the GroupNorm's own pass: GN_MAX_SLABS when the images fill the chip; a FEW
// images (--measure_time decodes ONE) get up to 512 -- 64 blocks walked a 256x256x128 map in 64 dependent 16-byte loads per thread, 68 us per GroupNorm and
// 38 % of the batch-1 decode (profiles/r06_latency_mode.txt) -- as far as ws.part has room (part_pairs = its capacity in pairs, 0 = unknown: the old cap).
struct VaeGnSlabs {
  int slabs, ppb;
};
static inline VaeGnSlabs vae_gn_slabs(int n, int HW, int C, size_t part_pairs, int ready_slabs) {
  if (ready_slabs) return {ready_slabs, HW / ready_slabs};
  int cap = GN_MAX_SLABS;
  if (part_pairs && n * GN_MAX_SLABS < 1024) {
    const long room = (long)(part_pairs / ((size_t)n * (C / 4)));
    const long want = 1024 / n;
    cap = (int)(want < room ? want : room);
    if (cap > 512) cap = 512;
    if (cap < GN_MAX_SLABS) cap = GN_MAX_SLABS;
  }
  int ppb = 1024;
  if (cap > GN_MAX_SLABS) ppb = cdiv(HW, cap) > 64 ? cdiv(HW, cap) : 64;  // >= 64 pixels per block: at least a few loads per thread
  if (cdiv(HW, ppb) > cap) ppb = cdiv(HW, cap);
  return {cdiv(HW, ppb), ppb};
}

// y = silu?(GroupNorm(in) g + b).  ready_slabs > 0: the convolution that produced `in` already left its partial sums in ws.part (EpiConvStatsF16), in
// that many slabs per image
int VaeCtx::gn(const half_t* in, half_t* y, const float* g, const float* b, int HW, int C, bool silu, int ready_slabs) const {
  if (C % 128 || 256 % (C / 8) || C > 512) return LFM_ERR_SHAPE;  // groups of >= 4 channels, octet-per-thread mapping
  const VaeGnSlabs s = vae_gn_slabs(n, HW, C, ws.part_pairs, ready_slabs);
  if (!ready_slabs) {
    hipLaunchKernelGGL(gn_stats_rows_kernel, dim3(s.slabs, n), dim3(256), 0, st, GnIn{in, nullptr, C, 0}, ws.part, HW, C, s.ppb);
    LFM_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(gn_finish_kernel, dim3(cdiv(n * 32, 4)), dim3(256), 0, st, ws.part, ws.stats, s.slabs, s.ppb, HW, C, n * 32);
  LFM_CHECK_LAUNCH();
  const int app = gn_pixels_per_block(HW);
  GN_LAUNCH_SILU(gn_apply_kernel, silu, dim3(cdiv(HW, app), n), st, in, y, ws.stats, g, b, HW, C, app);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// out[n,H,W,Cout] = conv3x3(in (optionally nearest-2x upsampled)) + bias (+ resid)
// stat_slabs (null: no statistics wanted): set to the number of partial-sum slabs per image this convolution left in ws.part for the GroupNorm that
// follows, or 0; *stat_kernel (optional): which kernel left them -- 1 the halo-tiled convolution, 2 a 256-row implicit GEMM, 0 none
int VaeCtx::conv3(const half_t* in, half_t* out, const half_t* resid, int H, int W, const VaeConv& c, int* stat_slabs, int* stat_kernel) const {
  const int Cin = c.Cin, Cout = c.Cout, HW = H * W, M = n * HW;
  const half_t* w = (const half_t*)c.w;
  if (Cin % 64 || Cout % 4) return LFM_ERR_SHAPE;
  if (stat_slabs) *stat_slabs = 0;
  if (stat_kernel) *stat_kernel = 0;
  // the statistics epilogue, as far as it does not depend on the kernel: a tile lies in one image, 16-byte stores, VAE_SEPARATE_STATS (A/B) not set
  const bool stats_ok = ws.part && stat_slabs && (HW % 256) == 0 && !(((uintptr_t)out | (uintptr_t)resid) & 15) &&
                        !(lfm_gemm_debug_flags() & LFM_DBG_VAE_SEPARATE_STATS);
  const EpiResidF16 ep{out, Cout, c.b, resid};
  const EpiConvStatsF16 es{ep, ws.part, HW, 2 * (HW / 256)};
  auto left = [&](int kernel) {
    *stat_slabs = es.slabs;
    if (stat_kernel) *stat_kernel = kernel;
  };
  // every 3x3 convolution on a 16-aligned map: the halo-tiled direct kernel (conv_halo_kernel.h; 1.1-1.2 PFLOP/s where the implicit GEMM reaches
  // 0.65-1.05, profiles/r03_halo_conv_probe.txt)
  if (conv_halo_allowed(out, resid)) {
    auto halo = [&](const auto& e) {
      return c.ups ? launch_conv3x3_halo<1>(in, ws.zeros, w, n, H, W, Cin, Cout, e, st) : launch_conv3x3_halo<0>(in, ws.zeros, w, n, H, W, Cin, Cout, e, st);
    };
    const int rc = stats_ok ? halo(es) : halo(ep);
    if (rc == 0 && stats_ok) left(1);
    if (rc != 1) return rc;
  }
  // the implicit GEMM.  The statistics epilogue leaves its partials in the slot layout of the 256-row kernels' tiles: ask which kernel runs for the types
  // about to be launched, take the epilogue only if that is one of them, and launch THAT kernel (one decision for the layout and the launch).
  auto gemm = [&](const auto& a) {
    const int kern = gemm_choose(M, Cout, 9 * Cin, 1, gemm_caps<std::decay_t<decltype(a)>, EpiConvStatsF16>(a, Cout, 9L * Cin));
    if (stats_ok && (kern == 4 || kern == 5) && (Cout % (kern == 4 ? 128 : 256)) == 0 && (Cout % 128) == 0 &&
        !(lfm_gemm_debug_flags() & LFM_DBG_GEMM_STORE8)) {
      left(2);
      return launch_gemm_kernel(kern, a, w, 9L * Cin, M, Cout, 9 * Cin, es, st);
    }
    return launch_gemm_auto(a, w, 9L * Cin, M, Cout, 9 * Cin, ep, st);
  };
  if (c.ups) return gemm(ASrcConv<1>{in, ws.zeros, H, W, Cin, M});
  return gemm(ASrcConv<0>{in, ws.zeros, H, W, Cin, M});
}

// ---- test entry points: the decoder's GroupNorm (gn, its own statistics pass) and the conv3 -> gn hand-over, on the decoder's host code.
// Workspace (vae_need_gn): stats for n images, the zero page, and part: the rest, in {mean, M2} pairs (the decoder sizes part by
// lfm_vae_workspace_bytes; gn picks as many statistics slabs as part has room for, as in the decoder).
static inline bool vae_groupnorm_shape_ok(int n, int HW, int C) { return n > 0 && HW > 0 && (C == 128 || C == 256 || C == 512); }  // gn's own rule
static inline VaeNeed vae_need_groupnorm(int n, int C, size_t bytes) { return vae_need_gn(n, bytes, (size_t)n * GN_MAX_SLABS * (C / 4)); }

extern "C" int lfm_vae_groupnorm_f16(const void* x, void* y, const float* gamma, const float* beta, void* workspace, size_t workspace_bytes, int n,
                                     int HW, int C, int silu, lfm_stream_t stream) {
  if (!x || !y || !gamma || !beta || !workspace) return LFM_ERR_ARG;
  if (!vae_groupnorm_shape_ok(n, HW, C)) return LFM_ERR_SHAPE;  // ahead of the set-up's zero fill
  if (((uintptr_t)x | (uintptr_t)y) & 15) return LFM_ERR_ALIGN;
  VaeCtx c;
  RC(vae_setup(vae_need_groupnorm(n, C, workspace_bytes), workspace, workspace_bytes, n, stream, false, c));
  return c.gn((const half_t*)x, (half_t*)y, gamma, beta, HW, C, silu != 0, 0);
}
// The slabs per image of that call's statistics pass, with its refusals of a shape and of a short workspace; no launch.
extern "C" int lfm_vae_groupnorm_plan(int n, int HW, int C, size_t workspace_bytes) {
  if (!vae_groupnorm_shape_ok(n, HW, C)) return LFM_ERR_SHAPE;
  const VaeNeed need = vae_need_groupnorm(n, C, workspace_bytes);
  if (vae_carve(need, nullptr, nullptr) > workspace_bytes) return LFM_ERR_WORKSPACE;
  return vae_gn_slabs(n, HW, C, need.part_pairs, 0).slabs;
}

extern "C" int lfm_vae_conv3x3_gn_f16(const void* in, const void* w, const float* bias, const void* resid, void* conv_out, void* y, const float* gamma,
                                      const float* beta, void* workspace, size_t workspace_bytes, int n, int H, int W, int Cin, int Cout, int ups,
                                      int silu, int* stat_slabs, int* stat_kernel, lfm_stream_t stream) {
  if (!in || !w || !bias || !conv_out || !y || !gamma || !beta || !workspace) return LFM_ERR_ARG;
  if (n <= 0 || H <= 0 || W <= 0 || (ups && ((H | W) & 1))) return LFM_ERR_SHAPE;
  if (((uintptr_t)in | (uintptr_t)w | (uintptr_t)resid | (uintptr_t)conv_out | (uintptr_t)y) & 15) return LFM_ERR_ALIGN;
  const size_t conv_pairs = (size_t)n * 2 * (H * W / 256) * (Cout / 4), stat_pairs = (size_t)n * GN_MAX_SLABS * (Cout / 4);
  VaeCtx c;
  RC(vae_setup(vae_need_gn(n, workspace_bytes, max_sz(conv_pairs, stat_pairs)), workspace, workspace_bytes, n, stream, false, c));
  int slabs = 0, kern = 0;
  RC(c.conv3((const half_t*)in, (half_t*)conv_out, (const half_t*)resid, H, W, VaeConv{w, bias, Cin, Cout, ups != 0}, &slabs, &kern));
  RC(c.gn((const half_t*)conv_out, (half_t*)y, gamma, beta, H * W, Cout, silu != 0, slabs));
  if (stat_slabs) *stat_slabs = slabs;
  if (stat_kernel) *stat_kernel = kern;
  return LFM_OK;
}

// diffusers ResnetBlock2D: GroupNorm+SiLU -> conv -> GroupNorm+SiLU -> conv + (1x1 shortcut of) x.  x is replaced by the result (buffers rotate).
int VaeCtx::resnet(const lfm_vae_resnet* r, int H, int W) {
  const int HW = H * W, M = n * HW;
  int mid_slabs = 0;
  RC(gn(x, t1, r->n1_g, r->n1_b, HW, r->cin, true, x_slabs));
  RC(conv3(t1, t2, nullptr, H, W, VaeConv{r->c1_w, r->c1_b, r->cin, r->cout, false}, &mid_slabs));
  RC(gn(t2, t1, r->n2_g, r->n2_b, HW, r->cout, true, mid_slabs));
  const half_t* skip = x;
  if (r->sc_w) {  // 1x1 conv shortcut
    RC(launch_gemm_auto(ASrcRowMajor{x, r->cin, M, 0}, (const half_t*)r->sc_w, r->cin, M, r->cout, r->cin, EpiResidF16{t3, r->cout, r->sc_b, nullptr}, st));
    skip = t3;
  }
  x_slabs = 0;
  RC(conv3(t1, t2, skip, H, W, VaeConv{r->c2_w, r->c2_b, r->cout, r->cout, false}, chain_stats ? &x_slabs : nullptr));
  rotate(t2);
  return LFM_OK;
}

// mid-block attention (diffusers Attention, 1 head of 512 channels over T tokens, residual): GroupNorm -> q, k, v -> softmax(q k^T / sqrt(C)) v
// -> to_out + x, all on the GEMM kernel.  x is replaced by the result (buffers rotate).
int VaeCtx::mid_attention(const VaeAttn& w, int T) {
  const int M = n * T, C = 512;
  RC(gn(x, t1, w.at_g, w.at_b, T, C, false, x_slabs));
  half_t* Qb = t2;                  // [M, C]
  half_t* Kb = t2 + (size_t)M * C;  // [M, C]
  half_t* Vt = t3;                  // [n, C, T]
  half_t* Pb = t3 + (size_t)M * C;  // [n, T, T]
  const ASrcRowMajor a{t1, C, M, 0};
  RC(launch_gemm_tn(a, (const half_t*)w.q_w, C, M, C, C, EpiResidF16{Qb, C, w.q_b, nullptr}, st));
  RC(launch_gemm_tn(a, (const half_t*)w.k_w, C, M, C, C, EpiResidF16{Kb, C, w.k_b, nullptr}, st));
  RC(launch_gemm_tn(a, (const half_t*)w.v_w, C, M, C, C, EpiTransposeF16{Vt, w.v_b, T, C}, st));
  RC(launch_gemm_tn(ASrcRowMajor{Qb, C, T, 0}, Kb, C, T, T, C, EpiBatchF32{ws.S, T}, st, n, (long)T * C, (long)T * C, (long)T * T));
  hipLaunchKernelGGL(softmax_rows_kernel, dim3(cdiv((long)n * T, 4)), dim3(256), 0, st, ws.S, Pb, (long)n * T, T, 1.4426950408889634f / sqrtf((float)C));
  LFM_CHECK_LAUNCH();
  half_t* Ob = t1;  // GN output is dead now
  RC(launch_gemm_tn(ASrcRowMajor{Pb, T, T, 0}, Vt, T, T, C, T, EpiBatchF16{Ob, C}, st, n, (long)T * T, (long)C * T, (long)T * C));
  RC(launch_gemm_tn(ASrcRowMajor{Ob, C, M, 0}, (const half_t*)w.o_w, C, M, C, C, EpiResidF16{t2, C, w.o_b, x}, st));
  x_slabs = 0;
  rotate(t2);
  return LFM_OK;
}

// ---- test entry point: the decoder's mid-block attention on the caller's weights.  Workspace: vae_need_attention, so the GroupNorm picks the slab
// count it picks in a decode at R^2 = T.
extern "C" size_t lfm_vae_mid_attention_workspace_bytes(int n, int T) {
  if (n <= 0 || T <= 0 || (T % 64)) return 0;
  return vae_carve(vae_need_attention(n, T), nullptr, nullptr);
}

extern "C" int lfm_vae_mid_attention_f16(const void* x, void* out, const float* gn_gamma, const float* gn_beta, const void* q_w, const float* q_b,
                                         const void* k_w, const float* k_b, const void* v_w, const float* v_b, const void* o_w, const float* o_b,
                                         void* workspace, size_t workspace_bytes, int n, int T, lfm_stream_t stream) {
  if (!x || !out || !gn_gamma || !gn_beta || !q_w || !q_b || !k_w || !k_b || !v_w || !v_b || !o_w || !o_b || !workspace) return LFM_ERR_ARG;
  if (n <= 0 || T <= 0 || (T % 64)) return LFM_ERR_SHAPE;  // the decoder's T = R^2 with R % 8 == 0
  if ((long)n * T * (T > 512 ? T : 512) >= (1L << 31)) return LFM_ERR_SHAPE;  // 32-bit row offsets of the GEMM operands
  if (((uintptr_t)x | (uintptr_t)out | (uintptr_t)q_w | (uintptr_t)k_w | (uintptr_t)v_w | (uintptr_t)o_w | (uintptr_t)gn_gamma | (uintptr_t)gn_beta |
       (uintptr_t)q_b | (uintptr_t)k_b | (uintptr_t)v_b | (uintptr_t)o_b) & 15)
    return LFM_ERR_ALIGN;
  VaeCtx c;
  RC(vae_setup(vae_need_attention(n, T), workspace, workspace_bytes, n, stream, false, c));
  const size_t bytes = (size_t)n * T * 512 * 2;
  if (hipMemcpyAsync(c.x, x, bytes, hipMemcpyDeviceToDevice, c.st) != hipSuccess) return LFM_ERR_LAUNCH;
  RC(c.mid_attention(VaeAttn{gn_gamma, gn_beta, q_w, q_b, k_w, k_b, v_w, v_b, o_w, o_b}, T));
  if (hipMemcpyAsync(out, c.x, bytes, hipMemcpyDeviceToDevice, c.st) != hipSuccess) return LFM_ERR_LAUNCH;
  return LFM_OK;
}

// post_quant_conv + conv_in: z [n,4,R,R] fp32 NCHW -> out fp16 NHWC [n,R,R,512]
static int vae_conv_in(const float* pq_w, const float* pq_b, const float* cin_w, const float* cin_b, const float* z, half_t* out, int n, int R,
                       hipStream_t st) {
  if (!lfm_kernel_lds<&vae_conv_in_kernel>(36 * 512 * 4)) return LFM_ERR_LAUNCH;
  // batch 1 (--measure_time: run_sampling(1, ..), reference test_flow_latent.py:223-246): 1024 pixels are FOUR blocks of 256 pixels -- 183 us for 38 MFLOP
  // (profiles/r06_latency_mode.txt); 16 pixels per block put them on 64 CUs
  const long pixels = (long)n * R * R;
  const int ppb = pixels >= 256L * VCI_PIX ? VCI_PIX : (pixels >= 64L * VCI_PIX ? 64 : 16);
  hipLaunchKernelGGL(vae_conv_in_kernel, dim3(cdiv(pixels, ppb)), dim3(256), 36 * 512 * 4, st, z, pq_w, pq_b, cin_w, cin_b, out, n, R, 512, ppb);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// ---- test entry point: the decoder's first kernel on the caller's tensors
extern "C" int lfm_vae_conv_in_f16(const float* pq_w, const float* pq_b, const float* cin_w, const float* cin_b, const float* z, void* out, int n, int R,
                                   lfm_stream_t stream) {
  if (!pq_w || !pq_b || !cin_w || !cin_b || !z || !out) return LFM_ERR_ARG;
  if (n <= 0 || R <= 0 || (long)n * R * R * 512 >= (1L << 31)) return LFM_ERR_SHAPE;  // any R: R % 8 is lfm_vae_decode's rule
  if (((uintptr_t)pq_w | (uintptr_t)pq_b | (uintptr_t)cin_w | (uintptr_t)cin_b | (uintptr_t)z | (uintptr_t)out) & 15) return LFM_ERR_ALIGN;
  return vae_conv_in(pq_w, pq_b, cin_w, cin_b, z, (half_t*)out, n, R, (hipStream_t)stream);
}

// one chunk of images: z [n,4,R,R] -> out [n,3,8R,8R]
static int vae_decode_chunk(VaeCtx& c, const lfm_vae_weights* w, const float* z, float* out, int R) {
  RC(vae_conv_in(w->pq_w, w->pq_b, w->cin_w, w->cin_b, z, c.x, c.n, R, c.st));
  int H = R;
  RC(c.resnet(&w->mid[0], H, H));
  RC(c.mid_attention(VaeAttn{w->at_g, w->at_b, w->q_w, w->q_b, w->k_w, w->k_b, w->v_w, w->v_b, w->o_w, w->o_b}, R * R));
  RC(c.resnet(&w->mid[1], H, H));
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 3; ++j) RC(c.resnet(&w->up[i][j], H, H));
    if (i < 3) {
      const int C = w->up[i][2].cout;
      H *= 2;
      RC(c.conv3(c.x, c.t1, nullptr, H, H, VaeConv{w->ups_w[i], w->ups_b[i], C, C, true}, &c.x_slabs));
      c.rotate(c.t1);
    }
  }
  RC(c.gn(c.x, c.t1, w->no_g, w->no_b, H * H, 128, true, c.x_slabs));
  return launch_conv3x3_out(c.t1, c.ws.zeros, (const half_t*)w->cout_w, c.n, H, H, 128, EpiNCHWF32{out, w->cout_b, H * H, 3}, c.st);
}

extern "C" int lfm_vae_decode(const lfm_vae_weights* w, void* workspace, size_t workspace_bytes, const float* z, float* out, int N, int R,
                              int chunk, lfm_stream_t stream) {
  if (!w || !workspace || !z || !out) return LFM_ERR_ARG;
  if (N <= 0 || R <= 0 || (R % 8) || chunk <= 0) return LFM_ERR_SHAPE;
  VaeCtx first;  // every pass starts from this state: the same buffers in the same roles, the room of `chunk` images
  RC(vae_setup(vae_need_coder(R, chunk), workspace, workspace_bytes, chunk, stream, true, first));
  for (int n0 = 0; n0 < N; n0 += chunk) {
    VaeCtx c = first;
    if (N - n0 < chunk) c.n = N - n0;
    RC(vae_decode_chunk(c, w, z + (long)n0 * 4 * R * R, out + (long)n0 * 3 * 64 * R * R, R));
  }
  return LFM_OK;
}


// ------------------------------------------------------------------ encoder (diffusers AutoencoderKL.encode, sd-vae-ft-mse config)
// Reference call sites: train_flow_latent.py:143 and downstream_tasks/test_flow_latent_inpainting.py:146
//   first_stage_model.encode(x).latent_dist.sample().mul_(scale_factor)
// moments[N,8,R,R] fp32 NCHW = quant_conv(Encoder(x)) for x[N,3,8R,8R] fp32 NCHW: channels 0..3 the mean, 4..7 the log-variance of the
// DiagonalGaussianDistribution (the sampling / clamping of the distribution is host code).  quant_conv (1x1, 8 -> 8) is folded into
// conv_out's weights by the caller (exact algebra).  Same workspace as the decoder (lfm_vae_workspace_bytes(R, chunk)).
extern "C" int lfm_conv3x3_in_f32(const float* x_nchw, const float* w, const float* bias, void* out_nhwc, int N, int H, int W, int Cin, int Cout,
                                  lfm_stream_t stream);

// diffusers Downsample2D (stride 2, input padded (0,1,0,1)): x [n, 2 Ho, 2 Wo, C] -> [n, Ho, Wo, C].  x is replaced by the result.
int VaeCtx::conv_down(const void* w, const float* b, int Ho, int Wo, int C) {
  if (C % 64) return LFM_ERR_SHAPE;
  const int M = n * Ho * Wo;
  RC(launch_gemm_auto(ASrcConv<3>{x, ws.zeros, Ho, Wo, C, M}, (const half_t*)w, 9L * C, M, C, 9 * C, EpiResidF16{t1, C, b, nullptr}, st));
  rotate(t1);
  return LFM_OK;
}

// encoder conv_out with quant_conv folded in: in fp16 NHWC [n,H,W,512] -> moments fp32 NCHW [n,8,H,W]; w8 fp16 [8][9][512], b8 fp32 [8].  Eight live columns
// of one 128-column tile; a 128-row tile may span several images (EpiMomentsNCHW scatters per row).
static int vae_conv_moments(const half_t* in, const half_t* zeros, const void* w8, const float* b8, float* moments, int n, int H, int W, hipStream_t st) {
  const int M = n * H * W;
  return launch_gemm_tn(ASrcConv<0>{in, zeros, H, W, 512, M}, (const half_t*)w8, 9L * 512, M, 8, 9 * 512, EpiMomentsNCHW{moments, b8, H * W, 8}, st);
}

// ---- test entry points: the encoder's downsampling convolution and its last convolution, and a run of resnets of either network, on the drivers' own
// host code.  Workspace of the two convolutions: 256 B of zeros (the padding rows of the gather).
extern "C" size_t lfm_vae_downsample_workspace_bytes(int n, int Ho, int Wo, int C) {
  if (n <= 0 || Ho <= 0 || Wo <= 0 || C <= 0 || (C % 64) || 4L * n * Ho * Wo * C >= (1L << 31)) return 0;
  return vae_carve(VAE_NEED_ZEROS, nullptr, nullptr);
}

extern "C" int lfm_vae_downsample_f16(const void* x, const void* w, const float* bias, void* out, void* workspace, size_t workspace_bytes, int n, int Ho,
                                      int Wo, int C, lfm_stream_t stream) {
  if (!x || !w || !bias || !out || !workspace) return LFM_ERR_ARG;
  if (!lfm_vae_downsample_workspace_bytes(n, Ho, Wo, C)) return LFM_ERR_SHAPE;
  if (((uintptr_t)x | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 15) return LFM_ERR_ALIGN;
  VaeCtx c;
  RC(vae_setup(VAE_NEED_ZEROS, workspace, workspace_bytes, n, stream, false, c));
  c.x = (half_t*)x;  // conv_down reads x and writes t1, then rotates: the result is in `out` and nothing is written to the caller's x
  c.t1 = (half_t*)out;
  return c.conv_down(w, bias, Ho, Wo, C);
}

extern "C" size_t lfm_vae_conv_moments_workspace_bytes(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0 || (long)n * H * W * 512 >= (1L << 31)) return 0;
  return vae_carve(VAE_NEED_ZEROS, nullptr, nullptr);
}

extern "C" int lfm_vae_conv_moments_f32(const void* in, const void* w8, const float* b8, float* moments, void* workspace, size_t workspace_bytes, int n,
                                        int H, int W, lfm_stream_t stream) {
  if (!in || !w8 || !b8 || !moments || !workspace) return LFM_ERR_ARG;
  if (!lfm_vae_conv_moments_workspace_bytes(n, H, W)) return LFM_ERR_SHAPE;
  if (((uintptr_t)in | (uintptr_t)w8 | (uintptr_t)b8 | (uintptr_t)moments) & 15) return LFM_ERR_ALIGN;
  VaeCtx c;
  RC(vae_setup(VAE_NEED_ZEROS, workspace, workspace_bytes, n, stream, false, c));
  return vae_conv_moments((const half_t*)in, c.ws.zeros, w8, b8, moments, n, H, W, c.st);
}

// Workspace of the resnets: vae_need_resnets.
extern "C" size_t lfm_vae_resnets_workspace_bytes(int n, int H, int W) {
  if (n <= 0 || H <= 0 || W <= 0 || (long)n * H * W * 512 >= (1L << 31)) return 0;
  return vae_carve(vae_need_resnets(n, H * W), nullptr, nullptr);
}

extern "C" int lfm_vae_resnets_f16(const lfm_vae_resnet* r, int n_res, const void* x, void* out, void* workspace, size_t workspace_bytes, int n, int H,
                                   int W, int chain_stats, int* last_slabs, lfm_stream_t stream) {
  if (!r || !x || !out || !workspace) return LFM_ERR_ARG;
  if (n_res < 1 || n_res > 3) return LFM_ERR_SHAPE;
  uintptr_t bits = (uintptr_t)x | (uintptr_t)out;
  for (int i = 0; i < n_res; ++i) {
    const lfm_vae_resnet& q = r[i];
    if (!q.n1_g || !q.n1_b || !q.c1_w || !q.c1_b || !q.n2_g || !q.n2_b || !q.c2_w || !q.c2_b || (q.sc_w && !q.sc_b)) return LFM_ERR_ARG;
    auto width = [](int ch) { return ch == 128 || ch == 256 || ch == 512; };
    if (!width(q.cin) || !width(q.cout)) return LFM_ERR_SHAPE;
    if ((q.cin != q.cout && !q.sc_w) || (i && r[i - 1].cout != q.cin)) return LFM_ERR_SHAPE;  // the identity skip needs equal widths
    bits |= (uintptr_t)q.n1_g | (uintptr_t)q.n1_b | (uintptr_t)q.c1_w | (uintptr_t)q.c1_b | (uintptr_t)q.n2_g | (uintptr_t)q.n2_b | (uintptr_t)q.c2_w |
            (uintptr_t)q.c2_b | (uintptr_t)q.sc_w | (uintptr_t)q.sc_b;
  }
  if (!lfm_vae_resnets_workspace_bytes(n, H, W)) return LFM_ERR_SHAPE;
  if (bits & 15) return LFM_ERR_ALIGN;
  VaeCtx c;
  RC(vae_setup(vae_need_resnets(n, H * W), workspace, workspace_bytes, n, stream, chain_stats != 0, c));
  if (hipMemcpyAsync(c.x, x, (size_t)n * H * W * r[0].cin * 2, hipMemcpyDeviceToDevice, c.st) != hipSuccess) return LFM_ERR_LAUNCH;
  for (int i = 0; i < n_res; ++i) RC(c.resnet(&r[i], H, W));
  if (hipMemcpyAsync(out, c.x, (size_t)n * H * W * r[n_res - 1].cout * 2, hipMemcpyDeviceToDevice, c.st) != hipSuccess) return LFM_ERR_LAUNCH;
  if (last_slabs) *last_slabs = c.x_slabs;
  return LFM_OK;
}

// one chunk of images: x [n,3,8R,8R] -> moments [n,8,R,R]
static int vae_encode_chunk(VaeCtx& c, const lfm_vae_enc_weights* w, const float* x, float* moments, int R) {
  int H = 8 * R;
  RC(lfm_conv3x3_in_f32(x, w->cin_w, w->cin_b, c.x, c.n, H, H, 3, 128, (lfm_stream_t)c.st));
  for (int i = 0; i < 4; ++i) {
    for (int j = 0; j < 2; ++j) RC(c.resnet(&w->down[i][j], H, H));
    if (i < 3) {
      H /= 2;
      RC(c.conv_down(w->ds_w[i], w->ds_b[i], H, H, w->down[i][1].cout));
    }
  }
  RC(c.resnet(&w->mid[0], H, H));
  RC(c.mid_attention(VaeAttn{w->at_g, w->at_b, w->q_w, w->q_b, w->k_w, w->k_b, w->v_w, w->v_b, w->o_w, w->o_b}, H * H));
  RC(c.resnet(&w->mid[1], H, H));
  RC(c.gn(c.x, c.t1, w->no_g, w->no_b, H * H, 512, true, 0));
  return vae_conv_moments(c.t1, c.ws.zeros, w->cout_w, w->cout_b, moments, c.n, H, H, c.st);
}

extern "C" int lfm_vae_encode(const lfm_vae_enc_weights* w, void* workspace, size_t workspace_bytes, const float* x, float* moments, int N, int R,
                              int chunk, lfm_stream_t stream) {
  if (!w || !workspace || !x || !moments) return LFM_ERR_ARG;
  if (N <= 0 || R <= 0 || (R % 8) || chunk <= 0) return LFM_ERR_SHAPE;
  VaeCtx first;  // as in lfm_vae_decode
  RC(vae_setup(vae_need_coder(R, chunk), workspace, workspace_bytes, chunk, stream, false, first));
  for (int n0 = 0; n0 < N; n0 += chunk) {
    VaeCtx c = first;
    if (N - n0 < chunk) c.n = N - n0;
    RC(vae_encode_chunk(c, w, x + (long)n0 * 3 * 64 * R * R, moments + (long)n0 * 8 * R * R, R));
  }
  return LFM_OK;
}

// images: u8 NHWC = trunc(clamp((x + 1) / 2, 0, 1) * 255)   (test_flow_latent_ddp.py:131-135), or with ROUND the single-process
// script's torchvision.utils.save_image conversion  trunc(clamp(.., 0, 1) * 255 + 0.5)  (test_flow_latent.py:264-269,297)
template <bool ROUND>
__global__ void to_uint8_nhwc_kernel(const float* __restrict__ x, uint8_t* __restrict__ o, int HW, long total) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;  // over N*HW pixels
  if (i >= total) return;
  const long n = i / HW, p = i - n * HW;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float v = (x[(n * 3 + c) * HW + p] + 1.0f) * 0.5f;
    v = fminf(fmaxf(v, 0.f), 1.f) * 255.0f;
    if (ROUND) v = fminf(v + 0.5f, 255.0f);
    o[i * 3 + c] = (uint8_t)v;
  }
}

extern "C" int lfm_images_to_uint8_mode(const float* x, uint8_t* out, int N, int H, int W, int rounding, lfm_stream_t stream) {
  if (!x || !out) return LFM_ERR_ARG;
  if (N <= 0 || H <= 0 || W <= 0) return LFM_ERR_SHAPE;
  const long total = (long)N * H * W;
  if (rounding) hipLaunchKernelGGL(to_uint8_nhwc_kernel<true>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, H * W, total);
  else hipLaunchKernelGGL(to_uint8_nhwc_kernel<false>, dim3(cdiv(total, 256)), dim3(256), 0, (hipStream_t)stream, x, out, H * W, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}
extern "C" int lfm_images_to_uint8(const float* x, uint8_t* out, int N, int H, int W, lfm_stream_t stream) {
  return lfm_images_to_uint8_mode(x, out, N, H, W, 0, stream);
}
