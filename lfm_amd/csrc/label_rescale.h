// Conditioning stage of mask-to-image synthesis (downstream_tasks/test_flow_latent_semantic_syn.py:131-135 over models/encoder.py:90-112):
//   one_hot(labels, num_cls) -> n x F.interpolate(scale_factor=0.5, mode="bilinear") -> 1x1 channel_mapper
// as ONE gather, lfm_label_rescale_f32.  At align_corners=False a bilinear x0.5 stage is a 2x2 mean, n stages of a 0/1 map are the mean over the 2^n x 2^n
// cell, and the 1x1 convolution of that mean is, per cell,  out[o] = (sum over the cell's pixels of w[o][label(p)]) / 4^n + bias[o]:  no one-hot tensor, no
// interpolation, no GEMM; every label is read once and nothing else of any size moves.
//
// Work split.  A lane owns V adjacent pixels of a cell's row (V = 2: one 16-byte load, when the label pointer is 16-byte aligned and W is even; else V = 1) and
// walks the cell's 2^n rows; consecutive lanes take consecutive pixels of the same image row, so a wave's load is one contiguous run of up to 1 KiB per row.
// The L = 2^n / V lanes of a cell are adjacent and L-aligned in the wave (L <= 16: inside one DPP row), every workgroup keeps the weight table in the LDS
// transposed to [num_cls][Cout] (one label = Cout adjacent floats) and strides over the batch, so the table is staged a bounded number of times.
//
// Summation order (fixed: no atomics, nothing depends on the batch size, the image's place in the batch, the grid or V): per pixel column of the cell the rows
// top to bottom, then a binary tree over the cell's columns, adjacent columns first (with V = 2 its first level happens inside the lane, with V = 1 between
// lanes 2k and 2k + 1: the same two numbers added).  The tree runs on the DPP network (quad_perm, row_half_mirror, row_mirror).  The scale 1 / 4^n is a power
// of two, so one rounding remains after the sum: the bias add.
//
// A label outside [0, num_cls) reads table row 0 and flags its lane; the flag is OR-ed over the cell's lanes and the cell's Cout outputs become NaN (an
// IndexError of F.one_hot in the reference; a kernel cannot return one).  Pixels right of / below the last whole cell are never addressed.
#pragma once
#include "common.h"

typedef long long i64x2 __attribute__((ext_vector_type(2)));

template <int CTRL>
__device__ __forceinline__ int dpp_or(int v) {
  return v | __builtin_amdgcn_update_dpp(0, v, CTRL, 0xf, 0xf, false);
}

template <int COUT, int V>
__global__ __launch_bounds__(256) void label_rescale_kernel(const long long* __restrict__ labels, const float* __restrict__ w, const float* __restrict__ bias,
                                                            float* __restrict__ out, int H, int W, int h, int wo, int num_cls, int n_stages, long total) {
  extern __shared__ __attribute__((aligned(16))) float tab[];  // [num_cls][COUT]
  for (int e = threadIdx.x; e < num_cls * COUT; e += 256) {
    const int o = e / num_cls, k = e - o * num_cls;
    tab[k * COUT + o] = w[e];
  }
  __syncthreads();
  const int c = 1 << n_stages, L = c / V, lanes_x = wo * L;
  const float inv = 1.0f / (float)(1 << (2 * n_stages));
  // total is a multiple of L and every base of 256: the lanes of a cell are all inside [0, total) or all beyond it.  Lanes beyond it redo the last lane's
  // cell (every address they form is one a live lane forms) and store nothing, so the whole wave reaches the DPP steps.
  for (long base = (long)blockIdx.x * 256; base < total; base += (long)gridDim.x * 256) {
    const bool live = base + threadIdx.x < total;
    const long t = live ? base + threadIdx.x : total - 1;
    const long row = t / lanes_x;  // n * h + i
    const int lx = (int)(t - row * lanes_x);
    const long n = row / h;
    const int i = (int)(row - n * h);
    const long long* p = labels + ((n * H + (long)i * c) * W + (long)lx * V);
    float acc[V][COUT];
#pragma unroll
    for (int v = 0; v < V; ++v)
#pragma unroll
      for (int o = 0; o < COUT; ++o) acc[v][o] = 0.f;
    int bad = 0;
    for (int r = 0; r < c; r += 2) {  // two rows per trip: both loads are in flight before the first table read
      long long lab[2][V];
#pragma unroll
      for (int q = 0; q < 2; ++q) {
        const long long* pr = p + (long)(r + q) * W;
        if constexpr (V == 2) {
          const i64x2 two = *(const i64x2*)pr;
          lab[q][0] = two[0];
          lab[q][1] = two[1];
        } else {
          lab[q][0] = *pr;
        }
      }
#pragma unroll
      for (int q = 0; q < 2; ++q)
#pragma unroll
        for (int v = 0; v < V; ++v) {
          const bool ok = (unsigned long long)lab[q][v] < (unsigned long long)num_cls;
          bad |= !ok;
          const float* tr = tab + (ok ? (int)lab[q][v] : 0) * COUT;
#pragma unroll
          for (int o = 0; o < COUT; ++o) acc[v][o] += tr[o];
        }
    }
    float s[COUT];
#pragma unroll
    for (int o = 0; o < COUT; ++o) s[o] = V == 2 ? acc[0][o] + acc[V - 1][o] : acc[0][o];
    if (L > 1) {
      bad = dpp_or<0xB1>(bad);  // quad_perm [1,0,3,2]: lane ^ 1
#pragma unroll
      for (int o = 0; o < COUT; ++o) s[o] = dpp_add<0xB1>(s[o]);
    }
    if (L > 2) {
      bad = dpp_or<0x4E>(bad);  // quad_perm [2,3,0,1]: lane ^ 2
#pragma unroll
      for (int o = 0; o < COUT; ++o) s[o] = dpp_add<0x4E>(s[o]);
    }
    if (L > 4) {
      bad = dpp_or<0x141>(bad);  // row_half_mirror: the quads hold their totals, lane 7 - i is in the other quad of the 8
#pragma unroll
      for (int o = 0; o < COUT; ++o) s[o] = dpp_add<0x141>(s[o]);
    }
    if (L > 8) {
      bad = dpp_or<0x140>(bad);  // row_mirror: lane 15 - i is in the other half of the 16
#pragma unroll
      for (int o = 0; o < COUT; ++o) s[o] = dpp_add<0x140>(s[o]);
    }
    if (live && (lx & (L - 1)) == 0) {
      const int j = lx / L;
      float* po = out + ((n * COUT * h + i) * (long)wo + j);
#pragma unroll
      for (int o = 0; o < COUT; ++o) {
        const float m = s[o] * inv;
        po[(long)o * h * wo] = bad ? __builtin_nanf("") : (bias ? m + bias[o] : m);
      }
    }
  }
}

template <int COUT>
static int label_rescale_launch(const long long* labels, const float* w, const float* bias, float* out, int N, int H, int W, int num_cls, int n_stages,
                                hipStream_t stream) {
  const int h = H >> n_stages, wo = W >> n_stages;
  const bool wide = !((uintptr_t)labels & 15) && W % 2 == 0;
  const long total = (long)N * h * wo * ((1 << n_stages) / (wide ? 2 : 1));
  // at most 2048 workgroups = 8 per CU, all resident at once (256 threads, <= 64 VGPRs, tables of a few KiB): enough loads in flight to cover HBM latency, and
  // the table is staged at most 2048 times however large the batch is; beyond that the workgroups stride
  const dim3 grid((unsigned)(total + 255 < 2048L * 256 ? (total + 255) / 256 : 2048));
  const size_t lds = (size_t)num_cls * COUT * sizeof(float);
  if (wide)
    hipLaunchKernelGGL((label_rescale_kernel<COUT, 2>), grid, dim3(256), lds, stream, labels, w, bias, out, H, W, h, wo, num_cls, n_stages, total);
  else
    hipLaunchKernelGGL((label_rescale_kernel<COUT, 1>), grid, dim3(256), lds, stream, labels, w, bias, out, H, W, h, wo, num_cls, n_stages, total);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_label_rescale_f32(const void* labels_int64, const float* w, const float* bias, float* out, int N, int H, int W, int num_cls, int Cout,
                                     int n_stages, lfm_stream_t stream) {
  if (!labels_int64 || !w || !out) return LFM_ERR_ARG;
  if (N <= 0 || n_stages < 1 || n_stages > 4 || Cout < 1 || Cout > 8 || num_cls < 1 || (long)num_cls * Cout * 4 > 65536 || H < (1 << n_stages) ||
      W < (1 << n_stages))
    return LFM_ERR_SHAPE;
  if (((uintptr_t)labels_int64 & 7) || (((uintptr_t)w | (uintptr_t)bias | (uintptr_t)out) & 3)) return LFM_ERR_ALIGN;
  const long long* lab = (const long long*)labels_int64;
  hipStream_t st = (hipStream_t)stream;
  switch (Cout) {
    case 1: return label_rescale_launch<1>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    case 2: return label_rescale_launch<2>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    case 3: return label_rescale_launch<3>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    case 4: return label_rescale_launch<4>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    case 5: return label_rescale_launch<5>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    case 6: return label_rescale_launch<6>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    case 7: return label_rescale_launch<7>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
    default: return label_rescale_launch<8>(lab, w, bias, out, N, H, W, num_cls, n_stages, st);
  }
}
