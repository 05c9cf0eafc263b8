// DiT device kernels around the MFMA GEMMs and the attention kernels (included by dit.hip, the only translation unit that uses them).
#pragma once

// ------------------------------------------------------------------ timestep embedder (DiT.py:29-69)
// temb[r] = W2 * silu(W0 * [cos(t f) | sin(t f)] + b0) + b2, fp32 throughout; one wave per output element.
__global__ __launch_bounds__(256) void temb1_kernel(const float* __restrict__ t, const float* __restrict__ w0, const float* __restrict__ b0,
                                                    float* __restrict__ h1, int D) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= D) return;
  const float tv = t[r];
  const float* w = w0 + (long)j * 256;
  float s = 0.f;
#pragma unroll
  for (int k = lane; k < 256; k += 64) {
    const int i = k & 127;
    const float a = tv * expf(-9.210340371976184f * (float)i / 128.0f);  // t * exp(-ln(1e4) i/half)
    s += w[k] * (k < 128 ? cosf(a) : sinf(a));
  }
  s = wave_sum(s);
  if (lane == 0) h1[(long)r * D + j] = silu_f(s + b0[j]);
}
__global__ __launch_bounds__(256) void temb2_kernel(const float* __restrict__ h1, const float* __restrict__ w2, const float* __restrict__ b2,
                                                    float* __restrict__ temb, int D) {
  const int r = blockIdx.y, lane = threadIdx.x & 63;
  const int j = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (j >= D) return;
  const float* w = w2 + (long)j * D;
  const float* h = h1 + (long)r * D;
  float s = 0.f;
  for (int k = lane; k < D; k += 64) s += w[k] * h[k];
  s = wave_sum(s);
  if (lane == 0) temb[(long)r * D + j] = s + b2[j];
}

// c_half[r] = fp16(silu(temb[t_len==1 ? 0 : r] + y_table[y ? y[r] : null_row]))   (DiT.py:259-264 + the SiLU of :125)
// A label outside [0, label_rows) is an IndexError in the reference (nn.Embedding); a kernel inside a captured graph cannot raise,
// so the row is POISONED with NaN instead of reading out of bounds (the host wrapper validates labels before they get here).
__global__ void cond_kernel(const float* __restrict__ temb, int t_len, const float* __restrict__ y_table, const int64_t* __restrict__ y,
                            int label_rows, half_t* __restrict__ c_half, int D, int rows) {
  const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (long)rows * D) return;
  const int r = (int)(i / D), j = (int)(i - (long)r * D);
  const long yr = y ? (long)y[r] : (long)(label_rows - 1);
  if (yr < 0 || yr >= label_rows) {
    c_half[i] = (half_t)__builtin_nanf("");
    return;
  }
  const float v = temb[(t_len == 1 ? 0 : (long)r * D) + j] + y_table[yr * D + j];
  c_half[i] = (half_t)silu_f(v);
}

// ------------------------------------------------------------------ patch embed (timm PatchEmbed + pos_embed, DiT.py:179,261)
// X[n*T + tok][j] = b[j] + pos[tok][j] + sum_{c,p,q} W[j][c][p][q] * x[n % xmod][c][hp+p][wp+q]
// blockDim = D/4 threads, thread = 4 consecutive output channels whose weight rows stay in registers (KK <= 16 here);
// a block walks PE_TOK tokens, whose KK input values are wave-uniform loads.
#define PE_TOK 16
#define PE_MAXK 16
__global__ __launch_bounds__(320) void patch_embed_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                          const float* __restrict__ pos, float* __restrict__ X, int M, int xmod, int C, int R,
                                                          int p, int D) {
  __shared__ float xs[PE_TOK][PE_MAXK];
  const int grid = R / p, T = grid * grid, KK = C * p * p;
  const long m_begin = (long)blockIdx.x * PE_TOK;
  for (int e = threadIdx.x; e < PE_TOK * PE_MAXK; e += blockDim.x) {  // stage the inputs: the token loop has no dependent global loads
    const int tt = e / PE_MAXK, k = e % PE_MAXK;
    const long m = m_begin + tt;
    float v = 0.f;
    if (m < M && k < KK) {
      const int tok = (int)(m % T), n = (int)(m / T) % xmod;
      const int c = k / (p * p), pp = (k / p) % p, q = k % p;
      v = x[(((long)n * C + c) * R + (tok / grid) * p + pp) * R + (tok % grid) * p + q];
    }
    xs[tt][k] = v;
  }
  const int j = threadIdx.x * 4;
  float wr[4][PE_MAXK];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int k = 0; k < PE_MAXK; ++k) wr[i][k] = (k < KK) ? w[(long)(j + i) * KK + k] : 0.f;
  const f32x4 bias = *(const f32x4*)(b + j);
  // every position-embedding row of the block's tokens is fetched BEFORE the first store: vmcnt counts stores too and returns in order, so a
  // load issued behind a store waits for that store's round trip (58 us per launch with the load inside the token loop)
  f32x4 pv[PE_TOK];
#pragma unroll
  for (int tt = 0; tt < PE_TOK; ++tt) {
    const long m = (m_begin + tt < M) ? m_begin + tt : M - 1;
    pv[tt] = *(const f32x4*)(pos + (long)(m % T) * D + j);
  }
  __syncthreads();
#pragma unroll
  for (int tt = 0; tt < PE_TOK; ++tt) {
    const long m = m_begin + tt;
    if (m >= M) break;
    f32x4 acc = bias + pv[tt];
#pragma unroll
    for (int k = 0; k < PE_MAXK; ++k) {
      const float xv = xs[tt][k];
      acc.x += wr[0][k] * xv;
      acc.y += wr[1][k] * xv;
      acc.z += wr[2][k] * xv;
      acc.w += wr[3][k] * xv;
    }
    *(f32x4*)(X + m * D + j) = acc;
  }
}

// Round 3: the patch embedding of the */2 models (K = p*p*C = 16) on v_mfma_f32_16x16x16_f16, fused with the FIRST LayerNorm of the forward.
// patch_embed_kernel above spends its time on 256 LDS broadcast reads and 1024 scalar FMAs per thread (55 us for 67 MB); the LayerNorm after it
// re-read the 67 MB it had just written (ln_center_mod_kernel / ln_modulate, 17-20 us).  Here a block of D / 256 waves walks 16-token tiles; wave w
// owns channels 256 w .. + 255 with its weight fragments (fp16 hi + lo, three MFMAs per tile pair = the fp32 dot product to 2^-22) and bias rows
// resident in registers.  The W rows of a 32-channel pair are fed through the permutation n = 8 (a >> 2) + 4 e + (a & 3) (a = fragment row, e = which
// MFMA of the pair), so a lane ends up with EIGHT CONSECUTIVE channels of one token: X leaves as 2 x 16-byte stores (four lanes = one 128-byte
// line), the fp16 operand of the first qkv GEMM as one.  The row statistics are in-lane sums + two lane exchanges + one LDS hand-over between the
// waves; the variance is the exact two-pass one (the values stay in registers).  With A == nullptr only X is written.
__global__ __launch_bounds__(320) void patch_embed_ln_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b,
                                                             const float* __restrict__ pos, float* __restrict__ X, int M, int xmod, int R, int D,
                                                             int tiles_per_block, half_t* __restrict__ A, const float* __restrict__ scale,
                                                             long mod_stride, float* __restrict__ part, int tiles_p, float* __restrict__ cen) {
  typedef half_t half4v __attribute__((ext_vector_type(4)));
  __shared__ float red[2][5][16];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, a = lane & 15, q = lane >> 4;
  const int grid = R >> 1, T = grid * grid;
  // resident weight fragments and bias rows of this wave's 8 channel pairs
  half4v wh[8][2], wl[8][2];
  f32x4 bias[8][2];
#pragma unroll
  for (int pr = 0; pr < 8; ++pr)
#pragma unroll
    for (int e = 0; e < 2; ++e) {
      const int n = 256 * wv + 32 * pr + 8 * (a >> 2) + 4 * e + (a & 3);  // the W row this lane feeds as fragment row a
      const f32x4 wf = *(const f32x4*)(w + (long)n * 16 + 4 * q);
      const float wa[4] = {wf.x, wf.y, wf.z, wf.w};
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        wh[pr][e][i] = (half_t)wa[i];
        wl[pr][e][i] = (half_t)(wa[i] - (float)wh[pr][e][i]);
      }
      bias[pr][e] = *(const f32x4*)(b + 256 * wv + 32 * pr + 8 * q + 4 * e);  // the channels this lane OWNS in the result
    }
  for (int it = 0; it < tiles_per_block; ++it) {
    const long tile = (long)blockIdx.x * tiles_per_block + it;
    if (tile * 16 >= M) break;  // (whole block)
    const long m = tile * 16 + a < M ? tile * 16 + a : M - 1;
    const int tok = (int)(m % T), n_img = (int)(m / T) % xmod;
    // the token's patch values k = 4 q .. 4 q + 3 = channel q, 2 x 2 pixels
    const float* xp = x + (((long)n_img * 4 + q) * R + (tok / grid) * 2) * R + (tok % grid) * 2;
    const f32x2 r0 = *(const f32x2*)xp, r1 = *(const f32x2*)(xp + R);
    const float xa[4] = {r0.x, r0.y, r1.x, r1.y};
    half4v xh, xl;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      xh[i] = (half_t)xa[i];
      xl[i] = (half_t)(xa[i] - (float)xh[i]);
    }
    f32x4 val[8][2];
    float sx = 0.f;
    const float* prow = pos + (long)tok * D + 256 * wv + 8 * q;
    float* xrow = X + m * D + 256 * wv + 8 * q;
    const bool live = tile * 16 + a < M;
#pragma unroll
    for (int pr = 0; pr < 8; ++pr)
#pragma unroll
      for (int e = 0; e < 2; ++e) {
        f32x4_t acc = {0.f, 0.f, 0.f, 0.f};
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(wh[pr][e], xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(wl[pr][e], xh, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f32_16x16x16f16(wh[pr][e], xl, acc, 0, 0, 0);
        const f32x4 v = (f32x4){acc[0], acc[1], acc[2], acc[3]} + bias[pr][e] + *(const f32x4*)(prow + 32 * pr + 4 * e);
        val[pr][e] = v;
        if (live) *(f32x4*)(xrow + 32 * pr + 4 * e) = v;
        sx += (v.x + v.y) + (v.z + v.w);
      }
    if (!A) continue;
    sx += __shfl_xor(sx, 16, 64);
    sx += __shfl_xor(sx, 32, 64);
    if (q == 0) red[0][wv][a] = sx;
    __syncthreads();
    float sum = 0.f;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) sum += red[0][i][a];
    const float mean = sum / (float)D;
    const float* srow = scale + (m / T) * mod_stride + 256 * wv + 8 * q;
    half_t* arow = A + m * D + 256 * wv + 8 * q;
    float sq = 0.f;
#pragma unroll
    for (int pr = 0; pr < 8; ++pr) {
      const f32x4 d0 = val[pr][0] - mean, d1 = val[pr][1] - mean;
      sq += (d0.x * d0.x + d0.y * d0.y) + (d0.z * d0.z + d0.w * d0.w) + (d1.x * d1.x + d1.y * d1.y) + (d1.z * d1.z + d1.w * d1.w);
      const f32x4 o0 = d0 * (1.0f + *(const f32x4*)(srow + 32 * pr)), o1 = d1 * (1.0f + *(const f32x4*)(srow + 32 * pr + 4));
      const half8_t h = {(half_t)o0.x, (half_t)o0.y, (half_t)o0.z, (half_t)o0.w, (half_t)o1.x, (half_t)o1.y, (half_t)o1.z, (half_t)o1.w};
      if (live) *(half8_t*)(arow + 32 * pr) = h;
    }
    sq += __shfl_xor(sq, 16, 64);
    sq += __shfl_xor(sq, 32, 64);
    if (q == 0) red[1][wv][a] = sq;
    __syncthreads();
    if (wv == 0 && q == 0 && live) {
      float qs = 0.f;
      for (int i = 0; i < (int)(blockDim.x >> 6); ++i) qs += red[1][i][a];
      float* pp = part + m * tiles_p * 2;
      pp[0] = sum;
      pp[1] = qs;
      for (int t2 = 1; t2 < tiles_p; ++t2) {
        pp[2 * t2] = 0.f;
        pp[2 * t2 + 1] = 0.f;
      }
      cen[m] = mean;
    }
  }
}

// Patch sizes with p*p*C > 16 (DiT-*/4, */8): the patch embedding is a real GEMM (K = p*p*C = 64 / 256).  This kernel gathers the patches
// into the fp16 A operand Ap[m][k], k = (c, pp, q) as x_embedder.proj.weight flattens, and pre-fills the residual stream with the
// position embedding; the GEMM then adds  1 * (patches W^T + bias)  through the gated-residual epilogue (gate = a row of ones).
__global__ __launch_bounds__(256) void patchify_kernel(const float* __restrict__ x, const float* __restrict__ pos, half_t* __restrict__ Ap,
                                                       float* __restrict__ X, float* __restrict__ ones, int M, int xmod, int C, int R, int p, int D) {
  const int grid = R / p, T = grid * grid, KK = C * p * p;
  const long m = blockIdx.x;
  const int tok = (int)(m % T), n = (int)(m / T) % xmod;
  for (int k = threadIdx.x; k < KK; k += 256) {
    const int c = k / (p * p), pp = (k / p) % p, q = k % p;
    Ap[m * KK + k] = (half_t)x[(((long)n * C + c) * R + (tok / grid) * p + pp) * R + (tok % grid) * p + q];
  }
  for (int j = threadIdx.x; j < D; j += 256) X[m * D + j] = pos[(long)tok * D + j];
  if (m == 0)
    for (int j = threadIdx.x; j < D; j += 256) ones[j] = 1.0f;
}

// ------------------------------------------------------------------ LayerNorm + modulate -> fp16 (DiT.py:20-21,119,129-130)
// one wave per token row; the row stays in registers (<= 5 float4 per lane => D <= 1280).
#define LN_MAXV 5
#define LN_ROWS 2  // rows per wave: both rows' loads are issued before either reduction, doubling the bytes in flight per wave
__global__ __launch_bounds__(256) void ln_modulate_kernel(const float* __restrict__ X, half_t* __restrict__ A, int M, int D, int tokens,
                                                          const float* __restrict__ shift, const float* __restrict__ scale, long mod_stride) {
  const int lane = threadIdx.x & 63;
  const long m0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * LN_ROWS;
  if (m0 >= M) return;
  const int nv = D >> 2;
  f32x4 v[LN_ROWS][LN_MAXV];
  float s[LN_ROWS];
#pragma unroll
  for (int r = 0; r < LN_ROWS; ++r) {
    const long m = (m0 + r < M) ? m0 + r : M - 1;
    const f32x4* xr = (const f32x4*)(X + m * D);
    s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) {
        v[r][i] = xr[c];
        s[r] += v[r][i].x + v[r][i].y + v[r][i].z + v[r][i].w;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < LN_ROWS; ++r) {
    const long m = m0 + r;
    if (m >= M) break;
    const float mean = wave_sum(s[r]) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) {
        v[r][i] -= mean;
        q += v[r][i].x * v[r][i].x + v[r][i].y * v[r][i].y + v[r][i].z * v[r][i].z + v[r][i].w * v[r][i].w;
      }
    }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + 1e-6f);
    const long mo = (m / tokens) * mod_stride;
    const f32x4* sh = (const f32x4*)(shift + mo);
    const f32x4* sc = (const f32x4*)(scale + mo);
    half4_t* ar = (half4_t*)(A + m * D);
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) {
        const f32x4 o = v[r][i] * rstd * (1.0f + sc[c]) + sh[c];
        half4_t h = {(half_t)o.x, (half_t)o.y, (half_t)o.z, (half_t)o.w};
        ar[c] = h;
      }
    }
  }
}

// Same computation with 16-byte stores: lane l owns EIGHT consecutive columns 8 (l + 64 i) .. + 7 (two adjacent float4 loads), so a row
// of the fp16 output goes out as 16 B per lane instead of 8 (the GEMM epilogues gained 3-4 % from the same change).  D % 8 == 0.
#define LN_MAXP 3  // column octets per lane: D <= 1536
// NR = rows per wave, DPP = row sums on the DPP cross-lane network instead of ds_bpermute (<1, true> ships; the others are A/B variants)
template <int NR, bool DPP = false>
__global__ __launch_bounds__(256) void ln_modulate8_kernel(const float* __restrict__ X, half_t* __restrict__ A, int M, int D, int tokens,
                                                           const float* __restrict__ shift, const float* __restrict__ scale, long mod_stride) {
  const int lane = threadIdx.x & 63;
  const long m0 = ((long)blockIdx.x * 4 + (threadIdx.x >> 6)) * NR;
  if (m0 >= M) return;
  const int np = D >> 3;
  f32x4 v[NR][LN_MAXP][2];
  float s[NR];
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const long m = (m0 + r < M) ? m0 + r : M - 1;
    const f32x4* xr = (const f32x4*)(X + m * D);
    s[r] = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXP; ++i) {
      const int c = lane + 64 * i;
      if (c < np) {
        v[r][i][0] = xr[2 * c];
        v[r][i][1] = xr[2 * c + 1];
        const f32x4 t = v[r][i][0] + v[r][i][1];
        s[r] += (t.x + t.y) + (t.z + t.w);
      }
    }
  }
#pragma unroll
  for (int r = 0; r < NR; ++r) {
    const long m = m0 + r;
    if (m >= M) break;
    const float mean = (DPP ? wave_sum_dpp(s[r]) : wave_sum(s[r])) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXP; ++i) {
      if (lane + 64 * i < np) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          v[r][i][h] -= mean;
          const f32x4 t = v[r][i][h] * v[r][i][h];
          q += (t.x + t.y) + (t.z + t.w);
        }
      }
    }
    const float rstd = rsqrtf((DPP ? wave_sum_dpp(q) : wave_sum(q)) / (float)D + 1e-6f);
    const long mo = (m / tokens) * mod_stride;
    const f32x4* sh = (const f32x4*)(shift + mo);
    const f32x4* sc = (const f32x4*)(scale + mo);
    half8_t* ar = (half8_t*)(A + m * D);
#pragma unroll
    for (int i = 0; i < LN_MAXP; ++i) {
      const int c = lane + 64 * i;
      if (c < np) {
        const f32x4 lo = v[r][i][0] * rstd * (1.0f + sc[2 * c]) + sh[2 * c];
        const f32x4 hi = v[r][i][1] * rstd * (1.0f + sc[2 * c + 1]) + sh[2 * c + 1];
        half8_t h = {(half_t)lo.x, (half_t)lo.y, (half_t)lo.z, (half_t)lo.w, (half_t)hi.x, (half_t)hi.y, (half_t)hi.z, (half_t)hi.w};
        ar[c] = h;
      }
    }
  }
}

// Folded LayerNorm-modulate (gemm_epilogues.h, "adaLN LayerNorm-modulate FOLDED into the GEMM epilogues"): the FIRST LayerNorm of a forward has no
// producer GEMM in front of it (x comes from the patch embedding), so this kernel plays the producer: A' = fp16((x - mu)(1 + scale)) with the exact
// row mean as the centring constant, partial slot 0 = (sum x, sum (x - mu)^2), the other slots 0, cen[m] = mu.  One row per wave, DPP sums.
__global__ __launch_bounds__(256) void ln_center_mod_kernel(const float* __restrict__ X, half_t* __restrict__ A, int M, int D, int tokens,
                                                            const float* __restrict__ scale, long mod_stride, float* __restrict__ part, int tiles_p,
                                                            float* __restrict__ cen) {
  const int lane = threadIdx.x & 63;
  const long m = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= M) return;
  const int np = D >> 3;
  f32x4 v[LN_MAXP][2];
  const f32x4* xr = (const f32x4*)(X + m * D);
  float s = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXP; ++i) {
    const int c = lane + 64 * i;
    if (c < np) {
      v[i][0] = xr[2 * c];
      v[i][1] = xr[2 * c + 1];
      const f32x4 t = v[i][0] + v[i][1];
      s += (t.x + t.y) + (t.z + t.w);
    }
  }
  const float sum = wave_sum_dpp(s), mean = sum / (float)D;
  float q = 0.f;
#pragma unroll
  for (int i = 0; i < LN_MAXP; ++i) {
    if (lane + 64 * i < np) {
#pragma unroll
      for (int h = 0; h < 2; ++h) {
        v[i][h] -= mean;
        const f32x4 t = v[i][h] * v[i][h];
        q += (t.x + t.y) + (t.z + t.w);
      }
    }
  }
  const float qs = wave_sum_dpp(q);
  const f32x4* sc = (const f32x4*)(scale + (m / tokens) * mod_stride);
  half8_t* ar = (half8_t*)(A + m * D);
#pragma unroll
  for (int i = 0; i < LN_MAXP; ++i) {
    const int c = lane + 64 * i;
    if (c < np) {
      const f32x4 lo = v[i][0] * (1.0f + sc[2 * c]), hi = v[i][1] * (1.0f + sc[2 * c + 1]);
      half8_t h = {(half_t)lo.x, (half_t)lo.y, (half_t)lo.z, (half_t)lo.w, (half_t)hi.x, (half_t)hi.y, (half_t)hi.z, (half_t)hi.w};
      ar[c] = h;
    }
  }
  if (lane < tiles_p) *(f32x2*)(part + (m * tiles_p + lane) * 2) = lane == 0 ? (f32x2){sum, qs} : (f32x2){0.f, 0.f};
  if (lane == 0) cen[m] = mean;
}

// A operand of the u / v GEMMs of the folded path: for block i and branch b (0 = msa, 1 = mlp) rows [0, R) = fp16(1 + scale), rows [R, 2R) = fp16(shift);
// Amod[((i * 2 + b) * 2 + h) * R + r][k].  (u only ever multiplies rstd (mu - c), a small correction, and v takes the place of a term that used
// to be rounded to fp16 inside the LN output anyway: fp16 operands cost nothing here.)
__global__ __launch_bounds__(256) void mod_rows_f16_kernel(const float* __restrict__ mod, long mod_stride, int depth, int R, int D,
                                                           half_t* __restrict__ Amod) {
  const long idx = (long)blockIdx.x * 256 + threadIdx.x;  // over depth * 2 * 2 * R * D / 4
  const int d4 = D >> 2;
  const long total = (long)depth * 4 * R * d4;
  if (idx >= total) return;
  const int k = (int)(idx % d4) * 4;
  long t = idx / d4;
  const int r = (int)(t % R);
  t /= R;
  const int h = (int)(t & 1), b = (int)((t >> 1) & 1), i = (int)(t >> 2);
  const float* src = mod + (long)r * mod_stride + (long)i * 6 * D + (b ? 3 * D : 0) + (h ? 0 : D) + k;  // h = 0: scale (+ 1), h = 1: shift
  f32x4 v = *(const f32x4*)src;
  if (!h) v += 1.0f;
  half4_t o = {(half_t)v.x, (half_t)v.y, (half_t)v.z, (half_t)v.w};
  *(half4_t*)(Amod + idx * 4) = o;
}

// u / v rows of the folded path when ONE conditioning row serves the whole batch (scalar time, no labels): a GEMV pair per weight row,
//   u[n] = sum_k (1 + scale[k]) W[n][k],   v[n] = sum_k shift[k] W[n][k] + bias[n],
// streamed straight from the fp16 weights with the fp32 modulation vectors in registers (no fp16 rounding of them at all).  One wave = eight
// weight rows (sixteen 16-byte loads in flight per lane); grid.y = block index.  This is pure weight streaming (352 MB per DiT-L/2 forward):
// the batched 128x128 MFMA GEMM it replaces for this case moved the same bytes at 4 TB/s with 126 of its 128 tile rows padding.
#define UV_ROWS 8
__global__ __launch_bounds__(256) void uv_gemv_kernel(const half_t* __restrict__ W, const float* __restrict__ bias, const float* __restrict__ mod,
                                                      int N, int D, int scale_off, int shift_off, float* __restrict__ out) {
  const int lane = threadIdx.x & 63, i = blockIdx.y;
  const int n0 = (blockIdx.x * 4 + (threadIdx.x >> 6)) * UV_ROWS;
  if (n0 >= N) return;
  const int nch = D >> 3;  // 16-byte chunks per row
  const float* sc = mod + (long)i * 6 * D + scale_off;
  const float* sh = mod + (long)i * 6 * D + shift_off;
  f32x4 au[LN_MAXP][2], av[LN_MAXP][2];
#pragma unroll
  for (int j = 0; j < LN_MAXP; ++j) {
    const int c = lane + 64 * j;
    if (c < nch) {
      au[j][0] = *(const f32x4*)(sc + 8 * c) + 1.0f;
      au[j][1] = *(const f32x4*)(sc + 8 * c + 4) + 1.0f;
      av[j][0] = *(const f32x4*)(sh + 8 * c);
      av[j][1] = *(const f32x4*)(sh + 8 * c + 4);
    }
  }
  const half_t* wb = W + ((long)i * N + n0) * D;
  half8_t wv[UV_ROWS][LN_MAXP];
#pragma unroll
  for (int r = 0; r < UV_ROWS; ++r)
#pragma unroll
    for (int j = 0; j < LN_MAXP; ++j) {
      const int c = lane + 64 * j;
      if (c < nch && n0 + r < N) wv[r][j] = *(const half8_t*)(wb + (long)r * D + 8 * c);
    }
  float* ob = out + (long)i * 2 * N;
#pragma unroll
  for (int r = 0; r < UV_ROWS; ++r) {
    float u = 0.f, v = 0.f;
#pragma unroll
    for (int j = 0; j < LN_MAXP; ++j) {
      if (lane + 64 * j < nch && n0 + r < N) {
        const half8_t h = wv[r][j];
        const f32x4 w0 = {(float)h[0], (float)h[1], (float)h[2], (float)h[3]}, w1 = {(float)h[4], (float)h[5], (float)h[6], (float)h[7]};
        const f32x4 pu = au[j][0] * w0 + au[j][1] * w1, pv = av[j][0] * w0 + av[j][1] * w1;
        u += (pu.x + pu.y) + (pu.z + pu.w);
        v += (pv.x + pv.y) + (pv.z + pv.w);
      }
    }
    u = wave_sum_dpp(u);
    v = wave_sum_dpp(v);
    if (lane == 0 && n0 + r < N) {
      ob[n0 + r] = u;
      ob[N + n0 + r] = v + bias[(long)i * N + n0 + r];
    }
  }
}

// ------------------------------------------------------------------ final layer + unpatchify + solver update
// (DiT.py:134-149,230-243,270-271; CFG combine :285-287; Euler update test_flow_latent.py:61-73 via torchdiffeq)
// out[n][c][hp+p][wp+q] = base + dt * v,  v = linear(modulate(LN(x)))[(p*P+q)*C + c].
// One wave owns FOUR token rows (under CFG: two conditional tokens and their two unconditional twins), so every row of the
// output matrix Wf is fetched once per four tokens; the 4 x 16 per-lane partial dot products are then reduced with a 6-step
// butterfly reduce-scatter (63 exchanges) that leaves lane l with the finished value of (row l>>4, output l&15).
#define FIN_MAXO 256  // outputs per token p*p*C, processed 16 per pass
template <bool CFG>
__global__ __launch_bounds__(256) void final_layer_kernel(const float* __restrict__ X, int M, int D, int tokens, const float* __restrict__ shift,
                                                          const float* __restrict__ scale, long mod_stride, const float* __restrict__ Wf,
                                                          const float* __restrict__ bf, int C, int R, int p, float cfg_scale,
                                                          float* out, const float* base, const float* __restrict__ dt_ptr) {
  const int lane = threadIdx.x & 63;
  const long wg = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  const int Mh = CFG ? M / 2 : M;
  const long mfirst = CFG ? wg * 2 : wg * 4;
  if (mfirst >= Mh) return;
  const int nv = D >> 2, NO = p * p * C;
  long mrow[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    long m = CFG ? mfirst + (r & 1) + (long)(r >> 1) * Mh : mfirst + r;
    mrow[r] = m < M ? m : M - 1;
  }
  f32x4 v[4][LN_MAXV];
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const f32x4* xr = (const f32x4*)(X + mrow[r] * D);
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) v[r][i] = xr[c];
    }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i)
      if (lane + 64 * i < nv) s += v[r][i].x + v[r][i].y + v[r][i].z + v[r][i].w;
    const float mean = wave_sum(s) / (float)D;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i)
      if (lane + 64 * i < nv) {
        v[r][i] -= mean;
        q += v[r][i].x * v[r][i].x + v[r][i].y * v[r][i].y + v[r][i].z * v[r][i].z + v[r][i].w * v[r][i].w;
      }
    const float rstd = rsqrtf(wave_sum(q) / (float)D + 1e-6f);
    const long mo = (mrow[r] / tokens) * mod_stride;
    const f32x4* sh = (const f32x4*)(shift + mo);
    const f32x4* sc = (const f32x4*)(scale + mo);
#pragma unroll
    for (int i = 0; i < LN_MAXV; ++i) {
      const int c = lane + 64 * i;
      if (c < nv) v[r][i] = v[r][i] * rstd * (1.0f + sc[c]) + sh[c];
    }
  }
  const int r = lane >> 4, ol = lane & 15;
  const long m = CFG ? mfirst + (r & 1) + (long)(r >> 1) * Mh : mfirst + r;
  for (int o0 = 0; o0 < NO; o0 += 16) {  // 16 outputs per pass: p*p*C = 16 (patch 2) is one pass, 64 / 256 (patch 4 / 8) four / sixteen
    float part[64];  // [r][o]
#pragma unroll
    for (int o = 0; o < 16; ++o) {
      f32x4 w4[LN_MAXV];
#pragma unroll
      for (int i = 0; i < LN_MAXV; ++i) {
        const int c = lane + 64 * i;
        w4[i] = (o0 + o < NO && c < nv) ? ((const f32x4*)(Wf + (long)(o0 + o) * D))[c] : (f32x4){0.f, 0.f, 0.f, 0.f};
      }
#pragma unroll
      for (int rr = 0; rr < 4; ++rr) {
        float a = 0.f;
#pragma unroll
        for (int i = 0; i < LN_MAXV; ++i)
          if (lane + 64 * i < nv) a += v[rr][i].x * w4[i].x + v[rr][i].y * w4[i].y + v[rr][i].z * w4[i].z + v[rr][i].w * w4[i].w;
        part[rr * 16 + o] = a;
      }
    }
    // reduce-scatter: at step s the lane bit (32 >> s) picks the upper/lower half of the remaining index range
#pragma unroll
    for (int s = 0; s < 6; ++s) {
      const int half_w = 32 >> s, mask = 32 >> s;
      const bool upper = (lane & mask) != 0;
#pragma unroll
      for (int k = 0; k < half_w; ++k) {
        const float keep = upper ? part[k + half_w] : part[k];
        const float send = upper ? part[k] : part[k + half_w];
        part[k] = keep + __shfl_xor(send, mask, 64);
      }
    }
    const int o = o0 + ol;
    float val = part[0] + (o < NO ? bf[o] : 0.f);
    if (CFG) {  // rows 0,1 conditional, rows 2,3 their unconditional twins: lane ^ 32 holds the twin's value
      const float other = xhalf(val);
      const float cond = r < 2 ? val : other, uncond = r < 2 ? other : val;
      val = uncond + cfg_scale * (cond - uncond);
    }
    if (o < NO && m < M && (CFG || m < Mh)) {
      const int grid = R / p;
      const int n = (int)(m / tokens), tok = (int)(m % tokens);
      const int pp = o / (p * C), qq = (o / C) % p, c = o % C;
      const long off = (((long)n * C + c) * R + (tok / grid) * p + pp) * R + (tok % grid) * p + qq;
      if (base) out[off] = base[off] + (*dt_ptr) * val;
      else out[off] = val;
    }
  }
}

// Round 3: the same layer as a skinny MFMA GEMM.  final_layer_kernel above keeps four whole rows per wave in registers (434+ VGPRs: one wave per SIMD)
// and reduces 64 partial dot products through 63 ds_bpermute exchanges: 64 us for 67 MB = 1.0 TB/s.  Here one wave owns SIXTEEN token rows as ONE
// v_mfma_f32_16x16x32_f16 row tile and N = p*p*C / 16 column tiles; K = D is walked in 32-deep steps with the operands built in registers in the
// MFMA fragment layout (lane l: row l & 15, eight consecutive k at 8 (l >> 4)), so
//   * the LayerNorm statistics are in-lane (count, mean, M2) merges plus two lane exchanges (the four lanes l, l^16, l^32, l^48 share a row);
//   * X is streamed twice (statistics, then operands): the second pass hits the L2 (64 KiB per wave), HBM sees the 67 MB once;
//   * fp32 fidelity on an fp16 matrix core: activation and weight are each split into fp16 hi + lo and three MFMAs (hi*hi + lo*hi + hi*lo)
//     accumulate in fp32 -- the dropped lo*lo term is 2^-22 relative, i.e. the result is the fp32 dot product to rounding, as before.
// Under CFG a tile holds eight conditional rows and their eight unconditional twins, which land in lanes l and l ^ 32 of the result.
// (D % 32 == 0: the four waves of a block take the 32-deep k-steps round-robin; with D % 128 != 0 they hold unequal numbers of them, at D = 64 two hold none.)
template <bool CFG, int NT>
__global__ __launch_bounds__(256) void final_layer_mfma_kernel(const float* __restrict__ X, int M, int D, int tokens, const float* __restrict__ shift,
                                                               const float* __restrict__ scale, long mod_stride, const float* __restrict__ Wf,
                                                               const float* __restrict__ bf, int C, int R, int p, float cfg_scale, float* out,
                                                               const float* base, const float* __restrict__ dt_ptr) {
  // one BLOCK per 16-row tile; its four waves split K (k-steps wv, wv + 4, ...) so that sixteen waves per CU cover the memory latency, and
  // combine their partial statistics / partial accumulators through the LDS in a fixed order
  __shared__ float st_s[4][16][3];
  __shared__ float acc_s[4][NT][64][4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, a = lane & 15, q = lane >> 4;
  const long tile = blockIdx.x;
  const int Mh = CFG ? M / 2 : M;
  const long m = CFG ? tile * 8 + (a & 7) + (a >> 3) * (long)Mh : tile * 16 + a;  // this lane's operand row
  const float* xr = X + m * D + 8 * q;
  const int nks = D >> 5;
  // ---- pass 1: centred statistics in one pass over X.  Every eight-value chunk gives its own mean and its sum of squares ABOUT that mean (the values are
  // in registers); chunks, lanes and waves are merged as (count, mean, M2) triples, M2 += M2' + (mean' - mean)^2 n n' / (n + n').  Every term is
  // non-negative, so nothing cancels wherever an outlier channel sits.
  float cn = 0.f, mu = 0.f, m2 = 0.f;
#pragma unroll 4
  for (int ks = wv; ks < nks; ks += 4) {
    const f32x4 x0 = *(const f32x4*)(xr + 32 * ks), x1 = *(const f32x4*)(xr + 32 * ks + 4);
    const float m8 = (((x0.x + x0.y) + (x0.z + x0.w)) + ((x1.x + x1.y) + (x1.z + x1.w))) * 0.125f;
    const f32x4 d0 = x0 - m8, d1 = x1 - m8;
    const float q8 = ((d0.x * d0.x + d0.y * d0.y) + (d0.z * d0.z + d0.w * d0.w)) + ((d1.x * d1.x + d1.y * d1.y) + (d1.z * d1.z + d1.w * d1.w));
    const float dl = m8 - mu, nn = cn + 8.f, f = 8.f / nn;
    mu += dl * f;
    m2 += q8 + dl * dl * (cn * f);
    cn = nn;
  }
#pragma unroll
  for (int mask = 16; mask <= 32; mask <<= 1) {  // the four lanes of a row hold equal counts
    const float dl = __shfl_xor(mu, mask, 64) - mu;
    m2 = (m2 + __shfl_xor(m2, mask, 64)) + dl * dl * (0.5f * cn);
    mu += 0.5f * dl;
    cn += cn;
  }
  if (q == 0) {
    st_s[wv][a][0] = cn;
    st_s[wv][a][1] = mu;
    st_s[wv][a][2] = m2;
  }
  __syncthreads();
  cn = st_s[0][a][0], mu = st_s[0][a][1], m2 = st_s[0][a][2];  // wave 0 always has a k-step; the others may hold fewer (D % 128 != 0) or none (D = 64)
#pragma unroll
  for (int w = 1; w < 4; ++w) {
    const float nb = st_s[w][a][0], dl = st_s[w][a][1] - mu, nn = cn + nb, f = nb / nn;
    mu += dl * f;
    m2 += st_s[w][a][2] + dl * dl * (cn * f);
    cn = nn;
  }
  const float mean = mu;
  const float rstd = rsqrtf(m2 / (float)D + 1e-6f);
  const long mo = (m / tokens) * mod_stride + 8 * q;
  // ---- pass 2: operands + MFMAs (X again, now from the L2)
  f32x4_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = (f32x4_t){0.f, 0.f, 0.f, 0.f};
  auto split = [](const f32x4& lo4, const f32x4& hi4, half8_t& h, half8_t& l) {
    const float v[8] = {lo4.x, lo4.y, lo4.z, lo4.w, hi4.x, hi4.y, hi4.z, hi4.w};
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      h[e] = (half_t)v[e];
      l[e] = (half_t)(v[e] - (float)h[e]);
    }
  };
#pragma unroll 2
  for (int ks = wv; ks < nks; ks += 4) {
    const f32x4 x0 = *(const f32x4*)(xr + 32 * ks), x1 = *(const f32x4*)(xr + 32 * ks + 4);
    const f32x4 s0 = *(const f32x4*)(scale + mo + 32 * ks), s1 = *(const f32x4*)(scale + mo + 32 * ks + 4);
    const f32x4 h0 = *(const f32x4*)(shift + mo + 32 * ks), h1 = *(const f32x4*)(shift + mo + 32 * ks + 4);
    const f32x4 a0 = (x0 - mean) * rstd * (1.0f + s0) + h0, a1 = (x1 - mean) * rstd * (1.0f + s1) + h1;
    half8_t ah, al;
    split(a0, a1, ah, al);
#pragma unroll
    for (int t = 0; t < NT; ++t) {
      const float* wr = Wf + (long)(t * 16 + a) * D + 32 * ks + 8 * q;  // output column t * 16 + (lane & 15), same k slice
      half8_t wh, wl;
      split(*(const f32x4*)wr, *(const f32x4*)(wr + 4), wh, wl);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wh, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, wh, acc[t], 0, 0, 0);
      acc[t] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, wl, acc[t], 0, 0, 0);
    }
  }
#pragma unroll
  for (int t = 0; t < NT; ++t) *(f32x4_t*)acc_s[wv][t][lane] = acc[t];
  __syncthreads();
  if (wv != 0) return;
  // ---- lane holds out[row 4 q + r][column o = t * 16 + (lane & 15)], r = 0..3
  const float dt = base ? *dt_ptr : 0.f;
  const int grid = R / p;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const f32x4_t tot = (*(const f32x4_t*)acc_s[0][t][lane] + *(const f32x4_t*)acc_s[1][t][lane]) +
                        (*(const f32x4_t*)acc_s[2][t][lane] + *(const f32x4_t*)acc_s[3][t][lane]);
    const int o = t * 16 + a;
    const float bo = bf[o];
    const int pp = o / (p * C), qq = (o / C) % p, c = o % C;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 4 * q + r;
      float val = tot[r] + bo;
      if (CFG) {  // rows 0..7 conditional, 8..15 their unconditional twins: lane ^ 32 holds the twin's value
        const float other = xhalf(val);
        const float cond = row < 8 ? val : other, uncond = row < 8 ? other : val;
        val = uncond + cfg_scale * (cond - uncond);
      }
      const long mr = CFG ? tile * 8 + (row & 7) + (row >> 3) * (long)Mh : tile * 16 + row;
      const int n = (int)(mr / tokens), tok = (int)(mr % tokens);
      const long off = (((long)n * C + c) * R + (tok / grid) * p + pp) * R + (tok % grid) * p + qq;
      out[off] = base ? base[off] + dt * val : val;
    }
  }
}

__global__ __launch_bounds__(256) void cond_row_copy_kernel(const float* __restrict__ table, long row_floats, const int* __restrict__ step, int offset,
                                                            int fixed_row, float* __restrict__ mod, long nmod, float* __restrict__ uvq, long nq,
                                                            float* __restrict__ uvf, long nf, int to_table, int rows) {
  const long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
  if (i >= nmod + nq + nf) return;
  const long row = step ? (long)(*step + offset) : (long)fixed_row;
  float* ws = i < nmod ? mod + i : (i < nmod + nq ? uvq + (i - nmod) : uvf + (i - nmod - nq));  // nmod, nq, nf are multiples of 4
  if (rows > 0 && (row < 0 || row >= rows)) {  // a row the table does not have (wrong offset / counter): poison instead of reading out of bounds
    if (!to_table) *(f32x4*)ws = (f32x4){__builtin_nanf(""), __builtin_nanf(""), __builtin_nanf(""), __builtin_nanf("")};
    return;
  }
  float* tb = (float*)table + row * row_floats + i;
  if (to_table) *(f32x4*)tb = *(const f32x4*)ws;
  else *(f32x4*)ws = *(const f32x4*)tb;
}
