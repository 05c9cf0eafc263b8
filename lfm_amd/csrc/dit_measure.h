// Measurement aids of the DiT path: event probes, trace readers, per-kernel checksums, the clock probe and the LFM_MEASURE GEMM variants
// (included by dit.hip after the option block and the kernel headers).
#pragma once

// ------------------------------------------------------------------ in-situ timing of the dominant kernel (measurement only)
// bench.py's roofline row needs the fc1 GEMM's duration INSIDE a real forward (real activations, real cache state); the
// captured graph cannot be bracketed from outside, so an eager forward can record one HIP event pair per block here.
#define LFM_PROF_MAX 64
#define LFM_PROF_BLK_MAX 16
static hipEvent_t g_prof_ev[2 * LFM_PROF_MAX];
static bool g_prof_init = false, g_prof_on = false;
static int g_prof_count = 0;
static hipEvent_t g_prof_blk_ev[2 * LFM_PROF_BLK_MAX];  // around the whole block loop of an evaluation (all blocks' qkv .. fc2)
static int g_prof_blk_count = 0;
static int g_prof_mode = 0;  // 1: an event pair around every fc1 launch (+ the block loop); 2: around the block loop only (no events between the kernels)
static hipStream_t g_prof_stream = nullptr;  // the stream that owns the probe (the first one that launches while it is on)
static bool g_prof_owned = false, g_prof_conflict = false;
// The probe is a measurement device for ONE stream driven by ONE host thread (bench.py).  Switching it, claiming it and reading it are serialised by a mutex, so
// that a second host thread enqueueing evaluations at the same time gets a clean refusal (g_prof_conflict) instead of a data race on the flags; the sample
// counters are touched only by the thread whose stream owns the probe (prof_claim returned true for it).
static std::mutex g_prof_mu;
extern "C" int lfm_profile_fc1(int enable) {
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (enable && !g_prof_init) {
    for (int i = 0; i < 2 * LFM_PROF_MAX; ++i)
      if (hipEventCreate(&g_prof_ev[i]) != hipSuccess) return LFM_ERR_LAUNCH;
    for (int i = 0; i < 2 * LFM_PROF_BLK_MAX; ++i)
      if (hipEventCreate(&g_prof_blk_ev[i]) != hipSuccess) return LFM_ERR_LAUNCH;
    g_prof_init = true;
  }
  g_prof_on = enable != 0;
  g_prof_mode = enable;
  if (enable) {
    g_prof_count = 0;
    g_prof_blk_count = 0;
    g_prof_owned = false;
    g_prof_conflict = false;
  }
  return LFM_OK;
}
static bool prof_claim(hipStream_t st) {  // may THIS evaluation record its fc1 launches?
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!g_prof_on) return false;
  if (!g_prof_owned) {
    g_prof_owned = true;
    g_prof_stream = st;
  }
  if (st != g_prof_stream) {
    g_prof_conflict = true;
    return false;
  }
  return true;
}
// The event pair around one fc1 launch of the evaluation that owns the probe (mode 1): begin returns whether the pair is recorded, end takes that answer.
// An evaluation that fails in between records no sample.
static inline bool prof_fc1_begin(bool prof_ok, hipStream_t st) {
  const bool on = prof_ok && g_prof_mode == 1 && g_prof_count < LFM_PROF_MAX;
  if (on) (void)hipEventRecord(g_prof_ev[2 * g_prof_count], st);
  return on;
}
static inline void prof_fc1_end(bool on, hipStream_t st) { if (on) (void)hipEventRecord(g_prof_ev[2 * g_prof_count++ + 1], st); }
extern "C" int lfm_profile_fc1_read(float* ms_out, int max_n) {  // synchronises; returns the number of samples written
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!ms_out || !g_prof_init) return LFM_ERR_ARG;
  if (g_prof_conflict) return LFM_ERR_ARG;  // a second stream launched evaluations while the probe was on: the samples would time its kernels too
  const int n = g_prof_count < max_n ? g_prof_count : max_n;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof_ev[2 * i + 1]) != hipSuccess) return LFM_ERR_LAUNCH;
    if (hipEventElapsedTime(&ms_out[i], g_prof_ev[2 * i], g_prof_ev[2 * i + 1]) != hipSuccess) return LFM_ERR_LAUNCH;
  }
  return n;
}

extern "C" int lfm_profile_blocks_read(float* ms_out, int max_n) {  // one sample per recorded evaluation: its whole block loop; synchronises
  std::lock_guard<std::mutex> lk(g_prof_mu);
  if (!ms_out || !g_prof_init) return LFM_ERR_ARG;
  if (g_prof_conflict) return LFM_ERR_ARG;
  const int n = g_prof_blk_count < max_n ? g_prof_blk_count : max_n;
  for (int i = 0; i < n; ++i) {
    if (hipEventSynchronize(g_prof_blk_ev[2 * i + 1]) != hipSuccess) return LFM_ERR_LAUNCH;
    if (hipEventElapsedTime(&ms_out[i], g_prof_blk_ev[2 * i], g_prof_blk_ev[2 * i + 1]) != hipSuccess) return LFM_ERR_LAUNCH;
  }
  return n;
}

#ifdef LFM_MEASURE  // s_memtime trace readers: measurement builds only (include/lfm_hip.h)
extern "C" int lfm_gemm_trace_read(unsigned long long* host_out, int n_per_group) {  // 2 x n stamps (group 0, group 1)
  if (!host_out || n_per_group <= 0 || n_per_group > G256Q_TRACE_MAX) return LFM_ERR_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return LFM_ERR_LAUNCH;
  for (int g = 0; g < 2; ++g)
    if (hipMemcpyFromSymbol(host_out + (size_t)g * n_per_group, HIP_SYMBOL(g256q_trace), sizeof(unsigned long long) * n_per_group,
                            sizeof(unsigned long long) * G256Q_TRACE_MAX * g, hipMemcpyDeviceToHost) != hipSuccess)
      return LFM_ERR_LAUNCH;
  return LFM_OK;
}

extern "C" int lfm_attention_trace_read(unsigned long long* host_out, int n) {  // the s_memtime stamps of the MODE 3 attention build
  if (!host_out || n <= 0 || n > ATT_TRACE_SLOTS) return LFM_ERR_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return LFM_ERR_LAUNCH;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(att_trace), sizeof(unsigned long long) * n, 0, hipMemcpyDeviceToHost) != hipSuccess) return LFM_ERR_LAUNCH;
  return LFM_OK;
}

extern "C" int lfm_attention_wg_trace_read(unsigned long long* host_out, int n_wg) {  // MODE 3: {hw id, start, landed, end} per workgroup
  if (!host_out || n_wg <= 0 || n_wg > ATT_WG_TRACE) return LFM_ERR_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return LFM_ERR_LAUNCH;
  if (hipMemcpyFromSymbol(host_out, HIP_SYMBOL(att_wg_trace), sizeof(unsigned long long) * 4 * n_wg, 0, hipMemcpyDeviceToHost) != hipSuccess) return LFM_ERR_LAUNCH;
  return LFM_OK;
}
// Per-kernel checksums of one armed evaluation (tools/concurrency_ws_diff.py): after every kernel of the folded block loop the 64-bit wrap-around sum of
// its output buffer's 32-bit words (integer adds: order-independent, so equal data <=> equal sum whatever the reduction order) goes into a slot
// [block][8]: 0 Q|K|V^T after qkv, 1 O after attention, 2 X / 3 A' (A2) / 4 row partials after proj, 5 H after fc1, 6 X / 7 A' (A) after fc2.
#define DIT_CHK_SLOTS (64 * 8)
static unsigned long long* g_chk = nullptr;
static const void* g_chk_ws = nullptr;
__global__ __launch_bounds__(256) void chk_kernel(const unsigned* __restrict__ p, long nwords, unsigned long long* __restrict__ out) {
  unsigned long long s = 0;
  for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (long)gridDim.x * 256) s += p[i];
  atomicAdd(out, s);
}
static void dit_chk(const void* buf, size_t bytes, int block, int slot, hipStream_t st) {
  if (!g_chk || block >= 64) return;
  hipLaunchKernelGGL(chk_kernel, dim3(1024), dim3(256), 0, st, (const unsigned*)buf, (long)(bytes / 4), g_chk + block * 8 + slot);
}
extern "C" int lfm_dit_chk_arm(const void* workspace) {  // the evaluations that run on THIS workspace record their checksums (nullptr: off)
  if (!g_chk && hipMalloc((void**)&g_chk, DIT_CHK_SLOTS * 8) != hipSuccess) return LFM_ERR_LAUNCH;
  g_chk_ws = workspace;
  return LFM_OK;
}
extern "C" int lfm_dit_chk_read(unsigned long long* host_out, int n) {
  if (!host_out || n <= 0 || n > DIT_CHK_SLOTS || !g_chk) return LFM_ERR_ARG;
  if (hipDeviceSynchronize() != hipSuccess) return LFM_ERR_LAUNCH;
  if (hipMemcpy(host_out, g_chk, (size_t)n * 8, hipMemcpyDeviceToHost) != hipSuccess) return LFM_ERR_LAUNCH;
  return LFM_OK;
}
#ifdef LFM_EXP_DUMP
// (experiment build, tools/cosched_dump.py) the folded fc1 epilogue of every block of the evaluations on THIS workspace dumps the operands of its affine
static float* g_dbg = nullptr;
static long g_dbg_stride = 0;
static const void* g_dbg_ws = nullptr;
extern "C" int lfm_dit_dbg_arm(const void* workspace, float* dump, long stride_floats) {
  g_dbg = dump;
  g_dbg_stride = stride_floats;
  g_dbg_ws = workspace;
  return LFM_OK;
}
#endif
#else
static inline void dit_chk(const void*, size_t, int, int, hipStream_t) {}  // the shipped build records no checksums
#endif  // LFM_MEASURE

// ------------------------------------------------------------------ effective clock under matrix load (measurement aid for bench.py)
// The GEMMs of this path run under the board power cap: boxes of the pool differ by 6-7 % in the clock they sustain, and a
// roofline fraction means little without it.  One workgroup per CU streams v_mfma_f32_16x16x32_f16 on pseudo-random fp16 operands (the load the GEMMs
// put on the chip) for `iters` x 64 instructions per wave and brackets the stream with s_memtime (one tick = one shader cycle, MI355X_MICROARCH.md):
// ticks / wall time = the sustained clock.  out[0 .. blocks) = ticks per workgroup.
__global__ __launch_bounds__(512) void clock_probe_kernel(unsigned long long* __restrict__ out, int iters, unsigned seed) {
  half8_t a[4], b[4];
  unsigned h = seed ^ (threadIdx.x * 2654435761u) ^ (blockIdx.x * 40503u);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      h = h * 1664525u + 1013904223u;
      a[i][e] = (half_t)(((int)(h >> 16) & 1023) * (1.0f / 512.0f) - 1.0f);
      h = h * 1664525u + 1013904223u;
      b[i][e] = (half_t)(((int)(h >> 16) & 1023) * (1.0f / 512.0f) - 1.0f);
    }
  f32x4 c[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) c[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
  unsigned long long t0, t1;
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t0)::"memory");
  for (int it = 0; it < iters; ++it) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int j = 0; j < 16; ++j) c[j] = __builtin_amdgcn_mfma_f32_16x16x32_f16(a[j & 3], b[(j >> 2) & 3], c[j], 0, 0, 0);
  }
  asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t1)::"memory");
  float s = 0.f;
#pragma unroll
  for (int j = 0; j < 16; ++j) s += c[j][0] + c[j][3];
  if (threadIdx.x == 0) out[blockIdx.x] = t1 - t0;
  if (s == 123.456f) out[blockIdx.x] = 0;  // keeps the accumulators live
}

extern "C" int lfm_clock_probe(int blocks, int iters, unsigned long long* ticks_out, lfm_stream_t stream) {
  if (!ticks_out || blocks <= 0 || iters <= 0) return LFM_ERR_ARG;
  hipLaunchKernelGGL(clock_probe_kernel, dim3(blocks), dim3(512), 0, (hipStream_t)stream, ticks_out, iters, 12345u);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

// lfm_gemm_f16 / lfm_gemm_qkv_f16: the automatic choice; in a measurement build, first the variants that a forced kernel 5 / 6 plus flags ask for.
// The main-loop-ablation and OPT variants exist for the GELU epilogue only (every further epilogue would multiply the measurement build's kernels).
template <class Epi>
static int gemm_f16_launch(const ASrcRowMajor& a, const half_t* W, long ldw, int M, int N, int K, const Epi& e, hipStream_t st) {
#ifdef LFM_MEASURE
  const int sel = gemm_sel(), dbg = gemm_dbg();
  if (K % G256Q_BK == 0 && sel == 5 && (dbg & LFM_DBG_TRACE_GEMM)) return launch_gemm256h_tn<ASrcRowMajor, Epi, true>(a, W, ldw, M, N, K, e, st);  // the epilogue-stamped build
  if constexpr (std::is_same<Epi, EpiBiasGeluF16>::value) {
    const int abl = (dbg >> LFM_DBG_GEMM_ABL_SHIFT) & LFM_DBG_GEMM_ABL_MASK, opt = (dbg >> LFM_DBG_GEMM_OPT_SHIFT) & LFM_DBG_GEMM_OPT_MASK;
    if (K % G256Q_BK == 0 && sel == 5 && (abl & 7)) {  // kernel 5, main-loop ablations: the field's low three bits, its top bit turns variant 7 into 8
      switch (abl & 7) {
        case 1: return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 1>(a, W, ldw, M, N, K, e, st);
        case 2: return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 2>(a, W, ldw, M, N, K, e, st);
        case 3: return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 3>(a, W, ldw, M, N, K, e, st);
        case 4: return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 4>(a, W, ldw, M, N, K, e, st);
        case 5: return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 5>(a, W, ldw, M, N, K, e, st);
        case 6: return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 6>(a, W, ldw, M, N, K, e, st);
        default: return (abl & 8) ? launch_gemm256h_tn<ASrcRowMajor, Epi, false, 8>(a, W, ldw, M, N, K, e, st)
                                  : launch_gemm256h_tn<ASrcRowMajor, Epi, false, 7>(a, W, ldw, M, N, K, e, st);
      }
    }
    if (K % G256Q_BK == 0 && (sel == 5 || sel == 6) && opt) {  // OPT variants
      if (sel == 6) return launch_gemm256w_tn<ASrcRowMajor, Epi, 0, 0, 1>(a, W, ldw, M, N, K, e, st);
      if (opt == 1) return launch_gemm256h_tn<ASrcRowMajor, Epi, false, 0, 1>(a, W, ldw, M, N, K, e, st);
      return LFM_ERR_ARG;  // (kernel 5 has no further OPT variant: bit 1 went with round 4's rejected DMA-before-reads placement)
    }
    if (K % G256Q_BK == 0 && sel == 6 && abl) {  // kernel 6: main-loop ablations 1..4, DMA placement 8
      switch (abl) {
        case 1: return launch_gemm256w_tn<ASrcRowMajor, Epi, 1>(a, W, ldw, M, N, K, e, st);
        case 2: return launch_gemm256w_tn<ASrcRowMajor, Epi, 2>(a, W, ldw, M, N, K, e, st);
        case 3: return launch_gemm256w_tn<ASrcRowMajor, Epi, 3>(a, W, ldw, M, N, K, e, st);
        case 4: return launch_gemm256w_tn<ASrcRowMajor, Epi, 4>(a, W, ldw, M, N, K, e, st);
        case 8: return launch_gemm256w_tn<ASrcRowMajor, Epi, 0, 1>(a, W, ldw, M, N, K, e, st);
        default: return LFM_ERR_ARG;
      }
    }
  }
#endif
  return launch_gemm_auto(a, W, ldw, M, N, K, e, st);
}
