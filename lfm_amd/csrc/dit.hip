// DiT velocity field on gfx950: the kernels around the MFMA GEMMs and the per-call driver.
// Reference behaviour: /root/reference/models/DiT.py (cited per kernel).
#include <mutex>

#include "../../include/lfm_hip.h"
#include "gemm_dispatch.h"
#include "gemm_skinny_kernel.h"
#include "gemm_sq64_kernel.h"
#include "qkv_attention_kernel.h"

// Library-wide switches = process-wide DEFAULTS (lfm_gemm_select, lfm_set_option); a call that carries its own values (lfm_dit_call.fold_ln /
// .gemm_select, ABI 4) overrides them in THREAD-LOCAL state for the duration of lfm_dit_forward: every launcher reads the effective value on the
// calling thread while it enqueues, so two host threads (or two lanes in flight with different settings) never see each other's choice.
// The defaults are written by one thread while others enqueue: relaxed atomics, each value stands on its own (as lfm_device_mask, common.h).
typedef std::atomic<int> Opt;
static inline int opt_get(const Opt& o) { return o.load(std::memory_order_relaxed); }
static inline void opt_set(Opt& o, int v) { o.store(v, std::memory_order_relaxed); }
static struct {
  Opt gemm_sel{0}, gemm_dbg{0};  // lfm_gemm_select: kernel, ablation flags (debug_flags.h)
  Opt fold_ln{1};                // LFM_OPT_FOLD_LN
  Opt v6{0};                     // LFM_OPT_GEMM_V6
  Opt skinny{1};  // LFM_OPT_SKINNY_GEMM: the batch-1 DiT linears on their own kernels (1: 64x64 tiles where the image has whole 64-token tiles,
                  // gemm_sq64_kernel.h, else all rows x 16 columns, gemm_skinny_kernel.h; 2: always the latter; 0: the rounds 2-4 split-K path)
  Opt stagger{0};     // measurement builds, lfm_set_option key 3
  Opt att_stream{1};  // LFM_OPT_ATTENTION_STREAM: 256 tokens x head_dim 64 with more than 64 (image, head) items on the persistent streamed kernel
  Opt fused_qkv{1};   // LFM_OPT_FUSED_QKV_ATTENTION: folded path at 256 tokens x head_dim 64: QKV projection + attention in one kernel (qkv_attention_kernel.h)
  Opt att_tiled{1};   // LFM_OPT_ATTENTION_TILED: DiT attention at the token counts no other kernel serves on the tiled any-T kernel (attention_tiled_kernel.h); 2: every shape it takes
  Opt unet_att_stream{1};  // LFM_OPT_UNET_ATTENTION_STREAM: UNet attention shapes neither the resident nor the VALU kernel serves on the streamed kernel (unet_attention_dispatch.h: unet_attention_choose)
} g_def;
static thread_local int tl_sel_set = 0, tl_gemm_sel = 0, tl_gemm_dbg = 0;  // per-call kernel selection active on this thread
static thread_local int tl_fold = 0;                                       // 0: default, LFM_CALL_OFF, LFM_CALL_ON
static inline int gemm_sel() { return tl_sel_set ? tl_gemm_sel : opt_get(g_def.gemm_sel); }
static inline int gemm_dbg() { return tl_sel_set ? tl_gemm_dbg : opt_get(g_def.gemm_dbg); }
static inline int opt_fold_ln() { return tl_fold ? (tl_fold == LFM_CALL_ON ? 1 : 0) : opt_get(g_def.fold_ln); }
int lfm_gemm_selected() { return gemm_sel(); }
int lfm_gemm_debug_flags() { return gemm_dbg(); }
int lfm_gemm_selected_v1_ok() { return gemm_sel() < 2 && !(gemm_dbg() & LFM_DBG_GEMM_NO_SPLITK); }
int lfm_gemm_prefers_v4(int M, int N, int K) {  // no shape today: only the A/B flags of the automatic choice
  (void)M;
  (void)N;
  (void)K;
  if (gemm_dbg() & LFM_DBG_GEMM_NEVER_V4) return 0;
  if (gemm_dbg() & LFM_DBG_GEMM_ALWAYS_V4) return 1;
  return 0;
}
int lfm_gemm_v6_default() { return opt_get(g_def.v6); }
int lfm_stagger_ticks() { return opt_get(g_def.stagger); }
int lfm_attention_stream_enabled() { return opt_get(g_def.att_stream); }
int lfm_attention_tiled_mode() { return opt_get(g_def.att_tiled); }
int lfm_unet_attention_stream_mode() { return opt_get(g_def.unet_att_stream); }
// Which kernel launch_gemm_auto runs for a shape under the calling thread's selection (host only, no GPU needed): caps bit 0 = the instantiation can take
// kernel 6 (row-major A, no per-lane tile accumulators in the epilogue), bit 1 = the operands fit 32-bit buffer offsets.
extern "C" int lfm_gemm_plan(int M, int N, int K, int batch, int caps) { return gemm_choose(M, N, K, batch, caps); }
static inline bool gemm_select_valid(int which) {
  const int k = which & 15;
  return which >= 0 && (k == 0 || k == 1 || k == 4 || k == 5 || k == 6 || k == 7 || k == 8);  // 7, 8: the latency-mode kernels through lfm_gemm_f16 (tests)
}
struct CallScope {  // per-call settings of one lfm_dit_forward on this thread (restored on every return path)
  int sel_set, sel, dbg, fold;
  CallScope() : sel_set(tl_sel_set), sel(tl_gemm_sel), dbg(tl_gemm_dbg), fold(tl_fold) {}
  ~CallScope() {
    tl_sel_set = sel_set;
    tl_gemm_sel = sel;
    tl_gemm_dbg = dbg;
    tl_fold = fold;
  }
};

static int call_scope_enter(const lfm_dit_call* c) {  // after a CallScope was opened on this thread
  if (c->fold_ln < 0 || c->fold_ln > LFM_CALL_ON || c->gemm_select < 0 || (c->gemm_select && !gemm_select_valid(c->gemm_select - 1)) || c->cond_rows < 0)
    return LFM_ERR_ARG;
  if (c->fold_ln) tl_fold = c->fold_ln;
  if (c->gemm_select) {
    tl_sel_set = 1;
    tl_gemm_sel = (c->gemm_select - 1) & 15;
    tl_gemm_dbg = (c->gemm_select - 1) >> 4;
  }
  return LFM_OK;
}
// What lfm_dit_forward would run `call` with on the calling thread, right now: gemm_select_out = kernel | flags << 4, fold_ln_out = 0 / 1.  Goes through
// the same scope code as the forward (no launch, no GPU needed): the CPU test of the per-call / per-thread scoping (tests/test_c_abi.py).
extern "C" int lfm_dit_call_settings(const lfm_dit_call* call, int* gemm_select_out, int* fold_ln_out) {
  if (!call || !gemm_select_out || !fold_ln_out) return LFM_ERR_ARG;
  CallScope scope;
  const int rc = call_scope_enter(call);
  if (rc) return rc;
  *gemm_select_out = gemm_sel() | (gemm_dbg() << 4);
  *fold_ln_out = opt_fold_ln();
  return LFM_OK;
}

extern "C" int lfm_set_option(int key, int value) {
  switch (key) {
    case 1: opt_set(g_def.fold_ln, value != 0); break;  // LFM_OPT_FOLD_LN: adaLN LayerNorm-modulate folded into the GEMM epilogues (default 1)
    case 2: opt_set(g_def.v6, value != 0); break;       // LFM_OPT_GEMM_V6: the one-wave-per-SIMD 256x256 kernel for the chip-filling row-major GEMMs
#ifdef LFM_MEASURE
    case 3: opt_set(g_def.stagger, value > 0 ? value : 0); break;  // start offset (s_memtime ticks) of the second resident workgroups of the two-per-CU kernels (gemm256_common.h)
#endif
    case 4: opt_set(g_def.skinny, value < 0 || value > 2 ? 1 : value); break;  // LFM_OPT_SKINNY_GEMM: 0 = the split-K 128x128 path of rounds 2-4 for M <= 256 (A/B, parity)
    case 5: opt_set(g_def.att_stream, value != 0); break;  // LFM_OPT_ATTENTION_STREAM: 0 = one workgroup per (image, head) item (the rounds 1-5 kernel; A/B and the bit-equality test)
    case 6: opt_set(g_def.fused_qkv, value != 0); break;   // LFM_OPT_FUSED_QKV_ATTENTION: 0 = the QKV GEMM and the attention kernel as two launches (A/B and the bit-equality test)
    case 7: opt_set(g_def.unet_att_stream, value < 0 || value > 2 ? 1 : value); break;  // LFM_OPT_UNET_ATTENTION_STREAM: 0 = those shapes refused (as before the kernel), 2 = every shape it takes (parity, A/B)
    case 8:  // LFM_OPT_ATTENTION_TILED: 0 = the token counts only the tiled kernel serves are refused (as before the kernel), 2 = every shape it takes (parity, A/B)
      if (value < 0 || value > 2) return LFM_ERR_ARG;
      opt_set(g_def.att_tiled, value);
      break;
    default: return LFM_ERR_ARG;
  }
  return LFM_OK;
}
extern "C" int lfm_gemm_select(int which) {  // low 4 bits: kernel choice (0 auto, 1, 4, 5, 6; 7, 8 for lfm_gemm_f16 only); bits 4+: ablation flags (measurement only)
  if (!gemm_select_valid(which)) return LFM_ERR_ARG;
  opt_set(g_def.gemm_sel, which & 15);
  opt_set(g_def.gemm_dbg, which >> 4);
  return LFM_OK;
}

#include "dit_kernels.h"
#include "attention_dispatch.h"  // the DiT attention kernels + attention_choose / attention_launch
#include "solver_kernels.h"
#include "dit_measure.h"

// ------------------------------------------------------------------ host side
static inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

struct DitWs {
  float* X;       // [M, D] fp32 residual stream
  half_t* A;      // [M, D] LN output / attention output
  half_t* A2;     // [M, D] folded path: the proj GEMM's A' output (fc1's operand).  NOT ws.A: proj's operand IS ws.A (the attention output), and a tile of
                  // a row panel may still be streaming columns that a sibling tile's epilogue would overwrite (round 4: found by the full-size parity test)
  half_t* QKVH;   // max(3*M*D, M*H): Q | K | Vt, later the fc1 activation
  float* temb;    // [B, D]
  float* temb_h;  // [B, D] hidden layer of the t-MLP
  half_t* c_half; // [B, D]
  float* mod;     // [B, J]
  float* ones;    // [D] of 1.0f: gate row of the patch-embedding GEMM (large patches)
  // folded LayerNorm-modulate (gemm_epilogues.h): row partials, two centring-constant arrays (ping-pong), the u / v GEMM's operand and results
  float* ln_part;  // [M][ceil(D / 256)][2]
  float* cen[2];   // [M] each
  half_t* amod;    // [depth][2 branches][2][rows][D] fp16: (1 + scale | shift) rows
  float* uvq;      // [depth][2 rows][3D]: u, v of the qkv projections
  float* uvf;      // [depth][2 rows][H]:  u, v of fc1
  float* slab;    // split-K partial tiles (small M only, else null)
  size_t slab_bytes;
  size_t total;
};

// The sizes every function of the driver derives from (shape, batch): computed here and nowhere else.
// B batch, T tokens per image, M token rows, D residual width, H MLP width, J floats of one conditioning row's adaLN output (six rows per block + the final
// layer's two), KK patch values per token = outputs per token of the final layer, tiles_p row-partial slots of the folded LayerNorm, hd head dimension,
// uvq_n / uvf_n floats of one conditioning row's u, v rows of the qkv / fc1 projections (0 for shapes that never fold).
struct DitDims {
  int B, T, M, D, H;
  long J, uvq_n, uvf_n;
  int KK, tiles_p, hd;
};
// Shapes that can ever take the folded LayerNorm path: row partials in whole 256-column slots, fc1 on the 256x256 kernels.  The workspace holds the fold's
// operands, a conditioning-table row holds u / v, and dit_plan() allows the fold for exactly these shapes.
static inline bool dit_fold_capable(const lfm_dit_shape* s) { return (s->hidden % 256) == 0 && (s->mlp_hidden % 64) == 0; }
static DitDims dit_dims(const lfm_dit_shape* s, int B) {
  const int grid = s->res / s->patch, T = grid * grid, D = s->hidden, H = s->mlp_hidden;
  const long uv = dit_fold_capable(s) ? (long)s->depth * 2 : 0;
  return DitDims{B, T, B * T, D, H, (long)s->depth * 6 * D + 2 * D, uv * 3 * D, uv * H, s->in_ch * s->patch * s->patch, D / 256, D / s->heads};
}

static DitWs carve(const lfm_dit_shape* s, const DitDims& d, void* ws, bool sizing = false) {
  const size_t B = d.B, T = d.T, M = d.M, D = d.D, H = d.H, J = d.J;
  size_t off = 0;
  char* base = (char*)ws;
  DitWs w;
  auto take = [&](size_t bytes) {
    char* p = (char*)((uintptr_t)base + off);  // with a null base the pointers ARE the byte offsets (lfm_dit_workspace_layout)
    off += align_up(bytes, 256);
    return p;
  };
  w.X = (float*)take(M * D * 4);
  w.A = (half_t*)take(M * D * 2);
  const size_t qkvh = (3 * M * D > M * H ? 3 * M * D : M * H) * 2;
  w.QKVH = (half_t*)take(qkvh);
  w.temb = (float*)take(B * D * 4);
  w.temb_h = (float*)take(B * D * 4);
  w.c_half = (half_t*)take(B * D * 2);
  w.mod = (float*)take(B * J * 4);
  w.ones = (float*)take(D * 4);
  w.ln_part = (float*)take(M * ((D + 255) / 256) * 8);
  w.cen[0] = (float*)take(M * 4);
  w.cen[1] = (float*)take(M * 4);
  const bool fold_ops = dit_fold_capable(s);  // only these shapes pay for the fold's operands
  w.amod = (half_t*)take(fold_ops ? (size_t)s->depth * 4 * B * D * 2 : 0);
  w.uvq = (float*)take(fold_ops ? (size_t)s->depth * 2 * B * 3 * D * 4 : 0);
  w.uvf = (float*)take(fold_ops ? (size_t)s->depth * 2 * B * H * 4 : 0);
  w.A2 = (half_t*)take(fold_ops ? M * D * 2 : 0);
  // latency mode: room for up to 4 K slices of the widest GEMM output (fc1), when the token count is small
  // (when SIZING for a maximum batch, reserve the slabs of the largest small batch too, so that the requirement is monotone in the
  // batch and a workspace sized for max_batch serves every smaller batch)
  const size_t Ms = sizing ? (M < 1024 ? M : (size_t)1024 / T * T) : M;
  w.slab_bytes = (sizing || M <= 1024) && Ms > 0 ? 4 * Ms * (H > 3 * D ? H : 3 * D) * 4 : 0;
  w.slab = w.slab_bytes ? (float*)take(w.slab_bytes) : nullptr;
  if (!base) w.slab = nullptr;
  w.total = off;
  return w;
}

static int check_shape(const lfm_dit_shape* s) {
  if (!s) return LFM_ERR_ARG;
  if (s->depth <= 0 || s->hidden <= 0 || s->heads <= 0 || s->patch <= 0 || s->in_ch <= 0 || s->res <= 0) return LFM_ERR_SHAPE;
  if (s->hidden % s->heads) return LFM_ERR_SHAPE;
  if (s->res % s->patch) return LFM_ERR_SHAPE;
  const int T = (s->res / s->patch) * (s->res / s->patch);
  // an attention kernel for (head_dim, tokens) -- S / B / L: 64; XL: 1152 / 16 = 72; LDS-resident K / V^T up to 256 tokens, 1024 = four key chunks, the other
  // square grids of a side that is a multiple of 4 up to 3600 tokens on the tiled kernel (the answer for ONE image: whether a shape is served does not
  // depend on the batch)
  if (attention_choose(1, s->heads, s->hidden / s->heads, T) < 0) return LFM_ERR_SHAPE;
  if (s->hidden % 64 || s->hidden > 256 * LN_MAXV || s->mlp_hidden % 64) return LFM_ERR_SHAPE;
  const int kk = s->patch * s->patch * s->in_ch;
  if (kk > FIN_MAXO || (kk > PE_MAXK && (kk % 64))) return LFM_ERR_SHAPE;  // small patches: register kernel; large: GEMM (K % 64 == 0)
  if (s->label_rows <= 0) return LFM_ERR_SHAPE;
  return LFM_OK;
}

extern "C" const char* lfm_strerror(int code) {
  switch (code) {
    case LFM_OK: return "ok";
    case LFM_ERR_SHAPE: return "unsupported or inconsistent shape";
    case LFM_ERR_ALIGN: return "pointer / leading dimension alignment";
    case LFM_ERR_WORKSPACE: return "workspace too small";
    case LFM_ERR_LAUNCH: return "kernel launch failed";
    case LFM_ERR_ARG: return "bad argument";
  }
  return "unknown";
}
extern "C" int lfm_abi_version(void) { return LFM_ABI_VERSION; }  // 2: lfm_time_embed takes label_rows; 3: lfm_dit_call carries the per-grid conditioning table; 4: + cond_rows, per-call fold_ln / gemm_select

extern "C" size_t lfm_dit_workspace_bytes(const lfm_dit_shape* shape, int max_batch) {
  if (check_shape(shape) != LFM_OK || max_batch <= 0) return 0;
  return carve(shape, dit_dims(shape, max_batch), nullptr, true).total;
}

// Byte offsets of the buffers an evaluation at `batch` reads and writes inside its workspace, from carve() itself (tests read intermediate results back).
extern "C" int lfm_dit_workspace_layout(const lfm_dit_shape* shape, int batch, size_t* offsets_out, int n) {
  const int rc = check_shape(shape);
  if (rc) return rc;
  if (!offsets_out || n < 0) return LFM_ERR_ARG;
  if (batch <= 0) return LFM_ERR_SHAPE;
  const DitWs w = carve(shape, dit_dims(shape, batch), nullptr);
  const bool fold_ops = dit_fold_capable(shape);
  const void* bufs[LFM_DIT_WS_BUFFERS] = {w.X, w.A, fold_ops ? w.A2 : nullptr, w.QKVH, w.mod, w.ln_part, w.cen[0], w.cen[1], fold_ops ? w.uvq : nullptr,
                                          fold_ops ? w.uvf : nullptr};
  for (int i = 0; i < n && i < LFM_DIT_WS_BUFFERS; ++i) offsets_out[i] = (size_t)(uintptr_t)bufs[i];
  return LFM_DIT_WS_BUFFERS;
}

extern "C" int lfm_dit_attention_hd(const void* Q, const void* K, const void* Vt, void* O, int batch, int heads, int head_dim, int T,
                                    lfm_stream_t stream) {
  if (!Q || !K || !Vt || !O) return LFM_ERR_ARG;
  if (batch <= 0 || heads <= 0) return LFM_ERR_SHAPE;
  if (((uintptr_t)Q | (uintptr_t)K | (uintptr_t)Vt | (uintptr_t)O) & 15) return LFM_ERR_ALIGN;
  return attention_launch((const half_t*)Q, (const half_t*)K, (const half_t*)Vt, (half_t*)O, batch, heads, head_dim, T, (hipStream_t)stream);
}
// Which kernel lfm_dit_attention_hd runs for a shape under the calling thread's flags and the library options (attention_kernel.h: attention_choose; host only).
extern "C" int lfm_attention_plan(int batch, int heads, int head_dim, int T) {
  if (batch <= 0 || heads <= 0) return LFM_ERR_SHAPE;
  return attention_choose(batch, heads, head_dim, T);
}
extern "C" int lfm_dit_attention(const void* Q, const void* K, const void* Vt, void* O, int batch, int heads, int T, lfm_stream_t stream) {
  return lfm_dit_attention_hd(Q, K, Vt, O, batch, heads, 64, T, stream);
}

static int ln_modulate_launch(const float* X, half_t* A, int M, int D, int tokens, const float* shift, const float* scale, long stride,
                              hipStream_t st) {
  if (D % 4 || D > 256 * LN_MAXV) return LFM_ERR_SHAPE;
  if (D % 8 == 0 && !(((uintptr_t)A | (uintptr_t)X) & 15) && !(gemm_dbg() & LFM_DBG_LN_STORE8)) {  // flag: the 8-byte-store kernel (A/B)
    // ONE row per wave and the two row sums on the DPP network (r02_probe3: 17.0-17.2 us = 5.9 TB/s at M 16384 x D 1024; two rows per wave with
    // ds_bpermute sums -- the round-1 choice -- 20.4-20.9 us, one row with ds_bpermute 17.5-17.8 us, four rows 23.3-24.0 us).  A/B flags:
    // LN_BPERMUTE = one row + ds_bpermute sums, LN_TWO_ROWS, LN_FOUR_ROWS.
    const int f = gemm_dbg();
    if (f & LFM_DBG_LN_BPERMUTE) hipLaunchKernelGGL(ln_modulate8_kernel<1>, dim3(cdiv(M, 4)), dim3(256), 0, st, X, A, M, D, tokens, shift, scale, stride);
    else if (f & LFM_DBG_LN_TWO_ROWS) hipLaunchKernelGGL(ln_modulate8_kernel<2>, dim3(cdiv(M, 8)), dim3(256), 0, st, X, A, M, D, tokens, shift, scale, stride);
    else if (f & LFM_DBG_LN_FOUR_ROWS) hipLaunchKernelGGL(ln_modulate8_kernel<4>, dim3(cdiv(M, 16)), dim3(256), 0, st, X, A, M, D, tokens, shift, scale, stride);
    else hipLaunchKernelGGL((ln_modulate8_kernel<1, true>), dim3(cdiv(M, 4)), dim3(256), 0, st, X, A, M, D, tokens, shift, scale, stride);
    LFM_CHECK_LAUNCH();
    return LFM_OK;
  }
  hipLaunchKernelGGL(ln_modulate_kernel, dim3(cdiv(M, 4 * LN_ROWS)), dim3(256), 0, st, X, A, M, D, tokens, shift, scale, stride);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_ln_modulate(const float* X, void* A, int M, int D, int tokens, const float* shift, const float* scale, long mod_stride,
                               lfm_stream_t stream) {
  if (!X || !A || !shift || !scale) return LFM_ERR_ARG;
  if (M <= 0 || tokens <= 0) return LFM_ERR_SHAPE;
  return ln_modulate_launch(X, (half_t*)A, M, D, tokens, shift, scale, mod_stride, (hipStream_t)stream);
}

extern "C" int lfm_gemm_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                            int epilogue, const float* gate, long gate_stride, int tokens, lfm_stream_t stream) {
  if (!A || !W || !C) return LFM_ERR_ARG;
  // every kernel moves 16-byte operand chunks, and every epilogue stores 4-element vectors at m * ldc + n: refused here, ahead of every shape check and launch
  if ((lda % 8) || (ldw % 8) || (ldc % 4) || (((uintptr_t)A | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  ASrcRowMajor a{(const half_t*)A, lda, M, 0};
  if (gemm_sel() == 7 || gemm_sel() == 8) {  // the latency-mode kernels on their own (parity tests): 7 = 64x64 tiles, 8 = all rows x 16 columns; <= 256 rows
    const int which = gemm_sel();
    auto lat = [&](const auto& e) {
      return which == 7 ? launch_gemm_sq64((const half_t*)A, lda, (const half_t*)W, ldw, M, N, K, e, 1, st)
                        : launch_gemm_skinny((const half_t*)A, lda, (const half_t*)W, ldw, M, N, K, e, 1, st);
    };
    switch (epilogue) {
      case 0: return lat(EpiBiasF16{(half_t*)C, ldc, bias});
      case 1: return bias ? lat(EpiBiasGeluF16{(half_t*)C, ldc, bias}) : LFM_ERR_ARG;
      case 2: return lat(EpiBiasF32{(float*)C, ldc, bias});
      default: return LFM_ERR_ARG;
    }
  }
  switch (epilogue) {
    case 0: return gemm_f16_launch(a, (const half_t*)W, ldw, M, N, K, EpiBiasF16{(half_t*)C, ldc, bias}, st);
    case 1: return bias ? gemm_f16_launch(a, (const half_t*)W, ldw, M, N, K, EpiBiasGeluF16{(half_t*)C, ldc, bias}, st) : LFM_ERR_ARG;
    case 2: return launch_gemm_auto(a, (const half_t*)W, ldw, M, N, K, EpiBiasF32{(float*)C, ldc, bias}, st);  // (no stamped build of this epilogue)
    case 3:
      if (!bias || !gate || tokens <= 0) return LFM_ERR_ARG;
      return gemm_f16_launch(a, (const half_t*)W, ldw, M, N, K, EpiGateResidF32{(float*)C, ldc, bias, gate, gate_stride, tokens}, st);
  }
  return LFM_ERR_ARG;
}

extern "C" int lfm_gemm_qkv_f16(const void* A, long lda, const void* W, long ldw, void* Q, void* Kout, void* Vt, int M, int D, int K,
                                const float* bias, int head_dim, int tokens, lfm_stream_t stream) {
  if (!A || !W || !Q || !Kout || !Vt || !bias) return LFM_ERR_ARG;
  if ((lda % 8) || (ldw % 8) || (((uintptr_t)A | (uintptr_t)W) & 15)) return LFM_ERR_ALIGN;
  if (head_dim <= 0 || tokens <= 0 || (D % head_dim) || (head_dim % 8) || (tokens % 16) || (M % tokens)) return LFM_ERR_SHAPE;  // 16: the V^T token groups (vt_pos)
  return gemm_f16_launch(ASrcRowMajor{(const half_t*)A, lda, M, 0}, (const half_t*)W, ldw, M, 3 * D, K,
                         EpiQKV::make((half_t*)Q, (half_t*)Kout, (half_t*)Vt, bias, D, head_dim, tokens), (hipStream_t)stream);
}

// ------------------------------------------------------------------ conditioning (everything the forward derives from t and y alone)
// c = t_emb(t) (+ y_emb), the adaLN modulation rows of every block and of the final layer (DiT.py:252-262, 128, 170) and -- for the folded
// LayerNorm path -- the u / v rows of the qkv and fc1 projections (gemm_epilogues.h).  One function, so that the per-grid tables below are written by
// exactly the launches a forward would make.
static int dit_conditioning(const lfm_dit_shape* s, const lfm_dit_weights* w, const DitWs& ws, const DitDims& d, const float* t, int t_len, const int64_t* y,
                            int rows, bool want_uv, hipStream_t st) {
  const int D = d.D, H = d.H;
  const long J = d.J, mstride = rows == 1 ? 0 : J;
  hipLaunchKernelGGL(temb1_kernel, dim3(cdiv(D, 4), t_len), dim3(256), 0, st, t, w->t_w0, w->t_b0, ws.temb_h, D);
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(temb2_kernel, dim3(cdiv(D, 4), t_len), dim3(256), 0, st, ws.temb_h, w->t_w2, w->t_b2, ws.temb, D);
  LFM_CHECK_LAUNCH();
  hipLaunchKernelGGL(cond_kernel, dim3(cdiv((long)rows * D, 256)), dim3(256), 0, st, ws.temb, t_len, w->y_table, y, s->label_rows, ws.c_half, D, rows);
  LFM_CHECK_LAUNCH();
  int rc = launch_gemm_tn(ASrcRowMajor{ws.c_half, D, rows, 0}, (const half_t*)w->ada_w, D, rows, (int)J, D, EpiBiasF32{ws.mod, J, w->ada_b}, st);
  if (rc || !want_uv) return rc;
  if (rows == 1 && D <= 8 * 64 * LN_MAXP) {  // one shared conditioning row: weight-streaming GEMVs (u, v of every block)
    hipLaunchKernelGGL(uv_gemv_kernel, dim3(cdiv(3 * D, 4 * UV_ROWS), s->depth), dim3(256), 0, st, (const half_t*)w->qkv_w, w->qkv_b, ws.mod, 3 * D, D, D, 0,
                       ws.uvq);
    LFM_CHECK_LAUNCH();
    hipLaunchKernelGGL(uv_gemv_kernel, dim3(cdiv(H, 4 * UV_ROWS), s->depth), dim3(256), 0, st, (const half_t*)w->fc1_w, w->fc1_b, ws.mod, H, D, 4 * D, 3 * D,
                       ws.uvf);
    LFM_CHECK_LAUNCH();
    return LFM_OK;
  }
  const long nmod = (long)s->depth * 4 * rows * (D / 4);
  hipLaunchKernelGGL(mod_rows_f16_kernel, dim3(cdiv(nmod, 256)), dim3(256), 0, st, ws.mod, mstride, s->depth, rows, D, ws.amod);
  LFM_CHECK_LAUNCH();
  // u, v of every block in two batched GEMMs (batch = depth): [2 rows x D] x [D x 3D] and [2 rows x D] x [D x H]
  rc = launch_gemm_auto(ASrcRowMajor{ws.amod, D, 2 * rows, 0}, (const half_t*)w->qkv_w, D, 2 * rows, 3 * D, D, EpiUV{ws.uvq, 3L * D, w->qkv_b, rows, 3L * D}, st,
                        s->depth, 4L * rows * D, 3L * D * D, 2L * rows * 3 * D);
  if (rc) return rc;
  return launch_gemm_auto(ASrcRowMajor{ws.amod + 2L * rows * D, D, 2 * rows, 0}, (const half_t*)w->fc1_w, D, 2 * rows, H, D,
                          EpiUV{ws.uvf, (long)H, w->fc1_b, rows, (long)H}, st, s->depth, 4L * rows * D, (long)H * D, 2L * rows * H);
}

// Per-grid conditioning tables (round 4).  For the unconditional models (one shared conditioning row: scalar t, no labels -- celeb256 / ffhq / bed /
// church_dit.txt) the conditioning is a pure function of the grid time, yet every evaluation re-streamed the adaLN table (304 MB of weights for
// DiT-L/2) and both u / v GEMVs: ~168 us = 1.6 % of an evaluation (profiles/r03_final_bench_kernel_stats.csv).  A table row holds, for one time,
// [mod: J floats | uvq: depth * 2 * 3D | uvf: depth * 2 * H]; rows are written by dit_conditioning itself (bit-identical to the per-evaluation path)
// and an evaluation copies its row into the workspace (one ~2 MB copy launch, cond_row_copy_kernel) -- the row index is read on the device, so one
// captured graph serves every interval of the grid.
static inline long cond_row_floats(const DitDims& d) { return d.J + d.uvq_n + d.uvf_n; }
static int dit_cond_copy(const DitWs& ws, const DitDims& d, const float* table, const int* step, int offset, int fixed_row, int to_table, hipStream_t st,
                         int rows = 0) {
  hipLaunchKernelGGL(cond_row_copy_kernel, dim3(cdiv(cond_row_floats(d) / 4, 256)), dim3(256), 0, st, table, cond_row_floats(d), step, offset, fixed_row, ws.mod,
                     d.J, ws.uvq, d.uvq_n, ws.uvf, d.uvf_n, to_table, rows);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" size_t lfm_dit_cond_table_bytes(const lfm_dit_shape* shape, int n_times) {
  if (check_shape(shape) != LFM_OK || n_times <= 0) return 0;
  return (size_t)cond_row_floats(dit_dims(shape, 1)) * 4 * (size_t)n_times;
}

extern "C" int lfm_dit_cond_table_build(const lfm_dit_shape* s, const lfm_dit_weights* w, void* workspace, size_t workspace_bytes, int batch,
                                        const float* t_values, int n_times, void* table, size_t table_bytes, lfm_stream_t stream) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (!w || !workspace || !t_values || !table || n_times <= 0 || batch <= 0) return LFM_ERR_ARG;
  if (table_bytes < lfm_dit_cond_table_bytes(s, n_times)) return LFM_ERR_WORKSPACE;
  const DitDims d = dit_dims(s, batch);
  const DitWs ws = carve(s, d, workspace);  // the buffers an evaluation at this batch would use (the conditioning part does not depend on it)
  if (ws.total > workspace_bytes) return LFM_ERR_WORKSPACE;
  if (((uintptr_t)workspace & 255) || ((uintptr_t)table & 15)) return LFM_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  for (int i = 0; i < n_times; ++i) {
    rc = dit_conditioning(s, w, ws, d, t_values + i, 1, nullptr, 1, dit_fold_capable(s), st);
    if (rc) return rc;
    rc = dit_cond_copy(ws, d, (const float*)table, nullptr, 0, i, 1, st, n_times);
    if (rc) return rc;
  }
  return LFM_OK;
}

// ------------------------------------------------------------------ the plan of one evaluation
// Every launch-shape decision of an evaluation, taken once: each setting is read ONCE here, on the calling thread and inside the call's scope (another host thread
// may store a default between two reads).  The launchers shared with the standalone entry points (ln_modulate_launch, attention_launch, gemm_choose) read theirs
// themselves.  The block loop is one of three:
//   folded    the adaLN LayerNorm-modulate folded into the GEMM epilogues (gemm_epilogues.h), optionally with QKV projection + attention as one kernel;
//   latency   one image of <= 256 tokens: the four linears on the latency-mode kernels (gemm_skinny_kernel.h / gemm_sq64_kernel.h);
//   separate  everything else: split-K GEMMs where they apply, else the automatic choice plus a LayerNorm-modulate launch.
enum DitLoop { DIT_LOOP_FOLDED, DIT_LOOP_LATENCY, DIT_LOOP_SEPARATE };
struct DitPlan {
  DitLoop loop;
  bool fold, w6, fused;    // folded loop; its GEMMs on the one-wave-per-SIMD kernel; QKV projection + attention in one kernel (lfm_dit_plan reports fold, fused)
  bool pe_mfma, fin_mfma;  // patch embedding / final layer on their MFMA kernels
  bool sq64;               // latency loop: the 64x64-tile kernel (else all rows x 16 columns) ...
  int s_proj, s_fc2;       // ... and the K slices of proj / fc2
};
// Without the workspace and the weights (lfm_dit_plan: host only) the choice between the latency and the separate loop stays open.
static DitPlan dit_plan(const lfm_dit_shape* s, const DitDims& d, int rows, const DitWs* ws = nullptr, const lfm_dit_weights* w = nullptr) {
  const int sel = gemm_sel(), dbg = gemm_dbg(), skinny = opt_get(g_def.skinny);
  const int D = d.D, H = d.H, T = d.T, M = d.M;
  DitPlan p{};
  // folded LayerNorm-modulate: only where its preconditions hold -- whole 256-row tiles of ONE image each (or one shared modulation row), row partials in D / 256
  // slots, all four GEMMs chip-filling on the 16x16x32 kernel
  p.fold = opt_fold_ln() && dit_fold_capable(s) && (M % 256 == 0) && (rows == 1 || T % 256 == 0) && (long)(M / 256) * d.tiles_p >= 192 && (sel == 0 || sel == 6) &&
           s->depth >= 1;
  p.w6 = sel == 6 || (sel == 0 && opt_get(g_def.v6));  // the block GEMMs of the folded path on the one-wave-per-SIMD kernel
  // QKV projection + attention in one kernel (qkv_attention_kernel.h): one (image, head) per work item -- images of exactly one 256-token tile, head_dim 64,
  // operands inside the unsigned 32-bit byte offsets of its LDS-DMAs
  p.fused = p.fold && opt_get(g_def.fused_qkv) && !p.w6 && T == 256 && D == s->heads * 64 && (long)M * D < (1L << 31) && (long)3 * D * D < (1L << 31);
  // the */2 patch embedding on MFMA, fused with the first LayerNorm of the forward (flag: the round-1 kernel)
  p.pe_mfma = s->patch == 2 && s->in_ch == 4 && (D % 256 == 0) && D <= 1280 && (s->res % 2 == 0) && !(dbg & LFM_DBG_DIT_PATCH_ROUND1);
  // the final layer as a skinny MFMA GEMM (16 rows per wave) when the shape allows it: whole 16-row tiles inside one image half, 16-column output tiles,
  // D % 32 == 0 (flag: the round-1 kernel, A/B)
  p.fin_mfma = (d.KK == 16 || d.KK == 64) && (D % 32 == 0) && (T % 16 == 0) && (M % 16 == 0) && !(dbg & LFM_DBG_DIT_FINAL_ROUND1);
  p.loop = p.fold ? DIT_LOOP_FOLDED : DIT_LOOP_SEPARATE;
  if (p.fold || !ws) return p;
  // latency loop: only where its kernels accept all four linears of a block.  proj / fc2 run as K slices (column tiles x slices ~ 256 workgroups, slabs must fit)
  // into the slabs of the row-owning finish + LayerNorm kernel; images of whole 64-token tiles take the 64x64 kernel (half the bytes per workgroup)
  auto slices = [&](bool sq, int N_, int K_) {
    const int wgs = sq ? (N_ / SQ_T) * (M / SQ_T) : N_ / SK_BN, bk = sq ? SQ_BK : SK_BK;
    int sl = 1;
    while (wgs * (sl * 2) <= 256 && (K_ % (sl * 2 * bk)) == 0 && K_ / (sl * 2) >= 2 * bk && (size_t)(sl * 2) * M * N_ * 4 <= ws->slab_bytes) sl *= 2;
    return sl;
  };
  p.sq64 = skinny == 1 && M >= SQ_T && (M % SQ_T) == 0 && gemm_sq64_ok(ws->A, D, w->qkv_w, D, M, 3 * D, D, 1) && gemm_sq64_ok(ws->A, D, w->fc1_w, D, M, H, D, 1) &&
           gemm_sq64_ok(ws->A, D, w->proj_w, D, M, D, D, slices(true, D, D)) && gemm_sq64_ok(ws->QKVH, H, w->fc2_w, H, M, D, H, slices(true, D, H));
  p.s_proj = slices(p.sq64, D, D);
  p.s_fc2 = slices(p.sq64, D, H);
  if (skinny && sel == 0 && M <= SK_ROWS && ws->slab && D <= 1024 * SPLITK_LN_MAXJ && (D % 4) == 0 && gemm_skinny_ok(ws->A, D, w->qkv_w, D, M, 3 * D, D, 1) &&
      gemm_skinny_ok(ws->A, D, w->fc1_w, D, M, H, D, 1) && gemm_skinny_ok(ws->A, D, w->proj_w, D, M, D, D, p.s_proj) &&
      gemm_skinny_ok(ws->QKVH, H, w->fc2_w, H, M, D, H, p.s_fc2))
    p.loop = DIT_LOOP_LATENCY;
  return p;
}
// The plan of an evaluation without launching it (tests; a caller that sizes its expectations): *plan_out = LFM_PLAN_* bits.  Same scope code as the forward.
extern "C" int lfm_dit_plan(const lfm_dit_shape* s, const lfm_dit_call* c, int* plan_out) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (!c || !plan_out) return LFM_ERR_ARG;
  const int B = c->batch;
  if (B <= 0 || (c->t_len != 1 && c->t_len != B)) return LFM_ERR_SHAPE;
  CallScope scope;
  if ((rc = call_scope_enter(c)) != LFM_OK) return rc;
  const DitPlan p = dit_plan(s, dit_dims(s, B), (c->t_len == 1 && !c->y) ? 1 : B);
  *plan_out = (p.fold ? LFM_PLAN_FOLDED_LN : 0) | (p.fused ? LFM_PLAN_FUSED_QKV_ATTENTION : 0);
  return LFM_OK;
}

// ------------------------------------------------------------------ the evaluation
// The operands of block i: its four weight matrices and biases, its six adaLN rows (DiT.py:128; images are mstride floats apart) and the two rows of the
// LayerNorm that FOLLOWS the block (block i + 1's shift_msa / scale_msa; not used after the last block).
struct BlockW {
  const half_t *qkv_w, *proj_w, *fc1_w, *fc2_w;
  const float *qkv_b, *proj_b, *fc1_b, *fc2_b;
  const float *shift_msa, *scale_msa, *gate_msa, *shift_mlp, *scale_mlp, *gate_mlp, *next_shift_msa, *next_scale_msa;
};
static BlockW block_weights(const lfm_dit_weights* w, const float* mod_rows, const DitDims& d, int i) {
  const size_t D = d.D, H = d.H, b = i;
  const float* mod = mod_rows + b * 6 * D;
  return BlockW{(const half_t*)w->qkv_w + b * 3 * D * D, (const half_t*)w->proj_w + b * D * D, (const half_t*)w->fc1_w + b * H * D, (const half_t*)w->fc2_w + b * D * H,
                w->qkv_b + b * 3 * D, w->proj_b + b * D, w->fc1_b + b * H, w->fc2_b + b * D,
                mod, mod + D, mod + 2 * D, mod + 3 * D, mod + 4 * D, mod + 5 * D, mod + 6 * D, mod + 7 * D};
}

// What the stages of one evaluation share; the stages themselves: embedding, one of the three block loops, final layer.
struct DitCtx : DitDims {
  const lfm_dit_shape* s;
  const lfm_dit_weights* w;
  const lfm_dit_call* c;
  const void* workspace;
  DitWs ws;
  DitPlan p;
  int rows;      // conditioning rows: one shared row when time is scalar and there are no labels
  long mstride;  // floats between the images' modulation rows (0: the shared row)
  hipStream_t st;
  half_t *Qb, *Kb, *Vb;  // ws.QKVH as Q | K | V^T
  bool prof_ok, chk;     // this evaluation owns the event probe; (measurement builds) it records per-kernel checksums (dit_measure.h)
  BlockW block(int i) const { return block_weights(w, ws.mod, *this, i); }
  void checksum(const void* buf, size_t bytes, int i, int slot) const { if (chk) dit_chk(buf, bytes, i, slot, st); }
  int embed() const, blocks_folded() const, blocks_latency() const, blocks_separate() const, final_layer() const;
};

// Patch embedding + position embedding -> X; on the folded path also the first LayerNorm's A', row partials and row means (cen[0]).
int DitCtx::embed() const {
  const int xmod = c->cfg ? B / 2 : B;
  if (p.pe_mfma) {  // (on the folded path it writes A', the partials and the row means itself)
    const int tpb = M <= 1024 ? 1 : 2;  // latency mode: twice the blocks (16 for one image), one 16-token tile each behind the weight-fragment prologue
    hipLaunchKernelGGL(patch_embed_ln_kernel, dim3(cdiv(M, 16 * tpb)), dim3(64 * (D / 256)), 0, st, c->x, w->patch_w, w->patch_b, w->pos_embed, ws.X,
                       M, xmod, s->res, D, tpb, p.fold ? ws.A : (half_t*)nullptr, ws.mod + D, mstride, ws.ln_part, tiles_p, ws.cen[0]);
    LFM_CHECK_LAUNCH();
  } else if (KK <= PE_MAXK) {
    hipLaunchKernelGGL(patch_embed_kernel, dim3(cdiv(M, PE_TOK)), dim3(D / 4), 0, st, c->x, w->patch_w, w->patch_b, w->pos_embed, ws.X, M,
                       xmod, s->in_ch, s->res, s->patch, D);
    LFM_CHECK_LAUNCH();
  } else {  // DiT-*/4, */8: patches -> fp16 A operand (in the LN buffer, free at this point), X = pos_embed, then X += patches W^T + bias on MFMA
    if (!w->patch_w16) return LFM_ERR_ARG;
    hipLaunchKernelGGL(patchify_kernel, dim3(M), dim3(256), 0, st, c->x, w->pos_embed, ws.A, ws.X, ws.ones, M, xmod, s->in_ch, s->res,
                       s->patch, D);
    LFM_CHECK_LAUNCH();
    const int rc = launch_gemm_auto(ASrcRowMajor{ws.A, KK, M, 0}, (const half_t*)w->patch_w16, KK, M, D, KK,
                                    EpiGateResidF32{ws.X, D, w->patch_b, ws.ones, 0, T}, st);
    if (rc) return rc;
  }
  if (p.fold && !p.pe_mfma) {
    hipLaunchKernelGGL(ln_center_mod_kernel, dim3(cdiv(M, 4)), dim3(256), 0, st, ws.X, ws.A, M, D, T, ws.mod + D, mstride, ws.ln_part, tiles_p,
                       ws.cen[0]);
    LFM_CHECK_LAUNCH();
  }
  return LFM_OK;
}

// FOLDED LayerNorm-modulate (default; gemm_epilogues.h): only where its preconditions hold (dit_plan).  Everything else (small batches, DiT-S / XL widths, patch 4 / 8
// token counts with per-image conditioning, forced kernels) takes the separate ln_modulate launches of the other two loops.
int DitCtx::blocks_folded() const {
  const long uvs_q = rows == 1 ? 0 : 3 * D, uvs_f = rows == 1 ? 0 : H;
  int rc, cen_cur = 0;
  auto rowstat_src = [&]() {  // consumer: reads cen[cen_cur], publishes the new row means into the other array, which becomes current
    RowStatSrc r{ws.ln_part, ws.cen[cen_cur], ws.cen[cen_cur ^ 1], tiles_p, 1.0f / (float)D, 1e-6f};
    cen_cur ^= 1;
    return r;
  };
  auto launch_fold = [&](const ASrcRowMajor& a, const half_t* Wp, long ldw_, int M_, int N_, int K_, const auto& e) {
    return p.w6 ? launch_gemm256w_tn(a, Wp, ldw_, M_, N_, K_, e, st) : launch_gemm256h_tn(a, Wp, ldw_, M_, N_, K_, e, st);
  };
  // attention output / proj operand `Ob` and the fc1 operand `A1b`: the two-kernel path reuses ws.A for O (the QKV GEMM is over); the fused kernel writes
  // an image's O while other heads of the image still read its A' rows, so O goes to ws.A2 and proj hands A' back through ws.A
  half_t *Ob = p.fused ? ws.A2 : ws.A, *A1b = p.fused ? ws.A : ws.A2;
  for (int i = 0; i < s->depth; ++i) {
    const BlockW b = block(i);
    const float *uq = ws.uvq + (long)i * 2 * rows * 3 * D, *uf = ws.uvf + (long)i * 2 * rows * H;
    if (p.fused) {
      const QkvAttnArgs e_qa{uq, uq + (long)rows * 3 * D, uvs_q, rowstat_src(), Ob, D, s->heads, 0.125f * 1.4426950408889634f, nullptr, 0};
      if ((rc = launch_qkv_attention(ws.A, D, b.qkv_w, D, M, D, s->heads, D, e_qa, st))) return rc;
    } else {
      const EpiQKVMod e_qkv{{}, Qb, Kb, Vb, uq, uq + (long)rows * 3 * D, uvs_q, D, hd, T, EpiQKV::log2_or_neg(T), rowstat_src(), nullptr, 0};
      if ((rc = launch_fold(ASrcRowMajor{ws.A, D, M, 0}, b.qkv_w, D, M, 3 * D, D, e_qkv))) return rc;
      checksum(ws.QKVH, (size_t)3 * M * D * 2, i, 0);
      if ((rc = attention_launch(Qb, Kb, Vb, Ob, B, s->heads, hd, T, st))) return rc;
    }
    checksum(Ob, (size_t)M * D * 2, i, 1);
    // proj: X += gate_msa * (.), A' for fc1 with scale_mlp, partials; c = the row means the qkv GEMM just published
    const EpiGateResidMod e_proj{ws.X, D, b.proj_b, b.gate_msa, mstride, T, A1b, b.scale_mlp, mstride, ws.cen[cen_cur], ws.ln_part, tiles_p};
    if ((rc = launch_fold(ASrcRowMajor{Ob, D, M, 0}, b.proj_w, D, M, D, D, e_proj))) return rc;
    checksum(ws.X, (size_t)M * D * 4, i, 2);
    checksum(A1b, (size_t)M * D * 2, i, 3);
    checksum(ws.ln_part, (size_t)M * tiles_p * 8, i, 4);
    const bool prof = prof_fc1_begin(prof_ok, st);
#if defined(LFM_MEASURE) && defined(LFM_EXP_DUMP)
    const EpiModGeluF16 e_fc1{ws.QKVH, H, uf, uf + (long)rows * H, uvs_f, T, rowstat_src(), nullptr, 0,
                              (g_dbg && workspace == g_dbg_ws) ? g_dbg + (long)i * g_dbg_stride : (float*)nullptr};
#else
    const EpiModGeluF16 e_fc1{ws.QKVH, H, uf, uf + (long)rows * H, uvs_f, T, rowstat_src(), nullptr, 0};
#endif
    if ((rc = launch_fold(ASrcRowMajor{A1b, D, M, 0}, b.fc1_w, D, M, H, D, e_fc1))) return rc;
    prof_fc1_end(prof, st);
    checksum(ws.QKVH, (size_t)M * H * 2, i, 5);
    const ASrcRowMajor a_fc2{ws.QKVH, H, M, 0};
    const EpiGateResidF32 e_fc2{ws.X, D, b.fc2_b, b.gate_mlp, mstride, T};
    // except after the last block, fc2 also writes the NEXT block's A' (its scale_msa)
    const EpiGateResidMod e_fc2_mod{e_fc2.X, D, e_fc2.bias, e_fc2.gate, mstride, T, ws.A, b.next_scale_msa, mstride, ws.cen[cen_cur], ws.ln_part, tiles_p};
    if ((rc = i + 1 < s->depth ? launch_fold(a_fc2, b.fc2_w, H, M, D, H, e_fc2_mod) : launch_fold(a_fc2, b.fc2_w, H, M, D, H, e_fc2))) return rc;
    checksum(ws.X, (size_t)M * D * 4, i, 6);
    checksum(ws.A, (size_t)M * D * 2, i, 7);
  }
  return LFM_OK;
}

// Latency mode (one image of <= 256 tokens): the four linears of a block on the latency-mode kernels: qkv / fc1 with their epilogues in the kernel, proj / fc2 as
// K slices into the slabs of the row-owning finish kernel, which is also the LayerNorm-modulate in front of the next linear (fc1; the next block's qkv).
int DitCtx::blocks_latency() const {
  auto lat_gemm = [&](const half_t* A_, const half_t* W_, int N_, int K_, const auto& epi_, int S_) {  // lda == ldw == K
    return p.sq64 ? launch_gemm_sq64(A_, (long)K_, W_, (long)K_, M, N_, K_, epi_, S_, st) : launch_gemm_skinny(A_, (long)K_, W_, (long)K_, M, N_, K_, epi_, S_, st);
  };
  auto finish = [&](int S_, const EpiGateResidF32& e, half_t* A_out, const float* shift, const float* scale) {  // X += gate * (slices + bias); A_out = LN-modulate(X)
    hipLaunchKernelGGL(splitk_finish_resid_ln_kernel, dim3(M), dim3(256), 0, st, ws.slab, S_, (long)M * D, D, e.X, e.ldx, e.bias, e.gate, e.gate_stride, e.tokens, A_out,
                       shift, scale, mstride);
    LFM_CHECK_LAUNCH();
    return LFM_OK;
  };
  const EpiSlabF32 e_slab{ws.slab, (long)D, (long)M * D};
  int rc = ln_modulate_launch(ws.X, ws.A, M, D, T, block(0).shift_msa, block(0).scale_msa, mstride, st);  // every later LayerNorm comes out of a finish kernel
  if (rc) return rc;
  for (int i = 0; i < s->depth; ++i) {
    const BlockW b = block(i);
    if ((rc = lat_gemm(ws.A, b.qkv_w, 3 * D, D, EpiQKV::make(Qb, Kb, Vb, b.qkv_b, D, hd, T), 1))) return rc;
    if ((rc = attention_launch(Qb, Kb, Vb, ws.A, B, s->heads, hd, T, st))) return rc;
    if ((rc = lat_gemm(ws.A, b.proj_w, D, D, e_slab, p.s_proj))) return rc;  // (consumes ws.A before the finish writes it)
    if ((rc = finish(p.s_proj, EpiGateResidF32{ws.X, D, b.proj_b, b.gate_msa, mstride, T}, ws.A, b.shift_mlp, b.scale_mlp))) return rc;
    const bool prof = prof_fc1_begin(prof_ok, st);
    if ((rc = lat_gemm(ws.A, b.fc1_w, H, D, EpiBiasGeluF16{ws.QKVH, H, b.fc1_b}, 1))) return rc;
    prof_fc1_end(prof, st);
    if ((rc = lat_gemm(ws.QKVH, b.fc2_w, D, H, e_slab, p.s_fc2))) return rc;
    // ... and, except after the last block, the LayerNorm in front of the NEXT block's qkv
    if ((rc = finish(p.s_fc2, EpiGateResidF32{ws.X, D, b.fc2_b, b.gate_mlp, mstride, T}, i + 1 < s->depth ? ws.A : nullptr, b.next_shift_msa, b.next_scale_msa))) return rc;
  }
  return LFM_OK;
}

// Everything else: each linear as a split-K GEMM where that applies (small M; the launcher answers 1 where it does not), else the automatic choice.  The split-K
// finish of proj / fc2 is also the LayerNorm-modulate in front of the next linear; the fall-back launches that LayerNorm on its own.
int DitCtx::blocks_separate() const {
  auto linear = [&](const half_t* W_, int N_, const auto& epi_) {  // ws.A [M, D] x W^T
    const int rc = launch_gemm_splitk(ws.A, D, W_, D, M, N_, D, epi_, ws.slab, ws.slab_bytes, st);
    return rc == 1 ? launch_gemm_auto(ASrcRowMajor{ws.A, D, M, 0}, W_, D, M, N_, D, epi_, st) : rc;
  };
  int rc;
  bool a_ready = false;  // the previous split-K finish already wrote this LayerNorm's output
  for (int i = 0; i < s->depth; ++i) {
    const BlockW b = block(i);
    if (!a_ready && (rc = ln_modulate_launch(ws.X, ws.A, M, D, T, b.shift_msa, b.scale_msa, mstride, st))) return rc;
    a_ready = false;
    if ((rc = linear(b.qkv_w, 3 * D, EpiQKV::make(Qb, Kb, Vb, b.qkv_b, D, hd, T)))) return rc;
    if ((rc = attention_launch(Qb, Kb, Vb, ws.A, B, s->heads, hd, T, st))) return rc;
    const EpiGateResidF32 e_proj{ws.X, D, b.proj_b, b.gate_msa, mstride, T};
    // (the finish's output ws.A is the slab GEMM's input: consumed before the finish writes it)
    rc = launch_gemm_splitk_resid_ln(ws.A, D, b.proj_w, D, M, D, D, e_proj, ws.A, b.shift_mlp, b.scale_mlp, mstride, ws.slab, ws.slab_bytes, st);
    if (rc == 1) {
      if ((rc = launch_gemm_auto(ASrcRowMajor{ws.A, D, M, 0}, b.proj_w, D, M, D, D, e_proj, st))) return rc;
      rc = ln_modulate_launch(ws.X, ws.A, M, D, T, b.shift_mlp, b.scale_mlp, mstride, st);
    }
    if (rc) return rc;
    const bool prof = prof_fc1_begin(prof_ok, st);
    if ((rc = linear(b.fc1_w, H, EpiBiasGeluF16{ws.QKVH, H, b.fc1_b}))) return rc;
    prof_fc1_end(prof, st);
    const EpiGateResidF32 e_fc2{ws.X, D, b.fc2_b, b.gate_mlp, mstride, T};
    const bool more = i + 1 < s->depth;  // ... and the one in front of the NEXT block's qkv (its shift_msa / scale_msa)
    rc = launch_gemm_splitk_resid_ln(ws.QKVH, H, b.fc2_w, H, M, D, H, e_fc2, more ? ws.A : (half_t*)nullptr, b.next_shift_msa, b.next_scale_msa, mstride, ws.slab,
                                     ws.slab_bytes, st);
    if (rc == LFM_OK) a_ready = more;
    if (rc == 1) rc = launch_gemm_auto(ASrcRowMajor{ws.QKVH, H, M, 0}, b.fc2_w, H, M, D, H, e_fc2, st);
    if (rc) return rc;
  }
  return LFM_OK;
}

// Final LayerNorm-modulate + linear + unpatchify, the CFG combine and the solver update (dit_kernels.h).
int DitCtx::final_layer() const {
  const bool cfg = c->cfg != 0;
  const float* fmod = ws.mod + (long)s->depth * 6 * D;
  const int Mh = cfg ? M / 2 : M;
  // all six kernels have one signature; the MFMA ones take one block per 16-row tile, with 1 / 4 column tiles for 16 / 64 outputs per token
  auto kernel = p.fin_mfma ? (cfg ? (KK == 16 ? final_layer_mfma_kernel<true, 1> : final_layer_mfma_kernel<true, 4>)
                                  : (KK == 16 ? final_layer_mfma_kernel<false, 1> : final_layer_mfma_kernel<false, 4>))
                           : (cfg ? final_layer_kernel<true> : final_layer_kernel<false>);
  const long blocks = p.fin_mfma ? (cfg ? Mh / 8 : M / 16) : cdiv(Mh, cfg ? 8 : 16);
  hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), 0, st, ws.X, M, D, T, fmod, fmod + D, mstride, w->final_w, w->final_b, s->in_ch, s->res, s->patch,
                     cfg ? c->cfg_scale : 1.0f, c->out, c->axpy_base, c->axpy_dt);
  LFM_CHECK_LAUNCH();
  return LFM_OK;
}

extern "C" int lfm_dit_forward(const lfm_dit_shape* s, const lfm_dit_weights* w, void* workspace, size_t workspace_bytes,
                               const lfm_dit_call* c, lfm_stream_t stream) {
  int rc = check_shape(s);
  if (rc) return rc;
  if (!w || !workspace || !c || !c->x || !c->t || !c->out) return LFM_ERR_ARG;
  const int B = c->batch;
  if (B <= 0 || (c->t_len != 1 && c->t_len != B)) return LFM_ERR_SHAPE;
  if (c->cfg && (B & 1)) return LFM_ERR_SHAPE;
  if (c->axpy_base && !c->axpy_dt) return LFM_ERR_ARG;
  const DitDims d = dit_dims(s, B);
  const DitWs ws = carve(s, d, workspace);
  if (ws.total > workspace_bytes) return LFM_ERR_WORKSPACE;
  if ((uintptr_t)workspace & 255) return LFM_ERR_ALIGN;
  hipStream_t st = (hipStream_t)stream;
  // per-call settings (ABI 4): thread-local for the duration of this call, the library defaults are not touched
  CallScope scope;
  if ((rc = call_scope_enter(c)) != LFM_OK) return rc;
  const bool prof_ok = prof_claim(st);
  const int rows = (c->t_len == 1 && !c->y) ? 1 : B;
  const bool tab = c->cond_table != nullptr;  // everything derived from t alone comes from a per-grid table (lfm_dit_cond_table_build)
  if (tab && (rows != 1 || !c->cond_step)) return LFM_ERR_ARG;
  DitCtx x{d, s, w, c, workspace, ws, dit_plan(s, d, rows, &ws, w), rows, /* mstride */ rows == 1 ? 0 : d.J, st,
           /* Q | K | V^T */ ws.QKVH, ws.QKVH + (size_t)d.M * d.D, ws.QKVH + (size_t)2 * d.M * d.D, prof_ok, /* chk */ false};

  if (tab) rc = dit_cond_copy(ws, d, (const float*)c->cond_table, c->cond_step, c->cond_offset, 0, 0, st, c->cond_rows);
  else rc = dit_conditioning(s, w, ws, d, c->t, c->t_len, c->y, rows, x.p.fold, st);
  if (rc) return rc;
  if ((rc = x.embed()) != LFM_OK) return rc;
#ifdef LFM_MEASURE
  x.chk = g_chk && workspace == g_chk_ws;
  if (x.chk) (void)hipMemsetAsync(g_chk, 0, DIT_CHK_SLOTS * 8, st);
#endif
  const bool prof_blk = prof_ok && g_prof_blk_count < LFM_PROF_BLK_MAX;  // the event pair around the whole block loop
  if (prof_blk) (void)hipEventRecord(g_prof_blk_ev[2 * g_prof_blk_count], st);
  switch (x.p.loop) {
    case DIT_LOOP_FOLDED: rc = x.blocks_folded(); break;
    case DIT_LOOP_LATENCY: rc = x.blocks_latency(); break;
    case DIT_LOOP_SEPARATE: rc = x.blocks_separate(); break;
  }
  if (rc) return rc;
  if (prof_blk) (void)hipEventRecord(g_prof_blk_ev[2 * g_prof_blk_count++ + 1], st);
  return x.final_layer();
}
