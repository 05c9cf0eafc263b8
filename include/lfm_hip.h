/* liblfm_hip.so -- C ABI of the MI355X (gfx950) sampling hot path of LFM.
 *
 * The reference (VinAIResearch/LFM) is pure Python and has no FFI; the drop-in boundary is the Python
 * surface (create_network / model(t, x, y) / sample_from_model / AutoencoderKL.decode).  This header is
 * the C boundary UNDER that surface: each entry point names the reference function it replaces
 * (paths relative to the reference checkout).  INTEGRATION.md shows the ctypes stub a maintainer of
 * the reference would add.
 *
 * Conventions (all entry points):
 *   - plain pointers + sizes; every pointer is a DEVICE pointer unless named host_*;
 *   - the caller owns every buffer, including the workspace (no allocation, no sync, no throw);
 *   - work is enqueued on `stream` (a hipStream_t passed as void*), so calls are graph-capturable;
 *   - return 0 on success, a negative LFM_ERR_* otherwise (see lfm_strerror).
 */
#ifndef LFM_HIP_H
#define LFM_HIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* lfm_stream_t; /* hipStream_t */

#define LFM_OK 0
#define LFM_ERR_SHAPE (-1)
#define LFM_ERR_ALIGN (-2)
#define LFM_ERR_WORKSPACE (-3)
#define LFM_ERR_LAUNCH (-4)
#define LFM_ERR_ARG (-5)

const char* lfm_strerror(int code);
/* The ABI this header describes.  The call structs below GROW between ABI versions (lfm_dit_call gained fields in 3 and 4) and the library reads every
 * field of the struct it is handed, so a caller compiled against an older header would pass a struct that is too short: a C / cgo / JNI caller checks
 * `lfm_abi_version() == LFM_ABI_VERSION` ONCE, after loading the library and before the first call (the Python binding refuses a mismatching library at
 * load time: lfm_amd/hip.py; tests/test_c_abi.py does it from C). */
#define LFM_ABI_VERSION 4
int lfm_abi_version(void);

/* ------------------------------------------------------------------ DiT velocity field
 * Shape of one DiT (models/DiT.py:157-184, configs :354-415). */
typedef struct lfm_dit_shape {
  int depth;      /* number of DiTBlocks */
  int hidden;     /* D */
  int heads;      /* head_dim = D / heads must be 64 or 72 (DiT-S / B / L: 64; DiT-XL: 1152 / 16 = 72) */
  int patch;      /* p: 2 (register patch-embed kernel), 4 or 8 (p*p*C % 64 == 0: patch embedding on the MFMA GEMM) */
  int in_ch;      /* C (4 for f8 latents) */
  int res;        /* latent side R = image_size / f */
  int mlp_hidden; /* int(D * mlp_ratio) */
  int label_rows; /* rows of y_embedder.embedding_table = num_classes + (label_dropout > 0) */
} lfm_dit_shape;

/* Packed weights.  fp16 tensors are the GEMM operands, row-major [out, in] exactly like nn.Linear;
 * everything else stays fp32.  J = depth*6*D + 2*D: the adaLN_modulation.1 rows of blocks 0..depth-1
 * (shift_msa, scale_msa, gate_msa, shift_mlp, scale_mlp, gate_mlp; models/DiT.py:128) followed by
 * final_layer.adaLN_modulation.1 (shift, scale; :146). */
typedef struct lfm_dit_weights {
  const float* pos_embed; /* [T, D]            pos_embed (models/DiT.py:184,203-205)                  */
  const float* patch_w;   /* [D, C*p*p]        x_embedder.proj.weight flattened (c, p, q)             */
  const float* patch_b;   /* [D]                                                                      */
  const float* t_w0;      /* [D, 256]          t_embedder.mlp.0                                       */
  const float* t_b0;      /* [D]                                                                      */
  const float* t_w2;      /* [D, D]            t_embedder.mlp.2                                       */
  const float* t_b2;      /* [D]                                                                      */
  const float* y_table;   /* [label_rows, D]   y_embedder.embedding_table.weight                      */
  const void* ada_w;      /* fp16 [J, D]                                                              */
  const float* ada_b;     /* [J]                                                                      */
  const void* qkv_w;      /* fp16 [depth, 3D, D]   blocks.i.attn.qkv.weight                           */
  const float* qkv_b;     /* [depth, 3D]                                                              */
  const void* proj_w;     /* fp16 [depth, D, D]    blocks.i.attn.proj.weight                          */
  const float* proj_b;    /* [depth, D]                                                               */
  const void* fc1_w;      /* fp16 [depth, H, D]    blocks.i.mlp.fc1.weight                            */
  const float* fc1_b;     /* [depth, H]                                                               */
  const void* fc2_w;      /* fp16 [depth, D, H]    blocks.i.mlp.fc2.weight                            */
  const float* fc2_b;     /* [depth, D]                                                               */
  const float* final_w;   /* [p*p*C, D]        final_layer.linear.weight                              */
  const float* final_b;   /* [p*p*C]                                                                  */
  const void* patch_w16;  /* fp16 [D, C*p*p]: x_embedder.proj.weight as a GEMM operand; needed when p*p*C > 16 (DiT-x/4, x/8), else may be NULL */
} lfm_dit_weights;

/* One evaluation of the velocity field, with the solver update optionally fused into the last kernel. */
typedef struct lfm_dit_call {
  int batch;              /* rows the network evaluates (already doubled under CFG)                   */
  const float* x;         /* [batch, C, R, R] fp32 NCHW                                               */
  const float* t;         /* [t_len] fp32, t_len = 1 (0-d / [1] time) or batch                        */
  int t_len;
  const int64_t* y;       /* [batch] class labels in [0, label_rows) (else the row is NaN), or NULL => row label_rows-1 (models/DiT.py:259-260) */
  int cfg;                /* 0: DiT.forward.  1: DiT.forward_with_cfg (models/DiT.py:274-290): rows
                             [0,batch/2) of x are used for BOTH halves, and both output halves carry
                             uncond + cfg_scale*(cond - uncond)                                        */
  float cfg_scale;
  float* out;             /* [batch, C, R, R]                                                         */
  const float* axpy_base; /* NULL: out = v.   else out = axpy_base + (*axpy_dt) * v  (may alias out)  */
  const float* axpy_dt;   /* device scalar (read at kernel run time => one captured graph per solver) */
  /* ABI 3: per-grid conditioning table (lfm_dit_cond_table_build), or NULL.  Only for evaluations with ONE shared conditioning row (t_len == 1, y == NULL):
   * everything the forward derives from t alone is then copied from table row *cond_step + cond_offset instead of being recomputed; t is not read. */
  const void* cond_table;
  const int* cond_step;   /* device int (a fixed-grid solver's interval counter) */
  int cond_offset;
  /* ABI 4.  Callers ZERO-INITIALISE the struct (memset / `= {0}`): every field below reads 0 as "as before". */
  int cond_rows;          /* rows of cond_table (the n_times it was built with).  > 0: a row index *cond_step + cond_offset outside [0, cond_rows) is not
                             read -- the evaluation's conditioning, and with it its output, becomes NaN (a kernel cannot return an error); 0: unchecked */
  int fold_ln;            /* per-call LFM_OPT_FOLD_LN: 0 = the library default (lfm_set_option), LFM_CALL_OFF = separate LayerNorm launches, LFM_CALL_ON = folded */
  int gemm_select;        /* per-call kernel selection: 0 = the library default (lfm_gemm_select), else LFM_CALL_GEMM_SELECT(value lfm_gemm_select would take) */
} lfm_dit_call;
#define LFM_CALL_OFF 1
#define LFM_CALL_ON 2
#define LFM_CALL_GEMM_SELECT(which) ((which) + 1)

/* Bytes of caller-owned scratch for batches up to max_batch: residual stream, LN / attention buffers, Q|K|Vt (reused for the fc1
 * activation), conditioning vectors, the adaLN table and -- for small batches (<= 1024 tokens, latency mode) -- the fp32 slabs of the
 * split-K GEMMs (reserved for every max_batch, so the requirement is monotone: a workspace sized for max_batch serves every smaller batch). */
size_t lfm_dit_workspace_bytes(const lfm_dit_shape* shape, int max_batch);

/* Where an evaluation at `batch` keeps its intermediate results inside the workspace (tests and tools read them back after a forward): byte offsets of
 * X (fp32 [M, D] residual stream), A, A2 (fp16 [M, D]), QKVH (fp16: Q | K | Vt, later the [M, H] fc1 activation), mod (fp32 [rows, J]), ln_part
 * (fp32 [M][D / 256][2]), cen[0], cen[1] (fp32 [M]), uvq, uvf, in this order, into offsets_out[0 .. min(n, LFM_DIT_WS_BUFFERS)); 0 where the shape has no such
 * buffer (X itself is at 0).  The offsets depend on the batch of the CALL, not on the size of the workspace.  Returns LFM_DIT_WS_BUFFERS or an error; no
 * launch; usable without a GPU. */
#define LFM_DIT_WS_BUFFERS 10
int lfm_dit_workspace_layout(const lfm_dit_shape* shape, int batch, size_t* offsets_out, int n);

/* Replaces DiT.forward / DiT.forward_with_cfg (models/DiT.py:252-290) as called by the solver closure
 * `denoiser` (test_flow_latent.py:55-59) and sampler/karras_sample.py:42-46. */
int lfm_dit_forward(const lfm_dit_shape* shape, const lfm_dit_weights* w, void* workspace, size_t workspace_bytes,
                    const lfm_dit_call* call, lfm_stream_t stream);

/* Which form of the block loop lfm_dit_forward would take for `call` if it were enqueued by the calling thread now (library defaults, per-call fields, shape and
 * batch): *plan_out = LFM_PLAN_FOLDED_LN (adaLN LayerNorm-modulate folded into the GEMM epilogues: LFM_OPT_FOLD_LN) | LFM_PLAN_FUSED_QKV_ATTENTION (QKV projection
 * + attention core as one kernel: LFM_OPT_FUSED_QKV_ATTENTION).  Reads call->batch, t_len, y (NULL or not), fold_ln, gemm_select; no launch; usable without a GPU. */
#define LFM_PLAN_FOLDED_LN 1
#define LFM_PLAN_FUSED_QKV_ATTENTION 2
int lfm_dit_plan(const lfm_dit_shape* shape, const lfm_dit_call* call, int* plan_out);

/* Per-grid conditioning tables for the unconditional models (test_args/{celeb256,ffhq,bed,church}_dit.txt: num_classes 1, no labels, scalar t -- the
 * closure `denoiser` of test_flow_latent.py:55-59 calls model(t, x) with the solver's grid time): c = t_embedder(t), the adaLN modulation of every block and
 * of the final layer (models/DiT.py:128, 170, 259-262) and the u / v rows of the folded LayerNorm path are pure functions of t, so a fixed-grid solver
 * computes them ONCE per grid time.  Rows are written by the same launches an evaluation would make: results are bit-identical.
 * t_values: device [n_times]; table: device, lfm_dit_cond_table_bytes(shape, n_times) bytes, 16-byte aligned; workspace / batch: as for lfm_dit_forward
 * (scratch).  The table depends on the weights and on the grid, not on x. */
size_t lfm_dit_cond_table_bytes(const lfm_dit_shape* shape, int n_times);
int lfm_dit_cond_table_build(const lfm_dit_shape* shape, const lfm_dit_weights* w, void* workspace, size_t workspace_bytes, int batch, const float* t_values,
                             int n_times, void* table, size_t table_bytes, lfm_stream_t stream);

/* ------------------------------------------------------------------ building blocks (exported for parity tests)
 * C[M,N] (+)= A[M,K] * W[N,K]^T on MFMA, fp16 operands, fp32 accumulate.  epilogue:
 *   0: C fp16 = acc + bias          1: C fp16 = gelu_tanh(acc + bias)       2: C fp32 = acc + bias
 *   3: C fp32 += gate[m / tokens][n] * (acc + bias)   (gate row stride gate_stride, 0 = shared row)
 * Replaces the nn.Linear calls inside timm Attention/Mlp (models/DiT.py:120,124) and adaLN (:128).
 * Alignment (this entry point, lfm_gemm_qkv_f16 and lfm_linear*_f16 alike; LFM_ERR_ALIGN before any shape check or launch): A and W 16-byte aligned,
 * lda and ldw multiples of 8 (operands move in 16-byte chunks), ldc a multiple of 4 (every epilogue stores 4-element vectors at m * ldc + n; the
 * strides may exceed the row length).  K a multiple of the kernel's K-tile (64; 32 on the 256x128 kernel), N a multiple of 4: LFM_ERR_SHAPE. */
int lfm_gemm_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                 int epilogue, const float* gate, long gate_stride, int tokens, lfm_stream_t stream);

/* The attention input projection with its fused split (timm Attention.qkv + reshape/permute, models/DiT.py:120):
 * [Q | K | V] = A[M,K] * W[3D,K]^T + bias;  Q, K fp16 [M, D] row-major;  V is written TRANSPOSED per head as
 * Vt[M / tokens][D / head_dim][head_dim][tokens] (what lfm_dit_attention reads), with the tokens of every group of 16 stored in the order
 * 0 1 2 3 8 9 10 11 4 5 6 7 12 13 14 15 (position p of a row holds token p with bits 2 and 3 exchanged: the operand order of the attention kernel's
 * P V MFMA, csrc/gemm_kernel.h: vt_pos; ABI 3).  head_dim % 8 == 0, tokens % 16 == 0. */
int lfm_gemm_qkv_f16(const void* A, long lda, const void* W, long ldw, void* Q, void* K_out, void* Vt, int M, int D, int K,
                     const float* bias, int head_dim, int tokens, lfm_stream_t stream);

/* Scope of the three library-wide switches below (lfm_gemm_select, lfm_set_option, lfm_profile_fc1): they set process-wide DEFAULTS and are meant for
 * measurement and tests; they are read when a call is ENQUEUED, on the calling thread.  A caller that needs a setting for ONE evaluation -- two
 * lanes in flight, several host threads -- passes it in lfm_dit_call (fold_ln, gemm_select): the per-call values live in thread-local state for the
 * duration of lfm_dit_forward and never touch the defaults, so concurrent callers do not see each other's choices (tests/test_c_abi.py).
 * Kernel selection for the GEMMs: 0 = automatic (the 256x256 quadrant-phased kernel on 16x16x32 MFMAs for chip-filling shapes with K % 64 == 0,
 * the 256x128 two-workgroups-per-CU kernel for chip-filling shapes that are only 128 columns wide, the 128x128 kernel otherwise), 1 = force
 * 128x128, 4 = force 256x128, 5 = force 256x256 with eight waves, 6 = force 256x256 with one wave per SIMD (128x128 wave tiles; row-major A
 * operands, K % 64 == 0 -- other cases take kernel 5); 7 / 8 = lfm_gemm_f16 (epilogues 0-2, <= 256 rows) on the latency-mode kernels -- 64x64 tiles /
 * all rows x 16 columns -- which refuse other shapes, every other entry point treats them as 1 (other values are refused); | flags << 4 =
 * ablation / A-B switches (LFM_DBG_*, named one by one in lfm_amd/csrc/debug_flags.h).  For measurement and parity tests. */
int lfm_gemm_select(int which);
/* Which kernel (1, 4, 5 or 6) a GEMM of this shape runs on under the calling thread's current selection.  caps: bit 0 = the caller's instantiation can
 * take kernel 6 (row-major A operand, an epilogue without per-lane tile accumulators), bit 1 = the operands fit the 32-bit buffer offsets of the 256x256
 * kernels (below 2^31 elements).  No launch; usable without a GPU. */
int lfm_gemm_plan(int M, int N, int K, int batch, int caps);

/* Measurement only: when enabled, every eager lfm_dit_forward records a HIP event pair around each block's fc1 GEMM (the
 * dominant kernel); lfm_profile_fc1_read synchronises and returns the per-launch durations in ms (bench.py roofline row).  One stream at a time:
 * the first stream that launches an evaluation while the probe is on owns it; an evaluation enqueued on ANOTHER stream meanwhile is not recorded
 * and makes lfm_profile_fc1_read return LFM_ERR_ARG (event pairs of interleaved streams would time the other stream's kernels too). */
int lfm_profile_fc1(int enable);
/* With the same probe on, every recorded evaluation also brackets its WHOLE block loop (all DiTBlocks: qkv .. fc2, models/DiT.py:112-131) with one
 * event pair: host_ms_out receives one duration per evaluation (at most 16); block time = duration / depth (bench.py `roofline_block`).
 * lfm_profile_fc1(2) records ONLY these (no events between the block's kernels). */
int lfm_profile_blocks_read(float* host_ms_out, int max_n);
/* Library-wide options.  key 1 (LFM_OPT_FOLD_LN), value 0 / 1, default 1: modulate(LayerNorm(x), shift, scale) (models/DiT.py:20-21, 129-130) FOLDED
 * into the GEMM epilogues around it -- the gated-residual GEMMs (proj, fc2) emit the centred, (1 + scale)-weighted fp16 operand and per-row partial
 * sums, the consuming GEMMs (qkv, fc1) apply rstd, the mean correction and the shift term in their epilogues -- wherever the shape allows it
 * (residual width a multiple of 256, whole 256-row tiles of one image or one shared conditioning row, chip-filling batch); 0 = always the separate
 * lfm_ln_modulate launches (the path every other shape takes).  Same result up to fp16 rounding of the operand (tests/test_gpu_dit.py). */
#define LFM_OPT_FOLD_LN 1
/* key 2 (LFM_OPT_GEMM_V6), value 0 / 1: the chip-filling row-major GEMMs (the four linears of a DiT block) on the one-wave-per-SIMD 256x256 kernel
 * (csrc/gemm256w_kernel.h) instead of the eight-wave one.  Same accumulation order per output element: bit-identical results. */
#define LFM_OPT_GEMM_V6 2
/* key 4 (LFM_OPT_SKINNY_GEMM), value 0 / 1 / 2, default 1: evaluations of <= 256 token rows (ONE image of 256 tokens: --measure_time, test_flow_latent.py:223-246)
 * run the four linears of a DiTBlock on the latency-mode kernels -- 64x64 tiles (csrc/gemm_sq64_kernel.h) where the rows are whole 64-row tiles, else all rows x
 * 16 columns (csrc/gemm_skinny_kernel.h); 2 = always the latter; 0 = the split-K 128x128 path (A/B and parity tests). */
#define LFM_OPT_SKINNY_GEMM 4
/* key 5 (LFM_OPT_ATTENTION_STREAM), value 0 / 1, default 1: lfm_dit_attention at 256 tokens x head_dim 64 with more than 64 (image, head) items runs on persistent
 * workgroups that stream K / V^T of consecutive items through an LDS ring (csrc/attention_stream_kernel.h); 0 = one workgroup per item (csrc/attention_kernel.h).
 * Same arithmetic in the same order per query: bit-identical results (tests/test_gpu_dit.py). */
#define LFM_OPT_ATTENTION_STREAM 5
/* key 6 (LFM_OPT_FUSED_QKV_ATTENTION), value 0 / 1, default 1: on the folded path, at 256 tokens per image and head_dim 64, the QKV projection and the attention
 * core of a DiTBlock (models/DiT.py:120) run as ONE kernel -- a workgroup per (image, head) computes the head's 256 x 192 slice of the projection and attends on
 * it out of the LDS; Q, K, V never reach HBM (csrc/qkv_attention_kernel.h); 0 = two kernels.  Same arithmetic in the same order: bit-identical results. */
#define LFM_OPT_FUSED_QKV_ATTENTION 6
/* key 7 (LFM_OPT_UNET_ATTENTION_STREAM), value 0 / 1 / 2, default 1: lfm_attention_small_f16 runs the shapes that neither its resident MFMA kernel nor
 * its VALU kernel serves (ch % 16 == 0, ch <= 256, any token count) on the streamed kernel (csrc/unet_attention_stream_kernel.h).  0 = those shapes are
 * refused (LFM_ERR_SHAPE); 2 = EVERY shape with ch % 16 == 0, ch <= 256 takes the streamed kernel (parity tests and A/B only). */
#define LFM_OPT_UNET_ATTENTION_STREAM 7
/* key 8 (LFM_OPT_ATTENTION_TILED), value 0 / 1 / 2, default 1 (any other value: LFM_ERR_ARG): lfm_dit_attention_hd runs the token counts no other kernel serves --
 * T the square of a grid side that is a multiple of 4, 144 <= T <= 3600: 144, 400, 576, 784, 1296, ... (--image_size 192 / 320 / 384 / 448 / 576 with a DiT-x/2) --
 * on the tiled kernel (csrc/attention_tiled_kernel.h: T a runtime argument, 128 queries per workgroup, keys in stages of 64 through an LDS ring).  0 = those
 * token counts are refused (LFM_ERR_SHAPE, by lfm_dit_forward too); 2 = EVERY shape the kernel takes (head_dim 64 / 72, T % 16 == 0, 16 <= T < 4096) runs on
 * it, the ones other kernels own included (parity tests and A/B only). */
#define LFM_OPT_ATTENTION_TILED 8
int lfm_set_option(int key, int value);
/* The settings lfm_dit_forward would run `call` with if it were enqueued by the calling thread now (per-call fields over the library defaults):
 * *gemm_select_out = kernel | flags << 4, *fold_ln_out = 0 / 1.  No launch; usable without a GPU. */
int lfm_dit_call_settings(const lfm_dit_call* call, int* gemm_select_out, int* fold_ln_out);

/* Measurement aid (bench.py): the clock the chip sustains under matrix load.  `blocks` workgroups of 512 threads each stream iters x 64 MFMAs per wave on
 * pseudo-random fp16 operands between two s_memtime reads; ticks_out[blocks] (device) receives the tick count of every workgroup (one tick = one shader
 * cycle).  Sustained clock = ticks / the launch's wall time (HIP events around the call). */
int lfm_clock_probe(int blocks, int iters, unsigned long long* ticks_out, lfm_stream_t stream);

/* ---- measurement-only entry points: exported by LFM_MEASURE builds of the library only (LFM_MEASURE=1 python -m lfm_amd._build; tools/README.md) */
#ifdef LFM_MEASURE
/* Measurement only: s_memtime stamps written by the quadrant-phased GEMM (select flag LFM_DBG_TRACE_GEMM, csrc/debug_flags.h) after every barrier of block 0,
 * wave groups 0 and 1; host_out receives 2 x n_per_group values. */
int lfm_gemm_trace_read(unsigned long long* host_out, int n_per_group);
/* Measurement only: s_memtime stamps of the attention kernel's trace build (select field LFM_DBG_ATT_MODE = 3, csrc/debug_flags.h; slot map in csrc/attention_kernel.h). */
int lfm_attention_trace_read(unsigned long long* host_out, int n);
/* Measurement only (LFM_MEASURE builds, same trace build): per attention workgroup {HW_ID | XCC_ID << 32, start, loads landed, end} -- which CU it ran on
 * and when; host_out receives 4 x n_wg values (n_wg <= 2048). */
int lfm_attention_wg_trace_read(unsigned long long* host_out, int n_wg);
/* Measurement only: per-kernel checksums of the evaluations that run on `workspace` (csrc/dit.hip: slot [block][8]); tools/concurrency_ws_diff.py. */
int lfm_dit_chk_arm(const void* workspace);
int lfm_dit_chk_read(unsigned long long* host_out, int n);
#endif /* LFM_MEASURE */
int lfm_profile_fc1_read(float* host_ms_out, int max_n);

/* A fp16 [M,D] = LayerNorm(X fp32 [M,D], eps 1e-6, no affine) * (1 + scale[img]) + shift[img]
 * (models/DiT.py:20-21,119,121,129-130).  mod_stride = floats between images' rows (0 = shared). */
int lfm_ln_modulate(const float* X, void* A, int M, int D, int tokens, const float* shift, const float* scale, long mod_stride,
                    lfm_stream_t stream);

/* softmax(q k^T / sqrt(hd)) v for hd = 64, T in {16,64,128,256,1024} (timm Attention as called at models/DiT.py:120; 1024 = four key chunks of 256) or the
 * square of a grid side that is a multiple of 4 with 144 <= T <= 3600 (the tiled kernel, LFM_OPT_ATTENTION_TILED); 4096 tokens and more are refused.
 * Q,K: fp16 [batch*T, D] token-major; Vt: fp16 [batch, heads, hd, T] in the token order lfm_gemm_qkv_f16 writes (16-groups permuted); O: fp16 [batch*T, D]. */
int lfm_dit_attention(const void* Q, const void* K, const void* Vt, void* O, int batch, int heads, int T, lfm_stream_t stream);
/* The same with the head size as an argument: head_dim 64 (DiT-S / B / L) or 72 (DiT-XL/{2,4,8}: 1152 / 16, models/DiT.py:354-363);
 * D = heads * head_dim. */
int lfm_dit_attention_hd(const void* Q, const void* K, const void* Vt, void* O, int batch, int heads, int head_dim, int T,
                         lfm_stream_t stream);
/* Which kernel lfm_dit_attention_hd runs for this shape under the calling thread's flags and the library options, or LFM_ERR_SHAPE for a shape no kernel
 * serves: 1 = the 16-token kernel, 2 = one workgroup per (image, head) item, 3 = the same with four waves x 64 queries (flag LFM_DBG_ATT_WIDE), 4 = four key
 * chunks (1024 tokens), 5 = the latency-mode query split (256 tokens x head_dim 64, at most 64 items), 6 = the streamed kernel (LFM_OPT_ATTENTION_STREAM;
 * more than 64 items, each tensor below 2 GiB), 7 = the tiled any-T kernel (LFM_OPT_ATTENTION_TILED: by default the square grids of a side that is a multiple of
 * 4 from 144 to 3600 tokens that 2 .. 6 do not serve).  No launch; usable without a GPU. */
int lfm_attention_plan(int batch, int heads, int head_dim, int T);

/* ------------------------------------------------------------------ first-stage VAE decoder
 * Decode half of diffusers AutoencoderKL, config stabilityai/sd-vae-ft-mse (latent 4, block_out_channels
 * [128,256,512,512], 2 layers/block, 32 GN groups, eps 1e-6), as the reference calls it:
 *   test_flow_latent.py:131,193   first_stage_model.decode(fake_sample / args.scale_factor).sample
 * conv3x3 weights are fp16 [Cout][tap = ky*3+kx][Cin]; 1x1 / linear weights fp16 [Cout][Cin]; GN affine and
 * biases fp32.  NULL sc_w = identity shortcut. */
typedef struct lfm_vae_resnet {
  const float* n1_g; const float* n1_b; const void* c1_w; const float* c1_b;
  const float* n2_g; const float* n2_b; const void* c2_w; const float* c2_b;
  const void* sc_w; const float* sc_b;
  int cin, cout;
} lfm_vae_resnet;

typedef struct lfm_vae_weights {
  const float* pq_w; const float* pq_b;   /* post_quant_conv [4,4], [4]           fp32 */
  const float* cin_w; const float* cin_b; /* decoder.conv_in [512,4,3,3], [512]   fp32 */
  lfm_vae_resnet mid[2];                  /* decoder.mid_block.resnets.{0,1}           */
  const float* at_g; const float* at_b;   /* decoder.mid_block.attentions.0.group_norm */
  const void* q_w; const float* q_b; const void* k_w; const float* k_b;
  const void* v_w; const float* v_b; const void* o_w; const float* o_b;   /* to_q/to_k/to_v/to_out.0 */
  lfm_vae_resnet up[4][3];                /* decoder.up_blocks.i.resnets.j             */
  const void* ups_w[3]; const float* ups_b[3]; /* decoder.up_blocks.i.upsamplers.0.conv */
  const float* no_g; const float* no_b;   /* decoder.conv_norm_out                     */
  const void* cout_w; const float* cout_b; /* decoder.conv_out padded to 4 outputs: fp16 [4][9][128], fp32 [4] */
} lfm_vae_weights;

/* Every VAE entry point lays its workspace out in one order -- four rotating activation buffers, {mean, rstd} per image and group, the partial
 * GroupNorm statistics in 8-byte {mean, M2} pairs, 256 B of zeros, the attention scores -- each piece rounded up to 256 bytes (a(v) below), a piece
 * the call does not use left out.
 * lfm_vae_workspace_bytes(R, c) = 4 a(c (8R)^2 512) + a(c 256) + a(c max((8R)^2 / 2, 8192) 8) + 256 + a(c R^4 4); 0 if R <= 0, c <= 0 or R % 8. */
size_t lfm_vae_workspace_bytes(int R, int chunk);

/* out[N,3,8R,8R] fp32 NCHW = decode(z[N,4,R,R] fp32 NCHW); images are processed `chunk` at a time so the
 * activation working set (4 x chunk x (8R)^2 x 256 fp16) stays bounded. */
int lfm_vae_decode(const lfm_vae_weights* w, void* workspace, size_t workspace_bytes, const float* z, float* out, int N, int R,
                   int chunk, lfm_stream_t stream);

/* Encoder half (diffusers AutoencoderKL.encode as called at train_flow_latent.py:143 and
 * downstream_tasks/test_flow_latent_inpainting.py:146).  fp16 tensors are GEMM operands [Cout][tap][Cin]. */
typedef struct lfm_vae_enc_weights {
  const float* cin_w; const float* cin_b;   /* encoder.conv_in [128,3,3,3], [128]         fp32 */
  lfm_vae_resnet down[4][2];                /* encoder.down_blocks.i.resnets.j                 */
  const void* ds_w[3]; const float* ds_b[3]; /* encoder.down_blocks.i.downsamplers.0.conv (stride 2, pad (0,1,0,1)) */
  lfm_vae_resnet mid[2];                    /* encoder.mid_block.resnets.{0,1}                 */
  const float* at_g; const float* at_b;     /* encoder.mid_block.attentions.0.group_norm       */
  const void* q_w; const float* q_b; const void* k_w; const float* k_b;
  const void* v_w; const float* v_b; const void* o_w; const float* o_b;
  const float* no_g; const float* no_b;     /* encoder.conv_norm_out                           */
  const void* cout_w; const float* cout_b;  /* quant_conv o encoder.conv_out folded: fp16 [8][9][512], fp32 [8] */
} lfm_vae_enc_weights;

/* moments[N,8,R,R] fp32 NCHW (mean | log-variance of the latent distribution) = quant_conv(Encoder(x)), x[N,3,8R,8R] fp32 NCHW.
 * Workspace: lfm_vae_workspace_bytes(R, chunk), as for the decoder. */
int lfm_vae_encode(const lfm_vae_enc_weights* w, void* workspace, size_t workspace_bytes, const float* x, float* moments, int N, int R,
                   int chunk, lfm_stream_t stream);

/* Test entry points for the decoder's GroupNorm (32 groups, eps 1e-6), running the decoder's own host code.  Workspace (256-byte aligned):
 * 256 B + n x 256 B (rounded up to 256) + the partial-statistics room in 8-byte pairs, used in whole 256-byte pieces -- the decoder gives
 * lfm_vae_workspace_bytes' share, and the statistics pass takes up to 512 slabs per image when n < 16 and that room allows it, else 64 (at least
 * n x 64 x C / 4 pairs are required).
 * lfm_vae_groupnorm_f16: y = silu?(GroupNorm(x) * gamma + beta), x, y fp16 NHWC [n, HW, C], C in {128, 256, 512}; statistics by their own pass. */
int lfm_vae_groupnorm_f16(const void* x, void* y, const float* gamma, const float* beta, void* workspace, size_t workspace_bytes, int n, int HW, int C,
                          int silu, lfm_stream_t stream);
/* The statistics slabs per image lfm_vae_groupnorm_f16's own pass takes for this shape with a workspace of workspace_bytes (the decoder's slab policy:
 * 64 at most, or up to 512 of at least 64 pixels when n < 16 and the room allows it); LFM_ERR_SHAPE / LFM_ERR_WORKSPACE exactly where that entry point
 * refuses the shape / the workspace size.  No launch; usable without a GPU.  Addition to ABI 4. */
int lfm_vae_groupnorm_plan(int n, int HW, int C, size_t workspace_bytes);
/* conv_out = conv3x3(in (nearest-2x upsampled when ups)) + bias (+ resid), then y = silu?(GroupNorm(conv_out) * gamma + beta), as a decoder resnet
 * hands a convolution to its GroupNorm: w fp16 [Cout][9][Cin], H, W the output size.  Needs also n x 2 (H W / 256) x Cout / 4 pairs of room.
 * *stat_slabs = the statistics slabs per image the convolution left (0: the GroupNorm ran its own pass); *stat_kernel = 1 (halo-tiled convolution),
 * 2 (256-row implicit GEMM) or 0.  Either pointer may be NULL. */
int lfm_vae_conv3x3_gn_f16(const void* in, const void* w, const float* bias, const void* resid, void* conv_out, void* y, const float* gamma,
                           const float* beta, void* workspace, size_t workspace_bytes, int n, int H, int W, int Cin, int Cout, int ups, int silu,
                           int* stat_slabs, int* stat_kernel, lfm_stream_t stream);
/* Test entry point for the mid-block attention of the decoder and the encoder, running their own host code (GroupNorm -> q, k, v -> softmax(q k^T / sqrt(512)) v
 * -> to_out + x): x, out fp16 NHWC [n, T, 512]; weights fp16 [512][512] row-major [out][in] as lfm_vae_weights holds them; biases and GroupNorm
 * parameters fp32; all 16-byte aligned.  T % 64 == 0 (the decoder's T = R^2 with R % 8 == 0).  Workspace (256-byte aligned):
 * lfm_vae_mid_attention_workspace_bytes(n, T) = 256 + a(n 256) + a(n max(32 T, 8192) 8) + 4 a(n T (512 + max(512, T)) 2) + a(n T^2 4), the
 * statistics room being the decoder's share per image at R^2 = T; 0 if n <= 0, T <= 0 or T % 64. */
size_t lfm_vae_mid_attention_workspace_bytes(int n, int T);
int lfm_vae_mid_attention_f16(const void* x, void* out, const float* gn_gamma, const float* gn_beta, const void* q_w, const float* q_b,
                              const void* k_w, const float* k_b, const void* v_w, const float* v_b, const void* o_w, const float* o_b,
                              void* workspace, size_t workspace_bytes, int n, int T, lfm_stream_t stream);
/* Test entry points for four more stages of the first-stage VAE, each running the decoder's / encoder's own host code on the caller's buffers.  Additions
 * to ABI 4.  All refuse before any launch: a null pointer (LFM_ERR_ARG), a shape outside the stated limits (LFM_ERR_SHAPE), a tensor that is not 16-byte
 * or a workspace that is not 256-byte aligned (LFM_ERR_ALIGN), a workspace below *_workspace_bytes (LFM_ERR_WORKSPACE; 0 for a refused shape).
 * Every VAE entry point with a workspace refuses in this order, lfm_vae_decode and lfm_vae_encode included: a workspace that is both misaligned and
 * short is LFM_ERR_ALIGN (those two answered LFM_ERR_WORKSPACE for it before they shared the set-up of the others).
 *
 * lfm_vae_conv_in_f16: diffusers AutoencoderKL.post_quant_conv (1x1, 4 -> 4) followed by Decoder.conv_in (3x3, pad 1, 4 -> 512) in one kernel:
 *   z fp32 NCHW [n,4,R,R] -> out fp16 NHWC [n,R,R,512]; pq_w fp32 [4][4], pq_b [4], cin_w fp32 [512][4][3][3], cin_b [512].  conv_in pads
 *   post_quant_conv(z) with zeros, so the 1x1 (its bias included) is skipped outside the image.  Any R >= 1 (R % 8 is lfm_vae_decode's rule). */
int lfm_vae_conv_in_f16(const float* pq_w, const float* pq_b, const float* cin_w, const float* cin_b, const float* z, void* out, int n, int R,
                        lfm_stream_t stream);
/* lfm_vae_downsample_f16: diffusers Downsample2D(use_conv=True, padding=0) of the encoder: F.pad(x, (0, 1, 0, 1)) then a 3x3 convolution at stride 2, i.e.
 *   out[oy][ox] reads x[2 oy + ky][2 ox + kx], zero beyond the bottom row and the right column.  x fp16 NHWC [n,2Ho,2Wo,C], w fp16 [C][9][C], bias fp32
 *   [C], out fp16 [n,Ho,Wo,C]; C % 64 == 0.  Runs on the GEMM kernel the calling thread's lfm_gemm_select asks for. */
size_t lfm_vae_downsample_workspace_bytes(int n, int Ho, int Wo, int C);
int lfm_vae_downsample_f16(const void* x, const void* w, const float* bias, void* out, void* workspace, size_t workspace_bytes, int n, int Ho, int Wo,
                           int C, lfm_stream_t stream);
/* lfm_vae_resnets_f16: n_res (1 .. 3) diffusers ResnetBlock2D (temb None: GroupNorm+SiLU -> conv1 -> GroupNorm+SiLU -> conv2 + (conv_shortcut of) x) in
 *   sequence on the drivers' four rotating buffers: x fp16 NHWC [n,H,W,r[0].cin] -> out [n,H,W,r[n_res-1].cout]; widths in {128, 256, 512}, r[i].cout ==
 *   r[i+1].cin, sc_w required where cin != cout.  chain_stats 1 (decoder): conv2 leaves the GroupNorm statistics of its output for the next resnet where its
 *   kernel can; 0 (encoder): every GroupNorm runs its own pass.  *last_slabs (may be NULL) = the statistics slabs per image the last conv2 left (0: none).
 *   lfm_vae_resnets_workspace_bytes(n, H, W) = 256 + a(n 256) + a(n max(2 ceil(H W / 256) 128, 8192) 8) + 4 a(n H W 512 2); 0 if an argument is <= 0
 *   or n H W 512 >= 2^31. */
size_t lfm_vae_resnets_workspace_bytes(int n, int H, int W);
int lfm_vae_resnets_f16(const lfm_vae_resnet* r, int n_res, const void* x, void* out, void* workspace, size_t workspace_bytes, int n, int H, int W,
                        int chain_stats, int* last_slabs, lfm_stream_t stream);
/* lfm_vae_conv_moments_f32: diffusers Encoder.conv_out (3x3, pad 1, 512 -> 8) with AutoencoderKL.quant_conv (1x1, 8 -> 8) folded into its weights by the
 *   caller: in fp16 NHWC [n,H,W,512], w8 fp16 [8][9][512], b8 fp32 [8] -> moments fp32 NCHW [n,8,H,W] (no fp16 rounding of the result). */
size_t lfm_vae_conv_moments_workspace_bytes(int n, int H, int W);
int lfm_vae_conv_moments_f32(const void* in, const void* w8, const float* b8, float* moments, void* workspace, size_t workspace_bytes, int n, int H,
                             int W, lfm_stream_t stream);

/* u8 NHWC = trunc(clamp((x+1)/2, 0, 1) * 255) of fp32 NCHW images (test_flow_latent_ddp.py:131-135). */
int lfm_images_to_uint8(const float* x, uint8_t* out, int N, int H, int W, lfm_stream_t stream);
/* Same with rounding != 0: trunc(clamp((x+1)/2, 0, 1) * 255 + 0.5), the conversion of torchvision.utils.save_image that the
 * single-process script applies (test_flow_latent.py:264-269,297). */
int lfm_images_to_uint8_mode(const float* x, uint8_t* out, int N, int H, int W, int rounding, lfm_stream_t stream);

/* ------------------------------------------------------------------ NHWC-fp16 building blocks (origin-ADM UNet)
 * The guided-diffusion UNet (models/guided_diffusion/unet.py:376-655) has a data-dependent layer list, so its forward is
 * sequenced by the host (lfm_amd/models/unet.py) over these ops.  Activations: fp16 NHWC [N*H*W, C].
 *
 * lfm_conv3x3_f16: out[N,H,W,Cout] = conv3x3(in, pad 1) + bias (+ resid); w fp16 [Cout][ky*3+kx][Cin], Cin % 64 == 0.
 *   mode 0: in is [N,H,W,Cin] (ResBlock convs, unet.py:171-175,193-198);  mode 1: in is [N,H/2,W/2,Cin], nearest-2x upsampled on
 *   the fly (Upsample, :73-100);  mode 2: in is [N,2H,2W,Cin], stride 2 (Downsample, :103-128).
 *   Kernel choice (same result up to the fp32 summation order): modes 0 / 1 with H, W multiples of 16, Cout % 128 == 0 and at least 256
 *   (16x16-pixel tile, 128-channel block) pairs run on the halo-tiled direct kernel (csrc/conv_halo_kernel.h); everything else is an
 *   implicit GEMM (split-K with a workspace for the small maps). */
int lfm_conv3x3_f16(const void* in, const void* w, const float* bias, const void* resid, void* out, int N, int H, int W, int Cin, int Cout,
                    int mode, lfm_stream_t stream);
/* The same with a caller-owned workspace of lfm_conv3x3_workspace_bytes(...) bytes (0 = none needed): small-M / huge-K convolutions (the
 * low-resolution levels of the UNets) then run split-K with a deterministic slab reduction.  workspace may be NULL. */
size_t lfm_conv3x3_workspace_bytes(int N, int H, int W, int Cin, int Cout);
int lfm_conv3x3_f16_ws(const void* in, const void* w, const float* bias, const void* resid, void* out, int N, int H, int W, int Cin, int Cout,
                       int mode, void* workspace, size_t workspace_bytes, lfm_stream_t stream);
/* The same with out = (conv3x3 + bias (+ resid)) * scale, the scale applied in fp32 to the finished sum before the fp16 store, on every path (halo
 * kernel, implicit GEMM, split-K finish): the residual epilogue of EDM's UNetBlock with skip_scale = sqrt(0.5) (SongUNet / ddpm++, models/EDM.py:272-274).
 * scale = 1 is bit-identical to lfm_conv3x3_f16_ws. */
int lfm_conv3x3_scaled_f16_ws(const void* in, const void* w, const float* bias, const void* resid, float scale, void* out, int N, int H, int W, int Cin,
                              int Cout, int mode, void* workspace, size_t workspace_bytes, lfm_stream_t stream);
/* Which path lfm_conv3x3_f16_ws (and its scaled form) takes for this shape with 16-byte aligned operands and a workspace of workspace_bytes, under the
 * calling thread's flags: 1 = the halo-tiled direct kernel, 2 = split-K slices + the finish kernel, 3 = one implicit GEMM; LFM_ERR_SHAPE for a shape that
 * is refused.  No launch; usable without a GPU. */
int lfm_conv3x3_plan(int N, int H, int W, int Cin, int Cout, int mode, size_t workspace_bytes);
/* first conv (unet.py:475): fp32 NCHW [N,Cin<=16,H,W] -> fp16 NHWC [N,H,W,Cout]; w fp32 [Cout,Cin,3,3].  Cout % 8 == 0.  out_nhwc and bias 16-byte
 * aligned, else LFM_ERR_ALIGN before any launch: the scalar kernel stores eight channels and loads four bias values at a time.  The one exception:
 * Cout of 64, 128, 192 or 256 on the MFMA kernel (the default there while its operand planes fit the LDS) needs out_nhwc 8-byte aligned only. */
int lfm_conv3x3_in_f32(const float* x_nchw, const float* w, const float* bias, void* out_nhwc, int N, int H, int W, int Cin, int Cout,
                       lfm_stream_t stream);
/* last conv (unet.py:594): fp16 NHWC -> fp32 NCHW [N,nch<=4,H,W]; w4 fp16 [4][9][Cin] (rows >= nch zero), bias4 fp32 [4] */
int lfm_conv3x3_out_f32(const void* in, const void* w4, const float* bias4, float* out_nchw, int N, int H, int W, int Cin, int nch,
                        lfm_stream_t stream);
/* C fp16 [M,N] = A[M,K] W[N,K]^T + bias (+ resid fp16 [M,N]): 1x1 convs / Conv1d(k=1) / skip connections (unet.py:204,266,276) */
int lfm_linear_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                   const void* resid, lfm_stream_t stream);
/* The same with A = the channel concat [A1 (K1 columns) | A2 (K2 columns)] of two dense fp16 tensors read in place: the 1x1 skip convolution of an
 * output-block ResBlock, whose input is th.cat([h, hs.pop()], dim=1) (unet.py:649 + :236).  K1 % 64 == 0, K2 % 8 == 0. */
int lfm_linear2_f16(const void* A1, int K1, const void* A2, int K2, const void* W, long ldw, void* C, long ldc, int M, int N, const float* bias,
                    const void* resid, lfm_stream_t stream);
/* lfm_linear_f16 / lfm_linear2_f16 with C = (A W^T + bias (+ resid)) * scale (fp32, before the fp16 store): the attention projection and the 1x1 skip of
 * EDM's UNetBlock with skip_scale != 1 (models/EDM.py:290-291).  scale = 1 is bit-identical to the unscaled entry points. */
int lfm_linear_scaled_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                          const void* resid, float scale, lfm_stream_t stream);
int lfm_linear2_scaled_f16(const void* A1, int K1, const void* A2, int K2, const void* W, long ldw, void* C, long ldc, int M, int N,
                           const float* bias, const void* resid, float scale, lfm_stream_t stream);
/* The linears of EDM's TransformerBlock (models/EDM.py:427-483; DhariwalUNet(use_context=True), model_type "adm_context").  Additions to ABI 4.
 *
 * lfm_linear_resid_vec_f16: C fp16 [M,N] = (A W^T + bias (+ resid) (+ vec[m / tokens][n])) * scale -- lfm_linear_scaled_f16 with one more fp32 row per image
 *   in the sum: vec fp32, rows vec_stride floats apart, `tokens` rows of C per row of vec.  attn1.proj of a TransformerBlock: the cross-attention over a
 *   ONE-key context is the same vector at every pixel, so both of the block's first two residual sums happen here.  vec = NULL or all zero is bit-identical
 *   to lfm_linear_scaled_f16.  Alignment and shape as lfm_linear_scaled_f16; also vec 16-byte aligned with vec_stride % 4 == 0 (LFM_ERR_ALIGN), tokens > 0
 *   and M % tokens == 0 (LFM_ERR_SHAPE), all before any launch.
 * lfm_linear_silu_f16: C fp16 [M,N] = silu(A W^T + bias) (ff.layer0): x / (1 + exp(-x)) in fp32 on the accumulator, one rounding to fp16.  bias required.
 * lfm_gather_rows_f32: out[r][0..cols) = table[y[r]][0..cols), r < N; table fp32 [rows, cols] dense, y int64 on the device, out rows out_stride floats
 *   apart.  cols % 4 == 0, out_stride >= cols (LFM_ERR_SHAPE); table / out 16-byte aligned, out_stride % 4 == 0 (LFM_ERR_ALIGN).  No readback: graph-
 *   capturable, and a replay follows labels rewritten in place.  Labels are validated by the caller; the kernel clamps to [0, rows) rather than read beyond
 *   the table. */
int lfm_linear_resid_vec_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias,
                             const void* resid, const float* vec, long vec_stride, int tokens, float scale, lfm_stream_t stream);
int lfm_linear_silu_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias, lfm_stream_t stream);
int lfm_gather_rows_f32(const float* table, int rows, int cols, const void* y_int64, int N, float* out, long out_stride, lfm_stream_t stream);
/* y = silu?( GroupNorm(groups <= 32)(x; gamma, beta, eps) * (1 + scale[n]) + shift[n] );  film = fp32 [N][scale(C) | shift(C)] rows film_stride apart,
 * or NULL (nn.py:17-19,93-100; scale-shift-norm unet.py:228-233).  scratch: lfm_groupnorm_scratch_bytes(N, C) bytes. */
size_t lfm_groupnorm_scratch_bytes(int N, int C);
int lfm_groupnorm_f16(const void* x, void* y, const float* gamma, const float* beta, const float* film, long film_stride, void* scratch, int N,
                      int HW, int C, int groups, float eps, int silu, lfm_stream_t stream);
/* Which kernels lfm_groupnorm_f16 runs for this shape under the calling thread's flags (csrc/groupnorm_dispatch.h: gn_choose): stats | apply << 4 with
 * stats 1 = the fused small-map kernel, 2 = row-wise slabs, 3 / 4 = per-group slabs read 4 / 1 channels at a time; apply 1 = inside the fused kernel,
 * 2 = a thread per channel octet, 3 = a thread per 16-byte chunk; LFM_ERR_SHAPE for a shape that is refused.  For lfm_groupnorm2_f16: the plan at
 * C = Ca + Cb.  No launch; usable without a GPU.  Addition to ABI 4. */
int lfm_groupnorm_plan(int N, int HW, int C, int groups);
/* The same on the channel concat [xa (Ca channels) | xb (Cb channels)] read in place (groups may straddle the seam); y is dense [N*HW, Ca + Cb];
 * scratch: lfm_groupnorm_scratch_bytes(N, Ca + Cb).  Ca % 8 == Cb % 8 == 0.  Bit-identical to lfm_concat_channels_f16 + lfm_groupnorm_f16. */
int lfm_groupnorm2_f16(const void* xa, int Ca, const void* xb, int Cb, void* y, const float* gamma, const float* beta, const float* film,
                       long film_stride, void* scratch, int N, int HW, int groups, float eps, int silu, lfm_stream_t stream);
/* y[N,Ho,Wo,C] = 2x2 mean of x[N,2Ho,2Wo,C]: EDM Conv2d(down=True) with the [1,1] resample filter (models/EDM.py:96-98,122-125) */
int lfm_avgpool2_f16(const void* x, void* y, int N, int Ho, int Wo, int C, lfm_stream_t stream);
/* y[N,Ho,Wo,C] = nearest-2x upsample of x[N,Ho/2,Wo/2,C]: EDM Conv2d(up=True, kernel=0) skip path (models/EDM.py:117-121) */
int lfm_upsample2_f16(const void* x, void* y, int N, int Ho, int Wo, int C, lfm_stream_t stream);
/* The [1,3,3,1] resampling filter of NCSN++ (EDM Conv2d with resample_filter = [1,3,3,1], models/EDM.py:96-98; f2 = outer(f, f) / 64), csrc/fir_resample.h.
 * NHWC fp16, C % 8 == 0 (LFM_ERR_SHAPE), x / y / resid 16-byte aligned (LFM_ERR_ALIGN), both before any launch; fp32 arithmetic, one rounding to fp16.
 *
 * lfm_fir_down2_f16: y[N,Ho,Wo,C] = ((sum_{a,b<4} f2[a][b] x[2 oy - pad + a][2 ox - pad + b]) (+ bias[c]) (+ resid)) * scale, zeros outside x.
 *   pad 1: x is [N,2Ho,2Wo,C] -- Conv2d(down=True) not fused, conv0 and skip of a `down` UNetBlock (:124-127);
 *   pad 0: x is [N,2Ho+2,2Wo+2,C], the output of a 3x3 convolution at padding 2 -- the second half of Conv2d(down=True, fused_resample=True), the
 *          aux_residual of the residual encoder (:116-118), whose bias is added AFTER the filter (:130-131).
 *   bias fp32 [C] or NULL, resid fp16 on the output grid or NULL, scale applied in fp32: (x + aux_residual(aux)) / sqrt(2) of SongUNet.forward (:686) in the
 *   same pass.  bias = resid = NULL and scale = 1: the bare filter. */
int lfm_fir_down2_f16(const void* x, void* y, const float* bias, const void* resid, float scale, int N, int Ho, int Wo, int C, int pad,
                      lfm_stream_t stream);
/* y[N,Ho,Wo,C] = conv_transpose2d(x[N,Ho/2,Wo/2,C], 4 f2, stride 2, padding 1): Conv2d(up=True) not fused, conv0 and skip of an `up` UNetBlock (:120-123).
 * Per axis y[2i] = (3 x[i] + x[i-1]) / 4, y[2i+1] = (3 x[i] + x[i+1]) / 4, zeros outside.  Ho, Wo even. */
int lfm_fir_up2_f16(const void* x, void* y, int N, int Ho, int Wo, int C, lfm_stream_t stream);
/* y[N,H+2,W+2,C] = x[N,H,W,C] inside a one-pixel border of zeros.  A pad-1 3x3 convolution (lfm_conv3x3_f16, mode 0, any path) of y on the (H+2) x (W+2)
 * grid IS the padding-2 convolution of x that the fused down path starts with (models/EDM.py:117).  C % 8 == 0, 16-byte aligned. */
int lfm_zero_border_f16(const void* x, void* y, int N, int H, int W, int C, lfm_stream_t stream);
/* The same for fp32 planes, y[planes,H+2,W+2] = x[planes,H,W]: the NCHW network input (planes = N * Cin) that the first aux_residual convolves through
 * lfm_conv3x3_in_f32.  Made by a kernel, not by a slice copy into a zeroed buffer: captured graphs of the UNets hold kernel nodes only. */
int lfm_zero_border_f32(const float* x, float* y, int planes, int H, int W, lfm_stream_t stream);
/* out[p][0:Ca | Ca:Ca+Cb] = a[p], b[p]   (th.cat([h, hs.pop()], dim=1), unet.py:649) */
int lfm_concat_channels_f16(const void* a, const void* b, void* out, long pixels, int Ca, int Cb, lfm_stream_t stream);
/* y = x + e[n][c] broadcast over the pixels of image n (ResBlock without scale-shift norm: h + emb_out[..., None, None], unet.py:233-235);
 * x, y fp16 NHWC [N*HW, C], e fp32 rows e_stride apart */
int lfm_add_image_vec_f16(const void* x, const float* e, long e_stride, void* y, int N, int HW, int C, lfm_stream_t stream);
/* QKVAttentionLegacy (unet.py:310-334) and the attention of EDM's UNetBlock: qkv fp16 [N*T, 3C], columns [head][q|k|v][ch]; out fp16 [N*T, C], columns
 * [head][ch]; softmax(q k^T / sqrt(ch)) v with fp32 scores and softmax.  Three kernels (csrc/unet_attention_dispatch.h; lfm_unet_attention_plan tells which):
 *   2 = the resident MFMA kernel (csrc/unet_attention_kernel.h, as the VALU kernel): T = 64 / 256 with ch = 64 / 128, all of K and V^T of a head in the LDS;
 *   1 = the VALU kernel: any ch, K, V and a 64-query score block in the LDS -- min(T, 64) (T + 1) 4 + 4 T (ch + 2) bytes <= 160 KiB
 *       (T <= 314 at ch = 64, T <= 127 at ch = 256);
 *   3 = the streamed MFMA kernel (csrc/unet_attention_stream_kernel.h, LFM_OPT_UNET_ATTENTION_STREAM): every other shape with ch % 16 == 0 and ch <= 256, ANY T -- keys in blocks of 64
 *       through a double-buffered LDS stage, online softmax.
 * The MFMA kernels need 16-byte aligned pointers; otherwise the VALU kernel runs where it fits.  LFM_ERR_SHAPE when no kernel serves the shape
 * (ch % 16 != 0 or ch > 256 beyond the VALU kernel's LDS bound).  No workspace, no synchronisation, graph-capturable. */
int lfm_attention_small_f16(const void* qkv, void* out, int N, int T, int heads, int ch, lfm_stream_t stream);
/* Which kernel lfm_attention_small_f16 runs for this shape with 16-byte aligned operands under the calling thread's flags (LFM_DBG_UNET_ATT_VALU decides
 * first: 1 or LFM_ERR_SHAPE) and the library options: 1 / 2 / 3 as above, or LFM_ERR_SHAPE.  No launch; usable without a GPU. */
int lfm_unet_attention_plan(int N, int T, int heads, int ch);
/* Cross-attention of the SpatialTransformer (guided_diffusion/attention.py:177-215, CrossAttention with a context; csrc/unet_cross_attention_kernel.h):
 *   out[n*Tq + i][head*ch + c] = softmax_j(q_i . k_j / sqrt(ch)) v_j over the Tk keys of image n.
 * Q fp16 rows [N*Tq] ldq elements apart; K and V fp16 rows [N*Tk] ldkv apart -- they may be two column slices of one projection buffer, hence one ld; out
 * fp16 rows [N*Tq] ldo apart; columns [head][ch] everywhere.  fp32 scores and softmax, P and V in fp16, 1 / sum applied to the fp32 accumulators: the
 * arithmetic and the 64-key block order of the streamed kernel of lfm_attention_small_f16 (bit-identical to it where Tq == Tk).  Any Tq >= 1 and Tk >= 1;
 * ch % 16 == 0, ch <= 256, every ld >= heads*ch (LFM_ERR_SHAPE); the four pointers 16-byte aligned and every ld % 8 == 0 (LFM_ERR_ALIGN); both checked before
 * any launch.  No mask argument.  No workspace, no allocation, no synchronisation: graph-capturable. */
int lfm_cross_attention_f16(const void* Q, long ldq, const void* K, const void* V, long ldkv, void* out, long ldo, int N, int Tq, int Tk, int heads,
                            int ch, lfm_stream_t stream);
/* 1 when lfm_cross_attention_f16 serves this shape (with aligned operands), LFM_ERR_SHAPE otherwise.  No launch; usable without a GPU. */
int lfm_cross_attention_plan(int N, int Tq, int Tk, int heads, int ch);
/* nn.LayerNorm(C) on fp16 rows: y[m] = (x[m] - mean) / sqrt(var + eps) * gamma + beta, x and y dense fp16 [M, C], gamma / beta fp32 [C].  fp32 statistics
 * in two passes (mean, then the centred sum of squares; biased variance), one rounding to fp16; one wave per row (csrc/token_ops.h).  C % 8 == 0
 * (LFM_ERR_SHAPE); x, y, gamma, beta 16-byte aligned (LFM_ERR_ALIGN).  No workspace, graph-capturable. */
int lfm_layernorm_f16(const void* x, void* y, const float* gamma, const float* beta, long M, int C, float eps, lfm_stream_t stream);
/* GEGLU (attention.py:85-92): y[m][i] = h[m][i] * gelu(h[m][I + i]) with the exact (erf) GELU of F.gelu's default -- not the tanh form.  h fp16 rows [M]
 * ldh elements apart, 2I columns used; y dense fp16 [M, I].  fp32 arithmetic, one rounding.  I % 8 == 0, ldh >= 2I (LFM_ERR_SHAPE); ldh % 8 == 0 and h, y
 * 16-byte aligned (LFM_ERR_ALIGN).  No workspace, graph-capturable. */
int lfm_geglu_f16(const void* h, long ldh, void* y, long M, int I, lfm_stream_t stream);
/* The two ops of the layout encoder (models/encoder.py:52-87 BERTEmbedder over models/x_transformer.py TransformerWrapper + Encoder) that the library did not
 * have.  Additions to ABI 4.  Everything else of that encoder runs on entry points above: lfm_layernorm_f16, lfm_linear_f16 (the row-stacked to_q | to_k |
 * to_v projection without bias into one [M, 3 * 512] buffer; to_out and net.2 with the residual) and lfm_cross_attention_f16 over the three column slices
 * of that buffer (ldq = ldkv = 1536, Tq = Tk = L, 8 heads of 64) -- BERTEmbedder.forward passes no mask, so there is no mask argument.
 *
 * lfm_token_embed_f16: out[n*L + p][0..D) = fp16(tok_emb[ids[n*L + p]][:] + pos_emb[p][:]) (x_transformer.py:586-587).  tok_emb fp32 [vocab, D] and pos_emb
 *   fp32 [pos_rows, D] dense; ids int64 [N*L] on the device; out dense fp16 [N*L, D].  The add is in fp32, one rounding to fp16.  D % 8 == 0 and L <= pos_rows
 *   (LFM_ERR_SHAPE); the four pointers 16-byte aligned (LFM_ERR_ALIGN); both before any launch.  An id outside [0, vocab) (an IndexError in the reference)
 *   poisons its row with NaN, as lfm_time_embed does for labels; the kernel never reads beyond a table.  No readback, no workspace: graph-capturable, and a
 *   replay follows ids rewritten in place.
 * lfm_linear_gelu_f16: C fp16 [M,N] = gelu(A W^T + bias) with the EXACT (erf) GELU of nn.GELU() -- x Phi(x) evaluated as 0.5 x erfc(-x / sqrt 2) in fp32 on the
 *   accumulator, one rounding to fp16; not the tanh form of lfm_gemm_f16's GELU epilogue (timm's Mlp).  bias required (LFM_ERR_ARG).  Alignment, shapes and
 *   kernel choice as lfm_linear_silu_f16. */
int lfm_token_embed_f16(const float* tok_emb, int vocab, const float* pos_emb, int pos_rows, const void* ids_int64, void* out, int N, int L, int D,
                        lfm_stream_t stream);
int lfm_linear_gelu_f16(const void* A, long lda, const void* W, long ldw, void* C, long ldc, int M, int N, int K, const float* bias, lfm_stream_t stream);
/* The conditioning stage of mask-to-image synthesis (downstream_tasks/test_flow_latent_semantic_syn.py:131-135: F.one_hot -> SpatialRescaler, models/encoder.py:
 * 90-112: n_stages x F.interpolate(scale_factor=0.5, mode="bilinear") -> the 1x1 channel_mapper) as one gather (csrc/label_rescale.h).  Addition to ABI 4.
 *   out[n][o][i][j] = (sum over the 2^n x 2^n cell (i, j) of w[o][labels[n][y][x]]) / 4^n_stages (+ bias[o])
 * which is that chain exactly: a bilinear x0.5 stage at align_corners=False is a 2x2 mean, and the means of a 0/1 map are exact in fp32.
 * labels int64 [N,H,W] dense; w fp32 [Cout,num_cls] dense (channel_mapper.weight as stored); bias fp32 [Cout] or NULL; out fp32 NCHW
 * [N,Cout,H >> n_stages,W >> n_stages] dense.  Any H, W >= 2^n_stages, odd and non-square included: rows and columns beyond the last whole cell are not read.
 * Refused before any launch, in this order: labels, w or out NULL (LFM_ERR_ARG); N < 1, n_stages outside 1..4, Cout outside 1..8, num_cls < 1,
 * num_cls * Cout * 4 > 65536 (the table lives in the LDS), H or W < 2^n_stages (LFM_ERR_SHAPE); labels not 8-byte, w / bias / out not 4-byte aligned
 * (LFM_ERR_ALIGN).  Labels 16-byte aligned with W even are read two per load; the result does not depend on that, nor on N or an image's place in the batch:
 * per cell the pixel columns are summed top to bottom, then combined by a binary tree, adjacent columns first.  A label outside [0, num_cls) (an error of
 * F.one_hot in the reference) makes the Cout outputs of ITS cell NaN and is not used as an index.  No readback, no workspace, no atomics: graph-capturable,
 * and a replay follows labels rewritten in place. */
int lfm_label_rescale_f32(const void* labels_int64, const float* w, const float* bias, float* out, int N, int H, int W, int num_cls, int Cout, int n_stages,
                          lfm_stream_t stream);
/* Baseline JPEG encoding of the samples on the device (csrc/jpeg_encode.h; DESIGN.md "JPEG encode").  Additions to ABI 4.
 *   img_nhwc uint8 [N,H,W,3] dense RGB, 1 <= H, W <= 4096, 1 <= N <= 65535; quality 1..100 (libjpeg's scaling of the Annex-K tables, 8-bit entries)
 *   out      uint8 [N][cap]: for image i the entropy-coded data and the EOI marker, i.e. everything that follows the header in the file
 *            PIL.Image.save(path, quality=quality) writes for it (4:2:0, baseline, Annex-K Huffman tables, no restart markers) -- byte for byte; the header is
 *            the host's (lfm_amd/io_formats.py: jpeg_header), the same 623 bytes for every image of a size and quality
 *   lengths  int32 [N]: the TRUE number of those bytes, also when it exceeds cap.  Then out[i] holds the first cap of them, and nothing is written at or
 *            beyond out[i] + cap, nor outside [workspace, workspace + lfm_jpeg_encode_workspace_bytes(N, H, W, cap)).
 * Refused before any launch, in this order: img_nhwc, workspace, out or lengths NULL, quality outside 1..100 (LFM_ERR_ARG); N, H, W outside the ranges above,
 * cap < 1 (LFM_ERR_SHAPE; lfm_jpeg_encode_workspace_bytes returns 0 for them); workspace not 16-byte or lengths not 4-byte aligned (LFM_ERR_ALIGN);
 * workspace_bytes too small (LFM_ERR_WORKSPACE).  img_nhwc needs no alignment (16-byte aligned with W % 16 == 0 it is read 16 bytes per lane).
 * Six kernels on `stream`, no host synchronisation, no readback, no one-time set-up, integer arithmetic only and no atomics on global memory: deterministic,
 * independent of N and of an image's place in the batch, graph-capturable, and a replay follows pixels rewritten in place. */
size_t lfm_jpeg_encode_workspace_bytes(int N, int H, int W, int cap);
int lfm_jpeg_encode_rgb8(const uint8_t* img_nhwc, int N, int H, int W, int quality, int cap, void* workspace, size_t workspace_bytes, uint8_t* out,
                         int32_t* lengths, lfm_stream_t stream);
/* The elementwise stages of an inpainting batch (downstream_tasks/test_flow_latent_inpainting.py: CustomizedInpaintingEvalDataset.__getitem__ :36-55, the loop
 * :147-150 and :157-160, torchvision.utils.save_image's quantisation) from the bytes the files hold (csrc/inpaint.h).  Additions to ABI 4.
 * Images are uint8 NHWC [N,H,W,3] dense, masks uint8 [N,H,W] dense, the PNG's bytes as stored: 255 = keep, 0 = hole, anything between blends.  H % 8 == 0 and
 * W % 8 == 0.  Every fp32 operation below is rounded on its own (no FMA contraction; byte / 255 is the correctly rounded quotient), in the order written, which is the reference's: prepare
 * and composite give the bits torch gives on the CPU.  The LFM_FAST_MATH=1 A/B build is not covered by that statement.
 *
 * lfm_inpaint_prepare_u8: per pixel  i = (float)b / 255.0f  per channel,  m = 1.0f - (float)p / 255.0f  (1 = hole),  masked = (1.0f - m) * i;
 *   masked_nchw [N,3,H,W] = masked * 2.0f - 1.0f  (the VAE encoder's input);  image_nchw [N,3,H,W] = i * 2.0f - 1.0f  where that pointer is not NULL;
 *   mask_latent[n * mask_latent_image_stride + (y / 8) * (W / 8) + x / 8] = m * 2.0f - 1.0f  for y % 8 == 0 and x % 8 == 0: F.interpolate(mask, size=(H/8, W/8))
 *   (nearest) is that pick.  The caller passes channel 4 of the [N,5,H/8,W/8] conditioning tensor with stride 5 * (H/8) * (W/8); nothing else of it is written.
 * lfm_inpaint_cond_f32: out[n * out_image_stride + c * hw + k] = (mean + expf(0.5f * clamp(logvar, -30, 20)) * eps) * scale  for c < 4, k < hw, with moments
 *   fp32 [N,8,hw] (mean | logvar, lfm_vae_encode's output) and eps fp32 [N,4,hw]: DiagonalGaussianDistribution.sample() scaled.  eps == NULL gives mean * scale
 *   (.mode(): one multiplication, exact) and the logvar half is not read.  Elements beyond the first 4 * hw of an image's stride (the mask channel) are not
 *   touched.  expf is the accurate library routine (OCML, documented at 1 ulp; no approximate v_exp_f32), the clamp keeps a NaN as torch.clamp does; four
 *   roundings and that ulp per element (tests/inpaint_cases.py derives the bound from them).
 * lfm_inpaint_composite_u8: per pixel and channel, from the bytes and the decoded sample fake_nchw fp32 [N,3,H,W]:
 *   f01 = (f + 1.0f) / 2.0f;  mm = ((m * 2.0f - 1.0f) + 1.0f) / 2.0f;  i01 = ((i * 2.0f - 1.0f) + 1.0f) / 2.0f;  o = f01 * mm + (1.0f - mm) * i01;
 *   out_nhwc uint8 [N,H,W,3] = (uint8_t)clamp(o * 255.0f + 0.5f, 0, 255).  The round trip through [-1,1] is part of the definition (i01 != i for 63 of the 256
 *   bytes).  A pixel with mask byte 255 comes out as its image byte, one with mask byte 0 as the quantised sample.  A NaN in o gives byte 0, +inf 255, -inf 0;
 *   a non-finite f reaches o also where the mask keeps the image (inf * 0), so such a pixel is 0 whatever the image holds.  Not compared with torch, whose
 *   float-to-uint8 conversion of a NaN is not defined.
 *
 * Alignment.  Served at any base alignment the element types allow: byte pointers anywhere, float pointers 4-byte aligned (LFM_ERR_ALIGN otherwise).  prepare
 * and composite run 16 pixels per lane with 16-byte accesses when W % 16 == 0 and every pointer is 16-byte aligned, 8 pixels per lane with 8-byte loads of the
 * bytes and 16-byte accesses of the floats when the byte pointers are 8-byte and the float pointers 16-byte aligned, one element per access otherwise; cond
 * runs four elements per access when hw % 4 == 0, out_image_stride % 4 == 0 and its pointers are 16-byte aligned.  Every variant gives the same bits.
 * mask_latent is written 4 bytes at a time.
 * Refused before any launch, in this order: a required pointer NULL (LFM_ERR_ARG; image_nchw and eps may be NULL); N, H, W or hw < 1, H % 8, W % 8, a stride
 * smaller than what is written per image (LFM_ERR_SHAPE); a misaligned float pointer (LFM_ERR_ALIGN).  One launch each on `stream`, no readback, no
 * workspace, no allocation, no atomics: graph-capturable, and a replay follows inputs rewritten in place. */
int lfm_inpaint_prepare_u8(const uint8_t* img_nhwc, const uint8_t* mask, float* masked_nchw, float* image_nchw, float* mask_latent,
                           long mask_latent_image_stride, int N, int H, int W, lfm_stream_t stream);
int lfm_inpaint_cond_f32(const float* moments, const float* eps, float scale, float* out, long out_image_stride, int N, int hw, lfm_stream_t stream);
int lfm_inpaint_composite_u8(const float* fake_nchw, const uint8_t* img_nhwc, const uint8_t* mask, uint8_t* out_nhwc, int N, int H, int W,
                             lfm_stream_t stream);
/* SSIM per image of two image batches, and the per-image sum of a mask's bytes: the score of the reference's inpainting evaluator
 * (datasets_prep/inpaint_preprocess/losses/ssim.py: SSIM._ssim :47-67 with size_average=False; losses/base_loss.py: SSIMScore; evaluator.py: the mask area
 * per image) in one tile kernel and one reduce kernel (csrc/ssim.h).  Additions to ABI 4.
 *   lfm_ssim_u8:  a, b uint8 NHWC [N,H,W,3] dense, each byte b taken as (float)b / 255.0f, the correctly rounded quotient (C = 3); mask uint8 [N,H,W] dense
 *                 or NULL.  With a mask, mask_sum[n] = the exact integer sum of image n's mask bytes; mask_sum is NULL if and only if mask is.
 *   lfm_ssim_f32: a, b fp32 NCHW [N,C,H,W] dense, 1 <= C <= 4, used as they are.
 * window: `window_size` floats in DEVICE memory, the 1-D Gaussian the caller builds as the reference's _gaussian does (sigma 1.5, normalised in fp32);
 * window_size odd, 3..11.  With x, y one channel of the two images, 0 outside the image (zero padding, window_size / 2 wide), and G(q)[r][c] =
 * sum_j w[j] * (sum_k w[k] * q[r + j - p][c + k - p]), p = window_size / 2 (horizontal pass, then vertical, FMAs in ascending tap order):
 *   mu1 = G(x), mu2 = G(y), s11 = G(x*x) - mu1*mu1, s22 = G(y*y) - mu2*mu2, s12 = G(x*y) - mu1*mu2
 *   map = ((2*mu1*mu2 + C1) * (2*s12 + C2)) / ((mu1*mu1 + mu2*mu2 + C1) * (s11 + s22 + C2)),  C1 = 1e-4f, C2 = 9e-4f
 *   out[n] = (float)(sum of map over c, r, c in fp64 of fp32 tile sums / (C*H*W))
 * Every product, sum and the division of the map are rounded on their own in fp32 (no FMA contraction), so identical images score exactly 1.0f.  The
 * reference's 2-D window is the fp32 outer product of w; the separable form differs from it by rounding only (tests/ssim_cases.py derives the bound
 * against the reference in fp64).  Sums are taken in a fixed order without float atomics: out[n] is bit-reproducible and does not depend on N or on the
 * image's place in the batch; a NaN in one image reaches that image's result only.  1 <= H, W <= 4096; N * ceil(H/32) * ceil(W/32) < 2^31.
 * workspace: lfm_ssim_workspace_bytes(N, H, W) bytes (8 per image and 32 x 32 tile, rounded up to 16; 0 for a refused shape), 16-byte aligned, no
 * initialisation needed.  Byte pointers need no alignment: with W % 4 == 0 and a, b, mask 4-byte aligned the bytes are read a word at a time, otherwise
 * byte by byte, with the same bits.
 * Refused before any launch, in this order: a required pointer NULL, or exactly one of mask and mask_sum NULL (LFM_ERR_ARG); N, H, W, C or window_size out of
 * range, or workspace_bytes too small (LFM_ERR_SHAPE); window, out, a float image pointer not 4-byte aligned, mask_sum not 8-byte aligned, or the workspace
 * not 16-byte aligned (LFM_ERR_ALIGN).  Two launches on `stream`, no host synchronisation, no readback, no allocation; writes only out, mask_sum and the
 * first lfm_ssim_workspace_bytes bytes of the workspace: graph-capturable, and a replay follows inputs rewritten in place. */
size_t lfm_ssim_workspace_bytes(int N, int H, int W);
int lfm_ssim_u8(const uint8_t* a_nhwc, const uint8_t* b_nhwc, const uint8_t* mask, int N, int H, int W, const float* window, int window_size,
                void* workspace, size_t workspace_bytes, float* out, long long* mask_sum, lfm_stream_t stream);
int lfm_ssim_f32(const float* a_nchw, const float* b_nchw, int N, int C, int H, int W, const float* window, int window_size, void* workspace,
                 size_t workspace_bytes, float* out, lfm_stream_t stream);
/* emb = time_embed(timestep_embedding(t, F)) (+ label_emb[y]) (nn.py:103-121, unet.py:633-641): fp32 [N,E] and fp16 silu(emb).
 * label_table has label_rows rows; a label outside [0, label_rows) (an IndexError in the reference) poisons its row with NaN. */
int lfm_time_embed(const float* t, int t_len, const float* w0, const float* b0, const float* w2, const float* b2, const float* label_table,
                   const int64_t* y, int label_rows, float* scratch_h1, float* emb, void* emb_silu_f16, int N, int F, int E,
                   lfm_stream_t stream);
/* DDPM++ mapping network of SongUNet (models/EDM.py:663-675, PositionalEmbedding :490-505 with endpoint = True), all fp32:
 *   in  = [sin(t f) | cos(t f)] (+ label_scale * label_table[y] + label_bias),  f_i = 10000^(-i / (F / 2 - 1)),  i < F / 2
 *   emb = silu(W1 silu(W0 in + b0) + b1):  fp32 [N,E] and its fp16 copy (already SiLU'd: the blocks' affine GEMM reads it as it is).
 * w0 [E,F], w1 [E,E] row-major; label_table = map_label.weight^T [label_rows][F], label_bias [F], label_scale = sqrt(label_dim); all three NULL / unused
 * for an unconditional evaluation.  t has t_len = 1 or N entries; scratch_h1: N x E floats.  F even, F >= 4.  A label outside [0, label_rows) poisons
 * its row with NaN. */
int lfm_song_embed(const float* t, int t_len, const float* w0, const float* b0, const float* w1, const float* b1, const float* label_table,
                   const float* label_bias, float label_scale, const int64_t* y, int label_rows, float* scratch_h1, float* emb, void* emb_f16, int N,
                   int F, int E, lfm_stream_t stream);
/* NCSN++ mapping network of SongUNet (embedding_type = "fourier": FourierEmbedding models/EDM.py:512-522 in place of the positional table; the rest of
 * :663-675 as lfm_song_embed):  in = [sin(t g) | cos(t g)] (+ label term),  g_i = fl32(fl32(2 pi) * freqs[i]),  t g_i rounded to fp32 once more -- the
 * reference's two fp32 roundings; freqs fp32 [F / 2] (the buffer map_noise.freqs, ~16 N(0,1): arguments of several hundred radians, full-range sine and
 * cosine).  F = noise_channels = 2 * model_channels for the preset.  Every other argument, the outputs and the NaN-poisoning as lfm_song_embed. */
int lfm_fourier_embed(const float* t, int t_len, const float* freqs, const float* w0, const float* b0, const float* w1, const float* b1,
                      const float* label_table, const float* label_bias, float label_scale, const int64_t* y, int label_rows, float* scratch_h1,
                      float* emb, void* emb_f16, int N, int F, int E, lfm_stream_t stream);

/* ------------------------------------------------------------------ solver helpers (device-resident time grid)
 * Advance the captured step:  s = *step;  t_cur[0] = ts[s];  t_next[0] = ts[s+1];  dt_cur[0] = dts[s];  *step = s+1.
 * ts has n+1 entries, dts n.  Lets ONE captured graph be replayed for every interval of the fixed grids of
 * test_flow_latent.py:42-76 (torchdiffeq euler) and sampler/karras_sample.py:85-161 (Euler / Heun). */
int lfm_grid_advance(const float* ts, const float* dts, int* step, float* t_cur, float* t_next, float* dt_cur, lfm_stream_t stream);

/* out = base + (scale ? *scale : 1) * sum_i coef[i] * k[i]   (i < nk <= 8), n fp32 elements (n % 4 == 0).
 * coef and scale are DEVICE memory (read at run time); k_host_ptrs is a HOST array of nk device pointers.
 * Covers the Heun update x + dt*(0.5 d + 0.5 d') (karras_sample.py:157-159) and the Runge-Kutta stage sums of
 * torchdiffeq's rk4 / dopri5.  out, base (when given) and every k[i] are read or written 16 bytes at a time: LFM_ERR_ALIGN, before any launch, for
 * one that is not 16-byte aligned or for n % 4 != 0. */
int lfm_lincomb(float* out, const float* base, const float* const* k_host_ptrs, const float* coef, const float* scale, int nk, long n,
                lfm_stream_t stream);

/* Error ratio of one adaptive Runge-Kutta step, as torchdiffeq's controller takes it (RMS over the WHOLE state tensor; reference call site
 * test_flow_latent.py:61-73, dopri5 at rtol = atol = 1e-5):  out[0] = sqrt(mean_i ((*dt) * sum_j e_coef[j] k_j[i] / (atol + rtol max(|y0[i]|, |y1[i]|)))^2).
 * e_coef, dt, out: DEVICE memory; k_host_ptrs: HOST array of nk <= 8 device pointers; scratch: >= 1024 floats of device memory; n % 4 == 0.
 * Deterministic (two fixed-order stages); the only value of the step the host has to read.  y0, y1 and every k_j are read 16 bytes at a time:
 * LFM_ERR_ALIGN, before any launch, for one that is not 16-byte aligned or for n % 4 != 0. */
int lfm_rk_error_norm(const float* y0, const float* y1, const float* const* k_host_ptrs, const float* e_coef, const float* dt, int nk, long n,
                      float rtol, float atol, float* scratch, float* out, lfm_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* LFM_HIP_H */
