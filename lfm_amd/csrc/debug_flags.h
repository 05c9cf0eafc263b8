// The ablation flags of lfm_gemm_select (bits 4+ of its argument, i.e. `flags << 4`; lfm_dit_call.gemm_select carries the same word) and the accessors of
// the library-wide switches (defined in dit.hip).  Every flag and every multi-bit field (NAME_SHIFT / NAME_MASK: value = (flags >> SHIFT) & MASK) is
// defined HERE, once, one per line; lfm_amd/hip.py exports the same names without the LFM_ prefix and tests/test_host_logic.py compares the two.
// A name starts with its consumer.  All 27 bits are taken and several serve two consumers: "shares" names every other flag on the same bits, so a run
// that sets one sets the other too.  tests/test_host_logic.py keeps the list of these overlaps; a new one fails there until it is added on purpose.
// Values are part of every recorded command line (profiles/, tools/archive/): do not renumber.
#pragma once

// ---- GEMM: the 256-row kernels, their dispatch and split-K (gemm256*_kernel.h, gemm_dispatch.h, gemm_kernel.h)
constexpr int LFM_DBG_GEMM_NO_EPILOGUE = 4;      // ablation: the main loop only, no epilogue
constexpr int LFM_DBG_GEMM_SETPRIO = 8;          // 256x128 kernel: raise the wave priority around the MFMA cluster
constexpr int LFM_DBG_GEMM_GM8 = 32;             // tile order: groups of 8 M-panels
constexpr int LFM_DBG_GEMM_GM2 = 64;             // tile order: groups of 2 M-panels
constexpr int LFM_DBG_GEMM_NO_XCD_REMAP = 128;   // tile order: no contiguous tile range per XCD
constexpr int LFM_DBG_GEMM_GM4 = 256;            // tile order: groups of 4 M-panels; shares ATT_WIDE
constexpr int LFM_DBG_GEMM_NO_SPLITK = 512;      // split-K off
constexpr int LFM_DBG_GEMM_STORE8 = 1024;        // the 8-byte-store epilogue instead of the 16-byte one (no tile statistics: the VAE convolution asks)
constexpr int LFM_DBG_GEMM_PARITY_PRIO = 2048;   // 256x128 kernel: static priority by block parity instead of the pipe's age order
constexpr int LFM_DBG_GEMM_NEVER_V4 = 4096;      // chip-filling shapes never take the 256x128 kernel
constexpr int LFM_DBG_GEMM_ALWAYS_V4 = 8192;     // chip-filling shapes always take the 256x128 kernel
constexpr int LFM_DBG_GEMM_SPLITK128 = 65536;    // deep small-map split-K on 128x128 slices instead of 256x256 ones; shares LN_BPERMUTE
constexpr int LFM_DBG_GEMM_ABL_SHIFT = 21;       // measurement build, lfm_gemm_f16 GELU epilogue: main-loop ablation of kernel 5 (1..7; 8 | 7 = variant 8) and of
constexpr int LFM_DBG_GEMM_ABL_MASK = 15;        //   kernel 6 (1..4, 8 = DMA placement); shares TRACE_COL, DIT_PATCH_ROUND1, VAE_SEPARATE_STATS, QKV_PER_ITEM, CONV_IMPLICIT_GEMM, CONV_HALO_SMALL
constexpr int LFM_DBG_GEMM_OPT_SHIFT = 25;       // measurement build, lfm_gemm_f16 GELU epilogue: OPT variant 1 of kernels 5 and 6 (2, 3: LFM_ERR_ARG on 5);
constexpr int LFM_DBG_GEMM_OPT_MASK = 3;         //   shares ATT_MODE, QKV_NO_KEY_LOOP, QKV_TWO_KTILES

// ---- TRACE: the s_memtime-stamped build of kernel 5 (measurement build, gemm256h_kernel.h)
constexpr int LFM_DBG_TRACE_GEMM = 2;            // lfm_gemm_f16 / lfm_gemm_qkv_f16 with kernel 5 forced run the stamped build; shares QKV_TRACE
constexpr int LFM_DBG_TRACE_NO_STORES = 131072;  // the stamped epilogue pass without its stores
constexpr int LFM_DBG_TRACE_COL_SHIFT = 21;      // the stamped tile: row 0, this tile column; shares GEMM_ABL, DIT_PATCH_ROUND1, VAE_SEPARATE_STATS, QKV_PER_ITEM,
constexpr int LFM_DBG_TRACE_COL_MASK = 15;       //   CONV_IMPLICIT_GEMM, CONV_HALO_SMALL

// ---- ATT: the DiT attention kernels (attention_kernel.h, attention_stream_kernel.h)
constexpr int LFM_DBG_ATT_WIDE = 256;            // 256 tokens: four waves x 64 queries instead of the narrow kernels; shares GEMM_GM4
constexpr int LFM_DBG_ATT_MODE_SHIFT = 25;       // measurement build: phase-split variants MODE 1 / 2 / 3 (head_dim 64, 256 tokens); shares GEMM_OPT,
constexpr int LFM_DBG_ATT_MODE_MASK = 3;         //   QKV_NO_KEY_LOOP, QKV_TWO_KTILES

// ---- QKV: the fused QKV projection + attention kernel (qkv_attention_kernel.h); it also takes the GEMM tile-order flags
constexpr int LFM_DBG_QKV_TRACE = 2;                // measurement build: s_memtime stamps of workgroup 0; shares TRACE_GEMM
constexpr int LFM_DBG_QKV_NO_VT_WRITES = 262144;    // measurement build, hand-over ablation: no V^T writes; shares LN_FOUR_ROWS
constexpr int LFM_DBG_QKV_NO_QK_WRITES = 524288;    // measurement build, hand-over ablation: no Q / K writes; shares LN_TWO_ROWS
constexpr int LFM_DBG_QKV_PER_ITEM = 4194304;       // one workgroup per item instead of one persistent workgroup per CU; shares VAE_SEPARATE_STATS, GEMM_ABL, TRACE_COL
constexpr int LFM_DBG_QKV_NO_KEY_LOOP = 33554432;   // measurement build, phase split: no key loop; shares ATT_MODE, GEMM_OPT
constexpr int LFM_DBG_QKV_TWO_KTILES = 67108864;    // measurement build, phase split: two K-tiles only; shares ATT_MODE, GEMM_OPT

// ---- LN: lfm_ln_modulate (dit.hip)
constexpr int LFM_DBG_LN_STORE8 = 32768;         // the 8-byte-store kernel instead of the one-row-per-wave kernels
constexpr int LFM_DBG_LN_BPERMUTE = 65536;       // one row per wave, ds_bpermute sums; shares GEMM_SPLITK128
constexpr int LFM_DBG_LN_FOUR_ROWS = 262144;     // four rows per wave; shares QKV_NO_VT_WRITES
constexpr int LFM_DBG_LN_TWO_ROWS = 524288;      // two rows per wave; shares QKV_NO_QK_WRITES

// ---- DIT: the layers around the blocks (dit.hip)
constexpr int LFM_DBG_DIT_FINAL_ROUND1 = 1048576;  // final layer: the round-1 kernel instead of the MFMA one
constexpr int LFM_DBG_DIT_PATCH_ROUND1 = 2097152;  // patch embedding: the round-1 kernel instead of the MFMA one; shares GEMM_ABL, TRACE_COL

// ---- CONV: the 3x3 convolutions of the UNets and the VAE decoder (ops.hip, vae.hip, conv_halo_kernel.h)
constexpr int LFM_DBG_CONV_IMPLICIT_GEMM = 8388608;  // the implicit GEMM instead of the halo-tiled kernel; shares GEMM_ABL, TRACE_COL
constexpr int LFM_DBG_CONV_HALO_SMALL = 16777216;    // the halo-tiled kernel for problems below 256 tiles too (parity tests); shares GEMM_ABL, TRACE_COL

// ---- VAE: the decoder (vae.hip)
constexpr int LFM_DBG_VAE_SEPARATE_STATS = 4194304;  // GroupNorm statistics in a pass of their own, not in the convolution's epilogue; shares QKV_PER_ITEM, GEMM_ABL, TRACE_COL

// ---- UNET: the UNets' own kernels (ops.hip, unet_attention_dispatch.h)
constexpr int LFM_DBG_UNET_CONV_IN_SCALAR = 1;   // input convolution: the scalar kernel instead of the MFMA one
constexpr int LFM_DBG_UNET_ATT_VALU = 16;        // attention: the VALU kernel instead of the MFMA one
constexpr int LFM_DBG_UNET_GN_ROWS = 16384;      // GroupNorm: the three-kernel path instead of the one-kernel path for small maps

// ---- the effective settings of the calling thread (per-call override, else the process-wide default; dit.hip)
int lfm_gemm_selected();        // 0 auto, 1 / 4 / 5 / 6 force the 128x128 / 256x128 / 256x256 / one-wave-per-SIMD 256x256 kernel (lfm_gemm_select)
int lfm_gemm_debug_flags();     // the flags above, measurement only
int lfm_gemm_selected_v1_ok();  // 1 unless a 256-row kernel is being forced or GEMM_NO_SPLITK is set: split-K runs on the 128x128 kernel
int lfm_gemm_prefers_v4(int M, int N, int K);  // shapes where the 256x128 two-workgroups-per-CU kernel measured faster than the 256x256 one
int lfm_gemm_v6_default();      // 1: chip-filling row-major GEMMs with K % 64 == 0 take kernel 6 instead of 5 (LFM_OPT_GEMM_V6)
int lfm_stagger_ticks();        // measurement builds (lfm_set_option key 3): s_memtime ticks by which workgroups 256..511 of a co-resident-pair kernel start late; else 0
int lfm_attention_stream_enabled();  // LFM_OPT_ATTENTION_STREAM
int lfm_attention_tiled_mode();     // LFM_OPT_ATTENTION_TILED: 0 never, 1 the DiT token counts no other attention kernel serves, 2 every shape it takes
int lfm_unet_attention_stream_mode();  // LFM_OPT_UNET_ATTENTION_STREAM: 0 never, 1 the shapes no other UNet attention kernel serves, 2 every shape it takes
