"""ctypes binding of liblfm_hip.so (C ABI: include/lfm_hip.h).  Fails loudly -- no fallback."""
import ctypes as C
import math
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "_lib", "liblfm_hip.so")
_lib = None


class LfmHipError(RuntimeError):
    pass


class DitShape(C.Structure):
    _fields_ = [(n, C.c_int) for n in ("depth", "hidden", "heads", "patch", "in_ch", "res", "mlp_hidden", "label_rows")]


_DIT_WEIGHT_FIELDS = ("pos_embed", "patch_w", "patch_b", "t_w0", "t_b0", "t_w2", "t_b2", "y_table", "ada_w", "ada_b",
                      "qkv_w", "qkv_b", "proj_w", "proj_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b", "final_w", "final_b", "patch_w16")


class DitWeights(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _DIT_WEIGHT_FIELDS]


class DitCall(C.Structure):
    _fields_ = [("batch", C.c_int), ("x", C.c_void_p), ("t", C.c_void_p), ("t_len", C.c_int), ("y", C.c_void_p),
                ("cfg", C.c_int), ("cfg_scale", C.c_float), ("out", C.c_void_p), ("axpy_base", C.c_void_p), ("axpy_dt", C.c_void_p),
                ("cond_table", C.c_void_p), ("cond_step", C.c_void_p), ("cond_offset", C.c_int),
                ("cond_rows", C.c_int), ("fold_ln", C.c_int), ("gemm_select", C.c_int)]  # ABI 4; zero = "as before" (ctypes zero-fills omitted fields)


class VaeResnet(C.Structure):  # include/lfm_hip.h: lfm_vae_resnet
    _fields_ = [(n, C.c_void_p) for n in ("n1_g", "n1_b", "c1_w", "c1_b", "n2_g", "n2_b", "c2_w", "c2_b", "sc_w", "sc_b")] + [
        ("cin", C.c_int), ("cout", C.c_int)]


ABI_VERSION = 4  # include/lfm_hip.h: lfm_abi_version()
CALL_OFF, CALL_ON = 1, 2  # lfm_dit_call.fold_ln


def call_gemm_select(which):
    """lfm_dit_call.gemm_select value for the kernel selection `which` (what lfm_gemm_select would take): per call, not library-wide."""
    return int(which) + 1


def lib():
    """Load the shared library.  With hipcc present the stamp-checked in-tree build runs first (a no-op when the sources are
    unchanged, a rebuild when they are stale); without hipcc the prebuilt library is used as shipped."""
    global _lib
    if _lib is not None:
        return _lib
    from . import _build

    override = os.environ.get("LFM_HIP_LIBRARY")  # measurement A/B only (tools/): a prebuilt experiment build of the SAME ABI instead of the in-tree one
    if override:
        if not os.path.exists(override):
            raise LfmHipError(f"LFM_HIP_LIBRARY={override} does not exist")
        path = override
    else:
        path = LIB_PATH
    if not override and (os.path.exists(_build.HIPCC) or not os.path.exists(LIB_PATH)):
        try:
            _build.build()
        except Exception as e:  # noqa
            if not os.path.exists(LIB_PATH):
                raise LfmHipError(f"liblfm_hip.so is missing and could not be built: {e}") from e
            raise LfmHipError(f"liblfm_hip.so is stale and could not be rebuilt: {e}") from e
    try:
        L = C.CDLL(path)
    except OSError as e:
        raise LfmHipError(f"cannot load {path}: {e}") from e
    L.lfm_strerror.restype = C.c_char_p
    L.lfm_strerror.argtypes = [C.c_int]
    L.lfm_abi_version.restype = C.c_int
    if L.lfm_abi_version() != ABI_VERSION:  # a stale prebuilt library would read the call structs of another layout
        raise LfmHipError(f"{path} has ABI {L.lfm_abi_version()}, this package binds ABI {ABI_VERSION}: rebuild it (python -m lfm_amd._build --force)")
    L.lfm_dit_workspace_bytes.restype = C.c_size_t
    L.lfm_dit_workspace_bytes.argtypes = [C.POINTER(DitShape), C.c_int]
    L.lfm_dit_workspace_layout.restype = C.c_int
    L.lfm_dit_workspace_layout.argtypes = [C.POINTER(DitShape), C.c_int, C.POINTER(C.c_size_t), C.c_int]
    L.lfm_dit_forward.restype = C.c_int
    L.lfm_dit_forward.argtypes = [C.POINTER(DitShape), C.POINTER(DitWeights), C.c_void_p, C.c_size_t, C.POINTER(DitCall), C.c_void_p]
    L.lfm_gemm_f16.restype = C.c_int
    L.lfm_gemm_f16.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_int, C.c_int, C.c_int,
                               C.c_void_p, C.c_int, C.c_void_p, C.c_long, C.c_int, C.c_void_p]
    L.lfm_dit_cond_table_bytes.restype = C.c_size_t
    L.lfm_dit_cond_table_bytes.argtypes = [C.c_void_p, C.c_int]
    L.lfm_dit_cond_table_build.restype = C.c_int
    L.lfm_dit_cond_table_build.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    L.lfm_clock_probe.restype = C.c_int
    L.lfm_clock_probe.argtypes = [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    L.lfm_gemm_select.restype = C.c_int
    L.lfm_gemm_select.argtypes = [C.c_int]
    L.lfm_gemm_qkv_f16.restype = C.c_int
    L.lfm_gemm_qkv_f16.argtypes = [C.c_void_p, C.c_long, C.c_void_p, C.c_long, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    if hasattr(L, "lfm_gemm_trace_read"):  # LFM_MEASURE builds only
        L.lfm_gemm_trace_read.restype = C.c_int
        L.lfm_gemm_trace_read.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
        L.lfm_attention_trace_read.restype = C.c_int
        L.lfm_attention_trace_read.argtypes = [C.POINTER(C.c_ulonglong), C.c_int]
    L.lfm_profile_fc1.restype = C.c_int
    L.lfm_profile_fc1.argtypes = [C.c_int]
    L.lfm_profile_fc1_read.restype = C.c_int
    L.lfm_profile_fc1_read.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.lfm_profile_blocks_read.restype = C.c_int
    L.lfm_profile_blocks_read.argtypes = [C.POINTER(C.c_float), C.c_int]
    L.lfm_ln_modulate.restype = C.c_int
    L.lfm_ln_modulate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_long, C.c_void_p]
    L.lfm_dit_attention.restype = C.c_int
    L.lfm_dit_attention.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lfm_set_option.restype = C.c_int
    L.lfm_set_option.argtypes = [C.c_int, C.c_int]
    L.lfm_dit_call_settings.restype = C.c_int
    L.lfm_dit_call_settings.argtypes = [C.POINTER(DitCall), C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.lfm_dit_plan.restype = C.c_int
    L.lfm_dit_plan.argtypes = [C.POINTER(DitShape), C.POINTER(DitCall), C.POINTER(C.c_int)]
    L.lfm_gemm_plan.restype = C.c_int
    L.lfm_gemm_plan.argtypes = [C.c_int] * 5
    L.lfm_attention_plan.restype = C.c_int
    L.lfm_attention_plan.argtypes = [C.c_int] * 4
    L.lfm_dit_attention_hd.restype = C.c_int
    L.lfm_dit_attention_hd.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lfm_grid_advance.restype = C.c_int
    L.lfm_grid_advance.argtypes = [C.c_void_p] * 7
    L.lfm_lincomb.restype = C.c_int
    L.lfm_lincomb.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_void_p]
    L.lfm_rk_error_norm.restype = C.c_int
    L.lfm_rk_error_norm.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_long, C.c_float, C.c_float,
                                    C.c_void_p, C.c_void_p, C.c_void_p]
    L.lfm_vae_workspace_bytes.restype = C.c_size_t
    L.lfm_vae_workspace_bytes.argtypes = [C.c_int, C.c_int]
    L.lfm_vae_decode.restype = C.c_int
    L.lfm_vae_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lfm_vae_encode.restype = C.c_int
    L.lfm_vae_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lfm_images_to_uint8.restype = C.c_int
    L.lfm_images_to_uint8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    L.lfm_images_to_uint8_mode.restype = C.c_int
    L.lfm_images_to_uint8_mode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    V, I, LG, F = C.c_void_p, C.c_int, C.c_long, C.c_float
    L.lfm_conv3x3_f16.restype = I
    L.lfm_conv3x3_f16.argtypes = [V, V, V, V, V, I, I, I, I, I, I, V]
    L.lfm_conv3x3_workspace_bytes.restype = C.c_size_t
    L.lfm_conv3x3_workspace_bytes.argtypes = [I, I, I, I, I]
    L.lfm_conv3x3_f16_ws.restype = I
    L.lfm_conv3x3_f16_ws.argtypes = [V, V, V, V, V, I, I, I, I, I, I, V, C.c_size_t, V]
    L.lfm_conv3x3_in_f32.restype = I
    L.lfm_conv3x3_in_f32.argtypes = [V, V, V, V, I, I, I, I, I, V]
    L.lfm_conv3x3_out_f32.restype = I
    L.lfm_conv3x3_out_f32.argtypes = [V, V, V, V, I, I, I, I, I, V]
    L.lfm_linear_f16.restype = I
    L.lfm_linear_f16.argtypes = [V, LG, V, LG, V, LG, I, I, I, V, V, V]
    L.lfm_groupnorm_scratch_bytes.restype = C.c_size_t
    L.lfm_groupnorm_scratch_bytes.argtypes = [I, I]
    L.lfm_groupnorm_f16.restype = I
    L.lfm_groupnorm_f16.argtypes = [V, V, V, V, V, LG, V, I, I, I, I, F, I, V]
    L.lfm_groupnorm2_f16.restype = I
    L.lfm_groupnorm2_f16.argtypes = [V, I, V, I, V, V, V, V, LG, V, I, I, I, F, I, V]
    if hasattr(L, "lfm_groupnorm_plan"):  # additions to ABI 4: an LFM_HIP_LIBRARY built before them (the parent of an A/B) still loads
        L.lfm_groupnorm_plan.restype = I
        L.lfm_groupnorm_plan.argtypes = [I, I, I, I]
        L.lfm_vae_groupnorm_plan.restype = I
        L.lfm_vae_groupnorm_plan.argtypes = [I, I, I, C.c_size_t]
    L.lfm_linear2_f16.restype = I
    L.lfm_linear2_f16.argtypes = [V, I, V, I, V, LG, V, LG, I, I, V, V, V]
    L.lfm_avgpool2_f16.restype = I
    L.lfm_avgpool2_f16.argtypes = [V, V, I, I, I, I, V]
    L.lfm_upsample2_f16.restype = I
    L.lfm_upsample2_f16.argtypes = [V, V, I, I, I, I, V]
    L.lfm_concat_channels_f16.restype = I
    L.lfm_concat_channels_f16.argtypes = [V, V, V, LG, I, I, V]
    L.lfm_add_image_vec_f16.restype = I
    L.lfm_add_image_vec_f16.argtypes = [V, V, LG, V, I, I, I, V]
    L.lfm_attention_small_f16.restype = I
    L.lfm_attention_small_f16.argtypes = [V, V, I, I, I, I, V]
    L.lfm_unet_attention_plan.restype = I
    L.lfm_unet_attention_plan.argtypes = [I, I, I, I]
    L.lfm_cross_attention_f16.restype = I
    L.lfm_cross_attention_f16.argtypes = [V, LG, V, V, LG, V, LG, I, I, I, I, I, V]
    L.lfm_cross_attention_plan.restype = I
    L.lfm_cross_attention_plan.argtypes = [I, I, I, I, I]
    L.lfm_layernorm_f16.restype = I
    L.lfm_layernorm_f16.argtypes = [V, V, V, V, LG, I, F, V]
    L.lfm_geglu_f16.restype = I
    L.lfm_geglu_f16.argtypes = [V, LG, V, LG, I, V]
    L.lfm_time_embed.restype = I
    L.lfm_time_embed.argtypes = [V, I, V, V, V, V, V, V, I, V, V, V, I, I, I, V]
    L.lfm_conv3x3_scaled_f16_ws.restype = I
    L.lfm_conv3x3_scaled_f16_ws.argtypes = [V, V, V, V, F, V, I, I, I, I, I, I, V, C.c_size_t, V]
    L.lfm_conv3x3_plan.restype = I
    L.lfm_conv3x3_plan.argtypes = [I, I, I, I, I, I, C.c_size_t]
    L.lfm_linear_scaled_f16.restype = I
    L.lfm_linear_scaled_f16.argtypes = [V, LG, V, LG, V, LG, I, I, I, V, V, F, V]
    L.lfm_linear2_scaled_f16.restype = I
    L.lfm_linear2_scaled_f16.argtypes = [V, I, V, I, V, LG, V, LG, I, I, V, V, F, V]
    L.lfm_linear_resid_vec_f16.restype = I
    L.lfm_linear_resid_vec_f16.argtypes = [V, LG, V, LG, V, LG, I, I, I, V, V, V, LG, I, F, V]
    L.lfm_linear_silu_f16.restype = I
    L.lfm_linear_silu_f16.argtypes = [V, LG, V, LG, V, LG, I, I, I, V, V]
    L.lfm_linear_gelu_f16.restype = I
    L.lfm_linear_gelu_f16.argtypes = [V, LG, V, LG, V, LG, I, I, I, V, V]
    L.lfm_token_embed_f16.restype = I
    L.lfm_token_embed_f16.argtypes = [V, I, V, I, V, V, I, I, I, V]
    L.lfm_gather_rows_f32.restype = I
    L.lfm_gather_rows_f32.argtypes = [V, I, I, V, I, V, LG, V]
    L.lfm_label_rescale_f32.restype = I
    L.lfm_label_rescale_f32.argtypes = [V, V, V, V, I, I, I, I, I, I, V]
    if hasattr(L, "lfm_jpeg_encode_rgb8"):  # additions to ABI 4 (an LFM_HIP_LIBRARY built before them still loads; jpeg_encode then fails loudly)
        L.lfm_jpeg_encode_workspace_bytes.restype = C.c_size_t
        L.lfm_jpeg_encode_workspace_bytes.argtypes = [I, I, I, I]
        L.lfm_jpeg_encode_rgb8.restype = I
        L.lfm_jpeg_encode_rgb8.argtypes = [V, I, I, I, I, I, V, C.c_size_t, V, V, V]
    if hasattr(L, "lfm_inpaint_prepare_u8"):  # additions to ABI 4 (an LFM_HIP_LIBRARY built before them still loads; the inpaint_* wrappers then fail loudly)
        L.lfm_inpaint_prepare_u8.restype = I
        L.lfm_inpaint_prepare_u8.argtypes = [V, V, V, V, V, LG, I, I, I, V]
        L.lfm_inpaint_cond_f32.restype = I
        L.lfm_inpaint_cond_f32.argtypes = [V, V, F, V, LG, I, I, V]
        L.lfm_inpaint_composite_u8.restype = I
        L.lfm_inpaint_composite_u8.argtypes = [V, V, V, V, I, I, I, V]
    if hasattr(L, "lfm_ssim_u8"):  # additions to ABI 4, likewise (ssim_u8 / ssim_f32 fail loudly without them)
        L.lfm_ssim_workspace_bytes.restype = C.c_size_t
        L.lfm_ssim_workspace_bytes.argtypes = [I, I, I]
        L.lfm_ssim_u8.restype = I
        L.lfm_ssim_u8.argtypes = [V, V, V, I, I, I, V, I, V, C.c_size_t, V, V, V]
        L.lfm_ssim_f32.restype = I
        L.lfm_ssim_f32.argtypes = [V, V, I, I, I, I, V, I, V, C.c_size_t, V, V]
    L.lfm_song_embed.restype = I
    L.lfm_song_embed.argtypes = [V, I, V, V, V, V, V, V, F, V, I, V, V, V, I, I, I, V]
    L.lfm_fourier_embed.restype = I
    L.lfm_fourier_embed.argtypes = [V, I, V, V, V, V, V, V, V, F, V, I, V, V, V, I, I, I, V]
    L.lfm_fir_down2_f16.restype = I
    L.lfm_fir_down2_f16.argtypes = [V, V, V, V, F, I, I, I, I, I, V]
    L.lfm_fir_up2_f16.restype = I
    L.lfm_fir_up2_f16.argtypes = [V, V, I, I, I, I, V]
    L.lfm_zero_border_f16.restype = I
    L.lfm_zero_border_f16.argtypes = [V, V, I, I, I, I, V]
    L.lfm_zero_border_f32.restype = I
    L.lfm_zero_border_f32.argtypes = [V, V, I, I, I, V]
    L.lfm_vae_groupnorm_f16.restype = I
    L.lfm_vae_groupnorm_f16.argtypes = [V, V, V, V, V, C.c_size_t, I, I, I, I, V]
    L.lfm_vae_conv3x3_gn_f16.restype = I
    L.lfm_vae_conv3x3_gn_f16.argtypes = [V, V, V, V, V, V, V, V, V, C.c_size_t, I, I, I, I, I, I, I, C.POINTER(C.c_int), C.POINTER(C.c_int), V]
    L.lfm_vae_mid_attention_workspace_bytes.restype = C.c_size_t
    L.lfm_vae_mid_attention_workspace_bytes.argtypes = [I, I]
    L.lfm_vae_mid_attention_f16.restype = I
    L.lfm_vae_mid_attention_f16.argtypes = [V] * 13 + [C.c_size_t, I, I, V]
    L.lfm_vae_conv_in_f16.restype = I
    L.lfm_vae_conv_in_f16.argtypes = [V] * 6 + [I, I, V]
    L.lfm_vae_downsample_workspace_bytes.restype = C.c_size_t
    L.lfm_vae_downsample_workspace_bytes.argtypes = [I, I, I, I]
    L.lfm_vae_downsample_f16.restype = I
    L.lfm_vae_downsample_f16.argtypes = [V] * 5 + [C.c_size_t, I, I, I, I, V]
    L.lfm_vae_resnets_workspace_bytes.restype = C.c_size_t
    L.lfm_vae_resnets_workspace_bytes.argtypes = [I, I, I]
    L.lfm_vae_resnets_f16.restype = I
    L.lfm_vae_resnets_f16.argtypes = [C.POINTER(VaeResnet), I, V, V, V, C.c_size_t, I, I, I, I, C.POINTER(C.c_int), V]
    L.lfm_vae_conv_moments_workspace_bytes.restype = C.c_size_t
    L.lfm_vae_conv_moments_workspace_bytes.argtypes = [I, I, I]
    L.lfm_vae_conv_moments_f32.restype = I
    L.lfm_vae_conv_moments_f32.argtypes = [V] * 5 + [C.c_size_t, I, I, I, V]
    _lib = L
    return L


def check(rc, what):
    if rc != 0:
        raise LfmHipError(f"{what} failed: {lib().lfm_strerror(rc).decode()} (code {rc})")


def stream_ptr(device=None):
    """Raw hipStream_t of torch's current stream (so launches are ordered with torch ops and graph-capturable)."""
    return C.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def check_labels(y, rows, what, noun="label", table="the embedding table",
                 hint=" (classifier-free guidance needs a model built with label_dropout > 0: its null class is row num_classes)"):
    """Labels must index the embedding table (the reference's nn.Embedding raises IndexError otherwise; a kernel cannot).  The check
    reads two scalars back from the device, so the verdict is remembered ON THE TENSOR OBJECT (attribute, keyed by its version counter and
    the table size; `noun` / `table` / `hint` word the message for other index tensors: the layout encoder's tokens) -- a solver loop that passes the same label tensor to every evaluation pays once, while a fresh tensor that merely
    reuses a freed tensor's address is checked again.  Skipped during graph capture (no readback possible there)."""
    if y is None or y.numel() == 0:
        return
    if y.is_cuda and torch.cuda.is_current_stream_capturing():
        return
    key = (y._version, y.numel(), rows)
    if getattr(y, "_lfm_labels_ok", None) == key:
        return
    lo, hi = (int(v) for v in torch.stack([y.min(), y.max()]).tolist())  # one readback
    if lo < 0 or hi >= rows:
        raise IndexError(f"{what}: {noun} {hi if hi >= rows else lo} is outside {table} [0, {rows}){hint}")
    try:
        y._lfm_labels_ok = key
    except Exception:  # noqa
        pass


def require_gpu(t, what):
    if not t.is_cuda:
        raise LfmHipError(f"{what}: tensor is on {t.device}; the LFM hot path only runs on an MI355X (no CPU fallback)")


# ----------------------------------------------------------------------------- thin op wrappers (used by tests)
def gemm_select(which):
    """Force a GEMM kernel (0 auto, 1 128x128, 4 256x128, 5 256x256 eight waves, 6 256x256 four waves; 7 / 8: gemm_f16 on the batch-1 kernels, 64x64 tiles /
    all rows x 16 columns) | ablation flags << 4; A/B measurements
    and parity tests only.  Raises on a value the library rejects (a silently ignored selection invalidates an A/B)."""
    check(lib().lfm_gemm_select(int(which)), "lfm_gemm_select")


def gemm_f16(A, W, bias=None, epilogue=0, out=None, gate=None, gate_stride=0, tokens=1):
    require_gpu(A, "gemm_f16")
    M, K = A.shape
    N = W.shape[0]
    if out is None:
        out = torch.empty(M, N, device=A.device, dtype=torch.float32 if epilogue in (2, 3) else torch.float16)
    check(lib().lfm_gemm_f16(ptr(A), A.stride(0), ptr(W), W.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), epilogue,
                             ptr(gate), gate_stride, tokens, stream_ptr()), "lfm_gemm_f16")
    return out


def gemm_qkv_f16(A, W, bias, head_dim, tokens):
    """Q, K [M, D] and V^T [M/tokens, D/head_dim, head_dim, tokens] of the fused attention input projection."""
    require_gpu(A, "gemm_qkv_f16")
    M, K = A.shape
    D = W.shape[0] // 3
    Q = torch.empty(M, D, device=A.device, dtype=torch.float16)
    Kt = torch.empty_like(Q)
    Vt = torch.empty(M // tokens, D // head_dim, head_dim, tokens, device=A.device, dtype=torch.float16)
    check(lib().lfm_gemm_qkv_f16(ptr(A), A.stride(0), ptr(W), W.stride(0), ptr(Q), ptr(Kt), ptr(Vt), M, D, K, ptr(bias), head_dim, tokens,
                                 stream_ptr()), "lfm_gemm_qkv_f16")
    return Q, Kt, Vt


def ln_modulate(X, shift, scale, tokens, mod_stride):
    require_gpu(X, "ln_modulate")
    M, D = X.shape
    A = torch.empty(M, D, device=X.device, dtype=torch.float16)
    check(lib().lfm_ln_modulate(ptr(X), ptr(A), M, D, tokens, ptr(shift), ptr(scale), mod_stride, stream_ptr()), "lfm_ln_modulate")
    return A


# Ablation flags of gemm_select (`kernel | flags << 4`) and lfm_dit_call.gemm_select: the names, values and meanings of csrc/debug_flags.h (the single
# definition; tests/test_host_logic.py compares the two).  NAME_SHIFT / NAME_MASK: a multi-bit field, value << NAME_SHIFT.  Several flags share bits.
DBG_GEMM_NO_EPILOGUE = 4
DBG_GEMM_SETPRIO = 8
DBG_GEMM_GM8 = 32
DBG_GEMM_GM2 = 64
DBG_GEMM_NO_XCD_REMAP = 128
DBG_GEMM_GM4 = 256
DBG_GEMM_NO_SPLITK = 512
DBG_GEMM_STORE8 = 1024
DBG_GEMM_PARITY_PRIO = 2048
DBG_GEMM_NEVER_V4 = 4096
DBG_GEMM_ALWAYS_V4 = 8192
DBG_GEMM_SPLITK128 = 65536
DBG_GEMM_ABL_SHIFT = 21
DBG_GEMM_ABL_MASK = 15
DBG_GEMM_OPT_SHIFT = 25
DBG_GEMM_OPT_MASK = 3
DBG_TRACE_GEMM = 2
DBG_TRACE_NO_STORES = 131072
DBG_TRACE_COL_SHIFT = 21
DBG_TRACE_COL_MASK = 15
DBG_ATT_WIDE = 256
DBG_ATT_MODE_SHIFT = 25
DBG_ATT_MODE_MASK = 3
DBG_QKV_TRACE = 2
DBG_QKV_NO_VT_WRITES = 262144
DBG_QKV_NO_QK_WRITES = 524288
DBG_QKV_PER_ITEM = 4194304
DBG_QKV_NO_KEY_LOOP = 33554432
DBG_QKV_TWO_KTILES = 67108864
DBG_LN_STORE8 = 32768
DBG_LN_BPERMUTE = 65536
DBG_LN_FOUR_ROWS = 262144
DBG_LN_TWO_ROWS = 524288
DBG_DIT_FINAL_ROUND1 = 1048576
DBG_DIT_PATCH_ROUND1 = 2097152
DBG_CONV_IMPLICIT_GEMM = 8388608
DBG_CONV_HALO_SMALL = 16777216
DBG_VAE_SEPARATE_STATS = 4194304
DBG_UNET_CONV_IN_SCALAR = 1
DBG_UNET_ATT_VALU = 16
DBG_UNET_GN_ROWS = 16384

OPT_FOLD_LN = 1  # adaLN LayerNorm-modulate folded into the GEMM epilogues, default on (include/lfm_hip.h)
OPT_SKINNY_GEMM = 4  # batch-1 DiT linears on the latency-mode kernels (1, default: csrc/gemm_sq64_kernel.h where rows % 64 == 0, else csrc/gemm_skinny_kernel.h; 2: always the latter; 0: split-K path)
OPT_ATTENTION_STREAM = 5  # 256-token hd-64 attention on persistent workgroups with an LDS ring of K / V^T stages (csrc/attention_stream_kernel.h), default on; 0: one workgroup per item
OPT_FUSED_QKV_ATTENTION = 6  # folded path, 256 tokens x hd 64: QKV projection + attention in one kernel (csrc/qkv_attention_kernel.h), default on; 0: two kernels
OPT_UNET_ATTENTION_STREAM = 7  # UNet attention shapes beyond the resident and the VALU kernel on the streamed kernel (csrc/unet_attention_stream_kernel.h; chooser: csrc/unet_attention_dispatch.h), default 1; 0: refused; 2: every shape it takes
OPT_ATTENTION_TILED = 8  # DiT attention at the token counts no other kernel serves on the tiled any-T kernel (csrc/attention_tiled_kernel.h), default 1; 0: refused; 2: every shape it takes
OPT_GEMM_V6 = 2  # chip-filling row-major GEMMs on the one-wave-per-SIMD 256x256 kernel (csrc/gemm256w_kernel.h) instead of the 8-wave one


def effective_clock_mhz(device=None, iters=20000):
    """The clock this GPU sustains under matrix load (lfm_clock_probe: one workgroup per CU streaming MFMAs on random operands for ~50 ms): s_memtime
    ticks of the slowest workgroup over the launch's wall time.  Boxes differ by several percent under the board power cap."""
    dev = torch.device(device or "cuda:0")
    n = torch.cuda.get_device_properties(dev).multi_processor_count
    ticks = torch.zeros(n, dtype=torch.int64, device=dev)
    for it in (200, iters):  # a short warm-up launch, then the measured one
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(torch.cuda.current_stream(dev))
        check(lib().lfm_clock_probe(n, it, ptr(ticks), stream_ptr(dev)), "lfm_clock_probe")
        e1.record(torch.cuda.current_stream(dev))
        torch.cuda.synchronize(dev)
    ms = e0.elapsed_time(e1)
    # Calibration (tools/clock_probe.py on an MI355X, round 4): the tick count is proportional to the MFMA count, not to wall time (20 802 844 ticks for
    # 2 560 000 MFMAs per SIMD in a 21.6 ms and in a 23.7 ms run) -- 8.13 ticks per 16-pass MFMA, i.e. one s_memtime tick = TWO shader cycles here; the
    # issue-bound estimate 16 cycles x MFMAs / wall time agrees within 2 %.
    return 2.0 * float(ticks.max()) / (ms * 1e3)


PLAN_FOLDED_LN, PLAN_FUSED_QKV_ATTENTION = 1, 2  # lfm_dit_plan bits


def dit_plan(shape, batch, t_len=1, labels=False, fold_ln=0, gemm_select=0):
    """LFM_PLAN_* bits of the block loop lfm_dit_forward would run for this shape / batch under the current library options (no launch, no GPU needed)."""
    call = DitCall()
    call.batch, call.t_len, call.y = int(batch), int(t_len), (1 if labels else None)  # y: only NULL-ness is read
    call.fold_ln, call.gemm_select = fold_ln, gemm_select
    plan = C.c_int(-1)
    check(lib().lfm_dit_plan(C.byref(shape), C.byref(call), C.byref(plan)), "lfm_dit_plan")
    return plan.value


DIT_WS_BUFFERS = ("X", "A", "A2", "QKVH", "mod", "ln_part", "cen0", "cen1", "uvq", "uvf")  # include/lfm_hip.h: lfm_dit_workspace_layout


def dit_workspace_layout(shape, batch):
    """{buffer name: byte offset} inside the workspace of an evaluation at this batch (csrc/dit.hip: carve; 0 where the shape has no such buffer; no GPU needed)."""
    offs = (C.c_size_t * len(DIT_WS_BUFFERS))()
    rc = lib().lfm_dit_workspace_layout(C.byref(shape), int(batch), offs, len(DIT_WS_BUFFERS))
    if rc < 0:
        check(rc, "lfm_dit_workspace_layout")
    assert rc == len(DIT_WS_BUFFERS), rc
    return dict(zip(DIT_WS_BUFFERS, (int(o) for o in offs)))


GEMM_CAP_V6, GEMM_CAP_FITS = 1, 2  # lfm_gemm_plan caps: row-major A and an epilogue the one-wave-per-SIMD kernel serves; operands within 32-bit buffer offsets


def gemm_plan(M, N, K, batch=1, caps=GEMM_CAP_V6 | GEMM_CAP_FITS):
    """The GEMM kernel (1 / 4 / 5 / 6) the library runs for this shape under the calling thread's current selection (no launch, no GPU needed)."""
    return lib().lfm_gemm_plan(int(M), int(N), int(K), int(batch), int(caps))


def attention_plan(batch, heads, head_dim, T):
    """The kernel id (1 .. 7, include/lfm_hip.h: lfm_attention_plan; 7 = the tiled any-T kernel) dit_attention runs for this shape under the calling thread's
    flags and the library options (OPT_ATTENTION_STREAM, OPT_ATTENTION_TILED), or LFM_ERR_SHAPE (-1) for a shape no kernel serves (no launch, no GPU needed)."""
    return lib().lfm_attention_plan(int(batch), int(heads), int(head_dim), int(T))


DIT_RESIDENT_TOKENS = (16, 64, 128, 256, 1024)  # token counts of the kernels with K / V^T resident in the LDS (csrc/attention_kernel.h)


def dit_tokens_served(tokens):
    """Whether a DiT attention kernel serves `tokens` tokens per image under the default library options (csrc/attention_dispatch.h: attention_choose, for
    head_dim 64 / 72): the resident kernels' 16 / 64 / 128 / 256 / 1024, or -- the tiled kernel -- the square of a grid side that is a multiple of 4
    with 144 <= tokens <= 3600.  Pure Python (a model is constructed without the library); tests/test_dit_attention_tiled_ref.py holds it against
    lfm_attention_plan."""
    tokens = int(tokens)
    if tokens in DIT_RESIDENT_TOKENS:
        return True
    side = math.isqrt(tokens) if tokens > 0 else 0
    return side * side == tokens and side % 4 == 0 and 144 <= tokens <= 3600


CONV_PLAN_HALO, CONV_PLAN_SPLITK, CONV_PLAN_GEMM = 1, 2, 3  # lfm_conv3x3_plan


def conv3x3_plan(N, H, W, Cin, Cout, mode=0, workspace_bytes=0):
    """The path (1 halo-tiled kernel, 2 split-K + finish kernel, 3 one implicit GEMM; include/lfm_hip.h: lfm_conv3x3_plan) lfm_conv3x3_f16_ws takes for this
    shape with 16-byte-aligned operands and that much workspace under the calling thread's flags, or LFM_ERR_SHAPE (-1) (no launch, no GPU needed)."""
    return lib().lfm_conv3x3_plan(int(N), int(H), int(W), int(Cin), int(Cout), int(mode), int(workspace_bytes))


GN_STATS_FUSED, GN_STATS_ROWS, GN_STATS_GROUPS4, GN_STATS_GROUPS1 = 1, 2, 3, 4  # lfm_groupnorm_plan: the statistics path
GN_APPLY_FUSED, GN_APPLY_OCTET, GN_APPLY_CHUNK = 1, 2, 3  # and the apply path


def groupnorm_plan(N, HW, C, groups):
    """(statistics path GN_STATS_*, apply path GN_APPLY_*) of lfm_groupnorm_f16 for this shape under the calling thread's flags (include/lfm_hip.h:
    lfm_groupnorm_plan, csrc/groupnorm_dispatch.h; lfm_groupnorm2_f16: C = Ca + Cb), or LFM_ERR_SHAPE (-1) (no launch, no GPU needed)."""
    plan = lib().lfm_groupnorm_plan(int(N), int(HW), int(C), int(groups))
    return plan if plan < 0 else (plan & 15, plan >> 4)


def vae_groupnorm_plan(n, HW, C, workspace_bytes):
    """The statistics slabs per image of lfm_vae_groupnorm_f16 for this shape and workspace size (include/lfm_hip.h: lfm_vae_groupnorm_plan), or
    LFM_ERR_SHAPE (-1) / LFM_ERR_WORKSPACE (-3) as that entry point refuses (no launch, no GPU needed)."""
    return lib().lfm_vae_groupnorm_plan(int(n), int(HW), int(C), int(workspace_bytes))


def unet_attention_plan(N, T, heads, ch):
    """The kernel (1 VALU, 2 resident MFMA, 3 streamed MFMA; include/lfm_hip.h: lfm_unet_attention_plan, csrc/unet_attention_dispatch.h) lfm_attention_small_f16 runs for this shape with
    16-byte-aligned operands under the calling thread's flags and the library options, or LFM_ERR_SHAPE (-1) (no launch, no GPU needed)."""
    return lib().lfm_unet_attention_plan(int(N), int(T), int(heads), int(ch))


def unet_attention(qkv, out, N, T, heads, ch):
    """lfm_attention_small_f16 on qkv fp16 [N*T, 3*heads*ch] -> out fp16 [N*T, heads*ch]; a shape no kernel serves is named with its limit."""
    if unet_attention_plan(N, T, heads, ch) < 0:
        raise LfmHipError(f"UNet attention: no kernel serves T = {T} tokens x {ch} channels per head (limit: channels per head % 16 == 0 and <= 256 for any "
                          f"token count; other widths only while min(T, 64) * (T + 1) * 4 + 4 * T * (ch + 2) <= {160 * 1024} bytes of LDS)")
    check(lib().lfm_attention_small_f16(ptr(qkv), ptr(out), N, T, heads, ch, stream_ptr(qkv.device)), "lfm_attention_small_f16")
    return out


def cross_attention_plan(N, Tq, Tk, heads, ch):
    """1 when lfm_cross_attention_f16 serves this shape (include/lfm_hip.h: any Tq, Tk >= 1; channels per head % 16 == 0 and <= 256), else LFM_ERR_SHAPE (-1)
    (no launch, no GPU needed)."""
    return lib().lfm_cross_attention_plan(int(N), int(Tq), int(Tk), int(heads), int(ch))


def cross_attention(Q, K, V, N, Tq, Tk, heads, ch, out=None):
    """lfm_cross_attention_f16: Q fp16 [N*Tq, heads*ch], K and V fp16 [N*Tk, heads*ch] -- row-strided views are read in place; K and V share a row stride
    (two column slices of one projection) -- -> out fp16 [N*Tq, heads*ch]; a shape the kernel does not serve is named with its limit."""
    require_gpu(Q, "cross_attention")
    if cross_attention_plan(N, Tq, Tk, heads, ch) < 0:
        raise LfmHipError(f"cross-attention: no kernel serves {Tq} queries x {Tk} keys x {ch} channels per head (limit: channels per head % 16 == 0 and "
                          "<= 256, any positive token counts)")
    if out is None:
        out = torch.empty(N * Tq, heads * ch, dtype=torch.float16, device=Q.device)
    C_ = heads * ch
    for name, t, rows in (("Q", Q, N * Tq), ("K", K, N * Tk), ("V", V, N * Tk), ("out", out, N * Tq)):
        if t.dtype != torch.float16 or tuple(t.shape) != (rows, C_) or t.stride(1) != 1 or t.device != Q.device:
            raise LfmHipError(f"cross-attention: {name} must be fp16 [{rows}, {C_}] with unit column stride on {Q.device}, got {t.dtype} {tuple(t.shape)} "
                              f"strides {t.stride()} on {t.device}")
    if K.stride(0) != V.stride(0):
        raise LfmHipError(f"cross-attention: K and V must share a row stride (two column slices of one buffer), got {K.stride(0)} and {V.stride(0)}")
    check(lib().lfm_cross_attention_f16(ptr(Q), Q.stride(0), ptr(K), ptr(V), K.stride(0), ptr(out), out.stride(0), N, Tq, Tk, heads, ch,
                                        stream_ptr(Q.device)), "lfm_cross_attention_f16")
    return out


def layernorm(x, gamma, beta, eps=1e-5, out=None):
    """lfm_layernorm_f16: nn.LayerNorm(C) on dense fp16 rows [M, C] (gamma, beta fp32 [C]) -> fp16 [M, C]."""
    require_gpu(x, "layernorm")
    M, C = x.shape
    if C % 8:
        raise LfmHipError(f"layernorm: {C} channels (limit: channels % 8 == 0)")
    if out is None:
        out = torch.empty(M, C, dtype=torch.float16, device=x.device)
    for name, t in (("x", x), ("out", out)):  # the kernel walks dense rows: a column slice of a wider buffer would be misread or overwritten
        if t.dtype != torch.float16 or tuple(t.shape) != (M, C) or t.stride() != (C, 1) or t.device != x.device:
            raise LfmHipError(f"layernorm: {name} must be dense fp16 [{M}, {C}] on {x.device}, got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    for name, t in (("gamma", gamma), ("beta", beta)):
        if t.dtype != torch.float32 or tuple(t.shape) != (C,) or t.stride() != (1,) or t.device != x.device:
            raise LfmHipError(f"layernorm: {name} must be dense fp32 [{C}] on {x.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    check(lib().lfm_layernorm_f16(ptr(x), ptr(out), ptr(gamma), ptr(beta), M, C, float(eps), stream_ptr(x.device)), "lfm_layernorm_f16")
    return out


def geglu(h, out=None):
    """lfm_geglu_f16: h fp16 [M, 2I] = [value | gate] (rows may be strided) -> value * gelu(gate) fp16 [M, I], the exact (erf) GELU."""
    require_gpu(h, "geglu")
    M, I2 = h.shape
    if I2 % 16:
        raise LfmHipError(f"geglu: {I2} columns (limit: half of them % 8 == 0)")
    if out is None:
        out = torch.empty(M, I2 // 2, dtype=torch.float16, device=h.device)
    if h.dtype != torch.float16 or h.stride(1) != 1:
        raise LfmHipError(f"geglu: h must be fp16 with unit column stride, got {h.dtype} strides {h.stride()}")
    if out.dtype != torch.float16 or tuple(out.shape) != (M, I2 // 2) or out.stride() != (I2 // 2, 1) or out.device != h.device:
        raise LfmHipError(f"geglu: out must be dense fp16 [{M}, {I2 // 2}] on {h.device}, got {out.dtype} {tuple(out.shape)} strides {out.stride()} on {out.device}")
    check(lib().lfm_geglu_f16(ptr(h), h.stride(0), ptr(out), M, I2 // 2, stream_ptr(h.device)), "lfm_geglu_f16")
    return out


def linear_resid_vec(x, w, bias, resid, vec, tokens, scale=1.0, out=None):
    """lfm_linear_resid_vec_f16: fp16 (x w^T + bias + resid + vec[m // tokens]) * scale; `vec` fp32 [M / tokens, N], a column slice of a wider buffer is read
    in place through its row stride (None: lfm_linear_scaled_f16's result)."""
    require_gpu(x, "linear_resid_vec")
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=x.device)
    if vec is not None and (vec.dtype != torch.float32 or tuple(vec.shape) != (M // tokens, N) or vec.stride(1) != 1):
        raise LfmHipError(f"linear_resid_vec: vec must be fp32 [{M // tokens}, {N}] with unit column stride, got {vec.dtype} {tuple(vec.shape)} strides {vec.stride()}")
    check(lib().lfm_linear_resid_vec_f16(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), ptr(resid), ptr(vec),
                                         vec.stride(0) if vec is not None else 0, int(tokens), float(scale), stream_ptr(x.device)), "lfm_linear_resid_vec_f16")
    return out


def linear_silu(x, w, bias, out=None):
    """lfm_linear_silu_f16: fp16 silu(x w^T + bias), SiLU in fp32 on the accumulator."""
    require_gpu(x, "linear_silu")
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=x.device)
    check(lib().lfm_linear_silu_f16(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), stream_ptr(x.device)),
          "lfm_linear_silu_f16")
    return out


def linear_gelu(x, w, bias, out=None):
    """lfm_linear_gelu_f16: fp16 gelu(x w^T + bias) with the exact (erf) GELU in fp32 on the accumulator; rows of x / w / out may be strided."""
    require_gpu(x, "linear_gelu")
    M, K = x.shape
    N = w.shape[0]
    if out is None:
        out = torch.empty(M, N, dtype=torch.float16, device=x.device)
    check(lib().lfm_linear_gelu_f16(ptr(x), x.stride(0), ptr(w), w.stride(0), ptr(out), out.stride(0), M, N, K, ptr(bias), stream_ptr(x.device)),
          "lfm_linear_gelu_f16")
    return out


def token_embed(tok_emb, pos_emb, ids, out=None):
    """lfm_token_embed_f16: fp16 (tok_emb[ids] + pos_emb[:L]) as rows [N*L, D]; tables dense fp32 [vocab, D] / [pos_rows, D], ids contiguous int64 [N, L] on
    the device.  No readback (capturable); an id outside the table gives a NaN row."""
    require_gpu(tok_emb, "token_embed")
    vocab, D = tok_emb.shape
    N, L = ids.shape
    for name, t in (("tok_emb", tok_emb), ("pos_emb", pos_emb)):
        if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != D or not t.is_contiguous() or t.device != tok_emb.device:
            raise LfmHipError(f"token_embed: {name} must be dense fp32 [rows, {D}] on {tok_emb.device}, got {t.dtype} {tuple(t.shape)} on {t.device}")
    if ids.dtype != torch.int64 or not ids.is_contiguous() or ids.device != tok_emb.device:
        raise LfmHipError(f"token_embed: ids must be contiguous int64 on {tok_emb.device}, got {ids.dtype} on {ids.device}")
    if out is None:
        out = torch.empty(N * L, D, dtype=torch.float16, device=tok_emb.device)
    if out.dtype != torch.float16 or tuple(out.shape) != (N * L, D) or not out.is_contiguous():
        raise LfmHipError(f"token_embed: out must be dense fp16 [{N * L}, {D}], got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    check(lib().lfm_token_embed_f16(ptr(tok_emb), vocab, ptr(pos_emb), pos_emb.shape[0], ptr(ids), ptr(out), N, L, D, stream_ptr(tok_emb.device)),
          "lfm_token_embed_f16")
    return out


def gather_rows(table, y, out=None):
    """lfm_gather_rows_f32: out[r] = table[y[r]]; table dense fp32 [rows, cols], y int64 on the device, out fp32 [N, cols] (rows may be strided).  The caller
    validates the labels (check_labels); no readback here, so the call is capturable."""
    require_gpu(table, "gather_rows")
    rows, cols = table.shape
    if table.dtype != torch.float32 or not table.is_contiguous() or y.dtype != torch.int64 or not y.is_contiguous() or y.device != table.device:
        raise LfmHipError(f"gather_rows: table must be dense fp32 and y contiguous int64 on {table.device}, got {table.dtype} / {y.dtype} on {y.device}")
    if out is None:
        out = torch.empty(y.numel(), cols, device=table.device)
    check(lib().lfm_gather_rows_f32(ptr(table), rows, cols, ptr(y), y.numel(), ptr(out), out.stride(0), stream_ptr(table.device)), "lfm_gather_rows_f32")
    return out


LABEL_RESCALE_MAX_STAGES, LABEL_RESCALE_MAX_COUT, LABEL_RESCALE_TABLE_BYTES = 4, 8, 65536  # include/lfm_hip.h: lfm_label_rescale_f32


def label_rescale_serves(num_cls, cout, n_stages):
    """The limits of lfm_label_rescale_f32 that do not depend on the label map."""
    return 1 <= n_stages <= LABEL_RESCALE_MAX_STAGES and 1 <= cout <= LABEL_RESCALE_MAX_COUT and num_cls >= 1 and num_cls * cout * 4 <= LABEL_RESCALE_TABLE_BYTES


def label_rescale(labels, w, bias, n_stages, out=None):
    """lfm_label_rescale_f32: out[n, o, i, j] = mean over the 2^n x 2^n cell of w[o, labels[n, y, x]] (+ bias[o]); labels contiguous int64 [N, H, W] on the
    device, w dense fp32 [Cout, num_cls], bias fp32 [Cout] or None, out fp32 [N, Cout, H >> n, W >> n].  No readback (capturable); a label outside
    [0, num_cls) gives a NaN cell."""
    require_gpu(labels, "label_rescale")
    if labels.dtype != torch.int64 or labels.dim() != 3 or not labels.is_contiguous():
        raise LfmHipError(f"label_rescale: labels must be contiguous int64 [N, H, W], got {labels.dtype} {tuple(labels.shape)} strides {labels.stride()}")
    N, H, W = labels.shape
    if w.dtype != torch.float32 or w.dim() != 2 or not w.is_contiguous() or w.device != labels.device:
        raise LfmHipError(f"label_rescale: w must be dense fp32 [Cout, num_cls] on {labels.device}, got {w.dtype} {tuple(w.shape)} on {w.device}")
    cout, num_cls = w.shape
    if bias is not None and (bias.dtype != torch.float32 or tuple(bias.shape) != (cout,) or not bias.is_contiguous() or bias.device != labels.device):
        raise LfmHipError(f"label_rescale: bias must be dense fp32 [{cout}] on {labels.device}, got {bias.dtype} {tuple(bias.shape)} on {bias.device}")
    shape = (N, cout, H >> n_stages, W >> n_stages)
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=labels.device)
    if out.dtype != torch.float32 or tuple(out.shape) != shape or not out.is_contiguous() or out.device != labels.device:
        raise LfmHipError(f"label_rescale: out must be dense fp32 {shape} on {labels.device}, got {out.dtype} {tuple(out.shape)} strides {out.stride()}")
    check(lib().lfm_label_rescale_f32(ptr(labels), ptr(w), ptr(bias), ptr(out), N, H, W, num_cls, cout, int(n_stages), stream_ptr(labels.device)),
          "lfm_label_rescale_f32")
    return out


JPEG_MAX_DIM = 4096  # csrc/jpeg_encode.h
# (device index, stream) -> uint8 workspace, grown on demand: calls on one stream are ordered, calls on two streams (the drivers' lanes) must not share one.
# A call under graph capture never reads or feeds this cache: its workspace comes from the graph's own pool and belongs to the graph.
_jpeg_ws = {}


def jpeg_default_capacity(H, W):
    """Bytes per image hip.jpeg_encode reserves unless told otherwise: one per pixel of the image rounded up to whole MCUs, several times what a photograph-like
    sample takes at quality 75 (noise at quality 100 takes more: its true length still comes back, and io_formats falls back to Pillow)."""
    return (-(-H // 16) * 16) * (-(-W // 16) * 16)


def jpeg_encode(img_u8, quality=75, capacity=None):
    """lfm_jpeg_encode_rgb8: contiguous uint8 [N, H, W, 3] RGB on the device -> (out uint8 [N, capacity], lengths int32 [N]).  out[i, :lengths[i]] is what follows
    the header (io_formats.jpeg_header) in the file PIL.Image.save writes for image i; lengths[i] is the true length also when it exceeds `capacity` (then out[i]
    holds the first `capacity` bytes).  No readback, current stream.  Capturable: under capture the outputs AND the workspace are allocated from the graph's
    private pool (they live as long as the graph does, and no eager call ever sees that memory); outside a capture the workspace is cached per stream."""
    require_gpu(img_u8, "jpeg_encode")
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3 or not img_u8.is_contiguous():
        raise LfmHipError(f"jpeg_encode: images must be contiguous uint8 [N, H, W, 3], got {img_u8.dtype} {tuple(img_u8.shape)} strides {img_u8.stride()}")
    N, H, W, _ = img_u8.shape
    cap = jpeg_default_capacity(H, W) if capacity is None else int(capacity)
    L = lib()
    if not hasattr(L, "lfm_jpeg_encode_rgb8"):
        raise LfmHipError("this liblfm_hip.so has no lfm_jpeg_encode_rgb8: rebuild it (python -m lfm_amd._build --force)")
    need = L.lfm_jpeg_encode_workspace_bytes(N, H, W, cap)
    if need == 0:
        raise LfmHipError(f"jpeg_encode: unsupported shape N={N} H={H} W={W} capacity={cap} (1 <= H, W <= {JPEG_MAX_DIM}, N >= 1, capacity >= 1)")
    dev = img_u8.device
    stream = torch.cuda.current_stream(dev)
    if torch.cuda.is_current_stream_capturing():
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
    else:
        key = (dev.index, stream.cuda_stream)
        ws = _jpeg_ws.get(key)
        if ws is None or ws.numel() < need:
            ws = _jpeg_ws[key] = torch.empty(need, dtype=torch.uint8, device=dev)
    out = torch.empty((N, cap), dtype=torch.uint8, device=dev)
    lengths = torch.empty((N,), dtype=torch.int32, device=dev)
    check(L.lfm_jpeg_encode_rgb8(ptr(img_u8), N, H, W, int(quality), cap, ptr(ws), ws.numel(), ptr(out), ptr(lengths), C.c_void_p(stream.cuda_stream)),
          "lfm_jpeg_encode_rgb8")
    if torch.cuda.is_current_stream_capturing():
        out._lfm_jpeg_ws = ws  # the graph's workspace lives as long as the graph's output does
    return out, lengths


def _inpaint_lib():
    L = lib()
    if not hasattr(L, "lfm_inpaint_prepare_u8"):
        raise LfmHipError("this liblfm_hip.so has no lfm_inpaint_prepare_u8: rebuild it (python -m lfm_amd._build --force)")
    return L


def _inpaint_bytes(what, img_u8, mask_u8):
    """The shape checks of the inpainting kernels' byte inputs -> (N, H, W)."""
    require_gpu(img_u8, what)
    if img_u8.dtype != torch.uint8 or img_u8.dim() != 4 or img_u8.shape[-1] != 3 or not img_u8.is_contiguous():
        raise LfmHipError(f"{what}: images must be contiguous uint8 [N, H, W, 3], got {img_u8.dtype} {tuple(img_u8.shape)} strides {img_u8.stride()}")
    N, H, W, _ = img_u8.shape
    if mask_u8.dtype != torch.uint8 or tuple(mask_u8.shape) != (N, H, W) or not mask_u8.is_contiguous() or mask_u8.device != img_u8.device:
        raise LfmHipError(f"{what}: masks must be contiguous uint8 [{N}, {H}, {W}] on {img_u8.device}, got {mask_u8.dtype} {tuple(mask_u8.shape)} on "
                          f"{mask_u8.device}")
    if H % 8 or W % 8 or N < 1:
        raise LfmHipError(f"{what}: H and W must be multiples of 8 and N >= 1, got N={N} H={H} W={W}")
    return N, H, W


def _inpaint_f32(what, name, t, shape, device):
    if t.dtype != torch.float32 or tuple(t.shape) != shape or not t.is_contiguous() or t.device != device:
        raise LfmHipError(f"{what}: {name} must be dense fp32 {shape} on {device}, got {t.dtype} {tuple(t.shape)} strides {t.stride()} on {t.device}")
    return t


def inpaint_prepare(img_u8, mask_u8, cond, want_image=False):
    """lfm_inpaint_prepare_u8: uint8 NHWC images [N,H,W,3] and the mask PNG's bytes [N,H,W] (255 = keep) -> (masked image fp32 [N,3,H,W] in [-1,1], the VAE
    encoder's input; the image itself likewise, or None), and channel 4 of `cond` (dense fp32 [N,5,H/8,W/8]) = the mask in {-1..+1} (+1 = hole) picked at
    [::8, ::8].  The reference's dataset arithmetic, bit for bit.  Channels 0..3 of `cond` are not written.  No readback (capturable)."""
    L = _inpaint_lib()
    N, H, W = _inpaint_bytes("inpaint_prepare", img_u8, mask_u8)
    h, w = H // 8, W // 8
    _inpaint_f32("inpaint_prepare", "cond", cond, (N, 5, h, w), img_u8.device)
    masked = torch.empty(N, 3, H, W, dtype=torch.float32, device=img_u8.device)
    image = torch.empty_like(masked) if want_image else None
    check(L.lfm_inpaint_prepare_u8(ptr(img_u8), ptr(mask_u8), ptr(masked), ptr(image), C.c_void_p(cond.data_ptr() + 4 * h * w * 4), 5 * h * w, N, H, W,
                                   stream_ptr(img_u8.device)), "lfm_inpaint_prepare_u8")
    return masked, image


def inpaint_cond(moments, eps, scale, cond):
    """lfm_inpaint_cond_f32: cond[:, :4] = (mean + exp(0.5 * clamp(logvar, -30, 20)) * eps) * scale from the VAE encoder's moments fp32 [N,8,h,w]
    (mean | logvar) and eps fp32 [N,4,h,w]; eps None: mean * scale (the posterior's mode).  cond dense fp32 [N,5,h,w]; its channel 4 is not written.  No
    readback (capturable).  Returns cond."""
    L = _inpaint_lib()
    require_gpu(moments, "inpaint_cond")
    if moments.dim() != 4 or moments.shape[1] != 8:
        raise LfmHipError(f"inpaint_cond: moments must be fp32 [N, 8, h, w], got {tuple(moments.shape)}")
    N, _, h, w = moments.shape
    _inpaint_f32("inpaint_cond", "moments", moments, (N, 8, h, w), moments.device)
    if eps is not None:
        _inpaint_f32("inpaint_cond", "eps", eps, (N, 4, h, w), moments.device)
    _inpaint_f32("inpaint_cond", "cond", cond, (N, 5, h, w), moments.device)
    check(L.lfm_inpaint_cond_f32(ptr(moments), ptr(eps), float(scale), ptr(cond), 5 * h * w, N, h * w, stream_ptr(moments.device)), "lfm_inpaint_cond_f32")
    return cond


def inpaint_composite(fake, img_u8, mask_u8, out=None):
    """lfm_inpaint_composite_u8: decoded sample fp32 [N,3,H,W] in [-1,1] + the image and mask bytes -> uint8 NHWC [N,H,W,3]: the reference's composite
    fake01 * mask01 + (1 - mask01) * image01 (:157-160) as torchvision.utils.save_image quantises it, bit for bit.  No readback (capturable)."""
    L = _inpaint_lib()
    N, H, W = _inpaint_bytes("inpaint_composite", img_u8, mask_u8)
    _inpaint_f32("inpaint_composite", "fake", fake, (N, 3, H, W), img_u8.device)
    if out is None:
        out = torch.empty(N, H, W, 3, dtype=torch.uint8, device=img_u8.device)
    if out.dtype != torch.uint8 or tuple(out.shape) != (N, H, W, 3) or not out.is_contiguous() or out.device != img_u8.device:
        raise LfmHipError(f"inpaint_composite: out must be contiguous uint8 [{N}, {H}, {W}, 3] on {img_u8.device}, got {out.dtype} {tuple(out.shape)}")
    check(L.lfm_inpaint_composite_u8(ptr(fake), ptr(img_u8), ptr(mask_u8), ptr(out), N, H, W, stream_ptr(img_u8.device)), "lfm_inpaint_composite_u8")
    return out


SSIM_MAX_DIM = 4096  # csrc/ssim.h
_ssim_windows = {}  # (device, window_size) -> the 1-D window on that device


def ssim_gaussian(window_size, sigma=1.5):
    """The reference's ``SSIM._gaussian`` (losses/ssim.py:36-40), operation for operation: a Python-float exp per tap, ``torch.Tensor`` (fp32), divided by
    its fp32 sum.  fp32 [window_size] on the host."""
    import numpy as np

    g = torch.Tensor([np.exp(-((x - (window_size // 2)) ** 2) / float(2 * sigma**2)) for x in range(window_size)])
    return g / g.sum()


def _ssim_setup(what, device, N, H, W, window_size):
    """-> (library, window on `device`, workspace, its size) for one call; the workspace is a fresh block of the caching allocator on the current stream."""
    L = lib()
    if not hasattr(L, "lfm_ssim_u8"):
        raise LfmHipError("this liblfm_hip.so has no lfm_ssim_u8: rebuild it (python -m lfm_amd._build --force)")
    ws = int(window_size)
    if ws < 3 or ws > 11 or ws % 2 == 0:
        raise LfmHipError(f"{what}: window_size must be odd and 3..11, got {window_size}")
    need = L.lfm_ssim_workspace_bytes(N, H, W)
    if need == 0:
        raise LfmHipError(f"{what}: unsupported shape N={N} H={H} W={W} (N >= 1, 1 <= H, W <= {SSIM_MAX_DIM})")
    key = (device, ws)
    window = _ssim_windows.get(key)
    if window is None:  # (a first call under graph capture would put the copy into the graph: warm up outside, as for every capture)
        window = _ssim_windows[key] = ssim_gaussian(ws).to(device)
    return L, window, torch.empty(need, dtype=torch.uint8, device=device), need


def ssim_u8(a, b, mask=None, window_size=11):
    """lfm_ssim_u8: two contiguous uint8 NHWC batches [N,H,W,3] on the device (each byte / 255) -> (SSIM per image fp32 [N], as the reference's
    ``SSIM(window_size, size_average=False)`` gives it; the int64 sum of each image's mask bytes [N], or None without a mask uint8 [N,H,W]).  One tile kernel
    and one reduce kernel on the current stream, no readback (capturable); bit-reproducible, independent of N and of the image's place in the batch."""
    require_gpu(a, "ssim_u8")
    for name, t in (("a", a), ("b", b)):
        if t.dtype != torch.uint8 or t.dim() != 4 or t.shape[-1] != 3 or not t.is_contiguous() or t.shape != a.shape or t.device != a.device:
            raise LfmHipError(f"ssim_u8: {name} must be contiguous uint8 [N, H, W, 3] on {a.device}, both alike, got {t.dtype} {tuple(t.shape)} strides "
                              f"{t.stride()} on {t.device}")
    N, H, W, _ = a.shape
    if mask is not None and (mask.dtype != torch.uint8 or tuple(mask.shape) != (N, H, W) or not mask.is_contiguous() or mask.device != a.device):
        raise LfmHipError(f"ssim_u8: mask must be contiguous uint8 [{N}, {H}, {W}] on {a.device}, got {mask.dtype} {tuple(mask.shape)} on {mask.device}")
    L, window, ws, need = _ssim_setup("ssim_u8", a.device, N, H, W, window_size)
    out = torch.empty(N, dtype=torch.float32, device=a.device)
    mask_sum = torch.empty(N, dtype=torch.int64, device=a.device) if mask is not None else None
    check(L.lfm_ssim_u8(ptr(a), ptr(b), ptr(mask), N, H, W, ptr(window), int(window_size), ptr(ws), need, ptr(out), ptr(mask_sum), stream_ptr(a.device)),
          "lfm_ssim_u8")
    return out, mask_sum


def ssim_f32(a, b, window_size=11):
    """lfm_ssim_f32: two contiguous fp32 NCHW batches [N,C,H,W] on the device, 1 <= C <= 4 -> SSIM per image fp32 [N] (``SSIM(window_size,
    size_average=False)``).  As ssim_u8 otherwise."""
    require_gpu(a, "ssim_f32")
    for name, t in (("a", a), ("b", b)):
        if t.dtype != torch.float32 or t.dim() != 4 or not t.is_contiguous() or t.shape != a.shape or t.device != a.device:
            raise LfmHipError(f"ssim_f32: {name} must be contiguous fp32 [N, C, H, W] on {a.device}, both alike, got {t.dtype} {tuple(t.shape)} strides "
                              f"{t.stride()} on {t.device}")
    N, Cn, H, W = a.shape
    if Cn < 1 or Cn > 4:
        raise LfmHipError(f"ssim_f32: 1 <= C <= 4, got C={Cn}")
    L, window, ws, need = _ssim_setup("ssim_f32", a.device, N, H, W, window_size)
    out = torch.empty(N, dtype=torch.float32, device=a.device)
    check(L.lfm_ssim_f32(ptr(a), ptr(b), N, Cn, H, W, ptr(window), int(window_size), ptr(ws), need, ptr(out), stream_ptr(a.device)), "lfm_ssim_f32")
    return out


def fir_down2(x, N, Ho, Wo, C, pad=1, bias=None, resid=None, scale=1.0, out=None):
    """lfm_fir_down2_f16: the [1,3,3,1] filter at stride 2 of x fp16 NHWC [N, 2Ho + 2 - 2pad, 2Wo + 2 - 2pad, C] onto the Ho x Wo grid,
    out = (filtered + bias + resid) * scale (bias fp32 [C], resid fp16 [N*Ho*Wo, C], both optional)."""
    require_gpu(x, "fir_down2")
    if out is None:
        out = torch.empty(N * Ho * Wo, C, dtype=torch.float16, device=x.device)
    check(lib().lfm_fir_down2_f16(ptr(x), ptr(out), ptr(bias), ptr(resid), float(scale), N, Ho, Wo, C, pad, stream_ptr(x.device)), "lfm_fir_down2_f16")
    return out


def fir_up2(x, N, Ho, Wo, C, out=None):
    """lfm_fir_up2_f16: the transposed [1,3,3,1] filter, x fp16 NHWC [N, Ho/2, Wo/2, C] -> [N*Ho*Wo, C]."""
    require_gpu(x, "fir_up2")
    if out is None:
        out = torch.empty(N * Ho * Wo, C, dtype=torch.float16, device=x.device)
    check(lib().lfm_fir_up2_f16(ptr(x), ptr(out), N, Ho, Wo, C, stream_ptr(x.device)), "lfm_fir_up2_f16")
    return out


def zero_border(x, N, H, W, C):
    """x inside a one-pixel border of zeros: fp16 NHWC [N*H*W, C] -> [N*(H+2)*(W+2), C] (lfm_zero_border_f16), or fp32 NCHW [N, C, H, W] ->
    [N, C, H+2, W+2] (lfm_zero_border_f32)."""
    require_gpu(x, "zero_border")
    if x.dtype == torch.float32:
        out = torch.empty(N, C, H + 2, W + 2, device=x.device)
        check(lib().lfm_zero_border_f32(ptr(x), ptr(out), N * C, H, W, stream_ptr(x.device)), "lfm_zero_border_f32")
    else:
        out = torch.empty(N * (H + 2) * (W + 2), C, dtype=torch.float16, device=x.device)
        check(lib().lfm_zero_border_f16(ptr(x), ptr(out), N, H, W, C, stream_ptr(x.device)), "lfm_zero_border_f16")
    return out


def set_option(key, value):
    check(lib().lfm_set_option(int(key), int(value)), "lfm_set_option")


def vt_token_perm(T, device=None):
    """Index tensor p with Vt_library[..., i] = Vt_plain[..., p[i]]: the V^T token order of the library (tokens of every 16-group stored as 0-3, 8-11, 4-7,
    12-15; include/lfm_hip.h: lfm_gemm_qkv_f16).  An involution: the same index restores the plain order."""
    i = torch.arange(T, device=device)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def dit_attention(Q, K, Vt, batch, heads, T, head_dim=64):
    """Q, K, O: fp16 [batch*T, heads*head_dim]; Vt: fp16 [batch, heads, head_dim, T] in the library's token order (vt_token_perm).  head_dim 64 or 72;
    T as dit_tokens_served says (attention_plan names the kernel)."""
    require_gpu(Q, "dit_attention")
    O = torch.empty_like(Q)
    check(lib().lfm_dit_attention_hd(ptr(Q), ptr(K), ptr(Vt), ptr(O), batch, heads, head_dim, T, stream_ptr()), "lfm_dit_attention_hd")
    return O


def rk_error_norm(y0, y1, ks, e_coef, dt, rtol, atol, scratch, out):
    """out[0] = sqrt(mean(((dt * sum e_j k_j) / (atol + rtol max(|y0|, |y1|)))^2)) -- device fp32 tensors; e_coef, dt, out on the device."""
    require_gpu(y0, "rk_error_norm")
    arr = (C.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
    check(lib().lfm_rk_error_norm(ptr(y0), ptr(y1), arr, ptr(e_coef), ptr(dt), len(ks), y0.numel(), float(rtol), float(atol), ptr(scratch), ptr(out),
                                  stream_ptr(y0.device)), "lfm_rk_error_norm")
    return out


def lincomb(out, base, ks, coef, scale=None):
    """out = base + (*scale) * sum coef[i]*ks[i]  (device fp32 tensors; coef/scale are device tensors)."""
    require_gpu(out, "lincomb")
    arr = (C.c_void_p * len(ks))(*[k.data_ptr() for k in ks])
    check(lib().lfm_lincomb(ptr(out), ptr(base), arr, ptr(coef), ptr(scale), len(ks), out.numel(), stream_ptr(out.device)), "lfm_lincomb")
    return out
