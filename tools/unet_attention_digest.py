"""SHA-256 of the raw output bytes of lfm_attention_small_f16, one line per case: evidence that a refactor of the UNet attention kernels
(csrc/unet_attention_common.h, unet_attention_kernel.h, unet_attention_stream_kernel.h, unet_attention_dispatch.h) keeps every result bit
(profiles/unet_attention_blocks_refactor.txt).  Run it once per library and compare the two outputs:
    python tools/unet_attention_digest.py > new.txt;  LFM_HIP_LIBRARY=/path/to/parent/liblfm_hip.so python tools/unet_attention_digest.py > parent.txt
Cases (those of tests/test_gpu_unet_attention_stream.py, same inputs: tests/unet_attention_cases.py): every (shape, family) of
test_streamed_kernel_serves_what_was_refused; every (shape, family) of test_streamed_kernel_forced_agrees_with_the_kernel_of_the_shape under
LFM_OPT_UNET_ATTENTION_STREAM = 1 and 2 and, where the VALU kernel's LDS fits, under flag UNET_ATT_VALU; the shapes of test_nothing_served_before_moved
under options 1 and 0.  Each line names the kernel the plan gives.  Not a test: a digest pins the compiler."""
import hashlib
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import unet_attention_cases as uc  # noqa: E402
from lfm_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
REFUSED = [(2, 2, 64, 333), (1, 2, 256, 130), (2, 3, 48, 577), (1, 2, 16, 1000), (3, 2, 128, 1024), (2, 2, 192, 320), (1, 1, 64, 4096)]
FORCED = [(2, 2, 64, 1), (2, 3, 64, 63), (2, 2, 64, 65), (1, 1, 32, 129), (2, 2, 64, 64), (2, 4, 64, 256), (2, 2, 128, 64), (2, 2, 96, 64), (1, 2, 128, 256)]
MOVED = [(2, 4, 128, 256), (3, 2, 64, 256), (2, 4, 64, 64), (1, 8, 128, 64), (2, 2, 96, 64)]


def digest(tag, family, shape, option, flags=0):
    N, heads, ch, T = shape
    tok = uc.tokens(uc.make_case(family, N, heads, ch, T)).to(dev)
    out = torch.zeros(N * T, heads * ch, dtype=torch.float16, device=dev)
    hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, option)
    hip.gemm_select(flags << 4)
    try:
        kern = hip.unet_attention_plan(N, T, heads, ch)
        hip.check(hip.lib().lfm_attention_small_f16(hip.ptr(tok), hip.ptr(out), N, T, heads, ch, hip.stream_ptr()), "lfm_attention_small_f16")
        torch.cuda.synchronize()
    finally:
        hip.gemm_select(0)
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 1)
    sha = hashlib.sha256(out.cpu().view(torch.uint8).numpy().tobytes()).hexdigest()
    print(f"DIGEST {tag} N{N} heads{heads} ch{ch} T{T} {family} option{option} flags{flags} kernel{kern} finite{bool(torch.isfinite(out).all())} {sha}", flush=True)


def valu_serves(shape):
    """Whether the VALU kernel's LDS fits the shape: the library's own answer under flag UNET_ATT_VALU (1, or LFM_ERR_SHAPE)."""
    N, heads, ch, T = shape
    hip.gemm_select(hip.DBG_UNET_ATT_VALU << 4)
    try:
        return hip.unet_attention_plan(N, T, heads, ch) == 1
    finally:
        hip.gemm_select(0)


if __name__ == "__main__":
    print(f"library {os.environ.get('LFM_HIP_LIBRARY') or hip.LIB_PATH}", flush=True)
    for shape in REFUSED:
        for family in uc.FAMILIES:
            digest("refused", family, shape, 1)
    for shape in FORCED:
        for family in uc.FAMILIES:
            digest("forced", family, shape, 1)
            digest("forced", family, shape, 2)
            if valu_serves(shape):
                digest("forced", family, shape, 1, hip.DBG_UNET_ATT_VALU)
    for shape in MOVED:
        digest("moved", "gauss", shape, 1)
        digest("moved", "gauss", shape, 0)
