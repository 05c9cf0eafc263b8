"""SHA-256 of the raw output bytes of the four GroupNorm entry points, one line per case: evidence that a refactor of the GroupNorm kernels and their host
code (csrc/groupnorm_common.h, groupnorm_kernels.h, groupnorm_dispatch.h, the GroupNorm parts of csrc/vae.hip) keeps every result bit
(profiles/groupnorm_refactor.txt).  Run it once per library and compare the two outputs:
    python tools/groupnorm_digest.py > new.txt;  LFM_HIP_LIBRARY=/path/to/parent/liblfm_hip.so python tools/groupnorm_digest.py > parent.txt
Cases: every row of UNET_CASES (lfm_groupnorm_f16), TWO_SOURCE_CASES (lfm_groupnorm2_f16), VAE_GN_CASES (lfm_vae_groupnorm_f16) and CONV_CASES
(lfm_vae_conv3x3_gn_f16: the convolution's output and the GroupNorm's) of tests/test_gpu_groupnorm.py, same inputs, in the `centred` and `offset300`
families, with FiLM where the case has it.  A PLAN line per case names the kernels / slab count where the library has the plan entry points (a
library from before them prints none: compare the DIGEST lines).  Not a test: a digest pins the compiler."""
import ctypes as C
import hashlib
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_gpu_groupnorm as t  # noqa: E402
from lfm_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
L = hip.lib()
FAMILIES = ["centred", "offset300"]
HAS_PLAN = hasattr(L, "lfm_groupnorm_plan")


def sha(x):
    torch.cuda.synchronize()
    return hashlib.sha256(x.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def show(entry, what, fam, plan, **outs):
    if HAS_PLAN:
        print(f"PLAN {entry} [{what}] {fam} {plan()}", flush=True)
    for name, x in outs.items():
        print(f"DIGEST {entry} [{what}] {fam} {name} finite{bool(torch.isfinite(x).all())} {sha(x)}", flush=True)


def unet(case, fam):
    N, HW, C_, groups, film_on, flags, _, what = case
    x = t.family(fam, N, HW, C_, groups, seed=HW + C_, dev=dev)
    gamma, beta, film = t.affine(C_, C_ + N, dev, N if film_on else 0)
    scr = torch.full((L.lfm_groupnorm_scratch_bytes(N, C_),), 255, dtype=torch.uint8, device=dev)
    y = torch.zeros_like(x)
    t.with_flags(flags, lambda: hip.check(L.lfm_groupnorm_f16(hip.ptr(x), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(film), 2 * C_ if film_on else 0,
                                                              hip.ptr(scr), N, HW, C_, groups, 1e-5, 1, hip.stream_ptr()), "lfm_groupnorm_f16"))
    show("lfm_groupnorm_f16", what, fam, lambda: t.with_flags(flags, lambda: hip.groupnorm_plan(N, HW, C_, groups)), y=y)


def two_source(case, fam):
    N, HW, Ca, Cb, film_on, _, what = case
    C_ = Ca + Cb
    xa = t.family(fam, N, HW, C_, t.G, seed=HW + Ca, dev=dev)[..., :Ca].contiguous()
    xb = t.family("centred", N, HW, Cb, 1, seed=HW + Cb + 1, dev=dev)
    gamma, beta, film = t.affine(C_, C_ + N, dev, N if film_on else 0)
    scr = torch.full((L.lfm_groupnorm_scratch_bytes(N, C_),), 255, dtype=torch.uint8, device=dev)
    y = torch.zeros(N, HW, C_, dtype=torch.float16, device=dev)
    hip.check(L.lfm_groupnorm2_f16(hip.ptr(xa), Ca, hip.ptr(xb), Cb, hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(film), 2 * C_ if film_on else 0,
                                   hip.ptr(scr), N, HW, t.G, 1e-5, 1, hip.stream_ptr()), "lfm_groupnorm2_f16")
    show("lfm_groupnorm2_f16", what, fam, lambda: hip.groupnorm_plan(N, HW, C_, t.G), y=y)


def vae(case, fam):
    n, HW, C_, _, what = case
    x = t.family(fam, n, HW, C_, t.G, seed=n + HW + C_, dev=dev)
    gamma, beta, _ = t.affine(C_, C_ + n, dev)
    ws = t.vae_gn_workspace(n, HW, C_, dev).fill_(255)
    y = torch.zeros_like(x)
    hip.check(L.lfm_vae_groupnorm_f16(hip.ptr(x), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(ws), ws.numel(), n, HW, C_, int(C_ != 512),
                                      hip.stream_ptr()), "lfm_vae_groupnorm_f16")
    show("lfm_vae_groupnorm_f16", what, fam, lambda: hip.vae_groupnorm_plan(n, HW, C_, ws.numel()), y=y)


def conv(case, fam):
    src, sel, n, H, Cin, Cout, ups, resid_on = case
    g = torch.Generator().manual_seed(n * 100 + H + Cout)
    bias, scale, family_resid = t.conv_family(fam, Cout, n + Cout)
    Hs, HW = H >> int(ups), H * H
    x = torch.randn(n, Hs, Hs, Cin, generator=g).half().to(dev)
    w = (torch.randn(Cout, 9 * Cin, generator=g) * (scale / (9 * Cin) ** 0.5)).half().to(dev)
    resid = (torch.randn(n, H, H, Cout, generator=g) * 0.5 if family_resid else torch.zeros(n, H, H, Cout)).half().to(dev) if resid_on else None
    bias = bias.float().to(dev)
    gamma, beta, _ = t.affine(Cout, Cout, dev)
    pairs = n * max(2 * (HW // 256) * Cout // 4, 64 * Cout // 4)
    ws = torch.full((256 + (n * 256 + 255) // 256 * 256 + pairs * 8,), 255, dtype=torch.uint8, device=dev)
    co = torch.zeros(n, HW, Cout, dtype=torch.float16, device=dev)
    y = torch.zeros_like(co)
    slabs, kern = C.c_int(-1), C.c_int(-1)
    t.with_flags(sel, lambda: hip.check(L.lfm_vae_conv3x3_gn_f16(
        hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(resid), hip.ptr(co), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(ws), ws.numel(), n, H, H, Cin,
        Cout, int(ups), 1, C.byref(slabs), C.byref(kern), hip.stream_ptr()), "lfm_vae_conv3x3_gn_f16"))
    what = f"{src} n{n} {H}px {Cin}to{Cout}{' ups' if ups else ''}{' resid' if resid_on else ''} slabs{slabs.value} kernel{kern.value}"
    show("lfm_vae_conv3x3_gn_f16", what, fam, lambda: "(reported by the call)", conv_out=co, y=y)


if __name__ == "__main__":
    print(f"library {os.environ.get('LFM_HIP_LIBRARY') or hip.LIB_PATH}", flush=True)
    for run, cases in ((unet, t.UNET_CASES), (two_source, t.TWO_SOURCE_CASES), (vae, t.VAE_GN_CASES), (conv, t.CONV_CASES)):
        for case in cases:
            for fam in FAMILIES:
                run(case, fam)
