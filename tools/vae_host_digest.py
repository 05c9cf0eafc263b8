"""SHA-256 of the raw output bytes of the VAE entry points, one line per call: evidence that a change of the VAE's host code (csrc/vae.hip below
`host side`, lfm_amd/autoencoder.py) keeps every result bit and every reported slab count (profiles/vae_host_refactor.txt).  Run it once per
library, each time in a fresh process, and compare the two outputs:
    python tools/vae_host_digest.py > new.txt;  LFM_HIP_LIBRARY=/path/to/parent/liblfm_hip.so python tools/vae_host_digest.py > parent.txt
Seeded weights and inputs; every workspace handed over is filled with 0xFF bytes (NaN in both precisions).  The stage entry points run under the
automatic kernel choice and again under flag CONV_HALO_SMALL (the halo-tiled convolution at any size: the statistics hand-over of a decode).
Not a test: a digest pins the compiler."""
import ctypes as C
import hashlib
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
from lfm_amd import hip  # noqa: E402
from lfm_amd.autoencoder import AutoencoderKL  # noqa: E402

dev = torch.device("cuda:0")
g = torch.Generator().manual_seed(1234)
L = hip.lib()


def sha(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.contiguous().cpu().view(torch.uint8).numpy().tobytes()).hexdigest()


def randn(*shape, dtype=torch.float32, scale=1.0):
    return (torch.randn(*shape, generator=g) * scale).to(dtype).to(dev)


def nan_bytes(n):
    return torch.full((n,), 255, dtype=torch.uint8, device=dev)


def show(what, t, **ints):
    print(what, sha(t), " ".join(f"{k}={v}" for k, v in ints.items()), flush=True)


# ---- whole decode / encode
vae = AutoencoderKL.from_random(0, with_encoder=True, decode_chunk=2).to(dev)
show("decode N=3 R=8 chunk=2", vae.decode(randn(3, 4, 8, 8)).sample)
show("encode N=3 S=64 chunk=2", vae.encode(randn(3, 3, 64, 64).clamp(-1, 1)).latent_dist.parameters)
vae.decode_chunk = None
show("decode N=1 R=32", vae.decode(randn(1, 4, 32, 32)).sample)


# ---- stage entry points
def resnet_params(cin, cout):
    p = {"n1_g": 1 + 0.1 * torch.randn(cin, generator=g), "n1_b": 0.1 * torch.randn(cin, generator=g),
         "c1_w": (torch.randn(cout, 9 * cin, generator=g) / (9 * cin) ** 0.5).half(), "c1_b": 0.02 * torch.randn(cout, generator=g),
         "n2_g": 1 + 0.1 * torch.randn(cout, generator=g), "n2_b": 0.1 * torch.randn(cout, generator=g),
         "c2_w": (torch.randn(cout, 9 * cout, generator=g) / (9 * cout) ** 0.5).half(), "c2_b": 0.02 * torch.randn(cout, generator=g)}
    if cin != cout:
        p["sc_w"], p["sc_b"] = (torch.randn(cout, cin, generator=g) / cin ** 0.5).half(), 0.02 * torch.randn(cout, generator=g)
    return {k: v.to(dev) for k, v in p.items()}


widths, n, H = [(512, 512), (512, 256)], 2, 16
params = [resnet_params(*w) for w in widths]
arr = (hip.VaeResnet * len(widths))()
for r, p, (cin, cout) in zip(arr, params, widths):
    for k, v in p.items():
        setattr(r, k, v.data_ptr())
    r.cin, r.cout = cin, cout
x = randn(n, H * H, 512, dtype=torch.float16)
for flags in (0, hip.DBG_CONV_HALO_SMALL):
    hip.gemm_select(flags << 4)
    for chain in (0, 1):
        out, slabs = torch.zeros(n, H * H, 256, dtype=torch.float16, device=dev), C.c_int(-1)
        ws = nan_bytes(L.lfm_vae_resnets_workspace_bytes(n, H, H))
        hip.check(L.lfm_vae_resnets_f16(arr, 2, hip.ptr(x), hip.ptr(out), hip.ptr(ws), ws.numel(), n, H, H, chain, C.byref(slabs), hip.stream_ptr()),
                  "lfm_vae_resnets_f16")
        show(f"resnets 512->512->256 n=2 16x16 flags={flags} chain_stats={chain}", out, last_slabs=slabs.value)
hip.gemm_select(0)

n, T = 2, 64
x = randn(n, T, 512, dtype=torch.float16)
att = [1 + 0.1 * torch.randn(512, generator=g), 0.1 * torch.randn(512, generator=g)]
for _ in range(4):
    att += [(torch.randn(512, 512, generator=g) / 512 ** 0.5).half(), 0.02 * torch.randn(512, generator=g)]
att = [t.to(dev) for t in att]
out, ws = torch.zeros_like(x), nan_bytes(L.lfm_vae_mid_attention_workspace_bytes(n, T))
hip.check(L.lfm_vae_mid_attention_f16(hip.ptr(x), hip.ptr(out), *[hip.ptr(t) for t in att], hip.ptr(ws), ws.numel(), n, T, hip.stream_ptr()),
          "lfm_vae_mid_attention_f16")
show("mid_attention n=2 T=64", out)

n, HW, Cc = 1, 4096, 128  # the workspace of tests/test_gpu_groupnorm.py: vae_gn_workspace
x, gamma, beta = randn(n, HW, Cc, dtype=torch.float16), randn(Cc), randn(Cc)
out, ws = torch.zeros_like(x), nan_bytes(256 + (n * 256 + 255) // 256 * 256 + n * max(HW * 256 // 512, 64 * 128) * 8)
hip.check(L.lfm_vae_groupnorm_f16(hip.ptr(x), hip.ptr(out), hip.ptr(gamma), hip.ptr(beta), hip.ptr(ws), ws.numel(), n, HW, Cc, 1, hip.stream_ptr()),
          "lfm_vae_groupnorm_f16")
show("groupnorm n=1 HW=4096 C=128", out)

n, H, Cc = 2, 16, 256
x, w, bias = randn(n, H * H, Cc, dtype=torch.float16), randn(Cc, 9 * Cc, dtype=torch.float16, scale=(9 * Cc) ** -0.5), randn(Cc, scale=0.1)
gamma, beta = randn(Cc), randn(Cc)
for flags in (0, hip.DBG_CONV_HALO_SMALL):
    hip.gemm_select(flags << 4)
    co, y, slabs, kern = torch.zeros_like(x), torch.zeros_like(x), C.c_int(-1), C.c_int(-1)
    ws = nan_bytes(256 + (n * 256 + 255) // 256 * 256 + n * max(2 * (H * H // 256) * Cc // 4, 64 * Cc // 4) * 8)
    hip.check(L.lfm_vae_conv3x3_gn_f16(hip.ptr(x), hip.ptr(w), hip.ptr(bias), None, hip.ptr(co), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(ws),
                                       ws.numel(), n, H, H, Cc, Cc, 0, 1, C.byref(slabs), C.byref(kern), hip.stream_ptr()), "lfm_vae_conv3x3_gn_f16")
    show(f"conv3x3_gn n=2 16x16 256->256 flags={flags} conv", co)
    show(f"conv3x3_gn n=2 16x16 256->256 flags={flags} gn", y, stat_slabs=slabs.value, stat_kernel=kern.value)
hip.gemm_select(0)
