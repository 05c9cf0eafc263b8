"""SHA-256 of the raw output bytes of every epilogue hand-over path, one line per case: evidence that a refactor of csrc/epilogue_handover.h /
gemm_epilogues.h keeps every result bit (profiles/epilogue_handover_refactor.txt).  Run it once per library and compare the two outputs:
    python tools/epilogue_digest.py > new.txt;  LFM_HIP_LIBRARY=/path/to/parent/liblfm_hip.so python tools/epilogue_digest.py > parent.txt
Cases (those of tests/test_gpu_dit.py and test_gpu_vae.py, same seeds): the (M, N, K) x epilogue 0-3 list of test_gemm256_kernels and the five shapes of
test_gemm_qkv_split with kernels 1, 4, 5, 6, each with and without GEMM_STORE8; the two folded-LayerNorm models at kernels 0 and 6 (output and the
whole, pre-zeroed workspace); one VAE decode (4 x 16 x 16 latents) on the halo kernel and on the implicit GEMM through kernels 4 and 5 (image and the
pre-zeroed workspace, GroupNorm partial sums included).  Not a test: a digest pins the compiler."""
import hashlib
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from lfm_amd import hip  # noqa: E402
from oracle import dit_ref, vae_ref  # noqa: E402

dev = torch.device("cuda:0")


def sha(*tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


def gemm_case(M, N, K, epi):  # tests/test_gpu_dit.py: _gemm_case
    g = torch.Generator().manual_seed(M + N * 3 + K + epi)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias = torch.randn(N, generator=g) * 0.1
    X = gate = None
    if epi == 3:
        X = torch.randn(M, N, generator=g)
        gate = torch.randn(M // 4, N, generator=g)
    return A, W, bias, X, gate


S8 = hip.DBG_GEMM_STORE8 << 4
KERNELS = [1, 1 | S8, 4, 4 | S8, 5, 5 | S8, 6, 6 | S8]
SHAPES = [(512, 512, 128), (1024, 768, 1024), (300, 260, 64), (4096, 1024, 4096), (8192, 3072, 1024), (512, 256, 192), (256, 512, 320), (768, 512, 576),
          (512, 128, 96), (384, 132, 160), (256, 128, 32), (65536, 128, 1152)]


def gemms():
    for M, N, K in SHAPES:
        for epi in range(4):
            A, W, bias, X, gate = gemm_case(M, N, K, epi)
            Ad, Wd, bd, gd = A.to(dev), W.to(dev), bias.to(dev), (gate.to(dev) if gate is not None else None)
            for k in KERNELS:
                if ((k & 15) != 4 and M > 8192 and N == 128) or ((k & 15) != 4 and K % 64):
                    continue  # the skips of the test: the narrow-N shape and the 32-deep K tails are the 256x128 kernel's
                hip.gemm_select(k)
                try:
                    out = hip.gemm_f16(Ad, Wd, bd, epilogue=epi, out=X.clone().to(dev) if epi == 3 else None, gate=gd, gate_stride=N, tokens=4)
                    torch.cuda.synchronize()
                finally:
                    hip.gemm_select(0)
                print(f"DIGEST gemm {M}x{N}x{K} epi{epi} k{k & 15}{'+store8' if k & S8 else ''} {sha(out)}", flush=True)


def qkvs():
    for batch, tokens, D, hd in [(3, 256, 384, 64), (8, 64, 512, 64), (2, 256, 1024, 64), (2, 256, 1152, 72), (3, 64, 576, 72)]:
        g = torch.Generator().manual_seed(batch + tokens + D)  # tests/test_gpu_dit.py: _qkv_case
        M = batch * tokens
        A = (torch.randn(M, D, generator=g) * 0.5).half().to(dev)
        W = (torch.randn(3 * D, D, generator=g) / D ** 0.5).half().to(dev)
        bias = (torch.randn(3 * D, generator=g) * 0.1).to(dev)
        for k in KERNELS:
            hip.gemm_select(k)
            try:
                Q, K, Vt = hip.gemm_qkv_f16(A, W, bias, hd, tokens)
                torch.cuda.synchronize()
            finally:
                hip.gemm_select(0)
            print(f"DIGEST qkv b{batch} t{tokens} D{D} hd{hd} k{k & 15}{'+store8' if k & S8 else ''} {sha(Q, K, Vt)}", flush=True)


def folded():
    from lfm_amd.models import DiT_models

    for name, batch, labels in [("DiT-L/2", 48, False), ("DiT-B/2", 64, True)]:
        kw = dict(num_classes=1000, label_dropout=0.1) if labels else dict(num_classes=1, label_dropout=0.0)
        sd = dit_ref.make_dit_state(dit_ref.DiTCfg.named(name, **kw), seed=6)
        m = DiT_models[name](img_resolution=32, in_channels=4, **kw)
        m.load_state_dict(sd, strict=True)
        m = m.to(dev).eval()
        g = torch.Generator().manual_seed(1)
        x = torch.randn(batch, 4, 32, 32, generator=g).to(dev)
        y = torch.randint(0, 1001, (batch,), generator=g).to(dev) if labels else None
        t = (torch.linspace(0.05, 0.95, batch) if labels else torch.tensor(0.6)).to(dev)
        for k in (0, 6):
            hip.gemm_select(k)
            try:
                m(t, x, y)  # allocates the workspace
                m._ws[1].zero_()
                out = m(t, x, y).clone()
                torch.cuda.synchronize()
            finally:
                hip.gemm_select(0)
            print(f"DIGEST folded {name} batch{batch} k{k} out {sha(out)} workspace {sha(m._ws[1])}", flush=True)


def vae():
    from lfm_amd.autoencoder import AutoencoderKL

    sd = vae_ref.make_vae_state(seed=3)
    v = AutoencoderKL()
    v.load_state_dict(sd, strict=True)
    v = v.to(dev)
    z = (torch.randn(4, 4, 16, 16, generator=torch.Generator().manual_seed(4 + 16)) * 1.5).to(dev)
    for tag, sel in [("halo", 0), ("implicit k4", 4 | (hip.DBG_CONV_IMPLICIT_GEMM << 4)), ("implicit k5", 5 | (hip.DBG_CONV_IMPLICIT_GEMM << 4))]:
        hip.gemm_select(sel)
        try:
            v.decode(z)
            v._ws.zero_()
            out = v.decode(z).sample.clone()
            torch.cuda.synchronize()
        finally:
            hip.gemm_select(0)
        print(f"DIGEST vae decode 4x16x16 {tag} out {sha(out)} workspace {sha(v._ws)}", flush=True)


if __name__ == "__main__":
    print(f"library {os.environ.get('LFM_HIP_LIBRARY') or hip.LIB_PATH}", flush=True)
    what = sys.argv[1:] or ["gemm", "qkv", "folded", "vae"]
    for w in what:
        {"gemm": gemms, "qkv": qkvs, "folded": folded, "vae": vae}[w]()
