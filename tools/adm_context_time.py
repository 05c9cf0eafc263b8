"""One evaluation of ``adm`` and of ``adm_context`` at the imnet_adm configuration (oracle/edm_state.py: nf 256, ch_mult 1 2 3 4, attention at 16 / 8 / 4, two
blocks per level, 32x32 latents, 1000 classes, label_dropout 0.1), batch 64, same process, no profiler.  Informational: no threshold.

    python tools/adm_context_time.py [windows]      # on the GPU: both times and their ratio next to the FLOP ratio
    python tools/adm_context_time.py --flops        # on the CPU, where the reference checkout exists (LFM_REFERENCE): recount FLOPS_PER_IMAGE

Timed: `windows` (default 5) windows of >= 0.3 s of back-to-back evaluations between two device events, after a warm-up, per-sample times and labels.
FLOPs per image: 2 x MACs of every convolution / linear, forward hooks on the REFERENCE's own layer classes as oracle/make_golden.py::golden_edm_full counts
them, plus the two attention einsums of every attention (4 T Tk C; Tk = T for self-attention, 1 for attn2).  The reference is not on the GPU machine, so the
counts are kept below and `--flops` recounts and compares them.  The count is the REFERENCE's work: the product skips attn2's q projection, k projection and
softmax (the one-key identity) -- `skipped` is their share."""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")

FLOPS_PER_IMAGE = {"adm": 73055813632.0, "adm_context": 85608169472.0, "skipped": 1279590400.0}  # recounted by --flops; "adm" is tests/golden/edm_full.pt's figure
N, WINDOW_S = 64, 0.3


def config(context):
    from oracle.edm_state import EDM_CONFIGS

    return dict(EDM_CONFIGS["imnet_adm"], use_context=context)


def count_flops():
    from oracle.make_golden import _import_reference

    _import_reference()
    import models.EDM as ref_edm

    out = {}
    for name, context in (("adm", False), ("adm_context", True)):
        with torch.device("meta"):
            m = ref_edm.DhariwalUNet(**config(context)).eval()
        flops, skipped = [0.0], [0.0]

        def conv_hook(mod, inp, outp):
            if mod.weight is not None:
                flops[0] += 2.0 * outp[0].numel() * mod.weight[0].numel()

        def lin_hook(mod, inp, outp):
            flops[0] += 2.0 * (outp.numel() // outp.shape[0]) * mod.weight.shape[1]

        def blk_hook(mod, inp, outp):
            if mod.num_heads:
                flops[0] += 4.0 * (outp.shape[2] * outp.shape[3]) ** 2 * outp.shape[1]

        def attn_hook(mod, args, kwargs, outp):
            ctx = kwargs.get("context", args[1] if len(args) > 1 else None)
            C, T = outp.shape[1], outp.shape[2] * outp.shape[3]
            Tk = T if ctx is None else ctx.shape[2] * ctx.shape[3]
            flops[0] += 4.0 * T * Tk * C
            if ctx is not None:  # attn2: what the one-key identity skips -- q on every pixel, k on the key, the two einsums
                skipped[0] += 2.0 * T * C * C + 2.0 * Tk * C * ctx.shape[1] + 4.0 * T * Tk * C

        for mod in m.modules():
            if isinstance(mod, ref_edm.Conv2d):
                mod.register_forward_hook(conv_hook)
            elif isinstance(mod, ref_edm.Linear):
                mod.register_forward_hook(lin_hook)
            elif isinstance(mod, ref_edm.CrossAttention):
                mod.register_forward_hook(attn_hook, with_kwargs=True)
            elif isinstance(mod, ref_edm.UNetBlock):
                mod.register_forward_hook(blk_hook)
        with torch.no_grad(), torch.device("meta"):
            m(torch.zeros(()), torch.zeros(1, 4, 32, 32), torch.zeros(1, dtype=torch.long))
        out[name] = flops[0]
        if context:
            out["skipped"] = skipped[0]
        print(f"{name}: {sum(p.numel() for p in m.parameters()) / 1e6:.1f} M parameters, {flops[0] / 1e9:.3f} GFLOP per image", flush=True)
    print("FLOPS_PER_IMAGE =", out, "" if out == FLOPS_PER_IMAGE else "   <- differs from the table in this file")
    print(f"adm_context / adm = {out['adm_context'] / out['adm']:.4f}; attn2's skipped share of adm_context: {out['skipped'] / out['adm_context'] * 100:.2f} %")
    return out


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def time_models(windows):
    import adm_context_cases as ac
    from lfm_amd import hip
    from lfm_amd.models.EDM import DhariwalUNet
    from oracle.edm_state import load_seeded

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    x, y, t = torch.randn(N, 4, 32, 32, generator=g).to(dev), torch.randint(0, 1000, (N,), generator=g).to(dev), torch.rand(N, generator=g).to(dev)
    print(f"sustained clock under matrix load (lfm_clock_probe): {hip.effective_clock_mhz(dev):.0f} MHz")
    med = {}
    for name, context in (("adm", False), ("adm_context", True)):
        m = DhariwalUNet(**config(context))
        (ac.load_seeded if context else lambda mod: load_seeded(mod, 64))(m)
        m = m.to(dev).eval()
        fn = lambda: m(t, x, y)  # noqa: E731
        timed(fn, 3)
        count = max(3, int(WINDOW_S / timed(fn, 5)) + 1)
        evals = [timed(fn, count) for _ in range(windows)]
        med[name] = statistics.median(evals)
        fl = FLOPS_PER_IMAGE[name] * N
        print(f"{name:12s} imnet_adm configuration, batch {N}: {count} per window; ms " + " ".join(f"{v * 1e3:.2f}" for v in evals) +
              f"; median {med[name] * 1e3:.2f} ms, spread {(max(evals) - min(evals)) / med[name] * 100:.1f} %; {N / med[name]:.0f} evaluations of one image / s; "
              f"{fl / med[name] / 1e12:.1f} TFLOP/s of the reference's count")
        del m, fn
        torch.cuda.empty_cache()
    fr = FLOPS_PER_IMAGE["adm_context"] / FLOPS_PER_IMAGE["adm"]
    tr = med["adm_context"] / med["adm"]
    print(f"time ratio adm_context / adm = {tr:.3f}; FLOP ratio (reference's count) = {fr:.3f}; time per FLOP relative to adm = {tr / fr:.3f}")


if __name__ == "__main__":
    if "--flops" in sys.argv:
        count_flops()
    else:
        time_models(int(sys.argv[1]) if len(sys.argv) > 1 else 5)
