"""One evaluation of the layout UNet (UNetModelAttn) and the share of its three own kernels, same process, no profiler.  Informational: no threshold.

    python tools/layout_unet_time.py [windows]

Model: nf = 128, channel_mult (1, 2, 3, 4), two ResBlocks per level, SpatialTransformers of depth 3 at 16x16 and 8x8 (4 heads), context [16, 77, 512], 32x32
latents, batch 16, seeded weights.  Timed: `windows` (default 5) windows of >= 0.3 s of back-to-back evaluations between two device events, after a warm-up
(the context projection is cached after the first evaluation, as in a solve).  Share of the new kernels: every call of lfm_cross_attention_f16 /
lfm_layernorm_f16 / lfm_geglu_f16 of ONE evaluation is recorded with its operands, then each recorded call is replayed alone, back to back, between two
events, and the sums are set against the evaluation's median time.  At small shapes such a replay loop runs at the host's launch rate, so the shares are
upper bounds of the kernels' device time; a kernel trace is the source for the durations themselves."""
import statistics
import sys

import torch

sys.path.insert(0, ".")
sys.path.insert(0, "tests")
import layout_cases as lc  # noqa: E402
from lfm_amd import hip  # noqa: E402
from lfm_amd.models.unet import UNetModelAttn  # noqa: E402

dev = torch.device("cuda:0")
windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WINDOW_S, N, L = 0.3, 16, 77

m = UNetModelAttn(image_size=32, in_channels=4, model_channels=128, out_channels=4, num_res_blocks=2, attention_resolutions=(2, 4), channel_mult=(1, 2, 3, 4),
                  num_heads=4, use_scale_shift_norm=True, use_spatial_transformer=True, transformer_depth=3, context_dim=512)
lc.load_seeded(m)
m = m.to(dev).eval()
g = torch.Generator().manual_seed(0)
x, ctx, t = torch.randn(N, 4, 32, 32, generator=g).to(dev), torch.randn(N, L, 512, generator=g).to(dev), torch.tensor(0.5, device=dev)


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def evaluate():
    return m(t, x, ctx)


# ---- the calls of the three kernels in one evaluation
recorded, real = [], {name: getattr(hip, name) for name in ("cross_attention", "layernorm", "geglu")}


def recorder(name):
    def call(*a, **k):
        recorded.append((name, a, k))
        return real[name](*a, **k)
    return call


evaluate()  # packs, projects the context
for name in real:
    setattr(hip, name, recorder(name))
evaluate()
for name, fn in real.items():
    setattr(hip, name, fn)
torch.cuda.synchronize()

print(f"sustained clock under matrix load (lfm_clock_probe): {hip.effective_clock_mhz(dev):.0f} MHz")
timed(evaluate, 5)
count = max(5, int(WINDOW_S / timed(evaluate, 10)) + 1)
evals = [timed(evaluate, count) for _ in range(windows)]
ev = statistics.median(evals)
print(f"evaluation nf 128, 32x32, batch {N}, L {L}: {count} per window; ms " + " ".join(f"{v * 1e3:.3f}" for v in evals) +
      f"; median {ev * 1e3:.3f}, spread {(max(evals) - min(evals)) / ev * 100:.1f} %")
total = 0.0
for name in real:
    calls = [(a, k) for n_, a, k in recorded if n_ == name]
    out = {}
    for a, k in calls:  # replay with an output buffer of its own: the evaluation's tensors are kept alive by `recorded`
        key = tuple(tuple(v.shape) if torch.is_tensor(v) else v for v in a)
        if key not in out:
            fn = lambda a=a, k=k: real[name](*a, **k)  # noqa: E731
            timed(fn, 20)
            out[key] = [timed(fn, 200), 0]
        out[key][1] += 1
    s = sum(tm * c for tm, c in out.values())
    total += s
    print(f"  {name:16s} {len(calls):3d} calls, {len(out)} shapes: {s * 1e6:8.1f} us in the replay loop (host launch rate at small shapes: an upper bound of device time; <= {s / ev * 100:5.2f} % of the evaluation)")
print(f"  the three kernels together: {total * 1e6:.1f} us in the replay loops (<= {total / ev * 100:.2f} % of the evaluation)")
