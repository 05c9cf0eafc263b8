"""UNet attention alone: the streamed kernel (csrc/unet_attention_stream_kernel.h) against the resident MFMA kernel (csrc/unet_attention_kernel.h), same process, no profiler.

    python tools/unet_attention_bench.py [windows]

Five configurations (N, heads, ch, T): the streamed kernel at (64, 4, 64, 1024); the resident kernel at (64, 4, 64, 256) and (64, 4, 128, 256); the two
resident shapes on the streamed kernel (LFM_OPT_UNET_ATTENTION_STREAM = 2).  Every configuration is warmed, then the configurations ALTERNATE: `windows`
(default 5) rounds, in each one window per configuration of >= 0.3 s of back-to-back launches between two device events.  Reported per configuration:
TFLOP/s (4 T^2 ch heads N FLOP per launch) of every window, the median and the spread (max - min) / median; the clock the box sustains under matrix load
(lfm_clock_probe); and the condition the streamed kernel was built to: its rate at T = 1024 x ch 64 >= 0.9 x the resident kernel's at T = 256 x ch 64."""
import os
import statistics
import sys

import torch

sys.path.insert(0, ".")
from lfm_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
windows = int(sys.argv[1]) if len(sys.argv) > 1 else 5
WINDOW_S = 0.3
CONFIGS = [  # name, (N, heads, ch, T), LFM_OPT_UNET_ATTENTION_STREAM, the kernel the plan must name
    ("streamed 1024x64", (64, 4, 64, 1024), 1, 3),
    ("resident 256x64", (64, 4, 64, 256), 1, 2),
    ("resident 256x128", (64, 4, 128, 256), 1, 2),
    ("streamed 256x64", (64, 4, 64, 256), 2, 3),
    ("streamed 256x128", (64, 4, 128, 256), 2, 3),
]
L = hip.lib()
g = torch.Generator().manual_seed(0)
bufs = {}
for _, shape, _, _ in CONFIGS:
    if shape not in bufs:
        N, heads, ch, T = shape
        qkv = (torch.randn(N * T, 3 * heads * ch, generator=g) * 1.6).half().to(dev)
        bufs[shape] = (qkv, torch.empty(N * T, heads * ch, dtype=torch.float16, device=dev))


def launch(shape, n):
    N, heads, ch, T = shape
    qkv, out = bufs[shape]
    st = hip.stream_ptr(dev)
    for _ in range(n):
        hip.check(L.lfm_attention_small_f16(hip.ptr(qkv), hip.ptr(out), N, T, heads, ch, st), "lfm_attention_small_f16")


def timed(shape, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    launch(shape, n)
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3


print(f"library {os.environ.get('LFM_HIP_LIBRARY') or os.path.relpath(hip.LIB_PATH)}")
print(f"sustained clock under matrix load (lfm_clock_probe): {hip.effective_clock_mhz(dev):.0f} MHz")
counts = {}
try:
    for name, shape, opt, kern in CONFIGS:  # warm-up and the launch count of a window
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, opt)
        assert hip.unet_attention_plan(shape[0], shape[3], shape[1], shape[2]) == kern, name
        timed(shape, 20)
        counts[name] = max(20, int(WINDOW_S / (timed(shape, 50) / 50)) + 1)
    rates = {name: [] for name, *_ in CONFIGS}
    for _ in range(windows):
        for name, shape, opt, _ in CONFIGS:
            hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, opt)
            N, heads, ch, T = shape
            s = timed(shape, counts[name])
            rates[name].append(4.0 * T * T * ch * heads * N * counts[name] / s / 1e12)
finally:
    hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 1)
med = {}
for name, shape, _, _ in CONFIGS:
    r = rates[name]
    med[name] = statistics.median(r)
    N, heads, ch, T = shape
    us = 4.0 * T * T * ch * heads * N / med[name] / 1e6
    print(f"{name:18s} N {N} heads {heads} ch {ch} T {T}: {counts[name]} launches / window; TFLOP/s " + " ".join(f"{v:.1f}" for v in r) +
          f"; median {med[name]:.1f} ({us:.1f} us / launch), spread {(max(r) - min(r)) / med[name] * 100:.1f} %")
ratio = med["streamed 1024x64"] / med["resident 256x64"]
print(f"condition: streamed 1024x64 / resident 256x64 = {ratio:.3f} (>= 0.9 asked): {'MET' if ratio >= 0.9 else 'MISSED'}")
print(f"same shape, streamed / resident: 256x64 {med['streamed 256x64'] / med['resident 256x64']:.3f}, 256x128 {med['streamed 256x128'] / med['resident 256x128']:.3f}")
