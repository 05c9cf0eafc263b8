"""The tiled any-T attention kernel (csrc/attention_tiled_kernel.h) at 64 images x 16 heads x 576 tokens, hd 64 (DiT-L/2 at --image_size 384), and -- under
LFM_OPT_ATTENTION_TILED = 2 -- at 1024 and 256 tokens against the kernels that own those shapes (four key chunks; the streamed kernel).  Interleaved rounds in
ONE process on random operands; median and min per variant.  Also says whether the two kernels' results are bit-equal.  Notes: profiles/dit_attention_tiled.txt.
usage: python tools/attn_tiled_time.py [rounds]"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from lfm_amd import hip  # noqa: E402

dev = torch.device("cuda:0")
ROUNDS = int(sys.argv[1]) if len(sys.argv) > 1 else 7


def timeit(fn, n=20, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / n * 1e3


def operands(batch, heads, T, hd):
    g = torch.Generator(device=dev).manual_seed(T + hd)
    Q = (torch.randn(batch * T, heads * hd, device=dev, generator=g) * 1.5).half()
    K = (torch.randn(batch * T, heads * hd, device=dev, generator=g) * 1.5).half()
    Vt = torch.randn(batch, heads, hd, T, device=dev, generator=g).half()
    return Q, K, Vt


def report(name, ts, flops):
    med = statistics.median(ts)
    print(f"  {name:<28} median {med:8.1f} us   min {min(ts):8.1f} us   {flops / med / 1e6:6.0f} TFLOP/s", flush=True)


for batch, heads, T, hd in ((64, 16, 576, 64), (64, 16, 1024, 64), (64, 16, 256, 64), (64, 16, 576, 72), (64, 16, 256, 72)):
    Q, K, Vt = operands(batch, heads, T, hd)
    flops = 4.0 * batch * heads * T * T * hd
    own = hip.attention_plan(batch, heads, hd, T)
    print(f"{batch} images x {heads} heads x {T} tokens x hd {hd}  (default kernel: {own})", flush=True)
    run = lambda: hip.dit_attention(Q, K, Vt, batch, heads, T, hd)
    times = {"tiled": [], "owner": []}
    outs = {}
    for _ in range(ROUNDS):
        for which in ("tiled", "owner"):
            if which == "owner" and own == 7:
                continue
            hip.set_option(hip.OPT_ATTENTION_TILED, 2 if which == "tiled" else 1)
            assert hip.attention_plan(batch, heads, hd, T) == (7 if which == "tiled" else own)
            times[which].append(timeit(run))
            outs[which] = run()
    hip.set_option(hip.OPT_ATTENTION_TILED, 1)
    report("tiled kernel (7)", times["tiled"], flops)
    if times["owner"]:
        report(f"owning kernel ({own})", times["owner"], flops)
        torch.cuda.synchronize()
        print(f"  results bit-equal: {torch.equal(outs['tiled'], outs['owner'])}", flush=True)
