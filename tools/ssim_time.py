"""Time the per-image SSIM of the inpainting evaluation on the GPU: one lfm_ssim_u8 call (csrc/ssim.h: the tile kernel and the reduce kernel, mask sums
included) against the reference's op chain for the same batch as torch ops on the device (lfm_amd.inpaint_eval.ssim_torch: five depthwise 11 x 11 convolutions
and the elementwise map, after the two byte / 255 conversions the evaluator's dataset does on the host, and the mask's mean), in one process.

    python -m tools.ssim_time [--out profiles/ssim.txt] [--batch 50] [--sizes 256 512] [--windows 5]

Per size: device time per call (HIP events around a window of calls after a warm-up, the device drained before and after; the windows of the two paths
alternate and the median window is reported with the spread), and the bytes the fused call has to move (7 per pixel in, 12 per image out).  The calls cycle
through copies of their inputs that together exceed the 256 MB Infinity Cache, so the bytes come from HBM.  bench.py does not time this stage."""
import argparse
import statistics
import sys

import torch

COLD_BYTES = 640 << 20  # the inputs cycled through: 2.5 x the Infinity Cache


def window(fn, iters):
    """us per call over `iters` calls of fn(i)."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def main(argv=None):
    from lfm_amd import hip
    from lfm_amd.inpaint_eval import SSIM, ssim_torch

    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--batch", type=int, default=50)
    p.add_argument("--sizes", type=int, nargs="+", default=[256, 512])
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    N = a.batch
    L, st = hip.lib(), hip.stream_ptr(dev)
    w1 = hip.ssim_gaussian(11).to(dev)
    w2 = SSIM(11).window(3, torch.zeros(1)).to(dev)
    d255 = torch.full((), 255.0, device=dev)
    lines = [f"per-image SSIM, window 11, batch of {N} ({torch.cuda.get_device_name(0)}); median of {a.windows} alternating windows, [min..max]",
             f"{'size':>9} | {'lfm_ssim_u8 us':>26} {'MB moved':>9} {'GB/s':>7} | {'torch ops us':>28} | {'ratio':>6}"]
    for S in a.sizes:
        g = torch.Generator(device=dev).manual_seed(S)
        nbytes = N * S * S * 7 + N * 12
        k = max(2, -(-COLD_BYTES // nbytes))
        gens = [torch.randint(0, 256, (N, S, S, 3), device=dev, dtype=torch.uint8, generator=g) for _ in range(k)]
        imgs = [torch.randint(0, 256, (N, S, S, 3), device=dev, dtype=torch.uint8, generator=g) for _ in range(k)]
        masks = [torch.randint(0, 256, (N, S, S), device=dev, dtype=torch.uint8, generator=g) for _ in range(k)]
        need = L.lfm_ssim_workspace_bytes(N, S, S)
        ws = torch.empty(need, dtype=torch.uint8, device=dev)
        out, msum = torch.empty(N, device=dev), torch.empty(N, dtype=torch.int64, device=dev)

        def fused(i):  # the entry point itself on preallocated outputs: the kernels, not torch's allocator
            j = i % k
            hip.check(L.lfm_ssim_u8(hip.ptr(gens[j]), hip.ptr(imgs[j]), hip.ptr(masks[j]), N, S, S, hip.ptr(w1), 11, hip.ptr(ws), need, hip.ptr(out), hip.ptr(msum), st),
                      "lfm_ssim_u8")

        def chain(i):
            j = i % k
            x = gens[j].permute(0, 3, 1, 2).to(torch.float32) / d255
            y = imgs[j].permute(0, 3, 1, 2).to(torch.float32) / d255
            area = (1 - masks[j].to(torch.float32) / d255).reshape(N, -1).mean(dim=-1)
            return ssim_torch(x, y, w2), area

        it_f, it_t = 4 * k, max(2, k // 2)
        fused(0), chain(0)  # warm-up: code objects, the allocator's blocks
        window(fused, it_f), window(chain, it_t)
        wf, wt = [], []
        for _ in range(a.windows):
            wf.append(window(fused, it_f))
            wt.append(window(chain, it_t))
        mf, mt = statistics.median(wf), statistics.median(wt)
        lines.append(f"{S:>4}x{S:<4} | {mf:9.2f} [{min(wf):7.2f}..{max(wf):7.2f}] {nbytes / 1e6:9.2f} {nbytes / (mf * 1e-6) / 1e9:7.1f} | "
                     f"{mt:10.1f} [{min(wt):8.1f}..{max(wt):8.1f}] | {mt / mf:6.1f}")
        print(lines[-1], flush=True)
        fused(0)
        ref, area = chain(0)
        diff = float((out.double() - ref.double()).abs().max())
        sums_ok = bool(((1 - msum.double() / (255.0 * S * S)) - area.double()).abs().max() < 1e-5)
        lines.append(f"          | fused against the torch chain on one batch: largest difference {diff:.2e}; mask sums agree with the chain's areas: {sums_ok}")
        del gens, imgs, masks
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    sys.exit(main())
