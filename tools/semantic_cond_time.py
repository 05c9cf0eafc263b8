"""Time the conditioning stage of mask-to-image synthesis (lfm_amd/downstream_tasks/flow_latent_semantic_syn.py) on the GPU: the fused gather
(``SpatialRescaler.encode_labels`` -> lfm_label_rescale_f32) against the one-hot path (F.one_hot -> three bilinear x0.5 passes -> the split-fp16 GEMM channel
mapper) at the reference's settings: 256 x 256 label maps, batch 50 and 200, 19 / 151 / 182 classes.

    python -m tools.semantic_cond_time [--out FILE] [--batches 50 200] [--classes 19 151 182]

Per setting: time per call (HIP events around `iters` calls after a warm-up, the device drained before and after), peak allocated memory above what the inputs
hold, the largest difference between the two latents, and the kernel's label bytes per second (N * 256 * 256 * 8 bytes over the fused time; the call is one
launch; the calls cycle through copies of the label maps that together exceed the Infinity Cache, so the labels come from HBM).  bench.py does not time this
stage."""
import argparse
import sys

import torch


COLD_BYTES = 640 << 20  # label maps cycled through per setting: 2.5 x the 256 MB Infinity Cache


def timed(fn, iters):
    """fn(i): call number i; ms per call."""
    fn(0)
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters  # ms


def peak_above_inputs(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    return out, peak


def main(argv=None):
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import SpatialRescaler, synthetic_labels

    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--batches", nargs="+", type=int, default=[50, 200])
    p.add_argument("--classes", nargs="+", type=int, default=[19, 151, 182])
    p.add_argument("--size", type=int, default=256)
    args = p.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    lines = [f"conditioning stage at {args.size} x {args.size}, SpatialRescaler(n_stages=3, num_cls -> 4): fused gather vs one-hot path ({torch.cuda.get_device_name(0)})",
             f"{'batch':>5} {'cls':>4} | {'fused ms':>9} {'peak MB':>8} {'labels GB/s':>11} | {'one-hot ms':>10} {'peak MB':>9} | {'speed-up':>8} {'max |diff|':>10}"]
    for n in args.batches:
        for k in args.classes:
            torch.manual_seed(0)
            cs = SpatialRescaler(n_stages=3, in_channels=k, out_channels=4, multiplier=0.5).to(dev).eval()
            seg = synthetic_labels(n, args.size, k, seed=1).to(dev)
            fused = lambda: cs.encode_labels(seg, k)  # noqa: E731
            onehot = lambda: cs(torch.nn.functional.one_hot(seg, k).permute(0, 3, 1, 2).float())  # noqa: E731
            a, peak_f = peak_above_inputs(fused)
            copies = [seg] + [seg.clone() for _ in range(-(-COLD_BYTES // (seg.numel() * 8)) - 1)]  # together beyond the Infinity Cache: every call reads HBM
            t_f = timed(lambda i: cs.encode_labels(copies[i % len(copies)], k), 5 * len(copies))
            del copies
            gbs = seg.numel() * 8 / (t_f * 1e-3) / 1e9
            try:
                b, peak_o = peak_above_inputs(onehot)
            except RuntimeError as e:  # out of device memory, or torch's own limits: bilinear interpolation refuses 2^31 elements and more (200 x 182 x 256 x 256)
                lines.append(f"{n:>5} {k:>4} | {t_f:>9.4f} {peak_f / 1e6:>8.2f} {gbs:>11.1f} | the one-hot path does not run: {str(e).splitlines()[0][:150]}")
                print(lines[-1], flush=True)
                continue
            diff = float((a - b).abs().max())
            del a, b
            t_o = timed(lambda i: onehot(), 3)
            lines.append(f"{n:>5} {k:>4} | {t_f:>9.4f} {peak_f / 1e6:>8.2f} {gbs:>11.1f} | {t_o:>10.2f} {peak_o / 1e6:>9.1f} | {t_o / t_f:>8.0f} {diff:>10.2e}")
            print(lines[-1], flush=True)
    text = "\n".join(lines) + "\n"
    print(text)
    if args.out:
        open(args.out, "w").write(text)


if __name__ == "__main__":
    sys.exit(main())
