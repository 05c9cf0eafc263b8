"""Time the elementwise work around VAE encode, solve and decode of an inpainting batch (lfm_amd/downstream_tasks/flow_latent_inpainting.py) on the GPU: the three
kernels of the "fused" path (lfm_inpaint_prepare_u8, lfm_inpaint_cond_f32, lfm_inpaint_composite_u8) against the "torch" path's op chain for the same three
stages (the reference's arithmetic as torch ops on the device), in one process, at the reference's batch: 50 x 256 x 256.

    python -m tools.inpaint_prep_time [--out FILE] [--batch 50] [--size 256] [--windows 5]

Per stage: device time per call (HIP events around a window of calls after a warm-up, the device drained before and after; the windows of the two paths
alternate and the median window is reported with the spread), the bytes the kernel has to move (computed from the shapes below), and those bytes over the
time as a fraction of the HBM bandwidth (8.0 TB/s spec; a float4 copy reaches 6.29).  The calls cycle through copies of their tensors that together exceed the
256 MB Infinity Cache, so inputs come from HBM and outputs go there.  Host-to-device bytes per batch are counted from the tensors each path uploads.  The
random draws (eps, z_0), the VAE and the solve are the same on both paths and not timed here; bench.py does not time this stage."""
import argparse
import statistics
import sys

import torch

COLD_BYTES = 640 << 20  # per stage, the tensors cycled through: 2.5 x the Infinity Cache
HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12


def window(fn, iters):
    """ms per call over `iters` calls of fn(i)."""
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for i in range(iters):
        fn(i)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main(argv=None):
    from lfm_amd import hip
    from lfm_amd.autoencoder import DiagonalGaussianDistribution
    from lfm_amd.downstream_tasks.flow_latent_inpainting import dataset_tensors, synthetic_pairs
    from lfm_amd.io_formats import to_uint8_rounding_device

    p = argparse.ArgumentParser()
    p.add_argument("--out", default=None)
    p.add_argument("--batch", type=int, default=50)
    p.add_argument("--size", type=int, default=256)
    p.add_argument("--windows", type=int, default=5)
    a = p.parse_args(argv)
    assert torch.cuda.is_available(), "this measurement needs the GPU"
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    N, S, R, scale = a.batch, a.size, a.size // 8, 0.18215
    px = N * S * S
    img, mask = (t.to(dev) for t in synthetic_pairs(N, S, seed=1))
    g = torch.Generator(device=dev).manual_seed(0)
    # bytes per call: what the stage must read and write once
    bytes_prepare = px * (3 + 1) + px * 3 * 4 + N * R * R * 4
    bytes_cond = N * R * R * (8 + 4 + 4) * 4
    bytes_comp = px * 3 * 4 + px * (3 + 1) + px * 3
    k = max(2, -(-COLD_BYTES // bytes_prepare))
    imgs, masks = [img.clone() for _ in range(k)], [mask.clone() for _ in range(k)]
    fakes = [torch.rand(N, 3, S, S, device=dev, generator=g) * 2.4 - 1.2 for _ in range(k)]
    kc = max(2, -(-COLD_BYTES // bytes_cond))
    moms = [torch.randn(N, 8, R, R, device=dev, generator=g) for _ in range(kc)]
    epss = [torch.randn(N, 4, R, R, device=dev, generator=g) for _ in range(kc)]
    conds = [torch.empty(N, 5, R, R, device=dev) for _ in range(kc)]
    maskeds = [torch.empty(N, 3, S, S, device=dev) for _ in range(k)]
    outs = [torch.empty(N, S, S, 3, dtype=torch.uint8, device=dev) for _ in range(k)]
    L, st = hip.lib(), hip.stream_ptr(dev)
    lat_off, stride = 4 * R * R * 4, 5 * R * R

    def f_prepare(i):  # the entry point itself on preallocated outputs: the kernel, not torch's allocator
        j = i % k
        hip.check(L.lfm_inpaint_prepare_u8(hip.ptr(imgs[j]), hip.ptr(masks[j]), hip.ptr(maskeds[j]), None, conds[i % kc].data_ptr() + lat_off, stride, N, S, S,
                                           st), "prepare")

    def f_cond(i):
        j = i % kc
        hip.check(L.lfm_inpaint_cond_f32(hip.ptr(moms[j]), hip.ptr(epss[j]), scale, hip.ptr(conds[j]), stride, N, R * R, st), "cond")

    def f_comp(i):
        j = i % k
        hip.check(L.lfm_inpaint_composite_u8(hip.ptr(fakes[j]), hip.ptr(imgs[j]), hip.ptr(masks[j]), hip.ptr(outs[j]), N, S, S, st), "composite")

    keep = {}

    def t_prepare(i):  # the dataset's tensors from the bytes and the mask on the latent grid (reference :42-53, :148)
        j = i % k
        image, m, masked = dataset_tensors(imgs[j], masks[j])
        keep["image"], keep["mask"] = image, m
        return masked, torch.nn.functional.interpolate(m, size=(R, R))

    def t_cond(i):  # .latent_dist.sample().mul_(scale_factor), the cat (:147, :150)
        j = i % kc
        d = DiagonalGaussianDistribution(moms[j])
        c = (d.mean + d.std * epss[j]).mul_(scale)
        return torch.cat((c, conds[j][:, 4:]), dim=1)

    def t_comp(i):  # three to_range_0_1, the composite, save_image's bytes (:157-160)
        j = i % k
        f, m, im = (fakes[j] + 1.0) / 2.0, (keep["mask"] + 1.0) / 2.0, (keep["image"] + 1.0) / 2.0
        return to_uint8_rounding_device(f * m + (1 - m) * im)

    # calls per window of the kernels (the torch chain gets a quarter of them): several hundred, each on another copy than the one before
    stages = [("prepare", f_prepare, t_prepare, bytes_prepare, 40 * k), ("cond", f_cond, t_cond, bytes_cond, 4 * kc), ("composite", f_comp, t_comp, bytes_comp, 40 * k)]
    lines = [f"inpainting, elementwise stages per batch of {N} x {S} x {S} ({torch.cuda.get_device_name(0)}); median of {a.windows} alternating windows, [min..max]",
             f"{'stage':>10} | {'kernel us':>22} {'MB moved':>9} {'TB/s':>6} {'of 8.0':>7} {'of 6.29':>8} | {'torch ops us':>24} | {'ratio':>6}"]
    total_f = total_t = 0.0
    for name, ff, ft, nbytes, iters in stages:
        ff(0), ft(0)  # warm-up: code objects, the allocator's blocks
        window(ff, iters), window(ft, max(2, iters // 4))
        wf, wt = [], []
        for _ in range(a.windows):
            wf.append(window(ff, iters) * 1e3)
            wt.append(window(ft, max(2, iters // 4)) * 1e3)
        mf, mt = statistics.median(wf), statistics.median(wt)
        total_f, total_t = total_f + mf, total_t + mt
        rate = nbytes / (mf * 1e-6)
        lines.append(f"{name:>10} | {mf:8.2f} [{min(wf):6.2f}..{max(wf):6.2f}] {nbytes / 1e6:9.2f} {rate / 1e12:6.2f} {rate / HBM_SPEC:7.1%} {rate / HBM_COPY:8.1%} | "
                     f"{mt:9.1f} [{min(wt):6.1f}..{max(wt):6.1f}] | {mt / mf:6.1f}")
        print(lines[-1], flush=True)
    lines.append(f"{'all three':>10} | {total_f:8.2f} us against {total_t:.1f} us of torch ops per batch ({total_t / total_f:.1f} x)")
    # the same bits?  prepare and composite of the two paths on one batch
    cond = torch.empty(N, 5, R, R, device=dev)
    masked, _ = hip.inpaint_prepare(imgs[0], masks[0], cond)
    tm, tcc = t_prepare(0)
    same = torch.equal(masked, tm) and torch.equal(cond[:, 4:], tcc) and torch.equal(hip.inpaint_composite(fakes[0], imgs[0], masks[0]), t_comp(0))
    lines.append(f"fused and torch outputs of prepare and composite on one batch bit-identical: {same}")
    h2d_f, h2d_t = px * 4, px * (3 + 1 + 3) * 4
    lines.append(f"host-to-device bytes per batch: fused {h2d_f / 1e6:.2f} MB (image and mask bytes, 4 per pixel); the reference's loop {h2d_t / 1e6:.2f} MB "
                 f"(img, mask, masked_img as fp32, 28 per pixel); --prep_path torch of this driver uploads the bytes too and builds the floats on the device")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        open(a.out, "w").write(text)


if __name__ == "__main__":
    sys.exit(main())
