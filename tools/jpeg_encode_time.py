"""What writing the samples' JPEGs costs, on the device (hip.jpeg_encode + the copy of the compressed bytes) and on the host (PIL.Image.save, the
--jpeg_encoder host path), same process, same images, no profiler, no file system; then the single-GPU --compute_fid driver with each encoder.

    python tools/jpeg_encode_time.py [--windows 5] [--no-driver] [--driver-samples 1920]      # on the GPU -> profiles/jpeg_encode.txt
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/jpeg_encode_time.py --kernels-only   # the kernel split, in a run of its own

Batches of 64 images at 256 x 256 and 512 x 512: decoded random-weight samples (seeded VAE, seeded latents: what the drivers write with --random_weights) and
blurred noise (photograph-like statistics: a few KB per image).  Device time: windows of >= 0.3 s of back-to-back encodes between two device events after a
warm-up.  Host times: time.perf_counter around work that ends on the host (tolist / .cpu() / Pillow's save into memory)."""
import argparse
import io
import os
import re
import statistics
import subprocess
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WINDOW_S = 0.3


def timed(fn, n):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(n):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / n


def host_timed(fn, repeats):
    out = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        out.append(time.perf_counter() - t0)
    return out


def decoded_samples(dev, n, size):
    from lfm_amd.autoencoder import AutoencoderKL, images_to_uint8

    vae = AutoencoderKL.from_random(seed=0).to(dev)
    z = torch.randn(n, 4, size // 8, size // 8, generator=torch.Generator().manual_seed(size)).to(dev)
    out = []
    for k in range(0, n, 16):
        out.append(images_to_uint8(vae.decode(z[k:k + 16] / 0.18215).sample, rounding=True))
    return torch.cat(out).contiguous()


def blurred_noise(dev, n, size):
    x = torch.rand(n, 3, size, size, generator=torch.Generator().manual_seed(size + 1)).to(dev)
    for _ in range(3):
        x = torch.nn.functional.avg_pool2d(x, 5, stride=1, padding=2, count_include_pad=False)
    x = (x - x.amin((1, 2, 3), keepdim=True)) / (x.amax((1, 2, 3), keepdim=True) - x.amin((1, 2, 3), keepdim=True))
    return (x * 255).round().to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def pillow_batch(u8_dev):
    from PIL import Image

    a = u8_dev.cpu().numpy()  # the pixels' device-to-host copy is part of the host path
    total = 0
    for j in range(a.shape[0]):
        buf = io.BytesIO()
        Image.fromarray(a[j]).save(buf, format="JPEG")
        total += buf.tell()
    return total


def one_batch(name, u8, windows):
    from lfm_amd import hip, io_formats

    n, h, w, _ = u8.shape
    enc = lambda: hip.jpeg_encode(u8)  # noqa: E731
    timed(enc, 3)
    count = max(3, int(WINDOW_S / timed(enc, 5)) + 1)
    dev_t = [timed(enc, count) for _ in range(windows)]
    job = io_formats.begin_jpegs_device(u8)
    torch.cuda.synchronize()
    files = io_formats.finish_jpegs_device(job)
    copy_t = host_timed(lambda: io_formats.finish_jpegs_device(job), windows)  # lengths + compressed bytes to the host, header + slice per image
    both_t = host_timed(lambda: io_formats.encode_jpegs_device(u8), windows)   # enqueue, wait, copy: the wall time of the device path for one batch
    pil_t = host_timed(lambda: pillow_batch(u8), windows)
    ref = pillow_batch(u8)
    lens = job["device"][1].tolist()
    fell_back = sum(1 for ln in lens if ln > job["device"][0].shape[1])
    assert sum(len(f) for f in files) == ref, "the device files are not Pillow's size"
    med = statistics.median
    px = n * h * w * 3
    print(f"{name}: {n} x {h}x{w}, {sum(lens) / n / 1024:.1f} KiB per image after the header, {fell_back} over the capacity")
    print(f"  device encode            {med(dev_t) * 1e3:8.3f} ms per batch (windows of {count}: {min(dev_t) * 1e3:.3f} .. {max(dev_t) * 1e3:.3f}), "
          f"{px / med(dev_t) / 1e9:.1f} GB/s of image read, {n / med(dev_t):.0f} images/s")
    print(f"  lengths + bytes to host  {med(copy_t) * 1e3:8.3f} ms per batch ({min(copy_t) * 1e3:.3f} .. {max(copy_t) * 1e3:.3f})")
    print(f"  device path, wall        {med(both_t) * 1e3:8.3f} ms per batch ({min(both_t) * 1e3:.3f} .. {max(both_t) * 1e3:.3f})   [encode + wait + copy]")
    print(f"  Pillow path, wall        {med(pil_t) * 1e3:8.3f} ms per batch ({min(pil_t) * 1e3:.3f} .. {max(pil_t) * 1e3:.3f})   [pixels to host + PIL save to memory], "
          f"{med(pil_t) / n * 1e3:.3f} ms per image")
    print(f"  CONDITION device wall < Pillow wall: {'met' if med(both_t) < med(pil_t) else 'NOT met'} ({med(pil_t) / med(both_t):.1f} x)")
    return med(both_t) < med(pil_t)


def driver_rate(encoder, samples, tmp):
    cmd = [sys.executable, "-m", "lfm_amd.flow_latent_jpeg", "--model_type", "DiT-L/2", "--num_classes", "1", "--label_dropout", "0.", "--method", "euler",
           "--step_size", "0.02", "--image_size", "256", "--f", "8", "--num_in_channels", "4", "--num_out_channels", "4", "--random_weights", "--generator",
           "device", "--batch_size", "64", "--n_sample", str(samples), "--compute_fid", "--jpeg_encoder", encoder, "--save_dir", os.path.join(tmp, encoder)]
    r = subprocess.run(cmd, cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=900)
    if r.returncode != 0:
        raise SystemExit(r.stdout[-2000:] + r.stderr[-2000:])
    m = re.search(r"wrote (\d+) images to .* in ([0-9.]+)s", r.stdout)
    return int(m.group(1)) / float(m.group(2))


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--windows", type=int, default=5)
    p.add_argument("--no-driver", action="store_true")
    p.add_argument("--driver-samples", type=int, default=1920, help="images per --compute_fid run: the driver prints its wall time to 0.1 s, so 1920 images (about 16 s) resolve 0.6 % of the rate")
    p.add_argument("--kernels-only", action="store_true", help="twenty encodes of each batch and nothing else (for a kernel trace)")
    a = p.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("this measurement needs the GPU")
    dev = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    ok = True
    for size in (256, 512):
        for name, make in (("decoded random-weight samples", decoded_samples), ("blurred noise", blurred_noise)):
            u8 = make(dev, 64, size)
            if a.kernels_only:
                from lfm_amd import hip

                for _ in range(20):
                    hip.jpeg_encode(u8)
                torch.cuda.synchronize()
                continue
            ok = one_batch(name, u8, a.windows) and ok
    if a.kernels_only or a.no_driver:
        return
    import tempfile

    print(f"single-GPU --compute_fid, DiT-L/2, 256 x 256, batch 64, 50 Euler steps, {a.driver_samples} images, two lanes; images/s from the driver's own clock "
          "(model build excluded, graph capture of the first batches included), host and device alternating:")
    with tempfile.TemporaryDirectory() as tmp:
        rates = {"host": [], "device": []}
        for _ in range(3):
            for enc in ("host", "device"):
                rates[enc].append(driver_rate(enc, a.driver_samples, tmp))
    for enc in ("host", "device"):
        print(f"  --jpeg_encoder {enc:6s} {statistics.median(rates[enc]):7.1f} images/s  (three runs: {', '.join(f'{r:.1f}' for r in rates[enc])})")
    spread = max(rates["host"]) - min(rates["host"])
    met = statistics.median(rates["device"]) >= statistics.median(rates["host"]) - spread
    print(f"  CONDITION device not slower than host beyond the host runs' spread ({spread:.1f} images/s): {'met' if met else 'NOT met'}")
    print("The eight-rank _ddp run, the case the device encoder is for, was not measured (one GPU here): per rank the device path above replaces the all-gather of "
          "world x batch x H x W x 3 bytes and rank 0's world x batch Pillow encodes per iteration; that argument rests on the per-batch figures, not on a run.")
    if not (ok and met):
        raise SystemExit(1)


if __name__ == "__main__":
    main()
