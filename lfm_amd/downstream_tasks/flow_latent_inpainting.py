"""Inpainting driver for image and mask files, with the elementwise work around the three heavy steps in three kernels (drop-in for
/root/reference/downstream_tasks/test_flow_latent_inpainting.py: ``sample_and_test``, its dataset class and its argument parser).  The sampler pieces --
``inpaint_batch`` on float tensors, the parser, ``build_models`` -- live in ``test_flow_latent_inpainting.py`` next to this file, which keeps its text; this
module extends them, as ``flow_latent_semantic_syn.py`` extends its sampler file.

The reference's loop reads ``./gt_celeb/%06d.jpg`` and ``masks_val_256_small_eval/%06d.png``, turns them into three fp32 tensors per image on the host
(``CustomizedInpaintingEvalDataset.__getitem__``: /255, 1 - mask, the masked image, three times ``* 2 - 1``), uploads those 28 bytes per pixel, and around VAE
encode, solve and decode runs some twenty elementwise torch ops (nearest resize, posterior sample and scale, cat, three ``to_range_0_1``, the composite,
``save_image``'s quantisation).  ``inpaint_batch_u8`` takes the bytes -- uint8 NHWC images and the mask PNG's bytes as stored (255 = keep, 0 = hole), 4 bytes per
pixel -- and with ``prep_path="fused"`` does all of that arithmetic in ``lfm_inpaint_prepare_u8``, ``lfm_inpaint_cond_f32`` and ``lfm_inpaint_composite_u8``
(csrc/inpaint.h), bit for bit as the reference's fp32 operation sequence does it; ``prep_path="torch"`` builds the dataset's tensors with torch ops on the
device and calls the sampler's ``inpaint_batch``.

    python -m lfm_amd.downstream_tasks.flow_latent_inpainting --exp NAME --images ./gt_celeb --masks ./dataset/masks_val_256_small_eval   # checkpoints under ./saved_info
    python -m lfm_amd.downstream_tasks.flow_latent_inpainting --random_weights --batch_size 4                                           # synthetic weights and batch"""
import os

import torch

from . import WrapperCondFlow, sample_from_model
from . import test_flow_latent_inpainting as sampler
from .test_flow_latent_inpainting import build_models  # noqa: F401  (the driver's models are the sampler's)

PREP_PATHS = ("fused", "torch")


def dataset_tensors(image_u8, mask_u8):
    """``CustomizedInpaintingEvalDataset.__getitem__`` (reference :36-55) on a batch of bytes, with torch ops where the bytes live: uint8 NHWC [N,S,S,3] and
    uint8 [N,S,S] -> (image [N,3,S,S] in [-1,1], mask [N,1,S,S] in [-1,1] with +1 = hole, masked image [N,3,S,S]), the same bits as the reference's host
    arithmetic.  The divisor is a tensor on the bytes' device: with a Python scalar torch multiplies by the rounded reciprocal on a GPU, which is one ulp off
    the dataset's division for some bytes."""
    d255 = torch.full((), 255.0, dtype=torch.float32, device=image_u8.device)
    img = image_u8.permute(0, 3, 1, 2).to(torch.float32) / d255
    mask = 1 - mask_u8.to(torch.float32) / d255
    masked = (1 - mask).unsqueeze(1) * img
    return img * 2.0 - 1.0, (mask * 2.0 - 1.0).unsqueeze(1), masked * 2.0 - 1.0


@torch.no_grad()
def inpaint_batch_u8(model_cond, vae, image_u8, mask_u8, args, z_0=None, generator=None, sample_posterior=True, prep_path="fused"):
    """One iteration of the reference's loop (:142-166) from the bytes: image_u8 uint8 NHWC [N,S,S,3] and mask_u8 uint8 [N,S,S] on the device ->
    (the composite as ``save_image`` quantises it, uint8 NHWC [N,S,S,3] on the device; the generated latent).

    "fused": lfm_inpaint_prepare_u8 -> ``vae.encode`` -> lfm_inpaint_cond_f32 (eps drawn by ``torch.randn`` on the device) -> solve -> ``vae.decode`` ->
    lfm_inpaint_composite_u8.  "torch": ``dataset_tensors``, the sampler's ``inpaint_batch`` and ``to_uint8_rounding_device``.  Both draw eps and then z_0 from
    `generator` in the same shapes and order, so one generator state gives one noise on either path; with ``sample_posterior=False`` (``dist.mode()``) no eps
    is drawn and the two paths give the same bits."""
    if prep_path not in PREP_PATHS:
        raise ValueError(f"prep_path must be one of {PREP_PATHS}, got {prep_path!r}")
    if prep_path == "torch":
        from ..io_formats import to_uint8_rounding_device

        image, mask, masked = dataset_tensors(image_u8, mask_u8)
        out, fake_sample = sampler.inpaint_batch(model_cond, vae, image, mask, masked, args, z_0=z_0, generator=generator, sample_posterior=sample_posterior)
        return to_uint8_rounding_device(out), fake_sample
    from .. import hip

    N, R = image_u8.shape[0], args.image_size // 8
    cond = torch.empty(N, 5, R, R, dtype=torch.float32, device=image_u8.device)
    masked, _ = hip.inpaint_prepare(image_u8, mask_u8, cond)
    moments = vae.encode(masked).latent_dist.parameters
    eps = torch.randn(N, 4, R, R, device=image_u8.device, generator=generator) if sample_posterior else None  # DiagonalGaussianDistribution.sample's draw
    model_cond.cond = hip.inpaint_cond(moments, eps, args.scale_factor, cond)
    if z_0 is None:
        z_0 = torch.randn(N, 4, R, R, device=image_u8.device, generator=generator)
    fake_sample = sample_from_model(model_cond, z_0, args)[-1]
    fake_image = vae.decode(fake_sample / args.scale_factor).sample
    return hip.inpaint_composite(fake_image, image_u8, mask_u8), fake_sample


def build_parser():
    """The reference's argparse surface (:171-222; the sampler file's parser, --random_weights included) plus --images, --masks, --prep_path, --posterior,
    --save_dir and --jpeg_encoder."""
    p = sampler.build_parser()
    p.add_argument("--images", type=str, default=None, help="the ground-truth images: a directory of %%06d.jpg (the reference's ./gt_celeb), walked from 0, or "
                   "FILE.npy holding uint8 [M, S, S, 3] with S == --image_size")
    p.add_argument("--masks", type=str, default=None, help="the masks, 255 = keep and 0 = hole: a directory of %%06d.png (the reference's "
                   "./dataset/masks_val_256_small_eval) or FILE.npy holding uint8 [M, S, S]")
    p.add_argument("--prep_path", type=str, default="fused", choices=list(PREP_PATHS), help="the arithmetic around encode, solve and decode: three HIP kernels "
                   "on the bytes, or the reference's torch ops on the device")
    p.add_argument("--posterior", type=str, default="sample", choices=["sample", "mode"], help="the masked image's latent: the reference's .sample(), or the mean")
    p.add_argument("--save_dir", type=str, default=None, help="default: the reference's ./inpainting_generated_samples/{dataset}")
    p.add_argument("--jpeg_encoder", type=str, default="host", choices=["host", "device"], help="host = PIL.Image.save on the CPU; device = the HIP JPEG "
                   "encoder, only the compressed bytes cross to the host (the same bytes in the same files)")
    return p


def driver_parser():
    """``build_parser()`` (the sampling surface, which keeps its set of arguments) plus the driver's evaluation flag --ssim."""
    p = build_parser()
    p.add_argument("--ssim", action="store_true", help="score each batch's composites against the ground truth on the device before they are encoded "
                   "(lfm_ssim_u8) and print SSIM in total and per decile of mask area at the end: the pre-JPEG score; the files are the same with or without")
    return p


def _load_npy(path, size, flag, tail):
    import numpy as np

    a = np.load(path, allow_pickle=False)
    want = (size, size) + tail
    if a.dtype != np.uint8 or a.ndim != 3 + len(tail) or a.shape[0] < 1 or a.shape[1:] != want:
        raise SystemExit(f"{flag} {path}: expected uint8 [M, {', '.join(str(v) for v in want)}] (S == --image_size), got {a.dtype} {a.shape}")
    return np.ascontiguousarray(a)


def _load_dir(path, size, flag, ext, rgb):
    """{path}/%06d.{ext} walked from 0 while the file exists, decoded with Pillow as the reference's dataset does (:37, :40)."""
    import numpy as np
    from PIL import Image

    out = []
    while os.path.exists(name := os.path.join(path, f"{len(out):06d}.{ext}")):
        with Image.open(name) as im:
            a = np.array(im.convert("RGB") if rgb else im)
        if not rgb and (a.ndim != 2 or a.dtype != np.uint8):
            raise SystemExit(f"{flag}: {name} is not a single-channel 8-bit mask (mode {im.mode}, array {a.dtype} {a.shape})")
        if a.shape[:2] != (size, size):
            raise SystemExit(f"{flag}: {name} is {a.shape[1]} x {a.shape[0]}, not --image_size {size}")
        out.append(a)
    if not out:
        raise SystemExit(f"{flag}: {name} does not exist")
    return np.stack(out)


def load_pairs(images, masks, size):
    """--images / --masks -> (uint8 [M,S,S,3], uint8 [M,S,S]) on the host: what the reference's dataset decodes, before any arithmetic.  Each is a directory in
    the reference's naming or a .npy; a mask that is not single-channel, a size other than `size` or unequal counts end in SystemExit naming the file."""
    img = _load_npy(images, size, "--images", (3,)) if images.endswith(".npy") else _load_dir(images, size, "--images", "jpg", True)
    msk = _load_npy(masks, size, "--masks", ()) if masks.endswith(".npy") else _load_dir(masks, size, "--masks", "png", False)
    if img.shape[0] != msk.shape[0]:
        (flag, path, ext), k = (("--masks", masks, "png") if msk.shape[0] < img.shape[0] else ("--images", images, "jpg")), min(img.shape[0], msk.shape[0])
        short = f"{path} holds {k}" if path.endswith(".npy") else f"{os.path.join(path, f'{k:06d}.{ext}')} does not exist"
        raise SystemExit(f"{flag}: {short}, but there are {img.shape[0]} images and {msk.shape[0]} masks")
    return torch.from_numpy(img), torch.from_numpy(msk)


def synthetic_pairs(n, size, seed=0):
    """The sampler file's ``synthetic_batch`` (smooth random images, box holes) as the bytes a dataset on disk would hold."""
    image, mask, _ = sampler.synthetic_batch(n, size, "cpu", seed=seed)
    img = ((image + 1) / 2).mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    return img, ((mask[:, 0] < 0).to(torch.uint8) * 255).contiguous()


def main(argv=None):
    from ..batch_pipeline import JpegSink, run_in_flight

    args = driver_parser().parse_args(argv)
    if (args.images is None) != (args.masks is None):
        raise SystemExit("--images and --masks go together")
    if args.images is None and not args.random_weights:
        raise SystemExit("give the reference's data as --images DIR|FILE.npy (./gt_celeb) and --masks DIR|FILE.npy (./dataset/masks_val_256_small_eval), call "
                         "inpaint_batch_u8() from your own loader, or run with --random_weights for synthetic weights and a synthetic batch")
    if args.image_size % 64:
        raise SystemExit(f"--image_size must be a multiple of 64 (the VAE encoder's), got {args.image_size}")
    imgs, masks = (load_pairs(args.images, args.masks, args.image_size) if args.images is not None
                   else synthetic_pairs(args.batch_size, args.image_size, seed=args.seed))
    torch.set_grad_enabled(False)
    device = torch.device("cuda:0")
    model, vae = build_models(args, device)
    model_cond = WrapperCondFlow(model, cond=None)
    save_dir = args.save_dir or "./inpainting_generated_samples/{}".format(args.dataset)
    os.makedirs(save_dir, exist_ok=True)
    torch.manual_seed(42)  # reference :95
    score = None
    if args.ssim:  # the composites are scored where they are: N floats and N mask sums per batch stay on the device until the table is printed
        from .. import inpaint_eval

        score = inpaint_eval.SSIMScore()
    sink = JpegSink(args.jpeg_encoder, save_dir)

    def produce(i, model_cond, vae):  # index = i * batch_size + j (:163; the last batch may be ragged)
        rows = slice(i * args.batch_size, (i + 1) * args.batch_size)
        image_u8, mask_u8 = imgs[rows].to(device), masks[rows].to(device)  # the bytes: 4 per pixel
        out, _ = inpaint_batch_u8(model_cond, vae, image_u8, mask_u8, args, sample_posterior=args.posterior == "sample", prep_path=args.prep_path)
        if score is not None:
            score(out, image_u8, mask_u8)
        print("generating batch ", i)
        return sink.begin(out)  # device: the encoder behind the composite on the same stream

    # device: a batch's files are written while the next batch's kernels run (one batch behind); host: right behind the batch
    run_in_flight([(model_cond, vae, torch.cuda.current_stream(device))], -(-imgs.shape[0] // args.batch_size), produce,
                  lambda i, job: sink.finish(job, i * args.batch_size), depth=1 if args.jpeg_encoder == "device" else 0)
    if score is not None:
        groups, names = inpaint_eval.area_bins(score.mask_sums, args.image_size, args.image_size)
        print(inpaint_eval.format_table(inpaint_eval.results_by_name(score, groups, names), title="SSIM of the composites before JPEG coding"))


if __name__ == "__main__":
    main()
