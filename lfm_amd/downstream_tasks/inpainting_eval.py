"""Score inpainted files against their ground truth: per-image SSIM on the device, reported for the whole set and per decile of the mask's area, as the
reference's ``InpaintingEvaluator`` with ``SSIMScore`` reports it (datasets_prep/inpaint_preprocess/evaluator.py, losses/base_loss.py; lfm_amd/inpaint_eval.py
is the host side, csrc/ssim.h the kernel).  This is the faithful evaluation: it scores the files as they were written, their JPEG coding included.

    python -m lfm_amd.downstream_tasks.inpainting_eval --generated ./inpainting_generated_samples/celeba_256 --images ./gt_celeb \\
        --masks ./dataset/masks_val_256_small_eval [--image_size 256] [--batch_size 32] [--bins 10] [--out scores.json]

--images and --masks are what ``flow_latent_inpainting`` takes (``load_pairs``: directories of %06d.jpg / %06d.png, or .npy); --generated is the directory that
driver wrote ({index}.jpg, walked from 0; %06d.jpg is understood too) or FILE.npy holding uint8 [M, S, S, 3].  LPIPS and FID, the reference evaluator's
other scores, need network weights and are not computed."""
import argparse
import json
import os

import torch

from .. import inpaint_eval
from .flow_latent_inpainting import _load_npy, load_pairs


def load_generated(path, size):
    """--generated -> uint8 [M,S,S,3] on the host."""
    import numpy as np
    from PIL import Image

    if path.endswith(".npy"):
        return torch.from_numpy(_load_npy(path, size, "--generated", (3,)))
    fmt = "{}.jpg" if os.path.exists(os.path.join(path, "0.jpg")) else "{:06d}.jpg"
    out = []
    while os.path.exists(name := os.path.join(path, fmt.format(len(out)))):
        with Image.open(name) as im:
            a = np.array(im.convert("RGB"))
        if a.shape[:2] != (size, size):
            raise SystemExit(f"--generated: {name} is {a.shape[1]} x {a.shape[0]}, not --image_size {size}")
        out.append(a)
    if not out:
        raise SystemExit(f"--generated: {name} does not exist")
    return torch.from_numpy(np.stack(out))


def build_parser():
    p = argparse.ArgumentParser(description="SSIM of inpainted images against the ground truth, in total and per decile of mask area")
    p.add_argument("--generated", type=str, required=True, help="the inpainted images: the inpainting driver's --save_dir ({index}.jpg) or FILE.npy uint8 [M, S, S, 3]")
    p.add_argument("--images", type=str, required=True, help="the ground truth: a directory of %%06d.jpg or FILE.npy uint8 [M, S, S, 3]")
    p.add_argument("--masks", type=str, required=True, help="the masks, 255 = keep and 0 = hole: a directory of %%06d.png or FILE.npy uint8 [M, S, S]")
    p.add_argument("--image_size", type=int, default=256)
    p.add_argument("--batch_size", type=int, default=32)
    p.add_argument("--bins", type=int, default=10, help="groups by the share of the image the mask opens")
    p.add_argument("--window_size", type=int, default=11)
    p.add_argument("--out", type=str, default=None, help="write the table as JSON to this file")
    return p


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.batch_size < 1 or args.bins < 1:
        raise SystemExit("--batch_size and --bins must be at least 1")
    imgs, masks = load_pairs(args.images, args.masks, args.image_size)
    gen = load_generated(args.generated, args.image_size)
    if gen.shape[0] != imgs.shape[0]:
        raise SystemExit(f"--generated: {args.generated} holds {gen.shape[0]} images, but there are {imgs.shape[0]} pairs")
    results = inpaint_eval.evaluate(gen, imgs, masks, batch_size=args.batch_size, bins=args.bins, window_size=args.window_size)
    print(inpaint_eval.format_table(results, title="SSIM of the files as written"))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(inpaint_eval.results_json(results), f, indent=1)
    return results


if __name__ == "__main__":
    main()
