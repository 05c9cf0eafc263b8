"""Mask-to-image synthesis driver with a one-kernel conditioning stage (drop-in for /root/reference/downstream_tasks/test_flow_latent_semantic_syn.py:
``sample_and_test`` and its argument parser).  The sampler pieces -- ``SpatialRescaler`` with the reference's one-hot chain, ``synthesize_batch`` -- live in
``test_flow_latent_semantic_syn.py`` next to this file, which keeps its text; this module extends them, as ``lfm_amd/flow_latent_layout.py`` extends the plain
driver.

``SpatialRescaler`` here is that class plus ``encode_labels``: the same conditioning latent from the integer label map alone.  A bilinear x0.5 stage at
align_corners=False is a 2x2 mean, three of them over a 0/1 map are the 8x8 cell mean, and the 1x1 convolution of that is, per cell, the mean of the weight
columns of its 64 labels -- one gather kernel (``lfm_label_rescale_f32``, csrc/label_rescale.h) that reads every label once; the one-hot tensor (19 GB as int64
at the reference's batch 200 x 182 classes x 256 x 256), the interpolation passes and the GEMMs are not run.  ``synthesize_batch`` here takes
``cond_path``: "onehot" (the default) IS the sampler's function, "fused" calls ``encode_labels``.

    python -m lfm_amd.downstream_tasks.flow_latent_semantic_syn --dataset celeba --exp NAME --segmentation maps.npy      # checkpoints under ./saved_info
    python -m lfm_amd.downstream_tasks.flow_latent_semantic_syn --dataset celeba --random_weights --batch_size 4        # synthetic weights and maps"""
import argparse

import torch

from . import WrapperCondFlow, sample_from_model
from . import test_flow_latent_semantic_syn as sampler
from .test_flow_latent_semantic_syn import to_range_0_1


class SpatialRescaler(sampler.SpatialRescaler):
    """The sampler's module (reference models/encoder.py:90-112: same constructor, parameters and ``forward``) with the label-map entry point."""

    def __init__(self, n_stages=1, method="bilinear", multiplier=0.5, in_channels=3, out_channels=None, bias=False):
        super().__init__(n_stages=n_stages, method=method, multiplier=multiplier, in_channels=in_channels, out_channels=out_channels, bias=bias)
        self.method = method

    def _fused(self, segmentation, num_cls):
        """Whether ``encode_labels`` runs as one lfm_label_rescale_f32 launch: label map and module on the device, bilinear x0.5 stages (each is then a 2x2 mean,
        and the chain is the mean over the 2^n x 2^n cell) and a channel mapper inside the kernel's limits."""
        from .. import hip

        if not (segmentation.is_cuda and self.remap_output and self.channel_mapper.weight.is_cuda):
            return False
        if self.method != "bilinear" or self.multiplier != 0.5 or self.channel_mapper.in_channels != num_cls:
            return False
        return hip.label_rescale_serves(num_cls, self.channel_mapper.out_channels, self.n_stages) and min(segmentation.shape[-2:]) >= 1 << self.n_stages

    def encode_labels(self, segmentation, num_cls):
        """The conditioning latent of an integer label map [N,H,W]: ``self(one_hot(segmentation, num_cls))`` without the one-hot tensor.  Where the
        module fits (``_fused``) it is one gather kernel that reads every label once (no readback: capturable, a replay follows labels rewritten in place; a
        label outside [0, num_cls) turns its cell into NaN where F.one_hot raises); everywhere else the one-hot path above."""
        if not self._fused(segmentation, num_cls):
            return self(torch.nn.functional.one_hot(segmentation, num_cls).permute(0, 3, 1, 2).float())
        from .. import hip

        cm = self.channel_mapper
        w = cm.weight.detach().reshape(cm.out_channels, num_cls).float().contiguous()  # (a view of the parameter when it is fp32, as nn.Conv2d keeps it)
        bias = cm.bias.detach().float().contiguous() if cm.bias is not None else None
        return hip.label_rescale(segmentation.contiguous(), w, bias, self.n_stages)


COND_PATHS = ("onehot", "fused")


@torch.no_grad()
def synthesize_batch(model_cond, first_stage_model, cond_stage_model, segmentation, num_cls, args, z_0=None, generator=None, cond_path="onehot"):
    """The sampler's ``synthesize_batch`` (reference :131-140; segmentation [N,S,S] int64 class ids -> images in [0,1] and the latent) with the conditioning
    stage as a choice: "onehot" calls that function as it is; "fused" takes the latent from ``SpatialRescaler.encode_labels`` (the same to fp32 rounding,
    from the labels alone) and runs the same solve and decode."""
    if cond_path not in COND_PATHS:
        raise ValueError(f"cond_path must be one of {COND_PATHS}, got {cond_path!r}")
    if cond_path == "onehot":
        return sampler.synthesize_batch(model_cond, first_stage_model, cond_stage_model, segmentation, num_cls, args, z_0=z_0, generator=generator)
    model_cond.cond = cond_stage_model.encode_labels(segmentation, num_cls)
    if z_0 is None:
        z_0 = torch.randn(segmentation.size(0), 4, args.image_size // 8, args.image_size // 8, device=segmentation.device, generator=generator)
    fake_sample = sample_from_model(model_cond, z_0, args)[-1]
    return to_range_0_1(first_stage_model.decode(fake_sample / args.scale_factor).sample), fake_sample


NUM_CLS = {"coco": 182, "ade20k": 151, "celeba": 19}  # reference :74-82


def build_parser():
    """The reference's argparse surface (:154-227), same names and defaults, plus --random_weights, --segmentation, --num_cls, --cond_path, --save_dir."""
    p = argparse.ArgumentParser("latent-flow semantic synthesis")
    p.add_argument("--seed", type=int, default=1024)
    p.add_argument("--compute_fid", action="store_true", default=False)
    p.add_argument("--epoch_id", type=int, default=425)
    p.add_argument("--image_size", type=int, default=256)
    p.add_argument("--num_in_channels", type=int, default=8)
    p.add_argument("--num_out_channels", type=int, default=4)
    p.add_argument("--nf", type=int, default=256)
    p.add_argument("--centered", action="store_false", default=True)
    p.add_argument("--resamp_with_conv", type=bool, default=True)
    p.add_argument("--num_res_blocks", type=int, default=2)
    p.add_argument("--num_heads", type=int, default=4)
    p.add_argument("--num_head_upsample", type=int, default=-1)
    p.add_argument("--num_head_channels", type=int, default=-1)
    p.add_argument("--attn_resolutions", nargs="+", type=int, default=(8, 4))
    p.add_argument("--ch_mult", nargs="+", type=int, default=(1, 2, 3, 4))
    p.add_argument("--dropout", type=float, default=0.0)
    p.add_argument("--num_classes", type=int, default=None)
    p.add_argument("--use_scale_shift_norm", type=bool, default=True)
    p.add_argument("--resblock_updown", type=bool, default=False)
    p.add_argument("--use_new_attention_order", type=bool, default=False)
    p.add_argument("--scale_factor", type=float, default=0.18215)
    p.add_argument("--exp", default="experiment_cifar_default")
    p.add_argument("--real_img_dir", default="./pytorch_fid/cifar10_train_stat.npy")
    p.add_argument("--dataset", default="cifar10")
    p.add_argument("--num_timesteps", type=int, default=200)
    p.add_argument("--batch_size", type=int, default=200)
    p.add_argument("--atol", type=float, default=1e-5)
    p.add_argument("--rtol", type=float, default=1e-5)
    p.add_argument("--method", type=str, default="dopri5", choices=["dopri5", "dopri8", "adaptive_heun", "bosh3", "euler", "midpoint", "rk4"])
    p.add_argument("--step_size", type=float, default=0.01)
    p.add_argument("--perturb", action="store_true", default=False)
    p.add_argument("--pretrained_autoencoder_ckpt", type=str, default="../stabilityai/sd-vae-ft-mse")
    p.add_argument("--random_weights", action="store_true", help="synthetic weights (and, without --segmentation, synthetic blocky label maps) instead of checkpoints")
    p.add_argument("--segmentation", type=str, default=None, help="FILE.npy: integer label maps [M, S, S] with S == --image_size, walked in batches of --batch_size")
    p.add_argument("--num_cls", type=int, default=None, help="classes of the label maps (default: the reference's table -- coco 182, ade20k 151, celeba 19)")
    p.add_argument("--cond_path", type=str, default="fused", choices=["fused", "onehot"], help="conditioning stage: one gather kernel, or the one-hot chain")
    p.add_argument("--save_dir", type=str, default=None, help="default: the reference's ./mask2image_generated_samples/{dataset}")
    # absent from the namespace unless given (read with getattr, "host" when absent): a default run's arguments stay the reference's plus the five above
    p.add_argument("--jpeg_encoder", type=str, default=argparse.SUPPRESS, choices=["host", "device"], help="host (default) = PIL.Image.save on the CPU; device = "
                   "the HIP JPEG encoder, only the compressed bytes cross to the host (the same bytes in the same files)")
    return p


def num_classes_of(args):
    if args.num_cls is not None:
        if args.num_cls < 1:
            raise SystemExit(f"--num_cls must be positive, got {args.num_cls}")
        return args.num_cls
    if args.dataset not in NUM_CLS:
        raise SystemExit(f"--dataset {args.dataset} is none of the reference's {sorted(NUM_CLS)}: give --num_cls")
    return NUM_CLS[args.dataset]


def build_models(args, device):
    """-> (8-in / 4-out origin-ADM UNet, VAE, SpatialRescaler(n_stages=3, num_cls -> 4)), from the reference's checkpoint paths (:94-116) or seeded."""
    from ..autoencoder import AutoencoderKL
    from ..io_formats import load_state_dict_file
    from ..models import get_flow_model
    from ..test_flow_latent import dezero_

    args.layout = False
    torch.manual_seed(args.seed)
    model = get_flow_model(args)
    cond_stage_model = SpatialRescaler(n_stages=3, in_channels=num_classes_of(args), out_channels=4, multiplier=0.5)
    if args.random_weights:
        dezero_(model)
        vae = AutoencoderKL.from_random(seed=args.seed)
    else:
        root = "./saved_info/latent_flow_mask2image/{}/{}".format(args.dataset, args.exp)
        cond_stage_model.load_state_dict(load_state_dict_file("{}/cond_stage_model_{}.pth".format(root, args.epoch_id)), strict=True)
        model.load_state_dict(load_state_dict_file("{}/model_{}.pth".format(root, args.epoch_id)), strict=True)
        vae = AutoencoderKL.from_pretrained(args.pretrained_autoencoder_ckpt)
    return model.to(device).eval(), vae.to(device), cond_stage_model.to(device).eval()


def synthetic_labels(n, size, num_cls, seed=0):
    """Stand-in for the reference's segmentation datasets (:74-82) when no label maps are given: 16 x 16-pixel blocks of random classes, int64 [n,size,size]."""
    g = torch.Generator().manual_seed(seed)
    blocks = torch.randint(0, num_cls, (n, -(-size // 16), -(-size // 16)), generator=g)
    return blocks.repeat_interleave(16, 1).repeat_interleave(16, 2)[:, :size, :size].contiguous()


def load_segmentation(path, size, num_cls):
    """FILE.npy -> int64 [M,size,size] on the host, every label inside [0, num_cls) (F.one_hot raises on the others in the reference)."""
    import numpy as np

    a = np.load(path, allow_pickle=False)
    if a.dtype.kind not in "iu" or a.ndim != 3 or a.shape[0] < 1 or a.shape[1:] != (size, size):
        raise SystemExit(f"--segmentation {path}: expected integer label maps [M, {size}, {size}] (S == --image_size), got {a.dtype} {a.shape}")
    seg = torch.from_numpy(a.astype(np.int64))
    lo, hi = int(seg.min()), int(seg.max())
    if lo < 0 or hi >= num_cls:
        raise SystemExit(f"--segmentation {path}: label {hi if hi >= num_cls else lo} is outside [0, {num_cls}) (--num_cls / --dataset)")
    return seg


def main(argv=None):
    import os

    from ..batch_pipeline import JpegSink, run_in_flight
    from ..io_formats import to_uint8_rounding, to_uint8_rounding_device

    args = build_parser().parse_args(argv)
    if not args.random_weights and args.segmentation is None:
        raise SystemExit("the reference's dataset classes (CocoImagesAndCaptionsValidation, ADE20kValidation, CelebAMaskValidation) are not part of this "
                         "package: give the label maps as --segmentation FILE.npy, call synthesize_batch() from your own loader, or run with "
                         "--random_weights for synthetic weights and label maps")
    num_cls = num_classes_of(args)
    seg = (load_segmentation(args.segmentation, args.image_size, num_cls) if args.segmentation is not None
           else synthetic_labels(args.batch_size, args.image_size, num_cls, seed=args.seed))
    torch.set_grad_enabled(False)
    device = torch.device("cuda:0")
    model, vae, cond_stage_model = build_models(args, device)
    model_cond = WrapperCondFlow(model, cond=None)
    save_dir = args.save_dir or "./mask2image_generated_samples/{}".format(args.dataset)
    os.makedirs(save_dir, exist_ok=True)
    torch.manual_seed(42)  # reference :71
    on_device = getattr(args, "jpeg_encoder", "host") == "device"
    sink = JpegSink("device" if on_device else "host", save_dir)
    # torchvision.utils.save_image's conversion (its `normalized=True` (:146) is no keyword of it): on the host, or where the image lives with the encoder behind it
    to_u8 = to_uint8_rounding_device if on_device else to_uint8_rounding

    def produce(i, model_cond, vae):
        batch = seg[i * args.batch_size:(i + 1) * args.batch_size].to(device)
        img, _ = synthesize_batch(model_cond, vae, cond_stage_model, batch, num_cls, args, cond_path=args.cond_path)
        print("generating batch ", i)
        return sink.begin(to_u8(img))

    # device: a batch's files are written while the next batch's kernels run (one batch behind); host: right behind the batch
    run_in_flight([(model_cond, vae, torch.cuda.current_stream(device))], -(-seg.shape[0] // args.batch_size), produce,
                  lambda i, job: sink.finish(job, i * args.batch_size), depth=1 if on_device else 0)


if __name__ == "__main__":
    main()
