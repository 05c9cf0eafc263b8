"""``test_flow_latent_ddp`` with ``--jpeg_encoder {host,device}`` (one process per GPU under torchrun, as that driver):

    torchrun --nproc-per-node 8 -m lfm_amd.flow_latent_jpeg_ddp <the arguments of lfm_amd.test_flow_latent_ddp> --compute_fid --jpeg_encoder device

``host`` (the default), and everything but ``--compute_fid``'s JPEG writing, IS ``lfm_amd.test_flow_latent_ddp.main`` with the flag taken off the command line:
every rank's pixels are all-gathered and rank 0 encodes ``world x batch`` JPEGs per iteration through PIL.Image.save.  With ``device`` nothing is gathered
and no ``GatherPipeline`` is built: every rank encodes its own batch on its GPU (csrc/jpeg_encode.h), copies the compressed bytes and
writes its own files under the reference's global index ``j * world + rank + start`` -- which is what the reference's ranks do (``test_flow_latent_ddp.py:138``).
Sharding, seeds, noise order and lanes are that driver's; the files hold the same bytes as with ``host``."""
import os
import sys

import torch
import torch.distributed as dist

from . import test_flow_latent_ddp as base
from .batch_pipeline import default_save_dir, join_lanes, lanes_for, run_in_flight
from .flow_latent_jpeg import build_parser, takes_device_path, without_encoder_flag
from .sampler.random_util import get_generator
from .test_flow_latent import build_models, run_sampling

__all__ = ["run", "main"]


def run(args, model, vae, generator, rank, world, device, to_uint8, save_encoded, log=print):
    """The sampling loop of test_flow_latent_ddp.run for one rank with the JPEGs encoded where the batch was made.  ``save_encoded(files, start)`` receives
    the finished files of this rank's batch whose first global index is ``start`` (file ``j`` is ``j * world + rank + start``).  Returns what was done:
    ``written`` lists (start, count) of THIS rank's batches."""
    from .io_formats import begin_jpegs_device, finish_jpegs_device

    total, _, iters = base.shard_plan(args.n_sample, args.batch_size, world)
    if rank == 0:
        log(f"Total number of images that will be sampled: {total}")
    lanes = lanes_for(args, model, vae, device)
    written = []

    def produce(i, mdl, va):  # the encoder rides the lane's stream
        return begin_jpegs_device(to_uint8(run_sampling(mdl, va, args, args.batch_size, generator, device)))

    def consume(i, job):  # the batch submitted `lanes` iterations ago: its lengths, its compressed bytes, one write per image; no rank waits for another
        start = i * args.batch_size * world
        save_encoded(finish_jpegs_device(job), start)
        written.append((start, int(job["images"].shape[0])))

    run_in_flight(lanes, iters, produce, consume)
    join_lanes(lanes, device)
    return {"total": total, "iters": iters, "written": written, "gather_seconds": 0.0, "lanes": len(lanes)}


def main(argv=None):
    from .autoencoder import images_to_uint8
    from .io_formats import write_indexed_files

    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if not takes_device_path(args):
        return base.main(without_encoder_flag(argv))
    torch.set_grad_enabled(False)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    device = torch.device(f"cuda:{int(os.environ.get('LOCAL_RANK', '0'))}")
    torch.cuda.set_device(device)
    dist.init_process_group("nccl", device_id=device)  # "nccl" is RCCL on ROCm; only the closing barrier uses it
    rank, world = dist.get_rank(), dist.get_world_size()
    model, vae = build_models(args, device)  # un-offset seed: --random_weights gives every rank the SAME model
    args.seed = args.seed + rank  # reference :28-32, and the global generators as test_flow_latent_ddp.main seeds them
    torch.manual_seed(args.seed)
    torch.cuda.manual_seed_all(args.seed)
    generator = get_generator(args.generator, args.n_sample, args.seed)
    save_dir = default_save_dir(args)
    res = run(args, model, vae, generator, rank, world, device, images_to_uint8,
              lambda files, start: write_indexed_files(files, save_dir, start, world_size=world, rank=rank))
    dist.barrier()
    if rank == 0:
        print(f"sampled {res['total']} images on {world} GPUs -> {save_dir} (every rank encoded and wrote its own JPEGs)")
    if dist.is_initialized():
        dist.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
