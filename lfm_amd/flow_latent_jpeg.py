"""``test_flow_latent`` with one more flag, ``--jpeg_encoder {host,device}``: who encodes the per-image JPEGs of ``--compute_fid``.

    python -m lfm_amd.flow_latent_jpeg <the arguments of lfm_amd.test_flow_latent> [--jpeg_encoder device]

``host`` (the default), and every mode but ``--compute_fid``'s JPEG writing, IS ``lfm_amd.test_flow_latent.main`` with the flag taken off the command line:
PIL.Image.save on the CPU.  ``device`` runs that loop -- the same lanes, the same noise order, the same file names -- with the HIP encoder
(csrc/jpeg_encode.h) enqueued on each lane's stream behind the uint8 conversion; the drain that already runs ``lanes`` iterations behind
fetches the lengths and the compressed bytes and writes the files: the same bytes as ``host`` in every file.  The multi-GPU twin is
``lfm_amd.flow_latent_jpeg_ddp``."""
import math
import sys
import time

import torch

from . import test_flow_latent as base
from .sampler.random_util import get_generator

ENCODERS = ("host", "device")


def build_parser():
    """test_flow_latent's parser (the reference's surface and its additions) plus --jpeg_encoder."""
    p = base.build_parser()
    p.add_argument("--jpeg_encoder", type=str, default="host", choices=list(ENCODERS), help="--compute_fid's per-image JPEGs: host = PIL.Image.save on the CPU; "
                   "device = the HIP encoder on the GPU that made the batch, only the compressed bytes cross to the host (the same bytes in the same files)")
    return p


def without_encoder_flag(argv):
    """The command line as lfm_amd.test_flow_latent takes it: argparse itself takes the flag out, in every spelling it accepts (``--jpeg_encoder X``,
    ``--jpeg_encoder=X``, an unambiguous abbreviation such as ``--jpeg_enc X``).  `argv` has passed build_parser() already."""
    import argparse

    only = argparse.ArgumentParser(add_help=False)
    only.add_argument("--jpeg_encoder", choices=list(ENCODERS))
    return only.parse_known_args(list(argv))[1]


def takes_device_path(args):
    """The device encoder serves --compute_fid's JPEG writing; the feature-extractor branch writes no JPEGs and the other modes no per-image files."""
    return args.jpeg_encoder == "device" and args.compute_fid and not args.compute_nfe and not args.measure_time and not getattr(args, "fid_feature_extractor", "")


def main(argv=None):
    from collections import deque

    from .autoencoder import images_to_uint8
    from .io_formats import begin_jpegs_device, finish_jpegs_device, write_indexed_files

    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if not takes_device_path(args):
        return base.main(without_encoder_flag(argv))
    args.world_size = args.num_proc_node * args.num_process_per_node
    torch.set_grad_enabled(False)
    device = torch.device("cuda:{}".format(args.local_rank))
    torch.cuda.set_device(device)
    model, vae = base.build_models(args, device)
    generator = get_generator(args.generator, args.n_sample, args.seed)
    save_dir = args.save_dir or "./generated_samples/{}/exp{}_ep{}_m{}".format(args.dataset, args.exp, args.epoch_id, args.method)
    n = args.batch_size
    total_samples = int(math.ceil(args.n_sample / n) * n)
    t0 = time.time()
    lanes = base.make_lanes(model, vae, device, int(getattr(args, "in_flight", 0) or 0) or 2)
    pending = deque()

    def drain(p):  # (event, encoder job, batch index): what is left for the host is N lengths, the compressed bytes and one write per image
        p[0].synchronize()
        write_indexed_files(finish_jpegs_device(p[1]), save_dir, p[2] * n)

    for i in range(total_samples // n):
        mdl, va, st = lanes[i % len(lanes)]
        with torch.cuda.stream(st):
            # the single-process script writes through torchvision.utils.save_image: ROUNDING uint8 conversion (reference :264-269)
            job = begin_jpegs_device(images_to_uint8(base.run_sampling(mdl, va, args, n, generator, device), rounding=True))
            done = torch.cuda.Event()
            done.record(st)
        pending.append((done, job, i))
        if len(pending) > len(lanes):
            drain(pending.popleft())
    while pending:
        drain(pending.popleft())
    print(f"wrote {total_samples} images to {save_dir} in {time.time() - t0:.1f}s (JPEGs encoded on the device); FID needs pytorch_fid + Inception weights "
          "(not available offline): run the reference's pytorch_fid on that directory")


if __name__ == "__main__":
    main()
