"""``test_flow_latent`` with one more flag, ``--jpeg_encoder {host,device}``: who encodes the per-image JPEGs of ``--compute_fid``.

    python -m lfm_amd.flow_latent_jpeg <the arguments of lfm_amd.test_flow_latent> [--jpeg_encoder device]

``host`` (the default), and every mode but ``--compute_fid``'s JPEG writing, IS ``lfm_amd.test_flow_latent.main`` with the flag taken off the command line:
PIL.Image.save on the CPU.  ``device`` runs that driver's ``run_modes`` -- the same loop, lanes, noise order and file names -- with the HIP encoder
(csrc/jpeg_encode.h) enqueued on each lane's stream behind the uint8 conversion; the consumer that already runs ``lanes`` batches behind
fetches the lengths and the compressed bytes and writes the files: the same bytes as ``host`` in every file.  The multi-GPU twin is
``lfm_amd.flow_latent_jpeg_ddp``."""
import sys

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
    argv = list(sys.argv[1:] if argv is None else argv)
    args = build_parser().parse_args(argv)
    if not takes_device_path(args):
        return base.main(without_encoder_flag(argv))
    device = base.set_up(args)
    model, vae = base.build_models(args, device)
    base.run_modes(args, model, vae, get_generator(args.generator, args.n_sample, args.seed), device, jpeg_encoder="device")


if __name__ == "__main__":
    main()
