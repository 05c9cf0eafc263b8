"""--jpeg_encoder device in the drivers (lfm_amd.flow_latent_jpeg, lfm_amd.flow_latent_jpeg_ddp, the semantic-synthesis driver): the same file names and the
same bytes in every file as --jpeg_encoder host (PIL.Image.save); the _ddp run() with it builds no gather pipeline and every rank accounts for its own files."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the smallest random-weight configuration of tests/test_gpu_cli.py, two batches of two images
FLOW_ARGS = ["--model_type", "DiT-S/2", "--num_classes", "1", "--label_dropout", "0.", "--method", "euler", "--step_size", "0.5", "--image_size", "256",
             "--f", "8", "--num_in_channels", "4", "--num_out_channels", "4", "--random_weights", "--generator", "device", "--batch_size", "2", "--n_sample", "4",
             "--compute_fid"]
SEMANTIC_ARGS = ["--dataset", "celeba", "--image_size", "64", "--nf", "64", "--ch_mult", "1", "2", "--num_res_blocks", "1", "--attn_resolutions", "2",
                 "--num_heads", "2", "--method", "euler", "--step_size", "0.5", "--batch_size", "2", "--random_weights"]


def _same_files(a, b, names):
    assert sorted(os.listdir(a), key=lambda s: int(s.split(".")[0])) == names == sorted(os.listdir(b), key=lambda s: int(s.split(".")[0]))
    for nm in names:
        assert open(os.path.join(a, nm), "rb").read() == open(os.path.join(b, nm), "rb").read(), nm


def test_compute_fid_writes_the_same_files_with_either_encoder(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for enc in ("host", "device"):
        r = subprocess.run([sys.executable, "-m", "lfm_amd.flow_latent_jpeg", *FLOW_ARGS, "--jpeg_encoder", enc, "--save_dir", str(tmp_path / enc)], cwd=ROOT,
                           env=env, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    _same_files(tmp_path / "host", tmp_path / "device", [f"{i}.jpg" for i in range(4)])
    from PIL import Image

    assert Image.open(tmp_path / "device" / "3.jpg").size == (256, 256)


def test_semantic_driver_writes_the_same_files_with_either_encoder(tmp_path):
    import numpy as np

    from lfm_amd.downstream_tasks import flow_latent_semantic_syn as drv

    np.save(tmp_path / "maps.npy", drv.synthetic_labels(3, 64, 19, seed=5).numpy())  # batches of 2 and 1
    for enc in ("host", "device"):
        drv.main([*SEMANTIC_ARGS, "--segmentation", str(tmp_path / "maps.npy"), "--jpeg_encoder", enc, "--save_dir", str(tmp_path / enc)])
    _same_files(tmp_path / "host", tmp_path / "device", [f"{i}.jpg" for i in range(3)])


def test_ddp_run_with_the_device_encoder_gathers_nothing(tmp_path, monkeypatch):
    from lfm_amd import flow_latent_jpeg_ddp as jddp
    from lfm_amd import io_formats
    from lfm_amd import test_flow_latent_ddp as ddp
    from lfm_amd.autoencoder import images_to_uint8
    from lfm_amd.flow_latent_jpeg import build_parser
    from lfm_amd.sampler.random_util import get_generator
    from lfm_amd.test_flow_latent import build_models

    built = []
    real = ddp.GatherPipeline

    class Counting(real):
        def __init__(self, *a, **k):
            built.append(1)
            super().__init__(*a, **k)

    monkeypatch.setattr(ddp, "GatherPipeline", Counting)
    device = torch.device("cuda:0")
    torch.set_grad_enabled(False)
    results = {}
    for enc in ("device", "host"):
        args = build_parser().parse_args([*FLOW_ARGS, "--jpeg_encoder", enc])
        model, vae = build_models(args, device)
        generator = get_generator(args.generator, args.n_sample, args.seed)
        out = str(tmp_path / enc)
        if enc == "device":
            res = jddp.run(args, model, vae, generator, 0, 1, device, images_to_uint8,
                           lambda files, start: io_formats.write_indexed_files(files, out, start, world_size=1, rank=0), log=lambda *_: None)
            assert not built, "--jpeg_encoder device must not build a GatherPipeline"
            assert res["written"] == [(0, 2), (2, 2)] and res["gather_seconds"] == 0.0 and res["total"] == 4
        else:  # what rank 0 writes from the gathered pixels: the same files
            res = ddp.run(args, model, vae, generator, 0, 1, device, images_to_uint8, log=lambda *_: None,
                          save=lambda block, start: io_formats.save_indexed_jpegs(block.cpu(), out, start))
            assert built and res["written"] == [(0, 2), (2, 2)]
        results[enc] = out
    torch.cuda.synchronize()
    _same_files(results["host"], results["device"], [f"{i}.jpg" for i in range(4)])
