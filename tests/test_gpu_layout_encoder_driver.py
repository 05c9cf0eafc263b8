"""The layout driver (lfm_amd/flow_latent_layout.py: the single-process driver plus the conditioning stage): ``--use_origin_adm --layout --layout_tokens FILE --random_weights`` end to end (tokens ->
BERTEmbedder -> context -> UNetModelAttn solve -> VAE decode -> the sample sheet), and that the tokens reach the images."""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHEET = "samples_cifar10_euler_1e-05_1e-05.jpg"


ARGS = ["--use_origin_adm", "--layout", "--image_size", "128", "--f", "8", "--num_in_channels", "4", "--num_out_channels", "4", "--nf", "64", "--ch_mult", "1", "2",
        "--num_res_blocks", "1", "--attn_resolutions", "1", "2", "--num_heads", "2", "--random_weights", "--generator", "device", "--batch_size", "2", "--method",
        "euler", "--step_size", "0.2"]


def _tokens(path):
    tok = np.random.default_rng(5).integers(0, 8192, size=(3, 92), dtype=np.int64)  # the default conditioner: 16 layers, 8192 ids, 92 positions
    np.save(path, tok)
    return tok


def test_single_process_driver_layout_tokens(tmp_path):
    _tokens(tmp_path / "tokens.npy")
    out = tmp_path / "out"
    out.mkdir()
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "lfm_amd.flow_latent_layout", *ARGS, "--layout_tokens", str(tmp_path / "tokens.npy"), "--save_dir", str(out)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(out) == [SHEET]
    from PIL import Image

    img = np.asarray(Image.open(out / SHEET), dtype=np.float64)
    assert img.shape == (128, 256, 3) and np.isfinite(img).all() and img.std() > 1.0  # two 128x128 images, not a constant sheet


def test_token_rows_are_taken_cyclically_and_reach_the_solve(tmp_path):
    """In process: K = 3 rows for batches of 2 -> rows (0, 1), then (2, 0); the context is computed once per batch; other tokens, another latent."""
    import torch

    from lfm_amd.flow_latent_layout import LayoutConditioner, build_cond_stage, build_models, build_parser, run_sampling

    tok = torch.from_numpy(_tokens(tmp_path / "tokens.npy"))
    args = build_parser().parse_args([*ARGS, "--layout_tokens", str(tmp_path / "tokens.npy"), "--cond_stage_layers", "2"])
    dev = torch.device("cuda:0")
    model, _, cond = build_models(args, dev)
    assert isinstance(cond, LayoutConditioner) and cond.embedder.n_layer == 2 and cond.embedder.vocab_size == 8192 and cond.embedder.max_seq_len == 92
    seen = []
    cond.embedder.register_forward_pre_hook(lambda m, inp: seen.append(inp[0].cpu()))
    x = torch.randn(2, 4, 16, 16, generator=torch.Generator().manual_seed(3)).to(dev)
    a = run_sampling(model, None, cond, args, 2, None, dev, x=x).clone()
    b = run_sampling(model, None, cond, args, 2, None, dev, x=x).clone()
    assert len(seen) == 2 and torch.equal(seen[0], tok[[0, 1]]) and torch.equal(seen[1], tok[[2, 0]])  # one encoder call per batch
    cond._cursor = 0
    assert torch.equal(run_sampling(model, None, cond, args, 2, None, dev, x=x), a)
    assert bool(a.isfinite().all()) and not torch.equal(a, b)
    plain = build_parser().parse_args(ARGS)
    assert plain.layout_tokens is None and plain.cond_stage_layers == 16 and plain.cond_stage_vocab == 8192 and plain.cond_stage_max_len == 92
    with pytest.raises(ValueError, match="--layout_tokens FILE is required"):
        build_cond_stage(plain, dev)
    with pytest.raises(ValueError, match="--use_origin_adm --layout"):
        build_cond_stage(build_parser().parse_args(["--layout_tokens", str(tmp_path / "tokens.npy"), "--random_weights"]), dev)
    with pytest.raises(ValueError, match="--cond_stage_ckpt FILE"):
        build_cond_stage(build_parser().parse_args([a_ for a_ in ARGS if a_ != "--random_weights"] + ["--layout_tokens", str(tmp_path / "tokens.npy")]), dev)


def test_one_embedder_handle_per_stream(tmp_path):
    """Batches in flight on two lanes: the conditioner drives the embedder itself on the first stream and a concurrency twin (same packed weights, its own
    workspace) on the second; the context is the same bits on either."""
    import torch

    from lfm_amd.flow_latent_layout import build_cond_stage, build_parser

    _tokens(tmp_path / "tokens.npy")
    dev = torch.device("cuda:0")
    torch.manual_seed(7)
    cond = build_cond_stage(build_parser().parse_args([*ARGS, "--layout_tokens", str(tmp_path / "tokens.npy"), "--cond_stage_layers", "2"]), dev)
    c0 = cond.context(2)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    cond._cursor = 0
    with torch.cuda.stream(side):
        c1 = cond.context(2)
    side.synchronize()
    torch.cuda.synchronize()
    first, second = cond._by_stream.values()
    assert first is cond.embedder and second is not first and second._packed is first._packed
    assert first._ws["x0"].data_ptr() != second._ws["x0"].data_ptr()
    assert torch.equal(c0, c1) and c0.data_ptr() != c1.data_ptr()


def test_compute_fid_mode_writes_every_image_through_the_lanes(tmp_path):
    """``--compute_fid`` without a feature extractor: two batches of 2 on the plain driver's two lanes, four indexed JPEGs; guidance is refused by the model
    that has no forward_with_cfg, as in the plain driver."""
    import torch

    from lfm_amd import flow_latent_layout as fl

    _tokens(tmp_path / "tokens.npy")
    common = [*ARGS, "--layout_tokens", str(tmp_path / "tokens.npy"), "--cond_stage_layers", "2", "--save_dir", str(tmp_path / "imgs")]
    try:
        fl.main([*common, "--compute_fid", "--n_sample", "4"])
        assert sorted(os.listdir(tmp_path / "imgs")) == ["0.jpg", "1.jpg", "2.jpg", "3.jpg"]
        with pytest.raises(NotImplementedError, match="forward_with_cfg"):
            fl.main([*common, "--num_classes", "5", "--cfg_scale", "1.5"])
    finally:
        torch.set_grad_enabled(True)
