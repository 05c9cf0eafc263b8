"""The DiT forward at token grids only the tiled attention kernel serves (12 x 12 = 144 tokens, 24 x 24 = 576): the golden of the unmodified reference, a table of
models against oracle/dit_ref.py through every block loop (latency, separate, folded with images that straddle 256-row tiles), the captured Euler solve and the
command-line driver at --image_size 384."""
import os
import subprocess
import sys

import pytest
import torch

pytestmark = pytest.mark.gpu

from lfm_amd import hip
from lfm_amd.models import DiT
from oracle import dit_ref, ode_ref  # checkers only

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm().clamp_min(1e-30))


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def make(dev, seed=5, **cfg_kw):
    cfg = dit_ref.DiTCfg(**cfg_kw)
    sd = dit_ref.make_dit_state(cfg, seed=seed)
    m = DiT(img_resolution=cfg.res, patch_size=cfg.patch, in_channels=cfg.in_ch, hidden_size=cfg.hidden, depth=cfg.depth, num_heads=cfg.heads,
            num_classes=cfg.num_classes, label_dropout=cfg.label_dropout)
    m.load_state_dict(sd, strict=True)
    return cfg, sd, m.to(dev).eval()


def per_image(got, ref):
    return max(rel_l2(got[i], ref[i]) for i in range(ref.shape[0]))


def test_golden_of_the_reference_at_grid_12(dev, golden_dir):
    rec = torch.load(os.path.join(golden_dir, "dit_grid12.pt"), map_location="cpu", weights_only=False)
    cfg, sd, m = make(dev, seed=rec["state_seed"], **rec["cfg"])
    assert cfg.tokens == 144 and hip.attention_plan(3, cfg.heads, cfg.hidden // cfg.heads, cfg.tokens) == 7
    x = rec["x"].to(dev)
    errs = {"v_t0d": rel_l2(m(rec["t0"].to(dev), x), rec["v_t0d"]),
            "v_tN": rel_l2(m(rec["tN"].to(dev), x, rec["y"].to(dev)), rec["v_tN"]),
            "v_cfg": rel_l2(m.forward_with_cfg(rec["t0"].to(dev), rec["x_cfg"].to(dev), rec["y_cfg"].to(dev), cfg_scale=rec["cfg_scale"]), rec["v_cfg"])}
    print(errs)
    assert max(errs.values()) < 2e-3, errs


# hidden 576 / 8 heads = head_dim 72 at 144 tokens: batch 1 takes the latency loop (144 rows are no whole 64-row tiles: the all-rows kernel), 3 and 16 the
# separate loop; hidden 128 at resolution 48 = 576 tokens
@pytest.mark.parametrize("hidden,heads,res,batch", [(576, 8, 24, 1), (576, 8, 24, 3), (576, 8, 24, 16), (128, 2, 48, 2)])
def test_models_at_the_new_grids_vs_oracle(dev, hidden, heads, res, batch):
    cfg, sd, m = make(dev, depth=2, hidden=hidden, patch=2, heads=heads, img_resolution=res, num_classes=10, label_dropout=0.1)
    assert hip.attention_plan(batch, heads, hidden // heads, cfg.tokens) == 7
    g = torch.Generator().manual_seed(hidden + batch)
    x = torch.randn(batch, 4, res, res, generator=g)
    y = torch.randint(0, 10, (batch,), generator=g)
    t = torch.rand(batch, generator=g)
    e_lab = per_image(m(t.to(dev), x.to(dev), y.to(dev)), dit_ref.dit_forward(sd, cfg, t, x, y))
    e_one = per_image(m(torch.tensor(0.37, device=dev), x.to(dev)), dit_ref.dit_forward(sd, cfg, torch.tensor(0.37), x))
    print(f"hidden {hidden} res {res} batch {batch}: per-image rel-L2 {e_lab:.3e} ([N] t, labels) {e_one:.3e} (0-d t)")
    assert e_lab < 2e-3 and e_one < 2e-3


def test_folded_path_with_images_that_straddle_tiles(dev):
    """One shared conditioning row and M = 352 x 144 = 198 tiles of 256 rows: the folded LayerNorm path runs, and an image begins in the middle of a tile."""
    batch, pick = 352, [0, 175, 351]
    cfg, sd, m = make(dev, depth=1, hidden=256, patch=2, heads=4, img_resolution=24, num_classes=1, label_dropout=0.0)
    assert (batch * cfg.tokens) % 256 == 0 and cfg.tokens % 256 != 0
    assert hip.dit_plan(m.shape_struct(), batch) == hip.PLAN_FOLDED_LN
    assert hip.dit_plan(m.shape_struct(), batch, fold_ln=hip.CALL_OFF) == 0
    x = torch.randn(batch, 4, 24, 24, generator=torch.Generator().manual_seed(352))
    t = torch.tensor(0.61)
    ref = dit_ref.dit_forward(sd, cfg, t, x[pick])
    for fold in (hip.CALL_ON, hip.CALL_OFF):
        got = m._run(t.to(dev), x.to(dev), None, False, 1.0, fold_ln=fold)
        e = per_image(got[pick], ref)
        print(f"fold_ln {fold}: per-image rel-L2 {e:.3e}")
        assert bool(torch.isfinite(got).all()) and e < 2e-3, fold


def test_captured_euler_solve_at_grid_12(dev):
    from lfm_amd.solvers import GraphedFixedGrid, torchdiffeq_euler_grid

    cfg, sd, m = make(dev, depth=2, hidden=128, patch=2, heads=2, img_resolution=24, num_classes=1, label_dropout=0.0)
    x0 = torch.randn(2, 4, 24, 24, generator=torch.Generator().manual_seed(24))
    ts, dts = torchdiffeq_euler_grid(0.1)
    s = GraphedFixedGrid(m, 2)
    s.set_grid(ts, dts)
    a = s.run(x0.to(dev)).clone()
    b = s.run(x0.to(dev)).clone()
    ref = ode_ref.odeint(lambda t, x: dit_ref.dit_forward(sd, cfg, t, x), x0, torch.tensor([1.0, 0.0]), method="euler", options={"step_size": 0.1})[-1]
    e = rel_l2(a, ref)
    print(f"10 Euler steps at 144 tokens: rel-L2 {e:.3e}")
    assert e < 1e-3
    assert torch.equal(a, b)


def test_single_process_driver_dit_at_384(tmp_path):
    """--image_size 384 with a DiT-S/2: 48 x 48 latents = 576 tokens per image, decoded at 384 x 384."""
    import numpy as np
    from PIL import Image

    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "lfm_amd.test_flow_latent", "--model_type", "DiT-S/2", "--num_classes", "1", "--label_dropout", "0.", "--method",
                        "euler", "--step_size", "0.25", "--save_dir", str(tmp_path / "g"), "--image_size", "384", "--f", "8", "--num_in_channels", "4",
                        "--num_out_channels", "4", "--random_weights", "--generator", "device", "--batch_size", "2", "--n_sample", "4"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "Samples are save at" in r.stdout
    img = Image.open(tmp_path / "g" / os.listdir(tmp_path / "g")[0])
    assert img.size == (768, 384)
    px = np.asarray(img).astype(np.float64)
    assert np.isfinite(px).all() and px.max() > px.min()  # not one colour
