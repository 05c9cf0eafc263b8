"""Mask-to-image synthesis with the fused conditioning stage (lfm_amd/downstream_tasks/flow_latent_semantic_syn.py): ``cond_path="fused"`` against the CPU
oracle at the shape and thresholds of tests/test_gpu_downstream.py::test_semantic_synthesis_batch_vs_oracle, the conditioning latent per element at the bound
of tests/semantic_cond_cases.py, a captured Euler solve replayed after the label map is rewritten in place, and the driver's ``main``."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import semantic_cond_cases as sc

pytestmark = pytest.mark.gpu

from oracle import ode_ref, unet_ref, vae_ref  # checkers only

NUM_CLS = 19
CFG = dict(image_size=8, in_channels=8, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
           num_classes=None, num_heads=2, num_head_channels=-1, num_heads_upsample=-1)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _args():
    return Namespace(image_size=64, num_in_channels=8, num_out_channels=4, nf=64, num_res_blocks=1, attn_resolutions=(2,), dropout=0.0,
                     ch_mult=(1, 2), num_classes=None, num_heads=2, num_head_channels=-1, num_head_upsample=-1, layout=False,
                     scale_factor=0.18215, method="euler", step_size=0.5, perturb=False, compute_fid=True, atol=1e-5, rtol=1e-5)


@pytest.fixture(scope="module")
def setup():
    """The models, weights and inputs of test_semantic_synthesis_batch_vs_oracle."""
    from lfm_amd.autoencoder import AutoencoderKL
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import SpatialRescaler
    from lfm_amd.models import get_flow_model

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    usd = unet_ref.make_unet_state(CFG, seed=9)
    m = get_flow_model(_args())
    m.load_state_dict(usd, strict=True)
    vsd = vae_ref.make_vae_state(seed=3)
    vae = AutoencoderKL()
    vae.load_state_dict(vsd, strict=True)
    torch.manual_seed(5)
    cs = SpatialRescaler(n_stages=3, in_channels=NUM_CLS, out_channels=4, multiplier=0.5)
    wmap = cs.channel_mapper.weight.detach().clone()
    seg = torch.randint(0, NUM_CLS, (2, 64, 64), generator=torch.Generator().manual_seed(3))
    z0 = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(4))
    return Namespace(dev=dev, usd=usd, vsd=vsd, m=m.to(dev).eval(), vae=vae.to(dev), cs=cs.to(dev), wmap=wmap, seg=seg, z0=z0)


def test_fused_conditioning_batch_vs_oracle(setup):
    from lfm_amd.downstream_tasks import WrapperCondFlow
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import synthesize_batch

    s, args = setup, _args()
    wrap = WrapperCondFlow(s.m)
    img, lat = synthesize_batch(wrap, s.vae, s.cs, s.seg.to(s.dev), NUM_CLS, args, z_0=s.z0.to(s.dev), cond_path="fused")
    # the conditioning latent itself, per element, against the float64 restatement; and the very bits of the kernel's stated order
    w2 = s.wmap.reshape(4, NUM_CLS)
    r = sc.error_ratio(wrap.cond.cpu(), sc.restate64(s.seg, w2, None, 3), sc.bound(s.seg, w2, None, 3))
    print(f"BOUND conditioning latent 2x64x64 cls19: error / bound {r:.3f}")
    assert wrap.cond.shape == (2, 4, 8, 8) and r <= 1.0
    assert torch.equal(wrap.cond.cpu(), sc.emulate_kernel32(s.seg, w2, None, 3))
    # oracle: the reference's chain on the CPU, unet_ref on the concatenated state, vae_ref
    c = F.one_hot(s.seg, NUM_CLS).permute(0, 3, 1, 2).float()
    for _ in range(3):
        c = F.interpolate(c, scale_factor=0.5, mode="bilinear")
    cond = F.conv2d(c, s.wmap)
    ref_lat = ode_ref.odeint(lambda t, x: unet_ref.unet_forward(s.usd, CFG, t, torch.cat([x, cond], 1)), s.z0, torch.tensor([1.0, 0.0]), method="euler",
                             options={"step_size": 0.5})[-1]
    ref_img = (vae_ref.vae_decode(s.vsd, ref_lat / args.scale_factor) + 1) / 2
    assert img.shape == (2, 3, 64, 64) and lat.shape == (2, 4, 8, 8)
    assert rel_l2(lat, ref_lat) < 3e-3
    assert rel_l2(img, ref_img) < 1e-2
    # the default path is the one-hot chain, as before
    _, lat1 = synthesize_batch(WrapperCondFlow(s.m), s.vae, s.cs, s.seg.to(s.dev), NUM_CLS, args, z_0=s.z0.to(s.dev))
    assert rel_l2(lat1, ref_lat) < 3e-3 and rel_l2(lat, lat1) < 3e-3


def test_captured_solve_replayed_after_the_label_map_is_rewritten_in_place(setup):
    from lfm_amd.downstream_tasks import WrapperCondFlow
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import synthesize_batch

    """What is captured here is the Euler step of the solve, which reads the condition from the wrapper's own buffer.  ``encode_labels`` runs eagerly before
    each solve and its result is copied into that buffer, so the second batch replays the first batch's graph on the new labels' latent.  The label kernel
    inside a captured graph, replayed on labels rewritten in place, is tests/test_gpu_label_rescale.py::test_captured_replay_follows_rewritten_labels."""
    s, args = setup, _args()
    wrap = WrapperCondFlow(s.m)
    seg, z0 = s.seg.to(s.dev), s.z0.to(s.dev)
    _, lat_a = synthesize_batch(wrap, s.vae, s.cs, seg, NUM_CLS, args, z_0=z0, cond_path="fused")
    solvers = list(wrap.__dict__["_fused_solvers"].values())
    assert len(solvers) == 1 and "euler" in solvers[0].graphs
    graph, cond_ptr = solvers[0].graphs["euler"], wrap.cond.data_ptr()
    other = torch.flip(s.seg, [0, 2]).contiguous()
    seg.copy_(other.to(s.dev))  # the same device tensor, new labels
    _, lat_b = synthesize_batch(wrap, s.vae, s.cs, seg, NUM_CLS, args, z_0=z0, cond_path="fused")
    assert solvers[0].graphs["euler"] is graph and wrap.cond.data_ptr() == cond_ptr  # replayed, not captured again
    assert torch.equal(wrap.cond.cpu(), sc.emulate_kernel32(other, s.wmap.reshape(4, NUM_CLS), None, 3))
    args.fused = False
    _, eager_b = synthesize_batch(WrapperCondFlow(s.m), s.vae, s.cs, other.to(s.dev), NUM_CLS, args, z_0=z0, cond_path="fused")
    assert rel_l2(lat_b, eager_b) < 1e-6
    assert rel_l2(lat_b, lat_a) > 1e-3


DRIVER_ARGS = ["--dataset", "celeba", "--image_size", "64", "--nf", "64", "--ch_mult", "1", "2", "--num_res_blocks", "1", "--attn_resolutions", "2",
               "--num_heads", "2", "--method", "euler", "--step_size", "0.5", "--batch_size", "2", "--random_weights"]


def test_main_writes_one_jpeg_per_label_map(tmp_path):
    from PIL import Image

    from lfm_amd.downstream_tasks import flow_latent_semantic_syn as drv

    maps = np.random.default_rng(7).integers(0, 19, size=(3, 4, 4)).repeat(16, 1).repeat(16, 2).astype(np.int32)
    np.save(tmp_path / "maps.npy", maps)
    out = tmp_path / "imgs"
    try:
        drv.main([*DRIVER_ARGS, "--segmentation", str(tmp_path / "maps.npy"), "--save_dir", str(out)])  # batches of 2 and 1
        with pytest.raises(SystemExit, match="--segmentation FILE.npy"):
            drv.main([a for a in DRIVER_ARGS if a != "--random_weights"])
    finally:
        torch.set_grad_enabled(True)
    assert sorted(os.listdir(out)) == ["0.jpg", "1.jpg", "2.jpg"]
    imgs = [np.asarray(Image.open(out / f"{k}.jpg"), dtype=np.float64) for k in range(3)]
    assert all(im.shape == (64, 64, 3) and np.isfinite(im).all() and im.std() > 1.0 for im in imgs)
    assert not np.array_equal(imgs[0], imgs[1])
