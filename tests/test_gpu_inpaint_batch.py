"""``inpaint_batch_u8`` and the inpainting driver (lfm_amd/downstream_tasks/flow_latent_inpainting.py) on the tiny 9-in / 4-out UNet and the shapes of
tests/test_gpu_downstream.py::test_inpainting_batch_vs_oracle: with the posterior's mode the fused and the torch path give the same bits; with sampling the
fused path matches the CPU oracle under that test's comparison and thresholds; a captured Euler solve is replayed on a second image / mask pair; the driver
writes one JPEG per pair, the same files with either JPEG encoder."""
import os
from argparse import Namespace

import pytest
import torch

import inpaint_cases as ic

pytestmark = pytest.mark.gpu

from oracle import ode_ref, unet_ref, vae_ref  # checkers only

CFG = dict(image_size=8, in_channels=9, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
           num_classes=None, num_heads=2, num_head_channels=-1, num_heads_upsample=-1)
LAT_TOL, IMG_TOL = 3e-3, 1e-2  # test_inpainting_batch_vs_oracle's


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _args():
    return Namespace(image_size=64, num_in_channels=9, num_out_channels=4, nf=64, num_res_blocks=1, attn_resolutions=(2,), dropout=0.0,
                     ch_mult=(1, 2), num_classes=None, num_heads=2, num_head_channels=-1, num_head_upsample=-1, layout=False,
                     scale_factor=0.18215, method="euler", step_size=0.25, perturb=False, compute_fid=True, atol=1e-5, rtol=1e-5)


@pytest.fixture(scope="module")
def setup():
    """The models and weights of test_inpainting_batch_vs_oracle; two image / mask pairs as bytes (box holes with a grey border: every kind of mask byte)."""
    from lfm_amd.autoencoder import AutoencoderKL
    from lfm_amd.models import get_flow_model

    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    dev = torch.device("cuda:0")
    usd = unet_ref.make_unet_state(CFG, seed=7)
    m = get_flow_model(_args())
    m.load_state_dict(usd, strict=True)
    vsd = vae_ref.make_vae_state(seed=3, with_encoder=True)
    vae = AutoencoderKL(with_encoder=True)
    vae.load_state_dict(vsd, strict=True)
    img, mask = ic.golden_pairs()
    z0 = torch.randn(2, 4, 8, 8, generator=torch.Generator().manual_seed(2))
    return Namespace(dev=dev, usd=usd, vsd=vsd, m=m.to(dev).eval(), vae=vae.to(dev), img=img[:2].contiguous(), mask=mask[:2].contiguous(),
                     img_b=img[1:].contiguous(), mask_b=mask[1:].contiguous(), z0=z0)


def test_mode_fused_and_torch_paths_give_the_same_bits(setup):
    from lfm_amd.downstream_tasks import WrapperCondFlow
    from lfm_amd.downstream_tasks.flow_latent_inpainting import dataset_tensors, inpaint_batch_u8

    s, args = setup, _args()
    img, mask, z0 = s.img.to(s.dev), s.mask.to(s.dev), s.z0.to(s.dev)
    image, mask_pm1, masked, _ = ic.prepare32(s.img, s.mask)
    for got, want in zip(dataset_tensors(img, mask), (image, mask_pm1, masked)):  # the torch path's tensors are the dataset's, bit for bit, on the device
        assert torch.equal(got.cpu(), want)
    wf, wt = WrapperCondFlow(s.m), WrapperCondFlow(s.m)
    out_f, lat_f = inpaint_batch_u8(wf, s.vae, img, mask, args, z_0=z0, sample_posterior=False, prep_path="fused")
    out_t, lat_t = inpaint_batch_u8(wt, s.vae, img, mask, args, z_0=z0, sample_posterior=False, prep_path="torch")
    assert out_f.dtype == torch.uint8 and out_f.shape == (2, 64, 64, 3) and out_f.is_cuda and lat_f.shape == (2, 4, 8, 8)
    assert torch.equal(wf.cond, wt.cond)
    assert torch.equal(lat_f, lat_t)
    assert torch.equal(out_f, out_t)
    keep = s.mask == 255
    assert torch.equal(out_f.cpu()[keep], s.img[keep])  # outside the hole: the input bytes
    with pytest.raises(ValueError, match="prep_path"):
        inpaint_batch_u8(wf, s.vae, img, mask, args, prep_path="eager")


def test_sampled_fused_batch_vs_oracle(setup):
    """The reference's loop with .sample(): the noise is drawn on the device from a seeded generator, eps first and z_0 second, and the oracle is given the
    same two draws."""
    import torch.nn.functional as F

    from lfm_amd.downstream_tasks import WrapperCondFlow
    from lfm_amd.downstream_tasks.flow_latent_inpainting import inpaint_batch_u8

    s, args = setup, _args()
    img, mask = s.img.to(s.dev), s.mask.to(s.dev)
    g = torch.Generator(device=s.dev).manual_seed(11)
    eps, z0 = (torch.randn(2, 4, 8, 8, device=s.dev, generator=g).cpu() for _ in range(2))
    wrap = WrapperCondFlow(s.m)
    out, lat = inpaint_batch_u8(wrap, s.vae, img, mask, args, generator=torch.Generator(device=s.dev).manual_seed(11))
    # oracle
    image, mask_pm1, masked, cc = ic.prepare32(s.img, s.mask)
    moments = vae_ref.vae_encode_moments(s.vsd, masked)
    c = ic.cond32(moments, eps, args.scale_factor)
    cond = torch.cat([c, F.interpolate(mask_pm1, size=c.shape[-2:])], 1)
    assert torch.equal(wrap.cond[:, 4:].cpu(), cc)
    ref_lat = ode_ref.odeint(lambda t, x: unet_ref.unet_forward(s.usd, CFG, t, torch.cat([x, cond], 1)), z0, torch.tensor([1.0, 0.0]), method="euler",
                             options={"step_size": 0.25})[-1]
    ref_img = (vae_ref.vae_decode(s.vsd, ref_lat / args.scale_factor) + 1) / 2
    m01, i01 = (mask_pm1 + 1) / 2, (image + 1) / 2
    ref_out = ref_img * m01 + (1 - m01) * i01
    print(f"fused sampled batch vs oracle: latent {rel_l2(lat, ref_lat):.2e}, composite bytes {rel_l2(out.float(), ic.save_image_bytes(ref_out).float()):.2e}")
    assert rel_l2(lat, ref_lat) < LAT_TOL
    assert rel_l2(out.float(), ic.save_image_bytes(ref_out).float()) < IMG_TOL  # both sides through save_image's quantisation
    keep = s.mask == 255
    assert torch.equal(out.cpu()[keep], s.img[keep])
    # the torch path draws the same noise from the same generator state (another noise would put the two latents a whole norm apart)
    _, lat_t = inpaint_batch_u8(WrapperCondFlow(s.m), s.vae, img, mask, args, generator=torch.Generator(device=s.dev).manual_seed(11), prep_path="torch")
    assert rel_l2(lat_t, lat) < 1e-3
    _, lat_other = inpaint_batch_u8(WrapperCondFlow(s.m), s.vae, img, mask, args, generator=torch.Generator(device=s.dev).manual_seed(12))
    assert rel_l2(lat_other, lat) > 0.1


def test_captured_solve_replayed_on_a_second_pair(setup):
    """What is captured is the Euler step of the solve, which reads the condition from the wrapper's own buffer (WrapperCondFlow copies an assignment of the
    same shape into it).  The three kernels run eagerly around it; inside a graph they are tests/test_gpu_inpaint_kernels.py's last test."""
    from lfm_amd.downstream_tasks import WrapperCondFlow
    from lfm_amd.downstream_tasks.flow_latent_inpainting import inpaint_batch_u8

    s, args = setup, _args()
    wrap, z0 = WrapperCondFlow(s.m), s.z0.to(s.dev)
    out_a, lat_a = inpaint_batch_u8(wrap, s.vae, s.img.to(s.dev), s.mask.to(s.dev), args, z_0=z0, sample_posterior=False)
    solvers = list(wrap.__dict__["_fused_solvers"].values())
    assert len(solvers) == 1 and "euler" in solvers[0].graphs
    graph, cond_ptr = solvers[0].graphs["euler"], wrap.cond.data_ptr()
    out_b, lat_b = inpaint_batch_u8(wrap, s.vae, s.img_b.to(s.dev), s.mask_b.to(s.dev), args, z_0=z0, sample_posterior=False)
    assert solvers[0].graphs["euler"] is graph and wrap.cond.data_ptr() == cond_ptr  # replayed, not captured again
    assert torch.equal(wrap.cond[:, 4:].cpu(), ic.prepare32(s.img_b, s.mask_b)[3])
    args.fused = False
    out_e, eager_b = inpaint_batch_u8(WrapperCondFlow(s.m), s.vae, s.img_b.to(s.dev), s.mask_b.to(s.dev), args, z_0=z0, sample_posterior=False)
    assert rel_l2(lat_b, eager_b) < 1e-6
    assert rel_l2(lat_b, lat_a) > 1e-3 and not torch.equal(out_a, out_b)
    keep = s.mask_b == 255
    assert torch.equal(out_b.cpu()[keep], s.img_b[keep])


DRIVER_ARGS = ["--image_size", "64", "--nf", "64", "--ch_mult", "1", "2", "--num_res_blocks", "1", "--attn_resolutions", "2", "--num_heads", "2",
               "--method", "euler", "--step_size", "0.5", "--batch_size", "2", "--random_weights"]


def test_driver_writes_one_jpeg_per_pair_and_the_same_files_with_either_encoder(tmp_path):
    import numpy as np
    from PIL import Image

    from lfm_amd.downstream_tasks import flow_latent_inpainting as drv

    img, mask = ic.golden_pairs()
    gt, md = str(tmp_path / "gt"), str(tmp_path / "masks")
    ic.write_pairs(gt, md, img, mask)
    decoded, _ = drv.load_pairs(gt, md, 64)
    try:
        for enc in ("host", "device"):
            drv.main([*DRIVER_ARGS, "--images", gt, "--masks", md, "--jpeg_encoder", enc, "--save_dir", str(tmp_path / enc)])  # batches of 2 and 1
        drv.main([*DRIVER_ARGS, "--save_dir", str(tmp_path / "synthetic")])  # no files: a synthetic batch
    finally:
        torch.set_grad_enabled(True)
    assert sorted(os.listdir(tmp_path / "host")) == sorted(os.listdir(tmp_path / "device")) == ["0.jpg", "1.jpg", "2.jpg"]
    assert sorted(os.listdir(tmp_path / "synthetic")) == ["0.jpg", "1.jpg"]
    for k in range(3):
        host = open(tmp_path / "host" / f"{k}.jpg", "rb").read()
        assert host == open(tmp_path / "device" / f"{k}.jpg", "rb").read(), k
        im = np.asarray(Image.open(tmp_path / "host" / f"{k}.jpg"), dtype=np.float64)
        assert im.shape == (64, 64, 3) and np.isfinite(im).all()
        keep = (mask[k] == 255).numpy()
        # outside the hole the written file is the input image up to its own JPEG coding; inside it is something else
        assert np.abs(im[~keep] - decoded[k].numpy()[~keep]).mean() > np.abs(im[keep] - decoded[k].numpy()[keep]).mean()
