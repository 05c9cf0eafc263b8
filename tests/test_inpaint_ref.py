"""CPU checks behind the GPU tests of the inpainting kernels and ``inpaint_batch_u8`` (cases, restatements, bound, mistakes: tests/inpaint_cases.py): the fp32
restatement equals what the unmodified reference's dataset class and loop lines computed (tests/golden/inpaint_prep.pt) bit for bit; every named mistake
leaves it on the GPU tests' own inputs; the fp32 restatement of the cond stage stays inside the derived bound against fp64; the driver's parser has the
reference's defaults; the file and .npy loaders and their refusals.  No GPU."""
import os

import numpy as np
import pytest
import torch

import inpaint_cases as ic


@pytest.fixture(scope="module")
def rec(golden_dir):
    return torch.load(os.path.join(golden_dir, "inpaint_prep.pt"), map_location="cpu", weights_only=False)


def test_fixture_holds_data_only(rec, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "inpaint_prep.pt")) < 700 << 10
    S, N = ic.GOLDEN_S, ic.GOLDEN_N
    assert set(rec) == {"decoded_u8", "mask_u8", "img", "mask", "masked_img", "c_in", "cc", "c5", "fake_seed", "composite", "save_image_u8", "parser_defaults"}
    assert rec["decoded_u8"].shape == (N, S, S, 3) and rec["decoded_u8"].dtype == torch.uint8 and rec["mask_u8"].shape == (N, S, S)
    assert rec["img"].shape == rec["masked_img"].shape == rec["composite"].shape == (N, 3, S, S) and rec["mask"].shape == (N, 1, S, S)
    assert rec["cc"].shape == (N, 1, S // 8, S // 8) and rec["c5"].shape == (N, 5, S // 8, S // 8) and rec["save_image_u8"].shape == (N, S, S, 3)
    vals = set(rec["mask_u8"].flatten().tolist())
    assert {0, 255} < vals and len(vals) > 20  # holes, kept pixels and intermediate greys
    assert torch.equal(rec["mask_u8"], ic.golden_pairs()[1])  # the PNG gave its bytes back


def test_fp32_restatement_is_the_reference_bit_for_bit(rec):
    image, mask, masked, cc = ic.prepare32(rec["decoded_u8"], rec["mask_u8"])
    assert torch.equal(image, rec["img"]) and torch.equal(mask, rec["mask"]) and torch.equal(masked, rec["masked_img"]) and torch.equal(cc, rec["cc"])
    assert torch.equal(cc, mask[:, :, ::8, ::8])  # F.interpolate(mask, size=R) is the pick [::8, ::8]
    assert torch.equal(ic.cond_cat32(rec["c_in"], cc, 1.0), rec["c5"])
    fake = ic.make_fake(ic.GOLDEN_N, ic.GOLDEN_S, ic.GOLDEN_S, seed=rec["fake_seed"])
    comp = ic.composite32(fake, image, mask)
    assert torch.equal(comp, rec["composite"])
    assert torch.equal(ic.save_image_bytes(comp), rec["save_image_u8"])
    assert torch.equal(ic.composite_bytes32(fake, rec["decoded_u8"], rec["mask_u8"]), rec["save_image_u8"])
    from lfm_amd.io_formats import to_uint8_rounding

    assert torch.equal(to_uint8_rounding(comp), rec["save_image_u8"])  # the package's writer conversion is the same one


def test_kept_pixels_are_the_input_byte_and_holes_the_quantised_sample():
    """Over all 256 x 256 (image byte, mask byte) pairs: mask byte 255 gives the image byte back, mask byte 0 the quantised decoded sample; and the round trip
    through [-1,1] moves 63 of the 256 image values."""
    img, mask = ic.all_pairs()
    fake = ic.make_fake(1, 256, 256, seed=1)
    out = ic.composite_bytes32(fake, img, mask)
    assert torch.equal(out[:, :, 255], img[:, :, 255])
    assert torch.equal(out[:, :, 0], ic.save_image_bytes((fake + 1.0) / 2.0)[:, :, 0])
    b = torch.arange(256, dtype=torch.float32) / 255.0
    assert int((((b * 2.0 - 1.0) + 1.0) / 2.0 != b).sum()) == 63


@pytest.mark.parametrize("name,inputs", list(ic.gpu_inputs()), ids=[n for n, _ in ic.gpu_inputs()])
def test_every_named_mistake_leaves_the_restatement_on_the_gpu_tests_inputs(name, inputs):
    """Each mistake changes at least one of the outputs the GPU test compares bit for bit, on every input that test uses.  One exception: the dropped round
    trip moves 63 of the 256 image values by one ulp and only under a grey mask byte; the 8 x 8 inputs hold some twenty grey pixels, and none of them turns
    that ulp into another byte (it shows from 8 x 24 on and 951 times on the all-pairs image).  The samples are make_fake_at_the_boundaries': at plain random
    samples neither it nor the contracted FMA would show anywhere but once on the all-pairs image."""
    img, mask, fake = inputs
    exempt = {("1x8x8", "no_round_trip"), ("3x8x8", "no_round_trip")}
    image, mask_pm1, masked, cc = ic.prepare32(img, mask)
    right = ic.composite_bytes32(fake, img, mask)
    c = torch.randn(img.shape[0], 4, *cc.shape[-2:], generator=torch.Generator().manual_seed(3))
    for m in ic.MISTAKES:
        if m in ("polarity", "pick_4", "latent_01", "layout"):
            w = ic.prepare32(img, mask, m)
            changed = [not torch.equal(a, b) for a, b in zip(w, (image, mask_pm1, masked, cc))]
            assert any(changed), (name, m)
            if m in ("pick_4", "latent_01"):
                assert changed == [False, False, False, True], (name, m, changed)
        if m in ("polarity", "trunc", "no_round_trip", "fma", "layout") and (name, m) not in exempt:
            assert not torch.equal(ic.composite_bytes32(fake, img, mask, m), right), (name, m)
        if m == "scale_mask":
            assert not torch.equal(ic.cond_cat32(c, cc, 0.18215, m)[:, 4], ic.cond_cat32(c, cc, 0.18215)[:, 4]), (name, m)
            assert torch.equal(ic.cond_cat32(c, cc, 0.18215)[:, 4:], cc)


def test_three_instruction_quotient_is_the_division_for_every_byte():
    """csrc/inpaint.h: inp_unit computes b / 255 as q = RN(b y), r = b - 255 q (one FMA, exact), RN(q + r y) with y = RN(1 / 255).  In exact rational
    arithmetic, rounded to fp32 where the kernel rounds, that is numpy's and torch's fp32 division for all 256 bytes."""
    from fractions import Fraction as Fr

    def rn(v):  # round to nearest even fp32; exact: a Fraction converts to the nearest double, and these values need far fewer than 53 - 24 guard bits
        f = np.float32(float(v))
        lo, hi = np.nextafter(f, np.float32(-np.inf)), np.nextafter(f, np.float32(np.inf))
        best = min((lo, f, hi), key=lambda c: (abs(Fr(float(c)) - v), int(np.float32(c).view(np.uint32)) & 1))
        return np.float32(best)

    y = rn(Fr(1, 255))
    assert y == np.float32(1.0) / np.float32(255.0)
    for b in range(256):
        q = rn(Fr(b) * Fr(float(y)))
        r = Fr(b) - 255 * Fr(float(q))
        assert Fr(float(rn(r))) == r  # the residual is a fp32 number: the FMA returns it exactly
        got = rn(Fr(float(q)) + r * Fr(float(y)))
        assert got == np.float32(b) / np.float32(255.0) == (torch.tensor([b], dtype=torch.uint8) / 255.0)[0].numpy(), b


COND_CASES =[(1, 1, 1), (3, 3, 5), (2, 8, 8), (3, 32, 32)]  # hw = 1 and 15: no group of four; 64 and 1024: the vector path


@pytest.mark.parametrize("N,h,w", COND_CASES)
def test_fp32_cond_restatement_stays_inside_the_derived_bound(N, h, w):
    worst = 0.0
    for extremes in (False, True):
        moments, eps = ic.make_moments(N, h, w, extremes=extremes)
        for e in (eps, None, torch.zeros_like(eps)):
            bound = ic.cond_bound(moments, e, 0.18215)
            assert bool((bound > 0).all())
            r = ic.error_ratio(ic.cond32(moments, e, 0.18215), ic.cond64(moments, e, 0.18215), bound)
            worst = max(worst, r)
    print(f"BOUND cond32 vs fp64 {N}x{h}x{w}: worst error / bound {worst:.3f}")
    assert worst <= 1.0
    moments, eps = ic.make_moments(N, h, w, extremes=True)
    assert torch.equal(ic.cond32(moments, torch.zeros_like(eps), 0.18215), ic.cond32(moments, None, 0.18215))  # eps == 0 is the mode, bit for bit
    # the bound tells a wrong clamp and a missing 0.5 from a rounding
    mean, logvar = torch.chunk(moments.double(), 2, dim=1)
    for wrong in ((mean + torch.exp(0.5 * logvar) * eps.double()) * ic.scale32(0.18215), (mean + torch.exp(torch.clamp(logvar, -30, 20)) * eps.double()) * ic.scale32(0.18215)):
        assert ic.error_ratio(wrong.float(), ic.cond64(moments, eps, 0.18215), ic.cond_bound(moments, eps, 0.18215)) > 1.0


def test_driver_parser_has_the_reference_defaults(rec):
    from lfm_amd.downstream_tasks.flow_latent_inpainting import build_parser

    mine, ref = vars(build_parser().parse_args([])), rec["parser_defaults"]
    assert {k: mine[k] for k in ref} == ref
    added = {"random_weights": False, "images": None, "masks": None, "prep_path": "fused", "posterior": "sample", "save_dir": None, "jpeg_encoder": "host"}
    assert {k: v for k, v in mine.items() if k not in ref} == added
    for bad in (["--prep_path", "eager"], ["--posterior", "mean"], ["--jpeg_encoder", "gpu"]):
        with pytest.raises(SystemExit):
            build_parser().parse_args(bad)


def test_loaders_and_their_refusals(tmp_path, rec):
    from PIL import Image

    from lfm_amd.downstream_tasks.flow_latent_inpainting import load_pairs, main, synthetic_pairs

    img, mask = ic.golden_pairs()
    gt, md = str(tmp_path / "gt"), str(tmp_path / "masks")
    ic.write_pairs(gt, md, img, mask)
    a, b = load_pairs(gt, md, 64)
    assert torch.equal(a, rec["decoded_u8"]) and torch.equal(b, rec["mask_u8"])  # Pillow decodes here what it decoded for the reference
    np.save(tmp_path / "i.npy", img.numpy())
    np.save(tmp_path / "m.npy", mask.numpy())
    a, b = load_pairs(str(tmp_path / "i.npy"), str(tmp_path / "m.npy"), 64)
    assert torch.equal(a, img) and torch.equal(b, mask) and a.dtype == b.dtype == torch.uint8
    a, b = load_pairs(str(tmp_path / "i.npy"), md, 64)  # one of each
    assert torch.equal(a, img) and torch.equal(b, mask)
    # refusals, each naming the file
    with pytest.raises(SystemExit, match=r"--image_size 32"):
        load_pairs(gt, md, 32)
    with pytest.raises(SystemExit, match=r"i\.npy: expected uint8 \[M, 32, 32, 3\]"):
        load_pairs(str(tmp_path / "i.npy"), str(tmp_path / "m.npy"), 32)
    np.save(tmp_path / "f.npy", mask.numpy().astype(np.float32))
    with pytest.raises(SystemExit, match=r"f\.npy: expected uint8"):
        load_pairs(str(tmp_path / "i.npy"), str(tmp_path / "f.npy"), 64)
    np.save(tmp_path / "m2.npy", mask.numpy()[:2])
    with pytest.raises(SystemExit, match=r"m2\.npy holds 2, but there are 3 images and 2 masks"):
        load_pairs(gt, str(tmp_path / "m2.npy"), 64)
    os.remove(os.path.join(md, "000002.png"))
    with pytest.raises(SystemExit, match=r"000002\.png does not exist, but there are 3 images and 2 masks"):
        load_pairs(gt, md, 64)
    Image.fromarray(img[1].numpy()).save(os.path.join(md, "000001.png"))  # an RGB mask
    with pytest.raises(SystemExit, match=r"000001\.png is not a single-channel 8-bit mask"):
        load_pairs(gt, md, 64)
    with pytest.raises(SystemExit, match=r"000000\.jpg does not exist"):
        load_pairs(str(tmp_path / "nothing"), md, 64)
    # the driver's own refusals come before it touches a device
    with pytest.raises(SystemExit, match="--images DIR"):
        main([])
    with pytest.raises(SystemExit, match="go together"):
        main(["--images", gt, "--random_weights"])
    with pytest.raises(SystemExit, match="multiple of 64"):
        main(["--images", gt, "--masks", md, "--image_size", "72", "--random_weights"])
    si, sm = synthetic_pairs(2, 64, seed=5)
    assert si.shape == (2, 64, 64, 3) and sm.shape == (2, 64, 64) and si.dtype == sm.dtype == torch.uint8 and set(sm.flatten().tolist()) == {0, 255}
    assert 0.05 < float((sm == 0).float().mean()) < 0.5  # 255 = keep: the box is the hole
