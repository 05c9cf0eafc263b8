"""The JPEG recipe on the CPU: the numpy restatement of jpeg_cases.py is byte-identical to Pillow on every case, io_formats.jpeg_header is the head of Pillow's
file, and each named mistake breaks identity on at least one listed case (so the list can tell a wrong kernel from a right one)."""
import numpy as np
import pytest

import jpeg_cases as jc
from lfm_amd import io_formats


@pytest.mark.parametrize("H,W", jc.SIZES)
def test_restatement_is_pillow(H, W):
    for family in jc.FAMILIES:
        img, q = jc.make_image(family, H, W)
        head, body = jc.split_pillow(jc.pillow_bytes(img, q))
        assert jc.encode_body(img, q) == body, (family, H, W)
        assert io_formats.jpeg_header(H, W, q) == head, (family, H, W)


@pytest.mark.parametrize("quality", jc.QUALITIES)
def test_header_is_pillows(quality):
    for H, W in ((1, 1), (17, 31), (250, 250)):
        img, _ = jc.make_image("noise", H, W)
        head, _ = jc.split_pillow(jc.pillow_bytes(img, quality))
        assert io_formats.jpeg_header(H, W, quality) == head
        assert len(head) == 623


def test_header_refuses_bad_quality():
    for q in (0, 101):
        with pytest.raises(ValueError):
            io_formats.jpeg_header(8, 8, q)


def test_saturated_case_stuffs_bytes():
    img, q = jc.make_image("saturated", 40, 56)
    body = jc.encode_body(img, q)
    assert body == jc.split_pillow(jc.pillow_bytes(img, q))[1]
    assert b"\xff\x00" in body[:-2]
    assert len(jc.encode_body(img, q, "no_stuffing")) < len(body)


def test_blur_q10_case_emits_zrl():
    img, q = jc.make_image("blur_q10", 40, 56)
    assert q == 10
    coef, dummy = jc.coefficients(img, q)
    data, zrl = jc.entropy(coef, dummy)
    assert data == jc.split_pillow(jc.pillow_bytes(img, q))[1]
    assert zrl >= 1


def test_flat_case_is_all_eob():
    img, q = jc.make_image("flat", 24, 40)
    coef, _ = jc.coefficients(img, q)
    assert not coef[:, 1:].any()


def test_cases_cover_dummy_blocks_and_padding():
    """the sizes reach dummy blocks to the right, below and both, odd and even heights short of a multiple of 16, and one image of many MCUs"""
    kinds = set()
    for H, W in jc.SIZES:
        _, dummy = jc.coefficients(np.zeros((H, W, 3), np.uint8))
        d = dummy.reshape(-1, 6)[:, :4]
        kinds |= {tuple(r) for r in d}
    assert {(False, True, False, True), (False, False, True, True), (False, True, True, True), (False, False, False, False)} <= kinds
    assert any(H % 2 == 0 and H % 16 for H, _ in jc.SIZES) and any(H % 2 for H, _ in jc.SIZES)


@pytest.mark.parametrize("mistake", jc.MISTAKES)
def test_named_mistake_breaks_identity(mistake):
    broken = []
    for H, W in jc.SIZES[:-1]:  # the small sizes are enough and keep this quick
        for family in ("noise", "blur", "saturated", "blur_q10"):
            img, q = jc.make_image(family, H, W)
            if jc.encode_body(img, q, mistake) != jc.encode_body(img, q):
                broken.append((family, H, W))
    assert broken, f"no listed case notices the mistake {mistake!r}"


def test_kernel_header_holds_the_same_tables():
    """csrc/jpeg_encode.h spells the Huffman specifications as the hex strings of io_formats.JPEG_HUFFMAN, and the quantisation and zig-zag tables as its tuples"""
    import os
    import re

    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lfm_amd", "csrc", "jpeg_encode.h")).read()
    for name, key in (("DC_LUMA", (0, 0)), ("AC_LUMA", (1, 0)), ("DC_CHROMA", (0, 1)), ("AC_CHROMA", (1, 1))):
        body = re.search(r"#define JPEG_DHT_%s\b(.*?)\n(?!\s*\")" % name, src, re.S).group(1)
        assert "".join(re.findall(r'"([0-9a-f]+)"', body)) == io_formats.JPEG_HUFFMAN[key].hex(), name
    numbers = lambda text: tuple(int(v) for v in re.findall(r"\d+", text))  # noqa: E731
    q = re.search(r"g_jpeg_qbase\[2\]\[64\] = \{(.*?)\};", src, re.S).group(1)
    assert numbers(q) == io_formats.JPEG_QUANT_BASE[0] + io_formats.JPEG_QUANT_BASE[1]
    z = re.search(r"zz\[64\] = \{(.*?)\};", src, re.S).group(1)
    assert numbers(z) == io_formats.JPEG_ZIGZAG
    for c in (0.298631336, 0.390180644, 0.541196100, 0.765366865, 0.899976223, 1.175875602, 1.501321110, 1.847759065, 1.961570560, 2.053119869, 2.562915447,
              3.072711026):
        assert re.search(r"= %d\b" % round(c * 8192), src), c


def test_host_side_of_the_device_writers(tmp_path):
    """Without a device: CPU and one-channel batches go to Pillow (save_jpeg's bytes), files get save_indexed_jpegs' names, the drivers' flag defaults to host."""
    import torch

    imgs = np.stack([jc.make_image(f, 17, 31)[0] for f in ("blur", "noise")])
    files = io_formats.encode_jpegs_device(torch.from_numpy(imgs))
    assert files == [jc.pillow_bytes(im) for im in imgs]
    assert io_formats.encode_jpegs_device(torch.from_numpy(imgs[..., :1].copy())) == [jc.pillow_bytes(im[..., 0]) for im in imgs]
    io_formats.save_indexed_jpegs(torch.from_numpy(imgs), str(tmp_path / "a"), 6, world_size=4, rank=1)
    io_formats.save_indexed_jpegs_device(torch.from_numpy(imgs), str(tmp_path / "b"), 6, world_size=4, rank=1)
    assert sorted(p.name for p in (tmp_path / "b").iterdir()) == ["11.jpg", "7.jpg"] == sorted(p.name for p in (tmp_path / "a").iterdir())
    for nm in ("7.jpg", "11.jpg"):
        assert (tmp_path / "a" / nm).read_bytes() == (tmp_path / "b" / nm).read_bytes()
    x = torch.rand(2, 3, 5, 7)
    assert torch.equal(io_formats.to_uint8_rounding_device(x), io_formats.to_uint8_rounding(x))
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import build_parser as semantic_parser
    from lfm_amd.flow_latent_jpeg import build_parser, takes_device_path, without_encoder_flag
    from lfm_amd.test_flow_latent import build_parser as base_parser

    assert build_parser().parse_args([]).jpeg_encoder == "host" and build_parser().parse_args(["--jpeg_encoder", "device"]).jpeg_encoder == "device"
    mine, base = vars(build_parser().parse_args([])), vars(base_parser().parse_args([]))
    assert {k: v for k, v in mine.items() if k != "jpeg_encoder"} == base  # the drivers' own surface, one flag more
    argv = ["--compute_fid", "--jpeg_encoder", "device", "--batch_size", "2", "--jpeg_encoder=host"]
    assert without_encoder_flag(argv) == ["--compute_fid", "--batch_size", "2"]
    assert without_encoder_flag(["--jpeg_enc", "host", "--compute_fid", "--batch_size", "2"]) == ["--compute_fid", "--batch_size", "2"]  # an abbreviation
    assert build_parser().parse_args(["--jpeg_enc", "device"]).jpeg_encoder == "device"
    assert takes_device_path(build_parser().parse_args(["--compute_fid", "--jpeg_encoder", "device"]))
    for other in (["--jpeg_encoder", "device"], ["--compute_fid"], ["--compute_fid", "--jpeg_encoder", "device", "--fid_feature_extractor", "a:b"]):
        assert not takes_device_path(build_parser().parse_args(other))
    assert getattr(semantic_parser().parse_args([]), "jpeg_encoder", "host") == "host"
    assert semantic_parser().parse_args(["--jpeg_encoder", "device"]).jpeg_encoder == "device"
    with pytest.raises(SystemExit):
        build_parser().parse_args(["--jpeg_encoder", "gpu"])
