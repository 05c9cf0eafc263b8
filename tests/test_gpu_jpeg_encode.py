"""lfm_jpeg_encode_rgb8 (include/lfm_hip.h, csrc/jpeg_encode.h): io_formats.jpeg_header + the device's bytes are the file PIL.Image.save writes, on every case
of tests/jpeg_cases.py (pinned on the CPU in tests/test_jpeg_ref.py), through hip.jpeg_encode and through the C entry points with poisoned guard rows around the
input and sentinels around `out` and the workspace; true lengths beyond the capacity; independence of the batch; refusals; a captured replay.  Pillow's bytes are
made here, on the machine the test runs on."""
import ctypes as C
from collections import defaultdict

import numpy as np
import pytest
import torch

import jpeg_cases as jc
from lfm_amd import hip, io_formats

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = 0xA5, 4096


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _encode_c(dev, imgs, quality, cap=None, shift=0):
    """The C entry points on guarded buffers -> (out [N, cap] uint8 on the host, lengths list).  imgs: uint8 [N, H, W, 3] numpy.  The input lies between two
    poisoned guard regions (0xFF: a row read beyond the image would change the bytes), `out` and the workspace between sentinels that must survive.
    shift: bytes the image is moved inside its buffer (1: not 16-byte aligned, the byte-wise loads)."""
    N, H, W, _ = imgs.shape
    cap = hip.jpeg_default_capacity(H, W) if cap is None else cap
    L = hip.lib()
    need = L.lfm_jpeg_encode_workspace_bytes(N, H, W, cap)
    assert need > 0 and need % 16 == 0
    g_in = 4 * W * 3 + 64  # four guard rows either side
    ibuf = torch.full((imgs.size + 2 * g_in + 16,), 0xFF, dtype=torch.uint8, device=dev)
    assert ibuf.data_ptr() % 16 == 0
    g_in = -(-g_in // 16) * 16 + shift
    din = ibuf[g_in:g_in + imgs.size]
    din.copy_(torch.from_numpy(imgs).reshape(-1))
    obuf = torch.full((N * cap + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    wbuf = torch.full((need + 2 * GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
    lbuf = torch.full((N + 2,), -77, dtype=torch.int32, device=dev)
    rc = L.lfm_jpeg_encode_rgb8(C.c_void_p(din.data_ptr()), N, H, W, quality, cap, C.c_void_p(wbuf.data_ptr() + GUARD), need,
                                C.c_void_p(obuf.data_ptr() + GUARD), C.c_void_p(lbuf.data_ptr() + 4), hip.stream_ptr(dev))
    assert rc == 0, rc
    torch.cuda.synchronize()
    o, w, l = obuf.cpu(), wbuf.cpu(), lbuf.cpu()
    assert bool((o[:GUARD] == SENTINEL).all()) and bool((o[GUARD + N * cap:] == SENTINEL).all()), "wrote outside out"
    assert bool((w[:GUARD] == SENTINEL).all()) and bool((w[GUARD + need:] == SENTINEL).all()), "wrote outside the workspace"
    assert int(l[0]) == -77 and int(l[-1]) == -77, "wrote outside lengths"
    return o[GUARD:GUARD + N * cap].view(N, cap).numpy(), l[1:-1].tolist()


def _encode_py(dev, imgs, quality, cap=None):
    out, lengths = hip.jpeg_encode(torch.from_numpy(imgs).to(dev), quality=quality, capacity=cap)
    assert out.dtype == torch.uint8 and lengths.dtype == torch.int32
    return out.cpu().numpy(), lengths.tolist()


def _check_against_pillow(imgs, quality, out, lengths, what):
    """Every image that fits: header + device bytes == Pillow's file; every length is Pillow's, fit or not; bytes beyond the length are not looked at."""
    N, H, W, _ = imgs.shape
    head = io_formats.jpeg_header(H, W, quality)
    for i in range(N):
        ref = jc.pillow_bytes(imgs[i], quality)
        assert lengths[i] == len(ref) - len(head), (what, i, lengths[i], len(ref) - len(head))
        if lengths[i] <= out.shape[1]:
            assert head + out[i, :lengths[i]].tobytes() == ref, (what, i)


def _batches(H, W):
    """The content families of one size, batched by quality: [(quality, names, uint8 [n, H, W, 3])]."""
    by_q = defaultdict(list)
    for family in jc.FAMILIES:
        img, q = jc.make_image(family, H, W)
        by_q[q].append((family, img))
    return [(q, [f for f, _ in v], np.stack([im for _, im in v])) for q, v in sorted(by_q.items())]


@pytest.mark.parametrize("H,W", jc.SIZES)
def test_every_case_is_pillows_file(dev, H, W):
    for quality, names, imgs in _batches(H, W):
        cap = 4 * hip.jpeg_default_capacity(H, W) + 64  # noise at quality 100 takes more than a byte per pixel; the default capacity has its own test
        out, lengths = _encode_c(dev, imgs, quality, cap)
        assert max(lengths) <= cap
        _check_against_pillow(imgs, quality, out, lengths, ("C", quality, names))
        if len(names) > 1 and H * W >= 256:  # (the 1 x 1 and 8 x 8 images of a batch can all take the same few bytes)
            assert len(set(lengths)) > 1, "the batch should mix lengths"
        out2, lengths2 = _encode_py(dev, imgs, quality, cap)
        assert lengths2 == lengths and all(np.array_equal(out2[i, :lengths[i]], out[i, :lengths[i]]) for i in range(len(names)))
        out3, lengths3 = _encode_c(dev, imgs, quality, cap, shift=1)  # an unaligned image pointer: the byte-wise loads (also taken when W % 16 != 0)
        assert lengths3 == lengths and all(np.array_equal(out3[i, :lengths[i]], out[i, :lengths[i]]) for i in range(len(names)))


def test_default_capacity_and_whole_files(dev):
    imgs = np.stack([jc.make_image(f, 40, 56)[0] for f in ("blur", "flat", "noise")])
    out, lengths = _encode_py(dev, imgs, 75)
    assert out.shape == (3, 48 * 64)
    _check_against_pillow(imgs, 75, out, lengths, "default capacity")
    files = io_formats.encode_jpegs_device(torch.from_numpy(imgs).to(dev))
    assert files == [jc.pillow_bytes(im) for im in imgs]
    # a CPU tensor and a one-channel batch go wholly to Pillow: the same bytes as save_jpeg writes
    assert io_formats.encode_jpegs_device(torch.from_numpy(imgs)) == files
    grey = torch.from_numpy(imgs[..., :1].copy())
    assert io_formats.encode_jpegs_device(grey.to(dev)) == [jc.pillow_bytes(imgs[i, ..., 0]) for i in range(3)]


def test_scans_span_several_workgroups(dev):
    """272 x 528 noise: 561 MCUs = 3366 blocks (fourteen tiles of the offset scan) and a stream of many 2 KiB chunks"""
    img = jc.make_image("noise", 272, 528)[0][None]
    out, lengths = _encode_c(dev, img, 75, 2 * 272 * 528)
    assert lengths[0] > 40 * 2048
    _check_against_pillow(img, 75, out, lengths, "272x528")


def test_batch_of_three_256(dev):
    imgs = np.stack([jc.make_image(f, 256, 256)[0] for f in ("blur", "noise", "saturated")])
    out, lengths = _encode_c(dev, imgs, 75, 3 * 256 * 256)
    _check_against_pillow(imgs, 75, out, lengths, "3x256x256")
    out2, lengths2 = _encode_py(dev, imgs[:1], 75)  # the default capacity holds a smooth 256 x 256 image
    _check_against_pillow(imgs[:1], 75, out2, lengths2, "256x256 default capacity")


def test_bytes_do_not_depend_on_the_batch(dev):
    imgs = np.stack([jc.make_image(f, 33, 47)[0] for f in ("blur", "noise", "saturated", "flat")])
    cap = 3 * 48 * 48
    full, lens = _encode_c(dev, imgs, 75, cap)
    for i in range(4):
        alone, l1 = _encode_c(dev, imgs[i:i + 1], 75, cap)
        first, l2 = _encode_c(dev, np.concatenate([imgs[i:i + 1], imgs[:2]]), 75, cap)
        last, l3 = _encode_c(dev, np.concatenate([imgs[2:], imgs[i:i + 1]]), 75, cap)
        assert l1[0] == l2[0] == l3[-1] == lens[i]
        ref = full[i, :lens[i]]
        assert np.array_equal(alone[0, :lens[i]], ref) and np.array_equal(first[0, :lens[i]], ref) and np.array_equal(last[-1, :lens[i]], ref)


def test_capacity_64_keeps_the_true_length(dev):
    img = jc.make_image("noise", 40, 56)[0][None]
    head, body = jc.split_pillow(jc.pillow_bytes(img[0]))
    out, lengths = _encode_c(dev, img, 75, 64)  # (its own guards prove that nothing lands at or beyond byte 64)
    assert lengths == [len(body)] and len(body) > 64
    assert out[0].tobytes() == body[:64]
    for cap in (1, 63, 65):  # EOI and stuffed bytes cut anywhere
        o, l = _encode_c(dev, img, 75, cap)
        assert l == [len(body)] and o[0].tobytes() == body[:cap]
    files = io_formats.encode_jpegs_device(torch.from_numpy(img).to(dev), capacity=64)
    assert files == [head + body]
    # a capacity that cuts inside the trailer: the length says so, the fallback still gives the file
    for cap in (len(body) - 1, len(body), len(body) + 1):
        o, l = _encode_c(dev, img, 75, cap)
        assert l == [len(body)] and o[0, :min(cap, len(body))].tobytes() == body[:cap]
        assert io_formats.encode_jpegs_device(torch.from_numpy(img).to(dev), capacity=cap) == [head + body]


def test_refusals_come_before_any_launch(dev):
    L = hip.lib()
    N, H, W, cap = 2, 16, 16, 512
    need = L.lfm_jpeg_encode_workspace_bytes(N, H, W, cap)
    img = torch.zeros(N * H * W * 3, dtype=torch.uint8, device=dev)
    ws = torch.full((need + 16,), SENTINEL, dtype=torch.uint8, device=dev)
    out = torch.full((N * cap,), SENTINEL, dtype=torch.uint8, device=dev)
    lens = torch.full((N + 1,), -77, dtype=torch.int32, device=dev)
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + off)  # noqa: E731
    st = hip.stream_ptr(dev)
    ARG, SHAPE, ALIGN, WORKSPACE = -5, -1, -2, -3

    def call(img_p=P(img), n=N, h=H, w=W, q=75, c=cap, ws_p=P(ws), ws_bytes=need, out_p=P(out), len_p=P(lens)):
        return L.lfm_jpeg_encode_rgb8(img_p, n, h, w, q, c, ws_p, ws_bytes, out_p, len_p, st)

    null = C.c_void_p(0)
    assert call(img_p=null) == ARG and call(ws_p=null) == ARG and call(out_p=null) == ARG and call(len_p=null) == ARG
    assert call(q=0) == ARG and call(q=101) == ARG
    assert call(h=0) == SHAPE and call(w=4097) == SHAPE and call(n=0) == SHAPE and call(c=0) == SHAPE and call(h=4097) == SHAPE and call(w=0) == SHAPE
    assert call(ws_bytes=need - 1) == WORKSPACE
    assert call(ws_p=P(ws, 8)) == ALIGN
    assert call(len_p=P(lens, 2)) == ALIGN
    for bad in ((0, H, W, cap), (N, 0, W, cap), (N, H, 4097, cap), (N, H, W, 0)):
        assert L.lfm_jpeg_encode_workspace_bytes(*bad) == 0
    torch.cuda.synchronize()
    assert bool((ws == SENTINEL).all()) and bool((out == SENTINEL).all()) and bool((lens == -77).all()), "a refused call wrote something"
    assert call() == 0
    with pytest.raises(hip.LfmHipError, match="contiguous uint8"):
        hip.jpeg_encode(img.view(N, H, W, 3).float())
    with pytest.raises(hip.LfmHipError, match=r"\(code -5\)"):
        hip.jpeg_encode(img.view(N, H, W, 3), quality=0)
    with pytest.raises(hip.LfmHipError, match="unsupported shape"):
        hip.jpeg_encode(torch.zeros(1, 1, 4097, 3, dtype=torch.uint8, device=dev))
    torch.cuda.synchronize()


def test_captured_replay_follows_rewritten_pixels(dev):
    a, b = jc.make_image("blur", 40, 56)[0], jc.make_image("saturated", 40, 56)[0]
    d = torch.from_numpy(a[None].copy()).to(dev)
    cap = 3 * 48 * 64
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        hip.jpeg_encode(d, capacity=cap)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out, lengths = hip.jpeg_encode(d, capacity=cap)
    for img in (a, b, a):
        d.copy_(torch.from_numpy(img[None].copy()).to(dev))
        graph.replay()
        torch.cuda.synchronize()
        _check_against_pillow(img[None], 75, out.cpu().numpy(), lengths.tolist(), "replay")
