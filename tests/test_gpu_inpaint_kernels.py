"""lfm_inpaint_prepare_u8, lfm_inpaint_cond_f32 and lfm_inpaint_composite_u8 (include/lfm_hip.h, csrc/inpaint.h) on the GPU.  prepare and composite bit for bit
against the fp32 restatement of the reference's op sequence (tests/inpaint_cases.py, pinned against the unmodified reference in tests/test_inpaint_ref.py) on
all 65 536 (image byte, mask byte) pairs and on 8x8, 8x24, 40x16, 64x64 at N = 1 and 3, through each of the three access variants the header names (chosen by
the base pointers' alignment), with sentinels around every output; the cond kernel per element against fp64 inside the derived bound; the three kernels
captured in one graph and replayed on inputs rewritten in place."""
import ctypes as C

import pytest
import torch

import inpaint_cases as ic
from lfm_amd import hip

pytestmark = pytest.mark.gpu

SENTINEL, BYTE_SENTINEL, GUARD = -1234.0, 0xA5, 32
# how far the byte / float base pointers are moved off their 256-byte aligned allocations, in elements: the 16-pixel variant where W % 16 == 0 (else the
# 8-pixel one); 8 bytes / 4 floats: the 8-pixel variant with 8-byte loads; 1 byte / 1 float: neither, one element per access
OFFSETS = {"aligned": (0, 0), "8-byte": (8, 4), "one element": (1, 1)}
INPUTS = dict(ic.gpu_inputs())
SCALE = 0.18215


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


class Guarded:
    """`numel` elements at element offset GUARD + off inside a buffer filled with a sentinel."""

    def __init__(self, dev, numel, dtype, off, fill):
        self.buf = torch.full((numel + 2 * GUARD + 16,), fill, dtype=dtype, device=dev)
        assert self.buf.data_ptr() % 256 == 0
        self.lo, self.hi, self.fill = GUARD + off, GUARD + off + numel, fill
        self.view = self.buf[self.lo:self.hi]

    def put(self, t):
        self.view.copy_(t.reshape(-1))
        return self

    def ptr(self):
        return C.c_void_p(self.view.data_ptr())

    def get(self, shape):
        host = self.buf.cpu()
        assert bool((host[:self.lo] == self.fill).all()) and bool((host[self.hi:] == self.fill).all()), "wrote outside the output"
        return host[self.lo:self.hi].reshape(shape).clone()


def run_prepare(dev, img, mask, want_image=True, offsets=(0, 0)):
    """-> (masked, image or None, the whole [N,5,h,w] conditioning tensor) on the host, every output checked for writes outside it."""
    N, H, W, _ = img.shape
    h, w = H // 8, W // 8
    ob, of = offsets
    dimg, dmask = Guarded(dev, img.numel(), torch.uint8, ob, 0).put(img), Guarded(dev, mask.numel(), torch.uint8, ob, 0).put(mask)
    masked, image = Guarded(dev, N * 3 * H * W, torch.float32, of, SENTINEL), Guarded(dev, N * 3 * H * W, torch.float32, of, SENTINEL)
    cond = Guarded(dev, N * 5 * h * w, torch.float32, min(of, 1), SENTINEL)  # mask_latent needs 4-byte alignment only
    rc = hip.lib().lfm_inpaint_prepare_u8(dimg.ptr(), dmask.ptr(), masked.ptr(), image.ptr() if want_image else None,
                                          C.c_void_p(cond.view.data_ptr() + 4 * h * w * 4), 5 * h * w, N, H, W, hip.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    got_image = image.get((N, 3, H, W))
    if not want_image:
        assert bool((got_image == SENTINEL).all())
    return masked.get((N, 3, H, W)), got_image if want_image else None, cond.get((N, 5, h, w))


def run_composite(dev, fake, img, mask, offsets=(0, 0)):
    N, H, W, _ = img.shape
    ob, of = offsets
    dimg, dmask = Guarded(dev, img.numel(), torch.uint8, ob, 0).put(img), Guarded(dev, mask.numel(), torch.uint8, ob, 0).put(mask)
    dfake = Guarded(dev, fake.numel(), torch.float32, of, 0.0).put(fake)
    out = Guarded(dev, img.numel(), torch.uint8, ob, BYTE_SENTINEL)
    rc = hip.lib().lfm_inpaint_composite_u8(dfake.ptr(), dimg.ptr(), dmask.ptr(), out.ptr(), N, H, W, hip.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    return out.get((N, H, W, 3))


@pytest.mark.parametrize("name", list(INPUTS))
def test_prepare_bit_for_bit(dev, name):
    img, mask, _ = INPUTS[name]
    image, _, masked, cc = ic.prepare32(img, mask)
    for label, offsets in OFFSETS.items():
        got_masked, got_image, cond = run_prepare(dev, img, mask, True, offsets)
        assert torch.equal(got_masked, masked), (name, label, "masked", int((got_masked != masked).sum()))
        assert torch.equal(got_image, image), (name, label, "image", int((got_image != image).sum()))
        assert torch.equal(cond[:, 4:], cc), (name, label, "mask on the latent grid")
        assert bool((cond[:, :4] == SENTINEL).all()), (name, label, "channels 0..3 of the conditioning tensor were written")
    got_masked, none, cond = run_prepare(dev, img, mask, False)  # image_nchw == NULL: nothing of it is written
    assert none is None and torch.equal(got_masked, masked) and torch.equal(cond[:, 4:], cc)


@pytest.mark.parametrize("name", list(INPUTS))
def test_composite_bit_for_bit(dev, name):
    img, mask, fake = INPUTS[name]
    ref = ic.composite_bytes32(fake, img, mask)
    for label, offsets in OFFSETS.items():
        got = run_composite(dev, fake, img, mask, offsets)
        assert torch.equal(got, ref), (name, label, int((got != ref).sum()))
    keep = mask == 255
    assert bool(keep.any()) and torch.equal(got[keep], img[keep])  # a pixel the mask keeps is the input byte
    hole = mask == 0
    assert torch.equal(got[hole], ic.save_image_bytes((fake + 1.0) / 2.0)[hole])  # a hole is the quantised sample


def test_composite_of_a_non_finite_sample_is_what_the_header_says(dev):
    img, mask = ic.make_bytes(1, 8, 8)
    mask[0, 0, :4] = torch.tensor([255, 255, 0, 0], dtype=torch.uint8)
    fake = torch.zeros(1, 3, 8, 8)
    fake[0, :, 0, 0], fake[0, :, 0, 1], fake[0, :, 0, 2], fake[0, :, 0, 3] = float("nan"), float("inf"), float("inf"), float("-inf")
    got = run_composite(dev, fake, img, mask)
    assert got[0, 0, :4].tolist() == [[0, 0, 0], [0, 0, 0], [255, 255, 255], [0, 0, 0]]  # NaN -> 0; inf * 0 = NaN under a keeping mask -> 0; +inf -> 255; -inf -> 0


def test_refusals_come_before_any_launch(dev):
    L = hip.lib()
    img, mask = ic.make_bytes(2, 16, 16)
    dimg, dmask = img.to(dev), mask.to(dev)
    f = torch.full((2 * 3 * 16 * 16 + 8,), SENTINEL, device=dev)
    cond = torch.full((2 * 5 * 4 + 8,), SENTINEL, device=dev)
    out = torch.full((2 * 16 * 16 * 3,), BYTE_SENTINEL, dtype=torch.uint8, device=dev)
    p, st = hip.ptr, hip.stream_ptr()
    odd = lambda t: C.c_void_p(t.data_ptr() + 2)  # noqa: E731  a float pointer that is not 4-byte aligned
    ARG, SHAPE, ALIGN = -5, -1, -2
    assert L.lfm_inpaint_prepare_u8(None, p(dmask), p(f), None, p(cond), 20, 2, 16, 16, st) == ARG
    assert L.lfm_inpaint_prepare_u8(p(dimg), p(dmask), p(f), None, None, 20, 2, 16, 16, st) == ARG
    assert L.lfm_inpaint_prepare_u8(p(dimg), p(dmask), p(f), None, p(cond), 20, 2, 16, 12, st) == SHAPE  # W % 8
    assert L.lfm_inpaint_prepare_u8(p(dimg), p(dmask), p(f), None, p(cond), 20, 0, 16, 16, st) == SHAPE
    assert L.lfm_inpaint_prepare_u8(p(dimg), p(dmask), p(f), None, p(cond), 3, 2, 16, 16, st) == SHAPE  # stride below the 4 values written per image
    assert L.lfm_inpaint_prepare_u8(p(dimg), p(dmask), odd(f), None, p(cond), 20, 2, 16, 16, st) == ALIGN
    assert L.lfm_inpaint_prepare_u8(p(dimg), p(dmask), p(f), None, odd(cond), 20, 2, 16, 16, st) == ALIGN
    assert L.lfm_inpaint_composite_u8(p(f), p(dimg), None, p(out), 2, 16, 16, st) == ARG
    assert L.lfm_inpaint_composite_u8(p(f), p(dimg), p(dmask), p(out), 2, 12, 16, st) == SHAPE
    assert L.lfm_inpaint_composite_u8(odd(f), p(dimg), p(dmask), p(out), 2, 16, 16, st) == ALIGN
    assert L.lfm_inpaint_cond_f32(None, None, SCALE, p(cond), 20, 2, 4, st) == ARG
    assert L.lfm_inpaint_cond_f32(p(f), None, SCALE, p(cond), 15, 2, 4, st) == SHAPE  # stride below 4 * hw
    assert L.lfm_inpaint_cond_f32(p(f), None, SCALE, p(cond), 20, 2, 0, st) == SHAPE
    assert L.lfm_inpaint_cond_f32(p(f), odd(f), SCALE, p(cond), 20, 2, 4, st) == ALIGN
    torch.cuda.synchronize()
    assert bool((f == SENTINEL).all()) and bool((cond == SENTINEL).all()) and bool((out == BYTE_SENTINEL).all())
    with pytest.raises(hip.LfmHipError, match="contiguous uint8"):
        hip.inpaint_prepare(dimg.float(), dmask, torch.empty(2, 5, 2, 2, device=dev))
    with pytest.raises(hip.LfmHipError, match="cond must be dense fp32"):
        hip.inpaint_prepare(dimg, dmask, torch.empty(2, 4, 2, 2, device=dev))
    with pytest.raises(hip.LfmHipError, match="multiples of 8"):
        hip.inpaint_composite(torch.empty(2, 3, 16, 12, device=dev), dimg[:, :, :12].contiguous(), dmask[:, :, :12].contiguous())


def run_cond(dev, moments, eps, off=0):
    N, _, h, w = moments.shape
    dm, out = Guarded(dev, moments.numel(), torch.float32, off, 0.0).put(moments), Guarded(dev, N * 5 * h * w, torch.float32, off, SENTINEL)
    de = Guarded(dev, N * 4 * h * w, torch.float32, off, 0.0).put(eps) if eps is not None else None
    rc = hip.lib().lfm_inpaint_cond_f32(dm.ptr(), de.ptr() if de else None, SCALE, out.ptr(), 5 * h * w, N, h * w, hip.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    cond = out.get((N, 5, h, w))
    assert bool((cond[:, 4] == SENTINEL).all()), "the mask channel was written"
    return cond[:, :4]


@pytest.mark.parametrize("N,h,w", [(1, 1, 1), (3, 3, 5), (2, 8, 8), (3, 32, 32)])  # hw = 1 and 15: one element per access; 64 and 1024: four
def test_cond_per_element_inside_the_bound(dev, N, h, w):
    moments, eps = ic.make_moments(N, h, w, extremes=True)  # logvar -40 and 25 among them: both clamps
    ref, bound = ic.cond64(moments, eps, SCALE), ic.cond_bound(moments, eps, SCALE)
    got = run_cond(dev, moments, eps)
    r = ic.error_ratio(got, ref, bound)
    print(f"BOUND inpaint_cond {N}x{h}x{w}: error / bound {r:.3f}")
    assert r <= 1.0
    assert torch.equal(run_cond(dev, moments, eps, off=1), got)  # the one-element variant: the same bits
    clamped = moments.clone()
    clamped[:, 4:].clamp_(-30.0, 20.0)
    assert not torch.equal(clamped, moments) and torch.equal(run_cond(dev, clamped, eps), got)  # beyond the clamps is at the clamps, bit for bit
    mode = run_cond(dev, moments, None)
    assert torch.equal(mode, ic.cond32(moments, None, SCALE))  # eps == NULL: mean * scale, one rounding, the very bits
    assert torch.equal(run_cond(dev, moments, torch.zeros_like(eps)), mode)  # eps == 0


def test_three_kernels_in_one_graph_follow_inputs_rewritten_in_place(dev):
    N, S, R = 3, 64, 8
    img, mask = ic.make_bytes(N, S, S, seed=1)
    fake = ic.make_fake_at_the_boundaries(img, mask, seed=1)
    moments, eps = ic.make_moments(N, R, R, seed=1)
    dimg, dmask, dfake, dmom, deps = (t.to(dev) for t in (img, mask, fake, moments, eps))
    cond, out = torch.zeros(N, 5, R, R, device=dev), torch.zeros(N, S, S, 3, dtype=torch.uint8, device=dev)
    masked = torch.zeros(N, 3, S, S, device=dev)
    L = hip.lib()

    def launch():
        s = hip.stream_ptr()
        assert L.lfm_inpaint_prepare_u8(hip.ptr(dimg), hip.ptr(dmask), hip.ptr(masked), None, C.c_void_p(cond.data_ptr() + 4 * R * R * 4), 5 * R * R, N, S, S, s) == 0
        assert L.lfm_inpaint_cond_f32(hip.ptr(dmom), hip.ptr(deps), SCALE, hip.ptr(cond), 5 * R * R, N, R * R, s) == 0
        assert L.lfm_inpaint_composite_u8(hip.ptr(dfake), hip.ptr(dimg), hip.ptr(dmask), hip.ptr(out), N, S, S, s) == 0

    def check(img, mask, fake, moments, eps):
        _, _, ref_masked, cc = ic.prepare32(img, mask)
        assert torch.equal(masked.cpu(), ref_masked) and torch.equal(cond[:, 4:].cpu(), cc)
        assert ic.error_ratio(cond[:, :4].cpu(), ic.cond64(moments, eps, SCALE), ic.cond_bound(moments, eps, SCALE)) <= 1.0
        assert torch.equal(out.cpu(), ic.composite_bytes32(fake, img, mask))

    launch()  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for t in (cond, out, masked):
        t.zero_()
    graph.replay()
    torch.cuda.synchronize()
    check(img, mask, fake, moments, eps)
    img2, mask2 = ic.make_bytes(N, S, S, seed=2)
    fake2 = ic.make_fake_at_the_boundaries(img2, mask2, seed=2)
    mom2, eps2 = ic.make_moments(N, R, R, seed=2)
    for d, t in ((dimg, img2), (dmask, mask2), (dfake, fake2), (dmom, mom2), (deps, eps2)):
        d.copy_(t.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert not torch.equal(mask2, mask)
    check(img2, mask2, fake2, mom2, eps2)
