"""GPU: the four NHWC glue ops of the UNets that only whole networks reached -- lfm_avgpool2_f16, lfm_upsample2_f16, lfm_add_image_vec_f16 and
lfm_concat_channels_f16 -- called directly, per element, in guarded buffers (NaN guard rows after operands, the sentinel after outputs).

upsample and concat are copies: bit-identical to torch indexing on arbitrary fp16 data, the extremes 65504, +-0 and a subnormal included.  avgpool and
add_image_vec are exact on integer data (integers below 512 average to multiples of 1/4 below 512; integer sums up to 2000) and round ONCE on Gaussian
data: at most one fp16 ulp from the fp16 rounding of the float64 result.

Shapes: C = 8 (one octet per pixel) and 24, non-square maps, N = 3, thread counts that are no multiple of the 256-thread block, below and above one block."""
import pytest
import torch

import gemm_exact_cases as gc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
N = 3
# (Ho, Wo, C) of the OUTPUT of avgpool (input 2Ho x 2Wo): 45, 108 and 1080 octets
POOL_SHAPES = [(3, 5, 8), (6, 2, 24), (12, 10, 24)]
# (Ho, Wo, C) of the OUTPUT of upsample (input Ho/2 x Wo/2): 180, 108 and 540 octets
UP_SHAPES = [(6, 10, 8), (6, 2, 24), (6, 10, 24)]
VEC_SHAPES = [(15, 8), (12, 24), (120, 24)]  # (HW, C)
CAT_SHAPES = [(45, 8, 24), (36, 24, 8), (360, 24, 16)]  # (pixels, Ca, Cb): Ca != Cb
SPECIALS = [65504.0, -65504.0, 0.0, -0.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -14, 1.0]  # fp16 extremes, both zeros, the smallest subnormal, the smallest normal


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def arbitrary_f16(g, rows, cols):
    """Gaussian fp16 rows with the special values planted at the start, the end and in between."""
    t = torch.randn(rows, cols, generator=g).half().reshape(-1)
    s = torch.tensor(SPECIALS, dtype=F16)
    for at in (0, t.numel() // 2, t.numel() - len(SPECIALS)):
        t[at:at + len(SPECIALS)] = s
    return t.reshape(rows, cols)


def ordinal(h):
    """fp16 -> integers in value order (+-0 -> 0): the distance of two values in ulps is the difference."""
    i = h.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def assert_bits(buf, ref, what):
    """buf [M + GUARD, C] holds exactly the bits of ref [M, C] (fp16), its guard rows the sentinel."""
    buf, (M, C_) = buf.cpu(), ref.shape
    same = buf[:M].view(torch.int16) == ref.contiguous().view(torch.int16)
    assert bool(same.all()), f"{what}: {int((~same).sum())} of {same.numel()} elements differ in bits; first {(~same).nonzero()[:4].tolist()}"
    assert not gc.touched_positions(buf, M, C_), f"{what}: guard rows written"


def assert_one_rounding(buf, ref64, what):
    """At most one fp16 ulp from the fp16 rounding of the float64 result; returns the share of elements that are that rounding exactly."""
    buf, (M, C_) = buf.cpu(), ref64.shape
    assert bool(torch.isfinite(buf[:M]).all()), what
    d = (ordinal(buf[:M]) - ordinal(ref64.half())).abs()
    assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} elements more than one ulp from the rounded float64 result, worst {int(d.max())} ulps"
    assert not gc.touched_positions(buf, M, C_), f"{what}: guard rows written"
    return float((d == 0).float().mean())


def run(fn, what, *args):
    rc = fn(*args, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (what, rc)


# ------------------------------------------------------------------------------------------------ copies
@pytest.mark.parametrize("Ho,Wo,Cc", UP_SHAPES)
def test_upsample2_is_a_copy(dev, Ho, Wo, Cc):
    g = torch.Generator().manual_seed(3 + Ho + 10 * Wo + Cc)
    x = arbitrary_f16(g, N * (Ho // 2) * (Wo // 2), Cc)
    ref = x.reshape(N, Ho // 2, Wo // 2, Cc)[:, torch.arange(Ho) // 2][:, :, torch.arange(Wo) // 2].reshape(N * Ho * Wo, Cc)
    dx, out = gc.embed(x).to(dev), gc.out_buffer(N * Ho * Wo, Cc, Cc, F16).to(dev)
    run(hip.lib().lfm_upsample2_f16, "upsample2", hip.ptr(dx), hip.ptr(out), N, Ho, Wo, Cc)
    assert_bits(out, ref, f"upsample2 ({N}, {Ho}, {Wo}, {Cc})")


@pytest.mark.parametrize("pixels,Ca,Cb", CAT_SHAPES)
def test_concat_channels_is_a_copy(dev, pixels, Ca, Cb):
    g = torch.Generator().manual_seed(5 + pixels + Ca)
    a, b = arbitrary_f16(g, pixels, Ca), arbitrary_f16(g, pixels, Cb)
    da, db, out = gc.embed(a).to(dev), gc.embed(b).to(dev), gc.out_buffer(pixels, Ca + Cb, Ca + Cb, F16).to(dev)
    run(hip.lib().lfm_concat_channels_f16, "concat", hip.ptr(da), hip.ptr(db), hip.ptr(out), pixels, Ca, Cb)
    assert_bits(out, torch.cat([a, b], 1), f"concat ({pixels}, {Ca} | {Cb})")


# ------------------------------------------------------------------------------------------------ one rounding
def pool64(x, Ho, Wo, Cc):
    v = x.double().reshape(N, Ho, 2, Wo, 2, Cc)
    return (v.sum((2, 4)) / 4).reshape(N * Ho * Wo, Cc)


@pytest.mark.parametrize("Ho,Wo,Cc", POOL_SHAPES)
def test_avgpool2_exact_and_one_rounding(dev, Ho, Wo, Cc):
    g = torch.Generator().manual_seed(7 + Ho + 10 * Wo + Cc)
    M = N * Ho * Wo
    out = gc.out_buffer(M, Cc, Cc, F16).to(dev)
    xi = gc.randint(g, (4 * M, Cc), 511)  # sums of four below 2048: the mean is a multiple of 1/4 below 512, exact in fp16
    ref = pool64(xi, Ho, Wo, Cc)
    assert float(ref.abs().max()) < 512 and bool((ref * 4 == (ref * 4).round()).all())
    run(hip.lib().lfm_avgpool2_f16, "avgpool2", hip.ptr(gc.embed(xi, dtype=F16).to(dev)), hip.ptr(out), N, Ho, Wo, Cc)
    gc.assert_exact(out, ref, M, Cc, f"avgpool2 exact ({N}, {Ho}, {Wo}, {Cc})")
    xg = torch.randn(4 * M, Cc, generator=g).half()
    out.fill_(gc.SENTINEL)
    run(hip.lib().lfm_avgpool2_f16, "avgpool2", hip.ptr(gc.embed(xg).to(dev)), hip.ptr(out), N, Ho, Wo, Cc)
    share = assert_one_rounding(out, pool64(xg, Ho, Wo, Cc), f"avgpool2 gauss ({N}, {Ho}, {Wo}, {Cc})")
    print(f"avgpool2 ({N},{Ho},{Wo},{Cc}): exact; gauss: {100 * share:.1f} % are the rounded float64 result, the rest one ulp off")


@pytest.mark.parametrize("HW,Cc", VEC_SHAPES)
def test_add_image_vec_exact_and_one_rounding(dev, HW, Cc):
    g = torch.Generator().manual_seed(9 + HW + Cc)
    M, stride = N * HW, Cc + 8  # e rows in a wider buffer whose pad columns hold NaN
    out = gc.out_buffer(M, Cc, Cc, F16).to(dev)
    for name, x, e in (("exact", gc.randint(g, (M, Cc), 1000).double(), gc.randint(g, (N, Cc), 1000).double()),
                       ("gauss", torch.randn(M, Cc, generator=g).half().double(), torch.randn(N, Cc, generator=g).double())):
        ref = x + e.float().double().repeat_interleave(HW, 0)  # e is fp32 on the device
        dx, de = gc.embed(x, dtype=F16).to(dev), gc.embed(e, stride, dtype=F32).to(dev)
        out.fill_(gc.SENTINEL)
        run(hip.lib().lfm_add_image_vec_f16, "add_image_vec", hip.ptr(dx), hip.ptr(de), stride, hip.ptr(out), N, HW, Cc)
        what = f"add_image_vec {name} ({N}, {HW}, {Cc}) e_stride {stride}"
        if name == "exact":
            assert float(ref.abs().max()) <= gc.CAP16
            gc.assert_exact(out, ref, M, Cc, what)
        else:
            share = assert_one_rounding(out, ref, what)
            print(f"{what}: {100 * share:.1f} % are the rounded float64 result, the rest one ulp off")


# ------------------------------------------------------------------------------------------------ refusals
def test_glue_ops_refuse_before_any_launch(dev):
    L, st = hip.lib(), hip.stream_ptr()
    x = torch.zeros(4096, dtype=F16, device=dev)
    e = torch.zeros(256, dtype=F32, device=dev)
    out = torch.full((4096,), gc.SENTINEL, dtype=F16, device=dev)
    p, pe, o = hip.ptr(x), hip.ptr(e), hip.ptr(out)
    SHAPE, ARG = -1, -5
    assert L.lfm_avgpool2_f16(p, o, 1, 2, 2, 12, st) == SHAPE and L.lfm_upsample2_f16(p, o, 1, 2, 2, 12, st) == SHAPE  # C % 8
    assert L.lfm_add_image_vec_f16(p, pe, 12, o, 1, 4, 12, st) == SHAPE
    assert L.lfm_concat_channels_f16(p, p, o, 4, 12, 8, st) == SHAPE and L.lfm_concat_channels_f16(p, p, o, 4, 8, 12, st) == SHAPE
    assert L.lfm_upsample2_f16(p, o, 1, 3, 2, 8, st) == SHAPE and L.lfm_upsample2_f16(p, o, 1, 2, 5, 8, st) == SHAPE  # odd output sizes
    assert L.lfm_avgpool2_f16(p, o, 0, 2, 2, 8, st) == SHAPE and L.lfm_concat_channels_f16(p, p, o, 0, 8, 8, st) == SHAPE
    assert L.lfm_avgpool2_f16(None, o, 1, 2, 2, 8, st) == ARG and L.lfm_avgpool2_f16(p, None, 1, 2, 2, 8, st) == ARG
    assert L.lfm_upsample2_f16(None, o, 1, 2, 2, 8, st) == ARG and L.lfm_upsample2_f16(p, None, 1, 2, 2, 8, st) == ARG
    assert L.lfm_add_image_vec_f16(None, pe, 8, o, 1, 4, 8, st) == ARG and L.lfm_add_image_vec_f16(p, None, 8, o, 1, 4, 8, st) == ARG
    assert L.lfm_add_image_vec_f16(p, pe, 8, None, 1, 4, 8, st) == ARG
    assert L.lfm_concat_channels_f16(None, p, o, 4, 8, 8, st) == ARG and L.lfm_concat_channels_f16(p, None, o, 4, 8, 8, st) == ARG
    assert L.lfm_concat_channels_f16(p, p, None, 4, 8, 8, st) == ARG
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())
