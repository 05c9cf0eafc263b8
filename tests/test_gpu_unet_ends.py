"""GPU: the two layers through which every UNet evaluation, every VAE encode and every VAE decode enters and leaves fp16, per element against float64
(cases, references, emulations and the derivation of the bounds: tests/unet_ends_cases.py; that the yardsticks tell right from wrong:
tests/test_unet_ends_ref.py).

  lfm_conv3x3_in_f32   fp32 NCHW (Cin <= 16) -> fp16 NHWC on conv_in_mfma_kernel (hi / lo fp16 planes, three MFMAs per k-step) and on conv_in_kernel
                       (flag UNET_CONV_IN_SCALAR, and every width the MFMA kernel does not take): an all-border map, a single row, ragged 64-pixel
                       chunks, workgroups that walk a second chunk, the zero-padded k range, Cin 3 / 4 / 8 / 9 / 16
  lfm_conv3x3_out_f32  fp16 NHWC -> fp32 NCHW (1..4 channels) on conv3x3_halo_out_kernel (flag CONV_HALO_SMALL below 256 tiles; the production gate at
                       256) and on the implicit GEMM with EpiNCHWF32 (a map that is not 16-aligned; flag CONV_IMPLICIT_GEMM): 2 / 4 / 6 quarters, the XCD
                       remap taken and not, border halos of images adjacent in memory, nch 1..4

Operands end in NaN guard elements (the pad entries of bias4 are NaN too), outputs lie between sentinel guard rows / planes that must survive; every
call runs twice and the two results are bit-equal.  Exact families are compared by equality (conv_in: with the one RNE rounding of the integer result to
fp16, and the two kernels with each other), real-valued families per element with the derived bound.

Measured on an MI355X (all of it: profiles/unet_ends_tests.txt; the bounds are derived, not taken from these):

  worst error / bound over the shapes (share of correctly rounded elements)     device                          CPU emulation
  conv_in  gauss   MFMA kernel                                                  0.869 .. 0.964 (>= 0.9974)      the same (>= 0.9969)
  conv_in  small   MFMA kernel: every lo operand an fp16 subnormal              0.748 .. 0.964 (>= 0.9844)      the same
  conv_in  tiny    MFMA kernel: the hi plane of x subnormal                     0.533 .. 0.723 (>= 0.8626)      the same
  conv_in  gauss / small / tiny   scalar kernel                                 0.807 .. 0.984 (>= 0.9990)      the same
  conv_out gauss   halo kernel / implicit GEMM                                  0.0005 .. 0.0030 / 0.0021       0.0023 .. 0.0083
  every integer family, both operations, every kernel: bit-exact; the matrix cores keep fp16 subnormal operands: no kernel change was needed.
The conv_in ratios near 1 are the fp16 store itself (2^-11 |ref| of the bound)."""
import ctypes as C

import pytest
import torch

import gemm_exact_cases as gc
import unet_ends_cases as uc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
G = gc.GUARD
ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -5


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


class flags:
    """lfm_gemm_select(flags << 4) for the block, the defaults afterwards (also when the block raises)."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        hip.gemm_select(self.value << 4)

    def __exit__(self, *exc):
        hip.gemm_select(0)


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


def bits(t):
    return t.view(torch.int16 if t.dtype == F16 else torch.int32)


def assert_bound(got, ref, bound, what):
    """|got - ref| <= bound per element (a NaN fails); returns the comparison (worst ratio, bit-exact share)."""
    r = uc.compare(got, ref, bound)
    assert r.bad == 0, f"{what}: {r.bad} of {ref.numel()} elements beyond the bound, worst {r.worst:.2f} x; first (position, got, expected) {r.first}"
    return r


# ------------------------------------------------------------------------------------------------ conv_in
def conv_in_once(dev, ops, c, scalar):
    buf = gc.out_buffer(G + c.M, c.Cout, c.Cout, F16).to(dev)  # G sentinel rows, the [M, Cout] block, G sentinel rows
    with flags(hip.DBG_UNET_CONV_IN_SCALAR if scalar else 0):
        rc = hip.lib().lfm_conv3x3_in_f32(*[hip.ptr(t) for t in ops], hip.ptr(buf[G:]), c.N, c.H, c.W, c.Cin, c.Cout, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    buf = buf.cpu()
    return torch.cat([buf[G:], buf[:G]])  # the block first, all guard rows after it: the layout gc.assert_exact and gc.touched_positions look at


def run_conv_in(dev, c, scalar):
    """The output buffer (block first, guard rows after) of lfm_conv3x3_in_f32; x, w and bias end in NaN guard elements; two runs, bit-equal."""
    ops = [gc.embed_vec(t.reshape(-1)).to(dev) for t in (c.x, c.w, c.b)]
    first, again = conv_in_once(dev, ops, c, scalar), conv_in_once(dev, ops, c, scalar)
    assert torch.equal(bits(first), bits(again)), "two runs differ"
    return first


def kernels_of(shape):
    """The kernels a conv_in shape runs on: (name, flag set)."""
    return [("mfma", False), ("scalar", True)] if uc.mfma_takes(shape[3], shape[4]) else [("scalar", False)]


CIN_SHAPES = uc.CIN_MFMA_SHAPES + uc.CIN_SCALAR_SHAPES


def test_the_mfma_shapes_are_the_mfma_kernels():
    assert all(uc.mfma_takes(s[3], s[4]) for s in uc.CIN_MFMA_SHAPES) and not any(uc.mfma_takes(s[3], s[4]) for s in uc.CIN_SCALAR_SHAPES)


@pytest.mark.parametrize("shape", CIN_SHAPES, ids=ids)
@pytest.mark.parametrize("family", uc.CIN_EXACT)
def test_conv_in_exact(dev, family, shape):
    c = uc.conv_in_case(family, *shape)
    outs = {}
    for kernel, scalar in kernels_of(shape):
        outs[kernel] = run_conv_in(dev, c, scalar)
        gc.assert_exact(outs[kernel], c.ref16, c.M, c.Cout, f"conv_in {family} {shape} {kernel}")
    if len(outs) == 2:
        assert torch.equal(bits(outs["mfma"]), bits(outs["scalar"])), "the two kernels differ"
    print(f"EXACT conv_in {family} {shape} kernels {sorted(outs)}: largest |ref| {int(c.ref.abs().max())}")


@pytest.mark.parametrize("shape", CIN_SHAPES, ids=ids)
@pytest.mark.parametrize("family", uc.CIN_REAL)
def test_conv_in_vs_fp64(dev, family, shape):
    c = uc.conv_in_case(family, *shape)
    failures = []
    for kernel, scalar in kernels_of(shape):
        out = run_conv_in(dev, c, scalar)
        touched = gc.touched_positions(out, c.M, c.Cout)
        assert not touched, f"conv_in {family} {shape} {kernel}: {len(touched)} guard elements written; first {touched[:4]}"
        r = uc.compare(out[:c.M], c.ref, uc.conv_in_bound(c, kernel))
        print(f"MEASURED conv_in {family} {shape} {kernel}: worst error / bound {r.worst:.3f}, bit-exact share {r.exact_share:.4f}")
        if r.bad:
            failures.append(f"{kernel}: {r.bad} of {c.ref.numel()} elements beyond the bound, worst {r.worst:.2f} x; first (position, got, expected) {r.first}")
    assert not failures, f"conv_in {family} {shape}: " + " | ".join(failures)


# ------------------------------------------------------------------------------------------------ conv_out
def conv_out_once(dev, ops, c, flag):
    buf = uc.planes_buffer(c.N, c.nch, c.HW).to(dev)
    with flags(flag):
        rc = hip.lib().lfm_conv3x3_out_f32(*[hip.ptr(t) for t in ops], hip.ptr(buf[uc.GUARD_PLANES:]), c.N, c.H, c.W, c.Cin, c.nch, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return buf.cpu()


def run_conv_out(dev, c, flag):
    """The planes buffer of lfm_conv3x3_out_f32: the fp16 input and w4 end in NaN guard rows, bias4 in NaN guard elements, its pad entries NaN as well (a
    pad channel that is stored anywhere shows); two runs, bit-equal."""
    b4 = c.b4.clone()
    b4[c.nch:] = float("nan")
    ops = [gc.embed(c.x, dtype=F16).to(dev), gc.embed(c.w4, dtype=F16).to(dev), gc.embed_vec(b4).to(dev)]
    first, again = conv_out_once(dev, ops, c, flag), conv_out_once(dev, ops, c, flag)
    assert torch.equal(bits(first), bits(again)), "two runs differ"
    return first


def halo_takes(N, H, W, flag):
    """csrc/conv_halo_kernel.h: launch_conv3x3_halo_out's gate, restated (Cin % 64 == 0 here)."""
    tiles = N * (H // 16) * (W // 16)
    return H % 16 == 0 and W % 16 == 0 and not flag & hip.DBG_CONV_IMPLICIT_GEMM and (tiles >= 256 or bool(flag & hip.DBG_CONV_HALO_SMALL))


def check_conv_out(dev, family, shape, flag, path):
    c = uc.conv_out_case(family, *shape)
    assert halo_takes(c.N, c.H, c.W, flag) == (path == "halo")
    buf = run_conv_out(dev, c, flag)
    rows = c.N * c.nch
    touched = uc.touched_planes(buf, rows)
    what = f"conv_out {family} {shape} {path}"
    assert not touched, f"{what}: {len(touched)} guard-plane elements written; first (plane, pixel) {touched[:4]}"
    r = assert_bound(buf[uc.GUARD_PLANES:uc.GUARD_PLANES + rows], c.ref, c.bound, what)  # bound None: equality
    print(f"{'EXACT' if c.exact else 'MEASURED'} conv_out {family} {shape} {path}: worst error / bound {r.worst:.4f}, bit-exact share {r.exact_share:.4f}")


@pytest.mark.parametrize("shape", uc.COUT_HALO_SHAPES, ids=ids)
@pytest.mark.parametrize("family", ("int", "gauss"))
def test_conv_out_halo(dev, family, shape):
    check_conv_out(dev, family, shape, 0 if shape == uc.COUT_BIG else hip.DBG_CONV_HALO_SMALL, "halo")


@pytest.mark.parametrize("shape,flag", list(zip(uc.COUT_GEMM_SHAPES, (0, hip.DBG_CONV_IMPLICIT_GEMM))), ids=ids)
@pytest.mark.parametrize("family", ("int", "gauss"))
def test_conv_out_implicit_gemm(dev, family, shape, flag):
    check_conv_out(dev, family, shape, flag, "gemm")


# ------------------------------------------------------------------------------------------------ refusals: before any launch, the output untouched
def off(t, nbytes):
    return C.c_void_p(t.data_ptr() + nbytes)


def test_conv_in_refusals(dev):
    """Buffers large enough for every shape asked for (a refusal that failed would stay in bounds); no misaligned pointer goes through a kernel: every
    call here must be refused."""
    L = hip.lib()
    x, w, b = torch.zeros(17 * 16 + 8, device=dev), torch.zeros(320 * 17 * 9 + 8, device=dev), torch.zeros(320 + 8, device=dev)
    out = torch.full((16 * 320 + 64,), gc.SENTINEL, dtype=F16, device=dev)
    px, pw, pb, po, st = hip.ptr(x), hip.ptr(w), hip.ptr(b), hip.ptr(out), hip.stream_ptr()
    null = C.c_void_p(0)

    def call(x_=px, w_=pw, b_=pb, o_=po, Cin=4, Cout=64):
        return L.lfm_conv3x3_in_f32(x_, w_, b_, o_, 1, 4, 4, Cin, Cout, st)

    for scalar in (False, True):
        with flags(hip.DBG_UNET_CONV_IN_SCALAR if scalar else 0):
            assert [call(x_=null), call(w_=null), call(b_=null), call(o_=null)] == [ERR_ARG] * 4
            assert [call(Cin=0), call(Cin=17), call(Cout=60), call(Cout=68), call(Cout=0), call(Cout=-8)] == [ERR_SHAPE] * 6
            assert L.lfm_conv3x3_in_f32(px, pw, pb, po, 0, 4, 4, 4, 64, st) == ERR_SHAPE
            # what the scalar kernel cannot take: its 16-byte stores to out, its 16-byte loads from bias
            assert [call(o_=off(out, 8), Cout=96), call(o_=off(out, 2), Cout=96), call(b_=off(b, 4), Cout=96), call(b_=off(b, 8), Cout=320)] == [ERR_ALIGN] * 4
            # an MFMA width: out must be 8-byte aligned there and bias 16-byte, else the scalar kernel is asked and refuses
            assert [call(o_=off(out, 4)), call(o_=off(out, 2)), call(b_=off(b, 4)), call(b_=off(b, 8))] == [ERR_ALIGN] * 4
    with flags(hip.DBG_UNET_CONV_IN_SCALAR):  # the 8-byte rule is the MFMA kernel's own: on the scalar path the same pointer is refused
        assert call(o_=off(out, 8)) == ERR_ALIGN
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())


def test_conv_out_refusals(dev):
    L = hip.lib()
    x, w4, b4 = torch.zeros(16 * 16 * 128, dtype=F16, device=dev), torch.zeros(4 * 9 * 128, dtype=F16, device=dev), torch.zeros(4, device=dev)
    out = torch.full((6 * 16 * 16,), gc.SENTINEL, device=dev)
    px, pw, pb, po, st = hip.ptr(x), hip.ptr(w4), hip.ptr(b4), hip.ptr(out), hip.stream_ptr()
    null = C.c_void_p(0)

    def call(x_=px, w_=pw, b_=pb, o_=po, N=1, Cin=64, nch=3):
        return L.lfm_conv3x3_out_f32(x_, w_, b_, o_, N, 16, 16, Cin, nch, st)

    for flag in (0, hip.DBG_CONV_HALO_SMALL, hip.DBG_CONV_IMPLICIT_GEMM):
        with flags(flag):
            assert [call(x_=null), call(w_=null), call(b_=null), call(o_=null)] == [ERR_ARG] * 4
            assert [call(nch=0), call(nch=5), call(Cin=32), call(Cin=96), call(Cin=100), call(N=0)] == [ERR_SHAPE] * 6
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())
