"""CPU: the yardsticks of tests/test_gpu_unet_ends.py can tell right from wrong (cases, emulations, bounds: tests/unet_ends_cases.py).

  - the float64 references agree with torch.nn.functional.conv2d on a non-square map, the [4][9][Cin] weight packing included;
  - every exact builder's caps hold (each builder asserts them), and the correct emulations return the exact families bit for bit;
  - the correct emulations are inside the derived bound at every element of every real-valued family and shape (worst error / bound printed);
  - every named mistake is unequal (exact families) or outside the bound (real-valued ones) at one element or more, on the shapes named here."""
import pytest
import torch
import torch.nn.functional as F

import gemm_exact_cases as gc
import unet_ends_cases as uc

ALL_CIN_SHAPES = uc.CIN_MFMA_SHAPES + uc.CIN_SCALAR_SHAPES
COUT_SHAPES = uc.COUT_HALO_SHAPES + uc.COUT_GEMM_SHAPES[:1]


def ids(v):
    return "x".join(map(str, v)) if isinstance(v, tuple) else str(v)


# ------------------------------------------------------------------------------------------------ references
def test_references_vs_conv2d_on_a_non_square_map():
    g = torch.Generator().manual_seed(1)
    N, H, W, Cin, Cout = 2, 5, 7, 3, 8
    x, w, b = gc.randint(g, (N, Cin, H, W), 9).double(), gc.randint(g, (Cout, Cin, 3, 3), 9).double(), gc.randint(g, (Cout,), 9).double()
    want = F.conv2d(x, w, b, padding=1)  # [N, Cout, H, W]
    assert torch.equal(uc.conv_in_ref(x, w, b).reshape(N, H, W, Cout).permute(0, 3, 1, 2), want)
    assert torch.equal((uc.im2col(x) @ w.reshape(Cout, -1).t() + b).reshape(N, H, W, Cout).permute(0, 3, 1, 2), want)  # k = c * 9 + tap
    # conv_out: NHWC rows in, NCHW planes out, w4 = [4][9][Cin] with k = tap * Cin + ci
    Cin, nch = 64, 3
    xr, w = gc.randint(g, (N * H * W, Cin), 9).double(), gc.randint(g, (nch, Cin, 3, 3), 9).double()
    b = gc.randint(g, (nch,), 9).double()
    want = F.conv2d(xr.reshape(N, H, W, Cin).permute(0, 3, 1, 2), w, b, padding=1)
    assert torch.equal(uc.conv_out_ref(xr, w, b, N, H, W).reshape(N, nch, H, W), want)
    w4 = uc.pack_w4(w)
    assert w4.shape == (4, 9 * Cin) and not bool(w4[nch:].any())
    assert float(w4[1, 5 * Cin + 17]) == float(w[1, 17, 1, 2])  # tap 5 = (ky 1, kx 2)
    rows = gc.conv_cols(xr, N, H, W, Cin, 0) @ w4.t()  # the library's k order
    assert torch.equal(rows[:, :nch].reshape(N, H * W, nch).permute(0, 2, 1).reshape(N, nch, H, W) + b.reshape(1, nch, 1, 1), want)
    assert not bool(rows[:, nch:].any())


# ------------------------------------------------------------------------------------------------ conv_in
@pytest.mark.parametrize("shape", ALL_CIN_SHAPES, ids=ids)
@pytest.mark.parametrize("family", uc.CIN_EXACT)
def test_conv_in_exact_caps_and_emulations(family, shape):
    c = uc.conv_in_case(family, *shape)  # asserts its caps
    assert torch.equal(uc.emulate_conv_in(c.x, c.w, c.b), c.ref16)
    assert torch.equal(uc.emulate_conv_in_scalar(c.x, c.w, c.b), c.ref16)
    print(f"EXACT conv_in {family} {shape}: largest |ref| {int(c.ref.abs().max())}, largest sum of |terms| {int(c.S.max())}")


@pytest.mark.parametrize("shape", ALL_CIN_SHAPES, ids=ids)
@pytest.mark.parametrize("family", uc.CIN_REAL)
def test_conv_in_emulations_inside_the_bound(family, shape):
    c = uc.conv_in_case(family, *shape)
    m = uc.compare(uc.emulate_conv_in(c.x, c.w, c.b).half(), c.ref, uc.conv_in_bound(c, "mfma"))
    s = uc.compare(uc.emulate_conv_in_scalar(c.x, c.w, c.b).half(), c.ref, uc.conv_in_bound(c, "scalar"))
    print(f"EMULATED conv_in {family} {shape}: worst error / bound mfma {m.worst:.3f} scalar {s.worst:.3f}; bit-exact share mfma {m.exact_share:.4f} scalar {s.exact_share:.4f}")
    assert m.bad == 0 and s.bad == 0, (m.first, s.first)
    assert bool((uc.conv_in_bound(c, "scalar") <= uc.conv_in_bound(c, "mfma")).all())  # the scalar kernel is held to the narrower bound


def conv_in_caught(mistake, family, shape):
    """Elements at which the MFMA emulation with `mistake` is unequal (exact family) or outside the MFMA bound (real-valued family)."""
    c = uc.conv_in_case(family, *shape)
    got = uc.emulate_conv_in(c.x, c.w, c.b, mistake)
    return uc.compare(got, c.ref16, None).bad if c.exact else uc.compare(got, c.ref, uc.conv_in_bound(c, "mfma")).bad


SMALL_MAPS = [s for s in uc.CIN_MFMA_SHAPES if s != uc.CIN_BIG]


@pytest.mark.parametrize("shape", uc.CIN_MFMA_SHAPES, ids=ids)
def test_a_dropped_plane_changes_the_exact_output(shape):
    """x_planes / w_planes: every operand of the one kind needs both planes and the hi planes cancel -- at every shape, the all-border ones included."""
    n = conv_in_caught("x_lo_dropped", "x_planes", shape), conv_in_caught("w_lo_dropped", "w_planes", shape)
    print(f"CAUGHT conv_in {shape}: x_lo_dropped at {n[0]} elements of x_planes, w_lo_dropped at {n[1]} of w_planes")
    assert n[0] > 0 and n[1] > 0
    # and the plane that the family does not exercise is all zeros there: dropping it changes nothing (the two families are both needed)
    assert conv_in_caught("w_lo_dropped", "x_planes", shape) == 0 and conv_in_caught("x_lo_dropped", "w_planes", shape) == 0


@pytest.mark.parametrize("shape", [s for s in SMALL_MAPS if s[1] * s[2] > 1], ids=ids)
def test_flushed_lo_subnormals_leave_the_bound_of_the_small_family(shape):
    """(1, 1, 1, 4, 64) is left out: 64 sums of 4 terms, too few for one to come out small against its own fp16 ulp; the shapes here all show it."""
    n = conv_in_caught("lo_subnormals_flushed", "small", shape)
    print(f"CAUGHT conv_in {shape}: lo_subnormals_flushed at {n} elements of small")
    assert n > 0
    assert conv_in_caught("lo_subnormals_flushed", "x_planes", shape) == 0  # the integer planes are normal numbers: only `small` sees a flush


def test_dropped_planes_leave_the_bound_of_the_real_families():
    """The real-valued families see a dropped plane too, where a sum comes out small against its terms: asserted at (3, 5, 7, 9, 192)."""
    shape = (3, 5, 7, 9, 192)
    for mistake in ("x_lo_dropped", "w_lo_dropped"):
        n = {f: conv_in_caught(mistake, f, shape) for f in ("gauss", "small")}
        print(f"CAUGHT conv_in {shape}: {mistake} at {n}")
        assert all(v > 0 for v in n.values()), (mistake, n)
    # (not `tiny`: below 2^-13 hi is already on the subnormal grid of 2^-24 and lo, on the same grid, is zero -- that family measures the floor itself)


# mistake -> the listed shapes that can show it (the others cannot: the reason)
STRUCTURAL = {
    "taps_transposed": [s for s in uc.CIN_MFMA_SHAPES if s[1] * s[2] > 1],  # a 1 x 1 map has the centre tap only
    "hw_exchanged": [s for s in uc.CIN_MFMA_SHAPES if s[1] != s[2]],  # a square map reads the same
    # Kp == KK at Cin 16; in the last image the padded k of x read what follows the tensor (a NaN guard on the GPU, nothing here): N >= 2
    "pad_k_not_zero": [s for s in uc.CIN_MFMA_SHAPES if s[3] * 9 % 16 and s[0] > 1],
    "border_wraps": [s for s in uc.CIN_MFMA_SHAPES if s[1] > 1 and s[2] > 1],  # row 0 has no previous row
}


@pytest.mark.parametrize("mistake", sorted(STRUCTURAL))
def test_structural_mistakes_of_conv_in_are_unequal(mistake):
    shapes = STRUCTURAL[mistake]
    assert shapes
    for shape in shapes:
        n = conv_in_caught(mistake, "int", shape)
        print(f"CAUGHT conv_in {shape}: {mistake} at {n} elements of int")
        assert n > 0, (mistake, shape)
    if mistake != "pad_k_not_zero":  # (the padded k meet zero lo planes and zero-sum weights in the other families)
        shape = shapes[0] if mistake != "border_wraps" else (3, 5, 7, 9, 192)
        assert conv_in_caught(mistake, "gauss", shape) > 0, (mistake, shape)


def test_every_conv_in_mistake_is_covered():
    covered = {"x_lo_dropped", "w_lo_dropped", "lo_subnormals_flushed"} | set(STRUCTURAL)
    assert covered == set(uc.CIN_MISTAKES)


# ------------------------------------------------------------------------------------------------ conv_out
def conv_out_result(c, mistake=None):
    """(elements of the block that are unequal / outside the bound, guard positions written, worst ratio) of the fp32 emulation."""
    buf = uc.emulate_conv_out(c.x, c.w4, c.b4, c.N, c.H, c.W, c.nch, mistake)
    rows = c.N * c.nch
    r = uc.compare(buf[uc.GUARD_PLANES:uc.GUARD_PLANES + rows], c.ref, c.bound)
    return r, uc.touched_planes(buf, rows)


@pytest.mark.parametrize("shape", COUT_SHAPES, ids=ids)
def test_conv_out_emulation_exact_and_inside_the_bound(shape):
    e, te = conv_out_result(uc.conv_out_case("int", *shape))
    g, tg = conv_out_result(uc.conv_out_case("gauss", *shape))
    print(f"EMULATED conv_out {shape}: int unequal {e.bad}; gauss worst error / bound {g.worst:.4f}, bit-exact share {g.exact_share:.4f}")
    assert e.bad == 0 and g.bad == 0 and not te and not tg


COUT_CAN_SHOW = {
    "pad_channel_stored": [s for s in uc.COUT_HALO_SHAPES if s[4] < 4 and s != uc.COUT_BIG],  # nch == 4 has no pad channel
    "neighbour_image_in_halo": [s for s in uc.COUT_HALO_SHAPES if s[0] > 1],  # one image has no neighbour
    "quarter_dropped": [s for s in uc.COUT_HALO_SHAPES if s != uc.COUT_BIG],
    "tap_major_vs_channel_major": [s for s in uc.COUT_HALO_SHAPES if s != uc.COUT_BIG],
}


@pytest.mark.parametrize("mistake", uc.COUT_MISTAKES)
def test_conv_out_mistakes_are_caught(mistake):
    shapes = COUT_CAN_SHOW[mistake]
    assert shapes
    for shape in shapes:
        for family in ("int", "gauss"):
            r, touched = conv_out_result(uc.conv_out_case(family, *shape), mistake)
            print(f"CAUGHT conv_out {shape} {family}: {mistake} at {r.bad} elements, {len(touched)} guard elements written")
            if mistake == "pad_channel_stored":
                # the spill into the next image's plane 0 may be overwritten by that image's own store; the last image's lands in the guard plane
                assert touched and all(m == c_rows(shape) for m, _ in touched), (shape, family)
            else:
                assert r.bad > 0 and not touched, (mistake, shape, family)


def c_rows(shape):
    return shape[0] * shape[4]
