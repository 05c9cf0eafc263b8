"""GPU: four stages of the first-stage VAE that only a whole decode / encode reached, each through a test entry point that runs the drivers' own host
code, per element against float64 (cases, references, bounds and their derivations: tests/vae_stage_cases.py; the references themselves and the
controls: tests/test_vae_stage_ref.py).

  conv_in     vae_conv_in_kernel: post_quant_conv folded into conv_in, all three pixels-per-block policies, ragged last blocks, all-border images
  downsample  VaeCtx::conv_down: ASrcConv gather mode 3 (stride 2 on the input padded (0, 1, 0, 1)) on the 128x128, 256x128 and 256x256 GEMM kernels
  moments     the encoder's conv_out: 8 live columns of a 128-column tile, EpiMomentsNCHW scattering a row tile over several images, fp32 out
  resnets     VaeCtx::resnet: identity and 1x1 shortcut, the rotation of the four buffers, statistics from the convolution epilogue or a pass of their
              own, and their hand-over from one resnet to the next (chain_stats)

Exact families are compared by equality, Gaussian families within the derived per-element bound, the resnets within 2 x the error of the float64 model
with the device's fp16 stores (the CPU test prints those errors; the ratios measured on an MI355X: profiles/vae_stage_tests.txt).  Operands end in NaN
guard rows, outputs in sentinel guard rows that must survive."""
import ctypes as C

import pytest
import torch

import gemm_exact_cases as gc
import vae_stage_cases as vc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


class selected:
    """lfm_gemm_select(kernel | flags << 4) for the block, the automatic choice afterwards (also when the block raises)."""

    def __init__(self, kernel, flags=0):
        self.which = kernel | (flags << 4)

    def __enter__(self):
        hip.gemm_select(self.which)

    def __exit__(self, *exc):
        hip.gemm_select(0)


def workspace(nbytes, dev):
    """0xFF bytes: NaN as fp16 and as fp32, so a read of anything the call did not write shows."""
    assert nbytes > 0
    return torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)


def assert_bound(buf, ref, bound, M, N, what, rows=None):
    """|got - ref| <= bound per element (a NaN fails), nothing written outside [0, M) x [0, N); returns the largest error / bound.  rows: a boolean
    mask -- only those rows are compared."""
    buf = buf.detach().cpu()
    ratio = (buf[:M, :N].double() - ref).abs() / bound
    if rows is not None:
        ratio = ratio[rows]
    bad = ~(ratio <= 1)
    touched = gc.touched_positions(buf, M, N)
    assert not bool(bad.any()), f"{what}: {int(bad.sum())} of {bad.numel()} elements beyond the bound, worst {float(ratio.nan_to_num(nan=float('inf')).max()):.2f} x; first {bad.nonzero()[:4].tolist()}"
    assert not touched, f"{what}: {len(touched)} elements outside [0, {M}) x [0, {N}) written; first {touched[:4]}"
    return float(ratio.max())


# ------------------------------------------------------------------------------------------------ conv_in
def run_conv_in(dev, c):
    ops = [gc.embed_vec(t.reshape(-1)).to(dev) for t in (c.pq_w, c.pq_b, c.cin_w, c.cin_b, c.z)]  # fp32, NaN after the last element
    out = gc.out_buffer(c.M, vc.CIN_OUT, vc.CIN_OUT, F16).to(dev)
    rc = hip.lib().lfm_vae_conv_in_f16(*[hip.ptr(t) for t in ops], hip.ptr(out), c.n, c.R, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


def pixels_per_block(pixels):
    return 256 if pixels >= 65536 else (64 if pixels >= 16384 else 16)


@pytest.mark.parametrize("n,R", vc.CONV_IN_SHAPES)
def test_conv_in_exact(dev, n, R):
    c = vc.conv_in_exact(n, R)
    out = run_conv_in(dev, c)
    gc.assert_exact(out, c.ref, c.M, vc.CIN_OUT, f"conv_in exact n={n} R={R}")
    ppb = pixels_per_block(c.M)
    print(f"EXACT conv_in n={n} R={R} pixels={c.M} pixels_per_block={ppb} last_block={c.M % ppb or ppb}")


@pytest.mark.parametrize("n,R", vc.CONV_IN_GAUSS_SHAPES)
def test_conv_in_gauss(dev, n, R):
    c = vc.conv_in_gauss(n, R)
    out = run_conv_in(dev, c)
    worst = assert_bound(out, c.ref, c.bound, c.M, vc.CIN_OUT, f"conv_in gauss n={n} R={R}")
    edge = vc.border_rows(n, R)
    worst_edge = assert_bound(out, c.ref, c.bound, c.M, vc.CIN_OUT, f"conv_in gauss n={n} R={R} border pixels", rows=edge)
    print(f"GAUSS conv_in n={n} R={R}: worst error / bound {worst:.3f} (border pixels {worst_edge:.3f})")


# ------------------------------------------------------------------------------------------------ downsample
def run_down(dev, c):
    dx, dW, dbias = gc.embed(c.x, dtype=F16).to(dev), gc.embed(c.Wt, dtype=F16).to(dev), gc.embed_vec(c.bias).to(dev)
    out = gc.out_buffer(c.M, c.Cout, c.Cout, F16).to(dev)
    L = hip.lib()
    ws = workspace(L.lfm_vae_downsample_workspace_bytes(c.N, c.H, c.W, c.Cin), dev)
    rc = L.lfm_vae_downsample_f16(hip.ptr(dx), hip.ptr(dW), hip.ptr(dbias), hip.ptr(out), hip.ptr(ws), ws.numel(), c.N, c.H, c.W, c.Cin, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("select", vc.DOWN_SELECT)
@pytest.mark.parametrize("n,Ho,Wo,Cc", vc.DOWN_SHAPES)
def test_downsample_exact(dev, n, Ho, Wo, Cc, select):
    c = vc.down_exact(n, Ho, Wo, Cc)
    last_row, last_col = vc.last_row_col(n, Ho, Wo)
    with selected(select):
        ran = hip.gemm_plan(c.M, Cc, 9 * Cc, caps=hip.GEMM_CAP_FITS)
        assert ran == (select or ran)
        out = run_down(dev, c)
    got = out[:c.M, :Cc].cpu().double()
    what = f"downsample exact select={select} kernel {ran} ({n}, {Ho}, {Wo}, {Cc})"
    for name, rows in (("last output row", last_row), ("last output column", last_col)):
        wrong = int((got[rows] != c.ref[rows].double()).sum())
        assert not wrong, f"{what}: {wrong} elements of the {name} differ (the gather beyond the bottom / right edge)"
    gc.assert_exact(out, c.ref, c.M, Cc, what, ran)
    print(f"EXACT downsample select={select} ran={ran} ({n},{Ho},{Wo},{Cc}) rows={c.M}")


@pytest.mark.parametrize("select", vc.DOWN_GAUSS_SELECT)
@pytest.mark.parametrize("n,Ho,Wo,Cc", vc.DOWN_SHAPES)
def test_downsample_gauss(dev, n, Ho, Wo, Cc, select):
    c = vc.down_gauss(n, Ho, Wo, Cc)
    last_row, last_col = vc.last_row_col(n, Ho, Wo)
    with selected(select):
        ran = hip.gemm_plan(c.M, Cc, 9 * Cc, caps=hip.GEMM_CAP_FITS)
        out = run_down(dev, c)
    what = f"downsample gauss select={select} kernel {ran} ({n}, {Ho}, {Wo}, {Cc})"
    r_row = assert_bound(out, c.ref, c.bound, c.M, Cc, what + " last output row", rows=last_row)
    r_col = assert_bound(out, c.ref, c.bound, c.M, Cc, what + " last output column", rows=last_col)
    worst = assert_bound(out, c.ref, c.bound, c.M, Cc, what)
    print(f"GAUSS downsample select={select} ran={ran} ({n},{Ho},{Wo},{Cc}): worst error / bound {worst:.3f} (last row {r_row:.3f}, last column {r_col:.3f})")


# ------------------------------------------------------------------------------------------------ moments
def run_moments(dev, c):
    dx, dW, dbias = gc.embed(c.x, dtype=F16).to(dev), gc.embed(c.Wt, dtype=F16).to(dev), gc.embed_vec(c.bias).to(dev)
    HW = c.H * c.W
    out = gc.out_buffer(c.N * 8, HW, HW, F32).to(dev)  # NCHW [n, 8, H, W] as rows [n 8, HW] + sentinel rows
    L = hip.lib()
    ws = workspace(L.lfm_vae_conv_moments_workspace_bytes(c.N, c.H, c.W), dev)
    rc = L.lfm_vae_conv_moments_f32(hip.ptr(dx), hip.ptr(dW), hip.ptr(dbias), hip.ptr(out), hip.ptr(ws), ws.numel(), c.N, c.H, c.W, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


@pytest.mark.parametrize("n,H,W", vc.MOMENTS_SHAPES)
def test_moments_exact_and_gauss(dev, n, H, W):
    e = vc.moments_exact(n, H, W)
    gc.assert_exact(run_moments(dev, e), e.ref, n * 8, H * W, f"moments exact ({n}, {H}, {W})")
    g = vc.moments_gauss(n, H, W)
    worst = assert_bound(run_moments(dev, g), g.ref, g.bound, n * 8, H * W, f"moments gauss ({n}, {H}, {W})")
    print(f"EXACT moments ({n},{H},{W}) rows={e.M} largest |ref| {int(e.ref.abs().max())}; GAUSS worst error / bound {worst:.2e}")


# ------------------------------------------------------------------------------------------------ resnets
def device_resnets(dev, params):
    """(the lfm_vae_resnet array, the tensors it points to): fp16 weights and fp32 vectors, each ending in NaN guard rows / elements."""
    arr, keep = (hip.VaeResnet * len(params))(), []
    for r, p in zip(arr, params):
        for name in vc.PARAM_NAMES:
            t = p[name]
            if t is None:
                setattr(r, name, None)
                continue
            d = (gc.embed(t, dtype=F16) if name.endswith("_w") else gc.embed_vec(t)).to(dev)
            keep.append(d)
            setattr(r, name, d.data_ptr())
        r.cout, r.cin = p["c1_w"].shape[0], p["c1_w"].shape[1] // 9
    return arr, keep


def run_resnets(dev, c, arr, dx, chain):
    cout = c.widths[-1][1]
    out = gc.out_buffer(c.M, cout, cout, F16).to(dev)
    L = hip.lib()
    ws = workspace(L.lfm_vae_resnets_workspace_bytes(c.n, c.H, c.W), dev)
    slabs = C.c_int(-1)
    rc = L.lfm_vae_resnets_f16(arr, len(c.widths), hip.ptr(dx), hip.ptr(out), hip.ptr(ws), ws.numel(), c.n, c.H, c.W, chain, C.byref(slabs), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out, slabs.value


@pytest.mark.parametrize("chain", (0, 1))
@pytest.mark.parametrize("widths,H,W", vc.resnet_case_list(), ids=lambda v: str(v).replace(" ", ""))
def test_resnets_vs_fp64(dev, widths, H, W, chain):
    c = vc.resnet_case(widths, H, W)
    arr, keep = device_resnets(dev, c.params)
    dx = gc.embed(c.x, dtype=F16).to(dev)
    cout = widths[-1][1]
    halo = H % 16 == 0 and W % 16 == 0  # the halo-tiled convolution takes a problem this small under its parity flag only
    with selected(0, hip.DBG_CONV_HALO_SMALL if halo else 0):
        out, slabs = run_resnets(dev, c, arr, dx, chain)
        again, slabs2 = run_resnets(dev, c, arr, dx, chain)
    got = out[:c.M, :cout].cpu()
    ok, a, b = vc.resnet_within_cap(got, c)
    print(f"MEASURED resnets {widths} {H}x{W} chain_stats={chain} last_slabs={slabs}: relL2 {vc.rel_l2(got, c.ref64):.3e} = {a:.3f} x ref_r's {c.e_l2:.3e}; "
          f"maxabs {vc.max_abs(got, c.ref64):.3e} = {b:.3f} x ref_r's {c.e_max:.3e}")
    assert not gc.touched_positions(out.cpu(), c.M, cout)
    assert ok, (widths, H, W, chain, a, b)
    assert torch.equal(out.view(torch.int16), again.view(torch.int16)) and slabs == slabs2  # two runs are bit-identical
    if chain and halo:
        assert slabs == 2 * (H * W // 256), slabs  # conv2's epilogue left the statistics of the result: the hand-over ran (inside a chain: consumed by the next GroupNorm)
    else:
        assert slabs == 0, slabs
    for i in range(c.n):  # whole-tensor norms dilute a write into a neighbour's rows
        rows = slice(i * H * W, (i + 1) * H * W)
        assert vc.rel_l2(got[rows], c.ref64[rows]) <= vc.RESNET_MARGIN * vc.rel_l2(c.ref_r[rows], c.ref64[rows]), (widths, H, W, chain, i)
