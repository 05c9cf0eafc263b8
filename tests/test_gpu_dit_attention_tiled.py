"""The tiled DiT attention kernel (csrc/attention_tiled_kernel.h) on the device against float64, per (image, head) item and per query row, on inputs whose spiky
keys sit in the first, a middle, the last full and the ragged last stage (tests/dit_attention_cases.py; bounds shown sound by
tests/test_dit_attention_tiled_ref.py).

Bounds: whole rel-L2 < 2e-3 and worst item < 4e-3 are tests/test_gpu_dit.py::test_attention's; worst query row < 4e-3 is ten times the emulation's 4.0e-4 -- the
device differs from the emulation by the order of its fp32 sums, the hardware exp2 and a maximum that is followed lazily.
Measured on an MI355X (whole / worst item / worst query row; two runs bit-equal at every shape; also in profiles/dit_attention_tiled.txt):
    T  144 hd 64   1.71e-4  1.85e-4  4.71e-4        T  144 hd 72   1.76e-4  1.84e-4  5.30e-4
    T  400 hd 64   1.77e-4  1.86e-4  5.20e-4        T  576 hd 72   1.76e-4  1.84e-4  5.31e-4
    T  784 hd 64   1.83e-4  1.87e-4  4.95e-4        T 1296 hd 72   1.73e-4  1.77e-4  5.12e-4
    T 2304 hd 64   1.78e-4  1.82e-4  5.84e-4        T 3600 hd 72   1.80e-4  1.80e-4  4.83e-4
Under LFM_OPT_ATTENTION_TILED = 2 the results equal the owning kernels' bit for bit (64 / 128 / 256 / 1024 tokens x hd 64, 256 x hd 72)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dit_attention_cases as ac
from lfm_amd import hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@pytest.fixture
def tiled_everywhere():
    """LFM_OPT_ATTENTION_TILED = 2 for one test: every shape the kernel takes runs on it."""
    hip.set_option(hip.OPT_ATTENTION_TILED, 2)
    yield
    hip.set_option(hip.OPT_ATTENTION_TILED, 1)


def run(dev, q, k, v):
    """hip.dit_attention on the library's operands -> ([batch, heads, T, hd] on the host, the raw device result)."""
    batch, heads, T, hd = q.shape
    Q, K, Vt = (t.to(dev) for t in ac.operands(q, k, v))
    O = hip.dit_attention(Q, K, Vt, batch, heads, T, head_dim=hd)
    return ac.as_rows(O.cpu(), batch, heads, T, hd), O


def check(got, ref, what):
    whole, item, row = ac.errors(got, ref)
    print(f"{what}: whole {whole:.3e} worst item {item:.3e} worst row {row:.3e}")
    assert bool(torch.isfinite(got).all()), what
    assert whole < ac.TOL_WHOLE and item < ac.TOL_ITEM and row < ac.TOL_ROW, (what, whole, item, row)


@pytest.mark.parametrize("T,heads,batch,hd", ac.SHAPES)
def test_tiled_attention_vs_float64(dev, T, heads, batch, hd):
    assert hip.attention_plan(batch, heads, hd, T) == 7
    q, k, v, ref = ac.case(T, heads, batch, hd)
    got, raw = run(dev, q, k, v)
    _, raw2 = run(dev, q, k, v)
    check(got, ref, f"T {T} heads {heads} batch {batch} hd {hd}")
    assert torch.equal(raw, raw2)


@pytest.mark.parametrize("T,heads,hd", [(144, 2, 64), (144, 2, 72), (400, 3, 64)])
def test_items_are_isolated(dev, T, heads, hd):
    """Image 1's K and V^T all NaN, then all Inf, then ordinary: images 0 and 2 -- whose ragged last stages end where image 1's rows begin, and begin where they end --
    come out bit for bit the same all three times."""
    q, k, v = ac.make_qkv(T, heads, 3, hd, seed=T + hd)
    outs = []
    for fill in (float("nan"), float("inf"), None):
        k2, v2 = k.clone(), v.clone()
        if fill is not None:
            k2[1] = fill
            v2[1] = fill
        got, _ = run(dev, q, k2, v2)
        outs.append(got)
    for o in outs[:2]:
        assert torch.equal(o[0], outs[2][0]) and torch.equal(o[2], outs[2][2])
        assert not bool(torch.isfinite(o[1]).any())  # the poisoned image really was poisoned
    check(outs[2], ac.reference(q, k, v), f"isolation T {T} hd {hd}")


@pytest.mark.parametrize("T,heads,batch,hd", [(144, 2, 3, 64), (144, 2, 3, 72), (400, 3, 2, 64)])
def test_every_access_stays_inside_its_tensor(dev, T, heads, batch, hd):
    """Q, K, V^T and O are views in the middle of larger allocations whose margins (>= 128 rows on both sides) are fp16 NaN -- a sentinel for O: a read outside a
    tensor shows as NaN in the result, a write outside as a changed margin, neither as a fault."""
    q, k, v, ref = ac.case(T, heads, batch, hd)
    D, margin = heads * hd, 128 * heads * hd
    views, bufs = [], []
    for t in ac.operands(q, k, v):
        buf = torch.full((t.numel() + 2 * margin,), float("nan"), dtype=torch.float16, device=dev)
        view = buf[margin:margin + t.numel()].view(t.shape)
        view.copy_(t)
        views.append(view)
        bufs.append(buf)
    Q, K, Vt = views
    obuf = torch.full((batch * T * D + 2 * margin,), -7.5, dtype=torch.float16, device=dev)
    O = obuf[margin:margin + batch * T * D].view(batch * T, D)
    assert all(x.data_ptr() % 16 == 0 for x in (Q, K, Vt, O))
    hip.check(hip.lib().lfm_dit_attention_hd(hip.ptr(Q), hip.ptr(K), hip.ptr(Vt), hip.ptr(O), batch, heads, hd, T, hip.stream_ptr()), "lfm_dit_attention_hd")
    torch.cuda.synchronize()
    assert bool((obuf[:margin] == -7.5).all()) and bool((obuf[margin + batch * T * D:] == -7.5).all())
    for buf, view in zip(bufs, views):  # the inputs were only read
        assert bool(torch.isnan(buf[:margin]).all()) and bool(torch.isnan(buf[margin + view.numel():]).all())
    check(ac.as_rows(O.cpu(), batch, heads, T, hd), ref, f"views T {T} hd {hd}")


@pytest.mark.parametrize("T,heads,batch,hd", [(64, 3, 2, 64), (128, 2, 2, 64), (256, 2, 3, 64), (1024, 2, 2, 64), (256, 2, 2, 72)])
def test_tiled_kernel_on_the_shapes_other_kernels_own(dev, T, heads, batch, hd, tiled_everywhere):
    """LFM_OPT_ATTENTION_TILED = 2: whole stages only, no tails -- the same bounds against float64, and bit for bit the result of the kernel that owns the shape
    (every piece of the arithmetic is one text for all kernels, csrc/attention_common.h, evaluated per query in the same key order)."""
    q, k, v = ac.make_qkv(T, heads, batch, hd)
    assert hip.attention_plan(batch, heads, hd, T) == 7
    tiled, _ = run(dev, q, k, v)
    hip.set_option(hip.OPT_ATTENTION_TILED, 1)
    assert hip.attention_plan(batch, heads, hd, T) in (2, 4, 5)
    own, _ = run(dev, q, k, v)
    check(tiled, ac.reference(q, k, v), f"option 2, T {T} hd {hd}")
    rel = float((tiled.double() - own.double()).norm() / own.double().norm())
    print(f"option 2, T {T} hd {hd}: against the owning kernel {rel:.3e}, bit-equal {torch.equal(tiled, own)}")
    assert rel < 2e-3
    assert torch.equal(tiled, own)


def test_option_zero_refuses_the_new_token_counts(dev):
    q, k, v, _ = ac.case(144, 2, 3, 64)
    hip.set_option(hip.OPT_ATTENTION_TILED, 0)
    try:
        with pytest.raises(hip.LfmHipError):
            run(dev, q, k, v)
    finally:
        hip.set_option(hip.OPT_ATTENTION_TILED, 1)
