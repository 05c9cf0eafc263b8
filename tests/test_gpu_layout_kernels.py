"""GPU tests of the three device ops of the SpatialTransformer (lfm_cross_attention_f16, lfm_layernorm_f16, lfm_geglu_f16) against float64, element by element
or per (image, head) item, at the bounds tests/layout_cases.py derives and tests/test_layout_ref.py shows able to tell right from wrong; the cross-attention
bit for bit where the result is exactly known; and the refusals."""
import pytest
import torch

import layout_cases as lc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -1234.0
N, HEADS = lc.CROSS_N, lc.CROSS_HEADS


def _dev():
    return torch.device("cuda:0")


def _guarded(rows, cols, spare=8):
    """(whole buffer, the [rows, cols] view inside it): GUARD sentinel rows before and after, `spare` sentinel columns to the right of every row."""
    buf = torch.full((rows + 2 * GUARD, cols + spare), SENTINEL, dtype=torch.float16, device=_dev())
    return buf, buf[GUARD:GUARD + rows, :cols]


def _sentinel_intact(buf, rows, cols):
    mask = torch.ones_like(buf, dtype=torch.bool)
    mask[GUARD:GUARD + rows, :cols] = False
    return bool((buf[mask] == SENTINEL).all())


def _kv_buffer(k, v):
    """K and V as two column slices of ONE [N * Tk, 2 C + 8] buffer whose spare columns are NaN."""
    kr, vr = lc.rows(k), lc.rows(v)
    C = kr.shape[1]
    buf = torch.full((kr.shape[0], 2 * C + 8), float("nan"), dtype=torch.float16)
    buf[:, :C], buf[:, C:2 * C] = kr, vr
    buf = buf.to(_dev())
    return buf[:, :C], buf[:, C:2 * C]


@pytest.mark.parametrize("Tq,Tk,ch", lc.CROSS_SHAPES)
def test_cross_attention_against_float64_per_item(Tq, Tk, ch):
    from lfm_amd import hip

    for family in lc.CROSS_FAMILIES:
        (q, k, v), ref = lc.cross_case(family, Tq, Tk, ch)
        K, V = _kv_buffer(k, v)
        buf, out = _guarded(N * Tq, HEADS * ch)
        hip.cross_attention(lc.rows(q).to(_dev()), K, V, N, Tq, Tk, HEADS, ch, out=out)
        torch.cuda.synchronize()
        assert _sentinel_intact(buf, N * Tq, HEADS * ch), (family, "a store outside the output")
        err = lc.worst(lc.items_of_rows(out, N, HEADS, Tq, ch), ref)
        print(f"cross-attention {family} Tq={Tq} Tk={Tk} ch={ch}: worst item {err:.3e}")
        assert err <= lc.TOL, (family, err)


def test_cross_attention_one_key_returns_the_images_value_row():
    from lfm_amd import hip

    Tq, ch = 100, 64
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(N, HEADS, t, ch, generator=g).half() for t in (Tq, 1, 1))
    out = hip.cross_attention(lc.rows(q).to(_dev()), lc.rows(k).to(_dev()), lc.rows(v).to(_dev()), N, Tq, 1, HEADS, ch)
    want = lc.rows(v).reshape(N, 1, HEADS * ch).expand(N, Tq, HEADS * ch).reshape(N * Tq, HEADS * ch)
    assert torch.equal(out.cpu(), want)  # softmax over one key is 1: the wrong image's context cannot pass


@pytest.mark.parametrize("Tk", [64, 128])
def test_cross_attention_identical_keys_return_the_exact_mean(Tk):
    from lfm_amd import hip

    Tq, ch = 100, 64
    g = torch.Generator().manual_seed(6 + Tk)
    q = torch.randn(N, HEADS, Tq, ch, generator=g).half()
    k = torch.randn(N, HEADS, 1, ch, generator=g).half().expand(N, HEADS, Tk, ch)
    v = torch.randint(-4, 5, (N, HEADS, Tk, ch), generator=g).half()
    out = hip.cross_attention(lc.rows(q).to(_dev()), lc.rows(k).to(_dev()), lc.rows(v).to(_dev()), N, Tq, Tk, HEADS, ch)
    # every P is 1, the sum is Tk (a power of two), sum(v) is an integer of at most 512 in magnitude: the mean is exact in fp32 and in fp16
    mean = lc.rows(v.double().mean(dim=2, keepdim=True)).reshape(N, 1, HEADS * ch).expand(N, Tq, HEADS * ch).reshape(N * Tq, HEADS * ch)
    assert torch.equal(out.cpu().double(), mean)  # a dropped or doubled key cannot pass


@pytest.mark.parametrize("T,ch", [(100, 64), (320, 128)])
def test_cross_attention_equals_the_streamed_self_attention_bit_for_bit(T, ch):
    """The kernel keeps the streamed kernel's block order and arithmetic, so with Tq == Tk on the same operands the results are the same bits.  The packed
    buffer is [q | k | v][head][ch], whose thirds are the cross-attention's operands; its column permutation [head][q | k | v][ch] is what
    lfm_attention_small_f16 reads."""
    from lfm_amd import hip

    g = torch.Generator().manual_seed(T + ch)
    C = HEADS * ch
    packed = (1.6 * torch.randn(N * T, 3, HEADS, ch, generator=g)).half().to(_dev())
    flat = packed.reshape(N * T, 3 * C)
    cross = hip.cross_attention(flat[:, :C], flat[:, C:2 * C], flat[:, 2 * C:], N, T, T, HEADS, ch)
    qkv = packed.permute(0, 2, 1, 3).reshape(N * T, 3 * C).contiguous()
    own = torch.empty(N * T, C, dtype=torch.float16, device=_dev())
    try:
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 2)
        assert hip.unet_attention_plan(N, T, HEADS, ch) == 3
        hip.unet_attention(qkv, own, N, T, HEADS, ch)
    finally:
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 1)
    assert torch.equal(cross, own)


def _over(got, ref, bound):
    return float("inf") if not bool(torch.isfinite(got).all()) else float(((got.double().cpu() - ref).abs() / bound).max())


@pytest.mark.parametrize("C", lc.LN_WIDTHS)
def test_layernorm_against_float64(C):
    from lfm_amd import hip

    for family in lc.LN_FAMILIES:
        x, gamma, beta, ref = lc.ln_case(family, C)
        buf, out = _guarded(lc.LN_ROWS, C, spare=0)
        hip.layernorm(x.to(_dev()), gamma.to(_dev()), beta.to(_dev()), eps=lc.LN_EPS, out=out)
        torch.cuda.synchronize()
        assert _sentinel_intact(buf, lc.LN_ROWS, C)
        r = _over(out, ref, lc.ln_bound(x, gamma, beta))
        print(f"LayerNorm {family} C={C}: worst element at {r:.3f} of its bound")
        assert r <= 1.0, (family, C, r)


@pytest.mark.parametrize("I", lc.GEGLU_WIDTHS)
def test_geglu_against_float64(I):
    from lfm_amd import hip

    h, ref = lc.geglu_case(I)
    buf, out = _guarded(lc.GEGLU_ROWS, I, spare=0)
    hip.geglu(h.to(_dev()), out=out)
    torch.cuda.synchronize()
    assert _sentinel_intact(buf, lc.GEGLU_ROWS, I)
    r = _over(out, ref, lc.geglu_bound(h))
    print(f"GEGLU I={I}: worst element at {r:.3f} of its bound")
    assert r <= 1.0, (I, r)
    wide = torch.full((lc.GEGLU_ROWS, 2 * I + 8), float("nan"), dtype=torch.float16)  # rows ldh = 2I + 8 apart: the same bits
    wide[:, :2 * I] = h
    assert torch.equal(hip.geglu(wide.to(_dev())[:, :2 * I]), out)


def test_refusals_leave_the_output_untouched():
    from lfm_amd import hip

    L, dev = hip.lib(), _dev()
    SHAPE, ALIGN = -1, -2
    st = hip.stream_ptr(dev)
    Tq, Tk, ch, C = 64, 17, 32, 64
    q = torch.zeros(N * Tq + 1, C + 8, dtype=torch.float16, device=dev)
    kv = torch.zeros(N * Tk + 1, 2 * C + 8, dtype=torch.float16, device=dev)
    out = torch.full((N * Tq + 1, C + 8), SENTINEL, dtype=torch.float16, device=dev)
    P = lambda t, off=0: hip.C.c_void_p(t.data_ptr() + off)  # noqa: E731

    def cross(qp=P(q), ldq=C + 8, kp=P(kv), vp=P(kv, 2 * C), ldkv=2 * C + 8, op=P(out), ldo=C + 8, ch=ch):
        return L.lfm_cross_attention_f16(qp, ldq, kp, vp, ldkv, op, ldo, N, Tq, Tk, HEADS, ch, st)

    assert cross(qp=P(q, 2)) == ALIGN and cross(kp=P(kv, 4)) == ALIGN and cross(vp=P(kv, 2 * C + 8)) == ALIGN and cross(op=P(out, 8)) == ALIGN
    assert cross(ldq=C + 4) == ALIGN and cross(ldkv=2 * C + 4) == ALIGN and cross(ldo=C + 12) == ALIGN
    assert cross(ch=40) == SHAPE and cross(ldo=C - 8) == SHAPE
    x = torch.zeros(5, 72, dtype=torch.float16, device=dev)
    gb = torch.zeros(80, device=dev)
    assert L.lfm_layernorm_f16(P(x), P(out), P(gb), P(gb), 5, 68, 1e-5, st) == SHAPE  # C % 8
    assert L.lfm_layernorm_f16(P(x, 2), P(out), P(gb), P(gb), 4, 72, 1e-5, st) == ALIGN and L.lfm_layernorm_f16(P(x), P(out, 2), P(gb), P(gb), 4, 72, 1e-5, st) == ALIGN
    assert L.lfm_geglu_f16(P(x), 72, P(out), 5, 36, st) == SHAPE and L.lfm_geglu_f16(P(x), 72, P(out), 5, 40, st) == SHAPE  # I % 8; ldh < 2I
    assert L.lfm_geglu_f16(P(x), 68, P(out), 5, 32, st) == ALIGN and L.lfm_geglu_f16(P(x, 2), 72, P(out), 4, 32, st) == ALIGN
    with pytest.raises(hip.LfmHipError, match="% 16"):
        hip.cross_attention(q, kv, kv, N, Tq, Tk, HEADS, 40)
    with pytest.raises(hip.LfmHipError, match="% 8"):
        hip.layernorm(x[:, :68], gb, gb)
    # the wrappers refuse what the C contract cannot express: strided rows where the kernel walks dense ones, other dtypes, other shapes
    wide = torch.full((5, 80), SENTINEL, dtype=torch.float16, device=dev)
    with pytest.raises(hip.LfmHipError, match="dense"):
        hip.layernorm(x[:, :64], gb[:64], gb[:64])  # x a column slice
    with pytest.raises(hip.LfmHipError, match="dense"):
        hip.layernorm(x[:, :64].contiguous(), gb[:64], gb[:64], out=wide[:, :64])
    with pytest.raises(hip.LfmHipError, match="gamma"):
        hip.layernorm(x[:, :64].contiguous(), gb[:128:2], gb[:64])
    with pytest.raises(hip.LfmHipError, match="dense"):
        hip.geglu(x[:, :64], out=wide[:, :32])
    with pytest.raises(hip.LfmHipError, match="unit column stride"):
        hip.geglu(torch.zeros(16, 8, dtype=torch.float16, device=dev).t())
    with pytest.raises(hip.LfmHipError, match="out must be"):
        hip.cross_attention(q[:N * Tq, :C], kv[:N * Tk, :C], kv[:N * Tk, C:2 * C], N, Tq, Tk, HEADS, ch, out=out[:N * Tq, :2 * C:2])
    with pytest.raises(hip.LfmHipError, match="Q must be"):
        hip.cross_attention(q[:N * Tq, :C].float(), kv[:N * Tk, :C], kv[:N * Tk, C:2 * C], N, Tq, Tk, HEADS, ch)
    with pytest.raises(hip.LfmHipError, match="share a row stride"):
        hip.cross_attention(q[:N * Tq, :C], kv[:N * Tk, :C], kv[:N * Tk, C:2 * C].contiguous(), N, Tq, Tk, HEADS, ch)
    assert bool((wide == SENTINEL).all())
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    assert cross() == 0  # the same call with nothing wrong runs
    torch.cuda.synchronize()
    assert bool((out[:N * Tq, :C] != SENTINEL).all()) and bool((out[N * Tq:] == SENTINEL).all()) and bool((out[:, C:] == SENTINEL).all())
