"""The three kernels ``adm_context`` added (include/lfm_hip.h): lfm_linear_resid_vec_f16 and lfm_linear_silu_f16 on every GEMM kernel the chooser can give
them, element by element, and lfm_gather_rows_f32 bit for bit.  Cases, references and the derived bounds: tests/adm_context_cases.py (pinned on the CPU in
tests/test_adm_context_ref.py); operand layouts, NaN pads, guard rows and sentinels: tests/gemm_exact_cases.py."""
import pytest
import torch

import adm_context_cases as ac
import gemm_exact_cases as gc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -5
RSQRT2 = float(torch.tensor(0.5).sqrt())  # the scale as the kernel receives it (fp32)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


class selected:
    def __init__(self, kernel):
        self.which = kernel

    def __enter__(self):
        hip.gemm_select(self.which)

    def __exit__(self, *exc):
        hip.gemm_select(0)


def _operands(dev, c, layout, with_resid=True):
    da, dw, dc = gc.LAYOUTS[layout]
    A, W = gc.embed(c.A, c.K + da, dtype=F16).to(dev), gc.embed(c.W, c.K + dw, dtype=F16).to(dev)
    bias = gc.embed_vec(c.bias).to(dev)
    resid = gc.embed(c.resid, c.N + dc, dtype=F16).to(dev) if with_resid else None
    out = gc.out_buffer(c.M, c.N, c.N + dc, F16).to(dev)
    return A, W, bias, resid, out, (c.K + da, c.K + dw, c.N + dc)


def _resid_vec(dev, c, layout, scale, vec="case"):
    """lfm_linear_resid_vec_f16 on case c; vec: "case" (strided where the layout is, NaN pads and guard rows), "zero", or None."""
    A, W, bias, resid, out, (lda, ldw, ldc) = _operands(dev, c, layout)
    v, vs = None, 0
    if vec is not None:
        vs = c.N + (ac.VEC_PAD if layout != "dense" else 0)
        v = gc.embed(c.vec if vec == "case" else torch.zeros_like(c.vec, dtype=F32), vs, dtype=F32).to(dev)
    rc = hip.lib().lfm_linear_resid_vec_f16(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(out), ldc, c.M, c.N, c.K, hip.ptr(bias), hip.ptr(resid), hip.ptr(v), vs,
                                            c.tokens, scale, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (rc, layout, scale, vec)
    return out


def _scaled(dev, c, layout, scale):
    A, W, bias, resid, out, (lda, ldw, ldc) = _operands(dev, c, layout)
    rc = hip.lib().lfm_linear_scaled_f16(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(out), ldc, c.M, c.N, c.K, hip.ptr(bias), hip.ptr(resid), scale, hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0
    return out


# ------------------------------------------------------------------------------------------------ lfm_linear_resid_vec_f16
@pytest.mark.parametrize("kernel", ac.KERNEL_SELECTIONS)
def test_resid_vec_exact_on_integer_data(dev, kernel):
    """(acc + bias + resid + vec[m // tokens]) * scale with integer-valued operands and scale 1 / 0.5: the int64 result bit for bit; vec = NULL and vec = 0
    equal lfm_linear_scaled_f16 bit for bit, pads and guard rows included."""
    n = 0
    with selected(kernel):
        for tokens, M, N, K in ac.kernel_shapes():
            plan = hip.gemm_plan(M, N, K)
            assert plan == (kernel or 1), f"selection {kernel} at {M} x {N} x {K} runs kernel {plan}"
            c = ac.resid_vec_int_case(tokens, M, N, K)
            for layout in ac.KERNEL_LAYOUTS:
                for scale, ref in ((1.0, c.ref), (0.5, c.ref.double() * 0.5)):
                    gc.assert_exact(_resid_vec(dev, c, layout, scale), ref, M, N, f"resid_vec kernel {plan} {layout} tokens {tokens} {M}x{N}x{K} scale {scale}", plan)
                    n += 1
                plain = _scaled(dev, c, layout, 0.5)
                gc.assert_exact(plain, c.ref_novec.double() * 0.5, M, N, f"linear_scaled kernel {plan} {layout}", plan)
                for vec in (None, "zero"):
                    assert torch.equal(_resid_vec(dev, c, layout, 0.5, vec), plain), (plan, layout, vec, tokens, M, N, K)
                    n += 1
    print(f"EXACT resid_vec select={kernel} shapes={len(ac.kernel_shapes())} cases={n}")


@pytest.mark.parametrize("kernel", ac.KERNEL_SELECTIONS)
def test_resid_vec_gaussian_per_element(dev, kernel):
    worst = 0.0
    with selected(kernel):
        for tokens, M, N, K in ac.kernel_shapes():
            c = ac.resid_vec_gauss_case(tokens, M, N, K, RSQRT2)
            for layout in ac.KERNEL_LAYOUTS:
                out = _resid_vec(dev, c, layout, RSQRT2).cpu()
                assert not gc.touched_positions(out, M, N)
                ratio = (out[:M, :N].double() - c.ref).abs() / c.bound
                r = float(ratio.max())
                m, nn = divmod(int(ratio.argmax()), N)
                assert r <= 1.0, f"kernel {kernel} {layout} tokens {tokens} {M}x{N}x{K}: error / bound {r:.3f} at ({m}, {nn})"
                worst = max(worst, r)
            # vec = NULL against lfm_linear_scaled_f16 on real-valued data too
            assert torch.equal(_resid_vec(dev, c, "dense", RSQRT2, None), _scaled(dev, c, "dense", RSQRT2))
    print(f"BOUND resid_vec kernel={kernel} largest error/bound={worst:.3f}")
    assert worst > 0.05  # (the bound is not vacuous: an fp16 rounding alone reaches about a third of it)


def test_resid_vec_refusals_come_before_any_launch(dev):
    c = ac.resid_vec_int_case(64, 192, 64, 64)
    A, W, bias, resid, out, (lda, ldw, ldc) = _operands(dev, c, "wide")
    vec = gc.embed(c.vec, c.N + 4, dtype=F32).to(dev)
    L, st = hip.lib(), hip.stream_ptr()

    def call(M=c.M, tokens=64, v=hip.ptr(vec), vs=c.N + 4, a=hip.ptr(A), lda_=lda, ldc_=ldc):
        return L.lfm_linear_resid_vec_f16(a, lda_, hip.ptr(W), ldw, hip.ptr(out), ldc_, M, c.N, c.K, hip.ptr(bias), hip.ptr(resid), v, vs, tokens, 1.0, st)

    assert call(tokens=0) == ERR_SHAPE and call(tokens=-64) == ERR_SHAPE
    assert call(tokens=80) == ERR_SHAPE  # M % tokens
    assert call(M=0) == ERR_SHAPE
    assert call(vs=c.N + 2) == ERR_ALIGN  # vec_stride % 4
    assert call(v=hip.ptr(vec.reshape(-1)[1:])) == ERR_ALIGN  # vec 4 bytes off a 16-byte boundary
    assert call(lda_=lda + 4) == ERR_ALIGN and call(ldc_=ldc + 2) == ERR_ALIGN
    assert call(a=hip.ptr(A.reshape(-1)[4:])) == ERR_ALIGN
    assert call(a=None) == ERR_ARG
    assert L.lfm_linear_resid_vec_f16(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(out), ldc, c.M, c.N, 48, hip.ptr(bias), hip.ptr(resid), hip.ptr(vec), c.N + 4,
                                      64, 1.0, st) == ERR_SHAPE  # K % 64, as lfm_linear_scaled_f16
    assert L.lfm_linear_silu_f16(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(out), ldc, c.M, c.N, c.K, None, st) == ERR_ARG  # the bias is required
    assert L.lfm_linear_silu_f16(hip.ptr(A), lda + 4, hip.ptr(W), ldw, hip.ptr(out), ldc, c.M, c.N, c.K, hip.ptr(bias), st) == ERR_ALIGN
    assert L.lfm_linear_silu_f16(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(out), ldc, c.M, c.N, 48, hip.ptr(bias), st) == ERR_SHAPE
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ lfm_linear_silu_f16
@pytest.mark.parametrize("kernel", ac.KERNEL_SELECTIONS)
def test_linear_silu_per_element(dev, kernel):
    worst = 0.0
    with selected(kernel):
        for _, M, N, K in ac.kernel_shapes():
            assert hip.gemm_plan(M, N, K) == (kernel or 1)
            c = ac.silu_case(M, N, K)
            for layout in ac.KERNEL_LAYOUTS:
                A, W, bias, _, out, (lda, ldw, ldc) = _operands(dev, c, layout, with_resid=False)
                rc = hip.lib().lfm_linear_silu_f16(hip.ptr(A), lda, hip.ptr(W), ldw, hip.ptr(out), ldc, M, N, K, hip.ptr(bias), hip.stream_ptr())
                torch.cuda.synchronize()
                assert rc == 0
                out = out.cpu()
                assert not gc.touched_positions(out, M, N)
                got = out[:M, :N].double()
                assert not bool(got.isnan().any())
                ratio = (got - c.ref).abs() / c.bound
                r = float(ratio.max())
                m, nn = divmod(int(ratio.argmax()), N)
                assert r <= 1.0, (f"kernel {kernel} {layout} {M}x{N}x{K}: error / bound {r:.3f} at ({m}, {nn}): x = {float(c.pre[m, nn])}, got {float(got[m, nn])!r}, "
                                  f"ref {float(c.ref[m, nn])!r}")
                worst = max(worst, r)
    print(f"BOUND silu kernel={kernel} largest error/bound={worst:.3f}")


# ------------------------------------------------------------------------------------------------ lfm_gather_rows_f32
@pytest.mark.parametrize("rows,cols,pad", [(11, 64, 0), (11, 1088, 0), (3, 192, 8), (1001, 68, 4)])
def test_gather_rows_bit_exact(dev, rows, cols, pad):
    """Repeated labels, the first and the last row, a column stride; a sentinel in the pad columns and after the last row; then the labels rewritten in
    place and the same call again."""
    g = torch.Generator().manual_seed(rows + cols)
    table = torch.randn(rows, cols, generator=g)
    y = torch.tensor([rows - 1, 0, rows // 2, rows - 1, 0, rows - 1, 1 % rows])
    N = y.numel()
    dt, dy = gc.embed(table, cols, dtype=F32).to(dev), y.to(dev)
    out = gc.out_buffer(N, cols, cols + pad, F32).to(dev)
    hip.gather_rows(dt[:rows], dy, out=out[:N, :cols])
    torch.cuda.synchronize()
    assert not gc.touched_positions(out.cpu(), N, cols)
    assert torch.equal(out[:N, :cols].cpu(), table[y])
    dy.copy_(torch.flip(y, [0]).to(dev))
    hip.gather_rows(dt[:rows], dy, out=out[:N, :cols])
    assert torch.equal(out[:N, :cols].cpu(), table[torch.flip(y, [0])])
    L, st = hip.lib(), hip.stream_ptr()
    assert L.lfm_gather_rows_f32(hip.ptr(dt), rows, cols - 2, hip.ptr(dy), N, hip.ptr(out), cols + pad, st) == ERR_SHAPE
    assert L.lfm_gather_rows_f32(hip.ptr(dt), rows, cols, hip.ptr(dy), N, hip.ptr(out), cols - 4, st) == ERR_SHAPE
    assert L.lfm_gather_rows_f32(hip.ptr(dt), rows, cols, hip.ptr(dy), N, hip.ptr(out.reshape(-1)[1:]), cols + pad, st) == ERR_ALIGN
    assert L.lfm_gather_rows_f32(hip.ptr(dt), rows, cols, None, N, hip.ptr(out), cols + pad, st) == ERR_ARG
