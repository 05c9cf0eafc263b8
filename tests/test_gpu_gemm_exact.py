"""Every GEMM and conv3x3 path of the library, element by element (cases, references and the checker: tests/gemm_exact_cases.py).

Exact part: fp16 operands holding small integers make every product and partial sum exact in fp32 in any order, so each kernel (128x128, 256x128, both
256x256, the two latency-mode kernels, the split-K slices with their finish kernel, the halo convolution), each tile order and each store width must
return the int64 product bit for bit.  Operands sit in larger buffers whose pad columns and guard rows hold NaN, outputs in buffers pre-filled with a
sentinel that must survive everywhere outside [0, M) x [0, N): a store out of bounds, a pad column read into a product, an exchanged H / W of a
non-square map or a dropped k-term of a tail K-tile fails AT ITS ELEMENT.  Layouts: dense, lda = K + 8 / ldw = K + 8 / ldc = N + 8, and ldc = N + 4 (the
8-byte-store path of the fp16 epilogues through a real ldc).

Real-valued part: the GELU epilogue and Gaussian operands against float64 with per-element bounds derived in gemm_exact_cases.py (not tuned)."""
import ctypes as C

import pytest
import torch

import gemm_exact_cases as gc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
ERR_SHAPE, ERR_ALIGN = -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


class selected:
    """lfm_gemm_select(kernel | flags << 4) for the block, the automatic choice afterwards."""

    def __init__(self, kernel, flags=0):
        self.which = kernel | (flags << 4)

    def __enter__(self):
        hip.gemm_select(self.which)

    def __exit__(self, *exc):
        hip.gemm_select(0)


def _gemm_f16(dev, c, layout):
    """lfm_gemm_f16 on case c in a layout: returns (return code, the guarded output buffer)."""
    da, dw, dc = gc.LAYOUTS[layout]
    M, N, K = c.M, c.N, c.K
    A = gc.embed(c.A, K + da, dtype=F16).to(dev)
    W = gc.embed(c.W, K + dw, dtype=F16).to(dev)
    bias = gc.embed_vec(c.bias).to(dev)
    out = gc.out_buffer(M, N, N + dc, F16 if c.epi in (0, 1) else F32, init=c.X).to(dev)
    gate, gstride = None, 0
    if c.gate is not None:
        gate = gc.embed(c.gate, N + (8 if dc else 0), dtype=F32).to(dev)
        gstride = 0 if c.gate.shape[0] == 1 else gate.stride(0)
    rc = hip.lib().lfm_gemm_f16(hip.ptr(A), K + da, hip.ptr(W), K + dw, hip.ptr(out), N + dc, M, N, K, hip.ptr(bias), c.epi, hip.ptr(gate), gstride, c.tokens,
                                hip.stream_ptr())
    torch.cuda.synchronize()
    return rc, out


# ------------------------------------------------------------------------------------------------ lfm_gemm_f16, exact
@pytest.mark.parametrize("kernel,M,N,K", gc.gemm_f16_cases())
def test_gemm_f16_exact(dev, kernel, M, N, K):
    n = 0
    with selected(kernel):
        plan = hip.gemm_plan(M, N, K)
        assert plan == (kernel or 1), f"selection {kernel} at {M} x {N} x {K} runs kernel {plan}"
        for epi, shared in gc.EPILOGUES:
            c = gc.gemm_case(M, N, K, epi, shared)
            for layout in gc.LAYOUTS:
                rc, out = _gemm_f16(dev, c, layout)
                assert rc == 0, (rc, epi, layout)
                gc.assert_exact(out, c.ref, M, N, f"lfm_gemm_f16 kernel {plan} epilogue {epi}{' shared gate' if shared else ''} {layout} {M} x {N} x {K}", plan)
                n += 1
    tiles = -(-M // gc.TILES[plan][0]) * -(-N // gc.TILES[plan][1])
    print(f"EXACT gemm_f16 select={kernel} ran={plan} {M}x{N}x{K} tiles={tiles} remap={'on' if tiles % 8 == 0 else 'off'} cases={n}")


@pytest.mark.parametrize("kernel,M,N,K", gc.latency_cases())
def test_latency_kernels_exact(dev, kernel, M, N, K):
    n = 0
    with selected(kernel):
        for epi in (0, 2):
            c = gc.gemm_case(M, N, K, epi)
            for layout in gc.LAYOUTS:  # (gemm_sq64_ok / gemm_skinny_ok take any lda, ldw % 8 == 0: no layout here is refused by contract)
                rc, out = _gemm_f16(dev, c, layout)
                assert rc == 0, (rc, epi, layout)
                gc.assert_exact(out, c.ref, M, N, f"latency kernel {kernel} epilogue {epi} {layout} {M} x {N} x {K}", kernel)
                n += 1
    print(f"EXACT latency select={kernel} ran={kernel} {M}x{N}x{K} cases={n}")


def test_latency_kernels_refuse_by_contract(dev):
    """What gemm_sq64_ok / gemm_skinny_ok refuse is refused, not launched: the output keeps its sentinel."""
    for kernel, M, N in [(7, 200, 64), (7, 192, 176), (8, 200, 132), (8, 320, 64)]:
        c = gc.gemm_case(320, 192, 64, 0)
        c = gc.SimpleNamespace(**{**vars(c), "M": M, "N": N, "A": c.A[:M], "W": c.W[:N], "bias": c.bias[:N]})
        with selected(kernel):
            rc, out = _gemm_f16(dev, c, "wide")
        assert rc == ERR_SHAPE, (kernel, M, N, rc)
        assert bool((out == gc.SENTINEL).all())


# ------------------------------------------------------------------------------------------------ lfm_gemm_qkv_f16, exact
@pytest.mark.parametrize("kernel", [1, 4, 5, 6])
@pytest.mark.parametrize("batch,tokens,D,hd", gc.QKV_SHAPES)
def test_gemm_qkv_exact(dev, batch, tokens, D, hd, kernel):
    c = gc.qkv_case(batch, tokens, D, hd)
    M = c.M
    A = gc.embed(c.A, D + 8, dtype=F16).to(dev)
    W = gc.embed(c.W, D + 8, dtype=F16).to(dev)
    bias = gc.embed_vec(c.bias).to(dev)
    Q, K = gc.out_buffer(M, D, D, F16).to(dev), gc.out_buffer(M, D, D, F16).to(dev)
    Vt = torch.full((batch + 1, D // hd, hd, tokens), gc.SENTINEL, dtype=F16, device=dev)  # one guard image
    with selected(kernel):
        plan = hip.gemm_plan(M, 3 * D, D)
        assert plan == kernel
        rc = hip.lib().lfm_gemm_qkv_f16(hip.ptr(A), D + 8, hip.ptr(W), D + 8, hip.ptr(Q), hip.ptr(K), hip.ptr(Vt), M, D, D, hip.ptr(bias), hd, tokens,
                                        hip.stream_ptr())
        torch.cuda.synchronize()
    assert rc == 0
    gc.assert_exact(Q, c.q, M, D, f"Q kernel {kernel}", kernel)
    gc.assert_exact(K, c.k, M, D, f"K kernel {kernel}", kernel)
    Vt = Vt.cpu()
    assert bool((Vt[batch] == gc.SENTINEL).all()), "V^T written past the last image"
    got = Vt[:batch][..., hip.vt_token_perm(tokens)].double()
    bad = (got != c.vt.double()).nonzero().tolist()
    assert not bad, f"V^T kernel {kernel}: {len(bad)} elements differ; first (image, head, d, token): {bad[:6]}"
    print(f"EXACT gemm_qkv select={kernel} ran={plan} {M}x{3 * D}x{D} hd={hd} cases=1")


# ------------------------------------------------------------------------------------------------ lfm_linear*_f16, exact
def _linear(dev, c, layout, scale=None):
    da, dw, dc = gc.LAYOUTS[layout]
    M, N, K = c.M, c.N, c.K
    A, W = gc.embed(c.A, K + da, dtype=F16).to(dev), gc.embed(c.W, K + dw, dtype=F16).to(dev)
    bias, resid = gc.embed_vec(c.bias).to(dev), gc.embed(c.resid, N + dc, dtype=F16).to(dev)
    out = gc.out_buffer(M, N, N + dc, F16).to(dev)
    L = hip.lib()
    if scale is None:
        rc = L.lfm_linear_f16(hip.ptr(A), K + da, hip.ptr(W), K + dw, hip.ptr(out), N + dc, M, N, K, hip.ptr(bias), hip.ptr(resid), hip.stream_ptr())
    else:
        rc = L.lfm_linear_scaled_f16(hip.ptr(A), K + da, hip.ptr(W), K + dw, hip.ptr(out), N + dc, M, N, K, hip.ptr(bias), hip.ptr(resid), scale,
                                     hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (rc, layout, scale)
    return out


@pytest.mark.parametrize("kernel", [0, 1, 4, 5, 6])
def test_linear_exact(dev, kernel):
    M, N, K = gc.LINEAR_SHAPES[0]
    c = gc.linear_case(M, N, K)
    n = 0
    with selected(kernel):
        plan = hip.gemm_plan(M, N, K)
        assert plan == (kernel or 1)
        for layout in gc.LAYOUTS:
            for scale, ref in ((None, c.ref), (1.0, c.ref), (0.5, c.ref.double() * 0.5)):
                gc.assert_exact(_linear(dev, c, layout, scale), ref, M, N, f"linear kernel {plan} {layout} scale {scale}", plan)
                n += 1
    print(f"EXACT linear select={kernel} ran={plan} {M}x{N}x{K} cases={n}")


def test_linear_exact_on_the_choosers_kernel_4(dev):
    """64 x 3 tiles of 256 x 128 but fewer than 192 tiles of 256 x 256, K a multiple of 32 only: the automatic choice is the 256x128 kernel (ragged last row tile,
    ragged last column tile, three 32-deep K-tiles)."""
    M, N, K = gc.LINEAR_SHAPES[1]
    c = gc.linear_case(M, N, K)
    assert hip.gemm_plan(M, N, K) == 4
    for layout, scale, ref in (("dense", None, c.ref), ("narrow", 0.5, c.ref.double() * 0.5)):
        gc.assert_exact(_linear(dev, c, layout, scale), ref, M, N, f"linear on the chooser's kernel 4 {layout} scale {scale}", 4)
    print(f"EXACT linear select=0 ran=4 {M}x{N}x{K} cases=2")


@pytest.mark.parametrize("K1", [64, 128])
@pytest.mark.parametrize("kernel", [0, 1, 4, 5])
def test_linear2_exact(dev, kernel, K1):
    """A = [A1 | A2] read in place: the seam after K-tile 1 and after K-tile 2 of 3 (after 32-deep tile 2 / 4 of 6 on the 256x128 kernel)."""
    M, N, K = gc.LINEAR_SHAPES[0]
    c = gc.linear_case(M, N, K)
    K2 = K - K1
    A1, A2 = gc.embed(c.A[:, :K1], dtype=F16).to(dev), gc.embed(c.A[:, K1:], dtype=F16).to(dev)  # dense by contract; NaN guard rows
    L, n = hip.lib(), 0
    with selected(kernel):
        plan = hip.gemm_plan(M, N, K, caps=hip.GEMM_CAP_FITS)
        assert plan == (kernel or 1)
        for layout in ("dense", "narrow"):
            _, dw, dc = gc.LAYOUTS[layout]
            W, bias, resid = gc.embed(c.W, K + dw, dtype=F16).to(dev), gc.embed_vec(c.bias).to(dev), gc.embed(c.resid, N + dc, dtype=F16).to(dev)
            for scale, ref in ((None, c.ref), (0.5, c.ref.double() * 0.5)):
                out = gc.out_buffer(M, N, N + dc, F16).to(dev)
                if scale is None:
                    rc = L.lfm_linear2_f16(hip.ptr(A1), K1, hip.ptr(A2), K2, hip.ptr(W), K + dw, hip.ptr(out), N + dc, M, N, hip.ptr(bias), hip.ptr(resid),
                                           hip.stream_ptr())
                else:
                    rc = L.lfm_linear2_scaled_f16(hip.ptr(A1), K1, hip.ptr(A2), K2, hip.ptr(W), K + dw, hip.ptr(out), N + dc, M, N, hip.ptr(bias),
                                                  hip.ptr(resid), scale, hip.stream_ptr())
                torch.cuda.synchronize()
                assert rc == 0
                gc.assert_exact(out, ref, M, N, f"linear2 kernel {plan} K1 {K1} {layout} scale {scale}", plan)
                n += 1
    print(f"EXACT linear2 select={kernel} ran={plan} {M}x{N}x{K1}+{K2} cases={n}")


# ------------------------------------------------------------------------------------------------ lfm_conv3x3*_f16_ws, exact
def _conv(dev, c, dx, dW, dbias, dresid, ws, ws_bytes, scale):
    out = gc.out_buffer(c.M, c.Cout, c.Cout, F16).to(dev)
    L = hip.lib()
    args = (c.N, c.H, c.W, c.Cin, c.Cout, c.mode, hip.ptr(ws) if ws_bytes else None, ws_bytes, hip.stream_ptr())
    if scale is None:
        rc = L.lfm_conv3x3_f16_ws(hip.ptr(dx), hip.ptr(dW), hip.ptr(dbias), hip.ptr(dresid), hip.ptr(out), *args)
    else:
        rc = L.lfm_conv3x3_scaled_f16_ws(hip.ptr(dx), hip.ptr(dW), hip.ptr(dbias), hip.ptr(dresid), scale, hip.ptr(out), *args)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out


CONV_PARAMS = [(path, N, H, W, Cin, Cout, mode) for path, N, H, W, Cin, Cout, modes in gc.CONV_CASES for mode in modes]


@pytest.mark.parametrize("path,N,H,W,Cin,Cout,mode", CONV_PARAMS)
def test_conv3x3_exact(dev, path, N, H, W, Cin, Cout, mode):
    """Every plan path x mode on a non-square map, bias + residual, the unscaled and the scaled entry point (scale 1/2 is exact on these integers)."""
    c = gc.conv_case(N, H, W, Cin, Cout, mode)
    M, K = c.M, 9 * Cin
    dx, dW = gc.embed(c.x, dtype=F16).to(dev), gc.embed(c.Wt, dtype=F16).to(dev)  # NaN guard rows after the last pixel / the last filter
    dbias, dresid = gc.embed_vec(c.bias).to(dev), gc.embed(c.resid, dtype=F16).to(dev)
    need = hip.lib().lfm_conv3x3_workspace_bytes(N, H, W, Cin, Cout)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=dev)
    IMPL, SMALL, S128 = hip.DBG_CONV_IMPLICIT_GEMM, hip.DBG_CONV_HALO_SMALL, hip.DBG_GEMM_SPLITK128
    # (name, kernel selection, flags, workspace bytes offered, lfm_conv3x3_plan's answer, the GEMM kernel where one implicit GEMM runs)
    if path == "halo":
        runs = [("halo kernel", 0, SMALL, 0, hip.CONV_PLAN_HALO, None)]
    elif path == "gemm":  # (no workspace offered: one implicit GEMM whatever the shape)
        runs =[("implicit GEMM", 0, IMPL, 0, hip.CONV_PLAN_GEMM, 1), ("implicit GEMM", 4, 0, 0, hip.CONV_PLAN_GEMM, 4), ("implicit GEMM", 5, 0, 0, hip.CONV_PLAN_GEMM, 5)]
    elif path == "splitk128":
        assert need > 0 and not gc.splitk256_slices(M, Cout, K, need)
        runs = [("split-K 128x128 slices", 0, IMPL | S128, need, hip.CONV_PLAN_SPLITK, None), ("workspace withheld", 0, IMPL | S128, 0, hip.CONV_PLAN_GEMM, 1)]
    else:
        assert gc.splitk256_slices(M, Cout, K, need) == 2 and need == 2 * M * Cout * 4
        runs = [("split-K 256x256 slices", 0, IMPL, need, hip.CONV_PLAN_SPLITK, None), ("split-K 128x128 slices", 0, IMPL | S128, need, hip.CONV_PLAN_SPLITK, None),
                ("workspace withheld", 0, IMPL, 0, hip.CONV_PLAN_GEMM, 1)]
    n = 0
    for name, kernel, flags, ws_bytes, want_plan, want_kernel in runs:
        with selected(kernel, flags):
            plan = hip.conv3x3_plan(N, H, W, Cin, Cout, mode, ws_bytes)
            assert plan == want_plan, (name, plan)
            ran = hip.gemm_plan(M, Cout, K, caps=hip.GEMM_CAP_FITS) if want_kernel else None
            assert ran == want_kernel, (name, ran)
            for scale, ref in ((None, c.ref), (0.5, c.ref.double() * 0.5)):
                out = _conv(dev, c, dx, dW, dbias, dresid, ws, ws_bytes, scale)
                gc.assert_exact(out, ref, M, Cout, f"conv3x3 {name} kernel {ran} mode {mode} ({N}, {H}, {W}, {Cin}, {Cout}) scale {scale}", ran)
                n += 1
        print(f"EXACT conv3x3 path={name} select={kernel} plan={plan} gemm_kernel={ran} mode={mode} ({N},{H},{W},{Cin},{Cout}) cases=2")


# ------------------------------------------------------------------------------------------------ real-valued: GELU, Gaussian operands
@pytest.mark.parametrize("kernel", [1, 4, 5, 6, 7, 8])
def test_gelu_epilogue_per_element(dev, kernel):
    """Epilogue 1 on a pre-activation that is exact in fp32 (multiples of 1/8 over about [-17, 18]): |got - gelu_tanh64(x)| <= 1.5 * 2^-11 |ref| + 2^-24 per element."""
    M, N = gc.GELU_SHAPES[kernel]
    c = gc.gelu_case(M, N)
    case = gc.SimpleNamespace(M=M, N=N, K=c.K, epi=1, A=c.A, W=c.W, bias=c.bias, X=None, gate=None, tokens=1)
    worst = 0.0
    for layout in ("dense", "narrow"):
        with selected(kernel):
            if kernel < 7:
                assert hip.gemm_plan(M, N, c.K) == kernel
            rc, out = _gemm_f16(dev, case, layout)
        assert rc == 0
        out = out.cpu()
        assert not gc.touched_positions(out, M, N)
        got = out[:M, :N].double()
        assert not bool(got.isnan().any())
        ratio = (got - c.ref).abs() / c.bound
        worst = max(worst, float(ratio.max()))
        m, n = divmod(int(ratio.argmax()), N)
        assert worst <= 1.0, f"kernel {kernel} {layout}: error / bound {float(ratio.max()):.3f} at ({m}, {n}): x = {float(c.pre[m, n])}, got {float(got[m, n])!r}, ref {float(c.ref[m, n])!r}"
    print(f"BOUND gelu kernel={kernel} {M}x{N}x{c.K} largest error/bound={worst:.3f}")


@pytest.mark.parametrize("kernel,epi", [(k, e) for k in (1, 4, 5, 6, 7, 8) for e in (0, 2, 3) if not (k >= 7 and e == 3)])
def test_gaussian_operands_per_element(dev, kernel, epi):
    """Gaussian operands against float64, per element: (K + 2) 2^-23 (|A| |W|^T + |bias|) (+ 2^-11 |ref| for an fp16 output; epilogue 3: gemm_exact_cases.py)."""
    M, N, K = gc.GAUSS_SHAPES[kernel]
    c = gc.gauss_case(M, N, K, epi)
    with selected(kernel):
        if kernel < 7:
            assert hip.gemm_plan(M, N, K) == kernel
        rc, out = _gemm_f16(dev, c, "dense")
    assert rc == 0
    out = out.cpu()
    assert not gc.touched_positions(out, M, N)
    ratio = (out[:M, :N].double() - c.ref).abs() / c.bound
    worst = float(ratio.max())
    m, n = divmod(int(ratio.argmax()), N)
    print(f"BOUND gauss kernel={kernel} epilogue={epi} {M}x{N}x{K} largest error/bound={worst:.3f}")
    assert worst <= 1.0, f"kernel {kernel} epilogue {epi}: error / bound {worst:.3f} at ({m}, {n})"


def test_misaligned_operands_are_refused_with_real_buffers(dev):
    """The refusals of tests/test_gemm_exact_ref.py once more with real operands of a launchable shape: LFM_ERR_ALIGN, and the output keeps its sentinel."""
    c = gc.gemm_case(300, 260, 64, 0)
    M, N, K = c.M, c.N, c.K
    A, W, bias = gc.embed(c.A, K + 8, dtype=F16).to(dev), gc.embed(c.W, K + 8, dtype=F16).to(dev), gc.embed_vec(c.bias).to(dev)
    out = gc.out_buffer(M, N, N + 8, F16).to(dev)
    L, v = hip.lib(), C.c_void_p
    for lda, ldw, ldc, a_off, w_off in [(K + 4, K + 8, N + 8, 0, 0), (K + 8, K + 4, N + 8, 0, 0), (K + 8, K + 8, N + 2, 0, 0), (K + 8, K + 8, N + 8, 8, 0),
                                        (K + 8, K + 8, N + 8, 0, 8)]:
        rc = L.lfm_gemm_f16(v(A.data_ptr() + a_off), lda, v(W.data_ptr() + w_off), ldw, hip.ptr(out), ldc, M, N, K, hip.ptr(bias), 0, None, 0, 1, hip.stream_ptr())
        assert rc == ERR_ALIGN, (lda, ldw, ldc, a_off, w_off, rc)
        rc = L.lfm_linear_f16(v(A.data_ptr() + a_off), lda, v(W.data_ptr() + w_off), ldw, hip.ptr(out), ldc, M, N, K, hip.ptr(bias), None, hip.stream_ptr())
        assert rc == ERR_ALIGN, (lda, ldw, ldc, a_off, w_off, rc)
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())
