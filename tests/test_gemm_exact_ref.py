"""CPU side of the exact GEMM / conv3x3 tests (tests/gemm_exact_cases.py): the exactness caps over the complete case list, the int64 convolution
reference against torch's own convolution, the checker against four seeded faults, and the alignment refusals of the GEMM entry points (host code that
returns before any launch).  tests/test_gpu_gemm_exact.py runs the cases on the GPU."""
import ctypes as C

import pytest
import torch

import gemm_exact_cases as gc


def test_exactness_caps_hold_for_every_case():
    """Every integer case the GPU tests run: |ref| <= 2048 for the fp16 outputs, |ref| and sum_k |a_k w_k| below 2^24 for all (asserted by the builders)."""
    n, top16, top32 = gc.build_all_exact_cases()
    print(f"{n} integer cases; largest |ref|: {top16} (fp16 out, cap {gc.CAP16}), {top32} (fp32 out, cap {gc.CAP32})")
    assert n == 4 * len(gc.gemm_f16_cases()) + 2 * len(gc.latency_cases()) + len(gc.QKV_SHAPES) + len(gc.LINEAR_SHAPES) + sum(len(c[-1]) for c in gc.CONV_CASES)
    assert 0 < top16 <= gc.CAP16 and top32 < gc.CAP32
    assert top32 > gc.CAP16  # the fp32 cases leave the fp16-exact range: an accumulator handed over in fp16 cannot pass them


def test_case_lists_reach_the_paths_they_name():
    """Tile counts with the XCD remap off and on for every kernel; the latency shapes inside the kernels' contracts; the split-K thresholds."""
    for kernel, (bm, bn) in gc.TILES.items():
        if kernel in (7, 8):
            continue
        counts = [-(-M // bm) * -(-N // bn) for M, N in gc.GEMM_SHAPES]
        assert any(c % 8 for c in counts) and any(c % 8 == 0 for c in counts), (kernel, counts)
        assert all(M % bm and N % bn and M > bm and N > bn for M, N in gc.GEMM_SHAPES)  # ragged and interior tiles in both directions
    assert all(M % 64 == 0 and N % 64 == 0 for M, N in gc.LATENCY_SHAPES[7]) and all(M <= 256 and N % 16 == 0 for M, N in gc.LATENCY_SHAPES[8])
    assert {(N // 64) % 8 == 0 for M, N in gc.LATENCY_SHAPES[7]} == {False, True}  # kernel 7's plain and XCD-grouped tile orders
    for path, N, H, W, Cin, Cout, modes in gc.CONV_CASES:
        assert H != W and Cin % 64 == 0 and Cout % 4 == 0 and (1 not in modes or (H % 2 == 0 and W % 2 == 0))
        s256 = gc.splitk256_slices(N * H * W, Cout, 9 * Cin, 1 << 40)
        assert (s256 > 0) == (path == "splitk256"), (path, s256)
    # the 256x256 split-K shape is minimal: one row tile fewer, one column tile fewer or the next narrower input does not split
    assert gc.splitk256_slices(2048, 2048, 9 * 384, 1 << 40) == 2
    assert not gc.splitk256_slices(2047, 2048, 9 * 384, 1 << 40) and not gc.splitk256_slices(2048, 1792, 9 * 384, 1 << 40)
    assert not gc.splitk256_slices(2048, 2048, 9 * 320, 1 << 40)


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_conv_reference_is_the_convolution(mode):
    """The int64 im2col (tap-major weights, fused upsample, stride 2) against torch.nn.functional.conv2d in float64 on a non-square map."""
    N, H, W, Cin, Cout = 2, 6, 10, 64, 8
    c = gc.conv_case(N, H, W, Cin, Cout, mode)
    Hi, Wi = gc.conv_input_size(H, W, mode)
    x = c.x.double().reshape(N, Hi, Wi, Cin).permute(0, 3, 1, 2)
    if mode == 1:
        x = torch.nn.functional.interpolate(x, scale_factor=2, mode="nearest")
    w = c.Wt.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2)
    y = torch.nn.functional.conv2d(x, w, c.bias.double(), stride=2 if mode == 2 else 1, padding=1)
    assert y.shape[-2:] == (H, W)
    want = y.permute(0, 2, 3, 1).reshape(N * H * W, Cout) + c.resid.double()
    assert torch.equal(want, c.ref.double())


def _correct_buffer(c, ldc):
    buf = gc.out_buffer(c.M, c.N, ldc, c.out_dtype)
    buf[:c.M, :c.N] = c.ref.to(c.out_dtype)
    return buf


@pytest.mark.parametrize("epi", [0, 2])
def test_checker_reports_seeded_faults(epi):
    """A correct result corrupted four ways: each fault is reported, at its place, and nothing else is."""
    M, N, K = 300, 260, 320
    c = gc.gemm_case(M, N, K, epi)
    ldc = N + 4
    good = _correct_buffer(c, ldc)
    r = gc.check(good, c.ref, M, N, kernel=5)
    assert not r.diffs and not r.touched and "untouched" in r.message

    # one element off by one k-term (the last term of the tail K-tile dropped) -- at a position where that term is not zero
    m, n = next((m, n) for m in range(257, M) for n in range(256, N) if int(c.A[m, K - 1] * c.W[n, K - 1]) != 0)
    bad = good.clone()
    bad[m, n] -= float(c.A[m, K - 1] * c.W[n, K - 1])
    r = gc.check(bad, c.ref, M, N, kernel=5)
    assert r.diffs == [[m, n]] and not r.touched
    assert f"({m}, {n}) tile (1, 1) of kernel 5" in r.message and "1 of 78000 elements differ" in r.message

    # two columns exchanged inside one 4-column store group
    m, n = next((m, n) for m in range(M) for n in range(128, N, 4) if int(c.ref[m, n + 1]) != int(c.ref[m, n + 2]))
    bad = good.clone()
    bad[m, n + 1], bad[m, n + 2] = good[m, n + 2], good[m, n + 1]
    r = gc.check(bad, c.ref, M, N, kernel=1)
    assert r.diffs == [[m, n + 1], [m, n + 2]] and not r.touched and f"tile ({m // 128}, {n // 128}) of kernel 1" in r.message

    # one pad element overwritten
    bad = good.clone()
    bad[17, N + 1] = 3.0
    r = gc.check(bad, c.ref, M, N, kernel=4)
    assert not r.diffs and r.touched == [[17, N + 1]] and "pad column" in r.message and "guard row" not in r.message

    # one row past M written
    bad = good.clone()
    bad[M, :N] = good[M - 1, :N]
    r = gc.check(bad, c.ref, M, N, kernel=4)
    assert not r.diffs and r.touched == [[M, n] for n in range(N)] and "guard row" in r.message
    with pytest.raises(AssertionError, match="guard row"):
        gc.assert_exact(bad, c.ref, M, N, "seeded", kernel=4)

    # a NaN (a pad column read into a product) differs
    bad = good.clone()
    bad[5, 7] = float("nan")
    assert gc.check(bad, c.ref, M, N).diffs == [[5, 7]]


def test_real_valued_bounds_are_what_they_say():
    c = gc.gelu_case(300, 260)
    assert float(c.pre.min()) < -15 and float(c.pre.max()) > 15 and 0.7 < float((c.pre.abs() < 6).double().mean()) < 0.9
    assert torch.equal(c.pre * 8, (c.pre * 8).round())  # an exact multiple of 1/8
    assert bool(((c.ref != 0) & (c.ref.abs() < 2.0 ** -14)).any())  # the fp16-subnormal part of the negative tail is there
    assert torch.allclose(c.ref, torch.nn.functional.gelu(c.pre, approximate="tanh"), rtol=1e-12, atol=1e-300)
    # the reference rounded to fp16 sits within the bound with room for the kernel's own error
    assert float(((c.ref.half().double() - c.ref).abs() / c.bound).max()) <= 2.0 / 3.0 + 1e-9
    for epi in (0, 2, 3):
        g = gc.gauss_case(300, 260, 320, epi)
        assert bool((g.bound > 0).all()) and bool(g.ref.isfinite().all())
        # an fp32 product in torch's own order meets the bound (the bound is not one only this project's kernels can meet)
        t = g.A.float() @ g.W.float().t() + g.bias
        if epi == 3:
            t = g.X + g.gate.repeat_interleave(g.tokens, 0) * t
        if epi == 0:
            t = t.half()
        assert float(((t.double() - g.ref).abs() / g.bound).max()) < 1.0


# ------------------------------------------------------------------------------------------------ alignment refusals (host code: no launch, no GPU)
ALIGN, SHAPE = -2, -1
P = 0x10000  # a 16-byte-aligned non-null address; never dereferenced: with zero rows every entry point returns before any launch


@pytest.mark.parametrize("what,kw", [("lda", dict(lda=68)), ("ldw", dict(ldw=68)), ("ldc % 4", dict(ldc=66)), ("ldc odd", dict(ldc=65)), ("A", dict(A=P + 8)),
                                      ("W", dict(W=P + 8))])
def test_gemm_entry_points_refuse_misaligned_operands(what, kw):
    """lfm_gemm_f16 (every epilogue), lfm_gemm_qkv_f16 and lfm_linear_f16 return LFM_ERR_ALIGN for a leading dimension of A / W that is not a multiple of 8,
    an ldc that is not a multiple of 4 (every epilogue stores 4-element vectors at m * ldc + n) and a 16-byte-misaligned A / W -- with ZERO rows, so the
    refusal is seen to come first; the same call with aligned operands is refused for its shape instead."""
    from lfm_amd import hip

    L = hip.lib()
    v = C.c_void_p

    def gemm(epi, A=P, lda=64, W=P, ldw=64, ldc=64):
        return L.lfm_gemm_f16(v(A), lda, v(W), ldw, v(P), ldc, 0, 64, 64, v(P), epi, v(P), 0, 1, None)

    def qkv(A=P, lda=64, W=P, ldw=64, ldc=None):
        return L.lfm_gemm_qkv_f16(v(A), lda, v(W), ldw, v(P), v(P), v(P), 0, 64, 64, v(P), 64, 16, None)

    def linear(A=P, lda=64, W=P, ldw=64, ldc=64):
        return L.lfm_linear_f16(v(A), lda, v(W), ldw, v(P), ldc, 0, 64, 64, v(P), v(P), None)

    for epi in range(4):
        assert gemm(epi) == SHAPE and gemm(epi, **kw) == ALIGN, (what, epi)
    assert linear() == SHAPE and linear(**kw) == ALIGN, what
    assert qkv() == SHAPE
    if "ldc" not in kw:  # (no ldc: Q, K, V^T are dense)
        assert qkv(**kw) == ALIGN, what
    assert L.lfm_linear2_f16(v(P), 64, v(P), 64, v(P), kw.get("ldw", 128), v(P), kw.get("ldc", 64), 0, 64, v(P), v(P), None) == (
        ALIGN if ("ldw" in kw or "ldc" in kw) else SHAPE)
