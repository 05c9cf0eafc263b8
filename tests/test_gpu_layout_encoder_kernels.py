"""The two kernels the layout encoder added (include/lfm_hip.h): lfm_token_embed_f16 bit for bit, and lfm_linear_gelu_f16 on every GEMM kernel the chooser
can give it, element by element against float64.  Cases, references and the derived bound: tests/layout_encoder_cases.py (pinned on the CPU in
tests/test_layout_encoder_ref.py); operand layouts, NaN pads, guard rows and sentinels: tests/gemm_exact_cases.py."""
import pytest
import torch

import gemm_exact_cases as gc
import layout_encoder_cases as ec
from lfm_amd import hip

pytestmark = pytest.mark.gpu

F16, F32 = torch.float16, torch.float32
ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -5


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


# ------------------------------------------------------------------------------------------------ lfm_token_embed_f16
def _embed_call(dev, D, L, ids=None):
    """-> (out buffer [N * L + guard rows, D] pre-filled with the sentinel, device tables, device ids, the case)."""
    tok, pos, case_ids, ref = ec.embed_case(D, L)
    ids = case_ids if ids is None else ids
    out = gc.out_buffer(ids.numel(), D, D, F16).to(dev)
    dt, dp, di = tok.to(dev), pos.to(dev), ids.to(dev)
    hip.token_embed(dt, dp, di, out=out[:ids.numel()])
    torch.cuda.synchronize()
    return out, dt, dp, di, ref


@pytest.mark.parametrize("L", ec.EMBED_LENGTHS)
@pytest.mark.parametrize("D", ec.EMBED_WIDTHS)
def test_token_embed_bit_exact(dev, D, L):
    tok, pos, ids, ref = ec.embed_case(D, L)
    assert not torch.equal(ref, (tok[ids].half() + pos[:L].half()).reshape(ref.shape))  # the case tells an fp16 add from the fp32 add rounded once
    out, *_ = _embed_call(dev, D, L)
    M = ids.numel()
    gc.assert_exact(out, ref.double(), M, D, f"token_embed D={D} L={L}")  # and the sentinel rows after the output are untouched


@pytest.mark.parametrize("D,L", [(8, 1), (128, 17), (512, 92)])
def test_token_embed_poisons_ids_outside_the_table(dev, D, L):
    """ids -1 and vocab (an IndexError in the reference): their rows are NaN, every other row is untouched by it, nothing is read beyond the table."""
    tok, pos, ids, ref = ec.embed_case(D, L)
    bad = ids.clone()
    flat = bad.view(-1)
    rows = sorted({0, flat.numel() - 1} if flat.numel() > 2 else {0})
    flat[rows[0]] = -1
    flat[rows[-1]] = ec.EMBED_VOCAB if len(rows) > 1 else -1
    out, *_ = _embed_call(dev, D, L, bad)
    got = out[:flat.numel()].cpu()
    assert not gc.touched_positions(out.cpu(), flat.numel(), D)
    for r in range(flat.numel()):
        if r in rows:
            assert bool(got[r].isnan().all()), (r, got[r])
        else:
            assert torch.equal(got[r], ref[r]), r
    # further out: ids that would index far beyond the table in either direction
    flat[rows[0]], flat[rows[-1]] = -(2 ** 40), 2 ** 40
    out, *_ = _embed_call(dev, D, L, bad)
    assert bool(out[rows[0]].isnan().all()) and bool(out[rows[-1]].isnan().all())


def test_token_embed_refusals_come_before_any_launch(dev):
    D, L = 128, 17
    tok, pos, ids, _ = ec.embed_case(D, L)
    N = ids.shape[0]
    out = gc.out_buffer(N * L, D, D, F16).to(dev)
    dt, dp, di = tok.to(dev), pos.to(dev), ids.to(dev)
    Lb, st = hip.lib(), hip.stream_ptr()

    def call(t=hip.ptr(dt), p=hip.ptr(dp), i=hip.ptr(di), o=hip.ptr(out), pos_rows=ec.EMBED_POS_ROWS, L_=L, D_=D, N_=N):
        return Lb.lfm_token_embed_f16(t, ec.EMBED_VOCAB, p, pos_rows, i, o, N_, L_, D_, st)

    assert call(D_=12) == ERR_SHAPE and call(D_=0) == ERR_SHAPE  # D % 8
    assert call(pos_rows=L - 1) == ERR_SHAPE  # L <= pos_rows
    assert call(L_=ec.EMBED_POS_ROWS + 1) == ERR_SHAPE
    assert call(N_=0) == ERR_SHAPE and call(L_=0) == ERR_SHAPE
    assert call(t=hip.ptr(dt.reshape(-1)[1:])) == ERR_ALIGN and call(p=hip.ptr(dp.reshape(-1)[2:])) == ERR_ALIGN
    assert call(i=hip.ptr(di.reshape(-1)[1:])) == ERR_ALIGN  # int64 ids 8 bytes off a 16-byte boundary
    assert call(o=hip.ptr(out.reshape(-1)[4:])) == ERR_ALIGN
    assert call(t=None) == ERR_ARG and call(p=None) == ERR_ARG and call(i=None) == ERR_ARG and call(o=None) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())
    assert call() == 0


def test_token_embed_captured_replay_follows_rewritten_ids(dev):
    D, L = 128, 17
    tok, pos, ids, ref = ec.embed_case(D, L)
    dt, dp, di = tok.to(dev), pos.to(dev), ids.to(dev)
    out = torch.empty(ids.numel(), D, dtype=F16, device=dev)
    hip.token_embed(dt, dp, di, out=out)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.token_embed(dt, dp, di, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), ref)
    other = torch.flip(ids, [0, 1]).contiguous()
    assert not torch.equal(other, ids)
    di.copy_(other.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), (tok[other] + pos[:L]).half().reshape(-1, D))


# ------------------------------------------------------------------------------------------------ lfm_linear_gelu_f16
def _gelu(dev, c, layout):
    da, dw, dc = gc.LAYOUTS[layout]
    A, W = gc.embed(c.A, c.K + da, dtype=F16).to(dev), gc.embed(c.W, c.K + dw, dtype=F16).to(dev)
    bias = gc.embed_vec(c.bias).to(dev)
    out = gc.out_buffer(c.M, c.N, c.N + dc, F16).to(dev)
    rc = hip.lib().lfm_linear_gelu_f16(hip.ptr(A), c.K + da, hip.ptr(W), c.K + dw, hip.ptr(out), c.N + dc, c.M, c.N, c.K, hip.ptr(bias), hip.stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0, (rc, layout)
    return out.cpu()


@pytest.mark.parametrize("kernel", ec.KERNEL_SELECTIONS)
def test_linear_gelu_per_element(dev, kernel):
    worst = 0.0
    with selected(kernel):
        for _, M, N, K in ec.kernel_shapes():
            assert hip.gemm_plan(M, N, K) == (kernel or 1), f"selection {kernel} at {M} x {N} x {K} runs kernel {hip.gemm_plan(M, N, K)}"
            c = ec.gelu_case(M, N, K)
            for layout in ec.KERNEL_LAYOUTS:
                out = _gelu(dev, c, layout)
                assert not gc.touched_positions(out, M, N)
                got = out[:M, :N].double()
                assert not bool(got.isnan().any())
                ratio = (got - c.ref).abs() / c.bound
                r = float(ratio.max())
                m, nn = divmod(int(ratio.argmax()), N)
                assert r <= 1.0, (f"kernel {kernel} {layout} {M}x{N}x{K}: error / bound {r:.3f} at ({m}, {nn}): x = {float(c.pre[m, nn])}, got {float(got[m, nn])!r}, "
                                  f"ref {float(c.ref[m, nn])!r}")
                worst = max(worst, r)
    print(f"BOUND gelu kernel={kernel} largest error/bound={worst:.3f}")
    assert worst > 0.05  # (the bound is not vacuous: an fp16 rounding alone reaches about a third of it)


@pytest.mark.parametrize("kernel", ec.KERNEL_SELECTIONS)
def test_linear_gelu_zero_accumulator_is_gelu_of_the_bias_rounded_once(dev, kernel):
    """Integer-valued operands whose dot products are all exactly zero, biases in [-3, -1.5]: every row is fp16(gelu_erf(bias)) bit for bit -- one rounding --
    which the tanh form misses in most columns; pads and guard rows untouched."""
    n = 0
    with selected(kernel):
        for _, M, N, K in ec.kernel_shapes():
            c = ec.gelu_zero_acc_case(M, N, K)
            for layout in ec.KERNEL_LAYOUTS:
                gc.assert_exact(_gelu(dev, c, layout), c.ref.half().double(), M, N, f"gelu(bias) kernel {kernel} {layout} {M}x{N}x{K}", hip.gemm_plan(M, N, K))
                n += 1
    print(f"EXACT gelu(bias) select={kernel} cases={n}")


def test_linear_gelu_refusals_come_before_any_launch(dev):
    c = ec.gelu_case(192, 64, 64)
    da, dw, dc = gc.LAYOUTS["wide"]
    A, W = gc.embed(c.A, c.K + da, dtype=F16).to(dev), gc.embed(c.W, c.K + dw, dtype=F16).to(dev)
    bias = gc.embed_vec(c.bias).to(dev)
    out = gc.out_buffer(c.M, c.N, c.N + dc, F16).to(dev)
    L, st = hip.lib(), hip.stream_ptr()
    lda, ldw, ldc = c.K + da, c.K + dw, c.N + dc

    def call(a=hip.ptr(A), b=hip.ptr(bias), lda_=lda, ldc_=ldc, K=c.K):
        return L.lfm_linear_gelu_f16(a, lda_, hip.ptr(W), ldw, hip.ptr(out), ldc_, c.M, c.N, K, b, st)

    assert call(b=None) == ERR_ARG  # the bias is required
    assert call(a=None) == ERR_ARG
    assert call(lda_=lda + 4) == ERR_ALIGN and call(ldc_=ldc + 2) == ERR_ALIGN and call(a=hip.ptr(A.reshape(-1)[4:])) == ERR_ALIGN
    assert call(K=48) == ERR_SHAPE  # K % 64, as lfm_linear_silu_f16
    torch.cuda.synchronize()
    assert bool((out == gc.SENTINEL).all())
