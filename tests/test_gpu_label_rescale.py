"""lfm_label_rescale_f32 (include/lfm_hip.h, csrc/label_rescale.h), the one-kernel conditioning stage of mask-to-image synthesis: bit for bit against int64
arithmetic on integer weights, per element against float64 on Gaussian weights (and bit for bit against the fp32 emulation of its stated summation order),
NaN cells for labels outside the table, independence of batch size / place in the batch / label alignment, refusals before any launch, and a captured replay.
Cases, references, the derived bound and the named mistakes it excludes: tests/semantic_cond_cases.py (pinned on the CPU in tests/test_semantic_cond_ref.py)."""
import pytest
import torch

import semantic_cond_cases as sc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

SENTINEL, GUARD = -1234.0, 8


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _run(dev, labels, w, b, n_stages, label_offset=0):
    """-> (out on the host, the whole sentinel-guarded buffer on the host).  label_offset: elements the label map is shifted inside its buffer (1: 8-byte but
    not 16-byte aligned)."""
    N, H, W = labels.shape
    shape = (N, w.shape[0], H >> n_stages, W >> n_stages)
    numel = shape[0] * shape[1] * shape[2] * shape[3]
    buf = torch.full((numel + 2 * GUARD,), SENTINEL, device=dev)
    lbuf = torch.zeros(labels.numel() + 2, dtype=torch.int64, device=dev)
    assert lbuf.data_ptr() % 16 == 0
    dl = lbuf[label_offset:label_offset + labels.numel()].view(N, H, W)
    dl.copy_(labels)
    out = hip.label_rescale(dl, w.to(dev), b.to(dev) if b is not None else None, n_stages, out=buf[GUARD:GUARD + numel].view(shape))
    torch.cuda.synchronize()
    host = buf.cpu()
    assert bool((host[:GUARD] == SENTINEL).all()) and bool((host[GUARD + numel:] == SENTINEL).all()), "wrote outside out"
    return out.cpu(), host


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_integer_weights_bit_for_bit(dev, shape):
    """Weights and bias integers in [-8, 8]: the cell sums stay below 2^11 and the divisor is a power of two, so the int64 result is the only fp32 answer.  Every
    pixel outside the last whole cell holds the invalid label num_cls (at 43 x 43 and n_stages 2, 3: rows and columns 40..42; at n_stages 1 the whole cells
    reach row 41, so row and column 42): reading one would make a NaN."""
    n = 0
    for c in sc.exact_cases(shape):
        labels = sc.make_labels(c)
        w, b = sc.int_weights(c)
        ref = sc.exact_int(labels, w, b, c.n_stages)
        got, _ = _run(dev, sc.poison_ragged_edge(c, labels), w, b, c.n_stages)
        assert got.dtype == torch.float32 and got.shape == ref.shape and torch.equal(got.double(), ref), (sc.case_id(c), float((got.double() - ref).abs().max()))
        n += 1
    print(f"EXACT label_rescale {shape}: cases={n}")


def test_integer_weights_bit_for_bit_beyond_one_pass_of_the_grid(dev):
    """5 x 512 x 512 labels: more lanes than one pass of the workgroups holds, so every workgroup walks several tiles of the batch."""
    c = sc.Case(5, 512, 512, 182, 4, 3, True)
    labels = sc.make_labels(c)
    w, b = sc.int_weights(c)
    got, _ = _run(dev, labels, w, b, c.n_stages)
    assert torch.equal(got.double(), sc.exact_int(labels, w, b, c.n_stages))
    got1, _ = _run(dev, labels, w, b, c.n_stages, label_offset=1)  # one label per load: twice the lanes
    assert torch.equal(got1, got)


@pytest.mark.parametrize("shape", sc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_gaussian_weights_per_element(dev, shape):
    """|err| <= (P + 2) 2^-24 (sum_p |w[o, label_p]| / P + |b_o|) against the float64 restatement (cell mean of the one-hot map, then the matmul), and the very
    bits of the stated summation order (columns top to bottom, then a binary tree over the columns)."""
    worst = 0.0
    for c in [c for c in sc.gauss_cases() if (c.H, c.W) == shape]:
        labels = sc.make_labels(c)
        w, b = sc.gauss_weights(c)
        got, _ = _run(dev, labels, w, b, c.n_stages)
        r = sc.error_ratio(got, sc.restate64(labels, w, b, c.n_stages), sc.bound(labels, w, b, c.n_stages))
        print(f"BOUND label_rescale {sc.case_id(c)}: error / bound {r:.3f}")
        assert r <= 1.0, (sc.case_id(c), r)
        assert torch.equal(got, sc.emulate_kernel32(labels, w, b, c.n_stages)), sc.case_id(c)
        worst = max(worst, r)
    assert 0.0 < worst  # (fp32 sums of Gaussian weights do round)


def test_table_of_exactly_64_kib(dev):
    c = sc.Case(2, 16, 16, 2048, 8, 2, True)
    labels = sc.make_labels(c)
    w, b = sc.gauss_weights(c)
    got, _ = _run(dev, labels, w, b, c.n_stages)
    assert sc.error_ratio(got, sc.restate64(labels, w, b, c.n_stages), sc.bound(labels, w, b, c.n_stages)) <= 1.0
    assert torch.equal(got, sc.emulate_kernel32(labels, w, b, c.n_stages))


@pytest.mark.parametrize("c", [sc.Case(3, 16, 16, 19, 4, 1, True), sc.Case(3, 43, 43, 182, 4, 2, False), sc.Case(3, 72, 72, 151, 4, 3, True),
                               sc.Case(3, 48, 80, 19, 7, 4, True), sc.Case(3, 43, 43, 19, 4, 4, False)], ids=sc.case_id)
def test_labels_outside_the_table_poison_their_own_cell_only(dev, c):
    labels = sc.make_labels(c)
    w, b = sc.gauss_weights(c)
    clean, _ = _run(dev, labels, w, b, c.n_stages)
    assert not bool(clean.isnan().any())
    cs = 1 << c.n_stages
    h, wo = c.H >> c.n_stages, c.W >> c.n_stages
    spots = [(0, 0, 0, cs - 1, 0), (c.N - 1, h - 1, wo - 1, 0, cs - 1)]  # (image, cell row, cell column, row and column inside the cell)
    for too_big, negative in ((c.num_cls, -1), (2 ** 40, -(2 ** 40)), (2 ** 32, -(2 ** 63))):  # 2^32: 0 in its low half
        bad = labels.clone()
        for (n, i, j, dy, dx), v in zip(spots, (too_big, negative)):
            bad[n, i * cs + dy, j * cs + dx] = v
        got, _ = _run(dev, bad, w, b, c.n_stages)
        poisoned = torch.zeros_like(got, dtype=torch.bool)
        for n, i, j, _, _ in spots:
            poisoned[n, :, i, j] = True
        assert bool(got[poisoned].isnan().all()) and torch.equal(got[~poisoned], clean[~poisoned]), (too_big, negative)
    assert int(poisoned.sum()) == 2 * c.cout or h * wo * c.N == 1


@pytest.mark.parametrize("c", [sc.Case(3, 43, 43, 182, 4, 3, True), sc.Case(3, 48, 80, 151, 4, 3, False), sc.Case(3, 72, 72, 19, 5, 2, True),
                               sc.Case(3, 16, 16, 1024, 4, 4, True), sc.Case(3, 8, 8, 19, 4, 1, False)], ids=sc.case_id)
def test_result_does_not_depend_on_the_batch_or_the_alignment(dev, c):
    """encode(x[:1]) is encode(x)[:1], every image alone is its row of the batch, and labels that are only 8-byte aligned (one per load) give the same bits."""
    labels = sc.make_labels(c)
    w, b = sc.gauss_weights(c)
    full, _ = _run(dev, labels, w, b, c.n_stages)
    for k in range(c.N):
        one, _ = _run(dev, labels[k:k + 1], w, b, c.n_stages)
        assert torch.equal(one, full[k:k + 1]), k
    shifted, _ = _run(dev, labels, w, b, c.n_stages, label_offset=1)
    assert torch.equal(shifted, full)


def test_refusals_come_before_any_launch(dev):
    lab, w = torch.zeros(2 * 16 * 16 + 8, dtype=torch.int64, device=dev), torch.zeros(16400 * 9, device=dev)
    bias, out = torch.zeros(16, device=dev), torch.full((2 * 9 * 8 * 8 + 64,), SENTINEL, device=dev)
    for changed, offsets, expected, got in sc.refusals(hip.lib(), lab, w, bias, out, hip.stream_ptr()):
        assert got == expected, (changed, offsets, expected, got)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    b = sc.REFUSAL_BASE
    args = (b["N"], b["H"], b["W"], b["num_cls"], b["cout"], b["n_stages"])
    assert hip.lib().lfm_label_rescale_f32(hip.ptr(lab), hip.ptr(w), None, hip.ptr(out), *args, hip.stream_ptr()) == 0  # bias may be NULL
    torch.cuda.synchronize()
    n = b["N"] * b["cout"] * 2 * 2
    assert bool((out[:n] == 0).all()) and bool((out[n:] == SENTINEL).all())
    with pytest.raises(hip.LfmHipError, match="contiguous int64"):
        hip.label_rescale(lab[:512].view(2, 16, 16).int(), w[:76].view(4, 19), None, 3)
    with pytest.raises(hip.LfmHipError, match="out must be dense fp32"):
        hip.label_rescale(lab[:512].view(2, 16, 16), w[:76].view(4, 19), None, 3, out=torch.empty(2, 4, 2, 3, device=dev))
    with pytest.raises(hip.LfmHipError, match=r"lfm_label_rescale_f32 failed: .*\(code -1\)"):
        hip.label_rescale(lab[:512].view(2, 16, 16), w[:171].view(9, 19), None, 3)  # Cout 9


def test_captured_replay_follows_rewritten_labels(dev):
    c = sc.Case(3, 72, 72, 182, 4, 3, True)
    labels = sc.make_labels(c)
    w, b = sc.gauss_weights(c)
    dl, dw, db = labels.to(dev), w.to(dev), b.to(dev)
    out = torch.empty(c.N, c.cout, 9, 9, device=dev)
    hip.label_rescale(dl, dw, db, c.n_stages, out=out)  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        hip.label_rescale(dl, dw, db, c.n_stages, out=out)
    out.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), sc.emulate_kernel32(labels, w, b, c.n_stages))
    other = torch.flip(labels, [0, 2]).contiguous()
    assert not torch.equal(other, labels)
    dl.copy_(other.to(dev))
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.cpu(), sc.emulate_kernel32(other, w, b, c.n_stages))
