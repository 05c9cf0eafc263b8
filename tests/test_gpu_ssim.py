"""lfm_ssim_u8 and lfm_ssim_f32 (include/lfm_hip.h, csrc/ssim.h) on the GPU, through the C ABI: every case of tests/ssim_cases.py inside its derived bound
against the unmodified reference in fp64 (tests/golden/ssim.pt; the GPU tests never read the reference), with NaN sentinels around `out`, sentinels around
`mask_sum` and a poisoned workspace; identical images exactly 1.0f; the mask sums exact; the word and the byte path, bytes and floats, alone and in a batch,
a first and a second run bit for bit alike; a NaN staying in its image; the refusals; one call captured in a graph and replayed on rewritten inputs."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import ssim_cases as sc
from lfm_amd import hip

pytestmark = pytest.mark.gpu

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "ssim.pt"), weights_only=False)
GUARD = 8
ONE = 0x3F800000  # 1.0f
ARG, SHAPE, ALIGN = -5, -1, -2


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def bits(t):
    return t.contiguous().view(torch.int32).tolist()


def put_bytes(dev, arr, off=0):
    """The bytes of `arr` on the device at byte offset `off` of a 256-byte aligned allocation -> (the view, its keeper)."""
    flat = torch.from_numpy(np.ascontiguousarray(arr)).reshape(-1)
    buf = torch.zeros(flat.numel() + off + 16, dtype=torch.uint8, device=dev)
    assert buf.data_ptr() % 256 == 0
    buf[off:off + flat.numel()].copy_(flat)
    return buf[off:off + flat.numel()]


def run(dev, kind, a, b, ws, mask=None, off=0, window=None):
    """One call through the C ABI -> (out fp32 [N] on the host, mask_sum int64 [N] or None).  out sits between NaNs, mask_sum between sentinels, the
    workspace is filled with 0xFF bytes (NaN partials, huge mask partials) and is exactly as large as the library asks."""
    L = hip.lib()
    if kind == "u8":
        N, H, W, _ = a.shape
        Cn = 3
        da, db = put_bytes(dev, a, off), put_bytes(dev, b, off)
    else:
        N, Cn, H, W = a.shape
        da, db = torch.from_numpy(np.ascontiguousarray(a)).to(dev), torch.from_numpy(np.ascontiguousarray(b)).to(dev)
    dm = put_bytes(dev, mask, off) if mask is not None else None
    w = (hip.ssim_gaussian(ws) if window is None else window).to(dev)
    need = L.lfm_ssim_workspace_bytes(N, H, W)
    assert need == (N * -(-H // sc.TILE) * -(-W // sc.TILE) * 8 + 15) // 16 * 16
    wsp = torch.full((need + 32,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((N + 2 * GUARD,), float("nan"), device=dev)
    msum = torch.full((N + 2 * GUARD,), -77, dtype=torch.int64, device=dev)
    o_ptr, m_ptr = C.c_void_p(out.data_ptr() + 4 * GUARD), C.c_void_p(msum.data_ptr() + 8 * GUARD)
    if kind == "u8":
        rc = L.lfm_ssim_u8(hip.ptr(da), hip.ptr(db), hip.ptr(dm), N, H, W, hip.ptr(w), ws, hip.ptr(wsp), need, o_ptr, m_ptr if mask is not None else None,
                           hip.stream_ptr())
    else:
        rc = L.lfm_ssim_f32(hip.ptr(da), hip.ptr(db), N, Cn, H, W, hip.ptr(w), ws, hip.ptr(wsp), need, o_ptr, hip.stream_ptr())
    assert rc == 0, rc
    torch.cuda.synchronize()
    out, msum, wsp = out.cpu(), msum.cpu(), wsp.cpu()
    assert bool(out[:GUARD].isnan().all()) and bool(out[N + GUARD:].isnan().all()), "wrote outside out"
    assert bool((msum[:GUARD] == -77).all()) and bool((msum[N + GUARD:] == -77).all()), "wrote outside mask_sum"
    assert bool((wsp[need:] == 0xFF).all()), "wrote outside the workspace"
    if mask is None:
        assert bool((msum == -77).all())
    return out[GUARD:N + GUARD].clone(), msum[GUARD:N + GUARD].clone() if mask is not None else None


@pytest.mark.parametrize("case", sc.all_cases(), ids=[c[0] for c in sc.all_cases()])
def test_every_case_inside_its_bound_against_the_reference_in_fp64(dev, case):
    d = sc.inputs(case)
    ref, bound = GOLDEN["cases"][case[0]]["ref64"].numpy(), sc.bound(d["a64"], d["b64"], d["ws"])
    got, _ = run(dev, d["kind"], d["a"], d["b"], d["ws"])
    err = np.abs(got.numpy().astype(np.float64) - ref)
    print(f"BOUND ssim {case[0]}: error {err.max():.2e}, bound {bound.max():.2e}, error / bound {(err / bound).max():.3f}")
    assert np.all(err <= bound)
    if case[1] in ("self", "zeros"):  # an image against itself, zeros against zeros: exactly 1.0f
        assert bits(got) == [ONE] * len(got)


@pytest.mark.parametrize("N,H,W", [(2, 13, 29), (2, 40, 72), (1, 33, 65)])
def test_mask_sums_are_exact(dev, N, H, W):
    a, b = sc.make_u8("pm3", N, H, W)
    rng = np.random.RandomState(H)
    for mask in (rng.randint(0, 256, (N, H, W)).astype(np.uint8), np.full((N, H, W), 255, np.uint8)):
        plain, _ = run(dev, "u8", a, b, 11)
        for off in (0, 1):
            got, sums = run(dev, "u8", a, b, 11, mask=mask, off=off)
            assert sums.tolist() == mask.astype(np.int64).sum(axis=(1, 2)).tolist()
            assert bits(got) == bits(plain)  # the mask does not touch the score


@pytest.mark.parametrize("family", ["random", "ramp"])
def test_word_path_and_byte_path_give_the_same_bits(dev, family):
    N, H, W = 2, 40, 72  # W % 4 == 0: words when the pointers are aligned, bytes at an odd offset
    a, b = sc.make_u8(family, N, H, W)
    mask = np.random.RandomState(3).randint(0, 256, (N, H, W)).astype(np.uint8)
    aligned, sums0 = run(dev, "u8", a, b, 11, mask=mask, off=0)
    for off in (1, 2, 3):
        odd, sums1 = run(dev, "u8", a, b, 11, mask=mask, off=off)
        assert bits(odd) == bits(aligned) and sums1.tolist() == sums0.tolist()


@pytest.mark.parametrize("N,H,W,ws", [(2, 13, 29, 11), (2, 40, 72, 11), (1, 33, 65, 7)])
def test_bytes_and_their_unit_floats_give_the_same_bits(dev, N, H, W, ws):
    a, b = sc.make_u8("random", N, H, W)
    got_u8, _ = run(dev, "u8", a, b, ws)
    got_f32, _ = run(dev, "f32", sc.unit32(a), sc.unit32(b), ws)
    assert bits(got_u8) == bits(got_f32)


def test_an_image_scores_the_same_alone_anywhere_in_a_batch_and_again(dev):
    H, W = 40, 72
    a, b = sc.make_u8("random", 3, H, W)
    alone, _ = run(dev, "u8", a[1:2], b[1:2], 11)
    for pos in range(3):
        order = [1 if k == pos else other for k, other in enumerate([0, 2, 0])]  # image 1 at `pos`, other images around it
        batch, _ = run(dev, "u8", a[order], b[order], 11)
        assert bits(batch[pos:pos + 1]) == bits(alone), pos
        again, _ = run(dev, "u8", a[order], b[order], 11)
        assert bits(again) == bits(batch)


def test_a_nan_stays_in_its_image(dev):
    a, b = sc.make_f32(3, 3, 40, 72)
    clean, _ = run(dev, "f32", a, b, 11)
    a = a.copy()
    a[1, 2, 17, 40] = np.nan
    got, _ = run(dev, "f32", a, b, 11)
    assert bool(got[1].isnan()) and bits(got[[0, 2]]) == bits(clean[[0, 2]])


def test_refusals_come_before_any_launch(dev):
    L = hip.lib()
    N, H, W = 2, 16, 16
    a, b = (torch.zeros(N, H, W, 3, dtype=torch.uint8, device=dev) for _ in range(2))
    fa, fb = (torch.zeros(N, 3, H, W, device=dev) for _ in range(2))
    mask = torch.zeros(N, H, W, dtype=torch.uint8, device=dev)
    w = hip.ssim_gaussian(11).to(dev)
    need = L.lfm_ssim_workspace_bytes(N, H, W)
    wsp = torch.full((need + 32,), 0xFF, dtype=torch.uint8, device=dev)
    out = torch.full((N + 2,), float("nan"), device=dev)
    msum = torch.full((N + 2,), -77, dtype=torch.int64, device=dev)
    p, st = hip.ptr, hip.stream_ptr()
    at = lambda t, k: C.c_void_p(t.data_ptr() + k)  # noqa: E731
    u8 = lambda **k: L.lfm_ssim_u8(*[k.get(n, v) for n, v in (("a", p(a)), ("b", p(b)), ("mask", p(mask)), ("N", N), ("H", H), ("W", W), ("w", p(w)),  # noqa: E731
                                                                ("ws", 11), ("wsp", p(wsp)), ("need", need), ("out", p(out)), ("msum", p(msum)), ("st", st))])
    f32 = lambda **k: L.lfm_ssim_f32(*[k.get(n, v) for n, v in (("a", p(fa)), ("b", p(fb)), ("N", N), ("C", 3), ("H", H), ("W", W), ("w", p(w)), ("ws", 11),  # noqa: E731
                                                                  ("wsp", p(wsp)), ("need", need), ("out", p(out)), ("st", st))])
    for name in ("a", "b", "w", "wsp", "out"):
        assert u8(**{name: None}) == ARG and f32(**{name: None}) == ARG, name
    assert u8(msum=None) == ARG and u8(mask=None) == ARG  # mask_sum is NULL if and only if mask is
    for bad in (dict(N=0), dict(H=0), dict(W=0), dict(H=4097), dict(W=4097), dict(ws=1), dict(ws=13), dict(ws=4), dict(need=need - 1)):
        assert u8(**bad) == SHAPE and f32(**bad) == SHAPE, bad
    assert f32(C=0) == SHAPE and f32(C=5) == SHAPE
    for bad in (dict(w=at(w, 2)), dict(out=at(out, 2)), dict(wsp=at(wsp, 8))):
        assert u8(**bad) == ALIGN and f32(**bad) == ALIGN, bad
    assert u8(msum=at(msum, 4)) == ALIGN and f32(a=at(fa, 2)) == ALIGN and f32(b=at(fb, 1)) == ALIGN
    assert L.lfm_ssim_workspace_bytes(0, 16, 16) == 0 and L.lfm_ssim_workspace_bytes(1, 4097, 16) == 0 and L.lfm_ssim_workspace_bytes(1, 16, 0) == 0
    assert L.lfm_ssim_workspace_bytes(1, 4096, 4096) == 128 * 128 * 8
    torch.cuda.synchronize()
    assert bool(out.isnan().all()) and bool((msum == -77).all()) and bool((wsp == 0xFF).all())
    with pytest.raises(hip.LfmHipError, match="contiguous uint8"):
        hip.ssim_u8(fa, fb)
    with pytest.raises(hip.LfmHipError, match="window_size"):
        hip.ssim_u8(a, b, window_size=4)
    with pytest.raises(hip.LfmHipError, match="1 <= C <= 4"):
        hip.ssim_f32(torch.zeros(1, 5, 8, 8, device=dev), torch.zeros(1, 5, 8, 8, device=dev))
    with pytest.raises(hip.LfmHipError, match="no CPU fallback"):
        hip.ssim_f32(fa.cpu(), fb.cpu())


def test_the_wrappers_give_the_abi_calls_bits(dev):
    a, b = sc.make_u8("pm3", 2, 40, 72)
    mask = np.random.RandomState(5).randint(0, 256, (2, 40, 72)).astype(np.uint8)
    ref, sums = run(dev, "u8", a, b, 7, mask=mask)
    got, got_sums = hip.ssim_u8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev), torch.from_numpy(mask).to(dev), window_size=7)
    assert got.dtype == torch.float32 and got_sums.dtype == torch.int64 and bits(got.cpu()) == bits(ref) and got_sums.cpu().tolist() == sums.tolist()
    assert hip.ssim_u8(torch.from_numpy(a).to(dev), torch.from_numpy(b).to(dev))[1] is None
    f = hip.ssim_f32(torch.from_numpy(sc.unit32(a)).to(dev), torch.from_numpy(sc.unit32(b)).to(dev), window_size=7)
    assert bits(f.cpu()) == bits(ref)


def test_one_call_in_a_graph_follows_inputs_rewritten_in_place(dev):
    N, H, W = 2, 40, 72
    a, b = sc.make_u8("random", N, H, W)
    mask = np.random.RandomState(8).randint(0, 256, (N, H, W)).astype(np.uint8)
    da, db, dm = (torch.from_numpy(t).to(dev) for t in (a, b, mask))
    L, w = hip.lib(), hip.ssim_gaussian(11).to(dev)
    need = L.lfm_ssim_workspace_bytes(N, H, W)
    wsp = torch.empty(need, dtype=torch.uint8, device=dev)
    out, msum = torch.zeros(N, device=dev), torch.zeros(N, dtype=torch.int64, device=dev)

    def launch():
        assert L.lfm_ssim_u8(hip.ptr(da), hip.ptr(db), hip.ptr(dm), N, H, W, hip.ptr(w), 11, hip.ptr(wsp), need, hip.ptr(out), hip.ptr(msum), hip.stream_ptr()) == 0

    launch()  # warm-up outside the capture
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        launch()
    for a_, b_, m_ in ((a, b, mask), (*sc.make_u8("pm3", N, H, W, seed=4), np.full((N, H, W), 255, np.uint8))):
        for d, t in ((da, a_), (db, b_), (dm, m_)):
            d.copy_(torch.from_numpy(t).to(dev))
        out.zero_(), msum.zero_(), wsp.fill_(0xFF)
        graph.replay()
        torch.cuda.synchronize()
        eager, sums = run(dev, "u8", a_, b_, 11, mask=m_)
        assert bits(out.cpu()) == bits(eager) and msum.cpu().tolist() == sums.tolist() == m_.astype(np.int64).sum(axis=(1, 2)).tolist()
