"""GPU tests of the layout UNet (``UNetModelAttn``: SpatialTransformers with HIP cross-attention) against the unmodified reference
(tests/golden/layout_{tiny,self}.pt, tools/make_layout_golden.py): the velocity for two context lengths and both time forms, that the context reaches the
right image, the once-per-context K / V projection and its invalidation, a 10-step Euler solve, and ``context=None`` with labels by keyword."""
from argparse import Namespace
import os

import pytest
import torch

import layout_cases as lc

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _model(golden_dir, name):
    from lfm_amd.models.unet import UNetModelAttn

    rec = torch.load(os.path.join(golden_dir, name), map_location="cpu", weights_only=False)
    m = UNetModelAttn(**rec["cfg"])
    checksum = lc.load_seeded(m, rec["state_seed"])
    assert abs(checksum - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"], "the seeded state differs from the one the reference was run with"
    return rec, m.to("cuda:0").eval()


@pytest.fixture(scope="module")
def tiny(golden_dir):
    return _model(golden_dir, "layout_tiny.pt")


def _count_projections(m):
    """Wrap the host's context projection; returns the list its calls are appended to."""
    calls, inner = [], m._project_context

    def counted(ctx16):
        calls.append(tuple(ctx16.shape))
        return inner(ctx16)

    m._project_context = counted
    return calls


def test_layout_tiny_matches_reference_golden(tiny):
    rec, m = tiny
    dev = torch.device("cuda:0")
    x = rec["x"].to(dev)
    errs = {}
    for L in lc.CONTEXT_LENGTHS:
        ctx = rec[f"ctx{L}"].to(dev)
        assert float(rec[f"v_tN_L{L}"].abs().mean()) > 1e-2
        errs[f"t0d L={L}"] = rel_l2(m(torch.tensor(0.6, device=dev), x, ctx), rec[f"v_t0d_L{L}"])
        errs[f"tN L={L}"] = rel_l2(m(rec["tN"].to(dev), x, ctx.float()), rec[f"v_tN_L{L}"])  # any float dtype
    print("layout_tiny rel-L2 vs reference:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < 3e-3, errs
    assert rel_l2(rec["v_tN_L17"], rec["v_tN_L77"]) > 1e-2  # the two contexts are two different answers


def test_each_image_attends_over_its_own_context(tiny):
    rec, m = tiny
    dev = torch.device("cuda:0")
    x, t, ctx = rec["x"].to(dev), rec["tN"].to(dev), rec["ctx77"].to(dev)
    a = m(t, x, ctx).clone()
    b = m(t, x, ctx[[1, 0, 2]].contiguous()).clone()
    moved = [rel_l2(b[i], a[i]) for i in (0, 1)]
    print("images 0 and 1 under each other's context: rel-L2", [f"{e:.3e}" for e in moved])
    assert min(moved) > 1e-2 and torch.equal(a[2], b[2])


def test_context_is_projected_once_per_context(tiny):
    rec, m = tiny
    dev = torch.device("cuda:0")
    x, t, ctx = rec["x"].to(dev), rec["tN"].to(dev), rec["ctx17"].to(dev)
    calls = _count_projections(m)
    try:
        a = m(t, x, ctx).clone()
        n0 = len(calls)
        assert n0 == 1 and calls[0] == (3 * 17, 512)  # ONE GEMM of N * L rows for every attn2 of the network
        b = m(torch.tensor(0.3, device=dev), x, ctx)  # another time, the same context: nothing to project
        assert len(calls) == n0
        assert torch.equal(a, m(t, x, context=ctx)) and len(calls) == n0  # by keyword: the same bits, still cached
        assert not torch.equal(a, b)
        ctx.mul_(1)  # an in-place edit bumps the version: the cache cannot know the values are the same
        assert torch.equal(a, m(t, x, ctx)) and len(calls) == n0 + 1
        m(t, x, ctx.clone())  # another tensor
        assert len(calls) == n0 + 2
        gen = m._gen
        m.load_state_dict(m.state_dict())  # new weights: the projection of the old ones is dropped
        assert m._gen > gen and torch.equal(a, m(t, x, ctx)) and len(calls) == n0 + 3
    finally:
        del m._project_context


def test_layout_tiny_euler_solve(tiny):
    from lfm_amd.test_flow_latent import sample_from_model

    rec, m = tiny
    dev = torch.device("cuda:0")
    x, ctx = rec["x"].to(dev), rec["ctx17"].to(dev)
    args = Namespace(method="euler", step_size=0.1, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)
    calls = _count_projections(m)
    try:
        first = sample_from_model(m, x, dict(context=ctx), args)[-1].clone()
        n0 = len(calls)
        second = sample_from_model(m, x, dict(context=ctx), args)[-1]
    finally:
        del m._project_context
    err = rel_l2(first, rec["x_euler10"])
    print(f"layout_tiny 10 Euler steps vs reference: {err:.3e}; context projections in the first solve {n0}, in the second {len(calls) - n0}")
    assert err < 1e-3
    assert torch.equal(first, second)
    if not getattr(m, "_fused_solvers", None):  # an eager solve: ten evaluations, at most one projection, none in the second solve
        assert n0 == 1 and len(calls) == n0


def test_captured_forward_projects_the_context_inside_the_graph(tiny):
    """Under capture the context projection is part of the graph and the eager cache is neither read nor written: after ``static_ctx.copy_(other)`` a replay
    is the forward on the other context.  The static tensor keeps its shape, so the other context is the L = 77 fixture context with its images permuted
    (the L = 17 one cannot be copied into it).  Captured against eager at the project's bound for that pair, 1e-5 rel-L2 (tests/test_gpu_song_unet.py:230)."""
    rec, m = tiny
    dev = torch.device("cuda:0")
    x, t = rec["x"].to(dev), rec["tN"].to(dev)
    ctx_a = rec["ctx77"].to(dev)
    ctx_b = ctx_a[[2, 0, 1]].contiguous()
    static_ctx = ctx_a.clone()
    eager_a = m(t, x, static_ctx).clone()  # the usual eager warm-up: packs, grows the scratch, and caches the projection of static_ctx
    key, kv, src = m._ctx_key, m._ctx_kv, m._ctx_src
    assert src is static_ctx
    kv_before = kv.clone()
    calls = _count_projections(m)
    try:
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(t, x, static_ctx)
        assert len(calls) == 1  # projected in the graph although the eager cache holds this very tensor
        assert m._ctx_key is key and m._ctx_kv is kv and m._ctx_src is src  # the capture did not touch the cache
        graph.replay()
        torch.cuda.synchronize()
        e_same = rel_l2(out, eager_a)
        static_ctx.copy_(ctx_b)
        graph.replay()
        torch.cuda.synchronize()
        replay_b = out.clone()
        assert torch.equal(kv, kv_before)  # no captured kernel writes the cached buffer
        assert len(calls) == 1  # a replay runs no Python
        eager_b = m(t, x, ctx_b)
        assert len(calls) == 2
    finally:
        del m._project_context
    e_other, moved = rel_l2(replay_b, eager_b), rel_l2(replay_b, eager_a)
    print(f"captured forward vs eager: same context {e_same:.3e}, after copy_ of another context {e_other:.3e}; the two contexts differ by {moved:.3e}")
    assert e_same < 1e-5 and e_other < 1e-5 and moved > 1e-2


def test_strided_context_views_are_told_apart(tiny):
    rec, m = tiny
    dev = torch.device("cuda:0")
    x, t = rec["x"].to(dev), rec["tN"].to(dev)
    base = rec["ctx77"].to(dev)[:, :34].contiguous()
    a, b = base[:, :17], base[:, ::2]  # the same first element, shape, dtype and version; other strides
    assert a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() != b.stride()
    va = m(t, x, a).clone()
    vb = m(t, x, b)
    assert torch.equal(vb, m(t, x, b.contiguous())) and torch.equal(va, m(t, x, a.contiguous())) and not torch.equal(va, vb)


def test_training_mode_is_refused(tiny):
    from lfm_amd import hip

    rec, m = tiny
    dev = torch.device("cuda:0")
    try:
        with pytest.raises(hip.LfmHipError, match="inference-only"):
            m.train()(rec["tN"].to(dev), rec["x"].to(dev), rec["ctx17"].to(dev))
    finally:
        m.eval()


def test_layout_self_context_none_and_labels_by_keyword(golden_dir):
    rec, m = _model(golden_dir, "layout_self.pt")
    dev = torch.device("cuda:0")
    x, y = rec["x"].to(dev), rec["y"].to(dev)
    a = m(rec["tN"].to(dev), x, y=y).clone()
    errs = dict(t0d=rel_l2(m(torch.tensor(0.6, device=dev), x, None, y=y), rec["v_t0d"]), tN=rel_l2(a, rec["v_tN"]))
    print("layout_self rel-L2 vs reference:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < 3e-3, errs
    with pytest.raises(AssertionError, match="class-conditional"):  # the third positional argument is the context, not y
        m(rec["tN"].to(dev), x, y)
    ctx = torch.randn(3, 9, 128, generator=torch.Generator().manual_seed(2)).to(dev)
    b = m(rec["tN"].to(dev), x, ctx, y)  # positionally: (t, x, context, y)
    assert torch.equal(b, m(rec["tN"].to(dev), x, y=y, context=ctx)) and rel_l2(b, a) > 1e-2
    with pytest.raises(ValueError, match="context must be"):
        m(rec["tN"].to(dev), x, ctx[:, :, :64], y=y)
