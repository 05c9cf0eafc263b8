"""The two ends of the DiT forward on the device against float64 (tests/dit_ends_cases.py; tolerances shown sound by tests/test_dit_ends_ref.py).

Every case is a depth-1 model with zero adaLN gates (the block is the identity on the residual stream), built through lfm_amd.models.DiT and run
through its public entries.  Tier A (adaLN weights zero: the modulation rows are the fp32 biases) holds patch_embed_ln_kernel, patch_embed_kernel, the
patchify GEMM, final_layer_mfma_kernel and final_layer_kernel to TOL_A per image; tier B (per-image rows) holds rows and indexing to the per-forward
budget; the conditioning kernels are read back through DiT.cond_table.
"""
import functools

import pytest
import torch

import dit_ends_cases as dc
from dit_ends_cases import COND_TS, tier_b_inputs, uv_bound

pytestmark = pytest.mark.gpu

from lfm_amd import hip

ROUND1 = (hip.DBG_DIT_PATCH_ROUND1 | hip.DBG_DIT_FINAL_ROUND1) << 4  # the VALU twins of the two MFMA kernels


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def with_flags(flags, fn):
    hip.gemm_select(flags)
    try:
        return fn()
    finally:
        hip.gemm_select(0)


def build(shape, sd, dev):
    from lfm_amd.models import DiT

    m = DiT(**dc.model_kwargs(shape))
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


@functools.lru_cache(maxsize=4)
def tier_a_model(case, family, dev):
    return build(case.shape, dc.tier_a(case, family)[0], dev)


def twice(fn):
    """Run twice: the outputs are bit-equal (every kernel at the ends combines its partial sums in a fixed order)."""
    a = fn().clone()
    b = fn().clone()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    return a


def run_tier_a(case, family, flags, dev, euler):
    sd, x, ref, _ = dc.tier_a(case, family)
    m = tier_a_model(case, family, dev)
    xd = x.to(dev)
    if case.cfg:
        xd[case.batch // 2:] = float("nan")  # the kernels read x[n % (N / 2)]: the second half must never be touched
    t = torch.tensor(dc.T_SCALAR, device=dev)
    scale = dc.CFG_SCALE if case.cfg else 1.0

    def go():
        out = twice(lambda: m._run(t, xd, None, case.cfg, scale))
        assert bool(torch.isfinite(out).all())
        err = dc.worst(out.cpu(), ref)
        print(f"tier A {case.name} {family} flags={flags:#x}: {err:.2e}")
        assert err <= dc.TOL_A, err
        if not euler:
            return out
        g = torch.Generator().manual_seed(7)
        base = torch.randn(x.shape, generator=g)
        dt = torch.tensor([-0.25], device=dev)
        want = base.double() + float(dt.cpu()) * ref
        bd = base.to(dev)
        apart = twice(lambda: m._run(t, xd, None, case.cfg, scale, out=torch.empty_like(bd), axpy_base=bd, axpy_dt=dt))
        assert torch.equal(bd.cpu(), base)
        inplace = bd.clone()
        m._run(t, xd, None, case.cfg, scale, out=inplace, axpy_base=inplace, axpy_dt=dt)
        assert torch.equal(apart, inplace)
        err = dc.worst(apart.cpu(), want)
        print(f"tier A {case.name} {family} flags={flags:#x} fused Euler: {err:.2e}")
        assert err <= dc.TOL_A, err
        return out

    return with_flags(flags, go)


def _has_mfma(shape):
    return dc.embed_kind(shape) == "hilo" or dc.final_kind(shape) == "hilo"


TIER_A_RUNS = [(c, f, fl) for c in dc.TIER_A_CASES for f in c.families for fl in ((0, ROUND1) if _has_mfma(c.shape) else (0,))]


@pytest.mark.parametrize("case,family,flags", TIER_A_RUNS, ids=[f"{c.name}-{f}-{'round1' if fl else 'default'}" for c, f, fl in TIER_A_RUNS])
def test_tier_a(dev, case, family, flags):
    """Device against float64 per image at TOL_A, twice bit-equal, CFG with a NaN second half, the fused Euler update apart and in place (gauss), and
    -- on the default kernels -- the same bits with the block loop on a forced GEMM kernel: the ends do not depend on the loop, and zero gates make
    every loop the identity."""
    out = run_tier_a(case, family, flags, dev, euler=family == "gauss")
    if flags == 0 and family in ("gauss", "massive0"):
        sd, x, _, _ = dc.tier_a(case, family)
        m = tier_a_model(case, family, dev)
        xd = x.to(dev)
        if case.cfg:
            xd[case.batch // 2:] = float("nan")
        forced = m._run(torch.tensor(dc.T_SCALAR, device=dev), xd, None, case.cfg, dc.CFG_SCALE if case.cfg else 1.0, gemm_select=hip.call_gemm_select(1))
        assert torch.equal(out, forced)


@pytest.mark.parametrize("family", dc.FOLDED_CASE.families)
@pytest.mark.parametrize("flags", [0, ROUND1], ids=["default", "round1"])
def test_tier_a_folded_plan(dev, family, flags):
    """patch_embed_ln_kernel with A != nullptr (it also writes the first LayerNorm's operand, partials and row means) still writes the right X; with the
    round-1 embedding, ln_center_mod_kernel follows patch_embed_kernel."""
    case = dc.FOLDED_CASE
    m = tier_a_model(case, family, dev)
    assert with_flags(flags, lambda: hip.dit_plan(m.shape_struct(), case.batch)) & hip.PLAN_FOLDED_LN
    out = run_tier_a(case, family, flags, dev, euler=False)
    if flags == 0:
        xd = dc.tier_a(case, family)[1].to(dev)
        forced = m._run(torch.tensor(dc.T_SCALAR, device=dev), xd, None, False, 1.0, gemm_select=hip.call_gemm_select(1))
        assert hip.dit_plan(m.shape_struct(), case.batch, gemm_select=hip.call_gemm_select(1)) == 0
        assert torch.equal(out, forced)


# ----------------------------------------------------------------------------- tier B: per-image rows
@pytest.mark.parametrize("shape", dc.TIER_B_SHAPES, ids=lambda s: f"D{s.hidden}p{s.patch}c{s.in_ch}")
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_tier_b_per_image_rows(dev, shape, cfg):
    """Labels (the null row included) and t of length B, each alone and together: every image is modulated with its own row (mod_stride = J)."""
    batch = 6 if cfg else 5
    sd, x, y, t = tier_b_inputs(shape, batch)
    m = build(shape, sd, dev)
    xd = x.to(dev)
    if cfg:
        xd[batch // 2:] = float("nan")
    scale = dc.CFG_SCALE if cfg else None
    emb = dc.staged_embedding(sd, shape, x, cfg) if dc.embed_kind(shape) == "f16" else None  # the fp16-by-design embedding, as in tier A
    for tt, yy, what in ((torch.tensor(0.37), y, "labels"), (t, None, "t"), (t, y, "both")):
        ref = dc.exact(sd, shape, x, tt, yy, scale, embedding=emb)
        for flags in (0, ROUND1):
            out = with_flags(flags, lambda: twice(lambda: m._run(tt.to(dev), xd, None if yy is None else yy.to(dev), cfg, scale or 1.0)))
            assert bool(torch.isfinite(out).all())
            err = dc.worst(out.cpu(), ref)
            print(f"tier B D={shape.hidden} cfg={cfg} {what} flags={flags:#x}: {err:.2e}")
            assert err <= dc.TOL_B, err


# ----------------------------------------------------------------------------- conditioning through the table
COND_SHAPES = [dc.Shape(64, 1, 2, 4, 8), dc.Shape(384, 6, 2, 4, 8), dc.Shape(1024, 16, 2, 4, 8), dc.Shape(1280, 20, 2, 4, 8), dc.Shape(256, 4, 2, 4, 8, 3)]


@pytest.mark.parametrize("shape", COND_SHAPES, ids=lambda s: f"D{s.hidden}x{s.depth}")
def test_conditioning_table(dev, shape):
    """temb1 / temb2 / cond / adaLN GEMM / uv_gemv / cond_row_copy: every row of DiT.cond_table for ts = 0 .. 1 against the emulation (c in fp16), in
    the order of ts; the u, v rows of shapes that fold against float64 sums over the device's OWN modulation row and the fp16 weights."""
    sd = dc.make_state(shape, 31, "B")
    m = build(shape, sd, dev)
    D, H, depth, n = shape.hidden, 4 * shape.hidden, shape.depth, len(COND_TS)
    J = depth * 6 * D + 2 * D
    uv = depth * 2 if D % 256 == 0 else 0  # dit.hip: dit_fold_capable
    row_floats = J + uv * 3 * D + uv * H
    ts = torch.tensor(COND_TS, device=dev)
    tab = twice(lambda: m.cond_table(ts, 1))
    assert tab.numel() == 4 * n * row_floats
    rows = tab.view(torch.float32).reshape(n, row_floats).cpu().double()
    assert bool(torch.isfinite(rows).all())
    ref = dc.conditioning(sd, shape, COND_TS, None, n, staged=True)
    errs = dc.image_errors(rows[:, :J], ref)
    print(f"cond table D={D} depth={depth}: " + ", ".join(f"t={t:g} {float(e):.2e}" for t, e in zip(COND_TS, errs)))
    assert float(errs.max()) <= dc.TOL_COND, errs
    dist = (rows[:, None, :J] - ref[None]).norm(dim=2)  # [device row, reference row]: every row is nearest to its own time
    assert dist.argmin(dim=1).tolist() == list(range(n)), dist
    if not uv:
        return
    uvq = rows[:, J:J + uv * 3 * D].reshape(n, depth, 2, 3 * D)
    uvf = rows[:, J + uv * 3 * D:].reshape(n, depth, 2, H)
    for i in range(depth):
        mod = rows[:, i * 6 * D:(i + 1) * 6 * D]
        for name, got, wkey, sh, sc in (("qkv", uvq[:, i], f"blocks.{i}.attn.qkv.", mod[:, 0:D], mod[:, D:2 * D]),
                                        ("fc1", uvf[:, i], f"blocks.{i}.mlp.fc1.", mod[:, 3 * D:4 * D], mod[:, 4 * D:5 * D])):
            W, b = sd[wkey + "weight"].half().double(), sd[wkey + "bias"].double()
            a = (1.0 + sc.float()).double()  # the kernel's fp32 1 + scale
            u, v = a @ W.T, sh @ W.T + b
            ubound = uv_bound(D) * (a.abs() @ W.abs().T)
            vbound = uv_bound(D) * (sh.abs() @ W.abs().T + b.abs())
            ru, rv = float(((got[:, 0] - u).abs() / ubound).max()), float(((got[:, 1] - v).abs() / vbound).max())
            print(f"  block {i} {name}: |u - ref| / bound {ru:.2f}, |v - ref| / bound {rv:.2f}")
            assert ru <= 1.0 and rv <= 1.0, (name, ru, rv)


def test_forward_with_the_table_is_bit_identical(dev):
    """One evaluation at scalar t with its conditioning computed in the call and one that copies the row of a table: the same bits."""
    case = dc.TIER_A_CASES[0]
    shape = case.shape
    sd = dc.make_state(shape, 31, "B")
    m = build(shape, sd, dev)
    x = dc.make_x(shape, case.batch, 3).to(dev)
    ts = torch.tensor(COND_TS, device=dev)
    table = m.cond_table(ts, case.batch)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    for row, tv in enumerate(COND_TS):
        t = torch.tensor(tv, device=dev)
        plain = m(t, x).clone()
        tabled = m._run(t, x, None, False, 1.0, cond=(table, step, row, len(COND_TS)))
        assert torch.equal(plain, tabled), tv
