"""The LayerNorm-modulate paths of the DiT block loops on the device, per element against float64 (tests/dit_ln_cases.py; bounds derived there and shown
sound by tests/test_dit_ln_ref.py).

  A  lfm_ln_modulate: its five kernels (the default, the three flag variants of ln_modulate8_kernel, the 8-byte-store ln_modulate_kernel by flag, by
     width and by alignment of the output) on every case x family, with a sentinel behind the output and NaN guard rows behind the inputs;
  B  splitk_finish_resid_ln_kernel in the latency loop and in the split-K loop;
  C  the folded path: the producer's partials and A', the published row means, the consumer's statistics through the fc1 activation.

B and C observe a depth-1 forward whose gate_mlp rows are zero: fc2 adds 0 x finite, so the workspace still holds the block's residual stream X1 and
what the LayerNorm paths computed from it (hip.dit_workspace_layout says where).  The float64 references are computed from the X1 READ BACK, so they do not
depend on attention or on the GEMMs in front.  Every forward and every kernel runs twice and the outputs are bit-equal; every flag and option is restored.
"""
import collections
import ctypes as C
import functools

import pytest
import torch

import dit_ends_cases as dc
import dit_ln_cases as lc

pytestmark = pytest.mark.gpu

from lfm_amd import hip


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


def with_flags(flags, fn):
    hip.gemm_select(flags << 4)
    try:
        return fn()
    finally:
        hip.gemm_select(0)


def with_option(opt, value, default, fn):
    hip.set_option(opt, value)
    try:
        return fn()
    finally:
        hip.set_option(opt, default)


# ============================================================================= A: lfm_ln_modulate
SENTINEL = 12344.0  # exact in fp16
LN_KERNELS = {  # name -> (flag, output offset in fp16 elements from a 16-byte boundary, the cases it runs)
    "default": (0, 0, lambda c: True),
    "bpermute": (hip.DBG_LN_BPERMUTE, 0, lambda c: True),
    "two-rows": (hip.DBG_LN_TWO_ROWS, 0, lambda c: True),
    "four-rows": (hip.DBG_LN_FOUR_ROWS, 0, lambda c: True),
    "store8-flag": (hip.DBG_LN_STORE8, 0, lambda c: True),
    "store8-width": (0, 0, lambda c: c.D % 8 == 4),
    "store8-alignment": (0, 4, lambda c: c.D % 8 == 0),
}


def _ln_call(X, out, M, D, tokens, shift, scale, stride):
    return hip.lib().lfm_ln_modulate(hip.ptr(X), hip.ptr(out), M, D, tokens, hip.ptr(shift), hip.ptr(scale), stride, hip.stream_ptr())


@pytest.mark.parametrize("kernel", list(LN_KERNELS))
def test_ln_modulate_per_element(dev, kernel):
    """Every case (widths 8 .. 1280 with one active lane, ragged chunks and the full register budget; 1 .. 37 rows ragged against 4, 8 and 16 rows per
    workgroup; 2051 rows; per-image rows at 1, 5, 16 tokens, a shared row, a wide stride) x every family against float64 within the DIRECT bound, no
    element exempt; constant rows give fp16(shift) bit for bit; the sentinel behind the last output row survives, the NaN rows behind X and behind the
    modulation rows are not read into any output."""
    flag, off, runs = LN_KERNELS[kernel]
    worst, n = 0.0, 0
    for case in lc.LN_CASES:
        if not runs(case):
            continue
        for fam in lc.FAMILIES:
            X, buf, shift, scale, ref, bound = lc.ln_case(case, fam)
            M, D = case.M, case.D
            Xd = torch.full((M + 1, D), float("nan"), device=dev)
            Xd[:M] = X.to(dev)
            md = torch.full((buf.shape[0] + 1, buf.shape[1]), float("nan"), device=dev)
            md[:-1] = buf.to(dev)
            assert Xd.data_ptr() % 16 == 0
            stride = 0 if case.rows == 0 else buf.shape[1]
            outs = []
            for _ in range(2):
                raw = torch.full((off + M * D + 64,), SENTINEL, device=dev, dtype=torch.float16)
                assert raw.data_ptr() % 16 == 0
                out = raw[off:]
                rc = with_flags(flag, lambda: _ln_call(Xd, out, M, D, case.tokens, md, md[:, D:], stride))
                assert rc == 0, (case.name, rc)
                torch.cuda.synchronize()
                assert bool((raw[:off] == SENTINEL).all()) and bool((out[M * D:] == SENTINEL).all()), (case.name, fam, "wrote outside the output")
                outs.append(out[:M * D].reshape(M, D).cpu())
            assert torch.equal(outs[0], outs[1]), (case.name, fam)
            got = outs[0]
            assert bool(torch.isfinite(got).all()), (case.name, fam)
            r = lc.ratio(got, ref, bound)
            worst, n = max(worst, r), n + 1
            assert r <= 1.0, (kernel, case.name, fam, r)
            if fam == "constant":
                idx = lc.image_of_row(M, shift.shape[0], case.tokens)
                assert torch.equal(got, shift[idx].half()), (case.name, "constant rows")
    print(f"BOUND ln_modulate kernel={kernel} {n} case x family runs largest error/bound={worst:.3f}")


def test_ln_modulate_refusals(dev):
    X = torch.zeros(4, 1288, device=dev)
    A = torch.zeros(4, 1288, device=dev, dtype=torch.float16)
    mod = torch.zeros(2 * 1288, device=dev)
    for M, D, tokens in ((4, 6, 1), (4, 1284, 1), (4, 1288, 1), (0, 64, 1), (-1, 64, 1), (4, 64, 0), (4, 64, -2)):
        assert _ln_call(X, A, M, D, tokens, mod, mod[D:], 0) == -1, (M, D, tokens)  # LFM_ERR_SHAPE
    null = C.c_void_p(None)
    L = hip.lib()
    for args in ((null, hip.ptr(A), hip.ptr(mod), hip.ptr(mod)), (hip.ptr(X), null, hip.ptr(mod), hip.ptr(mod)), (hip.ptr(X), hip.ptr(A), null, hip.ptr(mod)),
                 (hip.ptr(X), hip.ptr(A), hip.ptr(mod), null)):
        assert L.lfm_ln_modulate(args[0], args[1], 4, 64, 1, args[2], args[3], 0, hip.stream_ptr()) == -5  # LFM_ERR_ARG
    torch.cuda.synchronize()
    assert not bool(A.any())  # nothing was launched


# ============================================================================= the depth-1 models of B and C
def ln_state(shape, seed, tier, family, gate=None, beta=None):
    """dit_ends_cases.make_state with gate_msa's bias N(0, 0.1) (or the constant `gate`) and gate_mlp's zero; gate = 0: the identity twin.  beta: a
    constant proj bias (the mean-shift family)."""
    sd = dc.make_state(shape, seed, tier, "massive_mid" if family == "massive" else "gauss")
    D = shape.hidden
    b = sd["blocks.0.adaLN_modulation.1.bias"]
    b[2 * D:3 * D] = torch.randn(D, generator=torch.Generator().manual_seed(seed * 31 + 5)) * 0.1 if gate is None else float(gate)
    if beta is not None:
        sd["blocks.0.attn.proj.bias"][:] = float(beta)
    return sd


def build(shape, sd, dev):
    from lfm_amd.models import DiT

    m = DiT(**dc.model_kwargs(shape))
    m.load_state_dict(sd, strict=True)
    return m.to(dev).eval()


def read_ws(m, shape, batch, rows):
    """Clones of what a forward at this batch left in the workspace: X [M, D] fp32, A / A2 [M, D] fp16, act = QKVH as [M, H] fp16, the block's modulation
    rows [rows, 6 D], ln_part [M, D / 256, 2], cen0 / cen1 [M]."""
    lay = hip.dit_workspace_layout(m.shape_struct(), batch)
    ws = m._ws[1]
    D, H = shape.hidden, 4 * shape.hidden
    M = batch * dc.tokens_of(shape)
    J = shape.depth * 6 * D + 2 * D
    P = max(D // 256, 1)

    def take(name, count, dtype, size):
        assert name == "X" or lay[name] > 0, name
        return ws[lay[name]:lay[name] + count * size].view(dtype).clone()

    out = {"X": take("X", M * D, torch.float32, 4).reshape(M, D), "A": take("A", M * D, torch.float16, 2).reshape(M, D),
           "act": take("QKVH", M * H, torch.float16, 2).reshape(M, H), "mod": take("mod", rows * J, torch.float32, 4).reshape(rows, J)[:, :6 * D]}
    if D % 256 == 0:
        out["A2"] = take("A2", M * D, torch.float16, 2).reshape(M, D)
        out["part"] = take("ln_part", M * P * 2, torch.float32, 4).reshape(M, P, 2)
        out["cen0"], out["cen1"] = take("cen0", M, torch.float32, 4), take("cen1", M, torch.float32, 4)
    return out


def forward_twice(m, shape, batch, x, t, y, **kw):
    """Two forwards, their outputs and every buffer read back bit-equal; the buffers of the first."""
    rows = 1 if (y is None and t.numel() == 1) else batch
    snaps = []
    for _ in range(2):
        out = m._run(t, x, y, False, 1.0, **kw).clone()
        torch.cuda.synchronize()
        assert bool(torch.isfinite(out).all())
        s = read_ws(m, shape, batch, rows)
        s["out"] = out
        snaps.append(s)
    for k in snaps[0]:  # the BITS (a buffer the path does not write holds whatever it held, NaN patterns included)
        a, b = snaps[0][k], snaps[1][k]
        assert torch.equal(a.view(torch.int16 if a.dtype == torch.float16 else torch.int32), b.view(torch.int16 if b.dtype == torch.float16 else torch.int32)), k
    return snaps[0]


def inputs(shape, batch, seed, per_image, dev):
    x = dc.make_x(shape, batch, seed).to(dev)
    if not per_image:
        return x, torch.tensor(dc.T_SCALAR, device=dev), None
    y = ((torch.arange(batch) * 3 + 1) % (dc.NUM_CLASSES + 1)).to(dev)
    return x, torch.linspace(0.05, 0.95, batch).to(dev), y


def mlp_rows(s, shape):
    D = shape.hidden
    return s["mod"][:, 3 * D:4 * D], s["mod"][:, 4 * D:5 * D]  # shift_mlp, scale_mlp as the device holds them


# ============================================================================= B: the finish kernel of the latency and the split-K loop
LATENCY_SHAPES = [dc.Shape(384, 6, 2, 4, 32), dc.Shape(1024, 16, 2, 4, 32), dc.Shape(1024, 16, 2, 4, 16), dc.Shape(1152, 16, 2, 4, 32), dc.Shape(1280, 20, 2, 4, 8)]
SPLITK_SHAPES = [dc.Shape(384, 6, 2, 4, 16), dc.Shape(1024, 16, 2, 4, 16)]


def _check_finish(s, shape, tag):
    T = dc.tokens_of(shape)
    shift, scale = mlp_rows(s, shape)
    X = s["X"].double()
    r = lc.ratio(s["A"], lc.ln_ref(X, shift, scale, T), lc.ln_bound(X, shift, scale, T))
    print(f"BOUND finish-LN {tag} D={shape.hidden} M={X.shape[0]} largest error/bound={r:.3f}")
    assert r <= 1.0, (tag, r)
    return r


@pytest.mark.parametrize("shape", LATENCY_SHAPES, ids=lambda s: f"D{s.hidden}-res{s.res}")
def test_finish_ln_latency_loop(dev, shape):
    """Batch 1: ws.A = LayerNorm-modulate(ws.X; shift_mlp, scale_mlp) per element after the latency loop's proj finish (D = 384: a quarter-filled block of the
    kernel; 1152: the second column chunk partly filled; 1280 at res 8: 16 rows) and, with OPT_SKINNY_GEMM 0, on the path that replaces it.  The two
    runs' X differ in their bits, or the latency loop did not run."""
    sd = ln_state(shape, 41, "A", "gauss")
    m = build(shape, sd, dev)
    x, t, y = inputs(shape, 1, 41, False, dev)
    s = forward_twice(m, shape, 1, x, t, y)
    D = shape.hidden
    assert torch.equal(s["mod"][0].cpu(), sd["blocks.0.adaLN_modulation.1.bias"])  # tier A: the device's rows are the fp32 biases
    assert float((s["X"] - build_identity_x(shape, 41, "A", "gauss", 1, False, dev)).abs().max()) > 0  # the block really updated the stream
    _check_finish(s, shape, "latency")
    alt = with_option(hip.OPT_SKINNY_GEMM, 0, 1, lambda: forward_twice(m, shape, 1, x, t, y))
    _check_finish(alt, shape, "latency-off")
    assert not torch.equal(s["X"], alt["X"]), "OPT_SKINNY_GEMM changed nothing: the latency loop (splitk_finish_resid_ln_kernel) did not run"


@pytest.mark.parametrize("shape", SPLITK_SHAPES, ids=lambda s: f"D{s.hidden}")
def test_finish_ln_splitk_loop(dev, shape):
    """Batch 3 with per-image conditioning (labels, the null row included, and a t per image): the rows of one launch take different modulation rows.  At
    <= 256 token rows the latency loop comes first, so the split-K loop is the one OPT_SKINNY_GEMM 0 leaves; DBG_GEMM_NO_SPLITK then replaces its finish by
    the plain GEMM and lfm_ln_modulate.  All three satisfy the bound; X differs between split-K on and off, or the finish kernel did not run."""
    sd = ln_state(shape, 43, "B", "gauss")
    m = build(shape, sd, dev)
    x, t, y = inputs(shape, 3, 43, True, dev)
    s_lat = forward_twice(m, shape, 3, x, t, y)
    shift = mlp_rows(s_lat, shape)[0]
    assert not torch.equal(shift[0], shift[1]) and not torch.equal(shift[1], shift[2])  # the images' rows really differ
    _check_finish(s_lat, shape, "latency-3-images")
    s = with_option(hip.OPT_SKINNY_GEMM, 0, 1, lambda: forward_twice(m, shape, 3, x, t, y))
    _check_finish(s, shape, "split-K")
    alt = with_option(hip.OPT_SKINNY_GEMM, 0, 1, lambda: with_flags(hip.DBG_GEMM_NO_SPLITK, lambda: forward_twice(m, shape, 3, x, t, y)))
    _check_finish(alt, shape, "split-K-off")
    assert not torch.equal(s["X"], alt["X"]), "DBG_GEMM_NO_SPLITK changed nothing: the split-K finish did not run"
    assert not torch.equal(s["X"], s_lat["X"]), "OPT_SKINNY_GEMM changed nothing at batch 3"


# ============================================================================= C: the folded path
@functools.lru_cache(maxsize=2)
def _identity_x(shape, seed, tier, family, batch, per_image, flags, dev):
    m = build(shape, ln_state(shape, seed, tier, family, gate=0.0), dev)
    x, t, y = inputs(shape, batch, seed, per_image, dev)
    return with_flags(flags, lambda: forward_twice(m, shape, batch, x, t, y))["X"]


def build_identity_x(shape, seed, tier, family, batch, per_image, dev, flags=0):
    """x0 [M, D]: ws.X after a forward of the twin whose gate_msa is zero too (the identity model of test_gpu_dit_ends.py)."""
    return _identity_x(shape, seed, tier, family, batch, per_image, flags, dev)


FoldCase = collections.namedtuple("FoldCase", "name shape batch per_image")
FOLD_CASES = [FoldCase("D256-one-slot", dc.Shape(256, 4, 2, 4, 32), 192, False), FoldCase("D512-two-slots", dc.Shape(512, 8, 2, 4, 32), 96, False),
              FoldCase("D1280-five-slots", dc.Shape(1280, 20, 2, 4, 32), 39, False), FoldCase("D256-tiles-span-4-images", dc.Shape(256, 4, 2, 4, 16), 768, False),
              FoldCase("D512-class-conditional", dc.Shape(512, 8, 2, 4, 32), 96, True)]
FOLD_FAMILIES = ("gauss", "massive", "r0", "r1", "r8", "r64")
R_TABLE = {}  # (case, select, family) -> (r, folded worst rel-L2, separate worst rel-L2, folded error/bound): printed as the envelope table


def _check_rows(M, seed):
    tiles = M // 256
    rows = torch.cat([torch.arange(256), torch.arange(256) + (tiles // 2) * 256, torch.arange(256) + (tiles - 1) * 256,
                      torch.randperm(M, generator=torch.Generator().manual_seed(seed))[:64]])
    return torch.unique(rows)


def _act_error(s, shape, W1, b1, sel):
    """(largest error/bound, largest per-row rel-L2) of the fc1 activation on the checked rows against float64 from the X1 and c read back."""
    T = dc.tokens_of(shape)
    shift, scale = mlp_rows(s, shape)
    idx = torch.div(sel, T, rounding_mode="floor")
    f = lc.fold_ref(s["X"][sel], s["c"][sel], shift, scale, W1, b1, idx)
    got = s["act"][sel].double()
    return float(((got - f.act).abs() / f.e_act).max()), float(((got - f.act).norm(dim=1) / f.act.norm(dim=1)).max())


def run_fold_case(case, family, select, dev, flags=0):
    shape, batch = case.shape, case.batch
    D, T = shape.hidden, dc.tokens_of(shape)
    M = batch * T
    tier, seed = ("B" if case.per_image else "A"), 51 + FOLD_CASES.index(case)
    base = "massive" if family == "massive" else "gauss"
    x0 = build_identity_x(shape, seed, tier, base, batch, case.per_image, dev, flags)
    gate = beta = None
    if family.startswith("r"):  # gate_msa = 1, proj bias = beta: every row mean moves by about beta = r x the rows' standard deviation
        gate, beta = 1.0, float(family[1:]) * float(x0.double().std(dim=1).mean())
    sd = ln_state(shape, seed, tier, base, gate, beta)
    m = build(shape, sd, dev)
    x, t, y = inputs(shape, batch, seed, case.per_image, dev)
    kw = dict(gemm_select=hip.call_gemm_select(select)) if select else {}
    plan = with_flags(flags, lambda: hip.dit_plan(m.shape_struct(), batch, t.numel(), y is not None, gemm_select=kw.get("gemm_select", 0)))
    assert plan & hip.PLAN_FOLDED_LN, (case.name, "the fold does not run")
    fused_runs = [True, False] if plan & hip.PLAN_FUSED_QKV_ATTENTION else [False]
    W1, b1 = sd["blocks.0.mlp.fc1.weight"].half().to(dev), sd["blocks.0.mlp.fc1.bias"].to(dev)
    sel = _check_rows(M, seed).to(dev)
    worst = {}
    for fused in fused_runs:
        def go():
            p = hip.dit_plan(m.shape_struct(), batch, t.numel(), y is not None, gemm_select=kw.get("gemm_select", 0))
            assert p & hip.PLAN_FOLDED_LN and bool(p & hip.PLAN_FUSED_QKV_ATTENTION) == fused
            return forward_twice(m, shape, batch, x, t, y, **kw)

        s = with_flags(flags, go) if fused else with_flags(flags, lambda: with_option(hip.OPT_FUSED_QKV_ATTENTION, 0, 1, go))
        ap_dev = s["A"] if fused else s["A2"]  # dit.hip: the fused kernel hands A' back through ws.A
        s["c"] = s["cen1"]
        shift, scale = mlp_rows(s, shape)
        if tier == "A":
            assert torch.equal(s["mod"][0].cpu(), sd["blocks.0.adaLN_modulation.1.bias"])
        f = lc.fold_ref(s["X"], s["c"], shift, scale, None, None, T)
        f0 = lc.fold_ref(x0, s["c"], shift, scale, None, None, T)
        r1 = lc.ratio(s["cen0"], f.mean, f.e_cen)  # 1: the fc1 consumer published the row means of X1
        r2 = lc.ratio(s["cen1"], f0.mean, f0.e_cen)  # 2: the qkv consumer published the row means of x0
        assert bool(torch.isfinite(s["part"]).all())
        r3 = float(((s["part"].double() - f.part).abs() / torch.clamp(f.e_part, min=1e-300)).max())  # 3: every row, every slot, in order
        r4 = lc.ratio(ap_dev, f.aprime, f.e_aprime)  # 4
        share = float((ap_dev == lc.aprime_emulate(s["X"], s["c"], scale, T)).double().mean())
        r5, rel = _act_error(s, shape, W1, b1, sel)  # 5
        tag = f"{case.name} {family} select={select} fused={fused} flags={flags:#x}"
        print(f"BOUND folded {tag}: r {float(f.r.min()):.2f} .. {float(f.r.max()):.2f}; largest error/bound: cen0 {r1:.3f}, cen1 {r2:.3f}, partials {r3:.3f}, "
              f"A' {r4:.3f} (bit-equal to the fp32 emulation: {100 * share:.3f} %), fc1 activation {r5:.3f} (worst row rel-L2 {rel:.2e})")
        assert max(r1, r2, r3, r4, r5) <= 1.0, (tag, r1, r2, r3, r4, r5)
        worst[fused] = (float(f.r.mean()), rel, r5)
    if family.startswith("r") and flags == 0:  # the same model with separate LayerNorm launches: figures only
        s = forward_twice(m, shape, batch, x, t, y, fold_ln=hip.CALL_OFF, **kw)
        s["c"] = s["X"].double().mean(1).float()
        _, rel_sep = _act_error(s, shape, W1, b1, sel)
        r, rel, r5 = worst[fused_runs[0]]
        R_TABLE[(case.name, select, family)] = (r, rel, rel_sep, r5)
        print(f"ENVELOPE {case.name} select={select} r={r:.2f}: fc1 activation worst row rel-L2 folded {rel:.2e}, separate {rel_sep:.2e}; folded error/bound {r5:.3f}")


@pytest.mark.parametrize("family", FOLD_FAMILIES)
@pytest.mark.parametrize("select", [0, 6], ids=["eight-wave", "four-wave"])
@pytest.mark.parametrize("case", FOLD_CASES, ids=lambda c: c.name)
def test_folded_path(dev, case, select, family):
    """cen[0], cen[1], ln_part, A' and the fc1 activation of the folded loop against float64 from the X1 and c read back (checks 1 to 5 of the cases module's
    FOLDED bounds): one, two and five partial slots, 256-row tiles spanning four images, one modulation row per image; the 8-wave and the 4-wave producer
    epilogue; with the fused QKV + attention kernel (A' in ws.A) and without (ws.A2) where the plan reports it; gauss, massive channels and the mean-shift
    family r = |mean(X1) - c| / std(X1) ~ 0, 1, 8, 64, each held to the bound at the rows' OWN r."""
    run_fold_case(case, family, select, dev)


def test_folded_path_after_ln_center_mod_kernel(dev):
    """DBG_DIT_PATCH_ROUND1: the embedding is off its MFMA kernel, so ln_center_mod_kernel plays the first producer.  cen[1] is then the mean that kernel put
    into slot 0, re-summed by the qkv consumer; checks 1 to 5 hold unchanged.  The kernel's own A' cannot be observed from outside -- attention overwrites
    it (ws.A) or the proj producer does (fused) -- and no entry point is added for it: its arithmetic is held through cen[1] here and through the whole-forward
    parity tests."""
    for family in ("gauss", "r8"):
        run_fold_case(FOLD_CASES[1], family, 0, dev, flags=hip.DBG_DIT_PATCH_ROUND1)
