"""The yardsticks of the ``adm_context`` GPU tests, pinned on the CPU: the float64 restatements of tests/adm_context_cases.py against the unmodified
reference's recorded outputs (tests/golden/adm_context_tiny.pt), the seeded faults those bounds separate, the one-key identity of attn2, and the derived
per-element bounds of the two linear kernels against fp32 emulations.  No GPU."""
import os

import pytest
import torch

import adm_context_cases as ac

# The restatement is float64, the record fp32: what is measured below is the REFERENCE's fp32 round-off over ~25 layers (measured on the fixture:
# 6.2e-7 for v, 2.1e-7 for the lone block, 1.1e-6 for the guided combine, whose 1.5 (cond - uncond) amplifies it; profiles/adm_context_tests.txt).
# The bound is four times the largest of them.
CONTROL_BOUND = 4e-6
MODEL_BOUND = 3e-3  # the GPU model tests' rel-L2 bound: every seeded fault has to move v by ten times that


@pytest.fixture(scope="module")
def rec(golden_dir):
    return torch.load(os.path.join(golden_dir, "adm_context_tiny.pt"), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def state(rec):
    from lfm_amd.models.EDM import DhariwalUNet

    m = DhariwalUNet(**rec["cfg"])
    checksum = ac.load_seeded(m, rec["state_seed"])
    assert abs(checksum - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"]
    i = ac.inputs()
    assert abs(float(i.x.double().abs().sum()) - rec["x_checksum"]) <= 1e-9 * rec["x_checksum"]
    return {k: v.detach() for k, v in m.state_dict().items()}, i


@pytest.fixture(scope="module")
def restated(rec, state):
    """Computed once, shared, left unchanged."""
    sd, i = state
    t0 = torch.tensor(ac.T0D)
    return dict(v_t0d=ac.unet_ref64(sd, ac.TINY_CFG, t0, i.x, i.y), v_tN=ac.unet_ref64(sd, ac.TINY_CFG, i.tN[:2], i.x[:2], i.y[:2]),
                v_y2=ac.unet_ref64(sd, ac.TINY_CFG, t0, i.x[3:], i.y2), cfg_null=ac.cfg_ref64(sd, ac.TINY_CFG, t0, i.x, i.y_cfg_null)[:2],
                cfg_zero=ac.cfg_ref64(sd, ac.TINY_CFG, t0, i.x, i.y_cfg_zero)[:2])


def test_float64_restatement_reproduces_the_reference_records(rec, state, restated):
    sd, _ = state
    errs = {k: ac.rel_l2(v, rec[k]) for k, v in restated.items()}
    xb, yb = ac.block_input()
    ctx = sd["map_label.embedding_table.weight"][yb]
    pre = ac.BLOCK + ".transformer"
    errs["block (closed form of attn2)"] = ac.rel_l2(ac.transformer_ref64(sd, pre, xb, ctx), rec["block_out"])
    errs["block (attn2 as written)"] = ac.rel_l2(ac.transformer_ref64(sd, pre, xb, ctx, closed_form=False), rec["block_out"])
    print("float64 restatement vs the reference's fp32 records (control error), rel-L2:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < CONTROL_BOUND, errs
    assert rec["block_out"].shape == xb.shape and float(rec["block_out"].abs().mean()) > 0.5


def test_every_seeded_fault_moves_v_by_ten_times_the_model_bound(rec, state, restated):
    sd, i = state
    t0 = torch.tensor(ac.T0D)
    moved = {}
    for f in ac.FAULTS:
        if f == "cfg_null_row":  # a fault of the guided path: the record whose second half is class 0, evaluated with that half overwritten
            moved[f] = ac.rel_l2(ac.cfg_ref64(sd, ac.TINY_CFG, t0, i.x, i.y_cfg_zero, fault=f)[:2], rec["cfg_zero"])
        else:
            moved[f] = ac.rel_l2(ac.unet_ref64(sd, ac.TINY_CFG, t0, i.x, i.y, fault=f), rec["v_t0d"])
    print("seeded faults, rel-L2 of the restated v against the reference:", {k: f"{v:.3e}" for k, v in moved.items()})
    assert set(moved) == set(ac.FAULTS) and min(moved.values()) > 10 * MODEL_BOUND, moved
    # the faultless guided restatement with the null row IS the other record: the fault is the overwrite, not the label
    assert ac.rel_l2(ac.cfg_ref64(sd, ac.TINY_CFG, t0, i.x, i.y_cfg_zero, fault="cfg_null_row")[:2], rec["cfg_null"]) < CONTROL_BOUND


def test_attn2_has_one_key_its_query_side_is_never_read(rec, state, restated):
    """Softmax over ONE finite score is exp(0) / exp(0) = 1 exactly, whatever the score: attn2's output is proj(v(context)) at every pixel.  Drawing
    attn2.q / attn2.k anew changes no bit -- of the restated v (closed form) and of the block evaluated AS WRITTEN, q, k, softmax and all -- and the two
    forms agree to float64 round-off.  (A non-finite score -- inf - inf in the softmax -- would break the identity: DESIGN.md.)"""
    sd, i = state
    other = ac.redraw_attn2_qk(sd)
    assert not torch.equal(other[ac.BLOCK + ".transformer.attn2.q.weight"], sd[ac.BLOCK + ".transformer.attn2.q.weight"])
    assert torch.equal(ac.unet_ref64(other, ac.TINY_CFG, torch.tensor(ac.T0D), i.x, i.y), restated["v_t0d"])
    xb, yb = ac.block_input()
    ctx = sd["map_label.embedding_table.weight"][yb]
    pre = ac.BLOCK + ".transformer"
    written = ac.transformer_ref64(sd, pre, xb, ctx, closed_form=False)
    assert torch.equal(ac.transformer_ref64(other, pre, xb, ctx, closed_form=False), written)
    closed = ac.transformer_ref64(sd, pre, xb, ctx)
    d = float((written - closed).abs().max())
    # attn2 alone: no spatial variation at all, and the closed form to float64 round-off
    x = ac.gn64(xb.double(), sd, pre + ".norm2")
    a2 = ac.attn2_full64(sd, pre + ".attn2", x, ctx.double(), 2)
    u = ac.attn2_closed_form64(sd, pre + ".attn2", ctx.double())
    spread = float(a2.flatten(2).std(dim=2).max())
    print(f"attn2 as written vs closed form: block max |diff| {d:.3e}; attn2 spatial std {spread:.3e}; max |attn2 - u| {float((a2 - u[:, :, None, None]).abs().max()):.3e}")
    assert d < 1e-13 and spread < 1e-15 and float((a2 - u[:, :, None, None]).abs().max()) < 1e-13


def test_integer_cases_of_the_resid_vec_kernel_hold_their_caps():
    import gemm_exact_cases as gc

    top = 0
    for s in ac.kernel_shapes():
        c = ac.resid_vec_int_case(*s)
        top = max(top, int(c.ref.abs().max()))
        assert int((c.ref - c.ref_novec).abs().max()) > 0 and c.vec.shape == (c.M // c.tokens, c.N)
        assert c.M % 128 != 0 or c.M == 512  # a ragged last tile for every kernel, or exactly two 256-row tiles
    assert top <= gc.CAP16
    assert sorted({(t, M) for t, M, _, _ in ac.kernel_shapes()}) == [(16, 80), (64, 192), (256, 512)]


def test_derived_bounds_hold_fp32_emulations_and_reject_the_faults():
    """The per-element bounds of tests/adm_context_cases.py (derived there) against float32 emulations of the two epilogues -- torch's fp32 matmul, the
    epilogue arithmetic in fp32, one rounding to fp16 -- and against the faults: GELU for SiLU, the vec row left out, the vec row of the wrong image."""
    worst_silu = worst_vec = 0.0
    scale = float(torch.tensor(0.5).sqrt())
    for tokens, M, N, K in ac.kernel_shapes():
        c = ac.silu_case(M, N, K)
        x = c.A.float() @ c.W.float().t() + c.bias
        r = float(((torch.nn.functional.silu(x).half().double() - c.ref).abs() / c.bound).max())
        g = float(((torch.nn.functional.gelu(x, approximate="tanh").half().double() - c.ref).abs() / c.bound).max())
        twice = float(((torch.nn.functional.silu(x.half().float()).half().double() - c.ref).abs() / c.bound).max())  # SiLU of an fp16-ROUNDED pre-activation
        assert r <= 1.0 < 10 < g, (M, N, K, r, g)
        assert twice > 1.0, (M, N, K, twice)  # the bound tells one rounding from two
        worst_silu = max(worst_silu, r)
        v = ac.resid_vec_gauss_case(tokens, M, N, K, scale)
        acc = v.A.float() @ v.W.float().t()
        vr = v.vec.repeat_interleave(tokens, 0)
        ok = ((acc + (v.bias + vr)) + v.resid.float()) * scale
        r = float(((ok.half().double() - v.ref).abs() / v.bound).max())
        no_u = float(((((acc + v.bias) + v.resid.float()) * scale).half().double() - v.ref).abs().div(v.bound).max())
        m = torch.arange(M)
        wrong = float(((((acc + (v.bias + v.vec[(m % tokens) % v.vec.shape[0]])) + v.resid.float()) * scale).half().double() - v.ref).abs().div(v.bound).max())
        assert r <= 1.0 < 10 < min(no_u, wrong), (tokens, M, N, K, r, no_u, wrong)
        worst_vec = max(worst_vec, r)
    print(f"fp32 emulations, largest error / bound: silu {worst_silu:.3f}, resid_vec {worst_vec:.3f}")
