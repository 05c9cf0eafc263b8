"""Without a GPU: the yardsticks of tests/test_gpu_dit_ends.py are sound.

  * ``exact`` (float64) is the operation: it agrees with oracle/dit_ref.py in fp32 on the same gate-zeroed states to fp32 rounding -- which also shows
    that zero gates isolate the ends in the reference;
  * tier A: the emulation of correct kernels stays at least 4x inside TOL_A of ``exact`` on every case and family, every mistake that applies to a case
    lies at least 4x outside it on a family the GPU test runs, and the shifted one-pass variance lies outside on the massive0* families (at the widths
    where fp32 allows the factor: dit_ends_cases.var_shift_separable) and inside on the others;
  * tier B: the indexing mistakes lie at least 4x outside the per-forward budget;
  * the conditioning table: fp32 against float64 steps at least 8x inside TOL_COND, sin_before_cos and null_row_first at least 4x outside
    (freq_over_127 moves a row by 1e-3 at most: outside at t >= 0.999, not by 4x).
"""
import pytest
import torch

import dit_ends_cases as dc
from oracle import dit_ref

from dit_ends_cases import COND_TS, tier_b_inputs, uv_bound


# ----------------------------------------------------------------------------- exact is the operation
@pytest.mark.parametrize("shape", [dc.Shape(256, 4, 2, 4, 8), dc.Shape(384, 6, 4, 4, 16), dc.Shape(384, 6, 8, 4, 32), dc.Shape(384, 6, 2, 3, 8)],
                         ids=["p2", "p4", "p8", "k12"])
@pytest.mark.parametrize("tier", ["A", "B"])
def test_exact_agrees_with_the_fp32_oracle(shape, tier):
    cfg = dc.cfg_of(shape)
    sd = dc.make_state(shape, 3, tier)
    x = dc.make_x(shape, 4, 3)
    y = torch.tensor([2, 0, dc.NUM_CLASSES, dc.NUM_CLASSES])
    t4 = torch.tensor([0.9, 0.5, 0.02, 0.37])
    for t, labels in ((torch.tensor(0.37), None), (torch.tensor(0.37), y), (t4, None), (t4, y)):
        ref = dit_ref.dit_forward(sd, cfg, t, x, labels)
        err = dc.worst(ref, dc.exact(sd, shape, x, t, labels))
        print(f"oracle vs exact, tier {tier} {tuple(shape)} labels={labels is not None} t{tuple(t.shape)}: {err:.2e}")
        assert err < 2e-6, err
        ref = dit_ref.dit_forward_with_cfg(sd, cfg, t, x, y if labels is None else labels, dc.CFG_SCALE)
        got = dc.exact(sd, shape, x, t, y if labels is None else labels, cfg_scale=dc.CFG_SCALE)
        assert torch.equal(got[:2], got[2:])
        err = dc.worst(ref, got)
        assert err < 2e-6, err


def test_conditioning_agrees_with_the_fp32_oracle():
    shape = dc.Shape(256, 4, 2, 4, 8, 3)
    sd = dc.make_state(shape, 5, "B")
    t = torch.tensor(COND_TS)
    c = dit_ref.t_embedder(sd, t) + sd["y_embedder.embedding_table.weight"][-1]
    ref = torch.cat([torch.nn.functional.linear(torch.nn.functional.silu(c), sd[n + "weight"], sd[n + "bias"]) for n in
                     [f"blocks.{i}.adaLN_modulation.1." for i in range(3)] + ["final_layer.adaLN_modulation.1."]], 1)
    err = dc.worst(ref, dc.conditioning(sd, shape, t, None, len(COND_TS)))
    assert err < 2e-6, err


# ----------------------------------------------------------------------------- tier A
def _tier_a_errors(case, family, mistake=None):
    sd, x, ref, emb = dc.tier_a(case, family)
    got = dc.emulate(sd, case.shape, x, dc.T_SCALAR, None, dc.CFG_SCALE if case.cfg else None, mistake=mistake)
    return dc.worst(got, ref)


@pytest.mark.parametrize("case", dc.TIER_A_CASES, ids=lambda c: c.name)
def test_tier_a_tolerance_separates_correct_from_mistaken(case):
    """The fp16-by-design embedding (patch 4 / 8) is fed to the reference as staged (dit_ends_cases.tier_a), so one tolerance serves every case."""
    for family in case.families:
        err = _tier_a_errors(case, family)
        print(f"tier A correct {case.name} {family}: {err:.2e}")
        assert err * 4 <= dc.TOL_A, (family, err)
    for mistake in dc.applicable_mistakes(case):
        errs = {f: _tier_a_errors(case, f, mistake) for f in case.families}
        print(f"tier A {mistake} {case.name}: " + ", ".join(f"{f} {e:.2e}" for f, e in errs.items()))
        if mistake == "var_shift_first_element":
            for f, e in errs.items():  # what makes the massive0* families necessary
                if not f.startswith("massive0"):
                    assert e * 4 <= dc.TOL_A, (f, e)
                elif dc.var_shift_separable(case.shape, f):
                    assert dc.outside(e, dc.TOL_A), (f, e)
        else:
            assert any(dc.outside(e, dc.TOL_A) for e in errs.values()), (mistake, errs)


def test_fp16_embedding_against_exact_is_an_fp16_path():
    """Why the patch-4 / 8 cases compare from the staged embedding on: the embedding GEMM alone is ~3e-4 from float64, by design."""
    case = next(c for c in dc.TIER_A_CASES if c.name == "p4-gemm")
    sd, x, _, _ = dc.tier_a(case, "gauss")
    err = dc.worst(dc.emulate(sd, case.shape, x, dc.T_SCALAR), dc.exact(sd, case.shape, x, dc.T_SCALAR))
    print(f"fp16 embedding, end to end vs exact: {err:.2e}")
    assert dc.TOL_A < err < dc.TOL_B


# ----------------------------------------------------------------------------- tier B
@pytest.mark.parametrize("shape", dc.TIER_B_SHAPES, ids=lambda s: f"D{s.hidden}p{s.patch}c{s.in_ch}")
@pytest.mark.parametrize("cfg", [False, True], ids=["plain", "cfg"])
def test_tier_b_indexing_mistakes_are_far_outside(shape, cfg):
    batch = 6 if cfg else 5
    sd, x, y, t = tier_b_inputs(shape, batch)
    case = dc.Case("b", shape, batch, cfg, ("gauss",))
    emb = dc.staged_embedding(sd, shape, x, cfg) if dc.embed_kind(shape) == "f16" else None  # the fp16-by-design embedding, as in tier A
    scale = dc.CFG_SCALE if cfg else None
    for tt, yy, what in ((torch.tensor(0.37), y, "labels"), (t, None, "t"), (t, y, "both")):
        ref = dc.exact(sd, shape, x, tt, yy, scale, embedding=emb)
        err = dc.worst(dc.emulate(sd, shape, x, tt, yy, scale), ref)
        print(f"tier B correct D={shape.hidden} cfg={cfg} {what}: {err:.2e}")
        assert err * 4 <= dc.TOL_B, err
        ms = [m for m in dc.applicable_mistakes(case, "B") if m in ("twin_rows_swapped", "cfg_second_half_read", "unpatchify_pq_swapped",
                                                                    "unpatchify_c_major", "mod_row_of_image_0")]
        if yy is None:
            ms.append("null_row_first")
        for mistake in ms:
            e = dc.worst(dc.emulate(sd, shape, x, tt, yy, scale, mistake=mistake), ref)
            print(f"tier B {mistake} D={shape.hidden} cfg={cfg} {what}: {e:.2e}")
            assert dc.outside(e, dc.TOL_B), (mistake, e)


# ----------------------------------------------------------------------------- conditioning table
@pytest.mark.parametrize("shape", [dc.Shape(64, 1, 2, 4, 8), dc.Shape(384, 6, 2, 4, 8), dc.Shape(1024, 16, 2, 4, 8), dc.Shape(1280, 20, 2, 4, 8),
                                   dc.Shape(256, 4, 2, 4, 8, 3)], ids=lambda s: f"D{s.hidden}x{s.depth}")
def test_conditioning_tolerance(shape):
    sd = dc.make_state(shape, 31, "B")
    n = len(COND_TS)
    ref = dc.conditioning(sd, shape, COND_TS, None, n, staged=True)
    e64 = dc.worst(dc.conditioning(sd, shape, COND_TS, None, n, staged=True, fp32_steps=False), ref)
    print(f"conditioning D={shape.hidden} depth={shape.depth}: fp32 steps vs float64 steps {e64:.2e}")
    assert e64 * 8 <= dc.TOL_COND, e64
    for mistake in dc.COND_MISTAKES:
        errs = dc.image_errors(dc.conditioning(sd, shape, COND_TS, None, n, staged=True, mistake=mistake), ref)
        print(f"conditioning {mistake} D={shape.hidden}: " + ", ".join(f"t={t:g} {float(e):.2e}" for t, e in zip(COND_TS, errs)))
        if mistake == "freq_over_127":  # not separable by 4x at any shape (dit_ends_cases.TOL_COND): shown to be outside where t is large
            assert all(float(e) > dc.TOL_COND for t, e in zip(COND_TS, errs) if t >= 0.999), errs
        else:
            assert all(dc.outside(float(e), dc.TOL_COND) for e in errs), (mistake, errs)


def test_uv_bound_holds_for_an_fp32_summation():
    """The bound tests/test_gpu_dit_ends.py gives uv_gemv_kernel, against an fp32 emulation: products and sums in fp32 (per-lane chains, then a tree)."""
    D, N = 1024, 512
    g = torch.Generator().manual_seed(4)
    W = (torch.randn(N, D, generator=g) * 0.03).half().float()
    a = 1.0 + torch.randn(D, generator=g) * 0.3
    prod = (W * a).reshape(N, D // 512, 64, 8)  # lane l holds the chunks l, l + 64, ..: eight products each
    lane = torch.zeros(N, 64)
    for j in range(prod.shape[1]):
        for e in range(8):
            lane = lane + prod[:, j, :, e]
    while lane.shape[1] > 1:
        lane = lane[:, ::2] + lane[:, 1::2]
    exact = W.double() @ a.double()
    ratio = float(((lane[:, 0].double() - exact).abs() / (uv_bound(D) * (W.double().abs() @ a.double().abs()))).max())
    print(f"fp32 GEMV emulation: |error| / bound {ratio:.2f}")
    assert ratio <= 0.5
