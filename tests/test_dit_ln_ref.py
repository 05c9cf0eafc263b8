"""Without a GPU: the yardsticks of tests/test_gpu_dit_ln.py are sound (tests/dit_ln_cases.py).

  * the float64 references are the operation: torch.nn.functional.layer_norm in float64 and oracle/dit_ref.py's block agree with them;
  * over every case and family the emulation of a CORRECT kernel uses at most HALF of the derived fp32 allowance (the factor 2 covers summation orders the
    emulation does not reproduce; the one fp16 rounding of an fp16 quantity is granted whole, since a correctly rounded value reaches its half ulp): its
    error over the bound with the fp32 terms halved is printed and at most 1, for fp32 quantities error over bound at most 0.5; constant rows give
    fp16(shift) bit for bit;
  * every named mistake exceeds the bound 4x or more on a named case; where a mistake cannot be told from rounding at some case it is left out of the
    separation BY NAME with the reason (NOT_SEPARABLE) and shown to be inside there -- the bound is not widened.
"""
import functools
import math

import pytest
import torch

import dit_ends_cases as dc
import dit_ln_cases as lc
from oracle import dit_ref


# ----------------------------------------------------------------------------- the references are the operation
def test_ln_ref_is_layer_norm_modulate_in_float64():
    for name, fam in (("D520-M37", "gauss"), ("D1280-M33", "massive"), ("D12-M5", "offset"), ("wide-stride", "tiny")):
        case = _case(name)
        X, _, shift, scale, ref, _ = lc.ln_case(case, fam)
        idx = lc.image_of_row(case.M, shift.shape[0], case.tokens)
        want = torch.nn.functional.layer_norm(X.double(), (case.D,), eps=1e-6) * (1 + scale.double()[idx]) + shift.double()[idx]
        assert torch.allclose(ref, want, rtol=1e-11, atol=1e-11), (name, fam)


def test_fold_ref_is_the_oracles_block():
    """oracle/dit_ref.dit_block in float64 = X1 + gate_mlp (fold_ref.act fc2^T + b) with X1 the oracle's own first half of the block."""
    shape = dc.Shape(256, 4, 2, 4, 8)
    cfg = dc.cfg_of(shape)
    sd = {k: v.double() for k, v in dit_ref.make_dit_state(cfg, seed=4).items()}
    sd["blocks.0.adaLN_modulation.1.bias"] = torch.randn(6 * 256, generator=torch.Generator().manual_seed(1), dtype=torch.float64) * 0.3
    g = torch.Generator().manual_seed(2)
    x = torch.randn(3, 16, 256, generator=g, dtype=torch.float64)
    c = torch.randn(3, 256, generator=g, dtype=torch.float64)
    out = dit_ref.dit_block(sd, 0, x, c, 4)
    mod = torch.nn.functional.linear(torch.nn.functional.silu(c), sd["blocks.0.adaLN_modulation.1.weight"], sd["blocks.0.adaLN_modulation.1.bias"])
    s_msa, sc_msa, g_msa, s_mlp, sc_mlp, g_mlp = mod.chunk(6, dim=1)
    x1 = x + g_msa[:, None] * dit_ref.attention(sd, "blocks.0.attn.", dit_ref.modulate(torch.nn.functional.layer_norm(x, (256,), eps=1e-6), s_msa, sc_msa), 4)
    X1 = x1.reshape(48, 256)
    f = lc.fold_ref(X1, X1.mean(1), s_mlp, sc_mlp, sd["blocks.0.mlp.fc1.weight"], sd["blocks.0.mlp.fc1.bias"], 16)
    want = x1 + g_mlp[:, None] * (f.act @ sd["blocks.0.mlp.fc2.weight"].T + sd["blocks.0.mlp.fc2.bias"]).reshape(3, 16, 256)
    assert torch.allclose(out, want, rtol=1e-10, atol=1e-10)
    assert torch.allclose(lc.ln_ref(X1, s_mlp, sc_mlp, 16),
                          dit_ref.modulate(torch.nn.functional.layer_norm(x1, (256,), eps=1e-6), s_mlp, sc_mlp).reshape(48, 256), rtol=1e-11, atol=1e-11)


# ----------------------------------------------------------------------------- DIRECT
def _case(prefix):
    hits = [c for c in lc.LN_CASES if c.name == prefix] or [c for c in lc.LN_CASES if c.name.startswith(prefix + "-")]
    assert len(hits) == 1, (prefix, hits)
    return hits[0]


def test_direct_correct_emulation_is_within_half_the_bound():
    worst, worst32 = {}, {}
    for case in lc.LN_CASES:
        for fam in lc.FAMILIES:
            X, _, shift, scale, ref, _ = lc.ln_case(case, fam)
            got = lc.ln_emulate(X, shift, scale, case.tokens)
            r = lc.ratio(got, ref, lc.ln_bound(X, shift, scale, case.tokens, room=0.5))
            worst[fam] = max(worst.get(fam, 0.0), r)
            assert r <= 1.0, (case.name, fam, r)
            r32 = lc.ratio(lc.ln_emulate(X, shift, scale, case.tokens, round16=False), ref, lc.ln_bound(X, shift, scale, case.tokens, round16=False))
            worst32[fam] = max(worst32.get(fam, 0.0), r32)
            assert r32 <= 0.5, (case.name, fam, r32)  # in front of the fp16 rounding: the fp32 allowance alone
            if fam == "constant":  # d = 0 exactly: the output is the shift row, whatever rstd is
                idx = lc.image_of_row(case.M, shift.shape[0], case.tokens)
                assert torch.equal(got, shift[idx].half().double()), case.name
    print("DIRECT correct emulation, largest error / (fp16 rounding + HALF the fp32 allowance) per family: " + ", ".join(f"{f} {v:.3f}" for f, v in worst.items()))
    print("DIRECT correct emulation in front of the fp16 rounding, largest error / fp32 allowance per family: " + ", ".join(f"{f} {v:.3f}" for f, v in worst32.items()))


# mistake -> (case, family) on which it lies 4x or more outside the bound
DIRECT_SEPARATION = {
    "var_over_d_minus_1": ("D8-M37", "gauss"),
    "eps_1e-5": ("D1280-M5", "tiny"),
    "eps_missing": ("D520-M33", "tiny"),
    "uncentred_variance": ("D1024-M33", "offset"),
    "scale_msa_for_scale_mlp": ("D1152-M5", "gauss"),
    "one_plus_missing": ("D64-M33", "gauss"),
    "shift_scale_swapped": ("D1276-M37", "massive"),
    "mod_row_of_image_0": ("D256-M37", "gauss"),
    "mod_row_of_wave_first_row": ("D512-M37", "onehot"),
}
# (mistake, case, family) left out of the separation, with the reason; each is shown to be INSIDE 4x the bound below
DIRECT_NOT_SEPARABLE = {
    ("eps_1e-5", "D256-M33", "gauss"): "var = 4: rstd moves by 4.5e-6 / (2 var) = 1e-6 relative, far inside one fp16 rounding; eps decides on the tiny family only",
    ("eps_missing", "D256-M33", "gauss"): "as eps_1e-5",
    ("uncentred_variance", "D256-M33", "gauss"): "mean 0.3, sigma 2: E[x^2] - mu^2 loses no digits here; the offset family shows it",
    ("mod_row_of_image_0", "shared-row", "gauss"): "one shared modulation row: every row's image row IS row 0",
}


def _direct_mistake_ratio(mistake, name, fam):
    case = _case(name)
    X, _, shift, scale, ref, bound = lc.ln_case(case, fam)
    other = lc.make_mod(shift.shape[0], case.D, 977)[2]
    return lc.ratio(lc.ln_emulate(X, shift, scale, case.tokens, mistake=mistake, other_scale=other), ref, bound)


def test_direct_mistakes_are_outside_the_bound():
    assert set(DIRECT_SEPARATION) == set(lc.DIRECT_MISTAKES)
    for mistake, (name, fam) in DIRECT_SEPARATION.items():
        r = _direct_mistake_ratio(mistake, name, fam)
        print(f"DIRECT {mistake} on {name} {fam}: error/bound {r:.3g}")
        assert r >= 4.0, (mistake, r)
    for (mistake, name, fam), why in DIRECT_NOT_SEPARABLE.items():
        r = _direct_mistake_ratio(mistake, name, fam)
        print(f"DIRECT {mistake} on {name} {fam}: error/bound {r:.3g} (not separable: {why})")
        assert r < 4.0, (mistake, name, fam, r)


# ----------------------------------------------------------------------------- FOLDED
H_CPU = 192  # fc1 columns of the CPU cases (the bound is per column; the width of the MLP does not enter it)
FOLD_CPU = {  # name -> (D, rows M, tokens, modulation rows, family, target r)
    "gauss-256": (256, 40, 8, 1, "gauss", None), "gauss-512-rows": (512, 40, 8, 5, "gauss", None), "gauss-1280": (1280, 24, 8, 1, "gauss", None),
    "massive-512": (512, 40, 8, 1, "massive", None),
    "r0-512": (512, 40, 8, 1, "shift", 0.0), "r1-512": (512, 40, 8, 5, "shift", 1.0), "r8-512": (512, 40, 8, 1, "shift", 8.0), "r64-512": (512, 40, 8, 1, "shift", 64.0),
    "r1-1280": (1280, 24, 8, 1, "shift", 1.0),
}


@functools.lru_cache(maxsize=None)
def fold_case(name):
    D, M, tokens, rows, fam, r = FOLD_CPU[name]
    seed = 11 + sorted(FOLD_CPU).index(name)
    g = torch.Generator().manual_seed(seed)
    x0 = lc.make_rows("massive" if fam == "massive" else "gauss", M, D, seed)
    if fam == "shift":
        x0 = (x0 - 0.3) / 2.0 + 0.3  # sigma 1
    X1 = x0 + 0.05 * torch.randn(M, D, generator=g) + (0.0 if r is None else r * float(x0.std()))
    c = x0.sum(1) / D  # fp32: what the previous consumer published
    _, shift, scale = lc.make_mod(rows, D, seed)
    W1 = (torch.randn(H_CPU, D, generator=g) / math.sqrt(D)).half()
    b1 = torch.randn(H_CPU, generator=g) * 0.1
    return X1, c, shift, scale, W1, b1, tokens, lc.fold_ref(X1, c, shift, scale, W1, b1, tokens)


def test_fold_correct_emulation_is_within_half_the_bound():
    for name in FOLD_CPU:
        X1, c, shift, scale, W1, b1, tokens, f = fold_case(name)
        M, D = X1.shape
        h = lc.fold_ref(X1, c, shift, scale, W1, b1, tokens, room=0.5)  # the fp16 quantities: rounding + half the fp32 allowance
        act = lc.ratio(lc.fold_emulate(X1, c, shift, scale, W1, b1, tokens), f.act, h.e_act)
        ap = lc.ratio(lc.aprime_emulate(X1, c, scale, tokens), f.aprime, h.e_aprime)
        d = X1 - c[:, None]
        slots = torch.stack([X1.reshape(M, -1, 256).sum(2), (d * d).reshape(M, -1, 256).sum(2)], 2)
        # an all-zero slot bound means an all-zero slot: equality
        pr = float(((slots.double() - f.part).abs() / torch.clamp(f.e_part, min=1e-300)).max())
        cen = lc.ratio(slots[:, :, 0].sum(1) * torch.tensor(1.0 / D), f.mean, f.e_cen)
        print(f"FOLDED correct emulation {name}: r {float(f.r.min()):.2f} .. {float(f.r.max()):.2f}, error / (fp16 rounding + half the allowance): activation "
              f"{act:.3f}, A' {ap:.3f}; error/bound: slots {pr:.3f}, mean {cen:.3f}")
        assert max(act, ap) <= 1.0 and max(pr, cen) <= 0.5, (name, act, ap, pr, cen)


FOLD_SEPARATION = {
    "var_over_d_minus_1": None, "eps_1e-5": None, "eps_missing": None, "dl_sq_not_subtracted": "r1-512", "b_sign_flipped": "r1-512",
    "inv_n_1_over_256": "gauss-512-rows", "slot_0_only": "gauss-1280", "c_from_other_cen": "r8-512", "scale_msa_for_scale_mlp": "gauss-256",
    "one_plus_missing": "gauss-1280", "shift_scale_swapped": "massive-512", "mod_row_of_image_0": "gauss-512-rows",
}
FOLD_NOT_SEPARABLE = {
    ("eps_1e-5", "gauss-256"): "the residual stream of a forward has var >= 0.1: 1e-5 against 1e-6 moves rstd by < 5e-5; held on the DIRECT kernels' tiny family",
    ("eps_missing", "gauss-256"): "as eps_1e-5",
    ("dl_sq_not_subtracted", "gauss-256"): "r <= 0.05 here: dl^2 is 2e-3 of the variance, rstd moves by 1e-3 -- the worst-case A' term alone allows more; shown at r = 1",
    ("b_sign_flipped", "r0-512"): "r ~ 0: b u is rounding-sized; shown at r = 1",
    ("inv_n_1_over_256", "gauss-256"): "D = 256: 1 / 256 IS 1 / D",
    ("slot_0_only", "gauss-256"): "D = 256 has one slot",
    ("var_over_d_minus_1", "gauss-256"): "the fold needs D % 256 == 0: rstd moves by 1 / (2 D) <= 2e-3, inside the worst-case A' term; held on the DIRECT kernels",
}


def _fold_mistake_ratio(mistake, name, c_other=None):
    X1, c, shift, scale, W1, b1, tokens, f = fold_case(name)
    other = lc.make_mod(shift.shape[0], X1.shape[1], 977)[2]
    got = lc.fold_emulate(X1, c, shift, scale, W1, b1, tokens, mistake=mistake, c_other=c if c_other is None else c_other, other_scale=other)
    return lc.ratio(got, f.act, f.e_act)


def test_fold_mistakes_are_outside_the_bound():
    assert set(FOLD_SEPARATION) == set(lc.FOLD_MISTAKES)
    for mistake, name in FOLD_SEPARATION.items():
        if name is None:
            continue
        # c_from_other_cen: the other array holding the row means of X1 (what it holds once fc1 has published them)
        other = fold_case(name)[0].sum(1) / fold_case(name)[0].shape[1] if mistake == "c_from_other_cen" else None
        r = _fold_mistake_ratio(mistake, name, other)
        print(f"FOLDED {mistake} on {name}: error/bound {r:.3g}")
        assert r >= 4.0, (mistake, r)
    for (mistake, name), why in FOLD_NOT_SEPARABLE.items():
        r = _fold_mistake_ratio(mistake, name)
        print(f"FOLDED {mistake} on {name}: error/bound {r:.3g} (not separable: {why})")
        assert r < 4.0, (mistake, name, r)


def test_fold_c_from_other_cen_cannot_show_in_a_depth_1_forward():
    """When fc1 runs in a depth-1 forward, BOTH cen arrays hold the row means of x0: cen[0] from the embedding (two-pass), cen[1] from the qkv consumer
    (slot sums).  They differ by fp32 rounding, so reading the wrong one is not separable there -- by name, with this reason; the mistake is separated above
    with the other array holding different means."""
    X1, c, shift, scale, W1, b1, tokens, f = fold_case("r8-512")
    r = _fold_mistake_ratio("c_from_other_cen", "r8-512", torch.nextafter(c, c + 1.0))
    print(f"FOLDED c_from_other_cen with both arrays one ulp apart: error/bound {r:.3g}")
    assert r < 4.0


def test_fold_bound_against_the_per_forward_budget():
    """The envelope the design note asserts in words: per-row rel-L2 of the derived bound of the fc1 pre-activation... taken on the activation, as r grows."""
    rs, rel, rms = [], [], []
    D, M = 512, 16
    for r in (0.25, 0.5, 1.0, 2.0, 4.0, 8.0, 16.0, 32.0, 64.0, 128.0):
        g = torch.Generator().manual_seed(5)
        x0 = torch.randn(M, D, generator=g) + 0.3
        X1 = x0 + 0.05 * torch.randn(M, D, generator=g) + r * float(x0.std())
        _, shift, scale = lc.make_mod(1, D, 5)
        W1 = (torch.randn(H_CPU, D, generator=g) / math.sqrt(D)).half()
        f = lc.fold_ref(X1, x0.sum(1) / D, shift, scale, W1, torch.zeros(H_CPU), 8)
        rs.append(float(f.r.mean()))
        rel.append(float((f.e_act.norm(dim=1) / f.act.norm(dim=1)).max()))
        # the same operand term with INDEPENDENT roundings (each A'_k off by a uniform +-2^-11 |A'_k|: rms 2^-11 / sqrt 3), an estimate and not a bound
        rho = 1.0 / torch.sqrt(X1.double().var(1, unbiased=False, keepdim=True) + lc.EPS)
        e = 1.13 * rho * lc.U16 / math.sqrt(3.0) * torch.sqrt(f.aprime ** 2 @ (W1.double() ** 2).T)
        rms.append(float((e.norm(dim=1) / f.act.norm(dim=1)).max()))
    print("FOLDED worst-case bound, per-row rel-L2 against r: " + ", ".join(f"r={a:.2f} {b:.2e}" for a, b in zip(rs, rel))
          + f"; crosses 2e-3 at r = {lc.budget_crossing(rs, rel)}")
    print("FOLDED operand term with independent roundings (estimate): " + ", ".join(f"r={a:.2f} {b:.2e}" for a, b in zip(rs, rms))
          + f"; crosses 2e-3 at r = {lc.budget_crossing(rs, rms)}")
    assert all(b > a for a, b in zip(rel, rel[1:]))  # the bound grows with r
