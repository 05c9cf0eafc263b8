"""Without a GPU: the yardsticks of tests/test_gpu_layout_kernels.py are sound (as tests/test_unet_attention_ref.py shows for the streamed self-attention).

  * the fp32-staged emulation of a CORRECT cross-attention kernel stays within the GPU test's per-item bound on every case, and each mistake such a kernel can
    make -- a key dropped, padding not masked, the key loop bounded by the query count, the context of another image read, O or the sum not rescaled --
    exceeds it on at least one case: the cases can see it;
  * LayerNorm: the two-pass fp32 emulation is inside the derived per-element bound on every family and width, E[x^2] - E[x]^2 is outside it on the
    offset family at every width;
  * GEGLU: the fp32 erf-form emulation is inside the bound, the tanh approximation is outside it."""
import math

import pytest
import torch

import layout_cases as lc


def test_emulated_correct_cross_attention_is_inside_the_bound():
    for Tq, Tk, ch in lc.CROSS_SHAPES:
        for family in lc.CROSS_FAMILIES:
            qkv, ref = lc.cross_case(family, Tq, Tk, ch)
            err = lc.worst(lc.cross_emulate(*qkv), ref)
            print(f"emulation {family} Tq={Tq} Tk={Tk} ch={ch}: {err:.3e}")
            assert err <= lc.TOL, (family, Tq, Tk, ch, err)


@pytest.mark.parametrize("mistake", lc.CROSS_MISTAKES)
def test_every_emulated_cross_attention_mistake_is_visible_on_some_case(mistake):
    errs = {}
    for Tq, Tk, ch in lc.CROSS_SHAPES:
        for family in lc.CROSS_FAMILIES:
            qkv, ref = lc.cross_case(family, Tq, Tk, ch)
            errs[(family, Tq, Tk, ch)] = lc.worst(lc.cross_emulate(*qkv, mistake=mistake), ref)
    seen = [c for c, e in errs.items() if math.isnan(e) or e > lc.TOL]
    print(f"{mistake}: visible on {len(seen)} of {len(errs)} cases; worst {max((e for e in errs.values() if not math.isnan(e)), default=float('nan')):.2e}")
    assert seen, (mistake, errs)


def _over(got, ref, bound):
    """The worst error / bound over the elements; inf where the result is not finite."""
    r = (got - ref).abs() / bound
    return float("inf") if not bool(torch.isfinite(got).all()) else float(r.max())


@pytest.mark.parametrize("C", lc.LN_WIDTHS)
def test_layernorm_bound_admits_two_passes_and_refuses_one(C):
    for family in lc.LN_FAMILIES:
        x, gamma, beta, ref = lc.ln_case(family, C)
        bound = lc.ln_bound(x, gamma, beta)
        two, one = _over(lc.ln_emulate(x, gamma, beta), ref, bound), _over(lc.ln_emulate(x, gamma, beta, mistake="one_pass_variance"), ref, bound)
        print(f"LayerNorm {family} C={C}: two-pass {two:.3f} of the bound, one-pass {one:.3g}; bound at most {float(bound.max()):.3e}")
        assert two <= 1.0, (family, C, two)
        if family == "offset200":
            assert one > 1.0, (C, one)


@pytest.mark.parametrize("I", lc.GEGLU_WIDTHS)
def test_geglu_bound_admits_erf_and_refuses_tanh(I):
    h, ref = lc.geglu_case(I)
    bound = lc.geglu_bound(h)
    erf, tanh = _over(lc.geglu_emulate(h), ref, bound), _over(lc.geglu_emulate(h, mistake="tanh_gelu"), ref, bound)
    print(f"GEGLU I={I}: erf form {erf:.3f} of the bound, tanh form {tanh:.3g}")
    assert erf <= 1.0 and tanh > 1.0, (I, erf, tanh)
    gate = h.double()[:, I:]
    assert float(gate.min()) == -12 and float(gate.max()) == 12 and bool((ref[gate < -11].abs() < 2.0 ** -25).all())  # gates the erf form sends to +-0
