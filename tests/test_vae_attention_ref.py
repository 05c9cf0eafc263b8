"""oracle/vae_attention_ref.py without a GPU: the float64 reference against oracle.vae_ref, every input family in the regime its name promises, the
staging error small enough for the GPU bound to mean something, and the bound itself against five emulated softmax mistakes -- no faulty kernel is
built or run anywhere, the mutants are torch code in this file."""
import math

import pytest
import torch

from oracle import vae_attention_ref as ar
from oracle import vae_ref

SHAPES = [(2, 64), (3, 576), (1, 1024)]
_cases = {}


def case_of(family, n, T):
    """One case per (family, shape), with its references, shared by the tests of this module."""
    if (family, n, T) not in _cases:
        _cases[family, n, T] = ar.make_case(family, n, T)
    return _cases[family, n, T]


def test_exact_agrees_with_the_vae_oracle():
    """The same weights as a diffusers state dict, the tokens as an NCHW map: oracle.vae_ref.mid_attention (fp32) computes what `exact` computes."""
    c = ar.make_case("diffuse", 2, 64)
    pre = "decoder.mid_block.attentions.0"
    sd = {pre + ".group_norm.weight": c["gamma"], pre + ".group_norm.bias": c["beta"]}
    for ours, theirs in (("q", "to_q"), ("k", "to_k"), ("v", "to_v"), ("o", "to_out.0")):
        sd[f"{pre}.{theirs}.weight"] = c[ours + "_w"].float()
        sd[f"{pre}.{theirs}.bias"] = c[ours + "_b"]
    x = c["x"].float().transpose(1, 2).reshape(2, ar.C, 8, 8)
    ref = vae_ref.mid_attention(sd, pre, x).reshape(2, ar.C, 64).transpose(1, 2).double()
    out, branch = ar.exact(c)
    assert float((out - ref).norm() / ref.norm()) <= 1e-5
    assert torch.equal(branch, out - c["x"].double())


def test_cases_are_reproducible_and_distinct():
    a, b = ar.make_case("peaked", 2, 64), ar.make_case("peaked", 2, 64)
    assert all(torch.equal(a[k], b[k]) for k in a if torch.is_tensor(a[k]))
    assert not torch.equal(a["x"], ar.make_case("peaked", 2, 64, seed=1)["x"])
    assert not torch.equal(a["x"], ar.make_case("diffuse", 2, 64)["x"])
    s = ar.make_case("self_match", 1, 64)
    assert torch.equal(s["q_w"], s["k_w"])
    o = ar.make_case("offset_neg", 1, 64)
    assert torch.equal(o["q_b"], -o["k_b"])
    assert a["x"].dtype == a["q_w"].dtype == torch.float16 and a["gamma"].dtype == a["q_b"].dtype == torch.float32


@pytest.mark.parametrize("n,T", SHAPES)
@pytest.mark.parametrize("family", ar.FAMILIES)
def test_staging_error_is_small_and_the_family_is_in_its_regime(family, n, T):
    c = case_of(family, n, T)
    es, st = ar.e_stage(c), ar.logit_stats(c)
    print(f"{family} n={n} T={T}: e_stage {es:.2e} logits [{st['min']:.1f}, {st['max']:.1f}] sd {st['sd']:.2f} pmax_mean {st['pmax_mean']:.3f}")
    assert es <= 5e-3  # else 2 x e_stage would admit errors the image-level tests already see
    if family == "diffuse":
        assert st["pmax_mean"] < 0.2
    elif family == "peaked":
        assert st["pmax_mean"] > 0.5
    elif family == "self_match":
        assert st["max"] > 150
    elif family == "planted":
        assert st["max"] > 25
    elif family == "offset_pos":
        assert st["min"] > 120  # fp32 exp overflows at 88.7
    else:
        assert st["max"] < -120  # ... and underflows to zero


def test_staged_is_accepted_and_exact_rounded_is_accepted():
    for family in ar.FAMILIES:
        c = case_of(family, 3, 576)
        ok, ratio, _ = ar.check(ar.staged(c)[0], c)
        assert ok and ratio == pytest.approx(1.0)
        assert ar.check(ar.exact(c)[0].half(), c)[0]
        bad = ar.staged(c)[0].clone()
        bad[1, 5, 7] = float("nan")
        assert not ar.check(bad, c)[0]


# ---- the mistakes a softmax kernel makes, with the device's staging and fp32 arithmetic inside the softmax (as softmax_rows_kernel has it)
LOG2E = 1.4426950408889634


def _softmax_f32(s_scaled, max_of=lambda t: t.amax(dim=-1, keepdim=True), log2e=LOG2E):
    t = s_scaled.float() * log2e
    e = torch.exp2(t - max_of(t))
    return (e / e.sum(dim=-1, keepdim=True)).double()


def _swap_pairs(v):
    return v.reshape(v.shape[0], -1, 2, v.shape[2]).flip(2).reshape(v.shape)


MUTANTS = {
    "nomax": dict(softmax=lambda s: _softmax_f32(s, max_of=lambda t: torch.zeros_like(t[..., :1]))),
    "max_first64": dict(softmax=lambda s: _softmax_f32(s, max_of=lambda t: t[..., :64].amax(dim=-1, keepdim=True))),
    "s_fp16": dict(on_s=lambda s: s.half().double(), softmax=_softmax_f32),
    "nolog2e": dict(softmax=lambda s: _softmax_f32(s, log2e=1.0)),
    "vswap": dict(on_v=_swap_pairs, softmax=_softmax_f32),
}


@pytest.fixture(scope="module")
def verdicts():
    """{mutant: {family: (accepted, error / e_stage)}} at (3, 576), through the check the GPU test applies."""
    out = {}
    for name, hooks in MUTANTS.items():
        out[name] = {}
        for family in ar.FAMILIES:
            c = case_of(family, 3, 576)
            ok, ratio, _ = ar.check(ar.staged(c, **hooks)[0], c)
            out[name][family] = (ok, ratio)
        print(name, {f: ("ok" if ok else "REJECTED", round(r, 1) if math.isfinite(r) else r) for f, (ok, r) in out[name].items()})
    return out


def test_the_correct_softmax_in_fp32_is_accepted_everywhere():
    for family in ar.FAMILIES:
        c = case_of(family, 3, 576)
        ok, ratio, _ = ar.check(ar.staged(c, softmax=_softmax_f32)[0], c)
        assert ok and ratio < 1.5, (family, ratio)


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_every_mutant_is_rejected_by_some_family(verdicts, mutant):
    assert any(not ok for ok, _ in verdicts[mutant].values()), verdicts[mutant]


def test_diffuse_inputs_cannot_see_the_softmax_mutants(verdicts):
    """Why the families exist: on the inputs the whole-decode tests produce, these three mistakes pass the very same check."""
    for mutant in ("nomax", "max_first64", "s_fp16"):
        assert verdicts[mutant]["diffuse"][0], (mutant, verdicts[mutant]["diffuse"])
    assert not verdicts["nomax"]["offset_pos"][0] and not verdicts["nomax"]["self_match"][0]
    assert not verdicts["max_first64"]["self_match"][0]
    assert not verdicts["s_fp16"]["offset_pos"][0] and not verdicts["s_fp16"]["offset_neg"][0]
