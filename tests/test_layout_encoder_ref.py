"""CPU checks behind the layout-encoder GPU tests (``BERTEmbedder``, lfm_amd/models/encoder.py; cases and restatements: tests/layout_encoder_cases.py):
the float64 restatement is the unmodified reference (tests/golden/layout_encoder.pt) to float64 rounding; every named mistake leaves the bound the GPU test
uses while the fp16-store emulation of a correct device path stays inside it; the per-element bound of lfm_linear_gelu_f16 admits the erf form in fp32 and
refuses the tanh form; the module has the reference's keys and shapes; every refusal that needs no device.  No GPU."""
import os

import pytest
import torch

import layout_encoder_cases as ec


@pytest.fixture(scope="module")
def rec(golden_dir):
    return torch.load(os.path.join(golden_dir, "layout_encoder.pt"), map_location="cpu", weights_only=False)


def test_fixture_holds_the_cases_of_this_module_and_no_weights(rec, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "layout_encoder.pt")) < 1 << 20
    assert set(rec["cases"]) == set(ec.CASES)
    for name, (cfg, N, Ls) in ec.CASES.items():
        r = rec["cases"][name]
        assert r["cfg"] == cfg and r["batch"] == N and tuple(r["tokens"]) == Ls and r["state_seed"] == ec.STATE_SEED
        assert not any(torch.is_tensor(v) and v.is_floating_point() and v.numel() > 64 * N * max(Ls) for v in r.values())
        for L in Ls:
            assert torch.equal(r["tokens"][L], ec.make_tokens(name, L))
            t = r["tokens"][L]
            assert int(t.min()) == 0 and int(t.max()) == cfg["vocab_size"] - 1


@pytest.mark.parametrize("name,L", ec.case_ids())
def test_restatement_is_the_reference_to_float64_rounding(rec, name, L):
    r = rec["cases"][name]
    _, ref, _ = ec.case_exact(name, L)
    stored = r["out_sampled"][L]
    assert stored.dtype == torch.float64 and stored.shape == (ref.shape[0] * L, 64)
    err = ec.max_abs(ec.sampled(ref), stored)
    print(f"{name} L={L}: restatement vs the reference's stored values max-abs {err:.2e}; |out| {float(ref.norm()):.6f} vs {r['out_norm'][L]:.6f}")
    assert err < 1e-13  # outputs of order 1 after the final LayerNorm: a few hundred float64 roundings (measured 6e-15 when the fixture was written)
    assert abs(float(ref.norm()) - r["out_norm"][L]) < 1e-11 * r["out_norm"][L]  # the columns the fixture does not hold, through the norm of the whole output


@pytest.mark.parametrize("name,L", ec.case_ids())
def test_fp16_store_emulation_stays_inside_and_every_mistake_leaves_the_gpu_bound(name, L):
    """The GPU test's bound is MARGIN x the emulation's own error, in rel-L2 and in max-abs.  A correct device path that differs from the emulation only below
    its fp16 roundings stays inside; each named mistake is outside in rel-L2 (so the GPU test would fail on it), in every case where it can show at all --
    except the tanh GELU, which moves the output by less than the fp16 stores do (layout_encoder_cases.BELOW_STORE_NOISE) and is held per element instead."""
    cfg = ec.CASES[name][0]
    tok, ref, (e_l2, e_max) = ec.case_exact(name, L)
    assert 0 < e_l2 < 5e-3 and e_max < 0.05, (e_l2, e_max)  # the emulation is a small perturbation, not another function
    sd = ec.case_state(name)
    shown = {}
    for mistake in ec.MISTAKES:
        if not ec.mistake_shows(mistake, cfg, L):
            assert torch.equal(ec.encode64(sd, tok, cfg, mistake=mistake), ref)
            continue
        wrong = ec.encode64(sd, tok, cfg, fp16_stores=True, mistake=mistake)
        shown[mistake] = ec.rel_l2(wrong, ref)
        if mistake in ec.BELOW_STORE_NOISE:  # held per element by the kernel's own bound instead (test_gelu_bound_admits_the_erf_form_and_refuses_the_tanh_form)
            alone = ec.rel_l2(ec.encode64(sd, tok, cfg, mistake=mistake), ref)
            assert 0 < alone < e_l2, (mistake, alone, e_l2)  # (if this ever fails, the mistake has become visible here: move it out of BELOW_STORE_NOISE)
            continue
        assert shown[mistake] > ec.MARGIN * e_l2, (mistake, shown[mistake], e_l2)
    print(f"{name} L={L}: emulation rel-L2 {e_l2:.3e} max-abs {e_max:.3e}; mistakes rel-L2 " + ", ".join(f"{k} {v:.2e}" for k, v in shown.items()))
    assert len(shown) >= 3


def test_emulation_error_is_of_the_size_the_fp16_stores_explain():
    """Recorded when the encoder was built: rel-L2 1.0e-3 at 16 layers x 92 tokens and 6.5e-4 at 2 layers x 17 tokens under default initialisation.  The seeded
    state differs from the default initialisation, so only the order of magnitude is held: some 2^-11 per store, accumulated over the layers."""
    _, _, (deep, _) = ec.case_exact("deep16", 92)
    _, _, (shallow, _) = ec.case_exact("w512", 17)
    print(f"emulation rel-L2: 16 layers {deep:.3e}, 2 layers {shallow:.3e}")
    assert 2.0 ** -13 < shallow < 2.0 ** -9 and shallow < deep < 2.0 ** -8


def test_gelu_bound_admits_the_erf_form_and_refuses_the_tanh_form():
    """Pre-activations in about [-3, -1.5]: there the erf and the tanh GELU differ by far more than an fp16 ulp of the result."""
    g = torch.Generator().manual_seed(4)
    pre = -3 + 1.5 * torch.rand(64, 256, generator=g, dtype=torch.float64)
    pre = pre.float().double()  # as an fp32 accumulator holds it: the bound's accumulation term is then zero
    bound = ec.gelu_bound(pre, torch.zeros_like(pre), 0)
    ref = ec.gelu_erf64(pre)
    good = ((ec.gelu_emulate(pre) - ref).abs() / bound).max()
    bad = (ec.gelu_emulate(pre, "tanh_gelu") - ref).abs() / bound
    print(f"gelu bound on [-3, -1.5]: erf form error / bound {float(good):.3f}; tanh form median {float(bad.median()):.1f}, share outside {float((bad > 1).float().mean()):.3f}")
    assert float(good) <= 1.0
    assert float((bad > 1).float().mean()) > 0.5 and float(bad.max()) > 4
    # and on the Gaussian case of the GPU test, with its accumulation term: the erf form in fp32 on the exact pre-activation is inside everywhere
    c = ec.gelu_case(80, 64, 64)
    assert float(((ec.gelu_emulate(c.pre) - c.ref).abs() / c.bound).max()) <= 1.0
    assert float(c.pre.min()) < -6 and float(c.pre.max()) > 6  # both tails
    z = ec.gelu_zero_acc_case(80, 64, 64)
    assert float(z.bias.min()) >= -3 and float(z.bias.max()) <= -1.5
    assert float((torch.nn.functional.gelu(z.bias, approximate="tanh").half().double() != z.ref[0].half().double()).float().mean()) > 0.5


@pytest.mark.parametrize("name", list(ec.CASES))
def test_module_has_the_reference_keys_and_shapes(rec, name):
    from lfm_amd.models import BERTEmbedder

    cfg = ec.CASES[name][0]
    r = rec["cases"][name]
    assert r["keys"] == ec.key_shapes(**cfg)  # the list written out from the reference's source is the list the reference recorded
    m = BERTEmbedder(use_tokenizer=False, **cfg)
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == r["keys"]
    assert sum(p.numel() for p in m.parameters()) == r["params"]
    gen = m._gen
    sd, checksum = ec.load_seeded(m)  # strict, to_logits included
    assert m._gen > gen and abs(checksum - r["state_checksum"]) <= 1e-9 * r["state_checksum"]
    assert all(torch.equal(sd[k], ec.case_state(name)[k]) for k in sd)
    to_q = m.transformer.attn_layers.layers[0][1].to_q.weight
    assert to_q.shape == (512, cfg["n_embed"])  # 8 heads of 64 whatever n_embed is


def test_default_initialisation_follows_the_reference():
    from lfm_amd.models import BERTEmbedder

    torch.manual_seed(0)
    m = BERTEmbedder(512, 1, vocab_size=4096, max_seq_len=92, use_tokenizer=False)
    tr = m.transformer
    assert abs(float(tr.token_emb.weight.detach().std()) - 0.02) < 1e-3 and abs(float(tr.pos_emb.emb.weight.detach().std()) - 0.02) < 2e-3  # normal_(std=0.02), x_transformer.py:28, 580
    assert bool((tr.norm.weight == 1).all()) and not bool(tr.norm.bias.any())


def test_refusals_that_need_no_device():
    from lfm_amd import hip
    from lfm_amd.models import BERTEmbedder

    for n_embed in (96, 100, 0):
        with pytest.raises(NotImplementedError, match="n_embed % 64 == 0"):
            BERTEmbedder(n_embed, 2, vocab_size=64, max_seq_len=92, use_tokenizer=False)
    m = BERTEmbedder(64, 1, vocab_size=64, max_seq_len=20, use_tokenizer=False).eval()
    with pytest.raises(ValueError, match="max_seq_len = 20"):
        m(torch.zeros(2, 21, dtype=torch.long))
    with pytest.raises(ValueError, match="int64"):
        m(torch.zeros(2, 20, dtype=torch.int32))
    with pytest.raises(ValueError, match="int64"):
        m(torch.zeros(20, dtype=torch.long))
    with pytest.raises(hip.LfmHipError, match="no CPU fallback"):
        m(torch.zeros(2, 20, dtype=torch.long))  # tokens on the CPU
    with pytest.raises(hip.LfmHipError, match="no CPU fallback"):
        m.encode(torch.zeros(2, 20, dtype=torch.long))
