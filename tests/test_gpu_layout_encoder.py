"""GPU tests of the layout encoder (``BERTEmbedder``, lfm_amd/models/encoder.py) against the unmodified reference (tests/golden/layout_encoder.pt,
tools/make_layout_encoder_golden.py): every fixture case within twice the error of the fp16-store emulation, the strict load of a reference-shaped state dict,
a captured forward replayed on rewritten tokens, that ``UNetModelAttn`` never reuses the cached projection of earlier tokens, and tokens -> context -> a
10-step Euler solve.  Measured device errors: profiles/layout_encoder_tests.txt."""
from argparse import Namespace
import os

import pytest
import torch

import layout_cases as lc
import layout_encoder_cases as ec

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def rec(golden_dir):
    return torch.load(os.path.join(golden_dir, "layout_encoder.pt"), map_location="cpu", weights_only=False)


@pytest.fixture(scope="module")
def embedders(rec):
    """{case name: the seeded BERTEmbedder on the GPU}, built on first use and shared."""
    from lfm_amd.models import BERTEmbedder

    built = {}

    def get(name):
        if name not in built:
            r = rec["cases"][name]
            m = BERTEmbedder(use_tokenizer=False, **r["cfg"])
            _, checksum = ec.load_seeded(m, r["state_seed"])
            assert abs(checksum - r["state_checksum"]) <= 1e-9 * r["state_checksum"], "the seeded state differs from the one the reference was run with"
            built[name] = m.to(DEV).eval()
        return built[name]

    return get


@pytest.fixture(scope="module")
def tiny_unet(golden_dir):
    from lfm_amd.models.unet import UNetModelAttn

    r = torch.load(os.path.join(golden_dir, "layout_tiny.pt"), map_location="cpu", weights_only=False)
    m = UNetModelAttn(**r["cfg"])
    lc.load_seeded(m, r["state_seed"])
    return r, m.to(DEV).eval()


@pytest.mark.parametrize("name,L", ec.case_ids())
def test_every_fixture_case_matches_the_reference(rec, embedders, name, L):
    """Bound: MARGIN (2) x the error of the fp16-store emulation against float64 on the same inputs, recomputed here, in rel-L2 and in max-abs -- against the
    reference's stored values (64 columns per row) and, on every element, against the float64 restatement that test_layout_encoder_ref.py holds to them."""
    r = rec["cases"][name]
    tok, ref, (e_l2, e_max) = ec.case_exact(name, L)
    assert torch.equal(tok, r["tokens"][L])
    m = embedders(name)
    out = m(tok.to(DEV))
    assert out.dtype == torch.float16 and tuple(out.shape) == (tok.shape[0], L, r["cfg"]["n_embed"]) and out.is_contiguous()
    got = out.cpu().double()
    assert not bool(got.isnan().any())
    d_l2, d_max = ec.rel_l2(got, ref), ec.max_abs(got, ref)
    s_l2, s_max = ec.rel_l2(ec.sampled(got), r["out_sampled"][L]), ec.max_abs(ec.sampled(got), r["out_sampled"][L])
    print(f"ENCODER {name} L={L}: device vs float64 rel-L2 {d_l2:.3e} max-abs {d_max:.3e}; vs the reference's stored values rel-L2 {s_l2:.3e} max-abs {s_max:.3e}; "
          f"fp16-store emulation rel-L2 {e_l2:.3e} max-abs {e_max:.3e}; ratios {d_l2 / e_l2:.2f} {d_max / e_max:.2f}")
    assert torch.equal(m.encode(tok.to(DEV)), out)  # encode is forward; deterministic
    assert d_l2 <= ec.MARGIN * e_l2 and d_max <= ec.MARGIN * e_max, (d_l2, e_l2, d_max, e_max)
    assert s_l2 <= ec.MARGIN * e_l2 and s_max <= ec.MARGIN * e_max, (s_l2, e_l2, s_max, e_max)


def test_strict_load_of_a_reference_shaped_state_dict(rec, embedders):
    """The reference's recorded key / shape list, to_logits included, loads with strict=True; the result does not depend on to_logits; a repack follows."""
    from lfm_amd.models import BERTEmbedder

    r = rec["cases"]["w128"]
    tok = ec.make_tokens("w128", 17).to(DEV)
    sd = ec.seeded_state(r["keys"], r["state_seed"])  # shaped as the reference's RECORDED list, not as this module
    assert "transformer.to_logits.weight" in sd and "transformer.to_logits.bias" in sd
    m = BERTEmbedder(use_tokenizer=False, **r["cfg"]).to(DEV).eval()
    before = m(tok).clone()
    gen = m._gen
    m.load_state_dict(sd, strict=True)
    assert m._gen > gen
    after = m(tok)
    assert torch.equal(after, embedders("w128")(tok)) and not torch.equal(after, before)
    sd["transformer.to_logits.weight"] = torch.zeros_like(sd["transformer.to_logits.weight"])
    m.load_state_dict(sd, strict=True)
    assert torch.equal(m(tok), after)
    with pytest.raises(RuntimeError, match="to_q"):
        m.load_state_dict({k: v for k, v in sd.items() if "layers.0.1.to_q" not in k}, strict=True)


def test_refusals_on_the_device(embedders):
    from lfm_amd import hip

    m = embedders("w128")
    tok = ec.make_tokens("w128", 17).to(DEV)
    bad = tok.clone()
    bad[1, 3] = 64
    with pytest.raises(IndexError, match=r"token 64 is outside the vocabulary \[0, 64\)"):
        m(bad)
    bad[1, 3] = -1
    with pytest.raises(IndexError, match="token -1"):
        m(bad)
    with pytest.raises(ValueError, match="max_seq_len = 92"):
        m(torch.zeros(1, 93, dtype=torch.long, device=DEV))
    try:
        with pytest.raises(hip.LfmHipError, match="inference-only"):
            m.train()(tok)
    finally:
        m.eval()


def test_fresh_result_per_call_and_one_workspace_per_shape(embedders):
    m = embedders("w128")
    a_tok, b_tok = ec.make_tokens("w128", 17).to(DEV), torch.flip(ec.make_tokens("w128", 17), [1]).contiguous().to(DEV)
    a = m(a_tok)
    ws = m._ws
    b = m(b_tok)
    assert m._ws is ws  # the workspace of (N, L) is carved once
    assert a.data_ptr() != b.data_ptr() and not torch.equal(a, b)  # ... and the result is never a view of it
    assert torch.equal(a, m(a_tok))  # a is still what it was: the second call did not write into it
    lo = min(t.data_ptr() for t in ws.values())
    hi = max(t.data_ptr() + t.numel() * 2 for t in ws.values())
    assert not (lo <= a.data_ptr() < hi) and not (lo <= b.data_ptr() < hi)
    m(a_tok[:2])
    assert m._ws is not ws  # another (N, L): another carve


def test_captured_forward_follows_rewritten_tokens(embedders):
    """A replay after ``static_tokens.copy_(other)`` is the eager forward on the other tokens, bit for bit (the ids are read on the device)."""
    m = embedders("w512")
    tok_a = ec.make_tokens("w512", 77).to(DEV)
    tok_b = torch.flip(ec.make_tokens("w512", 77), [0, 1]).contiguous().to(DEV)
    eager_a, eager_b = m(tok_a).clone(), m(tok_b).clone()  # also the eager warm-up: packs and carves the workspace
    assert not torch.equal(eager_a, eager_b)
    static_tok = tok_a.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m(static_tok)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_a)
    static_tok.copy_(tok_b)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, eager_b)
    assert torch.equal(m(tok_a), eager_a)  # eager calls after the capture are unaffected


def test_unet_does_not_reuse_the_projection_of_earlier_tokens(embedders, tiny_unet):
    """UNetModelAttn caches the K | V projection of a context on (data_ptr, _version, shape, ...), and the embedder's kernels write through raw pointers, which
    bumps no version: were the second context handed out in the first one's storage, the UNet would answer with the first tokens' projection."""
    rec_u, unet = tiny_unet
    m = embedders("w512")
    x, t = rec_u["x"].to(DEV), rec_u["tN"].to(DEV)
    tok_a = ec.make_tokens("w512", 17).to(DEV)
    tok_b = torch.flip(ec.make_tokens("w512", 17), [1]).contiguous().to(DEV)
    assert tok_a.shape == tok_b.shape
    va = unet(t, x, m(tok_a)).clone()
    vb = unet(t, x, m(tok_b)).clone()
    expect = unet(t, x, m(tok_b).clone())
    assert torch.equal(vb, expect)
    assert not torch.equal(va, vb)
    # and across many calls (freed results may come back at an old address -- but never at the address of the context the UNet still holds)
    for k in range(4):
        tok = torch.roll(tok_a, k + 1, dims=1).contiguous()
        assert torch.equal(unet(t, x, m(tok)), unet(t, x, m(tok).clone()))


def _euler_args():
    return Namespace(method="euler", step_size=0.1, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)


def test_tokens_to_context_to_euler_solve(rec, embedders, tiny_unet):
    """Tokens -> context -> ten Euler steps through the layout UNet, against the reference UNet's solve on the reference encoder's context, at the layout
    UNet's own model-level tolerance for that solve (tests/test_gpu_layout_unet.py: 1e-3 rel-L2); then the same solve, encoder included, as ONE captured graph."""
    from lfm_amd.solvers import torchdiffeq_euler_grid
    from lfm_amd.test_flow_latent import sample_from_model

    rec_u, unet = tiny_unet
    name, L = ec.SOLVE_CASE
    m = embedders(name)
    x = rec_u["x"].to(DEV)
    tok = ec.make_tokens(name, L).to(DEV)
    ctx = m(tok)
    solved = sample_from_model(unet, x, dict(context=ctx), _euler_args())[-1].clone()
    err = ec.rel_l2(solved, rec["x_euler10"])
    # captured: the encoder and the ten evaluations in one graph (the UNet projects the context inside the graph at every evaluation)
    ts, dts = torchdiffeq_euler_grid(0.1)
    ts, dts = ts.to(DEV), dts.to(DEV)
    static_tok = tok.clone()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        c = m(static_tok)
        xs = x
        for k in range(dts.numel()):
            xs = xs + dts[k] * unet(ts[k:k + 1], xs, c)
    graph.replay()
    torch.cuda.synchronize()
    err_graph, apart = ec.rel_l2(xs, rec["x_euler10"]), ec.rel_l2(xs, solved)
    print(f"ENCODER solve: tokens -> context -> 10 Euler steps vs the reference: eager {err:.3e}, captured {err_graph:.3e}; captured vs eager {apart:.3e}")
    assert err < 1e-3 and err_graph < 1e-3
    assert apart < 1e-5  # captured against eager at the project's bound for that pair (tests/test_gpu_layout_unet.py)
    other = torch.flip(tok, [1]).contiguous()
    static_tok.copy_(other)
    graph.replay()
    torch.cuda.synchronize()
    moved = ec.rel_l2(xs, solved)
    again = ec.rel_l2(xs, sample_from_model(unet, x, dict(context=m(other)), _euler_args())[-1])
    print(f"ENCODER solve: replay on rewritten tokens vs its eager solve {again:.3e}; the two token sets differ by {moved:.3e}")
    assert again < 1e-5 and moved > 1e-3
