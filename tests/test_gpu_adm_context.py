"""GPU tests of ``DhariwalUNet(use_context=True)`` (``model_type == "adm_context"``): the model against the unmodified reference
(tests/golden/adm_context_tiny.pt, tools/make_adm_context_golden.py), a lone TransformerBlock against its float64 restatement (tests/adm_context_cases.py,
pinned to the reference in tests/test_adm_context_ref.py), the captured paths, the label checks, and one chip-filling shape whose linears reach the 256-row
GEMM kernels with the new epilogues."""
import os
from argparse import Namespace

import pytest
import torch

import adm_context_cases as ac

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
MODEL_BOUND = 3e-3  # rel-L2 against the reference: the bound of the DDPM++ / NCSN++ model tests for the same class of network (fp16 activations, fp32 sums)


@pytest.fixture(scope="module")
def tiny(golden_dir):
    from lfm_amd.models.EDM import DhariwalUNet

    rec = torch.load(os.path.join(golden_dir, "adm_context_tiny.pt"), map_location="cpu", weights_only=False)
    m = DhariwalUNet(**rec["cfg"])
    checksum = ac.load_seeded(m, rec["state_seed"])
    assert abs(checksum - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"], "the seeded state differs from the one the reference was run with"
    i = ac.inputs()
    assert abs(float(i.x.double().abs().sum()) - rec["x_checksum"]) <= 1e-9 * rec["x_checksum"], "the seeded inputs differ from the ones the reference was run on"
    return rec, m.to(DEV).eval(), i


def test_adm_context_tiny_matches_reference_golden(tiny):
    rec, m, i = tiny
    dev = torch.device(DEV)
    x, t0 = i.x.to(dev), torch.tensor(ac.T0D, device=dev)
    assert float(rec["v_t0d"].abs().mean()) > 1e-2
    a = m(t0, x, i.y.to(dev)).clone()
    errs = dict(t0d=ac.rel_l2(a, rec["v_t0d"]), tN=ac.rel_l2(m(i.tN[:2].to(dev), x[:2], i.y[:2].to(dev)), rec["v_tN"]),
                y2=ac.rel_l2(m(t0, x[3:], i.y2.to(dev)), rec["v_y2"]))
    for name, y in (("cfg_null", i.y_cfg_null), ("cfg_zero", i.y_cfg_zero)):
        out = m.forward_with_cfg(t0, x, y.to(dev), cfg_scale=ac.CFG_SCALE)
        assert torch.equal(out[:2], out[2:])
        errs[name] = ac.rel_l2(out[:2], rec[name])
    print("adm_context_tiny rel-L2 vs reference:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < MODEL_BOUND, errs
    assert ac.rel_l2(rec["cfg_null"], rec["cfg_zero"]) > 10 * MODEL_BOUND  # the two guided records differ: the second half's labels are read, not overwritten
    assert torch.equal(a, m(t0, x, i.y.to(dev)))  # bit-repeatable
    y_cpu_labels = m(t0, x, i.y)  # labels on the host are moved, as the time is
    assert torch.equal(a, y_cpu_labels)


def test_labels_are_checked_on_the_host_and_required(tiny):
    _, m, i = tiny
    dev = torch.device(DEV)
    x, t0 = i.x.to(dev), torch.tensor(ac.T0D, device=dev)
    rows = ac.TINY_CFG["label_dim"] + 1
    for bad in ([3, rows, 0, 7], [3, 1, -1, 7]):
        with pytest.raises(IndexError):
            m(t0, x, torch.tensor(bad, device=dev))
        with pytest.raises(IndexError):
            m.forward_with_cfg(t0, x, torch.tensor(bad, device=dev), cfg_scale=ac.CFG_SCALE)
    with pytest.raises(ValueError, match="labels"):
        m(t0, x)
    with pytest.raises(ValueError, match="labels"):
        m(t0, x, i.y[:3].to(dev))
    torch.cuda.synchronize()


def test_lone_transformer_block_vs_float64(tiny):
    """`_transformer` on the packed weights of two blocks of the tiny model -- 64 tokens x 128 channels x 2 heads, 256 tokens x 64 channels x 1 head -- against
    transformer_ref64; every seeded fault of the block lies outside the bound by more than ten times."""
    from lfm_amd import hip

    _, m, _ = tiny
    dev = torch.device(DEV)
    sd = {k: v.detach().cpu() for k, v in m.state_dict().items()}
    if m._packed is None:
        m._pack()
    for name, C, R in ((ac.BLOCK, 128, 8), ("enc.16x16_block0", 64, 16)):
        xb, yb = ac.block_input(C, R, 3)
        N, T = xb.shape[0], R * R
        ctx = sd["map_label.embedding_table.weight"][yb]
        ref = ac.transformer_ref64(sd, name + ".transformer", xb, ctx)
        tok = xb.permute(0, 2, 3, 1).reshape(N * T, C).half().to(dev)
        ctx_all = hip.gather_rows(m._packed["ctx_all"][0], yb.to(dev))
        co, cw = m._packed["ctx_all"][1][name]
        assert cw == C
        out = m._transformer(tok, m._packed[name]["tf"], ctx_all[:, co:co + cw], N, T, C // 64, C, min(32, C // 4), 1e-5)
        got = out.float().reshape(N, R, R, C).permute(0, 3, 1, 2)
        e = ac.rel_l2(got, ref)
        faults = {f: ac.rel_l2(ac.transformer_ref64(sd, name + ".transformer", xb, ctx, fault=f), ref) for f in ("no_u", "u_mod_tokens", "qkv_order", "gelu")}
        print(f"{name} ({T} tokens x {C} channels): rel-L2 vs float64 {e:.3e}; faults", {k: f"{v:.3e}" for k, v in faults.items()})
        # four fp16-rounded linears and an attention on O(1) data: the bound of the library's single-op tests (2e-3 each, tests/test_gpu_unet.py), not summed
        assert e < 2e-3
        for f, v in faults.items():
            if f == "qkv_order" and C == 64:
                assert v == 0.0  # one head: both orders are the same rows
            else:
                assert v > 10 * 2e-3, (name, f, v)


def _args(cfg_scale):
    return Namespace(method="euler", step_size=0.1, perturb=False, compute_nfe=False, cfg_scale=cfg_scale, atol=1e-5, rtol=1e-5)


def test_adm_context_tiny_euler_solves_captured_and_uncaptured(tiny):
    from lfm_amd.test_flow_latent import sample_from_model

    rec, m, i = tiny
    dev = torch.device(DEV)
    x2 = i.x[:2].to(dev)
    for name, x, kw, scale, want in (("unguided", x2, dict(y=i.y[:2].to(dev)), 1.0, rec["x_euler10"]),
                                     ("guided", torch.cat([x2, x2], 0), dict(y=i.y_cfg_null.to(dev), cfg_scale=ac.CFG_SCALE), ac.CFG_SCALE, rec["x_euler10_cfg"])):
        args = _args(scale)
        fused = sample_from_model(m, x, kw, args)[-1]
        assert m._fused_solvers and all(fg.graphs for fg in m._fused_solvers.values())  # the captured path is what ran
        e_ref = ac.rel_l2(fused[:2], want)
        args.fused = False
        e_unc = ac.rel_l2(sample_from_model(m, x, kw, args)[-1], fused)
        print(f"adm_context_tiny 10 Euler steps, {name}: captured vs reference {e_ref:.3e}, uncaptured vs captured {e_unc:.3e}")
        assert e_ref < 1e-3 and e_unc < 1e-5, name


def test_captured_forward_follows_labels_rewritten_in_place(tiny):
    """The gather kernel reads the label tensor on the device at replay time: a captured forward replayed after y.copy_(other labels) is the eager forward at
    the other labels, bit for bit (the host check cannot run during a replay; the kernel clamps instead of reading beyond the table)."""
    _, m, i = tiny
    dev = torch.device(DEV)
    x, t0 = i.x.to(dev), torch.tensor(ac.T0D, device=dev)
    y = i.y.to(dev)
    other = torch.tensor([ac.NULL_ROW, 2, 2, 9], device=dev)
    want_a, want_b = m(t0, x, y).clone(), m(t0, x, other).clone()
    assert ac.rel_l2(want_a, want_b) > 10 * MODEL_BOUND
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, capture_error_mode="thread_local"):
        out = m(t0, x, y)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_a)
    y.copy_(other)
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, want_b)


def test_chip_filling_shape_runs_the_new_epilogues_on_the_256_row_kernels():
    """Batch 64 at 32x32 with 256 / 512 channels, attention at 32 and 16: the transformers' linears have M = 65 536 (and 16 384) rows, which the chooser gives
    to the 256x256 and 256x128 kernels -- the new epilogues inside the 256-row hand-over.  One evaluation, against the same model with every GEMM forced onto
    the 128x128 kernel (selection 1: the per-(row, column) epilogue path; the halo convolutions become implicit GEMMs with it).  Both round every activation
    to fp16 once and differ in the order of the fp32 sums only: one fp16 ulp at a fraction of the elements of each of the ~25 layers, compounding through the
    network.  The bound is the one the library's whole-model comparison of two kernel selections uses, 3e-3 (tests/test_gpu_configs.py: the same images under
    the chip-filling and under the small-batch dispatch "stay within the budget of each other"); an epilogue that dropped or misplaced a term is O(0.1), and
    other labels move the output by 0.7.  The two new linears ALONE at the chip-filling shape are held to the single-kernel figure, 1e-3 (tests/test_gpu_unet.py).
    (The model comparison was first written against that single-kernel 1e-3 and measured 1.11e-3: the figure of one kernel does not bound 25 layers.)"""
    from lfm_amd import hip
    from lfm_amd.models.EDM import DhariwalUNet

    dev = torch.device(DEV)
    cfg = dict(ac.TINY_CFG, img_resolution=32, model_channels=256, attn_resolutions=[32, 16])
    m = DhariwalUNet(**cfg)
    ac.load_seeded(m)
    m = m.to(dev).eval()
    N = 64
    for M_, N_, K_ in ((N * 1024, 256, 256), (N * 1024, 1024, 256), (N * 1024, 256, 1024), (N * 256, 512, 512)):
        assert hip.gemm_plan(M_, N_, K_) in (4, 5, 6), (M_, N_, K_)  # attn1.proj, ff.layer0, ff.layer1 at 32x32; attn1.proj at 16x16
    assert hip.gemm_plan(N * 1024, 256, 256) in (5, 6) and hip.gemm_plan(N * 1024, 1024, 256) in (5, 6)  # the 256x256 kernels
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, 4, 32, 32, generator=g).to(dev)
    y = torch.randint(0, cfg["label_dim"] + 1, (N,), generator=g).to(dev)
    t = torch.rand(N, generator=g).to(dev)

    def both(fn):
        a = fn().clone()
        hip.gemm_select(1)
        try:
            b = fn().clone()
        finally:
            hip.gemm_select(0)
        return a, b

    auto, forced = both(lambda: m(t, x, y))
    torch.cuda.synchronize()
    assert bool(torch.isfinite(auto).all()) and float(auto.abs().mean()) > 1e-2
    e = ac.rel_l2(auto, forced)
    e_label = ac.rel_l2(m(t, x, torch.zeros_like(y)), auto)
    # the two new linears alone, M = 65 536 rows of 1024 tokens per image: attn1.proj (256 -> 256, residual + context row) and ff.layer0 (256 -> 1024, SiLU)
    M, T, C = N * 1024, 1024, 256
    A = (0.5 * torch.randn(M, C, generator=g)).half().to(dev)
    resid = torch.randn(M, C, generator=g).half().to(dev)
    vec = torch.randn(N, C + 64, generator=g).to(dev)[:, 64:]  # a column slice of a wider buffer, as the model passes it
    Wp, bp = (torch.randn(C, C, generator=g) / C ** 0.5).half().to(dev), (0.1 * torch.randn(C, generator=g)).to(dev)
    Wf, bf = (torch.randn(4 * C, C, generator=g) / C ** 0.5).half().to(dev), (0.1 * torch.randn(4 * C, generator=g)).to(dev)
    e_vec = ac.rel_l2(*both(lambda: hip.linear_resid_vec(A, Wp, bp, resid, vec, T)))
    e_silu = ac.rel_l2(*both(lambda: hip.linear_silu(A, Wf, bf)))
    no_vec = ac.rel_l2(hip.linear_resid_vec(A, Wp, bp, resid, None, T), hip.linear_resid_vec(A, Wp, bp, resid, vec, T))
    print(f"chip-filling adm_context (batch {N}, 256 channels, 32x32): automatic kernels vs selection 1 rel-L2 {e:.3e}; all labels 0 instead: {e_label:.3e}; "
          f"the linears alone: resid_vec {e_vec:.3e}, silu {e_silu:.3e}; without the context row {no_vec:.3e}")
    assert e < 3e-3 < 10 * 3e-3 < e_label
    assert e_vec < 1e-3 and e_silu < 1e-3 and no_vec > 0.1
