"""GPU parity of the origin-ADM UNet (HIP path through the C ABI) against golden vectors produced by the unmodified reference
``models/guided_diffusion/unet.py`` (tests/golden/unet_tiny.pt, oracle/make_golden.py).  Tolerance: rel-L2 <= 3e-3."""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


@pytest.mark.parametrize("which", ["ssn", "cls"])
def test_unet_matches_reference_golden(golden_dir, which):
    from lfm_amd.models.unet import UNetModel

    rec = torch.load(os.path.join(golden_dir, "unet_tiny.pt"), map_location="cpu", weights_only=False)[which]
    dev = torch.device("cuda:0")
    m = UNetModel(**rec["cfg"])
    m.load_state_dict({k: v.float() for k, v in rec["state_dict"].items()}, strict=True)
    m = m.to(dev).eval()
    y = rec["y"].to(dev) if "y" in rec else None
    got = m(rec["t"].to(dev), rec["x"].to(dev), y)
    assert float(rec["v"].abs().mean()) > 1e-2
    assert rel_l2(got, rec["v"]) < 3e-3
    # scalar time is broadcast (the reference needs device="cuda" for this, unet.py:629-630)
    got1 = m(torch.tensor(float(rec["t"][0]), device=dev), rec["x"][:1].to(dev), y[:1] if y is not None else None)
    assert rel_l2(got1, rec["v"][:1]) < 3e-3


def test_building_blocks_against_torch():
    """conv3x3 in its three modes, GroupNorm+FiLM+SiLU, legacy attention -- each against the fp32 torch op on identical data."""
    import torch.nn.functional as F

    from lfm_amd import hip

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    L = hip.lib()
    N, H, W, Cin, Cout = 2, 12, 12, 128, 192
    x = torch.randn(N, Cin, H, W, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    wp = w.permute(0, 2, 3, 1).reshape(Cout, -1).half().to(dev)
    xh = x.half()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    for mode, (ref, Ho) in {0: (F.conv2d(xh.float(), w.half().float(), b, padding=1), H),
                            1: (F.conv2d(F.interpolate(xh.float(), scale_factor=2, mode="nearest"), w.half().float(), b, padding=1), 2 * H),
                            2: (F.conv2d(xh.float(), w.half().float(), b, stride=2, padding=1), H // 2)}.items():
        out = torch.empty(N * Ho * Ho, Cout, dtype=torch.float16, device=dev)
        xin = nhwc(xh).to(dev)
        bd = b.to(dev)  # keep device tensors alive across the call (a temporary's block would be recycled)
        hip.check(L.lfm_conv3x3_f16(hip.ptr(xin), hip.ptr(wp), hip.ptr(bd), None, hip.ptr(out), N, Ho, Ho, Cin, Cout, mode,
                                    hip.stream_ptr()), "conv")
        assert rel_l2(out.reshape(N, Ho, Ho, Cout).permute(0, 3, 1, 2), ref) < 2e-3, mode
    # GroupNorm32 + FiLM + SiLU on a channel count whose groups are 6 wide (192 / 32)
    C = 192
    xg = (torch.randn(N, C, H, W, generator=g) * 2 + 0.5).half()
    gamma, beta = torch.randn(C, generator=g), torch.randn(C, generator=g)
    film = torch.randn(N, 2 * C, generator=g) * 0.3
    ref = F.group_norm(xg.float(), 32, gamma, beta, eps=1e-5) * (1 + film[:, :C, None, None]) + film[:, C:, None, None]
    ref = F.silu(ref)
    xin = nhwc(xg).to(dev)
    y = torch.empty_like(xin)
    scr = torch.empty(L.lfm_groupnorm_scratch_bytes(N, C), dtype=torch.uint8, device=dev)
    gd, bd, fd = gamma.to(dev), beta.to(dev), film.to(dev)
    hip.check(L.lfm_groupnorm_f16(hip.ptr(xin), hip.ptr(y), hip.ptr(gd), hip.ptr(bd), hip.ptr(fd), 2 * C,
                                  hip.ptr(scr), N, H * W, C, 32, 1e-5, 1, hip.stream_ptr()), "gn")
    assert rel_l2(y.permute(0, 3, 1, 2), ref) < 2e-3
    # legacy attention: [N, heads*3*ch, T] with per-head [q|k|v]
    heads, ch, T = 4, 128, 64
    qkv = torch.randn(N, heads * 3 * ch, T, generator=g).half()
    q, k, v = qkv.float().reshape(N * heads, 3 * ch, T).split(ch, dim=1)
    wgt = torch.softmax(torch.einsum("bct,bcs->bts", q * ch ** -0.25, k * ch ** -0.25), -1)
    ref = torch.einsum("bts,bcs->bct", wgt, v).reshape(N, heads * ch, T)
    tok = qkv.permute(0, 2, 1).reshape(N * T, heads * 3 * ch).contiguous().to(dev)
    out = torch.empty(N * T, heads * ch, dtype=torch.float16, device=dev)
    hip.check(L.lfm_attention_small_f16(hip.ptr(tok), hip.ptr(out), N, T, heads, ch, hip.stream_ptr()), "attn")
    assert rel_l2(out.reshape(N, T, heads * ch).permute(0, 2, 1), ref) < 2e-3


@pytest.mark.parametrize("N,HW,C,groups,film_on", [(3, 64, 256, 32, True), (2, 256, 768, 32, True), (32, 16, 1024, 32, False), (2, 4096, 512, 32, True),
                                                   (2, 64, 64, 16, True)])
def test_groupnorm_fused_small_path_vs_torch_and_three_kernel_path(N, HW, C, groups, film_on):
    """cpg % 8 == 0 and HW <= 4096: one fused launch (block per image x group chunk).  Against torch's group_norm and against the
    three-kernel path (flag UNET_GN_ROWS) on the same data; both deterministic."""
    import torch.nn.functional as F

    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(N + HW + C)
    x = (torch.randn(N, HW, C, generator=g) * 1.5 + 0.3).half()
    gamma, beta = 1 + 0.2 * torch.randn(C, generator=g), 0.2 * torch.randn(C, generator=g)
    film = torch.randn(N, 2 * C, generator=g) * 0.3 if film_on else None
    ref = F.group_norm(x.float().permute(0, 2, 1), groups, gamma, beta, eps=1e-5)
    if film_on:
        ref = ref * (1 + film[:, :C, None]) + film[:, C:, None]
    ref = F.silu(ref).permute(0, 2, 1)
    xin, gd, bd = x.reshape(N * HW, C).to(dev), gamma.to(dev), beta.to(dev)
    fd = film.to(dev) if film_on else None
    scr = torch.empty(L.lfm_groupnorm_scratch_bytes(N, C), dtype=torch.uint8, device=dev)

    def run():
        y = torch.empty_like(xin)
        hip.check(L.lfm_groupnorm_f16(hip.ptr(xin), hip.ptr(y), hip.ptr(gd), hip.ptr(bd), hip.ptr(fd), 2 * C if film_on else 0, hip.ptr(scr), N, HW, C,
                                      groups, 1e-5, 1, hip.stream_ptr()), "gn")
        torch.cuda.synchronize()
        return y

    fused = run()
    assert torch.equal(fused, run())
    hip.gemm_select(hip.DBG_UNET_GN_ROWS << 4)
    try:
        three = run()
    finally:
        hip.gemm_select(0)
    assert rel_l2(fused.reshape(N, HW, C), ref) < 2e-3
    assert rel_l2(three.reshape(N, HW, C), ref) < 2e-3
    assert rel_l2(fused, three) < 1e-3


@pytest.mark.parametrize("N,H,Cin,Cout,mode", [(32, 4, 1024, 1024, 0), (8, 8, 512, 512, 0), (2, 4, 2048, 1024, 0), (4, 8, 512, 512, 2), (4, 8, 512, 256, 1)])
def test_conv3x3_split_k_small_maps(N, H, Cin, Cout, mode):
    """Low-resolution UNet levels: small M, K = 9*Cin up to 18432.  With the workspace the K range is sliced (deterministic slab
    reduction); same result as the unsliced kernel and as torch's conv2d."""
    import torch.nn.functional as F

    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(N + H + Cin + mode)
    Hi = H * 2 if mode == 2 else (H // 2 if mode == 1 else H)
    x = torch.randn(N, Cin, Hi, Hi, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half()
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(N, Cout, H, H, generator=g).half()
    xf = x.float()
    if mode == 1:
        xf = F.interpolate(xf, scale_factor=2, mode="nearest")
    ref = F.conv2d(xf, w.float(), b, padding=1, stride=2 if mode == 2 else 1) + res.float()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xin, wp, bd, rd = nhwc(x).to(dev), w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(dev), b.to(dev), nhwc(res).to(dev)
    need = L.lfm_conv3x3_workspace_bytes(N, H, H, Cin, Cout)
    assert need > 0, "these shapes are the split-K regime"
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def run(use_ws):
        out = torch.empty(N * H * H, Cout, dtype=torch.float16, device=dev)
        hip.check(L.lfm_conv3x3_f16_ws(hip.ptr(xin), hip.ptr(wp), hip.ptr(bd), hip.ptr(rd), hip.ptr(out), N, H, H, Cin, Cout, mode,
                                       hip.ptr(ws) if use_ws else None, need if use_ws else 0, hip.stream_ptr()), "conv")
        torch.cuda.synchronize()
        return out

    split, plain = run(True), run(False)
    assert torch.equal(split, run(True))
    got = split.reshape(N, H, H, Cout).permute(0, 3, 1, 2)
    assert rel_l2(got, ref) < 2e-3
    assert rel_l2(split, plain) < 1e-3


@pytest.mark.parametrize("N,H,Cin,Cout,mode", [(64, 8, 768, 768, 0), (32, 16, 1024, 512, 2), (64, 8, 1536, 768, 1), (32, 8, 1024, 512, 0)])
def test_conv3x3_split_k_on_the_256_kernel(N, H, Cin, Cout, mode):
    """The UNets' deep small-map convolutions AT BENCH BATCH SIZES (M = N H W >= 2048, >= 24 K-tiles per slice) take their split-K slices on the 256x256 kernel
    (csrc/gemm_kernel.h: splitk256_slices -- the stateful ASrcConv tap walk started in the middle of the K range, stride-2 / nearest-upsample source addressing,
    the fp32 slab epilogue of that kernel); round-5 advisor finding: no parity case reached it (every shape of test_conv3x3_split_k_small_maps has M <= 512).
    Checked against torch's conv2d, against the 128x128 slices (flag GEMM_SPLITK128) and for bit-repeatability."""
    import torch.nn.functional as F

    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(N + H + Cin + mode)
    Hi = H * 2 if mode == 2 else (H // 2 if mode == 1 else H)
    x = torch.randn(N, Cin, Hi, Hi, generator=g).half()
    w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half()
    b = torch.randn(Cout, generator=g) * 0.1
    res = torch.randn(N, Cout, H, H, generator=g).half()
    xf = x.float()
    if mode == 1:
        xf = F.interpolate(xf, scale_factor=2, mode="nearest")
    ref = F.conv2d(xf, w.float(), b, padding=1, stride=2 if mode == 2 else 1) + res.float()
    nhwc = lambda t: t.permute(0, 2, 3, 1).contiguous()
    xin, wp, bd, rd = nhwc(x).to(dev), w.permute(0, 2, 3, 1).reshape(Cout, -1).contiguous().to(dev), b.to(dev), nhwc(res).to(dev)
    need = L.lfm_conv3x3_workspace_bytes(N, H, H, Cin, Cout)
    assert need > 0, "these shapes are the split-K regime"
    ws = torch.empty(need, dtype=torch.uint8, device=dev)

    def run(flags):
        out = torch.empty(N * H * H, Cout, dtype=torch.float16, device=dev)
        hip.gemm_select(flags << 4)
        try:
            hip.check(L.lfm_conv3x3_f16_ws(hip.ptr(xin), hip.ptr(wp), hip.ptr(bd), hip.ptr(rd), hip.ptr(out), N, H, H, Cin, Cout, mode, hip.ptr(ws), need,
                                           hip.stream_ptr()), "conv")
            torch.cuda.synchronize()
        finally:
            hip.gemm_select(0)
        return out

    big, small = run(0), run(hip.DBG_GEMM_SPLITK128)
    assert torch.equal(big, run(0))
    assert rel_l2(big.reshape(N, H, H, Cout).permute(0, 3, 1, 2), ref) < 2e-3
    assert rel_l2(small.reshape(N, H, H, Cout).permute(0, 3, 1, 2), ref) < 2e-3
    assert rel_l2(big, small) < 1e-3


def test_unet_fullsize_vs_oracle_and_fused_sampling():
    """celeb256-ADM-like configuration (nf 256, ch_mult 1 2 2 2, attn at ds 16/8, 4 heads) at reduced depth of batch:
    one velocity evaluation vs the CPU oracle, then a 4-step Euler solve: graph-captured vs eager loop vs oracle."""
    from argparse import Namespace

    from lfm_amd.models import create_network
    from lfm_amd.test_flow_latent import sample_from_model
    from oracle import ode_ref, unet_ref

    dev = torch.device("cuda:0")
    args = Namespace(use_origin_adm=True, layout=False, model_type="adm", image_size=128, f=8, num_in_channels=4, num_out_channels=4,
                     nf=128, num_res_blocks=1, attn_resolutions=(4, 2), dropout=0.0, ch_mult=(1, 2, 2), resamp_with_conv=True, num_classes=None,
                     num_heads=4, num_head_channels=-1, num_head_upsample=-1)  # the _ddp parser's missing flags take their defaults
    cfg = dict(image_size=16, in_channels=4, model_channels=128, out_channels=4, num_res_blocks=1, attention_resolutions=(4, 2),
               channel_mult=(1, 2, 2), num_classes=None, num_heads=4, num_head_channels=-1, num_heads_upsample=-1)
    sd = unet_ref.make_unet_state(cfg, seed=3)
    m = create_network(args)
    m.load_state_dict(sd, strict=True)
    m = m.to(dev).eval()
    g = torch.Generator().manual_seed(5)
    x0 = torch.randn(3, 4, 16, 16, generator=g)
    t = torch.tensor([0.9, 0.4, 0.1])
    ref = unet_ref.unet_forward(sd, cfg, t, x0)
    assert rel_l2(m(t.to(dev), x0.to(dev)), ref) < 3e-3
    sargs = Namespace(method="euler", step_size=0.25, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)
    fused = sample_from_model(m, x0.to(dev), {}, sargs)[-1]
    sargs.fused = False
    eager = sample_from_model(m, x0.to(dev), {}, sargs)[-1]
    oracle = ode_ref.odeint(lambda tt, xx: unet_ref.unet_forward(sd, cfg, tt, xx), x0, torch.tensor([1.0, 0.0]), method="euler",
                            options={"step_size": 0.25})[-1]
    # GroupNorm statistics are a two-stage fixed-order reduction (no atomics): the forward is deterministic bit for bit, and the
    # captured-graph solve runs exactly the kernels of the eager loop
    v1, v2 = m(t.to(dev), x0.to(dev)), m(t.to(dev), x0.to(dev))
    assert torch.equal(v1, v2)
    assert rel_l2(fused, eager) < 1e-6
    assert rel_l2(fused, oracle) < 2e-3


def test_graphed_solve_replayed_after_the_device_went_idle():
    """Regression: the GroupNorm statistics used to be zeroed with hipMemsetAsync, i.e. a memset NODE inside the captured graph of the
    host-sequenced UNet; replaying that graph on an idle device (a synchronize between two solves) produced NaN latents, while
    back-to-back solves and the eager loop were fine.  Two 50-step solves separated by a synchronize must agree with the eager loop."""
    from argparse import Namespace

    from lfm_amd.models import create_network
    from lfm_amd.test_flow_latent import dezero_, sample_from_model

    dev = torch.device("cuda:0")
    args = Namespace(use_origin_adm=True, layout=False, model_type="adm", image_size=128, f=8, num_in_channels=4, num_out_channels=4,
                     nf=128, num_res_blocks=1, attn_resolutions=(4, 2), dropout=0.0, ch_mult=(1, 2, 2), resamp_with_conv=True, num_classes=None,
                     num_heads=4, num_head_channels=-1, num_head_upsample=-1)
    torch.manual_seed(0)
    m = dezero_(create_network(args)).to(dev).eval()
    x = torch.randn(8, 4, 16, 16, device=dev)
    sargs = Namespace(method="euler", step_size=0.02, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)
    sample_from_model(m, x, {}, sargs)  # captures the graph; result dropped
    torch.cuda.synchronize()            # the device goes idle
    second = sample_from_model(m, x, {}, sargs)[-1].clone()
    torch.cuda.synchronize()
    third = sample_from_model(m, x, {}, sargs)[-1].clone()
    sargs.fused = False
    eager = sample_from_model(m, x, {}, sargs)[-1]
    assert bool(torch.isfinite(second).all()) and bool(torch.isfinite(third).all()) and bool(torch.isfinite(eager).all())
    assert torch.equal(second, third)  # deterministic replays
    assert rel_l2(second, eager.cpu()) < 1e-5 and rel_l2(third, eager.cpu()) < 1e-5


@pytest.mark.parametrize("which", ["all", "updown"])
def test_unet_options_match_reference_golden(golden_dir, which):
    """use_scale_shift_norm=False / resblock_updown=True / use_new_attention_order=True (unet.py:131-238,341-369), all together and up/down alone, against
    outputs of the unmodified reference UNetModel (tests/golden/unet_opts.pt)."""
    from lfm_amd.models.unet import UNetModel

    rec = torch.load(os.path.join(golden_dir, "unet_opts.pt"), map_location="cpu", weights_only=False)[which]
    dev = torch.device("cuda:0")
    m = UNetModel(**rec["cfg"])
    m.load_state_dict({k: v.float() for k, v in rec["state_dict"].items()}, strict=True)
    m = m.to(dev).eval()
    got = m(rec["t"].to(dev), rec["x"].to(dev))
    assert float(rec["v"].abs().mean()) > 1e-2
    assert rel_l2(got, rec["v"]) < 3e-3


@pytest.mark.parametrize("N,heads,ch,T", [(2, 4, 128, 256), (3, 2, 64, 256), (2, 4, 64, 64), (1, 8, 128, 64), (2, 2, 96, 64)])
def test_unet_attention_mfma_vs_torch_and_the_valu_kernel(N, heads, ch, T):
    """QKVAttentionLegacy (unet.py:310-334) on the resident MFMA kernel (csrc/unet_attention_kernel.h; T = 64 / 256, ch = 64 / 128) against fp32 torch on the same fp16 operands and
    against the VALU kernel (flag UNET_ATT_VALU); any other shape (ch = 96 here) must still take the VALU kernel and agree with torch.  Scores have a
    realistic spread (|s| up to ~8 after scaling), so a wrong max / sum would show."""
    from lfm_amd import hip

    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(N + heads + ch + T)
    L = hip.lib()
    qkv = (torch.randn(N, heads * 3 * ch, T, generator=g) * 1.6).half()
    q, k, v = qkv.float().reshape(N * heads, 3 * ch, T).split(ch, dim=1)
    wgt = torch.softmax(torch.einsum("bct,bcs->bts", q * ch ** -0.25, k * ch ** -0.25), -1)
    ref = torch.einsum("bts,bcs->bct", wgt, v).reshape(N, heads * ch, T)
    tok = qkv.permute(0, 2, 1).reshape(N * T, heads * 3 * ch).contiguous().to(dev)

    def run(flags):
        out = torch.full((N * T, heads * ch), float("nan"), dtype=torch.float16, device=dev)
        hip.gemm_select(flags << 4)
        try:
            hip.check(L.lfm_attention_small_f16(hip.ptr(tok), hip.ptr(out), N, T, heads, ch, hip.stream_ptr()), "attn")
        finally:
            hip.gemm_select(0)
        return out.reshape(N, T, heads * ch).permute(0, 2, 1).float().cpu()

    got = run(0)
    assert torch.isfinite(got).all()
    assert rel_l2(got, ref) < 2e-3
    if 64 * (T + 1) * 4 + 2 * T * (ch + 2) * 2 <= 160 * 1024:  # the VALU kernel keeps K, V and a score block in the LDS: T = 256 x ch = 128 does not fit (the rule itself: csrc/unet_attention_dispatch.h, unet_attention_valu_lds; written out here by hand on purpose)
        valu = run(hip.DBG_UNET_ATT_VALU)
        assert rel_l2(valu, ref) < 2e-3
        assert rel_l2(got, valu) < 2e-3
    else:
        with pytest.raises(hip.LfmHipError):
            run(hip.DBG_UNET_ATT_VALU)


@pytest.mark.parametrize("N,HW,Ca,Cb,film_on", [(2, 256, 1024, 512, True), (2, 4096, 256, 256, True), (3, 64, 64, 32, False), (2, 1024, 512, 256, True),
                                                 (1, 8192, 128, 256, False)])
def test_two_source_groupnorm_and_linear_equal_the_concatenated_path(N, HW, Ca, Cb, film_on):
    """lfm_groupnorm2_f16 / lfm_linear2_f16 read th.cat([h, skip], dim=1) (unet.py:649) in place: bit-identical to lfm_concat_channels_f16 followed
    by lfm_groupnorm_f16 / lfm_linear_f16.  Shapes: groups straddling the seam (1024 + 512: 48-wide groups) on the fused small-map kernel, the
    three-kernel path at 64x64, the general kernel (96 channels: groups of 3), and a wide map."""
    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(N + HW + Ca + Cb)
    C = Ca + Cb
    xa = (torch.randn(N * HW, Ca, generator=g) * 1.3 + 0.2).half().to(dev)
    xb = (torch.randn(N * HW, Cb, generator=g) * 0.7 - 0.4).half().to(dev)
    cat = torch.empty(N * HW, C, dtype=torch.float16, device=dev)
    hip.check(L.lfm_concat_channels_f16(hip.ptr(xa), hip.ptr(xb), hip.ptr(cat), N * HW, Ca, Cb, hip.stream_ptr()), "cat")
    assert torch.equal(cat, torch.cat([xa, xb], dim=1))
    gamma, beta = (1 + 0.2 * torch.randn(C, generator=g)).to(dev), (0.2 * torch.randn(C, generator=g)).to(dev)
    film = (torch.randn(N, 2 * C, generator=g) * 0.3).to(dev) if film_on else None
    scr = torch.empty(L.lfm_groupnorm_scratch_bytes(N, C), dtype=torch.uint8, device=dev)
    y1, y2 = torch.empty_like(cat), torch.full_like(cat, float("nan"))
    hip.check(L.lfm_groupnorm_f16(hip.ptr(cat), hip.ptr(y1), hip.ptr(gamma), hip.ptr(beta), hip.ptr(film), 2 * C if film_on else 0, hip.ptr(scr),
                                  N, HW, C, 32, 1e-5, 1, hip.stream_ptr()), "gn")
    hip.check(L.lfm_groupnorm2_f16(hip.ptr(xa), Ca, hip.ptr(xb), Cb, hip.ptr(y2), hip.ptr(gamma), hip.ptr(beta), hip.ptr(film),
                                   2 * C if film_on else 0, hip.ptr(scr), N, HW, 32, 1e-5, 1, hip.stream_ptr()), "gn2")
    assert torch.isfinite(y2).all() and torch.equal(y1, y2)
    if Ca % 64 == 0 and C % 64 == 0:  # (the GEMM kernels take K in 32- / 64-deep tiles)
        Nout = 256
        w = (torch.randn(Nout, C, generator=g) / C ** 0.5).half().to(dev)
        b = (torch.randn(Nout, generator=g) * 0.1).to(dev)
        o1, o2 = torch.empty(N * HW, Nout, dtype=torch.float16, device=dev), torch.full((N * HW, Nout), float("nan"), dtype=torch.float16, device=dev)
        hip.check(L.lfm_linear_f16(hip.ptr(cat), C, hip.ptr(w), C, hip.ptr(o1), Nout, N * HW, Nout, C, hip.ptr(b), None, hip.stream_ptr()), "linear")
        hip.check(L.lfm_linear2_f16(hip.ptr(xa), Ca, hip.ptr(xb), Cb, hip.ptr(w), C, hip.ptr(o2), Nout, N * HW, Nout, hip.ptr(b), None,
                                    hip.stream_ptr()), "linear2")
        assert torch.equal(o1, o2)
        ref = cat.float() @ w.float().t() + b
        assert rel_l2(o2, ref) < 2e-3


@pytest.mark.parametrize("N,H,W,Cin,nch", [(2, 32, 48, 128, 3), (1, 64, 64, 256, 4), (3, 16, 16, 192, 1)])
def test_halo_output_conv_vs_torch_and_the_implicit_gemm(N, H, W, Cin, nch):
    """lfm_conv3x3_out_f32 (the UNets' / the VAE decoder's <= 4-channel output convolution, fp16 NHWC -> fp32 NCHW) on the halo-tiled kernel
    (conv3x3_halo_out_kernel, forced at these small sizes with flag CONV_HALO_SMALL) against torch and against the implicit GEMM (flag CONV_IMPLICIT_GEMM):
    border and interior tiles, 4 / 6 / 8 channel quarters, 1 / 3 / 4 real output channels."""
    import torch.nn.functional as F

    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(N + H + Cin + nch)
    x = torch.randn(N, Cin, H, W, generator=g).half()
    w = (torch.randn(nch, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).half()
    b = torch.randn(nch, generator=g) * 0.1
    w4 = torch.zeros(4, 9 * Cin, dtype=torch.float16)
    w4[:nch] = w.permute(0, 2, 3, 1).reshape(nch, -1)
    b4 = torch.zeros(4)
    b4[:nch] = b
    xin, w4d, b4d = x.permute(0, 2, 3, 1).contiguous().to(dev), w4.to(dev), b4.to(dev)
    ref = F.conv2d(x.float(), w.float(), b, padding=1)

    def run(flags):
        out = torch.full((N, nch, H, W), float("nan"), device=dev)
        hip.gemm_select(flags << 4)
        try:
            hip.check(L.lfm_conv3x3_out_f32(hip.ptr(xin), hip.ptr(w4d), hip.ptr(b4d), hip.ptr(out), N, H, W, Cin, nch, hip.stream_ptr()), "out conv")
        finally:
            hip.gemm_select(0)
        return out.cpu()

    halo = run(hip.DBG_CONV_HALO_SMALL)
    assert torch.isfinite(halo).all()
    assert rel_l2(halo, ref) < 1e-4  # fp32 accumulation and output: only the summation order differs from torch
    assert rel_l2(run(hip.DBG_CONV_IMPLICIT_GEMM), halo) < 1e-5


@pytest.mark.parametrize("N,H,W,Cin,Cout", [(2, 24, 40, 4, 256), (3, 16, 16, 9, 128), (1, 33, 17, 8, 192), (2, 8, 8, 16, 64)])
def test_input_conv_mfma_vs_torch_and_the_scalar_kernel(N, H, W, Cin, Cout):
    """lfm_conv3x3_in_f32 (fp32 NCHW latent -> fp16 NHWC, unet.py:416-420; 4 / 8 / 9 / 16 input channels = plain, semantic, inpainting, widest) on
    the MFMA kernel with hi / lo-split operands against torch fp32 and against the scalar fp32 kernel (flag UNET_CONV_IN_SCALAR): the fp32 results agree to ~2^-20, so
    after the fp16 rounding of the output the two kernels differ by at most one ulp, and only rarely."""
    import torch.nn.functional as F

    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(N + H + Cin + Cout)
    x = torch.randn(N, Cin, H, W, generator=g) * 1.5
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g) * 0.1
    ref = F.conv2d(x, w, b, padding=1)
    xd, wd, bd = x.to(dev), w.reshape(Cout, -1).contiguous().to(dev), b.to(dev)

    def run(flags):
        out = torch.full((N * H * W, Cout), float("nan"), dtype=torch.float16, device=dev)
        hip.gemm_select(flags << 4)
        try:
            hip.check(L.lfm_conv3x3_in_f32(hip.ptr(xd), hip.ptr(wd), hip.ptr(bd), hip.ptr(out), N, H, W, Cin, Cout, hip.stream_ptr()), "conv in")
        finally:
            hip.gemm_select(0)
        return out.reshape(N, H, W, Cout).permute(0, 3, 1, 2).float().cpu()

    got, scalar = run(0), run(hip.DBG_UNET_CONV_IN_SCALAR)
    assert torch.isfinite(got).all()
    assert rel_l2(got, ref) < 5e-4 and rel_l2(scalar, ref) < 5e-4
    diff = (got - scalar).abs()
    assert float(diff.max()) <= 2.0 ** -10 * float(ref.abs().max())
    assert float((diff > 0).float().mean()) < 0.01
