"""The streamed UNet attention kernel (csrc/unet_attention_stream_kernel.h; its steps are one text with the resident kernel's, csrc/unet_attention_common.h; the
chooser and the launch: csrc/unet_attention_dispatch.h) behind lfm_attention_small_f16: shapes no other kernel serves, against
float64 per (image, head) item on six constructed input families (tests/unet_attention_cases.py; the yardstick itself is checked without a GPU in
tests/test_unet_attention_ref.py); the small shapes where indexing goes wrong first, forced onto it and compared with the kernel that serves them by
default; nothing that was served before moved; operands that are not 16-byte aligned fall back to the VALU kernel or are refused; and the models that need it, against the CPU oracles and the unmodified reference."""
import os

import pytest
import torch

import unet_attention_cases as uc

pytestmark = pytest.mark.gpu

GUARD = 64  # rows after the last token: NaN in qkv (a key or query read past the end poisons the result), a sentinel in out (a row stored past the end shows)
SENTINEL = -1234.0


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _run(qkv, N, heads, ch, T, flags=0, shift=0, out_shift=0):
    """lfm_attention_small_f16 on guarded buffers -> (out [N * T, heads * ch] fp16 on the device, the out guard on the CPU).  shift / out_shift: qkv / out
    starts that many fp16 values into its (16-byte aligned) buffer."""
    from lfm_amd import hip

    dev = torch.device("cuda:0")
    rows, C = N * T, heads * ch
    buf = torch.full(((rows + GUARD) * 3 * C + shift,), float("nan"), dtype=torch.float16, device=dev)
    tok = buf[shift:].view(rows + GUARD, 3 * C)
    assert tok.data_ptr() % 16 == 2 * shift % 16
    tok[:rows] = uc.tokens(qkv).to(dev)
    out = torch.full(((rows + GUARD) * C + out_shift,), SENTINEL, dtype=torch.float16, device=dev)[out_shift:].view(rows + GUARD, C)
    assert out.data_ptr() % 16 == 2 * out_shift % 16
    hip.gemm_select(flags << 4)
    try:
        hip.check(hip.lib().lfm_attention_small_f16(hip.ptr(tok), hip.ptr(out), N, T, heads, ch, hip.stream_ptr()), "lfm_attention_small_f16")
    finally:
        hip.gemm_select(0)
    torch.cuda.synchronize()
    return out[:rows], out[rows:].cpu()


def _check_case(family, N, heads, ch, T):
    """One family at one shape under the current options: per-item bound, finite, guard untouched, bit-repeatable.  Returns the items [items, T, ch]."""
    qkv, ref = uc.case(family, N, heads, ch, T)
    out, guard = _run(qkv, N, heads, ch, T)
    got = uc.items_of_output(out, N, heads, ch, T)
    err = uc.worst(got, ref)
    print(f"{family} N={N} heads={heads} ch={ch} T={T}: worst item {err:.3e}")
    assert bool(torch.isfinite(out).all()), family
    assert err <= uc.TOL, (family, uc.item_errors(got, ref).tolist())
    assert bool((guard == SENTINEL).all()), family
    again, _ = _run(qkv, N, heads, ch, T)
    assert torch.equal(out, again), family
    return got


# (N, heads, ch, T): beyond the VALU kernel's LDS at 64 / 256 / 48 / 16 / 128 / 192 channels per head; ragged last key blocks (333, 130, 577, 1000), a ragged last
# QUERY block (333: 13 queries in the last workgroup), whole blocks (1024, 320, 4096); 48 and 16 channels = a zero-filled half k-step; 64 key blocks at T = 4096
@pytest.mark.parametrize("N,heads,ch,T", [(2, 2, 64, 333), (1, 2, 256, 130), (2, 3, 48, 577), (1, 2, 16, 1000), (3, 2, 128, 1024), (2, 2, 192, 320),
                                          (1, 1, 64, 4096)])
def test_streamed_kernel_serves_what_was_refused(N, heads, ch, T):
    from lfm_amd import hip

    assert hip.unet_attention_plan(N, T, heads, ch) == 3
    for family in uc.FAMILIES:
        _check_case(family, N, heads, ch, T)


# the small shapes: one token, one short of / one past a key block, two blocks and a key, the four resident shapes (128 x 256 is the largest resident
# instantiation), a VALU shape (ch = 96)
@pytest.mark.parametrize("N,heads,ch,T", [(2, 2, 64, 1), (2, 3, 64, 63), (2, 2, 64, 65), (1, 1, 32, 129), (2, 2, 64, 64), (2, 4, 64, 256), (2, 2, 128, 64),
                                          (2, 2, 96, 64), (1, 2, 128, 256)])
def test_streamed_kernel_forced_agrees_with_the_kernel_of_the_shape(N, heads, ch, T):
    from lfm_amd import hip

    default_kernel = hip.unet_attention_plan(N, T, heads, ch)
    assert default_kernel in (1, 2)
    others = {f: uc.items_of_output(_run(uc.case(f, N, heads, ch, T)[0], N, heads, ch, T)[0], N, heads, ch, T) for f in uc.FAMILIES}
    hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 2)
    try:
        assert hip.unet_attention_plan(N, T, heads, ch) == 3
        for family in uc.FAMILIES:
            got = _check_case(family, N, heads, ch, T)
            agree = uc.worst(got, others[family])
            print(f"  against kernel {default_kernel}: {agree:.3e}")
            assert agree <= uc.TOL, (family, default_kernel)
    finally:
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 1)


@pytest.mark.parametrize("N,heads,ch,T", [(2, 4, 128, 256), (3, 2, 64, 256), (2, 4, 64, 64), (1, 8, 128, 64), (2, 2, 96, 64)])
def test_nothing_served_before_moved(N, heads, ch, T):
    """The shapes of tests/test_gpu_unet.py::test_unet_attention_mfma_vs_torch_and_the_valu_kernel: with the streamed kernel available (option 1) the
    output is bit for bit the output without it (option 0)."""
    from lfm_amd import hip

    qkv = uc.make_case("gauss", N, heads, ch, T)
    with_stream, _ = _run(qkv, N, heads, ch, T)
    hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 0)
    try:
        without, _ = _run(qkv, N, heads, ch, T)
    finally:
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 1)
    assert torch.equal(with_stream, without)


def test_misaligned_operands_take_the_valu_kernel_or_are_refused():
    """qkv, or out, 8 bytes past a 16-byte boundary (a view into a larger buffer): the MFMA kernels read and write 16-byte chunks, so the call runs the VALU
    kernel, which reads and writes single fp16 values, where its LDS fits -- (2, 2, 64, 64), a resident shape: bit for bit the aligned run under flag UNET_ATT_VALU -- and is
    refused where it does not: (2, 2, 64, 333), a streamed shape, needs 64 x 334 x 4 + 4 x 333 x 66 = 173 416 bytes > 160 KiB."""
    from lfm_amd import hip

    N, heads, ch, T = 2, 2, 64, 64
    assert hip.unet_attention_plan(N, T, heads, ch) == 2
    for family in uc.FAMILIES:
        qkv = uc.case(family, N, heads, ch, T)[0]
        aligned, _ = _run(qkv, N, heads, ch, T, flags=hip.DBG_UNET_ATT_VALU)
        for shifts in (dict(shift=4), dict(out_shift=4)):
            shifted, guard = _run(qkv, N, heads, ch, T, **shifts)
            assert bool(torch.isfinite(shifted).all()), (family, shifts)
            assert torch.equal(shifted, aligned), (family, shifts)
            assert bool((guard == SENTINEL).all()), (family, shifts)
    T = 333
    assert hip.unet_attention_plan(N, T, heads, ch) == 3
    for shifts in (dict(shift=4), dict(out_shift=4)):
        with pytest.raises(hip.LfmHipError):
            _run(uc.case("gauss", N, heads, ch, T)[0], N, heads, ch, T, **shifts)


# ----------------------------------------------------------------------------- models
def _origin_adm(num_heads, num_head_channels):
    from argparse import Namespace

    from lfm_amd.models import create_network
    from oracle import unet_ref

    args = Namespace(use_origin_adm=True, layout=False, model_type="adm", image_size=256, f=8, num_in_channels=4, num_out_channels=4, nf=64,
                     num_res_blocks=1, attn_resolutions=(1, 2), dropout=0.0, ch_mult=(1, 2), resamp_with_conv=True, num_classes=None,
                     num_heads=num_heads, num_head_channels=num_head_channels, num_head_upsample=-1)
    cfg = dict(image_size=32, in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(1, 2), channel_mult=(1, 2),
               num_classes=None, num_heads=num_heads, num_head_channels=num_head_channels, num_heads_upsample=-1)
    sd = unet_ref.make_unet_state(cfg, seed=3)
    m = create_network(args)
    m.load_state_dict(sd, strict=True)
    return m.to(torch.device("cuda:0")).eval(), sd, cfg


def test_origin_adm_attending_at_its_top_level_vs_oracle_and_fused_sampling():
    """guided-diffusion's attention at ds = 1 on 32x32 latents: 4 heads x 16 channels x T = 1024 at the top level (the streamed kernel), T = 256 below.
    One evaluation against the CPU oracle, then a 4-step Euler solve through the graph-captured fixed-grid solver against oracle/ode_ref.py."""
    from argparse import Namespace

    from lfm_amd import hip
    from lfm_amd.test_flow_latent import sample_from_model
    from oracle import ode_ref, unet_ref

    dev = torch.device("cuda:0")
    assert hip.unet_attention_plan(2, 1024, 4, 16) == 3
    m, sd, cfg = _origin_adm(4, -1)
    x0 = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(5))
    t = torch.tensor([0.9, 0.2])
    ref = unet_ref.unet_forward(sd, cfg, t, x0)
    assert float(ref.abs().mean()) > 1e-2
    assert rel_l2(m(t.to(dev), x0.to(dev)), ref) < 3e-3
    sargs = Namespace(method="euler", step_size=0.25, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)
    fused = sample_from_model(m, x0.to(dev), {}, sargs)[-1]
    oracle = ode_ref.odeint(lambda tt, xx: unet_ref.unet_forward(sd, cfg, tt, xx), x0, torch.tensor([1.0, 0.0]), method="euler",
                            options={"step_size": 0.25})[-1]
    assert rel_l2(fused, oracle) < 2e-3


def test_origin_adm_on_a_20x20_latent_with_64_channel_heads_vs_oracle():
    """The same network with num_head_channels = 64 on 20x20 latents: one head x T = 400 at the top level -- six whole key blocks and a ragged one."""
    from lfm_amd import hip
    from oracle import unet_ref

    dev = torch.device("cuda:0")
    assert hip.unet_attention_plan(2, 400, 1, 64) == 3
    m, sd, cfg = _origin_adm(-1, 64)
    x0 = torch.randn(2, 4, 20, 20, generator=torch.Generator().manual_seed(6))
    t = torch.tensor([0.7, 0.1])
    ref = unet_ref.unet_forward(sd, cfg, t, x0)
    assert float(ref.abs().mean()) > 1e-2
    assert rel_l2(m(t.to(dev), x0.to(dev)), ref) < 3e-3


def test_edm_adm_attending_at_32x32_vs_reference(golden_dir):
    """DhariwalUNet with attn_resolutions [32, 16] (its constructor default attends at 32 too) on 32x32 latents: one 64-channel head x T = 1024 (streamed)
    and T = 256 (resident); outputs of the unmodified reference models/EDM.py (tools/make_golden_edm_attn32.py), weights from the seeded state maker."""
    from lfm_amd.models.EDM import DhariwalUNet
    from oracle.edm_state import load_seeded

    dev = torch.device("cuda:0")
    rec = torch.load(os.path.join(golden_dir, "edm_attn32.pt"), map_location="cpu", weights_only=False)
    m = DhariwalUNet(**rec["cfg"])
    checksum = load_seeded(m, rec["state_seed"])
    assert abs(checksum - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"], "the seeded state differs from the one the reference was run with"
    m = m.to(dev).eval()
    x = rec["x"].to(dev)
    assert float(rec["v_t0d"].abs().mean()) > 1e-2
    assert rel_l2(m(torch.tensor(0.6, device=dev), x[:1]), rec["v_t0d"]) < 3e-3
    assert rel_l2(m(torch.tensor([0.9, 0.3], device=dev), x), rec["v_tN"]) < 3e-3


def test_create_network_edm_adm_attending_at_32x32():
    from argparse import Namespace

    from lfm_amd.models import create_network
    from lfm_amd.models.EDM import DhariwalUNet

    a = Namespace(use_origin_adm=False, model_type="adm", image_size=256, f=8, num_in_channels=4, num_out_channels=4, label_dim=0, nf=64,
                  ch_mult=(1, 2), num_res_blocks=1, attn_resolutions=(32, 16), dropout=0.0, label_dropout=0.0)
    m = create_network(a)
    assert isinstance(m, DhariwalUNet)
    m = m.cuda().eval()
    for p in m.parameters():  # de-zero (init_zero convs make the default model output 0)
        if not bool(p.any()):
            torch.nn.init.normal_(p, std=0.02)
    m._packed = None
    v = m(torch.tensor(0.3).cuda(), torch.randn(2, 4, 32, 32).cuda())
    assert v.shape == (2, 4, 32, 32) and torch.isfinite(v).all() and float(v.abs().mean()) > 0
