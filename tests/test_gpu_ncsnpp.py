"""GPU tests of the NCSN++ preset of ``SongUNet`` and of what it needed in kernels (csrc/fir_resample.h, lfm_fourier_embed): the [1,3,3,1] filter in both
directions bit for bit on integer data and element by element on Gaussian data, the zero-border copies, the fused "convolve at padding 2, then filter down"
chain, the Fourier mapping network, and the model against the unmodified reference (tests/golden/ncsnpp_tiny.pt, tools/make_ncsnpp_golden.py).  The float64
restatements are those of tests/ncsnpp_cases.py, pinned to the reference's own Conv2d and embedding in tests/test_ncsnpp_host.py."""
import os
from argparse import Namespace

import numpy as np
import pytest
import torch

import ncsnpp_cases as nc
import song_cases as sc

pytestmark = pytest.mark.gpu

GUARD, SENTINEL = 8, -1234.0  # rows after the last output row: a store past the end shows
RSQRT2 = float(np.float32(0.5 ** 0.5))  # the scale as the kernel receives it
DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _guarded_in(x):
    """x [N, H, W, C] (CPU) on the device between NaN guard rows (two image rows' worth before and after): a border tap that reads memory instead of taking a
    zero shows as NaN."""
    C, g = x.shape[-1], 2 * x.shape[2] + 2
    buf = torch.full((g + x.numel() // C + g, C), float("nan"), dtype=torch.float16, device=DEV)
    buf[g:-g] = x.reshape(-1, C).half().to(DEV)
    return buf[g:-g]


def _guarded_out(M, C):
    return torch.full((M + GUARD, C), SENTINEL, dtype=torch.float16, device=DEV)


def _ints(g, *shape):
    return torch.randint(-8, 9, shape, generator=g).float()


# ------------------------------------------------------------------------------------------------ the filters
@pytest.mark.parametrize("C", [8, 72])  # one 16-byte vector; no power of two
@pytest.mark.parametrize("Ho,Wo", [(3, 5), (8, 2)])
def test_fir_kernels_bit_for_bit_on_integer_data(Ho, Wo, C):
    """Integer-valued fp16 inputs, |x| <= 8; the down weights are k/64 and the up weights k/16, so every output is a multiple of 1/64 (1/16) below 2^10 and
    exactly representable: the kernels must EQUAL the float64 restatement.  N = 2 on non-square maps; NaN guard rows around every input, a sentinel after
    every output."""
    from lfm_amd import hip

    N, g = 2, torch.Generator().manual_seed(100 * Ho + C)
    M = N * Ho * Wo
    bias, resid = _ints(g, C), _ints(g, M, C)
    dbias, dresid = bias.to(DEV), resid.half().to(DEV)
    for pad in (1, 0):
        x = _ints(g, N, 2 * Ho + 2 - 2 * pad, 2 * Wo + 2 - 2 * pad, C)
        dx = _guarded_in(x)
        for epi in (False, True):
            out = _guarded_out(M, C)
            hip.fir_down2(dx, N, Ho, Wo, C, pad=pad, bias=dbias if epi else None, resid=dresid if epi else None, out=out)
            ref = nc.fir_down_ref64(x, pad, *((bias, resid) if epi else ()))
            assert bool((out[M:] == SENTINEL).all()), (pad, epi)
            assert torch.equal(out[:M].double().cpu(), ref.reshape(M, C)), (pad, epi)
            assert float((ref * 64).frac().abs().max()) == 0 and float(ref.abs().max()) < 32  # (the premise: multiples of 1/64 that fp16 holds)
    # up: the input is the Ho x Wo map, the output 2 Ho x 2 Wo
    x = _ints(g, N, Ho, Wo, C)
    out = _guarded_out(4 * M, C)
    hip.fir_up2(_guarded_in(x), N, 2 * Ho, 2 * Wo, C, out=out)
    ref = nc.fir_up_ref64(x)
    assert bool((out[4 * M:] == SENTINEL).all())
    assert torch.equal(out[:4 * M].double().cpu(), ref.reshape(4 * M, C))
    assert float((ref * 16).frac().abs().max()) == 0
    # the zero-border copies: fp16 NHWC, and fp32 planes (the NCHW network input)
    got = hip.zero_border(_guarded_in(x), N, Ho, Wo, C)
    assert torch.equal(got.cpu().reshape(N, Ho + 2, Wo + 2, C), torch.nn.functional.pad(x.half(), (0, 0, 1, 1, 1, 1)))
    planes = torch.full((1 + N * 3 + 1, Ho, Wo), float("nan"), device=DEV)
    planes[1:-1] = torch.arange(1, N * 3 * Ho * Wo + 1, device=DEV, dtype=torch.float32).reshape(N * 3, Ho, Wo)
    got = hip.zero_border(planes[1:-1].reshape(N, 3, Ho, Wo), N, Ho, Wo, 3)
    assert torch.equal(got, torch.nn.functional.pad(planes[1:-1].reshape(N, 3, Ho, Wo), (1, 1, 1, 1)))


def _within(out, ref, mag):
    """|err| <= 2^-11 |ref| (1 + 2^-9) + 2^-20 sum |w_k x_k| + 2^-25: one fp16 rounding (of a value that is itself off by the second term), fp32 accumulation of at
    most 18 terms -- 16 taps, the bias, the residual -- and the fp16 subnormal floor.  Derived, not measured: a kernel outside it rounds more than once."""
    err = (out.double().cpu() - ref).abs()
    bound = 2.0 ** -11 * ref.abs() * (1 + 2.0 ** -9) + 2.0 ** -20 * mag + 2.0 ** -25
    return float((err / bound).max())


@pytest.mark.parametrize("C", [8, 72])
@pytest.mark.parametrize("Ho,Wo", [(3, 5), (8, 2)])
def test_fir_kernels_round_once_on_gaussian_data(Ho, Wo, C):
    from lfm_amd import hip

    N, g = 2, torch.Generator().manual_seed(7 + 100 * Ho + C)
    M = N * Ho * Wo
    bias, resid = torch.randn(C, generator=g), torch.randn(M, C, generator=g).half().float()
    for pad in (1, 0):
        x = torch.randn(N, 2 * Ho + 2 - 2 * pad, 2 * Wo + 2 - 2 * pad, C, generator=g).half().float()
        out = hip.fir_down2(_guarded_in(x), N, Ho, Wo, C, pad=pad, bias=bias.to(DEV), resid=resid.half().to(DEV), scale=RSQRT2)
        ref, mag = nc.fir_down_ref64(x, pad, bias, resid, RSQRT2, terms=True)
        worst = _within(out, ref.reshape(M, C), mag.reshape(M, C))
        bare = _within(hip.fir_down2(_guarded_in(x), N, Ho, Wo, C, pad=pad), *[v.reshape(M, C) for v in nc.fir_down_ref64(x, pad, terms=True)])
        print(f"down pad {pad} {Ho}x{Wo} C={C}: worst |err| / bound = {worst:.3f} (epilogue, scale sqrt(1/2)), {bare:.3f} (bare)")
        assert worst <= 1 and bare <= 1
    x = torch.randn(N, Ho, Wo, C, generator=g).half().float()
    ref, mag = nc.fir_up_ref64(x, terms=True)
    worst = _within(hip.fir_up2(_guarded_in(x), N, 2 * Ho, 2 * Wo, C), ref.reshape(4 * M, C), mag.reshape(4 * M, C))
    print(f"up {Ho}x{Wo} C={C}: worst |err| / bound = {worst:.3f}")
    assert worst <= 1


def test_fir_kernels_refuse_what_they_do_not_serve():
    """The error code comes back before any launch: the output keeps its sentinel."""
    from lfm_amd import hip

    L, st = hip.lib(), hip.stream_ptr()
    x = torch.zeros(2 * 10 * 10 * 16 + 8, dtype=torch.float16, device=DEV)
    out = torch.full((2 * 4 * 4 * 16 + 8,), SENTINEL, dtype=torch.float16, device=DEV)
    p, o = hip.ptr(x), hip.ptr(out)
    odd_x, odd_o = hip.ptr(x[4:]), hip.ptr(out[4:])  # 8 bytes off a 16-byte boundary
    SHAPE, ALIGN, ARG = -1, -2, -5
    assert L.lfm_fir_down2_f16(p, o, None, None, 1.0, 2, 4, 4, 12, 1, st) == SHAPE  # C % 8 != 0
    assert L.lfm_fir_down2_f16(p, o, None, None, 1.0, 2, 4, 4, 16, 2, st) == SHAPE  # pad is 0 or 1
    assert L.lfm_fir_down2_f16(odd_x, o, None, None, 1.0, 2, 4, 4, 16, 1, st) == ALIGN
    assert L.lfm_fir_down2_f16(p, odd_o, None, None, 1.0, 2, 4, 4, 16, 1, st) == ALIGN
    assert L.lfm_fir_down2_f16(p, o, None, odd_x, 1.0, 2, 4, 4, 16, 1, st) == ALIGN  # the residual
    assert L.lfm_fir_down2_f16(None, o, None, None, 1.0, 2, 4, 4, 16, 1, st) == ARG
    assert L.lfm_fir_up2_f16(p, o, 2, 3, 4, 16, st) == SHAPE  # an odd Ho
    assert L.lfm_fir_up2_f16(p, o, 2, 4, 4, 12, st) == SHAPE
    assert L.lfm_fir_up2_f16(odd_x, o, 2, 4, 4, 16, st) == ALIGN
    assert L.lfm_zero_border_f16(p, o, 1, 2, 2, 12, st) == SHAPE
    assert L.lfm_zero_border_f16(p, odd_o, 1, 2, 2, 16, st) == ALIGN
    assert L.lfm_zero_border_f32(p, hip.ptr(out[1:]), 1, 2, 2, st) == ALIGN  # 2 bytes off
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ the fused path, composed
@pytest.mark.parametrize("Cin,Cout", [(64, 128), (4, 64)])  # fp16 NHWC through lfm_conv3x3_f16; the fp32 NCHW network input through lfm_conv3x3_in_f32
def test_fused_down_path_composed_of_border_conv_and_filter(Cin, Cout):
    """border copy -> the existing pad-1 3x3 convolution on the (H+2) x (W+2) map -> lfm_fir_down2_f16(pad 0, late bias, residual, scale) against the
    float64 restatement of Conv2d(kernel=3, down=True, fused_resample=True) and of the encoder's (x + .) / sqrt(2), at the rel-L2 bound of the scaled-
    epilogue convolution tests; filtering first (pad 1, then a pad-1 convolution on the small map) lies outside it."""
    from lfm_amd import hip

    L, N, H, W = hip.lib(), 2, 8, 12
    g = torch.Generator().manual_seed(11 + Cin)
    w4 = torch.randn(Cout, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5
    bias = 0.5 * torch.randn(Cout, generator=g)
    resid = torch.randn(N * (H // 2) * (W // 2), Cout, generator=g).half()
    if Cin % 64:
        x = torch.randn(N, Cin, H, W, generator=g)
        xb = hip.zero_border(x.to(DEV), N, H, W, Cin)
        full = torch.empty(N * (H + 2) * (W + 2), Cout, dtype=torch.float16, device=DEV)
        wd, no_bias = w4.to(DEV), torch.zeros(Cout, device=DEV)  # the bias comes after the filter
        hip.check(L.lfm_conv3x3_in_f32(hip.ptr(xb), hip.ptr(wd), hip.ptr(no_bias), hip.ptr(full), N, H + 2, W + 2, Cin, Cout, hip.stream_ptr()),
                  "lfm_conv3x3_in_f32")
        xh = nc.nhwc(x)
    else:
        xh, w4 = torch.randn(N, H, W, Cin, generator=g).half().float(), w4.half().float()
        xb = hip.zero_border(xh.half().to(DEV).reshape(-1, Cin), N, H, W, Cin)
        wk = w4.permute(0, 2, 3, 1).reshape(Cout, 9 * Cin).half().to(DEV)  # [Cout][tap][Cin], as pack_conv3 lays it out
        full = torch.empty(N * (H + 2) * (W + 2), Cout, dtype=torch.float16, device=DEV)
        hip.check(L.lfm_conv3x3_f16(hip.ptr(xb), hip.ptr(wk), None, None, hip.ptr(full), N, H + 2, W + 2, Cin, Cout, 0, hip.stream_ptr()), "lfm_conv3x3_f16")
    M = N * (H // 2) * (W // 2)
    out = _guarded_out(M, Cout)
    hip.fir_down2(full, N, H // 2, W // 2, Cout, pad=0, bias=bias.to(DEV), resid=resid.to(DEV), scale=RSQRT2, out=out)
    ref = nc.fused_down_ref64(xh, w4, bias, resid, RSQRT2).reshape(M, Cout)
    wrong = nc.fused_down_ref64(xh, w4, bias, resid, RSQRT2, fault="filter_first").reshape(M, Cout)
    e, e_fault = rel_l2(out[:M], ref), rel_l2(wrong, ref)
    print(f"fused down {Cin} -> {Cout}, {H}x{W}: rel-L2 vs float64 {e:.3e}; the filter-first fault {e_fault:.3e}")
    assert bool((out[M:] == SENTINEL).all())
    assert e < 2e-3 < 10 * 2e-3 < e_fault


# ------------------------------------------------------------------------------------------------ the Fourier mapping network
@pytest.mark.parametrize("F", [128, 256])
def test_fourier_mapping_kernel_vs_float64_with_song_embed_as_control(F):
    """lfm_fourier_embed against its float64 restatement (pinned to the reference in tests/test_ncsnpp_host.py; it takes the argument with the reference's
    two fp32 roundings), with lfm_song_embed against ITS restatement on the same weights, times and labels as the control: the kernels differ in the
    argument of the sine alone, so the new kernel's worst absolute error may be at most twice the control's -- the rule the DDPM++ mapping test set."""
    from lfm_amd import hip

    L, dev, N, E, rows = hip.lib(), torch.device(DEV), 5, 2 * F, 7  # noise_channels F = 2 model_channels, E = 4 model_channels
    g = torch.Generator().manual_seed(F)
    w0, b0 = torch.randn(E, F, generator=g) / F ** 0.5, 0.1 * torch.randn(E, generator=g)
    w1, b1 = torch.randn(E, E, generator=g) / E ** 0.5, 0.1 * torch.randn(E, generator=g)
    lab_w, lab_b = 0.3 * torch.randn(F, rows, generator=g), 0.1 * torch.randn(F, generator=g)
    freqs = nc.seeded_freqs(F // 2, seed=F)
    y = torch.tensor([3, 0, 6, 1, 5])
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    keep = [d(v) for v in (w0, b0, w1, b1)]
    dw = [hip.ptr(v) for v in keep]
    dlab_t, dlab_b, dy, dfreqs = d(lab_w.t()), d(lab_b), d(y), d(freqs)

    def run(fourier, t, labels, yy=dy):
        emb, emb16, h1 = torch.empty(N, E, device=dev), torch.empty(N, E, device=dev, dtype=torch.float16), torch.empty(N, E, device=dev)
        rest = (*dw, hip.ptr(dlab_t if labels else None), hip.ptr(dlab_b if labels else None), rows ** 0.5, hip.ptr(yy if labels else None), rows,
                hip.ptr(h1), hip.ptr(emb), hip.ptr(emb16), N, F, E, hip.stream_ptr())
        if fourier:
            hip.check(L.lfm_fourier_embed(hip.ptr(t), t.numel(), hip.ptr(dfreqs), *rest), "lfm_fourier_embed")
        else:
            hip.check(L.lfm_song_embed(hip.ptr(t), t.numel(), *rest), "lfm_song_embed")
        return emb, emb16

    assert float(nc.fourier_args32(torch.tensor([1.0]), freqs).abs().max()) > 100  # radians
    worst_new = worst_ctl = 0.0
    for t in (torch.tensor([0.6]), torch.tensor([1.0, 0.9, 0.31, 0.05, 0.0])):  # t_len 1 and N; the solver's range [0, 1] with both ends
        for labels in (False, True):
            lab = (lab_w, lab_b, y) if labels else ()
            emb, emb16 = run(True, d(t), labels)
            ref = nc.fourier_mapping_ref64(freqs, w0, b0, w1, b1, t, N, *lab)
            ctl, _ = run(False, d(t), labels)
            ctl_ref = sc.song_mapping_ref64(w0, b0, w1, b1, t, N, *lab)
            e_new, e_ctl = float((emb.double().cpu() - ref).abs().max()), float((ctl.double().cpu() - ctl_ref).abs().max())
            e_swap = float((nc.fourier_mapping_ref64(freqs, w0, b0, w1, b1, t, N, *lab, swap=False) - ref).abs().max())
            print(f"F={F} t_len={t.numel()} labels={labels}: lfm_fourier_embed {e_new:.3e}  lfm_song_embed (control) {e_ctl:.3e}  un-swapped order {e_swap:.3e}")
            assert bool(((emb16.double() - emb.double()).abs() <= 2.0 ** -11 * (1 + 2.0 ** -10) * emb.double().abs() + 2.0 ** -25).all())
            assert e_swap > 1e-2
            worst_new, worst_ctl = max(worst_new, e_new), max(worst_ctl, e_ctl)
    print(f"F={F}: worst lfm_fourier_embed {worst_new:.3e}, worst control {worst_ctl:.3e}, ratio {worst_new / worst_ctl:.2f}")
    assert worst_ctl < 1e-5  # the control itself is sane (fp32 round-off of O(1) sums)
    assert worst_new <= 2 * worst_ctl
    bad = d(torch.tensor([3, rows, 6, -1, 5]))  # out of range on rows 1 and 3: poisoned, the others untouched
    emb, emb16 = run(True, d(torch.tensor([0.6])), True, bad)
    good, _ = run(True, d(torch.tensor([0.6])), True)
    assert bool(emb[[1, 3]].isnan().all()) and bool(emb16[[1, 3]].isnan().all()) and torch.equal(emb[[0, 2, 4]], good[[0, 2, 4]])
    assert L.lfm_fourier_embed(hip.ptr(d(torch.tensor([0.6]))), 1, None, *dw, None, None, 1.0, None, 0, hip.ptr(emb), hip.ptr(emb), hip.ptr(emb16), N, F, E,
                               hip.stream_ptr()) == -5  # no table: an argument error, not the positional embedding


# ------------------------------------------------------------------------------------------------ the model against the reference
@pytest.fixture(scope="module")
def tiny(golden_dir):
    from lfm_amd.models.EDM import SongUNet

    rec = torch.load(os.path.join(golden_dir, "ncsnpp_tiny.pt"), map_location="cpu", weights_only=False)
    m = SongUNet(**rec["cfg"])
    checksum = nc.load_seeded(m, rec["state_seed"])
    assert abs(checksum - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"], "the seeded state differs from the one the reference was run with"
    return rec, m.to(DEV).eval()


def test_ncsnpp_tiny_matches_reference_golden(tiny):
    rec, m = tiny
    dev = torch.device(DEV)
    x, y = rec["x"].to(dev), rec["y"].to(dev)
    assert float(rec["v_t0d"].abs().mean()) > 1e-2
    a = m(torch.tensor(0.6, device=dev), x, y).clone()
    errs = dict(t0d=rel_l2(a, rec["v_t0d"]), tN=rel_l2(m(rec["tN"].to(dev), x, y), rec["v_tN"]),
                nolabel=rel_l2(m(torch.tensor(0.6, device=dev), x), rec["v_nolabel"]))
    print("ncsnpp_tiny rel-L2 vs reference:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < 3e-3, errs  # the DDPM++ test's bound for the same class
    assert torch.equal(a, m(torch.tensor(0.6, device=dev), x, y))  # bit-repeatable
    with pytest.raises(IndexError):
        m(torch.tensor(0.6, device=dev), x, torch.tensor([1, 5, 0], device=dev))  # label_dim is 5


def test_ncsnpp_tiny_euler_solve_captured_and_uncaptured(tiny):
    from lfm_amd.test_flow_latent import sample_from_model

    rec, m = tiny
    dev = torch.device(DEV)
    x, kw = rec["x"].to(dev), dict(y=rec["y"].to(dev))
    args = Namespace(method="euler", step_size=0.1, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)
    fused = sample_from_model(m, x, kw, args)[-1]
    assert m._fused_solvers and all(fg.graphs for fg in m._fused_solvers.values())  # the captured path is what ran
    e_ref = rel_l2(fused, rec["x_euler10"])
    args.fused = False
    e_unc = rel_l2(sample_from_model(m, x, kw, args)[-1], fused)
    print(f"ncsnpp_tiny 10 Euler steps: captured vs reference {e_ref:.3e}, uncaptured vs captured {e_unc:.3e}")
    assert e_ref < 1e-3 and e_unc < 1e-5
