"""GPU: every GroupNorm statistics path against a float64 reference of the very fp16 tensor the kernel normalised.

Paths: lfm_groupnorm_f16 (the UNets: fused small-map kernel, three-kernel "rows" and "groups" layouts), lfm_groupnorm2_f16 (the in-place channel
concat), lfm_vae_groupnorm_f16 (the decoder's own statistics pass, both slab policies) and lfm_vae_conv3x3_gn_f16 (the decoder's convolution ->
GroupNorm hand-over, statistics from the halo convolution's epilogue, the 256-row GEMM epilogues or the separate pass).

Input families: a centred control, whole-group offsets of 30 / 100 / 300 standard deviations, per-channel offsets inside a group, one channel per
group at +-3000, constant groups (output = silu(beta)) and near-constant groups (two adjacent fp16 values around 500: the true variance is tiny, so
any error of the computed one is multiplied by up to 1 / sqrt(eps)).  One bound for every family, the control's: rel-L2 <= 1e-3 and
max-abs <= 2^-8 max(1, max |ref|); two runs are bit-identical.
"""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from lfm_amd import hip

pytestmark = pytest.mark.gpu

FAMILIES = ["centred", "offset30", "offset100", "offset300", "channel_offsets", "spike3000", "constant", "near_constant"]
G = 32


def family(name, n, HW, C_, groups, seed, dev):
    """fp16 [n, HW, C_] whose groups (contiguous channel runs of C_ / groups) follow the family."""
    g = torch.Generator(device=dev).manual_seed(seed)
    cpg = C_ // groups
    noise = torch.randn(n, HW, C_, generator=g, device=dev)
    sign = torch.where(torch.arange(groups, device=dev) % 2 == 0, 1.0, -1.0).repeat_interleave(cpg)  # both signs of offset
    if name == "centred":
        x = noise
    elif name.startswith("offset"):
        x = noise + float(name[6:]) * sign
    elif name == "channel_offsets":
        x = noise + 100.0 * torch.randn(C_, generator=g, device=dev)
    elif name == "spike3000":
        spike = torch.zeros(C_, device=dev)
        spike[::cpg] = 3000.0 * sign[::cpg]
        x = noise + spike
    elif name == "constant":
        x = (torch.randn(n, 1, groups, 1, generator=g, device=dev) * 20).expand(n, HW, groups, cpg).reshape(n, HW, C_)
    elif name == "near_constant":  # 500 or 500.25 (adjacent fp16 values), a different mix per group
        p = torch.rand(n, 1, groups, 1, generator=g, device=dev).expand(n, HW, groups, cpg).reshape(n, HW, C_)
        x = 500.0 + 0.25 * (torch.rand(n, HW, C_, generator=g, device=dev) < p).float()
    else:
        raise ValueError(name)
    return x.half()


def reference(x, groups, gamma, beta, eps, silu, film=None):
    """float64 GroupNorm (+ FiLM, SiLU) of the fp16 tensor x [n, HW, C] -> [n, HW, C] float64."""
    n, HW, C_ = x.shape
    y = F.group_norm(x.double().permute(0, 2, 1), groups, gamma.double(), beta.double(), eps=eps)
    if film is not None:
        y = y * (1 + film[:, :C_, None].double()) + film[:, C_:, None].double()
    if silu:
        y = F.silu(y)
    return y.permute(0, 2, 1)


def check(got, ref, what):
    got = got.reshape(ref.shape).double()
    assert bool(torch.isfinite(got).all()), what
    err = got - ref
    rel = float(err.norm() / ref.norm().clamp_min(1e-30))
    mx, bound = float(err.abs().max()), 2.0 ** -8 * max(1.0, float(ref.abs().max()))
    assert rel <= 1e-3 and mx <= bound, f"{what}: rel-L2 {rel:.3e} (<= 1e-3), max-abs {mx:.3e} (<= {bound:.3e})"


def affine(C_, seed, dev, film_rows=0):
    g = torch.Generator().manual_seed(seed)
    gamma, beta = 1 + 0.2 * torch.randn(C_, generator=g), 0.5 * torch.randn(C_, generator=g)
    film = torch.randn(film_rows, 2 * C_, generator=g) * 0.3 if film_rows else None
    return gamma.to(dev), beta.to(dev), (film.to(dev) if film is not None else None)


def with_flags(flags, fn):
    from lfm_amd import hip

    hip.gemm_select(flags)
    try:
        return fn()
    finally:
        hip.gemm_select(0)


# ------------------------------------------------------------------ lfm_groupnorm_f16 (UNets)
# (N, HW, C, groups, film, flags, (statistics, apply) kernels the case is about -- asserted against lfm_groupnorm_plan before the launch; the rule itself
# is stated once, in the header of csrc/groupnorm_dispatch.h --, label)
FUSED = (hip.GN_STATS_FUSED, hip.GN_APPLY_FUSED)
ROWS, GROUPS4, GROUPS1 = hip.GN_STATS_ROWS, hip.GN_STATS_GROUPS4, hip.GN_STATS_GROUPS1
OCTET, CHUNK = hip.GN_APPLY_OCTET, hip.GN_APPLY_CHUNK
UNET_CASES = [
    (8, 1024, 256, 32, True, 0, FUSED, "fused, ADM 32x32 level (boundary HW = 1024)"),
    (3, 100, 512, 32, False, 0, FUSED, "fused, ragged 10x10"),
    (2, 64, 2048, 32, True, 0, FUSED, "fused, 64-wide groups"),
    (2, 4096, 128, 32, True, 0, (ROWS, OCTET), "rows, ADM 64x64 level"),
    (3, 1025, 256, 32, False, 0, (ROWS, OCTET), "rows, ragged (boundary HW = 1025)"),
    (4, 256, 512, 32, True, hip.DBG_UNET_GN_ROWS << 4, (ROWS, OCTET), "rows via flag 16384"),
    (2, 300, 96, 32, False, 0, (GROUPS1, CHUNK), "groups layout, cpg 3"),
    (2, 4100, 96, 32, True, 0, (GROUPS1, CHUNK), "groups layout, ragged slabs"),
    (1, 2048, 4096, 32, False, 0, (GROUPS4, CHUNK), "groups layout, cpg 128 (C / 8 > 256)"),
    (2, 300, 384, 32, False, 0, (ROWS, CHUNK), "rows, cpg 12, chunk apply (48 octets do not divide the block)"),
    (2, 300, 64, 32, False, 0, (GROUPS1, OCTET), "groups layout, cpg 2, octet apply"),
]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", UNET_CASES, ids=[c[-1] for c in UNET_CASES])
def test_groupnorm_f16_vs_fp64(case, fam):
    from lfm_amd import hip

    N, HW, C_, groups, film_on, flags, kernels, what = case
    assert with_flags(flags, lambda: hip.groupnorm_plan(N, HW, C_, groups)) == kernels  # the kernels this case is about really run
    dev = torch.device("cuda:0")
    L = hip.lib()
    x = family(fam, N, HW, C_, groups, seed=HW + C_, dev=dev)
    gamma, beta, film = affine(C_, C_ + N, dev, N if film_on else 0)
    eps = 1e-5
    scr = torch.empty(L.lfm_groupnorm_scratch_bytes(N, C_), dtype=torch.uint8, device=dev)

    def run():
        y = torch.empty_like(x)
        hip.check(L.lfm_groupnorm_f16(hip.ptr(x), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(film), 2 * C_ if film_on else 0, hip.ptr(scr), N, HW,
                                      C_, groups, eps, 1, hip.stream_ptr()), "lfm_groupnorm_f16")
        torch.cuda.synchronize()
        return y

    y = with_flags(flags, run)
    assert torch.equal(y, with_flags(flags, run))
    ref = reference(x, groups, gamma, beta, eps, True, film)
    check(y, ref, f"{what} / {fam}")
    # (constant groups: within the family bound.  This apply is x a + (beta - mean a), which leaves the fp32 rounding of mean a, |mean| / sqrt(eps),
    # in the output -- 2e-3 at |mean| = 60, eps = 1e-5 -- so it is not silu(beta) to the fp16 rounding as the decoder's centred apply is, below.)


TWO_SOURCE_CASES = [  # (N, HW, Ca, Cb, film, (statistics, apply) of the plan at C = Ca + Cb, label)
    (4, 256, 512, 256, True, FUSED, "fused, groups straddle the seam"),
    (2, 2048, 256, 128, False, (ROWS, CHUNK), "rows"),
    (2, 512, 128, 64, True, (GROUPS1, CHUNK), "groups layout, groups straddle the seam"),
]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", TWO_SOURCE_CASES, ids=[c[-1] for c in TWO_SOURCE_CASES])
def test_groupnorm2_f16_offset_on_one_source(case, fam):
    """lfm_groupnorm2_f16 on [xa | xb] with the family on xa only (a group that straddles the seam mixes both)."""
    from lfm_amd import hip

    N, HW, Ca, Cb, film_on, kernels, what = case
    C_ = Ca + Cb
    assert hip.groupnorm_plan(N, HW, C_, G) == kernels
    dev = torch.device("cuda:0")
    L = hip.lib()
    xa = family(fam, N, HW, C_, G, seed=HW + Ca, dev=dev)[..., :Ca].contiguous()  # the family's groups as the concat sees them, cut at the seam
    xb = family("centred", N, HW, Cb, 1, seed=HW + Cb + 1, dev=dev)
    gamma, beta, film = affine(C_, C_ + N, dev, N if film_on else 0)
    scr = torch.empty(L.lfm_groupnorm_scratch_bytes(N, C_), dtype=torch.uint8, device=dev)

    def run():
        y = torch.empty(N, HW, C_, dtype=torch.float16, device=dev)
        hip.check(L.lfm_groupnorm2_f16(hip.ptr(xa), Ca, hip.ptr(xb), Cb, hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(film), 2 * C_ if film_on else 0,
                                       hip.ptr(scr), N, HW, G, 1e-5, 1, hip.stream_ptr()), "lfm_groupnorm2_f16")
        torch.cuda.synchronize()
        return y

    y = run()
    assert torch.equal(y, run())
    check(y, reference(torch.cat([xa, xb], dim=2), G, gamma, beta, 1e-5, True, film), f"{what} / {fam}")


# ------------------------------------------------------------------ the VAE decoder's GroupNorm (eps 1e-6)
def vae_gn_workspace(n, HW, C_, dev):
    """The decoder's room for partial statistics (lfm_vae_workspace_bytes: the larger of the epilogue slabs of the full-resolution map and
    64 statistics slabs of 128 half-octets, per image), with this map taken as the full-resolution one."""
    pairs = n * max(HW * 256 // 512, 64 * 128)
    return torch.empty(256 + (n * 256 + 255) // 256 * 256 + pairs * 8, dtype=torch.uint8, device=dev)


# (n, HW, C, statistics slabs per image -- asserted against lfm_vae_groupnorm_plan before the launch --, label): n < 16 -> up to 512 slabs of at least 64 pixels
# per image as far as the workspace has room, n >= 16 -> at most 64 of 1024; HW 64 (R = 8 mid level) .. 65536 (full resolution at R = 32)
VAE_GN_CASES = [
    (1, 65536, 128, 512, "batch-1 full resolution, 512 slabs"),
    (3, 1000, 256, 16, "ragged slabs"),
    (15, 4096, 512, 4, "n = 15, room for 64 slabs only: the 64-slab launch"),
    (16, 4096, 256, 4, "n = 16, first on the 64-slab branch"),
    (64, 1024, 512, 1, "headline mid level (R = 32)"),
    (64, 64, 512, 1, "R = 8 mid level"),
    (16, 16384, 128, 16, "n = 16 at 128x128"),
    (15, 4608, 128, 68, "n = 15, last below the 64-slab branch: 1024 // 15 = 68 ragged slabs"),
]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", VAE_GN_CASES, ids=[c[-1] for c in VAE_GN_CASES])
def test_vae_groupnorm_vs_fp64(case, fam):
    from lfm_amd import hip

    n, HW, C_, slabs, what = case
    dev = torch.device("cuda:0")
    L = hip.lib()
    x = family(fam, n, HW, C_, G, seed=n + HW + C_, dev=dev)
    gamma, beta, _ = affine(C_, C_ + n, dev)
    ws = vae_gn_workspace(n, HW, C_, dev)
    assert hip.vae_groupnorm_plan(n, HW, C_, ws.numel()) == slabs  # the slab policy this case is about really runs
    silu = C_ != 512  # the mid-attention GroupNorm has no SiLU

    def run():
        y = torch.empty_like(x)
        hip.check(L.lfm_vae_groupnorm_f16(hip.ptr(x), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta), hip.ptr(ws), ws.numel(), n, HW, C_, int(silu),
                                          hip.stream_ptr()), "lfm_vae_groupnorm_f16")
        torch.cuda.synchronize()
        return y

    y = run()
    assert torch.equal(y, run())
    check(y, reference(x, G, gamma, beta, 1e-6, silu), f"{what} / {fam}")
    if fam == "constant":  # sigma = 0: (x - mean) rstd gamma + beta is exactly beta, then silu and the fp16 rounding
        b = F.silu(beta.double()) if silu else beta.double()
        assert float((y.double() - b).abs().max()) <= 2.0 ** -10 * max(1.0, float(b.abs().max()))


def test_vae_groupnorm_refuses_a_short_workspace():
    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    x = torch.zeros(16, 64, 128, dtype=torch.float16, device=dev)
    gamma, beta, _ = affine(128, 0, dev)
    ws = torch.empty(256 + 16 * 256 + 16 * 64 * 32 * 8 - 8, dtype=torch.uint8, device=dev)
    rc = L.lfm_vae_groupnorm_f16(hip.ptr(x), hip.ptr(x), hip.ptr(gamma), hip.ptr(beta), hip.ptr(ws), ws.numel(), 16, 64, 128, 1, hip.stream_ptr())
    assert rc == -3  # LFM_ERR_WORKSPACE


# ------------------------------------------------------------------ the decoder's conv3x3 -> GroupNorm hand-over
def conv_family(name, Cout, seed):
    """(bias, weight scale, residual on/off) that give the convolution OUTPUT the family's statistics: offsets through the bias, the spread from
    the convolution itself (std ~ scale); constant groups from zero weights, near-constant ones from 500 + a convolution of std 0.05 that rounds
    to 499.75 / 500 / 500.25."""
    g = torch.Generator().manual_seed(seed)
    cpg = Cout // G
    sign = torch.where(torch.arange(G) % 2 == 0, 1.0, -1.0).repeat_interleave(cpg)
    if name == "centred":
        return 0.1 * torch.randn(Cout, generator=g), 1.0, True
    if name.startswith("offset"):
        return float(name[6:]) * sign, 1.0, True
    if name == "channel_offsets":
        return 100.0 * torch.randn(Cout, generator=g), 1.0, True
    if name == "spike3000":
        b = torch.zeros(Cout)
        b[::cpg] = 3000.0 * sign[::cpg]
        return b, 1.0, True
    if name == "constant":
        return (20 * torch.randn(G, generator=g)).repeat_interleave(cpg), 0.0, False
    if name == "near_constant":
        return torch.full((Cout,), 500.0), 0.05, False
    raise ValueError(name)


# (source, gemm_select value, n, H, Cin, Cout, ups, resid): statistics from the halo convolution (flag CONV_HALO_SMALL: at any size), the 256x128 / 256x256
# implicit GEMMs (kernel selections 4 / 5 with CONV_IMPLICIT_GEMM), or the separate pass (flag VAE_SEPARATE_STATS); H = W the output size, n >= 2 so that slabs cross image boundaries
CONV_CASES = [
    ("halo", hip.DBG_CONV_HALO_SMALL << 4, 2, 32, 128, 128, False, False),
    ("halo", hip.DBG_CONV_HALO_SMALL << 4, 3, 32, 256, 256, True, True),
    ("halo", hip.DBG_CONV_HALO_SMALL << 4, 2, 16, 128, 512, False, True),
    ("gemm256x128", 4 | (hip.DBG_CONV_IMPLICIT_GEMM << 4), 2, 32, 128, 128, True, True),
    ("gemm256x128", 4 | (hip.DBG_CONV_IMPLICIT_GEMM << 4), 3, 16, 256, 256, False, False),
    ("gemm256x256", 5 | (hip.DBG_CONV_IMPLICIT_GEMM << 4), 2, 16, 128, 512, True, False),
    ("gemm256x256", 5 | (hip.DBG_CONV_IMPLICIT_GEMM << 4), 2, 32, 128, 256, False, True),
    ("separate", hip.DBG_VAE_SEPARATE_STATS << 4, 2, 32, 128, 256, False, True),
    ("separate", hip.DBG_VAE_SEPARATE_STATS << 4, 3, 32, 128, 128, True, False),
]


@pytest.mark.parametrize("fam", FAMILIES)
@pytest.mark.parametrize("case", CONV_CASES, ids=[f"{c[0]}-n{c[2]}-{c[3]}px-{c[4]}to{c[5]}{'-ups' if c[6] else ''}{'-resid' if c[7] else ''}" for c in CONV_CASES])
def test_vae_conv3x3_gn_vs_fp64(case, fam):
    from lfm_amd import hip

    src, sel, n, H, Cin, Cout, ups, resid_on = case
    dev = torch.device("cuda:0")
    L = hip.lib()
    g = torch.Generator().manual_seed(n * 100 + H + Cout)
    bias, scale, family_resid = conv_family(fam, Cout, n + Cout)
    Hs = H >> int(ups)
    x = torch.randn(n, Hs, Hs, Cin, generator=g).half().to(dev)
    w = (torch.randn(Cout, 9 * Cin, generator=g) * (scale / (9 * Cin) ** 0.5)).half().to(dev)
    resid = (torch.randn(n, H, H, Cout, generator=g) * 0.5 if family_resid else torch.zeros(n, H, H, Cout)).half().to(dev) if resid_on else None
    bias = bias.float().to(dev)
    gamma, beta, _ = affine(Cout, Cout, dev)
    HW = H * H
    pairs = n * max(2 * (HW // 256) * Cout // 4, 64 * Cout // 4)
    ws = torch.empty(256 + (n * 256 + 255) // 256 * 256 + pairs * 8, dtype=torch.uint8, device=dev)

    def run():
        co = torch.empty(n, HW, Cout, dtype=torch.float16, device=dev)
        y = torch.empty_like(co)
        slabs, kern = C.c_int(-1), C.c_int(-1)
        hip.check(L.lfm_vae_conv3x3_gn_f16(hip.ptr(x), hip.ptr(w), hip.ptr(bias), hip.ptr(resid), hip.ptr(co), hip.ptr(y), hip.ptr(gamma), hip.ptr(beta),
                                           hip.ptr(ws), ws.numel(), n, H, H, Cin, Cout, int(ups), 1, C.byref(slabs), C.byref(kern), hip.stream_ptr()),
                  "lfm_vae_conv3x3_gn_f16")
        torch.cuda.synchronize()
        return co, y, slabs.value, kern.value

    co, y, slabs, kern = with_flags(sel, run)
    # the statistics source this case is about really ran
    assert (slabs, kern) == {"halo": (2 * HW // 256, 1), "gemm256x128": (2 * HW // 256, 2), "gemm256x256": (2 * HW // 256, 2), "separate": (0, 0)}[src]
    co2, y2, _, _ = with_flags(sel, run)
    assert torch.equal(co, co2) and torch.equal(y, y2)
    if fam == "centred":  # the convolution itself (the statistics are what this test is about; the kernels' own parity tests live elsewhere)
        xs = x.permute(0, 3, 1, 2).double()
        if ups:
            xs = F.interpolate(xs, scale_factor=2, mode="nearest")
        cref = F.conv2d(xs, w.double().reshape(Cout, 3, 3, Cin).permute(0, 3, 1, 2), bias.double(), padding=1).permute(0, 2, 3, 1)
        if resid is not None:
            cref = cref + resid.double()
        assert float((co.double().reshape(cref.shape) - cref).norm() / cref.norm()) < 1e-3
    check(y, reference(co, G, gamma, beta, 1e-6, True), f"{src} / {fam}")
    if fam == "constant":
        assert float((y.double() - F.silu(beta.double())).abs().max()) <= 2.0 ** -10 * max(1.0, float(F.silu(beta.double()).abs().max()))
