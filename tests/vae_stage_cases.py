"""Cases and float64 references of the VAE stage tests (tests/test_vae_stage_ref.py on the CPU, tests/test_gpu_vae_stages.py on the GPU): conv_in
(post_quant_conv folded in), the encoder's asymmetric downsample, a run of resnets, and the encoder's conv_out to the moments.

Not a test module.  The integer builders, the guarded layouts and the checker are those of tests/gemm_exact_cases.py.

Two families per stage.
  exact: integer-valued operands; every product and partial sum is an integer below 2^24, so fp32 arithmetic returns the integer result in ANY order, and
         an fp16 output of magnitude <= 2048 holds it exactly.  Checked by equality (gc.assert_exact).  The two caps are conditions of that argument:
         every builder asserts them.
  gauss: fp16-rounded Gaussian operands against float64 with a DERIVED per-element bound (conv_in_gauss, conv_gauss: the derivations).
The resnet has no exact family (GroupNorm is not integer arithmetic) and no per-element bound (fp16 stores between its five operations): its bound is the
error of the float64 model with those stores rounded (resnet_case)."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import gemm_exact_cases as gc

F64 = torch.float64
CIN_OUT = 512  # decoder.conv_in output channels


def rel_l2(a, b):
    return float((a.double() - b.double()).norm() / b.double().norm())


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


def half_randn(g, shape, scale):
    """Gaussian values rounded to fp16 (the product of two of them is exact in fp32: 11 x 11 significand bits), as float64."""
    return (torch.randn(shape, generator=g) * scale).half().double()


# ------------------------------------------------------------------------------------------------ conv_in (post_quant_conv 1x1 + conv_in 3x3)
# (n, R): all-border and mostly-border images, 75 pixels in ragged blocks of 16; the 64-pixel policy begins at 16384 pixels (16641 leaves a one-pixel last
# block), the 256-pixel policy at 65536 (66049 likewise)
CONV_IN_SHAPES = [(1, 1), (1, 2), (3, 5), (2, 8), (1, 128), (1, 129), (1, 256), (1, 257)]
CONV_IN_GAUSS_SHAPES = [(1, 1), (1, 2), (3, 5), (2, 8), (1, 129)]


def conv_in_ref(z, pq_w, pq_b, cin_w, cin_b, bias_in_padding=False):
    """float64: conv_in(pad_0(post_quant_conv(z))) as NHWC rows [n R R, Cout], as AutoencoderKL.decode applies the two.  bias_in_padding (a CONTROL, the
    mistake the kernel's per-tap skip avoids): the 1x1 evaluated on the zero-padded z, so the padding holds pq_b instead of 0."""
    n, _, R, _ = z.shape
    pq = F.conv2d(F.pad(z.double(), (1, 1, 1, 1)), pq_w.double().reshape(4, 4, 1, 1), pq_b.double())
    if not bias_in_padding:
        inside = torch.zeros(1, 1, R + 2, R + 2, dtype=F64)
        inside[..., 1:-1, 1:-1] = 1
        pq = pq * inside
    out = F.conv2d(pq, cin_w.double(), cin_b.double())
    return out.permute(0, 2, 3, 1).reshape(n * R * R, -1)


def conv_in_exact(n, R):
    """z, pq_b in [-2, 2], pq_w, cin_w in [-1, 1], cin_b in [-8, 8]: |post-quant| <= 10, |out| <= 36 x 10 + 8 = 368.  Not cached (the 257^2 reference is large)."""
    g = torch.Generator().manual_seed(101 + 7 * n + R)
    z, pq_w, pq_b = gc.randint(g, (n, 4, R, R), 2), gc.randint(g, (4, 4), 1), gc.randint(g, (4,), 2)
    cin_w, cin_b = gc.randint(g, (CIN_OUT, 4, 3, 3), 1), gc.randint(g, (CIN_OUT,), 8)
    ref = conv_in_ref(z, pq_w, pq_b, cin_w, cin_b)
    mag = conv_in_ref(z.abs(), pq_w.abs(), pq_b.abs(), cin_w.abs(), cin_b.abs())  # every sum of absolute terms; the padding stays 0
    assert float(mag.max()) < gc.CAP32 and float(ref.abs().max()) <= gc.CAP16, (n, R, float(mag.max()), float(ref.abs().max()))
    assert bool((ref == ref.round()).all())
    return SimpleNamespace(n=n, R=R, M=n * R * R, z=z, pq_w=pq_w, pq_b=pq_b, cin_w=cin_w, cin_b=cin_b, ref=ref)


@functools.lru_cache(maxsize=None)
def conv_in_gauss(n, R):
    """Operands: fp16-rounded Gaussians held in fp32.  Bound per element
        |got - ref| <= (T + 2) 2^-23 S + 2^-11 |ref|,   T = 41,
    S = |cin_b| + sum over the taps inside the image and the 4 channels of |w| (|pq_b| + sum_c |pq_w| |z|), the float64 sum of the absolute value of every
    term.  Derivation: a post-quant value is 4 exact products (fp16-rounded factors) and 4 additions, each addition rounding by at most 2^-24 relative to
    a partial sum that its absolute sum bounds; it enters the output through |w|, so these cost 4 x 2^-24 S.  The 36 taps are 36 products of a full fp32
    value (one rounding each) and 36 additions: 72 x 2^-24 S when not contracted to FMAs, 36 when contracted.  76 x 2^-24 <= (41 + 2) 2^-23 = 86 x 2^-24
    leaves the rest to the second-order terms; 2^-11 |ref| is the one rounding of the fp16 store."""
    g = torch.Generator().manual_seed(211 + 7 * n + R)
    z, pq_w, pq_b = half_randn(g, (n, 4, R, R), 1.0), half_randn(g, (4, 4), 0.5), half_randn(g, (4,), 0.1)
    cin_w, cin_b = half_randn(g, (CIN_OUT, 4, 3, 3), 1 / 6.0), half_randn(g, (CIN_OUT,), 0.1)
    ref = conv_in_ref(z, pq_w, pq_b, cin_w, cin_b)
    S = conv_in_ref(z.abs(), pq_w.abs(), pq_b.abs(), cin_w.abs(), cin_b.abs())
    bound = (41 + 2) * 2.0 ** -23 * S + 2.0 ** -11 * ref.abs()
    return SimpleNamespace(n=n, R=R, M=n * R * R, z=z, pq_w=pq_w, pq_b=pq_b, cin_w=cin_w, cin_b=cin_b, ref=ref, bound=bound)


def border_rows(n, R):
    """Rows of the [n R R, C] output whose pixel touches the image border."""
    y, x = torch.meshgrid(torch.arange(R), torch.arange(R), indexing="ij")
    edge = ((y == 0) | (y == R - 1) | (x == 0) | (x == R - 1)).reshape(-1)
    return edge.repeat(n)


# ------------------------------------------------------------------------------------------------ 3x3 convolutions as im2col products
def conv_gauss(N, H, W, Cin, Cout, mode, out16, seed):
    """x ~ N(0, 1/4), w ~ N(0, 1 / K), both fp16; bias fp32 ~ N(0, 0.01).  Bound per element, the construction of gc.gauss_case with K = 9 Cin:
        |got - ref| <= (9 Cin + 2) 2^-23 S      (+ 2^-11 |ref| for an fp16 output),    S = (|cols| |w|^T + |bias|)[m, n]
    (the 9 Cin products are exact in fp32; each of the 9 Cin additions, the bias add included, rounds by at most 2^-24 relative to a partial sum that S
    bounds, in any order; the factor 2 of 2^-23 and the + 2 leave room for the second-order terms)."""
    g = torch.Generator().manual_seed(seed)
    Hi, Wi = gc.conv_input_size(H, W, mode)
    K = 9 * Cin
    x, w = half_randn(g, (N * Hi * Wi, Cin), 0.5), half_randn(g, (Cout, K), K ** -0.5)
    bias = (torch.randn(Cout, generator=g) * 0.1).double()
    cols = gc.conv_cols(x, N, H, W, Cin, mode)
    ref = cols @ w.t() + bias
    bound = (K + 2) * 2.0 ** -23 * (cols.abs() @ w.abs().t() + bias.abs())
    if out16:
        bound = bound + 2.0 ** -11 * ref.abs()
    return SimpleNamespace(N=N, H=H, W=W, Cin=Cin, Cout=Cout, M=N * H * W, mode=mode, x=x, Wt=w, bias=bias, ref=ref, bound=bound)


# ------------------------------------------------------------------------------------------------ downsample (ASrcConv mode 3)
# (n, Ho, Wo, C): one, two and more 128- / 256-row tiles, all ragged in M (30, 64, 48, 384 rows); every channel count of the encoder's downsamplers and 64
DOWN_SHAPES = [(2, 3, 5, 64), (1, 8, 8, 128), (3, 4, 4, 512), (1, 16, 24, 256)]
DOWN_SELECT = (0, 1, 4, 5)  # lfm_gemm_select: auto, 128x128, 256x128, 256x256
DOWN_GAUSS_SELECT = (0, 5)


@functools.lru_cache(maxsize=None)
def down_exact(n, Ho, Wo, C):
    g = torch.Generator().manual_seed(307 + n + 3 * Ho + 7 * Wo + C)
    x = gc.randint(g, (n * 4 * Ho * Wo, C), gc.R16["a"])
    Wt, bias = gc.randint(g, (C, 9 * C), gc.R16["w"]), gc.randint(g, (C,), gc.R16["bias"])
    ref, mag = gc.conv_ref(x, Wt, bias, None, n, Ho, Wo, C, 3)
    assert int(ref.abs().max()) <= gc.CAP16 and int(mag.max()) < gc.CAP32, (n, Ho, Wo, C, int(ref.abs().max()))
    wrong, _ = gc.conv_ref(x, Wt, bias, None, n, Ho, Wo, C, 2)  # CONTROL: stride 2 with pad 1 all round
    return SimpleNamespace(N=n, H=Ho, W=Wo, Cin=C, Cout=C, M=n * Ho * Wo, x=x, Wt=Wt, bias=bias, ref=ref, mode2=wrong)


@functools.lru_cache(maxsize=None)
def down_gauss(n, Ho, Wo, C):
    c = conv_gauss(n, Ho, Wo, C, C, 3, True, 401 + n + 3 * Ho + 7 * Wo + C)
    c.mode2 = gc.conv_cols(c.x, n, Ho, Wo, C, 2) @ c.Wt.t() + c.bias  # CONTROL
    return c


def last_row_col(n, Ho, Wo):
    """(rows of the last output row, rows of the last output column) as boolean masks over the n Ho Wo output rows."""
    y, x = torch.meshgrid(torch.arange(Ho), torch.arange(Wo), indexing="ij")
    return (y == Ho - 1).reshape(-1).repeat(n), (x == Wo - 1).reshape(-1).repeat(n)


# ------------------------------------------------------------------------------------------------ moments (encoder conv_out, N = 8, fp32 NCHW)
MOMENTS_SHAPES = [(3, 5, 5), (2, 8, 8), (1, 24, 24)]  # M = 75: one 128-row tile over three 25-pixel planes; 128: exactly one tile over two; 576: ragged fifth tile


def to_nchw_rows(t, n, HW):
    """[n HW, 8] -> [n 8, HW]: the rows of the NCHW moments."""
    return t.reshape(n, HW, 8).permute(0, 2, 1).reshape(n * 8, HW).contiguous()


@functools.lru_cache(maxsize=None)
def moments_exact(n, H, W):
    """gc.R32 ranges (a, w in [-8, 8], bias in [-64, 64]): sum |a w| <= 4608 x 64 < 2^24, and outputs beyond 2048 -- a hand-over through fp16 fails exactly."""
    g = torch.Generator().manual_seed(503 + n + 3 * H + 7 * W)
    x = gc.randint(g, (n * H * W, 512), gc.R32["a"])
    Wt, bias = gc.randint(g, (8, 9 * 512), gc.R32["w"]), gc.randint(g, (8,), gc.R32["bias"])
    ref, mag = gc.conv_ref(x, Wt, bias, None, n, H, W, 512, 0)
    assert int(mag.max()) < gc.CAP32 and int(ref.abs().max()) < gc.CAP32
    assert int((ref.abs() > gc.CAP16).sum()) > ref.numel() // 10, "the case must leave the fp16-exact range"
    return SimpleNamespace(N=n, H=H, W=W, M=n * H * W, x=x, Wt=Wt, bias=bias, ref=to_nchw_rows(ref, n, H * W))


@functools.lru_cache(maxsize=None)
def moments_gauss(n, H, W):
    c = conv_gauss(n, H, W, 512, 8, 0, False, 601 + n + 3 * H + 7 * W)
    c.ref, c.bound = to_nchw_rows(c.ref, n, H * W), to_nchw_rows(c.bound, n, H * W)
    return c


# ------------------------------------------------------------------------------------------------ resnets
RESNET_WIDTHS = [(128, 128), (256, 128), (128, 256), (512, 512)]  # identity / shortcut / shortcut / identity
RESNET_MAPS = [(16, 16), (12, 12)]  # halo convolution with the statistics from its epilogue (HW % 256 == 0) / implicit GEMM with a statistics pass
RESNET_N = 2
RESNET_CHAIN = ((256, 128), (128, 128))  # the chained case, at 16 x 16
RESNET_MARGIN = 2.0
PARAM_NAMES = ("n1_g", "n1_b", "c1_w", "c1_b", "n2_g", "n2_b", "c2_w", "c2_b", "sc_w", "sc_b")


def _r16(t, rounded):
    return t.half().double() if rounded else t


def gn_silu64(x, gamma, beta, n):
    """float64 GroupNorm(32 groups, eps 1e-6, biased variance) + SiLU on NHWC rows [n HW, C]."""
    C = x.shape[1]
    v = x.reshape(n, -1, 32, C // 32)
    mean = v.mean((1, 3), keepdim=True)
    var = ((v - mean) ** 2).mean((1, 3), keepdim=True)
    y = ((v - mean) / torch.sqrt(var + 1e-6)).reshape(-1, C) * gamma + beta
    return y * torch.sigmoid(y)


def resnet64(x, p, n, H, W, rounded=False, drop_sc_bias=False, identity_skip=False):
    """float64 ResnetBlock2D on NHWC rows.  rounded: every tensor the device stores as fp16 -- GN1 out, conv1 out, GN2 out, shortcut out, the result --
    is rounded to fp16 at that point (the error of an ideal implementation).  drop_sc_bias / identity_skip: CONTROLS (a shortcut without its bias; the
    input itself, its channels wrapped to the output width, where a shortcut is configured)."""
    cin, cout = x.shape[1], p["c1_w"].shape[0]
    h = _r16(gn_silu64(x, p["n1_g"], p["n1_b"], n), rounded)
    h = _r16(gc.conv_cols(h, n, H, W, cin, 0) @ p["c1_w"].t() + p["c1_b"], rounded)
    h = _r16(gn_silu64(h, p["n2_g"], p["n2_b"], n), rounded)
    skip = x
    if p["sc_w"] is not None:
        if identity_skip:
            skip = x[:, torch.arange(cout) % cin]
        else:
            skip = _r16(x @ p["sc_w"].t() + (0 if drop_sc_bias else p["sc_b"]), rounded)
    return _r16(gc.conv_cols(h, n, H, W, cout, 0) @ p["c2_w"].t() + p["c2_b"] + skip, rounded)


def resnet_params(g, cin, cout):
    """float64 values of what the device holds: fp16 convolution / shortcut weights [Cout][9][Cin], fp32 everything else."""
    def f32(shape, scale, shift=0.0):
        return (shift + scale * torch.randn(shape, generator=g)).double()

    p = dict(n1_g=f32(cin, 0.1, 1.0), n1_b=f32(cin, 0.1), c1_w=half_randn(g, (cout, 9 * cin), (9 * cin) ** -0.5), c1_b=f32(cout, 0.1),
             n2_g=f32(cout, 0.1, 1.0), n2_b=f32(cout, 0.1), c2_w=half_randn(g, (cout, 9 * cout), (9 * cout) ** -0.5), c2_b=f32(cout, 0.1),
             sc_w=None, sc_b=None)
    if cin != cout:
        p["sc_w"], p["sc_b"] = half_randn(g, (cout, cin), cin ** -0.5), f32(cout, 0.1)
    return p


@functools.lru_cache(maxsize=None)
def resnet_case(widths, H, W, n=RESNET_N):
    """widths: ((cin, cout), ...) of the resnets run in sequence.  ref64: float64 throughout on the fp16 operands; ref_r: the same with the device's fp16
    stores.  e_l2, e_max: the errors of ref_r, i.e. of an ideal implementation; the device differs from ref_r by fp32 accumulation (two orders below an
    fp16 ulp) and by the rounding flips that causes, each of the size of a rounding already counted and roughly independent of it -- at most a doubling
    of the variance, a factor sqrt(2).  The caps are RESNET_MARGIN = 2 times e_l2 and e_max."""
    g = torch.Generator().manual_seed(701 + sum(a + 3 * b for a, b in widths) + 5 * H + W)
    x = half_randn(g, (n * H * W, widths[0][0]), 1.0)
    params = [resnet_params(g, a, b) for a, b in widths]
    ref64, ref_r = x, x
    for p in params:
        ref64, ref_r = resnet64(ref64, p, n, H, W), resnet64(ref_r, p, n, H, W, rounded=True)
    return SimpleNamespace(n=n, H=H, W=W, M=n * H * W, widths=widths, x=x, params=params, ref64=ref64, ref_r=ref_r,
                           e_l2=rel_l2(ref_r, ref64), e_max=max_abs(ref_r, ref64))


def resnet_control(c, **wrong):
    """The rounded model of the whole chain with one mistake in every resnet that has a shortcut."""
    h = c.x
    for p in c.params:
        h = resnet64(h, p, c.n, c.H, c.W, rounded=True, **(wrong if p["sc_w"] is not None else {}))
    return h


def resnet_within_cap(got, c):
    """(ok, relL2 / e_l2, maxabs / e_max) of a result against the float64 model."""
    a, b = rel_l2(got, c.ref64) / c.e_l2, max_abs(got, c.ref64) / c.e_max
    return bool(torch.isfinite(got).all()) and a <= RESNET_MARGIN and b <= RESNET_MARGIN, a, b


def resnet_case_list():
    return [(((a, b),), H, W) for (a, b) in RESNET_WIDTHS for (H, W) in RESNET_MAPS] + [(RESNET_CHAIN, 16, 16)]
