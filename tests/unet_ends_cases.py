"""Cases, float64 references, emulations and derived bounds of the tests of the two fp32 ends of every UNet and of the VAE (tests/test_unet_ends_ref.py
on the CPU, tests/test_gpu_unet_ends.py on the GPU): lfm_conv3x3_in_f32 (fp32 NCHW, Cin <= 16 -> fp16 NHWC; conv_in_mfma_kernel and conv_in_kernel in
csrc/ops.hip) and lfm_conv3x3_out_f32 (fp16 NHWC -> fp32 NCHW, 1..4 channels; conv3x3_halo_out_kernel in csrc/conv_halo_kernel.h, or the implicit GEMM
with EpiNCHWF32).

Not a test module.  The integer builder, the guarded layouts and the checker are those of tests/gemm_exact_cases.py.

conv_in families
  int       integer x in [-64, 64], w in [-4, 4], bias in [-8, 8]
  x_planes  x = 2048 + d with d odd in [1, 15]: an fp16 number has spacing 2 there, so x needs BOTH planes of the hi / lo split (hi = x -+ 1, lo = +- 1).
            w in {-1, 0, 1} with sum_c w[co, c, tap] = 0 for every (co, tap): the 2048s cancel tap by tap, at border pixels too, and the result
            sum w d + bias stays below 2048, where fp16 holds every integer -- an x plane that is dropped changes the stored value
  w_planes  the mirror image: w = 2048 + d, x in {-1, 0, 1} with sum_c x[n, c, y, x] = 0 at every pixel
  gauss     x ~ 1.5 N(0, 1), w ~ N(0, 1 / (9 Cin)), bias ~ 0.1 N(0, 1), fp32 values that are NOT fp16 numbers
  small     |x|, |w| = 2^u, u uniform in [-6, -3), random sign: hi has an ulp of at most 2^-14, so EVERY lo value is an fp16 subnormal (asserted)
  tiny      |x| = 2^u, u in [-16, -13), the gauss weights, bias ~ 2^-12 N(0, 1): hi itself is subnormal or nearly so; the absolute floor of the split
            is the largest term of the bound
The three integer families are exact: every product and partial sum, of the planes too (they are integers themselves), is an integer below 2^24
(gc.CAP32, asserted), so fp32 arithmetic returns the integer result in ANY order and the output is its one RNE rounding to fp16, bit for bit
(|ref| <= 65504 asserted).

conv_in bound (the real-valued families), per element, S = |b| + sum over the taps inside the image of |w| |x| in float64:

  scalar kernel   |got - ref| <= (2 KK + 2) 2^-24 S + 2^-11 |ref| + 2^-25,    KK = 9 Cin
    a chain of KK multiply-adds that starts from the bias: a product and an addition each round by at most 2^-24 relative to a partial sum that S
    bounds (2 KK roundings; KK when contracted to FMAs), + 2 for the second-order terms.  One fp16 store: 2^-11 |ref|, or half the subnormal quantum
    2^-24 where the result lies below 2^-14.

  MFMA kernel     |got - ref| <= a 2^-24 S + F + 2^-11 |ref| + 2^-25,    a = 48 KS + 16,   KS = ceil(KK / 16)
    split     v = hi + lo + e with hi = fp16(v), lo = fp16(v - hi) (v - hi is exact in fp32): |e| <= 2^-22 |v| while lo is a normal fp16 number, and
              |e| <= 2^-25 (half the subnormal quantum) where it is not, so |e| <= 2^-22 |v| + 2^-25 always.
    products  x w - (xh wh + xh wl + xl wh) = xl wl + e_x w + x e_w - e_x e_w: |xl wl| <= 2^-22 |x w| (the dropped product), the relative parts of
              e_x w and x e_w 2^-22 |x w| each -- 3 x 2^-22 = 12 x 2^-24 per term, 12 2^-24 S in all -- and the absolute parts
                  F = 2^-25 (sum_taps |w| + sum_taps |x|)      (each operand's floor times the other operand's absolute sum over the taps inside the image).
              F assumes that the matrix cores KEEP fp16 subnormal operands, which is what the kernel's comment promises.
    sums      3 KS chained MFMAs, each adding 16 products (exact in fp32: 11 x 11 significand bits) to the accumulator that starts as the bias.  How
              often an fp16 MFMA rounds inside one instruction is not documented (the fp32 one rounds once per product), so every product added
              counts as one rounding of at most 2^-24 relative to a partial sum that S (1 + 2^-9) bounds: 48 KS roundings.
    a         48 KS + 12 + 4 (second-order terms, the rounding of 2^-11 times the error before the store).
The bounds come from this derivation alone; what the device measures against them is recorded in profiles/unet_ends_tests.txt.

conv_out: fp16 operands, w4 in the library's layout [4][9][Cin] (k = tap * Cin + ci), rows >= nch zero.  exact: integers (gc.R32 ranges), equality in fp32.
gauss: fp16-rounded Gaussians; the 9 Cin products are exact in fp32, and the 9 Cin + 1 additions (the bias) each round by at most 2^-24 relative to a
partial sum that S bounds: |got - ref| <= (9 Cin + 1) 2^-24 S, with no output rounding beyond fp32's.

One quarter (nh = 1 in conv3x3_halo_out_kernel: Cin = 32, a prologue and no double buffering) and an odd number of quarters cannot be reached: every
entry point that runs the kernel (lfm_conv3x3_out_f32, the VAE decoder's conv_out at Cin = 128) has Cin % 64 == 0, and lfm_conv3x3_out_f32 refuses
anything else.  The tests reach 2, 4 and 6 quarters."""
import functools
from types import SimpleNamespace

import torch
import torch.nn.functional as F

import gemm_exact_cases as gc

F64 = torch.float64
MIN_NORMAL16 = 2.0 ** -14
MAX16 = 65504.0
GUARD_PLANES = 2  # sentinel planes before and after the [N, nch, H, W] block of conv_out
CIN_EXACT = ("int", "x_planes", "w_planes")
CIN_REAL = ("gauss", "small", "tiny")
CIN_MISTAKES = ("x_lo_dropped", "w_lo_dropped", "lo_subnormals_flushed", "taps_transposed", "hw_exchanged", "pad_k_not_zero", "border_wraps")
COUT_MISTAKES = ("pad_channel_stored", "neighbour_image_in_halo", "quarter_dropped", "tap_major_vs_channel_major")

# (N, H, W, Cin, Cout)
CIN_MFMA_SHAPES = [
    (1, 1, 1, 4, 64),       # all border, one live lane
    (2, 1, 37, 3, 128),     # a single row; Cin 3: KK = 27, Kp = 32, five padded k
    (3, 5, 7, 9, 192),      # 105 pixels: a ragged second chunk
    (1, 33, 17, 8, 256),    # Cin 8, Cout 256
    (2, 8, 8, 16, 64),      # KK = 144 = Kp: no padded k
    (1, 260, 256, 4, 64),   # 66560 pixels = 1040 chunks on 1024 workgroups: sixteen of them walk a second chunk
]
CIN_SCALAR_SHAPES = [(2, 6, 10, 4, 96), (1, 9, 5, 16, 320)]  # widths the MFMA kernel does not take
CIN_BIG = (1, 260, 256, 4, 64)

# (N, H, W, Cin, nch)
COUT_HALO_SHAPES = [
    (3, 16, 16, 64, 3),     # one tile per image: every halo side is a border, and the images are adjacent in memory
    (2, 32, 48, 64, 1),     # 12 tiles: no XCD remap
    (1, 32, 64, 128, 4),    # 8 tiles: the remap branch
    (2, 16, 32, 192, 2),    # 6 quarters
    (1, 256, 256, 64, 3),   # 256 tiles: the production gate, no flag
]
COUT_GEMM_SHAPES = [(2, 24, 40, 64, 3), (3, 16, 16, 64, 3)]  # not 16-aligned: the halo kernel declines by itself; aligned: under CONV_IMPLICIT_GEMM
COUT_BIG = (1, 256, 256, 64, 3)


def mfma_takes(Cin, Cout):
    """csrc/ops.hip: lfm_conv3x3_in_f32 / launch_conv_in_mfma, restated (aligned operands, no flag)."""
    LD = -(-Cin * 9 // 16) * 16 + 8
    return Cout in (64, 128, 192, 256) and (2 * Cout + 128) * LD * 2 <= 160 * 1024


def f32(t):
    """float64 holding fp32 values."""
    return t.float().double()


# ------------------------------------------------------------------------------------------------ conv_in: reference
def im2col(x, border_wraps=False):
    """x [N, C, H, W] -> [N H W, C 9] with k = c * 9 + ky * 3 + kx (the MFMA kernel's k order), zero outside the image.  border_wraps (a MISTAKE): a tap
    left of column 0 reads the flat index iy * W - 1, the previous row's last pixel."""
    N, C, H, W = x.shape
    flat = torch.cat([x.reshape(N, C, H * W), x.new_zeros(N, C, 1)], 2)  # index H W: the zero
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    taps = []
    for t in range(9):
        iy, ix = yy + t // 3 - 1, xx + t % 3 - 1
        ok = (iy >= 0) & (iy < H) & (ix >= 0) & (ix < W)
        if border_wraps:
            ok = ok | ((iy >= 0) & (iy < H) & (ix == -1) & (iy * W + ix >= 0))
        idx = torch.where(ok, iy * W + ix, torch.full_like(iy, H * W)).reshape(-1)
        taps.append(flat[:, :, idx])
    return torch.stack(taps, 2).permute(0, 3, 1, 2).reshape(N * H * W, C * 9)


def conv_in_ref(x, w, b):
    """float64 conv2d (padding 1) of NCHW x as NHWC rows [N H W, Cout]."""
    out = F.conv2d(x.double(), w.double(), None if b is None else b.double(), padding=1)
    return out.permute(0, 2, 3, 1).reshape(-1, w.shape[0])


# ------------------------------------------------------------------------------------------------ conv_in: emulations
def split16(v):
    """The kernel's split of fp32 values: hi = fp16(v), lo = fp16(v - hi), as float64."""
    v32 = v.float()
    hi = v32.half()
    return hi.double(), (v32 - hi.float()).half().double()


def emulate_conv_in(x, w, b, mistake=None):
    """conv_in_mfma_kernel's arithmetic with its rounding points: fp16 hi / lo planes of the im2col rows and of the weights, k = c * 9 + tap, zero in
    [Cin 9, Kp); per 16-wide k-step the three products w_hi x_hi, w_hi x_lo, w_lo x_hi added in turn to an fp32 accumulator that starts as the bias (one
    rounding per MFMA; the 16 products inside one in float64); one fp16 store.  x [N, Cin, H, W], w [Cout, Cin, 3, 3], b [Cout], float64 holding fp32
    values; returns float64 rows [N H W, Cout].  mistake: one of CIN_MISTAKES."""
    assert mistake is None or mistake in CIN_MISTAKES, mistake
    N, Cin, H, W = x.shape
    Cout, KK = w.shape[0], Cin * 9
    KS = -(-KK // 16)
    pad = KS * 16 - KK
    if mistake == "hw_exchanged":  # the pixel index taken apart with H and W exchanged
        x = x.reshape(N, Cin, W, H)
    if mistake == "taps_transposed":
        w = w.transpose(2, 3)
    cols, wk = im2col(x, border_wraps=mistake == "border_wraps"), w.reshape(Cout, KK)
    xpad, wpad = cols.new_zeros(cols.shape[0], pad), wk.new_zeros(Cout, pad)
    if mistake == "pad_k_not_zero" and pad:
        # x: channel k / 9 >= Cin of image n is a channel of image n + 1 in memory (nothing after the last image); w: w[co * KK + k] is the next row's
        nxt = torch.cat([x[1:], torch.zeros_like(x[:1])], 0)
        xpad, wpad = im2col(nxt)[:, :pad], torch.cat([wk[1:], torch.zeros_like(wk[:1])], 0)[:, :pad]
    xh, xl = split16(torch.cat([cols, xpad], 1))
    wh, wl = split16(torch.cat([wk, wpad], 1))
    if mistake == "x_lo_dropped":
        xl = torch.zeros_like(xl)
    if mistake == "w_lo_dropped":
        wl = torch.zeros_like(wl)
    if mistake == "lo_subnormals_flushed":
        xl, wl = xl * (xl.abs() >= MIN_NORMAL16), wl * (wl.abs() >= MIN_NORMAL16)
    acc = f32(b).expand(cols.shape[0], Cout).clone()
    for s in range(KS):
        k = slice(16 * s, 16 * s + 16)
        for a, v in ((wh, xh), (wh, xl), (wl, xh)):
            acc = f32(acc + v[:, k] @ a[:, k].t())
    return acc.float().half().double()


def emulate_conv_in_scalar(x, w, b):
    """conv_in_kernel's arithmetic: an fp32 FMA chain over k = c * 9 + tap from the bias (a tap outside the image is skipped: adding an exact zero is the
    same), one fp16 store."""
    cols, wk = im2col(x), w.reshape(w.shape[0], -1)
    acc = f32(b).expand(cols.shape[0], wk.shape[0]).clone()
    for k in range(wk.shape[1]):
        acc = f32(acc + cols[:, k:k + 1] * wk[:, k])  # the product of two fp32 values is exact in float64
    return acc.float().half().double()


# ------------------------------------------------------------------------------------------------ conv_in: cases
def zero_sum_signs(g, shape):
    """{-1, 0, 1} of `shape` whose sum over dim 1 is zero everywhere: along dim 1 an independent random arrangement of +1, -1, +1, -1, ... (, 0)."""
    C = shape[1]
    pattern = torch.tensor([1, -1] * (C // 2) + [0] * (C % 2), dtype=torch.int64)
    order = torch.rand(shape, generator=g).argsort(1)
    return pattern[order]


def odd_above_2048(g, shape):
    return 2049 + 2 * torch.randint(0, 8, shape, generator=g, dtype=torch.int64)


def log_uniform(g, shape, lo, hi):
    """+- 2^u, u uniform in [lo, hi), as fp32 values clamped into [2^lo, 2^hi]."""
    mag = torch.exp2(lo + (hi - lo) * torch.rand(shape, generator=g, dtype=F64)).clamp(2.0 ** lo, 2.0 ** hi)
    sign = torch.randint(0, 2, shape, generator=g, dtype=torch.int64) * 2 - 1
    return f32(mag * sign).clamp(-2.0 ** hi, 2.0 ** hi)


def conv_in_bound(c, kernel):
    """The per-element bound of a real-valued case for `kernel` ("mfma" or "scalar"): the module docstring."""
    KK = 9 * c.Cin
    store = 2.0 ** -11 * c.ref.abs() + 2.0 ** -25
    if kernel == "scalar":
        return (2 * KK + 2) * 2.0 ** -24 * c.S + store
    a = 48 * -(-KK // 16) + 16
    return a * 2.0 ** -24 * c.S + c.F + store


@functools.lru_cache(maxsize=None)
def conv_in_case(family, N, H, W, Cin, Cout):
    """x [N, Cin, H, W], w [Cout, Cin, 3, 3], b [Cout] as float64 holding fp32 values; ref float64 rows [N H W, Cout]; S; exact families: ref16, the RNE
    rounding of the integer ref to fp16; real-valued families: F, the floor of the split."""
    g = torch.Generator().manual_seed(sum(map(ord, family)) + 1009 * N + 31 * H + 7 * W + 3 * Cin + Cout)
    xs, ws = (N, Cin, H, W), (Cout, Cin, 3, 3)
    if family == "int":
        x, w, b = gc.randint(g, xs, 64), gc.randint(g, ws, 4), gc.randint(g, (Cout,), 8)
    elif family == "x_planes":
        x, b = odd_above_2048(g, xs), gc.randint(g, (Cout,), 8)
        w = zero_sum_signs(g, (Cout, Cin, 9)).reshape(ws)
    elif family == "w_planes":
        w, b = odd_above_2048(g, ws), gc.randint(g, (Cout,), 8)
        x = zero_sum_signs(g, (N, Cin, H * W)).reshape(xs)
    elif family == "gauss":
        x, w, b = torch.randn(xs, generator=g) * 1.5, torch.randn(ws, generator=g) / (9 * Cin) ** 0.5, torch.randn(Cout, generator=g) * 0.1
    elif family == "small":
        x, w, b = log_uniform(g, xs, -6, -3), log_uniform(g, ws, -6, -3), torch.randn(Cout, generator=g) * 0.01
    elif family == "tiny":
        x, w = log_uniform(g, xs, -16, -13), torch.randn(ws, generator=g) / (9 * Cin) ** 0.5
        b = torch.randn(Cout, generator=g) * 2.0 ** -12
    else:
        raise ValueError(family)
    x, w, b = f32(x), f32(w), f32(b)
    c = SimpleNamespace(family=family, N=N, H=H, W=W, Cin=Cin, Cout=Cout, M=N * H * W, x=x, w=w, b=b, exact=family in CIN_EXACT)
    c.ref = conv_in_ref(x, w, b)
    c.S = conv_in_ref(x.abs(), w.abs(), b.abs())
    if c.exact:
        assert float(c.S.max()) < gc.CAP32 and float(c.ref.abs().max()) <= MAX16, (family, N, H, W, Cin, Cout, float(c.S.max()), float(c.ref.abs().max()))
        assert bool((c.ref == c.ref.round()).all())
        c.ref16 = c.ref.float().half().double()
        if family != "int":  # the hi planes cancel: every result is an integer that fp16 holds, so one unit of a lo plane shows
            assert float(c.ref.abs().max()) <= gc.CAP16 and bool((c.ref16 == c.ref).all())
            planes = x if family == "x_planes" else w
            assert bool((split16(planes)[1].abs() == 1).all())
    else:
        c.F = 2.0 ** -25 * (conv_in_ref(torch.ones_like(x), w.abs(), None) + conv_in_ref(x.abs(), torch.ones_like(w), None))
        if family == "small":
            for t in (x, w):
                assert float(t.abs().min()) >= 2.0 ** -6 and float(t.abs().max()) <= 2.0 ** -3
                lo = split16(t)[1]
                assert float(lo.abs().max()) < MIN_NORMAL16 and float((lo != 0).double().mean()) > 0.9  # every lo value is an fp16 subnormal (or zero)
        if family == "tiny":
            assert float(x.abs().min()) >= 2.0 ** -16 and float(x.abs().max()) <= 2.0 ** -13
    return c


def compare(got, ref, bound=None):
    """got (fp16 or fp32) against ref (float64, the same shape): SimpleNamespace(bad, worst, exact_share, first).  bound None: equality (a NaN differs);
    else |got - ref| <= bound (a NaN fails), worst = the largest error / bound.  exact_share: the share of elements that hold the correctly rounded
    result, ref rounded once to got's type."""
    best = ref.to(got.dtype).double()
    got = got.double()
    exact_share = float((got == best).double().mean())
    if bound is None:
        bad = got != ref
        worst = float("inf") if bool(bad.any()) else 0.0
    else:
        ratio = (got - ref).abs() / bound
        bad = ~(ratio <= 1)
        worst = float(ratio.nan_to_num(nan=float("inf")).max())
    first = [(pos, float(got[tuple(pos)]), float(ref[tuple(pos)])) for pos in bad.nonzero()[:4].tolist()]
    return SimpleNamespace(bad=int(bad.sum()), worst=worst, exact_share=exact_share, first=first)


# ------------------------------------------------------------------------------------------------ conv_out
def pack_w4(w):
    """[nch, Cin, 3, 3] -> the library's [4][9][Cin] (k = tap * Cin + ci), rows >= nch zero."""
    nch, Cin = w.shape[:2]
    w4 = w.new_zeros(4, 9 * Cin)
    w4[:nch] = w.permute(0, 2, 3, 1).reshape(nch, 9 * Cin)
    return w4


def conv_out_ref(x, w, b, N, H, W):
    """float64 conv2d of NHWC rows x [N H W, Cin] with w [nch, Cin, 3, 3], as NCHW planes [N nch, H W]."""
    xi = x.double().reshape(N, H, W, -1).permute(0, 3, 1, 2)
    return F.conv2d(xi, w.double(), b.double(), padding=1).reshape(N * w.shape[0], H * W)


def planes_buffer(N, nch, HW, dtype=torch.float32):
    """[GUARD_PLANES + N nch + GUARD_PLANES, H W] of the sentinel: the NCHW output block between guard planes."""
    return torch.full((2 * GUARD_PLANES + N * nch, HW), gc.SENTINEL, dtype=dtype)


def touched_planes(buf, rows):
    """Positions of the guard planes of a planes_buffer (rows: N nch) that no longer hold the sentinel, as (plane relative to the block, pixel)."""
    rolled = torch.cat([buf[GUARD_PLANES:], buf[:GUARD_PLANES]])  # the block first: gc.touched_positions looks after it
    return [(m if m < rows + GUARD_PLANES else m - rolled.shape[0], n) for m, n in gc.touched_positions(rolled, rows, buf.shape[1])]


def emulate_conv_out(x, w4, b4, N, H, W, nch, mistake=None):
    """The output convolution in fp32 (torch's fp32 conv2d with all four rows of w4 read as [4][9][Cin], + bias) scattered to NCHW planes inside a
    planes_buffer.  x [N H W, Cin], w4 [4, 9 Cin], b4 [4] float64 holding fp16 / fp16 / fp32 values.  mistake: one of COUT_MISTAKES."""
    assert mistake is None or mistake in COUT_MISTAKES, mistake
    Cin, HW = x.shape[1], H * W
    if mistake == "quarter_dropped":  # the last 32-channel quarter not accumulated
        x = torch.cat([x[:, :Cin - 32], torch.zeros_like(x[:, Cin - 32:])], 1)
    if mistake == "tap_major_vs_channel_major":  # the weight of (tap, ci) looked up at k = ci * 9 + tap
        w4 = w4.reshape(4, Cin, 9).permute(0, 2, 1).reshape(4, 9 * Cin)
    # neighbour_image_in_halo: the images stacked into one tall map -- an image's top / bottom halo row is then its neighbour's row, not zeros
    xi = x.reshape(1, N * H, W, Cin) if mistake == "neighbour_image_in_halo" else x.reshape(N, H, W, Cin)
    acc = F.conv2d(xi.permute(0, 3, 1, 2).float(), w4.reshape(4, 3, 3, Cin).permute(0, 3, 1, 2).float(), b4.float(), padding=1)
    acc = acc.permute(0, 2, 3, 1).reshape(N, HW, 4)
    buf = planes_buffer(N, nch, HW)
    for img in range(N):  # in ascending order: what image i spills into image i + 1's plane 0 is overwritten, only the last spill survives (the hardest case)
        for ch in range(nch + (mistake == "pad_channel_stored")):
            buf[GUARD_PLANES + img * nch + ch] = acc[img, :, ch]
    return buf


@functools.lru_cache(maxsize=None)
def conv_out_case(family, N, H, W, Cin, nch):
    """x [N H W, Cin] and w [nch, Cin, 3, 3] float64 holding fp16 values, b [nch] fp32 values; w4 [4, 9 Cin], b4 [4] (pads zero); ref float64 planes
    [N nch, H W]; gauss: bound."""
    g = torch.Generator().manual_seed(sum(map(ord, family)) + 811 * N + 31 * H + 7 * W + 3 * Cin + nch)
    if family == "int":
        r = gc.R32
        x, w, b = gc.randint(g, (N * H * W, Cin), r["a"]).double(), gc.randint(g, (nch, Cin, 3, 3), r["w"]).double(), gc.randint(g, (nch,), r["bias"]).double()
    elif family == "gauss":
        x = torch.randn(N * H * W, Cin, generator=g).half().double()
        w = (torch.randn(nch, Cin, 3, 3, generator=g) / (9 * Cin) ** 0.5).half().double()
        b = f32(torch.randn(nch, generator=g) * 0.1)
    else:
        raise ValueError(family)
    c = SimpleNamespace(family=family, N=N, H=H, W=W, Cin=Cin, nch=nch, HW=H * W, x=x, w=w, b=b, w4=pack_w4(w), exact=family == "int")
    c.b4 = torch.cat([b, b.new_zeros(4 - nch)])
    c.ref = conv_out_ref(x, w, b, N, H, W)
    c.S = conv_out_ref(x.abs(), w.abs(), b.abs(), N, H, W)
    if c.exact:
        assert float(c.S.max()) < gc.CAP32 and bool((c.ref == c.ref.round()).all())
        c.bound = None
    else:
        c.bound = (9 * Cin + 1) * 2.0 ** -24 * c.S
    return c
