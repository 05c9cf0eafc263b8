"""Cases, an fp32 emulation and the derived error bound for lfm_ssim_u8 / lfm_ssim_f32 (include/lfm_hip.h, csrc/ssim.h), shared by tests/test_ssim_ref.py
(CPU), tests/test_gpu_ssim.py, tests/test_gpu_inpaint_eval.py and tools/make_ssim_golden.py.  Pure numpy: nothing here needs a GPU or the reference.

The yardstick of every accuracy check is the UNMODIFIED reference (datasets_prep/inpaint_preprocess/losses/ssim.py, SSIM(size_average=False)) run in fp64 on
the same inputs, stored in tests/golden/ssim.pt by tools/make_ssim_golden.py; for bytes the fp64 input is the exact quotient b / 255 rounded to fp64.

The bound (`bound`), per image, u = 2^-24, gamma(n) = n u / (1 - n u), from the kernel's stated operation order (the header of csrc/ssim.h):
  inputs      a byte's value is the correctly rounded quotient: x^ = x (1 + d), |d| <= u.  The products x*x, y*y, x*y of rounded inputs, rounded once
              more: relative error within gamma(3).  (fp32 inputs carry no input error; the bound keeps the term, it is an upper bound either way.)
  window      the reference's 2-D window is fl(w[j] * w[k]), the kernel applies w[j] and w[k] one after the other: relative u per tap.  One more u per
              tap for the normalising fp32 sum, whose order of addition is torch's choice on the machine that builds the window.
  passes      horizontal then vertical, window_size FMAs each from an accumulator of 0: 2 * window_size rounded operations per quantity, every term of one
              sign bounded by the window applied to |q|: relative gamma(2 * window_size) of G(|q|), G the reference's 2-D window in fp64.
              => e_mu = gamma(2 ws + 3) G(|x|)           for mu1, mu2
                 e_q  = gamma(2 ws + 5) G(|q|)           for E11 = G(x x), E22, E12
  products    m11 = fl(mu1 mu1): e_m11 = 2 |mu1| e_mu1 + e_mu1^2 + u (|mu1| + e_mu1)^2; m22 alike; e_m12 = |mu1| e_mu2 + |mu2| e_mu1 + e_mu1 e_mu2 + u (..)(..)
  subtraction s11 = fl(E11^ - m11^): e_s11 = (e_E11 + e_m11) (1 + u) + u |s11|; s22, s12 alike
  map         A1 = 2 m12 + C1 (the doubling is exact; one rounded sum; C1 as fp32 is within u C1 of the reference's Python float):
                 e_A1 = 2 e_m12 + u (|A1| + 2 e_m12) + u C1;    e_A2 = 2 e_s12 + u (|A2| + 2 e_s12) + u C2
              B1 = (m11 + m22) + C1, two rounded sums:  e_B1 = (e_m11 + e_m22) + u (m11 + m22 + e_m11 + e_m22) + u (B1 + ..) + u C1;  B2 alike with s
              S = A1 A2 / (B1 B2), three more roundings (two products, the IEEE division): relative gamma(3).
              Through the partial derivatives dS/dA1 = A2 / (B1 B2), dS/dA2 = A1 / (B1 B2), dS/dB1 = -S / B1, dS/dB2 = -S / B2, with the perturbed
              denominators bounded below by B (1 - rho), rho = e_B1 / B1 + e_B2 / B2 (asserted < 1/2):
                 e_S = [ (|A2| e_A1 + |A1| e_A2 + e_A1 e_A2) / (B1 B2) + |S| rho ] / (1 - rho) + gamma(3) (|S| + that)
  tile sum    a lane adds at most 4 C values, six butterfly levels and three LDS adds follow: every value passes at most 4 C + 9 fp32 additions:
                 gamma(4 C + 9) * mean(|S| + e_S)
  final       the fp64 sum of the tile partials, the division by C H W and the one rounding to fp32: four fp32 ulps of 1.0 (4 * 2^-23) cover it.
  bound = mean over pixels and channels of e_S  +  the tile-sum term  +  4 * 2^-23.
On flat bright inputs (constants 200 against 201) E11 - mu1^2 cancels against C2 = 9e-4: the bound is 3e-5 (5 x 7) to 9e-3 (64 x 64) there, where the
reference's own fp32 run is up to 2.6e-4 off its fp64 run; on random bytes it is 0.8e-5 to 1.7e-5 (the reference's fp32: 5e-7), black against white 5e-7.  tests/test_ssim_ref.py shows the unmodified reference's fp32 results
inside it on every case and every named mistake outside it on some case."""
import numpy as np

TILE = 32  # csrc/ssim.h: SSIM_T
U = 2.0 ** -24
C1, C2 = 0.01 ** 2, 0.03 ** 2

SHAPES = [(3, 8, 8), (1, 5, 7), (2, 13, 29), (2, 40, 72), (1, 64, 64), (1, 33, 65)]  # the last: one more than 1 x 2 tiles, so a one-row and a one-column tile
FAMILIES = ["random", "pm3", "flat", "ramp", "blackwhite", "self", "zeros"]
SMALL_WINDOW_SHAPES = [(2, 13, 29), (2, 40, 72)]  # window sizes 7 and 3 as well
F32_CASES = [(1, (2, 13, 29)), (3, (2, 40, 72)), (4, (1, 33, 65)), (4, (3, 8, 8))]  # (C, shape)


def make_u8(family, N, H, W, seed=0):
    """-> (a, b) uint8 NHWC [N,H,W,3]."""
    rng = np.random.RandomState(1000 * seed + 7 * N + 31 * H + W)
    shape = (N, H, W, 3)
    a = rng.randint(0, 256, shape).astype(np.uint8)
    if family == "random":
        b = rng.randint(0, 256, shape).astype(np.uint8)
    elif family == "pm3":
        b = np.clip(a.astype(np.int32) + rng.randint(-3, 4, shape), 0, 255).astype(np.uint8)
    elif family == "flat":
        a, b = np.full(shape, 200, np.uint8), np.full(shape, 201, np.uint8)
    elif family == "ramp":
        y, x, c = np.meshgrid(np.arange(H), np.arange(W), np.arange(3), indexing="ij")
        a = np.broadcast_to((20 + (x + y + 10 * c) * 200 // (H + W + 20)).astype(np.uint8), shape).copy()
        b = (a + 1).astype(np.uint8)
    elif family == "blackwhite":
        a, b = np.zeros(shape, np.uint8), np.full(shape, 255, np.uint8)
    elif family == "self":
        b = a.copy()
    elif family == "zeros":
        a, b = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    else:
        raise ValueError(family)
    return a, b


def make_f32(C, N, H, W, seed=0):
    """-> (a, b) fp32 NCHW [N,C,H,W] in [0, 1]: b is a plus a small seeded perturbation, clipped."""
    rng = np.random.RandomState(5000 + 1000 * seed + 7 * N + 31 * H + W + C)
    a = rng.rand(N, C, H, W).astype(np.float32)
    b = np.clip(a + (rng.rand(N, C, H, W).astype(np.float32) - np.float32(0.5)) * np.float32(0.1), 0, 1).astype(np.float32)
    return a, b


def u8_cases():
    """[(name, family, (N, H, W), window_size)]"""
    out = [(f"{f}-{N}x{H}x{W}-w11", f, (N, H, W), 11) for (N, H, W) in SHAPES for f in FAMILIES]
    out += [(f"{f}-{N}x{H}x{W}-w{ws}", f, (N, H, W), ws) for (N, H, W) in SMALL_WINDOW_SHAPES for ws in (7, 3) for f in ("random", "pm3", "flat")]
    return out


def f32_cases():
    """[(name, C, (N, H, W), window_size)]"""
    return [(f"f32-c{C}-{N}x{H}x{W}-w{ws}", C, (N, H, W), ws) for (C, (N, H, W)) in F32_CASES for ws in ((11, 7) if C == 3 else (11,))]


def unit32(u8_nhwc):
    """bytes NHWC -> fp32 NCHW, each the correctly rounded b / 255 (numpy's fp32 division is IEEE): inp_unit of csrc/inpaint.h."""
    return np.ascontiguousarray((np.transpose(u8_nhwc, (0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)).astype(np.float32))


def unit64(u8_nhwc):
    return np.ascontiguousarray(np.transpose(u8_nhwc, (0, 3, 1, 2)).astype(np.float64) / 255.0)


def gaussian32(window_size, sigma=1.5, normalise=True):
    """losses/ssim.py:36-40 restated: a float64 exp per tap, ``torch.Tensor`` (fp32), divided by its fp32 sum as torch adds it (not in tap order: a sequential
    fp32 sum differs in the last place at window_size 11).  tests/test_ssim_ref.py pins this and lfm_amd.hip.ssim_gaussian to the window stored from the
    reference.  -> fp32 numpy [window_size]"""
    import torch

    g = torch.Tensor([np.exp(-((x - (window_size // 2)) ** 2) / float(2 * sigma ** 2)) for x in range(window_size)])
    return (g / g.sum() if normalise else g).numpy()


def _fma32(a, b, c):
    """fmaf on fp32 arrays: the product of two fp32 values is exact in fp64; the sum is rounded to fp64 and then to fp32 (a double rounding differs from the
    true FMA only where the fp64 sum lands on an fp32 tie, which moves a result by one ulp and is far inside the bound)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def _pad(x, r, mode="zero"):
    if mode == "reflect":
        return np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)), mode="reflect")
    return np.pad(x, ((0, 0), (0, 0), (r, r), (r, r)))


def _tile_sum32(vals):
    """One image's map [C, H, W] -> the kernel's tile partials, added in its order: per lane channel-major then j, a 64-lane butterfly, ((w0 + w1) + w2) + w3."""
    Cn, H, W = vals.shape
    parts = []
    for ty in range(-(-H // TILE)):
        for tx in range(-(-W // TILE)):
            t = np.zeros((Cn, TILE, TILE), np.float32)
            blk = vals[:, ty * TILE:(ty + 1) * TILE, tx * TILE:(tx + 1) * TILE]
            t[:, :blk.shape[1], :blk.shape[2]] = blk
            acc = np.zeros((8, TILE), np.float32)
            for c in range(Cn):
                for j in range(4):
                    acc = (acc + t[c, 8 * j:8 * j + 8]).astype(np.float32)
            v = acc.reshape(4, 64)
            idx = np.arange(64)
            for o in (32, 16, 8, 4, 2, 1):
                v = (v + v[:, idx ^ o]).astype(np.float32)
            w = v[:, 0]
            parts.append(np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3]))
    return parts


MISTAKES = ["reflect", "unnormalised", "sigma1", "swap_c", "interior_mean", "no_mu_sq", "channel_mean", "over256", "short_halo"]


def emulate32(a, b, window_size=11, mistake=None, u8=None):
    """The kernel's operation order in numpy fp32 on fp32 NCHW inputs -> fp32 [N].  `mistake` applies one of MISTAKES ("over256" needs the bytes as `u8` =
    (a_u8, b_u8) NHWC)."""
    if mistake == "over256":
        a, b = ((np.transpose(t, (0, 3, 1, 2)).astype(np.float32) / np.float32(256.0)).astype(np.float32) for t in u8)
    if mistake == "channel_mean":
        a, b = a.mean(1, keepdims=True, dtype=np.float32), b.mean(1, keepdims=True, dtype=np.float32)
    N, Cn, H, W = a.shape
    r = window_size // 2
    w = gaussian32(window_size, sigma=1.0 if mistake == "sigma1" else 1.5, normalise=mistake != "unnormalised")
    c1, c2 = (np.float32(C2), np.float32(C1)) if mistake == "swap_c" else (np.float32(C1), np.float32(C2))
    pa, pb = (_pad(t, r, "reflect" if mistake == "reflect" and min(H, W) > r else "zero") for t in (a, b))
    qs = [pa, pb, (pa * pa).astype(np.float32), (pb * pb).astype(np.float32), (pa * pb).astype(np.float32)]
    v = []
    for q in qs:
        h = np.zeros((N, Cn, H + 2 * r, W), np.float32)
        if mistake == "short_halo":  # every tile's staged rows lack their last halo column: the taps that reach it read 0
            for x0 in range(0, W, TILE):
                x1 = min(x0 + TILE, W)
                p = q[..., x0:x1 + 2 * r].copy()
                if x1 + r - 1 < W:  # (a column of the image, not padding)
                    p[..., -1] = 0
                acc = np.zeros((N, Cn, H + 2 * r, x1 - x0), np.float32)
                for k in range(window_size):
                    acc = _fma32(w[k], p[..., k:k + x1 - x0], acc)
                h[..., x0:x1] = acc
        else:
            for k in range(window_size):
                h = _fma32(w[k], q[..., k:k + W], h)
        acc = np.zeros((N, Cn, H, W), np.float32)
        for k in range(window_size):
            acc = _fma32(w[k], h[..., k:k + H, :], acc)
        v.append(acc)
    f = np.float32
    m11, m22, m12 = (v[0] * v[0]).astype(f), (v[1] * v[1]).astype(f), (v[0] * v[1]).astype(f)
    if mistake == "no_mu_sq":
        s11, s22, s12 = v[2], v[3], v[4]
    else:
        s11, s22, s12 = (v[2] - m11).astype(f), (v[3] - m22).astype(f), (v[4] - m12).astype(f)
    na, nb = (f(2) * m12 + c1).astype(f), (f(2) * s12 + c2).astype(f)
    da, db = ((m11 + m22).astype(f) + c1).astype(f), ((s11 + s22).astype(f) + c2).astype(f)
    with np.errstate(invalid="ignore", divide="ignore"):
        smap = ((na * nb).astype(f) / (da * db).astype(f)).astype(f)
    if mistake == "interior_mean" and H > 2 * r and W > 2 * r:
        return smap[:, :, r:H - r, r:W - r].astype(np.float64).mean(axis=(1, 2, 3)).astype(np.float32)
    out = np.zeros(N, np.float32)
    for n in range(N):
        out[n] = np.float32(np.sum(np.array(_tile_sum32(smap[n]), np.float64)) / float(Cn * H * W))
    return out


def _conv64(q, w2):
    """The reference's depthwise conv with zero padding, in fp64, tap by tap: q [N,C,H,W] fp64, w2 [ws,ws] fp64."""
    ws = w2.shape[0]
    r = ws // 2
    N, Cn, H, W = q.shape
    p = _pad(q, r)
    out = np.zeros_like(q)
    for j in range(ws):
        for k in range(ws):
            out += w2[j, k] * p[..., j:j + H, k:k + W]
    return out


def ref64(a64, b64, window_size=11):
    """losses/ssim.py:47-67 restated in fp64 with the reference's own fp32 2-D window -> (ssim per image, the intermediates the bound starts from).  The
    stored golden is the yardstick; this restatement only supplies the bound's intermediates (test_ssim_ref.py checks it equals the golden to 1e-12)."""
    w1 = gaussian32(window_size).reshape(-1, 1)
    w2 = (w1 @ w1.T).astype(np.float32).astype(np.float64)  # _1D_window.mm(_1D_window.t()).float()
    mu1, mu2 = _conv64(a64, w2), _conv64(b64, w2)
    e11, e22, e12 = _conv64(a64 * a64, w2), _conv64(b64 * b64, w2), _conv64(a64 * b64, w2)
    s11, s22, s12 = e11 - mu1 * mu1, e22 - mu2 * mu2, e12 - mu1 * mu2
    A1, A2, B1, B2 = 2 * mu1 * mu2 + C1, 2 * s12 + C2, mu1 * mu1 + mu2 * mu2 + C1, s11 + s22 + C2
    S = A1 * A2 / (B1 * B2)
    inter = dict(mu1=mu1, mu2=mu2, s11=s11, s22=s22, s12=s12, A1=A1, A2=A2, B1=B1, B2=B2, S=S,
                 g1=_conv64(np.abs(a64), w2), g2=_conv64(np.abs(b64), w2), g12=_conv64(np.abs(a64 * b64), w2), e11=e11, e22=e22)
    return S.mean(axis=(1, 2, 3)), inter


def gamma(n):
    return n * U / (1 - n * U)


def bound(a64, b64, window_size=11):
    """The per-image error bound of the module docstring -> fp64 [N]."""
    _, i = ref64(a64, b64, window_size)
    Cn = a64.shape[1]
    ws = window_size
    mu1, mu2 = np.abs(i["mu1"]), np.abs(i["mu2"])
    e_mu1, e_mu2 = gamma(2 * ws + 3) * i["g1"], gamma(2 * ws + 3) * i["g2"]
    e_e11, e_e22, e_e12 = gamma(2 * ws + 5) * i["e11"], gamma(2 * ws + 5) * i["e22"], gamma(2 * ws + 5) * i["g12"]
    e_m11 = 2 * mu1 * e_mu1 + e_mu1 ** 2 + U * (mu1 + e_mu1) ** 2
    e_m22 = 2 * mu2 * e_mu2 + e_mu2 ** 2 + U * (mu2 + e_mu2) ** 2
    e_m12 = mu1 * e_mu2 + mu2 * e_mu1 + e_mu1 * e_mu2 + U * (mu1 + e_mu1) * (mu2 + e_mu2)
    e_s11 = (e_e11 + e_m11) * (1 + U) + U * np.abs(i["s11"])
    e_s22 = (e_e22 + e_m22) * (1 + U) + U * np.abs(i["s22"])
    e_s12 = (e_e12 + e_m12) * (1 + U) + U * np.abs(i["s12"])
    e_A1 = 2 * e_m12 + U * (np.abs(i["A1"]) + 2 * e_m12) + U * C1
    e_A2 = 2 * e_s12 + U * (np.abs(i["A2"]) + 2 * e_s12) + U * C2
    sm, es = mu1 ** 2 + mu2 ** 2, e_m11 + e_m22
    e_B1 = es + U * (sm + es) + U * (i["B1"] + es + U * (sm + es)) + U * C1
    ss, ess = np.abs(i["s11"] + i["s22"]), e_s11 + e_s22
    e_B2 = ess + U * (ss + ess) + U * (i["B2"] + ess + U * (ss + ess)) + U * C2
    rho = e_B1 / i["B1"] + e_B2 / i["B2"]
    assert float(rho.max()) < 0.5, float(rho.max())
    S = np.abs(i["S"])
    first = ((np.abs(i["A2"]) * e_A1 + np.abs(i["A1"]) * e_A2 + e_A1 * e_A2) / (i["B1"] * i["B2"]) + S * rho) / (1 - rho)
    e_S = first + gamma(3) * (S + first)
    return e_S.mean(axis=(1, 2, 3)) + gamma(4 * Cn + 9) * (S + e_S).mean(axis=(1, 2, 3)) + 4 * 2.0 ** -23


def inputs(case):
    """A case of u8_cases() or f32_cases() -> dict(kind, a, b (as the kernel takes them), a32, b32 (fp32 NCHW), a64, b64, ws)."""
    name, what, (N, H, W), ws = case
    if isinstance(what, str):
        a, b = make_u8(what, N, H, W)
        return dict(kind="u8", a=a, b=b, a32=unit32(a), b32=unit32(b), a64=unit64(a), b64=unit64(b), ws=ws)
    a, b = make_f32(what, N, H, W)
    return dict(kind="f32", a=a, b=b, a32=a, b32=b, a64=a.astype(np.float64), b64=b.astype(np.float64), ws=ws)


def all_cases():
    return u8_cases() + f32_cases()


# ------------------------------------------------------------------ the evaluator's data: pairs, masks and the area bins
EVAL_N, EVAL_S = 24, 32
# rows of hole per mask (of 32): shares 0, 1/32 .. 1.0 over seven of the ten deciles, none on a decile's edge except 0 and 1.0 (16 / 32 is left out)
EVAL_HOLE_ROWS = [0, 0, 1, 2, 5, 7, 9, 11, 13, 15, 17, 19, 20, 22, 25, 27, 29, 31, 32, 32, 3, 4, 30, 12]


def eval_pairs():
    """-> (generated, image, mask): uint8 [24,32,32,3] twice and uint8 [24,32,32] in the driver's convention (255 = keep, 0 = hole; a few grey bytes)."""
    rng = np.random.RandomState(77)
    base = rng.randint(0, 256, (EVAL_N, EVAL_S // 4, EVAL_S // 4, 3))
    image = np.repeat(np.repeat(base, 4, 1), 4, 2)
    image = np.clip(image + rng.randint(-8, 9, image.shape), 0, 255).astype(np.uint8)
    mask = np.full((EVAL_N, EVAL_S, EVAL_S), 255, np.uint8)
    for n, k in enumerate(EVAL_HOLE_ROWS):
        mask[n, :k] = 0
        if 0 < k < EVAL_S and n % 3 == 0:
            mask[n, k, :5] = 128  # grey: part hole
    noise = np.clip(image.astype(np.int32) + rng.randint(-60, 61, image.shape), 0, 255).astype(np.uint8)
    generated = np.where((mask < 255)[..., None], noise, image).astype(np.uint8)
    return generated, image, mask
