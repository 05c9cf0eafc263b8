"""Cases, float64 references, rounding-placed emulations and DERIVED per-element bounds for the LayerNorm-modulate paths of the DiT block loops (TEST
INFRASTRUCTURE ONLY; shared by tests/test_dit_ln_ref.py and tests/test_gpu_dit_ln.py).

Two operations are observed.

DIRECT  y = (x - mu) rho (1 + s) + sh -> fp16, rho = 1 / sqrt(var + 1e-6), var = mean((x - mu)^2): lfm_ln_modulate's five kernels and
        splitk_finish_resid_ln_kernel.  x is an fp32 row (exact input), s / sh fp32 modulation rows of the row's image.
FOLDED  the producer epilogue writes A' = fp16((x - c)(1 + s)) and per 256-column slot (sum x, sum (x - c)^2); the consumer turns the slots into
        mu = sum x / D, dl = mu - c, var = max(sum (x - c)^2 / D - dl^2, 0), a = rho, b = -rho dl and stores gelu(a acc + (b u + v)) -> fp16 with
        acc = A' W^T (fp32 accumulation), u = (1 + s) W^T, v = sh W^T + bias.

``*_ref`` is the operation in float64, ``*_emulate`` the same with the roundings where a CORRECT kernel has them (fp32 statistics, rsqrt, fp16 output,
fp16 A', the one-pass shifted variance) and, with ``mistake=...``, one named mistake.

The bounds.  u32 = 2^-24, u16 = 2^-11; every quantity on the right-hand sides is taken from the float64 reference, none from a device.
K = SUM_DEPTH = 32 bounds the number of fp32 additions any one addend of a row sum passes through in any of the kernels: ln_modulate_kernel at D = 1280
has 20 in-lane additions, 6 exchange steps and the division = 27; ln_modulate8 19; the finish kernel 15; a producer slot 3 in-lane + 4 DPP + 4 quarters +
5 slots = 16.  A sum of terms t_k in any such order is off by at most K u32 sum |t_k| (first order).

  mean          e_mu  = (K + 1) u32 mean|x|                                                  (the sum, the division)
  variance      d_k = fl(x_k - mu^) is off by e_mu + u32 |d_k|; since sum d_k = 0 a shift of the mean enters the TWO-PASS sum of squares only in second
                order (D e_mu^2), so var^ = var (1 + th) + e_mu^2 with |th| <= (K + 4) u32 (2 for d_k^2, the square, the division, the sum)
  rho           e_rho = sqrt((var + eps) / (max(var - e_var, 0) + eps)) - 1 + 4 u32,  e_var = (K + 4) u32 var + e_mu^2   (eps add, rsqrt to 2 ulp, slack)
  fp32 output   e_32  = |1 + s| rho (e_mu + u32 |d|) + |d rho (1 + s)| (e_rho + 3 u32) + u32 |y|   (1 + s, two products, the final add)
  DIRECT bound  e_32 + half_ulp16(|y| + e_32)                                                (one fp16 rounding; 2^-25 among the subnormals)

For a row far from 0 the first term rules: the mean of fp32 values near 3000 is only known to about K u32 3000 = 6e-3, times rho.  That is what fp32
two-pass statistics can promise, and what the bound therefore allows; constant rows (d = 0 exactly when the sums are exact) are asserted bit for bit.

FOLDED, with r = |dl| / sqrt(var):
  cen           mu^ = fl(fl(sum of slots) inv_n): e_cen = (K + 7) u32 mean|x|                (five slot additions, inv_n = fl(1 / D), the product)
  slots         |sum x - ref| <= K u32 sum |x|,  |sum (x - c)^2 - ref| <= (K + 3) u32 sum (x - c)^2     over the slot's 256 columns
  A'            fl(fl(x - c) fl(1 + s)) -> fp16: 3 u32 |A'| + half_ulp16(|A'| (1 + 3 u32))
  dl            e_dl  = e_cen + u32 |dl|
  variance      sum (x - c)^2 / D = var + dl^2 = var (1 + r^2) carries (K + 10) u32 of ITSELF, dl^2 carries 2 |dl| e_dl + e_dl^2 + 2 u32 dl^2:
                e_var = (K + 10) u32 var (1 + r^2) + 2 |dl| e_dl + e_dl^2 + 2 u32 dl^2      -- the (1 + r^2) 2^-23-like growth of the one-pass form
  rho           e_rho as above from this e_var
  accumulator   each A'_k is off by (u16 + 3 u32) |A'_k|, the fp32 accumulation of D exact products by D u32 sum |A'_k W_nk|:
                e_acc = (u16 + (D + 3) u32) S1,  S1[m, n] = sum_k |(x_k - c)(1 + s_k)| |W_nk|  >= r sigma sum_k |(1 + s_k) W_nk| - ...: the r 2^-11 term
  u, v          e_u = uv_bound(D) sum |1 + s| |W|,  e_v = uv_bound(D) (sum |sh| |W| + |bias|)     (dit_ends_cases.uv_bound, held by test_gpu_dit_ends.py)
  pre-act       e_z = rho e_acc (1 + e_rho) + |rho (acc - dl u)| e_rho + rho |u| e_dl + rho |dl| e_u + e_v + 3 u32 (|rho acc| + |rho dl u| + |v|)
                (the last term: a acc and b u are both ~ r rho sigma |u| and cancel -- the rounding of the affine's products and additions)
  activation    |gelu'| <= 1.13 everywhere;  v_exp_f32 / v_rcp_f32 and the fp32 argument z2 = 2.3022 x (1 + 0.044715 x^2): (4 + 3 |z2|) u32 |y|
  FOLDED bound  e_y = 1.13 e_z + (4 + 3 |z2|) u32 |y|,  bound = e_y + half_ulp16(|y| + e_y)

ROOM = 2: the fp32 allowances e_32 (DIRECT) and 3 u32 |A'| (A') enter their bounds DOUBLED.  Their analysis is tight at small D (a handful of elementary
roundings, each of which the emulation really commits), it is first order, and the emulation evaluates the sums in one order and the products unfused; a
kernel may do either differently.  tests/test_dit_ln_ref.py holds the correct emulation to the analysis itself (room = 0.5 of the doubled allowance) and
to half of e_y, e_cen and the slot bounds, whose worst-case sums leave that factor as they stand; the fp16 rounding is never doubled.

These are worst-case bounds: the roundings of D terms are taken to conspire, a correct kernel sits near 1 / sqrt(D) of the A' term.  They catch every O(1)
mistake of the statistics, the rows and the operands; a mistake of a few ulps they do not claim to catch.
"""
import collections
import functools
import math

import torch

from dit_ends_cases import MASSIVE_MID, uv_bound

U32, U16 = 2.0 ** -24, 2.0 ** -11
SUM_DEPTH = 32
ROOM = 2.0
EPS = 1e-6
FAMILIES = ("gauss", "offset", "massive", "constant", "tiny", "onehot")
DIRECT_MISTAKES = ("var_over_d_minus_1", "eps_1e-5", "eps_missing", "uncentred_variance", "scale_msa_for_scale_mlp", "one_plus_missing",
                   "shift_scale_swapped", "mod_row_of_image_0", "mod_row_of_wave_first_row")
FOLD_MISTAKES = ("var_over_d_minus_1", "eps_1e-5", "eps_missing", "dl_sq_not_subtracted", "b_sign_flipped", "inv_n_1_over_256", "slot_0_only",
                 "c_from_other_cen", "scale_msa_for_scale_mlp", "one_plus_missing", "shift_scale_swapped", "mod_row_of_image_0")
CONSTANTS = (3000.0, -0.375, 17.25, 2.0 ** -10, 0.0, -1024.5)  # <= 13 significant bits: every partial sum of up to 1280 copies is exact in fp32


def half_ulp16(v):
    """Half an fp16 ulp at magnitude v (float64 tensor): 2^(floor(log2 v) - 11), 2^-25 below the smallest normal."""
    e = torch.floor(torch.log2(torch.clamp(v, min=2.0 ** -14)))
    return torch.exp2(e - 11.0)


def make_rows(family, M, D, seed):
    """fp32 [M, D] rows of one input family."""
    g = torch.Generator().manual_seed(seed * 7907 + 31 * M + D)
    n = torch.randn(M, D, generator=g)
    if family == "gauss":
        return n * 2.0 + 0.3
    if family == "offset":
        return n + 3000.0
    if family == "massive":
        for ch, v in MASSIVE_MID:
            n[:, ch % D] = v
        return n
    if family == "constant":
        return torch.tensor([CONSTANTS[m % len(CONSTANTS)] for m in range(M)])[:, None].expand(M, D).contiguous()
    if family == "tiny":
        return n * 1e-4 + 0.25
    assert family == "onehot"
    x = torch.zeros(M, D)
    x[torch.arange(M), (torch.arange(M) * 7) % D] = 5.0
    return x


def make_mod(rows, D, seed, stride=None):
    """(buffer fp32 [rows, stride], shift view, scale view): shift | scale side by side as in the library's conditioning row, stride >= 2 D."""
    stride = stride or 2 * D
    g = torch.Generator().manual_seed(seed * 613 + rows + D)
    buf = torch.randn(rows, stride, generator=g) * 0.5
    return buf, buf[:, :D], buf[:, D:2 * D]


def image_of_row(M, rows, tokens, device=None):
    """The modulation row of each of M token rows.  tokens may also be that index itself (a long tensor: a selection of rows of a larger matrix)."""
    if torch.is_tensor(tokens):
        return tokens.to(device) if rows > 1 else torch.zeros(M, dtype=torch.long, device=device)
    return torch.div(torch.arange(M, device=device), tokens, rounding_mode="floor") if rows > 1 else torch.zeros(M, dtype=torch.long, device=device)


# ----------------------------------------------------------------------------- DIRECT
def ln_ref(X, shift, scale, tokens):
    """float64 [M, D]: modulate(LayerNorm(x, eps 1e-6), shift, scale); shift / scale [rows, D], row m takes row m // tokens (rows == 1: the shared row)."""
    X = X.double()
    idx = image_of_row(X.shape[0], shift.shape[0], tokens, X.device)
    mu = X.mean(1, keepdim=True)
    var = ((X - mu) ** 2).mean(1, keepdim=True)
    return (X - mu) / torch.sqrt(var + EPS) * (1.0 + scale.double()[idx]) + shift.double()[idx]


def _erho(var, e_var):
    return torch.sqrt((var + EPS) / (torch.clamp(var - e_var, min=0.0) + EPS)) - 1.0 + 4 * U32


def ln_bound(X, shift, scale, tokens, room=1.0, round16=True):
    """float64 [M, D]: the DIRECT bound of the module docstring.  room: the share of the (doubled: ROOM) fp32 allowance granted -- the CPU test grants the
    correct emulation half of it; the fp16 rounding is granted whole (a correctly rounded result reaches its half ulp, no emulation can stay at half of that)."""
    X = X.double()
    idx = image_of_row(X.shape[0], shift.shape[0], tokens, X.device)
    s1, sh = 1.0 + scale.double()[idx], shift.double()[idx]
    mu = X.mean(1, keepdim=True)
    d = X - mu
    var = (d ** 2).mean(1, keepdim=True)
    rho = 1.0 / torch.sqrt(var + EPS)
    y = d * rho * s1 + sh
    e_mu = (SUM_DEPTH + 1) * U32 * X.abs().mean(1, keepdim=True)
    e_rho = _erho(var, (SUM_DEPTH + 4) * U32 * var + e_mu ** 2)
    e32 = room * ROOM * (s1.abs() * rho * (e_mu + U32 * d.abs()) + (d * rho * s1).abs() * (e_rho + 3 * U32) + U32 * y.abs())
    return e32 + half_ulp16(y.abs() + e32) if round16 else e32


def ln_emulate(X, shift, scale, tokens, mistake=None, wave_rows=4, other_scale=None, round16=True):
    """float64 view of the fp16 output of a correct DIRECT kernel (fp32 two-pass statistics, rsqrt, fp32 modulate, one fp16 rounding), or of one with a
    named mistake (round16=False: the fp32 value in front of that rounding; ln_bound(round16=False) is its allowance).  wave_rows: the rows that share a wave / workgroup (mod_row_of_wave_first_row); other_scale: the scale_msa rows."""
    assert mistake is None or mistake in DIRECT_MISTAKES, mistake
    Xf = X.float()
    M, D = Xf.shape
    m = torch.arange(M)
    if mistake == "mod_row_of_wave_first_row":
        m = torch.div(m, wave_rows, rounding_mode="floor") * wave_rows
    idx = torch.div(m, tokens, rounding_mode="floor") if shift.shape[0] > 1 else torch.zeros(M, dtype=torch.long)
    if mistake == "mod_row_of_image_0":
        idx = torch.zeros(M, dtype=torch.long)
    sh, sc = shift.float()[idx], (other_scale if mistake == "scale_msa_for_scale_mlp" else scale).float()[idx]
    if mistake == "shift_scale_swapped":
        sh, sc = sc, sh
    mean = Xf.sum(1, keepdim=True) / D
    d = Xf - mean
    if mistake == "uncentred_variance":
        var = torch.clamp((Xf * Xf).sum(1, keepdim=True) / D - mean * mean, min=0.0)
    else:
        var = (d * d).sum(1, keepdim=True) / (D - 1 if mistake == "var_over_d_minus_1" else D)
    eps = {"eps_1e-5": 1e-5, "eps_missing": 0.0}.get(mistake, EPS)
    rstd = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    one = 0.0 if mistake == "one_plus_missing" else 1.0
    o = d * rstd * (one + sc) + sh
    return o.half().double() if round16 else o.double()


def ratio(got, ref, bound):
    """Largest |got - ref| / bound over every element; inf when any element is not finite."""
    got = got.double()
    if not bool(torch.isfinite(got).all()):
        return float("inf")
    return float(((got - ref).abs() / bound).max())


# cases of lfm_ln_modulate: (name, M, D, tokens, mod rows (0 = one shared row, stride 0), stride of the modulation rows or None = 2 D)
LnCase = collections.namedtuple("LnCase", "name M D tokens rows stride")
WIDTHS = (8, 12, 64, 256, 512, 520, 1024, 1152, 1276, 1280)
ROW_COUNTS = (1, 5, 33, 37)


def _ln_cases():
    out = []
    for i, D in enumerate(WIDTHS):  # every width at every ragged row count, the token counts rotating
        for j, M in enumerate(ROW_COUNTS):
            tokens = (1, 5, 16)[(i + j) % 3]
            out.append(LnCase(f"D{D}-M{M}-T{tokens}", M, D, tokens, -(-M // tokens), None))
    out.append(LnCase("shared-row", 37, 1024, 16, 0, None))
    out.append(LnCase("shared-row-narrow", 33, 12, 5, 0, None))
    out.append(LnCase("wide-stride", 37, 520, 5, 8, 2 * 520 + 24))
    out.append(LnCase("many-workgroups", 2051, 256, 16, 129, None))
    return out


LN_CASES = _ln_cases()


@functools.lru_cache(maxsize=None)
def ln_case(case, family):
    """(X fp32, mod buffer, shift, scale, float64 reference, bound) of a DIRECT case: built once, shared, read-only."""
    seed = 1 + LN_CASES.index(case) * len(FAMILIES) + FAMILIES.index(family)
    X = make_rows(family, case.M, case.D, seed)
    buf, shift, scale = make_mod(max(case.rows, 1), case.D, seed, case.stride)
    return X, buf, shift, scale, ln_ref(X, shift, scale, case.tokens), ln_bound(X, shift, scale, case.tokens)


# ----------------------------------------------------------------------------- FOLDED
def gelu_tanh64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


Fold = collections.namedtuple("Fold", "mean part aprime act r e_cen e_part e_aprime e_act")


def fold_ref(X1, c, shift, scale, W1, b1, tokens, room=1.0):
    """float64 quantities of the FOLDED path from the residual rows X1 [M, D] and the centring constants c [M] (both fp32, exact inputs), the rows
    shift_mlp / scale_mlp [rows, D], the fp16 fc1 weights W1 [H, D] and the fp32 bias b1 -- and the bound of each (module docstring):
    mean [M]; part [M, D / 256, 2]; aprime [M, D]; act [M, H] = gelu_tanh(LN-modulate(X1) W1^T + b1); r [M].  room: as for ln_bound, on the fp16 quantities."""
    X, cc = X1.double(), c.double()[:, None]
    M, D = X.shape
    P = D // 256
    idx = image_of_row(M, shift.shape[0], tokens, X.device)
    s1, sh = 1.0 + scale.double()[idx], shift.double()[idx]
    mu = X.mean(1, keepdim=True)
    var = ((X - mu) ** 2).mean(1, keepdim=True)
    rho = 1.0 / torch.sqrt(var + EPS)
    dc = X - cc
    part = torch.stack([X.reshape(M, P, 256).sum(2), (dc ** 2).reshape(M, P, 256).sum(2)], 2)
    e_part = torch.stack([SUM_DEPTH * U32 * X.abs().reshape(M, P, 256).sum(2), (SUM_DEPTH + 3) * U32 * part[:, :, 1]], 2)
    ap = dc * s1
    e_ap = room * ROOM * 3 * U32 * ap.abs() + half_ulp16(ap.abs() * (1 + 3 * U32))
    dl = mu - cc
    e_cen = (SUM_DEPTH + 7) * U32 * X.abs().mean(1, keepdim=True)
    r = (dl.abs() / torch.sqrt(var))[:, 0]
    if W1 is None:  # the producer's quantities alone
        return Fold(mu[:, 0], part, ap, None, r, e_cen[:, 0], e_part, e_ap, None)
    W, b = W1.double(), b1.double()
    z = ((X - mu) * rho * s1 + sh) @ W.T + b
    y = gelu_tanh64(z)
    # the consumer's bound
    e_dl = e_cen + U32 * dl.abs()
    e_var = (SUM_DEPTH + 10) * U32 * (var + dl ** 2) + 2 * dl.abs() * e_dl + e_dl ** 2 + 2 * U32 * dl ** 2
    e_rho = _erho(var, e_var)
    acc = ap @ W.T
    S1 = ap.abs() @ W.abs().T
    uu, vv = s1 @ W.T, sh @ W.T + b
    e_u, e_v = uv_bound(D) * (s1.abs() @ W.abs().T), uv_bound(D) * (sh.abs() @ W.abs().T + b.abs())
    e_acc = (U16 + (D + 3) * U32) * S1
    e_z = (rho * e_acc * (1 + e_rho) + (rho * (acc - dl * uu)).abs() * e_rho + rho * uu.abs() * e_dl + rho * dl.abs() * e_u + e_v
           + 3 * U32 * ((rho * acc).abs() + (rho * dl * uu).abs() + vv.abs()))
    z2 = 2.3022082 * z.abs() * (1 + 0.044715 * z ** 2)
    e_y = room * (1.13 * e_z + (4 + 3 * z2) * U32 * y.abs())
    return Fold(mu[:, 0], part, ap, y, r, e_cen[:, 0], e_part, e_ap, e_y + half_ulp16(y.abs() + e_y))


def aprime_emulate(X1, c, scale, tokens):
    """fp16 [M, D]: fl(fl(x - c) fl(1 + s)) rounded to nearest even -- the producer epilogue's three operations."""
    idx = image_of_row(X1.shape[0], scale.shape[0], tokens, X1.device)
    return ((X1.float() - c.float()[:, None]) * (1.0 + scale.float()[idx])).half()


def fold_emulate(X1, c, shift, scale, W1, b1, tokens, mistake=None, c_other=None, other_scale=None):
    """float64 view of the fp16 fc1 activation a correct FOLDED path stores (fp32 slots in slot order, g256h_rowstat's arithmetic, fp16 A', fp32
    accumulation, fp32 affine and GELU, one fp16 rounding), or of one with a named mistake.  c_other: the other cen array (c_from_other_cen)."""
    assert mistake is None or mistake in FOLD_MISTAKES, mistake
    Xf, cf = X1.float(), c.float()[:, None]
    M, D = Xf.shape
    P = D // 256
    idx = image_of_row(M, shift.shape[0], tokens)
    if mistake == "mod_row_of_image_0":
        idx = torch.zeros(M, dtype=torch.long)
    sh, sc = shift.float()[idx], (other_scale if mistake == "scale_msa_for_scale_mlp" else scale).float()[idx]
    if mistake == "shift_scale_swapped":
        sh, sc = sc, sh
    s1 = (0.0 if mistake == "one_plus_missing" else 1.0) + sc
    d = Xf - cf
    ap = (d * s1).half()
    slots = P if mistake != "slot_0_only" else 1
    sx, sq = torch.zeros(M), torch.zeros(M)
    for t in range(slots):
        sx = sx + Xf[:, 256 * t:256 * t + 256].sum(1)
        sq = sq + (d * d)[:, 256 * t:256 * t + 256].sum(1)
    if mistake == "var_over_d_minus_1":  # (the divisor of the variance alone)
        sq = sq * (float(D) / (D - 1))
    inv_n = torch.tensor(1.0 / (256 if mistake == "inv_n_1_over_256" else D), dtype=torch.float32)
    mu = sx * inv_n
    dl = mu - (c_other.float() if mistake == "c_from_other_cen" else cf[:, 0])
    var = sq * inv_n if mistake == "dl_sq_not_subtracted" else torch.clamp(sq * inv_n - dl * dl, min=0.0)
    eps = {"eps_1e-5": 1e-5, "eps_missing": 0.0}.get(mistake, EPS)
    a = torch.rsqrt(var + torch.tensor(eps, dtype=torch.float32))
    b = a * dl if mistake == "b_sign_flipped" else -a * dl
    W = W1.double()
    acc = (ap.double() @ W.T).float()
    u, v = (s1.double() @ W.T).float(), (sh.double() @ W.T + b1.double()).float()
    z = a[:, None] * acc + (b[:, None] * u + v)
    return torch.nn.functional.gelu(z, approximate="tanh").half().double()


def budget_crossing(rs, rel):
    """The r at which a per-row rel-L2 bound (rel at the sorted rs) reaches the per-forward budget 2e-3, by log-log interpolation (None: not inside the range)."""
    for (r0, e0), (r1, e1) in zip(zip(rs, rel), zip(rs[1:], rel[1:])):
        if e0 < 2e-3 <= e1:
            return math.exp(math.log(r0) + (math.log(2e-3) - math.log(e0)) / (math.log(e1) - math.log(e0)) * (math.log(r1) - math.log(r0)))
    return None
