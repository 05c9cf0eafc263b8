"""Shared pieces of the layout-UNet tests (``UNetModelAttn``: the ADM UNet whose attention blocks are SpatialTransformers): the two fixture configurations,
the seeded weights both sides regenerate (the fixtures hold inputs, contexts, reference outputs, the reference's key / shape list and a checksum -- not the
parameters), float64 restatements of the three new device ops (cross-attention, LayerNorm, GEGLU), constructed inputs for them, the bounds the GPU tests
hold them to, and fp32-staged emulations of a correct kernel and of kernels with one named mistake each.

Not a test module.  tools/make_layout_golden.py imports it too, so that the generator and the tests cannot drift apart.  TEST INFRASTRUCTURE ONLY."""
import functools
import zlib

import torch

from unet_attention_cases import KEY_BLOCK, TOL, item_errors, worst  # noqa: F401  (the project's per-item tolerance and error measure)

STATE_SEED = 91

# tests/golden/layout_tiny.pt: SpatialTransformers of depth 3 at 256 tokens x 64 channels (heads of 32) and 64 tokens x 128 channels (heads of 64), in the
# input, middle and output blocks; context of 512 features
TINY_CFG = dict(image_size=16, in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(1, 2), channel_mult=(1, 2),
                num_heads=2, use_scale_shift_norm=True, use_spatial_transformer=True, transformer_depth=3, context_dim=512, legacy=True)
# tests/golden/layout_self.pt: context=None (attn2 attends over its own input: block width 128 == context_dim), class labels by keyword
SELF_CFG = dict(TINY_CFG, attention_resolutions=(2,), transformer_depth=1, context_dim=128, num_classes=5, num_heads=4)
TINY_BATCH = 3
CONTEXT_LENGTHS = (17, 77)  # one ragged key block; a full block plus a ragged one

_SMALL_GAIN = (".proj_out.weight", ".out_layers.3.weight", ".to_out.0.weight", ".ff.net.2.weight")  # the reference's zero-initialised layers and the residual writers


def seeded_state(named_shapes, seed=STATE_SEED):
    """{name: fp32 tensor} for the floating tensors of a UNetModelAttn: one generator per tensor name (order-independent), fp16-representable values, NO tensor
    left at the reference's zero initialisation (with proj_out at zero the whole transformer drops out of the output).  Matrices N(0, gain^2 / fan_in) with
    gain 0.3 for proj_out, out_layers.3, out.2, to_out.0, ff.net.2 and 1 elsewhere; GroupNorm / LayerNorm scales 1 + 0.1 n; every bias 0.05 n."""
    out = {}
    for name, shape in named_shapes:
        g = torch.Generator().manual_seed((int(seed) * 1000003 + zlib.crc32(name.encode())) % (2 ** 63 - 1))
        shape = tuple(shape)
        if name.endswith(".weight") and len(shape) >= 2:
            fan_in = 1
            for d in shape[1:]:
                fan_in *= d
            gain = 0.3 if name.endswith(_SMALL_GAIN) or name == "out.2.weight" else 1.0
            v = torch.randn(shape, generator=g) * (gain / fan_in ** 0.5)
        elif name.endswith(".weight"):
            v = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            v = 0.05 * torch.randn(shape, generator=g)
        out[name] = v.half().float()
    return out


def load_seeded(module, seed=STATE_SEED):
    """Fill a reference or product UNetModelAttn with the seeded state (strict); returns the checksum the fixture records."""
    sd = module.state_dict()
    new = seeded_state([(k, v.shape) for k, v in sd.items() if v.is_floating_point()], seed)
    sd.update(new)
    module.load_state_dict(sd, strict=True)
    return float(sum(v.double().abs().sum() for v in new.values()))


def make_inputs(cfg, batch=TINY_BATCH):
    """x, t [N], the contexts by length, labels: what both fixtures are evaluated on."""
    g = torch.Generator().manual_seed(113)
    x = torch.randn(batch, cfg["in_channels"], cfg["image_size"], cfg["image_size"], generator=g)
    tN = torch.tensor([0.9, 0.5, 0.05])[:batch]
    ctx = {L: torch.randn(batch, L, cfg["context_dim"], generator=g).half().float() for L in CONTEXT_LENGTHS}
    y = torch.tensor([1, 4, 0])[:batch]
    return x, tN, ctx, y


# ------------------------------------------------------------------------------------------------------------ cross-attention
CROSS_N, CROSS_HEADS = 3, 2
CROSS_FAMILIES = ("gauss", "spike_last", "offset_pos")
# (Tq, Tk, ch): Tq = 100 leaves dead queries in the last wave, ch = 48 uses the zero-padded channel tile, Tk straddles the 64-key block edge both ways
CROSS_SHAPES = [(64, 17, 32), (100, 65, 64), (256, 77, 64), (64, 130, 128), (17, 64, 48), (1, 1, 16), (256, 256, 256)]
CROSS_MISTAKES = ("last_key_dropped", "padding_not_masked", "keys_counted_as_queries", "next_image_context_read", "o_not_rescaled", "sum_not_rescaled")


def make_cross_case(family, Tq, Tk, ch, N=CROSS_N, heads=CROSS_HEADS):
    """fp16 q [N, heads, Tq, ch], k, v [N, heads, Tk, ch]: the families of unet_attention_cases.make_case with a token count per side."""
    fam = CROSS_FAMILIES.index(family)
    g = torch.Generator().manual_seed(((((fam * 64 + N) * 64 + heads) * 512 + ch) * 8192 + Tq) * 8192 + Tk)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    q, k, v = 1.6 * rn(N, heads, Tq, ch), 1.6 * rn(N, heads, Tk, ch), 1.6 * rn(N, heads, Tk, ch)
    if family == "spike_last":  # ONE key whose logit lies ~ 9 sqrt(ch) above the rest, the last one: in the ragged block
        s = torch.sign(q.mean(dim=2, keepdim=True))
        q = q + 1.5 * s
        k[:, :, Tk - 1] = 6 * s[:, :, 0]
    elif family == "offset_pos":  # a common component in q and k: every logit near +200
        a = (200 / ch ** 0.5) ** 0.5
        q, k = q + a, k + a
    return q.half(), k.half(), v.half()


def rows(t):
    """[N, heads, T, ch] -> the library's token-major [N * T, heads * ch]."""
    N, H, T, ch = t.shape
    return t.permute(0, 2, 1, 3).reshape(N * T, H * ch).contiguous()


def items_of_rows(out, N, heads, T, ch):
    """The library's out [N * T, heads * ch] -> float64 [N * heads, T, ch] on the CPU."""
    return out.detach().cpu().double().reshape(N, T, heads, ch).permute(0, 2, 1, 3).reshape(N * heads, T, ch)


@torch.no_grad()
def cross_exact(q, k, v):
    """float64 [N * heads, Tq, ch]."""
    q, k, v = (t.double().flatten(0, 1) for t in (q, k, v))
    return torch.softmax(q @ k.transpose(1, 2) * q.shape[-1] ** -0.5, dim=-1) @ v


def _rows_from(flat, first, count):
    """`count` rows of flat [rows, ch] from row `first` on; rows past the end of the buffer read as zeros (an emulation cannot read out of bounds)."""
    idx = torch.arange(first, first + count)
    got = flat[idx.clamp(max=flat.shape[0] - 1)].clone()
    got[idx >= flat.shape[0]] = 0
    return got


@torch.no_grad()
def cross_emulate(q, k, v, mistake=None):
    """float64 [N * heads, Tq, ch] holding fp16 values: a CORRECT kernel's staging -- keys in blocks of 64, fp32 scores, running maximum and sum, P rounded to
    fp16, fp32 accumulators rescaled when the maximum rises, fp16 output -- or, with `mistake`, the same with one indexing or rescaling mistake."""
    assert mistake is None or mistake in CROSS_MISTAKES
    N, H, Tq, ch = q.shape
    Tk = k.shape[2]
    scale = ch ** -0.5
    out = []
    for n in range(N):
        for h in range(H):
            qi, ki, vi = q[n, h].double(), k[n, h].double(), v[n, h].double()
            if mistake == "last_key_dropped":
                ki, vi = ki[:Tk - 1], vi[:Tk - 1]
            elif mistake == "keys_counted_as_queries":  # the key loop and its masks bounded by Tq: keys cut short, or rows of the next image read as keys
                kf, vf = k[:, h].double().reshape(N * Tk, ch), v[:, h].double().reshape(N * Tk, ch)
                ki, vi = _rows_from(kf, n * Tk, Tq), _rows_from(vf, n * Tk, Tq)
            elif mistake == "next_image_context_read":  # K / V row base n * Tq instead of n * Tk
                kf, vf = k[:, h].double().reshape(N * Tk, ch), v[:, h].double().reshape(N * Tk, ch)
                ki, vi = _rows_from(kf, n * Tq, Tk), _rows_from(vf, n * Tq, Tk)
            nk = ki.shape[0]
            m = torch.full((Tq, 1), -3.0e38, dtype=torch.float64)
            l = torch.zeros(Tq, 1, dtype=torch.float64)
            o = torch.zeros(Tq, ch, dtype=torch.float64)
            for k0 in range(0, nk, KEY_BLOCK):
                kb, vb = ki[k0:k0 + KEY_BLOCK], vi[k0:k0 + KEY_BLOCK]
                if mistake == "padding_not_masked" and kb.shape[0] < KEY_BLOCK:  # the zeros of the LDS image take part as keys
                    pad = torch.zeros(KEY_BLOCK - kb.shape[0], ch, dtype=torch.float64)
                    kb, vb = torch.cat([kb, pad]), torch.cat([vb, pad])
                s = (qi @ kb.t()).float().double()  # fp32 scores
                mn = torch.maximum(m, s.amax(dim=-1, keepdim=True))
                alpha = torch.exp(((m - mn) * scale).clamp(min=-1e4)).float().double()
                p = torch.exp((s - mn) * scale).float().double()
                l = ((l if mistake == "sum_not_rescaled" else l * alpha) + p.sum(dim=-1, keepdim=True)).float().double()
                o = ((o if mistake == "o_not_rescaled" else o * alpha) + p.half().double() @ vb).float().double()  # P in fp16, fp32 accumulators
                m = mn
            out.append((o / l).half().double())
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def cross_case(family, Tq, Tk, ch):
    """((q, k, v) fp16, exact float64 [items, Tq, ch]) of a family at a shape: built once, shared, read-only."""
    qkv = make_cross_case(family, Tq, Tk, ch)
    return qkv, cross_exact(*qkv)


# ------------------------------------------------------------------------------------------------------------ LayerNorm
LN_ROWS, LN_WIDTHS, LN_EPS = 37, (64, 128, 512, 1024), 1e-5
LN_FAMILIES = ("gauss", "offset200", "outlier")


@functools.lru_cache(maxsize=None)
def ln_case(family, C, M=LN_ROWS):
    """(x fp16 [M, C], gamma fp32 [C] = 1 + 0.1 n, beta fp32 [C] = 0.05 n, float64 reference)."""
    g = torch.Generator().manual_seed(LN_FAMILIES.index(family) * 100003 + C)
    x = torch.randn(M, C, generator=g, dtype=torch.float64)
    if family == "offset200":  # every value offset by +200 with unit spread: E[x^2] - E[x]^2 cancels five digits
        x = x + 200
    elif family == "outlier":  # channel 0 an outlier 1000x the rest
        x[:, 0] = 1000 * (1 + 0.1 * x[:, 0])
    x = x.half()
    gamma = (1 + 0.1 * torch.randn(C, generator=g)).float()
    beta = (0.05 * torch.randn(C, generator=g)).float()
    return x, gamma, beta, ln_exact(x, gamma, beta)


def ln_exact(x, gamma, beta, eps=LN_EPS):
    x = x.double()
    mu = x.mean(dim=1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * gamma.double() + beta.double()


def ln_bound(x, gamma, beta, eps=LN_EPS):
    """Per-element bound on |kernel - float64| for a two-pass fp32 LayerNorm with an fp16 result, derived (profiles/layout_unet_tests.txt), not measured.
    u = 2^-24, A = max |x| of the row, sigma = the row's exact standard deviation, r = 1 / sqrt(sigma^2 + eps):
      d_mu  <= C u A                                   the mean: a sum of C fp32 terms in ANY order ((C - 1) u sum|x|), its division, its rounding
      d_r/r <= (C + 2) u / 2 + d_mu^2 r^2 / 2 + 3 u    the centred sum of squares in any order, the shift by d_mu (second order), sqrt and division
      |err| <= |gamma| r d_mu (1 + d_r/r)              x - mean at the family's offset
             + |ref - beta| (d_r/r + 4 u)              the scale, and the roundings of the subtraction, the two products and the sum
             + 2^-11 (1 + 2^-10) |ref| + 2^-25         the one rounding to fp16 (of a value that already carries the errors above); fp16 subnormals."""
    u = 2.0 ** -24
    xd, C = x.double(), x.shape[1]
    A = xd.abs().amax(dim=1, keepdim=True)
    mu = xd.mean(dim=1, keepdim=True)
    r = 1 / torch.sqrt(((xd - mu) ** 2).mean(dim=1, keepdim=True) + eps)
    d_mu = C * u * A
    d_r = (C + 2) * u / 2 + (d_mu * r) ** 2 / 2 + 3 * u
    ref = ln_exact(x, gamma, beta, eps)
    pre = gamma.double().abs() * r * d_mu * (1 + d_r) + (ref - beta.double()).abs() * (d_r + 4 * u)
    return pre + 2.0 ** -11 * (1 + 2.0 ** -10) * (ref.abs() + pre) + 2.0 ** -25


def _sum32(t):
    """Row sums of fp32 [M, C] accumulated term by term in fp32 (torch's own sum is pairwise, and accumulates fp32 in double in places)."""
    s = torch.zeros(t.shape[0], dtype=torch.float32)
    for c in range(t.shape[1]):
        s = s + t[:, c]
    return s[:, None]


def ln_emulate(x, gamma, beta, eps=LN_EPS, mistake=None):
    """fp32 statistics and arithmetic, fp16 result, as float64.  mistake="one_pass_variance": var = E[x^2] - E[x]^2 from one pass of fp32 sums."""
    assert mistake in (None, "one_pass_variance")
    xf = x.float()
    C = xf.shape[1]
    mean = _sum32(xf) / C
    var = _sum32(xf * xf) / C - mean * mean if mistake else _sum32((xf - mean) ** 2) / C
    y = (xf - mean) * (1.0 / torch.sqrt(var + eps)) * gamma + beta  # a negative one-pass variance gives NaN, as it would on the device
    return y.half().double()


# ------------------------------------------------------------------------------------------------------------ GEGLU
GEGLU_ROWS, GEGLU_WIDTHS = 37, (256, 512, 2048)


@functools.lru_cache(maxsize=None)
def geglu_case(I, M=GEGLU_ROWS):
    """(h fp16 [M, 2I] = [value | gate], float64 reference): gates spread over [-12, 12], including values the erf form sends to +-0."""
    g = torch.Generator().manual_seed(7000 + I)
    a = 2 * torch.randn(M, I, generator=g, dtype=torch.float64)
    gate = 24 * torch.rand(M, I, generator=g, dtype=torch.float64) - 12
    gate[:, 0], gate[:, 1], gate[:, 2], gate[:, 3] = -12.0, 12.0, 0.0, -0.0
    h = torch.cat([a, gate], 1).half()
    return h, geglu_exact(h)


def geglu_exact(h):
    a, g = h.double().chunk(2, dim=1)
    return a * (0.5 * g * torch.special.erfc(-g / 2 ** 0.5))  # g Phi(g), without the cancellation of 1 + erf in float64 either


def geglu_bound(h):
    """Per element: 2^-11 (1 + 2^-7) |ref| + 2^-22 |x g| + 2^-25 -- the fp16 rounding with 2^-18 of relative fp32 error in front of it; the cancellation in
    1 + erf(g / sqrt 2) for negative gates in fp32; fp16 subnormals."""
    a, g = h.double().chunk(2, dim=1)
    return 2.0 ** -11 * (1 + 2.0 ** -7) * geglu_exact(h).abs() + 2.0 ** -22 * (a * g).abs() + 2.0 ** -25


def geglu_emulate(h, mistake=None):
    """fp32 arithmetic with the erf form, fp16 result, as float64.  mistake="tanh_gelu": the tanh approximation the library's other GELU is."""
    assert mistake in (None, "tanh_gelu")
    a, g = h.float().chunk(2, dim=1)
    if mistake:
        return (a * torch.nn.functional.gelu(g, approximate="tanh")).half().double()
    return (a * (0.5 * g * (1 + torch.erf(g * 0.70710678118654752)))).half().double()
