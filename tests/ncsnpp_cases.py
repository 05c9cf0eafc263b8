"""Shared pieces of the NCSN++ tests (``SongUNet`` with the Fourier embedding, the residual encoder and the [1,3,3,1] resampling filter): the fixture
configuration, the seeded state both sides regenerate, the three resampling cases of the reference's ``Conv2d`` and the Fourier mapping network restated
in float64, and the seeded faults that show what the tests' bounds separate.

Not a test module.  tools/make_ncsnpp_golden.py imports it too, so that the generator and the tests cannot drift apart."""
import math

import torch

import song_cases as sc

# tests/golden/ncsnpp_tiny.pt: three levels (16x16, 8x8, 4x4) of 64 / 128 / 128 channels.  Both kinds of aux_residual (4 -> 64 on the fp32 network input,
# 64 -> 128 on fp16), a `down` and an `up` block at each of two sizes, attention at 8x8 (64 tokens x 128 channels) and, in `in0`, at 4x4 (16 tokens)
NCSNPP = dict(embedding_type="fourier", channel_mult_noise=2, encoder_type="residual", decoder_type="standard", resample_filter=[1, 3, 3, 1])
TINY_CFG = dict(sc.TINY_CFG, channel_mult=[1, 2, 2], attn_resolutions=[8], **NCSNPP)
FREQS_SEED = 78

F4 = (1.0, 3.0, 3.0, 1.0)  # the filter's taps; f2 = outer(f, f) / 64


def seeded_freqs(n, seed=FREQS_SEED):
    """map_noise.freqs as the reference initialises it, 16 N(0, 1), fp16-representable: arguments 2 pi f t of several hundred radians at t <= 1."""
    return (16.0 * torch.randn(n, generator=torch.Generator().manual_seed(seed))).half().float()


def load_seeded(module, seed=sc.STATE_SEED):
    """song_cases.load_seeded, then map_noise.freqs through load_state_dict: oracle/edm_state.py fills that buffer like a bias (0.05 N(0, 1)), which never
    leaves the first period of the sine.  Returns the checksum the fixture records (the parameters' and the table's)."""
    sc.load_seeded(module, seed)
    sd = module.state_dict()
    sd["map_noise.freqs"] = seeded_freqs(sd["map_noise.freqs"].numel())
    module.load_state_dict(sd, strict=True)
    return float(sum(v.double().abs().sum() for k, v in sd.items() if v.is_floating_point() and not k.endswith("resample_filter")))


def conv_record_inputs(seed=79):
    """Inputs of the three stand-alone records of the reference's own Conv2d (8 channels on a 6 x 10 map): x NCHW, and the 3x3 weight and the non-zero bias
    of the fused record.  The fixture stores the reference's outputs only."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(1, 8, 6, 10, generator=g), torch.randn(8, 8, 3, 3, generator=g) / 72 ** 0.5, 0.5 * torch.randn(8, generator=g)


def nhwc(x):
    return x.permute(0, 2, 3, 1).contiguous()


# ------------------------------------------------------------------------------------------------ the three resampling cases, float64, NHWC
def _pad_hw(x, p):
    return torch.nn.functional.pad(x, (0, 0, p, p, p, p)) if p else x


def fir_down_ref64(x, pad, bias=None, resid=None, scale=1.0, taps=F4, terms=False):
    """x [N, Hi, Wi, C] -> [N, Ho, Wo, C], Hi = 2 Ho + 2 - 2 pad:  y[i, j] = sum_{a,b<4} f[a] f[b] / 64 * x[2i - pad + a, 2j - pad + b], zeros outside;
    then (y + bias + resid) * scale.  pad 1: Conv2d(down=True) not fused (reference models/EDM.py:124-127); pad 0: the filter stage of the fused path (:118).
    terms=True: also sum |w_k x_k| over the taps, the bias and the residual (the accumulation term of the element-wise bound)."""
    d = torch.float64
    xp = _pad_hw(x.to(d), pad)
    Ho, Wo = (xp.shape[1] - 2) // 2, (xp.shape[2] - 2) // 2
    f = torch.tensor(taps, dtype=d)
    y = torch.zeros(x.shape[0], Ho, Wo, x.shape[3], dtype=d)
    mag = torch.zeros_like(y)
    for a in range(4):
        for b in range(4):
            w = f[a] * f[b] / f.sum() ** 2
            v = xp[:, a:a + 2 * Ho:2, b:b + 2 * Wo:2, :]
            y += w * v
            mag += (w * v).abs()
    if bias is not None:
        y, mag = y + bias.to(d), mag + bias.to(d).abs()
    if resid is not None:
        y, mag = y + resid.to(d).reshape(y.shape), mag + resid.to(d).reshape(y.shape).abs()
    return (y * scale, mag * abs(scale)) if terms else y * scale


def fir_up_ref64(x, per_axis_gain=2.0, terms=False):
    """x [N, H, W, C] -> [N, 2H, 2W, C]: conv_transpose2d with 4 f2, stride 2, padding 1 (reference :120-123): along each axis
    y[2i] = (3 x[i] + x[i-1]) / 4, y[2i+1] = (3 x[i] + x[i+1]) / 4, zeros outside.  per_axis_gain = 1 is the seeded fault (taps f / 8, no x2)."""
    d = torch.float64
    g = per_axis_gain / 8.0

    def axis(v, dim):
        n = v.shape[dim]
        z = torch.zeros_like(v.narrow(dim, 0, 1))
        prev, nxt = torch.cat([z, v.narrow(dim, 0, n - 1)], dim), torch.cat([v.narrow(dim, 1, n - 1), z], dim)
        even, odd = g * (3 * v + prev), g * (3 * v + nxt)
        return torch.stack([even, odd], dim + 1).flatten(dim, dim + 1)

    y = axis(axis(x.to(d), 1), 2)
    if terms:
        return y, axis(axis(x.to(d).abs(), 1), 2)
    return y


def conv3x3_ref64(x, w, pad):
    """x [N, H, W, Cin] (*) w [Cout, Cin, 3, 3] at padding `pad`, float64, NHWC out [N, H + 2 pad - 2, W + 2 pad - 2, Cout]."""
    d = torch.float64
    y = torch.nn.functional.conv2d(x.to(d).permute(0, 3, 1, 2), w.to(d), padding=pad)
    return y.permute(0, 2, 3, 1).contiguous()


def fused_down_ref64(x, w, bias, resid=None, scale=1.0, fault=None):
    """Conv2d(kernel=3, down=True, fused_resample=True) (reference :116-118, :130-131): the 3x3 convolution at PADDING 2, H x W -> (H+2) x (W+2), then f2 at
    stride 2 with NO padding -> H/2 x W/2, the bias after the filter; then (. + resid) * scale, the encoder's (x + aux_residual(aux)) / sqrt(2) (:686).
    Faults: "filter_first" -- the filter at pad 1 before a pad-1 convolution on the small map (the zero border enters at another stage);
            "bias_first" -- the bias added to the convolution's output, before the filter."""
    if fault == "filter_first":
        y = conv3x3_ref64(fir_down_ref64(x, 1), w, 1) + bias.double()
    elif fault == "bias_first":
        y = fir_down_ref64(conv3x3_ref64(x, w, 2) + bias.double(), 0)
    else:
        assert fault is None
        y = fir_down_ref64(conv3x3_ref64(x, w, 2), 0) + bias.double()
    if resid is not None:
        y = y + resid.double().reshape(y.shape)
    return y * scale


# ------------------------------------------------------------------------------------------------ the Fourier mapping network, float64
def fourier_args32(t, freqs):
    """fl32(t * fl32(fl32(2 pi) * f)) as float64 values: the reference's two fp32 roundings (x.ger((2 * np.pi * self.freqs).to(x.dtype)), :520), so that
    the yardstick measures the kernel and not an ulp of a 300-radian argument."""
    g = torch.tensor(2 * math.pi, dtype=torch.float32) * freqs.float()
    return (t.float().reshape(-1, 1) * g.reshape(1, -1)).double()


def fourier_mapping_ref64(freqs, w0, b0, w1, b1, t, N, label_w=None, label_b=None, y=None, swap=True):
    """SongUNet's mapping network with embedding_type = "fourier" (reference :663-675, FourierEmbedding :512-522) in float64:
    emb = silu(W1 silu(W0 ([sin(a) | cos(a)] + sqrt(L) W_label[:, y] + b_label) + b0) + b1), a = fourier_args32(t, freqs).  swap=False is the seeded
    fault: the embedding's own [cos | sin] order, without forward's swap."""
    d = torch.float64
    a = fourier_args32(t, freqs)
    F = w0.shape[1]
    e = (torch.cat([a.sin(), a.cos()], 1) if swap else torch.cat([a.cos(), a.sin()], 1)).expand(N, F)
    if y is not None:
        e = e + math.sqrt(label_w.shape[1]) * label_w.to(d).t()[y] + label_b.to(d)
    h = sc.silu64(e @ w0.to(d).t() + b0.to(d))
    return sc.silu64(h @ w1.to(d).t() + b1.to(d))
