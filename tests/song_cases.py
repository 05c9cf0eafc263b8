"""Shared pieces of the SongUNet (ddpm++) tests: the two fixture configurations, the seeded weights both sides regenerate (the fixtures hold inputs,
reference outputs, the reference's key / shape list and a checksum -- not the 3 M / 13 M parameters), and the two mapping networks restated in float64.

Not a test module.  tools/make_song_golden.py imports it too, so that the generator and the tests cannot drift apart."""
import math

import torch

STATE_SEED = 77

# tests/golden/song_tiny.pt: two levels (16x16, 8x8), attention at 8x8 (64 tokens x 128 channels, one head) and in `in0`; class-conditional
TINY_CFG = dict(img_resolution=16, in_channels=4, out_channels=4, label_dim=5, augment_dim=0, model_channels=64, channel_mult=[1, 2], channel_mult_emb=4,
                num_blocks=1, attn_resolutions=[8], dropout=0.0, label_dropout=0.0, embedding_type="positional", channel_mult_noise=1,
                encoder_type="standard", decoder_type="standard", resample_filter=[1, 1])
# tests/golden/song_wide.pt: one head of 256 channels at 256 tokens (16x16) and at 64 tokens (8x8): the attention shape of the class defaults
WIDE_CFG = dict(TINY_CFG, label_dim=0, model_channels=128, attn_resolutions=[16, 8])


def load_seeded(module, seed=STATE_SEED):
    """Fill a reference or product SongUNet with the seeded state (oracle/edm_state.py: one generator per tensor name, fp16-representable values, no tensor
    left at the reference's 0 / 1e-5 initialisation); returns the checksum the fixture records."""
    from oracle.edm_state import load_seeded as _load

    return _load(module, seed)


def silu64(v):
    return v * torch.sigmoid(v)


def song_mapping_ref64(w0, b0, w1, b1, t, N, label_w=None, label_b=None, y=None):
    """SongUNet's mapping network (reference models/EDM.py:663-675, PositionalEmbedding :490-505 with endpoint=True) in float64:
    emb = silu(W1 silu(W0 ([sin(t f) | cos(t f)] + sqrt(L) W_label[:, y] + b_label) + b0) + b1),  f_i = 10000^(-i / (F/2 - 1)).  t: 1 or N values."""
    d = torch.float64
    F = w0.shape[1]
    half = F // 2
    f = torch.pow(torch.tensor(1.0 / 10000.0, dtype=d), torch.arange(half, dtype=d) / (half - 1))
    a = t.to(d).reshape(-1, 1) * f
    e = torch.cat([a.sin(), a.cos()], 1).expand(N, F)
    if y is not None:
        L = label_w.shape[1]
        e = e + math.sqrt(L) * label_w.to(d).t()[y] + label_b.to(d)
    h = silu64(e @ w0.to(d).t() + b0.to(d))
    return silu64(h @ w1.to(d).t() + b1.to(d))


def adm_time_embed_ref64(w0, b0, w2, b2, t, N, label_table=None, y=None):
    """lfm_time_embed's formula (include/lfm_hip.h) in float64: emb = W2 silu(W0 [cos(t f) | sin(t f)] + b0) + b2 (+ label_table[y]),
    f_i = 10000^(-i / (F/2)).  The control of the mapping-kernel test."""
    d = torch.float64
    F = w0.shape[1]
    half = F // 2
    f = torch.exp(-math.log(10000.0) * torch.arange(half, dtype=d) / half)
    a = t.to(d).reshape(-1, 1) * f
    e = torch.cat([a.cos(), a.sin()], 1).expand(N, F)
    emb = silu64(e @ w0.to(d).t() + b0.to(d)) @ w2.to(d).t() + b2.to(d)
    if y is not None:
        emb = emb + label_table.to(d)[y]
    return emb
