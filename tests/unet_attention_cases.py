"""Constructed inputs, a float64 reference and an fp16-staged online-softmax emulation for the UNet attention ``lfm_attention_small_f16`` (TEST
INFRASTRUCTURE ONLY; shared by tests/test_unet_attention_ref.py and tests/test_gpu_unet_attention_stream.py).

The operation (QKVAttentionLegacy, one (image, head) item at a time): ``softmax(q k^T / sqrt(ch)) v`` on fp16 operands.  Inputs have the reference's
layout ``[N, heads * 3 * ch, T]`` (per head ``[q | k | v]``) and are rounded to fp16; ``tokens`` gives the token-major tensor the library reads.
``exact`` is float64 throughout.  ``emulate`` is a CORRECT streamed kernel's staging -- keys in blocks of 64, fp32 scores, running maximum and sum,
P rounded to fp16, fp32 accumulators rescaled when the maximum rises, fp16 output -- and, with ``mistake=...``, the same with one indexing or
rescaling mistake a streamed kernel can make.  Errors are rel-L2 per (image, head) item, never over the tensor as a whole: one wrong item of many
must not hide in the norm of the others.
"""
import functools

import torch

FAMILIES = ("gauss", "rising", "spike_first", "spike_last", "offset_pos", "offset_neg")
MISTAKES = ("last_key_dropped", "padding_not_masked", "next_item_key_read", "block_maximum_only", "o_not_rescaled", "sum_not_rescaled")
KEY_BLOCK = 64
TOL = 2e-3  # the project's per-item tolerance of the UNet attention tests (tests/test_gpu_unet.py)


def make_case(family, N, heads, ch, T):
    """fp16 [N, heads * 3 * ch, T]; the seed depends on the family and the shape."""
    fam = FAMILIES.index(family)
    g = torch.Generator().manual_seed((((fam * 64 + N) * 64 + heads) * 512 + ch) * 8192 + T)

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    items = N * heads
    q, k, v = 1.6 * rn(items, ch, T), 1.6 * rn(items, ch, T), 1.6 * rn(items, ch, T)  # gauss: N(0, 1.6^2), the spread of tests/test_gpu_unet.py
    if family == "rising":  # the logit grows with the key index: the running maximum rises in every key block
        u = rn(items, ch, 1)
        q = 0.5 * rn(items, ch, T) + 2 * torch.sign(u)
        k = 0.5 * rn(items, ch, T) + u * torch.linspace(0.2, 3, T, dtype=torch.float64)
    elif family in ("spike_first", "spike_last"):  # ONE key whose logit lies ~ 9 sqrt(ch) above the rest, in the first / the last (ragged) key block
        s = torch.sign(q.mean(dim=2, keepdim=True))
        q = q + 1.5 * s
        k[:, :, 0 if family == "spike_first" else T - 1] = 6 * s[:, :, 0]
    elif family in ("offset_pos", "offset_neg"):  # a common component in q and k: every logit near +200 / -200
        a = (200 / ch ** 0.5) ** 0.5
        q = q + a
        k = k + (a if family == "offset_pos" else -a)
    return torch.stack([q, k, v], dim=1).reshape(N, heads * 3 * ch, T).half()


def tokens(qkv):
    """[N, heads * 3 * ch, T] -> the library's token-major [N * T, heads * 3 * ch] (columns [head][q | k | v][ch])."""
    N, W, T = qkv.shape
    return qkv.permute(0, 2, 1).reshape(N * T, W).contiguous()


def items_of_output(out, N, heads, ch, T):
    """The library's out [N * T, heads * ch] -> float64 [N * heads, T, ch] on the CPU."""
    return out.detach().cpu().double().reshape(N, T, heads, ch).permute(0, 2, 1, 3).reshape(N * heads, T, ch)


def _split(qkv, heads, ch):
    N, _, T = qkv.shape
    q, k, v = qkv.double().reshape(N * heads, 3, ch, T).unbind(dim=1)
    return q.transpose(1, 2), k.transpose(1, 2), v.transpose(1, 2)  # [items, T, ch]


@torch.no_grad()
def exact(qkv, heads, ch):
    """float64 [items, T, ch]."""
    q, k, v = _split(qkv, heads, ch)
    return torch.softmax(q @ k.transpose(1, 2) * ch ** -0.5, dim=-1) @ v


@torch.no_grad()
def emulate(qkv, heads, ch, mistake=None):
    """float64 [items, T, ch] holding fp16 values: the streamed kernel's arithmetic in float64, rounded where the kernel rounds."""
    assert mistake is None or mistake in MISTAKES
    q, k, v = _split(qkv, heads, ch)
    items, T, _ = q.shape
    scale = ch ** -0.5
    if mistake == "last_key_dropped":
        k, v = k[:, :T - 1], v[:, :T - 1]
    elif mistake == "next_item_key_read":  # token 0 of the next item follows this item's last token in memory
        k, v = torch.cat([k, k.roll(-1, 0)[:, :1]], 1), torch.cat([v, v.roll(-1, 0)[:, :1]], 1)
    nk = k.shape[1]
    m = torch.full((items, T, 1), -3.0e38, dtype=torch.float64)
    l = torch.zeros(items, T, 1, dtype=torch.float64)
    o = torch.zeros(items, T, ch, dtype=torch.float64)
    for k0 in range(0, nk, KEY_BLOCK):
        kb, vb = k[:, k0:k0 + KEY_BLOCK], v[:, k0:k0 + KEY_BLOCK]
        if mistake == "padding_not_masked" and kb.shape[1] < KEY_BLOCK:  # the zeros of the LDS image take part as keys
            pad = torch.zeros(items, KEY_BLOCK - kb.shape[1], ch, dtype=torch.float64)
            kb, vb = torch.cat([kb, pad], 1), torch.cat([vb, pad], 1)
        s = (q @ kb.transpose(1, 2)).float().double()  # fp32 scores
        bm = s.amax(dim=-1, keepdim=True)
        mn = bm if mistake == "block_maximum_only" else torch.maximum(m, bm)
        alpha = torch.exp(((m - mn) * scale).clamp(min=-1e4)).float().double()
        p = torch.exp((s - mn) * scale).float().double()
        l = ((l if mistake == "sum_not_rescaled" else l * alpha) + p.sum(dim=-1, keepdim=True)).float().double()
        o = ((o if mistake == "o_not_rescaled" else o * alpha) + p.half().double() @ vb).float().double()  # P in fp16, fp32 accumulators
        m = mn
    return (o / l).half().double()


def item_errors(got, ref):
    """rel-L2 per (image, head) item of got [items, T, ch] against ref; an item that is not finite counts as nan."""
    return (got.double() - ref).flatten(1).norm(dim=1) / ref.flatten(1).norm(dim=1)


def worst(got, ref):
    """The worst per-item error as a float; nan when any item is not finite."""
    e = item_errors(got, ref)
    return float("nan") if not bool(torch.isfinite(e).all()) else float(e.max())


@functools.lru_cache(maxsize=None)
def case(family, N, heads, ch, T):
    """(qkv fp16 [N, heads * 3 * ch, T], exact float64 [items, T, ch]) of a family at a shape: built once, shared, read-only."""
    qkv = make_case(family, N, heads, ch, T)
    return qkv, exact(qkv, heads, ch)
