"""Inputs, references and a device emulation for the tiled DiT attention kernel (csrc/attention_tiled_kernel.h), shared by tests/test_dit_attention_tiled_ref.py
(CPU) and tests/test_gpu_dit_attention_tiled.py.

Inputs as tests/test_gpu_dit.py::test_attention: q, k = randn * 1.5, v = randn, all fp16.  SPIKY keys: in every image the key rows (all heads) at four places
are scaled x 6 -- a score of ~13 standard deviations against ~2.25 for the others, so the running maximum of the online softmax jumps where the row sits and
the block takes its rescale path (a forced rescale needs an input of its own):
    key 7                     the first stage, and inside the first 16 keys: the rows that would LEAK in behind the previous image's last key are spiky
    a key of a middle stage
    key 64 (T // 64 - 1) + 20 the last FULL stage
    key T - 5                 the last 16 keys: what a dropped or mis-ordered tail loses
`reference` is float64 over the full tensor.  `emulate` is the kernel's arithmetic with its rounding points: fp32 scores from the fp16 operands, keys in blocks of
32, an online softmax that follows the maximum, P = 2^((s - m) scale) rounded to fp16 for the P V product, the row sum from the unrounded values in fp32, fp32
accumulation, fp16 output -- and, by name, the mistakes the kernel's two tails invite."""
import functools
import math

import torch

# (T, heads, batch, head_dim): 144 = 2.25 stages (grid 12 = 4 x 3: half a softmax block), 400 = 6.25 (grid 20), 576 = 9, 784 = 12.25 (grid 28), 1296 = 20.25,
# 2304 = 36, 3600 = 56.25 -- whole and ragged stage counts for both head sizes, one to three (image, head) items per image
SHAPES = [(144, 2, 3, 64), (144, 2, 3, 72), (400, 3, 2, 64), (576, 2, 2, 72), (784, 2, 2, 64), (1296, 1, 2, 72), (2304, 1, 2, 64), (3600, 1, 1, 72)]
MISTAKES = ("drop_last16", "leak_next16", "no_rescale", "tail_no_vt_pos", "pad72_not_zeroed")
TOL_WHOLE, TOL_ITEM, TOL_ROW = 2e-3, 4e-3, 4e-3  # rel-L2 against float64: whole tensor, worst (image, head) item, worst query row


def spiky_keys(T):
    nst = (T + 63) // 64
    keys = [7, 64 * (nst // 2) + 37, T - 5]
    if T >= 64:
        keys.append(64 * (T // 64 - 1) + 20)
    return sorted({k for k in keys if 0 <= k < T})


def make_qkv(T, heads, batch, hd, seed=None):
    """q, k, v fp16 [batch, heads, T, hd]."""
    g = torch.Generator().manual_seed(T + heads + hd if seed is None else seed)
    q = (torch.randn(batch, heads, T, hd, generator=g) * 1.5).half()
    k = (torch.randn(batch, heads, T, hd, generator=g) * 1.5).half()
    v = torch.randn(batch, heads, T, hd, generator=g).half()
    for key in spiky_keys(T):
        k[:, :, key] *= 6
    return q, k, v


def vt_token_perm(T):
    """Index p with Vt_library[..., i] = Vt_plain[..., p[i]] (lfm_amd.hip.vt_token_perm, restated so that the CPU side needs no library)."""
    i = torch.arange(T)
    return (i & ~12) | ((i & 4) << 1) | ((i & 8) >> 1)


def operands(q, k, v):
    """The library's operands: Q, K [batch * T, D] with head-major columns, V^T [batch, heads, hd, T] in the vt_pos token order."""
    batch, heads, T, hd = q.shape
    D = heads * hd
    Q = q.transpose(1, 2).reshape(batch * T, D).contiguous()
    K = k.transpose(1, 2).reshape(batch * T, D).contiguous()
    Vt = v.transpose(-1, -2)[..., vt_token_perm(T)].contiguous()
    return Q, K, Vt


def reference(q, k, v):
    """float64 softmax(q k^T hd^-0.5) v -> [batch, heads, T, hd]."""
    hd = q.shape[-1]
    out = torch.empty(q.shape, dtype=torch.float64)
    for b in range(q.shape[0]):  # per image: the score matrix of 3600 tokens is 100 MB in float64
        s = (q[b].double() @ k[b].double().transpose(-1, -2)) * hd ** -0.5
        out[b] = torch.softmax(s, -1) @ v[b].double()
    return out


@functools.lru_cache(maxsize=None)
def case(T, heads, batch, hd):
    """(q, k, v, float64 reference) of a shape: computed once, shared, never modified."""
    q, k, v = make_qkv(T, heads, batch, hd)
    return q, k, v, reference(q, k, v)


def as_rows(O, batch, heads, T, hd):
    """The library's O [batch * T, heads * hd] -> [batch, heads, T, hd]."""
    return O.reshape(batch, T, heads, hd).transpose(1, 2)


def errors(got, ref):
    """rel-L2 of got [batch, heads, T, hd] against the float64 ref: (whole, worst item, worst query row)."""
    d = got.double() - ref
    whole = float(d.norm() / ref.norm())
    item = float((d.pow(2).sum((2, 3)).sqrt() / ref.pow(2).sum((2, 3)).sqrt()).max())
    row = float((d.pow(2).sum(3).sqrt() / ref.pow(2).sum(3).sqrt()).max())
    return whole, item, row


def emulate(q, k, v, mistake=None):
    """The kernel's arithmetic (see the module docstring) -> fp16 [batch, heads, T, hd]; `mistake`: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES
    batch, heads, T, hd = q.shape
    sl2 = hd ** -0.5 * 1.4426950408889634
    qf, kf, vf = q.float(), k.float(), v.float()
    kext, vext = kf, vf
    Tk = T
    if mistake == "drop_last16":
        Tk = T - 16
    if mistake == "leak_next16":  # what lies behind the item: the next image's first 16 K rows; behind V^T row d, the first 16 entries of the row after it
        kext = torch.cat([kf, kf.roll(-1, 0)[:, :, :16]], 2)
        vt = v.transpose(-1, -2)[..., vt_token_perm(T)].contiguous()  # memory order
        flat = torch.cat([vt.reshape(-1), vt.reshape(-1)[:16]])
        idx = (torch.arange(batch * heads * hd) * T + T)[:, None] + torch.arange(16)[None]
        behind = flat[idx].reshape(batch, heads, hd, 16)[..., vt_token_perm(16)]  # positions -> tokens of the 16-group
        vext = torch.cat([vf, behind.float().transpose(-1, -2)], 2)
        Tk = T + 16
    if mistake == "tail_no_vt_pos":  # the last 16-group taken in memory order: token j gets the V row of token vt_pos(j)
        vext = vf.clone()
        vext[:, :, T - 16:] = vf[:, :, T - 16:][:, :, vt_token_perm(16)]
    s_extra = None
    if mistake == "pad72_not_zeroed":  # dims 72 .. 79 of the fifth k-slot: the next head's first 8 columns (the row's own first columns behind the last head)
        assert hd == 72
        s_extra = qf.roll(-1, 1)[..., :8] @ kf.roll(-1, 1)[..., :8].transpose(-1, -2)
    m = torch.full((batch, heads, T), -3.0e38)
    l = torch.zeros(batch, heads, T)
    o = torch.zeros(batch, heads, T, hd)
    for k0 in range(0, Tk, 32):
        k1 = min(k0 + 32, Tk)
        s = qf @ kext[:, :, k0:k1].transpose(-1, -2)
        if s_extra is not None:
            s = s + s_extra[..., k0:k1]
        mnew = torch.maximum(m, s.max(-1).values)
        alpha = torch.exp2((m - mnew) * sl2)
        if mistake == "no_rescale" and k0 >= 64:  # the state carried from stage to stage is left as it was
            alpha = torch.ones_like(alpha)
        p = torch.exp2((s - mnew[..., None]) * sl2)
        l = l * alpha + p.sum(-1)
        o = o * alpha[..., None] + p.half().float() @ vext[:, :, k0:k1]
        m = mnew
    return (o / l[..., None]).half()


def is_square_grid(T):
    g = math.isqrt(T)
    return g * g == T and g % 4 == 0
