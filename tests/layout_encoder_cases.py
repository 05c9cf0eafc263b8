"""Shared pieces of the layout-encoder tests (``BERTEmbedder``: tokens -> the context of ``UNetModelAttn``): the fixture configurations, the seeded weights
and tokens both sides regenerate (tests/golden/layout_encoder.pt holds configurations, tokens, reference outputs, the reference's key / shape list and a
checksum -- not the parameters), the float64 restatement of the encoder, the same restatement with fp16 roundings at exactly the places where the device
stores fp16, restatements with one named mistake each, and the cases, references and bounds of the two new device ops (lfm_token_embed_f16,
lfm_linear_gelu_f16).

Not a test module.  tools/make_layout_encoder_golden.py imports it too, so that the generator and the tests cannot drift apart.  TEST INFRASTRUCTURE ONLY."""
import functools
import zlib
from types import SimpleNamespace

import torch

import adm_context_cases as ac

from lfm_amd.models.encoder import DIM_HEAD, HEADS, INNER  # the product's head geometry (8 x 64): the restatement and the key list follow it

STATE_SEED = 97
assert (HEADS, DIM_HEAD, INNER) == (8, 64, 512)  # x_transformer.py:14, 211-212

# name -> (constructor arguments, batch, token counts).  L = 17: one ragged 64-key block; 77: a full block plus a ragged one; 92: the whole position table.
# n_embed = 128: to_q is [512, 128], the heads stay 8 x 64.  deep16: the LDM layout-to-image conditioner (16 layers, 92 tokens, vocabulary 8192).
CASES = {
    "w512": (dict(n_embed=512, n_layer=2, vocab_size=64, max_seq_len=92), 3, (17, 77, 92)),
    "w128": (dict(n_embed=128, n_layer=2, vocab_size=64, max_seq_len=92), 3, (17,)),
    "deep16": (dict(n_embed=512, n_layer=16, vocab_size=8192, max_seq_len=92), 2, (92,)),
}
SOLVE_CASE = ("w512", 17)  # the context of the 10-step Euler solve on layout_cases.TINY_CFG (context_dim 512, batch 3)


def case_ids():
    return [(name, L) for name, (_, _, Ls) in CASES.items() for L in Ls]


def seeded_state(named_shapes, seed=STATE_SEED):
    """{name: fp32 tensor}: one generator per tensor name (order-independent), fp16-representable values.  Linear weights N(0, 1 / fan_in), the two embedding
    tables N(0, 0.02^2) (the reference's own initialisation), LayerNorm scales 1 + 0.1 n, every bias 0.05 n (the reference's LayerNorm biases start at zero,
    where a dropped or misplaced bias would not show)."""
    out = {}
    for name, shape in named_shapes:
        g = torch.Generator().manual_seed((int(seed) * 1000003 + zlib.crc32(name.encode())) % (2 ** 63 - 1))
        shape = tuple(shape)
        if "emb.weight" in name:
            v = 0.02 * torch.randn(shape, generator=g)
        elif name.endswith(".weight") and len(shape) == 2:
            v = torch.randn(shape, generator=g) / shape[1] ** 0.5
        elif name.endswith(".weight"):
            v = 1.0 + 0.1 * torch.randn(shape, generator=g)
        else:
            v = 0.05 * torch.randn(shape, generator=g)
        out[name] = v.half().float()
    return out


def load_seeded(module, seed=STATE_SEED):
    """Fill a reference or product BERTEmbedder with the seeded state (strict); returns (the state, the checksum the fixture records)."""
    sd = module.state_dict()
    new = seeded_state([(k, v.shape) for k, v in sd.items() if v.is_floating_point()], seed)
    sd.update(new)
    module.load_state_dict(sd, strict=True)
    return new, float(sum(v.double().abs().sum() for v in new.values()))


def key_shapes(n_embed, n_layer, vocab_size, max_seq_len):
    """The reference's state-dict keys and shapes in its order, written out from x_transformer.py (the fixture's recorded list is compared with this one)."""
    D, p = n_embed, "transformer."
    ks = [(p + "token_emb.weight", (vocab_size, D)), (p + "pos_emb.emb.weight", (max_seq_len, D))]
    for i in range(n_layer):
        a, f = f"{p}attn_layers.layers.{2 * i}.", f"{p}attn_layers.layers.{2 * i + 1}."
        ks += [(a + "0.weight", (D,)), (a + "0.bias", (D,)), (a + "1.to_q.weight", (INNER, D)), (a + "1.to_k.weight", (INNER, D)), (a + "1.to_v.weight", (INNER, D)),
               (a + "1.to_out.weight", (D, INNER)), (a + "1.to_out.bias", (D,)),
               (f + "0.weight", (D,)), (f + "0.bias", (D,)), (f + "1.net.0.0.weight", (4 * D, D)), (f + "1.net.0.0.bias", (4 * D,)),
               (f + "1.net.2.weight", (D, 4 * D)), (f + "1.net.2.bias", (D,))]
    return ks + [(p + "norm.weight", (D,)), (p + "norm.bias", (D,)), (p + "to_logits.weight", (vocab_size, D)), (p + "to_logits.bias", (vocab_size,))]


@functools.lru_cache(maxsize=None)
def case_state(name):
    """The seeded state of a case without constructing a module: {key: fp32 tensor}.  Built once, shared, read-only."""
    return seeded_state(key_shapes(**CASES[name][0]))


@functools.lru_cache(maxsize=None)
def make_tokens(name, L):
    """int64 [N, L]: seeded ids over the whole vocabulary, the first and the last id among them, and a repeated id inside one sequence."""
    cfg, N, _ = CASES[name]
    g = torch.Generator().manual_seed(5000 + 131 * L + zlib.crc32(name.encode()) % 1000)
    t = torch.randint(0, cfg["vocab_size"], (N, L), generator=g)
    t[0, 0], t[-1, -1] = 0, cfg["vocab_size"] - 1
    if L > 2:
        t[0, 2] = t[0, 1]
    return t


def sample_cols(rows, D):
    """Column indices [rows, 64] of the reference values the fixture stores (the fixture stays well under 1 MB): every (D / 64)-th column, the offset rotating
    with the row, so that every column of the output is held in some row."""
    s = max(1, D // 64)
    return (torch.arange(64)[None, :] * s + (torch.arange(rows)[:, None] % s)) % D


def sampled(out):
    """[N, L, D] -> the stored values [N * L, 64]."""
    flat = out.reshape(-1, out.shape[-1])
    return torch.gather(flat, 1, sample_cols(flat.shape[0], flat.shape[1]))


# ------------------------------------------------------------------------------------------------------------ the encoder in float64
MISTAKES = ("tanh_gelu", "no_position_embedding", "positions_off_by_one", "post_norm", "no_final_norm", "to_out_bias_dropped", "scale_by_n_embed",
            "keys_up_to_max_seq_len")


# |gelu_tanh(x) - gelu_erf(x)| <= 4.8e-4 for every x, against hidden rows of rms ~0.6 that the device rounds to fp16 (2^-11 relative = 2.9e-4 of that rms, per
# store, eight stores per layer pair): at the level of the whole encoder the tanh form moves the output by LESS than the fp16 stores do (measured 2e-4 vs
# 8e-4 rel-L2 at two layers), so no bound made of those roundings separates the two.  The per-element bound of lfm_linear_gelu_f16 does, on pre-activations
# in [-3, -1.5] (test_layout_encoder_ref.py, test_gpu_layout_encoder_kernels.py): that is where this mistake is held.
BELOW_STORE_NOISE = ("tanh_gelu",)


def mistake_shows(mistake, cfg, L):
    """Whether a mistake can change the result of a case at all: keys taken up to max_seq_len are the right keys where L == max_seq_len."""
    return not (mistake == "keys_up_to_max_seq_len" and L == cfg["max_seq_len"])


def gelu_erf64(x):
    return 0.5 * x * torch.special.erfc(-x / 2 ** 0.5)


def gelu_tanh64(x):
    return 0.5 * x * (1 + torch.tanh((2 / torch.pi) ** 0.5 * (x + 0.044715 * x ** 3)))


def layernorm64(x, g, b, eps=1e-5):
    mu = x.mean(dim=-1, keepdim=True)
    var = ((x - mu) ** 2).mean(dim=-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * g + b


def _rows_from(flat, first, count):
    """`count` rows of flat [rows, C] from row `first` on; rows past the end of the buffer read as zeros (an emulation cannot read out of bounds)."""
    idx = torch.arange(first, first + count)
    got = flat[idx.clamp(max=flat.shape[0] - 1)].clone()
    got[idx >= flat.shape[0]] = 0
    return got


@torch.no_grad()
def encode64(sd, tokens, cfg, fp16_stores=False, mistake=None):
    """BERTEmbedder.forward(tokens) (encoder.py:77-83 -> x_transformer.py:582-605 with return_embeddings=True, :468-520, :260-356, :193-203) in float64:
    float64 [N, L, n_embed].  fp16_stores: every tensor the device path writes to memory as fp16 is rounded to fp16 there -- the embedding sum, every
    LayerNorm output, the QKV rows, the attention output, both residual sums, the GELU rows and the final norm (weights are fp16-representable already) -- and
    nothing else is (accumulators, scores, softmax and the GELU argument stay exact).  mistake: one of MISTAKES."""
    assert mistake is None or mistake in MISTAKES, mistake
    d = torch.float64
    r = (lambda t: t.half().to(d)) if fp16_stores else (lambda t: t)
    w = lambda k: sd["transformer." + k].to(d)  # noqa: E731
    N, L = tokens.shape
    D, rows = cfg["n_embed"], cfg["max_seq_len"]
    pos = w("pos_emb.emb.weight")
    x = w("token_emb.weight")[tokens]
    if mistake == "positions_off_by_one":
        x = x + pos[(torch.arange(L) + 1) % rows]
    elif mistake != "no_position_embedding":
        x = x + pos[:L]
    x = r(x).reshape(N * L, D)
    scale = (D if mistake == "scale_by_n_embed" else DIM_HEAD) ** -0.5
    gelu = gelu_tanh64 if mistake == "tanh_gelu" else gelu_erf64
    post = mistake == "post_norm"
    n_blocks = 2 * cfg["n_layer"]
    for i in range(n_blocks):
        p = f"attn_layers.layers.{i}."
        norm = lambda v: r(layernorm64(v, w(p + "0.weight"), w(p + "0.bias")))  # noqa: E731
        t = x if post else norm(x)
        if i % 2 == 0:
            q, k, v = (r(t @ w(p + f"1.to_{c}.weight").t()) for c in "qkv")
            a = torch.empty(N * L, INNER, dtype=d)
            for n in range(N):
                sl = slice(n * L, (n + 1) * L)
                kn, vn = (k[sl], v[sl]) if mistake != "keys_up_to_max_seq_len" else (_rows_from(k, n * L, rows), _rows_from(v, n * L, rows))
                qh = q[sl].reshape(L, HEADS, DIM_HEAD).transpose(0, 1)
                kh, vh = (m.reshape(-1, HEADS, DIM_HEAD).transpose(0, 1) for m in (kn, vn))
                a[sl] = (torch.softmax(qh @ kh.transpose(1, 2) * scale, dim=-1) @ vh).transpose(0, 1).reshape(L, INNER)
            out = r(a) @ w(p + "1.to_out.weight").t() + (0 if mistake == "to_out_bias_dropped" else w(p + "1.to_out.bias"))
        else:
            h = r(gelu(t @ w(p + "1.net.0.0.weight").t() + w(p + "1.net.0.0.bias")))
            out = h @ w(p + "1.net.2.weight").t() + w(p + "1.net.2.bias")
        x = r(out + x)
        if post and i != n_blocks - 1:  # x_transformer.py:512-513
            x = norm(x)
    if mistake != "no_final_norm":
        x = r(layernorm64(x, w("norm.weight"), w("norm.bias")))
    return x.reshape(N, L, D)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def max_abs(a, b):
    return float((a.double().cpu() - b.double().cpu()).abs().max())


MARGIN = 2.0  # device error <= MARGIN x the fp16-store emulation's error on the same inputs (the VAE resnet stage tests' margin: fp32 MFMA accumulation order lies below the fp16 store rounding the emulation already contains)


@functools.lru_cache(maxsize=None)
def case_exact(name, L):
    """(tokens, float64 restatement, (rel-L2, max-abs) of the fp16-store emulation against it): computed once per case, shared, read-only."""
    cfg = CASES[name][0]
    tok, sd = make_tokens(name, L), case_state(name)
    ref = encode64(sd, tok, cfg)
    emu = encode64(sd, tok, cfg, fp16_stores=True)
    return tok, ref, (rel_l2(emu, ref), max_abs(emu, ref))


# ------------------------------------------------------------------------------------------------------------ lfm_token_embed_f16
EMBED_WIDTHS, EMBED_LENGTHS, EMBED_VOCAB, EMBED_POS_ROWS, EMBED_N = (8, 128, 512), (1, 17, 92), 37, 92, 3


@functools.lru_cache(maxsize=None)
def embed_case(D, L):
    """(tok fp32 [vocab, D], pos fp32 [92, D], ids int64 [N, L], the reference fp16 [N * L, D] = (tok[ids] + pos[:L]).half()).  Table values with 24
    significant bits, so that the fp32 add and the one rounding are both exercised (a sum rounded to fp16 twice, or added in fp16, differs)."""
    g = torch.Generator().manual_seed(100 * D + L)
    tok, pos = torch.randn(EMBED_VOCAB, D, generator=g), torch.randn(EMBED_POS_ROWS, D, generator=g)
    ids = torch.randint(0, EMBED_VOCAB, (EMBED_N, L), generator=g)
    ids[0, 0], ids[-1, -1] = EMBED_VOCAB - 1, 0
    return tok, pos, ids, (tok[ids] + pos[:L]).half().reshape(EMBED_N * L, D)


# ------------------------------------------------------------------------------------------------------------ lfm_linear_gelu_f16
def gelu_bound(pre, mag, K):
    """Per-element bound on |kernel - float64| for C = fp16(gelu_erf(acc + bias)) with an fp32 accumulator, derived the way adm_context_cases.silu_case derives
    the SiLU one; x = the pre-activation, mag = |A| |W|^T + |bias|:
        bound = 1.13 (K + 2) 2^-23 mag           the fp32 accumulation error of x (K + 1 additions in any order) through |gelu'| <= 1.129
              + (x^2 + 8) 2^-23 |ref|            0.5 x erfc(z), z = -x / sqrt 2 rounded to fp32: d log erfc / d log z -> -2 z^2 = -x^2 on the negative tail, so
                                                 the argument's rounding costs x^2 2^-24 relative; erfcf itself and the two products a few ulp
              + 2^-11 (1 + 2^-9) |ref| + 2^-25   ONE rounding to fp16 (of a value already off by the terms above), the subnormal floor."""
    ref = gelu_erf64(pre)
    return 1.13 * (K + 2) * 2.0 ** -23 * mag + (pre ** 2 + 8) * 2.0 ** -23 * ref.abs() + 2.0 ** -11 * (1 + 2.0 ** -9) * ref.abs() + 2.0 ** -25


@functools.lru_cache(maxsize=None)
def gelu_case(M, N, K):
    """A, W fp16 N(0, 1) / N(0, 1 / K), bias fp32 spread over [-6, 6]: pre-activations on both tails of the GELU.  -> A, W, bias, pre, ref, bound, resid=None."""
    g = torch.Generator().manual_seed(9000 + M * 7 + N * 3 + K)
    A = torch.randn(M, K, generator=g).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias = (12 * torch.rand(N, generator=g) - 6).float()
    pre = A.double() @ W.double().t() + bias.double()
    mag = A.double().abs() @ W.double().abs().t() + bias.double().abs()
    return SimpleNamespace(M=M, N=N, K=K, A=A, W=W, bias=bias, pre=pre, ref=gelu_erf64(pre), bound=gelu_bound(pre, mag, K), resid=None)


@functools.lru_cache(maxsize=None)
def gelu_zero_acc_case(M, N, K):
    """Integer-valued operands whose every dot product is exactly zero (A's columns come in +v / -v pairs against equal W columns) and a bias in [-3, -1.5],
    where the erf and the tanh GELU differ by far more than an fp16 ulp of the result: the output must be fp16(gelu_erf(bias)) -- one rounding."""
    g = torch.Generator().manual_seed(9100 + M + N + K)
    a = torch.randint(-4, 5, (M, K // 2), generator=g).float()
    wv = torch.randint(-4, 5, (N, K // 2), generator=g).float()
    A, W = torch.cat([a, -a], 1).half(), torch.cat([wv, wv], 1).half()
    bias = (-3 + 1.5 * torch.rand(N, generator=g)).float()
    for _ in range(64):  # keep gelu(bias) 2^-17 (relative) away from every fp16 rounding boundary: an fp32 evaluation good to 2^-17 then rounds as float64 does
        y = gelu_erf64(bias.double())
        near = ((y * (1 + 2.0 ** -17)).half() != y.half()) | ((y * (1 - 2.0 ** -17)).half() != y.half())
        if not bool(near.any()):
            break
        bias = torch.where(near, (bias + 2.0 ** -10).clamp(max=-1.5), bias)
    assert not bool(near.any()) and not bool((A.double() @ W.double().t()).any())
    return SimpleNamespace(M=M, N=N, K=K, A=A, W=W, bias=bias, resid=None, ref=gelu_erf64(bias.double())[None, :].expand(M, N))


def gelu_emulate(pre, mistake=None):
    """fp32 arithmetic on the (float64-exact) pre-activation, fp16 result, as float64.  mistake="tanh_gelu": the tanh form of the library's other epilogue."""
    assert mistake in (None, "tanh_gelu")
    x = pre.float()
    if mistake:
        return torch.nn.functional.gelu(x, approximate="tanh").half().double()
    return (0.5 * x * torch.special.erfc(-x * 0.70710678118654752)).half().double()


KERNEL_SELECTIONS, KERNEL_LAYOUTS, kernel_shapes = ac.KERNEL_SELECTIONS, ac.KERNEL_LAYOUTS, ac.kernel_shapes
