"""Shared pieces of the ``adm_context`` tests (``DhariwalUNet(use_context=True)``: every block a ``UNetBlockWithContext``, the label embedding the context of a
``TransformerBlock``): the fixture configuration, the seeded state both sides regenerate, float64 restatements of the ``TransformerBlock``, of the closed
form of its one-key cross-attention and of the whole network, and the seeded faults that show what the tests' bounds separate.

Not a test module.  tools/make_adm_context_golden.py imports it too, so that the generator and the tests cannot drift apart."""
import math

import torch
import torch.nn.functional as F

STATE_SEED = 83
TABLE_SEED = 84
ATTN2_QK_SEED = 85  # a second draw of attn2.q / attn2.k: the output may not change in any bit

# tests/golden/adm_context_tiny.pt: two levels (16x16, 8x8) of 64 / 128 channels.  Transformers at 256 tokens x 64 channels x 1 head (16x16_block0 of the
# encoder, 16x16_block0/1 of the decoder), at 64 tokens x 128 channels x 2 heads (8x8_block0, 8x8_in0, 8x8_block0/1 of the decoder); context blocks WITHOUT a
# transformer in 8x8_down, 16x16_up and 8x8_in1.  label_dropout > 0: the embedding table has label_dim + 1 rows.
TINY_CFG = dict(img_resolution=16, in_channels=4, out_channels=4, label_dim=10, augment_dim=0, model_channels=64, channel_mult=[1, 2], channel_mult_emb=4,
                num_blocks=1, attn_resolutions=[16, 8], dropout=0.0, label_dropout=0.1, use_context=True)
NULL_ROW = TINY_CFG["label_dim"]  # the row label dropout trains
CFG_SCALE = 1.5

FAULTS = ("no_u", "u_mod_tokens", "cfg_null_row", "qkv_order", "gelu")
# no_u          the context term left out of the attn1.proj epilogue
# u_mod_tokens  the context row indexed by m % tokens instead of m / tokens (m = image * tokens + token)
# cfg_null_row  forward_with_cfg overwrites the second half's labels with the null row (what drop_half_label does WITHOUT use_context)
# qkv_order     the packed qkv rows left in [q | k | v][head][ch] order while the kernel reads [head][q | k | v][ch] (no effect on one head)
# gelu          tanh-GELU in place of SiLU in the feed-forward


def seeded_table(rows, emb, seed=TABLE_SEED):
    """map_label.embedding_table.weight at UNIT scale (nn.Embedding's own initialisation is N(0, 1)), fp16-representable.  oracle/edm_state.py would draw it
    like a linear weight, O(1 / sqrt(emb)): the context term would be ~0.03 of the residual stream and an error in it would hide below every bound."""
    return torch.randn(rows, emb, generator=torch.Generator().manual_seed(seed)).half().float()


def load_seeded(module, seed=STATE_SEED):
    """Fill a reference or product DhariwalUNet(use_context=True): oracle/edm_state.py's seeded state, then the label table re-drawn at unit scale.
    Returns the checksum the fixture records."""
    from oracle.edm_state import load_seeded as _load

    _load(module, seed)
    sd = module.state_dict()
    k = "map_label.embedding_table.weight"
    sd[k] = seeded_table(*sd[k].shape)
    module.load_state_dict(sd, strict=True)
    return float(sum(v.double().abs().sum() for kk, v in sd.items() if v.is_floating_point() and not kk.endswith("resample_filter")))


def redraw_attn2_qk(sd, seed=ATTN2_QK_SEED):
    """A copy of the state with every attn2.q / attn2.k tensor drawn anew (unit normal: far from the seeded values)."""
    g = torch.Generator().manual_seed(seed)
    out = dict(sd)
    n = 0
    for k, v in sd.items():
        if ".attn2.q." in k or ".attn2.k." in k:
            out[k] = torch.randn(v.shape, generator=g)
            n += 1
    assert n
    return out


T0D = 0.6


def inputs(seed=87):
    """The seeded inputs of the fixture (regenerated on both sides; the fixture keeps a checksum of x): x [4, 4, 16, 16]; labels that include the extra row
    `label_dim`; per-sample times; another label for a batch of ONE (x[3:]); the two label sets of the guided records -- second half the null row, second half
    class 0 (what the drivers pass for every non-DiT model)."""
    from types import SimpleNamespace

    x = torch.randn(4, 4, 16, 16, generator=torch.Generator().manual_seed(seed))
    return SimpleNamespace(x=x, y=torch.tensor([3, NULL_ROW, 0, 7]), tN=torch.tensor([0.9, 0.5, 0.3, 0.05]), y2=torch.tensor([5]),
                           y_cfg_null=torch.tensor([3, 7, NULL_ROW, NULL_ROW]), y_cfg_zero=torch.tensor([3, 7, 0, 0]))


def block_input(C=128, R=4, N=2, seed=86):
    """The seeded input of the lone-TransformerBlock record: x [N, C, R, R] fp16-representable, and labels (the null row among them)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(N, C, R, R, generator=g).half().float(), torch.tensor([7, NULL_ROW, 2, 7])[:N]


BLOCK = "dec.8x8_in0"  # the TransformerBlock of the lone record: 64 tokens x 128 channels x 2 heads


# ------------------------------------------------------------------------------------------------ float64 pieces
def silu64(v):
    return v * torch.sigmoid(v)


def gelu_tanh64(v):
    return 0.5 * v * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (v + 0.044715 * v ** 3)))


def _d(sd, k):
    return sd[k].double()


def gn64(x, sd, pre, eps=1e-5):
    C = x.shape[1]
    return F.group_norm(x, min(32, C // 4), _d(sd, pre + ".weight"), _d(sd, pre + ".bias"), eps)


def conv1x1_64(x, sd, pre):
    w = _d(sd, pre + ".weight")
    return torch.einsum("oc,nchw->nohw", w.reshape(w.shape[0], -1), x) + _d(sd, pre + ".bias").reshape(1, -1, 1, 1)


def attn2_closed_form64(sd, pre, ctx):
    """attn2(norm2(x), context) of a TransformerBlock whose context is ONE key per image: softmax over one finite score is exactly 1, so every pixel gets
    proj.W (v.W ctx[n] + v.b) + proj.b -- no x, no norm2, no q, no k.  ctx [N, E] float64 -> [N, C]."""
    C = sd[pre + ".v.weight"].shape[0]
    val = ctx @ _d(sd, pre + ".v.weight").reshape(C, -1).t() + _d(sd, pre + ".v.bias")
    return val @ _d(sd, pre + ".proj.weight").reshape(C, C).t() + _d(sd, pre + ".proj.bias")


def attn2_full64(sd, pre, x, ctx, heads):
    """The same module evaluated as written (reference CrossAttention.forward, :408-424) with its q, k and the softmax: the control of the closed form."""
    N, C, H, W = x.shape
    ch = C // heads
    q = conv1x1_64(x, sd, pre + ".q").reshape(N * heads, ch, H * W)
    c4 = ctx.reshape(N, -1, 1, 1)
    k = conv1x1_64(c4, sd, pre + ".k").reshape(N * heads, ch, 1)
    v = conv1x1_64(c4, sd, pre + ".v").reshape(N * heads, ch, 1)
    w = torch.einsum("ncq,nck->nqk", q, k / math.sqrt(ch)).softmax(dim=2)
    a = torch.einsum("nqk,nck->ncq", w, v)
    return conv1x1_64(a.reshape(N, C, H, W), sd, pre + ".proj")


def self_attention64(sd, pre, x, heads, fault=None):
    """attn1 (reference :408-424 with context = x): heads of C // heads channels, channel = head * ch + c, softmax(q^T k / sqrt(ch)) over the H*W keys."""
    N, C, H, W = x.shape
    ch = C // heads
    q, k, v = (conv1x1_64(x, sd, f"{pre}.{n}") for n in "qkv")
    if fault == "qkv_order":  # rows stacked [q | k | v][head][ch], read as [head][q | k | v][ch]
        s = torch.cat([q, k, v], 1).reshape(N, heads, 3, ch, H, W)
        q, k, v = (s[:, :, i].reshape(N, C, H, W) for i in range(3))
    q, k, v = (t.reshape(N * heads, ch, H * W) for t in (q, k, v))
    w = torch.einsum("ncq,nck->nqk", q, k / math.sqrt(ch)).softmax(dim=2)
    a = torch.einsum("nqk,nck->ncq", w, v)
    return conv1x1_64(a.reshape(N, C, H, W), sd, pre + ".proj")


def transformer_ref64(sd, pre, x, ctx, fault=None, closed_form=True):
    """TransformerBlock.forward (reference :477-483) in float64; x [N, C, H, W], ctx [N, E].  closed_form=False evaluates attn2 as written."""
    x, ctx = x.double(), ctx.double()
    N, C, H, W = x.shape
    heads = C // 64
    x = self_attention64(sd, pre + ".attn1", gn64(x, sd, pre + ".norm1"), heads, fault) + x
    if closed_form:
        u = attn2_closed_form64(sd, pre + ".attn2", ctx)  # [N, C]
        if fault == "no_u":
            u = torch.zeros_like(u)
        if fault == "u_mod_tokens":  # row m = n * T + tok of the token matrix takes u[(m % T) % N] instead of u[m // T]
            m = torch.arange(N * H * W)
            x = x + u[(m % (H * W)) % N].reshape(N, H, W, C).permute(0, 3, 1, 2)
        else:
            x = x + u.reshape(N, C, 1, 1)
    else:
        x = attn2_full64(sd, pre + ".attn2", gn64(x, sd, pre + ".norm2"), ctx, heads) + x
    t = gn64(x, sd, pre + ".norm3").reshape(N, C, H * W).permute(0, 2, 1)
    act = gelu_tanh64 if fault == "gelu" else silu64
    t = act(t @ _d(sd, pre + ".ff.layer0.weight").t() + _d(sd, pre + ".ff.layer0.bias"))
    t = t @ _d(sd, pre + ".ff.layer1.weight").t() + _d(sd, pre + ".ff.layer1.bias")
    return t.permute(0, 2, 1).reshape(N, C, H, W) + x


def _resample64(x, up, down):
    """EDM Conv2d's [1,1] filter (reference :96-127): nearest 2x up, 2x2 mean down."""
    if up:
        return x.repeat_interleave(2, 2).repeat_interleave(2, 3)
    if down:
        return F.avg_pool2d(x, 2)
    return x


def _conv64(x, sd, pre, up=False, down=False):
    x = _resample64(x, up, down)
    if pre + ".weight" in sd:
        w = _d(sd, pre + ".weight")
        x = F.conv2d(x, w, padding=w.shape[-1] // 2) + _d(sd, pre + ".bias").reshape(1, -1, 1, 1)
    return x


def block_ref64(sd, pre, x, emb, ctx, fault=None):
    """UNetBlockWithContext.forward (reference :349-367), skip_scale 1, adaptive scale."""
    up, down = pre.endswith("_up"), pre.endswith("_down")
    orig = x
    x = _conv64(silu64(gn64(x, sd, pre + ".norm0")), sd, pre + ".conv0", up, down)
    params = emb @ _d(sd, pre + ".affine.weight").t() + _d(sd, pre + ".affine.bias")
    scale, shift = params.reshape(*params.shape, 1, 1).chunk(2, dim=1)
    x = silu64(shift + gn64(x, sd, pre + ".norm1") * (scale + 1))
    x = _conv64(x, sd, pre + ".conv1")
    has_skip = up or down or (pre + ".skip.weight") in sd
    x = x + (_conv64(orig, sd, pre + ".skip", up, down) if has_skip else orig)
    if (pre + ".transformer.norm1.weight") in sd:
        x = transformer_ref64(sd, pre + ".transformer", x, ctx, fault)
    return x


def mapping_ref64(sd, t, N, model_channels):
    """emb = silu(map_layer1(silu(map_layer0([cos | sin](t f))))), f_i = 10000^(-i / (F/2)) (reference :814-818, :831; PositionalEmbedding :490-505).
    The time embedding ALONE: under use_context the label embedding is the context, not a term of emb."""
    d = torch.float64
    half = model_channels // 2
    f = (1.0 / 10000.0) ** (torch.arange(half, dtype=d) / half)
    a = t.to(d).reshape(-1, 1) * f
    e = torch.cat([a.cos(), a.sin()], 1).expand(N, 2 * half)
    h = silu64(e @ _d(sd, "map_layer0.weight").t() + _d(sd, "map_layer0.bias"))
    return silu64(h @ _d(sd, "map_layer1.weight").t() + _d(sd, "map_layer1.bias"))


def unet_ref64(sd, cfg, t, x, y, fault=None):
    """DhariwalUNet(use_context=True).forward (reference :812-845) in float64 on a state dict of the reference's names."""
    x = x.double()
    N = x.shape[0]
    emb = mapping_ref64(sd, t, N, cfg["model_channels"])
    ctx = _d(sd, "map_label.embedding_table.weight")[y]
    enc = [k[4:-len(".norm0.weight")] for k in sd if k.startswith("enc.") and k.endswith(".norm0.weight")]
    dec = [k[4:-len(".norm0.weight")] for k in sd if k.startswith("dec.") and k.endswith(".norm0.weight")]
    R = cfg["img_resolution"]
    x = _conv64(x, sd, f"enc.{R}x{R}_conv")
    skips = [x]
    for name in enc:
        x = block_ref64(sd, "enc." + name, x, emb, ctx, fault)
        skips.append(x)
    for name in dec:
        if x.shape[1] != sd[f"dec.{name}.norm0.weight"].shape[0]:
            x = torch.cat([x, skips.pop()], 1)
        x = block_ref64(sd, "dec." + name, x, emb, ctx, fault)
    return _conv64(silu64(gn64(x, sd, "out_norm")), sd, "out_conv")


def cfg_ref64(sd, cfg, t, x, y, scale=CFG_SCALE, fault=None):
    """forward_with_cfg (reference :847-861) under use_context: [half, half] evaluated with the labels AS GIVEN -- drop_half_label is ignored --, then
    uncond + scale (cond - uncond) in both halves."""
    n2 = x.shape[0] // 2
    y = y.clone()
    if fault == "cfg_null_row":
        y[n2:] = cfg["label_dim"]
    out = unet_ref64(sd, cfg, t, torch.cat([x[:n2], x[:n2]], 0), y, fault)
    cond, uncond = out[:n2], out[n2:]
    half = uncond + scale * (cond - uncond)
    return torch.cat([half, half], 0)


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------ the kernels' cases (lfm_linear_resid_vec_f16, lfm_linear_silu_f16)
# (tokens, M): a 128- or 256-row tile spans several images (16: five images in 80 rows), exactly one or two (64: three images, a ragged tile), half of one
# (256: two images in 512 rows).  Every M leaves the last tile ragged for the 128- and 256-row kernels alike, or fills it exactly (512).
KERNEL_ROWS = [(16, 5 * 16), (64, 3 * 64), (256, 2 * 256)]
KERNEL_NS = (64, 192)
KERNEL_KS = (64, 256)
KERNEL_SELECTIONS = (1, 4, 5, 6, 0)  # every selection the chooser can give a row-major linear (0: automatic, the 128x128 kernel at these sizes)
KERNEL_LAYOUTS = ("dense", "narrow")  # narrow: ldc % 8 == 4, the 8-byte-store path through a real ldc
VEC_PAD = 4  # vec rows are N + 4 floats apart in the strided layout (vec_stride % 4 == 0)


def kernel_shapes():
    return [(tokens, M, N, K) for tokens, M in KERNEL_ROWS for N in KERNEL_NS for K in KERNEL_KS]


def _gc():
    import gemm_exact_cases as gc

    return gc


def resid_vec_int_case(tokens, M, N, K):
    """Integer-valued operands, residual and vec: (acc + bias + resid + vec[m // tokens]) is an integer below 2048 with every partial sum exact in fp32, so the
    kernel must return it -- and half of it, scale 0.5 -- bit for bit (gemm_exact_cases.py: why integers)."""
    from types import SimpleNamespace

    gc = _gc()
    c = gc.linear_case(M, N, K)
    vec = gc.randint(torch.Generator().manual_seed(3 * M + N + K), (M // tokens, N), 32)
    ref = c.ref + vec.repeat_interleave(tokens, 0)
    assert int(ref.abs().max()) <= gc.CAP16
    return SimpleNamespace(M=M, N=N, K=K, tokens=tokens, A=c.A, W=c.W, bias=c.bias, resid=c.resid, vec=vec, ref=ref, ref_novec=c.ref)


def resid_vec_gauss_case(tokens, M, N, K, scale):
    """Gaussian fp16 operands and residual, fp32 bias and vec, against float64 per element:
        |got - ref| <= scale (K + 5) 2^-23 (|A| |W|^T + |bias| + |vec| + |resid|) + 2^-11 |ref| + 2^-25.
    K exact products; K accumulations, bias + vec, that sum onto the accumulator, the residual, the scale: K + 4 roundings of at most 2^-24 relative to a
    partial sum the magnitude sum bounds -- K + 5 with 2^-23 leaves the factor two gemm_exact_cases.gauss_case leaves; then ONE fp16 rounding."""
    from types import SimpleNamespace

    g = torch.Generator().manual_seed(17 + tokens + M + N + K)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias, vec = torch.randn(N, generator=g) * 0.1, torch.randn(M // tokens, N, generator=g)
    resid = torch.randn(M, N, generator=g).half()
    vr = vec.double().repeat_interleave(tokens, 0)
    ref = (A.double() @ W.double().t() + bias.double() + resid.double() + vr) * scale
    mag = A.double().abs() @ W.double().abs().t() + bias.double().abs() + resid.double().abs() + vr.abs()
    bound = abs(scale) * (K + 5) * 2.0 ** -23 * mag + 2.0 ** -11 * ref.abs() + 2.0 ** -25
    return SimpleNamespace(M=M, N=N, K=K, tokens=tokens, A=A, W=W, bias=bias, resid=resid, vec=vec, scale=scale, ref=ref, bound=bound)


def silu_case(M, N, K):
    """Gaussian operands with a pre-activation of standard deviation ~2 (both tails of SiLU, its minimum near -1.28 and the linear range), against
    silu64(acc64 + bias) per element:
        bound = 1.1 (K + 2) 2^-23 (|A| |W|^T + |bias|)      the fp32 accumulation error of the pre-activation (gauss_case) through |silu'| <= 1.0999
              + (|x| + 4) 2^-23 |ref|                        exp(-x) = 2^(-x log2 e): the fp32 rounding of the argument costs |x| 2^-24 relative, the
                                                             v_exp_f32, the 1 + e, the v_rcp_f32 and the product about an ulp each
              + 2^-11 (1 + 2^-9) |ref| + 2^-25               ONE rounding to fp16 (of a value already off by the terms above), the subnormal floor."""
    from types import SimpleNamespace

    g = torch.Generator().manual_seed(29 + M + N + K)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (4.0 * torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias = torch.randn(N, generator=g) * 0.5
    pre = A.double() @ W.double().t() + bias.double()
    mag = A.double().abs() @ W.double().abs().t() + bias.double().abs()
    ref = silu64(pre)
    bound = 1.1 * (K + 2) * 2.0 ** -23 * mag + (pre.abs() + 4) * 2.0 ** -23 * ref.abs() + 2.0 ** -11 * (1 + 2.0 ** -9) * ref.abs() + 2.0 ** -25
    return SimpleNamespace(M=M, N=N, K=K, A=A, W=W, bias=bias, pre=pre, ref=ref, bound=bound, gelu=gelu_tanh64(pre))
