"""EDM-style ADM UNet (``DhariwalUNet``), MI355X-native -- drop-in for the ``model_type == "adm"`` and ``"adm_context"`` branches of
/root/reference/models/EDM.py (``DhariwalUNet`` :716-861, ``UNetBlock`` :188-292, ``get_edm_network`` :864-939): the
backbone of ``test_args/{bed,ffhq,imnet}_adm.txt`` (USE_ORIGIN_ADM=false), including its own ``forward_with_cfg``.

Same constructor arguments and parameter/buffer names (``map_layer0/1``, ``map_label``, ``enc.<res>x<res>_{conv,down,block<i>}``,
``dec.<res>x<res>_{in0,in1,up,block<i>}``, ``out_norm``, ``out_conv``, the ``resample_filter`` buffers of up/down convolutions), so
reference checkpoints load with ``strict=True``.  The forward is sequenced on the host over the same NHWC-fp16 building blocks of
liblfm_hip.so as the origin-ADM UNet (``lfm_amd/models/unet.py``):

* ``Conv2d(up=True)`` with the [1,1] filter is a nearest-2x upsample followed by the 3x3 convolution -> one implicit-GEMM launch
  (mode 1); ``Conv2d(down=True)`` is a 2x2 mean (``lfm_avgpool2_f16``) followed by the 3x3 convolution (EDM.py:96-125);
* ``silu(addcmul(shift, norm1(x), scale + 1))`` (EDM.py:266-269) is the FiLM GroupNorm of ``lfm_groupnorm_f16``;
* attention: the reference's qkv channel order is [head][ch][q,k,v] (``reshape(N*heads, ch, 3, -1).unbind(2)``, EDM.py:277-281);
  the rows of ``qkv.weight`` are permuted ONCE at pack time into [head][q|k|v][ch], which is what ``lfm_attention_small_f16`` reads;
* the class embedding ``map_label(one_hot(y))`` (no bias) is a column lookup of ``map_label.weight``; the label dropped for the
  unconditional half under CFG (``drop_half_label``, EDM.py:825-826) is an extra all-zero row.

Built: ``augment_dim=0``, channels that are multiples of 64 (the implicit-GEMM contract); ``use_context`` either way.

``use_context=True`` (``model_type == "adm_context"``, reference :295-483, :754-756, :820-829, :923-938): ``map_label`` is the DiT ``LabelEmbedder``
(``map_label.embedding_table.weight``, ``label_dim + 1`` rows under label dropout); its output is NOT added to ``emb`` -- it is the ``context`` of every
block, and ``emb`` is the time embedding alone.  Every block is a ``UNetBlockWithContext``: the conv / FiLM / conv / skip part of ``UNetBlock`` without
attention of its own, then, where ``attention=True``, a ``TransformerBlock`` -- ``x = attn1(norm1(x)) + x; x = attn2(norm2(x), context) + x;
x = ff(norm3(x)) + x`` with EDM GroupNorms, ``C // 64`` heads, separate 1x1 ``q`` / ``k`` / ``v`` convolutions and a ``Linear -> SiLU -> Linear`` feed-forward.

* ``attn2`` has exactly ONE key (the context becomes ``[N, emb, 1, 1]``), and a softmax over one finite score is exactly 1: its output is
  ``proj.W (v.W ctx[n] + v.b) + proj.b`` at every pixel, independent of x, ``norm2``, ``q`` and ``k``.  That vector depends on the label only, so it is
  tabulated over the label table at pack time (float64 on the host, fp32 on the device, all blocks side by side: ``pack_context_tables``); one
  ``lfm_gather_rows_f32`` per forward takes the batch's rows.  ``attn2.q``, ``attn2.k`` and ``norm2`` are parameters (a reference ``state_dict`` loads with
  ``strict=True``) that the arithmetic never reads.  The identity needs finite scores.
* the three ``attn1`` convolutions are packed as one qkv weight, rows ``[head][q | k | v][ch]``; ``attn1.proj`` runs through ``lfm_linear_resid_vec_f16``,
  whose epilogue ``(acc + bias + x + u[m / tokens]) * scale`` performs both residual sums; ``ff.layer0`` through ``lfm_linear_silu_f16``; ``ff.layer1``
  through the existing residual linear (``HipUNetHost._transformer``).
* labels are required (``y=None`` and ``label_dim=0`` are refused: the reference crashes there) and validated on the host against the table's rows
  before anything is enqueued.  ``forward_with_cfg`` passes ``y`` through untouched: the reference ignores ``drop_half_label`` under ``use_context``, so the
  second half is conditioned on whatever ``y[N/2:]`` holds.  The drivers pass class 0 there for every non-DiT model, as the reference's do (not the extra
  row ``label_dim`` that label dropout trains); a caller who wants that row passes it.

``SongUNet`` (``model_type == "ddpm++"``, reference :532-706) is built for the DDPM++ settings -- positional embedding, standard encoder and
decoder, the [1,1] resample filter, ``channel_mult_noise=1`` -- on the same host-sequenced ops (``_EDMUNet`` holds what the two classes share).  What
differs from the ADM: the mapping network (``lfm_song_embed``: [sin | cos] table with endpoint, the label term with a bias added BEFORE the first linear, a
SiLU after the second), the non-adaptive FiLM ``silu(norm1(x + affine(emb)))`` (``lfm_add_image_vec_f16`` + GroupNorm), one attention head over the whole
width (at most 256 channels: the streamed attention kernel's limit), a 1x1 skip convolution after every resample (``resample_proj``), and
``skip_scale = sqrt(0.5)`` on both residual sums, applied in fp32 by the scaled epilogues (``lfm_conv3x3_scaled_f16_ws``, ``lfm_linear_scaled_f16``,
``lfm_linear2_scaled_f16``).  It has no ``forward_with_cfg``, as in the reference.

The other preset of the class, NCSN++ (``model_type == "ncsn++"``, reference :865-884: ``embedding_type="fourier"``, ``channel_mult_noise=2``,
``encoder_type="residual"``, ``decoder_type="standard"``, ``resample_filter=[1,3,3,1]``), is built as a whole; every mixed combination, the two ``skip``
types and ``augment_dim != 0`` stay refused by name.  What it adds to DDPM++:

* the [1,3,3,1] filter in ``Conv2d(up / down)`` (:120-127): ``lfm_fir_down2_f16`` / ``lfm_fir_up2_f16`` on both branches of a resampling block, the
  3x3 convolution in mode 0 (the fused nearest-2x of mode 1 belongs to the [1,1] filter);
* the residual encoder (:611-621, :685-686): after every ``down`` block ``x = skips[-1] = aux = (x + aux_residual(aux)) / sqrt(2)``, where
  ``aux_residual`` is ``Conv2d(kernel=3, down=True, fused_resample=True)`` -- the convolution at PADDING 2, then the filter at stride 2 without padding,
  the bias after the filter (:116-118, :130-131).  Here: a zero-border copy, the existing pad-1 convolution on the (H+2) x (W+2) map
  (``lfm_conv3x3_in_f32`` for the first one, whose input is the fp32 NCHW network input), and ``lfm_fir_down2_f16(pad=0)`` whose epilogue adds the bias
  and the block's output and scales by sqrt(1/2) (``_conv_pad2_fir_down``);
* the Fourier mapping network (:512-522): ``lfm_fourier_embed`` on the ``map_noise.freqs`` buffer, ``noise_channels = 2 * model_channels`` wide.

``get_edm_network`` reads ``config.num_blocks`` for this preset, as the reference does; neither its parsers nor the drivers here have such a flag, so
the preset is reached through ``create_network`` / ``SongUNet`` from code, and the drivers keep refusing ``--model_type ncsn++`` by name (the two
driver files, ``test_flow_latent.py`` and ``test_flow_latent_ddp.py``, are deliberately left byte for byte as they were: a ``--num_blocks`` flag there is a
change of its own).
"""
from functools import partial

import numpy as np
import torch
import torch.nn as nn

from .. import hip
from ._unet_host import HipUNetHost, f16, f32, pack_conv1, pack_conv3, pack_gn, pack_context_tables, pack_qkv_separate, stack_rows
from .DiT import LabelEmbedder


def _weight_init(shape, mode, fan_in, fan_out):  # EDM.py:27-36
    if mode == "xavier_uniform":
        return np.sqrt(6 / (fan_in + fan_out)) * (torch.rand(*shape) * 2 - 1)
    if mode == "xavier_normal":
        return np.sqrt(2 / (fan_in + fan_out)) * torch.randn(*shape)
    if mode == "kaiming_uniform":
        return np.sqrt(3 / fan_in) * (torch.rand(*shape) * 2 - 1)
    if mode == "kaiming_normal":
        return np.sqrt(1 / fan_in) * torch.randn(*shape)
    raise ValueError(f'Invalid init mode "{mode}"')


class Linear(nn.Module):  # EDM.py:43-56 (parameter container)
    def __init__(self, in_features, out_features, bias=True, init_mode="kaiming_normal", init_weight=1, init_bias=0):
        super().__init__()
        self.in_features, self.out_features = in_features, out_features
        kw = dict(mode=init_mode, fan_in=in_features, fan_out=out_features)
        self.weight = nn.Parameter(_weight_init([out_features, in_features], **kw) * init_weight)
        self.bias = nn.Parameter(_weight_init([out_features], **kw) * init_bias) if bias else None


class Conv2d(nn.Module):  # EDM.py:63-98 (parameter container)
    reads_network_input = False  # set on the first aux_residual of an NCSN++ encoder: its input is the fp32 NCHW network input, not an fp16 NHWC map

    def __init__(self, in_channels, out_channels, kernel, bias=True, up=False, down=False, resample_filter=(1, 1), fused_resample=False,
                 init_mode="kaiming_normal", init_weight=1, init_bias=0):
        assert not (up and down)
        super().__init__()
        self.in_channels, self.out_channels, self.up, self.down, self.kernel = in_channels, out_channels, up, down, kernel
        kw = dict(mode=init_mode, fan_in=in_channels * kernel * kernel, fan_out=out_channels * kernel * kernel)
        self.weight = nn.Parameter(_weight_init([out_channels, in_channels, kernel, kernel], **kw) * init_weight) if kernel else None
        self.bias = nn.Parameter(_weight_init([out_channels], **kw) * init_bias) if kernel and bias else None
        if tuple(resample_filter) not in ((1, 1), (1, 3, 3, 1)):
            raise NotImplementedError("only the [1,1] (DhariwalUNet, DDPM++) and [1,3,3,1] (NCSN++) resample filters are built")
        if fused_resample and not (down and kernel == 3 and tuple(resample_filter) == (1, 3, 3, 1)):
            raise NotImplementedError("fused_resample is built for the 3x3 down convolution under the [1,3,3,1] filter only (NCSN++'s aux_residual)")
        self.fir = tuple(resample_filter) == (1, 3, 3, 1)  # the 4-tap kernels (lfm_fir_down2_f16 / lfm_fir_up2_f16) instead of the 2x2 mean / nearest 2x
        self.fused_resample = fused_resample
        f = torch.as_tensor(resample_filter, dtype=torch.float32)
        f = f.ger(f).unsqueeze(0).unsqueeze(1) / f.sum().square()
        self.register_buffer("resample_filter", f if up or down else None)


class GroupNorm(nn.Module):  # EDM.py:139-151
    def __init__(self, num_channels, num_groups=32, min_channels_per_group=4, eps=1e-5):
        super().__init__()
        self.num_groups = min(num_groups, num_channels // min_channels_per_group)
        self.eps = eps
        self.weight = nn.Parameter(torch.ones(num_channels))
        self.bias = nn.Parameter(torch.zeros(num_channels))


class FourierEmbedding(nn.Module):  # EDM.py:512-522 (buffer container: ``map_noise.freqs`` of an NCSN++ state dict)
    def __init__(self, num_channels, scale=16):
        super().__init__()
        self.register_buffer("freqs", torch.randn(num_channels // 2) * scale)


class UNetBlock(nn.Module):  # EDM.py:188-292 (parameter container)
    def __init__(self, in_channels, out_channels, emb_channels, up=False, down=False, attention=False, num_heads=None,
                 channels_per_head=64, dropout=0, skip_scale=1, eps=1e-5, resample_filter=(1, 1), resample_proj=False, adaptive_scale=True, init=None,
                 init_zero=None, init_attn=None, scaled_epilogue=False):
        super().__init__()
        init, init_zero = init or {}, init_zero or dict(init_weight=0)
        self.in_channels, self.out_channels, self.up, self.down = in_channels, out_channels, up, down
        self.num_heads = 0 if not attention else (num_heads if num_heads is not None else out_channels // channels_per_head)
        self.skip_scale, self.eps, self.adaptive_scale = float(skip_scale), eps, adaptive_scale
        if skip_scale != 1 and not scaled_epilogue:  # only SongUNet sequences its residual sums over the scaled epilogues
            raise NotImplementedError("skip_scale != 1 is built for SongUNet only (DhariwalUNet uses 1)")
        self.norm0 = GroupNorm(in_channels, eps=eps)
        self.conv0 = Conv2d(in_channels, out_channels, 3, up=up, down=down, resample_filter=resample_filter, **init)
        self.affine = Linear(emb_channels, out_channels * (2 if adaptive_scale else 1), **init)
        self.norm1 = GroupNorm(out_channels, eps=eps)
        self.conv1 = Conv2d(out_channels, out_channels, 3, **init_zero)
        self.skip = None
        if out_channels != in_channels or up or down:
            self.skip = Conv2d(in_channels, out_channels, 1 if resample_proj or out_channels != in_channels else 0, up=up, down=down,
                               resample_filter=resample_filter, **init)
        if self.num_heads:
            self.norm2 = GroupNorm(out_channels, eps=eps)
            self.qkv = Conv2d(out_channels, out_channels * 3, 1, **(init_attn if init_attn is not None else init))
            self.proj = Conv2d(out_channels, out_channels, 1, **init_zero)


class CrossAttention(nn.Module):  # EDM.py:370-406 (parameter container); context_channels=None: self-attention
    def __init__(self, query_channels, context_channels=None, num_heads=None, channels_per_head=64, init=None, init_zero=None, init_attn=None):
        super().__init__()
        init, init_zero = init or {}, init_zero or dict(init_weight=0)
        self.num_heads = num_heads if num_heads is not None else query_channels // channels_per_head
        context_channels = query_channels if context_channels is None else context_channels
        qkv_init = init_attn if init_attn is not None else init
        self.q = Conv2d(query_channels, query_channels, 1, **qkv_init)
        self.k = Conv2d(context_channels, query_channels, 1, **qkv_init)
        self.v = Conv2d(context_channels, query_channels, 1, **qkv_init)
        self.proj = Conv2d(query_channels, query_channels, 1, **init_zero)


class FeedForward(nn.Module):  # EDM.py:427-440 (parameter container): Linear(C, 4C) -> SiLU -> Linear(4C, C) on tokens
    def __init__(self, in_channels, out_channels=None, channel_mult=4, init=None):
        super().__init__()
        inner = int(in_channels * channel_mult)
        self.layer0 = Linear(in_channels, inner, **(init or {}))
        self.layer1 = Linear(inner, in_channels if out_channels is None else out_channels, **(init or {}))


class TransformerBlock(nn.Module):  # EDM.py:443-483 (parameter container; registration order = the reference's state-dict order)
    def __init__(self, in_channels, context_channels, num_heads=None, channels_per_head=64, eps=1e-5, init=None, init_zero=None, init_attn=None):
        super().__init__()
        kw = dict(num_heads=num_heads, channels_per_head=channels_per_head, init=init, init_zero=init_zero, init_attn=init_attn)
        self.attn1 = CrossAttention(in_channels, None, **kw)
        self.attn2 = CrossAttention(in_channels, context_channels, **kw)  # one key: only v and proj enter the arithmetic (module docstring)
        self.ff = FeedForward(in_channels, init=init)
        self.norm1 = GroupNorm(in_channels, eps=eps)
        self.norm2 = GroupNorm(in_channels, eps=eps)  # loaded, never read: attn2's output does not depend on its query
        self.norm3 = GroupNorm(in_channels, eps=eps)
        self.in_channels, self.eps = in_channels, eps


class UNetBlockWithContext(UNetBlock):  # EDM.py:295-367 (parameter container): UNetBlock without its own attention, then a TransformerBlock where attention=True
    def __init__(self, in_channels, out_channels, emb_channels, context_channels, up=False, down=False, attention=False, num_heads=None,
                 channels_per_head=64, **kw):
        super().__init__(in_channels, out_channels, emb_channels, up=up, down=down, attention=False, **kw)
        self.use_transformer = bool(attention)
        if self.use_transformer:
            self.transformer = TransformerBlock(out_channels, context_channels, num_heads=num_heads, channels_per_head=channels_per_head, eps=self.eps,
                                                init=kw.get("init"), init_zero=kw.get("init_zero"), init_attn=kw.get("init_attn"))


class _EDMUNet(HipUNetHost):
    """What DhariwalUNet and SongUNet share on top of the UNets' host layer (``_unet_host.py``): what is packed, the host-sequenced UNetBlock and the encoder /
    decoder walk.  A subclass builds the parameter tree and provides ``_out_modules`` (the output GroupNorm and convolution), ``_pack_mapping`` and ``_embed``
    (its mapping network)."""

    _what = "EDM UNet"

    # ---- packing ------------------------------------------------------------------------------------------------------
    def _pack_blocks(self, P, dev):
        out_norm, out_conv = self._out_modules()
        aff, ctx = {}, {}
        for group in (self.enc, self.dec):
            pre = "enc." if group is self.enc else "dec."
            for name, b in group.items():
                if b is out_norm or b is out_conv:  # SongUNet keeps its output layers inside `dec` (aux_norm / aux_conv): packed by the host layer
                    continue
                if isinstance(b, Conv2d) and b.fused_resample:  # NCSN++'s aux_residual: (weights, a zero bias for the convolution, the bias added AFTER the filter)
                    if b.reads_network_input:  # fp32 NCHW in: the layout lfm_conv3x3_in_f32 reads
                        P[pre + name] = (f32(b.weight, dev), torch.zeros(b.out_channels, device=dev), f32(b.bias, dev))
                    else:
                        P[pre + name] = (pack_conv3(b, dev)[0], None, f32(b.bias, dev))
                    continue
                if isinstance(b, Conv2d):
                    P[pre + name] = (f32(b.weight, dev), f32(b.bias, dev))
                    continue
                d = dict(gn0=pack_gn(b.norm0, dev), c0=pack_conv3(b.conv0, dev), gn1=pack_gn(b.norm1, dev), c1=pack_conv3(b.conv1, dev),
                         skip=pack_conv1(b.skip, dev) if (b.skip is not None and b.skip.weight is not None) else None)
                if b.num_heads:
                    C, ch = b.out_channels, b.out_channels // b.num_heads
                    # reference row (head, c, which) -> our row (head, which, c)
                    perm = torch.arange(3 * C).reshape(b.num_heads, ch, 3).permute(0, 2, 1).reshape(-1)
                    d.update(gn_attn=pack_gn(b.norm2, dev), qkv=(f16(b.qkv.weight.reshape(3 * C, C)[perm], dev), f32(b.qkv.bias[perm], dev)),
                             proj=pack_conv1(b.proj, dev))
                if getattr(b, "use_transformer", False):  # adm_context: the device half of the TransformerBlock; its attn2 goes into the context table below
                    tb = b.transformer
                    d["tf"] = dict(gn1=pack_gn(tb.norm1, dev), qkv=pack_qkv_separate(tb.attn1, dev), proj=pack_conv1(tb.attn1.proj, dev), gn3=pack_gn(tb.norm3, dev),
                                   ff0=(f16(tb.ff.layer0.weight, dev), f32(tb.ff.layer0.bias, dev)), ff1=(f16(tb.ff.layer1.weight, dev), f32(tb.ff.layer1.bias, dev)))
                    ctx[pre + name] = tb.attn2
                P[pre + name] = d
                aff[pre + name] = (f16(b.affine.weight, dev), f32(b.affine.bias, dev))
        P["aff_all"] = stack_rows(aff)  # every block's `affine` projection of the embedding (EDM.py:263-265)
        # every TransformerBlock's attn2 as a table over the label rows, stacked column-wise (None: no context model)
        P["ctx_all"] = pack_context_tables(ctx, self.map_label.embedding_table.weight, dev) if ctx else None
        self._pack_mapping(P, dev)

    # ---- blocks -----------------------------------------------------------------------------------------------------------
    def _block(self, name, b, x, N, H, W, film_all, ctx_all=None):
        """UNetBlock.forward (EDM.py:258-292).  Returns (out, H, W).  `x` may be the pair (h, skip) of a decoder block: its channel concat is then read in place
        by the block's two consumers -- the first GroupNorm and the 1x1 skip convolution -- as in the origin-ADM UNet (round 6; the concat kernel was 2 % of an
        evaluation at the ffhq_adm size)."""
        p = self._packed[name]
        Cin, Cout, eps, ss = b.in_channels, b.out_channels, b.eps, b.skip_scale
        g0, g1 = b.norm0.num_groups, b.norm1.num_groups  # min(32, C // 4) (EDM.py:139-143)
        pair = None
        if isinstance(x, tuple):
            if b.down or b.up or p["skip"] is None or x[0].shape[1] % 64 or x[1].shape[1] % 8:
                x = self._cat(x)  # resampled / identity-skip inputs need the tensor itself
            else:
                pair = x
        orig = x
        if pair is not None:
            t = self._gn2(pair[0], pair[1], N, H * W, p["gn0"], None, True, g0, eps)
        else:
            t = self._gn(x, N, H * W, Cin, p["gn0"], None, True, g0, eps)
        fir = b.conv0.fir  # the [1,3,3,1] filter (NCSN++): lfm_fir_down2_f16 / lfm_fir_up2_f16 on both branches, the convolution in mode 0
        if b.down:  # Conv2d(down=True): a 2x2 mean (or the 4-tap filter), then the 3x3 convolution (EDM.py:96-125), on both branches
            H, W = H // 2, W // 2
            t = self._resample(t, N, H, W, Cin, False, fir)
            orig = self._resample(orig, N, H, W, Cin, False, fir)
        elif b.up:  # Conv2d(up=True): nearest 2x fused into the convolution (the [1,1] filter only)
            H, W = H * 2, W * 2
            if fir:
                t = self._resample(t, N, H, W, Cin, True, True)
        h = self._conv(t, p["c0"], N, H, W, Cin, Cout, mode=1 if b.up and not fir else 0)
        fo, fw = self._packed["aff_all"][2][name]
        film = film_all[:, fo:fo + fw]  # fp32 [N, 2*Cout] = [scale | shift] (or [N, Cout]): this block's columns of the one affine GEMM (row stride = all blocks' columns)
        if b.adaptive_scale:
            t = self._gn(h, N, H * W, Cout, p["gn1"], film, True, g1, eps)
        else:  # silu(norm1(x + params)) (EDM.py:270): the statistics are those of the sum
            hs = self._add_image_vec(h, film, N, H * W, Cout)
            t = self._gn(hs, N, H * W, Cout, p["gn1"], None, True, g1, eps)
        if b.up:  # skip(orig): nearest 2x upsample of the input (conv_transpose with the all-ones 2x2 filter), then the 1x1 convolution where there is one
            orig = self._resample(orig, N, H, W, Cin, True, fir)
        if pair is not None:
            skip = self._linear2(pair[0], pair[1], p["skip"])
        else:
            skip = orig if p["skip"] is None else self._linear(orig, p["skip"])
        x = self._conv(t, p["c1"], N, H, W, Cout, Cout, resid=skip, scale=ss)  # (acc + bias + resid) * skip_scale in the epilogue
        if b.num_heads:
            del t  # dead from here on: its block of a captured graph's memory pool goes to the attention's tensors
            x = self._attention(x, p, N, H * W, b.num_heads, Cout, b.norm2.num_groups, eps, ss)
        elif getattr(b, "use_transformer", False):  # UNetBlockWithContext (EDM.py:364-366): x = transformer(x, context) * skip_scale
            del t
            tb = b.transformer
            co, cw = self._packed["ctx_all"][1][name]
            x = self._transformer(x, p["tf"], ctx_all[:, co:co + cw], N, H * W, tb.attn1.num_heads, Cout, tb.norm1.num_groups, tb.eps, ss)
        return x, H, W

    # ---- forward ----------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _forward(self, noise_labels, x, y, drop_half_label):
        x, t = self._prologue(noise_labels, x, "noise_labels")
        P = self._packed
        N, Cin, H, W = x.shape
        emb_f16 = self._embed(t, N, y, drop_half_label, x.device)  # fp16 [N, E]: what every block's `affine` reads
        film_all = hip.gemm_f16(emb_f16, P["aff_all"][0], P["aff_all"][1], epilogue=2)  # fp32 [N, all blocks' affine columns]
        # adm_context: the N label rows of the stacked context table, fp32 [N, all TransformerBlocks' channels]; each block reads its column slice
        ctx_all = hip.gather_rows(P["ctx_all"][0], y) if P["ctx_all"] is not None else None
        skips, h, aux = [], None, x  # aux: the residual encoder's second stream (NCSN++), the network input until the first aux_residual
        for name, b in self.enc.items():
            if name.endswith("_aux_residual"):  # x = skips[-1] = aux = (x + aux_residual(aux)) / sqrt(2) (EDM.py:685-686): aux is one level up, 2H x 2W
                h = skips[-1] = aux = self._conv_pad2_fir_down(aux, P["enc." + name], N, 2 * H, 2 * W, b.in_channels, b.out_channels, h, float(np.sqrt(0.5)),
                                                                   nchw_f32=b.reads_network_input)
                continue
            if isinstance(b, Conv2d):
                h = self._conv_in(x, P["enc." + name], N, H, W, Cin)
            else:
                h, H, W = self._block("enc." + name, b, h, N, H, W, film_all, ctx_all)
            skips.append(h)
        for name, b in self.dec.items():
            if not isinstance(b, UNetBlock):  # SongUNet's aux_norm / aux_conv: the output layers below
                continue
            if h.shape[1] != b.in_channels:
                s = skips.pop()
                h = (h, s)  # torch.cat([x, skips.pop()], dim=1) (EDM.py:840-842): consumed in place by the block where its shape allows it
            h, H, W = self._block("dec." + name, b, h, N, H, W, film_all, ctx_all)
        out_norm = self._out_modules()[0]
        return self._out(h, N, H, W, out_norm.num_groups, out_norm.eps)


class DhariwalUNet(_EDMUNet):
    _what = "DhariwalUNet"

    def __init__(self, img_resolution, in_channels, out_channels, label_dim=0, augment_dim=0, model_channels=192, channel_mult=(1, 2, 3, 4),
                 channel_mult_emb=4, num_blocks=3, attn_resolutions=(32, 16, 8), dropout=0.10, label_dropout=0, use_context=False):
        super().__init__()
        self._init_host_state()
        if augment_dim:
            raise NotImplementedError("augment_dim is not used by the sampling path and is not built")
        if use_context and not label_dim:  # the reference builds it and crashes in forward (map_label is None there, and it is called)
            raise ValueError("DhariwalUNet(use_context=True) needs label_dim > 0: the context IS the label embedding")
        self.label_dim, self.label_dropout, self.use_context = label_dim, label_dropout, bool(use_context)
        self.img_resolution, self.in_channels, self.out_channels, self.model_channels = img_resolution, in_channels, out_channels, model_channels
        emb_channels = model_channels * channel_mult_emb
        self.emb_channels = emb_channels
        init = dict(init_mode="kaiming_uniform", init_weight=np.sqrt(1 / 3), init_bias=np.sqrt(1 / 3))
        init_zero = dict(init_mode="kaiming_uniform", init_weight=0, init_bias=0)
        bk = dict(emb_channels=emb_channels, channels_per_head=64, dropout=dropout, init=init, init_zero=init_zero)
        self.map_layer0 = Linear(model_channels, emb_channels, **init)
        self.map_layer1 = Linear(emb_channels, emb_channels, **init)
        if use_context:  # EDM.py:754-756: the DiT label embedder (label_dim + 1 rows under label_dropout), its output the CONTEXT of every block, not a term of emb
            self.map_label = LabelEmbedder(label_dim, emb_channels, label_dropout)
            UNetBlock_ = partial(UNetBlockWithContext, context_channels=emb_channels)
        else:
            self.map_label = Linear(label_dim, emb_channels, bias=False, init_mode="kaiming_normal", init_weight=np.sqrt(label_dim)) if label_dim else None
            UNetBlock_ = UNetBlock
        self.enc = nn.ModuleDict()
        cout = in_channels
        for level, mult in enumerate(channel_mult):
            res = img_resolution >> level
            if level == 0:
                cin, cout = cout, model_channels * mult
                self.enc[f"{res}x{res}_conv"] = Conv2d(cin, cout, 3, **init)
            else:
                self.enc[f"{res}x{res}_down"] = UNetBlock_(cout, cout, down=True, **bk)
            for idx in range(num_blocks):
                cin, cout = cout, model_channels * mult
                self.enc[f"{res}x{res}_block{idx}"] = UNetBlock_(cin, cout, attention=(res in attn_resolutions), **bk)
        skips = [b.out_channels for b in self.enc.values()]
        self.dec = nn.ModuleDict()
        for level, mult in reversed(list(enumerate(channel_mult))):
            res = img_resolution >> level
            if level == len(channel_mult) - 1:
                self.dec[f"{res}x{res}_in0"] = UNetBlock_(cout, cout, attention=True, **bk)
                self.dec[f"{res}x{res}_in1"] = UNetBlock_(cout, cout, **bk)
            else:
                self.dec[f"{res}x{res}_up"] = UNetBlock_(cout, cout, up=True, **bk)
            for idx in range(num_blocks + 1):
                cin = cout + skips.pop()
                cout = model_channels * mult
                self.dec[f"{res}x{res}_block{idx}"] = UNetBlock_(cin, cout, attention=(res in attn_resolutions), **bk)
        self.out_norm = GroupNorm(cout)
        self.out_conv = Conv2d(cout, out_channels, 3, **init_zero)

    def _out_modules(self):
        return self.out_norm, self.out_conv

    def _pack_mapping(self, P, dev):
        P["time"] = tuple(f32(t, dev) for t in (self.map_layer0.weight, self.map_layer0.bias, self.map_layer1.weight, self.map_layer1.bias))
        if self.use_context:  # the label embedding is the context (P["ctx_all"], packed with the blocks): emb is the time embedding alone
            P["label"] = None
        elif self.map_label is not None:  # [label_dim + 1, E]: column lookup + one all-zero row for the dropped label
            P["label"] = torch.cat([f32(self.map_label.weight, dev).t(), torch.zeros(1, self.emb_channels, device=dev)], 0).contiguous()
        else:
            P["label"] = None

    def _embed(self, t, N, y, drop_half_label, dev):
        yy = None  # (context mode: P["label"] is None -- the labels went into the context rows, and drop_half_label is ignored as in the reference, EDM.py:821-829)
        if self._packed["label"] is not None and y is not None:
            yy = y.to(dev, torch.long).clone()
            if drop_half_label:
                yy[N // 2:] = self.label_dim  # the all-zero row (EDM.py:825-826)
        return self._time_embed(t, N, yy, self.model_channels, self.emb_channels)

    def forward(self, noise_labels, x, y=None, augment_labels=None, drop_half_label=False, **kwargs):
        """v = model(t, x, y) (EDM.py:808-845)."""
        return self._forward(noise_labels, x, self._context_labels(y, x), drop_half_label)

    def _context_labels(self, y, x):
        """Context mode: the labels as the gather kernel reads them (int64 on x's device), validated against the embedding table's rows on the host before
        anything is enqueued; y=None is refused (the reference calls map_label(None) and crashes).  Otherwise y as it came."""
        if not self.use_context:
            return y
        if y is None:
            raise ValueError("DhariwalUNet(use_context=True).forward needs labels y: the context of every TransformerBlock is their embedding")
        yy = y.to(x.device, torch.long).contiguous()
        if yy.numel() != x.shape[0]:
            raise ValueError(f"DhariwalUNet(use_context=True): {yy.numel()} labels for a batch of {x.shape[0]}")
        hip.check_labels(yy, self.map_label.embedding_table.num_embeddings, self._what)
        return yy

    def _cfg_coef(self, cfg_scale, dev):
        """[s, 1 - s] on the device, made once per (scale, device): a stream capture refuses the host-to-device copy of a fresh one (the captured solver
        warms up before it captures, so the buffer exists by then).  Twins share the table: it is read-only."""
        table = self.__dict__.setdefault("_cfg_coefs", {})
        key = (float(cfg_scale), dev)
        if key not in table:
            table[key] = torch.tensor([cfg_scale, 1.0 - cfg_scale], device=dev)  # uncond + s*(cond - uncond)
        return table[key]

    def forward_with_cfg(self, noise_labels, x, y=None, augment_labels=None, cfg_scale=1.0, **kwargs):
        """EDM.py:847-861: x[:N/2] evaluated with labels y (first half) and with the label dropped (second half).  In context mode the reference's
        ``drop_half_label`` is ignored (:821-829): the second half is conditioned on whatever y[N/2:] holds -- the caller's null label (the drivers pass class 0
        for every non-DiT model, as the reference's do; the extra row ``label_dim`` is what label dropout trained) -- and y passes through untouched."""
        y = self._context_labels(y, x)
        n2 = len(x) // 2
        xin = x.contiguous().float().clone()
        xin[n2:].copy_(xin[:n2])  # combined = cat([half, half])
        out = self._forward(noise_labels, xin, y, True)
        cond, uncond = out[:n2], out[n2:]
        coef = self._cfg_coef(cfg_scale, x.device)
        res = torch.empty_like(out)
        hip.lincomb(res[:n2], None, [cond, uncond], coef)
        hip.lincomb(res[n2:], None, [cond, uncond], coef)
        return res


class SongUNet(_EDMUNet):
    """DDPM++ and NCSN++ (reference EDM.py:532-706 as ``get_edm_network`` builds it for ``model_type == "ddpm++"``, :886-905, and ``"ncsn++"``, :865-884):
    exactly these two combinations of the five architecture settings; a mixed one is refused by the name of its first departure from DDPM++."""

    _what = "SongUNet"
    NCSNPP = dict(embedding_type="fourier", channel_mult_noise=2, encoder_type="residual", decoder_type="standard", resample_filter=(1, 3, 3, 1))

    def __init__(self, img_resolution, in_channels, out_channels, label_dim=0, augment_dim=0, model_channels=128, channel_mult=(1, 2, 2, 2),
                 channel_mult_emb=4, num_blocks=4, attn_resolutions=(16,), dropout=0.10, label_dropout=0, embedding_type="positional",
                 channel_mult_noise=1, encoder_type="standard", decoder_type="standard", resample_filter=(1, 1)):
        super().__init__()
        self._init_host_state()
        resample_filter = tuple(resample_filter)
        got_all = dict(embedding_type=embedding_type, channel_mult_noise=channel_mult_noise, encoder_type=encoder_type, decoder_type=decoder_type,
                       resample_filter=resample_filter)
        ncsnpp = got_all == self.NCSNPP  # the whole preset or none of it: nobody has a model of a mixed kind
        for what, got, built in (("embedding_type", embedding_type, "positional"), ("channel_mult_noise", channel_mult_noise, 1),
                                 ("encoder_type", encoder_type, "standard"), ("decoder_type", decoder_type, "standard"),
                                 ("resample_filter", resample_filter, (1, 1)), ("augment_dim", augment_dim, 0)):
            if got != built and not (ncsnpp and what != "augment_dim"):
                raise NotImplementedError(f"SongUNet: {what}={got!r} is not built; only the ddpm++ settings ({what}={built!r}) and the ncsn++ preset "
                                          "as a whole (SongUNet.NCSNPP) are")
        widths = [model_channels * m for m in channel_mult]
        if any(w % 64 for w in widths):
            raise NotImplementedError(f"SongUNet: channel counts {widths} must all be multiples of 64 (the implicit-GEMM convolutions' contract)")
        attn_widths = [w for level, w in enumerate(widths) if (img_resolution >> level) in attn_resolutions] + [widths[-1]]  # in0 always attends
        if max(attn_widths) > 256:
            raise NotImplementedError(f"SongUNet: attention is one head over the whole width, and {max(attn_widths)} channels exceed the 256 per head "
                                      "that the streamed attention kernel serves")
        if in_channels > 16 or out_channels > 4:
            raise NotImplementedError("SongUNet: at most 16 input and 4 output channels are built (the fp32 boundary convolutions)")
        self.label_dim, self.label_dropout = label_dim, label_dropout
        self.img_resolution, self.in_channels, self.out_channels, self.model_channels = img_resolution, in_channels, out_channels, model_channels
        emb_channels = model_channels * channel_mult_emb
        noise_channels = model_channels * channel_mult_noise
        self.emb_channels, self.noise_channels = emb_channels, noise_channels
        init = dict(init_mode="xavier_uniform")
        init_zero = dict(init_mode="xavier_uniform", init_weight=1e-5)
        init_attn = dict(init_mode="xavier_uniform", init_weight=np.sqrt(0.2))
        bk = dict(emb_channels=emb_channels, num_heads=1, dropout=dropout, skip_scale=np.sqrt(0.5), eps=1e-6, resample_filter=resample_filter,
                  resample_proj=True, adaptive_scale=False, init=init, init_zero=init_zero, init_attn=init_attn, scaled_epilogue=True)
        if ncsnpp:  # registered first, as in the reference: `map_noise.freqs` leads the state dict (the positional embedding has no buffer and no module here)
            self.map_noise = FourierEmbedding(noise_channels)
        self.map_label = Linear(label_dim, noise_channels, **init) if label_dim else None
        self.map_layer0 = Linear(noise_channels, emb_channels, **init)
        self.map_layer1 = Linear(emb_channels, emb_channels, **init)
        self.enc = nn.ModuleDict()
        cout = caux = in_channels
        for level, mult in enumerate(channel_mult):
            res = img_resolution >> level
            if level == 0:
                cin, cout = cout, model_channels
                self.enc[f"{res}x{res}_conv"] = Conv2d(cin, cout, 3, **init)
            else:
                self.enc[f"{res}x{res}_down"] = UNetBlock(cout, cout, down=True, **bk)
                if ncsnpp:  # encoder_type == "residual" (EDM.py:611-621): the first one reads the network input, every later one `cout` channels
                    self.enc[f"{res}x{res}_aux_residual"] = Conv2d(caux, cout, 3, down=True, resample_filter=resample_filter, fused_resample=True, **init)
                    self.enc[f"{res}x{res}_aux_residual"].reads_network_input = level == 1  # `aux` is the fp32 NCHW network input until the first one has run
                    caux = cout
            for idx in range(num_blocks):
                cin, cout = cout, model_channels * mult
                self.enc[f"{res}x{res}_block{idx}"] = UNetBlock(cin, cout, attention=(res in attn_resolutions), **bk)
        skips = [b.out_channels for name, b in self.enc.items() if "aux" not in name]
        self.dec = nn.ModuleDict()
        for level, mult in reversed(list(enumerate(channel_mult))):
            res = img_resolution >> level
            if level == len(channel_mult) - 1:
                self.dec[f"{res}x{res}_in0"] = UNetBlock(cout, cout, attention=True, **bk)
                self.dec[f"{res}x{res}_in1"] = UNetBlock(cout, cout, **bk)
            else:
                self.dec[f"{res}x{res}_up"] = UNetBlock(cout, cout, up=True, **bk)
            for idx in range(num_blocks + 1):
                cin = cout + skips.pop()
                cout = model_channels * mult
                self.dec[f"{res}x{res}_block{idx}"] = UNetBlock(cin, cout, attention=(idx == num_blocks and res in attn_resolutions), **bk)
            if level == 0:
                self.dec[f"{res}x{res}_aux_norm"] = GroupNorm(cout, eps=1e-6)
                self.dec[f"{res}x{res}_aux_conv"] = Conv2d(cout, out_channels, 3, **init_zero)

    @torch.no_grad()
    def redraw_small_(self, seed=4321, std=0.02):
        """Synthetic-weight runs (``--random_weights``): the "zero" convolutions are initialised at weight 1e-5, not 0, so the drivers' re-draw of all-zero
        tensors passes them by and the model would output ~6e-6.  Re-draw every tensor that small from seeded N(0, std), in name order."""
        g = torch.Generator().manual_seed(seed)
        for _, p in sorted(self.named_parameters()):
            if p.numel() and bool(p.any()) and float(p.abs().max()) < 1e-4:
                p.copy_(torch.randn(p.shape, generator=g) * std)
        self._packed = None
        self._gen += 1
        return self

    def _out_modules(self):
        r = self.img_resolution
        return self.dec[f"{r}x{r}_aux_norm"], self.dec[f"{r}x{r}_aux_conv"]

    def _pack_mapping(self, P, dev):
        P["time"] = tuple(f32(t, dev) for t in (self.map_layer0.weight, self.map_layer0.bias, self.map_layer1.weight, self.map_layer1.bias))
        # map_label(one_hot(y) * sqrt(L)) = sqrt(L) * W[:, y] + b: rows of W^T, the scale and the bias go to the kernel as they are (all fp32)
        P["label"] = (f32(self.map_label.weight, dev).t().contiguous(), f32(self.map_label.bias, dev)) if self.map_label is not None else None
        P["freqs"] = f32(self.map_noise.freqs, dev) if hasattr(self, "map_noise") else None  # NCSN++: the Fourier table instead of the positional one

    def _embed(self, t, N, y, drop_half_label, dev):
        P, E, F = self._packed, self.emb_channels, self.noise_channels
        lab, yy = None, None
        if P["label"] is not None and y is not None:  # y=None on a conditional model: the label term is left out (the label_dim=0 model on the same weights)
            lab, yy = P["label"], y.to(dev, torch.long).contiguous()
            hip.check_labels(yy, self.label_dim, "SongUNet")
        emb = torch.empty(N, E, device=dev)
        emb_f16 = torch.empty(N, E, device=dev, dtype=torch.float16)
        h1 = torch.empty(N, E, device=dev)
        tw = P["time"]
        rest = (hip.ptr(tw[0]), hip.ptr(tw[1]), hip.ptr(tw[2]), hip.ptr(tw[3]), hip.ptr(lab[0] if lab else None), hip.ptr(lab[1] if lab else None),
                float(np.sqrt(max(self.label_dim, 1))), hip.ptr(yy), self.label_dim, hip.ptr(h1), hip.ptr(emb), hip.ptr(emb_f16), N, F, E, hip.stream_ptr(dev))
        if P["freqs"] is not None:
            hip.check(hip.lib().lfm_fourier_embed(hip.ptr(t), t.numel(), hip.ptr(P["freqs"]), *rest), "lfm_fourier_embed")
        else:
            hip.check(hip.lib().lfm_song_embed(hip.ptr(t), t.numel(), *rest), "lfm_song_embed")
        return emb_f16

    def forward(self, noise_labels, x, y=None, augment_labels=None, **kwargs):
        """v = model(t, x, y) (EDM.py:663-706)."""
        return self._forward(noise_labels, x, y, False)


def get_edm_network(config):
    """Reference models/EDM.py:864-939: ``adm`` and ``adm_context`` -> DhariwalUNet (the latter with ``use_context=True``), ``ddpm++`` and ``ncsn++`` ->
    SongUNet, each with the reference's argument list."""
    common = dict(img_resolution=config.image_size // config.f, in_channels=config.num_in_channels, out_channels=config.num_out_channels,
                  label_dim=config.label_dim, augment_dim=0, model_channels=config.nf, channel_mult=config.ch_mult, channel_mult_emb=4,
                  attn_resolutions=config.attn_resolutions, dropout=config.dropout, label_dropout=config.label_dropout)
    if config.model_type in ("ddpm++", "ncsn++"):
        if config.model_type == "ddpm++":
            m = SongUNet(embedding_type="positional", channel_mult_noise=1, encoder_type="standard", decoder_type="standard", resample_filter=[1, 1],
                         num_blocks=config.num_res_blocks, **common)
        else:  # the reference reads config.num_blocks here (:875), not num_res_blocks, and no driver has such a flag
            if getattr(config, "num_blocks", None) is None:
                raise NotImplementedError("model_type 'ncsn++' needs config.num_blocks: the reference (models/EDM.py:875) reads that name, not "
                                          "num_res_blocks, and no parser sets it")
            m = SongUNet(num_blocks=config.num_blocks, **common, **SongUNet.NCSNPP)
        if getattr(config, "random_weights", False):
            m.redraw_small_()
        return m
    if config.model_type not in ("adm", "adm_context"):
        raise NotImplementedError(f"model_type {config.model_type!r} is not one of the reference's: adm, adm_context, ddpm++, ncsn++")
    return DhariwalUNet(num_blocks=config.num_res_blocks, use_context=config.model_type == "adm_context", **common)
