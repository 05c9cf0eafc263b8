"""Origin-ADM UNet velocity field, MI355X-native (drop-in for ``UNetModel`` of
/root/reference/models/guided_diffusion/unet.py:376-655, the backbone behind ``--use_origin_adm``).

Same constructor arguments, same parameter tree (``time_embed.{0,2}``, ``label_emb``, ``input_blocks.i.j.{in_layers.{0,2},
emb_layers.1,out_layers.{0,3},skip_connection,norm,qkv,proj_out,op}``, ``middle_block.{0,1,2}``, ``output_blocks.i.j...{conv}``,
``out.{0,2}``) so reference checkpoints load with ``strict=True``; same call contract ``model(t, x, y=None) -> v``.

The layer list is data-dependent, so the forward is sequenced here, on the host, over the NHWC-fp16 building blocks of
liblfm_hip.so (implicit-GEMM 3x3 convolutions incl. stride-2 / fused nearest-2x upsample, GroupNorm32 with the FiLM
scale-shift, small-T legacy attention, 1x1 convolutions with fused residual).  Graph-capturable; no PyTorch compute ops.

Built: ``use_scale_shift_norm=True`` (the sampler default, test_flow_latent.py:356), ``resblock_updown=False``,
``use_new_attention_order=False``, ``dims=2``, conv resampling -- i.e. every ``test_args/*_adm.txt`` with
``USE_ORIGIN_ADM=true``.  Other combinations raise ``NotImplementedError``.

``UNetModelAttn`` (unet.py:882-1205, ``--layout``) is the same network with SpatialTransformers (attention.py:243-280) at the attention positions: the two
classes share the tree builder, the packing, the ResBlock, the block body and the walk (``_ADMHost``) and differ in what stands at those positions and in the
``context`` argument.  Its cross-attention, LayerNorm and GEGLU are kernels of their own (csrc/unet_cross_attention_kernel.h, csrc/token_ops.h).
"""
import torch
import torch.nn as nn

from .. import hip
from ._unet_host import HipUNetHost, f16, f32, pack_conv1, pack_conv3, pack_gn, stack_rows


class GroupNorm32(nn.GroupNorm):  # nn.py:17-19 (fp32 statistics; ours accumulates in fp32 too)
    pass


def normalization(channels):
    return GroupNorm32(32, channels)


class Upsample(nn.Module):  # unet.py:73-100
    def __init__(self, channels, use_conv, out_channels=None):
        super().__init__()
        self.channels, self.out_channels, self.use_conv = channels, out_channels or channels, use_conv
        if not use_conv:
            raise NotImplementedError("Upsample without conv (conv_resample=False) is not built")
        self.conv = nn.Conv2d(self.channels, self.out_channels, 3, padding=1)


class Downsample(nn.Module):  # unet.py:103-128
    def __init__(self, channels, use_conv, out_channels=None):
        super().__init__()
        self.channels, self.out_channels, self.use_conv = channels, out_channels or channels, use_conv
        if not use_conv:
            raise NotImplementedError("Downsample by average pooling (conv_resample=False) is not built")
        self.op = nn.Conv2d(self.channels, self.out_channels, 3, stride=2, padding=1)


class _Resample(nn.Module):
    """Parameter-free Upsample / Downsample (use_conv=False) inside a ResBlock(up= / down=): nearest 2x / 2x2 average pool (unet.py:73-128)."""

    def __init__(self, channels, up):
        super().__init__()
        self.channels, self.up = channels, up


class ResBlock(nn.Module):  # unet.py:131-238
    def __init__(self, channels, emb_channels, dropout, out_channels=None, use_scale_shift_norm=False, up=False, down=False):
        super().__init__()
        self.channels, self.out_channels = channels, out_channels or channels
        self.use_scale_shift_norm = use_scale_shift_norm
        self.updown = up or down
        self.in_layers = nn.Sequential(normalization(channels), nn.SiLU(), nn.Conv2d(channels, self.out_channels, 3, padding=1))
        if self.updown:  # same attribute names as the reference (they hold no parameters)
            self.h_upd, self.x_upd = _Resample(channels, up), _Resample(channels, up)
        else:
            self.h_upd = self.x_upd = nn.Identity()
        self.emb_layers = nn.Sequential(nn.SiLU(), nn.Linear(emb_channels, 2 * self.out_channels if use_scale_shift_norm else self.out_channels))
        self.out_layers = nn.Sequential(normalization(self.out_channels), nn.SiLU(), nn.Dropout(p=dropout),
                                        nn.Conv2d(self.out_channels, self.out_channels, 3, padding=1))
        for p in self.out_layers[-1].parameters():  # zero_module (unet.py:198)
            p.detach().zero_()
        self.skip_connection = nn.Identity() if self.out_channels == channels else nn.Conv2d(channels, self.out_channels, 1)


class AttentionBlock(nn.Module):  # unet.py:241-287
    def __init__(self, channels, num_heads=1, num_head_channels=-1, use_new_attention_order=False):
        super().__init__()
        self.channels = channels
        self.use_new_attention_order = use_new_attention_order
        self.num_heads = num_heads if num_head_channels == -1 else channels // num_head_channels
        assert channels % self.num_heads == 0
        self.norm = normalization(channels)
        self.qkv = nn.Conv1d(channels, channels * 3, 1)
        self.proj_out = nn.Conv1d(channels, channels, 1)
        for p in self.proj_out.parameters():
            p.detach().zero_()


class TimestepEmbedSequential(nn.Sequential):
    pass


class _ADMHost(HipUNetHost):
    """What ``UNetModel`` and ``UNetModelAttn`` share: the tree around the attention layers (`attention(ch, upsample)` makes one), its packing, the ResBlock,
    the block body and the encoder / decoder walk.  A subclass adds what it puts at the attention positions: `_pack_other`, `_run_other`."""

    def _build_tree(self, attention, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout, channel_mult,
                    conv_resample, dims, num_classes, use_fp16, use_scale_shift_norm, resblock_updown):
        self._init_host_state()
        if dims != 2 or use_fp16:
            raise NotImplementedError("only dims=2, use_fp16=False are built (the HIP path computes in fp16 operands / fp32 accumulate by itself)")
        self.image_size, self.in_channels, self.model_channels, self.out_channels = image_size, in_channels, model_channels, out_channels
        self.num_classes = num_classes
        ted = model_channels * 4
        self.time_embed = nn.Sequential(nn.Linear(model_channels, ted), nn.SiLU(), nn.Linear(ted, ted))
        if num_classes is not None:
            self.label_emb = nn.Embedding(num_classes, ted)
        ch = input_ch = int(channel_mult[0] * model_channels)
        self.input_blocks = nn.ModuleList([TimestepEmbedSequential(nn.Conv2d(in_channels, ch, 3, padding=1))])
        chans, ds = [ch], 1
        for level, mult in enumerate(channel_mult):
            for _ in range(num_res_blocks):
                layers = [ResBlock(ch, ted, dropout, out_channels=int(mult * model_channels), use_scale_shift_norm=use_scale_shift_norm)]
                ch = int(mult * model_channels)
                if ds in attention_resolutions:
                    layers.append(attention(ch, False))
                self.input_blocks.append(TimestepEmbedSequential(*layers))
                chans.append(ch)
            if level != len(channel_mult) - 1:
                self.input_blocks.append(TimestepEmbedSequential(
                    ResBlock(ch, ted, dropout, out_channels=ch, use_scale_shift_norm=use_scale_shift_norm, down=True) if resblock_updown
                    else Downsample(ch, conv_resample, out_channels=ch)))
                chans.append(ch)
                ds *= 2
        self.middle_block = TimestepEmbedSequential(
            ResBlock(ch, ted, dropout, use_scale_shift_norm=use_scale_shift_norm),
            attention(ch, False),
            ResBlock(ch, ted, dropout, use_scale_shift_norm=use_scale_shift_norm))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [ResBlock(ch + ich, ted, dropout, out_channels=int(model_channels * mult), use_scale_shift_norm=use_scale_shift_norm)]
                ch = int(model_channels * mult)
                if ds in attention_resolutions:
                    layers.append(attention(ch, True))
                if level and i == num_res_blocks:
                    layers.append(ResBlock(ch, ted, dropout, out_channels=ch, use_scale_shift_norm=use_scale_shift_norm, up=True) if resblock_updown
                                  else Upsample(ch, conv_resample, out_channels=ch))
                    ds //= 2
                self.output_blocks.append(TimestepEmbedSequential(*layers))
        self.out = nn.Sequential(normalization(ch), nn.SiLU(), nn.Conv2d(input_ch, out_channels, 3, padding=1))
        for p in self.out[-1].parameters():
            p.detach().zero_()

    # ---- packing ------------------------------------------------------------------------------------------------------
    def _out_modules(self):
        return self.out[0], self.out[2]

    def _pack_blocks(self, P, dev):
        emb = {}
        for name, m in self.named_modules():
            if isinstance(m, ResBlock):
                P[name] = dict(gn1=pack_gn(m.in_layers[0], dev), c1=pack_conv3(m.in_layers[2], dev), gn2=pack_gn(m.out_layers[0], dev),
                               c2=pack_conv3(m.out_layers[3], dev),
                               skip=None if isinstance(m.skip_connection, nn.Identity) else pack_conv1(m.skip_connection, dev))
                emb[name] = (f16(m.emb_layers[1].weight, dev), f32(m.emb_layers[1].bias, dev))
            elif isinstance(m, AttentionBlock):
                qw, qb = m.qkv.weight.reshape(3 * m.channels, -1), m.qkv.bias
                if m.use_new_attention_order:
                    # QKVAttention (unet.py:341-369) chunks [q | k | v] first and heads second; the kernel reads QKVAttentionLegacy's
                    # [head][q | k | v][ch] rows: a one-time row permutation of qkv.weight / bias makes the two the same computation
                    H, Cc = m.num_heads, m.channels // m.num_heads
                    perm = torch.arange(3 * m.channels, device=qw.device).reshape(3, H, Cc).permute(1, 0, 2).reshape(-1)
                    qw, qb = qw[perm], qb[perm]
                P[name] = dict(gn_attn=pack_gn(m.norm, dev), qkv=(f16(qw, dev), f32(qb, dev)), proj=pack_conv1(m.proj_out, dev))
            elif isinstance(m, Downsample):
                P[name] = pack_conv3(m.op, dev)
            elif isinstance(m, Upsample):
                P[name] = pack_conv3(m.conv, dev)
            else:
                self._pack_other(P, name, m, dev)
        P["emb_all"] = stack_rows(emb)  # every ResBlock's emb_layers Linear (unet.py:205-207)
        c0 = self.input_blocks[0][0]
        P["conv_in"] = (f32(c0.weight, dev), f32(c0.bias, dev))
        P["time"] = tuple(f32(t, dev) for t in (self.time_embed[0].weight, self.time_embed[0].bias, self.time_embed[2].weight, self.time_embed[2].bias))
        P["label"] = f32(self.label_emb.weight, dev) if self.num_classes is not None else None

    def _pack_other(self, P, name, m, dev):
        pass

    # ---- blocks (all enqueue on torch's current stream) ------------------------------------------------------------------
    def _resblock(self, name, m, h, N, H, W, film_all):
        p = self._packed[name]
        Cin, Cout = m.channels, m.out_channels
        pair = None
        if isinstance(h, tuple):  # (h, skip) of an output block: read in place by the first GroupNorm and the 1x1 skip convolution
            if m.updown or p["skip"] is None or h[0].shape[1] % 64 or h[1].shape[1] % 8:
                h = self._cat(h)  # resampled / identity-skip inputs need the tensor itself
            else:
                pair = h
        if pair is not None:
            t1 = self._gn2(pair[0], pair[1], N, H * W, p["gn1"], None, True)
        else:
            t1 = self._gn(h, N, H * W, Cin, p["gn1"], None, True)
        if m.updown:  # in_rest -> h_upd / x_upd -> in_conv (unet.py:219-224): nearest 2x or 2x2 mean on both branches
            H2, W2 = (H * 2, W * 2) if m.h_upd.up else (H // 2, W // 2)
            t1, h = self._resample(t1, N, H2, W2, Cin, m.h_upd.up), self._resample(h, N, H2, W2, Cin, m.h_upd.up)
            H, W = H2, W2
        a = self._conv(t1, p["c1"], N, H, W, Cin, Cout)
        o, wdt = self._packed["emb_all"][2][name]
        emb_out = film_all[:, o:o + wdt]  # a column slice of the one emb GEMM of this evaluation
        if m.use_scale_shift_norm:  # fp32 [N, 2*Cout] = [scale | shift] folded into the GroupNorm affine (unet.py:228-232)
            t2 = self._gn(a, N, H * W, Cout, p["gn2"], emb_out, True)
        else:                       # h = h + emb_out[..., None, None]; out_layers(h)  (unet.py:233-235)
            a2 = self._add_image_vec(a, emb_out, N, H * W, Cout)
            t2 = self._gn(a2, N, H * W, Cout, p["gn2"], None, True)
        if pair is not None:
            skip = self._linear2(pair[0], pair[1], p["skip"])
        else:
            skip = h if p["skip"] is None else self._linear(h, p["skip"])
        return self._conv(t2, p["c2"], N, H, W, Cout, Cout, resid=skip)

    def _run_block(self, prefix, block, h, N, H, W, film_all):
        for j, layer in enumerate(block):
            name = f"{prefix}.{j}"
            if isinstance(layer, ResBlock):
                h = self._resblock(name, layer, h, N, H, W, film_all)
                if layer.updown:
                    H, W = (H * 2, W * 2) if layer.h_upd.up else (H // 2, W // 2)
            elif isinstance(layer, AttentionBlock):
                h = self._attention(h, self._packed[name], N, H * W, layer.num_heads, layer.channels)
            elif isinstance(layer, Downsample):
                H, W = H // 2, W // 2
                h = self._conv(h, self._packed[name], N, H, W, layer.channels, layer.out_channels, mode=2)
            elif isinstance(layer, Upsample):
                H, W = H * 2, W * 2
                h = self._conv(h, self._packed[name], N, H, W, layer.channels, layer.out_channels, mode=1)
            else:
                h = self._run_other(name, layer, h, N, H, W)
        return h, H, W

    def _run_other(self, name, layer, h, N, H, W):
        raise TypeError(type(layer))

    # ---- forward ------------------------------------------------------------------------------------------------------
    def _walk(self, x, t, y):
        """The network on the prologue's x (contiguous fp32) and t (fp32 [1] or [N]) (unet.py:613-655)."""
        N, Cin, H, W = x.shape
        assert Cin == self.in_channels
        if y is not None:
            y = y.to(x.device, torch.long).contiguous()
            assert y.shape == (N,)
        emb_silu = self._time_embed(t, N, y, self.model_channels, self.model_channels * 4)
        ea = self._packed["emb_all"]
        film_all = hip.gemm_f16(emb_silu, ea[0], ea[1], epilogue=2)  # every ResBlock's emb_layers in one launch
        h = self._conv_in(x, self._packed["conv_in"], N, H, W, Cin)
        hs = [h]
        for i, block in enumerate(self.input_blocks):
            if i == 0:
                continue
            h, H, W = self._run_block(f"input_blocks.{i}", block, h, N, H, W, film_all)
            hs.append(h)
        h, H, W = self._run_block("middle_block", self.middle_block, h, N, H, W, film_all)
        for i, block in enumerate(self.output_blocks):
            skip = hs.pop()
            # th.cat([h, hs.pop()], dim=1) (unet.py:649) is consumed in place by a leading ResBlock's GroupNorm and skip conv
            h, H, W = self._run_block(f"output_blocks.{i}", block, (h, skip) if isinstance(block[0], ResBlock) else self._cat((h, skip)), N, H, W, film_all)
        return self._out(h, N, H, W)


class UNetModel(_ADMHost):
    _what, _what_eval = "UNetModel", "UNet"

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False,
                 num_heads=1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False):
        super().__init__()
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads

        def attention(ch, upsample):
            return AttentionBlock(ch, num_heads=num_heads_upsample if upsample else num_heads, num_head_channels=num_head_channels,
                                  use_new_attention_order=use_new_attention_order)

        self._build_tree(attention, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout, channel_mult,
                         conv_resample, dims, num_classes, use_fp16, use_scale_shift_norm, resblock_updown)

    @torch.no_grad()
    def forward(self, timesteps, x, y=None, **kwargs):
        """v = model(t, x, y) (unet.py:613-655).  t: 0-d / [1] / [N] (a scalar is broadcast; the reference's hard-coded
        ``device="cuda"`` at :630 is the tensor's device here)."""
        assert (y is not None) == (self.num_classes is not None), "must specify y if and only if the model is class-conditional"
        x, t = self._prologue(timesteps, x, "timesteps")
        return self._walk(x, t, y)

    def forward_with_cfg(self, *a, **k):
        raise NotImplementedError("UNetModel has no forward_with_cfg in the reference either (unet.py:376-655): CFG needs DiT or the EDM adm")


# ---- the layout UNet: UNetModelAttn, SpatialTransformer blocks at the attention positions (unet.py:882-1205, attention.py:85-280) ------------------------
class CrossAttention(nn.Module):  # attention.py:177-215
    def __init__(self, query_dim, context_dim=None, heads=8, dim_head=64, dropout=0.0):
        super().__init__()
        inner = dim_head * heads
        self.heads, self.dim_head, self.context_dim = heads, dim_head, query_dim if context_dim is None else context_dim
        self.to_q = nn.Linear(query_dim, inner, bias=False)
        self.to_k = nn.Linear(self.context_dim, inner, bias=False)
        self.to_v = nn.Linear(self.context_dim, inner, bias=False)
        self.to_out = nn.Sequential(nn.Linear(inner, query_dim), nn.Dropout(dropout))


class GEGLU(nn.Module):  # attention.py:85-92
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = nn.Linear(dim_in, dim_out * 2)


class FeedForward(nn.Module):  # attention.py:95-105 with glu=True, mult=4
    def __init__(self, dim, mult=4, dropout=0.0):
        super().__init__()
        self.net = nn.Sequential(GEGLU(dim, dim * mult), nn.Dropout(dropout), nn.Linear(dim * mult, dim))


class BasicTransformerBlock(nn.Module):  # attention.py:218-240: x += attn1(norm1 x); x += attn2(norm2 x, context); x += ff(norm3 x)
    def __init__(self, dim, n_heads, d_head, dropout=0.0, context_dim=None):
        super().__init__()
        self.attn1 = CrossAttention(dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.ff = FeedForward(dim, dropout=dropout)
        self.attn2 = CrossAttention(dim, context_dim=context_dim, heads=n_heads, dim_head=d_head, dropout=dropout)
        self.norm1, self.norm2, self.norm3 = nn.LayerNorm(dim), nn.LayerNorm(dim), nn.LayerNorm(dim)


class SpatialTransformer(nn.Module):  # attention.py:243-280
    def __init__(self, in_channels, n_heads, d_head, depth=1, dropout=0.0, context_dim=None):
        super().__init__()
        self.in_channels, self.n_heads, self.d_head, self.context_dim = in_channels, n_heads, d_head, context_dim
        inner = n_heads * d_head
        if d_head % 16 or d_head > 256:
            raise NotImplementedError(f"SpatialTransformer heads of {d_head} channels: the attention kernels serve channels per head % 16 == 0 and <= 256")
        self.norm = nn.GroupNorm(32, in_channels, eps=1e-6)
        self.proj_in = nn.Conv2d(in_channels, inner, 1)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, n_heads, d_head, dropout=dropout, context_dim=context_dim) for _ in range(depth)])
        self.proj_out = nn.Conv2d(inner, in_channels, 1)
        for p in self.proj_out.parameters():  # zero_module (attention.py:267)
            p.detach().zero_()


def _no_bias(w, dev):
    return f16(w, dev), None


class UNetModelAttn(_ADMHost):
    """``UNetModelAttn`` (unet.py:882-1205, behind ``--use_origin_adm --layout``): the ADM UNet whose attention blocks are SpatialTransformers -- per block a
    self-attention, a cross-attention over a context sequence [N, L, context_dim] and a GEGLU MLP between LayerNorms.  Same constructor arguments and
    parameter tree as the reference (``...{norm,proj_in,transformer_blocks.d.{attn1,attn2}.{to_q,to_k,to_v,to_out.0},ff.net.{0.proj,2},norm{1,2,3},proj_out}``),
    same call contract ``model(t, x, context=None, y=None) -> v``.

    On the device a transformer runs on the fp16 NHWC rows [N*T, C] (already ``b (h w) c``): GroupNorm(eps 1e-6), proj_in; per block LayerNorm -> one GEMM
    over [to_q | to_k | to_v] in the [head][q|k|v][ch] row order -> lfm_attention_small_f16 -> to_out + x;  LayerNorm -> to_q -> lfm_cross_attention_f16
    against the context K / V -> to_out + x;  LayerNorm -> ff.net.0.proj -> lfm_geglu_f16 -> ff.net.2 + x;  then proj_out + x_in.  to_k / to_v of EVERY attn2
    read the same context, which does not depend on t: their weights are stacked row-wise and a context is projected by ONE GEMM, cached per model on the
    context tensor's (data_ptr, _version, shape, stride, dtype, device) -- a 50-step solve pays once; a repack or a move of the model drops it.  While the
    current stream is capturing the cache is neither read nor written: the projection is part of the graph every time, so a replay projects whatever the
    static context tensor then holds and no graph points into a buffer that a later eager call replaces.  With ``context=None`` attn2 attends over its
    own normalised input, which needs block width == context_dim."""

    _what = _what_eval = "UNetModelAttn"
    _scratch_attrs = HipUNetHost._scratch_attrs + ("_ctx_key", "_ctx_kv", "_ctx_src")  # the cached context projection goes with the packed weights' device

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False,
                 num_heads=-1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False, use_spatial_transformer=False, transformer_depth=1, context_dim=None, legacy=True):
        super().__init__()
        if not use_spatial_transformer:
            raise NotImplementedError("UNetModelAttn is built with use_spatial_transformer=True only: the ADM UNet with AttentionBlocks is UNetModel")
        if context_dim is None:
            raise ValueError("use_spatial_transformer needs context_dim, the feature count of the cross-attention conditioning")
        if isinstance(context_dim, (list, tuple)):  # the reference turns an omegaconf list into a list; a one-element list is the only one it can use
            if len(context_dim) != 1:
                raise ValueError(f"context_dim={context_dim}: one feature count is expected")
            context_dim = context_dim[0]
        if num_heads == -1 and num_head_channels == -1:
            raise ValueError("Either num_heads or num_head_channels has to be set")
        self.context_dim, self.transformer_depth = int(context_dim), transformer_depth

        def attention(ch, upsample):  # unet.py:1010-1029: the decoder's transformers take num_heads too, not num_heads_upsample
            heads = num_heads if num_head_channels == -1 else ch // num_head_channels
            dim_head = ch // heads  # legacy or not: ch // num_heads, which is num_head_channels where that is set
            return SpatialTransformer(ch, heads, dim_head, depth=transformer_depth, context_dim=self.context_dim)

        self._build_tree(attention, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout, channel_mult,
                         conv_resample, dims, num_classes, use_fp16, use_scale_shift_norm, resblock_updown)
        self._ctx = None  # K | V of the context of the evaluation in flight
        self._widths = sorted({m.n_heads * m.d_head for m in self.modules() if isinstance(m, SpatialTransformer)})

    # ---- packing ------------------------------------------------------------------------------------------------------
    def _pack_blocks(self, P, dev):
        self._kv = {}
        super()._pack_blocks(P, dev)
        P["ctx_kv"] = stack_rows(self._kv)  # to_k | to_v of every attn2: one GEMM per context
        del self._kv
        self._ctx_key = self._ctx_kv = self._ctx_src = None

    def _pack_other(self, P, name, m, dev):
        if not isinstance(m, SpatialTransformer):
            return
        H, dh = m.n_heads, m.d_head
        perm = torch.arange(3 * H * dh).reshape(3, H, dh).permute(1, 0, 2).reshape(-1)  # [q | k | v][head][ch] -> the kernel's [head][q | k | v][ch]
        blocks = []
        for d, b in enumerate(m.transformer_blocks):
            qkv = torch.cat([b.attn1.to_q.weight, b.attn1.to_k.weight, b.attn1.to_v.weight], 0)[perm.to(b.attn1.to_q.weight.device)]
            kv = torch.cat([b.attn2.to_k.weight, b.attn2.to_v.weight], 0)
            self._kv[f"{name}.{d}"] = (f16(kv, dev), torch.zeros(kv.shape[0], device=dev))
            lin = lambda l: (f16(l.weight, dev), f32(l.bias, dev))  # noqa: E731
            blocks.append(dict(ln1=pack_gn(b.norm1, dev), ln2=pack_gn(b.norm2, dev), ln3=pack_gn(b.norm3, dev), qkv=_no_bias(qkv, dev),
                               out1=lin(b.attn1.to_out[0]), q=_no_bias(b.attn2.to_q.weight, dev), kv=(self._kv[f"{name}.{d}"][0], None), out2=lin(b.attn2.to_out[0]),
                               ff1=lin(b.ff.net[0].proj), ff2=lin(b.ff.net[2]), eps=(b.norm1.eps, b.norm2.eps, b.norm3.eps)))
        P[name] = dict(gn=pack_gn(m.norm, dev), proj_in=pack_conv1(m.proj_in, dev), proj_out=pack_conv1(m.proj_out, dev), blocks=blocks)

    # ---- the context ---------------------------------------------------------------------------------------------------
    def _project_context(self, ctx16):
        """K | V of every attn2 for a context fp16 [N*L, context_dim]: one GEMM over the stacked to_k / to_v rows."""
        w, _, _ = self._packed["ctx_kv"]
        return self._linear(ctx16, (w, None))

    def _context_kv(self, context, N):
        if context.dim() != 3 or context.shape[0] != N or context.shape[2] != self.context_dim:
            raise ValueError(f"context must be [{N}, L, {self.context_dim}], got {tuple(context.shape)}")
        hip.require_gpu(context, "UNetModelAttn.forward (context)")
        if torch.cuda.is_current_stream_capturing():
            # in the graph every time, the cache neither read nor written: a replay must project what the static tensor holds THEN (no Python runs on replay,
            # so a cached K | V would be the context of capture time for ever), and the graph must not point into a buffer a later eager call replaces
            return self._project_context(context.reshape(-1, self.context_dim).to(torch.float16).contiguous())
        # The weights are not in the key (no _gen, which scratch growth inside a walk bumps as well): every repack clears the cache (_pack_blocks; a
        # load_state_dict or a move forces one) and _apply clears it through _scratch_attrs.
        key = (context.data_ptr(), context._version, tuple(context.shape), context.stride(), context.dtype, context.device)
        if self._ctx_key != key:
            # the tensor itself is kept with its key: while it is cached its address cannot be handed to another tensor (hip.check_labels: the same hazard)
            self._ctx_kv = self._project_context(context.reshape(-1, self.context_dim).to(torch.float16).contiguous())
            self._ctx_key, self._ctx_src = key, context
        return self._ctx_kv

    # ---- the transformer -----------------------------------------------------------------------------------------------
    def _run_other(self, name, m, x_in, N, H, W):
        if not isinstance(m, SpatialTransformer):
            raise TypeError(type(m))
        p, T, heads, dh = self._packed[name], H * W, m.n_heads, m.d_head
        inner = heads * dh
        x = self._linear(self._gn(x_in, N, T, m.in_channels, p["gn"], None, False, eps=m.norm.eps), p["proj_in"])
        for d, b in enumerate(p["blocks"]):
            qkv = self._linear(hip.layernorm(x, *b["ln1"], eps=b["eps"][0]), b["qkv"])
            a = torch.empty(N * T, inner, dtype=torch.float16, device=x.device)
            hip.unet_attention(qkv, a, N, T, heads, dh)
            x = self._linear(a, b["out1"], resid=x)
            t = hip.layernorm(x, *b["ln2"], eps=b["eps"][1])
            q = self._linear(t, b["q"])
            if self._ctx is None:  # attn2 over its own normalised input (attention.py:196): the block's own [to_k | to_v] rows, packed once
                kv, Tk = self._linear(t, b["kv"]), T
            else:
                o, _ = self._packed["ctx_kv"][2][f"{name}.{d}"]
                kv, Tk = self._ctx[:, o:o + 2 * inner], self._ctx.shape[0] // N
            a = hip.cross_attention(q, kv[:, :inner], kv[:, inner:], N, T, Tk, heads, dh)
            x = self._linear(a, b["out2"], resid=x)
            g = hip.geglu(self._linear(hip.layernorm(x, *b["ln3"], eps=b["eps"][2]), b["ff1"]))
            x = self._linear(g, b["ff2"], resid=x)
        return self._linear(x, p["proj_out"], resid=x_in)

    # ---- forward -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, timesteps, x, context=None, y=None, **kwargs):
        """v = model(t, x, context, y) (unet.py:1174-1205): the THIRD positional argument is the context [N, L, context_dim] (any float dtype; converted once
        to contiguous fp16), labels go by keyword.  t: 0-d / [1] / [N]."""
        assert (y is not None) == (self.num_classes is not None), "must specify y if and only if the model is class-conditional"
        if context is None and self._widths != [self.context_dim]:
            width = next(w for w in self._widths if w != self.context_dim)
            raise ValueError(f"context=None makes attn2 attend over its own input, which needs the block width ({width}) to equal "
                             f"context_dim ({self.context_dim}): pass a context")
        x, t = self._prologue(timesteps, x, "timesteps")
        self._ctx = None if context is None else self._context_kv(context, x.shape[0])
        try:
            return self._walk(x, t, y)
        finally:
            self._ctx = None

    def forward_with_cfg(self, *a, **k):
        raise NotImplementedError("UNetModelAttn has no forward_with_cfg in the reference either (unet.py:882-1205): CFG needs DiT or the EDM adm")
