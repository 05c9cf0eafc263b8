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


class UNetModel(HipUNetHost):
    _what, _what_eval = "UNetModel", "UNet"

    def __init__(self, image_size, in_channels, model_channels, out_channels, num_res_blocks, attention_resolutions, dropout=0,
                 channel_mult=(1, 2, 4, 8), conv_resample=True, dims=2, num_classes=None, use_checkpoint=False, use_fp16=False,
                 num_heads=1, num_head_channels=-1, num_heads_upsample=-1, use_scale_shift_norm=False, resblock_updown=False,
                 use_new_attention_order=False):
        super().__init__()
        self._init_host_state()
        if dims != 2 or use_fp16:
            raise NotImplementedError("only dims=2, use_fp16=False are built (the HIP path computes in fp16 operands / fp32 accumulate by itself)")
        if num_heads_upsample == -1:
            num_heads_upsample = num_heads
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
                    layers.append(AttentionBlock(ch, num_heads=num_heads, num_head_channels=num_head_channels, use_new_attention_order=use_new_attention_order))
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
            AttentionBlock(ch, num_heads=num_heads, num_head_channels=num_head_channels, use_new_attention_order=use_new_attention_order),
            ResBlock(ch, ted, dropout, use_scale_shift_norm=use_scale_shift_norm))
        self.output_blocks = nn.ModuleList([])
        for level, mult in list(enumerate(channel_mult))[::-1]:
            for i in range(num_res_blocks + 1):
                ich = chans.pop()
                layers = [ResBlock(ch + ich, ted, dropout, out_channels=int(model_channels * mult), use_scale_shift_norm=use_scale_shift_norm)]
                ch = int(model_channels * mult)
                if ds in attention_resolutions:
                    layers.append(AttentionBlock(ch, num_heads=num_heads_upsample, num_head_channels=num_head_channels,
                                                 use_new_attention_order=use_new_attention_order))
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
        P["emb_all"] = stack_rows(emb)  # every ResBlock's emb_layers Linear (unet.py:205-207)
        c0 = self.input_blocks[0][0]
        P["conv_in"] = (f32(c0.weight, dev), f32(c0.bias, dev))
        P["time"] = tuple(f32(t, dev) for t in (self.time_embed[0].weight, self.time_embed[0].bias, self.time_embed[2].weight, self.time_embed[2].bias))
        P["label"] = f32(self.label_emb.weight, dev) if self.num_classes is not None else None

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
                raise TypeError(type(layer))
        return h, H, W

    # ---- forward ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, timesteps, x, y=None, **kwargs):
        """v = model(t, x, y) (unet.py:613-655).  t: 0-d / [1] / [N] (a scalar is broadcast; the reference's hard-coded
        ``device="cuda"`` at :630 is the tensor's device here)."""
        assert (y is not None) == (self.num_classes is not None), "must specify y if and only if the model is class-conditional"
        x, t = self._prologue(timesteps, x, "timesteps")
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

    def forward_with_cfg(self, *a, **k):
        raise NotImplementedError("UNetModel has no forward_with_cfg in the reference either (unet.py:376-655): CFG needs DiT or the EDM adm")
