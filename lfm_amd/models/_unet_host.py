"""The host layer the UNet backbones share (``UNetModel`` and ``UNetModelAttn``, ``DhariwalUNet``, ``SongUNet``): the packed-operand / scratch state and its invalidation,
the weight-packing helpers, and ONE copy of every host-sequenced op over the NHWC-fp16 building blocks of liblfm_hip.so -- GroupNorm (one or two sources),
3x3 convolution with its split-K workspace, linear (one or two sources), channel concat, 2x resampling, the FiLM add, attention, the fp32 input and output
convolutions, the time embedding and the forward prologue.  A backbone keeps its parameter tree, what it packs under which names, its block body, its
encoder / decoder walk and its mapping network.  Every op enqueues on torch's current stream; no PyTorch compute ops."""
import torch
import torch.nn as nn

from .. import hip


class PackedModule(nn.Module):
    """Weights packed for the device in ``_packed``, device scratch in the attributes ``_scratch_attrs`` names, and ``_gen``, bumped whenever device buffers a
    captured graph may point to are replaced."""

    _scratch_attrs = ()

    def _init_host_state(self):
        self._packed = None
        for name in self._scratch_attrs:
            setattr(self, name, None)
        self._gen = 0

    def _apply(self, fn, *a, **k):
        # only a real move / cast invalidates (NFECount(model).to(device) on an already-placed model must not re-pack the weights per call)
        before = [(p.data_ptr(), p.dtype, p.device) for p in self.parameters()]
        out = super()._apply(fn, *a, **k)
        if before != [(p.data_ptr(), p.dtype, p.device) for p in self.parameters()]:
            self._packed = None
            for name in self._scratch_attrs:
                setattr(self, name, None)
            self._gen += 1
        return out

    def load_state_dict(self, *a, **k):
        self._packed = None
        self._gen += 1
        return super().load_state_dict(*a, **k)


# ---- packing ------------------------------------------------------------------------------------------------------------
def f32(t, dev):
    return t.detach().to(dev, torch.float32).contiguous()


def f16(t, dev):
    return t.detach().to(dev, torch.float16).contiguous()


def pack_gn(m, dev):
    return f32(m.weight, dev), f32(m.bias, dev)


def pack_conv3(m, dev):
    w = m.weight
    if w.shape[1] % 64:
        raise hip.LfmHipError(f"3x3 conv with Cin={w.shape[1]}: the implicit-GEMM path needs Cin % 64 == 0")
    return f16(w.permute(0, 2, 3, 1).reshape(w.shape[0], -1), dev), f32(m.bias, dev)


def pack_conv1(m, dev):
    return f16(m.weight.reshape(m.weight.shape[0], -1), dev), f32(m.bias, dev)


def pack_conv_out4(m, dev):
    """The fp32-output 3x3 convolution: its (at most 4) output channels padded to 4."""
    wo = m.weight
    if wo.shape[0] > 4:
        raise hip.LfmHipError("output conv with more than 4 channels is not built")
    w4 = torch.zeros(4, wo.shape[1], 3, 3, device=dev)
    w4[: wo.shape[0]] = wo
    b4 = torch.zeros(4, device=dev)
    b4[: wo.shape[0]] = m.bias
    return f16(w4.permute(0, 2, 3, 1).reshape(4, -1), dev), f32(b4, dev)


def stack_rows(wbs):
    """{name: (w, b)} -> (weights stacked row-wise, biases, {name: (offset, width)}).  Every block projects the SAME embedding row through its own Linear:
    one GEMM per evaluation over the stacked weights (M = batch rows only -- some 28 tiny launches otherwise), each block then reads its column slice."""
    offs, off = {}, 0
    for name, (w, _) in wbs.items():
        offs[name] = (off, w.shape[0])
        off += w.shape[0]
    return torch.cat([w for w, _ in wbs.values()], 0).contiguous(), torch.cat([b for _, b in wbs.values()], 0).contiguous(), offs


def qkv_rows_separate(q, k, v, heads):
    """Three [C, ...] tensors whose rows are [head][ch] (EDM CrossAttention's q / k / v: ``reshape(N * heads, C // heads, -1)``) -> one [3C, ...] tensor with
    rows [head][q | k | v][ch], the layout lfm_attention_small_f16 reads."""
    C = q.shape[0]
    return torch.stack([q, k, v], 0).reshape(3, heads, C // heads, *q.shape[1:]).transpose(0, 1).reshape(3 * C, *q.shape[1:])


def pack_qkv_separate(attn, dev):
    """The three 1x1 convolutions of a self-attention CrossAttention (EDM.py:388-405) as ONE qkv linear."""
    C = attn.q.weight.shape[0]
    w = qkv_rows_separate(*(m.weight.detach().reshape(C, -1) for m in (attn.q, attn.k, attn.v)), attn.num_heads)
    b = qkv_rows_separate(*(m.bias.detach() for m in (attn.q, attn.k, attn.v)), attn.num_heads)
    return f16(w, dev), f32(b, dev)


def context_table(attn2, table):
    """A cross-attention over ONE key (EDM TransformerBlock.attn2 on a [N, E, 1, 1] context): the softmax over a single finite score is exactly 1, so its
    output is proj(v(context)) at every query, whatever the query, the q and k weights and the norm in front are.  Over all rows E[label] of the label table:
    U[label] = proj.W (v.W E[label] + v.b) + proj.b, in float64 on the host -> fp32 [rows, C]."""
    d = torch.float64
    C = attn2.v.weight.shape[0]
    E = table.detach().cpu().to(d)
    vw, pw = attn2.v.weight.detach().cpu().to(d).reshape(C, -1), attn2.proj.weight.detach().cpu().to(d).reshape(C, C)
    val = E @ vw.t() + attn2.v.bias.detach().cpu().to(d)
    return (val @ pw.t() + attn2.proj.bias.detach().cpu().to(d)).float()


def pack_context_tables(attn2s, table, dev):
    """{name: attn2} -> (fp32 [rows, sum of C] on the device: every block's context_table side by side, {name: (column offset, C)}).  One gather per forward
    takes the batch's label rows; each block then reads its column slice -- as `stack_rows` does for the blocks' `affine`."""
    offs, off, cols = {}, 0, []
    for name, a in attn2s.items():
        u = context_table(a, table)
        offs[name] = (off, u.shape[1])
        off += u.shape[1]
        cols.append(u)
    return torch.cat(cols, 1).contiguous().to(dev), offs


class HipUNetHost(PackedModule):
    """A subclass builds the parameter tree, calls ``_init_host_state()``, and provides ``_what`` (its name in error messages), ``_out_modules()`` (the output
    GroupNorm and convolution) and ``_pack_blocks(P, dev)`` (everything else it packs)."""

    _scratch_attrs = ("_scratch", "_conv_ws")  # GroupNorm statistics; split-K slabs of the 3x3 convolutions
    _what = "UNet"
    _what_eval = None  # the name in the inference-only message, where it is not `_what`

    @torch.no_grad()
    def _pack(self):
        out_norm, out_conv = self._out_modules()
        dev = out_conv.weight.device
        hip.require_gpu(out_conv.weight, self._what)
        P = {}
        self._pack_blocks(P, dev)
        P["gn_out"] = pack_gn(out_norm, dev)
        P["conv_out"] = pack_conv_out4(out_conv, dev)
        self._packed = P
        self._gen += 1
        return P

    def _grow(self, attr, need, device, floor=0):
        buf = getattr(self, attr)
        if buf is None or buf.numel() < need or buf.device != device:
            buf = torch.empty(max(need, floor), dtype=torch.uint8, device=device)
            setattr(self, attr, buf)
            self._gen += 1
        return buf

    # ---- ops --------------------------------------------------------------------------------------------------------------
    def _gn(self, x, N, HW, C, gb, film, silu, groups=32, eps=1e-5):
        """GroupNorm (+ FiLM: `film` fp32 [N, 2C] = [scale | shift], a column slice of the stacked projection) (+ SiLU)."""
        y = torch.empty_like(x)
        scratch = self._grow("_scratch", hip.lib().lfm_groupnorm_scratch_bytes(N, C), x.device, floor=1 << 20)
        hip.check(hip.lib().lfm_groupnorm_f16(hip.ptr(x), hip.ptr(y), hip.ptr(gb[0]), hip.ptr(gb[1]), hip.ptr(film),
                                              film.stride(0) if film is not None else 0, hip.ptr(scratch), N, HW, C, groups, eps,
                                              1 if silu else 0, hip.stream_ptr(x.device)), "lfm_groupnorm_f16")
        return y

    def _gn2(self, xa, xb, N, HW, gb, film, silu, groups=32, eps=1e-5):
        """GroupNorm of the channel concat [xa | xb] read in place (the decoder's ``cat([h, skip], dim=1)`` is never materialised)."""
        Ca, Cb = xa.shape[1], xb.shape[1]
        y = torch.empty(xa.shape[0], Ca + Cb, dtype=torch.float16, device=xa.device)
        scratch = self._grow("_scratch", hip.lib().lfm_groupnorm_scratch_bytes(N, Ca + Cb), xa.device, floor=1 << 20)
        hip.check(hip.lib().lfm_groupnorm2_f16(hip.ptr(xa), Ca, hip.ptr(xb), Cb, hip.ptr(y), hip.ptr(gb[0]), hip.ptr(gb[1]), hip.ptr(film),
                                               film.stride(0) if film is not None else 0, hip.ptr(scratch), N, HW, groups, eps,
                                               1 if silu else 0, hip.stream_ptr(xa.device)), "lfm_groupnorm2_f16")
        return y

    def _conv(self, x, wb, N, H, W, Cin, Cout, mode=0, resid=None, scale=1.0):
        """3x3 convolution on the H x W OUTPUT grid (mode 1: fused nearest-2x upsample, 2: stride 2); out = (acc + bias + resid) * scale."""
        out = torch.empty(N * H * W, Cout, dtype=torch.float16, device=x.device)
        need = hip.lib().lfm_conv3x3_workspace_bytes(N, H, W, Cin, Cout)  # > 0 for the small-M / huge-K low-resolution levels: split-K slabs
        ws = self._grow("_conv_ws", need, x.device) if need else None
        hip.check(hip.lib().lfm_conv3x3_scaled_f16_ws(hip.ptr(x), hip.ptr(wb[0]), hip.ptr(wb[1]), hip.ptr(resid), scale, hip.ptr(out), N, H, W, Cin, Cout,
                                                      mode, hip.ptr(ws), ws.numel() if ws is not None else 0, hip.stream_ptr(x.device)),
                  "lfm_conv3x3_scaled_f16_ws")
        return out

    def _linear(self, x, wb, resid=None, scale=1.0):
        M, K = x.shape
        Nout = wb[0].shape[0]
        out = torch.empty(M, Nout, dtype=torch.float16, device=x.device)
        hip.check(hip.lib().lfm_linear_scaled_f16(hip.ptr(x), x.stride(0), hip.ptr(wb[0]), wb[0].stride(0), hip.ptr(out), Nout, M, Nout, K,
                                                  hip.ptr(wb[1]), hip.ptr(resid), scale, hip.stream_ptr(x.device)), "lfm_linear_scaled_f16")
        return out

    def _linear2(self, xa, xb, wb):
        """Linear over the channel concat [xa | xb] read in place."""
        M, Nout = xa.shape[0], wb[0].shape[0]
        out = torch.empty(M, Nout, dtype=torch.float16, device=xa.device)
        hip.check(hip.lib().lfm_linear2_f16(hip.ptr(xa), xa.shape[1], hip.ptr(xb), xb.shape[1], hip.ptr(wb[0]), wb[0].stride(0), hip.ptr(out), Nout, M, Nout,
                                            hip.ptr(wb[1]), None, hip.stream_ptr(xa.device)), "lfm_linear2_f16")
        return out

    def _cat(self, pair):
        h, skip = pair
        cat = torch.empty(h.shape[0], h.shape[1] + skip.shape[1], dtype=torch.float16, device=h.device)
        hip.check(hip.lib().lfm_concat_channels_f16(hip.ptr(h), hip.ptr(skip), hip.ptr(cat), h.shape[0], h.shape[1], skip.shape[1],
                                                    hip.stream_ptr(h.device)), "lfm_concat_channels_f16")
        return cat

    def _resample(self, x, N, Ho, Wo, C, up, fir=False):
        """Nearest 2x (`up`) or 2x2 mean, to the Ho x Wo OUTPUT grid; `fir`: the [1,3,3,1] filter in either direction instead (NCSN++)."""
        if fir:
            return hip.fir_up2(x, N, Ho, Wo, C) if up else hip.fir_down2(x, N, Ho, Wo, C)
        y = torch.empty(N * Ho * Wo, C, dtype=torch.float16, device=x.device)
        fn, what = (hip.lib().lfm_upsample2_f16, "lfm_upsample2_f16") if up else (hip.lib().lfm_avgpool2_f16, "lfm_avgpool2_f16")
        hip.check(fn(hip.ptr(x), hip.ptr(y), N, Ho, Wo, C, hip.stream_ptr(x.device)), what)
        return y

    def _conv_pad2_fir_down(self, x, wb, N, H, W, Cin, Cout, resid, scale, nchw_f32=False):
        """EDM's Conv2d(kernel=3, down=True, fused_resample=True) under the [1,3,3,1] filter, with a residual epilogue: the 3x3 convolution at PADDING 2
        (the pad-1 convolution of x inside a zero border, on the (H+2) x (W+2) grid), then the filter at stride 2 without padding onto H/2 x W/2, then
        (. + bias + resid) * scale.  `x`: fp16 NHWC [N*H*W, Cin], or (`nchw_f32`) the fp32 NCHW network input.  `wb` = (weights, the convolution's zero bias, the late bias)."""
        xb = hip.zero_border(x, N, H, W, Cin)
        if nchw_f32:
            full = self._conv_in(xb, wb, N, H + 2, W + 2, Cin)
        else:
            full = self._conv(xb, wb, N, H + 2, W + 2, Cin, Cout)
        return hip.fir_down2(full, N, H // 2, W // 2, Cout, pad=0, bias=wb[2], resid=resid, scale=scale)

    def _add_image_vec(self, x, vec, N, HW, C):
        """x + vec[:, None, None]: `vec` fp32 [N, C], a column slice of the stacked projection."""
        y = torch.empty_like(x)
        hip.check(hip.lib().lfm_add_image_vec_f16(hip.ptr(x), hip.ptr(vec), vec.stride(0), hip.ptr(y), N, HW, C, hip.stream_ptr(x.device)),
                  "lfm_add_image_vec_f16")
        return y

    def _attention(self, x, p, N, T, heads, C, groups=32, eps=1e-5, scale=1.0):
        """(x + proj(attention(qkv(norm(x))))) * scale; the rows of `p["qkv"]` are [head][q | k | v][ch], whatever order the backbone's checkpoint has."""
        t = self._gn(x, N, T, C, p["gn_attn"], None, False, groups, eps)
        qkv = self._linear(t, p["qkv"])
        a = torch.empty(N * T, C, dtype=torch.float16, device=x.device)
        hip.unet_attention(qkv, a, N, T, heads, C // heads)
        return self._linear(a, p["proj"], resid=x, scale=scale)

    def _transformer(self, x, p, u, N, T, heads, C, groups=32, eps=1e-5, scale=1.0):
        """EDM TransformerBlock (EDM.py:477-483) on the [N*T, C] token layout the NHWC activations already have, times `scale`:
            x = attn1(norm1(x)) + x;  x = attn2(norm2(x), context) + x;  x = ff(norm3(x)) + x.
        `u` fp32 [N, C] (a column slice of the gathered context rows) IS attn2's output at every token of image n (`context_table`), so the attn1.proj epilogue
        (acc + bias + x + u[m // T]) performs the first two lines; ff.layer0 carries the SiLU in its epilogue, ff.layer1 the last residual sum."""
        t = self._gn(x, N, T, C, p["gn1"], None, False, groups, eps)
        qkv = self._linear(t, p["qkv"])
        a = torch.empty(N * T, C, dtype=torch.float16, device=x.device)
        hip.unet_attention(qkv, a, N, T, heads, C // heads)
        x = hip.linear_resid_vec(a, p["proj"][0], p["proj"][1], x, u, T)
        del t, qkv, a
        t = self._gn(x, N, T, C, p["gn3"], None, False, groups, eps)
        h = hip.linear_silu(t, p["ff0"][0], p["ff0"][1])
        return self._linear(h, p["ff1"], resid=x, scale=scale)

    def _conv_in(self, x, wb, N, H, W, Cin):
        """The first 3x3 convolution: fp32 NCHW in, fp16 NHWC out."""
        Cout = wb[0].shape[0]
        h = torch.empty(N * H * W, Cout, dtype=torch.float16, device=x.device)
        hip.check(hip.lib().lfm_conv3x3_in_f32(hip.ptr(x), hip.ptr(wb[0]), hip.ptr(wb[1]), hip.ptr(h), N, H, W, Cin, Cout, hip.stream_ptr(x.device)),
                  "lfm_conv3x3_in_f32")
        return h

    def _out(self, h, N, H, W, groups=32, eps=1e-5):
        """silu(norm(h)) through the last 3x3 convolution: fp16 NHWC in, fp32 NCHW out."""
        C = h.shape[1]
        t = self._gn(h, N, H * W, C, self._packed["gn_out"], None, True, groups, eps)
        out = torch.empty(N, self.out_channels, H, W, device=h.device)
        co = self._packed["conv_out"]
        hip.check(hip.lib().lfm_conv3x3_out_f32(hip.ptr(t), hip.ptr(co[0]), hip.ptr(co[1]), hip.ptr(out), N, H, W, C, self.out_channels,
                                                hip.stream_ptr(h.device)), "lfm_conv3x3_out_f32")
        return out

    def _time_embed(self, t, N, y, F, E):
        """lfm_time_embed: W2 silu(W0 [cos | sin](t) + b0) + b2 (+ label[y], the packed fp32 table; y None: no label term) -> its SiLU in fp16 [N, E], what
        every block's embedding projection reads."""
        table = self._packed["label"]
        n_labels = 0 if table is None else int(table.shape[0])
        label = None
        if y is not None:
            hip.check_labels(y, n_labels, self._what)
            label = table
        dev = t.device
        emb = torch.empty(N, E, device=dev)
        emb_silu = torch.empty(N, E, device=dev, dtype=torch.float16)
        h1 = torch.empty(N, E, device=dev)
        tw = self._packed["time"]
        hip.check(hip.lib().lfm_time_embed(hip.ptr(t), t.numel(), hip.ptr(tw[0]), hip.ptr(tw[1]), hip.ptr(tw[2]), hip.ptr(tw[3]), hip.ptr(label), hip.ptr(y),
                                           n_labels, hip.ptr(h1), hip.ptr(emb), hip.ptr(emb_silu), N, F, E, hip.stream_ptr(dev)), "lfm_time_embed")
        return emb_silu

    def _prologue(self, t, x, t_name):
        """The checks every forward starts with and the lazy pack.  Returns x as contiguous fp32 and t as fp32 [1] or [N]."""
        hip.require_gpu(x, self._what + ".forward")
        if self.training:
            raise hip.LfmHipError(f"the HIP {self._what_eval or self._what} is inference-only: call .eval()")
        if self._packed is None:
            self._pack()
        x = x.contiguous().float()
        t = torch.as_tensor(t, device=x.device).float().reshape(-1).contiguous()
        if t.numel() not in (1, x.shape[0]):
            raise ValueError(f"{t_name} must have 1 or {x.shape[0]} elements")
        return x, t
