"""The layout encoder of ``--layout``: ``BERTEmbedder`` (reference models/encoder.py:52-87 over models/x_transformer.py ``TransformerWrapper`` + ``Encoder``),
tokens [N, L] -> the context [N, L, n_embed] that ``UNetModelAttn``'s cross-attention reads.  Same constructor, same parameter tree and state-dict keys as
the reference, so the conditioning stage of a layout-to-image checkpoint loads with ``strict=True``.

On the device the residual stream is fp16 rows [N*L, n_embed] (as in the SpatialTransformer; the UNet projects the context from fp16 anyway):

    lfm_token_embed_f16                      token_emb[ids] + pos_emb[:L], fp32 add, one rounding
    per layer pair (pre-norm, x_transformer.py:476-502):
      lfm_layernorm_f16 -> lfm_linear_f16 over the row-stacked [to_q | to_k | to_v] (no bias) into one [M, 1536] buffer
        -> lfm_cross_attention_f16 on its three column slices (ldq = ldkv = 1536, Tq = Tk = L, 8 heads of 64 whatever n_embed is: x_transformer.py:211-212, 230)
        -> lfm_linear_f16 (to_out) + residual
      lfm_layernorm_f16 -> lfm_linear_gelu_f16 (net.0.0 with the exact GELU of nn.GELU() in the epilogue) -> lfm_linear_f16 (net.2) + residual
    lfm_layernorm_f16                        the final norm, into the returned tensor

``BERTEmbedder.forward`` passes no mask (encoder.py:82), so every token attends over all L tokens of its image and there is no mask argument anywhere.
Every op is enqueued on torch's current stream; no PyTorch compute ops."""
import torch
import torch.nn as nn

from .. import hip
from ._unet_host import PackedModule, f16, f32, pack_gn

HEADS, DIM_HEAD = 8, 64  # Attention's defaults, which Encoder(dim=, depth=) never overrides (x_transformer.py:14, 211-212)
INNER = HEADS * DIM_HEAD


class BERTTokenizer(nn.Module):
    """encoder.py:16-49 with vq_interface=False: the pretrained ``bert-base-uncased`` tokenizer, imported when it is constructed, from the local cache only."""

    def __init__(self, device="cuda", max_length=77):
        super().__init__()
        try:
            from transformers import BertTokenizerFast

            self.tokenizer = BertTokenizerFast.from_pretrained("bert-base-uncased", local_files_only=True)
        except Exception as e:  # noqa
            raise RuntimeError("BERTEmbedder(use_tokenizer=True) needs the `transformers` package and the bert-base-uncased tokenizer files in its local cache "
                               f"(nothing is downloaded here): {type(e).__name__}: {e}.  Tokenise elsewhere and pass use_tokenizer=False with int64 tokens "
                               "[N, L].") from e
        self.device, self.max_length = device, max_length

    def forward(self, text):
        enc = self.tokenizer(text, truncation=True, max_length=self.max_length, return_length=True, return_overflowing_tokens=False, padding="max_length",
                             return_tensors="pt")
        return enc["input_ids"].to(self.device)


class AbsolutePositionalEmbedding(nn.Module):  # x_transformer.py:21-32
    def __init__(self, dim, max_seq_len):
        super().__init__()
        self.emb = nn.Embedding(max_seq_len, dim)
        nn.init.normal_(self.emb.weight, std=0.02)


class Attention(nn.Module):  # x_transformer.py:207-258 at its defaults
    def __init__(self, dim):
        super().__init__()
        self.to_q = nn.Linear(dim, INNER, bias=False)
        self.to_k = nn.Linear(dim, INNER, bias=False)
        self.to_v = nn.Linear(dim, INNER, bias=False)
        self.to_out = nn.Linear(INNER, dim)


class FeedForward(nn.Module):  # x_transformer.py:193-203 with glu=False, mult=4
    def __init__(self, dim, mult=4):
        super().__init__()
        self.net = nn.Sequential(nn.Sequential(nn.Linear(dim, dim * mult), nn.GELU()), nn.Dropout(0.0), nn.Linear(dim * mult, dim))


class Residual(nn.Module):  # x_transformer.py:164-166 (no parameters; keeps the reference's [norm, layer, residual] triples)
    pass


class Encoder(nn.Module):  # x_transformer.py:359-526: ("a", "f") * depth, pre-norm LayerNorm
    def __init__(self, dim, depth):
        super().__init__()
        self.dim, self.depth = dim, depth
        self.layers = nn.ModuleList([nn.ModuleList([nn.LayerNorm(dim), Attention(dim) if kind == "a" else FeedForward(dim), Residual()])
                                     for _ in range(depth) for kind in ("a", "f")])


class TransformerWrapper(nn.Module):  # x_transformer.py:529-617
    def __init__(self, num_tokens, max_seq_len, attn_layers):
        super().__init__()
        dim = attn_layers.dim
        self.max_seq_len, self.num_tokens = max_seq_len, num_tokens
        self.token_emb = nn.Embedding(num_tokens, dim)
        self.pos_emb = AbsolutePositionalEmbedding(dim, max_seq_len)
        self.attn_layers = attn_layers
        self.norm = nn.LayerNorm(dim)
        nn.init.normal_(self.token_emb.weight, std=0.02)
        self.to_logits = nn.Linear(dim, num_tokens)  # in every reference checkpoint; return_embeddings=True never runs it


class BERTEmbedder(PackedModule):
    """``BERTEmbedder(n_embed, n_layer, vocab_size=30522, max_seq_len=77, device="cuda", use_tokenizer=True, embedding_dropout=0.0)`` (encoder.py:52-87):
    ``forward(tokens)`` / ``encode(tokens)`` take int64 [N, L] on the GPU with L <= max_seq_len (or, with ``use_tokenizer=True``, a list of strings) and return
    the context fp16 [N, L, n_embed].  State-dict keys are the reference's (``transformer.{token_emb,pos_emb.emb,attn_layers.layers.i.{0,1.*},norm,
    to_logits}``); ``to_logits`` is loaded and never used.  Inference only; dropout is the identity.

    The workspace (residual rows, the LayerNorm output, the [M, 1536] QKV buffer, the attention output, the [M, 4 n_embed] hidden rows) is carved once per
    (N, L) and reused.  THE RESULT IS A FRESHLY ALLOCATED TENSOR ON EVERY EAGER CALL, never a view of that workspace: ``UNetModelAttn`` caches the K | V
    projection of a context on (data_ptr, _version, shape, ...), and kernels that write through raw pointers do not bump ``_version`` -- an embedder that
    handed out the same storage twice with different contents would make the UNet reuse the projection of the previous tokens.  The UNet keeps the cached
    tensor alive, so its address cannot come back for another context either (tests/test_gpu_layout_encoder.py::
    test_unet_does_not_reuse_the_projection_of_earlier_tokens).  Inside a ``torch.cuda.graph`` capture the result is the graph's own static output; a replay
    follows tokens rewritten in place (the ids are read on the device), and the UNet projects the context inside the graph."""

    _scratch_attrs = ("_ws", "_ws_key")

    def __init__(self, n_embed, n_layer, vocab_size=30522, max_seq_len=77, device="cuda", use_tokenizer=True, embedding_dropout=0.0):
        super().__init__()
        if n_embed <= 0 or n_embed % 64:
            raise NotImplementedError(f"BERTEmbedder with n_embed={n_embed}: the GEMM kernels take reduction lengths % 64 == 0, so n_embed % 64 == 0 is built")
        self.n_embed, self.n_layer, self.vocab_size, self.max_seq_len = int(n_embed), int(n_layer), int(vocab_size), int(max_seq_len)
        self.use_tknz_fn = use_tokenizer
        if self.use_tknz_fn:
            self.tknz_fn = BERTTokenizer(device=device, max_length=max_seq_len)
        self.device = device
        self.transformer = TransformerWrapper(num_tokens=vocab_size, max_seq_len=max_seq_len, attn_layers=Encoder(dim=n_embed, depth=n_layer))
        self._init_host_state()

    # ---- packing ------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def _pack(self):
        tr = self.transformer
        dev = tr.token_emb.weight.device
        hip.require_gpu(tr.token_emb.weight, "BERTEmbedder")
        lin = lambda l: (f16(l.weight, dev), f32(l.bias, dev))  # noqa: E731
        layers = []
        for i in range(self.n_layer):
            (n1, at, _), (n2, ff, _) = tr.attn_layers.layers[2 * i], tr.attn_layers.layers[2 * i + 1]
            layers.append(dict(ln1=pack_gn(n1, dev), ln2=pack_gn(n2, dev), eps=(n1.eps, n2.eps),
                               qkv=f16(torch.cat([at.to_q.weight, at.to_k.weight, at.to_v.weight], 0), dev),  # rows [q | k | v], each [head][ch]
                               out=lin(at.to_out), ff1=lin(ff.net[0][0]), ff2=lin(ff.net[2])))
        self._packed = dict(tok=f32(tr.token_emb.weight, dev), pos=f32(tr.pos_emb.emb.weight, dev), layers=layers, norm=pack_gn(tr.norm, dev), eps=tr.norm.eps)
        self._gen += 1
        return self._packed

    def _workspace(self, N, L, dev):
        """One fp16 buffer per (N, L, device), carved into the six row buffers of a forward."""
        key = (N, L, dev)
        if self._ws is None or self._ws_key != key:  # (None with a key: a concurrency twin, which takes its own carve)
            M, D = N * L, self.n_embed
            widths = dict(x0=D, x1=D, t=D, qkv=3 * INNER, a=INNER, h=4 * D)
            rows = (M + 7) // 8 * 8  # every buffer starts 16-byte aligned whatever M is
            buf = torch.empty(rows * sum(widths.values()), dtype=torch.float16, device=dev)
            ws, off = {}, 0
            for name, w in widths.items():
                ws[name] = buf[off:off + M * w].view(M, w)
                off += rows * w
            self._ws, self._ws_key = ws, key
            self._gen += 1
        return self._ws

    @staticmethod
    def _linear(x, w, bias, out, resid=None):
        M, K = x.shape
        hip.check(hip.lib().lfm_linear_f16(hip.ptr(x), x.stride(0), hip.ptr(w), w.stride(0), hip.ptr(out), out.stride(0), M, w.shape[0], K, hip.ptr(bias),
                                           hip.ptr(resid), hip.stream_ptr(x.device)), "lfm_linear_f16")
        return out

    # ---- forward -------------------------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, text):
        tokens = self.tknz_fn(text) if self.use_tknz_fn else text
        if not torch.is_tensor(tokens) or tokens.dim() != 2 or tokens.dtype != torch.int64:
            raise ValueError(f"BERTEmbedder: tokens must be an int64 tensor [N, L], got {getattr(tokens, 'dtype', type(tokens))} "
                             f"{tuple(tokens.shape) if torch.is_tensor(tokens) else ''}")
        N, L = tokens.shape
        if N < 1 or L < 1 or L > self.max_seq_len:
            raise ValueError(f"BERTEmbedder: {L} tokens per sequence; the position table has max_seq_len = {self.max_seq_len} rows (and N, L >= 1)")
        hip.require_gpu(tokens, "BERTEmbedder.forward (tokens)")
        if self.training:
            raise hip.LfmHipError("the HIP BERTEmbedder is inference-only: call .eval()")
        if self._packed is None:
            self._pack()
        P, dev = self._packed, tokens.device
        if P["tok"].device != dev:
            raise hip.LfmHipError(f"BERTEmbedder: tokens on {dev}, weights on {P['tok'].device}")
        # the reference's nn.Embedding raises IndexError; one readback per token tensor, remembered on it; skipped under capture, where a replay gets NaN rows instead
        hip.check_labels(tokens, self.vocab_size, "BERTEmbedder", noun="token", table="the vocabulary", hint="")
        ws = self._workspace(N, L, dev)
        x, x_alt, t, qkv, a, h = ws["x0"], ws["x1"], ws["t"], ws["qkv"], ws["a"], ws["h"]
        hip.token_embed(P["tok"], P["pos"], tokens.contiguous(), out=x)
        q, k, v = qkv[:, :INNER], qkv[:, INNER:2 * INNER], qkv[:, 2 * INNER:]
        for p in P["layers"]:
            hip.layernorm(x, *p["ln1"], eps=p["eps"][0], out=t)
            self._linear(t, p["qkv"], None, qkv)
            hip.cross_attention(q, k, v, N, L, L, HEADS, DIM_HEAD, out=a)
            self._linear(a, *p["out"], x_alt, resid=x)
            x, x_alt = x_alt, x
            hip.layernorm(x, *p["ln2"], eps=p["eps"][1], out=t)
            hip.linear_gelu(t, *p["ff1"], out=h)
            self._linear(h, *p["ff2"], x_alt, resid=x)
            x, x_alt = x_alt, x
        out = torch.empty(N, L, self.n_embed, dtype=torch.float16, device=dev)  # fresh per call: see the class docstring
        hip.layernorm(x, *P["norm"], eps=P["eps"], out=out.view(N * L, self.n_embed))
        return out

    def encode(self, text):
        return self(text)
