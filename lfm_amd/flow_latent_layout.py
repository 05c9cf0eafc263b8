"""Sampling driver of the layout-to-image path with its conditioning stage: ``lfm_amd.test_flow_latent`` plus the token pipeline the reference leaves to its
callers.  The plain driver keeps the reference's argument surface, so the token flags live here, on a driver that takes every flag of that one and runs ITS
mode dispatch (``run_modes``), ``run_sampling``, solvers, lanes and image writers.

    python -m lfm_amd.flow_latent_layout --use_origin_adm --layout --layout_tokens tokens.npy [--cond_stage_ckpt FILE | --random_weights] <the driver's flags>

Five flags are added (absent from the reference):

    --layout_tokens FILE       .npy of int64 [K, L] token rows; sample j of the run is conditioned on row j % K
    --cond_stage_ckpt FILE     state dict of the encoder (keys transformer.*; the cond_stage_model. prefix of a whole LDM checkpoint is stripped), loaded strictly
    --cond_stage_layers 16  --cond_stage_vocab 8192  --cond_stage_max_len 92      the LDM layout-to-image conditioner; n_embed is the UNet's context_dim, 512

The tokens go through ``BERTEmbedder`` (lfm_amd/models/encoder.py) once per batch, before the solve.  The context reaches the model through a per-batch handle
(``Conditioned``) that adds ``context=`` to every evaluation, so the plain driver's ``run_sampling`` -- labels, guidance doubling, either solver family, the
null-half drop, the VAE decode -- runs as it is, not a copy of it."""
import torch

from . import test_flow_latent as tfl

__all__ = ["LayoutConditioner", "Conditioned", "build_cond_stage", "build_parser", "build_models", "run_sampling", "main"]


class Conditioned:
    """``model`` with the context of ONE batch bound to it: ``handle(t, x, **kw) == model(t, x, context=ctx, **kw)``.  Under guidance the drivers evaluate the
    doubled batch [conditional | null-label]: both halves then see the same context rows."""

    def __init__(self, model, context):
        self.model, self.context = model, context

    def _ctx(self, x):
        c = self.context
        if x.shape[0] == c.shape[0]:
            return c
        if x.shape[0] == 2 * c.shape[0]:
            return torch.cat([c, c], 0)
        raise ValueError(f"a batch of {x.shape[0]} against a context of {c.shape[0]} samples")

    def __call__(self, t, x, *args, **kwargs):
        return self.model(t, x, *args, context=self._ctx(x), **kwargs)

    def forward_with_cfg(self, t, x, *args, **kwargs):
        return self.model.forward_with_cfg(t, x, *args, context=self._ctx(x), **kwargs)

    def __getattr__(self, name):  # training flag, parameters(), device: whatever else a solver asks the model
        return getattr(self.model, name)


class LayoutConditioner:
    """Token rows [K, L] (``--layout_tokens``) and the BERTEmbedder that turns a batch of them into the context [n, L, 512] of ``UNetModelAttn``.  Sample j of
    the job takes row j % K.  One embedder handle per HIP stream (the drivers keep batches in flight on the lanes of ``make_lanes``, and two streams must not
    share a workspace): the first stream drives the embedder itself, every other one a concurrency twin on the same packed weights."""

    def __init__(self, embedder, tokens):
        self.embedder, self.tokens, self._by_stream, self._cursor = embedder, tokens, {}, 0

    def context(self, n):
        from .solvers import concurrency_twin

        rows = (torch.arange(n) + self._cursor) % self.tokens.shape[0]
        self._cursor = (self._cursor + n) % self.tokens.shape[0]
        dev = next(self.embedder.parameters()).device
        key = torch.cuda.current_stream(dev).cuda_stream
        if key not in self._by_stream:
            self._by_stream[key] = self.embedder if not self._by_stream else concurrency_twin(self.embedder)
        return self._by_stream[key](self.tokens[rows].to(dev))


def build_parser():
    p = tfl.build_parser()
    p.add_argument("--layout_tokens", type=str, default=None, help=".npy of int64 [K, L] token rows: sample j is conditioned on row j %% K through the layout "
                   "encoder (BERTEmbedder)")
    p.add_argument("--cond_stage_ckpt", type=str, default=None, help="state dict of the layout encoder (keys transformer.*; a cond_stage_model. prefix is stripped)")
    p.add_argument("--cond_stage_layers", type=int, default=16)
    p.add_argument("--cond_stage_vocab", type=int, default=8192)
    p.add_argument("--cond_stage_max_len", type=int, default=92)
    return p


def build_cond_stage(args, device):
    """``--layout_tokens FILE`` -> a LayoutConditioner over a BERTEmbedder(512, --cond_stage_layers, --cond_stage_vocab, --cond_stage_max_len) with the weights
    of ``--cond_stage_ckpt`` or, under ``--random_weights``, its seeded initialisation."""
    path = getattr(args, "layout_tokens", None)
    if not path:
        raise ValueError("this driver conditions the layout UNet on tokens: --layout_tokens FILE is required (without tokens, use lfm_amd.test_flow_latent)")
    if not (getattr(args, "use_origin_adm", False) and getattr(args, "layout", False)):
        raise ValueError("--layout_tokens conditions the layout UNet: it needs --use_origin_adm --layout")
    import numpy as np

    from .models import BERTEmbedder

    tokens = np.load(path, allow_pickle=False)
    if tokens.dtype != np.int64 or tokens.ndim != 2 or tokens.shape[0] < 1 or not 1 <= tokens.shape[1] <= args.cond_stage_max_len:
        raise ValueError(f"--layout_tokens {path}: expected int64 [K, L] with K >= 1 and 1 <= L <= --cond_stage_max_len = {args.cond_stage_max_len}, got "
                         f"{tokens.dtype} {tokens.shape}")
    if tokens.min() < 0 or tokens.max() >= args.cond_stage_vocab:
        raise ValueError(f"--layout_tokens {path}: ids span [{tokens.min()}, {tokens.max()}], the vocabulary is [0, {args.cond_stage_vocab})")
    emb = BERTEmbedder(512, args.cond_stage_layers, vocab_size=args.cond_stage_vocab, max_seq_len=args.cond_stage_max_len, use_tokenizer=False)
    if not args.random_weights:
        if not getattr(args, "cond_stage_ckpt", None):
            raise ValueError("--layout_tokens needs the conditioning stage's weights: --cond_stage_ckpt FILE (or --random_weights)")
        from .io_formats import load_state_dict_file

        sd = load_state_dict_file(args.cond_stage_ckpt, map_location="cpu", trust_checkpoint=getattr(args, "trust_checkpoint", False))
        prefix = "cond_stage_model."
        if any(k.startswith(prefix) for k in sd):
            sd = {k[len(prefix):]: v for k, v in sd.items() if k.startswith(prefix)}
        emb.load_state_dict(sd, strict=True)
    emb = emb.to(device).eval()
    emb._pack()  # on the stream the lanes wait for (make_lanes)
    return LayoutConditioner(emb, torch.from_numpy(tokens))


def build_models(args, device):
    """(model, vae, conditioner): the plain driver's models, then the conditioning stage -- under --random_weights its weights continue the same seeded stream."""
    model, vae = tfl.build_models(args, device)
    return model, vae, build_cond_stage(args, device)


def run_sampling(model, first_stage_model, cond, args, num_samples, generator, device, cls_index=None, x=None):
    """One batch: tokens -> context (once, before the solve), then the plain driver's ``run_sampling`` on the model with that context bound."""
    return tfl.run_sampling(Conditioned(model, cond.context(num_samples)), first_stage_model, args, num_samples, generator, device, cls_index=cls_index, x=x)


def main(argv=None):
    """The modes of ``lfm_amd.test_flow_latent.run_modes``, each evaluation through ``Conditioned``: the conditioner keeps one embedder handle per lane stream."""
    from .sampler.random_util import get_generator

    args = build_parser().parse_args(argv)
    device = tfl.set_up(args)
    model, vae, cond = build_models(args, device)
    tfl.run_modes(args, model, vae, get_generator(args.generator, args.n_sample, args.seed), device, bind=lambda m, n: Conditioned(m, cond.context(n)))


if __name__ == "__main__":
    main()
