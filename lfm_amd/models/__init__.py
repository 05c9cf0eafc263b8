"""Model-constructor interface of the sampling path (drop-in for /root/reference/models/__init__.py:6-17)."""
from .DiT import DiT, DiT_models


def create_network(config):
    """``create_network(args) -> nn.Module`` with the reference's dispatch (models/__init__.py:6-17).

    DiT-*, ``--use_origin_adm`` (guided-diffusion ``UNetModel``; with ``--layout`` the ``UNetModelAttn`` whose attention blocks are
    SpatialTransformers with cross-attention over a 512-feature context), the EDM ``adm`` and ``adm_context`` (``DhariwalUNet``; the latter with ``use_context=True``), ``ddpm++``
    and ``ncsn++`` (``SongUNet`` with the DDPM++ settings or the whole NCSN++ preset; the latter reads ``config.num_blocks``, as in the
    reference) are built on the HIP path: every branch of the reference's dispatch.
    """
    if getattr(config, "use_origin_adm", False):
        return get_flow_model(config)
    if "DiT" not in config.model_type:
        from .EDM import get_edm_network

        return get_edm_network(config)
    return DiT_models[config.model_type](
        img_resolution=config.image_size // config.f,
        in_channels=config.num_in_channels,
        label_dropout=config.label_dropout,
        num_classes=config.num_classes,
    )


def get_flow_model(config):
    """Origin-ADM constructor (reference models/__init__.py:20-70): ``UNetModel``, or ``UNetModelAttn`` under ``--layout``.  Flags the ``_ddp`` parser forgets
    (``use_scale_shift_norm`` etc., test_flow_latent_ddp.py:210-212) default to the single-file parser's values."""
    from .unet import UNetModel, UNetModelAttn

    # --layout: the reference's fixed SpatialTransformer settings (models/__init__.py:42-45)
    layout = dict(use_spatial_transformer=True, transformer_depth=3, context_dim=512, legacy=True) if getattr(config, "layout", False) else {}
    return (UNetModelAttn if layout else UNetModel)(
        image_size=config.image_size // 8,
        in_channels=config.num_in_channels,
        model_channels=config.nf,
        out_channels=config.num_out_channels,
        num_res_blocks=config.num_res_blocks,
        attention_resolutions=config.attn_resolutions,
        dropout=config.dropout,
        channel_mult=config.ch_mult,
        conv_resample=getattr(config, "resamp_with_conv", True),
        dims=2,
        num_classes=config.num_classes,
        use_checkpoint=False,
        use_fp16=False,
        num_heads=config.num_heads,
        num_head_channels=config.num_head_channels,
        num_heads_upsample=getattr(config, "num_head_upsample", -1),
        use_scale_shift_norm=getattr(config, "use_scale_shift_norm", True),
        resblock_updown=getattr(config, "resblock_updown", False),
        use_new_attention_order=getattr(config, "use_new_attention_order", False),
        **layout,
    )


def __getattr__(name):
    """``lfm_amd.models.BERTEmbedder`` (the layout encoder, models/encoder.py), imported on first use like the UNets: a DiT-only user loads nothing more."""
    if name == "BERTEmbedder":
        from .encoder import BERTEmbedder

        return BERTEmbedder
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


__all__ = ["create_network", "get_flow_model", "DiT", "DiT_models", "BERTEmbedder"]
