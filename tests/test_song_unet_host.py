"""Host-side checks of the ddpm++ backbone (``SongUNet``, lfm_amd/models/EDM.py) and of guided sampling on the fixed grids: the parameter tree against
the reference's recorded key / shape list, the refusals, the dispatch truth tables, and the float64 restatement of the mapping network against the
reference's own embedding (so that the GPU test's yardstick is itself pinned).  No GPU."""
import os
from argparse import Namespace
from types import SimpleNamespace

import pytest
import torch

import song_cases as sc


def _args(**kw):
    a = dict(use_origin_adm=False, model_type="ddpm++", image_size=128, f=8, num_in_channels=4, num_out_channels=4, label_dim=5, nf=64, ch_mult=(1, 2),
             num_res_blocks=1, attn_resolutions=(8,), dropout=0.0, label_dropout=0.0)
    a.update(kw)
    return Namespace(**a)


def _rec(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location="cpu", weights_only=False)


def test_create_network_builds_the_reference_parameter_tree(golden_dir):
    from lfm_amd.models import create_network
    from lfm_amd.models.EDM import SongUNet
    from oracle.edm_state import seeded_edm_state

    rec = _rec(golden_dir, "song_tiny.pt")
    m = create_network(_args())
    assert type(m) is SongUNet
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == rec["keys"]
    assert sum(p.numel() for p in m.parameters()) == rec["params"] == 2986116
    # a state dict shaped as the reference's (made from the RECORDED list, not from this module) loads strictly
    sd = seeded_edm_state(rec["keys"], rec["state_seed"])
    sd.update({k: torch.full(s, 0.25) for k, s in rec["keys"] if k.endswith("resample_filter")})
    gen = m._gen
    m.load_state_dict(sd, strict=True)
    assert m._gen > gen  # captured solver graphs of the old weights are dropped
    assert abs(sc.load_seeded(m) - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"]
    wide = _rec(golden_dir, "song_wide.pt")
    assert [(k, tuple(v.shape)) for k, v in SongUNet(**wide["cfg"]).state_dict().items()] == wide["keys"]


def test_song_unet_initialisers_follow_the_reference():
    from lfm_amd.models.EDM import SongUNet

    torch.manual_seed(3)
    m = SongUNet(**sc.TINY_CFG)
    b = m.dec["8x8_in0"]
    for w, fan, gain in ((b.conv0.weight, 2 * 128 * 9, 1.0), (b.conv1.weight, 2 * 128 * 9, 1e-5), (b.qkv.weight, 128 + 384, 0.2 ** 0.5),
                         (m.dec["16x16_aux_conv"].weight, (64 + 4) * 9, 1e-5), (m.map_layer0.weight, 64 + 256, 1.0)):
        w, bound = w.detach(), gain * (6.0 / fan) ** 0.5  # xavier-uniform: U(-bound, bound), std = bound / sqrt(3)
        assert float(w.abs().max()) <= bound and abs(float(w.std()) / (bound / 3 ** 0.5) - 1) < 0.05
    assert not bool(b.conv1.bias.any()) and b.skip_scale == pytest.approx(0.5 ** 0.5) and b.eps == 1e-6 and b.num_heads == 1
    assert m.enc["8x8_down"].skip.weight.shape == (64, 64, 1, 1)  # resample_proj: a 1x1 skip after the resample even at equal width
    assert [n for n, blk in m.dec.items() if getattr(blk, "num_heads", 0)] == ["8x8_in0", "8x8_block1"]  # the last block of a level, and in0


def test_what_is_not_built_is_refused_by_name():
    from lfm_amd.models import create_network
    from lfm_amd.models.EDM import DhariwalUNet, SongUNet, UNetBlock

    with pytest.raises(NotImplementedError, match="ncsn"):
        create_network(_args(model_type="ncsn++"))
    for setting, value in (("embedding_type", "fourier"), ("encoder_type", "residual"), ("encoder_type", "skip"), ("decoder_type", "skip"),
                           ("resample_filter", [1, 3, 3, 1]), ("channel_mult_noise", 2)):
        with pytest.raises(NotImplementedError, match=setting):
            SongUNet(**dict(sc.TINY_CFG, **{setting: value}))
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        SongUNet(**dict(sc.TINY_CFG, model_channels=96))
    with pytest.raises(NotImplementedError, match="256"):
        SongUNet(**dict(sc.TINY_CFG, model_channels=128, channel_mult=[1, 4], attn_resolutions=[]))  # in0 attends over 512 channels
    with pytest.raises(NotImplementedError, match="256"):
        SongUNet(**dict(sc.TINY_CFG, model_channels=320, channel_mult=[1, 1], attn_resolutions=[16]))
    SongUNet(16, 4, 4, num_blocks=1)  # the class defaults fit: 128 / 256 channels, attention at 256
    with pytest.raises(NotImplementedError, match="skip_scale"):
        UNetBlock(64, 64, 256, skip_scale=0.5 ** 0.5)  # lifted for SongUNet only
    assert not hasattr(SongUNet, "forward_with_cfg") and hasattr(DhariwalUNet, "forward_with_cfg")
    with pytest.raises(Exception, match="inference-only|MI355X"):
        SongUNet(**sc.TINY_CFG).train()(torch.tensor(0.5), torch.zeros(1, 4, 16, 16))


def test_fixed_grid_solver_accepts_song_unet_and_names_the_class_it_cannot_guide():
    from lfm_amd.models.EDM import SongUNet
    from lfm_amd.models.unet import UNetModel
    from lfm_amd.solvers import GraphedFixedGrid, fused_fixed_grid_available

    on_gpu = SimpleNamespace(is_cuda=True)  # the predicate reads nothing else of x
    m = SongUNet(**sc.TINY_CFG).eval()
    assert fused_fixed_grid_available(m, on_gpu)
    assert not fused_fixed_grid_available(m.train(), on_gpu)
    assert not fused_fixed_grid_available(m.eval(), SimpleNamespace(is_cuda=False))
    with pytest.raises(NotImplementedError, match="SongUNet"):
        GraphedFixedGrid(m, 2, y=torch.zeros(2, dtype=torch.long), cfg_scale=1.7, use_cfg=True, resolution=16)
    u = UNetModel(image_size=16, in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                  num_classes=5, num_heads=1).eval()
    with pytest.raises(NotImplementedError, match="UNetModel"):
        GraphedFixedGrid(u, 2, y=torch.zeros(2, dtype=torch.long), cfg_scale=1.7, use_cfg=True, resolution=16)


def test_mapping_network_float64_formula_matches_the_reference_embedding(golden_dir):
    """The reference's emb = silu(map_layer1(...)) (forward hook on the unmodified module, fp32) against the float64 restatement the GPU test uses."""
    from lfm_amd.models.EDM import SongUNet

    rec = _rec(golden_dir, "song_tiny.pt")
    m = SongUNet(**rec["cfg"])
    sc.load_seeded(m, rec["state_seed"])
    sd = m.state_dict()
    w = (sd["map_layer0.weight"], sd["map_layer0.bias"], sd["map_layer1.weight"], sd["map_layer1.bias"])
    lab = (sd["map_label.weight"], sd["map_label.bias"], rec["y"])
    for t, want in ((torch.tensor(0.6), rec["emb_t0d"]), (rec["tN"], rec["emb_tN"])):
        got = sc.song_mapping_ref64(*w, t, 4, *lab)
        err = float((got - want.double()).abs().max())
        print(f"t_len {t.numel()}: max |float64 formula - reference fp32 emb| = {err:.3e}")
        assert want.shape == (4, 256) and err < 2e-6  # fp32 round-off of a 256-term dot product of O(1) values; a wrong table or order is O(0.1)
    # the bound separates a wrong port: the table without the endpoint (f_i = 10000^(-i / (F/2))) is three orders of magnitude outside it
    d = torch.float64
    f_wrong = torch.pow(torch.tensor(1e-4, dtype=d), torch.arange(32, dtype=d) / 32)
    a = 0.6 * f_wrong
    e = torch.cat([a.sin(), a.cos()]).expand(4, 64) + 5 ** 0.5 * lab[0].to(d).t()[rec["y"]] + lab[1].to(d)
    wrong = sc.silu64(sc.silu64(e @ w[0].to(d).t() + w[1].to(d)) @ w[2].to(d).t() + w[3].to(d))
    assert float((wrong - rec["emb_t0d"].double()).abs().max()) > 1e-3


def test_conv3x3_plan_truth_table():
    """lfm_conv3x3_plan on the shapes the scaled-epilogue GPU test runs, and on their neighbours across each threshold."""
    from lfm_amd import hip

    L = hip.lib()
    assert hip.conv3x3_plan(4, 64, 64, 64, 512) == hip.CONV_PLAN_HALO  # 4 x 16 tiles x 4 channel blocks = 256 workgroups
    assert hip.conv3x3_plan(3, 64, 64, 64, 512) == hip.CONV_PLAN_GEMM  # 192: below one workgroup per CU
    assert hip.conv3x3_plan(4, 64, 64, 64, 512, mode=2) == hip.CONV_PLAN_GEMM  # stride 2 is never the halo kernel's
    assert hip.conv3x3_plan(4, 64, 60, 64, 512) == hip.CONV_PLAN_GEMM
    need = L.lfm_conv3x3_workspace_bytes(1, 9, 7, 128, 132)
    assert need == 2 * 63 * 132 * 4
    assert hip.conv3x3_plan(1, 9, 7, 128, 132, workspace_bytes=need) == hip.CONV_PLAN_SPLITK
    assert hip.conv3x3_plan(1, 9, 7, 128, 132, workspace_bytes=need - 4) == hip.CONV_PLAN_GEMM
    assert hip.conv3x3_plan(1, 9, 7, 128, 132) == hip.CONV_PLAN_GEMM
    assert L.lfm_conv3x3_workspace_bytes(1, 13, 11, 64, 132) == 0 and hip.conv3x3_plan(1, 13, 11, 64, 132, workspace_bytes=1 << 20) == hip.CONV_PLAN_GEMM
    assert hip.conv3x3_plan(1, 8, 8, 96, 128) < 0 and hip.conv3x3_plan(1, 7, 8, 64, 128, mode=1) < 0


def test_random_weights_redraw_the_1e5_scaled_tensors_too():
    """What the drivers do under --random_weights: create_network(args), then their re-draw of the all-zero tensors."""
    from lfm_amd.models import create_network
    from lfm_amd.test_flow_latent import dezero_

    plain = create_network(_args())
    assert 0 < float(plain.dec["16x16_aux_conv"].weight.detach().abs().max()) < 1e-5  # the reference's init_weight=1e-5: left alone without the flag
    m = dezero_(create_network(_args(random_weights=True)))
    for name, p in m.named_parameters():
        assert float(p.detach().abs().max()) > 1e-3, name  # N(0, 0.02) draws; the default "zero" convolutions would leave the model's output at ~6e-6
