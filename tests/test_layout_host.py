"""Host-side checks of the layout UNet (``UNetModelAttn``, lfm_amd/models/unet.py): ``create_network`` builds it with the reference's recorded parameter
tree, the constructor's head rule, the refusals that need no device, and the truth table of ``lfm_cross_attention_plan``.  No GPU."""
import os
from argparse import Namespace

import pytest
import torch

import layout_cases as lc


def _args(**kw):
    a = dict(use_origin_adm=True, layout=True, model_type="adm", image_size=128, f=8, num_in_channels=4, num_out_channels=4, nf=64, num_res_blocks=1,
             attn_resolutions=(1, 2), dropout=0.0, ch_mult=(1, 2), num_classes=None, num_heads=2, num_head_channels=-1, num_head_upsample=-1,
             use_scale_shift_norm=True, resblock_updown=False, use_new_attention_order=False)
    a.update(kw)
    return Namespace(**a)


def _rec(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location="cpu", weights_only=False)


def test_create_network_builds_the_reference_parameter_tree(golden_dir):
    from lfm_amd.models import create_network
    from lfm_amd.models.unet import UNetModel, UNetModelAttn

    rec = _rec(golden_dir, "layout_tiny.pt")
    m = create_network(_args())
    assert type(m) is UNetModelAttn and not isinstance(m, UNetModel)  # the captured fixed-grid solver, which passes no context, must not take it for one
    assert m.context_dim == 512 and m.transformer_depth == 3  # the reference's fixed --layout settings
    assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == rec["keys"]
    assert sum(p.numel() for p in m.parameters()) == rec["params"] == 9304900
    sd = lc.seeded_state(rec["keys"], rec["state_seed"])  # shaped as the reference's RECORDED list, not as this module: loads strictly
    gen = m._gen
    m.load_state_dict(sd, strict=True)
    assert m._gen > gen
    assert abs(lc.load_seeded(m) - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"]
    assert all(bool(v.any()) for v in m.state_dict().values())  # no tensor left at zero: every path of the network matters
    assert type(create_network(_args(layout=False))) is UNetModel
    self_rec = _rec(golden_dir, "layout_self.pt")
    assert [(k, tuple(v.shape)) for k, v in UNetModelAttn(**self_rec["cfg"]).state_dict().items()] == self_rec["keys"]


def test_head_rule_and_constructor_refusals():
    from lfm_amd.models.unet import SpatialTransformer, UNetModelAttn

    def heads(**kw):
        m = UNetModelAttn(**dict(lc.TINY_CFG, **kw))
        return [(t.in_channels, t.n_heads, t.d_head) for t in m.modules() if isinstance(t, SpatialTransformer)]

    assert heads() == [(64, 2, 32), (128, 2, 64), (128, 2, 64), (128, 2, 64), (128, 2, 64), (64, 2, 32), (64, 2, 32)]  # dim_head = ch // num_heads
    assert set(heads(num_heads=-1, num_head_channels=32)) == {(64, 2, 32), (128, 4, 32)}  # num_heads = ch // num_head_channels
    assert set(heads(num_heads=4, num_heads_upsample=1)) == {(64, 4, 16), (128, 4, 32)}  # the decoder's transformers take num_heads as well
    assert heads(legacy=False) == heads() and heads(context_dim=[512]) == heads()
    m = UNetModelAttn(**lc.TINY_CFG)
    b = m.middle_block[1].transformer_blocks[2]
    assert b.attn2.to_k.weight.shape == (128, 512) and b.attn1.to_k.weight.shape == (128, 128) and b.ff.net[0].proj.weight.shape == (1024, 128)
    assert not bool(m.middle_block[1].proj_out.weight.any()) and m.middle_block[1].norm.eps == 1e-6  # zero_module; Normalize's eps
    with pytest.raises(NotImplementedError, match="UNetModel"):
        UNetModelAttn(**dict(lc.TINY_CFG, use_spatial_transformer=False, context_dim=None))
    with pytest.raises(ValueError, match="context_dim"):
        UNetModelAttn(**dict(lc.TINY_CFG, context_dim=None))
    with pytest.raises(ValueError, match="num_heads"):
        UNetModelAttn(**dict(lc.TINY_CFG, num_heads=-1))
    with pytest.raises(NotImplementedError, match="% 16"):
        UNetModelAttn(**dict(lc.TINY_CFG, num_heads=8))  # heads of 8 channels: no attention kernel


def test_forward_refusals_need_no_device():
    from lfm_amd.models.unet import UNetModelAttn

    m = UNetModelAttn(**lc.TINY_CFG).eval()
    x = torch.zeros(1, 4, 16, 16)
    with pytest.raises(ValueError, match=r"\(64\).*\(512\)"):  # before any device call: x is a CPU tensor and nothing complains about that first
        m(torch.tensor(0.5), x)
    with pytest.raises(AssertionError, match="class-conditional"):
        m(torch.tensor(0.5), x, torch.zeros(1, 17, 512), y=torch.zeros(1, dtype=torch.long))
    with pytest.raises(Exception, match="inference-only|MI355X"):
        m.train()(torch.tensor(0.5), x, torch.zeros(1, 17, 512))
    with pytest.raises(NotImplementedError, match="forward_with_cfg"):
        m.forward_with_cfg(torch.tensor(0.5), x)
    import inspect

    assert list(inspect.signature(UNetModelAttn.forward).parameters)[:5] == ["self", "timesteps", "x", "context", "y"]  # the reference's argument order


def test_solver_does_not_capture_a_model_that_needs_a_context():
    from types import SimpleNamespace

    from lfm_amd.models.unet import UNetModelAttn
    from lfm_amd.solvers import fused_fixed_grid_available

    assert not fused_fixed_grid_available(UNetModelAttn(**lc.TINY_CFG).eval(), SimpleNamespace(is_cuda=True))


ERR = -1  # LFM_ERR_SHAPE


def test_cross_attention_plan_truth_table():
    from lfm_amd import hip

    tokens = (1, 17, 64, 65, 4096)
    for ch in (16, 32, 48, 64, 128, 256):
        for Tq in tokens:
            for Tk in tokens:
                assert hip.cross_attention_plan(3, Tq, Tk, 2, ch) == 1, (Tq, Tk, ch)
    for ch in (8, 40, 272):
        for Tq in tokens:
            assert hip.cross_attention_plan(3, Tq, 17, 2, ch) == ERR, (Tq, ch)
    for bad in ((0, 64, 17, 2, 64), (3, 0, 17, 2, 64), (3, 64, 0, 2, 64), (3, 64, 17, 0, 64), (3, 64, 17, 2, 0), (-1, 64, 17, 2, 64), (3, 64, -5, 2, 64)):
        assert hip.cross_attention_plan(*bad) == ERR, bad
    assert hip.cross_attention_plan(1 << 20, 4096, 17, 64, 64) == ERR  # 2^32 workgroups: past the grid
    with pytest.raises(hip.LfmHipError, match="% 16"):  # the wrapper names the limit before it touches a tensor's data
        hip.cross_attention(type("T", (), {"is_cuda": True})(), None, None, 3, 64, 17, 2, 40)
