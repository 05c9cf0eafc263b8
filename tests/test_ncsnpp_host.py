"""Host-side checks of the NCSN++ preset of ``SongUNet`` (lfm_amd/models/EDM.py): the parameter tree against the reference's recorded key / shape list, the
refusals that remain, and the float64 restatements of the three [1,3,3,1] resampling cases and of the Fourier mapping network (tests/ncsnpp_cases.py)
against the reference's own outputs (tests/golden/ncsnpp_tiny.pt, tools/make_ncsnpp_golden.py) -- so that the GPU tests' yardsticks are themselves pinned --
with the seeded faults those bounds separate.  No GPU."""
import itertools
import os
from argparse import Namespace

import pytest
import torch

import ncsnpp_cases as nc
import song_cases as sc


def _args(**kw):
    a = dict(use_origin_adm=False, model_type="ncsn++", image_size=128, f=8, num_in_channels=4, num_out_channels=4, label_dim=5, nf=64, ch_mult=(1, 2, 2),
             num_res_blocks=7, num_blocks=1, attn_resolutions=(8,), dropout=0.0, label_dropout=0.0)
    a.update(kw)
    return Namespace(**a)


@pytest.fixture(scope="module")
def rec(golden_dir):
    return torch.load(os.path.join(golden_dir, "ncsnpp_tiny.pt"), map_location="cpu", weights_only=False)


def test_ncsnpp_builds_the_reference_parameter_tree_and_loads_its_state_strictly(rec):
    from lfm_amd.models import create_network
    from lfm_amd.models.EDM import SongUNet
    from oracle.edm_state import seeded_edm_state

    assert rec["cfg"] == nc.TINY_CFG
    for m in (SongUNet(**nc.TINY_CFG), create_network(_args())):  # num_blocks is what the preset reads, not num_res_blocks (7 here)
        assert type(m) is SongUNet
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == rec["keys"]
        assert sum(p.numel() for p in m.parameters()) == rec["params"]
    keys = [k for k, _ in rec["keys"]]
    assert keys[0] == "map_noise.freqs" and {"enc.8x8_aux_residual.weight", "enc.4x4_aux_residual.resample_filter"} <= set(keys)
    f = torch.tensor([1.0, 3.0, 3.0, 1.0])
    for k in ("enc.8x8_down.conv0.resample_filter", "enc.8x8_aux_residual.resample_filter", "dec.8x8_up.skip.resample_filter"):
        assert torch.equal(m.state_dict()[k], (f.ger(f) / 64).reshape(1, 1, 4, 4)), k  # the reference's shape and values
    assert m.enc["8x8_aux_residual"].weight.shape == (64, 4, 3, 3) and m.enc["4x4_aux_residual"].weight.shape == (128, 64, 3, 3)
    # a state dict shaped as the reference's (made from the RECORDED list, not from this module) loads strictly, buffers included
    sd = seeded_edm_state(rec["keys"], rec["state_seed"])
    sd.update({k: torch.full(s, 0.25) for k, s in rec["keys"] if k.endswith("resample_filter")})
    assert sd["map_noise.freqs"].shape == (64,)
    m._packed, gen = "sentinel", m._gen
    m.load_state_dict(sd, strict=True)
    assert m._gen > gen and m._packed is None  # captured solver graphs and the pack of the old weights (the old frequency table among them) are dropped
    assert torch.equal(m.map_noise.freqs, sd["map_noise.freqs"])
    assert abs(nc.load_seeded(m) - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"]
    assert torch.equal(m.map_noise.freqs, nc.seeded_freqs(64)) and float(m.map_noise.freqs.abs().max()) > 20  # beyond the first period at t <= 1


def test_only_the_two_presets_are_built():
    from lfm_amd.models import create_network
    from lfm_amd.models.EDM import SongUNet
    from lfm_amd.solvers import fused_fixed_grid_available
    from types import SimpleNamespace

    order = ["embedding_type", "channel_mult_noise", "encoder_type", "decoder_type", "resample_filter"]
    departs = [k for k in order if nc.NCSNPP[k] != sc.TINY_CFG[k]]  # decoder_type is "standard" in both presets
    assert departs == ["embedding_type", "channel_mult_noise", "encoder_type", "resample_filter"]
    n = 0
    for r in range(1, len(departs)):
        for subset in itertools.combinations(departs, r):  # every proper subset of the preset's settings: refused by the name of its first departure
            with pytest.raises(NotImplementedError, match=f"^SongUNet: {subset[0]}="):
                SongUNet(**dict(sc.TINY_CFG, **{k: nc.NCSNPP[k] for k in subset}))
            n += 1
    assert n == 14
    for setting in ("encoder_type", "decoder_type"):  # the two `skip` types: refused by name beside DDPM++, and refused beside the rest of the preset
        with pytest.raises(NotImplementedError, match=f"^SongUNet: {setting}='skip'"):
            SongUNet(**dict(sc.TINY_CFG, **{setting: "skip"}))
        with pytest.raises(NotImplementedError):
            SongUNet(**dict(nc.TINY_CFG, **{setting: "skip"}))
    with pytest.raises(NotImplementedError, match="augment_dim"):
        SongUNet(**dict(nc.TINY_CFG, augment_dim=9))
    for bad in (dict(num_blocks=None), {}):
        a = vars(_args(**bad))
        if not bad:
            del a["num_blocks"]
        with pytest.raises(NotImplementedError, match="(?s)ncsn.*num_blocks"):
            create_network(Namespace(**a))
    # the width, head and boundary-channel checks hold for both presets
    with pytest.raises(NotImplementedError, match="multiples of 64"):
        SongUNet(**dict(nc.TINY_CFG, model_channels=96))
    with pytest.raises(NotImplementedError, match="256"):
        SongUNet(**dict(nc.TINY_CFG, model_channels=128, channel_mult=[1, 4], attn_resolutions=[]))
    with pytest.raises(NotImplementedError, match="16 input"):
        SongUNet(**dict(nc.TINY_CFG, in_channels=17))
    m = SongUNet(**nc.TINY_CFG).eval()
    assert fused_fixed_grid_available(m, SimpleNamespace(is_cuda=True)) and not hasattr(m, "forward_with_cfg")


def test_driver_arguments_plus_num_blocks_build_the_preset_and_random_weights_redraw_the_small_tensors():
    """The drivers' parser has no --num_blocks (as the reference's has none): its namespace refuses ncsn++ by name, and with num_blocks set from code it
    builds the preset, --random_weights redrawing the 1e-5-scaled tensors as for ddpm++."""
    from lfm_amd.models import create_network
    from lfm_amd.test_flow_latent import build_parser, dezero_

    args = build_parser().parse_args(["--model_type", "ncsn++", "--image_size", "128", "--f", "8", "--num_in_channels", "4", "--num_out_channels", "4", "--nf",
                                      "64", "--ch_mult", "1", "2", "--attn_resolutions", "8", "--random_weights"])
    with pytest.raises(NotImplementedError, match="(?s)ncsn.*num_blocks"):
        create_network(args)
    args.num_blocks = 1
    assert args.num_res_blocks == 2
    m = dezero_(create_network(args))
    assert "8x8_aux_residual" in m.enc and "16x16_block1" not in m.enc
    for name, p in m.named_parameters():
        assert float(p.detach().abs().max()) > 1e-3, name


def test_float64_restatements_match_the_reference_conv2d_and_the_faults_do_not(rec):
    """The reference's own Conv2d under the [1,3,3,1] filter (fp32, on seeded inputs) against the float64 restatements the GPU tests compare the kernels
    with: 1e-6 absolute on O(1) data; each seeded fault is orders of magnitude outside."""
    x, w, b = nc.conv_record_inputs()
    xh, c = nc.nhwc(x), rec["conv2d"]
    assert torch.equal(c["resample_filter"].reshape(4, 4), torch.tensor(nc.F4).ger(torch.tensor(nc.F4)) / 64)
    want = {k: nc.nhwc(c[k]).double() for k in ("down", "up", "fused_down")}
    assert want["down"].shape == (1, 3, 5, 8) and want["up"].shape == (1, 12, 20, 8) and want["fused_down"].shape == (1, 3, 5, 8)
    got = {"down": nc.fir_down_ref64(xh, 1), "up": nc.fir_up_ref64(xh), "fused_down": nc.fused_down_ref64(xh, w, b)}
    faults = {"down": ("pad 0 on a cropped map", torch.nn.functional.pad(nc.fir_down_ref64(xh, 0), (0, 0, 0, 1, 0, 1))),
              "up": ("taps [1,3,3,1]/8 without the x2 per axis", nc.fir_up_ref64(xh, per_axis_gain=1.0)),
              "fused_down": ("pad 1, filter first", nc.fused_down_ref64(xh, w, b, fault="filter_first"))}
    for k in want:
        err, (what, bad) = float((got[k] - want[k]).abs().max()), faults[k]
        ferr = float((bad - want[k]).abs().max())
        print(f"{k}: max |float64 restatement - reference fp32| = {err:.3e}; fault ({what}) = {ferr:.3e}; |ref| max {float(want[k].abs().max()):.2f}")
        assert err < 1e-6 < 1e-2 < ferr, k


def test_the_bias_may_stand_on_either_side_of_the_unpadded_filter(rec):
    """The fourth fault the issue lists, "the bias added before the filter", is NOT one on the fused path: f2 sums to 1 and that filter stage has no padding,
    so filter(conv + b) == filter(conv) + b exactly; the two restatements agree to float64 round-off, and both match the reference.  (On the pad-1 path a
    bias before the filter WOULD differ along the border -- measured here too -- but that path's Conv2d has no bias: kernel 0.)  What the kernel's late bias
    must not do is enter before a PADDED filter, and the composed GPU test's filter-first fault covers that stage order."""
    x, w, b = nc.conv_record_inputs()
    xh, want = nc.nhwc(x), nc.nhwc(rec["conv2d"]["fused_down"]).double()
    late, early = nc.fused_down_ref64(xh, w, b), nc.fused_down_ref64(xh, w, b, fault="bias_first")
    d_same, d_ref = float((late - early).abs().max()), float((early - want).abs().max())
    padded = float((nc.fir_down_ref64(xh + b, 1) - (nc.fir_down_ref64(xh, 1) + b.double())).abs().max())
    print(f"bias before vs after the unpadded filter: {d_same:.3e}; bias-first vs the reference: {d_ref:.3e}; before vs after a PADDED filter: {padded:.3e}")
    assert d_same < 1e-14 and d_ref < 1e-6 and padded > 1e-2


def test_fourier_mapping_float64_formula_matches_the_reference_embedding(rec):
    """The reference's emb = silu(map_layer1(...)) (forward hook on the unmodified module, fp32) against the float64 restatement the GPU test uses."""
    from lfm_amd.models.EDM import SongUNet

    m = SongUNet(**rec["cfg"])
    nc.load_seeded(m, rec["state_seed"])
    sd = m.state_dict()
    w = (sd["map_noise.freqs"], sd["map_layer0.weight"], sd["map_layer0.bias"], sd["map_layer1.weight"], sd["map_layer1.bias"])
    lab = (sd["map_label.weight"], sd["map_label.bias"], rec["y"])
    N = rec["x"].shape[0]
    assert float(nc.fourier_args32(torch.tensor(0.6), w[0]).abs().max()) > 100  # radians: far outside the first period
    for t, want in ((torch.tensor(0.6), rec["emb_t0d"]), (rec["tN"], rec["emb_tN"])):
        got = nc.fourier_mapping_ref64(*w, t, N, *lab)
        err = float((got - want.double()).abs().max())
        wrong = float((nc.fourier_mapping_ref64(*w, t, N, *lab, swap=False) - want.double()).abs().max())
        print(f"t_len {t.numel()}: max |float64 formula - reference fp32 emb| = {err:.3e}; un-swapped [cos | sin] = {wrong:.3e}")
        # fp32 round-off of a 256-term dot product of O(1) values (the DDPM++ embedding's bound); the un-swapped order is O(0.1)
        assert want.shape == (N, 256) and err < 2e-6 and wrong > 1e-3
