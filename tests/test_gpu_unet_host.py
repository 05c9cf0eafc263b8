"""The host layer the three UNet backbones share (lfm_amd/models/_unet_host.py), on the GPU: per backbone, one tiny model evaluated twice and once more
through a ``concurrency_twin`` on a second stream -- the same bits three times, from the same packed weights and separate scratch."""
import os

import pytest
import torch

import song_cases as sc

pytestmark = pytest.mark.gpu


def _rec(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location="cpu", weights_only=False)


def _model_and_inputs(which, golden_dir, dev):
    """(model, t, x, y): the 64-channel 16x16 models of the unet_tiny / edm_tiny / song_tiny fixtures with the fixtures' weights and inputs."""
    from lfm_amd.models.EDM import DhariwalUNet, SongUNet
    from lfm_amd.models.unet import UNetModel

    if which == "UNetModel":
        rec = _rec(golden_dir, "unet_tiny.pt")["ssn"]
        m, t, y = UNetModel(**rec["cfg"]), rec["t"], None
        m.load_state_dict({k: v.float() for k, v in rec["state_dict"].items()}, strict=True)
    elif which == "DhariwalUNet":
        rec = _rec(golden_dir, "edm_tiny.pt")
        m, t, y = DhariwalUNet(**rec["cfg"]), torch.tensor([0.9, 0.5, 0.3, 0.05]), rec["y"]
        m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in rec["state_dict"].items()}, strict=True)
    else:
        rec = _rec(golden_dir, "song_tiny.pt")
        m, t, y = SongUNet(**rec["cfg"]), rec["tN"], rec["y"]
        sc.load_seeded(m, rec["state_seed"])
    return m.to(dev).eval(), t.to(dev), rec["x"].to(dev), y.to(dev) if y is not None else None


@pytest.mark.parametrize("which", ["UNetModel", "DhariwalUNet", "SongUNet"])
def test_unet_twin_on_a_second_stream_is_bit_identical(golden_dir, which):
    from lfm_amd.solvers import concurrency_twin

    dev = torch.device("cuda:0")
    m, t, x, y = _model_and_inputs(which, golden_dir, dev)
    want = m(t, x, y).clone()
    assert float(want.abs().mean()) > 1e-2
    again = m(t, x, y).clone()
    twin = concurrency_twin(m)
    assert twin._packed is m._packed and twin._scratch is None and twin._conv_ws is None
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(s):
        got = twin(t, x, y)
    s.synchronize()
    assert torch.equal(again, want) and torch.equal(got, want)
    assert twin._scratch is not None and twin._scratch is not m._scratch
