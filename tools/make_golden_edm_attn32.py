"""Write tests/golden/edm_attn32.pt: the unmodified reference ``models/EDM.py::DhariwalUNet`` with attention at 32x32 and 16x16 on 32x32 latents.

    python tools/make_golden_edm_attn32.py      # needs the reference checkout (LFM_REFERENCE), not a GPU

The constructor default of DhariwalUNet attends at resolutions [32, 16, 8] (EDM.py:728); none of the fixtures of oracle/make_golden.py attends above
16x16.  Here: one 64-channel head over T = 1024 tokens at the top level (the streamed UNet attention kernel) and two over T = 256 below (the resident
kernel).  As golden_edm_full: the weights are regenerated on both sides from oracle.edm_state.load_seeded, so the fixture holds the configuration, the
seed, the checksum of the seeded state, the input and the reference's outputs only.
"""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CFG = dict(img_resolution=32, in_channels=4, out_channels=4, label_dim=0, augment_dim=0, model_channels=64, channel_mult=[1, 2], channel_mult_emb=4,
           num_blocks=1, attn_resolutions=[32, 16], dropout=0.0, label_dropout=0.0)
SEED = 64


def main():
    from oracle.edm_state import load_seeded
    from oracle.make_golden import OUT, _import_reference

    _import_reference()
    import models.EDM as ref_edm

    m = ref_edm.DhariwalUNet(**CFG).eval()
    checksum = load_seeded(m, SEED)
    x = torch.randn(2, 4, 32, 32, generator=torch.Generator().manual_seed(32))
    rec = {"cfg": CFG, "state_seed": SEED, "state_checksum": checksum, "x": x}
    with torch.no_grad():
        rec["v_t0d"] = m(torch.tensor(0.6), x[:1])
        rec["v_tN"] = m(torch.tensor([0.9, 0.3]), x)
    path = os.path.join(OUT, "edm_attn32.pt")
    torch.save(rec, path)
    print(path, os.path.getsize(path), "bytes; |v_tN| mean", float(rec["v_tN"].abs().mean()))


if __name__ == "__main__":
    main()
