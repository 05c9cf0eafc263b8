"""Generate tests/golden/ncsnpp_tiny.pt by running the UNMODIFIED reference models/EDM.py on the CPU.

    python -m tools.make_ncsnpp_golden          # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Writes data only, as tools/make_song_golden.py does for ddpm++: the NCSN++ configuration (tests/ncsnpp_cases.py), the seed and checksum of the state both
sides regenerate, the reference's key / shape list, seeded inputs and the reference's outputs -- v at a scalar and at a per-sample time, the label_dim = 0
model on the same weights, the mapping network's output (hook on map_layer1), ten Euler steps -- and the outputs of three stand-alone instances of the
reference's own Conv2d under the [1,3,3,1] filter on seeded inputs (kernel 0 down, kernel 0 up, kernel 3 down with fused_resample and a non-zero bias),
whose inputs and weights ncsnpp_cases.conv_record_inputs regenerates."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ncsnpp_cases as nc  # noqa: E402
from oracle.make_golden import OUT, _import_reference  # noqa: E402
from tools.make_song_golden import golden_song  # noqa: E402


def golden_conv2d(ref_edm):
    x, w, b = nc.conv_record_inputs()
    f = nc.NCSNPP["resample_filter"]
    down = ref_edm.Conv2d(8, 8, kernel=0, down=True, resample_filter=f)
    up = ref_edm.Conv2d(8, 8, kernel=0, up=True, resample_filter=f)
    fused = ref_edm.Conv2d(8, 8, kernel=3, down=True, resample_filter=f, fused_resample=True)
    with torch.no_grad():
        fused.weight.copy_(w)
        fused.bias.copy_(b)
        return {"down": down(x.clone()), "up": up(x.clone()), "fused_down": fused(x.clone()), "resample_filter": down.resample_filter.clone()}


def main():
    _import_reference()
    import models.EDM as ref_edm

    rec = golden_song(ref_edm, nc.TINY_CFG, 3, True, load=nc.load_seeded)  # batch 3: the file stays under the size of song_tiny.pt
    rec["freqs_seed"] = nc.FREQS_SEED
    rec["conv2d"] = golden_conv2d(ref_edm)
    torch.save(rec, os.path.join(OUT, "ncsnpp_tiny.pt"))


if __name__ == "__main__":
    main()
