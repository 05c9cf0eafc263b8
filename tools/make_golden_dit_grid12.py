"""Generate tests/golden/dit_grid12.pt by running the UNMODIFIED reference models/DiT.py on the CPU at a token grid of 12 x 12.

    python -m tools.make_golden_dit_grid12      # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

A depth-2 DiT with hidden 128, 2 heads (head_dim 64), img_resolution 24, patch 2: 144 tokens per image -- 2.25 key stages of the tiled attention kernel, the
last softmax block half full.  Writes data only: the configuration, seeded inputs and the reference's outputs (v for 0-d t, v for [N] t with labels,
forward_with_cfg).  The weights are NOT stored (0.8 M parameters = 3.3 MB, above the size a committed file may have): both sides regenerate them from the
seed with oracle.dit_ref.make_dit_state, as tests/golden/dit_hd72.pt does, and the fixture keeps a checksum.  That seeded state leaves no tensor at the
reference's zero initialisation (adaLN, final layer, biases), so every path of the network matters."""
import os

import torch

from oracle import dit_ref
from oracle.make_golden import OUT, _import_reference

SEED = 12
CFG = dict(depth=2, hidden=128, patch=2, heads=2, img_resolution=24, in_channels=4, num_classes=10, label_dropout=0.1)


def golden_dit_grid12(ref_dit):
    cfg = dit_ref.DiTCfg(**CFG)
    assert cfg.tokens == 144
    sd = dit_ref.make_dit_state(cfg, seed=SEED)
    assert all(bool(v.any()) for v in sd.values())  # de-zeroed
    m = ref_dit.DiT(img_resolution=24, patch_size=2, in_channels=4, hidden_size=128, depth=2, num_heads=2, num_classes=10, label_dropout=0.1).eval()
    m.load_state_dict(sd, strict=True)
    g = torch.Generator().manual_seed(SEED)
    x = torch.randn(3, 4, 24, 24, generator=g)
    y = torch.tensor([3, 0, 9])
    rec = {"cfg": CFG, "state_seed": SEED, "state_checksum": float(sum(v.double().abs().sum() for v in sd.values())), "x": x, "y": y,
           "t0": torch.tensor(0.37), "tN": torch.tensor([0.9, 0.5, 0.02])}
    with torch.no_grad():
        rec["v_t0d"] = m(rec["t0"], x)  # 0-d t, y=None: the null class row
        rec["v_tN"] = m(rec["tN"], x, y)
        x2 = torch.cat([x[:2], x[:2]], 0)
        y2 = torch.tensor([3, 7, 10, 10])
        rec["x_cfg"], rec["y_cfg"], rec["cfg_scale"] = x2, y2, 1.5
        rec["v_cfg"] = m.forward_with_cfg(rec["t0"], x2, y2, cfg_scale=1.5)
    return rec


def main():
    ref_dit, _, _ = _import_reference()
    path = os.path.join(OUT, "dit_grid12.pt")
    rec = golden_dit_grid12(ref_dit)
    torch.save(rec, path)
    print(path, os.path.getsize(path), "|v|", float(rec["v_tN"].abs().mean()))


if __name__ == "__main__":
    main()
