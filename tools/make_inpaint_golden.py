"""Generate tests/golden/inpaint_prep.pt by running the UNMODIFIED reference's inpainting dataset class and loop lines
(downstream_tasks/test_flow_latent_inpainting.py) on the CPU.

    python -m tools.make_inpaint_golden          # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Three 64 x 64 JPEG / PNG pairs (tests/inpaint_cases.py: golden_pairs; mask bytes 255, 0 and greys) are written to a temporary directory in the reference's
naming, and ``CustomizedInpaintingEvalDataset.__getitem__`` reads them back.  The loop's lines :148-150 (the mask onto the latent grid, the cat) and :157-160
(the three to_range_0_1 and the composite) run as they stand in the file, on a seeded latent ``c`` and a seeded ``fake_image``.  Writes data only: the bytes the
files decode to, the reference's img / mask / masked_img, cc and the 5-channel tensor, the composite and the bytes torchvision.utils.save_image makes of it
(its conversion mul(255).add_(0.5).clamp_(0, 255).to(uint8) applied here: torchvision is not needed for it), and the defaults the reference driver's own
argument parser returns.

The reference module imports torchvision, diffusers and torchdiffeq at its top and uses none of them in what runs here; where they are missing, empty
stand-in modules of those names are registered before the import."""
import argparse
import os
import sys
import tempfile
import types

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import inpaint_cases as ic  # noqa: E402
from oracle.make_golden import OUT, REF, _import_reference  # noqa: E402
from tools.make_layout_golden import _omegaconf_stand_in  # noqa: E402

REF_FILE = os.path.join(REF, "downstream_tasks", "test_flow_latent_inpainting.py")


def _stand_ins():
    for name, attrs in (("torchvision", {}), ("diffusers", {}), ("diffusers.models", {"AutoencoderKL": None}), ("torchdiffeq", {"odeint_adjoint": None})):
        try:
            __import__(name)
        except ImportError:
            mod = types.ModuleType(name)
            for k, v in attrs.items():
                setattr(mod, k, v)
            sys.modules[name] = mod
            if "." in name:
                setattr(sys.modules[name.split(".")[0]], name.split(".")[1], mod)


def _lines(first, last):
    """Lines first..last (1-based, inclusive) of the reference file, dedented to the first one's indentation."""
    src = open(REF_FILE).read().splitlines()[first - 1:last]
    pad = len(src[0]) - len(src[0].lstrip())
    return "\n".join(s[pad:] for s in src)


def parser_defaults():
    """What the reference driver's parser returns for an empty command line: its `parser = ...` statements (the block under __main__, up to parse_args)."""
    src = open(REF_FILE).read().splitlines()
    first = next(i for i, s in enumerate(src) if "argparse.ArgumentParser(" in s)
    last = next(i for i, s in enumerate(src) if "parser.parse_args()" in s)
    ns = {"argparse": argparse}
    exec("\n".join(s[4:] if s.startswith("    ") else s for s in src[first:last]), ns)  # noqa: S102
    return vars(ns["parser"].parse_args([]))


def main():
    _omegaconf_stand_in()
    _import_reference()
    _stand_ins()
    sys.path.insert(0, os.path.join(REF, "downstream_tasks"))
    import test_flow_latent_inpainting as ref

    img_u8, mask_u8 = ic.golden_pairs()
    with tempfile.TemporaryDirectory() as td:
        ic.write_pairs(os.path.join(td, "gt"), os.path.join(td, "masks"), img_u8, mask_u8)
        ds = ref.CustomizedInpaintingEvalDataset(os.path.join(td, "gt"), os.path.join(td, "masks"))
        items = [ds[k] for k in range(ic.GOLDEN_N)]
        from PIL import Image

        decoded = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(td, "gt", f"{k:06d}.jpg")).convert("RGB")) for k in range(ic.GOLDEN_N)]))
        stored = torch.from_numpy(np.stack([np.array(Image.open(os.path.join(td, "masks", f"{k:06d}.png"))) for k in range(ic.GOLDEN_N)]))
    assert torch.equal(stored, mask_u8)  # a PNG gives its bytes back; the JPEG gives `decoded`
    image, mask, masked = (torch.stack([it[k] for it in items]) for k in range(3))  # the DataLoader's default collation
    g = torch.Generator().manual_seed(65)
    R = ic.GOLDEN_S // 8
    c_in = torch.randn(ic.GOLDEN_N, 4, R, R, generator=g)
    fake = ic.make_fake(ic.GOLDEN_N, ic.GOLDEN_S, ic.GOLDEN_S, seed=9)  # (a seeded "decoded sample": the VAE is not part of what is pinned here)
    ns = {"F": F, "torch": torch, "device": "cpu", "c": c_in.clone(), "mask": mask.clone(), "image": image.clone(), "fake_image": fake.clone()}
    exec(_lines(148, 150), ns)  # noqa: S102  cc = F.interpolate(mask, size=c.shape[-2:]) ...; c = torch.cat((c, cc), dim=1)
    cc, c5 = ns["cc"], ns["c"]
    exec(_lines(98, 98), ns)  # noqa: S102  to_range_0_1
    exec(_lines(157, 160), ns)  # noqa: S102
    composite = ns["fake_image"]
    rec = {"decoded_u8": decoded, "mask_u8": stored, "img": image, "mask": mask, "masked_img": masked, "c_in": c_in, "cc": cc, "c5": c5,
           "fake_seed": 9,  # fake_image itself is inpaint_cases.make_fake(3, 64, 64, seed=9): regenerated, not stored
           "composite": composite, "save_image_u8": composite.mul(255).add_(0.5).clamp_(0, 255).permute(0, 2, 3, 1).to(torch.uint8).contiguous(),
           "parser_defaults": parser_defaults()}
    mine = ic.prepare32(decoded, stored)
    print("restatement == reference:", [bool(torch.equal(a, b)) for a, b in zip(mine, (image, mask, masked, cc))],
          bool(torch.equal(ic.composite_bytes32(fake, decoded, stored), rec["save_image_u8"])))
    path = os.path.join(OUT, "inpaint_prep.pt")
    torch.save(rec, path)
    print(f"{path} {os.path.getsize(path)} bytes; mask bytes {sorted(set(stored.flatten().tolist()))[:6]}... ({len(set(stored.flatten().tolist()))} values)")


if __name__ == "__main__":
    main()
