"""Generate tests/golden/{layout_tiny,layout_self}.pt by running the UNMODIFIED reference UNetModelAttn (models/guided_diffusion/unet.py) on the CPU.

    python -m tools.make_layout_golden          # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Writes data only: configurations, seeded inputs and contexts, the reference's outputs, its state-dict key / shape list and the checksum of the seeded state.
The weights are NOT stored: both sides regenerate them from (name, shape, seed) with tests/layout_cases.py, which leaves no tensor at the reference's zero
initialisation (with proj_out at zero the whole transformer drops out of the output).

The reference's constructor imports ``omegaconf.listconfig.ListConfig`` only to turn such a list into a plain one; where that package is missing, a stand-in
module with an empty class of that name is registered before the import (a plain int is never an instance of it)."""
import os
import sys
import types

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import layout_cases as lc  # noqa: E402
from oracle.make_golden import OUT, _import_reference  # noqa: E402


def _omegaconf_stand_in():
    try:
        import omegaconf.listconfig  # noqa: F401
    except ImportError:
        pkg, mod = types.ModuleType("omegaconf"), types.ModuleType("omegaconf.listconfig")
        mod.ListConfig = type("ListConfig", (list,), {})
        pkg.listconfig = mod
        sys.modules["omegaconf"], sys.modules["omegaconf.listconfig"] = pkg, mod


def _record(ref_cls, cfg):
    m = ref_cls(**cfg).eval()
    rec = {"cfg": cfg, "state_seed": lc.STATE_SEED, "state_checksum": lc.load_seeded(m), "params": sum(p.numel() for p in m.parameters()),
           "keys": [(k, tuple(v.shape)) for k, v in m.state_dict().items()]}
    rec["x"], rec["tN"], ctx, y = lc.make_inputs(cfg)
    return m, rec, ctx, y


def golden_tiny(ref_cls):
    from lfm_amd.solvers import torchdiffeq_euler_grid

    m, rec, ctx, _ = _record(ref_cls, lc.TINY_CFG)
    x, tN = rec["x"], rec["tN"]
    ones = torch.ones(x.shape[0])
    with torch.no_grad():
        for L, c in ctx.items():
            rec[f"ctx{L}"] = c.half()  # fp16-representable by construction: stored at half the size, exactly
            rec[f"v_t0d_L{L}"] = m(torch.tensor(0.6) * ones, x, c)  # the reference broadcasts a scalar t on "cuda" (unet.py:1188): broadcast here
            rec[f"v_tN_L{L}"] = m(tN, x, c)
        ts, dts = torchdiffeq_euler_grid(0.1)  # odeint(..., t=[1, 0], method="euler", options={"step_size": 0.1}): x += dt * v(t, x)
        xs, c = x.clone(), ctx[lc.CONTEXT_LENGTHS[0]]
        for k in range(dts.numel()):
            xs = xs + dts[k] * m(ts[k] * ones, xs, c)
        rec["x_euler10"] = xs
    print("tiny: params", rec["params"], "tensors", len(rec["keys"]), "|v|", float(rec["v_tN_L17"].abs().mean()), flush=True)
    return rec


def golden_self(ref_cls):
    m, rec, _, y = _record(ref_cls, lc.SELF_CFG)
    x, tN = rec["x"], rec["tN"]
    rec["y"] = y
    with torch.no_grad():
        rec["v_t0d"] = m(torch.tensor(0.6) * torch.ones(x.shape[0]), x, None, y=y)
        rec["v_tN"] = m(tN, x, y=y)
    print("self: params", rec["params"], "tensors", len(rec["keys"]), "|v|", float(rec["v_tN"].abs().mean()), flush=True)
    return rec


def main():
    _omegaconf_stand_in()
    _import_reference()
    from models.guided_diffusion.unet import UNetModelAttn as ref_cls

    torch.save(golden_tiny(ref_cls), os.path.join(OUT, "layout_tiny.pt"))
    torch.save(golden_self(ref_cls), os.path.join(OUT, "layout_self.pt"))


if __name__ == "__main__":
    main()
