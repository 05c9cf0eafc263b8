"""Generate tests/golden/adm_context_tiny.pt by running the UNMODIFIED reference models/EDM.py on the CPU.

    python -m tools.make_adm_context_golden     # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Writes data only, as tools/make_ncsnpp_golden.py does: the configuration of ``DhariwalUNet(use_context=True)`` (tests/adm_context_cases.py), the seed and
checksum of the state both sides regenerate, the reference's key / shape list, a checksum of the seeded inputs (regenerated too) and the reference's
outputs -- v at a 0-d and at a per-sample time with labels that include the extra row ``label_dim``, v of a batch of one under another label,
``forward_with_cfg`` at scale 1.5 with the second half's labels at the null row and at class 0 (one half each: the two halves of its output are equal), one
``TransformerBlock`` alone on a seeded input, and ten Euler steps on the torchdiffeq grid, unguided and guided."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import adm_context_cases as ac  # noqa: E402
from oracle.make_golden import OUT, _import_reference  # noqa: E402


def golden_adm_context(ref_edm):
    from lfm_amd.solvers import torchdiffeq_euler_grid

    cfg = ac.TINY_CFG
    m = ref_edm.DhariwalUNet(**cfg).eval()
    rec = {"cfg": cfg, "state_seed": ac.STATE_SEED, "state_checksum": ac.load_seeded(m), "params": sum(p.numel() for p in m.parameters()),
           "keys": [(k, tuple(v.shape)) for k, v in m.state_dict().items()]}
    i = ac.inputs()
    rec["x_checksum"] = float(i.x.double().abs().sum())
    with torch.no_grad():
        rec["v_t0d"] = m(torch.tensor(ac.T0D), i.x, i.y)
        rec["v_tN"] = m(i.tN[:2], i.x[:2], i.y[:2])
        rec["v_y2"] = m(torch.tensor(ac.T0D), i.x[3:], i.y2)
        n2 = 2
        for name, y in (("cfg_null", i.y_cfg_null), ("cfg_zero", i.y_cfg_zero)):
            out = m.forward_with_cfg(torch.tensor(ac.T0D), i.x, y, cfg_scale=ac.CFG_SCALE)
            assert torch.equal(out[:n2], out[n2:])
            rec[name] = out[:n2].clone()
        xb, yb = ac.block_input()
        tb = m.dec[ac.BLOCK.split(".", 1)[1]].transformer
        rec["block_out"] = tb(xb, m.map_label(yb, False))
        ts, dts = torchdiffeq_euler_grid(0.1)  # odeint(..., t=[1, 0], method="euler", options={"step_size": 0.1}): x += dt * v(t, x)
        xs = i.x[:2].clone()
        for k in range(dts.numel()):
            xs = xs + dts[k] * m(ts[k], xs, i.y[:2])
        rec["x_euler10"] = xs
        xs = torch.cat([i.x[:2], i.x[:2]], 0)
        for k in range(dts.numel()):
            xs = xs + dts[k] * m.forward_with_cfg(ts[k], xs, i.y_cfg_null, cfg_scale=ac.CFG_SCALE)
        assert torch.equal(xs[:n2], xs[n2:])
        rec["x_euler10_cfg"] = xs[:n2].clone()
    print("params", rec["params"], "tensors", len(rec["keys"]), "|v|", float(rec["v_t0d"].abs().mean()), "|block|", float(rec["block_out"].abs().mean()),
          "cfg null vs zero", ac.rel_l2(rec["cfg_null"], rec["cfg_zero"]), flush=True)
    return rec


def main():
    _import_reference()
    import models.EDM as ref_edm

    torch.save(golden_adm_context(ref_edm), os.path.join(OUT, "adm_context_tiny.pt"))


if __name__ == "__main__":
    main()
