"""Generate tests/golden/layout_encoder.pt by running the UNMODIFIED reference BERTEmbedder (models/encoder.py:52-87 over models/x_transformer.py) in
float64 on the CPU, and the unmodified reference UNetModelAttn on one of its contexts.

    python -m tools.make_layout_encoder_golden          # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Writes data only: configurations, token tensors, the reference's outputs, its state-dict key / shape list and the checksum of the seeded state.  The weights
are NOT stored: both sides regenerate them from (name, shape, seed) with tests/layout_encoder_cases.py.  To stay well under 1 MB the outputs are stored at
64 columns per row (layout_encoder_cases.sample_cols: every column of the output is held in some row); tests/test_layout_encoder_ref.py holds the float64
restatement to these values at float64 rounding, and the GPU tests compare the device with the restatement on every element as well."""
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import layout_cases as lc  # noqa: E402
import layout_encoder_cases as ec  # noqa: E402
from oracle.make_golden import OUT, _import_reference  # noqa: E402
from tools.make_layout_golden import _omegaconf_stand_in  # noqa: E402


def golden_case(ref_cls, name):
    cfg, N, Ls = ec.CASES[name]
    m = ref_cls(use_tokenizer=False, **cfg).eval()
    _, checksum = ec.load_seeded(m)
    rec = {"cfg": cfg, "batch": N, "state_seed": ec.STATE_SEED, "state_checksum": checksum, "params": sum(p.numel() for p in m.parameters()),
           "keys": [(k, tuple(v.shape)) for k, v in m.state_dict().items()], "tokens": {}, "out_sampled": {}, "out_norm": {}}
    m = m.double()
    full = {}
    with torch.no_grad():
        for L in Ls:
            tok = ec.make_tokens(name, L)
            out = m(tok)
            mine = ec.encode64(ec.case_state(name), tok, cfg)
            rec["tokens"][L], rec["out_sampled"][L], rec["out_norm"][L] = tok.clone(), ec.sampled(out), float(out.norm())
            full[L] = out
            print(f"{name} L={L}: |out| {float(out.abs().mean()):.4f}, restatement vs reference max-abs {ec.max_abs(mine, out):.2e}", flush=True)
    return rec, full


def golden_solve(ctx):
    """x after torchdiffeq's 10 Euler steps from t = 1 to 0 through the reference UNetModelAttn (layout_cases.TINY_CFG, its seeded state and its x) on the
    reference encoder's context."""
    from lfm_amd.solvers import torchdiffeq_euler_grid
    from models.guided_diffusion.unet import UNetModelAttn

    m = UNetModelAttn(**lc.TINY_CFG).eval()
    lc.load_seeded(m)
    x, _, _, _ = lc.make_inputs(lc.TINY_CFG)
    ts, dts = torchdiffeq_euler_grid(0.1)
    ones, xs, c = torch.ones(x.shape[0]), x.clone(), ctx.float()
    with torch.no_grad():
        for k in range(dts.numel()):
            xs = xs + dts[k] * m(ts[k] * ones, xs, c)
    return xs


def main():
    _omegaconf_stand_in()
    _import_reference()
    from models.encoder import BERTEmbedder as ref_cls

    rec = {"cases": {}}
    for name in ec.CASES:
        rec["cases"][name], full = golden_case(ref_cls, name)
        if name == ec.SOLVE_CASE[0]:
            rec["x_euler10"] = golden_solve(full[ec.SOLVE_CASE[1]])
    path = os.path.join(OUT, "layout_encoder.pt")
    torch.save(rec, path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
