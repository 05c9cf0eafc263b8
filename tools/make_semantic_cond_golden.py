"""Generate tests/golden/semantic_cond.pt by running the UNMODIFIED reference SpatialRescaler (models/encoder.py:90-112) in float64 on the CPU, on the
one-hot label maps its driver feeds it (downstream_tasks/test_flow_latent_semantic_syn.py:131-135).

    python -m tools.make_semantic_cond_golden          # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

Writes data only: per case of tests/semantic_cond_cases.py GOLDEN_CASES the reference's output and its state-dict key / shape list, and the defaults the
reference driver's own argument parser returns.  Neither labels nor weights are stored: both sides regenerate them from the case with
semantic_cond_cases.make_labels / gauss_weights.  Prints the distance of the float64 restatement from every stored output (the value quoted beside the margin in
tests/test_semantic_cond_ref.py)."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import semantic_cond_cases as sc  # noqa: E402
from oracle.make_golden import OUT, REF, _import_reference  # noqa: E402
from tools.make_layout_golden import _omegaconf_stand_in  # noqa: E402


def golden_case(ref_cls, c):
    m = ref_cls(n_stages=c.n_stages, in_channels=c.num_cls, out_channels=c.cout, multiplier=0.5, bias=c.bias).eval()
    keys = [(k, tuple(v.shape)) for k, v in m.state_dict().items()]
    w, b = sc.gauss_weights(c)
    sd = {"channel_mapper.weight": w.reshape(c.cout, c.num_cls, 1, 1)}
    if b is not None:
        sd["channel_mapper.bias"] = b
    m.load_state_dict(sd, strict=True)
    m = m.double()
    labels = sc.make_labels(c)
    with torch.no_grad():
        out = m(torch.nn.functional.one_hot(labels, c.num_cls).permute(0, 3, 1, 2).double())
    mine = sc.restate64(labels, w, b, c.n_stages)
    err = float((mine - out).abs().max())
    print(f"{sc.case_id(c)}: out {tuple(out.shape)}, |out| {float(out.abs().mean()):.4f}, restatement vs reference max-abs {err:.2e}", flush=True)
    return {"case": tuple(c), "keys": keys, "out": out}, err


def parser_defaults():
    """What the reference driver's parser returns for an empty command line: its `parser = ...` statements (the block under __main__, up to parse_args) run
    as they stand."""
    src = open(os.path.join(REF, "downstream_tasks", "test_flow_latent_semantic_syn.py")).read().splitlines()
    first = next(i for i, s in enumerate(src) if "argparse.ArgumentParser(" in s)
    last = next(i for i, s in enumerate(src) if "parser.parse_args()" in s)
    ns = {"argparse": argparse}
    exec("\n".join(s[4:] if s.startswith("    ") else s for s in src[first:last]), ns)  # noqa: S102
    return vars(ns["parser"].parse_args([]))


def main():
    _omegaconf_stand_in()
    _import_reference()
    from models.encoder import SpatialRescaler as ref_cls

    rec = {"cases": [], "parser_defaults": parser_defaults()}
    worst = 0.0
    for c in sc.GOLDEN_CASES:
        r, err = golden_case(ref_cls, c)
        rec["cases"].append(r)
        worst = max(worst, err)
    path = os.path.join(OUT, "semantic_cond.pt")
    torch.save(rec, path)
    print(f"{path} {os.path.getsize(path)} bytes; restatement vs reference, largest max-abs {worst:.2e}")


if __name__ == "__main__":
    main()
