"""Generate tests/golden/ssim.pt by running the UNMODIFIED reference's SSIM and inpainting evaluator on the CPU.

    python -m tools.make_ssim_golden          # where the reference checkout exists (LFM_REFERENCE, as oracle/make_golden.py)

``datasets_prep/inpaint_preprocess/losses/ssim.py`` is loaded from its file as it stands (it imports numpy and torch only) and ``SSIM(size_average=False)``
runs on every case of tests/ssim_cases.py in fp32 -- the tensors the evaluator's dataset would hand it, byte / 255 in fp32 -- and in fp64, which is the
yardstick of every accuracy test (for bytes the fp64 input is byte / 255 in fp64).

The evaluator: ``losses/base_loss.py`` and ``evaluator.py`` import packages that score other things (joblib, scipy, the segmentation and LPIPS networks) at
their top, so they cannot be imported whole; the statements this fixture needs -- ``get_groupings``, ``EvaluatorScore``, ``PairwiseScore``, ``SSIMScore``
and ``InpaintingEvaluator`` -- are taken out of the two files' syntax trees as they stand and executed here.  ``InpaintingEvaluator.evaluate`` then runs on
the 24 pairs of ssim_cases.eval_pairs() as a dataset of {"image", "mask", "inpainted"} (mask = 1 - byte / 255: 1 = hole), in fp32 and in fp64.

Writes data only: the reference's 1-D and 2-D windows, its per-image results, and the evaluator's result dictionaries, groups and interval names."""
import ast
import importlib.util
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ssim_cases as sc  # noqa: E402
from oracle.make_golden import OUT, REF  # noqa: E402

PRE = os.path.join(REF, "datasets_prep", "inpaint_preprocess")


def load_ssim():
    spec = importlib.util.spec_from_file_location("ref_ssim", os.path.join(PRE, "losses", "ssim.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def take(path, names, ns):
    """Execute the top-level functions and classes `names` of the file at `path`, as written there, in the namespace `ns`."""
    src = open(path).read()
    for node in ast.parse(src).body:
        if isinstance(node, (ast.FunctionDef, ast.ClassDef)) and node.name in names:
            exec(compile(ast.Module([node], []), path, "exec"), ns)  # noqa: S102
    missing = [n for n in names if n not in ns]
    assert not missing, missing
    return ns


def run_evaluator(ref_ssim, dtype):
    import tqdm
    import tqdm.auto  # noqa: F401
    from abc import ABC, abstractmethod
    from torch.utils.data import DataLoader

    ns = {"np": np, "torch": torch, "nn": torch.nn, "ABC": ABC, "abstractmethod": abstractmethod, "SSIM": ref_ssim.SSIM, "math": math, "tqdm": tqdm,
          "DataLoader": DataLoader, "move_to_device": lambda batch, device: batch, "Dict": dict}
    take(os.path.join(PRE, "losses", "base_loss.py"), ["get_groupings", "EvaluatorScore", "PairwiseScore", "SSIMScore"], ns)
    take(os.path.join(PRE, "evaluator.py"), ["InpaintingEvaluator"], ns)
    generated, image, mask = sc.eval_pairs()
    to = lambda u8: torch.from_numpy(np.transpose(u8, (0, 3, 1, 2)).copy()).to(dtype) / 255  # noqa: E731
    gen, img = to(generated), to(image)
    msk = 1 - torch.from_numpy(mask).to(dtype).unsqueeze(1) / 255
    dataset = [{"image": img[k], "mask": msk[k], "inpainted": gen[k]} for k in range(sc.EVAL_N)]
    score = ns["SSIMScore"]()
    ev = ns["InpaintingEvaluator"](dataset, {"ssim": score}, batch_size=8, device="cpu")
    groups, names = ev._get_bin_edges()
    results = ev.evaluate()
    return {"results": {k: {s: float(v) for s, v in d.items()} for k, d in results.items()}, "groups": [int(g) for g in groups], "interval_names": list(names),
            "individual_values": torch.from_numpy(np.asarray(score.individual_values, dtype=np.float64))}


def main():
    ref = load_ssim()
    rec = {"cases": {}, "windows": {}}
    for ws in (3, 5, 7, 9, 11):
        m = ref.SSIM(window_size=ws, size_average=False)
        rec["windows"][ws] = {"w1": m._gaussian(ws, 1.5).clone(), "w2": m.window[0, 0].clone()}
    worst = {}
    for case in sc.all_cases():
        d = sc.inputs(case)
        a32, b32 = torch.from_numpy(d["a32"]), torch.from_numpy(d["b32"])
        with torch.no_grad():
            r32 = ref.SSIM(window_size=d["ws"], size_average=False)(a32, b32)
            r64 = ref.SSIM(window_size=d["ws"], size_average=False)(torch.from_numpy(d["a64"]), torch.from_numpy(d["b64"]))
        assert r32.dtype == torch.float32 and r64.dtype == torch.float64
        rec["cases"][case[0]] = {"ref32": r32.clone(), "ref64": r64.clone()}
        fam = case[0].split("-")[0]
        worst[fam] = max(worst.get(fam, 0.0), float((r32.double() - r64).abs().max()))
    print("the reference's fp32 against its fp64, worst per family:", {k: f"{v:.2e}" for k, v in worst.items()})
    rec["eval32"] = run_evaluator(ref, torch.float32)
    rec["eval64"] = run_evaluator(ref, torch.float64)
    print("evaluator keys:", sorted(k[1] for k in rec["eval32"]["results"]), "groups", rec["eval32"]["groups"])
    assert rec["eval32"]["groups"] == rec["eval64"]["groups"]
    path = os.path.join(OUT, "ssim.pt")
    torch.save(rec, path)
    print(f"{path} {os.path.getsize(path)} bytes, {len(rec['cases'])} cases")


if __name__ == "__main__":
    main()
