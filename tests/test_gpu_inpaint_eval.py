"""The evaluator on the device (lfm_amd/inpaint_eval.py) and its two drivers: ``evaluate`` on the 24 synthetic 32 x 32 pairs of tests/ssim_cases.py against the
dictionary the unmodified reference's InpaintingEvaluator gave in fp64 (tests/golden/ssim.pt) -- bins and counts exactly, means and standard deviations
inside the per-image bounds combined; the evaluation CLI on a temporary directory of files in the drivers' naming; the inpainting driver with --ssim, which
prints the table and writes the same files as without it."""
import json
import os

import numpy as np
import pytest
import torch

import inpaint_cases as ic
import ssim_cases as sc
from lfm_amd import inpaint_eval as ie

pytestmark = pytest.mark.gpu

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "ssim.pt"), weights_only=False)


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def test_evaluate_gives_the_references_dictionary(dev):
    generated, image, mask = sc.eval_pairs()
    ref = GOLDEN["eval64"]
    results = ie.evaluate(generated, image, mask, batch_size=7)  # batches of 7, 7, 7 and 3: the batching does not show
    assert list(results) == list(ref["results"])  # total, then the bins that occur, in order
    assert len(results) - 1 >= 4 and ("ssim", "0-10%") in results and ("ssim", "90-100%") in results
    # mean and std are functions of the per-image values: |mean(a) - mean(b)| <= mean|a - b| and |std(a) - std(b)| <= std(a - b) <= rms(a - b), so the
    # per-image bounds combine to their mean and to their root mean square over the group
    bound = sc.bound(sc.unit64(generated), sc.unit64(image))
    groups = np.array(ref["groups"])
    for key, want in ref["results"].items():
        idx = np.arange(sc.EVAL_N) if key[1] == "total" else np.flatnonzero(groups == ref["interval_names"].index(key[1]))
        got = results[key]
        assert got["count"] == len(idx), key
        e_mean, e_std = abs(float(got["mean"]) - want["mean"]), abs(float(got["std"]) - want["std"])
        print(f"BOUND evaluate {key[1]}: mean off {e_mean:.2e} (bound {bound[idx].mean():.2e}), std off {e_std:.2e} (bound {np.sqrt((bound[idx] ** 2).mean()):.2e})")
        assert e_mean <= bound[idx].mean() and e_std <= np.sqrt((bound[idx] ** 2).mean()), key
    on_device = ie.evaluate(*(torch.from_numpy(t).to(dev) for t in (generated, image, mask)), batch_size=32)
    assert {k: (float(v["mean"]), float(v["std"]), v["count"]) for k, v in on_device.items()} == \
        {k: (float(v["mean"]), float(v["std"]), v["count"]) for k, v in results.items()}  # bit-reproducible whatever the batch size
    score = ie.SSIMScore()
    d255 = torch.full((), 255.0, device=dev)
    f = [torch.from_numpy(t).to(dev).permute(0, 3, 1, 2).float().div(d255).contiguous() for t in (generated, image)]
    assert torch.equal(score(f[0], f[1]), ie.hip.ssim_u8(torch.from_numpy(generated).to(dev), torch.from_numpy(image).to(dev))[0])  # floats on the device: lfm_ssim_f32
    # size_average: torch's fp32 mean over the 24 values, each at most 1: within 25 roundings of 2^-24 of their exact mean
    assert abs(float(ie.SSIM()(f[0], f[1])) - score.individual_values.mean()) <= 25 * 2.0 ** -24


def test_eval_cli_scores_the_files_as_written(dev, tmp_path, capsys):
    from lfm_amd.downstream_tasks import flow_latent_inpainting as drv
    from lfm_amd.downstream_tasks import inpainting_eval as cli
    from lfm_amd.io_formats import save_indexed_jpegs

    generated, image, mask = (torch.from_numpy(t) for t in sc.eval_pairs())
    gt, md, gen = str(tmp_path / "gt"), str(tmp_path / "masks"), str(tmp_path / "generated")
    ic.write_pairs(gt, md, image, mask)  # %06d.jpg, %06d.png
    save_indexed_jpegs(generated, gen, 0)  # the inpainting driver's files: {index}.jpg
    out = str(tmp_path / "scores.json")
    results = cli.main(["--generated", gen, "--images", gt, "--masks", md, "--image_size", str(sc.EVAL_S), "--batch_size", "10", "--out", out])
    printed = capsys.readouterr().out
    decoded, masks = drv.load_pairs(gt, md, sc.EVAL_S)
    assert torch.equal(masks, mask)
    want = ie.evaluate(cli.load_generated(gen, sc.EVAL_S), decoded, masks)
    assert ie.results_json(results) == ie.results_json(want)
    assert json.load(open(out)) == ie.results_json(want)
    assert "as written" in printed and "total" in printed and "90-100%" in printed
    assert [v["count"] for v in want.values()][0] == sc.EVAL_N
    # the same arrays as .npy give the same numbers
    np.save(tmp_path / "gen.npy", cli.load_generated(gen, sc.EVAL_S).numpy()), np.save(tmp_path / "gt.npy", decoded.numpy()), np.save(tmp_path / "m.npy", masks.numpy())
    again = cli.main(["--generated", str(tmp_path / "gen.npy"), "--images", str(tmp_path / "gt.npy"), "--masks", str(tmp_path / "m.npy"), "--image_size", str(sc.EVAL_S)])
    assert ie.results_json(again) == ie.results_json(want)
    np.save(tmp_path / "gt5.npy", decoded.numpy()[:5]), np.save(tmp_path / "m5.npy", masks.numpy()[:5])
    with pytest.raises(SystemExit, match="holds 24 images, but there are 5 pairs"):
        cli.main(["--generated", gen, "--images", str(tmp_path / "gt5.npy"), "--masks", str(tmp_path / "m5.npy"), "--image_size", str(sc.EVAL_S)])


DRIVER_ARGS = ["--image_size", "64", "--nf", "64", "--ch_mult", "1", "2", "--num_res_blocks", "1", "--attn_resolutions", "2", "--num_heads", "2",
               "--method", "euler", "--step_size", "0.5", "--batch_size", "2", "--random_weights"]  # tests/test_gpu_inpaint_batch.py's


def test_driver_with_ssim_prints_the_table_and_writes_the_same_files(dev, tmp_path, capsys):
    from lfm_amd.downstream_tasks import flow_latent_inpainting as drv

    img, mask = ic.golden_pairs()
    gt, md = str(tmp_path / "gt"), str(tmp_path / "masks")
    ic.write_pairs(gt, md, img, mask)
    try:
        drv.main([*DRIVER_ARGS, "--images", gt, "--masks", md, "--save_dir", str(tmp_path / "plain")])  # batches of 2 and 1
        plain = capsys.readouterr().out
        drv.main([*DRIVER_ARGS, "--images", gt, "--masks", md, "--save_dir", str(tmp_path / "scored"), "--ssim"])
        scored = capsys.readouterr().out
    finally:
        torch.set_grad_enabled(True)
    assert "SSIM" not in plain and "SSIM of the composites before JPEG coding" in scored and "total" in scored
    row = next(line.split() for line in scored.splitlines() if line.split()[:1] == ["total"])
    assert int(row[3]) == 3 and 0.0 < float(row[1]) <= 1.0
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(os.listdir(tmp_path / "scored")) == ["0.jpg", "1.jpg", "2.jpg"]
    for k in range(3):
        assert open(tmp_path / "plain" / f"{k}.jpg", "rb").read() == open(tmp_path / "scored" / f"{k}.jpg", "rb").read(), k
