"""The error bound of tests/ssim_cases.py is sound and not vacuous, and the host mirror of the evaluator (lfm_amd/inpaint_eval.py) equals the reference's
logic -- all on the CPU, against tests/golden/ssim.pt (tools/make_ssim_golden.py: the unmodified reference's SSIM in fp32 and fp64 on every case, and its
InpaintingEvaluator on the 24 evaluator pairs).

  * the fp64 restatement that supplies the bound's intermediates equals the stored fp64 reference;
  * an fp32 numpy emulation of the kernel's operation order stays inside the bound on every case;
  * the unmodified reference's own fp32 results stay inside the bound on every case (so the bound admits what fp32 honestly costs: 2.6e-4 on the flat case);
  * each named mistake, applied to the emulation, leaves the bound on at least one case;
  * SSIMScore.get_value, area_bins and the CPU path of SSIM / SSIMScore give the stored dictionaries of the reference's evaluator."""
import os

import numpy as np
import pytest
import torch

import ssim_cases as sc
from lfm_amd import hip, inpaint_eval as ie

GOLDEN = torch.load(os.path.join(os.path.dirname(__file__), "golden", "ssim.pt"), weights_only=False)
CASES = sc.all_cases()
_cache = {}


def prepared(case):
    """inputs, the stored references and the bound of one case, computed once per session."""
    if case[0] not in _cache:
        d = sc.inputs(case)
        g = GOLDEN["cases"][case[0]]
        d.update(ref64=g["ref64"].numpy(), ref32=g["ref32"].numpy().astype(np.float64), bound=sc.bound(d["a64"], d["b64"], d["ws"]))
        _cache[case[0]] = d
    return _cache[case[0]]


def test_the_golden_file_holds_every_case():
    assert sorted(GOLDEN["cases"]) == sorted(c[0] for c in CASES)
    for c in CASES:
        assert GOLDEN["cases"][c[0]]["ref64"].dtype == torch.float64 and GOLDEN["cases"][c[0]]["ref64"].shape == (c[2][0],)


@pytest.mark.parametrize("ws", [3, 5, 7, 9, 11])
def test_the_window_is_the_references(ws):
    w1 = GOLDEN["windows"][ws]["w1"]
    assert torch.equal(hip.ssim_gaussian(ws), w1) and np.array_equal(sc.gaussian32(ws), w1.numpy())
    assert torch.equal(ie.SSIM(ws).window(1, w1)[0, 0], GOLDEN["windows"][ws]["w2"])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_restatement_emulation_and_reference_fp32_inside_the_bound(case):
    d = prepared(case)
    mine, _ = sc.ref64(d["a64"], d["b64"], d["ws"])
    assert np.abs(mine - d["ref64"]).max() <= 1e-12  # the bound's intermediates are the reference's
    emu = sc.emulate32(d["a32"], d["b32"], d["ws"]).astype(np.float64)
    r_emu, r_ref = (np.abs(emu - d["ref64"]) / d["bound"]).max(), (np.abs(d["ref32"] - d["ref64"]) / d["bound"]).max()
    print(f"BOUND ssim {case[0]}: bound {d['bound'].max():.2e}, emulation / bound {r_emu:.3f}, reference fp32 / bound {r_ref:.3f}")
    assert r_emu <= 1.0
    assert r_ref <= 1.0
    if case[1] in ("self", "zeros"):
        assert np.all(emu == 1.0) and np.all(d["ref64"] == 1.0)


def test_the_bound_is_as_small_as_the_issue_needs_and_as_large_as_fp32_costs():
    flat = prepared(next(c for c in CASES if c[0] == "flat-1x64x64-w11"))
    rand = prepared(next(c for c in CASES if c[0] == "random-1x64x64-w11"))
    assert np.abs(flat["ref32"] - flat["ref64"]).max() > 5e-5 and flat["bound"].min() >= 1.0e-4  # the cancellation is real, and admitted
    assert 5e-7 <= rand["bound"].max() <= 5e-5  # random bytes: no room for more than rounding


@pytest.mark.parametrize("mistake", sc.MISTAKES)
def test_a_named_mistake_leaves_the_bound(mistake):
    worst, where = 0.0, None
    for case in CASES:
        d = prepared(case)
        if mistake == "over256" and d["kind"] != "u8":
            continue
        if mistake == "short_halo" and case[2][2] <= sc.TILE:
            continue  # one tile wide: no seam
        got = sc.emulate32(d["a32"], d["b32"], d["ws"], mistake=mistake, u8=(d["a"], d["b"])).astype(np.float64)
        r = float(np.nanmax(np.abs(got - d["ref64"]) / d["bound"]))
        if r > worst:
            worst, where = r, case[0]
        if worst > 1.0:
            break
    print(f"MISTAKE {mistake}: error / bound {worst:.1f} on {where}")
    assert worst > 1.0


def test_area_bins_on_and_off_the_edges():
    H = W = 10  # 255 * 100 per image: every decile edge is reachable exactly
    full = 255 * H * W
    sums = [full, full - 1, full * 9 // 10 + 1, full * 9 // 10, full * 7 // 10, full // 2, 1, 0]
    groups, names = ie.area_bins(sums, H, W)
    assert groups.tolist() == [0, 0, 0, 1, 3, 5, 9, 9]  # share 0, just above 0, just below 0.1, exactly 0.1, 0.3, 0.5, just below 1, exactly 1.0
    assert names == ["0-10%", "10-20%", "20-30%", "30-40%", "40-50%", "50-60%", "60-70%", "70-80%", "80-90%", "90-100%"]
    assert ie.interval_names(4) == ["0-25%", "25-50%", "50-75%", "75-100%"] and ie.interval_names(20)[:2] == ["0.0-5.0%", "5.0-10.0%"]
    with pytest.raises(ValueError):
        ie.area_bins([full + 1], H, W)


def test_get_value_and_area_bins_equal_the_references_evaluator():
    _, _, mask = sc.eval_pairs()
    groups, names = ie.area_bins(mask.astype(np.int64).sum(axis=(1, 2)), sc.EVAL_S, sc.EVAL_S)
    for key in ("eval32", "eval64"):
        ref = GOLDEN[key]
        assert groups.tolist() == ref["groups"] and names == ref["interval_names"]
        score = ie.SSIMScore()
        score._batches = [ref["individual_values"][:10], ref["individual_values"][10:]]
        total, per_group = score.get_value(groups)
        mine = {("ssim", "total"): total, **{("ssim", names[g]): v for g, v in per_group.items()}}
        assert list(mine) == list(ref["results"])
        for k, v in ref["results"].items():
            assert float(mine[k]["mean"]) == v["mean"] and float(mine[k]["std"]) == v["std"], k
    assert len(set(GOLDEN["eval32"]["groups"])) >= 4 and {0, 9} <= set(GOLDEN["eval32"]["groups"])
    assert score.get_value()[1] is None


def test_the_cpu_path_of_the_score_follows_the_reference():
    generated, image, mask = (torch.from_numpy(t) for t in sc.eval_pairs())
    ref = GOLDEN["eval32"]
    score = ie.SSIMScore()
    for s in range(0, sc.EVAL_N, 8):  # the golden tool's batches
        score(generated[s:s + 8], image[s:s + 8], mask[s:s + 8])
    # torch's CPU convolution may add in another order on another machine, so the values are held to the bound against the fp64 reference, not to the stored
    # fp32 bits; what get_value makes of given values is compared exactly in the test above
    values = score.individual_values
    bound = sc.bound(sc.unit64(generated.numpy()), sc.unit64(image.numpy()))
    assert values.dtype == np.float64 and np.all(np.abs(values - GOLDEN["eval64"]["individual_values"].numpy()) <= bound)
    assert np.all(values == values.astype(np.float32))  # fp32 values held as float64, as the reference's np.hstack leaves them
    groups, names = ie.area_bins(score.mask_sums, sc.EVAL_S, sc.EVAL_S)
    assert groups.tolist() == ref["groups"]
    results = ie.results_by_name(score, groups, names)
    for k, v in GOLDEN["eval64"]["results"].items():
        idx = np.flatnonzero(groups == names.index(k[1])) if k[1] != "total" else np.arange(sc.EVAL_N)
        assert abs(float(results[k]["mean"]) - v["mean"]) <= bound[idx].mean() and abs(float(results[k]["std"]) - v["std"]) <= np.sqrt((bound[idx] ** 2).mean()), k
    assert sum(v["count"] for k, v in results.items() if k[1] != "total") == results[("ssim", "total")]["count"] == sc.EVAL_N
    f = (generated[:4].permute(0, 3, 1, 2).float() / 255, image[:4].permute(0, 3, 1, 2).float() / 255)
    assert ie.SSIM(size_average=True)(*f).dim() == 0 and ie.SSIM(size_average=False)(*f).shape == (4,)
    score.reset()
    assert score.individual_values.size == 0
    text, js = ie.format_table(results), ie.results_json(results)
    assert "total" in text and "90-100%" in text and js["ssim"]["total"]["count"] == sc.EVAL_N
