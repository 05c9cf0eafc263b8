"""CPU checks behind the GPU tests of the label-map conditioning stage (lfm_label_rescale_f32, ``SpatialRescaler.encode_labels``, the mask-to-image driver;
cases, restatement and bound: tests/semantic_cond_cases.py): the float64 restatement is the unmodified reference (tests/golden/semantic_cond.pt) to float64
rounding; the reference's own fp32 chain and two fp32 emulations of a gather stay inside the per-element bound the GPU test uses, every named mistake leaves
it on the same inputs; the module has the reference's keys and shapes, the parser its defaults; every refusal that needs no device.  No GPU."""
import os

import numpy as np
import pytest
import torch

import semantic_cond_cases as sc


@pytest.fixture(scope="module")
def rec(golden_dir):
    return torch.load(os.path.join(golden_dir, "semantic_cond.pt"), map_location="cpu", weights_only=False)


def _inputs(c):
    return (sc.make_labels(c), *sc.gauss_weights(c))


def test_fixture_holds_outputs_only(rec, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "semantic_cond.pt")) < 1 << 20
    assert [sc.Case(*r["case"]) for r in rec["cases"]] == sc.GOLDEN_CASES
    for r in rec["cases"]:
        c = sc.Case(*r["case"])
        assert set(r) == {"case", "keys", "out"} and r["out"].dtype == torch.float64
        assert r["out"].shape == (c.N, c.cout, c.H >> c.n_stages, c.W >> c.n_stages)  # floor(S / 2^n): the ragged edge is dropped stage by stage
    g = sc.GOLDEN_CASES
    assert {(c.H, c.W) for c in g} >= set(sc.SHAPES) and {c.n_stages for c in g} == {1, 2, 3, 4} and {c.num_cls for c in g} == set(sc.CLASSES)
    assert {c.bias for c in g} == {False, True}


def test_restatement_is_the_reference_to_float64_rounding(rec):
    """Cell histogram / P times the weight against n x bilinear x0.5 + conv2d of the reference module in float64.  The means k / 4^n are exact and both sides
    then sum the same num_cls products; the margin allows one float64 rounding per class of outputs of order 1 (1024 x 2^-53 = 1.1e-13).  Measured when the
    fixture was written: 0.0 in every case."""
    worst = 0.0
    for r in rec["cases"]:
        c = sc.Case(*r["case"])
        labels, w, b = _inputs(c)
        worst = max(worst, float((sc.restate64(labels, w, b, c.n_stages) - r["out"]).abs().max()))
    print(f"restatement vs the reference's stored outputs: largest max-abs {worst:.2e}")
    assert worst <= 1.2e-13


@pytest.mark.parametrize("c", sc.gauss_cases(), ids=sc.case_id)
def test_fp32_paths_stay_inside_and_every_mistake_leaves_the_gpu_bound(c):
    labels, w, b = _inputs(c)
    ref, bnd = sc.restate64(labels, w, b, c.n_stages), sc.bound(labels, w, b, c.n_stages)
    assert bool((bnd > 0).all())
    r_chain = sc.error_ratio(sc.reference_chain(labels, w, b, c.n_stages), ref, bnd)  # the reference's own fp32 result
    r_kernel = sc.error_ratio(sc.emulate_kernel32(labels, w, b, c.n_stages), ref, bnd)
    r_seq = sc.error_ratio(sc.emulate_sequential32(labels, w, b, c.n_stages), ref, bnd)
    assert r_chain <= 1.0 and r_kernel <= 1.0 and r_seq <= 1.0, (r_chain, r_kernel, r_seq)
    shown = {}
    for m in sc.MISTAKES:
        wrong = sc.restate64(labels, w, b, c.n_stages, mistake=m)
        if not sc.mistake_shows(m, c):
            assert torch.equal(wrong, ref), m
            continue
        shown[m] = sc.error_ratio(wrong, ref, bnd)
        assert shown[m] > 1.0, (m, shown[m])
    print(f"{sc.case_id(c)}: error / bound: reference fp32 {r_chain:.3f}, kernel order {r_kernel:.3f}, sequential {r_seq:.3f}; mistakes "
          + ", ".join(f"{k} {v:.1e}" for k, v in shown.items()))
    assert len(shown) >= 2


def test_every_mistake_shows_in_some_gpu_case():
    assert all(any(sc.mistake_shows(m, c) for c in sc.gauss_cases()) for m in sc.MISTAKES)
    assert {c.n_stages for c in sc.gauss_cases()} == {1, 2, 3, 4} and {c.cout for c in sc.gauss_cases()} == set(range(1, 9))


def test_integer_cases_are_exact_in_every_order():
    """|weights| <= 8: the kernel-order emulation, the sequential sum and the reference's fp32 chain all give the int64 result bit for bit, poisoned ragged edge
    or not (the emulations never index it)."""
    for c in sc.exact_cases((43, 43))[::7] + sc.exact_cases((16, 16))[::11]:
        labels = sc.make_labels(c)
        w, b = sc.int_weights(c)
        ref = sc.exact_int(labels, w, b, c.n_stages)
        assert float(ref.abs().max()) <= 8 + 8 and torch.equal(ref.float().double(), ref)
        assert torch.equal(sc.emulate_kernel32(sc.poison_ragged_edge(c, labels), w, b, c.n_stages).double(), ref)
        assert torch.equal(sc.emulate_sequential32(labels, w, b, c.n_stages).double(), ref)
        assert torch.equal(sc.reference_chain(labels, w, b, c.n_stages).double(), ref)
        Hc, Wc = sc.whole(c)
        poisoned = sc.poison_ragged_edge(c, labels)
        assert torch.equal(poisoned[:, :Hc, :Wc], labels[:, :Hc, :Wc]) and int((poisoned == c.num_cls).sum()) == c.N * (c.H * c.W - Hc * Wc)


def test_module_has_the_reference_keys_and_shapes(rec):
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import SpatialRescaler

    for r in rec["cases"]:
        c = sc.Case(*r["case"])
        assert r["keys"] == sc.key_shapes(c.num_cls, c.cout, c.bias)
        m = SpatialRescaler(n_stages=c.n_stages, in_channels=c.num_cls, out_channels=c.cout, multiplier=0.5, bias=c.bias)
        assert [(k, tuple(v.shape)) for k, v in m.state_dict().items()] == r["keys"]


def test_module_on_the_cpu_is_the_reference_chain_through_either_entry(rec):
    """forward(one_hot) and encode_labels (which has no device here and takes the one-hot path) against the fixture."""
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import SpatialRescaler

    for r in rec["cases"][:6]:
        c = sc.Case(*r["case"])
        labels, w, b = _inputs(c)
        m = SpatialRescaler(n_stages=c.n_stages, in_channels=c.num_cls, out_channels=c.cout, multiplier=0.5, bias=c.bias).eval()
        m.load_state_dict({"channel_mapper.weight": w.reshape(c.cout, c.num_cls, 1, 1), **({"channel_mapper.bias": b} if c.bias else {})}, strict=True)
        with torch.no_grad():
            a = m(torch.nn.functional.one_hot(labels, c.num_cls).permute(0, 3, 1, 2).float())
            e = m.encode_labels(labels, c.num_cls)
        assert torch.equal(a, e) and sc.error_ratio(a, r["out"], sc.bound(labels, w, b, c.n_stages)) <= 1.0


def test_parser_defaults_match_the_reference(rec):
    from lfm_amd.downstream_tasks.flow_latent_semantic_syn import NUM_CLS, build_parser, num_classes_of

    ref = rec["parser_defaults"]
    assert ref == sc.REFERENCE_DEFAULTS  # what the reference's parser returned is what the cases module writes out
    mine = vars(build_parser().parse_args([]))
    assert {k: mine[k] for k in ref} == ref
    assert {k: v for k, v in mine.items() if k not in ref} == dict(random_weights=False, segmentation=None, num_cls=None, cond_path="fused", save_dir=None)
    assert NUM_CLS == {"coco": 182, "ade20k": 151, "celeba": 19}
    p = build_parser()
    assert num_classes_of(p.parse_args(["--dataset", "coco"])) == 182 and num_classes_of(p.parse_args(["--dataset", "coco", "--num_cls", "7"])) == 7
    with pytest.raises(SystemExit, match="give --num_cls"):
        num_classes_of(p.parse_args([]))  # the reference's default dataset, cifar10, has no label maps
    with pytest.raises(SystemExit):
        p.parse_args(["--cond_path", "gemm"])


def test_driver_refusals_that_need_no_device(tmp_path):
    from lfm_amd.downstream_tasks import flow_latent_semantic_syn as drv

    with pytest.raises(SystemExit, match="--segmentation FILE.npy"):
        drv.main(["--dataset", "celeba"])
    with pytest.raises(SystemExit, match="--segmentation FILE.npy"):
        drv.main([])
    np.save(tmp_path / "small.npy", np.zeros((3, 32, 32), dtype=np.int64))
    with pytest.raises(SystemExit, match=r"\[M, 64, 64\]"):
        drv.main(["--dataset", "celeba", "--random_weights", "--image_size", "64", "--segmentation", str(tmp_path / "small.npy")])
    np.save(tmp_path / "float.npy", np.zeros((3, 64, 64), dtype=np.float32))
    with pytest.raises(SystemExit, match="integer label maps"):
        drv.load_segmentation(str(tmp_path / "float.npy"), 64, 19)
    bad = np.zeros((2, 64, 64), dtype=np.int32)
    bad[1, 5, 7] = 19
    np.save(tmp_path / "bad.npy", bad)
    with pytest.raises(SystemExit, match=r"label 19 is outside \[0, 19\)"):
        drv.load_segmentation(str(tmp_path / "bad.npy"), 64, 19)
    bad[1, 5, 7] = -1
    np.save(tmp_path / "bad.npy", bad)
    with pytest.raises(SystemExit, match=r"label -1 is outside"):
        drv.load_segmentation(str(tmp_path / "bad.npy"), 64, 19)
    ok = drv.load_segmentation(str(tmp_path / "small.npy"), 32, 19)
    assert ok.dtype == torch.int64 and ok.shape == (3, 32, 32)
    syn = drv.synthetic_labels(3, 72, 19, seed=1)
    assert syn.shape == (3, 72, 72) and syn.dtype == torch.int64 and 0 <= int(syn.min()) and int(syn.max()) < 19
    assert bool((syn[:, :16, :16] == syn[:, :1, :1]).all())  # blocky
    with pytest.raises(ValueError, match="cond_path"):
        drv.synthesize_batch(None, None, None, syn, 19, None, cond_path="gemm")


def test_binding_refusals_that_need_no_device():
    from lfm_amd import hip

    lab, w = torch.zeros(2, 16, 16, dtype=torch.int64), torch.zeros(4, 19)
    with pytest.raises(hip.LfmHipError, match="no CPU fallback"):
        hip.label_rescale(lab, w, None, 3)
    assert hip.label_rescale_serves(182, 4, 3) and hip.label_rescale_serves(2048, 8, 4) and hip.label_rescale_serves(1, 1, 1)
    assert not hip.label_rescale_serves(2049, 8, 3) and not hip.label_rescale_serves(19, 9, 3) and not hip.label_rescale_serves(19, 4, 0)
    assert not hip.label_rescale_serves(19, 4, 5) and not hip.label_rescale_serves(0, 4, 3)


def test_entry_point_refuses_before_any_launch():
    """Every limit of include/lfm_hip.h, in its order (NULL pointer, shape, alignment), on buffers large enough for each call: no refused call touches a device,
    so this runs wherever the library loads."""
    from lfm_amd import hip

    dev = torch.device("cuda:0") if torch.cuda.is_available() else torch.device("cpu")
    lab, w = torch.zeros(2 * 16 * 16 + 8, dtype=torch.int64, device=dev), torch.zeros(16400 * 9, device=dev)
    bias, out = torch.zeros(16, device=dev), torch.full((2 * 9 * 8 * 8 + 64,), -1234.0, device=dev)
    for changed, offsets, expected, got in sc.refusals(hip.lib(), lab, w, bias, out, None):
        assert got == expected, (changed, offsets, expected, got)
    assert bool((out == -1234.0).all())
    assert {e for _, _, e in sc.REFUSALS} == {sc.ERR_ARG, sc.ERR_SHAPE, sc.ERR_ALIGN}
