"""CPU tests of the host logic: samplers / RNG against reference-generated golden vectors, the solver
module against the oracle restatement and analytic known answers, and the C-ABI export list."""
import math
import os
import re

import pytest
import torch

from oracle import ode_ref


def _load(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location="cpu", weights_only=False)


# ----------------------------------------------------------------------------- RNG (reference sampler/random_util.py)
def test_random_util_matches_reference(golden_dir):
    from lfm_amd.sampler.random_util import get_generator

    gold = _load(golden_dir, "randgen.pt")
    for n, seed, bs in ((64, 42, 8), (10, 7, 4)):
        gen = get_generator("determ", n, seed)
        assert torch.equal(gen.randn(bs, 4, 8, 8), gold[f"determ_n{n}_s{seed}_randn"])
        assert torch.equal(gen.randn(bs, 4, 8, 8), gold[f"determ_n{n}_s{seed}_randn2"])
        assert torch.equal(gen.randint(0, 1000, (bs,)), gold[f"determ_n{n}_s{seed}_randint"])
    gen = get_generator("determ-indiv", 6, 3)
    assert torch.equal(gen.randn(4, 2, 3, 3), gold["indiv_n6_s3_randn"])
    gen = get_generator("determ", 64, 42)
    gen.rank, gen.world_size = 1, 4
    assert torch.equal(gen.randn(8, 4, 8, 8), gold["determ_n64_s42_rank1of4_randn"])


def test_random_util_batch_size_independence():
    from lfm_amd.sampler.random_util import get_generator

    a = get_generator("determ", 32, 1).randn(8, 3)
    b = get_generator("determ", 32, 1).randn(4, 3)
    assert torch.equal(a[:4], b)  # same leading rows whatever the batch size (the point of the class)
    g = get_generator("determ", 8, 1)
    g.rank, g.world_size = 3, 4
    idx = g._indices(4)
    assert idx.tolist() == [3, 7, 7, 7]  # clamped at num_samples-1 (random_util.py:64)


# ----------------------------------------------------------------------------- Karras samplers (reference sampler/karras_sample.py)
class _Field:
    def __init__(self, A):
        self.A = A

    def __call__(self, t, x, **kw):
        flat = x.flatten(1)
        return (torch.tanh(flat @ self.A) * (1.0 + t[:, None]) - 0.5 * flat).reshape(x.shape)


@pytest.mark.parametrize("sampler,steps", [("euler", 11), ("euler", 51), ("heun", 11), ("heun", 50), ("heun", 40)])
def test_karras_sample_matches_reference(golden_dir, sampler, steps):
    from lfm_amd.sampler.karras_sample import karras_sample

    gold = _load(golden_dir, "karras.pt")
    out = karras_sample(_Field(gold["A"]), gold["x"].clone(), steps=steps, model_kwargs={}, device="cpu", clip_denoised=False,
                        sigma_min=1e-5, sigma_max=1.0, s_tmin=0.0, s_tmax=1.0, s_churn=0.0, sampler=sampler, rho=1.0, ts=range(0, steps, 15))
    torch.testing.assert_close(out, gold[f"{sampler}_{steps}"], rtol=0, atol=0)


@pytest.mark.parametrize("kind", ["determ", "determ-indiv"])
def test_heun_keeps_the_reference_rng_stream(golden_dir, kind):
    """Two consecutive Heun batches from ONE stateful generator: batch 2's x_T depends on the (zero-weighted) noise tensors the
    reference draws during batch 1 (karras_sample.py:143-145).  With the default reference_rng (on for determ*) the product
    reproduces both batches bit-for-bit; with the draws skipped only the first one."""
    from lfm_amd.sampler.karras_sample import karras_sample
    from lfm_amd.sampler.random_util import get_generator

    gold = _load(golden_dir, "karras_rng.pt")
    field = _Field(gold["A"])
    kw = dict(steps=11, model_kwargs={}, device="cpu", clip_denoised=False, sigma_min=1e-5, sigma_max=1.0, s_tmin=0.0, s_tmax=1.0,
              s_churn=0.0, sampler="heun")
    gen = get_generator(kind, 12, 5)
    for b in range(2):
        x = gen.randn(4, 1, 4, 4)
        assert torch.equal(x, gold[f"{kind}_x{b}"]), b
        assert torch.equal(karras_sample(field, x.clone(), generator=gen, **kw), gold[f"{kind}_out{b}"])
    gen = get_generator(kind, 12, 5)
    x0 = gen.randn(4, 1, 4, 4)
    assert torch.equal(karras_sample(field, x0.clone(), generator=gen, reference_rng=False, **kw), gold[f"{kind}_out0"])  # same batch result
    assert not torch.equal(gen.randn(4, 1, 4, 4), gold[f"{kind}_x1"])  # ... but the stream has left the reference's


def test_heun_quirk_counts_nfe():
    """steps=40 default is frozen: a 50-point grid does 49 predictor + 39 corrector evaluations = 88 NFE."""
    from lfm_amd.sampler.karras_sample import karras_sample

    calls = []

    def model(t, x, **kw):
        calls.append(float(t[0]))
        return -x

    x = torch.ones(2, 1, 2, 2)
    karras_sample(model, x, steps=50, model_kwargs={}, device="cpu", clip_denoised=False, sigma_min=1e-5, sigma_max=1.0, sampler="heun")
    assert len(calls) == 88
    calls.clear()
    karras_sample(model, x, steps=50, model_kwargs={}, device="cpu", clip_denoised=False, sigma_min=1e-5, sigma_max=1.0, sampler="heun",
                  heun_reference_quirk=False)
    assert len(calls) == 49 + 49  # quirk off: `i < steps - 1` with steps = the real grid length covers every interval
    calls.clear()
    karras_sample(model, x, steps=51, model_kwargs={}, device="cpu", clip_denoised=False, sigma_min=1e-5, sigma_max=1.0, sampler="euler")
    assert len(calls) == 50


# ----------------------------------------------------------------------------- odeint: product vs oracle vs analytic
def _lin(t, y):
    return -y * (1.0 + 0.5 * torch.sin(3 * t))


@pytest.mark.parametrize("method,h", [("euler", 0.02), ("euler", 0.03), ("midpoint", 0.1), ("rk4", 0.1)])
def test_fixed_grid_matches_oracle(method, h):
    from lfm_amd.solvers import odeint

    y0 = torch.randn(3, 4, generator=torch.Generator().manual_seed(0))
    t = torch.tensor([1.0, 0.0])
    a = odeint(_lin, y0, t, method=method, options={"step_size": h})
    b = ode_ref.odeint(_lin, y0, t, method=method, options={"step_size": h})
    assert a.shape == (2, 3, 4)
    torch.testing.assert_close(a, b, rtol=0, atol=0)


def test_euler_grid_and_nfe():
    from lfm_amd.solvers import odeint, torchdiffeq_euler_grid

    for h, n in ((0.02, 50), (0.01, 100), (0.1, 10), (0.03, 34)):
        ts, dts = torchdiffeq_euler_grid(h)
        assert dts.numel() == n and ts.numel() == n + 1
        assert float(ts[0]) == 1.0 and float(ts[-1]) == 0.0
        assert abs(float(dts.sum()) + 1.0) < 1e-6
        seen = []
        odeint(lambda t, y: (seen.append(float(t)), -y)[1], torch.ones(1), torch.tensor([1.0, 0.0]), method="euler", options={"step_size": h})
        assert len(seen) == n
        torch.testing.assert_close(torch.tensor(seen), ts[:-1], rtol=0, atol=0)
    ts, dts = torchdiffeq_euler_grid(0.03)
    assert abs(float(dts[-1]) + 0.01) < 1e-6  # short last step


def test_dopri5_matches_oracle_and_analytic():
    from lfm_amd.solvers import odeint

    y0 = torch.tensor([[1.0, 0.0], [0.5, -0.3]])
    w = 2.0

    def osc(t, y):  # harmonic oscillator, integrated backwards from t=1 to 0
        return torch.stack([y[:, 1] * w, -y[:, 0] * w], 1)

    t = torch.tensor([1.0, 0.0])
    st_a, st_b = {}, {}
    a = odeint(osc, y0, t, method="dopri5", rtol=1e-5, atol=1e-5, stats=st_a)
    b = ode_ref.odeint(osc, y0, t, method="dopri5", rtol=1e-5, atol=1e-5, stats=st_b)
    torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-6)
    assert st_a["steps"] == st_b["steps"] and st_a["accepted"] == st_b["accepted"]
    c, s = math.cos(-w), math.sin(-w)  # exact rotation by angle w*(0-1)
    exact = torch.stack([y0[:, 0] * c + y0[:, 1] * s, -y0[:, 0] * s + y0[:, 1] * c], 1)
    assert float((a[-1] - exact).abs().max()) < 2e-4


def test_fixed_grid_order_of_convergence():
    from lfm_amd.solvers import odeint

    y0 = torch.ones(1, dtype=torch.float64)
    f = lambda t, y: -y  # noqa
    exact = math.e  # y(0) = y(1) * e
    errs = {}
    for m in ("euler", "midpoint", "rk4"):
        errs[m] = [abs(float(odeint(f, y0, torch.tensor([1.0, 0.0], dtype=torch.float64), method=m, options={"step_size": h})[-1]) - exact)
                   for h in (0.1, 0.05)]
    assert 1.8 < errs["euler"][0] / errs["euler"][1] < 2.2
    assert 3.5 < errs["midpoint"][0] / errs["midpoint"][1] < 4.5
    assert 14 < errs["rk4"][0] / errs["rk4"][1] < 18


# ----------------------------------------------------------------------------- model-constructor boundary
def test_create_network_state_dict_matches_reference_names(golden_dir):
    from argparse import Namespace

    from lfm_amd.models import DiT, create_network

    rec = _load(golden_dir, "dit_tiny.pt")["cond"]
    c = rec["cfg"]
    m = DiT(img_resolution=c["img_resolution"], patch_size=c["patch"], in_channels=c["in_channels"], hidden_size=c["hidden"],
            depth=c["depth"], num_heads=c["heads"], label_dropout=c["label_dropout"], num_classes=c["num_classes"])
    ref_sd = rec["state_dict"]
    assert list(m.state_dict().keys()) == list(ref_sd.keys())
    assert all(m.state_dict()[k].shape == v.shape for k, v in ref_sd.items())
    m.load_state_dict(ref_sd, strict=True)
    net = create_network(Namespace(use_origin_adm=False, model_type="DiT-B/2", image_size=256, f=8, num_in_channels=4,
                                   label_dropout=0.0, num_classes=1))
    assert sum(p.numel() for p in net.parameters()) == 129_732_112  # == the reference DiT-B/2 constructor (checked against /root/reference; incl. the frozen pos_embed)
    # default init is adaLN-Zero (DiT.py:219-228)
    assert not bool(net.final_layer.linear.weight.any()) and not bool(net.blocks[0].adaLN_modulation[1].weight.any())
    torch.testing.assert_close(m.pos_embed, ref_sd["pos_embed"], rtol=0, atol=1e-6)


def test_cfg_without_classes_is_an_error():
    from argparse import Namespace

    from lfm_amd.test_flow_latent import make_model_kwargs

    with pytest.raises(ValueError):
        make_model_kwargs(Namespace(num_classes=1, cfg_scale=1.5, model_type="DiT-B/2"), torch.zeros(2, 4, 8, 8), None, "cpu")


# ----------------------------------------------------------------------------- C ABI
def test_c_abi_exports_every_declared_symbol():
    import ctypes

    from lfm_amd import _build

    lib_path = _build.build()
    lib = ctypes.CDLL(lib_path)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "lfm_hip.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)  # declarations only (comments name struct fields like lfm_dit_call.fold_ln)
    measure = re.findall(r"#ifdef LFM_MEASURE(.*?)#endif", hdr, flags=re.S)
    measure_names = set(re.findall(r"\b(lfm_[a-z0-9_]+)\s*\(", "".join(measure)))
    names = sorted(set(re.findall(r"\b(lfm_[a-z0-9_]+)\s*\(", hdr)) - measure_names)
    assert len(names) >= 12 and len(measure_names) == 5  # trace readers (3) + the per-kernel checksum pair
    for n in names:
        assert hasattr(lib, n), f"{n} declared in include/lfm_hip.h but not exported"
    if os.environ.get("LFM_MEASURE") != "1":  # the shipped library carries no measurement-only entry point
        for n in measure_names:
            assert not hasattr(lib, n), f"{n} is measurement-only but exported by the shipped build"
    lib.lfm_strerror.restype = ctypes.c_char_p
    assert lib.lfm_strerror(0) == b"ok" and lib.lfm_abi_version() >= 1


def test_no_packed_fp32_op_sel():
    """Guard of the co-scheduling fix (csrc/common.h: fma_v; profiles/r05_cosched_root_cause.txt): a packed-fp32 instruction whose half takes its source
    from the OTHER register of the pair (op_sel) read that operand as 0.0 in lanes 48-63 when a foreign wave shared the SIMD.  The shipped library must not
    contain the form in ANY kernel: every gfx950 code object of the built .so is disassembled and scanned."""
    from lfm_amd import _build

    if not os.path.exists(_build.OBJDUMP):
        # wherever the library can be BUILT the guard must run: a toolchain without its disassembler is a broken install, not a reason to skip
        assert not os.path.exists(_build.HIPCC), f"hipcc is installed but {_build.OBJDUMP} is not: the op_sel guard cannot run"
        pytest.skip("no ROCm toolchain here (nothing can be built either)")
    found = _build.opsel_scan(_build.build())
    assert not found, "packed-fp32 instructions with op_sel (write the expression with fma_v / scalars instead):\n" + "\n".join(
        f"  {n} x {ins} op_sel:[{sel}] in {k}" for (k, ins, sel), n in sorted(found.items(), key=lambda x: -x[1])[:10])
    assert "-fno-slp-vectorize" in _build.FLAGS


def test_unet_and_edm_state_dict_names_match_reference(golden_dir):
    """Key-for-key (and shape-for-shape) identity with state dicts produced by the unmodified reference classes."""
    from lfm_amd.models.EDM import DhariwalUNet
    from lfm_amd.models.unet import UNetModel

    for which, rec in _load(golden_dir, "unet_tiny.pt").items():
        m = UNetModel(**rec["cfg"])
        assert list(m.state_dict().keys()) == list(rec["state_dict"].keys()), which
        assert all(m.state_dict()[k].shape == v.shape for k, v in rec["state_dict"].items())
    rec = _load(golden_dir, "edm_tiny.pt")
    m = DhariwalUNet(**rec["cfg"])
    assert list(m.state_dict().keys()) == list(rec["state_dict"].keys())
    assert all(m.state_dict()[k].shape == v.shape for k, v in rec["state_dict"].items())
    assert any(k.endswith("resample_filter") for k in rec["state_dict"])  # the up/down convolutions' buffers are mirrored too


def test_dit_workspace_requirement_is_monotone_in_the_batch():
    """lfm_dit_workspace_bytes is host-only arithmetic: small batches add split-K slabs, and the size for max_batch must still cover every
    smaller batch (lfm_amd/models/DiT.py keeps ONE workspace sized for the largest batch it has seen)."""
    import ctypes as C

    from lfm_amd import hip

    L = hip.lib()
    for kw in (dict(depth=24, hidden=1024, heads=16, mlp_hidden=4096, patch=2, in_ch=4, res=32, label_rows=1),     # DiT-L/2, T = 256
               dict(depth=12, hidden=768, heads=12, mlp_hidden=3072, patch=2, in_ch=4, res=32, label_rows=1001),   # DiT-B/2 class-conditional
               dict(depth=12, hidden=384, heads=6, mlp_hidden=1536, patch=2, in_ch=4, res=16, label_rows=11),     # T = 64
               dict(depth=28, hidden=1152, heads=16, mlp_hidden=4608, patch=2, in_ch=4, res=32, label_rows=1)):   # DiT-XL/2: head_dim 72
        s = hip.DitShape(**kw)
        sizes = [L.lfm_dit_workspace_bytes(C.byref(s), b) for b in range(1, 70)]
        assert all(v > 0 for v in sizes)
        assert all(b >= a for a, b in zip(sizes, sizes[1:])), kw
    bad = hip.DitShape(depth=28, hidden=1280, heads=16, mlp_hidden=5120, patch=2, in_ch=4, res=32, label_rows=1)  # head_dim 80: no kernel
    assert L.lfm_dit_workspace_bytes(C.byref(bad), 1) == 0


def test_dit_workspace_layout_is_the_drivers_carve():
    """lfm_dit_workspace_layout (host only): the offsets of the buffers a forward at this batch uses, in the order of the header, 256-byte aligned, disjoint,
    inside lfm_dit_workspace_bytes, depending on the batch; buffers only the folded path has are 0 for shapes that never fold; bad arguments are refused."""
    import ctypes as C

    from lfm_amd import hip

    L = hip.lib()
    fold = hip.DitShape(depth=2, hidden=512, heads=8, mlp_hidden=2048, patch=2, in_ch=4, res=32, label_rows=5)
    plain = hip.DitShape(depth=2, hidden=384, heads=6, mlp_hidden=1536, patch=2, in_ch=4, res=16, label_rows=5)
    assert hip.DIT_WS_BUFFERS == ("X", "A", "A2", "QKVH", "mod", "ln_part", "cen0", "cen1", "uvq", "uvf")
    for s, B in ((fold, 1), (fold, 3), (fold, 96), (plain, 1), (plain, 7)):
        lay = hip.dit_workspace_layout(s, B)
        M, D, H = B * (s.res // s.patch) ** 2, s.hidden, s.mlp_hidden
        J = s.depth * 6 * D + 2 * D
        folds = D % 256 == 0
        size = {"X": M * D * 4, "A": M * D * 2, "A2": M * D * 2, "QKVH": max(3 * M * D, M * H) * 2, "mod": B * J * 4, "ln_part": M * ((D + 255) // 256) * 8,
                "cen0": M * 4, "cen1": M * 4, "uvq": s.depth * 2 * B * 3 * D * 4, "uvf": s.depth * 2 * B * H * 4}
        assert lay["X"] == 0 and lay["A"] == M * D * 4 + (-M * D * 4) % 256  # X first, A behind it (what test_trained_like_dynamic_range once computed by hand)
        present = [n for n in hip.DIT_WS_BUFFERS if folds or n not in ("A2", "uvq", "uvf")]
        assert all(lay[n] == 0 for n in hip.DIT_WS_BUFFERS if n not in present)
        spans = sorted((lay[n], lay[n] + size[n], n) for n in present)
        assert all(a % 256 == 0 for a, _, _ in spans)
        assert all(e0 <= a1 for (_, e0, _), (a1, _, _) in zip(spans, spans[1:])), spans  # disjoint
        assert spans[-1][1] <= L.lfm_dit_workspace_bytes(C.byref(s), B)
    assert hip.dit_workspace_layout(fold, 2)["A"] == 2 * hip.dit_workspace_layout(fold, 1)["A"]  # the batch of the call decides
    two = (C.c_size_t * 2)(7, 7)
    assert L.lfm_dit_workspace_layout(C.byref(fold), 1, two, 2) == len(hip.DIT_WS_BUFFERS) and list(two) == [0, hip.dit_workspace_layout(fold, 1)["A"]]
    assert L.lfm_dit_workspace_layout(C.byref(fold), 0, two, 2) == -1 and L.lfm_dit_workspace_layout(C.byref(fold), 1, None, 2) == -5
    bad = hip.DitShape(depth=28, hidden=1280, heads=16, mlp_hidden=5120, patch=2, in_ch=4, res=32, label_rows=1)  # head_dim 80: no kernel
    assert L.lfm_dit_workspace_layout(C.byref(bad), 1, two, 2) == -1


# ----------------------------------------------------------------------------- label bounds, buffer ownership, invalidation
def test_label_bounds_raise_like_nn_embedding():
    from lfm_amd import hip

    hip.check_labels(torch.tensor([0, 3, 9]), 10, "t")
    with pytest.raises(IndexError):
        hip.check_labels(torch.tensor([0, 10]), 10, "t")   # e.g. CFG's null class on a model built with label_dropout = 0
    with pytest.raises(IndexError):
        hip.check_labels(torch.tensor([-1, 2]), 10, "t")


def test_apply_without_a_move_keeps_the_packed_operands():
    """NFECount(model).to(device) / model.to(same device) must not drop packed weights, workspaces or captured graphs."""
    from lfm_amd.models import DiT_models

    m = DiT_models["DiT-S/2"](img_resolution=32, in_channels=4, num_classes=1, label_dropout=0.0).eval()
    m._packed, gen = "sentinel", m._gen
    m.to("cpu")
    m.float()
    assert m._packed == "sentinel" and m._gen == gen
    m.double()
    assert m._packed is None and m._gen == gen + 1


def _tiny_unet(which, golden_dir):
    """The three UNet backbones at their smallest: two levels of 64 / 128 channels on a 16x16 grid (a few million parameters)."""
    import json

    import song_cases as sc
    from lfm_amd.models.EDM import DhariwalUNet, SongUNet
    from lfm_amd.models.unet import UNetModel

    if which == "SongUNet":
        return SongUNet(**sc.TINY_CFG).eval()
    rec = json.load(open(os.path.join(golden_dir, "unet_state_keys.json")))[which]
    return (DhariwalUNet if which == "DhariwalUNet" else UNetModel)(**rec["cfg"]).eval()


_UNETS = ["UNetModel", "DhariwalUNet", "SongUNet"]


@pytest.mark.parametrize("which", _UNETS)
def test_unet_host_state_is_invalidated_by_a_real_move_or_a_reload_only(golden_dir, which):
    """The UNets' shared host layer (lfm_amd/models/_unet_host.py): every backbone has the whole host state from construction on; .to(same device) /
    .float() on fp32 weights keep it; a real cast drops the packed operands and both scratch buffers and bumps _gen once; load_state_dict drops the
    packed operands and bumps _gen once."""
    m = _tiny_unet(which, golden_dir)
    assert all(name in m.__dict__ for name in ("_packed", "_scratch", "_conv_ws", "_gen"))
    assert m._packed is None and m._scratch is None and m._conv_ws is None
    scratch, conv_ws = torch.zeros(8, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    m._packed, m._scratch, m._conv_ws, gen = "sentinel", scratch, conv_ws, m._gen
    m.to("cpu")
    m.float()
    assert m._packed == "sentinel" and m._scratch is scratch and m._conv_ws is conv_ws and m._gen == gen
    m.double()
    assert m._packed is None and m._scratch is None and m._conv_ws is None and m._gen == gen + 1
    m._packed = "sentinel"
    m.load_state_dict(m.state_dict())
    assert m._packed is None and m._gen == gen + 2
    assert len(list(m.buffers())) == sum(k.endswith("resample_filter") for k in m.state_dict())  # the host layer registers nothing


@pytest.mark.parametrize("which", _UNETS)
def test_concurrency_twin_of_a_unet_shares_weights_not_scratch(golden_dir, which):
    from lfm_amd.solvers import concurrency_twin

    m = _tiny_unet(which, golden_dir)
    scratch, conv_ws = torch.zeros(8, dtype=torch.uint8), torch.zeros(4, dtype=torch.uint8)
    m._scratch, m._conv_ws = scratch, conv_ws
    t = concurrency_twin(m)
    assert t is not m and type(t) is type(m)
    assert all(a is b for a, b in zip(m.parameters(), t.parameters()))
    assert t._scratch is None and t._conv_ws is None
    t._scratch, t._conv_ws = torch.zeros(2, dtype=torch.uint8), torch.zeros(2, dtype=torch.uint8)
    assert m._scratch is scratch and m._conv_ws is conv_ws
    t._gen += 5
    assert m._gen != t._gen


@pytest.mark.parametrize("which", ["UNetModel", "UNetModel_updown", "DhariwalUNet"])
def test_unet_state_dict_keys_are_the_recorded_ones(golden_dir, which):
    """tests/golden/unet_state_keys.json: the sorted state-dict keys of tiny models, recorded before the backbones were moved onto the shared host layer (a base
    class must add no parameter, buffer or submodule).  SongUNet's list is in song_tiny.pt (test_song_unet_host.py)."""
    import json

    rec = json.load(open(os.path.join(golden_dir, "unet_state_keys.json")))[which]
    assert sorted(_tiny_unet(which, golden_dir).state_dict().keys()) == rec["keys"]


# ----------------------------------------------------------------------------- training pair (train_flow_latent.py:143-155)
def test_flow_matching_pair_defines_the_sampled_ode():
    from lfm_amd.train_flow_latent import SIGMA_MIN, flow_matching_loss, flow_matching_pair

    g = torch.Generator().manual_seed(0)
    z0, z1 = torch.randn(3, 4, 8, 8, generator=g), torch.randn(3, 4, 8, 8, generator=g)
    t = torch.tensor([0.0, 0.3, 1.0])
    zt, u, _ = flow_matching_pair(z0, t, z1)
    tt = t.view(-1, 1, 1, 1)
    assert torch.equal(zt, (1 - tt) * z0 + (1e-5 + (1 - 1e-5) * tt) * z1)   # the reference's line, verbatim arithmetic
    assert torch.equal(u, (1 - 1e-5) * z1 - z0)
    torch.testing.assert_close(zt[0], z0[0] + SIGMA_MIN * z1[0])            # t = 0: data (+ sigma_min noise)
    torch.testing.assert_close(zt[2], z1[2])                                # t = 1: noise
    # d z_t / dt = u: the ODE the samplers integrate from t = 1 to 0 carries z_1 back to z_0 + sigma_min z_1 when v = u
    eps = 1e-3
    zt2, _, _ = flow_matching_pair(z0, t + eps, z1)
    torch.testing.assert_close((zt2 - zt) / eps, u, rtol=1e-2, atol=1e-3)
    loss = flow_matching_loss(lambda t, x, y: torch.zeros_like(x), z0, generator=torch.Generator().manual_seed(1))
    assert float(loss) > 0


def test_unbuilt_dit_shapes_are_refused_at_construction():
    from lfm_amd.models import DiT_models

    from lfm_amd.models import DiT

    with pytest.raises(NotImplementedError):
        DiT(img_resolution=32, hidden_size=1280, depth=2, num_heads=16, num_classes=1, label_dropout=0.0)   # head_dim 80: no attention kernel
    DiT_models["DiT-XL/2"](img_resolution=32, in_channels=4, num_classes=1, label_dropout=0.0)       # head_dim 72: built
    DiT_models["DiT-B/8"](img_resolution=32, in_channels=4, num_classes=1, label_dropout=0.0)        # 16 tokens: built
    DiT_models["DiT-S/2"](img_resolution=64, in_channels=4, num_classes=1, label_dropout=0.0)        # 1024 tokens: built (four key chunks)
    with pytest.raises(NotImplementedError):
        DiT_models["DiT-S/2"](img_resolution=128, in_channels=4, num_classes=1, label_dropout=0.0)   # 4096 tokens: no attention kernel
    DiT_models["DiT-S/4"](img_resolution=32, in_channels=4, num_classes=1, label_dropout=0.0)        # 64 tokens, K = 64: built
    DiT_models["DiT-S/8"](img_resolution=64, in_channels=4, num_classes=1, label_dropout=0.0)        # 64 tokens, K = 256: built


def test_dit_plan_says_which_block_loop_runs():
    """lfm_dit_plan (no launch): the folded LayerNorm path and the fused QKV + attention kernel are taken exactly where their preconditions hold -- residual width a
    multiple of 256, whole 256-row tiles, a chip-filling batch; 256 tokens per image and head_dim 64 for the fused kernel -- and follow the library options and
    the per-call fold switch."""
    from lfm_amd import hip

    def shape(depth, hidden, heads, patch=2, res=32):
        return hip.DitShape(depth, hidden, heads, patch, 4, res, 4 * hidden, 1)

    L2, B2, XL2, S2, L4 = shape(24, 1024, 16), shape(12, 768, 12), shape(28, 1152, 16), shape(12, 384, 6), shape(24, 1024, 16, patch=4)
    both = hip.PLAN_FOLDED_LN | hip.PLAN_FUSED_QKV_ATTENTION
    assert hip.dit_plan(L2, 64) == both and hip.dit_plan(L2, 48) == both
    assert hip.dit_plan(L2, 47) == 0  # 188 tiles: not chip-filling
    assert hip.dit_plan(B2, 64, t_len=64, labels=True) == both and hip.dit_plan(B2, 512) == both
    assert hip.dit_plan(XL2, 64) == 0 and hip.dit_plan(S2, 256) == 0  # 1152 / 384 are not multiples of 256
    assert hip.dit_plan(L4, 256) == hip.PLAN_FOLDED_LN  # 64 tokens per image, one shared conditioning row: folded, but an image is not one 256-row tile
    assert hip.dit_plan(L4, 256, t_len=256, labels=True) == 0  # per-image rows need whole tiles of ONE image
    assert hip.dit_plan(L2, 64, fold_ln=hip.CALL_OFF) == 0
    hip.set_option(hip.OPT_FUSED_QKV_ATTENTION, 0)
    try:
        assert hip.dit_plan(L2, 64) == hip.PLAN_FOLDED_LN
    finally:
        hip.set_option(hip.OPT_FUSED_QKV_ATTENTION, 1)
    assert hip.dit_plan(L2, 64, gemm_select=hip.call_gemm_select(6)) == hip.PLAN_FOLDED_LN  # the one-wave-per-SIMD kernels keep the two-kernel form
    assert hip.dit_plan(L2, 64, gemm_select=hip.call_gemm_select(1)) == 0  # a forced 128x128 kernel: separate LayerNorm launches


def test_library_options_are_host_state_only():
    """lfm_set_option touches no device: unknown keys are refused, the folded-LayerNorm switch toggles (default on)."""
    from lfm_amd import hip

    L = hip.lib()
    assert L.lfm_set_option(99, 1) < 0
    with pytest.raises(hip.LfmHipError):
        hip.set_option(99, 1)
    hip.set_option(hip.OPT_FOLD_LN, 0)
    hip.set_option(hip.OPT_FOLD_LN, 1)
    hip.set_option(hip.OPT_FUSED_QKV_ATTENTION, 0)  # QKV projection + attention as one kernel (default on)
    hip.set_option(hip.OPT_FUSED_QKV_ATTENTION, 1)


def test_conv_split_k_plan_for_the_small_maps():
    """lfm_conv3x3_workspace_bytes is host-only arithmetic = the split-K plan of the UNets' low-resolution 3x3 convolutions (csrc/ops.hip): up to 256
    tiles of 128x128 split (the 16x16 maps of the celeb512 UNet at batch 32 would otherwise run one four-wave workgroup per CU), to at most 512
    workgroups, slices at least 128 deep and a multiple of 64; chip-filling problems need no workspace."""
    from lfm_amd import hip

    L = hip.lib()
    ws = lambda n, h, cin, cout: L.lfm_conv3x3_workspace_bytes(n, h, h, cin, cout)
    assert ws(32, 64, 256, 256) == 0 and ws(32, 32, 512, 512) == 0          # 2048 / 1024 tiles: no split
    # round 5: deep problems with >= 2048 rows whose 256x256 tiles x slices keep at least half the CUs busy slice on the 256x256 kernel (gemm_kernel.h:
    # splitk256_slices: the largest divisor of the K-tile count with slices >= 24 K-tiles and at most 256 workgroups); the workspace covers the larger plan
    assert ws(32, 16, 512, 512) == 3 * 8192 * 512 * 4                        # 64 tiles of 256x256 x 3 slices of 24 K-tiles (128x128 plan: two slices)
    assert ws(32, 16, 1024, 512) == 4 * 8192 * 512 * 4                       # 64 tiles x 4 slices of 36 K-tiles
    assert ws(64, 8, 768, 768) == 4 * 4096 * 768 * 4                         # EDM ffhq_adm 8x8 maps at batch 64: 48 tiles x 4 slices of 27 K-tiles
    assert ws(32, 8, 512, 512) == 8 * 2048 * 512 * 4                         # 64 tiles -> eight slices of K / 8 = 576
    assert ws(32, 4, 1024, 1024) == 16 * 512 * 1024 * 4                      # 32 tiles -> sixteen slices of 576
    assert ws(2, 8, 64, 128) == 0                                            # K = 576: a half (288) is not a multiple of the 64-deep K-tile
    assert ws(0, 8, 64, 128) == 0


# (M, N, K) -> kernel under lfm_gemm_select 0 / 1 / 4 / 5 / 6 for an instantiation that fits 32-bit offsets but cannot take kernel 6 (a convolution source)
_GEMM_PLAN = [
    ((16384, 3072, 1024), (5, 1, 4, 5, 5)),   # DiT-L/2 qkv, batch 64
    ((16384, 1024, 1024), (5, 1, 4, 5, 5)),   # proj
    ((16384, 4096, 1024), (5, 1, 4, 5, 5)),   # fc1
    ((16384, 1024, 4096), (5, 1, 4, 5, 5)),   # fc2
    ((16384, 2304, 768), (5, 1, 4, 5, 5)),    # DiT-B/2
    ((16384, 768, 768), (5, 1, 4, 5, 5)),
    ((16384, 384, 384), (4, 1, 4, 5, 5)),     # `mid`: fewer than 192 tiles of 256x256, at least 192 of 256x128
    ((16384, 512, 512), (4, 1, 4, 5, 5)),
    ((4096, 1536, 512), (4, 1, 4, 5, 5)),
    ((32768, 256, 256), (4, 1, 4, 5, 5)),
    ((4096, 512, 512), (1, 1, 4, 5, 5)),      # below 192 tiles of either
    ((1048576, 128, 1152), (4, 1, 4, 5, 5)),  # `narrow`
    ((262144, 256, 2304), (5, 1, 4, 5, 5)),   # VAE
    ((65536, 512, 4608), (5, 1, 4, 5, 5)),
    ((1024, 512, 4608), (1, 1, 4, 5, 5)),
    ((256, 3072, 1024), (1, 1, 4, 5, 5)),
    ((1048576, 64, 64), (1, 1, 4, 5, 5)),
    ((16384, 1024, 96), (1, 1, 4, 1, 1)),     # K % 64 != 0: no 256x256 kernel
    ((65536, 128, 32), (4, 1, 4, 1, 1)),      # K % 64 != 0, K % 32 == 0, narrow
]


def test_gemm_plan_is_the_kernel_that_runs():
    """lfm_gemm_plan (no launch) = the one chooser every GEMM launch goes through (csrc/gemm_dispatch.h: gemm_choose): the kernel per shape under every
    selection, for an instantiation that cannot take kernel 6 (a forced 6 runs 5), for one that can (a forced 6 runs 6, and so does the automatic choice with
    LFM_OPT_GEMM_V6 wherever it picked 5), and for operands beyond 32-bit offsets (no 256x256 kernel: 1; the 256x128 kernel stays)."""
    from lfm_amd import hip

    sels = (0, 1, 4, 5, 6)
    try:
        for (M, N, K), want in _GEMM_PLAN:
            for sel, k in zip(sels, want):
                hip.gemm_select(sel)
                assert hip.gemm_plan(M, N, K, caps=hip.GEMM_CAP_FITS) == k, (M, N, K, sel)
                assert hip.gemm_plan(M, N, K, caps=hip.GEMM_CAP_FITS | hip.GEMM_CAP_V6) == (6 if sel == 6 and k == 5 else k), (M, N, K, sel, "v6-capable")
                for caps in (0, hip.GEMM_CAP_V6):
                    assert hip.gemm_plan(M, N, K, caps=caps) == (1 if k in (5, 6) else k), (M, N, K, sel, "does not fit")
        hip.gemm_select(0)
        hip.set_option(hip.OPT_GEMM_V6, 1)
        for (M, N, K), want in _GEMM_PLAN:
            assert hip.gemm_plan(M, N, K, caps=hip.GEMM_CAP_FITS | hip.GEMM_CAP_V6) == (6 if want[0] == 5 else want[0]), (M, N, K, "OPT_GEMM_V6")
            assert hip.gemm_plan(M, N, K, caps=hip.GEMM_CAP_FITS) == want[0], (M, N, K, "OPT_GEMM_V6, not v6-capable")
        assert [hip.gemm_plan(256, 256, 1024, batch=b) for b in (192, 191, 95)] == [6, 4, 1]  # a batch counts as tiles: 192 of 256x256; 382 / 190 of 256x128
    finally:
        hip.gemm_select(0)
        hip.set_option(hip.OPT_GEMM_V6, 0)


# (batch, heads, head_dim, tokens) -> lfm_attention_plan under (the defaults, flag ATT_WIDE, LFM_OPT_ATTENTION_STREAM off).  1 = the 16-token kernel, 2 = one workgroup
# per item, 3 = its wide form, 4 = four key chunks, 5 = the query split, 6 = the streamed kernel, -1 = LFM_ERR_SHAPE.  Written from the rules, not from the C++:
# only 256 tokens x head_dim 64 has more than one kernel -- wide if asked for, else the query split up to 64 items, else streamed while a tensor
# (items x 256 x 64 fp16 = items x 32 KiB) stays below 2 GiB = up to 65535 items, else per item.
_ATTENTION_PLAN = [
    ((4, 16, 64, 16), (1, 1, 1)), ((4, 16, 72, 16), (1, 1, 1)),
    ((4, 16, 64, 64), (2, 2, 2)), ((4, 16, 72, 64), (2, 2, 2)),
    ((4, 16, 64, 128), (2, 2, 2)), ((4, 16, 72, 128), (2, 2, 2)),
    ((4, 16, 64, 256), (5, 3, 5)),                                  # 64 items: the query split (wide: for 64 items too)
    ((4, 16, 72, 256), (2, 2, 2)),                                  # ATT_WIDE is a head_dim 64 kernel
    ((4, 16, 64, 1024), (4, 4, 4)), ((4, 16, 72, 1024), (4, 4, 4)),
    ((1, 1, 64, 1024), (4, 4, 4)), ((4096, 16, 64, 1024), (4, 4, 4)),  # four key chunks whatever the item count
    ((1, 1, 64, 256), (5, 3, 5)), ((1, 2, 64, 256), (5, 3, 5)),
    ((5, 13, 64, 256), (6, 3, 2)),                                  # 65 items
    ((65, 1, 64, 256), (6, 3, 2)),
    ((64, 16, 64, 256), (6, 3, 2)),                                 # the benchmarked shape
    ((4369, 15, 64, 256), (6, 3, 2)),                               # 65535 items: 2 GiB - 32 KiB per tensor
    ((4096, 16, 64, 256), (2, 3, 2)),                               # 65536 items: 2 GiB
    ((4096, 16, 72, 256), (2, 2, 2)),
    ((4, 16, 80, 256), (-1, -1, -1)), ((4, 16, 80, 16), (-1, -1, -1)), ((4, 16, 128, 64), (-1, -1, -1)),
    ((4, 16, 64, 4096), (-1, -1, -1)), ((4, 16, 72, 4096), (-1, -1, -1)), ((4, 16, 64, 32), (-1, -1, -1)), ((4, 16, 64, 512), (-1, -1, -1)),
]


def test_attention_plan_is_the_kernel_that_runs():
    """lfm_attention_plan (no launch) = the one chooser lfm_dit_attention_hd and the block loop go through (csrc/attention_kernel.h: attention_choose): the kernel per
    shape under the defaults, under flag ATT_WIDE and with the streamed kernel switched off; shapes no kernel serves are refused."""
    from lfm_amd import hip

    def plans():
        return [hip.attention_plan(*shape) for shape, _ in _ATTENTION_PLAN]

    want = lambda i: [w[i] for _, w in _ATTENTION_PLAN]
    shapes = [s for s, _ in _ATTENTION_PLAN]
    try:
        assert list(zip(shapes, plans())) == list(zip(shapes, want(0)))
        hip.gemm_select(hip.DBG_ATT_WIDE << 4)
        assert list(zip(shapes, plans())) == list(zip(shapes, want(1)))
        hip.gemm_select(0)
        hip.set_option(hip.OPT_ATTENTION_STREAM, 0)
        assert list(zip(shapes, plans())) == list(zip(shapes, want(2)))
        hip.gemm_select(hip.DBG_ATT_WIDE << 4)  # both: the flag decides first
        assert hip.attention_plan(64, 16, 64, 256) == 3
    finally:
        hip.gemm_select(0)
        hip.set_option(hip.OPT_ATTENTION_STREAM, 1)
    assert hip.attention_plan(0, 16, 64, 256) == -1 and hip.attention_plan(4, 0, 64, 256) == -1  # as lfm_dit_attention_hd refuses them


# (N, HW, C, groups) -> lfm_groupnorm_plan as (statistics, apply) under (the defaults, flag UNET_GN_ROWS); -1 = LFM_ERR_SHAPE.  Written from the rules, not from
# the C++, with cpg = C / groups.  Statistics: FUSED 1 = cpg % 8 == 0, cpg <= 2048, HW <= 1024 and the flag not set; else ROWS 2 = cpg % 4 == 0 and C / 8 <= 256; else
# GROUPS4 3 = cpg % 4 == 0; else GROUPS1 4.  Apply: FUSED 1 with the fused statistics; else OCTET 2 = C / 8 <= 256 and 256 % (C / 8) == 0; else CHUNK 3, refused
# from HW (C / 8) = 2^31.  GROUPS4 + OCTET cannot occur: GROUPS4 is what a cpg % 4 == 0 shape gets only when C / 8 > 256 kept it from ROWS, and OCTET needs C / 8 <= 256.
_F, _R, _G4, _G1 = (1, 1), 2, 3, 4
_O, _CH = 2, 3
_GROUPNORM_PLAN = [
    ((2, 1024, 256, 32), (_F, (_R, _O))),                  # cpg 8 at the HW boundary; the flag: the three-kernel path of a fused shape
    ((2, 1025, 256, 32), ((_R, _O), (_R, _O))),
    ((2, 1024, 128, 32), ((_R, _O), (_R, _O))),            # cpg 4
    ((2, 1025, 128, 32), ((_R, _O), (_R, _O))),
    ((2, 1024, 384, 32), ((_R, _CH), (_R, _CH))),          # cpg 12: 48 octets do not divide the block
    ((2, 300, 384, 32), ((_R, _CH), (_R, _CH))),
    ((2, 2000, 768, 32), ((_R, _CH), (_R, _CH))),          # cpg 24 above HW 1024: 96 octets
    ((2, 1024, 96, 32), ((_G1, _CH), (_G1, _CH))),         # cpg 3
    ((2, 1025, 96, 32), ((_G1, _CH), (_G1, _CH))),
    ((2, 1024, 64, 32), ((_G1, _O), (_G1, _O))),           # cpg 2: 8 octets
    ((2, 300, 64, 32), ((_G1, _O), (_G1, _O))),
    ((2, 64, 2048, 1), (_F, (_R, _O))),                    # groups = 1: cpg = 2048 is the widest fused group; C / 8 = 256 is the widest ROWS / OCTET
    ((2, 64, 4096, 1), ((_G4, _CH), (_G4, _CH))),          # cpg 4096 > 2048
    ((2, 1024, 2304, 32), (_F, (_G4, _CH))),               # cpg 72, C / 8 = 288 > 256: the flag on a shape the row kernels do not take
    ((2, 1025, 2304, 32), ((_G4, _CH), (_G4, _CH))),
    ((2, 64, 4096, 32), (_F, (_G4, _CH))),
    ((1, 178956970, 96, 32), ((_G1, _CH), (_G1, _CH))),    # HW x 12 = 2^31 - 8: the chunk kernel's last index
    ((1, 178956971, 96, 32), (-1, -1)),                    # HW x 12 = 2^31 + 4
    ((1, 300000000, 64, 32), ((_G1, _O), (_G1, _O))),      # the octet kernel has no such limit
    ((0, 64, 256, 32), (-1, -1)), ((2, 0, 256, 32), (-1, -1)), ((2, 64, 0, 32), (-1, -1)), ((2, 64, 256, 0), (-1, -1)),
    ((-1, 64, 256, 32), (-1, -1)), ((2, -64, 256, 32), (-1, -1)), ((2, 64, -256, 32), (-1, -1)), ((2, 64, 256, -32), (-1, -1)),
    ((2, 64, 264, 33), (-1, -1)),                          # groups > 32 (33 divides 264, 264 % 8 == 0)
    ((2, 64, 256, 3), (-1, -1)),                           # C % groups
    ((2, 64, 36, 4), (-1, -1)),                            # C % 8
]


def test_groupnorm_plan_is_the_kernels_that_run():
    """lfm_groupnorm_plan (no launch) = the one chooser lfm_groupnorm_f16 and lfm_groupnorm2_f16 launch through (csrc/groupnorm_dispatch.h: gn_choose): the statistics
    and the apply kernel per shape under the defaults and under flag UNET_GN_ROWS, and every refusal.  lfm_vae_groupnorm_plan = the slabs per image of the
    decoder's statistics pass (csrc/vae.hip: vae_gn_slabs) for the workspace tests/test_gpu_groupnorm.py gives it."""
    from lfm_amd import hip

    shapes = [s for s, _ in _GROUPNORM_PLAN]
    plans = lambda: [hip.groupnorm_plan(*s) for s in shapes]
    try:
        assert list(zip(shapes, plans())) == list(zip(shapes, [w[0] for _, w in _GROUPNORM_PLAN]))
        hip.gemm_select(hip.DBG_UNET_GN_ROWS << 4)
        assert list(zip(shapes, plans())) == list(zip(shapes, [w[1] for _, w in _GROUPNORM_PLAN]))
    finally:
        hip.gemm_select(0)
    assert hip.lib().lfm_groupnorm_plan(2, 1024, 256, 32) == 1 | 1 << 4 and hip.lib().lfm_groupnorm_plan(2, 300, 384, 32) == 2 | 3 << 4  # stats | apply << 4

    # the decoder: stats for n images, the zero page, then per image the larger of the full-resolution epilogue slabs and 64 slabs x 128 half-octets, 8 bytes a pair
    ws = lambda n, HW: 256 + (n * 256 + 255) // 256 * 256 + n * max(HW * 256 // 512, 64 * 128) * 8
    vae = lambda n, HW, C_: hip.vae_groupnorm_plan(n, HW, C_, ws(n, HW))
    assert vae(1, 65536, 128) == 512    # one image: room for 32768 / 32 = 1024 slabs, 1024 / n wanted, 512 the cap; 128 pixels each
    assert vae(16, 4096, 256) == 4      # n x 64 = 1024: the 64-slab policy, 1024 pixels per slab
    assert vae(15, 4096, 512) == 4      # n = 15 with room for 8192 / 128 = 64 slabs only: the same launch
    assert vae(15, 4608, 128) == 68     # n = 15 with room for 8192 / 32 = 256: 1024 // 15 = 68 slabs of ceil(4608 / 68) = 68 pixels
    assert vae(3, 1000, 256) == 16      # room for 128, but no slab below 64 pixels
    assert vae(64, 1024, 512) == 1 and vae(64, 64, 512) == 1 and vae(16, 16384, 128) == 16
    assert hip.vae_groupnorm_plan(15, 4096, 512, ws(15, 4096) + 15 * 4 * 128 * 8) == 64  # four more slabs of room per image: 68 allowed, 64 of 64 pixels taken
    short = 256 + 16 * 256 + 16 * 64 * 32 * 8  # tests/test_gpu_groupnorm.py: test_vae_groupnorm_refuses_a_short_workspace
    assert hip.vae_groupnorm_plan(16, 64, 128, short) == 1 and hip.vae_groupnorm_plan(16, 64, 128, short - 8) == -3
    assert vae(0, 64, 128) == -1 and vae(2, 0, 128) == -1 and vae(2, 64, 384) == -1 and vae(2, 64, 64) == -1


# pairs of flags of DIFFERENT consumers on the same bits (csrc/debug_flags.h says "shares" next to both): today's overlaps, acknowledged one by one.
# A new pair fails test_debug_flags_have_one_definition until it is added here on purpose.
_SHARED_FLAG_BITS = {
    ("DBG_QKV_TRACE", "DBG_TRACE_GEMM"),
    ("DBG_ATT_WIDE", "DBG_GEMM_GM4"),
    ("DBG_GEMM_SPLITK128", "DBG_LN_BPERMUTE"),
    ("DBG_LN_FOUR_ROWS", "DBG_QKV_NO_VT_WRITES"),
    ("DBG_LN_TWO_ROWS", "DBG_QKV_NO_QK_WRITES"),
    ("DBG_QKV_PER_ITEM", "DBG_VAE_SEPARATE_STATS"),
    ("DBG_GEMM_ABL", "DBG_TRACE_COL"),
    ("DBG_DIT_PATCH_ROUND1", "DBG_GEMM_ABL"), ("DBG_DIT_PATCH_ROUND1", "DBG_TRACE_COL"),
    ("DBG_GEMM_ABL", "DBG_QKV_PER_ITEM"), ("DBG_QKV_PER_ITEM", "DBG_TRACE_COL"),
    ("DBG_GEMM_ABL", "DBG_VAE_SEPARATE_STATS"), ("DBG_TRACE_COL", "DBG_VAE_SEPARATE_STATS"),
    ("DBG_CONV_IMPLICIT_GEMM", "DBG_GEMM_ABL"), ("DBG_CONV_IMPLICIT_GEMM", "DBG_TRACE_COL"),
    ("DBG_CONV_HALO_SMALL", "DBG_GEMM_ABL"), ("DBG_CONV_HALO_SMALL", "DBG_TRACE_COL"),
    ("DBG_ATT_MODE", "DBG_GEMM_OPT"),
    ("DBG_ATT_MODE", "DBG_QKV_NO_KEY_LOOP"), ("DBG_GEMM_OPT", "DBG_QKV_NO_KEY_LOOP"),
    ("DBG_ATT_MODE", "DBG_QKV_TWO_KTILES"), ("DBG_GEMM_OPT", "DBG_QKV_TWO_KTILES"),
}


def test_debug_flags_have_one_definition():
    """csrc/debug_flags.h defines every ablation flag of lfm_gemm_select once: lfm_amd.hip exports exactly the same names and values, no consumer uses a bit
    twice, every bit is a flag bit (27 of them above the 4-bit kernel id), and the flags of different consumers that share bits are the acknowledged ones."""
    from lfm_amd import hip

    src = open(os.path.join(os.path.dirname(hip.__file__), "csrc", "debug_flags.h")).read()
    header = {n: int(v) for n, v in re.findall(r"^constexpr int LFM_(DBG_\w+) = (\d+);", src, re.M)}
    assert len(header) == len(re.findall(r"LFM_DBG_\w+ =", src)) > 30  # every definition has the one-line form this test reads
    assert header == {n: v for n, v in vars(hip).items() if n.startswith("DBG_")}
    bits = {}  # name (a field without _SHIFT / _MASK) -> bit mask
    for n, v in header.items():
        if n.endswith("_SHIFT"):
            bits[n[:-6]] = header[n[:-6] + "_MASK"] << v
        elif not n.endswith("_MASK"):
            assert v & (v - 1) == 0, n  # a flag is one bit
            bits[n] = v
    assert all(0 < m < (1 << 27) for m in bits.values())
    prefix = lambda n: n.split("_")[1]
    shared = {(a, b) for a in bits for b in bits if a < b and bits[a] & bits[b]}
    assert not [p for p in shared if prefix(p[0]) == prefix(p[1])]
    assert shared == _SHARED_FLAG_BITS
    for a, b in shared:  # the header says so next to both
        for x, y in ((a, b), (b, a)):
            line = [l for l in src.splitlines() if ("LFM_" + x + " =") in l or ("LFM_" + x + "_SHIFT =") in l or ("LFM_" + x + "_MASK =") in l]
            assert any(y[4:] in l for l in line), (x, y)


def test_seeded_edm_state_is_order_independent_and_fp16_exact():
    """oracle/edm_state.py: the weights of the full-size EDM fixtures are regenerated from (tensor name, shape, seed) on both sides -- the reference module in
    oracle/make_golden.py, the product module in the GPU tests -- so the draw must not depend on the order parameters are registered in, and every value must
    be fp16-representable (the product packs GEMM operands in fp16: the fixture is about arithmetic, not weight rounding)."""
    from oracle.edm_state import seeded_edm_state

    names = [("enc.32x32_block0.conv0.weight", (8, 4, 3, 3)), ("enc.32x32_block0.conv1.weight", (8, 8, 3, 3)), ("enc.32x32_block0.norm0.weight", (8,)),
             ("enc.32x32_block0.conv0.bias", (8,)), ("map_label.weight", (16, 10)), ("enc.32x32_block0.conv0.resample_filter", (1, 1, 2, 2))]
    a = seeded_edm_state(names, 7)
    b = seeded_edm_state(list(reversed(names)), 7)
    assert set(a) == set(b) and "enc.32x32_block0.conv0.resample_filter" not in a
    for k in a:
        assert torch.equal(a[k], b[k]) and torch.equal(a[k], a[k].half().float())
    assert not torch.equal(a["enc.32x32_block0.conv0.weight"], seeded_edm_state(names, 8)["enc.32x32_block0.conv0.weight"])
    assert float(a["enc.32x32_block0.conv1.weight"].std()) < float(a["enc.32x32_block0.conv0.weight"].std())  # the reference's zero-init layers stay small
    assert abs(float(a["enc.32x32_block0.norm0.weight"].mean()) - 1.0) < 0.2



def test_concurrency_twin_shares_weights_not_scratch():
    """solvers.concurrency_twin: a second handle for a second HIP stream -- the same parameter tensors, its own workspace and its own solver cache."""
    from lfm_amd.models import DiT_models
    from lfm_amd.solvers import concurrency_twin

    m = DiT_models["DiT-S/2"](img_resolution=32, in_channels=4, num_classes=1, label_dropout=0.0).eval()
    m.__dict__["_fused_solvers"] = {"k": object()}
    m._ws = (4, torch.zeros(8))
    t = concurrency_twin(m)
    assert t is not m and type(t) is type(m)
    assert all(a is b for a, b in zip(m.parameters(), t.parameters()))  # shared weights
    assert t._ws is None and m._ws is not None  # own scratch
    assert "_fused_solvers" not in t.__dict__ and "_fused_solvers" in m.__dict__  # own captured solvers
    t._gen += 5
    assert m._gen != t._gen  # plain attributes are per handle
