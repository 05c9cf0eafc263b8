"""GPU tests of the ddpm++ backbone (``SongUNet``) and of what it needed in kernels -- the residual epilogue with a scale on every path a residual
convolution or linear can take, the DDPM++ mapping network -- against float64 and against the unmodified reference (tests/golden/song_*.pt,
tools/make_song_golden.py); and of guided sampling of the EDM ``adm`` on the fixed grids through the captured solver (tests/golden/edm_cfg_grid.pt)."""
import os
import subprocess
import sys
from argparse import Namespace

import pytest
import torch

import song_cases as sc

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD, SENTINEL = 8, -1234.0  # rows after the last output row: a store past the end shows
RSQRT2 = 0.5 ** 0.5


def rel_l2(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return float((a - b).norm() / b.norm())


def _rec(golden_dir, name):
    return torch.load(os.path.join(golden_dir, name), map_location="cpu", weights_only=False)


# ------------------------------------------------------------------------------------------------ the scaled residual epilogue
def _operands(M, K, Nout, seed):
    g = torch.Generator().manual_seed(seed)
    dev = torch.device("cuda:0")
    A = torch.randn(M, K, generator=g).half().to(dev)
    W = (torch.randn(Nout, K, generator=g) / K ** 0.5).half().to(dev)
    bias = (0.5 * torch.randn(Nout, generator=g)).to(dev)
    resid = torch.randn(M, Nout, generator=g).half().to(dev)
    return A, W, bias, resid


def _guarded(M, Nout):
    return torch.full((M + GUARD, Nout), SENTINEL, dtype=torch.float16, device="cuda:0")


def _check_scaled(run, ref64, M, what):
    """run(scale or None) -> guarded output; None = the unscaled entry point.  scale 1 is bit-identical to it, sqrt(1/2) matches float64."""
    old, one, half = run(None), run(1.0), run(RSQRT2)
    torch.cuda.synchronize()
    for o in (old, one, half):
        assert bool((o[M:] == SENTINEL).all()), what
    assert torch.equal(old, one), what
    e1, e2 = rel_l2(old[:M], ref64), rel_l2(half[:M], ref64 * RSQRT2)
    print(f"{what}: rel-L2 vs float64 {e1:.3e} (unscaled), {e2:.3e} (scale sqrt(1/2))")
    assert e1 < 2e-3 and e2 < 2e-3, what
    assert not torch.equal(old, half)


def _conv_ref64(x, W, bias, resid, N, H, Wd, Cin):
    """float64 3x3 convolution (pad 1) of NHWC x on the same fp16 operands: im2col with k = tap * Cin + ci, as the weights are laid out."""
    xp = torch.nn.functional.pad(x.double().reshape(N, H, Wd, Cin), (0, 0, 1, 1, 1, 1))
    cols = torch.cat([xp[:, ky:ky + H, kx:kx + Wd, :] for ky in range(3) for kx in range(3)], -1).reshape(N * H * Wd, 9 * Cin)
    return cols @ W.double().t() + bias.double() + resid.double()


# the smallest shape the dispatch sends down each path (tests/test_song_unet_host.py::test_conv3x3_plan_truth_table walks the thresholds):
#   halo kernel: 16-aligned maps, Cout % 128 == 0 and 256 (tile, channel block) pairs;  split-K: K = 9 Cin a multiple of 128 on at most 256 tiles, with the
#   workspace;  implicit GEMM: everything else -- odd map sizes, two row tiles and two (ragged) column tiles
@pytest.mark.parametrize("path,N,H,Wd,Cin,Cout", [("halo", 4, 64, 64, 64, 512), ("splitk", 1, 9, 7, 128, 132), ("gemm", 1, 13, 11, 64, 132)])
def test_scaled_epilogue_conv3x3(path, N, H, Wd, Cin, Cout):
    from lfm_amd import hip

    L, M = hip.lib(), N * H * Wd
    x, W, bias, resid = _operands(M, 9 * Cin, Cout, 5)
    x = x[:, :Cin].contiguous()
    need = L.lfm_conv3x3_workspace_bytes(N, H, Wd, Cin, Cout)
    ws = torch.empty(max(need, 16), dtype=torch.uint8, device=x.device)
    assert hip.conv3x3_plan(N, H, Wd, Cin, Cout, 0, need) == {"halo": hip.CONV_PLAN_HALO, "splitk": hip.CONV_PLAN_SPLITK, "gemm": hip.CONV_PLAN_GEMM}[path]
    assert (need > 0) == (path == "splitk")

    def run(scale):
        out = _guarded(M, Cout)
        if scale is None:
            hip.check(L.lfm_conv3x3_f16_ws(hip.ptr(x), hip.ptr(W), hip.ptr(bias), hip.ptr(resid), hip.ptr(out), N, H, Wd, Cin, Cout, 0, hip.ptr(ws), need,
                                           hip.stream_ptr()), "lfm_conv3x3_f16_ws")
        else:
            hip.check(L.lfm_conv3x3_scaled_f16_ws(hip.ptr(x), hip.ptr(W), hip.ptr(bias), hip.ptr(resid), scale, hip.ptr(out), N, H, Wd, Cin, Cout, 0,
                                                  hip.ptr(ws), need, hip.stream_ptr()), "lfm_conv3x3_scaled_f16_ws")
        return out

    _check_scaled(run, _conv_ref64(x, W, bias, resid, N, H, Wd, Cin), M, f"conv3x3 {path}")


def test_scaled_epilogue_linear_and_linear2():
    from lfm_amd import hip

    L, M, Nout = hip.lib(), 143, 132  # two row tiles, two column tiles, both ragged
    K = 192
    A, W, bias, resid = _operands(M, K, Nout, 6)
    assert hip.gemm_plan(M, Nout, K) == 1

    def run(scale):
        out = _guarded(M, Nout)
        if scale is None:
            hip.check(L.lfm_linear_f16(hip.ptr(A), K, hip.ptr(W), K, hip.ptr(out), Nout, M, Nout, K, hip.ptr(bias), hip.ptr(resid), hip.stream_ptr()),
                      "lfm_linear_f16")
        else:
            hip.check(L.lfm_linear_scaled_f16(hip.ptr(A), K, hip.ptr(W), K, hip.ptr(out), Nout, M, Nout, K, hip.ptr(bias), hip.ptr(resid), scale,
                                              hip.stream_ptr()), "lfm_linear_scaled_f16")
        return out

    ref = A.double() @ W.double().t() + bias.double() + resid.double()
    _check_scaled(run, ref, M, "linear")
    K1, K2 = 128, 64  # the concat [A1 | A2] read in place: K1 % 64 == 0 and (the GEMM's own contract) (K1 + K2) % 64 == 0; the seam after K-tile 2 of 3
    A1, A2 = A[:, :K1].contiguous(), A[:, K1:K1 + K2].contiguous()
    W2 = W[:, :K1 + K2].contiguous()
    assert hip.gemm_plan(M, Nout, K1 + K2, caps=hip.GEMM_CAP_FITS) == 1

    def run2(scale):
        out = _guarded(M, Nout)
        if scale is None:
            hip.check(L.lfm_linear2_f16(hip.ptr(A1), K1, hip.ptr(A2), K2, hip.ptr(W2), K1 + K2, hip.ptr(out), Nout, M, Nout, hip.ptr(bias), hip.ptr(resid),
                                        hip.stream_ptr()), "lfm_linear2_f16")
        else:
            hip.check(L.lfm_linear2_scaled_f16(hip.ptr(A1), K1, hip.ptr(A2), K2, hip.ptr(W2), K1 + K2, hip.ptr(out), Nout, M, Nout, hip.ptr(bias),
                                               hip.ptr(resid), scale, hip.stream_ptr()), "lfm_linear2_scaled_f16")
        return out

    ref2 = torch.cat([A1, A2], 1).double() @ W2.double().t() + bias.double() + resid.double()
    _check_scaled(run2, ref2, M, "linear2")


# ------------------------------------------------------------------------------------------------ the mapping network
@pytest.mark.parametrize("F", [64, 128])
def test_song_mapping_kernel_vs_float64_with_time_embed_as_control(F):
    """lfm_song_embed against its float64 formula (pinned to the reference in tests/test_song_unet_host.py), with lfm_time_embed against ITS float64
    formula on the same weights and times as the control: the two kernels differ in the frequency table, the place of the label term and one SiLU, so
    the new kernel's worst absolute error may be at most twice the control's."""
    from lfm_amd import hip

    L, dev, N, E, rows = hip.lib(), torch.device("cuda:0"), 5, 4 * F, 7
    g = torch.Generator().manual_seed(F)
    w0, b0 = torch.randn(E, F, generator=g) / F ** 0.5, 0.1 * torch.randn(E, generator=g)
    w1, b1 = torch.randn(E, E, generator=g) / E ** 0.5, 0.1 * torch.randn(E, generator=g)
    lab_w, lab_b = 0.3 * torch.randn(F, rows, generator=g), 0.1 * torch.randn(F, generator=g)  # map_label.weight [F, L], .bias [F]
    adm_table = 0.5 * torch.randn(rows, E, generator=g)  # the control's label embedding (added to its OUTPUT)
    y = torch.tensor([3, 0, 6, 1, 5])
    d = lambda t: t.to(dev).contiguous()  # noqa: E731
    dw = [d(v) for v in (w0, b0, w1, b1)]
    dlab_t, dlab_b, dtable, dy = d(lab_w.t()), d(lab_b), d(adm_table), d(y)

    def song(t, labels, yy=dy):
        emb, emb16, h1 = torch.empty(N, E, device=dev), torch.empty(N, E, device=dev, dtype=torch.float16), torch.empty(N, E, device=dev)
        hip.check(L.lfm_song_embed(hip.ptr(t), t.numel(), *[hip.ptr(v) for v in dw], hip.ptr(dlab_t if labels else None),
                                   hip.ptr(dlab_b if labels else None), rows ** 0.5, hip.ptr(yy if labels else None), rows, hip.ptr(h1), hip.ptr(emb),
                                   hip.ptr(emb16), N, F, E, hip.stream_ptr()), "lfm_song_embed")
        return emb, emb16

    def adm(t, labels):
        emb, emb16, h1 = torch.empty(N, E, device=dev), torch.empty(N, E, device=dev, dtype=torch.float16), torch.empty(N, E, device=dev)
        hip.check(L.lfm_time_embed(hip.ptr(t), t.numel(), *[hip.ptr(v) for v in dw], hip.ptr(dtable if labels else None), hip.ptr(dy if labels else None),
                                   rows, hip.ptr(h1), hip.ptr(emb), hip.ptr(emb16), N, F, E, hip.stream_ptr()), "lfm_time_embed")
        return emb

    worst_new = worst_ctl = 0.0
    for t in (torch.tensor([0.6]), torch.tensor([1.0, 0.9, 0.31, 0.05, 0.0])):  # t_len 1 and N; the solver's range [0, 1] with both ends
        for labels in (False, True):
            emb, emb16 = song(d(t), labels)
            ref = sc.song_mapping_ref64(w0, b0, w1, b1, t, N, *((lab_w, lab_b, y) if labels else ()))
            ctl = adm(d(t), labels)
            ctl_ref = sc.adm_time_embed_ref64(w0, b0, w1, b1, t, N, *((adm_table, y) if labels else ()))
            e_new, e_ctl = float((emb.double().cpu() - ref).abs().max()), float((ctl.double().cpu() - ctl_ref).abs().max())
            print(f"F={F} t_len={t.numel()} labels={labels}: lfm_song_embed {e_new:.3e}  lfm_time_embed (control) {e_ctl:.3e}  |emb| max {float(ref.abs().max()):.2f}")
            # the fp16 copy is the fp32 value rounded once more: within half an fp16 ulp of it (a fused multiply-convert may round the exact product instead,
            # which differs from rounding the fp32 value by one fp16 ulp on near-ties)
            assert bool(((emb16.double() - emb.double()).abs() <= 2.0 ** -11 * (1 + 2.0 ** -10) * emb.double().abs() + 2.0 ** -25).all())
            worst_new, worst_ctl = max(worst_new, e_new), max(worst_ctl, e_ctl)
    print(f"F={F}: worst lfm_song_embed {worst_new:.3e}, worst control {worst_ctl:.3e}, ratio {worst_new / worst_ctl:.2f}")
    assert worst_ctl < 1e-5  # the control itself is sane (fp32 round-off of O(1) sums)
    assert worst_new <= 2 * worst_ctl
    bad = d(torch.tensor([3, rows, 6, -1, 5]))  # out of range on rows 1 and 3: poisoned, the others untouched
    emb, emb16 = song(d(torch.tensor([0.6])), True, bad)
    good, _ = song(d(torch.tensor([0.6])), True)
    assert bool(emb[[1, 3]].isnan().all()) and bool(emb16[[1, 3]].isnan().all()) and torch.equal(emb[[0, 2, 4]], good[[0, 2, 4]])


# ------------------------------------------------------------------------------------------------ the model against the reference
def _song(rec, dev):
    from lfm_amd.models.EDM import SongUNet

    m = SongUNet(**rec["cfg"])
    checksum = sc.load_seeded(m, rec["state_seed"])
    assert abs(checksum - rec["state_checksum"]) <= 1e-9 * rec["state_checksum"], "the seeded state differs from the one the reference was run with"
    return m.to(dev).eval()


@pytest.fixture(scope="module")
def tiny(golden_dir):
    rec = _rec(golden_dir, "song_tiny.pt")
    return rec, _song(rec, torch.device("cuda:0"))


def test_song_tiny_matches_reference_golden(tiny):
    rec, m = tiny
    dev = torch.device("cuda:0")
    x, y = rec["x"].to(dev), rec["y"].to(dev)
    assert float(rec["v_t0d"].abs().mean()) > 1e-2
    a = m(torch.tensor(0.6, device=dev), x, y).clone()
    errs = dict(t0d=rel_l2(a, rec["v_t0d"]), tN=rel_l2(m(rec["tN"].to(dev), x, y), rec["v_tN"]),
                nolabel=rel_l2(m(torch.tensor(0.6, device=dev), x), rec["v_nolabel"]))
    print("song_tiny rel-L2 vs reference:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < 3e-3, errs
    assert torch.equal(a, m(torch.tensor(0.6, device=dev), x, y))  # bit-repeatable
    with pytest.raises(IndexError):
        m(torch.tensor(0.6, device=dev), x, torch.tensor([1, 5, 0, 2], device=dev))  # label_dim is 5


def test_song_tiny_euler_solve_captured_and_uncaptured(tiny):
    from lfm_amd.test_flow_latent import sample_from_model

    rec, m = tiny
    dev = torch.device("cuda:0")
    x, kw = rec["x"].to(dev), dict(y=rec["y"].to(dev))
    args = Namespace(method="euler", step_size=0.1, perturb=False, compute_nfe=False, cfg_scale=1.0, atol=1e-5, rtol=1e-5)
    fused = sample_from_model(m, x, kw, args)[-1]
    assert m._fused_solvers and all(fg.graphs for fg in m._fused_solvers.values())  # the captured path is what ran
    e_ref = rel_l2(fused, rec["x_euler10"])
    args.fused = False
    e_unc = rel_l2(sample_from_model(m, x, kw, args)[-1], fused)
    print(f"song_tiny 10 Euler steps: captured vs reference {e_ref:.3e}, uncaptured vs captured {e_unc:.3e}")
    assert e_ref < 1e-3 and e_unc < 1e-5
    args.fused, args.cfg_scale = True, 1.7
    with pytest.raises(NotImplementedError, match="SongUNet"):
        sample_from_model(m, torch.cat([x, x]), dict(y=torch.cat([kw["y"], kw["y"]]), cfg_scale=1.7), args)


def test_song_wide_one_256_channel_head_on_the_streamed_kernel(golden_dir):
    from lfm_amd import hip

    rec = _rec(golden_dir, "song_wide.pt")
    dev = torch.device("cuda:0")
    m = _song(rec, dev)
    assert hip.unet_attention_plan(2, 256, 1, 256) == 3  # 16x16 tokens x one 256-channel head: the streamed kernel is what runs
    x = rec["x"].to(dev)
    assert float(rec["v_t0d"].abs().mean()) > 1e-2
    errs = dict(t0d=rel_l2(m(torch.tensor(0.6, device=dev), x), rec["v_t0d"]), tN=rel_l2(m(rec["tN"].to(dev), x), rec["v_tN"]))
    print("song_wide rel-L2 vs reference:", {k: f"{v:.3e}" for k, v in errs.items()})
    assert max(errs.values()) < 3e-3, errs


# ------------------------------------------------------------------------------------------------ guided adm on the fixed grids
@pytest.fixture(scope="module")
def guided(golden_dir):
    from lfm_amd.models.EDM import DhariwalUNet

    tiny_rec = _rec(golden_dir, "edm_tiny.pt")
    m = DhariwalUNet(**tiny_rec["cfg"])
    m.load_state_dict({k: (v.float() if v.is_floating_point() else v) for k, v in tiny_rec["state_dict"].items()}, strict=True)
    return _rec(golden_dir, "edm_cfg_grid.pt"), m.to("cuda:0").eval()


def _solve(m, x, y, cfg_scale, how, fused):
    from lfm_amd.sampler.karras_sample import karras_sample
    from lfm_amd.test_flow_latent import sample_from_model

    kw = dict(y=y, cfg_scale=cfg_scale)
    if how == "euler10":
        args = Namespace(method="euler", step_size=0.1, perturb=False, compute_nfe=False, cfg_scale=cfg_scale, atol=1e-5, rtol=1e-5, fused=fused)
        return sample_from_model(m, x, kw, args)[-1]
    return karras_sample(m, x, steps=6, model_kwargs=kw, device=x.device, clip_denoised=False, sigma_min=1e-5, sigma_max=1.0, s_tmin=0.0, s_tmax=1.0,
                         s_churn=0.0, sampler=how.split("_")[1], rho=1.0, fused=fused)


@pytest.mark.parametrize("how", ["euler10", "karras_euler", "karras_heun"])
def test_guided_adm_on_the_fixed_grids_through_the_captured_solver(guided, how):
    rec, m = guided
    dev = torch.device("cuda:0")
    x, y, s = rec["x"].to(dev), rec["y"].to(dev), rec["cfg_scale"]
    n = x.shape[0] // 2
    out = _solve(m, x, y, s, how, True)
    fgs = [fg for fg in m._fused_solvers.values() if fg.use_cfg]
    assert fgs and all(fg.graphs and fg.host_cfg for fg in fgs)  # guidance ran inside captured graphs
    e_ref = rel_l2(out, rec["x_" + how])
    e_unc = rel_l2(_solve(m, x, y, s, how, False), out)
    print(f"guided adm {how}: captured vs reference {e_ref:.3e}, uncaptured vs captured {e_unc:.3e}")
    assert e_ref < 1e-3 and e_unc < 1e-5
    assert torch.equal(out[:n], out[n:])
    # other labels on the SAME captured graphs: they are read from the solver's buffer at replay, not baked in at capture
    graphs = {id(g) for fg in fgs for g in fg.graphs.values()}
    y2 = torch.tensor([0, 4, 0, 0], device=dev)
    out2 = _solve(m, x, y2, s, how, True)
    assert {id(g) for fg in m._fused_solvers.values() if fg.use_cfg for g in fg.graphs.values()} == graphs
    assert rel_l2(out2, out) > 1e-2  # the labels matter
    assert rel_l2(_solve(m, x, y2, s, how, False), out2) < 1e-5


def test_guidance_is_still_refused_where_there_is_no_forward_with_cfg():
    from lfm_amd.models.unet import UNetModel

    dev = torch.device("cuda:0")
    m = UNetModel(image_size=16, in_channels=4, model_channels=64, out_channels=4, num_res_blocks=1, attention_resolutions=(2,), channel_mult=(1, 2),
                  num_classes=5, num_heads=1).to(dev).eval()
    x = torch.zeros(2, 4, 16, 16, device=dev)
    with pytest.raises(NotImplementedError, match="UNetModel"):
        _solve(m, x, torch.zeros(2, dtype=torch.long, device=dev), 1.7, "euler10", True)


# ------------------------------------------------------------------------------------------------ the driver
def test_single_process_driver_ddpm_plus_plus(tmp_path):
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run([sys.executable, "-m", "lfm_amd.test_flow_latent", "--model_type", "ddpm++", "--image_size", "128", "--f", "8", "--num_in_channels", "4",
                        "--num_out_channels", "4", "--nf", "64", "--ch_mult", "1", "2", "--num_res_blocks", "1", "--attn_resolutions", "8", "--random_weights",
                        "--generator", "device", "--batch_size", "2", "--method", "euler", "--step_size", "0.2", "--save_dir", str(tmp_path)],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert os.listdir(tmp_path) == ["samples_cifar10_euler_1e-05_1e-05.jpg"]
    import numpy as np
    from PIL import Image

    img = np.asarray(Image.open(tmp_path / "samples_cifar10_euler_1e-05_1e-05.jpg"), dtype=np.float64)
    assert img.shape == (128, 256, 3) and np.isfinite(img).all() and img.std() > 1.0  # two 128x128 images, not a constant sheet
