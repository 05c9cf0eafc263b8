"""CPU: the cases and references of the VAE stage tests (tests/vae_stage_cases.py) are themselves checked here -- every case builds with its caps, the
float64 stage references agree with the fp32 oracle (oracle/vae_ref.py) on the same data, the checks reject the specific wrong answers they exist for,
and the four stage entry points refuse bad arguments before any launch (no GPU needed: integers stand in for the pointers)."""
import ctypes as C

import pytest
import torch

import gemm_exact_cases as gc
import vae_stage_cases as vc
from oracle import vae_ref as vr

ORACLE_TOL = 1e-5  # rel-L2: fp32 round-off of O(1) sums


def nchw(rows, n, H, W):
    return rows.reshape(n, H, W, -1).permute(0, 3, 1, 2).float().contiguous()


def rows_of(t):
    return t.permute(0, 2, 3, 1).reshape(-1, t.shape[1])


def conv_w(Wt, cin):
    """[Cout, 9 Cin] (tap, ci) -> torch [Cout, Cin, 3, 3]."""
    return Wt.reshape(Wt.shape[0], 3, 3, cin).permute(0, 3, 1, 2).float().contiguous()


# ------------------------------------------------------------------------------------------------ every case builds, its caps hold
def test_every_exact_case_builds_within_its_caps():
    tops = []
    for n, R in vc.CONV_IN_SHAPES:
        tops.append(float(vc.conv_in_exact(n, R).ref.abs().max()))
    for s in vc.DOWN_SHAPES:
        tops.append(float(vc.down_exact(*s).ref.abs().max()))
    assert max(tops) <= gc.CAP16
    top32 = max(float(vc.moments_exact(*s).ref.abs().max()) for s in vc.MOMENTS_SHAPES)
    assert gc.CAP16 < top32 < gc.CAP32
    print(f"exact cases: largest fp16-out |ref| {max(tops):.0f}, largest fp32-out |ref| {top32:.0f}")


def test_every_gauss_case_builds_with_a_positive_finite_bound():
    cases = [vc.conv_in_gauss(*s) for s in vc.CONV_IN_GAUSS_SHAPES] + [vc.down_gauss(*s) for s in vc.DOWN_SHAPES] + [vc.moments_gauss(*s) for s in vc.MOMENTS_SHAPES]
    for c in cases:
        assert torch.isfinite(c.ref).all() and torch.isfinite(c.bound).all() and float(c.bound.min()) > 0
        assert c.ref.shape == c.bound.shape
        # the worst-case bound grows with K: 1.3e-2 of an O(1) output at K = 4608 (C = 512), 2e-3 at K = 576.  What is below it at the wide shapes is
        # the exact family's to catch; the controls below show what this one rejects.
        assert float((c.bound / (c.ref.abs() + 1)).max()) < 2e-2


def test_mode3_reads_2oy_plus_ky_and_zero_beyond_the_bottom_right():
    """gc.conv_cols mode 3 against a direct loop on a tiny map."""
    N, H, W, Cin = 2, 2, 3, 2
    x = torch.arange(N * 2 * H * 2 * W * Cin, dtype=torch.int64).reshape(N, 2 * H, 2 * W, Cin) + 1
    cols = gc.conv_cols(x, N, H, W, Cin, 3).reshape(N, H, W, 9, Cin)
    for n in range(N):
        for oy in range(H):
            for ox in range(W):
                for ky in range(3):
                    for kx in range(3):
                        iy, ix = 2 * oy + ky, 2 * ox + kx
                        want = x[n, iy, ix] if iy < 2 * H and ix < 2 * W else torch.zeros(Cin, dtype=torch.int64)
                        assert torch.equal(cols[n, oy, ox, ky * 3 + kx], want), (n, oy, ox, ky, kx)


# ------------------------------------------------------------------------------------------------ the references against the fp32 oracle
@pytest.mark.parametrize("n,R", [(3, 5), (2, 8)])
def test_conv_in_reference_matches_the_oracle(n, R):
    c = vc.conv_in_gauss(n, R)
    sd = {"post_quant_conv.weight": c.pq_w.float().reshape(4, 4, 1, 1), "post_quant_conv.bias": c.pq_b.float(),
          "decoder.conv_in.weight": c.cin_w.float(), "decoder.conv_in.bias": c.cin_b.float()}
    h = vr._conv(sd, "decoder.conv_in", vr._conv(sd, "post_quant_conv", c.z.float(), 0), 1)  # as vr.vae_decode applies them
    assert vc.rel_l2(rows_of(h), c.ref) < ORACLE_TOL


@pytest.mark.parametrize("shape", vc.DOWN_SHAPES)
def test_downsample_reference_matches_the_oracle(shape):
    n, Ho, Wo, Cc = shape
    c = vc.down_gauss(*shape)
    sd = {"d.weight": conv_w(c.Wt, Cc), "d.bias": c.bias.float()}
    got = vr.downsample(sd, "d", nchw(c.x, n, 2 * Ho, 2 * Wo))
    assert vc.rel_l2(rows_of(got), c.ref) < ORACLE_TOL
    e = vc.down_exact(*shape)
    sd = {"d.weight": conv_w(e.Wt, Cc), "d.bias": e.bias.float()}
    assert torch.equal(rows_of(vr.downsample(sd, "d", nchw(e.x, n, 2 * Ho, 2 * Wo))).double(), e.ref.double())  # integers: fp32 is exact too


@pytest.mark.parametrize("shape", vc.MOMENTS_SHAPES)
def test_moments_reference_matches_the_oracle(shape):
    n, H, W = shape
    c = vc.moments_gauss(*shape)
    sd = {"o.weight": conv_w(c.Wt, 512), "o.bias": c.bias.float()}
    got = vr._conv(sd, "o", nchw(c.x, n, H, W), 1)  # NCHW [n, 8, H, W]: the layout of the moments
    assert vc.rel_l2(got.reshape(n * 8, H * W), c.ref) < ORACLE_TOL


def oracle_resnet(p, x_rows, n, H, W):
    cin, cout = x_rows.shape[1], p["c1_w"].shape[0]
    sd = {"r.norm1.weight": p["n1_g"].float(), "r.norm1.bias": p["n1_b"].float(), "r.conv1.weight": conv_w(p["c1_w"], cin), "r.conv1.bias": p["c1_b"].float(),
          "r.norm2.weight": p["n2_g"].float(), "r.norm2.bias": p["n2_b"].float(), "r.conv2.weight": conv_w(p["c2_w"], cout), "r.conv2.bias": p["c2_b"].float()}
    if p["sc_w"] is not None:
        sd["r.conv_shortcut.weight"], sd["r.conv_shortcut.bias"] = p["sc_w"].float().reshape(cout, cin, 1, 1), p["sc_b"].float()
    return rows_of(vr.resnet(sd, "r", nchw(x_rows, n, H, W)))


@pytest.mark.parametrize("widths,H,W", vc.resnet_case_list())
def test_resnet_reference_matches_the_oracle(widths, H, W):
    c = vc.resnet_case(widths, H, W)
    h = c.x
    for p in c.params:
        h = oracle_resnet(p, h, c.n, H, W)
    assert vc.rel_l2(h, c.ref64) < ORACLE_TOL


# ------------------------------------------------------------------------------------------------ controls: the checks are not vacuous
@pytest.mark.parametrize("shape", vc.DOWN_SHAPES)
def test_control_mode2_answer_fails_the_downsample_checks(shape):
    n, Ho, Wo, Cc = shape
    e = vc.down_exact(*shape)
    assert gc.check(gc.embed(e.mode2, fill=gc.SENTINEL, dtype=torch.float16), e.ref, e.M, Cc).diffs  # what assert_exact would refuse
    g = vc.down_gauss(*shape)
    last_row, last_col = vc.last_row_col(n, Ho, Wo)
    excess = ((g.mode2 - g.ref).abs() / g.bound)[last_row | last_col]
    assert float(excess.max()) > 10, float(excess.max())


@pytest.mark.parametrize("widths,H,W", [t for t in vc.resnet_case_list() if any(a != b for a, b in t[0])])
def test_control_shortcut_mistakes_exceed_the_resnet_cap(widths, H, W):
    c = vc.resnet_case(widths, H, W)
    assert vc.resnet_within_cap(c.ref_r, c)[0]  # the ideal implementation passes (ratios 1, 1)
    for wrong in (dict(drop_sc_bias=True), dict(identity_skip=True)):
        ok, a, b = vc.resnet_within_cap(vc.resnet_control(c, **wrong), c)
        print(f"control {wrong} {widths} {H}x{W}: relL2 ratio {a:.1f}, maxabs ratio {b:.1f}")
        assert not ok and a > vc.RESNET_MARGIN and b > vc.RESNET_MARGIN, (wrong, a, b)


@pytest.mark.parametrize("n,R", vc.CONV_IN_GAUSS_SHAPES[:4])
def test_control_post_quant_bias_in_the_padding_fails_on_the_border(n, R):
    c = vc.conv_in_gauss(n, R)
    wrong = vc.conv_in_ref(c.z, c.pq_w, c.pq_b, c.cin_w, c.cin_b, bias_in_padding=True)
    bad = (wrong - c.ref).abs() > c.bound
    edge = vc.border_rows(n, R)
    assert bool(bad[edge].any()) and not bool(bad[~edge].any())
    e = vc.conv_in_exact(n, R)
    wrong = vc.conv_in_ref(e.z, e.pq_w, e.pq_b, e.cin_w, e.cin_b, bias_in_padding=True)
    assert bool((wrong != e.ref)[edge].any()) and not bool((wrong != e.ref)[~edge].any())


@pytest.mark.parametrize("widths,H,W", vc.resnet_case_list())
def test_resnet_model_error_is_sane(widths, H, W):
    c = vc.resnet_case(widths, H, W)
    print(f"REF_R {widths} {H}x{W}: relL2(ref_r, ref64) {c.e_l2:.3e}, maxabs(ref_r - ref64) {c.e_max:.3e}")
    assert 0 < c.e_l2 < 2e-3 and c.e_max > 0


# ------------------------------------------------------------------------------------------------ refusals (validation precedes any launch)
OK, SHAPE, ALIGN, WORKSPACE, ARG = 0, -1, -2, -3, -5
P, ODD = 0x100000, 0x100002  # a 256-byte aligned and a misaligned stand-in for a device pointer


@pytest.fixture(scope="module")
def L():
    from lfm_amd import hip

    return hip.lib()


def test_conv_in_refusals(L):
    args = [P] * 6
    assert L.lfm_vae_conv_in_f16(*args, 0, 8, None) == SHAPE and L.lfm_vae_conv_in_f16(*args, 1, 0, None) == SHAPE
    assert L.lfm_vae_conv_in_f16(*args, 1, 4096, None) == SHAPE  # 2^24 pixels x 512 channels: beyond 32-bit element offsets
    for i in range(6):
        assert L.lfm_vae_conv_in_f16(*[None if j == i else P for j in range(6)], 1, 8, None) == ARG, i
        assert L.lfm_vae_conv_in_f16(*[ODD if j == i else P for j in range(6)], 1, 8, None) == ALIGN, i


def test_downsample_refusals(L):
    f, wsb = L.lfm_vae_downsample_f16, L.lfm_vae_downsample_workspace_bytes
    assert wsb(1, 4, 4, 64) == 256 and wsb(1, 4, 4, 96) == 0 and wsb(0, 4, 4, 64) == 0 and wsb(1, 0, 4, 64) == 0 and wsb(1, 4, 0, 64) == 0
    assert wsb(1, 1024, 1024, 512) == 0  # 2^31 input elements
    for bad in ((1, 4, 4, 96), (0, 4, 4, 64), (1, 0, 4, 64), (1, 4, 0, 64), (1, 4, 4, 0)):
        assert f(P, P, P, P, P, 256, *bad, None) == SHAPE, bad
    for i in range(5):
        assert f(*[None if j == i else P for j in range(5)], 256, 1, 4, 4, 64, None) == ARG, i
        assert f(*[ODD if j == i else P for j in range(5)], 256, 1, 4, 4, 64, None) == ALIGN, i
    assert f(P, P, P, P, P + 16, 256, 1, 4, 4, 64, None) == ALIGN  # the workspace: 256 bytes
    assert f(P, P, P, P, P, 255, 1, 4, 4, 64, None) == WORKSPACE


def test_moments_refusals(L):
    f, wsb = L.lfm_vae_conv_moments_f32, L.lfm_vae_conv_moments_workspace_bytes
    assert wsb(1, 4, 4) == 256 and wsb(0, 4, 4) == 0 and wsb(1, 0, 4) == 0 and wsb(1, 4, 0) == 0 and wsb(1, 2048, 2048) == 0
    for bad in ((0, 4, 4), (1, 0, 4), (1, 4, 0), (1, 2048, 2048)):
        assert f(P, P, P, P, P, 256, *bad, None) == SHAPE, bad
    for i in range(5):
        assert f(*[None if j == i else P for j in range(5)], 256, 1, 4, 4, None) == ARG, i
        assert f(*[ODD if j == i else P for j in range(5)], 256, 1, 4, 4, None) == ALIGN, i
    assert f(P, P, P, P, P + 16, 256, 1, 4, 4, None) == ALIGN
    assert f(P, P, P, P, P, 255, 1, 4, 4, None) == WORKSPACE


def fake_resnets(widths):
    from lfm_amd import hip

    arr = (hip.VaeResnet * len(widths))()
    for r, (cin, cout) in zip(arr, widths):
        for name in vc.PARAM_NAMES:
            setattr(r, name, P if (cin != cout or not name.startswith("sc_")) else None)
        r.cin, r.cout = cin, cout
    return arr


def test_resnets_refusals(L):
    f, wsb = L.lfm_vae_resnets_f16, L.lfm_vae_resnets_workspace_bytes
    need = wsb(2, 16, 16)
    assert need > 4 * 2 * 256 * 512 * 2 and wsb(0, 16, 16) == 0 and wsb(2, 0, 16) == 0 and wsb(2, 16, 0) == 0 and wsb(1, 2048, 2048) == 0
    one = fake_resnets([(256, 128)])

    def call(r=one, n_res=1, x=P, out=P, ws=P, nbytes=need, n=2, H=16, W=16):
        return f(r, n_res, x, out, ws, nbytes, n, H, W, 1, None, None)

    assert call(n_res=0) == SHAPE and call(r=fake_resnets([(128, 128)] * 4), n_res=4) == SHAPE
    assert call(n=0) == SHAPE and call(H=0) == SHAPE and call(W=0) == SHAPE
    assert call(r=fake_resnets([(256, 192)])) == SHAPE and call(r=fake_resnets([(64, 128)])) == SHAPE
    assert call(r=fake_resnets([(256, 128), (256, 128)]), n_res=2) == SHAPE  # the widths do not chain
    no_sc = fake_resnets([(256, 128)])
    no_sc[0].sc_w = None
    assert call(r=no_sc) == SHAPE  # an identity skip needs equal widths
    assert call(r=None) == ARG and call(x=None) == ARG and call(out=None) == ARG and call(ws=None) == ARG
    for name in vc.PARAM_NAMES:
        bad = fake_resnets([(256, 128)])
        setattr(bad[0], name, ODD)
        assert call(r=bad) == ALIGN, name
        if name != "sc_w":
            setattr(bad[0], name, None)
            assert call(r=bad) == ARG, name
    assert call(x=ODD) == ALIGN and call(out=ODD) == ALIGN and call(ws=P + 16) == ALIGN
    assert call(nbytes=need - 1) == WORKSPACE


# ------------------------------------------------------------------------------------------------ the carved workspaces (host arithmetic, no GPU)
def a(v):
    return (v + 255) // 256 * 256


def coder_bytes(R, c):  # include/lfm_hip.h: lfm_vae_workspace_bytes
    if R <= 0 or c <= 0 or R % 8:
        return 0
    return 4 * a(c * (8 * R) ** 2 * 512) + a(c * 256) + a(c * max((8 * R) ** 2 // 2, 8192) * 8) + 256 + a(c * R ** 4 * 4)


def attention_bytes(n, T):  # lfm_vae_mid_attention_workspace_bytes
    if n <= 0 or T <= 0 or T % 64:
        return 0
    return 256 + a(n * 256) + a(n * max(32 * T, 8192) * 8) + 4 * a(n * T * (512 + max(512, T)) * 2) + a(n * T * T * 4)


def resnets_bytes(n, H, W):  # lfm_vae_resnets_workspace_bytes
    if n <= 0 or H <= 0 or W <= 0 or n * H * W * 512 >= 2 ** 31:
        return 0
    return 256 + a(n * 256) + a(n * max(2 * -(-H * W // 256) * 128, 8192) * 8) + 4 * a(n * H * W * 512 * 2)


def test_workspace_bytes_follow_the_header_formulas(L):
    for R in (0, 4, 8, 16, 24, 32, 64):
        for c in (0, 1, 2, 3, 8, 64):
            assert L.lfm_vae_workspace_bytes(R, c) == coder_bytes(R, c), (R, c)
    for n in (0, 1, 2, 3, 7):
        for T in (0, 64, 100, 128, 576, 1024, 4096):
            assert L.lfm_vae_mid_attention_workspace_bytes(n, T) == attention_bytes(n, T), (n, T)
        for H, W in ((0, 4), (4, 4), (16, 16), (8, 24), (17, 5), (64, 64), (2048, 2048)):
            assert L.lfm_vae_resnets_workspace_bytes(n, H, W) == resnets_bytes(n, H, W), (n, H, W)


def test_decode_and_encode_refusals(L):
    """Misaligned before short (a workspace that is both answers LFM_ERR_ALIGN), after the arguments and the shape."""
    need = L.lfm_vae_workspace_bytes(8, 2)
    assert need > 0
    for f in (L.lfm_vae_decode, L.lfm_vae_encode):
        assert f(P, P + 16, need, P, P, 3, 8, 2, None) == ALIGN
        assert f(P, P, need - 1, P, P, 3, 8, 2, None) == WORKSPACE
        assert f(P, P + 16, need - 1, P, P, 3, 8, 2, None) == ALIGN
        for i in range(4):
            assert f(*[None if j == i else P for j in range(2)], need, *[None if j == i else P for j in range(2, 4)], 3, 8, 2, None) == ARG, i
        for bad in ((0, 8, 2), (3, 0, 2), (3, 12, 2), (3, 8, 0)):
            assert f(P, P, need, P, P, *bad, None) == SHAPE, bad
