"""GPU: the VAE mid-block attention (VaeCtx::mid_attention through lfm_vae_mid_attention_f16) against float64 on constructed inputs.

oracle/vae_attention_ref.py builds six input families (diffuse: what the whole-decode tests produce; peaked; self_match with logits to +200;
planted spiky tokens; every logit near +200 / -200) and two references: `exact`, float64 throughout, and `staged`, float64 rounded where the device
stores a tensor.  A result passes when it is finite and its error on the attention branch out - x is at most 2 x e_stage, e_stage being the branch
error of `staged` for that very case -- computed here on the CPU from the two references, never from the code under test.  The device differs from
`staged` only in fp32 accumulation order and the hardware exp2, so its error is another draw of e_stage's size; every emulated softmax mistake
that shows at all sits at 13 x or more (tests/test_vae_attention_ref.py).

Shapes: (1, 64) is one partial tile in M and N of the score GEMM and a single K-tile in P V; (3, 576) and (1, 1600) have a ragged last 128-row
tile per image, at (3, 576) with a neighbouring image on both sides (checked per image too: a write into the neighbour's rows hits one image);
(1, 4096) is the 512-pixel decode's T, where p ~ 2.4e-4 sits near the bottom of fp16's normal range.

Measured error / e_stage on an MI355X: NOT MEASURED YET -- this module has not run on a GPU.  Every case prints its ratio (`pytest -s`, lines that
begin with MEASURED); the first GPU run's figures belong here.  On the CPU, `staged` with the softmax in fp32 arithmetic (what the kernel does) lands
at 1.0 x in every family (tests/test_vae_attention_ref.py).
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

from oracle import vae_attention_ref as ar  # checker only

CASES = ([(f, n, T) for (n, T) in ((1, 64), (3, 576), (2, 1024)) for f in ar.FAMILIES] +
         [("peaked", 1, 1600), ("planted", 1, 1600), ("diffuse", 1, 4096), ("peaked", 1, 4096)])
PARAMS = ("gamma", "beta", "q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "o_w", "o_b")


def call(case_dev, x, out, ws, n, T, ws_bytes=None):
    from lfm_amd import hip

    w = [hip.ptr(case_dev[k]) for k in PARAMS]
    return hip.lib().lfm_vae_mid_attention_f16(hip.ptr(x), hip.ptr(out), *w, hip.ptr(ws), ws.numel() if ws_bytes is None else ws_bytes, n, T,
                                               hip.stream_ptr())


def workspace(n, T, dev):
    """Filled with 0xFF bytes: NaN as fp16 and as fp32, so a read of anything the call did not write shows."""
    from lfm_amd import hip

    nbytes = hip.lib().lfm_vae_mid_attention_workspace_bytes(n, T)
    assert nbytes > 0
    return torch.full((nbytes,), 255, dtype=torch.uint8, device=dev)


def run(case_dev, x, n, T):
    from lfm_amd import hip

    out = torch.full_like(x, float("nan"))
    hip.check(call(case_dev, x, out, workspace(n, T, x.device), n, T), "lfm_vae_mid_attention_f16")
    torch.cuda.synchronize()
    return out


@pytest.mark.parametrize("family,n,T", CASES, ids=[f"{f}-{n}x{T}" for f, n, T in CASES])
def test_mid_attention_vs_fp64(family, n, T):
    dev = torch.device("cuda:0")
    case = ar.make_case(family, n, T)
    case_dev = {k: case[k].to(dev) for k in PARAMS}
    x = case["x"].to(dev)
    got = run(case_dev, x, n, T)
    again = run(case_dev, x, n, T)
    ok, ratio, es = ar.check(got, case)
    print(f"MEASURED {family} n={n} T={T}: error / e_stage {ratio:.3f} (e_stage {es:.2e})")
    assert torch.isfinite(got).all()
    assert torch.equal(got.view(torch.int16), again.view(torch.int16))  # bit-identical, NaNs included
    assert ok, (family, n, T, ratio, es)
    if n > 1:
        for i in range(n):
            ok, ratio, es = ar.check(got, case, image=i)  # whole-tensor norms dilute a write into a neighbour's rows
            print(f"MEASURED {family} n={n} T={T} image {i}: error / e_stage {ratio:.3f} (e_stage {es:.2e})")
            assert ok, (family, n, T, i, ratio, es)
            alone = run(case_dev, x[i:i + 1].contiguous(), 1, T)  # the per-row arithmetic does not depend on n
            assert torch.equal(alone[0].view(torch.int16), got[i].view(torch.int16)), (family, n, T, i)


def test_mid_attention_refusals_leave_out_untouched():
    from lfm_amd import hip

    dev = torch.device("cuda:0")
    L = hip.lib()
    n, T = 1, 64
    case = ar.make_case("diffuse", n, T)
    case_dev = {k: case[k].to(dev) for k in PARAMS}
    x = case["x"].to(dev)
    ws = workspace(n, T, dev)
    out = torch.full_like(x, float("nan"))
    assert L.lfm_vae_mid_attention_workspace_bytes(1, 100) == 0
    x100 = torch.zeros(1, 100, ar.C, dtype=torch.float16, device=dev)
    out100 = torch.full_like(x100, float("nan"))
    assert call(case_dev, x100, out100, ws, 1, 100) == -1  # LFM_ERR_SHAPE: the decoder's T is a multiple of 64
    assert call(case_dev, x, out, ws, n, T, ws_bytes=ws.numel() - 1) == -3  # LFM_ERR_WORKSPACE
    shifted = torch.zeros(x.numel() + 1, dtype=torch.float16, device=dev)[1:].view_as(x)
    shifted.copy_(x)
    assert shifted.data_ptr() % 16 == 2
    assert call(case_dev, shifted, out, ws, n, T) == -2  # LFM_ERR_ALIGN
    assert call(case_dev, x, out, ws, 0, T) == -1
    assert L.lfm_vae_mid_attention_f16(None, hip.ptr(out), *[hip.ptr(case_dev[k]) for k in PARAMS], hip.ptr(ws), ws.numel(), n, T,
                                       hip.stream_ptr()) == -5  # LFM_ERR_ARG
    torch.cuda.synchronize()
    assert torch.isnan(out).all() and torch.isnan(out100).all()
    hip.check(call(case_dev, x, out, ws, n, T), "lfm_vae_mid_attention_f16")  # the same arguments, whole: accepted
    torch.cuda.synchronize()
    assert ar.check(out, case)[0]
