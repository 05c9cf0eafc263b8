"""CPU side of the tiled DiT attention kernel (csrc/attention_tiled_kernel.h): that the bounds the GPU test asserts are sound, the chooser's truth table, the
constructor, and the 12 x 12-grid golden of the unmodified reference.

Bounds (tests/dit_attention_cases.py: TOL_*, rel-L2 against float64): whole tensor 2e-3 and worst (image, head) item 4e-3 are tests/test_gpu_dit.py::test_attention's;
worst query row 4e-3 is new.  Measured here with the fp16-staged emulation (P rounded to fp16, fp32 sums, fp16 output) over dit_attention_cases.SHAPES:
    correct emulation    whole <= 1.74e-4   item <= 1.80e-4   row <= 4.28e-4     (a quarter of the bounds: 5e-4 / 1e-3 / 1e-3)
    drop_last16          whole >= 0.529     item >= 0.586     row >= 1.48        every item >= 0.468
    leak_next16          whole >= 0.338     item >= 0.338     row >= 0.874
    no_rescale           whole >= 0.708     item >= 0.727     row >= 0.981
    tail_no_vt_pos       whole >= 0.639     item >= 0.664     row >= 1.43
    pad72_not_zeroed     whole >= 0.481     item >= 0.500     row >= 6.30        (head_dim 72 shapes)
so every named mistake sits two orders of magnitude above four times each bound (8e-3 / 1.6e-2 / 1.6e-2)."""
import os

import pytest
import torch

import dit_attention_cases as ac
from oracle import dit_ref


@pytest.mark.parametrize("T,heads,batch,hd", ac.SHAPES)
def test_bounds_are_sound(T, heads, batch, hd):
    q, k, v, ref = ac.case(T, heads, batch, hd)
    whole, item, row = ac.errors(ac.emulate(q, k, v), ref)
    print(f"emulation {T=} {hd=}: whole {whole:.3e} item {item:.3e} row {row:.3e}")
    assert whole < ac.TOL_WHOLE / 4 and item < ac.TOL_ITEM / 4 and row < ac.TOL_ROW / 4, (whole, item, row)
    for mistake in ac.MISTAKES:
        if mistake == "pad72_not_zeroed" and hd != 72:
            continue
        got = ac.emulate(q, k, v, mistake)
        whole, item, row = ac.errors(got, ref)
        print(f"  {mistake}: whole {whole:.3e} item {item:.3e} row {row:.3e}")
        assert whole > 4 * ac.TOL_WHOLE and item > 4 * ac.TOL_ITEM and row > 4 * ac.TOL_ROW, (mistake, whole, item, row)
        if mistake == "drop_last16":  # ... on EVERY item: no item passes without its tail
            d = got.double() - ref
            assert float((d.pow(2).sum((2, 3)).sqrt() / ref.pow(2).sum((2, 3)).sqrt()).min()) >= 4.6e-2


def test_spiky_keys_sit_where_the_tails_are():
    for T, _, _, _ in ac.SHAPES:
        keys = ac.spiky_keys(T)
        nst = (T + 63) // 64
        assert any(k < 16 for k in keys) and any(k >= T - 16 for k in keys)
        assert any(0 < k // 64 < nst - 1 for k in keys)            # a middle stage
        assert any(k // 64 == T // 64 - 1 for k in keys)           # the last full stage


NEW_TOKENS = (144, 400, 576, 784, 1296, 2304, 3600)
RESIDENT = {64: 2, 128: 2, 1024: 4}  # token count -> the kernel that owns it at 64 items (256: head_dim 64 takes the query split, 72 the per-item kernel)


def test_chooser_truth_table():
    """attention_choose with the tiled kernel, written from the rules: by default 7 exactly for head_dim 64 / 72 and the square grids of a side that is a multiple
    of 4 from 144 to 3600 tokens that no other kernel serves; LFM_OPT_ATTENTION_TILED = 0 refuses those, = 2 sends every T % 16 == 0, 16 <= T < 4096 there."""
    from lfm_amd import hip

    plan = hip.attention_plan
    for hd in (64, 72):
        for T in NEW_TOKENS:
            for batch, heads in ((1, 1), (4, 16), (64, 16)):
                assert plan(batch, heads, hd, T) == 7, (batch, heads, hd, T)
    for T in (160, 288, 4096, 100, 1600 + 16, 3600 + 16, 3844, 4624):  # not a square; 4096 and beyond stay refused; 62^2: the side is no multiple of 4
        assert plan(4, 16, 64, T) == -1 and plan(4, 16, 72, T) == -1, T
    for T in NEW_TOKENS:
        assert plan(4, 16, 80, T) == -1
    # the Python rule a DiT is constructed by is the chooser's, for every token count
    for T in range(0, 4200):
        assert hip.dit_tokens_served(T) == (plan(1, 6, 64, T) > 0) == (plan(1, 16, 72, T) > 0), T
    before = {(hd, T): plan(4, 16, hd, T) for hd in (64, 72) for T in (16, 64, 128, 256, 1024)}
    assert before == {(64, 16): 1, (72, 16): 1, (64, 64): 2, (72, 64): 2, (64, 128): 2, (72, 128): 2, (64, 256): 5, (72, 256): 2, (64, 1024): 4, (72, 1024): 4}
    try:
        hip.set_option(hip.OPT_ATTENTION_TILED, 0)
        for hd in (64, 72):
            for T in NEW_TOKENS:
                assert plan(4, 16, hd, T) == -1
        assert {(hd, T): plan(4, 16, hd, T) for hd, T in before} == before
        hip.set_option(hip.OPT_ATTENTION_TILED, 2)
        for hd in (64, 72):
            for T in (16, 64, 128, 256, 1024, 32, 512, 160, 4080) + NEW_TOKENS:
                assert plan(4, 16, hd, T) == 7, (hd, T)
            for T in (0, 8, 24, 4096, 4112):
                assert plan(4, 16, hd, T) == -1, (hd, T)
        assert plan(4, 16, 80, 256) == -1
    finally:
        hip.set_option(hip.OPT_ATTENTION_TILED, 1)
    assert {(hd, T): plan(4, 16, hd, T) for hd, T in before} == before  # restored: every shape is back on its own kernel
    assert plan(64, 16, 64, 256) == 6
    L = hip.lib()
    for value in (0, 1, 2, 1):
        assert L.lfm_set_option(hip.OPT_ATTENTION_TILED, value) == 0
    assert L.lfm_set_option(hip.OPT_ATTENTION_TILED, 3) < 0 and L.lfm_set_option(hip.OPT_ATTENTION_TILED, -1) < 0
    assert plan(4, 16, 64, 576) == 7  # a refused value changes nothing


def test_dit_constructs_at_the_new_grids():
    """Refused before the tiled kernel: DiT-S/2 at resolution 24 (144 tokens) and 48 (576), DiT-XL/2 at 24; a 10 x 10 grid (no multiple of 4) still is."""
    from lfm_amd import hip
    from lfm_amd.models import DiT, DiT_models

    kw = dict(in_channels=4, num_classes=1, label_dropout=0.0)
    for name, res in (("DiT-S/2", 24), ("DiT-S/2", 48), ("DiT-XL/2", 24)):
        m = DiT_models[name](img_resolution=res, **kw)
        assert m.pos_embed.shape[1] == (res // 2) ** 2
        assert hip.lib().lfm_dit_workspace_bytes(m.shape_struct(), 2) > 0  # check_shape agrees
    with pytest.raises(NotImplementedError, match="100 tokens"):
        DiT(img_resolution=20, patch_size=2, hidden_size=384, depth=2, num_heads=6, **kw)
    with pytest.raises(NotImplementedError):
        DiT_models["DiT-S/2"](img_resolution=128, **kw)  # 4096 tokens


def test_dit_ref_matches_reference_at_grid_12(golden_dir):
    """oracle/dit_ref.py against the unmodified reference at 144 tokens (tests/golden/dit_grid12.pt, tools/make_golden_dit_grid12.py), at the tolerance
    tests/test_oracle_golden.py uses for the other DiT goldens."""
    rec = torch.load(os.path.join(golden_dir, "dit_grid12.pt"), map_location="cpu", weights_only=False)
    assert os.path.getsize(os.path.join(golden_dir, "dit_grid12.pt")) < os.path.getsize(os.path.join(golden_dir, "dit_hd72.pt"))  # data only, no weights
    cfg = dit_ref.DiTCfg(**rec["cfg"])
    assert cfg.tokens == 144
    sd = dit_ref.make_dit_state(cfg, seed=rec["state_seed"])
    assert abs(float(sum(v.double().abs().sum() for v in sd.values())) - rec["state_checksum"]) < 1e-6 * rec["state_checksum"]
    assert float(rec["v_tN"].abs().mean()) > 1e-3  # not comparing 0 with 0
    torch.testing.assert_close(dit_ref.dit_forward(sd, cfg, rec["t0"], rec["x"]), rec["v_t0d"], rtol=1e-5, atol=1e-6)
    torch.testing.assert_close(dit_ref.dit_forward(sd, cfg, rec["tN"], rec["x"], rec["y"]), rec["v_tN"], rtol=1e-5, atol=1e-6)
    v = dit_ref.dit_forward_with_cfg(sd, cfg, rec["t0"], rec["x_cfg"], rec["y_cfg"], rec["cfg_scale"])
    torch.testing.assert_close(v, rec["v_cfg"], rtol=1e-5, atol=1e-6)
