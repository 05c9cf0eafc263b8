"""Without a GPU: the yardstick of tests/test_gpu_unet_attention_stream.py is sound, and lfm_unet_attention_plan answers what the dispatch rules say.

  * the fp16-staged online-softmax emulation of a CORRECT streamed kernel (tests/unet_attention_cases.py: emulate) stays within 4e-4 of float64 per
    (image, head) item on every input family -- the GPU tests' tolerance of 2e-3 leaves a factor of five;
  * each mistake a streamed kernel can make (a key dropped, padding not masked, the next item's key read, a block-local maximum, O or the sum not
    rescaled) exceeds 2e-3 on at least one family at every shape: the families can see it;
  * the truth table of the chooser under the defaults, LFM_OPT_UNET_ATTENTION_STREAM = 0 / 2 and flag UNET_ATT_VALU.
"""
import math

import pytest

import unet_attention_cases as uc

SHAPES = [(2, 2, 64, 333), (2, 2, 256, 130), (2, 3, 48, 577)]  # (N, heads, ch, T): ragged last key blocks; 48 channels = a zero-filled half k-step
EMULATION_BOUND = 4e-4


@pytest.mark.parametrize("N,heads,ch,T", SHAPES)
def test_emulated_correct_kernel_is_well_inside_the_tolerance(N, heads, ch, T):
    for family in uc.FAMILIES:
        qkv, ref = uc.case(family, N, heads, ch, T)
        err = uc.worst(uc.emulate(qkv, heads, ch), ref)
        print(f"emulation {family} N={N} heads={heads} ch={ch} T={T}: {err:.3e}")
        assert err <= EMULATION_BOUND, (family, err)


@pytest.mark.parametrize("N,heads,ch,T", SHAPES)
def test_every_emulated_mistake_is_visible_on_some_family(N, heads, ch, T):
    for mistake in uc.MISTAKES:
        errs = {}
        for family in uc.FAMILIES:
            qkv, ref = uc.case(family, N, heads, ch, T)
            errs[family] = uc.worst(uc.emulate(qkv, heads, ch, mistake=mistake), ref)
        print(f"{mistake} N={N} heads={heads} ch={ch} T={T}: " + ", ".join(f"{f} {e:.2e}" for f, e in errs.items()))
        assert any(math.isnan(e) or e > uc.TOL for e in errs.values()), (mistake, errs)


ERR = -1  # LFM_ERR_SHAPE
# (T, ch) -> lfm_unet_attention_plan under the defaults.  Written from the rules, not from the C++: the four resident shapes; else the VALU kernel while
# min(T, 64) (T + 1) 4 + 4 T (ch + 2) <= 160 KiB; else the streamed kernel for ch % 16 == 0, ch <= 256.
_PLAN_DEFAULT = {
    (64, 64): 2, (256, 64): 2, (64, 128): 2, (256, 128): 2,
    (64, 96): 1, (64, 192): 1, (16, 64): 1, (314, 64): 1, (127, 256): 1, (64, 20): 1,
    (315, 64): 3, (128, 256): 3, (1024, 64): 3, (4096, 64): 3, (1024, 16): 3, (576, 48): 3,
    (1024, 72): ERR, (2000, 8): ERR, (1024, 264): ERR,
}


def test_unet_attention_plan_truth_table():
    from lfm_amd import hip

    def plans():
        return {(T, ch): hip.unet_attention_plan(2, T, 4, ch) for (T, ch) in _PLAN_DEFAULT}

    assert hip.OPT_UNET_ATTENTION_STREAM == 7
    try:
        assert plans() == _PLAN_DEFAULT
        for value in (0, 1, 2):
            hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, value)  # key 7 accepts 0 / 1 / 2
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 0)  # the streamed kernel is never chosen, nothing else changes
        assert plans() == {s: (ERR if k == 3 else k) for s, k in _PLAN_DEFAULT.items()}
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 2)  # every shape the streamed kernel takes
        assert [hip.unet_attention_plan(2, T, 4, ch) for T, ch in ((64, 64), (64, 96), (16, 64), (64, 20))] == [3, 3, 3, 1]
        assert plans() == {(T, ch): (3 if ch % 16 == 0 and ch <= 256 else k) for (T, ch), k in _PLAN_DEFAULT.items()}
        for value in (0, 1, 2):  # flag UNET_ATT_VALU decides first: the VALU kernel or a refusal
            hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, value)
            hip.gemm_select(hip.DBG_UNET_ATT_VALU << 4)
            assert [hip.unet_attention_plan(2, T, 4, ch) for T, ch in ((256, 128), (1024, 64), (64, 64))] == [ERR, ERR, 1], value
            hip.gemm_select(0)
    finally:
        hip.gemm_select(0)
        hip.set_option(hip.OPT_UNET_ATTENTION_STREAM, 1)
    assert plans() == _PLAN_DEFAULT
    assert hip.unet_attention_plan(0, 64, 4, 64) == ERR and hip.unet_attention_plan(2, 0, 4, 64) == ERR  # as lfm_attention_small_f16 refuses them
    assert hip.unet_attention_plan(2, 64, 0, 64) == ERR and hip.unet_attention_plan(2, 64, 4, 0) == ERR
