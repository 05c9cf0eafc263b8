"""Constructed inputs and two float64 references for the VAE mid-block attention (TEST INFRASTRUCTURE ONLY).

The operation (diffusers ``Attention`` with one head of C = 512 channels, as ``oracle.vae_ref.mid_attention`` restates it) on NHWC tokens:
    h = GroupNorm32(x) gamma + beta;  q, k, v = h W^T + b;  P = softmax(q k^T C^-0.5);  out = x + (P v) W_o^T + b_o
``make_vae_state`` weights put the softmax in a regime (logit sd ~1, row maximum of P ~0.05) in which a missing max subtraction, a partial max or
fp16 scores cannot be seen.  ``make_case`` builds families of inputs that leave it; ``exact`` is float64 throughout; ``staged`` is the same float64
arithmetic rounded where the device stores a tensor, so ``e_stage`` = |staged - exact| / |exact - x| is the error a correct implementation of that
staging has.  ``check`` accepts a result whose branch error is at most ``MARGIN`` x e_stage.
"""
import torch
import torch.nn.functional as F

C = 512
GROUPS = 32
EPS = 1e-6
FAMILIES = ("diffuse", "peaked", "self_match", "planted", "offset_pos", "offset_neg")
# The device rounds at the points `staged` rounds at and differs from it only by fp32 accumulation order and the hardware exp2, both > 100 x below an
# fp16 rounding: its error is another draw of the size of e_stage, and 2 covers the spread of two draws.
MARGIN = 2.0
# The seed of the tests.  Chosen on the INPUTS alone: at T = 64 three spiky tokens of 64 raise their own GroupNorm variance, the planted logits have a
# standard deviation of ~14, and of seeds 0 .. 7 only some reach the > 25 the family promises (3: 41 / 51 / 56 at T = 64 / 576 / 1024).
SEED = 3


def planted_tokens(T):
    """The first, a middle and the last key, in different 64-key strides of a softmax row."""
    return (0, T // 2 + 7, T - 1)


def make_case(family, n, T, seed=SEED):
    """fp16 x [n, T, C], fp32 gamma / beta [C], fp16 q_w / k_w / v_w / o_w [C, C] ([out][in]), fp32 q_b / k_b / v_b / o_b [C]."""
    fam = FAMILIES.index(family)
    g = torch.Generator().manual_seed(((int(seed) * 8 + fam) * 64 + int(n)) * 65536 + int(T))

    def rn(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    x = rn(n, T, C)
    gamma, beta = 1 + 0.2 * rn(C), 0.3 * rn(C)
    g2 = 8.0 if family in ("peaked", "self_match") else 1.0
    q_w, k_w = rn(C, C) * (g2 / C) ** 0.5, rn(C, C) * (g2 / C) ** 0.5
    v_w, o_w = rn(C, C) * C ** -0.5, rn(C, C) * C ** -0.5
    q_b, k_b, v_b, o_b = (0.1 * rn(C) for _ in range(4))
    b = 3 * rn(C)
    if family == "self_match":
        k_w = q_w.clone()
    elif family == "planted":
        x[:, list(planted_tokens(T))] *= 6
    elif family == "offset_pos":
        q_b, k_b = b, b.clone()
    elif family == "offset_neg":
        q_b, k_b = b, -b
    case = {"family": family, "n": n, "T": T, "seed": seed, "x": x.half()}
    for name, t in (("gamma", gamma), ("beta", beta), ("q_b", q_b), ("k_b", k_b), ("v_b", v_b), ("o_b", o_b)):
        case[name] = t.float()
    for name, t in (("q_w", q_w), ("k_w", k_w), ("v_w", v_w), ("o_w", o_w)):
        case[name] = t.half()
    return case


def _same(t):
    return t


def _f16(t):
    return t.half().double()


def _f32(t):
    return t.float().double()


def _softmax(s_scaled):
    return s_scaled.softmax(dim=-1)


@torch.no_grad()
def _forward(case, r16, r32, softmax=_softmax, on_s=_same, on_v=_same):
    """The operation in float64 with r16 / r32 applied where the device stores fp16 / fp32.  softmax / on_s / on_v: hooks for tests that emulate a
    faulty implementation (softmax maps SCALED logits to P; on_s sees the unscaled stored scores, on_v the stored V)."""
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.items()}
    x = d["x"]
    h = r16(F.group_norm(x.transpose(1, 2), GROUPS, d["gamma"], d["beta"], eps=EPS).transpose(1, 2))
    q = r16(h @ d["q_w"].T + d["q_b"])
    k = r16(h @ d["k_w"].T + d["k_b"])
    v = on_v(r16(h @ d["v_w"].T + d["v_b"]))
    s = on_s(r32(q @ k.transpose(1, 2)))
    p = r16(softmax(s * C ** -0.5))
    o = r16(p @ v)
    out = r16(o @ d["o_w"].T + d["o_b"] + x)
    return out, out - x


def exact(case):
    """(out, out - x) in float64 throughout."""
    return _forward(case, _same, _same)


def staged(case, **hooks):
    """(out, out - x): float64 arithmetic; GroupNorm output, Q, K, V, P, O and the final sum rounded to fp16, S to fp32 -- the device's stores."""
    return _forward(case, _f16, _f32, **hooks)


@torch.no_grad()
def logit_stats(case):
    """Of the exact scaled logits: their minimum, maximum and standard deviation, and the mean over rows of the row maximum of P."""
    d = {k: (v.double() if torch.is_tensor(v) else v) for k, v in case.items()}
    h = F.group_norm(d["x"].transpose(1, 2), GROUPS, d["gamma"], d["beta"], eps=EPS).transpose(1, 2)
    s = (h @ d["q_w"].T + d["q_b"]) @ (h @ d["k_w"].T + d["k_b"]).transpose(1, 2) * C ** -0.5
    return {"min": float(s.min()), "max": float(s.max()), "sd": float(s.std()), "pmax_mean": float(s.softmax(dim=-1).amax(dim=-1).mean())}


def references(case):
    """exact and staged of a case, computed once and kept on it (read-only)."""
    if "_refs" not in case:
        case["_refs"] = (exact(case), staged(case))
    return case["_refs"]


def e_stage(case, image=None):
    """|staged - exact| / |exact - x|: the error, on the attention branch, of the device's staging done correctly.  image: of that image alone."""
    (ex, ex_br), (st, _) = references(case)
    sl = slice(None) if image is None else slice(image, image + 1)
    return float((st[sl] - ex[sl]).norm() / ex_br[sl].norm())


def branch_error(got, case, image=None):
    """|(got - x) - (exact - x)| / |exact - x| of a result got [n, T, C] (any float type, any device)."""
    (ex, ex_br), _ = references(case)
    sl = slice(None) if image is None else slice(image, image + 1)
    return float((got.detach().cpu().double()[sl] - ex[sl]).norm() / ex_br[sl].norm())


def check(got, case, image=None):
    """A result passes when it is finite and its branch error is <= MARGIN x e_stage, both measured against `exact` (of the whole batch, or of one
    image).  Returns (passed, error / e_stage, e_stage)."""
    es = e_stage(case, image)
    if not bool(torch.isfinite(got).all()):
        return False, float("inf"), es
    err = branch_error(got, case, image)
    return err <= MARGIN * es, err / es, es
