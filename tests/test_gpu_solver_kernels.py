"""The solver kernels (csrc/solver_kernels.h) against float64: lincomb_kernel, rk_err_partial_kernel + rk_err_finish_kernel, grid_advance_kernel, and
the alignment refusals of lfm_lincomb / lfm_rk_error_norm.  The GPU tests are marked one by one: the bound the error-norm test relies on is first
confirmed WITHOUT a GPU on an fp32 emulation of the two kernels in their own order (test_rk_bound_holds_for_the_emulated_kernels)."""
import math

import pytest
import torch

from lfm_amd.solvers import _DP_E

U = 2.0 ** -24  # fp32 unit roundoff
RK_BLOCKS = 1024


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available(), "needs an MI355X"
    return torch.device("cuda:0")


# ----------------------------------------------------------------------------- lincomb
def lincomb_case(nk, n, seed):
    g = torch.Generator().manual_seed(seed)
    ks = [torch.randn(n, generator=g) for _ in range(nk)]
    coef = torch.randn(max(nk, 1), generator=g)
    if nk >= 2:  # a zero coefficient in the middle: the kernel skips it, so its k (all NaN) must never be read into the sum
        coef[nk // 2] = 0.0
        ks[nk // 2].fill_(float("nan"))
    return ks, coef, torch.randn(n, generator=g), torch.tensor([-0.37])


def lincomb_ref(ks, coef, base, scale):
    """float64 (value, sum of the magnitudes the roundings are relative to)."""
    n = base.numel()
    acc, mag = torch.zeros(n, dtype=torch.float64), torch.zeros(n, dtype=torch.float64)
    for c, k in zip(coef.double()[:len(ks)], ks):
        if float(c) != 0.0:
            acc += c * k.double()
            mag += (c * k.double()).abs()
    return acc, mag


@pytest.mark.gpu
@pytest.mark.parametrize("nk", [0, 1, 2, 7, 8])
def test_lincomb(dev, nk):
    """out = base + scale * sum c_j k_j.  The kernel rounds once per accumulated term (fused multiply-add; twice where the compiler does not fuse),
    once for the scale and once for the base: nk + 2 roundings, each relative to at most |scale| sum |c_j k_j| + |base|.  Allowed: 2 (nk + 2) ulps
    of that, elementwise."""
    from lfm_amd import hip

    for n in (4, 4 * 255, 4 * 256, 4 * 257, 4 * (256 * 40 + 1)):
        ks, coef, base, scale = lincomb_case(nk, n, seed=nk * 100003 + n)
        acc, mag = lincomb_ref(ks, coef, base, scale)
        kd, cd = [k.to(dev) for k in ks], coef.to(dev)
        for use_scale in (False, True):
            s = float(scale) if use_scale else 1.0
            for mode in ("none", "given", "is_out"):
                want = acc * s + (base.double() if mode != "none" else 0.0)
                bound = 2 * (nk + 2) * U * (mag * abs(s) + (base.double().abs() if mode != "none" else 0.0))
                bd = base.to(dev) if mode != "none" else None
                out = bd if mode == "is_out" else torch.full((n,), float("nan"), device=dev)
                hip.lincomb(out, bd, kd, cd, scale.to(dev) if use_scale else None)
                got = out.cpu().double()
                assert bool(torch.isfinite(got).all()), (n, use_scale, mode)
                excess = float(((got - want).abs() - bound).max())
                assert excess <= 0.0, (n, use_scale, mode, excess)
                if mode == "given":
                    assert torch.equal(bd.cpu(), base)


# ----------------------------------------------------------------------------- rk_error_norm
def rk_case(nk, n, seed):
    g = torch.Generator().manual_seed(seed)
    y0, y1 = torch.randn(n, generator=g), torch.randn(n, generator=g)  # mixed signs
    y0[::7] = 0.0
    y1[::21] = 0.0  # every 21st element has both exactly zero: the denominator is atol alone
    ks = [torch.randn(n, generator=g) for _ in range(nk)]
    coef = torch.tensor(_DP_E if nk == 7 else (0.75,), dtype=torch.float32)
    return y0, y1, ks, coef, torch.tensor([0.05])


def rk_ref(y0, y1, ks, coef, dt, rtol, atol):
    """float64 (value, relative bound).  Per element e = sum c_j k_j takes at most 2 nk roundings relative to E = sum |c_j k_j|; dt e, the denominator
    (two roundings on positive terms) and the division four more: |dr| <= (2 nk + 4) u R with R = dt E / den >= |r|, so the square moves by at most
    (4 nk + 9) u |r| R.  The squares are non-negative and are added in a tree: three adds per 16-byte step of a thread (at most three steps here), six
    across the wave, two across the block, then up to four per thread, six and two again in the finishing block: S = 3 steps + 20 roundings.  One for
    1 / n, and the square root halves the relative error and rounds once:  bound = ((4 nk + 9) sum |r| R / sum r^2 + S + 1) u / 2 + u.
    This is a WORST-CASE bound (every rounding in the same direction): the emulation below sits at 1e-8 .. 8e-8 against bounds of 1.2e-6 .. 2.5e-6.  It
    catches a dropped grid-stride tail (1 / 3 of the sum at the largest size), a wrong block count, an fp16-rounded operand or a wrong denominator, and
    would not catch a mistake of a few tens of ulps."""
    c = coef.double()
    e = sum(c[j] * ks[j].double() for j in range(len(ks)))
    E = sum((c[j] * ks[j].double()).abs() for j in range(len(ks)))
    den = float(torch.tensor(atol, dtype=torch.float32)) + float(torch.tensor(rtol, dtype=torch.float32)) * torch.maximum(y0.double().abs(), y1.double().abs())
    h = float(dt)
    r, R = h * e / den, abs(h) * E / den
    n = y0.numel()
    steps = -(-(n // 4) // (256 * min(-(-(n // 4) // 256), RK_BLOCKS)))
    S = 3 * steps + 20
    bound = ((4 * len(ks) + 9) * float((r.abs() * R).sum() / (r * r).sum()) + S + 1) * U / 2 + U
    return math.sqrt(float((r * r).mean())), bound


def rk_emulate(y0, y1, ks, coef, dt, rtol, atol):
    """The two kernels in fp32 in their own order: grid-stride steps per thread, xor-butterfly per wave, (0 + 1) + (2 + 3) per block; the finishing block the same."""
    n4 = y0.numel() // 4
    nb = min(-(-n4 // 256), RK_BLOCKS)
    e = torch.zeros_like(y0)
    for j, k in enumerate(ks):
        if float(coef[j]) != 0.0:
            e = e + coef[j] * k
    r = dt * e / (torch.tensor(atol) + torch.tensor(rtol) * torch.maximum(y0.abs(), y1.abs()))
    r2 = (r * r).reshape(n4, 4)
    q = (r2[:, 0] + r2[:, 1]) + (r2[:, 2] + r2[:, 3])

    def block_sums(v, blocks):  # v [steps, blocks * 256] -> [blocks]
        acc = torch.zeros(blocks * 256)
        for s in range(v.shape[0]):
            acc = acc + v[s]
        acc = acc.reshape(blocks, 4, 64)
        w = 32
        while w:
            acc = acc[..., :w] + acc[..., w:2 * w]
            w //= 2
        acc = acc[..., 0]
        return (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])

    steps = -(-n4 // (nb * 256))
    part = block_sums(torch.cat([q, torch.zeros(steps * nb * 256 - n4)]).reshape(steps, nb * 256), nb)
    fsteps = -(-nb // 256)
    total = block_sums(torch.cat([part, torch.zeros(fsteps * 256 - nb)]).reshape(fsteps, 256), 1)
    return float(torch.sqrt(total * torch.tensor(1.0 / y0.numel(), dtype=torch.float32)))


RK_SIZES = (4, 4 * 63, 4 * 256, 4 * 257, 4 * 256 * 1024, 4 * (256 * 1024 * 2 + 300))  # one thread .. RK_BLOCKS full blocks .. the grid-stride loop
RK_TOLS = ((1e-5, 1e-5), (1e-3, 1e-6))  # as the samplers use them; a looser pair


@pytest.mark.parametrize("n", (4, 4 * 257, 4 * 256 * 1024 + 4 * 300))
def test_rk_bound_holds_for_the_emulated_kernels(n):
    for nk in (7, 1):
        case = rk_case(nk, n, seed=nk * 7 + n)
        for rtol, atol in RK_TOLS:
            ref, bound = rk_ref(*case, rtol, atol)
            got = rk_emulate(*case, rtol, atol)
            print(f"rk emulation n={n} nk={nk} rtol={rtol:g}: value {ref:.6e}, |rel error| {abs(got - ref) / ref:.2e}, bound {bound:.2e}")
            assert abs(got - ref) <= bound * ref


@pytest.mark.gpu
@pytest.mark.parametrize("n", RK_SIZES)
def test_rk_error_norm(dev, n):
    """Against float64 within 4x the written bound (rk_ref); two calls give the same bits."""
    from lfm_amd import hip

    for nk in (7, 1):
        y0, y1, ks, coef, dt = rk_case(nk, n, seed=nk * 7 + n)
        d = [t.to(dev) for t in (y0, y1, *ks, coef, dt)]
        scratch = torch.zeros(RK_BLOCKS, device=dev)
        for rtol, atol in RK_TOLS:
            ref, bound = rk_ref(y0, y1, ks, coef, dt, rtol, atol)
            outs = [torch.full((1,), float("nan"), device=dev) for _ in range(2)]
            for o in outs:
                hip.rk_error_norm(d[0], d[1], d[2:2 + nk], d[2 + nk], d[3 + nk], rtol, atol, scratch, o)
            a, b = float(outs[0]), float(outs[1])
            print(f"rk_error_norm n={n} nk={nk} rtol={rtol:g}: {a:.6e} vs {ref:.6e}, |rel error| {abs(a - ref) / ref:.2e}, bound {bound:.2e}")
            assert outs[0].cpu().view(torch.int32).item() == outs[1].cpu().view(torch.int32).item(), (a, b)
            assert abs(a - ref) <= 4 * bound * ref, (a, ref, bound)


# ----------------------------------------------------------------------------- grid_advance
@pytest.mark.gpu
def test_grid_advance(dev):
    """After k launches on a grid of five times: step == k and t_cur, t_next, dt_cur are interval k - 1's.  Four intervals, four launches: never past the end."""
    from lfm_amd import hip

    ts = torch.tensor([1.0, 0.8, 0.45, 0.1, 0.0])
    dts = ts[1:] - ts[:-1]
    tsd, dtsd = ts.to(dev), dts.to(dev)
    step = torch.zeros(1, dtype=torch.int32, device=dev)
    cur, nxt, dt = (torch.full((1,), float("nan"), device=dev) for _ in range(3))
    for k in range(1, 5):
        hip.check(hip.lib().lfm_grid_advance(hip.ptr(tsd), hip.ptr(dtsd), hip.ptr(step), hip.ptr(cur), hip.ptr(nxt), hip.ptr(dt), hip.stream_ptr(dev)),
                  "lfm_grid_advance")
        assert int(step) == k
        assert (float(cur), float(nxt), float(dt)) == (float(ts[k - 1]), float(ts[k]), float(dts[k - 1]))
    assert torch.equal(tsd.cpu(), ts) and torch.equal(dtsd.cpu(), dts)


# ----------------------------------------------------------------------------- alignment refusals
@pytest.mark.gpu
def test_misaligned_operands_are_refused(dev):
    """base and every k are read 16 bytes at a time: a tensor offset by one float is refused with LFM_ERR_ALIGN before anything is launched (out stays as
    it was)."""
    from lfm_amd import hip

    n = 1024
    buf = torch.zeros(n + 4, device=dev)
    off = buf[1:n + 1]
    assert off.data_ptr() % 16 == 4
    good = [torch.ones(n, device=dev) for _ in range(3)]
    coef = torch.ones(3, device=dev)
    out = torch.full((n,), 5.0, device=dev)
    for ks, base in (([off], None), ([good[0], good[1], off], None), ([good[0]], off), ([], off)):
        with pytest.raises(hip.LfmHipError, match="alignment"):
            hip.lincomb(out, base, ks, coef)
    dt, scratch, res = torch.ones(1, device=dev), torch.zeros(RK_BLOCKS, device=dev), torch.full((1,), 5.0, device=dev)
    for ks in ([off], [good[0], off, good[1]]):
        with pytest.raises(hip.LfmHipError, match="alignment"):
            hip.rk_error_norm(good[0], good[1], ks, coef, dt, 1e-5, 1e-5, scratch, res)
    torch.cuda.synchronize()
    assert bool((out == 5.0).all()) and float(res) == 5.0
