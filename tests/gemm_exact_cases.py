"""Shared pieces of the exact GEMM / conv3x3 tests (tests/test_gemm_exact_ref.py on the CPU, tests/test_gpu_gemm_exact.py on the GPU): integer operand
builders, the float64 / int64 references, the strided and guarded buffer layouts, and the element-by-element checker.

Not a test module.

Why integers: fp16 operands that hold small integers give products and partial sums that are exact in fp32 in ANY summation order as long as
sum_k |a_k w_k| < 2^24, and the result is exactly representable in the output type (fp32, or fp16 while |value| <= 2048).  Every kernel, tile order,
split-K slicing and store width must then return the same bits as the integer product: the check is equality per element, with no tolerance.  The two caps
are CONDITIONS of that argument, not measurements: every builder below asserts them for the case it builds."""
import functools
import math
from types import SimpleNamespace

import torch

GUARD = 8  # rows after the last row of every operand (NaN) and of every output (sentinel)
SENTINEL = -1234.0  # exactly representable in fp16 and fp32; outside every output range of the fp16 cases, and never produced where it is looked for
CAP16 = 2048  # |integer| <= 2048 is exact in fp16
CAP32 = 1 << 24  # |integer| < 2^24 is exact in fp32
NAN = float("nan")

# operand ranges (inclusive): fp16-out epilogues / fp32-out epilogues.  The fp32 range is chosen to EXCEED 2048: a kernel that handed an accumulator through
# the LDS in fp16 then fails exactly.
R16 = dict(a=2, w=1, bias=8, resid=64)
R32 = dict(a=8, w=8, bias=64, gate=4, x=1000)

# name -> (lda - K, ldw - K, ldc - N).  narrow: ldc % 8 == 4 takes the 8-byte-store path of the fp16 epilogues (wide_ok() false) through a real ldc.
LAYOUTS = {"dense": (0, 0, 0), "wide": (8, 8, 8), "narrow": (8, 8, 4)}

# output tile of each kernel (rows, columns), for the failure message: lfm_gemm_select ids; 7 / 8 = the latency-mode kernels
TILES = {1: (128, 128), 4: (256, 128), 5: (256, 256), 6: (256, 256), 7: (64, 64), 8: (256, 16)}


def randint(g, shape, r):
    return torch.randint(-r, r + 1, shape, generator=g, dtype=torch.int64)


def exact_mm(a, w):
    """a [M, K] x w [N, K]^T of int64 operands as int64.  Computed in float64, which is exact here (every partial sum is an integer below 2^53 in any
    order) and runs on the BLAS; an int64 matmul gives the same integers and takes minutes at the split-K shapes."""
    assert float(a.abs().max()) * float(w.abs().max()) * a.shape[1] < 2.0 ** 53
    return (a.double() @ w.double().t()).round().to(torch.int64)


def abs_mm(a, w):
    """sum_k |a_k w_k| per output element: the bound on every partial sum in every order."""
    return exact_mm(a.abs(), w.abs())


# ------------------------------------------------------------------------------------------------ layouts
def embed(t, ld=None, fill=NAN, guard=GUARD, dtype=None):
    """t [rows, cols] inside a [rows + guard, ld] buffer of `fill` (NaN for operands: a pad column or a guard row that enters a product poisons it; the
    sentinel for outputs).  Returns the buffer; the tensor is buf[:rows, :cols], its leading dimension ld."""
    t = t if t.dim() == 2 else t.reshape(1, -1)
    rows, cols = t.shape
    ld = cols if ld is None else ld
    buf = torch.full((rows + guard, ld), fill, dtype=dtype or t.dtype)
    buf[:rows, :cols] = t.to(buf.dtype)
    return buf


def embed_vec(v, fill=NAN, dtype=torch.float32):
    """A bias-like row with GUARD NaN elements past its end."""
    buf = torch.full((v.numel() + GUARD,), fill, dtype=dtype)
    buf[:v.numel()] = v.to(dtype)
    return buf


def out_buffer(M, N, ldc, dtype, init=None):
    """The [M + GUARD, ldc] output buffer pre-filled with the sentinel; `init` (epilogue 3: the residual stream X) fills [0, M) x [0, N)."""
    buf = torch.full((M + GUARD, ldc), SENTINEL, dtype=dtype)
    if init is not None:
        buf[:M, :N] = init.to(dtype)
    return buf


# ------------------------------------------------------------------------------------------------ the checker
def diff_positions(got, ref):
    """The (m, n) positions where got [M, N] (any float type) differs from ref (int64 or float64); a NaN differs."""
    return (got.double() != ref.double()).nonzero().tolist()


def touched_positions(buf, M, N):
    """The positions of buf [M + GUARD, ldc] outside [0, M) x [0, N) that no longer hold the sentinel."""
    bad = buf != SENTINEL
    bad[:M, :N] = False
    return bad.nonzero().tolist()


def check(buf, ref, M, N, kernel=None):
    """One output buffer against its reference: SimpleNamespace(diffs, touched, message).  diffs: differing (m, n); touched: pad / guard positions written."""
    buf = buf.detach().cpu()
    diffs, touched = diff_positions(buf[:M, :N], ref), touched_positions(buf, M, N)
    msg = []
    if diffs:
        tile = TILES.get(kernel)
        first = []
        for m, n in diffs[:6]:
            where = f" tile ({m // tile[0]}, {n // tile[1]}) of kernel {kernel}" if tile else ""
            first.append(f"({m}, {n}){where}: got {float(buf[m, n])!r}, expected {float(ref[m, n])!r}")
        msg.append(f"{len(diffs)} of {M * N} elements differ; first: " + "; ".join(first))
    if touched:
        kinds = sorted({"guard row" if m >= M else "pad column" for m, n in touched})
        msg.append(f"{len(touched)} elements outside [0, {M}) x [0, {N}) written ({', '.join(kinds)}); first: " +
                   ", ".join(f"({m}, {n}) = {float(buf[m, n])!r}" for m, n in touched[:6]))
    else:
        msg.append("pad columns and guard rows untouched")
    return SimpleNamespace(diffs=diffs, touched=touched, message="; ".join(msg))


def assert_exact(buf, ref, M, N, what, kernel=None):
    r = check(buf, ref, M, N, kernel)
    assert not r.diffs and not r.touched, f"{what}: {r.message}"


# ------------------------------------------------------------------------------------------------ lfm_gemm_f16
# epilogue variants: (epilogue id, shared gate row)
EPILOGUES = [(0, False), (2, False), (3, False), (3, True)]
TOKENS = 4
# remap off: 9 / 6 / 4 tiles of kernels 1 / 4 / 5, 6; remap on (tile count % 8 == 0): 24 / 16 / 8.  Both ragged in rows and columns, interior tiles in both.
GEMM_SHAPES = [(300, 260), (300, 1000)]
# K-tile counts 1, 2, 3, 5, 16 (kernels 1, 5, 6: 64 deep; kernel 4: 32 deep, so 1, 3, 5, 10, 32): every prologue / steady / tail path of each K loop
GEMM_KS = {1: (64, 128, 192, 320, 1024), 4: (32, 96, 160, 320, 1024), 5: (64, 128, 192, 320, 576, 1024), 6: (64, 128, 192, 320, 576, 1024),
           0: (64, 320, 1024)}  # 0 = the automatic choice (the 128x128 kernel at these sizes)


def gemm_f16_cases():
    return [(kernel, M, N, K) for kernel in (1, 4, 5, 6, 0) for (M, N) in GEMM_SHAPES for K in GEMM_KS[kernel]]


@functools.lru_cache(maxsize=None)
def _int_operands(M, N, K, ra, rw, rb, seed):
    g = torch.Generator().manual_seed(seed)
    A, W, bias = randint(g, (M, K), ra), randint(g, (N, K), rw), randint(g, (N,), rb)
    return A, W, bias, exact_mm(A, W), abs_mm(A, W)


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, epi, shared_gate=False):
    """Integer operands and the int64 reference of lfm_gemm_f16 with epilogue 0 (fp16 out), 2 (fp32 out) or 3 (fp32 X += gate * (acc + bias))."""
    r = R16 if epi == 0 else R32
    A, W, bias, acc, mag = _int_operands(M, N, K, r["a"], r["w"], r["bias"], 1000 * epi + M + 3 * N + K)
    c = SimpleNamespace(M=M, N=N, K=K, epi=epi, A=A, W=W, bias=bias, X=None, gate=None, tokens=TOKENS, out_dtype=torch.float16 if epi == 0 else torch.float32)
    ref = acc + bias
    assert int(mag.max()) < CAP32 and int((mag + bias.abs()).max()) < CAP32
    if epi == 3:
        assert M % TOKENS == 0
        g = torch.Generator().manual_seed(7 + M + N + K)
        c.X = randint(g, (M, N), R32["x"])
        c.gate = randint(g, (1 if shared_gate else M // TOKENS, N), R32["gate"])
        prod = (c.gate if shared_gate else c.gate.repeat_interleave(TOKENS, 0)) * ref
        assert int(prod.abs().max()) < CAP32
        ref = c.X + prod
    c.ref = ref
    assert int(ref.abs().max()) < (CAP32 if epi else CAP16 + 1), (M, N, K, epi, int(ref.abs().max()))
    return c


# ------------------------------------------------------------------------------------------------ the latency-mode kernels
# kernel 7 at 512 columns: eight column tiles, the XCD-grouped tile order (xcd_map) -- one and three column tiles take the plain order
LATENCY_SHAPES = {7: [(M, N) for M in (64, 192) for N in (64, 192)] + [(192, 512)], 8: [(M, N) for M in (200, 256) for N in (64, 176, 192)]}
LATENCY_KS = (64, 512, 576)  # one K-tile, one full turn of the eight-stage ring (kernel 7; two turns of kernel 8's four stages), one wrap


def latency_cases():
    return [(kernel, M, N, K) for kernel in (7, 8) for (M, N) in LATENCY_SHAPES[kernel] for K in LATENCY_KS]


# ------------------------------------------------------------------------------------------------ lfm_gemm_qkv_f16
QKV_SHAPES = [(3, 64, 384, 64), (3, 64, 576, 72)]  # (batch, tokens, D, head_dim)


@functools.lru_cache(maxsize=None)
def qkv_case(batch, tokens, D, hd):
    M = batch * tokens
    A, W, bias, acc, mag = _int_operands(M, 3 * D, D, R16["a"], R16["w"], R16["bias"], 31 + batch + tokens + D)
    ref = acc + bias
    assert int(ref.abs().max()) <= CAP16 and int(mag.max()) < CAP32
    vt = ref[:, 2 * D:].reshape(batch, tokens, D // hd, hd).permute(0, 2, 3, 1).contiguous()  # [image, head, d, token], plain token order
    return SimpleNamespace(M=M, D=D, K=D, hd=hd, tokens=tokens, batch=batch, A=A, W=W, bias=bias, q=ref[:, :D].contiguous(), k=ref[:, D:2 * D].contiguous(), vt=vt)


# ------------------------------------------------------------------------------------------------ lfm_linear*_f16
LINEAR_SHAPES = [(143, 132, 192), (16271, 260, 96)]  # the second: 64 x 3 tiles of 256 x 128, fewer than 192 tiles of 256 x 256: the chooser's kernel 4


@functools.lru_cache(maxsize=None)
def linear_case(M, N, K):
    """acc + bias + resid, fp16 out; scale 0.5 is exact too: a multiple of 1/2 of magnitude <= 1024 is an fp16 number."""
    A, W, bias, acc, mag = _int_operands(M, N, K, R16["a"], R16["w"], R16["bias"], 57 + M + N + K)
    resid = randint(torch.Generator().manual_seed(M + N), (M, N), R16["resid"])
    ref = acc + bias + resid
    assert int(ref.abs().max()) <= CAP16 and int((mag + bias.abs() + resid.abs()).max()) < CAP32
    return SimpleNamespace(M=M, N=N, K=K, A=A, W=W, bias=bias, resid=resid, ref=ref)


# ------------------------------------------------------------------------------------------------ lfm_conv3x3*_f16_ws
def conv_input_size(H, W, mode):
    """Input map of an OUTPUT size H x W: the same (mode 0), half (mode 1: nearest-2x upsample fused), double (modes 2, 3: stride 2)."""
    return {0: (H, W), 1: (H // 2, W // 2), 2: (2 * H, 2 * W), 3: (2 * H, 2 * W)}[mode]


def conv_cols(x, N, H, W, Cin, mode):
    """The im2col matrix [N H W, 9 Cin] (k = tap * Cin + ci, tap = ky * 3 + kx) of NHWC x (any dtype) for an OUTPUT size H x W.  Modes 0 - 2 pad by one
    pixel all round; mode 1: on the nearest-2x upsampled input; mode 2: stride 2 -- output (oy, ox) reads input (2 oy + ky - 1, 2 ox + kx - 1); mode 3:
    stride 2 on the input padded (0, 1, 0, 1) (diffusers Downsample2D) -- reads (2 oy + ky, 2 ox + kx), zero beyond the bottom row and the right column."""
    Hi, Wi = conv_input_size(H, W, mode)
    x = x.reshape(N, Hi, Wi, Cin)
    if mode == 1:
        x = x.repeat_interleave(2, 1).repeat_interleave(2, 2)
    xp = torch.nn.functional.pad(x, (0, 0, 0, 1, 0, 1) if mode == 3 else (0, 0, 1, 1, 1, 1))
    s = 2 if mode >= 2 else 1
    return torch.cat([xp[:, ky:ky + s * H:s, kx:kx + s * W:s, :] for ky in range(3) for kx in range(3)], -1).reshape(N * H * W, 9 * Cin)


def conv_ref(x, Wt, bias, resid, N, H, W, Cin, mode):
    """3x3 convolution of NHWC int64 x with Wt [Cout, 9 Cin] as an int64 im2col product (conv_cols: the modes) + bias + resid."""
    cols = conv_cols(x, N, H, W, Cin, mode)
    out = exact_mm(cols, Wt) + bias
    mag = abs_mm(cols, Wt) + bias.abs()
    if resid is not None:
        out, mag = out + resid, mag + resid.abs()
    return out, mag


# (path, N, H, W, Cin, Cout, modes): H x W the OUTPUT size, never square; mode 1 needs it even
CONV_CASES = [
    ("halo", 1, 16, 32, 64, 128, (0, 1)), ("halo", 2, 32, 16, 128, 256, (0, 1)),
    ("gemm", 1, 10, 14, 64, 132, (0, 1, 2)), ("gemm", 2, 16, 24, 128, 256, (0, 1, 2)),  # 140 rows x two ragged column tiles; 768 rows = three 256-row tiles
    ("splitk128", 1, 9, 7, 128, 132, (0, 2)), ("splitk128", 1, 10, 6, 128, 132, (1,)),  # K = 1152 in two slices of 576: the tap walk starts in mid-tap 4
    # slices on the 256x256 kernel: M >= 2048 rows, whole 256-column tiles, tiles x slices in [128, 256] with slices >= 24 K-tiles deep (splitk256_slices):
    # Cin = 384 is the narrowest input that allows two such slices (54 K-tiles), which then asks for 64 tiles = 2048 x 2048; slice 1 starts in mid-tap 4
    ("splitk256", 1, 32, 64, 384, 2048, (0, 1, 2)),
]


def splitk256_slices(M, N, K, slab_bytes, min_tiles_k=24):
    """csrc/gemm_kernel.h: splitk256_slices, restated (the flag LFM_DBG_GEMM_SPLITK128 aside)."""
    if M < 2048 or N < 256 or N % 256 or K % 64:
        return 0
    tiles = -(-M // 256) * (N // 256)
    if tiles > 128:
        return 0
    kt, best = K // 64, 0
    for sl in range(2, 17):
        if kt % sl == 0 and tiles * sl <= 256 and kt // sl >= min_tiles_k and sl * M * N * 4 <= slab_bytes:
            best = sl
    return best if tiles * best >= 128 else 0


@functools.lru_cache(maxsize=None)
def _conv_weights(Cin, Cout):
    g = torch.Generator().manual_seed(11 + Cin + Cout)
    return randint(g, (Cout, 9 * Cin), R16["w"]), randint(g, (Cout,), R16["bias"])


@functools.lru_cache(maxsize=None)
def conv_case(N, H, W, Cin, Cout, mode):
    Hi, Wi = conv_input_size(H, W, mode)
    g = torch.Generator().manual_seed(5 + N + 3 * H + 7 * W + Cin + Cout + mode)
    x = randint(g, (N * Hi * Wi, Cin), R16["a"])
    Wt, bias = _conv_weights(Cin, Cout)
    M = N * H * W
    resid = randint(g, (M, Cout), R16["resid"])
    ref, mag = conv_ref(x, Wt, bias, resid, N, H, W, Cin, mode)
    assert int(ref.abs().max()) <= CAP16 and int(mag.max()) < CAP32, (N, H, W, Cin, Cout, mode, int(ref.abs().max()))
    return SimpleNamespace(N=N, H=H, W=W, Cin=Cin, Cout=Cout, mode=mode, M=M, x=x, Wt=Wt, bias=bias, resid=resid, ref=ref)


def build_all_exact_cases():
    """Every integer case of the GPU tests, built once (each builder asserts its caps); returns (count, largest |ref| of the fp16-out cases, of the fp32-out cases)."""
    n, top16, top32 = 0, 0, 0
    for _, M, N, K in gemm_f16_cases():
        for epi, shared in EPILOGUES:
            top = int(gemm_case(M, N, K, epi, shared).ref.abs().max())
            top16, top32 = (max(top16, top), top32) if epi == 0 else (top16, max(top32, top))
            n += 1
    for _, M, N, K in latency_cases():
        for epi in (0, 2):
            top = int(gemm_case(M, N, K, epi).ref.abs().max())
            top16, top32 = (max(top16, top), top32) if epi == 0 else (top16, max(top32, top))
            n += 1
    for s in QKV_SHAPES:
        c = qkv_case(*s)
        top16 = max(top16, int(c.q.abs().max()), int(c.k.abs().max()), int(c.vt.abs().max()))
        n += 1
    for s in LINEAR_SHAPES:
        top16 = max(top16, int(linear_case(*s).ref.abs().max()))
        n += 1
    for _, N, H, W, Cin, Cout, modes in CONV_CASES:
        for mode in modes:
            top16 = max(top16, int(conv_case(N, H, W, Cin, Cout, mode).ref.abs().max()))
            n += 1
    return n, top16, top32


# ------------------------------------------------------------------------------------------------ real-valued cases with a derived per-element bound
def gelu_tanh64(x):
    x = x.double()
    return 0.5 * x * (1.0 + torch.tanh(math.sqrt(2.0 / math.pi) * (x + 0.044715 * x ** 3)))


GELU_SHAPES = {1: (300, 260), 4: (300, 260), 5: (300, 260), 6: (300, 260), 7: (192, 192), 8: (200, 176)}
GELU_K = 64


@functools.lru_cache(maxsize=None)
def gelu_case(M, N, K=GELU_K):
    """A = integers / 8 in [-1, 1], W in {-1, 0, 1}, bias = integers / 8 in [-2, 2]: the pre-activation is an exact multiple of 1/8 (exact in fp32 in any
    order), known in float64.  At K = 64 its standard deviation is about 4.2: both saturated tails, the fp16-subnormal part of the negative tail included.
    bound = 1.5 * 2^-11 * |ref| + 2^-24: one fp16 rounding costs 2^-11 relative (2^-25 absolute among the subnormals); the fp32 v_exp_f32 / v_rcp_f32
    evaluation costs about 1e-5 relative at |z| = 24 and fits in the remaining half."""
    g = torch.Generator().manual_seed(97 + M + N + K)
    A, W, bias = randint(g, (M, K), 8), randint(g, (N, K), 1), randint(g, (N,), 16)
    pre = (exact_mm(A, W) + bias).double() / 8.0
    ref = gelu_tanh64(pre)
    return SimpleNamespace(M=M, N=N, K=K, A=A.double() / 8, W=W.double(), bias=bias.double() / 8, pre=pre, ref=ref,
                           bound=1.5 * 2.0 ** -11 * ref.abs() + 2.0 ** -24)


GAUSS_SHAPES = {1: (300, 260, 320), 4: (300, 260, 320), 5: (300, 260, 320), 6: (300, 260, 320), 7: (192, 192, 320), 8: (200, 176, 320)}


@functools.lru_cache(maxsize=None)
def gauss_case(M, N, K, epi):
    """Gaussian fp16 operands against float64 with the per-element bound of a K-term fp32 dot product:
        |got - ref| <= (K + 2) 2^-23 (|A| |W|^T + |bias|)[m, n]       (+ 2^-11 |ref| for the rounding of an fp16 output)
    (each of the K products is exact in fp32, each of the K additions -- in any order, the bias add included -- rounds by at most 2^-24 relative to a
    partial sum that |A| |W|^T + |bias| bounds; K + 2 leaves room for the second-order terms).  Epilogue 3, X + gate * t with t the above: the error of t
    times |gate|, plus two more roundings (the product, the final add; one if they are fused), each at most 2^-24 relative to |gate t| + |ref|."""
    g = torch.Generator().manual_seed(13 + M + N + K + epi)
    A = (torch.randn(M, K, generator=g) * 0.5).half()
    W = (torch.randn(N, K, generator=g) / K ** 0.5).half()
    bias = torch.randn(N, generator=g) * 0.1
    t = A.double() @ W.double().t() + bias.double()
    bound = (K + 2) * 2.0 ** -23 * (A.double().abs() @ W.double().abs().t() + bias.double().abs())
    c = SimpleNamespace(M=M, N=N, K=K, epi=epi, A=A, W=W, bias=bias, X=None, gate=None, tokens=TOKENS)
    if epi == 3:
        c.X = torch.randn(M, N, generator=g)
        c.gate = torch.randn(M // TOKENS, N, generator=g)
        gr = c.gate.double().repeat_interleave(TOKENS, 0)
        ref = c.X.double() + gr * t
        bound = gr.abs() * bound + 2.0 ** -23 * ((gr * t).abs() + ref.abs())
    else:
        ref = t
        if epi == 0:
            bound = bound + 2.0 ** -11 * ref.abs()
    c.ref, c.bound = ref, bound
    return c
