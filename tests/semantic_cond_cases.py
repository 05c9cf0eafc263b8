"""Cases, references and bounds of the label-map conditioning stage of mask-to-image synthesis (lfm_label_rescale_f32, csrc/label_rescale.h;
``SpatialRescaler.encode_labels``): shared by tests/test_semantic_cond_ref.py (CPU), tests/test_gpu_label_rescale.py, tests/test_gpu_semantic_syn.py and
tools/make_semantic_cond_golden.py, so the mistakes are shown to leave the bound on the very inputs the GPU test uses.

The stage (reference downstream_tasks/test_flow_latent_semantic_syn.py:131-135 over models/encoder.py:90-112):
    F.one_hot(labels, num_cls) -> n_stages x F.interpolate(scale_factor=0.5, mode="bilinear") -> 1x1 channel_mapper.
The float64 restatement here is NOT the gather the kernel runs: it builds, per 2^n x 2^n cell, the cell mean of the one-hot map (the class histogram / P,
P = 4^n) and multiplies it with the weight, as the reference does after its interpolation stages.

The bound, per element (P = 4^n pixels per cell):
    |err| <= (P + 2) * 2^-24 * (sum_p |w[o, label_p]| / P + |b_o|)
P - 1 fp32 additions of a sum whose partial sums never exceed sum_p |w|, each rounding at most 2^-24 of that, the division by a power of two exact, one
rounding for the bias add (at most 2^-24 of |sum| / P + |b|), and the weight itself exact in fp32: (P - 1 + 1) * 2^-24 suffice; P + 2 leaves room for the
second-order terms and for a reference that rounds the cell means' products one by one."""
import collections
import zlib

import torch

F32, F64, I64 = torch.float32, torch.float64, torch.int64
U = 2.0 ** -24

Case = collections.namedtuple("Case", "N H W num_cls cout n_stages bias")

SHAPES = [(8, 8), (16, 16), (43, 43), (48, 80), (72, 72)]
STAGES = (1, 2, 3)
CLASSES = (1, 19, 151, 182, 1024)
BATCHES = (1, 3)
COUT = 4  # the reference's conditioning latent
# beyond the issue's list: four stages (16 lanes per cell with one label per lane: the last step of the lane tree) wherever a whole 16 x 16 cell fits, and every
# Cout the entry point takes
DEEP_SHAPES = [(16, 16), (43, 43), (48, 80), (72, 72)]
COUT_SWEEP = (1, 2, 3, 5, 6, 7, 8)


def exact_cases(shape):
    """The bit-for-bit cases of one H x W: every n_stages x num_cls x N x bias of the lists above, plus n_stages 4 and the other widths."""
    H, W = shape
    out = [Case(N, H, W, k, COUT, n, b) for n in STAGES for k in CLASSES for N in BATCHES for b in (False, True)]
    if shape in DEEP_SHAPES:
        out += [Case(N, H, W, k, COUT, 4, True) for k in (19, 1024) for N in BATCHES]
    out += [Case(3, H, W, 182, c, 3 if H >= 8 else 2, c % 2 == 1) for c in COUT_SWEEP]
    return out


def gauss_cases():
    """Gaussian weights: every shape and n_stages it allows, three class counts, both bias settings spread over them, N = 3."""
    out = []
    for H, W in SHAPES:
        for n in (1, 2, 3, 4):
            if min(H, W) < (1 << n):
                continue
            for i, k in enumerate((19, 182, 1024)):
                out.append(Case(3, H, W, k, COUT, n, (i + n) % 2 == 0))
    out += [Case(3, 43, 43, 151, c, 3, c % 2 == 0) for c in COUT_SWEEP]
    return out


# the cases whose outputs the fixture holds (tests/golden/semantic_cond.pt): each shape, each n_stages, each class count and both bias settings at least once
GOLDEN_CASES = [Case(2, 8, 8, 1, 4, 1, True), Case(3, 8, 8, 19, 4, 3, False), Case(3, 16, 16, 151, 4, 2, True), Case(3, 16, 16, 19, 4, 4, False),
                Case(3, 43, 43, 182, 4, 3, True), Case(3, 43, 43, 19, 4, 1, False), Case(3, 43, 43, 151, 7, 3, True), Case(3, 48, 80, 182, 4, 3, False),
                Case(3, 48, 80, 1024, 4, 2, True), Case(3, 72, 72, 1024, 4, 3, True), Case(3, 72, 72, 182, 4, 4, False), Case(2, 64, 64, 19, 4, 3, False)]


def case_id(c):
    return f"{c.N}x{c.H}x{c.W}-cls{c.num_cls}-out{c.cout}-n{c.n_stages}-{'bias' if c.bias else 'nobias'}"


def _gen(c, salt):
    return torch.Generator().manual_seed(zlib.crc32(f"{salt}:{tuple(c)}".encode()))


def make_labels(c):
    """iid labels over the whole class range, first and last class present wherever there are two pixels."""
    lab = torch.randint(0, c.num_cls, (c.N, c.H, c.W), generator=_gen(c, "labels"), dtype=I64)
    lab[0, 0, 0], lab[-1, (c.H >> c.n_stages << c.n_stages) - 1, (c.W >> c.n_stages << c.n_stages) - 1] = 0, c.num_cls - 1
    return lab


def gauss_weights(c):
    """-> (w fp32 [Cout, num_cls], bias fp32 [Cout] or None), N(0, 1)."""
    g = _gen(c, "gauss")
    w = torch.randn(c.cout, c.num_cls, generator=g, dtype=F32)
    return w, (torch.randn(c.cout, generator=g, dtype=F32) if c.bias else None)


def int_weights(c):
    """Integers in [-8, 8]: |sum over a cell| <= 8 P <= 2048 and the divisor is a power of two, so every fp32 order of summation gives the exact result."""
    g = _gen(c, "int")
    w = torch.randint(-8, 9, (c.cout, c.num_cls), generator=g).to(F32)
    return w, (torch.randint(-8, 9, (c.cout,), generator=g).to(F32) if c.bias else None)


def whole(c):
    """Rows and columns covered by whole cells."""
    return (c.H >> c.n_stages) << c.n_stages, (c.W >> c.n_stages) << c.n_stages


def poison_ragged_edge(c, labels):
    """Every pixel outside the last whole cell holds the invalid label num_cls: a kernel that reads one of them makes a NaN.  (At 43 x 43 these are rows and
    columns 40..42 for n_stages 2 and 3; for n_stages 1 the last whole cell ends at 41, so only row and column 42 are outside.)"""
    Hc, Wc = whole(c)
    lab = labels.clone()
    lab[:, Hc:, :] = c.num_cls
    lab[:, :, Wc:] = c.num_cls
    return lab


# ------------------------------------------------------------------------------------------------ float64 restatement: cell mean, then matmul
MISTAKES = ("origin", "cell_size", "drop_row", "ragged", "transposed", "bias_first")


def mistake_shows(mistake, c):
    if mistake == "origin":  # a shifted window over iid labels: another histogram as soon as there are two classes (the restatement wraps at the image's end,
        return c.num_cls > 1 and (c.H, c.W) != (1 << c.n_stages, 1 << c.n_stages)  # so a single cell that IS the image keeps its histogram)
    if mistake == "ragged":
        return (c.H, c.W) != whole(c)
    if mistake == "transposed":
        return c.num_cls > 1 and c.cout > 1
    if mistake == "bias_first":
        return c.bias
    return True


def cell_histogram(labels, num_cls, n_stages, mistake=None):
    """-> float64 [N, h, w, num_cls]: how many pixels of each class the cell holds (what n x bilinear x0.5 of the one-hot map is, times P)."""
    N, H, W = labels.shape
    c = 1 << n_stages
    h, w = H >> n_stages, W >> n_stages
    if mistake == "origin":
        labels = torch.roll(labels, (-1, -1), (1, 2))
    ys, xs = torch.arange(H), torch.arange(W)
    cy, cx = ys // c, xs // c
    use_y, use_x = cy < h, cx < w
    if mistake == "ragged":
        cy, cx, use_y, use_x = cy.clamp(max=h - 1), cx.clamp(max=w - 1), torch.ones(H, dtype=torch.bool), torch.ones(W, dtype=torch.bool)
    if mistake == "drop_row":
        use_y = use_y & (ys % c != c - 1)
    cell = (cy[:, None] * w + cx[None, :]).expand(N, H, W) + (torch.arange(N) * h * w)[:, None, None]
    use = (use_y[:, None] & use_x[None, :]).expand(N, H, W)
    hist = torch.zeros(N * h * w * num_cls, dtype=F64)
    hist.index_add_(0, (cell[use] * num_cls + labels[use]), torch.ones(int(use.sum()), dtype=F64))
    return hist.reshape(N, h, w, num_cls)


def restate64(labels, w, bias, n_stages, mistake=None):
    """out[n, o, i, j] = (cell mean of the one-hot map) . w[o, :] + b[o] in float64, with one named mistake."""
    cout, num_cls = w.shape
    P = float(4 ** n_stages)
    w64 = w.to(F64)
    if mistake == "transposed":
        w64 = w64.reshape(num_cls, cout).t()
    b64 = bias.to(F64) if bias is not None else torch.zeros(cout, dtype=F64)
    hist = cell_histogram(labels, num_cls, n_stages, mistake)
    if mistake == "bias_first":
        out = (hist @ w64.t() + b64) / P
    else:
        out = (hist / (float(2 ** n_stages) if mistake == "cell_size" else P)) @ w64.t() + b64
    return out.permute(0, 3, 1, 2).contiguous()


def bound(labels, w, bias, n_stages):
    """The per-element bound of the module docstring, float64 [N, Cout, h, w]."""
    P = 4 ** n_stages
    mean_abs = restate64(labels, w.abs(), None, n_stages)
    b = bias.to(F64).abs() if bias is not None else torch.zeros(w.shape[0], dtype=F64)
    return (P + 2) * U * (mean_abs + b[None, :, None, None])


def exact_int(labels, w, bias, n_stages):
    """Integer weights: the sums in int64, one exact division by 4^n, -> float64 (every value is an fp32 number)."""
    cout, num_cls = w.shape
    hist = cell_histogram(labels, num_cls, n_stages).to(I64)
    s = (hist @ w.to(I64).t()).permute(0, 3, 1, 2)
    out = s.to(F64) / float(4 ** n_stages)
    return out + bias.to(F64)[None, :, None, None] if bias is not None else out


# ------------------------------------------------------------------------------------------------ fp32 emulations
def _cell_values(labels, w, n_stages):
    """fp32 [N, Cout, h, c, w, c]: w[o, label] of every pixel of every whole cell."""
    N, H, W = labels.shape
    c = 1 << n_stages
    h, wo = H >> n_stages, W >> n_stages
    vals = w[:, labels[:, :h * c, :wo * c]]  # [Cout, N, h c, w c]
    return vals.permute(1, 0, 2, 3).reshape(N, w.shape[0], h, c, wo, c)


def emulate_kernel32(labels, w, bias, n_stages):
    """The kernel's order in fp32 (csrc/label_rescale.h): per pixel column of the cell the rows top to bottom, a binary tree over the columns with adjacent
    columns first, the exact scale 1 / 4^n, one add for the bias."""
    v = _cell_values(labels, w, n_stages)
    s = torch.zeros_like(v[:, :, :, 0])  # [N, Cout, h, w, c]
    for r in range(v.shape[3]):
        s = s + v[:, :, :, r]
    while s.shape[-1] > 1:
        s = s[..., 0::2] + s[..., 1::2]
    out = s[..., 0] * F32_INV[n_stages]
    return out + bias[None, :, None, None] if bias is not None else out


F32_INV = {n: torch.tensor(1.0 / 4 ** n, dtype=F32) for n in (1, 2, 3, 4)}


def emulate_sequential32(labels, w, bias, n_stages):
    """One fp32 accumulator over the cell's pixels in raster order."""
    v = _cell_values(labels, w, n_stages).permute(0, 1, 2, 4, 3, 5)
    v = v.reshape(*v.shape[:4], -1)
    s = torch.zeros_like(v[..., 0])
    for p in range(v.shape[-1]):
        s = s + v[..., p]
    out = s * F32_INV[n_stages]
    return out + bias[None, :, None, None] if bias is not None else out


def reference_chain(labels, w, bias, n_stages, dtype=F32):
    """The reference's own chain of torch calls (one-hot, n x F.interpolate bilinear x0.5, F.conv2d) in `dtype` on the CPU."""
    x = torch.nn.functional.one_hot(labels, w.shape[1]).permute(0, 3, 1, 2).to(dtype)
    for _ in range(n_stages):
        x = torch.nn.functional.interpolate(x, scale_factor=0.5, mode="bilinear")
    return torch.nn.functional.conv2d(x, w.to(dtype)[:, :, None, None], bias.to(dtype) if bias is not None else None)


def error_ratio(got, ref, bnd):
    """Largest |got - ref| / bound; NaN anywhere counts as infinite."""
    r = (got.to(F64) - ref).abs() / bnd
    return float("inf") if bool(r.isnan().any()) else float(r.max())


# ------------------------------------------------------------------------------------------------ refusals of lfm_label_rescale_f32 (include/lfm_hip.h)
ERR_SHAPE, ERR_ALIGN, ERR_ARG = -1, -2, -5
REFUSAL_BASE = dict(N=2, H=16, W=16, num_cls=19, cout=4, n_stages=3)  # the buffers of a caller of `refusals` serve this call
# (changed arguments, pointer offsets in bytes -- None = a NULL pointer -- , expected code); order of the checks: NULL pointers, then shapes, then alignment
REFUSALS = [
    ({}, {"labels": None}, ERR_ARG), ({}, {"w": None}, ERR_ARG), ({}, {"out": None}, ERR_ARG),
    ({"N": 0}, {"labels": None}, ERR_ARG), ({"cout": 9}, {"out": None, "w": 2}, ERR_ARG),  # a NULL pointer is named before a bad shape or alignment
    ({"N": 0}, {}, ERR_SHAPE), ({"N": -1}, {}, ERR_SHAPE), ({"n_stages": 0}, {}, ERR_SHAPE), ({"n_stages": 5}, {}, ERR_SHAPE),
    ({"cout": 0}, {}, ERR_SHAPE), ({"cout": 9}, {}, ERR_SHAPE), ({"num_cls": 0}, {}, ERR_SHAPE),
    ({"num_cls": 2049, "cout": 8}, {}, ERR_SHAPE), ({"num_cls": 16385, "cout": 1}, {}, ERR_SHAPE),  # one row more than 64 KiB of table
    ({"H": 7}, {}, ERR_SHAPE), ({"W": 7}, {}, ERR_SHAPE), ({"H": 15, "n_stages": 4}, {}, ERR_SHAPE), ({"W": 1, "n_stages": 1}, {}, ERR_SHAPE),
    ({"H": 7}, {"labels": 4, "out": 2}, ERR_SHAPE),  # a bad shape is named before a bad alignment
    ({}, {"labels": 4}, ERR_ALIGN), ({}, {"labels": 1}, ERR_ALIGN), ({}, {"w": 2}, ERR_ALIGN), ({}, {"bias": 1}, ERR_ALIGN), ({}, {"out": 2}, ERR_ALIGN),
]


def refusals(lib, labels, w, bias, out, stream):
    """Run every refusal on the caller's buffers (of REFUSAL_BASE's sizes: should a refusal fail to refuse, the call stays inside them or fails to launch).
    -> list of (changed arguments, offsets, expected, got)."""
    import ctypes

    base = {"labels": labels.data_ptr(), "w": w.data_ptr(), "bias": bias.data_ptr(), "out": out.data_ptr()}
    res = []
    for changed, offsets, expected in REFUSALS:
        a = dict(REFUSAL_BASE, **changed)
        p = {k: ctypes.c_void_p(None if k in offsets and offsets[k] is None else v + offsets.get(k, 0)) for k, v in base.items()}
        got = lib.lfm_label_rescale_f32(p["labels"], p["w"], p["bias"], p["out"], a["N"], a["H"], a["W"], a["num_cls"], a["cout"], a["n_stages"], stream)
        res.append((changed, offsets, expected, got))
    return res


# ------------------------------------------------------------------------------------------------ the module, as the reference declares it
def key_shapes(num_cls, cout, bias):
    """state_dict of models/encoder.py SpatialRescaler(in_channels=num_cls, out_channels=cout, bias=bias): one Conv2d named channel_mapper."""
    return [("channel_mapper.weight", (cout, num_cls, 1, 1))] + ([("channel_mapper.bias", (cout,))] if bias else [])


# defaults of the reference's parser (downstream_tasks/test_flow_latent_semantic_syn.py:154-227), written out; the fixture holds what the reference's own
# parser returned and tests/test_semantic_cond_ref.py compares all three
REFERENCE_DEFAULTS = dict(
    seed=1024, compute_fid=False, epoch_id=425, image_size=256, num_in_channels=8, num_out_channels=4, nf=256, centered=True, resamp_with_conv=True,
    num_res_blocks=2, num_heads=4, num_head_upsample=-1, num_head_channels=-1, attn_resolutions=(8, 4), ch_mult=(1, 2, 3, 4), dropout=0.0, num_classes=None,
    use_scale_shift_norm=True, resblock_updown=False, use_new_attention_order=False, scale_factor=0.18215, exp="experiment_cifar_default",
    real_img_dir="./pytorch_fid/cifar10_train_stat.npy", dataset="cifar10", num_timesteps=200, batch_size=200, atol=1e-5, rtol=1e-5, method="dopri5",
    step_size=0.01, perturb=False, pretrained_autoencoder_ckpt="../stabilityai/sd-vae-ft-mse")
