"""Shapes, inputs, references and named mistakes for the inpainting kernels (csrc/inpaint.h: lfm_inpaint_prepare_u8, lfm_inpaint_cond_f32,
lfm_inpaint_composite_u8) and ``inpaint_batch_u8``.  Shared by tests/test_inpaint_ref.py (CPU: pins everything here against the unmodified reference's stored
results, tests/golden/inpaint_prep.pt) and the GPU tests; tools/make_inpaint_golden.py draws its files from here too.

The fp32 restatement IS the reference's op sequence as torch and numpy run it on the CPU (downstream_tasks/test_flow_latent_inpainting.py: the dataset class
:36-55, the loop :148-150 and :157-160, torchvision.utils.save_image's mul(255).add_(0.5).clamp_(0, 255).to(uint8)): eager ops, each rounded on its own, no
FMA.  prepare and composite are compared with it bit for bit.  The cond stage has an exp in it, so it is compared per element with the fp64 restatement
inside a bound derived below from its operation count."""
import numpy as np
import torch
import torch.nn.functional as F

SHAPES = [(8, 8), (8, 24), (40, 16), (64, 64)]  # one group of 8; W % 16 != 0; several rows of 16; more than one workgroup's worth at N = 3 with 8 per lane
BATCHES = (1, 3)
GOLDEN_S, GOLDEN_N = 64, 3

MISTAKES = ("polarity", "pick_4", "latent_01", "scale_mask", "trunc", "no_round_trip", "fma", "layout")


def all_pairs():
    """One 256 x 256 image whose image byte is the row and whose mask byte is the column: all 65 536 (image byte, mask byte) pairs.  Channel c holds
    (row + 85 c) % 256, so every channel sees every pair and the three differ."""
    r = torch.arange(256).view(256, 1, 1)
    img = ((r + 85 * torch.arange(3).view(1, 1, 3)) % 256).expand(256, 256, 3).to(torch.uint8).contiguous().unsqueeze(0)
    mask = torch.arange(256).view(1, 256).expand(256, 256).to(torch.uint8).contiguous().unsqueeze(0)
    return img, mask


def make_bytes(N, H, W, seed=0):
    """-> (image uint8 [N,H,W,3], mask uint8 [N,H,W]): random image bytes; mask bytes a third 255, a third 0, a third anything, pixel by pixel (so the
    pick [::8, ::8] differs from every other pick)."""
    g = torch.Generator().manual_seed(1000 * seed + 7 * H + W + N)
    img = torch.randint(0, 256, (N, H, W, 3), generator=g, dtype=torch.uint8)
    kind = torch.randint(0, 3, (N, H, W), generator=g)
    grey = torch.randint(0, 256, (N, H, W), generator=g)
    mask = torch.where(kind == 0, torch.full_like(grey, 255), torch.where(kind == 1, torch.zeros_like(grey), grey)).to(torch.uint8)
    return img, mask


def make_fake(N, H, W, seed=0):
    """A decoded sample: fp32 [N,3,H,W], mostly inside [-1,1], some beyond it (both clamps of the quantisation)."""
    g = torch.Generator().manual_seed(2000 * seed + 5 * H + W + N)
    return (torch.rand(N, 3, H, W, generator=g) * 2.6 - 1.3).float()


def make_fake_at_the_boundaries(img_u8, mask_u8, seed=0):
    """make_fake, but wherever the mask lets the sample through and a solution inside [-1,1] exists (three elements in four of those), the sample is chosen so
    that composite * 255 + 0.5 lands within a few fp32 ulps of an integer: there the last bit of every operation decides the byte, so one contracted FMA, a
    dropped round trip or a reordered sum shows in the bytes, which at random samples happens once in some 10^5 elements."""
    N, H, W, _ = img_u8.shape
    g = torch.Generator().manual_seed(4000 * seed + 3 * H + W + N)
    fake = make_fake(N, H, W, seed)
    image, mask_pm1, _, _ = prepare32(img_u8, mask_u8)
    mm, i01 = ((mask_pm1 + 1.0) / 2.0).double().expand(N, 3, H, W), ((image + 1.0) / 2.0).double()
    k = torch.randint(1, 255, (N, 3, H, W), generator=g).double()
    f01 = ((k - 0.5) / 255.0 - (1 - mm) * i01) / mm.clamp_min(1e-9)
    jitter = 1.0 + torch.randint(-2, 3, (N, 3, H, W), generator=g).double() * 2.0 ** -23
    use = (mm > 0) & (f01 >= 0) & (f01 <= 1) & (torch.rand(N, 3, H, W, generator=g) < 0.75)
    return torch.where(use, ((2.0 * f01 - 1.0) * jitter).float(), fake)


def gpu_inputs():
    """(name, (image bytes, mask bytes, decoded sample)) of every prepare / composite case of tests/test_gpu_inpaint_kernels.py."""
    img, mask = all_pairs()
    yield "pairs", (img, mask, make_fake_at_the_boundaries(img, mask, seed=1))
    for (H, W) in SHAPES:
        for N in BATCHES:
            img, mask = make_bytes(N, H, W)
            yield f"{N}x{H}x{W}", (img, mask, make_fake_at_the_boundaries(img, mask))


def fma32(a, b, c):
    """round32(a * b + c) with one rounding: the product of two fp32 is exact in fp64 (the fp64 sum's own rounding is far below half an fp32 ulp)."""
    return (a.double() * b.double() + c.double()).float()


# ------------------------------------------------------------------ the fp32 restatement (the reference's ops on the CPU)
def prepare32(img_u8, mask_u8, mistake=None):
    """The dataset's three tensors and the mask on the latent grid: (image [N,3,H,W], mask [N,1,H,W] (+1 = hole), masked image [N,3,H,W], cc [N,1,H/8,W/8])."""
    N, H, W, _ = img_u8.shape
    a = img_u8.numpy()
    a = a.reshape(N, 3, H, W) if mistake == "layout" else np.transpose(a, (0, 3, 1, 2))  # :38
    img = torch.from_numpy(np.ascontiguousarray(a).astype(np.float32) / 255.0)  # :45-46
    mask = mask_u8 / 255.0  # :42
    if mistake != "polarity":
        mask = 1 - mask  # :43
    masked = (1 - mask).unsqueeze(1) * img  # :47
    image, mask_pm1, masked = img * 2.0 - 1.0, (mask * 2.0 - 1.0).unsqueeze(1), masked * 2.0 - 1.0  # :51-54
    src = mask.unsqueeze(1) if mistake == "latent_01" else mask_pm1
    cc = src[:, :, 4::8, 4::8].contiguous() if mistake == "pick_4" else F.interpolate(src, size=(H // 8, W // 8))  # :148
    return image, mask_pm1, masked, cc


def composite32(fake, image, mask_pm1, mistake=None):
    """The loop's :157-160 on the dataset's tensors -> the composite in [0,1], fp32 [N,3,H,W]."""
    to_range_0_1 = lambda x: (x + 1.0) / 2.0  # noqa: E731
    f01, mm = to_range_0_1(fake), to_range_0_1(mask_pm1)
    i01 = (image + 1.0) / 2.0
    if mistake == "fma":
        return fma32(f01, mm.expand_as(f01), (1 - mm) * i01)
    return f01 * mm + (1 - mm) * i01


def save_image_bytes(x01, mistake=None):
    """torchvision.utils.save_image's conversion of [N,3,H,W] in [0,1] -> uint8 NHWC (lfm_amd.io_formats.to_uint8_rounding)."""
    x = x01.mul(255) if mistake == "trunc" else x01.mul(255).add_(0.5)
    x = x.clamp_(0, 255).to(torch.uint8)
    return x.reshape(x.shape[0], x.shape[2], x.shape[3], 3) if mistake == "layout" else x.permute(0, 2, 3, 1).contiguous()


def composite_bytes32(fake, img_u8, mask_u8, mistake=None):
    """What lfm_inpaint_composite_u8 states: the dataset's tensors from the bytes, :157-160, save_image's bytes."""
    image, mask_pm1, _, _ = prepare32(img_u8, mask_u8, mistake if mistake in ("polarity", "layout") else None)
    if mistake == "no_round_trip":  # the image and mask taken in [0,1] directly instead of through [-1,1] and back
        i01 = torch.from_numpy(np.ascontiguousarray(np.transpose(img_u8.numpy(), (0, 3, 1, 2))).astype(np.float32) / 255.0)
        mm = (1 - mask_u8 / 255.0).unsqueeze(1)
        return save_image_bytes(((fake + 1.0) / 2.0) * mm + (1 - mm) * i01)
    return save_image_bytes(composite32(fake, image, mask_pm1, mistake), mistake)


def cond_cat32(c, cc, scale, mistake=None):
    """:147 (.mul_(scale_factor) on the latent) and :150 -- the 5-channel conditioning tensor from the sampled latent c (unscaled here) and the mask cc."""
    out = torch.cat((c * scale, cc), dim=1)
    return torch.cat((c, cc), dim=1) * scale if mistake == "scale_mask" else out


# ------------------------------------------------------------------ the cond stage: fp32 as torch does it, fp64, and the bound
def make_moments(N, h, w, seed=0, extremes=False):
    """-> (moments fp32 [N,8,h,w], eps fp32 [N,4,h,w]).  logvar ~ N(-3, 4) as an encoder gives; `extremes` plants -40 and 25 (beyond both clamps), +-30, 20."""
    g = torch.Generator().manual_seed(3000 * seed + 11 * h + w + N)
    mean, logvar = torch.randn(N, 4, h, w, generator=g) * 3, torch.randn(N, 4, h, w, generator=g) * 2 - 3
    if extremes:
        flat = logvar.view(-1)
        for k, v in enumerate((-40.0, 25.0, -30.0, 20.0, -1e30, 1e30)):
            flat[k * 5 % flat.numel()] = v
    return torch.cat((mean, logvar), 1).contiguous(), torch.randn(N, 4, h, w, generator=g)


def scale32(scale):
    """The scale factor as a fp32 kernel argument and as torch's mul_ on a fp32 tensor see it."""
    return float(np.float32(scale))


def cond32(moments, eps, scale):
    """DiagonalGaussianDistribution.sample() with the noise given, then .mul_(scale) (:147), in fp32 on the CPU; eps None: .mode()."""
    mean, logvar = torch.chunk(moments, 2, dim=1)
    if eps is None:
        return mean.clone().mul_(scale)
    std = torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0))
    return (mean + std * eps).mul_(scale)


def cond64(moments, eps, scale):
    mean, logvar = torch.chunk(moments.double(), 2, dim=1)
    if eps is None:
        return mean * scale32(scale)
    return (mean + torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * eps.double()) * scale32(scale)


U = 2.0 ** -24  # unit roundoff of fp32: one rounded operation is off by at most U relative
EXP_ULP = 2.0 ** -23  # expf documented at 1 ulp (HIP's OCML routine; torch's CPU exp likewise): at most 2^-23 relative


def cond_bound(moments, eps, scale):
    """Per-element bound of |fp32 result - fp64 result|.  0.5 * clamp(logvar) is exact.  With t = std * eps:  std carries the exp's ulp, the product one rounding
    (t off by |t| (EXP_ULP + U)), the sum one more ((|mean| + |t|) U), the scaling a last one ((|mean| + |t|) U):
        |err| <= |scale| (|t| (EXP_ULP + 3 U) + 2 U |mean|)
    to first order; (1 + 2^-20) covers the products of those terms and 2^-148 a result in the subnormals.  eps None: mean * scale, one rounding."""
    mean, logvar = torch.chunk(moments.double(), 2, dim=1)
    s = abs(scale32(scale))
    if eps is None:
        return s * mean.abs() * U + 2.0 ** -148
    t = (torch.exp(0.5 * torch.clamp(logvar, -30.0, 20.0)) * eps.double()).abs()
    return s * (t * (EXP_ULP + 3 * U) + 2 * U * mean.abs()) * (1 + 2.0 ** -20) + 2.0 ** -148


def error_ratio(got, ref64, bound):
    """max over the elements of |got - ref| / bound (a non-finite element counts as infinitely wrong)."""
    err = (got.double() - ref64).abs()
    if not bool(torch.isfinite(err).all()):
        return float("inf")
    return float((err / bound).max())


# ------------------------------------------------------------------ files
def write_pairs(img_dir, mask_dir, img_u8, mask_u8, quality=95):
    """The reference's naming: {img_dir}/%06d.jpg, {mask_dir}/%06d.png."""
    import os

    from PIL import Image

    os.makedirs(img_dir, exist_ok=True)
    os.makedirs(mask_dir, exist_ok=True)
    for k in range(img_u8.shape[0]):
        Image.fromarray(img_u8[k].numpy()).save(os.path.join(img_dir, f"{k:06d}.jpg"), quality=quality)
        Image.fromarray(mask_u8[k].numpy()).save(os.path.join(mask_dir, f"{k:06d}.png"))


def golden_pairs():
    """The fixture's three 64 x 64 pairs before they are written to files: smooth images (a JPEG keeps them close), masks with a box hole, a soft (grey) border
    around it and a few grey pixels elsewhere."""
    g = torch.Generator().manual_seed(64)
    S, N = GOLDEN_S, GOLDEN_N
    img = F.interpolate(torch.rand(N, 3, S // 8, S // 8, generator=g), size=(S, S), mode="bilinear", align_corners=False)
    img = img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()
    mask = torch.full((N, S, S), 255, dtype=torch.uint8)
    for k in range(N):
        y0, x0 = 8 + 5 * k, 12 + 7 * k
        mask[k, y0 - 3:y0 + 27, x0 - 3:x0 + 23] = 128 + 40 * k - 3
        mask[k, y0:y0 + 24, x0:x0 + 20] = 0
        mask[k, ::9, ::11] = torch.randint(1, 255, mask[k, ::9, ::11].shape, generator=g, dtype=torch.uint8)
    return img, mask
