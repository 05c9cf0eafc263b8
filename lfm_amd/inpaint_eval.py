"""The SSIM half of the reference's inpainting evaluation on the device (drop-in for the pieces of the reference's datasets_prep/inpaint_preprocess that
need nothing but arithmetic: ``losses/ssim.py`` ``SSIM``, ``losses/base_loss.py`` ``SSIMScore`` / ``PairwiseScore.get_value`` / ``get_groupings``, and
``evaluator.py`` ``InpaintingEvaluator``'s bins by mask area and its result dictionary).  LPIPS and FID, the evaluator's other scores, need network weights
and are not here.

The reference's ``SSIM._ssim`` is five depthwise 11 x 11 convolutions and about fifteen elementwise ops over full-resolution fp32 tensors;
``lfm_ssim_u8`` / ``lfm_ssim_f32`` (csrc/ssim.h) read the two images once and write one float per image, and for bytes also the exact sum of each mask, from
which the bins follow.  Device tensors go through those kernels; CPU tensors go through a plain torch restatement of the reference's lines (no HIP there).

    results = evaluate(generated_u8, image_u8, mask_u8)     # {("ssim", "total"): {"mean", "std"}, ("ssim", "10-20%"): {...}, ...}
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from . import hip


class SSIM(torch.nn.Module):
    """``losses/ssim.py`` ``SSIM``: the constructor and ``forward(img1, img2)`` on [N,C,H,W] tensors; a scalar with ``size_average`` (the mean over the
    whole batch), else one value per image.  fp32 tensors on the device run ``hip.ssim_f32`` (1 <= C <= 4, window_size odd and 3..11; anything else there is
    an error, not a slower path); CPU tensors of any float dtype run the torch ops below."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        self.window_size = window_size
        self.size_average = size_average

    def window(self, channel, like):
        w1 = hip.ssim_gaussian(self.window_size).unsqueeze(1)
        w2 = w1.mm(w1.t()).float().unsqueeze(0).unsqueeze(0)
        return w2.expand(channel, 1, self.window_size, self.window_size).contiguous().type_as(like)

    def forward(self, img1, img2):
        assert len(img1.shape) == 4
        if img1.is_cuda:
            if img1.dtype != torch.float32:
                raise hip.LfmHipError(f"SSIM: device tensors must be fp32 (lfm_ssim_f32), got {img1.dtype}")
            per_image = hip.ssim_f32(img1.contiguous(), img2.contiguous(), self.window_size)
            return per_image.mean() if self.size_average else per_image
        per_image = ssim_torch(img1, img2, self.window(img1.shape[1], img1))
        return per_image.mean() if self.size_average else per_image


def ssim_torch(img1, img2, window):
    """``SSIM._ssim`` with size_average=False as plain torch ops (losses/ssim.py:47-67), on whatever device the tensors are: the CPU path of ``SSIM``, and
    the op chain tools/ssim_time.py times the kernel against.  `window` is the [C,1,ws,ws] depthwise weight.  (The mean over H*W*C of equally sized
    images' maps is the mean of the per-image means: ``ssim_map.mean()`` of the reference's size_average up to rounding.)"""
    channel, pad = img1.shape[1], window.shape[-1] // 2
    mu1 = F.conv2d(img1, window, padding=pad, groups=channel)
    mu2 = F.conv2d(img2, window, padding=pad, groups=channel)
    mu1_sq, mu2_sq, mu1_mu2 = mu1.pow(2), mu2.pow(2), mu1 * mu2
    sigma1_sq = F.conv2d(img1 * img1, window, padding=pad, groups=channel) - mu1_sq
    sigma2_sq = F.conv2d(img2 * img2, window, padding=pad, groups=channel) - mu2_sq
    sigma12 = F.conv2d(img1 * img2, window, padding=pad, groups=channel) - mu1_mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    ssim_map = ((2 * mu1_mu2 + C1) * (2 * sigma12 + C2)) / ((mu1_sq + mu2_sq + C1) * (sigma1_sq + sigma2_sq + C2))
    return ssim_map.mean(1).mean(1).mean(1)


def get_groupings(groups):
    """{group index: the indices of its elements, in the order a plain argsort of `groups` gives} (``base_loss.get_groupings``)."""
    labels, counts = np.unique(groups, return_counts=True)
    order, grouping, start = np.argsort(groups), {}, 0
    for label, count in zip(labels, counts):
        grouping[label] = order[start:start + count]
        start += count
    return grouping


class SSIMScore(torch.nn.Module):
    """``base_loss.SSIMScore``: ``forward(pred, target, mask=None)`` scores a batch and keeps the per-image values, ``get_value(groups=None)`` returns
    ({"mean", "std"} over all images, None or {group: {"mean", "std"}}) with numpy's population std over the values held as float64, ``reset()`` forgets
    them.  Besides the reference's float [N,C,H,W] tensors in [0,1] it takes uint8 NHWC [N,H,W,3] batches: on the device they run ``hip.ssim_u8``, and a
    uint8 mask [N,H,W] given with them has its byte sums kept in ``mask_sums`` (for ``area_bins``); on the CPU they are divided by 255 first.  Values and sums stay
    on their device until ``get_value``, ``individual_values`` or ``mask_sums`` asks for them, so scoring a batch does not wait for it."""

    def __init__(self, window_size=11):
        super().__init__()
        self.window_size = window_size
        self.score = SSIM(window_size=window_size, size_average=False).eval()
        self.reset()

    def reset(self):
        self._batches, self._mask_batches = [], []

    @torch.no_grad()
    def forward(self, pred_batch, target_batch, mask=None):
        if pred_batch.dtype == torch.uint8:
            if pred_batch.is_cuda:
                m = mask if mask is not None and mask.dtype == torch.uint8 and mask.dim() == 3 else None
                batch_values, sums = hip.ssim_u8(pred_batch.contiguous(), target_batch.contiguous(), m.contiguous() if m is not None else None, self.window_size)
                if sums is not None:
                    self._mask_batches.append(sums)
            else:
                d255 = torch.full((), 255.0)
                batch_values = self.score(pred_batch.permute(0, 3, 1, 2).float() / d255, target_batch.permute(0, 3, 1, 2).float() / d255)
                if mask is not None and mask.dtype == torch.uint8 and mask.dim() == 3:
                    self._mask_batches.append(mask.to(torch.int64).sum(dim=(1, 2)))
        else:
            batch_values = self.score(pred_batch, target_batch)
        self._batches.append(batch_values.detach())
        return batch_values

    @property
    def individual_values(self):
        """float64 numpy, as the reference's ``np.hstack`` of its float32 batches onto an empty list gives."""
        return np.hstack([np.array([])] + [b.cpu().numpy() for b in self._batches])

    @property
    def mask_sums(self):
        return np.hstack([np.array([], dtype=np.int64)] + [b.cpu().numpy() for b in self._mask_batches])

    def get_value(self, groups=None):
        values = self.individual_values
        total = {"mean": values.mean(), "std": values.std()}
        if groups is None:
            return total, None
        group_results = {}
        for label, index in get_groupings(groups).items():
            scores = values[index]
            group_results[label] = {"mean": scores.mean(), "std": scores.std()}
        return total, group_results


def interval_names(bins=10):
    """``InpaintingEvaluator._get_bin_edges``' names: "0-10%", "10-20%", ... with ceil(log10(bins)) - 1 decimals."""
    edges = np.linspace(0, 1, bins + 1)
    digits = max(0, math.ceil(math.log10(bins)) - 1)
    fmt = lambda v: "{:.{n}f}".format(round(100 * v, digits), n=digits)  # noqa: E731
    return ["{0}-{1}%".format(fmt(edges[k]), fmt(edges[k + 1])) for k in range(bins)]


def area_bins(mask_sum, H, W, bins=10):
    """Per-image sums of mask bytes (the driver's convention: 255 = keep, 0 = hole) -> (group index per image, the interval names).

    The reference's evaluator takes ``area = mask.mean()`` of its float mask (1 = hole), i.e. the hole share ``1 - sum / (255 H W)``, and bins it with
    ``np.searchsorted(np.linspace(0, 1, bins + 1), area, side="right") - 1``, an area of 1.0 going to the last bin.  Here the share is the exact rational
    ``(255 H W - sum) / (255 H W)`` and the index is ``floor(share * bins)`` in integer arithmetic, the last bin taking 1.0: a share in [k / bins, (k + 1) /
    bins) has index k, and a mask that sits exactly on an edge k / bins has the one defined index k.  The reference's ``area`` is an fp32 mean of fp32
    quotients and can fall on the other side of such an edge (and its edges are the float64 values of linspace, e.g. 0.30000000000000004); away from the
    edges the two agree."""
    full = 255 * int(H) * int(W)
    groups = []
    for s in np.asarray(mask_sum).reshape(-1).tolist():
        s = int(s)
        if s < 0 or s > full:
            raise ValueError(f"area_bins: a mask sum of {s} is outside [0, 255 * {H} * {W}]")
        groups.append(min(((full - s) * bins) // full, bins - 1))
    return np.array(groups, dtype=np.int64), interval_names(bins)


def results_by_name(score, groups, names, score_name="ssim"):
    """The evaluator's result dictionary: {(score_name, "total"): {...}, (score_name, interval name): {...}} with a "count" beside mean and std."""
    total, per_group = score.get_value(groups=groups)
    results = {(score_name, "total"): dict(total, count=int(len(groups)))}
    for index, values in per_group.items():
        results[(score_name, names[index])] = dict(values, count=int((np.asarray(groups) == index).sum()))
    return results


@torch.no_grad()
def evaluate(generated_u8, image_u8, mask_u8, batch_size=32, bins=10, window_size=11, device=None):
    """``InpaintingEvaluator(dataset, {"ssim": SSIMScore()}, bins=bins, batch_size=batch_size).evaluate()`` on bytes: generated and ground-truth images uint8
    [M,H,W,3] and masks uint8 [M,H,W] (255 = keep, 0 = hole), numpy or torch, host or device -> {("ssim", "total" | interval name): {"mean", "std",
    "count"}}.  Each batch is one ``lfm_ssim_u8`` call; M floats and M integers come back, once, at the end."""
    as_t = lambda a: a if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
    gen, img, msk = as_t(generated_u8), as_t(image_u8), as_t(mask_u8)
    if gen.shape != img.shape or gen.dim() != 4 or gen.shape[-1] != 3 or tuple(msk.shape) != tuple(gen.shape[:3]):
        raise ValueError(f"evaluate: expected uint8 [M,H,W,3], [M,H,W,3] and [M,H,W], got {tuple(gen.shape)}, {tuple(img.shape)}, {tuple(msk.shape)}")
    device = torch.device(device or "cuda:0")
    score = SSIMScore(window_size)
    for start in range(0, gen.shape[0], batch_size):
        part = [t[start:start + batch_size].to(device).contiguous() for t in (gen, img, msk)]
        score(part[0], part[1], part[2])
    groups, names = area_bins(score.mask_sums, gen.shape[1], gen.shape[2], bins)
    return results_by_name(score, groups, names)


def format_table(results, title="SSIM"):
    """The result dictionary as the lines the drivers print: total first, then the bins in order."""
    lines = [f"{title}: mean, std and count per share of the image the mask opens", f"  {'group':>10s} {'mean':>10s} {'std':>10s} {'count':>6s}"]
    for (_, name), v in results.items():
        lines.append(f"  {name:>10s} {v['mean']:10.6f} {v['std']:10.6f} {v.get('count', 0):6d}")
    return "\n".join(lines)


def results_json(results):
    """{"ssim": {"total": {...}, "0-10%": {...}}}: the dictionary with its tuple keys nested, floats as Python floats."""
    out = {}
    for (score_name, name), v in results.items():
        out.setdefault(score_name, {})[name] = {k: (int(x) if k == "count" else float(x)) for k, x in v.items()}
    return out
