"""Wire / disk formats either side of the sampling path: checkpoints in, images and FID statistics out.

Host-side only; nothing here touches the GPU path.  Reference behaviour followed, with file:line:

* checkpoints   ``model_{epoch}.pth`` = flat ``state_dict`` of an accelerate/DDP-wrapped model, every key prefixed ``module.``
                (train_flow_latent.py:211-214, stripped unconditionally at test_flow_latent.py:140-141);
                ``content.pth`` = dict(epoch, global_step, args, model_dict, optimizer, scheduler) (train_flow_latent.py:196-203).
* images        single-process script: ``torchvision.utils.save_image`` = ``mul(255).add_(0.5).clamp_(0, 255).to(uint8)`` (ROUNDING),
                per-image JPEGs (test_flow_latent.py:269) or one nrow=8, padding=0 grid (:297);
                DDP script: ``clamp((x + 1) / 2, 0, 1) * 255 -> uint8`` (TRUNCATION) (test_flow_latent_ddp.py:131-139).
                Both end in ``PIL.Image.save(path)`` with PIL's default JPEG settings.
* FID           ``.npy`` / ``.npz`` statistics with the two layouts accepted at pytorch_fid/fid_score.py:254-260, activation statistics
                (:228-246) and the Frechet distance incl. its eps and imaginary-part rules (:177-225).  The Inception feature extractor
                itself needs torchvision + downloaded weights and is not available offline.
"""
import os

import numpy as np
import torch


# ------------------------------------------------------------------ checkpoints
def extract_state_dict(obj):
    """Flat, prefix-free state_dict from any checkpoint object the reference writes."""
    if isinstance(obj, dict) and "model_dict" in obj and isinstance(obj["model_dict"], dict):
        obj = obj["model_dict"]  # content.pth
    if not isinstance(obj, dict) or not obj or not all(isinstance(k, str) for k in obj):
        raise ValueError("not a state_dict / content.pth object")
    if not all(torch.is_tensor(v) for v in obj.values()):
        raise ValueError("checkpoint dict holds non-tensor values and no 'model_dict' entry")
    # the reference strips 7 characters from EVERY key; strip only a real 'module.' prefix
    return {(k[7:] if k.startswith("module.") else k): v for k, v in obj.items()}


def load_state_dict_file(path, map_location="cpu", trust_checkpoint=False):
    """Read ``model_{epoch}.pth`` / ``content.pth`` with the SAFE unpickler only.  ``content.pth`` pickles an ``argparse.Namespace``
    next to the tensors (train_flow_latent.py:196-203): that one class is allow-listed; anything else the safe loader rejects stays
    rejected (a file the safe loader refuses is exactly the file that must not reach the full unpickler), unless the caller passes
    ``trust_checkpoint=True`` explicitly (``--trust_checkpoint``), which is logged."""
    import argparse

    if trust_checkpoint:
        import warnings

        warnings.warn(f"loading {path} with the full (unsafe) unpickler because trust_checkpoint=True", stacklevel=2)
        return extract_state_dict(torch.load(path, map_location=map_location, weights_only=False))
    with torch.serialization.safe_globals([argparse.Namespace]):
        obj = torch.load(path, map_location=map_location, weights_only=True)
    return extract_state_dict(obj)


# ------------------------------------------------------------------ images
def to_uint8_rounding(img01):
    """torchvision.utils.save_image's conversion of a [0,1] float image tensor [...,C,H,W] -> uint8 [...,H,W,C]."""
    x = img01.detach().to("cpu", torch.float32)
    x = x.mul(255).add_(0.5).clamp_(0, 255)
    return x.movedim(-3, -1).to(torch.uint8)


def to_uint8_truncating(img_pm1):
    """test_flow_latent_ddp.py:131-135 on a [-1,1] image tensor [...,C,H,W] -> uint8 [...,H,W,C] (what lfm_images_to_uint8 does on the GPU)."""
    x = img_pm1.detach().to("cpu", torch.float32)
    x = torch.clamp((x + 1.0) / 2.0, 0, 1) * 255
    return x.movedim(-3, -1).to(torch.uint8)


def make_grid_nhwc(img_u8, nrow=8, padding=0):
    """Tile [N,H,W,C] uint8 images row-major, ``nrow`` per row, like torchvision.utils.make_grid(padding=0) does for the sample sheet."""
    if padding != 0:
        raise NotImplementedError("the reference only uses padding=0")
    n, h, w, c = img_u8.shape
    cols = min(nrow, n)
    rows = (n + cols - 1) // cols
    grid = torch.zeros(rows * h, cols * w, c, dtype=torch.uint8)
    for k in range(n):
        r, q = divmod(k, cols)
        grid[r * h:(r + 1) * h, q * w:(q + 1) * w] = img_u8[k]
    return grid


def save_jpeg(hwc_u8, path):
    from PIL import Image

    a = hwc_u8.cpu().numpy() if torch.is_tensor(hwc_u8) else np.asarray(hwc_u8)
    Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a).save(path)


def save_image_grid(img01, path, nrow=8, padding=0):
    """torchvision.utils.save_image(fake_image, path, padding=0, nrow=8) (test_flow_latent.py:297)."""
    save_jpeg(make_grid_nhwc(to_uint8_rounding(img01), nrow=nrow, padding=padding), path)


def save_indexed_jpegs(img_u8_nhwc, save_dir, start_index, world_size=1, rank=0):
    """One JPEG per image named by the reference's global index ``j * world + rank + total`` (test_flow_latent_ddp.py:138)."""
    os.makedirs(save_dir, exist_ok=True)
    for j in range(img_u8_nhwc.shape[0]):
        save_jpeg(img_u8_nhwc[j], os.path.join(save_dir, f"{j * world_size + rank + start_index}.jpg"))


# ------------------------------------------------------------------ JPEG on the device (DESIGN.md section "JPEG encode"): the header, the tables, the writers
# ITU-T T.81 Annex K: the two base quantisation tables (K.1, K.2; natural order), the zig-zag scan and the four Huffman specifications (K.3-K.6: sixteen code
# counts, then the symbols) that libjpeg, and so Pillow, uses by default.  lfm_amd/csrc/jpeg_encode.h holds the same tables for the kernels.
JPEG_QUANT_BASE = (
    (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99),
    (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99) + (99,) * 32)
JPEG_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
               35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
JPEG_HUFFMAN = {  # (class: 0 DC / 1 AC, table id: 0 luminance / 1 chrominance) -> counts[16] + symbols
    (0, 0): bytes.fromhex("00010501010101010100000000000000" "000102030405060708090a0b"),
    (1, 0): bytes.fromhex("0002010303020403050504040000017d"
                          "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
                          "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
                          "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"),
    (0, 1): bytes.fromhex("00030101010101010101010000000000" "000102030405060708090a0b"),
    (1, 1): bytes.fromhex("00020102040403040705040400010277"
                          "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a"
                          "434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aa"
                          "b2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"),
}


def jpeg_quant_tables(quality):
    """libjpeg's jpeg_set_quality(quality, force_baseline=TRUE): the two 8-bit tables in natural order."""
    quality = int(quality)
    if not 1 <= quality <= 100:
        raise ValueError(f"JPEG quality {quality} is outside 1..100")
    s = 5000 // quality if quality < 50 else 200 - 2 * quality
    return tuple(tuple(min(max((b * s + 50) // 100, 1), 255) for b in base) for base in JPEG_QUANT_BASE)


def jpeg_header(H, W, quality=75):
    """Everything ``PIL.Image.save(path)`` writes before the entropy-coded data of an RGB ``H x W`` image: SOI, JFIF 1.01 APP0, two DQT, SOF0 (4:2:0), four DHT, SOS."""
    H, W = int(H), int(W)
    if not (1 <= H <= 65535 and 1 <= W <= 65535):
        raise ValueError(f"JPEG size {H}x{W} is outside 1..65535")

    def seg(marker, payload):
        return bytes((0xFF, marker)) + (len(payload) + 2).to_bytes(2, "big") + payload

    out = b"\xff\xd8" + seg(0xE0, b"JFIF\0" + bytes((1, 1, 0, 0, 1, 0, 1, 0, 0)))
    for i, q in enumerate(jpeg_quant_tables(quality)):
        out += seg(0xDB, bytes((i,)) + bytes(q[z] for z in JPEG_ZIGZAG))
    out += seg(0xC0, bytes((8,)) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes((3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for (cls, tid) in ((0, 0), (1, 0), (0, 1), (1, 1)):
        out += seg(0xC4, bytes((cls << 4 | tid,)) + JPEG_HUFFMAN[(cls, tid)])
    return out + seg(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


def _jpeg_bytes_pillow(hwc_u8, quality=75):
    import io

    from PIL import Image

    a = hwc_u8.cpu().numpy() if torch.is_tensor(hwc_u8) else np.asarray(hwc_u8)
    buf = io.BytesIO()
    kw = {} if quality == 75 else {"quality": int(quality)}  # 75 is Pillow's default: save_jpeg's call exactly
    Image.fromarray(a[..., 0] if a.shape[-1] == 1 else a).save(buf, format="JPEG", **kw)
    return buf.getvalue()


def to_uint8_rounding_device(img01):
    """to_uint8_rounding where the tensor lives: the same three fp32 operations element by element, so the same bytes, without moving the floats to the host."""
    x = img01.detach().to(torch.float32)
    x = x.mul(255).add_(0.5).clamp_(0, 255)
    return x.movedim(-3, -1).to(torch.uint8).contiguous()


def begin_jpegs_device(img_u8_nhwc, quality=75, capacity=None):
    """Enqueue the HIP JPEG encoder (hip.jpeg_encode) for a uint8 [N,H,W,3] batch on its device's CURRENT stream and return at once; finish_jpegs_device
    turns the result into files once that stream has got there.  A one-channel or CPU batch has nothing to enqueue: it is kept for Pillow."""
    job = {"images": img_u8_nhwc, "quality": int(quality), "device": None}
    if torch.is_tensor(img_u8_nhwc) and img_u8_nhwc.is_cuda and img_u8_nhwc.dim() == 4 and img_u8_nhwc.shape[-1] == 3 and img_u8_nhwc.shape[0] > 0:
        from . import hip

        job["images"] = img_u8_nhwc = img_u8_nhwc.contiguous()
        job["device"] = hip.jpeg_encode(img_u8_nhwc, quality=quality, capacity=capacity)
    return job


def finish_jpegs_device(job):
    """The whole files of begin_jpegs_device's batch, one ``bytes`` per image.  The caller has made sure the encoder's stream is done, or calls this on that
    stream (the two copies below are ordered on the current stream and wait for it).  Only the lengths and the compressed bytes cross to the host; an image
    whose stream did not fit the capacity is encoded by Pillow, and so is everything of a batch that was kept for it: identical bytes either way."""
    img, quality = job["images"], job["quality"]
    if job["device"] is None:
        return [_jpeg_bytes_pillow(img[j], quality) for j in range(img.shape[0])]
    out, lengths = job["device"]
    cap = out.shape[1]
    lens = lengths.tolist()  # N int32
    head = jpeg_header(img.shape[1], img.shape[2], quality)
    body = out[:, :min(max(lens), cap)].cpu().numpy()  # the compressed bytes, not the capacity
    return [head + body[j, :ln].tobytes() if ln <= cap else _jpeg_bytes_pillow(img[j], quality) for j, ln in enumerate(lens)]


def encode_jpegs_device(img_u8_nhwc, quality=75, capacity=None):
    """Whole JPEG files of a uint8 [N,H,W,3] batch, byte for byte what ``PIL.Image.save`` writes (with ``quality=`` when it is not Pillow's default 75),
    encoded on the tensor's own device: begin_jpegs_device + finish_jpegs_device on the current stream."""
    return finish_jpegs_device(begin_jpegs_device(img_u8_nhwc, quality, capacity))


def write_indexed_files(files, save_dir, start_index, world_size=1, rank=0):
    """Finished JPEG files under save_indexed_jpegs' names: ``j * world + rank + start``.jpg."""
    os.makedirs(save_dir, exist_ok=True)
    for j, data in enumerate(files):
        with open(os.path.join(save_dir, f"{j * world_size + rank + start_index}.jpg"), "wb") as f:
            f.write(data)


def save_indexed_jpegs_device(img_u8_nhwc, save_dir, start_index, world_size=1, rank=0, quality=75):
    """save_indexed_jpegs with the files encoded on the device: the same names, the same bytes; the host's work per image is one write."""
    write_indexed_files(encode_jpegs_device(img_u8_nhwc, quality=quality), save_dir, start_index, world_size, rank)


# ------------------------------------------------------------------ FID statistics
def read_fid_stats(path):
    """(mu, sigma) from a ``.npz`` (keys mu, sigma) or a ``.npy`` holding a pickled dict (fid_score.py:254-260)."""
    f = np.load(path, allow_pickle=True)
    try:
        return f["mu"][:], f["sigma"][:]
    except (IndexError, KeyError, TypeError):
        d = f.item()
        return d["mu"][:], d["sigma"][:]


def activation_statistics(act):
    """fid_score.py:243-246: mean and (unbiased, rowvar=False) covariance of [n, dims] activations."""
    act = np.asarray(act, dtype=np.float64)
    return np.mean(act, axis=0), np.cov(act, rowvar=False)


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """fid_score.py:177-225, same order of operations (sqrtm of the product, eps retry, imaginary-part tolerance 1e-3)."""
    from scipy import linalg

    mu1, mu2 = np.atleast_1d(mu1), np.atleast_1d(mu2)
    sigma1, sigma2 = np.atleast_2d(sigma1), np.atleast_2d(sigma2)
    if mu1.shape != mu2.shape:
        raise ValueError("Training and test mean vectors have different lengths")
    if sigma1.shape != sigma2.shape:
        raise ValueError("Training and test covariances have different dimensions")
    diff = mu1 - mu2
    covmean = linalg.sqrtm(sigma1.dot(sigma2))
    if isinstance(covmean, tuple):  # older scipy returns (sqrtm, errest) with disp=False only; keep robust
        covmean = covmean[0]
    if not np.isfinite(covmean).all():
        offset = np.eye(sigma1.shape[0]) * eps
        covmean = linalg.sqrtm((sigma1 + offset).dot(sigma2 + offset))
    if np.iscomplexobj(covmean):
        if not np.allclose(np.diagonal(covmean).imag, 0, atol=1e-3):
            raise ValueError("Imaginary component {}".format(np.max(np.abs(covmean.imag))))
        covmean = covmean.real
    return diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2 * np.trace(covmean)
