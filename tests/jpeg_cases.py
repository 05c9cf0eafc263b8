"""The cases of the JPEG tests and a plain numpy restatement of the encoder's arithmetic ("JPEG encode"): integer colour conversion, 4:2:0
down-sampling, libjpeg's jfdctint, quantisation and the Annex-K Huffman coding, written for reading and not for speed.  test_jpeg_ref.py shows it byte-identical
to Pillow; test_gpu_jpeg_encode.py holds the HIP kernels to Pillow on the same cases.  `mistake` re-introduces one named error at a time."""
import io

import numpy as np

from lfm_amd.io_formats import JPEG_HUFFMAN, JPEG_ZIGZAG, jpeg_quant_tables

SIZES = ((1, 1), (8, 8), (8, 16), (16, 8), (16, 16), (17, 31), (24, 40), (33, 47), (40, 56), (250, 250))
QUALITIES = (1, 10, 50, 75, 90, 95, 100)
FAMILIES = ("noise", "blur", "flat", "saturated", "blur_q10", "noise_q100") + tuple(f"blur_q{q}" for q in QUALITIES if q != 10) + ("noise_q1",)
MISTAKES = ("constant_bias", "rows_before_downsample", "dummy_from_pixels", "quant_floor", "no_stuffing", "zero_padding", "dc_skips_dummy")


def _blur(a):
    a = a.astype(np.float64)
    for _ in range(3):
        for ax in (0, 1):
            a = (a + np.roll(a, 1, ax) + np.roll(a, -1, ax)) / 3.0
    return a


def make_image(family, H, W):
    """-> (uint8 [H, W, 3], quality).  Deterministic: the seed is the family's place in FAMILIES and the size."""
    rng = np.random.default_rng(1000 * FAMILIES.index(family) + 37 * H + W)
    quality = int(family.split("_q")[1]) if "_q" in family else 75
    kind = family.split("_q")[0]
    if kind == "noise":
        img = rng.integers(0, 256, (H, W, 3))
    elif kind == "blur":  # smooth, full range: long zero runs at low quality
        b = _blur(rng.integers(0, 256, (H, W, 3)))
        lo, hi = b.min(), b.max()
        img = np.rint((b - lo) / max(hi - lo, 1e-9) * 255.0)
        # ... except one pixel-level checkerboard block: a lone coefficient at the far end of the zig-zag scan, behind a run of zeros that takes ZRLs
        yy, xx = np.mgrid[0:min(H, 8), 0:min(W, 8)]
        img[:8, :8] = (28 + 200 * ((yy + xx) & 1))[..., None]
    elif kind == "flat":
        img = np.broadcast_to(np.array([90, 160, 200]), (H, W, 3))
    elif kind == "saturated":  # 0 / 255 per channel: large coefficients, long codes, 0xFF bytes in the stream
        img = rng.integers(0, 2, (H, W, 3)) * 255
    else:
        raise ValueError(family)
    return np.ascontiguousarray(img, dtype=np.uint8), quality


def pillow_bytes(img, quality=75):
    from PIL import Image

    buf = io.BytesIO()
    if quality == 75:
        Image.fromarray(img).save(buf, format="JPEG")  # the defaults, as PIL.Image.save(path) of the sample writers
    else:
        Image.fromarray(img).save(buf, format="JPEG", quality=quality)
    return buf.getvalue()


def split_pillow(data):
    """(header up to and including SOS, entropy-coded data + EOI) of a JPEG file, by walking its marker segments."""
    assert data[:2] == b"\xff\xd8"
    i = 2
    while True:
        assert data[i] == 0xFF
        marker, ln = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        i += 2 + ln
        if marker == 0xDA:
            return data[:i], data[i:]


# ------------------------------------------------------------------ the restatement
def _fix(c):
    return int(round(c * 8192))


F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = map(_fix, (0.298631336, 0.390180644, 0.541196100, 0.765366865, 0.899976223, 1.175875602))
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = map(_fix, (1.501321110, 1.847759065, 1.961570560, 2.053119869, 2.562915447, 3.072711026))


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, first):
    """One pass of jfdctint over the LAST axis of int64 [..., 8]."""
    d0, d1, d2, d3, d4, d5, d6, d7 = (d[..., i] for i in range(8))
    t0, t7, t1, t6, t2, t5, t3, t4 = d0 + d7, d0 - d7, d1 + d6, d1 - d6, d2 + d5, d2 - d5, d3 + d4, d3 - d4
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 11 if first else 15
    o = [None] * 8
    if first:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    else:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    z1 = (t12 + t13) * F_0_541
    o[2] = _descale(z1 + t13 * F_0_765, n)
    o[6] = _descale(z1 - t12 * F_1_847, n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * F_1_175
    t4, t5, t6, t7 = t4 * F_0_298, t5 * F_2_053, t6 * F_3_072, t7 * F_1_501
    z1, z2, z3, z4 = -z1 * F_0_899, -z2 * F_2_562, -z3 * F_1_961 + z5, -z4 * F_0_390 + z5
    o[7], o[5], o[3], o[1] = _descale(t4 + z1 + z3, n), _descale(t5 + z2 + z4, n), _descale(t6 + z2 + z3, n), _descale(t7 + z1 + z4, n)
    return np.stack(o, axis=-1)


def fdct_quant(block, q, mistake=None):
    """8x8 samples (0..255) -> 64 quantised coefficients in zig-zag order.  q: the 64 table entries in natural order."""
    d = block.astype(np.int64) - 128
    d = _fdct_pass(d, True)                                  # rows
    d = _fdct_pass(d.swapaxes(0, 1), False).swapaxes(0, 1)   # columns
    t = d.reshape(64)
    div = np.asarray(q, dtype=np.int64) << 3
    if mistake == "quant_floor":
        r = (t + (div >> 1)) // div
    else:
        r = np.sign(t) * ((np.abs(t) + (div >> 1)) // div)
    return r[list(JPEG_ZIGZAG)]


def planes(img, mistake=None):
    """-> (Y [Hp, Wp], Cb [Hp/2, Wp/2], Cr [Hp/2, Wp/2]) as int64, padded as libjpeg pads them."""
    H, W, _ = img.shape
    Hp, Wp = -(-H // 16) * 16, -(-W // 16) * 16
    R, G, B = (img[..., i].astype(np.int64) for i in range(3))
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    Y = np.pad(Y, ((0, Hp - H), (0, Wp - W)), mode="edge")
    He = Hp if mistake == "rows_before_downsample" else H + (H & 1)
    out = [Y]
    for Cc in (Cb, Cr):
        Cc = np.pad(Cc, ((0, He - H), (0, Wp - W)), mode="edge")
        bias = np.ones(Wp // 2, dtype=np.int64) * 2 if mistake == "constant_bias" else 1 + (np.arange(Wp // 2) & 1)
        ds = (Cc[0::2, 0::2] + Cc[0::2, 1::2] + Cc[1::2, 0::2] + Cc[1::2, 1::2] + bias[None, :]) >> 2
        out.append(np.pad(ds, ((0, Hp // 2 - ds.shape[0]), (0, 0)), mode="edge"))
    return out


def coefficients(img, quality=75, mistake=None):
    """-> int64 [blocks, 64] in scan order (per MCU: four Y, Cb, Cr), zig-zag inside, dummy blocks included, and the per-block flag `dummy`."""
    H, W, _ = img.shape
    Y, Cb, Cr = planes(img, mistake)
    ql, qc = jpeg_quant_tables(quality)
    Wr, Hr = -(-W // 8) * 8, -(-H // 8) * 8
    blocks, dummy = [], []
    for my in range(Y.shape[0] // 16):
        for mx in range(Y.shape[1] // 16):
            for k in range(4):
                y0, x0 = my * 16 + 8 * (k >> 1), mx * 16 + 8 * (k & 1)
                if (x0 >= Wr or y0 >= Hr) and mistake != "dummy_from_pixels":
                    c = np.zeros(64, dtype=np.int64)
                    # dc_skips_dummy: with the copied DC a chain that skips the dummy blocks codes the very same differences, so the mistake is stated in
                    # the form in which it shows: dummy blocks left as zero blocks AND left out of the prediction chain
                    c[0] = 0 if mistake == "dc_skips_dummy" else blocks[-1][0]
                    dummy.append(True)
                else:
                    c = fdct_quant(Y[y0:y0 + 8, x0:x0 + 8], ql, mistake)
                    dummy.append(False)
                blocks.append(c)
            for P in (Cb, Cr):
                blocks.append(fdct_quant(P[my * 8:my * 8 + 8, mx * 8:mx * 8 + 8], qc, mistake))
                dummy.append(False)
    return np.stack(blocks), np.array(dummy)


def huffman_codes(spec):
    """counts[16] + symbols -> {symbol: (code, length)} (T.81 Annex C)."""
    counts, syms = spec[:16], spec[16:]
    table, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(counts[ln - 1]):
            table[syms[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return table


def entropy(coef, dummy=None, mistake=None):
    """Scan-order coefficient blocks -> (entropy-coded data with stuffing, padding and EOI, number of ZRL symbols emitted)."""
    dc_t = (huffman_codes(JPEG_HUFFMAN[(0, 0)]), huffman_codes(JPEG_HUFFMAN[(0, 1)]))
    ac_t = (huffman_codes(JPEG_HUFFMAN[(1, 0)]), huffman_codes(JPEG_HUFFMAN[(1, 1)]))
    acc, nbits, zrl = 0, 0, 0
    pred = [0, 0, 0]

    def put(code, ln):
        nonlocal acc, nbits
        acc = (acc << ln) | code
        nbits += ln

    def put_value(v, tab, run):
        s = int(abs(v)).bit_length()
        put(*tab[run << 4 | s])
        if s:
            put((v - 1 if v < 0 else v) & ((1 << s) - 1), s)

    for b in range(coef.shape[0]):
        k = b % 6
        comp = 0 if k < 4 else k - 3
        c = [int(v) for v in coef[b]]
        put_value(c[0] - pred[comp], dc_t[comp > 0], 0)
        if not (mistake == "dc_skips_dummy" and dummy is not None and dummy[b]):
            pred[comp] = c[0]
        run = 0
        for v in c[1:]:
            if v == 0:
                run += 1
                continue
            while run > 15:
                put(*ac_t[comp > 0][0xF0])
                zrl += 1
                run -= 16
            put_value(v, ac_t[comp > 0], run)
            run = 0
        if run:
            put(*ac_t[comp > 0][0x00])
    pad = -nbits % 8
    acc = (acc << pad) | (0 if mistake == "zero_padding" else (1 << pad) - 1)
    raw = acc.to_bytes((nbits + pad) // 8, "big")
    if mistake != "no_stuffing":
        raw = raw.replace(b"\xff", b"\xff\x00")
    return raw + b"\xff\xd9", zrl


def encode_body(img, quality=75, mistake=None):
    """What follows the header in Pillow's file of `img`."""
    coef, dummy = coefficients(img, quality, mistake)
    return entropy(coef, dummy, mistake)[0]
