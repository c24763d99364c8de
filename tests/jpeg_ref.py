"""NumPy restatement of the device's baseline JPEG encoder (csrc/jpeg.hip): 4:2:0, 16x16 MCUs in raster
order, integer colour conversion, integer forward DCT on a 2^14-scaled table, round-half-away quantisation, the four
typical Huffman tables of Annex K.3, restart intervals.  Everything is integer arithmetic, so the device has to agree
bit for bit.  Also the host side of a file (the header segments), written independently of acimg/jpeg.py, and the PSNR
helpers of the comparison against libjpeg."""
import struct

import numpy as np

# ---- the standard's data (ITU-T T.81 Annex K) -------------------------------------------------------------------------
LUMA_Q = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                   14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                   49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99], np.int64)
CHROMA_Q = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                     47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32, np.int64)
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,
                   7, 14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31,
                   39, 46, 53, 60, 61, 54, 47, 55, 62, 63])            # zig-zag position -> natural (row-major) index
DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32,
    0x81, 0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16,
    0x17, 0x18, 0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45,
    0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69,
    0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94,
    0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6,
    0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8,
    0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81,
    0x08, 0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34,
    0xE1, 0x25, 0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44,
    0x45, 0x46, 0x47, 0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68,
    0x69, 0x6A, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92,
    0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4,
    0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6,
    0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4, 0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8,
    0xF9, 0xFA]

BLOCK_BITS = 22 + 63 * 26          # most bits one block can take: DC code 11 + 11 bits, 63 x (16-bit code + 10 bits)
MCU_BYTES = 6 * BLOCK_BITS // 8    # 1245, exactly


def huffman_codes(bits, vals):
    """Annex C: symbol -> (code, length)"""
    table, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            table[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return table


DC_TABLES = (huffman_codes(DC_LUMA_BITS, DC_VALS), huffman_codes(DC_CHROMA_BITS, DC_VALS))
AC_TABLES = (huffman_codes(AC_LUMA_BITS, AC_LUMA_VALS), huffman_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))


def quant_tables(quality):
    """[2,64] natural order, luma then chroma: (base * s + 50) / 100 clamped to 1..255"""
    q = int(quality)
    if not 1 <= q <= 100:
        raise ValueError("quality is 1..100")
    s = 5000 // q if q < 50 else 200 - 2 * q
    return np.stack([np.clip((b * s + 50) // 100, 1, 255) for b in (LUMA_Q, CHROMA_Q)]).astype(np.uint8)


def dct_table():
    """T = rint(2^14 A), A the orthonormal DCT-II matrix, int64 [u][x]"""
    u, x = np.arange(8).reshape(8, 1), np.arange(8).reshape(1, 8)
    a = 0.5 * np.cos((2 * x + 1) * u * np.pi / 16)
    a[0, :] = np.sqrt(1.0 / 8.0)
    return np.rint(16384.0 * a).astype(np.int64)


def mcu_grid(H, W):
    return -(-H // 16), -(-W // 16)          # mcu_h, mcu_w


def num_intervals(H, W, restart_mcus):
    mh, mw = mcu_grid(H, W)
    return -(-(mh * mw) // restart_mcus)


def scan_capacity(H, W, restart_mcus):
    mh, mw = mcu_grid(H, W)
    return 2 * MCU_BYTES * mh * mw + 4 * num_intervals(H, W, restart_mcus)


def planes(rgb):
    """[H,W,3] uint8 -> Y, Cb, Cr int64 planes on the MCU grid (last column / row replicated), chroma at half size"""
    H, W = rgb.shape[:2]
    mh, mw = mcu_grid(H, W)
    ext = np.pad(rgb, ((0, mh * 16 - H), (0, mw * 16 - W), (0, 0)), mode="edge").astype(np.int64)
    R, G, B = ext[..., 0], ext[..., 1], ext[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = np.clip(((-11059 * R - 21709 * G + 32768 * B + 32767) >> 16) + 128, 0, 255)
    Cr = np.clip(((32768 * R - 27439 * G - 5329 * B + 32767) >> 16) + 128, 0, 255)

    def half(p):
        # 2x2 mean; the rounding term alternates 1, 2 along a row of chroma samples, so that it does not lift the mean
        s = p[0::2, 0::2] + p[0::2, 1::2] + p[1::2, 0::2] + p[1::2, 1::2]
        return (s + 1 + (np.arange(s.shape[1]) & 1).reshape(1, -1)) >> 2
    return Y, half(Cb), half(Cr)


def blocks(rgb, qtables):
    """[H,W,3] uint8, qtables [2,64] -> int16 [mcus,6,64] quantised coefficients in zig-zag order"""
    H, W = rgb.shape[:2]
    mh, mw = mcu_grid(H, W)
    Y, Cb, Cr = planes(rgb)
    yb = Y.reshape(mh, 2, 8, mw, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(mh * mw, 4, 8, 8)
    cb = Cb.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 1, 8, 8)
    cr = Cr.reshape(mh, 8, mw, 8).transpose(0, 2, 1, 3).reshape(mh * mw, 1, 8, 8)
    s = np.concatenate([yb, cb, cr], 1) - 128                                  # [mcus, 6, y, x]
    T = dct_table()
    p = np.einsum("ux,mbyx->mbyu", T, s)
    assert np.abs(p).max() <= 1 << 23
    p = (p + 256) >> 9
    q = np.einsum("vy,mbyu->mbvu", T, p)
    assert np.abs(q).max() < 1 << 30
    qt = np.asarray(qtables, np.int64).reshape(2, 64)
    d = np.stack([qt[0]] * 4 + [qt[1]] * 2).reshape(1, 6, 8, 8) << 19
    c = np.sign(q) * ((np.abs(q) + (d >> 1)) // d)
    c = c.reshape(mh * mw, 6, 64)
    c[:, :, 1:] = np.clip(c[:, :, 1:], -1023, 1023)
    return c[:, :, ZIGZAG].astype(np.int16)


class BitWriter(object):
    """MSB-first bits into bytes, 0x00 stuffed after every 0xFF"""

    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            b = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def pad(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


def _magnitude(v):
    size = int(abs(v)).bit_length()
    return size, (v if v >= 0 else v + (1 << size) - 1)


def encode_block(w, zz, pred, comp):
    """one block's 64 zig-zag coefficients; returns its DC value (the next predictor)"""
    dc = int(zz[0])
    size, bits = _magnitude(dc - pred)
    w.put(*DC_TABLES[comp][size])
    if size:
        w.put(bits, size)
    ac, run = AC_TABLES[comp], 0
    last = 0
    for k in np.flatnonzero(zz[1:]) + 1:
        run = int(k) - last - 1
        while run > 15:
            w.put(*ac[0xF0])
            run -= 16
        size, bits = _magnitude(int(zz[k]))
        w.put(*ac[(run << 4) | size])
        w.put(bits, size)
        last = int(k)
    if last != 63:
        w.put(*ac[0x00])
    return dc


def scan(coef, restart_mcus):
    """int16 [mcus,6,64] -> the bytes between the SOS header and EOI: intervals padded with 1-bits, RSTm between them"""
    mcus = coef.shape[0]
    out = bytearray()
    for j, m0 in enumerate(range(0, mcus, restart_mcus)):
        if j:
            out += bytes([0xFF, 0xD0 + ((j - 1) & 7)])
        w, pred = BitWriter(), [0, 0, 0]
        for m in range(m0, min(m0 + restart_mcus, mcus)):
            for b in range(6):
                c = 0 if b < 4 else b - 3
                pred[c] = encode_block(w, coef[m, b], pred[c], 0 if b < 4 else 1)
        w.pad()
        out += w.out
    return bytes(out)


def synthetic_coefficients(n, mcus, full):
    """int16 [n,mcus,6,64] whose blocks walk through every path of the coder; full: the capacity case"""
    c = np.zeros((n, mcus, 6, 64), np.int16)
    if full:
        c[..., 1:] = 1023
        c[..., 1::2] = -1023                                  # every AC at +-1023: 16-bit codes, ten bits each
        flat = c.reshape(-1, 64)
        flat[0::2, 0], flat[1::2, 0] = -1024, 1016            # category-11 differences
        return c
    rng = np.random.RandomState(n * 100 + mcus)
    flat = c.reshape(-1, 64)
    for b in range(flat.shape[0]):
        kind = b % 7
        if kind == 1:
            flat[b, 63] = 1 if b % 2 else -1                  # three ZRL, no EOB
        elif kind == 2:
            flat[b, 0], flat[b, 16] = 5, -3                   # a run of exactly 15 zeros
        elif kind == 3:
            flat[b, 0], flat[b, 17] = -7, 1023                # 16: one ZRL, then run 0
        elif kind == 4:
            flat[b, 1], flat[b, 34] = -1023, 2                # 32: two ZRL
        elif kind == 5:
            k = rng.randint(1, 64, size=6)
            flat[b, k] = rng.randint(-40, 41, size=6)
            flat[b, 0] = rng.randint(-1024, 1017)
        elif kind == 6:
            flat[b] = rng.randint(-3, 4, size=64)
        # kind 0: all zeros, EOB only
    return c


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def header(H, W, qtables, restart_mcus):
    """SOI, APP0 (JFIF 1.01, no density unit, 1:1), two DQT, SOF0 (2x2 / 1x1 / 1x1), four DHT, DRI, SOS"""
    qt = np.asarray(qtables, np.uint8).reshape(2, 64)
    h = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for i in range(2):
        h += _segment(0xDB, bytes([i]) + qt[i][ZIGZAG].tobytes())
    h += _segment(0xC0, struct.pack(">BHHB", 8, H, W, 3) + bytes([1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        h += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    h += _segment(0xDD, struct.pack(">H", restart_mcus))
    h += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return h


def default_restart(W):
    return -(-W // 16)                   # one MCU row


ENCODER_SCANS = [(H, W, full) for (H, W) in ((16, 16), (72, 40)) for full in (False, True)]


def encoder_files(H, W, full):
    """complete 4:2:0 files around the scans that this restatement of the ENCODER (`scan`) writes of synthetic coefficient
    arrays, at restart intervals 0 (none), 1 and the default of one MCU row -> (files, int16 [3][mcus][6][64] in NATURAL
    order: what a decoder must give back).  full: every AC at +-1023, DC differences of category 11 - outside what a forward
    DCT gives, so only the entropy stage is asked about them."""
    mh, mw = mcu_grid(H, W)
    coef = synthetic_coefficients(3, mh * mw, full)
    qt = quant_tables(90)
    files = [header(H, W, qt, r) + scan(coef[i], r if r else mh * mw) + b"\xFF\xD9"
             for i, r in enumerate((0, 1, default_restart(W)))]
    natural = np.zeros_like(coef)
    natural[..., ZIGZAG] = coef
    return files, natural


def encode(rgb, quality=90, restart_mcus=None):
    """[H,W,3] uint8 -> a complete JFIF file"""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3
    H, W = rgb.shape[:2]
    r = default_restart(W) if restart_mcus is None else int(restart_mcus)
    qt = quant_tables(quality)
    return header(H, W, qt, r) + scan(blocks(rgb, qt), r) + b"\xFF\xD9"


def psnr(a, b):
    d = np.asarray(a, np.float64) - np.asarray(b, np.float64)
    mse = float((d * d).mean())
    return float("inf") if mse == 0 else 10.0 * np.log10(255.0 * 255.0 / mse)


# ---- the inputs and the decoder side of the comparison against libjpeg (tests/test_video_cpu.py, test_video_gpu.py) ----
def smooth_image(H=224, W=298):
    yy, xx = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 100 * np.sin(xx / 40.0) * np.cos(yy / 30.0), 128 + 80 * np.cos(xx / 25.0), 100 + 0.4 * yy], -1)
    return img.clip(0, 255).astype(np.uint8)


def overlay_image(table_gray, table_jet, seed=3):
    """a jet energy map at alpha 0.7 over a grey noise frame, as `python -m acimg.show` renders it (tests/render_ref.py)"""
    import render_ref
    frame = np.random.RandomState(seed).rand(224, 298, 3).astype(np.float32)
    energy = np.outer(np.hanning(36), np.hanning(48)).astype(np.float32)
    return render_ref.render(frame, energy, table_gray, table_jet)


def noise_image(H, W, seed):
    return np.random.RandomState(seed).randint(0, 256, size=(H, W, 3)).astype(np.uint8)


def pil_decode(data):
    import io

    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def pil_encode(rgb, qtables):
    """libjpeg's own file of `rgb` at the same two quantisation tables (natural order), 4:2:0"""
    import io

    from PIL import Image
    bio = io.BytesIO()
    qt = np.asarray(qtables).reshape(2, 64)
    Image.fromarray(rgb).save(bio, "JPEG", qtables=[[int(v) for v in qt[i]] for i in range(2)], subsampling=2)
    return bio.getvalue()


MARGIN_DB = 0.1          # ours may lie this far below libjpeg's PSNR, no further


def psnr_pair(rgb, ours, quality):
    """(PSNR of our file, PSNR of libjpeg's file at the same tables), both decoded by libjpeg, against the source"""
    return psnr(pil_decode(ours), rgb), psnr(pil_decode(pil_encode(rgb, quant_tables(quality))), rgb)
