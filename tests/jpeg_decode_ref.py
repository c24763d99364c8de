"""The NumPy restatement of the baseline JPEG decoder (csrc/jpeg_decode.hip, acimg/jpeg.py), stage by stage and written
independently of both: its own marker walk, its own Huffman tables, a SEQUENTIAL walk of the scan that meets every RSTn
marker where the stream puts it (the device finds them with a byte search instead), libjpeg's `jpeg_idct_islow` in 32-bit
integers, libjpeg's fancy upsampling and its 16-bit fixed-point colour conversion.  DESIGN section 8 has the definition;
tests/golden/jpeg_decode_golden.npz holds what Pillow (libjpeg-turbo) makes of the same files.

    info = parse_stream(data)                      geometry, tables, where the scan lies
    coef, status, offsets = entropy(info)   int16 [mcus][blocks][64] in NATURAL order, 0 / STATUS_*, interval offsets
    planes = idct(info, coef)               [uint8 plane per component], padded to the MCU grid
    bgr = colour(info, planes)              uint8 [H][W][3], B G R
"""
import struct

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14,
                   21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53,
                   60, 61, 54, 47, 55, 62, 63])
STATUS_OK, STATUS_BAD_CODE, STATUS_RUN, STATUS_EARLY_END = 0, 1, 2, 3


class Info(object):
    pass


def parse_stream(data):
    """the header segments of a baseline file this project decodes (no refusals here: the fixture holds such files only)"""
    data = bytes(data)
    assert data[:2] == b"\xFF\xD8"
    info = Info()
    info.data, info.restart = data, 0
    qt, huff = {}, {}
    pos = 2
    while True:
        assert data[pos] == 0xFF
        marker = data[pos + 1]
        length = struct.unpack_from(">H", data, pos + 2)[0]
        body = data[pos + 4:pos + 2 + length]
        if marker == 0xDB:
            at = 0
            while at < len(body):
                assert body[at] >> 4 == 0
                t = np.zeros(64, np.int64)
                t[ZIGZAG] = np.frombuffer(body[at + 1:at + 65], np.uint8)
                qt[body[at] & 15] = t
                at += 65
        elif marker == 0xC4:
            at = 0
            while at < len(body):
                counts = list(body[at + 1:at + 17])
                n = sum(counts)
                huff[body[at]] = (counts, list(body[at + 17:at + 17 + n]))
                at += 17 + n
        elif marker == 0xC0:
            assert body[0] == 8
            info.height, info.width, info.comps = struct.unpack_from(">HHB", body, 1)
            frame = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(info.comps)]
        elif marker == 0xDD:
            info.restart = struct.unpack_from(">H", body)[0]
        elif marker == 0xDA:
            assert body[0] == info.comps
            sel = {body[1 + 2 * i]: (body[2 + 2 * i] >> 4, body[2 + 2 * i] & 15) for i in range(info.comps)}
            info.scan_begin = pos + 2 + length
            break
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, hex(marker)
        pos += 2 + length
    if info.comps == 1:                      # a one-component scan is not interleaved: 8 x 8 MCUs whatever the factors say
        frame = [(frame[0][0], 1, 1, frame[0][3])]
    info.hs, info.vs = frame[0][1], frame[0][2]
    assert all(f[1:3] == (1, 1) for f in frame[1:])
    info.sampling = [(f[1], f[2]) for f in frame]
    info.quant = [qt[f[3]] for f in frame]
    info.dc = [lookup16(*huff[sel[f[0]][0]]) for f in frame]
    info.ac = [lookup16(*huff[0x10 | sel[f[0]][1]]) for f in frame]
    info.mcu_w = -(-info.width // (8 * info.hs))
    info.mcu_h = -(-info.height // (8 * info.vs))
    info.mcus = info.mcu_w * info.mcu_h
    info.blocks = sum(h * v for h, v in info.sampling)
    return info


def lookup16(counts, vals):
    """Annex C codes -> uint16 [65536]: (length << 8) | symbol for the 16 bits that follow, 0 where no code matches"""
    table = np.zeros(65536, np.uint16)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(counts[length - 1]):
            table[code << (16 - length):(code + 1) << (16 - length)] = (length << 8) | vals[k]
            code += 1
            k += 1
        code <<= 1
    return table


class Bits(object):
    """MSB-first bits of data[pos:end] with FF 00 un-stuffed; any other FF xx ends the data, zeros follow"""

    def __init__(self, data, pos, end):
        self.data, self.pos, self.end, self.start = data, pos, end, pos
        self.acc, self.n, self.used = 0, 0, 0
        self.after = []                                  # per real byte taken in: the position behind it

    def _fill(self, need):
        while self.n < need:
            byte, p = 0, self.pos
            if p < self.end and not (self.data[p] == 0xFF and (p + 1 >= self.end or self.data[p + 1] != 0)):
                byte = self.data[p]
                self.pos += 2 if byte == 0xFF else 1
                self.after.append(self.pos)
            self.acc = ((self.acc << 8) | byte) & ((1 << 64) - 1)
            self.n += 8

    def peek16(self):
        self._fill(16)
        return (self.acc >> (self.n - 16)) & 0xFFFF

    def skip(self, k):
        self.n -= k
        self.used += k

    def take(self, k):
        if k == 0:
            return 0
        self._fill(k)
        self.skip(k)
        return (self.acc >> self.n) & ((1 << k) - 1)

    def overrun(self):
        """more bits used than the data holds"""
        return self.used > 8 * len(self.after)

    def align(self):
        """the position behind the byte that holds the last used bit"""
        return self.after[(self.used + 7) // 8 - 1] if self.used else self.start


def extend(v, s):
    return v - (1 << s) + 1 if s and v < (1 << (s - 1)) else v


def entropy(info, end=None, reached=None):
    """walk the scan MCU by MCU -> (coef int16 [mcus][blocks][64] natural order, status, [offset of each interval's first
    byte from the scan's start]); after a nonzero status the rest of the image is zero.  reached: a dict that receives the
    largest DC category, AC size, DC and AC code length and |DC|, |AC| coefficient that the walk decoded"""
    seen = dict(dc_category=0, ac_size=0, dc_code_bits=0, ac_code_bits=0, dc_abs=0, ac_abs=0)

    def note(key, value):
        seen[key] = max(seen[key], value)
    data = info.data
    end = len(data) if end is None else end
    coef = np.zeros((info.mcus, info.blocks, 64), np.int16)
    comp_of_block = [c for c, (h, v) in enumerate(info.sampling) for _ in range(h * v)]
    pos, offsets = info.scan_begin, [0]
    interval = info.restart if info.restart else info.mcus
    zz = ZIGZAG.tolist()
    for first in range(0, info.mcus, interval):
        if first:
            assert data[pos] == 0xFF and data[pos + 1] == 0xD0 + ((first // interval - 1) & 7), "RST marker expected"
            pos += 2
            offsets.append(pos - info.scan_begin)
        bits = Bits(data, pos, end)
        pred = [0] * info.comps
        for m in range(first, min(first + interval, info.mcus)):
            for b, c in enumerate(comp_of_block):
                e = int(info.dc[c][bits.peek16()])
                if e == 0:
                    return coef, STATUS_BAD_CODE, offsets
                bits.skip(e >> 8)
                s = e & 255
                note("dc_code_bits", e >> 8)
                note("dc_category", s)
                pred[c] += extend(bits.take(s), s)
                if bits.overrun():
                    return coef, STATUS_EARLY_END, offsets
                block = [0] * 64
                block[0] = ((pred[c] + 32768) & 0xFFFF) - 32768
                k = 1
                while k < 64:
                    e = int(info.ac[c][bits.peek16()])
                    if e == 0:
                        return coef, STATUS_BAD_CODE, offsets
                    bits.skip(e >> 8)
                    r, s = (e >> 4) & 15, e & 15
                    note("ac_code_bits", e >> 8)
                    note("ac_size", s)
                    if s:
                        k += r
                        if k > 63:
                            return coef, STATUS_RUN, offsets
                        block[zz[k]] = extend(bits.take(s), s)
                        k += 1
                    elif r == 15:
                        k += 16
                    else:
                        break
                    if bits.overrun():
                        return coef, STATUS_EARLY_END, offsets
                if bits.overrun():
                    return coef, STATUS_EARLY_END, offsets
                coef[m, b] = block
                note("dc_abs", abs(block[0]))
                note("ac_abs", max(abs(v) for v in block[1:]))
                if reached is not None:
                    reached.update(seen)
        pos = bits.align()
    return coef, STATUS_OK, offsets


# ---- jpeg_idct_islow -------------------------------------------------------------------------------------------------------
F_0_298, F_0_390, F_0_541, F_0_765, F_0_899, F_1_175 = 2446, 3196, 4433, 6270, 7373, 9633
F_1_501, F_1_847, F_1_961, F_2_053, F_2_562, F_3_072 = 12299, 15137, 16069, 16819, 20995, 25172


def _wrap32(a):
    return ((a + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _pass(x, shift, first):
    """the butterfly along the LAST axis of int64 [..., 8]; results wrapped to int32 before the descale"""
    x0, x1, x2, x3, x4, x5, x6, x7 = [x[..., i] for i in range(8)]
    z1 = (x2 + x6) * F_0_541
    tmp2 = z1 + x6 * -F_1_847
    tmp3 = z1 + x2 * F_0_765
    tmp0 = (x0 + x4) << 13
    tmp1 = (x0 - x4) << 13
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    t0, t1, t2, t3 = x7, x5, x3, x1
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * F_1_175
    t0, t1, t2, t3 = t0 * F_0_298, t1 * F_2_053, t2 * F_3_072, t3 * F_1_501
    z1, z2, z3, z4 = z1 * -F_0_899, z2 * -F_2_562, z3 * -F_1_961 + z5, z4 * -F_0_390 + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)
    return (_wrap32(out) + (1 << (shift - 1))) >> shift


def idct_blocks(coef, quant):
    """int16 [...][64] natural order, quant int [64] -> uint8 [...][8][8]"""
    x = _wrap32(coef.astype(np.int64) * quant.astype(np.int64)).reshape(coef.shape[:-1] + (8, 8))
    cols = _pass(np.swapaxes(x, -1, -2), 11, True)          # columns first: [.., column, v] -> [.., column, y]
    rows = _pass(np.swapaxes(cols, -1, -2), 18, False)      # [.., y, u] -> [.., y, x]
    return np.clip(rows + 128, 0, 255).astype(np.uint8)


def idct(info, coef):
    """-> one uint8 plane per component, (mcu_h * v * 8) x (mcu_w * h * 8)"""
    planes, b0 = [], 0
    for c, (h, v) in enumerate(info.sampling):
        px = idct_blocks(coef[:, b0:b0 + h * v], info.quant[c])                       # [mcus][h*v][8][8]
        px = px.reshape(info.mcu_h, info.mcu_w, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5)   # my, by, y, mx, bx, x
        planes.append(np.ascontiguousarray(px.reshape(info.mcu_h * v * 8, info.mcu_w * h * 8)))
        b0 += h * v
    return planes


# ---- fancy upsampling and colour ---------------------------------------------------------------------------------------------
def upsample_h2v1(a, width):
    a = a.astype(np.int64)
    left = np.concatenate([a[:, :1], a[:, :-1]], 1)
    right = np.concatenate([a[:, 1:], a[:, -1:]], 1)
    out = np.empty((a.shape[0], 2 * a.shape[1]), np.int64)
    out[:, 0::2] = (3 * a + left + 1) >> 2
    out[:, 1::2] = (3 * a + right + 2) >> 2
    out[:, 0], out[:, -1] = a[:, 0], a[:, -1]
    return out[:, :width]


def upsample_h2v2(a, height, width):
    a = a.astype(np.int64)
    above = np.concatenate([a[:1], a[:-1]], 0)
    below = np.concatenate([a[1:], a[-1:]], 0)
    s = np.empty((2 * a.shape[0], a.shape[1]), np.int64)
    s[0::2] = 3 * a + above
    s[1::2] = 3 * a + below
    left = np.concatenate([s[:, :1], s[:, :-1]], 1)
    right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
    out = np.empty((s.shape[0], 2 * s.shape[1]), np.int64)
    out[:, 0::2] = (3 * s + left + 8) >> 4
    out[:, 1::2] = (3 * s + right + 7) >> 4
    return out[:height, :width]


def colour(info, planes):
    H, W = info.height, info.width
    y = planes[0][:H, :W].astype(np.int64)
    if info.comps == 1:
        return np.repeat(y[..., None], 3, 2).astype(np.uint8)
    cw, ch = -(-W // info.hs), -(-H // info.vs)
    chroma = []
    for p in planes[1:]:
        p = p[:ch, :cw]
        if (info.hs, info.vs) == (2, 2):
            p = upsample_h2v2(p, H, W)
        elif (info.hs, info.vs) == (2, 1):
            p = upsample_h2v1(p, W)
        chroma.append(p.astype(np.int64) - 128)
    cb, cr = chroma
    r = y + ((91881 * cr + 32768) >> 16)
    b = y + ((116130 * cb + 32768) >> 16)
    g = y + ((-22554 * cb - 46802 * cr + 32768) >> 16)
    return np.clip(np.stack([b, g, r], -1), 0, 255).astype(np.uint8)


def decode(data):
    """a whole file -> uint8 [H][W][3] in B, G, R order"""
    info = parse_stream(data)
    coef, status, _ = entropy(info)
    assert status == STATUS_OK, status
    return colour(info, idct(info, coef))


# ---- the fixture and streams derived from it --------------------------------------------------------------------------------
GOLDEN_FILES = ("jpeg_decode_golden.npz", "jpeg_decode_extreme_golden.npz")       # mild inputs; full-swing inputs


def load_golden(files=GOLDEN_FILES):
    """tests/golden/jpeg_decode_golden.npz and jpeg_decode_extreme_golden.npz -> {name: (file bytes, Pillow's pixels as uint8
    [H][W][3] B G R)}, in file order"""
    import collections
    import os
    out = collections.OrderedDict()
    for f in files:
        z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f))
        for name in z["names"].tolist():
            assert name not in out, name
            px = z["pixels_" + name]
            bgr = px[::-1].transpose(1, 2, 0) if px.ndim == 3 else np.repeat(px[..., None], 3, 2)
            bgr = np.ascontiguousarray(bgr)
            bgr.setflags(write=False)
            out[name] = (z["jpeg_" + name].tobytes(), bgr)
    return out


def payload_offset(data, marker):
    """offset of the payload of the first segment FF `marker` in front of the scan"""
    pos = 2
    while True:
        m, length = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        if m == marker:
            return pos + 4
        assert m != 0xDA, "no segment FF %02X" % marker
        pos += 2 + length


def patched(data, offset, value):
    return data[:offset] + bytes((value,)) + data[offset + 1:]


def as_progressive(data):
    """the same bytes under an SOF2 marker: what a progressive file looks like to a parser"""
    return patched(data, payload_offset(data, 0xC0) - 3, 0xC2)
