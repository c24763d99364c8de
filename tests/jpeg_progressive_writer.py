"""Writes a progressive JPEG file (SOF2) from coefficients and an ARBITRARY scan script, with Huffman tables built per scan
from the scan's own statistics (T.81 K.2) and an optional restart interval: the paths of Annex G that Pillow's one script
never takes need a writer of their own, as tests/deflate_writer.py does for DEFLATE.  The four encoding procedures of
Annex G are restated here from the standard; tests/golden/make_jpeg_progressive_golden.py checks that Pillow
(libjpeg-turbo) decodes these files to the restatement's pixels, so they are real JPEG and no private dialect.

    write(coef, quant, geometry, script, restart=0) -> bytes
        coef      int [mcus][blocks][64] NATURAL order, the decoder's layout (Y blocks in raster order, Cb, Cr)
        quant     one uint8 [64] NATURAL-order table per component
        geometry  (H, W, comps, hs, vs)
        script    [(components, Ss, Se, Ah, Al)], components: indices into the frame
        restart   DRI, in each scan's own units (MCUs if interleaved, blocks of the component's grid otherwise); 0: none
"""
import struct

import numpy as np

from jpeg_decode_ref import ZIGZAG

PILLOW_SCRIPT_3 = [((0, 1, 2), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((2,), 1, 63, 0, 1), ((1,), 1, 63, 0, 1), ((0,), 6, 63, 0, 2),
                   ((0,), 1, 63, 2, 1), ((0, 1, 2), 0, 0, 1, 0), ((2,), 1, 63, 1, 0), ((1,), 1, 63, 1, 0), ((0,), 1, 63, 1, 0)]
PILLOW_SCRIPT_1 = [((0,), 0, 0, 0, 1), ((0,), 1, 5, 0, 2), ((0,), 6, 63, 0, 2), ((0,), 1, 63, 2, 1), ((0,), 0, 0, 1, 0),
                   ((0,), 1, 63, 1, 0)]


def _marker_segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


class _BitWriter(object):
    def __init__(self):
        self.out, self.acc, self.n = bytearray(), 0, 0

    def put(self, value, nbits):
        if nbits == 0:
            return
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 0xFF
            self.out.append(byte)
            if byte == 0xFF:
                self.out.append(0)
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)           # pad with ones


def optimal_table(freq):
    """{symbol: count} -> (BITS [16], HUFFVAL): T.81 K.2 with the all-ones code point reserved, lengths limited to 16"""
    f = dict((s, c) for s, c in freq.items() if c > 0)
    if not f:
        f = {0: 1}
    f[256] = 1                                                      # reserves the all-ones code
    size = dict((s, 0) for s in f)
    other = dict((s, -1) for s in f)
    live = dict(f)
    while len(live) > 1:
        c1 = min(live, key=lambda s: (live[s], -s))
        rest = dict(live)
        del rest[c1]
        c2 = min(rest, key=lambda s: (rest[s], -s))
        live[c1] += live.pop(c2)
        size[c1] += 1
        while other[c1] >= 0:
            c1 = other[c1]
            size[c1] += 1
        other[c1] = c2
        size[c2] += 1
        while other[c2] >= 0:
            c2 = other[c2]
            size[c2] += 1
    bits = [0] * 34
    for s in size:
        bits[size[s]] += 1
    i = 32
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1                                                    # the reserved code point goes
    vals = [s for length in range(1, 33) for s in sorted(k for k in size if k != 256 and size[k] == length)]
    return bits[1:17], vals


def _codes(bits, vals):
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


def _nbits(v):
    return int(v).bit_length()


def _scan_symbols(coef, geometry, scan, restart):
    """the scan as [interval: [(table key, symbol, extra value, extra bits) ...]]; a symbol of None is raw bits.  Table key:
    ("dc", c) or ("ac", c)"""
    H, W, comps, hs, vs = geometry
    members, ss, se, ah, al = scan
    sampling = [(hs, vs)] + [(1, 1)] * (comps - 1) if comps == 3 else [(1, 1)]
    mcu_w, mcu_h = -(-W // (8 * hs)), -(-H // (8 * vs))
    first_block = [sum(a * b for a, b in sampling[:c]) for c in range(comps)]
    if len(members) > 1:
        units = [[(m, first_block[c] + q, c) for c in members for q in range(sampling[c][0] * sampling[c][1])]
                 for m in range(mcu_w * mcu_h)]
    else:
        c = members[0]
        h, v = sampling[c]
        rows, cols = -(-(-(-H * v // vs)) // 8), -(-(-(-W * h // hs)) // 8)
        units = [[((br // v) * mcu_w + bc // h, first_block[c] + (br % v) * h + bc % h, c)] for br in range(rows)
                 for bc in range(cols)]
    per = restart if 0 < restart < len(units) else len(units)
    zz = ZIGZAG.tolist()
    intervals = []
    for first in range(0, len(units), per):
        out = []
        pred = dict((c, 0) for c in members)
        state = dict(eobrun=0, be=[])

        def flush_eobrun(c):
            if state["eobrun"] > 0:
                n = _nbits(state["eobrun"]) - 1
                out.append((("ac", c), n << 4, state["eobrun"] & ((1 << n) - 1), n))
                state["eobrun"] = 0
            for b in state["be"]:
                out.append((None, None, b, 1))
            state["be"] = []

        for unit in units[first:first + per]:
            for m, b, c in unit:
                blk = [int(v) for v in coef[m][b]]
                if ss == 0 and ah == 0:
                    v = blk[0] >> al
                    diff = v - pred[c]
                    pred[c] = v
                    n = _nbits(abs(diff))
                    out.append((("dc", c), n, diff if diff >= 0 else diff - 1, n))
                elif ss == 0:
                    out.append((None, None, (blk[0] >> al) & 1, 1))
                elif ah == 0:
                    r = 0
                    for k in range(ss, se + 1):
                        t = blk[zz[k]]
                        a = abs(t) >> al
                        if a == 0:
                            r += 1
                            continue
                        flush_eobrun(c)
                        while r > 15:
                            out.append((("ac", c), 0xF0, 0, 0))
                            r -= 16
                        n = _nbits(a)
                        out.append((("ac", c), (r << 4) | n, a if t >= 0 else ~a, n))
                        r = 0
                    if r > 0:
                        state["eobrun"] += 1
                        if state["eobrun"] == 0x7FFF:
                            flush_eobrun(c)
                else:
                    absval = [abs(blk[zz[k]]) >> al for k in range(64)]
                    eob = max([k for k in range(ss, se + 1) if absval[k] == 1] or [0])
                    r, br_bits = 0, []
                    for k in range(ss, se + 1):
                        a = absval[k]
                        if a == 0:
                            r += 1
                            continue
                        while r > 15 and k <= eob:
                            flush_eobrun(c)
                            out.append((("ac", c), 0xF0, 0, 0))
                            r -= 16
                            out.extend((None, None, bit, 1) for bit in br_bits)
                            br_bits = []
                        if a > 1:
                            br_bits.append(a & 1)
                            continue
                        flush_eobrun(c)
                        out.append((("ac", c), (r << 4) | 1, 0 if blk[zz[k]] < 0 else 1, 1))
                        out.extend((None, None, bit, 1) for bit in br_bits)
                        br_bits = []
                        r = 0
                    if r > 0 or br_bits:
                        state["eobrun"] += 1
                        state["be"] += br_bits
                        if state["eobrun"] == 0x7FFF:
                            flush_eobrun(c)
        if ss > 0:
            flush_eobrun(members[0])
        intervals.append(out)
    return intervals


def write(coef, quant, geometry, script, restart=0):
    H, W, comps, hs, vs = geometry
    out = bytearray(b"\xFF\xD8")
    for c in range(comps):
        out += _marker_segment(0xDB, bytes((c,)) + np.asarray(quant[c], np.uint8)[ZIGZAG].tobytes())
    frame = struct.pack(">BHHB", 8, H, W, comps)
    for c in range(comps):
        frame += bytes((c + 1, (hs << 4 | vs) if (c == 0 and comps == 3) else 0x11, c))
    out += _marker_segment(0xC2, frame)
    if restart:
        out += _marker_segment(0xDD, struct.pack(">H", restart))
    for scan in script:
        members, ss, se, ah, al = scan
        intervals = _scan_symbols(coef, geometry, scan, restart)
        freq = {}
        for items in intervals:
            for key, sym, _, _ in items:
                if key is not None:
                    freq.setdefault(key, {})
                    freq[key][sym] = freq[key].get(sym, 0) + 1
        codes = {}
        for key in sorted(freq):
            bits, vals = optimal_table(freq[key])
            codes[key] = _codes(bits, vals)
            tc_th = (0x00 | key[1]) if key[0] == "dc" else 0x10
            out += _marker_segment(0xC4, bytes((tc_th,)) + bytes(bits) + bytes(vals))
        head = bytes((len(members),))
        for c in members:
            head += bytes((c + 1, (c << 4) if ss == 0 else 0))
        out += _marker_segment(0xDA, head + bytes((ss, se, ah << 4 | al)))
        for i, items in enumerate(intervals):
            if i:
                out += bytes((0xFF, 0xD0 + ((i - 1) & 7)))
            w = _BitWriter()
            for key, sym, value, nbits in items:
                if key is not None:
                    code, length = codes[key][sym]
                    w.put(code, length)
                w.put(value, nbits)
            w.flush()
            out += w.out
    return bytes(out + b"\xFF\xD9")
