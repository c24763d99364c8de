"""The NumPy / Python restatement of the progressive entropy stage (csrc/jpeg_decode.hip: jpeg_progressive_kernel,
acimg/jpeg.py: the SOF2 path of parse_jpeg), written independently of both: the definition the device is held to.

It walks an SOF2 file SEQUENTIALLY, marker by marker and scan by scan, binds the tables and the restart interval in force at
each SOS, and decodes every scan bit by bit with the four procedures of T.81 Annex G, meeting each RSTn marker and each
following segment where the bit walk ends (the product finds them with a byte search instead).  A scan of one component
walks that component's own block grid; a scan of several walks the MCUs.  The first error in (scan, interval) order ends
the walk: that is the status the device reports, since an item depends on earlier scans only.

    r = walk_progressive(data)      r.coef int16 [mcus][blocks][64] NATURAL order, r.status, r.scans (what each SOS said, and the offset
                        of each interval), r.census (what the stream reached), and the geometry jpeg_decode_ref.idct / colour
                        take (height width comps hs vs sampling quant mcu_w mcu_h mcus blocks)
    decode_progressive(data)        -> uint8 [H][W][3] B G R, through jpeg_decode_ref's later stages
    levels(script)      the level rule, restated
    record_status(...)  the legal ranges of a device scan record, restated
"""
import collections
import struct

import numpy as np

import jpeg_decode_ref as jref
from jpeg_decode_ref import STATUS_BAD_CODE, STATUS_EARLY_END, STATUS_OK, STATUS_RUN, ZIGZAG, Bits, extend, lookup16

STATUS_DESCRIPTOR = 4
MAX_SCANS, MAX_TABLES = 256, 512

# what the case set (fixture + writer cases) must reach; tests/test_jpeg_progressive_cpu.py fails when one is lost
CENSUS = tuple(["eobrun_category_%d" % c for c in range(15)] +
               ["zrl_first", "zrl_refine", "correction_bit_0", "correction_bit_1", "new_plus", "new_minus",
                "dc_interleaved", "dc_non_interleaved", "padding_blocks", "ac_scan_of_several_intervals",
                "restart_cuts_an_eob_run", "refinement_block_inside_an_eob_run", "zero_run_of_15_crosses_nonzero",
                "dc_depth_0_0", "dc_depth_0_1", "dc_depth_1_0", "dc_depth_0_2", "dc_depth_2_1",
                "ac_depth_0_0", "ac_depth_0_1", "ac_depth_1_0", "ac_depth_0_2", "ac_depth_2_1"])


class Scan(object):
    """comps: indices in the frame; ss se ah al; restart (as DRI said, in the scan's units); begin: offset of its
    entropy-coded segment; offsets: of each interval's first byte from `begin`; end: where the walk left the segment"""


class Walk(object):
    pass


def levels(script):
    """[(components, Ss, Se, ...)] -> per scan 0, or 1 + the highest level of an earlier scan that shares a component and
    overlaps [Ss, Se]"""
    out = []
    for k, s in enumerate(script):
        lv = 0
        for j in range(k):
            p = script[j]
            if set(p[0]) & set(s[0]) and not (p[2] < s[1] or s[2] < p[1]):
                lv = max(lv, out[j] + 1)
        out.append(lv)
    return out


def record_status(fields, comps, scans_of_image, tables, intervals, units_of):
    """a device scan record (include/acimg.h: ACIMG_JPEG_PROG_SCAN_FIELDS int32) -> STATUS_OK or STATUS_DESCRIPTOR.
    units_of(mask) -> MCUs or blocks the scan walks"""
    mask, ss, se, ah, al, t0, t1, t2, restart, _, _, first, level = [int(v) for v in fields[:13]]
    if not 1 <= mask < (1 << comps) or not 0 <= ss <= se <= 63 or (ss == 0 and se != 0):
        return STATUS_DESCRIPTOR
    members = [c for c in range(comps) if mask >> c & 1]
    if ss > 0 and len(members) != 1:
        return STATUS_DESCRIPTOR
    if not (0 <= ah <= 13 and 0 <= al <= 13 and restart >= 0 and 0 <= level < scans_of_image):
        return STATUS_DESCRIPTOR
    if any(int(v) for v in fields[13:16]):
        return STATUS_DESCRIPTOR
    if not (ss == 0 and ah != 0) and any(not 0 <= (t0, t1, t2)[c] < tables for c in members):
        return STATUS_DESCRIPTOR
    units = units_of(mask)
    per = restart if 1 <= restart <= units else units
    if first < 0 or first > intervals or -(-units // per) > intervals - first:
        return STATUS_DESCRIPTOR
    return STATUS_OK


def _next_marker(data, pos, end):
    """the first FF xx at or after pos with xx neither 00 nor FF, or end"""
    while pos + 1 < end:
        if data[pos] == 0xFF and data[pos + 1] not in (0x00, 0xFF):
            return pos
        pos += 1
    return end


def walk_progressive(data, census=None):
    """the whole file -> Walk (see the module docstring).  census: a Counter that receives what the stream reached"""
    data = bytes(data)
    size = len(data)
    assert data[:2] == b"\xFF\xD8"
    w = Walk()
    w.data, w.scans, w.status, w.slack = data, [], STATUS_OK, 0
    w.census = census if census is not None else collections.Counter()
    note = w.census
    qt, huff, restart, frame = {}, {}, 0, None
    pos = 2
    sent = None
    while pos + 4 <= size:
        assert data[pos] == 0xFF, pos
        marker = data[pos + 1]
        if marker == 0xD9:
            break
        length = struct.unpack_from(">H", data, pos + 2)[0]
        body = data[pos + 4:pos + 2 + length]
        pos += 2 + length
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
                huff[body[at]] = lookup16(counts, list(body[at + 17:at + 17 + n]))
                at += 17 + n
        elif marker == 0xC2:
            assert body[0] == 8 and frame is None
            w.height, w.width, w.comps = struct.unpack_from(">HHB", body, 1)
            frame = [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i]) for i in range(w.comps)]
            if w.comps == 1:
                frame = [(frame[0][0], 1, 1, frame[0][3])]
            w.hs, w.vs = frame[0][1], frame[0][2]
            assert all(f[1:3] == (1, 1) for f in frame[1:])
            w.sampling = [(f[1], f[2]) for f in frame]
            w.mcu_w, w.mcu_h = -(-w.width // (8 * w.hs)), -(-w.height // (8 * w.vs))
            w.mcus = w.mcu_w * w.mcu_h
            w.blocks = sum(h * v for h, v in w.sampling)
            w.coef = np.zeros((w.mcus, w.blocks, 64), np.int16)
            # each component's own block grid
            w.grid = [(-(-(-(-w.height * v // w.vs)) // 8), -(-(-(-w.width * h // w.hs)) // 8)) for h, v in w.sampling]
            sent = np.full((w.comps, 64), -1)
        elif marker == 0xDD:
            restart = struct.unpack_from(">H", body)[0]
        elif marker == 0xDA:
            if not w.scans:
                w.quant = [qt[f[3]] for f in frame]
            s = Scan()
            ns = body[0]
            ids = [f[0] for f in frame]
            s.comps = [ids.index(body[1 + 2 * j]) for j in range(ns)]
            sel = [body[2 + 2 * j] for j in range(ns)]
            s.ss, s.se = body[1 + 2 * ns], body[2 + 2 * ns]
            s.ah, s.al = body[3 + 2 * ns] >> 4, body[3 + 2 * ns] & 15
            s.restart, s.begin = restart, pos
            s.dc = {c: huff.get(sel[j] >> 4) for j, c in enumerate(s.comps)}
            s.ac = huff.get(0x10 | (sel[0] & 15))
            w.scans.append(s)
            for c in s.comps:
                sent[c, s.ss:s.se + 1] = s.al
            kind = "dc" if s.ss == 0 else "ac"
            note["%s_depth_%d_%d" % (kind, s.ah, s.al)] += 1
            status = _scan(w, s, note)
            if status != STATUS_OK:
                w.status = status
                return w
            nxt = _next_marker(data, s.end, size)
            w.slack += nxt - s.end
            pos = nxt
        else:
            assert 0xE0 <= marker <= 0xEF or marker == 0xFE, hex(marker)
    w.complete = sent is not None and bool((sent == 0).all())
    return w


def _block_of(w, c, br, bc):
    """(block row, block column) of component c's own grid -> (MCU, block in MCU)"""
    h, v = w.sampling[c]
    first = sum(a * b for a, b in w.sampling[:c])
    return (br // v) * w.mcu_w + bc // h, first + (br % v) * h + bc % h


def _scan(w, s, note):
    """one scan, interval by interval; leaves s.offsets and s.end; -> status of its first bad interval"""
    data = w.data
    end = len(data)
    interleaved = len(s.comps) > 1
    if interleaved:
        units = [[(m, sum(a * b for a, b in w.sampling[:c]) + q, c) for c in s.comps
                  for q in range(w.sampling[c][0] * w.sampling[c][1])] for m in range(w.mcus)]
    else:
        c = s.comps[0]
        rows, cols = w.grid[c]
        units = [[_block_of(w, c, br, bc) + (c,)] for br in range(rows) for bc in range(cols)]
        if s.ss == 0:
            note["dc_non_interleaved"] += 1
        if rows * cols < w.mcus * w.sampling[c][0] * w.sampling[c][1]:
            note["padding_blocks"] += 1
    if interleaved:
        note["dc_interleaved"] += 1
    per = s.restart if 0 < s.restart < len(units) else len(units)
    if s.ss > 0 and per < len(units):
        note["ac_scan_of_several_intervals"] += 1
    zz = ZIGZAG.tolist()
    p1 = 1 << s.al
    pos, s.offsets = s.begin, [0]
    last_block_in_run = False
    for first in range(0, len(units), per):
        if first:
            if not (pos + 1 < end and data[pos] == 0xFF and data[pos + 1] == 0xD0 + ((first // per - 1) & 7)):
                s.end = pos
                return STATUS_EARLY_END                          # the interval is not there: its lane finds no bits
            pos += 2
            s.offsets.append(pos - s.begin)
        bits = Bits(data, pos, end)
        pred = {c: 0 for c in s.comps}
        eobrun = 0
        s.end = pos
        for n_unit, unit in enumerate(units[first:first + per]):
            for m, b, c in unit:
                blk = w.coef[m, b]
                if s.ss == 0 and s.ah == 0:                      # DC first
                    e = int(s.dc[c][bits.peek16()]) if s.dc[c] is not None else 0
                    if e == 0 or (e & 255) > 15:
                        return STATUS_BAD_CODE
                    bits.skip(e >> 8)
                    cat = e & 255
                    diff = extend(bits.take(cat), cat)
                    if bits.overrun():
                        return STATUS_EARLY_END
                    pred[c] += diff
                    blk[0] = _i16(pred[c] << s.al)
                elif s.ss == 0:                                  # DC refinement
                    bit = bits.take(1)
                    if bits.overrun():
                        return STATUS_EARLY_END
                    if bit:
                        blk[0] = _i16(int(blk[0]) | p1)
                elif s.ah == 0:                                  # AC first
                    if eobrun > 0:
                        eobrun -= 1
                        last_block_in_run = True
                        continue
                    ended_by_eob = False
                    if n_unit == 0 and first and last_block_in_run:
                        e = int(s.ac[bits.peek16()])
                        if e and (e & 15) == 0 and ((e >> 4) & 15) != 15:
                            note["restart_cuts_an_eob_run"] += 1
                    k = s.ss
                    while k <= s.se:
                        e = int(s.ac[bits.peek16()]) if s.ac is not None else 0
                        if e == 0:
                            return STATUS_BAD_CODE
                        bits.skip(e >> 8)
                        r, size = (e >> 4) & 15, e & 15
                        if size:
                            k += r
                            val = extend(bits.take(size), size)
                            if bits.overrun():
                                return STATUS_EARLY_END
                            if k > s.se:
                                return STATUS_RUN
                            blk[zz[k]] = _i16(val << s.al)
                        elif r == 15:
                            k += 15
                            note["zrl_first"] += 1
                        else:
                            eobrun = (1 << r) + (bits.take(r) if r else 0)
                            if bits.overrun():
                                return STATUS_EARLY_END
                            note["eobrun_category_%d" % r] += 1
                            eobrun -= 1
                            ended_by_eob = True
                            break
                        if bits.overrun():
                            return STATUS_EARLY_END
                        k += 1
                    last_block_in_run = ended_by_eob             # the interval's last block lay in an end-of-band run
                else:                                            # AC refinement
                    k = s.ss
                    if eobrun == 0:
                        while k <= s.se:
                            e = int(s.ac[bits.peek16()]) if s.ac is not None else 0
                            if e == 0:
                                return STATUS_BAD_CODE
                            bits.skip(e >> 8)
                            r, size = (e >> 4) & 15, e & 15
                            val = 0
                            if size:
                                if size != 1:
                                    return STATUS_BAD_CODE
                                val = p1 if bits.take(1) else -p1
                                note["new_plus" if val > 0 else "new_minus"] += 1
                            elif r != 15:
                                eobrun = (1 << r) + (bits.take(r) if r else 0)
                                if bits.overrun():
                                    return STATUS_EARLY_END
                                note["eobrun_category_%d" % r] += 1
                                break
                            else:
                                note["zrl_refine"] += 1
                            if bits.overrun():
                                return STATUS_EARLY_END
                            run, crossed = r, False
                            while k <= s.se:
                                at = zz[k]
                                if blk[at] != 0:
                                    crossed = True
                                    if not _correct(bits, blk, at, p1, note):
                                        return STATUS_EARLY_END
                                else:
                                    r -= 1
                                    if r < 0:
                                        break
                                k += 1
                            if run == 15 and crossed and size:
                                note["zero_run_of_15_crosses_nonzero"] += 1
                            if val:
                                if k > s.se:
                                    return STATUS_RUN
                                blk[zz[k]] = _i16(val)
                            k += 1
                    if eobrun > 0:
                        if k == s.ss:
                            note["refinement_block_inside_an_eob_run"] += 1
                        while k <= s.se:
                            at = zz[k]
                            if blk[at] != 0 and not _correct(bits, blk, at, p1, note):
                                return STATUS_EARLY_END
                            k += 1
                        eobrun -= 1
        pos = bits.align()
        s.end = pos
    return STATUS_OK


def _i16(v):
    return ((int(v) + 32768) & 0xFFFF) - 32768


def _correct(bits, blk, at, p1, note):
    """the correction bit of a coefficient that is already nonzero; False where the data has no such bit"""
    bit = bits.take(1)
    if bits.overrun():
        return False
    note["correction_bit_%d" % bit] += 1
    v = int(blk[at])
    if bit and (v & p1) == 0:
        blk[at] = _i16(v + p1 if v >= 0 else v - p1)
    return True


def decode_progressive(data):
    """a whole progressive file -> uint8 [H][W][3] in B, G, R order"""
    w = walk_progressive(data)
    assert w.status == STATUS_OK and w.complete, (w.status, w.complete)
    return jref.colour(w, jref.idct(w, w.coef))


def load_progressive_golden():
    """tests/golden/jpeg_progressive_golden.npz -> {name: (file bytes, Pillow's pixels uint8 [H][W][3] B G R)}, in file
    order.  A name in `pixels_in_baseline_fixture` has the pixels of its baseline twin in jpeg_decode_golden.npz: the
    generator asserted that Pillow decodes both files to the same pixels."""
    import os
    golden = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    z, base = np.load(os.path.join(golden, "jpeg_progressive_golden.npz")), np.load(os.path.join(golden, "jpeg_decode_golden.npz"))
    elsewhere = set(z["pixels_in_baseline_fixture"].tolist())
    out = collections.OrderedDict()
    for name in z["names"].tolist():
        px = (base if name in elsewhere else z)["pixels_" + name]
        bgr = np.ascontiguousarray(px[::-1].transpose(1, 2, 0) if px.ndim == 3 else np.repeat(px[..., None], 3, 2))
        bgr.setflags(write=False)
        out[name] = (z["jpeg_" + name].tobytes(), bgr)
    return out
