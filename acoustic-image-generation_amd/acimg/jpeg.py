"""Baseline JPEG files (JFIF, 4:2:0) of RGB8 device tensors: the two kernels of csrc/jpeg.hip (`acimg_jpeg_blocks`,
`acimg_jpeg_scan`) produce each frame's entropy-coded segment on the device; the header segments, which depend on the
size, the quality and the restart interval alone, are built here once per encoder and size.  Per `encode` call two
transfers come back: the frames' byte counts and their packed bytes.  No imaging library is involved.

The other direction - baseline, extended sequential and progressive files to B, G, R pixels, the `cv2.imread` of
convert_data2.py:157 - is `parse_jpeg` (the markers, on the host: geometry, tables in the device's layout, where the
scans and their restart intervals lie, for a progressive file the scan list with its levels; everything outside the
decoder's scope is refused by name before any launch) and `JpegDecoder` (the kernels of csrc/jpeg_decode.hip: entropy
decode - one kernel for sequential files, one for progressive ones - dequantise + inverse DCT, upsample + colour)."""
import collections
import ctypes as C
import struct

import numpy as np
import torch

from . import _lib, ops
from .convert import ConvertError

# zig-zag position -> natural (row-major) index: the order a DQT segment stores a table in
ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
          35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
          62, 63)

# ITU-T T.81 Annex K.3: (table class << 4 | destination, BITS, HUFFVAL) of the four typical tables, in file order
_DC_VALS = bytes(range(12))
_AC_LUMA_VALS = bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a"
    "434445464748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9"
    "aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA_VALS = bytes.fromhex(
    "0001020311040521310612415107617113223281081442 91a1b1c109233352f0156272d10a162434e125f11718191a262728292a353637"
    "38393a434445464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4"
    "a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")
HUFFMAN_TABLES = (
    (0x00, bytes((0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0)), _DC_VALS),
    (0x10, bytes((0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D)), _AC_LUMA_VALS),
    (0x01, bytes((0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0)), _DC_VALS),
    (0x11, bytes((0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77)), _AC_CHROMA_VALS),
)
EOI = b"\xFF\xD9"


def quant_tables(quality):
    """uint8 [2,64], natural order, luma then chroma (`acimg_jpeg_quant_tables`)"""
    out = np.zeros(128, np.uint8)
    _lib.check(_lib.load().acimg_jpeg_quant_tables(int(quality), out.ctypes.data_as(C.c_void_p)), "jpeg_quant_tables")
    return out.reshape(2, 64)


def _segment(marker, payload):
    return struct.pack(">BBH", 0xFF, marker, len(payload) + 2) + payload


def jfif_header(height, width, qtables, restart_mcus):
    """SOI, APP0, two DQT, SOF0 (Y 2x2, Cb 1x1, Cr 1x1), four DHT, DRI, SOS: everything in front of the scan"""
    qt = np.asarray(qtables, np.uint8).reshape(2, 64)
    zz = list(ZIGZAG)
    h = b"\xFF\xD8" + _segment(0xE0, b"JFIF\x00" + struct.pack(">BBBHHBB", 1, 1, 0, 1, 1, 0, 0))
    for i in range(2):
        h += _segment(0xDB, bytes((i,)) + qt[i][zz].tobytes())
    h += _segment(0xC0, struct.pack(">BHHB", 8, height, width, 3) + bytes((1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1)))
    for tc_th, bits, vals in HUFFMAN_TABLES:
        h += _segment(0xC4, bytes((tc_th,)) + bits + vals)
    h += _segment(0xDD, struct.pack(">H", restart_mcus))
    return h + _segment(0xDA, bytes((3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0)))


class JpegEncoder(object):
    """quality 1..100 (the libjpeg scaling of the Annex K tables); restart_mcus: MCUs (16 x 16 pixels) per restart
    interval, None = one MCU row.  The intervals are what the device codes in parallel."""

    def __init__(self, device, quality=90, restart_mcus=None):
        self.device = torch.device(device)
        self.lib = _lib.load()
        self.quality = int(quality)
        if restart_mcus is not None and not 1 <= int(restart_mcus) <= 65535:
            raise ValueError("restart_mcus is 1..65535 or None, got %r" % (restart_mcus,))
        self._restart = None if restart_mcus is None else int(restart_mcus)
        self.qtables = quant_tables(self.quality)
        self._qt_dev = torch.from_numpy(self.qtables.reshape(128).copy()).to(self.device)
        self._headers = {}

    def restart_mcus(self, width):
        return self._restart if self._restart is not None else -(-int(width) // 16)

    def header(self, height, width):
        key = (int(height), int(width))
        if key not in self._headers:
            self._headers[key] = jfif_header(key[0], key[1], self.qtables, self.restart_mcus(width))
        return self._headers[key]

    def scan(self, frames):
        """uint8 [n,H,W,3] -> (scan uint8 [n,stride] on the device, scan_bytes int32 [n] on the device)"""
        f = frames.to(self.device)
        if f.dtype != torch.uint8 or f.dim() != 4 or f.shape[3] != 3 or f.shape[0] < 1:
            raise ValueError("frames are uint8 [n,H,W,3], got %s %s" % (frames.dtype, tuple(frames.shape)))
        f = f.contiguous()
        n, H, W = int(f.shape[0]), int(f.shape[1]), int(f.shape[2])
        L, r = self.lib, self.restart_mcus(W)
        stride = int(L.acimg_jpeg_scan_capacity(H, W, r))
        if stride == 0:
            raise ValueError("a JPEG frame is 1..65535 pixels wide and high, got %d x %d" % (H, W))
        stride = -(-stride // 16) * 16
        coef = torch.empty(int(L.acimg_jpeg_coef_bytes(n, H, W)) // 2, dtype=torch.int16, device=self.device)
        ws_bytes = int(L.acimg_jpeg_scan_workspace(n, H, W, r))
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device)
        out = torch.empty(n, stride, dtype=torch.uint8, device=self.device)
        nbytes = torch.empty(n, dtype=torch.int32, device=self.device)
        st = ops.current_stream_handle(self.device)
        _lib.check(L.acimg_jpeg_blocks(f.data_ptr(), n, H, W, self._qt_dev.data_ptr(), coef.data_ptr(), st), "jpeg_blocks")
        _lib.check(L.acimg_jpeg_scan(coef.data_ptr(), n, H, W, r, out.data_ptr(), stride, nbytes.data_ptr(), ws.data_ptr(),
                                     ws_bytes, st), "jpeg_scan")
        return out, nbytes

    def encode(self, frames):
        """uint8 [n,H,W,3] (device or host tensor) -> a list of n complete JFIF files as bytes"""
        out, nbytes = self.scan(frames)
        counts = nbytes.cpu().tolist()                                       # read-back 1: n int32
        packed = torch.cat([out[i, :c] for i, c in enumerate(counts)]).cpu().numpy().tobytes()    # read-back 2
        head = self.header(frames.shape[1], frames.shape[2])
        files, at = [], 0
        for c in counts:
            files.append(head + packed[at:at + c] + EOI)
            at += c
        return files


def encode_jpeg(rgb_uint8, quality=90, restart_mcus=None, device="cuda:0"):
    """[H,W,3] uint8 (array or tensor) -> the bytes of a JFIF file, encoded on `device`"""
    a = torch.as_tensor(rgb_uint8)
    if a.dtype != torch.uint8 or a.dim() != 3 or a.shape[2] != 3:
        raise ValueError("write_jpeg wants a [H,W,3] uint8 image, got %s %s" % (a.dtype, tuple(a.shape)))
    return JpegEncoder(device, quality, restart_mcus).encode(a.unsqueeze(0))[0]


def write_jpeg(path, rgb_uint8, quality=90, restart_mcus=None, device="cuda:0"):
    data = encode_jpeg(rgb_uint8, quality, restart_mcus, device)
    with open(path, "wb") as f:
        f.write(data)
    return len(data)


# ---- decoding -------------------------------------------------------------------------------------------------------------
HUFF_BYTES = 904                      # ACIMG_JPEG_HUFF_BYTES: look uint16[256], maxcode int32[17], valoff int32[17], vals uint8[256]
STATUS_TEXT = {0: "ok", 1: "a code that is in no Huffman table", 2: "a run past coefficient 63", 3: "the data ends early",
               4: "a bad scan or interval descriptor"}
MAX_SCANS, MAX_TABLES, MAX_INTERVALS, SCAN_FIELDS = 256, 512, 1 << 24, 16      # ACIMG_JPEG_PROG_* of include/acimg.h
_SOF_NAMES = {0xC3: "lossless", 0xC5: "differential sequential",
              0xC6: "differential progressive", 0xC7: "differential lossless", 0xC9: "arithmetic-coded sequential",
              0xCA: "arithmetic-coded progressive", 0xCB: "arithmetic-coded lossless", 0xCD: "arithmetic-coded differential",
              0xCE: "arithmetic-coded differential progressive", 0xCF: "arithmetic-coded differential lossless"}

JpegInfo = collections.namedtuple(
    "JpegInfo", "height width comps hs vs mcu_w mcu_h mcus blocks quant huff scan_begin scan_end restart_mcus intervals "
                "sof scans pool", defaults=(0xC0, None, None))
JpegInfo.__doc__ = """what `parse_jpeg` finds: quant uint8 [3][64] natural order, per component; huff uint8 [6][HUFF_BYTES],
DC and AC table per component in the device layout; [scan_begin, scan_end) the entropy-coded segment in the file;
restart_mcus (0: none); intervals int32 [count][2]: first and end byte of each restart interval relative to scan_begin,
count = ceil(mcus / restart_mcus) whatever the file holds (an interval the file lacks is empty); sof: the frame's marker
(0xC0, 0xC1 or 0xC2).  A progressive file (sof 0xC2) has scans: a tuple of ScanInfo in file order, and pool uint8
[tables][HUFF_BYTES]: the tables its scans name; its huff is None, restart_mcus 0, [scan_begin, scan_end) reaches from its
first scan to the end of its last, and intervals holds those of all scans back to back, each relative to ITS scan's begin.
scans and pool are None for a sequential file."""
ScanInfo = collections.namedtuple("ScanInfo", "comps ss se ah al tables restart begin end first_interval count level")
ScanInfo.__doc__ = """one scan of a progressive file: comps: indices of its components in the frame; tables: per frame
component the index in the pool of the DC (Ss = 0) or AC table the scan reads for it, -1 where it reads none; restart: the
interval in the scan's own units (MCUs if interleaved, else blocks of the component's own grid; 0: none); [begin, end):
its entropy-coded segment in the file; its `count` intervals start at `first_interval` of JpegInfo.intervals; level: 0, or
1 + the highest level of an earlier scan that shares a component and overlaps [ss, se] (`scan_levels`)"""


def derive_huffman(counts, vals, name="<jpeg>"):
    """BITS (codes per length 1..16) and HUFFVAL of a DHT segment -> uint8 [HUFF_BYTES], the layout csrc/jpeg_decode.hip
    reads (Annex C codes; an over-full code space is refused)"""
    out = np.zeros(HUFF_BYTES, np.uint8)
    look = out[:512].view(np.uint16)
    maxcode = out[512:580].view(np.int32)
    valoff = out[580:648].view(np.int32)
    maxcode[:] = -1
    out[648:648 + len(vals)] = np.frombuffer(bytes(vals), np.uint8)
    code = k = 0
    for length in range(1, 17):
        n = counts[length - 1]
        if code + n > (1 << length):
            raise ConvertError("%s: a Huffman table with more codes of %d bits than there are" % (name, length))
        if n:
            valoff[length] = k - code
            maxcode[length] = code + n - 1
            if length <= 8:
                for i in range(n):
                    look[(code + i) << (8 - length):(code + i + 1) << (8 - length)] = (length << 8) | vals[k + i]
            code += n
            k += n
        code <<= 1
    return out


def _read_dht(body, name, cut):
    """the tables of one DHT segment -> [(Tc << 4 | Th, uint8 [HUFF_BYTES])]"""
    out, at = [], 0
    while at < len(body):
        if at + 17 > len(body):
            raise cut("a DHT segment")
        counts = list(body[at + 1:at + 17])
        n = sum(counts)
        if n > 256 or at + 17 + n > len(body):
            raise cut("a DHT segment")
        vals = body[at + 17:at + 17 + n]
        if body[at] >> 4 == 0 and any(v > 15 for v in vals):
            raise ConvertError("%s: a DC Huffman table with a category above 15" % name)
        out.append((body[at], derive_huffman(counts, vals, name)))
        at += 17 + n
    return out


def scan_levels(scans):
    """[(components, Ss, Se)] in file order -> the level of each: 0, or 1 + the highest level of an earlier scan that shares
    a component with it and whose band overlaps its own.  Scans of one level touch disjoint coefficients."""
    levels = []
    for k, (comps, ss, se) in enumerate(scans):
        below = [levels[j] for j, (c, a, e) in enumerate(scans[:k]) if set(c) & set(comps) and a <= se and ss <= e]
        levels.append(1 + max(below) if below else 0)
    return levels


def parse_jpeg(data, name="<jpeg>"):
    """the markers of one file -> JpegInfo.  Taken: SOF0 and SOF1 (sequential; SOF1 is the same process with up to four
    tables a class) of 8 bits with one or three components in one interleaved scan, and SOF2 (progressive) of 8 bits with
    any legal scan script that sends every coefficient down to bit 0; luma 1x1 / 2x1 / 2x2 over 1x1 chroma, any 8-bit DQT
    and any DHT, DRI / RSTn; APPn and COM are skipped.  Everything else is a ConvertError that names the file and the
    reason; every refusal of an SOF2 file begins "<name>: progressive JPEG".  A scan that ends early is NOT refused here:
    the device reports it."""
    buf = bytes(data)
    size = len(buf)

    who = name                                            # name + ": progressive JPEG" once an SOF2 marker was met

    def cut(what):
        return ConvertError("%s: truncated JPEG file: %d bytes end inside %s" % (who, size, what))

    if size < 4 or buf[:2] != b"\xFF\xD8":
        raise ConvertError("%s: not a JPEG file (no SOI marker)" % name)
    qt, huff, frame, restart, pos, sof, pool, pooled = {}, {}, None, 0, 2, 0xC0, [], {}
    while True:
        if pos + 4 > size:
            raise cut("the header segments")
        if buf[pos] != 0xFF:
            raise ConvertError("%s: byte %d is no marker" % (who, pos))
        marker = buf[pos + 1]
        if marker == 0xFF:                                # fill byte
            pos += 1
            continue
        length = struct.unpack_from(">H", buf, pos + 2)[0]
        if length < 2 or pos + 2 + length > size:
            raise cut("segment FF %02X" % marker)
        body = buf[pos + 4:pos + 2 + length]
        if marker in _SOF_NAMES:
            raise ConvertError("%s: %s JPEG (SOF%d): only sequential and progressive Huffman files (SOF0, SOF1, SOF2) are "
                               "decoded" % (name, _SOF_NAMES[marker], marker - 0xC0))
        if marker in (0xC0, 0xC1, 0xC2):
            who = name + ": progressive JPEG" if marker == 0xC2 else who
            if frame is not None or len(body) < 6:
                raise ConvertError("%s: a second or short frame header" % who)
            sof = marker
            precision, height, width, comps = struct.unpack_from(">BHHB", body)
            if precision != 8:
                raise ConvertError("%s: %d-bit samples: only 8-bit files are decoded" % (who, precision))
            if comps not in (1, 3):
                raise ConvertError("%s: %d components: only one (grey) or three (Y Cb Cr) are decoded" % (who, comps))
            if len(body) < 6 + 3 * comps or height < 1 or width < 1:
                raise ConvertError("%s: frame header of %d bytes for %d x %d pixels" % (who, len(body), width, height))
            frame = (height, width, [(body[6 + 3 * i], body[7 + 3 * i] >> 4, body[7 + 3 * i] & 15, body[8 + 3 * i])
                                     for i in range(comps)])
        elif marker == 0xDB:
            at = 0
            while at < len(body):
                if body[at] >> 4:
                    raise ConvertError("%s: 16-bit DQT entries: only 8-bit quantisation tables are decoded" % who)
                if at + 65 > len(body):
                    raise cut("a DQT segment")
                t = np.zeros(64, np.uint8)
                t[list(ZIGZAG)] = np.frombuffer(body[at + 1:at + 65], np.uint8)
                qt[body[at] & 15] = t
                at += 65
        elif marker == 0xC4:
            for key, table in _read_dht(body, who, cut):
                huff[key] = table
                pooled[key] = len(pool)
                pool.append(table)
        elif marker == 0xDD:
            if len(body) < 2:
                raise cut("the DRI segment")
            restart = struct.unpack_from(">H", body)[0]
        elif marker == 0xDA:
            break
        elif not (0xE0 <= marker <= 0xEF or marker == 0xFE):
            raise ConvertError("%s: marker FF %02X is not decoded" % (who, marker))
        pos += 2 + length
    if frame is None:
        raise ConvertError("%s: a scan without a frame header" % name)
    if sof == 0xC2:
        return _parse_progressive(buf, name, frame, qt, pool, pooled, restart, pos, cut)
    height, width, comp = frame
    comps = len(comp)
    if len(body) < 4 + 2 * body[0] or body[0] != comps:
        raise ConvertError("%s: a scan of %d of the %d components: only one interleaved scan is decoded (multiple scans)"
                           % (name, body[0], comps))
    ss, se, ahal = body[1 + 2 * comps:4 + 2 * comps]
    if (ss, se, ahal) != (0, 63, 0):
        raise ConvertError("%s: a scan of coefficients %d..%d: only one full scan is decoded" % (name, ss, se))
    if comps == 1:                                        # one component is never interleaved: 8 x 8 MCUs
        comp = [(comp[0][0], 1, 1, comp[0][3])]
    hs, vs = comp[0][1], comp[0][2]
    if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comp[1:]):
        raise ConvertError("%s: sampling %s: only luma 1x1, 2x1 or 2x2 over 1x1 chroma is decoded"
                           % (name, " ".join("%dx%d" % c[1:3] for c in comp)))
    quant, tables = np.zeros((3, 64), np.uint8), np.zeros((6, HUFF_BYTES), np.uint8)
    for i, (cid, _, _, tq) in enumerate(comp):
        sel = [body[2 + 2 * j] for j in range(comps) if body[1 + 2 * j] == cid]
        if len(sel) != 1:
            raise ConvertError("%s: the scan does not name component %d once" % (name, cid))
        if tq not in qt:
            raise ConvertError("%s: no quantisation table %d" % (name, tq))
        quant[i] = qt[tq]
        for j, key in enumerate((sel[0] >> 4, 0x10 | (sel[0] & 15))):
            if key not in huff:
                raise ConvertError("%s: no Huffman table %d of class %d" % (name, key & 15, key >> 4))
            tables[2 * i + j] = huff[key]
    mcu_w, mcu_h = -(-width // (8 * hs)), -(-height // (8 * vs))
    mcus = mcu_w * mcu_h
    scan_begin = pos + 2 + length
    # the segment ends at the first FF that neither stuffs (FF 00) nor restarts (FF D0..D7) nor fills (FF FF)
    seg = np.frombuffer(buf, np.uint8, offset=scan_begin)
    ff = np.flatnonzero(seg[:-1] == 0xFF) if seg.size > 1 else np.zeros(0, np.int64)
    nxt = seg[ff + 1]
    rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    other = np.flatnonzero(~rst & (nxt != 0) & (nxt != 0xFF))
    scan_len = int(ff[other[0]]) if other.size else seg.size
    if other.size:
        after = int(nxt[other[0]])
        if after != 0xD9:
            raise ConvertError("%s: marker FF %02X follows the scan: only one scan is decoded (multiple scans)" % (name, after))
    marks = ff[rst]
    marks = marks[marks < scan_len]
    per = restart if 0 < restart < mcus else mcus
    count = -(-mcus // per)
    intervals = np.full((count, 2), scan_len, np.int32)
    starts = np.concatenate([[0], marks + 2])[:count]
    ends = np.concatenate([marks, [scan_len]])[:count]
    intervals[:len(starts), 0] = starts
    intervals[:len(ends), 1] = ends
    if scan_begin + scan_len >= 2 ** 31:
        raise ConvertError("%s: a scan of %d bytes" % (name, scan_len))
    return JpegInfo(height, width, comps, hs, vs, mcu_w, mcu_h, mcus, 1 if comps == 1 else hs * vs + 2, quant, tables,
                    scan_begin, scan_begin + scan_len, restart if restart < mcus else 0, intervals, sof)


def _parse_progressive(buf, name, frame, qt, pool, pooled, restart, pos, cut):
    """the scans of an SOF2 file from its first SOS (at `pos`) to EOI or the end of the file -> JpegInfo.  Every scan binds
    the tables and the restart interval in force at its own SOS.  Refused here, by name: what T.81 G.1.1.1 forbids, a
    file that ends before every coefficient has reached bit 0 (libjpeg smooths such files, so they are not bit-exact
    ground), and more scans, tables or intervals than the device record holds."""
    size = len(buf)

    def bad(why):
        return ConvertError("%s: progressive JPEG: %s" % (name, why))

    height, width, comp = frame
    comps = len(comp)
    if comps == 1:                                        # one component is never interleaved: 8 x 8 MCUs
        comp = [(comp[0][0], 1, 1, comp[0][3])]
    hs, vs = comp[0][1], comp[0][2]
    if (hs, vs) not in ((1, 1), (2, 1), (2, 2)) or any(c[1:3] != (1, 1) for c in comp[1:]):
        raise bad("sampling %s: only luma 1x1, 2x1 or 2x2 over 1x1 chroma is decoded" % " ".join("%dx%d" % c[1:3] for c in comp))
    quant = np.zeros((3, 64), np.uint8)
    for i, (_, _, _, tq) in enumerate(comp):
        if tq not in qt:
            raise bad("no quantisation table %d" % tq)
        quant[i] = qt[tq]
    mcu_w, mcu_h = -(-width // (8 * hs)), -(-height // (8 * vs))
    mcus = mcu_w * mcu_h
    # a scan of one component walks that component's own grid of blocks
    grid = [-(-(-(-width * h // hs)) // 8) * -(-(-(-height * v // vs)) // 8) for _, h, v, _ in comp]
    arr = np.frombuffer(buf, np.uint8)
    ff = np.flatnonzero(arr[:-1] == 0xFF)
    nxt = arr[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    stops = ff[~is_rst & (nxt != 0) & (nxt != 0xFF)]      # an FF that neither stuffs nor restarts nor fills ends a segment
    rsts = ff[is_rst]
    sent = np.full((comps, 64), -1, np.int64)             # the Al each coefficient was last sent at
    ids = [c[0] for c in comp]
    scans, parts, used, total = [], [], {}, 0
    while pos + 2 <= size:                                # the end of the file stands for EOI
        if buf[pos] != 0xFF:
            raise bad("byte %d is no marker" % pos)
        marker = buf[pos + 1]
        if marker == 0xFF:                                # fill byte
            pos += 1
            continue
        if marker == 0xD9:
            break
        if pos + 4 > size:
            raise cut("the segments between two scans")
        length = struct.unpack_from(">H", buf, pos + 2)[0]
        if length < 2 or pos + 2 + length > size:
            raise cut("segment FF %02X" % marker)
        body = buf[pos + 4:pos + 2 + length]
        pos += 2 + length
        if marker == 0xC4:
            for key, table in _read_dht(body, name + ": progressive JPEG", cut):
                pooled[key] = len(pool)
                pool.append(table)
        elif marker == 0xDD:
            if len(body) < 2:
                raise cut("the DRI segment")
            restart = struct.unpack_from(">H", body)[0]
        elif marker == 0xDB:
            raise bad("a DQT segment after the first scan")
        elif 0xE0 <= marker <= 0xEF or marker == 0xFE:
            pass
        elif marker != 0xDA:
            raise bad("marker FF %02X between two scans is not decoded" % marker)
        if marker != 0xDA:
            continue
        ns = body[0] if body else 0
        if not 1 <= ns <= comps or len(body) < 4 + 2 * ns:
            raise bad("a scan header of %d bytes for %d of the %d components" % (len(body), ns, comps))
        if len(scans) == MAX_SCANS:
            raise bad("more than %d scans" % MAX_SCANS)
        ss, se, ahal = body[1 + 2 * ns:4 + 2 * ns]
        ah, al = ahal >> 4, ahal & 15
        what = "scan %d (coefficients %d..%d, Ah %d, Al %d)" % (len(scans), ss, se, ah, al)
        try:
            members = [ids.index(body[1 + 2 * j]) for j in range(ns)]
        except ValueError:
            raise bad("%s names a component the frame does not have" % what)
        if len(set(members)) != ns:
            raise bad("%s names a component twice" % what)
        # T.81 G.1.1.1
        if ss > se or se > 63:
            raise bad("illegal progression: %s is no band" % what)
        if ss == 0 and se != 0:
            raise bad("illegal progression: %s mixes DC and AC coefficients" % what)
        if ss > 0 and ns != 1:
            raise bad("illegal progression: %s is an AC scan of %d components" % (what, ns))
        if al > 13 or ah > 13:
            raise bad("illegal progression: %s has a bit position above 13" % what)
        tables = [-1, -1, -1]
        for j, c in enumerate(members):
            if ss > 0 and sent[c, 0] < 0:
                raise bad("illegal progression: %s is an AC scan of component %d before its first DC scan" % (what, c))
            band = sent[c, ss:se + 1]
            if ah == 0:
                if (band >= 0).any():
                    raise bad("illegal progression: %s is a first scan over coefficients already sent" % what)
            else:
                if (band < 0).any():
                    raise bad("illegal progression: %s is a first scan of its band with Ah other than 0" % what)
                if (band != ah).any() or al != ah - 1:
                    raise bad("illegal progression: %s refines a band last sent at bit %s down to bit %d"
                              % (what, sorted(set(band.tolist())), al))
            sent[c, ss:se + 1] = al
            if ss > 0 or ah == 0:                         # a DC refinement scan reads no table
                key = (0x10 | (body[2 + 2 * j] & 15)) if ss > 0 else body[2 + 2 * j] >> 4
                if key not in pooled:
                    raise bad("no Huffman table %d of class %d at %s" % (key & 15, key >> 4, what))
                tables[c] = used.setdefault(pooled[key], len(used))
        if len(used) > MAX_TABLES:
            raise bad("more than %d Huffman tables" % MAX_TABLES)
        units = mcus if ns > 1 else grid[members[0]]
        per = restart if 0 < restart < units else units
        count = -(-units // per)
        if total + count > MAX_INTERVALS:
            raise bad("more than %d restart intervals" % MAX_INTERVALS)
        begin = pos
        k = int(np.searchsorted(stops, begin))
        end = int(stops[k]) if k < stops.size else size
        marks = rsts[np.searchsorted(rsts, begin):np.searchsorted(rsts, end)] - begin
        intervals = np.full((count, 2), end - begin, np.int32)
        starts = np.concatenate([[0], marks + 2])[:count]
        ends = np.concatenate([marks, [end - begin]])[:count]
        intervals[:len(starts), 0] = starts
        intervals[:len(ends), 1] = ends
        parts.append(intervals)
        scans.append(ScanInfo(tuple(members), ss, se, ah, al, tuple(tables), restart if restart < units else 0, begin, end,
                              total, count, 0))
        total += count
        pos = end
    if not scans:
        raise bad("no scan")
    if (sent != 0).any():
        c, k = [int(v[0]) for v in np.nonzero(sent != 0)]
        raise bad("incomplete progressive JPEG: coefficient %d of component %d %s when the file ends" % (
            k, c, "was never sent" if sent[c, k] < 0 else "has reached bit %d only" % sent[c, k]))
    if scans[-1].end - scans[0].begin >= 2 ** 31:
        raise bad("scans of %d bytes" % (scans[-1].end - scans[0].begin))
    levels = scan_levels([(s.comps, s.ss, s.se) for s in scans])
    scans = tuple(s._replace(level=v) for s, v in zip(scans, levels))
    tables = np.zeros((max(len(used), 1), HUFF_BYTES), np.uint8)
    for src, dst in used.items():
        tables[dst] = pool[src]
    return JpegInfo(height, width, comps, hs, vs, mcu_w, mcu_h, mcus, 1 if comps == 1 else hs * vs + 2, quant, None,
                    scans[0].begin, scans[-1].end, 0, np.concatenate(parts), 0xC2, scans, tables)


def pack_progressive_group(files, infos):
    """what one launch of the progressive entropy stage reads, as host arrays: (data uint8: each file from its first scan to
    the end of its last, back to back; img int64 [n,4]; scans int32 [total,SCAN_FIELDS]; intervals int32 [total,2]; huff
    uint8 [tables,HUFF_BYTES]; quant uint8 [n,3,64]) - the layout of include/acimg.h"""
    n = len(files)
    segs, img, rows, at, first_interval, first_table = [], np.zeros((n, 4), np.int64), [], 0, 0, 0
    for i, (f, info) in enumerate(zip(files, infos)):
        seg = np.frombuffer(f, np.uint8)[info.scan_begin:info.scan_end]
        segs.append(seg)
        img[i] = (at, at + seg.size, len(rows), len(info.scans))
        for s in info.scans:
            mask = sum(1 << c for c in s.comps)
            rows.append([mask, s.ss, s.se, s.ah, s.al] + [t + first_table if t >= 0 else -1 for t in s.tables] +
                        [s.restart, s.begin - info.scan_begin, s.end - info.scan_begin, first_interval + s.first_interval,
                         s.level, 0, 0, 0])
        at += seg.size
        first_interval += len(info.intervals)
        first_table += len(info.pool)
    data = np.concatenate(segs) if at else np.zeros(1, np.uint8)
    arrays = (data, img, np.array(rows, np.int32).reshape(-1, SCAN_FIELDS), np.concatenate([i.intervals for i in infos]),
              np.concatenate([i.pool for i in infos]), np.stack([i.quant for i in infos]))
    return tuple(np.ascontiguousarray(a) for a in arrays)


def pack_group(files, infos):
    """what one launch reads, as host arrays: (data uint8: the entropy-coded segments back to back, desc int64 [n,4],
    intervals int32 [total,2], huff uint8 [n,6,HUFF_BYTES], quant uint8 [n,3,64]) - the layout of include/acimg.h"""
    n = len(files)
    segs, desc, at, first = [], np.zeros((n, 4), np.int64), 0, 0
    for i, (f, info) in enumerate(zip(files, infos)):
        seg = np.frombuffer(f, np.uint8)[info.scan_begin:info.scan_end]
        segs.append(seg)
        desc[i] = (at, at + seg.size, info.restart_mcus, first)
        at += seg.size
        first += len(info.intervals)
    data = np.concatenate(segs) if at else np.zeros(1, np.uint8)
    arrays = (data, desc, np.concatenate([i.intervals for i in infos]), np.stack([i.huff for i in infos]),
              np.stack([i.quant for i in infos]))
    return tuple(np.ascontiguousarray(a) for a in arrays)


def group_key(info):
    """what the files of one launch share: height, width, components, sampling, and the process (sequential or progressive)"""
    return (info.height, info.width, info.comps, info.hs, info.vs, info.scans is not None)


class JpegDecoder(object):
    """Sequential and progressive JPEG files -> B, G, R pixels on `device`.  `decode(files)` groups the files by geometry
    (height, width, components, sampling) and process, runs the three stages once per group and returns (pixels, status): per file a uint8 [H,W,3]
    device tensor (a view of its group's tensor) and the int32 status the entropy stage gave it (0 = ok; the pixels of any
    other are what its partly zero coefficients give)."""

    def __init__(self, device):
        self.device = torch.device(device)
        self.lib = _lib.load()

    def upload(self, files, infos):
        """the entropy-coded segments of one group, their descriptors and tables, on the device: `pack_group`'s five arrays
        for sequential files, `pack_progressive_group`'s six for progressive ones"""
        pack = pack_group if infos[0].scans is None else pack_progressive_group
        return tuple(torch.from_numpy(a).to(self.device) for a in pack(files, infos))

    def stages(self, files, infos, coef=None, planes=None, bgr=None, status=None):
        """one group through the three kernels (the entropy stage is the progressive kernel for a group of progressive
        files); buffers are allocated where the caller gives none ->
        (coef int16 [n,mcus,blocks,64], planes uint8 [n, blocks * mcus * 64], bgr uint8 [n,H,W,3], status int32 [n])"""
        L, g, n = self.lib, infos[0], len(files)
        geo = (g.height, g.width, g.comps, g.hs, g.vs)
        if any((i.height, i.width, i.comps, i.hs, i.vs) != geo for i in infos):
            raise ValueError("the images of one launch share height, width, components and sampling")
        progressive = g.scans is not None
        if any((i.scans is not None) != progressive for i in infos):
            raise ValueError("the images of one launch are all sequential or all progressive")
        up = self.upload(files, infos)
        quant = up[-1]
        dev = self.device
        if coef is None:
            coef = torch.empty(n, g.mcus, g.blocks, 64, dtype=torch.int16, device=dev)
        if planes is None:
            planes = torch.empty(n, g.blocks * g.mcus * 64, dtype=torch.uint8, device=dev)
        if bgr is None:
            bgr = torch.empty(n, g.height, g.width, 3, dtype=torch.uint8, device=dev)
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=dev)
        st = ops.current_stream_handle(dev)
        if progressive:
            data, img, scans, intervals, huff = up[:5]
            _lib.check(L.acimg_jpeg_decode_progressive(data.data_ptr(), data.numel(), img.data_ptr(), scans.data_ptr(),
                                                       scans.shape[0], intervals.data_ptr(), intervals.shape[0],
                                                       huff.data_ptr(), huff.shape[0], n, *geo, coef.data_ptr(),
                                                       coef.numel() * 2, status.data_ptr(), st), "jpeg_decode_progressive")
        else:
            data, desc, intervals, huff = up[:4]
            _lib.check(L.acimg_jpeg_decode_entropy(data.data_ptr(), data.numel(), desc.data_ptr(), intervals.data_ptr(),
                                                   intervals.shape[0], huff.data_ptr(), n, *geo, coef.data_ptr(),
                                                   coef.numel() * 2, status.data_ptr(), st), "jpeg_decode_entropy")
        _lib.check(L.acimg_jpeg_decode_idct(coef.data_ptr(), quant.data_ptr(), n, *geo, planes.data_ptr(), planes.numel(), st),
                   "jpeg_decode_idct")
        _lib.check(L.acimg_jpeg_decode_colour(planes.data_ptr(), n, *geo, bgr.data_ptr(), bgr.numel(), st), "jpeg_decode_colour")
        return coef, planes, bgr, status

    def decode(self, files, names=None, infos=None):
        """files: a list of whole files (bytes) -> ([uint8 [H,W,3] device tensor per file], int32 [files] status on the host)"""
        names = names or ["<jpeg %d>" % i for i in range(len(files))]
        infos = infos or [parse_jpeg(f, nm) for f, nm in zip(files, names)]
        groups = collections.OrderedDict()
        for i, info in enumerate(infos):
            groups.setdefault(group_key(info), []).append(i)
        pixels, status, parts = [None] * len(files), np.zeros(len(files), np.int32), []
        for members in groups.values():
            _, _, bgr, st = self.stages([files[i] for i in members], [infos[i] for i in members])
            for k, i in enumerate(members):
                pixels[i] = bgr[k]
            parts.append((members, st))
        for members, st in parts:                          # one read-back per group, after every launch is queued
            status[members] = st.cpu().numpy()
        return pixels, status


def decode_jpeg(data, device="cuda:0", name="<jpeg>"):
    """one sequential or progressive file -> uint8 [H,W,3] B, G, R on the host; a corrupt scan is a ConvertError"""
    pixels, status = JpegDecoder(device).decode([data], [name])
    if status[0]:
        raise ConvertError("%s: corrupt JPEG scan: %s" % (name, STATUS_TEXT.get(int(status[0]), status[0])))
    return pixels[0].cpu().numpy()
