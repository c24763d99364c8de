"""The progressive decoder's host side without a GPU: the restatement (tests/jpeg_progressive_ref.py) against Pillow's pixels
of the committed fixture, bit for bit; the writer (tests/jpeg_progressive_writer.py) through the restatement back to its
coefficients; the census of what the case set reaches; the level rule; `parse_jpeg` on SOF2 and SOF1 files - agreement with
the restatement's sequential walk, every refusal by name - and unchanged on baseline files; the C entry point's refusals
through fake pointers.  No Pillow here."""
import collections
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import jpeg_decode_ref as jref  # noqa: E402
import jpeg_progressive_cases as pc  # noqa: E402
import jpeg_progressive_ref as pref  # noqa: E402
import jpeg_progressive_writer as pw  # noqa: E402

PILLOW_LEVELS = [0, 0, 0, 0, 0, 1, 1, 1, 1, 2]


@pytest.fixture(scope="module")
def golden():
    return pref.load_progressive_golden()


@pytest.fixture(scope="module")
def walks(golden):
    """name -> the restatement's walk of every fixture file and writer case, with one census over all of them"""
    census = collections.Counter()
    out = collections.OrderedDict((name, pref.walk_progressive(data, census)) for name, (data, _) in golden.items())
    for name, case in pc.cases().items():
        out[name] = pref.walk_progressive(case.data, census)
    out["census"] = census
    return out


def test_fixture_holds_the_cases(golden):
    assert len(golden) == 39
    shapes = {(p.shape[1], p.shape[0]) for _, p in golden.values()}
    assert shapes >= {(1, 1), (17, 9), (16, 16), (24, 24), (37, 53), (8, 24), (40, 72), (256, 256)}
    px = golden["q5_noise_420_40x72"][1]
    assert px.min() == 0 and px.max() == 255
    assert os.path.getsize(os.path.join(HERE, "golden", "jpeg_progressive_golden.npz")) <= 200000


def test_restatement_equals_pillow_bit_for_bit(golden, walks):
    for name, (_, want) in golden.items():
        w = walks[name]
        assert w.status == 0 and w.complete and w.slack == 0, name
        got = jref.colour(w, jref.idct(w, w.coef))
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d of %d bytes differ" % (
            name, int((got != want).sum()), want.size)


def test_writer_files_give_back_their_coefficients(walks):
    for name, case in pc.cases().items():
        w = walks[name]
        assert w.status == 0 and w.complete and w.slack == 0, name
        assert (w.height, w.width, w.comps, w.hs, w.vs) == case.geometry
        assert [(tuple(s.comps), s.ss, s.se, s.ah, s.al) for s in w.scans] == list(case.script), name
        assert np.array_equal(w.coef, case.coef), "%s: %d coefficients differ" % (name, int((w.coef != case.coef).sum()))


def test_census_is_complete(walks):
    census = walks["census"]
    print()
    for key in pref.CENSUS:
        print("%-40s %d" % (key, census[key]))
    missing = [k for k in pref.CENSUS if not census[k]]
    assert not missing, "the case set no longer reaches: %s" % ", ".join(missing)
    # the big picture is one run of 129 * 128 - 1 blocks; the restart cases count MCUs in DC scans and blocks in AC scans
    assert len(walks["eob_run_category_14_grey_1032x1024"].scans[1].offsets) == 1
    r1 = walks["restart1_420_37x53"]
    assert [len(s.offsets) for s in r1.scans] == [12, 35, 12, 12, 35, 35, 12, 12, 12, 35]      # RSTn wraps past 7


def test_level_rule(golden, walks):
    from acimg import jpeg
    assert pref.levels(pw.PILLOW_SCRIPT_3) == PILLOW_LEVELS
    assert jpeg.scan_levels([s[:3] for s in pw.PILLOW_SCRIPT_3]) == PILLOW_LEVELS
    info = jpeg.parse_jpeg(golden["noise_420_24x24"][0])
    assert [(s.comps, s.ss, s.se, s.ah, s.al) for s in info.scans] == pw.PILLOW_SCRIPT_3
    assert [s.level for s in info.scans] == PILLOW_LEVELS
    assert [s.level for s in jpeg.parse_jpeg(golden["grey_17x9"][0]).scans] == pref.levels(pw.PILLOW_SCRIPT_1) == [0, 0, 0, 1, 1, 2]
    for name, case in pc.cases().items():
        got = [s.level for s in jpeg.parse_jpeg(case.data).scans]
        assert got == pref.levels(case.script), name
        # scans of one level touch disjoint coefficients
        for lv in set(got):
            seen = set()
            for s, l in zip(case.script, got):
                if l == lv:
                    cells = {(c, k) for c in s[0] for k in range(s[1], s[2] + 1)}
                    assert not cells & seen, (name, lv)
                    seen |= cells
    assert max(s.level for s in jpeg.parse_jpeg(pc.cases()["one_band_per_coefficient_444_9x9"].data).scans) == 0


def test_parser_agrees_with_the_restatement(golden, walks):
    """geometry, scan headers, the tables each scan binds, each scan's byte range and the restart offsets the byte search
    finds against those the restatement meets while it walks the bits"""
    from acimg import jpeg
    files = [(n, d) for n, (d, _) in golden.items()] + [(n, c.data) for n, c in pc.cases().items()]
    for name, data in files:
        info, w = jpeg.parse_jpeg(data, name), walks[name]
        assert (info.height, info.width, info.comps, info.hs, info.vs) == (w.height, w.width, w.comps, w.hs, w.vs)
        assert (info.mcu_w, info.mcu_h, info.mcus, info.blocks) == (w.mcu_w, w.mcu_h, w.mcus, w.blocks)
        assert info.sof == 0xC2 and info.huff is None and info.restart_mcus == 0 and len(info.scans) == len(w.scans)
        assert all(np.array_equal(info.quant[c], w.quant[c]) for c in range(w.comps))
        assert (info.scan_begin, info.scan_end) == (w.scans[0].begin, w.scans[-1].end)
        assert len(info.intervals) == sum(s.count for s in info.scans)
        for s, r in zip(info.scans, w.scans):
            assert (list(s.comps), s.ss, s.se, s.ah, s.al) == (r.comps, r.ss, r.se, r.ah, r.al), name
            assert (s.begin, s.end) == (r.begin, r.end), name
            mine = info.intervals[s.first_interval:s.first_interval + s.count]
            assert mine[:, 0].tolist() == r.offsets, name
            assert mine[1:, 0].tolist() == (mine[:-1, 1] + 2).tolist() and mine[-1, 1] == s.end - s.begin
            for c in range(info.comps):
                reads = c in s.comps and not (s.ss == 0 and s.ah)
                assert (s.tables[c] >= 0) == reads, name
                if reads:                                     # the pooled table decodes like the restatement's look-up
                    t = info.pool[s.tables[c]]
                    look, want = t[:512].view(np.uint16), (r.dc[c] if s.ss == 0 else r.ac)
                    assert all(int(look[b >> 8]) in (0, int(want[b])) for b in range(0, 65536, 257)), name
    host = jpeg.pack_progressive_group([golden["noise_420_24x24"][0]] * 2, [jpeg.parse_jpeg(golden["noise_420_24x24"][0])] * 2)
    data, img, scans, intervals, huff, quant = host
    assert img.dtype == np.int64 and img[:, 2:].tolist() == [[0, 10], [10, 10]] and img[1, 0] == img[0, 1]
    assert scans.dtype == np.int32 and scans.shape == (20, jpeg.SCAN_FIELDS) and scans[:10, 12].tolist() == PILLOW_LEVELS
    assert scans[0, :5].tolist() == [7, 0, 0, 0, 1] and scans[6, 5:8].tolist() == [-1, -1, -1]
    assert (scans[10:, 5:8][scans[10:, 5:8] >= 0] >= huff.shape[0] // 2).all() and scans[10, 11] == len(intervals) // 2
    assert huff.shape[1] == jpeg.HUFF_BYTES and quant.shape == (2, 3, 64)


def _patch_scan(data, k, **fields):
    """the file with Ss / Se / Ah / Al of its k-th SOS changed"""
    pos, seen = 2, 0
    while True:
        marker, length = data[pos + 1], struct.unpack_from(">H", data, pos + 2)[0]
        if marker == 0xDA:
            if seen == k:
                ns = data[pos + 4]
                at = pos + 5 + 2 * ns
                ss, se, ah, al = data[at], data[at + 1], data[at + 2] >> 4, data[at + 2] & 15
                ss, se = fields.get("ss", ss), fields.get("se", se)
                ah, al = fields.get("ah", ah), fields.get("al", al)
                return data[:at] + bytes((ss, se, ah << 4 | al)) + data[at + 3:]
            seen += 1
            pos += 2 + length
            while not (data[pos] == 0xFF and data[pos + 1] not in (0, 0xFF) and not 0xD0 <= data[pos + 1] <= 0xD7):
                pos += 1
        else:
            pos += 2 + length


def test_parser_refusals_by_name(golden):
    from acimg import jpeg
    from acimg.convert import ConvertError
    cases = pc.cases()
    spectral, deep = cases["spectral_only_420_24x24"].data, cases["three_bits_deep_422_17x9"].data
    assert [s[1:] for s in cases["spectral_only_420_24x24"].script[:5]] == [(0, 0, 0, 0), (1, 5, 0, 0), (1, 5, 0, 0), (1, 5, 0, 0),
                                                                             (6, 20, 0, 0)]
    assert [s[1:] for s in cases["three_bits_deep_422_17x9"].script[:4]] == [(0, 0, 0, 2), (0, 0, 2, 1), (0, 0, 1, 0), (1, 63, 0, 2)]
    g1 = (8, 8, 1, 1, 1)
    one = np.zeros((1, 1, 64), np.int16)
    one[0, 0, :] = 5
    q = [np.ones(64, np.uint8)]
    info = jpeg.parse_jpeg(spectral)
    many = [((0,), 0, 0, 0, 13)] + [((0,), 0, 0, a, a - 1) for a in range(13, 0, -1)]
    many += [((0,), k, k, 0, 3) for k in range(1, 64)] + [((0,), k, k, a, a - 1) for a in (3, 2, 1) for k in range(1, 64)]
    assert len(many) == 266
    baseline = jref.load_golden(jref.GOLDEN_FILES[:1])["noise_420_16x16"][0]
    refusals = [
        (_patch_scan(spectral, 0, se=5), "illegal progression.*mixes DC and AC"),
        (_three_component_ac_scan(), "illegal progression.*AC scan of 3 components"),
        (_patch_scan(spectral, 4, ss=21), "illegal progression.*no band"),
        (_patch_scan(spectral, 4, se=64), "illegal progression.*no band"),
        (pw.write(one, q, g1, [((0,), 1, 63, 0, 0), ((0,), 0, 0, 0, 0)]), "illegal progression.*before its first DC scan"),
        (_patch_scan(spectral, 0, ah=1), "illegal progression.*first scan of its band with Ah other than 0"),
        (_patch_scan(deep, 1, ah=1, al=0), "illegal progression.*refines a band last sent at bit"),
        (_patch_scan(deep, 1, ah=2, al=0), "illegal progression.*refines a band last sent at bit"),
        (_patch_scan(spectral, 4, ss=5), "illegal progression.*first scan over coefficients already sent"),
        (_patch_scan(spectral, 1, al=14), "illegal progression.*bit position above 13"),
        (spectral[:info.scans[-2].end] + b"\xFF\xD9", "incomplete progressive JPEG.*was never sent"),
        (spectral[:info.scans[-2].end], "incomplete progressive JPEG"),
        (pw.write(one, q, g1, [((0,), 0, 0, 0, 1), ((0,), 1, 63, 0, 0)]), "incomplete progressive JPEG.*has reached bit 1 only"),
        (pw.write(one, q, g1, many), "more than 256 scans"),
        (spectral[:info.scans[3].begin - 3], "truncated JPEG file.*segment FF DA"),
        (jref.as_progressive(baseline), "illegal progression"),
        (jref.patched(spectral, jref.payload_offset(spectral, 0xC2) + 7, 0x12), "sampling 1x2"),
        (jref.patched(spectral, jref.payload_offset(spectral, 0xC2), 12), "12-bit"),
    ]
    for bad, word in refusals:
        with pytest.raises(ConvertError, match=word) as e:
            jpeg.parse_jpeg(bad, "some/dir/frame.jpg")
        assert str(e.value).startswith("some/dir/frame.jpg: progressive JPEG"), str(e.value)
    # 255 scans and the complete script of 256 + are on either side of the cap: the longest script the cases hold is taken
    assert len(jpeg.parse_jpeg(cases["one_band_per_coefficient_444_9x9"].data).scans) == 190 <= jpeg.MAX_SCANS
    assert len(jpeg.parse_jpeg(pw.write(one, q, g1, many[:14] + [((0,), 1, 63, 0, 0)])).scans) == 15
    # still refused by name, as before: other processes, and sequential files split into several scans
    for marker, word in ((0xC9, "arithmetic"), (0xC3, "lossless"), (0xC5, "differential"), (0xCA, "arithmetic-coded progressive")):
        with pytest.raises(ConvertError, match=word):
            jpeg.parse_jpeg(jref.patched(spectral, jref.payload_offset(spectral, 0xC2) - 3, marker), "f.jpg")
    with pytest.raises(ConvertError, match="only one full scan"):
        jpeg.parse_jpeg(jref.patched(spectral, jref.payload_offset(spectral, 0xC2) - 3, 0xC0), "f.jpg")
    # a scan that ends early is the device's to report
    cut = spectral[:info.scans[-1].begin + 3]
    assert jpeg.parse_jpeg(cut).scans[-1].end == len(cut) and pref.walk_progressive(cut).status == jref.STATUS_EARLY_END


def _three_component_ac_scan():
    """a legal DC scan, then an AC scan that names all three components (the writer codes what it is told to)"""
    coef = np.zeros((1, 3, 64), np.int16)
    coef[..., :3] = 4
    return pw.write(coef, [np.ones(64, np.uint8)] * 3, (8, 8, 3, 1, 1), [((0, 1, 2), 0, 0, 0, 0), ((0, 1, 2), 1, 63, 0, 0)])


def test_an_sof1_file_parses_like_its_sof0_original():
    from acimg import jpeg
    for name, (data, _) in jref.load_golden().items():
        a = jpeg.parse_jpeg(data, name)
        b = jpeg.parse_jpeg(jref.patched(data, jref.payload_offset(data, 0xC0) - 3, 0xC1), name)
        assert (a.sof, b.sof) == (0xC0, 0xC1) and a.scans is None and b.scans is None and b.pool is None
        for x, y in zip(a[:15], b[:15]):
            assert np.array_equal(x, y), name
    # SOF1 may name tables 2 and 3: the host resolves tables per component
    data = jref.load_golden()["optimize_420_37x53"][0]
    sof1 = bytearray(jref.patched(data, jref.payload_offset(data, 0xC0) - 3, 0xC1))
    pos = 2
    while sof1[pos + 1] != 0xDA:
        if sof1[pos + 1] == 0xC4 and sof1[pos + 4] & 15 == 1:
            sof1[pos + 4] = (sof1[pos + 4] & 0xF0) | 3                # table 1 becomes table 3 ...
        pos += 2 + struct.unpack_from(">H", sof1, pos + 2)[0]
    for j in (1, 2):
        assert sof1[pos + 6 + 2 * j] == 0x11
        sof1[pos + 6 + 2 * j] = 0x33                                  # ... and the chroma components name it
    b = jpeg.parse_jpeg(bytes(sof1), "t3")
    assert np.array_equal(b.huff, jpeg.parse_jpeg(data).huff)


def test_baseline_files_are_parsed_and_packed_as_before():
    from acimg import jpeg
    fields = "height width comps hs vs mcu_w mcu_h mcus blocks quant huff scan_begin scan_end restart_mcus intervals".split()
    assert list(jpeg.JpegInfo._fields[:15]) == fields and jpeg.JpegInfo._fields[15:] == ("sof", "scans", "pool")
    golden = jref.load_golden(jref.GOLDEN_FILES[:1])
    names = ["noise_420_37x53", "restart3_420_37x53", "optimize_420_37x53"]
    infos = [jpeg.parse_jpeg(golden[n][0], n) for n in names]
    for info in infos:
        assert (info.sof, info.scans, info.pool) == (0xC0, None, None) and info.huff.shape == (6, jpeg.HUFF_BYTES)
    packed = jpeg.pack_group([golden[n][0] for n in names], infos)
    assert len(packed) == 5
    data, desc, intervals, huff, quant = packed
    assert desc.shape == (3, 4) and desc.dtype == np.int64 and huff.shape == (3, 6, jpeg.HUFF_BYTES) and quant.shape == (3, 3, 64)
    assert desc[:, 3].tolist() == [0, 1, 5] and desc[:, 2].tolist() == [0, 3, 0] and data.size == int(desc[-1, 1])
    assert jpeg.group_key(infos[0])[-1] is False


_BIG = (C.c_char * 8192)()
A = C.addressof(_BIG) + (-C.addressof(_BIG)) % 256          # a fake, 256-byte aligned "device pointer": never dereferenced


def test_entry_point_refusals_through_fake_pointers():
    """every call here must be refused before a launch: one that is not comes back as a launch error on a machine without
    a GPU, which the message then shows"""
    import __graft_entry__ as ge
    ge.build()
    from acimg import _lib
    L = _lib.load()
    ok = [A, 16, A, A, 1, A, 1, A, 1, 1, 8, 8, 3, 2, 2, A, 768, A, None]
    names = "data data_bytes img scans total_scans intervals total_intervals huff total_tables n H W comps hs vs coef " \
            "coef_bytes status stream".split()
    assert len(ok) == len(names)

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[names.index(k)] = v
        return L.acimg_jpeg_decode_progressive(*a)
    for pointer in ("data", "img", "scans", "intervals", "huff", "coef", "status"):
        assert call(**{pointer: None}) == -1 and "null" in _lib.last_error(), pointer
    for pointer in ("img", "scans", "intervals", "huff", "coef"):
        assert call(**{pointer: A + 8}) == -1 and "16-byte aligned" in _lib.last_error(), pointer
    for count in ("total_scans", "total_intervals", "total_tables", "n"):
        assert call(**{count: 0}) == -1, count
    assert call(hs=1, vs=2) == -1 and "sampling 1 x 2" in _lib.last_error()
    assert call(comps=4, hs=1, vs=1) == -1 and call(H=0) == -1 and call(W=65536) == -1
    assert call(coef_bytes=767) == -2 and "coef of 767 < 768" in _lib.last_error()
    assert call(n=2) == -2
