"""Progressive JPEG on the device: `acimg_jpeg_decode_progressive` through the raw C ABI with every operand inside guard
bands, stage by stage against the restatement (tests/jpeg_progressive_ref.py), against Pillow's pixels of the committed
fixture and against the coefficients the writer cases were written from; sequential and progressive files in one `decode`
call; a launch of five whose third is corrupt in four ways; `python -m acimg.convert_boxes` on progressive files against
their baseline twins; an SOF1 file."""
import os
import sys

import numpy as np
import pytest
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import convert_boxes_support as support  # noqa: E402
import jpeg_decode_ref as jref  # noqa: E402
import jpeg_progressive_cases as pc  # noqa: E402
import jpeg_progressive_ref as pref  # noqa: E402
from guard_arena import GuardArena  # noqa: E402

pytestmark = pytest.mark.gpu

SENT = 0x7B
FIVE = ("smooth_420_37x53", "restart3_420_37x53", "noise_420_37x53", "restart1_420_37x53", "restart5_420_37x53")
REFINEMENT_SCAN = 5       # of Pillow's ten: Y 1..63, Ah 2, Al 1
FLIP_AT = 12              # byte of that scan of noise_420_37x53 whose complement the restatement cannot decode


@pytest.fixture(scope="module")
def golden():
    return pref.load_progressive_golden()


@pytest.fixture(scope="module")
def baseline():
    return jref.load_golden()


def restate(data):
    """-> (coef, planes, bgr) of the restatement, read-only"""
    w = pref.walk_progressive(data)
    assert w.status == 0 and w.complete and w.slack == 0
    planes = jref.idct(w, w.coef)
    arrays = (w.coef, np.concatenate([p.reshape(-1) for p in planes]), jref.colour(w, planes))
    for a in arrays:
        a.setflags(write=False)
    return arrays


@pytest.fixture(scope="module")
def restated(golden):
    return {name: restate(data) for name, (data, _) in golden.items()}


def device_decode_progressive(device, files, what="", tamper=None):
    """one launch of each stage on progressive `files` (one geometry) -> (coef, planes, bgr, status) as host arrays.  Inputs
    and outputs lie in one guard arena; the outputs are pre-filled with a sentinel (the entropy stage zeroes its slot
    itself) and the bands are checked after every stage.  tamper(host arrays as a list): changes them before the upload"""
    from acimg import _lib, jpeg, ops
    L = _lib.load()
    infos = [jpeg.parse_jpeg(f, "%s[%d]" % (what, i)) for i, f in enumerate(files)]
    g, n = infos[0], len(files)
    assert all(i.scans is not None for i in infos)
    geo = (g.height, g.width, g.comps, g.hs, g.vs)
    host = list(jpeg.pack_progressive_group(files, infos))
    if tamper is not None:
        tamper(host)
    sizes = dict(coef=n * g.mcus * g.blocks * 128, planes=n * g.mcus * g.blocks * 64, bgr=n * g.height * g.width * 3, status=4 * n)
    assert int(L.acimg_jpeg_decode_coef_bytes(n, *geo)) == sizes["coef"]
    arena = GuardArena.for_sizes(device, [a.nbytes for a in host] + list(sizes.values()))
    ins = []
    for a, name in zip(host, ("data", "img", "scans", "intervals", "huff", "quant")):
        r = arena.region(a.nbytes, name=name)
        r.u8.copy_(torch.from_numpy(a.reshape(-1).view(np.uint8)))
        ins.append(r)
    data, img, scans, intervals, huff, quant = ins
    outs = {k: arena.region(v, fill=SENT, name=k) for k, v in sizes.items()}
    st = ops.current_stream_handle(device)
    rc = L.acimg_jpeg_decode_progressive(data.ptr, host[0].nbytes, img.ptr, scans.ptr, host[2].shape[0], intervals.ptr,
                                         host[3].shape[0], huff.ptr, host[4].shape[0], n, *geo, outs["coef"].ptr, sizes["coef"],
                                         outs["status"].ptr, st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " progressive entropy")
    assert (outs["planes"].u8 == SENT).all() and (outs["bgr"].u8 == SENT).all(), what
    rc = L.acimg_jpeg_decode_idct(outs["coef"].ptr, quant.ptr, n, *geo, outs["planes"].ptr, sizes["planes"], st)
    assert rc == 0, _lib.last_error()
    rc = L.acimg_jpeg_decode_colour(outs["planes"].ptr, n, *geo, outs["bgr"].ptr, sizes["bgr"], st)
    assert rc == 0, _lib.last_error()
    torch.cuda.synchronize(device)
    arena.check(what + " idct and colour")
    for r, a in zip(ins, host):
        assert np.array_equal(r.u8.cpu().numpy(), a.reshape(-1).view(np.uint8)), "%s: input %s was written" % (what, r.name)
    return (outs["coef"].u8.cpu().numpy().view(np.int16).reshape(n, g.mcus, g.blocks, 64),
            outs["planes"].u8.cpu().numpy().reshape(n, -1), outs["bgr"].u8.cpu().numpy().reshape(n, g.height, g.width, 3),
            outs["status"].u8.cpu().numpy().view(np.int32))


def assert_progressive_stages(got, k, want, pillow, name):
    coef, planes, bgr, status = got
    assert status[k] == 0, "%s: status %d" % (name, status[k])
    pairs = [("coefficients", coef[k], want[0]), ("planes", planes[k], want[1]), ("pixels", bgr[k], want[2])]
    if pillow is not None:
        pairs.append(("pixels against Pillow", bgr[k], pillow))
    for stage, g, w in pairs:
        assert g.shape == w.shape and np.array_equal(g, w), "%s: %s differ at %d of %d places" % (
            name, stage, int((g != w).sum()), w.size)


def test_every_fixture_stream_stage_by_stage(device, golden, restated):
    for name, (data, pillow) in golden.items():
        assert_progressive_stages(device_decode_progressive(device, [data], name), 0, restated[name], pillow, name)


@pytest.mark.parametrize("name", list(pc.cases()))
def test_every_writer_case_gives_back_its_coefficients(device, name):
    """the oracle is what the writer was given, independent of the restatement; the later stages against the restatement"""
    case = pc.cases()[name]
    got = device_decode_progressive(device, [case.data], name)
    assert got[3].tolist() == [0], (name, got[3])
    bad = np.argwhere(got[0][0] != case.coef)
    assert bad.size == 0, "%s: %d coefficients differ, first at %s: %d against %d" % (
        name, len(bad), bad[0].tolist(), got[0][0][tuple(bad[0])], case.coef[tuple(bad[0])])
    assert_progressive_stages(got, 0, restate(case.data), None, name)


def test_two_runs_of_a_batch_give_the_same_bytes(device, golden, restated):
    files = [golden[n][0] for n in FIVE]
    a, b = device_decode_progressive(device, files, "five"), device_decode_progressive(device, files, "five again")
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    for k, name in enumerate(FIVE):
        assert_progressive_stages(a, k, restated[name], golden[name][1], name)


def _first_bad_record(host, image, info):
    """the restatement's verdict on the scan records of one image, in order"""
    img, scans, intervals, huff = host[1], host[2], host[3], host[4]
    grid = [info.mcus, info.mcus, info.mcus]
    grid[0] = -(-info.width // 8) * -(-info.height // 8)

    def units_of(mask):
        return info.mcus if mask & (mask - 1) else grid[mask.bit_length() - 1]
    first, count = int(img[image, 2]), int(img[image, 3])
    for k in range(count):
        s = pref.record_status(scans[first + k], info.comps, count, huff.shape[0], intervals.shape[0], units_of)
        if s:
            return s
    return 0


@pytest.mark.parametrize("form", ("cut mid-scan in an early scan", "cut in the last scan", "flipped byte in an AC refinement",
                                  "garbage scan records"))
def test_corrupt_third_image_of_five(device, golden, restated, form):
    """five images with their own tables and restart intervals of 0, 3, 0, 1 and 5 in one launch; the third is corrupt: it
    ends with the restatement's status, the other four are exact, nothing leaves the operands"""
    from acimg import jpeg
    files = [golden[n][0] for n in FIVE]
    good = files[2]
    info = jpeg.parse_jpeg(good)
    tamper, seen = None, {}
    if form == "cut mid-scan in an early scan":
        s = info.scans[1]
        files[2] = good[:s.begin + (s.end - s.begin) // 2] + good[s.end:]
        want = jref.STATUS_EARLY_END
    elif form == "cut in the last scan":
        s = info.scans[-1]
        files[2] = good[:s.begin + (s.end - s.begin) // 2]
        want = jref.STATUS_EARLY_END
    elif form == "flipped byte in an AC refinement":
        s = info.scans[REFINEMENT_SCAN]
        assert (s.ss, s.ah, s.al) == (1, 2, 1)
        at = s.begin + FLIP_AT
        files[2] = jref.patched(good, at, good[at] ^ 0xFF)
        changed = jpeg.parse_jpeg(files[2])
        assert [(c.begin, c.end, c.count) for c in changed.scans] == [(c.begin, c.end, c.count) for c in info.scans]
        want = None
    else:
        def tamper(host):
            seen["host"] = host
            first = int(host[1][2, 2])
            host[2][first + 4, 2] = 77                     # Se
            host[2][first + 6, 5] = 1 << 20                # a table outside the pool
            host[2][first + 8, 12] = -3                    # a level
            host[2][first + 9, :] = np.random.RandomState(9).randint(-2 ** 31, 2 ** 31, size=16)
        want = pref.STATUS_DESCRIPTOR
    if form != "garbage scan records":
        restatement = pref.walk_progressive(files[2]).status
        assert restatement != 0 and want in (None, restatement), (form, restatement)
        want = restatement
    got = device_decode_progressive(device, files, form, tamper=tamper)
    if tamper:
        assert _first_bad_record(seen["host"], 2, info) == want
    print("%s: status %s, the restatement's %d" % (form, got[3].tolist(), want))
    assert got[3][2] != 0 and got[3][2] == want
    for k, name in enumerate(FIVE):
        if k != 2:
            assert_progressive_stages(got, k, restated[name], golden[name][1], name)


def test_refusals_before_any_launch(device):
    from acimg import _lib
    L = _lib.load()
    buf = torch.zeros(65536, dtype=torch.uint8, device=device)
    p = buf.data_ptr()
    ok = (p, 16, p, p, 1, p, 1, p, 1, 1, 8, 8, 3, 2, 2, p, 65536, p, None)

    def call(**change):
        a = list(ok)
        for k, v in change.items():
            a[int(k[1:])] = v
        return L.acimg_jpeg_decode_progressive(*a)
    assert call(a0=None) == -1 and call(a3=None) == -1 and call(a17=None) == -1
    assert call(a13=1, a14=2) == -1 and "sampling 1 x 2" in _lib.last_error()
    assert call(a4=0) == -1 and call(a6=0) == -1 and call(a8=0) == -1 and call(a9=0) == -1
    assert call(a15=p + 2) == -1 and call(a2=p + 8) == -1 and call(a3=p + 4) == -1
    assert call(a16=767) == -2
    torch.cuda.synchronize(device)
    assert not buf.any()


def test_sequential_and_progressive_files_in_one_call(device, golden, baseline):
    from acimg import jpeg
    from acimg.convert import ConvertError
    names = [("p", "noise_420_37x53"), ("b", "noise_420_37x53"), ("p", "grey_17x9"), ("b", "smooth_422_1x1"), ("p", "smooth_422_1x1"),
             ("p", "restart1_420_37x53"), ("b", "grey_17x9"), ("p", "smooth_420_37x53")]
    files = [(golden if kind == "p" else baseline)[n][0] for kind, n in names]
    infos = [jpeg.parse_jpeg(f) for f in files]
    assert len({jpeg.group_key(i) for i in infos}) == 6
    pixels, status = jpeg.JpegDecoder(device).decode(files, ["%s:%s" % kn for kn in names])
    assert status.dtype == np.int32 and not status.any()
    for (kind, n), p in zip(names, pixels):
        want = (golden if kind == "p" else baseline)[n][1]
        assert p.device.type == "cuda" and p.dtype == torch.uint8 and np.array_equal(p.cpu().numpy(), want), (kind, n)
    assert np.array_equal(jpeg.decode_jpeg(golden["q5_noise_420_40x72"][0], device), golden["q5_noise_420_40x72"][1])
    with pytest.raises(ConvertError, match="x.jpg: corrupt JPEG scan"):
        jpeg.decode_jpeg(golden["noise_420_37x53"][0][:-40], device, "x.jpg")


def test_an_sof1_file_decodes_to_its_sof0_pixels(device, baseline):
    from acimg import jpeg
    for name in ("optimize_420_37x53", "grey_17x9", "restart3_420_37x53"):
        data, want = baseline[name]
        sof1 = jref.patched(data, jref.payload_offset(data, 0xC0) - 3, 0xC1)
        assert jpeg.parse_jpeg(sof1).sof == 0xC1
        assert np.array_equal(jpeg.decode_jpeg(sof1, device, name), want), name


def test_convert_boxes_on_progressive_files_equals_the_baseline_twins(device, golden, baseline, tmp_path):
    """the same pictures as baseline and as progressive files: the pixels are equal, so the records are, byte for byte"""
    from acimg import convert_boxes as cb
    from acimg import tfio
    records = {}
    for kind, files in (("baseline", baseline), ("progressive", golden)):
        raw, out = tmp_path / kind / "raw", tmp_path / kind / "out"
        (raw / "Dataset" / "Annotations").mkdir(parents=True)
        (raw / "Dataset" / "Data" / "0").mkdir(parents=True)
        out.mkdir()
        for ident, name in (("2001", "smooth_420_256x256"), ("2002", "restart3_420_37x53"), ("2003", "smooth_420_256x256")):
            (raw / "Dataset" / "Data" / "0" / (ident + ".jpg")).write_bytes(files[name][0])
            (raw / "Dataset" / "Annotations" / (ident + ".xml")).write_bytes(
                support.annotation_xml(ident, [("object", 64, 4, 192, 12)]))
        (raw / "test_list.txt").write_text("2001.jpg\n2002.jpg\n2003.jpg\n")
        assert cb.main([str(raw), str(out), "--device", str(device), "--modalities", "2"]) == 0
        records[kind] = {f: list(tfio.read_tfrecord(str(out / f))) for f in sorted(os.listdir(str(out)))}
    assert sorted(records["baseline"]) == ["2001.tfrecord", "2002.tfrecord", "2003.tfrecord"]
    assert records["progressive"] == records["baseline"]
