"""What the PNG cases (tests/png_cases.py) reach, counted by walking every case's file with the restatement
(tests/png_decode_ref.py): each filter on a first row and on a later row, Paeth choosing left, up and upleft and each of
its ties, Average with a sum of 256 or more, every colour-type / depth form, every Adam7 pass present and absent, a band
edge crossed.  `missing()` names what is no longer reached, so a change of the cases cannot leave softer tests behind."""
import collections
import functools

import png_cases
import png_decode_ref as ref

REQUIRED = (["filter %d on a %s row" % (f, r) for f in range(5) for r in ("first", "later")] +
            ["paeth chooses " + w for w in "abc"] + ["paeth tie " + t for t in ("a=b=c", "a=b", "a=c", "b=c")] +
            ["average with a sum of 256 or more", "sum wraps"] +
            ["form colour type %d depth %d" % f for f in ref.FORMS] +
            ["form colour type %d depth %d interlaced" % f for f in ref.FORMS] +
            ["adam7 pass %d %s" % (p, s) for p in range(7) for s in ("present", "absent") if (p, s) != (0, "absent")] +   # pass 0 holds pixel (0, 0)

            ["band edge crossed with filter %d" % f for f in range(5)] +
            ["filter unit %d" % b for b in (1, 2, 3, 4, 6, 8)])


@functools.lru_cache(maxsize=None)
def count_cases():
    """-> Counter over every case"""
    count = collections.Counter()
    for name, data in png_cases.files().items():
        hdr = ref.png_header(data)
        form = "form colour type %d depth %d" % (hdr.colour_type, hdr.bit_depth)
        count[form + (" interlaced" if hdr.interlace else "")] += 1
        count["filter unit %d" % ref.bpp_of(hdr.colour_type, hdr.bit_depth)] += 1
        if hdr.interlace:
            present = {p.index for p in ref.passes(hdr.height, hdr.width, hdr.colour_type, hdr.bit_depth, 1)}
            for p in range(7):
                count["adam7 pass %d %s" % (p, "present" if p in present else "absent")] += 1
        ref.unfilter(ref.inflate_idat(hdr), hdr, count)
    return count


def missing():
    c = count_cases()
    return [k for k in REQUIRED if not c[k]]
