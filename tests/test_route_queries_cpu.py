"""What the host-side queries answer, pinned: for every descriptor and configuration of tests/golden/make_route_golden.py
the built library's workspace sizes, statistics rows, tilings, affine-input answers and split weight-image sizes must equal
tests/golden/route_queries.json exactly.  The C++ dispatch decides which kernel a descriptor runs on and what that kernel
needs; these queries are what it promises the Python host about that decision."""
import importlib.util
import os

import pytest

_GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
_spec = importlib.util.spec_from_file_location("make_route_golden", os.path.join(_GOLDEN_DIR, "make_route_golden.py"))
mk = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(mk)

# The entries allowed to differ from the build that made the golden: descriptors with an output of 2 GiB or more.  The launch
# has always run the one-tile kernel on them (its stores take 64-bit pointers; the persistent kernel's a 32-bit descriptor),
# but acimg_conv2d_fwd_split3_tiling used to report the persistent kernel (third word 1) where the tile count asked for it.
# It now reports 0.  {descriptor fields: reason}; every other answer about these descriptors is pinned like the rest.
TILING_CHANGED = {
    (512, 56, 75, 64, 64, 256, 256, 56, 75, 1, 1, 1, 0, 0, 256, 0): "batch-512 1x1 64 -> 256 at 56x75: a 2.2 GB output",
}


def expected(want, descs):
    """the golden, with the tiling's third word 1 -> 0 for the descriptors of TILING_CHANGED"""
    for i, d in enumerate(descs):
        if tuple(d) in TILING_CHANGED:
            for a in want.values():
                bm, bn, kind = a["acimg_conv2d_fwd_split3_tiling"][i]
                a["acimg_conv2d_fwd_split3_tiling"][i] = [bm, bn, 0 if kind == 1 else kind]
    return want


@pytest.fixture(scope="module")
def swept():
    import __graft_entry__ as ge

    ge.build()
    descs, want = mk.load_golden()
    return descs, expected(want, descs), mk.sweep(descs)


def test_golden_covers_the_configurations_and_queries(swept):
    descs, want, got = swept
    assert list(want) == [n for n, _ in mk.configurations()]
    assert len(descs) > 300 and len({tuple(d) for d in descs}) == len(descs)
    for name, a in want.items():
        assert list(a) == list(mk.QUERIES), name
        assert all(len(v) == len(descs) for v in a.values()), name
    big = {tuple(d) for d in descs if 4 * d[0] * d[7] * d[8] * d[6] >= 2 ** 31}                           # N * OH * OW * ldy
    assert big == set(TILING_CHANGED) and len(big) == 1
    i = [tuple(d) for d in descs].index(next(iter(big)))           # the one changed answer is in the sweep: persistent by tile count, reported as 0
    assert got["default"]["acimg_conv2d_fwd_split3_tiling"][i] == [128, 128, 0]


@pytest.mark.parametrize("name", [n for n, _ in mk.configurations()])
def test_query_answers_match_the_golden(swept, name):
    descs, want, got = swept
    for q in mk.QUERIES:
        if got[name][q] == want[name][q]:
            continue
        bad = [i for i, (a, b) in enumerate(zip(got[name][q], want[name][q])) if a != b]
        i = bad[0]
        pytest.fail("%s: %s differs on %d of %d descriptors, first on %s: the library answers %s, the golden has %s" % (
            name, q, len(bad), len(descs), dict(zip(mk.FIELDS, descs[i])), got[name][q][i], want[name][q][i]))
