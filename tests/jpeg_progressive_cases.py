"""The writer cases of the progressive decoder: coefficients and scan scripts that reach what Pillow's one script never
does (tests/jpeg_progressive_writer.py writes them).  `cases()` -> {name: Case(data, coef, geometry, script, restart)},
built once and never modified.  The coefficients are the oracle: a decoder must give them back."""
import collections
import functools

import numpy as np

import jpeg_progressive_writer as pw

Case = collections.namedtuple("Case", "data coef geometry script restart")
FLAT_QUANT = np.ones(64, np.uint8)


def _blocks(geometry):
    H, W, comps, hs, vs = geometry
    return -(-W // (8 * hs)) * -(-H // (8 * vs)), (hs * vs + 2 if comps == 3 else 1)


def _own_grid_mask(geometry):
    """bool [mcus][blocks]: the blocks a scan of one component reaches (luma blocks in the MCU padding are False)"""
    H, W, comps, hs, vs = geometry
    mcus, blocks = _blocks(geometry)
    mcu_w = -(-W // (8 * hs))
    mask = np.ones((mcus, blocks), bool)
    if comps == 3:
        rows, cols = -(-H // 8), -(-W // 8)
        for m in range(mcus):
            for q in range(hs * vs):
                br, bc = (m // mcu_w) * vs + q // hs, (m % mcu_w) * hs + q % hs
                mask[m, q] = br < rows and bc < cols
    return mask


def random_coef(geometry, seed, density=0.3, amplitude=40, dc=200, pad_dc=True):
    """sparse coefficients in the decoder's layout; AC of the luma padding blocks is zero (no scan of one component sends
    it), their DC too unless pad_dc (only an interleaved DC scan sends that)"""
    rng = np.random.RandomState(seed)
    mcus, blocks = _blocks(geometry)
    coef = rng.randint(-amplitude, amplitude + 1, size=(mcus, blocks, 64))
    coef *= rng.rand(mcus, blocks, 64) < density
    coef[..., 0] = rng.randint(-dc, dc + 1, size=(mcus, blocks))
    own = _own_grid_mask(geometry)
    coef[~own, 1:] = 0
    if not pad_dc:
        coef[~own, 0] = 0
    return coef.astype(np.int16)


def _script(comps, dc, ac):
    """dc: [(Ah, Al)] interleaved; ac: [(Ss, Se, Ah, Al)] for every component in turn"""
    members = tuple(range(comps))
    return [(members, 0, 0, ah, al) for ah, al in dc] + [((c,), ss, se, ah, al) for ss, se, ah, al in ac for c in members]


def _eob_runs(lengths, total):
    """grey coefficients of `total` blocks: runs of blocks without AC of the given lengths, one block with AC between two"""
    coef = np.zeros((total, 1, 64), np.int16)
    at = 0
    for n in lengths:
        at += n
        if at < total:
            coef[at, 0, 1] = 3
        at += 1
    assert at <= total + 1, (at, total)
    return coef


@functools.lru_cache(maxsize=None)
def cases():
    out = collections.OrderedDict()

    def add(name, coef, geometry, script, restart=0):
        quant = [FLAT_QUANT] * geometry[2]
        coef = np.ascontiguousarray(coef, np.int16)
        coef.setflags(write=False)
        out[name] = Case(pw.write(coef, quant, geometry, script, restart), coef, geometry, tuple(script), restart)

    g = (24, 24, 3, 2, 2)
    add("spectral_only_420_24x24", random_coef(g, 1), g, _script(3, [(0, 0)], [(1, 5, 0, 0), (6, 20, 0, 0), (21, 63, 0, 0)]))
    g = (9, 17, 3, 2, 1)
    add("three_bits_deep_422_17x9", random_coef(g, 2), g,
        _script(3, [(0, 2), (2, 1), (1, 0)], [(1, 63, 0, 2), (1, 63, 2, 1), (1, 63, 1, 0)]))
    g = (24, 8, 3, 2, 2)
    add("dc_per_component_420_8x24", random_coef(g, 3, pad_dc=False), g,
        [((c,), 0, 0, 0, 1) for c in range(3)] + [((c,), 0, 0, 1, 0) for c in (2, 0, 1)] +
        [((c,), 1, 63, 0, 0) for c in range(3)])
    g = (9, 9, 3, 1, 1)
    add("one_band_per_coefficient_444_9x9", random_coef(g, 4, density=0.5), g,
        _script(3, [(0, 0)], [(k, k, 0, 0) for k in range(1, 64)]))
    g = (37, 53, 1, 1, 1)
    add("pillow_script_grey_53x37_restart4", random_coef(g, 5), g, pw.PILLOW_SCRIPT_1, restart=4)
    # refinement without one new coefficient: every block of the refinement scans lies inside one end-of-band run
    g = (16, 24, 3, 1, 1)
    coef = random_coef(g, 6, density=0.2)
    coef[np.abs(coef) == 1] = 2
    add("refinement_inside_one_eob_run_444_24x16", coef, g, _script(3, [(0, 0)], [(1, 63, 0, 1), (1, 63, 1, 0)]))
    # one block: history at 3 and 7, a new -1 at 18 after 15 coefficients that are still zero; ZRL in both procedures
    g = (8, 16, 1, 1, 1)
    coef = np.zeros((2, 1, 64), np.int16)
    zz = pw.ZIGZAG
    coef[0, 0, zz[3]], coef[0, 0, zz[7]], coef[0, 0, zz[18]], coef[0, 0, zz[40]] = 6, -5, -1, 7
    coef[1, 0, zz[45]], coef[1, 0, zz[60]], coef[1, 0, zz[2]] = 9, 1, -3
    coef[:, 0, 0] = (100, -50)
    add("runs_and_zrl_grey_16x8", coef, g, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)])
    # end-of-band runs of every category: 129 x 128 blocks
    g = (1024, 1032, 1, 1, 1)
    total = 129 * 128
    coef = np.zeros((total, 1, 64), np.int16)
    coef[-1, 0, 1] = 5
    coef[::97, 0, 0] = 33
    add("eob_run_category_14_grey_1032x1024", coef, g, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)])
    coef = _eob_runs([1 << c for c in range(14)] + [70], total)
    add("eob_run_categories_0_to_13_grey_1032x1024", coef, g, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 0)])
    # a restart interval of 2 blocks cuts the runs of a sparse picture
    g = (24, 24, 3, 2, 2)
    add("restart_cuts_eob_runs_420_24x24", random_coef(g, 7, density=0.01), g,
        _script(3, [(0, 1), (1, 0)], [(1, 63, 0, 1), (1, 63, 1, 0)]), restart=2)
    return out


def small():
    """the cases without the two 1032 x 1024 pictures"""
    return collections.OrderedDict((k, v) for k, v in cases().items() if "1032" not in k)
