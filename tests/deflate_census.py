"""What a payload makes the device DEFLATE encoder do: the restatement's own plan of every block (tests/deflate_ref.py,
`plan_block`: the parse, the three codes, the header counts, the exact bit count and every token's bits) and counters over
the plans.  tests/test_deflate_cpu.py asserts the counters over the payloads of tests/deflate_cases.py, so that a path of
`deflate_block_kernel` cannot silently stop being tested.  CPU only; nothing here states a rule of the encoder."""
import deflate_ref as ref

LIMITS = (15, 15, 7)               # literal/length, distance, code-length


class Block(object):
    """One block of a payload.  n; final; dynamic (the form chosen); margin: dyn_bytes - (n + 5), stored exactly when >= 0;
    pad: the zero bits behind a NON-FINAL DYNAMIC block (None otherwise: no marker rule applies); hlit, hdist, hclen (counts
    sent); longest: the longest code of (literal/length, distance, code-length); depth: the unlimited two-queue depth of
    the three; limited: depth > limit, per alphabet; lengths, length_codes (0..28), dists, dist_codes: the sets emitted;
    dist_max; used_dist_codes: the distance codes with a non-zero length; widths: every token's bits, the end-of-block
    symbol last; shifts: every token's bit offset in the block mod 32; third_word: the indices of the tokens whose put reaches
    a third 32-bit word ((offset & 31) + bits > 64); clipped: [(p, length, distance)] of the match that ends the block
    below 258 bytes, which min(258, n - p) cut whatever the source holds behind it; plan"""


def block(data, final):
    pl = ref.plan_block(data)
    b = Block()
    b.plan, b.n, b.final, b.dynamic = pl, pl.n, final, pl.dynamic
    b.margin = pl.dyn_bytes - (pl.n + 5)
    b.pad = pl.pad if pl.dynamic and not final else None
    b.hlit, b.hdist, b.hclen = pl.hlit, pl.hdist, pl.hclen
    b.longest = (max(pl.len_ll), max(pl.len_d), max(pl.len_cl))
    b.depth = (ref.unlimited_depth(pl.hist_ll), ref.unlimited_depth(pl.hist_d), ref.unlimited_depth(pl.hist_cl))
    b.limited = tuple(d > lim for d, lim in zip(b.depth, LIMITS))
    copies = [(p, l, d) for p, l, d in pl.toks if l]
    b.lengths = set(l for _, l, _ in copies)
    b.length_codes = set(ref.length_code(l)[0] for l in b.lengths)
    b.dists = set(d for _, _, d in copies)
    b.dist_codes = set(ref.dist_code(d)[0] for d in b.dists)
    b.dist_max = max(b.dists) if b.dists else 0
    b.used_dist_codes = [c for c in range(30) if pl.len_d[c]]
    b.widths = list(pl.widths)
    at, b.shifts = pl.token_at, []
    for w in b.widths:
        b.shifts.append(at & 31)
        at += w
    b.third_word = [i for i, (s, w) in enumerate(zip(b.shifts, b.widths)) if s + w > 64]
    # a match that stops at the block's end below 258 was cut by min(258, n - p), whatever the source holds behind it
    b.clipped = [(p, l, d) for p, l, d in copies if p + l == pl.n and l < ref.MAX_MATCH]
    return b


def census_blocks(payload):
    """[Block] of a payload's blocks, in order"""
    payload = bytes(payload)
    n = len(payload)
    return [block(payload[s:s + ref.BLOCK], s + ref.BLOCK >= n) for s in range(0, n, ref.BLOCK)]


def table(blocks):
    """the counters over [Block]: the rows of DESIGN section 8's table"""
    dyn = [b for b in blocks if b.dynamic]
    widths = [w for b in dyn for w in b.widths]
    c = dict(blocks=len(blocks), dynamic=len(dyn), stored=len(blocks) - len(dyn))
    c["widest"] = max(widths + [0])
    c["over_32"] = sum(1 for w in widths if w > 32)
    c["third_word"] = sum(len(b.third_word) for b in dyn)
    c["third_word_shift"] = max([b.shifts[i] for b in dyn for i in b.third_word] + [-1])
    c["length_codes"] = sorted(set().union(*[b.length_codes for b in dyn]))
    c["lengths"] = sorted(set().union(*[b.lengths for b in dyn]))
    c["dist_codes"] = sorted(set().union(*[b.dist_codes for b in dyn]))
    c["dists"] = set().union(*[b.dists for b in dyn])
    c["dist_max"] = max([b.dist_max for b in dyn] + [0])
    c["longest"] = tuple(max([b.longest[a] for b in dyn] + [0]) for a in range(3))
    c["limited"] = tuple(sum(1 for b in dyn if b.limited[a]) for a in range(3))
    c["hclen"] = sorted(set(b.hclen for b in dyn))
    c["pads"] = sorted(set(b.pad for b in dyn if b.pad is not None))
    c["off_the_edge"] = min(min(abs(b.margin), abs(b.margin + 1)) for b in blocks)     # the edge: margins -1 and 0
    c["clipped"] = sum(len(b.clipped) for b in dyn)
    c["one_dist_code"] = sorted(b.used_dist_codes[0] for b in dyn if len(b.used_dist_codes) == 1 and b.dists)
    return c
