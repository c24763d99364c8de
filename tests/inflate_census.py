"""What a deflate stream reaches of RFC 1951: one serial walk with the restatement's own reader and codes
(tests/inflate_ref.py) that records every block and every token, and counters over them.  `place_in_chunks` adds, from a
`Result` of `inflate_ref.inflate`, the live chunk that decodes each block and how many bytes that chunk had produced before
each copy.  tests/test_inflate_cpu.py asserts the counters over the streams of tests/inflate_cases.py, so that a feature the
device decoder has a path for cannot silently stop being tested."""
import inflate_ref as ref


class Block(object):
    """bit: of the header; btype; final; out: bytes produced before it; for a dynamic block hlit, hdist, hclen, cl (the 19
    code-length lengths) and crossing: [(symbol, value)] of the repeat runs that begin in the literal/length lengths and end
    in the distance lengths; for a stored block ln and end (the bit behind its data); tokens: [Token]"""


class Token(object):
    """literal: the byte or None; out: bytes produced before it; ll_bits, and for a copy length, dist, symbol (the length's)
    and d_bits: the bits of the codes that were decoded"""


def _crossing_runs(r, clc, nll, total):
    """walk the code-length symbols again from the reader's position -> [(symbol, repeated value)] of the runs over nll"""
    have, prev, out = 0, 0, []
    while have < total:
        s = clc.decode(r)
        rep, val = 1, s
        if s == 16:
            rep, val = 3 + r.take(2), prev
        elif s == 17:
            rep, val = 3 + r.take(3), 0
        elif s == 18:
            rep, val = 11 + r.take(7), 0
        if s >= 16 and have < nll < have + rep:
            out.append((s, val))
        prev = val
        have += rep
    return out


def walk(stream):
    """the blocks of a valid stream, serially"""
    r = ref.Reader(bytes(stream))
    blocks, produced = [], 0
    while True:
        b = Block()
        b.bit, b.out, b.tokens = r.pos, produced, []
        b.final, b.btype = r.take(1), r.take(2)
        blocks.append(b)
        if b.btype == 0:
            r.pos = (r.pos + 7) & ~7
            b.ln = r.take(16)
            assert r.take(16) == b.ln ^ 0xFFFF
            r.pos += 8 * b.ln
            assert r.pos <= r.n8
            b.end = r.pos
            produced += b.ln
        else:
            assert b.btype in (1, 2)
            ll, d = ref.FIXED_LL, ref.FIXED_D
            if b.btype == 2:
                at = r.pos
                ll, d, clc = ref.read_dynamic_lengths(r)
                after = r.pos
                b.hlit, b.hdist = len(ll) - 257, len(d) - 1
                r.pos = at + 10
                b.hclen = r.take(4)
                b.cl = [0] * 19
                for i in range(b.hclen + 4):
                    b.cl[ref.CL_ORDER[i]] = r.take(3)
                b.crossing = _crossing_runs(r, clc, len(ll), len(ll) + len(d))
                assert r.pos == after
            llc, dc = ref.Code(ll), ref.Code(d)
            while True:
                t = Token()
                at = r.pos
                s = llc.decode(r)
                t.ll_bits, t.out, t.literal = r.pos - at, produced, s if s < 256 else None
                if s == 256:
                    b.eob_bits = t.ll_bits
                    break
                b.tokens.append(t)
                if s < 256:
                    produced += 1
                    continue
                base, k = ref.length_base(s - 257)
                t.symbol, t.length = s, base + r.take(k)
                at = r.pos
                base, k = ref.dist_base(dc.decode(r))
                t.d_bits = r.pos - at
                t.dist = base + r.take(k)
                assert t.dist <= produced
                produced += t.length
        if b.final:
            b.end = r.pos
            return blocks


def runs_of_literals(blocks):
    """[(literals, what ends the run)]: a run is the literals between two copies, stored blocks or ends of the stream - the
    end-of-block symbol of a Huffman block does not end it, the decoder keeps them waiting.  What ends it: "copy", "eob" (the
    end-of-block symbol right behind the last literal, the next block a Huffman block), "stored" (the same, the next block a
    stored one) or "end" (the stream's)"""
    out, n, after_eob = [], 0, False
    for b in blocks:
        if b.btype == 0:
            if n:
                out.append((n, "stored" if after_eob else "copy"))
            n = 0
            continue
        for t in b.tokens:
            if t.literal is not None:
                n, after_eob = n + 1, False
            else:
                if n:
                    out.append((n, "eob" if after_eob else "copy"))
                n = 0
        after_eob = n > 0
    if n:
        out.append((n, "end"))
    return out


def place_in_chunks(blocks, result):
    """sets block.chunk (the live chunk of `result` that decodes the block), block.starts_chunk (the block's header is that
    chunk's start) and, on every copy, token.produced: the bytes its chunk had produced before it"""
    live = [j for j, l in enumerate(result.live) if l]
    for b in blocks:
        b.chunk = max(j for j in live if result.starts[j] <= b.bit)
        b.starts_chunk = result.starts[b.chunk] == b.bit
        for t in b.tokens:
            t.produced = t.out - result.offsets[b.chunk]
    return blocks


def census(stream):
    """the counters of one stream, and its blocks"""
    blocks = walk(stream)
    copies = [t for b in blocks for t in b.tokens if t.literal is None]
    dyn = [b for b in blocks if b.btype == 2]
    c = dict(blocks=blocks)
    c["ll_bits"] = max([t.ll_bits for b in blocks for t in b.tokens] + [b.eob_bits for b in blocks if b.btype] + [0])
    c["d_bits"] = max([t.d_bits for t in copies] + [0])
    c["hclen"] = max([b.hclen for b in dyn] + [0])
    c["cl_symbol_15"] = sum(1 for b in dyn if b.hclen == 15 and b.cl[15])
    c["cl_bits"] = max([max(b.cl) for b in dyn] + [0])
    c["len258_as_284"] = sum(1 for t in copies if t.length == 258 and t.symbol == 284)
    c["len258_as_285"] = sum(1 for t in copies if t.symbol == 285)
    c["dist_max"] = max([t.dist for t in copies] + [0])
    c["dist_32768"] = sum(1 for t in copies if t.dist == 32768)
    c["stored_len_max"] = max([b.ln for b in blocks if b.btype == 0] + [-1])
    c["crossing"] = sorted(set(x for b in dyn for x in b.crossing))
    c["hlit29_hdist29"] = sum(1 for b in dyn if b.hlit == 29 and b.hdist == 29)
    return c
