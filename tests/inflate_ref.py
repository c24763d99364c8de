"""Plain-Python restatement of the device inflater (csrc/inflate.hip, `acimg_inflate`): the finder's rule, the count pass
with its stop rule, the chain, the offsets, the 16-bit window markers and both resolve steps.  Slow (about 0.2 MB/s): the
tests keep every payload at or below 256 KiB.  `inflate(stream, out_len, chunk_bytes)` returns a `Result` whose fields
the GPU test compares with the debug view of the workspace."""
OK, CORRUPT, SIZE, TRUNCATED = 0, 1, 2, 3
MARK = 0x8000
WINDOW = 32768
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
REV15 = [int(format(v, "015b")[::-1], 2) for v in range(1 << 15)]


class Fail(Exception):
    def __init__(self, status):
        Exception.__init__(self, status)
        self.status = status


def length_base(c):
    """length code c = symbol - 257 in 0..28 -> (base length, extra bits)"""
    if c < 8:
        return 3 + c, 0
    if c == 28:
        return 258, 0
    k = (c - 4) >> 2
    return 3 + ((4 + (c & 3)) << k), k


def dist_base(c):
    """distance code 0..29 -> (base distance, extra bits)"""
    if c < 4:
        return 1 + c, 0
    k = (c - 2) >> 1
    return 1 + ((2 + (c & 1)) << k), k


class Reader(object):
    """bits of `data`, least significant first; bits past the end read as 0 but may not be consumed"""

    def __init__(self, data, pos=0):
        self.data, self.n8, self.pos = data, 8 * len(data), pos

    def peek(self, k):
        b = self.pos >> 3
        return (int.from_bytes(self.data[b:b + 5], "little") >> (self.pos & 7)) & ((1 << k) - 1)

    def take(self, k):
        if self.pos + k > self.n8:
            raise Fail(TRUNCATED)
        v = self.peek(k)
        self.pos += k
        return v


class Code(object):
    """canonical code of `lens`: a symbol of length L is the shortest L whose left-aligned limit exceeds the next 15 bits"""

    def __init__(self, lens):
        count = [0] * 16
        for l in lens:
            count[l] += 1
        count[0] = 0
        self.kraft = sum(count[L] << (15 - L) for L in range(1, 16))
        self.used = sum(count)
        self.single = self.used == 1 and count[1] == 1
        self.first, self.index, self.limit = [0] * 16, [0] * 16, [0] * 16
        code = at = 0
        for L in range(1, 16):
            code = (code + count[L - 1]) << 1
            self.first[L], self.index[L] = code, at
            self.limit[L] = (code + count[L]) << (15 - L)
            at += count[L]
        self.sorted = sorted((s for s, l in enumerate(lens) if l), key=lambda s: (lens[s], s))

    def check(self):
        """zlib's rule: over-subscribed is an error; incomplete only with no code at all or a single code of length 1"""
        if self.kraft > WINDOW or (self.kraft < WINDOW and self.used and not self.single):
            raise Fail(CORRUPT)

    def decode(self, r):
        c = REV15[r.peek(15)]
        for L in range(1, 16):
            if c < self.limit[L]:
                if r.pos + L > r.n8:
                    raise Fail(TRUNCATED)
                r.pos += L
                return self.sorted[self.index[L] + (c >> (15 - L)) - self.first[L]]
        raise Fail(TRUNCATED if r.pos + 15 > r.n8 else CORRUPT)


def read_dynamic_lengths(r):
    """HLIT, HDIST, HCLEN, the code-length code and the lengths -> (literal/length lengths, distance lengths, the code-length
    Code); every violation raises Fail"""
    hlit, hdist, hclen = r.take(5), r.take(5), r.take(4)
    if hlit > 29 or hdist > 29:
        raise Fail(CORRUPT)
    cl = [0] * 19
    for i in range(hclen + 4):
        cl[CL_ORDER[i]] = r.take(3)
    clc = Code(cl)
    clc.check()
    total, lens = hlit + 257 + hdist + 1, []
    while len(lens) < total:
        s = clc.decode(r)
        if s < 16:
            lens.append(s)
            continue
        if s == 16:
            if not lens:
                raise Fail(CORRUPT)
            rep, val = 3 + r.take(2), lens[-1]
        elif s == 17:
            rep, val = 3 + r.take(3), 0
        else:
            rep, val = 11 + r.take(7), 0
        if len(lens) + rep > total:
            raise Fail(CORRUPT)
        lens.extend([val] * rep)
    if lens[256] == 0:
        raise Fail(CORRUPT)
    return lens[:hlit + 257], lens[hlit + 257:], clc


def is_start(data, o):
    """the finder's rule at bit offset o"""
    r = Reader(data, o)
    try:
        if r.take(1) != 0 or r.take(2) != 2:
            return False
        ll, d, clc = read_dynamic_lengths(r)
    except Fail:
        return False
    if clc.kraft != WINDOW or Code(ll).kraft != WINDOW:
        return False
    dc = Code(d)
    return dc.kraft == WINDOW or dc.used <= 1


def find_starts(data, chunk_bytes):
    """start bit of every chunk (chunk 0: 0), -1 where no offset of the chunk passes"""
    n = len(data)
    nchunks = max(1, -(-n // chunk_bytes))
    starts = [0] + [-1] * (nchunks - 1)
    for j in range(1, nchunks):
        for o in range(8 * j * chunk_bytes, min(8 * (j + 1) * chunk_bytes, 8 * n)):
            b = o >> 3
            if ((data[b] | (data[b + 1] << 8 if b + 1 < n else 0)) >> (o & 7)) & 7 != 4:      # BFINAL 0, BTYPE 2
                continue
            if is_start(data, o):
                starts[j] = o
                break
    return starts


def run_chunk(data, j, starts, chunk_bytes, out_len, base=None, boundaries=None):
    """chunk j from its start to its link or past the BFINAL block -> (status, produced, end bit, next chunk or -1, symbols).
    base None: the count pass (no symbols); else the chunk's output offset (the decode pass).  boundaries: a list that
    receives (bit, BFINAL, BTYPE) of every block header read."""
    r = Reader(data, starts[j])
    syms = [] if base is not None else None
    produced, begun = 0, False

    def emit(count):
        if produced + count > out_len:
            raise Fail(SIZE)

    try:
        while True:
            if begun:
                k = r.pos // (8 * chunk_bytes)
                if j < k < len(starts) and starts[k] == r.pos:
                    return OK, produced, r.pos, k, syms
            begun = True
            at = r.pos
            final, btype = r.take(1), r.take(2)
            if boundaries is not None:
                boundaries.append((at, final, btype))
            if btype == 3:
                raise Fail(CORRUPT)
            if btype == 0:
                r.pos = (r.pos + 7) & ~7
                ln, nln = r.take(16), r.take(16)
                if ln != (~nln & 0xFFFF):
                    raise Fail(CORRUPT)
                if r.pos + 8 * ln > r.n8:
                    raise Fail(TRUNCATED)
                emit(ln)
                if syms is not None:
                    syms.extend(data[r.pos >> 3:(r.pos >> 3) + ln])
                produced += ln
                r.pos += 8 * ln
            else:
                if btype == 1:
                    ll, d = FIXED_LL, FIXED_D
                else:
                    ll, d, _ = read_dynamic_lengths(r)
                llc, dc = Code(ll), Code(d)
                llc.check()
                dc.check()
                while True:
                    s = llc.decode(r)
                    if s < 256:
                        emit(1)
                        if syms is not None:
                            syms.append(s)
                        produced += 1
                        continue
                    if s == 256:
                        break
                    if s >= 286:
                        raise Fail(CORRUPT)
                    ln, k = length_base(s - 257)
                    ln += r.take(k)
                    ds = dc.decode(r)
                    if ds >= 30:
                        raise Fail(CORRUPT)
                    dist, k = dist_base(ds)
                    dist += r.take(k)
                    if j == 0 and dist > produced:
                        raise Fail(CORRUPT)
                    if base is not None and dist > produced + base:
                        raise Fail(CORRUPT)
                    emit(ln)
                    if syms is not None:
                        for _ in range(ln):
                            src = len(syms) - dist
                            syms.append(syms[src] if src >= 0 else MARK + WINDOW + src)      # the byte -src before the chunk
                    produced += ln
            if final:
                return OK, produced, r.pos, -1, syms
    except Fail as f:
        return f.status, produced, r.pos, -1, syms


class Result(object):
    pass


def block_headers(data, out_len):
    """[(bit, BFINAL, BTYPE)] of every block of a valid stream, by one serial decode"""
    found = []
    st = run_chunk(bytes(data), 0, [0], 8 * len(data) + 8, out_len, boundaries=found)[0]
    assert st == OK, st
    return found


def inflate(data, out_len, chunk_bytes):
    """the whole plan on one stream"""
    data = bytes(data)
    res = Result()
    res.starts = find_starts(data, chunk_bytes)
    nchunks = len(res.starts)
    counted = {j: run_chunk(data, j, res.starts, chunk_bytes, out_len) for j in range(nchunks) if res.starts[j] >= 0}
    # chain
    res.live, res.lengths, res.offsets = [0] * nchunks, [0] * nchunks, [0] * nchunks
    res.status, res.end_bits, j, total = OK, 0, 0, 0
    while j >= 0:
        st, produced, end, nxt, _ = counted[j]
        res.live[j], res.lengths[j], res.offsets[j] = 1, produced, total
        total += produced
        if st != OK:
            res.status = st
            break
        if nxt < 0:
            res.end_bits = end
        j = nxt
    if res.status == OK and total != out_len:
        res.status = SIZE
    # decode
    sym = [0] * out_len
    for j in range(nchunks):
        if res.live[j]:
            st, produced, _, _, syms = run_chunk(data, j, res.starts, chunk_bytes, out_len, base=res.offsets[j])
            if st != OK and res.status == OK:
                res.status = st
            syms = syms[:max(0, out_len - res.offsets[j])]
            sym[res.offsets[j]:res.offsets[j] + len(syms)] = syms
    # resolve the tails in chain order, then everything
    res.marker_reach = 0          # the most live chunks between a marker's chunk and the chunk that holds its source
    live_offsets = [res.offsets[j] for j in range(nchunks) if res.live[j]]
    for j in range(1, nchunks):
        if not res.live[j]:
            continue
        off, ln = res.offsets[j], min(res.lengths[j], out_len - res.offsets[j])
        for i in range(max(0, ln - WINDOW), ln):
            m = sym[off + i]
            if m >= MARK:
                src = off - WINDOW + (m - MARK)
                if src >= 0:
                    res.marker_reach = max(res.marker_reach, sum(1 for o in live_offsets if src < o <= off))
                if src < 0:
                    res.status = res.status or CORRUPT
                else:
                    sym[off + i] = sym[src]
    out = bytearray(out_len)
    for j in range(nchunks):
        if not res.live[j]:
            continue
        off, ln = res.offsets[j], min(res.lengths[j], out_len - res.offsets[j])
        for i in range(ln):
            m = sym[off + i]
            if m >= MARK:
                src = off - WINDOW + (m - MARK)
                m = sym[src] if src >= 0 else 0
            out[off + i] = m & 0xFF
    res.out = bytes(out)
    if res.status != OK:
        res.end_bits = 0
    return res
