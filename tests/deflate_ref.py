"""Restatement of csrc/deflate.hip in Python / NumPy: the same parse rule, the same code construction and the same header
choices, so that `deflate(payload)` equals the device's stream byte for byte (tests/test_deflate_gpu.py) and the format
can be checked against zlib on a machine without a GPU (tests/test_deflate_cpu.py).  DESIGN section 8 has the prose.

Stream: the payload is cut into blocks of BLOCK bytes; each block is coded on its own (no match reaches before its first
byte) as ONE stored or dynamic-Huffman DEFLATE block, whichever has fewer bytes (dynamic only when strictly smaller);
every block but the last is followed by an empty stored block (the sync-flush form), so that the next block starts on a
byte boundary; the last carries BFINAL.  The empty block's three header bits 000 lie in the zero bits that pad the block
to a byte when at least three are left (then 00 00 FF FF follows, 4 bytes), else in a byte of their own (00 00 00 FF FF).
A payload of 0 bytes is the final empty stored block 01 00 00 FF FF.

Parse of one block of n bytes (positions p, bytes b):
  hash(p) = ((b[p] | b[p+1] << 8 | b[p+2] << 16) * 0x9E3779B1 mod 2^32) >> (32 - HASH_BITS), for p + 2 < n
  candidate A of p: the LARGEST q with hash(q) == hash(p) among the positions before the start of p's sub-step
      (q < CHUNK * (p // CHUNK)); none if there is no such q or p + 2 >= n
  candidate B of p: p - 1 (p >= 1)
  length of a candidate q: the number of leading bytes b[q + i] == b[p + i], i < min(258, n - p)
  the match of p: B if its length >= A's, else A; no match if that length is below 3
  greedy walk: p = 0; a position with a match of length l emits (l, p - q) and moves to p + l, one without emits the
      literal b[p] and moves to p + 1; then the end-of-block symbol.
Codes: `huffman_lengths` for the literal/length (286, limit 15), distance (30, limit 15) and code-length (19, limit 7)
alphabets; a block without a match sends the one distance code length 1 for symbol 0.  The header sends HLIT / HDIST with
trailing zero lengths dropped and every code length as its own symbol 0..15: the run symbols 16, 17, 18 are not used."""
import heapq

import numpy as np

BLOCK = 16384
CHUNK = 256
HASH_BITS = 13
MIN_MATCH, MAX_MATCH = 3, 258
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
EMPTY_FINAL = b"\x01\x00\x00\xff\xff"
SYNC = b"\x00\x00\x00\xff\xff"


def bound(n):
    """acimg_deflate_bound"""
    return n + 10 * (-(-n // BLOCK)) + 5


def length_code(l):
    """match length 3..258 -> (code 0..28 above symbol 257, extra bits, extra value)"""
    if l == 258:
        return 28, 0, 0
    v = l - 3
    if v < 8:
        return v, 0, 0
    k = v.bit_length() - 3
    return 4 * k + 4 + ((v >> k) & 3), k, v & ((1 << k) - 1)


def dist_code(d):
    """distance 1..32768 -> (code 0..29, extra bits, extra value)"""
    v = d - 1
    if v < 4:
        return v, 0, 0
    k = v.bit_length() - 2
    return 2 * k + 2 + ((v >> k) & 1), k, v & ((1 << k) - 1)


LEN_EXTRA = [length_code(b)[1] for b in (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115,
                                         131, 163, 195, 227, 258)]
DIST_EXTRA = [dist_code(b)[1] for b in (1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537,
                                        2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577)]


def leaf_depths(freq):
    """(order, depth) of the two-queue Huffman merge, before any limit: the used symbols ordered by (freq, symbol) and the
    depth of each one's leaf (of two equal weights the LEAF is taken first); two or more used symbols"""
    order = sorted((i for i in range(len(freq)) if freq[i] > 0), key=lambda i: (freq[i], i))
    used = len(order)
    assert used >= 2
    w = [freq[i] for i in order] + [0] * (used - 1)
    parent = [0] * (2 * used - 1)
    i, j = 0, used
    for nxt in range(used, 2 * used - 1):
        pick = []
        for _ in range(2):
            if i < used and (j >= nxt or w[i] <= w[j]):
                pick.append(i)
                i += 1
            else:
                pick.append(j)
                j += 1
        w[nxt] = w[pick[0]] + w[pick[1]]
        parent[pick[0]] = parent[pick[1]] = nxt
    depth = [0] * (2 * used - 1)
    for k in range(2 * used - 3, -1, -1):
        depth[k] = depth[parent[k]] + 1
    return order, depth[:used]


def unlimited_depth(freq):
    """the deepest leaf of `leaf_depths` (the number of used symbols when there are fewer than two): above the alphabet's
    limit exactly when the limiter of `huffman_lengths` acts"""
    freq = [int(f) for f in freq]
    used = sum(1 for f in freq if f > 0)
    return max(leaf_depths(freq)[1]) if used >= 2 else used


def huffman_lengths(freq, limit):
    """Code lengths of one alphabet (the device's `huffman_lengths`): symbols with freq <= 0 get 0; one used symbol gets 1.
    Otherwise the used symbols are ordered by (freq, symbol); a two-queue Huffman merge (of two equal weights the LEAF
    is taken first) gives the leaf depths; depths above `limit` are set to `limit`, and while the Kraft sum exceeds 1 by
    E units of 2^-limit, E times: the deepest level b < limit that holds a leaf gives one up to level b + 1, together with
    one leaf taken from level `limit` (count[b] -= 1, count[b + 1] += 2, count[limit] -= 1: the sum falls by one unit).
    Last, the levels' counts are dealt out in the order of the sort, the longest lengths to the least frequent symbols."""
    freq = [int(f) for f in freq]
    out = [0] * len(freq)
    used = sum(1 for f in freq if f > 0)
    if used == 0:
        return out
    if used == 1:
        out[next(i for i, f in enumerate(freq) if f > 0)] = 1
        return out
    order, depth = leaf_depths(freq)
    count = [0] * (limit + 1)
    for k in range(used):
        count[min(depth[k], limit)] += 1
    excess = sum(count[b] << (limit - b) for b in range(1, limit + 1)) - (1 << limit)
    while excess > 0:
        b = limit - 1
        while b > 0 and count[b] == 0:
            b -= 1
        if b == 0 or count[limit] == 0:
            break
        count[b] -= 1
        count[b + 1] += 2
        count[limit] -= 1
        excess -= 1
    k = 0
    for b in range(limit, 0, -1):
        for _ in range(count[b]):
            out[order[k]] = b
            k += 1
    return out


def heap_huffman_cost(freq):
    """(cost, depth) of a textbook heapq Huffman build: sum of freq * length, and the longest length"""
    heap = [(f, 0, i) for i, f in enumerate(freq) if f > 0]
    if len(heap) < 2:
        return sum(f for f, _, _ in heap), len(heap)
    heapq.heapify(heap)
    cost, tick = 0, len(freq)
    while len(heap) > 1:
        a = heapq.heappop(heap)
        b = heapq.heappop(heap)
        cost += a[0] + b[0]
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1, tick))
        tick += 1
    return cost, heap[0][1]


def canonical_codes(lengths):
    """RFC 1951 3.2.2 codes, bit-reversed (DEFLATE sends Huffman codes most significant bit first)"""
    count = [0] * 16
    for l in lengths:
        count[l] += 1
    count[0] = 0
    nxt, code = [0] * 16, 0
    for b in range(1, 16):
        code = (code + count[b - 1]) << 1
        nxt[b] = code
    out = []
    for l in lengths:
        if l == 0:
            out.append(0)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append(int(format(c, "0%db" % l)[::-1], 2))
    return out


def hashes(b):
    """int64 [n - 2]: hash(p) of every position of the uint8 array `b` that has three bytes (n >= 3)"""
    b = b.astype(np.uint32)
    w = b[:-2] | (b[1:-1] << 8) | (b[2:] << 16)
    return ((w * np.uint32(0x9E3779B1)) >> np.uint32(32 - HASH_BITS)).astype(np.int64)


def find_matches(b):
    """(length uint16 [n], distance uint16 [n]) of every position of one block (length 0: no match)"""
    n = len(b)
    pad = np.zeros(n + MAX_MATCH + 2, np.uint8)
    pad[:n] = b
    cand = np.zeros(n, np.int64)                       # q + 1, 0 = none
    if n >= 3:
        h = hashes(pad[:n])
        head = np.zeros(1 << HASH_BITS, np.int64)
        for s in range(0, n - 2, CHUNK):
            e = min(s + CHUNK, n - 2)
            cand[s:e] = head[h[s:e]]
            np.maximum.at(head, h[s:e], np.arange(s + 1, e + 1))
    pos = np.arange(n)
    maxl = np.minimum(MAX_MATCH, n - pos)

    def lengths(q, have):
        l = np.zeros(n, np.int64)
        idx = np.nonzero(have)[0]
        for i in range(MAX_MATCH):
            idx = idx[(i < maxl[idx]) & (pad[q[idx] + i] == pad[idx + i])]
            if idx.size == 0:
                break
            l[idx] += 1
        return l

    la = lengths(np.maximum(cand - 1, 0), cand > 0)
    lb = lengths(np.maximum(pos - 1, 0), pos >= 1)
    take_b = lb >= la
    length = np.where(take_b, lb, la)
    dist = np.where(take_b, 1, pos - (cand - 1))
    none = length < MIN_MATCH
    length[none] = 0
    dist[none] = 0
    return length.astype(np.uint16), dist.astype(np.uint16)


def greedy_parse(b):
    """the greedy walk: [(position, length, distance)], length 0 for a literal"""
    length, dist = find_matches(b)
    length, dist = length.tolist(), dist.tolist()
    toks, p, n = [], 0, len(b)
    while p < n:
        toks.append((p, length[p], dist[p]))
        p += length[p] if length[p] else 1
    return toks


def _put(out, off, val, nbits):
    """OR the low `nbits` of every val (< 2^48) into the byte array `out` at bit offsets `off` (least significant first)"""
    val = np.asarray(val, np.uint64) << (np.asarray(off, np.uint64) & np.uint64(7))
    byte = np.asarray(off, np.int64) >> 3
    for k in range(8):
        part = ((val >> np.uint64(8 * k)) & np.uint64(0xFF)).astype(np.uint8)
        keep = part != 0
        np.bitwise_or.at(out, byte[keep] + k, part[keep])


class Plan(object):
    """What is decided about one block before a bit is written, the one statement of the rules that `code_block` writes out
    and tests/deflate_census.py counts.  data (uint8 [n]), n; toks (the greedy parse); hist_ll, hist_d, hist_cl; len_ll,
    len_d, len_cl and code_ll, code_d, code_cl; hlit, hdist, hclen (the counts sent, not the header fields); seq (the code
    lengths the header sends, in order); bits (the dynamic form's exact bit count), dyn_bytes, dynamic (the form chosen), pad
    (the zero bits that fill the dynamic form's last byte); token_at (the bit offset in the block of the first token);
    vals, widths (every token's bits and their count, the end-of-block symbol last)"""


def plan_block(b):
    """the Plan of one block of 1..BLOCK bytes"""
    pl = Plan()
    pl.data = b = np.frombuffer(bytes(b), np.uint8)
    pl.n = n = len(b)
    assert 1 <= n <= BLOCK
    pl.toks = toks = greedy_parse(b)
    pl.hist_ll, pl.hist_d = hist_ll, hist_d = [0] * 286, [0] * 30
    hist_ll[256] = 1
    for p, l, d in toks:
        if l:
            hist_ll[257 + length_code(l)[0]] += 1
            hist_d[dist_code(d)[0]] += 1
        else:
            hist_ll[int(b[p])] += 1
    pl.len_ll = len_ll = huffman_lengths(hist_ll, 15)
    pl.len_d = len_d = huffman_lengths(hist_d, 15)
    if not any(len_d):
        len_d[0] = 1
    pl.hlit = hlit = max(257, max(i for i in range(286) if len_ll[i]) + 1)
    pl.hdist = hdist = max(1, max(i for i in range(30) if len_d[i]) + 1)
    pl.seq = seq = len_ll[:hlit] + len_d[:hdist]
    pl.hist_cl = hist_cl = [0] * 19
    for s in seq:
        hist_cl[s] += 1
    pl.len_cl = len_cl = huffman_lengths(hist_cl, 7)
    pl.hclen = hclen = max(4, max(i for i in range(19) if len_cl[CL_ORDER[i]]) + 1)
    pl.token_at = 17 + 3 * hclen + sum(hist_cl[s] * len_cl[s] for s in range(19))
    bits = pl.token_at + sum(hist_ll[s] * len_ll[s] for s in range(257))
    bits += sum(hist_ll[257 + c] * (len_ll[257 + c] + LEN_EXTRA[c]) for c in range(29))
    bits += sum(hist_d[c] * (len_d[c] + DIST_EXTRA[c]) for c in range(30))
    pl.bits = bits
    pl.dyn_bytes = (bits + 7) >> 3
    pl.pad = pl.dyn_bytes * 8 - bits
    pl.dynamic = pl.dyn_bytes < n + 5
    pl.code_ll, pl.code_d, pl.code_cl = code_ll, code_d, _ = canonical_codes(len_ll), canonical_codes(len_d), canonical_codes(len_cl)
    pl.vals, pl.widths = vals, nb = [], []
    for p, l, d in toks:
        if l == 0:
            s = int(b[p])
            vals.append(code_ll[s])
            nb.append(len_ll[s])
        else:
            lc, lk, lx = length_code(l)
            dc, dk, dx = dist_code(d)
            v, k = code_ll[257 + lc], len_ll[257 + lc]
            v |= lx << k
            k += lk
            v |= code_d[dc] << k
            k += len_d[dc]
            v |= dx << k
            k += dk
            vals.append(v)
            nb.append(k)
    vals.append(code_ll[256])
    nb.append(len_ll[256])
    assert pl.token_at + sum(nb) == bits
    return pl


def code_block(b, final):
    """one block's bytes: stored or dynamic, padded to a byte; the sync marker behind it unless `final`"""
    pl = plan_block(b)
    n = pl.n
    if not pl.dynamic:
        tail = b"" if final else SYNC
        return bytes([1 if final else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + pl.data.tobytes() + tail
    tail = b"" if final else (SYNC[1:] if pl.pad >= 3 else SYNC)
    out = np.zeros(pl.dyn_bytes + 8, np.uint8)
    head = (1 if final else 0) | (2 << 1) | ((pl.hlit - 257) << 3) | ((pl.hdist - 1) << 8) | ((pl.hclen - 4) << 13)
    for i in range(pl.hclen):
        head |= pl.len_cl[CL_ORDER[i]] << (17 + 3 * i)
    _put(out, [0], [head & ((1 << 40) - 1)], 40)
    _put(out, [40], [head >> 40], 40)
    nb = np.array([pl.len_cl[s] for s in pl.seq], np.int64)
    offs = 17 + 3 * pl.hclen + np.concatenate(([0], np.cumsum(nb)[:-1]))
    _put(out, offs, [pl.code_cl[s] for s in pl.seq], nb)
    nb = np.array(pl.widths, np.int64)
    offs = pl.token_at + np.concatenate(([0], np.cumsum(nb)[:-1]))
    _put(out, offs, pl.vals, nb)
    return out[:pl.dyn_bytes].tobytes() + tail


def deflate(payload):
    """the raw RFC 1951 stream of `payload` (bytes-like), as acimg.deflate.DeviceDeflater.deflate writes it"""
    payload = bytes(payload)
    if not payload:
        return EMPTY_FINAL
    n = len(payload)
    return b"".join(code_block(payload[s:s + BLOCK], s + BLOCK >= n) for s in range(0, n, BLOCK))
