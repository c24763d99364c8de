// INFLATE (RFC 1951) of raw deflate streams on the GPU: the reader behind `DeviceDataLoader(inflate="device")`, where the
// workers' zlib bounds the pass.  A deflate stream is one bit-serial chain; the parallelism is found
// INSIDE it: block starts are searched speculatively, chunks decode side by side with the unknown 32 KiB window carried as
// 16-bit markers, and the markers are resolved afterwards (the two-stage scheme of pugz / rapidgzip).  Integer arithmetic
// throughout; tests/inflate_ref.py restates every rule below, and the device's chunk table equals the restatement's.
//
// A stream of n bytes is cut into chunks of C = chunk_bytes compressed bytes.  Launches of one acimg_inflate call:
//   1 inflate_find_kernel, a workgroup per chunk j >= 1: the bit offsets [8jC, min(8(j+1)C, 8n)) are tested one per lane in
//     ascending sweeps; the chunk's start is the lowest offset o at which: bit o is 0 and BTYPE is 2; HLIT, HDIST <= 29; the
//     code-length code (HCLEN + 4 lengths, the rest 0) has Kraft sum exactly 1; the HLIT + 257 + HDIST + 1 lengths decode
//     inside the stream with no repeat-16 before a first length and no overrun of the total; symbol 256 has a length; the
//     literal/length code is complete; the distance code is complete or has at most one length.  A lane does this alone, in
//     registers: the 19 code-length lengths are 3-bit fields of one 64-bit word, their canonical order 5-bit fields of two.
//     Only dynamic headers are sought (a fixed block has nothing to check, a stored block's LEN / ~LEN too little).
//   2 inflate_chunk_kernel<false> (count), ONE WAVE per chunk with a start: decodes without writing, sums the bytes, and at
//     every block boundary b looks at the chunk whose range holds b: if that is a later chunk and b is its start, b is the
//     link and the wave stops; it also stops past the BFINAL block.  An invalid code or code set, BTYPE 3, LEN != ~NLEN,
//     a distance before the stream (chunk 0), a read past n or more bytes than out_len end it with a status, never a fault.
//   3 inflate_chain_kernel, a thread per stream: walks the links from chunk 0; the chunks on the chain are live and get
//     their exclusive output offsets; the stream's status is the first live failure, else SIZE when the total differs
//     from out_len.  A live chunk's start is a true boundary because a live decoder reached it; everything else was
//     wasted work and is ignored whatever its status.
//   4 inflate_chunk_kernel<true> (decode): the live chunks again, writing uint16 symbols at their offsets: a byte, or
//     0x8000 + (32768 - k) for "the byte k before this chunk's first".  Copies copy symbols, so markers propagate.  A
//     distance that reaches before the stream's first byte (known now: the offset is) is CORRUPT.
//   5 inflate_resolve_kernel, a workgroup per stream: in chain order, replaces the markers in each live chunk's last 32768
//     symbols (all of a shorter chunk) from the 32768 symbols before the chunk's offset - resolved already by the order
//     of the walk, also when short chunks make that span reach back several chunks.
//   6 inflate_finish_kernel: every symbol to its byte; a marker left at position i of chunk j reads
//     sym[offset_j - 32768 + (m - 0x8000)], which lies in a resolved tail.
// The wave decoder.  Bit buffer (64 bits), position and every decision are wave-uniform; lanes differ only where they
//   share work.  A canonical code lives in lanes 1..15: lane L holds the left-aligned limit (first[L] + count[L]) << (15 - L),
//   first[L] and the index of the length's first symbol; a symbol is decoded by comparing the next 15 bits, reversed, with
//   every limit at once - the lowest lane of the ballot is the length - and one LDS read of the symbols sorted by
//   (length, symbol).  The sort is 15 ballots per 64 symbols.  Stored blocks and copies are moved by the whole wave; a
//   copy reads sym[p - dist + i % dist], all written before it began.  Literals wait in a register, one per lane, and leave 64 at a time or
//   before a copy; a wavefront fence orders the wave's stores before a copy's loads.  The stream is read with aligned scalar
//   dword loads; every uniform value is passed through readfirstlane so that the decoder's control flow is scalar.  LDS per wave: 320 lengths + 288 + 32 sorted symbols = 960 bytes.
// Every loop consumes at least one bit per turn and ends at 8n; every store is guarded by the stream's out_len.
#include <vector>

#include "common.hpp"

namespace acimg {

constexpr int IF_WAVES = 4;             // chunks per workgroup of the chunk kernel (one wave each, no workgroup barrier)
constexpr int IF_FIND_THREADS = 1024;
constexpr int IF_WINDOW = 32768;
constexpr int IF_MARK = 0x8000;
constexpr int IF_FINISH_SPLIT = 8;      // workgroups per chunk in the finish pass
constexpr int IF_MIN_CHUNK = 256, IF_MAX_CHUNK = 1 << 24;

__constant__ uint8_t c_if_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

typedef AcimgInflateChunk Chunk;

// ---- 1 find: one lane checks one offset ----------------------------------------------------------------------------------
struct LaneBits {   // a lane's own reader; bits past the stream read as 0, consuming them sets `bad`
    const uint8_t* s;
    long n, next;   // stream bytes; the next byte to load
    uint64_t bb;
    int nb;
    bool bad;
    __device__ void fill() {
        while (nb <= 56) {
            bb |= (uint64_t)(next < n ? s[next] : 0) << nb;
            ++next;
            nb += 8;
        }
    }
    __device__ long pos() const { return 8 * next - nb; }
    __device__ uint32_t take(int k) {   // k <= 16
        if (nb < k) fill();
        if (pos() + k > 8 * n) bad = true;
        const uint32_t v = (uint32_t)bb & ((1u << k) - 1);
        bb >>= k;
        nb -= k;
        return v;
    }
};

__device__ bool find_check(const uint8_t* s, long n, long o) {
    LaneBits b{s, n, o >> 3, 0, 0, false};
    b.fill();
    b.bb >>= (o & 7);
    b.nb -= (int)(o & 7);
    if (b.take(3) != 4) return false;   // BFINAL 0, BTYPE 2
    const int hlit = b.take(5), hdist = b.take(5), hclen = b.take(4);
    if (hlit > 29 || hdist > 29) return false;
    uint64_t clp = 0, cntp = 0;   // lengths of the 19 symbols (3 bits each); symbols per length 0..7 (5 bits each)
    for (int i = 0; i < hclen + 4; ++i) {
        const uint64_t v = b.take(3);
        clp |= v << (3 * c_if_order[i]);
        cntp += 1ull << (5 * v);
    }
    if (b.bad) return false;
    int kraft = 0;
    for (int L = 1; L <= 7; ++L) kraft += (int)((cntp >> (5 * L)) & 31) << (7 - L);
    if (kraft != 128) return false;
    // canonical order: first code (7 bits) and first index (5 bits) per length, symbols by (length, symbol) in 5-bit fields
    uint64_t firstp = 0, indexp = 0, sorted[2] = {0, 0};
    int code = 0, at = 0;
    for (int L = 1; L <= 7; ++L) {
        code = (code + (L > 1 ? (int)((cntp >> (5 * (L - 1))) & 31) : 0)) << 1;
        firstp |= (uint64_t)code << (7 * L);
        indexp |= (uint64_t)at << (5 * L);
        for (int sym = 0; sym < 19; ++sym)
            if ((int)((clp >> (3 * sym)) & 7) == L) {
                sorted[at >= 12] |= (uint64_t)sym << (5 * (at >= 12 ? at - 12 : at));
                ++at;
            }
    }
    const int nll = hlit + 257, total = nll + hdist + 1;
    int have = 0, prev = -1, kll = 0, kd = 0, nzd = 0;
    bool has256 = false;
    while (have < total) {
        if (b.nb < 7) b.fill();
        const int c7 = (int)(__brev((uint32_t)b.bb) >> 25);
        int sym = -1, len = 0;
        for (int L = 1; L <= 7; ++L) {
            const int idx = (c7 >> (7 - L)) - (int)((firstp >> (7 * L)) & 127);
            if (idx >= 0 && idx < (int)((cntp >> (5 * L)) & 31)) {
                const int k = idx + (int)((indexp >> (5 * L)) & 31);
                sym = (int)((sorted[k >= 12] >> (5 * (k >= 12 ? k - 12 : k))) & 31);
                len = L;
                break;
            }
        }
        if (sym < 0) return false;   // cannot happen with a complete code
        b.take(len);
        int rep = 1, val = sym;
        if (sym == 16) {
            if (prev < 0) return false;
            rep = 3 + (int)b.take(2);
            val = prev;
        } else if (sym == 17) {
            rep = 3 + (int)b.take(3);
            val = 0;
        } else if (sym == 18) {
            rep = 11 + (int)b.take(7);
            val = 0;
        }
        if (b.bad || have + rep > total) return false;
        prev = val;
        if (val)
            for (int r = 0; r < rep; ++r) {
                const int i = have + r;
                if (i < nll) {
                    kll += 1 << (15 - val);
                    has256 = has256 || i == 256;
                } else {
                    kd += 1 << (15 - val);
                    ++nzd;
                }
            }
        have += rep;
    }
    return has256 && kll == IF_WINDOW && (kd == IF_WINDOW || nzd <= 1);
}

__global__ __launch_bounds__(IF_FIND_THREADS) void inflate_find_kernel(const uint8_t* src, Chunk* table, int chunk_bytes) {
    __shared__ int s_hit;
    Chunk& c = table[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid == 0) {
        c.end = 0, c.length = 0, c.offset = 0;
        c.next = -1, c.status = ACIMG_INFLATE_OK, c.live = 0, c.reserved = 0;
        s_hit = INT32_MAX;
    }
    if (c.index == 0) {
        if (tid == 0) c.start = 0;
        return;
    }
    __syncthreads();
    const uint8_t* s = src + c.src_off;
    const long n = c.src_len, lo = 8L * c.index * chunk_bytes;
    const long hi = min(lo + 8L * chunk_bytes, 8 * n);
    int hit = INT32_MAX;
    for (long base = lo; base < hi; base += IF_FIND_THREADS) {
        const long o = base + tid;
        if (o < hi && find_check(s, n, o)) atomicMin(&s_hit, (int)(o - lo));
        __syncthreads();
        hit = s_hit;
        __syncthreads();   // nobody enters the next sweep's atomicMin before everybody has read this one's result
        if (hit != INT32_MAX) break;
    }
    if (tid == 0) c.start = hit == INT32_MAX ? -1 : lo + hit;
}

// ---- 2, 4 the wave decoder -----------------------------------------------------------------------------------------------
// a value that is the same in every lane, told to the compiler: it then lives in scalar registers and branches are scalar
__device__ __forceinline__ int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ __forceinline__ long uni(long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((uint64_t)v >> 32));
    return (long)(((uint64_t)hi << 32) | lo);
}

struct WaveBits {   // wave-uniform reader: every field is scalar, the stream is read with aligned scalar dword loads
    const uint8_t* s;
    const uint32_t* w;   // s rounded down to a dword; `lead` bytes lie before the stream in its first dword
    long n, nextw;       // stream bytes; the next dword of w to load
    int lead;
    uint64_t bb;
    int nb;
    __device__ __forceinline__ void init(const uint8_t* stream, long bytes) {
        s = stream, n = bytes;
        lead = (int)(reinterpret_cast<uintptr_t>(stream) & 3);
        w = reinterpret_cast<const uint32_t*>(stream - lead);
        nextw = 0, bb = 0, nb = 0;
    }
    // dword i of w with the bytes past the stream zeroed.  A dword that holds one byte of the stream lies in the stream's
    // pages; the bytes before the stream in dword 0 are dropped by seek()
    __device__ __forceinline__ uint32_t word(long i) const {
        const long first = 4 * i - lead;
        if (first >= n) return 0;
        uint32_t v = w[i];
        if (first + 4 > n) v &= (1u << (8 * (int)(n - first))) - 1;
        return v;
    }
    __device__ __forceinline__ void seek(long bit) {
        const long a = bit + 8 * lead;
        nextw = a >> 5, bb = 0, nb = 0;
        ensure();
        bb >>= (a & 31);
        nb -= (int)(a & 31);
    }
    __device__ __forceinline__ void ensure() {   // at least 32 bits
        if (nb >= 32) return;
        bb |= (uint64_t)word(nextw) << nb;
        nextw += 1;
        nb += 32;
    }
    __device__ __forceinline__ long pos() const { return 32 * nextw - nb - 8 * lead; }
    __device__ __forceinline__ bool has(int k) const { return pos() + k <= 8 * n; }
    __device__ __forceinline__ uint32_t peek(int k) const { return (uint32_t)bb & ((1u << k) - 1); }
    __device__ __forceinline__ void drop(int k) {
        bb >>= k;
        nb -= k;
    }
};

struct LaneCode {   // lane L in 1..15 holds the code's length L
    uint32_t limit;
    int first, index;
};

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the code of lens[0 .. nsym) (LDS): the lane table and the symbols sorted by (length, symbol).  Returns 0, or CORRUPT for an
// over-subscribed set or an incomplete one other than no code at all or a single code of length 1 (zlib's rule).
__device__ int build_code(const uint8_t* lens, int nsym, uint16_t* sorted, LaneCode& lc) {
    const int lane = threadIdx.x & 63;
    int cnt = 0;
    for (int g = 0; g < nsym; g += 64) {
        const int l = g + lane < nsym ? lens[g + lane] : 0;
#pragma unroll
        for (int L = 1; L <= 15; ++L) {
            const int c = __popcll(__ballot(l == L));
            if (lane == L) cnt += c;
        }
    }
    int code = 0, at = 0, kraft = 0, prev = 0, c1 = 0;
    lc.limit = 0, lc.first = 0, lc.index = 0;
#pragma unroll
    for (int L = 1; L <= 15; ++L) {
        const int c = __builtin_amdgcn_readlane(cnt, L);
        code = (code + prev) << 1;
        if (lane == L) lc.first = code, lc.index = at, lc.limit = (uint32_t)(code + c) << (15 - L);
        kraft += c << (15 - L);
        at += c;
        prev = c;
        if (L == 1) c1 = c;
    }
    if (kraft > IF_WINDOW || (kraft < IF_WINDOW && at != 0 && !(at == 1 && c1 == 1))) return ACIMG_INFLATE_CORRUPT;
    int run = lc.index;
    const uint64_t below = (1ull << lane) - 1;
    for (int g = 0; g < nsym; g += 64) {
        const int l = g + lane < nsym ? lens[g + lane] : 0;
#pragma unroll
        for (int L = 1; L <= 15; ++L) {
            const uint64_t m = __ballot(l == L);
            const int b = __builtin_amdgcn_readlane(run, L);
            if (l == L) sorted[b + __popcll(m & below)] = (uint16_t)(g + lane);
            if (lane == L) run += __popcll(m);
        }
    }
    wave_lds_sync();
    return 0;
}

// the next symbol of the code; -1: no code matches.  len: its bits (not yet dropped)
__device__ __forceinline__ int decode_sym(const WaveBits& b, const LaneCode& lc, const uint16_t* sorted, int& len) {
    const int lane = threadIdx.x & 63;
    const uint32_t c15 = __brev(b.peek(15)) >> 17;
    const uint64_t m = __ballot(lane >= 1 && lane <= 15 && c15 < lc.limit);
    if (m == 0) {
        len = 0;
        return -1;
    }
    const int L = __builtin_amdgcn_readfirstlane(__ffsll((unsigned long long)m) - 1);
    len = L;
    const int first = __builtin_amdgcn_readlane(lc.first, L), index = __builtin_amdgcn_readlane(lc.index, L);
    return uni((int)sorted[index + (int)(c15 >> (15 - L)) - first]);
}

#define IF_FAIL(st)    \
    {                  \
        status = (st); \
        goto done;     \
    }
#define IF_TAKE(var, k)                              \
    {                                                \
        b.ensure();                                  \
        if (!b.has(k)) IF_FAIL(ACIMG_INFLATE_TRUNCATED); \
        var = (int)b.peek(k);                        \
        b.drop(k);                                   \
    }
#define IF_DECODE(var, lc, sorted)                                                                  \
    {                                                                                               \
        b.ensure();                                                                                 \
        int len_;                                                                                   \
        var = decode_sym(b, lc, sorted, len_);                                                      \
        if (var < 0) IF_FAIL(b.has(15) ? ACIMG_INFLATE_CORRUPT : ACIMG_INFLATE_TRUNCATED);          \
        if (!b.has(len_)) IF_FAIL(ACIMG_INFLATE_TRUNCATED);                                         \
        b.drop(len_);                                                                               \
    }

template <bool WRITE>
__global__ __launch_bounds__(64 * IF_WAVES) void inflate_chunk_kernel(const uint8_t* __restrict__ src, Chunk* table, int nchunks, int chunk_bytes,
                                                                      uint16_t* sym, int32_t* stream_status) {
    __shared__ uint8_t s_lens[IF_WAVES][320];
    __shared__ uint16_t s_ll[IF_WAVES][288], s_d[IF_WAVES][32];
    const int wave = uni((int)(threadIdx.x >> 6)), lane = threadIdx.x & 63;
    const int ci = blockIdx.x * IF_WAVES + wave;
    if (ci >= nchunks) return;
    Chunk& c = table[ci];
    const long start = uni((long)c.start);
    const int stream = uni(c.stream);
    if (WRITE ? (uni(c.live) == 0 || uni(stream_status[stream]) != ACIMG_INFLATE_OK) : start < 0) return;   // a failed stream's bytes are unspecified
    uint8_t* lens = s_lens[wave];
    uint16_t *sorted_ll = s_ll[wave], *sorted_d = s_d[wave];
    const long n = uni((long)c.src_len), out_len = uni((long)c.out_len), base = WRITE ? uni((long)c.offset) : 0;
    const int j = uni(c.index);
    const Chunk* stream_chunks = table + uni(c.first);
    const int stream_nchunks = uni(c.nchunks);
    uint16_t* S = sym + uni((long)c.out_off);   // the stream's symbols
    WaveBits b;
    b.init(src + uni((long)c.src_off), n);
    b.seek(start);
    uint16_t pend = 0;   // literals not yet stored: lane i holds the one for position produced - pend_n + i
    int pend_n = 0;
    long produced = 0;
    int status = ACIMG_INFLATE_OK, next = -1;
    bool begun = false;
    LaneCode ll, dd;

    for (;;) {
        if (begun) {   // a block boundary: the start of a later chunk?
            const long p = b.pos();
            const long k = p / (8L * chunk_bytes);
            if (k > j && k < stream_nchunks && uni((long)stream_chunks[k].start) == p) {
                next = (int)k;
                break;
            }
        }
        begun = true;
        int final, btype;
        IF_TAKE(final, 1);
        IF_TAKE(btype, 2);
        if (btype == 3) IF_FAIL(ACIMG_INFLATE_CORRUPT);
        if (btype == 0) {
            b.drop(b.nb & 7);
            int ln, nln;
            IF_TAKE(ln, 16);
            IF_TAKE(nln, 16);
            if (ln != (~nln & 0xFFFF)) IF_FAIL(ACIMG_INFLATE_CORRUPT);
            const long p = b.pos();
            if (p + 8L * ln > 8 * n) IF_FAIL(ACIMG_INFLATE_TRUNCATED);
            if (produced + ln > out_len) IF_FAIL(ACIMG_INFLATE_SIZE);
            if (WRITE) {
                if (lane < pend_n && base + produced - pend_n + lane < out_len) S[base + produced - pend_n + lane] = pend;
                pend_n = 0;   // the waiting literals lie before this block's bytes
                const uint8_t* from = b.s + (p >> 3);
                for (int i = lane; i < ln; i += 64)
                    if (base + produced + i < out_len) S[base + produced + i] = from[i];
            }
            produced += ln;
            b.seek(p + 8L * ln);
        } else {
            if (btype == 1) {
                for (int i = lane; i < 320; i += 64) lens[i] = i < 144 ? 8 : i < 256 ? 9 : i < 280 ? 7 : i < 288 ? 8 : 5;
                wave_lds_sync();
                build_code(lens, 288, sorted_ll, ll);
                build_code(lens + 288, 32, sorted_d, dd);
            } else {
                int hlit, hdist, hclen;
                IF_TAKE(hlit, 5);
                IF_TAKE(hdist, 5);
                IF_TAKE(hclen, 4);
                if (hlit > 29 || hdist > 29) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                if (lane < 19) lens[lane] = 0;
                wave_lds_sync();
                for (int i = 0; i < hclen + 4; ++i) {
                    int v;
                    IF_TAKE(v, 3);
                    if (lane == 0) lens[c_if_order[i]] = (uint8_t)v;
                }
                wave_lds_sync();
                LaneCode cl;
                uint16_t* sorted_cl = sorted_d;   // 19 <= 32 entries; the distance code is built after the lengths are read
                if (build_code(lens, 19, sorted_cl, cl)) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                const int nll = hlit + 257, total = nll + hdist + 1;
                int have = 0, prev = 0;
                while (have < total) {
                    int s;
                    IF_DECODE(s, cl, sorted_cl);
                    int rep = 1, val = s;
                    if (s == 16) {
                        if (have == 0) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                        IF_TAKE(rep, 2);
                        rep += 3, val = prev;
                    } else if (s == 17) {
                        IF_TAKE(rep, 3);
                        rep += 3, val = 0;
                    } else if (s == 18) {
                        IF_TAKE(rep, 7);
                        rep += 11, val = 0;
                    }
                    if (have + rep > total) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                    for (int i = lane; i < rep; i += 64) lens[have + i] = (uint8_t)val;
                    prev = val;
                    have += rep;
                }
                wave_lds_sync();
                if (uni((int)lens[256]) == 0) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                if (build_code(lens, nll, sorted_ll, ll)) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                if (build_code(lens + nll, hdist + 1, sorted_d, dd)) IF_FAIL(ACIMG_INFLATE_CORRUPT);
            }
            for (;;) {
                int s;
                IF_DECODE(s, ll, sorted_ll);
                if (s < 256) {
                    if (produced + 1 > out_len) IF_FAIL(ACIMG_INFLATE_SIZE);
                    if (WRITE) {
                        if (lane == pend_n) pend = (uint16_t)s;
                        if (++pend_n == 64) {
                            if (base + produced - 63 + lane < out_len) S[base + produced - 63 + lane] = pend;
                            pend_n = 0;
                        }
                    }
                    ++produced;
                    continue;
                }
                if (s == 256) break;
                if (s >= 286) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                const int lc = s - 257;
                int len = lc < 8 ? 3 + lc : 258, k = 0, x;
                if (lc >= 8 && lc < 28) {
                    k = (lc - 4) >> 2;
                    len = 3 + ((4 + (lc & 3)) << k);
                }
                IF_TAKE(x, k);
                len += x;
                int ds;
                IF_DECODE(ds, dd, sorted_d);
                if (ds >= 30) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                int dist = 1 + ds;
                k = 0;
                if (ds >= 4) {
                    k = (ds - 2) >> 1;
                    dist = 1 + ((2 + (ds & 1)) << k);
                }
                IF_TAKE(x, k);
                dist += x;
                if (j == 0 && dist > produced) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                if (WRITE && dist > produced + base) IF_FAIL(ACIMG_INFLATE_CORRUPT);
                if (produced + len > out_len) IF_FAIL(ACIMG_INFLATE_SIZE);
                if (WRITE) {
                    if (lane < pend_n && base + produced - pend_n + lane < out_len) S[base + produced - pend_n + lane] = pend;
                    pend_n = 0;
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");   // this wave's earlier stores before these loads
                    for (int i = lane; i < len; i += 64) {
                        const long p = produced - dist + (dist >= len ? i : i % dist);   // before the copy's first symbol
                        const uint16_t v = p >= 0 ? (base + p < out_len ? S[base + p] : 0) : (uint16_t)(IF_MARK + IF_WINDOW + p);
                        if (base + produced + i < out_len) S[base + produced + i] = v;
                    }
                    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
                }
                produced += len;
            }
        }
        if (final) break;
    }
done:
    if (WRITE && lane < pend_n && base + produced - pend_n + lane < out_len) S[base + produced - pend_n + lane] = pend;
    if (lane == 0) {
        if (!WRITE) {
            c.status = status;
            c.length = produced;
            c.end = b.pos();
            c.next = status == ACIMG_INFLATE_OK ? next : -1;
        } else if (status != ACIMG_INFLATE_OK) {
            atomicCAS(&stream_status[stream], ACIMG_INFLATE_OK, status);
        }
    }
}

// ---- 3 chain: a thread per stream ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inflate_chain_kernel(Chunk* table, const int32_t* first, int count, int32_t* status, long* end_bits) {
    const int s = blockIdx.x * 256 + threadIdx.x;
    if (s >= count) return;
    Chunk* ch = table + first[s];
    const int nchunks = ch[0].nchunks;
    const long out_len = ch[0].out_len;
    long total = 0, end = 0;
    int st = ACIMG_INFLATE_OK, j = 0;
    for (int step = 0; step < nchunks && j >= 0; ++step) {
        Chunk& c = ch[j];
        c.live = 1;
        c.offset = total;
        total += c.length;
        if (c.status != ACIMG_INFLATE_OK) {
            st = c.status;
            break;
        }
        if (c.next < 0) end = c.end;
        j = c.next > j && c.next < nchunks ? c.next : -1;
    }
    if (st == ACIMG_INFLATE_OK && total != out_len) st = ACIMG_INFLATE_SIZE;
    status[s] = st;
    end_bits[s] = st == ACIMG_INFLATE_OK ? end : 0;
}

// ---- 5 resolve: a workgroup per stream ---------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void inflate_resolve_kernel(const Chunk* table, const int32_t* first, uint16_t* sym, int32_t* status) {
    const int s = blockIdx.x;
    if (status[s] != ACIMG_INFLATE_OK) return;   // the bytes of a failed stream are unspecified
    const Chunk* ch = table + first[s];
    const int nchunks = ch[0].nchunks;
    const long out_len = ch[0].out_len;
    uint16_t* S = sym + ch[0].out_off;
    bool before = false;
    int j = ch[0].next;
    for (int step = 1; step < nchunks && j > 0 && j < nchunks; ++step) {
        const Chunk& c = ch[j];
        const long off = c.offset, ln = min(c.length, out_len - off);
        for (long i = max(0L, ln - IF_WINDOW) + threadIdx.x; i < ln; i += 1024) {
            const int m = S[off + i];
            if (m >= IF_MARK) {
                const long from = off - IF_WINDOW + (m - IF_MARK);
                if (from < 0) before = true;
                else S[off + i] = S[from];
            }
        }
        __syncthreads();
        j = c.next;
    }
    if (before) atomicCAS(&status[s], ACIMG_INFLATE_OK, ACIMG_INFLATE_CORRUPT);
}

// ---- 6 finish ----------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void inflate_finish_kernel(const Chunk* table, const uint16_t* sym, const int32_t* status, uint8_t* out) {
    const Chunk& c = table[blockIdx.x];
    if (c.live == 0 || status[c.stream] != ACIMG_INFLATE_OK) return;
    const uint16_t* S = sym + c.out_off;
    uint8_t* dst = out + c.out_off;
    const long off = c.offset, ln = min(c.length, c.out_len - off);
    for (long i = (long)blockIdx.y * 256 + threadIdx.x; i < ln; i += 256L * IF_FINISH_SPLIT) {
        int m = S[off + i];
        if (m >= IF_MARK) {
            const long from = off - IF_WINDOW + (m - IF_MARK);
            m = from >= 0 ? S[from] : 0;
        }
        dst[off + i] = (uint8_t)m;
    }
}

inline size_t if_align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline bool if_chunk_ok(int c) { return c >= IF_MIN_CHUNK && c <= IF_MAX_CHUNK && (c & (c - 1)) == 0; }
constexpr long IF_MAX_BYTES = 1L << 40;

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_inflate_workspace(long total_src, long total_out, int count, int chunk_bytes) {
    if (total_src < 1 || total_out < 1 || total_src > IF_MAX_BYTES || total_out > IF_MAX_BYTES || count < 1 || count > total_src ||
        count > total_out || !if_chunk_ok(chunk_bytes))
        return 0;
    const size_t chunks = (size_t)(total_src / chunk_bytes) + (size_t)count;   // every stream ends with at most one short chunk
    return if_align16(chunks * sizeof(Chunk)) + if_align16((size_t)count * sizeof(int32_t)) + if_align16((size_t)total_out * 2);
}

int acimg_inflate(const uint8_t* src, const long* src_lengths, const long* out_lengths, int count, int chunk_bytes, uint8_t* out,
                  int32_t* status, long* end_bits, void* ws, size_t ws_bytes, void* stream) {
    if (!src || !src_lengths || !out_lengths || !out || !status || !end_bits || !ws) return fail(ACIMG_EINVAL, "inflate: null argument");
    if (count < 1) return fail(ACIMG_EINVAL, "inflate: count = %d must be positive", count);
    if (!if_chunk_ok(chunk_bytes))
        return fail(ACIMG_EINVAL, "inflate: chunk_bytes = %d is no power of two in %d..%d", chunk_bytes, IF_MIN_CHUNK, IF_MAX_CHUNK);
    long total_src = 0, total_out = 0, chunks = 0;
    for (int i = 0; i < count; ++i) {
        if (src_lengths[i] < 1 || src_lengths[i] > IF_MAX_BYTES - total_src)
            return fail(ACIMG_EINVAL, "inflate: stream %d has %ld bytes", i, src_lengths[i]);
        if (out_lengths[i] < 1 || out_lengths[i] >= (1L << 31))
            return fail(ACIMG_EINVAL, "inflate: stream %d is expected to inflate to %ld bytes, outside 1..2^31 - 1", i, out_lengths[i]);
        total_src += src_lengths[i];
        total_out += out_lengths[i];
        chunks += (src_lengths[i] + chunk_bytes - 1) / chunk_bytes;
    }
    if (chunks > (long)INT32_MAX / 2) return fail(ACIMG_EINVAL, "inflate: %ld chunks exceed the grid", chunks);
    if (!aligned16(ws)) return fail(ACIMG_EINVAL, "inflate: ws must be 16-byte aligned");
    const size_t need = acimg_inflate_workspace(total_src, total_out, count, chunk_bytes);
    if (need == 0) return fail(ACIMG_EINVAL, "inflate: %d streams of %ld bytes together are outside the decoder's range", count, total_src);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "inflate: workspace %zu < %zu bytes", ws_bytes, need);
    const size_t bound = (size_t)(total_src / chunk_bytes) + (size_t)count;
    std::vector<Chunk> table((size_t)chunks);
    std::vector<int32_t> first((size_t)count);
    long src_off = 0, out_off = 0, at = 0;
    for (int i = 0; i < count; ++i) {
        const long k = (src_lengths[i] + chunk_bytes - 1) / chunk_bytes;
        first[i] = (int32_t)at;
        for (long j = 0; j < k; ++j) {
            Chunk c = {};
            c.src_off = src_off, c.src_len = src_lengths[i], c.out_off = out_off, c.out_len = out_lengths[i];
            c.stream = i, c.index = (int32_t)j, c.first = first[i], c.nchunks = (int32_t)k;
            c.start = -1, c.next = -1;
            table[at + j] = c;
        }
        at += k;
        src_off += src_lengths[i];
        out_off += out_lengths[i];
    }
    Chunk* d_table = (Chunk*)ws;
    uint8_t* p = (uint8_t*)ws + if_align16(bound * sizeof(Chunk));
    int32_t* d_first = (int32_t*)p;
    p += if_align16((size_t)count * sizeof(int32_t));
    uint16_t* d_sym = (uint16_t*)p;
    hipStream_t s = (hipStream_t)stream;
    // the tables are host memory of this call: they have reached the device before the call returns
    hipError_t e = hipMemcpyAsync(d_table, table.data(), (size_t)chunks * sizeof(Chunk), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemcpyAsync(d_first, first.data(), (size_t)count * sizeof(int32_t), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "inflate (chunk table): %s", hipGetErrorString(e));
    const unsigned nc = (unsigned)chunks, groups = (nc + IF_WAVES - 1) / IF_WAVES;
    hipLaunchKernelGGL(inflate_find_kernel, dim3(nc), dim3(IF_FIND_THREADS), 0, s, src, d_table, chunk_bytes);
    int rc = check_launch("inflate (find)");
    if (rc) return rc;
    hipLaunchKernelGGL(inflate_chunk_kernel<false>, dim3(groups), dim3(64 * IF_WAVES), 0, s, src, d_table, (int)nc, chunk_bytes, d_sym,
                       status);
    rc = check_launch("inflate (count)");
    if (rc) return rc;
    hipLaunchKernelGGL(inflate_chain_kernel, dim3((count + 255) / 256), dim3(256), 0, s, d_table, (const int32_t*)d_first, count, status,
                       end_bits);
    rc = check_launch("inflate (chain)");
    if (rc) return rc;
    hipLaunchKernelGGL(inflate_chunk_kernel<true>, dim3(groups), dim3(64 * IF_WAVES), 0, s, src, d_table, (int)nc, chunk_bytes, d_sym,
                       status);
    rc = check_launch("inflate (decode)");
    if (rc) return rc;
    hipLaunchKernelGGL(inflate_resolve_kernel, dim3(count), dim3(1024), 0, s, (const Chunk*)d_table, (const int32_t*)d_first, d_sym, status);
    rc = check_launch("inflate (resolve)");
    if (rc) return rc;
    hipLaunchKernelGGL(inflate_finish_kernel, dim3(nc, IF_FINISH_SPLIT), dim3(256), 0, s, (const Chunk*)d_table, (const uint16_t*)d_sym,
                       (const int32_t*)status, out);
    return check_launch("inflate (finish)");
}

}  // extern "C"
