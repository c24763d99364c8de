// The containers' checksums on the GPU - CRC-32 (zlib / gzip / PNG), CRC-32C (TFRecord, plain or masked), Adler-32 (zlib) -
// and the gather that assembles framed records from pieces: what lets `--assemble device` of `python -m acimg.convert` and
// `png.encode_png_many` finish a file's bytes where its payload lives.  Integer arithmetic throughout,
// no atomics: a value is a function of the input alone.  tests/checksum_ref.py restates the algebra.
//
// Algebra.  A 32-bit value stands for a polynomial over GF(2) in the reflected order of the standards: bit 31 is x^0, bit 0
//   is x^31, so "times x" is a right shift with the polynomial XORed in when a one falls out.  Without its init and its
//   final XOR a CRC is linear: pure(D) = D(x) x^32 mod P, pure(A || B) = pure(A) x^(8 |B|) ^ pure(B), zero bytes in FRONT
//   of D change nothing and k zero bytes BEHIND it multiply by x^(8 k).  The standard's value of n bytes is
//   pure(D) ^ 0xFFFFFFFF x^(8 n) ^ 0xFFFFFFFF (the init register is one more term).  P has the constant term 1, so x has
//   the inverse (P + 1) / x, in this order (poly << 1) | 1.
// Segments.  The address range of `in` is cut on the grid of CS_SEGMENT = 16384 ABSOLUTE bytes; a segment is a payload's
//   part of one grid window (at most n / CS_SEGMENT + 2 per payload).  One workgroup of 256 lanes takes one window, lane t
//   its bytes [64 t, 64 t + 64) as four 16-byte words: an aligned 16-byte load where the word lies inside the payload,
//   bytewise where a payload's first or last byte cuts it, no load at all outside; bytes outside the payload count as 0.
//   Horner over the word's dwords d0..d3 (little endian): c = (c ^ d0) x^128 ^ d1 x^96 ^ d2 x^64 ^ d3 x^32.
//   Then a butterfly (__shfl_xor): at level k the lower lane's value is multiplied by x^(512 * 2^k), the bits of the
//   upper block; the four waves combine through LDS with x^32768, x^65536, x^98304.  EVERY such multiplier is a
//   compile-time constant: 32 masked XORs of literals, no table, no LDS traffic with data-dependent addresses.  The
//   window's value - the payload's part followed by z = CS_SEGMENT - hi zero bytes - is multiplied ONCE at run time (a
//   32-step shift-and-add) by the segment's host-built multiplier x^(8 (bytes of the payload behind the segment)) x^(-8 z).
// Adler-32.  A = 1 + sum b, B = n + sum (n - i) b (mod 65521).  A lane sums its bytes (a <= 16320) and their weights
//   64..1 (b), and adds (hi - 64 (t + 1)) a: every byte then weighs its distance to the segment's end; reduced mod 65521
//   per lane, so the 32-bit sums over the workgroup stay below 2^25.  The segment's multiplier is the payload's bytes
//   behind it mod 65521; 64-bit products in one lane only.
// checksum_finish_kernel, one wave per payload: XOR (or sum) of its segments' values, the init term, the final XOR, the
//   TFRecord mask for kind 2; the value goes to out[i] and, where asked, as four little-endian bytes to store_base +
//   store_at[i] (byte stores: any alignment).  A payload of 0 bytes has no segment and gets the standard's value here.
// record_gather_kernel: segment s of the table {dst_off, src_off, len, which} is copied by the workgroups (s, 0..GT_Y-1),
//   16384 bytes at a time; 16-byte moves where dst and src are congruent mod 16, 4-byte moves where mod 4, bytes else and
//   at the edges.  Exactly the bytes [dst_off, dst_off + len) are written.
#include <algorithm>
#include <utility>
#include <vector>

#include "common.hpp"

namespace acimg {

constexpr int CS_SEGMENT = ACIMG_CHECKSUM_SEGMENT;
constexpr int CS_THREADS = 256;
constexpr int CS_RUN = CS_SEGMENT / CS_THREADS;     // a lane's bytes
constexpr uint32_t CS_POLY_CRC32 = 0xEDB88320u, CS_POLY_CRC32C = 0x82F63B78u;
constexpr uint32_t CS_ADLER = 65521u;
constexpr uint32_t CS_MASK_DELTA = 0xa282ead8u;
constexpr int GT_CHUNK = 16384, GT_Y = 8;
static_assert(CS_RUN == 64 && CS_THREADS == 256, "the butterfly's constants are those of 64-byte runs and four waves");

// ---- GF(2) polynomials mod P, reflected ------------------------------------------------------------------------------------
constexpr __host__ __device__ uint32_t gf_mulx(uint32_t v, uint32_t poly) { return (v >> 1) ^ ((v & 1u) ? poly : 0u); }
constexpr __host__ __device__ uint32_t gf_mul(uint32_t a, uint32_t b, uint32_t poly) {
    uint32_t r = 0;
    for (int i = 0; i < 32; ++i) {
        if (a & (0x80000000u >> i)) r ^= b;
        b = gf_mulx(b, poly);
    }
    return r;
}
constexpr uint32_t gf_pow(uint32_t base, unsigned long e, uint32_t poly) {
    uint32_t r = 0x80000000u;                       // the polynomial 1
    while (e) {
        if (e & 1) r = gf_mul(r, base, poly);
        base = gf_mul(base, base, poly);
        e >>= 1;
    }
    return r;
}
constexpr uint32_t gf_xpow(unsigned long e, uint32_t poly) { return gf_pow(0x40000000u, e, poly); }
constexpr uint32_t gf_xinv(uint32_t poly) { return (poly << 1) | 1u; }
static_assert(gf_mulx(gf_xinv(CS_POLY_CRC32), CS_POLY_CRC32) == 0x80000000u, "x^-1 of CRC-32");
static_assert(gf_mulx(gf_xinv(CS_POLY_CRC32C), CS_POLY_CRC32C) == 0x80000000u, "x^-1 of CRC-32C");

// v * x^E mod P for a compile-time E: bit I of v stands for x^(31 - I)
template <uint32_t POLY, int E, int I>
struct CsTerm {
    enum : uint32_t { value = gf_xpow((unsigned long)(E + 31 - I), POLY) };
};
template <uint32_t POLY, int E, size_t... I>
__device__ __forceinline__ uint32_t cs_mulc_bits(uint32_t v, std::index_sequence<I...>) {
    return (((0u - ((v >> I) & 1u)) & (uint32_t)CsTerm<POLY, E, (int)I>::value) ^ ...);
}
template <uint32_t POLY, int E>
__device__ __forceinline__ uint32_t cs_mulc(uint32_t v) {
    return cs_mulc_bits<POLY, E>(v, std::make_index_sequence<32>());
}

struct CsSegment {      // built on the host by acimg_checksum
    long base;          // the window's first byte relative to `in` (negative where `in` starts inside a window)
    int lo, hi;         // the payload's bytes of the window: [lo, hi), 0 <= lo < hi <= CS_SEGMENT
    uint32_t mult;      // CRC: x^(8 behind) x^(-8 (CS_SEGMENT - hi)); Adler: behind mod 65521
    int payload;
};
struct CsPayload {
    long store_at;      // < 0: no store
    int first, nseg;    // its segments
    uint32_t init;      // CRC: 0xFFFFFFFF x^(8 n); Adler: n mod 65521
    int reserved;
};

// the window's bytes [o, o + 16) that lie in [lo, hi) as four little-endian dwords; the others are 0 and are not read
__device__ __forceinline__ uint4 cs_load16(const uint8_t* win, int o, int lo, int hi) {
    if (o >= lo && o + 16 <= hi) return *reinterpret_cast<const uint4*>(win + o);
    uint32_t w0 = 0, w1 = 0, w2 = 0, w3 = 0;
    if (o + 16 > lo && o < hi) {
#pragma unroll
        for (int k = 0; k < 16; ++k) {
            const int i = o + k;
            const uint32_t b = (i >= lo && i < hi) ? (uint32_t)win[i] << (8 * (k & 3)) : 0u;
            if (k < 4) w0 |= b;
            else if (k < 8) w1 |= b;
            else if (k < 12) w2 |= b;
            else w3 |= b;
        }
    }
    return make_uint4(w0, w1, w2, w3);
}

template <uint32_t POLY, int E>
__device__ __forceinline__ uint32_t cs_level(uint32_t c, int offset) {
    const uint32_t other = __shfl_xor(c, offset, 64);
    const bool upper = (threadIdx.x & offset) != 0;
    return cs_mulc<POLY, E>(upper ? other : c) ^ (upper ? c : other);
}

// one workgroup per segment
template <uint32_t POLY>
__global__ __launch_bounds__(CS_THREADS) void checksum_crc_kernel(const uint8_t* in, const CsSegment* segs, uint2* vals) {
    __shared__ uint32_t s_wave[CS_THREADS / 64];
    const CsSegment s = segs[blockIdx.x];
    const uint8_t* win = in + s.base;
    const int t = threadIdx.x, o = CS_RUN * t;
    uint32_t c = 0;
    if (o < s.hi && o + CS_RUN > s.lo) {
#pragma unroll
        for (int j = 0; j < CS_RUN / 16; ++j) {
            const uint4 w = cs_load16(win, o + 16 * j, s.lo, s.hi);
            c = cs_mulc<POLY, 128>(c ^ w.x) ^ cs_mulc<POLY, 96>(w.y) ^ cs_mulc<POLY, 64>(w.z) ^ cs_mulc<POLY, 32>(w.w);
        }
    }
    c = cs_level<POLY, 8 * CS_RUN>(c, 1);
    c = cs_level<POLY, 16 * CS_RUN>(c, 2);
    c = cs_level<POLY, 32 * CS_RUN>(c, 4);
    c = cs_level<POLY, 64 * CS_RUN>(c, 8);
    c = cs_level<POLY, 128 * CS_RUN>(c, 16);
    c = cs_level<POLY, 256 * CS_RUN>(c, 32);
    if ((t & 63) == 0) s_wave[t >> 6] = c;
    __syncthreads();
    if (t == 0) {
        constexpr int W = 8 * 64 * CS_RUN;          // a wave's bits
        const uint32_t r = cs_mulc<POLY, 3 * W>(s_wave[0]) ^ cs_mulc<POLY, 2 * W>(s_wave[1]) ^ cs_mulc<POLY, W>(s_wave[2]) ^ s_wave[3];
        vals[blockIdx.x] = make_uint2(gf_mul(r, s.mult, POLY), 0u);
    }
}

__global__ __launch_bounds__(CS_THREADS) void checksum_adler_kernel(const uint8_t* in, const CsSegment* segs, uint2* vals) {
    __shared__ uint32_t s_a[CS_THREADS / 64], s_b[CS_THREADS / 64];
    const CsSegment s = segs[blockIdx.x];
    const uint8_t* win = in + s.base;
    const int t = threadIdx.x, o = CS_RUN * t;
    uint32_t a = 0, b = 0;
    if (o < s.hi && o + CS_RUN > s.lo) {
#pragma unroll
        for (int j = 0; j < CS_RUN / 16; ++j) {
            const uint4 w = cs_load16(win, o + 16 * j, s.lo, s.hi);
            const uint32_t d[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
            for (int k = 0; k < 16; ++k) {
                const uint32_t v = (d[k >> 2] >> (8 * (k & 3))) & 0xFFu;
                a += v;
                b += (uint32_t)(CS_RUN - 16 * j - k) * v;
            }
        }
        // every byte's weight becomes its distance to the segment's end: never negative in the sum (absent bytes are 0)
        b = (uint32_t)((int)b + (s.hi - (o + CS_RUN)) * (int)a) % CS_ADLER;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        a += __shfl_xor(a, off, 64);
        b += __shfl_xor(b, off, 64);
    }
    if ((t & 63) == 0) {
        s_a[t >> 6] = a;
        s_b[t >> 6] = b;
    }
    __syncthreads();
    if (t == 0) {
        const uint32_t A = (s_a[0] + s_a[1] + s_a[2] + s_a[3]) % CS_ADLER;
        const unsigned long long B = (unsigned long long)(s_b[0] + s_b[1] + s_b[2] + s_b[3]) + (unsigned long long)s.mult * A;
        vals[blockIdx.x] = make_uint2(A, (uint32_t)(B % CS_ADLER));
    }
}

// one wave per payload
__global__ __launch_bounds__(64) void checksum_finish_kernel(const CsPayload* payloads, const uint2* vals, int kind, uint32_t* out,
                                                             uint8_t* store_base) {
    const CsPayload p = payloads[blockIdx.x];
    const int lane = threadIdx.x;
    uint32_t v;
    if (kind == ACIMG_CHECKSUM_ADLER32) {
        unsigned long long a = 0, b = 0;
        for (int i = lane; i < p.nseg; i += 64) {
            const uint2 s = vals[p.first + i];
            a += s.x;
            b += s.y;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            a += __shfl_xor(a, off, 64);
            b += __shfl_xor(b, off, 64);
        }
        v = (uint32_t)((b + p.init) % CS_ADLER) << 16 | (uint32_t)((a + 1) % CS_ADLER);
    } else {
        uint32_t x = 0;
        for (int i = lane; i < p.nseg; i += 64) x ^= vals[p.first + i].x;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) x ^= __shfl_xor(x, off, 64);
        v = x ^ p.init ^ 0xFFFFFFFFu;
        if (kind == ACIMG_CHECKSUM_CRC32C_MASKED) v = ((v >> 15) | (v << 17)) + CS_MASK_DELTA;
    }
    if (lane == 0) {
        out[blockIdx.x] = v;
        if (store_base && p.store_at >= 0) {
            uint8_t* d = store_base + p.store_at;
            d[0] = (uint8_t)v;
            d[1] = (uint8_t)(v >> 8);
            d[2] = (uint8_t)(v >> 16);
            d[3] = (uint8_t)(v >> 24);
        }
    }
}

struct GatherSegment {  // a row of the caller's table
    long dst_off, src_off, len, which;
};

template <typename T>
__device__ __forceinline__ void gt_copy(uint8_t* d, const uint8_t* s, long n) {     // n bytes, both T-aligned
    for (long i = (long)threadIdx.x * (long)sizeof(T); i < n; i += (long)CS_THREADS * (long)sizeof(T))
        *reinterpret_cast<T*>(d + i) = *reinterpret_cast<const T*>(s + i);
}

__global__ __launch_bounds__(CS_THREADS) void record_gather_kernel(const uint8_t* src0, const uint8_t* src1, const GatherSegment* segs,
                                                                   uint8_t* dst) {
    const GatherSegment g = segs[blockIdx.x];
    const uint8_t* src = (g.which ? src1 : src0) + g.src_off;
    uint8_t* out = dst + g.dst_off;
    for (long at = (long)blockIdx.y * GT_CHUNK; at < g.len; at += (long)gridDim.y * GT_CHUNK) {
        const long n = min((long)GT_CHUNK, g.len - at);
        uint8_t* d = out + at;
        const uint8_t* s = src + at;
        const unsigned rel = (unsigned)((uintptr_t)d ^ (uintptr_t)s);
        const int unit = (rel & 15u) == 0 ? 16 : (rel & 3u) == 0 ? 4 : 1;
        long head = unit == 1 ? n : (long)((0 - (uintptr_t)d) & (uintptr_t)(unit - 1));     // bytes before d is unit-aligned
        if (head > n) head = n;
        const long body = (n - head) / unit * unit;
        for (long i = threadIdx.x; i < head; i += CS_THREADS) d[i] = s[i];
        if (unit == 16) gt_copy<uint4>(d + head, s + head, body);
        else if (unit == 4) gt_copy<uint32_t>(d + head, s + head, body);
        for (long i = head + body + threadIdx.x; i < n; i += CS_THREADS) d[i] = s[i];
    }
}

inline size_t cs_align16(size_t v) { return (v + 15) & ~(size_t)15; }

// What the host needs to build a call's multipliers cheaply, per polynomial, built once: the powers x^(8 * 2^k) and
// x^(-8 * 2^k), and a byte-sliced table of "times x^(8 CS_SEGMENT)".  Walking a payload's segments from the last to the
// first, the multiplier starts as x^(-8 z) (z zeros behind the payload in its last window) and is multiplied by
// x^(8 CS_SEGMENT) per step: hi_last = CS_SEGMENT - z, so the recurrence is uniform - one power per payload, four
// look-ups per segment.
struct CsHost {
    uint32_t poly, xp[32], xn[15], seg[4][256];
    explicit CsHost(uint32_t p) : poly(p) {
        xp[0] = gf_xpow(8, p);
        for (int k = 1; k < 32; ++k) xp[k] = gf_mul(xp[k - 1], xp[k - 1], p);
        xn[0] = gf_pow(gf_xinv(p), 8, p);
        for (int k = 1; k < 15; ++k) xn[k] = gf_mul(xn[k - 1], xn[k - 1], p);
        static_assert(CS_SEGMENT == 1 << 14, "xp[14] is x^(8 CS_SEGMENT)");
        for (int j = 0; j < 4; ++j)
            for (uint32_t b = 0; b < 256; ++b) seg[j][b] = gf_mul(b << (8 * j), xp[14], p);
    }
    uint32_t xpow8(unsigned long n) const {         // x^(8 n), n < 2^32
        uint32_t r = 0x80000000u;
        for (int k = 0; n; ++k, n >>= 1)
            if (n & 1) r = gf_mul(r, xp[k], poly);
        return r;
    }
    uint32_t xneg8(unsigned n) const {              // x^(-8 n), n < 2^15
        uint32_t r = 0x80000000u;
        for (int k = 0; n; ++k, n >>= 1)
            if (n & 1) r = gf_mul(r, xn[k], poly);
        return r;
    }
    uint32_t times_segment(uint32_t v) const { return seg[0][v & 0xFF] ^ seg[1][(v >> 8) & 0xFF] ^ seg[2][(v >> 16) & 0xFF] ^ seg[3][v >> 24]; }
};
inline const CsHost& cs_host(int kind) {
    static const CsHost crc32(CS_POLY_CRC32), crc32c(CS_POLY_CRC32C);
    return kind == ACIMG_CHECKSUM_CRC32 ? crc32 : crc32c;
}
constexpr long CS_MAX_LENGTH = (1L << 31) - 1;

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_checksum_workspace(long total_bytes, int count) {
    if (total_bytes < 0 || count < 1 || total_bytes / count > CS_MAX_LENGTH) return 0;
    const size_t segs = (size_t)(total_bytes / CS_SEGMENT) + 2 * (size_t)count;     // a payload ends and starts inside a window
    return cs_align16(segs * sizeof(CsSegment)) + cs_align16((size_t)count * sizeof(CsPayload)) + cs_align16(segs * sizeof(uint2));
}

int acimg_checksum(const uint8_t* in, const long* lengths, int count, int kind, uint32_t* out, uint8_t* store_base,
                   const long* store_at, void* ws, size_t ws_bytes, void* stream) {
    if (!in || !lengths || !out || !ws) return fail(ACIMG_EINVAL, "checksum: null argument");
    if (store_at && !store_base) return fail(ACIMG_EINVAL, "checksum: store_at without store_base");
    if (count < 1) return fail(ACIMG_EINVAL, "checksum: count = %d must be positive", count);
    if (kind < ACIMG_CHECKSUM_CRC32 || kind > ACIMG_CHECKSUM_ADLER32) return fail(ACIMG_EINVAL, "checksum: unknown kind %d", kind);
    long total = 0;
    for (int i = 0; i < count; ++i) {
        if (lengths[i] < 0 || lengths[i] > CS_MAX_LENGTH)
            return fail(ACIMG_EINVAL, "checksum: payload %d has %ld bytes, outside 0 .. 2^31 - 1", i, lengths[i]);
        total += lengths[i];
    }
    if (!aligned16(ws)) return fail(ACIMG_EINVAL, "checksum: ws must be 16-byte aligned");
    const size_t need = acimg_checksum_workspace(total, count);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "checksum: workspace %zu < %zu bytes", ws_bytes, need);
    const bool adler = kind == ACIMG_CHECKSUM_ADLER32;
    const CsHost& H = cs_host(kind);
    const size_t max_segs = (size_t)(total / CS_SEGMENT) + 2 * (size_t)count;
    const size_t seg_bytes = cs_align16(max_segs * sizeof(CsSegment)), pay_bytes = cs_align16((size_t)count * sizeof(CsPayload));
    std::vector<uint8_t> table(seg_bytes + pay_bytes, 0);
    CsSegment* segs = reinterpret_cast<CsSegment*>(table.data());
    CsPayload* pays = reinterpret_cast<CsPayload*>(table.data() + seg_bytes);
    const uintptr_t base = reinterpret_cast<uintptr_t>(in);
    long at = 0;
    size_t ns = 0;
    for (int i = 0; i < count; ++i) {
        const long n = lengths[i];
        pays[i].store_at = store_at ? store_at[i] : -1;
        pays[i].first = (int)ns;
        pays[i].init = adler ? (uint32_t)(n % CS_ADLER) : gf_mul(0xFFFFFFFFu, H.xpow8((unsigned long)n), H.poly);
        const uintptr_t a0 = base + (uintptr_t)at, a1 = a0 + (uintptr_t)n;
        for (uintptr_t w = a0 & ~(uintptr_t)(CS_SEGMENT - 1); w < a1; w += CS_SEGMENT, ++ns) {
            if (ns >= max_segs) return fail(ACIMG_EINVAL, "checksum: more than %zu segments", max_segs);     // cannot happen
            CsSegment& s = segs[ns];
            s.base = (long)(w - base);              // two's complement: negative before `in`
            s.lo = w < a0 ? (int)(a0 - w) : 0;
            s.hi = a1 - w < (uintptr_t)CS_SEGMENT ? (int)(a1 - w) : CS_SEGMENT;
            s.payload = i;
            s.mult = (uint32_t)((unsigned long)(a1 - (w + (uintptr_t)s.hi)) % CS_ADLER);       // Adler: the bytes behind
        }
        pays[i].nseg = (int)ns - pays[i].first;
        if (!adler && pays[i].nseg) {               // CRC: x^(8 behind) x^(-8 z), from the last segment to the first
            uint32_t m = H.xneg8((unsigned)(CS_SEGMENT - segs[ns - 1].hi));
            for (size_t k = ns; k-- > (size_t)pays[i].first; m = H.times_segment(m)) segs[k].mult = m;
        }
        at += n;
    }
    if (ns > (size_t)INT32_MAX) return fail(ACIMG_EINVAL, "checksum: %zu segments exceed the grid", ns);
    CsSegment* d_segs = (CsSegment*)ws;
    CsPayload* d_pays = (CsPayload*)((uint8_t*)ws + seg_bytes);
    uint2* vals = (uint2*)((uint8_t*)ws + seg_bytes + pay_bytes);
    hipStream_t s = (hipStream_t)stream;
    // the tables are host memory of this call: they have reached the device before the call returns
    hipError_t e = hipMemcpyAsync(ws, table.data(), table.size(), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "checksum (tables): %s", hipGetErrorString(e));
    if (ns) {
        if (adler)
            hipLaunchKernelGGL(checksum_adler_kernel, dim3((unsigned)ns), dim3(CS_THREADS), 0, s, in, (const CsSegment*)d_segs, vals);
        else if (kind == ACIMG_CHECKSUM_CRC32)
            hipLaunchKernelGGL(checksum_crc_kernel<CS_POLY_CRC32>, dim3((unsigned)ns), dim3(CS_THREADS), 0, s, in,
                               (const CsSegment*)d_segs, vals);
        else
            hipLaunchKernelGGL(checksum_crc_kernel<CS_POLY_CRC32C>, dim3((unsigned)ns), dim3(CS_THREADS), 0, s, in,
                               (const CsSegment*)d_segs, vals);
        const int rc = check_launch("checksum (segments)");
        if (rc) return rc;
    }
    hipLaunchKernelGGL(checksum_finish_kernel, dim3((unsigned)count), dim3(64), 0, s, (const CsPayload*)d_pays, (const uint2*)vals, kind,
                       out, store_at ? store_base : (uint8_t*)nullptr);
    return check_launch("checksum (finish)");
}

size_t acimg_record_gather_workspace(int nseg) {
    if (nseg < 1) return 0;
    return cs_align16((size_t)nseg * sizeof(GatherSegment));
}

int acimg_record_gather(const uint8_t* src0, const uint8_t* src1, const long* segments, int nseg, uint8_t* dst, size_t dst_bytes,
                        void* ws, size_t ws_bytes, void* stream) {
    if (!segments || !dst || !ws) return fail(ACIMG_EINVAL, "record_gather: null argument");
    if (nseg < 1) return fail(ACIMG_EINVAL, "record_gather: nseg = %d must be positive", nseg);
    if (!aligned16(ws)) return fail(ACIMG_EINVAL, "record_gather: ws must be 16-byte aligned");
    const size_t need = acimg_record_gather_workspace(nseg);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "record_gather: workspace %zu < %zu bytes", ws_bytes, need);
    std::vector<std::pair<long, long>> spans;       // {dst_off, len} of the segments that write
    for (int i = 0; i < nseg; ++i) {
        const long d = segments[4 * i], so = segments[4 * i + 1], len = segments[4 * i + 2], which = segments[4 * i + 3];
        if (which != 0 && which != 1) return fail(ACIMG_EINVAL, "record_gather: segment %d names source %ld", i, which);
        if (!(which ? src1 : src0)) return fail(ACIMG_EINVAL, "record_gather: segment %d reads src%ld, which is null", i, which);
        if (d < 0 || so < 0 || len < 0 || (size_t)d > dst_bytes || (size_t)len > dst_bytes - (size_t)d)
            return fail(ACIMG_EINVAL, "record_gather: segment %d = {dst %ld, src %ld, len %ld} outside dst of %zu bytes", i, d, so, len,
                        dst_bytes);
        if (len) spans.emplace_back(d, len);
    }
    std::sort(spans.begin(), spans.end());
    for (size_t i = 1; i < spans.size(); ++i)
        if (spans[i - 1].first + spans[i - 1].second > spans[i].first)
            return fail(ACIMG_EINVAL, "record_gather: segments overlap in dst at byte %ld", spans[i].first);
    hipStream_t s = (hipStream_t)stream;
    // the table is host memory of this call: it has reached the device before the call returns
    hipError_t e = hipMemcpyAsync(ws, segments, (size_t)nseg * sizeof(GatherSegment), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "record_gather (table): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(record_gather_kernel, dim3((unsigned)nseg, GT_Y), dim3(CS_THREADS), 0, s, src0, src1, (const GatherSegment*)ws,
                       dst);
    return check_launch("record_gather");
}

}  // extern "C"
