// DEFLATE (RFC 1951) of byte payloads on the GPU: LZ77 with a greedy parse and one dynamic-Huffman (or stored) block per
// BLOCK input bytes - the encoder behind `--deflate device` of `python -m acimg.convert` / `acimg.convert_boxes` and
// `--png_deflate device` of `python -m acimg.show`, where the host's zlib was the wall.  Integer
// arithmetic throughout; tests/deflate_ref.py restates the parse rule, the code construction and the header bit for bit.
//
// Stream.  A payload is cut into blocks of BLOCK = 16384 bytes that are coded independently: no match reaches before its
//   block's first byte (distances stay below 16384), ONE workgroup of 1024 threads codes one block, and one launch
//   codes every block of every payload.  A block becomes one DEFLATE block, stored (5 + n bytes) or dynamic, dynamic
//   only when it has strictly fewer bytes, decided from the exact bit count before a bit is written.  Every block but a
//   payload's last is followed by an empty stored block (zlib's sync flush), so blocks start on byte boundaries and are
//   concatenated as bytes: its header bits 000 lie in the zero bits that pad the block to a byte when at least three are
//   left (00 00 FF FF follows, 4 bytes), else in a byte of their own (00 00 00 FF FF).  The last block carries BFINAL.
//   Hence a stream has at most n + 10 per block bytes: acimg_deflate_bound(n) = n + 10 ceil(n / BLOCK) + 5.
// Why 16384 and not 32768: the parse keeps the block (1 byte), the match distance and the match length (2 bytes each, a
//   length of 258 does not fit one) of every position in LDS, because the greedy walk is a chain of dependent reads.
//   At 32768 these are 160 KiB, the whole LDS of a CU, with nothing left for the hash table, the output and the code
//   tables.  At 16384: block 16 KiB + distances 32 + lengths 32 + hash heads (2^13 int32) 32 + output words 16 + token
//   flags 2 + histograms, lengths, codes and the code builder's scratch 10 = 140 KiB (143304 bytes) of the CU's 160,
//   nothing aliased.  One workgroup per CU; 68 VGPRs, no scratch.
// Stages of deflate_block_kernel (a __syncthreads between any two):
//   1 match candidates.  hash(p) = (b[p] | b[p+1] << 8 | b[p+2] << 16) * 0x9E3779B1 >> 19 indexes 2^13 heads that hold the
//     latest position + 1.  Sub-steps of CHUNK = 256 positions: the sub-step's threads READ their head, a barrier, then
//     they insert with atomicMax.  So candidate A of p is the largest q of equal hash BEFORE p's sub-step: a function of
//     the input alone, whatever the lanes' timing.  Candidate B is p - 1 (runs, which A cannot see inside a sub-step).
//   2 match lengths, a thread per position: common leading bytes with each candidate, at most min(258, n - p); B wins
//     a tie; below 3 there is no match.
//   3 the greedy walk next = p + max(1, len[p]): ONE LANE walks the block's lengths in LDS and flags the token starts
//     (at most 16384 dependent LDS reads; bench_deflate.py times it - DESIGN section 8).
//   4 histograms of the tokens (LDS integer atomics: sums commute), literal/length with the end-of-block symbol, distance.
//   5 huffman_lengths for literal/length (286, limit 15) and distance (30, limit 15); a block without a match sends the
//     one distance code length 1 for symbol 0 (RFC 1951 3.2.7).  HLIT / HDIST drop trailing zero lengths.  The code lengths
//     are sent one symbol 0..15 each - the run symbols 16, 17, 18 are not used (cost: DESIGN section 8) - so the
//     code-length alphabet's histogram (19, limit 7) is that of the lengths themselves.  Canonical codes, bit-reversed.
//   6 exact bit count -> stored or dynamic.
//   7 bits: header fields, then the code lengths, then the tokens sub-step by sub-step: a workgroup scan of the
//     tokens' bit lengths (at most 48: 15 + 5 + 15 + 13) gives each its bit offset, and it ORs its bits into the output words
//     in LDS with atomicOr (OR commutes: deterministic).  The bytes then leave for the block's slot of the workspace.
// Then deflate_offsets_kernel (one workgroup) prefixes the blocks' byte counts over ALL payloads and forms each payload's
// stream length, and deflate_pack_kernel copies the blocks densely: only compressed bytes cross to the host.
// huffman_lengths (one function for the three alphabets, also launched alone as acimg_huffman_lengths): symbols with
//   freq <= 0 get 0; one used symbol gets 1.  Else every thread ranks symbols by (freq, symbol); one thread runs the
//   two-queue Huffman merge over the sorted leaves (of two equal weights the leaf is taken first) and the depths; depths
//   above the limit are set to it, and the Kraft excess E (units of 2^-limit) is repaired as zlib does, E times:
//   count[b] -= 1, count[b + 1] += 2, count[limit] -= 1 for the deepest level b < limit that holds a leaf, one unit each.
//   The counts are then dealt out in sorted order, the longest lengths to the least frequent symbols.
// No floating point; every loop is bounded by a constant above; nothing is read or written outside the stated extents.
#include <vector>

#include "common.hpp"

namespace acimg {

constexpr int DF_BLOCK = ACIMG_DEFLATE_BLOCK;
constexpr int DF_THREADS = 1024;
constexpr int DF_CHUNK = 256;
constexpr int DF_HASH_BITS = 13;
constexpr int DF_MIN_MATCH = 3, DF_MAX_MATCH = 258;
constexpr int DF_MAXSYM = 288;                      // symbols of one alphabet at most (acimg_huffman_lengths: nsym <= 288)
constexpr int DF_OUT_WORDS = DF_BLOCK / 4 + 4;      // a dynamic block has fewer than n + 5 bytes
constexpr int DF_SLOT = DF_BLOCK + 16;              // a block's bytes and its sync marker: at most n + 10
static_assert(DF_BLOCK % DF_CHUNK == 0 && DF_BLOCK <= 32768 && DF_BLOCK % 32 == 0, "block size");

__constant__ uint8_t c_cl_order[19] = {16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15};

struct DeflateBlockDesc {   // built on the host by acimg_deflate
    long in_off;            // the block's first byte in `in`
    int n;                  // its bytes, 1..BLOCK
    int payload;            // which payload it belongs to
    int first;              // that payload's first block
    int final;              // 1 for the payload's last block
};

struct HuffScratch {
    long long w[2 * DF_MAXSYM];
    uint16_t order[DF_MAXSYM], parent[2 * DF_MAXSYM], depth[2 * DF_MAXSYM];
    int count[16], next_code[16], used;
};

// Code lengths of one alphabet; called by EVERY thread of the workgroup.  freq, len: LDS, nsym <= DF_MAXSYM entries;
// 2^limit >= nsym, limit <= 15.  On return s.used is the number of symbols with freq > 0.
__device__ void huffman_lengths(const int* freq, int nsym, int limit, uint8_t* len, HuffScratch& s) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) s.used = 0;
    __syncthreads();
    for (int i = tid; i < nsym; i += nt) {
        len[i] = 0;
        const int f = freq[i];
        if (f > 0) {
            int r = 0;
            for (int j = 0; j < nsym; ++j) {
                const int g = freq[j];
                r += (g > 0 && (g < f || (g == f && j < i))) ? 1 : 0;
            }
            s.order[r] = (uint16_t)i;
            atomicAdd(&s.used, 1);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int used = s.used;
        if (used == 1) len[s.order[0]] = 1;
        if (used >= 2) {
            for (int k = 0; k < used; ++k) s.w[k] = freq[s.order[k]];
            int i = 0, j = used;
            for (int nxt = used; nxt < 2 * used - 1; ++nxt) {   // leaves i.., merged nodes j..nxt-1, both ascending
                long long sum = 0;
                for (int t = 0; t < 2; ++t) {
                    int pick;
                    if (i < used && (j >= nxt || s.w[i] <= s.w[j])) pick = i++;
                    else pick = j++;
                    sum += s.w[pick];
                    s.parent[pick] = (uint16_t)nxt;
                }
                s.w[nxt] = sum;
            }
            s.depth[2 * used - 2] = 0;
            for (int k = 2 * used - 3; k >= 0; --k) s.depth[k] = (uint16_t)(s.depth[s.parent[k]] + 1);
            for (int b = 0; b < 16; ++b) s.count[b] = 0;
            for (int k = 0; k < used; ++k) s.count[min((int)s.depth[k], limit)] += 1;
            int excess = -(1 << limit);
            for (int b = 1; b <= limit; ++b) excess += s.count[b] << (limit - b);
            for (int it = 0; it < DF_MAXSYM && excess > 0; ++it, --excess) {
                int b = limit - 1;
                while (b > 0 && s.count[b] == 0) --b;
                if (b == 0 || s.count[limit] == 0) break;   // cannot happen while 2^limit >= nsym; keeps the loop honest
                s.count[b] -= 1;
                s.count[b + 1] += 2;
                s.count[limit] -= 1;
            }
            int k = 0;
            for (int b = limit; b >= 1; --b)
                for (int c = 0; c < s.count[b] && k < used; ++c) len[s.order[k++]] = (uint8_t)b;
        }
    }
    __syncthreads();
}

// RFC 1951 3.2.2 codes of the lengths, bit-reversed (Huffman codes go out most significant bit first); every thread calls
__device__ void canonical_codes(const uint8_t* len, int nsym, uint16_t* code, HuffScratch& s) {
    const int tid = threadIdx.x, nt = blockDim.x;
    if (tid < 16) s.count[tid] = 0;
    __syncthreads();
    for (int i = tid; i < nsym; i += nt)
        if (len[i]) atomicAdd(&s.count[len[i]], 1);
    __syncthreads();
    if (tid == 0) {
        int c = 0;
        s.count[0] = 0;
        for (int b = 1; b < 16; ++b) {
            c = (c + s.count[b - 1]) << 1;
            s.next_code[b] = c;
        }
    }
    __syncthreads();
    for (int i = tid; i < nsym; i += nt) {
        const int l = len[i];
        uint32_t c = 0;
        if (l) {
            int k = 0;
            for (int j = 0; j < i; ++j) k += len[j] == l ? 1 : 0;
            c = __brev((uint32_t)(s.next_code[l] + k)) >> (32 - l);
        }
        code[i] = (uint16_t)c;
    }
    __syncthreads();
}

// match length 3..258 -> code above symbol 257, extra bits, their value
__device__ __forceinline__ void length_code(int l, int& code, int& k, int& x) {
    const int v = l - 3;
    if (l == DF_MAX_MATCH) {
        code = 28, k = 0, x = 0;
    } else if (v < 8) {
        code = v, k = 0, x = 0;
    } else {
        k = 29 - __clz(v);
        code = 4 * k + 4 + ((v >> k) & 3);
        x = v & ((1 << k) - 1);
    }
}
// distance 1..32768 -> code, extra bits, their value
__device__ __forceinline__ void dist_code(int d, int& code, int& k, int& x) {
    const int v = d - 1;
    if (v < 4) {
        code = v, k = 0, x = 0;
    } else {
        k = 30 - __clz(v);
        code = 2 * k + 2 + ((v >> k) & 1);
        x = v & ((1 << k) - 1);
    }
}
__device__ __forceinline__ int length_extra(int code) { return code < 8 || code == 28 ? 0 : (code - 4) >> 2; }
__device__ __forceinline__ int dist_extra(int code) { return code < 4 ? 0 : (code - 2) >> 1; }

// exclusive scan of v over the workgroup (blockDim.x a multiple of 64, <= 1024); total in every thread; every thread calls
__device__ __forceinline__ int block_scan_excl(int v, int& total, int* part /* 16 ints */) {
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    int inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int up = __shfl_up(inc, o, 64);
        if (lane >= o) inc += up;
    }
    __syncthreads();
    if (lane == 63) part[wid] = inc;
    __syncthreads();
    int base = 0, tot = 0;
    for (int i = 0; i < nw; ++i) {
        const int t = part[i];
        base += i < wid ? t : 0;
        tot += t;
    }
    total = tot;
    return base + inc - v;
}

// OR the low nb <= 48 bits of val into the bit string `out` (least significant bit first) at bit `off`
__device__ __forceinline__ void put_bits(uint32_t* out, int off, uint64_t val, int nb) {
    if (nb == 0) return;
    const int w = off >> 5, sh = off & 31;
    if (w < DF_OUT_WORDS) atomicOr(&out[w], (uint32_t)(val << sh));
    if (sh + nb > 32 && w + 1 < DF_OUT_WORDS) atomicOr(&out[w + 1], (uint32_t)(val >> (32 - sh)));
    if (sh + nb > 64 && w + 2 < DF_OUT_WORDS) atomicOr(&out[w + 2], (uint32_t)(val >> (64 - sh)));
}

__global__ __launch_bounds__(DF_THREADS) void deflate_block_kernel(const uint8_t* in, const DeflateBlockDesc* desc, uint8_t* slots,
                                                                   int32_t* sizes) {
    __shared__ __attribute__((aligned(16))) uint8_t s_data[DF_BLOCK];
    __shared__ uint16_t s_dist[DF_BLOCK];   // stage 1: candidate A + 1 (0: none); from stage 2: the match distance
    __shared__ uint16_t s_len[DF_BLOCK];    // match length, 0: none
    __shared__ int s_head[1 << DF_HASH_BITS];
    __shared__ uint32_t s_out[DF_OUT_WORDS];
    __shared__ uint32_t s_flag[DF_BLOCK / 32];   // bit p: a token starts at p
    __shared__ int s_hist_ll[DF_MAXSYM], s_hist_d[32], s_hist_cl[32];
    __shared__ uint8_t s_len_ll[DF_MAXSYM], s_len_d[32], s_len_cl[32];
    __shared__ uint16_t s_code_ll[DF_MAXSYM], s_code_d[32], s_code_cl[32];
    __shared__ HuffScratch s_h;
    __shared__ int s_part[16];
    __shared__ int s_bits, s_hlit, s_hdist, s_hclen;

    const int tid = threadIdx.x;
    const DeflateBlockDesc d = desc[blockIdx.x];
    const int n = min(max(d.n, 1), DF_BLOCK);
    const uint8_t* src = in + d.in_off;
    uint8_t* const slot = slots + (size_t)blockIdx.x * DF_SLOT;

    for (int p = tid; p < n; p += DF_THREADS) {
        s_data[p] = src[p];
        s_dist[p] = 0;
    }
    for (int i = tid; i < (1 << DF_HASH_BITS); i += DF_THREADS) s_head[i] = 0;
    for (int i = tid; i < DF_BLOCK / 32; i += DF_THREADS) s_flag[i] = 0;
    for (int i = tid; i < DF_MAXSYM; i += DF_THREADS) s_hist_ll[i] = 0;
    if (tid < 32) s_hist_d[tid] = 0, s_hist_cl[tid] = 0, s_len_cl[tid] = 0, s_len_d[tid] = 0;
    if (tid == 0) s_bits = 0;
    __syncthreads();

    // 1 candidates: read the heads, barrier, insert
    for (int s = 0; s + 2 < n; s += DF_CHUNK) {
        const int p = s + tid;
        const bool on = tid < DF_CHUNK && p + 2 < n;
        uint32_t h = 0;
        if (on) {
            h = ((uint32_t)s_data[p] | ((uint32_t)s_data[p + 1] << 8) | ((uint32_t)s_data[p + 2] << 16)) * 0x9E3779B1u;
            h >>= 32 - DF_HASH_BITS;
            s_dist[p] = (uint16_t)s_head[h];
        }
        __syncthreads();
        if (on) atomicMax(&s_head[h], p + 1);
        __syncthreads();
    }

    // 2 match lengths
    for (int p = tid; p < n; p += DF_THREADS) {
        const int maxl = min(DF_MAX_MATCH, n - p);
        const int qa = (int)s_dist[p] - 1;
        int la = 0, lb = 0;
        if (qa >= 0)
            while (la < maxl && s_data[qa + la] == s_data[p + la]) ++la;
        if (p >= 1)
            while (lb < maxl && s_data[p - 1 + lb] == s_data[p + lb]) ++lb;
        int len = la, dist = p - qa;
        if (lb >= la) len = lb, dist = 1;
        if (len < DF_MIN_MATCH) len = 0, dist = 0;
        s_len[p] = (uint16_t)len;
        s_dist[p] = (uint16_t)dist;
    }
    __syncthreads();

    // 3 the greedy walk, one lane
    if (tid == 0) {
        int p = 0;
        for (int step = 0; step < DF_BLOCK && p < n; ++step) {
            s_flag[p >> 5] |= 1u << (p & 31);
            const int l = s_len[p];
            p += l ? l : 1;
        }
        s_hist_ll[256] = 1;
    }
    __syncthreads();

    // 4 histograms
    for (int p = tid; p < n; p += DF_THREADS) {
        if (!((s_flag[p >> 5] >> (p & 31)) & 1u)) continue;
        const int l = s_len[p];
        if (l == 0) {
            atomicAdd(&s_hist_ll[s_data[p]], 1);
        } else {
            int c, k, x;
            length_code(l, c, k, x);
            atomicAdd(&s_hist_ll[257 + c], 1);
            dist_code(s_dist[p], c, k, x);
            atomicAdd(&s_hist_d[c], 1);
        }
    }
    __syncthreads();

    // 5 codes
    huffman_lengths(s_hist_ll, 286, 15, s_len_ll, s_h);
    huffman_lengths(s_hist_d, 30, 15, s_len_d, s_h);
    if (tid == 0) {
        if (s_h.used == 0) s_len_d[0] = 1;
        int hl = 286, hd = 30;
        while (hl > 257 && s_len_ll[hl - 1] == 0) --hl;
        while (hd > 1 && s_len_d[hd - 1] == 0) --hd;
        s_hlit = hl;
        s_hdist = hd;
    }
    __syncthreads();
    const int hlit = s_hlit, hdist = s_hdist;
    for (int i = tid; i < hlit + hdist; i += DF_THREADS) atomicAdd(&s_hist_cl[i < hlit ? s_len_ll[i] : s_len_d[i - hlit]], 1);
    __syncthreads();
    huffman_lengths(s_hist_cl, 19, 7, s_len_cl, s_h);
    canonical_codes(s_len_ll, 286, s_code_ll, s_h);
    canonical_codes(s_len_d, 30, s_code_d, s_h);
    canonical_codes(s_len_cl, 19, s_code_cl, s_h);
    if (tid == 0) {
        int hc = 19;
        while (hc > 4 && s_len_cl[c_cl_order[hc - 1]] == 0) --hc;
        s_hclen = hc;
        atomicAdd(&s_bits, 17 + 3 * hc);
    }
    // 6 the exact bit count
    for (int i = tid; i < 286; i += DF_THREADS)
        atomicAdd(&s_bits, s_hist_ll[i] * ((int)s_len_ll[i] + (i >= 257 ? length_extra(i - 257) : 0)));
    if (tid < 30) atomicAdd(&s_bits, s_hist_d[tid] * ((int)s_len_d[tid] + dist_extra(tid)));
    if (tid < 19) atomicAdd(&s_bits, s_hist_cl[tid] * (int)s_len_cl[tid]);
    __syncthreads();
    const int bits = s_bits, hclen = s_hclen;
    const int dyn_bytes = (bits + 7) >> 3;
    const bool dynamic = dyn_bytes < n + 5;
    const int body = dynamic ? dyn_bytes : n + 5;
    const int marker = d.final ? 0 : (dynamic && dyn_bytes * 8 - bits >= 3 ? 4 : 5);

    if (!dynamic) {
        if (tid == 0) {
            slot[0] = d.final ? 1 : 0;
            slot[1] = (uint8_t)(n & 255);
            slot[2] = (uint8_t)(n >> 8);
            slot[3] = (uint8_t)(~n & 255);
            slot[4] = (uint8_t)((~n >> 8) & 255);
        }
        for (int i = tid; i < n; i += DF_THREADS) slot[5 + i] = s_data[i];
    } else {
        // 7 bits
        const int words = min((dyn_bytes + 3) / 4 + 2, DF_OUT_WORDS);
        for (int i = tid; i < words; i += DF_THREADS) s_out[i] = 0;
        __syncthreads();
        if (tid == 0) {   // BFINAL, BTYPE = 10, HLIT, HDIST, HCLEN
            const int head = (d.final ? 1 : 0) | (2 << 1) | ((hlit - 257) << 3) | ((hdist - 1) << 8) | ((hclen - 4) << 13);
            put_bits(s_out, 0, (uint64_t)head, 17);
        }
        if (tid < hclen) put_bits(s_out, 17 + 3 * tid, s_len_cl[c_cl_order[tid]], 3);
        int at = 17 + 3 * hclen, total;
        {   // hlit + hdist <= 316 code lengths: one sub-step
            int sym = 0, nb = 0;
            if (tid < hlit + hdist) {
                sym = tid < hlit ? s_len_ll[tid] : s_len_d[tid - hlit];
                nb = s_len_cl[sym];
            }
            const int off = block_scan_excl(nb, total, s_part);
            put_bits(s_out, at + off, s_code_cl[sym], nb);
            at += total;
        }
        for (int s = 0; s < n; s += DF_THREADS) {
            const int p = s + tid;
            uint64_t val = 0;
            int nb = 0;
            if (p < n && ((s_flag[p >> 5] >> (p & 31)) & 1u)) {
                const int l = s_len[p];
                if (l == 0) {
                    const int c = s_data[p];
                    val = s_code_ll[c];
                    nb = s_len_ll[c];
                } else {
                    int c, k, x;
                    length_code(l, c, k, x);
                    val = s_code_ll[257 + c];
                    nb = s_len_ll[257 + c];
                    val |= (uint64_t)x << nb;
                    nb += k;
                    dist_code(s_dist[p], c, k, x);
                    val |= (uint64_t)s_code_d[c] << nb;
                    nb += s_len_d[c];
                    val |= (uint64_t)x << nb;
                    nb += k;
                }
            }
            const int off = block_scan_excl(nb, total, s_part);
            put_bits(s_out, at + off, val, nb);
            at += total;
        }
        if (tid == 0) put_bits(s_out, at, s_code_ll[256], s_len_ll[256]);
        __syncthreads();
        for (int i = tid; i < dyn_bytes; i += DF_THREADS) slot[i] = (uint8_t)(s_out[i >> 2] >> ((i & 3) * 8));
    }
    if (tid < marker) slot[body + tid] = tid >= marker - 2 ? 0xFF : 0x00;
    if (tid == 0) sizes[blockIdx.x] = body + marker;
}

// one workgroup: the blocks' offsets in the dense output (all payloads, in order) and every payload's stream length
__global__ __launch_bounds__(1024) void deflate_offsets_kernel(const DeflateBlockDesc* desc, const int32_t* sizes, long* offs,
                                                               long nblocks, long* out_sizes) {
    __shared__ long part[1024];
    const int tid = threadIdx.x;
    const long chunk = (nblocks + 1023) / 1024;
    const long a = tid * chunk < nblocks ? tid * chunk : nblocks;
    const long e = a + chunk < nblocks ? a + chunk : nblocks;
    long sum = 0;
    for (long b = a; b < e; ++b) sum += sizes[b];
    part[tid] = sum;
    __syncthreads();
    long at = 0;
    for (int t = 0; t < tid; ++t) at += part[t];
    for (long b = a; b < e; ++b) {
        offs[b] = at;
        at += sizes[b];
    }
    __syncthreads();
    for (long b = tid; b < nblocks; b += 1024)
        if (desc[b].final) out_sizes[desc[b].payload] = offs[b] + sizes[b] - offs[desc[b].first];
}

__global__ __launch_bounds__(256) void deflate_pack_kernel(const uint8_t* slots, const int32_t* sizes, const long* offs,
                                                           uint8_t* out) {
    const uint8_t* src = slots + (size_t)blockIdx.x * DF_SLOT;
    uint8_t* dst = out + offs[blockIdx.x];
    const int len = min(max(sizes[blockIdx.x], 0), DF_SLOT);
    for (int i = threadIdx.x; i < len; i += 256) dst[i] = src[i];
}

// one workgroup per histogram
__global__ __launch_bounds__(256) void huffman_lengths_kernel(const int32_t* freq, int nsym, int limit, uint8_t* lengths) {
    __shared__ int s_freq[DF_MAXSYM];
    __shared__ uint8_t s_len[DF_MAXSYM];
    __shared__ HuffScratch s_h;
    const size_t row = (size_t)blockIdx.x * nsym;
    for (int i = threadIdx.x; i < nsym; i += 256) s_freq[i] = freq[row + i];
    __syncthreads();
    huffman_lengths(s_freq, nsym, limit, s_len, s_h);
    for (int i = threadIdx.x; i < nsym; i += 256) lengths[row + i] = s_len[i];
}

inline size_t df_align16(size_t v) { return (v + 15) & ~(size_t)15; }
inline long df_blocks(long n) { return (n + DF_BLOCK - 1) / DF_BLOCK; }
inline size_t df_workspace(long blocks) {
    return df_align16((size_t)blocks * sizeof(DeflateBlockDesc)) + df_align16((size_t)blocks * sizeof(int32_t)) +
           df_align16((size_t)blocks * sizeof(long)) + (size_t)blocks * DF_SLOT;
}
constexpr long DF_MAX_BYTES = 1L << 40;

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_deflate_bound(long n) {
    if (n < 0 || n > DF_MAX_BYTES) return 0;
    return (size_t)n + 10 * (size_t)df_blocks(n) + 5;
}

size_t acimg_deflate_workspace(long total_bytes, int count) {
    if (total_bytes < 1 || total_bytes > DF_MAX_BYTES || count < 1 || count > total_bytes) return 0;
    return df_workspace(total_bytes / DF_BLOCK + count);   // every payload ends with at most one short block
}

int acimg_deflate(const uint8_t* in, const long* lengths, int count, uint8_t* out, size_t out_bytes, long* out_sizes, void* ws,
                  size_t ws_bytes, void* stream) {
    if (!in || !lengths || !out || !out_sizes || !ws) return fail(ACIMG_EINVAL, "deflate: null argument");
    if (count < 1) return fail(ACIMG_EINVAL, "deflate: count = %d must be positive", count);
    long total = 0, blocks = 0;
    size_t need_out = 0;
    for (int i = 0; i < count; ++i) {
        if (lengths[i] < 1 || lengths[i] > DF_MAX_BYTES - total)
            return fail(ACIMG_EINVAL, "deflate: payload %d has %ld bytes (an empty payload is the caller's 5-byte stored block)", i,
                        lengths[i]);
        total += lengths[i];
        blocks += df_blocks(lengths[i]);
        need_out += acimg_deflate_bound(lengths[i]);
    }
    if (blocks > (long)INT32_MAX) return fail(ACIMG_EINVAL, "deflate: %ld blocks exceed the grid", blocks);
    if (out_bytes < need_out) return fail(ACIMG_EINVAL, "deflate: out_bytes = %zu < the payloads' bounds %zu", out_bytes, need_out);
    if (!aligned16(ws)) return fail(ACIMG_EINVAL, "deflate: ws must be 16-byte aligned");
    const size_t need = acimg_deflate_workspace(total, count);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "deflate: workspace %zu < %zu bytes", ws_bytes, need);
    std::vector<DeflateBlockDesc> table((size_t)blocks);
    long at = 0, b = 0;
    for (int i = 0; i < count; ++i) {
        const long first = b;
        for (long o = 0; o < lengths[i]; o += DF_BLOCK, ++b) {
            const long left = lengths[i] - o;
            table[b] = {at + o, (int)(left < DF_BLOCK ? left : DF_BLOCK), i, (int)first, left <= DF_BLOCK ? 1 : 0};
        }
        at += lengths[i];
    }
    DeflateBlockDesc* desc = (DeflateBlockDesc*)ws;
    uint8_t* p = (uint8_t*)ws + df_align16((size_t)blocks * sizeof(DeflateBlockDesc));
    int32_t* sizes = (int32_t*)p;
    p += df_align16((size_t)blocks * sizeof(int32_t));
    long* offs = (long*)p;
    p += df_align16((size_t)blocks * sizeof(long));
    uint8_t* slots = p;
    hipStream_t s = (hipStream_t)stream;
    // the table is host memory of this call: it has reached the device before the call returns
    hipError_t e = hipMemcpyAsync(desc, table.data(), (size_t)blocks * sizeof(DeflateBlockDesc), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "deflate (block table): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(deflate_block_kernel, dim3((unsigned)blocks), dim3(DF_THREADS), 0, s, in, (const DeflateBlockDesc*)desc, slots,
                       sizes);
    int rc = check_launch("deflate (blocks)");
    if (rc) return rc;
    hipLaunchKernelGGL(deflate_offsets_kernel, dim3(1), dim3(1024), 0, s, (const DeflateBlockDesc*)desc, (const int32_t*)sizes, offs,
                       blocks, out_sizes);
    rc = check_launch("deflate (offsets)");
    if (rc) return rc;
    hipLaunchKernelGGL(deflate_pack_kernel, dim3((unsigned)blocks), dim3(256), 0, s, (const uint8_t*)slots, (const int32_t*)sizes,
                       (const long*)offs, out);
    return check_launch("deflate (pack)");
}

int acimg_huffman_lengths(const int32_t* freq, int n, int nsym, int limit, uint8_t* lengths, void* stream) {
    if (!freq || !lengths) return fail(ACIMG_EINVAL, "huffman_lengths: null argument");
    if (n < 1) return fail(ACIMG_EINVAL, "huffman_lengths: n = %d must be positive", n);
    if (nsym < 1 || nsym > DF_MAXSYM) return fail(ACIMG_EINVAL, "huffman_lengths: nsym = %d outside 1..%d", nsym, DF_MAXSYM);
    if (limit < 1 || limit > 15 || (1 << limit) < nsym)
        return fail(ACIMG_EINVAL, "huffman_lengths: a limit of %d bits outside 1..15 or too short for %d symbols", limit, nsym);
    hipLaunchKernelGGL(huffman_lengths_kernel, dim3((unsigned)n), dim3(256), 0, (hipStream_t)stream, freq, nsym, limit, lengths);
    return check_launch("huffman_lengths");
}

}  // extern "C"
