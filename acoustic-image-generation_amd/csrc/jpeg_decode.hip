// Baseline and progressive JPEG (ITU-T T.81, DCT, Huffman, 8 bit; SOF0, SOF1, SOF2) to B, G, R pixels on the GPU: the decoder behind
// `python -m acimg.convert_boxes` (the `cv2.imread` of convert_data2.py:157), the mirror of jpeg.hip.  Integer arithmetic
// throughout, so that tests/jpeg_decode_ref.py restates every stage bit for bit on any machine and the pixels equal
// libjpeg's (`jpeg_idct_islow`, fancy upsampling, 16-bit fixed-point colour) - DESIGN section 8.
//
// The images of one launch share H, W, the number of components (1 or 3) and the luma sampling hs x vs (1x1, 2x1 or 2x2
// over 1x1 chroma); an MCU is 8 hs x 8 vs pixels and holds B = hs vs + 2 blocks (Y in raster order, Cb, Cr), B = 1 for one
// component.  Everything else is per image: where its entropy-coded segment lies, its restart interval, its three quant
// tables and its six Huffman tables (DC and AC of each component).
//
// acimg_jpeg_decode_entropy: one workgroup (one wave) per image with the image's Huffman tables in LDS, ONE LANE per
//   restart interval (a file without DRI is one interval: the parallelism is the batch).  The host has found the intervals
//   (a byte search for FF D0..D7), so a lane reads the bytes of its interval only, un-stuffs FF 00 as it goes, starts with
//   DC predictors of 0 and writes the blocks of its MCUs, de-zig-zagged, into the image's coefficient slot.
//   The input is a file from disk, so nothing in it is trusted: every range the descriptors give is clamped to the data,
//   an interval's reads end at its end (zeros follow, and using one of them is an error), every block index comes from
//   the loop over the interval's own MCUs, a coefficient index is checked against 63 before the store, and every loop
//   runs a number of times fixed by the geometry.  A lane that meets an error writes zeros for the rest of its interval;
//   the image's status is the error of its first bad interval.  Other images never see it.
// acimg_jpeg_decode_progressive: the same coefficient slot from a progressive file (SOF2; T.81 Annex G: spectral selection
//   and successive approximation over several scans).  One workgroup (one wave) per image again; the unit of work is one
//   (scan, restart interval) pair, ONE LANE each.  Scans are separate byte-aligned bit streams and depend on each other only
//   where they touch the same coefficients of the same component, so the host gives every scan a LEVEL (0, or 1 + the
//   highest level of an earlier scan that shares a component and overlaps its band); the kernel zeroes the slot, then runs
//   the levels in order with a fence and a workgroup barrier between them, all items of a level side by side.  A scan of
//   one component walks that component's OWN block grid, not the MCU-padded one.  The scan records are checked field by
//   field into LDS before anything of them is used; a record that fails is one item that reports DESCRIPTOR and writes
//   nothing.  An item that meets an error stops writing there; the status is that of the first bad item in (scan,
//   interval) order, and later levels still run on what is there.
//   The Huffman tables are read from GLOBAL memory, not staged in LDS: a legal level may hold one scan per coefficient and
//   component (189 scans with a table each, 171 KB) which no LDS holds, so staging would need a second path for the levels
//   that do not fit; the tables of a level are a few KB that every lane reads again and again, so they stay in the CU's
//   vector cache, and the wave is bound by its serial bit walk, not by these loads.
// acimg_jpeg_decode_idct: dequantise + libjpeg's jpeg_idct_islow (CONST_BITS 13, PASS1_BITS 2) in wrapping 32-bit
//   integers, eight threads per block: a column each, then a row each; +128, clamp, eight bytes per thread into the
//   component's plane (padded to the MCU grid).
// acimg_jpeg_decode_colour: one thread per pixel: libjpeg's fancy (triangle) chroma upsampling on the component's true
//   size, then Y Cb Cr -> B G R in 16-bit fixed point.
// No atomics, no floating point; every output byte is written by exactly one thread: bit-identical from run to run.
#include "common.hpp"

namespace acimg {

constexpr int JPEG_DEC_MAX_DIM = 65535;
constexpr int ST_OK = 0, ST_BAD_CODE = ACIMG_JPEG_STATUS_BAD_CODE, ST_RUN = ACIMG_JPEG_STATUS_RUN,
              ST_EARLY_END = ACIMG_JPEG_STATUS_EARLY_END, ST_DESCRIPTOR = ACIMG_JPEG_STATUS_DESCRIPTOR;

// zig-zag position -> natural (row-major) index
__constant__ uint8_t c_dezigzag[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                       41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                       30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// one derived Huffman table as the host lays it out (acimg/jpeg.py: derive_huffman)
struct HuffDec {
    uint16_t look[256];    // the next 8 bits -> (length << 8) | symbol of a code of at most 8 bits, else 0
    int32_t maxcode[17];   // [l], l = 1..16: the largest code of l bits, -1 if there is none
    int32_t valoff[17];    // [l]: index of the first symbol of l bits minus the smallest code of l bits
    uint8_t vals[256];     // HUFFVAL
};
static_assert(sizeof(HuffDec) == ACIMG_JPEG_HUFF_BYTES, "the device layout of a Huffman table");
constexpr int HUFFDEC_WORDS = sizeof(HuffDec) / 4;

struct DecGeometry {
    int blocks;            // per MCU
    long mcu_w, mcu_h, mcus;
};
inline bool jpeg_dec_args_ok(int H, int W, int comps, int hs, int vs) {
    if (H < 1 || H > JPEG_DEC_MAX_DIM || W < 1 || W > JPEG_DEC_MAX_DIM) return false;
    if (comps == 1) return hs == 1 && vs == 1;
    return comps == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
}
inline DecGeometry jpeg_dec_geometry(int H, int W, int comps, int hs, int vs) {
    DecGeometry g;
    g.blocks = comps == 1 ? 1 : hs * vs + 2;
    g.mcu_w = (W + 8 * hs - 1) / (8 * hs);
    g.mcu_h = (H + 8 * vs - 1) / (8 * vs);
    g.mcus = g.mcu_w * g.mcu_h;
    return g;
}

// ---- entropy decoding -----------------------------------------------------------------------------------------------
struct BitSource {   // MSB-first bits of [p, end) with FF 00 un-stuffed; any other FF ends the data; zeros follow the data
    const uint8_t* p;
    const uint8_t* end;
    uint64_t acc;
    int n;      // bits in acc
    int real;   // of these, bits that came from the data; negative once more bits were used than the data holds
    __device__ __forceinline__ void fill() {   // n >= 57 afterwards
        while (n <= 56) {
            uint32_t byte = 0;
            if (p < end) {
                const uint32_t b = *p;
                if (b != 0xFFu) {
                    byte = b;
                    ++p;
                    real += 8;
                } else if (p + 1 < end && p[1] == 0) {
                    byte = 0xFFu;
                    p += 2;
                    real += 8;
                } else {
                    end = p;   // a marker, or an FF that ends the data
                }
            }
            acc = (acc << 8) | byte;
            n += 8;
        }
    }
    __device__ __forceinline__ uint32_t peek(int k) const { return (uint32_t)(acc >> (n - k)) & ((1u << k) - 1u); }   // 1 <= k <= 16
    __device__ __forceinline__ void skip(int k) {
        n -= k;
        real -= k;
    }
    __device__ __forceinline__ int receive_extend(int s) {   // 0 <= s <= 15
        if (s == 0) return 0;
        const int v = (int)peek(s);
        skip(s);
        return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
    }
};

// the next symbol of table t, or -1 where no code of up to 16 bits matches
__device__ __forceinline__ int huff_symbol(BitSource& s, const HuffDec& t) {
    const uint32_t e = t.look[s.peek(8)];
    if (e) {
        s.skip((int)(e >> 8));
        return (int)(e & 255u);
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)s.peek(l);
        if (code <= t.maxcode[l]) {
            s.skip(l);
            return t.vals[(t.valoff[l] + code) & 255];
        }
    }
    return -1;
}

// desc int64 [n][4]: first and end byte of the image's entropy-coded segment in `data`, MCUs per restart interval (0: the
// whole image is one), index of its first interval in `intervals`; intervals int32 [..][2]: first and end byte of an
// interval, relative to the segment.
__global__ __launch_bounds__(64) void jpeg_entropy_kernel(const uint8_t* data, long data_bytes, const int64_t* desc,
                                                          const int32_t* intervals, long total_intervals, const uint8_t* huff,
                                                          int comps, int luma_blocks, int blocks, long mcus, int16_t* coef,
                                                          int32_t* status) {
    __shared__ HuffDec tab[6];
    __shared__ long long first_error[64];
    const int lane = threadIdx.x;
    const long img = blockIdx.x;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(huff + (size_t)img * 6 * sizeof(HuffDec));
        uint32_t* dst = reinterpret_cast<uint32_t*>(tab);
        for (int i = lane; i < 2 * comps * HUFFDEC_WORDS; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    long seg_begin = desc[img * 4 + 0], seg_end = desc[img * 4 + 1];
    long restart = desc[img * 4 + 2];
    const long first = desc[img * 4 + 3];
    seg_begin = seg_begin < 0 ? 0 : (seg_begin > data_bytes ? data_bytes : seg_begin);
    seg_end = seg_end < seg_begin ? seg_begin : (seg_end > data_bytes ? data_bytes : seg_end);
    const long seg_len = seg_end - seg_begin;
    if (restart < 1 || restart > mcus) restart = mcus;
    const long count = (mcus + restart - 1) / restart;
    const bool desc_ok = first >= 0 && first <= total_intervals && count <= total_intervals - first;
    int16_t* const slot = coef + (size_t)img * mcus * blocks * 64;
    long long err = 0x7FFFFFFFFFFFFFFFll;   // (interval << 3) | code of this lane's first error
    for (long j = lane; j < count; j += 64) {
        const long m0 = j * restart, m1 = m0 + restart < mcus ? m0 + restart : mcus;
        int code = desc_ok ? ST_OK : ST_DESCRIPTOR;
        BitSource s = {data, data, 0, 0, 0};
        if (desc_ok) {
            long a = intervals[(first + j) * 2 + 0], e = intervals[(first + j) * 2 + 1];
            a = a < 0 ? 0 : (a > seg_len ? seg_len : a);
            e = e < a ? a : (e > seg_len ? seg_len : e);
            s.p = data + seg_begin + a;
            s.end = data + seg_begin + e;
        }
        int pred[3] = {0, 0, 0};
        for (long m = m0; m < m1; ++m) {
            for (int b = 0; b < blocks; ++b) {
                uint4* const blk4 = reinterpret_cast<uint4*>(slot + (m * blocks + b) * 64);
#pragma unroll
                for (int i = 0; i < 8; ++i) blk4[i] = make_uint4(0, 0, 0, 0);
                if (code != ST_OK) continue;   // after an error the rest of the interval is zeros
                int16_t* const blk = reinterpret_cast<int16_t*>(blk4);
                const int c = b < luma_blocks ? 0 : b - luma_blocks + 1;
                s.fill();
                int sym = huff_symbol(s, tab[2 * c]);
                if (sym < 0 || sym > 15) {
                    code = ST_BAD_CODE;
                    continue;
                }
                const int dc = pred[c] + s.receive_extend(sym);
                if (s.real < 0) {
                    code = ST_EARLY_END;
                    continue;
                }
                pred[c] = dc;
                blk[0] = (int16_t)dc;
                const HuffDec& ac = tab[2 * c + 1];
                int k = 1;
                for (int step = 0; step < 63 && k < 64; ++step) {   // a symbol advances k by at least one
                    s.fill();
                    sym = huff_symbol(s, ac);
                    if (sym < 0) {
                        code = ST_BAD_CODE;
                        break;
                    }
                    const int r = sym >> 4, size = sym & 15;
                    if (size) {
                        k += r;
                        if (k > 63) {
                            code = ST_RUN;
                            break;
                        }
                        blk[c_dezigzag[k]] = (int16_t)s.receive_extend(size);
                        ++k;
                    } else if (r == 15) {
                        k += 16;
                    } else {
                        k = 64;   // EOB
                    }
                    if (s.real < 0) {
                        code = ST_EARLY_END;
                        break;
                    }
                }
                if (code != ST_OK) {   // the block that met the error is zeros too
#pragma unroll
                    for (int i = 0; i < 8; ++i) blk4[i] = make_uint4(0, 0, 0, 0);
                }
            }
        }
        if (code != ST_OK && err == 0x7FFFFFFFFFFFFFFFll) err = ((long long)j << 3) | code;
    }
    first_error[lane] = err;
    __syncthreads();
    if (lane == 0) {
        long long least = first_error[0];
        for (int i = 1; i < 64; ++i) least = first_error[i] < least ? first_error[i] : least;
        status[img] = least == 0x7FFFFFFFFFFFFFFFll ? ST_OK : (int)(least & 7);
    }
}

// ---- progressive entropy decoding (T.81 Annex G) ----------------------------------------------------------------------
// One validated scan record in LDS.  `code` is ST_OK or ST_DESCRIPTOR; a record that fails a check has ONE item, which
// reports the error and touches nothing.
struct ProgScan {
    int code, level, mask, ncomp;   // components of the scan as a bit mask, and how many
    int ss, se, refine, al;
    int tab[3];                     // per component: index into the table pool (DC first: DC table; AC scans: AC table)
    int comp;                       // the component of a one-component scan
    int units, restart, count;      // MCUs (interleaved) or blocks of the component's own grid; per interval; intervals
    int bw;                         // blocks per row of the component's own grid (one-component scans)
    int seg_a, seg_e;               // the scan's bytes relative to the image's data, clamped
    int first;                      // index of its first interval in `intervals`
};
constexpr int PROG_MAX_SCANS = ACIMG_JPEG_PROG_MAX_SCANS;
constexpr int PROG_FIELDS = ACIMG_JPEG_PROG_SCAN_FIELDS;

struct ProgGeometry {
    int comps, hs, vs, luma_blocks, blocks;
    int mcu_w, mcus;
    int bw[3], bh[3];   // each component's own block grid: ceil(ceil(W h / hmax) / 8) x ceil(ceil(H v / vmax) / 8)
};

__device__ __forceinline__ int take_bit(BitSource& s) {
    s.fill();
    const int v = (int)s.peek(1);
    s.skip(1);
    return v;
}

// the correction bit of one coefficient that is already nonzero (G.1.2.3): 16-bit arithmetic that wraps, as a JCOEF does
__device__ __forceinline__ void refine_nonzero(BitSource& s, int16_t* at, int p1) {
    const int bit = take_bit(s);
    if (s.real < 0) return;   // the caller reports it; nothing is written from bits the data does not hold
    const int v = *at;
    if (bit && (v & p1) == 0) *at = (int16_t)(v >= 0 ? v + p1 : v - p1);
}

// One (scan, restart interval) pair: the blocks [u0, u1) of the scan, in the image's coefficient slot.  Returns its status.
__device__ int prog_item(const ProgScan& sc, const ProgGeometry& g, long j, const uint8_t* data, long img_a,
                         const int32_t* intervals, const HuffDec* pool, int16_t* slot) {
    if (sc.code != ST_OK) return sc.code;
    long a = intervals[((long)sc.first + j) * 2 + 0], e = intervals[((long)sc.first + j) * 2 + 1];
    const long seg_len = (long)sc.seg_e - sc.seg_a;
    a = a < 0 ? 0 : (a > seg_len ? seg_len : a);
    e = e < a ? a : (e > seg_len ? seg_len : e);
    BitSource s = {data + img_a + sc.seg_a + a, data + img_a + sc.seg_a + e, 0, 0, 0};
    const long u0 = j * (long)sc.restart;
    const long u1 = u0 + sc.restart < sc.units ? u0 + sc.restart : sc.units;
    const int p1 = 1 << sc.al;
    int pred[3] = {0, 0, 0};
    int eobrun = 0;
    for (long u = u0; u < u1; ++u) {
        if (sc.ss == 0) {   // DC: every block of the scan's components in this MCU, or the one block of a one-component scan
            const int b_hi = sc.ncomp > 1 ? g.blocks : 1;
            for (int bi = 0; bi < b_hi; ++bi) {
                int c, b;
                long m;
                if (sc.ncomp > 1) {
                    b = bi;
                    m = u;
                    c = b < g.luma_blocks ? 0 : b - g.luma_blocks + 1;
                    if (!((sc.mask >> c) & 1)) continue;
                } else {
                    c = sc.comp;
                    const int br = (int)(u / sc.bw), bc = (int)(u - (long)br * sc.bw);
                    const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
                    m = (long)(br / v) * g.mcu_w + bc / h;
                    b = c == 0 ? (br % v) * h + bc % h : g.luma_blocks + c - 1;
                }
                if (m < 0 || m >= g.mcus || b < 0 || b >= g.blocks) return ST_DESCRIPTOR;   // cannot happen for a checked record
                int16_t* const blk = slot + (m * g.blocks + b) * 64;
                if (!sc.refine) {
                    s.fill();
                    const int sym = huff_symbol(s, pool[sc.tab[c]]);
                    if (sym < 0 || sym > 15) return ST_BAD_CODE;
                    const int diff = s.receive_extend(sym);
                    if (s.real < 0) return ST_EARLY_END;
                    pred[c] += diff;
                    blk[0] = (int16_t)((uint32_t)pred[c] << sc.al);
                } else {
                    const int bit = take_bit(s);
                    if (s.real < 0) return ST_EARLY_END;
                    if (bit) blk[0] = (int16_t)(blk[0] | p1);
                }
            }
            continue;
        }
        // AC: one component, its own block grid
        const int c = sc.comp;
        const int br = (int)(u / sc.bw), bc = (int)(u - (long)br * sc.bw);
        const int h = c == 0 ? g.hs : 1, v = c == 0 ? g.vs : 1;
        const long m = (long)(br / v) * g.mcu_w + bc / h;
        const int b = c == 0 ? (br % v) * h + bc % h : g.luma_blocks + c - 1;
        if (m < 0 || m >= g.mcus || b < 0 || b >= g.blocks) return ST_DESCRIPTOR;
        int16_t* const blk = slot + (m * g.blocks + b) * 64;
        const HuffDec& ac = pool[sc.tab[c]];
        if (!sc.refine) {
            if (eobrun > 0) {
                --eobrun;
                continue;
            }
            for (int k = sc.ss; k <= sc.se; ++k) {   // a symbol advances k by at least one
                s.fill();
                const int sym = huff_symbol(s, ac);
                if (sym < 0) return ST_BAD_CODE;
                const int r = sym >> 4, size = sym & 15;
                if (size) {
                    k += r;
                    const int val = s.receive_extend(size);
                    if (s.real < 0) return ST_EARLY_END;
                    if (k > sc.se || k > 63) return ST_RUN;
                    blk[c_dezigzag[k]] = (int16_t)((uint32_t)val << sc.al);
                } else if (r == 15) {
                    k += 15;
                } else {
                    eobrun = 1 << r;
                    if (r) {
                        eobrun += (int)s.peek(r);
                        s.skip(r);
                    }
                    if (s.real < 0) return ST_EARLY_END;
                    --eobrun;
                    break;
                }
                if (s.real < 0) return ST_EARLY_END;
            }
        } else {
            int k = sc.ss;
            if (eobrun == 0) {
                for (; k <= sc.se; ++k) {
                    s.fill();
                    const int sym = huff_symbol(s, ac);
                    if (sym < 0) return ST_BAD_CODE;
                    int r = sym >> 4;
                    const int size = sym & 15;
                    int val = 0;
                    if (size) {
                        if (size != 1) return ST_BAD_CODE;
                        val = take_bit(s) ? p1 : -p1;
                    } else if (r != 15) {
                        eobrun = 1 << r;
                        if (r) {
                            eobrun += (int)s.peek(r);
                            s.skip(r);
                        }
                        if (s.real < 0) return ST_EARLY_END;
                        break;   // the rest of the band is handled as the first block of the run
                    }
                    if (s.real < 0) return ST_EARLY_END;
                    // over the coefficients with a history (a correction bit each) and r that have none
                    for (; k <= sc.se; ++k) {
                        int16_t* const at = blk + c_dezigzag[k];
                        if (*at != 0) {
                            refine_nonzero(s, at, p1);
                            if (s.real < 0) return ST_EARLY_END;
                        } else if (--r < 0) {
                            break;
                        }
                    }
                    if (val) {
                        if (k > sc.se || k > 63) return ST_RUN;
                        blk[c_dezigzag[k]] = (int16_t)val;
                    }
                }
            }
            if (eobrun > 0) {
                for (; k <= sc.se; ++k) {
                    int16_t* const at = blk + c_dezigzag[k];
                    if (*at != 0) {
                        refine_nonzero(s, at, p1);
                        if (s.real < 0) return ST_EARLY_END;
                    }
                }
                --eobrun;
            }
        }
    }
    return ST_OK;
}

// img int64 [n][4], scans int32 [total_scans][PROG_FIELDS], intervals int32 [total_intervals][2], pool of total_tables
// tables: include/acimg.h has the layout.  Levels run in order; between two levels every lane's stores are made visible to
// the workgroup (one wave: the fence is what matters) before the barrier lets anyone read them.
__global__ __launch_bounds__(64) void jpeg_progressive_kernel(const uint8_t* data, long data_bytes, const int64_t* img,
                                                              const int32_t* scans, long total_scans, const int32_t* intervals,
                                                              long total_intervals, const uint8_t* huff, long total_tables,
                                                              ProgGeometry g, int16_t* coef, int32_t* status) {
    __shared__ ProgScan rec[PROG_MAX_SCANS];
    __shared__ long long first_error[64];
    const int lane = threadIdx.x;
    const long i = blockIdx.x;
    const long per_image = (long)g.mcus * g.blocks * 64;
    int16_t* const slot = coef + (size_t)i * per_image;
    {   // the slot starts as zeros: 128 bytes a block, so 16-byte stores cover it exactly
        uint4* const z = reinterpret_cast<uint4*>(slot);
        for (long q = lane; q < per_image / 8; q += 64) z[q] = make_uint4(0, 0, 0, 0);
    }
    long img_a = img[i * 4 + 0], img_e = img[i * 4 + 1];
    const long first_scan = img[i * 4 + 2], nscan_l = img[i * 4 + 3];
    img_a = img_a < 0 ? 0 : (img_a > data_bytes ? data_bytes : img_a);
    img_e = img_e < img_a ? img_a : (img_e > data_bytes ? data_bytes : img_e);
    if (img_e - img_a > 0x7FFFFFFFl) img_e = img_a + 0x7FFFFFFFl;
    const long img_len = img_e - img_a;
    const bool img_ok = first_scan >= 0 && nscan_l >= 1 && nscan_l <= PROG_MAX_SCANS && first_scan <= total_scans &&
                        nscan_l <= total_scans - first_scan;
    const int nscan = img_ok ? (int)nscan_l : 0;
    for (int k = lane; k < nscan; k += 64) {   // validate: nothing of a record is used before its check
        const int32_t* f = scans + (first_scan + k) * PROG_FIELDS;
        ProgScan sc;
        sc.mask = f[0];
        sc.ss = f[1];
        sc.se = f[2];
        const int ah = f[3];
        sc.al = f[4];
        sc.tab[0] = f[5];
        sc.tab[1] = f[6];
        sc.tab[2] = f[7];
        long restart = f[8];
        long sa = f[9], se = f[10];
        const long first = f[11];
        sc.level = f[12];
        bool ok = sc.mask >= 1 && sc.mask < (1 << g.comps) && sc.ss >= 0 && sc.ss <= sc.se && sc.se <= 63 &&
                  (sc.ss != 0 || sc.se == 0) && ah >= 0 && ah <= 13 && sc.al >= 0 && sc.al <= 13 && restart >= 0 &&
                  sc.level >= 0 && sc.level < nscan && f[13] == 0 && f[14] == 0 && f[15] == 0;
        sc.ncomp = ok ? __popc((unsigned)sc.mask) : 1;
        sc.comp = ok ? __ffs(sc.mask) - 1 : 0;
        ok = ok && (sc.ss == 0 || sc.ncomp == 1);
        sc.refine = ah != 0;
        if (ok && !(sc.ss == 0 && sc.refine))   // DC refinement reads no table
            for (int c = 0; c < g.comps; ++c)
                if (((sc.mask >> c) & 1) && (sc.tab[c] < 0 || sc.tab[c] >= total_tables)) ok = false;
        sc.bw = g.bw[sc.comp];
        const long units = sc.ncomp > 1 ? (long)g.mcus : (long)g.bw[sc.comp] * g.bh[sc.comp];
        if (restart < 1 || restart > units) restart = units;
        const long count = (units + restart - 1) / restart;
        ok = ok && first >= 0 && first <= total_intervals && count <= total_intervals - first;
        sa = sa < 0 ? 0 : (sa > img_len ? img_len : sa);
        se = se < sa ? sa : (se > img_len ? img_len : se);
        sc.units = (int)units;
        sc.restart = (int)restart;
        sc.count = ok ? (int)count : 1;
        sc.seg_a = (int)sa;
        sc.seg_e = (int)se;
        sc.first = (int)first;
        sc.code = ok ? ST_OK : ST_DESCRIPTOR;
        if (!ok) sc.level = 0;
        rec[k] = sc;
    }
    __threadfence_block();
    __syncthreads();
    int top = 0;
    for (int k = 0; k < nscan; ++k) top = rec[k].level > top ? rec[k].level : top;
    long long err = 0x7FFFFFFFFFFFFFFFll;   // (scan << 40) | (interval << 3) | code of this lane's first error in that order
    const HuffDec* const pool = reinterpret_cast<const HuffDec*>(huff);
    for (int level = 0; level <= top; ++level) {
        long t = lane, base = 0;   // item t of this level; items of the level's scans before scan k
        int k = 0;
        while (true) {
            while (k < nscan && (rec[k].level != level || t >= base + rec[k].count)) {
                if (rec[k].level == level) base += rec[k].count;
                ++k;
            }
            if (k >= nscan) break;
            const long j = t - base;
            const int code = prog_item(rec[k], g, j, data, img_a, intervals, pool, slot);
            if (code != ST_OK) {
                const long long key = ((long long)k << 40) | ((long long)j << 3) | code;
                err = key < err ? key : err;
            }
            t += 64;
        }
        __threadfence_block();
        __syncthreads();
    }
    first_error[lane] = err;
    __syncthreads();
    if (lane == 0) {
        long long least = first_error[0];
        for (int q = 1; q < 64; ++q) least = first_error[q] < least ? first_error[q] : least;
        status[i] = !img_ok ? ST_DESCRIPTOR : (least == 0x7FFFFFFFFFFFFFFFll ? ST_OK : (int)(least & 7));
    }
}

// ---- dequantise + jpeg_idct_islow -----------------------------------------------------------------------------------
// 13-bit fixed point; unsigned arithmetic wraps like the 32-bit integers of the definition, the descale is arithmetic
constexpr uint32_t FIX_0_298631336 = 2446, FIX_0_390180644 = 3196, FIX_0_541196100 = 4433, FIX_0_765366865 = 6270,
                   FIX_0_899976223 = 7373, FIX_1_175875602 = 9633, FIX_1_501321110 = 12299, FIX_1_847759065 = 15137,
                   FIX_1_961570560 = 16069, FIX_2_053119869 = 16819, FIX_2_562915447 = 20995, FIX_3_072711026 = 25172;

template <int SHIFT>
__device__ __forceinline__ void idct_1d(const uint32_t x[8], int out[8]) {
    uint32_t z1 = (x[2] + x[6]) * FIX_0_541196100;
    const uint32_t tmp2 = z1 - x[6] * FIX_1_847759065;
    const uint32_t tmp3 = z1 + x[2] * FIX_0_765366865;
    const uint32_t tmp0 = (x[0] + x[4]) << 13, tmp1 = (x[0] - x[4]) << 13;
    const uint32_t tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    uint32_t t0 = x[7], t1 = x[5], t2 = x[3], t3 = x[1];
    z1 = t0 + t3;
    uint32_t z2 = t1 + t2, z3 = t0 + t2, z4 = t1 + t3;
    const uint32_t z5 = (z3 + z4) * FIX_1_175875602;
    t0 *= FIX_0_298631336;
    t1 *= FIX_2_053119869;
    t2 *= FIX_3_072711026;
    t3 *= FIX_1_501321110;
    z1 = 0u - z1 * FIX_0_899976223;
    z2 = 0u - z2 * FIX_2_562915447;
    z3 = z5 - z3 * FIX_1_961570560;
    z4 = z5 - z4 * FIX_0_390180644;
    t0 += z1 + z3;
    t1 += z2 + z4;
    t2 += z2 + z3;
    t3 += z1 + z4;
    const uint32_t o[8] = {tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3};
#pragma unroll
    for (int i = 0; i < 8; ++i) out[i] = ((int)o[i] + (1 << (SHIFT - 1))) >> SHIFT;
}

// 32 blocks per workgroup, eight threads per block.  quant uint8 [n][3][64] natural order, per component.
__global__ __launch_bounds__(256) void jpeg_idct_kernel(const int16_t* coef, const uint8_t* quant, int hs, int vs, int luma_blocks,
                                                        int blocks, long mcu_w, long mcus, long total_blocks, uint8_t* planes) {
    __shared__ int ws[32][64];
    const int tid = threadIdx.x, q = tid >> 3, t = tid & 7;
    const long g = (long)blockIdx.x * 32 + q;   // block b of MCU m of image i
    const bool live = g < total_blocks;
    const long per_image = mcus * blocks;
    const long i = live ? g / per_image : 0, rest = live ? g - i * per_image : 0;
    const long m = rest / blocks;
    const int b = (int)(rest - m * blocks);
    const int c = b < luma_blocks ? 0 : b - luma_blocks + 1;
    if (live) {   // column t
        const int16_t* in = coef + g * 64 + t;
        const uint8_t* qt = quant + (i * 3 + c) * 64 + t;
        uint32_t x[8];
#pragma unroll
        for (int r = 0; r < 8; ++r) x[r] = (uint32_t)((int)in[r * 8] * (int)qt[r * 8]);
        int o[8];
        idct_1d<11>(x, o);
#pragma unroll
        for (int r = 0; r < 8; ++r) ws[q][r * 8 + t] = o[r];
    }
    __syncthreads();
    if (live) {   // row t
        uint32_t x[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) x[u] = (uint32_t)ws[q][t * 8 + u];
        int o[8];
        idct_1d<18>(x, o);
        uint32_t w[2] = {0, 0};
#pragma unroll
        for (int u = 0; u < 8; ++u) w[u >> 2] |= (uint32_t)min(max(o[u] + 128, 0), 255) << ((u & 3) * 8);
        const int h = c == 0 ? hs : 1, v = c == 0 ? vs : 1, bc = c == 0 ? b : 0;
        const long mx = m % mcu_w, my = m / mcu_w;
        const long pw = mcu_w * h * 8;
        const long x0 = (mx * h + bc % h) * 8, y = (my * v + bc / h) * 8 + t;
        const long plane0 = c == 0 ? 0 : mcus * 64 * (luma_blocks + c - 1);
        uint8_t* dst = planes + i * per_image * 64 + plane0 + y * pw + x0;
        *reinterpret_cast<uint2*>(dst) = make_uint2(w[0], w[1]);
    }
}

// ---- fancy upsampling + colour ----------------------------------------------------------------------------------------
// chroma sample (y, x) of the picture from plane p of cw x ch true samples, pw bytes a row
__device__ __forceinline__ int chroma_at(const uint8_t* p, long pw, int cw, int ch, int hs, int vs, int y, int x) {
    if (hs == 1) return p[(long)y * pw + x];
    const int i = x >> 1;
    const int il = i > 0 ? i - 1 : 0, ir = i < cw - 1 ? i + 1 : cw - 1;
    if (vs == 1) {
        const uint8_t* a = p + (long)y * pw;
        if (x & 1) return i == cw - 1 ? a[i] : (3 * a[i] + a[ir] + 2) >> 2;
        return i == 0 ? a[i] : (3 * a[i] + a[il] + 1) >> 2;
    }
    const int r = y >> 1;
    const int rn = (y & 1) ? (r < ch - 1 ? r + 1 : ch - 1) : (r > 0 ? r - 1 : 0);
    const uint8_t* a = p + (long)r * pw;
    const uint8_t* nb = p + (long)rn * pw;
    const int s = 3 * a[i] + nb[i];
    if (x & 1) return (3 * s + (3 * a[ir] + nb[ir]) + 7) >> 4;   // at the right edge ir = i: (4 s + 7) >> 4
    return (3 * s + (3 * a[il] + nb[il]) + 8) >> 4;
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(const uint8_t* planes, int H, int W, int comps, int hs, int vs,
                                                          long mcu_w, long mcus, int blocks, long total, uint8_t* bgr) {
    const long g = (long)blockIdx.x * 256 + threadIdx.x;   // pixel (y, x) of image i
    if (g >= total) return;
    const long hw = (long)H * W;
    const long i = g / hw, rest = g - i * hw;
    const int y = (int)(rest / W), x = (int)(rest - (long)y * W);
    const uint8_t* base = planes + i * mcus * blocks * 64;
    const long pwy = mcu_w * hs * 8;
    const int Y = base[(long)y * pwy + x];
    int R = Y, G = Y, B = Y;
    if (comps == 3) {
        const long pwc = mcu_w * 8, csize = mcus * 64;
        const uint8_t* pcb = base + mcus * 64 * hs * vs;
        const int cw = (W + hs - 1) / hs, ch = (H + vs - 1) / vs;
        const int cb = chroma_at(pcb, pwc, cw, ch, hs, vs, y, x) - 128;
        const int cr = chroma_at(pcb + csize, pwc, cw, ch, hs, vs, y, x) - 128;
        R = Y + ((91881 * cr + 32768) >> 16);
        B = Y + ((116130 * cb + 32768) >> 16);
        G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
    }
    uint8_t* o = bgr + g * 3;
    o[0] = (uint8_t)min(max(B, 0), 255);
    o[1] = (uint8_t)min(max(G, 0), 255);
    o[2] = (uint8_t)min(max(R, 0), 255);
}

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_jpeg_decode_coef_bytes(int n, int H, int W, int comps, int hs, int vs) {
    if (n < 1 || !jpeg_dec_args_ok(H, W, comps, hs, vs)) return 0;
    const DecGeometry g = jpeg_dec_geometry(H, W, comps, hs, vs);
    return (size_t)n * g.mcus * g.blocks * 64 * sizeof(int16_t);
}

size_t acimg_jpeg_decode_plane_bytes(int n, int H, int W, int comps, int hs, int vs) {
    if (n < 1 || !jpeg_dec_args_ok(H, W, comps, hs, vs)) return 0;
    const DecGeometry g = jpeg_dec_geometry(H, W, comps, hs, vs);
    return (size_t)n * g.mcus * g.blocks * 64;
}

size_t acimg_jpeg_decode_pixel_bytes(int n, int H, int W) {
    if (n < 1 || H < 1 || H > JPEG_DEC_MAX_DIM || W < 1 || W > JPEG_DEC_MAX_DIM) return 0;
    return (size_t)n * H * W * 3;
}

int acimg_jpeg_decode_entropy(const uint8_t* data, size_t data_bytes, const int64_t* desc, const int32_t* intervals,
                              long total_intervals, const uint8_t* huff, int n, int H, int W, int comps, int hs, int vs,
                              int16_t* coef, size_t coef_bytes, int32_t* status, void* stream) {
    if (!data || !desc || !intervals || !huff || !coef || !status) return fail(ACIMG_EINVAL, "jpeg_decode_entropy: null argument");
    if (n < 1) return fail(ACIMG_EINVAL, "jpeg_decode_entropy: n = %d must be positive", n);
    if (!jpeg_dec_args_ok(H, W, comps, hs, vs))
        return fail(ACIMG_EINVAL, "jpeg_decode_entropy: %d x %d, %d component(s), sampling %d x %d is not decoded", H, W, comps,
                    hs, vs);
    if (total_intervals < 1 || data_bytes > (size_t)INT64_MAX)
        return fail(ACIMG_EINVAL, "jpeg_decode_entropy: %ld intervals in %zu bytes", total_intervals, data_bytes);
    if (!aligned16(coef) || !aligned16(huff) || !aligned16(desc) || !aligned16(intervals))
        return fail(ACIMG_EINVAL, "jpeg_decode_entropy: coef, huff, desc and intervals must be 16-byte aligned");
    const size_t need = acimg_jpeg_decode_coef_bytes(n, H, W, comps, hs, vs);
    if (coef_bytes < need) return fail(ACIMG_EWORKSPACE, "jpeg_decode_entropy: coef of %zu < %zu bytes", coef_bytes, need);
    const DecGeometry g = jpeg_dec_geometry(H, W, comps, hs, vs);
    hipLaunchKernelGGL(jpeg_entropy_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, data, (long)data_bytes, desc,
                       intervals, total_intervals, huff, comps, comps == 1 ? 1 : hs * vs, g.blocks, g.mcus, coef, status);
    return check_launch("jpeg_decode_entropy");
}

int acimg_jpeg_decode_progressive(const uint8_t* data, size_t data_bytes, const int64_t* img, const int32_t* scans,
                                  long total_scans, const int32_t* intervals, long total_intervals, const uint8_t* huff,
                                  long total_tables, int n, int H, int W, int comps, int hs, int vs, int16_t* coef,
                                  size_t coef_bytes, int32_t* status, void* stream) {
    if (!data || !img || !scans || !intervals || !huff || !coef || !status)
        return fail(ACIMG_EINVAL, "jpeg_decode_progressive: null argument");
    if (n < 1) return fail(ACIMG_EINVAL, "jpeg_decode_progressive: n = %d must be positive", n);
    if (!jpeg_dec_args_ok(H, W, comps, hs, vs))
        return fail(ACIMG_EINVAL, "jpeg_decode_progressive: %d x %d, %d component(s), sampling %d x %d is not decoded", H, W,
                    comps, hs, vs);
    if (total_scans < 1 || total_intervals < 1 || total_tables < 1 || data_bytes > (size_t)INT64_MAX)
        return fail(ACIMG_EINVAL, "jpeg_decode_progressive: %ld scans, %ld intervals, %ld tables in %zu bytes", total_scans,
                    total_intervals, total_tables, data_bytes);
    if (!aligned16(coef) || !aligned16(huff) || !aligned16(img) || !aligned16(scans) || !aligned16(intervals))
        return fail(ACIMG_EINVAL, "jpeg_decode_progressive: coef, huff, img, scans and intervals must be 16-byte aligned");
    const size_t need = acimg_jpeg_decode_coef_bytes(n, H, W, comps, hs, vs);
    if (coef_bytes < need) return fail(ACIMG_EWORKSPACE, "jpeg_decode_progressive: coef of %zu < %zu bytes", coef_bytes, need);
    const DecGeometry d = jpeg_dec_geometry(H, W, comps, hs, vs);
    ProgGeometry g;
    g.comps = comps;
    g.hs = hs;
    g.vs = vs;
    g.luma_blocks = comps == 1 ? 1 : hs * vs;
    g.blocks = d.blocks;
    g.mcu_w = (int)d.mcu_w;
    g.mcus = (int)d.mcus;
    for (int c = 0; c < 3; ++c) {   // component 0 has the largest factors, so its samples are the picture's
        const int cw = c == 0 ? W : (W + hs - 1) / hs, ch = c == 0 ? H : (H + vs - 1) / vs;
        g.bw[c] = (cw + 7) / 8;
        g.bh[c] = (ch + 7) / 8;
    }
    hipLaunchKernelGGL(jpeg_progressive_kernel, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, data, (long)data_bytes, img,
                       scans, total_scans, intervals, total_intervals, huff, total_tables, g, coef, status);
    return check_launch("jpeg_decode_progressive");
}

int acimg_jpeg_decode_idct(const int16_t* coef, const uint8_t* quant, int n, int H, int W, int comps, int hs, int vs,
                           uint8_t* planes, size_t plane_bytes, void* stream) {
    if (!coef || !quant || !planes) return fail(ACIMG_EINVAL, "jpeg_decode_idct: null argument");
    if (n < 1) return fail(ACIMG_EINVAL, "jpeg_decode_idct: n = %d must be positive", n);
    if (!jpeg_dec_args_ok(H, W, comps, hs, vs))
        return fail(ACIMG_EINVAL, "jpeg_decode_idct: %d x %d, %d component(s), sampling %d x %d is not decoded", H, W, comps, hs,
                    vs);
    if (!aligned16(coef) || !aligned16(planes)) return fail(ACIMG_EINVAL, "jpeg_decode_idct: coef and planes must be 16-byte aligned");
    const size_t need = acimg_jpeg_decode_plane_bytes(n, H, W, comps, hs, vs);
    if (plane_bytes < need) return fail(ACIMG_EWORKSPACE, "jpeg_decode_idct: planes of %zu < %zu bytes", plane_bytes, need);
    const DecGeometry g = jpeg_dec_geometry(H, W, comps, hs, vs);
    const long total = (long)n * g.mcus * g.blocks;
    const long grid = (total + 31) / 32;
    if (grid > (long)INT32_MAX) return fail(ACIMG_EINVAL, "jpeg_decode_idct: %ld blocks exceed the grid", total);
    hipLaunchKernelGGL(jpeg_idct_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, coef, quant, hs, vs,
                       comps == 1 ? 1 : hs * vs, g.blocks, g.mcu_w, g.mcus, total, planes);
    return check_launch("jpeg_decode_idct");
}

int acimg_jpeg_decode_colour(const uint8_t* planes, int n, int H, int W, int comps, int hs, int vs, uint8_t* bgr,
                             size_t bgr_bytes, void* stream) {
    if (!planes || !bgr) return fail(ACIMG_EINVAL, "jpeg_decode_colour: null argument");
    if (n < 1) return fail(ACIMG_EINVAL, "jpeg_decode_colour: n = %d must be positive", n);
    if (!jpeg_dec_args_ok(H, W, comps, hs, vs))
        return fail(ACIMG_EINVAL, "jpeg_decode_colour: %d x %d, %d component(s), sampling %d x %d is not decoded", H, W, comps,
                    hs, vs);
    const size_t need = acimg_jpeg_decode_pixel_bytes(n, H, W);
    if (bgr_bytes < need) return fail(ACIMG_EWORKSPACE, "jpeg_decode_colour: pixels of %zu < %zu bytes", bgr_bytes, need);
    const DecGeometry g = jpeg_dec_geometry(H, W, comps, hs, vs);
    const long total = (long)n * H * W;
    const long grid = (total + 255) / 256;
    if (grid > (long)INT32_MAX) return fail(ACIMG_EINVAL, "jpeg_decode_colour: %ld pixels exceed the grid", total);
    hipLaunchKernelGGL(jpeg_colour_kernel, dim3((unsigned)grid), dim3(256), 0, (hipStream_t)stream, planes, H, W, comps, hs, vs,
                       g.mcu_w, g.mcus, g.blocks, total, bgr);
    return check_launch("jpeg_decode_colour");
}

}  // extern "C"
