// Baseline JPEG (ITU-T T.81, sequential DCT, Huffman, 8 bit) of RGB8 frames on the GPU, 4:2:0: the encoder behind the
// Motion-JPEG track of `python -m acimg.show video --avi 1` (the clip showvideo.py:239-263 leaves to two ffmpeg runs).
// Integer arithmetic throughout, so that tests/jpeg_ref.py restates it bit for bit on any machine.
//
// acimg_jpeg_blocks: one workgroup of 384 threads per 16 x 16 MCU (raster order; the frame is extended to the MCU grid by
//   replicating its last column and row).  256 threads convert one pixel each (JFIF full range, 16-bit fixed point),
//   128 form the 2 x 2 chroma means, then every thread owns one coefficient of the MCU's six 8 x 8 blocks (Y00 Y01 Y10 Y11
//   Cb Cr) through the row pass, the column pass and the quantiser, and the block leaves in zig-zag order as int16.
//     s = sample - 128;  T = rint(2^14 A) (A the orthonormal DCT-II matrix, formed in fp64 and kept below as constants)
//     rows     p[y][u] = sum_x T[u][x] s[y][x]      |p| <= 2^23      p' = (p + 256) >> 9
//     columns  q[v][u] = sum_y T[v][y] p'[y][u]     |q| <  2^30      (the scale of q is 2^19)
//     quantise d = Q[v][u] << 19,  c = sign(q) (|q| + (d >> 1)) / d,  AC clamped to +-1023
// acimg_jpeg_scan: the entropy coder, three launches.  The DC predictors of an MCU are the previous MCU's DC values (0
//   at the start of a restart interval of restart_mcus MCUs), so every MCU can be coded on its own: ONE LANE per MCU
//   writes its six blocks as unstuffed bits into the MCU's slot of the workspace and records the bit count.  Then one
//   wave per (frame, interval) turns the counts into bit offsets (a wave scan) and assembles the interval's bytes, 64 per
//   step: a lane gathers its byte from the one or two MCUs that hold its eight bits, the last byte is padded with
//   1-bits, and a ballot counts the 0xFF bytes in front of a lane, behind each of which a 0x00 is stuffed.  Last, one
//   workgroup per frame forms the prefix of the interval lengths and copies the intervals and the RSTm markers between
//   them densely into the frame's output, one wave per interval.  The four Huffman tables are Annex K.3's, derived from
//   BITS / HUFFVAL at compile time into constant memory and copied to LDS by each workgroup (a lane's look-ups diverge).
//   Worst case: a block takes at most 22 bits of DC (11-bit code + 11 bits) and 63 x 26 bits of AC (16-bit code + 10
//   bits): 1660 bits, so an MCU's six blocks take at most 9960 bits = 1245 bytes, 2490 with every byte stuffed.  The
//   coder clamps what it reads (DC difference to +-2047, AC to +-1023), so no input exceeds that.
// No atomics, no floating point; every output byte is written by exactly one thread: bit-identical from run to run.
#include "common.hpp"

namespace acimg {

constexpr int MCU_BYTES_MAX = 2490;       // stuffed bytes of one MCU at most (see above)
constexpr int JPEG_MAX_DIM = 65535;

// T = rint(2^14 A), [u][x]
__constant__ int c_dct[64] = {
    5793, 5793,  5793,  5793,  5793,  5793,  5793,  5793,   //
    8035, 6811,  4551,  1598,  -1598, -4551, -6811, -8035,  //
    7568, 3135,  -3135, -7568, -7568, -3135, 3135,  7568,   //
    6811, -1598, -8035, -4551, 4551,  8035,  1598,  -6811,  //
    5793, -5793, -5793, 5793,  5793,  -5793, -5793, 5793,   //
    4551, -8035, 1598,  6811,  -6811, -1598, 8035,  -4551,  //
    3135, -7568, 7568,  -3135, -3135, 7568,  -7568, 3135,   //
    1598, -4551, 6811,  -8035, 8035,  -6811, 4551,  -1598};

// natural (row-major) index -> position in zig-zag order
__constant__ uint8_t c_zigzag_pos[64] = {0,  1,  5,  6,  14, 15, 27, 28, 2,  4,  7,  13, 16, 26, 29, 42, 3,  8,  12, 17, 25, 30,
                                         41, 43, 9,  11, 18, 24, 31, 40, 44, 53, 10, 19, 23, 32, 39, 45, 52, 54, 20, 22, 33, 38,
                                         46, 51, 55, 60, 21, 34, 37, 47, 50, 56, 59, 61, 35, 36, 48, 49, 57, 58, 62, 63};

// Annex K.1 / K.2 (quality 50), natural order
constexpr uint8_t BASE_Q[2][64] = {
    {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
     103, 99},
    {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99,
     99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99}};

// Annex K.3: BITS (codes per length 1..16) and HUFFVAL of the four typical tables
constexpr uint8_t DC_LUMA_BITS[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
constexpr uint8_t DC_CHROMA_BITS[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
constexpr uint8_t DC_VALS[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
constexpr uint8_t AC_LUMA_BITS[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
constexpr uint8_t AC_LUMA_VALS[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xa1, 0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18,
    0x19, 0x1a, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3,
    0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5,
    0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};
constexpr uint8_t AC_CHROMA_BITS[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
constexpr uint8_t AC_CHROMA_VALS[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25,
    0xf1, 0x17, 0x18, 0x19, 0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba,
    0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4,
    0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9, 0xfa};

// symbol -> (length << 16) | code; 0 for a symbol the table does not hold.  dc[comp][category], ac[comp][run << 4 | size]
struct HuffTables {
    uint32_t dc[2][16];
    uint32_t ac[2][256];
};
constexpr int HUFF_WORDS = sizeof(HuffTables) / 4;

constexpr void huff_fill(uint32_t* table, const uint8_t* bits, const uint8_t* vals) {   // Annex C
    uint32_t code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i) table[vals[k++]] = ((uint32_t)len << 16) | code++;
        code <<= 1;
    }
}
constexpr HuffTables make_huff() {
    HuffTables t{};
    huff_fill(t.dc[0], DC_LUMA_BITS, DC_VALS);
    huff_fill(t.dc[1], DC_CHROMA_BITS, DC_VALS);
    huff_fill(t.ac[0], AC_LUMA_BITS, AC_LUMA_VALS);
    huff_fill(t.ac[1], AC_CHROMA_BITS, AC_CHROMA_VALS);
    return t;
}
__constant__ HuffTables c_huff = make_huff();

struct JpegGeometry {
    long mcu_w, mcu_h, mcus, intervals;
    size_t slot_stride, capacity;
};
inline bool jpeg_dims_ok(int H, int W) { return H >= 1 && H <= JPEG_MAX_DIM && W >= 1 && W <= JPEG_MAX_DIM; }
inline JpegGeometry jpeg_geometry(int H, int W, int restart_mcus) {
    JpegGeometry g;
    g.mcu_w = (W + 15) / 16;
    g.mcu_h = (H + 15) / 16;
    g.mcus = g.mcu_w * g.mcu_h;
    g.intervals = (g.mcus + restart_mcus - 1) / restart_mcus;
    g.slot_stride = (size_t)MCU_BYTES_MAX * restart_mcus + 2;                 // an interval's bytes, its pad stuffed
    g.capacity = (size_t)MCU_BYTES_MAX * g.mcus + 4 * (size_t)g.intervals;    // + pad (stuffed) and marker per interval
    return g;
}
inline size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// ---- colour, chroma means, DCT, quantiser ---------------------------------------------------------------------------
__global__ __launch_bounds__(384) void jpeg_blocks_kernel(const uint8_t* rgb, int H, int W, int mcu_w, const uint8_t* qtables,
                                                          int16_t* coef) {
    __shared__ int smp[6][64];      // level-shifted samples, then the coefficients in zig-zag order
    __shared__ int row[6][64];      // after the row pass
    __shared__ int chroma[2][256];  // Cb, Cr of the MCU's 256 pixels
    __shared__ int T[64];
    const int tid = threadIdx.x;
    const long m = blockIdx.x, n = blockIdx.y, mcus = gridDim.x;
    const int mx = (int)(m % mcu_w), my = (int)(m / mcu_w);
    if (tid < 64) T[tid] = c_dct[tid];
    if (tid < 256) {
        const int py = tid >> 4, px = tid & 15;
        const int gy = min(my * 16 + py, H - 1), gx = min(mx * 16 + px, W - 1);
        const uint8_t* p = rgb + (((long)n * H + gy) * W + gx) * 3;
        const int R = p[0], G = p[1], B = p[2];
        const int Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16;
        const int Cb = ((-11059 * R - 21709 * G + 32768 * B + 32767) >> 16) + 128;
        const int Cr = ((32768 * R - 27439 * G - 5329 * B + 32767) >> 16) + 128;
        smp[(py >> 3) * 2 + (px >> 3)][(py & 7) * 8 + (px & 7)] = Y - 128;
        chroma[0][tid] = min(max(Cb, 0), 255);
        chroma[1][tid] = min(max(Cr, 0), 255);
    }
    __syncthreads();
    if (tid < 128) {   // 2 x 2 means; the rounding term alternates 1, 2 along a row of chroma samples (8 per MCU: cx's parity)
        const int c = tid >> 6, i = tid & 63, cy = i >> 3, cx = i & 7;
        const int* q = &chroma[c][cy * 32 + cx * 2];
        smp[4 + c][i] = ((q[0] + q[1] + q[16] + q[17] + 1 + (cx & 1)) >> 2) - 128;
    }
    __syncthreads();
    const int b = tid >> 6, i = tid & 63, hi = i >> 3, lo = i & 7;
    {   // rows: hi = y, lo = u
        int p = 0;
#pragma unroll
        for (int x = 0; x < 8; ++x) p += T[lo * 8 + x] * smp[b][hi * 8 + x];
        row[b][i] = (p + 256) >> 9;
    }
    __syncthreads();
    int q = 0;   // columns: hi = v, lo = u
#pragma unroll
    for (int y = 0; y < 8; ++y) q += T[hi * 8 + y] * row[b][y * 8 + lo];
    const int Q = max((int)qtables[(b < 4 ? 0 : 64) + i], 1);
    const unsigned d = (unsigned)Q << 19;
    int c = (int)(((unsigned)abs(q) + (d >> 1)) / d);
    if (q < 0) c = -c;
    if (i != 0) c = min(max(c, -1023), 1023);
    smp[b][c_zigzag_pos[i]] = c;   // every thread read its samples before the last barrier
    __syncthreads();
    coef[((n * mcus + m) * 6 + b) * 64 + i] = (int16_t)smp[b][i];
}

// ---- entropy coding ---------------------------------------------------------------------------------------------------
constexpr int MCU_SLOT = 1248;    // 1245 unstuffed bytes of an MCU at most, rounded up to 16

struct BitSink {   // MSB-first bits into bytes; no stuffing here: the merge stuffs once the bytes have their final phase
    uint64_t acc;
    int n;
    uint8_t* p;
    __device__ __forceinline__ void put(uint32_t code, int len) {   // len <= 26; the bits above `len` of code are 0
        acc = (acc << len) | code;
        n += len;
        while (n >= 8) {
            *p++ = (uint8_t)(acc >> (n - 8));
            n -= 8;
        }
    }
    __device__ __forceinline__ void put_symbol(uint32_t entry) { put(entry & 0xFFFFu, (int)(entry >> 16)); }
};

// category of v (bits of |v|) and the bits that follow the symbol: v, or v + 2^size - 1 for a negative v
__device__ __forceinline__ int magnitude(int v, uint32_t& bits) {
    const int a = abs(v);
    const int size = 32 - __clz(a);
    bits = (uint32_t)(v < 0 ? v + (1 << size) - 1 : v) & ((1u << size) - 1);
    return size;
}

// one lane per MCU: its six blocks as unstuffed bits at the start of its slot (the last byte's unused low bits are 0), and
// the number of bits.  The DC predictors are the previous MCU's DC values, 0 at the start of a restart interval.
__global__ __launch_bounds__(64) void jpeg_code_kernel(const int16_t* coef, long mcus, int restart_mcus, long total,
                                                       uint8_t* mcu_slots, int32_t* mcu_bits) {
    __shared__ HuffTables huff;
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(&c_huff);
        uint32_t* dst = reinterpret_cast<uint32_t*>(&huff);
        for (int i = threadIdx.x; i < HUFF_WORDS; i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const long g = (long)blockIdx.x * 64 + threadIdx.x;   // MCU m of frame f
    if (g >= total) return;
    const long m = g % mcus;
    const int16_t* c = coef + g * 384;
    int pred_y = 0, pred_cb = 0, pred_cr = 0;
    if (m % restart_mcus != 0) {
        pred_y = c[-384 + 3 * 64];
        pred_cb = c[-384 + 4 * 64];
        pred_cr = c[-384 + 5 * 64];
    }
    uint8_t* const out = mcu_slots + (size_t)g * MCU_SLOT;
    BitSink w = {0, 0, out};
    const uint4* blk = reinterpret_cast<const uint4*>(c);
    for (int b = 0; b < 6; ++b, blk += 8) {
        const int comp = b < 4 ? 0 : 1;
        int run = 0;
        for (int v = 0; v < 8; ++v) {
            const uint4 q = blk[v];
            if (v > 0 && (q.x | q.y | q.z | q.w) == 0) {
                run += 8;
                continue;
            }
            const uint32_t word[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                int val = (int)(int16_t)(word[e >> 1] >> ((e & 1) * 16));
                uint32_t bits;
                if (v == 0 && e == 0) {
                    const int pred = b < 4 ? pred_y : (b == 4 ? pred_cb : pred_cr);
                    const int diff = min(max(val - pred, -2047), 2047);
                    if (b < 4) pred_y = val;
                    const int size = magnitude(diff, bits);
                    w.put_symbol(huff.dc[comp][size]);
                    w.put(bits, size);
                    continue;
                }
                if (val == 0) {
                    ++run;
                    continue;
                }
                while (run > 15) {
                    w.put_symbol(huff.ac[comp][0xF0]);   // ZRL
                    run -= 16;
                }
                val = min(max(val, -1023), 1023);
                const int size = magnitude(val, bits);
                w.put_symbol(huff.ac[comp][(run << 4) | size]);
                w.put(bits, size);
                run = 0;
            }
        }
        if (run > 0) w.put_symbol(huff.ac[comp][0x00]);   // EOB
    }
    const int nbits = (int)(w.p - out) * 8 + w.n;
    if (w.n > 0) *w.p = (uint8_t)(w.acc << (8 - w.n));
    mcu_bits[g] = nbits;
}

// one wave per (frame, interval): the bit offsets of its MCUs (in place of their bit counts), then the interval's bytes, 64
// per step: a lane gathers its byte from the one or two MCUs that hold its bits (an MCU has at least 32 bits), the tail of
// the last byte is padded with 1-bits, and the bytes go to the interval's slot behind the 0x00s stuffed so far.
__global__ __launch_bounds__(64) void jpeg_merge_kernel(const uint8_t* mcu_slots, int32_t* mcu_bits, long mcus, int restart_mcus,
                                                        long intervals, uint8_t* slots, size_t slot_stride, int32_t* lens) {
    const int lane = threadIdx.x;
    const long g = blockIdx.x;   // interval j of frame f
    const long f = g / intervals, j = g - f * intervals;
    const long m0 = j * restart_mcus;
    const int count = (int)((m0 + restart_mcus < mcus ? m0 + restart_mcus : mcus) - m0);
    int32_t* const pre = mcu_bits + f * mcus + m0;
    const uint8_t* const src = mcu_slots + (size_t)(f * mcus + m0) * MCU_SLOT;
    int total_bits = 0;
    for (int base = 0; base < count; base += 64) {   // exclusive prefix, a wave scan per 64 MCUs
        const int i = base + lane;
        const int bits = i < count ? pre[i] : 0;
        int inc = bits;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int up = __shfl_up(inc, o, 64);
            if (lane >= o) inc += up;
        }
        if (i < count) pre[i] = total_bits + inc - bits;
        total_bits += __shfl(inc, 63, 64);
    }
    __syncthreads();   // one wave: orders the prefix stores before the reads below
    const int nbytes = (total_bits + 7) >> 3;
    uint8_t* const out = slots + (size_t)g * slot_stride;
    int stuffed = 0;
    for (int base = 0; base < nbytes; base += 64) {
        const int k = base + lane;
        uint32_t byte = 0;
        if (k < nbytes) {
            const int p = k * 8;
            int lo = 0, hi = count - 1;   // the last MCU whose offset is <= p
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= p) lo = mid;
                else hi = mid - 1;
            }
            const int end = lo + 1 < count ? pre[lo + 1] : total_bits;
            const int o = p - pre[lo], avail = end - p;   // avail >= 1 bits of this MCU from bit o on
            const uint8_t* s = src + (size_t)lo * MCU_SLOT + (o >> 3);
            byte = ((((uint32_t)s[0] << 8) | s[1]) >> (8 - (o & 7))) & 0xFFu;
            if (avail < 8) {
                const uint32_t rest = lo + 1 < count ? src[(size_t)(lo + 1) * MCU_SLOT] : 0xFFu;   // next MCU, or the pad
                byte = (byte & (0xFF00u >> avail) & 0xFFu) | (rest >> avail);
            }
        }
        const bool ff = k < nbytes && byte == 0xFFu;
        const uint64_t mask = __ballot(ff);
        if (k < nbytes) {
            uint8_t* d = out + k + stuffed + __popcll(mask & ((1ull << lane) - 1));
            d[0] = (uint8_t)byte;
            if (ff) d[1] = 0;
        }
        stuffed += __popcll(mask);
    }
    if (lane == 0) lens[g] = nbytes + stuffed;
}

// one workgroup per frame: offsets of its intervals (each followed by a 2-byte marker, but the last), then the copy
__global__ __launch_bounds__(256) void jpeg_pack_kernel(const uint8_t* slots, size_t slot_stride, const int32_t* lens, int32_t* offs,
                                                        long intervals, uint8_t* scan, size_t frame_stride, int32_t* scan_bytes) {
    __shared__ int32_t part[256];
    const int tid = threadIdx.x;
    const long f = blockIdx.x;
    lens += f * intervals;
    offs += f * intervals;
    const long chunk = (intervals + 255) / 256;
    const long a = tid * chunk < intervals ? tid * chunk : intervals;
    const long e = a + chunk < intervals ? a + chunk : intervals;
    int32_t sum = 0;
    for (long j = a; j < e; ++j) sum += lens[j] + 2;
    part[tid] = sum;
    __syncthreads();
    int32_t base = 0;
    for (int t = 0; t < tid; ++t) base += part[t];
    int32_t at = base;
    for (long j = a; j < e; ++j) {
        offs[j] = at;
        at += lens[j] + 2;
    }
    if (tid == 255) scan_bytes[f] = base + sum - 2;
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    for (long j = wave; j < intervals; j += 4) {
        const uint8_t* src = slots + (size_t)(f * intervals + j) * slot_stride;
        uint8_t* dst = scan + (size_t)f * frame_stride + offs[j];
        const int len = lens[j];
        for (int i = lane; i < len; i += 64) dst[i] = src[i];
        if (lane == 0 && j + 1 < intervals) {
            dst[len] = 0xFF;
            dst[len + 1] = (uint8_t)(0xD0 + (j & 7));
        }
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_jpeg_quant_tables(int quality, uint8_t* out) {
    if (quality < 1 || quality > 100) return fail(ACIMG_EINVAL, "jpeg_quant_tables: quality = %d outside 1..100", quality);
    if (!out) return fail(ACIMG_EINVAL, "jpeg_quant_tables: null argument");
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality;
    for (int t = 0; t < 2; ++t)
        for (int i = 0; i < 64; ++i) {
            const int v = (BASE_Q[t][i] * s + 50) / 100;
            out[t * 64 + i] = (uint8_t)(v < 1 ? 1 : (v > 255 ? 255 : v));
        }
    return ACIMG_OK;
}

size_t acimg_jpeg_coef_bytes(int n, int H, int W) {
    if (n < 1 || !jpeg_dims_ok(H, W)) return 0;
    return (size_t)n * jpeg_geometry(H, W, 1).mcus * 6 * 64 * sizeof(int16_t);
}

size_t acimg_jpeg_scan_capacity(int H, int W, int restart_mcus) {
    if (!jpeg_dims_ok(H, W) || restart_mcus < 1 || restart_mcus > 65535) return 0;
    return jpeg_geometry(H, W, restart_mcus).capacity;
}

size_t acimg_jpeg_scan_workspace(int n, int H, int W, int restart_mcus) {
    if (n < 1 || !jpeg_dims_ok(H, W) || restart_mcus < 1 || restart_mcus > 65535) return 0;
    const JpegGeometry g = jpeg_geometry(H, W, restart_mcus);
    const size_t slots = (size_t)n * g.intervals, units = (size_t)n * g.mcus;
    return align16(slots * 2 * sizeof(int32_t)) + align16(units * sizeof(int32_t)) + units * MCU_SLOT + slots * g.slot_stride;
}

int acimg_jpeg_blocks(const uint8_t* rgb, int n, int H, int W, const uint8_t* qtables, int16_t* coef, void* stream) {
    if (!rgb || !qtables || !coef) return fail(ACIMG_EINVAL, "jpeg_blocks: null argument");
    if (n < 1 || n > 65535) return fail(ACIMG_EINVAL, "jpeg_blocks: n = %d outside 1..65535", n);
    if (!jpeg_dims_ok(H, W)) return fail(ACIMG_EINVAL, "jpeg_blocks: %d x %d outside 1..65535", H, W);
    const JpegGeometry g = jpeg_geometry(H, W, 1);
    hipLaunchKernelGGL(jpeg_blocks_kernel, dim3((unsigned)g.mcus, n), dim3(384), 0, (hipStream_t)stream, rgb, H, W, (int)g.mcu_w,
                       qtables, coef);
    return check_launch("jpeg_blocks");
}

int acimg_jpeg_scan(const int16_t* coef, int n, int H, int W, int restart_mcus, uint8_t* scan, size_t frame_stride,
                    int32_t* scan_bytes, void* ws, size_t ws_bytes, void* stream) {
    if (!coef || !scan || !scan_bytes || !ws) return fail(ACIMG_EINVAL, "jpeg_scan: null argument");
    if (n < 1) return fail(ACIMG_EINVAL, "jpeg_scan: n = %d must be positive", n);
    if (!jpeg_dims_ok(H, W)) return fail(ACIMG_EINVAL, "jpeg_scan: %d x %d outside 1..65535", H, W);
    if (restart_mcus < 1 || restart_mcus > 65535)
        return fail(ACIMG_EINVAL, "jpeg_scan: restart_mcus = %d outside 1..65535", restart_mcus);
    const JpegGeometry g = jpeg_geometry(H, W, restart_mcus);
    if (g.capacity > (size_t)INT32_MAX)
        return fail(ACIMG_EINVAL, "jpeg_scan: a frame's capacity of %zu bytes exceeds the int32 of scan_bytes", g.capacity);
    if (frame_stride < g.capacity)
        return fail(ACIMG_EINVAL, "jpeg_scan: frame_stride = %zu < capacity %zu", frame_stride, g.capacity);
    const long total = (long)n * g.intervals;
    if (total > (long)INT32_MAX) return fail(ACIMG_EINVAL, "jpeg_scan: %ld intervals exceed the grid", total);
    if (!aligned16(coef) || !aligned16(ws)) return fail(ACIMG_EINVAL, "jpeg_scan: coef and ws must be 16-byte aligned");
    const size_t need = acimg_jpeg_scan_workspace(n, H, W, restart_mcus);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "jpeg_scan: workspace %zu < %zu bytes", ws_bytes, need);
    const long units = (long)n * g.mcus;
    int32_t* lens = (int32_t*)ws;
    int32_t* offs = lens + total;
    uint8_t* at = (uint8_t*)ws + align16((size_t)total * 2 * sizeof(int32_t));
    int32_t* mcu_bits = (int32_t*)at;
    at += align16((size_t)units * sizeof(int32_t));
    uint8_t* mcu_slots = at;
    uint8_t* slots = at + (size_t)units * MCU_SLOT;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(jpeg_code_kernel, dim3((unsigned)((units + 63) / 64)), dim3(64), 0, s, coef, g.mcus, restart_mcus, units,
                       mcu_slots, mcu_bits);
    int rc = check_launch("jpeg_scan (code)");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_merge_kernel, dim3((unsigned)total), dim3(64), 0, s, (const uint8_t*)mcu_slots, mcu_bits, g.mcus,
                       restart_mcus, g.intervals, slots, g.slot_stride, lens);
    rc = check_launch("jpeg_scan (merge)");
    if (rc) return rc;
    hipLaunchKernelGGL(jpeg_pack_kernel, dim3((unsigned)n), dim3(256), 0, s, (const uint8_t*)slots, g.slot_stride,
                       (const int32_t*)lens, offs, g.intervals, scan, frame_stride, scan_bytes);
    return check_launch("jpeg_scan (pack)");
}

}  // extern "C"
