// The part of PNG that is not DEFLATE, on the GPU: undoing the five scanline filters (RFC 2083 section 6) of many images in
// one launch, and turning the reconstructed samples of every colour type, bit depth and interlace form into the 8-bit
// B, G, R pixels `cv2.imread` returns (`python -m acimg.convert_collected`).  Integer arithmetic on
// bytes, no atomics: every output byte is a function of the input alone.  tests/png_decode_ref.py restates both stages.
//
// png_unfilter_kernel.  One wave per job (a job is one file, or one Adam7 pass of one).  Byte x of row r needs
//   (r, x - bpp), (r - 1, x) and (r - 1, x - bpp), so the wave runs a WAVEFRONT over a band of up to 64 consecutive rows:
//   lane l owns row band + l and at step t reconstructs filter unit t - l of it (a unit is the bpp bytes one pixel back
//   refers to).  `up` is the unit lane l - 1 produced one step earlier: ONE cross-lane move (__shfl_up) of the unit's one
//   or two dwords per step; `upleft` is the `up` of the step before and `left` the lane's own last unit, both registers.
//   A band of 64 rows costs units + 63 steps; a job of R rows costs ceil(R / 64) (units + 63), never R * units, and the
//   jobs of a launch run side by side on the card's CUs.
//   The filter type differs from lane to lane: the five predictors are computed by select, the only branches are the
//   lane's activity (its unit lies inside its row) and the block-uniform choice of bpp.
//   Loads: the lanes are staggered, so a lane's bytes have no common alignment; each lane fetches the raw bytes of its
//   next PNG_CHUNK units with byte loads issued back to back (one latency per chunk, not per step) and keeps them in
//   registers.  Stores are byte stores as the units are produced.
//   Hand-over.  A band's first row needs the last row of the band before it.  It goes through the OUTPUT BUFFER: lane 63
//   has stored that row, the workgroup (this one wave) passes __syncthreads() between two bands - a barrier with a
//   workgroup-scope release / acquire of global memory - and lane 0 then fetches its `up` units from dst with the same
//   chunked loads.  That is safe because writer and reader are the same workgroup, no other workgroup writes the rows of
//   this job, and it needs no LDS, so a row may have any length.
//   A filter byte above 4 stores ACIMG_PNG_BAD_FILTER to the file's status (a plain store: every writer stores the same
//   value) and is decoded as filter 0, so the file's bytes stay inside its extent and no other file is touched.
// png_pixels_kernel.  One lane per output pixel, grid.y = the file: the pass and the position inside it from the Adam7
//   table, the sample from the pass's packed rows (MSB first below 8 bits, the high byte of 16), PLTE / grey scaling /
//   replication, alpha dropped, B G R stored.
#include <vector>

#include "common.hpp"

namespace acimg {

constexpr int PNG_JOB_FIELDS = ACIMG_PNG_JOB_FIELDS, PNG_FILE_FIELDS = ACIMG_PNG_FILE_FIELDS;
constexpr long PNG_MAX_BYTES = 2147483647L;
constexpr int PNG_PIXEL_THREADS = 256;

struct PngJob {
    long src_off, dst_off, rows, row_bytes, bpp, file;
};
struct PngFile {
    long sample_off, height, width, colour_type, bit_depth, interlace, palette_off, palette_len, out_off;
};
static_assert(sizeof(PngJob) == PNG_JOB_FIELDS * sizeof(long) && sizeof(PngFile) == PNG_FILE_FIELDS * sizeof(long), "table rows");

__host__ __device__ constexpr int png_adam7_x0(int p) { return p == 1 ? 4 : p == 3 ? 2 : p == 5 ? 1 : 0; }
__host__ __device__ constexpr int png_adam7_dx(int p) { return p < 2 ? 8 : p < 4 ? 4 : p < 6 ? 2 : 1; }
__host__ __device__ constexpr int png_adam7_y0(int p) { return p == 2 ? 4 : p == 4 ? 2 : p == 6 ? 1 : 0; }
__host__ __device__ constexpr int png_adam7_dy(int p) { return p < 3 ? 8 : p < 5 ? 4 : p < 7 ? 2 : 1; }
static_assert(png_adam7_dy(6) == 2 && png_adam7_dy(4) == 4 && png_adam7_dy(2) == 8 && png_adam7_dx(6) == 1, "Adam7");

__host__ __device__ inline int png_channels(int colour_type) {
    return colour_type == 0 || colour_type == 3 ? 1 : colour_type == 2 ? 3 : colour_type == 4 ? 2 : 4;
}
__host__ __device__ inline long png_row_bytes(long width, int colour_type, int bit_depth) {
    return (width * png_channels(colour_type) * bit_depth + 7) / 8;
}

static bool png_form_ok(int colour_type, int bit_depth) {
    switch (colour_type) {
        case 0: return bit_depth == 1 || bit_depth == 2 || bit_depth == 4 || bit_depth == 8 || bit_depth == 16;
        case 3: return bit_depth == 1 || bit_depth == 2 || bit_depth == 4 || bit_depth == 8;
        case 2: case 4: case 6: return bit_depth == 8 || bit_depth == 16;
        default: return false;
    }
}

// bytes of the file's passes: rows * (row bytes + filter) each; 0 when out of range
static size_t png_extent(int height, int width, int colour_type, int bit_depth, int interlace, int filter) {
    if (height < 1 || width < 1 || !png_form_ok(colour_type, bit_depth) || interlace < 0 || interlace > 1) return 0;
    unsigned long total = 0;
    for (int p = 0; p < (interlace ? 7 : 1); ++p) {
        const long ph = interlace ? (height - png_adam7_y0(p) + png_adam7_dy(p) - 1) / png_adam7_dy(p) : height;
        const long pw = interlace ? (width - png_adam7_x0(p) + png_adam7_dx(p) - 1) / png_adam7_dx(p) : width;
        if (ph < 1 || pw < 1) continue;
        total += (unsigned long)ph * (unsigned long)(png_row_bytes(pw, colour_type, bit_depth) + filter);
        if (total > (unsigned long)PNG_MAX_BYTES) return 0;
    }
    return (size_t)total;
}

// ---- the filters ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int png_predict(int ft, int a, int b, int c) {
    const int p = a + b - c;
    const int pa = abs(p - a), pb = abs(p - b), pc = abs(p - c);
    const int paeth = (pa <= pb && pa <= pc) ? a : (pb <= pc ? b : c);
    int v = 0;
    v = ft == 1 ? a : v;
    v = ft == 2 ? b : v;
    v = ft == 3 ? (a + b) >> 1 : v;
    v = ft == 4 ? paeth : v;
    return v;
}

template <int BPP>
struct PngUnit {                                  // the BPP bytes of one filter unit in one or two dwords
    static constexpr int W = (BPP + 3) / 4;
    uint32_t w[W];
    __device__ __forceinline__ void clear() {
#pragma unroll
        for (int i = 0; i < W; ++i) w[i] = 0;
    }
    __device__ __forceinline__ int get(int j) const { return (int)((w[j >> 2] >> (8 * (j & 3))) & 255u); }
    __device__ __forceinline__ void put(int j, int v) { w[j >> 2] |= (uint32_t)(v & 255) << (8 * (j & 3)); }
};

template <int BPP>
__device__ __forceinline__ void png_unfilter_job(const uint8_t* __restrict__ src, uint8_t* dst, const PngJob job, int32_t* status) {
    constexpr int CHUNK = BPP <= 1 ? 32 : BPP <= 2 ? 16 : BPP <= 4 ? 8 : 4;     // units a lane fetches at once
    const int lane = threadIdx.x;
    const long rows = job.rows, row_bytes = job.row_bytes, units = row_bytes / BPP;
    for (long band = 0; band < rows; band += 64) {
        if (band) __syncthreads();                // the band before has stored its last row: lane 0 reads it from dst
        const long r = band + lane;
        const bool valid = r < rows;
        const uint8_t* in = src + job.src_off + (valid ? r : 0) * (row_bytes + 1);
        uint8_t* out = dst + job.dst_off + (valid ? r : 0) * row_bytes;
        const uint8_t* above = dst + job.dst_off + (band ? band - 1 : 0) * row_bytes;     // lane 0's `up` row, band > 0
        int ft = valid ? (int)in[0] : 0;
        if (ft > 4) {
            status[job.file] = ACIMG_PNG_BAD_FILTER;
            ft = 0;
        }
        const bool from_dst = lane == 0 && band > 0;
        const bool first_row = r == 0;
        const long live = rows - band < 64 ? rows - band : 64;      // rows of this band
        PngUnit<BPP> cur, up, left;
        cur.clear();
        up.clear();
        left.clear();
        const long steps = units + live - 1;
        for (long t0 = 0; t0 < steps; t0 += CHUNK) {
            const long x0 = t0 - lane;
            uint8_t raw[CHUNK * BPP], prev[CHUNK * BPP];
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) {
                const long x = x0 + k;
                const bool on = valid && x >= 0 && x < units;
#pragma unroll
                for (int j = 0; j < BPP; ++j) {
                    raw[k * BPP + j] = on ? in[1 + x * BPP + j] : (uint8_t)0;
                    prev[k * BPP + j] = (on && from_dst) ? above[x * BPP + j] : (uint8_t)0;
                }
            }
#pragma unroll
            for (int k = 0; k < CHUNK; ++k) {
                const long x = x0 + k;
                const bool on = valid && x >= 0 && x < units;
                // what lane l - 1 produced one step ago is this lane's `up`; the `up` of one step ago is its `upleft`
                PngUnit<BPP> upleft = up;
#pragma unroll
                for (int i = 0; i < PngUnit<BPP>::W; ++i) up.w[i] = __shfl_up(cur.w[i], 1);
                if (from_dst) {
                    up.clear();
#pragma unroll
                    for (int j = 0; j < BPP; ++j) up.put(j, prev[k * BPP + j]);
                }
                if (first_row) up.clear();
                if (x == 0 || first_row) upleft.clear();
                if (x == 0) left.clear();
                if (on) {
                    PngUnit<BPP> now;
                    now.clear();
#pragma unroll
                    for (int j = 0; j < BPP; ++j) {
                        const int v = (raw[k * BPP + j] + png_predict(ft, left.get(j), up.get(j), upleft.get(j))) & 255;
                        now.put(j, v);
                        out[x * BPP + j] = (uint8_t)v;
                    }
                    cur = now;
                    left = now;
                }
            }
        }
    }
}

__global__ __launch_bounds__(64) void png_unfilter_kernel(const uint8_t* __restrict__ src, uint8_t* dst,
                                                          const PngJob* __restrict__ jobs, int32_t* status) {
    const PngJob job = jobs[blockIdx.x];
    switch ((int)job.bpp) {                       // block-uniform
        case 1: png_unfilter_job<1>(src, dst, job, status); break;
        case 2: png_unfilter_job<2>(src, dst, job, status); break;
        case 3: png_unfilter_job<3>(src, dst, job, status); break;
        case 4: png_unfilter_job<4>(src, dst, job, status); break;
        case 6: png_unfilter_job<6>(src, dst, job, status); break;
        default: png_unfilter_job<8>(src, dst, job, status); break;
    }
}

// ---- samples -> B, G, R ----------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(PNG_PIXEL_THREADS) void png_pixels_kernel(const uint8_t* __restrict__ samples,
                                                                       const PngFile* __restrict__ files,
                                                                       const uint8_t* __restrict__ palette,
                                                                       uint8_t* __restrict__ out, int32_t* status) {
    const PngFile f = files[blockIdx.y];
    const long pixels = f.height * f.width;
    const int ct = (int)f.colour_type, depth = (int)f.bit_depth;
    const int channels = png_channels(ct);
    for (long i = (long)blockIdx.x * PNG_PIXEL_THREADS + threadIdx.x; i < pixels; i += (long)gridDim.x * PNG_PIXEL_THREADS) {
        const long y = i / f.width, x = i - y * f.width;
        long row_off = 0, px = x, pw = f.width;   // the pass's first byte, the pixel's column and the pass's width
        if (f.interlace) {
            int pass = 6;
            if ((y & 7) == 0 && (x & 7) == 0) pass = 0;
            else if ((y & 7) == 0 && (x & 7) == 4) pass = 1;
            else if ((y & 7) == 4 && (x & 3) == 0) pass = 2;
            else if ((y & 3) == 0 && (x & 3) == 2) pass = 3;
            else if ((y & 3) == 2 && (x & 1) == 0) pass = 4;
            else if ((y & 1) == 0 && (x & 1) == 1) pass = 5;
            for (int p = 0; p < pass; ++p) {
                const long ph = (f.height - png_adam7_y0(p) + png_adam7_dy(p) - 1) / png_adam7_dy(p);
                const long qw = (f.width - png_adam7_x0(p) + png_adam7_dx(p) - 1) / png_adam7_dx(p);
                if (ph > 0 && qw > 0) row_off += ph * png_row_bytes(qw, ct, depth);
            }
            pw = (f.width - png_adam7_x0(pass) + png_adam7_dx(pass) - 1) / png_adam7_dx(pass);
            px = (x - png_adam7_x0(pass)) / png_adam7_dx(pass);
            row_off += ((y - png_adam7_y0(pass)) / png_adam7_dy(pass)) * png_row_bytes(pw, ct, depth);
        } else {
            row_off = y * png_row_bytes(pw, ct, depth);
        }
        const uint8_t* row = samples + f.sample_off + row_off;
        int c0, c1, c2;                           // R, G, B
        if (depth >= 8) {
            const int step = depth >> 3;          // 16-bit samples are big-endian: the high byte comes first
            const uint8_t* s = row + px * channels * step;
            c0 = s[0];
            c1 = channels >= 3 ? s[step] : c0;
            c2 = channels >= 3 ? s[2 * step] : c0;
        } else {
            const long bit = px * depth;
            c0 = (row[bit >> 3] >> (8 - depth - (int)(bit & 7))) & ((1 << depth) - 1);
            if (ct == 0) c0 *= depth == 1 ? 255 : depth == 2 ? 85 : 17;
            c1 = c2 = c0;
        }
        if (ct == 3) {
            if (c0 < f.palette_len) {
                const uint8_t* e = palette + f.palette_off + 3 * c0;
                c0 = e[0];
                c1 = e[1];
                c2 = e[2];
            } else {
                status[blockIdx.y] = ACIMG_PNG_BAD_INDEX;
                c0 = c1 = c2 = 0;
            }
        }
        uint8_t* o = out + f.out_off + 3 * i;
        o[0] = (uint8_t)c2;
        o[1] = (uint8_t)c1;
        o[2] = (uint8_t)c0;
    }
}

static size_t png_align16(size_t n) { return (n + 15) & ~(size_t)15; }

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_png_inflated_bytes(int height, int width, int colour_type, int bit_depth, int interlace) {
    return png_extent(height, width, colour_type, bit_depth, interlace, 1);
}

size_t acimg_png_sample_bytes(int height, int width, int colour_type, int bit_depth, int interlace) {
    return png_extent(height, width, colour_type, bit_depth, interlace, 0);
}

size_t acimg_png_pixel_bytes(int height, int width) {
    if (height < 1 || width < 1 || (long)height * width > PNG_MAX_BYTES / 3) return 0;
    return (size_t)height * (size_t)width * 3;
}

size_t acimg_png_unfilter_workspace(int njobs) {
    if (njobs < 1) return 0;
    return png_align16((size_t)njobs * sizeof(PngJob));
}

int acimg_png_unfilter(const uint8_t* src, size_t src_bytes, const long* jobs, int njobs, int nfiles, uint8_t* dst, size_t dst_bytes,
                       int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    if (!src || !jobs || !dst || !status || !ws) return fail(ACIMG_EINVAL, "png_unfilter: null argument");
    if (njobs < 1 || nfiles < 1) return fail(ACIMG_EINVAL, "png_unfilter: %d jobs of %d files", njobs, nfiles);
    if (!aligned16(ws)) return fail(ACIMG_EINVAL, "png_unfilter: ws must be 16-byte aligned");
    const size_t need = acimg_png_unfilter_workspace(njobs);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "png_unfilter: workspace %zu < %zu bytes", ws_bytes, need);
    for (int i = 0; i < njobs; ++i) {
        const long* j = jobs + (size_t)i * PNG_JOB_FIELDS;
        const long so = j[0], d = j[1], rows = j[2], rb = j[3], bpp = j[4], file = j[5];
        if (!(bpp == 1 || bpp == 2 || bpp == 3 || bpp == 4 || bpp == 6 || bpp == 8))
            return fail(ACIMG_EINVAL, "png_unfilter: job %d has a filter unit of %ld bytes", i, bpp);
        if (rows < 1 || rb < 1 || rb % bpp || rows > PNG_MAX_BYTES / (rb + 1))
            return fail(ACIMG_EINVAL, "png_unfilter: job %d has %ld rows of %ld bytes (unit %ld)", i, rows, rb, bpp);
        if (file < 0 || file >= nfiles) return fail(ACIMG_EINVAL, "png_unfilter: job %d names file %ld of %d", i, file, nfiles);
        if (so < 0 || (size_t)so > src_bytes || (size_t)(rows * (rb + 1)) > src_bytes - (size_t)so)
            return fail(ACIMG_EINVAL, "png_unfilter: job %d reads %ld bytes at %ld of %zu", i, rows * (rb + 1), so, src_bytes);
        if (d < 0 || (size_t)d > dst_bytes || (size_t)(rows * rb) > dst_bytes - (size_t)d)
            return fail(ACIMG_EINVAL, "png_unfilter: job %d writes %ld bytes at %ld of %zu", i, rows * rb, d, dst_bytes);
    }
    hipStream_t s = (hipStream_t)stream;
    // the table is host memory of this call: it has reached the device before the call returns
    hipError_t e = hipMemcpyAsync(ws, jobs, (size_t)njobs * sizeof(PngJob), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, (size_t)nfiles * sizeof(int32_t), s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "png_unfilter (table): %s", hipGetErrorString(e));
    hipLaunchKernelGGL(png_unfilter_kernel, dim3((unsigned)njobs), dim3(64), 0, s, src, dst, (const PngJob*)ws, status);
    return check_launch("png_unfilter");
}

size_t acimg_png_pixels_workspace(int nfiles) {
    if (nfiles < 1) return 0;
    return png_align16((size_t)nfiles * sizeof(PngFile));
}

int acimg_png_pixels(const uint8_t* samples, size_t sample_bytes, const long* files, int nfiles, const uint8_t* palette,
                     size_t palette_bytes, uint8_t* out, size_t out_bytes, int32_t* status, void* ws, size_t ws_bytes, void* stream) {
    if (!samples || !files || !out || !status || !ws) return fail(ACIMG_EINVAL, "png_pixels: null argument");
    if (nfiles < 1 || nfiles > 65535) return fail(ACIMG_EINVAL, "png_pixels: %d files, 1 .. 65535 go into one launch", nfiles);
    if (!aligned16(ws)) return fail(ACIMG_EINVAL, "png_pixels: ws must be 16-byte aligned");
    const size_t need = acimg_png_pixels_workspace(nfiles);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "png_pixels: workspace %zu < %zu bytes", ws_bytes, need);
    long most = 0;
    for (int i = 0; i < nfiles; ++i) {
        const long* f = files + (size_t)i * PNG_FILE_FIELDS;
        const long so = f[0], h = f[1], w = f[2], ct = f[3], depth = f[4], il = f[5], po = f[6], pl = f[7], oo = f[8];
        if (h < 1 || w < 1 || h > INT32_MAX || w > INT32_MAX)
            return fail(ACIMG_EINVAL, "png_pixels: file %d is %ld x %ld", i, h, w);
        const size_t sb = acimg_png_sample_bytes((int)h, (int)w, (int)ct, (int)depth, (int)il), pb = acimg_png_pixel_bytes((int)h, (int)w);
        if (!sb || !pb)
            return fail(ACIMG_EINVAL, "png_pixels: file %d: %ld x %ld of colour type %ld, depth %ld, interlace %ld is no PNG form in range",
                        i, h, w, ct, depth, il);
        if (so < 0 || (size_t)so > sample_bytes || sb > sample_bytes - (size_t)so)
            return fail(ACIMG_EINVAL, "png_pixels: file %d reads %zu bytes at %ld of %zu", i, sb, so, sample_bytes);
        if (oo < 0 || (size_t)oo > out_bytes || pb > out_bytes - (size_t)oo)
            return fail(ACIMG_EINVAL, "png_pixels: file %d writes %zu bytes at %ld of %zu", i, pb, oo, out_bytes);
        if (ct == 3 && (!palette || pl < 1 || pl > 256 || po < 0 || (size_t)po > palette_bytes || (size_t)(3 * pl) > palette_bytes - (size_t)po))
            return fail(ACIMG_EINVAL, "png_pixels: file %d has a palette of %ld entries at %ld of %zu bytes", i, pl, po, palette_bytes);
        if (h * w > most) most = h * w;
    }
    hipStream_t s = (hipStream_t)stream;
    // the table is host memory of this call: it has reached the device before the call returns
    hipError_t e = hipMemcpyAsync(ws, files, (size_t)nfiles * sizeof(PngFile), hipMemcpyHostToDevice, s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) return fail(ACIMG_ELAUNCH, "png_pixels (table): %s", hipGetErrorString(e));
    static_assert(PNG_PIXEL_THREADS == 256, "clamped_blocks counts workgroups of 256");
    const int gx = clamped_blocks(most, 1024);
    hipLaunchKernelGGL(png_pixels_kernel, dim3((unsigned)gx, (unsigned)nfiles), dim3(PNG_PIXEL_THREADS), 0, s, samples,
                       (const PngFile*)ws, palette, out, status);
    return check_launch("png_pixels");
}

}  // extern "C"
