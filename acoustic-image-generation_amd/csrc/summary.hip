// TensorBoard summaries on the GPU: the two reductions that turn device tensors into summary values without a copy of
// the tensors to the host (include/acimg.h spells both rules out).
//
// acimg_summary_images: tf.summary.image on float input.  One launch, one workgroup per (image, channel group): a min /
// max reduction over the finite values of the group's H*W*3 slice (order-free: the same value in any order), then the
// store pass.  No atomics, no workspace.  This file is compiled with contraction off, so v * scale + offset is an fp32
// multiply followed by an fp32 add.
//
// acimg_histogram_segments: TF's summary histogram of V boxes of one flat fp32 buffer.  Three launches:
//   0. zero counts / nonfinite; one thread turns the segment table into a prefix of CHUNK-element chunks (workspace)
//   1. every workgroup takes a contiguous run of chunks: 16-byte loads where the segment allows them, the coordinates of
//      a 4-vector decoded once, the bucket found through a 4096-entry table keyed by the value's sign, exponent and top
//      three mantissa bits (the first candidate bucket of that key) and corrected against the limits in LDS; counters
//      privatised in LDS and flushed with 64-bit integer atomics when the segment changes (integer adds: exact in any
//      order); {min, max, sum, sum_squares} of every chunk reduced in a fixed order and left in the workspace
//   2. one workgroup per segment sums its chunks' records in a fixed order.
// No floating atomics: two runs are bit-equal.
#include "common.hpp"

#include <cfloat>

#pragma clang fp contract(off)

namespace acimg {

// ---- images -----------------------------------------------------------------------------------------------------------
__device__ __forceinline__ bool finite_f(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

__global__ __launch_bounds__(256) void summary_images_kernel(const float* x, int ldc, long HW, int c0, int G,
                                                             uint8_t* out) {
    __shared__ float smin[4], smax[4];
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const long slice = blockIdx.x;                  // n * G + g
    const long n = slice / G;
    const int g = (int)(slice - n * G);
    const float* src = x + n * HW * (long)ldc + c0 + 3 * g;
    float lo = __builtin_inff(), hi = -__builtin_inff();
    for (long p = tid; p < HW; p += 256) {
        const float* px = src + p * ldc;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            const float v = px[k];
            if (finite_f(v)) {
                lo = fminf(lo, v);
                hi = fmaxf(hi, v);
            }
        }
    }
    lo = wave_min(lo);
    hi = wave_max(hi);
    if (lane == 0) {
        smin[wid] = lo;
        smax[wid] = hi;
    }
    __syncthreads();
    const float image_min = fminf(fminf(smin[0], smin[1]), fminf(smin[2], smin[3]));
    const float image_max = fmaxf(fmaxf(smax[0], smax[1]), fmaxf(smax[2], smax[3]));
    float scale, offset;
    if (image_min < 0.f) {
        const float m = fmaxf(fabsf(image_min), fabsf(image_max));
        scale = m < 1e-6f ? 0.f : 127.f / m;
        offset = 128.f;
    } else {
        scale = image_max < 1e-6f ? 0.f : 255.f / image_max;
        offset = 0.f;
    }
    uint8_t* dst = out + slice * HW * 3;
    for (long p = tid; p < HW; p += 256) {
        const float* px = src + p * ldc;
        const float v0 = px[0], v1 = px[1], v2 = px[2];
        uint8_t b0 = 255, b1 = 0, b2 = 0;
        if (finite_f(v0) && finite_f(v1) && finite_f(v2)) {
            const float q0 = v0 * scale, q1 = v1 * scale, q2 = v2 * scale;
            int i0 = (int)(q0 + offset), i1 = (int)(q1 + offset), i2 = (int)(q2 + offset);
            b0 = (uint8_t)(i0 < 0 ? 0 : (i0 > 255 ? 255 : i0));
            b1 = (uint8_t)(i1 < 0 ? 0 : (i1 > 255 ? 255 : i1));
            b2 = (uint8_t)(i2 < 0 ? 0 : (i2 > 255 ? 255 : i2));
        }
        dst[p * 3 + 0] = b0;
        dst[p * 3 + 1] = b1;
        dst[p * 3 + 2] = b2;
    }
}

// ---- histograms -------------------------------------------------------------------------------------------------------
constexpr int HIST_THREADS = 512;
constexpr long HIST_CHUNK = 8192;          // elements per chunk: 4 float4 loads per thread
constexpr int HIST_GRID = 512;             // workgroups of launch 1 at most: one sweep = HIST_GRID * HIST_CHUNK elements
constexpr int HIST_MAX_L = 4096;           // limits + counters + key table: 56 KiB of LDS at most
constexpr int HIST_KEYS = 4096;            // sign, exponent, three mantissa bits
constexpr int HIST_FLUSH_CHUNKS = 65536;   // a workgroup's 32-bit counters are flushed before they can wrap
constexpr int SEG_WORDS = 13;              // offset, dims[4], lo[4], hi[4]

struct ChunkStats {
    double mn, mx, sum, sq;
};
static_assert(sizeof(ChunkStats) == 32, "workspace record");

struct Segment {
    long offset, numel;
    long d1, d2, d3;       // dims 1..3 (dim 0 is numel / (d1 * d2 * d3))
    long lo[4], hi[4];
};

__device__ __forceinline__ Segment load_segment(const int64_t* table, int v) {
    const int64_t* s = table + (long)v * SEG_WORDS;
    Segment g;
    g.offset = s[0];
    const long d0 = s[1];
    g.d1 = s[2];
    g.d2 = s[3];
    g.d3 = s[4];
    const bool ok = d0 > 0 && g.d1 > 0 && g.d2 > 0 && g.d3 > 0 && g.offset >= 0;
    g.numel = ok ? d0 * g.d1 * g.d2 * g.d3 : 0;
    if (!ok) g.d1 = g.d2 = g.d3 = 1;
    long d[4] = {d0, g.d1, g.d2, g.d3}, lo[4], hi[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lo[k] = s[5 + k] < 0 ? 0 : s[5 + k];
        hi[k] = s[9 + k] > d[k] ? d[k] : s[9 + k];
    }
    // unused trailing dims (1) move to the front, so that the fastest dim is a real one and its rows take 16-byte loads;
    // a unit dim whose box does not hold coordinate 0 keeps the segment empty through the dim that takes its place
    for (int r = 0; r < 3 && d[3] == 1; ++r) {
        const bool open = lo[3] <= 0 && hi[3] >= 1;
        for (int k = 3; k > 0; --k) {
            d[k] = d[k - 1];
            lo[k] = lo[k - 1];
            hi[k] = hi[k - 1];
        }
        d[0] = 1;
        lo[0] = open ? 0 : 1;
        hi[0] = 1;
    }
    g.d1 = d[1];
    g.d2 = d[2];
    g.d3 = d[3];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        g.lo[k] = lo[k];
        g.hi[k] = hi[k];
    }
    return g;
}

__device__ __forceinline__ long segment_chunks(const int64_t* table, int v) {
    const int64_t* s = table + (long)v * SEG_WORDS;
    if (s[0] < 0 || s[1] <= 0 || s[2] <= 0 || s[3] <= 0 || s[4] <= 0) return 0;
    const long numel = s[1] * s[2] * s[3] * s[4];
    return (numel + HIST_CHUNK - 1) / HIST_CHUNK;
}

// launch 0: zero the counters; chunk prefix of the segment table, clamped to the capacity the host sized the workspace for
__global__ __launch_bounds__(256) void hist_prepare_kernel(const int64_t* table, int V, int L, long cap, long* prefix,
                                                           unsigned long long* counts, unsigned long long* nonfinite) {
    const long total = (long)V * L;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) counts[i] = 0ull;
    if (blockIdx.x == 0) {
        for (int v = threadIdx.x; v < V; v += 256) nonfinite[v] = 0ull;
        if (threadIdx.x == 0) {
            long acc = 0;
            prefix[0] = 0;
            for (int v = 0; v < V; ++v) {
                acc += segment_chunks(table, v);
                if (acc > cap) acc = cap;      // a table larger than the caller promised: the excess is not read
                prefix[v + 1] = acc;
            }
        }
    }
}

// index of the first limit greater than d, at most L - 1
__device__ __forceinline__ int upper_bound_lds(const double* lim, int L, double d) {
    int lo = 0, n = L;
    while (n > 0) {
        const int half = n >> 1;
        if (!(d < lim[lo + half])) {
            lo += half + 1;
            n -= half + 1;
        } else {
            n = half;
        }
    }
    return lo < L ? lo : L - 1;
}

struct ThreadStats {
    double mn, mx, sum, sq;
    unsigned bad;
};

__device__ __forceinline__ void count_value(float v, const double* lim, const unsigned short* key, unsigned* cnt, int L,
                                            ThreadStats& st) {
    const unsigned bits = __float_as_uint(v);
    if ((bits & 0x7f800000u) == 0x7f800000u) {
        st.bad += 1u;
        return;
    }
    const double d = (double)v;
#ifdef ACIMG_HIST_BSEARCH
    const int b = upper_bound_lds(lim, L, d);
#else
    int b = key[bits >> 20];
    while (b < L - 1 && !(d < lim[b])) ++b;
#endif
    atomicAdd(&cnt[b], 1u);
    st.mn = fmin(st.mn, d);
    st.mx = fmax(st.mx, d);
    st.sum += d;
    st.sq += d * d;
}

template <typename I>
__device__ __forceinline__ void decode(I e, I d1, I d2, I d3, long* c) {
    const I r3 = e / d3;
    c[3] = (long)(e - r3 * d3);
    const I r2 = r3 / d2;
    c[2] = (long)(r3 - r2 * d2);
    const I r1 = r2 / d1;
    c[1] = (long)(r2 - r1 * d1);
    c[0] = (long)r1;
}

__device__ __forceinline__ void decode_any(long e, const Segment& g, bool small, long* c) {
    if (small)
        decode<unsigned>((unsigned)e, (unsigned)g.d1, (unsigned)g.d2, (unsigned)g.d3, c);
    else
        decode<long>(e, g.d1, g.d2, g.d3, c);
}

__global__ __launch_bounds__(HIST_THREADS) void hist_partial_kernel(const float* base, const int64_t* table, int V,
                                                                    const double* limits, int L, const long* prefix,
                                                                    ChunkStats* chunk_stats, unsigned long long* counts,
                                                                    unsigned long long* nonfinite) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* lim = reinterpret_cast<double*>(smem);
    unsigned* cnt = reinterpret_cast<unsigned*>(lim + L);
    unsigned short* key = reinterpret_cast<unsigned short*>(cnt + L);
    __shared__ double red[4][HIST_THREADS / 64];
    __shared__ unsigned redbad[HIST_THREADS / 64];
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const long T = prefix[V];
    const long per = (T + gridDim.x - 1) / gridDim.x;
    const long c_lo = (long)blockIdx.x * per;
    const long c_hi = c_lo + per < T ? c_lo + per : T;
    if (c_lo >= c_hi) return;
    for (int i = tid; i < L; i += HIST_THREADS) {
        lim[i] = limits[i];
        cnt[i] = 0u;
    }
    __syncthreads();
#ifndef ACIMG_HIST_BSEARCH
    // key table: the bucket of the smallest value that has the key (finite keys only; the others are never looked up)
    for (int k = tid; k < HIST_KEYS; k += HIST_THREADS) {
        const unsigned low = (k & 0x800) ? (((unsigned)k << 20) | 0xfffffu) : ((unsigned)k << 20);
        int b = 0;
        if (((k >> 3) & 0xff) != 0xff) b = upper_bound_lds(lim, L, (double)__uint_as_float(low));
        key[k] = (unsigned short)b;
    }
    __syncthreads();
#endif
    // the segment of the first chunk: the last v with prefix[v] <= c_lo
    int v = 0;
    {
        int lo = 0, hi = V;      // prefix[lo] <= c_lo < prefix[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) >> 1;
            if (prefix[mid] <= c_lo) lo = mid; else hi = mid;
        }
        v = lo;
    }
    Segment g = load_segment(table, v);
    unsigned bad_run = 0;
    int since_flush = 0;
    for (long c = c_lo; c < c_hi; ++c) {
        bool moved = false;
        int v_new = v;
        while (c >= prefix[v_new + 1]) ++v_new;      // c < T = prefix[V]: ends at v_new < V
        moved = v_new != v;
        if (moved || since_flush >= HIST_FLUSH_CHUNKS) {
            // flush the private counters into segment v's row (block-uniform branch)
            __syncthreads();
            for (int i = tid; i < L; i += HIST_THREADS) {
                const unsigned k = cnt[i];
                if (k) {
                    atomicAdd(&counts[(long)v * L + i], (unsigned long long)k);
                    cnt[i] = 0u;
                }
            }
            if (tid == 0 && bad_run) atomicAdd(&nonfinite[v], (unsigned long long)bad_run);
            bad_run = 0;
            since_flush = 0;
            __syncthreads();
            if (moved) {
                v = v_new;
                g = load_segment(table, v);
            }
        }
        ++since_flush;
        const long e0 = (c - prefix[v]) * HIST_CHUNK;
        const long e1 = e0 + HIST_CHUNK < g.numel ? e0 + HIST_CHUNK : g.numel;
        const float* src = base + g.offset;
        const bool small = g.numel <= 0xffffffffl;
        const bool vec = (g.d3 & 3) == 0 && (reinterpret_cast<uintptr_t>(src) & 15u) == 0;
        ThreadStats st = {__builtin_inf(), -__builtin_inf(), 0.0, 0.0, 0u};
        for (long e = e0 + (long)tid * 4; e < e1; e += (long)HIST_THREADS * 4) {
            long cd[4];
            if (vec) {      // e % 4 == 0 and d3 % 4 == 0: the four elements share a row and e + 3 < numel
                decode_any(e, g, small, cd);
                const bool row = cd[0] >= g.lo[0] && cd[0] < g.hi[0] && cd[1] >= g.lo[1] && cd[1] < g.hi[1] &&
                                 cd[2] >= g.lo[2] && cd[2] < g.hi[2];
                if (row && cd[3] + 3 >= g.lo[3] && cd[3] < g.hi[3]) {      // vectors outside the box are not loaded
                    const float4 q = *reinterpret_cast<const float4*>(src + e);
                    const float qv[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (cd[3] + j >= g.lo[3] && cd[3] + j < g.hi[3]) count_value(qv[j], lim, key, cnt, L, st);
                }
            } else {
                for (int j = 0; j < 4 && e + j < e1; ++j) {
                    decode_any(e + j, g, small, cd);
                    const bool in = cd[0] >= g.lo[0] && cd[0] < g.hi[0] && cd[1] >= g.lo[1] && cd[1] < g.hi[1] &&
                                    cd[2] >= g.lo[2] && cd[2] < g.hi[2] && cd[3] >= g.lo[3] && cd[3] < g.hi[3];
                    if (in) count_value(src[e + j], lim, key, cnt, L, st);
                }
            }
        }
        // the chunk's record: lanes, then waves, in a fixed order
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            st.mn = fmin(st.mn, __shfl_xor(st.mn, o, 64));
            st.mx = fmax(st.mx, __shfl_xor(st.mx, o, 64));
            st.sum += __shfl_xor(st.sum, o, 64);
            st.sq += __shfl_xor(st.sq, o, 64);
            st.bad += __shfl_xor(st.bad, o, 64);
        }
        __syncthreads();      // the previous chunk's record has been read
        if (lane == 0) {
            red[0][wid] = st.mn;
            red[1][wid] = st.mx;
            red[2][wid] = st.sum;
            red[3][wid] = st.sq;
            redbad[wid] = st.bad;
        }
        __syncthreads();
        ChunkStats r = {red[0][0], red[1][0], red[2][0], red[3][0]};
        unsigned bad = redbad[0];
        for (int w = 1; w < HIST_THREADS / 64; ++w) {
            r.mn = fmin(r.mn, red[0][w]);
            r.mx = fmax(r.mx, red[1][w]);
            r.sum += red[2][w];
            r.sq += red[3][w];
            bad += redbad[w];
        }
        bad_run += bad;      // every thread keeps the same total; thread 0's copy is flushed
        if (tid == 0) chunk_stats[c] = r;
    }
    __syncthreads();
    for (int i = tid; i < L; i += HIST_THREADS) {
        const unsigned k = cnt[i];
        if (k) atomicAdd(&counts[(long)v * L + i], (unsigned long long)k);
    }
    if (tid == 0 && bad_run) atomicAdd(&nonfinite[v], (unsigned long long)bad_run);
}

// launch 2: segment v's chunk records, thread-strided then lanes then waves: a fixed order
__global__ __launch_bounds__(256) void hist_finish_kernel(int V, const long* prefix, const ChunkStats* chunk_stats,
                                                          double* stats) {
    __shared__ double red[4][4];
    const int tid = threadIdx.x, wid = tid >> 6, lane = tid & 63;
    const int v = blockIdx.x;
    double mn = __builtin_inf(), mx = -__builtin_inf(), sum = 0.0, sq = 0.0;
    for (long c = prefix[v] + tid; c < prefix[v + 1]; c += 256) {
        const ChunkStats r = chunk_stats[c];
        mn = fmin(mn, r.mn);
        mx = fmax(mx, r.mx);
        sum += r.sum;
        sq += r.sq;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        mn = fmin(mn, __shfl_xor(mn, o, 64));
        mx = fmax(mx, __shfl_xor(mx, o, 64));
        sum += __shfl_xor(sum, o, 64);
        sq += __shfl_xor(sq, o, 64);
    }
    if (lane == 0) {
        red[0][wid] = mn;
        red[1][wid] = mx;
        red[2][wid] = sum;
        red[3][wid] = sq;
    }
    __syncthreads();
    if (tid == 0) {
        double* o = stats + (long)v * 4;
        o[0] = fmin(fmin(red[0][0], red[0][1]), fmin(red[0][2], red[0][3]));
        o[1] = fmax(fmax(red[1][0], red[1][1]), fmax(red[1][2], red[1][3]));
        o[2] = ((red[2][0] + red[2][1]) + red[2][2]) + red[2][3];
        o[3] = ((red[3][0] + red[3][1]) + red[3][2]) + red[3][3];
    }
}

inline long hist_chunk_capacity(int V, long total_elements) { return total_elements / HIST_CHUNK + V; }
inline size_t hist_prefix_bytes(int V) { return (((size_t)V + 1) * sizeof(long) + 31) & ~(size_t)31; }

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_summary_images(const float* x, int ldc, long HW, int c0, int G, int n_images, uint8_t* out, void* stream) {
    if (!x || !out) return fail(ACIMG_EINVAL, "summary_images: null argument");
    if (HW <= 0 || G <= 0 || n_images <= 0)
        return fail(ACIMG_EINVAL, "summary_images: HW = %ld, G = %d, n_images = %d must be positive", HW, G, n_images);
    if (c0 < 0 || ldc <= 0 || (long)c0 + 3l * G > (long)ldc)
        return fail(ACIMG_EINVAL, "summary_images: channels %d .. %ld do not fit ldc = %d", c0, (long)c0 + 3l * G, ldc);
    if ((long)n_images * G > 0x7fffffffl)
        return fail(ACIMG_EINVAL, "summary_images: %d images x %d groups exceed the grid", n_images, G);
    hipLaunchKernelGGL(summary_images_kernel, dim3((unsigned)((long)n_images * G)), dim3(256), 0, (hipStream_t)stream, x,
                       ldc, HW, c0, G, out);
    return check_launch("summary_images");
}

size_t acimg_histogram_segments_workspace(int V, int L, long total_elements) {
    if (V <= 0 || L <= 0 || total_elements <= 0) return 0;
    return hist_prefix_bytes(V) + (size_t)hist_chunk_capacity(V, total_elements) * sizeof(ChunkStats);
}

int acimg_histogram_segments(const float* base, const int64_t* segments, int V, const double* limits, int L,
                             long total_elements, uint64_t* counts, double* stats, uint64_t* nonfinite, void* ws,
                             size_t ws_bytes, void* stream) {
    if (V <= 0 || L <= 0 || total_elements <= 0)
        return fail(ACIMG_EINVAL, "histogram_segments: V = %d, L = %d, total_elements = %ld must be positive", V, L,
                    total_elements);
    if (!base || !segments || !limits || !counts || !stats || !nonfinite || !ws)
        return fail(ACIMG_EINVAL, "histogram_segments: null argument");
    if (L > HIST_MAX_L) return fail(ACIMG_EINVAL, "histogram_segments: L = %d exceeds %d limits", L, HIST_MAX_L);
    if (reinterpret_cast<uintptr_t>(ws) & 7u) return fail(ACIMG_EINVAL, "histogram_segments: workspace not 8-byte aligned");
    const size_t need = acimg_histogram_segments_workspace(V, L, total_elements);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "histogram_segments: workspace %zu < %zu bytes", ws_bytes, need);
    hipStream_t s = (hipStream_t)stream;
    long* prefix = (long*)ws;
    ChunkStats* chunk_stats = (ChunkStats*)((char*)ws + hist_prefix_bytes(V));
    const long cap = hist_chunk_capacity(V, total_elements);
    unsigned long long* cnt = (unsigned long long*)counts;
    unsigned long long* bad = (unsigned long long*)nonfinite;
    const long cells = (long)V * L;
    const int zero_blocks = (int)(cells / 2048 + 1 < 1024 ? cells / 2048 + 1 : 1024);
    hipLaunchKernelGGL(hist_prepare_kernel, dim3(zero_blocks), dim3(256), 0, s, segments, V, L, cap, prefix, cnt, bad);
    int rc = check_launch("histogram_segments (prepare)");
    if (rc) return rc;
    const int grid = (int)(cap < HIST_GRID ? cap : HIST_GRID);
    const size_t lds = (size_t)L * (sizeof(double) + sizeof(unsigned)) + HIST_KEYS * sizeof(unsigned short);
    hipLaunchKernelGGL(hist_partial_kernel, dim3(grid), dim3(HIST_THREADS), lds, s, base, segments, V, limits, L, prefix,
                       chunk_stats, cnt, bad);
    rc = check_launch("histogram_segments (partial)");
    if (rc) return rc;
    hipLaunchKernelGGL(hist_finish_kernel, dim3(V), dim3(256), 0, s, V, prefix, chunk_stats, stats);
    return check_launch("histogram_segments (finish)");
}

}  // extern "C"
