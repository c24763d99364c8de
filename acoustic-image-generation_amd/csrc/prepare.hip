// Batch assembly for the device-resident record loader (acimg/data.py: DeviceDataLoader): the per-frame maps of
// dataloader/outdoor_data_mfcc.py:634-703 applied WHILE the frames of a batch are gathered out of a pool of decoded
// records, so that the video never exists as float32 on the host.
//
// Per output frame n < N, with s = slots[n]:
//   video    uint8 [pixels][3] in stored (BGR) order -> float32 [pixels][3] reversed, * (float)(1.0 / 255.0): ONE fp32
//            multiply per value, the arithmetic of `vi[..., ::-1].astype(np.float32) * np.float32(1.0 / 255.0)`;
//   acoustic float32 [elems] -> (a - min(a)) / max(a - min(a)), a correctly rounded subtraction and division (this file
//            is compiled with contraction off; there is no reciprocal): NumPy's result on finite input, NaN for a
//            constant frame (0 / 0) as NumPy gives;
//   the two MFCC rows copied; the two labels turned into one-hot float32 rows (a label outside the row: all zeros).
//
// Launches: TWO, both on the caller's stream, no atomics, every reduction in a fixed order.
//   1. batch_video_kernel, grid (tiles per frame, N), 256 threads.  A tile is 256 chunks of 48 bytes = 16 pixels: the
//      workgroup reads its 12 KiB with three 16-byte loads per thread at consecutive addresses (1 KiB per wave
//      instruction), parks them in LDS, and writes the 48 KiB of floats with twelve float4 stores per thread, again at
//      consecutive addresses; the channel reversal is four LDS byte reads per store.  Frames whose pixel count is no
//      multiple of 4 (their float rows are not 16-byte aligned) and the pixels past the last whole chunk go through
//      scalar tail workgroups of 4096 floats each.
//   2. batch_frame_kernel, grid N, 1024 threads: one workgroup per frame holds the acoustic image in LDS (20736 floats
//      = 82944 bytes for 36 x 48 x 12), so the pool is read once and the output written once; min, then max of the
//      differences, each as per-thread strided runs -> wave butterflies -> 16 wave values folded in index order (min
//      and max are exact, so the order only has to be fixed, not NumPy's).  The frame moves as float4 when elems is a
//      multiple of 4 and both images are 16-byte aligned, else float by float; four loads are in flight per thread.
//      The same workgroup copies the MFCC rows, writes the one-hot rows and leaves (min, max(a - min)) in the workspace.
//
// acimg_batch_gather_pairs (the correspondence pairs of outdoor_data_mfcc.py:888-928) is the same two launches over a list
// of ROW CODES: code >= 0 is the real row of slot code - everything above -, code < 0 the silent row of slot ~code: the
// same video and labels, the low-passed MFCC row as the MFCC row and, tiled over the pixels, as the acoustic image (not
// normalised).  The video kernel decodes the slot (template parameter); batch_pair_kernel takes batch_frame_kernel's
// place and shares its normalisation (frame_normalise), so a real row is the same arithmetic in the same order.
#include "common.hpp"

#pragma clang fp contract(off)

namespace acimg {

constexpr int GATHER_MFCC = 12;                 // floats per MFCC row
constexpr int GATHER_MAX_ELEMS = 32768;         // acoustic floats the LDS image holds (128 KiB of the CU's 160)
constexpr int VID_THREADS = 256;
constexpr int VID_TILE_BYTES = VID_THREADS * 48;
constexpr int VID_TAIL_FLOATS = 4096;

// floats [f0, f0 + count) of one frame, one at a time: out[f] = src[3 * (f / 3) + 2 - f % 3] / 255
__device__ __forceinline__ void video_scalar(const uint8_t* src, float* dst, long f0, long count, float k) {
    for (long i = threadIdx.x; i < count; i += VID_THREADS) {
        const long f = f0 + i, p = f / 3;
        const int c = (int)(f - 3 * p);
        dst[f] = (float)src[3 * p + 2 - c] * k;
    }
}

// the slot of a row code: code >= 0 is the real row of slot code, code < 0 the silent row of slot ~code
__device__ __forceinline__ int32_t code_slot(int32_t code) { return code < 0 ? ~code : code; }

// CODES: `slots` holds row codes (acimg_batch_gather_pairs); the video of a row is its slot's, whatever its kind
template <bool CODES>
__global__ __launch_bounds__(VID_THREADS) void batch_video_kernel(const uint8_t* pool, size_t stride, const int32_t* slots,
                                                                  long pixels, long chunks, int tiles, float* out) {
    __shared__ __attribute__((aligned(16))) uint8_t lds[VID_TILE_BYTES];
    const int tid = threadIdx.x, n = blockIdx.y;
    const uint8_t* src = pool + (size_t)(CODES ? code_slot(slots[n]) : slots[n]) * stride;
    float* dst = out + (long)n * pixels * 3;
    const float k = (float)(1.0 / 255.0);
    if ((int)blockIdx.x >= tiles) {              // scalar tail: the floats past the last whole chunk
        const long f0 = chunks * 48 + (long)(blockIdx.x - tiles) * VID_TAIL_FLOATS;
        const long left = pixels * 3 - f0;
        video_scalar(src, dst, f0, left < VID_TAIL_FLOATS ? left : VID_TAIL_FLOATS, k);
        return;
    }
    const long c0 = (long)blockIdx.x * VID_THREADS;                     // first chunk of this tile
    const int nch = (int)(chunks - c0 < VID_THREADS ? chunks - c0 : VID_THREADS);
    const int in16 = nch * 3, out16 = nch * 12;                         // 16-byte pieces in, float4 out
    const uint4* g = reinterpret_cast<const uint4*>(src + c0 * 48);
#pragma unroll
    for (int j = 0; j < 3; ++j) {
        const int q = j * VID_THREADS + tid;
        if (q < in16) reinterpret_cast<uint4*>(lds)[q] = g[q];
    }
    __syncthreads();
    float4* o = reinterpret_cast<float4*>(dst + c0 * 48);
#pragma unroll
    for (int j = 0; j < 12; ++j) {
        const int q = j * VID_THREADS + tid;
        if (q < out16) {
            float v[4];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int f = 4 * q + e, p = f / 3, c = f - 3 * p;      // the tile starts on a pixel boundary
                v[e] = (float)lds[3 * p + 2 - c] * k;
            }
            o[q] = make_float4(v[0], v[1], v[2], v[3]);
        }
    }
}

// block-wide min / max over 1024 threads in a fixed order; result valid in every thread
__device__ __forceinline__ float block_min16(float v, float* sm) {
    v = wave_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) r = fminf(r, sm[i]);
    return r;
}
__device__ __forceinline__ float block_max16(float v, float* sm) {
    v = wave_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    float r = sm[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) r = fmaxf(r, sm[i]);
    return r;
}

// a float or a float4 of the frame: the reductions' terms, the difference and the quotient per lane
__device__ __forceinline__ float lanes_min(float v) { return v; }
__device__ __forceinline__ float lanes_min(float4 v) { return fminf(fminf(v.x, v.y), fminf(v.z, v.w)); }
__device__ __forceinline__ float lanes_max(float v) { return v; }
__device__ __forceinline__ float lanes_max(float4 v) { return fmaxf(fmaxf(v.x, v.y), fmaxf(v.z, v.w)); }
__device__ __forceinline__ float lanes_sub(float v, float m) { return v - m; }
__device__ __forceinline__ float4 lanes_sub(float4 v, float m) { return make_float4(v.x - m, v.y - m, v.z - m, v.w - m); }
__device__ __forceinline__ float lanes_div(float v, float d) { return v / d; }
__device__ __forceinline__ float4 lanes_div(float4 v, float d) { return make_float4(v.x / d, v.y / d, v.z / d, v.w / d); }

// the min-max normalisation of one frame by the whole workgroup of 1024 threads: pool -> LDS -> out, in T = float or
// float4 pieces; leaves min(a) and max(a - min(a)) in every thread
template <typename T>
__device__ __forceinline__ void frame_normalise(const float* src, int elems, float* dst, float* frame_lds, float* sm,
                                                float& mn, float& mx) {
    T* frame = reinterpret_cast<T*>(frame_lds);
    const int tid = threadIdx.x;
    const int cnt = elems / (int)(sizeof(T) / sizeof(float));
    const T* a = reinterpret_cast<const T*>(src);
    mn = __builtin_inff();
    for (int i0 = tid; i0 < cnt; i0 += 4 * 1024) {       // four loads in flight per thread
        T v[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * 1024 < cnt) v[u] = a[i0 + u * 1024];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (i0 + u * 1024 < cnt) {
                frame[i0 + u * 1024] = v[u];
                mn = fminf(mn, lanes_min(v[u]));
            }
    }
    mn = block_min16(mn, sm);
    mx = -__builtin_inff();
    for (int i = tid; i < cnt; i += 1024) {       // every thread revisits the elements it wrote itself
        const T d = lanes_sub(frame[i], mn);
        frame[i] = d;
        mx = fmaxf(mx, lanes_max(d));
    }
    mx = block_max16(mx, sm);
    T* o = reinterpret_cast<T*>(dst);
    for (int i = tid; i < cnt; i += 1024) o[i] = lanes_div(frame[i], mx);
}

// the two one-hot rows of output row n from the labels of slot s
__device__ __forceinline__ void one_hot_rows(const int32_t* pool_labels, long s, int n, int A, int L, float* action,
                                             float* location) {
    const int tid = threadIdx.x;
    const int cls = pool_labels[2 * s], loc = pool_labels[2 * s + 1];
    for (int i = tid; i < A; i += 1024) action[(long)n * A + i] = i == cls ? 1.f : 0.f;
    for (int i = tid; i < L; i += 1024) location[(long)n * L + i] = i == loc ? 1.f : 0.f;
}

// T = float4 when elems % 4 == 0 and both images are 16-byte aligned, else float
template <typename T>
__global__ __launch_bounds__(1024) void batch_frame_kernel(const float* pool_ac, const float* pool_mfcc,
                                                           const float* pool_mfcc_low, const int32_t* pool_labels,
                                                           const int32_t* slots, int elems, int A, int L, float* acoustic,
                                                           float* mfcc, float* mfcc_low, float* action, float* location,
                                                           float* stats) {
    extern __shared__ __attribute__((aligned(16))) float frame_lds[];
    __shared__ float sm[16];
    const int tid = threadIdx.x, n = blockIdx.x;
    const long s = slots[n];
    float mn, mx;
    frame_normalise<T>(pool_ac + s * elems, elems, acoustic + (long)n * elems, frame_lds, sm, mn, mx);
    if (tid < GATHER_MFCC) mfcc[(long)n * GATHER_MFCC + tid] = pool_mfcc[s * GATHER_MFCC + tid];
    else if (tid < 2 * GATHER_MFCC)
        mfcc_low[(long)n * GATHER_MFCC + tid - GATHER_MFCC] = pool_mfcc_low[s * GATHER_MFCC + tid - GATHER_MFCC];
    one_hot_rows(pool_labels, s, n, A, L, action, location);
    if (tid == 0) *reinterpret_cast<float4*>(stats + 4 * (long)n) = make_float4(mn, mx, 0.f, 0.f);
}

// The per-row kernel of acimg_batch_gather_pairs: one workgroup per row code; the row's kind is the same for the whole
// workgroup, so the branch costs nothing.  A real row is batch_frame_kernel's (the same device function).  A silent row
// reads the 48 bytes of its slot's low-passed MFCC row and nothing else of the pool: acoustic[i] = low[i % 12].  As
// float4 (T) a store i holds channels 4 (i % 3) .. + 3, and 1024 % 3 == 1, so a thread's stores cycle through the three
// quarters of the row with period three: it selects its three float4 once and then only stores.
template <typename T>
__global__ __launch_bounds__(1024) void batch_pair_kernel(const float* pool_ac, const float* pool_mfcc,
                                                          const float* pool_mfcc_low, const int32_t* pool_labels,
                                                          const int32_t* codes, int elems, int A, int L, float* acoustic,
                                                          float* mfcc, float* pair, float* action, float* location,
                                                          float* stats) {
    extern __shared__ __attribute__((aligned(16))) float frame_lds[];
    __shared__ float sm[16];
    const int tid = threadIdx.x, n = blockIdx.x;
    const int32_t code = codes[n];
    const bool silent = code < 0;
    const long s = code_slot(code);
    float* out = acoustic + (long)n * elems;
    if (silent) {
        const float* low = pool_mfcc_low + s * GATHER_MFCC;
        if constexpr (sizeof(T) == sizeof(float4)) {
            float4 q[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) q[j] = make_float4(low[4 * j], low[4 * j + 1], low[4 * j + 2], low[4 * j + 3]);
            const int ph = tid % 3;
            const float4 q0 = ph == 0 ? q[0] : ph == 1 ? q[1] : q[2];
            const float4 q1 = ph == 0 ? q[1] : ph == 1 ? q[2] : q[0];
            const float4 q2 = ph == 0 ? q[2] : ph == 1 ? q[0] : q[1];
            float4* o = reinterpret_cast<float4*>(out);
            const int cnt = elems / 4;
            for (int i = tid; i < cnt; i += 3 * 1024) {
                o[i] = q0;
                if (i + 1024 < cnt) o[i + 1024] = q1;
                if (i + 2048 < cnt) o[i + 2048] = q2;
            }
        } else {
            for (int i = tid; i < elems; i += 1024) out[i] = low[i % GATHER_MFCC];
        }
        if (tid < GATHER_MFCC) mfcc[(long)n * GATHER_MFCC + tid] = low[tid];
        if (tid == 0) *reinterpret_cast<float4*>(stats + 4 * (long)n) = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
        float mn, mx;
        frame_normalise<T>(pool_ac + s * elems, elems, out, frame_lds, sm, mn, mx);
        if (tid < GATHER_MFCC) mfcc[(long)n * GATHER_MFCC + tid] = pool_mfcc[s * GATHER_MFCC + tid];
        if (tid == 0) *reinterpret_cast<float4*>(stats + 4 * (long)n) = make_float4(mn, mx, 0.f, 0.f);
    }
    if (tid < 2) pair[2 * (long)n + tid] = (tid == 0) == silent ? 1.f : 0.f;      // {0, 1} real, {1, 0} silent
    one_hot_rows(pool_labels, s, n, A, L, action, location);
}

}  // namespace acimg

using namespace acimg;

namespace {

// What the two entry points share: the refusals, the video launch and the per-row launch.  PAIRS: `slots` holds row
// codes and `sixth` is the pair output (batch_pair_kernel); else slots and the low-passed MFCC output (batch_frame_kernel).
template <bool PAIRS>
int gather(const char* who, const uint8_t* pool_video, size_t video_stride, const float* pool_acoustic, const float* pool_mfcc,
           const float* pool_mfcc_low, const int32_t* pool_labels, const int32_t* slots, int N, int pixels, int elems,
           int num_actions, int num_locations, float* video, float* acoustic, float* mfcc, float* sixth, float* action,
           float* location, void* ws, size_t ws_bytes, void* stream) {
    if (N <= 0) return fail(ACIMG_EINVAL, "%s: N must be positive", who);
    if (N > 65535) return fail(ACIMG_EINVAL, "%s: N = %d exceeds the grid's y extent", who, N);
    if (pixels <= 0 || elems <= 0 || num_actions <= 0 || num_locations <= 0)
        return fail(ACIMG_EINVAL, "%s: pixels, elems and the one-hot widths must be positive", who);
    if (elems > GATHER_MAX_ELEMS)
        return fail(ACIMG_EINVAL, "%s: elems = %d exceeds the %d floats of the LDS image", who, elems, GATHER_MAX_ELEMS);
    if (PAIRS && elems % GATHER_MFCC != 0)
        return fail(ACIMG_EINVAL, "%s: elems = %d is no multiple of %d: a silent row tiles whole pixels of MFCC rows", who,
                    elems, GATHER_MFCC);
    if (video_stride % 16 != 0 || video_stride < (size_t)pixels * 3)
        return fail(ACIMG_EINVAL, "%s: slot stride %zu must be a multiple of 16 and hold %ld bytes", who, video_stride,
                    (long)pixels * 3);
    if (!pool_video || !pool_acoustic || !pool_mfcc || !pool_mfcc_low || !pool_labels || !slots || !video || !acoustic ||
        !mfcc || !sixth || !action || !location || !ws)
        return fail(ACIMG_EINVAL, "%s: null argument", who);
    if (!aligned16(pool_video) || !aligned16(ws))
        return fail(ACIMG_EINVAL, "%s: the video pool and the workspace must be 16-byte aligned", who);
    const size_t need = acimg_batch_gather_workspace(N, elems);
    if (ws_bytes < need) return fail(ACIMG_EWORKSPACE, "%s: workspace %zu < %zu bytes", who, ws_bytes, need);
    hipStream_t st = (hipStream_t)stream;
    // whole 16-pixel chunks take the vector path when every frame's float row starts 16-byte aligned
    const long chunks = (pixels % 4 == 0 && aligned16(video)) ? pixels / 16 : 0;
    const int tiles = cdiv(chunks, VID_THREADS);
    const int tails = cdiv((long)pixels * 3 - chunks * 48, VID_TAIL_FLOATS);
    if ((long)tiles + tails > 0x7fffffffL) return fail(ACIMG_EINVAL, "%s: %d pixels exceed the grid", who, pixels);
    hipLaunchKernelGGL(batch_video_kernel<PAIRS>, dim3(tiles + tails, N), dim3(VID_THREADS), 0, st, pool_video, video_stride,
                       slots, (long)pixels, chunks, tiles, video);
    int rc = check_launch(PAIRS ? "batch_gather_pairs (video)" : "batch_gather (video)");
    if (rc) return rc;
    const int lds = ((elems + 3) & ~3) * (int)sizeof(float);
    const bool vec = elems % 4 == 0 && aligned16(pool_acoustic) && aligned16(acoustic);
    const auto scalar_kernel = PAIRS ? batch_pair_kernel<float> : batch_frame_kernel<float>;
    const auto vector_kernel = PAIRS ? batch_pair_kernel<float4> : batch_frame_kernel<float4>;
    static bool attr = false;
    if (!attr) {
        for (const void* k : {reinterpret_cast<const void*>(scalar_kernel), reinterpret_cast<const void*>(vector_kernel)})
            (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, GATHER_MAX_ELEMS * (int)sizeof(float));
        attr = true;
    }
    hipLaunchKernelGGL(vec ? vector_kernel : scalar_kernel, dim3(N), dim3(1024), lds, st, pool_acoustic, pool_mfcc,
                       pool_mfcc_low, pool_labels, slots, elems, num_actions, num_locations, acoustic, mfcc, sixth, action,
                       location, (float*)ws);
    return check_launch(PAIRS ? "batch_gather_pairs (rows)" : "batch_gather (frames)");
}

}  // namespace

extern "C" {

size_t acimg_batch_gather_workspace(int N, int elems) {
    (void)elems;
    return N > 0 ? (size_t)N * 4 * sizeof(float) : 0;
}

int acimg_batch_gather(const uint8_t* pool_video, size_t video_stride, const float* pool_acoustic, const float* pool_mfcc,
                       const float* pool_mfcc_low, const int32_t* pool_labels, const int32_t* slots, int N, int pixels,
                       int elems, int num_actions, int num_locations, float* video, float* acoustic, float* mfcc,
                       float* mfcc_low, float* action, float* location, void* ws, size_t ws_bytes, void* stream) {
    return gather<false>("batch_gather", pool_video, video_stride, pool_acoustic, pool_mfcc, pool_mfcc_low, pool_labels, slots,
                         N, pixels, elems, num_actions, num_locations, video, acoustic, mfcc, mfcc_low, action, location, ws,
                         ws_bytes, stream);
}

size_t acimg_batch_gather_pairs_workspace(int N, int elems) { return acimg_batch_gather_workspace(N, elems); }

int acimg_batch_gather_pairs(const uint8_t* pool_video, size_t video_stride, const float* pool_acoustic,
                             const float* pool_mfcc, const float* pool_mfcc_low, const int32_t* pool_labels,
                             const int32_t* rows, int N, int pixels, int elems, int num_actions, int num_locations,
                             float* video, float* acoustic, float* mfcc, float* pair, float* action, float* location, void* ws,
                             size_t ws_bytes, void* stream) {
    return gather<true>("batch_gather_pairs", pool_video, video_stride, pool_acoustic, pool_mfcc, pool_mfcc_low, pool_labels,
                        rows, N, pixels, elems, num_actions, num_locations, video, acoustic, mfcc, pair, action, location, ws,
                        ws_bytes, stream);
}

}  // extern "C"
