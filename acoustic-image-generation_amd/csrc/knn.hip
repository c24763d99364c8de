// Exact k-nearest-neighbour search in fp64 and the neighbour vote of the latent-space evaluation (knn.py, retrieve.py).
//
// acimg_knn_topk: a workgroup owns KNN_QB = 32 queries (8 per wave) and streams the gallery rows of its slab through LDS
// in tiles of KNN_TG = 64 rows, D in chunks of KNN_DC = 32 (zero-padded on both sides, so a pad adds exactly +0).  Lane
// l of wave w accumulates the direct-difference squares of gallery row (tile + l) against the wave's 8 queries, so one
// query's 64 candidates of a tile sit in the 64 lanes of one wave.  Each query keeps its sorted K-list of
// (dist2, index) keys in LDS; a tile's candidates are first compared with the current K-th key (one compare, one
// ballot) and only the survivors are ranked into the list (merge by counting: ranks are a permutation, so the writes
// never collide).  Keys are unique (indices are), so the order is total and the result does not depend on the tile
// order.  When the query blocks cannot fill the chip the gallery is cut into slabs; each (query block, slab) work item
// writes its K-list to the workspace and a second launch merges the slab lists of each query in slab order.  The work
// items are renumbered so that the workgroups dealt to one XCD (b, b + 8, ...) take consecutive slabs of one query
// block (placement is a speed matter only).  No atomics: every run is bit-identical.
#include <algorithm>
#include <climits>
#include <cmath>

#include "common.hpp"

namespace acimg {

constexpr int KNN_QB = 32;             // queries per workgroup
constexpr int KNN_QW = 8;              // queries per wave
constexpr int KNN_TG = 64;             // gallery rows per tile (one per lane)
constexpr int KNN_DC = 32;             // feature chunk
constexpr int KNN_KMAX = 64;
constexpr int KNN_QPAD = KNN_QB + 2;   // 16-byte aligned rows, fewer bank conflicts on the transposed store
constexpr int KNN_TARGET_WG = 512;     // two workgroups per CU
constexpr int KNN_MIN_TILES = 4;       // gallery tiles per slab at least
static_assert(KNN_QB == 4 * KNN_QW, "four waves");

__device__ __forceinline__ bool key_less(double da, int ia, double db, int ib) {
    return da < db || (da == db && ia < ib);
}

// LDS ordering between the lanes of one wave: wait for this wave's LDS operations, no code motion across
__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
    __builtin_amdgcn_wave_barrier();
}

// rank the candidate (cd, ci) of every lane with `pass` set into the sorted K-list (ld, li); sd / si: 64-entry scratch
__device__ __forceinline__ void knn_insert(double* ld, int* li, int K, bool pass, double cd, int ci, double* sd, int* si,
                                           int lane) {
    const uint64_t m = __ballot(pass);
    if (m == 0) return;
    const int n = __popcll(m);
    const int p = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
    if (pass) {
        sd[p] = cd;
        si[p] = ci;
    }
    wave_lds_sync();
    double ed = 0.0;
    int ei = 0, erank = KNN_KMAX, srank = KNN_KMAX;
    if (lane < K) {
        ed = ld[lane];
        ei = li[lane];
        int c = 0;
        for (int s = 0; s < n; ++s) c += key_less(sd[s], si[s], ed, ei);
        erank = lane + c;
    }
    if (pass) {
        int lo = 0, hi = K;   // list entries below the candidate
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (key_less(ld[mid], li[mid], cd, ci)) lo = mid + 1;
            else hi = mid;
        }
        int c = 0;
        for (int s = 0; s < n; ++s) c += key_less(sd[s], si[s], cd, ci);
        srank = lo + c;
    }
    wave_lds_sync();
    if (erank < K) {
        ld[erank] = ed;
        li[erank] = ei;
    }
    if (srank < K) {
        ld[srank] = cd;
        li[srank] = ci;
    }
    wave_lds_sync();
}

// blocks dealt round-robin over 8 XCDs: the blocks of one XCD get consecutive work items
__device__ __forceinline__ int xcd_work_item(int b, int nb) {
    const int xcd = b & 7, per = nb >> 3, rem = nb & 7;
    return (xcd < rem ? xcd * (per + 1) : rem * (per + 1) + (xcd - rem) * per) + (b >> 3);
}

__global__ __launch_bounds__(256) void knn_slab_kernel(const double* __restrict__ query, int ldq, int Q,
                                                       const double* __restrict__ gallery, int ldg, int G, int D, int K,
                                                       int slabs, int tiles_per_slab, double* out_d, int* out_i) {
    __shared__ double gT[KNN_DC][KNN_TG + 1];
    __shared__ __attribute__((aligned(16))) double qT[KNN_DC][KNN_QPAD];
    __shared__ double lst_d[KNN_QB][KNN_KMAX];
    __shared__ int lst_i[KNN_QB][KNN_KMAX];
    __shared__ double scr_d[4][64];
    __shared__ int scr_i[4][64];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int item = xcd_work_item(blockIdx.x, gridDim.x);
    const int qb = item / slabs, slab = item - qb * slabs;
    const int q0 = qb * KNN_QB;
    const int gbeg = slab * tiles_per_slab * KNN_TG;
    const int gend = min(G, gbeg + tiles_per_slab * KNN_TG);

    for (int e = tid; e < KNN_QB * KNN_KMAX; e += 256) {
        lst_d[e / KNN_KMAX][e % KNN_KMAX] = INFINITY;
        lst_i[e / KNN_KMAX][e % KNN_KMAX] = INT_MAX;
    }
    __syncthreads();

    for (int g0 = gbeg; g0 < gend; g0 += KNN_TG) {
        double acc[KNN_QW];
#pragma unroll
        for (int j = 0; j < KNN_QW; ++j) acc[j] = 0.0;
        for (int d0 = 0; d0 < D; d0 += KNN_DC) {
            __syncthreads();   // the previous chunk has been read (and the lists initialised)
#pragma unroll
            for (int k = 0; k < KNN_TG * KNN_DC / 256; ++k) {
                const int e = tid + k * 256, r = e / KNN_DC, c = e % KNN_DC;
                const int g = g0 + r, d = d0 + c;
                gT[c][r] = (g < gend && d < D) ? gallery[(size_t)g * ldg + d] : 0.0;
            }
#pragma unroll
            for (int k = 0; k < KNN_QB * KNN_DC / 256; ++k) {
                const int e = tid + k * 256, r = e / KNN_DC, c = e % KNN_DC;
                const int q = q0 + r, d = d0 + c;
                qT[c][r] = (q < Q && d < D) ? query[(size_t)q * ldq + d] : 0.0;
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < KNN_DC; ++c) {
                const double gv = gT[c][lane];
                const double2* qv = reinterpret_cast<const double2*>(&qT[c][w * KNN_QW]);
#pragma unroll
                for (int j = 0; j < KNN_QW / 2; ++j) {
                    const double2 v = qv[j];
                    const double a = v.x - gv, b = v.y - gv;
                    acc[2 * j] = fma(a, a, acc[2 * j]);
                    acc[2 * j + 1] = fma(b, b, acc[2 * j + 1]);
                }
            }
        }
        const int g = g0 + lane;
        const bool gvalid = g < gend;
#pragma unroll
        for (int j = 0; j < KNN_QW; ++j) {
            const int ql = w * KNN_QW + j;
            if (q0 + ql >= Q) break;   // wave-uniform
            double* ld = lst_d[ql];
            int* li = lst_i[ql];
            const bool pass = gvalid && key_less(acc[j], g, ld[K - 1], li[K - 1]);
            knn_insert(ld, li, K, pass, acc[j], g, scr_d[w], scr_i[w], lane);
        }
    }

    // this wave's queries: the slab list (sentinels kept) or, unsplit, the final answer (-1 / +inf past G)
    for (int j = 0; j < KNN_QW; ++j) {
        const int ql = w * KNN_QW + j, q = q0 + ql;
        if (q >= Q || lane >= K) continue;
        const double d = lst_d[ql][lane];
        const int i = lst_i[ql][lane];
        if (slabs > 1) {
            const size_t o = ((size_t)q * slabs + slab) * K + lane;
            out_d[o] = d;
            out_i[o] = i;
        } else {
            const size_t o = (size_t)q * K + lane;
            out_d[o] = i == INT_MAX ? INFINITY : d;
            out_i[o] = i == INT_MAX ? -1 : i;
        }
    }
}

// one wave per query: merge its slab lists in slab order (a stable two-list merge by ranks: equal sentinel keys of
// the running list rank before those of the next slab, so the ranks stay a permutation)
__global__ __launch_bounds__(256) void knn_merge_kernel(const double* part_d, const int* part_i, int Q, int K, int slabs,
                                                        double* dist2, int* idx) {
    __shared__ double ad[4][KNN_KMAX], bd[4][KNN_KMAX];
    __shared__ int ai[4][KNN_KMAX], bi[4][KNN_KMAX];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= Q) return;   // whole waves only
    const size_t base = (size_t)q * slabs * K;
    if (lane < K) {
        ad[w][lane] = part_d[base + lane];
        ai[w][lane] = part_i[base + lane];
    }
    for (int s = 1; s < slabs; ++s) {
        if (lane < K) {
            bd[w][lane] = part_d[base + (size_t)s * K + lane];
            bi[w][lane] = part_i[base + (size_t)s * K + lane];
        }
        wave_lds_sync();
        int ra = KNN_KMAX, rb = KNN_KMAX;
        double xa = 0.0, xb = 0.0;
        int ia = 0, ib = 0;
        if (lane < K) {
            xa = ad[w][lane];
            ia = ai[w][lane];
            xb = bd[w][lane];
            ib = bi[w][lane];
            int lo = 0, hi = K;   // b strictly below a[lane]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (key_less(bd[w][mid], bi[w][mid], xa, ia)) lo = mid + 1;
                else hi = mid;
            }
            ra = lane + lo;
            lo = 0;
            hi = K;               // a at or below b[lane]
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (!key_less(xb, ib, ad[w][mid], ai[w][mid])) lo = mid + 1;
                else hi = mid;
            }
            rb = lane + lo;
        }
        wave_lds_sync();
        if (ra < K) {
            ad[w][ra] = xa;
            ai[w][ra] = ia;
        }
        if (rb < K) {
            ad[w][rb] = xb;
            ai[w][rb] = ib;
        }
        wave_lds_sync();
    }
    if (lane < K) {
        const int i = ai[w][lane];
        dist2[(size_t)q * K + lane] = i == INT_MAX ? INFINITY : ad[w][lane];
        idx[(size_t)q * K + lane] = i == INT_MAX ? -1 : i;
    }
}

// one wave per query: lane c counts class c among the first K labels; lane j checks neighbour j for first_hit
__global__ __launch_bounds__(256) void knn_vote_kernel(const int* __restrict__ idx, int ldidx, int Q, int K,
                                                       const int* __restrict__ gallery_labels,
                                                       const int* __restrict__ query_labels, int num_classes, int* pred,
                                                       int* first_hit) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int q = blockIdx.x * 4 + w;
    if (q >= Q) return;
    int lab = -1;
    if (lane < K) {
        const int g = idx[(size_t)q * ldidx + lane];
        if (g >= 0) lab = gallery_labels[g];
    }
    if (pred) {
        int cnt = 0;
        for (int j = 0; j < K; ++j) cnt += __shfl(lab, j, 64) == lane;
        // the largest count, the smallest class on a tie
        int key = lane < num_classes ? (cnt << 8) | (255 - lane) : -1;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) key = max(key, __shfl_xor(key, o, 64));
        if (lane == 0) pred[q] = 255 - (key & 255);
    }
    if (first_hit) {
        const int want = query_labels[q];
        const uint64_t m = __ballot(lane < K && lab >= 0 && lab == want);
        if (lane == 0) first_hit[q] = m ? (int)__builtin_ctzll(m) + 1 : 0;
    }
}

// slab count and tiles per slab of a launch (host and workspace query agree through this one function)
static void knn_split(int Q, int G, int& slabs, int& tiles_per_slab) {
    const int tiles = cdiv(G, KNN_TG), qblocks = cdiv(Q, KNN_QB);
    int s = 1;
    if (qblocks < KNN_TARGET_WG) s = std::min(cdiv(KNN_TARGET_WG, qblocks), cdiv(tiles, KNN_MIN_TILES));
    s = std::max(s, 1);
    tiles_per_slab = cdiv(tiles, s);
    slabs = cdiv(tiles, tiles_per_slab);
}

static int knn_check(int ldq, int Q, int ldg, int G, int D, int K) {
    if (K < 1 || K > KNN_KMAX) return fail(ACIMG_EINVAL, "knn_topk: K = %d outside [1, %d]", K, KNN_KMAX);
    if (D < 1) return fail(ACIMG_EINVAL, "knn_topk: D = %d must be positive", D);
    if (ldq < D || ldg < D) return fail(ACIMG_EINVAL, "knn_topk: leading dimensions %d / %d below D = %d", ldq, ldg, D);
    if (G < 1) return fail(ACIMG_EINVAL, "knn_topk: empty gallery (G = %d)", G);
    if (Q < 0) return fail(ACIMG_EINVAL, "knn_topk: Q = %d is negative", Q);
    return ACIMG_OK;
}

}  // namespace acimg

using namespace acimg;

extern "C" {

size_t acimg_knn_topk_workspace(int Q, int G, int D, int K) {
    if (knn_check(D, Q, D, G, D, K) != ACIMG_OK || Q == 0) return 0;
    int slabs, tps;
    knn_split(Q, G, slabs, tps);
    if (slabs == 1) return 0;
    return (size_t)Q * slabs * K * (sizeof(double) + sizeof(int));
}

int acimg_knn_topk(const double* query, int ldq, int Q, const double* gallery, int ldg, int G, int D, int K,
                   double* dist2, int32_t* idx, void* ws, size_t ws_bytes, void* stream) {
    int rc = knn_check(ldq, Q, ldg, G, D, K);
    if (rc) return rc;
    if (Q == 0) return ACIMG_OK;
    if (!query || !gallery || !dist2 || !idx) return fail(ACIMG_EINVAL, "knn_topk: null argument");
    int slabs, tps;
    knn_split(Q, G, slabs, tps);
    const size_t need = acimg_knn_topk_workspace(Q, G, D, K);
    if (need && (!ws || ws_bytes < need))
        return fail(ACIMG_EWORKSPACE, "knn_topk: workspace %zu < %zu bytes", ws ? ws_bytes : (size_t)0, need);
    const long nb = (long)cdiv(Q, KNN_QB) * slabs;
    if (nb > INT_MAX) return fail(ACIMG_EINVAL, "knn_topk: %ld workgroups", nb);
    hipStream_t s = (hipStream_t)stream;
    double* part_d = slabs > 1 ? (double*)ws : dist2;
    int* part_i = slabs > 1 ? (int*)((char*)ws + (size_t)Q * slabs * K * sizeof(double)) : idx;
    hipLaunchKernelGGL(knn_slab_kernel, dim3((unsigned)nb), dim3(256), 0, s, query, ldq, Q, gallery, ldg, G, D, K, slabs,
                       tps, part_d, part_i);
    rc = check_launch("knn_topk");
    if (rc || slabs == 1) return rc;
    hipLaunchKernelGGL(knn_merge_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, s, part_d, part_i, Q, K, slabs, dist2, idx);
    return check_launch("knn_topk (merge)");
}

int acimg_knn_vote(const int32_t* idx, int ldidx, int Q, int K, const int32_t* gallery_labels,
                   const int32_t* query_labels, int num_classes, int32_t* pred, int32_t* first_hit, void* stream) {
    if (K < 1 || K > KNN_KMAX) return fail(ACIMG_EINVAL, "knn_vote: K = %d outside [1, %d]", K, KNN_KMAX);
    if (ldidx < K) return fail(ACIMG_EINVAL, "knn_vote: ldidx = %d below K = %d", ldidx, K);
    if (num_classes < 1 || num_classes > 64) return fail(ACIMG_EINVAL, "knn_vote: num_classes = %d outside [1, 64]",
                                                         num_classes);
    if (Q < 0) return fail(ACIMG_EINVAL, "knn_vote: Q = %d is negative", Q);
    if (Q == 0 || (!pred && !first_hit)) return ACIMG_OK;
    if (!idx || !gallery_labels) return fail(ACIMG_EINVAL, "knn_vote: null argument");
    if (first_hit && !query_labels) return fail(ACIMG_EINVAL, "knn_vote: first_hit needs query_labels");
    hipLaunchKernelGGL(knn_vote_kernel, dim3(cdiv(Q, 4)), dim3(256), 0, (hipStream_t)stream, idx, ldidx, Q, K,
                       gallery_labels, query_labels, num_classes, pred, first_hit);
    return check_launch("knn_vote");
}

}  // extern "C"
