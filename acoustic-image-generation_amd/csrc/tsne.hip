// Exact two-component t-SNE in fp64 (van der Maaten & Hinton; knn.py:67-90 calls sklearn's TSNE on the test dump): the
// conditional affinities with their per-row precision search, the symmetrisation, and the descent as two launches per
// iteration (row sums of the gradient terms, then the update of Y, V and the gains).
//
// acimg_tsne_affinities: one workgroup of 256 threads per row i.  Thread t owns the columns j = t, t + 256, ... of
// the row from start to end: it forms their distances (the rows x_j go through LDS in tiles of 256 rows x 8 features,
// summed in feature order, direct-difference form as in knn.hip), parks them in row i of P, reads only its own
// entries back in every search step and overwrites them with p_{j|i} at the end.  So the row is NOT cached in LDS:
// it is re-read through L1 / L2 (a row of 16384 columns is 128 KB), which costs little next to the exp of every
// entry, and leaves one code path for every N.  The two sums of a search step are block reductions; every thread
// receives the same bits, so the whole workgroup takes the same branch.
//
// acimg_tsne_symmetrize: 32 x 32 tiles; the workgroup of tile pair (a, b), a <= b, owns both tiles, and one thread
// forms each unordered pair's value once and parks it in LDS at both places, from where both tiles are stored with
// coalesced rows.
//
// acimg_tsne_gradient: one workgroup per row i reads row i of P once (coalesced) and Y through L1 / L2 (16 bytes
// per row; Y of 16384 rows is 256 KB), and leaves six sums.  acimg_tsne_update: one thread per row of Y; every
// workgroup first sums the N per-row normalisers in the same order.
//
// Every reduction is a fixed tree (a thread's own entries in ascending order, the xor butterfly of its wave, the
// four waves in order): no atomics, two runs are bit-identical.
#include <cmath>

#include "common.hpp"

namespace acimg {

constexpr int TSNE_T = 256;            // threads per workgroup
constexpr int TSNE_DC = 8;             // feature chunk of the distance tiles
constexpr int TSNE_MAX_STEPS = 100;    // precision search
constexpr double TSNE_SEARCH_TOL = 1e-5;
constexpr int TSNE_SY = 32;            // symmetrisation tile

// sum over the workgroup (256 threads); every thread receives the same bits.  smem: 4 doubles, reusable after return
__device__ __forceinline__ double tsne_block_sum(double v, double* smem) {
    v = wave_sum_d(v);
    __syncthreads();                   // the previous use has been read
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

__global__ __launch_bounds__(TSNE_T) void tsne_affinities_kernel(const double* __restrict__ x, int ldx, int N, int D,
                                                                 double log_perplexity, double* __restrict__ P, int ldp,
                                                                 double* __restrict__ beta_out,
                                                                 int* __restrict__ steps_out) {
    __shared__ double tile[TSNE_T][TSNE_DC + 1];
    __shared__ double xi[TSNE_DC];
    __shared__ double red[2][4];
    const int tid = threadIdx.x, i = blockIdx.x;
    double* row = P + (size_t)i * ldp;

    // distances: d_ij = sum_d (x_i[d] - x_j[d])^2
    for (int j0 = 0; j0 < N; j0 += TSNE_T) {
        double acc = 0.0;
        for (int d0 = 0; d0 < D; d0 += TSNE_DC) {
            __syncthreads();           // the previous chunk has been read
#pragma unroll
            for (int k = 0; k < TSNE_DC; ++k) {
                const int e = tid + k * TSNE_T, r = e / TSNE_DC, c = e % TSNE_DC;
                const int j = j0 + r, d = d0 + c;
                tile[r][c] = (j < N && d < D) ? x[(size_t)j * ldx + d] : 0.0;
            }
            if (tid < TSNE_DC) xi[tid] = d0 + tid < D ? x[(size_t)i * ldx + d0 + tid] : 0.0;
            __syncthreads();
#pragma unroll
            for (int c = 0; c < TSNE_DC; ++c) {
                const double a = xi[c] - tile[tid][c];   // a pad column gives 0 - 0
                acc = fma(a, a, acc);
            }
        }
        if (j0 + tid < N) row[j0 + tid] = acc;
    }

    // precision search (sklearn's _binary_search_perplexity); every thread re-reads its own entries only
    double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY, S = 1.0;
    int steps = 0;
    for (int step = 0; step < TSNE_MAX_STEPS; ++step) {
        double s = 0.0, sd = 0.0;
        for (int j = tid; j < N; j += TSNE_T) {
            if (j == i) continue;
            const double d = row[j], p = exp(-d * beta);
            s += p;
            sd = fma(d, p, sd);
        }
        S = tsne_block_sum(s, red[0]);
        const double SD = tsne_block_sum(sd, red[1]);
        if (S == 0.0) S = 1e-8;
        const double H = log(S) + beta * SD / S;
        const double diff = H - log_perplexity;
        steps = step + 1;
        if (fabs(diff) <= TSNE_SEARCH_TOL || step == TSNE_MAX_STEPS - 1) break;   // beta stays the one evaluated
        if (diff > 0.0) {
            beta_min = beta;
            beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
        } else {
            beta_max = beta;
            beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
        }
    }
    for (int j = tid; j < N; j += TSNE_T) row[j] = j == i ? 0.0 : exp(-row[j] * beta) / S;
    if (tid == 0) {
        beta_out[i] = beta;
        steps_out[i] = steps;
    }
}

__global__ __launch_bounds__(TSNE_T) void tsne_symmetrize_kernel(double* __restrict__ P, int ldp, int N, double two_n) {
    __shared__ double A[TSNE_SY][TSNE_SY + 1], B[TSNE_SY][TSNE_SY + 1];
    const int ta = blockIdx.y, tb = blockIdx.x;
    if (ta > tb) return;               // the pair (tb, ta) owns these tiles
    const int r0 = ta * TSNE_SY, c0 = tb * TSNE_SY;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const bool diag = ta == tb;
    // A = P[r0.., c0..], B = P[c0.., r0..]
    for (int a = ty; a < TSNE_SY; a += TSNE_T / 32) {
        const bool inA = r0 + a < N && c0 + tx < N, inB = c0 + a < N && r0 + tx < N;
        A[a][tx] = inA ? P[(size_t)(r0 + a) * ldp + c0 + tx] : 0.0;
        if (!diag) B[a][tx] = inB ? P[(size_t)(c0 + a) * ldp + r0 + tx] : 0.0;
    }
    __syncthreads();
    // the pair (r0 + a, c0 + tx): on a diagonal tile only a < tx, whose thread also fills the mirrored place
    double v[TSNE_SY / (TSNE_T / 32)];
#pragma unroll
    for (int k = 0; k < TSNE_SY / (TSNE_T / 32); ++k) {
        const int a = ty + k * (TSNE_T / 32);
        v[k] = (A[a][tx] + (diag ? A[tx][a] : B[tx][a])) / two_n;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < TSNE_SY / (TSNE_T / 32); ++k) {
        const int a = ty + k * (TSNE_T / 32);
        if (!diag) {
            A[a][tx] = v[k];
            B[tx][a] = v[k];
        } else if (a < tx) {
            A[a][tx] = v[k];
            A[tx][a] = v[k];
        } else if (a == tx) {
            A[a][tx] = 0.0;
        }
    }
    __syncthreads();
    for (int a = ty; a < TSNE_SY; a += TSNE_T / 32) {
        if (r0 + a < N && c0 + tx < N) P[(size_t)(r0 + a) * ldp + c0 + tx] = A[a][tx];
        if (!diag && c0 + a < N && r0 + tx < N) P[(size_t)(c0 + a) * ldp + r0 + tx] = B[a][tx];
    }
}

__global__ __launch_bounds__(TSNE_T) void tsne_gradient_kernel(const double* __restrict__ P, int ldp, int N,
                                                               const double* __restrict__ Y, int want_kl,
                                                               double* __restrict__ rows) {
    __shared__ double red[6][4];
    const int tid = threadIdx.x, i = blockIdx.x;
    const double* prow = P + (size_t)i * ldp;
    const double yx = Y[2 * (size_t)i], yy = Y[2 * (size_t)i + 1];
    double ax = 0.0, ay = 0.0, rx = 0.0, ry = 0.0, sw = 0.0, kl = 0.0;
#pragma unroll 4
    for (int j = tid; j < N; j += TSNE_T) {
        if (j == i) continue;
        const double p = prow[j];
        const double dx = yx - Y[2 * (size_t)j], dy = yy - Y[2 * (size_t)j + 1];
        const double w = 1.0 / (1.0 + (dx * dx + dy * dy));
        const double pw = p * w, ww = w * w;
        ax = fma(pw, dx, ax);
        ay = fma(pw, dy, ay);
        rx = fma(ww, dx, rx);
        ry = fma(ww, dy, ry);
        sw += w;
        if (want_kl && p > 0.0) kl = fma(p, log(p) - log(w), kl);
    }
    ax = tsne_block_sum(ax, red[0]);
    ay = tsne_block_sum(ay, red[1]);
    rx = tsne_block_sum(rx, red[2]);
    ry = tsne_block_sum(ry, red[3]);
    sw = tsne_block_sum(sw, red[4]);
    kl = want_kl ? tsne_block_sum(kl, red[5]) : 0.0;   // want_kl is uniform
    if (tid == 0) {
        double* o = rows + 6 * (size_t)i;
        o[0] = ax;
        o[1] = ay;
        o[2] = rx;
        o[3] = ry;
        o[4] = sw;
        o[5] = kl;
    }
}

__global__ __launch_bounds__(TSNE_T) void tsne_update_kernel(const double* __restrict__ rows, int N, double e,
                                                             double momentum, double learning_rate,
                                                             double* __restrict__ Y, double* __restrict__ V,
                                                             double* __restrict__ G, double* __restrict__ kl) {
    __shared__ double red[2][4];
    const int tid = threadIdx.x;
    // Z: the same order in every workgroup, so the same bits
    double z = 0.0;
    for (int r = tid; r < N; r += TSNE_T) z += rows[6 * (size_t)r + 4];
    const double Z = tsne_block_sum(z, red[0]);
    if (kl && blockIdx.x == 0) {       // uniform in the workgroup
        double k = 0.0;
        for (int r = tid; r < N; r += TSNE_T) k += rows[6 * (size_t)r + 5];
        k = tsne_block_sum(k, red[1]);
        if (tid == 0) kl[0] = k + log(Z);
    }
    const int i = blockIdx.x * TSNE_T + tid;
    if (i >= N || !Y) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const size_t o = 2 * (size_t)i + c;
        const double g = 4.0 * (e * rows[6 * (size_t)i + c] - rows[6 * (size_t)i + 2 + c] / Z);
        const double v = V[o];
        double gain = G[o];
        gain = g * v < 0.0 ? gain + 0.2 : gain * 0.8;
        gain = fmax(gain, 0.01);
        const double vn = momentum * v - learning_rate * gain * g;
        G[o] = gain;
        V[o] = vn;
        Y[o] += vn;
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_tsne_affinities(const double* x, int ldx, int N, int D, double perplexity, double* P, int ldp, double* beta,
                          int32_t* steps, void* stream) {
    if (N < 4) return fail(ACIMG_EINVAL, "tsne_affinities: N = %d below 4", N);
    if (D < 1) return fail(ACIMG_EINVAL, "tsne_affinities: D = %d must be positive", D);
    if (ldx < D || ldp < N)
        return fail(ACIMG_EINVAL, "tsne_affinities: leading dimensions %d / %d below D = %d / N = %d", ldx, ldp, D, N);
    if (!(perplexity > 1.0 && perplexity < (double)(N - 1)))
        return fail(ACIMG_EINVAL, "tsne_affinities: perplexity %g outside (1, N - 1 = %d)", perplexity, N - 1);
    if (!x || !P || !beta || !steps) return fail(ACIMG_EINVAL, "tsne_affinities: null argument");
    hipLaunchKernelGGL(tsne_affinities_kernel, dim3(N), dim3(TSNE_T), 0, (hipStream_t)stream, x, ldx, N, D,
                       std::log(perplexity), P, ldp, beta, steps);
    return check_launch("tsne_affinities");
}

int acimg_tsne_symmetrize(double* P, int ldp, int N, void* stream) {
    if (N < 1) return fail(ACIMG_EINVAL, "tsne_symmetrize: N = %d must be positive", N);
    if (ldp < N) return fail(ACIMG_EINVAL, "tsne_symmetrize: ldp = %d below N = %d", ldp, N);
    if (!P) return fail(ACIMG_EINVAL, "tsne_symmetrize: null argument");
    const int nt = cdiv(N, TSNE_SY);
    if (nt > 65535) return fail(ACIMG_EINVAL, "tsne_symmetrize: N = %d exceeds %d", N, 65535 * TSNE_SY);
    hipLaunchKernelGGL(tsne_symmetrize_kernel, dim3(nt, nt), dim3(TSNE_T), 0, (hipStream_t)stream, P, ldp, N,
                       2.0 * (double)N);
    return check_launch("tsne_symmetrize");
}

int acimg_tsne_gradient(const double* P, int ldp, int N, const double* Y, int want_kl, double* rows, void* stream) {
    if (N < 1) return fail(ACIMG_EINVAL, "tsne_gradient: N = %d must be positive", N);
    if (ldp < N) return fail(ACIMG_EINVAL, "tsne_gradient: ldp = %d below N = %d", ldp, N);
    if (!P || !Y || !rows) return fail(ACIMG_EINVAL, "tsne_gradient: null argument");
    hipLaunchKernelGGL(tsne_gradient_kernel, dim3(N), dim3(TSNE_T), 0, (hipStream_t)stream, P, ldp, N, Y,
                       want_kl ? 1 : 0, rows);
    return check_launch("tsne_gradient");
}

int acimg_tsne_update(const double* rows, int N, double e, double momentum, double learning_rate, double* Y, double* V,
                      double* G, double* kl, void* stream) {
    if (N < 1) return fail(ACIMG_EINVAL, "tsne_update: N = %d must be positive", N);
    if (!(e > 0.0) || !(momentum >= 0.0) || !(learning_rate > 0.0) || std::isinf(e) || std::isinf(momentum) ||
        std::isinf(learning_rate))
        return fail(ACIMG_EINVAL, "tsne_update: e = %g, momentum = %g, learning_rate = %g must be finite, e and the rate "
                                  "positive, the momentum not negative", e, momentum, learning_rate);
    const bool kl_only = !Y && !V && !G;   // the divergence of the rows alone: workgroup 0 forms it
    if (!rows || (!kl_only && (!Y || !V || !G)) || (kl_only && !kl))
        return fail(ACIMG_EINVAL, "tsne_update: null argument");
    hipLaunchKernelGGL(tsne_update_kernel, dim3(kl_only ? 1 : cdiv(N, TSNE_T)), dim3(TSNE_T), 0, (hipStream_t)stream, rows, N, e,
                       momentum, learning_rate, Y, V, G, kl);
    return check_launch("tsne_update");
}

}  // extern "C"
