// Latent ops and losses of the acoustic-image train step for gfx950 (MI355X): what sits between the networks' last layers and
// the scalars a step reports.  This file owns
//   latent_fwd / _bwd_kernel, latent_linear_fwd / _bwd_kernel,   acimg_latent_fwd / _bwd, acimg_latent_linear_fwd / _bwd,
//   softplus_fwd / _bwd_kernel                                   acimg_softplus_fwd / _bwd (reparameterisation, KL)
//   clip_softmax_ce_kernel                                       acimg_clip_softmax_ce (the classifier's clip loss)
//   clip_eval_kernel, ClipEvalHead                               acimg_clip_eval, acimg_clip_eval_state_bytes
//   recon_loss_kernel, sumsq_kernel, sqerr_channels_kernel,      acimg_recon_loss, acimg_sumsq, acimg_sqerr_channels,
//   loss_finalize_kernel, ordered_block_sums                     acimg_loss_finalize, acimg_loss_scratch_bytes
// Callers: acimg/ops.py.  Sums that a step reports are combined in a fixed order (ordered_block_sums, clip_eval_kernel).
#include "common.hpp"

namespace acimg {

// ------------------------------------------------------------------------------------------
// latent: softplus, reparameterisation, KL ; one block per sample
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ float softplus_f(float x) {
    // log(1+exp(x)) evaluated as TF does: max(x,0) + log1p(exp(-|x|))
    return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x)));
}

__global__ __launch_bounds__(256) void latent_fwd_kernel(const float* heads, const float* eps,
                                                         float* z, int ldz, float* sigma, float* kl,
                                                         int Z) {
    __shared__ float sm[32];
    const int n = blockIdx.x;
    float acc = 0.f;
    for (int j = threadIdx.x; j < Z; j += 256) {
        const float mu = heads[(long)n * 2 * Z + j];
        const float sg = softplus_f(heads[(long)n * 2 * Z + Z + j]);
        sigma[(long)n * Z + j] = sg;
        z[(long)n * ldz + j] = mu + sg * eps[(long)n * Z + j];
        acc += mu * mu + sg * sg - logf(1e-8f + sg * sg) - 1.f;
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) kl[n] = 0.5f * acc;
}

__global__ __launch_bounds__(256) void latent_bwd_kernel(const float* heads, const float* eps,
                                                         const float* sigma, const float* gz, int ldgz,
                                                         float klw, float* gheads, int N, int Z) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * Z) return;
    const int n = idx / Z, j = idx - n * Z;
    const float mu = heads[(long)n * 2 * Z + j];
    const float sraw = heads[(long)n * 2 * Z + Z + j];
    const float sg = sigma[idx];
    const float g = gz[(long)n * ldgz + j];
    const float dmu = g + klw * mu;
    const float dsg = g * eps[idx] + klw * (sg - sg / (1e-8f + sg * sg));
    const float dsp = 1.f / (1.f + expf(-sraw));  // d softplus
    gheads[(long)n * 2 * Z + j] = dmu;
    gheads[(long)n * 2 * Z + Z + j] = dsg * dsp;
}

// softplus and its backward (the std tower of the latent associators, models/multimodal.py:48,107)
__global__ __launch_bounds__(256) void softplus_fwd_kernel(const float* x, int ldx, float* y, int ldy, int rows, int C) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C) return;
    const int r = idx / C, c = idx - r * C;
    y[(long)r * ldy + c] = softplus_f(x[(long)r * ldx + c]);
}
__global__ __launch_bounds__(256) void softplus_bwd_kernel(const float* x, int ldx, const float* gy, int ldgy, float* gx,
                                                           int ldgx, int rows, int C) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * C) return;
    const int r = idx / C, c = idx - r * C;
    gx[(long)r * ldgx + c] = gy[(long)r * ldgy + c] / (1.f + expf(-x[(long)r * ldx + c]));
}

// the RGB / spectrogram U-Nets use the second head as sigma directly (models/unet_architecture.py:66-69):
// z = mean + variance * eps, kl[n] = 0.5 * sum_j (mu^2 + s^2 - log(1e-8 + s^2) - 1)
__global__ __launch_bounds__(256) void latent_linear_fwd_kernel(const float* heads, const float* eps, float* z,
                                                                int ldz, float* kl, int Z) {
    __shared__ float sm[32];
    const int n = blockIdx.x;
    float acc = 0.f;
    for (int j = threadIdx.x; j < Z; j += 256) {
        const float mu = heads[(long)n * 2 * Z + j];
        const float sg = heads[(long)n * 2 * Z + Z + j];
        z[(long)n * ldz + j] = mu + sg * eps[(long)n * Z + j];
        acc += mu * mu + sg * sg - logf(1e-8f + sg * sg) - 1.f;
    }
    acc = block_sum(acc, sm);
    if (threadIdx.x == 0) kl[n] = 0.5f * acc;
}

__global__ __launch_bounds__(256) void latent_linear_bwd_kernel(const float* heads, const float* eps,
                                                                const float* gz, int ldgz, float klw,
                                                                float* gheads, int N, int Z) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= N * Z) return;
    const int n = idx / Z, j = idx - n * Z;
    const float mu = heads[(long)n * 2 * Z + j];
    const float sg = heads[(long)n * 2 * Z + Z + j];
    const float g = gz[(long)n * ldgz + j];
    gheads[(long)n * 2 * Z + j] = g + klw * mu;
    gheads[(long)n * 2 * Z + Z + j] = g * eps[idx] + klw * (sg - sg / (1e-8f + sg * sg));
}

// ------------------------------------------------------------------------------------------
// DualCamNet classifier (models/dualcamnet.py:82-106, models/base.py:34-38; its pooling: glue.hip): the clip-level
// softmax cross-entropy of trainer/trainer_reconstructed_class.py:49-56 (logits averaged over the clip's frames).
// ------------------------------------------------------------------------------------------
// one workgroup per clip: logits averaged over the F frames, softmax cross-entropy against `label`;
// out[0] += loss / clips, out[1] += (argmax == label); g[n*F+f][c] = (p_c - [c == label]) / (clips * F)
__global__ __launch_bounds__(64) void clip_softmax_ce_kernel(const float* logits, int ldl, int F, int K,
                                                             const int* labels, int clips, float* out, float* g,
                                                             int ldg) {
    const int n = blockIdx.x, c = threadIdx.x;
    float m = -INFINITY;
    if (c < K) {
        float a = 0.f;
        for (int f = 0; f < F; ++f) a += logits[((long)n * F + f) * ldl + c];
        m = a / (float)F;
    }
    const float mx = wave_max(m);
    const float e = c < K ? expf(m - mx) : 0.f;
    const float se = wave_sum(e);
    const float p = e / se;
    const int lab = labels[n];
    // argmax with the lowest index among ties (tf.argmax)
    int am = c < K && m == mx ? c : 1 << 20;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
    if (c == lab) {
        atomicAdd(out, -(m - mx - logf(se)) / (float)clips);
        if (am == lab) atomicAdd(out + 1, 1.f);
    }
    if (g && c < K) {
        const float gv = (p - (c == lab ? 1.f : 0.f)) / ((float)clips * (float)F);
        for (int f = 0; f < F; ++f) g[((long)n * F + f) * ldg + c] = gv;
    }
}

// Dataset-level evaluation of clip logits (acimg_clip_eval).  ONE workgroup of four waves walks all clips in chunks of
// CLIP_EVAL_CHUNK: a wave takes one clip at a time and applies clip_softmax_ce_kernel's per-clip arithmetic (fp32 sum of
// the F frame logits in frame order / F, max-subtracted softmax, lowest index among exact ties); the integer counters and
// the confusion matrix collect in LDS (integer atomics commute), and after each chunk thread 0 folds that chunk's losses
// in clip order onto a double that started from state->loss_sum.  No float atomics, so two identical passes leave
// identical bits.  A label outside [0, K) adds to `invalid` alone (clip_loss 0, clip_pred still the argmax).
static constexpr int CLIP_EVAL_CHUNK = 64;
struct ClipEvalHead {
    double loss_sum;
    long long clips, correct, invalid;
};
static_assert(sizeof(ClipEvalHead) == 32, "include/acimg.h documents a 32-byte head before confusion[K][K]");

__global__ __launch_bounds__(256) void clip_eval_kernel(const float* logits, int ldl, int clips, int F, int K,
                                                        const int* labels, float* clip_loss, int* clip_pred,
                                                        void* state) {
    __shared__ int conf[64 * 64];
    __shared__ float loss_s[CLIP_EVAL_CHUNK];
    __shared__ int cnt[3];              // valid clips, correct, invalid
    ClipEvalHead* head = static_cast<ClipEvalHead*>(state);
    int* confusion = reinterpret_cast<int*>(head + 1);
    const int c = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < K * K; i += 256) conf[i] = 0;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    double acc = threadIdx.x == 0 ? head->loss_sum : 0.0;
    __syncthreads();
    for (int base = 0; base < clips; base += CLIP_EVAL_CHUNK) {
        const int nchunk = min(CLIP_EVAL_CHUNK, clips - base);
        for (int i = wave; i < nchunk; i += 4) {
            const int n = base + i;
            float m = -INFINITY;
            if (c < K) {
                float a = 0.f;
                for (int f = 0; f < F; ++f) a += logits[((long)n * F + f) * ldl + c];
                m = a / (float)F;
            }
            const float mx = wave_max(m);
            const float e = c < K ? expf(m - mx) : 0.f;
            const float se = wave_sum(e);
            int am = c < K && m == mx ? c : 1 << 20;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) am = min(am, __shfl_xor(am, o, 64));
            const int lab = labels[n];
            const bool valid = lab >= 0 && lab < K;
            const float ml = __shfl(m, lab & 63, 64);
            if (c == 0) {
                const float loss = valid ? -(ml - mx - logf(se)) : 0.f;
                loss_s[i] = loss;
                if (clip_loss) clip_loss[n] = loss;
                if (clip_pred) clip_pred[n] = am;
                if (valid) {
                    atomicAdd(&conf[lab * K + am], 1);
                    atomicAdd(&cnt[0], 1);
                    if (am == lab) atomicAdd(&cnt[1], 1);
                } else {
                    atomicAdd(&cnt[2], 1);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < nchunk; ++i) acc += (double)loss_s[i];
        __syncthreads();
    }
    for (int i = threadIdx.x; i < K * K; i += 256) confusion[i] += conf[i];
    if (threadIdx.x == 0) {
        head->loss_sum = acc;
        head->clips += cnt[0];
        head->correct += cnt[1];
        head->invalid += cnt[2];
    }
}

// ------------------------------------------------------------------------------------------
// reconstruction loss (MSE + Huber delta=1) and gradient w.r.t. pre-sigmoid logits
// ------------------------------------------------------------------------------------------
// Ordered combination of per-workgroup partial sums (bit-reproducible, unlike float atomics): every workgroup
// parks its NV partials in `scratch` (agent-scope stores), takes a ticket, and the LAST arriver adds all
// partials in workgroup order with a fixed tree and accumulates them into dst[0..NV).  scratch: int ticket at
// [0] (zero before the first use; the last arriver resets it), partials from float index 4 on.  Call from all
// 256 threads; v is meaningful on thread 0.  scratch == nullptr: plain float atomics.
template <int NV>
__device__ __forceinline__ void ordered_block_sums(const float (&v)[NV], float* scratch, float* dst, float* sm) {
    if (scratch == nullptr) {
        if (threadIdx.x == 0)
#pragma unroll
            for (int i = 0; i < NV; ++i) atomicAdd(&dst[i], v[i]);
        return;
    }
    int* ticket = reinterpret_cast<int*>(scratch);
    float* part = scratch + 4;
    __shared__ int last_flag;
    if (threadIdx.x == 0) {
#pragma unroll
        for (int i = 0; i < NV; ++i)
            __hip_atomic_store(&part[(long)blockIdx.x * NV + i], v[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        const int t = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        last_flag = t == (int)gridDim.x - 1;
        if (last_flag) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
    if (!last_flag) return;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        float acc = 0.f;
        for (int b = threadIdx.x; b < (int)gridDim.x; b += 256)
            acc += __hip_atomic_load(&part[(long)b * NV + i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        acc = block_sum(acc, sm);
        if (threadIdx.x == 0) dst[i] += acc;
    }
    if (threadIdx.x == 0) __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void recon_loss_kernel(const float* yhat, const float* target,
                                                         float* glogit, float* sums, long count,
                                                         float w_mse, float w_huber, float* scratch) {
    __shared__ float sm[32];
    float s_mse = 0.f, s_hub = 0.f;
    const float inv = 1.f / (float)count;
    const long n4 = count >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 yh = reinterpret_cast<const float4*>(yhat)[i];
        const float4 tg = reinterpret_cast<const float4*>(target)[i];
        float4 g;
        const float yv[4] = {yh.x, yh.y, yh.z, yh.w};
        const float tv[4] = {tg.x, tg.y, tg.z, tg.w};
        float gv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const float e = yv[k] - tv[k];
            const float ae = fabsf(e);
            const float q = fminf(ae, 1.f);
            s_mse += e * e;
            s_hub += 0.5f * q * q + (ae - q);
            const float dl = (w_mse * 2.f * e + w_huber * fminf(fmaxf(e, -1.f), 1.f)) * inv;
            gv[k] = dl * yv[k] * (1.f - yv[k]);
        }
        g.x = gv[0];
        g.y = gv[1];
        g.z = gv[2];
        g.w = gv[3];
        if (glogit) reinterpret_cast<float4*>(glogit)[i] = g;
    }
    // tail (count not a multiple of 4)
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long)gridDim.x * 256) {
        const float e = yhat[i] - target[i];
        const float ae = fabsf(e);
        const float q = fminf(ae, 1.f);
        s_mse += e * e;
        s_hub += 0.5f * q * q + (ae - q);
        if (glogit)
            glogit[i] = (w_mse * 2.f * e + w_huber * fminf(fmaxf(e, -1.f), 1.f)) * inv * yhat[i] * (1.f - yhat[i]);
    }
    s_mse = block_sum(s_mse, sm);
    s_hub = block_sum(s_hub, sm);
    const float v[2] = {s_mse, s_hub};
    ordered_block_sums<2>(v, scratch, sums, sm);
}

__global__ __launch_bounds__(256) void sumsq_kernel(const float* x, long n, float* out, float* scratch) {
    __shared__ float sm[32];
    float s = 0.f;
    const long n4 = n >> 2;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n4; i += (long)gridDim.x * 256) {
        const float4 v = reinterpret_cast<const float4*>(x)[i];
        s += v.x * v.x + v.y * v.y + v.z * v.z + v.w * v.w;
    }
    for (long i = (n4 << 2) + (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        s += x[i] * x[i];
    s = block_sum(s, sm);
    const float v[1] = {s};
    ordered_block_sums<1>(v, scratch, out, sm);
}

// per-channel sum of squared errors: out[c] += sum_p (a[p][c]-b[p][c])^2  (C <= 64)
__global__ __launch_bounds__(256) void sqerr_channels_kernel(const float* a, const float* b, long pixels, int C,
                                                             float* out) {
    __shared__ float acc[64];
    if (threadIdx.x < 64) acc[threadIdx.x] = 0.f;
    __syncthreads();
    const long total = pixels * C;
    // each thread keeps a fixed channel: stride of the loop is a multiple of C
    const long stride = ((long)gridDim.x * 256 / C) * C;
    const long start = (long)blockIdx.x * 256 + threadIdx.x;
    float s = 0.f;
    int c = -1;
    if (start < stride) {
        c = (int)(start % C);
        for (long i = start; i < total; i += stride) {
            const float e = a[i] - b[i];
            s += e * e;
        }
    }
    if (c >= 0) atomicAdd(&acc[c], s);
    __syncthreads();
    if (threadIdx.x < C) atomicAdd(&out[threadIdx.x], acc[threadIdx.x]);
}

// out = {mse, huber, latent, reg, total}
__global__ void loss_finalize_kernel(const float* sums, const float* kl, int N, double count, float latent_w,
                                     float half_wd, float w_mse, float w_huber, float* out) {
    __shared__ float sm[32];
    float a = 0.f;
    if (kl)
        for (int i = threadIdx.x; i < N; i += blockDim.x) a += kl[i];
    a = block_sum(a, sm);
    if (threadIdx.x == 0) {
        const float mse = (float)((double)sums[0] / count);
        const float hub = (float)((double)sums[1] / count);
        const float lat = kl ? latent_w * (a / (float)N) : 0.f;
        const float reg = half_wd * sums[2];
        out[0] = mse;
        out[1] = hub;
        out[2] = lat;
        out[3] = reg;
        out[4] = lat + w_mse * mse + w_huber * hub + reg;
    }
}

}  // namespace acimg

using namespace acimg;

extern "C" {

int acimg_latent_fwd(const float* heads, const float* eps, float* z, int ldz, float* sigma,
                     float* kl, int N, int Z, void* stream) {
    hipLaunchKernelGGL(latent_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, heads, eps, z, ldz,
                       sigma, kl, Z);
    return check_launch("latent_fwd");
}

int acimg_latent_bwd(const float* heads, const float* eps, const float* sigma, const float* gz,
                     int ldgz, float kl_weight, float* g_heads, int N, int Z, void* stream) {
    hipLaunchKernelGGL(latent_bwd_kernel, dim3(cdiv((long)N * Z, 256)), dim3(256), 0, (hipStream_t)stream,
                       heads, eps, sigma, gz, ldgz, kl_weight, g_heads, N, Z);
    return check_launch("latent_bwd");
}

int acimg_softplus_fwd(const float* x, int ldx, float* y, int ldy, int rows, int C, void* stream) {
    hipLaunchKernelGGL(softplus_fwd_kernel, dim3(cdiv((long)rows * C, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, y,
                       ldy, rows, C);
    return check_launch("softplus_fwd");
}

int acimg_softplus_bwd(const float* x, int ldx, const float* gy, int ldgy, float* gx, int ldgx, int rows, int C,
                       void* stream) {
    hipLaunchKernelGGL(softplus_bwd_kernel, dim3(cdiv((long)rows * C, 256)), dim3(256), 0, (hipStream_t)stream, x, ldx, gy,
                       ldgy, gx, ldgx, rows, C);
    return check_launch("softplus_bwd");
}

int acimg_latent_linear_fwd(const float* heads, const float* eps, float* z, int ldz, float* kl, int N, int Z,
                            void* stream) {
    hipLaunchKernelGGL(latent_linear_fwd_kernel, dim3(N), dim3(256), 0, (hipStream_t)stream, heads, eps, z, ldz, kl, Z);
    return check_launch("latent_linear_fwd");
}

int acimg_latent_linear_bwd(const float* heads, const float* eps, const float* gz, int ldgz, float kl_weight,
                            float* g_heads, int N, int Z, void* stream) {
    hipLaunchKernelGGL(latent_linear_bwd_kernel, dim3(cdiv((long)N * Z, 256)), dim3(256), 0, (hipStream_t)stream,
                       heads, eps, gz, ldgz, kl_weight, g_heads, N, Z);
    return check_launch("latent_linear_bwd");
}

int acimg_clip_softmax_ce(const float* logits, int ldl, int clips, int F, int K, const int* labels, float* out,
                          float* g_logits, int ldg, void* stream) {
    if (K <= 0 || K > 64 || F <= 0) return fail(ACIMG_EINVAL, "clip_softmax_ce: classes must be in 1..64 (got %d)", K);
    hipLaunchKernelGGL(clip_softmax_ce_kernel, dim3(clips), dim3(64), 0, (hipStream_t)stream, logits, ldl, F, K, labels,
                       clips, out, g_logits, ldg);
    return check_launch("clip_softmax_ce");
}

size_t acimg_clip_eval_state_bytes(int K) {
    if (K <= 0 || K > 64) return 0;
    return sizeof(ClipEvalHead) + (size_t)K * K * sizeof(int);
}

int acimg_clip_eval(const float* logits, int ldl, int clips, int F, int K, const int* labels, float* clip_loss,
                    int* clip_pred, void* state, void* stream) {
    if (K <= 0 || K > 64) return fail(ACIMG_EINVAL, "clip_eval: classes must be in 1..64 (got %d)", K);
    if (F <= 0 || clips <= 0) return fail(ACIMG_EINVAL, "clip_eval: %d clips of %d frames", clips, F);
    if (ldl < K) return fail(ACIMG_EINVAL, "clip_eval: row stride %d < %d classes", ldl, K);
    if (!logits || !labels || !state) return fail(ACIMG_EINVAL, "clip_eval: logits, labels and state must be given");
    if (reinterpret_cast<uintptr_t>(state) & 7) return fail(ACIMG_EINVAL, "clip_eval: state must be 8-byte aligned");
    hipLaunchKernelGGL(clip_eval_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, logits, ldl, clips, F, K, labels,
                       clip_loss, clip_pred, state);
    return check_launch("clip_eval");
}

size_t acimg_loss_scratch_bytes(void) { return (size_t)(4 + 2 * 1024) * sizeof(float); }

int acimg_recon_loss(const float* yhat, const float* target, float* g_logit, float* sums,
                     long count, float w_mse, float w_huber, void* scratch, size_t scratch_bytes, void* stream) {
    if (!aligned16(yhat) || !aligned16(target) || (g_logit && !aligned16(g_logit)))
        return fail(ACIMG_EINVAL, "recon_loss: buffers must be 16-byte aligned");
    if (scratch && scratch_bytes < acimg_loss_scratch_bytes())
        return fail(ACIMG_EWORKSPACE, "recon_loss: scratch %zu < %zu", scratch_bytes, acimg_loss_scratch_bytes());
    // one ordered hand-off (or two float atomics) per workgroup: keep them few
    hipLaunchKernelGGL(recon_loss_kernel, dim3(clamped_blocks(count / 4, 160)), dim3(256), 0, (hipStream_t)stream, yhat,
                       target, g_logit, sums, count, w_mse, w_huber, static_cast<float*>(scratch));
    return check_launch("recon_loss");
}

int acimg_sumsq(const float* x, long n, float* out, void* scratch, size_t scratch_bytes, void* stream) {
    if (!aligned16(x)) return fail(ACIMG_EINVAL, "sumsq: buffer must be 16-byte aligned");
    if (scratch && scratch_bytes < acimg_loss_scratch_bytes())
        return fail(ACIMG_EWORKSPACE, "sumsq: scratch %zu < %zu", scratch_bytes, acimg_loss_scratch_bytes());
    hipLaunchKernelGGL(sumsq_kernel, dim3(clamped_blocks(n / 4, 1024)), dim3(256), 0, (hipStream_t)stream, x, n, out,
                       static_cast<float*>(scratch));
    return check_launch("sumsq");
}

int acimg_sqerr_channels(const float* a, const float* b, long pixels, int C, float* out, void* stream) {
    if (C <= 0 || C > 64) return fail(ACIMG_EINVAL, "sqerr_channels: C must be in 1..64");
    // (the kernel needs a thread per channel: one workgroup already has them)
    hipLaunchKernelGGL(sqerr_channels_kernel, dim3(clamped_blocks(pixels * C, 512)), dim3(256), 0, (hipStream_t)stream, a, b,
                       pixels, C, out);
    return check_launch("sqerr_channels");
}

int acimg_loss_finalize(const float* sums, const float* kl, int N, double count, float latent_w,
                        float half_wd, float w_mse, float w_huber, float* out, void* stream) {
    hipLaunchKernelGGL(loss_finalize_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, sums, kl, N, count,
                       latent_w, half_wd, w_mse, w_huber, out);
    return check_launch("loss_finalize");
}

}  // extern "C"
