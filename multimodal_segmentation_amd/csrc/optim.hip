// Optimiser and regulariser kernels (gfx950, HBM-bound).
//   * Keras 2.1.6 Adam:  m,v EMA;  p -= lr_t * m / (sqrt(v) + eps),  lr_t = lr*sqrt(1-b2^t)/(1-b1^t), eps = 1e-7
//     (call sites models/dafnet.py:93,114,155,161,349 of the reference) over one flat parameter arena:
//     28 B/param (read p,g,m,v; write p,m,v), one launch per trainer.
//   * Spectral regulariser (layers/spectralnorm.py:199-239): 3 power iterations from the constant u0, then
//     alpha*mean|stop_grad(W/sigma) - W| whose gradient is (alpha/N)*sign(W)*sign(1 - 1/sigma).
#include "common.hpp"

__global__ void adam_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                            long n4, long n, float lr_host, const float* __restrict__ lr_dev, float b1, float b2, float eps) {
    // lr_dev != NULL: the bias-corrected step size is read from device memory, so that a captured launch (hipGraph replay of a
    // training step) sees the value of the step being replayed, not the one baked into the launch at capture time
    const float lr_t = lr_dev ? lr_dev[0] : lr_host;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i], pp = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mm[e] = b1 * mm[e] + (1.f - b1) * gg[e];
            vv[e] = b2 * vv[e] + (1.f - b2) * gg[e] * gg[e];
            pp[e] = pp[e] - lr_t * mm[e] / (sqrtf(vv[e]) + eps);
        }
        reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv; reinterpret_cast<f32x4*>(p)[i] = pp;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (long i = n4 * 4; i < n; ++i) {
            m[i] = b1 * m[i] + (1.f - b1) * g[i];
            v[i] = b2 * v[i] + (1.f - b2) * g[i] * g[i];
            p[i] = p[i] - lr_t * m[i] / (sqrtf(v[i]) + eps);
        }
    }
}

// ---- dynamic loss scaling (conf.loss_scale = 'dynamic', build-defined; torch.cuda.amp.GradScaler semantics) --------------------
// Device state of one trainer: scale[1] (a power of two) and st[4] = {found_inf, growth counter, skipped steps, Adam iterations}.
// A step: the seeds multiply their host weights by scale[0] (loss.hip, spec_grad_multi_s_kernel) -> unscale_check_kernel over the
// trainer's gradient arenas (g *= 1/scale, found_inf |= any non-finite element) -> adam_guarded_kernel per arena (no write at all
// when found_inf) -> loss_scale_update_kernel (backoff or growth, counters, flag cleared).  No host read anywhere in the step.
#define LS_MAXA 8
#define LS_BLOCK 256
struct UnscaleBatch { float* g[LS_MAXA]; long n[LS_MAXA]; int blk0[LS_MAXA + 1]; };
// all-ones exponent = +-inf or NaN; a bit test, so that no floating-point mode can fold the check away
__device__ __forceinline__ bool nonfinite_bits(float x) { return (__float_as_uint(x) & 0x7f800000u) == 0x7f800000u; }
__global__ __launch_bounds__(LS_BLOCK) void unscale_check_kernel(UnscaleBatch b, int na, const float* __restrict__ scale,
                                                                 int* __restrict__ st) {
    __shared__ int red[LS_BLOCK / 64];
    int z = 0;                                             // the arena of this block: blocks [blk0[z], blk0[z+1]) cover arena z
    while (z + 1 < na && (int)blockIdx.x >= b.blk0[z + 1]) ++z;
    const int nb = b.blk0[z + 1] - b.blk0[z], bi = (int)blockIdx.x - b.blk0[z];
    float* __restrict__ g = b.g[z];
    const long n = b.n[z], n4 = n >> 2;
    const float inv = 1.f / scale[0];                      // exact: the scale is a power of two
    bool bad = false;
    for (long i = (long)bi * LS_BLOCK + threadIdx.x; i < n4; i += (long)nb * LS_BLOCK) {
        f32x4 x = reinterpret_cast<f32x4*>(g)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            bad |= nonfinite_bits(x[e]);
            x[e] = x[e] * inv;
        }
        reinterpret_cast<f32x4*>(g)[i] = x;
    }
    if (bi == 0 && (long)threadIdx.x < n - n4 * 4) {      // the 1-3 elements past the last full f32x4
        const long i = n4 * 4 + threadIdx.x;
        const float x = g[i];
        bad |= nonfinite_bits(x);
        g[i] = x * inv;
    }
    const unsigned long long w = __ballot(bad);            // wave -> one bit per wave in LDS -> at most one store per block
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = w != 0ull;
    __syncthreads();
    if (threadIdx.x == 0) {
        int any = 0;
#pragma unroll
        for (int k = 0; k < LS_BLOCK / 64; ++k) any |= red[k];
        if (any) st[0] = 1;                                // every writer stores the same value: no atomic needed
    }
}
// Adam with the step skipped when st[0] (found_inf) is set; lr_t(k) of iteration k = st[3] + 1 from the host-written table
// lr_table[j] = lr_t(j + 1), j < table_len (the last entry is lr itself: every later iteration uses it)
__global__ void adam_guarded_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                    long n4, long n, const float* __restrict__ lr_table, int table_len, const int* __restrict__ st,
                                    float b1, float b2, float eps) {
    if (st[0]) return;
    const int k = st[3] + 1;
    const int j = k < 1 ? 0 : (k < table_len ? k : table_len) - 1;      // (the count only grows from 0; clamped all the same)
    const float lr_t = lr_table[j];
    // the update of adam_kernel, statement for statement (bitwise equal results: tests/test_dynamic_loss_scale.py)
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (long)gridDim.x * blockDim.x) {
        const f32x4 gg = reinterpret_cast<const f32x4*>(g)[i];
        f32x4 mm = reinterpret_cast<f32x4*>(m)[i], vv = reinterpret_cast<f32x4*>(v)[i], pp = reinterpret_cast<f32x4*>(p)[i];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            mm[e] = b1 * mm[e] + (1.f - b1) * gg[e];
            vv[e] = b2 * vv[e] + (1.f - b2) * gg[e] * gg[e];
            pp[e] = pp[e] - lr_t * mm[e] / (sqrtf(vv[e]) + eps);
        }
        reinterpret_cast<f32x4*>(m)[i] = mm; reinterpret_cast<f32x4*>(v)[i] = vv; reinterpret_cast<f32x4*>(p)[i] = pp;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (long i = n4 * 4; i < n; ++i) {
            m[i] = b1 * m[i] + (1.f - b1) * g[i];
            v[i] = b2 * v[i] + (1.f - b2) * g[i] * g[i];
            p[i] = p[i] - lr_t * m[i] / (sqrtf(v[i]) + eps);
        }
    }
}
// the largest finite power of two: growth stops there
#define LS_SCALE_MAX 1.7014118346046923e38f
__global__ void loss_scale_update_kernel(float* __restrict__ scale, int* __restrict__ st, int growth_interval) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (st[0]) {                                           // skipped step: back off (never below 1), restart the growth count
        const float s = scale[0] * 0.5f;
        scale[0] = s < 1.f ? 1.f : s;
        st[1] = 0;
        st[2] += 1;
    } else {                                               // applied step: one more Adam iteration, grow after `growth_interval`
        st[3] += 1;
        const int c = st[1] + 1;
        if (c >= growth_interval) {
            if (scale[0] < LS_SCALE_MAX) scale[0] = scale[0] * 2.f;
            st[1] = 0;
        } else {
            st[1] = c;
        }
    }
    st[0] = 0;
}

// ---- power iteration pieces ---------------------------------------------------------------------------
#define SPEC_KS 32
// part[ks][n] = sum_{k in slice} W[k][n] * u[k]
__global__ void spec_gemv_t_kernel(const float* __restrict__ w, const float* __restrict__ u, float* __restrict__ part, int K, int N, int kper) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int k0 = blockIdx.y * kper, k1 = min(K, k0 + kper);
    float a = 0.f;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) a += w[(size_t)k * N + n] * u[k];          // (unrolled: 8 independent row loads in flight, same summation order)
    part[(size_t)blockIdx.y * N + n] = a;
}
// out[k] = sum_n W[k][n] * v[n]  (one wave per row)
__global__ void spec_gemv_n_kernel(const float* __restrict__ w, const float* __restrict__ v, float* __restrict__ out, int K, int N) {
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= K) return;
    float a = 0.f;
    for (int n = lane; n < N; n += 64) a += w[(size_t)k * N + n] * v[n];
    a = wave_sum(a);
    if (lane == 0) out[k] = a;
}
// vec[i] = (sum_s part[s][i]) / || . ||   ; norm_out[0] = || . ||     (single block)
__global__ void spec_normalize_kernel(const float* __restrict__ part, int S, int n, float* __restrict__ vec, float* __restrict__ norm_out) {
    __shared__ float red[17];
    float ss = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float a = 0.f;
        for (int s = 0; s < S; ++s) a += part[(size_t)s * n + i];
        vec[i] = a;
        ss += a * a;
    }
    ss = block_sum(ss, red);
    const float nrm = sqrtf(ss);
    for (int i = threadIdx.x; i < n; i += blockDim.x) vec[i] = vec[i] / nrm;
    if (threadIdx.x == 0 && norm_out) norm_out[0] = nrm;
}
// sum |W| partials
__global__ void spec_abs_partial_kernel(const float* __restrict__ w, long n, float* __restrict__ part) {
    __shared__ float red[17];
    float a = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) a += fabsf(w[i]);
    a = block_sum(a, red);
    if (threadIdx.x == 0) part[blockIdx.x] = a;
}
// loss = alpha * |1/sigma - 1| * mean|W| ; sgn[0] = alpha/N * sign(1 - 1/sigma)
__global__ void spec_final_kernel(const float* __restrict__ part, int nblk, const float* __restrict__ sigma, long n, float alpha,
                                  float* __restrict__ loss, float* __restrict__ sgn) {
    __shared__ float red[17];
    float a = 0.f;
    for (int i = threadIdx.x; i < nblk; i += blockDim.x) a += part[i];
    a = block_sum(a, red);
    if (threadIdx.x == 0) {
        const float d = 1.f - 1.f / sigma[0];
        loss[0] = alpha * fabsf(d) * a / (float)n;
        sgn[0] = (alpha / (float)n) * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
}
// dW = scale * sgn[0] * sign(W)
__global__ void spec_grad_kernel(const float* __restrict__ w, const float* __restrict__ sgn, float scale, long n, float* __restrict__ dw) {
    const float s = sgn[0] * scale;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const float x = w[i];
        dw[i] = x > 0.f ? s : (x < 0.f ? -s : 0.f);
    }
}

// ---- the same, for up to 4 independent matrices per launch (the 4 down-sample blocks of one discriminator) --------------
// Each single-matrix step above is a tiny launch (the largest W is 4096 x 512); a discriminator's regulariser is 4 x 14 of
// them and an iteration evaluates 7 discriminators.  Batched: blockIdx.z (or .y) selects the matrix, grids cover the largest.
#define SPEC_MAXP 4
struct SpecBatch {
    const float* w[SPEC_MAXP];
    const float* u0[SPEC_MAXP];
    float* ws[SPEC_MAXP];          // per-matrix workspace: part | u | v | apart | sigma  (mmseg_spectral_workspace_floats)
    int K[SPEC_MAXP], N[SPEC_MAXP];
};
__device__ __forceinline__ long spec_part_floats_dev(int K, int N) { const long a = (long)SPEC_KS * N; return a > K ? a : K; }
__global__ void spec_gemv_t_multi_kernel(SpecBatch b, int first) {
    const int z = blockIdx.z, K = b.K[z], N = b.N[z];
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const float* w = b.w[z];
    float* part = b.ws[z];
    const float* u = first ? b.u0[z] : part + spec_part_floats_dev(K, N);
    const int kper = (K + SPEC_KS - 1) / SPEC_KS;
    const int k0 = blockIdx.y * kper, k1 = min(K, k0 + kper);
    float a = 0.f;
#pragma unroll 8
    for (int k = k0; k < k1; ++k) a += w[(size_t)k * N + n] * u[k];          // (unrolled: 8 independent row loads in flight, same summation order)
    part[(size_t)blockIdx.y * N + n] = a;
}
__global__ void spec_gemv_n_multi_kernel(SpecBatch b) {
    const int z = blockIdx.y, K = b.K[z], N = b.N[z];
    const int lane = threadIdx.x & 63;
    const int k = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (k >= K) return;
    const float* w = b.w[z];
    float* part = b.ws[z];
    const float* v = part + spec_part_floats_dev(K, N) + K;
    float a = 0.f;
    for (int n = lane; n < N; n += 64) a += w[(size_t)k * N + n] * v[n];
    a = wave_sum(a);
    if (lane == 0) part[k] = a;
}
// which = 0: v = normalise(sum_s part[s][:N]);  which = 1: u = normalise(part[:K]), sigma = the norm
__global__ void spec_normalize_multi_kernel(SpecBatch b, int which) {
    __shared__ float red[17];
    const int z = blockIdx.x, K = b.K[z], N = b.N[z];
    float* part = b.ws[z];
    float* u = part + spec_part_floats_dev(K, N);
    float* v = u + K;
    float* sigma = v + N + 1024;
    const int S = which ? 1 : SPEC_KS, n = which ? K : N;
    float* vec = which ? u : v;
    float ss = 0.f;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        float a = 0.f;
        for (int s = 0; s < S; ++s) a += part[(size_t)s * n + i];
        vec[i] = a;
        ss += a * a;
    }
    ss = block_sum(ss, red);
    const float nrm = sqrtf(ss);
    for (int i = threadIdx.x; i < n; i += blockDim.x) vec[i] = vec[i] / nrm;
    if (threadIdx.x == 0 && which) sigma[0] = nrm;
}
__global__ void spec_abs_partial_multi_kernel(SpecBatch b) {
    __shared__ float red[17];
    const int z = blockIdx.y, K = b.K[z], N = b.N[z];
    const long n = (long)K * N;
    const float* w = b.w[z];
    float* apart = b.ws[z] + spec_part_floats_dev(K, N) + K + N;
    float a = 0.f;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) a += fabsf(w[i]);
    a = block_sum(a, red);
    if (threadIdx.x == 0) apart[blockIdx.x] = a;
}
__global__ void spec_final_multi_kernel(SpecBatch b, float alpha, float* __restrict__ loss, float* __restrict__ sgn) {
    __shared__ float red[17];
    const int z = blockIdx.x, K = b.K[z], N = b.N[z];
    const long n = (long)K * N;
    const float* apart = b.ws[z] + spec_part_floats_dev(K, N) + K + N;
    const float* sigma = apart + 1024;
    float a = 0.f;
    for (int i = threadIdx.x; i < 1024; i += blockDim.x) a += apart[i];
    a = block_sum(a, red);
    if (threadIdx.x == 0) {
        const float d = 1.f - 1.f / sigma[0];
        loss[z] = alpha * fabsf(d) * a / (float)n;
        sgn[z] = (alpha / (float)n) * (d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f));
    }
}
struct SpecGradBatch { const float* w[SPEC_MAXP]; float* dw[SPEC_MAXP]; long n[SPEC_MAXP]; };
// dW[z] += scale * sgn[z] * sign(W[z])
__global__ void spec_grad_multi_kernel(SpecGradBatch b, const float* __restrict__ sgn, float scale) {
    const int z = blockIdx.y;
    const float s = sgn[z] * scale;
    const float* w = b.w[z];
    float* dw = b.dw[z];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < b.n[z]; i += (long)gridDim.x * blockDim.x) {
        const float x = w[i];
        dw[i] += x > 0.f ? s : (x < 0.f ? -s : 0.f);
    }
}
// the same with the factor scale * scale_dev[0] (the dynamic loss scale; a power of two, so the product is exact)
__global__ void spec_grad_multi_s_kernel(SpecGradBatch b, const float* __restrict__ sgn, float scale, const float* __restrict__ scale_dev) {
    const int z = blockIdx.y;
    const float s = sgn[z] * (scale * scale_dev[0]);
    const float* w = b.w[z];
    float* dw = b.dw[z];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < b.n[z]; i += (long)gridDim.x * blockDim.x) {
        const float x = w[i];
        dw[i] += x > 0.f ? s : (x < 0.f ? -s : 0.f);
    }
}

static int spectral_grad4_s(const float* w0, const float* w1, const float* w2, const float* w3, const float* sgn, float* dw0, float* dw1,
                            float* dw2, float* dw3, int n, long n0, long n1, long n2, long n3, float scale, const float* scale_dev, void* stream) {
    if (n < 1 || n > SPEC_MAXP) return (int)hipErrorInvalidValue;
    SpecGradBatch b;
    const float* ws_[4] = {w0, w1, w2, w3};
    float* ds_[4] = {dw0, dw1, dw2, dw3};
    const long ns[4] = {n0, n1, n2, n3};
    long mx = 0;
    for (int i = 0; i < SPEC_MAXP; ++i) {
        const int j = i < n ? i : 0;
        b.w[i] = ws_[j]; b.dw[i] = ds_[j]; b.n[i] = i < n ? ns[i] : 0;
        if (b.n[i] > mx) mx = b.n[i];
    }
    long blocks = (mx + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(spec_grad_multi_s_kernel, dim3((unsigned)blocks, n), dim3(256), 0, (hipStream_t)stream, b, sgn, scale, scale_dev);
    return MMSEG_CHECK_LAUNCH();
}

extern "C" {

int mmseg_adam(float* p, const float* g, float* m, float* v, long n, float lr_t, float b1, float b2, float eps, void* stream) {
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n / 4, n, lr_t, (const float*)nullptr, b1, b2, eps);
    return MMSEG_CHECK_LAUNCH();
}
// the same update with lr_t read from device memory (one float): the form a hipGraph capture of a training step records
int mmseg_adam_p(float* p, const float* g, float* m, float* v, long n, const float* lr_t, float b1, float b2, float eps, void* stream) {
    if (lr_t == nullptr) return (int)hipErrorInvalidValue;
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adam_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n / 4, n, 0.f, lr_t, b1, b2, eps);
    return MMSEG_CHECK_LAUNCH();
}

// ---- dynamic loss scaling ----
// g_i *= 1 / scale[0] over up to 8 arenas in one launch; st[0] = 1 if any element of any arena is +-inf or NaN (never cleared here).
// Arenas must be 16-byte aligned (the f32x4 body); any length (the 1-3 tail elements are handled by the arena's first block).
int mmseg_unscale_check8(float* g0, float* g1, float* g2, float* g3, float* g4, float* g5, float* g6, float* g7, long n0, long n1,
                         long n2, long n3, long n4, long n5, long n6, long n7, int count, const float* scale, int* st, void* stream) {
    if (count < 1 || count > LS_MAXA || scale == nullptr || st == nullptr) return (int)hipErrorInvalidValue;
    float* gs[LS_MAXA] = {g0, g1, g2, g3, g4, g5, g6, g7};
    const long ns[LS_MAXA] = {n0, n1, n2, n3, n4, n5, n6, n7};
    UnscaleBatch b;
    int blocks = 0;
    for (int i = 0; i < LS_MAXA; ++i) {
        b.blk0[i] = blocks;
        b.g[i] = i < count ? gs[i] : gs[0];
        b.n[i] = i < count ? ns[i] : 0;
        if (i >= count) continue;
        if (ns[i] < 0 || (ns[i] > 0 && (gs[i] == nullptr || ((uintptr_t)gs[i] & 15)))) return (int)hipErrorInvalidValue;
        long nb = (ns[i] / 4 + LS_BLOCK - 1) / LS_BLOCK;   // one f32x4 per thread and pass; the largest arena loops
        if (nb > 2048) nb = 2048;
        if (nb < 1) nb = 1;
        blocks += (int)nb;
    }
    b.blk0[LS_MAXA] = blocks;
    hipLaunchKernelGGL(unscale_check_kernel, dim3((unsigned)blocks), dim3(LS_BLOCK), 0, (hipStream_t)stream, b, count, scale, st);
    return MMSEG_CHECK_LAUNCH();
}
// mmseg_adam_p's update, skipped entirely (p, m, v untouched) when st[0] is set; lr_t = lr_table[min(st[3] + 1, table_len) - 1]
int mmseg_adam_guarded(float* p, const float* g, float* m, float* v, long n, const float* lr_table, int table_len, const int* st,
                       float b1, float b2, float eps, void* stream) {
    if (lr_table == nullptr || st == nullptr || table_len < 1) return (int)hipErrorInvalidValue;
    long blocks = (n / 4 + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(adam_guarded_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, p, g, m, v, n / 4, n, lr_table,
                       table_len, st, b1, b2, eps);
    return MMSEG_CHECK_LAUNCH();
}
// end of a step: st[0] set -> scale = max(scale / 2, 1), growth count 0, skipped + 1; else iterations + 1, growth count + 1 and at
// growth_interval scale * 2 (up to 2^127) and count 0.  st[0] cleared.
int mmseg_loss_scale_update(float* scale, int* st, int growth_interval, void* stream) {
    if (scale == nullptr || st == nullptr || growth_interval < 1) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(loss_scale_update_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, scale, st, growth_interval);
    return MMSEG_CHECK_LAUNCH();
}

// workspace floats: max(SPEC_KS*N, K) + K + N + 1024 + 2
static inline long spec_part_floats(int K, int N) { const long a = (long)SPEC_KS * N; return a > K ? a : K; }
long mmseg_spectral_workspace_floats(int K, int N) { return spec_part_floats(K, N) + K + N + 1024 + 2; }

// W: [K][N] (conv kernel reshaped (-1, Cout)), u0: [K].  Writes loss[0] and sgn[0] (see mmseg_spectral_grad).
int mmseg_spectral_fwd(const float* w, const float* u0, float* loss, float* sgn, float* ws, int K, int N, float alpha, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    float* part = ws;                       // max(SPEC_KS * N, K)
    float* u = part + spec_part_floats(K, N);  // K
    float* v = u + K;                       // N
    float* apart = v + N;                   // 1024
    float* sigma = apart + 1024;            // 1
    const int kper = (K + SPEC_KS - 1) / SPEC_KS;
    const float* ucur = u0;
    for (int it = 0; it < 3; ++it) {
        hipLaunchKernelGGL(spec_gemv_t_kernel, dim3((N + 255) / 256, SPEC_KS), dim3(256), 0, st, w, ucur, part, K, N, kper);
        hipLaunchKernelGGL(spec_normalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)part, SPEC_KS, N, v, (float*)nullptr);
        hipLaunchKernelGGL(spec_gemv_n_kernel, dim3((K + 3) / 4), dim3(256), 0, st, w, (const float*)v, part, K, N);
        hipLaunchKernelGGL(spec_normalize_kernel, dim3(1), dim3(1024), 0, st, (const float*)part, 1, K, u, sigma);
        ucur = u;
    }
    // sigma = u^T W v = ||W v|| of the last iteration
    const long n = (long)K * N;
    hipLaunchKernelGGL(spec_abs_partial_kernel, dim3(1024), dim3(256), 0, st, w, n, apart);
    hipLaunchKernelGGL(spec_final_kernel, dim3(1), dim3(256), 0, st, (const float*)apart, 1024, (const float*)sigma, n, alpha, loss, sgn);
    return MMSEG_CHECK_LAUNCH();
}
// The Spectral penalties of up to 4 matrices in one batch of launches (14 instead of 14 per matrix): loss[i], sgn[i] for
// matrix i.  ws = the matrices' workspaces back to back (mmseg_spectral_workspace_floats(K_i, N_i) floats each).
int mmseg_spectral_fwd4(const float* w0, const float* w1, const float* w2, const float* w3, const float* u0, const float* u1,
                        const float* u2, const float* u3, float* loss, float* sgn, float* ws, int n, int K0, int N0, int K1, int N1,
                        int K2, int N2, int K3, int N3, float alpha, void* stream) {
    if (n < 1 || n > SPEC_MAXP) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    SpecBatch b;
    const float* ws_[4] = {w0, w1, w2, w3};
    const float* us_[4] = {u0, u1, u2, u3};
    const int Ks[4] = {K0, K1, K2, K3}, Ns[4] = {N0, N1, N2, N3};
    int maxK = 0, maxN = 0;
    long off = 0;
    for (int i = 0; i < SPEC_MAXP; ++i) {
        const int j = i < n ? i : 0;
        b.w[i] = ws_[j]; b.u0[i] = us_[j]; b.K[i] = Ks[j]; b.N[i] = Ns[j];
        b.ws[i] = ws + (i < n ? off : 0);
        if (i < n) {
            if (Ks[i] < 1 || Ns[i] < 1) return (int)hipErrorInvalidValue;
            off += mmseg_spectral_workspace_floats(Ks[i], Ns[i]);
            if (Ks[i] > maxK) maxK = Ks[i];
            if (Ns[i] > maxN) maxN = Ns[i];
        }
    }
    for (int it = 0; it < 3; ++it) {
        hipLaunchKernelGGL(spec_gemv_t_multi_kernel, dim3((maxN + 255) / 256, SPEC_KS, n), dim3(256), 0, st, b, it == 0 ? 1 : 0);
        hipLaunchKernelGGL(spec_normalize_multi_kernel, dim3(n), dim3(1024), 0, st, b, 0);
        hipLaunchKernelGGL(spec_gemv_n_multi_kernel, dim3((maxK + 3) / 4, n), dim3(256), 0, st, b);
        hipLaunchKernelGGL(spec_normalize_multi_kernel, dim3(n), dim3(1024), 0, st, b, 1);
    }
    hipLaunchKernelGGL(spec_abs_partial_multi_kernel, dim3(1024, n), dim3(256), 0, st, b);
    hipLaunchKernelGGL(spec_final_multi_kernel, dim3(n), dim3(256), 0, st, b, alpha, loss, sgn);
    return MMSEG_CHECK_LAUNCH();
}
// dW_i += scale * sgn[i] * sign(W_i): the penalties' gradients accumulated straight into the gradient arena
int mmseg_spectral_grad4(const float* w0, const float* w1, const float* w2, const float* w3, const float* sgn, float* dw0, float* dw1,
                         float* dw2, float* dw3, int n, long n0, long n1, long n2, long n3, float scale, void* stream) {
    if (n < 1 || n > SPEC_MAXP) return (int)hipErrorInvalidValue;
    SpecGradBatch b;
    const float* ws_[4] = {w0, w1, w2, w3};
    float* ds_[4] = {dw0, dw1, dw2, dw3};
    const long ns[4] = {n0, n1, n2, n3};
    long mx = 0;
    for (int i = 0; i < SPEC_MAXP; ++i) {
        const int j = i < n ? i : 0;
        b.w[i] = ws_[j]; b.dw[i] = ds_[j]; b.n[i] = i < n ? ns[i] : 0;
        if (b.n[i] > mx) mx = b.n[i];
    }
    long blocks = (mx + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    hipLaunchKernelGGL(spec_grad_multi_kernel, dim3((unsigned)blocks, n), dim3(256), 0, (hipStream_t)stream, b, sgn, scale);
    return MMSEG_CHECK_LAUNCH();
}
// the same with the factor scale * scale_dev[0] (dynamic loss scale in device memory)
int mmseg_spectral_grad4_s(const float* w0, const float* w1, const float* w2, const float* w3, const float* sgn, float* dw0, float* dw1,
                           float* dw2, float* dw3, int n, long n0, long n1, long n2, long n3, float scale, const float* scale_dev,
                           void* stream) {
    if (scale_dev == nullptr) return (int)hipErrorInvalidValue;
    return spectral_grad4_s(w0, w1, w2, w3, sgn, dw0, dw1, dw2, dw3, n, n0, n1, n2, n3, scale, scale_dev, stream);
}
int mmseg_spectral_grad(const float* w, const float* sgn, float scale, long n, float* dw, void* stream) {
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(spec_grad_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, w, sgn, scale, n, dw);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
