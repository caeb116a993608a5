// MR intensity augmentation of a gathered training batch on the device (gfx950; build-defined, after nnU-Net's gamma / contrast /
// noise / blur transforms and TorchIO's RandomBiasField).  x [B,H,W,C] fp32 is an image array of one batch as the gather kernels of
// augment.hip wrote it; every sample has its own draws (utils/augment.intensity_draws, Philox words on the host).  With lo, hi, mean the
// minimum, maximum and mean of the sample BEFORE any intensity operation, all arithmetic in fp64 and one rounding to fp32 at the end:
//   blur      v = scipy.ndimage.gaussian_filter(x, sigma, mode='reflect', truncate=4.0) over the two spatial axes, rounded to fp32
//   bias      v = lo + (v - lo) * exp(f[r, c]),  f = component 0 of an mmseg_elastic_field of this array
//   contrast  v = mean + (v - mean) * c
//   clip      v = min(max(v, lo), hi)            (only after bias or contrast)
//   gamma     t = clamp((v - lo) / (hi - lo), 0, 1);  t = invert ? 1 - pow(1 - t, g) : pow(t, g);  v = lo + t * (hi - lo)     (hi > lo)
//   noise     v += std * sqrt(-2 ln u1) * cos(2 pi u2),  u1 = ((P[0] >> 8) + 1) * 2^-24, u2 = (P[1] >> 8) * 2^-24,
//             P = Philox4x32-10(counter (e, b, array, 3), key (seed, batch)),  e = (r*W + c)*C + ch
// Three entry points, all bandwidth-bound:
//   mmseg_intensity_stats   two launches: per-block (min, max, sum) partials (wave64 __shfl_xor + LDS), then one block per sample folds
//                           its <= AUG_MAXBLK partials.  Every sum runs in a fixed order: the table is bitwise reproducible.
//   mmseg_intensity_blur    two launches, the radius and the weight row read per sample: along W into an fp64 scratch, then along H.
//   mmseg_intensity_apply   one launch, in place: one read and one write per element of the samples that have an operation on.
#include "common.hpp"
#include "philox.hpp"

#define IN_MAXBLK 256        // = AUG_MAXBLK of augment.hip: blocks per sample and threads per block of the strided kernels
#define IN_MAXR 32           // INTENSITY_BLUR_MAX_RADIUS of ops.py
#define IN_TW 128            // pixels of one row per block, pass along W
#define IN_TH 64             // rows per block, pass along H
#define IN_TC 8              // columns (of the flat W*C axis) per block, pass along H
#define IN_P 5               // doubles per sample of the parameter table: flags, c, g, invert, std
#define IN_BIAS 1
#define IN_CONTRAST 2
#define IN_GAMMA 4
#define IN_NOISE 8

// block-wide (min, max, sum) in a fixed order: xor butterfly inside each wave, then thread 0 folds the waves in wave order
__device__ __forceinline__ void in_stats_block(double lo, double hi, double s, double* dst) {
    __shared__ double red[3][IN_MAXBLK / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
        s += __shfl_xor(s, o, 64);
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) { red[0][wid] = lo; red[1][wid] = hi; red[2][wid] = s; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) { lo = fmin(lo, red[0][w]); hi = fmax(hi, red[1][w]); s += red[2][w]; }
        dst[0] = lo;
        dst[1] = hi;
        dst[2] = s;
    }
}

// grid (nblk, B), block IN_MAXBLK: block j of sample b strides over the sample's per elements -> part[b][j][3]
__global__ void __launch_bounds__(IN_MAXBLK) intensity_stats_kernel(const float* __restrict__ x, double* __restrict__ part, int per) {
    const int b = blockIdx.y;
    const float* src = x + (size_t)b * per;
    double lo = INFINITY, hi = -INFINITY, s = 0.0;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
        const double v = (double)src[e];
        lo = fmin(lo, v);
        hi = fmax(hi, v);
        s += v;
    }
    in_stats_block(lo, hi, s, part + ((size_t)b * gridDim.x + blockIdx.x) * 3);
}

// grid (B), block IN_MAXBLK: thread j holds partial j (nblk <= IN_MAXBLK) -> stats[b] = (min, max, sum)
__global__ void __launch_bounds__(IN_MAXBLK) intensity_stats_fold_kernel(const double* __restrict__ part, double* __restrict__ stats,
                                                                        int nblk) {
    const int b = blockIdx.x, j = threadIdx.x;
    double lo = INFINITY, hi = -INFINITY, s = 0.0;
    if (j < nblk) {
        const double* p = part + ((size_t)b * nblk + j) * 3;
        lo = p[0];
        hi = p[1];
        s = p[2];
    }
    in_stats_block(lo, hi, s, stats + (size_t)b * 3);
}

// Pass along W.  grid (ceil(W / IN_TW), H, B*C), block IN_TW: pixels c0-R .. c0+IN_TW-1+R of one row and one channel in LDS (reflected),
// R + 1 weights of the sample's row, fp64 sums in the order w_0 x_0 + sum_k w_k (x_-k + x_+k) -> ws [B,H,W,C] fp64.  A sample with
// R == 0 is skipped (the second pass copies it).  LDS: (IN_TW + 2 IN_MAXR) * 4 + (IN_MAXR + 1) * 8 = 1032 bytes per block.
__global__ void __launch_bounds__(IN_TW) intensity_blur_w_kernel(const float* __restrict__ x, const int* __restrict__ radius,
                                                                 const double* __restrict__ wts, double* __restrict__ ws, int H, int W,
                                                                 int C) {
    __shared__ float t[IN_TW + 2 * IN_MAXR];
    __shared__ double wk[IN_MAXR + 1];
    const int b = blockIdx.z / C, ch = blockIdx.z - b * C, r = blockIdx.y, c0 = blockIdx.x * IN_TW;
    const int R = min(radius[b], IN_MAXR);                         // uniform over the block; the cap keeps every LDS index inside
    if (R <= 0) return;
    const size_t row = ((size_t)b * H + r) * W;
    for (int i = threadIdx.x; i <= R; i += IN_TW) wk[i] = wts[(size_t)b * (IN_MAXR + 1) + i];
    for (int i = threadIdx.x; i < IN_TW + 2 * R; i += IN_TW) t[i] = x[(row + el_reflect(c0 - R + i, W)) * C + ch];
    __syncthreads();
    const int c = c0 + threadIdx.x;
    if (c >= W) return;
    const int q = threadIdx.x + R;
    double a = wk[0] * (double)t[q];
    for (int k = 1; k <= R; ++k) a += wk[k] * ((double)t[q - k] + (double)t[q + k]);
    ws[(row + c) * C + ch] = a;
}

// Pass along H over the flat [H, W*C] matrix.  grid (ceil(W*C / IN_TC), ceil(H / IN_TH), B), block IN_TC x IN_TH/2: rows r0-R ..
// r0+IN_TH-1+R of IN_TC columns of ws in LDS, two output rows per thread, rounded to fp32.  R == 0: the sample is copied from x bit
// for bit.  LDS, sized for IN_MAXR = 32: (IN_TH + 2 IN_MAXR) * IN_TC * 8 + (IN_MAXR + 1) * 8 = 8456 bytes per block of 4 waves, so
// the 160 KiB of a CU would hold 19 blocks; the compiler's 68 VGPRs admit 7 waves per SIMD, i.e. 7 blocks per CU: the registers, not the
// LDS, bound the occupancy.
__global__ void __launch_bounds__(IN_TC * IN_TH / 2) intensity_blur_h_kernel(const float* __restrict__ x, const int* __restrict__ radius,
                                                                             const double* __restrict__ wts,
                                                                             const double* __restrict__ ws, float* __restrict__ out,
                                                                             int H, int WC) {
    __shared__ double t[(IN_TH + 2 * IN_MAXR) * IN_TC];
    __shared__ double wk[IN_MAXR + 1];
    const int b = blockIdx.z, r0 = blockIdx.y * IN_TH, c0 = blockIdx.x * IN_TC;
    const int tc = threadIdx.x % IN_TC, tr = threadIdx.x / IN_TC;
    const int R = min(radius[b], IN_MAXR);                         // uniform over the block
    const int c = c0 + tc;
    if (R <= 0) {
        if (c < WC)
            for (int q = 0; q < 2; ++q) {
                const int r = r0 + tr + q * (IN_TH / 2);
                if (r < H) out[((size_t)b * H + r) * WC + c] = x[((size_t)b * H + r) * WC + c];
            }
        return;
    }
    for (int i = threadIdx.x; i <= R; i += blockDim.x) wk[i] = wts[(size_t)b * (IN_MAXR + 1) + i];
    const int nrow = IN_TH + 2 * R;
    for (int i = tr; i < nrow; i += IN_TH / 2)
        t[i * IN_TC + tc] = c < WC ? ws[((size_t)b * H + el_reflect(r0 - R + i, H)) * WC + c] : 0.0;
    __syncthreads();
    if (c >= WC) return;
    const double* lo = t + (tr + R) * IN_TC + tc;                  // output row r0 + tr
    const double* hi = lo + (IN_TH / 2) * IN_TC;                   // output row r0 + tr + IN_TH / 2
    double a0 = wk[0] * lo[0], a1 = wk[0] * hi[0];
    for (int k = 1; k <= R; ++k) {
        const double w = wk[k];
        const int d = k * IN_TC;
        a0 += w * (lo[-d] + lo[d]);
        a1 += w * (hi[-d] + hi[d]);
    }
    const int r = r0 + tr;
    if (r < H) out[((size_t)b * H + r) * WC + c] = (float)a0;
    if (r + IN_TH / 2 < H) out[((size_t)b * H + r + IN_TH / 2) * WC + c] = (float)a1;
}

// grid (nblk, B), block IN_MAXBLK, in place.  A sample whose flags are 0 is neither read nor written; Philox, log, sqrt and cos run
// only in the samples whose noise is on.
__global__ void __launch_bounds__(IN_MAXBLK) intensity_apply_kernel(float* __restrict__ x, const double* __restrict__ params,
                                                                   const double* __restrict__ stats, const float* __restrict__ field,
                                                                   uint32_t seed, uint32_t batch, uint32_t array, int HW, int C, int per) {
    const int b = blockIdx.y;
    const double* p = params + (size_t)b * IN_P;
    const int flags = (int)p[0];                                   // uniform over the block
    if (!(flags & (IN_BIAS | IN_CONTRAST | IN_GAMMA | IN_NOISE))) return;
    const double lo = stats[(size_t)b * 3], hi = stats[(size_t)b * 3 + 1], mean = stats[(size_t)b * 3 + 2] / (double)per;
    const double range = hi - lo;
    const bool bias = (flags & IN_BIAS) && field, contrast = flags & IN_CONTRAST, gamma = (flags & IN_GAMMA) && hi > lo;
    const bool noise = flags & IN_NOISE, invert = p[3] != 0.0;
    const double c = p[1], g = p[2], sd = p[4];
    float* dst = x + (size_t)b * per;
    const float* f = field + (size_t)b * HW * 2;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
        double v = (double)dst[e];
        if (bias) v = lo + (v - lo) * exp((double)f[(size_t)(e / C) * 2]);
        if (contrast) v = mean + (v - mean) * c;
        if (bias || contrast) v = fmin(fmax(v, lo), hi);
        if (gamma) {
            double u = fmin(fmax((v - lo) / range, 0.0), 1.0);
            u = invert ? 1.0 - pow(1.0 - u, g) : pow(u, g);
            v = lo + u * range;
        }
        if (noise) {
            uint32_t p0, p1;
            philox4x32_10((uint32_t)e, (uint32_t)b, array, 3u, seed, batch, p0, p1);
            const double u1 = (double)((p0 >> 8) + 1u) * 0x1p-24, u2 = (double)(p1 >> 8) * 0x1p-24;
            v += sd * (sqrt(-2.0 * log(u1)) * cos(6.283185307179586 * u2));
        }
        dst[e] = (float)v;
    }
}

static int in_blocks(long per) {
    const long n = (per + IN_MAXBLK - 1) / IN_MAXBLK;
    return (int)(n < IN_MAXBLK ? n : IN_MAXBLK);
}

// 32-bit element indices inside a sample (the gather kernels' limit, below the 2^32 of the noise counter)
static bool intensity_shape_ok(int B, int H, int W, int C) {
    return B >= 1 && H >= 1 && W >= 1 && C >= 1 && B <= 65535 && (long)H * W * C <= 0x7fffffffL - (long)IN_MAXBLK * IN_MAXBLK;
}

extern "C" {

// doubles of the scratch buffer that mmseg_intensity_stats (its partials) or mmseg_intensity_blur (the fp64 image between its passes)
// needs, whichever is larger; 0 for a shape they refuse.  Launches nothing.
long mmseg_intensity_workspace_doubles(int B, int H, int W, int C) {
    if (!intensity_shape_ok(B, H, W, C)) return 0;
    const long per = (long)H * W * C, part = 3L * in_blocks(per);
    return B * (per > part ? per : part);
}

// x [B,H,W,C] fp32 -> stats [B,3] fp64: (min, max, sum) of every sample
int mmseg_intensity_stats(const float* x, double* stats, double* ws, int B, int H, int W, int C, void* stream) {
    if (B <= 0) return 0;
    if (!intensity_shape_ok(B, H, W, C) || !x || !stats || !ws) return (int)hipErrorInvalidValue;
    const long per = (long)H * W * C;
    const int nblk = in_blocks(per);
    hipLaunchKernelGGL(intensity_stats_kernel, dim3(nblk, B), dim3(IN_MAXBLK), 0, (hipStream_t)stream, x, ws, (int)per);
    const int rc = MMSEG_CHECK_LAUNCH();
    if (rc) return rc;
    hipLaunchKernelGGL(intensity_stats_fold_kernel, dim3(B), dim3(IN_MAXBLK), 0, (hipStream_t)stream, ws, stats, nblk);
    return MMSEG_CHECK_LAUNCH();
}

// x [B,H,W,C] fp32, radius [B] int32 (0: copy the sample; values above 32 are read as 32), weights [B,33] fp64 (row b: w_0 .. w_R[b] of
// the normalised kernel), out [B,H,W,C] fp32 (not x)
int mmseg_intensity_blur(const float* x, const int* radius, const double* weights, float* out, double* ws, int B, int H, int W, int C,
                         void* stream) {
    if (B <= 0) return 0;
    if (!intensity_shape_ok(B, H, W, C) || H > 65535 || (long)B * C > 65535 || (long)H * W > 0x3fffffffL || !x || !radius || !weights || !out || !ws || out == x)
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(intensity_blur_w_kernel, dim3((W + IN_TW - 1) / IN_TW, H, B * C), dim3(IN_TW), 0, (hipStream_t)stream, x, radius,
                       weights, ws, H, W, C);
    const int rc = MMSEG_CHECK_LAUNCH();
    if (rc) return rc;
    const int WC = W * C;
    hipLaunchKernelGGL(intensity_blur_h_kernel, dim3((WC + IN_TC - 1) / IN_TC, (H + IN_TH - 1) / IN_TH, B), dim3(IN_TC * IN_TH / 2), 0,
                       (hipStream_t)stream, x, radius, weights, ws, out, H, WC);
    return MMSEG_CHECK_LAUNCH();
}

// x [B,H,W,C] fp32 in place, params [B,5] fp64 (flags = 1 bias + 2 contrast + 4 gamma + 8 noise, c, g, invert != 0, std), stats [B,3]
// fp64 of mmseg_intensity_stats, field [B,H,W,2] fp32 (component 0 is read) or nullptr (no sample is biased)
int mmseg_intensity_apply(float* x, const double* params, const double* stats, const float* field, int seed, int batch, int array,
                          int B, int H, int W, int C, void* stream) {
    if (B <= 0) return 0;
    if (!intensity_shape_ok(B, H, W, C) || !x || !params || !stats) return (int)hipErrorInvalidValue;
    const long per = (long)H * W * C;
    hipLaunchKernelGGL(intensity_apply_kernel, dim3(in_blocks(per), B), dim3(IN_MAXBLK), 0, (hipStream_t)stream, x, params, stats, field,
                       (uint32_t)seed, (uint32_t)batch, (uint32_t)array, H * W, C, (int)per);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
