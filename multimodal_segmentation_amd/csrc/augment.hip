// Batch assembly + rotation augmentation on the device (gfx950).
//
// The reference augments on the host, one slice at a time: keras ImageDataGenerator(rotation_range=20).flow(...)
// (model_executors/base_executor.py:37-78,103-110) rotates every sample of a batch about the image centre with
// scipy.ndimage.affine_transform(order=1, mode='nearest') per channel.  Here the whole training set stays resident in
// HBM and one launch gathers the B slices of the batch (rows[]) and resamples them with a per-sample 2x3 matrix:
//     src(r, c) = (m0*r + m1*c + m2,  m3*r + m4*c + m5)      coordinates clamped to the image ('nearest' extension),
//     out[b, r, c, :] = bilinear(data[rows[b]], src(r, c))         (order 1; order 0 = the tap at floor(src + 0.5))
// HBM-bound: one read of ~B slices + one write.  One thread per output element; consecutive threads walk the
// channel-fastest NHWC order, so stores are fully coalesced and the 4 taps of neighbouring pixels share cache lines.
#include "common.hpp"

__global__ void affine_gather_kernel(const float* __restrict__ data, const int* __restrict__ rows, const float* __restrict__ mat,
                                     float* __restrict__ out, int H, int W, int C, long per_sample, int order) {
    const int b = blockIdx.y;
    const long e = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= per_sample) return;
    const int ch = (int)(e % C);
    const int p = (int)(e / C);
    const int r = p / W, c = p - r * W;
    const float* m = mat + b * 6;
    float sr = m[0] * (float)r + m[1] * (float)c + m[2];
    float sc = m[3] * (float)r + m[4] * (float)c + m[5];
    sr = fminf(fmaxf(sr, 0.f), (float)(H - 1));
    sc = fminf(fmaxf(sc, 0.f), (float)(W - 1));
    if (order == 0) { sr = floorf(sr + 0.5f); sc = floorf(sc + 0.5f); }
    const int r0 = min((int)sr, H - 1), c0 = min((int)sc, W - 1);
    const int r1 = min(r0 + 1, H - 1), c1 = min(c0 + 1, W - 1);
    const float ar = sr - (float)r0, ac = sc - (float)c0;
    const float* src = data + (size_t)(rows ? rows[b] : b) * per_sample + ch;
    const float v00 = src[((size_t)r0 * W + c0) * C], v01 = src[((size_t)r0 * W + c1) * C];
    const float v10 = src[((size_t)r1 * W + c0) * C], v11 = src[((size_t)r1 * W + c1) * C];
    out[(size_t)b * per_sample + e] = (1.f - ar) * ((1.f - ac) * v00 + ac * v01) + ar * ((1.f - ac) * v10 + ac * v11);
}

extern "C" {

// data [N,H,W,C] (N > max(rows)), rows [B] int32 or nullptr (= identity), mat [B,6], out [B,H,W,C]
int mmseg_affine_gather(const float* data, const int* rows, const float* mat, float* out, int B, int H, int W, int C, int order,
                        void* stream) {
    if (B <= 0) return 0;
    if (H < 1 || W < 1 || C < 1 || B > 65535 || order < 0 || order > 1) return (int)hipErrorInvalidValue;
    const long per = (long)H * W * C;
    dim3 grid((unsigned)((per + 255) / 256), B);
    hipLaunchKernelGGL(affine_gather_kernel, grid, dim3(256), 0, (hipStream_t)stream, data, rows, mat, out, H, W, C, per, order);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// The full ImageDataGenerator pixel augmentation (keras 2.1.6 random_transform; the reference's switches are
// get_datagen_params(), model_executors/base_executor.py:103-110): rotation, shift, shear and zoom composed into one 2x3
// matrix per sample on the host, horizontal / vertical flips folded into that matrix (a flip after the resample is a
// reflection of the OUTPUT grid, i.e. a right factor of the matrix -- exact, and it commutes with the channel shift), four
// fill modes, and keras' random_channel_shift: out = clip(x_c + shift[b, c], min(x), max(x)) with min / max over the whole
// transformed sample.
//
// Boundary rules = scipy.ndimage.affine_transform (the call keras makes), probed against scipy 1.15.3 in 1-D and 2-D at
// order 0 and 1 (every coordinate of a dense grid incl. half-integers and the exact edges, n = 1..8).  Per axis, coordinate c,
// extent n, computed in fp64 (as scipy does):
//   nearest   c = clamp(c, 0, n-1)
//   constant  c < 0 or c > n-1 on either axis -> cval (strict: -1e-9 and n-1+1e-9 are outside); else interpolate inside
//   reflect   half-sample symmetric, period 2n: t = c mod 2n in [0, 2n); t >= n -> 2n-1-t; taps beyond the edge reflect
//             (-1 -> 0, n -> n-1)
//   wrap      scipy's legacy 'wrap', period n-1 (not 'grid-wrap'): c < 0 -> (n-1) - fmod(-c, n-1) in (0, n-1];
//             c > n-1 -> fmod(c, n-1) in [0, n-1); c in [0, n-1] unchanged
//   (reflect / wrap with n == 1: c = 0)
//   order 1: bilinear on taps floor(c), floor(c)+1 (a tap beyond n-1 carries weight 0 or reflects); order 0: tap floor(c + 0.5)
// Bitwise: a zero interpolation weight skips its taps, so an identity matrix (and a pure flip) copies the input bit for bit.
//
// Launches: augment_gather_kernel (one read of the source slices, one write; with the channel shift it also writes per-block
// (min, max) partials, wave64 __shfl_xor + LDS), then -- only with the channel shift -- augment_shift_kernel, which folds the
// <= AUG_MAXBLK partials of its sample and applies shift + clip in place.  min / max are order independent: the output is
// bitwise reproducible.
#define AUG_MAXBLK 256
#define AUG_NEAREST 0
#define AUG_CONSTANT 1
#define AUG_REFLECT 2
#define AUG_WRAP 3

__device__ __forceinline__ double aug_map(double c, int n, int mode, bool& inside) {
    const double hi = (double)(n - 1);
    if (c >= 0.0 && c <= hi) return c;
    switch (mode) {
        case AUG_CONSTANT: inside = false; return 0.0;
        case AUG_REFLECT: {
            if (n == 1) return 0.0;
            const double p = 2.0 * n;
            const double t = c - p * floor(c / p);
            return t >= (double)n ? p - 1.0 - t : t;
        }
        case AUG_WRAP:
            if (n == 1) return 0.0;
            return c < 0.0 ? hi - fmod(-c, hi) : fmod(c, hi);
        default: return c < 0.0 ? 0.0 : hi;        // nearest (also NaN-safe: the taps are clamped below)
    }
}

__device__ __forceinline__ int aug_tap(int i, int n, int mode) {
    if (mode == AUG_REFLECT) {
        if (i < 0) i = -1 - i;
        if (i >= n) i = 2 * n - 1 - i;
    }
    return min(max(i, 0), n - 1);                  // also keeps every read inside the slice whatever the coordinate
}

__device__ __forceinline__ void aug_minmax_block(float lo, float hi, float* part) {
    __shared__ float red[2][AUG_MAXBLK / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if (lane == 0) { red[0][wid] = lo; red[1][wid] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < nw; ++w) { lo = fminf(lo, red[0][w]); hi = fmaxf(hi, red[1][w]); }
        part[0] = lo;
        part[1] = hi;
    }
}

// grid (nblk, B), block AUG_MAXBLK; nblk <= AUG_MAXBLK blocks stride over the sample's per = H*W*C elements (NHWC order,
// channel fastest: coalesced stores; neighbouring pixels' taps share cache lines)
__global__ void __launch_bounds__(AUG_MAXBLK) augment_gather_kernel(
        const float* __restrict__ data, const int* __restrict__ rows, const double* __restrict__ mat, float* __restrict__ out,
        float* __restrict__ part, int N, int H, int W, int C, int per, int order, int mode, float cval) {
    const int b = blockIdx.y;
    const int j = rows ? rows[b] : b;
    const double* m = mat + (size_t)b * 6;
    const double m0 = m[0], m1 = m[1], m2 = m[2], m3 = m[3], m4 = m[4], m5 = m[5];
    const bool row_ok = j >= 0 && j < N;
    const float* src = data + (size_t)(row_ok ? j : 0) * per;
    float* dst = out + (size_t)b * per;
    float lo = INFINITY, hi = -INFINITY;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x) {
        const int ch = e % C;
        const int p = e / C;
        const int r = p / W, c = p - r * W;
        bool inside = row_ok;
        const double sr = aug_map(m0 * r + m1 * c + m2, H, mode, inside);
        const double sc = aug_map(m3 * r + m4 * c + m5, W, mode, inside);
        float v = row_ok ? cval : __builtin_nanf("");
        if (inside) {
            const float* s = src + ch;
            if (order == 0) {
                const int rr = aug_tap((int)floor(sr + 0.5), H, mode), cc = aug_tap((int)floor(sc + 0.5), W, mode);
                v = s[((size_t)rr * W + cc) * C];
            } else {
                const double fr = floor(sr), fc = floor(sc);
                const float ar = (float)(sr - fr), ac = (float)(sc - fc);
                const int r0 = aug_tap((int)fr, H, mode), c0 = aug_tap((int)fc, W, mode);
                const float v00 = s[((size_t)r0 * W + c0) * C];
                float top = v00, bot = 0.f;
                int c1 = c0;
                if (ac != 0.f) {
                    c1 = aug_tap((int)fc + 1, W, mode);
                    top = (1.f - ac) * v00 + ac * s[((size_t)r0 * W + c1) * C];
                }
                if (ar != 0.f) {
                    const int r1 = aug_tap((int)fr + 1, H, mode);
                    const float v10 = s[((size_t)r1 * W + c0) * C];
                    bot = ac != 0.f ? (1.f - ac) * v10 + ac * s[((size_t)r1 * W + c1) * C] : v10;
                    v = (1.f - ar) * top + ar * bot;
                } else {
                    v = top;
                }
            }
        }
        dst[e] = v;
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    if (part) aug_minmax_block(lo, hi, part + ((size_t)b * gridDim.x + blockIdx.x) * 2);
}

// grid (nblk, B), block AUG_MAXBLK: fold the nblk partials of sample b (the same fixed set in every block), then
// out = clip(out + shift[b, c], lo, hi) in place
__global__ void __launch_bounds__(AUG_MAXBLK) augment_shift_kernel(float* __restrict__ out, const float* __restrict__ shift,
                                                                   const float* __restrict__ part, int C, int per) {
    __shared__ float mm[2];
    const int b = blockIdx.y;
    const float* pp = part + (size_t)b * gridDim.x * 2;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < (int)gridDim.x; i += blockDim.x) { lo = fminf(lo, pp[2 * i]); hi = fmaxf(hi, pp[2 * i + 1]); }
    aug_minmax_block(lo, hi, mm);
    __syncthreads();
    lo = mm[0];
    hi = mm[1];
    const float* sh = shift + (size_t)b * C;
    float* dst = out + (size_t)b * per;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < per; e += gridDim.x * blockDim.x)
        dst[e] = fminf(fmaxf(dst[e] + sh[e % C], lo), hi);
}

static int aug_blocks(long per) {
    const long n = (per + AUG_MAXBLK - 1) / AUG_MAXBLK;
    return (int)(n < AUG_MAXBLK ? n : AUG_MAXBLK);
}

extern "C" {

long mmseg_augment_workspace_floats(int B, int H, int W, int C) {
    if (B < 1 || H < 1 || W < 1 || C < 1) return 0;
    return 2L * B * aug_blocks((long)H * W * C);
}

// data [N,H,W,C], rows [B] int32 or nullptr (= identity; a row outside [0, N) yields NaN, nothing is read), mat [B,6] fp64,
// shift [B,C] or nullptr (no channel shift), out [B,H,W,C], ws: mmseg_augment_workspace_floats(B, H, W, C) floats (unused
// without shift).  fill_mode: 0 nearest, 1 constant (cval), 2 reflect, 3 wrap.
int mmseg_augment_gather(const float* data, const int* rows, const double* mat, const float* shift, float* out, float* ws, int N, int B,
                         int H, int W, int C, int order, int fill_mode, float cval, void* stream) {
    if (B <= 0) return 0;
    if (N < 1 || H < 1 || W < 1 || C < 1 || B > 65535 || order < 0 || order > 1 || fill_mode < AUG_NEAREST || fill_mode > AUG_WRAP ||
        (shift && !ws))
        return (int)hipErrorInvalidValue;
    const long per = (long)H * W * C;
    if (per > 0x7fffffffL - (long)AUG_MAXBLK * AUG_MAXBLK) return (int)hipErrorInvalidValue;      // 32-bit element indices
    const dim3 grid((unsigned)aug_blocks(per), B);
    hipLaunchKernelGGL(augment_gather_kernel, grid, dim3(AUG_MAXBLK), 0, (hipStream_t)stream, data, rows, mat, out,
                       shift ? ws : nullptr, N, H, W, C, (int)per, order, fill_mode, cval);
    if (shift) {
        const int rc = MMSEG_CHECK_LAUNCH();
        if (rc) return rc;
        hipLaunchKernelGGL(augment_shift_kernel, grid, dim3(AUG_MAXBLK), 0, (hipStream_t)stream, out, shift, ws, C, (int)per);
    }
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
