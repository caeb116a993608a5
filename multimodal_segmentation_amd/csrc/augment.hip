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
#include "philox.hpp"

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
// FIELD: disp [B,H,W,2] fp32 (row, column) is added to the output pixel before the matrix (mmseg_elastic_gather); without it disp is
// not read and the kernel is the plain affine gather
template <bool FIELD>
__global__ void __launch_bounds__(AUG_MAXBLK) augment_gather_kernel(
        const float* __restrict__ data, const int* __restrict__ rows, const double* __restrict__ mat, float* __restrict__ out,
        float* __restrict__ part, int N, int H, int W, int C, int per, int order, int mode, float cval, const float* __restrict__ disp) {
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
        double sr, sc;
        if constexpr (FIELD) {
            const float* d = disp + ((size_t)b * H * W + p) * 2;
            const double pr = r + (double)d[0], pc = c + (double)d[1];
            sr = aug_map(m0 * pr + m1 * pc + m2, H, mode, inside);
            sc = aug_map(m3 * pr + m4 * pc + m5, W, mode, inside);
        } else {
            sr = aug_map(m0 * r + m1 * c + m2, H, mode, inside);
            sc = aug_map(m3 * r + m4 * c + m5, W, mode, inside);
        }
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

// the launches shared by mmseg_augment_gather (disp == nullptr) and mmseg_elastic_gather
static int augment_launch(const float* data, const int* rows, const double* mat, const float* disp, const float* shift, float* out,
                          float* ws, int N, int B, int H, int W, int C, int order, int fill_mode, float cval, void* stream) {
    if (B <= 0) return 0;
    if (N < 1 || H < 1 || W < 1 || C < 1 || B > 65535 || order < 0 || order > 1 || fill_mode < AUG_NEAREST || fill_mode > AUG_WRAP ||
        (shift && !ws))
        return (int)hipErrorInvalidValue;
    const long per = (long)H * W * C;
    if (per > 0x7fffffffL - (long)AUG_MAXBLK * AUG_MAXBLK) return (int)hipErrorInvalidValue;      // 32-bit element indices
    const dim3 grid((unsigned)aug_blocks(per), B);
    if (disp)
        hipLaunchKernelGGL(augment_gather_kernel<true>, grid, dim3(AUG_MAXBLK), 0, (hipStream_t)stream, data, rows, mat, out,
                           shift ? ws : nullptr, N, H, W, C, (int)per, order, fill_mode, cval, disp);
    else
        hipLaunchKernelGGL(augment_gather_kernel<false>, grid, dim3(AUG_MAXBLK), 0, (hipStream_t)stream, data, rows, mat, out,
                           shift ? ws : nullptr, N, H, W, C, (int)per, order, fill_mode, cval, (const float*)nullptr);
    if (shift) {
        const int rc = MMSEG_CHECK_LAUNCH();
        if (rc) return rc;
        hipLaunchKernelGGL(augment_shift_kernel, grid, dim3(AUG_MAXBLK), 0, (hipStream_t)stream, out, shift, ws, C, (int)per);
    }
    return MMSEG_CHECK_LAUNCH();
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
    return augment_launch(data, rows, mat, nullptr, shift, out, ws, N, B, H, W, C, order, fill_mode, cval, stream);
}

// mmseg_augment_gather with a displacement field disp [B,H,W,2] fp32 (row, column) added to the output pixel before the matrix:
//     sr = m0*(r + disp_r) + m1*(c + disp_c) + m2,   sc = m3*(r + disp_r) + m4*(c + disp_c) + m5      (fp64)
// i.e. z(p) = x(M (p + d(p))), an elastic warp of the affinely transformed sample with ONE interpolation; everything after the
// coordinates is the code of mmseg_augment_gather.  A zero field gives its bits.
int mmseg_elastic_gather(const float* data, const int* rows, const double* mat, const float* disp, const float* shift, float* out,
                         float* ws, int N, int B, int H, int W, int C, int order, int fill_mode, float cval, void* stream) {
    if (B > 0 && !disp) return (int)hipErrorInvalidValue;
    return augment_launch(data, rows, mat, disp, shift, out, ws, N, B, H, W, C, order, fill_mode, cval, stream);
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------------------------------------
// Elastic deformation (Simard 2003; albumentations' ElasticTransform): a random smooth displacement field, a function of
// (seed, batch number, sample, pixel) only.
//   noise   P = Philox4x32-10(counter (r*W + c, b, 0, 0), key (seed, batch));  u_a = (P[a] >> 8) * 2^-23 - 1 in [-1, 1 - 2^-23],
//           exact in fp32, a = 0 (row) / 1 (column)
//   blur    g_a = scipy.ndimage.gaussian_filter(u_a[b], sigma, mode='reflect', truncate=4): separable, radius R, the host's R+1
//           fp64 weights w_0 .. w_R (w_-k = w_k), half-sample symmetric reflection of period 2n (right for R > n too)
//   field   disp[b,r,c,a] = fp32(scale[b] * g_a), scale [B] fp64; scale[b] == 0 -> +0.0 and no blur for that sample
// Two launches, both accumulating in fp64 in a fixed order (bitwise reproducible):
//   elastic_blur_cols_kernel  grid (ceil(W / EL_TW), H, B), block EL_TW: the noise of columns c0-R .. c0+EL_TW-1+R of one row is drawn
//                             once into LDS (Philox per staged pixel, not per tap), blurred along the row -> ws [B,H,W,2] fp64
//   elastic_blur_rows_kernel  grid (ceil(W / EL_TC), ceil(H / EL_TH), B), block EL_TC x EL_TH/2: rows r0-R .. r0+EL_TH-1+R of EL_TC
//                             columns of ws in LDS ((EL_TH + 2R) * EL_TC * 16 bytes: 40 KiB at R = 128), two output rows per thread
#define EL_MAXR 128
#define EL_TW 128
#define EL_TH 64
#define EL_TC 8

// philox4x32_10 and el_reflect (half-sample symmetric reflection, period 2n): philox.hpp

__global__ void __launch_bounds__(EL_TW) elastic_blur_cols_kernel(const double* __restrict__ scale, const double* __restrict__ wts,
                                                                  double* __restrict__ ws, uint32_t seed, uint32_t batch, int H, int W,
                                                                  int R) {
    __shared__ float nz[2][EL_TW + 2 * EL_MAXR];                    // fp32 holds the noise exactly; fp64 here was slower (LDS-bound)
    __shared__ double wk[EL_MAXR + 1];
    const int b = blockIdx.z, r = blockIdx.y, c0 = blockIdx.x * EL_TW;
    if (scale[b] == 0.0) return;                                   // uniform over the block
    for (int i = threadIdx.x; i <= R; i += EL_TW) wk[i] = wts[i];
    for (int i = threadIdx.x; i < EL_TW + 2 * R; i += EL_TW) {
        const int cc = el_reflect(c0 - R + i, W);
        uint32_t p0, p1;
        philox4x32_10((uint32_t)r * (uint32_t)W + (uint32_t)cc, (uint32_t)b, 0u, 0u, seed, batch, p0, p1);
        nz[0][i] = (float)(p0 >> 8) * 0x1p-23f - 1.f;
        nz[1][i] = (float)(p1 >> 8) * 0x1p-23f - 1.f;
    }
    __syncthreads();
    const int c = c0 + threadIdx.x;
    if (c >= W) return;
    const int t = threadIdx.x + R;
    double a0 = wk[0] * (double)nz[0][t], a1 = wk[0] * (double)nz[1][t];
    for (int k = 1; k <= R; ++k) {
        const double w = wk[k];
        a0 += w * ((double)nz[0][t - k] + (double)nz[0][t + k]);
        a1 += w * ((double)nz[1][t - k] + (double)nz[1][t + k]);
    }
    double* o = ws + (((size_t)b * H + r) * W + c) * 2;
    o[0] = a0;
    o[1] = a1;
}

__global__ void __launch_bounds__(EL_TC * EL_TH / 2) elastic_blur_rows_kernel(const double* __restrict__ scale,
                                                                              const double* __restrict__ wts,
                                                                              const double* __restrict__ ws, float* __restrict__ disp,
                                                                              int H, int W, int R) {
    extern __shared__ double2 el_lds[];                            // [(EL_TH + 2R)][EL_TC] (row, column) pairs, 16-byte reads; then R + 1 weights
    const int b = blockIdx.z, r0 = blockIdx.y * EL_TH, c0 = blockIdx.x * EL_TC;
    const int tc = threadIdx.x % EL_TC, tr = threadIdx.x / EL_TC;
    const int nrow = EL_TH + 2 * R;
    double* wk = reinterpret_cast<double*>(el_lds + (size_t)nrow * EL_TC);
    const double s = scale[b];
    const int c = c0 + tc;
    if (s == 0.0) {                                                // uniform over the block
        if (c < W)
            for (int q = 0; q < 2; ++q) {
                const int r = r0 + tr + q * (EL_TH / 2);
                if (r < H) {
                    float* o = disp + (((size_t)b * H + r) * W + c) * 2;
                    o[0] = 0.f;
                    o[1] = 0.f;
                }
            }
        return;
    }
    for (int i = threadIdx.x; i <= R; i += blockDim.x) wk[i] = wts[i];
    for (int i = tr; i < nrow; i += EL_TH / 2) {
        double2 v = make_double2(0.0, 0.0);
        if (c < W) v = reinterpret_cast<const double2*>(ws)[((size_t)b * H + el_reflect(r0 - R + i, H)) * W + c];
        el_lds[i * EL_TC + tc] = v;
    }
    __syncthreads();
    if (c >= W) return;
    const double2* lo = el_lds + (size_t)(tr + R) * EL_TC + tc;              // output row r0 + tr
    const double2* hi = lo + (size_t)(EL_TH / 2) * EL_TC;                    // output row r0 + tr + EL_TH / 2
    double a0 = wk[0] * lo->x, a1 = wk[0] * lo->y, b0 = wk[0] * hi->x, b1 = wk[0] * hi->y;
    for (int k = 1; k <= R; ++k) {
        const double w = wk[k];
        const int d = k * EL_TC;
        const double2 lm = lo[-d], lp = lo[d], hm = hi[-d], hp = hi[d];
        a0 += w * (lm.x + lp.x);
        a1 += w * (lm.y + lp.y);
        b0 += w * (hm.x + hp.x);
        b1 += w * (hm.y + hp.y);
    }
    const int r = r0 + tr;
    if (r < H) {
        float* o = disp + (((size_t)b * H + r) * W + c) * 2;
        o[0] = (float)(s * a0);
        o[1] = (float)(s * a1);
    }
    if (r + EL_TH / 2 < H) {
        float* o = disp + (((size_t)b * H + r + EL_TH / 2) * W + c) * 2;
        o[0] = (float)(s * b0);
        o[1] = (float)(s * b1);
    }
}

static bool elastic_shape_ok(int B, int H, int W) {
    return B >= 1 && H >= 1 && W >= 1 && B <= 65535 && H <= 65535 && (long)H * W <= 0x3fffffffL;
}

extern "C" {

// doubles of the scratch buffer between the two passes; 0 for a shape mmseg_elastic_field refuses.  Launches nothing.
long mmseg_elastic_workspace_doubles(int B, int H, int W) {
    return elastic_shape_ok(B, H, W) ? 2L * B * H * W : 0;
}

// scale [B] fp64, weights [R+1] fp64 (w_0 .. w_R of the normalised kernel), disp [B,H,W,2] fp32, ws:
// mmseg_elastic_workspace_doubles(B, H, W) doubles, 16-byte aligned; seed and batch are read as 32-bit patterns
int mmseg_elastic_field(const double* scale, const double* weights, float* disp, double* ws, int seed, int batch, int B, int H, int W,
                        int R, void* stream) {
    if (R < 1 || R > EL_MAXR) return (int)hipErrorInvalidValue;
    if (B <= 0) return 0;
    if (!elastic_shape_ok(B, H, W) || !scale || !weights || !disp || !ws || ((uintptr_t)ws & 15)) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(elastic_blur_cols_kernel, dim3((W + EL_TW - 1) / EL_TW, H, B), dim3(EL_TW), 0, (hipStream_t)stream, scale,
                       weights, ws, (uint32_t)seed, (uint32_t)batch, H, W, R);
    const int rc = MMSEG_CHECK_LAUNCH();
    if (rc) return rc;
    const size_t lds = ((size_t)(EL_TH + 2 * R) * EL_TC * 2 + R + 1) * sizeof(double);
    hipLaunchKernelGGL(elastic_blur_rows_kernel, dim3((W + EL_TC - 1) / EL_TC, (H + EL_TH - 1) / EL_TH, B), dim3(EL_TC * EL_TH / 2), lds,
                       (hipStream_t)stream, scale, weights, ws, disp, H, W, R);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
