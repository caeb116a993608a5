// Bias-field (coil shading) correction of one MR volume on the device (gfx950; build-defined, an N3 / N4-family rule: Sled's log-domain
// histogram sharpening in the form of N4's SharpenImage, the residual smoothed by a masked, normalised Gaussian convolution in mm in
// place of N4's B-spline fit).  The rule is stated in include/mmseg_hip.h and restated in numpy by tests/volume_bias_ref.py.
// x [S,H,W] fp32, n = S*H*W < 2^31; all arithmetic fp64, one rounding to fp32 at the end; no fp contraction outside the tap loops, so
// that the Otsu threshold, the bin of a voxel and the interpolation follow the restatement operation by operation.
// Everything the iteration decides lives in a BiasState at the head of the workspace: nothing comes back to the host, and a volume the
// rule leaves alone (constant, empty mask, one masked value) sets `frozen`, which every later kernel reads and returns on.
//   begin    reset, x's extremes (ordered integer keys, atomicMin / atomicMax), 256-bin Otsu histogram (LDS + integer atomics), the
//            threshold (one thread, fp64 on the counts), mask + log + f = 0
//   level    den = G * m once, then per iteration: extremes of v = v0 - f on the mask, 200-bin histogram, the one-block sharpen (five
//            512-point radix-2 Stockham transforms in LDS over a root table made by the host), residual, three separable passes, update
//   finish   x = fp32(fp64(x) * exp(-f)) in place; not launched into a volume whose field was never updated
// The separable passes are the hot path: a row piece plus halo in LDS along W; along H and along S one kernel on tiles of BF_TC adjacent
// columns x BF_TL lines plus halo, so that global accesses stay contiguous.  Taps outside the volume are zeros in LDS.  Sums run in the
// fixed order w_0 x_0 + sum_k w_k (x_-k + x_+k), k ascending; integer atomics only: two runs are bitwise equal.
#include "common.hpp"
#pragma clang fp contract(off)

#define BF_BINS 200
#define BF_PAD 512           // padded length of the sharpen's transforms
#define BF_OFF 156           // (BF_PAD - BF_BINS) / 2
#define BF_OTSU 256
#define BF_MAXR 128          // BIAS_MAX_RADIUS of ops.py
#define BF_NT 256            // threads of the element-wise and reduction kernels
#define BF_MAXBLK 1024       // blocks of the strided kernels
#define BF_TW 128            // pixels of one row per block, pass along W
#define BF_TC 16             // adjacent columns per block, passes along H and S
#define BF_TL 32             // lines per block, passes along H and S (two per thread)
#define BF_FWHM 0.15
#define BF_NOISE 0.01
#define BF_LN2X4 2.772588722239781          // 4 ln 2
#define BF_GNORM 0.9394372786996513         // 2 sqrt(ln 2 / pi)

struct BiasState {
    unsigned long long vkey[2];      // ordered keys of min / max of v over the mask, of the iteration under way
    unsigned int xkey[2];            // ordered keys of min / max of x
    int frozen;                      // sticky: the rule changes nothing any more
    int updates;                     // iterations that reached the field update
    double lo, hi, thr;              // x's extremes, the Otsu threshold (after max(., 0))
    double vmin, vmax;               // of the iteration under way, for the residual
    int otsu[BF_OTSU];
    int hist[BF_BINS];
    double E[BF_BINS];
};
#define BF_STATE_DOUBLES 512         // >= sizeof(BiasState) / 8, the arrays start 4096 bytes into the workspace

// order-preserving integer keys of finite floating-point values
__device__ __forceinline__ unsigned int bf_key32(float v) {
    const unsigned int b = __float_as_uint(v);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float bf_unkey32(unsigned int k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
__device__ __forceinline__ unsigned long long bf_key64(double v) {
    const unsigned long long b = (unsigned long long)__double_as_longlong(v);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double bf_unkey64(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

// block-wide minimum and maximum, valid in thread 0
__device__ __forceinline__ void bf_block_minmax(double& lo, double& hi) {
    __shared__ double red[2][BF_NT / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fmin(lo, __shfl_xor(lo, o, 64));
        hi = fmax(hi, __shfl_xor(hi, o, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[0][wid] = lo; red[1][wid] = hi; }
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < BF_NT / 64; ++w) { lo = fmin(lo, red[0][w]); hi = fmax(hi, red[1][w]); }
}

// <<<1, BF_NT>>>
__global__ void __launch_bounds__(BF_NT) bias_reset_kernel(BiasState* st) {
    const int t = threadIdx.x;
    if (t < BF_OTSU) st->otsu[t] = 0;
    if (t < BF_BINS) { st->hist[t] = 0; st->E[t] = 0.0; }
    if (t == 0) {
        st->vkey[0] = ~0ull; st->vkey[1] = 0ull;
        st->xkey[0] = ~0u; st->xkey[1] = 0u;
        st->frozen = 0; st->updates = 0;
        st->lo = st->hi = st->thr = st->vmin = st->vmax = 0.0;
    }
}

__global__ void __launch_bounds__(BF_NT) bias_xrange_kernel(const float* __restrict__ x, size_t n, BiasState* st) {
    double lo = INFINITY, hi = -INFINITY;
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) {
        const double v = (double)x[e];
        lo = fmin(lo, v);
        hi = fmax(hi, v);
    }
    bf_block_minmax(lo, hi);
    if (threadIdx.x == 0 && lo <= hi) {
        atomicMin(&st->xkey[0], bf_key32((float)lo));
        atomicMax(&st->xkey[1], bf_key32((float)hi));
    }
}

__global__ void __launch_bounds__(BF_NT) bias_otsu_hist_kernel(const float* __restrict__ x, size_t n, BiasState* st) {
    __shared__ int h[BF_OTSU];
    const double lo = (double)bf_unkey32(st->xkey[0]), hi = (double)bf_unkey32(st->xkey[1]);
    if (!(hi > lo)) return;                                      // uniform over the grid
    h[threadIdx.x] = 0;
    __syncthreads();
    const double scale = 256.0 / (hi - lo);
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) {
        int b = (int)floor(((double)x[e] - lo) * scale);
        b = b < 0 ? 0 : (b > BF_OTSU - 1 ? BF_OTSU - 1 : b);
        atomicAdd(&h[b], 1);
    }
    __syncthreads();
    if (h[threadIdx.x]) atomicAdd(&st->otsu[threadIdx.x], h[threadIdx.x]);
}

// <<<1, 64>>>: 255 cuts walked by one thread in fp64 on integer sums; the first maximum wins
__global__ void bias_otsu_kernel(BiasState* st) {
    if (threadIdx.x != 0) return;
    const double lo = (double)bf_unkey32(st->xkey[0]), hi = (double)bf_unkey32(st->xkey[1]);
    st->lo = lo;
    st->hi = hi;
    if (!(hi > lo)) { st->frozen = 1; st->thr = lo; return; }
    long long total = 0, first = 0;
    for (int j = 0; j < BF_OTSU; ++j) { total += st->otsu[j]; first += (long long)j * st->otsu[j]; }
    long long w0 = 0, s0 = 0;
    double best = -1.0;
    int cut = 0;
    for (int t = 0; t < BF_OTSU - 1; ++t) {
        w0 += st->otsu[t];
        s0 += (long long)t * st->otsu[t];
        const long long w1 = total - w0;
        double var = 0.0;
        if (w0 > 0 && w1 > 0) {
            const double d = (double)s0 / (double)w0 - (double)(first - s0) / (double)w1;
            var = ((double)w0 * (double)w1) * (d * d);
        }
        if (var > best) { best = var; cut = t; }
    }
    const double thr = lo + ((double)(cut + 1) * (hi - lo)) / 256.0;
    st->thr = fmax(thr, 0.0);
}

__global__ void __launch_bounds__(BF_NT) bias_mask_kernel(const float* __restrict__ x, size_t n, const BiasState* st,
                                                          unsigned char* __restrict__ mask, double* __restrict__ v0,
                                                          double* __restrict__ f) {
    if (st->frozen) return;
    const double thr = st->thr;
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) {
        const double v = (double)x[e];
        const bool m = v > thr;                                  // thr >= 0: the logarithm is of a positive value
        mask[e] = m ? 1 : 0;
        v0[e] = m ? log(v) : 0.0;
        f[e] = 0.0;
    }
}

// extremes of v = v0 - f over the mask (f may be null: v = v0) into the ordered keys
__global__ void __launch_bounds__(BF_NT) bias_vrange_kernel(const double* __restrict__ v0, const double* __restrict__ f,
                                                            const unsigned char* __restrict__ mask, size_t n, BiasState* st) {
    if (st->frozen) return;
    double lo = INFINITY, hi = -INFINITY;
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT)
        if (mask[e]) {
            const double v = f ? v0[e] - f[e] : v0[e];
            lo = fmin(lo, v);
            hi = fmax(hi, v);
        }
    bf_block_minmax(lo, hi);
    if (threadIdx.x == 0 && lo <= hi) {
        atomicMin(&st->vkey[0], bf_key64(lo));
        atomicMax(&st->vkey[1], bf_key64(hi));
    }
}

// nearest bin of c = (v - vmin) / slope; the untouched keys of an empty mask decode to NaN and count nothing
__global__ void __launch_bounds__(BF_NT) bias_hist_kernel(const double* __restrict__ v0, const double* __restrict__ f,
                                                          const unsigned char* __restrict__ mask, size_t n, BiasState* st) {
    __shared__ int h[BF_BINS];
    if (st->frozen) return;
    const double vmin = bf_unkey64(st->vkey[0]), vmax = bf_unkey64(st->vkey[1]);
    if (!(vmax > vmin)) return;
    if (threadIdx.x < BF_BINS) h[threadIdx.x] = 0;
    __syncthreads();
    const double slope = (vmax - vmin) / (double)(BF_BINS - 1);
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT)
        if (mask[e]) {
            const double v = f ? v0[e] - f[e] : v0[e];
            int b = (int)floor((v - vmin) / slope + 0.5);
            b = b < 0 ? 0 : (b > BF_BINS - 1 ? BF_BINS - 1 : b);
            atomicAdd(&h[b], 1);
        }
    __syncthreads();
    if (threadIdx.x < BF_BINS && h[threadIdx.x]) atomicAdd(&st->hist[threadIdx.x], h[threadIdx.x]);
}

// One 512-point transform by BF_NT = 256 threads: nine radix-2 Stockham passes between two LDS images, the result in dst.
// roots [512][2] = (cos, sin)(2 pi q / 512); the forward transform multiplies by the conjugate.  Unscaled.
__device__ __forceinline__ void bf_fft512(double2* src, double2* dst, const double* __restrict__ roots, bool inverse) {
    const int t = threadIdx.x;
    for (int p = 1; p < BF_PAD; p <<= 1) {
        __syncthreads();
        const int k = t & (p - 1), j = ((t - k) << 1) + k, q = k * (BF_PAD / 2 / p);
        const double c = roots[2 * q], s = inverse ? roots[2 * q + 1] : -roots[2 * q + 1];
        const double2 a = src[t], b = src[t + BF_PAD / 2];
        const double2 w = make_double2(b.x * c - b.y * s, b.x * s + b.y * c);
        dst[j] = make_double2(a.x + w.x, a.y + w.y);
        dst[j + p] = make_double2(a.x - w.x, a.y - w.y);
        double2* tmp = src; src = dst; dst = tmp;
    }
    __syncthreads();
}

// <<<1, BF_NT>>>: the sharpen of one iteration.  Takes the counts and the extremes, leaves E, vmin, vmax for the residual and resets the
// counts and the keys for the next iteration.  LDS: 3 * 512 * 16 = 24 KiB.
__global__ void __launch_bounds__(BF_NT) bias_sharpen_kernel(BiasState* st, const double* __restrict__ roots) {
    __shared__ double2 X[BF_PAD], Y[BF_PAD], Fh[BF_PAD];
    if (st->frozen) return;
    const int t = threadIdx.x;
    const double vmin = bf_unkey64(st->vkey[0]), vmax = bf_unkey64(st->vkey[1]);
    __syncthreads();                                             // every thread has read the keys
    if (!(vmax > vmin)) {                                        // uniform: an empty mask or one masked value
        if (t == 0) st->frozen = 1;
        return;
    }
    const double slope = (vmax - vmin) / (double)(BF_BINS - 1), w = BF_FWHM / slope;
    for (int n = t; n < BF_PAD; n += BF_NT) {
        const int m = n < BF_PAD - n ? n : BF_PAD - n;
        X[n] = make_double2((BF_GNORM / w) * exp(-((double)(m * m) * BF_LN2X4) / (w * w)), 0.0);
    }
    bf_fft512(X, Y, roots, false);
    for (int n = t; n < BF_PAD; n += BF_NT) {
        Fh[n] = Y[n];
        const int j = n - BF_OFF;
        X[n] = make_double2(j >= 0 && j < BF_BINS ? (double)st->hist[j] : 0.0, 0.0);
    }
    __syncthreads();
    if (t < BF_BINS) st->hist[t] = 0;
    if (t == 0) {
        st->vkey[0] = ~0ull; st->vkey[1] = 0ull;
        st->vmin = vmin; st->vmax = vmax;
        st->updates += 1;
    }
    bf_fft512(X, Y, roots, false);
    for (int n = t; n < BF_PAD; n += BF_NT) {
        const double2 fh = Fh[n];
        const double g = fh.x / ((fh.x * fh.x + fh.y * fh.y) + BF_NOISE);        // Re(conj(F^) / (|F^|^2 + noise))
        Y[n] = make_double2(Y[n].x * g, Y[n].y * g);
    }
    bf_fft512(Y, X, roots, true);
    for (int n = t; n < BF_PAD; n += BF_NT) {
        const double u = fmax(X[n].x / (double)BF_PAD, 0.0);
        const double b = vmin + (double)(n - BF_OFF) * slope;
        Y[n] = make_double2(u * b, u);                           // both real signals in one transform
    }
    bf_fft512(Y, X, roots, false);
    for (int n = t; n < BF_PAD; n += BF_NT) {
        const double2 a = X[n], fh = Fh[n];
        X[n] = make_double2(a.x * fh.x - a.y * fh.y, a.x * fh.y + a.y * fh.x);
    }
    bf_fft512(X, Y, roots, true);
    if (t < BF_BINS) {
        const double num = Y[t + BF_OFF].x / (double)BF_PAD, den = Y[t + BF_OFF].y / (double)BF_PAD;
        st->E[t] = den != 0.0 ? num / den : 0.0;
    }
}

__global__ void __launch_bounds__(BF_NT) bias_residual_kernel(const double* __restrict__ v0, const double* __restrict__ f,
                                                              const unsigned char* __restrict__ mask, double* __restrict__ r, size_t n,
                                                              const BiasState* st) {
    __shared__ double E[BF_BINS];
    if (st->frozen) return;
    if (threadIdx.x < BF_BINS) E[threadIdx.x] = st->E[threadIdx.x];
    __syncthreads();
    const double vmin = st->vmin, slope = (st->vmax - vmin) / (double)(BF_BINS - 1);
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) {
        double res = 0.0;
        if (mask[e]) {
            const double v = v0[e] - f[e], c = (v - vmin) / slope;
            int i = (int)floor(c);
            i = i < 0 ? 0 : (i > BF_BINS - 2 ? BF_BINS - 2 : i);
            res = v - (E[i] + (c - (double)i) * (E[i + 1] - E[i]));
        }
        r[e] = res;
    }
}

__global__ void __launch_bounds__(BF_NT) bias_maskd_kernel(const unsigned char* __restrict__ mask, double* __restrict__ r, size_t n,
                                                           const int* frozen) {
    if (frozen && *frozen) return;
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) r[e] = mask[e] ? 1.0 : 0.0;
}

// Pass along W.  grid (S*H, ceil(W / BF_TW)), block BF_TW: columns c0-R .. c0+BF_TW-1+R of one row in LDS, zeros outside the row.
// LDS: (BF_TW + 2 BF_MAXR) * 8 + (BF_MAXR + 1) * 8 = 4104 bytes.
__global__ void __launch_bounds__(BF_TW) bias_smooth_row_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                const double* __restrict__ wts, const int* frozen, int W, int R) {
    __shared__ double t[BF_TW + 2 * BF_MAXR];
    __shared__ double wk[BF_MAXR + 1];
    if (frozen && *frozen) return;
    const int c0 = blockIdx.y * BF_TW;
    const size_t row = (size_t)blockIdx.x * W;
    for (int i = threadIdx.x; i <= R; i += BF_TW) wk[i] = wts[i];
    for (int i = threadIdx.x; i < BF_TW + 2 * R; i += BF_TW) {
        const int c = c0 - R + i;
        t[i] = c >= 0 && c < W ? in[row + c] : 0.0;
    }
    __syncthreads();
    const int c = c0 + threadIdx.x;
    if (c >= W) return;
    const double* p = t + threadIdx.x + R;
    double a = wk[0] * p[0];
    for (int k = 1; k <= R; ++k) a = fma(wk[k], p[-k] + p[k], a);
    out[row + c] = a;
}

// Pass along the line axis of a [batch, L, ncol] array (H: L = H, ncol = W, batch = S; S: L = S, ncol = H*W, batch = 1).
// grid (ceil(ncol / BF_TC), ceil(L / BF_TL), batch), block BF_TC x BF_TL/2: lines l0-R .. l0+BF_TL-1+R of BF_TC adjacent columns in
// LDS, zeros outside the axis, two output lines per thread.  A wave reads 4 lines x 16 columns = 64 consecutive doubles of LDS.
// LDS: (BF_TL + 2 BF_MAXR) * BF_TC * 8 + (BF_MAXR + 1) * 8 = 37896 bytes.
__global__ void __launch_bounds__(BF_TC * BF_TL / 2) bias_smooth_col_kernel(const double* __restrict__ in, double* __restrict__ out,
                                                                            const double* __restrict__ wts, const int* frozen, int L,
                                                                            int ncol, int R) {
    __shared__ double t[(BF_TL + 2 * BF_MAXR) * BF_TC];
    __shared__ double wk[BF_MAXR + 1];
    if (frozen && *frozen) return;
    const int tc = threadIdx.x % BF_TC, tr = threadIdx.x / BF_TC;
    const int l0 = blockIdx.y * BF_TL, c = blockIdx.x * BF_TC + tc;
    const size_t base = (size_t)blockIdx.z * L * ncol;
    for (int i = threadIdx.x; i <= R; i += BF_TC * BF_TL / 2) wk[i] = wts[i];
    for (int i = tr; i < BF_TL + 2 * R; i += BF_TL / 2) {
        const int l = l0 - R + i;
        t[i * BF_TC + tc] = c < ncol && l >= 0 && l < L ? in[base + (size_t)l * ncol + c] : 0.0;
    }
    __syncthreads();
    if (c >= ncol) return;
    const double* lo = t + (tr + R) * BF_TC + tc;                // output line l0 + tr
    const double* hi = lo + (BF_TL / 2) * BF_TC;                 // output line l0 + tr + BF_TL / 2
    double a0 = wk[0] * lo[0], a1 = wk[0] * hi[0];
    for (int k = 1; k <= R; ++k) {
        const double w = wk[k];
        const int d = k * BF_TC;
        a0 = fma(w, lo[-d] + lo[d], a0);
        a1 = fma(w, hi[-d] + hi[d], a1);
    }
    const int l = l0 + tr;
    if (l < L) out[base + (size_t)l * ncol + c] = a0;
    if (l + BF_TL / 2 < L) out[base + (size_t)(l + BF_TL / 2) * ncol + c] = a1;
}

__global__ void __launch_bounds__(BF_NT) bias_update_kernel(double* __restrict__ f, const double* __restrict__ num,
                                                            const double* __restrict__ den, size_t n, const int* frozen) {
    if (frozen && *frozen) return;
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) {
        const double d = den[e];
        if (d > 0.0) f[e] += num[e] / d;
    }
}

__global__ void __launch_bounds__(BF_NT) bias_final_kernel(float* __restrict__ x, const double* __restrict__ f, size_t n,
                                                           const BiasState* st) {
    if (st->updates == 0) return;                                // the volume keeps its bits: nothing is written
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT)
        x[e] = (float)((double)x[e] * exp(-f[e]));
}

// the stage entry points' way in and out of the state
__global__ void __launch_bounds__(BF_NT) bias_import_kernel(BiasState* st, const int* __restrict__ hist, const double* __restrict__ range) {
    if (threadIdx.x < BF_BINS) st->hist[threadIdx.x] = hist[threadIdx.x];
    if (threadIdx.x == 0 && range[0] <= range[1]) { st->vkey[0] = bf_key64(range[0]); st->vkey[1] = bf_key64(range[1]); }
}
__global__ void __launch_bounds__(BF_NT) bias_export_kernel(const BiasState* st, double* otsu, int* hist, double* range, double* E) {
    const int t = threadIdx.x;
    if (otsu && t == 0) { otsu[0] = st->lo; otsu[1] = st->hi; otsu[2] = st->thr; otsu[3] = (double)st->frozen; }
    if (hist && t < BF_BINS) hist[t] = st->hist[t];
    if (range && t == 0) { range[0] = bf_unkey64(st->vkey[0]); range[1] = bf_unkey64(st->vkey[1]); }
    if (E && t < BF_BINS) E[t] = st->E[t];
}
__global__ void __launch_bounds__(BF_NT) bias_field_kernel(const BiasState* st, const double* __restrict__ f, double* __restrict__ out,
                                                           int* info, size_t n) {
    const bool live = st->updates != 0;
    if (info && blockIdx.x == 0 && threadIdx.x == 0) { info[0] = st->frozen; info[1] = st->updates; }
    for (size_t e = (size_t)blockIdx.x * BF_NT + threadIdx.x; e < n; e += (size_t)gridDim.x * BF_NT) out[e] = live ? f[e] : 0.0;
}

static int bf_blocks(size_t n) {
    const size_t b = (n + BF_NT - 1) / BF_NT;
    return (int)(b < BF_MAXBLK ? (b ? b : 1) : BF_MAXBLK);
}

static bool bf_shape_ok(int S, int H, int W) {
    return S >= 1 && H >= 1 && W >= 1 && S <= 65535 && H <= 65535 && W <= 65535 && (long)S * H * W < 0x7fffffffL;
}

struct BiasLayout {
    BiasState* st;
    double *v0, *f, *r, *t1, *t2, *den;
    unsigned char* mask;
};

static BiasLayout bf_layout(double* ws, size_t n) {
    BiasLayout b;
    b.st = (BiasState*)ws;
    b.v0 = ws + BF_STATE_DOUBLES;
    b.f = b.v0 + n;
    b.r = b.f + n;
    b.t1 = b.r + n;
    b.t2 = b.t1 + n;
    b.den = b.t2 + n;
    b.mask = (unsigned char*)(b.den + n);
    return b;
}

static_assert(sizeof(BiasState) <= BF_STATE_DOUBLES * sizeof(double), "BiasState outgrew its slot");

// in -> out through t1, t2: along W, along H, then along S when Rs > 0 (in == out is allowed; t1, t2 are neither)
static int bf_smooth(const double* in, double* out, double* t1, double* t2, const double* wts, const int* frozen, int S, int H, int W,
                     int Rs, int Rr, int Rc, hipStream_t stream) {
    hipLaunchKernelGGL(bias_smooth_row_kernel, dim3(S * H, (W + BF_TW - 1) / BF_TW), dim3(BF_TW), 0, stream, in, t1,
                       wts + 2 * (BF_MAXR + 1), frozen, W, Rc);
    int rc = MMSEG_CHECK_LAUNCH();
    if (rc) return rc;
    hipLaunchKernelGGL(bias_smooth_col_kernel, dim3((W + BF_TC - 1) / BF_TC, (H + BF_TL - 1) / BF_TL, S), dim3(BF_TC * BF_TL / 2), 0, stream,
                       (const double*)t1, Rs > 0 ? t2 : out, wts + (BF_MAXR + 1), frozen, H, W, Rr);
    rc = MMSEG_CHECK_LAUNCH();
    if (rc || Rs <= 0) return rc;
    const int HW = H * W;
    hipLaunchKernelGGL(bias_smooth_col_kernel, dim3((HW + BF_TC - 1) / BF_TC, (S + BF_TL - 1) / BF_TL, 1), dim3(BF_TC * BF_TL / 2), 0, stream,
                       (const double*)t2, out, wts, frozen, S, HW, Rs);
    return MMSEG_CHECK_LAUNCH();
}

static bool bf_radii_ok(int Rs, int Rr, int Rc) {
    return Rs >= 0 && Rs <= BF_MAXR && Rr >= 1 && Rr <= BF_MAXR && Rc >= 1 && Rc <= BF_MAXR;
}

extern "C" {

// doubles of the workspace of one volume: the state, six fp64 volumes (v0, f, r, two between the passes, den) and the mask's bytes
long mmseg_bias_workspace_doubles(int S, int H, int W) {
    if (!bf_shape_ok(S, H, W)) return 0;
    const long n = (long)S * H * W;
    return BF_STATE_DOUBLES + 6 * n + (n + 7) / 8;
}

int mmseg_bias_otsu(const float* x, double* ws, double* out, int S, int H, int W, void* stream) {
    if (!bf_shape_ok(S, H, W) || !x || !ws || !out) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)S * H * W;
    BiasState* st = (BiasState*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_reset_kernel, dim3(1), dim3(BF_NT), 0, s, st);
    hipLaunchKernelGGL(bias_xrange_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, s, x, n, st);
    hipLaunchKernelGGL(bias_otsu_hist_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, s, x, n, st);
    hipLaunchKernelGGL(bias_otsu_kernel, dim3(1), dim3(64), 0, s, st);
    hipLaunchKernelGGL(bias_export_kernel, dim3(1), dim3(BF_NT), 0, s, (const BiasState*)st, out, (int*)nullptr, (double*)nullptr,
                       (double*)nullptr);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_bias_histogram(const double* v, const unsigned char* mask, double* ws, int* hist, double* range, long n, void* stream) {
    if (n < 1 || n >= 0x7fffffffL || !v || !mask || !ws || !hist || !range) return (int)hipErrorInvalidValue;
    BiasState* st = (BiasState*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_reset_kernel, dim3(1), dim3(BF_NT), 0, s, st);
    hipLaunchKernelGGL(bias_vrange_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, s, v, (const double*)nullptr, mask, (size_t)n, st);
    hipLaunchKernelGGL(bias_hist_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, s, v, (const double*)nullptr, mask, (size_t)n, st);
    hipLaunchKernelGGL(bias_export_kernel, dim3(1), dim3(BF_NT), 0, s, (const BiasState*)st, (double*)nullptr, hist, range, (double*)nullptr);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_bias_sharpen(const int* hist, const double* range, const double* roots, double* ws, double* E, void* stream) {
    if (!hist || !range || !roots || !ws || !E) return (int)hipErrorInvalidValue;
    BiasState* st = (BiasState*)ws;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(bias_reset_kernel, dim3(1), dim3(BF_NT), 0, s, st);
    hipLaunchKernelGGL(bias_import_kernel, dim3(1), dim3(BF_NT), 0, s, st, hist, range);
    hipLaunchKernelGGL(bias_sharpen_kernel, dim3(1), dim3(BF_NT), 0, s, st, roots);
    hipLaunchKernelGGL(bias_export_kernel, dim3(1), dim3(BF_NT), 0, s, (const BiasState*)st, (double*)nullptr, (int*)nullptr, (double*)nullptr, E);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_bias_smooth(const double* in, double* out, double* tmp, const double* weights, int S, int H, int W, int Rs, int Rr, int Rc,
                      void* stream) {
    if (!bf_shape_ok(S, H, W) || !bf_radii_ok(Rs, Rr, Rc) || !in || !out || !tmp || !weights) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)S * H * W;
    return bf_smooth(in, out, tmp, tmp + n, weights, nullptr, S, H, W, Rs, Rr, Rc, (hipStream_t)stream);
}

int mmseg_bias_update(double* f, const double* num, const double* den, long n, void* stream) {
    if (n < 1 || n >= 0x7fffffffL || !f || !num || !den) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(bias_update_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, (hipStream_t)stream, f, num, den, (size_t)n, (const int*)nullptr);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_bias_begin(const float* x, double* ws, int S, int H, int W, void* stream) {
    if (!bf_shape_ok(S, H, W) || !x || !ws) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)S * H * W;
    const BiasLayout b = bf_layout(ws, n);
    hipStream_t s = (hipStream_t)stream;
    const int nb = bf_blocks(n);
    hipLaunchKernelGGL(bias_reset_kernel, dim3(1), dim3(BF_NT), 0, s, b.st);
    hipLaunchKernelGGL(bias_xrange_kernel, dim3(nb), dim3(BF_NT), 0, s, x, n, b.st);
    hipLaunchKernelGGL(bias_otsu_hist_kernel, dim3(nb), dim3(BF_NT), 0, s, x, n, b.st);
    hipLaunchKernelGGL(bias_otsu_kernel, dim3(1), dim3(64), 0, s, b.st);
    hipLaunchKernelGGL(bias_mask_kernel, dim3(nb), dim3(BF_NT), 0, s, x, n, (const BiasState*)b.st, b.mask, b.v0, b.f);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_bias_level(double* ws, const double* roots, const double* weights, int S, int H, int W, int Rs, int Rr, int Rc, int iterations,
                     void* stream) {
    if (!bf_shape_ok(S, H, W) || !bf_radii_ok(Rs, Rr, Rc) || iterations < 1 || iterations > 1000 || !ws || !roots || !weights)
        return (int)hipErrorInvalidValue;
    const size_t n = (size_t)S * H * W;
    const BiasLayout b = bf_layout(ws, n);
    hipStream_t s = (hipStream_t)stream;
    const int nb = bf_blocks(n);
    const int* frozen = &b.st->frozen;
    hipLaunchKernelGGL(bias_maskd_kernel, dim3(nb), dim3(BF_NT), 0, s, (const unsigned char*)b.mask, b.r, n, frozen);
    int rc = bf_smooth(b.r, b.den, b.t1, b.t2, weights, frozen, S, H, W, Rs, Rr, Rc, s);
    for (int it = 0; it < iterations && !rc; ++it) {
        hipLaunchKernelGGL(bias_vrange_kernel, dim3(nb), dim3(BF_NT), 0, s, (const double*)b.v0, (const double*)b.f,
                           (const unsigned char*)b.mask, n, b.st);
        hipLaunchKernelGGL(bias_hist_kernel, dim3(nb), dim3(BF_NT), 0, s, (const double*)b.v0, (const double*)b.f,
                           (const unsigned char*)b.mask, n, b.st);
        hipLaunchKernelGGL(bias_sharpen_kernel, dim3(1), dim3(BF_NT), 0, s, b.st, roots);
        hipLaunchKernelGGL(bias_residual_kernel, dim3(nb), dim3(BF_NT), 0, s, (const double*)b.v0, (const double*)b.f,
                           (const unsigned char*)b.mask, b.r, n, (const BiasState*)b.st);
        rc = MMSEG_CHECK_LAUNCH();
        if (rc) break;
        rc = bf_smooth(b.r, b.r, b.t1, b.t2, weights, frozen, S, H, W, Rs, Rr, Rc, s);
        if (rc) break;
        hipLaunchKernelGGL(bias_update_kernel, dim3(nb), dim3(BF_NT), 0, s, b.f, (const double*)b.r, (const double*)b.den, n, frozen);
        rc = MMSEG_CHECK_LAUNCH();
    }
    return rc;
}

int mmseg_bias_finish(float* x, const double* ws, int S, int H, int W, void* stream) {
    if (!bf_shape_ok(S, H, W) || !x || !ws) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)S * H * W;
    const BiasLayout b = bf_layout(const_cast<double*>(ws), n);
    hipLaunchKernelGGL(bias_final_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, (hipStream_t)stream, x, (const double*)b.f, n,
                       (const BiasState*)b.st);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_bias_field(const double* ws, double* field, int* info, int S, int H, int W, void* stream) {
    if (!bf_shape_ok(S, H, W) || !ws || !field) return (int)hipErrorInvalidValue;
    const size_t n = (size_t)S * H * W;
    const BiasLayout b = bf_layout(const_cast<double*>(ws), n);
    hipLaunchKernelGGL(bias_field_kernel, dim3(bf_blocks(n)), dim3(BF_NT), 0, (hipStream_t)stream, (const BiasState*)b.st,
                       (const double*)b.f, field, info, n);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
