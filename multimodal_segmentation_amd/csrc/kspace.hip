// MR k-space artefact augmentation of a gathered training batch on the device (gfx950; build-defined, after TorchIO's RandomMotion /
// RandomGhosting / RandomSpike and MONAI's GibbsNoise / KSpaceSpikeNoise / RicianNoise).  x [B,H,W,C] fp32 is an image array of one
// batch as the gather kernels of augment.hip wrote it.  Per sample b and channel, with lo the sample's minimum (column 0 of the table
// of mmseg_intensity_stats), y = x - lo >= 0 and X = fft2(y) in complex fp64, numpy's convention (unshifted, the inverse scaled by
// 1 / (H W)); signed frequencies ky = u < ceil(H/2) ? u : u - H, kx likewise; p the phase-encode axis (0 rows, 1 columns), k_p the
// signed frequency along it and P its extent.  In this order, each only where its flag is set (the table: KS_* below):
//   motion  X *= exp(-2 pi i (ky dy / H + kx dx / W)), (dy, dx) the shift of segment seg(k_p + floor(P/2)), seg(l) = number of breaks <= l
//   ghost   X *= 1 - a where k_p != 0 and k_p mod n == 0 (the sign of the divisor)
//   gibbs   X = 0 where 4 (ky^2 W^2 + kx^2 H^2) > T;  the left side is an exact integer in fp64
//   spikes  X[ky_s mod H][kx_s mod W] += A (c_s + i s_s), then X[-ky_s mod H][-kx_s mod W] += A (c_s - i s_s), A = (sum - H W C lo) / C, the
//           mean over the channels of sum(y) (for C = 1 the DC term), spike after spike; every element looks its spikes up, nothing is scattered
//   rician  z = ifft2(X);  z += std sqrt(-2 ln u1) (cos 2 pi u2 + i sin 2 pi u2), u1 = ((P[0] >> 8) + 1) 2^-24, u2 = (P[1] >> 8) 2^-24,
//           P = Philox4x32-10(counter (e, b, array, 5), key (seed, batch)), e = (r W + c) C + ch
//   output  x = fp32(lo + |z|), no clip
//
// The transform.  Lengths 2 <= N <= 1024 with prime factors in {2, 3, 5}.  A line is transformed in LDS by Stockham autosort passes
// of radix 4 (while 4 divides what is left), then 2, 3 and 5, between two images of the line: pass (R, Ns) has N / R butterflies, butterfly
// j reads src[j + q N/R], q < R, multiplies by the root exp(-+2 pi i q k / (Ns R)), k = j mod Ns, which is entry q k N / (Ns R) of the host's
// table cos / sin(2 pi k / N) (conjugated for the forward transform), takes the R-point DFT (radix 2 and 4 by additions, radix 3 and 5
// as the plain sum over the table's roots) and writes dst[(j - k) R + k + q Ns].  Every value is computed by one thread in a fixed
// order and there are no atomics: two runs are bitwise equal.
//   along W   one block of KS_WT threads per (b, ch, row); the two images are 2 * 16 W bytes, 32 KiB at W = 1024.
//   along H   one block of KS_HT threads per tile of TC adjacent columns, TC = 16 / 8 / 4 / 2 for H <= 128 / 256 / 512 / 1024 (the
//             largest power of two that keeps the two images, 2 * 16 H TC bytes, within 64 KiB).  Thread t holds column t % TC and
//             butterflies t / TC, t / TC + KS_HT / TC, ...; global reads and writes are contiguous over 16 TC bytes (32-byte pieces at
//             H = 1024).
// LDS layout: image[element][TC] complex fp64, NOT padded.  The compiler reads and stores the values as ds_read_b128 / ds_write_b128; by
// the bank rule of the cdna_hip_programming guide, section 2 (a 16-byte read is served in groups of 16 lanes over 64 banks = 16 slots of
// 16 bytes, a 16-byte store in groups of 8 consecutive lanes over 32 banks = 8 slots), enumerated by tools/kspace_lds_check.py:
//   reads    butterfly j reads element j + q N/R, so thread t reads slot t + const: lane-linear, conflict-free in every pass and tile.
//   stores   along H with TC >= 8 (H <= 256: the default 192 and the benchmark's 256) the 8 lanes of a group hold 8 adjacent columns of
//            ONE row, 128 contiguous bytes: conflict-free in every pass, however far apart the rows of neighbouring butterflies lie.
//            With TC = 4 (2) a group holds 2 (4) butterflies; once Ns >= 2 (4) their rows are adjacent and the group is contiguous again,
//            before that their rows lie R Ns apart: the first pass of H > 256 lands 2-way (4-way at H > 512) on a slot.  Along W a
//            group holds 8 butterflies: 4-way in a first radix-4 pass, 2-way while Ns < 8, conflict-free from then on.
//            Padding one slot per 4, 8, 16 or 32 elements or rotating the slots of a 128-byte line trades these for 2- and 3-way READ
//            conflicts in every pass (enumerated; DESIGN section 9 names the one candidate that halves them).  Nothing here was measured
//            with counters.
// Five launches per image array: forward along W (reads x, writes the spectrum), forward along H, the rule, inverse along H, inverse
// along W (writes x): 4 + 8 * 16 + 4 = 136 bytes per pixel and channel.
#include "common.hpp"
#include "philox.hpp"

#define KS_WT 64             // threads per block, passes along W
#define KS_HT 256            // threads per block, passes along H
#define KS_MAXN 1024         // longest line
#define KS_MAXBLK 256        // threads per block and most blocks per (sample, channel) of the rule's kernel
// the table: KS_P doubles per sample
#define KS_P 48
#define KS_FLAGS 0           // 1 motion + 2 ghost + 4 gibbs + 8 spikes + 16 rician
#define KS_AXIS 1            // phase-encode axis: 0 rows, 1 columns
#define KS_BREAKS 2          // number of breaks, S - 1 <= 7
#define KS_BREAK0 3          // 7 sorted breaks
#define KS_SHIFT0 10         // 8 segments x (dy, dx) in pixels; the segment that holds k_p = 0 carries (0, 0)
#define KS_GHOST_N 26
#define KS_GHOST_F 27        // 1 - a
#define KS_GIBBS_T 28        // f f H H W W
#define KS_SPIKES 29         // K <= 4
#define KS_SPIKE0 30         // 4 spikes x (ky mod H, kx mod W, s cos phi, s sin phi)
#define KS_STD 46
#define KS_MOTION 1
#define KS_GHOST 2
#define KS_GIBBS 4
#define KS_SPIKE 8
#define KS_RICIAN 16

__device__ __forceinline__ double2 ks_mul(double2 a, double2 b) { return make_double2(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
__device__ __forceinline__ double2 ks_add(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 ks_sub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }

// entry k of the table as exp(-2 pi i k / N) (forward) or exp(+2 pi i k / N) (inverse)
template <bool INV>
__device__ __forceinline__ double2 ks_root(const double2* __restrict__ tw, int k) {
    double2 w = tw[k];
    if (!INV) w.y = -w.y;
    return w;
}

// butterfly j of the Stockham pass (R, Ns) of a line of length N; element i of the line of this thread sits at [i * ld + col]
template <int R, bool INV>
__device__ __forceinline__ void ks_butterfly(const double2* src, double2* dst, const double2* __restrict__ tw, int N, int Ns, int j,
                                             int ld, int col) {
    const int M = N / R, k = j % Ns, tstep = N / (Ns * R);
    double2 v[R], y[R];
#pragma unroll
    for (int q = 0; q < R; ++q) v[q] = src[(j + q * M) * ld + col];
#pragma unroll
    for (int q = 1; q < R; ++q) v[q] = ks_mul(v[q], ks_root<INV>(tw, q * k * tstep));
    if constexpr (R == 2) {
        y[0] = ks_add(v[0], v[1]);
        y[1] = ks_sub(v[0], v[1]);
    } else if constexpr (R == 4) {
        const double2 t0 = ks_add(v[0], v[2]), t1 = ks_sub(v[0], v[2]), t2 = ks_add(v[1], v[3]), t3 = ks_sub(v[1], v[3]);
        const double2 it3 = INV ? make_double2(-t3.y, t3.x) : make_double2(t3.y, -t3.x);          // (+-i) t3, the sign of the exponent
        y[0] = ks_add(t0, t2);
        y[1] = ks_add(t1, it3);
        y[2] = ks_sub(t0, t2);
        y[3] = ks_sub(t1, it3);
    } else {
#pragma unroll
        for (int p = 0; p < R; ++p) {
            double2 a = v[0];
#pragma unroll
            for (int q = 1; q < R; ++q) a = ks_add(a, ks_mul(v[q], ks_root<INV>(tw, ((p * q) % R) * M)));
            y[p] = a;
        }
    }
    const int o = (j - k) * R + k;
#pragma unroll
    for (int q = 0; q < R; ++q) dst[(o + q * Ns) * ld + col] = y[q];
}

// All passes of the lines held in image a (b is the second image); this thread runs butterflies j0, j0 + jstep, ... of column col.
// Every thread of the block calls it (the barriers); returns the image that holds the result.
template <bool INV>
__device__ __forceinline__ double2* ks_line(double2* a, double2* b, const double2* __restrict__ tw, int N, int ld, int col, int j0,
                                            int jstep) {
    int Ns = 1;
    for (int n = N; n > 1;) {
        const int R = n % 4 == 0 ? 4 : (n % 2 == 0 ? 2 : (n % 3 == 0 ? 3 : 5));
        const int M = N / R;
        if (R == 4)
            for (int j = j0; j < M; j += jstep) ks_butterfly<4, INV>(a, b, tw, N, Ns, j, ld, col);
        else if (R == 2)
            for (int j = j0; j < M; j += jstep) ks_butterfly<2, INV>(a, b, tw, N, Ns, j, ld, col);
        else if (R == 3)
            for (int j = j0; j < M; j += jstep) ks_butterfly<3, INV>(a, b, tw, N, Ns, j, ld, col);
        else
            for (int j = j0; j < M; j += jstep) ks_butterfly<5, INV>(a, b, tw, N, Ns, j, ld, col);
        __syncthreads();
        double2* t = a;
        a = b;
        b = t;
        Ns *= R;
        n /= R;
    }
    return a;
}

extern __shared__ double2 ks_lds[];

// grid (H, B*C), block KS_WT, LDS 2 W complex: row r of channel ch of sample b, y = x - lo -> its transform along W -> spec [B,C,H,W]
__global__ void __launch_bounds__(KS_WT) kspace_fwd_w_kernel(const float* __restrict__ x, const double* __restrict__ table,
                                                              const double* __restrict__ stats, const double2* __restrict__ tw,
                                                              double2* __restrict__ spec, int H, int W, int C) {
    const int bc = blockIdx.y, b = bc / C, ch = bc - b * C, r = blockIdx.x;
    if ((int)table[(size_t)b * KS_P + KS_FLAGS] == 0) return;          // uniform over the block
    const double lo = stats[(size_t)b * 3];
    const float* src = x + ((size_t)b * H + r) * W * C + ch;
    double2* a = ks_lds;
    for (int c = threadIdx.x; c < W; c += KS_WT) a[c] = make_double2((double)src[(size_t)c * C] - lo, 0.0);
    __syncthreads();
    const double2* res = ks_line<false>(a, a + W, tw, W, 1, 0, threadIdx.x, KS_WT);
    double2* dst = spec + ((size_t)bc * H + r) * W;
    for (int c = threadIdx.x; c < W; c += KS_WT) dst[c] = res[c];
}

// grid (ceil(W / TC), B*C), block KS_HT, LDS 2 H TC complex: TC adjacent columns of one channel, transformed along H in place
template <bool INV>
__global__ void __launch_bounds__(KS_HT) kspace_h_kernel(double2* __restrict__ spec, const double* __restrict__ table,
                                                          const double2* __restrict__ tw, int H, int W, int C, int TC) {
    const int bc = blockIdx.y, b = bc / C, c0 = blockIdx.x * TC;
    if ((int)table[(size_t)b * KS_P + KS_FLAGS] == 0) return;
    const int tc = threadIdx.x & (TC - 1), jj = threadIdx.x / TC, nj = KS_HT / TC;
    const bool live = c0 + tc < W;
    double2* g = spec + (size_t)bc * H * W + c0 + tc;
    double2* a = ks_lds;
    for (int r = jj; r < H; r += nj) a[r * TC + tc] = live ? g[(size_t)r * W] : make_double2(0.0, 0.0);
    __syncthreads();
    const double2* res = ks_line<INV>(a, a + H * TC, tw, H, TC, tc, jj, nj);
    if (live)
        for (int r = jj; r < H; r += nj) g[(size_t)r * W] = res[r * TC + tc];
}

// grid (nblk, B*C), block KS_MAXBLK: the rule, element by element, in place
__global__ void __launch_bounds__(KS_MAXBLK) kspace_apply_kernel(double2* __restrict__ spec, const double* __restrict__ table,
                                                                  const double* __restrict__ stats, int H, int W, int C) {
    const int bc = blockIdx.y, b = bc / C;
    const double* p = table + (size_t)b * KS_P;
    const int flags = (int)p[KS_FLAGS];
    if (!(flags & (KS_MOTION | KS_GHOST | KS_GIBBS | KS_SPIKE))) return;
    const bool motion = flags & KS_MOTION, ghost = flags & KS_GHOST, gibbs = flags & KS_GIBBS;
    const int axis = (int)p[KS_AXIS], P = axis ? W : H, nbreak = min(max((int)p[KS_BREAKS], 0), 7);
    const int gn = max((int)p[KS_GHOST_N], 1), K = (flags & KS_SPIKE) ? min(max((int)p[KS_SPIKES], 0), 4) : 0;
    const double gf = p[KS_GHOST_F], T = p[KS_GIBBS_T];
    const double A = (stats[(size_t)b * 3 + 2] - (double)H * (double)W * (double)C * stats[(size_t)b * 3]) / (double)C;
    double2* dst = spec + (size_t)bc * H * W;
    const int HW = H * W;
    for (int e = blockIdx.x * blockDim.x + threadIdx.x; e < HW; e += gridDim.x * blockDim.x) {
        const int u = e / W, v = e - u * W;
        const int ky = u < (H + 1) / 2 ? u : u - H, kx = v < (W + 1) / 2 ? v : v - W, kp = axis ? kx : ky;
        double2 X = dst[e];
        if (motion) {
            const int l = kp + P / 2;
            int seg = 0;
            for (int i = 0; i < nbreak; ++i) seg += (int)p[KS_BREAK0 + i] <= l;
            const double dy = p[KS_SHIFT0 + 2 * seg], dx = p[KS_SHIFT0 + 2 * seg + 1];
            if (dy != 0.0 || dx != 0.0) {
                const double t = -6.283185307179586 * ((double)ky * dy / (double)H + (double)kx * dx / (double)W);
                double sn, cs;
                sincos(t, &sn, &cs);
                X = ks_mul(X, make_double2(cs, sn));
            }
        }
        if (ghost && kp != 0 && kp % gn == 0) {          // a zero remainder has no sign: C's % agrees with Python's here
            X.x *= gf;
            X.y *= gf;
        }
        if (gibbs && 4.0 * ((double)ky * (double)ky * (double)W * (double)W + (double)kx * (double)kx * (double)H * (double)H) > T)
            X = make_double2(0.0, 0.0);
        for (int s = 0; s < K; ++s) {
            const double* sp = p + KS_SPIKE0 + 4 * s;
            const int su = (int)sp[0], sv = (int)sp[1];
            if (u == su && v == sv) X = ks_add(X, make_double2(A * sp[2], A * sp[3]));
            if (u == (su ? H - su : 0) && v == (sv ? W - sv : 0)) X = ks_add(X, make_double2(A * sp[2], -(A * sp[3])));
        }
        dst[e] = X;
    }
}

// grid (H, B*C), block KS_WT, LDS 2 W complex: row r of the spectrum (already inverted along H) -> inverse along W, / (H W), the
// Rician draw, x = fp32(lo + |z|)
__global__ void __launch_bounds__(KS_WT) kspace_inv_w_kernel(const double2* __restrict__ spec, const double* __restrict__ table,
                                                              const double* __restrict__ stats, const double2* __restrict__ tw,
                                                              float* __restrict__ x, uint32_t seed, uint32_t batch, uint32_t array, int H,
                                                              int W, int C) {
    const int bc = blockIdx.y, b = bc / C, ch = bc - b * C, r = blockIdx.x;
    const int flags = (int)table[(size_t)b * KS_P + KS_FLAGS];
    if (flags == 0) return;
    const bool rician = flags & KS_RICIAN;
    const double lo = stats[(size_t)b * 3], sd = table[(size_t)b * KS_P + KS_STD], hw = (double)H * (double)W;
    const double2* src = spec + ((size_t)bc * H + r) * W;
    double2* a = ks_lds;
    for (int c = threadIdx.x; c < W; c += KS_WT) a[c] = src[c];
    __syncthreads();
    const double2* res = ks_line<true>(a, a + W, tw, W, 1, 0, threadIdx.x, KS_WT);
    float* dst = x + ((size_t)b * H + r) * W * C + ch;
    for (int c = threadIdx.x; c < W; c += KS_WT) {
        double2 z = make_double2(res[c].x / hw, res[c].y / hw);
        if (rician) {
            uint32_t p0, p1;
            philox4x32_10((uint32_t)((r * W + c) * C + ch), (uint32_t)b, array, 5u, seed, batch, p0, p1);
            const double u1 = (double)((p0 >> 8) + 1u) * 0x1p-24, u2 = (double)(p1 >> 8) * 0x1p-24;
            const double rad = sd * sqrt(-2.0 * log(u1));
            double sn, cs;
            sincos(6.283185307179586 * u2, &sn, &cs);
            z.x += rad * cs;
            z.y += rad * sn;
        }
        dst[(size_t)c * C] = (float)(lo + hypot(z.x, z.y));
    }
}

// 2 <= n <= 1024 and no prime factor but 2, 3, 5
static bool ks_extent_ok(int n) {
    if (n < 2 || n > KS_MAXN) return false;
    while (n % 2 == 0) n /= 2;
    while (n % 3 == 0) n /= 3;
    while (n % 5 == 0) n /= 5;
    return n == 1;
}

static bool kspace_shape_ok(int B, int H, int W, int C) {
    return B >= 1 && C >= 1 && (long)B * C <= 65535 && ks_extent_ok(H) && ks_extent_ok(W) && (long)H * W * C <= 0x7fffffffL;
}

static int ks_tile_columns(int H) { return H <= 128 ? 16 : (H <= 256 ? 8 : (H <= 512 ? 4 : 2)); }

static bool ks_aligned(const void* p) { return ((uintptr_t)p & 15) == 0; }

static int ks_launch_h(bool inverse, double* spec, const double* table, const double* tw, int B, int H, int W, int C, hipStream_t stream) {
    const int TC = ks_tile_columns(H);
    const dim3 grid((W + TC - 1) / TC, B * C);
    const size_t lds = (size_t)2 * H * TC * sizeof(double2);
    if (inverse)
        hipLaunchKernelGGL(kspace_h_kernel<true>, grid, dim3(KS_HT), lds, stream, (double2*)spec, table, (const double2*)tw, H, W, C, TC);
    else
        hipLaunchKernelGGL(kspace_h_kernel<false>, grid, dim3(KS_HT), lds, stream, (double2*)spec, table, (const double2*)tw, H, W, C, TC);
    return MMSEG_CHECK_LAUNCH();
}

extern "C" {

// doubles of the spectrum of x [B,H,W,C]: 2 B C H W; 0 for a shape the transform refuses.  Launches nothing.
long mmseg_kspace_workspace_doubles(int B, int H, int W, int C) {
    if (!kspace_shape_ok(B, H, W, C)) return 0;
    return 2L * B * C * H * W;
}

// x [B,H,W,C] fp32, table [B,48] fp64 (column 0: the flags), stats [B,3] fp64 of mmseg_intensity_stats on x, twiddles [H + W] complex
// fp64 (cos, sin (2 pi k / H), k < H, then the same for W) -> spec [B,C,H,W] complex fp64 = fft2(x - lo_b) of the flagged samples
int mmseg_kspace_forward(const float* x, const double* table, const double* stats, const double* twiddles, double* spec, int B, int H,
                         int W, int C, void* stream) {
    if (B <= 0) return 0;
    if (!kspace_shape_ok(B, H, W, C) || !x || !table || !stats || !twiddles || !spec || !ks_aligned(twiddles) || !ks_aligned(spec))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(kspace_fwd_w_kernel, dim3(H, B * C), dim3(KS_WT), (size_t)2 * W * sizeof(double2), (hipStream_t)stream, x, table,
                       stats, (const double2*)twiddles + H, (double2*)spec, H, W, C);
    const int rc = MMSEG_CHECK_LAUNCH();
    if (rc) return rc;
    return ks_launch_h(false, spec, table, twiddles, B, H, W, C, (hipStream_t)stream);
}

// the rule's motion, ghosting, Gibbs truncation and spikes on spec, in place; stats as above (the spikes' amplitude)
int mmseg_kspace_apply(double* spec, const double* table, const double* stats, int B, int H, int W, int C, void* stream) {
    if (B <= 0) return 0;
    if (!kspace_shape_ok(B, H, W, C) || !spec || !table || !stats || !ks_aligned(spec)) return (int)hipErrorInvalidValue;
    const int HW = H * W, n = (HW + KS_MAXBLK - 1) / KS_MAXBLK;
    hipLaunchKernelGGL(kspace_apply_kernel, dim3(n < KS_MAXBLK ? n : KS_MAXBLK, B * C), dim3(KS_MAXBLK), 0, (hipStream_t)stream,
                       (double2*)spec, table, stats, H, W, C);
    return MMSEG_CHECK_LAUNCH();
}

// x = fp32(lo_b + |ifft2(spec) + the Rician draw|) for the flagged samples; spec is overwritten (it holds the transform along H
// afterwards).  seed, batch and array are read as 32-bit patterns.
int mmseg_kspace_inverse(double* spec, const double* table, const double* stats, const double* twiddles, float* x, int seed, int batch,
                         int array, int B, int H, int W, int C, void* stream) {
    if (B <= 0) return 0;
    if (!kspace_shape_ok(B, H, W, C) || !x || !table || !stats || !twiddles || !spec || !ks_aligned(twiddles) || !ks_aligned(spec))
        return (int)hipErrorInvalidValue;
    const int rc = ks_launch_h(true, spec, table, twiddles, B, H, W, C, (hipStream_t)stream);
    if (rc) return rc;
    hipLaunchKernelGGL(kspace_inv_w_kernel, dim3(H, B * C), dim3(KS_WT), (size_t)2 * W * sizeof(double2), (hipStream_t)stream,
                       (const double2*)spec, table, stats, (const double2*)twiddles + H, x, (uint32_t)seed, (uint32_t)batch,
                       (uint32_t)array, H, W, C);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
