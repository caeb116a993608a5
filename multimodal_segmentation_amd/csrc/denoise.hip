// Non-local means denoising of one MR volume at load time (build-defined: the reference loads CHAOS as exported; the rule is in
// include/mmseg_hip.h, "non-local means denoising", and in INTEGRATION.md section 5).
//
// mmseg_nlm_sigma: x [S,H,W] fp32 -> Immerkaer's noise estimate, one fp64 scalar on the device.  Two launches:
//   nlm_sigma_partial_kernel  NB = min(NLM_SIGMA_BLOCKS, ceil(interior / 256)) blocks; a thread walks the interior pixels blk * 256 + tid +
//                             k * NB * 256, k ascending, and adds |L * x| in fp64; the block's 256 sums are added by a tree in LDS; one
//                             partial per block goes to the workspace
//   nlm_sigma_final_kernel    one block adds the partials (thread t takes t, t + 256, ..., then the same tree) and writes sigma
// The order depends on the shape alone, so two runs are bitwise equal; no block waits for another.
//
// mmseg_nlm_denoise: one launch of nlm_kernel<RP>.  A block of 256 threads owns a 32 x 8 tile of one slice, a thread one voxel.  The
// tile of the centre plane with a halo of Rs + Rp is staged in LDS with its coordinates already clamped to the slice, so that the walk
// over offsets and patch taps holds no bounds logic: a tap beyond the slice reads the replicated edge, as the rule says.  For dz != 0 the
// same window of the neighbour plane is staged into a second plane (two planes of 58 x 34 floats at the largest radii: 15.8 KB, so
// several blocks share a CU).  A thread keeps its own (2 Rp + 1)^2 patch in registers and reads the neighbour's patch from LDS, one
// word per tap; a neighbour outside the slice takes part with the weight 0, which leaves every sum's bits as skipping it would.  The 32
// lanes of a half wave read 32 consecutive floats of one LDS row at every tap, so that no read has a bank conflict whatever the row
// length (tools/volume_denoise_bench.py --lds enumerates it); rows are therefore not padded.  A gather: no atomics, sums in the rule's
// walk order, two runs are bitwise equal.  With Rz = 0 a block reads its own slice only.
//
// The other form that was measured -- per offset the squared differences of the tile plus its Rp rim written to LDS once and the patch
// distance taken as a separable box sum over them, two barriers per offset -- took 0.36 ms against 0.20 ms at the defaults (Rp = 1) on a
// 36 x 256 x 256 volume and is not kept; at Rp = 3 it was the faster one, 2.1 ms against 3.3 ms (profiles/volume_denoise_bench.md, DESIGN.md
// section 8).
#include "common.hpp"

#include <math.h>

namespace {

constexpr int NLM_TW = 32, NLM_TH = 8, NLM_BLOCK = NLM_TW * NLM_TH;
constexpr int NLM_MAX_RS = 10, NLM_MAX_RP = 3, NLM_MAX_RZ = 4;
constexpr int NLM_SIGMA_BLOCKS = 1024;          // partials of the sigma reduction: the workspace holds this many doubles
constexpr float NLM_LOG2E = 1.4426950408889634f;
constexpr float NLM_MIN_ARG = -126.f;          // a weight below 2^-126 is 0

// the 256 values of a block, one per thread, added by a tree in LDS; the sum is valid in thread 0
__device__ __forceinline__ double nlm_block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
#pragma unroll
    for (int o = NLM_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(NLM_BLOCK) void nlm_sigma_partial_kernel(const float* __restrict__ x, double* __restrict__ part, long interior,
                                                                       int H, int W) {
    __shared__ double red[NLM_BLOCK];
    const int IW = W - 2, IHW = (H - 2) * IW;
    const long stride = (long)gridDim.x * NLM_BLOCK;
    double acc = 0.0;
    for (long i = (long)blockIdx.x * NLM_BLOCK + threadIdx.x; i < interior; i += stride) {
        const long s = i / IHW;
        const int r = (int)(i - s * IHW), y = 1 + r / IW, c = 1 + r % IW;
        const float* p = x + (size_t)s * H * W + (size_t)y * W + c;
        const double corners = (double)p[-W - 1] + (double)p[-W + 1] + (double)p[W - 1] + (double)p[W + 1];
        const double edges = (double)p[-W] + (double)p[-1] + (double)p[1] + (double)p[W];
        acc += fabs(corners - 2.0 * edges + 4.0 * (double)p[0]);
    }
    const double sum = nlm_block_sum(acc, red);
    if (threadIdx.x == 0) part[blockIdx.x] = sum;
}

// <<<1, NLM_BLOCK>>>
__global__ __launch_bounds__(NLM_BLOCK) void nlm_sigma_final_kernel(const double* __restrict__ part, int nb, double* __restrict__ sigma,
                                                                     double interior) {
    __shared__ double red[NLM_BLOCK];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += NLM_BLOCK) acc += part[b];
    const double sum = nlm_block_sum(acc, red);
    if (threadIdx.x == 0) sigma[0] = interior > 0.0 ? 1.2533141373155003 / (6.0 * interior) * sum : 0.0;          // sqrt(pi / 2)
}

// plane [SH, SW] <- the window of slice `src` [H, W] whose corner is (y0 - halo, x0 - halo), coordinates clamped to the slice
__device__ __forceinline__ void nlm_stage(float* __restrict__ plane, const float* __restrict__ src, int y0, int x0, int halo, int SW, int SH,
                                          int H, int W) {
    for (int i = threadIdx.x; i < SW * SH; i += NLM_BLOCK) {
        const int sy = i / SW, sx = i - sy * SW;
        const int gy = min(max(y0 - halo + sy, 0), H - 1), gx = min(max(x0 - halo + sx, 0), W - 1);
        plane[i] = src[(size_t)gy * W + gx];
    }
}

template <int RP>
__global__ __launch_bounds__(NLM_BLOCK) void nlm_kernel(const float* __restrict__ x, float* __restrict__ out,
                                                        const double* __restrict__ sigma_dev, double sigma_val, int S, int H, int W, int Rs,
                                                        int Rz, float h, int rician, int tiles_x, int tiles_y) {
    extern __shared__ float lds[];
    constexpr int PW = 2 * RP + 1, TAPS = PW * PW;
    const int halo = Rs + RP, SW = NLM_TW + 2 * halo, SH = NLM_TH + 2 * halo;
    float* sc = lds;
    float* sn = lds + SW * SH;
    int b = blockIdx.x;
    const int x0 = (b % tiles_x) * NLM_TW;
    b /= tiles_x;
    const int y0 = (b % tiles_y) * NLM_TH, s = b / tiles_y;
    const int lx = threadIdx.x & (NLM_TW - 1), ly = threadIdx.x / NLM_TW;
    const int gx = x0 + lx, gy = y0 + ly;
    const bool mine = gx < W && gy < H;
    const size_t HW = (size_t)H * W, px = (size_t)s * HW + (size_t)gy * W + gx;

    // the constants of the weight, in fp32.  A sigma that leaves one of them outside the positive finite numbers: the volume keeps its bits
    const float sig = (float)(sigma_dev ? sigma_dev[0] : sigma_val);
    const float two_s2 = 2.f * sig * sig, hs = h * sig, g = hs * hs;
    const float cw = -NLM_LOG2E / g;
    if (!(sig > 0.f && two_s2 < INFINITY && g > 0.f && g < INFINITY && cw > -INFINITY)) {          // the same decision in every block
        if (mine) out[px] = x[px];
        return;
    }

    nlm_stage(sc, x + (size_t)s * HW, y0, x0, halo, SW, SH, H, W);
    __syncthreads();
    const int centre = (ly + halo) * SW + lx + halo;
    float cp[TAPS];
#pragma unroll
    for (int a = 0; a < PW; ++a)
#pragma unroll
        for (int c = 0; c < PW; ++c) cp[a * PW + c] = sc[centre + (a - RP) * SW + (c - RP)];
    const float up = cp[RP * PW + RP];
    const float inv_taps = 1.f / (float)TAPS;

    float sw = 0.f, sv = 0.f, wmax = 0.f;
    for (int dz = -Rz; dz <= Rz; ++dz) {
        const int sz = s + dz;
        if (sz < 0 || sz >= S) continue;          // block-uniform: every thread of the block takes the barriers below or none does
        const float* nb = sc;
        if (dz != 0) {
            __syncthreads();          // every thread is done with the previous neighbour plane
            nlm_stage(sn, x + (size_t)sz * HW, y0, x0, halo, SW, SH, H, W);
            __syncthreads();
            nb = sn;
        }
        for (int dy = -Rs; dy <= Rs; ++dy) {
            const bool row_in = (unsigned)(gy + dy) < (unsigned)H;
            const float* q = nb + centre + dy * SW - RP * SW - RP;          // the corner of the neighbour's patch at dx = 0
            for (int dx = -Rs; dx <= Rs; ++dx) {
                if ((dz | dy | dx) == 0) continue;
                float d = 0.f;
#pragma unroll
                for (int a = 0; a < PW; ++a)
#pragma unroll
                    for (int c = 0; c < PW; ++c) {
                        const float e = cp[a * PW + c] - q[dx + a * SW + c];
                        d = fmaf(e, e, d);
                    }
                const float uq = q[dx + RP * SW + RP];
                const float arg = fmaxf(fmaf(d, inv_taps, -two_s2), 0.f) * cw;
                float w = arg >= NLM_MIN_ARG ? __builtin_amdgcn_exp2f(arg) : 0.f;          // no denormal weights, whatever the hardware's mode
                w = (row_in && (unsigned)(gx + dx) < (unsigned)W) ? w : 0.f;          // a neighbour outside the slice: as if skipped
                wmax = fmaxf(wmax, w);
                sw += w;
                sv = fmaf(w, rician ? uq * uq : uq, sv);
            }
        }
    }
    if (!mine) return;
    sw += wmax;          // the centre, last, with the largest of the other weights
    sv = fmaf(wmax, rician ? up * up : up, sv);
    float r = up;
    if (sw > 0.f) {
        const float m = sv / sw;
        r = rician ? sqrtf(fmaxf(m - two_s2, 0.f)) : m;
    }
    out[px] = r;
}

// S, H, W >= 1 (S >= 0 when `empty`) and S * H * W < 2^31 - 1
bool nlm_shape_ok(int S, int H, int W, bool empty) {
    if (S < (empty ? 0 : 1) || H < 1 || W < 1) return false;
    return (long)S * H < 0x7fffffffL && (long)S * H * W < 0x7fffffffL;          // S * H < 2^31, so the second product fits 62 bits
}

}  // namespace

extern "C" {

long mmseg_nlm_workspace_bytes(int S, int H, int W) {
    return nlm_shape_ok(S, H, W, false) ? (long)sizeof(double) * NLM_SIGMA_BLOCKS : 0;
}

int mmseg_nlm_sigma(const float* x, double* ws, double* sigma_out, int S, int H, int W, void* stream) {
    if (!nlm_shape_ok(S, H, W, true)) return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    if (!x || !ws || !sigma_out || ((uintptr_t)ws & 7) || ((uintptr_t)sigma_out & 7)) return (int)hipErrorInvalidValue;
    const long interior = (H < 3 || W < 3) ? 0 : (long)S * (H - 2) * (W - 2);
    const long want = (interior + NLM_BLOCK - 1) / NLM_BLOCK;
    const int nb = want < 1 ? 1 : (want > NLM_SIGMA_BLOCKS ? NLM_SIGMA_BLOCKS : (int)want);
    const hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(nlm_sigma_partial_kernel, dim3(nb), dim3(NLM_BLOCK), 0, st, x, ws, interior, H, W);
    hipLaunchKernelGGL(nlm_sigma_final_kernel, dim3(1), dim3(NLM_BLOCK), 0, st, (const double*)ws, nb, sigma_out, (double)interior);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_nlm_denoise(const float* x, float* out, const double* sigma_dev, double sigma, int S, int H, int W, int search_radius,
                      int patch_radius, int search_radius_z, float h, int rician, void* stream) {
    if (!nlm_shape_ok(S, H, W, true) || search_radius < 1 || search_radius > NLM_MAX_RS || patch_radius < 1 || patch_radius > NLM_MAX_RP ||
        search_radius_z < 0 || search_radius_z > NLM_MAX_RZ || !(h > 0.f && h < INFINITY) || (rician != 0 && rician != 1))
        return (int)hipErrorInvalidValue;
    if (S == 0) return 0;
    if (!x || !out || ((uintptr_t)sigma_dev & 7)) return (int)hipErrorInvalidValue;
    const uintptr_t bytes = (uintptr_t)sizeof(float) * S * H * W, a = (uintptr_t)x, o = (uintptr_t)out;
    if (a < o + bytes && o < a + bytes) return (int)hipErrorInvalidValue;          // out overlaps x
    const int tiles_x = (W + NLM_TW - 1) / NLM_TW, tiles_y = (H + NLM_TH - 1) / NLM_TH;
    const long blocks = (long)tiles_x * tiles_y * S;          // at most one block per voxel: below 2^31
    const int halo = search_radius + patch_radius;
    const size_t lds = sizeof(float) * 2 * (NLM_TW + 2 * halo) * (NLM_TH + 2 * halo);
    const hipStream_t st = (hipStream_t)stream;
#define NLM_LAUNCH(RP)                                                                                                                     \
    hipLaunchKernelGGL(nlm_kernel<RP>, dim3((unsigned)blocks), dim3(NLM_BLOCK), lds, st, x, out, sigma_dev, sigma, S, H, W, search_radius, \
                       search_radius_z, h, rician, tiles_x, tiles_y)
    switch (patch_radius) {
        case 1: NLM_LAUNCH(1); break;
        case 2: NLM_LAUNCH(2); break;
        default: NLM_LAUNCH(3); break;
    }
#undef NLM_LAUNCH
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
