// Windowed mean-field CRF refinement of predicted probability maps (build-defined: the reference writes no segmentation; the rule is
// in INTEGRATION.md section 5, "Maps refined against the image", and in include/mmseg_hip.h).
//
// mmseg_crf_refine: prob [N,H,W,C] fp32 (the K organ channels first), image [N,H,W,1] fp32 -> out [N,H,W,K] fp32, the organ channels of
// Q^T.  L = K + 1 labels, the last one "rest" = max(0, 1 - sum of the organs).  Launches, all on the caller's stream:
//   crf_table_kernel  once: per window offset the appearance exponent -|d|^2 / (2 theta_alpha^2) * log2(e) and the smoothness factor
//                     exp(-|d|^2 / (2 theta_gamma^2)), both from fp64, into the head of the workspace
//   crf_init_kernel   once: Q^0 = softmax(u), planar [N,L,H,W], into the first Q buffer
//   crf_iter_kernel   once per iteration, ping-pong between the two Q buffers; the last one writes `out` instead
//
// crf_iter_kernel: a block of 256 threads owns a 32 x 8 tile of one slice, a thread one pixel.  The image tile with its halo of r pixels
// and the Q tile with its halo for a chunk of CH <= 6 labels are staged in LDS (planes of (8 + 2r) x (32 + 2r) floats: 32 KB at r = 8,
// CH = 6; 18 KB at r = 5, CH = 5, so that several blocks share a CU).  Pixels beyond the slice are staged as +inf (image) and 0 (Q): the
// appearance weight of such a neighbour is exp2(-inf) = 0 and its Q adds nothing, so that the window loop holds no bounds test; the
// smoothness sum counts a neighbour when its image value is finite.  The appearance weight is computed once per neighbour and used
// for every label of the chunk; L > 6 takes 2 or 3 chunks of equal size (labels past L are staged as 0 and dropped), each of which
// walks the window again.  The lanes of a half wave read consecutive floats of an LDS row: no bank conflicts.  The unary is
// recomputed from prob in every iteration.  A gather: no atomics, a fixed order of summation, two runs are bitwise equal.
#include "common.hpp"

#include <math.h>

namespace {

constexpr int CRF_TW = 32, CRF_TH = 8, CRF_BLOCK = CRF_TW * CRF_TH;
constexpr int CRF_MAXR = 8, CRF_MAXT = 20, CRF_MAXK = 16;
constexpr int CRF_TABLE = (2 * CRF_MAXR + 1) * (2 * CRF_MAXR + 1);          // entries of one table of window offsets
constexpr long CRF_HEAD_FLOATS = 1024;          // the two tables at the head of the workspace, rounded up
constexpr float CRF_FLOOR = 1e-6f;

// the messages of a pixel in v (labels j < L = K + 1 are in use) -> Q = softmax_l(log(max(P_l, 1e-6)) + v_l); p: the pixel's channels
template <int CAP> __device__ __forceinline__ void crf_softmax(const float* __restrict__ p, int K, float (&v)[CAP]) {
    const int L = K + 1;
    float organs = 0.f;
    for (int k = 0; k < K; ++k) organs += p[k];
    const float rest = fmaxf(0.f, 1.f - organs);
    float top = -INFINITY;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j < L) {
            v[j] += logf(fmaxf(j < K ? p[j] : rest, CRF_FLOOR));
            top = fmaxf(top, v[j]);
        }
    float sum = 0.f;
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j < L) {
            v[j] = expf(v[j] - top);
            sum += v[j];
        }
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j < L) v[j] = v[j] / sum;
}

// tab[i] = -|d|^2 / (2 theta_alpha^2) * log2(e), tab[CRF_TABLE + i] = exp(-|d|^2 / (2 theta_gamma^2)) for offset i = (dy + r) * (2r + 1) + dx + r
__global__ void crf_table_kernel(float* __restrict__ tab, int r, double theta_alpha, double theta_gamma) {
    const int side = 2 * r + 1, i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= side * side) return;
    const int dy = i / side - r, dx = i % side - r;
    const double d2 = (double)(dy * dy + dx * dx);
    tab[i] = (float)(-d2 / (2.0 * theta_alpha * theta_alpha) * 1.4426950408889634);
    tab[CRF_TABLE + i] = (float)exp(-d2 / (2.0 * theta_gamma * theta_gamma));
}

template <int CAP>
__global__ __launch_bounds__(CRF_BLOCK) void crf_init_kernel(const float* __restrict__ prob, float* __restrict__ q, long pixels, int HW,
                                                             int C, int K) {
    const long i = (long)blockIdx.x * CRF_BLOCK + threadIdx.x;
    if (i >= pixels) return;
    float v[CAP];
#pragma unroll
    for (int j = 0; j < CAP; ++j) v[j] = 0.f;
    crf_softmax<CAP>(prob + (size_t)i * C, K, v);
    const long n = i / HW;
    float* dst = q + (size_t)n * (K + 1) * HW + (i - n * HW);
#pragma unroll
    for (int j = 0; j < CAP; ++j)
        if (j <= K) dst[(size_t)j * HW] = v[j];
}

// One mean-field iteration.  qin, qout: planar [N,L,H,W]; on the last iteration qout is null and `out` [N,H,W,K] is written.
template <int CH, int NCH>
__global__ __launch_bounds__(CRF_BLOCK) void crf_iter_kernel(const float* __restrict__ prob, const float* __restrict__ image,
                                                             const float* __restrict__ qin, float* __restrict__ qout,
                                                             float* __restrict__ out, const float* __restrict__ tab, int H, int W, int C,
                                                             int K, int r, int tiles_x, int tiles_y, float cb, float w_a, float w_s) {
    extern __shared__ float lds[];
    const int L = K + 1, HW = H * W;
    const int SW = CRF_TW + 2 * r, plane = SW * (CRF_TH + 2 * r), side = 2 * r + 1;
    float* simg = lds;
    float* sq = lds + plane;
    int b = blockIdx.x;
    const int x0 = (b % tiles_x) * CRF_TW;
    b /= tiles_x;
    const int y0 = (b % tiles_y) * CRF_TH, n = b / tiles_y;
    const int lx = threadIdx.x & (CRF_TW - 1), ly = threadIdx.x / CRF_TW;
    const int x = x0 + lx, y = y0 + ly;
    const float* img = image + (size_t)n * HW;
    const float* qn = qin + (size_t)n * L * HW;
    const int centre = (ly + r) * SW + lx + r;

    float m[CH * NCH];
#pragma unroll
    for (int c = 0; c < NCH; ++c) {
        if (c) __syncthreads();          // every thread is done with the previous chunk
        for (int i = threadIdx.x; i < plane; i += CRF_BLOCK) {
            const int sy = i / SW, gy = y0 - r + sy, gx = x0 - r + (i - sy * SW);
            const bool inside = (unsigned)gy < (unsigned)H && (unsigned)gx < (unsigned)W;
            const int g = gy * W + gx;
            if (c == 0) simg[i] = inside ? img[g] : INFINITY;
#pragma unroll
            for (int j = 0; j < CH; ++j) sq[j * plane + i] = (inside && c * CH + j < L) ? qn[(size_t)(c * CH + j) * HW + g] : 0.f;
        }
        __syncthreads();
        const float ip = simg[centre];
        float na[CH], ns[CH], da = 0.f, ds = 0.f;
#pragma unroll
        for (int j = 0; j < CH; ++j) na[j] = ns[j] = 0.f;
        for (int dy = -r; dy <= r; ++dy) {
            const float* ta = tab + (dy + r) * side + r;
            const int row = centre + dy * SW;
            for (int dx = -r; dx <= r; ++dx) {
                if ((dy | dx) == 0) continue;
                const float ka = ta[dx], ks = ta[CRF_TABLE + dx];
                const float iq = simg[row + dx], d = ip - iq;
                const float a = __builtin_amdgcn_exp2f(fmaf(d * d, cb, ka));          // 0 for a neighbour beyond the slice
                da += a;
                ds += iq < INFINITY ? ks : 0.f;
#pragma unroll
                for (int j = 0; j < CH; ++j) {
                    const float q = sq[j * plane + row + dx];
                    na[j] = fmaf(a, q, na[j]);
                    ns[j] = fmaf(ks, q, ns[j]);
                }
            }
        }
        // each kernel is normalised by its own sum; no neighbour (or an appearance sum that underflowed to 0) gives no message
#pragma unroll
        for (int j = 0; j < CH; ++j) m[c * CH + j] = w_a * (da > 0.f ? na[j] / da : 0.f) + w_s * (ds > 0.f ? ns[j] / ds : 0.f);
    }
    if (x >= W || y >= H) return;
    const size_t px = (size_t)n * HW + (size_t)y * W + x;
    crf_softmax<CH * NCH>(prob + px * C, K, m);
    if (qout) {
        float* dst = qout + (size_t)n * L * HW + (size_t)y * W + x;
#pragma unroll
        for (int j = 0; j < CH * NCH; ++j)
            if (j < L) dst[(size_t)j * HW] = m[j];
    } else {
#pragma unroll
        for (int j = 0; j < CH * NCH; ++j)
            if (j < K) out[px * K + j] = m[j];
    }
}

struct crf_args {
    const float *prob, *image;
    float *out, *ws;
    int N, H, W, C, K, radius, iterations;
    float w_a, theta_alpha, theta_beta, w_s, theta_gamma;
};

template <int CH, int NCH> int crf_launch(const crf_args& a, hipStream_t st) {
    const int L = a.K + 1, HW = a.H * a.W;
    const long pixels = (long)a.N * HW;
    float* tab = a.ws;
    float* q[2] = {a.ws + CRF_HEAD_FLOATS, a.ws + CRF_HEAD_FLOATS + (size_t)pixels * L};
    const int side = 2 * a.radius + 1;
    hipLaunchKernelGGL(crf_table_kernel, dim3((side * side + 63) / 64), dim3(64), 0, st, tab, a.radius, (double)a.theta_alpha,
                       (double)a.theta_gamma);
    hipLaunchKernelGGL(crf_init_kernel<CH * NCH>, dim3((unsigned)((pixels + CRF_BLOCK - 1) / CRF_BLOCK)), dim3(CRF_BLOCK), 0, st, a.prob, q[0],
                       pixels, HW, a.C, a.K);
    const int tiles_x = (a.W + CRF_TW - 1) / CRF_TW, tiles_y = (a.H + CRF_TH - 1) / CRF_TH;
    const long blocks = (long)tiles_x * tiles_y * a.N;          // at most one block per pixel: below 2^29
    const size_t lds = sizeof(float) * (1 + CH) * (CRF_TW + 2 * a.radius) * (CRF_TH + 2 * a.radius);
    const float cb = (float)(-1.4426950408889634 / (2.0 * (double)a.theta_beta * (double)a.theta_beta));
    for (int t = 0; t < a.iterations; ++t) {
        const bool last = t + 1 == a.iterations;
        hipLaunchKernelGGL((crf_iter_kernel<CH, NCH>), dim3((unsigned)blocks), dim3(CRF_BLOCK), lds, st, a.prob, a.image, q[t & 1],
                           last ? nullptr : q[(t + 1) & 1], a.out, tab, a.H, a.W, a.C, a.K, a.radius, tiles_x, tiles_y, cb, a.w_a, a.w_s);
    }
    return MMSEG_CHECK_LAUNCH();
}

// bytes of [lo, lo + n) and [p, p + m) overlap
bool crf_overlap(const void* lo, long n, const void* p, long m) {
    const uintptr_t a = (uintptr_t)lo, b = (uintptr_t)p;
    return a < b + (uintptr_t)m && b < a + (uintptr_t)n;
}

bool crf_positive(float v) { return v > 0.f && v < INFINITY; }
bool crf_weight(float v) { return v >= 0.f && v < INFINITY; }

// the sizes of the rule; bytes[0..2] = prob, image, out
bool crf_sizes_ok(int N, int H, int W, int C, int K, long* bytes) {
    if (N < 1 || H < 1 || W < 1 || C < 1 || K < 1 || K > C || K > CRF_MAXK) return false;
    const long lim = 0x80000000L;
    long px = (long)sizeof(float) * N;          // factor by factor, so that no product overflows before it is compared
    for (const int f : {H, W}) {
        px *= f;
        if (px >= lim) return false;
    }
    if (px * C >= lim) return false;
    if (bytes) bytes[0] = px * C, bytes[1] = px, bytes[2] = px * K;
    return true;
}

}  // namespace

extern "C" {

// the two tables, then two planar Q buffers [N,K+1,H,W]
long mmseg_crf_refine_workspace_bytes(int N, int H, int W, int K) {
    if (!crf_sizes_ok(N, H, W, K, K, nullptr)) return 0;
    return (long)sizeof(float) * (CRF_HEAD_FLOATS + 2L * N * H * W * (K + 1));
}

int mmseg_crf_refine(const float* prob, const float* image, float* out, void* ws, int N, int H, int W, int C, int K, int radius,
                     int iterations, float w_a, float theta_alpha, float theta_beta, float w_s, float theta_gamma, void* stream) {
    if (N == 0) return 0;
    long bytes[3];
    if (!prob || !image || !out || !ws || !crf_sizes_ok(N, H, W, C, K, bytes) || radius < 1 || radius > CRF_MAXR || iterations < 1 ||
        iterations > CRF_MAXT || !crf_positive(theta_alpha) || !crf_positive(theta_beta) || !crf_positive(theta_gamma) || !crf_weight(w_a) ||
        !crf_weight(w_s) || (w_a == 0.f && w_s == 0.f))
        return (int)hipErrorInvalidValue;
    const long ws_bytes = mmseg_crf_refine_workspace_bytes(N, H, W, K);
    if (crf_overlap(out, bytes[2], prob, bytes[0]) || crf_overlap(out, bytes[2], image, bytes[1]) || crf_overlap(ws, ws_bytes, prob, bytes[0]) ||
        crf_overlap(ws, ws_bytes, image, bytes[1]) || crf_overlap(ws, ws_bytes, out, bytes[2]) || ((uintptr_t)ws & 3))
        return (int)hipErrorInvalidValue;
    const crf_args a = {prob, image, out, (float*)ws, N, H, W, C, K, radius, iterations, w_a, theta_alpha, theta_beta, w_s, theta_gamma};
    const hipStream_t st = (hipStream_t)stream;
    switch (K + 1) {          // chunks of equal size, at most 6 labels each
        case 2: return crf_launch<2, 1>(a, st);
        case 3: return crf_launch<3, 1>(a, st);
        case 4: return crf_launch<4, 1>(a, st);
        case 5: return crf_launch<5, 1>(a, st);
        case 6: return crf_launch<6, 1>(a, st);
        case 7: case 8: return crf_launch<4, 2>(a, st);
        case 9: case 10: return crf_launch<5, 2>(a, st);
        case 11: case 12: return crf_launch<6, 2>(a, st);
        case 13: case 14: case 15: return crf_launch<5, 3>(a, st);
        default: return crf_launch<6, 3>(a, st);
    }
}

}  // extern "C"
