// Volume preprocessing on the device (gfx950): what the reference does on the host, slice by slice, between reading a volume and
// filling its containers (loaders/chaos.py:242-246 `rescale`, 248-264 `crop_same`, 303-319 label split, 324-343 `resample`).
//
// One (volume, modality) = S raw slices [S,H,W] (image fp32, label uint8) uploaded once.  Per slice, in the reference's order:
//   resample   to RH x RW = round(H * old_res / target_res) (half to even, decided by the host).  Source coordinate of resampled pixel d:
//              (d + 0.5) * (in / out) - 0.5 in fp64 (no contraction, so the host can reproduce it bit for bit).  A coordinate outside
//              [0, in-1] on either axis gives 0 (scipy's strict 'constant' rule, as in augment.hip).  Image: bilinear,
//              v = (1-fy)*((1-fx)*a00 + fx*a01) + fy*((1-fx)*a10 + fx*a11) in fp32 in that order; label: the tap floor(c + 0.5).
//   split      channel k = (resampled label == values[k]) as 0 / 1
//   rescale    every slice to [-1, 1] with the (min, max) of the WHOLE resampled slice: out = 2*(v - lo)/(hi - lo) - 1, a constant
//              slice becomes -1.  v == lo gives exactly -1, v == hi exactly +1 (x / x == 1 in IEEE division).
//   crop / pad to OH x OW: final index o -> resampled index lo + clamp(o - before, 0, kept - 1) per axis; (lo, kept, before) come
//              from the host and carry the odd-surplus quirk of utils/data_utils._crop.  Edge padding is the clamp.
// The resampled slice never exists in memory: pp_minmax_kernel recomputes the interpolation over the RH x RW frame and leaves
// per-block (min, max) partials; pp_image_kernel folds the partials of its slice (a fixed set, min / max are order independent:
// bitwise reproducible), recomputes the interpolation at the pixels it keeps and writes channel `ch` of the NHWC container
// [S,OH,OW,C] that the gather kernels of augment.hip read.  Both passes call the same non-contracted pp_bilinear, so the extreme
// pixel reproduces the reduced extreme bit for bit.
// Traffic: one read of the raw slices per pass, one write of the container -- a few hundred MB for a whole data set, once per run.
// Stores: consecutive lanes take consecutive pixels.  A modality owns ONE image channel of the container, so its image stores are 4
// bytes at a stride of C floats (C = 2 or 3 modalities): a wave's store covers 512 or 768 contiguous bytes and fills a half or a
// third of them; the other modalities' launches fill the rest.  Writing all channels from one launch would need every modality's
// raw slices, each with its own geometry, in one kernel -- not worth it for a few MB per volume.  A modality's num_masks mask
// channels are contiguous: one 16-byte store per pixel when num_masks == 4 (the channel offset is then a multiple of 16 bytes).
#include "common.hpp"
#include "resample.hpp"

#define PP_BLOCK 256
#define PP_MAXBLK 64
#define PP_MAXVALUES 16

struct pp_axis {
    int lo, kept, before;
};

// pp_coord and pp_bilinear, the resampling itself, are in resample.hpp (align.hip meets the same values)

__device__ __forceinline__ void pp_minmax_block(float lo, float hi, float* out) {
    __shared__ float red[2][PP_BLOCK / 64];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        lo = fminf(lo, __shfl_xor(lo, o, 64));
        hi = fmaxf(hi, __shfl_xor(hi, o, 64));
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    if (lane == 0) { red[0][wid] = lo; red[1][wid] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < PP_BLOCK / 64; ++w) { lo = fminf(lo, red[0][w]); hi = fmaxf(hi, red[1][w]); }
        out[0] = lo;
        out[1] = hi;
    }
}

// grid (nblk, S), block PP_BLOCK: part[s][blk] = (min, max) of this block's share of the resampled slice s
__global__ void __launch_bounds__(PP_BLOCK) pp_minmax_kernel(const float* __restrict__ img, float* __restrict__ part, int H, int W,
                                                             int RH, int RW, double ry, double rx) {
    const int s = blockIdx.y;
    const float* src = img + (size_t)s * H * W;
    float lo = INFINITY, hi = -INFINITY;
    const int n = RH * RW;
    for (int e = blockIdx.x * PP_BLOCK + threadIdx.x; e < n; e += gridDim.x * PP_BLOCK) {
        const int dr = e / RW, dc = e - dr * RW;
        const float v = pp_bilinear(src, H, W, dr, dc, ry, rx);
        lo = fminf(lo, v);
        hi = fmaxf(hi, v);
    }
    pp_minmax_block(lo, hi, part + ((size_t)s * gridDim.x + blockIdx.x) * 2);
}

// grid (nblk, S), block PP_BLOCK: out[s, r, c, ch] = rescaled resampled pixel; `npart` partials per slice from pp_minmax_kernel
__global__ void __launch_bounds__(PP_BLOCK) pp_image_kernel(const float* __restrict__ img, const float* __restrict__ part, int npart,
                                                            float* __restrict__ out, int H, int W, double ry, double rx, int OH, int OW,
                                                            pp_axis ar, pp_axis ac, int C, int ch) {
    __shared__ float mm[2];
    const int s = blockIdx.y;
    const float* pp = part + (size_t)s * npart * 2;
    float lo = INFINITY, hi = -INFINITY;
    for (int i = threadIdx.x; i < npart; i += PP_BLOCK) { lo = fminf(lo, pp[2 * i]); hi = fmaxf(hi, pp[2 * i + 1]); }
    pp_minmax_block(lo, hi, mm);
    __syncthreads();
    lo = mm[0];
    hi = mm[1];
    const float range = hi - lo;
    const float* src = img + (size_t)s * H * W;
    float* dst = out + (size_t)s * OH * OW * C + ch;
    const int n = OH * OW;
    for (int e = blockIdx.x * PP_BLOCK + threadIdx.x; e < n; e += gridDim.x * PP_BLOCK) {
        const int r = e / OW, c = e - r * OW;
        const int dr = ar.lo + min(max(r - ar.before, 0), ar.kept - 1);
        const int dc = ac.lo + min(max(c - ac.before, 0), ac.kept - 1);
        const float v = pp_bilinear(src, H, W, dr, dc, ry, rx);
        dst[(size_t)e * C] = hi == lo ? -1.f : 2.f * (v - lo) / range - 1.f;
    }
}

// grid (nblk, S), block PP_BLOCK: out[s, r, c, ch0 + k] = (nearest resampled label == values[k])
__global__ void __launch_bounds__(PP_BLOCK) pp_label_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int K,
                                                            float* __restrict__ out, int H, int W, double ry, double rx, int OH, int OW,
                                                            pp_axis ar, pp_axis ac, int C, int ch0) {
    __shared__ int vals[PP_MAXVALUES];
    if (threadIdx.x < K) vals[threadIdx.x] = values[threadIdx.x];
    __syncthreads();
    const int s = blockIdx.y;
    const unsigned char* src = lab + (size_t)s * H * W;
    float* dst = out + (size_t)s * OH * OW * C + ch0;
    const int n = OH * OW;
    const bool vec4 = K == 4 && (C & 3) == 0 && (ch0 & 3) == 0 && ((uintptr_t)out & 15) == 0;
    for (int e = blockIdx.x * PP_BLOCK + threadIdx.x; e < n; e += gridDim.x * PP_BLOCK) {
        const int r = e / OW, c = e - r * OW;
        const int dr = ar.lo + min(max(r - ar.before, 0), ar.kept - 1);
        const int dc = ac.lo + min(max(c - ac.before, 0), ac.kept - 1);
        const double sy = pp_coord(dr, ry), sx = pp_coord(dc, rx);
        int g = 0;
        if (sy >= 0.0 && sy <= (double)(H - 1) && sx >= 0.0 && sx <= (double)(W - 1)) {
            const int rr = min((int)floor(sy + 0.5), H - 1), cc = min((int)floor(sx + 0.5), W - 1);
            g = src[(size_t)rr * W + cc];
        }
        float* p = dst + (size_t)e * C;
        if (vec4) {
            f32x4 o;
            o[0] = g == vals[0] ? 1.f : 0.f;
            o[1] = g == vals[1] ? 1.f : 0.f;
            o[2] = g == vals[2] ? 1.f : 0.f;
            o[3] = g == vals[3] ? 1.f : 0.f;
            *reinterpret_cast<f32x4*>(p) = o;
        } else {
            for (int k = 0; k < K; ++k) p[k] = g == vals[k] ? 1.f : 0.f;
        }
    }
}

static int pp_blocks(long n) {
    const long b = (n + PP_BLOCK - 1) / PP_BLOCK;
    return (int)(b < 1 ? 1 : (b < PP_MAXBLK ? b : PP_MAXBLK));
}

// the output index map must stay inside the resampled frame: 0 <= lo, 1 <= kept, lo + kept <= R, 0 <= before < O
static bool pp_axis_ok(int lo, int kept, int before, int R, int O) {
    return lo >= 0 && kept >= 1 && (long)lo + kept <= R && before >= 0 && before < O;
}

static bool pp_geometry_ok(int S, int H, int W, int RH, int RW) {
    return S <= 65535 && H >= 1 && W >= 1 && RH >= 1 && RW >= 1 && (long)H * W < 0x7fffffffL && (long)RH * RW < 0x7fffffffL - PP_MAXBLK * PP_BLOCK;
}

extern "C" {

// floats of the (min, max) partials that mmseg_preprocess_minmax writes and mmseg_preprocess_image reads
long mmseg_preprocess_workspace_floats(int S, int RH, int RW) {
    if (S < 1 || RH < 1 || RW < 1) return 0;
    return 2L * S * pp_blocks((long)RH * RW);
}

// img [S,H,W] raw slices; ws: mmseg_preprocess_workspace_floats(S, RH, RW) floats
int mmseg_preprocess_minmax(const float* img, float* ws, int S, int H, int W, int RH, int RW, void* stream) {
    if (S <= 0) return 0;
    if (!img || !ws || !pp_geometry_ok(S, H, W, RH, RW)) return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)pp_blocks((long)RH * RW), S);
    hipLaunchKernelGGL(pp_minmax_kernel, grid, dim3(PP_BLOCK), 0, (hipStream_t)stream, img, ws, H, W, RH, RW, (double)H / (double)RH,
                       (double)W / (double)RW);
    return MMSEG_CHECK_LAUNCH();
}

// out [S,OH,OW,C]: channel ch is written.  Per axis the final index o reads resampled index lo + clamp(o - before, 0, kept - 1).
int mmseg_preprocess_image(const float* img, const float* ws, float* out, int S, int H, int W, int RH, int RW, int OH, int OW, int lo_r,
                           int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int ch, void* stream) {
    if (S <= 0) return 0;
    if (!img || !ws || !out || !pp_geometry_ok(S, H, W, RH, RW) || OH < 1 || OW < 1 || (long)OH * OW >= 0x7fffffffL - PP_MAXBLK * PP_BLOCK ||
        C < 1 || ch < 0 || ch >= C || !pp_axis_ok(lo_r, kept_r, before_r, RH, OH) || !pp_axis_ok(lo_c, kept_c, before_c, RW, OW))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)pp_blocks((long)OH * OW), S);
    const pp_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    hipLaunchKernelGGL(pp_image_kernel, grid, dim3(PP_BLOCK), 0, (hipStream_t)stream, img, ws, pp_blocks((long)RH * RW), out, H, W,
                       (double)H / (double)RH, (double)W / (double)RW, OH, OW, ar, ac, C, ch);
    return MMSEG_CHECK_LAUNCH();
}

// lab [S,H,W] uint8 grey values, values [K] int32 (device), out [S,OH,OW,C]: channels ch0 .. ch0 + K - 1 are written
int mmseg_preprocess_label(const unsigned char* lab, const int* values, float* out, int S, int H, int W, int RH, int RW, int OH, int OW,
                           int lo_r, int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int ch0, int K, void* stream) {
    if (S <= 0) return 0;
    if (!lab || !values || !out || !pp_geometry_ok(S, H, W, RH, RW) || OH < 1 || OW < 1 || (long)OH * OW >= 0x7fffffffL - PP_MAXBLK * PP_BLOCK ||
        K < 1 || K > PP_MAXVALUES || C < 1 || ch0 < 0 || ch0 + K > C || !pp_axis_ok(lo_r, kept_r, before_r, RH, OH) ||
        !pp_axis_ok(lo_c, kept_c, before_c, RW, OW))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)pp_blocks((long)OH * OW), S);
    const pp_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    hipLaunchKernelGGL(pp_label_kernel, grid, dim3(PP_BLOCK), 0, (hipStream_t)stream, lab, values, K, out, H, W, (double)H / (double)RH,
                       (double)W / (double)RW, OH, OW, ar, ac, C, ch0);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"

// ---- percentile-window and landmark normalisation (build-defined; the definition is in include/mmseg_hip.h) -------------------------
// Instead of the (min, max) of a slice, K order statistics ("knots") of a segment -- one resampled slice, or all resampled slices of
// the volume -- and a clamped piecewise-linear map through them.  Selection is a radix select on the order-preserving 32-bit key of
// an fp32 value, most significant 8-bit digit first: pq_hist_kernel recomputes pp_bilinear over the resampled frame (the frame still
// never exists in memory: one read of the raw slices per pass, four passes, a fifth read by the map), counts per rank the digit of
// every value whose higher digits equal that rank's prefix in LDS histograms [K][256] and adds its non-empty bins to the segment's
// global histogram with integer atomics (order independent: bitwise reproducible); pq_pick_kernel, one block per segment, scans the
// K histograms, extends the K prefixes and reduces the K ranks.  After the fourth pass a prefix is the key of the selected value,
// an element of the population bit for bit, which pp_image_map_kernel meets again because it calls the same pp_bilinear.
// The grid stays (blocks, S) in both scopes: with one segment per volume the blocks of every slice add to segment 0, which fills the
// device better than 64 blocks for a whole volume would.  No block waits for another; every loop is bounded by the frame or by K.
#define PQ_MAXKNOTS 16
#define PQ_BINS 256
#define PQ_PASSES 4

// workspace of one call, in 32-bit words: per segment prefix [K] and remaining rank [K], then per pass and segment hist [K][256]
static long pq_state_words(int G, int K) { return 2L * G * K; }
static long pq_hist_words(int G, int K) { return (long)G * K * PQ_BINS; }

// monotone in the value: negative values have all bits flipped, the others get the sign bit (-0 sorts directly below +0)
__device__ __forceinline__ unsigned pq_key(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float pq_value(unsigned key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

// grid (nblk, S), block PP_BLOCK: hist[g][j][digit `pass` of key] += 1 for every resampled pixel of slice s whose higher digits equal
// prefix[g][j]; g = per_volume ? 0 : s.  state / hist: this call's, hist of this pass
__global__ void __launch_bounds__(PP_BLOCK) pq_hist_kernel(const float* __restrict__ img, const unsigned* __restrict__ state,
                                                           unsigned* __restrict__ hist, int K, int per_volume, int pass, int H, int W,
                                                           int RH, int RW, double ry, double rx) {
    __shared__ unsigned lh[PQ_MAXKNOTS][PQ_BINS];
    __shared__ unsigned pfx[PQ_MAXKNOTS];
    const int s = blockIdx.y, g = per_volume ? 0 : s;
    const int shift = 32 - 8 * (pass + 1);
    for (int j = 0; j < K; ++j) lh[j][threadIdx.x] = 0u;
    if (threadIdx.x < K) pfx[threadIdx.x] = pass ? state[(size_t)g * 2 * K + threadIdx.x] >> (shift + 8) : 0u;   // pass 0: all match
    __syncthreads();
    const float* src = img + (size_t)s * H * W;
    const int n = RH * RW;
    for (int e = blockIdx.x * PP_BLOCK + threadIdx.x; e < n; e += gridDim.x * PP_BLOCK) {
        const int dr = e / RW, dc = e - dr * RW;
        const unsigned key = pq_key(pp_bilinear(src, H, W, dr, dc, ry, rx));
        const unsigned d = (key >> shift) & (PQ_BINS - 1), hb = pass ? key >> (shift + 8) : 0u;
        for (int j = 0; j < K; ++j)
            if (hb == pfx[j]) atomicAdd(&lh[j][d], 1u);
    }
    __syncthreads();
    unsigned* gh = hist + (size_t)g * K * PQ_BINS;
    for (int j = 0; j < K; ++j) {
        const unsigned c = lh[j][threadIdx.x];
        if (c) atomicAdd(gh + j * PQ_BINS + threadIdx.x, c);
    }
}

// grid G, block PP_BLOCK: per rank j the bin of this pass's histogram that holds the (remaining) rank extends prefix[g][j] and the
// rank is reduced by the count below that bin.  Pass 0 starts from `ranks`; the last pass writes the knots x[g][j].
__global__ void __launch_bounds__(PP_BLOCK) pq_pick_kernel(unsigned* __restrict__ state, const unsigned* __restrict__ hist,
                                                           const int* __restrict__ ranks, float* __restrict__ x, int K, int pass) {
    __shared__ unsigned lh[PQ_MAXKNOTS][PQ_BINS];
    const int g = blockIdx.x;
    const unsigned* gh = hist + (size_t)g * K * PQ_BINS;
    for (int j = 0; j < K; ++j) lh[j][threadIdx.x] = gh[j * PQ_BINS + threadIdx.x];
    __syncthreads();
    if (threadIdx.x >= K) return;
    const int j = threadIdx.x;
    unsigned* prefix = state + (size_t)g * 2 * K;
    unsigned* rank = prefix + K;
    unsigned r = pass ? rank[j] : (unsigned)ranks[j];
    unsigned p = pass ? prefix[j] : 0u;
    unsigned below = 0u;
    for (int b = 0; b < PQ_BINS; ++b) {
        const unsigned c = lh[j][b];
        if (r < below + c) {          // true for exactly one b when 0 <= rank < N
            p |= (unsigned)b << (32 - 8 * (pass + 1));
            r -= below;
            break;
        }
        below += c;
    }
    prefix[j] = p;
    rank[j] = r;
    if (pass == PQ_PASSES - 1) x[(size_t)g * K + j] = pq_value(p);
}

// pp_image_kernel with the map through the knots in place of the rescale: xs [G][K] from pq_pick_kernel (row per_volume ? 0 : s),
// ys [K] the targets.  v <= x_0 -> y_0, v >= x_{K-1} -> y_{K-1}, else with the largest k that has x_k < v:
// min(y_k + (v - x_k) * ((y_{k+1} - y_k) / (x_{k+1} - x_k)), y_{k+1}); x_{k+1} >= v > x_k, so the denominator is positive
__global__ void __launch_bounds__(PP_BLOCK) pp_image_map_kernel(const float* __restrict__ img, const float* __restrict__ xs,
                                                                const float* __restrict__ ys, int K, int per_volume,
                                                                float* __restrict__ out, int H, int W, double ry, double rx, int OH,
                                                                int OW, pp_axis ar, pp_axis ac, int C, int ch) {
#pragma clang fp contract(off)
    __shared__ float kx[PQ_MAXKNOTS], ky[PQ_MAXKNOTS], slope[PQ_MAXKNOTS];
    const int s = blockIdx.y;
    if (threadIdx.x < K) {
        const float* row = xs + (size_t)(per_volume ? 0 : s) * K;
        kx[threadIdx.x] = row[threadIdx.x];
        ky[threadIdx.x] = ys[threadIdx.x];
        if (threadIdx.x < K - 1) {
            const float dx = row[threadIdx.x + 1] - row[threadIdx.x];
            slope[threadIdx.x] = dx > 0.f ? (ys[threadIdx.x + 1] - ys[threadIdx.x]) / dx : 0.f;          // equal knots: never selected
        }
    }
    __syncthreads();
    const float x0 = kx[0], xl = kx[K - 1], y0 = ky[0], yl = ky[K - 1];
    const float* src = img + (size_t)s * H * W;
    float* dst = out + (size_t)s * OH * OW * C + ch;
    const int n = OH * OW;
    for (int e = blockIdx.x * PP_BLOCK + threadIdx.x; e < n; e += gridDim.x * PP_BLOCK) {
        const int r = e / OW, c = e - r * OW;
        const int dr = ar.lo + min(max(r - ar.before, 0), ar.kept - 1);
        const int dc = ac.lo + min(max(c - ac.before, 0), ac.kept - 1);
        const float v = pp_bilinear(src, H, W, dr, dc, ry, rx);
        float o;
        if (v <= x0) o = y0;
        else if (v >= xl) o = yl;
        else {
            int k = K - 2;
            while (k > 0 && !(kx[k] < v)) --k;
            o = fminf(ky[k] + (v - kx[k]) * slope[k], ky[k + 1]);
        }
        dst[(size_t)e * C] = o;
    }
}

static bool pq_ok(int S, int RH, int RW, int K, int per_volume) {
    return K >= 2 && K <= PQ_MAXKNOTS && (per_volume ? (long)S : 1L) * RH * RW < 0x80000000L;
}

extern "C" {

// bytes of the state and the four histograms of one mmseg_preprocess_quantiles call
long mmseg_preprocess_quantiles_workspace_bytes(int S, int K, int per_volume) {
    if (S < 1 || K < 2 || K > PQ_MAXKNOTS) return 0;
    const int G = per_volume ? 1 : S;
    return 4L * (pq_state_words(G, K) + PQ_PASSES * pq_hist_words(G, K));
}

// img [S,H,W] raw slices, ranks [K] int32 (device), ws: mmseg_preprocess_quantiles_workspace_bytes(S, K, per_volume) bytes, zeroed
// here on the stream -> x [G,K]
int mmseg_preprocess_quantiles(const float* img, const int* ranks, int* ws, float* x, int S, int H, int W, int RH, int RW, int K,
                               int per_volume, void* stream) {
    if (S <= 0) return 0;
    if (!img || !ranks || !ws || !x || !pp_geometry_ok(S, H, W, RH, RW) || !pq_ok(S, RH, RW, K, per_volume)) return (int)hipErrorInvalidValue;
    const int G = per_volume ? 1 : S;
    const hipError_t zeroed = hipMemsetAsync(ws, 0, (size_t)mmseg_preprocess_quantiles_workspace_bytes(S, K, per_volume), (hipStream_t)stream);
    if (zeroed != hipSuccess) return (int)zeroed;
    unsigned* state = reinterpret_cast<unsigned*>(ws);
    unsigned* hist = state + pq_state_words(G, K);
    const dim3 grid((unsigned)pp_blocks((long)RH * RW), S);
    for (int pass = 0; pass < PQ_PASSES; ++pass, hist += pq_hist_words(G, K)) {
        hipLaunchKernelGGL(pq_hist_kernel, grid, dim3(PP_BLOCK), 0, (hipStream_t)stream, img, state, hist, K, per_volume ? 1 : 0, pass, H, W,
                           RH, RW, (double)H / (double)RH, (double)W / (double)RW);
        hipLaunchKernelGGL(pq_pick_kernel, dim3(G), dim3(PP_BLOCK), 0, (hipStream_t)stream, state, hist, ranks, x, K, pass);
    }
    return MMSEG_CHECK_LAUNCH();
}

// out [S,OH,OW,C]: channel ch is written, as by mmseg_preprocess_image; x [G,K] from mmseg_preprocess_quantiles, y [K] (device)
int mmseg_preprocess_image_map(const float* img, const float* x, const float* y, float* out, int S, int H, int W, int RH, int RW, int OH,
                               int OW, int lo_r, int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int ch, int K,
                               int per_volume, void* stream) {
    if (S <= 0) return 0;
    if (!img || !x || !y || !out || !pp_geometry_ok(S, H, W, RH, RW) || !pq_ok(S, RH, RW, K, per_volume) || OH < 1 || OW < 1 ||
        (long)OH * OW >= 0x7fffffffL - PP_MAXBLK * PP_BLOCK || C < 1 || ch < 0 || ch >= C || !pp_axis_ok(lo_r, kept_r, before_r, RH, OH) ||
        !pp_axis_ok(lo_c, kept_c, before_c, RW, OW))
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)pp_blocks((long)OH * OW), S);
    const pp_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    hipLaunchKernelGGL(pp_image_map_kernel, grid, dim3(PP_BLOCK), 0, (hipStream_t)stream, img, x, y, K, per_volume ? 1 : 0, out, H, W,
                       (double)H / (double)RH, (double)W / (double)RW, OH, OW, ar, ac, C, ch);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
