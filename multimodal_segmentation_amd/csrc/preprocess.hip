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

#define PP_BLOCK 256
#define PP_MAXBLK 64
#define PP_MAXVALUES 16

struct pp_axis {
    int lo, kept, before;
};

// source coordinate of resampled pixel d; `ratio` = in / out computed in fp64 by the launcher
__device__ __forceinline__ double pp_coord(int d, double ratio) {
#pragma clang fp contract(off)
    return ((double)d + 0.5) * ratio - 0.5;
}

// bilinear sample of one raw slice at resampled pixel (dr, dc); 0 outside (strict)
__device__ __forceinline__ float pp_bilinear(const float* __restrict__ s, int H, int W, int dr, int dc, double ry, double rx) {
#pragma clang fp contract(off)
    const double sy = pp_coord(dr, ry), sx = pp_coord(dc, rx);
    if (!(sy >= 0.0 && sy <= (double)(H - 1) && sx >= 0.0 && sx <= (double)(W - 1))) return 0.f;
    const double fyd = floor(sy), fxd = floor(sx);
    const float fy = (float)(sy - fyd), fx = (float)(sx - fxd);
    const int r0 = (int)fyd, c0 = (int)fxd;
    const int r1 = min(r0 + 1, H - 1), c1 = min(c0 + 1, W - 1);        // a tap beyond the edge carries weight 0
    const float a00 = s[(size_t)r0 * W + c0], a01 = s[(size_t)r0 * W + c1];
    const float a10 = s[(size_t)r1 * W + c0], a11 = s[(size_t)r1 * W + c1];
    const float top = (1.f - fx) * a00 + fx * a01;
    const float bot = (1.f - fx) * a10 + fx * a11;
    return (1.f - fy) * top + fy * bot;
}

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
