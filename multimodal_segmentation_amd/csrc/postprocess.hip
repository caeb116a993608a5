// Predicted label volumes on the device (gfx950): the way back from the network's frame to a volume's own grid, and the counts for a
// Dice measured there.  Build-defined (the reference writes no segmentation); the geometry is the inverse of preprocess.hip's.
//
// mmseg_restore_label: prob [S,OH,OW,C] (the segmentor's output, organ channels first) -> out [S,H,W] uint8 grey values.  Per axis,
// for raw index d:
//   coordinate  s = (d + 0.5) * (R / n) - 0.5 in fp64 without contraction (pp_coord with the ratio turned round), clamped into
//               [0, R - 1]: the edge rule of a resize to an exact size (the outermost raw pixels of an up-sampled volume fall just
//               outside otherwise).  R = the resampled extent, n = the raw one.
//   window      s outside [lo, lo + kept - 1] on either axis: the pixel was cropped away on the way in -> 0 (background).
//   container   index = s - lo + before.  s - lo is exact in fp64 (lo is an integer below s), so the fractional part is that of s.
//   order 1     every organ channel is sampled bilinearly, v = (1-fy)*((1-fx)*a00 + fx*a01) + fy*((1-fx)*a10 + fx*a11) in fp32 in that
//               order (pp_bilinear's); a tap past the window's last index carries weight 0.
//   order 0     the tap floor(s + 0.5), limited to the window.
//   0.5 rule    the pixel gets values[k] of the lowest k whose sampled probability is > 0.5 (what costs.dice(binarise=True) rounds to
//               1), else 0.  No arg-max: the only decision point is a probability at 0.5.
// Stores: consecutive lanes take consecutive raw columns.  Where W % 4 == 0 a lane owns 4 adjacent columns and stores one packed
// dword, a wave 256 contiguous bytes; otherwise one byte per lane.  Reads: the K organ channels of a tap are one 16-byte load when
// K == 4 and the pixel stride C is a multiple of 4 floats; scalar loads otherwise (a softmax with a background channel has C = 5).
// Traffic: the container is read about once (neighbouring raw pixels share taps through the caches), 1 byte per raw pixel is written.
//
// mmseg_label_overlap: pred, truth [S,n] uint8 -> counts [S,K,3] int32 = (|pred == v|, |truth == v|, |both|) per slice and organ.
// Per-thread counters, a wave reduction, one LDS pass across the block's waves, one integer atomicAdd per (block, counter).  Integer
// addition is order independent: two runs are bitwise equal.  The launcher zeroes `counts` on the stream before the kernel.
#include "common.hpp"

#define PO_BLOCK 256
#define PO_MAXBLK 256
#define PO_MAXVALUES 16

struct po_axis {
    int lo, kept, before;
};

// one axis of one raw pixel: container taps i0 <= i1, weight f of i1, inside the kept window or not
struct po_tap {
    int i0, i1;
    float f;
    bool in;
};

__device__ __forceinline__ po_tap po_axis_tap(int d, double ratio, int R, po_axis a, int order) {
#pragma clang fp contract(off)
    double s = ((double)d + 0.5) * ratio - 0.5;
    s = fmin(fmax(s, 0.0), (double)(R - 1));
    po_tap t;
    t.in = s >= (double)a.lo && s <= (double)(a.lo + a.kept - 1);
    t.i0 = t.i1 = a.before;
    t.f = 0.f;
    if (t.in) {
        if (order == 0) {
            const int n = min(max((int)floor(s + 0.5), a.lo), a.lo + a.kept - 1);
            t.i0 = t.i1 = n - a.lo + a.before;
        } else {
            const double w = s - (double)a.lo, fl = floor(w);
            const int i = (int)fl;
            t.f = (float)(w - fl);
            t.i0 = i + a.before;
            t.i1 = min(i + 1, a.kept - 1) + a.before;
        }
    }
    return t;
}

__device__ __forceinline__ float po_mix(float a00, float a01, float a10, float a11, float fy, float fx) {
#pragma clang fp contract(off)
    const float top = (1.f - fx) * a00 + fx * a01;
    const float bot = (1.f - fx) * a10 + fx * a11;
    return (1.f - fy) * top + fy * bot;
}

// grey value of one raw pixel; src = the slice's container [OH,OW,C]
template <bool VEC4>
__device__ __forceinline__ unsigned po_pixel(const float* __restrict__ src, int OW, int C, int K, const int* vals, po_tap ty, po_tap tx,
                                             int order) {
    if (!(ty.in && tx.in)) return 0u;
    const float* p00 = src + ((size_t)ty.i0 * OW + tx.i0) * C;
    if (order == 0) {
        if constexpr (VEC4) {
            const f32x4 a = *reinterpret_cast<const f32x4*>(p00);
            return a[0] > 0.5f ? vals[0] : a[1] > 0.5f ? vals[1] : a[2] > 0.5f ? vals[2] : a[3] > 0.5f ? vals[3] : 0;
        } else {
            for (int k = 0; k < K; ++k)
                if (p00[k] > 0.5f) return (unsigned)vals[k];
            return 0u;
        }
    }
    const float* p01 = src + ((size_t)ty.i0 * OW + tx.i1) * C;
    const float* p10 = src + ((size_t)ty.i1 * OW + tx.i0) * C;
    const float* p11 = src + ((size_t)ty.i1 * OW + tx.i1) * C;
    if constexpr (VEC4) {
        const f32x4 a00 = *reinterpret_cast<const f32x4*>(p00), a01 = *reinterpret_cast<const f32x4*>(p01);
        const f32x4 a10 = *reinterpret_cast<const f32x4*>(p10), a11 = *reinterpret_cast<const f32x4*>(p11);
        unsigned g = 0u;
#pragma unroll
        for (int k = 3; k >= 0; --k)          // descending, so that the lowest k above 0.5 is the one kept
            if (po_mix(a00[k], a01[k], a10[k], a11[k], ty.f, tx.f) > 0.5f) g = (unsigned)vals[k];
        return g;
    } else {
        for (int k = 0; k < K; ++k)
            if (po_mix(p00[k], p01[k], p10[k], p11[k], ty.f, tx.f) > 0.5f) return (unsigned)vals[k];
        return 0u;
    }
}

// grid (nblk, S), block PO_BLOCK.  PACK: a lane owns 4 adjacent columns (W % 4 == 0, out 4-byte aligned) and stores one dword.
template <bool VEC4, bool PACK>
__global__ void __launch_bounds__(PO_BLOCK) po_restore_kernel(const float* __restrict__ prob, const int* __restrict__ values, int K,
                                                              unsigned char* __restrict__ out, int H, int W, int RH, int RW, double ry,
                                                              double rx, int OH, int OW, po_axis ar, po_axis ac, int C, int order) {
    __shared__ int vals[PO_MAXVALUES];
    if (threadIdx.x < K) vals[threadIdx.x] = values[threadIdx.x] & 255;
    __syncthreads();
    const int s = blockIdx.y;
    const float* src = prob + (size_t)s * OH * OW * C;
    unsigned char* dst = out + (size_t)s * H * W;
    if constexpr (PACK) {
        const int W4 = W >> 2, n = H * W4;
        for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += gridDim.x * PO_BLOCK) {
            const int r = e / W4, c = (e - r * W4) << 2;
            const po_tap ty = po_axis_tap(r, ry, RH, ar, order);
            unsigned word = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                word |= po_pixel<VEC4>(src, OW, C, K, vals, ty, po_axis_tap(c + j, rx, RW, ac, order), order) << (8 * j);
            reinterpret_cast<unsigned*>(dst)[e] = word;          // byte j of the dword = column c + j (little endian)
        }
    } else {
        const int n = H * W;
        for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += gridDim.x * PO_BLOCK) {
            const int r = e / W, c = e - r * W;
            dst[e] = (unsigned char)po_pixel<VEC4>(src, OW, C, K, vals, po_axis_tap(r, ry, RH, ar, order),
                                                   po_axis_tap(c, rx, RW, ac, order), order);
        }
    }
}

// grid (nblk, S), block PO_BLOCK: counts[s][k] += (|pred == values[k]|, |truth == values[k]|, |both|) over this block's share of slice s
__global__ void __launch_bounds__(PO_BLOCK) po_overlap_kernel(const unsigned char* __restrict__ pred, const unsigned char* __restrict__ truth,
                                                              const int* __restrict__ values, int K, int* __restrict__ counts, int n) {
    __shared__ int vals[PO_MAXVALUES];
    __shared__ int red[PO_BLOCK / 64][PO_MAXVALUES * 3];
    if (threadIdx.x < PO_MAXVALUES) vals[threadIdx.x] = threadIdx.x < K ? values[threadIdx.x] : -1;      // -1 matches no byte
    __syncthreads();
    const int s = blockIdx.y;
    const unsigned char* p = pred + (size_t)s * n;
    const unsigned char* t = truth + (size_t)s * n;
    int cp[PO_MAXVALUES], ct[PO_MAXVALUES], cb[PO_MAXVALUES];
#pragma unroll
    for (int k = 0; k < PO_MAXVALUES; ++k) cp[k] = ct[k] = cb[k] = 0;
    for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += gridDim.x * PO_BLOCK) {
        const int pv = p[e], tv = t[e];
#pragma unroll
        for (int k = 0; k < PO_MAXVALUES; ++k) {
            const int a = pv == vals[k], b = tv == vals[k];
            cp[k] += a;
            ct[k] += b;
            cb[k] += a & b;
        }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int k = 0; k < PO_MAXVALUES; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cp[k] += __shfl_xor(cp[k], o, 64);
            ct[k] += __shfl_xor(ct[k], o, 64);
            cb[k] += __shfl_xor(cb[k], o, 64);
        }
        if (lane == 0) {
            red[wid][3 * k] = cp[k];
            red[wid][3 * k + 1] = ct[k];
            red[wid][3 * k + 2] = cb[k];
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * K) {
        int v = 0;
        for (int w = 0; w < PO_BLOCK / 64; ++w) v += red[w][threadIdx.x];
        if (v) atomicAdd(counts + (size_t)s * K * 3 + threadIdx.x, v);
    }
}

static int po_blocks(long n) {
    const long b = (n + PO_BLOCK - 1) / PO_BLOCK;
    return (int)(b < 1 ? 1 : (b < PO_MAXBLK ? b : PO_MAXBLK));
}

// as pp_axis_ok (0 <= lo, 1 <= kept, lo + kept <= R, 0 <= before < O), and the kept window must lie inside the container, which is
// what this direction reads: before + kept <= O
static bool po_axis_ok(int lo, int kept, int before, int R, int O) {
    return lo >= 0 && kept >= 1 && (long)lo + kept <= R && before >= 0 && before < O && (long)before + kept <= O;
}

static bool po_geometry_ok(int S, int H, int W, int RH, int RW, int OH, int OW) {
    const long lim = 0x7fffffffL - (long)PO_MAXBLK * PO_BLOCK;
    return S <= 65535 && H >= 1 && W >= 1 && RH >= 1 && RW >= 1 && OH >= 1 && OW >= 1 && (long)H * W < lim && (long)RH * RW < lim &&
           (long)OH * OW < lim;
}

template <bool VEC4, bool PACK>
static void po_launch(dim3 grid, hipStream_t stream, const float* prob, const int* values, int K, unsigned char* out, int H, int W, int RH,
                      int RW, int OH, int OW, po_axis ar, po_axis ac, int C, int order) {
    hipLaunchKernelGGL((po_restore_kernel<VEC4, PACK>), grid, dim3(PO_BLOCK), 0, stream, prob, values, K, out, H, W, RH, RW,
                       (double)RH / (double)H, (double)RW / (double)W, OH, OW, ar, ac, C, order);
}

extern "C" {

// prob [S,OH,OW,C] fp32, values [K] int32 (device, grey values 0..255), out [S,H,W] uint8: every byte is written
int mmseg_restore_label(const float* prob, const int* values, unsigned char* out, int S, int H, int W, int RH, int RW, int OH, int OW,
                        int lo_r, int kept_r, int before_r, int lo_c, int kept_c, int before_c, int C, int K, int order, void* stream) {
    if (S <= 0) return 0;
    if (!prob || !values || !out || !po_geometry_ok(S, H, W, RH, RW, OH, OW) || K < 1 || K > PO_MAXVALUES || C < 1 || K > C ||
        (order != 0 && order != 1) || !po_axis_ok(lo_r, kept_r, before_r, RH, OH) || !po_axis_ok(lo_c, kept_c, before_c, RW, OW))
        return (int)hipErrorInvalidValue;
    const bool pack = (W & 3) == 0 && ((uintptr_t)out & 3) == 0;
    const bool vec4 = K == 4 && (C & 3) == 0 && ((uintptr_t)prob & 15) == 0;
    const dim3 grid((unsigned)po_blocks(pack ? (long)H * (W >> 2) : (long)H * W), S);
    const po_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    const hipStream_t st = (hipStream_t)stream;
    if (vec4 && pack) po_launch<true, true>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    else if (vec4) po_launch<true, false>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    else if (pack) po_launch<false, true>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    else po_launch<false, false>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    return MMSEG_CHECK_LAUNCH();
}

// pred, truth [S,n] uint8 (n = H * W), values [K] int32 (device), counts [S,K,3] int32: zeroed here, on the stream, then accumulated
int mmseg_label_overlap(const unsigned char* pred, const unsigned char* truth, const int* values, int* counts, int S, int n, int K,
                        void* stream) {
    if (S <= 0) return 0;
    if (!pred || !truth || !values || !counts || S > 65535 || n < 1 || (long)n >= 0x7fffffffL - (long)PO_MAXBLK * PO_BLOCK || K < 1 ||
        K > PO_MAXVALUES)
        return (int)hipErrorInvalidValue;
    const hipError_t rc = hipMemsetAsync(counts, 0, sizeof(int) * 3 * (size_t)K * S, (hipStream_t)stream);
    if (rc != hipSuccess) return (int)rc;
    const dim3 grid((unsigned)po_blocks(n), S);
    hipLaunchKernelGGL(po_overlap_kernel, grid, dim3(PO_BLOCK), 0, (hipStream_t)stream, pred, truth, values, K, counts, n);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
