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
//
// Scores in mm on a volume's own grid (build-defined; definitions in INTEGRATION.md section 5).  K + 1 binary problems per label volume:
// problem k < K is "== values[k]", problem K "equals any of values".
// mmseg_label_surface: label [S,H,W] -> surf [K+1,S,H,W] 0 / 1: a foreground voxel with a background (or outside) face neighbour.  One
//   sweep: a lane reads its voxel and the six neighbours once and writes the K + 1 bytes; consecutive lanes, consecutive voxels.
//   Optionally counts [K+1][2] int32 = (|foreground|, |surface|) with integer atomics.
// Exact squared Euclidean distance to the nearest site, separable: three passes out[i] = min over ALL j of in[j] + (sp * (i - j))^2 in
//   fp64 (fma(d, d, in[j]), d = sp * (i - j) with i - j exact), along W, H, S.  The minimum over a fixed set of values is the same in any
//   order, so two runs are bitwise equal.  Pass along W (po_edt_row_kernel): a row per wave, lanes own outputs lane + 64 m, the row is
//   staged in LDS in tiles and every lane reads the same LDS address (a broadcast).  Passes along H and S (po_edt_col_kernel): the
//   volume is seen as [A, L, B] with B contiguous; a block owns 64 consecutive b and 64 outputs i, stages [64 j][64 b] tiles in LDS
//   (global reads and LDS reads: consecutive lanes, consecutive doubles), a thread keeps 16 consecutive i in registers.  The last
//   pass takes the square root.
// po_surface_walk (behind mmseg_surface_metrics and mmseg_surface_scores): per problem the two distance maps, each reduced over the
//   other side's surface: per-thread partial sums in grid-stride order, a fixed LDS tree per block, partials [blocks][2] = (sum, max),
//   and one block that adds the partials in a fixed tree: no floating-point atomics.  Only the [K+1,6] table is meant to leave the device.
//
// Order statistics of the surface distances (build-defined; HD(q) and NSD(tau) in INTEGRATION.md section 5).
// mmseg_masked_select: the multiset {a[e] : ma[e] != 0} + {b[e] : mb[e] != 0} of finite fp64 values >= 0 -> out [5] = N, |{x <= tolerance}|,
//   the percentile by numpy's linear rule, and the two order statistics D_(lo), D_(hi) it is interpolated from.  os_append_kernel
//   compacts the selected values into a list (one integer atomicAdd per wave on the list's counter), then eight passes of
//   os_hist_kernel (per-block LDS histograms of one 8-bit digit of the bit patterns, most significant first, one global integer atomic
//   per non-empty bin) and os_pick_kernel (one block: scan, pick the digit, narrow the prefix) follow both ranks at once.  Exact and,
//   integer counts being order independent, bitwise reproducible.  Nothing reaches the host: N and the ranks are computed on the device.
// mmseg_surface_scores: the same walk, told to append every distance map's surface values to the problem's list before the map is
//   overwritten -> table [K+1,8]: the six columns of mmseg_surface_metrics (same launches), |{x <= tolerance}|, HD(percentile).
//
// The largest connected component of every organ (build-defined; the rule is in INTEGRATION.md section 5).
// mmseg_label_components: label [S,H,W] -> comp [S,H,W] int32 = 1 + the smallest linear index of the voxel's component, 0 for a voxel
//   that is no organ's; all K organs in one pass (a union-find in comp itself, see the kernels).
// mmseg_keep_largest_components: the components, their sizes (integer atomics on the root's slot), per organ one 64-bit atomicMax on
//   (size << 32) | (0xffffffff - root), and a pass that zeroes the organ voxels outside their organ's winner.
//
// Enclosed holes of every organ (build-defined; the rule is in INTEGRATION.md section 5).
// mmseg_fill_label_holes: per organ k, in order on the stream, the same union-find over the COMPLEMENT of the organ ("!= values[k]", faces
//   only, in 3-D or slice by slice), a mark on the root of every set that holds a border voxel (an idempotent byte store), and a pass
//   that gives the input's zeros in unmarked sets to the organ where `out` still holds 0: the lowest k wins.
//
// Opening, closing and smoothing of every organ by a ball in mm (build-defined; the rule is in INTEGRATION.md section 5 and the header).
// mmseg_smooth_label: a windowed kernel pair, not po_edt: the cost follows the reach of the ball, not the extent of the volume.  One
//   block writes the row table of the ball (per (|oz|, |oy|) the largest ox inside it, from t(o) in the order of po_edt's passes); then,
//   per organ and erosion or dilation, po_mo_run_kernel maps every voxel to the distance along x to the nearest site of its row (a byte,
//   capped at the reach) and po_mo_ball_kernel asks, per row of the ball inside the volume, whether that byte is within the row's reach:
//   (2 rz + 1)(2 ry + 1) bytes per voxel at most, read by consecutive lanes from consecutive addresses, with an early exit, and only for
//   the voxels whose answer is open.  "min over sites of the separable squared distance <= r^2" and "a site at an offset in the ball" are
//   the same statement bit for bit, fma(b, b, v) being monotone in v.  An axis of reach 0 adds nothing: no run map along x, one row
//   along y or z.  Erosion never looks outside the volume, so the volume's faces erode nothing.
//
// Frames larger than the network's input (build-defined; the rule is in INTEGRATION.md section 5).
// mmseg_blend_tiles: prob [TR*TC,S,OH,OW,C], the segmentor's output for every tile of a TR x TC plan -> out [S,RH,RW,K], the weighted mean of
//   the covering tiles at every pixel of the resampled frame, weights wr[tr][iy] * wc[tc][ix].  A gather: every output element is
//   written by one thread, the covering tiles are visited in ascending (tr, tc) order, so two runs are bitwise equal; a pixel that one
//   tile covers is copied.  mmseg_restore_label then takes the whole frame as its window.
//
// Views of a slice, merged (test-time augmentation; build-defined; the rule is in INTEGRATION.md section 5).
// mmseg_merge_views: prob [V*N,OH,OW,C], the segmentor's output for V views of N slices, view-major -> out [N,OH,OW,K], at every pixel the
//   mean over the views that cover it of the view's map sampled bilinearly at back[v] (r, c), an fp64 2 x 3 matrix per view.  A gather
//   like the blend: one thread per output element, the views in ascending order, two runs bitwise equal; a pixel that one view covers
//   is that view's sample, and an integer coordinate (every flip and right-angle turn) is a tap, copied.
//
// Several models and views, their mean, its uncertainty and its calibration (build-defined; the rule is in INTEGRATION.md section 5 and the
// header).
// mmseg_members_accumulate: the merge with state: one model's V views of N slices are added, per pixel, into sum [N,OH,OW,K] and aux
//   [N,OH,OW,2] = (sum of the views' entropies over the K organs and the rest, their number), so that any number of models stream through
//   one pair of buffers.  mmseg_members_finish, in place: the mean (merge_views's rule, so one model's mean is its merged map bit for bit),
//   H = the entropy of the mean and I = H - the mean entropy of the members (mutual information), as shares of ln(K + 1).  A thread owns
//   a pixel on both paths: the entropy needs a pixel's channels in one place and in one order.
// mmseg_restore_map: mmseg_restore_label's geometry and taps with a grey level in place of the 0.5 rule: one plane of [S,OH,OW,U] -> uint8.
// mmseg_calibration_table: per organ and confidence bin the pixel counts (integer atomics) and the fp64 sums a reliability diagram, ECE,
//   Brier score and NLL are made of; tiles of 256 pixels staged in LDS, every table entry summed by the one thread that owns it, in a
//   fixed order, then over the blocks in a fixed order: no floating-point atomics, two runs bitwise equal.
// mmseg_uncertainty_by_error: counts and level sums of the uncertainty planes over the correctly and the wrongly labelled pixels; integers.
#include "common.hpp"
#include <math.h>

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

// ---- tiles of a frame larger than the network's input, blended back into one probability map ------------------------------------------
#define BT_MAXTILES 8          // per axis

// VEC4: a thread owns one frame pixel, K == 4 channels as one 16-byte load per tile and one 16-byte store (C % 4 == 0, both pointers
// 16-byte aligned).  Otherwise a thread owns one output float (pixel, k): consecutive lanes store consecutive floats and the lanes of a
// pixel read consecutive channels of the same tile pixel.  Grid-stride over n = S * RH * RW [* K] elements, n < 2^29.
// The sums run over the covering tiles in ascending (tr, tc) order, starting from 0, in fp32 without contraction.  A tile covers a
// frame index y when lo <= y < lo + kept AND its container index y - lo + before lies inside [0, O): the tables come from the device,
// so the second condition is what keeps every read inside `prob`.
template <bool VEC4>
__global__ void __launch_bounds__(PO_BLOCK) po_blend_kernel(const float* __restrict__ prob, const int* __restrict__ rows,
                                                            const int* __restrict__ cols, const float* __restrict__ wr,
                                                            const float* __restrict__ wc, float* __restrict__ out, int S, int TR, int TC,
                                                            int OH, int OW, int C, int K, int RH, int RW, int n) {
#pragma clang fp contract(off)
    __shared__ int ar[BT_MAXTILES * 3], ac[BT_MAXTILES * 3];
    if (threadIdx.x < TR * 3) ar[threadIdx.x] = rows[threadIdx.x];
    if (threadIdx.x >= 32 && threadIdx.x < 32 + TC * 3) ac[threadIdx.x - 32] = cols[threadIdx.x - 32];
    __syncthreads();
    const int plane = RH * RW;
    for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += gridDim.x * PO_BLOCK) {
        const int pix = VEC4 ? e : e / K, k = VEC4 ? 0 : e - pix * K;
        const int s = pix / plane, r = pix - s * plane;
        const int y = r / RW, x = r - y * RW;
        int cnt = 0;
        float den = 0.f;
        f32x4 num4 = {0.f, 0.f, 0.f, 0.f}, first4 = {0.f, 0.f, 0.f, 0.f};
        float num = 0.f, first = 0.f;
        for (int tr = 0; tr < TR; ++tr) {
            const int iy = y - ar[3 * tr] + ar[3 * tr + 2];
            if (y < ar[3 * tr] || y >= ar[3 * tr] + ar[3 * tr + 1] || iy < 0 || iy >= OH) continue;
            const float wy = wr[tr * OH + iy];
            for (int tc = 0; tc < TC; ++tc) {
                const int ix = x - ac[3 * tc] + ac[3 * tc + 2];
                if (x < ac[3 * tc] || x >= ac[3 * tc] + ac[3 * tc + 1] || ix < 0 || ix >= OW) continue;
                const float w = wy * wc[tc * OW + ix];
                const float* p = prob + ((((size_t)(tr * TC + tc) * S + s) * OH + iy) * OW + ix) * C;
                if constexpr (VEC4) {
                    const f32x4 v = *reinterpret_cast<const f32x4*>(p);
                    if (cnt == 0) first4 = v;
                    num4 = num4 + w * v;
                } else {
                    const float v = p[k];
                    if (cnt == 0) first = v;
                    num = num + w * v;
                }
                den = den + w;
                ++cnt;
            }
        }
        // one covering tile: its value as it is (no multiply, no divide); none: 0
        if constexpr (VEC4) reinterpret_cast<f32x4*>(out)[e] = cnt == 1 ? first4 : cnt == 0 ? num4 : num4 / den;
        else out[e] = cnt == 1 ? first : cnt == 0 ? 0.f : num / den;
    }
}

// ---- views of one slice (test-time augmentation), brought back and averaged -----------------------------------------------------------------
#define MV_MAXVIEWS 16

// one axis of one view's coordinate: taps i0 <= i1 inside [0, n), weight f of i1.  Only called for 0 <= s <= n - 1.
__device__ __forceinline__ void mv_axis(double s, int n, int& i0, int& i1, float& f) {
    const double fl = floor(s);
    i0 = (int)fl;
    i1 = min(i0 + 1, n - 1);
    f = (float)(s - fl);
}

// augment_gather_kernel's order: a zero fraction skips its taps, so an integer coordinate returns the tap bit for bit; otherwise po_mix's
// expression.  T = float (channel k of a pixel) or f32x4 (its four channels).
template <typename T>
__device__ __forceinline__ T mv_sample(const float* __restrict__ src, int OW, int C, int r0, int r1, int c0, int c1, float fy, float fx) {
#pragma clang fp contract(off)
    const T a00 = *reinterpret_cast<const T*>(src + ((size_t)r0 * OW + c0) * C);
    T top = a00;
    if (fx != 0.f) top = (1.f - fx) * a00 + fx * *reinterpret_cast<const T*>(src + ((size_t)r0 * OW + c1) * C);
    if (fy == 0.f) return top;
    const T a10 = *reinterpret_cast<const T*>(src + ((size_t)r1 * OW + c0) * C);
    T bot = a10;
    if (fx != 0.f) bot = (1.f - fx) * a10 + fx * *reinterpret_cast<const T*>(src + ((size_t)r1 * OW + c1) * C);
    return (1.f - fy) * top + fy * bot;
}

// VEC4: a thread owns one pixel of the merged map, K == 4 channels as one 16-byte load per tap and one 16-byte store (C % 4 == 0, both
// pointers 16-byte aligned).  Otherwise a thread owns one output float (pixel, k): consecutive lanes store consecutive floats and the
// lanes of a pixel read consecutive channels of the same taps.  Grid-stride over total = N * OH * OW [* K] elements; N * OH * OW < 2^29,
// so a pixel index fits an int, and `small` (total < 2^31, a launch constant) keeps the scalar path's division by K in 32 bits.
// The sum runs over the covering views in ascending order, starting from 0, in fp32 without contraction.  A view covers the pixel iff
// its fp64 coordinate lies inside [0, OH-1] x [0, OW-1] (a NaN fails every comparison), which also keeps every read inside `prob`.
// A flip or a half turn reads rows backwards (whole cache lines all the same); a transposing view reads with a stride of one container
// row between neighbouring lanes, out of L2, which holds a slice's container.
template <bool VEC4>
__global__ void __launch_bounds__(PO_BLOCK) po_merge_kernel(const float* __restrict__ prob, const double* __restrict__ back,
                                                            float* __restrict__ out, int V, int N, int OH, int OW, int C, int K, long total,
                                                            bool small) {
#pragma clang fp contract(off)
    __shared__ double mb[MV_MAXVIEWS * 6];
    if (threadIdx.x < V * 6) mb[threadIdx.x] = back[threadIdx.x];
    __syncthreads();
    const int plane = OH * OW;
    const double hr = (double)(OH - 1), hc = (double)(OW - 1);
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < total; e += (long)gridDim.x * PO_BLOCK) {
        const int pix = VEC4 ? (int)e : small ? (int)((unsigned)e / (unsigned)K) : (int)(e / K);
        const int k = VEC4 ? 0 : (int)(e - (long)pix * K);
        const int s = pix / plane, q = pix - s * plane;
        const int r = q / OW, c = q - r * OW;
        int cnt = 0;
        f32x4 num4 = {0.f, 0.f, 0.f, 0.f}, first4 = {0.f, 0.f, 0.f, 0.f};
        float num = 0.f, first = 0.f;
        for (int v = 0; v < V; ++v) {
            const double* b = mb + 6 * v;
            const double sr = (b[0] * r + b[1] * c) + b[2], sc = (b[3] * r + b[4] * c) + b[5];
            if (!(sr >= 0.0 && sr <= hr && sc >= 0.0 && sc <= hc)) continue;
            int r0, r1, c0, c1;
            float fy, fx;
            mv_axis(sr, OH, r0, r1, fy);
            mv_axis(sc, OW, c0, c1, fx);
            const float* src = prob + ((size_t)v * N + s) * plane * C;
            if constexpr (VEC4) {
                const f32x4 x = mv_sample<f32x4>(src, OW, C, r0, r1, c0, c1, fy, fx);
                if (cnt == 0) first4 = x;
                num4 = num4 + x;
            } else {
                const float x = mv_sample<float>(src + k, OW, C, r0, r1, c0, c1, fy, fx);
                if (cnt == 0) first = x;
                num = num + x;
            }
            ++cnt;
        }
        // one covering view: its sample as it is (no add, no divide); none: 0
        if constexpr (VEC4) reinterpret_cast<f32x4*>(out)[e] = cnt == 1 ? first4 : cnt == 0 ? num4 : num4 / (float)cnt;
        else out[e] = cnt == 1 ? first : cnt == 0 ? 0.f : num / (float)cnt;
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

// ---- several models and views of a slice: the mean map, its entropy and the members' disagreement -------------------------------------------
// t(x) = -x ln x, 0 for x <= 0 (and for a NaN)
__device__ __forceinline__ float po_xlogx(float x) {
#pragma clang fp contract(off)
    return x > 0.f ? -x * logf(x) : 0.f;
}

// the entropy, in nats, of the K organ probabilities q and of rest = max(0, 1 - (((q0 + q1) + ..) + q[K-1])): the terms added from 0 in
// ascending k, the rest last.  One body for the accumulation and for the finish, so that the entropy of a single member's map and the
// entropy of its mean are the same instructions on the same bits.  Inlined into fully unrolled callers: q stays in registers.
__device__ __forceinline__ float po_entropy(const float (&q)[PO_MAXVALUES], int K) {
#pragma clang fp contract(off)
    float total = q[0], h = 0.f;
#pragma unroll
    for (int k = 0; k < PO_MAXVALUES; ++k)
        if (k < K) {
            if (k > 0) total = total + q[k];
            h = h + po_xlogx(q[k]);
        }
    return h + po_xlogx(fmaxf(0.f, 1.f - total));
}

// Both paths: a thread owns one PIXEL (the entropy needs all of a pixel's channels in one place, in a fixed order of addition).  VEC4: K == 4,
// C % 4 == 0, prob and sum 16-byte aligned: one 16-byte load per tap, one 16-byte load and store of the sums.  Otherwise K scalar loads per
// tap at a stride of C floats between neighbouring lanes (a wave still reads whole cache lines: its 64 pixels are contiguous) and K scalar
// stores at a stride of K floats.  The K accumulators and the K samples of a view live in registers: every loop over k is unrolled to
// PO_MAXVALUES with `k < K` as a uniform branch.  Grid-stride over the N * OH * OW < 2^29 pixels.  Coverage and sample: po_merge_kernel's.
template <bool VEC4>
__global__ void __launch_bounds__(PO_BLOCK) po_members_kernel(const float* __restrict__ prob, const double* __restrict__ back,
                                                              float* __restrict__ sum, float* __restrict__ aux, int first, int V, int N,
                                                              int OH, int OW, int C, int K, int pixels) {
#pragma clang fp contract(off)
    __shared__ double mb[MV_MAXVIEWS * 6];
    if (threadIdx.x < V * 6) mb[threadIdx.x] = back[threadIdx.x];
    __syncthreads();
    const int plane = OH * OW;
    const double hr = (double)(OH - 1), hc = (double)(OW - 1);
    for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < pixels; e += gridDim.x * PO_BLOCK) {
        const int s = e / plane, p = e - s * plane;
        const int r = p / OW, c = p - r * OW;
        float acc[PO_MAXVALUES], q[PO_MAXVALUES];
#pragma unroll
        for (int k = 0; k < PO_MAXVALUES; ++k) acc[k] = q[k] = 0.f;
        float sh = 0.f, cnt = 0.f;
        if (!first) {
            if constexpr (VEC4) {
                const f32x4 a = reinterpret_cast<const f32x4*>(sum)[e];
                acc[0] = a[0], acc[1] = a[1], acc[2] = a[2], acc[3] = a[3];
            } else {
#pragma unroll
                for (int k = 0; k < PO_MAXVALUES; ++k)
                    if (k < K) acc[k] = sum[(size_t)e * K + k];
            }
            sh = aux[2 * (size_t)e];
            cnt = aux[2 * (size_t)e + 1];
        }
        for (int v = 0; v < V; ++v) {
            const double* b = mb + 6 * v;
            const double sr = (b[0] * r + b[1] * c) + b[2], sc = (b[3] * r + b[4] * c) + b[5];
            if (!(sr >= 0.0 && sr <= hr && sc >= 0.0 && sc <= hc)) continue;
            int r0, r1, c0, c1;
            float fy, fx;
            mv_axis(sr, OH, r0, r1, fy);
            mv_axis(sc, OW, c0, c1, fx);
            const float* src = prob + ((size_t)v * N + s) * plane * C;
            if constexpr (VEC4) {
                const f32x4 x = mv_sample<f32x4>(src, OW, C, r0, r1, c0, c1, fy, fx);
                q[0] = x[0], q[1] = x[1], q[2] = x[2], q[3] = x[3];
            } else {
#pragma unroll
                for (int k = 0; k < PO_MAXVALUES; ++k)
                    if (k < K) q[k] = mv_sample<float>(src + k, OW, C, r0, r1, c0, c1, fy, fx);
            }
#pragma unroll
            for (int k = 0; k < PO_MAXVALUES; ++k)
                if (k < (VEC4 ? 4 : K)) acc[k] = acc[k] + q[k];
            sh = sh + po_entropy(q, VEC4 ? 4 : K);
            cnt = cnt + 1.f;
        }
        if constexpr (VEC4) {
            reinterpret_cast<f32x4*>(sum)[e] = f32x4{acc[0], acc[1], acc[2], acc[3]};
        } else {
#pragma unroll
            for (int k = 0; k < PO_MAXVALUES; ++k)
                if (k < K) sum[(size_t)e * K + k] = acc[k];
        }
        aux[2 * (size_t)e] = sh;
        aux[2 * (size_t)e + 1] = cnt;
    }
}

// in place: sum -> the mean map, aux (sum of the members' entropies, their number) -> (H, I); inv = (float)(1 / ln(K + 1))
template <bool VEC4>
__global__ void __launch_bounds__(PO_BLOCK) po_members_finish_kernel(float* __restrict__ sum, float* __restrict__ aux, int K, float inv,
                                                                     int pixels) {
#pragma clang fp contract(off)
    for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < pixels; e += gridDim.x * PO_BLOCK) {
        float q[PO_MAXVALUES];
#pragma unroll
        for (int k = 0; k < PO_MAXVALUES; ++k) q[k] = 0.f;
        const float sh = aux[2 * (size_t)e], cnt = aux[2 * (size_t)e + 1];
        if constexpr (VEC4) {
            const f32x4 a = reinterpret_cast<const f32x4*>(sum)[e];
            q[0] = a[0], q[1] = a[1], q[2] = a[2], q[3] = a[3];
        } else {
#pragma unroll
            for (int k = 0; k < PO_MAXVALUES; ++k)
                if (k < K) q[k] = sum[(size_t)e * K + k];
        }
#pragma unroll
        for (int k = 0; k < PO_MAXVALUES; ++k)
            if (k < (VEC4 ? 4 : K)) q[k] = cnt == 1.f ? q[k] : cnt == 0.f ? 0.f : q[k] / cnt;
        const float raw = po_entropy(q, VEC4 ? 4 : K);
        const float mean = cnt == 1.f ? sh : sh / cnt;
        const bool none = cnt == 0.f;
        if constexpr (VEC4) {
            reinterpret_cast<f32x4*>(sum)[e] = f32x4{q[0], q[1], q[2], q[3]};
        } else {
#pragma unroll
            for (int k = 0; k < PO_MAXVALUES; ++k)
                if (k < K) sum[(size_t)e * K + k] = q[k];
        }
        aux[2 * (size_t)e] = none ? 0.f : fminf(1.f, raw * inv);
        aux[2 * (size_t)e + 1] = none ? 0.f : fmaxf(0.f, raw - mean) * inv;
    }
}

// plane u of one raw pixel of a [OH,OW,U] fp32 container as a grey level: 0 outside the window, else the sample (restore_label's taps and
// po_mix) limited to [0, 1], times 255, rounded half up
__device__ __forceinline__ unsigned po_level(const float* __restrict__ src, int OW, int U, int u, po_tap ty, po_tap tx, int order) {
#pragma clang fp contract(off)
    if (!(ty.in && tx.in)) return 0u;
    float v = src[((size_t)ty.i0 * OW + tx.i0) * U + u];
    if (order != 0)
        v = po_mix(v, src[((size_t)ty.i0 * OW + tx.i1) * U + u], src[((size_t)ty.i1 * OW + tx.i0) * U + u],
                   src[((size_t)ty.i1 * OW + tx.i1) * U + u], ty.f, tx.f);
    return (unsigned)(unsigned char)(fminf(fmaxf(v, 0.f), 1.f) * 255.f + 0.5f);
}

// grid (nblk, S), block PO_BLOCK, as po_restore_kernel.  PACK: a lane owns 4 adjacent columns (W % 4 == 0, out 4-byte aligned), one dword.
template <bool PACK>
__global__ void __launch_bounds__(PO_BLOCK) po_restore_map_kernel(const float* __restrict__ planes, unsigned char* __restrict__ out, int H,
                                                                  int W, int RH, int RW, double ry, double rx, int OH, int OW, po_axis ar,
                                                                  po_axis ac, int U, int u, int order) {
    const int s = blockIdx.y;
    const float* src = planes + (size_t)s * OH * OW * U;
    unsigned char* dst = out + (size_t)s * H * W;
    if constexpr (PACK) {
        const int W4 = W >> 2, n = H * W4;
        for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += gridDim.x * PO_BLOCK) {
            const int r = e / W4, c = (e - r * W4) << 2;
            const po_tap ty = po_axis_tap(r, ry, RH, ar, order);
            unsigned word = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) word |= po_level(src, OW, U, u, ty, po_axis_tap(c + j, rx, RW, ac, order), order) << (8 * j);
            reinterpret_cast<unsigned*>(dst)[e] = word;
        }
    } else {
        const int n = H * W;
        for (int e = blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += gridDim.x * PO_BLOCK) {
            const int r = e / W, c = e - r * W;
            dst[e] = (unsigned char)po_level(src, OW, U, u, po_axis_tap(r, ry, RH, ar, order), po_axis_tap(c, rx, RW, ac, order), order);
        }
    }
}

// ---- the reliability table of a probability map against a label volume ----------------------------------------------------------------------------
#define CT_MAXBINS 64
#define CT_MAXBLK 1024         // blocks, and so partial tables that po_calibration_final_kernel adds
#define CT_SKIP 255            // code of a pixel outside the window; otherwise bin | (y << 7), bin < 64
#define CT_MAXOWN ((PO_MAXVALUES * (CT_MAXBINS + 2) + PO_BLOCK - 1) / PO_BLOCK)          // entries of the table per thread

// A block takes tiles of PO_BLOCK consecutive raw pixels of [S,H,W] in grid-stride order.  Per tile every thread samples the K organ
// channels of its pixel (restore_label's taps and po_mix) and stages p, the nll term and a code (bin, y, or CT_SKIP) in LDS; then thread
// t OWNS the entries t, t + PO_BLOCK, .. of the [K][B+2] table and walks the tile's PO_BLOCK staged pixels in ascending order, adding
// the ones of its organ (and bin).  So every entry is a sum in one fixed order (tiles ascending, pixels ascending), in fp64, whatever the
// scheduling: no floating-point atomics.  The owners of bin entries count (n, positives) on the way and add them to `bins` with one
// integer atomic each at the end.  part [gridDim.x][K * (B + 2)].  LDS: K * PO_BLOCK * 9 bytes, dynamic.
__global__ void __launch_bounds__(PO_BLOCK) po_calibration_kernel(const float* __restrict__ prob, const unsigned char* __restrict__ truth,
                                                                  const int* __restrict__ values, int* __restrict__ bins,
                                                                  double* __restrict__ part, long n, int H, int W, int RH, int RW, double ry,
                                                                  double rx, int OH, int OW, po_axis ar, po_axis ac, int C, int K, int B,
                                                                  int order) {
#pragma clang fp contract(off)
    extern __shared__ float ct_lds[];
    float* sp = ct_lds;                                                       // [K][PO_BLOCK]
    float* sl = ct_lds + (size_t)K * PO_BLOCK;                                // [K][PO_BLOCK]
    unsigned char* sc = reinterpret_cast<unsigned char*>(sl + (size_t)K * PO_BLOCK);          // [K][PO_BLOCK]
    __shared__ int vals[PO_MAXVALUES];
    if (threadIdx.x < K) vals[threadIdx.x] = values[threadIdx.x];
    const int entries = K * (B + 2), plane = H * W;
    double acc[CT_MAXOWN];
    int cn[CT_MAXOWN], cy[CT_MAXOWN];
#pragma unroll
    for (int j = 0; j < CT_MAXOWN; ++j) acc[j] = 0.0, cn[j] = cy[j] = 0;
    __syncthreads();
    for (long base = (long)blockIdx.x * PO_BLOCK; base < n; base += (long)gridDim.x * PO_BLOCK) {
        const long e = base + threadIdx.x;
        bool in = false;
        po_tap ty, tx;
        const float* src = prob;
        int tv = 0;
        if (e < n) {
            const int s = (int)(e / plane), p = (int)(e - (long)s * plane);
            const int r = p / W, c = p - r * W;
            ty = po_axis_tap(r, ry, RH, ar, order);
            tx = po_axis_tap(c, rx, RW, ac, order);
            in = ty.in && tx.in;
            src = prob + (size_t)s * OH * OW * C;
            tv = truth[e];
        }
        for (int k = 0; k < K; ++k) {
            unsigned char code = CT_SKIP;
            float p = 0.f, nll = 0.f;
            if (in) {
                p = src[((size_t)ty.i0 * OW + tx.i0) * C + k];
                if (order != 0)
                    p = po_mix(p, src[((size_t)ty.i0 * OW + tx.i1) * C + k], src[((size_t)ty.i1 * OW + tx.i0) * C + k],
                               src[((size_t)ty.i1 * OW + tx.i1) * C + k], ty.f, tx.f);
                const bool y = tv == vals[k];
                const int b = min(B - 1, max(0, (int)(p * (float)B)));          // the lower limit only matters for a p outside [0, 1]
                nll = -logf(fmaxf(y ? p : 1.f - p, 1e-6f));
                code = (unsigned char)(b | (y ? 128 : 0));
            }
            sp[k * PO_BLOCK + threadIdx.x] = p;
            sl[k * PO_BLOCK + threadIdx.x] = nll;
            sc[k * PO_BLOCK + threadIdx.x] = code;
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < CT_MAXOWN; ++j) {
            const int entry = j * PO_BLOCK + threadIdx.x;
            if (entry < entries) {
                const int k = entry / (B + 2), b = entry - k * (B + 2);
                const float* pk = sp + k * PO_BLOCK;
                const float* lk = sl + k * PO_BLOCK;
                const unsigned char* ck = sc + k * PO_BLOCK;
                if (b < B) {
                    for (int i = 0; i < PO_BLOCK; ++i) {
                        const int code = ck[i];
                        if ((code & 127) == b && code != CT_SKIP) {
                            acc[j] += (double)pk[i];
                            cn[j] += 1;
                            cy[j] += code >> 7;
                        }
                    }
                } else if (b == B) {
                    for (int i = 0; i < PO_BLOCK; ++i) {
                        const int code = ck[i];
                        if (code != CT_SKIP) {
                            const double d = (double)pk[i] - (double)(code >> 7);
                            acc[j] += d * d;
                        }
                    }
                } else {
                    for (int i = 0; i < PO_BLOCK; ++i)
                        if (ck[i] != CT_SKIP) acc[j] += (double)lk[i];
                }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int j = 0; j < CT_MAXOWN; ++j) {
        const int entry = j * PO_BLOCK + threadIdx.x;
        if (entry < entries) {
            part[(size_t)blockIdx.x * entries + entry] = acc[j];
            const int k = entry / (B + 2), b = entry - k * (B + 2);
            if (b < B && cn[j]) {
                atomicAdd(bins + ((size_t)k * B + b) * 2, cn[j]);
                if (cy[j]) atomicAdd(bins + ((size_t)k * B + b) * 2 + 1, cy[j]);
            }
        }
    }
}

// sums [entries] = the partial tables added in ascending block order, one thread per entry
__global__ void __launch_bounds__(PO_BLOCK) po_calibration_final_kernel(const double* __restrict__ part, int nblk, int entries,
                                                                        double* __restrict__ sums) {
    const int entry = blockIdx.x * PO_BLOCK + threadIdx.x;
    if (entry >= entries) return;
    double s = 0.0;
    for (int b = 0; b < nblk; ++b) s += part[(size_t)b * entries + entry];
    sums[entry] = s;
}

// ---- the levels of the uncertainty planes over the correctly and the wrongly labelled pixels -----------------------------------------------------
#define UE_MAXPLANES 4

// out [2][1 + U] += (count, sum of levels per plane) of this block's grid-stride share, row = pred != truth.  A thread visits at most
// 2^31 / (PO_MAXBLK * PO_BLOCK) = 2^15 pixels, so its 32-bit sums stay below 2^23; the block's sums are 64-bit.
__global__ void __launch_bounds__(PO_BLOCK) po_uncertainty_error_kernel(const unsigned char* __restrict__ pred,
                                                                        const unsigned char* __restrict__ truth,
                                                                        const unsigned char* __restrict__ levels,
                                                                        unsigned long long* __restrict__ out, long n, int U) {
    __shared__ unsigned red[PO_BLOCK / 64][2 * (1 + UE_MAXPLANES)];
    unsigned c[2 * (1 + UE_MAXPLANES)];
#pragma unroll
    for (int j = 0; j < 2 * (1 + UE_MAXPLANES); ++j) c[j] = 0u;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const unsigned wrong = pred[e] != truth[e];
        c[0] += 1u - wrong;
        c[1 + UE_MAXPLANES] += wrong;
#pragma unroll
        for (int u = 0; u < UE_MAXPLANES; ++u)
            if (u < U) {
                const unsigned l = levels[(size_t)u * n + e];
                c[1 + u] += wrong ? 0u : l;
                c[2 + UE_MAXPLANES + u] += wrong ? l : 0u;
            }
    }
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int j = 0; j < 2 * (1 + UE_MAXPLANES); ++j) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) c[j] += __shfl_xor(c[j], o, 64);          // a wave's sum: below 64 * 2^23
        if (lane == 0) red[wid][j] = c[j];
    }
    __syncthreads();
    if (threadIdx.x < 2 * (1 + UE_MAXPLANES)) {
        const int row = threadIdx.x / (1 + UE_MAXPLANES), col = threadIdx.x - row * (1 + UE_MAXPLANES);
        unsigned long long v = 0ull;
        for (int w = 0; w < PO_BLOCK / 64; ++w) v += red[w][threadIdx.x];
        if (col <= U && v) atomicAdd(out + (size_t)row * (1 + U) + col, v);
    }
}

// ---- scores in mm: surfaces, exact distance transform, reductions ---------------------------------------------------------------------
#define PO_SURF_MAXBLK 1024
#define PO_RED_BLOCKS 256
#define ED_ROW_TJ 256          // doubles of a row staged per tile and wave
#define ED_ROW_NI 8            // outputs per lane and chunk: a chunk is 512 outputs
#define ED_COL_T 64            // tile edge of the strided passes
#define ED_COL_NI 16           // outputs per thread (4 thread rows x 16 = 64 outputs per block)

// grid-stride over the n = S * H * W voxels.  surf [K+1][n]; counts [K+1][2] or null
__global__ void __launch_bounds__(PO_BLOCK) po_surface_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int K,
                                                              unsigned char* __restrict__ surf, int* __restrict__ counts, int S, int H,
                                                              int W) {
    __shared__ int vals[PO_MAXVALUES];
    __shared__ unsigned member[9];          // bit g: grey value g is one of `values`
    __shared__ int red[(PO_MAXVALUES + 1) * 2];
    if (threadIdx.x < PO_MAXVALUES) vals[threadIdx.x] = threadIdx.x < K ? (values[threadIdx.x] & 255) : -1;      // -1 matches no byte
    if (threadIdx.x < (PO_MAXVALUES + 1) * 2) red[threadIdx.x] = 0;
    if (threadIdx.x == 0) {
        for (int i = 0; i < 9; ++i) member[i] = 0u;
        for (int k = 0; k < K; ++k) member[(values[k] & 255) >> 5] |= 1u << (values[k] & 31);
    }
    __syncthreads();
    const long plane = (long)H * W, n = plane * S;
    int cf[PO_MAXVALUES + 1], cs[PO_MAXVALUES + 1];
#pragma unroll
    for (int k = 0; k <= PO_MAXVALUES; ++k) cf[k] = cs[k] = 0;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const int z = (int)(e / plane);
        const int r = (int)(e - (long)z * plane);
        const int y = r / W, x = r - y * W;
        const int c = lab[e];
        int nb[6];          // 256: outside the volume, which is background for every problem
        nb[0] = x > 0 ? lab[e - 1] : 256;
        nb[1] = x < W - 1 ? lab[e + 1] : 256;
        nb[2] = y > 0 ? lab[e - W] : 256;
        nb[3] = y < H - 1 ? lab[e + W] : 256;
        nb[4] = z > 0 ? lab[e - plane] : 256;
        nb[5] = z < S - 1 ? lab[e + plane] : 256;
#pragma unroll
        for (int k = 0; k < PO_MAXVALUES; ++k) {
            const int v = vals[k];
            const int fg = c == v;
            const int sf = fg & ((nb[0] != v) | (nb[1] != v) | (nb[2] != v) | (nb[3] != v) | (nb[4] != v) | (nb[5] != v));
            if (k < K) surf[(size_t)k * n + e] = (unsigned char)sf;
            cf[k] += fg;
            cs[k] += sf;
        }
        int all_in = 1;
#pragma unroll
        for (int i = 0; i < 6; ++i) all_in &= nb[i] < 256 ? (int)((member[nb[i] >> 5] >> (nb[i] & 31)) & 1u) : 0;
        const int fg = (int)((member[c >> 5] >> (c & 31)) & 1u);
        const int sf = fg & (all_in ^ 1);
        surf[(size_t)K * n + e] = (unsigned char)sf;
        cf[PO_MAXVALUES] += fg;
        cs[PO_MAXVALUES] += sf;
    }
    if (!counts) return;          // uniform: a kernel argument
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k <= PO_MAXVALUES; ++k) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            cf[k] += __shfl_xor(cf[k], o, 64);
            cs[k] += __shfl_xor(cs[k], o, 64);
        }
        if (lane == 0) {
            atomicAdd(&red[2 * k], cf[k]);
            atomicAdd(&red[2 * k + 1], cs[k]);
        }
    }
    __syncthreads();
    if (threadIdx.x < 2 * (K + 1)) {          // problem K (the joint one) sits in slot PO_MAXVALUES of the block's counters
        const int k = threadIdx.x >> 1, slot = k == K ? PO_MAXVALUES : k;
        const int v = red[2 * slot + (threadIdx.x & 1)];
        if (v) atomicAdd(counts + threadIdx.x, v);
    }
}

__device__ __forceinline__ double ed_load(const unsigned char* p, long i) { return p[i] ? 0.0 : (double)INFINITY; }
__device__ __forceinline__ double ed_load(const double* p, long i) { return p[i]; }

// the pass along the contiguous axis: in, out [A][L].  grid ceil(A / 4), block 256: wave w of a block owns row 4 * blockIdx.x + w
template <typename TIN, bool SQRT>
__global__ void __launch_bounds__(PO_BLOCK) po_edt_row_kernel(const TIN* __restrict__ in, double* __restrict__ out, long A, int L,
                                                              double sp) {
    __shared__ double line[PO_BLOCK / 64][ED_ROW_TJ];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const long row = (long)blockIdx.x * (PO_BLOCK / 64) + wid;
    const bool live = row < A;
    const long base = live ? row * L : 0;
    for (int i0 = 0; i0 < L; i0 += 64 * ED_ROW_NI) {
        double acc[ED_ROW_NI];
#pragma unroll
        for (int m = 0; m < ED_ROW_NI; ++m) acc[m] = (double)INFINITY;
        for (int j0 = 0; j0 < L; j0 += ED_ROW_TJ) {
            __syncthreads();          // L is uniform, so every wave of the block reaches every barrier
            for (int t = lane; t < ED_ROW_TJ; t += 64) line[wid][t] = (live && j0 + t < L) ? ed_load(in, base + j0 + t) : (double)INFINITY;
            __syncthreads();
            const int nj = min(ED_ROW_TJ, L - j0);
            double dj[ED_ROW_NI];          // i - j0 per output: integers, exact in fp64
#pragma unroll
            for (int m = 0; m < ED_ROW_NI; ++m) dj[m] = (double)(i0 + lane + 64 * m - j0);
            for (int t = 0; t < nj; ++t) {
                const double v = line[wid][t], ft = (double)t;
#pragma unroll
                for (int m = 0; m < ED_ROW_NI; ++m)
                    if (i0 + 64 * m < L) {          // wave-uniform
                        const double d = sp * (dj[m] - ft);
                        acc[m] = fmin(acc[m], fma(d, d, v));
                    }
            }
        }
#pragma unroll
        for (int m = 0; m < ED_ROW_NI; ++m) {
            const int i = i0 + lane + 64 * m;
            if (live && i < L) out[base + i] = SQRT ? sqrt(acc[m]) : acc[m];
        }
    }
}

// a pass along a strided axis: in, out [A][L][B], B contiguous.  grid A * nb * ni (nb = ceil(B / 64), ni = ceil(L / 64)), block 256 =
// 64 columns b x 4 thread rows; thread row ty owns the outputs i = 64 * ic + 16 * ty + m, m < 16
template <bool SQRT>
__global__ void __launch_bounds__(PO_BLOCK) po_edt_col_kernel(const double* __restrict__ in, double* __restrict__ out, int L, long B, long nb,
                                                              int ni, double sp) {
    __shared__ double tile[ED_COL_T][ED_COL_T];          // [j][b]
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    long bid = blockIdx.x;
    const int ic = (int)(bid % ni);
    bid /= ni;
    const long bb = bid % nb, a = bid / nb;
    const long b = bb * ED_COL_T + tx;
    const bool live = b < B;
    const long base = a * (long)L * B + (live ? b : 0);
    const int i_base = ic * ED_COL_T + ty * ED_COL_NI;
    double acc[ED_COL_NI];
#pragma unroll
    for (int m = 0; m < ED_COL_NI; ++m) acc[m] = (double)INFINITY;
    for (int j0 = 0; j0 < L; j0 += ED_COL_T) {
        __syncthreads();
        for (int r = ty; r < ED_COL_T; r += PO_BLOCK / 64) tile[r][tx] = (live && j0 + r < L) ? in[base + (long)(j0 + r) * B] : (double)INFINITY;
        __syncthreads();
        const int nj = min(ED_COL_T, L - j0);
        const double d0 = (double)(i_base - j0);
        for (int t = 0; t < nj; ++t) {
            const double v = tile[t][tx], dj = d0 - (double)t;
#pragma unroll
            for (int m = 0; m < ED_COL_NI; ++m) {
                const double d = sp * (dj + (double)m);
                acc[m] = fmin(acc[m], fma(d, d, v));
            }
        }
    }
#pragma unroll
    for (int m = 0; m < ED_COL_NI; ++m) {
        const int i = i_base + m;
        if (live && i < L) out[base + (long)i * B] = SQRT ? sqrt(acc[m]) : acc[m];
    }
}

// fixed-order block sum / order-free maximum over PO_BLOCK threads; results valid in thread 0
__device__ __forceinline__ void po_block_sum_max(double& s, double& mx, double* rs, double* rm) {
    rs[threadIdx.x] = s;
    rm[threadIdx.x] = mx;
    __syncthreads();
    for (int o = PO_BLOCK / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            rs[threadIdx.x] += rs[threadIdx.x + o];
            rm[threadIdx.x] = fmax(rm[threadIdx.x], rm[threadIdx.x + o]);
        }
        __syncthreads();
    }
    s = rs[0];
    mx = rm[0];
}

// part [gridDim.x][2] = (sum, max) of dist over the voxels where surf != 0, this block's grid-stride share
__global__ void __launch_bounds__(PO_BLOCK) po_surface_reduce_kernel(const unsigned char* __restrict__ surf, const double* __restrict__ dist,
                                                                     long n, double* __restrict__ part) {
    __shared__ double rs[PO_BLOCK], rm[PO_BLOCK];
    double s = 0.0, mx = 0.0;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK)
        if (surf[e]) {
            const double d = dist[e];
            s += d;
            mx = fmax(mx, d);
        }
    po_block_sum_max(s, mx, rs, rm);
    if (threadIdx.x == 0) {
        part[2 * blockIdx.x] = s;
        part[2 * blockIdx.x + 1] = mx;
    }
}

// one block: row [6] = nP, nT, |surface(P)|, |surface(T)|, sum, max from the counts [K+1][2] of either side and the partials
// part [2][nblk][2] of the two directions; sum and max are nan when either surface is empty
__global__ void __launch_bounds__(PO_BLOCK) po_surface_final_kernel(const int* __restrict__ cp, const int* __restrict__ ct,
                                                                    const double* __restrict__ part, int nblk, int k,
                                                                    double* __restrict__ row) {
    __shared__ double rs[PO_BLOCK], rm[PO_BLOCK];
    double s = 0.0, mx = 0.0;
    if ((int)threadIdx.x < nblk) {
        const double* a = part + 2 * threadIdx.x;
        const double* b = part + 2 * (size_t)nblk + 2 * threadIdx.x;
        s = a[0] + b[0];
        mx = fmax(a[1], b[1]);
    }
    po_block_sum_max(s, mx, rs, rm);
    if (threadIdx.x == 0) {
        const int sp = cp[2 * k + 1], st = ct[2 * k + 1];
        const bool empty = sp == 0 || st == 0;
        row[0] = (double)cp[2 * k];
        row[1] = (double)ct[2 * k];
        row[2] = (double)sp;
        row[3] = (double)st;
        row[4] = empty ? (double)NAN : s;
        row[5] = empty ? (double)NAN : mx;
    }
}

// blocks of PO_BLOCK threads for n >= 1 elements, at most `cap`: PO_MAXBLK restore / overlap, PO_SURF_MAXBLK the surface sweep, the hole fill, the tile blend and the merge of views, PO_RED_BLOCKS
// the reductions (po_surface_final_kernel adds that many partials with one block), OS_MAXBLK the order statistics, CC_MAXBLK the components
static unsigned po_grid(long n, long cap) {
    const long b = (n + PO_BLOCK - 1) / PO_BLOCK;
    return (unsigned)(b < cap ? b : cap);
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

// [S,H,W] with 1 <= H, W and fewer than 2^31 voxels
static bool po_volume_ok(int S, int H, int W) { return H >= 1 && W >= 1 && (long)S * H * W < 0x7fffffffL; }
static bool po_spacing_ok(double d) { return isfinite(d) && d > 0.0; }
static bool po_spacings_ok(double dz, double dy, double dx) { return po_spacing_ok(dz) && po_spacing_ok(dy) && po_spacing_ok(dx); }
static bool po_problem_ok(int S, int H, int W, int K) { return po_volume_ok(S, H, W) && K >= 1 && K <= PO_MAXVALUES; }

// sites [S,H,W] -> a [S,H,W] distances in mm; b is scratch of the same size.  W pass sites -> a, H pass a -> b, S pass b -> a (sqrt)
static int po_edt(const unsigned char* sites, double* a, double* b, int S, int H, int W, double dz, double dy, double dx, hipStream_t st) {
    const long rows = (long)S * H;
    hipLaunchKernelGGL((po_edt_row_kernel<unsigned char, false>), dim3((unsigned)((rows + 3) / 4)), dim3(PO_BLOCK), 0, st, sites, a, rows, W,
                       dx);
    long nb = ((long)W + ED_COL_T - 1) / ED_COL_T;
    int ni = (H + ED_COL_T - 1) / ED_COL_T;
    hipLaunchKernelGGL((po_edt_col_kernel<false>), dim3((unsigned)((long)S * nb * ni)), dim3(PO_BLOCK), 0, st, a, b, H, (long)W, nb, ni, dy);
    const long plane = (long)H * W;
    nb = (plane + ED_COL_T - 1) / ED_COL_T;
    ni = (S + ED_COL_T - 1) / ED_COL_T;
    hipLaunchKernelGGL((po_edt_col_kernel<true>), dim3((unsigned)(nb * ni)), dim3(PO_BLOCK), 0, st, b, a, S, plane, nb, ni, dz);
    return MMSEG_CHECK_LAUNCH();
}

static int po_surface(const unsigned char* label, const int* values, unsigned char* surf, int* counts, int S, int H, int W, int K,
                      hipStream_t st) {
    const long n = (long)S * H * W;
    if (counts) {
        const hipError_t rc = hipMemsetAsync(counts, 0, sizeof(int) * 2 * (size_t)(K + 1), st);
        if (rc != hipSuccess) return (int)rc;
    }
    hipLaunchKernelGGL(po_surface_kernel, dim3(po_grid(n, PO_SURF_MAXBLK)), dim3(PO_BLOCK), 0, st, label, values, K, surf, counts, S, H, W);
    return MMSEG_CHECK_LAUNCH();
}

static long po_round8(long bytes) { return (bytes + 7) / 8; }

// ---- order statistics of the surface distances -----------------------------------------------------------------------------------------
// A non-negative finite fp64 orders as its bit pattern read as a 64-bit unsigned integer, so the k-th smallest value is found digit by
// digit on the patterns, most significant digit first: of the elements whose higher digits equal the prefix found so far, count the
// current digit's values, pick the digit d whose bin holds the rank (count of smaller digits <= rank < count up to d), append d to the
// prefix and reduce the rank by the count of smaller digits.  After 64 / OS_BITS passes the prefix is the value itself: exact, no
// comparison of rounded numbers anywhere.  The ranks lo and hi of the percentile are followed in the same passes (two prefixes, two
// histograms).
// The list's order differs from run to run (the waves' atomicAdds on its counter land in any order).  Nothing downstream depends on
// it: the list is only ever counted (integer histograms, integer sums of which are order independent), never summed in floating
// point or indexed by position, so out is bitwise equal between two runs.
// No launch waits for another block: no spin loops, no cooperative launch; every loop is bounded by n (the grid-stride loops over the
// inputs and over the list, whose length is at most 2 n) or by the number of digits (the launcher's pass loop, the 8-step scan).
#define OS_BITS 8
#define OS_BINS (1 << OS_BITS)          // == PO_BLOCK: thread t owns bin t
#define OS_PASSES (64 / OS_BITS)
#define OS_MAXBLK 512

struct os_state {
    unsigned count;                    // length of the list = N
    unsigned le;                       // |{x <= tolerance}|
    unsigned rank[2];                  // of lo, hi among the elements whose higher digits equal prefix[.]
    unsigned long long prefix[2];      // the digits found so far, in place
    double frac;                       // h - lo
    double pad;                        // the histograms that follow start on a 16-byte boundary
};
#define OS_STATE_DOUBLES ((long)(sizeof(os_state) / 8 + OS_PASSES * 2 * OS_BINS * sizeof(unsigned) / 8))

// list[count ...] <- the v[e] with m[e] != 0, in any order.  Wave-aggregated: a ballot, one returning atomicAdd per wave that selected
// something, every selected lane stores at its rank among the wave's selected lanes.  The list has room for 2 n values and each of the
// two calls per list appends at most n.
__global__ void __launch_bounds__(PO_BLOCK) os_append_kernel(const double* __restrict__ v, const unsigned char* __restrict__ m, long n,
                                                             double tol, double* __restrict__ list, os_state* __restrict__ st) {
    const int lane = threadIdx.x & 63;
    for (long e0 = (long)blockIdx.x * PO_BLOCK + (threadIdx.x - lane); e0 < n; e0 += (long)gridDim.x * PO_BLOCK) {          // wave-uniform
        const long e = e0 + lane;
        const bool sel = e < n && m[e] != 0;
        const double x = sel ? v[e] : 0.0;
        const unsigned long long picked = __ballot(sel);
        if (!picked) continue;
        const int leader = __ffsll((long long)picked) - 1;
        int base = 0;
        if (lane == leader) base = (int)atomicAdd(&st->count, (unsigned)__popcll(picked));
        base = __shfl(base, leader, 64);
        if (sel) list[(size_t)(unsigned)base + (unsigned)__popcll(picked & ((1ull << lane) - 1ull))] = x;
        const unsigned long long within = __ballot(sel && x <= tol);
        if (within && lane == leader) atomicAdd(&st->le, (unsigned)__popcll(within));
    }
}

// hist [2][OS_BINS] += the digit `pass` (0 = most significant) of the list's elements whose higher digits equal prefix[r]
__global__ void __launch_bounds__(PO_BLOCK) os_hist_kernel(const double* __restrict__ list, const os_state* __restrict__ st,
                                                           unsigned* __restrict__ hist, int pass) {
    __shared__ unsigned lh[2][OS_BINS];
    const unsigned long count = st->count;
    if ((unsigned long)blockIdx.x * PO_BLOCK >= count) return;          // block-uniform: nothing of the list is this block's
    lh[0][threadIdx.x] = 0u;
    lh[1][threadIdx.x] = 0u;
    __syncthreads();
    const int shift = 64 - OS_BITS * (pass + 1);
    const int up = (shift + OS_BITS) & 63;          // pass 0 has no higher digits: every element matches
    const unsigned long long p0 = pass ? st->prefix[0] >> up : 0ull, p1 = pass ? st->prefix[1] >> up : 0ull;
    for (unsigned long e = (unsigned long)blockIdx.x * PO_BLOCK + threadIdx.x; e < count; e += (unsigned long)gridDim.x * PO_BLOCK) {
        const unsigned long long b = (unsigned long long)__double_as_longlong(list[e]);
        const unsigned d = (unsigned)(b >> shift) & (OS_BINS - 1);
        const unsigned long long hb = pass ? b >> up : 0ull;
        if (hb == p0) atomicAdd(&lh[0][d], 1u);
        if (hb == p1) atomicAdd(&lh[1][d], 1u);
    }
    __syncthreads();
    for (int r = 0; r < 2; ++r) {
        const unsigned c = lh[r][threadIdx.x];
        if (c) atomicAdd(hist + r * OS_BINS + threadIdx.x, c);
    }
}

// one block.  Pass 0 first turns the list's length into the two ranks: h = (N - 1) * (percentile / 100) in fp64, lo = floor(h),
// hi = min(lo + 1, N - 1).  Then an inclusive scan of either histogram; the one bin that holds the rank extends the prefix.  With
// N == 0 no bin does, and the state stays zero.
__global__ void __launch_bounds__(PO_BLOCK) os_pick_kernel(os_state* __restrict__ st, const unsigned* __restrict__ hist, int pass,
                                                           double percentile) {
#pragma clang fp contract(off)
    __shared__ unsigned sc[2][OS_BINS];
    __shared__ unsigned rk[2];
    const int t = threadIdx.x;
    if (t == 0) {
        if (pass == 0) {
            const unsigned N = st->count;
            unsigned lo = 0u, hi = 0u;
            double frac = 0.0;
            if (N > 0u) {
                const double h = (double)(N - 1u) * (percentile / 100.0);          // numpy's order: the quantile first
                const double fl = fmin(floor(h), (double)(N - 1u));
                lo = (unsigned)fl;
                hi = lo + 1u < N ? lo + 1u : N - 1u;
                frac = h - fl;
            }
            st->rank[0] = lo;
            st->rank[1] = hi;
            st->frac = frac;
        }
        rk[0] = st->rank[0];
        rk[1] = st->rank[1];
    }
    const unsigned own[2] = {hist[t], hist[OS_BINS + t]};
    sc[0][t] = own[0];
    sc[1][t] = own[1];
    __syncthreads();
    for (int o = 1; o < OS_BINS; o <<= 1) {
        const unsigned a0 = t >= o ? sc[0][t - o] : 0u, a1 = t >= o ? sc[1][t - o] : 0u;
        __syncthreads();
        sc[0][t] += a0;
        sc[1][t] += a1;
        __syncthreads();
    }
    const int shift = 64 - OS_BITS * (pass + 1);
    for (int r = 0; r < 2; ++r) {
        const unsigned incl = sc[r][t], excl = incl - own[r];
        if (excl <= rk[r] && rk[r] < incl) {          // true for exactly one t when the list is not empty
            st->prefix[r] |= (unsigned long long)t << shift;
            st->rank[r] = rk[r] - excl;
        }
    }
}

// D_(lo) + (h - lo) * (D_(hi) - D_(lo)), without contraction
__device__ __forceinline__ double os_percentile(const os_state* st, double& lo, double& hi) {
#pragma clang fp contract(off)
    lo = __longlong_as_double((long long)st->prefix[0]);
    hi = __longlong_as_double((long long)st->prefix[1]);
    const double step = hi - lo;
    return lo + st->frac * step;
}

// out [5] = N, |{x <= tolerance}|, the percentile, D_(lo), D_(hi); the last three nan for an empty list
__global__ void os_out_kernel(const os_state* __restrict__ st, double* __restrict__ out) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double lo, hi;
    const double v = os_percentile(st, lo, hi);
    const bool empty = st->count == 0u;
    out[0] = (double)st->count;
    out[1] = (double)st->le;
    out[2] = empty ? (double)NAN : v;
    out[3] = empty ? (double)NAN : lo;
    out[4] = empty ? (double)NAN : hi;
}

// row [8] of mmseg_surface_scores: columns 7 and 8 = |{x <= tolerance}|, the percentile; nan when either surface is empty
__global__ void os_row_kernel(const os_state* __restrict__ st, const int* __restrict__ cp, const int* __restrict__ ct, int k,
                              double* __restrict__ row) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double lo, hi;
    const double v = os_percentile(st, lo, hi);
    const bool empty = cp[2 * k + 1] == 0 || ct[2 * k + 1] == 0;
    row[6] = empty ? (double)NAN : (double)st->le;
    row[7] = empty ? (double)NAN : v;
}

struct os_args {
    double percentile, tolerance;
};

static bool os_args_ok(double percentile, double tolerance) {
    return isfinite(percentile) && percentile >= 0.0 && percentile <= 100.0 && isfinite(tolerance) && tolerance >= 0.0;
}

// state: the os_state, then the OS_PASSES histograms [2][OS_BINS]; all of it is zeroed here, on the stream
static int os_reset(double* state, hipStream_t st) {
    return (int)hipMemsetAsync(state, 0, sizeof(double) * (size_t)OS_STATE_DOUBLES, st);
}

static void os_append(const double* v, const unsigned char* m, long n, double tol, double* list, double* state, hipStream_t st) {
    hipLaunchKernelGGL(os_append_kernel, dim3(po_grid(n, OS_MAXBLK)), dim3(PO_BLOCK), 0, st, v, m, n, tol, list,
                       reinterpret_cast<os_state*>(state));
}

// the radix passes over a list of at most `capacity` values; the grid is sized by the capacity, the loops by the device's count
static void os_select(const double* list, double* state, long capacity, double percentile, hipStream_t st) {
    os_state* s = reinterpret_cast<os_state*>(state);
    unsigned* hist = reinterpret_cast<unsigned*>(state + sizeof(os_state) / 8);
    for (int pass = 0; pass < OS_PASSES; ++pass) {
        hipLaunchKernelGGL(os_hist_kernel, dim3(po_grid(capacity, OS_MAXBLK)), dim3(PO_BLOCK), 0, st, list, s, hist + pass * 2 * OS_BINS, pass);
        hipLaunchKernelGGL(os_pick_kernel, dim3(1), dim3(PO_BLOCK), 0, st, s, hist + pass * 2 * OS_BINS, pass, percentile);
    }
}

// ---- connected components per organ, and the largest one of each --------------------------------------------------------------------
// A union-find whose parent array is `comp` itself: comp[e] = 1 + (linear index of the parent of voxel e), 0 for a voxel that is no
// organ's; a root points to itself.  A link always hangs the larger index below the smaller one (an integer atomic minimum), so
// parents only decrease, every chain ends, and the root of a set is its smallest index: the labelling is canonical whatever the
// order of blocks and atomics.  Three launches, none of which waits for another block:
//   po_cc_local_kernel    a tile of 4 x 8 x 32 voxels per block, resolved in LDS (links along the row for free, the other backward
//                         neighbours by unions), written out as global indices
//   po_cc_merge_kernel    every voxel with a backward neighbour in another tile joins the two sets in global memory
//   po_cc_flatten_kernel  comp[e] = 1 + root
// "Backward" neighbours are those with a smaller linear index: 3 of the 6 face neighbours, 13 of the 26.
#define CC_TX 32
#define CC_TY 8
#define CC_TZ 4
#define CC_TILE (CC_TX * CC_TY * CC_TZ)
#define CC_MAXBLK 4096          // of the grid-stride kernels

// (dz, dy, dx) of the backward neighbours: the row neighbour, the other two faces, then the ten that only 26-connectivity has
__device__ const signed char cc_off[13][3] = {{0, 0, -1}, {0, -1, 0},  {-1, 0, 0},  {0, -1, -1}, {0, -1, 1}, {-1, 0, -1}, {-1, 0, 1},
                                              {-1, -1, 0}, {-1, 1, 0}, {-1, -1, -1}, {-1, -1, 1}, {-1, 1, -1}, {-1, 1, 1}};

// p[i] = 1 + parent of i.  SCOPE: workgroup for LDS, agent for global memory (loads that other CUs' atomics are visible to)
template <int SCOPE>
__device__ __forceinline__ int cc_find(int* p, int i) {
    for (;;) {
        const int q = __hip_atomic_load(p + i, __ATOMIC_RELAXED, SCOPE) - 1;
        if (q == i) return i;
        i = q;          // q < i: the chain ends
    }
}

template <int SCOPE>
__device__ __forceinline__ void cc_union(int* p, int a, int b) {
    for (;;) {
        a = cc_find<SCOPE>(p, a);
        b = cc_find<SCOPE>(p, b);
        if (a == b) return;
        if (a < b) {
            const int t = a;
            a = b;
            b = t;
        }
        const int old = __hip_atomic_fetch_min(p + a, b + 1, __ATOMIC_RELAXED, SCOPE) - 1;          // hang a below b
        if (old == a) return;
        a = old;          // a was no root any more and now points to min(old, b): join its former parent old < a with b as well
    }
}

// bit g of member[]: grey value g is one of `values`
__device__ __forceinline__ void cc_member_init(unsigned* member, const int* __restrict__ values, int K) {
    if (threadIdx.x == 0) {
        for (int i = 0; i < 8; ++i) member[i] = 0u;
        for (int k = 0; k < K; ++k) {
            const int v = values[k];
            if (v >= 0 && v <= 255) member[v >> 5] |= 1u << (v & 31);
        }
    }
}

// grid = number of tiles (x fastest), block PO_BLOCK: thread t owns the voxels (lz, t >> 5, t & 31), lz < 4.
// COMPLEMENT (the hole filling): one class, the voxels whose grey value is not values[K]; K is then that organ's index.  nnb = 2 leaves
// the link across slices out (cc_off[2]): every slice is a problem of its own.
template <bool COMPLEMENT>
__global__ void __launch_bounds__(PO_BLOCK) po_cc_local_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int K,
                                                               int* __restrict__ comp, int S, int H, int W, int ntx, int nty, int nnb) {
    __shared__ unsigned member[8];
    __shared__ int grey[CC_TILE];          // the grey value of an organ voxel (COMPLEMENT: 0 for a voxel of the complement), -1 for
    __shared__ int par[CC_TILE];           // everything else and outside the volume
    const int organ = COMPLEMENT ? values[K] : 0;
    if constexpr (!COMPLEMENT) {
        cc_member_init(member, values, K);
        __syncthreads();
    }
    int tile = blockIdx.x;
    const int x0 = (tile % ntx) * CC_TX;
    tile /= ntx;
    const int y0 = (tile % nty) * CC_TY, z0 = (tile / nty) * CC_TZ;
    const int lx = threadIdx.x & (CC_TX - 1), ly = threadIdx.x >> 5;
    const int x = x0 + lx, y = y0 + ly;
    const long plane = (long)H * W;
#pragma unroll
    for (int lz = 0; lz < CC_TZ; ++lz) {
        int v = -1;
        if (x < W && y < H && z0 + lz < S) {
            v = lab[(long)(z0 + lz) * plane + (long)y * W + x];
            if constexpr (COMPLEMENT) v = v != organ ? 0 : -1;
            else if (!((member[v >> 5] >> (v & 31)) & 1u)) v = -1;
        }
        grey[lz * PO_BLOCK + threadIdx.x] = v;
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < CC_TZ; ++lz) {          // the row neighbour is linked without an atomic
        const int l = lz * PO_BLOCK + threadIdx.x, v = grey[l];
        par[l] = v < 0 ? 0 : ((lx > 0 && grey[l - 1] == v) ? l : l + 1);
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < CC_TZ; ++lz) {          // shorten the row chains (a racing reader sees the old or the new parent: both valid)
        const int l = lz * PO_BLOCK + threadIdx.x;
        if (grey[l] >= 0) par[l] = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l) + 1;
    }
    __syncthreads();
    for (int lz = 0; lz < CC_TZ; ++lz) {
        const int l = lz * PO_BLOCK + threadIdx.x, v = grey[l];
        if (v < 0) continue;
        for (int i = 1; i < nnb; ++i) {
            const int nz = lz + cc_off[i][0], ny = ly + cc_off[i][1], nx = lx + cc_off[i][2];
            if (nz < 0 || ny < 0 || ny >= CC_TY || nx < 0 || nx >= CC_TX) continue;
            const int m = (nz * CC_TY + ny) * CC_TX + nx;
            if (grey[m] == v) cc_union<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l, m);
        }
    }
    __syncthreads();
#pragma unroll
    for (int lz = 0; lz < CC_TZ; ++lz) {
        if (!(x < W && y < H && z0 + lz < S)) continue;
        const int l = lz * PO_BLOCK + threadIdx.x;
        int c = 0;
        if (grey[l] >= 0) {          // local order = global order inside a tile, so the local root is the tile's smallest index too
            const int r = cc_find<__HIP_MEMORY_SCOPE_WORKGROUP>(par, l);
            c = 1 + (int)((long)(z0 + r / (CC_TY * CC_TX)) * plane + (long)(y0 + (r / CC_TX) % CC_TY) * W + x0 + r % CC_TX);
        }
        comp[(long)(z0 + lz) * plane + (long)y * W + x] = c;
    }
}

// grid-stride over the voxels: unions across tile faces.  COMPLEMENT: every labelled voxel is of the one class (lab is not read)
template <bool COMPLEMENT>
__global__ void __launch_bounds__(PO_BLOCK) po_cc_merge_kernel(const unsigned char* __restrict__ lab, int* comp, int S, int H, int W, int nnb) {
    const long plane = (long)H * W, n = plane * S;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const int z = (int)(e / plane);
        const int r = (int)(e - (long)z * plane);
        const int y = r / W, x = r - y * W;
        const int lx = x & (CC_TX - 1), ly = y & (CC_TY - 1);
        if (lx != 0 && lx != CC_TX - 1 && ly != 0 && ly != CC_TY - 1 && (z & (CC_TZ - 1)) != 0) continue;          // inside its tile
        if (comp[e] == 0) continue;          // no organ's voxel (comp[e] only changes between non-zero values)
        const int v = COMPLEMENT ? 0 : lab[e];
        for (int i = 0; i < nnb; ++i) {
            const int nz = z + cc_off[i][0], ny = y + cc_off[i][1], nx = x + cc_off[i][2];
            if (nz < 0 || ny < 0 || ny >= H || nx < 0 || nx >= W) continue;
            if (nz / CC_TZ == z / CC_TZ && ny / CC_TY == y / CC_TY && nx / CC_TX == x / CC_TX) continue;          // po_cc_local_kernel's
            const long m = (long)nz * plane + (long)ny * W + nx;
            if (COMPLEMENT ? comp[m] != 0 : lab[m] == v) cc_union<__HIP_MEMORY_SCOPE_AGENT>(comp, (int)e, (int)m);
        }
    }
}

__global__ void __launch_bounds__(PO_BLOCK) po_cc_flatten_kernel(int* comp, long n) {
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK)
        if (comp[e]) comp[e] = cc_find<__HIP_MEMORY_SCOPE_AGENT>(comp, (int)e) + 1;          // a racing reader: old or new parent, both valid
}

// size[root] += voxels of the component.  Lanes of a wave that hold the same root add once (one atomic per wave inside a large body)
__global__ void __launch_bounds__(PO_BLOCK) po_cc_size_kernel(const int* __restrict__ comp, int* __restrict__ size, long n) {
    const int lane = threadIdx.x & 63;
    for (long e0 = (long)blockIdx.x * PO_BLOCK + (threadIdx.x - lane); e0 < n; e0 += (long)gridDim.x * PO_BLOCK) {          // wave-uniform
        const long e = e0 + lane;
        const int c = e < n ? comp[e] : 0;
        unsigned long long todo = __ballot(c != 0);
        while (todo) {
            const int leader = __ffsll((long long)todo) - 1;
            const int r = __shfl(c, leader, 64);
            const unsigned long long same = __ballot(c == r);
            if (lane == leader) atomicAdd(size + (r - 1), __popcll(same));
            todo &= ~same;
        }
    }
}

// lut[g] = the lowest k with values[k] == g, or -1
__device__ __forceinline__ void cc_lut_init(int* lut, const int* __restrict__ values, int K) {
    lut[threadIdx.x] = -1;          // PO_BLOCK == 256 entries
    __syncthreads();
    if (threadIdx.x == 0)
        for (int k = K - 1; k >= 0; --k) {
            const int v = values[k];
            if (v >= 0 && v <= 255) lut[v] = k;
        }
    __syncthreads();
}

// per root: stats[k] += (1, size, .), keys[k] = max over (size << 32) | (0xffffffff - root): the largest, of equals the smallest root
__global__ void __launch_bounds__(PO_BLOCK) po_cc_winner_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int K,
                                                                const int* __restrict__ comp, const int* __restrict__ size,
                                                                unsigned long long* __restrict__ keys, int* __restrict__ stats, long n) {
    __shared__ int lut[256];
    cc_lut_init(lut, values, K);
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        if (comp[e] != (int)e + 1) continue;
        const int k = lut[lab[e]], sz = size[e];
        atomicAdd(stats + 3 * k, 1);
        atomicAdd(stats + 3 * k + 1, sz);
        atomicMax(keys + k, ((unsigned long long)(unsigned)sz << 32) | (unsigned long long)(0xffffffffu - (unsigned)e));
    }
}

// out = label, but 0 on organ voxels outside their organ's winner; stats[k][2] = the winner's size
__global__ void __launch_bounds__(PO_BLOCK) po_cc_keep_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int K,
                                                              const int* __restrict__ comp, const unsigned long long* __restrict__ keys,
                                                              unsigned char* __restrict__ out, int* __restrict__ stats, long n) {
    __shared__ int lut[256];
    __shared__ int win[PO_MAXVALUES];          // comp of the winner's voxels, 0 for an organ without voxels
    cc_lut_init(lut, values, K);
    if (threadIdx.x < K) {
        const unsigned long long key = keys[threadIdx.x];
        win[threadIdx.x] = key ? (int)(0xffffffffu - (unsigned)(key & 0xffffffffull)) + 1 : 0;
        if (blockIdx.x == 0) stats[3 * threadIdx.x + 2] = (int)(key >> 32);
    }
    __syncthreads();
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const int c = comp[e], g = lab[e];
        out[e] = (unsigned char)((c == 0 || c == win[lut[g]]) ? g : 0);
    }
}

static bool po_cc_args_ok(int S, int H, int W, int K, int connectivity) {
    return po_problem_ok(S, H, W, K) && (connectivity == 6 || connectivity == 26);
}

static int po_components(const unsigned char* label, const int* values, int* comp, int S, int H, int W, int K, int connectivity,
                         hipStream_t st) {
    const long n = (long)S * H * W;
    const int ntx = (W + CC_TX - 1) / CC_TX, nty = (H + CC_TY - 1) / CC_TY, ntz = (S + CC_TZ - 1) / CC_TZ;
    const int nnb = connectivity == 26 ? 13 : 3;
    hipLaunchKernelGGL(po_cc_local_kernel<false>, dim3((unsigned)((long)ntx * nty * ntz)), dim3(PO_BLOCK), 0, st, label, values, K, comp, S, H, W,
                       ntx, nty, nnb);
    hipLaunchKernelGGL(po_cc_merge_kernel<false>, dim3(po_grid(n, CC_MAXBLK)), dim3(PO_BLOCK), 0, st, label, comp, S, H, W, nnb);
    hipLaunchKernelGGL(po_cc_flatten_kernel, dim3(po_grid(n, CC_MAXBLK)), dim3(PO_BLOCK), 0, st, comp, n);
    return MMSEG_CHECK_LAUNCH();
}

// ---- enclosed holes of every organ ----------------------------------------------------------------------------------------------------------
// comp[e] = 1 + root for every voxel of the complement, and mark[root] = 1 where e lies on the border: the six faces of the volume, or
// with per_slice the four edges of its slice.  Every thread that marks a root stores the same byte; mark is zeroed before the launch.
__global__ void __launch_bounds__(PO_BLOCK) po_fh_flatten_kernel(int* comp, unsigned char* __restrict__ mark, int S, int H, int W,
                                                                 int per_slice) {
    const long plane = (long)H * W, n = plane * S;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        if (comp[e] == 0) continue;
        const int root = cc_find<__HIP_MEMORY_SCOPE_AGENT>(comp, (int)e);
        comp[e] = root + 1;          // a racing reader: old or new parent, both valid
        const int z = (int)(e / plane);
        const int r = (int)(e - (long)z * plane);
        const int y = r / W, x = r - y * W;
        if (x == 0 || x == W - 1 || y == 0 || y == H - 1 || (!per_slice && (z == 0 || z == S - 1))) mark[root] = 1;
    }
}

// stats[k] += (unmarked roots, voxels of values[k], voxels filled); a zero of the input in an unmarked set becomes values[k] where out
// still holds 0.  FIRST (k == 0): out holds nothing yet, and every byte of it is written here.
template <bool FIRST>
__global__ void __launch_bounds__(PO_BLOCK) po_fh_fill_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int k,
                                                              const int* __restrict__ comp, const unsigned char* __restrict__ mark,
                                                              unsigned char* out, int* __restrict__ stats, long n) {
    __shared__ int red[3];
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    __syncthreads();
    const int v = values[k];
    int holes = 0, before = 0, added = 0;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const int g = lab[e], c = comp[e];
        before += c == 0;          // comp is 0 on the organ's own voxels and nowhere else
        bool enclosed = false;
        if (c != 0) {
            enclosed = mark[c - 1] == 0;
            holes += enclosed && c == (int)e + 1;
        }
        bool fill = enclosed && g == 0;
        if constexpr (FIRST) {
            out[e] = (unsigned char)(fill ? v : g);
        } else if (fill) {
            fill = out[e] == 0;          // a lower k has been here first: this thread alone touches out[e]
            if (fill) out[e] = (unsigned char)v;
        }
        added += fill;
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        holes += __shfl_xor(holes, o, 64);
        before += __shfl_xor(before, o, 64);
        added += __shfl_xor(added, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (holes) atomicAdd(&red[0], holes);
        if (before) atomicAdd(&red[1], before);
        if (added) atomicAdd(&red[2], added);
    }
    __syncthreads();
    if (threadIdx.x < 3 && red[threadIdx.x]) atomicAdd(stats + 3 * k + threadIdx.x, red[threadIdx.x]);          // one per block and counter
}

static bool po_fh_args_ok(int S, int H, int W, int K, int per_slice) {
    return po_problem_ok(S, H, W, K) && (per_slice == 0 || per_slice == 1);
}

// the workspace of mmseg_fill_label_holes: comp [n] int32, then mark [n] bytes
static long po_fh_workspace_bytes(long n) { return (long)sizeof(int) * n + 4 * ((n + 3) / 4); }

// ---- opening, closing and smoothing of every organ by a ball in mm ------------------------------------------------------------------------
#define MO_MAXREACH 32          // voxels per axis; the row table below has (MO_MAXREACH + 1)^2 entries
#define MO_TABLE ((MO_MAXREACH + 1) * (MO_MAXREACH + 1))
#define MO_TABLE_BYTES 2048     // of the workspace, a multiple of 8 above MO_TABLE
#define MO_NONE 255             // a run: no site within the reach along x

// t(o) of the rule, in the order of the W, H and S passes of po_edt; flat (one slice at a time): dz is not read
__host__ __device__ static inline double mo_t(double dz, double dy, double dx, int oz, int oy, int ox, bool flat) {
#pragma clang fp contract(off)
    const double a = dx * (double)ox;
    double t = a * a;
    const double b = dy * (double)oy;
    t = __builtin_fma(b, b, t);
    if (!flat) {
        const double c = dz * (double)oz;
        t = __builtin_fma(c, c, t);
    }
    return t;
}

// table[oz * (ry + 1) + oy] = the largest ox <= rx with (oz, oy, ox) in the ball, -1 when the row holds none; t grows with |ox|.  One block.
__global__ void __launch_bounds__(PO_BLOCK) po_mo_table_kernel(signed char* __restrict__ table, double dz, double dy, double dx, double r2,
                                                               int rz, int ry, int rx, int flat) {
    for (int i = threadIdx.x; i < (rz + 1) * (ry + 1); i += PO_BLOCK) {
        const int oz = i / (ry + 1), oy = i - oz * (ry + 1);
        int reach = -1;
        for (int ox = 0; ox <= rx && mo_t(dz, dy, dx, oz, oy, ox, flat != 0) <= r2; ++ox) reach = ox;
        table[i] = (signed char)reach;
    }
}

// a voxel of src is a site when (src == v) == EQ; v = values[k], or 1 for a mask (k < 0)
__device__ __forceinline__ int mo_value(const int* __restrict__ values, int k) { return k < 0 ? 1 : values[k]; }

// run[e] = the distance in voxels along x from e to the nearest site of its row, MO_NONE when there is none within rx.  Grid-stride;
// at most 2 rx + 1 bytes of the row are read per voxel, consecutive lanes read consecutive bytes.
template <bool EQ>
__global__ void __launch_bounds__(PO_BLOCK) po_mo_run_kernel(const unsigned char* __restrict__ src, const int* __restrict__ values, int k,
                                                             unsigned char* __restrict__ run, int W, int rx, long n) {
    const int v = mo_value(values, k);
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const int x = (int)(e % W);
        const unsigned char* row = src + (e - x);
        const int lim = min(rx, max(x, W - 1 - x));
        int d = MO_NONE;
        for (int o = 0; o <= lim; ++o) {
            const bool left = x - o >= 0 && ((row[x - o] == v) == EQ);
            const bool right = x + o < W && ((row[x + o] == v) == EQ);
            if (left || right) {
                d = o;
                break;
            }
        }
        run[e] = (unsigned char)d;
    }
}

// is there a site q inside the volume with q - (z, y, x) in the ball?  RUN: `from` is po_mo_run_kernel's map of the sites, one byte per
// row of the ball; else rx == 0 and `from` is src itself.  Rows outside the volume are not visited.
template <bool EQ, bool RUN>
__device__ __forceinline__ bool mo_hit(const unsigned char* __restrict__ from, int v, const signed char* tab, int z, int y, int x, int S,
                                       int H, int W, int rz, int ry) {
    const int z0 = max(-rz, -z), z1 = min(rz, S - 1 - z), y0 = max(-ry, -y), y1 = min(ry, H - 1 - y);
    for (int oz = z0; oz <= z1; ++oz) {
        const signed char* trow = tab + abs(oz) * (ry + 1);
        const unsigned char* col = from + ((long)(z + oz) * H + y) * W + x;
        for (int oy = y0; oy <= y1; ++oy) {
            const int reach = trow[abs(oy)];
            if (reach < 0) continue;
            const int b = col[(long)oy * W];
            if (RUN ? b <= reach : (b == v) == EQ) return true;
        }
    }
    return false;
}

// The four passes over the rows of the ball; v = values[k], m = the mask of the pass before.
//   MO_ERODE   m[e]   = lab[e] == v and no voxel != v of the volume within the ball                       (sites: lab != v)
//   MO_OPEN    out[e] = 0 where lab[e] == v and no voxel of m within the ball, else lab[e]                (sites: m)
//   MO_DILATE  m[e]   = lab[e] == v or a voxel == v within the ball                                       (sites: lab == v)
//   MO_CLOSE   out[e] = v where lab[e] == 0, m[e], no voxel outside m within the ball and out[e] is still 0; else lab[e]   (sites: not m)
// first (k == 0): out holds nothing yet, and every byte of it is written here; later organs touch their own voxels (MO_OPEN) or
// zeros (MO_CLOSE) only, and this thread alone touches out[e].  stats[k] += (voxels == v when `before`, removed, added).
enum { MO_ERODE = 0, MO_OPEN = 1, MO_DILATE = 2, MO_CLOSE = 3 };

template <int PASS, bool RUN>
__global__ void __launch_bounds__(PO_BLOCK) po_mo_ball_kernel(const unsigned char* __restrict__ lab, const int* __restrict__ values, int k,
                                                              const unsigned char* __restrict__ from, const unsigned char* __restrict__ m,
                                                              unsigned char* dst, int* __restrict__ stats,
                                                              const signed char* __restrict__ table, int S, int H, int W, int rz, int ry,
                                                              int first, int before) {
    __shared__ signed char tab[MO_TABLE];
    __shared__ int red[3];
    for (int i = threadIdx.x; i < (rz + 1) * (ry + 1); i += PO_BLOCK) tab[i] = table[i];
    if (threadIdx.x < 3) red[threadIdx.x] = 0;
    __syncthreads();
    const int v = values[k];
    const long plane = (long)H * W, n = plane * S;
    int own = 0, removed = 0, added = 0;
    for (long e = (long)blockIdx.x * PO_BLOCK + threadIdx.x; e < n; e += (long)gridDim.x * PO_BLOCK) {
        const int z = (int)(e / plane);
        const int r = (int)(e - (long)z * plane);
        const int y = r / W, x = r - y * W;
        const int g = lab[e];
        if constexpr (PASS == MO_ERODE) {
            dst[e] = g == v && !mo_hit<false, RUN>(from, v, tab, z, y, x, S, H, W, rz, ry);
        } else if constexpr (PASS == MO_DILATE) {
            dst[e] = g == v || mo_hit<true, RUN>(from, v, tab, z, y, x, S, H, W, rz, ry);
        } else if constexpr (PASS == MO_OPEN) {
            own += g == v;
            const bool gone = g == v && !m[e] && !mo_hit<true, RUN>(from, 1, tab, z, y, x, S, H, W, rz, ry);
            if (first) dst[e] = (unsigned char)(gone ? 0 : g);
            else if (gone) dst[e] = 0;
            removed += gone;
        } else {
            own += g == v;
            bool fill = g == 0 && m[e] && (first || dst[e] == 0);
            fill = fill && !mo_hit<false, RUN>(from, 1, tab, z, y, x, S, H, W, rz, ry);
            if (first) dst[e] = (unsigned char)(fill ? v : g);
            else if (fill) dst[e] = (unsigned char)v;
            added += fill;
        }
    }
    if constexpr (PASS == MO_OPEN || PASS == MO_CLOSE) {
        if (!before) own = 0;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            own += __shfl_xor(own, o, 64);
            removed += __shfl_xor(removed, o, 64);
            added += __shfl_xor(added, o, 64);
        }
        if ((threadIdx.x & 63) == 0) {
            if (own) atomicAdd(&red[0], own);
            if (removed) atomicAdd(&red[1], removed);
            if (added) atomicAdd(&red[2], added);
        }
        __syncthreads();
        if (threadIdx.x < 3 && red[threadIdx.x]) atomicAdd(stats + 3 * k + threadIdx.x, red[threadIdx.x]);          // one per block and counter
    }
}

// what mmseg_smooth_label works with: the reach per axis in voxels (0 along the slices with per_slice) and the squared radius
struct mo_plan {
    int rz, ry, rx;
    double r2;
};

// the largest o <= MO_MAXREACH + 1 with t(o) <= r2 on an axis of spacing sp: every axis alone rounds (sp * o)^2 once
static int mo_reach(double sp, double r2) {
    int o = 0;
    while (o <= MO_MAXREACH && mo_t(0.0, 0.0, sp, 0, 0, o + 1, true) <= r2) ++o;
    return o;
}

static bool mo_axis_ok(double sp, double radius, double r2, int* reach) {
    if (!po_spacing_ok(sp) || !(floor(radius / sp) <= (double)MO_MAXREACH)) return false;
    *reach = mo_reach(sp, r2);
    return *reach <= MO_MAXREACH;
}

static bool mo_args_ok(int S, int H, int W, int K, double dz, double dy, double dx, double radius, int op, int per_slice, mo_plan* p) {
    if (!po_problem_ok(S, H, W, K) || op < 0 || op > 2 || (per_slice != 0 && per_slice != 1) || !po_spacing_ok(radius)) return false;
    p->r2 = radius * radius;
    p->rz = 0;
    if (!per_slice && !mo_axis_ok(dz, radius, p->r2, &p->rz)) return false;
    return mo_axis_ok(dy, radius, p->r2, &p->ry) && mo_axis_ok(dx, radius, p->r2, &p->rx);
}

// one map of the sites' runs along x (skipped when the ball is one voxel wide), then one pass over the rows of the ball
template <int PASS>
static void mo_pass(const unsigned char* lab, const int* values, int k, const unsigned char* sites, const unsigned char* m,
                    unsigned char* dst, int* stats, const signed char* table, unsigned char* run, int S, int H, int W, const mo_plan& p,
                    int first, int before, hipStream_t st) {
    constexpr bool EQ = PASS == MO_OPEN || PASS == MO_DILATE;          // the sites are the voxels of the set, not of its complement
    constexpr bool MASK = PASS == MO_OPEN || PASS == MO_CLOSE;        // the sites are read from the mask, not from the label volume
    const long n = (long)S * H * W;
    const dim3 grid(po_grid(n, CC_MAXBLK)), block(PO_BLOCK);
    if (p.rx > 0) {
        hipLaunchKernelGGL(po_mo_run_kernel<EQ>, grid, block, 0, st, sites, values, MASK ? -1 : k, run, W, p.rx, n);
        hipLaunchKernelGGL((po_mo_ball_kernel<PASS, true>), grid, block, 0, st, lab, values, k, (const unsigned char*)run, m, dst, stats,
                           table, S, H, W, p.rz, p.ry, first, before);
    } else {
        hipLaunchKernelGGL((po_mo_ball_kernel<PASS, false>), grid, block, 0, st, lab, values, k, sites, m, dst, stats, table, S, H, W, p.rz,
                           p.ry, first, before);
    }
}

// dst = lab opened (closing == false) or closed by the ball, organ after organ on the stream; dst must not be lab
static void mo_apply(bool closing, const unsigned char* lab, const int* values, unsigned char* dst, int* stats, const signed char* table,
                     unsigned char* run, unsigned char* mask, int S, int H, int W, int K, const mo_plan& p, int before, hipStream_t st) {
    for (int k = 0; k < K; ++k) {
        if (closing) {
            mo_pass<MO_DILATE>(lab, values, k, lab, nullptr, mask, stats, table, run, S, H, W, p, 0, 0, st);
            mo_pass<MO_CLOSE>(lab, values, k, mask, mask, dst, stats, table, run, S, H, W, p, k == 0, before, st);
        } else {
            mo_pass<MO_ERODE>(lab, values, k, lab, nullptr, mask, stats, table, run, S, H, W, p, 0, 0, st);
            mo_pass<MO_OPEN>(lab, values, k, mask, mask, dst, stats, table, run, S, H, W, p, k == 0, before, st);
        }
    }
}

// the workspace of po_surface_walk, in this order; n = S * H * W
struct po_walk_ws {
    double *da, *db;               // two distance maps [n]
    double* part;                  // the partials [2][PO_RED_BLOCKS][2] of the two directions
    int *cp, *ct;                  // counts [K+1][2] of pred and of truth
    unsigned char *sp, *st;        // surfaces [K+1][n] of pred and of truth
    double *list, *state;          // with the order statistics only: the list [2 n] and the selection's state
};

// the one place that knows the layout: fills w from ws, or only sizes it when ws is null; returns the doubles needed
static long po_walk_carve(double* ws, long n, int K, bool robust, po_walk_ws* w) {
    const long counts = po_round8((long)sizeof(int) * 4 * (K + 1));
    const long plain = 2 * n + 4 * PO_RED_BLOCKS + counts + po_round8(2 * (long)(K + 1) * n);
    if (ws) {
        w->da = ws;
        w->db = w->da + n;
        w->part = w->db + n;
        w->cp = reinterpret_cast<int*>(w->part + 4 * PO_RED_BLOCKS);
        w->ct = w->cp + 2 * (K + 1);
        w->sp = reinterpret_cast<unsigned char*>(w->part + 4 * PO_RED_BLOCKS + counts);
        w->st = w->sp + (size_t)(K + 1) * n;
        w->list = ws + plain;
        w->state = w->list + 2 * n;
    }
    return robust ? plain + 2 * n + OS_STATE_DOUBLES : plain;
}

// A loop of launches over the K + 1 problems on the stream: row k of `table` (rows `stride` doubles apart) gets its six columns and, with
// `robust`, two more: every map's surface distances are then appended to the problem's list before the next transform overwrites the map
static int po_surface_walk(const unsigned char* pred, const unsigned char* truth, const int* values, double* table, double* ws, int S,
                           int H, int W, int K, double dz, double dy, double dx, int stride, const os_args* robust /* null: six columns */,
                           hipStream_t st) {
    const long n = (long)S * H * W;
    po_walk_ws w;
    po_walk_carve(ws, n, K, robust != nullptr, &w);
    int rc = po_surface(pred, values, w.sp, w.cp, S, H, W, K, st);
    if (rc) return rc;
    rc = po_surface(truth, values, w.st, w.ct, S, H, W, K, st);
    if (rc) return rc;
    const int nblk = (int)po_grid(n, PO_RED_BLOCKS);
    for (int k = 0; k <= K; ++k) {
        const unsigned char* side[2] = {w.sp + (size_t)k * n, w.st + (size_t)k * n};
        double* row = table + (size_t)stride * k;
        if (robust && (rc = os_reset(w.state, st))) return rc;
        for (int d = 0; d < 2; ++d) {          // the distance to surface(T) over surface(P), then the other way round
            rc = po_edt(side[1 - d], w.da, w.db, S, H, W, dz, dy, dx, st);
            if (rc) return rc;
            hipLaunchKernelGGL(po_surface_reduce_kernel, dim3(nblk), dim3(PO_BLOCK), 0, st, side[d], w.da, n, w.part + d * 2 * nblk);
            if (robust) os_append(w.da, side[d], n, robust->tolerance, w.list, w.state, st);
        }
        hipLaunchKernelGGL(po_surface_final_kernel, dim3(1), dim3(PO_BLOCK), 0, st, w.cp, w.ct, w.part, nblk, k, row);
        if (robust) {
            os_select(w.list, w.state, 2 * n, robust->percentile, st);
            hipLaunchKernelGGL(os_row_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const os_state*>(w.state), w.cp, w.ct, k, row);
        }
    }
    return MMSEG_CHECK_LAUNCH();
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
    const dim3 grid(po_grid(pack ? (long)H * (W >> 2) : (long)H * W, PO_MAXBLK), S);
    const po_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    const hipStream_t st = (hipStream_t)stream;
    if (vec4 && pack) po_launch<true, true>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    else if (vec4) po_launch<true, false>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    else if (pack) po_launch<false, true>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    else po_launch<false, false>(grid, st, prob, values, K, out, H, W, RH, RW, OH, OW, ar, ac, C, order);
    return MMSEG_CHECK_LAUNCH();
}

// prob [TR*TC,S,OH,OW,C] fp32 (tile tr * TC + tc), rows [TR,3] / cols [TC,3] int32 (lo, kept, before) and wr [TR,OH] / wc [TC,OW] fp32 on
// the device, out [S,RH,RW,K] fp32: every element is written.  One launch; no atomics, nothing allocated or synchronised.
int mmseg_blend_tiles(const float* prob, const int* rows, const int* cols, const float* wr, const float* wc, float* out, int S, int TR,
                      int TC, int OH, int OW, int C, int K, int RH, int RW, void* stream) {
    if (S == 0) return 0;
    const long lim = 0x80000000L;          // bytes of either tensor
    if (!prob || !rows || !cols || !wr || !wc || !out || prob == out || S < 0 || TR < 1 || TR > BT_MAXTILES || TC < 1 || TC > BT_MAXTILES ||
        OH < 1 || OW < 1 || RH < 1 || RW < 1 || C < 1 || K < 1 || K > C || K > PO_MAXVALUES)
        return (int)hipErrorInvalidValue;
    // the products are taken factor by factor, so that none of them overflows before it is compared
    long in = (long)sizeof(float) * TR * TC, px = (long)sizeof(float) * S;
    for (const int f : {S, OH, OW, C}) {
        in *= f;
        if (in >= lim) return (int)hipErrorInvalidValue;
    }
    for (const int f : {RH, RW, K}) {
        px *= f;
        if (px >= lim) return (int)hipErrorInvalidValue;
    }
    const bool vec4 = K == 4 && (C & 3) == 0 && ((uintptr_t)prob & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const int n = (int)((long)S * RH * RW * (vec4 ? 1 : K));
    const dim3 grid(po_grid(n, PO_SURF_MAXBLK)), block(PO_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (vec4) hipLaunchKernelGGL(po_blend_kernel<true>, grid, block, 0, st, prob, rows, cols, wr, wc, out, S, TR, TC, OH, OW, C, K, RH, RW, n);
    else hipLaunchKernelGGL(po_blend_kernel<false>, grid, block, 0, st, prob, rows, cols, wr, wc, out, S, TR, TC, OH, OW, C, K, RH, RW, n);
    return MMSEG_CHECK_LAUNCH();
}

// prob [V*N,OH,OW,C] fp32 (view v holds slices v * N .. v * N + N - 1), back [V,6] fp64 on the device, out [N,OH,OW,K] fp32: every element is
// written.  One launch; no atomics, nothing allocated or synchronised.
int mmseg_merge_views(const float* prob, const double* back, float* out, int V, int N, int OH, int OW, int C, int K, void* stream) {
    if (N == 0) return 0;
    if (!prob || !back || !out || prob == out || N < 0 || V < 1 || V > MV_MAXVIEWS || OH < 1 || OW < 1 || C < 1 || K < 1 || K > C ||
        K > PO_MAXVALUES)
        return (int)hipErrorInvalidValue;
    // factor by factor, so that the product does not overflow before it is compared
    long pixels = N;
    for (const int f : {OH, OW}) {
        pixels *= f;
        if (pixels >= (1L << 29)) return (int)hipErrorInvalidValue;
    }
    const bool vec4 = K == 4 && (C & 3) == 0 && ((uintptr_t)prob & 15) == 0 && ((uintptr_t)out & 15) == 0;
    const long total = pixels * (vec4 ? 1 : K);
    const dim3 grid(po_grid(total, PO_SURF_MAXBLK)), block(PO_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (vec4) hipLaunchKernelGGL(po_merge_kernel<true>, grid, block, 0, st, prob, back, out, V, N, OH, OW, C, K, total, true);
    else hipLaunchKernelGGL(po_merge_kernel<false>, grid, block, 0, st, prob, back, out, V, N, OH, OW, C, K, total, total < 0x7fffffffL);
    return MMSEG_CHECK_LAUNCH();
}

// N * OH * OW of a member map, or -1 for a shape that the member kernels refuse (2^29 pixels or more; taken factor by factor)
static long po_member_pixels(int N, int OH, int OW) {
    if (N < 0 || OH < 1 || OW < 1) return -1;
    long pixels = N;
    for (const int f : {OH, OW}) {
        pixels *= f;
        if (pixels >= (1L << 29)) return -1;
    }
    return pixels;
}

// prob [V*N,OH,OW,C] fp32, back [V,6] fp64 (device), sum [N,OH,OW,K] and aux [N,OH,OW,2] fp32: read unless first != 0, every element
// written.  One launch; no atomics, nothing allocated or synchronised.
int mmseg_members_accumulate(const float* prob, const double* back, float* sum, float* aux, int first, int V, int N, int OH, int OW, int C,
                             int K, void* stream) {
    if (N == 0) return 0;
    const long pixels = po_member_pixels(N, OH, OW);
    if (!prob || !back || !sum || !aux || prob == sum || prob == aux || sum == aux || pixels < 0 || V < 1 || V > MV_MAXVIEWS || C < 1 ||
        K < 1 || K > C || K > PO_MAXVALUES || (long)sizeof(float) * pixels * V >= 0x80000000L ||
        (long)sizeof(float) * pixels * V * C >= 0x80000000L)          // bytes of prob; the first product bounds the second below 2^62
        return (int)hipErrorInvalidValue;
    const bool vec4 = K == 4 && (C & 3) == 0 && ((uintptr_t)prob & 15) == 0 && ((uintptr_t)sum & 15) == 0;
    const dim3 grid(po_grid(pixels, PO_SURF_MAXBLK)), block(PO_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (vec4) hipLaunchKernelGGL(po_members_kernel<true>, grid, block, 0, st, prob, back, sum, aux, first, V, N, OH, OW, C, K, (int)pixels);
    else hipLaunchKernelGGL(po_members_kernel<false>, grid, block, 0, st, prob, back, sum, aux, first, V, N, OH, OW, C, K, (int)pixels);
    return MMSEG_CHECK_LAUNCH();
}

// sum [N,OH,OW,K] -> the mean map, aux [N,OH,OW,2] -> (H, I), in place.  One launch.
int mmseg_members_finish(float* sum, float* aux, int N, int OH, int OW, int K, void* stream) {
    if (N == 0) return 0;
    const long pixels = po_member_pixels(N, OH, OW);
    if (!sum || !aux || sum == aux || pixels < 0 || K < 1 || K > PO_MAXVALUES) return (int)hipErrorInvalidValue;
    const bool vec4 = K == 4 && ((uintptr_t)sum & 15) == 0;
    const float inv = (float)(1.0 / log((double)(K + 1)));
    const dim3 grid(po_grid(pixels, PO_SURF_MAXBLK)), block(PO_BLOCK);
    const hipStream_t st = (hipStream_t)stream;
    if (vec4) hipLaunchKernelGGL(po_members_finish_kernel<true>, grid, block, 0, st, sum, aux, K, inv, (int)pixels);
    else hipLaunchKernelGGL(po_members_finish_kernel<false>, grid, block, 0, st, sum, aux, K, inv, (int)pixels);
    return MMSEG_CHECK_LAUNCH();
}

// planes [S,OH,OW,U] fp32, out [S,H,W] uint8: every byte is written
int mmseg_restore_map(const float* planes, unsigned char* out, int S, int H, int W, int RH, int RW, int OH, int OW, int lo_r, int kept_r,
                      int before_r, int lo_c, int kept_c, int before_c, int U, int u, int order, void* stream) {
    if (S <= 0) return 0;
    if (!planes || !out || !po_geometry_ok(S, H, W, RH, RW, OH, OW) || U < 1 || U > UE_MAXPLANES || u < 0 || u >= U ||
        (order != 0 && order != 1) || !po_axis_ok(lo_r, kept_r, before_r, RH, OH) || !po_axis_ok(lo_c, kept_c, before_c, RW, OW))
        return (int)hipErrorInvalidValue;
    const bool pack = (W & 3) == 0 && ((uintptr_t)out & 3) == 0;
    const dim3 grid(po_grid(pack ? (long)H * (W >> 2) : (long)H * W, PO_MAXBLK), S), block(PO_BLOCK);
    const po_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    const double ry = (double)RH / (double)H, rx = (double)RW / (double)W;
    const hipStream_t st = (hipStream_t)stream;
    if (pack) hipLaunchKernelGGL(po_restore_map_kernel<true>, grid, block, 0, st, planes, out, H, W, RH, RW, ry, rx, OH, OW, ar, ac, U, u, order);
    else hipLaunchKernelGGL(po_restore_map_kernel<false>, grid, block, 0, st, planes, out, H, W, RH, RW, ry, rx, OH, OW, ar, ac, U, u, order);
    return MMSEG_CHECK_LAUNCH();
}

static bool po_calibration_ok(int S, int H, int W, int RH, int RW, int OH, int OW, int C, int K, int B) {
    return S >= 1 && po_geometry_ok(S, H, W, RH, RW, OH, OW) && (long)S * H * W < 0x7fffffffL && C >= 1 && K >= 1 && K <= C &&
           K <= PO_MAXVALUES && B >= 2 && B <= CT_MAXBINS;
}

// bytes of ws for mmseg_calibration_table: one partial [K][B+2] fp64 table per block; 0 for arguments that it would refuse
long mmseg_calibration_table_workspace_bytes(int S, int H, int W, int K, int B) {
    if (!po_calibration_ok(S, H, W, 1, 1, 1, 1, K, K, B)) return 0;
    return (long)sizeof(double) * po_grid((long)S * H * W, CT_MAXBLK) * K * (B + 2);
}

// prob [S,OH,OW,C] fp32, truth [S,H,W] uint8, values [K] int32 (device) -> bins [K,B,2] int32 (zeroed here, on the stream), sums [K,B+2]
// fp64, every element written.  ws: mmseg_calibration_table_workspace_bytes bytes.  One memset and two launches.
int mmseg_calibration_table(const float* prob, const unsigned char* truth, const int* values, int* bins, double* sums, double* ws, int S,
                            int H, int W, int RH, int RW, int OH, int OW, int lo_r, int kept_r, int before_r, int lo_c, int kept_c,
                            int before_c, int C, int K, int B, int order, void* stream) {
    if (S == 0) return 0;
    if (!prob || !truth || !values || !bins || !sums || !ws || !po_calibration_ok(S, H, W, RH, RW, OH, OW, C, K, B) ||
        (order != 0 && order != 1) || !po_axis_ok(lo_r, kept_r, before_r, RH, OH) || !po_axis_ok(lo_c, kept_c, before_c, RW, OW))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t rc = hipMemsetAsync(bins, 0, sizeof(int) * 2 * (size_t)K * B, st);
    if (rc != hipSuccess) return (int)rc;
    const long n = (long)S * H * W;
    const int nblk = (int)po_grid(n, CT_MAXBLK), entries = K * (B + 2);
    const po_axis ar = {lo_r, kept_r, before_r}, ac = {lo_c, kept_c, before_c};
    double* part = ws;
    hipLaunchKernelGGL(po_calibration_kernel, dim3(nblk), dim3(PO_BLOCK), (size_t)K * PO_BLOCK * 9, st, prob, truth, values, bins, part, n, H,
                       W, RH, RW, (double)RH / (double)H, (double)RW / (double)W, OH, OW, ar, ac, C, K, B, order);
    hipLaunchKernelGGL(po_calibration_final_kernel, dim3((entries + PO_BLOCK - 1) / PO_BLOCK), dim3(PO_BLOCK), 0, st, part, nblk, entries,
                       sums);
    return MMSEG_CHECK_LAUNCH();
}

// pred, truth [n] uint8, levels [U,n] uint8 -> out [2,1+U] int64 (zeroed here, on the stream): per row (pred == truth, pred != truth) the
// number of pixels and the sum of every plane's levels over them
int mmseg_uncertainty_by_error(const unsigned char* pred, const unsigned char* truth, const unsigned char* levels, long long* out, long n,
                               int U, void* stream) {
    if (n == 0) return 0;
    if (!pred || !truth || !levels || !out || n < 0 || n >= 0x7fffffffL || U < 1 || U > UE_MAXPLANES) return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const hipError_t rc = hipMemsetAsync(out, 0, sizeof(long long) * 2 * (size_t)(1 + U), st);
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(po_uncertainty_error_kernel, dim3(po_grid(n, PO_MAXBLK)), dim3(PO_BLOCK), 0, st, pred, truth, levels,
                       reinterpret_cast<unsigned long long*>(out), n, U);
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
    const dim3 grid(po_grid(n, PO_MAXBLK), S);
    hipLaunchKernelGGL(po_overlap_kernel, grid, dim3(PO_BLOCK), 0, (hipStream_t)stream, pred, truth, values, K, counts, n);
    return MMSEG_CHECK_LAUNCH();
}

// label [S,H,W] uint8, values [K] int32 (device) -> surf [K+1,S,H,W] uint8 0 / 1, every byte written; counts [K+1][2] int32 =
// (|foreground|, |surface|) per problem, zeroed here on the stream, or null
int mmseg_label_surface(const unsigned char* label, const int* values, unsigned char* surf, int* counts, int S, int H, int W, int K,
                        void* stream) {
    if (S <= 0) return 0;
    if (!label || !values || !surf || !po_problem_ok(S, H, W, K)) return (int)hipErrorInvalidValue;
    return po_surface(label, values, surf, counts, S, H, W, K, (hipStream_t)stream);
}

// sites [S,H,W] uint8 -> out [S,H,W] fp64: mm to the nearest non-zero voxel (+inf without one); tmp: S * H * W doubles of scratch
int mmseg_distance_to_sites(const unsigned char* sites, double* out, double* tmp, int S, int H, int W, double dz, double dy, double dx,
                            void* stream) {
    if (S <= 0) return 0;
    if (!sites || !out || !tmp || !po_volume_ok(S, H, W) || !po_spacings_ok(dz, dy, dx)) return (int)hipErrorInvalidValue;
    return po_edt(sites, out, tmp, S, H, W, dz, dy, dx, (hipStream_t)stream);
}

// doubles of workspace of mmseg_surface_metrics: two distance maps, the partials, the counts and the 2 (K + 1) surface volumes
long mmseg_surface_metrics_workspace_doubles(int S, int H, int W, int K) {
    if (S <= 0 || !po_problem_ok(S, H, W, K)) return 0;
    return po_walk_carve(nullptr, (long)S * H * W, K, false, nullptr);
}

// pred, truth [S,H,W] uint8 -> table [K+1,6] fp64 = nP, nT, |surface(P)|, |surface(T)|, sum and max of the surface distances in mm
// (nan when either surface is empty)
int mmseg_surface_metrics(const unsigned char* pred, const unsigned char* truth, const int* values, double* table, double* ws, int S,
                          int H, int W, int K, double dz, double dy, double dx, void* stream) {
    if (S <= 0) return 0;
    if (!pred || !truth || !values || !table || !ws || !po_problem_ok(S, H, W, K) || !po_spacings_ok(dz, dy, dx))
        return (int)hipErrorInvalidValue;
    return po_surface_walk(pred, truth, values, table, ws, S, H, W, K, dz, dy, dx, 6, nullptr, (hipStream_t)stream);
}

// doubles of workspace of mmseg_masked_select: the list (2 n) and the selection's state; 0 for an n that it would refuse
long mmseg_masked_select_workspace_doubles(long n) {
    if (n < 0 || n >= 0x80000000L) return 0;
    return 2 * n + OS_STATE_DOUBLES;
}

// a, b [n] fp64 (finite, >= 0), ma, mb [n] uint8 -> out [5] = N, |{x <= tolerance}|, the percentile (numpy's linear rule), D_(lo), D_(hi)
// over {a[e] : ma[e] != 0} + {b[e] : mb[e] != 0}; the last three nan when N == 0.  No host synchronisation, allocation or copy.
int mmseg_masked_select(const double* a, const unsigned char* ma, const double* b, const unsigned char* mb, long n, double percentile,
                        double tolerance, double* out, double* ws, void* stream) {
    if (!a || !ma || !b || !mb || !out || !ws || n < 0 || n >= 0x80000000L || !os_args_ok(percentile, tolerance))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    double* list = ws;
    double* state = ws + 2 * n;
    const int rc = os_reset(state, st);
    if (rc) return rc;
    if (n > 0) {
        os_append(a, ma, n, tolerance, list, state, st);
        os_append(b, mb, n, tolerance, list, state, st);
        os_select(list, state, 2 * n, percentile, st);
    }
    hipLaunchKernelGGL(os_out_kernel, dim3(1), dim3(64), 0, st, reinterpret_cast<const os_state*>(state), out);
    return MMSEG_CHECK_LAUNCH();
}

// doubles of workspace of mmseg_surface_scores: that of mmseg_surface_metrics, then the list (2 S H W) and the selection's state
long mmseg_surface_scores_workspace_doubles(int S, int H, int W, int K) {
    if (S <= 0 || !po_problem_ok(S, H, W, K)) return 0;
    return po_walk_carve(nullptr, (long)S * H * W, K, true, nullptr);
}

// pred, truth [S,H,W] uint8 -> table [K+1,8] fp64: the six columns of mmseg_surface_metrics, |{x <= tolerance}| and the percentile of the
// surface distances of both directions together (nan when either surface is empty)
int mmseg_surface_scores(const unsigned char* pred, const unsigned char* truth, const int* values, double* table, double* ws, int S,
                         int H, int W, int K, double dz, double dy, double dx, double percentile, double tolerance, void* stream) {
    if (S <= 0) return 0;
    if (!pred || !truth || !values || !table || !ws || !po_problem_ok(S, H, W, K) || !po_spacings_ok(dz, dy, dx) ||
        !os_args_ok(percentile, tolerance))
        return (int)hipErrorInvalidValue;
    const os_args robust = {percentile, tolerance};
    return po_surface_walk(pred, truth, values, table, ws, S, H, W, K, dz, dy, dx, 8, &robust, (hipStream_t)stream);
}

// label [S,H,W] uint8, values [K] int32 (device) -> comp [S,H,W] int32, every element written: 0 where the grey value is none of
// `values`, else 1 + the smallest linear index of the voxel's component (same grey value, joined through 6 or 26 neighbours)
int mmseg_label_components(const unsigned char* label, const int* values, int* comp, int S, int H, int W, int K, int connectivity,
                           void* stream) {
    if (S <= 0) return 0;
    if (!label || !values || !comp || !po_cc_args_ok(S, H, W, K, connectivity)) return (int)hipErrorInvalidValue;
    return po_components(label, values, comp, S, H, W, K, connectivity, (hipStream_t)stream);
}

// bytes of workspace of mmseg_keep_largest_components: the K <= 16 winner keys, then the sizes and the components of the n voxels
long mmseg_keep_largest_workspace_bytes(int S, int H, int W, int K) {
    if (S <= 0 || !po_cc_args_ok(S, H, W, K, 6)) return 0;
    return (long)sizeof(unsigned long long) * PO_MAXVALUES + 2 * (long)sizeof(int) * S * H * W;
}

// out [S,H,W] uint8 = label with every organ voxel outside its organ's largest component set to 0; stats [K,3] int32 = (components,
// voxels before, voxels kept).  ws: mmseg_keep_largest_workspace_bytes(S, H, W, K) bytes, 8-byte aligned
int mmseg_keep_largest_components(const unsigned char* label, const int* values, unsigned char* out, int* stats, int* ws, int S, int H,
                                  int W, int K, int connectivity, void* stream) {
    if (S <= 0) return 0;
    if (!label || !values || !out || !stats || !ws || !po_cc_args_ok(S, H, W, K, connectivity))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const long n = (long)S * H * W;
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(ws);
    int* size = reinterpret_cast<int*>(keys + PO_MAXVALUES);
    int* comp = size + n;
    hipError_t rc = hipMemsetAsync(ws, 0, sizeof(unsigned long long) * PO_MAXVALUES + sizeof(int) * (size_t)n, st);          // keys and sizes
    if (rc != hipSuccess) return (int)rc;
    rc = hipMemsetAsync(stats, 0, sizeof(int) * 3 * (size_t)K, st);
    if (rc != hipSuccess) return (int)rc;
    const int err = po_components(label, values, comp, S, H, W, K, connectivity, st);
    if (err) return err;
    const dim3 grid(po_grid(n, CC_MAXBLK)), block(PO_BLOCK);
    hipLaunchKernelGGL(po_cc_size_kernel, grid, block, 0, st, comp, size, n);
    hipLaunchKernelGGL(po_cc_winner_kernel, grid, block, 0, st, label, values, K, comp, size, keys, stats, n);
    hipLaunchKernelGGL(po_cc_keep_kernel, grid, block, 0, st, label, values, K, comp, keys, out, stats, n);
    return MMSEG_CHECK_LAUNCH();
}

// bytes of workspace of mmseg_fill_label_holes: the parents of the n voxels and one byte each for the border marks
long mmseg_fill_label_holes_workspace_bytes(int S, int H, int W, int K) {
    if (S <= 0 || !po_fh_args_ok(S, H, W, K, 0)) return 0;
    return po_fh_workspace_bytes((long)S * H * W);
}

// out [S,H,W] uint8 = label with the zeros that an organ encloses set to that organ's grey value (faces only; per_slice: every slice on
// its own); stats [K,3] int32 = (holes, voxels of values[k] before, voxels added).  ws: mmseg_fill_label_holes_workspace_bytes(S, H, W, K)
// bytes, 4-byte aligned.  Four launches and one memset per organ, all on the stream.
int mmseg_fill_label_holes(const unsigned char* label, const int* values, unsigned char* out, int* stats, void* ws, int S, int H, int W,
                           int K, int per_slice, void* stream) {
    if (S <= 0) return 0;
    if (!label || !values || !out || !stats || !ws || label == out || !po_fh_args_ok(S, H, W, K, per_slice))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const long n = (long)S * H * W;
    int* comp = reinterpret_cast<int*>(ws);
    unsigned char* mark = reinterpret_cast<unsigned char*>(comp + n);
    hipError_t rc = hipMemsetAsync(stats, 0, sizeof(int) * 3 * (size_t)K, st);
    if (rc != hipSuccess) return (int)rc;
    const int ntx = (W + CC_TX - 1) / CC_TX, nty = (H + CC_TY - 1) / CC_TY, ntz = (S + CC_TZ - 1) / CC_TZ;
    const int nnb = per_slice ? 2 : 3;
    const dim3 tiles((unsigned)((long)ntx * nty * ntz)), grid(po_grid(n, CC_MAXBLK)), block(PO_BLOCK);
    const dim3 few(po_grid(n, PO_SURF_MAXBLK));          // the fill pass: every block ends with three atomics on the same three counters
    for (int k = 0; k < K; ++k) {
        rc = hipMemsetAsync(mark, 0, (size_t)n, st);
        if (rc != hipSuccess) return (int)rc;
        hipLaunchKernelGGL(po_cc_local_kernel<true>, tiles, block, 0, st, label, values, k, comp, S, H, W, ntx, nty, nnb);
        hipLaunchKernelGGL(po_cc_merge_kernel<true>, grid, block, 0, st, label, comp, S, H, W, nnb);
        hipLaunchKernelGGL(po_fh_flatten_kernel, grid, block, 0, st, comp, mark, S, H, W, per_slice);
        if (k == 0) hipLaunchKernelGGL(po_fh_fill_kernel<true>, few, block, 0, st, label, values, k, comp, mark, out, stats, n);
        else hipLaunchKernelGGL(po_fh_fill_kernel<false>, few, block, 0, st, label, values, k, comp, mark, out, stats, n);
    }
    return MMSEG_CHECK_LAUNCH();
}

// bytes of workspace of mmseg_smooth_label: the row table of the ball, then three bytes per voxel (the runs along x, the mask of the
// pass before, and the opened volume that `smooth` closes)
long mmseg_smooth_label_workspace_bytes(int S, int H, int W, int K) {
    if (S <= 0 || !po_problem_ok(S, H, W, K)) return 0;
    return MO_TABLE_BYTES + 3 * (long)S * H * W;
}

// out [S,H,W] uint8 = label opened (op 0), closed (1) or opened and then closed (2) by the ball of `radius` mm on the grid of spacings
// (dz, dy, dx), organ by organ; per_slice: the ball lies in the slice and dz is not read.  stats [K,3] int32 = (voxels of values[k] in
// label, removed, added).  ws: mmseg_smooth_label_workspace_bytes(S, H, W, K) bytes.  Per organ and opening or closing two passes over the
// rows of the ball, each after one map of runs along x unless the ball is one voxel wide there; all on the stream.
int mmseg_smooth_label(const unsigned char* label, const int* values, unsigned char* out, int* stats, void* ws, int S, int H, int W, int K,
                       double dz, double dy, double dx, double radius, int op, int per_slice, void* stream) {
    if (S <= 0) return 0;
    mo_plan p;
    if (!label || !values || !out || !stats || !ws || label == out || !mo_args_ok(S, H, W, K, dz, dy, dx, radius, op, per_slice, &p))
        return (int)hipErrorInvalidValue;
    const hipStream_t st = (hipStream_t)stream;
    const long n = (long)S * H * W;
    signed char* table = reinterpret_cast<signed char*>(ws);
    unsigned char* run = reinterpret_cast<unsigned char*>(ws) + MO_TABLE_BYTES;
    unsigned char *mask = run + n, *opened = mask + n;
    hipError_t rc = hipMemsetAsync(stats, 0, sizeof(int) * 3 * (size_t)K, st);
    if (rc != hipSuccess) return (int)rc;
    hipLaunchKernelGGL(po_mo_table_kernel, dim3(1), dim3(PO_BLOCK), 0, st, table, dz, dy, dx, p.r2, p.rz, p.ry, p.rx, per_slice);
    if (op == 2) {
        mo_apply(false, label, values, opened, stats, table, run, mask, S, H, W, K, p, 1, st);
        mo_apply(true, opened, values, out, stats, table, run, mask, S, H, W, K, p, 0, st);
    } else {
        mo_apply(op == 1, label, values, out, stats, table, run, mask, S, H, W, K, p, 1, st);
    }
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
