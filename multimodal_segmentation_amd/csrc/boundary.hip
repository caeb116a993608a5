// Boundary loss (Kervadec et al., MIDL 2019) for the segmentor: the signed distance map of every ground-truth mask, built on the
// device from the batch as it is trained on, and the term L_B = mean(p * phi) with its gradient.  BUILD-DEFINED: the reference has
// no distance in its losses.
//
//   phi(q) =  d_fg(q)           q background      d_fg / d_bg: Euclidean distance in pixels to the nearest foreground / background
//   phi(q) = -(d_bg(q) - 1)     q foreground      pixel of the same sample and channel; the image edge is not background
//   phi    =  0 everywhere      the mask is empty or full
//
// (one_hot2dist of the paper's code over scipy.ndimage.distance_transform_edt).  Exact: squared distances are int32, minimised
// separably (row pass, then column pass), one correctly rounded sqrtf at the end.  H, W <= 2048 keeps H^2 + W^2 < 2^24.
//
// Layout.  The intermediate ws [B][H][W][nm] uint32 has the layout of phi: the low half of a word is the distance along the row to
// the nearest foreground pixel of that row, the high half the distance to the nearest background pixel (0xFFFF: the row has none).
//   row pass    one block per (b, h): the NHWC row of the target is read once, coalesced, and thresholded into LDS [k][x]; a wave takes
//               a channel, a lane an odd-length run of pixels (odd: the 32 lanes of a half wave fall on 32 different banks), the runs are
//               joined by a prefix maximum / suffix minimum over the lanes; the words leave LDS in NHWC order, coalesced.
//   column pass one block per (b, tile of TX columns, all nm channels): the tile [H][TX * nm] words is staged in LDS (every row of it is
//               one contiguous piece of ws); a thread owns an element, reads its own class from its word, and walks outward from its row
//               over the OTHER class's half only, until d^2 alone cannot improve the minimum.  Neighbouring lanes hold neighbouring
//               words of one row: no bank conflict in the walk, and the store of phi is contiguous over x and k.
#include "common.hpp"

#define BND_MAXC 8            // SEG_MAXC of loss.hip
#define BND_MAXHW 2048
#define BND_CHUNKS 128
#define BND_NONE 0xFFFFu
#define BND_INFSQ 0x7FFFFFFF
#define BND_TILE_WORDS 8192   // LDS words of a column tile (32 KiB) unless one column of all channels needs more (at most 64 KiB)
#define BND_FILL_BLOCKS 1024  // blocks of the column pass that fill the device: 4 per CU

__device__ __forceinline__ int wave_prefix_max_excl(int v, int lane, int none) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(v, o, 64); if (lane >= o) v = max(v, t); }
    const int e = __shfl_up(v, 1, 64);
    return lane == 0 ? none : e;
}
__device__ __forceinline__ int wave_suffix_min_excl(int v, int lane, int none) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_down(v, o, 64); if (lane + o < 64) v = min(v, t); }
    const int e = __shfl_down(v, 1, 64);
    return lane == 63 ? none : e;
}

// grid B * H, block 256, LDS nm * W words
__global__ __launch_bounds__(256) void boundary_row_kernel(const float* __restrict__ target, unsigned* __restrict__ ws, int H, int W, int C, int nm) {
    extern __shared__ unsigned bnd_lds[];
    const size_t row = blockIdx.x;                       // b * H + h
    const float* t = target + row * (size_t)W * C;
    for (int e = threadIdx.x; e < W * C; e += 256) {
        const int c = e % C, x = e / C;
        if (c < nm) bnd_lds[c * W + x] = t[e] > 0.5f ? 1u : 0u;
    }
    __syncthreads();
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int seg = ((W + 63) >> 6) | 1;
    const int x0 = min(W, lane * seg), x1 = min(W, x0 + seg);
    const int FAR = 1 << 20;
    for (int k = wid; k < nm; k += 4) {
        unsigned* a = bnd_lds + k * W;
        int lastF = -1, lastB = -1, firstF = FAR, firstB = FAR;
        for (int x = x0; x < x1; ++x) {
            if (a[x]) { lastF = x; firstF = min(firstF, x); } else { lastB = x; firstB = min(firstB, x); }
        }
        int lf = wave_prefix_max_excl(lastF, lane, -1), lb = wave_prefix_max_excl(lastB, lane, -1);
        int nf = wave_suffix_min_excl(firstF, lane, FAR), nb = wave_suffix_min_excl(firstB, lane, FAR);
        // left to right: bit 0 keeps the class, the rest the distance to the nearest pixel of the other class on the left
        for (int x = x0; x < x1; ++x) {
            const unsigned m = a[x];
            if (m) lf = x; else lb = x;
            const int o = m ? lb : lf;
            a[x] = m | ((o < 0 ? BND_NONE : (unsigned)(x - o)) << 1);
        }
        for (int x = x1 - 1; x >= x0; --x) {
            const unsigned v = a[x], m = v & 1u;
            if (m) nf = x; else nb = x;
            const int o = m ? nb : nf;
            const unsigned d = min(v >> 1, o >= FAR ? BND_NONE : (unsigned)(o - x));
            a[x] = m ? (d << 16) : d;                    // own class: 0
        }
    }
    __syncthreads();
    unsigned* o = ws + row * (size_t)W * nm;
    for (int e = threadIdx.x; e < W * nm; e += 256) o[e] = bnd_lds[(e % nm) * W + e / nm];
}

// grid (ceil(W / TX), B), block 256, LDS H * TX * nm words
__global__ __launch_bounds__(256) void boundary_col_kernel(const unsigned* __restrict__ ws, float* __restrict__ phi, int H, int W, int nm, int TX) {
    extern __shared__ unsigned bnd_lds[];
    const int b = blockIdx.y, x0 = blockIdx.x * TX;
    const int L = min(TX, W - x0) * nm;                  // words of one tile row
    const size_t base = ((size_t)b * H * W + x0) * nm, pitch = (size_t)W * nm;
    const int n = H * L;
    for (int e = threadIdx.x; e < n; e += 256) { const int i = e / L; bnd_lds[e] = ws[base + i * pitch + (e - i * L)]; }
    __syncthreads();
    for (int e = threadIdx.x; e < n; e += 256) {
        const int i = e / L;
        const unsigned v = bnd_lds[e];
        const bool fg = (v & 0xFFFFu) == 0u;
        const int sh = fg ? 16 : 0;
        const unsigned g = (v >> sh) & 0xFFFFu;
        int best = g == BND_NONE ? BND_INFSQ : (int)(g * g);
        for (int d = 1; d < H; ++d) {
            const int dd = d * d;
            if (dd >= best) break;
            const bool up = i - d >= 0, dn = i + d < H;
            if (!up && !dn) break;
            if (up) {
                const unsigned q = (bnd_lds[e - d * L] >> sh) & 0xFFFFu;
                if (q != BND_NONE) best = min(best, dd + (int)(q * q));
            }
            if (dn) {
                const unsigned q = (bnd_lds[e + d * L] >> sh) & 0xFFFFu;
                if (q != BND_NONE) best = min(best, dd + (int)(q * q));
            }
        }
        float r = 0.f;                                   // no pixel of the other class anywhere: the mask is empty or full
        if (best != BND_INFSQ) {
            r = sqrtf((float)best);
            if (fg) r = -(r - 1.f);
        }
        phi[base + i * pitch + (e - i * L)] = r;
    }
}

// part[b][chunk] = sum over the chunk's pixels and k < nm of pred * phi (one fused multiply-add per element, fixed order)
__global__ __launch_bounds__(256) void boundary_partial_kernel(const float* __restrict__ pred, const float* __restrict__ phi, float* __restrict__ part,
                                                               long HW, int C, int nm) {
    __shared__ float red[17];
    const int b = blockIdx.y;
    const long per = (HW + BND_CHUNKS - 1) / BND_CHUNKS;
    const long p0 = (long)blockIdx.x * per, p1 = min(HW, p0 + per);
    float a = 0.f;
    for (long px = p0 + threadIdx.x; px < p1; px += 256) {
        const float* p = pred + ((size_t)b * HW + px) * C;
        const float* f = phi + ((size_t)b * HW + px) * nm;
        for (int k = 0; k < nm; ++k) a = __fmaf_rn(p[k], f[k], a);
    }
    a = block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)b * BND_CHUNKS + blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void boundary_final_kernel(const float* __restrict__ part, int npart, float count, float* __restrict__ loss_b) {
    __shared__ float red[17];
    float a = 0.f;
    for (int i = threadIdx.x; i < npart; i += 256) a += part[i];
    a = block_sum(a, red);
    if (threadIdx.x == 0) loss_b[0] = a / count;
}
// dpred[b,px,k] += s * phi[b,px,k], s = ((scale_host * scale_dev[0]) * weight_dev[0]) / count, k < nm.  Every step is rounded on its own
// (no contraction into fused multiply-adds: the product s * phi is the same number whatever it is added to)
__global__ void boundary_grad_add_kernel(const float* __restrict__ phi, float* __restrict__ dpred, long n, int C, int nm, float scale_host,
                                         const float* __restrict__ scale_dev, const float* __restrict__ weight_dev, float count) {
#pragma clang fp contract(off)
    float s = scale_host;
    if (scale_dev) s = s * scale_dev[0];
    s = (s * weight_dev[0]) / count;
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long px = i / nm; const int k = (int)(i - px * nm);
        float* d = dpred + px * C + k;
        const float g = s * phi[i];
        *d = *d + g;
    }
}
__global__ void boundary_combine_kernel(float* __restrict__ loss, const float* __restrict__ loss_b, const float* __restrict__ weight_dev) {
#pragma clang fp contract(off)
    if (threadIdx.x == 0 && blockIdx.x == 0) { const float t = weight_dev[0] * loss_b[0]; loss[0] = loss[0] + t; }
}

static inline bool bnd_shape_ok(int B, int H, int W, int nm) {
    return B >= 1 && B <= 65535 && H >= 1 && W >= 1 && H <= BND_MAXHW && W <= BND_MAXHW && nm >= 1 && nm <= BND_MAXC;
}
// Columns of a tile of the column pass.  The walk is latency-bound and its length varies from tile to tile, so many small blocks beat few
// large ones: about BND_FILL_BLOCKS blocks when the batch is large enough, but rows of at least 4 words (16 B pieces of ws), and never
// more than the LDS budget holds.  (8 x 256 x 256 x 4 channels with 8-column tiles, one block per CU: 955 us; with 2-column tiles: see
// DESIGN.md.)
static inline int bnd_tile_cols(int B, int H, int W, int nm) {
    int tx = (int)(((long)B * W) / BND_FILL_BLOCKS);
    if (tx * nm < 4) tx = (4 + nm - 1) / nm;
    if (tx > BND_TILE_WORDS / (H * nm)) tx = BND_TILE_WORDS / (H * nm);
    if (tx < 1) tx = 1;
    if (tx > W) tx = W;
    return tx;
}

extern "C" {

long mmseg_boundary_workspace_bytes(int B, int H, int W, int nm) {
    if (!bnd_shape_ok(B, H, W, nm)) return 0;
    return (long)B * H * W * nm * 4;
}
int mmseg_boundary_map(const float* target, float* phi, int* ws, int B, int H, int W, int C, int nm, void* stream) {
    if (target == nullptr || phi == nullptr || ws == nullptr || !bnd_shape_ok(B, H, W, nm) || nm > C || C > BND_MAXC) return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(boundary_row_kernel, dim3(B * H), dim3(256), (size_t)nm * W * 4, st, target, (unsigned*)ws, H, W, C, nm);
    const int tx = bnd_tile_cols(B, H, W, nm);
    hipLaunchKernelGGL(boundary_col_kernel, dim3((W + tx - 1) / tx, B), dim3(256), (size_t)H * tx * nm * 4, st, (const unsigned*)ws, phi, H, W, nm, tx);
    return MMSEG_CHECK_LAUNCH();
}
int mmseg_boundary_loss_workspace_floats(int B) { return B >= 1 && B <= 65535 ? B * BND_CHUNKS : 0; }
int mmseg_boundary_loss(const float* pred, const float* phi, float* loss_b, float* ws, int B, long HW, int C, int nm, void* stream) {
    if (pred == nullptr || phi == nullptr || loss_b == nullptr || ws == nullptr || B < 1 || B > 65535 || HW < 1 || nm < 1 || nm > C || C > BND_MAXC)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(boundary_partial_kernel, dim3(BND_CHUNKS, B), dim3(256), 0, st, pred, phi, ws, HW, C, nm);
    hipLaunchKernelGGL(boundary_final_kernel, dim3(1), dim3(256), 0, st, (const float*)ws, B * BND_CHUNKS, (float)((double)B * HW * nm), loss_b);
    return MMSEG_CHECK_LAUNCH();
}
int mmseg_boundary_grad_add(const float* phi, float* dpred, int B, long HW, int C, int nm, float scale_host, const float* scale_dev,
                            const float* weight_dev, void* stream) {
    if (phi == nullptr || dpred == nullptr || weight_dev == nullptr || B < 1 || HW < 1 || nm < 1 || nm > C || C > BND_MAXC)
        return (int)hipErrorInvalidValue;
    const long n = (long)B * HW * nm;
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(boundary_grad_add_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, phi, dpred, n, C, nm, scale_host, scale_dev,
                       weight_dev, (float)((double)B * HW * nm));
    return MMSEG_CHECK_LAUNCH();
}
int mmseg_boundary_combine(float* loss, const float* loss_b, const float* weight_dev, void* stream) {
    if (loss == nullptr || loss_b == nullptr || weight_dev == nullptr) return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(boundary_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, loss, loss_b, weight_dev);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
