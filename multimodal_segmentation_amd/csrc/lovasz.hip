// Lovasz-Softmax loss (Berman et al., CVPR 2018) for the segmentor, per image and over the organ channels: the convex surrogate of the
// Jaccard index.  BUILD-DEFINED: the reference's losses hold no sort.  Per sample b and channel k < nm, over the P = HW pixels:
//
//   y_i = target > 0.5,  e_i = fabsf(y_i - p_i) (fp32, one subtraction);  order: e descending, equal e by pixel index ascending;
//   G = sum y;  for the pixel at a sorted position, c / n = positives / negatives strictly before it;
//   g = 1 / (G + n)                              y = 1
//   g = (G - c) / ((G + n) (G + n + 1))          y = 0, G > 0
//   g = 1 at the first position, 0 elsewhere     G = 0
//   m[b,i,k] = s_i g_i q_b,  s = +1 (y = 0) / -1 (y = 1),  m = 0 where e_i == 0,  q_b = 1 / (B |K_b|), K_b the classes with G > 0
//   ('present') or all nm classes ('all'); m = 0 for a class outside K_b.      L = sum m (p - y),   dL/dp = m.
//
// Layout.  A segment is one (b, k): S = B * nm segments of HW records.  A record is one 64-bit word [~key : 32 | pixel : 22 + label : 1],
// key the bit pattern of e (e >= 0: its order as uint32 is the order of e), inverted so that an ascending sort is e descending.  A
// least-significant-digit radix sort over the four bytes of the key, every pass stable, so equal keys stay in pixel order:
//   build    one block per (tile of LV_TILE pixels, b): thresholds, subtracts, writes the nm record streams and the per-block histograms
//            of the lowest byte (integer LDS atomics)
//   scan     one block per segment, thread = digit: exclusive scan over (digit, block) of hist [segment][block][digit], in place
//   scatter  one block per (segment, tile): a wave takes LV_ITEMS consecutive rows of 64 records; per row the lanes that hold the same
//            digit find each other with 8 wave-wide ballots, the lowest of them bumps the wave's counter of that digit in LDS, the rank
//            is the counter before + the number of lower matching lanes; then wave counters are prefixed over the 4 waves and
//            added to the block's base of the digit
//   hist     the per-block histogram of the next byte, on the new arrangement
//   count    positives per tile of the sorted order;  final: a block sums the counts of the tiles before it (c of its first record)
//            and of every tile of the nm segments of its sample (G, |K_b|), scans the label bit over its tile, evaluates g in fp64
//            from the integers, multiplies by q_b, rounds to fp32 once and writes the pixel's own place: each (b, i, k) once.
// Every grid is a function of (B, HW, nm); no float atomics; non-finite predictions are just other bit patterns to sort.
#include "common.hpp"

#define LV_MAXC 8                 // SEG_MAXC of loss.hip
#define LV_MAXHW (1L << 22)       // 22 bits of pixel index in a record
#define LV_ITEMS 8                // rows of 64 records per wave
#define LV_WAVE (64 * LV_ITEMS)   // records of a wave: 512
#define LV_TILE (4 * LV_WAVE)     // records of a block: 2048
#define LV_CHUNKS 128

typedef unsigned long long lv_rec;

__device__ __forceinline__ lv_rec lv_make(float p, float t, unsigned px) {
    const unsigned y = t > 0.5f ? 1u : 0u;
    const float e = fabsf((float)y - p);
    return ((lv_rec)(~__float_as_uint(e)) << 32) | (lv_rec)((px << 1) | y);
}

// grid (nblk, B), block 256
__global__ __launch_bounds__(256) void lovasz_build_kernel(const float* __restrict__ pred, const float* __restrict__ target, lv_rec* __restrict__ rec,
                                                           unsigned* __restrict__ hist, long HW, int C, int nm, int nblk) {
    __shared__ unsigned lh[LV_MAXC * 256];
    const int b = blockIdx.y, tile = blockIdx.x;
    for (int i = threadIdx.x; i < nm * 256; i += 256) lh[i] = 0u;
    __syncthreads();
    const long p0 = (long)tile * LV_TILE, p1 = min(HW, p0 + LV_TILE);
    for (long px = p0 + threadIdx.x; px < p1; px += 256) {
        const float* p = pred + ((size_t)b * HW + px) * C;
        const float* t = target + ((size_t)b * HW + px) * C;
        for (int k = 0; k < nm; ++k) {
            const lv_rec r = lv_make(p[k], t[k], (unsigned)px);
            rec[((size_t)b * nm + k) * HW + px] = r;
            atomicAdd(&lh[k * 256 + (int)((r >> 32) & 255u)], 1u);
        }
    }
    __syncthreads();
    for (int k = 0; k < nm; ++k) hist[(((size_t)b * nm + k) * nblk + tile) * 256 + threadIdx.x] = lh[k * 256 + threadIdx.x];
}

// grid (S, nblk), block 256
__global__ __launch_bounds__(256) void lovasz_hist_kernel(const lv_rec* __restrict__ rec, unsigned* __restrict__ hist, long HW, int nblk, int shift) {
    __shared__ unsigned lh[256];
    const size_t seg = blockIdx.x;
    const int tile = blockIdx.y;
    lh[threadIdx.x] = 0u;
    __syncthreads();
    const long p0 = (long)tile * LV_TILE, p1 = min(HW, p0 + LV_TILE);
    const lv_rec* in = rec + seg * HW;
    for (long i = p0 + threadIdx.x; i < p1; i += 256) atomicAdd(&lh[(int)((in[i] >> shift) & 255u)], 1u);
    __syncthreads();
    hist[(seg * nblk + tile) * 256 + threadIdx.x] = lh[threadIdx.x];
}

// grid S, block 256 (thread = digit): hist[seg][block][digit] -> the number of records of the segment with a lower digit, or the same
// digit in an earlier block
__global__ __launch_bounds__(256) void lovasz_scan_kernel(unsigned* __restrict__ hist, int nblk) {
    __shared__ unsigned tot[256];
    unsigned* h = hist + (size_t)blockIdx.x * nblk * 256 + threadIdx.x;
    unsigned s = 0u;
    for (int t = 0; t < nblk; ++t) s += h[(size_t)t * 256];
    tot[threadIdx.x] = s;
    __syncthreads();
    for (int o = 1; o < 256; o <<= 1) {                    // inclusive scan over the digits
        const unsigned v = threadIdx.x >= o ? tot[threadIdx.x - o] : 0u;
        __syncthreads();
        tot[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned run = tot[threadIdx.x] - s;
    for (int t = 0; t < nblk; ++t) { const unsigned v = h[(size_t)t * 256]; h[(size_t)t * 256] = run; run += v; }
}

// grid (S, nblk), block 256
__global__ __launch_bounds__(256) void lovasz_scatter_kernel(const lv_rec* __restrict__ src, lv_rec* __restrict__ dst, const unsigned* __restrict__ base,
                                                             long HW, int nblk, int shift) {
    __shared__ unsigned wh[4 * 256];
    const size_t seg = blockIdx.x;
    const int tile = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    for (int i = threadIdx.x; i < 4 * 256; i += 256) wh[i] = 0u;
    __syncthreads();
    const lv_rec* in = src + seg * HW;
    volatile unsigned* cnt = wh + wid * 256;
    const long w0 = (long)tile * LV_TILE + (long)wid * LV_WAVE;
    lv_rec r[LV_ITEMS];
    unsigned off[LV_ITEMS];
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long pos = w0 + j * 64 + lane;
        const bool valid = pos < HW;
        r[j] = valid ? in[pos] : 0ull;
        const unsigned d = (unsigned)(r[j] >> shift) & 255u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int bit = 0; bit < 8; ++bit) {
            const bool on = (d >> bit) & 1u;
            const unsigned long long bal = __ballot(on);
            peers &= on ? bal : ~bal;
        }
        if (!valid) peers = 0ull;
        const int leader = peers ? __ffsll((long long)peers) - 1 : lane;
        unsigned before = 0u;
        if (valid && lane == leader) { before = cnt[d]; cnt[d] = before + (unsigned)__popcll(peers); }
        __builtin_amdgcn_wave_barrier();
        before = __shfl(before, leader, 64);
        off[j] = before + (unsigned)__popcll(peers & ((1ull << lane) - 1ull));
    }
    __syncthreads();
    {   // thread = digit: the wave counters become block base + records of the digit in earlier waves
        unsigned run = base[(seg * nblk + tile) * 256 + threadIdx.x];
#pragma unroll
        for (int w = 0; w < 4; ++w) { const unsigned v = wh[w * 256 + threadIdx.x]; wh[w * 256 + threadIdx.x] = run; run += v; }
    }
    __syncthreads();
    lv_rec* out = dst + seg * HW;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long pos = w0 + j * 64 + lane;
        if (pos < HW) {
            const unsigned d = (unsigned)(r[j] >> shift) & 255u;
            const long to = (long)wh[wid * 256 + d] + off[j];
            if (to < HW) out[to] = r[j];                  // (always, for histograms of this arrangement)
        }
    }
}

// grid (S, nblk), block 256: positives per tile of the sorted order
__global__ __launch_bounds__(256) void lovasz_count_kernel(const lv_rec* __restrict__ rec, unsigned* __restrict__ tcnt, long HW, int nblk) {
    __shared__ unsigned tot;
    const size_t seg = blockIdx.x;
    const int tile = blockIdx.y;
    if (threadIdx.x == 0) tot = 0u;
    __syncthreads();
    const long p0 = (long)tile * LV_TILE, p1 = min(HW, p0 + LV_TILE);
    const lv_rec* in = rec + seg * HW;
    unsigned c = 0u;
    for (long i = p0 + threadIdx.x; i < p1; i += 256) c += (unsigned)(in[i] & 1ull);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if ((threadIdx.x & 63) == 0) atomicAdd(&tot, c);
    __syncthreads();
    if (threadIdx.x == 0) tcnt[seg * nblk + tile] = tot;
}

// grid (S, nblk), block 256; a thread owns LV_ITEMS consecutive records of the sorted order
__global__ __launch_bounds__(256) void lovasz_final_kernel(const lv_rec* __restrict__ rec, const unsigned* __restrict__ tcnt, float* __restrict__ m,
                                                           long HW, int nm, int nblk, int B, int classes_all) {
    __shared__ unsigned sums[LV_MAXC + 1];                 // G of the nm classes of the sample; positives before this tile
    __shared__ unsigned wtot[4];
    const size_t seg = blockIdx.x;
    const int tile = blockIdx.y, lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int b = (int)(seg / nm), k = (int)(seg - (size_t)b * nm);
    if (threadIdx.x <= LV_MAXC) sums[threadIdx.x] = 0u;
    __syncthreads();
    for (int kk = 0; kk < nm; ++kk) {
        const unsigned* tc = tcnt + ((size_t)b * nm + kk) * nblk;
        unsigned a = 0u, before = 0u;
        for (int t = threadIdx.x; t < nblk; t += 256) { const unsigned v = tc[t]; a += v; if (kk == k && t < tile) before += v; }
        for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o, 64); before += __shfl_xor(before, o, 64); }
        if (lane == 0) { atomicAdd(&sums[kk], a); if (kk == k) atomicAdd(&sums[LV_MAXC], before); }
    }
    const long p0 = (long)tile * LV_TILE + (long)threadIdx.x * LV_ITEMS;
    const lv_rec* in = rec + seg * HW;
    lv_rec r[LV_ITEMS];
    unsigned mine = 0u;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) { r[j] = p0 + j < HW ? in[p0 + j] : 0ull; mine += (unsigned)(r[j] & 1ull); }
    unsigned incl = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const unsigned t = __shfl_up(incl, o, 64); if (lane >= o) incl += t; }
    if (lane == 63) wtot[wid] = incl;
    __syncthreads();
    unsigned c = sums[LV_MAXC] + incl - mine;
    for (int w = 0; w < wid; ++w) c += wtot[w];
    const unsigned G = sums[k];
    int present = 0;
    for (int kk = 0; kk < nm; ++kk) present += sums[kk] > 0u ? 1 : 0;
    const int nk = classes_all ? nm : present;
    const double q = nk > 0 && (classes_all || G > 0u) ? 1.0 / ((double)B * (double)nk) : 0.0;     // a class outside K_b pays nothing
    float* out = m + (size_t)b * HW * nm + k;
#pragma unroll
    for (int j = 0; j < LV_ITEMS; ++j) {
        const long pos = p0 + j;
        if (pos < HW) {
            const unsigned y = (unsigned)(r[j] & 1ull);
            const unsigned px = ((unsigned)r[j] >> 1) & 0x3FFFFFu;
            const double Gn = (double)G + (double)((unsigned long long)pos - c);     // G + negatives before
            double g;
            if (G == 0u) g = pos == 0 ? 1.0 : 0.0;
            else if (y) g = 1.0 / Gn;
            else g = (double)(G - min(c, G)) / (Gn * (Gn + 1.0));
            float v = (float)((y ? -g : g) * q);
            if ((unsigned)(r[j] >> 32) == 0xFFFFFFFFu) v = 0.f;                     // e == 0
            if ((long)px < HW) out[(size_t)px * nm] = v;   // (always: a record carries its own pixel)
            c += y;
        }
    }
}

__device__ __forceinline__ double lv_block_sum(double v, double* red /* 4 doubles */) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((red[0] + red[1]) + red[2]) + red[3];
}
// part[b][chunk] = sum over the chunk's pixels and k < nm of m * (p - y), in fp64, fixed order
__global__ __launch_bounds__(256) void lovasz_partial_kernel(const float* __restrict__ pred, const float* __restrict__ target, const float* __restrict__ m,
                                                             double* __restrict__ part, long HW, int C, int nm) {
    __shared__ double red[4];
    const int b = blockIdx.y;
    const long per = (HW + LV_CHUNKS - 1) / LV_CHUNKS;
    const long p0 = (long)blockIdx.x * per, p1 = min(HW, p0 + per);
    double a = 0.0;
    for (long px = p0 + threadIdx.x; px < p1; px += 256) {
        const float* p = pred + ((size_t)b * HW + px) * C;
        const float* t = target + ((size_t)b * HW + px) * C;
        const float* f = m + ((size_t)b * HW + px) * nm;
        for (int k = 0; k < nm; ++k) a += (double)f[k] * ((double)p[k] - (t[k] > 0.5f ? 1.0 : 0.0));
    }
    a = lv_block_sum(a, red);
    if (threadIdx.x == 0) part[(size_t)b * LV_CHUNKS + blockIdx.x] = a;
}
__global__ __launch_bounds__(256) void lovasz_sum_kernel(const double* __restrict__ part, int npart, float* __restrict__ loss_l) {
    __shared__ double red[4];
    double a = 0.0;
    for (int i = threadIdx.x; i < npart; i += 256) a += part[i];
    a = lv_block_sum(a, red);
    if (threadIdx.x == 0) loss_l[0] = (float)a;
}
// dpred[b,px,k] += s * m[b,px,k], s = (scale_host * scale_dev[0]) * weight_dev[0], k < nm; every step rounded on its own
__global__ void lovasz_grad_add_kernel(const float* __restrict__ m, float* __restrict__ dpred, long n, int C, int nm, float scale_host,
                                       const float* __restrict__ scale_dev, const float* __restrict__ weight_dev) {
#pragma clang fp contract(off)
    float s = scale_host;
    if (scale_dev) s = s * scale_dev[0];
    s = s * weight_dev[0];
    for (long i = (long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long)gridDim.x * blockDim.x) {
        const long px = i / nm; const int k = (int)(i - px * nm);
        float* d = dpred + px * C + k;
        const float g = s * m[i];
        *d = *d + g;
    }
}

static inline bool lv_shape_ok(int B, long HW, int nm) { return B >= 1 && B <= 65535 && HW >= 1 && HW <= LV_MAXHW && nm >= 1 && nm <= LV_MAXC; }
static inline int lv_blocks(long HW) { return (int)((HW + LV_TILE - 1) / LV_TILE); }

extern "C" {

// [records A | records B] (8 B each), [histograms: S * nblk * 256], [tile counts: S * nblk]
long mmseg_lovasz_workspace_bytes(int B, long HW, int nm) {
    if (!lv_shape_ok(B, HW, nm)) return 0;
    const long S = (long)B * nm, nblk = lv_blocks(HW);
    return 2 * S * HW * 8 + S * nblk * 256 * 4 + S * nblk * 4;
}
int mmseg_lovasz_map(const float* pred, const float* target, float* m, int* ws, int B, long HW, int C, int nm, int classes_all, void* stream) {
    if (pred == nullptr || target == nullptr || m == nullptr || ws == nullptr || !lv_shape_ok(B, HW, nm) || nm > C || C > LV_MAXC)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    const long S = (long)B * nm;
    const int nblk = lv_blocks(HW);
    lv_rec* ra = (lv_rec*)ws;
    lv_rec* rb = ra + S * HW;
    unsigned* hist = (unsigned*)(rb + S * HW);
    unsigned* tcnt = hist + S * nblk * 256;
    const dim3 grid((unsigned)S, (unsigned)nblk);
    hipLaunchKernelGGL(lovasz_build_kernel, dim3(nblk, B), dim3(256), 0, st, pred, target, ra, hist, HW, C, nm, nblk);
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 32 + 8 * pass;
        if (pass > 0) hipLaunchKernelGGL(lovasz_hist_kernel, grid, dim3(256), 0, st, (const lv_rec*)ra, hist, HW, nblk, shift);
        hipLaunchKernelGGL(lovasz_scan_kernel, dim3((unsigned)S), dim3(256), 0, st, hist, nblk);
        hipLaunchKernelGGL(lovasz_scatter_kernel, grid, dim3(256), 0, st, (const lv_rec*)ra, rb, (const unsigned*)hist, HW, nblk, shift);
        lv_rec* t = ra; ra = rb; rb = t;
    }
    hipLaunchKernelGGL(lovasz_count_kernel, grid, dim3(256), 0, st, (const lv_rec*)ra, tcnt, HW, nblk);
    hipLaunchKernelGGL(lovasz_final_kernel, grid, dim3(256), 0, st, (const lv_rec*)ra, (const unsigned*)tcnt, m, HW, nm, nblk, B, classes_all ? 1 : 0);
    return MMSEG_CHECK_LAUNCH();
}
// B * LV_CHUNKS fp64 partials
int mmseg_lovasz_loss_workspace_floats(int B) { return B >= 1 && B <= 65535 ? 2 * B * LV_CHUNKS : 0; }
int mmseg_lovasz_loss(const float* pred, const float* target, const float* m, float* loss_l, float* ws, int B, long HW, int C, int nm, void* stream) {
    if (pred == nullptr || target == nullptr || m == nullptr || loss_l == nullptr || ws == nullptr || B < 1 || B > 65535 || HW < 1 || nm < 1 ||
        nm > C || C > LV_MAXC)
        return (int)hipErrorInvalidValue;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(lovasz_partial_kernel, dim3(LV_CHUNKS, B), dim3(256), 0, st, pred, target, m, (double*)ws, HW, C, nm);
    hipLaunchKernelGGL(lovasz_sum_kernel, dim3(1), dim3(256), 0, st, (const double*)ws, B * LV_CHUNKS, loss_l);
    return MMSEG_CHECK_LAUNCH();
}
int mmseg_lovasz_grad_add(const float* m, float* dpred, int B, long HW, int C, int nm, float scale_host, const float* scale_dev,
                          const float* weight_dev, void* stream) {
    if (m == nullptr || dpred == nullptr || weight_dev == nullptr || B < 1 || HW < 1 || nm < 1 || nm > C || C > LV_MAXC)
        return (int)hipErrorInvalidValue;
    const long n = (long)B * HW * nm;
    long blocks = (n + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(lovasz_grad_add_kernel, dim3((int)blocks), dim3(256), 0, (hipStream_t)stream, m, dpred, n, C, nm, scale_host, scale_dev,
                       weight_dev);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
