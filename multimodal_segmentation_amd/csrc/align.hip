// Cross-modality alignment of one volume by normalised mutual information (gfx950; build-defined, the rule is in include/mmseg_hip.h).
//
// Translation only: an integer slice shift dz and an integer in-plane shift (dy, dx) in pixels of the loader's resampled frames.  Both
// volumes are quantised once to one byte per resampled pixel (al_quantise_kernel; pp_bilinear of resample.hpp, so the values are the
// ones the percentiles were selected from).  A search stage then scores C candidates in three launches, none of which returns to
// the host:
//   al_hist_kernel    grid (slabs, C): a block owns one candidate and a share of its (slice, row) pairs; a wave owns a row and its
//                     lanes walk the sampled columns, so the byte loads of a wave are consecutive at stride t.  Counts go to a B x B
//                     uint32 table in LDS (16 KB at 64 bins) with LDS atomics and are merged into h [C,B,B] with integer atomics, the
//                     empty bins skipped.  MR frames are mostly air, so most lanes of a wave meet the SAME bin: with `aggregate` the
//                     lanes that hold the bin of the wave's first active lane are counted with one ballot and added by one atomic.
//   al_score_kernel   grid C: marginals by LDS integer atomics, the three entropies in fp64 (a thread adds its terms in index order,
//                     the block adds the threads' sums in a fixed tree), the admissibility test and the score.
//   al_select_kernel  one block: the arg max under the tie rule (a strict total order, so the result does not depend on who compares
//                     first), written into the state block that the next stage's enumeration reads.
// Candidates are never stored: every kernel enumerates candidate c of the stage from (mode, t, Z, Py, Px) and, for a refinement stage,
// the centre in the state block (al_candidate).  Integer atomics and fixed-order fp64 only: two runs are bitwise equal.
#include "common.hpp"
#include "resample.hpp"

#define AL_BLOCK 256
#define AL_MAXBINS 64
#define AL_MAXSLABS 64
#define AL_SLAB_PAIRS 16384
#define AL_MAXCAND 65535          // gridDim.y
#define AL_STATE 8                // doubles: centre dz, dy, dx; best score; zero-shift score; N of the best; found; stage counter

#define AL_EXPLICIT 0
#define AL_LATTICE 1
#define AL_REFINE 2

struct al_geo {
    int Sa, RHa, RWa, Sb, RHb, RWb;
    int cay, cax, cby, cbx;          // centre_start of each frame against the window O, per axis
};

struct al_stage {
    int mode, t, Z, Py, Px, C;
};

// centre_start of loaders/volume_folder.py: the signed start of the centre window of extent O in a frame of extent R
static int al_centre(int R, int O) { return R > O ? (R - O + 1) / 2 : -((O - R) / 2); }

// candidate c of a stage -> (dz, dy, dx); false where it lies outside the search range (a refinement stage at the border)
__device__ __forceinline__ bool al_candidate(const al_stage& st, const int* __restrict__ cand, const double* __restrict__ state, int c,
                                             int& dz, int& dy, int& dx) {
    if (st.mode == AL_EXPLICIT) {
        dz = cand[3 * c]; dy = cand[3 * c + 1]; dx = cand[3 * c + 2];
        return true;
    }
    if (c == st.C - 1) {          // the zero-shift probe: scored, never selected
        dz = dy = dx = 0;
        return true;
    }
    if (st.mode == AL_LATTICE) {
        const int my = st.Py / st.t, mx = st.Px / st.t, ny = 2 * my + 1, nx = 2 * mx + 1;
        const int iz = c / (ny * nx), r = c - iz * ny * nx, iy = r / nx, ix = r - iy * nx;
        dz = iz - st.Z; dy = (iy - my) * st.t; dx = (ix - mx) * st.t;
        return true;
    }
    const int jz = c / 9, r = c - jz * 9, jy = r / 3, jx = r - jy * 3;
    dz = (int)state[0] + jz - 1; dy = (int)state[1] + (jy - 1) * st.t; dx = (int)state[2] + (jx - 1) * st.t;
    return dz >= -st.Z && dz <= st.Z && dy >= -st.Py && dy <= st.Py && dx >= -st.Px && dx <= st.Px;
}

// the window coordinates o of one axis at which both frames are read: lo <= o < hi, o mod t == 0 (floor-mod) -> first o and count
__device__ __forceinline__ void al_axis(int Ra, int ca, int Rb, int cb, int d, int t, int& first, int& count) {
    const int lo = max(-ca, -cb - d), hi = min(Ra - ca, Rb - cb - d);
    const int q = lo >= 0 ? (lo + t - 1) / t : -((-lo) / t);          // ceil(lo / t)
    first = q * t;
    count = hi > first ? (hi - first + t - 1) / t : 0;
}

__device__ __forceinline__ void al_slices(const al_geo& g, int dz, int& s0, int& ns) {
    s0 = max(0, -dz);
    ns = max(0, min(g.Sa, g.Sb - dz) - s0);
}

// the stride-1 overlap pair count of a shift, in closed form
__device__ __forceinline__ double al_full(const al_geo& g, int dz, int dy, int dx) {
    int s0, ns, f, ny, nx;
    al_slices(g, dz, s0, ns);
    al_axis(g.RHa, g.cay, g.RHb, g.cby, dy, 1, f, ny);
    al_axis(g.RWa, g.cax, g.RWb, g.cbx, dx, 1, f, nx);
    return (double)ns * (double)ny * (double)nx;
}

// grid (nblk, S), block AL_BLOCK: q[s, r, c] = the bin of the resampled pixel between knots[0] and knots[1]
__global__ void __launch_bounds__(AL_BLOCK) al_quantise_kernel(const float* __restrict__ img, const float* __restrict__ knots,
                                                               unsigned char* __restrict__ q, int H, int W, int RH, int RW, double ry,
                                                               double rx, int B) {
#pragma clang fp contract(off)
    const int s = blockIdx.y;
    const float lo = knots[0], hi = knots[1];
    const float scale = hi > lo ? (float)B / (hi - lo) : 0.f;
    const float* src = img + (size_t)s * H * W;
    unsigned char* dst = q + (size_t)s * RH * RW;
    const int n = RH * RW;
    for (int e = blockIdx.x * AL_BLOCK + threadIdx.x; e < n; e += gridDim.x * AL_BLOCK) {
        const int dr = e / RW, dc = e - dr * RW;
        const float v = pp_bilinear(src, H, W, dr, dc, ry, rx);
        int b = 0;
        if (hi > lo && v > lo) b = v >= hi ? B - 1 : min(B - 1, (int)floorf((v - lo) * scale));
        dst[e] = (unsigned char)b;
    }
}

// grid (slabs, C), block AL_BLOCK: h[c] += the joint histogram of this block's share of candidate c's sampled pairs
template <bool AGG>
__global__ void __launch_bounds__(AL_BLOCK) al_hist_kernel(const unsigned char* __restrict__ qa, const unsigned char* __restrict__ qb,
                                                           const int* __restrict__ cand, const double* __restrict__ state,
                                                           unsigned* __restrict__ h, al_geo g, al_stage st, int B) {
    __shared__ unsigned lh[AL_MAXBINS * AL_MAXBINS];
    const int c = blockIdx.y, nb = B * B;
    int dz, dy, dx;
    if (!al_candidate(st, cand, state, c, dz, dy, dx)) return;          // uniform over the block: h[c] stays 0
    int s0, ns, oy0, ny, ox0, nx;
    al_slices(g, dz, s0, ns);
    al_axis(g.RHa, g.cay, g.RHb, g.cby, dy, st.t, oy0, ny);
    al_axis(g.RWa, g.cax, g.RWb, g.cbx, dx, st.t, ox0, nx);
    const int rows = ns * ny;
    if (rows == 0 || nx == 0) return;
    for (int i = threadIdx.x; i < nb; i += AL_BLOCK) lh[i] = 0u;
    __syncthreads();
    const int lane = threadIdx.x & 63, top = B - 1;
    for (int r = blockIdx.x * (AL_BLOCK / 64) + (threadIdx.x >> 6); r < rows; r += gridDim.x * (AL_BLOCK / 64)) {
        const int si = r / ny, oy = oy0 + (r - si * ny) * st.t;
        const unsigned char* pa = qa + ((size_t)(s0 + si) * g.RHa + (oy + g.cay)) * g.RWa + g.cax;
        const unsigned char* pb = qb + ((size_t)(s0 + si + dz) * g.RHb + (oy + g.cby + dy)) * g.RWb + (g.cbx + dx);
        for (int i0 = 0; i0 < nx; i0 += 64) {          // uniform over the wave
            const int i = i0 + lane;
            int bin = -1;
            if (i < nx) {
                const int ox = ox0 + i * st.t;
                bin = min((int)pa[ox], top) * B + min((int)pb[ox], top);
            }
            if (AGG) {
                const unsigned long long active = __ballot(bin >= 0);          // never empty: i0 < nx
                const int lead = __ffsll((long long)active) - 1;
                const int lbin = __shfl(bin, lead, 64);
                const unsigned long long same = __ballot(bin == lbin);
                if (lane == lead) atomicAdd(&lh[lbin], (unsigned)__popcll(same));
                else if (bin >= 0 && bin != lbin) atomicAdd(&lh[bin], 1u);
            } else if (bin >= 0) {
                atomicAdd(&lh[bin], 1u);
            }
        }
    }
    __syncthreads();
    unsigned* gh = h + (size_t)c * nb;
    for (int i = threadIdx.x; i < nb; i += AL_BLOCK) {
        const unsigned v = lh[i];
        if (v) atomicAdd(gh + i, v);
    }
}

// sum over the block in a fixed tree; the result is valid in every thread.  red: AL_BLOCK doubles of LDS
__device__ __forceinline__ double al_block_sum(double v, double* red) {
    __syncthreads();
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = AL_BLOCK / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

// -p log p of a count among n; 0 for an empty bin
__device__ __forceinline__ double al_term(unsigned cnt, double n) {
    if (cnt == 0u) return 0.0;
    const double p = (double)cnt / n;
    return -(p * log(p));
}

// grid C, block AL_BLOCK: scores[c] = (score, N) of h[c]
__global__ void __launch_bounds__(AL_BLOCK) al_score_kernel(const unsigned* __restrict__ h, const int* __restrict__ cand,
                                                            const double* __restrict__ state, double* __restrict__ scores, al_geo g,
                                                            al_stage st, int B, double min_overlap) {
#pragma clang fp contract(off)
    __shared__ unsigned ma[AL_MAXBINS], mb[AL_MAXBINS];
    __shared__ double red[AL_BLOCK];
    const int c = blockIdx.x, nb = B * B;
    const unsigned* hc = h + (size_t)c * nb;
    if (threadIdx.x < AL_MAXBINS) ma[threadIdx.x] = mb[threadIdx.x] = 0u;
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += AL_BLOCK) {
        const unsigned v = hc[i];
        if (v) {
            atomicAdd(&ma[i / B], v);
            atomicAdd(&mb[i - (i / B) * B], v);
        }
    }
    __syncthreads();
    unsigned total = 0u;
    for (int i = 0; i < B; ++i) total += ma[i];          // < 2^31 pairs (the launcher's limit), the same in every thread
    const double n = (double)total;
    double tj = 0.0;
    if (total)
        for (int i = threadIdx.x; i < nb; i += AL_BLOCK) tj += al_term(hc[i], n);
    const double hab = al_block_sum(tj, red);
    const double ha = al_block_sum(total && threadIdx.x < B ? al_term(ma[threadIdx.x], n) : 0.0, red);
    const double hb = al_block_sum(total && threadIdx.x < B ? al_term(mb[threadIdx.x], n) : 0.0, red);
    if (threadIdx.x) return;
    int dz, dy, dx;
    double score = -1.0;
    if (al_candidate(st, cand, state, c, dz, dy, dx) && total && hab != 0.0 &&
        al_full(g, dz, dy, dx) >= min_overlap * al_full(g, 0, 0, 0))
        score = (ha + hb) / hab;
    scores[2 * c] = score;
    scores[2 * c + 1] = n;
}

// true where candidate (sa, a) is better than (sb, b): the higher score, then the smaller dz^2, the smaller dy^2 + dx^2, the
// lexicographically smaller (dz, dy, dx)
__device__ __forceinline__ bool al_better(double sa, int az, int ay, int ax, double sb, int bz, int by, int bx) {
    if (sa != sb) return sa > sb;
    const long a1 = (long)az * az, b1 = (long)bz * bz;
    if (a1 != b1) return a1 < b1;
    const long a2 = (long)ay * ay + (long)ax * ax, b2 = (long)by * by + (long)bx * bx;
    if (a2 != b2) return a2 < b2;
    if (az != bz) return az < bz;
    if (ay != by) return ay < by;
    return ax < bx;
}

// one block of AL_BLOCK threads: the best candidate of the stage -> state
__global__ void __launch_bounds__(AL_BLOCK) al_select_kernel(const double* __restrict__ scores, const int* __restrict__ cand,
                                                             double* __restrict__ state, al_stage st) {
    __shared__ double bs[AL_BLOCK];
    __shared__ int bc[AL_BLOCK];
    const int nsel = st.mode == AL_EXPLICIT ? st.C : st.C - 1;          // the probe is not selectable
    double best = -2.0;
    int bi = -1, bz = 0, by = 0, bx = 0;
    for (int c = threadIdx.x; c < nsel; c += AL_BLOCK) {
        int dz, dy, dx;
        if (!al_candidate(st, cand, state, c, dz, dy, dx)) continue;
        const double s = scores[2 * c];
        if (bi < 0 || al_better(s, dz, dy, dx, best, bz, by, bx)) { best = s; bi = c; bz = dz; by = dy; bx = dx; }
    }
    bs[threadIdx.x] = best;
    bc[threadIdx.x] = bi;
    __syncthreads();
    for (int o = AL_BLOCK / 2; o > 0; o >>= 1) {
        if (threadIdx.x < o) {
            const int ci = bc[threadIdx.x], cj = bc[threadIdx.x + o];
            bool take = false;
            if (cj >= 0) {
                take = ci < 0;
                if (!take) {
                    int iz, iy, ix, jz, jy, jx;
                    al_candidate(st, cand, state, ci, iz, iy, ix);
                    al_candidate(st, cand, state, cj, jz, jy, jx);
                    take = al_better(bs[threadIdx.x + o], jz, jy, jx, bs[threadIdx.x], iz, iy, ix);
                }
            }
            if (take) { bs[threadIdx.x] = bs[threadIdx.x + o]; bc[threadIdx.x] = cj; }
        }
        __syncthreads();          // every read of the old centre in `state` lies before the last of these
    }
    if (threadIdx.x) return;
    int dz = 0, dy = 0, dx = 0;
    const int win = bc[0];
    const bool found = win >= 0 && bs[0] >= 0.0;
    if (found) al_candidate(st, cand, state, win, dz, dy, dx);
    const int rec = found ? win : (st.mode == AL_EXPLICIT ? -1 : st.C - 1);          // no admissible candidate: the zero shift's record
    const double score = rec >= 0 ? scores[2 * rec] : -1.0, n = rec >= 0 ? scores[2 * rec + 1] : 0.0;
    const double zero = st.mode == AL_EXPLICIT ? state[4] : scores[2 * (st.C - 1)];
    const double stages = state[7];
    state[0] = (double)dz; state[1] = (double)dy; state[2] = (double)dx;
    state[3] = score; state[4] = zero; state[5] = n;
    state[6] = found ? 1.0 : 0.0;
    state[7] = stages + 1.0;
}

static int al_blocks(long n) {
    const long b = (n + AL_BLOCK - 1) / AL_BLOCK;
    return (int)(b < 1 ? 1 : (b < AL_MAXSLABS ? b : AL_MAXSLABS));
}

static long al_count(int mode, int t, int Z, int Py, int Px) {
    if (t < 1 || Z < 0 || Py < 0 || Px < 0 || Z > 4096 || Py > (1 << 20) || Px > (1 << 20)) return 0;
    if (mode == AL_REFINE) return 28;
    if (mode != AL_LATTICE) return 0;
    return (2L * Z + 1) * (2L * (Py / t) + 1) * (2L * (Px / t) + 1) + 1;
}

// geometry and stage of one call, checked: every index the kernels form stays inside qa / qb / h by al_axis and al_slices, given
// frames below 2^31 bytes and a window of at least one pixel
static bool al_setup(int Sa, int RHa, int RWa, int Sb, int RHb, int RWb, int OH, int OW, int mode, int t, int Z, int Py, int Px, int C,
                     int B, const void* cand, const void* state, al_geo& g, al_stage& st) {
    if (Sa < 1 || RHa < 1 || RWa < 1 || Sb < 1 || RHb < 1 || RWb < 1 || OH < 1 || OW < 1 || B < 2 || B > AL_MAXBINS || C < 1 ||
        C > AL_MAXCAND || t < 1 || t > (1 << 16))
        return false;
    if ((long)Sa * RHa * RWa >= 0x7fffffffL || (long)Sb * RHb * RWb >= 0x7fffffffL) return false;
    if (mode == AL_EXPLICIT) {
        if (!cand) return false;
    } else if (al_count(mode, t, Z, Py, Px) != C || (mode == AL_REFINE && !state)) {
        return false;
    }
    g = {Sa, RHa, RWa, Sb, RHb, RWb, al_centre(RHa, OH), al_centre(RWa, OW), al_centre(RHb, OH), al_centre(RWb, OW)};
    st = {mode, t, Z, Py, Px, C};
    return true;
}

extern "C" {

// the candidates of a stage, the trailing zero-shift probe included; 0 for a stage the kernels refuse
long mmseg_align_stage_candidates(int mode, int stride, int Z, int Py, int Px) {
    const long c = al_count(mode, stride, Z, Py, Px);
    return c > AL_MAXCAND ? 0 : c;
}

// bytes of h [C,B,B] uint32 and scores [C,2] fp64 of one stage (h first; 8-byte aligned); 0 outside the limits
long mmseg_align_workspace_bytes(int C, int bins) {
    if (C < 1 || C > AL_MAXCAND || bins < 2 || bins > AL_MAXBINS) return 0;
    return (((long)C * bins * bins * 4 + 7) / 8) * 8 + (long)C * 16;
}

int mmseg_align_quantise(const float* img, const float* knots, unsigned char* q, int S, int H, int W, int RH, int RW, int bins,
                         void* stream) {
    if (S <= 0) return 0;
    if (!img || !knots || !q || S > 65535 || H < 1 || W < 1 || RH < 1 || RW < 1 || (long)H * W >= 0x7fffffffL ||
        (long)RH * RW >= 0x7fffffffL - AL_MAXSLABS * AL_BLOCK || bins < 2 || bins > AL_MAXBINS)
        return (int)hipErrorInvalidValue;
    const dim3 grid((unsigned)al_blocks((long)RH * RW), S);
    hipLaunchKernelGGL(al_quantise_kernel, grid, dim3(AL_BLOCK), 0, (hipStream_t)stream, img, knots, q, H, W, RH, RW,
                       (double)H / (double)RH, (double)W / (double)RW, bins);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_align_histograms(const unsigned char* qa, const unsigned char* qb, const int* cand, const double* state, int* h, int Sa,
                           int RHa, int RWa, int Sb, int RHb, int RWb, int OH, int OW, int mode, int stride, int Z, int Py, int Px, int C,
                           int bins, int aggregate, void* stream) {
    al_geo g;
    al_stage st;
    if (!qa || !qb || !h || !al_setup(Sa, RHa, RWa, Sb, RHb, RWb, OH, OW, mode, stride, Z, Py, Px, C, bins, cand, state, g, st))
        return (int)hipErrorInvalidValue;
    const hipError_t zeroed = hipMemsetAsync(h, 0, (size_t)C * bins * bins * 4, (hipStream_t)stream);
    if (zeroed != hipSuccess) return (int)zeroed;
    // a block merges up to B * B bins into h, so it should have counted many more pairs than that: one slab per AL_SLAB_PAIRS sampled
    // pairs of the reference frame (a coarse stage has thousands of candidates and fills the device with one slab each)
    const long pairs = (long)Sa * ((RHa + stride - 1) / stride) * ((RWa + stride - 1) / stride);
    const long slabs = (pairs + AL_SLAB_PAIRS - 1) / AL_SLAB_PAIRS;
    const dim3 grid((unsigned)(slabs < 1 ? 1 : (slabs < AL_MAXSLABS ? slabs : AL_MAXSLABS)), C);
    unsigned* hu = reinterpret_cast<unsigned*>(h);
    if (aggregate)
        hipLaunchKernelGGL(al_hist_kernel<true>, grid, dim3(AL_BLOCK), 0, (hipStream_t)stream, qa, qb, cand, state, hu, g, st, bins);
    else
        hipLaunchKernelGGL(al_hist_kernel<false>, grid, dim3(AL_BLOCK), 0, (hipStream_t)stream, qa, qb, cand, state, hu, g, st, bins);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_align_scores(const int* h, const int* cand, const double* state, double* scores, int Sa, int RHa, int RWa, int Sb, int RHb,
                       int RWb, int OH, int OW, int mode, int stride, int Z, int Py, int Px, int C, int bins, double min_overlap,
                       void* stream) {
    al_geo g;
    al_stage st;
    if (!h || !scores || !(min_overlap >= 0.0 && min_overlap <= 1.0) ||
        !al_setup(Sa, RHa, RWa, Sb, RHb, RWb, OH, OW, mode, stride, Z, Py, Px, C, bins, cand, state, g, st))
        return (int)hipErrorInvalidValue;
    hipLaunchKernelGGL(al_score_kernel, dim3(C), dim3(AL_BLOCK), 0, (hipStream_t)stream, reinterpret_cast<const unsigned*>(h), cand, state,
                       scores, g, st, bins, min_overlap);
    return MMSEG_CHECK_LAUNCH();
}

int mmseg_align_select(const double* scores, const int* cand, double* state, int mode, int stride, int Z, int Py, int Px, int C,
                       void* stream) {
    if (!scores || !state || C < 1 || C > AL_MAXCAND || stride < 1 || (mode == AL_EXPLICIT ? !cand : al_count(mode, stride, Z, Py, Px) != C))
        return (int)hipErrorInvalidValue;
    const al_stage st = {mode, stride, Z, Py, Px, C};
    hipLaunchKernelGGL(al_select_kernel, dim3(1), dim3(AL_BLOCK), 0, (hipStream_t)stream, scores, cand, state, st);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
