// Fused Winograd F(2x2, 3x3) for the inference forward (Conv2D -> folded BatchNorm [-> ReLU]) of the wide fp32 3x3 'same' layers.
// Included by conv.hip after wino.hpp: the identities, the plane numbering p = i * 4 + j and the weight image U[16][Cout][Cin]
// (mmseg_conv2d_wprep_wino) are those of wino.hpp.  ONE launch: the transformed input V and the sixteen products M never reach HBM.
//
// A block owns 64 Winograd tiles (8 image rows x 32 columns of one image: 4 x 16 tiles of 2 x 2 outputs) x 64 output channels; its four
// waves are the 2 x 2 quarters (32 tiles x 32 channels) of that block, and a wave holds ALL sixteen planes of its quarter: 16
// accumulators of v_mfma_f32_32x32x2_f32 = 256 registers per lane, one wave per SIMD.  The MFMA's A operand is U (rows = output
// channels), its B operand is V (columns = tiles), so a lane holds, in every plane, the same tile (lane & 31) and the same sixteen
// channels (8 g + 4 (lane >> 5) + e of register 4 g + e): A^T M A is lane-local, and its results are 16-byte channel vectors.
//
// K loop in chunks of 16 input channels (x1's chunks, then x2's).  Per chunk a thread loads one tile's 4 x 4 patch of 4 channels (16
// loads of 16 bytes; a pixel outside the image has an out-of-range buffer offset = 0 before the transform) and sixteen 16-byte pieces
// of U, into registers, WHILE the previous chunk is multiplied (one load between every four MFMAs); after a barrier it transforms the patch (adds only) and stores V
// [16][64 tiles][16] and U [16][64 channels][16] into LDS (64 KB each, single-buffered; 64-byte rows with the 16-byte chunk swizzle
// (row >> 2) & 3, conflict-free for the ds_read_b128 fragment reads as in conv_fast_body).  Per chunk and wave: 128 MFMAs (8 192 clocks)
// on 64 fragment reads.  Lane half lh reads chunk 2 q + lh of a row: element t of both operands is k = 4 (2 q + lh) + t.
// The grid is persistent (at most one block per CU; block b takes work items b, b + grid, ...): the first chunk of the next item is
// loaded during the last products and the epilogue of this one.  Every sum has a fixed order that does not depend on the grid.

struct WinofParams {
    const float* x1; const float* x2; const float* U; const float* bias; const float* oscale; float* y;
    int B, H, W, C1, C2, Cout, act, nwork;
    float alpha;
};

#define WINOF_TH 8      // image rows per block
#define WINOF_TW 32     // image columns per block
#define WINOF_BN 64     // output channels per block
#define WINOF_KC 16     // input channels per chunk

__global__ __launch_bounds__(256) void winof_kernel(WinofParams p) {
    __shared__ __attribute__((aligned(1024))) float Vs[16 * 64 * WINOF_KC];
    __shared__ __attribute__((aligned(1024))) float Us[16 * 64 * WINOF_KC];

    const int tid = threadIdx.x, lane = tid & 63, wid = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wm = wid >> 1, wn = wid & 1, li = lane & 31, lh = lane >> 5;
    const int K = p.C1 + p.C2, nch = K / WINOF_KC, ntn = p.Cout / WINOF_BN;
    const int tpr = p.W / WINOF_TW, tpi = (p.H / WINOF_TH) * tpr;

    const __amdgpu_buffer_rsrc_t r1 = __builtin_amdgcn_make_buffer_rsrc((void*)p.x1, 0, p.B * p.H * p.W * p.C1 * 4, 0x00020000);
    const __amdgpu_buffer_rsrc_t r2 = __builtin_amdgcn_make_buffer_rsrc((void*)(p.C2 ? p.x2 : p.x1), 0,
                                                                        p.C2 ? p.B * p.H * p.W * p.C2 * 4 : 0, 0x00020000);
    const __amdgpu_buffer_rsrc_t ru = __builtin_amdgcn_make_buffer_rsrc((void*)p.U, 0, 16 * p.Cout * K * 4, 0x00020000);

    // loader role: tile (or U row) lt, 16-byte chunk lc of the 16-channel row; LDS float offset of that piece inside a plane
    const int lt = tid >> 2, lc = tid & 3;
    const int lty = lt >> 4, ltx = lt & 15;
    const int lds_o = lt * WINOF_KC + 4 * (lc ^ ((lt >> 2) & 3));

    f32x4 d[4][4], u[16];
    // chunk c of work item w -> registers in 32 pieces (16 patch pixels, 16 planes of U), one per MFMA step of the previous chunk: a wave
    // that queued all 32 loads at once would wait for the address unit before its first MFMA.  Everything is out of range (= 0 and no
    // traffic) when the item does not exist.
    __amdgpu_buffer_rsrc_t rx = r1;
    int o00 = 0, rstep = 0, pstep = 0, uo = 0, lm = 0, ym[4], xm[4];
    const int ups = p.Cout * K * 4;
    auto prefetch_setup = [&](const int w, const int c, const bool live) {
        const int mt = w / ntn, n0 = (w - mt * ntn) * WINOF_BN;
        const int b = mt / tpi, tr = mt - b * tpi;
        const int y0 = (tr / tpr) * WINOF_TH, x0 = (tr % tpr) * WINOF_TW;
        const int k0 = c * WINOF_KC;
        const bool first = k0 < p.C1;
        const int cs = first ? p.C1 : p.C2;
        const int kc = (first ? k0 : k0 - p.C1) + 4 * lc;
        rx = first ? r1 : r2;
        // byte offset of the patch's first pixel (row y0 + 2 lty - 1, column x0 + 2 ltx - 1; only in-range pixels use it)
        const int yy0 = y0 + 2 * lty - 1, xx0 = x0 + 2 * ltx - 1;
        pstep = cs * 4; rstep = p.W * pstep;
        lm = -(int)live;
        o00 = ((b * p.H + yy0) * p.W + xx0) * pstep + kc * 4;
#pragma unroll
        for (int r = 0; r < 4; ++r) {          // all ones / zero: no short-circuit branches
            ym[r] = -(int)((unsigned)(yy0 + r) < (unsigned)p.H) & lm;
            xm[r] = -(int)((unsigned)(xx0 + r) < (unsigned)p.W);
        }
        uo = ((n0 + lt) * K + k0 + 4 * lc) * 4;
    };
    auto prefetch_piece = [&](const int i) {
        if (i < 16) {
            const int r = i >> 2, s = i & 3, m = ym[r] & xm[s];
            d[r][s] = buf_load4(rx, ((o00 + r * rstep + s * pstep) & m) | (BUF_OOB & ~m));
        } else {
            u[i - 16] = buf_load4(ru, ((uo + (i - 16) * ups) & lm) | (BUF_OOB & ~lm));
        }
    };
    // registers -> LDS: V = B^T d B (the expressions of wino_input_kernel), U as loaded
    auto fill = [&]() {
#pragma unroll
        for (int s = 0; s < 4; ++s) {          // B^T d: over the rows
            const f32x4 d0 = d[0][s], d1 = d[1][s], d2 = d[2][s], d3 = d[3][s];
            d[0][s] = d0 - d2; d[1][s] = d1 + d2; d[2][s] = d2 - d1; d[3][s] = d1 - d3;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {          // (B^T d) B: over the columns
            const f32x4 d0 = d[r][0], d1 = d[r][1], d2 = d[r][2], d3 = d[r][3];
            float* o = Vs + (r * 4) * (64 * WINOF_KC) + lds_o;
            *reinterpret_cast<f32x4*>(o + 0 * (64 * WINOF_KC)) = d0 - d2;
            *reinterpret_cast<f32x4*>(o + 1 * (64 * WINOF_KC)) = d1 + d2;
            *reinterpret_cast<f32x4*>(o + 2 * (64 * WINOF_KC)) = d2 - d1;
            *reinterpret_cast<f32x4*>(o + 3 * (64 * WINOF_KC)) = d1 - d3;
        }
#pragma unroll
        for (int q = 0; q < 16; ++q) *reinterpret_cast<f32x4*>(Us + q * (64 * WINOF_KC) + lds_o) = u[q];
    };

    f32x16 acc[16];
    auto zero = [&]() {
#pragma unroll
        for (int q = 0; q < 16; ++q)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[q][r] = 0.f;
    };
    // fragment rows of this lane: U row (channel) wn * 32 + li, V row (tile) wm * 32 + li
    const int urow = wn * 32 + li, vrow = wm * 32 + li;
    const int ukey = (urow >> 2) & 3, vkey = (vrow >> 2) & 3;
    const float* const ufr = Us + urow * WINOF_KC;
    const float* const vfr = Vs + vrow * WINOF_KC;
    auto mma = [&]() {
        f32x4 a[2], b[2];
        auto frags = [&](const int set, const int st) {      // step st = plane st / 2, half st % 2 of the chunk
            const int q = st / (WINOF_KC / 8), h = st % (WINOF_KC / 8);
            a[set] = *reinterpret_cast<const f32x4*>(ufr + q * (64 * WINOF_KC) + 4 * ((2 * h + lh) ^ ukey));
            b[set] = *reinterpret_cast<const f32x4*>(vfr + q * (64 * WINOF_KC) + 4 * ((2 * h + lh) ^ vkey));
        };
        constexpr int NST = 16 * (WINOF_KC / 8);
        static_assert(NST == 32, "one load piece per MFMA step");
        frags(0, 0);
#pragma unroll
        for (int st = 0; st < NST; ++st) {
            prefetch_piece(st);
            if (st + 1 < NST) frags((st + 1) & 1, st + 1);
            __builtin_amdgcn_sched_barrier(0);
            const int q = st / (WINOF_KC / 8);
#pragma unroll
            for (int t = 0; t < 4; ++t) acc[q] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[st & 1][t], b[st & 1][t], acc[q], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    // y = act((A^T M A) * oscale + bias): the expressions of wino_output_kernel; 16-byte stores of 4 channels
    auto epilogue = [&](const int w) {
        const int mt = w / ntn, n0 = (w - mt * ntn) * WINOF_BN;
        const int b = mt / tpi, tr = mt - b * tpi;
        const int y0 = (tr / tpr) * WINOF_TH, x0 = (tr % tpr) * WINOF_TW;
        const int t = wm * 32 + li;
        const int oy = y0 + 2 * (t >> 4), ox = x0 + 2 * (t & 15);
        float* const yb = p.y + ((size_t)(b * p.H + oy) * p.W + ox) * p.Cout + n0 + wn * 32 + 4 * lh;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            f32x4 sv = {1.f, 1.f, 1.f, 1.f}, bv = {0.f, 0.f, 0.f, 0.f};
            if (p.oscale) sv = *reinterpret_cast<const f32x4*>(p.oscale + n0 + wn * 32 + 4 * lh + 8 * g);
            if (p.bias) bv = *reinterpret_cast<const f32x4*>(p.bias + n0 + wn * 32 + 4 * lh + 8 * g);
            f32x4 o[2][2];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                float q0[4], q1[4];                 // A^T M: over the rows
#pragma unroll
                for (int s = 0; s < 4; ++s) {
                    const float m0 = acc[s][4 * g + e], m1 = acc[4 + s][4 * g + e], m2 = acc[8 + s][4 * g + e], m3 = acc[12 + s][4 * g + e];
                    q0[s] = m0 + m1 + m2;
                    q1[s] = m1 - m2 - m3;
                }
                // (A^T M) A: over the columns
                o[0][0][e] = act_apply((q0[0] + q0[1] + q0[2]) * sv[e] + bv[e], p.act, p.alpha);
                o[0][1][e] = act_apply((q0[1] - q0[2] - q0[3]) * sv[e] + bv[e], p.act, p.alpha);
                o[1][0][e] = act_apply((q1[0] + q1[1] + q1[2]) * sv[e] + bv[e], p.act, p.alpha);
                o[1][1][e] = act_apply((q1[1] - q1[2] - q1[3]) * sv[e] + bv[e], p.act, p.alpha);
            }
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) *reinterpret_cast<f32x4*>(yb + ((size_t)i * p.W + j) * p.Cout + 8 * g) = o[i][j];
            __builtin_amdgcn_sched_barrier(0);     // one channel group at a time: the next chunk's loads are waiting in registers
        }
    };

    if ((int)blockIdx.x >= p.nwork) return;
    prefetch_setup(blockIdx.x, 0, true);
#pragma unroll
    for (int i = 0; i < 32; ++i) prefetch_piece(i);
    for (int w = blockIdx.x; w < p.nwork; w += gridDim.x) {
        zero();
        for (int c = 0; c < nch; ++c) {
            __syncthreads();                       // every wave has read the previous chunk's fragments
            fill();
            __syncthreads();
            const bool last = c + 1 == nch;
            const int wnext = last ? w + (int)gridDim.x : w;
            prefetch_setup(wnext, last ? 0 : c + 1, wnext < p.nwork);
            mma();                                 // (queues the next chunk's loads between its products)
        }
        epilogue(w);
    }
}

// Default mode: a region of the per-layer A/B (tools/winof_bench.py -> profiles/winof_ab.txt, batch 8) in which every measured shape
// beats the parent's route (the direct launch, or the un-fused sequence where that one has the layer) by more than the spread of its
// rounds: planes of at least 64 x 64 pixels, at most 256 input channels in all (K = C1 + C2), at most 256 output channels and at least two
// rounds of blocks on the 256 CUs.  Outside it stay 64 x 64, 256+256 -> 256 (1.12 x) and 32 x 32, 256 -> 512 (1.11 x), which passed the
// rule only after the region was fixed, and the layers with 512 -> 512 channels (0.95 - 1.00 x: every extra N block repeats
// the input transform).
static bool winof_default_shape(int B, int H, int W, int K, int Cout) {
    const long nwork = (long)B * (H / WINOF_TH) * (W / WINOF_TW) * (Cout / WINOF_BN);
    return H >= 64 && W >= 64 && K <= 256 && Cout <= 256 && nwork >= 512;
}

extern "C" {

// structural conditions of the fused route, shared by the switch below and the entry point
static bool winof_structural(int B, int H, int W, int C1, int C2, int Cout) {
    if (g_conv_bf16 != 0 || B < 1 || H < WINOF_TH || W < WINOF_TW || H % WINOF_TH != 0 || W % WINOF_TW != 0) return false;
    if (C1 < 32 || C1 % 32 != 0 || C2 < 0 || C2 % 32 != 0 || Cout < WINOF_BN || Cout % WINOF_BN != 0) return false;
    const long lim = (1L << 31) - 64;
    const long P = (long)B * H * W, K = (long)C1 + C2;
    // 32-bit buffer offsets: every tensor and the whole weight image
    if (P * C1 * 4 >= lim || P * C2 * 4 >= lim || P * Cout * 4 >= lim || 16 * K * Cout * 4 >= lim) return false;
    if (P / (WINOF_TH * WINOF_TW) * (Cout / WINOF_BN) >= lim) return false;
    return true;
}
// The one place that decides whether the inference forward of a 3x3, stride 1, 'same' layer without up-sampling, whose caller has
// opted in (its output is seen only through a Rounding layer), takes the fused Winograd route.  Asked before mmseg_conv2d_wino_ok.
int mmseg_conv2d_winof_ok(int B, int H, int W, int C1, int C2, int Cout) {
    if (g_wino_mode == 0 || !winof_structural(B, H, W, C1, C2, Cout)) return 0;
    if (g_wino_mode == 2) return 1;
    return winof_default_shape(B, H, W, C1 + C2, Cout) ? 1 : 0;
}
// y = act(conv3x3_same(concat(x1, x2)) * oscale[c] + bias[c]) in one launch; U from mmseg_conv2d_wprep_wino.  No workspace.
// Everything is checked before the launch is queued.
int mmseg_conv2d_fwd_winof(const float* x1, const float* x2, const float* U, const float* bias, const float* oscale, float* y, int B, int H,
                           int W, int C1, int C2, int Cout, int act, float alpha, void* stream) {
    if (!winof_structural(B, H, W, C1, C2, Cout)) return (int)hipErrorInvalidValue;
    if (x1 == nullptr || U == nullptr || y == nullptr || (C2 > 0 && x2 == nullptr)) return (int)hipErrorInvalidValue;
    if (!aligned16(x1) || (C2 > 0 && !aligned16(x2)) || !aligned16(U) || !aligned16(y) || (bias != nullptr && !aligned16(bias)) ||
        (oscale != nullptr && !aligned16(oscale)))
        return (int)hipErrorInvalidValue;
    WinofParams p;
    p.x1 = x1; p.x2 = C2 > 0 ? x2 : nullptr; p.U = U; p.bias = bias; p.oscale = oscale; p.y = y;
    p.B = B; p.H = H; p.W = W; p.C1 = C1; p.C2 = C2; p.Cout = Cout; p.act = act; p.alpha = alpha;
    p.nwork = B * (H / WINOF_TH) * (W / WINOF_TW) * (Cout / WINOF_BN);
    const int grid = p.nwork < 256 ? p.nwork : 256;      // one block per CU (128 KB of LDS, 512 registers per lane)
    MMSEG_SET_LAST(26, 64, WINOF_BN);
    hipLaunchKernelGGL(winof_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
