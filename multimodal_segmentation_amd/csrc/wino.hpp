// Winograd F(2x2, 3x3) for the inference forward (Conv2D -> folded BatchNorm [-> ReLU]) of the deep fp32 3x3 'same' layers.
// Included at the end of conv.hip: the sixteen products run on conv_fast_body.
//
//   Y = A^T [ (G g G^T) .* (B^T d B) ] A        d: 4 x 4 input patch of a 2 x 2 output tile (rows 2ty-1 .. 2ty+2, zero outside the image)
//   B^T = | 1  0 -1  0 |     G = |  1    0    0  |     A^T = | 1  1  1  0 |
//         | 0  1  1  0 |         | 1/2  1/2  1/2 |           | 0  1 -1 -1 |
//         | 0 -1  1  0 |         | 1/2 -1/2  1/2 |
//         | 0  1  0 -1 |         |  0    0    1  |
//
// Four launches, no fusion (the tensors of these layers are a few MB; the transformed planes stay in L2 / MALL):
//   wino_wprep_kernel    U[p][co][ci] = (G w G^T)[p]                      p = i * 4 + j, rows K-contiguous like the other `wt` images
//   wino_input_kernel    V[p][t][c]   = (B^T d B)[p]                      t = (b, ty, tx), c over x1 then x2 (the concat is one plane row)
//   conv_fast_planes_kernel   M[p] = V[p] . U[p]^T                        a 1x1 convolution with M = T, K = C1 + C2, N = Cout per plane,
//                                                                         blockIdx.y = p; no bias or activation
//   wino_output_kernel   y = act((A^T M A) * oscale[n] + bias[n])         the expression of the mmseg_conv2d_fwd_scaled epilogue
// 4 multiplications per output and input channel instead of 9.  Every sum has a fixed order: the route is deterministic.

// one 32 x 32 (ci, co) tile of the four planes of row i = blockIdx.z of G w G^T, transposed through LDS
__global__ __launch_bounds__(256) void wino_wprep_kernel(const float* __restrict__ w, float* __restrict__ U, int Cin, int Cout) {
    __shared__ float t[4][32][33];
    const int co0 = blockIdx.x * 32, ci0 = blockIdx.y * 32, i = blockIdx.z;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int rr = ty; rr < 32; rr += 8) {
        const int ci = ci0 + rr, co = co0 + tx;
        float r[3] = {0.f, 0.f, 0.f};          // row i of G w: one value per kernel column
        if (ci < Cin && co < Cout) {
            const size_t o = (size_t)ci * Cout + co, tap = (size_t)Cin * Cout;
#pragma unroll
            for (int kw = 0; kw < 3; ++kw) {
                if (i == 0) r[kw] = w[kw * tap + o];
                else if (i == 3) r[kw] = w[(6 + kw) * tap + o];
                else {
                    const float a = w[kw * tap + o], b = w[(3 + kw) * tap + o], c = w[(6 + kw) * tap + o];
                    r[kw] = (i == 1 ? (a + b + c) : (a - b + c)) * 0.5f;
                }
            }
        }
        t[0][rr][tx] = r[0];
        t[1][rr][tx] = (r[0] + r[1] + r[2]) * 0.5f;
        t[2][rr][tx] = (r[0] - r[1] + r[2]) * 0.5f;
        t[3][rr][tx] = r[2];
    }
    __syncthreads();
    for (int rr = ty; rr < 32; rr += 8) {
        const int co = co0 + rr, ci = ci0 + tx;
        if (co < Cout && ci < Cin)
#pragma unroll
            for (int j = 0; j < 4; ++j) U[((size_t)(i * 4 + j) * Cout + co) * Cin + ci] = t[j][tx][rr];
    }
}

// one thread = 4 consecutive channels of one 2 x 2 output tile: 16 loads of 16 bytes, adds only, 16 stores of 16 bytes (one per plane)
__global__ __launch_bounds__(256) void wino_input_kernel(const float* __restrict__ x1, const float* __restrict__ x2, float* __restrict__ V,
                                                         int H, int W, int C1, int C2, long T) {
    const int Cin = C1 + C2, c4n = Cin >> 2, TH = H >> 1, TW = W >> 1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * c4n) return;
    const int c = (int)(idx % c4n) * 4;
    const long t = idx / c4n;
    const int tx = (int)(t % TW), ty = (int)((t / TW) % TH), b = (int)(t / ((long)TW * TH));
    const bool first = c < C1;
    const float* src = first ? x1 : x2;
    const int cs = first ? C1 : C2, cc = first ? c : c - C1;
    f32x4 d[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int hi = 2 * ty - 1 + r;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const int wi = 2 * tx - 1 + s;
            d[r][s] = f32x4{0.f, 0.f, 0.f, 0.f};
            if ((unsigned)hi < (unsigned)H && (unsigned)wi < (unsigned)W)
                d[r][s] = *reinterpret_cast<const f32x4*>(src + (((size_t)b * H + hi) * W + wi) * cs + cc);
        }
    }
#pragma unroll
    for (int s = 0; s < 4; ++s) {          // B^T d: over the rows
        const f32x4 d0 = d[0][s], d1 = d[1][s], d2 = d[2][s], d3 = d[3][s];
        d[0][s] = d0 - d2; d[1][s] = d1 + d2; d[2][s] = d2 - d1; d[3][s] = d1 - d3;
    }
    const size_t plane = (size_t)T * Cin;
    float* o = V + (size_t)t * Cin + c;
#pragma unroll
    for (int r = 0; r < 4; ++r) {          // (B^T d) B: over the columns
        const f32x4 d0 = d[r][0], d1 = d[r][1], d2 = d[r][2], d3 = d[r][3];
        *reinterpret_cast<f32x4*>(o + (size_t)(r * 4 + 0) * plane) = d0 - d2;
        *reinterpret_cast<f32x4*>(o + (size_t)(r * 4 + 1) * plane) = d1 + d2;
        *reinterpret_cast<f32x4*>(o + (size_t)(r * 4 + 2) * plane) = d2 - d1;
        *reinterpret_cast<f32x4*>(o + (size_t)(r * 4 + 3) * plane) = d1 - d3;
    }
}

// strided-batch variant of conv_fast_kernel: gridDim.y problems that differ only by a plane stride (floats) of x1, wt and y
template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void conv_fast_planes_kernel(ConvParams p, long sx, long sw, long sy) {
    const long z = blockIdx.y;
    p.x1 += z * sx; p.wt += z * sw; p.y += z * sy;
    conv_fast_body<BM, BN, WM, WN>(p, blockIdx.x, gridDim.x);
}
template <int BM, int BN, int WM, int WN>
static int launch_fast_planes(const ConvParams& p, int planes, long sx, long sw, long sy, hipStream_t st) {
    const int ntm = (p.M + BM - 1) / BM, ntn = (p.Cout + BN - 1) / BN;
    MMSEG_SET_LAST(25, BM, BN);
    hipLaunchKernelGGL((conv_fast_planes_kernel<BM, BN, WM, WN>), dim3(ntm * ntn, planes), dim3(WM * WN * 64), 0, st, p, sx, sw, sy);
    return MMSEG_CHECK_LAUNCH();
}

// one thread = 4 consecutive output channels of one 2 x 2 output tile: 16 loads of 16 bytes, A^T M A, scale, bias, activation, 4 stores
__global__ __launch_bounds__(256) void wino_output_kernel(const float* __restrict__ Mp, const float* __restrict__ bias,
                                                          const float* __restrict__ oscale, float* __restrict__ y, int H, int W, int Cout,
                                                          long T, int act, float alpha) {
    const int n4n = Cout >> 2, TH = H >> 1, TW = W >> 1;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= T * n4n) return;
    const int n = (int)(idx % n4n) * 4;
    const long t = idx / n4n;
    const int tx = (int)(t % TW), ty = (int)((t / TW) % TH), b = (int)(t / ((long)TW * TH));
    const size_t plane = (size_t)T * Cout;
    const float* m = Mp + (size_t)t * Cout + n;
    f32x4 q[2][4];                         // A^T M: over the rows
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        const f32x4 m0 = *reinterpret_cast<const f32x4*>(m + (size_t)(0 + s) * plane), m1 = *reinterpret_cast<const f32x4*>(m + (size_t)(4 + s) * plane);
        const f32x4 m2 = *reinterpret_cast<const f32x4*>(m + (size_t)(8 + s) * plane), m3 = *reinterpret_cast<const f32x4*>(m + (size_t)(12 + s) * plane);
        q[0][s] = m0 + m1 + m2;
        q[1][s] = m1 - m2 - m3;
    }
    f32x4 sv = {1.f, 1.f, 1.f, 1.f}, bv = {0.f, 0.f, 0.f, 0.f};
    if (oscale) sv = *reinterpret_cast<const f32x4*>(oscale + n);
    if (bias) bv = *reinterpret_cast<const f32x4*>(bias + n);
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const f32x4 acc[2] = {q[i][0] + q[i][1] + q[i][2], q[i][1] - q[i][2] - q[i][3]};      // (A^T M) A: over the columns
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = act_apply(acc[j][e] * sv[e] + bv[e], act, alpha);
            *reinterpret_cast<f32x4*>(y + (((size_t)b * H + 2 * ty + i) * W + 2 * tx + j) * Cout + n) = v;
        }
    }
}

// Default mode: the region of the per-layer A/B (tools/wino_bench.py -> profiles/wino_ab.txt, batch 8) in which every measured shape beats
// the direct launch by more than the spread of its rounds: planes of 16 x 16 to 64 x 64 pixels with at least 512 tiles (T), at least 256
// input channels in all (K = C1 + C2) and at least 256 output channels.  128 -> 256 at 64 x 64 (K loop of 4 tiles) was inside the spread
// and stays out; larger planes were not measured (their transformed planes are 0.27 - 2 GB).
static bool wino_default_shape(long T, int H, int W, int K, int Cout) {
    return H <= 64 && W <= 64 && T >= 512 && K >= 256 && Cout >= 256;
}

extern "C" {

// 0 = never; 1 (default) = the shapes profiles/wino_ab.txt shows faster than the direct launch; 2 = wherever the structural conditions
// hold.  Only the inference forward (ops.conv2d_bn_infer) asks: its results end in the anatomy encoder's Rounding layer, like those of
// the folded up-sampling.  Training forwards and both gradients keep their kernels and their bits.
static int g_wino_mode = 1;
int mmseg_conv2d_wino_mode(int mode) {
    const int old = g_wino_mode;
    if (mode >= 0 && mode <= 2) g_wino_mode = mode;
    return old;
}
// floats of workspace of mmseg_conv2d_fwd_wino: the sixteen planes of V [T][C1 + C2] and of M [T][Cout], T = B * H/2 * W/2
long mmseg_conv2d_wino_workspace(int B, int H, int W, int C1, int C2, int Cout) {
    if (B < 1 || H < 2 || W < 2 || C1 < 0 || C2 < 0 || Cout < 0) return 0;
    return 16L * B * (H / 2) * (W / 2) * ((long)C1 + C2 + Cout);
}
// structural conditions of the route, shared by the switch below and the entry point
static bool wino_structural(int B, int H, int W, int C1, int C2, int Cout) {
    if (g_conv_bf16 != 0 || B < 1 || H < 2 || W < 2 || (H & 1) || (W & 1)) return false;
    if (C1 < 32 || C1 % 32 != 0 || C2 < 0 || C2 % 32 != 0 || Cout < 32 || Cout % 32 != 0) return false;
    const long lim = (1L << 31) - 64;
    const long T = (long)B * (H / 2) * (W / 2), K = (long)C1 + C2;
    // tensors, and one plane each of V, M and U (32-bit buffer offsets; the weight plane below 2^30 bytes like the other images)
    if (4 * T * C1 * 4 >= lim || 4 * T * C2 * 4 >= lim || 4 * T * Cout * 4 >= lim) return false;
    if (T * K * 4 >= lim || T * Cout * 4 >= lim || K * Cout * 4 >= (1L << 30)) return false;
    return true;
}
// The one place that decides whether the inference forward of a 3x3, stride 1, 'same' layer without up-sampling
// x1 [B,H,W,C1] (+ x2 [B,H,W,C2]) -> y [B,H,W,Cout] takes the Winograd route.
int mmseg_conv2d_wino_ok(int B, int H, int W, int C1, int C2, int Cout) {
    if (g_wino_mode == 0 || !wino_structural(B, H, W, C1, C2, Cout)) return 0;
    if (g_wino_mode == 2) return 1;
    return wino_default_shape((long)B * (H / 2) * (W / 2), H, W, C1 + C2, Cout) ? 1 : 0;
}
// U [16][Cout][Cin] = G w G^T of w [3,3,Cin,Cout] (Keras layout)
int mmseg_conv2d_wprep_wino(const float* w, float* out, int Cin, int Cout, void* stream) {
    if (g_conv_bf16 != 0 || Cin < 1 || Cout < 1 || (Cin + 31) / 32 > 65535) return (int)hipErrorInvalidValue;
    const dim3 grid((Cout + 31) / 32, (Cin + 31) / 32, 4);
    hipLaunchKernelGGL(wino_wprep_kernel, grid, dim3(256), 0, (hipStream_t)stream, w, out, Cin, Cout);
    return MMSEG_CHECK_LAUNCH();
}
// y = act(conv3x3_same(concat(x1, x2)) * oscale[c] + bias[c]) through the four launches above; U from mmseg_conv2d_wprep_wino, ws >=
// mmseg_conv2d_wino_workspace floats.  Everything is checked before the first launch is queued.
int mmseg_conv2d_fwd_wino(const float* x1, const float* x2, const float* U, const float* bias, const float* oscale, float* y, int B, int H,
                          int W, int C1, int C2, int Cout, int act, float alpha, float* ws, long ws_floats, void* stream) {
    if (!wino_structural(B, H, W, C1, C2, Cout)) return (int)hipErrorInvalidValue;
    if (x1 == nullptr || U == nullptr || y == nullptr || ws == nullptr || (C2 > 0 && x2 == nullptr)) return (int)hipErrorInvalidValue;
    if (!aligned16(x1) || (C2 > 0 && !aligned16(x2)) || !aligned16(U) || !aligned16(y) || !aligned16(ws) ||
        (bias != nullptr && !aligned16(bias)) || (oscale != nullptr && !aligned16(oscale)))
        return (int)hipErrorInvalidValue;
    if (ws_floats < mmseg_conv2d_wino_workspace(B, H, W, C1, C2, Cout)) return (int)hipErrorInvalidValue;
    const long T = (long)B * (H / 2) * (W / 2);
    const int K = C1 + C2;
    float* V = ws;
    float* Mp = ws + 16 * T * K;
    hipStream_t st = (hipStream_t)stream;
    const long nin = T * (K / 4), nout = T * (Cout / 4);
    if ((nin + 255) / 256 >= (1L << 31) || (nout + 255) / 256 >= (1L << 31)) return (int)hipErrorInvalidValue;

    hipLaunchKernelGGL(wino_input_kernel, dim3((unsigned)((nin + 255) / 256)), dim3(256), 0, st, x1, x2, V, H, W, C1, C2, T);
    int rc = MMSEG_CHECK_LAUNCH();
    if (rc != 0) return rc;

    ConvParams p;
    p.x1 = V; p.x2 = nullptr; p.w = nullptr; p.wt = U; p.bias = nullptr; p.oscale = nullptr; p.y = Mp; p.y2 = nullptr;
    p.B = 1; p.H = 1; p.W = (int)T; p.C1 = K; p.C2 = 0; p.H1 = 1; p.W1 = (int)T;
    p.Ho = 1; p.Wo = (int)T; p.Cout = Cout; p.KH = 1; p.KW = 1; p.stride = 1; p.pad_h = 0; p.pad_w = 0;
    p.ups = 0; p.transposed = 0; p.act = 0; p.alpha = 0.f; p.M = (int)T; p.K = K; p.nsplit1 = 0;
    p.oH = 1; p.oW = (int)T; p.osh = 1; p.osw = 1; p.ooh = 0; p.oow = 0; p.io = 0;
    p.qepi = quad_epilogue_ok(p);
    const long sx = T * K, sw = (long)K * Cout, sy = T * Cout;
    // the dispatcher's bar for a grid that fills the chip, counted over the sixteen planes
    const long tiles_big = ((T + 127) / 128) * ((Cout + 127) / 128) * 16;
    const long tiles_mid = ((T + 127) / 128) * ((Cout + 63) / 64) * 16;
    if (Cout > 64 && tiles_big >= 384) rc = launch_fast_planes<128, 128, 2, 2>(p, 16, sx, sw, sy, st);
    else if (Cout > 32 && tiles_mid >= 384) rc = launch_fast_planes<128, 64, 2, 2>(p, 16, sx, sw, sy, st);
    else if (Cout > 32) rc = launch_fast_planes<64, 64, 2, 2>(p, 16, sx, sw, sy, st);
    else rc = launch_fast_planes<128, 32, 4, 1>(p, 16, sx, sw, sy, st);
    if (rc != 0) return rc;

    hipLaunchKernelGGL(wino_output_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, st, Mp, bias, oscale, y, H, W, Cout, T, act, alpha);
    return MMSEG_CHECK_LAUNCH();
}

}  // extern "C"
