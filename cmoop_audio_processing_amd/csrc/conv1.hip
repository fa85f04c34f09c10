// The first layer of every candidate (no Python module of its own: Net's plan calls these launchers): the C_in = 1
// direct convolution on the VALU and on the matrix core (the default; CMOOP_CONV1_MFMA=0 keeps the VALU kernel),
// forward and weight gradient.  Bound by the layer's 66 MB output / dY, not by its FLOPs; every cross-thread sum has a
// fixed order.
#include "kernels.h"
#include <cstdlib>
#include <algorithm>

namespace cmoop {

// ===========================================================================
// first layer: C_in = 1 direct conv (Keras Conv2D(filters, k, padding='same') on
// the (T,F,1) input, nsga_penalty.py:255 / sa_nsga_penalty.py:151)
// ===========================================================================
// Thread = 4 consecutive pixels of one row x 4 output channels: each input row segment (4 + KS - 1 values)
// is loaded once and reused by the KS horizontal taps of all four pixels; weights come from LDS as float4.
template <int KS>
__global__ __launch_bounds__(256) void conv1_fwd_kernel(const float* __restrict__ X, const int32_t* __restrict__ idx,
                                                        int64_t row0, const float* __restrict__ Wt,
                                                        const float* __restrict__ bias, float* __restrict__ Y, int B,
                                                        int H, int W, int Cout, int relu, const StepState* __restrict__ st,
                                                        int64_t n_rows) {
    constexpr int TAPS = KS * KS, SEG = 4 + KS - 1, p = (KS - 1) >> 1;
    __shared__ __attribute__((aligned(16))) float Ws[TAPS * 64];
    if (st) row0 = st->row0;
    const int t = threadIdx.x;
    for (int i = t; i < TAPS * Cout; i += 256) {
        int co = i / TAPS, tap = i - co * TAPS;
        Ws[tap * Cout + co] = Wt[i];
    }
    __syncthreads();
    const int TPG = Cout >> 2, GPB = 256 / TPG;
    const int W4 = (W + 3) >> 2;
    const int64_t group = (int64_t)blockIdx.x * GPB + t / TPG;
    const int c4 = t % TPG;
    if (group >= (int64_t)B * H * W4) return;
    const int b = (int)(group / (H * W4)), r = (int)(group - (int64_t)b * H * W4);
    const int h = r / W4, w0 = (r - h * W4) * 4;
    const int64_t src = gather_row(idx, row0 + b, n_rows);
    const float* xb = X + src * (int64_t)H * W;
    const f32x4 bv = *reinterpret_cast<const f32x4*>(bias + 4 * c4);
    f32x4 acc[4] = {bv, bv, bv, bv};
#pragma unroll
    for (int kh = 0; kh < KS; ++kh) {
        const int ih = h + kh - p;
        if ((unsigned)ih >= (unsigned)H) continue;
        float xr[SEG];
#pragma unroll
        for (int j = 0; j < SEG; ++j) {
            const int iw = w0 - p + j;
            xr[j] = (unsigned)iw < (unsigned)W ? xb[ih * W + iw] : 0.f;
        }
#pragma unroll
        for (int kw = 0; kw < KS; ++kw) {
            const f32x4 w4 = *reinterpret_cast<const f32x4*>(&Ws[(kh * KS + kw) * Cout + 4 * c4]);
#pragma unroll
            for (int px = 0; px < 4; ++px) {
                const float xv = xr[px + kw];
                acc[px][0] = fmaf(xv, w4[0], acc[px][0]); acc[px][1] = fmaf(xv, w4[1], acc[px][1]);
                acc[px][2] = fmaf(xv, w4[2], acc[px][2]); acc[px][3] = fmaf(xv, w4[3], acc[px][3]);
            }
        }
    }
    const int64_t pix0 = ((int64_t)b * H + h) * W + w0;
#pragma unroll
    for (int px = 0; px < 4; ++px) {
        if (w0 + px >= W) break;
        f32x4 v = acc[px];
        if (relu) { v[0] = fmaxf(v[0], 0.f); v[1] = fmaxf(v[1], 0.f); v[2] = fmaxf(v[2], 0.f); v[3] = fmaxf(v[3], 0.f); }
        *reinterpret_cast<f32x4*>(Y + (pix0 + px) * Cout + 4 * c4) = v;
    }
}

// ---------------------------------------------------------------------------
// The same layer on the matrix core [r3]: out[pixel][co] = sum_tap x[pixel + tap] W[co][tap] is a GEMM with K = KS*KS (9 / 25,
// padded to 12 / 28 with zero weights).  It is not the 0.8 GFLOP that matter -- the layer is bound by its 66 MB output -- but the
// 400 FMAs per thread of the VALU form above execute on the SIMDs the other candidates' MFMA kernels are issuing on.  Here a
// workgroup stages the single-channel input halo of 256 consecutive output pixels (a few KB; rows of the virtual tall image as
// in halo_fwd_kernel, the shuffle gather resolved once per halo ROW), every lane reads its K values straight from that image
// (one ds_read_b32 per MFMA operand), the weights sit in registers, and the epilogue is the straight-line one of the halo
// kernel with the BatchNorm statistics partials riding along (no stand-alone statistics pass after the first layer).
// ---------------------------------------------------------------------------
struct Conv1Dev {
    int B, H, W, Cout, M, WP, VH, rows_max;
    uint32_t hw_magic, hw_shift, w_magic, w_shift, wp_magic, wp_shift, vh_magic, vh_shift;
};
__device__ __forceinline__ int c1_fastdiv(int n, uint32_t magic, uint32_t shift) {
    return (int)((__umulhi((uint32_t)n, magic) + (uint32_t)n) >> shift);
}

template <int KS, int CT>   // CT = Cout / 16
__global__ __launch_bounds__(256) void conv1_fwd_mfma_kernel(const float* __restrict__ X, const int32_t* __restrict__ idx, int64_t row0,
                                                             const float* __restrict__ Wt, const float* __restrict__ bias,
                                                             float* __restrict__ Y, Conv1Dev g, int relu,
                                                             const StepState* __restrict__ st, int64_t n_rows,
                                                             float* __restrict__ stats) {
    constexpr int R = KS / 2, T = KS * KS, NJ = (T + 3) / 4, BM = 256, RT = 4, NIT = 4;
    extern __shared__ __attribute__((aligned(16))) float c1_lds[];
    float* const img = c1_lds;                                                   // [rows_max][WP]
    long long* const row_src = reinterpret_cast<long long*>(c1_lds + g.rows_max * g.WP);   // element offset of each halo row's x = 0, or -1
    if (st) row0 = st->row0;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lr = lane & 15, q = lane >> 4;
    const int m0 = blockIdx.x * BM, N = g.Cout;
    auto vrow = [&](int m, int& x) {
        const int b = c1_fastdiv(m, g.hw_magic, g.hw_shift), r = m - b * (g.H * g.W);
        const int y = c1_fastdiv(r, g.w_magic, g.w_shift);
        x = r - y * g.W;
        return b * g.VH + y;
    };
    int xd;
    const int vbase = vrow(m0, xd), vlast = vrow(min(m0 + BM, g.M) - 1, xd);
    const int nrows = vlast - vbase + 1 + 2 * R;
    if (t < g.rows_max) {
        const int v = vbase - R + t, vc = max(v, 0);
        const int b = c1_fastdiv(vc, g.vh_magic, g.vh_shift), y = vc - b * g.VH;
        const bool ok = t < nrows && v >= 0 && b < g.B && y < g.H;
        row_src[t] = ok ? gather_row(idx, row0 + b, n_rows) * (long long)(g.H * g.W) + (long long)y * g.W : -1ll;
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < NIT; ++it) {
        const int i = t + 256 * it;
        if (i < g.rows_max * g.WP) {
            const int hy = c1_fastdiv(i, g.wp_magic, g.wp_shift), x = i - hy * g.WP - R;
            const long long src = row_src[hy];
            img[i] = (src >= 0 && (unsigned)x < (unsigned)g.W) ? X[src + x] : 0.f;
        }
    }
    // weights: lane (co = 16 ct + lr, k slot q) holds tap 4 j + q of its output channel for the j-th MFMA (zero past the window)
    float bw[CT][NJ];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
        for (int j = 0; j < NJ; ++j) bw[ct][j] = (4 * j + q < T) ? Wt[(ct * 16 + lr) * T + 4 * j + q] : 0.f;
    // this lane's tap offsets inside the halo image, and its four pixels
    int tap_off[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        const int tap = min(4 * j + q, T - 1), ky = tap / KS;
        tap_off[j] = ky * g.WP + (tap - ky * KS);
    }
    int a_base[RT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt) {
        int x;
        const int v = vrow(min(m0 + wave * 64 + rt * 16 + lr, g.M - 1), x);
        a_base[rt] = (v - vbase) * g.WP + x;
    }
    f32x4 acc[RT][CT];
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = f32x4{0.f, 0.f, 0.f, 0.f};
    __syncthreads();
#pragma unroll
    for (int rt = 0; rt < RT; ++rt)
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            float a = img[a_base[rt] + tap_off[j]];
            if (4 * j + q >= T) a = 0.f;                   // the padded K slots: 0 x W(0) even if the image held a non-finite value
#pragma unroll
            for (int ct = 0; ct < CT; ++ct) acc[rt][ct] = __builtin_amdgcn_mfma_f32_16x16x4f32(a, bw[ct][j], acc[rt][ct], 0, 0, 0);
        }

    // epilogue (C/D map of 16x16x4: col = lane & 15, row = 4 (lane >> 4) + reg); whole tiles take the straight-line form
    float csum[CT], csq[CT], bias_v[CT];
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) { csum[ct] = 0.f; csq[ct] = 0.f; bias_v[ct] = bias[ct * 16 + lr]; }
    if (m0 + BM <= g.M) {
        const __amdgpu_buffer_rsrc_t yrs = __builtin_amdgcn_make_buffer_rsrc(Y, 0, g.M * N * 4, 0x00020000);
        const uint32_t e_lane = (uint32_t)((m0 + wave * 64 + q * 4) * N + lr) * 4u;
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int soff = (rt * 16 + r) * N * 4;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    float v = acc[rt][ct][r] + bias_v[ct];
                    v = relu ? fmaxf(v, 0.f) : v;
                    __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(v), yrs, (int)(e_lane + ct * 64), soff, 0);
                    csum[ct] += v; csq[ct] += v * v;
                }
            }
    } else {
#pragma unroll
        for (int rt = 0; rt < RT; ++rt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = m0 + wave * 64 + rt * 16 + q * 4 + r;
                if (row >= g.M) continue;
#pragma unroll
                for (int ct = 0; ct < CT; ++ct) {
                    float v = acc[rt][ct][r] + bias_v[ct];
                    v = relu ? fmaxf(v, 0.f) : v;
                    Y[(size_t)row * N + ct * 16 + lr] = v;
                    csum[ct] += v; csq[ct] += v * v;
                }
            }
    }
    if (stats) {   // column partials of this tile: lane's rows -> the wave's four row groups (shuffle) -> the four waves (LDS), fixed order
        __syncthreads();
        float* red = c1_lds;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) {
            csum[ct] += __shfl_xor(csum[ct], 16, 64); csq[ct] += __shfl_xor(csq[ct], 16, 64);
            csum[ct] += __shfl_xor(csum[ct], 32, 64); csq[ct] += __shfl_xor(csq[ct], 32, 64);
            if (q == 0) { red[(wave * N + ct * 16 + lr) * 2] = csum[ct]; red[(wave * N + ct * 16 + lr) * 2 + 1] = csq[ct]; }
        }
        __syncthreads();
        if (t < N) {
            float a = 0.f, b = 0.f;
#pragma unroll
            for (int w = 0; w < 4; ++w) { a += red[(w * N + t) * 2]; b += red[(w * N + t) * 2 + 1]; }
            stats[((size_t)blockIdx.x * 2) * N + t] = a;
            stats[((size_t)blockIdx.x * 2 + 1) * N + t] = b;
        }
    }
}

void launch_conv1_fwd(const float* X, const BatchRows& batch, const float* Wt, const float* bias, float* Y, int B, int H, int W,
                      int Cout, int KS, int relu, hipStream_t s, float* stats, int* stats_blocks) {
    CMOOP_REQUIRE(Cout % 4 == 0 && Cout <= 64 && 64 % (Cout / 4) == 0 && (KS == 3 || KS == 5), "conv1: unsupported shape");
    if (stats_blocks) *stats_blocks = 0;
    // matrix-core form (default; CMOOP_CONV1_MFMA=0 keeps the VALU kernel): C_out a multiple of 16, halo image within the staging slots
    static const bool mfma_on = [] { const char* v = std::getenv("CMOOP_CONV1_MFMA"); return !(v && v[0] == '0'); }();
    {
        const int R = KS / 2, wp = (W + KS - 1 + 7) / 8 * 8;
        const int span = (256 - 2 + W) / W + 1 + ((256 - 1) / (H * W) + 1) * R, rows = span + 2 * R;
        const int64_t M = (int64_t)B * H * W;
        if (mfma_on && (Cout == 16 || Cout == 32 || Cout == 64) && rows * wp <= 4 * 256 && rows <= 256 && M > 0 && M * Cout < (1ll << 29)) {
            Conv1Dev g;
            g.B = B; g.H = H; g.W = W; g.Cout = Cout; g.M = (int)M; g.WP = wp; g.VH = H + R; g.rows_max = rows;
            fastdiv_init(H * W, &g.hw_magic, &g.hw_shift);
            fastdiv_init(W, &g.w_magic, &g.w_shift);
            fastdiv_init(wp, &g.wp_magic, &g.wp_shift);
            fastdiv_init(H + R, &g.vh_magic, &g.vh_shift);
            const size_t lds = std::max((size_t)rows * wp * 4 + (size_t)rows * 8, (size_t)4 * Cout * 2 * 4);
            const dim3 grid((unsigned)cdiv64(M, 256));
#define CMOOP_C1(KS_, CT_) hipLaunchKernelGGL((conv1_fwd_mfma_kernel<KS_, CT_>), grid, dim3(256), lds, s, X, batch.idx, batch.row0, Wt, bias, Y, g, relu, batch.st, batch.n_rows, stats)
            if (KS == 3) { if (Cout == 16) CMOOP_C1(3, 1); else if (Cout == 32) CMOOP_C1(3, 2); else CMOOP_C1(3, 4); }
            else         { if (Cout == 16) CMOOP_C1(5, 1); else if (Cout == 32) CMOOP_C1(5, 2); else CMOOP_C1(5, 4); }
#undef CMOOP_C1
            CMOOP_HIP(hipGetLastError());
            if (stats && stats_blocks) *stats_blocks = (int)grid.x;
            return;
        }
    }
    const int GPB = 256 / (Cout / 4);
    const int64_t groups = (int64_t)B * H * ((W + 3) / 4);
    if (groups == 0) return;
    const dim3 grid((unsigned)cdiv64(groups, GPB));
    if (KS == 3) hipLaunchKernelGGL(conv1_fwd_kernel<3>, grid, dim3(256), 0, s, X, batch.idx, batch.row0, Wt, bias, Y, B, H, W, Cout, relu, batch.st, batch.n_rows);
    else hipLaunchKernelGGL(conv1_fwd_kernel<5>, grid, dim3(256), 0, s, X, batch.idx, batch.row0, Wt, bias, Y, B, H, W, Cout, relu, batch.st, batch.n_rows);
    CMOOP_HIP(hipGetLastError());
}

// partial slabs of the first layer's weight gradient: one per workgroup = (sample, chunk of image rows); ~512 chip-wide
static int conv1_row_chunks(int B, int H) { return std::max(1, std::min(H, 512 / std::max(B, 1))); }
int conv1_wgrad_blocks(int B, int H, int W) {
    (void)W;
    return std::max(1, B) * conv1_row_chunks(B, H);
}

template <int KS>
__global__ __launch_bounds__(256) void conv1_wgrad_kernel(const float* __restrict__ X, const int32_t* __restrict__ idx,
                                                          int64_t row0, const float* __restrict__ dY,
                                                          float* __restrict__ P, int B, int H, int W, int Cout,
                                                          const StepState* __restrict__ st, int64_t n_rows) {
    constexpr int TAPS = KS * KS, SEG = 4 + KS - 1, p = (KS - 1) >> 1;
    __shared__ float red[4 * (TAPS + 1) * 64];
    if (st) row0 = st->row0;
    const int t = threadIdx.x;
    const int TPG = Cout >> 2, GPB = 256 / TPG;
    const int gl = t / TPG, c4 = t % TPG;
    const int W4 = (W + 3) >> 2;
    const int64_t groups = (int64_t)B * H * W4;
    f32x4 acc[TAPS + 1];
#pragma unroll
    for (int i = 0; i <= TAPS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int64_t group = (int64_t)blockIdx.x * GPB + gl; group < groups; group += (int64_t)gridDim.x * GPB) {
        const int b = (int)(group / (H * W4)), r = (int)(group - (int64_t)b * H * W4);
        const int h = r / W4, w0 = (r - h * W4) * 4;
        const int64_t src = gather_row(idx, row0 + b, n_rows);
        const float* xb = X + src * (int64_t)H * W;
        const int64_t pix0 = ((int64_t)b * H + h) * W + w0;
        f32x4 dy[4];
#pragma unroll
        for (int px = 0; px < 4; ++px) {
            dy[px] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (w0 + px < W) dy[px] = *reinterpret_cast<const f32x4*>(dY + (pix0 + px) * Cout + 4 * c4);
            acc[TAPS] += dy[px];
        }
#pragma unroll
        for (int kh = 0; kh < KS; ++kh) {
            const int ih = h + kh - p;
            if ((unsigned)ih >= (unsigned)H) continue;
            float xr[SEG];
#pragma unroll
            for (int j = 0; j < SEG; ++j) {
                const int iw = w0 - p + j;
                xr[j] = (unsigned)iw < (unsigned)W ? xb[ih * W + iw] : 0.f;
            }
#pragma unroll
            for (int kw = 0; kw < KS; ++kw) {
                f32x4& a = acc[kh * KS + kw];
#pragma unroll
                for (int px = 0; px < 4; ++px) {
                    const float xv = xr[px + kw];
                    a[0] = fmaf(xv, dy[px][0], a[0]); a[1] = fmaf(xv, dy[px][1], a[1]);
                    a[2] = fmaf(xv, dy[px][2], a[2]); a[3] = fmaf(xv, dy[px][3], a[3]);
                }
            }
        }
    }
    // lanes sharing c4 sit TPG apart inside the wave: butterfly down to TPG
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int i = 0; i <= TAPS; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = acc[i][j];
            for (int off = 32; off >= TPG; off >>= 1) v += __shfl_xor(v, off, 64);
            acc[i][j] = v;
        }
    if (lane < TPG) {
#pragma unroll
        for (int i = 0; i <= TAPS; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) red[(wave * (TAPS + 1) + i) * 64 + 4 * c4 + j] = acc[i][j];
    }
    __syncthreads();
    float* Pb = P + (size_t)blockIdx.x * (Cout * (TAPS + 1));
    for (int i = t; i < (TAPS + 1) * Cout; i += 256) {
        const int tap = i / Cout, co = i - tap * Cout;
        float v = red[(0 * (TAPS + 1) + tap) * 64 + co] + red[(1 * (TAPS + 1) + tap) * 64 + co];
        v += red[(2 * (TAPS + 1) + tap) * 64 + co];
        v += red[(3 * (TAPS + 1) + tap) * 64 + co];
        if (tap < TAPS) Pb[co * TAPS + tap] = v;        // kernel grad, canonical [co][tap]
        else Pb[Cout * TAPS + co] = v;                  // bias grad
    }
}

// The same gradient on the matrix cores (Cout in {16, 32, 64}: the search space): dW[tap][co] = sum over pixels of
// x[pixel + tap] * dY[pixel][co] is a [taps x pixels] x [pixels x Cout] product with a 66 MB reduction axis for 1.7 k
// outputs.  One v_mfma_f32_16x16x4_f32 reduces FOUR pixels: lane (lr, q) supplies A[tap 16 tt + lr][pixel q] -- its own
// tap's shifted input value, a gather from the 16 KB image (L1) -- and B[pixel q][column lr]; the bias gradient is the
// extra "tap" whose input is the constant 1.  dY is read once, as one 16 / 8 / 4-byte load per lane of NCH consecutive
// channels: MFMA j of a group uses component j, so column lr of accumulator j IS channel NCH*lr + j (a permutation of
// the output columns, undone when the tile is written).  Workgroup = (sample, row chunk); its four waves take rows
// h, h+4, ...; U groups of 4 pixels have their loads in flight together.  The VALU form above took 49 us per step on
// 64 filters k5 (104 accumulator registers, 40 scalar loads per 400 FMAs); the floor here is the 66 MB read of dY.
template <int KS, int NCH, int U>
__global__ __launch_bounds__(256) void conv1_wgrad_mfma_kernel(const float* __restrict__ X, const int32_t* __restrict__ idx,
                                                               int64_t row0, const float* __restrict__ dY,
                                                               float* __restrict__ P, int H, int W, int RC,
                                                               const StepState* __restrict__ st, int64_t n_rows) {
    constexpr int TAPS = KS * KS, TT = (TAPS + 1 + 15) / 16, pad = (KS - 1) >> 1, Cout = 16 * NCH;
    typedef float dyvec __attribute__((ext_vector_type(NCH)));
    __shared__ __attribute__((aligned(16))) float red[3 * TT * NCH * 256];
    if (st) row0 = st->row0;
    const int t = threadIdx.x, wave = t >> 6, lane = t & 63, lr = lane & 15, q = lane >> 4;
    const int b = blockIdx.x / RC, rc = blockIdx.x - b * RC;
    const int rows_per = (H + RC - 1) / RC;
    const int h_begin = rc * rows_per, h_end = min(H, h_begin + rows_per);
    const int64_t src = gather_row(idx, row0 + b, n_rows);
    const float* xb = X + src * (int64_t)H * W;
    const float* dyb = dY + (int64_t)b * H * W * Cout + NCH * lr;
    int dh[TT], dw[TT], kind[TT];   // kind 0: a real tap (input shifted by dh, dw); 1: the bias row (input 1); 2: unused row
#pragma unroll
    for (int tt = 0; tt < TT; ++tt) {
        const int tap = tt * 16 + lr;
        kind[tt] = tap < TAPS ? 0 : (tap == TAPS ? 1 : 2);
        dh[tt] = tap < TAPS ? tap / KS - pad : 0;
        dw[tt] = tap < TAPS ? tap % KS - pad : 0;
    }
    f32x4 acc[TT][NCH];
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int j = 0; j < NCH; ++j) acc[tt][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int h = h_begin + wave; h < h_end; h += 4) {
        const float* xrow[TT];
        bool rok[TT];
#pragma unroll
        for (int tt = 0; tt < TT; ++tt) {
            const int ih = h + dh[tt];
            rok[tt] = kind[tt] == 0 && (unsigned)ih < (unsigned)H;
            xrow[tt] = xb + (rok[tt] ? ih : 0) * W + dw[tt];
        }
        const float* dyrow = dyb + (int64_t)h * W * Cout;
        for (int w0 = 0; w0 < W; w0 += 4 * U) {
            float a[U][TT];
            dyvec d[U];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                const int w = w0 + 4 * u + q;
                const bool ok = w < W;
#pragma unroll
                for (int j = 0; j < NCH; ++j) d[u][j] = 0.f;
                if (ok) d[u] = *reinterpret_cast<const dyvec*>(dyrow + (int64_t)w * Cout);
#pragma unroll
                for (int tt = 0; tt < TT; ++tt) {
                    const bool in = ok && rok[tt] && (unsigned)(w + dw[tt]) < (unsigned)W;
                    const float xv = in ? xrow[tt][w] : 0.f;
                    a[u][tt] = kind[tt] == 1 ? 1.f : xv;      // where the pixel is outside the row, dY is 0
                }
            }
#pragma unroll
            for (int u = 0; u < U; ++u)
#pragma unroll
                for (int tt = 0; tt < TT; ++tt)
#pragma unroll
                    for (int j = 0; j < NCH; ++j)
                        acc[tt][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(a[u][tt], d[u][j], acc[tt][j], 0, 0, 0);
        }
    }
    // waves 1..3 park their tiles, wave 0 adds them in wave order and writes the slab
    if (wave > 0) {
#pragma unroll
        for (int tt = 0; tt < TT; ++tt)
#pragma unroll
            for (int j = 0; j < NCH; ++j)
                *reinterpret_cast<f32x4*>(&red[(((wave - 1) * TT + tt) * NCH + j) * 256 + lane * 4]) = acc[tt][j];
    }
    __syncthreads();
    if (wave != 0) return;
    float* Pb = P + (size_t)blockIdx.x * (Cout * (TAPS + 1));
#pragma unroll
    for (int tt = 0; tt < TT; ++tt)
#pragma unroll
        for (int j = 0; j < NCH; ++j) {
            f32x4 v = acc[tt][j];
#pragma unroll
            for (int w = 0; w < 3; ++w) v += *reinterpret_cast<const f32x4*>(&red[((w * TT + tt) * NCH + j) * 256 + lane * 4]);
            const int co = NCH * lr + j;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int tap = tt * 16 + 4 * q + r;
                if (tap < TAPS) Pb[co * TAPS + tap] = v[r];           // kernel grad, canonical [co][tap]
                else if (tap == TAPS) Pb[Cout * TAPS + co] = v[r];    // bias grad
            }
        }
}

template <int KS, int NCH>
static void launch_conv1_wgrad_mfma(const float* X, const BatchRows& rows, const float* dY, float* P, int B, int H, int W,
                                    hipStream_t s) {
    const int RC = conv1_row_chunks(B, H), W4 = (W + 3) / 4;
    const dim3 grid((unsigned)(B * RC));
    // groups of 4 pixels per row, U at a time: pick the U that wastes no masked group (W = 40: 10 groups = 2 x 5)
    if (W4 % 5 == 0)
        hipLaunchKernelGGL((conv1_wgrad_mfma_kernel<KS, NCH, 5>), grid, dim3(256), 0, s, X, rows.idx, rows.row0, dY, P, H, W, RC, rows.st, rows.n_rows);
    else if (W4 % 3 == 0 && W4 % 4 != 0)
        hipLaunchKernelGGL((conv1_wgrad_mfma_kernel<KS, NCH, 3>), grid, dim3(256), 0, s, X, rows.idx, rows.row0, dY, P, H, W, RC, rows.st, rows.n_rows);
    else
        hipLaunchKernelGGL((conv1_wgrad_mfma_kernel<KS, NCH, 4>), grid, dim3(256), 0, s, X, rows.idx, rows.row0, dY, P, H, W, RC, rows.st, rows.n_rows);
}

void launch_conv1_wgrad(const float* X, const BatchRows& rows, const float* dY, float* P, int B, int H, int W, int Cout, int KS,
                        hipStream_t s) {
    CMOOP_REQUIRE(Cout % 4 == 0 && Cout <= 64 && 64 % (Cout / 4) == 0, "conv1 wgrad: unsupported Cout");
    if (B == 0) return;
    if ((Cout == 16 || Cout == 32 || Cout == 64) && (KS == 3 || KS == 5)) {
        const int nch = Cout / 16;
        if (KS == 3) {
            if (nch == 1) launch_conv1_wgrad_mfma<3, 1>(X, rows, dY, P, B, H, W, s);
            else if (nch == 2) launch_conv1_wgrad_mfma<3, 2>(X, rows, dY, P, B, H, W, s);
            else launch_conv1_wgrad_mfma<3, 4>(X, rows, dY, P, B, H, W, s);
        } else {
            if (nch == 1) launch_conv1_wgrad_mfma<5, 1>(X, rows, dY, P, B, H, W, s);
            else if (nch == 2) launch_conv1_wgrad_mfma<5, 2>(X, rows, dY, P, B, H, W, s);
            else launch_conv1_wgrad_mfma<5, 4>(X, rows, dY, P, B, H, W, s);
        }
        CMOOP_HIP(hipGetLastError());
        return;
    }
    const int nb = conv1_wgrad_blocks(B, H, W);
    if (KS == 3) hipLaunchKernelGGL(conv1_wgrad_kernel<3>, dim3(nb), dim3(256), 0, s, X, rows.idx, rows.row0, dY, P, B, H, W, Cout, rows.st, rows.n_rows);
    else if (KS == 5) hipLaunchKernelGGL(conv1_wgrad_kernel<5>, dim3(nb), dim3(256), 0, s, X, rows.idx, rows.row0, dY, P, B, H, W, Cout, rows.st, rows.n_rows);
    else CMOOP_REQUIRE(false, "conv1 wgrad: kernel size must be 3 or 5");
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
