// HBM-bound kernels of the candidate-training path: first-layer direct conv,
// BatchNorm (train / eval / backward), max-pool, residual add, GAP, softmax-CE,
// Adam, confusion matrix.  All loads/stores are float4 along the channel axis of
// NHWC tensors (coalesced 16 B/lane); every cross-thread sum has a fixed order so
// a training run is bit-reproducible.
#include "kernels.h"
#include <cstdlib>
#include <algorithm>
#include <cmath>
#include <mutex>

namespace cmoop {

typedef float f32x4 __attribute__((ext_vector_type(4)));

// row of the resident tensor a batch position maps to: idx[pos] (the epoch permutation) or pos itself; with n_rows > 0
// the result is clamped into [0, n_rows): a corrupt index can then mis-train but never fault
__device__ __forceinline__ int64_t gather_row(const int32_t* __restrict__ idx, int64_t pos, int64_t n_rows) {
    int64_t src = idx ? (int64_t)idx[pos] : pos;
    if (n_rows > 0) src = src < 0 ? 0 : (src >= n_rows ? n_rows - 1 : src);
    return src;
}

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
static void c1_fastdiv_init(int d, uint32_t* magic, uint32_t* shift) {     // Granlund-Montgomery, exact for n < 2^31 (as in gemm.hip)
    uint32_t sh = 0;
    while ((1u << sh) < (uint32_t)d) ++sh;
    *shift = sh;
    *magic = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << sh) - (uint64_t)d)) / (uint64_t)d + 1);
}
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
            c1_fastdiv_init(H * W, &g.hw_magic, &g.hw_shift);
            c1_fastdiv_init(W, &g.w_magic, &g.w_shift);
            c1_fastdiv_init(wp, &g.wp_magic, &g.wp_shift);
            c1_fastdiv_init(H + R, &g.vh_magic, &g.vh_shift);
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

// ===========================================================================
// per-channel reductions over [M][C]
// ===========================================================================
int colreduce_blocks(int64_t M, int C) {
    const int lanes = C / 4;
    const int rpp = std::max(1, 256 / lanes);
    int64_t nb = cdiv64(M, (int64_t)rpp * 16);
    return (int)std::max<int64_t>(1, std::min<int64_t>(1024, nb));
}

struct StatsOp {   // (sum x, sum x^2)
    const float* X;
    __device__ void operator()(size_t off, int, f32x4& s0, f32x4& s1) const {
        f32x4 x = *reinterpret_cast<const f32x4*>(X + off);
        s0 += x;
        s1 += x * x;
    }
};
struct BnBwdOp {   // (sum dy, sum dy * xhat)
    const float* dY; const float* X; const float* mean; const float* invstd;
    __device__ void operator()(size_t off, int c, f32x4& s0, f32x4& s1) const {
        f32x4 dy = *reinterpret_cast<const f32x4*>(dY + off);
        f32x4 x = *reinterpret_cast<const f32x4*>(X + off);
        f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
        f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
        s0 += dy;
        s1 += dy * ((x - mu) * is);
    }
};

template <class Op>
__global__ __launch_bounds__(256) void colreduce_kernel(Op op, float* __restrict__ P, int64_t M, int C, int64_t rows_per_block) {
    __shared__ __attribute__((aligned(16))) float red[256 * 8];
    const int t = threadIdx.x;
    const int lanes = C >> 2;
    const int rpp = 256 / lanes;
    const int rl = t / lanes, cl = t - rl * lanes;
    f32x4 s0 = {0.f, 0.f, 0.f, 0.f}, s1 = {0.f, 0.f, 0.f, 0.f};
    const int64_t rbeg = (int64_t)blockIdx.x * rows_per_block;
    const int64_t rend = min(M, rbeg + rows_per_block);
    if (rl < rpp)
        for (int64_t r = rbeg + rl; r < rend; r += rpp) op((size_t)r * C + 4 * cl, 4 * cl, s0, s1);
    *reinterpret_cast<f32x4*>(&red[t * 8]) = s0;
    *reinterpret_cast<f32x4*>(&red[t * 8 + 4]) = s1;
    __syncthreads();
    if (rl == 0 && cl < lanes) {
        for (int r = 1; r < rpp; ++r) {
            s0 += *reinterpret_cast<const f32x4*>(&red[(r * lanes + cl) * 8]);
            s1 += *reinterpret_cast<const f32x4*>(&red[(r * lanes + cl) * 8 + 4]);
        }
        float* Pb = P + (size_t)blockIdx.x * 2 * C;
        *reinterpret_cast<f32x4*>(Pb + 4 * cl) = s0;
        *reinterpret_cast<f32x4*>(Pb + C + 4 * cl) = s1;
    }
}

static void check_colreduce(int64_t M, int C) {
    CMOOP_REQUIRE(C % 4 == 0 && C / 4 <= 256 && C >= 4, "colreduce: C must be a multiple of 4, <= 1024");
    (void)M;
}

void launch_colstats(const float* X, float* P, int64_t M, int C, int blocks, hipStream_t s) {
    check_colreduce(M, C);
    StatsOp op{X};
    hipLaunchKernelGGL((colreduce_kernel<StatsOp>), dim3(blocks), dim3(256), 0, s, op, P, M, C, cdiv64(M, blocks));
    CMOOP_HIP(hipGetLastError());
}

void launch_bn_bwd_reduce(const float* dY, const float* X, const float* mean, const float* invstd, float* P,
                          int64_t M, int C, int blocks, hipStream_t s) {
    check_colreduce(M, C);
    BnBwdOp op{dY, X, mean, invstd};
    hipLaunchKernelGGL((colreduce_kernel<BnBwdOp>), dim3(blocks), dim3(256), 0, s, op, P, M, C, cdiv64(M, blocks));
    CMOOP_HIP(hipGetLastError());
}

// Per-channel totals of the [blocks][2][C] partials a reduction (or a conv epilogue) left: PS_CH channels per workgroup,
// 64 lanes per channel, lane l sums partials l, l+64, ... into four independent double accumulators (eight loads in
// flight: the 4 040 partials of a 101x40 layer are 16 rounds, not 126), then lane 0 adds the 64 lane sums in lane order.
constexpr int PS_CH = 4;
__device__ __forceinline__ bool partial_sums(const float* __restrict__ P, int blocks, int C, double* s1, double* s2,
                                             int* c_out) {
    __shared__ double sh[2][PS_CH][64];
    const int cl = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int c = blockIdx.x * PS_CH + cl;
    double a[4] = {0.0, 0.0, 0.0, 0.0}, b[4] = {0.0, 0.0, 0.0, 0.0};
    if (c < C) {
        int blk = lane;
        for (; blk + 192 < blocks; blk += 256) {
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                a[u] += (double)P[(size_t)(blk + 64 * u) * 2 * C + c];
                b[u] += (double)P[(size_t)(blk + 64 * u) * 2 * C + C + c];
            }
        }
        for (; blk < blocks; blk += 64) {
            a[0] += (double)P[(size_t)blk * 2 * C + c];
            b[0] += (double)P[(size_t)blk * 2 * C + C + c];
        }
    }
    sh[0][cl][lane] = (a[0] + a[1]) + (a[2] + a[3]);
    sh[1][cl][lane] = (b[0] + b[1]) + (b[2] + b[3]);
    __syncthreads();
    *c_out = c;
    if (lane != 0 || c >= C) return false;
    double x = 0.0, y = 0.0;
    for (int l = 0; l < 64; ++l) { x += sh[0][cl][l]; y += sh[1][cl][l]; }
    *s1 = x; *s2 = y;
    return true;
}

__global__ __launch_bounds__(256) void bn_finalize_kernel(const float* __restrict__ P, int blocks, int64_t M, int C,
                                   const float* __restrict__ gamma, const float* __restrict__ beta,
                                   float* __restrict__ mm, float* __restrict__ mv, float* __restrict__ mean,
                                   float* __restrict__ invstd, float* __restrict__ scale, float* __restrict__ shift,
                                   float eps, float momentum, float one_minus_momentum) {
    double s1, s2;
    int c;
    if (!partial_sums(P, blocks, C, &s1, &s2, &c)) return;
    const double mu = s1 / (double)M;
    double var = s2 / (double)M - mu * mu;
    if (var < 0.0) var = 0.0;
    const float muf = (float)mu, varf = (float)var;
    const float is = (float)(1.0 / sqrt((double)varf + (double)eps));
    const float sc = gamma[c] * is;
    mean[c] = muf;
    invstd[c] = is;
    scale[c] = sc;
    shift[c] = beta[c] - muf * sc;
    mm[c] = mm[c] * momentum + muf * one_minus_momentum;
    mv[c] = mv[c] * momentum + varf * one_minus_momentum;
}

void launch_bn_finalize(const float* P, int blocks, int64_t M, int C, const float* gamma, const float* beta,
                        float* moving_mean, float* moving_var, float* mean, float* invstd, float* scale, float* shift,
                        float eps, float momentum, float omm, hipStream_t s) {
    hipLaunchKernelGGL(bn_finalize_kernel, dim3(cdiv(C, PS_CH)), dim3(256), 0, s, P, blocks, M, C, gamma, beta, moving_mean,
                       moving_var, mean, invstd, scale, shift, eps, momentum, omm);
    CMOOP_HIP(hipGetLastError());
}

__global__ void bn_eval_prepare_kernel(const float* __restrict__ gamma, const float* __restrict__ beta,
                                       const float* __restrict__ mm, const float* __restrict__ mv,
                                       float* __restrict__ scale, float* __restrict__ shift, int C, float eps) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    const float is = (float)(1.0 / sqrt((double)mv[c] + (double)eps));
    const float sc = gamma[c] * is;
    scale[c] = sc;
    shift[c] = beta[c] - mm[c] * sc;
}

void launch_bn_eval_prepare(const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                            float* scale, float* shift, int C, float eps, hipStream_t s) {
    hipLaunchKernelGGL(bn_eval_prepare_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, gamma, beta, moving_mean, moving_var,
                       scale, shift, C, eps);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void scale_shift_kernel(const float* __restrict__ X, float* __restrict__ Y,
                                                          const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int64_t n4, int C, int relu) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        f32x4 x = *reinterpret_cast<const f32x4*>(X + i * 4);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + c);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + c);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float v = x[j] * sc[j] + sh[j];
            y[j] = relu ? fmaxf(v, 0.f) : v;
        }
        *reinterpret_cast<f32x4*>(Y + i * 4) = y;
    }
}

static inline unsigned ew_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n, 256), 8192)); }

void launch_scale_shift(const float* X, float* Y, const float* scale, const float* shift, int64_t M, int C, int relu,
                        hipStream_t s) {
    CMOOP_REQUIRE(C % 4 == 0, "scale_shift: C % 4");
    const int64_t n4 = M * C / 4;
    if (n4 == 0) return;
    hipLaunchKernelGGL(scale_shift_kernel, dim3(ew_grid(n4)), dim3(256), 0, s, X, Y, scale, shift, n4, C, relu);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void bn_bwd_finalize_kernel(const float* __restrict__ P, int blocks, int C,
                                                              float* __restrict__ sums, float* __restrict__ dgamma,
                                                              float* __restrict__ dbeta) {
    double s1, s2;
    int c;
    if (!partial_sums(P, blocks, C, &s1, &s2, &c)) return;
    sums[c] = (float)s1;
    sums[C + c] = (float)s2;
    dbeta[c] = (float)s1;
    dgamma[c] = (float)s2;
}

__global__ __launch_bounds__(256) void bn_bwd_apply_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ invstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ sums, float* __restrict__ dX,
                                                           int64_t n4, int C, float invM, int mask_x_pos) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 dy = *reinterpret_cast<const f32x4*>(dY + i * 4);
        const f32x4 x = *reinterpret_cast<const f32x4*>(X + i * 4);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
        const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c);
        const f32x4 s1 = *reinterpret_cast<const f32x4*>(sums + c);
        const f32x4 s2 = *reinterpret_cast<const f32x4*>(sums + C + c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (x[j] - mu[j]) * is[j];
            float v = ga[j] * is[j] * (dy[j] - s1[j] * invM - xh * (s2[j] * invM));
            if (mask_x_pos && !(x[j] > 0.f)) v = 0.f;
            o[j] = v;
        }
        *reinterpret_cast<f32x4*>(dX + i * 4) = o;
    }
}

void launch_bn_bwd_apply(const float* dY, const float* X, const float* mean, const float* invstd, const float* gamma,
                         const float* P, int blocks, float* dX, float* dgamma, float* dbeta, int64_t M, int C,
                         int mask_x_pos, hipStream_t s) {
    // sums live right after the partials (caller reserves 2*C floats there)
    float* sums = const_cast<float*>(P) + (size_t)blocks * 2 * C;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, PS_CH)), dim3(256), 0, s, P, blocks, C, sums, dgamma, dbeta);
    CMOOP_HIP(hipGetLastError());
    const int64_t n4 = M * C / 4;
    if (n4 == 0) return;
    hipLaunchKernelGGL(bn_bwd_apply_kernel, dim3(ew_grid(n4)), dim3(256), 0, s, dY, X, mean, invstd, gamma, sums, dX, n4,
                       C, (float)(1.0 / (double)M), mask_x_pos);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void colsum_finalize_kernel(const float* __restrict__ P, int blocks, int C,
                                                              float* __restrict__ out) {
    double s1, s2;
    int c;
    if (!partial_sums(P, blocks, C, &s1, &s2, &c)) return;
    out[c] = (float)s1;
}

void launch_colsum_finalize(const float* P, int blocks, int C, float* out, hipStream_t s) {
    hipLaunchKernelGGL(colsum_finalize_kernel, dim3(cdiv(C, PS_CH)), dim3(256), 0, s, P, blocks, C, out);
    CMOOP_HIP(hipGetLastError());
}

// tiny helpers for the output layer (C_out = classes is not a multiple of 4 / power of two)
__global__ void colsum_small_kernel(const float* __restrict__ X, float* __restrict__ out, int M, int C) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= C) return;
    float s = 0.f;
    for (int m = 0; m < M; ++m) s += X[(size_t)m * C + c];
    out[c] = s;
}

void launch_colsum_small(const float* X, float* out, int M, int C, hipStream_t s) {
    hipLaunchKernelGGL(colsum_small_kernel, dim3(cdiv(C, 64)), dim3(64), 0, s, X, out, M, C);
    CMOOP_HIP(hipGetLastError());
}

// dX[m][i] = sum_o dY[m][o] * W[o][i], optionally masked by (mask[m][i] > 0) * scale
__global__ __launch_bounds__(256) void dense_dgrad_small_kernel(const float* __restrict__ dY, const float* __restrict__ W,
                                                                float* __restrict__ dX, int M, int N, int K,
                                                                const float* __restrict__ mask, float scale) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= M * K) return;
    const int m = i / K, k = i - m * K;
    float s = 0.f;
    for (int o = 0; o < N; ++o) s = fmaf(dY[(size_t)m * N + o], W[(size_t)o * K + k], s);
    if (mask) s = mask[i] > 0.f ? s * scale : 0.f;
    dX[i] = s;
}

void launch_dense_dgrad_small(const float* dY, const float* W, float* dX, int M, int N, int K, const float* mask,
                              float scale, hipStream_t s) {
    if (M * K == 0) return;
    hipLaunchKernelGGL(dense_dgrad_small_kernel, dim3(cdiv(M * K, 256)), dim3(256), 0, s, dY, W, dX, M, N, K, mask, scale);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// MaxPooling2D((2,2), strides 2, padding='same'): out = ceil(n/2), the window is
// clipped at the bottom/right edge (TF pads with -inf).  First max wins ties.
// ===========================================================================
__global__ __launch_bounds__(256) void maxpool_fwd_kernel(const float* __restrict__ X, float* __restrict__ Y,
                                                          uint8_t* __restrict__ arg, int B, int H, int W, int C, int OH,
                                                          int OW) {
    const int C4 = C >> 2;
    const int64_t n = (int64_t)B * OH * OW * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        int64_t p = i / C4;
        const int ow = (int)(p % OW); p /= OW;
        const int oh = (int)(p % OH);
        const int b = (int)(p / OH);
        f32x4 best;
        uchar4 a = {0, 0, 0, 0};
        bool first = true;
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) {
            const int ih = 2 * oh + (pos >> 1), iw = 2 * ow + (pos & 1);
            if (ih >= H || iw >= W) continue;
            const f32x4 v = *reinterpret_cast<const f32x4*>(X + ((size_t)(b * H + ih) * W + iw) * C + 4 * c4);
            if (first) { best = v; first = false; continue; }
            if (v[0] > best[0]) { best[0] = v[0]; a.x = pos; }
            if (v[1] > best[1]) { best[1] = v[1]; a.y = pos; }
            if (v[2] > best[2]) { best[2] = v[2]; a.z = pos; }
            if (v[3] > best[3]) { best[3] = v[3]; a.w = pos; }
        }
        *reinterpret_cast<f32x4*>(Y + i * 4) = best;
        *reinterpret_cast<uchar4*>(arg + i * 4) = a;
    }
}

void launch_maxpool_fwd(const float* X, float* Y, uint8_t* arg, int B, int H, int W, int C, hipStream_t s) {
    CMOOP_REQUIRE(C % 4 == 0, "maxpool: C % 4");
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    const int64_t n = (int64_t)B * OH * OW * (C / 4);
    if (n == 0) return;
    hipLaunchKernelGGL(maxpool_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, s, X, Y, arg, B, H, W, C, OH, OW);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void maxpool_bwd_kernel(const float* __restrict__ dY, const uint8_t* __restrict__ arg,
                                                          const float* __restrict__ Y, float* __restrict__ dX, int B,
                                                          int H, int W, int C, int OH, int OW, int mask_y_pos) {
    const int C4 = C >> 2;
    const int64_t n = (int64_t)B * OH * OW * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        int64_t p = i / C4;
        const int ow = (int)(p % OW); p /= OW;
        const int oh = (int)(p % OH);
        const int b = (int)(p / OH);
        f32x4 g = *reinterpret_cast<const f32x4*>(dY + i * 4);
        if (mask_y_pos) {
            const f32x4 y = *reinterpret_cast<const f32x4*>(Y + i * 4);
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (!(y[j] > 0.f)) g[j] = 0.f;
        }
        const uchar4 a = *reinterpret_cast<const uchar4*>(arg + i * 4);
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) {
            const int ih = 2 * oh + (pos >> 1), iw = 2 * ow + (pos & 1);
            if (ih >= H || iw >= W) continue;
            f32x4 o;
            o[0] = a.x == pos ? g[0] : 0.f; o[1] = a.y == pos ? g[1] : 0.f;
            o[2] = a.z == pos ? g[2] : 0.f; o[3] = a.w == pos ? g[3] : 0.f;
            *reinterpret_cast<f32x4*>(dX + ((size_t)(b * H + ih) * W + iw) * C + 4 * c4) = o;
        }
    }
}

void launch_maxpool_bwd(const float* dY, const uint8_t* arg, const float* Y, float* dX, int B, int H, int W, int C,
                        int mask_y_pos, hipStream_t s) {
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    const int64_t n = (int64_t)B * OH * OW * (C / 4);
    if (n == 0) return;
    hipLaunchKernelGGL(maxpool_bwd_kernel, dim3(ew_grid(n)), dim3(256), 0, s, dY, arg, Y, dX, B, H, W, C, OH, OW,
                       mask_y_pos);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// BatchNorm-apply (+ReLU) + MaxPool 2x2 SAME in one pass, and its backward twins: the normalised full-resolution
// tensor and its gradient are never written.  Arithmetic and tie rules are those of scale_shift_kernel followed by
// maxpool_fwd_kernel (bit-identical results); backward: dY_full[b,ih,iw,c] = (arg[b,oh,ow,c] == pos) ? g[b,oh,ow,c] : 0
// is formed on the fly where bn_bwd_reduce / bn_bwd_apply would have read the materialised tensor.
// ===========================================================================
__global__ __launch_bounds__(256) void bn_pool_fwd_kernel(const float* __restrict__ X, float* __restrict__ Y,
                                                          uint8_t* __restrict__ arg, const float* __restrict__ scale,
                                                          const float* __restrict__ shift, int B, int H, int W, int C,
                                                          int OH, int OW, int relu) {
    const int C4 = C >> 2;
    const int64_t n = (int64_t)B * OH * OW * C4;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int c4 = (int)(i % C4);
        int64_t p = i / C4;
        const int ow = (int)(p % OW); p /= OW;
        const int oh = (int)(p % OH);
        const int b = (int)(p / OH);
        const f32x4 sc = *reinterpret_cast<const f32x4*>(scale + 4 * c4);
        const f32x4 sh = *reinterpret_cast<const f32x4*>(shift + 4 * c4);
        f32x4 best;
        uchar4 a = {0, 0, 0, 0};
        bool first = true;
#pragma unroll
        for (int pos = 0; pos < 4; ++pos) {
            const int ih = 2 * oh + (pos >> 1), iw = 2 * ow + (pos & 1);
            if (ih >= H || iw >= W) continue;
            const f32x4 x = *reinterpret_cast<const f32x4*>(X + ((size_t)(b * H + ih) * W + iw) * C + 4 * c4);
            f32x4 v;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float t = x[j] * sc[j] + sh[j];
                v[j] = relu ? fmaxf(t, 0.f) : t;
            }
            if (first) { best = v; first = false; continue; }
            if (v[0] > best[0]) { best[0] = v[0]; a.x = pos; }
            if (v[1] > best[1]) { best[1] = v[1]; a.y = pos; }
            if (v[2] > best[2]) { best[2] = v[2]; a.z = pos; }
            if (v[3] > best[3]) { best[3] = v[3]; a.w = pos; }
        }
        *reinterpret_cast<f32x4*>(Y + i * 4) = best;
        *reinterpret_cast<uchar4*>(arg + i * 4) = a;
    }
}

void launch_bn_pool_fwd(const float* X, float* Y, uint8_t* arg, const float* scale, const float* shift, int B, int H, int W,
                        int C, int relu, hipStream_t s) {
    CMOOP_REQUIRE(C % 4 == 0, "bn_pool: C % 4");
    const int OH = (H + 1) / 2, OW = (W + 1) / 2;
    const int64_t n = (int64_t)B * OH * OW * (C / 4);
    if (n == 0) return;
    hipLaunchKernelGGL(bn_pool_fwd_kernel, dim3(ew_grid(n)), dim3(256), 0, s, X, Y, arg, scale, shift, B, H, W, C, OH, OW, relu);
    CMOOP_HIP(hipGetLastError());
}

// gradient of the (never materialised) BN output at full-resolution row r = (b, ih, iw), channels c..c+3
struct PooledGrad {
    const float* g; const uint8_t* arg;
    int H, W, OH, OW, C;
    __device__ __forceinline__ f32x4 at(int64_t row, int c) const {
        const int iw = (int)(row % W);
        const int64_t t = row / W;
        const int ih = (int)(t % H), b = (int)(t / H);
        const size_t o = (((size_t)b * OH + (ih >> 1)) * OW + (iw >> 1)) * C + c;
        const f32x4 gv = *reinterpret_cast<const f32x4*>(g + o);
        const uchar4 a = *reinterpret_cast<const uchar4*>(arg + o);
        const int pos = ((ih & 1) << 1) | (iw & 1);
        return f32x4{a.x == pos ? gv[0] : 0.f, a.y == pos ? gv[1] : 0.f, a.z == pos ? gv[2] : 0.f, a.w == pos ? gv[3] : 0.f};
    }
};

struct BnBwdPooledOp {   // (sum dy, sum dy * xhat) with dy scattered from the pooled gradient
    PooledGrad pg; const float* X; const float* mean; const float* invstd;
    __device__ void operator()(size_t off, int c, f32x4& s0, f32x4& s1) const {
        const f32x4 dy = pg.at((int64_t)(off / pg.C), c);
        const f32x4 x = *reinterpret_cast<const f32x4*>(X + off);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
        const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
        s0 += dy;
        s1 += dy * ((x - mu) * is);
    }
};

void launch_bn_pool_bwd_reduce(const float* g_pooled, const uint8_t* arg, const float* X, const float* mean, const float* invstd,
                               float* P, int B, int H, int W, int C, int blocks, hipStream_t s) {
    const int64_t M = (int64_t)B * H * W;
    check_colreduce(M, C);
    BnBwdPooledOp op{PooledGrad{g_pooled, arg, H, W, (H + 1) / 2, (W + 1) / 2, C}, X, mean, invstd};
    hipLaunchKernelGGL((colreduce_kernel<BnBwdPooledOp>), dim3(blocks), dim3(256), 0, s, op, P, M, C, cdiv64(M, blocks));
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void bn_pool_bwd_apply_kernel(PooledGrad pg, const float* __restrict__ X,
                                                                const float* __restrict__ mean,
                                                                const float* __restrict__ invstd,
                                                                const float* __restrict__ gamma,
                                                                const float* __restrict__ sums, float* __restrict__ dX,
                                                                int64_t n4, int C, float invM, int mask_x_pos) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int c = (int)((i * 4) % C);
        const f32x4 dy = pg.at((i * 4) / C, c);
        const f32x4 x = *reinterpret_cast<const f32x4*>(X + i * 4);
        const f32x4 mu = *reinterpret_cast<const f32x4*>(mean + c);
        const f32x4 is = *reinterpret_cast<const f32x4*>(invstd + c);
        const f32x4 ga = *reinterpret_cast<const f32x4*>(gamma + c);
        const f32x4 s1 = *reinterpret_cast<const f32x4*>(sums + c);
        const f32x4 s2 = *reinterpret_cast<const f32x4*>(sums + C + c);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float xh = (x[j] - mu[j]) * is[j];
            float v = ga[j] * is[j] * (dy[j] - s1[j] * invM - xh * (s2[j] * invM));
            if (mask_x_pos && !(x[j] > 0.f)) v = 0.f;
            o[j] = v;
        }
        *reinterpret_cast<f32x4*>(dX + i * 4) = o;
    }
}

void launch_bn_pool_bwd_apply(const float* g_pooled, const uint8_t* arg, const float* X, const float* mean, const float* invstd,
                              const float* gamma, const float* P, int blocks, float* dX, float* dgamma, float* dbeta, int B,
                              int H, int W, int C, int mask_x_pos, hipStream_t s) {
    const int64_t M = (int64_t)B * H * W;
    float* sums = const_cast<float*>(P) + (size_t)blocks * 2 * C;
    hipLaunchKernelGGL(bn_bwd_finalize_kernel, dim3(cdiv(C, PS_CH)), dim3(256), 0, s, P, blocks, C, sums, dgamma, dbeta);
    CMOOP_HIP(hipGetLastError());
    const int64_t n4 = M * C / 4;
    if (n4 == 0) return;
    PooledGrad pg{g_pooled, arg, H, W, (H + 1) / 2, (W + 1) / 2, C};
    hipLaunchKernelGGL(bn_pool_bwd_apply_kernel, dim3(ew_grid(n4)), dim3(256), 0, s, pg, X, mean, invstd, gamma, sums, dX, n4, C,
                       (float)(1.0 / (double)M), mask_x_pos);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void add_relu_kernel(const float* __restrict__ A, const float* __restrict__ Bt,
                                                       float* __restrict__ Y, int64_t n4) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(A + i * 4);
        const f32x4 b = *reinterpret_cast<const f32x4*>(Bt + i * 4);
        f32x4 y;
#pragma unroll
        for (int j = 0; j < 4; ++j) y[j] = fmaxf(a[j] + b[j], 0.f);
        *reinterpret_cast<f32x4*>(Y + i * 4) = y;
    }
}

void launch_add_relu(const float* A, const float* Bt, float* Y, int64_t n, hipStream_t s) {
    CMOOP_REQUIRE(n % 4 == 0, "add_relu: n % 4");
    if (n == 0) return;
    hipLaunchKernelGGL(add_relu_kernel, dim3(ew_grid(n / 4)), dim3(256), 0, s, A, Bt, Y, n / 4);
    CMOOP_HIP(hipGetLastError());
}

// GlobalAveragePooling2D: one workgroup per sample; lanes = channel quads, the remaining threads split the pixels;
// float4 loads, fixed-order LDS reduction over the pixel slices (the old one-thread-per-(b,c) loop took 69 us on a
// 26x10x32 tensor -- 12 % of a small candidate's step)
__global__ __launch_bounds__(256) void gap_fwd_kernel(const float* __restrict__ X, float* __restrict__ Y, int HW, int C,
                                                      float inv) {
    __shared__ __attribute__((aligned(16))) float red[256 * 4];
    const int t = threadIdx.x, lanes = C >> 2;
    const int slices = 256 / lanes;
    const int sl = t / lanes, cl = t - sl * lanes;
    const float* x = X + (size_t)blockIdx.x * HW * C + 4 * cl;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (sl < slices)
        for (int p = sl; p < HW; p += slices) s += *reinterpret_cast<const f32x4*>(x + (size_t)p * C);
    *reinterpret_cast<f32x4*>(&red[t * 4]) = s;
    __syncthreads();
    if (sl == 0) {
        for (int r = 1; r < slices; ++r) s += *reinterpret_cast<const f32x4*>(&red[(r * lanes + cl) * 4]);
        *reinterpret_cast<f32x4*>(Y + (size_t)blockIdx.x * C + 4 * cl) = s * inv;
    }
}

void launch_gap_fwd(const float* X, float* Y, int B, int HW, int C, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(C % 4 == 0 && C / 4 <= 256 && 256 % (C / 4) == 0, "gap: C must be 4 x a divisor of 256");
    hipLaunchKernelGGL(gap_fwd_kernel, dim3(B), dim3(256), 0, s, X, Y, HW, C, (float)(1.0 / HW));
    CMOOP_HIP(hipGetLastError());
}

// seeded glorot-uniform initial weights / constant fill (Net::build_plan)
__global__ __launch_bounds__(256) void glorot_init_kernel(float* __restrict__ w, int64_t n, uint32_t prefix, float scale) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const int u24 = (int)(fmix32(prefix ^ (uint32_t)i) >> 8);
        w[i] = (float)(2 * u24 - 16777216) * scale;
    }
}
void launch_glorot_init(float* w, int64_t n, uint32_t prefix, float scale, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(glorot_init_kernel, dim3(ew_grid(n)), dim3(256), 0, s, w, n, prefix, scale);
    CMOOP_HIP(hipGetLastError());
}
__global__ __launch_bounds__(256) void fill_kernel(float* __restrict__ w, float v, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) w[i] = v;
}
void launch_fill(float* w, float v, int64_t n, hipStream_t s) {
    if (n == 0) return;
    hipLaunchKernelGGL(fill_kernel, dim3(ew_grid(n)), dim3(256), 0, s, w, v, n);
    CMOOP_HIP(hipGetLastError());
}

__global__ void step_advance_kernel(StepState* st, int batch) {
    st->row0 += batch;
    st->step += 1;
    st->iter += 1;
}
void launch_step_advance(StepState* st, int batch, hipStream_t s) {
    hipLaunchKernelGGL(step_advance_kernel, dim3(1), dim3(1), 0, s, st, batch);
    CMOOP_HIP(hipGetLastError());
}

__global__ __launch_bounds__(256) void gap_bwd_kernel(const float* __restrict__ dY, const float* __restrict__ X,
                                                      float* __restrict__ dX, int64_t n4, int HW, int C, float inv) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n4; i += (int64_t)gridDim.x * 256) {
        const int64_t e = i * 4;
        const int c = (int)(e % C);
        const int64_t b = e / ((int64_t)HW * C);
        const f32x4 g = *reinterpret_cast<const f32x4*>(dY + b * C + c);
        const f32x4 x = *reinterpret_cast<const f32x4*>(X + e);
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = x[j] > 0.f ? g[j] * inv : 0.f;
        *reinterpret_cast<f32x4*>(dX + e) = o;
    }
}

void launch_gap_bwd(const float* dY, const float* X, float* dX, int B, int HW, int C, hipStream_t s) {
    const int64_t n4 = (int64_t)B * HW * C / 4;
    if (n4 == 0) return;
    hipLaunchKernelGGL(gap_bwd_kernel, dim3(ew_grid(n4)), dim3(256), 0, s, dY, X, dX, n4, HW, C, (float)(1.0 / HW));
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// softmax + Keras-3 sparse_categorical_crossentropy(from_logits=False):
//   p = softmax(z); pc = clip(p, 1e-7, 1-1e-7); loss = -(log pc_y - log sum_j pc_j)
// (nsga_penalty.py:377-379 via the TF backend).  One block; rows strided over
// lanes; wavefront (shuffle) reductions for the loss / correct counters.
//
// ONE body for the three training losses (kernels.h: semantics), so that the loops they share -- the maximum, the sum, p,
// pc and S, the gradient's dot product, the fixed-order reduction -- are the same text and the promise that one-hot
// targets give the sparse loss's bits (kernels.h) cannot be broken by an edit to one of them:
//   CE_SPARSE   the label y = labels[row(r)] read through the batch-row source
//   CE_SOFT     a dense target row tg with weight w.  On a one-hot row with unit weight the only extra operations are
//               1.0f * x and x + 0.0f, so the loss, dz, the predictions and the correct count carry CE_SPARSE's bits
//   CE_DISTILL  CE_SOFT plus the tempered term: s = softmax(z / T) held as an un-clipped log-softmax against the teacher row qt
// p and pc are recomputed in every loop that needs them, never carried from one to the next.
// ===========================================================================
enum CeMode { CE_SPARSE, CE_SOFT, CE_DISTILL };

template <CeMode MODE>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ Z, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ idx, int64_t row0,
                                                         const StepState* __restrict__ st, int64_t n_rows,
                                                         const float* __restrict__ Tg, const float* __restrict__ Wr,
                                                         const int32_t* __restrict__ primary, const float* __restrict__ Qt,
                                                         DistillParams d, int B, int C, float* __restrict__ dZ,
                                                         double* __restrict__ acc, int32_t* __restrict__ preds) {
    constexpr bool SPARSE = MODE == CE_SPARSE, DISTILL = MODE == CE_DISTILL;
    __shared__ double lsum[4];
    if constexpr (SPARSE) { if (st) row0 = st->row0; }
    __shared__ int csum[4];
    const int t = threadIdx.x;
    const float lo = 1e-7f, hi = 1.0f - 1e-7f;
    double myloss = 0.0;
    int mycorrect = 0;
    for (int r = t; r < B; r += 256) {
        const float* z = Z + (size_t)r * C;
        const float* tg = SPARSE ? nullptr : Tg + (size_t)r * C;
        const float* qt = DISTILL ? Qt + (size_t)r * C : nullptr;
        float w = 1.0f;
        int y;
        if constexpr (SPARSE) {
            y = labels[gather_row(idx, row0 + r, n_rows)];
        } else {
            if (Wr) w = Wr[r];
            if (primary) {
                y = primary[r];
            } else {                           // the first maximum of the target row
                y = 0;
                float tm = tg[0];
                for (int j = 1; j < C; ++j)
                    if (tg[j] > tm) { tm = tg[j]; y = j; }
            }
        }
        float mx = z[0];
        int am = 0;
        for (int j = 1; j < C; ++j)
            if (z[j] > mx) { mx = z[j]; am = j; }
        float se = 0.f;
        for (int j = 0; j < C; ++j) se += expf(z[j] - mx);
        float S = 0.f, Tsum = 0.f, pyc = 1.f;
        for (int j = 0; j < C; ++j) {
            const float p = expf(z[j] - mx) / se;
            const float pc = fminf(fmaxf(p, lo), hi);
            S += pc;
            if constexpr (SPARSE) { if (j == y) pyc = pc; }
            else Tsum += tg[j];
        }
        [[maybe_unused]] double seT = 0.0, Qs = 0.0;
        if constexpr (SPARSE) {
            myloss += (double)(-(logf(pyc) - logf(S)));
        } else {
            const float logS = logf(S);
            float l = 0.f;
            for (int j = 0; j < C; ++j) {
                const float tj = tg[j];
                if (tj > 0.f) {
                    const float p = expf(z[j] - mx) / se;
                    const float pc = fminf(fmaxf(p, lo), hi);
                    l += tj * (logf(pc) - logS);
                }
            }
            if constexpr (!DISTILL) {
                myloss += (double)(w * -l);
            } else {
                // the tempered student: e_j = expf((z_j - mx) / T), seT = sum_j e_j, ls_j = (z_j - mx) / T - log seT;
                // KD = sum q_j (log q_j - ls_j).  Both KD and the gradient term Qs s_i - q_i are small differences of large
                // terms -- where distillation converges to, s = q, they vanish -- and T^2 / T scale them: the sums seT and
                // Qs, the two logarithms of KD, its sum and the difference Qs s_i - q_i are formed in double from the fp32
                // e_j and q_j.  (The device's float32 log is low on average -- tools/device_log_bias.py,
                // profiles/distill_logf_bias.txt -- and both logarithms enter KD with the same sign;
                // tests/test_gpu_distill.py holds loss sum and dZ to 8 x the error of a float32 autograd restatement.)
                for (int j = 0; j < C; ++j) {
                    seT += (double)expf((z[j] - mx) / d.T);
                    Qs += (double)qt[j];
                }
                const double logseT = log(seT);
                double kd = 0.0;
                for (int j = 0; j < C; ++j) {
                    const float qj = qt[j];
                    if (qj > 0.f) kd += (double)qj * (log((double)qj) - ((double)((z[j] - mx) / d.T) - logseT));
                }
                myloss += (double)w * ((double)(d.one_minus_alpha * -l) + (double)d.alpha_t2 * kd);
            }
        }
        mycorrect += (am == y);
        if (preds) preds[r] = am;
        if (dZ) {
            // q_j = gate_j * (1/S - [j==y]/pc_y), dense targets: gate_j * (Tsum/S - t_j/pc_j);
            // g_i = p_i * (q_i - sum_j p_j q_j); dz_i = g_i / B, times w, distill: w ((1 - alpha) g_i + alpha T (Qs s_i - q_i)) / B
            auto q_of = [&](int j, float p) -> float {
                [[maybe_unused]] const float pc = fminf(fmaxf(p, lo), hi);
                const float gate = (p >= lo && p <= hi) ? 1.f : 0.f;
                if constexpr (SPARSE) return gate * (1.f / S - (j == y ? 1.f / pyc : 0.f));
                else return gate * (Tsum / S - tg[j] / pc);
            };
            float dot = 0.f;
            for (int j = 0; j < C; ++j) {
                const float p = expf(z[j] - mx) / se;
                dot += p * q_of(j, p);
            }
            const float invB = 1.f / (float)B;
            [[maybe_unused]] const double rseT = DISTILL ? 1.0 / seT : 0.0;
            for (int j = 0; j < C; ++j) {
                const float p = expf(z[j] - mx) / se;
                const float qj = q_of(j, p);
                if constexpr (SPARSE) {
                    dZ[(size_t)r * C + j] = p * (qj - dot) * invB;
                } else if constexpr (!DISTILL) {
                    dZ[(size_t)r * C + j] = w * (p * (qj - dot) * invB);
                } else {
                    const float g = p * (qj - dot);
                    const float kg = (float)(Qs * ((double)expf((z[j] - mx) / d.T) * rseT) - (double)qt[j]);   // Qs s_j - q_j
                    dZ[(size_t)r * C + j] = w * ((d.one_minus_alpha * g + d.alpha_t * kg) * invB);
                }
            }
        }
    }
    // wavefront reduction (fixed butterfly order: deterministic), then the four wave sums in wave order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        myloss += __shfl_xor(myloss, off, 64);
        mycorrect += __shfl_xor(mycorrect, off, 64);
    }
    if ((t & 63) == 0) { lsum[t >> 6] = myloss; csum[t >> 6] = mycorrect; }
    __syncthreads();
    if (t == 0 && acc) {
        acc[0] += ((lsum[0] + lsum[1]) + lsum[2]) + lsum[3];
        reinterpret_cast<long long*>(acc)[1] += (csum[0] + csum[1]) + (csum[2] + csum[3]);
    }
}

void launch_softmax_ce(const float* Z, const int32_t* labels, const BatchRows& rows, int B, int C, float* dZ, double* acc,
                       int32_t* preds, hipStream_t s) {
    if (B == 0) return;
    hipLaunchKernelGGL(softmax_ce_kernel<CE_SPARSE>, dim3(1), dim3(256), 0, s, Z, labels, rows.idx, rows.row0, rows.st, rows.n_rows,
                       nullptr, nullptr, nullptr, nullptr, DistillParams(), B, C, dZ, acc, preds);
    CMOOP_HIP(hipGetLastError());
}

// Model.predict: the probabilities softmax_ce_kernel forms and discards.  One thread per row; the same serial loops in
// the same order (maximum, sum over ascending j, expf(z_j - max) / sum), so p is bit-equal to the p behind the loss and
// the row's arg max is the prediction evaluate returns.  C <= a few dozen floats per row: the pass is launch-bound.
__global__ __launch_bounds__(256) void softmax_probs_kernel(const float* __restrict__ Z, float* __restrict__ P, int B, int C) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    const float* z = Z + (size_t)r * C;
    float* p = P + (size_t)r * C;
    float mx = z[0];
    for (int j = 1; j < C; ++j)
        if (z[j] > mx) mx = z[j];
    float se = 0.f;
    for (int j = 0; j < C; ++j) se += expf(z[j] - mx);
    for (int j = 0; j < C; ++j) p[j] = expf(z[j] - mx) / se;
}

void launch_softmax_probs(const float* Z, float* P, int B, int C, hipStream_t s) {
    if (B == 0) return;
    hipLaunchKernelGGL(softmax_probs_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, Z, P, B, C);
    CMOOP_HIP(hipGetLastError());
}

// Sliding-window scoring: window w = rows [w hop, w hop + T) of a feature stream [n_frames][F] -- T F CONTIGUOUS floats
// at element offset w hop F.  One workgroup copies one window into the [B][T][F] chunk the forward pass reads, applying
// on the way (a) the dB reference / top_db floor of THIS window (the tail of logmel_ex_kernel with "window" for "clip":
// workgroup maximum, then max(v - ref, floor)) and (b) the StandardScaler, (float)(((double)v - mean[c]) / scale[c]) as
// standardize_kernel.  64-bit base per window, 32-bit index inside it; the column of element i = t + 256 k is carried
// along (c += 256 mod F) instead of a modulo per element.  The stream itself is only read.
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ feat, float* __restrict__ chunk, int64_t w0,
                                                            int hop, int TF, int F, int db, int db_ref_max, float amin,
                                                            float top_db, const double* __restrict__ mean,
                                                            const double* __restrict__ scale) {
    __shared__ float s_red[4];
    const int t = threadIdx.x;
    const float* src = feat + (w0 + blockIdx.x) * (int64_t)hop * F;
    float* dst = chunk + (size_t)blockIdx.x * TF;
    float ref = 0.f, floor_db = -INFINITY;
    if (db) {                                                     // kernel argument: uniform over the grid
        float vmax = -INFINITY;
        for (int i = t; i < TF; i += 256) vmax = fmaxf(vmax, src[i]);
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) vmax = fmaxf(vmax, __shfl_xor(vmax, off, 64));
        if ((t & 63) == 0) s_red[t >> 6] = vmax;
        __syncthreads();
        const float cmax = fmaxf(fmaxf(s_red[0], s_red[1]), fmaxf(s_red[2], s_red[3]));
        ref = db_ref_max ? cmax : 10.f * log10f(fmaxf(amin, 1.f));
        floor_db = top_db >= 0.f ? (cmax - ref) - top_db : -INFINITY;
    }
    const int step = 256 % F;
    int c = t % F;
    for (int i = t; i < TF; i += 256) {
        float v = src[i];
        if (db) v = fmaxf(v - ref, floor_db);
        if (mean) v = (float)(((double)v - mean[c]) / scale[c]);
        dst[i] = v;
        c += step;
        if (c >= F) c -= F;
    }
}

void launch_window_gather(const float* feat, float* chunk, int64_t w0, int B, int hop, int T, int F, int db, int db_ref_max,
                          float amin, float top_db, const double* mean, const double* scale, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE((int64_t)T * F <= 0x7fffffff - 256, "window gather: T * F out of range");
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)B), dim3(256), 0, s, feat, chunk, w0, hop, T * F, F, db, db_ref_max, amin,
                       top_db, mean, scale);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// Train-time augmentation (kernels.h: semantics).  One work item = 256-thread slice `chunk` of `cpr` of batch row b; the
// grid strides over the B cpr items.  Thread 0 makes the row's draws once per item into LDS; every thread then moves VEC
// floats per trip: the frame test (shift range, time masks) once per vector, the band test per float.
// ===========================================================================
// x + (float)n * k as two separately rounded operations (the numpy twin multiplies, then adds): no fused multiply-add,
// for adam_update's reason
__device__ __forceinline__ float augment_add_noise(float x, uint32_t ua, uint32_t uc, float k) {
#pragma clang fp contract(off)
    const int n = (int)((ua & 0xFFFFu) + (ua >> 16) + (uc & 0xFFFFu) + (uc >> 16)) - 131070;
    const float nk = (float)n * k;
    return x + nk;
}

template <int VEC>
__global__ __launch_bounds__(256) void augment_gather_kernel(const float* __restrict__ X, const int32_t* __restrict__ idx,
                                                             int64_t row0, float* __restrict__ out, int B, int T, int F,
                                                             AugmentParams a, uint32_t seed, uint32_t step, int cpr,
                                                             const StepState* __restrict__ st, int64_t n_rows) {
    __shared__ int32_t d[AUGMENT_DRAWS];
    if (st) { row0 = st->row0; step = st->step; }
    const int FV = F / VEC, TFV = T * FV;
    const uint32_t pa = rng_prefix(seed, STREAM_AUGMENT + 1u, step), pc = rng_prefix(seed, STREAM_AUGMENT + 2u, step);
    const int items = B * cpr;
    for (int w = blockIdx.x; w < items; w += gridDim.x) {
        const int b = w / cpr, chunk = w - b * cpr;
        __syncthreads();                       // the previous item's readers are done with d
        if (threadIdx.x == 0) augment_row_draws(a, seed, step, (uint32_t)b, T, F, d);
        __syncthreads();
        const int s = d[1];
        const bool noisy = a.noise && d[0];
        const float* src = X + gather_row(idx, row0 + b, n_rows) * (int64_t)T * F;
        float* dst = out + (int64_t)b * T * F;
        for (int i = chunk * 256 + threadIdx.x; i < TFV; i += cpr * 256) {
            const int t = i / FV, f = (i - t * FV) * VEC, ts = t - s;
            bool drop = (unsigned)ts >= (unsigned)T;
#pragma unroll
            for (int j = 0; j < AUGMENT_MAX_MASKS; ++j) drop |= (unsigned)(t - d[3 + 2 * j]) < (unsigned)d[2 + 2 * j];
            float v[VEC];
            if (drop) {
#pragma unroll
                for (int q = 0; q < VEC; ++q) v[q] = a.fill;
            } else {
                if constexpr (VEC == 4) {
                    const f32x4 x4 = *reinterpret_cast<const f32x4*>(src + (int64_t)ts * F + f);
                    v[0] = x4.x; v[1] = x4.y; v[2] = x4.z; v[3] = x4.w;
                } else {
                    v[0] = src[(int64_t)ts * F + f];
                }
#pragma unroll
                for (int q = 0; q < VEC; ++q) {
                    const int ff = f + q;
                    bool fm = false;
#pragma unroll
                    for (int j = 0; j < AUGMENT_MAX_MASKS; ++j) fm |= (unsigned)(ff - d[11 + 2 * j]) < (unsigned)d[10 + 2 * j];
                    if (fm) {
                        v[q] = a.fill;
                    } else if (noisy) {
                        const uint32_t e = ((uint32_t)b * (uint32_t)T + (uint32_t)t) * (uint32_t)F + (uint32_t)ff;
                        v[q] = augment_add_noise(v[q], fmix32(pa ^ e), fmix32(pc ^ e), a.noise_k);
                    }
                }
            }
            if constexpr (VEC == 4) {
                f32x4 o; o.x = v[0]; o.y = v[1]; o.z = v[2]; o.w = v[3];
                *reinterpret_cast<f32x4*>(dst + (int64_t)t * F + f) = o;
            } else {
                dst[(int64_t)t * F + f] = v[0];
            }
        }
    }
}

void augment_check(const AugmentCfg& c, int T, int F) {
    CMOOP_REQUIRE(T >= 1 && F >= 1, "augment: bad feature shape");
    CMOOP_REQUIRE(c.p >= 0.0 && c.p <= 1.0, "augment: p must be in [0, 1]");   // (a NaN fails both comparisons)
    CMOOP_REQUIRE(c.time_shift >= 0 && c.time_shift < T, "augment: time_shift must be in [0, T = " + std::to_string(T) + ")");
    CMOOP_REQUIRE(c.time_masks >= 0 && c.time_masks <= AUGMENT_MAX_MASKS, "augment: time_masks must be in [0, 4]");
    CMOOP_REQUIRE(c.time_mask_max >= 0 && c.time_mask_max <= T, "augment: time_mask_max must be in [0, T = " + std::to_string(T) + "]");
    CMOOP_REQUIRE(c.freq_masks >= 0 && c.freq_masks <= AUGMENT_MAX_MASKS, "augment: freq_masks must be in [0, 4]");
    CMOOP_REQUIRE(c.freq_mask_max >= 0 && c.freq_mask_max <= F, "augment: freq_mask_max must be in [0, F = " + std::to_string(F) + "]");
    CMOOP_REQUIRE(std::isfinite(c.noise_std) && c.noise_std >= 0.0, "augment: noise_std must be finite and >= 0");
    CMOOP_REQUIRE(std::isfinite(c.fill), "augment: fill must be finite");
}

bool augment_enabled(const AugmentCfg& c) {
    return c.p > 0.0 && (c.time_shift > 0 || (c.time_masks > 0 && c.time_mask_max > 0) || (c.freq_masks > 0 && c.freq_mask_max > 0) ||
                         c.noise_std > 0.0);
}

AugmentParams augment_params(const AugmentCfg& c) {
    AugmentParams a;
    a.S = c.time_shift; a.time_masks = c.time_masks; a.time_mask_max = c.time_mask_max;
    a.freq_masks = c.freq_masks; a.freq_mask_max = c.freq_mask_max;
    a.gate_thr = (uint32_t)std::floor(c.p * 16777216.0);
    a.noise = c.noise_std > 0.0 ? 1 : 0;
    a.noise_k = (float)(c.noise_std * std::sqrt(3.0) / 65536.0);   // evaluated in double, rounded once
    a.fill = (float)c.fill;
    return a;
}

void launch_augment_gather(const float* X, const BatchRows& rows, float* out, int B, int T, int F, const AugmentParams& a,
                           uint32_t seed, uint32_t step, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && T >= 1 && F >= 1 && X && out, "augment gather: bad arguments");
    CMOOP_REQUIRE((int64_t)T * F < (1ll << 30) && (int64_t)B * T * F < (1ll << 32), "augment gather: B * T * F must stay below 2^32");
    CMOOP_REQUIRE(a.S >= 0 && a.S < T && a.time_masks >= 0 && a.time_masks <= AUGMENT_MAX_MASKS && a.time_mask_max >= 0 &&
                      a.time_mask_max <= T && a.freq_masks >= 0 && a.freq_masks <= AUGMENT_MAX_MASKS && a.freq_mask_max >= 0 &&
                      a.freq_mask_max <= F, "augment gather: config outside the domain (augment_check)");
    const bool vec = F % 4 == 0 && ((reinterpret_cast<uintptr_t>(X) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int TFV = vec ? T * (F / 4) : T * F;
    // slices per row: enough for one trip per thread, while the grid stays within ~2048 workgroups
    const int cpr = std::max(1, std::min(cdiv(TFV, 256), 2048 / B));
    const unsigned grid = (unsigned)std::min<int64_t>((int64_t)B * cpr, 2048);
    if (vec)
        hipLaunchKernelGGL(augment_gather_kernel<4>, dim3(grid), dim3(256), 0, s, X, rows.idx, rows.row0, out, B, T, F, a, seed, step, cpr, rows.st,
                           rows.n_rows);
    else
        hipLaunchKernelGGL(augment_gather_kernel<1>, dim3(grid), dim3(256), 0, s, X, rows.idx, rows.row0, out, B, T, F, a, seed, step, cpr, rows.st,
                           rows.n_rows);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// Soft-target training loss (kernels.h: semantics): the mixup blend of two batch rows, the dense targets / row weights,
// and cross-entropy against them.
// ===========================================================================
// lam x + mu xq as two products and one add, each rounded separately (the numpy twin multiplies, multiplies, adds): no
// fused multiply-add, for augment_add_noise's reason
__device__ __forceinline__ float mixup_blend(float x, float xq, float lam, float mu) {
#pragma clang fp contract(off)
    const float a = lam * x;
    const float c = mu * xq;
    return a + c;
}

// Work items as augment_gather_kernel: 256-thread slice `chunk` of `cpr` of batch row b; thread 0 makes the row's draw
// once per item into LDS.  An un-mixed row is a plain copy
template <int VEC>
__global__ __launch_bounds__(256) void mixup_gather_kernel(const float* __restrict__ src, const int32_t* __restrict__ idx,
                                                           int64_t row0, int from_batch, float* __restrict__ out, int B, int TF,
                                                           MixupParams m, uint32_t seed, uint32_t step, int cpr,
                                                           const StepState* __restrict__ st, int64_t n_rows) {
    __shared__ int32_t dq[2];
    __shared__ float dlam;
    if (st) {
        step = st->step;
        if (!from_batch) row0 = st->row0;      // the batch buffer always starts at its row 0
    }
    const int TFV = TF / VEC;
    const int items = B * cpr;
    for (int w = blockIdx.x; w < items; w += gridDim.x) {
        const int b = w / cpr, chunk = w - b * cpr;
        __syncthreads();                       // the previous item's readers are done with the draw
        if (threadIdx.x == 0) mixup_row_draws(m, seed, step, (uint32_t)b, (uint32_t)B, &dq[0], &dq[1], &dlam);
        __syncthreads();
        const int q = dq[1];
        const float lam = dlam, mu = 1.0f - lam;
        const float* xb = src + (from_batch ? (int64_t)b : gather_row(idx, row0 + b, n_rows)) * (int64_t)TF;
        const float* xq = src + (from_batch ? (int64_t)q : gather_row(idx, row0 + q, n_rows)) * (int64_t)TF;
        float* dst = out + (int64_t)b * TF;
        const bool mixed = q != b;
        for (int i = chunk * 256 + threadIdx.x; i < TFV; i += cpr * 256) {
            if constexpr (VEC == 4) {
                f32x4 v = *reinterpret_cast<const f32x4*>(xb + 4 * i);
                if (mixed) {
                    const f32x4 u = *reinterpret_cast<const f32x4*>(xq + 4 * i);
                    v.x = mixup_blend(v.x, u.x, lam, mu); v.y = mixup_blend(v.y, u.y, lam, mu);
                    v.z = mixup_blend(v.z, u.z, lam, mu); v.w = mixup_blend(v.w, u.w, lam, mu);
                }
                *reinterpret_cast<f32x4*>(dst + 4 * i) = v;
            } else {
                float v = xb[i];
                if (mixed) v = mixup_blend(v, xq[i], lam, mu);
                dst[i] = v;
            }
        }
    }
}

void launch_mixup_gather(const float* src, const BatchRows& rows, int from_batch, float* out, int B, int T, int F,
                         const MixupParams& m, uint32_t seed, uint32_t step, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && T >= 1 && F >= 1 && src && out && src != out, "mixup gather: bad arguments");
    CMOOP_REQUIRE((int64_t)T * F < (1ll << 30), "mixup gather: T * F must stay below 2^30");
    CMOOP_REQUIRE(!m.on || m.tab != nullptr, "mixup gather: the lam table is missing");
    const bool vec = F % 4 == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int TF = T * F, TFV = vec ? TF / 4 : TF;
    const int cpr = std::max(1, std::min(cdiv(TFV, 256), std::max(1, 2048 / B)));
    const unsigned grid = (unsigned)std::min<int64_t>((int64_t)B * cpr, 2048);
    if (vec)
        hipLaunchKernelGGL(mixup_gather_kernel<4>, dim3(grid), dim3(256), 0, s, src, rows.idx, rows.row0, from_batch, out, B, TF, m,
                           seed, step, cpr, rows.st, rows.n_rows);
    else
        hipLaunchKernelGGL(mixup_gather_kernel<1>, dim3(grid), dim3(256), 0, s, src, rows.idx, rows.row0, from_batch, out, B, TF, m,
                           seed, step, cpr, rows.st, rows.n_rows);
    CMOOP_HIP(hipGetLastError());
}

// One thread per batch row: the row's draw, its two labels, then C targets.  A label outside [0, C) matches no class (its
// share of the target is dropped, as the sparse kernel's comparison drops it) and reads the weight of the nearest class
__global__ __launch_bounds__(256) void soft_targets_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ idx,
                                                           int64_t row0, int B, int C, MixupParams m, TargetParams tp, uint32_t seed,
                                                           uint32_t step, float* __restrict__ T, float* __restrict__ W,
                                                           int32_t* __restrict__ primary, const StepState* __restrict__ st,
                                                           int64_t n_rows) {
#pragma clang fp contract(off)
    if (st) { row0 = st->row0; step = st->step; }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int32_t gate, q;
    float lam;
    mixup_row_draws(m, seed, step, (uint32_t)b, (uint32_t)B, &gate, &q, &lam);
    const float mu = 1.0f - lam;
    const int a = labels[gather_row(idx, row0 + b, n_rows)];
    const int c = q == b ? a : labels[gather_row(idx, row0 + q, n_rows)];
    float* t = T + (size_t)b * C;
    for (int j = 0; j < C; ++j) {
        const float mj = (j == a ? lam : 0.f) + (j == c ? mu : 0.f);
        const float sc = mj * tp.one_minus_eps;
        t[j] = sc + tp.eps_over_c;
    }
    float w = 1.0f;
    if (tp.cw) {
        const float wa = lam * tp.cw[min(max(a, 0), C - 1)];
        const float wc = mu * tp.cw[min(max(c, 0), C - 1)];
        w = wa + wc;
    }
    W[b] = w;
    primary[b] = a;
}

void launch_soft_targets(const int32_t* labels, const BatchRows& rows, int B, int C, const MixupParams& m, const TargetParams& tp,
                         uint32_t seed, uint32_t step, float* t, float* w, int32_t* primary, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && labels && t && w && primary, "soft targets: bad arguments");
    CMOOP_REQUIRE(!m.on || m.tab != nullptr, "soft targets: the lam table is missing");
    hipLaunchKernelGGL(soft_targets_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, labels, rows.idx, rows.row0, B, C, m, tp, seed, step,
                       t, w, primary, rows.st, rows.n_rows);
    CMOOP_HIP(hipGetLastError());
}

void launch_softmax_ce_soft(const float* Z, const float* t, const float* w, const int32_t* primary, int B, int C, float* dZ,
                            double* acc, int32_t* preds, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && Z && t, "softmax_ce_soft: bad arguments");
    hipLaunchKernelGGL(softmax_ce_kernel<CE_SOFT>, dim3(1), dim3(256), 0, s, Z, nullptr, nullptr, 0, nullptr, 0, t, w, primary, nullptr,
                       DistillParams(), B, C, dZ, acc, preds);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// Knowledge distillation (kernels.h: semantics): the tempered teacher rows of a batch, and the loss against them.
// ===========================================================================
// One thread per batch row, as soft_targets_kernel: the row's draw, then max-subtracted softmax(zt[row] / T) with serial
// loops in class order -- a row's result depends on its own logits (and its partner's) only, never on the batch or its
// position in it.  An un-mixed row stores u's bits; a MIXED one lam u_j + mu v_j, two products and one add, no contraction
__global__ __launch_bounds__(256) void teacher_targets_kernel(const float* __restrict__ Zt, const int32_t* __restrict__ idx,
                                                              int64_t row0, int64_t n_rows, int B, int C, float T, MixupParams m,
                                                              uint32_t seed, uint32_t step, float* __restrict__ Q,
                                                              const StepState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st) { row0 = st->row0; step = st->step; }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int32_t gate, p;
    float lam;
    mixup_row_draws(m, seed, step, (uint32_t)b, (uint32_t)B, &gate, &p, &lam);
    const float mu = 1.0f - lam;
    const float* zu = Zt + gather_row(idx, row0 + b, n_rows) * (int64_t)C;
    float* q = Q + (size_t)b * C;
    float mxu = zu[0];
    for (int j = 1; j < C; ++j)
        if (zu[j] > mxu) mxu = zu[j];
    float seu = 0.f;
    for (int j = 0; j < C; ++j) seu += expf((zu[j] - mxu) / T);
    if (p == b) {
        for (int j = 0; j < C; ++j) q[j] = expf((zu[j] - mxu) / T) / seu;
        return;
    }
    const float* zv = Zt + gather_row(idx, row0 + p, n_rows) * (int64_t)C;
    float mxv = zv[0];
    for (int j = 1; j < C; ++j)
        if (zv[j] > mxv) mxv = zv[j];
    float sev = 0.f;
    for (int j = 0; j < C; ++j) sev += expf((zv[j] - mxv) / T);
    for (int j = 0; j < C; ++j) {
        const float u = expf((zu[j] - mxu) / T) / seu;
        const float v = expf((zv[j] - mxv) / T) / sev;
        const float a = lam * u;
        const float c = mu * v;
        q[j] = a + c;
    }
}

void launch_teacher_targets(const float* zt, const BatchRows& rows, int B, int C, float T, const MixupParams& m, uint32_t seed,
                            uint32_t step, float* q, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && rows.n_rows >= 1 && zt && q, "teacher targets: bad arguments");
    CMOOP_REQUIRE(T >= 1.0f && T <= 64.0f, "teacher targets: temperature must be in [1, 64]");
    CMOOP_REQUIRE(!m.on || m.tab != nullptr, "teacher targets: the lam table is missing");
    hipLaunchKernelGGL(teacher_targets_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, zt, rows.idx, rows.row0, rows.n_rows, B, C, T, m, seed,
                       step, q, rows.st);
    CMOOP_HIP(hipGetLastError());
}

void launch_softmax_ce_distill(const float* Z, const float* t, const float* w, const int32_t* primary, const float* q,
                               const DistillParams& d, int B, int C, float* dZ, double* acc, int32_t* preds, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && Z && t && q, "softmax_ce_distill: bad arguments");
    CMOOP_REQUIRE(d.T >= 1.0f && d.T <= 64.0f, "softmax_ce_distill: temperature must be in [1, 64]");
    hipLaunchKernelGGL(softmax_ce_kernel<CE_DISTILL>, dim3(1), dim3(256), 0, s, Z, nullptr, nullptr, 0, nullptr, 0, t, w, primary, q, d, B, C,
                       dZ, acc, preds);
    CMOOP_HIP(hipGetLastError());
}

void distill_check(const DistillCfg& c, int classes, int64_t n_train) {
    CMOOP_REQUIRE(classes >= 1, "distill: classes must be >= 1");
    CMOOP_REQUIRE(c.alpha >= 0.0 && c.alpha <= 1.0, "distill: alpha must be in [0, 1]");   // (a NaN fails)
    CMOOP_REQUIRE(std::isfinite(c.temperature) && c.temperature >= 1.0 && c.temperature <= 64.0,
                  "distill: temperature must be finite and in [1, 64]");
    if (c.teacher_logits)
        CMOOP_REQUIRE(c.n_rows >= 1 && c.n_rows == n_train, "distill: n_rows must equal the training rows = " + std::to_string(n_train) +
                                                                " (got " + std::to_string(c.n_rows) + ")");
}

DistillParams distill_params(const DistillCfg& c) {
    DistillParams d;
    d.one_minus_alpha = (float)(1.0 - c.alpha);
    d.alpha_t = (float)(c.alpha * c.temperature);
    d.alpha_t2 = (float)(c.alpha * c.temperature * c.temperature);
    d.T = (float)c.temperature;
    return d;
}

void loss_check(const LossCfg& c, int classes) {
    CMOOP_REQUIRE(classes >= 1, "loss: classes must be >= 1");
    CMOOP_REQUIRE(c.label_smoothing >= 0.0 && c.label_smoothing < 1.0, "loss: label_smoothing must be in [0, 1)");   // (a NaN fails)
    CMOOP_REQUIRE(std::isfinite(c.mixup_alpha) && c.mixup_alpha >= 0.0 && c.mixup_alpha <= 64.0,
                  "loss: mixup_alpha must be finite and in [0, 64]");
    CMOOP_REQUIRE(c.mixup_p >= 0.0 && c.mixup_p <= 1.0, "loss: mixup_p must be in [0, 1]");
    if (c.class_weight) {
        CMOOP_REQUIRE(c.n_class_weight == classes, "loss: n_class_weight must equal classes = " + std::to_string(classes) + " (got " +
                                                       std::to_string(c.n_class_weight) + ")");
        for (int j = 0; j < classes; ++j)
            CMOOP_REQUIRE(std::isfinite(c.class_weight[j]) && c.class_weight[j] > 0.0,
                          "loss: class_weight[" + std::to_string(j) + "] must be finite and > 0");
    }
}

bool loss_enabled(const LossCfg& c) { return c.label_smoothing > 0.0 || loss_mixup_on(c) || c.class_weight != nullptr; }

TargetParams target_params(const LossCfg& c, int classes, const float* cw_dev) {
    TargetParams tp;
    tp.one_minus_eps = (float)(1.0 - c.label_smoothing);
    tp.eps_over_c = (float)(c.label_smoothing / (double)classes);
    tp.cw = c.class_weight ? cw_dev : nullptr;
    return tp;
}

// I_y(a, a) for 0 < y <= 1/2 (where the continued fraction of the incomplete beta converges fastest): modified Lentz
static double inc_beta_sym(double a, double y, double ln_beta) {
    if (y <= 0.0) return 0.0;
    const double tiny = 1e-300, b = a, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * y / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 1000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * y / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * y / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 3e-16) break;
    }
    return std::exp(a * std::log(y) + b * std::log1p(-y) - ln_beta) * h / a;
}

void mixup_table(double alpha, float out[MIXUP_TABLE]) {
    CMOOP_REQUIRE(std::isfinite(alpha) && alpha > 0.0 && alpha <= 64.0, "mixup table: alpha must be finite and in (0, 64]");
    // every candidate of a population asks for the same table: keep the last one
    static std::mutex mu;
    static double last_alpha = 0.0;
    static float last_tab[MIXUP_TABLE];
    std::lock_guard<std::mutex> lock(mu);
    if (alpha == last_alpha) { std::copy(last_tab, last_tab + MIXUP_TABLE, out); return; }
    const double ln_beta = 2.0 * std::lgamma(alpha) - std::lgamma(2.0 * alpha);
    for (int k = 0; k < MIXUP_TABLE; ++k) {
        // Q(0.5 + (k + 0.5) / 2048) = 1 - y with I_y(alpha, alpha) = 0.5 - (k + 0.5) / 2048 (symmetry), y in (0, 1/2):
        // solved on the lower tail, where the small quantiles of a small alpha keep their relative precision
        const double target = 0.5 - ((double)k + 0.5) / 2048.0;
        double ylo = 0.0, yhi = 0.5;
        for (int it = 0; it < 1200; ++it) {
            const double mid = 0.5 * (ylo + yhi);
            if (!(mid > ylo && mid < yhi)) break;
            if (inc_beta_sym(alpha, mid, ln_beta) < target) ylo = mid; else yhi = mid;
        }
        out[k] = (float)(1.0 - 0.5 * (ylo + yhi));
    }
    std::copy(out, out + MIXUP_TABLE, last_tab);
    last_alpha = alpha;
}

// Every operation of the update is a separately rounded IEEE single operation, in the order the reference's CPU path and
// the oracle apply them (oracle/net.py train_step): no fused multiply-add.  Left to the compiler, the contraction of
// m + (g - m) * c1 differed BETWEEN TWO KERNELS of this file (fused in one, mul + add in the other), an ulp apart --
// enough to change the predictions of a BatchNorm + dropout candidate 100 steps later.
__device__ __forceinline__ void adam_update(float* __restrict__ w, float* __restrict__ m, float* __restrict__ v, int64_t i,
                                            float gi, float alpha, float c1, float c2, float eps) {
#pragma clang fp contract(off)
    float mi = m[i], vi = v[i];
    const float dm = (gi - mi) * c1;
    mi = mi + dm;
    const float gg = gi * gi;
    const float dv = (gg - vi) * c2;
    vi = vi + dv;
    m[i] = mi;
    v[i] = vi;
    const float num = mi * alpha;
    const float den = sqrtf(vi) + eps;
    w[i] = w[i] - num / den;
}

// adam_update on values, for adamw_kernel (which decays w first and moves four elements per 16-byte access): the same
// operations in the same order.  A twin, not a shared body: adam_update rewritten over these two compiles adam_segments_kernel
// to another instruction schedule, and the default path is to stay the kernel it was
__device__ __forceinline__ void adam_moments(float& mi, float& vi, float gi, float c1, float c2) {
#pragma clang fp contract(off)
    const float dm = (gi - mi) * c1;
    mi = mi + dm;
    const float gg = gi * gi;
    const float dv = (gg - vi) * c2;
    vi = vi + dv;
}
__device__ __forceinline__ float adam_delta(float mi, float vi, float alpha, float eps) {
#pragma clang fp contract(off)
    const float num = mi * alpha;
    const float den = sqrtf(vi) + eps;
    return num / den;
}

// Keras-form Adam: m += (g-m)(1-b1); v += (g^2-v)(1-b2); w -= m*alpha/(sqrt(v)+eps)
__global__ __launch_bounds__(256) void adam_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                   float* __restrict__ v, int64_t n, float alpha, float c1, float c2,
                                                   float eps, const StepState* __restrict__ st,
                                                   const float* __restrict__ alpha_table) {
    if (st) alpha = alpha_table[st->iter];
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256)
        adam_update(w, m, v, i, g[i], alpha, c1, c2, eps);
}

void launch_adam(float* w, const float* g, float* m, float* v, int64_t n, float alpha, float c1, float c2, float eps,
                 hipStream_t s, const StepState* st, const float* alpha_table) {
    if (n == 0) return;
    hipLaunchKernelGGL(adam_kernel, dim3(ew_grid(n)), dim3(256), 0, s, w, g, m, v, n, alpha, c1, c2, eps, st, alpha_table);
    CMOOP_HIP(hipGetLastError());
}

// slab segment: 64 column groups of VEC floats x 4 slice lanes per workgroup; lane sl sums slices sl, sl+4, ... with four
// independent accumulators of eight (the order of reduce_slices_kernel, gemm.hip), lane 0 combines, stores g and updates w/m/v
template <int VEC>
__device__ __forceinline__ void adam_slab_block(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                                float* __restrict__ v, const AdamSeg sg, int b, float (*red)[256],
                                                float alpha, float c1, float c2, float eps) {
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int64_t i = ((int64_t)b * 64 + e) * VEC;
    float acc[8][VEC];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[u][j] = 0.f;
    if (i < sg.n) {
        int s = sl;
        for (; s + 28 < sg.S; s += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float* src = sg.slab + (size_t)(s + 4 * u) * sg.stride + i;
                if constexpr (VEC == 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(src);
                    acc[u][0] += q[0]; acc[u][1] += q[1]; acc[u][2] += q[2]; acc[u][3] += q[3];
                } else {
                    acc[u][0] += src[0];
                }
            }
        }
        for (; s < sg.S; s += 4) {
            const float* src = sg.slab + (size_t)s * sg.stride + i;
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[0][j] += src[j];
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        red[sl][e * VEC + j] = ((acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j])) + ((acc[4][j] + acc[5][j]) + (acc[6][j] + acc[7][j]));
    __syncthreads();
    if (sl == 0 && i < sg.n) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float gi = ((red[0][e * VEC + j] + red[1][e * VEC + j]) + red[2][e * VEC + j]) + red[3][e * VEC + j];
            g[sg.off + i + j] = gi;
            adam_update(w, m, v, sg.off + i + j, gi, alpha, c1, c2, eps);
        }
    }
}

constexpr int ADAM_PLAIN_PER_BLOCK = 1024;

__global__ __launch_bounds__(256) void adam_segments_kernel(float* __restrict__ w, float* __restrict__ g, float* __restrict__ m,
                                                            float* __restrict__ v, const AdamSegTable tab, float alpha, float c1,
                                                            float c2, float eps, const StepState* __restrict__ st,
                                                            const float* __restrict__ alpha_table) {
    __shared__ float red[4][256];
    if (st) alpha = alpha_table[st->iter];
    int si = 0;
    while (si + 1 < tab.count && (int)blockIdx.x >= tab.seg[si + 1].block0) ++si;
    const AdamSeg sg = tab.seg[si];
    const int b = (int)blockIdx.x - sg.block0;
    if (sg.slab == nullptr) {
        const int64_t base = (int64_t)b * ADAM_PLAIN_PER_BLOCK;
#pragma unroll
        for (int k = 0; k < ADAM_PLAIN_PER_BLOCK / 256; ++k) {
            const int64_t i = base + k * 256 + threadIdx.x;
            if (i < sg.n) adam_update(w, m, v, sg.off + i, g[sg.off + i], alpha, c1, c2, eps);
        }
        return;
    }
    const bool vec = (sg.n % 4 == 0) && (sg.stride % 4 == 0) && (sg.off % 4 == 0) &&
                     (reinterpret_cast<uintptr_t>(sg.slab) % 16 == 0);
    if (vec) adam_slab_block<4>(w, g, m, v, sg, b, red, alpha, c1, c2, eps);
    else adam_slab_block<1>(w, g, m, v, sg, b, red, alpha, c1, c2, eps);
}

void adam_segments_finalize(AdamSegTable& tab) {
    CMOOP_REQUIRE(tab.count >= 0 && tab.count <= ADAM_MAX_SEGS, "adam segment table overflow");
    int64_t blocks = 0, pos = tab.count ? tab.seg[0].off : 0;
    for (int i = 0; i < tab.count; ++i) {
        AdamSeg& sg = tab.seg[i];
        CMOOP_REQUIRE(sg.off == pos && sg.n > 0, "adam segments must tile the arena in order");
        pos += sg.n;
        sg.block0 = (int32_t)blocks;
        if (sg.slab) {
            const bool vec = (sg.n % 4 == 0) && (sg.stride % 4 == 0) && (sg.off % 4 == 0) &&
                             (reinterpret_cast<uintptr_t>(sg.slab) % 16 == 0);
            blocks += vec ? cdiv64(sg.n / 4, 64) : cdiv64(sg.n, 64);
        } else {
            blocks += cdiv64(sg.n, ADAM_PLAIN_PER_BLOCK);
        }
    }
    CMOOP_REQUIRE(blocks < (int64_t)1 << 30, "adam grid too large");
    tab.blocks = (int32_t)blocks;
}

void launch_adam_segments(float* w, float* g, float* m, float* v, const AdamSegTable& tab, float alpha, float c1, float c2,
                          float eps, hipStream_t s, const StepState* st, const float* alpha_table) {
    if (tab.blocks == 0) return;
    hipLaunchKernelGGL(adam_segments_kernel, dim3((unsigned)tab.blocks), dim3(256), 0, s, w, g, m, v, tab, alpha, c1, c2, eps, st,
                       alpha_table);
    CMOOP_HIP(hipGetLastError());
}

// ---- optimiser options: schedule, decoupled weight decay, clipping (kernels.h) ------------------------------------------------
void optim_check(const OptimCfg& c) {
    auto fin = [](double x) { return std::isfinite(x); };
    CMOOP_REQUIRE(c.schedule >= 0 && c.schedule <= 3, "optim: schedule must be 0 (constant), 1 (cosine), 2 (exponential) or 3 (piecewise)");
    CMOOP_REQUIRE(c.staircase == 0 || c.staircase == 1, "optim: staircase must be 0 or 1");
    CMOOP_REQUIRE(c.decay_mask == 0 || c.decay_mask == 1, "optim: decay_mask must be 0 (kernels) or 1 (every trainable tensor)");
    CMOOP_REQUIRE(fin(c.weight_decay) && c.weight_decay >= 0, "optim: weight_decay must be finite and >= 0");
    CMOOP_REQUIRE(fin(c.global_clipnorm) && c.global_clipnorm >= 0, "optim: global_clipnorm must be finite and >= 0");
    CMOOP_REQUIRE(fin(c.clipvalue) && c.clipvalue >= 0, "optim: clipvalue must be finite and >= 0");
    CMOOP_REQUIRE(!(c.global_clipnorm > 0 && c.clipvalue > 0), "optim: global_clipnorm and clipvalue cannot both be set");
    if (c.schedule == 1) {
        CMOOP_REQUIRE(c.warmup_steps >= 0, "optim: warmup_steps must be >= 0");
        CMOOP_REQUIRE(fin(c.warmup_start) && c.warmup_start >= 0, "optim: warmup_start must be finite and >= 0");
        CMOOP_REQUIRE(c.decay_steps >= 1, "optim: decay_steps must be >= 1 for the cosine schedule");
        CMOOP_REQUIRE(fin(c.alpha) && c.alpha >= 0, "optim: alpha must be finite and >= 0");
    } else if (c.schedule == 2) {
        CMOOP_REQUIRE(c.decay_steps >= 1, "optim: decay_steps must be >= 1 for the exponential schedule");
        CMOOP_REQUIRE(fin(c.decay_rate) && c.decay_rate >= 0, "optim: decay_rate must be finite and >= 0");
    } else if (c.schedule == 3) {
        CMOOP_REQUIRE(c.n_boundaries >= 0 && c.n_boundaries <= OPTIM_MAX_BOUNDARIES, "optim: n_boundaries must be in [0, 8]");
        for (int k = 0; k < c.n_boundaries; ++k)
            CMOOP_REQUIRE(c.boundaries[k] >= 0 && (k == 0 || c.boundaries[k] > c.boundaries[k - 1]),
                          "optim: boundaries must be >= 0 and strictly increasing");
        for (int k = 0; k <= c.n_boundaries; ++k)
            CMOOP_REQUIRE(fin(c.values[k]) && c.values[k] >= 0, "optim: values must be finite and >= 0");
    }
}

OptimRates optim_rates(const OptimCfg& c, double base_lr, double beta1, double beta2, int64_t iteration) {
    CMOOP_REQUIRE(iteration >= 0, "optim rates: iteration must be >= 0");
    const double i = (double)iteration;
    double lr = base_lr;                       // the constant schedule: today's expression, bit for bit
    if (c.schedule == 1) {
        double f;
        if (iteration < c.warmup_steps) {
            f = c.warmup_start + (1.0 - c.warmup_start) * i / (double)c.warmup_steps;
        } else {
            const double s = (double)std::min(iteration - c.warmup_steps, c.decay_steps);
            f = (1.0 - c.alpha) * 0.5 * (1.0 + std::cos(M_PI * s / (double)c.decay_steps)) + c.alpha;
        }
        lr = base_lr * f;
    } else if (c.schedule == 2) {
        double p = i / (double)c.decay_steps;
        if (c.staircase) p = std::floor(p);
        lr = base_lr * std::pow(c.decay_rate, p);
    } else if (c.schedule == 3) {
        int k = 0;
        while (k < c.n_boundaries && iteration > c.boundaries[k]) ++k;
        lr = base_lr * c.values[k];
    }
    const double t = (double)(iteration + 1);
    OptimRates r;
    r.lr = lr;
    r.lr_f32 = (float)lr;
    r.alpha_f32 = (float)(lr * std::sqrt(1.0 - std::pow(beta2, t)) / (1.0 - std::pow(beta1, t)));
    return r;
}

// sum of one value per thread over the 256-thread workgroup, in ONE fixed order whatever else runs on the chip: a shuffle
// tree inside each wave (offsets 32 .. 1), then the four wave sums through LDS as ((s0 + s1) + s2) + s3.  No atomics
__device__ __forceinline__ float block_sum_256(float x, float* wsum) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    return ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
}

// adam_slab_block without the update: the same lanes, accumulators and order, so the stored g carries the fused launch's bits;
// returns the thread's sum of squares of its non-frozen gradients (index order).  A twin for adam_moments' reason
template <int VEC>
__device__ __forceinline__ float grad_slab_block(float* __restrict__ g, const uint8_t* __restrict__ kinds, const AdamSeg sg, int b,
                                                 float (*red)[256]) {
#pragma clang fp contract(off)
    const int e = threadIdx.x & 63, sl = threadIdx.x >> 6;
    const int64_t i = ((int64_t)b * 64 + e) * VEC;
    float acc[8][VEC];
#pragma unroll
    for (int u = 0; u < 8; ++u)
#pragma unroll
        for (int j = 0; j < VEC; ++j) acc[u][j] = 0.f;
    if (i < sg.n) {
        int s = sl;
        for (; s + 28 < sg.S; s += 32) {
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float* src = sg.slab + (size_t)(s + 4 * u) * sg.stride + i;
                if constexpr (VEC == 4) {
                    const f32x4 q = *reinterpret_cast<const f32x4*>(src);
                    acc[u][0] += q[0]; acc[u][1] += q[1]; acc[u][2] += q[2]; acc[u][3] += q[3];
                } else {
                    acc[u][0] += src[0];
                }
            }
        }
        for (; s < sg.S; s += 4) {
            const float* src = sg.slab + (size_t)s * sg.stride + i;
#pragma unroll
            for (int j = 0; j < VEC; ++j) acc[0][j] += src[j];
        }
    }
#pragma unroll
    for (int j = 0; j < VEC; ++j)
        red[sl][e * VEC + j] = ((acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j])) + ((acc[4][j] + acc[5][j]) + (acc[6][j] + acc[7][j]));
    __syncthreads();
    float sq = 0.f;
    if (sl == 0 && i < sg.n) {
#pragma unroll
        for (int j = 0; j < VEC; ++j) {
            const float gi = ((red[0][e * VEC + j] + red[1][e * VEC + j]) + red[2][e * VEC + j]) + red[3][e * VEC + j];
            g[sg.off + i + j] = gi;
            if (!kinds || kinds[sg.off + i + j] != KIND_FROZEN) {
                const float gg = gi * gi;
                sq = sq + gg;
            }
        }
    }
    return sq;
}


// The first launch of the finish + update path: the workgroups and segments of adam_segments_kernel, with no weight moved.
// A slab segment is summed by grad_slab_block and g stored; a plain segment reads g.  Every thread adds the squares
// of its (at most four) non-frozen gradients in index order, the workgroup sums them (block_sum_256): one fp32 partial per
// workgroup, the same bits on every run and for every number of candidates in flight
__global__ __launch_bounds__(256) void grad_finish_kernel(float* __restrict__ g, const AdamSegTable tab,
                                                          const uint8_t* __restrict__ kinds, float* __restrict__ partials) {
    __shared__ float red[4][256];
    __shared__ float wsum[4];
    int si = 0;
    while (si + 1 < tab.count && (int)blockIdx.x >= tab.seg[si + 1].block0) ++si;
    const AdamSeg sg = tab.seg[si];
    const int b = (int)blockIdx.x - sg.block0;
    float sq = 0.f;
    if (sg.slab == nullptr) {
#pragma clang fp contract(off)
        const int64_t base = (int64_t)b * ADAM_PLAIN_PER_BLOCK;
#pragma unroll
        for (int k = 0; k < ADAM_PLAIN_PER_BLOCK / 256; ++k) {
            const int64_t i = base + k * 256 + threadIdx.x;
            if (i < sg.n && (!kinds || kinds[sg.off + i] != KIND_FROZEN)) {
                const float gi = g[sg.off + i];
                const float gg = gi * gi;
                sq = sq + gg;
            }
        }
    } else {
        const bool vec = (sg.n % 4 == 0) && (sg.stride % 4 == 0) && (sg.off % 4 == 0) &&
                         (reinterpret_cast<uintptr_t>(sg.slab) % 16 == 0);
        sq = vec ? grad_slab_block<4>(g, kinds, sg, b, red) : grad_slab_block<1>(g, kinds, sg, b, red);
    }
    const float total = block_sum_256(sq, wsum);
    if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

void launch_grad_finish(float* g, const AdamSegTable& tab, const uint8_t* kinds, float* partials, hipStream_t s) {
    if (tab.blocks == 0) return;
    hipLaunchKernelGGL(grad_finish_kernel, dim3((unsigned)tab.blocks), dim3(256), 0, s, g, tab, kinds, partials);
    CMOOP_HIP(hipGetLastError());
}

// The second launch: ONE workgroup.  Thread t sums the partials [t chunk, (t + 1) chunk) in index order in double
// (chunk = ceil(n / 256): a function of n alone), thread 0 then the 256 chunk sums in index order
__global__ __launch_bounds__(256) void clip_scale_kernel(const float* __restrict__ partials, int n, double clip,
                                                         OptimRecord* __restrict__ rec) {
    __shared__ double part[256];
    const int chunk = (n + 255) / 256;
    const int lo = min(n, (int)threadIdx.x * chunk), hi = min(n, lo + chunk);
    double acc = 0.0;
    for (int i = lo; i < hi; ++i) acc += (double)partials[i];
    part[threadIdx.x] = acc;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sum = 0.0;
    for (int i = 0; i < 256; ++i) sum += part[i];
    const double norm = sqrt(sum);
    rec->sumsq = sum;
    rec->norm = (float)norm;
    rec->scale = (clip > 0.0 && norm > clip) ? (float)(clip / norm) : 1.0f;   // an inactive clip is exactly 1: g * scale keeps g's bits
}

void launch_clip_scale(const float* partials, int n_partials, double clip, OptimRecord* rec, hipStream_t s) {
    CMOOP_REQUIRE(n_partials >= 0 && n_partials < (1 << 30), "clip_scale: too many partials");
    hipLaunchKernelGGL(clip_scale_kernel, dim3(1), dim3(256), 0, s, partials, n_partials, clip, rec);
    CMOOP_HIP(hipGetLastError());
}

// one element of the third launch, Keras' order: clip, decoupled decay with the un-corrected rate, then adam_update on the
// decayed weight -- every operation a separately rounded fp32 operation.  A frozen element (BatchNorm moving statistics)
// keeps w, m and v.  A NaN gradient passes the value clamp unchanged
__device__ __forceinline__ void adamw_element(float& wi, float& mi, float& vi, float gi, unsigned kind, float scale, float alpha,
                                              float lr, const AdamwArgs& a) {
#pragma clang fp contract(off)
    if (kind == KIND_FROZEN) return;
    gi = gi * scale;
    if (a.clipvalue > 0.f) gi = gi < -a.clipvalue ? -a.clipvalue : (gi > a.clipvalue ? a.clipvalue : gi);
    if (a.weight_decay > 0.f && (a.decay_all || kind == KIND_KERNEL)) {
        const float d = wi * a.weight_decay;
        wi = wi - d * lr;
    }
    adam_moments(mi, vi, gi, a.c1, a.c2);
    wi = wi - adam_delta(mi, vi, alpha, a.eps);
}

// The third launch: grid-stride over the whole arena, 16-byte accesses (4 kind bytes per float4) when vec, the last n % 4
// elements and an unaligned arena one element at a time.  kinds null: every element is a kernel tensor
__global__ __launch_bounds__(256) void adamw_kernel(float* __restrict__ w, const float* __restrict__ g, float* __restrict__ m,
                                                    float* __restrict__ v, const uint8_t* __restrict__ kinds, int64_t n,
                                                    const OptimRecord* __restrict__ rec, const AdamwArgs a,
                                                    const StepState* __restrict__ st, const float* __restrict__ alpha_table,
                                                    const float* __restrict__ lr_table, int vec) {
    float alpha = a.alpha, lr = a.lr;
    if (st) { alpha = alpha_table[st->iter]; lr = lr_table[st->iter]; }
    const float scale = rec->scale;
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t q = t0; q < n4; q += stride) {
        f32x4 wq = reinterpret_cast<f32x4*>(w)[q], mq = reinterpret_cast<f32x4*>(m)[q], vq = reinterpret_cast<f32x4*>(v)[q];
        const f32x4 gq = reinterpret_cast<const f32x4*>(g)[q];
        const uint32_t kq = kinds ? reinterpret_cast<const uint32_t*>(kinds)[q] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float wi = wq[j], mi = mq[j], vi = vq[j];
            adamw_element(wi, mi, vi, gq[j], (kq >> (8 * j)) & 0xffu, scale, alpha, lr, a);
            wq[j] = wi; mq[j] = mi; vq[j] = vi;
        }
        reinterpret_cast<f32x4*>(w)[q] = wq;
        reinterpret_cast<f32x4*>(m)[q] = mq;
        reinterpret_cast<f32x4*>(v)[q] = vq;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) {
        float wi = w[i], mi = m[i], vi = v[i];
        adamw_element(wi, mi, vi, g[i], kinds ? kinds[i] : 0u, scale, alpha, lr, a);
        w[i] = wi; m[i] = mi; v[i] = vi;
    }
}

constexpr int64_t ADAMW_MAX_BLOCKS = 2048;   // 8 workgroups per CU; a larger arena wraps the grid-stride loop

void launch_adamw(float* w, const float* g, float* m, float* v, const uint8_t* kinds, int64_t n, const OptimRecord* rec,
                  const AdamwArgs& a, hipStream_t s, const StepState* st, const float* alpha_table, const float* lr_table) {
    if (n == 0) return;
    CMOOP_REQUIRE(rec != nullptr, "adamw: the clip record is NULL");
    CMOOP_REQUIRE(!st || (alpha_table && lr_table), "adamw: a device step state needs both rate tables");
    auto al = [](const void* p, size_t k) { return reinterpret_cast<uintptr_t>(p) % k == 0; };
    const int vec = al(w, 16) && al(g, 16) && al(m, 16) && al(v, 16) && al(kinds, 4);
    const int64_t items = vec ? std::max<int64_t>(n / 4, 1) : n;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(items, 256), ADAMW_MAX_BLOCKS);
    hipLaunchKernelGGL(adamw_kernel, dim3(grid), dim3(256), 0, s, w, g, m, v, kinds, n, rec, a, st, alpha_table, lr_table, vec);
    CMOOP_HIP(hipGetLastError());
}

// ---- weight EMA: an averaged copy of the parameter arena (kernels.h) -----------------------------------------------------------
void ema_check(const EmaCfg& c) {
    CMOOP_REQUIRE(std::isfinite(c.momentum) && c.momentum >= 0 && c.momentum < 1, "ema: momentum must be finite and in [0, 1)");
    CMOOP_REQUIRE(c.warmup == 0 || c.warmup == 1, "ema: warmup must be 0 or 1");
    CMOOP_REQUIRE(c.reserved == 0, "ema: reserved must be 0");
}

EmaRates ema_rates(const EmaCfg& c, int64_t iteration) {
    CMOOP_REQUIRE(iteration >= 0, "ema rates: iteration must be >= 0");
    double m = c.momentum;
    if (c.warmup) m = std::min(m, (1.0 + (double)iteration) / (10.0 + (double)iteration));
    EmaRates r;
    r.m = m;
    r.mf = (float)m;
    r.omf = (float)(1.0 - m);
    return r;
}

// one element of the average: two products and one add, each rounded separately, for adam_update's reason; a frozen
// element (BatchNorm moving statistics) is a copy of the weight, so the average is a complete inference parameter set
__device__ __forceinline__ float ema_element(float ai, float wi, unsigned kind, float mf, float omf) {
#pragma clang fp contract(off)
    if (kind == KIND_FROZEN) return wi;
    const float keep = mf * ai;
    const float take = omf * wi;
    return keep + take;
}

// A launch of its own after the optimiser's: reads w (already updated), a and the kind bytes, writes a only.  Shaped as
// adamw_kernel: grid-stride, 16-byte accesses (4 kind bytes per float4) when vec, the last n % 4 elements and an unaligned
// arena one element at a time.  kinds null: every element is trainable
__global__ __launch_bounds__(256) void ema_kernel(float* __restrict__ a, const float* __restrict__ w,
                                                  const uint8_t* __restrict__ kinds, int64_t n, float mf, float omf,
                                                  const StepState* __restrict__ st, const EmaPair* __restrict__ table, int vec) {
    if (st) { const EmaPair p = table[st->iter]; mf = p.mf; omf = p.omf; }
    const int64_t t0 = (int64_t)blockIdx.x * 256 + threadIdx.x, stride = (int64_t)gridDim.x * 256;
    const int64_t n4 = vec ? n / 4 : 0;
    for (int64_t q = t0; q < n4; q += stride) {
        f32x4 aq = reinterpret_cast<f32x4*>(a)[q];
        const f32x4 wq = reinterpret_cast<const f32x4*>(w)[q];
        const uint32_t kq = kinds ? reinterpret_cast<const uint32_t*>(kinds)[q] : 0u;
#pragma unroll
        for (int j = 0; j < 4; ++j) aq[j] = ema_element(aq[j], wq[j], (kq >> (8 * j)) & 0xffu, mf, omf);
        reinterpret_cast<f32x4*>(a)[q] = aq;
    }
    for (int64_t i = 4 * n4 + t0; i < n; i += stride) a[i] = ema_element(a[i], w[i], kinds ? kinds[i] : 0u, mf, omf);
}

void launch_ema(float* a, const float* w, const uint8_t* kinds, int64_t n, float mf, float omf, hipStream_t s, const StepState* st,
                const EmaPair* table) {
    if (n == 0) return;
    CMOOP_REQUIRE(a && w && a != w, "ema: the average and the weights are two arenas");
    CMOOP_REQUIRE(!st || table, "ema: a device step state needs the rate table");
    auto al = [](const void* p, size_t k) { return reinterpret_cast<uintptr_t>(p) % k == 0; };
    const int vec = al(a, 16) && al(w, 16) && al(kinds, 4);
    const int64_t items = vec ? std::max<int64_t>(n / 4, 1) : n;
    const unsigned grid = (unsigned)std::min<int64_t>(cdiv64(items, 256), ADAMW_MAX_BLOCKS);
    hipLaunchKernelGGL(ema_kernel, dim3(grid), dim3(256), 0, s, a, w, kinds, n, mf, omf, st, table, vec);
    CMOOP_HIP(hipGetLastError());
}

// Epoch shuffle on the device (Keras fit(shuffle=True), nsga_penalty.py:383; seeded here): the permutation that sorts
// the keys (fmix32(prefix ^ i) << 32 | i), i.e. exactly what the host twin (net.hip epoch_permutation, oracle/rng.py)
// produces with std::sort -- computed as a rank sort: out[#{j : key_j < key_i}] = i.  O(n^2) compares on LDS tiles
// (0.6 G for n = 24 000: tens of microseconds chip-wide), no host sort, no H2D copy, no stream stall.
__global__ __launch_bounds__(256) void epoch_permutation_kernel(uint32_t prefix, int n, int32_t* __restrict__ out) {
    __shared__ uint32_t hs[1024];
    const int t = threadIdx.x;
    const int i = blockIdx.x * 256 + t;
    const uint32_t hi = fmix32(prefix ^ (uint32_t)i);
    int rank = 0;
    for (int j0 = 0; j0 < n; j0 += 1024) {
#pragma unroll
        for (int u = 0; u < 4; ++u) hs[t + 256 * u] = fmix32(prefix ^ (uint32_t)(j0 + t + 256 * u));
        __syncthreads();
        const int lim = min(1024, n - j0);
        for (int j = 0; j < lim; ++j) {
            const uint32_t hj = hs[j];
            rank += (hj < hi || (hj == hi && j0 + j < i)) ? 1 : 0;
        }
        __syncthreads();
    }
    if (i < n) out[rank] = i;
}

void launch_epoch_permutation(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out, hipStream_t s) {
    CMOOP_REQUIRE(n >= 0 && n <= EPOCH_PERMUTATION_DEVICE_MAX, "device epoch permutation: n too large (use the host twin)");
    if (n == 0) return;
    hipLaunchKernelGGL(epoch_permutation_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s,
                       rng_prefix(seed, STREAM_SHUFFLE, epoch), (int)n, out);
    CMOOP_HIP(hipGetLastError());
}

// confusion_matrix(y_true, y_pred, labels=range(C)) (nsga_penalty.py:355): LDS histogram
__global__ __launch_bounds__(256) void confusion_kernel(const int32_t* __restrict__ yt, const int32_t* __restrict__ yp,
                                                        int64_t n, int C, int force_true_zero, long long* __restrict__ cm) {
    extern __shared__ int hist[];
    for (int i = threadIdx.x; i < C * C; i += 256) hist[i] = 0;
    __syncthreads();
    for (int64_t i = threadIdx.x; i < n; i += 256) {
        const int a = force_true_zero ? 0 : yt[i];
        const int b = yp[i];
        if ((unsigned)a < (unsigned)C && (unsigned)b < (unsigned)C) atomicAdd(&hist[a * C + b], 1);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < C * C; i += 256) cm[i] = hist[i];
}

void launch_confusion(const int32_t* y_true, const int32_t* y_pred, int64_t n, int C, int force_true_zero, int64_t* cm,
                      hipStream_t s) {
    CMOOP_REQUIRE(C * C * 4 <= 64 * 1024, "confusion: too many classes");
    hipLaunchKernelGGL(confusion_kernel, dim3(1), dim3(256), C * C * sizeof(int), s, y_true, y_pred, n, C,
                       force_true_zero, reinterpret_cast<long long*>(cm));
    CMOOP_HIP(hipGetLastError());
}

// ---- operating-point read-out: score ranking per class (kernels.h) -------------------------------------------------------------
void opoint_check(const OpointCfg& c) {
    CMOOP_REQUIRE(std::isfinite(c.recall) && c.recall >= 0 && c.recall <= 1, "opoint: recall must be finite and in [0, 1]");
    CMOOP_REQUIRE(c.objective == 0 || c.objective == 1, "opoint: objective must be 0 or 1");
    CMOOP_REQUIRE(c.reserved == 0, "opoint: reserved must be 0");
}

void opoint_check_shape(int64_t n, int C) {
    CMOOP_REQUIRE(C >= 1 && C <= OPOINT_MAX_CLASSES, "opoint: classes must be in [1, " + std::to_string(OPOINT_MAX_CLASSES) + "]");
    CMOOP_REQUIRE(n >= 0 && n <= OPOINT_MAX_ROWS,
                  "opoint: " + std::to_string(n) + " rows, the read-out ranks at most " + std::to_string(OPOINT_MAX_ROWS) + " (n^2 compares)");
}

// the total order on float bit patterns: negative values reversed below the positive ones, -0 < +0, NaNs at both ends
__device__ __forceinline__ uint32_t score_key(float s) {
    const uint32_t b = __float_as_uint(s);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float score_of_key(uint32_t k) {
    return __uint_as_float((k >> 31) ? (k ^ 0x80000000u) : ~k);
}

// The transpose [n][C] -> [C][n]: thread = one row, its C scores read in order (a wave covers 64 C consecutive floats), each
// class's keys written unit-stride.  Every later pass reads one class's keys contiguously
__global__ __launch_bounds__(256) void score_keys_kernel(const float* __restrict__ p, uint32_t* __restrict__ key, int n, int C) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* row = p + (size_t)i * C;
    for (int c = 0; c < C; ++c) key[(size_t)c * n + i] = score_key(row[c]);
}

void launch_score_keys(const float* p, uint32_t* key, int64_t n, int C, hipStream_t s) {
    opoint_check_shape(n, C);
    if (n == 0) return;
    hipLaunchKernelGGL(score_keys_kernel, dim3((unsigned)cdiv64(n, 256)), dim3(256), 0, s, p, key, (int)n, C);
    CMOOP_HIP(hipGetLastError());
}

// Shaped as epoch_permutation_kernel: a workgroup owns 256 rows i of class blockIdx.y and walks every row j in runs of
// ROC_TILE staged in LDS as (key, y[j] == c) pairs.  In the compare loop all lanes read the SAME 8-byte LDS word (a broadcast:
// no bank conflict) and add into four int32 counters -- at most n <= 2^18 each.  Rows past n are neither staged (the n % 256
// and n % ROC_TILE remainders read nothing past their ends) nor compared (lim) nor written
__global__ __launch_bounds__(256) void roc_counts_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ y,
                                                         int32_t* __restrict__ cnt, int n) {
    __shared__ uint2 tile[ROC_TILE];
    const int t = threadIdx.x, c = blockIdx.y;
    const int i = blockIdx.x * 256 + t;
    const uint32_t* kc = key + (size_t)c * n;
    const uint32_t ki = i < n ? kc[i] : 0u;
    uint32_t ge_all = 0, gt_all = 0, ge_pos = 0, gt_pos = 0;
    for (int j0 = 0; j0 < n; j0 += ROC_TILE) {
#pragma unroll
        for (int u = 0; u < ROC_TILE / 256; ++u) {
            const int j = j0 + t + 256 * u;
            if (j < n) tile[t + 256 * u] = make_uint2(kc[j], y[j] == c ? 1u : 0u);
        }
        __syncthreads();
        const int lim = min(ROC_TILE, n - j0);
        for (int j = 0; j < lim; ++j) {
            const uint2 e = tile[j];
            const uint32_t ge = e.x >= ki ? 1u : 0u, gt = e.x > ki ? 1u : 0u;
            ge_all += ge; gt_all += gt;
            ge_pos += ge & e.y; gt_pos += gt & e.y;
        }
        __syncthreads();
    }
    if (i < n) {
        int32_t* out = cnt + ((size_t)c * n + i) * 4;
        out[0] = (int32_t)ge_pos; out[1] = (int32_t)(ge_all - ge_pos); out[2] = (int32_t)gt_pos; out[3] = (int32_t)(gt_all - gt_pos);
    }
}

void launch_roc_counts(const uint32_t* key, const int32_t* y, int32_t* cnt, int64_t n, int C, hipStream_t s) {
    opoint_check_shape(n, C);
    if (n == 0) return;
    hipLaunchKernelGGL(roc_counts_kernel, dim3((unsigned)cdiv64(n, 256), (unsigned)C), dim3(256), 0, s, key, y, cnt, (int)n);
    CMOOP_HIP(hipGetLastError());
}

// integer sums over the 256-thread workgroup in block_sum_256's order (shuffle tree, then the four wave sums through LDS);
// integer addition is exact in any order, the fixed one keeps the code one shape with the float reductions
__device__ __forceinline__ long long block_sum_256_i64(long long x, long long* wsum) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) x = x + __shfl_down(x, off, 64);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = x;
    __syncthreads();
    const long long r = ((wsum[0] + wsum[1]) + wsum[2]) + wsum[3];
    __syncthreads();   // wsum is reused
    return r;
}

// One workgroup per class.  Pass 1: P_c and S = sum over positives of (ge_neg + gt_neg), so U2 = 2 N P - S (the contract's sum
// with N taken out of it; int64).  Then k from ONE double product and one ceil.  Pass 2: among positives with ge_pos >= k the
// largest key and its (ge_pos, ge_neg) -- rows with equal keys carry equal counts, so which of them wins a tie changes nothing
__global__ __launch_bounds__(256) void opoint_select_kernel(const uint32_t* __restrict__ key, const int32_t* __restrict__ y,
                                                            const int32_t* __restrict__ cnt, int n, double recall,
                                                            OpointClass* __restrict__ rec) {
    __shared__ long long wsum[4];
    __shared__ uint32_t wkey[4];
    __shared__ int wtp[4], wfp[4], wany[4];
    const int t = threadIdx.x, c = blockIdx.x;
    const uint32_t* kc = key + (size_t)c * n;
    const int32_t* cc = cnt + (size_t)c * n * 4;
    long long p = 0, sneg = 0;
    for (int i = t; i < n; i += 256) {
        if (y[i] == c) {
            ++p;
            sneg += (long long)cc[4 * i + 1] + (long long)cc[4 * i + 3];
        }
    }
    const long long P = block_sum_256_i64(p, wsum);
    const long long S = block_sum_256_i64(sneg, wsum);
    const long long N = (long long)n - P;
    int k = 0;
    if (P > 0) {
        const double want = ceil(recall * (double)P);
        k = (int)want;
        k = k < 1 ? 1 : k;
        k = k > (int)P ? (int)P : k;
    }
    uint32_t bk = 0;
    int btp = 0, bfp = 0, any = 0;
    for (int i = t; i < n; i += 256) {
        if (y[i] != c) continue;
        const int gp = cc[4 * i];
        const uint32_t ki = kc[i];
        if (gp >= k && (!any || ki > bk)) { bk = ki; btp = gp; bfp = cc[4 * i + 1]; any = 1; }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const uint32_t ok = __shfl_down(bk, off, 64);
        const int otp = __shfl_down(btp, off, 64), ofp = __shfl_down(bfp, off, 64), oany = __shfl_down(any, off, 64);
        if (oany && (!any || ok > bk)) { bk = ok; btp = otp; bfp = ofp; any = 1; }
    }
    if ((t & 63) == 0) { wkey[t >> 6] = bk; wtp[t >> 6] = btp; wfp[t >> 6] = bfp; wany[t >> 6] = any; }
    __syncthreads();
    if (t != 0) return;
    for (int w = 1; w < 4; ++w)
        if (wany[w] && (!any || wkey[w] > bk)) { bk = wkey[w]; btp = wtp[w]; bfp = wfp[w]; any = 1; }
    OpointClass r;
    r.P = (int32_t)P; r.N = (int32_t)N; r.k = k;
    if (P > 0) {
        r.u2 = 2 * N * P - S;
        r.tp = btp; r.fp = bfp; r.thr = score_of_key(bk);
    } else {
        r.u2 = 0;
        r.tp = 0; r.fp = 0; r.thr = INFINITY;
    }
    rec[c] = r;
}

void launch_opoint_select(const uint32_t* key, const int32_t* y, const int32_t* cnt, int64_t n, int C, double recall,
                          OpointClass* rec, hipStream_t s) {
    opoint_check_shape(n, C);
    hipLaunchKernelGGL(opoint_select_kernel, dim3((unsigned)C), dim3(256), 0, s, key, y, cnt, (int)n, recall, rec);
    CMOOP_HIP(hipGetLastError());
}

void opoint_summary(const OpointClass* rec, int C, double out[4]) {
    double fpr = 0.0, rec_sum = 0.0, auc = 0.0;
    int scored = 0, ranked = 0;
    for (int c = 0; c < C; ++c) {
        const OpointClass& r = rec[c];
        if (r.P < 1) continue;
        ++scored;
        fpr += r.N > 0 ? (double)r.fp / (double)r.N : 0.0;
        rec_sum += (double)r.tp / (double)r.P;
        if (r.N >= 1) { auc += (double)r.u2 / (2.0 * (double)r.P * (double)r.N); ++ranked; }
    }
    out[0] = scored ? fpr / (double)scored : 0.0;
    out[1] = scored ? rec_sum / (double)scored : 0.0;
    out[2] = ranked ? auc / (double)ranked : NAN;
    out[3] = (double)scored;
}

}  // namespace cmoop
