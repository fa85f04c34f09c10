// Depthwise k x k convolution (SAME, stride 1, depth multiplier 1) of the separable layers of topologies A_ds / B_ds:
// forward, data gradient (the forward body with flipped taps and an optional x > 0 mask) and weight gradient.
// NHWC fp32 in every gemm_mode, C a power of two in 16..512, K in {3, 5}.  Memory-bound VALU kernels: no MFMA.
//
// Work item = (sample, run of RH image rows, column): a lane owns 4 channels of one item and walks down its column.
// Every input row of the run (plus the K - 1 halo rows) is loaded ONCE per lane, as K 16-byte loads for the K horizontal
// taps, and feeds the K outputs (forward) / the K dY rows (weight gradient) it overlaps from registers.  A workgroup is
// 256 threads = CB4 channel quads x 256 / CB4 items with consecutive columns, so its loads run along the NHWC rows;
// blockIdx.y selects the chunk of CB4 * 4 channels.
#include "kernels.h"

#include <algorithm>

namespace cmoop {
namespace {

constexpr int DW_MAX_CB4 = 16;         // channel quads per workgroup (64 channels = 256 contiguous bytes per pixel)
constexpr int DW_TARGET_THREADS = 256 * 1024;
constexpr int DW_ITEMS_PER_SLOT = 4;   // weight gradient: items a lane walks before the workgroup reduction
constexpr int DW_MAX_SLICES = 512;
constexpr int64_t DW_MAX_SLAB_FLOATS = 1 << 22;

struct DwPlan {
    int cb4_log, slots, chunks;   // log2 channel quads per workgroup, items per workgroup, channel chunks (grid.y)
    int RH, runs, items;          // rows per run, runs per image, B * runs * W
};

DwPlan dw_plan(int B, int H, int W, int C, int KS) {
    CMOOP_REQUIRE(B >= 1 && H >= 1 && W >= 1, "dwconv: bad shape");
    CMOOP_REQUIRE(KS == 3 || KS == 5, "dwconv: kernel size must be 3 or 5");
    CMOOP_REQUIRE(C >= 16 && C <= 512 && ilog2_exact(C) >= 0, "dwconv: channels must be a power of two in 16..512");
    CMOOP_REQUIRE((int64_t)B * H * W * C < (1ll << 29), "dwconv: activation exceeds 2^29 elements (32-bit offsets)");
    DwPlan p;
    const int C4 = C / 4, CB4 = std::min(C4, DW_MAX_CB4);
    p.cb4_log = ilog2_exact(CB4);
    p.slots = 256 / CB4;
    p.chunks = C4 / CB4;
    // shorter runs (more halo rows re-read through the caches) until the launch fills the chip
    p.RH = std::min(H, 16);
    while (p.RH > 4 && (int64_t)B * cdiv(H, p.RH) * W * C4 < DW_TARGET_THREADS) p.RH = (p.RH + 1) / 2;
    p.runs = cdiv(H, p.RH);
    p.items = B * p.runs * W;
    return p;
}

// item -> (sample b, first / one-past-last row of the run, column): 32-bit divisions, once per item
struct DwItem { int row_base, h0, h1, w; };
__device__ __forceinline__ DwItem dw_item(int item, int H, int W, int RH, int runs) {
    const unsigned q = (unsigned)item / (unsigned)W;
    const unsigned b = q / (unsigned)runs, run = q - b * (unsigned)runs;
    DwItem it;
    it.w = (int)((unsigned)item - q * (unsigned)W);
    it.row_base = (int)b * H;
    it.h0 = (int)run * RH;
    it.h1 = min(H, it.h0 + RH);
    return it;
}

// the K horizontal taps of image row r around column w (zeros outside the image)
template <int K>
__device__ __forceinline__ void dw_load_row(const float* __restrict__ X, int row_base, int r, int w, int H, int W, int C, int c,
                                            f32x4 (&x)[K]) {
    constexpr int P = (K - 1) / 2;
    const bool rv = r >= 0 && r < H;
    const int base = ((row_base + r) * W + (w - P)) * C + c;
#pragma unroll
    for (int kx = 0; kx < K; ++kx) {
        const int col = w + kx - P;
        const bool v = rv && col >= 0 && col < W;
        x[kx] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (v) x[kx] = *reinterpret_cast<const f32x4*>(X + base + kx * C);
    }
}

// Y[b,h,w,c] = sum_{ky,kx} X[b,h+ky-p,w+kx-p,c] * Wt[ky][kx][c];  FLIP: the taps reversed (the data gradient, X = dY);
// mask != null: Y = mask > 0 ? Y : 0 (ReLU backward of the layer's input)
template <int K, bool FLIP>
__global__ __launch_bounds__(256) void dwconv_fwd_kernel(const float* __restrict__ X, const float* __restrict__ Wt,
                                                         float* __restrict__ Y, const float* __restrict__ mask, int H, int W,
                                                         int C, int RH, int runs, int items, int cb4_log) {
    constexpr int P = (K - 1) / 2, TAPS = K * K;
    __shared__ f32x4 wl[TAPS * DW_MAX_CB4];
    const int t = threadIdx.x, CB4 = 1 << cb4_log;
    const int cql = t & (CB4 - 1), slot = t >> cb4_log;
    const int c0 = (int)blockIdx.y * CB4 * 4;
    for (int i = t; i < TAPS * CB4; i += 256) {   // the workgroup's K*K x (CB4*4) weights, staged once
        const int tap = i >> cb4_log, q = i & (CB4 - 1);
        wl[tap * DW_MAX_CB4 + q] = *reinterpret_cast<const f32x4*>(Wt + tap * C + c0 + q * 4);
    }
    __syncthreads();
    const int item = (int)blockIdx.x * (256 >> cb4_log) + slot;
    if (item >= items) return;
    f32x4 wr[TAPS];
#pragma unroll
    for (int i = 0; i < TAPS; ++i) wr[i] = wl[(FLIP ? TAPS - 1 - i : i) * DW_MAX_CB4 + cql];
    const DwItem it = dw_item(item, H, W, RH, runs);
    const int c = c0 + cql * 4;
    f32x4 acc[K];   // acc[j]: output row r - P + j, which input row r reaches through vertical tap K - 1 - j
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = it.h0 - P; r < it.h1 + P; ++r) {
        f32x4 x[K];
        dw_load_row<K>(X, it.row_base, r, it.w, H, W, C, c, x);
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc[j] += x[kx] * wr[(K - 1 - j) * K + kx];
        const int h = r - P;   // complete: r is its last input row
        if (h >= it.h0) {
            const int o = ((it.row_base + h) * W + it.w) * C + c;
            f32x4 v = acc[0];
            if (mask) {
                const f32x4 m = *reinterpret_cast<const f32x4*>(mask + o);
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = m[e] > 0.f ? v[e] : 0.f;
            }
            *reinterpret_cast<f32x4*>(Y + o) = v;
        }
#pragma unroll
        for (int j = 0; j + 1 < K; ++j) acc[j] = acc[j + 1];
        acc[K - 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// P[slice][ky][kx][c] = sum over the slice's items of X[b,h+ky-p,w+kx-p,c] * dY[b,h,w,c].  A slice is `ips` consecutive
// items; lane (slot, channel quad) walks items slot, slot + slots, ... keeping the K*K sums of its 4 channels, then the
// workgroup adds its lanes in a fixed order (xor-shuffles inside a wave, the four waves through LDS): no atomics
template <int K>
__global__ __launch_bounds__(256) void dwconv_wgrad_kernel(const float* __restrict__ X, const float* __restrict__ dY,
                                                           float* __restrict__ Pout, int H, int W, int C, int RH, int runs,
                                                           int items, int ips, int cb4_log) {
    constexpr int P = (K - 1) / 2, TAPS = K * K;
    __shared__ f32x4 red[TAPS][4][DW_MAX_CB4];
    const int t = threadIdx.x, CB4 = 1 << cb4_log, slots = 256 >> cb4_log;
    const int cql = t & (CB4 - 1), slot = t >> cb4_log;
    const int c0 = (int)blockIdx.y * CB4 * 4, c = c0 + cql * 4;
    const int i0 = (int)blockIdx.x * ips, i1 = min(items, i0 + ips);
    f32x4 acc[TAPS];
#pragma unroll
    for (int i = 0; i < TAPS; ++i) acc[i] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int item = i0 + slot; item < i1; item += slots) {
        const DwItem it = dw_item(item, H, W, RH, runs);
        f32x4 d[K];   // d[j]: dY row r - P + j of this run (zero outside it), paired with vertical tap K - 1 - j
#pragma unroll
        for (int j = 0; j < K; ++j) d[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int r = it.h0 - P; r < it.h1 + P; ++r) {
#pragma unroll
            for (int j = 0; j + 1 < K; ++j) d[j] = d[j + 1];
            const int hn = r + P;
            d[K - 1] = f32x4{0.f, 0.f, 0.f, 0.f};
            if (hn >= it.h0 && hn < it.h1) d[K - 1] = *reinterpret_cast<const f32x4*>(dY + ((it.row_base + hn) * W + it.w) * C + c);
            f32x4 x[K];
            dw_load_row<K>(X, it.row_base, r, it.w, H, W, C, c, x);
#pragma unroll
            for (int j = 0; j < K; ++j)
#pragma unroll
                for (int kx = 0; kx < K; ++kx) acc[(K - 1 - j) * K + kx] += x[kx] * d[j];
        }
    }
    const int lane = t & 63, wave = t >> 6;
#pragma unroll
    for (int i = 0; i < TAPS; ++i) {
        f32x4 v = acc[i];
        for (int off = 32; off >= CB4; off >>= 1) {
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] += __shfl_xor(v[e], off, 64);
        }
        if (lane < CB4) red[i][wave][cql] = v;
    }
    __syncthreads();
    float* out = Pout + (size_t)blockIdx.x * TAPS * C;
    for (int i = t; i < TAPS * CB4; i += 256) {
        const int tap = i >> cb4_log, q = i & (CB4 - 1);
        const f32x4 s = ((red[tap][0][q] + red[tap][1][q]) + red[tap][2][q]) + red[tap][3][q];
        *reinterpret_cast<f32x4*>(out + tap * C + c0 + q * 4) = s;
    }
}

}  // namespace

void launch_dwconv_fwd(const float* X, const float* Wt, float* Y, int B, int H, int W, int C, int KS, int flip, const float* mask,
                       hipStream_t s) {
    const DwPlan p = dw_plan(B, H, W, C, KS);
    const dim3 grid((unsigned)cdiv(p.items, p.slots), (unsigned)p.chunks);
#define CMOOP_DW_FWD(K, FL) \
    hipLaunchKernelGGL((dwconv_fwd_kernel<K, FL>), grid, dim3(256), 0, s, X, Wt, Y, mask, H, W, C, p.RH, p.runs, p.items, p.cb4_log)
    if (KS == 3) { if (flip) CMOOP_DW_FWD(3, true); else CMOOP_DW_FWD(3, false); }
    else { if (flip) CMOOP_DW_FWD(5, true); else CMOOP_DW_FWD(5, false); }
#undef CMOOP_DW_FWD
    CMOOP_HIP(hipGetLastError());
}

static int dw_items_per_slice(const DwPlan& p, int C, int KS) {
    const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(DW_MAX_SLICES, DW_MAX_SLAB_FLOATS / ((int64_t)KS * KS * C)));
    const int64_t want = std::min<int64_t>(cap, cdiv64(p.items, (int64_t)p.slots * DW_ITEMS_PER_SLOT));
    return (int)cdiv64(p.items, want);
}

int dwconv_wgrad_slices(int B, int H, int W, int C, int KS) {
    const DwPlan p = dw_plan(B, H, W, C, KS);
    return cdiv(p.items, dw_items_per_slice(p, C, KS));
}

void launch_dwconv_wgrad(const float* X, const float* dY, float* P, int B, int H, int W, int C, int KS, hipStream_t s) {
    const DwPlan p = dw_plan(B, H, W, C, KS);
    const int ips = dw_items_per_slice(p, C, KS);
    const dim3 grid((unsigned)cdiv(p.items, ips), (unsigned)p.chunks);
    if (KS == 3) hipLaunchKernelGGL(dwconv_wgrad_kernel<3>, grid, dim3(256), 0, s, X, dY, P, H, W, C, p.RH, p.runs, p.items, ips, p.cb4_log);
    else hipLaunchKernelGGL(dwconv_wgrad_kernel<5>, grid, dim3(256), 0, s, X, dY, P, H, W, C, p.RH, p.runs, p.items, ips, p.cb4_log);
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
