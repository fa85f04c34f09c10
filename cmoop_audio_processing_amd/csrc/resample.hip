// Polyphase resampler: rational rate change by up / down (gcd 1) with an odd-length centred FIR h of n_taps = 2 half + 1 taps.
// For a row x[0..L), x = 0 outside (include/cmoop.h, "resampling"):
//     n_out = ceil(L up / down);   y[n] = sum_i x[i] h[n down - i up + half]   over 0 <= n down - i up + half <= 2 half, 0 <= i < L
// which is scipy.signal.resample_poly(x, up, down) for the default filter (resample_filter below restates its design).
//
// Output n sits at position P = n down + half; it reads the tpp = ceil(n_taps / up) inputs i = floor(P / up) - tpp + 1 ..
// floor(P / up) against row p = P mod up of the polyphase table [up][tpp], which the host lays out in ascending i
// (tab[p][j] = h[p + (tpp - 1 - j) up], zero where that index passes the last tap).  A padded zero tap adds fmaf(x, 0, acc) = acc,
// so the sum is the definition's: one fp32 accumulator from 0.0f, terms in ascending i, one fmaf each -- the same bits from
// every launch shape.
//
// One launch serves clip batches [n_clips][L] and one long recording: a 256-thread workgroup owns `tile` consecutive outputs of
// one row, stages the input span they read (at most RESAMPLE_LDS_FLOATS, zero outside [0, L) of ITS row) into LDS with coalesced
// 4-byte loads and accumulates from LDS; lanes hold consecutive outputs, so their LDS reads step by down / up words (unit
// stride at ratio 1, conflict-free at every odd down when up = 1).  The table sits in device memory (86 KB at most for the
// default filter, L2-resident).  With up = 1 it has one row and its reads are wave-uniform.  Otherwise every lane reads its own
// row: where span and table fit 64 KiB of LDS together (every default filter up to up = 640) persistent workgroups copy the
// table into LDS once, rows at an odd stride, and stride over the tiles; a larger table is read from device memory row by row
// (a gather of 64 cache lines per load: 5x the time of the LDS form when both were measured at 160 / 441).
// The tile's first position and first input index are 64-bit, computed once per workgroup; everything inside the tile is 32-bit (the window_gather_kernel convention), and every staged
// load is predicated on 0 <= i < L after the final index is formed: a wrong index can only give a wrong value.
// HBM-bound: 4 L + 4 n_out bytes and tpp n_out FMA per row.  No atomics.
#include "kernels.h"
#include <cmath>
#include <numeric>
#include <stdexcept>
#include <string>

namespace cmoop {

namespace {
[[noreturn]] void resample_fail(const std::string& field, const std::string& rule, const std::string& got) {
    throw std::runtime_error("resample: " + field + " " + rule + " (got " + got + ")");
}

void check_ratio(int up, int down) {
    if (up < 1 || up > RESAMPLE_MAX_RATE) resample_fail("up", "must lie in 1..1024", std::to_string(up));
    if (down < 1 || down > RESAMPLE_MAX_RATE) resample_fail("down", "must lie in 1..1024", std::to_string(down));
    if (std::gcd(up, down) != 1)
        resample_fail("up / down", "must be reduced, gcd(up, down) = 1", std::to_string(up) + " / " + std::to_string(down));
}

// I0 from its power series sum_k ((x / 2)^2)^k / (k!)^2, summed until a term no longer changes the sum
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        const double next = sum + term;
        if (next == sum) break;
        sum = next;
    }
    return sum;
}
}  // namespace

int resample_filter_taps(int up, int down, int half_width) {
    check_ratio(up, down);
    if (half_width < 1 || half_width > RESAMPLE_MAX_HALF_WIDTH) resample_fail("half_width", "must lie in 1..4096", std::to_string(half_width));
    return 2 * half_width * std::max(up, down) + 1;
}

void resample_filter(int up, int down, int half_width, double beta, float* taps) {
    const int n_taps = resample_filter_taps(up, down, half_width);
    if (!(beta >= 0.0) || !std::isfinite(beta)) resample_fail("beta", "must be finite and >= 0", std::to_string(beta));
    const int half = (n_taps - 1) / 2;
    const double fc = 1.0 / (double)std::max(up, down), pi = 3.14159265358979323846, i0b = bessel_i0(beta);
    std::vector<double> h((size_t)n_taps);
    double sum = 0.0;
    for (int k = 0; k < n_taps; ++k) {
        const double m = (double)(k - half), r = m / (double)half;
        const double w = bessel_i0(beta * std::sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
        // pi (fc m) in this order: where fc m is an integer the tap is the rounding residue of that product, not 0, in scipy too
        const double a = pi * (fc * m);
        h[(size_t)k] = fc * (k == half ? 1.0 : std::sin(a) / a) * w;
        sum += h[(size_t)k];
    }
    for (int k = 0; k < n_taps; ++k) taps[k] = (float)((double)up * h[(size_t)k] / sum);
}

ResamplePlan resample_plan(int64_t n_samples, int up, int down, int n_taps) {
    check_ratio(up, down);
    if (n_taps < 1 || n_taps % 2 == 0) resample_fail("n_taps", "must be odd and >= 1", std::to_string(n_taps));
    const int tpp = (int)cdiv64(n_taps, up);
    if (tpp > RESAMPLE_MAX_TPP)
        resample_fail("n_taps", "allows at most 256 taps per output, ceil(n_taps / up) <= 256", std::to_string(n_taps) + " at up " + std::to_string(up));
    if (n_samples < 1 || n_samples >= RESAMPLE_MAX_ELEMS) resample_fail("n_samples", "must lie in 1..2^36 - 1", std::to_string(n_samples));
    ResamplePlan p;
    p.up = up; p.down = down; p.n_taps = n_taps; p.half = (n_taps - 1) / 2; p.tpp = tpp; p.n_samples = n_samples;
    p.n_out = cdiv64(n_samples * up, down);
    // the widest tile whose span, (tile - 1) down / up + 1 + tpp at most, fits the LDS budget; whole waves where it can
    int64_t tile = ((int64_t)(RESAMPLE_LDS_FLOATS - tpp - 2) * up) / down;
    tile = std::max<int64_t>(1, std::min<int64_t>(tile, RESAMPLE_MAX_TILE));
    if (tile >= 64) tile -= tile % 64;
    p.tile = (int)tile;
    p.n_tiles = cdiv64(p.n_out, p.tile);
    // LDS of a workgroup: the widest span of a tile, then the table where both stay within 64 KiB (rows at an odd stride)
    p.span_floats = (int)(((int64_t)(p.tile - 1) * down / up + tpp + 1 + 3) / 4 * 4);
    p.tab_in_lds = up > 1 && ((int64_t)p.span_floats + (int64_t)up * (tpp | 1)) * 4 <= RESAMPLE_LDS_BYTES;
    p.tab_stride = p.tab_in_lds ? (tpp | 1) : tpp;
    return p;
}

ResampleSpan resample_tile_span(const ResamplePlan& p, int64_t tile_index) {
    if (tile_index < 0 || tile_index >= p.n_tiles)
        resample_fail("tile_index", "must lie in 0..n_tiles - 1", std::to_string(tile_index));
    ResampleSpan s;
    s.out_first = tile_index * p.tile;
    s.out_count = (int)std::min<int64_t>(p.tile, p.n_out - s.out_first);
    const int64_t pos0 = s.out_first * p.down + p.half;
    s.in_first = pos0 / p.up - p.tpp + 1;
    s.in_count = (int)((pos0 + (int64_t)(s.out_count - 1) * p.down) / p.up - s.in_first + 1);
    return s;
}

void resample_check_rows(const ResamplePlan& p, int64_t n_clips) {
    if (n_clips < 0) resample_fail("n_clips", "must be >= 0", std::to_string(n_clips));
    if (n_clips > 0 && n_clips > (RESAMPLE_MAX_ELEMS - 1) / std::max(p.n_samples, p.n_out))
        resample_fail("n_clips", "times max(n_samples, n_out) must stay below 2^36", std::to_string(n_clips));
}

std::vector<float> resample_polyphase_table(const ResamplePlan& p, const float* taps) {
    std::vector<float> tab((size_t)p.up * p.tab_stride, 0.f);
    for (int ph = 0; ph < p.up; ++ph)
        for (int j = 0; j < p.tpp; ++j) {
            const int64_t k = ph + (int64_t)(p.tpp - 1 - j) * p.up;
            if (k < p.n_taps) tab[(size_t)ph * p.tab_stride + j] = taps[k];
        }
    return tab;
}

// where a lane's table row comes from
enum { TAB_GLOBAL = 0,     // device memory, one row per lane: any table the domain allows (up to 1 MB)
       TAB_ONE_PHASE = 1,  // up = 1: the one row is wave-uniform
       TAB_LDS = 2 };      // copied into LDS once per workgroup, rows at an odd stride: every table that fits beside the span

// work item w = row * n_tiles + tile index; the grid strides over them.  LDS: the span (span_floats), then the table (TAB_LDS)
template <int TAB>
__global__ __launch_bounds__(256) void resample_kernel(const float* __restrict__ x, float* __restrict__ y, const float* __restrict__ tab,
                                                       int64_t n_samples, int64_t n_out, int64_t n_tiles, int64_t n_work, int tile,
                                                       int up, int down, int half, int tpp, int tab_stride, int span_floats) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    float* __restrict__ span = lds;
    const int tid = (int)threadIdx.x;
    if (TAB == TAB_LDS) {
        float* __restrict__ ltab = lds + span_floats;
        for (int e = tid; e < up * tab_stride; e += 256) ltab[e] = tab[e];     // visible after the first barrier below
    }
    const float* __restrict__ rows = TAB == TAB_LDS ? lds + span_floats : tab;
    for (int64_t w = blockIdx.x; w < n_work; w += gridDim.x) {
        // 64-bit, once per workgroup: the tile's first output, its position and its first input index
        const int64_t row = w / n_tiles, out_first = (w - row * n_tiles) * tile;
        const int64_t left = n_out - out_first;
        const int count = left < (int64_t)tile ? (int)left : tile;
        const int64_t pos0 = out_first * down + half;
        const int64_t q0 = pos0 / up;
        const int r0 = (int)(pos0 - q0 * up);
        const int64_t in_first = q0 - tpp + 1;
        const int in_count = (r0 + (count - 1) * down) / up + tpp;        // <= span_floats by the host's choice of tile
        const float* __restrict__ xr = x + row * n_samples;
        for (int s = tid; s < in_count && s < span_floats; s += 256) {
            const int64_t i = in_first + s;
            span[s] = (i >= 0 && i < n_samples) ? xr[i] : 0.f;
        }
        __syncthreads();
        for (int t = tid; t < count; t += 256) {
            const int a = r0 + t * down, q = a / up;                     // < 2^20: 32-bit inside the tile
            const float* __restrict__ trow = TAB == TAB_ONE_PHASE ? rows : rows + (a - q * up) * tab_stride;
            const float* __restrict__ xs = span + q;
            float acc = 0.0f;
            int j = 0;
            for (; j + 8 <= tpp; j += 8) {                               // eight loads of each in flight, the sum still in order
                float xv[8], tv[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) { xv[u] = xs[j + u]; tv[u] = trow[j + u]; }
#pragma unroll
                for (int u = 0; u < 8; ++u) acc = fmaf(xv[u], tv[u], acc);
            }
            for (; j < tpp; ++j) acc = fmaf(xs[j], trow[j], acc);
            y[row * n_out + out_first + t] = acc;
        }
        __syncthreads();
    }
}

void launch_resample(const float* x, int64_t n_clips, const ResamplePlan& p, const float* tab_dev, float* y, int compute_units, hipStream_t s) {
    const int64_t n_work = n_clips * p.n_tiles;
    if (n_work < 1) return;
    CMOOP_REQUIRE((int64_t)(p.tile - 1) * p.down / p.up + p.tpp + 1 <= p.span_floats && p.span_floats <= RESAMPLE_LDS_FLOATS,
                  "resample: the tile's span exceeds the LDS budget");
    const size_t lds_bytes = ((size_t)p.span_floats + (p.tab_in_lds ? (size_t)p.up * p.tab_stride : 0)) * sizeof(float);
    CMOOP_REQUIRE(lds_bytes <= (size_t)RESAMPLE_LDS_BYTES, "resample: span and table exceed the workgroup's LDS");
    // TAB_LDS workgroups are persistent, as many as stay resident: each copies the table once and strides over the tiles
    const int64_t resident = (int64_t)std::max(1, compute_units) * std::min<int64_t>(8, RESAMPLE_CU_LDS_BYTES / lds_bytes);
    const unsigned grid = (unsigned)std::min<int64_t>(n_work, p.tab_in_lds ? resident : RESAMPLE_MAX_GRID);
    auto* kernel = p.up == 1 ? resample_kernel<TAB_ONE_PHASE> : p.tab_in_lds ? resample_kernel<TAB_LDS> : resample_kernel<TAB_GLOBAL>;
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), lds_bytes, s, x, y, tab_dev, p.n_samples, p.n_out, p.n_tiles, n_work, p.tile, p.up, p.down,
                       p.half, p.tpp, p.tab_stride, p.span_floats);
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
