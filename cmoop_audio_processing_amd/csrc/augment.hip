// What assembles an input batch (augment.py, the input half of loss.py's mixup, deploy.py's StreamScorer): the
// sliding-window gather of the stream scorer, train-time augmentation and the mixup blend.  HBM-bound copies with the
// draws of a batch row made once per work item.
#include "kernels.h"
#include <algorithm>
#include <cmath>

namespace cmoop {

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
// Mixup (kernels.h: semantics): the blend of two batch rows.  The targets that go with it are loss.hip's.
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

}  // namespace cmoop
