// The optimiser family (optim.py, ema.py): Keras-form Adam, the segment launch that also finishes the slab gradients,
// the finish + clip + AdamW path of the optimiser options with its schedules, and the weight EMA.  Every operation of
// an update is a separately rounded fp32 operation; the value twins (adam_update / adam_moments + adam_delta,
// adam_slab_block / grad_slab_block) stay twins: DESIGN.md, "Optimiser options".
#include "kernels.h"
#include <algorithm>
#include <cmath>

namespace cmoop {

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

}  // namespace cmoop
