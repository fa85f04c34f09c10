// Per-channel reductions over [M][C] and BatchNorm (train / eval / backward), with the fused BatchNorm-apply + max-pool
// pass and its backward twins.  colreduce_kernel<Op> is instantiated with StatsOp, BnBwdOp and BnBwdPooledOp, so the
// template and the three ops share this translation unit.  HBM-bound: float4 along the channel axis of NHWC tensors;
// every cross-thread sum has a fixed order.
#include "kernels.h"
#include <algorithm>

namespace cmoop {

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

}  // namespace cmoop
