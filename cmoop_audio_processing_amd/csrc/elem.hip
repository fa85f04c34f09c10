// The small HBM-bound kernels between the layers of the candidate-training path: max-pool forward and backward,
// residual add + ReLU, global average pooling forward and backward, the seeded glorot initialiser and constant fill,
// the device step counter, the epoch permutation and the confusion matrix.  Loads and stores are float4 along the
// channel axis of NHWC tensors (coalesced 16 B/lane); every cross-thread sum has a fixed order so a training run is
// bit-reproducible.  The other stages have files of their own ("File map of csrc/").
#include "kernels.h"
#include <algorithm>

namespace cmoop {

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

}  // namespace cmoop
