// The operating-point read-out (opoint.py): score keys per class, the n^2 ROC counts, the per-class selection and the
// host summary.  Integer counts throughout: exact in any order.
#include "kernels.h"
#include <cmath>

namespace cmoop {

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
