// Magnitude pruning of the kernel tensors of a parameter arena (pruning in training; include/cmoop.h fixes the semantics at
// cmoop_prune): per tensor the k-th smallest key, key = bits(w) & 0x7FFFFFFF as uint32, is found EXACTLY by a radix select
// over the 31 key bits (digits of 11 / 10 / 10 bits, most significant first), then every element whose key is not above it
// becomes +0.0f.  Integer compares and integer atomics only, so the result does not depend on any order of execution.
//
// One call is FOUR launches over the same grid (a tensor's workgroups are found by binary search of block0 in the device
// table, PRUNE_BLOCK_ELEMS elements per workgroup, 16-byte loads between a scalar head and tail):
//   hist<1>  counts the top digit of every key of a tensor with k > 0 (one LDS histogram per wave64, LDS integer atomics,
//            flushed with global integer atomics into hist1 of the tensor); clears the tensor's hist3
//   hist<2>  every workgroup redoes the pick of the top digit from hist1 (the bucket the k-th key lies in and its rank
//            inside the bucket), then counts the middle digit of the keys of that bucket into hist2
//   hist<3>  redoes both picks, counts the low digit of the keys with the chosen 21-bit prefix into hist3; the tensor's
//            first workgroup records (prefix, rank) in the tensor's state words
//   apply    picks the low digit from hist3: the threshold t is complete.  Writes every element of every tensor (k == 0: a
//            copy), the optional zero count of the tensor (keys below the bucket + keys in it, from the histogram), and
//            clears hist1 and hist2 again
// so hist1 / hist2 are all zero between calls (PruneWorkspace: zeroed once when it is made) and no launch only clears.
// When every k is 0 the three select launches are skipped.  Memory-bound: no MFMA, no float atomics, 32-bit indices.
#include "kernels.h"

#include <algorithm>
#include <cmath>

namespace cmoop {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t ABS_MASK = 0x7FFFFFFFu;
constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int BINS1 = PRUNE_BINS_TOP, BINS23 = PRUNE_BINS_LOW;   // 2048, 1024
constexpr int SHIFT1 = 20, SHIFT2 = 10;

struct Block {
    PruneRow t;
    int tensor, b, k;
};

// the tensor of this workgroup (the last row whose block0 is not past blockIdx.x: the same in every lane) and its k
__device__ __forceinline__ Block find_block(const PruneRow* __restrict__ rows, int count, double s) {
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= rows[mid].block0) lo = mid;
        else hi = mid - 1;
    }
    Block blk;
    blk.t = rows[lo];
    blk.tensor = lo;
    blk.b = (int)blockIdx.x - blk.t.block0;
    blk.k = blk.t.k >= 0 ? blk.t.k : (int)floor(s * (double)blk.t.len);   // one IEEE double product, as prune_row_k on the host
    return blk;
}

// The bucket of a histogram of `bins` counters the rank-th smallest key (1-indexed) lies in, and its rank inside that bucket.
// All THREADS threads call it; scan is THREADS + 2 words of LDS.  rank <= the histogram's total by construction; a
// histogram that does not reach it (never the case for one this file filled) yields the last bucket
template <int BINS>
__device__ __forceinline__ void pick_digit(const uint32_t* __restrict__ hist, uint32_t rank, uint32_t* scan, uint32_t& digit,
                                           uint32_t& rank_in) {
    constexpr int bins = BINS, per = BINS / THREADS;          // 8 or 4 consecutive buckets per thread
    const int tid = (int)threadIdx.x;
    uint32_t c[per];
    uint32_t sum = 0;
#pragma unroll
    for (int j = 0; j < per; ++j) { c[j] = hist[tid * per + j]; sum += c[j]; }
    __syncthreads();                       // the previous use of scan is over
    scan[tid] = sum;
    if (tid == 0) { scan[THREADS] = (uint32_t)(bins - 1); scan[THREADS + 1] = 1u; }
    __syncthreads();
    for (int off = 1; off < THREADS; off <<= 1) {   // inclusive scan
        const uint32_t add = tid >= off ? scan[tid - off] : 0u;
        __syncthreads();
        scan[tid] += add;
        __syncthreads();
    }
    const uint32_t incl = scan[tid], excl = incl - sum;
    if (excl < rank && rank <= incl) {     // exactly one thread
        uint32_t run = excl;
        bool found = false;
#pragma unroll
        for (int j = 0; j < per; ++j) {
            if (!found && rank <= run + c[j]) { scan[THREADS] = (uint32_t)(tid * per + j); scan[THREADS + 1] = rank - run; found = true; }
            run += c[j];
        }
    }
    __syncthreads();
    digit = scan[THREADS];
    rank_in = scan[THREADS + 1];
}

// f(i) for every arena index i of [c0, c1) by scalar accesses, or f4(i) for every 16-byte aligned group of four inside it
// and f(i) for the head and the tail around them.  align_off: the element phase of index 0 against 16 bytes
template <class F1, class F4>
__device__ __forceinline__ void for_chunk(int c0, int c1, int align_off, bool vec, F1 f, F4 f4) {
    const int tid = (int)threadIdx.x;
    if (!vec) {
        for (int i = c0 + tid; i < c1; i += THREADS) f(i);
        return;
    }
    const int head = min((4 - ((c0 + align_off) & 3)) & 3, c1 - c0);
    const int v0 = c0 + head, nvec = (c1 - v0) >> 2, tail0 = v0 + (nvec << 2);
    if (tid < head) f(c0 + tid);
    for (int v = tid; v < nvec; v += THREADS) f4(v0 + (v << 2));
    if (tid < c1 - tail0) f(tail0 + tid);
}

template <int PASS>
__global__ __launch_bounds__(THREADS) void prune_hist_kernel(const float* __restrict__ w, const PruneRow* __restrict__ rows,
                                                             int count, double s, uint32_t* __restrict__ hist1,
                                                             uint32_t* __restrict__ hist2, uint32_t* __restrict__ hist3,
                                                             uint32_t* __restrict__ state) {
    constexpr int BINS = PASS == 1 ? BINS1 : BINS23;
    __shared__ uint32_t lh[WAVES * BINS + THREADS + 2];
    uint32_t* scan = lh + WAVES * BINS;
    const Block blk = find_block(rows, count, s);
    if (blk.k == 0) return;                // a copy: nothing to select (uniform over the workgroup)
    const int tid = (int)threadIdx.x;
    uint32_t* h1 = hist1 + (size_t)blk.tensor * BINS1;
    uint32_t* h2 = hist2 + (size_t)blk.tensor * BINS23;
    uint32_t* h3 = hist3 + (size_t)blk.tensor * BINS23;

    uint32_t prefix = 0, rank = (uint32_t)blk.k;
    if (PASS == 1) {
        if (blk.b == 0)
            for (int i = tid; i < BINS23; i += THREADS) h3[i] = 0u;    // nothing else touches hist3 in this launch
    } else {
        uint32_t d;
        pick_digit<BINS1>(h1, rank, scan, d, rank);
        prefix = d;
        if (PASS == 3) {
            pick_digit<BINS23>(h2, rank, scan, d, rank);
            prefix = (prefix << 10) | d;
            if (blk.b == 0 && tid == 0) { state[2 * blk.tensor] = prefix; state[2 * blk.tensor + 1] = rank; }
        }
    }
    for (int i = tid; i < WAVES * BINS; i += THREADS) lh[i] = 0u;
    __syncthreads();
    uint32_t* mine = lh + (tid >> 6) * BINS;           // this wave's histogram
    auto count_key = [&](uint32_t bits) {
        const uint32_t key = bits & ABS_MASK;
        if (PASS == 1) atomicAdd(&mine[key >> SHIFT1], 1u);
        else if (PASS == 2) { if ((key >> SHIFT1) == prefix) atomicAdd(&mine[(key >> SHIFT2) & (BINS23 - 1)], 1u); }
        else { if ((key >> SHIFT2) == prefix) atomicAdd(&mine[key & (BINS23 - 1)], 1u); }
    };
    const uint32_t* wb = reinterpret_cast<const uint32_t*>(w);
    const int c0 = blk.t.off + blk.b * PRUNE_BLOCK_ELEMS;
    const int c1 = min(c0 + PRUNE_BLOCK_ELEMS, blk.t.off + blk.t.len);
    const int align_off = (int)((reinterpret_cast<uintptr_t>(w) >> 2) & 3);
    const bool vec = (reinterpret_cast<uintptr_t>(w) & 3) == 0;
    for_chunk(c0, c1, align_off, vec, [&](int i) { count_key(wb[i]); },
              [&](int i) {
                  const u32x4 v = *reinterpret_cast<const u32x4*>(wb + i);
                  count_key(v.x); count_key(v.y); count_key(v.z); count_key(v.w);
              });
    __syncthreads();
    uint32_t* out = PASS == 1 ? h1 : PASS == 2 ? h2 : h3;
    for (int i = tid; i < BINS; i += THREADS) {
        uint32_t c = 0;
        for (int wv = 0; wv < WAVES; ++wv) c += lh[wv * BINS + i];
        if (c) atomicAdd(&out[i], c);
    }
}

__global__ __launch_bounds__(THREADS) void prune_apply_kernel(const float* __restrict__ w, float* __restrict__ out,
                                                              uint32_t* __restrict__ zeros, const PruneRow* __restrict__ rows,
                                                              int count, double s, uint32_t* __restrict__ hist1,
                                                              uint32_t* __restrict__ hist2, const uint32_t* __restrict__ hist3,
                                                              const uint32_t* __restrict__ state) {
    __shared__ uint32_t scan[THREADS + 2];
    const Block blk = find_block(rows, count, s);
    const int tid = (int)threadIdx.x;
    const uint32_t* wb = reinterpret_cast<const uint32_t*>(w);
    uint32_t* ob = reinterpret_cast<uint32_t*>(out);
    const int c0 = blk.t.off + blk.b * PRUNE_BLOCK_ELEMS;
    const int c1 = min(c0 + PRUNE_BLOCK_ELEMS, blk.t.off + blk.t.len);
    const int align_off = (int)((reinterpret_cast<uintptr_t>(w) >> 2) & 3);
    const bool vec = (reinterpret_cast<uintptr_t>(w) & 3) == 0 && (reinterpret_cast<uintptr_t>(w) & 15) == (reinterpret_cast<uintptr_t>(out) & 15);
    if (blk.k == 0) {                      // a copy, bit for bit
        if (blk.b == 0 && tid == 0 && zeros) zeros[blk.tensor] = 0u;
        for_chunk(c0, c1, align_off, vec, [&](int i) { ob[i] = wb[i]; },
                  [&](int i) { *reinterpret_cast<u32x4*>(ob + i) = *reinterpret_cast<const u32x4*>(wb + i); });
        return;
    }
    const uint32_t* h3 = hist3 + (size_t)blk.tensor * BINS23;
    const uint32_t prefix = state[2 * blk.tensor], rank2 = state[2 * blk.tensor + 1];
    uint32_t d, rank3;
    pick_digit<BINS23>(h3, rank2, scan, d, rank3);
    const uint32_t t = (prefix << 10) | d;             // the k-th smallest key
    if (blk.b == 0) {
        // keys below t: k - rank3 (rank3 is t's 1-indexed rank among the keys equal to it, from the k-th on); keys equal: h3[d]
        if (tid == 0 && zeros) zeros[blk.tensor] = (uint32_t)blk.k - rank3 + h3[d];
        uint32_t* h1 = hist1 + (size_t)blk.tensor * BINS1;
        uint32_t* h2 = hist2 + (size_t)blk.tensor * BINS23;
        for (int i = tid; i < BINS1; i += THREADS) h1[i] = 0u;      // nothing reads hist1 / hist2 in this launch
        for (int i = tid; i < BINS23; i += THREADS) h2[i] = 0u;
    }
    auto thr = [&](uint32_t bits) { return (bits & ABS_MASK) <= t ? 0u : bits; };
    for_chunk(c0, c1, align_off, vec, [&](int i) { ob[i] = thr(wb[i]); },
              [&](int i) {
                  const u32x4 v = *reinterpret_cast<const u32x4*>(wb + i);
                  const u32x4 r = {thr(v.x), thr(v.y), thr(v.z), thr(v.w)};
                  *reinterpret_cast<u32x4*>(ob + i) = r;
              });
}

}  // namespace

void prune_check(const PruneCfg& c) {
    CMOOP_REQUIRE(c.sparsity >= 0.0 && c.sparsity < 1.0, "prune: sparsity must be 0 (off) or in (0, 1)");   // a NaN fails too
    CMOOP_REQUIRE(c.begin_step >= 0, "prune: begin_step must be >= 0");
    CMOOP_REQUIRE(c.end_step >= 0, "prune: end_step must be >= 0");
    CMOOP_REQUIRE(c.objective == 0 || c.objective == 1, "prune: objective must be 0 or 1");
    CMOOP_REQUIRE(c.skip_small == 0 || c.skip_small == 1, "prune: skip_small must be 0 or 1");
}

double prune_sparsity_at(const PruneCfg& c, int64_t it) {
    if (it < (int64_t)c.begin_step) return 0.0;
    if (it >= (int64_t)c.end_step || c.end_step <= c.begin_step) return c.sparsity;
    const double u = (double)(it - (int64_t)c.begin_step) / (double)((int64_t)c.end_step - (int64_t)c.begin_step);
    const double r = 1.0 - u;
    const double r2 = r * r;
    const double r3 = r2 * r;
    const double f = 1.0 - r3;
    return c.sparsity * f;
}

int32_t prune_row_k(const PruneRow& r, double s) {
    return r.k >= 0 ? r.k : (int32_t)std::floor(s * (double)r.len);
}

void prune_table_finalize(PruneTable& tab, int64_t n) {
    CMOOP_REQUIRE(n >= 0 && n <= PRUNE_MAX_ARENA, "prune: the arena must stay below 2^31 elements (PRUNE_MAX_ARENA: 32-bit index math)");
    CMOOP_REQUIRE((int64_t)tab.rows.size() <= PRUNE_MAX_ROWS, "prune: too many kernel tensors in one table (PRUNE_MAX_ROWS)");
    int64_t blocks = 0, elems = 0, end = 0;
    for (PruneRow& r : tab.rows) {
        CMOOP_REQUIRE(r.off >= 0 && r.len >= 1, "prune: a table row needs off >= 0 and len >= 1");
        CMOOP_REQUIRE(r.k >= -1 && r.k <= r.len, "prune: a table row needs k in [-1, len] (-1: floor(s len))");
        CMOOP_REQUIRE((int64_t)r.off + r.len <= n, "prune: a table row reaches past the arena");
        CMOOP_REQUIRE(r.off >= end, "prune: the table rows must be in arena order and must not overlap");
        end = (int64_t)r.off + r.len;
        r.block0 = (int32_t)blocks;
        blocks += cdiv64(r.len, PRUNE_BLOCK_ELEMS);
        elems += r.len;
    }
    CMOOP_REQUIRE(blocks < ((int64_t)1 << 30), "prune: grid too large");
    tab.blocks = (int32_t)blocks;
    tab.kernel_elems = elems;
}

int64_t prune_size_bytes(const PruneTable& tab, int64_t n_params, double sparsity, int bits, int64_t quant_channels) {
    CMOOP_REQUIRE(sparsity >= 0.0 && sparsity < 1.0, "prune: sparsity must be in [0, 1)");
    CMOOP_REQUIRE(bits == 0 || (bits >= 2 && bits <= 8), "prune: bits must be 0 (fp32 values) or in [2, 8]");
    int64_t bytes = 0;
    for (const PruneRow& r : tab.rows) {
        const int64_t k = prune_row_k(r, sparsity), kept = (int64_t)r.len - k;
        if (k > 0) bytes += ((int64_t)r.len + 7) / 8;                  // the mask, one bit per element
        bytes += bits ? (kept * bits + 7) / 8 : 4 * kept;              // the values that remain (all of them when k == 0)
    }
    return bytes + (bits ? 4 * quant_channels : 0) + 4 * (n_params - tab.kernel_elems);
}

size_t prune_workspace_words(int rows) {
    return (size_t)std::max(rows, 1) * (PRUNE_BINS_TOP + 2 * PRUNE_BINS_LOW + 2);
}

void prune_workspace_init(PruneWorkspace& ws, uint32_t* words_dev, int rows, hipStream_t s) {
    CMOOP_REQUIRE(words_dev != nullptr && rows >= 0 && rows <= PRUNE_MAX_ROWS, "prune: workspace");
    const size_t r = (size_t)std::max(rows, 1);
    ws.hist1 = words_dev;
    ws.hist2 = ws.hist1 + r * PRUNE_BINS_TOP;
    ws.hist3 = ws.hist2 + r * PRUNE_BINS_LOW;
    ws.state = ws.hist3 + r * PRUNE_BINS_LOW;
    ws.rows = rows;
    CMOOP_HIP(hipMemsetAsync(words_dev, 0, prune_workspace_words(rows) * sizeof(uint32_t), s));
}

int launch_prune_weights(const float* w, float* out, uint32_t* zeros, const PruneTable& tab, const PruneRow* rows_dev,
                         const PruneWorkspace& ws, double s, hipStream_t stream) {
    CMOOP_REQUIRE(s >= 0.0 && s < 1.0, "prune: the sparsity of a launch must be in [0, 1)");
    if (tab.blocks == 0) return 0;
    CMOOP_REQUIRE(w && out && rows_dev, "prune_weights: NULL buffer");
    CMOOP_REQUIRE(ws.hist1 && ws.rows >= (int)tab.rows.size(), "prune_weights: the workspace is smaller than the table");
    bool any = false;
    for (const PruneRow& r : tab.rows) any = any || prune_row_k(r, s) > 0;
    const dim3 grid((unsigned)tab.blocks), block(THREADS);
    const int count = (int)tab.rows.size();
    int launches = 0;
    if (any) {    // else: every tensor is a copy, and the bytes are those of the full sequence
        hipLaunchKernelGGL(prune_hist_kernel<1>, grid, block, 0, stream, w, rows_dev, count, s, ws.hist1, ws.hist2, ws.hist3, ws.state);
        hipLaunchKernelGGL(prune_hist_kernel<2>, grid, block, 0, stream, w, rows_dev, count, s, ws.hist1, ws.hist2, ws.hist3, ws.state);
        hipLaunchKernelGGL(prune_hist_kernel<3>, grid, block, 0, stream, w, rows_dev, count, s, ws.hist1, ws.hist2, ws.hist3, ws.state);
        launches += 3;
    }
    hipLaunchKernelGGL(prune_apply_kernel, grid, block, 0, stream, w, out, zeros, rows_dev, count, s, ws.hist1, ws.hist2, ws.hist3,
                       ws.state);
    CMOOP_HIP(hipGetLastError());
    return launches + 1;
}

}  // namespace cmoop
