// Shared host/device helpers for libcmoop_hip.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <stdexcept>
#include <string>

namespace cmoop {

struct Error : std::runtime_error {
    using std::runtime_error::runtime_error;
};

#define CMOOP_HIP(expr)                                                                    \
    do {                                                                                   \
        hipError_t e__ = (expr);                                                           \
        if (e__ != hipSuccess)                                                             \
            throw ::cmoop::Error(std::string(#expr) + ": " + hipGetErrorString(e__) +      \
                                 " (" __FILE__ ":" + std::to_string(__LINE__) + ")");      \
    } while (0)

#define CMOOP_REQUIRE(cond, msg)                                                           \
    do {                                                                                   \
        if (!(cond)) throw ::cmoop::Error(std::string("cmoop: ") + (msg));                 \
    } while (0)

// ---------------------------------------------------------------------------
// Counter-based RNG, bit-exact twin of oracle/rng.py (murmur3 fmix32 chain).
// Streams: 0x1000+tensor (init), 0x2000+fc layer (dropout), 0x3000 (shuffle),
// 0x4000 (train-time augmentation: row draws; 0x4001 / 0x4002 the two noise words), 0x5000 (mixup: gate / partner / lam).
// ---------------------------------------------------------------------------
constexpr uint32_t STREAM_INIT = 0x1000u, STREAM_DROPOUT = 0x2000u, STREAM_SHUFFLE = 0x3000u, STREAM_AUGMENT = 0x4000u,
                   STREAM_MIXUP = 0x5000u;

__host__ __device__ __forceinline__ uint32_t fmix32(uint32_t h) {
    h ^= h >> 16; h *= 0x85EBCA6Bu; h ^= h >> 13; h *= 0xC2B2AE35u; h ^= h >> 16;
    return h;
}
__host__ __device__ __forceinline__ uint32_t rng_prefix(uint32_t seed, uint32_t stream, uint32_t ctr) {
    return fmix32(fmix32(fmix32(seed + 0x9E3779B9u) ^ stream) ^ ctr);
}
__host__ __device__ __forceinline__ uint32_t rng_u32(uint32_t seed, uint32_t stream, uint32_t ctr, uint32_t idx) {
    return fmix32(rng_prefix(seed, stream, ctr) ^ idx);
}

static inline int ilog2_exact(int v) {
    int s = 0;
    while ((1 << s) < v) ++s;
    return ((1 << s) == v) ? s : -1;
}
static inline int cdiv(int a, int b) { return (a + b - 1) / b; }
static inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

// ---------------------------------------------------------------------------
// What several kernel files share ("File map of csrc/").
// ---------------------------------------------------------------------------
// 16 / 8 bytes of floats: one global or LDS access per lane, one MFMA accumulator
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x2 __attribute__((ext_vector_type(2)));

// row of the resident tensor a batch position maps to: idx[pos] (the epoch permutation) or pos itself; with n_rows > 0
// the result is clamped into [0, n_rows): a corrupt index can then mis-train but never fault
__device__ __forceinline__ int64_t gather_row(const int32_t* __restrict__ idx, int64_t pos, int64_t n_rows) {
    int64_t src = idx ? (int64_t)idx[pos] : pos;
    if (n_rows > 0) src = src < 0 ? 0 : (src >= n_rows ? n_rows - 1 : src);
    return src;
}

// grid of a grid-stride elementwise launch over n items, 256 threads per workgroup
static inline unsigned ew_grid(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv64(n, 256), 8192)); }

// Granlund-Montgomery division by an invariant: q = (umulhi(n, magic) + n) >> shift, exact for n < 2^31.  The host half;
// each user keeps its own one-line device half beside its kernels
static inline void fastdiv_init(int d, uint32_t* magic, uint32_t* shift) {
    uint32_t s = 0;
    while ((1u << s) < (uint32_t)d) ++s;
    *shift = s;
    *magic = (uint32_t)((((uint64_t)1 << 32) * (((uint64_t)1 << s) - (uint64_t)d)) / (uint64_t)d + 1);
}

}  // namespace cmoop
