// Fake quantisation of the kernel tensors of a parameter arena (quantisation-aware training; include/cmoop.h fixes the
// semantics at cmoop_quant): symmetric, per output channel, weights only, 2 .. 8 bits.  ONE launch for a whole arena,
// driven by a device table of QuantRow (kernels.h).  Memory-bound VALU kernel: no MFMA, no LDS, no atomics, 32-bit indices.
//
// Row tensor ([C_out][kh][kw][C_in], [out][in]; len 9 .. 12800): one wave64 per channel, 4 channels per workgroup.  Pass 1
// takes the integer maximum of the magnitudes' bit patterns (16-byte loads when the row start and len allow, 4-byte loads
// otherwise) and reduces it across the lanes; pass 2 reads the row again (at most 50 KiB, still in L2) and writes wq and
// the codes.  Strided tensor (depthwise [kh][kw][C]): one lane per channel walks the kh kw taps, consecutive lanes on
// consecutive addresses.
#include "kernels.h"

#include <algorithm>

namespace cmoop {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t ABS_MASK = 0x7FFFFFFFu, CANONICAL_NAN = 0x7FC00000u;

// s = a / qmax, one correctly rounded fp32 division; a NaN is stored as the canonical quiet NaN
__device__ __forceinline__ float quant_scale(uint32_t abits, float qmaxf) {
    const float s = __uint_as_float(abits) / qmaxf;
    return s == s ? s : __uint_as_float(CANONICAL_NAN);
}

// the code and the dequantised value of w under scale s; live: s > 0
__device__ __forceinline__ void quant_element(float w, float s, bool live, float qmaxf, int& q, float& wq) {
#pragma clang fp contract(off)
    float r = 0.f;
    if (live) {
        r = rintf(w / s);                          // one fp32 division, then round half to even
        if (!(r == r)) r = 0.f;                    // inf / inf
        r = fminf(fmaxf(r, -qmaxf), qmaxf);
    }
    q = (int)r;
    const float x = (float)q * s;                  // one fp32 product; 0 * s = +0 for every s > 0
    wq = x == x ? x : __uint_as_float(CANONICAL_NAN);
}

__device__ __forceinline__ uint32_t pack_codes(int q0, int q1, int q2, int q3) {
    return ((uint32_t)q0 & 0xFFu) | (((uint32_t)q1 & 0xFFu) << 8) | (((uint32_t)q2 & 0xFFu) << 16) | (((uint32_t)q3 & 0xFFu) << 24);
}

__global__ __launch_bounds__(256) void quantize_weights_kernel(const float* __restrict__ w, float* __restrict__ wq,
                                                               int8_t* __restrict__ codes, float* __restrict__ scales,
                                                               const QuantRow* __restrict__ rows, int count, float qmaxf) {
    // the tensor of this workgroup: the last row whose block0 is not past blockIdx.x (the same in every lane)
    int lo = 0, hi = count - 1;
    while (lo < hi) {
        const int mid = (lo + hi + 1) >> 1;
        if ((int)blockIdx.x >= rows[mid].block0) lo = mid;
        else hi = mid - 1;
    }
    const QuantRow t = rows[lo];
    const int b = (int)blockIdx.x - t.block0;

    if (t.elem_stride != 1) {   // strided tensor: a lane per channel
        const int c = b * QUANT_LANE_CHANNELS + (int)threadIdx.x;
        if (c >= t.channels) return;
        const int base = t.off + c * t.chan_stride;
        uint32_t m = 0;
        for (int k = 0; k < t.len; ++k) m = max(m, __float_as_uint(w[base + k * t.elem_stride]) & ABS_MASK);
        const float s = quant_scale(m, qmaxf);
        const bool live = s > 0.f;
        if (scales) scales[t.scale_off + c] = s;
        for (int k = 0; k < t.len; ++k) {
            const int i = base + k * t.elem_stride;
            int q; float x;
            quant_element(w[i], s, live, qmaxf, q, x);
            wq[i] = x;
            if (codes) codes[i] = (int8_t)q;
        }
        return;
    }

    // row tensor: a wave per channel
    const int lane = (int)threadIdx.x & 63;
    const int c = b * QUANT_ROW_CHANNELS + ((int)threadIdx.x >> 6);
    if (c >= t.channels) return;
    const int base = t.off + c * t.chan_stride;
    const bool vec = (t.len % 4 == 0) && (reinterpret_cast<uintptr_t>(w + base) % 16 == 0) &&
                     (reinterpret_cast<uintptr_t>(wq + base) % 16 == 0) &&
                     (codes == nullptr || reinterpret_cast<uintptr_t>(codes + base) % 4 == 0);
    uint32_t m = 0;
    if (vec) {
        for (int i = lane * 4; i < t.len; i += 256) {
            const u32x4 v = *reinterpret_cast<const u32x4*>(w + base + i);
            m = max(max(m, v.x & ABS_MASK), max(v.y & ABS_MASK, max(v.z & ABS_MASK, v.w & ABS_MASK)));
        }
    } else {
        for (int i = lane; i < t.len; i += 64) m = max(m, __float_as_uint(w[base + i]) & ABS_MASK);
    }
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    const float s = quant_scale(m, qmaxf);
    const bool live = s > 0.f;
    if (lane == 0 && scales) scales[t.scale_off + c] = s;
    if (vec) {
        for (int i = lane * 4; i < t.len; i += 256) {
            const f32x4 v = *reinterpret_cast<const f32x4*>(w + base + i);
            int q0, q1, q2, q3;
            float x0, x1, x2, x3;
            quant_element(v.x, s, live, qmaxf, q0, x0);
            quant_element(v.y, s, live, qmaxf, q1, x1);
            quant_element(v.z, s, live, qmaxf, q2, x2);
            quant_element(v.w, s, live, qmaxf, q3, x3);
            const f32x4 x = {x0, x1, x2, x3};
            *reinterpret_cast<f32x4*>(wq + base + i) = x;
            if (codes) *reinterpret_cast<uint32_t*>(codes + base + i) = pack_codes(q0, q1, q2, q3);
        }
    } else {
        for (int i = lane; i < t.len; i += 64) {
            int q; float x;
            quant_element(w[base + i], s, live, qmaxf, q, x);
            wq[base + i] = x;
            if (codes) codes[base + i] = (int8_t)q;
        }
    }
}

}  // namespace

void quant_check(const QuantCfg& c) {
    CMOOP_REQUIRE(c.bits == 0 || (c.bits >= 2 && c.bits <= 8), "quant: bits must be 0 (off) or in [2, 8]");
    CMOOP_REQUIRE(c.objective == 0 || c.objective == 1, "quant: objective must be 0 or 1");
    CMOOP_REQUIRE(c.reserved[0] == 0 && c.reserved[1] == 0, "quant: reserved must be 0");
}

void quant_table_finalize(QuantTable& tab, int64_t n) {
    CMOOP_REQUIRE(n >= 0 && n <= QUANT_MAX_ARENA, "quant: the arena must stay below 2^31 elements (QUANT_MAX_ARENA: 32-bit index math)");
    CMOOP_REQUIRE((int64_t)tab.rows.size() <= QUANT_MAX_ROWS, "quant: too many kernel tensors in one table (QUANT_MAX_ROWS)");
    int64_t blocks = 0, channels = 0, elems = 0;
    for (QuantRow& r : tab.rows) {
        CMOOP_REQUIRE(r.off >= 0 && r.channels >= 1 && r.len >= 1 && r.chan_stride >= 1 && r.elem_stride >= 1,
                      "quant: a table row needs off >= 0 and channels, len, chan_stride, elem_stride >= 1");
        const int64_t last = (int64_t)r.off + (int64_t)(r.channels - 1) * r.chan_stride + (int64_t)(r.len - 1) * r.elem_stride;
        CMOOP_REQUIRE(last < n, "quant: a table row reaches past the arena");
        r.scale_off = (int32_t)channels;
        r.block0 = (int32_t)blocks;
        blocks += cdiv64(r.channels, r.elem_stride == 1 ? QUANT_ROW_CHANNELS : QUANT_LANE_CHANNELS);
        channels += r.channels;
        elems += (int64_t)r.channels * r.len;
        CMOOP_REQUIRE(blocks < ((int64_t)1 << 30) && channels <= QUANT_MAX_ARENA, "quant: grid too large");
    }
    tab.blocks = (int32_t)blocks;
    tab.total_channels = (int32_t)channels;
    tab.kernel_elems = elems;
}

int64_t quant_size_bytes(const QuantTable& tab, int64_t n_params, int bits) {
    CMOOP_REQUIRE(bits >= 2 && bits <= 8, "quant: bits must be in [2, 8]");
    int64_t bytes = 0;
    for (const QuantRow& r : tab.rows) bytes += ((int64_t)r.channels * r.len * bits + 7) / 8;
    return bytes + 4 * (int64_t)tab.total_channels + 4 * (n_params - tab.kernel_elems);
}

void launch_quantize_weights(const float* w, float* wq, int8_t* codes, float* scales, const QuantTable& tab, const QuantRow* rows_dev,
                             int bits, hipStream_t s) {
    CMOOP_REQUIRE(bits >= 2 && bits <= 8, "quant: bits must be in [2, 8]");
    if (tab.blocks == 0) return;
    CMOOP_REQUIRE(w && wq && rows_dev, "quantize_weights: NULL buffer");
    hipLaunchKernelGGL(quantize_weights_kernel, dim3((unsigned)tab.blocks), dim3(256), 0, s, w, wq, codes, scales, rows_dev,
                       (int)tab.rows.size(), (float)quant_qmax(bits));
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
