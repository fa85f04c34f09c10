// The element arithmetic of the fake quantisers (quant.hip): ONE statement of the scale and of the code / dequantised value,
// shared by the per-channel weight quantiser and the per-tensor activation quantiser (include/cmoop.h fixes the semantics at
// cmoop_quant and cmoop_actquant).  fp contraction is off where two operations meet.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace cmoop {

constexpr uint32_t QUANT_ABS_MASK = 0x7FFFFFFFu, QUANT_CANONICAL_NAN = 0x7FC00000u;

// s = a / qmax, one correctly rounded fp32 division; a NaN is stored as the canonical quiet NaN
__device__ __forceinline__ float quant_scale(uint32_t abits, float qmaxf) {
    const float s = __uint_as_float(abits) / qmaxf;
    return s == s ? s : __uint_as_float(QUANT_CANONICAL_NAN);
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
    wq = x == x ? x : __uint_as_float(QUANT_CANONICAL_NAN);
}

// four codes as one word, code 0 in the lowest byte: what a lane that owns four consecutive channels stores
__device__ __forceinline__ uint32_t quant_pack4(const int q[4]) {
    return ((uint32_t)q[0] & 0xFFu) | (((uint32_t)q[1] & 0xFFu) << 8) | (((uint32_t)q[2] & 0xFFu) << 16) | (((uint32_t)q[3] & 0xFFu) << 24);
}

}  // namespace cmoop
