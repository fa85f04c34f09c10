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
#include "quant_math.h"

#include <algorithm>

namespace cmoop {
namespace {

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t ABS_MASK = QUANT_ABS_MASK;

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

// ---- activation fake quantisation: one tensor, one range ---------------------------------------------------------------
// Both kernels split x [n] the same way: `head` elements up to the first 16-byte boundary (0 .. 3, all of x when n is smaller),
// nv whole 16-byte groups, then the rest (0 .. 3).  Groups go through 16-byte accesses in a grid stride; the at most 6 edge
// elements through 4-byte ones, one per lane of the first lanes of the grid.
struct ActSpan { int head, nv, tail0; };
__device__ __forceinline__ ActSpan act_span(const float* x, int n) {
    ActSpan sp;
    sp.head = min(n, (int)((16u - (uint32_t)(reinterpret_cast<uintptr_t>(x) & 15u)) & 15u) >> 2);
    sp.nv = (n - sp.head) >> 2;
    sp.tail0 = sp.head + 4 * sp.nv;
    return sp;
}

// the maximum of m over the workgroup's 256 lanes, the same value in every lane (red: 4 words of LDS)
__device__ __forceinline__ uint32_t block_max_256(uint32_t m, uint32_t* red) {
    for (int off = 32; off >= 1; off >>= 1) m = max(m, (uint32_t)__shfl_xor((int)m, off, 64));
    if (((int)threadIdx.x & 63) == 0) red[(int)threadIdx.x >> 6] = m;
    __syncthreads();
    return max(max(red[0], red[1]), max(red[2], red[3]));
}

__global__ __launch_bounds__(256) void act_absmax_kernel(const float* __restrict__ x, int n, uint32_t* __restrict__ partials) {
    __shared__ uint32_t red[4];
    const ActSpan sp = act_span(x, n);
    const int gid = (int)(blockIdx.x * 256u + threadIdx.x), stride = (int)(gridDim.x * 256u);
    const u32x4* xv = reinterpret_cast<const u32x4*>(x + sp.head);
    uint32_t m = 0;
    for (int i = gid; i < sp.nv; i += stride) {
        const u32x4 v = xv[i];
        m = max(max(m, v.x & ABS_MASK), max(v.y & ABS_MASK, max(v.z & ABS_MASK, v.w & ABS_MASK)));
    }
    if (gid < sp.head) m = max(m, __float_as_uint(x[gid]) & ABS_MASK);
    if (gid < n - sp.tail0) m = max(m, __float_as_uint(x[sp.tail0 + gid]) & ABS_MASK);
    m = block_max_256(m, red);
    if (threadIdx.x == 0) partials[blockIdx.x] = m;
}

// the record after a train step whose tensor had the absmax bits `abits`
__device__ __forceinline__ void act_range_advance(ActRange* rec, uint32_t abits, float mu, float omu) {
#pragma clang fp contract(off)
    const float nan = __uint_as_float(QUANT_CANONICAL_NAN);
    float mb = __uint_as_float(abits);
    if (!(mb == mb)) mb = nan;
    const int count = rec->count;
    float r = mb;
    if (count != 0) {
        const float keep = mu * rec->r;            // three fp32 operations, each rounded on its own
        const float add = omu * mb;
        r = keep + add;
        if (!(r == r)) r = nan;
    }
    rec->m_b = mb;
    rec->r = r;
    rec->count = count == 0x7FFFFFFF ? count : count + 1;
    rec->reserved = 0;
}

// CODES (tracked mode only, integer inference): the int8 code of every element goes to codes [n] next to the fp32 value, four
// codes per store where the group's first code is 4-byte aligned.  !CODES is the kernel as it always was
template <bool TRACKED, bool CODES = false>
__global__ __launch_bounds__(256) void act_quant_apply_kernel(float* __restrict__ x, int n, const uint32_t* __restrict__ partials,
                                                              int nparts, ActRange* __restrict__ rec, float qmaxf, float mu, float omu,
                                                              int8_t* __restrict__ codes = nullptr) {
    __shared__ uint32_t red[4];
    uint32_t abits;
    if (TRACKED) {
        abits = __float_as_uint(rec->r);           // read only: no workgroup writes the record in this mode
    } else {
        uint32_t m = 0;                            // every workgroup folds all the partials: at most 4 per lane
        for (int i = (int)threadIdx.x; i < nparts; i += 256) m = max(m, partials[i]);
        abits = block_max_256(m, red);
        // no other lane of the grid reads the record in this mode
        if (blockIdx.x == 0 && threadIdx.x == 0) act_range_advance(rec, abits, mu, omu);
    }
    const float s = quant_scale(abits, qmaxf);
    const bool live = s > 0.f;
    const ActSpan sp = act_span(x, n);
    const int gid = (int)(blockIdx.x * 256u + threadIdx.x), stride = (int)(gridDim.x * 256u);
    f32x4* xv = reinterpret_cast<f32x4*>(x + sp.head);
    const bool packed = CODES && reinterpret_cast<uintptr_t>(codes + sp.head) % 4 == 0;
    for (int i = gid; i < sp.nv; i += stride) {
        const f32x4 v = xv[i];
        int q0, q1, q2, q3;
        float y0, y1, y2, y3;
        quant_element(v.x, s, live, qmaxf, q0, y0);
        quant_element(v.y, s, live, qmaxf, q1, y1);
        quant_element(v.z, s, live, qmaxf, q2, y2);
        quant_element(v.w, s, live, qmaxf, q3, y3);
        const f32x4 y = {y0, y1, y2, y3};
        xv[i] = y;
        if (CODES) {
            int8_t* c = codes + sp.head + 4 * i;
            if (packed) *reinterpret_cast<uint32_t*>(c) = pack_codes(q0, q1, q2, q3);
            else { c[0] = (int8_t)q0; c[1] = (int8_t)q1; c[2] = (int8_t)q2; c[3] = (int8_t)q3; }
        }
    }
    if (gid < sp.head) {
        int q; float y;
        quant_element(x[gid], s, live, qmaxf, q, y);
        x[gid] = y;
        if (CODES) codes[gid] = (int8_t)q;
    }
    if (gid < n - sp.tail0) {
        int q; float y;
        quant_element(x[sp.tail0 + gid], s, live, qmaxf, q, y);
        x[sp.tail0 + gid] = y;
        if (CODES) codes[sp.tail0 + gid] = (int8_t)q;
    }
}

}  // namespace

void actquant_check(const ActQuantCfg& c) {
    CMOOP_REQUIRE(c.bits == 0 || (c.bits >= 2 && c.bits <= 8), "actquant: bits must be 0 (off) or in [2, 8]");
    CMOOP_REQUIRE(c.momentum >= 0.f && c.momentum < 1.f, "actquant: momentum must be in [0, 1)");
    CMOOP_REQUIRE(c.reserved[0] == 0 && c.reserved[1] == 0, "actquant: reserved must be 0");
}

EmaPair actquant_rates(float momentum) { return EmaPair{momentum, (float)(1.0 - (double)momentum)}; }

void launch_fake_quant_act(float* x, int64_t n, int bits, bool tracked, uint32_t* partials, ActRange* rec, float mu, float omu,
                           hipStream_t s, int8_t* codes) {
    CMOOP_REQUIRE(bits >= 2 && bits <= 8, "fake_quant_act: bits must be in [2, 8]");
    CMOOP_REQUIRE(n >= 0 && n <= ACT_QUANT_MAX_ELEMS, "fake_quant_act: n must stay below 2^31 elements (ACT_QUANT_MAX_ELEMS: 32-bit index math)");
    if (n == 0) return;
    CMOOP_REQUIRE(x && rec && (tracked || partials), "fake_quant_act: NULL buffer");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(x) % 4 == 0, "fake_quant_act: x must be aligned to 4 bytes");
    const int blocks = act_quant_blocks(n);
    const float qmaxf = (float)quant_qmax(bits);
    CMOOP_REQUIRE(!codes || tracked, "fake_quant_act: codes are written in tracked mode only");
    if (tracked && codes) {
        hipLaunchKernelGGL((act_quant_apply_kernel<true, true>), dim3((unsigned)blocks), dim3(256), 0, s, x, (int)n, nullptr, 0, rec, qmaxf,
                           mu, omu, codes);
    } else if (tracked) {
        hipLaunchKernelGGL(act_quant_apply_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, s, x, (int)n, nullptr, 0, rec, qmaxf, mu, omu,
                           nullptr);
    } else {
        hipLaunchKernelGGL(act_absmax_kernel, dim3((unsigned)blocks), dim3(256), 0, s, x, (int)n, partials);
        hipLaunchKernelGGL(act_quant_apply_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, s, x, (int)n, partials, blocks, rec, qmaxf, mu,
                           omu, nullptr);
    }
    CMOOP_HIP(hipGetLastError());
}

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
