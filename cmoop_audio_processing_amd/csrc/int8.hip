// Integer inference (include/cmoop.h fixes the arithmetic at "Integer inference"): the OP_CONV / OP_DENSE layers of a full-int8
// model on the i8 matrix cores of gfx950 (v_mfma_i32_16x16x64_i8), exact int32 accumulation of the int8 codes and ONE
// dequantising epilogue per output:  y = fl(fl((float)acc * fl(s_x * s_w[c])) + bias[c]), then max(y, 0) where the op has a ReLU.
// Inference only: no split-K, no atomics, no statistics epilogue; 32-bit index math inside the bounds the launchers check.
//
// Tiling (the simplest correct one: operands straight from global memory, no LDS).  K is a sequence of 16-byte FRAGMENTS: 16
// input channels of one (pixel, tap) -- [Cout][kh][kw][Cin] weight rows and NHWC activation pixels hold them contiguously, so a
// fragment is one 16-byte load, and a padding tap is a zero fragment that is never read from memory.  One MFMA takes four
// fragments of K (lane l: fragment l >> 4); a K that is no multiple of 64 ends in zero fragments.  The WEIGHTS are the
// instruction's row operand and the activations its column operand: lane l of the 16x16 result then holds, for output row
// m0 + (l & 15), the four consecutive channels n0 + 4 (l >> 4) + {0..3} -- one 16-byte store.  A wave computes MT x NT such
// blocks (16 MT output rows, 16 NT channels), a workgroup is four waves on consecutive row groups of the same channels.
#include "kernels.h"
#include "quant_math.h"

#pragma clang fp contract(off)

namespace cmoop {
namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

struct I8Geom {
    int H, W, Cin, OH, OW, Cout, KS, stride, pad_t, pad_l;
    int M;        // output rows: B OH OW (dense: the batch rows)
    int F;        // fragments of one weight row: KS KS Cin / 16
    int CC;       // fragments of one tap: Cin / 16
};
struct I8Epi {
    const float* s_w;       // [Cout] weight channel scales
    const float* bias;      // [Cout]
    const ActRange* rec;    // non-null: s_x = quant_scale(rec->r, qmaxf), formed as the tracked apply kernel forms it
    float s_x, qmaxf;
    int relu, vec;          // vec: y is 16-byte aligned and Cout % 4 == 0 -> 16-byte stores
};

template <bool CONV, int MT, int NT>
__device__ __forceinline__ void i8_tile(const int8_t* __restrict__ xq, const int8_t* __restrict__ wq, float* __restrict__ y,
                                        const I8Geom g, const I8Epi e) {
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int r16 = lane & 15, kg = lane >> 4;
    const int m_base = ((int)blockIdx.x * 4 + wave) * (16 * MT);
    const int n_base = (int)blockIdx.y * (16 * NT);
    if (m_base >= g.M) return;                       // the whole wave

    // column operand: the output row of this lane in each of the MT blocks
    int xoff[MT], ih0[MT], iw0[MT];
    bool mv[MT];
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m_base + 16 * i + r16;
        mv[i] = m < g.M;
        if (CONV) {
            const int hw = g.OH * g.OW;
            const int b = m / hw, rem = m - b * hw;
            const int oh = rem / g.OW, ow = rem - oh * g.OW;
            xoff[i] = b * g.H * g.W;                 // first pixel of the image
            ih0[i] = oh * g.stride - g.pad_t;
            iw0[i] = ow * g.stride - g.pad_l;
        } else {
            xoff[i] = m * g.Cin;
            ih0[i] = iw0[i] = 0;
        }
    }
    // row operand: the output channel of this lane in each of the NT blocks
    int woff[NT];
    bool nv[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) {
        const int n = n_base + 16 * j + r16;
        nv[j] = n < g.Cout;
        woff[j] = n * (g.F * 16);
    }

    i32x4 acc[MT][NT];
#pragma unroll
    for (int i = 0; i < MT; ++i)
#pragma unroll
        for (int j = 0; j < NT; ++j) acc[i][j] = i32x4{0, 0, 0, 0};

    // the lane's fragment f = f0 + kg as (kh, kw, cc), advanced by four fragments per step
    int kh = 0, kw = 0, cc = kg;
    if (CONV)
        while (cc >= g.CC) { cc -= g.CC; if (++kw == g.KS) { kw = 0; ++kh; } }
    const i32x4 zero = {0, 0, 0, 0};
    for (int f0 = 0; f0 < g.F; f0 += 4) {
        const int f = f0 + kg;
        const bool fv = f < g.F;                     // past the row: a zero fragment
        i32x4 a[NT], b[MT];
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            a[j] = zero;
            if (fv && nv[j]) a[j] = *reinterpret_cast<const i32x4*>(wq + woff[j] + f * 16);
        }
#pragma unroll
        for (int i = 0; i < MT; ++i) {
            b[i] = zero;
            if (CONV) {
                const int ih = ih0[i] + kh, iw = iw0[i] + kw;
                if (fv && mv[i] && (unsigned)ih < (unsigned)g.H && (unsigned)iw < (unsigned)g.W)   // else SAME padding: zero
                    b[i] = *reinterpret_cast<const i32x4*>(xq + (xoff[i] + ih * g.W + iw) * g.Cin + cc * 16);
            } else {
                if (fv && mv[i]) b[i] = *reinterpret_cast<const i32x4*>(xq + xoff[i] + f * 16);
            }
        }
#pragma unroll
        for (int i = 0; i < MT; ++i)
#pragma unroll
            for (int j = 0; j < NT; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[j], b[i], acc[i][j], 0, 0, 0);
        if (CONV) {
            cc += 4;
            while (cc >= g.CC) { cc -= g.CC; if (++kw == g.KS) { kw = 0; ++kh; } }
        }
    }

    // epilogue: result element (row = channel 4 kg + r of the block, column = output row r16)
    const float s_x = e.rec ? quant_scale(__float_as_uint(e.rec->r), e.qmaxf) : e.s_x;
#pragma unroll
    for (int i = 0; i < MT; ++i) {
        const int m = m_base + 16 * i + r16;
        if (m >= g.M) continue;
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n_base + 16 * j + 4 * kg;
            if (n >= g.Cout) continue;
            float v[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int c = min(n + r, g.Cout - 1);                 // a channel past the end is computed, never stored
                const float sc = s_x * e.s_w[c];                     // one product
                float t = (float)acc[i][j][r] * sc;                  // int32 -> fp32 round to nearest even, one product
                t = t + e.bias[c];                                   // one sum
                v[r] = e.relu ? fmaxf(t, 0.f) : t;
            }
            float* out = y + m * g.Cout + n;
            if (e.vec) {
                *reinterpret_cast<f32x4*>(out) = f32x4{v[0], v[1], v[2], v[3]};
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (n + r < g.Cout) out[r] = v[r];
            }
        }
    }
}

template <int MT, int NT>
__global__ __launch_bounds__(256) void conv_i8_fwd_kernel(const int8_t* __restrict__ xq, const int8_t* __restrict__ wq,
                                                          float* __restrict__ y, const I8Geom g, const I8Epi e) {
    i8_tile<true, MT, NT>(xq, wq, y, g, e);
}

template <int MT, int NT>
__global__ __launch_bounds__(256) void dense_i8_fwd_kernel(const int8_t* __restrict__ xq, const int8_t* __restrict__ wq,
                                                           float* __restrict__ y, const I8Geom g, const I8Epi e) {
    i8_tile<false, MT, NT>(xq, wq, y, g, e);
}

constexpr int64_t I8_MAX_ELEMS = ((int64_t)1 << 31) - 1;   // every operand and the output: 32-bit index math

void i8_check_common(const void* xq, const void* wq, const float* s_w, const float* bias, const float* y, int64_t x_elems,
                     int64_t M, int64_t K, int Cout, const char* who) {
    const std::string w(who);
    CMOOP_REQUIRE(K >= 16 && K % 16 == 0, w + ": the reduction must be whole 16-channel fragments");
    // |acc| <= 127 * 127 * K must stay inside int32 (the largest layer of the search space, 512 -> 512 k5: K = 12800)
    CMOOP_REQUIRE((int64_t)127 * 127 * K < ((int64_t)1 << 31), w + ": 127^2 K must stay below 2^31 (exact int32 accumulation)");
    CMOOP_REQUIRE(Cout >= 1 && x_elems <= I8_MAX_ELEMS && M * Cout <= I8_MAX_ELEMS && (int64_t)Cout * K <= I8_MAX_ELEMS,
                  w + ": operands and output must stay below 2^31 elements (32-bit index math)");
    CMOOP_REQUIRE(xq && wq && s_w && bias && y, w + ": NULL buffer");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(xq) % 16 == 0 && reinterpret_cast<uintptr_t>(wq) % 16 == 0,
                  w + ": code buffers must be aligned to 16 bytes");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(y) % 4 == 0, w + ": y must be aligned to 4 bytes");
}

}  // namespace

bool int8_layer_ok(int Cin, int Cout, int KS, int stride) {
    return Cin >= 16 && Cin % 16 == 0 && Cout >= 1 && (KS == 1 || KS == 3 || KS == 5) && (stride == 1 || (stride == 2 && KS == 1)) &&
           (int64_t)127 * 127 * KS * KS * Cin < ((int64_t)1 << 31);
}

void launch_conv_i8_fwd(const int8_t* xq, const int8_t* wq, float s_x, const ActRange* rec, int act_bits, const float* s_w,
                        const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int KS, int stride, int relu,
                        hipStream_t s) {
    CMOOP_REQUIRE(B >= 0 && H >= 1 && W >= 1, "conv_fwd_i8: empty image");
    CMOOP_REQUIRE(KS == 1 || KS == 3 || KS == 5, "conv_fwd_i8: KS must be 1, 3 or 5");
    CMOOP_REQUIRE(stride == 1 || (stride == 2 && KS == 1), "conv_fwd_i8: stride 1, or the 1x1 stride-2 projection");
    CMOOP_REQUIRE(Cin >= 16 && Cin % 16 == 0, "conv_fwd_i8: Cin must be a multiple of 16");
    CMOOP_REQUIRE(!rec || (act_bits >= 2 && act_bits <= 8), "conv_fwd_i8: activation bits must be in [2, 8]");
    if (B == 0) return;
    const int64_t OH = (H + stride - 1) / stride, OW = (W + stride - 1) / stride;
    const int64_t M = (int64_t)B * OH * OW, K = (int64_t)KS * KS * Cin;
    i8_check_common(xq, wq, s_w, bias, y, (int64_t)B * H * W * Cin, M, K, Cout, "conv_fwd_i8");
    const ConvGeom cg = conv_geometry(B, H, W, Cin, Cout, KS, stride);
    const I8Geom g{H, W, Cin, cg.OH, cg.OW, Cout, KS, stride, cg.pad_t, cg.pad_l, (int)M, (int)(K / 16), Cin / 16};
    const I8Epi e{s_w, bias, rec, s_x, rec ? (float)quant_qmax(act_bits) : 0.f, relu,
                  (reinterpret_cast<uintptr_t>(y) % 16 == 0 && Cout % 4 == 0) ? 1 : 0};
    constexpr int MT = 2;
    const unsigned gx = (unsigned)cdiv64(M, 64 * MT);
    if (Cout > 32) hipLaunchKernelGGL((conv_i8_fwd_kernel<MT, 4>), dim3(gx, (unsigned)cdiv(Cout, 64)), dim3(256), 0, s, xq, wq, y, g, e);
    else if (Cout > 16) hipLaunchKernelGGL((conv_i8_fwd_kernel<MT, 2>), dim3(gx, 1u), dim3(256), 0, s, xq, wq, y, g, e);
    else hipLaunchKernelGGL((conv_i8_fwd_kernel<MT, 1>), dim3(gx, 1u), dim3(256), 0, s, xq, wq, y, g, e);
    CMOOP_HIP(hipGetLastError());
}

void launch_dense_i8_fwd(const int8_t* xq, const int8_t* wq, float s_x, const ActRange* rec, int act_bits, const float* s_w,
                         const float* bias, float* y, int M, int N, int K, int relu, hipStream_t s) {
    CMOOP_REQUIRE(M >= 0 && N >= 1, "dense_fwd_i8: M >= 0 and N >= 1");
    CMOOP_REQUIRE(K >= 16 && K % 16 == 0, "dense_fwd_i8: K must be a multiple of 16");
    CMOOP_REQUIRE(!rec || (act_bits >= 2 && act_bits <= 8), "dense_fwd_i8: activation bits must be in [2, 8]");
    if (M == 0) return;
    i8_check_common(xq, wq, s_w, bias, y, (int64_t)M * K, M, K, N, "dense_fwd_i8");
    const I8Geom g{1, 1, K, 1, 1, N, 1, 1, 0, 0, M, K / 16, K / 16};
    const I8Epi e{s_w, bias, rec, s_x, rec ? (float)quant_qmax(act_bits) : 0.f, relu,
                  (reinterpret_cast<uintptr_t>(y) % 16 == 0 && N % 4 == 0) ? 1 : 0};
    const unsigned gx = (unsigned)cdiv(M, 64);
    if (N > 32) hipLaunchKernelGGL((dense_i8_fwd_kernel<1, 4>), dim3(gx, (unsigned)cdiv(N, 64)), dim3(256), 0, s, xq, wq, y, g, e);
    else if (N > 16) hipLaunchKernelGGL((dense_i8_fwd_kernel<1, 2>), dim3(gx, 1u), dim3(256), 0, s, xq, wq, y, g, e);
    else hipLaunchKernelGGL((dense_i8_fwd_kernel<1, 1>), dim3(gx, 1u), dim3(256), 0, s, xq, wq, y, g, e);
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
