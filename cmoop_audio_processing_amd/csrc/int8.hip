// Integer inference (include/cmoop.h fixes the arithmetic at "Integer inference"): the OP_CONV / OP_DENSE layers of a full-int8
// model on the i8 matrix cores of gfx950 (v_mfma_i32_16x16x64_i8), exact int32 accumulation of the int8 codes and ONE
// dequantising epilogue per output:  y = fl(fl((float)acc * fl(s_x * s_w[c])) + bias[c]), then max(y, 0) where the op has a ReLU.
// Inference only: no split-K, no atomics, no statistics epilogue; 32-bit index math inside the bounds the launchers check.
// The ..._q kernels are the same tiles with the requantising epilogue ("Integer inference: requantising epilogue"): the eval
// BatchNorm as one fma, its ReLU, and the tracked quantiser of the site written -- the fp32 quad and one word of four codes.
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
// the requantising epilogue (include/cmoop.h, "Integer inference: requantising epilogue"): after the epilogue above, the eval
// BatchNorm affine as ONE fma (what scale_shift_kernel compiles to) with its ReLU, then the tracked quantiser of the site written
struct I8Req {
    const float* bn_scale;  // [Cout] or null (then bn_shift is null too): what bn_eval_prepare_kernel left
    const float* bn_shift;
    const ActRange* rec_out;   // s_out = quant_scale(rec_out->r, qmax_out), formed as the tracked apply kernel forms it
    int8_t* codes;          // [M][Cout], 4-byte aligned
    float qmax_out;
    int relu_after;
};

template <bool CONV, int MT, int NT, bool REQ = false>
__device__ __forceinline__ void i8_tile(const int8_t* __restrict__ xq, const int8_t* __restrict__ wq, float* __restrict__ y,
                                        const I8Geom g, const I8Epi e, const I8Req q = I8Req()) {
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
    const float s_out = REQ ? quant_scale(__float_as_uint(q.rec_out->r), q.qmax_out) : 0.f;
    const bool live = s_out > 0.f;
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
            if (REQ) {   // Cout % 4 == 0 (the launcher's): the quad is whole.  y is the SITE's act; one word of four codes
                int qc[4];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    float t = v[r];
                    if (q.bn_scale) {
                        t = __builtin_fmaf(t, q.bn_scale[n + r], q.bn_shift[n + r]);   // ONE rounding, as scale_shift_kernel
                        t = q.relu_after ? fmaxf(t, 0.f) : t;
                    }
                    quant_element(t, s_out, live, q.qmax_out, qc[r], v[r]);
                }
                *reinterpret_cast<f32x4*>(out) = f32x4{v[0], v[1], v[2], v[3]};
                *reinterpret_cast<uint32_t*>(q.codes + m * g.Cout + n) = quant_pack4(qc);
            } else if (e.vec) {
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

template <int MT, int NT>
__global__ __launch_bounds__(256) void conv_i8_fwd_q_kernel(const int8_t* __restrict__ xq, const int8_t* __restrict__ wq,
                                                            float* __restrict__ y, const I8Geom g, const I8Epi e, const I8Req q) {
    i8_tile<true, MT, NT, true>(xq, wq, y, g, e, q);
}

template <int MT, int NT>
__global__ __launch_bounds__(256) void dense_i8_fwd_q_kernel(const int8_t* __restrict__ xq, const int8_t* __restrict__ wq,
                                                             float* __restrict__ y, const I8Geom g, const I8Epi e, const I8Req q) {
    i8_tile<false, MT, NT, true>(xq, wq, y, g, e, q);
}

constexpr int64_t I8_MAX_ELEMS = ((int64_t)1 << 31) - 1;   // every operand and the output: 32-bit index math

// ---- integer depthwise (include/cmoop.h, "Integer depthwise") -------------------------------------------------------------------
// dwconv_fwd_kernel's work split on int8 codes: work item = (sample, run of RH image rows, column), a lane owns 4 channels of
// one item -- ONE 4-byte load per horizontal tap of an input row, read once and reused by the K output rows it reaches -- and
// a workgroup is CB4 channel quads x 256 / CB4 items with consecutive columns.  (16 channels per lane, a 16-byte load per tap,
// would need K K 16 weight registers: 400 at K = 5.)  The codes are converted to fp32 once per load and accumulated with FMAs:
// every partial sum is an integer below 2^24, so each FMA is exact and the sum is the int32 sum.  The workgroup's weight codes
// are staged once through LDS with 16-byte loads and converted once per lane.  The epilogue dequantises once and, with a
// record of the output site, applies the tracked quantiser (quant_math.h) and stores the four codes as one word.
constexpr int DWI8_MAX_CB4 = 16;                // channel quads per workgroup: 64 bytes of one pixel
constexpr int DWI8_TARGET_THREADS = 256 * 1024;

struct DwI8Args {
    const int8_t* xq;           // [B][H][W][C] codes
    const int8_t* wq;           // [K][K][C] codes
    const float* s_w;           // [C]
    const ActRange* rec_in;     // non-null: s_x = quant_scale(rec_in->r, qmax_in)
    const ActRange* rec_out;    // non-null: the tracked quantiser of the output under rec_out->r; null: y = z
    float* y;                   // [B][H][W][C]
    int8_t* codes;              // [B][H][W][C] or null (only with rec_out)
    float s_x, qmax_in, qmax_out;
    int H, W, C, RH, runs, items, cb4_log;
};

__device__ __forceinline__ f32x4 dwi8_unpack(uint32_t v) {   // four signed bytes -> fp32, exact
    return f32x4{(float)(int8_t)(v & 0xFFu), (float)(int8_t)((v >> 8) & 0xFFu), (float)(int8_t)((v >> 16) & 0xFFu),
                 (float)(int8_t)(v >> 24)};
}

template <int K>
__global__ __launch_bounds__(256) void dwconv_i8_fwd_kernel(const DwI8Args a) {
    constexpr int P = (K - 1) / 2, TAPS = K * K;
    __shared__ i32x4 wl[TAPS * DWI8_MAX_CB4 / 4];   // [tap][DWI8_MAX_CB4] words of four codes
    const int t = threadIdx.x, CB4 = 1 << a.cb4_log;
    const int cql = t & (CB4 - 1), slot = t >> a.cb4_log;
    const int c0 = (int)blockIdx.y * CB4 * 4;
    const int pl = a.cb4_log - 2;                   // log2 of the 16-byte pieces of one tap's row (CB4 >= 4)
    for (int i = t; i < (TAPS << pl); i += 256) {   // the workgroup's K*K x (CB4*4) weight codes, staged once
        const int tap = i >> pl, p = i & ((1 << pl) - 1);
        wl[tap * (DWI8_MAX_CB4 / 4) + p] = *reinterpret_cast<const i32x4*>(a.wq + tap * a.C + c0 + p * 16);
    }
    __syncthreads();
    const int item = (int)blockIdx.x * (256 >> a.cb4_log) + slot;
    if (item >= a.items) return;
    const uint32_t* wlw = reinterpret_cast<const uint32_t*>(wl);
    f32x4 wr[TAPS];
#pragma unroll
    for (int i = 0; i < TAPS; ++i) wr[i] = dwi8_unpack(wlw[i * DWI8_MAX_CB4 + cql]);
    // item -> (sample, run, column): 32-bit divisions, once per item
    const unsigned q = (unsigned)item / (unsigned)a.W;
    const unsigned b = q / (unsigned)a.runs, run = q - b * (unsigned)a.runs;
    const int w = (int)((unsigned)item - q * (unsigned)a.W);
    const int row_base = (int)b * a.H, h0 = (int)run * a.RH, h1 = min(a.H, h0 + a.RH);
    const int c = c0 + cql * 4;
    // scales: one product per channel; the output site's scale as the tracked apply kernel forms it
    const float s_x = a.rec_in ? quant_scale(__float_as_uint(a.rec_in->r), a.qmax_in) : a.s_x;
    const f32x4 sw = *reinterpret_cast<const f32x4*>(a.s_w + c);
    const f32x4 sc = {s_x * sw[0], s_x * sw[1], s_x * sw[2], s_x * sw[3]};
    const float s_out = a.rec_out ? quant_scale(__float_as_uint(a.rec_out->r), a.qmax_out) : 0.f;
    const bool live = s_out > 0.f;
    f32x4 acc[K];   // acc[j]: output row r - P + j, which input row r reaches through vertical tap K - 1 - j
#pragma unroll
    for (int j = 0; j < K; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int r = h0 - P; r < h1 + P; ++r) {
        f32x4 x[K];
        const bool rv = r >= 0 && r < a.H;
        const int base = ((row_base + r) * a.W + (w - P)) * a.C + c;
#pragma unroll
        for (int kx = 0; kx < K; ++kx) {
            const int col = w + kx - P;
            uint32_t v = 0u;                        // SAME padding: zero codes, never read from memory
            if (rv && col >= 0 && col < a.W) v = *reinterpret_cast<const uint32_t*>(a.xq + base + kx * a.C);
            x[kx] = dwi8_unpack(v);
        }
#pragma unroll
        for (int j = 0; j < K; ++j)
#pragma unroll
            for (int kx = 0; kx < K; ++kx) acc[j] = __builtin_elementwise_fma(x[kx], wr[(K - 1 - j) * K + kx], acc[j]);   // exact
        const int h = r - P;   // complete: r is its last input row
        if (h >= h0) {
            const int o = ((row_base + h) * a.W + w) * a.C + c;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = acc[0][e] * sc[e];      // z: one product
            if (a.rec_out) {
                int qc[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    float yq;
                    quant_element(v[e], s_out, live, a.qmax_out, qc[e], yq);
                    v[e] = yq;
                }
                if (a.codes)
                    *reinterpret_cast<uint32_t*>(a.codes + o) = quant_pack4(qc);
            }
            *reinterpret_cast<f32x4*>(a.y + o) = v;
        }
#pragma unroll
        for (int j = 0; j + 1 < K; ++j) acc[j] = acc[j + 1];
        acc[K - 1] = f32x4{0.f, 0.f, 0.f, 0.f};
    }
}

// THE shape rules of the integer kernels, one predicate per refusal: the launchers' checks and the plan's predicates
// (int8_layer_ok / int8_dw_layer_ok) are made of these
bool i8_ks_ok(int KS) { return KS == 1 || KS == 3 || KS == 5; }
bool i8_stride_ok(int KS, int stride) { return stride == 1 || (stride == 2 && KS == 1); }
bool i8_cin_ok(int Cin) { return Cin >= 16 && Cin % 16 == 0; }
// |acc| <= 127 * 127 * K must stay inside int32 (the largest layer of the search space, 512 -> 512 k5: K = 12800)
bool i8_acc_ok(int64_t K) { return (int64_t)127 * 127 * K < ((int64_t)1 << 31); }
bool dwi8_ks_ok(int KS) { return KS == 3 || KS == 5; }
bool dwi8_channels_ok(int C) { return C >= 16 && C <= 512 && ilog2_exact(C) >= 0; }

}  // namespace

bool int8_dw_layer_ok(int C, int KS) { return dwi8_channels_ok(C) && dwi8_ks_ok(KS); }

void launch_dwconv_i8_fwd(const int8_t* xq, const int8_t* wq, float s_x, const ActRange* rec_in, int act_bits, const float* s_w,
                          const ActRange* rec_out, int out_bits, float* y, int8_t* codes, int B, int H, int W, int C, int KS,
                          hipStream_t s) {
    CMOOP_REQUIRE(B >= 0 && H >= 1 && W >= 1, "dwconv_fwd_i8: empty image");
    CMOOP_REQUIRE(dwi8_ks_ok(KS), "dwconv_fwd_i8: KS must be 3 or 5");
    CMOOP_REQUIRE(dwi8_channels_ok(C), "dwconv_fwd_i8: channels must be a power of two in 16..512");
    CMOOP_REQUIRE(!rec_in || (act_bits >= 2 && act_bits <= 8), "dwconv_fwd_i8: activation bits must be in [2, 8]");
    CMOOP_REQUIRE(!rec_out || (out_bits >= 2 && out_bits <= 8), "dwconv_fwd_i8: output bits must be in [2, 8]");
    CMOOP_REQUIRE(!codes || rec_out, "dwconv_fwd_i8: codes are written only under an output range");
    if (B == 0) return;
    // 32-bit index math: element offsets of the codes, byte offsets of y four times as large
    CMOOP_REQUIRE((int64_t)B * H * W * C < (1ll << 29), "dwconv_fwd_i8: activation exceeds 2^29 elements (32-bit offsets)");
    CMOOP_REQUIRE(xq && wq && s_w && y, "dwconv_fwd_i8: NULL buffer");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(xq) % 16 == 0 && reinterpret_cast<uintptr_t>(wq) % 16 == 0,
                  "dwconv_fwd_i8: code buffers must be aligned to 16 bytes");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(y) % 16 == 0 && reinterpret_cast<uintptr_t>(s_w) % 16 == 0,
                  "dwconv_fwd_i8: y and s_w must be aligned to 16 bytes");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(codes) % 4 == 0, "dwconv_fwd_i8: the output codes must be aligned to 4 bytes");
    DwI8Args a;
    a.xq = xq; a.wq = wq; a.s_w = s_w; a.rec_in = rec_in; a.rec_out = rec_out; a.y = y; a.codes = codes;
    a.s_x = s_x;
    a.qmax_in = rec_in ? (float)quant_qmax(act_bits) : 0.f;
    a.qmax_out = rec_out ? (float)quant_qmax(out_bits) : 0.f;
    a.H = H; a.W = W; a.C = C;
    const int C4 = C / 4, CB4 = std::min(C4, DWI8_MAX_CB4);
    a.cb4_log = ilog2_exact(CB4);
    // rows per run: shorter runs (more halo rows re-read through the caches) until the launch fills the chip
    a.RH = std::min(H, 16);
    while (a.RH > 4 && (int64_t)B * cdiv(H, a.RH) * W * C4 < DWI8_TARGET_THREADS) a.RH = (a.RH + 1) / 2;
    a.runs = cdiv(H, a.RH);
    a.items = B * a.runs * W;
    const dim3 grid((unsigned)cdiv(a.items, 256 / CB4), (unsigned)(C4 / CB4));
    if (KS == 3) hipLaunchKernelGGL(dwconv_i8_fwd_kernel<3>, grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL(dwconv_i8_fwd_kernel<5>, grid, dim3(256), 0, s, a);
    CMOOP_HIP(hipGetLastError());
}

bool int8_layer_ok(int Cin, int Cout, int KS, int stride) {
    return i8_cin_ok(Cin) && Cout >= 1 && i8_ks_ok(KS) && i8_stride_ok(KS, stride) && i8_acc_ok((int64_t)KS * KS * Cin);
}

// the four kernel families at one NT; the conv tiles are two row blocks high, the dense tiles one
template <int NT>
static void i8_launch_nt(bool conv, dim3 grid, hipStream_t s, const int8_t* xq, const int8_t* wq, float* y, const I8Geom& g, const I8Epi& e,
                         const I8Req* q) {
    if (conv && q) hipLaunchKernelGGL((conv_i8_fwd_q_kernel<2, NT>), grid, dim3(256), 0, s, xq, wq, y, g, e, *q);
    else if (conv) hipLaunchKernelGGL((conv_i8_fwd_kernel<2, NT>), grid, dim3(256), 0, s, xq, wq, y, g, e);
    else if (q) hipLaunchKernelGGL((dense_i8_fwd_q_kernel<1, NT>), grid, dim3(256), 0, s, xq, wq, y, g, e, *q);
    else hipLaunchKernelGGL((dense_i8_fwd_kernel<1, NT>), grid, dim3(256), 0, s, xq, wq, y, g, e);
}

void launch_i8_fwd(const I8Layer& L, const int8_t* xq, const int8_t* wq, float s_x, const ActRange* rec, int act_bits, const float* s_w,
                   const float* bias, float* y, int relu, const I8Requant* rq, hipStream_t s) {
    const std::string w = std::string(L.conv ? "conv_fwd_i8" : "dense_fwd_i8") + (rq ? "_q" : "");
    const int Cout = L.Cout;
    if (L.conv) {
        CMOOP_REQUIRE(L.B >= 0 && L.H >= 1 && L.W >= 1, w + ": empty image");
        CMOOP_REQUIRE(i8_ks_ok(L.KS), w + ": KS must be 1, 3 or 5");
        CMOOP_REQUIRE(i8_stride_ok(L.KS, L.stride), w + ": stride 1, or the 1x1 stride-2 projection");
        CMOOP_REQUIRE(i8_cin_ok(L.Cin), w + ": Cin must be a multiple of 16");
    } else {
        CMOOP_REQUIRE(L.B >= 0 && Cout >= 1, w + ": M >= 0 and N >= 1");
        CMOOP_REQUIRE(i8_cin_ok(L.Cin), w + ": K must be a multiple of 16");
    }
    CMOOP_REQUIRE(!rec || (act_bits >= 2 && act_bits <= 8), w + ": activation bits must be in [2, 8]");
    I8Req q{};
    if (rq) {   // the checks the requantising epilogue adds, ahead of the empty-batch return
        CMOOP_REQUIRE(Cout % 4 == 0, w + ": Cout must be a multiple of 4 (a lane stores four channels as one word of codes)");
        CMOOP_REQUIRE((rq->bn_scale != nullptr) == (rq->bn_shift != nullptr), w + ": bn_scale and bn_shift come together or not at all");
        CMOOP_REQUIRE(rq->rec_out != nullptr, w + ": the record of the site written is required");
        CMOOP_REQUIRE(rq->out_bits >= 2 && rq->out_bits <= 8, w + ": output bits must be in [2, 8]");
        CMOOP_REQUIRE(rq->codes != nullptr, w + ": NULL codes");
        CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(y) % 16 == 0, w + ": y must be aligned to 16 bytes");
        CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(rq->codes) % 4 == 0, w + ": the output codes must be aligned to 4 bytes");
        q = I8Req{rq->bn_scale, rq->bn_shift, rq->rec_out, rq->codes, (float)quant_qmax(rq->out_bits), rq->relu_after};
    }
    if (L.B == 0) return;
    const int64_t OH = (L.H + L.stride - 1) / L.stride, OW = (L.W + L.stride - 1) / L.stride;
    const int64_t M = (int64_t)L.B * OH * OW, K = (int64_t)L.KS * L.KS * L.Cin;
    CMOOP_REQUIRE(K >= 16 && K % 16 == 0, w + ": the reduction must be whole 16-channel fragments");
    CMOOP_REQUIRE(i8_acc_ok(K), w + ": 127^2 K must stay below 2^31 (exact int32 accumulation)");
    CMOOP_REQUIRE(Cout >= 1 && (int64_t)L.B * L.H * L.W * L.Cin <= I8_MAX_ELEMS && M * Cout <= I8_MAX_ELEMS && (int64_t)Cout * K <= I8_MAX_ELEMS,
                  w + ": operands and output must stay below 2^31 elements (32-bit index math)");
    CMOOP_REQUIRE(xq && wq && s_w && bias && y, w + ": NULL buffer");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(xq) % 16 == 0 && reinterpret_cast<uintptr_t>(wq) % 16 == 0,
                  w + ": code buffers must be aligned to 16 bytes");
    CMOOP_REQUIRE(reinterpret_cast<uintptr_t>(y) % 4 == 0, w + ": y must be aligned to 4 bytes");
    const ConvGeom cg = conv_geometry(L.B, L.H, L.W, L.Cin, Cout, L.KS, L.stride);   // dense (1 x 1, KS 1): OH = OW = 1, no padding
    const I8Geom g{L.H, L.W, L.Cin, cg.OH, cg.OW, Cout, L.KS, L.stride, cg.pad_t, cg.pad_l, (int)M, (int)(K / 16), L.Cin / 16};
    const I8Epi e{s_w, bias, rec, s_x, rec ? (float)quant_qmax(act_bits) : 0.f, relu,
                  (rq || (reinterpret_cast<uintptr_t>(y) % 16 == 0 && Cout % 4 == 0)) ? 1 : 0};
    const unsigned gx = (unsigned)cdiv64(M, L.conv ? 128 : 64);   // four waves of 16 MT rows
    const I8Req* qp = rq ? &q : nullptr;
    if (Cout > 32) i8_launch_nt<4>(L.conv, dim3(gx, (unsigned)cdiv(Cout, 64)), s, xq, wq, y, g, e, qp);
    else if (Cout > 16) i8_launch_nt<2>(L.conv, dim3(gx, 1u), s, xq, wq, y, g, e, qp);
    else i8_launch_nt<1>(L.conv, dim3(gx, 1u), s, xq, wq, y, g, e, qp);
    CMOOP_HIP(hipGetLastError());
}

}  // namespace cmoop
