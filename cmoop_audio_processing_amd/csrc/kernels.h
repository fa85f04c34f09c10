// Host-side launchers of every HIP kernel in libcmoop_hip.so (gfx950 / CDNA4).
// All tensors are fp32, activations NHWC, conv/dense kernels in the canonical
// [C_out][kh][kw][C_in] layout (K = kh*kw*C_in contiguous) -- see genes.py.
#pragma once
#include "common.h"
#include <string>
#include <vector>

namespace cmoop {

// ---------------------------------------------------------------------------
// Implicit-GEMM convolution on the fp32 MFMA (v_mfma_f32_16x16x4_f32).
// Replaces the Keras Conv2D / Dense fwd+bwd the reference delegates to TF
// (nsga_penalty.py:255-330 via Model.fit, :383).
// ---------------------------------------------------------------------------
struct ConvGeom {
    int B, H, W, Cin;        // input  [B,H,W,Cin]
    int OH, OW, Cout;        // output [B,OH,OW,Cout]
    int KH, KW, stride;
    int pad_t, pad_l;        // TF "SAME": total//2 on top/left, remainder bottom/right
    int M() const { return B * OH * OW; }
    int K() const { return KH * KW * Cin; }
};
// geometry of a square-window SAME convolution (output ceil(H / stride) x ceil(W / stride))
inline ConvGeom conv_geometry(int B, int H, int W, int Cin, int Cout, int KS, int stride) {
    ConvGeom g;
    g.B = B; g.H = H; g.W = W; g.Cin = Cin; g.Cout = Cout; g.KH = g.KW = KS; g.stride = stride;
    g.OH = (H + stride - 1) / stride; g.OW = (W + stride - 1) / stride;
    const int th = (g.OH - 1) * stride + KS - H, tw = (g.OW - 1) * stride + KS - W;
    g.pad_t = (th > 0 ? th : 0) / 2; g.pad_l = (tw > 0 ? tw : 0) / 2;
    return g;
}

// Arithmetic of the MFMA GEMM kernels.  GEMM_FP32 (exact v_mfma_f32_16x16x4_f32) is the product default;
// the bf16 matrix-core modes are opt-in (cmoop_config.gemm_mode or CMOOP_GEMM_MODE=bf16x3|bf16), see gemm.hip.
enum GemmMode { GEMM_DEFAULT = -1, GEMM_FP32 = 0, GEMM_FP32_DMA = 1 /* kernel-internal: fp32 with LDS-DMA operand loads */, GEMM_BF16X3 = 2, GEMM_BF16 = 3,
                GEMM_FP32_HALO = 4 /* kernel-internal: fp32, halo-tiled direct convolution (halo_fwd_kernel) */ };
int gemm_mode_default();   // CMOOP_GEMM_MODE, else GEMM_FP32

struct GemmEpilogue {
    int mode = GEMM_DEFAULT;       // GemmMode of this launch (GEMM_DEFAULT: gemm_mode_default())
    const float* bias = nullptr;   // + bias[col]
    int relu = 0;                  // max(v, 0)
    const float* mask = nullptr;   // v = mask[out] > 0 ? v * mask_scale : 0   (ReLU/dropout backward)
    float mask_scale = 1.f;
    int accumulate = 0;            // out += v
    int out_stride = 1;            // >1: row (b,oh,ow) is stored at (b, oh*s, ow*s) of [B,OHf,OWf,N]
    int OHf = 0, OWf = 0;
    int dropout = 0;               // inverted dropout keyed by fmix32(drop_prefix ^ (row*N+col))
    uint32_t drop_prefix = 0, drop_thr = 0;
    float drop_scale = 1.f;
    // optional: column partials (sum, sum of squares) of the stored output, one per M tile: [tiles][2][Cout] floats --
    // the BatchNorm batch statistics computed in the producing conv's epilogue.  Needs room for cdiv(M, 64) tiles.
    float* stats = nullptr;
};

// Y[m][n] = sum_k im2col(X)[m][k] * Wt[n][k]  (+ epilogue).  Cin must be a power of two >= 16.
// optional start/stop events.  ext: filled with the kernel's own begin/end by hipExtLaunchKernelGGL
// (exact even with other streams in flight); !ext: plain hipEventRecord pair around the launch
// (what works under rocprofv3, whose tool library crashes on ext launches in ROCm 7.2).
struct GemmTiming {
    hipEvent_t start = nullptr, stop = nullptr;
    bool ext = true;
};
// returns the instantiation code mode*1e8 + BM*100000 + BN*100 + BK of the kernel that was launched
// splitk_ws (optional, >= igemm_splitk_workspace(g) floats): lets under-filled grids split the K axis
// stats_blocks (with e.stats): receives the number of M-tile partials written, 0 when the launch was split-K (no fused statistics)
// rowtab / tab_rows (optional): the row table of THIS geometry (launch_build_rowtab), covering at least every 128-row tile
// the launch touches: the kernel then reads each row's offset / padding mask instead of deriving them
// flags_out (optional): GEMM_FLAG_* of the path the launch took (parity-coverage bookkeeping)
enum GemmFlags { GEMM_FLAG_SPLITK = 1, GEMM_FLAG_STATS = 2, GEMM_FLAG_ROWTAB = 4, GEMM_FLAG_BALANCED = 8, GEMM_FLAG_SLABS = 16 };
int launch_igemm_fwd(const float* X, const float* Wt, float* Y, const ConvGeom& g,
                     const GemmEpilogue& e, hipStream_t s, const GemmTiming* tm = nullptr,
                     float* splitk_ws = nullptr, size_t splitk_ws_floats = 0, int* stats_blocks = nullptr,
                     const void* rowtab = nullptr, int tab_rows = 0, int* flags_out = nullptr);
size_t igemm_splitk_workspace(const ConvGeom& g);
// host-only twins of the two launchers' choices (no HIP call): the instantiation code and GemmFlags a launch of this
// geometry takes -- ws_floats: split-K workspace the caller would pass (0: none); S: wgrad row slices (wgrad_slices)
int igemm_fwd_plan(const ConvGeom& g, const GemmEpilogue& e, size_t ws_floats, bool want_stats, bool have_rowtab, int* flags_out);
int igemm_wgrad_plan(const ConvGeom& g, int S, int mode, bool have_rowtab, int* flags_out);
// host-only (tests): rows the halo kernel's LDS image is sized for, the most rows any tile of this geometry spans, and the rows
// the per-thread staging slots can hold -- need <= bound <= items_cap must hold for every eligible geometry; all 0 if not eligible
void halo_rows_bound_and_need(const ConvGeom& g, int* bound, int* need, int* items_cap);
// throws when a tensor of this geometry is beyond the kernels' 32-bit BYTE offsets (buffer descriptors, row tables):
// B*H*W*Cin (+ padding bias) and M*Cout must stay below 2^29 elements
void igemm_check_range(const ConvGeom& g);
// kernel instantiation name as rocprofv3 prints it; cls 0: launch_igemm_fwd's return code, 1: launch_igemm_wgrad's
std::string gemm_kernel_name(int cls, int code);

// dWt[n][k] = sum_m dY[m][n] * im2col(X)[m][k], split over S row-slices into P[S][N][K].
int wgrad_slices(const ConvGeom& g);
// returns the instantiation code mode*1e7 + (64-row chunks ? 1e6 : 0) + BCO*1000 + BKI of the kernel that was launched
// Pbias (optional): [S][N] per-slice column sums of dY (the bias gradient), fused into the first K tile's blocks
// slab_stride: floats between consecutive slices of P and of Pbias (0 = N*K, bias slabs packed [S][N]);
// the trainer lays slices out as [S][N*K + N] so one reduction yields kernel and bias gradients.
// rowtab (optional, fp32 kernel): the layer's row table (launch_build_rowtab, tab_rows = rowtab_rows(geometry it was
// built for)) -- switches the gather to buffer loads without per-element divisions / bounds arithmetic.  It is used only
// when tab_rows covers this launch's rows rounded up to the kernel's chunk depth: 64 rows for the single-image kernel of the
// <= 64-channel tiles, which a table covering only the 32-row rounding demotes to the 32-row kernel; 32 rows otherwise.
// A table built for the full batch serves every smaller batch of the same layer.
int launch_igemm_wgrad(const float* X, const float* dY, float* P, const ConvGeom& g, int S, hipStream_t s,
                       const GemmTiming* tm = nullptr, float* Pbias = nullptr, size_t slab_stride = 0,
                       int mode = GEMM_DEFAULT, const void* rowtab = nullptr, int tab_rows = 0, int* flags_out = nullptr);
int rowtab_rows(const ConvGeom& g);                                           // entries (8 bytes each) the table needs
void launch_build_rowtab(const ConvGeom& g, void* tab, hipStream_t s);        // needs KH*KW <= 32
// out[i] = sum_s P[s][i]  (fixed order -> deterministic)
void launch_reduce_slices(const float* P, float* out, int S, int64_t n, hipStream_t s, int64_t stride = 0);
// Wd[ci][KH-1-kh][KW-1-kw][co] = W[co][kh][kw][ci]   (operand of the dgrad implicit GEMM)
void launch_flip_transpose(const float* W, float* Wd, int Cout, int KH, int KW, int Cin, hipStream_t s);
// the same for every conv layer of a net in ONE launch per train step (table rows in device memory)
struct FlipEntry { int64_t w_off, wd_off; int Cout, KH, KW, Cin; };
void launch_flip_transpose_all(const float* params, float* wd_all, const FlipEntry* table_dev, int layers, int64_t max_elems,
                               hipStream_t s);

// ---------------------------------------------------------------------------
// Device-resident step state of a candidate's training run.  Every per-step quantity a kernel needs (the batch's first
// row in the epoch permutation, the step counter that keys the dropout masks, the optimiser iteration that selects
// Adam's bias-corrected step size) is read from here, so a train step's launch sequence has NO host-side arguments
// that change from step to step and can be captured once as a hipGraph and replayed (net.hip).
// ---------------------------------------------------------------------------
struct StepState {
    long long row0;        // first row of the current batch in idx (advanced by the batch size after every step)
    unsigned step;         // global train step (dropout counter)
    unsigned iter;         // optimizer.iterations BEFORE this step's update (alpha_table[iter] is its step size)
};
void launch_step_advance(StepState* st, int batch, hipStream_t s);
// Where the rows of a batch come from: batch position b is row idx[row0 + b] (idx null: row0 + b) of a resident tensor.
// The default is "rows 0 .. B of the buffer handed in, no clamp, host arguments".
struct BatchRows {
    const int32_t* idx = nullptr;   // the epoch permutation (Keras' shuffle + batch gather, nsga_penalty.py:383, fused into the load)
    int64_t row0 = 0;               // first position of the batch in idx
    int64_t n_rows = 0;             // > 0: rows the resident tensor holds -- a gathered row is clamped into [0, n_rows) so that a
                                    // corrupt idx can never address outside it (the only producer of idx is the device
                                    // permutation; this is a fault fence)
    const StepState* st = nullptr;  // non-null: row0 (and, where a kernel draws, the step) come from the device state (graph replay)
};
// w[i] = (float)(2 * (fmix32(prefix ^ i) >> 8) - 2^24) * scale: the seeded glorot-uniform twin of oracle/rng.py; constant fill
void launch_glorot_init(float* w, int64_t n, uint32_t prefix, float scale, hipStream_t s);
void launch_fill(float* w, float v, int64_t n, hipStream_t s);

// ---------------------------------------------------------------------------
// Dense layers of the MLP head (dense.hip): M = batch rows, K = C_in (multiple of 16), N = units (any).
// One workgroup per 16x16 output tile, operands read straight from global memory in the MFMA lane layout,
// fixed-order 4-wave reduction: no split-K slabs, no flip-transposed weights, no slice reduction.
// mode GEMM_BF16 rounds both operands to bf16 (fp32 accumulation); every other mode is exact fp32.
// ---------------------------------------------------------------------------
// dropout: st == null -> mask keyed by drop_prefix; st != null -> by rng_prefix(drop_seed, drop_stream, st->step) (graph replay)
void launch_dense_fwd(const float* X, const float* W, const float* bias, float* Y, int M, int N, int K, int relu,
                      int dropout, uint32_t drop_prefix, uint32_t drop_thr, float drop_scale, int mode, hipStream_t s,
                      const StepState* st = nullptr, uint32_t drop_seed = 0, uint32_t drop_stream = 0);
// dX[m][k] = sum_n dY[m][n] W[n][k]; mask != null: dX = mask > 0 ? dX * mask_scale : 0 (ReLU / dropout backward of the layer's input)
void launch_dense_dgrad(const float* dY, const float* W, float* dX, int M, int N, int K, const float* mask, float mask_scale,
                        int mode, hipStream_t s);
// dW[n][k] = sum_m dY[m][n] X[m][k], dB[n] = sum_m dY[m][n]
void launch_dense_wgrad(const float* X, const float* dY, float* dW, float* dB, int M, int N, int K, int mode, hipStream_t s);
// both of the above in one launch (same arithmetic, bit-identical results): the trainer's backward of a hidden dense layer
void launch_dense_bwd(const float* X, const float* dY, const float* W, float* dW, float* dB, float* dX, int M, int N, int K,
                      const float* mask, float mask_scale, int mode, hipStream_t s);

// ---------------------------------------------------------------------------
// First layer (conv1.hip; C_in = 1, K = 9 or 25: too small for MFMA) -- direct conv on the VALU.
// X is the resident feature tensor [N_total, H, W]; `idx` (may be null) gathers the
// batch rows, fusing Keras' shuffle+batch gather (nsga_penalty.py:383) into the load.
// ---------------------------------------------------------------------------
// stats / stats_blocks (optional): column partials (sum, sum of squares) of the stored output, [blocks][2][Cout] -- written by the
// matrix-core form only (*stats_blocks = 0 otherwise: the caller then runs the stand-alone reduction)
void launch_conv1_fwd(const float* X, const BatchRows& rows, const float* Wt, const float* bias, float* Y, int B, int H, int W,
                      int Cout, int KS, int relu, hipStream_t s, float* stats = nullptr, int* stats_blocks = nullptr);
// Depthwise k x k convolution of the separable layers (dwconv.hip): SAME, stride 1, depth multiplier 1, no bias; NHWC fp32
// in every gemm_mode.  C a power of two in 16..512, KS in {3, 5}, B H W C < 2^29.  Wt [KS][KS][C].
// flip: the taps reversed -- the data gradient when X = dY; mask (optional, output-shaped): Y = mask > 0 ? Y : 0
void launch_dwconv_fwd(const float* X, const float* Wt, float* Y, int B, int H, int W, int C, int KS, int flip, const float* mask,
                       hipStream_t s);
// row-run slices of the weight gradient: a function of the shape alone, NOT monotone in B
int dwconv_wgrad_slices(int B, int H, int W, int C, int KS);
// P[slice][KS][KS][C]: per-slice partial weight gradients (no atomics); their fixed-order sum is the caller's
void launch_dwconv_wgrad(const float* X, const float* dY, float* P, int B, int H, int W, int C, int KS, hipStream_t s);
int conv1_wgrad_blocks(int B, int H, int W);
// P[blk][Cout*(KS*KS) + Cout]: per-block partial kernel grads then bias grads
void launch_conv1_wgrad(const float* X, const BatchRows& rows, const float* dY, float* P, int B, int H, int W, int Cout, int KS,
                        hipStream_t s);

// ---------------------------------------------------------------------------
// Train-time augmentation of the [T][F] feature patches (augment.hip; opt-in; no reference counterpart): random time shift,
// SpecAugment time / frequency masks and additive feature noise, keyed by (net seed, global train step, position in the
// batch) on the counter RNG -- the same bits on the device, in augment_row_draws on the host and in augment.py.
//   u(k)    = rng_u32(seed, STREAM_AUGMENT, step, 32 b + k),   R(u, n) = ((uint64)u n) >> 32
//   gate    : (u(0) >> 8) < floor(p 2^24), else the row is a plain copy of its source row
//   shift   : s = R(u(1), 2 S + 1) - S
//   t-mask j: w = R(u(2+2j), time_mask_max + 1), t0 = R(u(3+2j), T - w + 1)     (j < time_masks <= 4)
//   f-mask j: w = R(u(10+2j), freq_mask_max + 1), f0 = R(u(11+2j), F - w + 1)   (j < freq_masks <= 4)
//   out[b][t][f] = fill when t - s is outside [0, T) or t / f lies in a mask (output coordinates), else x[row][t - s][f],
//   plus, with noise_std > 0, (float)n * k: n = the four 16-bit halves of rng_u32(seed, STREAM_AUGMENT + 1 | + 2, step, e)
//   summed minus 131070 (Irwin-Hall, exact integer), e = (b T + t) F + f, k = (float)(noise_std sqrt(3) / 65536)
// ---------------------------------------------------------------------------
struct AugmentCfg {
    int time_shift = 0, time_masks = 0, time_mask_max = 0, freq_masks = 0, freq_mask_max = 0;
    double p = 1.0, noise_std = 0.0, fill = 0.0;
};
constexpr int AUGMENT_MAX_MASKS = 4;
constexpr int AUGMENT_DRAWS = 18;   // gate, shift, 4 x (w, t0), 4 x (w, f0)
// host-only: throws with a message naming the offending field when the config is outside the domain for [T][F] patches
void augment_check(const AugmentCfg& c, int T, int F);
// p > 0 and at least one of: a shift, a mask with a non-zero largest width, noise.  A disabled config is no config
bool augment_enabled(const AugmentCfg& c);
// the config as the kernel reads it: the doubles reduced once on the host
struct AugmentParams {
    int S = 0, time_masks = 0, time_mask_max = 0, freq_masks = 0, freq_mask_max = 0;
    uint32_t gate_thr = 0;   // floor(p 2^24)
    int noise = 0;           // noise_std > 0
    float noise_k = 0.f, fill = 0.f;
};
AugmentParams augment_params(const AugmentCfg& c);
// draws of batch position b: d[0] gate, d[1] shift, d[2 + 2j] / d[3 + 2j] width / first frame of time mask j,
// d[10 + 2j] / d[11 + 2j] width / first band of frequency mask j.  Unused masks are zero; so is everything after the
// gate of a gated-off row (it is a plain copy)
__host__ __device__ __forceinline__ uint32_t augment_range(uint32_t u, uint32_t n) { return (uint32_t)(((uint64_t)u * n) >> 32); }
__host__ __device__ __forceinline__ void augment_row_draws(const AugmentParams& a, uint32_t seed, uint32_t step, uint32_t b, int T,
                                                           int F, int32_t* d) {
    const uint32_t prefix = rng_prefix(seed, STREAM_AUGMENT, step), base = 32u * b;
    for (int k = 1; k < AUGMENT_DRAWS; ++k) d[k] = 0;
    d[0] = (fmix32(prefix ^ base) >> 8) < a.gate_thr ? 1 : 0;
    if (!d[0]) return;
    d[1] = (int32_t)augment_range(fmix32(prefix ^ (base + 1u)), 2u * (uint32_t)a.S + 1u) - a.S;
    for (int j = 0; j < a.time_masks; ++j) {
        const uint32_t w = augment_range(fmix32(prefix ^ (base + 2u + 2u * j)), (uint32_t)a.time_mask_max + 1u);
        d[2 + 2 * j] = (int32_t)w;
        d[3 + 2 * j] = (int32_t)augment_range(fmix32(prefix ^ (base + 3u + 2u * j)), (uint32_t)T - w + 1u);
    }
    for (int j = 0; j < a.freq_masks; ++j) {
        const uint32_t w = augment_range(fmix32(prefix ^ (base + 10u + 2u * j)), (uint32_t)a.freq_mask_max + 1u);
        d[10 + 2 * j] = (int32_t)w;
        d[11 + 2 * j] = (int32_t)augment_range(fmix32(prefix ^ (base + 11u + 2u * j)), (uint32_t)F - w + 1u);
    }
}
// out[B][T][F] = the augmented rows (BatchRows) of the resident tensor X, b = 0 .. B-1.  A streaming
// kernel: 16-byte loads / stores along F when F % 4 == 0 and both buffers are 16-byte aligned (a whole-frame shift keeps the
// alignment), else element by element.  rows.st != null: row0 and step are read from the device state (graph replay).
// Needs B T F < 2^32 (the noise counter) and T F < 2^30.
void launch_augment_gather(const float* X, const BatchRows& rows, float* out, int B, int T, int F, const AugmentParams& a,
                           uint32_t seed, uint32_t step, hipStream_t s);

// ---------------------------------------------------------------------------
// Soft-target training loss (loss.hip, the blend of the rows: augment.hip; opt-in; no reference counterpart, BUILD-DEFINED --
// include/cmoop.h fixes the semantics): mixup
// of two rows of a batch, label smoothing and class weights, all funnelled into cross-entropy against a dense target
// distribution t[B][C] with a per-row weight w[B].  Draws on the counter RNG, keyed like dropout and augmentation:
//   u(k) = rng_u32(seed, STREAM_MIXUP, step, 4 b + k),   R(u, n) = ((uint64)u n) >> 32
//   gate (u(0) >> 8) < floor(mixup_p 2^24);  partner q = R(u(1), B);  lam = tab[R(u(2), 1024)]
//   tab[k] = (float)Q(0.5 + (k + 0.5) / 2048), Q the quantile function of Beta(alpha, alpha): the upper half, lam in [0.5, 1]
//   a row is MIXED iff mixup is on, its gate is on, q != b and lam < 1; otherwise lam := 1, q := b
// Validation never sees any of this: evaluate / predict / the val_loss EarlyStopping monitors stay the sparse cross-entropy.
// ---------------------------------------------------------------------------
struct LossCfg {
    double label_smoothing = 0.0, mixup_alpha = 0.0, mixup_p = 1.0;
    const double* class_weight = nullptr;   // null: off; else n_class_weight values
    int n_class_weight = 0;
};
constexpr int MIXUP_TABLE = 1024;
// host-only: throws with a message naming the offending field when the config is outside the domain for `classes` classes
void loss_check(const LossCfg& c, int classes);
// eps > 0, or (alpha > 0 and p > 0), or class weights.  A disabled config is no config
bool loss_enabled(const LossCfg& c);
inline bool loss_mixup_on(const LossCfg& c) { return c.mixup_alpha > 0.0 && c.mixup_p > 0.0; }
// host-only: the lam table of Beta(alpha, alpha), evaluated in double (regularised incomplete beta by continued fraction,
// then bisection), each entry rounded once
void mixup_table(double alpha, float out[MIXUP_TABLE]);
// the config as the kernels read it; tab / cw are device pointers in a launch (host pointers in mixup_row_draws on the host)
struct MixupParams {
    int on = 0;                  // mixup on (alpha > 0 and p > 0)
    uint32_t gate_thr = 0;       // floor(mixup_p 2^24)
    const float* tab = nullptr;  // [MIXUP_TABLE], required when on
};
struct TargetParams {
    float one_minus_eps = 1.f;   // (float)(1 - eps)
    float eps_over_c = 0.f;      // (float)(eps / C)
    const float* cw = nullptr;   // [C] (float)class_weight, null: every weight 1.0f
};
TargetParams target_params(const LossCfg& c, int classes, const float* cw_dev);
// effective draws of batch position b of a batch of B rows: *gate = the gate bit (0 with mixup off), *q / *lam after the MIXED rule
__host__ __device__ __forceinline__ void mixup_row_draws(const MixupParams& m, uint32_t seed, uint32_t step, uint32_t b, uint32_t B,
                                                         int32_t* gate, int32_t* q, float* lam) {
    *gate = 0; *q = (int32_t)b; *lam = 1.0f;
    if (!m.on) return;
    const uint32_t prefix = rng_prefix(seed, STREAM_MIXUP, step), base = 4u * b;
    if (!((fmix32(prefix ^ base) >> 8) < m.gate_thr)) return;
    *gate = 1;
    const uint32_t qq = augment_range(fmix32(prefix ^ (base + 1u)), B);
    const float l = m.tab[augment_range(fmix32(prefix ^ (base + 2u)), (uint32_t)MIXUP_TABLE)];
    if (qq != b && l < 1.0f) { *q = (int32_t)qq; *lam = l; }
}
// out[B][T][F]: row b = lam x[b] + (1 - lam) x[q] (two fp32 products, one fp32 add, separately rounded) for a MIXED row,
// a plain copy (bits kept, the sign of a zero included) otherwise.  from_batch == 0: x[b] = row b of `rows` in the resident
// tensor src; from_batch != 0: x[b] = row b of the already gathered batch buffer src (rows.idx / row0 / n_rows unused).
// rows.st != null: step -- and, from_batch == 0 only, row0 -- come from the device state (graph replay).  16-byte accesses
// under launch_augment_gather's rule.  T F < 2^30.
void launch_mixup_gather(const float* src, const BatchRows& rows, int from_batch, float* out, int B, int T, int F,
                         const MixupParams& m, uint32_t seed, uint32_t step, hipStream_t s);
// t[B][C], w[B], primary[B] from the labels a = y[row(b)], c = y[row(q)] (rows through BatchRows as above), fp32,
// every operation rounded separately:  m_j = (j == a ? lam : 0) + (j == c ? mu : 0),  mu = 1 - lam (exact);
// t[b][j] = m_j (float)(1 - eps) + (float)(eps / C);  w[b] = lam cw[a] + mu cw[c] (1.0f without class weights);  primary[b] = a
void launch_soft_targets(const int32_t* labels, const BatchRows& rows, int B, int C, const MixupParams& m, const TargetParams& tp,
                         uint32_t seed, uint32_t step, float* t, float* w, int32_t* primary, hipStream_t s);
// softmax + clipped cross-entropy against dense targets (softmax_ce_kernel<CE_SOFT>): p, pc = clip(p, 1e-7, 1 - 1e-7),
// S = sum pc by the loops every instantiation of that kernel shares;  l_b = -sum_{t_j > 0} t_j (log pc_j - log S);
// acc[0] += w_b l_b;  acc[1] += (argmax z == primary[b]);
// dz_i = w_b p_i (q_i - sum_j p_j q_j) / B with q_j = gate_j (sum_j t_j / S - t_j / pc_j).  w null: 1; primary null: the
// first maximum of t[b].  One-hot t and unit w give softmax_ce_kernel<CE_SPARSE>'s bits (loss, dz, preds, correct)
void launch_softmax_ce_soft(const float* Z, const float* t, const float* w, const int32_t* primary, int B, int C, float* dZ,
                            double* acc, int32_t* preds, hipStream_t s);

// ---------------------------------------------------------------------------
// Knowledge distillation (loss.hip; opt-in; no reference counterpart, BUILD-DEFINED -- include/cmoop.h fixes the semantics): OFFLINE,
// against one device table zt[n_rows][classes] of a teacher's logits of the resident training rows, computed once and
// shared by every candidate.  The teacher saw the un-augmented, un-mixed row; a MIXED batch row blends the two teacher
// rows with the blend kernel's own draws.  Validation never sees any of this.
// ---------------------------------------------------------------------------
struct DistillCfg {
    double alpha = 0.0, temperature = 1.0;
    const float* teacher_logits = nullptr;   // [n_rows][classes] fp32, device; null: off
    int64_t n_rows = 0;
};
// host-only: throws with a message naming the offending field; n_rows is compared with n_train only when there is a table
void distill_check(const DistillCfg& c, int classes, int64_t n_train);
// alpha > 0 and a table.  A disabled config is no config
inline bool distill_enabled(const DistillCfg& c) { return c.alpha > 0.0 && c.teacher_logits != nullptr; }
// the config as the loss kernel reads it, each value rounded once from the double expression
struct DistillParams {
    float one_minus_alpha = 1.f;   // (float)(1 - alpha)
    float alpha_t = 0.f;           // (float)(alpha T)
    float alpha_t2 = 0.f;          // (float)(alpha T^2)
    float T = 1.f;                 // (float)T
};
DistillParams distill_params(const DistillCfg& c);
// q[B][C]: u = softmax(zt[row(b)] / T) -- mx = max_j z_j, e_j = expf((z_j - mx) / T), se = sum e_j over ascending j,
// u_j = e_j / se -- with row(b) of `rows` ALWAYS clamped into [0, rows.n_rows), rows.n_rows >= 1 the rows of the table (no
// "0 = no clamp" here).  Un-mixed row: q[b] = u (its bits); MIXED row (mixup_row_draws): v the same of row(partner),
// q[b][j] = lam u_j + mu v_j, two fp32 products and one add, separately rounded.  rows.st != null: row0 and step come from
// the device state (graph replay)
void launch_teacher_targets(const float* zt, const BatchRows& rows, int B, int C, float T, const MixupParams& m, uint32_t seed,
                            uint32_t step, float* q, hipStream_t s);
// softmax_ce_kernel<CE_DISTILL>: launch_softmax_ce_soft's CE_b = l_b and g_i = p_i (q'_i - dot) from z, t (the same kernel
// body) plus the tempered term against the teacher row q:
//   e_j = expf((z_j - mx) / T), seT = sum e_j, s_j = e_j / seT, ls_j = (z_j - mx) / T - log(seT) (no clipping), Qs = sum_j q_j
//   KD_b = sum_{q_j > 0} q_j (log(q_j) - ls_j);   acc[0] += w_b ((1 - alpha) CE_b + alpha T^2 KD_b).  KD_b and Qs s_i - q_i
//   are small differences of large terms that T^2 / T then scale: seT, Qs, the two logarithms, KD's sum and
//   Qs s_i - q_i are formed in double from the fp32 e_j and q_j, the latter rounded to fp32 once
//   dz_i = w_b ((1 - alpha) g_i + alpha T (Qs s_i - q_i)) / B;   acc[1] += (argmax z == primary[b])
// w / primary null as launch_softmax_ce_soft.  It reads nothing of the batch position: t, w, primary and q were built for
// the step by the two targets launches before it
void launch_softmax_ce_distill(const float* Z, const float* t, const float* w, const int32_t* primary, const float* q,
                               const DistillParams& d, int B, int C, float* dZ, double* acc, int32_t* preds, hipStream_t s);

// ---------------------------------------------------------------------------
// Per-channel reductions over the M rows of an [M][C] tensor (C % 4 == 0) and BatchNorm (bn.hip; the two output-layer
// helpers: dense.hip).
// Two-stage and order-fixed: `blocks` partials then a double-precision finalize.
// ---------------------------------------------------------------------------
int colreduce_blocks(int64_t M, int C);
// P[blk][2][C] = (sum x, sum x^2)
void launch_colstats(const float* X, float* P, int64_t M, int C, int blocks, hipStream_t s);
// P[blk][2][C] = (sum dy, sum dy*xhat), xhat = (x-mean)*invstd
void launch_bn_bwd_reduce(const float* dY, const float* X, const float* mean, const float* invstd,
                          float* P, int64_t M, int C, int blocks, hipStream_t s);
// BN train finalize: batch mean / biased var -> (mean, invstd, scale, shift), moving stats update
void launch_bn_finalize(const float* P, int blocks, int64_t M, int C, const float* gamma, const float* beta,
                        float* moving_mean, float* moving_var, float* mean, float* invstd, float* scale,
                        float* shift, float eps, float momentum, float one_minus_momentum, hipStream_t s);
// BN inference: scale/shift from the moving statistics
void launch_bn_eval_prepare(const float* gamma, const float* beta, const float* moving_mean,
                            const float* moving_var, float* scale, float* shift, int C, float eps, hipStream_t s);
// y = x*scale[c] + shift[c]  (optional ReLU)
void launch_scale_shift(const float* X, float* Y, const float* scale, const float* shift, int64_t M, int C,
                        int relu, hipStream_t s);
// BN backward apply: dgamma/dbeta from the partials (written by block 0), then
// dx = gamma*invstd*(dy - sum_dy/M - xhat*sum_dyxhat/M), optionally masked by (x > 0)
void launch_bn_bwd_apply(const float* dY, const float* X, const float* mean, const float* invstd,
                         const float* gamma, const float* P, int blocks, float* dX, float* dgamma, float* dbeta,
                         int64_t M, int C, int mask_x_pos, hipStream_t s);
// output layer helpers (C_out = classes: not a multiple of 4 / power of two)
void launch_colsum_small(const float* X, float* out, int M, int C, hipStream_t s);
void launch_dense_dgrad_small(const float* dY, const float* W, float* dX, int M, int N, int K, const float* mask,
                              float scale, hipStream_t s);
// out[c] = sum_blk P[blk][0][c]  (bias gradients)
void launch_colsum_finalize(const float* P, int blocks, int C, float* out, hipStream_t s);

// ---------------------------------------------------------------------------
// Pool / residual / GAP (elem.hip; BatchNorm + pool in one pass: bn.hip) / loss (loss.hip; the window gather: augment.hip) /
// optimiser (optim.hip)
// ---------------------------------------------------------------------------
void launch_maxpool_fwd(const float* X, float* Y, uint8_t* arg, int B, int H, int W, int C, hipStream_t s);
void launch_maxpool_bwd(const float* dY, const uint8_t* arg, const float* Y, float* dX, int B, int H, int W, int C,
                        int mask_y_pos, hipStream_t s);
// BatchNorm-apply (+ReLU) + MaxPool in one pass and the matching backward (the full-resolution normalised tensor and
// its gradient are never materialised); results bit-identical to scale_shift + maxpool_fwd / maxpool_bwd + bn_bwd_*.
void launch_bn_pool_fwd(const float* X, float* Y, uint8_t* arg, const float* scale, const float* shift, int B, int H, int W,
                        int C, int relu, hipStream_t s);
void launch_bn_pool_bwd_reduce(const float* g_pooled, const uint8_t* arg, const float* X, const float* mean, const float* invstd,
                               float* P, int B, int H, int W, int C, int blocks, hipStream_t s);
void launch_bn_pool_bwd_apply(const float* g_pooled, const uint8_t* arg, const float* X, const float* mean, const float* invstd,
                              const float* gamma, const float* P, int blocks, float* dX, float* dgamma, float* dbeta, int B,
                              int H, int W, int C, int mask_x_pos, hipStream_t s);
void launch_add_relu(const float* A, const float* Bt, float* Y, int64_t n, hipStream_t s);
void launch_gap_fwd(const float* X, float* Y, int B, int HW, int C, hipStream_t s);
void launch_gap_bwd(const float* dY, const float* X, float* dX, int B, int HW, int C, hipStream_t s);
// softmax + clipped sparse CE (+ gradient wrt logits when dZ != null) against labels[row(r)], rows through BatchRows
// (softmax_ce_kernel<CE_SPARSE>); adds into acc[0] (double: sum of per-sample losses) and acc[1] (as int64: correct); writes
// preds when non-null.
void launch_softmax_ce(const float* Z, const int32_t* labels, const BatchRows& rows, int B, int C, float* dZ, double* acc,
                       int32_t* preds, hipStream_t s);
// P[r][j] = the p softmax_ce_kernel forms for row r (same loops, same order): Model.predict
void launch_softmax_probs(const float* Z, float* P, int B, int C, hipStream_t s);
// windows w0 .. w0 + B of a feature stream [n_frames][F] (window w = rows [w hop, w hop + T)) into chunk [B][T][F]; db: the
// per-window dB reference / top_db floor first; mean / scale (device doubles [F], both or neither): the StandardScaler next
void launch_window_gather(const float* feat, float* chunk, int64_t w0, int B, int hop, int T, int F, int db, int db_ref_max,
                          float amin, float top_db, const double* mean, const double* scale, hipStream_t s);
// st != null: alpha = alpha_table[st->iter] (host-precomputed per iteration: the Keras step size in double, rounded once)
void launch_adam(float* w, const float* g, float* m, float* v, int64_t n, float alpha, float c1, float c2,
                 float eps, hipStream_t s, const StepState* st = nullptr, const float* alpha_table = nullptr);
// One optimiser launch for the whole parameter arena that ALSO finishes the weight gradients: the arena is cut into
// segments; a plain segment reads its gradient from g[], a slab segment sums the S row-slice partials its weight-gradient
// kernel left in `slab` (same fixed order as reduce_slices_kernel), stores the sum to g[] and applies Adam to it.
struct AdamSeg {
    int64_t off = 0, n = 0;        // arena range [off, off + n)
    const float* slab = nullptr;   // null: plain segment
    int64_t stride = 0;            // floats between consecutive slices
    int32_t S = 0;                 // slices
    int32_t block0 = 0;            // first workgroup of the segment
};
constexpr int ADAM_MAX_SEGS = 64;
struct AdamSegTable {
    int32_t count = 0, blocks = 0;
    AdamSeg seg[ADAM_MAX_SEGS];
};
// fills block0 / blocks from off, n, slab of the first `count` entries (segments must tile the arena in order)
void adam_segments_finalize(AdamSegTable& tab);
void launch_adam_segments(float* w, float* g, float* m, float* v, const AdamSegTable& tab, float alpha, float c1, float c2,
                          float eps, hipStream_t s, const StepState* st = nullptr, const float* alpha_table = nullptr);
// ---------------------------------------------------------------------------
// Optimiser options (optim.hip; opt-in, build-defined; include/cmoop.h fixes the semantics at cmoop_optim): a learning-rate schedule,
// decoupled weight decay, global-norm / value clipping.  A schedule alone only changes the step-size table of the fused
// launch above.  Decay or a clip take the FINISH + UPDATE path, three launches on one stream: launch_grad_finish (slab
// sums stored to g, one fp32 partial of sum g^2 per workgroup) -> launch_clip_scale (partials summed in double, the
// OptimRecord written) -> launch_adamw (clip, decay, adam_update).
// ---------------------------------------------------------------------------
constexpr int OPTIM_MAX_BOUNDARIES = 8;
struct OptimCfg {
    int schedule = 0;              // 0 constant, 1 cosine (+ linear warm-up), 2 exponential, 3 piecewise constant
    int staircase = 0, decay_mask = 0, n_boundaries = 0;
    int64_t warmup_steps = 0, decay_steps = 0;
    double warmup_start = 0, alpha = 0, decay_rate = 0;
    int64_t boundaries[OPTIM_MAX_BOUNDARIES] = {};
    double values[OPTIM_MAX_BOUNDARIES + 1] = {};
    double weight_decay = 0, global_clipnorm = 0, clipvalue = 0;
};
// host-only: throws with a message naming the offending field
void optim_check(const OptimCfg& c);
inline bool optim_finish_path(const OptimCfg& c) { return c.weight_decay > 0 || c.global_clipnorm > 0 || c.clipvalue > 0; }
inline bool optim_enabled(const OptimCfg& c) { return c.schedule != 0 || optim_finish_path(c); }
// host-only, THE place of the rates: lr(i) = base_lr f(i) in double, and the two fp32 values the kernels consume --
// (float)lr(i) (decay) and the bias-corrected step size (float)(lr(i) sqrt(1 - b2^t) / (1 - b1^t)), t = i + 1
struct OptimRates { double lr; float lr_f32, alpha_f32; };
OptimRates optim_rates(const OptimCfg& c, double base_lr, double beta1, double beta2, int64_t iteration);
// tensor kind of a parameter (one byte per arena element): decay_mask 0 decays KIND_KERNEL only; KIND_FROZEN (BatchNorm
// moving statistics) is never decayed, never in the norm, never updated
enum ParamKind : uint8_t { KIND_KERNEL = 0, KIND_TRAINABLE = 1, KIND_FROZEN = 2 };
struct OptimRecord { double sumsq; float norm, scale; };   // what launch_clip_scale leaves on the device
// g finished as launch_adam_segments finishes it (no weight moves); partials[b] = workgroup b's sum of g^2 over its
// non-frozen elements (kinds null: all trainable).  tab.blocks partials are written
void launch_grad_finish(float* g, const AdamSegTable& tab, const uint8_t* kinds, float* partials, hipStream_t s);
// rec = {sum of the partials in double, sqrt of it, clip / norm where norm > clip > 0 else exactly 1}
void launch_clip_scale(const float* partials, int n_partials, double clip, OptimRecord* rec, hipStream_t s);
struct AdamwArgs {
    float alpha, lr, c1, c2, eps;  // alpha / lr: used when st is null
    float weight_decay, clipvalue; // 0: off
    int clip_norm, decay_all;      // clip_norm: g *= rec->scale; decay_all: decay_mask 1
};
// st != null: alpha = alpha_table[st->iter], lr = lr_table[st->iter]
void launch_adamw(float* w, const float* g, float* m, float* v, const uint8_t* kinds, int64_t n, const OptimRecord* rec,
                  const AdamwArgs& a, hipStream_t s, const StepState* st = nullptr, const float* alpha_table = nullptr,
                  const float* lr_table = nullptr);
// ---------------------------------------------------------------------------
// Weight EMA (optim.hip; opt-in, build-defined; include/cmoop.h fixes the semantics at cmoop_ema): an average arena a in the parameter
// arena's layout, advanced by ONE launch after the optimiser's launch(es) of a step.  The optimiser kernels are untouched.
// ---------------------------------------------------------------------------
struct EmaCfg {
    double momentum = 0;           // m, 0 <= m < 1; 0 = off
    int warmup = 0, reserved = 0;  // warmup 1: m(i) = min(m, (1 + i) / (10 + i))
};
// host-only: throws with a message naming the offending field
void ema_check(const EmaCfg& c);
inline bool ema_enabled(const EmaCfg& c) { return c.momentum > 0; }
// host-only, THE place of the rates: m(i) in double, and the two fp32 values the kernel consumes -- (float)m(i) and
// (float)(1.0 - m(i)), the subtraction in double, each rounded once
struct EmaRates { double m; float mf, omf; };
EmaRates ema_rates(const EmaCfg& c, int64_t iteration);
struct EmaPair { float mf, omf; };   // one entry of the device-state steps' rate table
// a[i] = (mf a[i]) + (omf w[i]) for trainable elements (no fused multiply-add), a[i] = w[i] for KIND_FROZEN ones; kinds
// null: all trainable.  st != null: (mf, omf) = table[st->iter].  Writes a only
void launch_ema(float* a, const float* w, const uint8_t* kinds, int64_t n, float mf, float omf, hipStream_t s,
                const StepState* st = nullptr, const EmaPair* table = nullptr);

// ---------------------------------------------------------------------------
// Quantisation-aware training (opt-in, build-defined; include/cmoop.h fixes the semantics at cmoop_quant): symmetric,
// per-output-channel, weight-only fake quantisation of every KIND_KERNEL tensor, ONE launch for a whole arena (quant.hip).
// ---------------------------------------------------------------------------
struct QuantCfg {
    int bits = 0;                    // 0 = off, else 2 .. 8
    int objective = 0;               // 1: the evaluator ranks candidates by the quantised size (read by the host layers only)
    int reserved[2] = {0, 0};
};
// host-only: throws with a message naming the offending field
void quant_check(const QuantCfg& c);
inline bool quant_enabled(const QuantCfg& c) { return c.bits != 0; }
inline int quant_qmax(int bits) { return (1 << (bits - 1)) - 1; }
constexpr int64_t QUANT_MAX_ARENA = ((int64_t)1 << 31) - 1;   // elements: the kernel's index math is 32-bit
constexpr int QUANT_MAX_ROWS = 128;                           // tensors of one table
constexpr int QUANT_ROW_CHANNELS = 4;                         // channels per workgroup of a row tensor: one wave64 each
constexpr int QUANT_LANE_CHANNELS = 256;                      // channels per workgroup of a strided (depthwise) tensor: one lane each
// One kernel tensor: channel c holds the len elements off + c chan_stride + t elem_stride, t < len.  elem_stride == 1: a row
// tensor ([C_out][kh][kw][C_in], [out][in]: chan_stride == len), one wave per channel; else a strided one (depthwise
// [kh][kw][C]: chan_stride 1, elem_stride C), one lane per channel.  scale_off: the tensor's first scale; block0: its first workgroup
struct QuantRow { int32_t off, channels, len, chan_stride, elem_stride, scale_off, block0; };
struct QuantTable {
    std::vector<QuantRow> rows;
    int32_t blocks = 0, total_channels = 0;
    int64_t kernel_elems = 0;
};
// fills scale_off / block0 / blocks / total_channels / kernel_elems from the first five fields of every row and checks every
// row against an arena of n elements (n <= QUANT_MAX_ARENA, at most QUANT_MAX_ROWS rows, nothing past the arena)
void quant_table_finalize(QuantTable& tab, int64_t n);
// sum over the tensors of ceil(elements bits / 8) + 4 total_channels + 4 (n_params - kernel_elems)
int64_t quant_size_bytes(const QuantTable& tab, int64_t n_params, int bits);
// wq / codes / scales of every tensor of the table (rows_dev: tab.rows on the device) from w, as cmoop_quant defines them.
// codes and scales may be null.  Writes ONLY the tensors' elements of wq and codes, and tab.total_channels scales
void launch_quantize_weights(const float* w, float* wq, int8_t* codes, float* scales, const QuantTable& tab, const QuantRow* rows_dev,
                             int bits, hipStream_t s);

// ---------------------------------------------------------------------------
// Activation fake quantisation (opt-in, build-defined; include/cmoop.h fixes the semantics at cmoop_actquant): symmetric, signed,
// PER-TENSOR fake quantisation of an fp32 tensor in place, the weight quantiser's element arithmetic (quant_math.h) on one channel
// that spans the whole tensor.  Batch mode (train steps): the range is this tensor's own absmax, TWO launches (act_absmax_kernel
// leaves one partial per workgroup, act_quant_apply_kernel folds them, quantises and advances the site's record).  Tracked mode
// (inference): the range is the record's r, ONE launch.  No atomics, nothing to zero: every partial is written before it is read.
// ---------------------------------------------------------------------------
struct ActQuantCfg {
    int bits = 0;                    // 0 = off, else 2 .. 8
    float momentum = 0.99f;          // of the tracked range, in [0, 1)
    int reserved[2] = {0, 0};
};
// host-only: throws with a message naming the offending field
void actquant_check(const ActQuantCfg& c);
inline bool actquant_enabled(const ActQuantCfg& c) { return c.bits != 0; }
// the record of one site: the absmax of the last train step's tensor, the tracked range, the train steps seen (saturating)
struct ActRange { float m_b, r; int32_t count, reserved; };
// (mu, omu) = ((float)momentum, (float)(1.0 - (double)momentum)), each rounded once (as ema_rates forms an EmaPair)
EmaPair actquant_rates(float momentum);
constexpr int64_t ACT_QUANT_MAX_ELEMS = ((int64_t)1 << 31) - 1;   // the kernels' index math is 32-bit
constexpr int ACT_QUANT_MAX_BLOCKS = 1024;                        // workgroup cap: the partials one workgroup folds with one load per lane
constexpr int ACT_QUANT_BLOCK_ELEMS = 1024;                       // elements a workgroup takes per grid stride: 256 lanes x 16 bytes
// workgroups of both kernels (and partials of the first): a function of n alone
inline int act_quant_blocks(int64_t n) {
    const int64_t b = (n + ACT_QUANT_BLOCK_ELEMS - 1) / ACT_QUANT_BLOCK_ELEMS;
    return (int)(b < 1 ? 1 : (b > ACT_QUANT_MAX_BLOCKS ? ACT_QUANT_MAX_BLOCKS : b));
}
// x [n] quantised in place at `bits`.  tracked: a = rec->r, rec is only read, partials unused (may be null).  Else batch mode:
// a = absmax(x) through partials [act_quant_blocks(n)], and rec becomes {a, count == 0 ? a : (mu r) + (omu a), count + 1}.
// n == 0: nothing is launched.  codes (tracked mode only, may be null): the int8 code of every element, [n], next to x
void launch_fake_quant_act(float* x, int64_t n, int bits, bool tracked, uint32_t* partials, ActRange* rec, float mu, float omu,
                           hipStream_t s, int8_t* codes = nullptr);

// ---------------------------------------------------------------------------
// Integer inference (opt-in, build-defined; include/cmoop.h fixes the arithmetic at "Integer inference"): a conv / dense layer on
// int8 codes, exact int32 accumulation on v_mfma_i32_16x16x64_i8 and one dequantising epilogue (int8.hip).  Inference only.
// ---------------------------------------------------------------------------
// what the kernels take: Cin a multiple of 16, KS 1 / 3 / 5, stride 1 or the 1x1 stride-2 projection, 127^2 K < 2^31
bool int8_layer_ok(int Cin, int Cout, int KS, int stride);
// One matrix-core layer.  conv: y [B][OH][OW][Cout] from xq [B][H][W][Cin] and wq [Cout][KS][KS][Cin].  dense: y [M][N] from
// xq [M][K] and wq [N][K], K a multiple of 16, any N -- the 1 x 1 image of I8Layer::dense
struct I8Layer {
    bool conv;
    int B, H, W, Cin, Cout, KS, stride;
    static I8Layer dense(int M, int N, int K) { return I8Layer{false, M, 1, 1, K, N, 1, 1}; }
};
// The requantising epilogue (include/cmoop.h, "Integer inference: requantising epilogue"): the tail of the op fused into the
// launch.  bn_scale / bn_shift [Cout] (both null: no BatchNorm; one without the other: an error) are what launch_bn_eval_prepare
// left: t = fma(t, scale[c], shift[c]), then max(t, 0) under relu_after.  rec_out (required) is the record of the site written:
// y (then 16-byte aligned) receives the tracked-mode dequantised values at out_bits and codes (required, 4-byte aligned,
// [rows][Cout]) their codes.  Cout % 4 == 0.  Every element of both outputs of the B rows is written
struct I8Requant {
    const float *bn_scale, *bn_shift;
    int relu_after;
    const ActRange* rec_out;
    int out_bits;
    int8_t* codes;
};
// y fp32 from int8 xq and wq (both 16-byte aligned), s_w / bias [Cout].  rec non-null: s_x = quant_scale(rec->r, qmax(act_bits))
// read on the device (the tracked scale of the input site), else s_x.  rq null: the plain kernels (refusals under conv_fwd_i8 /
// dense_fwd_i8), else their ..._q twins (conv_fwd_i8_q / dense_fwd_i8_q).  B == 0: nothing is launched
void launch_i8_fwd(const I8Layer& L, const int8_t* xq, const int8_t* wq, float s_x, const ActRange* rec, int act_bits, const float* s_w,
                   const float* bias, float* y, int relu, const I8Requant* rq, hipStream_t s);
// Integer depthwise (include/cmoop.h, "Integer depthwise"): what launch_dwconv_i8_fwd accepts
bool int8_dw_layer_ok(int C, int KS);
// y [B][H][W][C] fp32 from xq [B][H][W][C] and wq [KS][KS][C] int8 (both 16-byte aligned), s_w [C] (16-byte aligned): SAME,
// stride 1, no bias, no activation.  rec_in as launch_i8_fwd's rec.  rec_out null: y = z, the dequantised sums; non-null:
// y is z under the tracked quantiser of that record (out_bits) and codes (may be null; 4-byte aligned) receives its codes.
// Every element of y (and of codes) of the B rows is written.  B == 0: nothing is launched
void launch_dwconv_i8_fwd(const int8_t* xq, const int8_t* wq, float s_x, const ActRange* rec_in, int act_bits, const float* s_w,
                          const ActRange* rec_out, int out_bits, float* y, int8_t* codes, int B, int H, int W, int C, int KS,
                          hipStream_t s);

// ---------------------------------------------------------------------------
// Magnitude pruning in training (opt-in, build-defined; include/cmoop.h fixes the semantics at cmoop_prune): per kernel tensor
// the k = floor(s len) elements of smallest magnitude become +0.0f, the threshold found by an exact radix select on the
// integer keys bits(w) & 0x7FFFFFFF; FOUR launches for a whole arena (prune.hip).
// ---------------------------------------------------------------------------
struct PruneCfg {
    double sparsity = 0.0;           // the final sparsity, 0 = off, else in (0, 1)
    int begin_step = 0, end_step = 0;   // the cubic ramp of prune_sparsity_at, in Adam iterations
    int objective = 0;               // 1: the evaluator ranks candidates by the pruned size (read by the host layers only)
    int skip_small = 1;              // 1: the first convolution and the depthwise kernels are copied, not pruned
};
// host-only: throws with a message naming the offending field
void prune_check(const PruneCfg& c);
inline bool prune_enabled(const PruneCfg& c) { return c.sparsity != 0.0; }
// TF-MOT's PolynomialDecay, power 3 from 0: 0 before begin_step, sparsity from end_step on (or when end_step <= begin_step),
// else sparsity (1 - (1-u)(1-u)(1-u)), u = (it - begin) / (double)(end - begin); IEEE double products only, no pow
double prune_sparsity_at(const PruneCfg& c, int64_t it);
constexpr int64_t PRUNE_MAX_ARENA = ((int64_t)1 << 31) - 1;   // elements: the kernels' index math is 32-bit
constexpr int PRUNE_MAX_ROWS = 128;                           // tensors of one table
constexpr int PRUNE_BLOCK_ELEMS = 8192;                       // elements of a tensor per workgroup
constexpr int PRUNE_BINS_TOP = 2048, PRUNE_BINS_LOW = 1024;   // the digits of the radix select: 11, 10 and 10 bits of the 31
// One kernel tensor: the len contiguous elements from off.  k: how many to prune (0: the tensor is copied; -1: floor(s len)
// at the s of the launch).  block0: its first workgroup
struct PruneRow { int32_t off, len, k, block0; };
struct PruneTable {
    std::vector<PruneRow> rows;
    int32_t blocks = 0;
    int64_t kernel_elems = 0;
};
// fills block0 / blocks / kernel_elems and checks every row against an arena of n elements (n <= PRUNE_MAX_ARENA, at most
// PRUNE_MAX_ROWS rows in arena order without overlap, k in [-1, len], nothing past the arena)
void prune_table_finalize(PruneTable& tab, int64_t n);
int32_t prune_row_k(const PruneRow& r, double s);   // the k of a row at sparsity s (host twin of the kernels' own)
// The stored bytes of a model pruned at `sparsity`: per tensor with k > 0 a ceil(len / 8) byte mask and its len - k values, 4
// bytes each or (bits in 2..8) packed ceil((len - k) bits / 8); every other tensor and parameter as size_mb (bits 0) or
// quant_size_bytes (bits 2..8, with 4 quant_channels bytes of scales) counts it.  An upper bound when keys tie at the threshold
int64_t prune_size_bytes(const PruneTable& tab, int64_t n_params, double sparsity, int bits, int64_t quant_channels);
// The select's device words for a table of `rows` tensors: histograms of the three digits and two state words per tensor.
// prune_workspace_init slices words_dev [prune_workspace_words(rows)] and zeroes it ONCE; every launch_prune_weights leaves
// hist1 / hist2 zero again, so no later call clears anything in a launch of its own
struct PruneWorkspace { uint32_t *hist1 = nullptr, *hist2 = nullptr, *hist3 = nullptr, *state = nullptr; int rows = 0; };
size_t prune_workspace_words(int rows);
void prune_workspace_init(PruneWorkspace& ws, uint32_t* words_dev, int rows, hipStream_t s);
// out := w at every element of every tensor of the table (rows_dev: tab.rows on the device), the k elements of smallest key
// (and every key tied with the k-th) as +0.0f; zeros (may be null) [rows]: how many elements of each tensor became zero.
// Writes ONLY the tensors' elements of out.  Returns the number of launches: 4, or 1 when every k is 0 (the same bytes)
int launch_prune_weights(const float* w, float* out, uint32_t* zeros, const PruneTable& tab, const PruneRow* rows_dev,
                         const PruneWorkspace& ws, double s, hipStream_t stream);

// device twin of epoch_permutation (net.h): out[rank of key_i] = i; n <= EPOCH_PERMUTATION_DEVICE_MAX (O(n^2) rank sort)
constexpr int64_t EPOCH_PERMUTATION_DEVICE_MAX = 262144;
void launch_epoch_permutation(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out, hipStream_t s);
void launch_confusion(const int32_t* y_true, const int32_t* y_pred, int64_t n, int C, int force_true_zero,
                      int64_t* cm, hipStream_t s);

// ---------------------------------------------------------------------------
// Operating-point read-out (opoint.hip; opt-in, build-defined; include/cmoop.h fixes the semantics at cmoop_opoint): per class, one-vs-rest,
// the threshold that still catches `recall` of the positives, the false positives at it, and twice the Mann-Whitney U.
// Defined in integers on the total order of the score bit patterns: three launches (keys, counts, select), no atomics.
// ---------------------------------------------------------------------------
struct OpointCfg {
    double recall = 0;               // 0 <= recall <= 1; 0 = off
    int objective = 0, reserved = 0; // objective 1: the evaluator ranks candidates by fpr_at_recall (read by the host layers only)
};
// host-only: throws with a message naming the offending field
void opoint_check(const OpointCfg& c);
inline bool opoint_enabled(const OpointCfg& c) { return c.recall > 0; }
struct OpointClass {                 // cmoop_opoint_class, 32 bytes
    int64_t u2;
    int32_t P, N, k, tp, fp;
    float thr;
};
static_assert(sizeof(OpointClass) == 32, "the select kernel writes 32-byte records");
constexpr int64_t OPOINT_MAX_ROWS = EPOCH_PERMUTATION_DEVICE_MAX;   // n^2 compares, as the device epoch permutation
constexpr int OPOINT_MAX_CLASSES = 64;
constexpr int ROC_TILE = 1024;       // rows j a workgroup of roc_counts_kernel stages in LDS per run
// throws naming the bound when (n, C) is outside 0 <= n <= OPOINT_MAX_ROWS, 1 <= C <= OPOINT_MAX_CLASSES
void opoint_check_shape(int64_t n, int C);
// key[c][i] = the order key of p[i][c] (p [n][C] row-major): b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) of its IEEE bits b
void launch_score_keys(const float* p, uint32_t* key, int64_t n, int C, hipStream_t s);
// cnt[c][i] = {ge_pos, ge_neg, gt_pos, gt_neg}: rows j with key[c][j] >= (>) key[c][i], split by y[j] == c
void launch_roc_counts(const uint32_t* key, const int32_t* y, int32_t* cnt, int64_t n, int C, hipStream_t s);
// rec[c] from key, y and cnt: one workgroup per class, every reduction in a fixed order
void launch_opoint_select(const uint32_t* key, const int32_t* y, const int32_t* cnt, int64_t n, int C, double recall,
                          OpointClass* rec, hipStream_t s);
// host-only, the float64 finish: out = {fpr_at_recall, recall_achieved, macro_auc, n_scored}, sums left to right in class order
void opoint_summary(const OpointClass* rec, int C, double out[4]);

// ---------------------------------------------------------------------------
// Audio front end (north-star addition; no reference counterpart)
// ---------------------------------------------------------------------------
constexpr int FRONTEND_MAX_MELS = 128;
struct FrontendCfg {
    int sr = 16000, n_fft = 512, win = 400, hop = 160, n_mels = 40;
    float fmin = 20.f, fmax = 7600.f, log_eps = 1e-6f;
    int scale = 0;             // 0: log(mel + log_eps) ; 1: dB, 10 log10(max(db_amin, mel)) - 10 log10(max(db_amin, ref)) ; 2: mel power
    int db_ref_max = 0;        // dB reference: 0 -> 1.0, 1 -> the clip's own largest mel power
    float db_amin = 1e-10f, top_db = 80.f;   // top_db >= 0: values below (clip maximum - top_db) are raised to it
};
// host-only: throws with a message naming the offending field when the config is outside the kernels' domain
void frontend_check(const FrontendCfg& c);
bool frontend_cfg_equal(const FrontendCfg& a, const FrontendCfg& b);
// n_fft 512, n_mels <= 64, log scale: served by logmel_kernel; everything else by logmel_ex_kernel
bool frontend_uses_fixed_kernel(const FrontendCfg& c);
int frontend_frames(const FrontendCfg& c, int n_samples);   // 1 + n_samples / hop
// host-only tables (built in double, stored as float); the sparse mel basis is band i = melw[start[i] .. + count[i]) on bins first_bin[i] ..
struct FrontendHostTables {
    std::vector<float> tw, win, melw;        // [n_fft][2] cos, -sin ; [n_fft] ; non-zero weights band after band
    std::vector<int> first_bin, count, start;
};
FrontendHostTables frontend_host_tables(const FrontendCfg& c);
struct FrontendTables;   // device-resident twiddles / window / sparse mel weights
FrontendTables* frontend_tables_create(const FrontendCfg& c);
void frontend_tables_destroy(FrontendTables* t);
void launch_logmel(const float* wav, int64_t n_clips, int n_samples, float* out, const FrontendTables* t, hipStream_t s);
// ONE recording [n_samples] -> out [T][n_mels], its frames spread over the chip in runs of frontend_stream_run frames per
// workgroup; frame f carries the bits launch_logmel gives it for the recording passed as one clip, the dB scale WITHOUT
// the clip reference / top_db floor (un-referenced 10 log10(max(db_amin, mel)))
int frontend_stream_run(int T, int compute_units);
void launch_logmel_stream(const float* wav, int64_t n_samples, float* out, const FrontendTables* t, int compute_units, hipStream_t s);
// Per-channel energy normalisation of mel power, per band over time (E = input_scale P):
//   M[t] = M[t-1] + s (E[t] - M[t-1]), M[-1] = E[0];  out[t] = (E[t] / (eps + M[t])^alpha + delta)^r - delta^r
struct PcenCfg {
    double s = 0.025, alpha = 0.98, delta = 2.0, r = 0.5, eps = 1e-6, input_scale = 1.0;
};
struct PcenParams {            // the fp32 values the kernels compute with
    float s, alpha, delta, r, eps, input_scale;
};
// host-only: throws with a message naming the offending field (0 < s <= 1, 0 <= alpha <= 1, delta >= 0, 0 < r <= 1, eps > 0,
// input_scale > 0, everything finite)
void pcen_check(const PcenCfg& c);
PcenParams pcen_params(const PcenCfg& c);
// host-only: the smoothing coefficient of a time constant, s = (sqrt(1 + 4 Tf^2) - 1) / (2 Tf^2), Tf = time_constant_s sr / hop
double pcen_smoothing(double time_constant_s, int sr, int hop);
// host-only: frames per chunk (a function of n_frames alone, at least PCEN_MIN_CHUNK) and chunks of the stream form
constexpr int PCEN_MIN_CHUNK = 64;
void pcen_stream_plan(int64_t n_frames, int* chunk, int* n_chunks);
// clip form, in place on e [n][T][F]: one thread per (clip, band) walks the frames
void launch_pcen_apply(const PcenParams& p, float* e, int64_t n, int T, int F, hipStream_t s);
// mel power of every clip (tables of a scale-2 config) and its PCEN in ONE launch; the bits of launch_logmel + launch_pcen_apply
void launch_logmel_pcen(const float* wav, int64_t n_clips, int n_samples, float* out, const FrontendTables* t, const PcenParams& p,
                        hipStream_t s);
// stream form, in place on e [T][F] of ONE recording: local pass, carry pass, apply pass (three launches).
// ws: pcen_stream_workspace_floats(T, F) floats; a_chunk = (1 - s)^chunk in double with the fp32 s.
size_t pcen_stream_workspace_floats(int T, int F);
void launch_pcen_stream(const PcenParams& p, float* e, int T, int F, float* ws, hipStream_t s);
void launch_mfcc(const float* X, float* Y, int64_t rows, int n_mels, int n_mfcc, hipStream_t s);   // DCT-II ortho along the mel axis
void launch_standardize(float* X, const double* mean, const double* scale, int64_t rows, int C, hipStream_t s);
void colstats_finalize_f64(const float* P, int blocks, int64_t M, int C, double* mean, double* scale, hipStream_t s);

// ---------------------------------------------------------------------------
// Polyphase resampler (resample.hip; north-star addition, the reference has no front end): audio at any rate -> the front
// end's rate.  y[n] = sum_i x[i] h[n down - i up + half], n_out = ceil(L up / down); include/cmoop.h fixes the semantics.
// ---------------------------------------------------------------------------
constexpr int RESAMPLE_MAX_RATE = 1024;            // 1 <= up, down
constexpr int RESAMPLE_MAX_HALF_WIDTH = 4096;      // of the designed filter, in periods of the slower rate
constexpr int RESAMPLE_MAX_TPP = 256;              // taps per output, ceil(n_taps / up)
constexpr int RESAMPLE_MAX_TILE = 512;             // outputs per workgroup
constexpr int RESAMPLE_LDS_FLOATS = 8192;          // 32 KiB: the input span a workgroup stages, at most
constexpr int RESAMPLE_LDS_BYTES = 64 * 1024;      // span and, where it fits beside it, the polyphase table: one workgroup's LDS
constexpr int RESAMPLE_CU_LDS_BYTES = 160 * 1024;  // of a compute unit: how many table-holding workgroups stay resident
constexpr int64_t RESAMPLE_MAX_ELEMS = 1ll << 36;  // n_clips * max(n_samples, n_out) stays below
constexpr int64_t RESAMPLE_MAX_GRID = 1 << 16;     // workgroups of a launch; they stride over the (row, tile) pairs
struct ResamplePlan {
    int up = 1, down = 1, n_taps = 1, half = 0, tpp = 1, tile = 1;
    int span_floats = 4, tab_stride = 1;             // LDS floats of the widest span; floats between two rows of the table
    bool tab_in_lds = false;                         // the table is copied into LDS beside the span (up > 1, both within 64 KiB)
    int64_t n_samples = 0, n_out = 0, n_tiles = 0;   // per row
};
struct ResampleSpan {                               // what the workgroup of one tile writes and stages
    int64_t out_first = 0, in_first = 0;            // in_first may be negative, in_first + in_count may pass n_samples
    int out_count = 0, in_count = 0;
};
// host-only; each throws "resample: <argument> <rule> (got ..)" outside the domain
int resample_filter_taps(int up, int down, int half_width);   // 2 half_width max(up, down) + 1
// the Kaiser-windowed sinc of scipy.signal.resample_poly, designed in double, rounded once to fp32: taps[n_taps]
void resample_filter(int up, int down, int half_width, double beta, float* taps);
// tile is a function of (up, down, n_taps) alone: min(512, (8192 - tpp - 2) up / down), whole waves from 64 on, at least 1
ResamplePlan resample_plan(int64_t n_samples, int up, int down, int n_taps);
// out_first = tile_index tile; in_first = (out_first down + half) / up - tpp + 1;
// in_count = ((out_first + out_count - 1) down + half) / up - in_first + 1
ResampleSpan resample_tile_span(const ResamplePlan& p, int64_t tile_index);
void resample_check_rows(const ResamplePlan& p, int64_t n_clips);
// [up][tab_stride], row p = the tpp taps of phase p = (n down + half) mod up in ascending input index, zero-padded
std::vector<float> resample_polyphase_table(const ResamplePlan& p, const float* taps);
void launch_resample(const float* x, int64_t n_clips, const ResamplePlan& p, const float* tab_dev, float* y, int compute_units,
                     hipStream_t s);

}  // namespace cmoop
