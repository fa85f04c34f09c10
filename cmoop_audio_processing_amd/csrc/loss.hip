// The loss stage (loss.py, distill.py): softmax cross-entropy in its three modes -- sparse labels, soft targets,
// distillation -- the kernels that build the soft and the teacher targets, the host checks of both configs and the
// mixup lam table.  One small workgroup per launch: latency-bound; fixed-order reductions.
#include "kernels.h"
#include <algorithm>
#include <cmath>
#include <mutex>

namespace cmoop {

// ===========================================================================
// softmax + Keras-3 sparse_categorical_crossentropy(from_logits=False):
//   p = softmax(z); pc = clip(p, 1e-7, 1-1e-7); loss = -(log pc_y - log sum_j pc_j)
// (nsga_penalty.py:377-379 via the TF backend).  One block; rows strided over
// lanes; wavefront (shuffle) reductions for the loss / correct counters.
//
// ONE body for the three training losses (kernels.h: semantics), so that the loops they share -- the maximum, the sum, p,
// pc and S, the gradient's dot product, the fixed-order reduction -- are the same text and the promise that one-hot
// targets give the sparse loss's bits (kernels.h) cannot be broken by an edit to one of them:
//   CE_SPARSE   the label y = labels[row(r)] read through the batch-row source
//   CE_SOFT     a dense target row tg with weight w.  On a one-hot row with unit weight the only extra operations are
//               1.0f * x and x + 0.0f, so the loss, dz, the predictions and the correct count carry CE_SPARSE's bits
//   CE_DISTILL  CE_SOFT plus the tempered term: s = softmax(z / T) held as an un-clipped log-softmax against the teacher row qt
// p and pc are recomputed in every loop that needs them, never carried from one to the next.
// ===========================================================================
enum CeMode { CE_SPARSE, CE_SOFT, CE_DISTILL };

template <CeMode MODE>
__global__ __launch_bounds__(256) void softmax_ce_kernel(const float* __restrict__ Z, const int32_t* __restrict__ labels,
                                                         const int32_t* __restrict__ idx, int64_t row0,
                                                         const StepState* __restrict__ st, int64_t n_rows,
                                                         const float* __restrict__ Tg, const float* __restrict__ Wr,
                                                         const int32_t* __restrict__ primary, const float* __restrict__ Qt,
                                                         DistillParams d, int B, int C, float* __restrict__ dZ,
                                                         double* __restrict__ acc, int32_t* __restrict__ preds) {
    constexpr bool SPARSE = MODE == CE_SPARSE, DISTILL = MODE == CE_DISTILL;
    __shared__ double lsum[4];
    if constexpr (SPARSE) { if (st) row0 = st->row0; }
    __shared__ int csum[4];
    const int t = threadIdx.x;
    const float lo = 1e-7f, hi = 1.0f - 1e-7f;
    double myloss = 0.0;
    int mycorrect = 0;
    for (int r = t; r < B; r += 256) {
        const float* z = Z + (size_t)r * C;
        const float* tg = SPARSE ? nullptr : Tg + (size_t)r * C;
        const float* qt = DISTILL ? Qt + (size_t)r * C : nullptr;
        float w = 1.0f;
        int y;
        if constexpr (SPARSE) {
            y = labels[gather_row(idx, row0 + r, n_rows)];
        } else {
            if (Wr) w = Wr[r];
            if (primary) {
                y = primary[r];
            } else {                           // the first maximum of the target row
                y = 0;
                float tm = tg[0];
                for (int j = 1; j < C; ++j)
                    if (tg[j] > tm) { tm = tg[j]; y = j; }
            }
        }
        float mx = z[0];
        int am = 0;
        for (int j = 1; j < C; ++j)
            if (z[j] > mx) { mx = z[j]; am = j; }
        float se = 0.f;
        for (int j = 0; j < C; ++j) se += expf(z[j] - mx);
        float S = 0.f, Tsum = 0.f, pyc = 1.f;
        for (int j = 0; j < C; ++j) {
            const float p = expf(z[j] - mx) / se;
            const float pc = fminf(fmaxf(p, lo), hi);
            S += pc;
            if constexpr (SPARSE) { if (j == y) pyc = pc; }
            else Tsum += tg[j];
        }
        [[maybe_unused]] double seT = 0.0, Qs = 0.0;
        if constexpr (SPARSE) {
            myloss += (double)(-(logf(pyc) - logf(S)));
        } else {
            const float logS = logf(S);
            float l = 0.f;
            for (int j = 0; j < C; ++j) {
                const float tj = tg[j];
                if (tj > 0.f) {
                    const float p = expf(z[j] - mx) / se;
                    const float pc = fminf(fmaxf(p, lo), hi);
                    l += tj * (logf(pc) - logS);
                }
            }
            if constexpr (!DISTILL) {
                myloss += (double)(w * -l);
            } else {
                // the tempered student: e_j = expf((z_j - mx) / T), seT = sum_j e_j, ls_j = (z_j - mx) / T - log seT;
                // KD = sum q_j (log q_j - ls_j).  Both KD and the gradient term Qs s_i - q_i are small differences of large
                // terms -- where distillation converges to, s = q, they vanish -- and T^2 / T scale them: the sums seT and
                // Qs, the two logarithms of KD, its sum and the difference Qs s_i - q_i are formed in double from the fp32
                // e_j and q_j.  (The device's float32 log is low on average -- tools/device_log_bias.py,
                // profiles/distill_logf_bias.txt -- and both logarithms enter KD with the same sign;
                // tests/test_gpu_distill.py holds loss sum and dZ to 8 x the error of a float32 autograd restatement.)
                for (int j = 0; j < C; ++j) {
                    seT += (double)expf((z[j] - mx) / d.T);
                    Qs += (double)qt[j];
                }
                const double logseT = log(seT);
                double kd = 0.0;
                for (int j = 0; j < C; ++j) {
                    const float qj = qt[j];
                    if (qj > 0.f) kd += (double)qj * (log((double)qj) - ((double)((z[j] - mx) / d.T) - logseT));
                }
                myloss += (double)w * ((double)(d.one_minus_alpha * -l) + (double)d.alpha_t2 * kd);
            }
        }
        mycorrect += (am == y);
        if (preds) preds[r] = am;
        if (dZ) {
            // q_j = gate_j * (1/S - [j==y]/pc_y), dense targets: gate_j * (Tsum/S - t_j/pc_j);
            // g_i = p_i * (q_i - sum_j p_j q_j); dz_i = g_i / B, times w, distill: w ((1 - alpha) g_i + alpha T (Qs s_i - q_i)) / B
            auto q_of = [&](int j, float p) -> float {
                [[maybe_unused]] const float pc = fminf(fmaxf(p, lo), hi);
                const float gate = (p >= lo && p <= hi) ? 1.f : 0.f;
                if constexpr (SPARSE) return gate * (1.f / S - (j == y ? 1.f / pyc : 0.f));
                else return gate * (Tsum / S - tg[j] / pc);
            };
            float dot = 0.f;
            for (int j = 0; j < C; ++j) {
                const float p = expf(z[j] - mx) / se;
                dot += p * q_of(j, p);
            }
            const float invB = 1.f / (float)B;
            [[maybe_unused]] const double rseT = DISTILL ? 1.0 / seT : 0.0;
            for (int j = 0; j < C; ++j) {
                const float p = expf(z[j] - mx) / se;
                const float qj = q_of(j, p);
                if constexpr (SPARSE) {
                    dZ[(size_t)r * C + j] = p * (qj - dot) * invB;
                } else if constexpr (!DISTILL) {
                    dZ[(size_t)r * C + j] = w * (p * (qj - dot) * invB);
                } else {
                    const float g = p * (qj - dot);
                    const float kg = (float)(Qs * ((double)expf((z[j] - mx) / d.T) * rseT) - (double)qt[j]);   // Qs s_j - q_j
                    dZ[(size_t)r * C + j] = w * ((d.one_minus_alpha * g + d.alpha_t * kg) * invB);
                }
            }
        }
    }
    // wavefront reduction (fixed butterfly order: deterministic), then the four wave sums in wave order
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        myloss += __shfl_xor(myloss, off, 64);
        mycorrect += __shfl_xor(mycorrect, off, 64);
    }
    if ((t & 63) == 0) { lsum[t >> 6] = myloss; csum[t >> 6] = mycorrect; }
    __syncthreads();
    if (t == 0 && acc) {
        acc[0] += ((lsum[0] + lsum[1]) + lsum[2]) + lsum[3];
        reinterpret_cast<long long*>(acc)[1] += (csum[0] + csum[1]) + (csum[2] + csum[3]);
    }
}

void launch_softmax_ce(const float* Z, const int32_t* labels, const BatchRows& rows, int B, int C, float* dZ, double* acc,
                       int32_t* preds, hipStream_t s) {
    if (B == 0) return;
    hipLaunchKernelGGL(softmax_ce_kernel<CE_SPARSE>, dim3(1), dim3(256), 0, s, Z, labels, rows.idx, rows.row0, rows.st, rows.n_rows,
                       nullptr, nullptr, nullptr, nullptr, DistillParams(), B, C, dZ, acc, preds);
    CMOOP_HIP(hipGetLastError());
}

// Model.predict: the probabilities softmax_ce_kernel forms and discards.  One thread per row; the same serial loops in
// the same order (maximum, sum over ascending j, expf(z_j - max) / sum), so p is bit-equal to the p behind the loss and
// the row's arg max is the prediction evaluate returns.  C <= a few dozen floats per row: the pass is launch-bound.
__global__ __launch_bounds__(256) void softmax_probs_kernel(const float* __restrict__ Z, float* __restrict__ P, int B, int C) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= B) return;
    const float* z = Z + (size_t)r * C;
    float* p = P + (size_t)r * C;
    float mx = z[0];
    for (int j = 1; j < C; ++j)
        if (z[j] > mx) mx = z[j];
    float se = 0.f;
    for (int j = 0; j < C; ++j) se += expf(z[j] - mx);
    for (int j = 0; j < C; ++j) p[j] = expf(z[j] - mx) / se;
}

void launch_softmax_probs(const float* Z, float* P, int B, int C, hipStream_t s) {
    if (B == 0) return;
    hipLaunchKernelGGL(softmax_probs_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, Z, P, B, C);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// Soft-target training loss (kernels.h: semantics): the dense targets / row weights, and cross-entropy against them
// (the mixup blend of the two batch rows is mixup_gather_kernel, augment.hip).
// ===========================================================================
// One thread per batch row: the row's draw, its two labels, then C targets.  A label outside [0, C) matches no class (its
// share of the target is dropped, as the sparse kernel's comparison drops it) and reads the weight of the nearest class
__global__ __launch_bounds__(256) void soft_targets_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ idx,
                                                           int64_t row0, int B, int C, MixupParams m, TargetParams tp, uint32_t seed,
                                                           uint32_t step, float* __restrict__ T, float* __restrict__ W,
                                                           int32_t* __restrict__ primary, const StepState* __restrict__ st,
                                                           int64_t n_rows) {
#pragma clang fp contract(off)
    if (st) { row0 = st->row0; step = st->step; }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int32_t gate, q;
    float lam;
    mixup_row_draws(m, seed, step, (uint32_t)b, (uint32_t)B, &gate, &q, &lam);
    const float mu = 1.0f - lam;
    const int a = labels[gather_row(idx, row0 + b, n_rows)];
    const int c = q == b ? a : labels[gather_row(idx, row0 + q, n_rows)];
    float* t = T + (size_t)b * C;
    for (int j = 0; j < C; ++j) {
        const float mj = (j == a ? lam : 0.f) + (j == c ? mu : 0.f);
        const float sc = mj * tp.one_minus_eps;
        t[j] = sc + tp.eps_over_c;
    }
    float w = 1.0f;
    if (tp.cw) {
        const float wa = lam * tp.cw[min(max(a, 0), C - 1)];
        const float wc = mu * tp.cw[min(max(c, 0), C - 1)];
        w = wa + wc;
    }
    W[b] = w;
    primary[b] = a;
}

void launch_soft_targets(const int32_t* labels, const BatchRows& rows, int B, int C, const MixupParams& m, const TargetParams& tp,
                         uint32_t seed, uint32_t step, float* t, float* w, int32_t* primary, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && labels && t && w && primary, "soft targets: bad arguments");
    CMOOP_REQUIRE(!m.on || m.tab != nullptr, "soft targets: the lam table is missing");
    hipLaunchKernelGGL(soft_targets_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, labels, rows.idx, rows.row0, B, C, m, tp, seed, step,
                       t, w, primary, rows.st, rows.n_rows);
    CMOOP_HIP(hipGetLastError());
}

void launch_softmax_ce_soft(const float* Z, const float* t, const float* w, const int32_t* primary, int B, int C, float* dZ,
                            double* acc, int32_t* preds, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && Z && t, "softmax_ce_soft: bad arguments");
    hipLaunchKernelGGL(softmax_ce_kernel<CE_SOFT>, dim3(1), dim3(256), 0, s, Z, nullptr, nullptr, 0, nullptr, 0, t, w, primary, nullptr,
                       DistillParams(), B, C, dZ, acc, preds);
    CMOOP_HIP(hipGetLastError());
}

// ===========================================================================
// Knowledge distillation (kernels.h: semantics): the tempered teacher rows of a batch, and the loss against them.
// ===========================================================================
// One thread per batch row, as soft_targets_kernel: the row's draw, then max-subtracted softmax(zt[row] / T) with serial
// loops in class order -- a row's result depends on its own logits (and its partner's) only, never on the batch or its
// position in it.  An un-mixed row stores u's bits; a MIXED one lam u_j + mu v_j, two products and one add, no contraction
__global__ __launch_bounds__(256) void teacher_targets_kernel(const float* __restrict__ Zt, const int32_t* __restrict__ idx,
                                                              int64_t row0, int64_t n_rows, int B, int C, float T, MixupParams m,
                                                              uint32_t seed, uint32_t step, float* __restrict__ Q,
                                                              const StepState* __restrict__ st) {
#pragma clang fp contract(off)
    if (st) { row0 = st->row0; step = st->step; }
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= B) return;
    int32_t gate, p;
    float lam;
    mixup_row_draws(m, seed, step, (uint32_t)b, (uint32_t)B, &gate, &p, &lam);
    const float mu = 1.0f - lam;
    const float* zu = Zt + gather_row(idx, row0 + b, n_rows) * (int64_t)C;
    float* q = Q + (size_t)b * C;
    float mxu = zu[0];
    for (int j = 1; j < C; ++j)
        if (zu[j] > mxu) mxu = zu[j];
    float seu = 0.f;
    for (int j = 0; j < C; ++j) seu += expf((zu[j] - mxu) / T);
    if (p == b) {
        for (int j = 0; j < C; ++j) q[j] = expf((zu[j] - mxu) / T) / seu;
        return;
    }
    const float* zv = Zt + gather_row(idx, row0 + p, n_rows) * (int64_t)C;
    float mxv = zv[0];
    for (int j = 1; j < C; ++j)
        if (zv[j] > mxv) mxv = zv[j];
    float sev = 0.f;
    for (int j = 0; j < C; ++j) sev += expf((zv[j] - mxv) / T);
    for (int j = 0; j < C; ++j) {
        const float u = expf((zu[j] - mxu) / T) / seu;
        const float v = expf((zv[j] - mxv) / T) / sev;
        const float a = lam * u;
        const float c = mu * v;
        q[j] = a + c;
    }
}

void launch_teacher_targets(const float* zt, const BatchRows& rows, int B, int C, float T, const MixupParams& m, uint32_t seed,
                            uint32_t step, float* q, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && rows.n_rows >= 1 && zt && q, "teacher targets: bad arguments");
    CMOOP_REQUIRE(T >= 1.0f && T <= 64.0f, "teacher targets: temperature must be in [1, 64]");
    CMOOP_REQUIRE(!m.on || m.tab != nullptr, "teacher targets: the lam table is missing");
    hipLaunchKernelGGL(teacher_targets_kernel, dim3(cdiv(B, 256)), dim3(256), 0, s, zt, rows.idx, rows.row0, rows.n_rows, B, C, T, m, seed,
                       step, q, rows.st);
    CMOOP_HIP(hipGetLastError());
}

void launch_softmax_ce_distill(const float* Z, const float* t, const float* w, const int32_t* primary, const float* q,
                               const DistillParams& d, int B, int C, float* dZ, double* acc, int32_t* preds, hipStream_t s) {
    if (B == 0) return;
    CMOOP_REQUIRE(B >= 1 && C >= 1 && Z && t && q, "softmax_ce_distill: bad arguments");
    CMOOP_REQUIRE(d.T >= 1.0f && d.T <= 64.0f, "softmax_ce_distill: temperature must be in [1, 64]");
    hipLaunchKernelGGL(softmax_ce_kernel<CE_DISTILL>, dim3(1), dim3(256), 0, s, Z, nullptr, nullptr, 0, nullptr, 0, t, w, primary, q, d, B, C,
                       dZ, acc, preds);
    CMOOP_HIP(hipGetLastError());
}

void distill_check(const DistillCfg& c, int classes, int64_t n_train) {
    CMOOP_REQUIRE(classes >= 1, "distill: classes must be >= 1");
    CMOOP_REQUIRE(c.alpha >= 0.0 && c.alpha <= 1.0, "distill: alpha must be in [0, 1]");   // (a NaN fails)
    CMOOP_REQUIRE(std::isfinite(c.temperature) && c.temperature >= 1.0 && c.temperature <= 64.0,
                  "distill: temperature must be finite and in [1, 64]");
    if (c.teacher_logits)
        CMOOP_REQUIRE(c.n_rows >= 1 && c.n_rows == n_train, "distill: n_rows must equal the training rows = " + std::to_string(n_train) +
                                                                " (got " + std::to_string(c.n_rows) + ")");
}

DistillParams distill_params(const DistillCfg& c) {
    DistillParams d;
    d.one_minus_alpha = (float)(1.0 - c.alpha);
    d.alpha_t = (float)(c.alpha * c.temperature);
    d.alpha_t2 = (float)(c.alpha * c.temperature * c.temperature);
    d.T = (float)c.temperature;
    return d;
}

void loss_check(const LossCfg& c, int classes) {
    CMOOP_REQUIRE(classes >= 1, "loss: classes must be >= 1");
    CMOOP_REQUIRE(c.label_smoothing >= 0.0 && c.label_smoothing < 1.0, "loss: label_smoothing must be in [0, 1)");   // (a NaN fails)
    CMOOP_REQUIRE(std::isfinite(c.mixup_alpha) && c.mixup_alpha >= 0.0 && c.mixup_alpha <= 64.0,
                  "loss: mixup_alpha must be finite and in [0, 64]");
    CMOOP_REQUIRE(c.mixup_p >= 0.0 && c.mixup_p <= 1.0, "loss: mixup_p must be in [0, 1]");
    if (c.class_weight) {
        CMOOP_REQUIRE(c.n_class_weight == classes, "loss: n_class_weight must equal classes = " + std::to_string(classes) + " (got " +
                                                       std::to_string(c.n_class_weight) + ")");
        for (int j = 0; j < classes; ++j)
            CMOOP_REQUIRE(std::isfinite(c.class_weight[j]) && c.class_weight[j] > 0.0,
                          "loss: class_weight[" + std::to_string(j) + "] must be finite and > 0");
    }
}

bool loss_enabled(const LossCfg& c) { return c.label_smoothing > 0.0 || loss_mixup_on(c) || c.class_weight != nullptr; }

TargetParams target_params(const LossCfg& c, int classes, const float* cw_dev) {
    TargetParams tp;
    tp.one_minus_eps = (float)(1.0 - c.label_smoothing);
    tp.eps_over_c = (float)(c.label_smoothing / (double)classes);
    tp.cw = c.class_weight ? cw_dev : nullptr;
    return tp;
}

// I_y(a, a) for 0 < y <= 1/2 (where the continued fraction of the incomplete beta converges fastest): modified Lentz
static double inc_beta_sym(double a, double y, double ln_beta) {
    if (y <= 0.0) return 0.0;
    const double tiny = 1e-300, b = a, qab = a + b, qap = a + 1.0, qam = a - 1.0;
    double c = 1.0, d = 1.0 - qab * y / qap;
    if (std::fabs(d) < tiny) d = tiny;
    d = 1.0 / d;
    double h = d;
    for (int m = 1; m <= 1000; ++m) {
        const double m2 = 2.0 * m;
        double aa = m * (b - m) * y / ((qam + m2) * (a + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        h *= d * c;
        aa = -(a + m) * (qab + m) * y / ((a + m2) * (qap + m2));
        d = 1.0 + aa * d; if (std::fabs(d) < tiny) d = tiny;
        c = 1.0 + aa / c; if (std::fabs(c) < tiny) c = tiny;
        d = 1.0 / d;
        const double del = d * c;
        h *= del;
        if (std::fabs(del - 1.0) < 3e-16) break;
    }
    return std::exp(a * std::log(y) + b * std::log1p(-y) - ln_beta) * h / a;
}

void mixup_table(double alpha, float out[MIXUP_TABLE]) {
    CMOOP_REQUIRE(std::isfinite(alpha) && alpha > 0.0 && alpha <= 64.0, "mixup table: alpha must be finite and in (0, 64]");
    // every candidate of a population asks for the same table: keep the last one
    static std::mutex mu;
    static double last_alpha = 0.0;
    static float last_tab[MIXUP_TABLE];
    std::lock_guard<std::mutex> lock(mu);
    if (alpha == last_alpha) { std::copy(last_tab, last_tab + MIXUP_TABLE, out); return; }
    const double ln_beta = 2.0 * std::lgamma(alpha) - std::lgamma(2.0 * alpha);
    for (int k = 0; k < MIXUP_TABLE; ++k) {
        // Q(0.5 + (k + 0.5) / 2048) = 1 - y with I_y(alpha, alpha) = 0.5 - (k + 0.5) / 2048 (symmetry), y in (0, 1/2):
        // solved on the lower tail, where the small quantiles of a small alpha keep their relative precision
        const double target = 0.5 - ((double)k + 0.5) / 2048.0;
        double ylo = 0.0, yhi = 0.5;
        for (int it = 0; it < 1200; ++it) {
            const double mid = 0.5 * (ylo + yhi);
            if (!(mid > ylo && mid < yhi)) break;
            if (inc_beta_sym(alpha, mid, ln_beta) < target) ylo = mid; else yhi = mid;
        }
        out[k] = (float)(1.0 - 0.5 * (ylo + yhi));
    }
    std::copy(out, out + MIXUP_TABLE, last_tab);
    last_alpha = alpha;
}

}  // namespace cmoop
