/* cmoop.h -- C ABI of libcmoop_hip.so: the MI355X-native population-fitness evaluator.
 *
 * This is the drop-in boundary for ONE path of sumansamui/CMOOP_Audio_Processing:
 *     compute_objectives_and_constraints(population) -> evaluate_individual(hparams)
 *       -> build_model / compile / fit / evaluate / predict / calculate_fpr / compute_model_size_mb
 * (reference nsga_penalty.py:225-442, sa_nsga_penalty.py:137-253 and their copies in
 * mobo_penalty.py and ablation_study/).  The reference is pure Python over TensorFlow;
 * it has no FFI of its own, so the functions below are what a ctypes binding of that
 * path binds (INTEGRATION.md shows the stub).  Plain pointers and sizes only: device
 * buffers are raw HIP device pointers (e.g. torch.Tensor.data_ptr()), no torch types.
 *
 * Every function returns 0 on success, non-zero on failure; cmoop_last_error() returns
 * the message of the calling thread's last failure.  The reference's own error
 * convention is "any exception kills the run" (no try/except around
 * nsga_penalty.py:383); the Python shim re-raises these codes as RuntimeError.
 */
#ifndef CMOOP_H
#define CMOOP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMOOP_ABI_VERSION 3

/* topologies hidden behind the reference's build_model(hparams) */
#define CMOOP_VARIANT_A 0 /* "deep":    nsga_penalty.py:225-334, mobo_penalty.py:128-194 */
#define CMOOP_VARIANT_B 1 /* "shallow": sa_nsga_penalty.py:137-177 and the sa_/psi_/init_ ablations */
/* the depthwise-separable search space (build-defined, no reference counterpart): A / B with every k x k stride-1 convolution
 * of C_in >= 16 replaced by a Keras-SeparableConv2D-style layer (depth multiplier 1): depthwise k x k (SAME, no bias, no
 * activation), then pointwise 1 x 1 with the bias, the ReLU and the BatchNorm role of the convolution it replaces.
 * Canonical tensors per separable layer: depthwise_kernel [k][k][C_in], pointwise_kernel [C_out][1][1][C_in], bias [C_out] */
#define CMOOP_VARIANT_A_DS 2
#define CMOOP_VARIANT_B_DS 3

/* calculate_fpr variants */
#define CMOOP_FPR_V1 0       /* nsga_penalty.py:351-364 (= sa_nsga_penalty.py:189-202) */
#define CMOOP_FPR_V1_QUIRK 1 /* V1 with y_true = argmax of an (N,1) array == zeros, nsga_penalty.py:387 */
#define CMOOP_FPR_V3 2       /* ablation_study/sa_nsga_local.py:138-141 */

/* arithmetic of the MFMA conv/dense GEMM kernels (first conv, C_in = 1, and the classifier layer are always fp32).
 * The reference trains in fp32 (TF default, no mixed-precision policy set anywhere); DEFAULT/FP32 is that.
 * BF16X3 and BF16 are opt-in: BF16X3 = fp32 operands split exactly into 3 bf16, six bf16 MFMA terms
 * (fp32-accurate); BF16 = operands rounded to bf16, fp32 accumulation (BASELINE.json configs[4] "bf16 train"). */
#define CMOOP_GEMM_DEFAULT 0 /* exact fp32 unless the environment variable CMOOP_GEMM_MODE=bf16x3|bf16 overrides */
#define CMOOP_GEMM_FP32 1  /* exact fp32 whatever the environment says: the kernel-level cmoop_dense_*_ex calls only */
#define CMOOP_GEMM_BF16X3 2
#define CMOOP_GEMM_BF16 3

/* Evaluation protocol: the module-level constants the reference's evaluate_individual
 * closes over (nsga_penalty.py:176-179) plus the Keras defaults it relies on. */
typedef struct cmoop_config {
    int32_t variant;       /* CMOOP_VARIANT_* */
    int32_t classes;       /* CLASSES           nsga_penalty.py:176 (10) / sa_nsga_penalty.py:102 (11) */
    int32_t epochs;        /* EPOCHS            :177 */
    int32_t batch;         /* BATCH_SIZE        :178 */
    int32_t patience;      /* PATIENCE          :179 */
    int32_t early_stop;    /* 1: EarlyStopping(monitor='val_loss') (:382); 0: run all epochs (throughput mode) */
    int32_t restore_best;  /* restore_best_weights: 0 in nsga_penalty.py:382, 1 in sa_nsga_penalty.py:215 */
    int32_t acc_readout;   /* 0: history['val_accuracy'][-1] (:384); 1: model.evaluate (sa_nsga_penalty.py:219) */
    int32_t fpr_variant;   /* CMOOP_FPR_* */
    int32_t shuffle;       /* Model.fit shuffle=True default */
    int32_t eval_batch;    /* rows per inference launch (results do not depend on it) */
    int32_t n_slots;       /* candidates in flight per GPU, each on its own HIP stream */
    int32_t profile_every; /* >0: HIP-event-time the MFMA GEMM launches of every n-th train step */
    int32_t gemm_mode;     /* CMOOP_GEMM_*: arithmetic of the MFMA conv/dense GEMMs (0 = library default = exact fp32) */
    double lr;             /* 1e-3: optimizer='adam' (:377); LEARNING_RATE (:162) is unused by the reference */
    double beta1, beta2, adam_eps; /* Keras Adam defaults .9 / .999 / 1e-7 */
    double bn_eps, bn_momentum;    /* Keras BatchNormalization defaults 1e-3 / .99 */
    double dropout;        /* 0.3 (nsga_penalty.py:323) */
} cmoop_config;

/* The module globals X_train, y_train, X_validation, y_validation (nsga_penalty.py:167),
 * resident in HBM: features [n, T, F] fp32 (the trailing channel axis of :151-153 is
 * implicit), labels [n] int32. */
typedef struct cmoop_dataset {
    const float* x_train;
    const int32_t* y_train;
    int64_t n_train;
    const float* x_val;
    const int32_t* y_val;
    int64_t n_val;
    int32_t T, F;
} cmoop_dataset;

int cmoop_abi_version(void);
const char* cmoop_last_error(void);
void cmoop_config_default(cmoop_config* cfg);

/* compute_model_size_mb's count_params() without building a model (nsga_penalty.py:337-344);
 * gene = {filters, kernel_size, use_bn, residual_blocks, fc_layers, use_dropout}. */
int cmoop_param_count(const int32_t gene[6], int32_t variant, int32_t classes, int64_t* out);
int cmoop_fwd_flops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, double* out);

/* compute_objectives_and_constraints' inner loop (nsga_penalty.py:426-427): evaluate n
 * candidates; outputs are host arrays of length n (any may be NULL).
 * THE POPULATION CALL.  The eleven cmoop_eval_population* symbols are ONE call, cmoop_eval_population_aq, each with fewer
 * of its arguments: next (with ctx and evaluated; NULL: the library's own longest-first queue, evaluated may then be
 * NULL too) and the nine options aug, loss, distill, optim, ema, op, q, pr, aq (cmoop_augment, cmoop_loss, cmoop_distill,
 * cmoop_optim, cmoop_ema, cmoop_opoint, cmoop_quant, cmoop_prune, cmoop_actquant below, checked in that order).  An option that is
 * NULL or disabled gives exactly -- launch for launch, bit for bit -- the call without it, so a caller may always take _aq (or _p,
 * which is _aq with aq NULL) and pass NULL for what is off. */
int cmoop_eval_population(const cmoop_config* cfg, const cmoop_dataset* ds, const int32_t* genes /* [n][6] */,
                          const uint32_t* seeds /* [n] */, int32_t n, double* acc, double* size_mb, double* fpr,
                          int32_t* epochs_run, double* val_loss, double* seconds);

/* The population call drained through a caller-supplied queue (next and evaluated required): the library's worker threads (cfg.n_slots of them,
 * concurrently) call next(ctx) for the index in [0,n) of the next candidate to train; a negative return ends that
 * worker.  Several processes (one per GPU) that share one counter therefore drain ONE longest-first queue, which
 * balances the early-stopped protocol where epochs run are unknown in advance (the reference's loop is serial,
 * nsga_penalty.py:426-427; it has no counterpart).  evaluated[i] = 1 for the candidates this call trained; the
 * other outputs of un-evaluated candidates are left untouched. */
typedef int32_t (*cmoop_next_fn)(void* ctx);
int cmoop_eval_population_pull(const cmoop_config* cfg, const cmoop_dataset* ds, const int32_t* genes /* [n][6] */,
                               const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next, void* ctx, double* acc,
                               double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss, double* seconds,
                               int32_t* evaluated /* [n], required */);

/* ---- train-time augmentation of the [T][F] feature patches (opt-in, off by default; the reference has none).
 * Keyed by (seed of the net, global train step -- the `steps` of cmoop_net_get_state, the counter that keys dropout --,
 * position b of the row inside its batch), so the same bits come out of the device, of cmoop_augment_draws and of the
 * numpy restatement in augment.py:
 *   u(k) = rng_u32(seed, 0x4000, step, 32 b + k),  R(u, n) = ((uint64)u * n) >> 32
 *   gate         the row is augmented iff (u(0) >> 8) < floor(p * 2^24), else it is a plain copy of its source row
 *   time shift   s = R(u(1), 2 time_shift + 1) - time_shift
 *   time mask j  w = R(u(2+2j), time_mask_max + 1), t0 = R(u(3+2j), T - w + 1): frames [t0, t0 + w)    (j < time_masks)
 *   freq mask j  w = R(u(10+2j), freq_mask_max + 1), f0 = R(u(11+2j), F - w + 1): bands [f0, f0 + w)   (j < freq_masks)
 *   out[b][t][f] = fill when t - s is outside [0, T) or t is in a time mask or f in a frequency mask (masks are in output
 *                  coordinates: applied after the shift), else x[row(b)][t - s][f]
 *   noise (noise_std > 0, un-filled positions of gated-on rows): + (float)n * k, two separately rounded fp32 operations;
 *                  e = (b T + t) F + f, a = rng_u32(seed, 0x4001, step, e), c = rng_u32(seed, 0x4002, step, e),
 *                  n = lo16(a) + hi16(a) + lo16(c) + hi16(c) - 131070, k = (float)(noise_std * sqrt(3) / 65536):
 *                  a 4-term Irwin-Hall variate, mean 0, standard deviation noise_std, |.| <= 3.47 noise_std
 * Domain: 0 <= p <= 1, 0 <= time_shift < T, 0 <= time_masks, freq_masks <= 4, 0 <= time_mask_max <= T,
 * 0 <= freq_mask_max <= F, noise_std >= 0 and finite, fill finite (0.0 is the feature mean after the StandardScaler).
 * A config is ENABLED iff p > 0 and it has a shift, a mask with a non-zero largest width, or noise; a disabled config
 * is the same as no config. */
typedef struct cmoop_augment {
    int32_t time_shift, time_masks, time_mask_max, freq_masks, freq_mask_max, reserved;
    double p, noise_std, fill;
} cmoop_augment;
int cmoop_augment_default(cmoop_augment* aug); /* everything off: p 1, no shift, no masks, no noise, fill 0 */
/* host-only: non-zero + a message naming the offending field when the config is outside the domain for [T][F] patches */
int cmoop_augment_check(const cmoop_augment* aug, int32_t T, int32_t F);
/* host-only: the draws of batch position b at `step`: out = gate, s, (w, t0) of the four time masks, (w, f0) of the four
 * frequency masks.  Unused masks are zero, and so is everything after the gate of a gated-off row. */
int cmoop_augment_draws(const cmoop_augment* aug, uint32_t seed, uint32_t step, int32_t b, int32_t T, int32_t F, int32_t out[18]);
/* the kernel alone, on the library stream: out_dev [B][T][F] = the augmented rows idx_dev[row0 + b] (idx_dev NULL:
 * row0 + b) of x_dev [.][T][F].  Any config of the domain, enabled or not (p = 0 is a plain gather).  B * T * F < 2^32. */
int cmoop_augment_batch(const cmoop_augment* aug, const float* x_dev, const int32_t* idx_dev /* may be NULL */, int64_t row0,
                        int32_t B, int32_t T, int32_t F, uint32_t seed, uint32_t step, float* out_dev);
/* the population call (above) with next and aug */
int cmoop_eval_population_aug(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_dataset* ds,
                              const int32_t* genes /* [n][6] */, const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next,
                              void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss,
                              double* seconds, int32_t* evaluated);

/* ---- soft-target training loss: mixup, label smoothing, class weights (opt-in, off by default).  BUILD-DEFINED: the
 * reference trains on one hard label per row, unweighted, and has no counterpart; with no loss config, or a disabled one,
 * every launch and every bit is the reference's sparse cross-entropy.
 * VALIDATION IS NEVER CHANGED: cmoop_net_evaluate / _predict / _predict_stream, the per-epoch val_loss that EarlyStopping
 * monitors and the final read-outs stay the plain sparse cross-entropy, so val_loss stays comparable between configs.
 * Draws, for batch position b of a batch of B rows (the batch actually stepped: a last partial batch draws from its own
 * size) at global train step `step` -- the counter that keys dropout and augmentation:
 *   u(k) = rng_u32(seed, 0x5000, step, 4 b + k),  R(u, n) = ((uint64)u * n) >> 32
 *   gate (u(0) >> 8) < floor(mixup_p * 2^24);  partner q = R(u(1), B);  lam = tab[R(u(2), 1024)]
 *   tab[k] = (float)Q(0.5 + (k + 0.5) / 2048), Q the quantile function of Beta(alpha, alpha), evaluated in double on the
 *            host (regularised incomplete beta by continued fraction, then bisection) and rounded once; the upper half
 *            of the symmetric distribution, i.e. lam' = max(lam, 1 - lam): lam is in [0.5, 1], a row's own label dominates
 *   a row is MIXED iff mixup is on (alpha > 0 and p > 0), its gate is on, q != b and lam < 1; otherwise lam := 1, q := b
 * Row blend, mu = 1.0f - lam (exact):  x'[b][e] = lam * x[b][e] + mu * x[q][e], two fp32 products and one fp32 add, each
 *   rounded separately; an un-mixed row is a plain copy (its bits, the sign of a zero included).  With augmentation also on,
 *   x[b] and x[q] are the already augmented rows, each augmented with its own batch position's draws.
 * Targets and weights, fp32, every operation rounded separately, a = y[row(b)], c = y[row(q)]:
 *   m_j = (j == a ? lam : 0) + (j == c ? mu : 0);   t[b][j] = m_j * (float)(1 - eps) + (float)(eps / C)
 *   w[b] = lam * cw[a] + mu * cw[c], cw = (float)class_weight[.]  (1.0f without class weights);   primary[b] = a
 * Loss: p, pc = clip(p, 1e-7, 1 - 1e-7), S = sum_j pc_j exactly as cmoop_softmax_ce forms them; then
 *   l_b = -sum over j with t_j > 0 of t_j (logf(pc_j) - logf(S));  loss sum += w_b * l_b;  correct += (argmax z == primary[b])
 *   q_j = gate_j (Tsum / S - t_j / pc_j), Tsum = sum_j t_j, gate_j = (lo <= p_j <= hi);  dz_i = w_b p_i (q_i - sum_j p_j q_j) / B
 *   (Keras' sum-over-batch-size reduction: divided by B, not by the sum of the weights).
 * With one-hot targets and unit weights the loss sum, dz, the predictions and the correct count are bit-equal to
 * cmoop_softmax_ce on the same logits.
 * Domain: 0 <= label_smoothing < 1; mixup_alpha finite, 0 <= alpha <= 64; 0 <= mixup_p <= 1; class_weight NULL or
 * n_class_weight == classes values, each finite and > 0.  A config is ENABLED iff label_smoothing > 0, or (mixup_alpha > 0
 * and mixup_p > 0), or class_weight != NULL; a disabled config is the same as no config. */
typedef struct cmoop_loss {
    double label_smoothing;      /* eps, 0 <= eps < 1; 0 = off */
    double mixup_alpha;          /* Beta(alpha, alpha); 0 = off; finite, 0 <= alpha <= 64 */
    double mixup_p;              /* probability that a row is mixed, in [0, 1] */
    const double* class_weight;  /* NULL = off, else n_class_weight values, each finite and > 0 */
    int32_t n_class_weight;      /* must equal cfg.classes when class_weight != NULL */
    int32_t reserved;
} cmoop_loss;
int cmoop_loss_default(cmoop_loss* loss); /* everything off: eps 0, alpha 0, p 1, no class weights */
/* host-only: non-zero + a message naming the offending field when the config is outside the domain for `classes` classes */
int cmoop_loss_check(const cmoop_loss* loss, int32_t classes);
/* host-only: the lam table of Beta(alpha, alpha), 0 < alpha <= 64 */
int cmoop_mixup_table(double alpha, float out[1024]);
/* host-only: the draws of a batch of B rows at `step`, AFTER the MIXED rule: gate[b] = the gate bit (0 with mixup off),
 * partner[b] = q and lam[b] of a MIXED row, else b and 1.0f.  class_weight is not read. */
int cmoop_mixup_draws(const cmoop_loss* loss, uint32_t seed, uint32_t step, int32_t B, int32_t* gate /* [B] */,
                      int32_t* partner /* [B] */, float* lam /* [B] */);
/* the blend kernel alone, on the library stream: out_dev [B][T][F], x[b] = row idx_dev[row0 + b] (idx_dev NULL: row0 + b) of
 * x_dev [.][T][F].  Any config of the domain, enabled or not (mixup off: a plain gather).  T * F < 2^30. */
int cmoop_mixup_batch(const cmoop_loss* loss, const float* x_dev, const int32_t* idx_dev /* may be NULL */, int64_t row0, int32_t B,
                      int32_t T, int32_t F, uint32_t seed, uint32_t step, float* out_dev);
/* the targets kernel alone: t_dev [B][C], w_dev [B], primary_dev [B] from labels_dev through idx_dev / row0 / n_rows as
 * cmoop_softmax_ce reads them.  Labels must lie in [0, C). */
int cmoop_soft_targets(const cmoop_loss* loss, const int32_t* labels_dev, const int32_t* idx_dev /* may be NULL */, int64_t row0,
                       int64_t n_rows, int32_t B, int32_t C, uint32_t seed, uint32_t step, float* t_dev, float* w_dev,
                       int32_t* primary_dev);
/* softmax + clipped cross-entropy of z[B][C] against the dense targets t[B][C]; w (may be NULL): row weights, 1 when NULL;
 * primary (may be NULL): the class a row counts as correct for, NULL = arg max of its target row, first maximum.  dz, acc
 * and preds as cmoop_softmax_ce */
int cmoop_softmax_ce_soft(const float* z_dev, const float* t_dev, const float* w_dev /* may be NULL */,
                          const int32_t* primary_dev /* may be NULL */, int32_t B, int32_t C, float* dz_dev /* may be NULL */,
                          double* acc_dev, int32_t* preds_dev /* may be NULL */);
/* the population call (above) with next, aug and loss */
int cmoop_eval_population_ex(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_dataset* ds,
                             const int32_t* genes /* [n][6] */, const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next,
                             void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss,
                             double* seconds, int32_t* evaluated);

/* ---- knowledge distillation: train a candidate against a teacher's tempered logits (opt-in, off by default).
 * BUILD-DEFINED: the reference has no counterpart; with no distill config, or a disabled one, every launch and every bit is
 * that of a build without it.  No accuracy gain is claimed.
 * OFFLINE: the teacher's logits of the resident training rows are computed ONCE (cmoop_net_predict_logits) into one device
 * table zt[n_rows][classes], fp32, shared by every candidate and owned by the caller for as long as anything trains on it.
 * The teacher therefore sees the un-augmented, un-mixed row: a student row that augmentation has shifted or masked is still
 * trained against the teacher's view of the clean row.  row(b) is the training row at batch position b, through the shuffle
 * index, row0 and the device step state exactly as the labels, ALWAYS clamped into [0, n_rows).
 * VALIDATION IS NEVER CHANGED, as with cmoop_loss.
 * Teacher rows, fp32:  mx = max_j z_j, e_j = expf((z_j - mx) / T), se = sum_j e_j over ascending j, u_j = e_j / se, z =
 *   zt[row(b)]: a row's u depends on its own logits and T only, never on the batch or its position in it.  With mixup on
 *   and row b MIXED (the draws of cmoop_loss: the same gate, partner and lam as the row blend and the label targets),
 *   v = the same of zt[row(partner)] and q[b][j] = lam * u_j + mu * v_j, two fp32 products and one fp32 add, each rounded
 *   separately; an un-mixed row carries u's bits.
 * Loss.  The step ALWAYS builds t / w / primary through cmoop_soft_targets' kernel (a default cmoop_loss: one-hot t, unit w,
 *   primary = label), so smoothing, mixup and class weights compose.  CE_b and g_i = p_i (q'_i - sum_j p_j q'_j) are exactly
 *   what cmoop_softmax_ce_soft forms from z, t (its l_b and, without w and / B, its dz).  With Tf = (float)T:
 *   e_j = expf((z_j - mx) / Tf), seT = sum_j e_j, s_j = e_j / seT, ls_j = (z_j - mx) / Tf - log(seT) (no clipping), Qs = sum_j q_j
 *   KD_b = sum over j with q_j > 0 of q_j (log(q_j) - ls_j).  KD_b and Qs s_i - q_i are small differences of large terms
 *   (both vanish at s = q, where distillation converges to) that T^2 and T then scale: the sums seT and Qs, the two
 *   logarithms, KD_b's sum and Qs s_i - q_i are formed in double from the fp32 e_j and q_j, the last rounded to fp32 once
 *   loss sum += w_b ((float)(1 - alpha) CE_b + (float)(alpha T^2) KD_b);   correct += (argmax z == primary[b])
 *   dz_i = w_b ((float)(1 - alpha) g_i + (float)(alpha T) (Qs s_i - q_i)) / B
 * Domain: 0 <= alpha <= 1; T finite, 1 <= T <= 64; with a table, n_rows == the training rows of the call.  A config is
 * ENABLED iff alpha > 0 and teacher_logits_dev != NULL; a disabled config is the same as no config. */
typedef struct cmoop_distill {
    double alpha;                    /* weight of the distillation term, 0 <= alpha <= 1; 0 = off */
    double temperature;              /* T, finite, 1 <= T <= 64 */
    const float* teacher_logits_dev; /* [n_rows][classes] fp32, device; NULL = off */
    int64_t n_rows;                  /* must equal the training rows of the call (ds->n_train / gather rows) */
} cmoop_distill;
int cmoop_distill_default(cmoop_distill* distill); /* off: alpha 0, T 1, no table */
/* host-only: non-zero + a message naming the offending field (alpha, temperature, n_rows) when the config is outside the
 * domain for `classes` classes and `n_train` training rows.  n_rows is only compared when there is a table. */
int cmoop_distill_check(const cmoop_distill* distill, int32_t classes, int64_t n_train);
/* the teacher-targets kernel alone, on the library stream: q_dev [B][C] from zt_dev [n_rows][C] through idx_dev / row0.
 * loss: read for the mixup draws only (NULL: no mixup). */
int cmoop_teacher_targets(const cmoop_loss* loss /* may be NULL */, const float* zt_dev, const int32_t* idx_dev /* may be NULL */,
                          int64_t row0, int64_t n_rows, int32_t B, int32_t C, double temperature, uint32_t seed, uint32_t step,
                          float* q_dev);
/* the distillation loss kernel alone: z, t, q [B][C]; w / primary / dz / preds may be NULL as in cmoop_softmax_ce_soft */
int cmoop_softmax_ce_distill(const float* z_dev, const float* t_dev, const float* w_dev /* may be NULL */,
                             const int32_t* primary_dev /* may be NULL */, const float* q_dev, double alpha, double temperature,
                             int32_t B, int32_t C, float* dz_dev /* may be NULL */, double* acc_dev, int32_t* preds_dev /* may be NULL */);
/* the population call (above) with next, aug, loss and distill */
int cmoop_eval_population_kd(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                             const cmoop_dataset* ds, const int32_t* genes /* [n][6] */, const uint32_t* seeds /* [n] */, int32_t n,
                             cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run,
                             double* val_loss, double* seconds, int32_t* evaluated);

/* ---- optimiser options: learning-rate schedule, decoupled weight decay, gradient clipping (opt-in, off by default).
 * BUILD-DEFINED: the reference builds Adam() with none of them; with no optim config, or a disabled one, every launch and every
 * bit is that of a build without it.  No accuracy gain is claimed.  i is optimizer.iterations BEFORE the update, t = i + 1.
 * Schedule: lr(i) = cfg.lr f(i), evaluated in double on the host (the formulas of Keras' CosineDecay with warm-up,
 *   ExponentialDecay and PiecewiseConstantDecay, cfg.lr as the initial rate):
 *   cosine       i < warmup_steps: f = warmup_start + (1 - warmup_start) i / warmup_steps; after it s = min(i - warmup_steps,
 *                decay_steps), f = (1 - alpha) 0.5 (1 + cos(pi s / decay_steps)) + alpha
 *   exponential  f = decay_rate ^ (i / decay_steps), the exponent floored with staircase
 *   piecewise    values[0] for i <= boundaries[0], values[k] for boundaries[k-1] < i <= boundaries[k], values[n_boundaries] after
 *   The step size stays alpha(i) = (float)(lr(i) sqrt(1 - beta2^t) / (1 - beta1^t)), in double, rounded once.
 * Per element, in Keras' order, every operation a separately rounded fp32 operation (no fused multiply-add):
 *   g = g scale                         scale = (float)(clip / norm) where norm > global_clipnorm > 0, else EXACTLY 1.0f: an
 *                                       inactive clip leaves the gradient's bits (Keras forms clip min(1 / norm, 1 / clip), which
 *                                       can leave 1 by an ulp); norm = sqrt(sum of g^2 over every trainable tensor), the sum formed
 *                                       as one fp32 partial per workgroup in a fixed order, the partials summed in double
 *   g = g < -c ? -c : (g > c ? c : g)   c = (float)clipvalue > 0 (a NaN passes)
 *   w = w - (w (float)weight_decay) (float)lr(i)      decay_mask 0: kernels only (conv, depthwise, pointwise, dense); 1: every
 *                                       trainable tensor (Keras' default)
 *   then the Adam update of cmoop_adam on the decayed weight.
 * BatchNorm moving statistics live in the parameter arena and are NOT trainable: never decayed, never in the norm, w / m / v kept.
 * Non-finite gradients propagate.  A config is ENABLED iff schedule != 0 or any of weight_decay, global_clipnorm, clipvalue > 0.
 * A schedule alone keeps the fused optimiser launch; decay or a clip take three launches (cmoop_grad_finish's two, cmoop_adamw). */
typedef struct cmoop_optim {
    double weight_decay;     /* >= 0; 0 = off */
    double global_clipnorm;  /* >= 0; 0 = off; not together with clipvalue */
    double clipvalue;        /* >= 0; 0 = off */
    double warmup_start;     /* cosine: f(0) of the linear warm-up, >= 0 */
    double alpha;            /* cosine: the floor of f, >= 0 */
    double decay_rate;       /* exponential, >= 0 */
    double values[9];        /* piecewise: n_boundaries + 1 factors, >= 0 */
    int64_t warmup_steps;    /* cosine, >= 0 */
    int64_t decay_steps;     /* cosine / exponential, >= 1 */
    int64_t boundaries[8];   /* piecewise: >= 0, strictly increasing */
    int32_t schedule;        /* 0 constant, 1 cosine, 2 exponential, 3 piecewise */
    int32_t staircase;       /* exponential: 0 / 1 */
    int32_t decay_mask;      /* 0 kernels only, 1 every trainable tensor */
    int32_t n_boundaries;    /* piecewise: 0 .. 8 */
    int32_t reserved[2];     /* 0 */
} cmoop_optim;               /* 224 bytes */
int cmoop_optim_default(cmoop_optim* optim); /* everything off: all zero */
/* host-only: non-zero + a message naming the offending field when the config is outside the domain (negative or non-finite
 * values, both clips, decay_steps < 1 where the schedule reads it, boundaries that do not increase, unknown codes) */
int cmoop_optim_check(const cmoop_optim* optim);
/* host-only, the numbers the kernels consume at `iteration`: lr(i) in double, (float)lr(i), and the step size alpha(i).
 * optim NULL: the constant schedule.  Any output may be NULL. */
int cmoop_optim_rates(const cmoop_optim* optim, const cmoop_config* cfg, int64_t iteration, double* lr, float* lr_f32, float* alpha_f32);
/* host-only: the tensor kind of every parameter of a candidate in arena order (cmoop_net_get_params), kinds[n]:
 * 0 kernel, 1 other trainable (bias, gamma, beta), 2 not trainable (BatchNorm moving mean / variance); n must be its parameter count */
int cmoop_param_kinds(const int32_t gene[6], int32_t variant, int32_t classes, uint8_t* kinds, int64_t n);
/* the population call (above) with every argument but ema: forwards to cmoop_eval_population_avg with NULL */
int cmoop_eval_population_opt(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                              const cmoop_optim* optim, const cmoop_dataset* ds, const int32_t* genes /* [n][6] */,
                              const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb,
                              double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated);

/* ---- weight EMA: an exponential moving average of the weights, read by validation, early stopping and the read-outs (opt-in,
 * off by default).  BUILD-DEFINED: the reference builds Adam() without it (Keras' use_ema=True, ema_momentum); with no ema
 * config, or a disabled one, every launch and every bit is that of a build without it.  No accuracy gain is claimed.
 * i is optimizer.iterations BEFORE the update, the counter the step-size table is indexed by.
 *   m(i) = momentum, or with warmup min(momentum, (1 + i) / (10 + i)) (TF's ExponentialMovingAverage(num_updates) rule),
 *   evaluated in double on the host; mf(i) = (float)m(i), omf(i) = (float)(1.0 - m(i)), the subtraction in double, each
 *   rounded once.  A config is ENABLED iff momentum > 0.
 * The average arena a holds one float per parameter in the parameter arena's layout.  When an enabled config is first set on
 * a net, a becomes a bit copy of the whole parameter arena at that moment; setting a config again keeps a.  After the optimiser
 * launch(es) of every train step (every step path, both optimiser paths), with w' the weight after the update:
 *   trainable element (kind 0 or 1, cmoop_param_kinds):  a' = (mf a) + (omf w')   two fp32 products and one fp32 add, each
 *                                                         rounded separately (no fused multiply-add)
 *   BatchNorm moving mean / variance (kind 2):            a' = w'                 a copy of the bits
 * so a is at all times a complete parameter set inference can run on.  Non-finite values propagate.  The training trajectory
 * is never touched: w, Adam's m / v, the gradients, dropout and the counters carry the bits of the same net without the
 * average.  One extra launch per step; the step is not captured as a graph.
 * A fit with the average on (cmoop_net_fit, the population call): every per-epoch validation pass runs on a -- the val_loss
 * EarlyStopping monitors, the history, acc_readout "last" and the predictions behind the FPR are those of a; with restore_best
 * the best-epoch snapshot is a snapshot of a.  At the end of the fit the parameter arena is overwritten (Keras'
 * finalize_variable_values) with exactly the weights that were read out: the restored best-epoch snapshot, else a of the last
 * epoch.  Adam's moments, the counters and a itself stay.  Training between validations continues on the raw weights. */
typedef struct cmoop_ema {
    double  momentum;   /* m, 0 <= m < 1, finite; 0 = off.  Keras' ema_momentum (its default is 0.99) */
    int32_t warmup;     /* 0 / 1: m(i) = min(m, (1 + i) / (10 + i)) */
    int32_t reserved;   /* 0 */
} cmoop_ema;            /* 16 bytes */
int cmoop_ema_default(cmoop_ema* ema);   /* off: all zero */
/* host-only: non-zero + a message naming the offending field (momentum, warmup, reserved) when the config is outside the domain */
int cmoop_ema_check(const cmoop_ema* ema);
/* host-only, the numbers the kernel consumes at `iteration`: m(i) in double, mf(i), omf(i).  Any output may be NULL. */
int cmoop_ema_rates(const cmoop_ema* ema, int64_t iteration, double* m, float* mf, float* omf);
/* the kernel alone on the library stream: a_dev [n] advanced against w_dev [n] at the rates of `iteration`; kinds_dev [n]
 * bytes (NULL: every element trainable).  Reads w, a and kinds, writes a only. */
int cmoop_ema_update(const cmoop_ema* ema, int64_t iteration, float* a_dev, const float* w_dev, const uint8_t* kinds_dev, int64_t n);
/* the population call (above) with every argument but the operating point: forwards to cmoop_eval_population_op with NULL, NULL */
int cmoop_eval_population_avg(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                              const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_dataset* ds, const int32_t* genes /* [n][6] */,
                              const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb,
                              double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated);

/* ---- operating-point read-out: FPR at a target recall, AUC, one threshold per class (opt-in, off by default).
 * BUILD-DEFINED: the reference scores arg-max predictions only (calculate_fpr, which stays the third objective); with no opoint
 * config, or a disabled one, every launch and every bit is that of a build without it.  The read-out only ADDS numbers: with it
 * on, acc, size_mb, fpr, epochs_run and val_loss are still the bytes of the fit without it.
 * Inputs: scores p[n][C] float32 row-major (in the trainer: cmoop_net_predict's output on the validation split with the final
 * weights), labels y[n] int32 -- always the TRUE labels; fpr_variant and its y_true quirk belong to the arg-max FPR only.
 * 1 <= C <= 64, 0 <= n <= 262144 (n^2 compares, as cmoop_epoch_permutation_device); beyond it is an error naming the bound.
 * Everything below is defined in integers and tested for equality:
 *   Order        key(s) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000), b the IEEE bits of s as uint32: a total order on bit patterns,
 *                -0 < +0, positive NaNs above +inf, negative NaNs below -inf.  No value is special-cased.
 *   One-vs-rest  row j is positive for class c iff y[j] == c; a label outside [0, C) is negative for every class.
 *                P_c = positives, N_c = n - P_c.
 *   Counts       cnt[c][i][0..3] = ge_pos, ge_neg, gt_pos, gt_neg: the rows j with key(p[j][c]) >= key(p[i][c]) that are
 *                positive, the same for negative rows, then both again with >.  Row i counts itself in ge.
 *   Per class with P_c >= 1 (a "scored" class):
 *     U2_c  = sum over positive i of 2 (N_c - ge_neg_i) + (ge_neg_i - gt_neg_i), int64: twice the Mann-Whitney U, ties at 1/2
 *     k_c   = min(P_c, max(1, (int)ceil(recall * (double)P_c))): one double product, one ceil
 *     among positives i with ge_pos_i >= k_c the one with the largest key: thr_c = its score, TP_c = its ge_pos, FP_c = its
 *     ge_neg (both counts are monotone in the key: they are the minima over that set).  A detector that fires on
 *     p[.][c] >= thr_c catches TP_c of the P_c positives and raises FP_c false alarms on these rows.
 *   A class with P_c = 0: thr = +inf, TP = FP = k = 0, U2 = 0.
 *   Summary, float64, sums left to right in class order, as double[4]:
 *     [0] fpr_at_recall    mean over scored classes of (N_c > 0 ? FP_c / N_c : 0.0); 0.0 when no class is scored
 *     [1] recall_achieved  mean over scored classes of TP_c / P_c; 0.0 when no class is scored
 *     [2] macro_auc        mean over classes with P_c >= 1 and N_c >= 1 of U2_c / (2.0 * P_c * N_c); NaN when there is none
 *     [3] n_scored
 * Domain: 0 <= recall <= 1 and finite, objective in {0, 1}, reserved 0.  A config is ENABLED iff recall > 0.  objective is read
 * by the host layers only (1: the evaluator puts fpr_at_recall in the place of the arg-max FPR); the library checks it. */
typedef struct cmoop_opoint {
    double  recall;     /* target recall per class, 0 <= recall <= 1; 0 = off */
    int32_t objective;  /* 0 / 1 */
    int32_t reserved;   /* 0 */
} cmoop_opoint;         /* 16 bytes */
typedef struct cmoop_opoint_class {
    int64_t u2;
    int32_t P, N, k, tp, fp;
    float   thr;
} cmoop_opoint_class;   /* 32 bytes */
int cmoop_opoint_default(cmoop_opoint* op);   /* off: all zero */
/* host-only: non-zero + a message naming the offending field (recall, objective, reserved) when the config is outside the domain */
int cmoop_opoint_check(const cmoop_opoint* op);
/* the key and count kernels alone, on the library stream: counts_dev [C][n][4] int32 from probs_dev [n][C] and y_dev [n] */
int cmoop_roc_counts(const float* probs_dev, const int32_t* y_dev, int64_t n, int32_t C, int32_t* counts_dev /* [C][n][4] */);
/* the three launches (keys, counts, select) on the library stream and the float64 finish: classes_host [C], summary [4].
 * Any config of the domain, enabled or not (recall 0 gives k = 1: the highest-scoring positive) */
int cmoop_operating_point(const float* probs_dev, const int32_t* y_dev, int64_t n, int32_t C, const cmoop_opoint* op,
                          cmoop_opoint_class* classes_host /* [C] */, double* summary /* [4] */);
/* average milliseconds per iteration over `iters` back-to-back iterations between two HIP events on the library stream, after 3
 * warm-up iterations each: avg_ms [4] = the three launches together, then the key, count and select launch alone.  n >= 1 */
int cmoop_operating_point_time(const float* probs_dev, const int32_t* y_dev, int64_t n, int32_t C, const cmoop_opoint* op,
                               int32_t iters, double* avg_ms /* [4] */);
/* host-only: the float64 finish alone, summary [4] from classes_host [C] */
int cmoop_opoint_summary(const cmoop_opoint_class* classes_host, int32_t C, double* summary /* [4] */);
/* the population call (above) with every argument but the quantiser: forwards to cmoop_eval_population_q with NULL, NULL.  op NULL
 * or disabled: cmoop_eval_population_avg's launches and bytes, and opoint (may be NULL) receives zeros; enabled: opoint [n][4]
 * receives every candidate's summary */
int cmoop_eval_population_op(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                             const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_dataset* ds,
                             const int32_t* genes /* [n][6] */, const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next, void* ctx,
                             double* acc, double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss, double* seconds,
                             int32_t* evaluated, double* opoint /* [n][4], may be NULL */);

/* ---- quantisation-aware training (QAT): int8 (or narrower) per-channel weights inside the train step, their size, their export
 * (opt-in, off by default).  BUILD-DEFINED: the reference trains and sizes an fp32 model and has no counterpart; with no quant
 * config, or a disabled one, every launch and every bit is that of a build without it.  No accuracy gain is claimed.
 * Symmetric, per-output-channel, WEIGHT-ONLY fake quantisation of every kernel tensor (kind 0 of cmoop_param_kinds: conv, first
 * conv, depthwise, pointwise, dense, output layer).  bits in 2..8, qmax = 2^(bits-1) - 1.
 *   Channels   a tensor stored [C_out][kh][kw][C_in] or [out][in] has one channel per leading index, its elements the contiguous
 *              row; a depthwise kernel [kh][kw][C] has one channel per c, its elements the kh kw taps at stride C.
 *   Per channel with elements w_i:
 *     a    = the float whose bits are max_i (bits(w_i) & 0x7FFFFFFF), compared as uint32: exact and order-free; a NaN outranks
 *            inf and propagates.  No value is special-cased.
 *     s    = a / (float)qmax, one correctly rounded fp32 division.
 *     if s > 0 is false (a is zero, a / qmax underflows to zero, or NaN): every code is 0 and s is stored as computed.
 *     else r_i = rintf(w_i / s): one fp32 division, then round half to even; a NaN r_i (a = inf: inf / inf) is code 0;
 *          q_i = (int8) clamp(r_i, -qmax, qmax).
 *     wq_i = (float)(int)q_i * s, one fp32 product.  A zero code gives +0.0f for every s > 0.
 *     NaNs are stored in ONE form: a scale or a product that is NaN (a NaN; 0 * inf) is stored as the quiet NaN 0x7FC00000.
 *     Non-finite weights are not a supported regime, only a deterministic one.
 *   Straight-through gradient: the gradients the backward pass forms with wq in place of w are applied unchanged to the latent
 *     fp32 w.  The absmax scale never clips (|r_i| <= qmax before the clamp for every finite row with a normal s), so there is no
 *     mask; the scale's own gradient is ignored.
 *   With an enabled config on a net: every train step first runs ONE launch that quantises the current latent kernels of the whole
 *     arena; the flip-transposed dgrad operands are built from the quantised kernels; forward and backward read kernels from the
 *     quantised copy and biases, gamma, beta and the moving statistics from the parameter arena (BatchNorm's moving-statistics
 *     writes land there).  The optimiser, Adam's moments, the EMA and the snapshots keep operating on the latent weights.  Every
 *     inference call (cmoop_net_evaluate, _predict, _predict_logits, _predict_stream) runs the launch once at its start on the arena
 *     it is about to read: the average under cmoop_net_use_ema.  A fit therefore validates, early-stops and reads out the quantised
 *     model; restore_best snapshots latent weights and the read-out re-quantises them, which is deterministic, so it is the same
 *     model.  The step is not captured as a graph.
 *   Out of scope: activations stay fp32 under this option (weight-only; cmoop_actquant below is the separate, opt-in activation
 *     quantiser); BatchNorm folding; TFLite / ONNX writers.  It composes with every gemm_mode (the bf16 bodies round wq); only
 *     fp32 is tested.
 *   Size: quant_size_bytes = sum over kernel tensors of ceil(elements * bits / 8) + 4 * (total channels) + 4 * (n_params -
 *     kernel elements).  size_mb of the population call stays count_params * 4 / 2^20; the new number is returned next to it.
 * Domain: bits in {0, 2..8}, objective in {0, 1}, reserved 0.  A config is ENABLED iff bits != 0.  objective is read by the host
 * layers only (1: the evaluator puts the quantised size in the place of size_mb); the library checks it. */
typedef struct cmoop_quant {
    int32_t bits;         /* 0 = off, else 2 .. 8 */
    int32_t objective;    /* 0 / 1 */
    int32_t reserved[2];  /* 0 */
} cmoop_quant;            /* 16 bytes */
int cmoop_quant_default(cmoop_quant* q);   /* off: all zero */
/* host-only: non-zero + a message naming the offending field (bits, objective, reserved) when the config is outside the domain */
int cmoop_quant_check(const cmoop_quant* q);
/* host-only: the kernel tensors of a candidate in arena order, rows [count][5] = {off, channels, len, chan_stride, elem_stride}:
 * channel c holds the elements off + c chan_stride + t elem_stride, t < len (row tensors: chan_stride = len, elem_stride = 1;
 * depthwise: chan_stride = 1, elem_stride = C).  cap: rows the buffer holds (an error when too small); count and total_channels
 * (the number of scales) may be NULL.  The elements covered are exactly those of kind 0 in cmoop_param_kinds. */
int cmoop_quant_table(const int32_t gene[6], int32_t variant, int32_t classes, int64_t* rows /* [cap][5] */, int32_t cap,
                      int32_t* count, int64_t* total_channels);
/* host-only: quant_size_bytes of a candidate at `bits` in 2..8 */
int cmoop_quant_size_bytes(const int32_t gene[6], int32_t variant, int32_t classes, int32_t bits, int64_t* out);
/* the kernel alone on the library stream: the tensors of rows_host [count][5] (as cmoop_quant_table gives them; at most 128 rows,
 * every one inside the arena of n < 2^31 elements, else an error) of w_dev [n] into wq_dev [n], codes_dev [n] int8 (may be NULL)
 * and scales_dev [total channels, in row order] (may be NULL).  q must be enabled.  Writes ONLY the tensors' elements of wq_dev
 * and codes_dev and exactly total-channels scales. */
int cmoop_quantize_weights(const cmoop_quant* q, const float* w_dev, int64_t n, const int64_t* rows_host /* [count][5] */,
                           int32_t count, float* wq_dev, int8_t* codes_dev, float* scales_dev);
/* average milliseconds of that launch over `iters` back-to-back launches between two HIP events on the library stream, after 3
 * warm-up launches */
int cmoop_quantize_weights_time(const cmoop_quant* q, const float* w_dev, int64_t n, const int64_t* rows_host, int32_t count,
                                float* wq_dev, int8_t* codes_dev, float* scales_dev, int32_t iters, double* avg_ms);
/* the population call (above) with every argument but the pruner: forwards to cmoop_eval_population_p with NULL, NULL.  q NULL or
 * disabled: cmoop_eval_population_op's launches and bytes, and quant (may be NULL) receives zeros; enabled: quant [n][2] receives
 * every candidate's {quant_size_bytes / 2^20, bits} */
int cmoop_eval_population_q(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                            const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_quant* q,
                            const cmoop_dataset* ds, const int32_t* genes /* [n][6] */, const uint32_t* seeds /* [n] */, int32_t n,
                            cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run,
                            double* val_loss, double* seconds, int32_t* evaluated, double* opoint /* [n][4], may be NULL */,
                            double* quant /* [n][2], may be NULL */);

/* ---- magnitude pruning in training: sparse kernels inside the train step, their size, their export (opt-in, off by default).
 * BUILD-DEFINED: the reference trains and sizes a dense model and has no counterpart; with no prune config, or a disabled one,
 * every launch and every bit is that of a build without it.  No accuracy figure is claimed.
 *   Pruned tensors   every convolution kernel after the first one ([C_out][kh][kw][C_in], the pointwise kernels of the
 *              depthwise-separable variants included) and every dense kernel ([out][in]), each as ONE tensor of len elements.
 *              The first convolution and the depthwise kernels (a small share of the parameters) are copied unchanged unless
 *              skip_small = 0.  Biases, BatchNorm and the moving statistics are never touched.
 *   The operator, per tensor, at sparsity s (a double), with no floating-point compare:
 *     key_i = bits(w_i) & 0x7FFFFFFF as uint32: a NaN outranks inf, -0.0 has key 0.
 *     k     = floor(s * len) in IEEE double.  k = 0: the tensor is copied bit for bit.
 *     else t = the k-th smallest key (1-indexed) and w_eff_i = (key_i <= t) ? +0.0f : w_i.
 *     So at least k elements are pruned, exactly k unless keys tie at t, and the result does not depend on any order.
 *     numpy: t = np.partition(keys, k-1)[k-1]; keep = keys > t.
 *   Schedule (TF-MOT's PolynomialDecay, power 3, initial sparsity 0), `it` the Adam iteration the step is about to take:
 *     s(it) = 0 for it < begin_step; s(it) = sparsity for it >= end_step or end_step <= begin_step; otherwise
 *     s(it) = sparsity * (1 - (1-u)*(1-u)*(1-u)), u = (it - begin_step) / (double)(end_step - begin_step): double products, no pow.
 *   Straight-through: every train step first prunes the latent kernels at s(it) into an effective arena (FOUR launches: an exact
 *     radix select on the keys, 11 / 10 / 10 bits, then the threshold pass; one launch when every k is 0); forward, backward and
 *     the flip-transposed dgrad operands read kernels from that arena; the gradients go unchanged to the DENSE latent fp32
 *     weights, so a pruned weight can regrow.  The optimiser, Adam's moments, the EMA, the snapshots and cmoop_net_get_params /
 *     _set_params / _get_state / _set_state see latent weights only.
 *   Inference ALWAYS prunes at the final `sparsity`, whatever the iteration: cmoop_net_evaluate, _predict, _predict_logits,
 *     _predict_stream, the operating-point pass and every validation pass of a fit prune the arena they are about to read (the
 *     average under cmoop_net_use_ema).  A fit therefore validates, early-stops and snapshots on the model it would ship if it
 *     stopped now; restore_best restores latent weights and the read-out re-prunes them, which is deterministic, so it is the
 *     same model.  CONSEQUENCE: val_loss before end_step is that of a net that has not yet adapted to its final sparsity, and
 *     early stopping sees it; choose end_step (and patience) accordingly.
 *   With cmoop_quant on as well: prune, then quantise the pruned kernels; a pruned element has code 0.
 *   The step is not captured as a graph while the option is on.
 *   Size: prune_size_bytes = per pruned tensor with k > 0 at the final sparsity ceil(len / 8) mask bytes + its (len - k) values,
 *     4 bytes each, or with the quantiser on packed ceil((len - k) * bits / 8); every other tensor and parameter as size_mb or
 *     quant_size_bytes counts it.  An upper bound on the stored model when keys tie at t.
 * Domain: sparsity 0 or in (0, 1), begin_step >= 0, end_step >= 0, objective and skip_small in {0, 1}.  A config is ENABLED iff
 * sparsity != 0.  objective is read by the host layers only (1: the evaluator puts the pruned size in the place of size_mb). */
typedef struct cmoop_prune {
    double sparsity;      /* the final sparsity; 0 = off, else in (0, 1) */
    int32_t begin_step;   /* Adam iterations */
    int32_t end_step;
    int32_t objective;    /* 0 / 1 */
    int32_t skip_small;   /* 1 (default): the first convolution and the depthwise kernels are copied */
} cmoop_prune;            /* 24 bytes */
int cmoop_prune_default(cmoop_prune* p);   /* off: all zero but skip_small = 1 */
/* host-only: non-zero + a message naming the offending field when the config is outside the domain */
int cmoop_prune_check(const cmoop_prune* p);
/* host-only: s(it) of the schedule above */
int cmoop_prune_sparsity_at(const cmoop_prune* p, int64_t it, double* out);
/* host-only: the kernel tensors of a candidate in arena order, rows [count][3] = {off, len, k}: k = -1 for a pruned tensor
 * (k = floor(s len) at the s of each call), k = 0 for a copied one.  cap: rows the buffer holds (an error when too small); count
 * may be NULL.  The elements covered are exactly those of kind 0 in cmoop_param_kinds. */
int cmoop_prune_table(const int32_t gene[6], int32_t variant, int32_t classes, int32_t skip_small, int64_t* rows /* [cap][3] */,
                      int32_t cap, int32_t* count);
/* host-only: prune_size_bytes of a candidate at `sparsity` in [0, 1) and `bits` (0: fp32 values, else 2..8) */
int cmoop_prune_size_bytes(const int32_t gene[6], int32_t variant, int32_t classes, double sparsity, int32_t bits, int32_t skip_small,
                           int64_t* out);
/* the launch sequence alone on the library stream: the tensors of rows_host [count][3] = {off, len, k} (as cmoop_prune_table
 * gives them, or with an explicit k in [0, len]; at most 128 rows in arena order without overlap, every one inside the arena of
 * n < 2^31 elements, else an error before any launch) of w_dev [n] into out_dev [n]; zeros_dev [count] uint32 (may be NULL)
 * receives how many elements of each tensor became zero; launches (may be NULL) how many launches the call made (4, or 1 when
 * every k is 0).  Writes ONLY the tensors' elements of out_dev. */
int cmoop_prune_weights(const float* w_dev, int64_t n, const int64_t* rows_host /* [count][3] */, int32_t count, double s,
                        float* out_dev, uint32_t* zeros_dev, int32_t* launches);
/* average milliseconds of that sequence over `iters` back-to-back calls between two HIP events on the library stream, after 3
 * warm-up calls */
int cmoop_prune_weights_time(const float* w_dev, int64_t n, const int64_t* rows_host, int32_t count, double s, float* out_dev,
                             uint32_t* zeros_dev, int32_t iters, double* avg_ms);
/* the population call (above) with every argument but the activation quantiser: forwards to cmoop_eval_population_aq with NULL.
 * pr NULL or disabled: cmoop_eval_population_q's
 * launches and bytes, and prune (may be NULL) receives zeros; enabled: prune [n][3] receives every candidate's
 * {prune_size_bytes / 2^20, sparsity, zero fraction of the pruned tensors of the scored model} */
int cmoop_eval_population_p(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                            const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_quant* q,
                            const cmoop_prune* pr, const cmoop_dataset* ds, const int32_t* genes /* [n][6] */,
                            const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb,
                            double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated,
                            double* opoint /* [n][4], may be NULL */, double* quant /* [n][2], may be NULL */,
                            double* prune /* [n][3], may be NULL */);

/* ---- activation fake quantisation: train and score full-int8 candidates (opt-in, off by default).  BUILD-DEFINED: the reference
 * trains and scores an fp32 model and has no counterpart; with no actquant config, or a disabled one, every launch and every bit is
 * that of a build without it.  No accuracy figure is measured or claimed.
 * Per-tensor, symmetric, signed fake quantisation of an fp32 tensor, in place.  bits in 2..8, qmax = 2^(bits-1) - 1.  The
 * arithmetic is cmoop_quant's, applied to ONE channel that spans the whole tensor, with elements x_i and a range a:
 *     s    = a / (float)qmax, one correctly rounded fp32 division.
 *     if s > 0 is false (a is zero, a / qmax underflows to zero, or NaN): every code is 0.
 *     else q_i = clamp(rintf(x_i / s), -qmax, qmax): one fp32 division, round half to even; a NaN quotient is code 0.
 *     y_i  = (float)q_i * s, one fp32 product.  NaNs are stored in ONE form, the quiet NaN 0x7FC00000.
 *   Two range modes:
 *     BATCH mode (train steps): a = m_b, the float whose bits are max_i (bits(x_i) & 0x7FFFFFFF) compared as uint32, over the B
 *       rows actually in the batch: exact and order-free.  It never clips, so the straight-through gradient needs no upper mask.
 *     TRACKED mode (every inference pass): a = r, the site's tracked range; the clamp now does real work.
 *   Tracking, on each train step, count being the number of steps the site has seen: count == 0: r = m_b; otherwise
 *     r = fl(fl(mu * r) + fl(omu * m_b)) in fp32 with no contraction, mu = (float)momentum and omu = (float)(1.0 - (double)momentum)
 *     formed on the host; a NaN m_b propagates in the canonical form.  Then count += 1 (saturating).
 *   Sites of a net: act i of the plan is a site iff i is not the input features, not the logits, is materialised (not a BatchNorm
 *     output fused into its max-pool) and is the input of at least one convolution (full, depthwise, pointwise, skip projection),
 *     dense layer or the global average pool: the operand tensors of every MAC layer and of the global pool, numbered in act
 *     order (cmoop_actquant_sites).  The forward pass quantises a site right after the launch that writes it (for a fused
 *     BatchNorm + pool: the pool's output); every consumer reads the quantised tensor.  Two launches per site per train step
 *     (absmax partials; fold + quantise + record), one per site per inference chunk.
 *   GAPS: the first layer reads the resident feature tensor, which stays untouched; the operands of the residual add + ReLU stay
 *     fp32.  Symmetric signed ranges cost one bit on ReLU outputs.  Asymmetric or unsigned ranges, per-channel activation scales,
 *     learned clipping, a quantiser fused into the producers' epilogues (but for the depthwise producer of "Integer depthwise"
 *     and the conv / dense producers of "Integer inference: requantising epilogue" below) and BatchNorm folding are out of scope (the conv and dense layers can be executed on int8 codes: "Integer
 *     inference" below).  It composes with the bf16 gemm modes, untested.
 *   The backward pass is not changed.  Weight gradients are formed with the quantised operands.  The x > 0 masks the dgrad / pool
 *     / GAP kernels already take from the layer input now read quantised values, so an element that rounds to code 0 passes no
 *     gradient, exactly as the integer model's ReLU would see it.  Everything else is straight-through.
 *   Inference with the option on is refused, with a message and before anything is launched, while no train step has run with
 *     the option on and no ranges were loaded (cmoop_net_set_act_ranges).  The restore_best snapshot of a fit carries the site
 *     records with the weights: the best-epoch model has the ranges it was validated with.  Under cmoop_net_use_ema the tracked
 *     ranges are those of the raw-weight trajectory.  Independent of cmoop_quant and cmoop_prune, and composes with both.  The
 *     step is not captured as a graph while the option is on.
 * Domain: bits in {0, 2..8}, momentum in [0, 1), reserved 0.  A config is ENABLED iff bits != 0. */
typedef struct cmoop_actquant {
    int32_t bits;         /* 0 = off, else 2 .. 8 */
    float momentum;       /* of the tracked range, in [0, 1) */
    int32_t reserved[2];  /* 0 */
} cmoop_actquant;         /* 16 bytes */
typedef struct cmoop_act_range {
    float m_b;            /* absmax of the site's tensor at the last train step */
    float r;              /* the tracked range */
    int32_t count;        /* train steps the site has seen (saturating) */
    int32_t reserved;     /* 0 */
} cmoop_act_range;        /* 16 bytes */
int cmoop_actquant_default(cmoop_actquant* aq);   /* off: bits 0, momentum 0.99 */
/* host-only: non-zero + a message naming the offending field (bits, momentum, reserved) when the config is outside the domain */
int cmoop_actquant_check(const cmoop_actquant* aq);
/* host-only: the sites of a candidate at a T x F patch in site order, rows [count][4] = {act index, H, W, C}.  cap: rows the
 * buffer holds (an error when too small); count may be NULL */
int cmoop_actquant_sites(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int32_t* rows /* [cap][4] */,
                         int32_t cap, int32_t* count);
/* the operator alone on the library stream: x_dev [n] (n < 2^31, aligned to 4 bytes) quantised in place at `bits`.  a_in NULL:
 * batch mode, and record_inout (required) advances as a site's record does under `momentum`.  a_in given: tracked mode with
 * a = *a_in; record_inout (may be NULL) is left as it is */
int cmoop_fake_quant_act(float* x_dev, int64_t n, int32_t bits, const float* a_in, cmoop_act_range* record_inout, float momentum);
/* average milliseconds of that call's launches (two in batch mode, one in tracked mode) over `iters` back-to-back repetitions
 * between two HIP events on the library stream, after 3 warm-up repetitions */
int cmoop_fake_quant_act_time(float* x_dev, int64_t n, int32_t bits, const float* a_in, float momentum, int32_t iters, double* avg_ms);

/* ---- Integer inference (opt-in, BUILD-DEFINED; off by default) ---------------------------------------------------------------------
 * THE arithmetic of an integer layer (quant.py restates it in numpy: conv_i8_ref / dense_i8_ref / act_codes_ref).  A model trained
 * under cmoop_quant and cmoop_actquant has int8 weight codes qw with one scale s_w[c] per output channel (the value the weight
 * quantiser stores) and, per site, int8 activation codes qx under the tracked-mode scale s_x = r / (float)qmax_act (the scale the
 * tracked apply kernel forms from the site's record).  For a conv / dense layer whose input is a site:
 *     acc[m][c] = sum over (kh, kw, ci) of (int32) qx[pixel(m, kh, kw)][ci] * (int32) qw[c][kh][kw][ci]     exact, in int32;
 *                 a tap in the SAME padding contributes 0
 *     y[m][c]   = fl( fl( (float)acc[m][c] * fl(s_x * s_w[c]) ) + bias[c] )                                  then ReLU if the op has it
 *   (float)acc is the correctly rounded int32 -> fp32 conversion (round to nearest even): accumulators above 2^24 occur and round
 *   there, which is part of the definition.  Every fl() is ONE correctly rounded fp32 operation, contraction off (no fma), so
 *   np.float32 arithmetic restates it bit for bit.  |acc| <= 127 * 127 * K must stay below 2^31: it does for every layer of the
 *   search space (K <= 12800: 512 -> 512, k5), and a launch asserts it from the shape.  The ReLU is the fp32 conv and dense
 *   epilogues' max(y, 0) (fmaxf): a NaN becomes 0 and a zero result is +0.0.  A scale of 0 (an all-zero channel or site: s > 0
 *   false) is legal, its codes are 0 and y = bias.
 * In a net (cmoop_net_set_int8) every OP_CONV and OP_DENSE whose input is an activation-quantisation site runs this way
 *   (cmoop_int8_ops): stride-1 convs, pointwise halves, the 1x1 stride-2 skip projections and every dense layer.  Everything else is
 *   launch for launch what it was: the first convolution (its input is no site), depthwise convolutions (unless "Integer depthwise"
 *   below is on as well) and the global pool (they keep reading the fp32 site tensor, which stays written), BatchNorm, pooling,
 *   add + ReLU, and every train step.  gemm_mode is
 *   ignored by integer ops.  Weights come through the existing weight stage (snapshots, EMA, cmoop_net_use_ema and pruning compose).
 * Kernels (int8.hip): implicit GEMM on v_mfma_i32_16x16x64_i8, Cin a multiple of 16, KS 1 / 3 / 5 at stride 1 or the 1x1 stride-2
 *   projection; 16-byte code loads, so code buffers must be 16-byte aligned.  No split-K, no atomics.
 * OUT OF SCOPE: integer BatchNorm / pool / add / GAP, BatchNorm folding, int8 outputs between layers (but for the opt-in levels
 *   below: "Integer depthwise", the second, and "Integer inference: requantising epilogue", the third), asymmetric or per-channel activation scales, training on integer kernels, the population
 *   objectives. */
/* the lone conv layer on the library stream: y_dev [B][ceil(H/stride)][ceil(W/stride)][Cout] fp32 from xq_dev [B][H][W][Cin] and
 * wq_dev [Cout][KS][KS][Cin] int8 codes (16-byte aligned), s_w_dev / bias_dev [Cout].  B == 0: success, nothing written */
int cmoop_conv_fwd_i8(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                      int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu);
/* the lone dense layer: y_dev [M][N] from xq_dev [M][K] and wq_dev [N][K]; K a multiple of 16, any N.  M == 0: success, nothing written */
int cmoop_dense_fwd_i8(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                       int32_t M, int32_t N, int32_t K, int32_t relu);
/* average milliseconds of cmoop_conv_fwd_i8's launch over `iters` back-to-back repetitions between two HIP events on the library
 * stream, after 3 warm-up repetitions */
int cmoop_conv_fwd_i8_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                           int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu,
                           int32_t iters, double* avg_ms);
/* cmoop_fake_quant_act in tracked mode (a_in required) with the codes output: codes_dev [n] int8 receives the code of every element
 * next to the fp32 value in x_dev.  codes_dev NULL: cmoop_fake_quant_act's launch and bytes */
int cmoop_fake_quant_act_codes(float* x_dev, int64_t n, int32_t bits, const float* a_in, int8_t* codes_dev);
/* average milliseconds of cmoop_fake_quant_act_codes' launch (n >= 1), as cmoop_conv_fwd_i8_time: what a site's quantiser costs an
 * integer inference pass, and the second launch of the pair "Integer depthwise" below replaces */
int cmoop_fake_quant_act_codes_time(float* x_dev, int64_t n, int32_t bits, const float* a_in, int8_t* codes_dev, int32_t iters,
                                    double* avg_ms);
/* host-only: the ops of a candidate at a T x F patch that run integer under cmoop_net_set_int8, in op order: rows [count][16] =
 * {op index, kind (0 conv, 1 dense), input act, output act, input site, H, W, Cin, Cout, KS, stride, relu, w_off, b_off (offsets
 * into the parameter arena), scale_off (first scale of the tensor in cmoop_net_get_quantized's scales), 0}.  An error when cap is
 * too small, or when such an op is beyond the kernels (Cin % 16, w_off % 16, 127^2 K < 2^31); count may be NULL */
int cmoop_int8_ops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows /* [cap][16] */,
                   int32_t cap, int32_t* count);
/* ---- Integer depthwise: the second level of integer inference (opt-in on top of it, BUILD-DEFINED; off by default) ---------------
 * THE arithmetic of an integer depthwise layer (quant.py restates it in numpy: dwconv_i8_acc / dwconv_i8_ref).  With the input
 * site's scale s_x = r_in / (float)qmax_act, the depthwise weight codes qw[ky][kx][c] (the layout of the parameter arena), their
 * channel scales s_w[c] and the tracked range r_out of the site the layer writes:
 *     acc[b,h,w,c] = sum over (ky, kx) of (int32) qx[b,h+ky-p,w+kx-p,c] * (int32) qw[ky][kx][c]      p = (K-1)/2; exact; a tap in
 *                    the SAME padding contributes 0
 *     z            = fl( (float)acc * fl(s_x * s_w[c]) )                        no bias, no activation (as the fp32 depthwise op)
 *     q, y         = the tracked-mode code and dequantised value of z under r_out: cmoop_actquant's element arithmetic, unchanged
 *   |acc| <= 25 * 127^2 = 403 225 < 2^24, so (float)acc is exact and ANY exact way of forming it gives the same bytes: int32
 *   multiply-adds, or fp32 FMAs on the converted codes (what the kernel does: every partial sum is an integer below 2^24).  Every
 *   fl() is ONE correctly rounded fp32 operation, contraction off.  A scale with s > 0 false gives codes 0 and y = +0.0.
 * In a net (cmoop_net_set_int8_depthwise, which needs cmoop_net_set_int8) every OP_DWCONV of an inference pass is ONE launch: it
 *   reads the input site's codes and the staged weight codes and writes the output site's quantised fp32 tensor AND its codes, so
 *   the fp32 depthwise launch and the site's quantiser launch are not made.  The fp32 tensor of the site stays written
 *   (cmoop_net_get_act and every fp32 reader keep working).  Every depthwise op of the search space reads a site and writes a site
 *   whose only reader is a pointwise op of cmoop_int8_ops (cmoop_int8_dw_ops asserts the former).  Train steps never take it.
 * Kernel (int8.hip, dwconv_i8_fwd_kernel<K>): NHWC int8 in, C a power of two in 16..512, K 3 / 5; a lane owns four channels
 *   (4-byte code loads, a 16-byte fp32 store and ONE packed store of four codes), an input row is read once and reused by the K
 *   output rows it reaches; weight codes [K][K][C] must be 16-byte aligned (w_off % 16 == 0 over the whole search space), as must
 *   the scales; 32-bit index math below 2^29 elements; no atomics.
 * OUT OF SCOPE: codes-only sites (the fp32 tensor not written), a fused depthwise + pointwise kernel. */
/* the lone integer depthwise layer on the library stream: xq_dev [B][H][W][C] and wq_dev [KS][KS][C] int8 codes (16-byte aligned),
 * s_w_dev [C] (16-byte aligned), y_dev [B][H][W][C] fp32 (16-byte aligned).  a_out (host) NULL: y = z, codes_dev must be NULL;
 * a_out given: y and codes_dev (may be NULL; 4-byte aligned) are z's dequantised value and code under the range *a_out at
 * out_bits.  Every element of the B rows of both outputs is written.  B == 0: success, nothing written.  C no power of two in
 * 16..512, KS not 3 or 5, a misaligned buffer or 2^29 elements and more: an error */
int cmoop_dwconv_fwd_i8(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, int32_t B, int32_t H, int32_t W,
                        int32_t C, int32_t KS, int32_t out_bits, const float* a_out /* host, may be NULL */, float* y_dev,
                        int8_t* codes_dev /* may be NULL */);
/* average milliseconds of cmoop_dwconv_fwd_i8's launch, as cmoop_conv_fwd_i8_time */
int cmoop_dwconv_fwd_i8_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, int32_t B, int32_t H, int32_t W,
                             int32_t C, int32_t KS, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev,
                             int32_t iters, double* avg_ms);
/* host-only: the depthwise ops of a candidate that run integer under cmoop_net_set_int8_depthwise, in op order: rows [count][16] in
 * cmoop_int8_ops' layout with kind 2, Cin = Cout = C, stride 1, relu 0, b_off -1 (no bias), and the OUTPUT site in the last
 * field: {op index, 2, input act, output act, input site, H, W, C, C, KS, 1, 0, w_off, -1, scale_off, output site}.  Empty for
 * variants A / B.  An error when cap is too small, when a depthwise op reads or writes an act that is no site, or is beyond the
 * kernel (C, KS, w_off % 16, scale_off % 4); count may be NULL */
int cmoop_int8_dw_ops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows /* [cap][16] */,
                      int32_t cap, int32_t* count);
/* ---- Integer inference: requantising epilogue, the third level (opt-in on top of integer inference, independent of "Integer
 * depthwise"; BUILD-DEFINED; off by default) ------------------------------------------------------------------------------------
 * THE arithmetic of a conv / dense op of cmoop_int8_ops whose output reaches an activation-quantisation site through per-channel
 * elementwise ops only (quant.py restates it in numpy: conv_i8_q_ref / dense_i8_q_ref, with fma32_ref).  acc, s_x and s_w[c] as in
 * "Integer inference"; scale[c] / shift[c] the fp32 vectors the eval BatchNorm prepares (cmoop_bn_eval_fwd's scale_dev / shift_dev);
 * r_out the tracked range of the site written:
 *     t = fl( fl( (float)acc * fl(s_x * s_w[c]) ) + bias[c] ) ;  t = fmaxf(t, 0) if the op has a ReLU      ("Integer inference")
 *     with a BatchNorm only:  t = fma(t, scale[c], shift[c])     ONE rounding ;  t = fmaxf(t, 0) if that BatchNorm has relu_after
 *     q, y = the tracked-mode code and dequantised value of t under r_out: cmoop_actquant's element arithmetic, unchanged
 *   The affine is a fused multiply-add because the eval BatchNorm's apply kernel (scale_shift_kernel, compiled at the default
 *   contraction setting) is one v_fma_f32 per element on gfx950.  The purpose of the definition is EQUALITY OF BYTES with the
 *   un-fused chain (cmoop_conv_fwd_i8 -> cmoop_bn_eval_fwd -> cmoop_fake_quant_act_codes): where the device's chain disagrees with
 *   this paragraph, the chain wins.  A scale with s > 0 false gives codes 0 and y = +0.0.
 * Which ops (cmoop_int8_fused_ops): T0 -- the op's own output act is a site (every hidden dense layer; the first convolution of a
 *   residual block and the pointwise halves when bn = 0); T1 -- the op's output is read only by an OP_BN that is not fused with a
 *   pool, and that BatchNorm's output act is a site (res*_conv1 -> bn -> ReLU of topology A, and the same on A_ds' pointwise
 *   halves).  Tails through a pool or the residual add, the skip projections, the output layer and the first convolution keep
 *   their launches.
 * In a net (cmoop_net_set_int8_fused, which needs cmoop_net_set_int8) such an op is ONE launch in an inference pass: for T1 the
 *   BatchNorm's tiny prepare launch moves ahead of it; the fused launch writes the site's quantised fp32 tensor and its codes; the
 *   scale_shift launch and the site's quantiser launch are not made.  The act between a T1 op and its BatchNorm is no longer
 *   written (nothing else reads it: the plan walk asserts this).  Train steps never take it.  It composes with "Integer depthwise".
 * Kernels (int8.hip, conv_i8_fwd_q_kernel / dense_i8_fwd_q_kernel): the tiles of "Integer inference" with this epilogue: a lane
 *   holds four consecutive channels of an output row and stores the fp32 quad as one 16-byte store and the four codes as ONE
 *   32-bit word.  Cout % 4 == 0, y 16-byte and codes 4-byte aligned; the same 32-bit index bounds; no atomics, no LDS.
 * OUT OF SCOPE: code emission from the pool, add + ReLU, global-pool and first-layer producers; dropping the fp32 tensor of a site
 *   whose readers are all integer ops; BatchNorm folding into the weights. */
/* the lone requantising conv layer on the library stream: cmoop_conv_fwd_i8's operands, then bn_scale_dev / bn_shift_dev [Cout]
 * (both NULL: no BatchNorm; one without the other: an error), relu_after (ignored without a BatchNorm), and the site written:
 * the range *a_out (host, required) at out_bits in [2, 8]; y_dev [B][OH][OW][Cout] fp32 (16-byte aligned) receives the dequantised
 * values and codes_dev (required, 4-byte aligned) the codes.  Cout % 4 != 0: an error.  B == 0: success, nothing written */
int cmoop_conv_fwd_i8_q(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                        const float* bn_scale_dev, const float* bn_shift_dev, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                        int32_t KS, int32_t stride, int32_t relu, int32_t relu_after, int32_t out_bits, const float* a_out /* host */,
                        float* y_dev, int8_t* codes_dev);
/* average milliseconds of cmoop_conv_fwd_i8_q's launch, as cmoop_conv_fwd_i8_time */
int cmoop_conv_fwd_i8_q_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                             const float* bn_scale_dev, const float* bn_shift_dev, int32_t B, int32_t H, int32_t W, int32_t Cin,
                             int32_t Cout, int32_t KS, int32_t stride, int32_t relu, int32_t relu_after, int32_t out_bits, const float* a_out,
                             float* y_dev, int8_t* codes_dev, int32_t iters, double* avg_ms);
/* the lone requantising dense layer: cmoop_dense_fwd_i8's operands and the tail of cmoop_conv_fwd_i8_q; y_dev [M][N], codes_dev
 * [M][N].  N % 4 != 0: an error.  M == 0: success, nothing written */
int cmoop_dense_fwd_i8_q(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                         const float* bn_scale_dev, const float* bn_shift_dev, int32_t M, int32_t N, int32_t K, int32_t relu,
                         int32_t relu_after, int32_t out_bits, const float* a_out /* host */, float* y_dev, int8_t* codes_dev);
/* average milliseconds of cmoop_dense_fwd_i8_q's launch */
int cmoop_dense_fwd_i8_q_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                              const float* bn_scale_dev, const float* bn_shift_dev, int32_t M, int32_t N, int32_t K, int32_t relu,
                              int32_t relu_after, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev, int32_t iters,
                              double* avg_ms);
/* average milliseconds of cmoop_dense_fwd_i8's launch and of the eval BatchNorm's apply launch alone (y = fma(x, scale[c], shift[c]),
 * then max(y, 0) under relu; x_dev / y_dev [M][C], C % 4 == 0), as cmoop_conv_fwd_i8_time: with cmoop_fake_quant_act_codes_time, the
 * launches of the chain a requantising launch replaces */
int cmoop_dense_fwd_i8_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                            int32_t M, int32_t N, int32_t K, int32_t relu, int32_t iters, double* avg_ms);
int cmoop_scale_shift_time(const float* x_dev, float* y_dev, const float* scale_dev, const float* shift_dev, int64_t M, int32_t C,
                           int32_t relu, int32_t iters, double* avg_ms);
/* host-only: the ops of a candidate that take the requantising epilogue under cmoop_net_set_int8_fused, in op order: rows
 * [count][20] = the op's cmoop_int8_ops row (16 fields, the last 0), then {the OP_BN's op index (-1: T0), that BatchNorm's
 * relu_after (0 for T0), the output site, the act written (the site's)}.  Every row's first 16 fields are a row of cmoop_int8_ops.
 * An error when cap is too small, when Cout % 4 != 0, when the act written is no site, or when the act between a T1 op and its
 * BatchNorm has another reader; count may be NULL */
int cmoop_int8_fused_ops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows /* [cap][20] */,
                         int32_t cap, int32_t* count);
/* the population call (above) with every argument: the other ten forward here.  aq NULL or disabled: cmoop_eval_population_p's
 * launches and bytes */
int cmoop_eval_population_aq(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                             const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_quant* q,
                             const cmoop_prune* pr, const cmoop_actquant* aq, const cmoop_dataset* ds, const int32_t* genes /* [n][6] */,
                             const uint32_t* seeds /* [n] */, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb,
                             double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated,
                             double* opoint /* [n][4], may be NULL */, double* quant /* [n][2], may be NULL */,
                             double* prune /* [n][3], may be NULL */);

/* host-only: does every conv layer of this candidate at `batch` rows per launch (pass max(batch, eval_batch)) stay inside
 * the kernels' 32-bit byte offsets (each activation / kernel tensor below 2^29 elements)?  Non-zero + message if not;
 * cmoop_net_create and the population calls make the same check before they allocate anything. */
int cmoop_plan_check(const int32_t gene[6], int32_t variant, int32_t T, int32_t F, int32_t batch);

/* host-only: the launch-path variant (kernel instantiation as rocprofv3 names it + "+sk" / "+stats" / "+tab" / "+slabs",
 * see cmoop_profile_variant) the TRAINER uses for one conv layer at this batch: op 0 forward (want_stats: the layer
 * feeds a BatchNorm), 1 dgrad, 2 wgrad.  Pure arithmetic on the shape -- tests enumerate every layer of every gene with
 * it and require a GPU parity case for each variant.  The layer is planned ALONE, as cmoop_conv_fwd_trainer /
 * cmoop_conv_bwd_trainer launch it: with the split-K workspace of its own geometry at this batch. */
int cmoop_conv_launch_plan(int32_t op, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride,
                           int32_t want_stats, char* name, int32_t name_cap);

/* host-only: the MFMA (implicit-GEMM) conv layers of a candidate in forward order, from the same plan walk the trainer
 * allocates for: layers[7 * i ..] = H, W, Cin, Cout, KS, stride, feeds_bn (the layer's output goes straight into a
 * BatchNorm).  At most `cap` layers are written; *count receives how many there are. */
int cmoop_plan_convs(const int32_t gene[6], int32_t variant, int32_t T, int32_t F, int32_t* layers /* [cap][7] */, int32_t cap,
                     int32_t* count);

/* host-only: the depthwise layers of a candidate (variants A_DS / B_DS; none for A / B) in forward order, the counterpart of
 * cmoop_plan_convs, where their pointwise halves appear with KS = 1, stride = 1: layers[4 * i ..] = H, W, C, KS */
int cmoop_plan_dwconvs(const int32_t gene[6], int32_t variant, int32_t T, int32_t F, int32_t* layers /* [cap][4] */, int32_t cap,
                       int32_t* count);

/* host-only: the launch-path variants, ';'-separated as in cmoop_last_kernels and in launch order, of the MFMA conv launches
 * a net created with (gene, cfg, T, F) makes in ONE train step at batch B (train != 0: forward with the statistics
 * epilogue where a layer feeds a BatchNorm, then weight and data gradients) or in one inference pass at batch B
 * (train == 0).  Unlike cmoop_conv_launch_plan this is computed with the net's SHARED split-K workspace, which is sized
 * from cfg.batch and max(cfg.batch, cfg.eval_batch) only: on an under-filled partial batch a layer may take another
 * tile or partition than the lone-layer plan of the same batch names. */
int cmoop_net_launch_plan(const int32_t gene[6], const cmoop_config* cfg, int32_t T, int32_t F, int32_t B, int32_t train,
                          char* buf, int32_t cap);

/* host-only: the halo-tiled direct convolution (stride-1 KS x KS layers) stages the input rows of a 128- / 256-pixel tile in LDS;
 * rows_bound = rows its LDS image is sized for (closed form), rows_needed = the most rows any tile of this geometry really
 * spans, rows_stageable = rows the per-thread staging slots can hold.  All 0 when the geometry runs on the implicit GEMM.
 * Tests sweep geometries and require rows_needed <= rows_bound <= rows_stageable. */
int cmoop_halo_tile_check(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t* rows_bound,
                          int32_t* rows_needed, int32_t* rows_stageable);

/* host-only: number of row slices the weight-gradient kernel splits a conv/dense layer into (workspace sizing;
 * NOT monotone in B -- tests pin that the trainer sizes its slab workspace for the worst batch 1..cfg.batch) */
int cmoop_wgrad_slices(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t* out);

/* host-only: row-run slices of the depthwise weight gradient, a function of the shape alone (NOT monotone in B: the trainer
 * sizes the layer's slab region for the worst batch 1..cfg.batch) */
int cmoop_dwconv_wgrad_slices(int32_t B, int32_t H, int32_t W, int32_t C, int32_t KS, int32_t* out);

/* calculate_fpr on host label arrays (nsga_penalty.py:351-364 and variants) */
int cmoop_calculate_fpr(const int32_t* y_true, const int32_t* y_pred, int64_t n, int32_t classes, int32_t fpr_variant,
                        double* out);

/* ---- audio front end (north-star addition; the reference loads pre-extracted features,
 *      nsga_penalty.py:64-71) and prepare_dataset's StandardScaler (nsga_penalty.py:103-141) */
int cmoop_logmel(const float* wav_dev /* [n_clips][n_samples] */, int64_t n_clips, int32_t n_samples,
                 float* out_dev /* [n_clips][1+n_samples/160][40] */);
/* Configurable front end.  Domain: n_fft in {256, 512, 1024, 2048}; 1 <= win <= n_fft (periodic Hann of win points centred
 * in n_fft); hop >= 1; 1 <= n_mels <= 128; 0 <= fmin < fmax <= sr/2; n_samples >= 1; T = 1 + n_samples / hop frames,
 * centre-padded with zeros.  scale 0: log(mel + log_eps).  scale 1: 10 log10(max(db_amin, mel)) - 10 log10(max(db_amin, ref))
 * with ref = 1.0 (db_ref_max 0) or the clip's own largest mel power (db_ref_max 1), then, when top_db >= 0, every value below
 * (the clip's maximum - top_db) is raised to it.  scale 2: the linear mel power itself (a band that holds no FFT bin gives 0);
 * it is what the PCEN calls below normalise.  The default is the geometry of the fixed-geometry call above. */
typedef struct cmoop_frontend_config {
    int32_t sr, n_fft, win, hop, n_mels;
    int32_t scale;       /* 0 log, 1 dB, 2 power */
    int32_t db_ref_max;
    float fmin, fmax, log_eps, db_amin, top_db;
} cmoop_frontend_config;
int cmoop_frontend_config_default(cmoop_frontend_config* c);
/* host-only: non-zero + a message naming the offending field when the config is outside the domain */
int cmoop_frontend_check(const cmoop_frontend_config* c);
/* host-only: T = 1 + n_samples / hop */
int cmoop_frontend_frames(const cmoop_frontend_config* c, int32_t n_samples, int32_t* T);
/* host-only: the dense form [n_mels][1 + n_fft/2] of the sparse mel table the kernel reads (Slaney scale, slaney norm) */
int cmoop_frontend_mel_basis(const cmoop_frontend_config* c, float* out_host);
/* Configs with n_fft 512, n_mels <= 64 and the log scale run on the fixed-geometry call's kernel, every other (the dB and
 * power scales always) on the general one. */
int cmoop_logmel_ex(const cmoop_frontend_config* c, const float* wav_dev /* [n_clips][n_samples] */, int64_t n_clips,
                    int32_t n_samples, float* out_dev /* [n_clips][T][n_mels] */);
/* average milliseconds of `iters` launches of the call above between two HIP events on the library's stream, after 3 warm-up launches */
int cmoop_logmel_ex_time(const cmoop_frontend_config* c, const float* wav_dev, int64_t n_clips, int32_t n_samples, float* out_dev,
                         int32_t iters, double* avg_ms);
/* Stream front end: ONE recording, its frames spread over the whole chip.  out_dev [T][n_mels], T = cmoop_frontend_frames.
 * scale 0: the values cmoop_logmel_ex gives for the recording passed as one clip, bit for bit (the same kernel arithmetic,
 *          the 512-point kernel included; only the grid differs).
 * scale 1: the UN-REFERENCED dB value 10 log10(max(db_amin, mel)); db_ref_max / top_db are per-window quantities and are
 *          applied by cmoop_net_predict_stream, not here.
 * scale 2: the mel power, bit for bit the clip call's.
 * Domain: cmoop_frontend_check's, 1 <= n_samples < 2^31 - 2 n_fft (the kernels index samples in 32 bits), T * n_mels < 2^31. */
int cmoop_logmel_stream(const cmoop_frontend_config* c, const float* wav_dev /* [n_samples] */, int64_t n_samples, float* out_dev);
/* as cmoop_logmel_ex_time: average milliseconds of `iters` launches between two HIP events after 3 warm-up launches */
int cmoop_logmel_stream_time(const cmoop_frontend_config* c, const float* wav_dev, int64_t n_samples, float* out_dev,
                             int32_t iters, double* avg_ms);
/* host-only: n_windows = 1 + (n_frames - T) / hop_frames; error when n_frames < T or hop_frames < 1 */
int cmoop_stream_windows(int64_t n_frames, int32_t T, int32_t hop_frames, int64_t* n_windows);
/* ---- PCEN: per-channel energy normalisation of mel power (north-star addition; the reference has no front end).
 * For one band of one clip or recording with mel power P[t], t = 0..T-1, and E[t] = input_scale * P[t]:
 *     M[-1] = E[0];   M[t] = M[t-1] + s * (E[t] - M[t-1])        (so M[0] = E[0])
 *     out[t] = (E[t] / (eps + M[t])^alpha + delta)^r - delta^r
 * Domain, all values finite: 0 < s <= 1, 0 <= alpha <= 1, delta >= 0, 0 < r <= 1, eps > 0, input_scale > 0.
 * The device computes in fp32 with the six values rounded to fp32: the update is fmaf(s, E - M, M), delta^r comes from the
 * same powf that raises the first term, so an all-zero band gives exactly 0.0f.  One device function holds this arithmetic
 * for every call below: the clip, stand-alone and stream forms agree bit for bit wherever their carry-in is the same. */
typedef struct cmoop_pcen {
    double s, alpha, delta, r, eps, input_scale;
} cmoop_pcen;
int cmoop_pcen_default(cmoop_pcen* p); /* s 0.025, alpha 0.98, delta 2, r 0.5, eps 1e-6, input_scale 1 */
/* host-only: non-zero + a message naming the offending field when a value is outside the domain */
int cmoop_pcen_check(const cmoop_pcen* p);
/* host-only: the s of a smoother with time constant time_constant_s: Tf = time_constant_s * sr / hop frames,
 * s = (sqrt(1 + 4 Tf^2) - 1) / (2 Tf^2) */
int cmoop_pcen_smoothing(double time_constant_s, int32_t sr, int32_t hop, double* s);
/* Clip form on a power tensor, in place: every (clip, band) column of e_dev [n][T][F] is normalised from its own first
 * frame.  1 <= F <= 128, T >= 1, n * T * F < 2^31. */
int cmoop_pcen_apply(const cmoop_pcen* p, float* e_dev /* [n][T][F], in place */, int64_t n, int32_t T, int32_t F);
/* Mel power of every clip and its PCEN in ONE launch; c->scale must be 2.  Bit-equal to cmoop_logmel_ex followed by
 * cmoop_pcen_apply. */
int cmoop_logmel_pcen(const cmoop_frontend_config* c, const cmoop_pcen* p, const float* wav_dev /* [n_clips][n_samples] */,
                      int64_t n_clips, int32_t n_samples, float* out_dev /* [n_clips][T][n_mels] */);
/* host-only: the stream form cuts a recording of n_frames frames into n_chunks = ceil(n_frames / chunk) chunks; chunk is a
 * function of n_frames alone (never of the device): ceil(sqrt(n_frames)) / 4 rounded up to a multiple of 64, at least 64 */
int cmoop_pcen_stream_plan(int64_t n_frames, int32_t* chunk, int32_t* n_chunks);
/* The same recurrence for ONE recording, in place on e_dev [n_frames][F], spread over the chip as three launches on the
 * library stream: (1) per (chunk, band) the chunk's end state from a zero start, (2) one workgroup, serial over the chunks,
 * carry[0] = E[0], carry[c+1] = (1-s)^chunk * carry[c] + local[c] with (1-s)^chunk computed in double on the host,
 * (3) per (chunk, band) the serial recurrence from carry[c].  Chunk 0 starts from E[0]: a recording of at most `chunk` frames
 * carries the bits of cmoop_pcen_apply (and then needs no launch 1).  1 <= F <= 128, n_frames * F < 2^31. */
int cmoop_pcen_stream(const cmoop_pcen* p, float* e_dev /* [n_frames][F], in place */, int64_t n_frames, int32_t F);
/* cmoop_logmel_stream at scale 2 (c->scale must be 2) followed by cmoop_pcen_stream on its output */
int cmoop_logmel_pcen_stream(const cmoop_frontend_config* c, const cmoop_pcen* p, const float* wav_dev /* [n_samples] */,
                             int64_t n_samples, float* out_dev /* [T][n_mels] */);
/* as cmoop_logmel_stream_time, for the four launches of the call above */
int cmoop_logmel_pcen_stream_time(const cmoop_frontend_config* c, const cmoop_pcen* p, const float* wav_dev, int64_t n_samples,
                                  float* out_dev, int32_t iters, double* avg_ms);
/* ---- resampling: clips and recordings at any sample rate, brought to the front end's rate on the GPU (north-star addition;
 *      the reference has no front end).  No audio-quality or accuracy claim is made beyond "this is the default filter of
 *      scipy.signal.resample_poly".
 * Rational rate change by up / down with gcd(up, down) = 1 and an odd-length centred FIR h of n_taps = 2 half + 1 taps.
 * For a row x[0..L), x = 0 outside:
 *     n_out = ceil(L up / down)
 *     y[n]  = sum_i x[i] h[n down - i up + half]      over all i with 0 <= n down - i up + half <= 2 half and 0 <= i < L
 * With the default filter this is scipy.signal.resample_poly(x, up, down) (float64: equal lengths, outputs to 1e-15 of the maximum).
 * Default filter (cmoop_resample_filter): half = half_width max(up, down) (half_width 10 is scipy's), fc = 1 / max(up, down),
 *     h[k] = up w[k] fc sinc(fc (k - half)) / sum_k(w[k] fc sinc(fc (k - half)))
 * w the Kaiser window of n_taps points (beta 5.0 is scipy's), designed in double on the host with I0 from its power series
 * (scipy.signal.firwin(n_taps, fc, window=("kaiser", beta)) * up to 1.3e-15 of the maximum) and rounded once to fp32.
 * A caller may pass any odd number of any fp32 taps instead (scipy's window=<array> form).
 * Device arithmetic: one fp32 accumulator per output, started at 0.0f, terms in ascending i, one fmaf per term; the order is
 * part of the definition, so every launch shape gives the same bits.
 * Domain: 1 <= up, down <= 1024 (reduced); n_taps odd; taps per output tpp = ceil(n_taps / up) <= 256 (the default filter
 * therefore serves every down <= 12 up); n_clips >= 0; 1 <= n_samples; n_clips * max(n_samples, n_out) < 2^36.  up = down = 1
 * is a plain FIR.  Errors start with "resample: " and name the offending argument.
 * Launch: a workgroup owns `tile` consecutive outputs of one row and stages the inputs they read, zero outside [0, L) of its
 * own row.  tile = min(512, (8192 - tpp - 2) up / down), rounded down to a multiple of 64 from 64 on and at least 1: a function
 * of (up, down, n_taps) alone, never of the device, that keeps the staged span within 8192 floats.  Tile j of a row holds
 * outputs out_first = j tile .. + out_count and stages in_count inputs from
 *     in_first = (out_first down + half) / up - tpp + 1      up to      ((out_first + out_count - 1) down + half) / up
 * (64-bit, computed once per workgroup; indices inside the tile are 32-bit).  in_first may be negative and the span may run
 * past n_samples: the zero-filled part counts.  HBM-bound: 4 L + 4 n_out bytes and tpp n_out FMA per row. */
/* host-only: the default filter.  *n_taps = 2 half_width max(up, down) + 1 always (taps_host NULL: only that); otherwise
 * cap >= *n_taps values are needed.  1 <= half_width <= 4096, beta >= 0 */
int cmoop_resample_filter(int32_t up, int32_t down, int32_t half_width, double beta, float* taps_host, int32_t cap, int32_t* n_taps);
/* host-only: output length, tile, tiles per row and taps per output of a row of n_samples; NULL outputs are skipped */
int cmoop_resample_plan(int64_t n_samples, int32_t up, int32_t down, int32_t n_taps, int64_t* n_out, int32_t* tile, int64_t* n_tiles,
                        int32_t* taps_per_output);
/* host-only: what workgroup `tile_index` of a row stages -- the launcher's own arithmetic */
int cmoop_resample_tile_span(int64_t n_samples, int32_t up, int32_t down, int32_t n_taps, int64_t tile_index, int64_t* out_first,
                             int32_t* out_count, int64_t* in_first, int32_t* in_count);
/* One launch on the library's stream for clip batches and for one long recording (n_clips 1) alike; out of place.  The
 * polyphase table [up][tpp] (86 KB at most for the default filter) is built on the host per call and uploaded into pooled
 * device memory; where it fits a workgroup's LDS beside the span, persistent workgroups copy it there once. */
int cmoop_resample(const float* wav_dev /* [n_clips][n_samples] */, int64_t n_clips, int64_t n_samples, int32_t up, int32_t down,
                   const float* taps_host /* [n_taps] */, int32_t n_taps, float* out_dev /* [n_clips][n_out] */);
/* as cmoop_logmel_stream_time: average milliseconds of `iters` launches between two HIP events after 3 warm-up launches
 * (the table upload is outside the timed window) */
int cmoop_resample_time(const float* wav_dev, int64_t n_clips, int64_t n_samples, int32_t up, int32_t down, const float* taps_host,
                        int32_t n_taps, float* out_dev, int32_t iters, double* avg_ms);
/* optional MFCC features: DCT-II, ortho-normalised, along the mel axis of log-mel rows; first n_mfcc coefficients.
 * The reference ships no front end; its comment at ablation_study/sa_nsga_init.py:68 calls the stored features MFCCs. */
int cmoop_mfcc(const float* logmel_dev /* [rows][n_mels] */, int64_t rows, int32_t n_mels, int32_t n_mfcc,
               float* out_dev /* [rows][n_mfcc] */);
int cmoop_standardize_fit(const float* x_dev, int64_t rows, int32_t cols, double* mean_host, double* scale_host);
int cmoop_standardize_apply(float* x_dev, int64_t rows, int32_t cols, const double* mean_host, const double* scale_host);

/* ---- HIP-event profile of the MFMA GEMM kernels sampled during cmoop_eval_population
 *      (cfg.profile_every): one entry per kernel instantiation, named as rocprofv3 names it */
int cmoop_profile_reset(void);
int cmoop_profile_count(int32_t* out);
int cmoop_profile_entry(int32_t i, char* name, int32_t name_cap, int64_t* launches, double* total_ms, double* total_flops);
/* launch-path variants of the sampled launches: instantiation name + "+sk" (split-K slabs and combine) / "+bal" /
 * "+stats" (BatchNorm statistics in the epilogue) / "+tab" (row-table operand loader) / "+slabs" (wgrad row slices) */
int cmoop_profile_variant_count(int32_t* out);
int cmoop_profile_variant(int32_t i, char* name, int32_t name_cap);

/* ---- single-candidate session (parity tests, smoke): one net on the library's stream */
typedef struct cmoop_net cmoop_net;
int cmoop_net_create(const int32_t gene[6], const cmoop_config* cfg, int32_t T, int32_t F, uint32_t seed, cmoop_net** out);
int cmoop_net_destroy(cmoop_net* net);
int cmoop_net_total_params(cmoop_net* net, int64_t* out);
int cmoop_net_get_params(cmoop_net* net, float* host);       /* canonical order, see genes.py */
int cmoop_net_set_params(cmoop_net* net, const float* host);
int cmoop_net_get_grads(cmoop_net* net, float* host);
int cmoop_net_train_step(cmoop_net* net, const float* x_dev, const int32_t* y_dev, const int32_t* idx_dev, int64_t row0,
                         int32_t B);
int cmoop_net_evaluate(cmoop_net* net, const float* x_dev, const int32_t* y_dev, int64_t n, double* loss_sum,
                       int64_t* correct, int32_t* preds_dev);
int cmoop_net_train_metrics(cmoop_net* net, double* loss_sum, int64_t* correct, int32_t reset);
/* Model.predict: class probabilities of n rows, inference mode (moving statistics, no dropout), eval_batch rows per launch;
 * p_j = exp(z_j - max) / sum, the p behind cmoop_net_evaluate's loss, so argmax p is the prediction that call returns */
int cmoop_net_predict(cmoop_net* net, const float* x_dev /* [n][T][F] */, int64_t n, float* probs_dev /* [n][classes] */);
/* Sliding-window scoring: window i = rows [i*hop_frames, i*hop_frames + T) of feat_dev [n_frames][F] (T, F: the net's).
 * Per window, in this order:
 *   (a) when db != NULL and db->scale == 1: cmax = the window's largest value,
 *       ref = db_ref_max ? cmax : 10 log10(max(db_amin, 1)),
 *       floor = top_db >= 0 ? (cmax - ref) - top_db : -inf, value = max(value - ref, floor)
 *       -- the dB tail of cmoop_logmel_ex with "window" for "clip", on the un-referenced values of cmoop_logmel_stream;
 *   (b) when mean_host != NULL (then scale_host too, both [F]): (float)(((double)v - mean[c]) / scale[c]),
 *       as cmoop_standardize_apply;
 *   (c) forward + softmax, eval_batch windows per launch.
 * feat_dev is not modified and the window tensor is never materialised (one eval_batch * T * F chunk, whatever n_frames).
 * probs_dev [n_windows][classes], n_windows = cmoop_stream_windows(n_frames, T, hop_frames). */
int cmoop_net_predict_stream(cmoop_net* net, const float* feat_dev, int64_t n_frames, int32_t hop_frames,
                             const cmoop_frontend_config* db, const double* mean_host, const double* scale_host,
                             float* probs_dev);
/* Full training state of the net (host arrays of cmoop_net_total_params floats; any pointer may be NULL): parameters in
 * canonical order INCLUDING the BatchNorm moving statistics, Adam's m and v in the same layout (zero in the
 * non-trainable slots), optimizer.iterations and the global train-step count that keys the dropout masks.  With these a
 * checker can re-synchronise with the GPU at every epoch boundary of Model.fit (nsga_penalty.py:383) instead of
 * comparing two long, chaotic fp32 trajectories at their ends. */
int cmoop_net_get_state(cmoop_net* net, float* params, float* adam_m, float* adam_v, int64_t* iterations, int64_t* steps);
int cmoop_net_set_state(cmoop_net* net, const float* params, const float* adam_m, const float* adam_v, int64_t iterations,
                        int64_t steps);
/* Train-time augmentation of every following cmoop_net_train_step / _run_epoch / _fit step of this net (aug NULL or a
 * disabled config: off, and the net steps bit for bit as one that never had one).  cmoop_net_evaluate / _predict /
 * _predict_stream never augment.  The loss and accuracy cmoop_net_train_metrics reports are those of the augmented batches.
 * The draws are keyed by the position in the batch and the step: another cfg.batch gives other draws. */
int cmoop_net_set_augment(cmoop_net* net, const cmoop_augment* aug /* NULL = off */);
/* Soft-target training loss (cmoop_loss above) of every following cmoop_net_train_step / _run_epoch / _fit step of this net
 * (loss NULL or a disabled config: off, and the net steps bit for bit as one that never had one).  The config is copied.
 * cmoop_net_evaluate / _predict / _predict_stream and the validation loss of cmoop_net_fit stay the sparse cross-entropy.
 * cmoop_net_train_metrics then reports the weighted soft-target loss sum and the count of argmax z == primary. */
int cmoop_net_set_loss(cmoop_net* net, const cmoop_loss* loss /* NULL = off */);
/* ONE optimiser step on rows and targets given by the caller (device pointers): x_rows_dev [B][T][F], t_dev [B][classes],
 * w_dev [B] (NULL: 1), primary_dev [B] (NULL: arg max of t).  No augmentation, no mixing and no target construction, whatever
 * the net's augment / loss settings; dropout, Adam and the counters advance as in any step.  The hook for soft targets
 * from elsewhere (a teacher's probabilities, for one). */
int cmoop_net_train_step_targets(cmoop_net* net, const float* x_rows_dev, const float* t_dev, const float* w_dev,
                                 const int32_t* primary_dev, int32_t B);
/* floats the net has allocated for the loss: out = mixup batch buffer, t, w, primary (0: that buffer does not exist) */
int cmoop_net_loss_buffers(cmoop_net* net, int64_t out[4]);
/* Distillation (cmoop_distill above) of every following cmoop_net_train_step / _run_epoch / _fit step of this net (NULL or a
 * disabled config: off, and the net steps bit for bit as one that never had one).  alpha and T are copied; the TABLE IS NOT:
 * it must stay allocated while the net trains.  A step whose gather rows are known and differ from n_rows fails.
 * cmoop_net_train_metrics then reports the distillation loss sum and the count of argmax z == primary. */
int cmoop_net_set_distill(cmoop_net* net, const cmoop_distill* distill /* NULL = off */);
/* Optimiser options (cmoop_optim above) of every following train step of this net, from the next step on (NULL or a disabled
 * config: off, and the net steps bit for bit as one that never had one).  The config is copied; the rate tables of a fit under
 * way are rebuilt.  The schedule is a function of `iterations`, so cmoop_net_get_state / _set_state carry it unchanged.  With
 * decay or a clip on, the step is not captured as a graph. */
int cmoop_net_set_optim(cmoop_net* net, const cmoop_optim* optim /* NULL = off */);
/* the last train step's out = {sum of squares of the trainable gradients, their norm, the clip scale, launch path (0: the fused
 * launch, which computes no norm: 0, 0, 1; 1: finish + update)} */
int cmoop_net_optim_stats(cmoop_net* net, double out[4]);
/* Weight EMA (cmoop_ema above) of every following train step of this net, from the next step on (NULL or a disabled config:
 * off, and the net steps bit for bit as one that never had one; an average that already exists is kept, no longer advanced).
 * The first enabled config makes the average a bit copy of the parameter arena; a later one keeps it.  The config is copied; the
 * rate table of a fit under way is rebuilt.  cmoop_net_set_state leaves the average untouched: a re-synchronising checker calls
 * cmoop_net_set_ema_params as well. */
int cmoop_net_set_ema(cmoop_net* net, const cmoop_ema* ema /* NULL = off */);
/* the average arena to / from a host array of cmoop_net_total_params floats; an error when the net has no average */
int cmoop_net_get_ema(cmoop_net* net, float* host);
int cmoop_net_set_ema_params(cmoop_net* net, const float* host);
/* on != 0: cmoop_net_evaluate / _predict / _predict_logits / _predict_stream read the average in place of the parameters (a
 * pointer swap, no copy) until on == 0.  An error when the net has no average; a train step while it is on is refused.
 * cmoop_net_get_params / _set_params / _get_state / _set_state always mean the raw parameters. */
int cmoop_net_use_ema(cmoop_net* net, int32_t on);
/* w := a (Keras' finalize_variable_values), for callers that step by hand; cmoop_net_fit does it itself.  Adam's moments, the
 * counters and the average stay. */
int cmoop_net_finalize_ema(cmoop_net* net);
/* Operating-point read-out (cmoop_opoint above) of every following cmoop_net_fit of this net (NULL or a disabled config: off,
 * and the fit is launch for launch the one of a net that never had it).  The config is copied.  No train step and no earlier
 * read-out changes: after the weights are final -- the restored snapshot, the finalised average or the last epoch -- the fit
 * runs one more cmoop_net_predict pass over the validation split and the three read-out launches. */
int cmoop_net_set_opoint(cmoop_net* net, const cmoop_opoint* op /* NULL = off */);
/* the record of the last cmoop_net_fit: classes_host [classes] and summary [4] (either may be NULL); an error when that fit ran
 * without the option */
int cmoop_net_last_opoint(cmoop_net* net, cmoop_opoint_class* classes_host, double* summary);
/* cmoop_net_predict's pass over x_dev [n][T][F] into a pooled buffer, then cmoop_operating_point against y_dev [n] */
int cmoop_net_operating_point(cmoop_net* net, const float* x_dev, const int32_t* y_dev, int64_t n, const cmoop_opoint* op,
                              cmoop_opoint_class* classes_host /* [classes] */, double* summary /* [4] */);
/* Quantisation-aware training (cmoop_quant above) of every following train step and inference call of this net (NULL or a disabled
 * config: off, and the net is one that never had it, launch for launch and bit for bit).  The config is copied.  Switching it on
 * after a plain fit and evaluating is post-training quantisation.  cmoop_net_get_params / _set_params / _get_state / _set_state
 * always mean the latent fp32 weights. */
int cmoop_net_set_quant(cmoop_net* net, const cmoop_quant* q /* NULL = off */);
/* the arena inference would read now (the average under cmoop_net_use_ema), quantised: wq_params_host [total params] (kernels
 * dequantised, every other element copied), codes_host [total params] int8 (the code of every kernel element at its arena
 * index, 0 elsewhere), scales_host [total channels of cmoop_quant_table]; any may be NULL.  An error while the option is off. */
int cmoop_net_get_quantized(cmoop_net* net, float* wq_params_host, int8_t* codes_host, float* scales_host);
/* Magnitude pruning (cmoop_prune above) of every following train step and inference call of this net (NULL or a disabled config:
 * off, and the net is one that never had it, launch for launch and bit for bit).  The config is copied.  Switching it on after a
 * plain fit and evaluating is one-shot magnitude pruning.  With cmoop_net_set_quant on as well, cmoop_net_get_quantized returns
 * the pruned kernels quantised. */
int cmoop_net_set_prune(cmoop_net* net, const cmoop_prune* p /* NULL = off */);
/* the arena inference would read now (the average under cmoop_net_use_ema) pruned at the final sparsity, not quantised:
 * weff_params_host [total params] (every element outside the pruned tensors copied) and zeros_host [count of cmoop_prune_table]
 * uint32, the elements of each tensor that became zero; either may be NULL.  An error while the option is off. */
int cmoop_net_get_pruned(cmoop_net* net, float* weff_params_host, uint32_t* zeros_host);
/* Activation fake quantisation (cmoop_actquant above) of every following train step and inference call of this net (NULL or a
 * disabled config: off, and every launch and bit is that of a net that never had one; the site records are kept).  The per-site
 * records (count 0) and the partials workspace are allocated on first use.  cmoop_net_get_state / _set_state do not carry the
 * records: a re-synchronising caller uses the two entry points below as well. */
int cmoop_net_set_actquant(cmoop_net* net, const cmoop_actquant* aq /* NULL = off */);
/* the site records in site order: host [cap] receives count = the number of sites of them (an error when cap is smaller; count
 * may be NULL).  host NULL with count given: the number of sites alone.  An error while no records exist (the option was never
 * on). */
int cmoop_net_get_act_ranges(cmoop_net* net, cmoop_act_range* host, int32_t cap, int32_t* count);
/* loads the site records (count must be the number of sites; every count >= 0, no negative r or m_b).  When every record has
 * count > 0, inference is possible from here on. */
int cmoop_net_set_act_ranges(cmoop_net* net, const cmoop_act_range* host, int32_t count);
/* Integer inference ("Integer inference" above) of every following inference call of this net; train steps never take it.  on != 0
 * is refused, with a message, before anything is launched and with the net unchanged, unless cmoop_net_set_quant and
 * cmoop_net_set_actquant are both on and the ranges are ready; and when a tracked r or a weight scale, read on the host here, is
 * not finite.  The weight-code arena, the scale buffer and one int8 buffer per site (max(batch, eval_batch) samples) are allocated
 * on first use.  on == 0: off, and every launch and byte is that of a net that never had it.  Turning cmoop_net_set_quant or
 * cmoop_net_set_actquant off turns it off as well.  Finiteness is checked HERE and by cmoop_net_set_act_ranges while the mode is
 * on (a non-finite r is then an error and nothing is loaded), not per pass: a train step or cmoop_net_set_params that later
 * yields a NaN or Inf range or scale is not caught, and integer passes then return NaN logits without a fault, as fp32 passes do. */
int cmoop_net_set_int8(cmoop_net* net, int32_t on);
/* cmoop_int8_ops of this net's plan (host arithmetic; the mode need not be on) */
int cmoop_net_int8_ops(cmoop_net* net, int64_t* rows /* [cap][16] */, int32_t cap, int32_t* count);
/* Integer depthwise ("Integer depthwise" above) of every following inference call of this net; train steps never take it.  on != 0
 * is refused, with a message and the net unchanged, unless cmoop_net_set_int8 is on; a net without a depthwise op (variants A / B)
 * accepts it and nothing changes.  on == 0: off, and every launch and byte is that of cmoop_net_set_int8 alone.  Turning
 * cmoop_net_set_int8, cmoop_net_set_quant or cmoop_net_set_actquant off turns it off as well */
int cmoop_net_set_int8_depthwise(cmoop_net* net, int32_t on);
/* cmoop_int8_dw_ops of this net's plan (host arithmetic; the level need not be on) */
int cmoop_net_int8_dw_ops(cmoop_net* net, int64_t* rows /* [cap][16] */, int32_t cap, int32_t* count);
/* The requantising epilogue ("Integer inference: requantising epilogue" above) of every following inference call of this net;
 * train steps never take it.  on != 0 is refused, with a message and the net unchanged, unless cmoop_net_set_int8 is on; a net
 * without a fusible op accepts it and nothing changes.  on == 0: off, and every launch and byte is that of the levels that stay
 * on.  Turning cmoop_net_set_int8, cmoop_net_set_quant or cmoop_net_set_actquant off turns it off as well.  While it is on, an
 * inference pass does not write the act between a fused op and its BatchNorm (cmoop_net_get_act then returns what an earlier
 * pass or step left there) */
int cmoop_net_set_int8_fused(cmoop_net* net, int32_t on);
/* cmoop_int8_fused_ops of this net's plan (host arithmetic; the level need not be on) */
int cmoop_net_int8_fused_ops(cmoop_net* net, int64_t* rows /* [cap][20] */, int32_t cap, int32_t* count);
/* debug read-out of act index i of the plan: dims (may be NULL) = {H, W, C, 1 if materialised, 1 if it has a gradient buffer,
 * the number of acts}; data_host / grad_host (either may be NULL; both NULL: dims only) receive the first B rows of the data and
 * of the gradient as the last step or pass left them.  An error for an act that is never materialised. */
int cmoop_net_get_act(cmoop_net* net, int32_t i, int32_t B, int32_t dims[6], float* data_host, float* grad_host);
/* cmoop_net_train_step_targets with a teacher row per batch row, q_dev [B][classes], and the distillation loss at
 * (alpha, temperature), whatever cmoop_net_set_distill says. */
int cmoop_net_train_step_distill_targets(cmoop_net* net, const float* x_rows_dev, const float* t_dev, const float* w_dev,
                                         const int32_t* primary_dev, const float* q_dev, double alpha, double temperature, int32_t B);
/* cmoop_net_predict with the logits themselves in place of their softmax: logits_dev [n][classes].  cmoop_softmax_probs of
 * them is cmoop_net_predict's output bit for bit.  What a teacher hands to cmoop_distill. */
int cmoop_net_predict_logits(cmoop_net* net, const float* x_dev /* [n][T][F] */, int64_t n, float* logits_dev /* [n][classes] */);
/* rows the resident training tensor holds: gathered row indices are clamped into [0, n_rows) (0 = unknown, no clamp) */
int cmoop_net_set_gather_rows(cmoop_net* net, int64_t n_rows);
/* ONE epoch of Model.fit on the trainer's own path: epoch permutation of (seed, epoch) computed on the device when
 * cfg.shuffle, ceil(n_train / batch) steps driven by the device-resident step state, last partial batch kept. */
int cmoop_net_run_epoch(cmoop_net* net, const float* x_train_dev, const int32_t* y_train_dev, int64_t n_train, int32_t epoch);
/* What the fit loop's train steps (cmoop_net_run_epoch, cmoop_net_fit, cmoop_eval_population*) did, as process-wide totals since
 * the library was loaded: out = {steps launched eagerly, steps replayed from a captured graph, captures made, captures
 * dropped}.  Without CMOOP_GRAPH=1 in the environment the last three stay 0.  With it, a full-batch step after a net's first is
 * captured once and replayed; the capture is dropped, and the step captured again, when an option setter or
 * cmoop_net_set_state ran, when the step budget was rebuilt (a second fit, an epoch past cfg.epochs) or when the training
 * tensors, the split length or the teacher table differ from the ones it froze.  Partial batches, profiled steps and nets with
 * an option that forbids capture step eagerly.  A capture that the runtime refuses is not an error: the net steps eagerly, and
 * only these totals show it.  Host only: launches nothing, allocates nothing; the totals are atomic, a read while other threads
 * step is a snapshot of each. */
int cmoop_step_launch_counts(int64_t out[4]);
/* evaluate_individual's fit + read-outs (nsga_penalty.py:377-392) on THIS net -- the body of cmoop_eval_population's
 * per-candidate work -- with the per-epoch validation history (first hist_cap epochs), the epoch EarlyStopping took its
 * best weights from (-1: none / early_stop off) and the epochs run. */
int cmoop_net_fit(cmoop_net* net, const cmoop_dataset* ds, int32_t hist_cap, double* val_loss_hist, double* val_acc_hist,
                  int32_t* epochs_run, int32_t* best_epoch, double* acc, double* fpr, double* val_loss);
int cmoop_epoch_permutation(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out_host);
/* the same permutation computed on the GPU (what the trainer uses: no host sort / H2D copy per epoch); n <= 262144 */
int cmoop_epoch_permutation_device(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out_dev);

/* ---- kernel-level entry points (parity tests and the roofline leg of bench.py).
 *      conv: y[B,OH,OW,Cout] = SAME-conv(x[B,H,W,Cin], w[Cout][KS][KS][Cin]) + bias, optional ReLU */
int cmoop_conv_fwd(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t B, int32_t H,
                   int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu);
/* dx = dgrad(dy) (optionally masked by x > 0), dw[Cout][KS][KS][Cin], db[Cout] */
int cmoop_conv_bwd(const float* x_dev, const float* w_dev, const float* dy_dev, float* dx_dev, float* dw_dev, float* db_dev,
                   int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t mask_relu);
/* The same two operations launched EXACTLY as the trainer launches them (Net::forward / Net::backward): row-table operand
 * loader, split-K workspace, flip-transposed dgrad operand prepared up front, weight-gradient slabs + fixed-order slice
 * sum, and -- forward, col_sum != NULL -- the BatchNorm batch statistics taken in the conv epilogue (per-tile partials
 * summed here in float64 into col_sum / col_sumsq [Cout]; *stats_fused = 0 when the launch was split-K and the
 * statistics came from the stand-alone reduction, as in the trainer).  Cin must be a power of two >= 16. */
int cmoop_conv_fwd_trainer(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t B, int32_t H,
                           int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu, double* col_sum,
                           double* col_sumsq, int32_t* stats_fused);
int cmoop_conv_bwd_trainer(const float* x_dev, const float* w_dev, const float* dy_dev, float* dx_dev, float* dw_dev,
                           float* db_dev, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride,
                           int32_t mask_relu);
/* kernel instantiations (+ launch-path variant suffixes, see cmoop_profile_variant) the calling thread's last
 * cmoop_conv_fwd* / cmoop_conv_bwd* call launched, ';'-separated */
int cmoop_last_kernels(char* buf, int32_t cap);
/* average ms per launch over `iters` back-to-back launches (HIP events on the library stream);
 * mode 0: forward implicit GEMM, 1: dgrad implicit GEMM (y holds dY, x receives dX), 2: wgrad MFMA kernel */
int cmoop_conv_time(int32_t mode, const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t B,
                    int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t iters, double* avg_ms);
/* MLP-head layers (Dense+ReLU ladder, nsga_penalty.py:306-330) on the dense.hip kernels: y[M][N] = x[M][K] w[N][K]^T + b
 * (optional ReLU); dx (optionally masked by x > 0), dw[N][K], db[N].  K a multiple of 16. */
int cmoop_dense_fwd(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t M, int32_t N, int32_t K,
                    int32_t relu);
int cmoop_dense_bwd(const float* x_dev, const float* w_dev, const float* dy_dev, float* dx_dev, float* dw_dev, float* db_dev,
                    int32_t M, int32_t N, int32_t K, int32_t mask_relu);
/* The same kernels launched as a train step launches them (tests).  gemm_mode: CMOOP_GEMM_* (FP32 and BF16 do not depend
 * on the environment).  dropout_rate in [0,1), 0: no dropout; else the inverted-dropout epilogue of fc layer dropout_layer:
 * element (m, n) is kept, and multiplied by (float)(1 / (1 - rate)), iff the 24-bit draw of (seed, 0x2000 + dropout_layer,
 * step, m N + n) is >= (uint32_t)(rate 2^24).  step_state_dev == NULL: step is the host argument.  Else it points to the
 * 16-byte device step state {int64 row0; uint32 step; uint32 iter} of a fit, the kernel reads step from there and the host
 * argument is ignored. */
int cmoop_dense_fwd_ex(const float* x_dev, const float* w_dev, const float* bias_dev, float* y_dev, int32_t M, int32_t N, int32_t K,
                       int32_t relu, int32_t gemm_mode, double dropout_rate, uint32_t seed, int32_t dropout_layer, uint32_t step,
                       const void* step_state_dev);
/* dx = mask_relu ? (x > 0 ? dx mask_scale : 0) : dx (ReLU / dropout backward of the layer's input); merged != 0: the one
 * launch of the trainer's default backward, 0: weight gradient and data gradient as two launches */
int cmoop_dense_bwd_ex(const float* x_dev, const float* w_dev, const float* dy_dev, float* dx_dev, float* dw_dev, float* db_dev,
                       int32_t M, int32_t N, int32_t K, int32_t mask_relu, double mask_scale, int32_t gemm_mode, int32_t merged);
/* depthwise k x k convolution (SAME, stride 1, depth multiplier 1, no bias; NHWC fp32 in every gemm_mode), launched as the
 * trainer launches it.  C a power of two in 16..512, KS in {3, 5}, B H W C < 2^29; w_dev [KS][KS][C].
 * y[b,h,w,c] = sum_{ky,kx} x[b,h+ky-p,w+kx-p,c] w[ky][kx][c], p = (KS-1)/2, zeros outside the image */
int cmoop_dwconv_fwd(const float* x_dev, const float* w_dev, float* y_dev, int32_t B, int32_t H, int32_t W, int32_t C, int32_t KS);
/* dw [KS][KS][C] (per-slice partials into a workspace allocated inside the call, summed in the optimiser launch's fixed order:
 * bit-reproducible, no atomics) and, when dx_dev != NULL, dx = mask_relu ? (x > 0 ? dx : 0) : dx */
int cmoop_dwconv_bwd(const float* x_dev, const float* w_dev, const float* dy_dev, float* dx_dev, float* dw_dev, int32_t B, int32_t H,
                     int32_t W, int32_t C, int32_t KS, int32_t mask_relu);
/* average milliseconds of `iters` back-to-back launches (HIP events on the library stream, after three warm-up launches) of
 * one depthwise kernel alone.  mode 0: forward into out_dev; 1: data gradient of dy_dev with the x > 0 mask into out_dev;
 * 2: the weight-gradient kernel (per-slice partials into a workspace of the call; out_dev unused) */
int cmoop_dwconv_time(int32_t mode, const float* x_dev, const float* w_dev, const float* dy_dev, float* out_dev, int32_t B, int32_t H,
                      int32_t W, int32_t C, int32_t KS, int32_t iters, double* avg_ms);
int cmoop_maxpool_fwd(const float* x_dev, float* y_dev, uint8_t* arg_dev, int32_t B, int32_t H, int32_t W, int32_t C);
int cmoop_maxpool_bwd(const float* dy_dev, const uint8_t* arg_dev, const float* y_dev, float* dx_dev, int32_t B, int32_t H,
                      int32_t W, int32_t C, int32_t mask_y_pos);
/* ---- per-kernel entry points of the BatchNorm / pooling / loss / optimiser kernels (parity tests).  Each call launches
 *      what the trainer launches for the operation, in the trainer's order, on device pointers; reduction workspaces are
 *      allocated and freed inside the call; hyper-parameters travel as double and are cast to float where the trainer casts.
 *      blocks: 0 = the trainer's partial count for (M, C); 1..4096 forces that many reduction workgroups.
 *      BatchNorm over x[M][C] (C % 4 == 0, C <= 1024): batch statistics -> mean / invstd / scale / shift [C] each, moving
 *      statistics updated in place, y = x scale + shift (optional ReLU) */
int cmoop_bn_train_fwd(const float* x_dev, const float* gamma_dev, const float* beta_dev, float* moving_mean_dev,
                       float* moving_var_dev, float* y_dev, float* mean_dev, float* invstd_dev, float* scale_dev, float* shift_dev,
                       int64_t M, int32_t C, double eps, double momentum, int32_t relu, int32_t blocks);
int cmoop_bn_eval_fwd(const float* x_dev, const float* gamma_dev, const float* beta_dev, const float* moving_mean_dev,
                      const float* moving_var_dev, float* y_dev, float* scale_dev, float* shift_dev, int64_t M, int32_t C,
                      double eps, int32_t relu);
/* dx (optionally masked by x > 0), dgamma, dbeta; sums_dev (may be NULL): the finalised (sum dy, sum dy xhat) [2][C] */
int cmoop_bn_bwd(const float* dy_dev, const float* x_dev, const float* mean_dev, const float* invstd_dev, const float* gamma_dev,
                 float* dx_dev, float* dgamma_dev, float* dbeta_dev, float* sums_dev, int64_t M, int32_t C, int32_t mask_x_pos,
                 int32_t blocks);
/* BatchNorm-apply (+ReLU) + MaxPool 2x2 SAME in one pass over x[B,H,W,C], and its backward from the pooled gradient */
int cmoop_bn_pool_fwd(const float* x_dev, const float* scale_dev, const float* shift_dev, float* y_dev, uint8_t* arg_dev, int32_t B,
                      int32_t H, int32_t W, int32_t C, int32_t relu);
int cmoop_bn_pool_bwd(const float* g_pooled_dev, const uint8_t* arg_dev, const float* x_dev, const float* mean_dev,
                      const float* invstd_dev, const float* gamma_dev, float* dx_dev, float* dgamma_dev, float* dbeta_dev,
                      float* sums_dev, int32_t B, int32_t H, int32_t W, int32_t C, int32_t mask_x_pos, int32_t blocks);
/* y = max(a + b, 0) over n floats (n % 4 == 0); global average pooling of x[B][HW][C] and its backward (masked by x > 0) */
int cmoop_add_relu(const float* a_dev, const float* b_dev, float* y_dev, int64_t n);
int cmoop_gap_fwd(const float* x_dev, float* y_dev, int32_t B, int32_t HW, int32_t C);
int cmoop_gap_bwd(const float* dy_dev, const float* x_dev, float* dx_dev, int32_t B, int32_t HW, int32_t C);
/* softmax + clipped sparse cross-entropy of z[B][C]; row r's label is labels[idx ? idx[row0 + r] : row0 + r], the row index
 * clamped into [0, n_rows) when n_rows > 0.  dz (may be NULL): d(mean loss)/dz; acc (two 8-byte words: double loss sum,
 * int64 correct) is ADDED into; preds (may be NULL): the row arg max */
int cmoop_softmax_ce(const float* z_dev, const int32_t* labels_dev, const int32_t* idx_dev, int64_t row0, int64_t n_rows, int32_t B,
                     int32_t C, float* dz_dev, double* acc_dev, int32_t* preds_dev);
int cmoop_softmax_probs(const float* z_dev, float* p_dev, int32_t B, int32_t C);
/* one Keras-form Adam update of n floats with the step size alpha (the caller's bias-corrected lr) */
int cmoop_adam(float* w_dev, const float* g_dev, float* m_dev, float* v_dev, int64_t n, double alpha, double beta1, double beta2,
               double eps);
/* the fused optimiser launch: `count` (<= 64) segments tiling the arena in order, host arrays; S[i] == 0: plain segment
 * (gradient read from g); S[i] > 0: g = fixed-order sum of the S[i] slices at slab_dev + slab_off[i] + s stride[i] */
int cmoop_adam_segments(float* w_dev, float* g_dev, float* m_dev, float* v_dev, const float* slab_dev, int32_t count,
                        const int64_t* off, const int64_t* n, const int32_t* S, const int64_t* stride, const int64_t* slab_off,
                        double alpha, double beta1, double beta2, double eps);
/* the first two launches of the finish + update path on the segments of cmoop_adam_segments: g finished (slab sums stored,
 * bit-equal to the fused launch's), no weight moved; partials_dev[b] (cap >= the workgroup count, returned in *n_partials) =
 * workgroup b's fp32 sum of g^2 over its elements whose kind is not 2 (kinds_dev NULL: all); record_dev (16 bytes:
 * double sum of squares, float norm, float scale) from the partials summed in double and global_clipnorm (0: scale 1) */
int cmoop_grad_finish(float* g_dev, const float* slab_dev, int32_t count, const int64_t* off, const int64_t* n, const int32_t* S,
                      const int64_t* stride, const int64_t* slab_off, const uint8_t* kinds_dev /* may be NULL */,
                      double global_clipnorm, float* partials_dev, int32_t cap, int32_t* n_partials, void* record_dev);
/* the third launch on n floats: g scale (read from record_dev), the value clamp, the masked decay with lr, then cmoop_adam's
 * update with the step size alpha; kinds_dev NULL: every element is a kernel.  Elements of kind 2 keep w, m and v */
int cmoop_adamw(float* w_dev, const float* g_dev, float* m_dev, float* v_dev, const uint8_t* kinds_dev /* may be NULL */, int64_t n,
                const void* record_dev, double alpha, double lr, double beta1, double beta2, double eps, double weight_decay,
                int32_t decay_mask, double clipvalue);
/* cm[C][C] (int64) = confusion matrix of n label pairs (out-of-range labels ignored; force_true_zero: every true label 0) */
int cmoop_confusion(const int32_t* y_true_dev, const int32_t* y_pred_dev, int64_t n, int32_t C, int32_t force_true_zero,
                    int64_t* cm_dev);
/* output-layer helpers: out[C] = column sums of x[M][C]; dx[M][K] = dy[M][N] w[N][K], mask (may be NULL): dx = mask > 0 ? dx scale : 0 */
int cmoop_colsum_small(const float* x_dev, float* out_dev, int32_t M, int32_t C);
int cmoop_dense_dgrad_small(const float* dy_dev, const float* w_dev, float* dx_dev, int32_t M, int32_t N, int32_t K,
                            const float* mask_dev, double scale);
int cmoop_device_synchronize(void);

#ifdef __cplusplus
}
#endif
#endif /* CMOOP_H */
