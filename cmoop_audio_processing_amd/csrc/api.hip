// extern "C" boundary of libcmoop_hip.so -- see include/cmoop.h for the contract.
#include "../../include/cmoop.h"
#include "net.h"

#include <cstddef>
#include <cstring>
#include <memory>
#include <mutex>
#include <vector>

using namespace cmoop;

static thread_local std::string g_err;
static thread_local std::string g_last_kernels;   // cmoop_last_kernels

template <class F>
static int guard(F&& f) {
    try {
        f();
        return 0;
    } catch (const std::exception& e) {
        g_err = e.what();
        return 1;
    } catch (...) {
        g_err = "unknown error";
        return 2;
    }
}

constexpr int MAX_DEVICES = 16;

// one library stream per (calling thread, device): switching devices neither leaks nor reuses the other device's stream
static hipStream_t lib_stream() {
    static thread_local hipStream_t streams[MAX_DEVICES] = {nullptr};
    int dev = 0;
    CMOOP_HIP(hipGetDevice(&dev));
    CMOOP_REQUIRE(dev >= 0 && dev < MAX_DEVICES, "device index out of range");
    if (!streams[dev]) CMOOP_HIP(hipStreamCreateWithFlags(&streams[dev], hipStreamNonBlocking));
    return streams[dev];
}

// front-end tables (twiddles / window / sparse mel weights): one set per device, created once under a lock
static const FrontendTables* frontend_tables_for_current_device() {
    static std::mutex mu;
    static FrontendTables* tables[MAX_DEVICES] = {nullptr};
    int dev = 0;
    CMOOP_HIP(hipGetDevice(&dev));
    CMOOP_REQUIRE(dev >= 0 && dev < MAX_DEVICES, "device index out of range");
    std::lock_guard<std::mutex> l(mu);
    if (!tables[dev]) tables[dev] = frontend_tables_create(FrontendCfg());
    return tables[dev];
}

// tables of the configurable front end: a bounded map keyed by (device, config), oldest entry dropped first.  A caller
// keeps its shared_ptr for the length of its launch, so dropping an entry never frees tables another thread is using.
static std::shared_ptr<const FrontendTables> frontend_tables_for(const FrontendCfg& c) {
    struct Entry { int dev; FrontendCfg cfg; std::shared_ptr<const FrontendTables> t; };
    constexpr size_t CAP = 16;
    static std::mutex mu;
    static std::vector<Entry>& cache = *new std::vector<Entry>;   // never destroyed: no hipFree after the runtime has shut down
    int dev = 0;
    CMOOP_HIP(hipGetDevice(&dev));
    std::lock_guard<std::mutex> l(mu);
    for (const Entry& e : cache)
        if (e.dev == dev && frontend_cfg_equal(e.cfg, c)) return e.t;
    std::shared_ptr<const FrontendTables> t(frontend_tables_create(c), [dev](const FrontendTables* p) {
        int cur = 0;
        if (hipGetDevice(&cur) == hipSuccess && cur != dev) hipSetDevice(dev);
        frontend_tables_destroy(const_cast<FrontendTables*>(p));
        if (cur != dev) hipSetDevice(cur);
    });
    if (cache.size() >= CAP) cache.erase(cache.begin());
    cache.push_back(Entry{dev, c, t});
    return t;
}

static FrontendCfg to_frontend_cfg(const cmoop_frontend_config* c) {
    CMOOP_REQUIRE(c != nullptr, "front end config is NULL");
    FrontendCfg f;
    f.sr = c->sr; f.n_fft = c->n_fft; f.win = c->win; f.hop = c->hop; f.n_mels = c->n_mels; f.scale = c->scale;
    f.db_ref_max = c->db_ref_max != 0; f.fmin = c->fmin; f.fmax = c->fmax; f.log_eps = c->log_eps; f.db_amin = c->db_amin;
    f.top_db = c->top_db;
    frontend_check(f);
    return f;
}

static_assert(sizeof(cmoop_pcen) == 48, "cmoop_pcen is part of the ABI");
static PcenParams to_pcen(const cmoop_pcen* p) {
    CMOOP_REQUIRE(p != nullptr, "pcen config is NULL");
    PcenCfg c;
    c.s = p->s; c.alpha = p->alpha; c.delta = p->delta; c.r = p->r; c.eps = p->eps; c.input_scale = p->input_scale;
    pcen_check(c);
    return pcen_params(c);
}
// the front end config of a PCEN call: any scale but 2 (power) is the caller's mistake, not something to override
static FrontendCfg to_pcen_frontend_cfg(const cmoop_frontend_config* c, const char* who) {
    const FrontendCfg f = to_frontend_cfg(c);
    CMOOP_REQUIRE(f.scale == 2, std::string(who) + ": PCEN normalises mel power, the front end config must have scale 2 (got scale " +
                                    std::to_string(f.scale) + ")");
    return f;
}

static NetConfig to_cfg(const cmoop_config* c) {
    CMOOP_REQUIRE(c != nullptr, "config is NULL");
    NetConfig n;
    n.variant = c->variant; n.classes = c->classes; n.epochs = c->epochs; n.batch = c->batch; n.patience = c->patience;
    n.early_stop = c->early_stop; n.restore_best = c->restore_best; n.acc_readout = c->acc_readout;
    n.fpr_variant = c->fpr_variant; n.shuffle = c->shuffle; n.eval_batch = c->eval_batch; n.n_slots = c->n_slots;
    n.profile_every = c->profile_every;
    n.gemm_mode = c->gemm_mode == CMOOP_GEMM_DEFAULT ? gemm_mode_default() : c->gemm_mode;
    n.lr = c->lr; n.beta1 = c->beta1; n.beta2 = c->beta2; n.adam_eps = c->adam_eps; n.bn_eps = c->bn_eps;
    n.bn_momentum = c->bn_momentum; n.dropout = c->dropout;
    CMOOP_REQUIRE(n.variant >= 0 && n.variant <= 3, "variant must be CMOOP_VARIANT_A, _B, _A_DS or _B_DS");
    CMOOP_REQUIRE(n.fpr_variant >= 0 && n.fpr_variant <= 2, "bad fpr_variant");
    CMOOP_REQUIRE(n.epochs >= 0 && n.patience >= 0 && n.batch >= 1 && n.eval_batch >= 1, "bad epochs/patience/batch");
    CMOOP_REQUIRE(n.dropout >= 0.0 && n.dropout < 1.0, "dropout must be in [0,1)");
    CMOOP_REQUIRE(n.gemm_mode == GEMM_FP32 || n.gemm_mode == GEMM_BF16X3 || n.gemm_mode == GEMM_BF16, "bad gemm_mode");
    return n;
}

static_assert(sizeof(cmoop_augment) == 48, "cmoop_augment is part of the ABI");
static AugmentCfg to_augment(const cmoop_augment* a) {
    CMOOP_REQUIRE(a != nullptr, "augment config is NULL");
    AugmentCfg c;
    c.time_shift = a->time_shift; c.time_masks = a->time_masks; c.time_mask_max = a->time_mask_max;
    c.freq_masks = a->freq_masks; c.freq_mask_max = a->freq_mask_max;
    c.p = a->p; c.noise_std = a->noise_std; c.fill = a->fill;
    return c;
}

static_assert(sizeof(cmoop_loss) == 40, "cmoop_loss is part of the ABI");
static LossCfg to_loss(const cmoop_loss* l) {   // class_weight stays the caller's array
    CMOOP_REQUIRE(l != nullptr, "loss config is NULL");
    LossCfg c;
    c.label_smoothing = l->label_smoothing; c.mixup_alpha = l->mixup_alpha; c.mixup_p = l->mixup_p;
    c.class_weight = l->class_weight; c.n_class_weight = l->n_class_weight;
    return c;
}
// the lam table of an enabled mixup on the device for one kernel-alone call (null with mixup off)
static MixupParams scratch_mixup(const LossCfg& c, float* tab_dev, hipStream_t s) {
    MixupParams m;
    if (!loss_mixup_on(c)) return m;
    std::vector<float> tab(MIXUP_TABLE);
    mixup_table(c.mixup_alpha, tab.data());
    CMOOP_HIP(hipMemcpyAsync(tab_dev, tab.data(), MIXUP_TABLE * 4, hipMemcpyHostToDevice, s));
    CMOOP_HIP(hipStreamSynchronize(s));
    m.on = 1;
    m.gate_thr = (uint32_t)std::floor(c.mixup_p * 16777216.0);
    m.tab = tab_dev;
    return m;
}

static_assert(sizeof(cmoop_distill) == 32, "cmoop_distill is part of the ABI");
static DistillCfg to_distill(const cmoop_distill* d) {   // the table stays the caller's
    CMOOP_REQUIRE(d != nullptr, "distill config is NULL");
    DistillCfg c;
    c.alpha = d->alpha; c.temperature = d->temperature; c.teacher_logits = d->teacher_logits_dev; c.n_rows = d->n_rows;
    return c;
}

static_assert(sizeof(cmoop_optim) == 224, "cmoop_optim is part of the ABI");
static OptimCfg to_optim(const cmoop_optim* o) {
    CMOOP_REQUIRE(o != nullptr, "optim config is NULL");
    OptimCfg c;
    c.schedule = o->schedule; c.staircase = o->staircase; c.decay_mask = o->decay_mask; c.n_boundaries = o->n_boundaries;
    c.warmup_steps = o->warmup_steps; c.decay_steps = o->decay_steps;
    c.warmup_start = o->warmup_start; c.alpha = o->alpha; c.decay_rate = o->decay_rate;
    std::copy(o->boundaries, o->boundaries + OPTIM_MAX_BOUNDARIES, c.boundaries);
    std::copy(o->values, o->values + OPTIM_MAX_BOUNDARIES + 1, c.values);
    c.weight_decay = o->weight_decay; c.global_clipnorm = o->global_clipnorm; c.clipvalue = o->clipvalue;
    return c;
}

static_assert(sizeof(cmoop_ema) == 16, "cmoop_ema is part of the ABI");
static EmaCfg to_ema(const cmoop_ema* e) {
    CMOOP_REQUIRE(e != nullptr, "ema config is NULL");
    EmaCfg c;
    c.momentum = e->momentum; c.warmup = e->warmup; c.reserved = e->reserved;
    return c;
}

static_assert(sizeof(cmoop_opoint) == 16, "cmoop_opoint is part of the ABI");
static_assert(sizeof(cmoop_opoint_class) == 32 && sizeof(cmoop_opoint_class) == sizeof(OpointClass), "cmoop_opoint_class is part of the ABI");
static OpointCfg to_opoint(const cmoop_opoint* p) {
    CMOOP_REQUIRE(p != nullptr, "opoint config is NULL");
    OpointCfg c;
    c.recall = p->recall; c.objective = p->objective; c.reserved = p->reserved;
    return c;
}
static_assert(sizeof(cmoop_quant) == 16, "cmoop_quant is part of the ABI");
static QuantCfg to_quant(const cmoop_quant* q) {
    CMOOP_REQUIRE(q != nullptr, "quant config is NULL");
    QuantCfg c;
    c.bits = q->bits; c.objective = q->objective; c.reserved[0] = q->reserved[0]; c.reserved[1] = q->reserved[1];
    return c;
}
// the finalised table of rows_host [count][5] against an arena of n elements
static QuantTable to_quant_table(const int64_t* rows, int32_t count, int64_t n) {
    CMOOP_REQUIRE(count >= 0 && count <= QUANT_MAX_ROWS && (count == 0 || rows), "quant: 0 <= count <= 128 and the rows");
    QuantTable tab;
    for (int i = 0; i < count; ++i) {
        const int64_t* r = rows + 5 * (size_t)i;
        for (int k = 0; k < 5; ++k) CMOOP_REQUIRE(r[k] >= 0 && r[k] <= QUANT_MAX_ARENA, "quant: a table value is outside [0, 2^31)");
        tab.rows.push_back(QuantRow{(int32_t)r[0], (int32_t)r[1], (int32_t)r[2], (int32_t)r[3], (int32_t)r[4], 0, 0});
    }
    quant_table_finalize(tab, n);
    return tab;
}
static_assert(sizeof(cmoop_prune) == 24, "cmoop_prune is part of the ABI");
static PruneCfg to_prune(const cmoop_prune* p) {
    CMOOP_REQUIRE(p != nullptr, "prune config is NULL");
    PruneCfg c;
    c.sparsity = p->sparsity; c.begin_step = p->begin_step; c.end_step = p->end_step; c.objective = p->objective;
    c.skip_small = p->skip_small;
    return c;
}
// the finalised table of rows_host [count][3] against an arena of n elements
static PruneTable to_prune_table(const int64_t* rows, int32_t count, int64_t n) {
    CMOOP_REQUIRE(count >= 0 && count <= PRUNE_MAX_ROWS && (count == 0 || rows), "prune: 0 <= count <= 128 and the rows");
    PruneTable tab;
    for (int i = 0; i < count; ++i) {
        const int64_t* r = rows + 3 * (size_t)i;
        for (int k = 0; k < 3; ++k) CMOOP_REQUIRE(r[k] >= -1 && r[k] <= PRUNE_MAX_ARENA, "prune: a table value is outside [-1, 2^31)");
        tab.rows.push_back(PruneRow{(int32_t)r[0], (int32_t)r[1], (int32_t)r[2], 0});
    }
    prune_table_finalize(tab, n);
    return tab;
}
static_assert(sizeof(cmoop_actquant) == 16, "cmoop_actquant is part of the ABI");
static ActQuantCfg to_actquant(const cmoop_actquant* a) {
    CMOOP_REQUIRE(a != nullptr, "actquant config is NULL");
    ActQuantCfg c;
    c.bits = a->bits; c.momentum = a->momentum; c.reserved[0] = a->reserved[0]; c.reserved[1] = a->reserved[1];
    return c;
}
// cmoop_act_range and ActRange are one layout
static_assert(sizeof(cmoop_act_range) == sizeof(ActRange) && offsetof(cmoop_act_range, m_b) == offsetof(ActRange, m_b) &&
              offsetof(cmoop_act_range, r) == offsetof(ActRange, r) && offsetof(cmoop_act_range, count) == offsetof(ActRange, count) &&
              offsetof(cmoop_act_range, reserved) == offsetof(ActRange, reserved), "cmoop_act_range layout");
// cmoop_opoint_class and OpointClass are one layout (asserted above and field by field here)
static OpointClass* as_classes(cmoop_opoint_class* c) {
    static_assert(offsetof(cmoop_opoint_class, u2) == offsetof(OpointClass, u2) && offsetof(cmoop_opoint_class, P) == offsetof(OpointClass, P) &&
                  offsetof(cmoop_opoint_class, N) == offsetof(OpointClass, N) && offsetof(cmoop_opoint_class, k) == offsetof(OpointClass, k) &&
                  offsetof(cmoop_opoint_class, tp) == offsetof(OpointClass, tp) && offsetof(cmoop_opoint_class, fp) == offsetof(OpointClass, fp) &&
                  offsetof(cmoop_opoint_class, thr) == offsetof(OpointClass, thr), "cmoop_opoint_class layout");
    return reinterpret_cast<OpointClass*>(c);
}

// The converted training options of one population call: to_* and the matching *_check of every struct handed in, in the
// order augment, loss, distill, optim, ema, opoint, quant, prune, actquant (what a call with two bad structs reports first); owns what opt points into
namespace {
struct AbiTrainOptions {
    AugmentCfg aug;
    LossCfg loss;
    DistillCfg distill;
    OptimCfg optim;
    EmaCfg ema;
    OpointCfg opoint;
    QuantCfg quant;
    PruneCfg prune;
    ActQuantCfg actq;
    TrainOptions opt;
    AbiTrainOptions(const cmoop_augment* a, const cmoop_loss* l, const cmoop_distill* d, const cmoop_optim* o, const cmoop_ema* e,
                    const cmoop_opoint* p, const cmoop_quant* q, const cmoop_prune* pr, const cmoop_actquant* aq, const NetConfig& c,
                    const Dataset& ds) {
        if (a) { aug = to_augment(a); augment_check(aug, ds.T, ds.F); opt.aug = &aug; }
        if (l) { loss = to_loss(l); loss_check(loss, c.classes); opt.loss = &loss; }
        if (d) { distill = to_distill(d); distill_check(distill, c.classes, ds.n_train); opt.distill = &distill; }
        if (o) { optim = to_optim(o); optim_check(optim); opt.optim = &optim; }
        if (e) { ema = to_ema(e); ema_check(ema); opt.ema = &ema; }
        if (p) { opoint = to_opoint(p); opoint_check(opoint); opt.opoint = &opoint; }
        if (q) { quant = to_quant(q); quant_check(quant); opt.quant = &quant; }
        if (pr) { prune = to_prune(pr); prune_check(prune); opt.prune = &prune; }
        if (aq) { actq = to_actquant(aq); actquant_check(actq); opt.actq = &actq; }
    }
    AbiTrainOptions(const AbiTrainOptions&) = delete;
};
}  // namespace

static Dataset to_dataset(const cmoop_dataset* ds) {
    Dataset d;
    d.x_train = ds->x_train; d.y_train = ds->y_train; d.n_train = ds->n_train;
    d.x_val = ds->x_val; d.y_val = ds->y_val; d.n_val = ds->n_val; d.T = ds->T; d.F = ds->F;
    return d;
}

// average ms of `iters` back-to-back runs of once() on stream s, after three warm-up runs (HIP events)
template <class F>
static double time_launches(hipStream_t s, int iters, F&& once) {
    for (int i = 0; i < 3; ++i) once();
    hipEvent_t a, b;
    CMOOP_HIP(hipEventCreate(&a));
    CMOOP_HIP(hipEventCreate(&b));
    CMOOP_HIP(hipEventRecord(a, s));
    for (int i = 0; i < iters; ++i) once();
    CMOOP_HIP(hipEventRecord(b, s));
    CMOOP_HIP(hipEventSynchronize(b));
    float ms = 0.f;
    CMOOP_HIP(hipEventElapsedTime(&ms, a, b));
    hipEventDestroy(a); hipEventDestroy(b);
    return (double)ms / std::max(1, iters);
}

// the three PCEN launches on s with their pooled workspace; the workspace goes back once the stream has drained
template <class F>
static void with_pcen_workspace(int T, int n_bands, hipStream_t s, F&& body) {
    PoolScope pool(s);
    body(pool.get<float>(std::max<size_t>(pcen_stream_workspace_floats(T, n_bands), 4) * sizeof(float)));
    CMOOP_HIP(hipStreamSynchronize(s));
}

// device scratch of one call: released when the call ends, after its stream has drained
struct Scratch {
    hipStream_t s;
    std::vector<void*> ptrs;
    explicit Scratch(hipStream_t stream) : s(stream) {}
    Scratch(const Scratch&) = delete;
    ~Scratch() { hipStreamSynchronize(s); for (void* p : ptrs) hipFree(p); }
    float* floats(size_t n) {   // null for n == 0
        void* p = nullptr;
        if (n) {
            const int fill = pool_fill_value();
            CMOOP_HIP(hipMalloc(&p, n * 4));
            ptrs.push_back(p);
            pool_fill_device(p, n * 4, fill);
        }
        return static_cast<float*>(p);
    }
    void* rowtab(const ConvGeom& g, int rows) {   // a lone layer's row table of geometry g (rows == 0: it has none)
        void* t = floats((size_t)rows * 2);
        if (t) launch_build_rowtab(g, t, s);
        return t;
    }
};

// records the launch-path variant names of the GEMM launches a kernel-level call makes (cmoop_last_kernels)
struct RecordingHook : GemmHook {
    int cls = 0;
    std::string* out;
    explicit RecordingHook(std::string* o) : out(o) {}
    const GemmTiming* begin(int c, double) override { cls = c; return nullptr; }
    void end(int code, int flags) override {
        if (!out->empty()) *out += ";";
        *out += gemm_variant_name(cls, code, flags);
    }
};

struct cmoop_net {
    Net* net;
};

// the body of cmoop_net_set_<who>: a NULL struct is sent on as null, anything else converted first
template <class Abi, class Cfg>
static int net_set_option(cmoop_net* h, const char* who, const Abi* abi, Cfg (*convert)(const Abi*), void (Net::*set)(const Cfg*)) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, std::string(who) + ": NULL net");
        if (!abi) { (h->net->*set)(nullptr); return; }
        const Cfg c = convert(abi);
        (h->net->*set)(&c);
    });
}

extern "C" {

int cmoop_abi_version(void) { return CMOOP_ABI_VERSION; }
const char* cmoop_last_error(void) { return g_err.c_str(); }

void cmoop_config_default(cmoop_config* c) {
    if (!c) return;
    std::memset(c, 0, sizeof(*c));
    c->variant = CMOOP_VARIANT_A; c->classes = 10; c->epochs = 300; c->batch = 64; c->patience = 5;
    c->early_stop = 1; c->restore_best = 0; c->acc_readout = 0; c->fpr_variant = CMOOP_FPR_V1; c->shuffle = 1;
    c->eval_batch = 256; c->n_slots = 8; c->profile_every = 0;
    c->lr = 1e-3; c->beta1 = 0.9; c->beta2 = 0.999; c->adam_eps = 1e-7; c->bn_eps = 1e-3; c->bn_momentum = 0.99;
    c->dropout = 0.3;
}

int cmoop_param_count(const int32_t gene[6], int32_t variant, int32_t classes, int64_t* out) {
    return guard([&] { *out = param_count(gene, variant, classes); });
}
int cmoop_fwd_flops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, double* out) {
    return guard([&] { *out = fwd_flops_per_sample(gene, variant, classes, T, F); });
}

// every population call; next == NULL: candidates are taken longest-first from a process-local counter; a NULL option: off
static void eval_population_abi(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss,
                                const cmoop_distill* distill, const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op,
                                const cmoop_quant* q, const cmoop_prune* pr, const cmoop_actquant* aq, const cmoop_dataset* ds,
                                const int32_t* genes, const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr,
                                int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated, double* opoint, double* quant,
                                double* prune) {
    CMOOP_REQUIRE(ds && genes && seeds, "NULL argument");
    CMOOP_REQUIRE(n >= 0, "negative population size");
    CMOOP_REQUIRE(!next || evaluated, "NULL argument");
    NetConfig c = to_cfg(cfg);
    const Dataset d = to_dataset(ds);
    const AbiTrainOptions options(aug, loss, distill, optim, ema, op, q, pr, aq, c, d);
    CMOOP_REQUIRE(n == 0 || (d.x_train && d.y_train && d.x_val && d.y_val), "dataset pointers are NULL");
    for (int i = 0; i < n; ++i) check_plan_ranges(genes + 6 * i, c.variant, d.T, d.F, std::max(c.batch, c.eval_batch));
    std::vector<EvalResult> r(n);
    std::function<int()> pull;   // empty: the process-local longest-first counter
    if (next) pull = [&]() { return (int)next(ctx); };
    eval_population(c, d, genes, seeds, n, r.data(), pull, options.opt);
    for (int i = 0; i < n; ++i) {
        if (evaluated) evaluated[i] = r[i].evaluated;
        if (acc) acc[i] = r[i].acc;
        if (size_mb) size_mb[i] = r[i].size_mb;
        if (fpr) fpr[i] = r[i].fpr;
        if (epochs_run) epochs_run[i] = r[i].epochs_run;
        if (val_loss) val_loss[i] = r[i].val_loss;
        if (seconds) seconds[i] = r[i].seconds;
        if (opoint) std::memcpy(opoint + 4 * (size_t)i, r[i].opoint, sizeof(r[i].opoint));
        if (quant) std::memcpy(quant + 2 * (size_t)i, r[i].quant, sizeof(r[i].quant));
        if (prune) std::memcpy(prune + 3 * (size_t)i, r[i].prune, sizeof(r[i].prune));
    }
}

int cmoop_eval_population(const cmoop_config* cfg, const cmoop_dataset* ds, const int32_t* genes, const uint32_t* seeds,
                          int32_t n, double* acc, double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss,
                          double* seconds) {
    return cmoop_eval_population_aug(cfg, nullptr, ds, genes, seeds, n, nullptr, nullptr, acc, size_mb, fpr, epochs_run, val_loss, seconds,
                                     nullptr);
}

int cmoop_eval_population_pull(const cmoop_config* cfg, const cmoop_dataset* ds, const int32_t* genes, const uint32_t* seeds,
                               int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr,
                               int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated) {
    if (!next || !evaluated) return guard([] { CMOOP_REQUIRE(false, "NULL argument"); });
    return cmoop_eval_population_aug(cfg, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr, epochs_run, val_loss, seconds,
                                     evaluated);
}

int cmoop_eval_population_aug(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_dataset* ds, const int32_t* genes,
                              const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb,
                              double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated) {
    return cmoop_eval_population_ex(cfg, aug, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr, epochs_run, val_loss, seconds,
                                    evaluated);
}

int cmoop_eval_population_ex(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_dataset* ds,
                             const int32_t* genes, const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx, double* acc,
                             double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated) {
    return cmoop_eval_population_kd(cfg, aug, loss, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr, epochs_run, val_loss,
                                    seconds, evaluated);
}

int cmoop_eval_population_kd(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                             const cmoop_dataset* ds, const int32_t* genes, const uint32_t* seeds, int32_t n, cmoop_next_fn next,
                             void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss,
                             double* seconds, int32_t* evaluated) {
    return cmoop_eval_population_opt(cfg, aug, loss, distill, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr, epochs_run,
                                     val_loss, seconds, evaluated);
}

int cmoop_eval_population_opt(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                              const cmoop_optim* optim, const cmoop_dataset* ds, const int32_t* genes, const uint32_t* seeds, int32_t n,
                              cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run,
                              double* val_loss, double* seconds, int32_t* evaluated) {
    return cmoop_eval_population_avg(cfg, aug, loss, distill, optim, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr,
                                     epochs_run, val_loss, seconds, evaluated);
}

int cmoop_eval_population_avg(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                              const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_dataset* ds, const int32_t* genes,
                              const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr,
                              int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated) {
    return cmoop_eval_population_op(cfg, aug, loss, distill, optim, ema, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr,
                                    epochs_run, val_loss, seconds, evaluated, nullptr);
}

int cmoop_eval_population_op(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                             const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_dataset* ds,
                             const int32_t* genes, const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx, double* acc,
                             double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated,
                             double* opoint) {
    return cmoop_eval_population_q(cfg, aug, loss, distill, optim, ema, op, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr,
                                   epochs_run, val_loss, seconds, evaluated, opoint, nullptr);
}

int cmoop_eval_population_q(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                            const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_quant* q,
                            const cmoop_dataset* ds, const int32_t* genes, const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx,
                            double* acc, double* size_mb, double* fpr, int32_t* epochs_run, double* val_loss, double* seconds,
                            int32_t* evaluated, double* opoint, double* quant) {
    return cmoop_eval_population_p(cfg, aug, loss, distill, optim, ema, op, q, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr,
                                   epochs_run, val_loss, seconds, evaluated, opoint, quant, nullptr);
}

int cmoop_eval_population_p(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                            const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_quant* q,
                            const cmoop_prune* pr, const cmoop_dataset* ds, const int32_t* genes, const uint32_t* seeds, int32_t n,
                            cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr, int32_t* epochs_run,
                            double* val_loss, double* seconds, int32_t* evaluated, double* opoint, double* quant, double* prune) {
    return cmoop_eval_population_aq(cfg, aug, loss, distill, optim, ema, op, q, pr, nullptr, ds, genes, seeds, n, next, ctx, acc, size_mb,
                                    fpr, epochs_run, val_loss, seconds, evaluated, opoint, quant, prune);
}

int cmoop_eval_population_aq(const cmoop_config* cfg, const cmoop_augment* aug, const cmoop_loss* loss, const cmoop_distill* distill,
                             const cmoop_optim* optim, const cmoop_ema* ema, const cmoop_opoint* op, const cmoop_quant* q,
                             const cmoop_prune* pr, const cmoop_actquant* aq, const cmoop_dataset* ds, const int32_t* genes,
                             const uint32_t* seeds, int32_t n, cmoop_next_fn next, void* ctx, double* acc, double* size_mb, double* fpr,
                             int32_t* epochs_run, double* val_loss, double* seconds, int32_t* evaluated, double* opoint, double* quant,
                             double* prune) {
    return guard([&] {
        eval_population_abi(cfg, aug, loss, distill, optim, ema, op, q, pr, aq, ds, genes, seeds, n, next, ctx, acc, size_mb, fpr,
                            epochs_run, val_loss, seconds, evaluated, opoint, quant, prune);
    });
}

// ---- activation fake quantisation ----------------------------------------------------
int cmoop_actquant_default(cmoop_actquant* aq) {
    return guard([&] {
        CMOOP_REQUIRE(aq != nullptr, "actquant config is NULL");
        std::memset(aq, 0, sizeof(*aq));
        aq->momentum = 0.99f;
    });
}

int cmoop_actquant_check(const cmoop_actquant* aq) {
    return guard([&] { actquant_check(to_actquant(aq)); });
}

int cmoop_actquant_sites(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int32_t* rows, int32_t cap,
                         int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(gene != nullptr && T >= 1 && F >= 1, "actquant_sites: NULL gene or an empty patch");
        NetConfig cfg;
        cfg.variant = variant; cfg.classes = classes;
        const NetPlan plan = plan_net(gene, cfg, T, F);
        CMOOP_REQUIRE(rows && cap >= plan.n_sites, "actquant_sites: the rows buffer is too small");
        for (int i = 0; i < (int)plan.acts.size(); ++i) {
            const Act& a = plan.acts[i];
            if (a.site < 0) continue;
            const int32_t v[4] = {i, a.H, a.W, a.C};
            std::memcpy(rows + 4 * (size_t)a.site, v, sizeof(v));
        }
        if (count) *count = plan.n_sites;
    });
}

// the body of cmoop_fake_quant_act(_time): record and partials on pooled buffers, then avg_ms null: one call, else timed calls
static void fake_quant_act_abi(float* x, int64_t n, int32_t bits, const float* a_in, cmoop_act_range* record, float momentum,
                               int32_t iters, double* avg_ms) {
    ActQuantCfg c;
    c.bits = bits; c.momentum = momentum;
    actquant_check(c);
    CMOOP_REQUIRE(actquant_enabled(c), "fake_quant_act: bits must be in [2, 8]");
    CMOOP_REQUIRE(n >= 0 && n <= ACT_QUANT_MAX_ELEMS, "fake_quant_act: n must stay below 2^31 elements");
    const bool tracked = a_in != nullptr;
    CMOOP_REQUIRE(tracked || record || avg_ms, "fake_quant_act: batch mode needs record_inout");
    if (n == 0) { if (avg_ms) *avg_ms = 0.0; return; }
    CMOOP_REQUIRE(x != nullptr && reinterpret_cast<uintptr_t>(x) % 4 == 0, "fake_quant_act: x_dev is NULL or not aligned to 4 bytes");
    ActRange rec{0.f, 0.f, 0, 0};
    if (record) std::memcpy(&rec, record, sizeof(rec));
    CMOOP_REQUIRE(rec.count >= 0, "fake_quant_act: the record's count must not be negative");
    if (tracked) rec.r = *a_in;
    const EmaPair m = actquant_rates(c.momentum);
    hipStream_t s = lib_stream();
    PoolScope pool(s);
    ActRange* rec_dev = pool.get<ActRange>(sizeof(ActRange));
    uint32_t* partials = pool.get<uint32_t>((size_t)ACT_QUANT_MAX_BLOCKS * 4);
    CMOOP_HIP(hipMemcpyAsync(rec_dev, &rec, sizeof(rec), hipMemcpyHostToDevice, s));
    CMOOP_HIP(hipStreamSynchronize(s));
    auto once = [&] { launch_fake_quant_act(x, n, c.bits, tracked, partials, rec_dev, m.mf, m.omf, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    if (record && !tracked) CMOOP_HIP(hipMemcpyAsync(record, rec_dev, sizeof(rec), hipMemcpyDeviceToHost, s));
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_fake_quant_act(float* x_dev, int64_t n, int32_t bits, const float* a_in, cmoop_act_range* record_inout, float momentum) {
    return guard([&] { fake_quant_act_abi(x_dev, n, bits, a_in, record_inout, momentum, 0, nullptr); });
}

int cmoop_fake_quant_act_time(float* x_dev, int64_t n, int32_t bits, const float* a_in, float momentum, int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "fake_quant_act_time: iters >= 1 and avg_ms");
        fake_quant_act_abi(x_dev, n, bits, a_in, nullptr, momentum, iters, avg_ms);
    });
}

// ---- integer inference ---------------------------------------------------------------
int cmoop_fake_quant_act_codes(float* x_dev, int64_t n, int32_t bits, const float* a_in, int8_t* codes_dev) {
    return guard([&] {
        CMOOP_REQUIRE(a_in != nullptr, "fake_quant_act_codes: tracked mode only (a_in is required)");
        CMOOP_REQUIRE(bits >= 2 && bits <= 8, "fake_quant_act_codes: bits must be in [2, 8]");
        CMOOP_REQUIRE(n >= 0 && n <= ACT_QUANT_MAX_ELEMS, "fake_quant_act_codes: n must stay below 2^31 elements");
        if (n == 0) return;
        CMOOP_REQUIRE(x_dev != nullptr && reinterpret_cast<uintptr_t>(x_dev) % 4 == 0, "fake_quant_act_codes: x_dev is NULL or not aligned to 4 bytes");
        const ActRange rec{0.f, *a_in, 0, 0};
        hipStream_t s = lib_stream();
        PoolScope pool(s);
        ActRange* rec_dev = pool.get<ActRange>(sizeof(ActRange));
        CMOOP_HIP(hipMemcpyAsync(rec_dev, &rec, sizeof(rec), hipMemcpyHostToDevice, s));
        CMOOP_HIP(hipStreamSynchronize(s));
        launch_fake_quant_act(x_dev, n, bits, true, nullptr, rec_dev, 0.f, 0.f, s, codes_dev);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_fake_quant_act_codes_time(float* x_dev, int64_t n, int32_t bits, const float* a_in, int8_t* codes_dev, int32_t iters,
                                    double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "fake_quant_act_codes_time: iters >= 1 and avg_ms");
        CMOOP_REQUIRE(a_in != nullptr, "fake_quant_act_codes_time: tracked mode only (a_in is required)");
        CMOOP_REQUIRE(bits >= 2 && bits <= 8, "fake_quant_act_codes_time: bits must be in [2, 8]");
        CMOOP_REQUIRE(n >= 1 && n <= ACT_QUANT_MAX_ELEMS, "fake_quant_act_codes_time: n must be in [1, 2^31)");
        CMOOP_REQUIRE(x_dev != nullptr && reinterpret_cast<uintptr_t>(x_dev) % 4 == 0, "fake_quant_act_codes_time: x_dev is NULL or not aligned to 4 bytes");
        const ActRange rec{0.f, *a_in, 0, 0};
        hipStream_t s = lib_stream();
        PoolScope pool(s);
        ActRange* rec_dev = pool.get<ActRange>(sizeof(ActRange));
        CMOOP_HIP(hipMemcpyAsync(rec_dev, &rec, sizeof(rec), hipMemcpyHostToDevice, s));
        CMOOP_HIP(hipStreamSynchronize(s));
        *avg_ms = time_launches(s, iters, [&] { launch_fake_quant_act(x_dev, n, bits, true, nullptr, rec_dev, 0.f, 0.f, s, codes_dev); });
    });
}

int cmoop_conv_fwd_i8(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                      int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_i8_fwd(I8Layer{true, B, H, W, Cin, Cout, KS, stride}, xq_dev, wq_dev, s_x, nullptr, 0, s_w_dev, bias_dev, y_dev, relu, nullptr, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_dense_fwd_i8(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                       int32_t M, int32_t N, int32_t K, int32_t relu) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_i8_fwd(I8Layer::dense(M, N, K), xq_dev, wq_dev, s_x, nullptr, 0, s_w_dev, bias_dev, y_dev, relu, nullptr, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_conv_fwd_i8_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                           int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu,
                           int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "conv_fwd_i8_time: iters >= 1 and avg_ms");
        hipStream_t s = lib_stream();
        const I8Layer L{true, B, H, W, Cin, Cout, KS, stride};
        *avg_ms = time_launches(s, iters, [&] { launch_i8_fwd(L, xq_dev, wq_dev, s_x, nullptr, 0, s_w_dev, bias_dev, y_dev, relu, nullptr, s); });
    });
}

int cmoop_dense_fwd_i8_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev, float* y_dev,
                            int32_t M, int32_t N, int32_t K, int32_t relu, int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "dense_fwd_i8_time: iters >= 1 and avg_ms");
        hipStream_t s = lib_stream();
        const I8Layer L = I8Layer::dense(M, N, K);
        *avg_ms = time_launches(s, iters, [&] { launch_i8_fwd(L, xq_dev, wq_dev, s_x, nullptr, 0, s_w_dev, bias_dev, y_dev, relu, nullptr, s); });
    });
}

int cmoop_scale_shift_time(const float* x_dev, float* y_dev, const float* scale_dev, const float* shift_dev, int64_t M, int32_t C, int32_t relu,
                           int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "scale_shift_time: iters >= 1 and avg_ms");
        CMOOP_REQUIRE(M >= 1 && C >= 4 && C % 4 == 0, "scale_shift_time: M >= 1 and C a multiple of 4");
        CMOOP_REQUIRE(x_dev && y_dev && scale_dev && shift_dev, "scale_shift_time: NULL buffer");
        hipStream_t s = lib_stream();
        *avg_ms = time_launches(s, iters, [&] { launch_scale_shift(x_dev, y_dev, scale_dev, shift_dev, M, C, relu, s); });
    });
}

// The plan rows of one level of integer inference -- 0: cmoop_int8_ops [count][16], 1: cmoop_int8_dw_ops [count][16], 2:
// cmoop_int8_fused_ops [count][20], a level-0 row and four more columns.  Only level 0 refuses a NULL rows for an empty plan
static const char* const INT8_PLAN_NAME[3] = {"int8_ops", "int8_dw_ops", "int8_fused_ops"};

static void int8_rows_abi(int level, const NetPlan& plan, int64_t* rows, int32_t cap, int32_t* count) {
    std::vector<int64_t> v;
    auto matrix_row = [&](const Int8Op& o) {
        const Op& op = plan.ops[o.op];
        v.insert(v.end(), {o.op, op.kind == OP_DENSE ? 1 : 0, o.in, o.out, o.site, op.H, op.W, op.Cin, op.Cout, op.KS, op.stride, op.relu, op.w_off,
                           op.b_off, o.scale_off, 0});
    };
    if (level == 0) {
        for (const Int8Op& o : int8_ops(plan)) matrix_row(o);
    } else if (level == 1) {
        for (const Int8DwOp& o : int8_dw_ops(plan)) {
            const Op& op = plan.ops[o.op];
            v.insert(v.end(), {o.op, 2, o.in, o.out, o.site, op.H, op.W, op.Cin, op.Cin, op.KS, 1, 0, op.w_off, -1, o.scale_off, o.out_site});
        }
    } else {
        for (const Int8FusedOp& o : int8_fused_ops(plan)) {
            matrix_row(o.i8);
            v.insert(v.end(), {o.bn, o.relu_after, o.out_site, o.site_act});
        }
    }
    const int32_t n = (int32_t)(v.size() / (level == 2 ? 20 : 16));
    CMOOP_REQUIRE((rows || (level != 0 && n == 0)) && cap >= n, std::string(INT8_PLAN_NAME[level]) + ": the rows buffer is too small");
    if (n) std::memcpy(rows, v.data(), v.size() * sizeof(int64_t));
    if (count) *count = n;
}

static int int8_plan_abi(int level, const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows, int32_t cap,
                         int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(gene != nullptr && T >= 1 && F >= 1, std::string(INT8_PLAN_NAME[level]) + ": NULL gene or an empty patch");
        NetConfig cfg;
        cfg.variant = variant; cfg.classes = classes;
        int8_rows_abi(level, plan_net(gene, cfg, T, F), rows, cap, count);
    });
}

static int int8_net_plan_abi(int level, cmoop_net* h, int64_t* rows, int32_t cap, int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, std::string(INT8_PLAN_NAME[level]) + ": NULL net");
        int8_rows_abi(level, h->net->plan(), rows, cap, count);
    });
}

int cmoop_int8_ops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows, int32_t cap, int32_t* count) {
    return int8_plan_abi(0, gene, variant, classes, T, F, rows, cap, count);
}
int cmoop_int8_dw_ops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows, int32_t cap, int32_t* count) {
    return int8_plan_abi(1, gene, variant, classes, T, F, rows, cap, count);
}
int cmoop_int8_fused_ops(const int32_t gene[6], int32_t variant, int32_t classes, int32_t T, int32_t F, int64_t* rows, int32_t cap, int32_t* count) {
    return int8_plan_abi(2, gene, variant, classes, T, F, rows, cap, count);
}

// the lone requantising conv / dense layer L under the range *a_out; avg_ms non-null: timed over `iters` launches
static void fwd_i8_q_abi(const I8Layer& L, const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                         const float* bn_scale_dev, const float* bn_shift_dev, int32_t relu, int32_t relu_after, int32_t out_bits,
                         const float* a_out, float* y_dev, int8_t* codes_dev, int32_t iters, double* avg_ms) {
    const std::string who = L.conv ? "conv_fwd_i8_q" : "dense_fwd_i8_q";
    CMOOP_REQUIRE(a_out != nullptr, who + ": the output range (a_out) is required");
    CMOOP_REQUIRE(out_bits >= 2 && out_bits <= 8, who + ": output bits must be in [2, 8]");
    hipStream_t s = lib_stream();
    PoolScope pool(s);
    const ActRange rec{0.f, *a_out, 0, 0};
    ActRange* rec_dev = pool.get<ActRange>(sizeof(ActRange));
    CMOOP_HIP(hipMemcpyAsync(rec_dev, &rec, sizeof(rec), hipMemcpyHostToDevice, s));
    CMOOP_HIP(hipStreamSynchronize(s));            // rec is this frame's
    const I8Requant rq{bn_scale_dev, bn_shift_dev, relu_after, rec_dev, out_bits, codes_dev};
    auto once = [&] { launch_i8_fwd(L, xq_dev, wq_dev, s_x, nullptr, 0, s_w_dev, bias_dev, y_dev, relu, &rq, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_conv_fwd_i8_q(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                        const float* bn_scale_dev, const float* bn_shift_dev, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout,
                        int32_t KS, int32_t stride, int32_t relu, int32_t relu_after, int32_t out_bits, const float* a_out, float* y_dev,
                        int8_t* codes_dev) {
    return guard([&] {
        fwd_i8_q_abi(I8Layer{true, B, H, W, Cin, Cout, KS, stride}, xq_dev, wq_dev, s_x, s_w_dev, bias_dev, bn_scale_dev, bn_shift_dev, relu,
                   relu_after, out_bits, a_out, y_dev, codes_dev, 0, nullptr);
    });
}

int cmoop_conv_fwd_i8_q_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                             const float* bn_scale_dev, const float* bn_shift_dev, int32_t B, int32_t H, int32_t W, int32_t Cin,
                             int32_t Cout, int32_t KS, int32_t stride, int32_t relu, int32_t relu_after, int32_t out_bits, const float* a_out,
                             float* y_dev, int8_t* codes_dev, int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "conv_fwd_i8_q_time: iters >= 1 and avg_ms");
        fwd_i8_q_abi(I8Layer{true, B, H, W, Cin, Cout, KS, stride}, xq_dev, wq_dev, s_x, s_w_dev, bias_dev, bn_scale_dev, bn_shift_dev, relu,
                   relu_after, out_bits, a_out, y_dev, codes_dev, iters, avg_ms);
    });
}

int cmoop_dense_fwd_i8_q(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                         const float* bn_scale_dev, const float* bn_shift_dev, int32_t M, int32_t N, int32_t K, int32_t relu,
                         int32_t relu_after, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev) {
    return guard([&] {
        fwd_i8_q_abi(I8Layer::dense(M, N, K), xq_dev, wq_dev, s_x, s_w_dev, bias_dev, bn_scale_dev, bn_shift_dev, relu, relu_after, out_bits,
                   a_out, y_dev, codes_dev, 0, nullptr);
    });
}

int cmoop_dense_fwd_i8_q_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, const float* bias_dev,
                              const float* bn_scale_dev, const float* bn_shift_dev, int32_t M, int32_t N, int32_t K, int32_t relu,
                              int32_t relu_after, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev, int32_t iters,
                              double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "dense_fwd_i8_q_time: iters >= 1 and avg_ms");
        fwd_i8_q_abi(I8Layer::dense(M, N, K), xq_dev, wq_dev, s_x, s_w_dev, bias_dev, bn_scale_dev, bn_shift_dev, relu, relu_after, out_bits,
                   a_out, y_dev, codes_dev, iters, avg_ms);
    });
}

// the lone integer depthwise layer; avg_ms non-null: timed over `iters` launches
static void dwconv_fwd_i8_abi(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, int32_t B, int32_t H, int32_t W,
                              int32_t C, int32_t KS, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev, int32_t iters,
                              double* avg_ms) {
    CMOOP_REQUIRE(a_out || !codes_dev, "dwconv_fwd_i8: codes need an output range (a_out)");
    CMOOP_REQUIRE(!a_out || (out_bits >= 2 && out_bits <= 8), "dwconv_fwd_i8: output bits must be in [2, 8]");
    hipStream_t s = lib_stream();
    PoolScope pool(s);
    ActRange* rec_dev = nullptr;
    if (a_out) {
        const ActRange rec{0.f, *a_out, 0, 0};
        rec_dev = pool.get<ActRange>(sizeof(ActRange));
        CMOOP_HIP(hipMemcpyAsync(rec_dev, &rec, sizeof(rec), hipMemcpyHostToDevice, s));
        CMOOP_HIP(hipStreamSynchronize(s));        // rec is this frame's
    }
    auto once = [&] { launch_dwconv_i8_fwd(xq_dev, wq_dev, s_x, nullptr, 0, s_w_dev, rec_dev, out_bits, y_dev, codes_dev, B, H, W, C, KS, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_dwconv_fwd_i8(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, int32_t B, int32_t H, int32_t W,
                        int32_t C, int32_t KS, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev) {
    return guard([&] { dwconv_fwd_i8_abi(xq_dev, wq_dev, s_x, s_w_dev, B, H, W, C, KS, out_bits, a_out, y_dev, codes_dev, 0, nullptr); });
}

int cmoop_dwconv_fwd_i8_time(const int8_t* xq_dev, const int8_t* wq_dev, float s_x, const float* s_w_dev, int32_t B, int32_t H, int32_t W,
                             int32_t C, int32_t KS, int32_t out_bits, const float* a_out, float* y_dev, int8_t* codes_dev, int32_t iters,
                             double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "dwconv_fwd_i8_time: iters >= 1 and avg_ms");
        dwconv_fwd_i8_abi(xq_dev, wq_dev, s_x, s_w_dev, B, H, W, C, KS, out_bits, a_out, y_dev, codes_dev, iters, avg_ms);
    });
}

// ---- quantisation-aware training ---------------------------------------------------
int cmoop_quant_default(cmoop_quant* q) {
    return guard([&] {
        CMOOP_REQUIRE(q != nullptr, "quant config is NULL");
        std::memset(q, 0, sizeof(*q));
    });
}

int cmoop_quant_check(const cmoop_quant* q) {
    return guard([&] { quant_check(to_quant(q)); });
}

static QuantTable quant_table_of(const int32_t gene[6], int32_t variant, int32_t classes) {
    CMOOP_REQUIRE(gene != nullptr, "quant_table: NULL gene");
    NetConfig cfg;
    cfg.variant = variant; cfg.classes = classes;
    return quant_table(plan_net(gene, cfg, 26, 10));   // offsets and kernel shapes do not depend on the patch size
}

int cmoop_quant_table(const int32_t gene[6], int32_t variant, int32_t classes, int64_t* rows, int32_t cap, int32_t* count,
                      int64_t* total_channels) {
    return guard([&] {
        const QuantTable tab = quant_table_of(gene, variant, classes);
        CMOOP_REQUIRE(rows && cap >= (int32_t)tab.rows.size(), "quant_table: the rows buffer is too small");
        for (size_t i = 0; i < tab.rows.size(); ++i) {
            const QuantRow& r = tab.rows[i];
            const int64_t v[5] = {r.off, r.channels, r.len, r.chan_stride, r.elem_stride};
            std::memcpy(rows + 5 * i, v, sizeof(v));
        }
        if (count) *count = (int32_t)tab.rows.size();
        if (total_channels) *total_channels = tab.total_channels;
    });
}

int cmoop_quant_size_bytes(const int32_t gene[6], int32_t variant, int32_t classes, int32_t bits, int64_t* out) {
    return guard([&] {
        CMOOP_REQUIRE(out != nullptr, "quant_size_bytes: NULL output");
        *out = quant_size_bytes(quant_table_of(gene, variant, classes), param_count(gene, variant, classes), bits);
    });
}

// the body of cmoop_quantize_weights(_time): the table uploaded to a pooled buffer, then iters < 0: one launch, else timed launches
static void quantize_weights_abi(const cmoop_quant* q, const float* w, int64_t n, const int64_t* rows, int32_t count, float* wq,
                                 int8_t* codes, float* scales, int32_t iters, double* avg_ms) {
    const QuantCfg c = to_quant(q);
    quant_check(c);
    CMOOP_REQUIRE(quant_enabled(c), "quantize_weights: the config is disabled (bits 0)");
    const QuantTable tab = to_quant_table(rows, count, n);
    if (tab.blocks == 0) { if (avg_ms) *avg_ms = 0.0; return; }
    CMOOP_REQUIRE(w && wq, "quantize_weights: NULL arena");
    hipStream_t s = lib_stream();
    PoolScope pool(s);
    QuantRow* rows_dev = pool.get<QuantRow>(tab.rows.size() * sizeof(QuantRow));
    CMOOP_HIP(hipMemcpyAsync(rows_dev, tab.rows.data(), tab.rows.size() * sizeof(QuantRow), hipMemcpyHostToDevice, s));
    CMOOP_HIP(hipStreamSynchronize(s));
    auto once = [&] { launch_quantize_weights(w, wq, codes, scales, tab, rows_dev, c.bits, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_quantize_weights(const cmoop_quant* q, const float* w_dev, int64_t n, const int64_t* rows_host, int32_t count, float* wq_dev,
                           int8_t* codes_dev, float* scales_dev) {
    return guard([&] { quantize_weights_abi(q, w_dev, n, rows_host, count, wq_dev, codes_dev, scales_dev, 0, nullptr); });
}

int cmoop_quantize_weights_time(const cmoop_quant* q, const float* w_dev, int64_t n, const int64_t* rows_host, int32_t count,
                                float* wq_dev, int8_t* codes_dev, float* scales_dev, int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "quantize_weights_time: iters >= 1 and avg_ms");
        quantize_weights_abi(q, w_dev, n, rows_host, count, wq_dev, codes_dev, scales_dev, iters, avg_ms);
    });
}

// ---- magnitude pruning in training -------------------------------------------------
int cmoop_prune_default(cmoop_prune* p) {
    return guard([&] {
        CMOOP_REQUIRE(p != nullptr, "prune config is NULL");
        std::memset(p, 0, sizeof(*p));
        p->skip_small = 1;
    });
}

int cmoop_prune_check(const cmoop_prune* p) {
    return guard([&] { prune_check(to_prune(p)); });
}

int cmoop_prune_sparsity_at(const cmoop_prune* p, int64_t it, double* out) {
    return guard([&] {
        CMOOP_REQUIRE(out != nullptr, "prune_sparsity_at: NULL output");
        const PruneCfg c = to_prune(p);
        prune_check(c);
        *out = prune_sparsity_at(c, it);
    });
}

static NetPlan prune_plan_of(const int32_t gene[6], int32_t variant, int32_t classes) {
    CMOOP_REQUIRE(gene != nullptr, "prune_table: NULL gene");
    NetConfig cfg;
    cfg.variant = variant; cfg.classes = classes;
    return plan_net(gene, cfg, 26, 10);   // offsets and kernel shapes do not depend on the patch size
}

int cmoop_prune_table(const int32_t gene[6], int32_t variant, int32_t classes, int32_t skip_small, int64_t* rows, int32_t cap,
                      int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(skip_small == 0 || skip_small == 1, "prune: skip_small must be 0 or 1");
        const PruneTable tab = prune_table(prune_plan_of(gene, variant, classes), skip_small != 0);
        CMOOP_REQUIRE(rows && cap >= (int32_t)tab.rows.size(), "prune_table: the rows buffer is too small");
        for (size_t i = 0; i < tab.rows.size(); ++i) {
            const int64_t v[3] = {tab.rows[i].off, tab.rows[i].len, tab.rows[i].k};
            std::memcpy(rows + 3 * i, v, sizeof(v));
        }
        if (count) *count = (int32_t)tab.rows.size();
    });
}

int cmoop_prune_size_bytes(const int32_t gene[6], int32_t variant, int32_t classes, double sparsity, int32_t bits, int32_t skip_small,
                           int64_t* out) {
    return guard([&] {
        CMOOP_REQUIRE(out != nullptr, "prune_size_bytes: NULL output");
        CMOOP_REQUIRE(skip_small == 0 || skip_small == 1, "prune: skip_small must be 0 or 1");
        const NetPlan plan = prune_plan_of(gene, variant, classes);
        *out = prune_size_bytes(prune_table(plan, skip_small != 0), param_count(gene, variant, classes), sparsity, bits,
                                bits ? quant_table(plan).total_channels : 0);
    });
}

// the body of cmoop_prune_weights(_time): table and zeroed workspace on pooled buffers, then iters < 1: one call, else timed calls
static void prune_weights_abi(const float* w, int64_t n, const int64_t* rows, int32_t count, double sp, float* out, uint32_t* zeros,
                              int32_t* launches, int32_t iters, double* avg_ms) {
    CMOOP_REQUIRE(sp >= 0.0 && sp < 1.0, "prune_weights: s must be in [0, 1)");
    const PruneTable tab = to_prune_table(rows, count, n);
    if (launches) *launches = 0;
    if (tab.blocks == 0) { if (avg_ms) *avg_ms = 0.0; return; }
    CMOOP_REQUIRE(w && out, "prune_weights: NULL arena");
    hipStream_t s = lib_stream();
    PoolScope pool(s);
    PruneRow* rows_dev = pool.get<PruneRow>(tab.rows.size() * sizeof(PruneRow));
    uint32_t* words = pool.get<uint32_t>(prune_workspace_words(count) * sizeof(uint32_t));
    PruneWorkspace ws;
    prune_workspace_init(ws, words, count, s);   // once per workspace, not per call: the calls below keep it clean themselves
    CMOOP_HIP(hipMemcpyAsync(rows_dev, tab.rows.data(), tab.rows.size() * sizeof(PruneRow), hipMemcpyHostToDevice, s));
    CMOOP_HIP(hipStreamSynchronize(s));
    int did = 0;
    auto once = [&] { did = launch_prune_weights(w, out, zeros, tab, rows_dev, ws, sp, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    if (launches) *launches = did;
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_prune_weights(const float* w_dev, int64_t n, const int64_t* rows_host, int32_t count, double s, float* out_dev,
                        uint32_t* zeros_dev, int32_t* launches) {
    return guard([&] { prune_weights_abi(w_dev, n, rows_host, count, s, out_dev, zeros_dev, launches, 0, nullptr); });
}

int cmoop_prune_weights_time(const float* w_dev, int64_t n, const int64_t* rows_host, int32_t count, double s, float* out_dev,
                             uint32_t* zeros_dev, int32_t iters, double* avg_ms) {
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && iters >= 1, "prune_weights_time: iters >= 1 and avg_ms");
        prune_weights_abi(w_dev, n, rows_host, count, s, out_dev, zeros_dev, nullptr, iters, avg_ms);
    });
}

// ---- operating-point read-out ----------------------------------------------------
int cmoop_opoint_default(cmoop_opoint* op) {
    return guard([&] {
        CMOOP_REQUIRE(op != nullptr, "opoint config is NULL");
        std::memset(op, 0, sizeof(*op));
    });
}

int cmoop_opoint_check(const cmoop_opoint* op) {
    return guard([&] { opoint_check(to_opoint(op)); });
}

int cmoop_roc_counts(const float* probs, const int32_t* y, int64_t n, int32_t C, int32_t* counts) {
    return guard([&] {
        opoint_check_shape(n, C);
        CMOOP_REQUIRE(n == 0 || (probs && y && counts), "roc_counts: NULL buffer");
        if (n == 0) return;
        hipStream_t s = lib_stream();
        PoolScope pool(s);
        uint32_t* key = pool.get<uint32_t>((size_t)n * C * 4);
        launch_score_keys(probs, key, n, C, s);
        launch_roc_counts(key, y, counts, n, C, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_operating_point(const float* probs, const int32_t* y, int64_t n, int32_t C, const cmoop_opoint* op,
                          cmoop_opoint_class* classes, double* summary) {
    return guard([&] {
        const OpointCfg c = to_opoint(op);
        opoint_check(c);
        operating_point(probs, y, n, C, c.recall, as_classes(classes), summary, lib_stream());
    });
}

int cmoop_operating_point_time(const float* probs, const int32_t* y, int64_t n, int32_t C, const cmoop_opoint* op, int32_t iters,
                               double* avg_ms) {
    return guard([&] {
        const OpointCfg c = to_opoint(op);
        opoint_check(c);
        opoint_check_shape(n, C);
        CMOOP_REQUIRE(n >= 1 && probs && y && avg_ms && iters >= 1, "operating_point_time: n >= 1, iters >= 1 and every buffer");
        hipStream_t s = lib_stream();
        PoolScope pool(s);
        uint32_t* key = pool.get<uint32_t>((size_t)n * C * 4);
        int32_t* cnt = pool.get<int32_t>((size_t)n * C * 16);
        OpointClass* rec = pool.get<OpointClass>((size_t)C * sizeof(OpointClass));
        auto keys = [&] { launch_score_keys(probs, key, n, C, s); };
        auto counts = [&] { launch_roc_counts(key, y, cnt, n, C, s); };
        auto select = [&] { launch_opoint_select(key, y, cnt, n, C, c.recall, rec, s); };
        avg_ms[0] = time_launches(s, iters, [&] { keys(); counts(); select(); });
        avg_ms[1] = time_launches(s, iters, keys);
        avg_ms[2] = time_launches(s, iters, counts);
        avg_ms[3] = time_launches(s, iters, select);
    });
}

int cmoop_opoint_summary(const cmoop_opoint_class* classes, int32_t C, double* summary) {
    return guard([&] {
        CMOOP_REQUIRE(classes && summary, "opoint_summary: NULL argument");
        CMOOP_REQUIRE(C >= 1 && C <= OPOINT_MAX_CLASSES, "opoint_summary: classes must be in [1, 64]");
        opoint_summary(as_classes(const_cast<cmoop_opoint_class*>(classes)), C, summary);
    });
}

// ---- weight EMA ------------------------------------------------------------------
int cmoop_ema_default(cmoop_ema* ema) {
    return guard([&] {
        CMOOP_REQUIRE(ema != nullptr, "ema config is NULL");
        std::memset(ema, 0, sizeof(*ema));
    });
}

int cmoop_ema_check(const cmoop_ema* ema) {
    return guard([&] { ema_check(to_ema(ema)); });
}

int cmoop_ema_rates(const cmoop_ema* ema, int64_t iteration, double* m, float* mf, float* omf) {
    return guard([&] {
        const EmaCfg c = to_ema(ema);
        ema_check(c);
        const EmaRates r = ema_rates(c, iteration);
        if (m) *m = r.m;
        if (mf) *mf = r.mf;
        if (omf) *omf = r.omf;
    });
}

int cmoop_ema_update(const cmoop_ema* ema, int64_t iteration, float* a_dev, const float* w_dev, const uint8_t* kinds_dev, int64_t n) {
    return guard([&] {
        CMOOP_REQUIRE(n >= 0 && (n == 0 || (a_dev && w_dev)), "ema_update: n >= 0 and both arenas");
        const EmaCfg c = to_ema(ema);
        ema_check(c);
        const EmaRates r = ema_rates(c, iteration);
        hipStream_t s = lib_stream();
        launch_ema(a_dev, w_dev, kinds_dev, n, r.mf, r.omf, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

// ---- optimiser options ----------------------------------------------------------
int cmoop_optim_default(cmoop_optim* optim) {
    return guard([&] {
        CMOOP_REQUIRE(optim != nullptr, "optim config is NULL");
        std::memset(optim, 0, sizeof(*optim));
    });
}

int cmoop_optim_check(const cmoop_optim* optim) {
    return guard([&] { optim_check(to_optim(optim)); });
}

int cmoop_optim_rates(const cmoop_optim* optim, const cmoop_config* cfg, int64_t iteration, double* lr, float* lr_f32, float* alpha_f32) {
    return guard([&] {
        CMOOP_REQUIRE(cfg != nullptr, "optim_rates: config is NULL");
        OptimCfg c;
        if (optim) {
            c = to_optim(optim);
            optim_check(c);
        }
        const OptimRates r = optim_rates(c, cfg->lr, cfg->beta1, cfg->beta2, iteration);
        if (lr) *lr = r.lr;
        if (lr_f32) *lr_f32 = r.lr_f32;
        if (alpha_f32) *alpha_f32 = r.alpha_f32;
    });
}

int cmoop_param_kinds(const int32_t gene[6], int32_t variant, int32_t classes, uint8_t* kinds, int64_t n) {
    return guard([&] {
        CMOOP_REQUIRE(gene && kinds, "param_kinds: NULL argument");
        NetConfig c;
        c.variant = variant; c.classes = classes;
        const std::vector<uint8_t> k = plan_net(gene, c, 32, 32).param_kinds();   // parameter offsets do not depend on T, F
        CMOOP_REQUIRE((int64_t)k.size() == n, "param_kinds: n must be the candidate's parameter count");
        std::copy(k.begin(), k.end(), kinds);
    });
}

// ---- knowledge distillation ------------------------------------------------------
int cmoop_distill_default(cmoop_distill* distill) {
    return guard([&] {
        CMOOP_REQUIRE(distill != nullptr, "distill config is NULL");
        const DistillCfg c;
        std::memset(distill, 0, sizeof(*distill));
        distill->alpha = c.alpha; distill->temperature = c.temperature;
    });
}

int cmoop_distill_check(const cmoop_distill* distill, int32_t classes, int64_t n_train) {
    return guard([&] { distill_check(to_distill(distill), classes, n_train); });
}

int cmoop_teacher_targets(const cmoop_loss* loss, const float* zt_dev, const int32_t* idx_dev, int64_t row0, int64_t n_rows, int32_t B,
                          int32_t C, double temperature, uint32_t seed, uint32_t step, float* q_dev) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && B < (1 << 27) && C >= 1 && row0 >= 0 && n_rows >= 1, "teacher_targets: 0 <= B < 2^27, C >= 1, row0 >= 0, n_rows >= 1");
        CMOOP_REQUIRE(B == 0 || (zt_dev && q_dev), "teacher_targets: NULL buffer");
        DistillCfg dc;
        dc.temperature = temperature;
        distill_check(dc, C, 0);
        LossCfg c;
        if (loss) {
            c = to_loss(loss);
            c.class_weight = nullptr;           // not read here
            loss_check(c, 1);
        }
        hipStream_t s = lib_stream();
        Scratch m(s);
        const MixupParams mp = scratch_mixup(c, loss_mixup_on(c) ? m.floats(MIXUP_TABLE) : nullptr, s);
        launch_teacher_targets(zt_dev, BatchRows{idx_dev, row0, n_rows}, B, C, (float)temperature, mp, seed, step, q_dev, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_softmax_ce_distill(const float* z, const float* t, const float* w, const int32_t* primary, const float* q, double alpha,
                             double temperature, int32_t B, int32_t C, float* dz, double* acc, int32_t* preds) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && C >= 1, "softmax_ce_distill: B >= 0, C >= 1");
        CMOOP_REQUIRE(B == 0 || (z && t && q), "softmax_ce_distill: NULL logits, targets or teacher rows");
        DistillCfg dc;
        dc.alpha = alpha; dc.temperature = temperature;
        distill_check(dc, C, 0);
        hipStream_t s = lib_stream();
        launch_softmax_ce_distill(z, t, w, primary, q, distill_params(dc), B, C, dz, acc, preds, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

// ---- soft-target training loss ---------------------------------------------------
int cmoop_loss_default(cmoop_loss* loss) {
    return guard([&] {
        CMOOP_REQUIRE(loss != nullptr, "loss config is NULL");
        const LossCfg c;
        std::memset(loss, 0, sizeof(*loss));
        loss->label_smoothing = c.label_smoothing; loss->mixup_alpha = c.mixup_alpha; loss->mixup_p = c.mixup_p;
    });
}

int cmoop_loss_check(const cmoop_loss* loss, int32_t classes) {
    return guard([&] { loss_check(to_loss(loss), classes); });
}

int cmoop_mixup_table(double alpha, float out[1024]) {
    return guard([&] {
        CMOOP_REQUIRE(out != nullptr, "mixup_table: NULL output");
        mixup_table(alpha, out);
    });
}

int cmoop_mixup_draws(const cmoop_loss* loss, uint32_t seed, uint32_t step, int32_t B, int32_t* gate, int32_t* partner, float* lam) {
    return guard([&] {
        LossCfg c = to_loss(loss);
        c.class_weight = nullptr;               // not read here
        loss_check(c, 1);
        CMOOP_REQUIRE(B >= 0 && B < (1 << 27) && (B == 0 || (gate && partner && lam)), "mixup_draws: B must be in [0, 2^27), outputs non-NULL");
        std::vector<float> tab;
        MixupParams m;
        if (loss_mixup_on(c)) {
            tab.resize(MIXUP_TABLE);
            mixup_table(c.mixup_alpha, tab.data());
            m.on = 1;
            m.gate_thr = (uint32_t)std::floor(c.mixup_p * 16777216.0);
            m.tab = tab.data();
        }
        for (int32_t b = 0; b < B; ++b) mixup_row_draws(m, seed, step, (uint32_t)b, (uint32_t)B, gate + b, partner + b, lam + b);
    });
}

int cmoop_mixup_batch(const cmoop_loss* loss, const float* x_dev, const int32_t* idx_dev, int64_t row0, int32_t B, int32_t T, int32_t F,
                      uint32_t seed, uint32_t step, float* out_dev) {
    return guard([&] {
        LossCfg c = to_loss(loss);
        c.class_weight = nullptr;
        loss_check(c, 1);
        CMOOP_REQUIRE(B >= 0 && row0 >= 0 && T >= 1 && F >= 1 && (B == 0 || (x_dev && out_dev)), "mixup_batch: bad arguments");
        hipStream_t s = lib_stream();
        Scratch m(s);
        const MixupParams mp = scratch_mixup(c, m.floats(MIXUP_TABLE), s);
        launch_mixup_gather(x_dev, BatchRows{idx_dev, row0}, 0, out_dev, B, T, F, mp, seed, step, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_soft_targets(const cmoop_loss* loss, const int32_t* labels_dev, const int32_t* idx_dev, int64_t row0, int64_t n_rows,
                       int32_t B, int32_t C, uint32_t seed, uint32_t step, float* t_dev, float* w_dev, int32_t* primary_dev) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && C >= 1 && row0 >= 0 && n_rows >= 0, "soft_targets: B >= 0, C >= 1, row0 >= 0, n_rows >= 0");
        const LossCfg c = to_loss(loss);
        loss_check(c, C);
        CMOOP_REQUIRE(B == 0 || (labels_dev && t_dev && w_dev && primary_dev), "soft_targets: NULL buffer");
        hipStream_t s = lib_stream();
        Scratch m(s);
        const MixupParams mp = scratch_mixup(c, m.floats(MIXUP_TABLE), s);
        float* cw_dev = nullptr;
        std::vector<float> cw;
        if (c.class_weight) {
            cw.resize(C);
            for (int j = 0; j < C; ++j) cw[j] = (float)c.class_weight[j];
            cw_dev = m.floats(C);
            CMOOP_HIP(hipMemcpyAsync(cw_dev, cw.data(), (size_t)C * 4, hipMemcpyHostToDevice, s));
        }
        launch_soft_targets(labels_dev, BatchRows{idx_dev, row0, n_rows}, B, C, mp, target_params(c, C, cw_dev), seed, step, t_dev, w_dev,
                            primary_dev, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_softmax_ce_soft(const float* z, const float* t, const float* w, const int32_t* primary, int32_t B, int32_t C, float* dz,
                          double* acc, int32_t* preds) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && C >= 1, "softmax_ce_soft: B >= 0, C >= 1");
        CMOOP_REQUIRE(B == 0 || (z && t), "softmax_ce_soft: NULL logits or targets");
        hipStream_t s = lib_stream();
        launch_softmax_ce_soft(z, t, w, primary, B, C, dz, acc, preds, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

// ---- train-time augmentation ----------------------------------------------------
int cmoop_augment_default(cmoop_augment* aug) {
    return guard([&] {
        CMOOP_REQUIRE(aug != nullptr, "augment config is NULL");
        const AugmentCfg c;
        std::memset(aug, 0, sizeof(*aug));
        aug->time_shift = c.time_shift; aug->time_masks = c.time_masks; aug->time_mask_max = c.time_mask_max;
        aug->freq_masks = c.freq_masks; aug->freq_mask_max = c.freq_mask_max;
        aug->p = c.p; aug->noise_std = c.noise_std; aug->fill = c.fill;
    });
}

int cmoop_augment_check(const cmoop_augment* aug, int32_t T, int32_t F) {
    return guard([&] { augment_check(to_augment(aug), T, F); });
}

int cmoop_augment_draws(const cmoop_augment* aug, uint32_t seed, uint32_t step, int32_t b, int32_t T, int32_t F, int32_t out[18]) {
    return guard([&] {
        const AugmentCfg c = to_augment(aug);
        augment_check(c, T, F);
        CMOOP_REQUIRE(out != nullptr && b >= 0 && b < (1 << 27), "augment_draws: b must be in [0, 2^27)");
        augment_row_draws(augment_params(c), seed, step, (uint32_t)b, T, F, out);
    });
}

int cmoop_augment_batch(const cmoop_augment* aug, const float* x_dev, const int32_t* idx_dev, int64_t row0, int32_t B, int32_t T,
                        int32_t F, uint32_t seed, uint32_t step, float* out_dev) {
    return guard([&] {
        const AugmentCfg c = to_augment(aug);
        augment_check(c, T, F);
        CMOOP_REQUIRE(B >= 0 && row0 >= 0 && (B == 0 || (x_dev && out_dev)), "augment_batch: bad arguments");
        hipStream_t s = lib_stream();
        launch_augment_gather(x_dev, BatchRows{idx_dev, row0}, out_dev, B, T, F, augment_params(c), seed, step, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_plan_check(const int32_t gene[6], int32_t variant, int32_t T, int32_t F, int32_t batch) {
    return guard([&] {
        CMOOP_REQUIRE(gene && (variant >= 0 && variant <= 3) && T >= 1 && F >= 1 && batch >= 1, "plan_check: bad arguments");
        check_plan_ranges(gene, variant, T, F, batch);
    });
}

int cmoop_conv_launch_plan(int32_t op, int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride,
                           int32_t want_stats, char* name, int32_t name_cap) {
    return guard([&] {
        CMOOP_REQUIRE(name && name_cap > 0 && op >= 0 && op <= 2, "launch_plan: bad arguments");
        CMOOP_REQUIRE(B >= 1 && H >= 1 && W >= 1 && Cin >= 16 && Cout >= 1 && KS >= 1 && stride >= 1, "bad conv shape");
        // a lone layer: the split-K workspace is the launch's own geometry's (cmoop_conv_*_trainer allocate the same)
        const ConvLayer L{H, W, Cin, Cout, KS, stride};
        const std::string v = op == 0   ? L.plan_forward(B, want_stats != 0, igemm_splitk_workspace(L.geometry(B)), GEMM_DEFAULT)
                              : op == 1 ? L.plan_dgrad(B, igemm_splitk_workspace(L.dgrad_geom(B)), GEMM_DEFAULT)
                                        : L.plan_wgrad(B, GEMM_DEFAULT);
        std::snprintf(name, name_cap, "%s", v.c_str());
    });
}

int cmoop_plan_convs(const int32_t gene[6], int32_t variant, int32_t T, int32_t F, int32_t* layers, int32_t cap, int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(gene && count && (variant >= 0 && variant <= 3) && T >= 1 && F >= 1 && cap >= 0 && (layers || cap == 0), "plan_convs: bad arguments");
        NetConfig cfg;
        cfg.variant = variant;
        int n = 0;
        for (const Op& op : plan_net(gene, cfg, T, F).ops) {
            if (op.kind != OP_CONV) continue;
            if (n < cap) {
                const int32_t row[7] = {op.H, op.W, op.Cin, op.Cout, op.KS, op.stride, op.feeds_bn};
                std::memcpy(layers + 7 * n, row, sizeof(row));
            }
            ++n;
        }
        *count = n;
    });
}

int cmoop_plan_dwconvs(const int32_t gene[6], int32_t variant, int32_t T, int32_t F, int32_t* layers, int32_t cap, int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(gene && count && (variant >= 0 && variant <= 3) && T >= 1 && F >= 1 && cap >= 0 && (layers || cap == 0), "plan_dwconvs: bad arguments");
        NetConfig cfg;
        cfg.variant = variant;
        int n = 0;
        for (const Op& op : plan_net(gene, cfg, T, F).ops) {
            if (op.kind != OP_DWCONV) continue;
            if (n < cap) {
                const int32_t row[4] = {op.H, op.W, op.Cin, op.KS};
                std::memcpy(layers + 4 * n, row, sizeof(row));
            }
            ++n;
        }
        *count = n;
    });
}

int cmoop_dwconv_wgrad_slices(int32_t B, int32_t H, int32_t W, int32_t C, int32_t KS, int32_t* out) {
    return guard([&] {
        CMOOP_REQUIRE(out, "dwconv_wgrad_slices: NULL output");
        *out = dwconv_wgrad_slices(B, H, W, C, KS);
    });
}

int cmoop_net_launch_plan(const int32_t gene[6], const cmoop_config* cfg, int32_t T, int32_t F, int32_t B, int32_t train, char* buf,
                          int32_t cap) {
    return guard([&] {
        CMOOP_REQUIRE(gene && buf && cap > 0 && T >= 1 && F >= 1, "net_launch_plan: bad arguments");
        const NetConfig c = to_cfg(cfg);
        const std::string v = plan_net(gene, c, T, F).launch_plan(c.batch, std::max(c.batch, c.eval_batch), B, train != 0);
        CMOOP_REQUIRE((int)v.size() < cap, "net_launch_plan: buffer too small");
        std::memcpy(buf, v.c_str(), v.size() + 1);
    });
}

int cmoop_halo_tile_check(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t* rows_bound,
                          int32_t* rows_needed, int32_t* rows_stageable) {
    return guard([&] {
        CMOOP_REQUIRE(rows_bound && rows_needed && rows_stageable && B >= 1 && H >= 1 && W >= 1 && Cin >= 16 && Cout >= 1 && KS >= 1, "bad conv shape");
        int b = 0, n = 0, c = 0;
        halo_rows_bound_and_need(conv_geometry(B, H, W, Cin, Cout, KS, 1), &b, &n, &c);
        *rows_bound = b; *rows_needed = n; *rows_stageable = c;
    });
}

int cmoop_wgrad_slices(int32_t B, int32_t H, int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t* out) {
    return guard([&] {
        CMOOP_REQUIRE(out && B >= 1 && H >= 1 && W >= 1 && Cin >= 1 && Cout >= 1 && KS >= 1 && stride >= 1, "bad conv shape");
        *out = wgrad_slices(conv_geometry(B, H, W, Cin, Cout, KS, stride));
    });
}

int cmoop_calculate_fpr(const int32_t* y_true, const int32_t* y_pred, int64_t n, int32_t classes, int32_t fpr_variant,
                        double* out) {
    return guard([&] {
        CMOOP_REQUIRE(classes >= 1 && classes <= 4096, "bad class count");
        std::vector<int64_t> cm((size_t)classes * classes, 0);
        for (int64_t i = 0; i < n; ++i) {
            const int a = fpr_variant == CMOOP_FPR_V1_QUIRK ? 0 : y_true[i];
            const int b = y_pred[i];
            if (a >= 0 && a < classes && b >= 0 && b < classes) cm[(size_t)a * classes + b] += 1;
        }
        *out = fpr_from_confusion(cm.data(), classes, fpr_variant == CMOOP_FPR_V3 ? 2 : 0);
    });
}

// ---- front end ---------------------------------------------------------------
int cmoop_logmel(const float* wav_dev, int64_t n_clips, int32_t n_samples, float* out_dev) {
    return guard([&] {
        const FrontendTables* tables = frontend_tables_for_current_device();
        CMOOP_REQUIRE(n_samples >= 160, "clip shorter than one hop");
        hipStream_t s = lib_stream();
        launch_logmel(wav_dev, n_clips, n_samples, out_dev, tables, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_frontend_config_default(cmoop_frontend_config* c) {
    return guard([&] {
        CMOOP_REQUIRE(c != nullptr, "front end config is NULL");
        const FrontendCfg f;
        c->sr = f.sr; c->n_fft = f.n_fft; c->win = f.win; c->hop = f.hop; c->n_mels = f.n_mels; c->scale = f.scale;
        c->db_ref_max = f.db_ref_max; c->fmin = f.fmin; c->fmax = f.fmax; c->log_eps = f.log_eps; c->db_amin = f.db_amin;
        c->top_db = f.top_db;
    });
}

int cmoop_frontend_check(const cmoop_frontend_config* c) {
    return guard([&] { to_frontend_cfg(c); });
}

int cmoop_frontend_frames(const cmoop_frontend_config* c, int32_t n_samples, int32_t* T) {
    return guard([&] {
        CMOOP_REQUIRE(T != nullptr, "frontend_frames: NULL output");
        *T = frontend_frames(to_frontend_cfg(c), n_samples);
    });
}

int cmoop_frontend_mel_basis(const cmoop_frontend_config* c, float* out_host) {
    return guard([&] {
        CMOOP_REQUIRE(out_host != nullptr, "frontend_mel_basis: NULL output");
        const FrontendCfg f = to_frontend_cfg(c);
        const FrontendHostTables h = frontend_host_tables(f);
        const int nb = f.n_fft / 2 + 1;
        std::memset(out_host, 0, (size_t)f.n_mels * nb * sizeof(float));
        for (int i = 0; i < f.n_mels; ++i)
            for (int k = 0; k < h.count[i]; ++k) out_host[(size_t)i * nb + h.first_bin[i] + k] = h.melw[h.start[i] + k];
    });
}

// The front end's entry points and their timed twins share a body each, as quantize_weights_abi: the entry point makes its own
// argument checks (no device needed), the body then takes the tables and the stream; avg_ms null: one launch, else timed launches
static void logmel_ex_abi(const FrontendCfg& f, const float* wav, int64_t n_clips, int32_t n_samples, float* out, int32_t iters,
                          double* avg_ms) {
    const std::shared_ptr<const FrontendTables> tables = frontend_tables_for(f);
    hipStream_t s = lib_stream();
    auto once = [&] { launch_logmel(wav, n_clips, n_samples, out, tables.get(), s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_logmel_ex(const cmoop_frontend_config* c, const float* wav_dev, int64_t n_clips, int32_t n_samples, float* out_dev) {
    return guard([&] {
        const FrontendCfg f = to_frontend_cfg(c);
        CMOOP_REQUIRE(n_samples >= 1 && n_clips >= 0, "logmel_ex: n_samples >= 1, n_clips >= 0");
        logmel_ex_abi(f, wav_dev, n_clips, n_samples, out_dev, 0, nullptr);
    });
}

int cmoop_logmel_ex_time(const cmoop_frontend_config* c, const float* wav_dev, int64_t n_clips, int32_t n_samples, float* out_dev,
                         int32_t iters, double* avg_ms) {
    return guard([&] {
        const FrontendCfg f = to_frontend_cfg(c);
        CMOOP_REQUIRE(n_samples >= 1 && n_clips >= 1 && iters >= 1 && avg_ms, "logmel_ex_time: n_samples, n_clips, iters >= 1");
        logmel_ex_abi(f, wav_dev, n_clips, n_samples, out_dev, iters, avg_ms);
    });
}

static int compute_units_of_current_device() {
    int dev = 0, cu = 0;
    CMOOP_HIP(hipGetDevice(&dev));
    CMOOP_HIP(hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, dev));
    return cu > 0 ? cu : 256;
}

static void logmel_stream_abi(const FrontendCfg& f, const float* wav, int64_t n_samples, float* out, int32_t iters, double* avg_ms) {
    const std::shared_ptr<const FrontendTables> tables = frontend_tables_for(f);
    const int cu = compute_units_of_current_device();
    hipStream_t s = lib_stream();
    auto once = [&] { launch_logmel_stream(wav, n_samples, out, tables.get(), cu, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_logmel_stream(const cmoop_frontend_config* c, const float* wav_dev, int64_t n_samples, float* out_dev) {
    return guard([&] { logmel_stream_abi(to_frontend_cfg(c), wav_dev, n_samples, out_dev, 0, nullptr); });
}

int cmoop_logmel_stream_time(const cmoop_frontend_config* c, const float* wav_dev, int64_t n_samples, float* out_dev, int32_t iters,
                             double* avg_ms) {
    return guard([&] {
        const FrontendCfg f = to_frontend_cfg(c);
        CMOOP_REQUIRE(iters >= 1 && avg_ms, "logmel_stream_time: iters >= 1");
        logmel_stream_abi(f, wav_dev, n_samples, out_dev, iters, avg_ms);
    });
}

// ---- PCEN ----------------------------------------------------------------------
int cmoop_pcen_default(cmoop_pcen* p) {
    return guard([&] {
        CMOOP_REQUIRE(p != nullptr, "pcen config is NULL");
        const PcenCfg c;
        p->s = c.s; p->alpha = c.alpha; p->delta = c.delta; p->r = c.r; p->eps = c.eps; p->input_scale = c.input_scale;
    });
}

int cmoop_pcen_check(const cmoop_pcen* p) {
    return guard([&] { to_pcen(p); });
}

int cmoop_pcen_smoothing(double time_constant_s, int32_t sr, int32_t hop, double* s) {
    return guard([&] {
        CMOOP_REQUIRE(s != nullptr, "pcen_smoothing: NULL output");
        *s = pcen_smoothing(time_constant_s, sr, hop);
    });
}

int cmoop_pcen_stream_plan(int64_t n_frames, int32_t* chunk, int32_t* n_chunks) {
    return guard([&] {
        int ch = 0, nc = 0;
        pcen_stream_plan(n_frames, &ch, &nc);
        if (chunk) *chunk = ch;
        if (n_chunks) *n_chunks = nc;
    });
}

int cmoop_pcen_apply(const cmoop_pcen* p, float* e_dev, int64_t n, int32_t T, int32_t F) {
    return guard([&] {
        const PcenParams pp = to_pcen(p);
        hipStream_t s = lib_stream();
        launch_pcen_apply(pp, e_dev, n, T, F, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_logmel_pcen(const cmoop_frontend_config* c, const cmoop_pcen* p, const float* wav_dev, int64_t n_clips, int32_t n_samples,
                      float* out_dev) {
    return guard([&] {
        const FrontendCfg f = to_pcen_frontend_cfg(c, "logmel_pcen");
        const PcenParams pp = to_pcen(p);
        CMOOP_REQUIRE(n_samples >= 1 && n_clips >= 0, "logmel_pcen: n_samples >= 1, n_clips >= 0");
        const std::shared_ptr<const FrontendTables> tables = frontend_tables_for(f);
        hipStream_t s = lib_stream();
        launch_logmel_pcen(wav_dev, n_clips, n_samples, out_dev, tables.get(), pp, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_pcen_stream(const cmoop_pcen* p, float* e_dev, int64_t n_frames, int32_t F) {
    return guard([&] {
        const PcenParams pp = to_pcen(p);
        CMOOP_REQUIRE(F >= 1 && F <= FRONTEND_MAX_MELS, "pcen_stream: F must lie in 1..128 (got " + std::to_string(F) + ")");
        CMOOP_REQUIRE(n_frames >= 1 && n_frames * F <= 0x7fffffffll - 256, "pcen_stream: n_frames >= 1, n_frames * F must stay below 2^31");
        CMOOP_REQUIRE(e_dev != nullptr, "pcen_stream: NULL buffer");
        hipStream_t s = lib_stream();
        with_pcen_workspace((int)n_frames, F, s, [&](float* ws) { launch_pcen_stream(pp, e_dev, (int)n_frames, F, ws, s); });
    });
}

// (the n_samples check sits after lib_stream(), where both entry points always had it)
static void logmel_pcen_stream_abi(const FrontendCfg& f, const PcenParams& pp, const float* wav, int64_t n_samples, float* out,
                                   int32_t iters, double* avg_ms) {
    const std::shared_ptr<const FrontendTables> tables = frontend_tables_for(f);
    const int cu = compute_units_of_current_device();
    hipStream_t s = lib_stream();
    CMOOP_REQUIRE(n_samples >= 1 && n_samples <= 0x7fffffffll - 2 * f.n_fft, "stream front end: 1 <= n_samples < 2^31 - 2 n_fft");
    const int T = frontend_frames(f, (int)n_samples);
    with_pcen_workspace(T, f.n_mels, s, [&](float* ws) {
        auto once = [&] {
            launch_logmel_stream(wav, n_samples, out, tables.get(), cu, s);
            launch_pcen_stream(pp, out, T, f.n_mels, ws, s);
        };
        if (avg_ms) *avg_ms = time_launches(s, iters, once);
        else once();
    });
}

int cmoop_logmel_pcen_stream(const cmoop_frontend_config* c, const cmoop_pcen* p, const float* wav_dev, int64_t n_samples,
                             float* out_dev) {
    return guard([&] {
        const FrontendCfg f = to_pcen_frontend_cfg(c, "logmel_pcen_stream");
        const PcenParams pp = to_pcen(p);
        logmel_pcen_stream_abi(f, pp, wav_dev, n_samples, out_dev, 0, nullptr);
    });
}

int cmoop_logmel_pcen_stream_time(const cmoop_frontend_config* c, const cmoop_pcen* p, const float* wav_dev, int64_t n_samples,
                                  float* out_dev, int32_t iters, double* avg_ms) {
    return guard([&] {
        const FrontendCfg f = to_pcen_frontend_cfg(c, "logmel_pcen_stream_time");
        const PcenParams pp = to_pcen(p);
        CMOOP_REQUIRE(iters >= 1 && avg_ms, "logmel_pcen_stream_time: iters >= 1");
        logmel_pcen_stream_abi(f, pp, wav_dev, n_samples, out_dev, iters, avg_ms);
    });
}

int cmoop_stream_windows(int64_t n_frames, int32_t T, int32_t hop_frames, int64_t* n_windows) {
    return guard([&] {
        CMOOP_REQUIRE(n_windows != nullptr, "stream_windows: NULL output");
        *n_windows = stream_windows(n_frames, T, hop_frames);
    });
}

// ---- resampling ----------------------------------------------------------------
int cmoop_resample_filter(int32_t up, int32_t down, int32_t half_width, double beta, float* taps_host, int32_t cap, int32_t* n_taps) {
    return guard([&] {
        const int n = resample_filter_taps(up, down, half_width);
        if (n_taps) *n_taps = n;
        if (!taps_host) return;                                       // the size query
        if (cap < n) throw std::runtime_error("resample: cap must hold n_taps = " + std::to_string(n) + " values (got " + std::to_string(cap) + ")");
        resample_filter(up, down, half_width, beta, taps_host);
    });
}

int cmoop_resample_plan(int64_t n_samples, int32_t up, int32_t down, int32_t n_taps, int64_t* n_out, int32_t* tile, int64_t* n_tiles,
                        int32_t* taps_per_output) {
    return guard([&] {
        const ResamplePlan p = resample_plan(n_samples, up, down, n_taps);
        if (n_out) *n_out = p.n_out;
        if (tile) *tile = p.tile;
        if (n_tiles) *n_tiles = p.n_tiles;
        if (taps_per_output) *taps_per_output = p.tpp;
    });
}

int cmoop_resample_tile_span(int64_t n_samples, int32_t up, int32_t down, int32_t n_taps, int64_t tile_index, int64_t* out_first,
                             int32_t* out_count, int64_t* in_first, int32_t* in_count) {
    return guard([&] {
        const ResampleSpan s = resample_tile_span(resample_plan(n_samples, up, down, n_taps), tile_index);
        if (out_first) *out_first = s.out_first;
        if (out_count) *out_count = s.out_count;
        if (in_first) *in_first = s.in_first;
        if (in_count) *in_count = s.in_count;
    });
}

// the whole domain is checked before the stream is taken; avg_ms null: one launch, else timed launches (the table goes up once)
static void resample_abi(const float* wav, int64_t n_clips, int64_t n_samples, int32_t up, int32_t down, const float* taps, int32_t n_taps,
                         float* out, int32_t iters, double* avg_ms) {
    const ResamplePlan p = resample_plan(n_samples, up, down, n_taps);
    resample_check_rows(p, n_clips);
    if (!taps) throw std::runtime_error("resample: taps_host must not be NULL (got NULL)");
    if (n_clips > 0 && (!wav || !out || wav == out))
        throw std::runtime_error("resample: wav_dev and out_dev must be two device buffers (got NULL or the same pointer)");
    const std::vector<float> tab = resample_polyphase_table(p, taps);
    const int cu = compute_units_of_current_device();
    hipStream_t s = lib_stream();
    PoolScope pool(s);
    float* tab_dev = pool.get<float>(tab.size() * sizeof(float));
    CMOOP_HIP(hipMemcpyAsync(tab_dev, tab.data(), tab.size() * sizeof(float), hipMemcpyHostToDevice, s));
    auto once = [&] { launch_resample(wav, n_clips, p, tab_dev, out, cu, s); };
    if (avg_ms) *avg_ms = time_launches(s, iters, once);
    else once();
    CMOOP_HIP(hipStreamSynchronize(s));
}

int cmoop_resample(const float* wav_dev, int64_t n_clips, int64_t n_samples, int32_t up, int32_t down, const float* taps_host,
                   int32_t n_taps, float* out_dev) {
    return guard([&] { resample_abi(wav_dev, n_clips, n_samples, up, down, taps_host, n_taps, out_dev, 0, nullptr); });
}

int cmoop_resample_time(const float* wav_dev, int64_t n_clips, int64_t n_samples, int32_t up, int32_t down, const float* taps_host,
                        int32_t n_taps, float* out_dev, int32_t iters, double* avg_ms) {
    return guard([&] {
        if (iters < 1 || !avg_ms) throw std::runtime_error("resample: iters must be >= 1 with an avg_ms to write (got " + std::to_string(iters) + ")");
        resample_abi(wav_dev, n_clips, n_samples, up, down, taps_host, n_taps, out_dev, iters, avg_ms);
    });
}

int cmoop_mfcc(const float* logmel_dev, int64_t rows, int32_t n_mels, int32_t n_mfcc, float* out_dev) {
    return guard([&] {
        CMOOP_REQUIRE(rows >= 0 && (rows == 0 || (logmel_dev && out_dev && logmel_dev != out_dev)), "mfcc: out of place, rows >= 0");
        hipStream_t s = lib_stream();
        launch_mfcc(logmel_dev, out_dev, rows, n_mels, n_mfcc, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_standardize_fit(const float* x_dev, int64_t rows, int32_t cols, double* mean_host, double* scale_host) {
    return guard([&] {
        CMOOP_REQUIRE(rows >= 1 && cols >= 4 && cols % 4 == 0, "standardize: cols must be a multiple of 4");
        hipStream_t s = lib_stream();
        const int nb = colreduce_blocks(rows, cols);
        Scratch m(s);
        float* P = m.floats((size_t)nb * 2 * cols);
        double* ms = reinterpret_cast<double*>(m.floats((size_t)4 * cols));
        launch_colstats(x_dev, P, rows, cols, nb, s);
        colstats_finalize_f64(P, nb, rows, cols, ms, ms + cols, s);
        CMOOP_HIP(hipMemcpyAsync(mean_host, ms, cols * 8, hipMemcpyDeviceToHost, s));
        CMOOP_HIP(hipMemcpyAsync(scale_host, ms + cols, cols * 8, hipMemcpyDeviceToHost, s));
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_standardize_apply(float* x_dev, int64_t rows, int32_t cols, const double* mean_host, const double* scale_host) {
    return guard([&] {
        hipStream_t s = lib_stream();
        Scratch m(s);
        double* ms = reinterpret_cast<double*>(m.floats((size_t)4 * cols));
        CMOOP_HIP(hipMemcpyAsync(ms, mean_host, cols * 8, hipMemcpyHostToDevice, s));
        CMOOP_HIP(hipMemcpyAsync(ms + cols, scale_host, cols * 8, hipMemcpyHostToDevice, s));
        launch_standardize(x_dev, ms, ms + cols, rows, cols, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

// ---- profile -------------------------------------------------------------------
int cmoop_profile_reset(void) { return guard([] { profile_totals().reset(); }); }
int cmoop_profile_count(int32_t* out) {
    return guard([&] {
        ProfileTotals& t = profile_totals();
        std::lock_guard<std::mutex> l(t.mu);
        *out = (int32_t)t.by_kernel.size();
    });
}
int cmoop_profile_entry(int32_t i, char* name, int32_t name_cap, int64_t* launches, double* total_ms, double* total_flops) {
    return guard([&] {
        ProfileTotals& t = profile_totals();
        std::lock_guard<std::mutex> l(t.mu);
        CMOOP_REQUIRE(i >= 0 && i < (int)t.by_kernel.size() && name_cap > 0, "profile entry out of range");
        auto it = t.by_kernel.begin();
        std::advance(it, i);
        std::snprintf(name, name_cap, "%s", it->first.c_str());
        *launches = it->second.launches; *total_ms = it->second.ms; *total_flops = it->second.flops;
    });
}

int cmoop_profile_variant_count(int32_t* out) {
    return guard([&] {
        ProfileTotals& t = profile_totals();
        std::lock_guard<std::mutex> l(t.mu);
        *out = (int32_t)t.variants.size();
    });
}
int cmoop_profile_variant(int32_t i, char* name, int32_t name_cap) {
    return guard([&] {
        ProfileTotals& t = profile_totals();
        std::lock_guard<std::mutex> l(t.mu);
        CMOOP_REQUIRE(i >= 0 && i < (int)t.variants.size() && name_cap > 0, "profile variant out of range");
        auto it = t.variants.begin();
        std::advance(it, i);
        std::snprintf(name, name_cap, "%s", it->c_str());
    });
}

// ---- session -------------------------------------------------------------------
int cmoop_net_create(const int32_t gene[6], const cmoop_config* cfg, int32_t T, int32_t F, uint32_t seed, cmoop_net** out) {
    return guard([&] {
        NetConfig c = to_cfg(cfg);
        auto* h = new cmoop_net;
        h->net = nullptr;
        try {
            h->net = new Net(gene, c, T, F, seed, lib_stream());
        } catch (...) {
            delete h;
            throw;
        }
        *out = h;
    });
}
int cmoop_net_destroy(cmoop_net* h) {
    return guard([&] {
        if (!h) return;
        if (h->net) { hipStreamSynchronize(h->net->stream()); delete h->net; }
        delete h;
    });
}
int cmoop_net_total_params(cmoop_net* h, int64_t* out) { return guard([&] { *out = h->net->total_params(); }); }
int cmoop_net_get_params(cmoop_net* h, float* host) { return guard([&] { h->net->get_params(host); }); }
int cmoop_net_set_params(cmoop_net* h, const float* host) { return guard([&] { h->net->set_params(host); }); }
int cmoop_net_get_grads(cmoop_net* h, float* host) { return guard([&] { h->net->get_grads(host); }); }
int cmoop_net_train_step(cmoop_net* h, const float* x, const int32_t* y, const int32_t* idx, int64_t row0, int32_t B) {
    return guard([&] {
        h->net->train_step(x, y, idx, row0, B);
        CMOOP_HIP(hipStreamSynchronize(h->net->stream()));
        h->net->drain_profile();     // cfg.profile_every > 0: the sampled launches enter cmoop_profile_entry / _variant
    });
}
int cmoop_net_get_state(cmoop_net* h, float* params, float* adam_m, float* adam_v, int64_t* iterations, int64_t* steps) {
    return guard([&] {
        long long it = 0, st = 0;
        h->net->get_state(params, adam_m, adam_v, &it, &st);
        if (iterations) *iterations = it;
        if (steps) *steps = st;
    });
}
int cmoop_net_set_state(cmoop_net* h, const float* params, const float* adam_m, const float* adam_v, int64_t iterations,
                        int64_t steps) {
    return guard([&] { h->net->set_state(params, adam_m, adam_v, iterations, steps); });
}
int cmoop_net_set_augment(cmoop_net* h, const cmoop_augment* aug) { return net_set_option(h, "set_augment", aug, to_augment, &Net::set_augment); }
int cmoop_net_set_loss(cmoop_net* h, const cmoop_loss* loss) { return net_set_option(h, "set_loss", loss, to_loss, &Net::set_loss); }
int cmoop_net_train_step_targets(cmoop_net* h, const float* x_rows, const float* t, const float* w, const int32_t* primary, int32_t B) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "train_step_targets: NULL net");
        h->net->train_step_targets(x_rows, t, w, primary, B);
        CMOOP_HIP(hipStreamSynchronize(h->net->stream()));
        h->net->drain_profile();
    });
}
int cmoop_net_set_distill(cmoop_net* h, const cmoop_distill* distill) {
    return net_set_option(h, "set_distill", distill, to_distill, &Net::set_distill);
}
int cmoop_net_set_optim(cmoop_net* h, const cmoop_optim* optim) { return net_set_option(h, "set_optim", optim, to_optim, &Net::set_optim); }
int cmoop_net_optim_stats(cmoop_net* h, double out[4]) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net && out, "optim_stats: NULL argument");
        h->net->optim_stats(out);
    });
}
int cmoop_net_set_ema(cmoop_net* h, const cmoop_ema* ema) { return net_set_option(h, "set_ema", ema, to_ema, &Net::set_ema); }
int cmoop_net_get_ema(cmoop_net* h, float* host) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "get_ema: NULL net");
        h->net->get_average(host);
    });
}
int cmoop_net_set_ema_params(cmoop_net* h, const float* host) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "set_ema_params: NULL net");
        h->net->set_average(host);
    });
}
int cmoop_net_use_ema(cmoop_net* h, int32_t on) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "use_ema: NULL net");
        h->net->use_average(on != 0);
    });
}
int cmoop_net_finalize_ema(cmoop_net* h) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "finalize_ema: NULL net");
        h->net->finalize_average();
        CMOOP_HIP(hipStreamSynchronize(h->net->stream()));
    });
}
int cmoop_net_set_opoint(cmoop_net* h, const cmoop_opoint* op) { return net_set_option(h, "set_opoint", op, to_opoint, &Net::set_opoint); }
int cmoop_net_set_quant(cmoop_net* h, const cmoop_quant* q) { return net_set_option(h, "set_quant", q, to_quant, &Net::set_quant); }
int cmoop_net_set_prune(cmoop_net* h, const cmoop_prune* p) { return net_set_option(h, "set_prune", p, to_prune, &Net::set_prune); }
int cmoop_net_set_actquant(cmoop_net* h, const cmoop_actquant* aq) {
    return net_set_option(h, "set_actquant", aq, to_actquant, &Net::set_actquant);
}
int cmoop_net_get_act_ranges(cmoop_net* h, cmoop_act_range* host, int32_t cap, int32_t* count) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "get_act_ranges: NULL net");
        if (count) *count = h->net->act_sites();
        if (!host && count) return;   // the number of sites alone
        CMOOP_REQUIRE(host && cap >= h->net->act_sites(), "get_act_ranges: the buffer is too small");
        h->net->get_act_ranges(reinterpret_cast<ActRange*>(host));
    });
}
int cmoop_net_set_act_ranges(cmoop_net* h, const cmoop_act_range* host, int32_t count) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "set_act_ranges: NULL net");
        CMOOP_REQUIRE(host && count == h->net->act_sites(), "set_act_ranges: count must be the number of sites");
        h->net->set_act_ranges(reinterpret_cast<const ActRange*>(host));
    });
}
int cmoop_net_set_int8(cmoop_net* h, int32_t on) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "set_int8: NULL net");
        h->net->set_int8(on != 0);
    });
}
int cmoop_net_int8_ops(cmoop_net* h, int64_t* rows, int32_t cap, int32_t* count) { return int8_net_plan_abi(0, h, rows, cap, count); }
int cmoop_net_set_int8_depthwise(cmoop_net* h, int32_t on) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "set_int8_depthwise: NULL net");
        h->net->set_int8_depthwise(on != 0);
    });
}
int cmoop_net_int8_dw_ops(cmoop_net* h, int64_t* rows, int32_t cap, int32_t* count) { return int8_net_plan_abi(1, h, rows, cap, count); }
int cmoop_net_set_int8_fused(cmoop_net* h, int32_t on) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "set_int8_fused: NULL net");
        h->net->set_int8_fused(on != 0);
    });
}
int cmoop_net_int8_fused_ops(cmoop_net* h, int64_t* rows, int32_t cap, int32_t* count) { return int8_net_plan_abi(2, h, rows, cap, count); }
int cmoop_net_get_act(cmoop_net* h, int32_t i, int32_t B, int32_t dims[6], float* data_host, float* grad_host) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "get_act: NULL net");
        h->net->get_act(i, B, dims, data_host, grad_host);
    });
}
int cmoop_net_get_pruned(cmoop_net* h, float* weff_params_host, uint32_t* zeros_host) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "get_pruned: NULL net");
        h->net->get_pruned(weff_params_host, zeros_host);
    });
}
int cmoop_net_get_quantized(cmoop_net* h, float* wq_params_host, int8_t* codes_host, float* scales_host) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "get_quantized: NULL net");
        h->net->get_quantized(wq_params_host, codes_host, scales_host);
    });
}
int cmoop_net_last_opoint(cmoop_net* h, cmoop_opoint_class* classes, double* summary) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "last_opoint: NULL net");
        h->net->last_opoint(classes ? as_classes(classes) : nullptr, summary);
    });
}
int cmoop_net_operating_point(cmoop_net* h, const float* x, const int32_t* y, int64_t n, const cmoop_opoint* op,
                              cmoop_opoint_class* classes, double* summary) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "operating_point: NULL net");
        const OpointCfg c = to_opoint(op);
        opoint_check(c);
        const int C = h->net->config().classes;
        opoint_check_shape(n, C);
        CMOOP_REQUIRE(classes && summary && (n == 0 || (x && y)), "operating_point: NULL buffer");
        PoolScope pool(h->net->stream());
        float* probs = pool.get<float>(std::max<size_t>((size_t)n * C, 1) * 4);
        h->net->predict(x, n, probs);
        operating_point(probs, y, n, C, c.recall, as_classes(classes), summary, h->net->stream());
    });
}
int cmoop_net_train_step_distill_targets(cmoop_net* h, const float* x_rows, const float* t, const float* w, const int32_t* primary,
                                         const float* q, double alpha, double temperature, int32_t B) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "train_step_distill_targets: NULL net");
        h->net->train_step_distill_targets(x_rows, t, w, primary, q, alpha, temperature, B);
        CMOOP_HIP(hipStreamSynchronize(h->net->stream()));
        h->net->drain_profile();
    });
}
int cmoop_net_loss_buffers(cmoop_net* h, int64_t out[4]) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net && out, "loss_buffers: NULL argument");
        h->net->loss_buffers(out);
    });
}
int cmoop_net_set_gather_rows(cmoop_net* h, int64_t n_rows) {
    return guard([&] {
        CMOOP_REQUIRE(n_rows >= 0, "negative row count");
        h->net->set_gather_rows(n_rows);
    });
}
int cmoop_net_run_epoch(cmoop_net* h, const float* x, const int32_t* y, int64_t n_train, int32_t epoch) {
    return guard([&] {
        CMOOP_REQUIRE(x && y && n_train >= 1, "run_epoch: NULL / empty training split");
        h->net->run_epoch(x, y, n_train, epoch);
        CMOOP_HIP(hipStreamSynchronize(h->net->stream()));
        h->net->drain_profile();
    });
}
int cmoop_step_launch_counts(int64_t out[4]) {
    return guard([&] {
        CMOOP_REQUIRE(out, "step_launch_counts: NULL output");
        step_launch_counts(out);
    });
}
int cmoop_net_fit(cmoop_net* h, const cmoop_dataset* ds, int32_t hist_cap, double* val_loss_hist, double* val_acc_hist,
                  int32_t* epochs_run, int32_t* best_epoch, double* acc, double* fpr, double* val_loss) {
    return guard([&] {
        CMOOP_REQUIRE(ds && ds->x_train && ds->y_train && ds->x_val && ds->y_val, "fit: dataset pointers are NULL");
        const Dataset d = to_dataset(ds);
        CMOOP_REQUIRE(d.T == h->net->feature_T() && d.F == h->net->feature_F(), "fit: dataset feature shape differs from the net's");
        FitHistory hist;
        const EvalResult r = fit_and_read_out(*h->net, h->net->config(), d, h->net->seed(), &hist);
        for (int i = 0; i < hist_cap && i < (int)hist.val_loss.size(); ++i) {
            if (val_loss_hist) val_loss_hist[i] = hist.val_loss[i];
            if (val_acc_hist) val_acc_hist[i] = hist.val_acc[i];
        }
        if (epochs_run) *epochs_run = r.epochs_run;
        if (best_epoch) *best_epoch = hist.best_epoch;
        if (acc) *acc = r.acc;
        if (fpr) *fpr = r.fpr;
        if (val_loss) *val_loss = r.val_loss;
    });
}
int cmoop_net_evaluate(cmoop_net* h, const float* x, const int32_t* y, int64_t n, double* loss_sum, int64_t* correct,
                       int32_t* preds_dev) {
    return guard([&] {
        long long c = 0;
        h->net->evaluate(x, y, n, loss_sum, &c, preds_dev);
        *correct = c;
    });
}
int cmoop_net_predict(cmoop_net* h, const float* x, int64_t n, float* probs) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "predict: NULL net");
        h->net->predict(x, n, probs);
    });
}
int cmoop_net_predict_logits(cmoop_net* h, const float* x, int64_t n, float* logits) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "predict_logits: NULL net");
        h->net->predict_logits(x, n, logits);
    });
}
int cmoop_net_predict_stream(cmoop_net* h, const float* feat, int64_t n_frames, int32_t hop_frames, const cmoop_frontend_config* db,
                             const double* mean_host, const double* scale_host, float* probs) {
    return guard([&] {
        CMOOP_REQUIRE(h && h->net, "predict_stream: NULL net");
        FrontendCfg f;
        const bool db_scale = db != nullptr && db->scale == 1;
        if (db_scale) {
            f = to_frontend_cfg(db);
            CMOOP_REQUIRE(f.n_mels == h->net->feature_F(), "predict_stream: the front end config has " + std::to_string(f.n_mels) +
                          " mel bands, the net reads " + std::to_string(h->net->feature_F()) + " features per frame");
        }
        h->net->predict_stream(feat, n_frames, hop_frames, db_scale, f.db_ref_max != 0, f.db_amin, f.top_db, mean_host, scale_host, probs);
    });
}
int cmoop_net_train_metrics(cmoop_net* h, double* loss_sum, int64_t* correct, int32_t reset) {
    return guard([&] {
        long long c = 0;
        h->net->read_train_metrics(loss_sum, &c, reset != 0);
        *correct = c;
    });
}
int cmoop_epoch_permutation(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out_host) {
    return guard([&] { epoch_permutation(seed, epoch, n, out_host); });
}

int cmoop_epoch_permutation_device(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out_dev) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_epoch_permutation(seed, epoch, n, out_dev, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

// ---- kernel-level ---------------------------------------------------------------

int cmoop_conv_fwd(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t H, int32_t W, int32_t Cin,
                   int32_t Cout, int32_t KS, int32_t stride, int32_t relu) {
    return guard([&] {
        g_last_kernels.clear();
        hipStream_t s = lib_stream();
        Scratch m(s);
        if (Cin == 1) {
            CMOOP_REQUIRE(stride == 1 && bias, "first-layer conv: stride 1 with bias");
            launch_conv1_fwd(x, BatchRows(), w, bias, y, B, H, W, Cout, KS, relu, s);
        } else {
            GemmEpilogue e;
            e.bias = bias; e.relu = relu;
            const ConvGeom g = conv_geometry(B, H, W, Cin, Cout, KS, stride);
            const size_t skf = igemm_splitk_workspace(g);
            int flags = 0;
            const int code = launch_igemm_fwd(x, w, y, g, e, s, nullptr, m.floats(skf), skf, nullptr, nullptr, 0, &flags);
            g_last_kernels = gemm_variant_name(0, code, flags);
        }
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_conv_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int32_t B, int32_t H,
                   int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t mask_relu) {
    return guard([&] {
        hipStream_t s = lib_stream();
        Scratch m(s);
        if (Cin == 1) {
            const int nb = conv1_wgrad_blocks(B, H, W);
            const int64_t per = (int64_t)Cout * (KS * KS + 1);
            float *P = m.floats((size_t)nb * per), *tmp = m.floats((size_t)per);
            launch_conv1_wgrad(x, BatchRows(), dy, P, B, H, W, Cout, KS, s);
            launch_reduce_slices(P, tmp, nb, per, s);
            CMOOP_HIP(hipMemcpyAsync(dw, tmp, (size_t)Cout * KS * KS * 4, hipMemcpyDeviceToDevice, s));
            CMOOP_HIP(hipMemcpyAsync(db, tmp + (size_t)Cout * KS * KS, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s));
            CMOOP_HIP(hipStreamSynchronize(s));
            return;
        }
        // the launchers with defaults: this batch's slabs, separate dw / db reduction, no dgrad row table, dgrad split-K
        // slabs for stride-1 layers only
        const ConvLayer L{H, W, Cin, Cout, KS, stride};
        ConvBuffers buf;
        buf.slab_floats = L.slab_floats_at(B);
        buf.slabs = m.floats(buf.slab_floats);
        buf.wd = m.floats(L.flip_floats());
        buf.tab_rows = L.table_rows(B);
        buf.tab = m.rowtab(L.geometry(B), buf.tab_rows);
        g_last_kernels.clear();
        RecordingHook hook(&g_last_kernels);
        L.wgrad(x, dy, dw, db, B, buf, GEMM_DEFAULT, s, &hook);
        if (dx) {
            int accumulate = 0;
            if (stride != 1) {
                CMOOP_HIP(hipMemsetAsync(dx, 0, (size_t)B * H * W * Cin * 4, s));
                accumulate = 1;
            }
            buf.splitk_floats = (stride == 1 && L.mfma_dgrad()) ? igemm_splitk_workspace(L.dgrad_geom(B)) : 0;
            buf.splitk = m.floats(buf.splitk_floats);
            L.dgrad(dy, w, dx, B, mask_relu ? x : nullptr, 1.f, accumulate, false, buf, GEMM_DEFAULT, s, &hook);
        }
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

// ---- depthwise half of a separable layer, launched as Net::forward / Net::backward launch it ------------------------------
int cmoop_dwconv_fwd(const float* x, const float* w, float* y, int32_t B, int32_t H, int32_t W, int32_t C, int32_t KS) {
    return guard([&] {
        CMOOP_REQUIRE(x && w && y, "dwconv_fwd: NULL buffer");
        hipStream_t s = lib_stream();
        launch_dwconv_fwd(x, w, y, B, H, W, C, KS, 0, nullptr, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_dwconv_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, int32_t B, int32_t H, int32_t W,
                     int32_t C, int32_t KS, int32_t mask_relu) {
    return guard([&] {
        CMOOP_REQUIRE(x && w && dy && dw, "dwconv_bwd: NULL buffer");
        hipStream_t s = lib_stream();
        Scratch m(s);
        // the trainer's order: weight-gradient slabs, data gradient, then the fixed-order slice sum (the optimiser launch's order)
        const int S = dwconv_wgrad_slices(B, H, W, C, KS);
        const int64_t per = (int64_t)KS * KS * C;
        float* P = m.floats((size_t)S * per);
        launch_dwconv_wgrad(x, dy, P, B, H, W, C, KS, s);
        if (dx) launch_dwconv_fwd(dy, w, dx, B, H, W, C, KS, 1, mask_relu ? x : nullptr, s);
        launch_reduce_slices(P, dw, S, per, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_dwconv_time(int32_t mode, const float* x, const float* w, const float* dy, float* out, int32_t B, int32_t H, int32_t W,
                      int32_t C, int32_t KS, int32_t iters, double* avg_ms) {
    // mode 0: forward (out = y); 1: data gradient with the x > 0 mask (out = dx); 2: weight-gradient kernel alone (partials
    // into a scratch buffer; out unused)
    return guard([&] {
        CMOOP_REQUIRE(avg_ms && mode >= 0 && mode <= 2 && iters >= 1, "dwconv_time: bad arguments");
        hipStream_t s = lib_stream();
        Scratch m(s);
        float* P = mode == 2 ? m.floats((size_t)dwconv_wgrad_slices(B, H, W, C, KS) * KS * KS * C) : nullptr;
        *avg_ms = time_launches(s, iters, [&] {
            if (mode == 0) launch_dwconv_fwd(x, w, out, B, H, W, C, KS, 0, nullptr, s);
            else if (mode == 1) launch_dwconv_fwd(dy, w, out, B, H, W, C, KS, 1, x, s);
            else launch_dwconv_wgrad(x, dy, P, B, H, W, C, KS, s);
        });
    });
}

// ---- the same two operations launched as the trainer launches them: ConvLayer's launches, with a lone layer's buffers
//      (tables and split-K workspace of the batch at hand; Net's are shared and planned for its batch / eval_batch) ------
int cmoop_conv_fwd_trainer(const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t H, int32_t W,
                           int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t relu, double* col_sum,
                           double* col_sumsq, int32_t* stats_fused) {
    return guard([&] {
        g_last_kernels.clear();
        hipStream_t s = lib_stream();
        Scratch m(s);
        const ConvLayer L{H, W, Cin, Cout, KS, stride};
        GemmEpilogue e;
        e.bias = bias; e.relu = relu;
        const bool want_stats = col_sum != nullptr && col_sumsq != nullptr;
        CMOOP_REQUIRE(!want_stats || Cout % 4 == 0, "statistics need Cout % 4 == 0");
        ConvBuffers buf;
        buf.splitk_floats = igemm_splitk_workspace(L.geometry(B));
        buf.splitk = m.floats(buf.splitk_floats);
        buf.tab_rows = L.table_rows(B);
        buf.tab = m.rowtab(L.geometry(B), buf.tab_rows);
        if (want_stats) buf.stats = m.floats(L.stats_floats(B));
        RecordingHook hook(&g_last_kernels);
        bool fused = false;
        const int nb = L.forward(x, w, y, B, e, want_stats, buf, s, &hook, &fused);
        if (want_stats) {
            if (stats_fused) *stats_fused = fused ? 1 : 0;
            std::vector<float> hp((size_t)nb * 2 * Cout);
            CMOOP_HIP(hipMemcpyAsync(hp.data(), buf.stats, hp.size() * 4, hipMemcpyDeviceToHost, s));
            CMOOP_HIP(hipStreamSynchronize(s));
            for (int c = 0; c < Cout; ++c) { col_sum[c] = 0.0; col_sumsq[c] = 0.0; }
            for (int b = 0; b < nb; ++b)
                for (int c = 0; c < Cout; ++c) {
                    col_sum[c] += (double)hp[((size_t)b * 2) * Cout + c];
                    col_sumsq[c] += (double)hp[((size_t)b * 2 + 1) * Cout + c];
                }
        }
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_conv_bwd_trainer(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int32_t B, int32_t H,
                           int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t stride, int32_t mask_relu) {
    return guard([&] {
        g_last_kernels.clear();
        hipStream_t s = lib_stream();
        Scratch m(s);
        const ConvLayer L{H, W, Cin, Cout, KS, stride};
        RecordingHook hook(&g_last_kernels);
        const size_t NK = L.flip_floats();
        ConvBuffers buf;
        buf.slab_floats = L.slab_floats_at(B);       // (the trainer: the worst batch's)
        buf.slabs = m.floats(buf.slab_floats);
        float* dwb = m.floats(NK + Cout);            // the trainer's arena layout: bias gradient directly after the kernel gradient
        buf.tab_rows = L.table_rows(B);
        buf.tab = m.rowtab(L.geometry(B), buf.tab_rows);
        L.wgrad(x, dy, dwb, dwb + NK, B, buf, GEMM_DEFAULT, s, &hook);
        CMOOP_HIP(hipMemcpyAsync(dw, dwb, NK * 4, hipMemcpyDeviceToDevice, s));
        CMOOP_HIP(hipMemcpyAsync(db, dwb + NK, (size_t)Cout * 4, hipMemcpyDeviceToDevice, s));
        if (dx) {
            int accumulate = 0;
            if (stride != 1) {
                CMOOP_HIP(hipMemsetAsync(dx, 0, (size_t)B * H * W * Cin * 4, s));
                accumulate = 1;
            }
            if (L.mfma_dgrad()) {
                buf.wd = m.floats(NK);
                launch_flip_transpose(w, buf.wd, Cout, KS, KS, Cin, s);       // the trainer's one-launch-per-step refresh, for one layer
                buf.tab_d_rows = L.dgrad_table_rows(B);
                buf.tab_d = m.rowtab(L.dgrad_geom(B), buf.tab_d_rows);
                buf.splitk_floats = igemm_splitk_workspace(L.dgrad_geom(B));      // the trainer passes its workspace to every dgrad, the skip projection's too
                buf.splitk = m.floats(buf.splitk_floats);
            }
            L.dgrad(dy, w, dx, B, mask_relu ? x : nullptr, 1.f, accumulate, L.mfma_dgrad(), buf, GEMM_DEFAULT, s, &hook);
        }
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}

int cmoop_last_kernels(char* buf, int32_t cap) {
    return guard([&] {
        CMOOP_REQUIRE(buf && cap > 0, "last_kernels: no buffer");
        std::snprintf(buf, cap, "%s", g_last_kernels.c_str());
    });
}

int cmoop_conv_time(int32_t mode, const float* x, const float* w, const float* bias, float* y, int32_t B, int32_t H,
                    int32_t W, int32_t Cin, int32_t Cout, int32_t KS, int32_t iters, double* avg_ms) {
    // mode 0: forward implicit GEMM; 1: dgrad implicit GEMM (y = dY [B,H,W,Cout] in, x = dX out);
    // mode 2: wgrad MFMA kernel only (y = dY in, partials into a scratch buffer)
    return guard([&] {
        hipStream_t s = lib_stream();
        Scratch m(s);
        const ConvLayer L{H, W, Cin, Cout, KS, 1};
        const ConvGeom g = L.geometry(B), gd = L.dgrad_geom(B);
        float *wd = nullptr, *wg = nullptr;
        GemmEpilogue e;
        const int S = wgrad_slices(g);
        if (mode == 0) e.bias = bias;
        if (mode == 1) {
            wd = m.floats(L.flip_floats());
            launch_flip_transpose(w, wd, Cout, KS, KS, Cin, s);
        }
        if (mode == 2) wg = m.floats((size_t)S * g.Cout * g.K());      // kernel partials only: no bias slabs
        // the layer's row table, as the trainer passes it (forward / wgrad: forward geometry; dgrad: its own)
        const int tab_rows = (L.has_tables() && Cin >= 16) ? rowtab_rows(mode == 1 ? gd : g) : 0;
        void* tab = m.rowtab(mode == 1 ? gd : g, tab_rows);
        const size_t skf = mode == 0 ? igemm_splitk_workspace(g) : (mode == 1 ? igemm_splitk_workspace(gd) : 0);
        float* sk = m.floats(skf);
        *avg_ms = time_launches(s, iters, [&] {
            if (mode == 0) launch_igemm_fwd(x, w, y, g, e, s, nullptr, sk, skf, nullptr, tab, tab_rows);
            else if (mode == 1) launch_igemm_fwd(y, wd, const_cast<float*>(x), gd, e, s, nullptr, sk, skf, nullptr, tab, tab_rows);
            else launch_igemm_wgrad(x, y, wg, g, S, s, nullptr, nullptr, 0, GEMM_DEFAULT, tab, tab_rows);
        });
    });
}

int cmoop_dense_fwd(const float* x, const float* w, const float* bias, float* y, int32_t M, int32_t N, int32_t K, int32_t relu) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_dense_fwd(x, w, bias, y, M, N, K, relu, 0, 0u, 0u, 1.f, GEMM_DEFAULT, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_dense_bwd(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int32_t M, int32_t N, int32_t K,
                    int32_t mask_relu) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_dense_wgrad(x, dy, dw, db, M, N, K, GEMM_DEFAULT, s);
        if (dx) launch_dense_dgrad(dy, w, dx, M, N, K, mask_relu ? x : nullptr, 1.f, GEMM_DEFAULT, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
// CMOOP_GEMM_* of a kernel-level dense call -> the GemmMode a Net would hold for it
static int dense_ex_mode(int32_t gemm_mode) {
    CMOOP_REQUIRE(gemm_mode == CMOOP_GEMM_DEFAULT || gemm_mode == CMOOP_GEMM_FP32 || gemm_mode == CMOOP_GEMM_BF16X3 ||
                      gemm_mode == CMOOP_GEMM_BF16, "bad gemm_mode");
    if (gemm_mode == CMOOP_GEMM_DEFAULT) return gemm_mode_default();
    return gemm_mode == CMOOP_GEMM_FP32 ? (int)GEMM_FP32 : (int)gemm_mode;
}
int cmoop_dense_fwd_ex(const float* x, const float* w, const float* bias, float* y, int32_t M, int32_t N, int32_t K, int32_t relu,
                       int32_t gemm_mode, double dropout_rate, uint32_t seed, int32_t dropout_layer, uint32_t step,
                       const void* step_state_dev) {
    return guard([&] {
        const int mode = dense_ex_mode(gemm_mode);
        const DropoutParams dp = dropout_params(dropout_rate);
        const bool drop = dropout_rate > 0.0;
        CMOOP_REQUIRE(!drop || dropout_layer >= 0, "dense_fwd_ex: dropout_layer >= 0");
        static_assert(sizeof(StepState) == 16, "cmoop_dense_fwd_ex documents a 16-byte step state");
        const StepState* st = drop ? static_cast<const StepState*>(step_state_dev) : nullptr;
        const uint32_t drop_stream = drop ? DropoutParams::stream(dropout_layer) : 0u;
        hipStream_t s = lib_stream();
        // the argument list of Net::forward's OP_DENSE launch (the host prefix is passed in both forms, as there)
        launch_dense_fwd(x, w, bias, y, M, N, K, relu, drop ? 1 : 0, drop ? rng_prefix(seed, drop_stream, step) : 0u, dp.thr,
                         dp.keep_scale, mode, s, st, seed, drop_stream);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_dense_bwd_ex(const float* x, const float* w, const float* dy, float* dx, float* dw, float* db, int32_t M, int32_t N,
                       int32_t K, int32_t mask_relu, double mask_scale, int32_t gemm_mode, int32_t merged) {
    return guard([&] {
        const int mode = dense_ex_mode(gemm_mode);
        CMOOP_REQUIRE(dx != nullptr, "dense_bwd_ex: dx is NULL");
        hipStream_t s = lib_stream();
        const float* mask = mask_relu ? x : nullptr;
        if (merged) {
            launch_dense_bwd(x, dy, w, dw, db, dx, M, N, K, mask, (float)mask_scale, mode, s);
        } else {
            launch_dense_wgrad(x, dy, dw, db, M, N, K, mode, s);
            launch_dense_dgrad(dy, w, dx, M, N, K, mask, (float)mask_scale, mode, s);
        }
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_maxpool_fwd(const float* x, float* y, uint8_t* arg, int32_t B, int32_t H, int32_t W, int32_t C) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_maxpool_fwd(x, y, arg, B, H, W, C, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_maxpool_bwd(const float* dy, const uint8_t* arg, const float* y, float* dx, int32_t B, int32_t H, int32_t W,
                      int32_t C, int32_t mask_y_pos) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_maxpool_bwd(dy, arg, y, dx, B, H, W, C, mask_y_pos, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
// ---- kernel-level entry points of bn.hip, elem.hip, loss.hip and optim.hip (per-kernel parity tests): each launches what
//      Net::forward / Net::backward / Net::step_body launch for the operation, in their order and with their argument
//      casts; reduction workspaces live for the length of the call
static int reduce_blocks_arg(int32_t blocks, int64_t M, int32_t C) {
    CMOOP_REQUIRE(M >= 1 && C >= 4 && C % 4 == 0, "M >= 1 and C a multiple of 4 (>= 4)");
    CMOOP_REQUIRE(blocks >= 0 && blocks <= 4096, "blocks must be 0 (the trainer's count) or 1..4096");
    return blocks ? blocks : colreduce_blocks(M, C);
}

int cmoop_bn_train_fwd(const float* x, const float* gamma, const float* beta, float* moving_mean, float* moving_var, float* y,
                       float* mean, float* invstd, float* scale, float* shift, int64_t M, int32_t C, double eps, double momentum,
                       int32_t relu, int32_t blocks) {
    return guard([&] {
        const int nb = reduce_blocks_arg(blocks, M, C);
        hipStream_t s = lib_stream();
        Scratch ws(s);
        float* P = ws.floats((size_t)nb * 2 * C);
        launch_colstats(x, P, M, C, nb, s);
        launch_bn_finalize(P, nb, M, C, gamma, beta, moving_mean, moving_var, mean, invstd, scale, shift, (float)eps,
                           (float)momentum, (float)(1.0 - momentum), s);
        launch_scale_shift(x, y, scale, shift, M, C, relu, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_bn_eval_fwd(const float* x, const float* gamma, const float* beta, const float* moving_mean, const float* moving_var,
                      float* y, float* scale, float* shift, int64_t M, int32_t C, double eps, int32_t relu) {
    return guard([&] {
        CMOOP_REQUIRE(M >= 0 && C >= 4 && C % 4 == 0, "bn_eval_fwd: C must be a multiple of 4");
        hipStream_t s = lib_stream();
        launch_bn_eval_prepare(gamma, beta, moving_mean, moving_var, scale, shift, C, (float)eps, s);
        launch_scale_shift(x, y, scale, shift, M, C, relu, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_bn_bwd(const float* dy, const float* x, const float* mean, const float* invstd, const float* gamma, float* dx,
                 float* dgamma, float* dbeta, float* sums, int64_t M, int32_t C, int32_t mask_x_pos, int32_t blocks) {
    return guard([&] {
        const int nb = reduce_blocks_arg(blocks, M, C);
        hipStream_t s = lib_stream();
        Scratch ws(s);
        float* P = ws.floats((size_t)nb * 2 * C + 2 * C);       // the finalised sums sit right after the partials
        launch_bn_bwd_reduce(dy, x, mean, invstd, P, M, C, nb, s);
        launch_bn_bwd_apply(dy, x, mean, invstd, gamma, P, nb, dx, dgamma, dbeta, M, C, mask_x_pos, s);
        if (sums) CMOOP_HIP(hipMemcpyAsync(sums, P + (size_t)nb * 2 * C, (size_t)2 * C * 4, hipMemcpyDeviceToDevice, s));
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_bn_pool_fwd(const float* x, const float* scale, const float* shift, float* y, uint8_t* arg, int32_t B, int32_t H,
                      int32_t W, int32_t C, int32_t relu) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_bn_pool_fwd(x, y, arg, scale, shift, B, H, W, C, relu, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_bn_pool_bwd(const float* g_pooled, const uint8_t* arg, const float* x, const float* mean, const float* invstd,
                      const float* gamma, float* dx, float* dgamma, float* dbeta, float* sums, int32_t B, int32_t H, int32_t W,
                      int32_t C, int32_t mask_x_pos, int32_t blocks) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 1 && H >= 1 && W >= 1, "bn_pool_bwd: empty tensor");
        const int nb = reduce_blocks_arg(blocks, (int64_t)B * H * W, C);
        hipStream_t s = lib_stream();
        Scratch ws(s);
        float* P = ws.floats((size_t)nb * 2 * C + 2 * C);
        launch_bn_pool_bwd_reduce(g_pooled, arg, x, mean, invstd, P, B, H, W, C, nb, s);
        launch_bn_pool_bwd_apply(g_pooled, arg, x, mean, invstd, gamma, P, nb, dx, dgamma, dbeta, B, H, W, C, mask_x_pos, s);
        if (sums) CMOOP_HIP(hipMemcpyAsync(sums, P + (size_t)nb * 2 * C, (size_t)2 * C * 4, hipMemcpyDeviceToDevice, s));
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_add_relu(const float* a, const float* b, float* y, int64_t n) {
    return guard([&] {
        hipStream_t s = lib_stream();
        launch_add_relu(a, b, y, n, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_gap_fwd(const float* x, float* y, int32_t B, int32_t HW, int32_t C) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && HW >= 1 && C >= 4, "gap_fwd: HW >= 1, C >= 4");
        hipStream_t s = lib_stream();
        launch_gap_fwd(x, y, B, HW, C, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_gap_bwd(const float* dy, const float* x, float* dx, int32_t B, int32_t HW, int32_t C) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && HW >= 1 && C >= 4 && C % 4 == 0, "gap_bwd: HW >= 1, C a multiple of 4");
        hipStream_t s = lib_stream();
        launch_gap_bwd(dy, x, dx, B, HW, C, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_softmax_ce(const float* z, const int32_t* labels, const int32_t* idx, int64_t row0, int64_t n_rows, int32_t B, int32_t C,
                     float* dz, double* acc, int32_t* preds) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && C >= 1 && row0 >= 0, "softmax_ce: B >= 0, C >= 1, row0 >= 0");
        hipStream_t s = lib_stream();
        launch_softmax_ce(z, labels, BatchRows{idx, row0, n_rows}, B, C, dz, acc, preds, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_softmax_probs(const float* z, float* p, int32_t B, int32_t C) {
    return guard([&] {
        CMOOP_REQUIRE(B >= 0 && C >= 1, "softmax_probs: B >= 0, C >= 1");
        hipStream_t s = lib_stream();
        launch_softmax_probs(z, p, B, C, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_adam(float* w, const float* g, float* m, float* v, int64_t n, double alpha, double beta1, double beta2, double eps) {
    return guard([&] {
        CMOOP_REQUIRE(n >= 0, "adam: n >= 0");
        hipStream_t s = lib_stream();
        launch_adam(w, g, m, v, n, (float)alpha, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
// the segment table of the host arrays cmoop_adam_segments / cmoop_grad_finish take
static AdamSegTable segment_table(const float* slab, int32_t count, const int64_t* off, const int64_t* n, const int32_t* S,
                                  const int64_t* stride, const int64_t* slab_off) {
    CMOOP_REQUIRE(count >= 0 && count <= ADAM_MAX_SEGS, "adam_segments: at most 64 segments");
    CMOOP_REQUIRE(count == 0 || (off && n && S && stride && slab_off), "adam_segments: NULL segment array");
    AdamSegTable tab;
    for (int i = 0; i < count; ++i) {
        AdamSeg sg;
        sg.off = off[i]; sg.n = n[i];
        CMOOP_REQUIRE(S[i] >= 0 && (S[i] == 0 || (slab && stride[i] >= n[i] && slab_off[i] >= 0)),
                      "adam_segments: a slab segment needs the slab buffer, stride >= n and slab_off >= 0");
        if (S[i] > 0) { sg.slab = slab + slab_off[i]; sg.stride = stride[i]; sg.S = S[i]; }
        tab.seg[tab.count++] = sg;
    }
    adam_segments_finalize(tab);
    return tab;
}
int cmoop_adam_segments(float* w, float* g, float* m, float* v, const float* slab, int32_t count, const int64_t* off,
                        const int64_t* n, const int32_t* S, const int64_t* stride, const int64_t* slab_off, double alpha,
                        double beta1, double beta2, double eps) {
    return guard([&] {
        const AdamSegTable tab = segment_table(slab, count, off, n, S, stride, slab_off);
        hipStream_t s = lib_stream();
        launch_adam_segments(w, g, m, v, tab, (float)alpha, (float)(1.0 - beta1), (float)(1.0 - beta2), (float)eps, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_grad_finish(float* g, const float* slab, int32_t count, const int64_t* off, const int64_t* n, const int32_t* S,
                      const int64_t* stride, const int64_t* slab_off, const uint8_t* kinds, double global_clipnorm, float* partials,
                      int32_t cap, int32_t* n_partials, void* record) {
    return guard([&] {
        CMOOP_REQUIRE(std::isfinite(global_clipnorm) && global_clipnorm >= 0, "grad_finish: global_clipnorm must be finite and >= 0");
        CMOOP_REQUIRE(partials && record, "grad_finish: NULL partial buffer or record");
        const AdamSegTable tab = segment_table(slab, count, off, n, S, stride, slab_off);
        CMOOP_REQUIRE(tab.blocks <= cap, "grad_finish: the partial buffer holds fewer than " + std::to_string(tab.blocks) + " floats");
        hipStream_t s = lib_stream();
        launch_grad_finish(g, tab, kinds, partials, s);
        launch_clip_scale(partials, tab.blocks, global_clipnorm, static_cast<OptimRecord*>(record), s);
        CMOOP_HIP(hipStreamSynchronize(s));
        if (n_partials) *n_partials = tab.blocks;
    });
}
int cmoop_adamw(float* w, const float* g, float* m, float* v, const uint8_t* kinds, int64_t n, const void* record, double alpha,
                double lr, double beta1, double beta2, double eps, double weight_decay, int32_t decay_mask, double clipvalue) {
    return guard([&] {
        CMOOP_REQUIRE(n >= 0 && record, "adamw: n >= 0 and a record");
        OptimCfg c;
        c.weight_decay = weight_decay; c.decay_mask = decay_mask; c.clipvalue = clipvalue;
        optim_check(c);
        AdamwArgs a;
        a.alpha = (float)alpha; a.lr = (float)lr; a.c1 = (float)(1.0 - beta1); a.c2 = (float)(1.0 - beta2); a.eps = (float)eps;
        a.weight_decay = (float)weight_decay; a.clipvalue = (float)clipvalue; a.decay_all = decay_mask;
        hipStream_t s = lib_stream();
        launch_adamw(w, g, m, v, kinds, n, static_cast<const OptimRecord*>(record), a, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_confusion(const int32_t* y_true, const int32_t* y_pred, int64_t n, int32_t C, int32_t force_true_zero, int64_t* cm) {
    return guard([&] {
        CMOOP_REQUIRE(n >= 0 && C >= 1 && cm, "confusion: n >= 0, C >= 1");
        hipStream_t s = lib_stream();
        launch_confusion(y_true, y_pred, n, C, force_true_zero, cm, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_colsum_small(const float* x, float* out, int32_t M, int32_t C) {
    return guard([&] {
        CMOOP_REQUIRE(M >= 0 && C >= 1, "colsum_small: M >= 0, C >= 1");
        hipStream_t s = lib_stream();
        launch_colsum_small(x, out, M, C, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_dense_dgrad_small(const float* dy, const float* w, float* dx, int32_t M, int32_t N, int32_t K, const float* mask,
                            double scale) {
    return guard([&] {
        CMOOP_REQUIRE(M >= 0 && N >= 0 && K >= 0, "dense_dgrad_small: negative size");
        hipStream_t s = lib_stream();
        launch_dense_dgrad_small(dy, w, dx, M, N, K, mask, (float)scale, s);
        CMOOP_HIP(hipStreamSynchronize(s));
    });
}
int cmoop_device_synchronize(void) { return guard([] { CMOOP_HIP(hipDeviceSynchronize()); }); }

}  // extern "C"
