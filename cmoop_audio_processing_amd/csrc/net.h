// One candidate CNN resident on the GPU: plan (from the six genes), parameter /
// Adam arenas, forward, backward, optimiser step, inference.  The MI355X-native
// replacement of build_model + model.fit/evaluate/predict
// (/root/reference/nsga_penalty.py:225-334,375-388; sa_nsga_penalty.py:137-177,211-221).
#pragma once
#include "kernels.h"
#include <atomic>
#include <functional>
#include <map>
#include <mutex>
#include <set>
#include <string>
#include <vector>

namespace cmoop {

struct NetConfig {
    int variant = 0, classes = 10, epochs = 300, batch = 64, patience = 5;
    int early_stop = 1, restore_best = 0, acc_readout = 0, fpr_variant = 0, shuffle = 1;
    int eval_batch = 256, n_slots = 8, profile_every = 0;
    int gemm_mode = GEMM_FP32;   // resolved GemmMode of the MFMA layers (never GEMM_DEFAULT here)
    double lr = 1e-3, beta1 = 0.9, beta2 = 0.999, adam_eps = 1e-7, bn_eps = 1e-3, bn_momentum = 0.99, dropout = 0.3;
};

// Inverted dropout of a Dense+ReLU layer as dense_fwd_kernel takes it: element (row, col) of fc layer `layer` is kept iff
// its 24-bit draw from stream(layer) is >= thr, kept values are multiplied by keep_scale (and so is the layer's input
// gradient).  THE place of these three values: Net::forward, plan_net's mask scales and the kernel-level entry point
// cmoop_dense_fwd_ex all take them from here.
struct DropoutParams {
    uint32_t thr;
    float keep_scale;
    static uint32_t stream(int layer) { return STREAM_DROPOUT + (uint32_t)layer; }
};
DropoutParams dropout_params(double rate);

struct Dataset {
    const float* x_train = nullptr; const int32_t* y_train = nullptr; int64_t n_train = 0;
    const float* x_val = nullptr;   const int32_t* y_val = nullptr;   int64_t n_val = 0;
    int T = 0, F = 0;
};

// topologies: 0 = A, 1 = B, 2 = A_ds, 3 = B_ds (A / B with every k x k stride-1 conv of C_in >= 16 made depthwise-separable)
inline bool variant_is_a(int variant) { return (variant & 1) == 0; }
inline bool variant_is_ds(int variant) { return variant >= 2; }
// host-side closed forms (bit-exact twins of genes.py)
int64_t param_count(const int32_t g[6], int variant, int classes);
double fwd_flops_per_sample(const int32_t g[6], int variant, int classes, int T, int F);
void validate_gene(const int32_t g[6]);

// HIP-event sampling of the MFMA GEMM kernels inside the timed region (bench.py roofline)
struct ProfileEntry { double ms = 0, flops = 0; long long launches = 0; };
struct ProfileTotals {   // keyed by kernel instantiation name, e.g. "igemm_fwd_kernel<128,32>"
    std::mutex mu;
    std::map<std::string, ProfileEntry> by_kernel;
    // launch-path variants seen: name + "+sk" (split-K slabs + combine) / "+stats" (BatchNorm statistics epilogue) /
    // "+tab" (row-table operand loader) / "+bal" / "+slabs" (several row slices) -- what the parity-coverage test compares
    std::set<std::string> variants;
    void reset() { std::lock_guard<std::mutex> l(mu); by_kernel.clear(); variants.clear(); }
};
std::string gemm_variant_name(int cls, int code, int flags);
ProfileTotals& profile_totals();

struct GemmHook {   // brackets every MFMA GEMM launch (HIP-event sampling)
    virtual const GemmTiming* begin(int cls, double flops) = 0;   // null: do not time this launch
    virtual void end(int code, int flags) = 0;   // code: instantiation (gemm_kernel_name), flags: GemmFlags of the path taken
    virtual ~GemmHook() {}
};
// geometry of the implicit GEMM that computes dX from dY for forward geometry g (stride 1: flipped SAME padding;
// the strided 1x1 skip projection: a 1x1 GEMM over the output pixels, scattered by the epilogue)
ConvGeom dgrad_geometry(const ConvGeom& g);
// floats of BatchNorm statistics partials for an [M][C] tensor: the stand-alone reduction's blocks, or one partial per
// 64-row tile of the producing conv (fused statistics), plus the finalised pair
size_t stats_partials_floats(int64_t M, int C);

// Device memory the launches of one conv layer use.  The caller owns all of it: the trainer hands out slices of its
// arenas, the lone-layer entry points (api.hip) allocate per call.
struct ConvBuffers {
    const void* tab = nullptr;      // row table of geometry(B') for a B' >= the launch batch (forward and weight gradient)
    int tab_rows = 0;
    const void* tab_d = nullptr;    // row table of dgrad_geom(B') (data gradient)
    int tab_d_rows = 0;
    float* splitk = nullptr;        // split-K / balanced-partition slabs of the forward-type launches
    size_t splitk_floats = 0;
    float* slabs = nullptr;         // weight-gradient row-slice slabs
    size_t slab_floats = 0;
    float* wd = nullptr;            // flip-transposed weights (dgrad operand), flip_floats()
    float* stats = nullptr;         // BatchNorm statistics partials, stats_floats(B)
};

// One implicit-GEMM conv layer as the trainer launches it: THE place of every per-layer launch decision.  Net's plan,
// forward and backward, the lone-layer entry points of api.hip (cmoop_conv_*_trainer, cmoop_conv_time) and the host-only
// launch plans (cmoop_conv_launch_plan, cmoop_net_launch_plan) all go through it.  A host-side value: owns no memory.
struct ConvLayer {
    int H, W, Cin, Cout, KS, stride;

    ConvGeom geometry(int B) const { return conv_geometry(B, H, W, Cin, Cout, KS, stride); }
    ConvGeom dgrad_geom(int B) const { return dgrad_geometry(geometry(B)); }
    // row tables (geometry only: a table built for a batch serves every smaller one); the dgrad's when it is an MFMA launch
    bool has_tables() const { return KS * KS <= 32; }
    bool mfma_dgrad() const { return ilog2_exact(Cout) >= 4; }   // else: the classifier's tiny VALU kernel (dense layers only)
    int table_rows(int B) const { return has_tables() ? rowtab_rows(geometry(B)) : 0; }
    int dgrad_table_rows(int B) const { return has_tables() && mfma_dgrad() ? rowtab_rows(dgrad_geom(B)) : 0; }
    // workspace sizes in floats.  The weight gradient's slice count is NOT monotone in the batch rows (a smaller M can
    // flip the K-tile width and the co-resident workgroup count): slabs are sized for the worst train batch 1..b
    size_t slab_floats_at(int B) const;   // this batch's slices
    size_t slab_floats(int b) const;
    size_t stats_floats(int B) const { return stats_partials_floats(geometry(B).M(), Cout); }
    size_t flip_floats() const { return (size_t)Cout * KS * KS * Cin; }
    // split-K floats this layer asks of a net planned for train batch `batch` and Bmax = max(batch, eval_batch): forward
    // at both, dgrad (stride-1 layers) at the train batch.  NOT every partial batch: an under-filled one may want more,
    // and then takes another tile or partition than a lone launch of the same batch ("Launch plan")
    size_t splitk_need(int batch, int Bmax) const;

    // Y = conv(X, Wt) + epilogue e (bias / ReLU / mode; e.stats is set here).  want_stats: BatchNorm column partials into
    // buf.stats, by the conv's epilogue when the launch allows (*fused), else by the stand-alone reduction right after
    // it; returns the number of partials (0 without want_stats)
    int forward(const float* X, const float* Wt, float* Y, int B, GemmEpilogue e, bool want_stats, const ConvBuffers& buf,
                hipStream_t s, GemmHook* hook, bool* fused = nullptr) const;
    // dW [Cout][K] and dB [Cout] through buf.slabs; the slice count is clamped to the slab_floats that fit (never written
    // past).  defer != null (requires dB == dW + Cout*K): the slice sum is left to the optimiser launch -- *defer receives
    // the slab pointer / stride / slice count (slab stays null when one slice wrote dW, dB in place)
    void wgrad(const float* X, const float* dY, float* dW, float* dB, int B, const ConvBuffers& buf, int mode, hipStream_t s,
               GemmHook* hook, AdamSeg* defer = nullptr) const;
    // dX; wd_ready: buf.wd already holds the flip-transposed weights (the trainer refreshes all layers in one launch per step)
    void dgrad(const float* dY, const float* W, float* dX, int B, const float* mask, float mask_scale, int accumulate,
               bool wd_ready, const ConvBuffers& buf, int mode, hipStream_t s, GemmHook* hook) const;
    // host-only twins: the gemm_variant_name the launch above takes when handed splitk_floats of split-K workspace
    std::string plan_forward(int B, bool want_stats, size_t splitk_floats, int mode) const;
    std::string plan_wgrad(int B, int mode) const;
    std::string plan_dgrad(int B, size_t splitk_floats, int mode) const;
};

// cached device allocations (net.hip): get may return stale contents, free never blocks on other streams
void* pool_alloc(size_t bytes);
// CMOOP_POOL_FILL (net.hip): its byte, -1 when unset; and the fill of a device buffer about to be handed out (fill < 0: nothing)
int pool_fill_value();
void pool_fill_device(void* p, size_t bytes, int fill);
void pool_free(void* p);
void* pool_alloc_pinned(size_t bytes);
void pool_free_pinned(void* p);
// pooled buffers of one call: at scope exit, a throw included, the stream is drained first, then the buffers go back
struct PoolScope {
    hipStream_t s;
    std::vector<void*> bufs, pinned;
    explicit PoolScope(hipStream_t stream) : s(stream) {}
    PoolScope(const PoolScope&) = delete;
    ~PoolScope() { hipStreamSynchronize(s); for (void* p : pinned) pool_free_pinned(p); for (void* p : bufs) pool_free(p); }
    template <class T> T* get(size_t bytes) { bufs.push_back(pool_alloc(bytes)); return static_cast<T*>(bufs.back()); }
    template <class T> T* get_pinned(size_t bytes) { pinned.push_back(pool_alloc_pinned(bytes)); return static_cast<T*>(pinned.back()); }
};

struct Act {
    float* data = nullptr;
    float* grad = nullptr;
    int H = 0, W = 0, C = 0;
    bool own_grad = false;
    bool virt = false;         // never materialised (BatchNorm output consumed by a fused max-pool)
    int site = -1;             // activation-quantisation site number (plan_net), -1: not a site
    size_t per_sample() const { return (size_t)H * W * C; }
};

// OP_DWCONV: the depthwise half of a separable layer (topologies A_ds / B_ds); its pointwise half is an OP_CONV with KS = 1
enum OpKind { OP_CONV1, OP_CONV, OP_BN, OP_POOL, OP_ADDRELU, OP_GAP, OP_DENSE, OP_DWCONV };

struct Op {
    OpKind kind;
    int in = -1, in2 = -1, out = -1;
    // conv / dense
    int KS = 1, stride = 1, Cin = 0, Cout = 0;
    int H = 0, W = 0;          // spatial size of the input
    ConvLayer conv() const { return ConvLayer{H, W, Cin, Cout, KS, stride}; }   // OP_CONV: the layer's launch context
    int relu = 0, in_is_relu = 0, dgrad_accumulate = 0, dropout_layer = -1;
    float in_mask_scale = 1.f;
    int gemm_mode = GEMM_FP32;   // arithmetic of this layer's three GEMMs
    void* rowtab = nullptr;    // conv: row table of the layer (forward tile prologue and weight-gradient gather), max(batch, eval_batch) samples
    int rowtab_rows = 0;
    void* rowtab_d = nullptr;  // conv: row table of the layer's dgrad geometry (dY as input, flipped padding), train batch
    int rowtab_d_rows = 0;
    int64_t w_off = 0, b_off = 0, wd_off = -1;   // wd_off: this layer's slice of the flip-transposed copy (dgrad operand)
    int64_t slab_off = -1;     // conv / first conv / depthwise: this layer's weight-gradient slabs in the candidate's slab arena
    size_t slab_floats = 0;    // (kept until the optimiser launch sums them), sized for the worst train batch
    int tensor_index = 0;   // canonical index of the kernel tensor (RNG init stream)
    // bn
    int64_t gamma_off = 0, beta_off = 0, mm_off = 0, mv_off = 0;
    int relu_after = 0, mask_in_pos = 0;
    int fuse_pool = 0;         // bn: the next op is the max-pool of this BN's output -> one fused kernel, output never materialised
    int feeds_bn = 0;          // conv: the next op is the BatchNorm of this conv's output (statistics fused into the epilogue)
    float* bn_buf = nullptr;   // mean | invstd | scale | shift, each [C]
    // pool
    uint8_t* arg = nullptr;
    int mask_y_pos = 0;
    int fused_into_bn = 0;     // pool: executed inside the preceding BatchNorm's fused kernels
};

// One KIND_KERNEL tensor of a plan (ops[op], of that kind): `channels` output channels of `len` elements, element e of channel
// c at off + c * chan_stride + e * elem_stride ([Cout][k k Cin] kernels: (len, 1); a depthwise [k][k][C] kernel: (1, C))
struct KernelTensor {
    int op;
    OpKind kind;
    int64_t off;
    int channels, len, chan_stride, elem_stride;
    int64_t elems() const { return (int64_t)channels * len; }
};

// The op list and activation shapes of a candidate, from the six genes: host arithmetic only.  Net::build_plan allocates
// for it; check_plan_ranges, cmoop_plan_convs and cmoop_net_launch_plan walk it without a device.
struct NetPlan {
    std::vector<Act> acts;
    std::vector<Op> ops;
    int logits = -1;
    int n_sites = 0;           // activation-quantisation sites: the acts with site >= 0, numbered in act order
    int64_t n_params = 0;
    // THE walk over the kernel tensors, in arena order (under param_kinds, the quant / prune tables, the seeded init, the flip table)
    std::vector<KernelTensor> kernel_tensors() const;
    // ParamKind of every arena element: conv / depthwise / pointwise / dense kernels, other trainable tensors (biases, gamma,
    // beta), BatchNorm moving statistics
    std::vector<uint8_t> param_kinds() const;
    // the net's shared split-K workspace for train batch `batch` and Bmax = max(batch, eval_batch)
    size_t splitk_floats(int batch, int Bmax) const;
    // ';'-joined launch-path variants (gemm_variant_name) of the MFMA conv launches of one train step (forward with the
    // statistics epilogue where a layer feeds a BatchNorm, then weight and data gradients in backward order) or of one
    // inference pass at batch B, in launch order, under that workspace
    std::string launch_plan(int batch, int Bmax, int B, bool train) const;
};
NetPlan plan_net(const int32_t gene[6], const NetConfig& cfg, int T, int F);
// host-only: the quantisation and the pruning table of a plan (kernels.h), one row per kernel_tensors() entry, finalised against
// plan.n_params.  Pruning rows have k = -1 (pruned at the sparsity of each launch); with skip_small the first convolution and
// the depthwise kernels have k = 0 (copied)
QuantTable quant_table(const NetPlan& plan);
// host-only: the ops that run integer under Net::set_int8 -- every OP_CONV / OP_DENSE whose input is an activation-quantisation
// site -- in op order.  Throws when such an op is beyond the integer kernels (int8_layer_ok) or its code rows would not be
// 16-byte aligned (w_off % 16)
struct Int8Op { int op, in, out, site; int64_t scale_off; };
std::vector<Int8Op> int8_ops(const NetPlan& plan);
// host-only: the ops that run integer under Net::set_int8_depthwise -- every OP_DWCONV -- in op order; site / out_site are the
// sites of its input and output.  Throws when one reads or writes an act that is no site, is beyond the kernel
// (int8_dw_layer_ok), or its code rows (w_off % 16) or scales (scale_off % 4) would not be 16-byte aligned
struct Int8DwOp { int op, in, out, site, out_site; int64_t scale_off; };
std::vector<Int8DwOp> int8_dw_ops(const NetPlan& plan);
// host-only: the ops of int8_ops that take the requantising epilogue under Net::set_int8_fused, in op order: the act they feed
// reaches an activation-quantisation site through per-channel elementwise ops only.  bn < 0 (T0): the op's own output act is the
// site.  bn >= 0 (T1): that OP_BN (not fused with a pool) is the only reader of the op's output and ITS output act is the site;
// relu_after is that BN's.  site_act / out_site: the act and the site the launch writes.  Throws when Cout % 4 != 0
struct Int8FusedOp { Int8Op i8; int bn, relu_after, site_act, out_site; };
std::vector<Int8FusedOp> int8_fused_ops(const NetPlan& plan);
PruneTable prune_table(const NetPlan& plan, bool skip_small = true);

// The optional training options of a candidate's fit, each null = off (kernels.h; Net::set_augment / set_loss /
// set_distill / set_optim / set_ema / set_opoint / set_quant / set_prune / set_actquant say what each does).  The pointees stay the caller's for the length of the call
struct TrainOptions {
    const AugmentCfg* aug = nullptr;
    const LossCfg* loss = nullptr;
    const DistillCfg* distill = nullptr;
    const OptimCfg* optim = nullptr;
    const EmaCfg* ema = nullptr;
    const OpointCfg* opoint = nullptr;
    const QuantCfg* quant = nullptr;
    const PruneCfg* prune = nullptr;
    const ActQuantCfg* actq = nullptr;
};

// What a captured train step (CMOOP_GRAPH=1, Net::train_step_stateful) froze and a later call can change under it;
// Net::capture_key fills it and lists why each field is there
struct StepCaptureKey {
    const float* X = nullptr;
    const int32_t* y = nullptr;
    const int32_t* idx = nullptr;
    int64_t gather_rows = 0;
    const float* alpha_tab = nullptr;
    const float* kd_zt = nullptr;
    int64_t kd_rows = 0;
    int env_knobs = 0;
    bool operator==(const StepCaptureKey& o) const {
        return X == o.X && y == o.y && idx == o.idx && gather_rows == o.gather_rows && alpha_tab == o.alpha_tab && kd_zt == o.kd_zt &&
               kd_rows == o.kd_rows && env_knobs == o.env_knobs;
    }
};
// process-wide totals since load of Net::train_step_stateful: {steps launched eagerly, steps replayed from a captured graph,
// captures made, captures dropped while their net lived}.  Host only: launches nothing, allocates nothing
void step_launch_counts(int64_t out[4]);

class Net : public GemmHook {
  public:
    const GemmTiming* begin(int cls, double flops) override;
    void end(int code, int flags) override;
    Net(const int32_t gene[6], const NetConfig& cfg, int T, int F, uint32_t seed, hipStream_t stream);
    ~Net();
    Net(const Net&) = delete;
    Net& operator=(const Net&) = delete;

    int64_t total_params() const { return n_params_; }
    void get_params(float* host);
    void set_params(const float* host);
    void get_grads(float* host);
    void snapshot_params();   // device copy (restore_best_weights) of the arena inference currently reads (use_average)
    void restore_snapshot();  // into the parameter arena; both carry the activation-quantisation site records with the weights
    // full training state: parameters (BatchNorm moving statistics included), Adam m / v, optimizer.iterations and the
    // global step that keys the dropout masks -- what a checker needs to re-synchronise with this net at an epoch boundary
    void get_state(float* params, float* m, float* v, long long* iterations, long long* steps);
    // the average arena of set_ema is NOT part of this state: set_state leaves it untouched, and a re-synchronising checker
    // calls set_average as well
    void set_state(const float* params, const float* m, const float* v, long long iterations, long long steps);
    // Train-time augmentation (kernels.h) of every following train step, both step paths; null or a disabled config: off,
    // and a step's launches and allocations are those of a net that never had one.  Enabled: each step first writes its
    // augmented batch (keyed by seed, the global step and the position in the batch) to a buffer of cfg.batch rows,
    // allocated on first use, which the first-layer kernels then read in place of the resident tensor.  Labels, loss,
    // dropout and Adam are untouched; evaluate / predict / predict_stream never augment.  Drops a captured step graph
    void set_augment(const AugmentCfg* aug);
    // Soft-target training loss (kernels.h) of every following train step, both step paths; null or a disabled config: off,
    // and a step's launches and allocations are those of a net that never had one.  Enabled: the domain is checked against
    // cfg.classes, the lam table and the class weights are uploaded, the target / weight / primary buffers (and, with mixup,
    // a second [cfg.batch][T][F] batch buffer) are allocated on first use; each step then blends its batch (mixup only),
    // builds t / w / primary after the forward pass and takes softmax_ce_kernel<CE_SOFT> in place of <CE_SPARSE>.
    // evaluate / predict / predict_stream and the validation loss of a fit stay the sparse cross-entropy.  Drops a captured
    // step graph
    void set_loss(const LossCfg* loss);
    // floats (int32 words) allocated for the mixup batch buffer, t, w and primary: 0 where the buffer does not exist
    void loss_buffers(int64_t out[4]) const;
    // Knowledge distillation (kernels.h) of every following train step, both step paths; null or a disabled config: off, and
    // a step's launches and bits are those of a net that never had one.  Enabled: the config is checked against cfg.classes
    // (n_rows against itself: the table's rows are what a step's gather rows must equal), q [cfg.batch][classes] and the
    // target buffers are allocated on first use; each step then builds t / w / primary (one-hot, unit weight and the label
    // under a default loss), the teacher rows q, and takes softmax_ce_kernel<CE_DISTILL> as its loss.  The table stays the
    // caller's and must outlive the steps.  Inference and the validation loss are untouched.  Drops a captured step graph
    void set_distill(const DistillCfg* distill);
    // Optimiser options (kernels.h) of every following train step, both step paths; null or a disabled config: off, and a
    // step's launches and bits are those of a net that never had one.  A schedule alone keeps the fused optimiser launch and
    // only changes the step-size table (rebuilt here when a fit is under way).  Weight decay or a clip: the finish + update
    // path (grad_finish -> clip_scale -> adamw); the kind arena, the partial buffer (sized once for the worst workgroup
    // count) and the device record are allocated on first use, and the step is no longer captured as a graph
    void set_optim(const OptimCfg* optim);
    // Weight EMA (kernels.h) of every following train step, every step path and both optimiser paths; null or a disabled
    // config: off, and a step's launches and bits are those of a net that never had one (an average arena that already
    // exists is kept but no longer advanced).  Enabled: the domain is checked; on first use the average arena, the kind
    // arena and (when a fit is under way) the rate table are allocated and the average becomes a bit copy of the parameter
    // arena -- a later call with other values keeps the average.  Each step then launches launch_ema after the optimiser's
    // launch(es): the training trajectory is never touched.  The step is no longer captured as a graph
    void set_ema(const EmaCfg* ema);
    bool has_average() const { return ema_ != nullptr; }
    bool average_on() const { return ema_on_; }            // train steps advance the average
    // inference switch: while on, evaluate / predict / predict_logits / predict_stream (and snapshot_params) read the average
    // arena in place of the parameters -- a host-side pointer swap, no copy.  Must be off again before the next train step
    // (a step refuses otherwise); get_params / set_params / get_state / set_state always mean the raw parameters
    void use_average(bool on);
    void get_average(float* host);
    void set_average(const float* host);
    void finalize_average();   // w := a (Keras' finalize_variable_values); Adam's moments, the counters and a stay
    // Operating-point read-out (kernels.h) of every following fit_and_read_out on this net; null or a disabled config: off, and
    // the fit's launches and allocations are those of a net that never had one.  Enabled: the domain is checked and the config
    // copied.  No train step, validation pass or earlier read-out changes: after the weights are final the fit runs ONE more
    // predict over the validation split and the three read-out launches, and keeps the record for last_opoint
    void set_opoint(const OpointCfg* op);
    const OpointCfg& opoint() const { return opoint_cfg_; }
    // the record of the last fit_and_read_out: classes [cfg.classes] and summary [4]; throws when that fit ran without the option
    void last_opoint(OpointClass* classes, double summary[4]) const;
    void store_opoint(const OpointClass* classes, const double summary[4]);   // classes null: the last fit had none
    // Quantisation-aware training (kernels.h) of every following train step and inference call; null or a disabled config: off,
    // and every launch and bit is that of a net that never had one (the quantised arena, once allocated, is kept).  Enabled:
    // the domain is checked; on first use the table is built from the plan and uploaded and the quantised arena allocated.
    // Every train step and inference call then starts with the weight stage (stage_kernels); forward, backward and the
    // flip-transposed dgrad operands read the kernels from the arena it returns and everything else (biases, gamma, beta, moving
    // statistics and their writes) from the parameter arena; the gradients go unchanged to the latent weights (straight-through),
    // which the optimiser, the EMA, get/set_params and the snapshots keep meaning.  The step is no longer captured as a graph
    void set_quant(const QuantCfg* quant);
    bool quant_on() const { return quant_on_; }
    const QuantCfg& quant() const { return quant_cfg_; }
    // the arena inference would read now, quantised: wq [n_params] (kernels dequantised, every other element copied), codes
    // [n_params] (0 outside the kernel tensors), scales [the table's total_channels]; any may be null.  Throws while the option is off
    void get_quantized(float* wq_host, int8_t* codes_host, float* scales_host);
    int64_t quant_size_bytes();          // kernels.h, at the bits of the config; throws while the option is off
    // Magnitude pruning (kernels.h) of every following train step and inference call; null or a disabled config: off, and every
    // launch and bit is that of a net that never had one (the pruned arena, once allocated, is kept).  Enabled: the domain is
    // checked; on first use the table is built from the plan and uploaded, the pruned arena and the select's workspace allocated.
    // As set_quant from there on: the weight stage of a train step prunes at prune_sparsity_at(cfg, iterations_), that of an
    // inference call at the FINAL sparsity, whatever the iteration; straight-through, so a pruned weight can regrow
    void set_prune(const PruneCfg* prune);
    bool prune_on() const { return prune_on_; }
    const PruneCfg& prune() const { return prune_cfg_; }
    // the arena inference would read now, pruned at the final sparsity (not quantised): weff [n_params] (every other element
    // copied) and zeros [rows of the table]: the elements of each tensor that became zero; either may be null.  Throws while off
    void get_pruned(float* weff_host, uint32_t* zeros_host);
    int prune_rows();                    // rows of the table (the length of zeros)
    // sum of zeros / sum of len over the tensors with k > 0 at the final sparsity (0 when there is none)
    double prune_achieved(const uint32_t* zeros);
    int64_t prune_size_bytes();          // kernels.h, at the final sparsity and the quantiser's bits; throws while the option is off
    // Activation fake quantisation (kernels.h) of every following train step and inference call; null or a disabled config: off,
    // and every launch and bit is that of a net that never had one (the site records, once allocated, are kept).  Enabled: the
    // domain is checked; on first use the per-site records (zeroed: count 0) and the partials workspace are allocated.  forward
    // then quantises every site (plan_net) in place right after the op that writes it: train steps in batch mode, which also
    // advances the site's record, inference in tracked mode -- refused, before anything is launched, while no train step has run
    // with the option on and no ranges were loaded.  backward is unchanged.  Independent of set_quant / set_prune.  Under
    // use_average the ranges stay those of the raw-weight trajectory.  The step is no longer captured as a graph
    void set_actquant(const ActQuantCfg* actq);
    bool actquant_on() const { return actq_on_; }
    const ActQuantCfg& actquant() const { return actq_cfg_; }
    int act_sites() const { return plan_.n_sites; }
    // the site records {m_b, r, count}, [act_sites()]; throws while no records exist (the option was never on).  set: count >= 0
    // and r not negative; a record with count > 0 makes inference possible
    void get_act_ranges(ActRange* host);
    void set_act_ranges(const ActRange* host);
    // Integer inference (kernels.h; include/cmoop.h fixes the arithmetic).  on: refused, before anything is launched and with the
    // net unchanged, unless set_quant and set_actquant are both on and the ranges are ready, or when a tracked r or a weight
    // scale (both read on the host here) is not finite.  First use allocates the weight-code arena, the scale buffer and one int8
    // buffer per site.  While on, every inference pass stages the weights with codes and scales, the tracked apply kernel writes
    // each site's codes next to its fp32 tensor, and the ops of int8_ops(plan) take the integer launch in place of the fp32 one
    // (gemm_mode is ignored by them); every other launch, and every train step, is what it was.  Turning set_quant or
    // set_actquant off turns the mode off as well.  The finiteness check is made when enabling and by set_act_ranges while the
    // mode is on, NOT per pass: a train step or set_params that later produces a NaN or Inf range or scale is not caught, and
    // the integer passes then return NaN logits without a fault, as the fp32 passes do
    void set_int8(bool on);
    bool int8_on() const { return int8_.on; }
    // Integer depthwise, the second level of integer inference (include/cmoop.h, "Integer depthwise").  on: refused unless
    // set_int8 is on.  While on, every OP_DWCONV of an inference pass is ONE launch that reads the input site's codes and the
    // staged weight codes and writes the output site's quantised fp32 tensor and its codes: the fp32 depthwise launch and the
    // site's quantiser launch are not made.  Train steps never take it.  A plan without a depthwise op accepts it and does
    // nothing.  Turning set_int8, set_quant or set_actquant off turns it off
    void set_int8_depthwise(bool on);
    bool int8_depthwise_on() const { return int8_.depthwise; }
    // The requantising epilogue, the third level of integer inference (include/cmoop.h, "Integer inference: requantising
    // epilogue"), independent of the depthwise level.  on: refused unless set_int8 is on.  While on, every op of int8_fused_ops
    // is ONE launch in an inference pass: it applies the op's bias / ReLU, the eval BatchNorm that follows it (whose
    // bn_eval_prepare launch moves ahead of it) and the quantiser of the site, and writes the site's fp32 tensor and codes: the
    // scale_shift launch and the site's quantiser launch are not made, and the pre-BatchNorm act is not written.  Train steps
    // never take it.  A plan without such an op accepts it and does nothing.  Turning set_int8, set_quant or set_actquant off
    // turns it off
    void set_int8_fused(bool on);
    bool int8_fused_on() const { return int8_.fused; }
    const NetPlan& plan() const { return plan_; }
    // debug read-out: dims = {H, W, C, materialised, has a gradient, number of acts} of act i; data / grad (either may be null)
    // receive the first B rows as the last step or pass left them (grad: B <= cfg.batch).  Under set_int8_fused an inference pass
    // does not write the act between a fused op and its BatchNorm (nothing reads it): it keeps what an earlier pass or step left
    void get_act(int i, int B, int32_t dims[6], float* data_host, float* grad_host);
    // the enabled ones of o through the nine setters above, in that order: augment, loss, distill, optim, ema, opoint, quant, prune, actq.  THE
    // place of "a disabled config is no config": null or disabled is not applied at all, and the net stays one that never had it
    void set_options(const TrainOptions& o);
    // the last step's {sum of squares, norm, scale, launch path (0 fused, 1 finish + update)}; path 0 computes no norm: 0, 0, 1
    void optim_stats(double out[4]);
    // rows of the resident tensor the next train steps gather from (0: unknown, no clamp)
    // with distillation on, n must be the rows of the teacher table: refused here, before any step is enqueued
    void set_gather_rows(int64_t n);
    // ONE epoch of Model.fit on the production path (device permutation of (seed, epoch) when cfg.shuffle, device
    // StepState steps, last partial batch kept).  The permutation goes into a buffer of the net, which stays where it is from
    // epoch to epoch (a captured step keeps reading it) and grows when a longer split comes
    void run_epoch(const float* X, const int32_t* y, int64_t n_train, int epoch);

    // fwd + bwd + Adam on rows idx[row0 .. row0+B) (idx may be null -> rows row0..)
    void train_step(const float* X, const int32_t* y, const int32_t* idx, int64_t row0, int B);
    // one optimiser step on caller-built rows and targets: x_rows [B][T][F], t [B][classes], w [B] (null: 1), primary [B]
    // (null: the first maximum of t), all on the device.  No augmentation, no mixing, no target construction, whatever
    // set_augment / set_loss say; dropout, Adam and the counters advance as in train_step
    void train_step_targets(const float* x_rows, const float* t, const float* w, const int32_t* primary, int B);
    // train_step_targets with a caller-built teacher row q [B][classes] and the distillation loss at (alpha, temperature),
    // whatever set_distill says
    void train_step_distill_targets(const float* x_rows, const float* t, const float* w, const int32_t* primary, const float* q,
                                    double alpha, double temperature, int B);
    // The fit loop's form of the same step: the batch position, dropout counter and Adam iteration live in a device
    // StepState (kernels.h), so a full-batch step has no per-step host arguments; with CMOOP_GRAPH=1 it is captured ONCE
    // as a hipGraph and replayed (opt-in: measured no faster than eager launches, see begin_fit).
    // A capture freezes every host-side argument of the step's launches.  What of that can change while the net lives is in
    // StepCaptureKey (above; capture_key in net.hip is the complete list): the caller's X / y / idx, the split length, the
    // step-size table, the teacher table and the per-step environment knobs.  train_step_stateful compares the key before
    // every replay; a mismatch drops the capture and the same step captures again.  Every option setter and set_state drop
    // it too (option_changed), and so does a re-entered begin_fit, which also gives the previous tables back to the pool.
    // Steps that are never captured or replayed: step 0, partial batches, profiled steps, and every step of a net with an
    // AdamW / clipping optimiser, EMA, weight or activation quantisation or pruning on.  step_launch_counts() says which
    // of these happened.
    void begin_fit(int64_t total_steps);      // uploads Adam's per-iteration step sizes, sets the device state to (0, step, iterations)
    void begin_epoch();                       // state.row0 = 0
    void train_step_stateful(const float* X, const int32_t* y, const int32_t* idx, int B);
    // inference over n rows of (X, y); returns sum of per-sample losses and #correct, fills preds (device, may be null)
    void evaluate(const float* X, const int32_t* y, int64_t n, double* loss_sum, long long* correct, int32_t* preds);
    // Model.predict: probs [n][classes] (device) of n rows of X, inference mode, eval_batch rows per launch
    void predict(const float* X, int64_t n, float* probs);
    // the same pass with the logits themselves copied out, logits [n][classes] (device): what predict's softmax reads
    void predict_logits(const float* X, int64_t n, float* logits);
    // the same over the windows [i hop, i hop + T) of a feature stream [n_frames][F]: eval_batch windows at a time are
    // gathered (per-window dB tail when db_scale, StandardScaler when mean / scale: host doubles [F]) into one chunk buffer
    void predict_stream(const float* feat, int64_t n_frames, int hop, bool db_scale, bool db_ref_max, float db_amin, float top_db,
                        const double* mean, const double* scale, float* probs);
    void read_train_metrics(double* loss_sum, long long* correct, bool reset);
    void drain_profile();
    hipStream_t stream() const { return stream_; }
    uint32_t seed() const { return seed_; }
    const NetConfig& config() const { return cfg_; }
    int feature_T() const { return T_; }
    int feature_F() const { return F_; }
    long long steps_done() const { return step_; }
    long long iterations_done() const { return iterations_; }

  private:
    void build_plan();
    // rows: where the batch's rows lie in X (kernels.h); the first layer clamps by rows.n_rows in training only
    void forward(const float* X, const BatchRows& rows, int B, bool train);
    void backward(const float* X, const BatchRows& rows, int B);
    // THE step: refused under use_average; weight stage at this iteration's sparsity, [gather: augment / mixup into batch_in_],
    // forward, loss(), backward, optimiser_step.  rows.st: the device state the step reads and advances, null: host arguments
    template <class Loss> void step_body(const float* X, const BatchRows& rows, int B, bool gather, Loss&& loss);
    void gathered_step(const float* X, const int32_t* y, const BatchRows& rows, int B);   // step_body, gathering, with launch_train_loss
    // the targets launches set_loss / set_distill ask for, then the matching softmax_ce launch
    void launch_train_loss(const int32_t* y, const BatchRows& rows, int B);
    template <class Body> void counted_step(Body&& body);   // body() under the step's ProfilingScope, then the counters advance
    // THE inference pass: weight stage at the final sparsity, then per chunk of eval_batch rows (the last one partial)
    // source(s, B) -> {X, rows} of rows [s, s + B), forward in inference mode, sink(s, B) on their logits
    template <class Source, class Sink> void inference_pass(int64_t n, Source&& source, Sink&& sink);
    void optimiser_step(int B, const StepState* st);   // the tail of a step: weight-gradient slabs summed + Adam (+ state advance)
    void upload_rate_tables();                          // alpha_tab_ (and, on the finish + update path, lr_tab_) from optim_rates; ema_tab_ from ema_rates
    void ensure_kinds();                                // kinds_dev_, uploaded once (set_optim's finish path and set_ema share it)
    void option_changed(bool breaks_graph);             // every setter's tail: the captured step is stale; breaks_graph: and none is captured again
    void require_step_allowed(bool gather) const;       // the whole-step refusals, before anything is enqueued: step_body's first lines, and in front of every replay
    StepCaptureKey capture_key(const float* X, const int32_t* y, const int32_t* idx) const;   // what a capture made now would freeze
    void dfree(void* p);                                // a dalloc'd buffer back to the pool (the caller has drained the stream); null: no-op
    void upload_step_state();                           // enqueues the device StepState at (0, step_, iterations_); no-op without one
    void ensure_target_buffers();                       // t / w / primary, allocated by the first enabled set_loss or set_distill
    void ensure_quant_table();                          // qtab_ from the plan, once (host only)
    void ensure_prune_table();                          // ptab_ from the plan and the config's skip_small (host only)
    void require_act_ranges() const;                    // first line of every public inference entry: with set_actquant on, tracked ranges
    void quantise_site(int act, int B, bool train);     // forward's launch(es) for a site the op just wrote
    // the integer work of op oi in an inference pass, by int8_ and int8_tab_: the op's integer launch (a fused op's
    // bn_eval_prepare ahead of it), or nothing.  What forward still owes the op:
    enum Int8Done {
        INT8_NOT_HERE,     // not integer here: run the fp32 launch
        INT8_WROTE_OUT,    // wrote the op's output: quantise the site as usual
        INT8_WROTE_SITE    // wrote the site itself (or a fused producer did, for its BatchNorm): skip the quantiser
    };
    Int8Done forward_int8(size_t oi, int B);
    void int8_levels_off() { int8_ = Int8Levels(); }    // set_quant / set_actquant off and set_int8(false): no level outlives them
    // THE weight stage, from params_ (the average under use_average).  Prune on: its kernels pruned at `sparsity` into wp (zeros:
    // per-row counts, or null).  Quant on and wq given: the kernels of wp, else of params_, quantised into wq (codes / scales or
    // null).  Returns the arena of the last stage that ran, params_ when none did: where forward / backward read kernel tensors
    const float* stage_kernels(double sparsity, float* wp, uint32_t* zeros, float* wq, int8_t* codes, float* scales);
    void refresh_kernels(double sparsity) { kernels_ = stage_kernels(sparsity, wp_, nullptr, wq_, nullptr, nullptr); }
    ConvBuffers buffers_of(const Op& op) const;   // the slices of the arenas an OP_CONV's launches use
    float* dalloc(size_t floats);

    int32_t gene_[6];
    NetConfig cfg_;
    int T_, F_, Bmax_;
    uint32_t seed_;
    hipStream_t stream_;
    NetPlan plan_;                      // the plan the net was built from; build_plan fills its acts' and ops' device pointers in place
    std::vector<Act>& acts_ = plan_.acts;
    std::vector<Op>& ops_ = plan_.ops;
    const int& logits_ = plan_.logits;
    const int64_t& n_params_ = plan_.n_params;
    std::vector<void*> allocs_;
    float *params_ = nullptr, *grads_ = nullptr, *adam_m_ = nullptr, *adam_v_ = nullptr, *snap_ = nullptr;
    const float* kernels_ = nullptr;    // refresh_kernels
    float* weights_ = nullptr;          // the parameter arena; params_ (what forward reads) is this, or ema_ under use_average
    float* ema_ = nullptr;              // the average arena, allocated by the first enabled set_ema
    EmaCfg ema_cfg_;                    // set_ema; the default is off
    bool ema_on_ = false;               // train steps advance ema_ after the optimiser launch(es)
    EmaPair* ema_tab_ = nullptr;        // (mf, omf) per iteration, alpha_tab_n_ entries, next to alpha_tab_
    OpointCfg opoint_cfg_;              // set_opoint; the default is off
    QuantCfg quant_cfg_;                // set_quant; the default is off
    bool quant_on_ = false;             // steps and inference calls quantise first and read kernels from wq_
    float* wq_ = nullptr;               // the quantised arena (only kernel elements are ever written or read), first enabled set_quant
    QuantTable qtab_;                   // host table of the plan's kernel tensors
    bool qtab_ready_ = false;
    QuantRow* qtab_dev_ = nullptr;
    PruneCfg prune_cfg_;                // set_prune; the default is off
    bool prune_on_ = false;             // steps and inference calls prune first and read kernels from wp_ (or quantise wp_)
    float* wp_ = nullptr;               // the pruned arena (only kernel elements are ever written or read), first enabled set_prune
    PruneTable ptab_;                   // host table of the plan's kernel tensors
    int ptab_skip_small_ = -1;          // the skip_small ptab_ was built with; -1: not built
    PruneRow* ptab_dev_ = nullptr;
    PruneWorkspace prune_ws_;
    ActQuantCfg actq_cfg_;              // set_actquant; the default is off
    bool actq_on_ = false;              // forward quantises the sites
    ActRange *act_rec_ = nullptr, *act_rec_snap_ = nullptr;   // [n_sites] records and their snapshot_params copy, first enabled set_actquant
    uint32_t* act_partials_ = nullptr;  // [ACT_QUANT_MAX_BLOCKS] absmax partials of the site being quantised
    bool act_ranges_ready_ = false, act_ranges_ready_snap_ = false;   // host mirror of "every record has count > 0", and of the snapshot's
    // the three levels of integer inference: set_int8 (the matrix-core ops), set_int8_depthwise, set_int8_fused
    struct Int8Levels { bool on = false, depthwise = false, fused = false; } int8_;
    int8_t* w_codes_ = nullptr;         // [n_params] weight codes (only kernel elements are ever written or read), first set_int8(true)
    float* w_scales_ = nullptr;         // [qtab_.total_channels]
    std::vector<int8_t*> site_codes_;   // per site: [Bmax][per_sample] activation codes
    // per op, what integer inference can make of it; each level fills its part when it is turned on (the first set_int8 the
    // matrix-core ops) and the level's flag in int8_ says whether a pass uses it: a fused op runs as a matrix-core op and the
    // BatchNorm it would apply as itself while the fused level is off, a depthwise op in fp32 while the depthwise level is off
    enum Int8Role : uint8_t { I8_NONE, I8_MATRIX, I8_DEPTHWISE, I8_FUSED, I8_FUSED_BN /* a BatchNorm a fused op applies */ };
    struct Int8Entry {
        Int8Role role = I8_NONE;
        int64_t scale_off = -1;         // first scale of the op's kernel tensor
        int bn = -1, site_act = -1;     // I8_FUSED: the BatchNorm op it applies (-1: none) and the act (a site) it writes
    };
    std::vector<Int8Entry> int8_tab_;
    std::vector<OpointClass> last_op_classes_;   // store_opoint: empty when the last fit ran without the read-out
    double last_op_summary_[4] = {0, 0, 0, 0};
    float *wgrad_ws_ = nullptr, *wd_ws_ = nullptr, *red_ws_ = nullptr, *splitk_ws_ = nullptr;
    bool aug_on_ = false;               // train steps read aug_buf_ (set_augment)
    AugmentParams aug_;
    float* aug_buf_ = nullptr;          // [cfg.batch][T][F], allocated by the first enabled set_augment
    bool loss_on_ = false, mix_on_ = false;   // train steps take the soft-target loss / blend their batch first (set_loss)
    MixupParams mixp_;                  // tab: lam_tab_
    TargetParams tgtp_;                 // cw: cw_dev_ or null
    float *lam_tab_ = nullptr, *cw_dev_ = nullptr;
    float* mix_buf_ = nullptr;          // [cfg.batch][T][F], allocated by the first set_loss with mixup on
    float *tgt_t_ = nullptr, *tgt_w_ = nullptr;   // [cfg.batch][classes], [cfg.batch]: ensure_target_buffers
    int32_t* tgt_primary_ = nullptr;    // [cfg.batch]
    bool distill_on_ = false;           // train steps take the distillation loss (set_distill)
    DistillParams kdp_;
    const float* kd_zt_ = nullptr;      // the caller's teacher table [kd_rows_][classes]
    int64_t kd_rows_ = 0;
    float* kd_q_ = nullptr;             // [cfg.batch][classes], allocated by the first enabled set_distill
    const float* batch_in_ = nullptr;   // this train step's gathered batch (mix_buf_ / aug_buf_), null: rows come from (X, rows)
    StepState* st_dev_ = nullptr;       // device step state (train_step_stateful)
    StepState st_up_{};                 // what upload_step_state copies from: outlives the enqueued copy
    float* alpha_tab_ = nullptr;        // Adam step size per iteration
    OptimCfg optim_;                    // set_optim; the default is today's constant-rate Adam
    bool optim_finish_ = false;         // train steps take the finish + update path (decay or a clip is set)
    float* lr_tab_ = nullptr;           // un-corrected rate per iteration (weight decay), alpha_tab_n_ entries; finish + update path only
    uint8_t* kinds_dev_ = nullptr;      // ParamKind per arena element, uploaded once
    float* optim_partials_ = nullptr;   // one sum of squares per grad_finish workgroup
    int64_t optim_partials_cap_ = 0;
    OptimRecord* optim_rec_ = nullptr;
    int optim_last_path_ = 0;
    int64_t alpha_tab_n_ = 0, host_row0_ = 0, gather_rows_ = 0;
    hipGraphExec_t graph_exec_ = nullptr;   // the captured full-batch train step
    StepCaptureKey graph_key_;              // what graph_exec_ froze; compared before every replay
    bool graph_ok_ = true;
    int32_t* epoch_idx_ = nullptr;          // run_epoch's permutation buffer, grown on demand
    int64_t epoch_idx_n_ = 0;
    FlipEntry* flip_table_ = nullptr;   // device table of the conv layers whose dgrad needs flip-transposed weights
    int flip_layers_ = 0;
    int64_t flip_max_elems_ = 0;
    std::vector<AdamSeg> slab_segs_;    // this step's unreduced weight-gradient slabs (backward fills, the optimiser launch consumes)
    size_t wgrad_ws_floats_ = 0, wd_ws_floats_ = 0, red_ws_floats_ = 0, splitk_ws_floats_ = 0;
    double* acc_train_ = nullptr;   // [2]: loss sum, correct (int64 bits)
    double* acc_eval_ = nullptr;
    long long step_ = 0, iterations_ = 0;
    bool profiling_now_ = false, hook_live_ = false;
    int fused_stats_blocks_ = 0;   // > 0: the conv just launched left this many BatchNorm statistic partials in red_ws_
    struct EvPair { GemmTiming t; double flops; int cls, code, flags; };
    std::vector<EvPair> ev_pool_;
    size_t ev_used_ = 0;
};

struct EvalResult {
    double acc = 0, size_mb = 0, fpr = 0, val_loss = 0, seconds = 0;
    int epochs_run = 0;
    int evaluated = 0;   // 1 when THIS call trained the candidate (always, unless a pull callback handed it to another rank)
    // the operating-point read-out (Net::set_opoint): fpr_at_recall, recall_achieved, macro_auc, n_scored; zeros when it is off
    double opoint[4] = {0, 0, 0, 0};
    // quantisation-aware training (Net::set_quant): quant_size_bytes / 2^20, bits; zeros when it is off
    double quant[2] = {0, 0};
    // magnitude pruning (Net::set_prune): prune_size_bytes / 2^20, the final sparsity, the zero fraction of the pruned tensors
    // of the scored model; zeros when it is off
    double prune[3] = {0, 0, 0};
};

// per-epoch record of a fit (tests: the early-stopping decisions are checked against the validation-loss history)
struct FitHistory {
    std::vector<double> val_loss, val_acc;
    int best_epoch = -1;
};
// Model.fit + EarlyStopping + the read-outs on an EXISTING net (the body of run_candidate); seed keys the epoch shuffle
EvalResult fit_and_read_out(Net& net, const NetConfig& cfg, const Dataset& ds, uint32_t seed, FitHistory* hist = nullptr);
// train-to-early-stop + readouts for one candidate (evaluate_individual, nsga_penalty.py:368-395)
// opt: the training options of the candidate's fit (Net::set_options)
EvalResult run_candidate(const int32_t gene[6], const NetConfig& cfg, const Dataset& ds, uint32_t seed, hipStream_t stream,
                         const TrainOptions& opt = {});
// host-only: every implicit-GEMM conv geometry of a candidate at batch B (a walk of plan_net's ops); throws
// through igemm_check_range when a layer is beyond the kernels' 32-bit byte offsets (depthwise activations: 2^29 elements)
void check_plan_ranges(const int32_t gene[6], int variant, int T, int F, int B);
// the population loop (compute_objectives_and_constraints, nsga_penalty.py:418-442): n_slots
// candidates in flight on their own HIP streams, longest-first
// pull (optional): called by the worker threads (concurrently) for the next candidate index, < 0 = queue exhausted --
// lets several ranks drain ONE longest-first queue (cross-rank dynamic scheduling, evaluator.py); without it the
// n candidates are taken longest-first from a process-local counter.  opt: every candidate's training options.
void eval_population(const NetConfig& cfg, const Dataset& ds, const int32_t* genes, const uint32_t* seeds, int n,
                     EvalResult* out, const std::function<int()>& pull = {}, const TrainOptions& opt = {});

// host-only: windows of T frames at hop frames in a stream of n_frames, 1 + (n_frames - T) / hop; throws when n_frames < T or hop < 1
int64_t stream_windows(int64_t n_frames, int T, int hop);
double fpr_from_confusion(const int64_t* cm, int C, int variant);
// the operating-point read-out of probs [n][C] against y [n] (device pointers) at `recall`: keys, counts and select on s with
// pooled workspaces, every byte written before it is read; classes [C] and summary [4] are host arrays (kernels.h, OpointClass)
void operating_point(const float* probs, const int32_t* y, int64_t n, int C, double recall, OpointClass* classes, double summary[4],
                     hipStream_t s);
void epoch_permutation(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out);

}  // namespace cmoop
