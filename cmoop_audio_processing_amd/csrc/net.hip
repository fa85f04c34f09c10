// Candidate network: plan, training step, inference, early-stopped fit and the
// population driver.  See net.h for the reference lines each piece replaces.
#include "net.h"

#include <algorithm>
#include <cctype>
#include <cerrno>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <numeric>
#include <thread>

namespace cmoop {

static const int FC_LADDER[5][4] = {{0, 0, 0, 0}, {64, 0, 0, 0}, {128, 64, 0, 0}, {256, 128, 64, 0}, {512, 256, 128, 64}};

void validate_gene(const int32_t g[6]) {
    const bool ok = (g[0] == 16 || g[0] == 32 || g[0] == 64) && (g[1] == 3 || g[1] == 5) && (g[2] == 0 || g[2] == 1) &&
                    (g[3] >= 1 && g[3] <= 3) && (g[4] >= 1 && g[4] <= 4) && (g[5] == 0 || g[5] == 1);
    CMOOP_REQUIRE(ok, "gene outside the search space (filters{16,32,64}, kernel{3,5}, bn{0,1}, res{1..3}, fc{1..4}, dropout{0,1})");
}

DropoutParams dropout_params(double rate) {
    CMOOP_REQUIRE(rate >= 0.0 && rate < 1.0, "dropout must be in [0,1)");
    return DropoutParams{(uint32_t)(rate * 16777216.0), (float)(1.0 / (1.0 - rate))};
}

int64_t param_count(const int32_t g[6], int variant, int classes) {
    validate_gene(g);
    CMOOP_REQUIRE(variant >= 0 && variant <= 3, "variant must be CMOOP_VARIANT_A, _B, _A_DS or _B_DS");
    const int64_t f = g[0], kk = (int64_t)g[1] * g[1], bn = g[2], R = g[3], fc = g[4];
    const bool ds = variant_is_ds(variant);
    // a k x k stride-1 conv with C_in >= 16: full, or depthwise [k][k][cin] + pointwise [cout][cin] + bias
    auto convp = [&](int64_t cin, int64_t cout) { return ds ? kk * cin + cin * cout + cout : kk * cin * cout + cout; };
    int64_t p, c = f;
    if (variant_is_a(variant)) {
        p = (kk * f + f) + convp(f, f) + (bn ? 8 * f : 0);
        for (int r = 0; r < R; ++r) {
            p += c * 2 * c + 2 * c;
            p += convp(c, 2 * c);
            p += convp(2 * c, 2 * c);
            p += bn ? 16 * c : 0;
            c *= 2;
        }
    } else {
        p = (kk * f + f) + (bn ? 4 * f : 0);
        for (int r = 0; r < R; ++r) {
            p += c * 2 * c + 2 * c;
            p += convp(c, 2 * c);
            p += bn ? 8 * c : 0;
            c *= 2;
        }
    }
    int64_t prev = c;
    for (int i = 0; i < fc; ++i) {
        const int64_t u = FC_LADDER[fc][i];
        p += prev * u + u;
        prev = u;
    }
    p += prev * classes + classes;
    return p;
}

double fwd_flops_per_sample(const int32_t g[6], int variant, int classes, int T, int F) {
    validate_gene(g);
    CMOOP_REQUIRE(variant >= 0 && variant <= 3, "variant must be CMOOP_VARIANT_A, _B, _A_DS or _B_DS");
    const double f = g[0], kk = (double)g[1] * g[1];
    const int R = g[3], fc = g[4];
    const bool A = variant_is_a(variant), ds = variant_is_ds(variant);
    auto convf = [&](double hw, double cin, double cout) { return ds ? 2.0 * hw * kk * cin + 2.0 * hw * cin * cout : 2.0 * hw * kk * cin * cout; };
    double fl = 2.0 * T * F * kk * f;
    if (A) fl += convf((double)T * F, f, f);
    int h = (T + 1) / 2, w = (F + 1) / 2;
    double c = f;
    for (int r = 0; r < R; ++r) {
        const int h2 = (h + 1) / 2, w2 = (w + 1) / 2;
        fl += 2.0 * h2 * w2 * c * 2 * c;
        fl += convf((double)h * w, c, 2 * c);
        if (A) fl += convf((double)h * w, 2 * c, 2 * c);
        h = h2; w = w2; c *= 2;
    }
    double prev = c;
    for (int i = 0; i < fc; ++i) {
        fl += 2.0 * prev * FC_LADDER[fc][i];
        prev = FC_LADDER[fc][i];
    }
    fl += 2.0 * prev * classes;
    return fl;
}

ProfileTotals& profile_totals() {
    static ProfileTotals t;
    return t;
}

// ---------------------------------------------------------------------------
// Device-memory cache shared by the candidates of a process.  hipFree waits for the work already queued on EVERY
// stream of the device, so tearing a candidate down buffer by buffer (~100 buffers) stalls its worker while the other
// streams' queues drain; candidates of one search reuse a handful of buffer sizes, so finished candidates hand their
// buffers to the next one instead.  Buffers are handed out with stale contents (as hipMalloc may): every consumer
// writes before it reads -- tests/test_gpu_stale_memory.py holds that sentence: under CMOOP_POOL_FILL=<byte> (below) every
// result the library returns is bit-identical whatever the buffers held.  CMOOP_POOL_GB caps the cached bytes (default 96;
// 0 disables the cache).

// CMOOP_POOL_FILL=<byte> (decimal or 0x.., 0..255; read at each allocation, as CMOOP_ADAM_UNFUSED is per step: tests flip it):
// -1 when unset or empty -- the plain path -- and a throw naming the variable for anything else that is no byte
int pool_fill_value() {
    const char* e = std::getenv("CMOOP_POOL_FILL");
    if (!e || !e[0]) return -1;
    char* end = nullptr;
    errno = 0;
    const long v = std::strtol(e, &end, 0);
    CMOOP_REQUIRE(errno == 0 && end != e && *end == 0 && v >= 0 && v <= 255 && e[0] != '-' && e[0] != '+' && !std::isspace((unsigned char)e[0]),
                  std::string("CMOOP_POOL_FILL must be a byte 0..255, decimal or 0x.. (got '") + e + "')");
    return (int)v;
}

// the whole of a buffer about to be handed out := fill (a blocking memset: the caller's stream sees it whatever its flags)
void pool_fill_device(void* p, size_t bytes, int fill) {
    if (fill < 0 || !p || !bytes) return;
    CMOOP_HIP(hipMemset(p, fill, bytes));
    CMOOP_HIP(hipStreamSynchronize(nullptr));
}

namespace {
class DevicePool {
  public:
    explicit DevicePool(bool host) : host_(host) {}
    void* get(size_t bytes) {
        const int fill = pool_fill_value();   // before anything is taken: a bad value fails the call and leaks nothing
        const size_t want = round_up(bytes);
        int dev = 0;
        CMOOP_HIP(hipGetDevice(&dev));
        void* p = nullptr;
        size_t have = 0;
        if (cap_bytes() > 0) {
            std::lock_guard<std::mutex> l(mu_);
            auto& fl = free_[dev];
            auto it = fl.lower_bound(want);
            if (it != fl.end() && it->first <= want + want / 8) {
                p = it->second;
                have = it->first;
                cached_ -= it->first;
                sizes_[p] = it->first;
                fl.erase(it);
            }
        }
        if (!p) {
            if (host_) CMOOP_HIP(hipHostMalloc(&p, want));
            else CMOOP_HIP(hipMalloc(&p, want));
            have = want;
            std::lock_guard<std::mutex> l(mu_);
            sizes_[p] = want;
        }
        if (fill >= 0) {
            if (host_) std::memset(p, fill, have);
            else pool_fill_device(p, have, fill);
        }
        return p;
    }
    void put(void* p) {
        if (!p) return;
        size_t bytes = 0;
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess) dev = 0;
        {
            std::lock_guard<std::mutex> l(mu_);
            auto it = sizes_.find(p);
            if (it != sizes_.end()) { bytes = it->second; sizes_.erase(it); }
            if (bytes && cached_ + bytes <= cap_bytes()) {
                free_[dev].emplace(bytes, p);
                cached_ += bytes;
                return;
            }
        }
        if (host_) hipHostFree(p);
        else hipFree(p);
    }
  private:
    static size_t round_up(size_t b) {
        const size_t g = b <= (1u << 20) ? 4096 : (256u << 10);
        return std::max<size_t>((b + g - 1) / g * g, g);
    }
    static size_t cap_bytes() {
        static const size_t v = [] {
            const char* e = std::getenv("CMOOP_POOL_GB");
            const double gb = e ? std::atof(e) : 96.0;
            return gb > 0 ? (size_t)(gb * (double)(1ull << 30)) : (size_t)0;
        }();
        return v;
    }
    const bool host_;
    std::mutex mu_;
    std::map<int, std::multimap<size_t, void*>> free_;
    std::map<void*, size_t> sizes_;
    size_t cached_ = 0;
};
DevicePool& pool(bool host) {
    // leaked on purpose: worker threads may outlive static destructors
    static DevicePool* dev = new DevicePool(false);
    static DevicePool* pinned = new DevicePool(true);
    return host ? *pinned : *dev;
}
}  // namespace

void* pool_alloc(size_t bytes) { return pool(false).get(bytes); }
void pool_free(void* p) { pool(false).put(p); }
void* pool_alloc_pinned(size_t bytes) { return pool(true).get(bytes); }
void pool_free_pinned(void* p) { pool(true).put(p); }

// step_launch_counts: what train_step_stateful did, over every net of the process (the population path steps from several threads)
enum { STEP_COUNT_EAGER = 0, STEP_COUNT_REPLAYS = 1, STEP_COUNT_CAPTURES = 2, STEP_COUNT_DROPS = 3 };
static std::atomic<int64_t> g_step_counts[4];

float* Net::dalloc(size_t floats) {
    void* p = pool_alloc(std::max<size_t>(floats, 4) * sizeof(float));
    allocs_.push_back(p);
    return static_cast<float*>(p);
}

Net::Net(const int32_t gene[6], const NetConfig& cfg, int T, int F, uint32_t seed, hipStream_t stream)
    : cfg_(cfg), T_(T), F_(F), seed_(seed), stream_(stream) {
    validate_gene(gene);
    CMOOP_REQUIRE(cfg.classes >= 2 && cfg.classes <= 64, "classes must be in [2, 64]");
    CMOOP_REQUIRE(cfg.batch >= 1 && cfg.batch <= 4096 && cfg.eval_batch >= 1, "bad batch size");
    CMOOP_REQUIRE(T >= 1 && F >= 1, "bad feature shape");
    std::memcpy(gene_, gene, sizeof(gene_));
    Bmax_ = std::max(cfg.batch, cfg.eval_batch);
    check_plan_ranges(gene, cfg.variant, T, F, Bmax_);   // fail at creation, not in the middle of a fit
    build_plan();
}

Net::~Net() {
    for (auto& e : ev_pool_) { hipEventDestroy(e.t.start); hipEventDestroy(e.t.stop); }
    hipStreamSynchronize(stream_);
    if (graph_exec_) hipGraphExecDestroy(graph_exec_);            // nothing of this candidate may still be running when its buffers are reused
    for (void* p : allocs_) pool_free(p);
}

NetPlan plan_net(const int32_t gene[6], const NetConfig& cfg, int T, int F) {
    validate_gene(gene);
    const int f = gene[0], k = gene[1], bn = gene[2], R = gene[3], fc = gene[4], dr = gene[5];
    CMOOP_REQUIRE(cfg.variant >= 0 && cfg.variant <= 3, "variant must be CMOOP_VARIANT_A, _B, _A_DS or _B_DS");
    const bool A = variant_is_a(cfg.variant), ds = variant_is_ds(cfg.variant);
    NetPlan plan;
    std::vector<Act>& acts = plan.acts;
    std::vector<Op>& ops = plan.ops;
    int64_t off = 0;
    int tindex = 0;

    auto new_act = [&](int H, int W, int C) {
        Act a; a.H = H; a.W = W; a.C = C;
        acts.push_back(a);
        return (int)acts.size() - 1;
    };
    new_act(T, F, 1);   // 0: the input features (never materialised: conv1 reads the resident tensor)

    auto add_conv = [&](OpKind kind, int in, int Cout, int KS, int stride, int relu, int in_is_relu, float mask_scale,
                        int accumulate) {
        Op op; op.kind = kind; op.in = in;
        const Act& ia = acts[in];
        op.KS = KS; op.stride = stride; op.Cin = ia.C; op.Cout = Cout; op.H = ia.H; op.W = ia.W; op.relu = relu;
        op.in_is_relu = in_is_relu; op.in_mask_scale = mask_scale; op.dgrad_accumulate = accumulate;
        op.w_off = off; op.tensor_index = tindex;
        op.gemm_mode = cfg.gemm_mode;
        off += (int64_t)Cout * KS * KS * ia.C;
        op.b_off = off; off += Cout;
        tindex += 2;
        op.out = new_act((ia.H + stride - 1) / stride, (ia.W + stride - 1) / stride, Cout);
        ops.push_back(op);
        return op.out;
    };
    // a k x k stride-1 conv of the block body: full, or (A_ds / B_ds) depthwise k x k (no bias, no activation; its data
    // gradient carries the x > 0 mask of the conv it replaces and never accumulates) + pointwise 1 x 1 (bias, ReLU, and
    // the "feeds a BatchNorm" role).  Canonical tensors: depthwise kernel [k][k][C_in], pointwise kernel, bias
    auto add_sepconv = [&](int in, int Cout, int KS, int relu, int in_is_relu) {
        if (!ds) return add_conv(OP_CONV, in, Cout, KS, 1, relu, in_is_relu, 1.f, 0);
        Op op; op.kind = OP_DWCONV; op.in = in;
        const Act ia = acts[in];
        op.KS = KS; op.stride = 1; op.Cin = op.Cout = ia.C; op.H = ia.H; op.W = ia.W; op.in_is_relu = in_is_relu;
        op.w_off = op.b_off = off; op.tensor_index = tindex;
        off += (int64_t)KS * KS * ia.C;
        tindex += 1;
        op.out = new_act(ia.H, ia.W, ia.C);
        ops.push_back(op);
        return add_conv(OP_CONV, op.out, Cout, 1, 1, relu, 0, 1.f, 0);
    };
    auto add_bn = [&](int in, int relu_after, int mask_in_pos) {
        if (!ops.empty() && (ops.back().kind == OP_CONV || ops.back().kind == OP_CONV1) && ops.back().out == in) ops.back().feeds_bn = 1;
        Op op; op.kind = OP_BN; op.in = in; op.relu_after = relu_after; op.mask_in_pos = mask_in_pos;
        const Act ia = acts[in];
        op.Cout = ia.C;
        op.gamma_off = off; off += ia.C;
        op.beta_off = off; off += ia.C;
        op.mm_off = off; off += ia.C;
        op.mv_off = off; off += ia.C;
        tindex += 4;
        op.out = new_act(ia.H, ia.W, ia.C);
        ops.push_back(op);
        return op.out;
    };
    auto add_pool = [&](int in, int mask_y_pos) {
        Op op; op.kind = OP_POOL; op.in = in; op.mask_y_pos = mask_y_pos;
        // CMOOP_BN_POOL_UNFUSED=1 (read per net: tests A/B the fused kernels against scale_shift + maxpool, bit for bit)
        const char* unf = std::getenv("CMOOP_BN_POOL_UNFUSED");
        const bool fuse_ok = !(unf && unf[0] == '1');
        if (fuse_ok && !ops.empty() && ops.back().kind == OP_BN && ops.back().out == in && !mask_y_pos) {
            ops.back().fuse_pool = 1;      // BN-apply (+ReLU) + pool in one pass; the BN output is never written
            op.fused_into_bn = 1;
            acts[in].virt = true;
        }
        const Act ia = acts[in];
        op.out = new_act((ia.H + 1) / 2, (ia.W + 1) / 2, ia.C);
        ops.push_back(op);
        return op.out;
    };

    int x;
    if (A) {   // nsga_penalty.py:255-265
        x = add_conv(OP_CONV1, 0, f, k, 1, !bn, 0, 1.f, 0);
        if (bn) x = add_bn(x, 1, 0);
        x = add_sepconv(x, f, k, !bn, 1);
        if (bn) x = add_bn(x, 1, 0);
        x = add_pool(x, 0);
    } else {   // sa_nsga_penalty.py:151-153 (ReLU fused into the conv, BN after it)
        x = add_conv(OP_CONV1, 0, f, k, 1, 1, 0, 1.f, 0);
        if (bn) x = add_bn(x, 0, 1);
        x = add_pool(x, !bn);
    }
    int c = f;
    for (int r = 0; r < R; ++r) {
        // the block input is a ReLU output (so consumers mask their dgrad by x > 0), except
        // topology B's first block, whose input is pool(BN(.)) or pool(relu(.)) handled in the pool
        const int in_relu = (A || r > 0) ? 1 : 0;
        const int skip = add_conv(OP_CONV, x, 2 * c, 1, 2, 0, in_relu, 1.f, 1);
        int y;
        if (A) {   // nsga_penalty.py:276-301
            y = add_sepconv(x, 2 * c, k, !bn, in_relu);
            if (bn) y = add_bn(y, 1, 0);
            y = add_sepconv(y, 2 * c, k, 0, 1);
            if (bn) y = add_bn(y, 0, 0);
            y = add_pool(y, 0);
        } else {   // sa_nsga_penalty.py:155-165
            y = add_sepconv(x, 2 * c, k, 1, in_relu);
            if (bn) y = add_bn(y, 0, 1);
            y = add_pool(y, !bn);
        }
        Op op; op.kind = OP_ADDRELU; op.in = y; op.in2 = skip;
        op.out = new_act(acts[y].H, acts[y].W, acts[y].C);
        ops.push_back(op);
        x = op.out;
        c *= 2;
    }
    {
        Op op; op.kind = OP_GAP; op.in = x;
        op.out = new_act(1, 1, acts[x].C);
        ops.push_back(op);
        x = op.out;
    }
    const float keep_scale = dropout_params(cfg.dropout).keep_scale;
    for (int i = 0; i < fc; ++i) {
        const int in_relu = i > 0;
        const float ms = (in_relu && dr) ? keep_scale : 1.f;
        x = add_conv(OP_DENSE, x, FC_LADDER[fc][i], 1, 1, 1, in_relu, ms, 0);
        if (dr) ops.back().dropout_layer = i;
    }
    x = add_conv(OP_DENSE, x, cfg.classes, 1, 1, 0, 1, dr ? keep_scale : 1.f, 0);
    ops.back().gemm_mode = GEMM_FP32;   // the classifier layer stays fp32 in every mode (as does the C_in = 1 first conv)
    plan.logits = x;
    // Activation-quantisation sites (Net::set_actquant): the materialised operand tensors of the MAC layers and of the global
    // pool, but for the input features (act 0, the resident tensor) and the logits; numbered in act order.  Every consumer of a
    // site reads the quantised tensor, and none should see the unquantised one: in all four variants a site (a block input, a
    // BatchNorm / pool / add+ReLU / depthwise / conv / dense output that feeds a conv, a dense layer or the global pool) is read
    // by OP_CONV / OP_DWCONV / OP_DENSE / OP_GAP only -- the tensors BatchNorm, max-pool and add+ReLU read (conv outputs, the
    // skip projection, the block's pooled branch) feed nothing else, so they are no sites
    for (int i = 1; i < (int)acts.size(); ++i) {
        if (i == plan.logits || acts[i].virt) continue;
        bool mac = false;
        for (const Op& op : ops)
            mac = mac || (op.in == i && (op.kind == OP_CONV || op.kind == OP_DWCONV || op.kind == OP_DENSE || op.kind == OP_GAP));
        if (mac) acts[i].site = plan.n_sites++;
    }
    for (const Op& op : ops) {   // the comment above, checked: a site has no other reader
        const bool mac = op.kind == OP_CONV || op.kind == OP_DWCONV || op.kind == OP_DENSE || op.kind == OP_GAP;
        CMOOP_REQUIRE(mac || ((op.in < 0 || acts[op.in].site < 0) && (op.in2 < 0 || acts[op.in2].site < 0)),
                      "plan: an activation-quantisation site is read by an op that is no MAC layer");
    }
    plan.n_params = off;
    CMOOP_REQUIRE(plan.n_params == param_count(gene, cfg.variant, cfg.classes), "plan / closed-form parameter count mismatch");
    return plan;
}

std::vector<KernelTensor> NetPlan::kernel_tensors() const {
    std::vector<KernelTensor> out;
    for (int i = 0; i < (int)ops.size(); ++i) {
        const Op& op = ops[i];
        const int kk = op.KS * op.KS;
        if (op.kind == OP_CONV1 || op.kind == OP_CONV || op.kind == OP_DENSE)
            out.push_back(KernelTensor{i, op.kind, op.w_off, op.Cout, kk * op.Cin, kk * op.Cin, 1});
        else if (op.kind == OP_DWCONV)
            out.push_back(KernelTensor{i, op.kind, op.w_off, op.Cin, kk, 1, op.Cin});
    }
    return out;
}

std::vector<uint8_t> NetPlan::param_kinds() const {
    std::vector<uint8_t> kinds((size_t)n_params, (uint8_t)KIND_TRAINABLE);
    for (const KernelTensor& t : kernel_tensors())
        std::fill(kinds.begin() + t.off, kinds.begin() + t.off + t.elems(), (uint8_t)KIND_KERNEL);
    for (const Op& op : ops)
        if (op.kind == OP_BN) std::fill(kinds.begin() + op.mm_off, kinds.begin() + op.mv_off + op.Cout, (uint8_t)KIND_FROZEN);
    return kinds;
}

QuantTable quant_table(const NetPlan& plan) {
    QuantTable tab;
    for (const KernelTensor& t : plan.kernel_tensors()) {
        CMOOP_REQUIRE(t.off <= QUANT_MAX_ARENA, "quant: the arena must stay below 2^31 elements (QUANT_MAX_ARENA)");
        tab.rows.push_back(QuantRow{(int32_t)t.off, t.channels, t.len, t.chan_stride, t.elem_stride, 0, 0});
    }
    quant_table_finalize(tab, plan.n_params);
    return tab;
}

std::vector<Int8Op> int8_ops(const NetPlan& plan) {
    std::vector<Int8Op> out;
    int64_t channels = 0;                              // quant_table's scale_off: the channels of the kernel tensors before this one
    for (const KernelTensor& t : plan.kernel_tensors()) {
        const Op& op = plan.ops[t.op];
        if ((op.kind == OP_CONV || op.kind == OP_DENSE) && plan.acts[op.in].site >= 0) {
            CMOOP_REQUIRE(int8_layer_ok(op.Cin, op.Cout, op.KS, op.stride), "int8: a layer is beyond the integer kernels (Cin % 16, KS, stride, 127^2 K < 2^31)");
            CMOOP_REQUIRE(op.w_off % 16 == 0, "int8: a kernel tensor's code rows are not 16-byte aligned (w_off % 16)");
            out.push_back(Int8Op{t.op, op.in, op.out, plan.acts[op.in].site, channels});
        }
        channels += t.channels;
    }
    return out;
}

std::vector<Int8DwOp> int8_dw_ops(const NetPlan& plan) {
    std::vector<Int8DwOp> out;
    int64_t channels = 0;                              // as int8_ops: quant_table's scale_off
    for (const KernelTensor& t : plan.kernel_tensors()) {
        const Op& op = plan.ops[t.op];
        if (op.kind == OP_DWCONV) {
            const int si = plan.acts[op.in].site, so = plan.acts[op.out].site;
            CMOOP_REQUIRE(si >= 0 && so >= 0, "int8 depthwise: a depthwise op reads or writes an act that is no activation-quantisation site");
            CMOOP_REQUIRE(int8_dw_layer_ok(op.Cin, op.KS), "int8 depthwise: a layer is beyond the integer kernel (C a power of two in 16..512, KS 3 or 5)");
            CMOOP_REQUIRE(op.w_off % 16 == 0, "int8 depthwise: a kernel tensor's code rows are not 16-byte aligned (w_off % 16)");
            CMOOP_REQUIRE(channels % 4 == 0, "int8 depthwise: a kernel tensor's scales are not 16-byte aligned (scale_off % 4)");
            out.push_back(Int8DwOp{t.op, op.in, op.out, si, so, channels});
        }
        channels += t.channels;
    }
    return out;
}

std::vector<Int8FusedOp> int8_fused_ops(const NetPlan& plan) {
    std::vector<Int8FusedOp> out;
    for (const Int8Op& o : int8_ops(plan)) {
        const Op& op = plan.ops[o.op];
        int bn = -1, site_act = -1;
        if (plan.acts[op.out].site >= 0) {                       // T0: the op's own output is a site
            site_act = op.out;
        } else {                                                 // T1: op -> BatchNorm (no fused pool) -> site
            int readers = 0, reader = -1;
            for (int j = 0; j < (int)plan.ops.size(); ++j)
                if (plan.ops[j].in == op.out || plan.ops[j].in2 == op.out) { ++readers; reader = j; }
            if (readers == 0 || plan.ops[reader].kind != OP_BN || plan.ops[reader].fuse_pool || plan.acts[plan.ops[reader].out].site < 0)
                continue;
            CMOOP_REQUIRE(readers == 1, "int8 fused: the pre-BatchNorm act of a fusible op has another reader");
            bn = reader;
            site_act = plan.ops[reader].out;
        }
        const int so = plan.acts[site_act].site;
        CMOOP_REQUIRE(so >= 0, "int8 fused: the act a fusible op writes is no activation-quantisation site");
        CMOOP_REQUIRE(op.Cout % 4 == 0, "int8 fused: Cout must be a multiple of 4 (a lane stores four codes as one word)");
        out.push_back(Int8FusedOp{o, bn, bn >= 0 ? plan.ops[bn].relu_after : 0, site_act, so});
    }
    return out;
}

PruneTable prune_table(const NetPlan& plan, bool skip_small) {
    PruneTable tab;
    for (const KernelTensor& t : plan.kernel_tensors()) {
        CMOOP_REQUIRE(t.off <= PRUNE_MAX_ARENA, "prune: the arena must stay below 2^31 elements (PRUNE_MAX_ARENA)");
        const bool small = t.kind == OP_CONV1 || t.kind == OP_DWCONV;   // a few hundred weights that every pixel goes through
        tab.rows.push_back(PruneRow{(int32_t)t.off, (int32_t)t.elems(), small && skip_small ? 0 : -1, 0});
    }
    prune_table_finalize(tab, plan.n_params);
    return tab;
}

size_t NetPlan::splitk_floats(int batch, int Bmax) const {
    size_t need = 0;
    for (const Op& op : ops)
        if (op.kind == OP_CONV) need = std::max(need, op.conv().splitk_need(batch, Bmax));
    return need;
}

std::string NetPlan::launch_plan(int batch, int Bmax, int B, bool train) const {
    CMOOP_REQUIRE(B >= 1 && B <= (train ? batch : Bmax), "launch plan: batch larger than the net is planned for");
    const size_t sk = splitk_floats(batch, Bmax);
    std::string out;
    auto add = [&](const std::string& v) { out += (out.empty() ? "" : ";") + v; };
    for (const Op& op : ops)
        if (op.kind == OP_CONV) add(op.conv().plan_forward(B, train && op.feeds_bn, sk, op.gemm_mode));
    if (train)
        for (auto op = ops.rbegin(); op != ops.rend(); ++op)
            if (op->kind == OP_CONV) {
                add(op->conv().plan_wgrad(B, op->gemm_mode));
                add(op->conv().plan_dgrad(B, sk, op->gemm_mode));
            }
    return out;
}

void Net::build_plan() {
    plan_ = plan_net(gene_, cfg_, T_, F_);
    splitk_ws_floats_ = plan_.splitk_floats(cfg_.batch, Bmax_);
    const std::vector<KernelTensor> tensors = plan_.kernel_tensors();

    // ---- activations ------------------------------------------------------
    for (size_t i = 1; i < acts_.size(); ++i)
        if (!acts_[i].virt) acts_[i].data = dalloc((size_t)Bmax_ * acts_[i].per_sample());
    // gradients: residual add aliases its operands' grads with its output's
    for (size_t i = 1; i < acts_.size(); ++i) {
        if (acts_[i].virt) continue;
        acts_[i].grad = dalloc((size_t)cfg_.batch * acts_[i].per_sample());
        acts_[i].own_grad = true;
    }
    for (auto& op : ops_)
        if (op.kind == OP_ADDRELU) {
            acts_[op.in].grad = acts_[op.out].grad;
            acts_[op.in2].grad = acts_[op.out].grad;
        }
    // ---- parameters / optimiser state ---------------------------------------
    params_ = weights_ = dalloc(n_params_); grads_ = dalloc(n_params_);
    adam_m_ = dalloc(n_params_); adam_v_ = dalloc(n_params_);
    CMOOP_HIP(hipMemsetAsync(grads_, 0, n_params_ * 4, stream_));
    CMOOP_HIP(hipMemsetAsync(adam_m_, 0, n_params_ * 4, stream_));
    CMOOP_HIP(hipMemsetAsync(adam_v_, 0, n_params_ * 4, stream_));
    // initial weights are generated ON THE DEVICE (bit-identical to the host / oracle twin: the counter RNG is integer
    // arithmetic and (float)(2 u24 - 2^24) * scale is one exact conversion and one correctly rounded multiply): a
    // 13.6 M-parameter candidate no longer spends ~50 ms of host hashing + an H2D copy with its stream idle
    CMOOP_HIP(hipMemsetAsync(params_, 0, n_params_ * 4, stream_));
    auto kt = tensors.begin();   // in op order, as the launches always were
    for (int oi = 0; oi < (int)ops_.size(); ++oi) {
        const Op& op = ops_[oi];
        if (op.kind == OP_BN) {
            launch_fill(params_ + op.gamma_off, 1.f, op.Cout, stream_);
            launch_fill(params_ + op.mv_off, 1.f, op.Cout, stream_);
        } else if (kt != tensors.end() && kt->op == oi) {
            // glorot_uniform: limit = sqrt(6 / (fan_in + fan_out)), fan = k*k*C  (oracle/rng.py twin); Keras' fans of a
            // depthwise kernel (k, k, C, 1): fan_in = k*k*C, fan_out = k*k
            const double kk = (double)op.KS * op.KS;
            const double fan_in = kk * op.Cin, fan_out = op.kind == OP_DWCONV ? kk : kk * op.Cout;
            const float scale = (float)(std::sqrt(6.0 / (fan_in + fan_out)) / 16777216.0);
            launch_glorot_init(params_ + kt->off, kt->elems(), rng_prefix(seed_, STREAM_INIT + (uint32_t)op.tensor_index, 0), scale, stream_);
            ++kt;
        }
    }

    // ---- per-op buffers and shared workspaces --------------------------------
    for (auto& op : ops_) {
        if (op.kind == OP_BN) op.bn_buf = dalloc(4 * (size_t)op.Cout);
        if (op.kind == OP_POOL) {
            void* p = pool_alloc((size_t)Bmax_ * acts_[op.out].per_sample());
            allocs_.push_back(p);
            op.arg = static_cast<uint8_t*>(p);
        }
        if (op.kind == OP_CONV) {   // (dense layers need no workspace: dense.hip)
            const ConvLayer L = op.conv();
            // row tables: the layer's for the largest batch, its dgrad's for the train batch; built once
            if ((op.rowtab_rows = L.table_rows(Bmax_)) > 0) {
                op.rowtab = dalloc((size_t)op.rowtab_rows * 2);
                launch_build_rowtab(L.geometry(Bmax_), op.rowtab, stream_);
            }
            if ((op.rowtab_d_rows = L.dgrad_table_rows(cfg_.batch)) > 0) {
                op.rowtab_d = dalloc((size_t)op.rowtab_d_rows * 2);
                launch_build_rowtab(L.dgrad_geom(cfg_.batch), op.rowtab_d, stream_);
            }
            // Each layer owns its slabs: they live until the optimiser launch at the end of the step sums them.
            op.slab_floats = L.slab_floats(cfg_.batch);
            op.slab_off = (int64_t)wgrad_ws_floats_;
            wgrad_ws_floats_ += (op.slab_floats + 3) / 4 * 4;
            op.wd_off = (int64_t)wd_ws_floats_;
            wd_ws_floats_ += L.flip_floats();
            // (the shared split-K workspace is sized by NetPlan::splitk_floats)
            const int64_t M = L.geometry(cfg_.batch).M();
            if (op.Cout % 4 == 0)
                red_ws_floats_ = std::max(red_ws_floats_, (size_t)colreduce_blocks(M, op.Cout) * 2 * op.Cout + 2 * op.Cout);
        }
        if (op.kind == OP_CONV1) {
            const size_t per = (size_t)op.Cout * (op.KS * op.KS + 1);
            for (int b = 1; b <= cfg_.batch; ++b) op.slab_floats = std::max(op.slab_floats, per * conv1_wgrad_blocks(b, T_, F_));
            op.slab_off = (int64_t)wgrad_ws_floats_;
            wgrad_ws_floats_ += (op.slab_floats + 3) / 4 * 4;
            red_ws_floats_ = std::max(red_ws_floats_, (size_t)colreduce_blocks((int64_t)Bmax_ * T_ * F_, op.Cout) * 2 * op.Cout + 2 * op.Cout);
        }
        if (op.kind == OP_DWCONV) {   // slice counts are not monotone in the batch: the worst train batch
            const size_t per = (size_t)op.KS * op.KS * op.Cin;
            for (int b = 1; b <= cfg_.batch; ++b)
                op.slab_floats = std::max(op.slab_floats, per * dwconv_wgrad_slices(b, op.H, op.W, op.Cin, op.KS));
            op.slab_off = (int64_t)wgrad_ws_floats_;
            wgrad_ws_floats_ += (op.slab_floats + 3) / 4 * 4;
        }
        if (op.kind == OP_BN) {
            red_ws_floats_ = std::max(red_ws_floats_, stats_partials_floats((int64_t)Bmax_ * acts_[op.in].H * acts_[op.in].W, op.Cout));
        }
    }
    wgrad_ws_ = dalloc(wgrad_ws_floats_);
    wd_ws_ = dalloc(wd_ws_floats_);
    {   // one table row per conv layer with a data gradient: refreshed by ONE flip-transpose launch per train step
        std::vector<FlipEntry> tab;
        for (const KernelTensor& t : tensors) {
            const Op& op = ops_[t.op];
            if (t.kind == OP_CONV && op.wd_off >= 0) {
                tab.push_back(FlipEntry{t.off, op.wd_off, op.Cout, op.KS, op.KS, op.Cin});
                flip_max_elems_ = std::max(flip_max_elems_, t.elems());
            }
        }
        flip_layers_ = (int)tab.size();
        if (flip_layers_) {
            flip_table_ = reinterpret_cast<FlipEntry*>(dalloc(tab.size() * sizeof(FlipEntry) / sizeof(float) + 4));
            CMOOP_HIP(hipMemcpyAsync(flip_table_, tab.data(), tab.size() * sizeof(FlipEntry), hipMemcpyHostToDevice, stream_));
            CMOOP_HIP(hipStreamSynchronize(stream_));   // tab is a local
        }
    }
    splitk_ws_ = splitk_ws_floats_ ? dalloc(splitk_ws_floats_) : nullptr;
    red_ws_ = dalloc(red_ws_floats_ + 64);
    acc_train_ = reinterpret_cast<double*>(dalloc(8));
    acc_eval_ = acc_train_ + 2;
    CMOOP_HIP(hipMemsetAsync(acc_train_, 0, 32, stream_));
    if (cfg_.profile_every > 0) {
        ev_pool_.resize(1024);
        // CMOOP_PROFILE_PAIRS=1 (set by bench.py when it runs under rocprofv3): plain event pairs
        const char* pm = std::getenv("CMOOP_PROFILE_PAIRS");
        const bool ext = !(pm && pm[0] == '1');
        static std::atomic<bool> said{false};
        if (!said.exchange(true)) std::fprintf(stderr, "[cmoop] GEMM launch timing: %s\n", ext ? "hipExtLaunchKernelGGL events" : "hipEventRecord pairs");
        for (auto& e : ev_pool_) {
            CMOOP_HIP(hipEventCreate(&e.t.start));
            CMOOP_HIP(hipEventCreate(&e.t.stop));
            e.t.ext = ext;
        }
    }
}

ConvBuffers Net::buffers_of(const Op& op) const {
    ConvBuffers b;
    b.tab = op.rowtab; b.tab_rows = op.rowtab_rows; b.tab_d = op.rowtab_d; b.tab_d_rows = op.rowtab_d_rows;
    b.slabs = wgrad_ws_ + op.slab_off; b.slab_floats = op.slab_floats; b.wd = wd_ws_ + op.wd_off;
    b.splitk = splitk_ws_; b.splitk_floats = splitk_ws_floats_; b.stats = red_ws_;
    return b;
}

void Net::get_params(float* host) {
    CMOOP_HIP(hipMemcpyAsync(host, weights_, n_params_ * 4, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}
void Net::set_params(const float* host) {
    CMOOP_HIP(hipMemcpyAsync(weights_, host, n_params_ * 4, hipMemcpyHostToDevice, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}
void Net::get_grads(float* host) {
    CMOOP_HIP(hipMemcpyAsync(host, grads_, n_params_ * 4, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}
void Net::snapshot_params() {
    if (!snap_) snap_ = dalloc(n_params_);
    CMOOP_HIP(hipMemcpyAsync(snap_, params_, n_params_ * 4, hipMemcpyDeviceToDevice, stream_));
    if (act_rec_) {   // the ranges this model was validated with travel with its weights
        CMOOP_HIP(hipMemcpyAsync(act_rec_snap_, act_rec_, (size_t)plan_.n_sites * sizeof(ActRange), hipMemcpyDeviceToDevice, stream_));
        act_ranges_ready_snap_ = act_ranges_ready_;
    }
}
void Net::restore_snapshot() {
    if (snap_) CMOOP_HIP(hipMemcpyAsync(weights_, snap_, n_params_ * 4, hipMemcpyDeviceToDevice, stream_));
    if (snap_ && act_rec_) {   // (a snapshot older than the records holds count 0 everywhere: the ranges start over)
        CMOOP_HIP(hipMemcpyAsync(act_rec_, act_rec_snap_, (size_t)plan_.n_sites * sizeof(ActRange), hipMemcpyDeviceToDevice, stream_));
        act_ranges_ready_ = act_ranges_ready_snap_;
    }
}

const GemmTiming* Net::begin(int cls, double flops) {
    hook_live_ = profiling_now_ && ev_used_ < ev_pool_.size();
    if (!hook_live_) return nullptr;
    ev_pool_[ev_used_].flops = flops;
    ev_pool_[ev_used_].cls = cls;
    return &ev_pool_[ev_used_].t;
}
void Net::end(int code, int flags) {
    if (!hook_live_) return;
    ev_pool_[ev_used_].code = code;
    ev_pool_[ev_used_].flags = flags;
    ++ev_used_;
    hook_live_ = false;
}

std::string gemm_variant_name(int cls, int code, int flags) {
    std::string v = gemm_kernel_name(cls, code);
    if (flags & GEMM_FLAG_SPLITK) v += "+sk";
    if (flags & GEMM_FLAG_BALANCED) v += "+bal";
    if (flags & GEMM_FLAG_STATS) v += "+stats";
    if (flags & GEMM_FLAG_ROWTAB) v += "+tab";
    if (flags & GEMM_FLAG_SLABS) v += "+slabs";
    return v;
}

// ---------------------------------------------------------------------------
// ConvLayer: sizes, launches and host-only launch plans of one implicit-GEMM conv layer
// dW[N][K] and db[N]: MFMA split over row slices, then a fixed-order slice sum
void ConvLayer::wgrad(const float* X, const float* dY, float* dW, float* dB, int B, const ConvBuffers& buf, int mode, hipStream_t s,
                      GemmHook* hook, AdamSeg* defer) const {
    const ConvGeom g = geometry(B);
    const int M = g.M(), N = g.Cout, K = g.K();
    int S = wgrad_slices(g);
    // never write past the slab workspace: fewer slices is always correct (each slice is a row range)
    const size_t per_slice = (size_t)N * (K + 1);
    if (S > 1 && (size_t)S * per_slice > buf.slab_floats) S = (int)std::max<size_t>(1, buf.slab_floats / per_slice);
    CMOOP_REQUIRE(S == 1 || (size_t)S * per_slice <= buf.slab_floats, "wgrad slab workspace too small");
    // slices are laid out [S][N*K + N] (kernel partials then bias partials): when dB directly follows dW
    // (the trainer's arena) a single fixed-order reduction produces both; one slice writes in place.
    const size_t NK = (size_t)N * K, stride = NK + N;
    const bool in_place = S == 1;
    float* Pk = in_place ? dW : buf.slabs;
    float* Pbias = in_place ? dB : buf.slabs + NK;
    const GemmTiming* tm = hook ? hook->begin(1, 2.0 * M * (double)N * K) : nullptr;
    int flags = 0;
    const int code = launch_igemm_wgrad(X, dY, Pk, g, S, s, tm, Pbias, in_place ? NK : stride, mode, buf.tab, buf.tab_rows, &flags);
    if (hook) hook->end(code, flags);
    if (defer) {
        CMOOP_REQUIRE(dB == dW + NK, "deferred slice sum needs the bias gradient directly after the kernel gradient");
        defer->n = (int64_t)stride;
        defer->slab = in_place ? nullptr : buf.slabs;
        defer->stride = (int64_t)stride;
        defer->S = S;
        return;
    }
    if (!in_place) {
        if (dB == dW + NK) {
            launch_reduce_slices(buf.slabs, dW, S, (int64_t)stride, s, (int64_t)stride);
        } else {
            launch_reduce_slices(buf.slabs, dW, S, (int64_t)NK, s, (int64_t)stride);
            launch_reduce_slices(buf.slabs + NK, dB, S, N, s, (int64_t)stride);
        }
    }
}

// the part of the dgrad launch's epilogue its tile / path choice depends on (`g` is the FORWARD geometry)
static GemmEpilogue dgrad_epilogue(const ConvGeom& g, int mode, int accumulate) {
    GemmEpilogue e;
    if (g.stride != 1) {
        CMOOP_REQUIRE(g.KH == 1 && g.KW == 1 && accumulate, "strided conv dgrad: only the 1x1 skip projection (accumulating)");
        e.out_stride = g.stride; e.OHf = g.H; e.OWf = g.W;
    }
    e.mode = mode;
    e.accumulate = accumulate;
    return e;
}

// dX: the same implicit-GEMM kernel on dY with flip-transposed weights.  mask != null applies the ReLU (and dropout
// scale) backward of the layer's input in the epilogue; accumulate adds into dX (second consumer of a tensor).
void ConvLayer::dgrad(const float* dY, const float* W, float* dX, int B, const float* mask, float mask_scale, int accumulate,
                      bool wd_ready, const ConvBuffers& buf, int mode, hipStream_t s, GemmHook* hook) const {
    const ConvGeom g = geometry(B);
    const int N = g.Cout;
    if (!mfma_dgrad()) {   // a classifier-shaped layer: K_dgrad = classes (10/11/35) -- tiny VALU kernel
        CMOOP_REQUIRE(g.KH == 1 && g.H == 1 && g.W == 1 && !accumulate, "non power-of-two C_out only supported for dense layers");
        launch_dense_dgrad_small(dY, W, dX, g.M(), N, g.K(), mask, mask_scale, s);
        return;
    }
    if (!wd_ready) launch_flip_transpose(W, buf.wd, N, g.KH, g.KW, g.Cin, s);
    const ConvGeom gd = dgrad_geometry(g);
    GemmEpilogue e = dgrad_epilogue(g, mode, accumulate);
    e.mask = mask;
    e.mask_scale = mask_scale;
    const GemmTiming* tm = hook ? hook->begin(0, 2.0 * gd.M() * (double)gd.Cout * gd.K()) : nullptr;
    int flags = 0;
    const int code = launch_igemm_fwd(dY, buf.wd, dX, gd, e, s, tm, buf.splitk, buf.splitk_floats, nullptr, buf.tab_d, buf.tab_d_rows, &flags);
    if (hook) hook->end(code, flags);
}

ConvGeom dgrad_geometry(const ConvGeom& g) {
    ConvGeom gd;
    gd.B = g.B; gd.H = g.OH; gd.W = g.OW; gd.Cin = g.Cout; gd.Cout = g.Cin; gd.stride = 1;
    if (g.stride == 1) {
        gd.OH = g.H; gd.OW = g.W; gd.KH = g.KH; gd.KW = g.KW;
        gd.pad_t = g.KH - 1 - g.pad_t; gd.pad_l = g.KW - 1 - g.pad_l;
    } else {
        gd.OH = g.OH; gd.OW = g.OW; gd.KH = gd.KW = 1; gd.pad_t = gd.pad_l = 0;
    }
    return gd;
}

size_t stats_partials_floats(int64_t M, int C) {
    const size_t blocks = std::max<size_t>((size_t)colreduce_blocks(M, C), (size_t)cdiv64(M, 64));
    return blocks * 2 * C + 2 * C;
}

size_t ConvLayer::slab_floats_at(int B) const {   // [slices][Cout * K kernel partials + Cout bias partials]
    const ConvGeom g = geometry(B);
    return (size_t)wgrad_slices(g) * g.Cout * (g.K() + 1);
}

size_t ConvLayer::slab_floats(int b) const {
    size_t worst = 0;
    for (int i = 1; i <= b; ++i) worst = std::max(worst, slab_floats_at(i));
    return worst;
}

size_t ConvLayer::splitk_need(int batch, int Bmax) const {
    size_t need = std::max(igemm_splitk_workspace(geometry(batch)), igemm_splitk_workspace(geometry(Bmax)));
    if (stride == 1 && mfma_dgrad()) need = std::max(need, igemm_splitk_workspace(dgrad_geom(batch)));
    return need;
}

int ConvLayer::forward(const float* X, const float* Wt, float* Y, int B, GemmEpilogue e, bool want_stats, const ConvBuffers& buf,
                       hipStream_t s, GemmHook* hook, bool* fused) const {
    const ConvGeom g = geometry(B);
    e.stats = want_stats ? buf.stats : nullptr;
    const GemmTiming* tm = hook ? hook->begin(0, 2.0 * g.M() * (double)g.Cout * g.K()) : nullptr;
    int nb = 0, flags = 0;
    const int code = launch_igemm_fwd(X, Wt, Y, g, e, s, tm, buf.splitk, buf.splitk_floats, want_stats ? &nb : nullptr, buf.tab,
                                      buf.tab_rows, &flags);
    if (hook) hook->end(code, flags);
    if (fused) *fused = nb > 0;
    if (want_stats && nb == 0) {   // split launch (raw partial sums, no fused statistics): the stand-alone reduction
        nb = colreduce_blocks(g.M(), Cout);
        launch_colstats(Y, buf.stats, g.M(), Cout, nb, s);
    }
    return nb;
}

std::string ConvLayer::plan_forward(int B, bool want_stats, size_t splitk_floats, int mode) const {
    GemmEpilogue e;
    e.mode = mode;
    int flags = 0;
    const int code = igemm_fwd_plan(geometry(B), e, splitk_floats, want_stats, has_tables(), &flags);
    return gemm_variant_name(0, code, flags);
}

std::string ConvLayer::plan_wgrad(int B, int mode) const {   // (slabs sized by slab_floats never clamp the slice count)
    const ConvGeom g = geometry(B);
    int flags = 0;
    const int code = igemm_wgrad_plan(g, wgrad_slices(g), mode, has_tables(), &flags);
    return gemm_variant_name(1, code, flags);
}

std::string ConvLayer::plan_dgrad(int B, size_t splitk_floats, int mode) const {
    CMOOP_REQUIRE(mfma_dgrad(), "launch plan: the dgrad of this layer does not run on the MFMA kernel");
    const ConvGeom g = geometry(B);
    int flags = 0;
    const int code = igemm_fwd_plan(dgrad_geometry(g), dgrad_epilogue(g, mode, stride != 1), splitk_floats, false, has_tables(), &flags);
    return gemm_variant_name(0, code, flags);
}

void Net::drain_profile() {
    if (!ev_used_) return;
    ProfileTotals& t = profile_totals();
    std::lock_guard<std::mutex> l(t.mu);
    for (size_t i = 0; i < ev_used_; ++i) {
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, ev_pool_[i].t.start, ev_pool_[i].t.stop) == hipSuccess) {
            // instantiation names as rocprofv3 prints them (codes: launch_igemm_fwd / launch_igemm_wgrad)
            const std::string name = gemm_kernel_name(ev_pool_[i].cls, ev_pool_[i].code);
            t.variants.insert(gemm_variant_name(ev_pool_[i].cls, ev_pool_[i].code, ev_pool_[i].flags));
            ProfileEntry& e = t.by_kernel[name];
            e.ms += ms;
            e.flops += ev_pool_[i].flops;
            e.launches += 1;
        }
    }
    ev_used_ = 0;
}

// ---------------------------------------------------------------------------
void Net::forward(const float* X, const BatchRows& rows, int B, bool train) {
    CMOOP_REQUIRE(B >= 1 && B <= Bmax_, "batch larger than the net was planned for");
    const float* kern = kernels_;   // what the caller's weight stage left: the source arena, the pruned or the quantised one
    for (size_t oi = 0; oi < ops_.size(); ++oi) {
        const Op& op = ops_[oi];
        const Int8Done i8 = train ? INT8_NOT_HERE : forward_int8(oi, B);   // integer inference made the op's launch(es), or the fp32 ones follow
        if (i8 == INT8_NOT_HERE) {
            switch (op.kind) {
            case OP_CONV1: {
                fused_stats_blocks_ = 0;
                const float* bin = train ? batch_in_ : nullptr;   // the batch is rows 0 .. B of the buffer step_body's augment / mixup launch wrote
                BatchRows first = bin ? BatchRows() : rows;
                if (!train) first.n_rows = 0;
                launch_conv1_fwd(bin ? bin : X, first, kern + op.w_off, params_ + op.b_off, acts_[op.out].data, B, T_, F_, op.Cout,
                                 op.KS, op.relu, stream_, (train && op.feeds_bn) ? red_ws_ : nullptr,
                                 (train && op.feeds_bn) ? &fused_stats_blocks_ : nullptr);
                break;
            }
            case OP_CONV: {
                GemmEpilogue e;
                e.mode = op.gemm_mode;
                e.bias = params_ + op.b_off;
                e.relu = op.relu;
                // train && feeds_bn: the BatchNorm batch statistics come with the conv (its epilogue, or the reduction after it)
                fused_stats_blocks_ = op.conv().forward(acts_[op.in].data, kern + op.w_off, acts_[op.out].data, B, e,
                                                        train && op.feeds_bn, buffers_of(op), stream_, this);
                break;
            }
            case OP_DWCONV:
                launch_dwconv_fwd(acts_[op.in].data, kern + op.w_off, acts_[op.out].data, B, op.H, op.W, op.Cin, op.KS, 0, nullptr, stream_);
                break;
            case OP_DENSE: {
                const bool drop = train && op.dropout_layer >= 0;
                const DropoutParams dp = dropout_params(cfg_.dropout);
                const uint32_t drop_stream = drop ? DropoutParams::stream(op.dropout_layer) : 0u;
                launch_dense_fwd(acts_[op.in].data, kern + op.w_off, params_ + op.b_off, acts_[op.out].data, B, op.Cout, op.Cin,
                                 op.relu, drop ? 1 : 0, drop ? rng_prefix(seed_, drop_stream, (uint32_t)step_) : 0u, dp.thr,
                                 dp.keep_scale, op.gemm_mode, stream_, drop ? rows.st : nullptr, seed_, drop_stream);
                break;
            }
            case OP_BN: {
                const Act& ia = acts_[op.in];
                const int64_t M = (int64_t)B * ia.H * ia.W;
                const int C = op.Cout;
                float *mean = op.bn_buf, *invstd = mean + C, *scale = invstd + C, *shift = scale + C;
                if (train) {
                    int nb = fused_stats_blocks_;              // partials the producing conv left, if any
                    fused_stats_blocks_ = 0;
                    if (nb == 0) {                             // first conv on the VALU kernel
                        nb = colreduce_blocks(M, C);
                        launch_colstats(ia.data, red_ws_, M, C, nb, stream_);
                    }
                    launch_bn_finalize(red_ws_, nb, M, C, params_ + op.gamma_off, params_ + op.beta_off, params_ + op.mm_off,
                                       params_ + op.mv_off, mean, invstd, scale, shift, (float)cfg_.bn_eps, (float)cfg_.bn_momentum,
                                       (float)(1.0 - cfg_.bn_momentum), stream_);
                } else {
                    launch_bn_eval_prepare(params_ + op.gamma_off, params_ + op.beta_off, params_ + op.mm_off,
                                           params_ + op.mv_off, scale, shift, C, (float)cfg_.bn_eps, stream_);
                }
                if (op.fuse_pool) {
                    const Op& pool = ops_[oi + 1];
                    launch_bn_pool_fwd(ia.data, acts_[pool.out].data, pool.arg, scale, shift, B, ia.H, ia.W, C, op.relu_after, stream_);
                } else {
                    launch_scale_shift(ia.data, acts_[op.out].data, scale, shift, M, C, op.relu_after, stream_);
                }
                break;
            }
            case OP_POOL: {
                if (op.fused_into_bn) break;
                const Act& ia = acts_[op.in];
                launch_maxpool_fwd(ia.data, acts_[op.out].data, op.arg, B, ia.H, ia.W, ia.C, stream_);
                break;
            }
            case OP_ADDRELU:
                launch_add_relu(acts_[op.in].data, acts_[op.in2].data, acts_[op.out].data,
                                (int64_t)B * acts_[op.out].per_sample(), stream_);
                break;
            case OP_GAP: {
                const Act& ia = acts_[op.in];
                launch_gap_fwd(ia.data, acts_[op.out].data, B, ia.H * ia.W, ia.C, stream_);
                break;
            }
            }
        }
        if (actq_on_ && i8 != INT8_WROTE_SITE) {   // the act this op's launches just wrote: a fused BatchNorm + pool writes the pool's output
            const int written = (op.kind == OP_BN && op.fuse_pool) ? ops_[oi + 1].out : (op.kind == OP_POOL && op.fused_into_bn) ? -1 : op.out;
            if (written >= 0 && acts_[written].site >= 0) quantise_site(written, B, train);
        }
    }
}

Net::Int8Done Net::forward_int8(size_t oi, int B) {
    if (!int8_.on) return INT8_NOT_HERE;
    const Int8Entry& t = int8_tab_[oi];
    const Op& op = ops_[oi];
    switch (t.role) {
    case I8_NONE:
        break;
    case I8_FUSED_BN:      // the producer's requantising epilogue applied it and wrote its site
        if (int8_.fused) return INT8_WROTE_SITE;
        break;
    case I8_DEPTHWISE:     // codes in, the output site's quantised tensor and codes out
        if (int8_.depthwise) {
            const Act &ia = acts_[op.in], &oa = acts_[op.out];
            launch_dwconv_i8_fwd(site_codes_[ia.site], w_codes_ + op.w_off, 0.f, act_rec_ + ia.site, actq_cfg_.bits, w_scales_ + t.scale_off,
                                 act_rec_ + oa.site, actq_cfg_.bits, oa.data, site_codes_[oa.site], B, op.H, op.W, op.Cin, op.KS, stream_);
            return INT8_WROTE_SITE;
        }
        break;
    case I8_MATRIX:
    case I8_FUSED: {       // the input site's codes against the staged weight codes
        const Act& ia = acts_[op.in];
        const I8Layer L = op.kind == OP_CONV ? I8Layer{true, B, op.H, op.W, op.Cin, op.Cout, op.KS, op.stride} : I8Layer::dense(B, op.Cout, op.Cin);
        const bool fused = t.role == I8_FUSED && int8_.fused;
        if (op.kind == OP_CONV) fused_stats_blocks_ = 0;   // as the fp32 conv launch leaves it in an inference pass
        I8Requant rq{};
        float* y = acts_[op.out].data;
        if (fused) {       // the requantising epilogue: the site's tensor and codes, one launch
            const Act& sa = acts_[t.site_act];
            rq.rec_out = act_rec_ + sa.site;
            rq.out_bits = actq_cfg_.bits;
            rq.codes = site_codes_[sa.site];
            y = sa.data;
            if (t.bn >= 0) {   // the eval BatchNorm vectors of the BN the op applies, prepared ahead of it
                const Op& bn = ops_[t.bn];
                const int C = bn.Cout;
                float *scale = bn.bn_buf + 2 * C, *shift = scale + C;
                launch_bn_eval_prepare(params_ + bn.gamma_off, params_ + bn.beta_off, params_ + bn.mm_off, params_ + bn.mv_off, scale, shift, C,
                                       (float)cfg_.bn_eps, stream_);
                rq.bn_scale = scale; rq.bn_shift = shift; rq.relu_after = bn.relu_after;
            }
        }
        launch_i8_fwd(L, site_codes_[ia.site], w_codes_ + op.w_off, 0.f, act_rec_ + ia.site, actq_cfg_.bits, w_scales_ + t.scale_off,
                      params_ + op.b_off, y, op.relu, fused ? &rq : nullptr, stream_);
        return fused ? INT8_WROTE_SITE : INT8_WROTE_OUT;
    }
    }
    return INT8_NOT_HERE;
}

void Net::quantise_site(int act, int B, bool train) {
    const Act& a = acts_[act];
    const EmaPair m = actquant_rates(actq_cfg_.momentum);
    // train: batch mode over the B rows of this step, and the site's record advances; inference: the tracked range
    // integer inference: the codes go to the site's int8 buffer as well (the fp32 tensor stays: OP_GAP / OP_DWCONV read it)
    launch_fake_quant_act(a.data, (int64_t)B * (int64_t)a.per_sample(), actq_cfg_.bits, !train, act_partials_, act_rec_ + a.site, m.mf, m.omf,
                          stream_, (!train && int8_.on) ? site_codes_[a.site] : nullptr);
}

void Net::require_act_ranges() const {
    CMOOP_REQUIRE(!actq_on_ || act_ranges_ready_,
                  "actquant: inference needs tracked ranges -- run a train step with the option on or load them (set_act_ranges) first");
}

void Net::backward(const float* X, const BatchRows& rows, int B) {
    slab_segs_.clear();
    const float* kern = kernels_;   // as forward: the gradients formed with it go unchanged to the latent weights (straight-through)
    // dgrad operands: flip-transposed copies of every conv kernel, one launch for the whole net
    launch_flip_transpose_all(kern, wd_ws_, flip_table_, flip_layers_, flip_max_elems_, stream_);
    for (int oi = (int)ops_.size() - 1; oi >= 0; --oi) {
        const Op& op = ops_[oi];
        switch (op.kind) {
        case OP_DENSE: {
            const float* dY = acts_[op.out].grad;
            Act& ia = acts_[op.in];
            // CMOOP_DENSE_UNFUSED=1 (read per step, like CMOOP_ADAM_UNFUSED): the two launches of round 2 instead of the merged one
            const char* du = std::getenv("CMOOP_DENSE_UNFUSED");
            const bool unfused = du && du[0] == '1';
            if (!unfused) {
                launch_dense_bwd(ia.data, dY, kern + op.w_off, grads_ + op.w_off, grads_ + op.b_off, ia.grad, B, op.Cout, op.Cin,
                                 op.in_is_relu ? ia.data : nullptr, op.in_mask_scale, op.gemm_mode, stream_);
                break;
            }
            launch_dense_wgrad(ia.data, dY, grads_ + op.w_off, grads_ + op.b_off, B, op.Cout, op.Cin, op.gemm_mode, stream_);
            launch_dense_dgrad(dY, kern + op.w_off, ia.grad, B, op.Cout, op.Cin, op.in_is_relu ? ia.data : nullptr,
                               op.in_mask_scale, op.gemm_mode, stream_);
            break;
        }
        case OP_CONV: {
            const ConvLayer L = op.conv();
            const ConvBuffers buf = buffers_of(op);
            const float* dY = acts_[op.out].grad;
            Act& ia = acts_[op.in];
            // (measured, not adopted: wgrad on a low-priority side stream forked per layer and joined before Adam -- off the
            // dgrad critical path -- ran 35 % SLOWER, 65 vs 100 TFLOP/s whole-job: the cross-stream event waits cost more
            // than the overlap wins)
            AdamSeg sg;
            sg.off = op.w_off;
            L.wgrad(ia.data, dY, grads_ + op.w_off, grads_ + op.b_off, B, buf, op.gemm_mode, stream_, this, &sg);
            if (sg.slab) slab_segs_.push_back(sg);
            L.dgrad(dY, kern + op.w_off, ia.grad, B, op.in_is_relu ? ia.data : nullptr, op.in_mask_scale, op.dgrad_accumulate,
                    true, buf, op.gemm_mode, stream_, this);
            break;
        }
        case OP_DWCONV: {
            const float* dY = acts_[op.out].grad;
            Act& ia = acts_[op.in];
            launch_dwconv_wgrad(ia.data, dY, wgrad_ws_ + op.slab_off, B, op.H, op.W, op.Cin, op.KS, stream_);
            AdamSeg sg;
            sg.off = op.w_off;
            sg.n = sg.stride = (int64_t)op.KS * op.KS * op.Cin;
            sg.slab = wgrad_ws_ + op.slab_off;
            sg.S = dwconv_wgrad_slices(B, op.H, op.W, op.Cin, op.KS);
            CMOOP_REQUIRE((size_t)sg.S * sg.n <= op.slab_floats, "depthwise slab region");
            slab_segs_.push_back(sg);
            launch_dwconv_fwd(dY, kern + op.w_off, ia.grad, B, op.H, op.W, op.Cin, op.KS, 1, op.in_is_relu ? ia.data : nullptr, stream_);
            break;
        }
        case OP_BN: {
            const Act& ia = acts_[op.in];
            const int64_t M = (int64_t)B * ia.H * ia.W;
            const int C = op.Cout;
            float *mean = op.bn_buf, *invstd = mean + C;
            const int nb = colreduce_blocks(M, C);
            if (op.fuse_pool) {   // the pool's backward is folded in: dY is scattered from the pooled gradient on the fly
                const Op& pool = ops_[oi + 1];
                launch_bn_pool_bwd_reduce(acts_[pool.out].grad, pool.arg, ia.data, mean, invstd, red_ws_, B, ia.H, ia.W, C, nb, stream_);
                launch_bn_pool_bwd_apply(acts_[pool.out].grad, pool.arg, ia.data, mean, invstd, params_ + op.gamma_off, red_ws_, nb,
                                         ia.grad, grads_ + op.gamma_off, grads_ + op.beta_off, B, ia.H, ia.W, C, op.mask_in_pos, stream_);
                break;
            }
            launch_bn_bwd_reduce(acts_[op.out].grad, ia.data, mean, invstd, red_ws_, M, C, nb, stream_);
            launch_bn_bwd_apply(acts_[op.out].grad, ia.data, mean, invstd, params_ + op.gamma_off, red_ws_, nb, ia.grad,
                                grads_ + op.gamma_off, grads_ + op.beta_off, M, C, op.mask_in_pos, stream_);
            break;
        }
        case OP_POOL: {
            if (op.fused_into_bn) break;
            const Act& ia = acts_[op.in];
            launch_maxpool_bwd(acts_[op.out].grad, op.arg, acts_[op.out].data, ia.grad, B, ia.H, ia.W, ia.C, op.mask_y_pos,
                               stream_);
            break;
        }
        case OP_ADDRELU:
            break;   // operands alias the output gradient (consumers already applied the ReLU mask)
        case OP_GAP: {
            const Act& ia = acts_[op.in];
            launch_gap_bwd(acts_[op.out].grad, ia.data, ia.grad, B, ia.H * ia.W, ia.C, stream_);
            break;
        }
        case OP_CONV1: {
            launch_conv1_wgrad(batch_in_ ? batch_in_ : X, batch_in_ ? BatchRows() : rows, acts_[op.out].grad, wgrad_ws_ + op.slab_off, B,
                               T_, F_, op.Cout, op.KS, stream_);
            AdamSeg sg;
            sg.off = op.w_off;
            sg.n = sg.stride = (int64_t)op.Cout * (op.KS * op.KS + 1);
            sg.slab = wgrad_ws_ + op.slab_off;
            sg.S = conv1_wgrad_blocks(B, T_, F_);
            CMOOP_REQUIRE((size_t)sg.S * sg.n <= op.slab_floats && op.b_off == op.w_off + (int64_t)op.Cout * op.KS * op.KS,
                          "first-layer slab region");
            slab_segs_.push_back(sg);
            break;
        }
        }
    }
}

const float* Net::stage_kernels(double sparsity, float* wp, uint32_t* zeros, float* wq, int8_t* codes, float* scales) {
    const float* src = params_;
    if (prune_on_) {
        launch_prune_weights(src, wp, zeros, ptab_, ptab_dev_, prune_ws_, sparsity, stream_);
        src = wp;
    }
    if (quant_on_ && wq) {
        launch_quantize_weights(src, wq, codes, scales, qtab_, qtab_dev_, quant_cfg_.bits, stream_);
        src = wq;
    }
    return src;
}

void Net::require_step_allowed(bool gather) const {
    CMOOP_REQUIRE(params_ == weights_, "train step while inference reads the average: use_average(false) first");
    // before anything is enqueued: a teacher table of another length than the split the step gathers from is refused whole
    CMOOP_REQUIRE(!gather || !distill_on_ || gather_rows_ == 0 || gather_rows_ == kd_rows_, "distill: the teacher table has " +
                  std::to_string(kd_rows_) + " rows, the training split " + std::to_string(gather_rows_));
}

template <class Loss> void Net::step_body(const float* X, const BatchRows& rows, int B, bool gather, Loss&& loss) {
    require_step_allowed(gather);
    refresh_kernels(prune_sparsity_at(prune_cfg_, iterations_));   // the step's first launches, on the latent weights of this moment
    batch_in_ = nullptr;
    if (gather) {
        // augmentation on: the batch's rows are gathered and augmented into aug_buf_ first (rows.st != null: the kernel reads
        // the batch position and the step from the device state, so a replayed graph draws for the step it replays)
        if (aug_on_) launch_augment_gather(X, rows, aug_buf_, B, T_, F_, aug_, seed_, (uint32_t)step_, stream_);
        // mixup on: the (augmented) rows are blended into mix_buf_ next; each row keeps its own batch position's augmentation
        // (from the augment buffer the launch takes only the step from rows.st: the buffer always starts at its row 0)
        if (mix_on_)
            launch_mixup_gather(aug_on_ ? aug_buf_ : X, rows, aug_on_ ? 1 : 0, mix_buf_, B, T_, F_, mixp_, seed_, (uint32_t)step_, stream_);
        batch_in_ = mix_on_ ? mix_buf_ : (aug_on_ ? aug_buf_ : nullptr);
    }
    forward(X, rows, B, true);
    if (actq_on_) act_ranges_ready_ = true;   // every site's record has seen a step
    loss();
    backward(X, rows, B);
    optimiser_step(B, rows.st);
}

void Net::gathered_step(const float* X, const int32_t* y, const BatchRows& rows, int B) {
    step_body(X, rows, B, true, [&] { launch_train_loss(y, rows, B); });
}

void Net::launch_train_loss(const int32_t* y, const BatchRows& rows, int B) {
    float *z = acts_[logits_].data, *dz = acts_[logits_].grad;
    if (!distill_on_ && !loss_on_) {
        launch_softmax_ce(z, y, rows, B, cfg_.classes, dz, acc_train_, nullptr, stream_);
        return;
    }
    // t / w / primary as the soft-target loss builds them (a default loss: one-hot, unit weight, the label)
    launch_soft_targets(y, rows, B, cfg_.classes, mixp_, tgtp_, seed_, (uint32_t)step_, tgt_t_, tgt_w_, tgt_primary_, stream_);
    if (!distill_on_) {
        launch_softmax_ce_soft(z, tgt_t_, tgt_w_, tgt_primary_, B, cfg_.classes, dz, acc_train_, nullptr, stream_);
        return;
    }
    // the teacher rows of the same batch positions under the same mixup draws, always clamped into the teacher's own table
    BatchRows teacher = rows;
    teacher.n_rows = kd_rows_;
    launch_teacher_targets(kd_zt_, teacher, B, cfg_.classes, kdp_.T, mixp_, seed_, (uint32_t)step_, kd_q_, stream_);
    launch_softmax_ce_distill(z, tgt_t_, tgt_w_, tgt_primary_, kd_q_, kdp_, B, cfg_.classes, dz, acc_train_, nullptr, stream_);
}

void Net::optimiser_step(int B, const StepState* st) {
    const double b1 = cfg_.beta1, b2 = cfg_.beta2;
    const OptimRates rates = optim_rates(optim_, cfg_.lr, b1, b2, iterations_);
    const float alpha = rates.alpha_f32;
    // ONE launch finishes the weight gradients (fixed-order sum of every layer's row-slice slabs) and applies Adam to the
    // whole arena: the per-layer reduce_slices launches of round 1 are gone from the step
    std::sort(slab_segs_.begin(), slab_segs_.end(), [](const AdamSeg& a, const AdamSeg& b) { return a.off < b.off; });
    AdamSegTable tab;
    int64_t pos = 0;
    auto push = [&](const AdamSeg& sg) {
        CMOOP_REQUIRE(tab.count < ADAM_MAX_SEGS, "too many optimiser segments");
        tab.seg[tab.count++] = sg;
    };
    for (const AdamSeg& sg : slab_segs_) {
        CMOOP_REQUIRE(sg.off >= pos && sg.off + sg.n <= n_params_, "slab segment outside the arena");
        if (sg.off > pos) { AdamSeg pl; pl.off = pos; pl.n = sg.off - pos; push(pl); }
        push(sg);
        pos = sg.off + sg.n;
    }
    if (pos < n_params_) { AdamSeg pl; pl.off = pos; pl.n = n_params_ - pos; push(pl); }
    if (optim_finish_) {   // a global norm needs every finished gradient before any weight moves: finish, scale, update
        adam_segments_finalize(tab);
        CMOOP_REQUIRE(tab.blocks <= optim_partials_cap_, "optimiser partial buffer too small");
        launch_grad_finish(grads_, tab, kinds_dev_, optim_partials_, stream_);
        launch_clip_scale(optim_partials_, tab.blocks, optim_.global_clipnorm, optim_rec_, stream_);
        AdamwArgs a;
        a.alpha = alpha; a.lr = rates.lr_f32; a.c1 = (float)(1.0 - b1); a.c2 = (float)(1.0 - b2); a.eps = (float)cfg_.adam_eps;
        a.weight_decay = (float)optim_.weight_decay; a.clipvalue = (float)optim_.clipvalue; a.decay_all = optim_.decay_mask;
        launch_adamw(params_, grads_, adam_m_, adam_v_, kinds_dev_, n_params_, optim_rec_, a, stream_, st, alpha_tab_, lr_tab_);
    } else if (getenv("CMOOP_ADAM_UNFUSED") != nullptr) {   // A/B knob (read per step: tests flip it): round-1 launch sequence
        for (const AdamSeg& sg : slab_segs_) launch_reduce_slices(sg.slab, grads_ + sg.off, sg.S, sg.n, stream_, sg.stride);
        launch_adam(params_, grads_, adam_m_, adam_v_, n_params_, alpha, (float)(1.0 - b1), (float)(1.0 - b2),
                    (float)cfg_.adam_eps, stream_, st, alpha_tab_);
    } else {
        adam_segments_finalize(tab);
        launch_adam_segments(params_, grads_, adam_m_, adam_v_, tab, alpha, (float)(1.0 - b1), (float)(1.0 - b2),
                             (float)cfg_.adam_eps, stream_, st, alpha_tab_);
    }
    optim_last_path_ = optim_finish_ ? 1 : 0;
    if (ema_on_) {   // the average follows the updated weights, whichever of the three paths moved them; it reads st->iter before the advance
        const EmaRates er = ema_rates(ema_cfg_, iterations_);
        launch_ema(ema_, weights_, kinds_dev_, n_params_, er.mf, er.omf, stream_, st, ema_tab_);
    }
    if (st) launch_step_advance(st_dev_, B, stream_);
}

// profiling_now_ for the length of one step: false again however the step ends, a throw included
struct ProfilingScope {
    bool& flag;
    ProfilingScope(bool& f, bool on) : flag(f) { flag = on; }
    ~ProfilingScope() { flag = false; }
};

template <class Body> void Net::counted_step(Body&& body) {
    ProfilingScope prof(profiling_now_, cfg_.profile_every > 0 && (step_ % cfg_.profile_every) == 0);
    body();
    ++iterations_;
    ++step_;
}

void Net::train_step(const float* X, const int32_t* y, const int32_t* idx, int64_t row0, int B) {
    CMOOP_REQUIRE(B >= 1 && B <= cfg_.batch, "train batch larger than configured");
    counted_step([&] { gathered_step(X, y, BatchRows{idx, row0, gather_rows_, nullptr}, B); });
}

// the explicit-targets steps.  BatchRows(): x_rows holds exactly the B rows of the step, no resident tensor to clamp into
void Net::train_step_targets(const float* x_rows, const float* t, const float* w, const int32_t* primary, int B) {
    CMOOP_REQUIRE(B >= 1 && B <= cfg_.batch, "train batch larger than configured");
    CMOOP_REQUIRE(x_rows && t, "train_step_targets: NULL rows or targets");
    Act& z = acts_[logits_];
    counted_step([&] {
        step_body(x_rows, BatchRows(), B, false,
                  [&] { launch_softmax_ce_soft(z.data, t, w, primary, B, cfg_.classes, z.grad, acc_train_, nullptr, stream_); });
    });
}

void Net::train_step_distill_targets(const float* x_rows, const float* t, const float* w, const int32_t* primary, const float* q,
                                     double alpha, double temperature, int B) {
    CMOOP_REQUIRE(B >= 1 && B <= cfg_.batch, "train batch larger than configured");
    CMOOP_REQUIRE(x_rows && t && q, "train_step_distill_targets: NULL rows, targets or teacher rows");
    DistillCfg dc;
    dc.alpha = alpha; dc.temperature = temperature;
    distill_check(dc, cfg_.classes, 0);
    const DistillParams dp = distill_params(dc);
    Act& z = acts_[logits_];
    counted_step([&] {
        step_body(x_rows, BatchRows(), B, false,
                  [&] { launch_softmax_ce_distill(z.data, t, w, primary, q, dp, B, cfg_.classes, z.grad, acc_train_, nullptr, stream_); });
    });
}

void Net::begin_fit(int64_t total_steps) {
    // total_steps counts from optimizer.iterations == 0; a net that has already trained (session API: state loaded with
    // set_state, or earlier epochs) continues from its own counters
    if (alpha_tab_ || graph_exec_) {
        // re-entered (a second fit, or run_epoch past the budget): a kept capture would go on reading the previous, shorter
        // table.  It is dropped, and once nothing queued reads them the previous tables go back to the pool: a net holds one set
        CMOOP_HIP(hipStreamSynchronize(stream_));
        option_changed(false);
        dfree(alpha_tab_); dfree(lr_tab_); dfree(ema_tab_);
        alpha_tab_ = nullptr; lr_tab_ = nullptr; ema_tab_ = nullptr;
        alpha_tab_n_ = 0;
    }
    if (total_steps < 1 || total_steps > (1ll << 24)) { graph_ok_ = false; st_dev_ = nullptr; return; }   // explicit-argument steps beyond 16 M iterations
    alpha_tab_ = dalloc(total_steps);
    alpha_tab_n_ = total_steps;
    if (!st_dev_) st_dev_ = reinterpret_cast<StepState*>(dalloc(8));
    upload_rate_tables();
    upload_step_state();
    CMOOP_HIP(hipStreamSynchronize(stream_));     // the state is there before a step reads it
    // hipGraph replay of the captured step is OPT-IN (CMOOP_GRAPH=1).  Measured: a lone 16-filter candidate runs 2 591
    // steps/s replayed vs 2 625 launched eagerly (its stream is kept busy either way: ~50 kernels of ~8 us per step,
    // the host launches faster than that), and the pop-40 bench is 1.5 % slower replayed (2 089 vs 2 121 evals/h).
    static const bool use_graph = [] { const char* v = std::getenv("CMOOP_GRAPH"); return v && v[0] == '1'; }();
    if (!use_graph || optim_finish_ || ema_on_ || quant_on_ || prune_on_ || actq_on_) graph_ok_ = false;
}

// the per-iteration rates of the device-state steps, from the one host function the explicit-argument steps use
void Net::upload_rate_tables() {
    if (!alpha_tab_ || alpha_tab_n_ < 1) return;
    if (optim_finish_ && !lr_tab_) lr_tab_ = dalloc(alpha_tab_n_);
    std::vector<float> alpha(alpha_tab_n_), lr(optim_finish_ ? alpha_tab_n_ : 0);
    for (int64_t i = 0; i < alpha_tab_n_; ++i) {
        const OptimRates r = optim_rates(optim_, cfg_.lr, cfg_.beta1, cfg_.beta2, i);
        alpha[i] = r.alpha_f32;
        if (optim_finish_) lr[i] = r.lr_f32;
    }
    CMOOP_HIP(hipMemcpyAsync(alpha_tab_, alpha.data(), alpha_tab_n_ * 4, hipMemcpyHostToDevice, stream_));
    if (optim_finish_) CMOOP_HIP(hipMemcpyAsync(lr_tab_, lr.data(), alpha_tab_n_ * 4, hipMemcpyHostToDevice, stream_));
    std::vector<EmaPair> ema(ema_on_ ? alpha_tab_n_ : 0);
    if (ema_on_) {   // the same iterations, indexed by the same st->iter
        if (!ema_tab_) ema_tab_ = reinterpret_cast<EmaPair*>(dalloc(2 * alpha_tab_n_));
        for (int64_t i = 0; i < alpha_tab_n_; ++i) {
            const EmaRates r = ema_rates(ema_cfg_, i);
            ema[i] = EmaPair{r.mf, r.omf};
        }
        CMOOP_HIP(hipMemcpyAsync(ema_tab_, ema.data(), alpha_tab_n_ * sizeof(EmaPair), hipMemcpyHostToDevice, stream_));
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));     // the tables are locals
}

void Net::option_changed(bool breaks_graph) {
    if (breaks_graph) graph_ok_ = false;          // nothing is promised under CMOOP_GRAPH=1
    if (graph_exec_) {
        hipGraphExecDestroy(graph_exec_);
        graph_exec_ = nullptr;
        g_step_counts[STEP_COUNT_DROPS].fetch_add(1, std::memory_order_relaxed);
    }
    graph_key_ = StepCaptureKey();
}

void step_launch_counts(int64_t out[4]) {
    for (int i = 0; i < 4; ++i) out[i] = g_step_counts[i].load(std::memory_order_relaxed);
}

void Net::dfree(void* p) {
    if (!p) return;
    auto it = std::find(allocs_.begin(), allocs_.end(), p);
    CMOOP_REQUIRE(it != allocs_.end(), "dfree: not a buffer of this net");
    allocs_.erase(it);
    pool_free(p);
}

// THE list of what a captured step depends on beyond the net's own buffers and options.  The net's buffers (arenas, acts,
// workspaces, st_dev_, the option buffers) are allocated once and live as long as the net; every option a launch reads
// (augment, loss, distill, optimiser, EMA, quantisation, pruning, the loaded state) is changed only by a setter, and every
// setter ends in option_changed, which drops the capture.  What is left is what callers hand in per call and what
// begin_fit / run_epoch replace:
//   X, y          the resident training tensors: by value in the gather, first-layer, loss and wgrad launches
//   idx           the epoch's permutation buffer (null: shuffle off): a fit's pooled buffer or run_epoch's own
//   gather_rows   gather_rows_, the clamp of every gather launch (set_gather_rows does not drop the capture: the key does)
//   alpha_tab     the step-size table the Adam launch indexes with st->iter; a re-entered begin_fit replaces it
//   kd_zt/kd_rows the caller's teacher table and its clamp (set_distill drops the capture too)
//   env_knobs     CMOOP_ADAM_UNFUSED and CMOOP_DENSE_UNFUSED, which choose launches per step and which tests flip
// A launch argument that can change without passing through here or through option_changed is a bug in this list.
static int step_env_knobs() {
    const char* du = std::getenv("CMOOP_DENSE_UNFUSED");
    return (std::getenv("CMOOP_ADAM_UNFUSED") != nullptr ? 1 : 0) | (du && du[0] == '1' ? 2 : 0);
}
StepCaptureKey Net::capture_key(const float* X, const int32_t* y, const int32_t* idx) const {
    StepCaptureKey k;
    k.X = X; k.y = y; k.idx = idx;
    k.gather_rows = gather_rows_;
    k.alpha_tab = alpha_tab_;
    k.kd_zt = kd_zt_; k.kd_rows = kd_rows_;
    k.env_knobs = step_env_knobs();
    return k;
}

void Net::upload_step_state() {
    if (!st_dev_) return;
    st_up_ = StepState{0, (unsigned)step_, (unsigned)iterations_};
    CMOOP_HIP(hipMemcpyAsync(st_dev_, &st_up_, sizeof(StepState), hipMemcpyHostToDevice, stream_));
}

void Net::ensure_target_buffers() {
    if (tgt_t_) return;
    tgt_t_ = dalloc((size_t)cfg_.batch * cfg_.classes);
    tgt_w_ = dalloc((size_t)cfg_.batch);
    tgt_primary_ = reinterpret_cast<int32_t*>(dalloc((size_t)cfg_.batch));
}

void Net::set_options(const TrainOptions& o) {
    if (o.aug && augment_enabled(*o.aug)) set_augment(o.aug);
    if (o.loss && loss_enabled(*o.loss)) set_loss(o.loss);
    if (o.distill && distill_enabled(*o.distill)) set_distill(o.distill);
    if (o.optim && optim_enabled(*o.optim)) set_optim(o.optim);
    if (o.ema && ema_enabled(*o.ema)) set_ema(o.ema);
    if (o.opoint && opoint_enabled(*o.opoint)) set_opoint(o.opoint);
    if (o.quant && quant_enabled(*o.quant)) set_quant(o.quant);
    if (o.prune && prune_enabled(*o.prune)) set_prune(o.prune);
    if (o.actq && actquant_enabled(*o.actq)) set_actquant(o.actq);
}

void Net::set_opoint(const OpointCfg* op) {
    if (op) opoint_check(*op);
    opoint_cfg_ = op && opoint_enabled(*op) ? *op : OpointCfg();   // read by fit_and_read_out alone: no step changes, the graph stays
}

void Net::store_opoint(const OpointClass* classes, const double summary[4]) {
    last_op_classes_.clear();
    if (!classes) return;
    last_op_classes_.assign(classes, classes + cfg_.classes);
    std::memcpy(last_op_summary_, summary, sizeof(last_op_summary_));
}

void Net::last_opoint(OpointClass* classes, double summary[4]) const {
    CMOOP_REQUIRE(!last_op_classes_.empty(), "last_opoint: the last fit ran without the operating-point read-out (set_opoint with recall > 0 first)");
    if (classes) std::memcpy(classes, last_op_classes_.data(), last_op_classes_.size() * sizeof(OpointClass));
    if (summary) std::memcpy(summary, last_op_summary_, sizeof(last_op_summary_));
}

void Net::ensure_kinds() {
    if (kinds_dev_) return;
    const std::vector<uint8_t> kinds = plan_.param_kinds();
    kinds_dev_ = reinterpret_cast<uint8_t*>(dalloc((size_t)(n_params_ + 3) / 4));
    CMOOP_HIP(hipMemcpyAsync(kinds_dev_, kinds.data(), (size_t)n_params_, hipMemcpyHostToDevice, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));     // kinds is a local
}

void Net::set_optim(const OptimCfg* optim) {
    if (optim) optim_check(*optim);
    const OptimCfg c = optim && optim_enabled(*optim) ? *optim : OptimCfg();
    const bool finish = optim_finish_path(c);
    if (finish) ensure_kinds();
    if (finish && !optim_rec_) {
        // a slab segment takes a workgroup per 64 elements at the most, a plain one per 1024, each of the segments rounds up
        optim_partials_cap_ = n_params_ / 64 + ADAM_MAX_SEGS + 1;
        optim_partials_ = dalloc((size_t)optim_partials_cap_);
        optim_rec_ = reinterpret_cast<OptimRecord*>(dalloc(sizeof(OptimRecord) / 4));
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));     // nothing of the old options is still running
    optim_ = c;
    optim_finish_ = finish;
    upload_rate_tables();                         // takes effect from the next step
    option_changed(finish);
}

void Net::set_ema(const EmaCfg* ema) {
    if (ema) ema_check(*ema);
    const bool on = ema != nullptr && ema_enabled(*ema);
    if (on) {
        ensure_kinds();
        if (!ema_) {   // first use: the average starts as the parameter arena of this moment, moving statistics included
            ema_ = dalloc(n_params_);
            CMOOP_HIP(hipMemcpyAsync(ema_, weights_, n_params_ * 4, hipMemcpyDeviceToDevice, stream_));
        }
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));
    ema_cfg_ = on ? *ema : EmaCfg();
    ema_on_ = on;
    if (on) upload_rate_tables();                 // a fit under way: its table, from the next step
    option_changed(on);
}

void Net::use_average(bool on) {
    CMOOP_REQUIRE(ema_ != nullptr, "use_average: the net has no average (set_ema with momentum > 0 first)");
    params_ = on ? ema_ : weights_;
}

void Net::get_average(float* host) {
    CMOOP_REQUIRE(ema_ != nullptr, "get_average: the net has no average (set_ema with momentum > 0 first)");
    CMOOP_REQUIRE(host != nullptr, "get_average: NULL buffer");
    CMOOP_HIP(hipMemcpyAsync(host, ema_, n_params_ * 4, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::set_average(const float* host) {
    CMOOP_REQUIRE(ema_ != nullptr, "set_average: the net has no average (set_ema with momentum > 0 first)");
    CMOOP_REQUIRE(host != nullptr, "set_average: NULL buffer");
    CMOOP_HIP(hipMemcpyAsync(ema_, host, n_params_ * 4, hipMemcpyHostToDevice, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::finalize_average() {
    CMOOP_REQUIRE(ema_ != nullptr, "finalize_average: the net has no average (set_ema with momentum > 0 first)");
    CMOOP_HIP(hipMemcpyAsync(weights_, ema_, n_params_ * 4, hipMemcpyDeviceToDevice, stream_));
}

void Net::ensure_quant_table() {
    if (qtab_ready_) return;
    qtab_ = quant_table(plan_);
    qtab_ready_ = true;
}

void Net::set_quant(const QuantCfg* quant) {
    if (quant) quant_check(*quant);
    const bool on = quant != nullptr && quant_enabled(*quant);
    if (on && !wq_) {
        ensure_quant_table();
        wq_ = dalloc(n_params_);
        qtab_dev_ = reinterpret_cast<QuantRow*>(dalloc(qtab_.rows.size() * sizeof(QuantRow) / sizeof(float) + 4));
        CMOOP_HIP(hipMemcpyAsync(qtab_dev_, qtab_.rows.data(), qtab_.rows.size() * sizeof(QuantRow), hipMemcpyHostToDevice, stream_));
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));     // nothing of the old option is still running; the table's upload is done
    quant_cfg_ = on ? *quant : QuantCfg();
    quant_on_ = on;
    if (!on) int8_levels_off();                   // integer inference needs the weight codes
    option_changed(on);
}

int64_t Net::quant_size_bytes() {
    CMOOP_REQUIRE(quant_on_, "quant_size_bytes: the option is off (set_quant with bits in [2, 8] first)");
    return cmoop::quant_size_bytes(qtab_, n_params_, quant_cfg_.bits);
}

void Net::get_quantized(float* wq_host, int8_t* codes_host, float* scales_host) {
    CMOOP_REQUIRE(quant_on_, "get_quantized: the option is off (set_quant with bits in [2, 8] first)");
    PoolScope pool(stream_);   // full-arena copies of this call: the net's own quantised arena holds kernel elements only
    const size_t n = (size_t)n_params_;
    float* d_wq = pool.get<float>(std::max<size_t>(n, 1) * 4);
    int8_t* d_codes = pool.get<int8_t>(std::max<size_t>(n, 4));
    float* d_scales = pool.get<float>(std::max<size_t>((size_t)qtab_.total_channels, 1) * 4);
    CMOOP_HIP(hipMemcpyAsync(d_wq, params_, n * 4, hipMemcpyDeviceToDevice, stream_));
    CMOOP_HIP(hipMemsetAsync(d_codes, 0, n, stream_));
    stage_kernels(prune_cfg_.sparsity, wp_, nullptr, d_wq, d_codes, d_scales);   // what inference reads
    if (wq_host) CMOOP_HIP(hipMemcpyAsync(wq_host, d_wq, n * 4, hipMemcpyDeviceToHost, stream_));
    if (codes_host) CMOOP_HIP(hipMemcpyAsync(codes_host, d_codes, n, hipMemcpyDeviceToHost, stream_));
    if (scales_host) CMOOP_HIP(hipMemcpyAsync(scales_host, d_scales, (size_t)qtab_.total_channels * 4, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::ensure_prune_table() {
    if (ptab_skip_small_ == prune_cfg_.skip_small) return;
    ptab_ = prune_table(plan_, prune_cfg_.skip_small != 0);
    ptab_skip_small_ = prune_cfg_.skip_small;
}

void Net::set_prune(const PruneCfg* prune) {
    if (prune) prune_check(*prune);
    const bool on = prune != nullptr && prune_enabled(*prune);
    CMOOP_HIP(hipStreamSynchronize(stream_));     // nothing of the old option is still running
    prune_cfg_ = on ? *prune : PruneCfg();
    if (on) {
        const bool fresh = wp_ == nullptr;
        const int before = ptab_skip_small_;
        ensure_prune_table();
        if (fresh) {
            wp_ = dalloc(n_params_);
            ptab_dev_ = reinterpret_cast<PruneRow*>(dalloc(ptab_.rows.size() * sizeof(PruneRow) / sizeof(float) + 4));
            uint32_t* words = reinterpret_cast<uint32_t*>(dalloc(prune_workspace_words((int)ptab_.rows.size())));
            prune_workspace_init(prune_ws_, words, (int)ptab_.rows.size(), stream_);
        }
        if (fresh || before != ptab_skip_small_)   // the rows differ only in k: the same count, the same buffer
            CMOOP_HIP(hipMemcpyAsync(ptab_dev_, ptab_.rows.data(), ptab_.rows.size() * sizeof(PruneRow), hipMemcpyHostToDevice, stream_));
        CMOOP_HIP(hipStreamSynchronize(stream_)); // the table's upload is done: ptab_ may be rebuilt by a later call
    }
    prune_on_ = on;
    option_changed(on);
}

int Net::prune_rows() {
    CMOOP_REQUIRE(prune_on_, "prune_rows: the option is off (set_prune with sparsity in (0, 1) first)");
    return (int)ptab_.rows.size();
}

double Net::prune_achieved(const uint32_t* zeros) {
    CMOOP_REQUIRE(prune_on_ && zeros, "prune_achieved: the option is off, or zeros is NULL");
    int64_t z = 0, len = 0;
    for (size_t i = 0; i < ptab_.rows.size(); ++i)
        if (prune_row_k(ptab_.rows[i], prune_cfg_.sparsity) > 0) { z += zeros[i]; len += ptab_.rows[i].len; }
    return len ? (double)z / (double)len : 0.0;
}

int64_t Net::prune_size_bytes() {
    CMOOP_REQUIRE(prune_on_, "prune_size_bytes: the option is off (set_prune with sparsity in (0, 1) first)");
    if (quant_on_) ensure_quant_table();
    return cmoop::prune_size_bytes(ptab_, n_params_, prune_cfg_.sparsity, quant_on_ ? quant_cfg_.bits : 0,
                                   quant_on_ ? qtab_.total_channels : 0);
}

void Net::get_pruned(float* weff_host, uint32_t* zeros_host) {
    CMOOP_REQUIRE(prune_on_, "get_pruned: the option is off (set_prune with sparsity in (0, 1) first)");
    PoolScope pool(stream_);   // a full-arena copy of this call: the net's own pruned arena holds kernel elements only
    const size_t n = (size_t)n_params_, rows = ptab_.rows.size();
    float* d_w = pool.get<float>(std::max<size_t>(n, 1) * 4);
    uint32_t* d_zeros = pool.get<uint32_t>(std::max<size_t>(rows, 1) * 4);
    CMOOP_HIP(hipMemcpyAsync(d_w, params_, n * 4, hipMemcpyDeviceToDevice, stream_));
    stage_kernels(prune_cfg_.sparsity, d_w, d_zeros, nullptr, nullptr, nullptr);   // pruned, not quantised
    if (weff_host) CMOOP_HIP(hipMemcpyAsync(weff_host, d_w, n * 4, hipMemcpyDeviceToHost, stream_));
    if (zeros_host) CMOOP_HIP(hipMemcpyAsync(zeros_host, d_zeros, rows * 4, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::set_actquant(const ActQuantCfg* actq) {
    if (actq) actquant_check(*actq);
    const bool on = actq != nullptr && actquant_enabled(*actq);
    if (on && !act_rec_) {   // first use: every site starts unseen (count 0); the partials need no initial value
        const size_t words = (size_t)std::max(plan_.n_sites, 1) * sizeof(ActRange) / sizeof(float);
        act_rec_ = reinterpret_cast<ActRange*>(dalloc(words));
        act_rec_snap_ = reinterpret_cast<ActRange*>(dalloc(words));
        act_partials_ = reinterpret_cast<uint32_t*>(dalloc(ACT_QUANT_MAX_BLOCKS));
        CMOOP_HIP(hipMemsetAsync(act_rec_, 0, words * sizeof(float), stream_));
        CMOOP_HIP(hipMemsetAsync(act_rec_snap_, 0, words * sizeof(float), stream_));   // a snapshot of "no step seen" until the first real one
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));     // nothing of the old option is still running
    actq_cfg_ = on ? *actq : ActQuantCfg();
    actq_on_ = on;
    if (!on) int8_levels_off();                   // integer inference needs the sites' codes
    option_changed(on);
}

void Net::set_int8(bool on) {
    if (!on) {
        CMOOP_HIP(hipStreamSynchronize(stream_));
        int8_levels_off();
        return;
    }
    // every refusal comes before the first allocation or launch: a refused net is the net it was
    CMOOP_REQUIRE(quant_on_, "int8: needs quantised weights -- set_quant with bits in [2, 8] first");
    CMOOP_REQUIRE(actq_on_, "int8: needs quantised activations -- set_actquant with bits in [2, 8] first");
    CMOOP_REQUIRE(act_ranges_ready_, "int8: needs tracked ranges -- run a train step with set_actquant on or load them (set_act_ranges) first");
    const std::vector<Int8Op> iops = int8_ops(plan_);
    CMOOP_HIP(hipStreamSynchronize(stream_));
    std::vector<ActRange> rec((size_t)std::max(plan_.n_sites, 1));
    CMOOP_HIP(hipMemcpy(rec.data(), act_rec_, (size_t)plan_.n_sites * sizeof(ActRange), hipMemcpyDeviceToHost));
    for (int i = 0; i < plan_.n_sites; ++i)
        CMOOP_REQUIRE(std::isfinite(rec[i].r), "int8: the tracked range of site " + std::to_string(i) + " is not finite");
    {   // the scales inference would form now, into pooled buffers.  With pruning on the stage rewrites the net's own pruned
        // arena at the final sparsity on the way: harmless, every step and every pass restages it before reading it
        PoolScope pool(stream_);
        const size_t n = (size_t)n_params_, ch = (size_t)qtab_.total_channels;
        float* d_wq = pool.get<float>(std::max<size_t>(n, 1) * 4);
        float* d_scales = pool.get<float>(std::max<size_t>(ch, 1) * 4);
        stage_kernels(prune_cfg_.sparsity, wp_, nullptr, d_wq, nullptr, d_scales);
        std::vector<float> sc(ch);
        CMOOP_HIP(hipMemcpyAsync(sc.data(), d_scales, ch * 4, hipMemcpyDeviceToHost, stream_));
        CMOOP_HIP(hipStreamSynchronize(stream_));
        for (size_t i = 0; i < ch; ++i) CMOOP_REQUIRE(std::isfinite(sc[i]), "int8: a weight scale is not finite (channel " + std::to_string(i) + ")");
    }
    if (!w_codes_) {
        w_codes_ = reinterpret_cast<int8_t*>(dalloc(((size_t)n_params_ + 3) / 4 + 4));
        w_scales_ = dalloc((size_t)qtab_.total_channels);
        site_codes_.assign((size_t)plan_.n_sites, nullptr);
        for (const Act& a : acts_)
            if (a.site >= 0) site_codes_[a.site] = reinterpret_cast<int8_t*>(dalloc(((size_t)Bmax_ * a.per_sample() + 3) / 4 + 4));
        int8_tab_.assign(ops_.size(), Int8Entry());
        for (const Int8Op& o : iops) int8_tab_[o.op] = Int8Entry{I8_MATRIX, o.scale_off, -1, -1};
    }
    int8_.on = true;
}

void Net::set_int8_depthwise(bool on) {
    if (on) {
        CMOOP_REQUIRE(int8_.on, "int8 depthwise: needs integer inference -- set_int8 first");
        const std::vector<Int8DwOp> dops = int8_dw_ops(plan_);   // asserts that every depthwise op reads and writes a site
        for (const Int8DwOp& o : dops) int8_tab_[o.op] = Int8Entry{I8_DEPTHWISE, o.scale_off, -1, -1};
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));     // nothing of the old level is still running
    int8_.depthwise = on;
}

void Net::set_int8_fused(bool on) {
    if (on) {
        CMOOP_REQUIRE(int8_.on, "int8 fused: needs integer inference -- set_int8 first");
        const std::vector<Int8FusedOp> fops = int8_fused_ops(plan_);   // asserts the sites, Cout % 4 and the lone reader
        for (const Int8FusedOp& o : fops) {    // a subset of the matrix-core ops: the scale offset is the one set_int8 wrote
            int8_tab_[o.i8.op] = Int8Entry{I8_FUSED, o.i8.scale_off, o.bn, o.site_act};
            if (o.bn >= 0) int8_tab_[o.bn].role = I8_FUSED_BN;
        }
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));     // nothing of the old level is still running
    int8_.fused = on;
}

void Net::get_act_ranges(ActRange* host) {
    CMOOP_REQUIRE(act_rec_ && host, "get_act_ranges: no site records (set_actquant with bits in [2, 8] first), or NULL output");
    CMOOP_HIP(hipMemcpyAsync(host, act_rec_, (size_t)plan_.n_sites * sizeof(ActRange), hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::set_act_ranges(const ActRange* host) {
    CMOOP_REQUIRE(act_rec_ && host, "set_act_ranges: no site records (set_actquant with bits in [2, 8] first), or NULL input");
    bool ready = plan_.n_sites > 0 ? true : act_ranges_ready_;
    for (int i = 0; i < plan_.n_sites; ++i) {
        CMOOP_REQUIRE(host[i].count >= 0, "set_act_ranges: count must not be negative");
        CMOOP_REQUIRE(!(host[i].r < 0.f) && !(host[i].m_b < 0.f), "set_act_ranges: r and m_b must not be negative");
        // integer inference is on: what set_int8 refused at enabling is refused here as well (nothing is loaded)
        CMOOP_REQUIRE(!int8_.on || std::isfinite(host[i].r), "set_act_ranges: the tracked range of site " + std::to_string(i) +
                      " is not finite while integer inference is on (set_int8(false) first)");
        ready = ready && host[i].count > 0;
    }
    CMOOP_HIP(hipMemcpyAsync(act_rec_, host, (size_t)plan_.n_sites * sizeof(ActRange), hipMemcpyHostToDevice, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));     // host is the caller's
    act_ranges_ready_ = ready;
}

void Net::get_act(int i, int B, int32_t dims[6], float* data_host, float* grad_host) {
    CMOOP_REQUIRE(i >= 0 && i < (int)acts_.size(), "get_act: act index out of range");
    const Act& a = acts_[i];
    if (dims) {
        dims[0] = a.H; dims[1] = a.W; dims[2] = a.C; dims[3] = a.data != nullptr; dims[4] = a.grad != nullptr;
        dims[5] = (int32_t)acts_.size();
    }
    if (!data_host && !grad_host) return;
    CMOOP_REQUIRE(a.data != nullptr, "get_act: this act is never materialised (the input features, or a BatchNorm output fused into its pool)");
    CMOOP_REQUIRE(B >= 1 && B <= Bmax_ && (!grad_host || B <= cfg_.batch), "get_act: B outside the rows the net holds");
    const size_t bytes = (size_t)B * a.per_sample() * 4;
    if (data_host) CMOOP_HIP(hipMemcpyAsync(data_host, a.data, bytes, hipMemcpyDeviceToHost, stream_));
    if (grad_host) {
        CMOOP_REQUIRE(a.grad != nullptr, "get_act: this act has no gradient buffer");
        CMOOP_HIP(hipMemcpyAsync(grad_host, a.grad, bytes, hipMemcpyDeviceToHost, stream_));
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::optim_stats(double out[4]) {
    out[0] = 0.0; out[1] = 0.0; out[2] = 1.0; out[3] = (double)optim_last_path_;
    if (optim_last_path_ != 1) { CMOOP_HIP(hipStreamSynchronize(stream_)); return; }
    OptimRecord rec;
    CMOOP_HIP(hipMemcpyAsync(&rec, optim_rec_, sizeof(rec), hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
    out[0] = rec.sumsq; out[1] = (double)rec.norm; out[2] = (double)rec.scale;
}

void Net::begin_epoch() {
    host_row0_ = 0;
    if (st_dev_) CMOOP_HIP(hipMemsetAsync(&st_dev_->row0, 0, sizeof(long long), stream_));
}

void Net::train_step_stateful(const float* X, const int32_t* y, const int32_t* idx, int B) {
    CMOOP_REQUIRE(B >= 1 && B <= cfg_.batch, "train batch larger than configured");
    if (!st_dev_) {   // no device state (step budget beyond the table limit): explicit-argument steps
        train_step(X, y, idx, host_row0_, B);
        host_row0_ += B;
        g_step_counts[STEP_COUNT_EAGER].fetch_add(1, std::memory_order_relaxed);
        return;
    }
    CMOOP_REQUIRE(iterations_ < alpha_tab_n_, "train_step_stateful outside begin_fit's step budget");
    const BatchRows rows{idx, 0, gather_rows_, st_dev_};
    counted_step([&] {
        // EMA (like the other options begin_fit lists) stays out of captures: graph_ok_ is false for good once one was on
        if (graph_ok_ && !ema_on_ && B == cfg_.batch && !profiling_now_ && step_ >= 1) {
            // a replay runs none of step_body's host code: what it refuses is refused here, whatever a capture holds
            require_step_allowed(true);
            const StepCaptureKey key = capture_key(X, y, idx);
            if (graph_exec_ && !(key == graph_key_)) {   // the capture froze other arguments than this call's: it is stale
                CMOOP_HIP(hipStreamSynchronize(stream_));   // its earlier replays have finished before it is destroyed
                option_changed(false);
            }
            if (!graph_exec_) {   // capture the step once (thread-local mode: the other candidates' threads keep launching)
                hipGraph_t graph = nullptr;
                bool ok = hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal) == hipSuccess;
                if (ok) {
                    try {
                        gathered_step(X, y, rows, B);
                    } catch (...) {
                        hipStreamEndCapture(stream_, &graph);
                        if (graph) hipGraphDestroy(graph);
                        throw;
                    }
                    ok = hipStreamEndCapture(stream_, &graph) == hipSuccess && graph != nullptr;
                }
                if (ok) ok = hipGraphInstantiate(&graph_exec_, graph, nullptr, nullptr, 0) == hipSuccess;
                if (graph) hipGraphDestroy(graph);
                if (!ok) {
                    (void)hipGetLastError();
                    graph_exec_ = nullptr;
                    graph_ok_ = false;      // fall back to eager steps for this candidate (step_launch_counts shows it: no capture, no replay)
                } else {
                    graph_key_ = key;
                    g_step_counts[STEP_COUNT_CAPTURES].fetch_add(1, std::memory_order_relaxed);
                }
            }
            if (graph_exec_) {
                CMOOP_HIP(hipGraphLaunch(graph_exec_, stream_));
                g_step_counts[STEP_COUNT_REPLAYS].fetch_add(1, std::memory_order_relaxed);
                return;
            }
        }
        gathered_step(X, y, rows, B);
        g_step_counts[STEP_COUNT_EAGER].fetch_add(1, std::memory_order_relaxed);
    });
}

void Net::get_state(float* params, float* m, float* v, long long* iterations, long long* steps) {
    if (params) CMOOP_HIP(hipMemcpyAsync(params, weights_, n_params_ * 4, hipMemcpyDeviceToHost, stream_));
    if (m) CMOOP_HIP(hipMemcpyAsync(m, adam_m_, n_params_ * 4, hipMemcpyDeviceToHost, stream_));
    if (v) CMOOP_HIP(hipMemcpyAsync(v, adam_v_, n_params_ * 4, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
    if (iterations) *iterations = iterations_;
    if (steps) *steps = step_;
}

void Net::set_state(const float* params, const float* m, const float* v, long long iterations, long long steps) {
    CMOOP_REQUIRE(iterations >= 0 && steps >= 0 && iterations < (1ll << 31) && steps < (1ll << 31), "set_state: counters out of range");
    if (params) CMOOP_HIP(hipMemcpyAsync(weights_, params, n_params_ * 4, hipMemcpyHostToDevice, stream_));
    if (m) CMOOP_HIP(hipMemcpyAsync(adam_m_, m, n_params_ * 4, hipMemcpyHostToDevice, stream_));
    if (v) CMOOP_HIP(hipMemcpyAsync(adam_v_, v, n_params_ * 4, hipMemcpyHostToDevice, stream_));
    iterations_ = iterations;
    step_ = steps;
    upload_step_state();
    CMOOP_HIP(hipStreamSynchronize(stream_));
    option_changed(false);
}

void Net::set_augment(const AugmentCfg* aug) {
    const bool on = aug != nullptr && augment_enabled(*aug);
    if (aug) augment_check(*aug, T_, F_);
    if (on) {
        CMOOP_REQUIRE((int64_t)cfg_.batch * T_ * F_ < (1ll << 32), "augment: batch * T * F must stay below 2^32");
        aug_ = augment_params(*aug);
        if (!aug_buf_) aug_buf_ = dalloc((size_t)cfg_.batch * T_ * F_);
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));
    aug_on_ = on;
    option_changed(false);
}

void Net::set_loss(const LossCfg* loss) {
    const bool on = loss != nullptr && loss_enabled(*loss);
    if (loss) loss_check(*loss, cfg_.classes);
    const bool mix = on && loss_mixup_on(*loss);
    MixupParams mp;
    TargetParams tp;
    if (on) {
        const size_t C = (size_t)cfg_.classes;
        ensure_target_buffers();
        std::vector<float> tab, cw;
        if (mix) {
            CMOOP_REQUIRE((int64_t)T_ * F_ < (1ll << 30), "mixup: T * F must stay below 2^30");
            tab.resize(MIXUP_TABLE);
            mixup_table(loss->mixup_alpha, tab.data());
            if (!lam_tab_) lam_tab_ = dalloc(MIXUP_TABLE);
            if (!mix_buf_) mix_buf_ = dalloc((size_t)cfg_.batch * T_ * F_);
            CMOOP_HIP(hipMemcpyAsync(lam_tab_, tab.data(), MIXUP_TABLE * 4, hipMemcpyHostToDevice, stream_));
            mp.on = 1;
            mp.gate_thr = (uint32_t)std::floor(loss->mixup_p * 16777216.0);
            mp.tab = lam_tab_;
        }
        if (loss->class_weight) {
            cw.resize(C);
            for (size_t j = 0; j < C; ++j) cw[j] = (float)loss->class_weight[j];
            if (!cw_dev_) cw_dev_ = dalloc(C);
            CMOOP_HIP(hipMemcpyAsync(cw_dev_, cw.data(), C * 4, hipMemcpyHostToDevice, stream_));
        }
        tp = target_params(*loss, cfg_.classes, cw_dev_);
        CMOOP_HIP(hipStreamSynchronize(stream_));   // tab and cw are locals
    } else {
        CMOOP_HIP(hipStreamSynchronize(stream_));
    }
    loss_on_ = on;
    mix_on_ = mix;
    mixp_ = mp;
    tgtp_ = tp;
    option_changed(false);
}

void Net::set_gather_rows(int64_t n) {
    CMOOP_REQUIRE(!distill_on_ || n == 0 || n == kd_rows_, "distill: the teacher table has " + std::to_string(kd_rows_) +
                  " rows, the training split " + std::to_string(n));
    gather_rows_ = n;
}

void Net::set_distill(const DistillCfg* distill) {
    if (distill) distill_check(*distill, cfg_.classes, distill->n_rows);
    const bool on = distill != nullptr && distill_enabled(*distill);
    if (on) {
        ensure_target_buffers();
        if (!kd_q_) kd_q_ = dalloc((size_t)cfg_.batch * cfg_.classes);
    }
    CMOOP_HIP(hipStreamSynchronize(stream_));
    distill_on_ = on;
    kdp_ = on ? distill_params(*distill) : DistillParams();
    kd_zt_ = on ? distill->teacher_logits : nullptr;
    kd_rows_ = on ? distill->n_rows : 0;
    option_changed(false);
}

void Net::loss_buffers(int64_t out[4]) const {
    out[0] = mix_buf_ ? (int64_t)cfg_.batch * T_ * F_ : 0;
    out[1] = tgt_t_ ? (int64_t)cfg_.batch * cfg_.classes : 0;
    out[2] = tgt_w_ ? (int64_t)cfg_.batch : 0;
    out[3] = tgt_primary_ ? (int64_t)cfg_.batch : 0;
}

void Net::run_epoch(const float* X, const int32_t* y, int64_t n_train, int epoch) {
    CMOOP_REQUIRE(n_train >= 1 && n_train < (1ll << 31) && epoch >= 0, "run_epoch: bad arguments");
    const int64_t spe = (n_train + cfg_.batch - 1) / cfg_.batch;
    // the device StepState / step-size table of the fit loop, (re)built when this epoch runs past what is there
    if (!st_dev_ || iterations_ + spe > alpha_tab_n_)
        begin_fit(std::max<int64_t>((int64_t)std::max(cfg_.epochs, 1) * spe, iterations_ + spe));
    set_gather_rows(n_train);
    const int32_t* idx = nullptr;
    if (cfg_.shuffle) {
        // the permutation lives in a buffer of the net, at the same address every epoch, so a captured step stays valid
        // across epochs (a pooled buffer per call moves: the pool hands equal-sized blocks out oldest first)
        if (n_train > epoch_idx_n_) {
            CMOOP_HIP(hipStreamSynchronize(stream_));   // nothing queued still reads the shorter one
            dfree(epoch_idx_);
            epoch_idx_ = nullptr; epoch_idx_n_ = 0;
            epoch_idx_ = reinterpret_cast<int32_t*>(dalloc((size_t)n_train));
            epoch_idx_n_ = n_train;
        }
        if (n_train <= EPOCH_PERMUTATION_DEVICE_MAX) {
            launch_epoch_permutation(seed_, (uint32_t)epoch, n_train, epoch_idx_, stream_);
        } else {
            std::vector<int32_t> h(n_train);
            epoch_permutation(seed_, (uint32_t)epoch, n_train, h.data());
            CMOOP_HIP(hipMemcpyAsync(epoch_idx_, h.data(), n_train * 4, hipMemcpyHostToDevice, stream_));
            CMOOP_HIP(hipStreamSynchronize(stream_));
        }
        idx = epoch_idx_;
    }
    if (st_dev_) {   // explicit-argument steps (session API) do not advance the device state: start the epoch from the host's counters
        upload_step_state();
        CMOOP_HIP(hipStreamSynchronize(stream_));
    }
    begin_epoch();
    for (int64_t s = 0; s < n_train; s += cfg_.batch)
        train_step_stateful(X, y, idx, (int)std::min<int64_t>(cfg_.batch, n_train - s));
}

template <class Source, class Sink> void Net::inference_pass(int64_t n, Source&& source, Sink&& sink) {
    // once per call, on the arena this pass reads; integer inference: with the codes and scales its integer launches take
    if (int8_.on) kernels_ = stage_kernels(prune_cfg_.sparsity, wp_, nullptr, wq_, w_codes_, w_scales_);
    else refresh_kernels(prune_cfg_.sparsity);
    for (int64_t s = 0; s < n; s += cfg_.eval_batch) {
        const int B = (int)std::min<int64_t>(cfg_.eval_batch, n - s);
        const std::pair<const float*, BatchRows> in = source(s, B);
        forward(in.first, in.second, B, false);
        sink(s, B);
    }
}
// the chunk source of a resident tensor: rows [s, s + B) of X
static auto resident_rows(const float* X) {
    return [X](int64_t s, int) { return std::make_pair(X, BatchRows{nullptr, s}); };
}

void Net::evaluate(const float* X, const int32_t* y, int64_t n, double* loss_sum, long long* correct, int32_t* preds) {
    require_act_ranges();   // before the accumulator's memset: a refused call enqueues nothing
    CMOOP_HIP(hipMemsetAsync(acc_eval_, 0, 16, stream_));
    inference_pass(n, resident_rows(X), [&](int64_t s, int B) {
        launch_softmax_ce(acts_[logits_].data, y, BatchRows{nullptr, s}, B, cfg_.classes, nullptr, acc_eval_, preds ? preds + s : nullptr, stream_);
    });
    double host[2];
    CMOOP_HIP(hipMemcpyAsync(host, acc_eval_, 16, hipMemcpyDeviceToHost, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
    *loss_sum = host[0];
    std::memcpy(correct, &host[1], 8);
}

void Net::predict(const float* X, int64_t n, float* probs) {
    CMOOP_REQUIRE(n >= 0 && (n == 0 || (X && probs)), "predict: NULL buffer");
    require_act_ranges();
    inference_pass(n, resident_rows(X),
                   [&](int64_t s, int B) { launch_softmax_probs(acts_[logits_].data, probs + s * cfg_.classes, B, cfg_.classes, stream_); });
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

void Net::predict_logits(const float* X, int64_t n, float* logits) {
    CMOOP_REQUIRE(n >= 0 && (n == 0 || (X && logits)), "predict_logits: NULL buffer");
    require_act_ranges();
    inference_pass(n, resident_rows(X), [&](int64_t s, int B) {
        CMOOP_HIP(hipMemcpyAsync(logits + s * cfg_.classes, acts_[logits_].data, (size_t)B * cfg_.classes * 4, hipMemcpyDeviceToDevice,
                                 stream_));
    });
    CMOOP_HIP(hipStreamSynchronize(stream_));
}

int64_t stream_windows(int64_t n_frames, int T, int hop) {
    CMOOP_REQUIRE(hop >= 1, "stream windows: hop_frames must be at least 1");
    CMOOP_REQUIRE(T >= 1 && n_frames >= T, "stream windows: the stream has " + std::to_string(n_frames) + " frames, a window needs " + std::to_string(T));
    return 1 + (n_frames - T) / hop;
}

void Net::predict_stream(const float* feat, int64_t n_frames, int hop, bool db_scale, bool db_ref_max, float db_amin, float top_db,
                         const double* mean, const double* scale, float* probs) {
    const int64_t n = stream_windows(n_frames, T_, hop);
    CMOOP_REQUIRE(feat && probs, "predict_stream: NULL buffer");
    CMOOP_REQUIRE((mean == nullptr) == (scale == nullptr), "predict_stream: mean and scale come together (both or neither)");
    require_act_ranges();
    const int B0 = (int)std::min<int64_t>(cfg_.eval_batch, n);
    PoolScope pool(stream_);   // the chunk and the scaler go back once the stream has drained
    float* chunk = pool.get<float>((size_t)B0 * T_ * F_ * 4);
    double* ms = mean ? pool.get<double>((size_t)2 * F_ * 8) : nullptr;
    if (ms) {
        CMOOP_HIP(hipMemcpyAsync(ms, mean, (size_t)F_ * 8, hipMemcpyHostToDevice, stream_));
        CMOOP_HIP(hipMemcpyAsync(ms + F_, scale, (size_t)F_ * 8, hipMemcpyHostToDevice, stream_));
    }
    auto gather = [&](int64_t w, int B) {   // window i sits at position i % eval_batch of chunk i / eval_batch
        launch_window_gather(feat, chunk, w, B, hop, T_, F_, db_scale ? 1 : 0, db_ref_max ? 1 : 0, db_amin, top_db, ms,
                             ms ? ms + F_ : nullptr, stream_);
        return std::make_pair((const float*)chunk, BatchRows());
    };
    inference_pass(n, gather, [&](int64_t w, int B) { launch_softmax_probs(acts_[logits_].data, probs + w * cfg_.classes, B, cfg_.classes, stream_); });
}

void Net::read_train_metrics(double* loss_sum, long long* correct, bool reset) {
    double host[2];
    CMOOP_HIP(hipMemcpyAsync(host, acc_train_, 16, hipMemcpyDeviceToHost, stream_));
    if (reset) CMOOP_HIP(hipMemsetAsync(acc_train_, 0, 16, stream_));
    CMOOP_HIP(hipStreamSynchronize(stream_));
    *loss_sum = host[0];
    std::memcpy(correct, &host[1], 8);
}

// ---------------------------------------------------------------------------
void epoch_permutation(uint32_t seed, uint32_t epoch, int64_t n, int32_t* out) {
    std::vector<uint64_t> key(n);
    const uint32_t prefix = rng_prefix(seed, STREAM_SHUFFLE, epoch);
    for (int64_t i = 0; i < n; ++i) key[i] = ((uint64_t)fmix32(prefix ^ (uint32_t)i) << 32) | (uint64_t)i;
    std::sort(key.begin(), key.end());
    for (int64_t i = 0; i < n; ++i) out[i] = (int32_t)(key[i] & 0xFFFFFFFFull);
}

double fpr_from_confusion(const int64_t* cm, int C, int variant) {
    // calculate_fpr: V1 nsga_penalty.py:351-364 ; V3 ablation_study/sa_nsga_local.py:138-141
    long long total = 0;
    std::vector<long long> row(C, 0), col(C, 0);
    for (int i = 0; i < C; ++i)
        for (int j = 0; j < C; ++j) { total += cm[i * C + j]; row[i] += cm[i * C + j]; col[j] += cm[i * C + j]; }
    double sum = 0.0;
    int cnt = 0;
    for (int i = 0; i < C; ++i) {
        const long long fp = col[i] - cm[i * C + i];
        if (variant == 2) {
            const long long den = total - row[i];
            if (den > 0) { sum += (double)fp / (double)den; ++cnt; }
        } else {
            const long long tn = total - (row[i] + col[i] - cm[i * C + i]);
            sum += (fp + tn) > 0 ? (double)fp / (double)(fp + tn) : 0.0;
            ++cnt;
        }
    }
    // np.mean sums left to right in float64 for such short lists (pairwise kicks in at 128 elements)
    return cnt ? sum / cnt : 0.0;
}

void operating_point(const float* probs, const int32_t* y, int64_t n, int C, double recall, OpointClass* classes, double summary[4],
                     hipStream_t s) {
    opoint_check_shape(n, C);
    CMOOP_REQUIRE(classes && summary && (n == 0 || (probs && y)), "operating_point: NULL buffer");
    PoolScope pool(s);   // key, counts and records go back once the stream has drained
    const size_t cells = std::max<size_t>((size_t)n * C, 1);
    uint32_t* d_key = pool.get<uint32_t>(cells * 4);
    int32_t* d_cnt = pool.get<int32_t>(cells * 16);
    OpointClass* d_rec = pool.get<OpointClass>((size_t)C * sizeof(OpointClass));
    launch_score_keys(probs, d_key, n, C, s);
    launch_roc_counts(d_key, y, d_cnt, n, C, s);
    launch_opoint_select(d_key, y, d_cnt, n, C, recall, d_rec, s);
    CMOOP_HIP(hipMemcpyAsync(classes, d_rec, (size_t)C * sizeof(OpointClass), hipMemcpyDeviceToHost, s));
    CMOOP_HIP(hipStreamSynchronize(s));
    opoint_summary(classes, C, summary);
}

EvalResult fit_and_read_out(Net& net, const NetConfig& cfg, const Dataset& ds, uint32_t seed, FitHistory* hist) {
    const auto t0 = std::chrono::steady_clock::now();
    CMOOP_REQUIRE(ds.n_train >= 1 && ds.n_val >= 1, "empty train or validation split");
    CMOOP_REQUIRE(ds.n_train < (1ll << 31) && ds.n_val < (1ll << 31), "split too large");
    if (opoint_enabled(net.opoint())) opoint_check_shape(ds.n_val, cfg.classes);   // fail before the fit, not after it
    hipStream_t stream = net.stream();
    EvalResult res;
    res.size_mb = (double)(net.total_params() * 4) / (1024.0 * 1024.0);   // compute_model_size_mb, nsga_penalty.py:337-344
    if (net.quant_on()) {   // the size of the model the fit trains and scores; size_mb stays the fp32 bytes
        res.quant[0] = (double)net.quant_size_bytes() / (1024.0 * 1024.0);
        res.quant[1] = (double)net.quant().bits;
    }
    if (net.prune_on()) {   // the size of the sparse model the fit scores (with the quantiser's bits when both are on)
        res.prune[0] = (double)net.prune_size_bytes() / (1024.0 * 1024.0);
        res.prune[1] = net.prune().sparsity;
    }

    PoolScope pool(stream);   // everything below goes back once the stream has drained, however the fit ends
    int32_t* h_idx = nullptr;
    int32_t* d_idx = pool.get<int32_t>(ds.n_train * 4);
    int32_t* d_preds = pool.get<int32_t>(ds.n_val * 4);
    int64_t* d_cm = pool.get<int64_t>((size_t)cfg.classes * cfg.classes * 8);
    // Model.fit + EarlyStopping(monitor='val_loss', patience) -- keras/src/callbacks/early_stopping.py (3.6)
    double best = INFINITY, last_val_acc = 0.0, last_val_loss = 0.0;
    long long last_corr = 0;
    int wait = 0, best_epoch = -1;
    bool have_best = false, preds_are_final = false;
    net.set_gather_rows(ds.n_train);
    // (a session net that has already trained continues from its own optimizer.iterations)
    net.begin_fit(net.iterations_done() + (int64_t)cfg.epochs * ((ds.n_train + cfg.batch - 1) / cfg.batch));
    // Weight EMA on: every validation pass (and so the monitored loss, the history, the snapshot and the read-outs) is that
    // of the average arena; training between them continues on the raw weights.  Off: nothing below changes
    const bool avg = net.average_on();
    struct AverageScope {   // inference reads the parameters again however the fit ends, a throw included
        Net& net; bool avg;
        ~AverageScope() { if (avg) net.use_average(false); }
    } average_scope{net, avg};
    for (int epoch = 0; epoch < cfg.epochs; ++epoch) {
        if (avg) net.use_average(false);
        if (cfg.shuffle && ds.n_train <= EPOCH_PERMUTATION_DEVICE_MAX) {
            launch_epoch_permutation(seed, (uint32_t)epoch, ds.n_train, d_idx, stream);   // no host sort, no H2D
        } else if (cfg.shuffle || epoch == 0) {
            if (!h_idx) h_idx = pool.get_pinned<int32_t>(ds.n_train * 4);
            if (cfg.shuffle) epoch_permutation(seed, (uint32_t)epoch, ds.n_train, h_idx);
            else std::iota(h_idx, h_idx + ds.n_train, 0);
            CMOOP_HIP(hipMemcpyAsync(d_idx, h_idx, ds.n_train * 4, hipMemcpyHostToDevice, stream));
            CMOOP_HIP(hipStreamSynchronize(stream));   // h_idx is rewritten next epoch
        }
        net.begin_epoch();
        for (int64_t s = 0; s < ds.n_train; s += cfg.batch)
            net.train_step_stateful(ds.x_train, ds.y_train, d_idx, (int)std::min<int64_t>(cfg.batch, ds.n_train - s));
        double ls; long long corr;
        if (avg) net.use_average(true);   // until the next epoch's first step: snapshot_params below copies what this pass read
        net.evaluate(ds.x_val, ds.y_val, ds.n_val, &ls, &corr, d_preds);   // keeps this epoch's predictions
        net.drain_profile();
        last_val_loss = ls / (double)ds.n_val;
        last_val_acc = (double)corr / (double)ds.n_val;
        last_corr = corr;
        preds_are_final = true;     // d_preds / last_val_* describe the weights the net holds right now
        res.epochs_run = epoch + 1;
        if (hist) { hist->val_loss.push_back(last_val_loss); hist->val_acc.push_back(last_val_acc); }
        if (!cfg.early_stop) continue;
        if (cfg.restore_best && !have_best) { net.snapshot_params(); have_best = true; }
        ++wait;
        if (last_val_loss < best) {
            best = last_val_loss;
            if (cfg.restore_best) net.snapshot_params();
            best_epoch = epoch;
            wait = 0;
            continue;
        }
        if (wait >= cfg.patience && epoch > 0) break;
    }
    if (hist) hist->best_epoch = best_epoch;
    if (avg) net.use_average(false);
    if (cfg.early_stop && cfg.restore_best && have_best && best_epoch != res.epochs_run - 1) {
        net.restore_snapshot();      // weights of an earlier epoch: the last pass's predictions no longer apply
        preds_are_final = false;
    } else if (avg) {
        // the parameter arena becomes the weights that were scored (Keras' finalize_variable_values): the average of the last
        // epoch, which the last validation pass read -- so that pass still IS the read-out pass below
        net.finalize_average();
    }
    // readouts: model.evaluate / model.predict + argmax + confusion matrix (one inference pass yields both).  When
    // the net still holds the weights of its last epoch, that epoch's validation pass IS this pass (inference is
    // deterministic): its loss, accuracy and predictions are reused instead of recomputing N_val forward passes.
    double ls = last_val_loss * (double)ds.n_val;
    long long corr = last_corr;
    if (!preds_are_final) net.evaluate(ds.x_val, ds.y_val, ds.n_val, &ls, &corr, d_preds);
    res.val_loss = cfg.acc_readout == 0 ? last_val_loss : ls / (double)ds.n_val;
    res.acc = cfg.acc_readout == 0 ? last_val_acc : (double)corr / (double)ds.n_val;
    launch_confusion(ds.y_val, d_preds, ds.n_val, cfg.classes, cfg.fpr_variant == 1, d_cm, stream);
    std::vector<int64_t> cm((size_t)cfg.classes * cfg.classes);
    CMOOP_HIP(hipMemcpyAsync(cm.data(), d_cm, cm.size() * 8, hipMemcpyDeviceToHost, stream));
    CMOOP_HIP(hipStreamSynchronize(stream));
    res.fpr = fpr_from_confusion(cm.data(), cfg.classes, cfg.fpr_variant == 2 ? 2 : 0);
    // Operating-point read-out (opt-in): the weights are final here -- the restored snapshot, the finalised average or the last
    // epoch -- so one predict over the validation split gives the scores a deployed model would give; always against the true
    // labels (the y_true quirk belongs to the arg-max FPR above).  Off: nothing is launched or allocated
    if (opoint_enabled(net.opoint())) {
        float* d_probs = pool.get<float>((size_t)ds.n_val * cfg.classes * 4);
        net.predict(ds.x_val, ds.n_val, d_probs);
        std::vector<OpointClass> classes(cfg.classes);
        operating_point(d_probs, ds.y_val, ds.n_val, cfg.classes, net.opoint().recall, classes.data(), res.opoint, stream);
        net.store_opoint(classes.data(), res.opoint);
    } else {
        net.store_opoint(nullptr, nullptr);
    }
    if (net.prune_on()) {   // the zero fraction of the pruned tensors of the model that was just scored
        std::vector<uint32_t> zeros((size_t)net.prune_rows());
        net.get_pruned(nullptr, zeros.data());
        res.prune[2] = net.prune_achieved(zeros.data());
    }
    res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return res;
}

EvalResult run_candidate(const int32_t gene[6], const NetConfig& cfg, const Dataset& ds, uint32_t seed, hipStream_t stream,
                         const TrainOptions& opt) {
    const auto t0 = std::chrono::steady_clock::now();
    CMOOP_REQUIRE(ds.n_train >= 1 && ds.n_val >= 1, "empty train or validation split");
    Net net(gene, cfg, ds.T, ds.F, seed, stream);
    net.set_options(opt);
    EvalResult res = fit_and_read_out(net, cfg, ds, seed, nullptr);
    res.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    return res;
}

// conv geometries of a candidate at batch B, from the host-only plan
void check_plan_ranges(const int32_t gene[6], int variant, int T, int F, int B) {
    NetConfig cfg;
    cfg.variant = variant;
    const NetPlan plan = plan_net(gene, cfg, T, F);
    // first conv (C_in = 1, direct kernel): its output feeds the GEMM layers, so the same element bound applies to it
    CMOOP_REQUIRE((int64_t)B * T * F * gene[0] < (1ll << 29), "first-layer output exceeds 2^29 elements (32-bit byte offsets): lower the batch / eval_batch");
    for (const Op& op : plan.ops) {
        if (op.kind == OP_CONV) igemm_check_range(op.conv().geometry(B));
        if (op.kind == OP_DWCONV)
            CMOOP_REQUIRE((int64_t)B * op.H * op.W * op.Cin < (1ll << 29), "depthwise activation exceeds 2^29 elements (32-bit offsets): lower the batch / eval_batch");
    }
}

void eval_population(const NetConfig& cfg, const Dataset& ds, const int32_t* genes, const uint32_t* seeds, int n,
                     EvalResult* out, const std::function<int()>& pull, const TrainOptions& opt) {
    if (n <= 0) return;
    for (int i = 0; i < n; ++i) validate_gene(genes + 6 * i);
    for (int i = 0; i < n; ++i) out[i].evaluated = 0;
    // longest first (closed-form FLOPs) so the tail of the generation is made of cheap candidates
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::vector<double> cost(n);
    for (int i = 0; i < n; ++i) cost[i] = fwd_flops_per_sample(genes + 6 * i, cfg.variant, cfg.classes, ds.T, ds.F);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return cost[a] > cost[b]; });
    int dev = 0;
    CMOOP_HIP(hipGetDevice(&dev));
    const int slots = std::max(1, std::min(cfg.n_slots, n));
    std::atomic<int> next{0};
    std::mutex err_mu;
    std::string err;
    auto worker = [&]() {
        hipStream_t stream = nullptr;
        try {
            CMOOP_HIP(hipSetDevice(dev));
            CMOOP_HIP(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking));
            for (;;) {
                { std::lock_guard<std::mutex> l(err_mu); if (!err.empty()) break; }
                int i;
                if (pull) {   // cross-rank queue: the caller hands out candidate indices (shared counter on the c10d store)
                    i = pull();
                    if (i < 0) break;
                    CMOOP_REQUIRE(i < n, "pull callback returned an index outside the population");
                } else {
                    const int j = next.fetch_add(1);
                    if (j >= n) break;
                    i = order[j];
                }
                out[i] = run_candidate(genes + 6 * i, cfg, ds, seeds[i], stream, opt);
                out[i].evaluated = 1;
            }
        } catch (const std::exception& e) {
            std::lock_guard<std::mutex> l(err_mu);
            if (err.empty()) err = e.what();
        }
        if (stream) { hipStreamSynchronize(stream); hipStreamDestroy(stream); }
    };
    std::vector<std::thread> th;
    for (int s = 1; s < slots; ++s) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    if (!err.empty()) throw Error(err);
}

}  // namespace cmoop
