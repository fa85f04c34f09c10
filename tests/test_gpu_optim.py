"""GPU: optimiser options.  The three kernels of the finish + update path alone (``cmoop_grad_finish``: the gradient-finish
and clip-scale launches; ``cmoop_adamw``) -- exact in the integer regime, inside a bound derived from the kernel's structure
in the Gaussian regime, bit-equal to ``optim.adamw_step_ref`` over consecutive updates -- and the trainer: off means off,
an inactive clip holds the three launches to the fused one on a real net's slabs, active options against the statement step
by step, device state against host arguments, a late ``set_optim``, composition with augment / loss / distill, the
population path, inference.  Run with -s to see the figures."""
import ctypes as C
import dataclasses
import functools
import struct

import numpy as np
import pytest
import torch

import _elem_reference as R
from _elem_reference import U, gamma_n
from cmoop_audio_processing_amd import (AugmentConfig, DistillConfig, EvalConfig, LossConfig, OptimConfig, PopulationEvaluator, _lib,
                                        genes as G)
from cmoop_audio_processing_amd import augment as A
from cmoop_audio_processing_amd import distill as D
from cmoop_audio_processing_amd import loss as Ls
from cmoop_audio_processing_amd import optim as O
from cmoop_audio_processing_amd.session import NetSession, epoch_permutation
from test_gpu_net import make_data, make_split

pytestmark = pytest.mark.gpu

P = _lib.ptr
LR, B1, B2, AEPS = 1e-3, 0.9, 0.999, 1e-7               # cmoop_config_default's optimiser constants
# grad_finish_kernel's structure (optim.hip): 256 threads, a plain workgroup covers 1024 elements (4 per thread), a vector slab
# workgroup 64 x 4 and a scalar slab workgroup 64; the longest fp32 chain of a partial is one square, 3 adds in the thread,
# 6 shuffle levels in the wave of 64, 3 adds over the four waves
PLAIN_PER_BLOCK, SLAB_COLS = 1024, 64
CHAIN = 1 + (PLAIN_PER_BLOCK // 256 - 1) + 6 + (256 // 64 - 1)


def L():
    return _lib.lib()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def ok(rc):
    torch.cuda.synchronize()
    _lib.check(rc)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


def make_record(scale):
    return dev(np.frombuffer(struct.pack("<dff", 0.0, 0.0, scale), np.uint8).copy())


def read_record(rec):
    """(sumsq float64, norm float32, scale float32) of the 16-byte device record."""
    raw = host(rec).tobytes()
    return struct.unpack("<d", raw[:8])[0], np.frombuffer(raw[8:12], np.float32)[0], np.frombuffer(raw[12:16], np.float32)[0]


# ---- arenas ------------------------------------------------------------------------------------------------------------------
class Arena:
    """Plain and slab segments tiling an arena as cmoop_adam_segments takes them; segs: [(n, S)], S = 0 plain."""

    def __init__(self, segs):
        self.segs = segs
        self.off, self.n, self.S, self.stride, self.slab_off = [], [], [], [], []
        pos = spos = 0
        for n, S in segs:
            self.off.append(pos); self.n.append(n); self.S.append(S)
            st = (n + 7) // 4 * 4 if S else 0                               # stride > n, a multiple of 4
            self.stride.append(st); self.slab_off.append(spos)
            pos += n
            spos += S * st
        self.total, self.slab_floats = pos, spos
        arr = lambda a, t: np.ascontiguousarray(a, t)
        self.args = (arr(self.off, np.int64), arr(self.n, np.int64), arr(self.S, np.int32), arr(self.stride, np.int64), arr(self.slab_off, np.int64))

    def vector(self, i):
        return self.S[i] > 0 and self.n[i] % 4 == 0 and self.off[i] % 4 == 0

    def blocks(self):
        """[(first element, one past the last)] of every workgroup, in launch order."""
        out = []
        for i, (n, S) in enumerate(self.segs):
            per = PLAIN_PER_BLOCK if S == 0 else (4 * SLAB_COLS if self.vector(i) else SLAB_COLS)
            out += [(self.off[i] + b, self.off[i] + min(n, b + per)) for b in range(0, n, per)]
        return out

    def slab_sums(self, slab, g):
        """g with every slab segment's range replaced by its float64 slice sum; g_in with NaN there (must be overwritten)."""
        g, g_in = g.astype(np.float64), g.copy()
        for i, (n, S) in enumerate(self.segs):
            if S:
                sl = slab[self.slab_off[i]:self.slab_off[i] + S * self.stride[i]].reshape(S, self.stride[i])[:, :n]
                g[self.off[i]:self.off[i] + n] = sl.astype(np.float64).sum(axis=0)
                g_in[self.off[i]:self.off[i] + n] = np.nan
        return g, g_in

    def seg_args(self):
        return [len(self.segs)] + [P(a) for a in self.args]


# the mixed arena of test_gpu_elem_kernels.test_adam_segments_mixed_arena (S = 1 / 3 / 4 / 5 / 32 / 33 / 64, a slab segment with
# n % 4 != 0 and one at off % 4 != 0, a plain segment longer than 1024 and one of length 1) + plain 1023 / 1024 / 1025
MIXED = [(1, 0), (64, 1), (3, 0), (260, 3), (8, 4), (7, 5), (1501, 0), (128, 32), (300, 33), (68, 64), (5, 33), (1023, 0), (12, 4),
         (1024, 0), (516, 5), (1025, 0)]


def fused_g(ar, g_in, slabd):
    """g as the fused launch (cmoop_adam_segments) stores it."""
    gd = dev(g_in)
    z = [dev(np.zeros(ar.total, np.float32)) for _ in range(3)]
    ok(L().cmoop_adam_segments(P(z[0]), P(gd), P(z[1]), P(z[2]), P(slabd), *ar.seg_args(), 1e-3, B1, B2, AEPS))
    return host(gd)


def grad_finish(ar, g_in, slabd, kinds, clip, guard=3):
    """-> (g, partials, sumsq, norm, scale); the partial buffer sits between NaN guards that must survive."""
    nb = len(ar.blocks())
    gd = dev(g_in)
    part = torch.full((nb + 2 * guard,), float("nan"), device="cuda", dtype=torch.float32)
    rec, count = make_record(-7.0), C.c_int32(-1)
    kd = dev(kinds) if kinds is not None else None
    ok(L().cmoop_grad_finish(P(gd), P(slabd), *ar.seg_args(), P(kd), float(clip), P(part[guard:]), nb, C.byref(count), P(rec)))
    p = host(part)
    assert count.value == nb, (count.value, nb)
    assert np.isnan(p[:guard]).all() and np.isnan(p[guard + nb:]).all(), "guards of the partial buffer unchanged"
    return (host(gd), p[guard:guard + nb]) + read_record(rec)


def kind_masks(ar, seed):
    """None, all trainable, and an arena with whole segments and partial ranges (across workgroup edges) frozen."""
    rs = np.random.RandomState(seed)
    k = rs.randint(0, 2, ar.total).astype(np.uint8)
    for i in range(0, len(ar.segs), 3):
        k[ar.off[i]:ar.off[i] + ar.n[i]] = O.KIND_FROZEN                        # whole segments
    for i in range(1, len(ar.segs), 3):
        k[ar.off[i] + ar.n[i] // 3:ar.off[i] + ar.n[i] // 3 + max(1, ar.n[i] // 2)] = O.KIND_FROZEN       # partial ranges
    return [None, np.ones(ar.total, np.uint8), k]


# ---- 1. cmoop_grad_finish -----------------------------------------------------------------------------------------------------
INT_ARENAS = [MIXED, [(1, 0)], [(1023, 0)], [(1024, 0)], [(1025, 0)], [(1, 1)], [(1023, 3)], [(1024, 33)], [(1025, 64)], [(2, 0)]]


@pytest.mark.parametrize("case", range(len(INT_ARENAS)))
def test_grad_finish_integer_regime(case):
    """g in {-3 .. 3}, slab entries in {-1, 0, 1}: every slab sum, every square and every partial is an integer below 2^24, so
    the stored g, each partial and the sum of squares are EXACT; norm and scale within one fp32 ulp of float64; scale is
    exactly 1 wherever norm <= clip."""
    ar = Arena(INT_ARENAS[case])
    rs = np.random.RandomState(50 + case)
    slab = rs.randint(-1, 2, ar.slab_floats).astype(np.float32)
    g0 = rs.randint(-3, 4, ar.total).astype(np.float32)
    if INT_ARENAS[case] == [(2, 0)]:
        g0[:] = (3.0, 4.0)                                                   # norm 5 exactly: the norm == clip case
    g64, g_in = ar.slab_sums(slab, g0)
    gmax = max(4, max(ar.S))                                                 # |plain g| <= 4 (the 3, 4 pair), |slab sum| <= S
    assert 4 * SLAB_COLS * max(ar.S) ** 2 < 2 ** 24 and PLAIN_PER_BLOCK * 16 < 2 ** 24, "every partial stays below 2^24 (from the shape)"
    slabd = dev(slab) if ar.slab_floats else None
    want_g = fused_g(ar, g_in, slabd)
    assert np.array_equal(want_g, g64.astype(np.float32)) and np.abs(g64).max() <= gmax
    for kinds in kind_masks(ar, case):
        live = np.ones(ar.total, bool) if kinds is None else kinds != O.KIND_FROZEN
        sq = np.where(live, g64 * g64, 0.0)
        want_part = np.array([sq[a:b].sum() for a, b in ar.blocks()])
        assert want_part.max() < 2 ** 24
        ss64, norm64 = O.global_norm_ref(g64, kinds)
        assert ss64 == sq.sum()
        clips = [0.0, 1e30, norm64, 0.5 * norm64, float(np.nextafter(norm64, 0.0)), 0.125]
        for clip in clips:
            g, part, ss, norm, scale = grad_finish(ar, g_in, slabd, kinds, clip)
            assert same_bits(g, want_g), "g is bit-equal to the fused launch's"
            assert np.array_equal(part.astype(np.float64), want_part), "every partial is exact"
            assert ss == ss64, (ss, ss64)
            assert abs(float(norm) - norm64) <= ulp32(norm64), (norm, norm64)
            want_scale = O.clip_scale_ref(norm64, clip)
            if clip == 0.0 or norm64 <= clip:
                assert scale == np.float32(1.0) and want_scale == 1.0, (clip, norm64, scale)
            else:                                    # (a clip one double ulp below the norm rounds to 1.0f too)
                assert scale <= 1.0 and abs(float(scale) - want_scale) <= ulp32(want_scale), (clip, scale, want_scale)
    if INT_ARENAS[case] == [(2, 0)]:
        _, _, ss, norm, scale = grad_finish(ar, g_in, slabd, None, 5.0)
        assert (ss, float(norm), float(scale)) == (25.0, 5.0, 1.0), "norm == clip leaves the gradient alone"
        assert grad_finish(ar, g_in, slabd, None, 4.0)[4] == np.float32(0.8)


def test_grad_finish_gaussian_regime_and_reproducibility():
    """Random normal gradients and slabs: g keeps the fused launch's bits; each partial and the sum of squares lie within
    gamma_CHAIN of the float64 sum of the DEVICE's g (every term is >= 0, so sum|term| is the sum); two runs agree bit for bit."""
    ar = Arena(MIXED + [(5000, 0), (4096, 7)])
    rs = np.random.RandomState(77)
    slab = rs.randn(ar.slab_floats).astype(np.float32)
    g0 = (rs.randn(ar.total) * 10.0 ** rs.uniform(-3, 1, ar.total)).astype(np.float32)
    _, g_in = ar.slab_sums(slab, g0)
    slabd = dev(slab)
    want_g = fused_g(ar, g_in, slabd)
    for kinds in kind_masks(ar, 5):
        g, part, ss, norm, scale = grad_finish(ar, g_in, slabd, kinds, 1.0)
        assert same_bits(g, want_g)
        live = np.ones(ar.total, bool) if kinds is None else kinds != O.KIND_FROZEN
        sq = np.where(live, g.astype(np.float64) ** 2, 0.0)
        want_part = np.array([sq[a:b].sum() for a, b in ar.blocks()])
        err = np.abs(part.astype(np.float64) - want_part)
        print(f"\n  partials: worst err / (gamma_{CHAIN} sum) {float((err / np.maximum(gamma_n(CHAIN) * want_part, 1e-300)).max()):.3f}")
        assert (err <= gamma_n(CHAIN) * want_part).all()
        ss64, norm64 = O.global_norm_ref(g, kinds)
        bound = (gamma_n(CHAIN) + len(part) * 2.0 ** -53) * ss64             # + the double sum of the partials
        print(f"  sumsq {ss:.9e} float64 {ss64:.9e} err {abs(ss - ss64):.3e} bound {bound:.3e}")
        assert abs(ss - ss64) <= bound
        assert abs(ss - part.astype(np.float64).sum()) <= len(part) * 2.0 ** -53 * ss, "the double sum of the device's own partials"
        assert abs(float(norm) - norm64) <= (gamma_n(CHAIN) + 2 * U) * norm64
        assert abs(float(scale) - 1.0 / norm64) <= (gamma_n(CHAIN) + 4 * U) / norm64 and scale < 1
        again = grad_finish(ar, g_in, slabd, kinds, 1.0)
        assert same_bits(again[0], g) and same_bits(again[1], part) and again[2] == ss and again[3] == norm and again[4] == scale


# ---- 2. cmoop_adamw ---------------------------------------------------------------------------------------------------------
def adamw(wd, gd, md, vd, kd, n, rec, alpha, lr, weight_decay=0.0, decay_mask=0, clipvalue=0.0):
    ok(L().cmoop_adamw(P(wd), P(gd), P(md), P(vd), P(kd), n, P(rec), alpha, lr, B1, B2, AEPS, weight_decay, decay_mask, clipvalue))


def test_adamw_wraps_the_grid_stride_loop():
    """2 112 000 elements: more than 2048 workgroups x 256 threads x 4 -- every element against the statement."""
    n = 2_112_000
    rs = np.random.RandomState(9)
    w, m, v = rs.randn(n).astype(np.float32), (0.1 * rs.randn(n)).astype(np.float32), (rs.rand(n) * 1e-2).astype(np.float32)
    g = R.adam_gradients(n, 10)
    kinds = rs.randint(0, 3, n).astype(np.uint8)
    wd, gd, md, vd, kd = dev(w), dev(g), dev(m), dev(v), dev(kinds)
    alpha, lr = R.keras_alpha(LR, B1, B2, 3), 0.5
    adamw(wd, gd, md, vd, kd, n, make_record(0.75), alpha, lr, weight_decay=0.1)
    w1, m1, v1 = O.adamw_step_ref(w, g, m, v, alpha, lr, B1, B2, AEPS, scale=0.75, weight_decay=0.1, kinds=kinds)
    for name, a, b in (("w", wd, w1), ("m", md, m1), ("v", vd, v1)):
        assert same_bits(host(a), b), name
    assert same_bits(host(gd), g), "the gradient is read only"


ADAMW_CASES = {
    "off": dict(),
    "decay, kernels": dict(weight_decay=0.05),
    "decay, every trainable tensor": dict(weight_decay=0.05, decay_mask=1),
    "norm clip": dict(clip=0.5),
    "value clip": dict(clipvalue=0.01),
    "decay + norm clip": dict(weight_decay=0.05, decay_mask=1, clip=0.25),
}


@pytest.mark.parametrize("guard", [4, 1])                 # 16-byte aligned operands (the float4 path) / odd offset (one element at a time)
@pytest.mark.parametrize("name", list(ADAMW_CASES))
def test_adamw_five_iterations_are_bit_equal_to_the_statement(name, guard):
    case = dict(ADAMW_CASES[name])
    clip_frac = case.pop("clip", 0.0)
    n = 2051                                                                  # n % 4 = 3: a scalar tail on the float4 path
    rs = np.random.RandomState(len(name) + guard)
    w = rs.randn(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    kinds = rs.randint(0, 3, n).astype(np.uint8)
    kinds[:8] = (0, 1, 2, 2, 1, 0, 2, 0)
    frozen = kinds == O.KIND_FROZEN
    m[frozen], v[frozen] = 0.25, 0.5                                          # planted: must come back untouched
    w0, m0, v0 = w.copy(), m.copy(), v.copy()

    def guarded(a, fill):
        t = torch.full((n + 2 * guard,), fill, device="cuda", dtype=torch.from_numpy(a).dtype)
        t[guard:guard + n] = dev(a)
        return t
    wt, mt, vt, kt = guarded(w, float("nan")), guarded(m, float("nan")), guarded(v, float("nan")), guarded(kinds, 2)
    ar = Arena([(n, 0)])
    for t in range(1, 6):
        g = R.adam_gradients(n, 30 + t)                                       # exact zeros and 1e-25 included
        assert (g == 0).any() and (g == np.float32(1e-25)).any() and (g[frozen] != 0).any(), "frozen slots carry planted gradients"
        gt = guarded(g, float("nan"))
        alpha, lr = R.keras_alpha(LR, B1, B2, t), LR * (1.0 - 0.1 * t)
        if clip_frac:
            _, norm64 = O.global_norm_ref(g, kinds)
            rec = make_record(-1.0)
            part, cnt = torch.empty(8, device="cuda"), C.c_int32()
            ok(L().cmoop_grad_finish(P(gt[guard:]), None, *ar.seg_args(), P(kt[guard:]), clip_frac * norm64, P(part), 8, C.byref(cnt), P(rec)))
            scale = read_record(rec)[2]
            assert 0 < scale < 1 and abs(float(scale) - clip_frac) <= 1e-5
        else:
            rec, scale = make_record(1.0), np.float32(1.0)
        adamw(wt[guard:], gt[guard:], mt[guard:], vt[guard:], kt[guard:], n, rec, alpha, lr, **case)
        w, m, v = O.adamw_step_ref(w, g, m, v, alpha, lr, B1, B2, AEPS, scale=scale, kinds=kinds, **case)
        for nm, a, b in (("w", wt, w), ("m", mt, m), ("v", vt, v)):
            out = host(a)
            assert np.isnan(out[:guard]).all() and np.isnan(out[guard + n:]).all(), (nm, "guards")
            assert same_bits(out[guard:guard + n], b), f"{name} iteration {t}: {nm}"
        assert same_bits(host(gt)[guard:guard + n], g)
    assert same_bits(w[frozen], w0[frozen]) and same_bits(m[frozen], m0[frozen]) and same_bits(v[frozen], v0[frozen])
    assert not same_bits(w[~frozen], w0[~frozen])


def test_adamw_with_everything_off_is_cmoop_adam():
    n = 1025
    rs = np.random.RandomState(4)
    w = rs.randn(n).astype(np.float32)
    a = [dev(w), dev(np.zeros(n, np.float32)), dev(np.zeros(n, np.float32))]
    b = [dev(w), dev(np.zeros(n, np.float32)), dev(np.zeros(n, np.float32))]
    for t in range(1, 6):
        gd = dev(R.adam_gradients(n, 60 + t))
        alpha = R.keras_alpha(LR, B1, B2, t)
        ok(L().cmoop_adam(P(a[0]), P(gd), P(a[1]), P(a[2]), n, alpha, B1, B2, AEPS))
        adamw(b[0], gd, b[1], b[2], None, n, make_record(1.0), alpha, LR)
        for x, y in zip(a, b):
            assert same_bits(host(x), host(y)), t


# ---- 3. the trainer ---------------------------------------------------------------------------------------------------------
T_, F_, CLASSES, BATCH, SEED = 21, 12, 4, 8, 1234
GENE = (16, 3, 1, 1, 1, 0)                                  # the smallest BatchNorm + residual gene
NETS = [(GENE, "A"), (GENE, "A_ds")]
CFG = EvalConfig(variant="A", classes=CLASSES, batch=BATCH, eval_batch=16, epochs=2, early_stop=False, shuffle=True)
SCHED = OptimConfig(schedule="cosine", warmup_steps=2, warmup_start=0.25, decay_steps=6, alpha=0.1)
FULL = dataclasses.replace(SCHED, weight_decay=0.05, global_clipnorm=0.05)
STEPS_B = (8, 5, 8, 5)                                      # full and partial batches


def cfg_of(variant, **over):
    return dataclasses.replace(CFG, variant=variant, **over)


@functools.lru_cache(maxsize=None)
def data(n=40):
    X, y = make_data(n, T_, F_, CLASSES, 7)
    return X, y


def state_equal(a, b, what):
    sa, sb = (a if isinstance(a, dict) else a.get_state()), (b if isinstance(b, dict) else b.get_state())
    assert (sa["iterations"], sa["steps"]) == (sb["iterations"], sb["steps"]), what
    for k in ("params", "m", "v"):
        assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k, int((bits(sa[k]) != bits(sb[k])).sum()))


def run_steps(net, Xd, yd, permd, Bs=STEPS_B[:3]):
    row0 = 0
    for B in Bs:
        net.train_step(Xd, yd, permd, row0=row0, B=B)
        row0 += B


def predicted(state, g, scale, opt, cfg, kinds):
    """The statement's next (params, m, v) from the state before the step, the step's gradient and the reported scale."""
    _, lr32, a32 = O.rates(opt, cfg.to_struct(), state["iterations"])
    return O.adamw_step_ref(state["params"], g, state["m"], state["v"], a32, lr32, B1, B2, AEPS, scale=scale, weight_decay=opt.weight_decay,
                            decay_mask=opt.decay_mask, clipvalue=opt.clipvalue, kinds=kinds)


@pytest.mark.parametrize("gene,variant", NETS)
def test_off_means_off_and_an_inactive_clip_is_the_fused_launch(gene, variant):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    permd = dev(np.random.RandomState(8).permutation(len(X)).astype(np.int32))
    cfg = cfg_of(variant)
    with NetSession(gene, cfg, T_, F_, SEED) as never, NetSession(gene, cfg, T_, F_, SEED) as none, \
            NetSession(gene, dataclasses.replace(cfg, optim=OptimConfig()), T_, F_, SEED) as default, \
            NetSession(gene, cfg, T_, F_, SEED) as huge:
        none.set_optim(None)
        huge.set_optim(OptimConfig(global_clipnorm=1e30))
        assert none.optim is None and default.optim is None and huge.optim is not None
        for net in (never, none, default, huge):
            run_steps(net, Xd, yd, permd)
        for name, net in (("set_optim(None)", none), ("default OptimConfig", default)):
            state_equal(never, net, name)
            assert net.optim_stats() == dict(sumsq=0.0, norm=0.0, scale=1.0, path=0), name
        assert never.optim_stats()["path"] == 0
        st = huge.optim_stats()
        assert st["path"] == 1 and st["scale"] == 1.0 and st["norm"] > 0
        state_equal(never, huge, "global_clipnorm = 1e30: the three launches against the fused one")
        assert np.array_equal(bits(never.get_grads()), bits(huge.get_grads()))


@pytest.mark.parametrize("gene,variant", NETS)
def test_active_options_follow_the_statement_step_by_step(gene, variant):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    permd = dev(np.random.RandomState(8).permutation(len(X)).astype(np.int32))
    cfg = cfg_of(variant)
    kinds = O.param_kinds(gene, G.VARIANT_NAMES[variant], CLASSES)
    frozen = kinds == O.KIND_FROZEN
    assert frozen.any()
    no_decay = dataclasses.replace(FULL, weight_decay=0.0)
    with NetSession(gene, dataclasses.replace(cfg, optim=FULL), T_, F_, SEED) as net, \
            NetSession(gene, dataclasses.replace(cfg, optim=no_decay), T_, F_, SEED) as twin:
        row0, clipped = 0, 0
        for B in STEPS_B:
            old = net.get_state()
            twin.set_state(old)
            net.train_step(Xd, yd, permd, row0=row0, B=B)
            twin.train_step(Xd, yd, permd, row0=row0, B=B)
            row0 += B
            g, st, new = net.get_grads(), net.optim_stats(), net.get_state()
            ss64, norm64 = O.global_norm_ref(g, kinds)
            print(f"\n  {variant} B={B}: norm {st['norm']:.6e} float64 {norm64:.6e} scale {st['scale']:.6f}")
            assert st["path"] == 1
            assert abs(st["sumsq"] - ss64) <= (gamma_n(CHAIN) + 1e-12) * ss64
            assert abs(st["norm"] - norm64) <= (gamma_n(CHAIN) + 2 * U) * norm64
            clipped += st["scale"] < 1.0
            if norm64 > FULL.global_clipnorm * (1 + 1e-5):
                assert st["scale"] < 1.0
            w1, m1, v1 = predicted(old, g, st["scale"], FULL, cfg, kinds)
            assert np.array_equal(bits(new["params"][~frozen]), bits(w1[~frozen])), int((bits(new["params"][~frozen]) != bits(w1[~frozen])).sum())
            assert np.array_equal(bits(new["m"]), bits(m1)) and np.array_equal(bits(new["v"]), bits(v1))
            # the moving statistics: moved by the forward pass only -- the same step with decay off leaves the same bits
            assert np.array_equal(bits(new["params"][frozen]), bits(twin.get_state()["params"][frozen]))
            assert not np.array_equal(bits(new["params"][frozen]), bits(old["params"][frozen]))
            assert not np.array_equal(bits(new["params"][~frozen]), bits(twin.get_state()["params"][~frozen])), "decay moves the weights"
        assert clipped >= 1, "the clip was active"


def test_run_epoch_equals_explicit_steps_and_a_late_set_optim():
    """Device state and rate tables (run_epoch) against host arguments (train_step), schedule + decay + clip on; then options
    set after two plain steps continue as the statement predicts."""
    X, y = data(37)                                          # 8, 8, 8, 8, 5 rows
    n = len(X)
    Xd, yd = dev(X), dev(y)
    cfg = dataclasses.replace(CFG, optim=FULL)
    with NetSession(GENE, cfg, T_, F_, SEED) as net, NetSession(GENE, cfg, T_, F_, SEED) as ref:
        for epoch in range(2):
            net.run_epoch(Xd, yd, epoch)
            permd = dev(epoch_permutation(SEED, epoch, n))
            for s in range(0, n, BATCH):
                ref.train_step(Xd, yd, permd, row0=s, B=min(BATCH, n - s))
            state_equal(net, ref, f"epoch {epoch}")
            assert net.optim_stats() == ref.optim_stats()
    kinds = O.param_kinds(GENE, 0, CLASSES)
    frozen = kinds == O.KIND_FROZEN
    permd = dev(np.random.RandomState(8).permutation(n).astype(np.int32))
    with NetSession(GENE, CFG, T_, F_, SEED) as net, NetSession(GENE, CFG, T_, F_, SEED) as plain:
        run_steps(net, Xd, yd, permd, (8, 8))
        run_steps(plain, Xd, yd, permd, (8, 8))
        state_equal(net, plain, "before set_optim")
        net.set_optim(FULL)
        for s in (2, 3):
            old = net.get_state()
            assert old["iterations"] == s
            net.train_step(Xd, yd, permd, row0=8 * s, B=8)
            st, new = net.optim_stats(), net.get_state()
            w1, m1, v1 = predicted(old, net.get_grads(), st["scale"], FULL, CFG, kinds)
            assert st["path"] == 1
            assert np.array_equal(bits(new["params"][~frozen]), bits(w1[~frozen])) and np.array_equal(bits(new["m"]), bits(m1))
        # and a late schedule alone, through the rebuilt table of a fit under way
        plain.run_epoch(Xd, yd, 0)
        plain.set_optim(SCHED)
        old = plain.get_state()
        plain.run_epoch(Xd, yd, 1)
        with NetSession(GENE, CFG, T_, F_, SEED) as ref:
            ref.set_state(old)
            ref.set_optim(SCHED)
            perm1 = dev(epoch_permutation(SEED, 1, n))
            for s in range(0, n, BATCH):
                ref.train_step(Xd, yd, perm1, row0=s, B=min(BATCH, n - s))
            state_equal(plain, ref, "schedule set between two epochs")
            assert plain.optim_stats()["path"] == 0


CW4 = (0.5, 0.75, 1.0, 1.25)
MIX_LOSS = LossConfig(mixup_alpha=0.2, mixup_p=0.5, label_smoothing=0.1, class_weight=CW4)
AUG = AugmentConfig(p=0.5, time_shift=3, time_masks=2, time_mask_max=4, freq_masks=2, freq_mask_max=3, noise_std=0.1)
KD = DistillConfig(alpha=0.7, temperature=4.0)


def test_composes_with_augment_loss_and_distill():
    """All four on: the same steps driven through the targets twins on a net that has only the optimiser options."""
    X, y = data()
    n = len(X)
    perm = np.random.RandomState(8).permutation(n).astype(np.int32)
    Xd, yd, permd = dev(X), dev(y), dev(perm)
    ztd = dev((2.0 * np.random.RandomState(21).randn(n, CLASSES)).astype(np.float32))
    with NetSession(GENE, dataclasses.replace(CFG, optim=FULL, augment=AUG, loss=MIX_LOSS, distill=KD), T_, F_, SEED) as net, \
            NetSession(GENE, dataclasses.replace(CFG, optim=FULL), T_, F_, SEED) as ref:
        net.set_distill(teacher_logits=ztd)
        row0 = 0
        for B in STEPS_B:
            step = net.get_state()["steps"]
            rows = perm[row0:row0 + B]
            Xa = A.augment_reference(X[rows], AUG, SEED, step)
            Xm = Ls.mixup_reference(Xa, MIX_LOSS, SEED, step)
            t, w, primary = Ls.soft_targets_reference(y[rows], MIX_LOSS, CLASSES, SEED, step)
            q = D.teacher_targets(ztd, KD.temperature, MIX_LOSS, SEED, step, idx=permd, row0=row0, B=B)
            net.train_step(Xd, yd, permd, row0=row0, B=B)
            ref.train_step_distill_targets(dev(Xm), dev(t), q, KD.alpha, KD.temperature, w=dev(w), primary=dev(primary))
            row0 += B
            state_equal(net, ref, ("composition", step))
            assert np.array_equal(bits(net.get_grads()), bits(ref.get_grads())) and net.optim_stats() == ref.optim_stats()
            assert net.optim_stats()["path"] == 1


# ---- 4. the population path --------------------------------------------------------------------------------------------------
POP = [(16, 3, 1, 1, 1, 0), (16, 3, 1, 1, 1, 1), (16, 5, 0, 1, 2, 0), (16, 3, 1, 2, 1, 0)]


def test_population_path_matches_session_fit_and_train_model():
    Xtr, ytr, Xva, yva = make_split(40, 16, T_, F_, CLASSES, 31)
    pop = [G.gene_to_hparams(g) for g in POP]
    spe = 5
    opt = OptimConfig.cosine(2, 1, spe, warmup_start=0.1, weight_decay=0.02, global_clipnorm=0.5)
    base = dataclasses.replace(CFG, optim=opt, seed=5)
    results = []
    for slots in (1, 4, 4):
        ev = PopulationEvaluator(Xtr, ytr, Xva, yva, dataclasses.replace(base, n_slots=slots))
        res = ev.compute_objectives_and_constraints(pop)
        results.append(([r["objs"] for r in res], list(ev.last_epochs_run), list(ev.last_seeds)))
    assert results[0] == results[1] == results[2], "n_slots 1 and 4, and two calls"
    objs, epochs_run, seeds = results[2]
    assert epochs_run == [2] * 4
    for g, o, sd in zip(POP, objs, seeds):
        with NetSession(g, base, T_, F_, sd) as net:
            r = net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
            assert net.optim_stats()["path"] == 1
        assert (r["acc"], r["fpr"], r["epochs_run"]) == (-o[0], o[2], 2), (g, r, o)
    on = ev.train_model(POP[0], seeds[0])
    assert (on.objectives["acc"], on.objectives["fpr"]) == (-objs[0][0], objs[0][2])
    off = PopulationEvaluator(Xtr, ytr, Xva, yva, dataclasses.replace(base, optim=None)).train_model(POP[0], seeds[0])
    assert on.params.shape == off.params.shape and not np.array_equal(on.params, off.params)


def test_population_call_without_optim_is_the_kd_call():
    Xtr, ytr, Xva, yva = make_split(40, 16, T_, F_, CLASSES, 31)
    base = dataclasses.replace(CFG, seed=5, n_slots=2, loss=LossConfig(label_smoothing=0.1))
    ev = PopulationEvaluator(Xtr, ytr, Xva, yva, base)
    genes = np.ascontiguousarray(np.array(POP[:2], np.int32))
    seeds = np.array([5, 6], np.uint32)
    cfg, ds, loss = base.to_struct(), ev._dataset(), base.loss_struct()
    off = OptimConfig()._struct()
    out = []
    for call in ("kd", "opt_null", "opt_disabled", "opt_on"):
        acc, size, fpr, vl = (np.zeros(2, np.float64) for _ in range(4))
        ep = np.zeros(2, np.int32)
        tail = (C.byref(ds), P(genes), P(seeds), C.c_int32(2), None, None, P(acc), P(size), P(fpr), P(ep), P(vl), None, None)
        torch.cuda.synchronize()
        if call == "kd":
            _lib.check(L().cmoop_eval_population_kd(C.byref(cfg), None, C.byref(loss), None, *tail))
        else:
            st = {"opt_null": None, "opt_disabled": off, "opt_on": FULL._struct()}[call]
            _lib.check(L().cmoop_eval_population_opt(C.byref(cfg), None, C.byref(loss), None, C.byref(st) if st is not None else None, *tail))
        out.append(tuple(a.tobytes() for a in (acc, size, fpr, ep, vl)))
    assert out[0] == out[1] == out[2]
    assert out[3][4] != out[0][4], "enabled options change the fit"
    assert ev.config.optim_struct() is None
    bad = OptimConfig(global_clipnorm=1.0)._struct()
    bad.clipvalue = 1.0
    with pytest.raises(_lib.CmoopError, match="both"):
        _lib.check(L().cmoop_eval_population_opt(C.byref(cfg), None, None, None, C.byref(bad), *tail))


# ---- 5. inference ------------------------------------------------------------------------------------------------------------
def test_inference_is_untouched():
    X, y = data()
    Xd, yd = dev(X), dev(y)
    with NetSession(GENE, dataclasses.replace(CFG, optim=FULL), T_, F_, SEED) as net, NetSession(GENE, CFG, T_, F_, SEED) as ref:
        run_steps(net, Xd, yd, None, (8, 8))
        ref.set_state(net.get_state())
        la, aa, pa = net.evaluate(Xd, yd)
        lr, ar, pr = ref.evaluate(Xd, yd)
        assert (la, aa) == (lr, ar) and torch.equal(pa, pr)
        assert torch.equal(net.predict_proba(Xd), ref.predict_proba(Xd))
