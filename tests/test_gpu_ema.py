"""GPU: weight EMA.  The kernel alone (``cmoop_ema_update``) against ``ema.ema_step_ref``, and the trainer: the average only
observes (the training trajectory keeps its bits on all three optimiser paths), follows the statement step by step on both
step paths, off means off, inference on the average, the fit (validation, early stopping, snapshot, read-outs and the
end-of-fit overwrite all on the average), the population call, deployment, and composition with the four other options.
Everything is compared bit for bit: the arithmetic is three separately rounded fp32 operations, or a copy."""
import ctypes as C
import dataclasses
import functools
import itertools
import threading

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import (AugmentConfig, DistillConfig, EmaConfig, EvalConfig, LossConfig, OptimConfig,
                                        PopulationEvaluator, _lib, calculate_fpr, genes as G)
from cmoop_audio_processing_amd import ema as E
from cmoop_audio_processing_amd import optim as O
from cmoop_audio_processing_amd.session import NetSession, epoch_permutation
from test_gpu_net import make_data, make_split

pytestmark = pytest.mark.gpu

P = _lib.ptr


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


# ---- 1. the kernel -----------------------------------------------------------------------------------------------------------
def ema_update(cfg, i, a, w, kinds, n):
    st = cfg._struct()
    ok(L().cmoop_ema_update(C.byref(st), i, P(a), P(w), P(kinds), n))


def edge_weights(n, seed):
    """Random weights with the edge values mixed in: exact zeros, -0.0, 1e-25 (its products underflow) and 3e38."""
    rs = np.random.RandomState(seed)
    w = (rs.randn(n) * 10.0 ** rs.uniform(-4, 1, n)).astype(np.float32)
    w[rs.rand(n) < 0.1] = 0.0
    w[rs.rand(n) < 0.05] = -0.0
    w[rs.rand(n) < 0.05] = np.float32(1e-25)
    w[rs.rand(n) < 0.02] = np.float32(3e38)
    if n >= 8:
        w[:8] = np.array([0.0, -0.0, 1e-25, 3e38, -3e38, 1.0, -0.0, 0.0], np.float32)
    return w


@pytest.mark.parametrize("guard", [4, 1])                 # 16-byte aligned operands (the float4 path) / odd offset (one element at a time)
def test_five_iterations_are_bit_equal_to_the_statement(guard):
    n = 2051                                                                  # n % 4 = 3: a scalar tail on the float4 path
    rs = np.random.RandomState(40 + guard)
    a = rs.randn(n).astype(np.float32)
    a[8:12] = np.array([0.0, -0.0, -0.0, 0.0], np.float32)
    kinds = rs.randint(0, 3, n).astype(np.uint8)
    kinds[:8] = (0, 1, 2, 2, 1, 0, 2, 0)
    kinds[8:12] = 0
    frozen = kinds == O.KIND_FROZEN
    cfg = EmaConfig(0.99, warmup=True)

    def guarded(x, fill):
        t = torch.full((n + 2 * guard,), fill, device="cuda", dtype=torch.from_numpy(x).dtype)
        t[guard:guard + n] = dev(x)
        return t
    at, kt = guarded(a, float("nan")), guarded(kinds, 2)
    seen = set()
    for i in range(5):
        w = edge_weights(n, 70 + i)
        w[8:12] = np.array([-0.0, -0.0, 0.0, 0.0], np.float32)                # every sign pair of two zeros
        for v in (0.0, 1e-25, 3e38):
            assert (w == np.float32(v)).any()
        assert (np.signbit(w) & (w == 0)).any(), "-0.0 among the weights"
        wt = guarded(w, float("nan"))
        w_before = host(wt).copy()
        _, mf, omf = E.rates(cfg, i)
        seen.add((float(mf), float(omf)))
        ema_update(cfg, i, at[guard:], wt[guard:], kt[guard:], n)
        a = E.ema_step_ref(a, w, mf, omf, kinds)
        out = host(at)
        assert np.isnan(out[:guard]).all() and np.isnan(out[guard + n:]).all(), "the guards of a"
        assert same_bits(out[guard:guard + n], a), f"iteration {i}: {int((bits(out[guard:guard + n]) != bits(a)).sum())} elements differ"
        assert same_bits(out[guard:guard + n][frozen], w[frozen]), "kind 2: w's bits"
        assert np.array_equal(bits(host(wt)), bits(w_before)), "w, guards included, is read only"
        assert np.array_equal(host(kt), np.concatenate([np.full(guard, 2, np.uint8), kinds, np.full(guard, 2, np.uint8)]))
    assert len(seen) == 5, "five different (mf, omf)"


@pytest.mark.parametrize("n", [1, 3, 4, 5])
def test_tiny_arenas_without_kinds(n):
    rs = np.random.RandomState(n)
    a, w = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    at, wt = torch.full((n + 4,), float("nan"), device="cuda"), dev(w)
    at[:n] = dev(a)
    cfg = EmaConfig(0.9)
    for i in range(2):
        ema_update(cfg, i, at, wt, None, n)
        a = E.ema_step_ref(a, w, *E.rates(cfg, i)[1:])
    out = host(at)
    assert same_bits(out[:n], a) and np.isnan(out[n:]).all()
    assert same_bits(host(wt), w)


def test_wraps_the_grid_stride_loop():
    """2 112 000 elements: more than 2048 workgroups x 256 threads x 4 -- every element against the statement."""
    n = 2_112_000
    rs = np.random.RandomState(9)
    a, w = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    kinds = rs.randint(0, 3, n).astype(np.uint8)
    at, wt, kt = dev(a), dev(w), dev(kinds)
    cfg = EmaConfig(0.999)
    ema_update(cfg, 3, at, wt, kt, n)
    want = E.ema_step_ref(a, w, *E.rates(cfg, 3)[1:], kinds)
    assert same_bits(host(at), want)
    assert same_bits(host(wt), w) and np.array_equal(host(kt), kinds)
    assert not same_bits(want, a)


def test_update_refuses_a_bad_config_before_launching():
    at, wt = dev(np.ones(4, np.float32)), dev(np.zeros(4, np.float32))
    st = EmaConfig(0.9)._struct()
    st.warmup = 3
    assert L().cmoop_ema_update(C.byref(st), 0, P(at), P(wt), None, 4) != 0 and b"warmup" in L().cmoop_last_error()
    st.warmup = 0
    assert L().cmoop_ema_update(C.byref(st), 0, P(at), P(at), None, 4) != 0, "in place is refused"
    assert L().cmoop_ema_update(C.byref(st), -1, P(at), P(wt), None, 4) != 0
    torch.cuda.synchronize()
    assert same_bits(host(at), np.ones(4, np.float32))


# ---- 2. the trainer ----------------------------------------------------------------------------------------------------------
T_, F_, CLASSES, BATCH, SEED = 21, 12, 4, 16, 1234
GENE_BN, GENE_FC = (16, 3, 1, 1, 1, 0), (16, 3, 0, 1, 2, 1)      # BatchNorm (kind-2 slots exist) / two dense layers with dropout
NETS = [(GENE_BN, "A"), (GENE_BN, "B_ds"), (GENE_FC, "A"), (GENE_FC, "B_ds")]
CFG = EvalConfig(variant="A", classes=CLASSES, batch=BATCH, eval_batch=32, epochs=2, early_stop=False, shuffle=True)
EMA = EmaConfig(0.99)
WARM = EmaConfig(0.99, warmup=True)
FINISH = OptimConfig(weight_decay=1e-2, global_clipnorm=1.0)
STEPS_B = (16, 16, 16, 16, 16, 11)                          # the last one a partial batch
N_ROWS = sum(STEPS_B)


def cfg_of(variant, **over):
    return dataclasses.replace(CFG, variant=variant, **over)


@functools.lru_cache(maxsize=None)
def data(n=N_ROWS):
    return make_data(n, T_, F_, CLASSES, 7)


def state_equal(a, b, what, params=True):
    sa, sb = (a if isinstance(a, dict) else a.get_state()), (b if isinstance(b, dict) else b.get_state())
    assert (sa["iterations"], sa["steps"]) == (sb["iterations"], sb["steps"]), what
    for k in ("params", "m", "v") if params else ("m", "v"):
        assert np.array_equal(bits(sa[k]), bits(sb[k])), (what, k, int((bits(sa[k]) != bits(sb[k])).sum()))


def explicit_epoch(net, Xd, yd, epoch, n, after_step=None):
    permd = dev(epoch_permutation(SEED, epoch, n))
    for s in range(0, n, BATCH):
        net.train_step(Xd, yd, permd, row0=s, B=min(BATCH, n - s))
        if after_step:
            after_step()


PATHS = [(g, v, "fused") for g, v in NETS] + [(GENE_BN, "A", "finish"), (GENE_FC, "B_ds", "finish"), (GENE_BN, "B_ds", "unfused"),
                                              (GENE_FC, "A", "unfused")]


@pytest.mark.parametrize("gene,variant,path", PATHS)
def test_the_average_only_observes_and_follows_the_statement(gene, variant, path, monkeypatch):
    """Two nets on one seed, one with the average: after every step the average is the host-advanced one, and w, m, v, the
    counters and the train metrics keep the bits of the net without it -- on the fused optimiser launch, the finish + update
    path and the un-fused A/B knob."""
    if path == "unfused":
        monkeypatch.setenv("CMOOP_ADAM_UNFUSED", "1")
    X, y = data()
    Xd, yd = dev(X), dev(y)
    permd = dev(np.random.RandomState(8).permutation(len(X)).astype(np.int32))
    cfg = cfg_of(variant, optim=FINISH if path == "finish" else None)
    kinds = O.param_kinds(gene, G.VARIANT_NAMES[variant], CLASSES)
    assert np.array_equal(kinds, O.param_kinds_lib(gene, G.VARIANT_NAMES[variant], CLASSES))
    frozen = kinds == O.KIND_FROZEN
    assert frozen.any() == bool(gene[2])
    with NetSession(gene, cfg, T_, F_, SEED) as plain, NetSession(gene, dataclasses.replace(cfg, ema=EMA), T_, F_, SEED) as net:
        assert net.ema == EMA and plain.ema is None
        a = net.get_ema()
        assert same_bits(a, net.get_params()), "the average starts as a bit copy of the parameter arena"
        row0 = 0
        for i, B in enumerate(STEPS_B):
            plain.train_step(Xd, yd, permd, row0=row0, B=B)
            net.train_step(Xd, yd, permd, row0=row0, B=B)
            row0 += B
            w = net.get_params()
            a = E.ema_step_ref(a, w, *E.rates(EMA, i)[1:], kinds)
            got = net.get_ema()
            assert same_bits(got, a), (path, i, int((bits(got) != bits(a)).sum()))
            assert same_bits(got[frozen], w[frozen]), "kind-2 slots carry w's bits"
            assert not same_bits(got[~frozen], w[~frozen])
            assert net.optim_stats()["path"] == (1 if path == "finish" else 0)
        state_equal(plain, net, path)
        assert np.array_equal(bits(plain.get_grads()), bits(net.get_grads()))
        assert plain.train_metrics() == net.train_metrics()


def test_run_epoch_equals_explicit_steps_and_a_late_set_ema():
    """Device state and the rate table (run_epoch) against host arguments (train_step), warm-up on; then an average set after
    one epoch starts as the copy of that moment and its warm-up is indexed by the absolute iteration."""
    X, y = data()
    n = len(X)
    Xd, yd = dev(X), dev(y)
    cfg = dataclasses.replace(CFG, ema=WARM)
    with NetSession(GENE_BN, cfg, T_, F_, SEED) as net, NetSession(GENE_BN, cfg, T_, F_, SEED) as ref:
        for epoch in range(2):
            net.run_epoch(Xd, yd, epoch)
            explicit_epoch(ref, Xd, yd, epoch, n)
            state_equal(net, ref, f"epoch {epoch}")
            assert same_bits(net.get_ema(), ref.get_ema()), f"epoch {epoch}"
    kinds = O.param_kinds(GENE_BN, 0, CLASSES)
    with NetSession(GENE_BN, CFG, T_, F_, SEED) as late, NetSession(GENE_BN, CFG, T_, F_, SEED) as ref:
        late.run_epoch(Xd, yd, 0)
        explicit_epoch(ref, Xd, yd, 0, n)
        state_equal(late, ref, "before set_ema")
        late.set_ema(WARM)
        ref.set_ema(WARM)
        stmt = [late.get_params()]
        assert same_bits(late.get_ema(), stmt[0]) and same_bits(ref.get_ema(), stmt[0]), "the copy of that moment"
        i0 = late.get_state()["iterations"]
        assert i0 == len(STEPS_B)

        def advance():
            i = ref.get_state()["iterations"] - 1
            stmt[0] = E.ema_step_ref(stmt[0], ref.get_params(), *E.rates(WARM, i)[1:], kinds)
        late.run_epoch(Xd, yd, 1)
        explicit_epoch(ref, Xd, yd, 1, n, after_step=advance)
        state_equal(late, ref, "after the late set_ema")
        assert same_bits(ref.get_ema(), stmt[0]), "the warm-up is indexed by the absolute iteration"
        assert same_bits(late.get_ema(), stmt[0])
        assert E.rates(WARM, i0)[1] != E.rates(WARM, 0)[1]
        # setting a config again keeps the average
        late.set_ema(EmaConfig(0.5))
        assert same_bits(late.get_ema(), stmt[0])


def test_targets_steps_advance_the_average():
    """train_step_targets / train_step_distill_targets end in the same optimiser tail: the average follows them too, and the
    trajectory keeps the bits of a net without it."""
    X, y = data()
    rs = np.random.RandomState(5)
    kinds = O.param_kinds(GENE_BN, 0, CLASSES)
    with NetSession(GENE_BN, dataclasses.replace(CFG, ema=WARM), T_, F_, SEED) as net, NetSession(GENE_BN, CFG, T_, F_, SEED) as plain:
        a = net.get_ema()
        for i, B in enumerate((16, 11, 16)):
            rows = dev(X[i * 16:i * 16 + B])
            t = dev(np.eye(CLASSES, dtype=np.float32)[y[i * 16:i * 16 + B]])
            q = dev(rs.dirichlet(np.ones(CLASSES), B).astype(np.float32))
            for n in (net, plain):
                if i == 1:
                    n.train_step_distill_targets(rows, t, q, 0.7, 4.0)
                else:
                    n.train_step_targets(rows, t)
            a = E.ema_step_ref(a, net.get_params(), *E.rates(WARM, i)[1:], kinds)
            assert same_bits(net.get_ema(), a), i
        state_equal(net, plain, "targets steps")


def test_off_means_off():
    X, y = data()
    Xd, yd = dev(X), dev(y)
    permd = dev(np.random.RandomState(8).permutation(len(X)).astype(np.int32))
    with NetSession(GENE_BN, CFG, T_, F_, SEED) as never, NetSession(GENE_BN, CFG, T_, F_, SEED) as none, \
            NetSession(GENE_BN, dataclasses.replace(CFG, ema=EmaConfig(momentum=0.0)), T_, F_, SEED) as zero:
        none.set_ema(None)
        assert none.ema is None and zero.ema is None
        row0 = 0
        for B in STEPS_B[-3:]:
            for net in (never, none, zero):
                net.train_step(Xd, yd, permd, row0=row0, B=B)
            row0 += B
        for name, net in (("set_ema(None)", none), ("EmaConfig(momentum=0)", zero)):
            state_equal(never, net, name)
            assert never.train_metrics(reset=False) == net.train_metrics(reset=False)
            for call in (net.get_ema, lambda: net.use_ema(True), net.finalize_ema, lambda: net.set_ema_params(np.zeros(net.n_params, np.float32))):
                with pytest.raises(_lib.CmoopError, match="no average"):
                    call()
        with pytest.raises(ValueError, match="momentum"):
            none.set_ema(EmaConfig(1.0))
        # on, then off: the average exists and is no longer advanced
        none.set_ema(EMA)
        none.train_step(Xd, yd, permd, row0=0, B=BATCH)
        a = none.get_ema()
        none.set_ema(None)
        none.train_step(Xd, yd, permd, row0=BATCH, B=BATCH)
        never.train_step(Xd, yd, permd, row0=0, B=BATCH)
        never.train_step(Xd, yd, permd, row0=BATCH, B=BATCH)
        assert same_bits(none.get_ema(), a)
        state_equal(never, none, "on, then off")


@pytest.mark.parametrize("gene,variant", [(GENE_BN, "A"), (GENE_FC, "B_ds")])
def test_inference_on_the_average(gene, variant):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    permd = dev(np.random.RandomState(8).permutation(len(X)).astype(np.int32))
    cfg = cfg_of(variant)
    on_cfg = dataclasses.replace(cfg, ema=EmaConfig(0.9))

    def same_inference(a, b, what, equal=True):
        (la, aa, pa), (lb, ab, pb) = a.evaluate(Xd, yd), b.evaluate(Xd, yd)
        feat = Xd[:4].reshape(-1, F_).contiguous()           # a stream of 4 T frames: windows at hop 7
        checks = [(la, aa) == (lb, ab) and torch.equal(pa, pb), torch.equal(a.predict_proba(Xd), b.predict_proba(Xd)),
                  torch.equal(a.predict_logits(Xd), b.predict_logits(Xd)), torch.equal(a.predict_stream(feat, 7), b.predict_stream(feat, 7))]
        assert all(checks) if equal else not checks[2], (what, checks)
    with NetSession(gene, on_cfg, T_, F_, SEED) as net, NetSession(gene, on_cfg, T_, F_, SEED) as twin, \
            NetSession(gene, cfg, T_, F_, SEED) as avg, NetSession(gene, cfg, T_, F_, SEED) as raw:
        row0 = 0
        for B in STEPS_B[:4]:
            net.train_step(Xd, yd, permd, row0=row0, B=B)
            twin.train_step(Xd, yd, permd, row0=row0, B=B)
            row0 += B
        avg.set_params(net.get_ema())
        raw.set_params(net.get_params())
        same_inference(net, raw, "before the switch")
        net.use_ema(True)
        same_inference(net, avg, "use_ema(1)")
        same_inference(net, raw, "the average is another net", equal=False)
        assert same_bits(net.get_params(), raw.get_params()), "get_params stays the raw parameters"
        with pytest.raises(_lib.CmoopError, match="use_average"):
            net.train_step(Xd, yd, permd, row0=row0, B=BATCH)
        state_equal(net, twin, "a refused step enqueues nothing")
        net.use_ema(False)
        same_inference(net, raw, "use_ema(0)")
        net.train_step(Xd, yd, permd, row0=row0, B=BATCH)
        twin.train_step(Xd, yd, permd, row0=row0, B=BATCH)
        state_equal(net, twin, "a step after the detour")
        assert same_bits(net.get_ema(), twin.get_ema())
        # finalize: w := a; set_state leaves the average alone, set_ema_params writes it
        a = net.get_ema()
        net.finalize_ema()
        assert same_bits(net.get_params(), a) and same_bits(net.get_ema(), a)
        state_equal(net, twin, "finalize keeps the moments and the counters", params=False)
        net.set_state(twin.get_state())
        assert same_bits(net.get_ema(), a) and same_bits(net.get_params(), twin.get_params())
        net.set_ema_params(raw.get_params())
        assert same_bits(net.get_ema(), raw.get_params())


# ---- 3. the fit ----------------------------------------------------------------------------------------------------------------
N_TRAIN, N_VAL = 96, 64            # 64: sums over the validation split divide exactly
FIT = dataclasses.replace(CFG, epochs=8, early_stop=True, patience=2, acc_readout="evaluate", fpr_variant="v1", ema=EmaConfig(0.7))


@functools.lru_cache(maxsize=None)
def split():
    return make_split(N_TRAIN, N_VAL, T_, F_, CLASSES, 31, noise=2.5, label_noise=0.3)      # noisy: the validation loss turns early


def keras_early_stopping(val_loss, patience):
    """(epochs_run, best_epoch) of EarlyStopping(monitor='val_loss', patience) over a history that may run on."""
    best, wait, best_epoch = np.inf, 0, -1
    for e, vl in enumerate(val_loss):
        wait += 1
        if vl < best:
            best, best_epoch, wait = vl, e, 0
        elif wait >= patience and e > 0:
            return e + 1, best_epoch
    return len(val_loss), best_epoch


@pytest.mark.parametrize("restore_best", [False, True])
def test_fit_validates_stops_and_reads_out_on_the_average(restore_best):
    Xtr, ytr, Xva, yva = (dev(a) for a in split())
    cfg = dataclasses.replace(FIT, restore_best=restore_best)
    with NetSession(GENE_BN, cfg, T_, F_, SEED) as net, NetSession(GENE_BN, cfg, T_, F_, SEED) as twin, \
            NetSession(GENE_BN, dataclasses.replace(cfg, ema=None), T_, F_, SEED) as judge:
        r = net.fit(Xtr, ytr, Xva, yva)
        hist_l, hist_a, avgs, raw_l = [], [], [], []
        for epoch in range(r["epochs_run"]):
            twin.run_epoch(Xtr, ytr, epoch)
            raw_l.append(twin.evaluate(Xva, yva)[0])
            twin.use_ema(True)
            loss, acc, _ = twin.evaluate(Xva, yva)
            twin.use_ema(False)
            hist_l.append(loss); hist_a.append(acc); avgs.append(twin.get_ema())
        print(f"\n  restore_best={restore_best}: val_loss on the average {hist_l}\n  on the raw weights {raw_l}")
        assert r["val_loss_history"].tolist() == hist_l and r["val_accuracy_history"].tolist() == hist_a
        assert hist_l != raw_l, "the history is that of the average, not of the raw weights"
        epochs_run, best_epoch = keras_early_stopping(hist_l, cfg.patience)
        assert (r["epochs_run"], r["best_epoch"]) == (epochs_run, best_epoch)
        if epochs_run < cfg.epochs:      # stopped early: one more epoch would not have been run
            assert keras_early_stopping(hist_l[:-1], cfg.patience)[0] == epochs_run - 1
        assert epochs_run < cfg.epochs and best_epoch < epochs_run - 1, "this split stops early, past its best epoch"
        readout = best_epoch if restore_best else epochs_run - 1
        final = net.get_params()
        assert same_bits(final, avgs[readout]), "the parameters are the weights that were read out"
        assert same_bits(net.get_ema(), avgs[-1]), "the average itself is left as it is"
        state_equal(net, twin, "Adam's moments and the counters", params=False)
        judge.set_params(final)
        loss, acc, preds = judge.evaluate(Xva, yva)
        assert (r["val_loss"], r["acc"]) == (loss, acc)
        assert r["fpr"] == calculate_fpr(host(yva), host(preds), CLASSES, "v1")
        assert (loss, acc) == (hist_l[readout], hist_a[readout])


def test_fit_with_last_epoch_readout_reuses_the_last_validation_pass():
    """acc_readout 'last', no early stopping: the last validation pass IS the read-out pass, and it ran on the average the
    parameters are then overwritten with."""
    Xtr, ytr, Xva, yva = (dev(a) for a in split())
    cfg = dataclasses.replace(FIT, epochs=3, early_stop=False, acc_readout="last", ema=WARM)
    with NetSession(GENE_FC, cfg, T_, F_, SEED) as net, NetSession(GENE_FC, dataclasses.replace(cfg, ema=None), T_, F_, SEED) as judge:
        r = net.fit(Xtr, ytr, Xva, yva)
        assert r["epochs_run"] == 3
        assert same_bits(net.get_params(), net.get_ema())
        judge.set_params(net.get_params())
        loss, acc, preds = judge.evaluate(Xva, yva)
        assert (r["val_loss"], r["acc"]) == (loss, acc) == (r["val_loss_history"][-1], r["val_accuracy_history"][-1])
        assert r["fpr"] == calculate_fpr(host(yva), host(preds), CLASSES, "v1")


# ---- 4. the population call and deployment -------------------------------------------------------------------------------------
POP = [GENE_BN, GENE_FC]
SEEDS = [5, 6]
POP_CFG = dataclasses.replace(FIT, restore_best=True, seed=SEEDS[0], n_slots=2)


def ref(st):
    return C.byref(st) if st is not None else None


def population(ev, cfg, structs, symbol="_avg", pull=None):
    """One direct call of cmoop_eval_population_avg (five option structs) or _opt (four) -> the bytes of (acc, size_mb, fpr,
    epochs_run, val_loss)."""
    n = len(POP)
    genes, seeds = np.ascontiguousarray(np.array(POP, np.int32)), np.array(SEEDS, np.uint32)
    acc, size, fpr, vl = (np.zeros(n, np.float64) for _ in range(4))
    ep, done = np.zeros(n, np.int32), np.zeros(n, np.int32)
    c, ds = cfg.to_struct(), ev._dataset()
    assert len(structs) == {"_avg": 5, "_opt": 4}[symbol]
    cb = _lib.NEXT_FN(lambda _ctx: pull()) if pull is not None else None
    torch.cuda.synchronize()
    _lib.check(getattr(L(), "cmoop_eval_population" + symbol)(
        C.byref(c), *(ref(s) for s in structs), C.byref(ds), P(genes), P(seeds), C.c_int32(n), C.cast(cb, C.c_void_p) if cb is not None else None,
        None, P(acc), P(size), P(fpr), P(ep), P(vl), None, P(done) if cb is not None else None))
    if pull is not None:
        assert done.tolist() == [1] * n
    return tuple(a.tobytes() for a in (acc, size, fpr, ep, vl))


def index_pull(order):
    ctr, lock = itertools.count(), threading.Lock()

    def pull():
        with lock:
            j = next(ctr)
        return order[j] if j < len(order) else -1
    return pull


def test_population_call_matches_the_session_fit_and_train_model():
    ev = PopulationEvaluator(*split(), POP_CFG)
    st = POP_CFG.ema_struct()
    assert POP_CFG.option_structs(T_, F_, None, N_TRAIN) == (None, None, None, None) and st is not None
    none4 = (None, None, None, None)
    direct = population(ev, POP_CFG, none4 + (st,))
    assert population(ev, POP_CFG, none4 + (st,), pull=index_pull([1, 0])) == direct
    with NetSession(POP[0], POP_CFG, T_, F_, SEEDS[0]) as net:
        r = net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
        final = net.get_params()
    acc, fpr, ep, vl = (np.frombuffer(direct[k], dt)[0] for k, dt in ((0, np.float64), (2, np.float64), (3, np.int32), (4, np.float64)))
    assert (r["acc"], r["fpr"], r["epochs_run"], r["val_loss"]) == (acc, fpr, ep, vl)
    # NULL or a disabled struct: the bytes of cmoop_eval_population_opt
    off = population(ev, POP_CFG, none4, symbol="_opt")
    assert population(ev, POP_CFG, none4 + (None,)) == off
    assert population(ev, POP_CFG, none4 + (EmaConfig()._struct(),)) == off
    assert population(ev, POP_CFG, none4 + (EmaConfig()._struct(),), pull=index_pull([0, 1])) == off
    assert direct[4] != off[4], "the average changes the fit's read-outs"
    bad = EmaConfig(0.9)._struct()
    bad.reserved = 1
    with pytest.raises(_lib.CmoopError, match="reserved"):
        population(ev, POP_CFG, none4 + (bad,))
    # the evaluator takes the same route
    rows = ev.evaluate_genes(POP, SEEDS)
    assert tuple(np.ascontiguousarray(rows[:, k]).tobytes() for k in range(3)) + (rows[:, 3].astype(np.int32).tobytes(),) == direct[:4]
    rows_off = PopulationEvaluator(*split(), dataclasses.replace(POP_CFG, ema=EmaConfig())).evaluate_genes(POP, SEEDS)
    assert tuple(np.ascontiguousarray(rows_off[:, k]).tobytes() for k in range(3)) == off[:3]
    # deployment: train_model needs nothing but the option -- its parameters are the finalised ones, and predicting with them
    # reproduces the reported accuracy
    tm = ev.train_model(POP[0], SEEDS[0])
    assert same_bits(tm.params, final)
    assert (tm.objectives["acc"], tm.objectives["fpr"], tm.objectives["epochs_run"]) == (acc, fpr, ep)
    with tm.session(dataclasses.replace(POP_CFG, ema=None)) as scorer:
        pred = scorer.predict_proba(ev.X_val).argmax(dim=1).to(torch.int32)
    assert float((pred == ev.y_val).sum().item()) / N_VAL == acc


def test_composes_with_the_four_other_options_by_every_route():
    """Augment, loss, distill, optim and ema all on: the direct call, the evaluator and a session from the same config agree."""
    teacher = torch.from_numpy((2.0 * np.random.RandomState(21).randn(N_TRAIN, CLASSES)).astype(np.float32)).cuda()
    optim = OptimConfig(schedule="cosine", warmup_steps=2, warmup_start=0.25, decay_steps=10, alpha=0.1, weight_decay=0.05,
                        global_clipnorm=0.05)
    four = dataclasses.replace(POP_CFG, epochs=2, early_stop=False, restore_best=False, acc_readout="last", ema=None,
                               augment=AugmentConfig(time_shift=3), loss=LossConfig(label_smoothing=0.1),
                               distill=DistillConfig(alpha=0.7, temperature=4.0), optim=optim)
    on = dataclasses.replace(four, ema=WARM)
    ev = PopulationEvaluator(*split(), on)
    ev.set_teacher(teacher)
    structs = on.option_structs(T_, F_, teacher, N_TRAIN)
    assert len(structs) == 4 and all(s is not None for s in structs)
    direct = population(ev, on, structs + (on.ema_struct(),))
    assert population(ev, on, structs + (on.ema_struct(),), pull=index_pull([0, 1])) == direct
    without = population(ev, four, structs + (None,))
    assert without == population(ev, four, structs, symbol="_opt")
    assert direct[4] != without[4], "the average changes the read-outs of the same four-option fit"
    rows = ev.evaluate_genes(POP, SEEDS)
    assert tuple(np.ascontiguousarray(rows[:, k]).tobytes() for k in range(3)) + (rows[:, 3].astype(np.int32).tobytes(),) == direct[:4]
    with NetSession(POP[0], on, T_, F_, SEEDS[0]) as net:
        net.set_distill(teacher_logits=teacher)
        r = net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
        assert net.optim_stats()["path"] == 1 and net.ema == WARM
        assert same_bits(net.get_params(), net.get_ema())
    acc, fpr, ep, vl = (np.frombuffer(direct[k], dt)[0] for k, dt in ((0, np.float64), (2, np.float64), (3, np.int32), (4, np.float64)))
    assert (r["acc"], r["fpr"], r["epochs_run"], r["val_loss"]) == (acc, fpr, ep, vl)
