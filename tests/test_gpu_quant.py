"""GPU: quantisation-aware training (include/cmoop.h, cmoop_quant).  Every comparison is an equality of bytes:

1. the kernel against ``quant.fake_quant_ref`` on ONE synthetic arena (every launch path, the special rows, sentinels around
   and between the outputs, the same bytes whatever the pooled buffers held);
2. a train step of a net with the option on = a plain net's step on the quantised weights (gradients, metrics, Adam's
   moments, BatchNorm's moving statistics), and the update lands unchanged on the latent weights (straight-through);
3. inference on the quantised copy; ``get_quantized``; post-training use;
4. off is off, down to the population call;
5. a fit validates, stops and reads out the quantised model, with the EMA and the operating-point read-out on top;
6. the evaluator's objective vector and ``train_model``.

Run with -s for the launch paths and times (profiles/quant_parity.txt)."""
import ctypes as C
import dataclasses
import functools
import os
import time

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import (EmaConfig, EvalConfig, OperatingPointConfig, PopulationEvaluator, QuantConfig, _lib,
                                        calculate_fpr, genes as G)
from cmoop_audio_processing_amd import optim as O
from cmoop_audio_processing_amd import quant as Q
from cmoop_audio_processing_amd.session import NetSession
from test_gpu_net import make_data, make_split

pytestmark = pytest.mark.gpu

P = _lib.ptr
F32 = np.float32
T0 = time.time()


def L():
    return _lib.lib()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def host(t):
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, F32), np.ascontiguousarray(b, F32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def n_diff(a, b):
    return int((bits(a) != bits(b)).sum())


# ---- 1. the kernel ---------------------------------------------------------------------------------------------------------------
GUARD = 64
SENT_F, SENT_C = F32(-12345.678), np.int8(0x55)
VAR = "CMOOP_POOL_FILL"


class pool_fill:
    """The variable set to `value` (None: unset) for the length of a with block, then as it was before."""

    def __init__(self, value):
        self.value = value

    def __enter__(self):
        self.before = os.environ.get(VAR)
        if self.value is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = self.value

    def __exit__(self, *exc):
        if self.before is None:
            os.environ.pop(VAR, None)
        else:
            os.environ[VAR] = self.before


def special_block():
    """[8 channels][8]: ties at s = 0.5, all zero, a / 127 underflows, one NaN, one inf, signed zeros, two denormal rows"""
    z = np.zeros((8, 8), F32)
    z[0, :7] = np.array([127, .5, 1.5, 2.5, -.5, -1.5, -2.5], np.float64) * 0.5
    z[2, :3] = [1e-45, 0, -1e-45]
    z[3, :4] = [1.0, np.nan, -2.0, 0.5]
    z[4, :4] = [1.0, np.inf, -2.0, -np.inf]
    z[5] = np.array([-0.0, 0.0] * 4, F32)
    z[6, :4] = [3e-43, -1e-43, 2e-44, 0]
    z[7] = np.array([1e-39, -9e-40, 5e-40, 1.1e-39, -1e-41, 3e-40, 0, 7e-40], F32)
    return z


@functools.lru_cache(maxsize=None)
def synthetic_arena():
    """(flat float32 arena, table rows, {path name: row indices}).  Row tensors of len 9 / 25 (scalar: len % 4), 16 / 144 /
    1600 / 12800 (16-byte path; 1600 and 12800 run the 256-element wave loop 7 and 50 times), a len-16 tensor at an odd
    offset (scalar: alignment), depthwise C 16 / 64 at k 3 / 5 and C 512 (two workgroups of lanes), channel counts 1, 10, 11,
    64; the special block as an aligned row tensor, an odd-offset row tensor and a strided tensor.  Gaps between tensors."""
    rs = np.random.RandomState(11)
    specs = [("row9", 16, 9, False), ("row25", 1, 25, False), ("row16", 10, 16, False), ("row144", 11, 144, False),
             ("row1600", 64, 1600, False), ("row12800", 2, 12800, False), ("row16_odd", 3, 16, True), ("special_vec", 8, 8, False),
             ("special_odd", 8, 8, True)]
    dws = [("dw16k3", 16, 3), ("dw64k3", 64, 3), ("dw16k5", 16, 5), ("dw64k5", 64, 5), ("dw512k3", 512, 3)]
    parts, rows, names, off = [], [], [], 0

    def gap(n):
        nonlocal off
        parts.append(rs.randn(n).astype(F32))
        off += n

    def pad_to(align, odd):
        while off % align != (1 if odd else 0):
            gap(1)

    gap(5)
    for name, ch, ln, odd in specs:
        pad_to(4, odd)
        block = special_block() if name.startswith("special") else (rs.randn(ch, ln) * 10.0 ** rs.uniform(-3, 2, (ch, 1))).astype(F32)
        rows.append((off, ch, ln, ln, 1))
        names.append(name)
        parts.append(block.reshape(-1))
        off += ch * ln
        gap(int(rs.randint(1, 9)))
    for name, c, k in dws:
        block = (rs.randn(k * k, c) * 10.0 ** rs.uniform(-3, 2, (1, c))).astype(F32)
        rows.append((off, c, k * k, 1, c))
        names.append(name)
        parts.append(block.reshape(-1))
        off += k * k * c
        gap(int(rs.randint(1, 9)))
    rows.append((off, 8, 8, 1, 8))                      # the special block, one channel per column
    names.append("special_strided")
    parts.append(np.ascontiguousarray(special_block().T).reshape(-1))
    off += 64
    gap(3)
    flat = np.concatenate(parts)
    assert flat.size == off
    return flat, rows, names


def run_kernel(flat, rows, nbits, with_codes=True, with_scales=True):
    """cmoop_quantize_weights on guarded, sentinel-filled outputs -> (wq, codes, scales) with their guards, as host arrays"""
    n, channels = flat.size, sum(r[1] for r in rows)
    w = dev(flat)
    wq = torch.full((n + 2 * GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    codes = torch.full((n + 2 * GUARD,), int(SENT_C), dtype=torch.int8, device="cuda")
    scales = torch.full((channels + 2 * GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    Q.quantize_weights(w, rows, nbits, wq[GUARD:GUARD + n], codes[GUARD:GUARD + n] if with_codes else None,
                       scales[GUARD:GUARD + channels] if with_scales else None)
    torch.cuda.synchronize()
    assert same_bits(host(w), flat), "w is only read"
    return host(wq), host(codes), host(scales)


def expected(flat, rows, nbits):
    n = flat.size
    wq_ref, codes_ref, scales_ref = Q.quantize_table_ref(flat, rows, nbits)
    wq = np.full(n + 2 * GUARD, SENT_F, F32)
    codes = np.full(n + 2 * GUARD, SENT_C, np.int8)
    for row in rows:
        Q.channel_view(wq[GUARD:GUARD + n], row)[...] = Q.channel_view(wq_ref, row)
        Q.channel_view(codes[GUARD:GUARD + n], row)[...] = Q.channel_view(codes_ref, row)
    scales = np.concatenate([np.full(GUARD, SENT_F, F32), scales_ref, np.full(GUARD, SENT_F, F32)])
    return wq, codes, scales


@pytest.mark.parametrize("nbits", [8, 4, 2])
def test_kernel_equals_the_restatement_on_every_path(nbits):
    flat, rows, names = synthetic_arena()
    assert {r[2] for r in rows} >= {9, 25, 16, 144, 1600, 12800} and {r[1] for r in rows} >= {1, 10, 11, 64}
    assert any(r[0] % 4 == 1 and r[4] == 1 for r in rows) and sum(r[4] != 1 for r in rows) >= 5
    want = expected(flat, rows, nbits)
    got = {}
    t0 = time.time()
    for fill in (None, "0x00", "0x7F", "0xFF"):
        with pool_fill(fill):
            got[fill] = run_kernel(flat, rows, nbits)
    for k, what in enumerate(("wq", "codes", "scales")):
        for name, row in zip(names, rows):
            if what == "wq":
                a, b = (Q.channel_view(x[GUARD:GUARD + flat.size], row) for x in (got[None][0], want[0]))
                assert np.array_equal(bits(a), bits(b)), (nbits, name, int((bits(a) != bits(b)).sum()))
        assert got[None][k].tobytes() == want[k].tobytes(), (nbits, what, "a tensor, a gap or a guard differs")
        for fill in ("0x00", "0x7F", "0xFF"):
            assert got[fill][k].tobytes() == got[None][k].tobytes(), (nbits, what, fill)
    # the optional outputs: absent, nothing of them is written and wq keeps its bytes
    only_wq = run_kernel(flat, rows, nbits, with_codes=False, with_scales=False)
    assert only_wq[0].tobytes() == want[0].tobytes()
    assert (only_wq[1] == SENT_C).all() and (bits(only_wq[2]) == bits(SENT_F)).all()
    paths = {"wave+16B": [n for n, r in zip(names, rows) if r[4] == 1 and r[2] % 4 == 0 and r[0] % 4 == 0],
             "wave+scalar": [n for n, r in zip(names, rows) if r[4] == 1 and not (r[2] % 4 == 0 and r[0] % 4 == 0)],
             "lane": [n for n, r in zip(names, rows) if r[4] != 1]}
    print(f"\n  [quant kernel] bits={nbits} n={flat.size} tensors={len(rows)} channels={sum(r[1] for r in rows)} paths={paths} "
          f"4 fills + 1: {time.time() - t0:.2f}s")


def test_kernel_refuses_bad_tables_before_launching():
    flat, rows, _ = synthetic_arena()
    w = dev(flat)
    out = torch.zeros_like(w)
    with pytest.raises(_lib.CmoopError, match="past the arena"):
        Q.quantize_weights(w, [(flat.size - 10, 2, 9, 9, 1)], 8, out)
    with pytest.raises(_lib.CmoopError, match="past the arena"):
        Q.quantize_weights(w, [(0, 16, 9, 1, flat.size)], 8, out)
    with pytest.raises(_lib.CmoopError, match="table row"):
        Q.quantize_weights(w, [(0, 0, 9, 9, 1)], 8, out)
    with pytest.raises(ValueError, match="bits"):
        Q.quantize_weights(w, rows, 9, out)
    st = QuantConfig(bits=0)._struct()
    tab = np.asarray(rows, np.int64)
    assert L().cmoop_quantize_weights(C.byref(st), P(w), flat.size, P(tab), len(tab), P(out), None, None) != 0
    assert "disabled" in L().cmoop_last_error().decode()
    torch.cuda.synchronize()
    assert not host(out).any(), "nothing was launched"


# ---- 2. the train step -------------------------------------------------------------------------------------------------------------
T_, F_, CLASSES, BATCH, SEED = 21, 12, 10, 8, 77
NETS = [((16, 3, 1, 1, 1, 1), "A"), ((16, 5, 1, 1, 2, 0), "B_ds")]
CFG = EvalConfig(variant="A", classes=CLASSES, batch=BATCH, eval_batch=8, epochs=2, early_stop=False, shuffle=True)
QUANT = QuantConfig(bits=8)


def cfg_of(variant, **over):
    return dataclasses.replace(CFG, variant=variant, **over)


@functools.lru_cache(maxsize=None)
def data(n=2 * BATCH + 3):
    return make_data(n, T_, F_, CLASSES, 7)


def qref(flat, gene, variant, nbits=8):
    return Q.quantize_params_ref(flat, gene, G.VARIANT_NAMES[variant], CLASSES, nbits)


@pytest.mark.parametrize("gene,variant", NETS)
@pytest.mark.parametrize("B", [BATCH, 5])
@pytest.mark.parametrize("nbits", [8, 4])
def test_train_step_is_the_plain_step_on_quantised_weights(gene, variant, B, nbits):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    cfg = cfg_of(variant)
    kinds = O.param_kinds(gene, G.VARIANT_NAMES[variant], CLASSES)
    frozen = kinds == O.KIND_FROZEN
    cs = cfg.to_struct()
    t0 = time.time()
    with NetSession(gene, dataclasses.replace(cfg, quant=QuantConfig(bits=nbits)), T_, F_, SEED) as q, \
            NetSession(gene, cfg, T_, F_, SEED) as p:
        assert q.quant == QuantConfig(bits=nbits) and p.quant is None
        w = q.get_params()
        assert same_bits(w, p.get_params())
        m = v = np.zeros_like(w)
        for step in range(2):
            wq = qref(w, gene, variant, nbits)[0]
            assert n_diff(wq[kinds == 0], w[kinds == 0]) > 0 and same_bits(wq[kinds != 0], w[kinds != 0])
            st = p.get_state()
            st["params"] = wq               # step 2: Q's new latent weights, re-quantised, into P
            p.set_state(st)
            assert same_bits(q.get_params(), w), "the latent weights are untouched until the optimiser moves them"
            q.train_step(Xd, yd, None, row0=step * B, B=B)
            p.train_step(Xd, yd, None, row0=step * B, B=B)
            g = q.get_grads()
            assert same_bits(g, p.get_grads()), (step, n_diff(g, p.get_grads()))
            assert q.train_metrics() == p.train_metrics()
            sq, sp = q.get_state(), p.get_state()
            assert same_bits(sq["m"], sp["m"]) and same_bits(sq["v"], sp["v"])
            assert (sq["iterations"], sq["steps"]) == (sp["iterations"], sp["steps"]) == (step + 1, step + 1)
            assert same_bits(sq["params"][frozen], sp["params"][frozen]), "BatchNorm's moving statistics land in the parameter arena"
            if frozen.any():
                assert not same_bits(sq["params"][frozen], w[frozen])
            # straight-through: the update computed from the quantised forward / backward is applied to the LATENT weights
            _lr, lr32, a32 = O.rates(None, cs, step)
            w2, m, v = O.adamw_step_ref(w, g, m, v, a32, lr32, cs.beta1, cs.beta2, cs.adam_eps, kinds=kinds)
            assert same_bits(sq["params"][~frozen], w2[~frozen]), (step, n_diff(sq["params"][~frozen], w2[~frozen]))
            assert same_bits(sq["m"], m) and same_bits(sq["v"], v)
            assert not same_bits(sq["params"][kinds == 0], sp["params"][kinds == 0]), "P moved the quantised weights instead"
            w = sq["params"]
    print(f"\n  [quant step] {gene} {variant} B={B} bits={nbits}: 2 steps x 2 nets {time.time() - t0:.2f}s")


# ---- 3. inference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gene,variant", NETS)
def test_inference_reads_the_quantised_copy(gene, variant):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    assert len(X) == 2 * CFG.eval_batch + 3
    cfg = cfg_of(variant)
    feat = dev(np.random.RandomState(5).randn(T_ + 2 * 3, F_).astype(F32))
    with NetSession(gene, dataclasses.replace(cfg, quant=QUANT), T_, F_, SEED) as q, NetSession(gene, cfg, T_, F_, SEED) as p, \
            NetSession(gene, cfg, T_, F_, SEED) as late:
        q.train_step(Xd, yd, None, row0=0, B=BATCH)          # moving statistics and weights off their initial values
        w = q.get_params()
        wq, codes, scales = qref(w, gene, variant)
        p.set_params(wq)
        for a, b, what in zip(q.get_quantized(), (wq, codes, scales), ("wq", "codes", "scales")):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), what
        assert same_bits(q.get_params(), w)

        def reads(net):
            loss, acc, preds = net.evaluate(Xd, yd)
            return (loss, acc, host(preds).tobytes(), host(net.predict_proba(Xd)).tobytes(), host(net.predict_logits(Xd)).tobytes(),
                    host(net.predict_stream(feat, 3)).tobytes())
        want = reads(p)
        assert reads(q) == want
        # post-training use: a plain net with the latent weights, the option switched on afterwards
        late.set_params(w)
        assert reads(late) != want
        late.set_quant(QUANT)
        assert reads(late) == want
        for a, b in zip(late.get_quantized(), (wq, codes, scales)):
            assert a.tobytes() == b.tobytes()
        late.set_quant(None)
        with pytest.raises(_lib.CmoopError, match="off"):
            late.get_quantized()


# ---- 4. off is off -------------------------------------------------------------------------------------------------------------------
def test_off_means_off():
    gene, variant = NETS[0]
    X, y = data()
    Xd, yd = dev(X), dev(y)
    cfg = cfg_of(variant)

    def run(net):
        for step in range(2):
            net.train_step(Xd, yd, None, row0=step * BATCH, B=BATCH)
        st = net.get_state()
        loss, acc, preds = net.evaluate(Xd, yd)
        return (st["params"].tobytes(), st["m"].tobytes(), st["v"].tobytes(), net.get_grads().tobytes(), net.train_metrics(), loss, acc,
                host(preds).tobytes())
    with NetSession(gene, cfg, T_, F_, SEED) as never:
        want = run(never)
    with NetSession(gene, cfg, T_, F_, SEED) as null:
        null.set_quant(None)
        assert null.quant is None and run(null) == want
    with NetSession(gene, dataclasses.replace(cfg, quant=QuantConfig(bits=0)), T_, F_, SEED) as zero:
        assert zero.quant is None and run(zero) == want
    with NetSession(gene, dataclasses.replace(cfg, quant=QUANT), T_, F_, SEED) as was_on:
        was_on.set_quant(QuantConfig(bits=0))
        assert run(was_on) == want, "switched off again before the first step: a net that never had it"
    with NetSession(gene, dataclasses.replace(cfg, quant=QUANT), T_, F_, SEED) as on:
        assert run(on)[0] != want[0]


N_TRAIN, N_VAL = 192, 64
FIT = dataclasses.replace(CFG, epochs=4, early_stop=True, patience=1, acc_readout="evaluate", fpr_variant="v1", eval_batch=32)


@functools.lru_cache(maxsize=None)
def split():
    return make_split(N_TRAIN, N_VAL, T_, F_, CLASSES, 31, noise=2.5, label_noise=0.3)


def population(ev, cfg, quant_struct, symbol, genes_, seeds_):
    """One direct call of cmoop_eval_population_q / _op, every other option NULL -> (bytes of acc, size_mb, fpr, epochs_run,
    val_loss; the quant array or None)"""
    n = len(genes_)
    genes, seeds = np.ascontiguousarray(np.array(genes_, np.int32)), np.array(seeds_, np.uint32)
    acc, size, fpr, vl = (np.zeros(n, np.float64) for _ in range(4))
    ep = np.zeros(n, np.int32)
    quant = np.ones((n, 2), np.float64)
    c, ds = cfg.to_struct(), ev._dataset()
    extra = ([C.byref(quant_struct) if quant_struct is not None else None] if symbol == "_q" else [])
    tail = [None, P(quant)] if symbol == "_q" else [None]
    torch.cuda.synchronize()
    _lib.check(getattr(L(), "cmoop_eval_population" + symbol)(
        C.byref(c), None, None, None, None, None, None, *extra, C.byref(ds), P(genes), P(seeds), C.c_int32(n), None, None, P(acc), P(size),
        P(fpr), P(ep), P(vl), None, None, *tail))
    return tuple(a.tobytes() for a in (acc, size, fpr, ep, vl)), (quant if symbol == "_q" else None)


def test_population_call_with_null_is_the_op_call():
    pop, seeds = [NETS[0][0], (16, 3, 0, 1, 2, 1)], [5, 6]
    cfg = dataclasses.replace(FIT, epochs=2, n_slots=2)
    ev = PopulationEvaluator(*split(), cfg)
    off, _ = population(ev, cfg, None, "_op", pop, seeds)
    null, quant = population(ev, cfg, None, "_q", pop, seeds)
    assert null == off and not quant.any(), "quant receives zeros"
    zero, quant = population(ev, cfg, QuantConfig(bits=0)._struct(), "_q", pop, seeds)
    assert zero == off and not quant.any()
    on, quant = population(ev, cfg, QuantConfig(bits=4)._struct(), "_q", pop, seeds)
    assert on[1] == off[1], "size_mb stays count_params * 4 / 2^20"
    assert on[4] != off[4], "the fit is another fit"
    assert quant.tolist() == [[G.quant_size_mb(g, 0, CLASSES, 4), 4.0] for g in pop]
    bad = QuantConfig(bits=8)._struct()
    bad.reserved[1] = 1
    with pytest.raises(_lib.CmoopError, match="reserved"):
        population(ev, cfg, bad, "_q", pop, seeds)


# ---- 5. the fit ----------------------------------------------------------------------------------------------------------------------
def same_dict(a, b):
    assert sorted(a) == sorted(b)
    for k in a:
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), k


@pytest.mark.parametrize("restore_best", [False, True])
@pytest.mark.parametrize("ema", [None, EmaConfig(momentum=0.9)])
def test_fit_scores_the_quantised_model(restore_best, ema):
    gene, variant = NETS[0]
    Xtr, ytr, Xva, yva = (dev(a) for a in split())
    op = OperatingPointConfig(recall=0.9)
    # lr 1e-2: on this split the validation loss of the quantised fit turns after its first epoch, so the fit stops early, past
    # its best epoch, and restore_best reads out an earlier epoch's snapshot than the weights the net holds
    cfg = dataclasses.replace(FIT, lr=1e-2, restore_best=restore_best, quant=QUANT, ema=ema, operating_point=op)
    plain = dataclasses.replace(cfg, quant=None, ema=None, operating_point=None)
    t0 = time.time()
    with NetSession(gene, cfg, T_, F_, SEED) as net, NetSession(gene, plain, T_, F_, SEED) as twin:
        r = net.fit(Xtr, ytr, Xva, yva)
        assert r["epochs_run"] < cfg.epochs and r["best_epoch"] < r["epochs_run"] - 1, "this split stops early, past its best epoch"
        final = net.get_params()
        wq, codes, scales = net.get_quantized()
        ref = qref(final, gene, variant)
        for a, b in zip((wq, codes, scales), ref):
            assert a.tobytes() == b.tobytes()
        if ema is not None and (not restore_best or r["best_epoch"] == r["epochs_run"] - 1):
            assert same_bits(wq, qref(net.get_ema(), gene, variant)[0]), "the finalised average, quantised"
        twin.set_params(wq)
        loss, acc, preds = twin.evaluate(Xva, yva)
        assert (r["val_loss"], r["acc"]) == (loss, acc)
        assert r["fpr"] == calculate_fpr(host(yva), host(preds), CLASSES, "v1")
        readout = r["best_epoch"] if restore_best else r["epochs_run"] - 1
        assert (loss, acc) == (r["val_loss_history"][readout], r["val_accuracy_history"][readout]), "validation saw the same model"
        twin.set_params(final)
        assert twin.evaluate(Xva, yva)[0] != loss, "the latent weights are another model"
        twin.set_params(wq)
        same_dict(r["operating_point"], twin.operating_point(Xva, yva, recall=op.recall))
    print(f"\n  [quant fit] restore_best={restore_best} ema={ema is not None}: epochs_run={r['epochs_run']} best={r['best_epoch']} "
          f"val_loss={r['val_loss_history'].tolist()} {time.time() - t0:.2f}s")


# ---- 6. the evaluator ----------------------------------------------------------------------------------------------------------------
def test_evaluator_objectives_and_train_model():
    pop = [NETS[0][0], (16, 3, 0, 1, 2, 1), (16, 5, 1, 1, 1, 0)]
    hps = [G.gene_to_hparams(g) for g in pop]
    base = dataclasses.replace(FIT, epochs=2, n_slots=3, seed=9, max_model_size=0.05)
    on = dataclasses.replace(base, quant=QuantConfig(bits=8, objective=True))
    add = dataclasses.replace(base, quant=QuantConfig(bits=8, objective=False))
    res_on = PopulationEvaluator(*split(), on).compute_objectives_and_constraints(hps)
    ev = PopulationEvaluator(*split(), add)
    res_add = ev.compute_objectives_and_constraints(hps)
    res_off = PopulationEvaluator(*split(), base).compute_objectives_and_constraints(hps)
    for g, a, b, c in zip(pop, res_on, res_add, res_off):
        q_mb, f_mb = G.quant_size_mb(g, 0, CLASSES, 8), G.model_size_mb(g, 0, CLASSES)
        assert a["objs"][1] == q_mb and a["quant"] == {"size_mb": q_mb, "bits": 8} and a["size_fp32_mb"] == f_mb
        assert b["objs"][1] == f_mb and b["quant"] == {"size_mb": q_mb, "bits": 8} and "size_fp32_mb" not in b
        assert "quant" not in c and c["objs"][1] == f_mb
        assert a["objs"][0] == b["objs"][0] and a["objs"][2] == b["objs"][2], "objective only moves the size"
        assert a["CV"] == max(0.0, on.min_accuracy + a["objs"][0]) + max(0.0, q_mb - on.max_model_size) + max(0.0, a["objs"][2] - on.max_fpr)
        assert b["CV"] == max(0.0, on.min_accuracy + b["objs"][0]) + max(0.0, f_mb - on.max_model_size) + max(0.0, b["objs"][2] - on.max_fpr)
    assert any(a["CV"] != b["CV"] for a, b in zip(res_on, res_add)), "the size constraint reads the quantised size"
    # train_model: candidate 0 again, its invariant, and plain fp32 scoring of the quantised model
    tm = ev.train_model(hps[0], ev.last_seeds[0])
    assert (-tm.objectives["acc"], tm.objectives["fpr"]) == (res_add[0]["objs"][0], res_add[0]["objs"][2])
    assert tm.quant_bits == 8 and tm.quant_codes.dtype == np.int8 and tm.quant_scales.dtype == F32
    rows = Q.quant_table(pop[0], 0, CLASSES)
    assert same_bits(Q.dequantize(tm.quant_codes, tm.quant_scales, rows, like=tm.params), tm.params)
    assert np.abs(tm.quant_codes.astype(int)).max() == 127
    X = ev.X_val
    with NetSession(pop[0], add, T_, F_, ev.last_seeds[0]) as net:
        net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
        want = host(net.predict_logits(X))
        assert same_bits(net.get_quantized()[0], tm.params)
        assert not same_bits(net.get_params(), tm.params)
    assert same_bits(host(tm.logits(X, base)), want), "no option set: the fp32 paths score the int8-weight model"
    print(f"\n  [quant total] module wall time so far {time.time() - T0:.1f}s")
