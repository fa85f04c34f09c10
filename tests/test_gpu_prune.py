"""GPU: magnitude pruning in training (include/cmoop.h, cmoop_prune).  Every comparison is an equality of bytes:

1. the launch sequence against ``prune.prune_ref`` on ONE synthetic arena (every length class, odd and aligned offsets, an
   excluded tensor in between, every k, the value blocks that make each radix pass decide, the zero counts, sentinels around
   and between the outputs, the same bytes whatever the pooled buffers held);
2. a train step of a net with the option on = a plain net's step on the pruned weights (gradients, metrics, Adam's moments,
   BatchNorm's moving statistics) before, inside and after the ramp, and the update lands unchanged on the dense latent
   weights (straight-through); the same with the quantiser on top;
3. inference reads the final-sparsity copy whatever the iteration; ``get_pruned``; one-shot use;
4. off is off, down to the population call;
5. a fit validates, stops and reads out the pruned model, with the EMA on top;
6. the evaluator's objective vector and ``train_model``.

Run with -s for the times."""
import ctypes as C
import dataclasses
import functools
import time

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import (EmaConfig, PopulationEvaluator, PruneConfig, QuantConfig, TrainedModel, _lib,
                                        calculate_fpr, genes as G)
from cmoop_audio_processing_amd import optim as O
from cmoop_audio_processing_amd import prune as PR
from cmoop_audio_processing_amd import quant as Q
from cmoop_audio_processing_amd.session import NetSession
from test_gpu_quant import (BATCH, CLASSES, F_, FIT, NETS, SEED, T_, bits, cfg_of, data, dev, host, n_diff, pool_fill, same_bits, split)

pytestmark = pytest.mark.gpu

P = _lib.ptr
F32 = np.float32
U32 = np.uint32
T0 = time.time()


def L():
    return _lib.lib()


# ---- 1. the launch sequence ------------------------------------------------------------------------------------------------------
GUARD = 64
SENT_F, SENT_Z = F32(-12345.678), np.int32(0x5A5A5A5A)
LENGTHS = [1, 9, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 12800, 300001]
MODES = ["k0", "k1", "len-1", 0.5, 0.8, 0.999]


def from_keys(keys, rs):
    """float32 values with the given 31-bit keys and random signs"""
    keys = np.asarray(keys, np.uint64).astype(U32)
    return (keys | (rs.randint(0, 2, keys.size).astype(U32) << U32(31))).view(F32)


def value_block(kind, n, rs):
    if kind == "normal":
        return (rs.randn(n) * 10.0 ** rs.uniform(-3, 2)).astype(F32)
    if kind == "ties":            # 40 % small distinct, a run of one magnitude with both signs across the middle ranks, the rest larger
        lo, run = (2 * n) // 5, max(1, (3 * n) // 10)
        mag = np.concatenate([np.linspace(0.001, 0.4, lo), np.full(run, 0.5), np.linspace(0.6, 9.0, n - lo - run)])[:n]
        return (rs.permutation(mag) * rs.choice([-1.0, 1.0], n)).astype(F32)
    if kind == "equal":
        return np.full(n, -1.25, F32) * rs.choice([-1.0, 1.0], n).astype(F32)
    if kind == "zeros":           # +0.0 and -0.0 in the majority, so every k up to 0.8 len has its threshold at key 0
        v = rs.randn(n).astype(F32)
        z = rs.rand(n) < 0.9
        v[z] = np.where(rs.rand(int(z.sum())) < 0.5, F32(0.0), F32(-0.0))
        return v
    if kind == "denormal":        # keys below 2^23: the top digit is 0 .. 7, mostly 0
        return from_keys(rs.randint(0, 1 << 23, n), rs)
    if kind == "nonfinite":       # inf and NaNs of several payloads among normals
        v = rs.randn(n).astype(F32)
        sel = rs.rand(n) < 0.3
        v.view(U32)[sel] = rs.choice(np.array([0x7F800000, 0xFF800000, 0x7FC00000, 0xFFC00001, 0x7F800001, 0x7FFFFFFF], U32), int(sel.sum()))
        return v
    if kind == "top":             # keys that differ only in the top digit: the first pass decides alone
        return from_keys((rs.randint(1, 2048, n).astype(np.uint64) << 20) | 0x5A5A5, rs)
    if kind == "mid":             # one top digit, one low digit: the second pass decides
        return from_keys((0x3F8 << 20) | (rs.randint(0, 1024, n).astype(np.uint64) << 10) | 0x155, rs)
    if kind == "low":             # keys that differ only in the lowest digit: the third pass decides
        return from_keys((0x3F8 << 20) | (0x2AA << 10) | rs.randint(0, 1024, n).astype(np.uint64), rs)
    raise ValueError(kind)


@functools.lru_cache(maxsize=None)
def synthetic_arena():
    """(flat float32 arena, [(off, len, prunable)], names).  Every length of LENGTHS as a normal tensor, alternately at an odd
    offset and at a 16-byte aligned one; every special value block at lengths 9, 257, 2049 and 12800 (and the tie run and the
    low-digit block at 300001 / 65); excluded tensors (copied whatever s is) between the pruned ones; gaps between all."""
    rs = np.random.RandomState(23)
    parts, rows, names, off = [], [], [], 0

    def gap(n):
        nonlocal off
        parts.append(rs.randn(n).astype(F32))
        off += n

    def add(name, block, odd, prunable=True):
        nonlocal off
        while off % 4 != (1 if odd else 0):
            gap(1)
        rows.append((off, block.size, prunable))
        names.append(name)
        parts.append(block.reshape(-1))
        off += block.size
        gap(int(rs.randint(1, 9)))

    gap(5)
    for i, n in enumerate(LENGTHS):
        add(f"normal{n}", value_block("normal", n, rs), odd=i % 2 == 0)
        if n == 64:
            add("excluded_dw", rs.randn(9, 16).astype(F32), odd=True, prunable=False)     # a depthwise [kh kw][C] kernel: copied
        if n in (9, 257, 2049, 12800):
            for j, kind in enumerate(("ties", "equal", "zeros", "denormal", "nonfinite", "top", "mid", "low")):
                add(f"{kind}{n}", value_block(kind, n, rs), odd=(i + j) % 2 == 1)
    add("normal2048_odd", value_block("normal", 2048, rs), odd=True)
    add("normal300001_aligned", value_block("normal", 300001, rs), odd=False)
    add("ties300001", value_block("ties", 300001, rs), odd=True)
    add("low65", value_block("low", 65, rs), odd=True)
    add("excluded_conv1", rs.randn(16, 9).astype(F32), odd=False, prunable=False)
    gap(3)
    flat = np.concatenate(parts)
    assert flat.size == off and len(rows) <= 128
    return flat, rows, names


def table_of(rows, mode):
    """(table rows {off, len, k}, s of the call): explicit k for the three k modes, k = -1 (floor(s len) on the device) for a sparsity"""
    if mode == "k0":
        return [(off, n, 0) for off, n, _p in rows], 0.0
    if mode == "k1":
        return [(off, n, 1 if p else 0) for off, n, p in rows], 0.0
    if mode == "len-1":
        return [(off, n, n - 1 if p else 0) for off, n, p in rows], 0.0
    return [(off, n, -1 if p else 0) for off, n, p in rows], float(mode)


def run_launches(flat, table, s, with_zeros=True):
    """cmoop_prune_weights on guarded, sentinel-filled outputs -> (out, zeros with their guards as host arrays, launches)"""
    n = flat.size
    w = dev(flat)
    out = torch.full((n + 2 * GUARD,), float(SENT_F), dtype=torch.float32, device="cuda")
    zeros = torch.full((len(table) + 2 * GUARD,), int(SENT_Z), dtype=torch.int32, device="cuda")
    launches = PR.prune_weights(w, table, s, out[GUARD:GUARD + n], zeros[GUARD:GUARD + len(table)] if with_zeros else None)
    torch.cuda.synchronize()
    assert same_bits(host(w), flat), "w is only read"
    return host(out), host(zeros), launches


def expected(flat, table, s):
    n = flat.size
    out = np.full(n + 2 * GUARD, SENT_F, F32)
    zeros = np.full(len(table) + 2 * GUARD, SENT_Z, np.int32)
    for i, row in enumerate(table):
        off, ln = row[0], row[1]
        out[GUARD + off:GUARD + off + ln], zeros[GUARD + i] = PR.prune_ref(flat[off:off + ln], PR.row_k(row, s))
    return out, zeros


@pytest.mark.parametrize("mode", MODES, ids=[str(m) for m in MODES])
def test_launch_sequence_equals_the_restatement(mode):
    flat, rows, names = synthetic_arena()
    assert {r[1] for r in rows} >= set(LENGTHS)
    assert any(r[0] % 4 == 1 for r in rows) and any(r[0] % 4 == 0 for r in rows) and sum(not r[2] for r in rows) == 2
    table, s = table_of(rows, mode)
    want_out, want_zeros = expected(flat, table, s)
    t0 = time.time()
    got = {}
    for fill in ("0x00", "0xFF"):
        with pool_fill(fill):
            got[fill] = run_launches(flat, table, s)
    out, zeros, launches = got["0x00"]
    for name, row in zip(names, table):
        a, b = (x[GUARD + row[0]:GUARD + row[0] + row[1]] for x in (out, want_out))
        assert np.array_equal(bits(a), bits(b)), (mode, name, PR.row_k(row, s), int((bits(a) != bits(b)).sum()))
    assert out.tobytes() == want_out.tobytes(), (mode, "a tensor, a gap or a guard differs")
    assert zeros.tobytes() == want_zeros.tobytes(), (mode, [(n, int(a), int(b)) for n, a, b in
                                                            zip(names, zeros[GUARD:], want_zeros[GUARD:]) if a != b])
    assert got["0xFF"][0].tobytes() == out.tobytes() and got["0xFF"][1].tobytes() == zeros.tobytes(), "whatever the pooled buffers held"
    assert launches == got["0xFF"][2] == (1 if mode == "k0" else 4), "at most four launches; the select is skipped when every k is 0"
    if mode == "k0":
        assert same_bits(out[GUARD:-GUARD][np.concatenate([np.arange(o, o + n) for o, n, _k in table])],
                         flat[np.concatenate([np.arange(o, o + n) for o, n, _k in table])]), "a bit copy"
    # the zero counts are optional: absent, nothing of them is written and out keeps its bytes
    only_out = run_launches(flat, table, s, with_zeros=False)
    assert only_out[0].tobytes() == want_out.tobytes() and (only_out[1] == SENT_Z).all()
    tied = [n for n, row, z in zip(names, table, want_zeros[GUARD:]) if z > PR.row_k(row, s)]
    print(f"\n  [prune kernel] mode={mode} n={flat.size} tensors={len(table)} launches={launches} tied tensors={len(tied)} "
          f"2 fills + 1: {time.time() - t0:.2f}s")


def test_mixed_copy_and_pruned_rows_in_one_call_and_a_second_call_on_the_same_buffers():
    """k = 0 rows next to pruned ones take the four-launch path as copies; the arena's own output buffer is reused."""
    flat, rows, _names = synthetic_arena()
    table = [(off, n, (-1 if i % 3 else 0) if p else 0) for i, (off, n, p) in enumerate(rows)]
    want_out, want_zeros = expected(flat, table, 0.8)
    out, zeros, launches = run_launches(flat, table, 0.8)
    assert launches == 4 and out.tobytes() == want_out.tobytes() and zeros.tobytes() == want_zeros.tobytes()


def test_bad_tables_are_refused_before_any_launch():
    flat, rows, _ = synthetic_arena()
    w = dev(flat)
    out = torch.zeros_like(w)
    n = flat.size
    for table, word in (([(n - 10, 11, 1)], "past the arena"), ([(0, 0, 0)], "len >= 1"), ([(0, 9, 10)], r"k in \[-1, len\]"),
                        ([(0, 9, -2)], "outside"), ([(10, 9, 1), (0, 9, 1)], "arena order"),
                        ([(0, 9, 1), (8, 9, 1)], "overlap"), ([(-1, 9, 1)], "off >= 0"),
                        ([(i * 4, 4, 1) for i in range(129)], "128")):
        with pytest.raises(_lib.CmoopError, match=word):
            PR.prune_weights(w, table, 0.5, out)
    with pytest.raises(_lib.CmoopError, match=r"s must be in \[0, 1\)"):
        PR.prune_weights(w, [(0, 9, -1)], 1.0, out)
    with pytest.raises(_lib.CmoopError, match=r"s must be in \[0, 1\)"):
        PR.prune_weights(w, [(0, 9, -1)], float("nan"), out)
    with pytest.raises(_lib.CmoopError, match="past the arena"):
        PR.prune_weights(w[:100], [(0, 101, 1)], 0.5, out)
    torch.cuda.synchronize()
    assert not host(out).any(), "nothing was launched"


# ---- 2. the train step -------------------------------------------------------------------------------------------------------------
PRUNE = PruneConfig(sparsity=0.8, begin_step=1, end_step=4)        # iterations 0, 1: s = 0; 2, 3: inside the ramp; 4: the end


def pref(flat, gene, variant, s, nbits=None):
    """the arena forward reads at sparsity s: pruned, then (nbits) quantised"""
    v = G.VARIANT_NAMES[variant]
    w = PR.prune_params_ref(flat, gene, v, CLASSES, s)[0]
    return w if nbits is None else Q.quantize_params_ref(w, gene, v, CLASSES, nbits)[0]


@pytest.mark.parametrize("gene,variant", NETS)
@pytest.mark.parametrize("nbits", [None, 8])
def test_train_step_is_the_plain_step_on_pruned_weights(gene, variant, nbits):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    B = 3                                # five steps of three rows inside the 19 rows of data()
    cfg = cfg_of(variant)
    kinds = O.param_kinds(gene, G.VARIANT_NAMES[variant], CLASSES)
    frozen = kinds == O.KIND_FROZEN
    cs = cfg.to_struct()
    on = dataclasses.replace(cfg, prune=PRUNE, quant=QuantConfig(bits=nbits) if nbits else None)
    ss = [PR.sparsity_at(PRUNE, it) for it in range(5)]
    assert ss[0] == ss[1] == 0.0 and 0.0 < ss[2] < ss[3] < ss[4] == 0.8, "before begin, mid-ramp, after end"
    t0 = time.time()
    with NetSession(gene, on, T_, F_, SEED) as q, NetSession(gene, cfg, T_, F_, SEED) as p:
        assert q.prune == PRUNE and p.prune is None
        w = q.get_params()
        assert same_bits(w, p.get_params())
        m = v = np.zeros_like(w)
        for step in range(5):
            weff = pref(w, gene, variant, ss[step], nbits)
            if ss[step] > 0:
                assert n_diff(weff[kinds == 0], w[kinds == 0]) > 0
            elif nbits is None:
                assert same_bits(weff, w), "s = 0: the step is the plain step"
            assert same_bits(weff[kinds != 0], w[kinds != 0])
            st = p.get_state()
            st["params"] = weff
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
            # straight-through: the update computed on the pruned forward / backward is applied to the DENSE latent weights
            _lr, lr32, a32 = O.rates(None, cs, step)
            w2, m, v = O.adamw_step_ref(w, g, m, v, a32, lr32, cs.beta1, cs.beta2, cs.adam_eps, kinds=kinds)
            assert same_bits(sq["params"][~frozen], w2[~frozen]), (step, n_diff(sq["params"][~frozen], w2[~frozen]))
            assert same_bits(sq["m"], m) and same_bits(sq["v"], v)
            if ss[step] > 0:
                pruned = (weff == 0) & (w != 0) & (kinds == 0)
                assert pruned.any() and (sq["params"][pruned] != 0).all(), "pruned weights keep their latent values and can regrow"
            w = sq["params"]
    print(f"\n  [prune step] {gene} {variant} bits={nbits}: 5 steps x 2 nets {time.time() - t0:.2f}s")


# ---- 3. inference ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gene,variant", NETS)
def test_inference_reads_the_final_sparsity_copy_whatever_the_iteration(gene, variant):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    cfg = cfg_of(variant)
    far = PruneConfig(sparsity=0.8, begin_step=1000, end_step=2000)      # training never leaves s = 0 here
    v = G.VARIANT_NAMES[variant]
    feat = dev(np.random.RandomState(5).randn(T_ + 2 * 3, F_).astype(F32))
    with NetSession(gene, dataclasses.replace(cfg, prune=far), T_, F_, SEED) as q, NetSession(gene, cfg, T_, F_, SEED) as p, \
            NetSession(gene, cfg, T_, F_, SEED) as late:
        q.train_step(Xd, yd, None, row0=0, B=BATCH)          # iteration 0 < begin_step: a plain step
        p.train_step(Xd, yd, None, row0=0, B=BATCH)
        w = q.get_params()
        assert same_bits(w, p.get_params()), "s(0) = 0: the step was the plain step"
        weff, zeros = PR.prune_params_ref(w, gene, v, CLASSES, 0.8)
        p.set_params(weff)
        got_w, got_z = q.get_pruned()
        assert got_w.tobytes() == weff.tobytes() and got_z.dtype == np.uint32 and got_z.tobytes() == zeros.tobytes()
        rows = PR.prune_table(gene, v, CLASSES)
        assert all(z >= PR.row_k(r, 0.8) for z, r in zip(got_z, rows)) and any(r[2] == 0 for r in rows) and any(z > 0 for z in got_z)
        assert same_bits(q.get_params(), w)

        def reads(net):
            loss, acc, preds = net.evaluate(Xd, yd)
            return (loss, acc, host(preds).tobytes(), host(net.predict_proba(Xd)).tobytes(), host(net.predict_logits(Xd)).tobytes(),
                    host(net.predict_stream(feat, 3)).tobytes())
        want = reads(p)
        assert reads(q) == want, "the final sparsity, although the schedule is still at 0"
        # one-shot use: a plain net with the latent weights, the option switched on afterwards; then the quantiser on top
        late.set_params(w)
        assert reads(late) != want
        late.set_prune(PruneConfig(sparsity=0.8))
        assert reads(late) == want
        late.set_quant(QuantConfig(bits=8))
        wq, codes, scales = Q.quantize_params_ref(weff, gene, v, CLASSES, 8)
        for a, b in zip(late.get_quantized(), (wq, codes, scales)):
            assert a.tobytes() == b.tobytes(), "prune, then quantise the pruned kernels"
        kinds = O.param_kinds(gene, v, CLASSES)
        assert not codes[(weff == 0) & (kinds == 0)].any(), "a pruned element has code 0"
        p.set_params(wq)
        assert reads(late) == reads(p)
        assert late.get_pruned()[0].tobytes() == weff.tobytes(), "get_pruned stays the pruned, not quantised, arena"
        late.set_quant(None)
        late.set_prune(PruneConfig(sparsity=0.5, skip_small=False))
        weff2, zeros2 = PR.prune_params_ref(w, gene, v, CLASSES, 0.5, skip_small=False)
        got_w, got_z = late.get_pruned()
        assert got_w.tobytes() == weff2.tobytes() and got_z.tobytes() == zeros2.tobytes() and (got_z > 0).all(), "every kernel tensor"
        late.set_prune(None)
        with pytest.raises(_lib.CmoopError, match="off"):
            late.get_pruned()


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
        null.set_prune(None)
        assert null.prune is None and run(null) == want
    with NetSession(gene, dataclasses.replace(cfg, prune=PruneConfig(sparsity=0.0, begin_step=3, end_step=9)), T_, F_, SEED) as zero:
        assert zero.prune is None and run(zero) == want
    with NetSession(gene, dataclasses.replace(cfg, prune=PruneConfig(sparsity=0.8)), T_, F_, SEED) as was_on:
        was_on.set_prune(PruneConfig(sparsity=0.0))
        assert run(was_on) == want, "switched off again before the first step: a net that never had it"
    with NetSession(gene, dataclasses.replace(cfg, prune=PruneConfig(sparsity=0.8)), T_, F_, SEED) as on:
        assert run(on)[0] != want[0]


def population(ev, cfg, quant_struct, prune_struct, symbol, genes_, seeds_):
    """One direct call of cmoop_eval_population_p / _q, every other option NULL -> (bytes of acc, size_mb, fpr, epochs_run,
    val_loss; the quant array; the prune array or None)"""
    n = len(genes_)
    genes, seeds = np.ascontiguousarray(np.array(genes_, np.int32)), np.array(seeds_, np.uint32)
    acc, size, fpr, vl = (np.zeros(n, np.float64) for _ in range(4))
    ep = np.zeros(n, np.int32)
    quant, prune = np.ones((n, 2), np.float64), np.ones((n, 3), np.float64)
    c, ds = cfg.to_struct(), ev._dataset()
    ref = lambda s: C.byref(s) if s is not None else None        # noqa: E731
    extra = [ref(quant_struct)] + ([ref(prune_struct)] if symbol == "_p" else [])
    tail = [None, P(quant)] + ([P(prune)] if symbol == "_p" else [])
    torch.cuda.synchronize()
    _lib.check(getattr(L(), "cmoop_eval_population" + symbol)(
        C.byref(c), None, None, None, None, None, None, *extra, C.byref(ds), P(genes), P(seeds), C.c_int32(n), None, None, P(acc), P(size),
        P(fpr), P(ep), P(vl), None, None, *tail))
    return tuple(a.tobytes() for a in (acc, size, fpr, ep, vl)), quant, (prune if symbol == "_p" else None)


def test_population_call_with_null_is_the_q_call():
    pop, seeds = [NETS[0][0], (16, 3, 0, 1, 2, 1)], [5, 6]
    cfg = dataclasses.replace(FIT, epochs=2, n_slots=2)
    ev = PopulationEvaluator(*split(), cfg)
    for q in (QuantConfig(bits=4)._struct(), None):          # the last round leaves `off`: the call with no option at all
        off, quant_off, _ = population(ev, cfg, q, None, "_q", pop, seeds)
        null, quant, prune = population(ev, cfg, q, None, "_p", pop, seeds)
        assert null == off and quant.tobytes() == quant_off.tobytes() and not prune.any(), "prune receives zeros"
        zero, quant, prune = population(ev, cfg, q, PruneConfig(sparsity=0.0, begin_step=4)._struct(), "_p", pop, seeds)
        assert zero == off and quant.tobytes() == quant_off.tobytes() and not prune.any()
    pc = PruneConfig(sparsity=0.75, begin_step=0, end_step=6)
    on, quant, prune = population(ev, cfg, None, pc._struct(), "_p", pop, seeds)
    assert on[1] == off[1], "size_mb stays count_params * 4 / 2^20"
    assert on[4] != off[4], "the fit is another fit"
    assert not quant.any()
    for g, row in zip(pop, prune.tolist()):
        assert row[:2] == [G.prune_size_mb(g, 0, CLASSES, 0.75), 0.75]
        rows = PR.prune_table(g, 0, CLASSES)
        floor = sum(PR.row_k(r, 0.75) for r in rows) / sum(r[1] for r in rows if r[2] != 0)
        assert floor <= row[2] < 1.0, "at least k zeros in every pruned tensor of the scored model"
    both, quant, prune = population(ev, cfg, QuantConfig(bits=4)._struct(), pc._struct(), "_p", pop, seeds)
    assert [r[0] for r in prune.tolist()] == [G.prune_size_mb(g, 0, CLASSES, 0.75, 4) for g in pop]
    assert quant.tolist() == [[G.quant_size_mb(g, 0, CLASSES, 4), 4.0] for g in pop]
    bad = pc._struct()
    bad.objective = 5
    with pytest.raises(_lib.CmoopError, match="objective"):
        population(ev, cfg, None, bad, "_p", pop, seeds)


# ---- 5. the fit ----------------------------------------------------------------------------------------------------------------------
STEPS_PER_EPOCH = 192 // BATCH


@pytest.mark.parametrize("restore_best", [False, True])
@pytest.mark.parametrize("ema", [None, EmaConfig(momentum=0.9)])
def test_fit_scores_the_pruned_model(restore_best, ema):
    gene, variant = NETS[0]
    v = G.VARIANT_NAMES[variant]
    Xtr, ytr, Xva, yva = (dev(a) for a in split())
    assert len(Xtr) == 192
    pc = PruneConfig.polynomial(0.8, 0, 2, STEPS_PER_EPOCH)
    cfg = dataclasses.replace(FIT, lr=1e-2, restore_best=restore_best, prune=pc, ema=ema)
    plain = dataclasses.replace(cfg, prune=None, ema=None)
    t0 = time.time()
    with NetSession(gene, cfg, T_, F_, SEED) as net, NetSession(gene, plain, T_, F_, SEED) as twin:
        r = net.fit(Xtr, ytr, Xva, yva)
        final = net.get_params()
        weff, zeros = net.get_pruned()
        ref_w, ref_z = PR.prune_params_ref(final, gene, v, CLASSES, 0.8)
        assert weff.tobytes() == ref_w.tobytes() and zeros.tobytes() == ref_z.tobytes()
        rows = PR.prune_table(gene, v, CLASSES)
        assert all(int(z) >= PR.row_k(row, 0.8) for z, row in zip(zeros, rows)), "get_pruned has >= k zeros per tensor"
        assert not same_bits(weff, final), "the latent weights stay dense"
        twin.set_params(weff)
        loss, acc, preds = twin.evaluate(Xva, yva)
        assert (r["val_loss"], r["acc"]) == (loss, acc), "the read-out is that of the pruned model"
        assert r["fpr"] == calculate_fpr(host(yva), host(preds), CLASSES, "v1")
        readout = r["best_epoch"] if restore_best else r["epochs_run"] - 1
        assert (loss, acc) == (r["val_loss_history"][readout], r["val_accuracy_history"][readout]), "validation saw the same model"
        assert int(np.argmin(r["val_loss_history"])) == r["best_epoch"], "early stopping monitors the pruned model's loss"
        twin.set_params(final)
        assert twin.evaluate(Xva, yva)[0] != loss, "the latent weights are another model"
    print(f"\n  [prune fit] restore_best={restore_best} ema={ema is not None}: epochs_run={r['epochs_run']} best={r['best_epoch']} "
          f"val_loss={np.asarray(r['val_loss_history']).tolist()} {time.time() - t0:.2f}s")


# ---- 6. the evaluator ----------------------------------------------------------------------------------------------------------------
def test_evaluator_objectives_and_train_model(tmp_path):
    pop = [NETS[0][0], (16, 3, 0, 1, 2, 1), (16, 5, 1, 1, 1, 0)]
    hps = [G.gene_to_hparams(g) for g in pop]
    base = dataclasses.replace(FIT, epochs=2, n_slots=3, seed=9, max_model_size=0.05)
    pc = PruneConfig.polynomial(0.8, 0, 1, STEPS_PER_EPOCH)
    on = dataclasses.replace(base, prune=pc)
    add = dataclasses.replace(base, prune=dataclasses.replace(pc, objective=False))
    both = dataclasses.replace(base, prune=pc, quant=QuantConfig(bits=8))
    res_on = PopulationEvaluator(*split(), on).compute_objectives_and_constraints(hps)
    ev = PopulationEvaluator(*split(), add)
    res_add = ev.compute_objectives_and_constraints(hps)
    res_both = PopulationEvaluator(*split(), both).compute_objectives_and_constraints(hps)
    res_off = PopulationEvaluator(*split(), base).compute_objectives_and_constraints(hps)
    for g, a, b, c, d in zip(pop, res_on, res_add, res_off, res_both):
        p_mb, f_mb, pq_mb = G.prune_size_mb(g, 0, CLASSES, 0.8), G.model_size_mb(g, 0, CLASSES), G.prune_size_mb(g, 0, CLASSES, 0.8, 8)
        assert a["objs"][1] == p_mb and a["prune"] == {"size_mb": p_mb, "sparsity": 0.8} and a["size_fp32_mb"] == f_mb
        assert b["objs"][1] == f_mb and b["prune"] == {"size_mb": p_mb, "sparsity": 0.8} and "size_fp32_mb" not in b
        assert "prune" not in c and c["objs"][1] == f_mb
        assert d["objs"][1] == pq_mb < p_mb and d["prune"] == {"size_mb": pq_mb, "sparsity": 0.8} and d["size_fp32_mb"] == f_mb
        assert d["quant"] == {"size_mb": G.quant_size_mb(g, 0, CLASSES, 8), "bits": 8}
        assert a["objs"][0] == b["objs"][0] and a["objs"][2] == b["objs"][2], "objective only moves the size"
        assert a["CV"] == max(0.0, on.min_accuracy + a["objs"][0]) + max(0.0, p_mb - on.max_model_size) + max(0.0, a["objs"][2] - on.max_fpr)
        assert b["CV"] == max(0.0, on.min_accuracy + b["objs"][0]) + max(0.0, f_mb - on.max_model_size) + max(0.0, b["objs"][2] - on.max_fpr)
    assert any(a["CV"] != b["CV"] for a, b in zip(res_on, res_add)), "the size constraint reads the pruned size"
    # train_model: candidate 0 again, its invariant, the file round trip, and plain fp32 scoring of the pruned model
    tm = ev.train_model(hps[0], ev.last_seeds[0])
    assert (-tm.objectives["acc"], tm.objectives["fpr"]) == (res_add[0]["objs"][0], res_add[0]["objs"][2])
    rows = PR.prune_table(pop[0], 0, CLASSES)
    assert tm.prune_sparsity == 0.8 and tm.prune_k.tolist() == [PR.row_k(r, 0.8) for r in rows] and tm.quant_codes is None
    rep = tm.sparsity_report()
    assert rep["total"]["zeros"] >= rep["total"]["k"] > 0 and 0.8 - 1e-3 < rep["total"]["sparsity"] < 1.0
    X = ev.X_val
    with NetSession(pop[0], add, T_, F_, ev.last_seeds[0]) as net:
        net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
        want = host(net.predict_logits(X))
        assert same_bits(net.get_pruned()[0], tm.params)
        assert not same_bits(net.get_params(), tm.params)
    assert same_bits(host(tm.logits(X, base)), want), "no option set: the fp32 paths score the sparse model"
    path = tmp_path / "sparse.npz"
    tm.save(path)
    back = TrainedModel.load(path)
    assert same_bits(back.params, tm.params) and back.prune_sparsity == 0.8 and np.array_equal(back.prune_k, tm.prune_k)
    assert back.sparsity_report() == rep
    with back.session(base) as s:
        assert same_bits(host(s.predict_logits(X)), want), "the loaded model's session scores the same logits"
    print(f"\n  [prune total] module wall time so far {time.time() - T0:.1f}s")
