"""The training options as ONE record from EvalConfig down to Net: the six cmoop_eval_population* symbols are one call, the
evaluator reaches it through cmoop_eval_population_opt alone, and NULL, None or a disabled struct is the call without the
option, byte for byte."""
import ctypes as C
import dataclasses
import functools
import itertools
import threading

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import AugmentConfig, DistillConfig, LossConfig, OptimConfig, PopulationEvaluator, _lib, genes as G
from cmoop_audio_processing_amd.session import NetSession
from test_gpu_net import make_split
from test_gpu_optim import CFG, CLASSES, FULL, F_, POP, T_

pytestmark = pytest.mark.gpu

P = _lib.ptr
N_TRAIN, N_VAL = 40, 16
SEEDS = [5, 6, 7, 8]
BASE = dataclasses.replace(CFG, seed=SEEDS[0], n_slots=2)          # 21 x 12, 4 classes, batch 8 / 16, 2 epochs, no early stop
AUG, LOSS, KD = AugmentConfig(time_shift=3), LossConfig(label_smoothing=0.1), DistillConfig(alpha=0.7, temperature=4.0)
ON = dataclasses.replace(BASE, augment=AUG, loss=LOSS, distill=KD, optim=FULL)


@functools.lru_cache(maxsize=None)
def split():
    return make_split(N_TRAIN, N_VAL, T_, F_, CLASSES, 31)


@functools.lru_cache(maxsize=None)
def teacher():
    return torch.from_numpy((2.0 * np.random.RandomState(21).randn(N_TRAIN, CLASSES)).astype(np.float32)).cuda()


def evaluator(cfg):
    ev = PopulationEvaluator(*split(), cfg)
    if cfg.distill is not None:
        ev.set_teacher(teacher())
    return ev


def longest_first_pull():
    """A local twin of the library's own queue: candidate indices by falling closed-form cost, then -1."""
    cost = [G.fwd_flops_per_sample(g, 0, CLASSES, T_, F_) for g in POP]
    order = sorted(range(len(POP)), key=lambda i: (-cost[i], i))
    ctr, lock = itertools.count(), threading.Lock()

    def pull():
        with lock:
            j = next(ctr)
        return order[j] if j < len(order) else -1
    return pull


def ref(st):
    return C.byref(st) if st is not None else None


def call(symbol, ev, cfg, structs=(None, None, None, None), pull=None):
    """One direct call of a population symbol -> the bytes of (acc, size_mb, fpr, epochs_run, val_loss); `structs` are the
    (augment, loss, distill, optim) structs, of which the symbol takes its leading ones (the rest must be None)."""
    n = len(POP)
    genes = np.ascontiguousarray(np.array(POP, np.int32))
    seeds = np.array(SEEDS, np.uint32)
    acc, size, fpr, vl = (np.zeros(n, np.float64) for _ in range(4))
    ep, done = np.zeros(n, np.int32), np.zeros(n, np.int32)
    c, ds = cfg.to_struct(), ev._dataset()
    data = (C.byref(ds), P(genes), P(seeds), C.c_int32(n))
    outs = (P(acc), P(size), P(fpr), P(ep), P(vl), None)
    cb = _lib.NEXT_FN(lambda _ctx: pull()) if pull is not None else None
    n_opts = {"": 0, "_pull": 0, "_aug": 1, "_ex": 2, "_kd": 3, "_opt": 4}[symbol]
    assert all(s is None for s in structs[n_opts:]), "the symbol cannot carry these options"
    torch.cuda.synchronize()
    fn = getattr(_lib.lib(), "cmoop_eval_population" + symbol)
    if symbol == "":
        assert pull is None
        rc = fn(C.byref(c), *data, *outs)
    elif symbol == "_pull":
        rc = fn(C.byref(c), *data, cb, None, *outs, P(done))
    else:
        rc = fn(C.byref(c), *(ref(s) for s in structs[:n_opts]), *data, C.cast(cb, C.c_void_p) if cb is not None else None, None,
                *outs, P(done) if cb is not None else None)
    _lib.check(rc)
    if pull is not None:
        assert done.tolist() == [1] * n, "every candidate is trained by the one process that pulls"
    return tuple(a.tobytes() for a in (acc, size, fpr, ep, vl))


def evaluator_bytes(rows):
    """evaluate_genes' [n, 5] rows (or evaluate_genes_pull's dict of them) -> the bytes of (acc, size_mb, fpr, epochs_run)."""
    if isinstance(rows, dict):
        assert sorted(rows) == list(range(len(POP)))
        rows = np.stack([rows[i] for i in range(len(POP))])
    return tuple(np.ascontiguousarray(rows[:, k]).tobytes() for k in range(3)) + (rows[:, 3].astype(np.int32).tobytes(),)


@functools.lru_cache(maxsize=None)
def off_bytes():
    return call("", evaluator(BASE), BASE)


def test_options_off_the_six_symbols_and_the_evaluator_are_one_call():
    ev = evaluator(BASE)
    off = off_bytes()
    assert np.frombuffer(off[3], np.int32).tolist() == [2] * len(POP)
    assert call("_pull", ev, BASE, pull=longest_first_pull()) == off
    for symbol in ("_aug", "_ex", "_kd", "_opt"):
        assert call(symbol, ev, BASE) == off, symbol
        assert call(symbol, ev, BASE, pull=longest_first_pull()) == off, symbol + " with a callback"
    assert BASE.option_structs(T_, F_, None, N_TRAIN) == (None, None, None, None)
    assert evaluator_bytes(ev.evaluate_genes(POP, SEEDS)) == off[:4]
    assert evaluator_bytes(ev.evaluate_genes_pull(POP, SEEDS, longest_first_pull())) == off[:4]
    assert evaluator_bytes(ev.evaluate_genes_pull(POP, SEEDS, longest_first_pull(), workers=1)) == off[:4]


def test_all_four_options_on_reach_the_trainer_the_same_way_by_every_route():
    ev = evaluator(ON)
    structs = ON.option_structs(T_, F_, teacher(), N_TRAIN)
    singles = (ON.augment_struct(T_, F_), ON.loss_struct(), ON.distill_struct(teacher(), N_TRAIN), ON.optim_struct())
    assert [bytes(s) for s in structs] == [bytes(s) for s in singles] and all(s is not None for s in structs)
    for name, st in zip(("augment", "loss", "distill", "optim"), singles):     # each option alone: the one struct, three Nones
        alone = dataclasses.replace(BASE, **{name: getattr(ON, name)}).option_structs(T_, F_, teacher(), N_TRAIN)
        assert [bytes(s) if s is not None else None for s in alone] == [bytes(s) if s is st else None for s in singles], name
    direct = call("_opt", ev, ON, structs)
    assert direct[:4] != off_bytes()[:4] and direct[4] != off_bytes()[4], "the options change the fit"
    assert call("_opt", ev, ON, structs, pull=longest_first_pull()) == direct
    assert evaluator_bytes(ev.evaluate_genes(POP, SEEDS)) == direct[:4]
    assert evaluator_bytes(ev.evaluate_genes_pull(POP, SEEDS, longest_first_pull())) == direct[:4]
    # a session from the same config is candidate 0 of that call
    with NetSession(POP[0], ON, T_, F_, SEEDS[0]) as net:
        net.set_distill(teacher_logits=teacher())
        r = net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
        assert net.optim_stats()["path"] == 1
    acc, fpr, ep = (np.frombuffer(direct[k], dt)[0] for k, dt in ((0, np.float64), (2, np.float64), (3, np.int32)))
    assert (r["acc"], r["fpr"], r["epochs_run"]) == (acc, fpr, ep)
    with pytest.raises(ValueError, match="no teacher is set"):
        PopulationEvaluator(*split(), ON).evaluate_genes(POP, SEEDS)


def test_a_disabled_struct_for_every_option_is_options_off():
    ev = evaluator(BASE)
    disabled = (AugmentConfig()._struct(), LossConfig()._struct(), DistillConfig(alpha=0.0)._struct(teacher()), OptimConfig()._struct())
    assert not (AugmentConfig().enabled or LossConfig().enabled or DistillConfig(alpha=0.0).enabled or OptimConfig().enabled)
    assert bytes(disabled[3]) == bytes(C.sizeof(_lib.Optim))
    assert call("_opt", ev, BASE, disabled) == off_bytes()
    assert call("_opt", ev, BASE, disabled, pull=longest_first_pull()) == off_bytes()
    assert call("_kd", ev, BASE, disabled[:3] + (None,)) == off_bytes()
    off_cfg = dataclasses.replace(BASE, augment=AugmentConfig(), loss=LossConfig(), distill=DistillConfig(alpha=0.0), optim=OptimConfig())
    assert off_cfg.option_structs(T_, F_, None, N_TRAIN) == (None, None, None, None)
    assert evaluator_bytes(evaluator(off_cfg).evaluate_genes(POP, SEEDS)) == off_bytes()[:4]
