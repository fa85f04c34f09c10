"""GPU: stale-memory parity.  Every device buffer of a candidate comes from the process-wide cache of csrc/net.hip, which hands
buffers out with whatever they held: "every consumer writes before it reads".  This module holds that sentence.  The criterion
needs no tolerance: EVERY RESULT THE LIBRARY RETURNS IS BIT-IDENTICAL WHATEVER BYTES ITS POOLED BUFFERS HELD WHEN THEY WERE
HANDED OUT.

CMOOP_POOL_FILL=<byte> (read at each allocation) fills every pooled device buffer, every pinned host buffer and every scratch
allocation of the kernel-level entry points before it is returned.  Each case runs unset and under three fills:

  0x00  what a fresh allocation usually looks like -- the masking case;
  0xFF  every float a NaN: catches 0 * stale, stale operands of sums, unwritten outputs;
  0x7F  every float 3.39e38, finite: catches reads a `> 0` gate or a max swallows as NaN-false (as uint8 / int32 / double a large
        ordinary value).

and asserts equality of bytes against the unset run, plus np.isfinite on it.  Only regions the API defines are compared.  The
nets are chosen with the host-only launch plan, asserted before anything is launched.  One case needs no knob at all: a net
trained after a different, larger net (driven to NaN) has handed its buffers back gives the bits it gave before.

A difference under a fill is a read of memory the consumer did not write: a finding, not a tolerance question (DESIGN.md,
"Stale-memory parity").  Run with -s for the launch-path variants reached and the time (profiles/stale_memory_parity.txt)."""
import ctypes as C
import dataclasses
import functools
import os
import time

import numpy as np
import pytest
import torch

import _elem_reference as R
from _sweep_shapes import SWEEP_CONVS, integer_regime_is_exact
from cmoop_audio_processing_amd import (AugmentConfig, DistillConfig, EmaConfig, EvalConfig, LossConfig, OptimConfig,
                                        PopulationEvaluator, _lib, frontend)
from cmoop_audio_processing_amd.session import NetSession
from test_gpu_dwconv import integers as dw_integers, run as dw_run
from test_gpu_elem_kernels import bn_bwd, bn_train_fwd
from test_gpu_geometry_sweep import _operands as conv_operands, _reference as conv_reference
from test_gpu_net import make_data, make_split
from test_gpu_optim import MIXED, Arena, grad_finish

pytestmark = pytest.mark.gpu

P = _lib.ptr
VAR = "CMOOP_POOL_FILL"
FILLS = (None, "0x00", "0x7F", "0xFF")         # None: the variable unset -- the plain path every other run is held against
T0 = time.time()
#: set by the first runtime error of a device call (a CmoopError, or a fault torch meets in a later copy): every later case skips
DEVICE_ERROR = []


@pytest.fixture(autouse=True)
def stop_after_a_device_error():
    if DEVICE_ERROR:
        pytest.skip(f"stopped at the first device error: {DEVICE_ERROR[0]}")
    yield


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---- the helper: one closure under each fill -----------------------------------------------------------------------------------
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


def flatten(x, path="", out=None):
    """A result (dicts, sequences, tensors, arrays, numbers) -> {path: (dtype, shape, bytes)}; floats travel as float64 bits."""
    out = {} if out is None else out
    if isinstance(x, dict):
        for k in sorted(x):
            flatten(x[k], f"{path}.{k}", out)
    elif isinstance(x, (list, tuple)):
        for i, v in enumerate(x):
            flatten(v, f"{path}[{i}]", out)
    else:
        if isinstance(x, torch.Tensor):
            x = x.detach().cpu().numpy()
        a = np.ascontiguousarray(x)
        assert a.dtype != object, (path, type(x))
        out[path] = (a.dtype.str, a.shape, a.tobytes())
    return out


def is_finite(entry):
    dt, shape, raw = entry
    a = np.frombuffer(raw, np.dtype(dt))
    return a.dtype.kind != "f" or bool(np.isfinite(a).all())


def n_differ(a, b):
    x, y = np.frombuffer(a[2], np.uint8), np.frombuffer(b[2], np.uint8)
    return int((x != y).sum()) if x.size == y.size else -1


def under_fills(run, fills=FILLS):
    """run() under each fill -> {fill: flattened result}"""
    out = {}
    for fill in fills:
        try:
            with pool_fill(fill):
                out[fill] = flatten(run())
            torch.cuda.synchronize()
        except RuntimeError as e:         # a finding to diagnose from the code, not something to run again
            DEVICE_ERROR.append(f"{VAR}={fill}: {type(e).__name__}: {e}")
            raise
    return out


def assert_fill_parity(results, what):
    """Every entry of every filled run has the bytes of the unset run, and every float of the unset run is finite."""
    plain = results[None]
    assert plain, what
    bad = [k for k, v in plain.items() if not is_finite(v)]
    assert not bad, f"{what}: non-finite values in the plain run: {bad}"
    diff = {}
    for fill, res in results.items():
        assert sorted(res) == sorted(plain), (what, fill)
        d = {k: n_differ(plain[k], res[k]) for k in plain if plain[k] != res[k]}
        if d:
            diff[f"{VAR}={fill}"] = d
    assert not diff, f"{what}: these results differ from the plain run (bytes that differ, per fill): {diff}"


# ---- 1. net level --------------------------------------------------------------------------------------------------------------
CLASSES, SEED = 10, 7


def variant_class(name):
    """'igemm_fwd_kernel<128, 16, 16, 4, 0>+sk+tab' -> 'igemm_fwd_kernel+sk+tab': the launch path without the tile sizes."""
    base, _, rest = name.partition("<")
    return base + (rest.partition(">")[2] if rest else "")


#: (gene, variant, T, F, batch, launch-path variants its steps must reach -- asserted from the host-only plan before anything is
#: launched).  The first five are the smallest nets that reach each variant; then topology B with BatchNorm and dropout (the fused
#: BN-pool kernels, the skip projection's accumulating dgrad into an aliased gradient buffer), the two depthwise-separable
#: topologies (slabs whose slice count is not monotone in the batch) and a net without BatchNorm.
NETS = [
    ((16, 3, 1, 1, 1, 0), "A", 21, 12, 3, ("igemm_fwd_kernel+sk+tab", "igemm_fwd_kernel+stats+tab", "igemm_fwd_kernel+tab",
                                          "igemm_wgrad_kernel+tab", "igemm_wgrad_kernel+tab+slabs")),
    ((64, 3, 1, 1, 1, 0), "A", 41, 20, 3, ("halo_wgrad_kernel+slabs",)),
    ((16, 3, 1, 1, 1, 0), "A", 101, 40, 13, ("halo_fwd_kernel", "halo_fwd_kernel+stats")),
    ((64, 5, 0, 2, 1, 0), "A", 41, 20, 13, ("igemm_fwd_kernel+bal+tab",)),
    ((64, 3, 1, 3, 4, 1), "A", 41, 20, 32, ("halo_fwd_kernel+bal",)),
    ((16, 5, 1, 2, 3, 1), "B", 21, 12, 8, ()),
    ((16, 3, 1, 1, 2, 1), "A_ds", 21, 12, 8, ()),
    ((16, 5, 1, 2, 3, 1), "B_ds", 21, 12, 8, ()),
    ((16, 5, 0, 1, 2, 0), "A", 21, 12, 8, ()),
]
REQUIRED = {v for case in NETS for v in case[5]}
#: variant classes the host plan names for the cases that ran, and the full names behind them
REACHED, REACHED_NAMES = set(), set()


def net_cfg(variant, B):
    # eval_batch > batch: the activations hold rows the train steps never write; the validation set is no multiple of it
    return EvalConfig(variant=variant, classes=CLASSES, batch=B, eval_batch=B + 2)


def step_batches(B):
    return (B, B - B // 3, B)                   # full, partial, full: slice and tile counts change, a slab's tail is stale there


def planned(gene, variant, T, F, B):
    cfg = net_cfg(variant, B).to_struct()
    names = set()
    for b in set(step_batches(B)):
        names |= set(_lib.net_launch_plan(gene, cfg, T, F, b, 1))
    for b in (B + 2, 1):                        # the inference batches of a validation set of 2 (B + 2) + 1 rows
        names |= set(_lib.net_launch_plan(gene, cfg, T, F, b, 0))
    return names


@pytest.mark.parametrize("gene,variant,T,F,B,reaches", NETS, ids=[f"{'.'.join(map(str, c[0]))}-{c[1]}-{c[2]}x{c[3]}-B{c[4]}" for c in NETS])
def test_net_results_do_not_depend_on_what_the_pooled_buffers_held(gene, variant, T, F, B, reaches):
    """A fresh net under each fill: three train steps (full, partial, full), then every read-out."""
    names = planned(gene, variant, T, F, B)
    classes = {variant_class(n) for n in names}
    for v in reaches:
        assert v in classes, (v, sorted(names))
    Bs = step_batches(B)
    EB = B + 2
    X, y = make_data(sum(Bs), T, F, CLASSES, 11)
    Xv, yv = make_data(2 * EB + 1, T, F, CLASSES, 12)
    Xd, yd, Xvd, yvd = dev(X), dev(y), dev(Xv), dev(yv)
    rs = np.random.RandomState(13)
    stream = dev(rs.randn(T + 2 * (EB + 1), F).astype(np.float32))      # EB + 2 windows at hop 2: a full chunk and one window
    mean, scale = rs.randn(F), 0.5 + rs.rand(F)
    cfg = net_cfg(variant, B)

    def run():
        with NetSession(gene, cfg, T, F, SEED) as net:
            row0 = 0
            for b in Bs:
                net.train_step(Xd, yd, None, row0=row0, B=b)
                row0 += b
            loss, acc, preds = net.evaluate(Xvd, yvd)
            return dict(state=net.get_state(), grads=net.get_grads(), train_metrics=net.train_metrics(), eval_loss=loss, eval_acc=acc,
                        preds=preds, proba=net.predict_proba(Xvd), logits=net.predict_logits(Xvd),
                        stream=net.predict_stream(stream, 2, mean=mean, scale=scale))

    assert_fill_parity(under_fills(run), (gene, variant, T, F, B))
    REACHED.update(classes)
    REACHED_NAMES.update(names)


def test_the_net_cases_reach_every_launch_path_variant_they_were_chosen_for():
    """Over the list, the union of the host plan's names holds every variant a case was picked for."""
    if not REACHED:
        pytest.skip("run together with the net cases of this module (they fill the set)")
    print(f"\n{len(REACHED_NAMES)} launch-path variants planned for the net cases, in {len(REACHED)} classes:")
    for n in sorted(REACHED_NAMES):
        print("  " + n)
    print(f"module time so far {time.time() - T0:.1f} s")
    assert REQUIRED <= REACHED, sorted(REQUIRED - REACHED)


# ---- 2. the training options ---------------------------------------------------------------------------------------------------
OT, OF, OCLASSES, OBATCH = 21, 12, 4, 8        # tests/test_gpu_train_options.py's sizes
N_TRAIN, N_VAL = 37, 19                         # a partial last train batch; a validation split that is no multiple of eval_batch
GENE = (16, 3, 1, 1, 1, 1)                      # BatchNorm, residual, dropout
FIT = EvalConfig(variant="A", classes=OCLASSES, batch=OBATCH, eval_batch=16, epochs=6, early_stop=True, patience=2, restore_best=True,
                 acc_readout="evaluate", fpr_variant="v1", shuffle=True)
OPTIONS = dict(
    augment=AugmentConfig(p=0.5, time_shift=3, time_masks=2, time_mask_max=4, freq_masks=2, freq_mask_max=3, noise_std=0.1),
    loss=LossConfig(mixup_alpha=0.2, mixup_p=0.5, label_smoothing=0.1, class_weight=(0.5, 0.75, 1.0, 1.25)),
    distill=DistillConfig(alpha=0.7, temperature=4.0),
    optim=OptimConfig(schedule="cosine", warmup_steps=2, warmup_start=0.25, decay_steps=6, alpha=0.1, weight_decay=0.05, global_clipnorm=0.05),
    ema=EmaConfig(0.9),
)
OPTION_CASES = {"all": OPTIONS, "none-unshuffled": {}, **{k: {k: v} for k, v in OPTIONS.items()}}


@functools.lru_cache(maxsize=None)
def fit_split():
    return tuple(dev(a) for a in make_split(N_TRAIN, N_VAL, OT, OF, OCLASSES, 31, noise=2.5, label_noise=0.3))


@functools.lru_cache(maxsize=None)
def teacher():
    return dev((2.0 * np.random.RandomState(21).randn(N_TRAIN, OCLASSES)).astype(np.float32))


@pytest.mark.parametrize("case", list(OPTION_CASES))
def test_fit_and_run_epoch_with_the_options_on_do_not_depend_on_what_the_pooled_buffers_held(case):
    """One fit() with early stop and restore_best, and two epochs of run_epoch on the device-state path, with every option on,
    with each alone (the lazily allocated buffers differ per option) and with none (unshuffled: the pinned index buffer)."""
    opts = OPTION_CASES[case]
    cfg = dataclasses.replace(FIT, shuffle=case != "none-unshuffled", **opts)
    Xtr, ytr, Xva, yva = fit_split()

    def session():
        net = NetSession(GENE, cfg, OT, OF, SEED)
        if "distill" in opts:
            net.set_distill(teacher_logits=teacher())
        return net

    def read(net):
        out = dict(state=net.get_state(), optim=net.optim_stats(), grads=net.get_grads())
        if "ema" in opts:
            out["ema"] = net.get_ema()
        return out

    def run():
        with session() as net:
            record = net.fit(Xtr, ytr, Xva, yva)
            fit = dict(read(net), record=record, params=net.get_params())
        with session() as net:
            for epoch in range(2):
                net.run_epoch(Xtr, ytr, epoch)
            epochs = dict(read(net), train_metrics=net.train_metrics(), evaluate=net.evaluate(Xva, yva))
        return dict(fit=fit, run_epoch=epochs)

    results = under_fills(run)
    rec = {k: np.frombuffer(results[None][f".fit.record.{k}"][2], np.dtype(results[None][f".fit.record.{k}"][0])) for k in ("epochs_run", "best_epoch")}
    print(f"\n{case}: fit ran {int(rec['epochs_run'][0])} epochs, best epoch {int(rec['best_epoch'][0])}")
    assert_fill_parity(results, case)


# ---- 3. the population path ----------------------------------------------------------------------------------------------------
POP = [(16, 3, 1, 1, 1, 0), (16, 3, 1, 1, 1, 1), (16, 5, 0, 1, 2, 0), (16, 3, 1, 2, 1, 0)]
POP_SEEDS = [5, 6, 7, 8]


def population_columns(ev, genes, seeds):
    """One population call of the evaluator's own symbol -> (acc, size_mb, fpr, epochs_run, val_loss), one row per gene."""
    n = len(genes)
    g = np.ascontiguousarray(np.array(genes, np.int32))
    sd = np.array(seeds, np.uint32)
    acc, size, fpr, vl = (np.zeros(n, np.float64) for _ in range(4))
    ep = np.zeros(n, np.int32)
    cfg, ds = ev.config.to_struct(), ev._dataset()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_eval_population_avg(C.byref(cfg), None, None, None, None, None, C.byref(ds), P(g), P(sd), C.c_int32(n), None,
                                                    None, P(acc), P(size), P(fpr), P(ep), P(vl), None, None))
    return [acc, size, fpr, ep, vl]


def test_population_results_do_not_depend_on_the_fill_or_on_the_order_of_the_genes():
    """Four genes on two slots, in order and reversed: whichever worker's finished candidate a buffer comes from, the five
    result columns are those of the plain run, row for row by gene; evaluate_genes returns the same first four."""
    cfg = dataclasses.replace(FIT, epochs=2, early_stop=False, n_slots=2, seed=POP_SEEDS[0])
    ev = PopulationEvaluator(*fit_split(), cfg)

    def run():
        fwd = population_columns(ev, POP, POP_SEEDS)
        rev = population_columns(ev, POP[::-1], POP_SEEDS[::-1])
        rows = ev.evaluate_genes(POP, POP_SEEDS)
        return dict(forward=fwd, reversed=[c[::-1].copy() for c in rev], evaluate_genes=[rows[:, k].copy() for k in range(3)] + [rows[:, 3].astype(np.int32)])

    results = under_fills(run)
    assert_fill_parity(results, "population")
    for fill, res in results.items():
        for k in range(5):
            assert res[f".forward[{k}]"] == res[f".reversed[{k}]"], (fill, k, "the order of the genes changed a result")
        for k in range(4):
            assert res[f".forward[{k}]"] == res[f".evaluate_genes[{k}]"], (fill, k)


# ---- 4. history, without the knob ----------------------------------------------------------------------------------------------
def test_a_net_trained_after_a_larger_one_gave_its_buffers_back_repeats_its_first_run():
    """The production situation itself, and a guard against a bug of the knob's own: net Y; then a different, larger net X --
    same feature size and batch, so that the cache hands it Y's buffers and, once it is closed, hands Y's successor a mixture of
    both -- trained on inputs that drive it to NaN; then Y again.  The two Y results are equal."""
    B, T, F = 8, 21, 12
    Bs = step_batches(B)
    X, y = make_data(sum(Bs), T, F, CLASSES, 11)
    Xd, yd = dev(X), dev(y)
    Xbad = dev((X * np.float32(1e30)).astype(np.float32))
    cfg = net_cfg("A", B)

    def train(gene, variant, Xin, seed):
        with NetSession(gene, dataclasses.replace(cfg, variant=variant), T, F, seed) as net:
            row0 = 0
            for b in Bs:
                net.train_step(Xin, yd, None, row0=row0, B=b)
                row0 += b
            loss, acc, preds = net.evaluate(Xd, yd)
            return dict(state=net.get_state(), grads=net.get_grads(), train_metrics=net.train_metrics(), eval_loss=loss, preds=preds,
                        proba=net.predict_proba(Xd))

    with pool_fill(None):
        first = flatten(train((16, 3, 1, 1, 1, 0), "A", Xd, SEED))
        other = flatten(train((16, 5, 1, 2, 3, 1), "B", Xbad, SEED + 1))
        second = flatten(train((16, 3, 1, 1, 1, 0), "A", Xd, SEED))
    assert not is_finite(other[".state.params"]), "the net in between left non-finite values behind"
    assert_fill_parity({None: first, "after X": second}, "Y, X, Y")


# ---- 5. kernel level, through the scratch of the kernel-level entry points -----------------------------------------------------
def conv_plan(op, case, stats=0):
    buf = C.create_string_buffer(200)
    _lib.check(_lib.lib().cmoop_conv_launch_plan(op, *case, stats, buf, 200))
    return buf.value.decode()


#: the workspace-bearing conv launches: (what, predicate on the host plan of a sweep case); the first case of each kind runs
CONV_KINDS = {
    "split-K forward": lambda c: "+sk" in conv_plan(0, c),
    "split-K dgrad, mask in the combine": lambda c: "+sk" in conv_plan(1, c),
    "forward with the statistics epilogue": lambda c: "+stats" in conv_plan(0, c, 1),
    "weight gradient through slabs": lambda c: conv_plan(2, c).startswith("igemm_wgrad") and "+slabs" in conv_plan(2, c),
    "halo weight gradient through slabs": lambda c: conv_plan(2, c).startswith("halo_wgrad") and "+slabs" in conv_plan(2, c),
}


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


@pytest.mark.parametrize("kind", list(CONV_KINDS))
def test_conv_launches_do_not_depend_on_what_their_scratch_held(kind):
    """cmoop_conv_fwd_trainer (with the statistics epilogue; with ReLU) and cmoop_conv_bwd_trainer in the sweep's exact integer
    regime: equal bytes under every fill, and the plain run EQUALS the float64 reference."""
    case = next(c for c in SWEEP_CONVS if CONV_KINDS[kind](c))
    B, H, W, Cin, Cout, KS, stride = case
    assert integer_regime_is_exact(*case)
    x, w, b, dy = conv_operands("integer", *case, seed=1000 + B + H + Cin + Cout + KS)
    ref = conv_reference(x, w, b, dy, stride)
    OH, OW = -(-H // stride), -(-W // stride)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    L = _lib.lib()
    launched = []

    def run():
        y, y2, dx = nan(B, OH, OW, Cout), nan(B, OH, OW, Cout), nan(B, H, W, Cin)
        dw, db = nan(Cout, KS, KS, Cin), nan(Cout)
        cs, cq, fused = np.zeros(Cout), np.zeros(Cout), C.c_int32(-1)
        torch.cuda.synchronize()
        _lib.check(L.cmoop_conv_fwd_trainer(P(xd), P(wd), P(bd), P(y), B, H, W, Cin, Cout, KS, stride, 0, P(cs), P(cq), C.byref(fused)))
        launched.extend(_lib.last_kernels())
        _lib.check(L.cmoop_conv_fwd_trainer(P(xd), P(wd), P(bd), P(y2), B, H, W, Cin, Cout, KS, stride, 1, None, None, None))
        launched.extend(_lib.last_kernels())
        _lib.check(L.cmoop_conv_bwd_trainer(P(xd), P(wd), P(dyd), P(dx), P(dw), P(db), B, H, W, Cin, Cout, KS, stride, 1))
        launched.extend(_lib.last_kernels())
        torch.cuda.synchronize()
        return dict(y=y, relu_y=y2, dx=dx, dw=dw, db=db, colsum=cs, colsumsq=cq, fused=fused.value)

    results = under_fills(run)
    print(f"\n{kind}: {case} {sorted(set(launched))}")
    assert_fill_parity(results, (kind, case))
    with pool_fill(None):
        got = run()
    want = dict(ref, relu_y=np.maximum(ref["y"], 0))
    for k, v in want.items():
        assert np.array_equal(got[k].cpu().numpy().astype(np.float64), v), (kind, case, k)


def test_first_layer_weight_gradient_with_empty_workgroups_does_not_depend_on_its_scratch():
    """(33, 5, 4, 64, 3) of tests/test_gpu_kernels.py: more row chunks than rows for some samples' share."""
    B, H, W, Cout, KS = 33, 5, 4, 64, 3
    rs = np.random.RandomState(3)
    xd = dev(rs.randint(0, 4, (B, H, W, 1)).astype(np.float32))
    wd = dev(rs.randint(-2, 3, (Cout, KS, KS, 1)).astype(np.float32))
    dyd = dev(rs.randint(-2, 3, (B, H, W, Cout)).astype(np.float32))

    def run():
        dw, db, dx = nan(Cout, KS, KS, 1), nan(Cout), torch.zeros((B, H, W, 1), device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_conv_bwd(P(xd), P(wd), P(dyd), P(dx), P(dw), P(db), B, H, W, 1, Cout, KS, 1, 0))
        torch.cuda.synchronize()
        return dict(dw=dw, db=db)

    assert_fill_parity(under_fills(run), "first-layer weight gradient")


def test_depthwise_backward_with_several_slices_does_not_depend_on_its_scratch():
    B, H, W, Cn, K = 5, 26, 10, 64, 3
    assert _lib.dwconv_wgrad_slices(B, H, W, Cn, K) > 1
    x, w, dy = dw_integers(B, H, W, Cn, K, 9)
    assert_fill_parity(under_fills(lambda: dw_run(x, w, dy, mask_relu=True)), "depthwise backward")


def test_batchnorm_with_several_blocks_does_not_depend_on_its_scratch():
    M, Cn = 2080, 64
    assert R.colreduce_blocks(M, Cn) > 1
    x, gamma, beta, eps, _, _ = R.exact_bn_input(M, Cn, 1000 + M + Cn)
    dy = R.exact_grad((M, Cn), 2000 + M)
    ref = R.bn_train_ref(x, gamma, beta, eps, 1)
    xd, gd, bd, dyd = dev(x), dev(gamma), dev(beta), dev(dy)
    md, isd = dev(ref["mean"].astype(np.float32)), dev(ref["invstd"].astype(np.float32))

    def run():
        mm, mv = dev(np.full(Cn, 4.0, np.float32)), dev(np.full(Cn, 8.0, np.float32))
        fwd = bn_train_fwd(xd, gd, bd, mm, mv, eps, 0.75, 1, 0)
        return dict(fwd=fwd, mm=mm, mv=mv, bwd=bn_bwd(dyd, xd, md, isd, gd, 1, 0))

    assert_fill_parity(under_fills(run), "batchnorm")


def test_grad_finish_does_not_depend_on_its_scratch():
    ar = Arena(MIXED)
    rs = np.random.RandomState(50)
    slab = rs.randint(-1, 2, ar.slab_floats).astype(np.float32)
    _, g_in = ar.slab_sums(slab, rs.randint(-3, 4, ar.total).astype(np.float32))
    slabd = dev(slab)
    kinds = rs.randint(0, 2, ar.total).astype(np.uint8)
    assert_fill_parity(under_fills(lambda: [grad_finish(ar, g_in, slabd, k, clip) for k in (None, kinds) for clip in (0.0, 0.125)]),
                       "grad_finish")


def test_front_end_launches_do_not_depend_on_their_workspace():
    """cmoop_standardize_fit over several blocks, cmoop_pcen_stream over several chunks (its pooled workspace) and
    cmoop_logmel_stream."""
    rs = np.random.RandomState(4)
    feats = dev(rs.randn(48, 26, 40).astype(np.float32))
    assert R.colreduce_blocks(48 * 26, 40) > 1
    T = 3000
    assert frontend.pcen_stream_plan(T)[1] > 1
    power = dev((rs.rand(T, 40) ** 2).astype(np.float32))
    wav = dev((0.1 * rs.randn(16000)).astype(np.float32))

    def run():
        return dict(standardize=frontend.standardize_fit(feats), pcen=frontend.pcen(power), logmel=frontend.log_mel_stream(wav))

    assert_fill_parity(under_fills(run), "front end")


# ---- 6. the knob itself --------------------------------------------------------------------------------------------------------
def test_a_bad_value_raises_naming_the_variable_and_unsetting_restores_the_plain_path():
    gene, T, F, B = (16, 3, 1, 1, 1, 0), 21, 12, 3
    X, y = make_data(B, T, F, CLASSES, 11)
    Xd, yd = dev(X), dev(y)
    feats = dev(np.random.RandomState(4).randn(48, 26, 40).astype(np.float32))

    def run():
        with NetSession(gene, net_cfg("A", B), T, F, SEED) as net:
            net.train_step(Xd, yd, None, row0=0, B=B)
            return dict(state=net.get_state(), scaler=frontend.standardize_fit(feats))

    with pool_fill(None):
        first = flatten(run())
    for bad in ("256", "-1", "0x100", "1.5", "ff", "0x", "12 "):
        with pool_fill(bad):
            with pytest.raises(_lib.CmoopError, match=VAR):
                NetSession(gene, net_cfg("A", B), T, F, SEED)
            with pytest.raises(_lib.CmoopError, match=VAR):
                frontend.standardize_fit(feats)
    for good in ("0", "255", "0xff", "127", ""):          # empty: unset
        with pool_fill(good):
            assert flatten(run()) == first, good
    with pool_fill(None):
        assert flatten(run()) == first
    print(f"\nmodule time {time.time() - T0:.1f} s")
