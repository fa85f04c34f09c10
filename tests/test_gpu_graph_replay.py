"""GPU: the captured train step.  ``CMOOP_GRAPH=1`` captures a full-batch step of the fit loop once as a hipGraph and replays it
(``Net::train_step_stateful``, csrc/net.hip).  A capture freezes every host-side argument of its launches, so the risk is a
replay of a capture that no longer matches what the caller asked for: wrong numbers and no error.  The reference is the eager
device-state path, which other modules hold to the explicit-argument steps and to the float64 oracle (test_gpu_dsnet,
test_gpu_ema, test_gpu_optim, test_gpu_distill).  Same kernels, same arguments, no atomics: every comparison here is equality
in bytes, with no tolerance.

``CMOOP_GRAPH`` is read once per process, so the replay side runs in child processes: ONE for every session scenario, ONE for
the population call.  The eager side runs in this process and writes its records under a temporary directory; a child re-runs
the same scenario functions, compares bytes and checks ``cmoop_step_launch_counts`` against counts the test derives from each
scenario's own schedule (``Sched``) -- so a capture that silently never happens, or a replay that silently turns eager, fails
too.  A child that times out or dies on a signal stops the module: the remaining tests skip, nothing is retried.

Shapes: 21 x 12 features, 4 classes, batch 8, eval_batch 16, 52 training rows (6 full steps and a partial one of 4 per epoch;
the partial step and step 0 run eagerly between replays), 24 validation rows, shuffle on.

Measured on an MI355X (run with -s for the per-scenario counts): the module 5.5 s wall; the eager side 0.5 s; the session child
2.4 s wall (0.53 s in its 24 scenarios, the rest interpreter start, imports and library load); the population child 2.1 s wall
(0.19 s in the call).  No scenario takes more than 0.32 s, the first one included, which loads the kernels.

Against a build without the key comparison, scenario (c) differs from the eager run in 14 of its 24 arrays, from the first
epoch on the second tensor onwards, with 1 capture and 0 drops where the schedule gives 3 and 2.  Scenario (b) and the second
fit of (a) were never run against a library without the begin_fit fix: there a replay reads past the end of the old table.
Case 2 of the stale captures, the pooled index buffer that run_epoch took per call, cannot be forced from Python (the pool
usually hands the same block back); run_epoch now keeps the permutation in a buffer of the net, and the key holds its pointer.
"""
import json
import os
import subprocess
import sys
import time
import traceback

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import (ActQuantConfig, AugmentConfig, DistillConfig, EmaConfig, EvalConfig, LossConfig, OptimConfig,
                                        PopulationEvaluator, PruneConfig, QuantConfig, _lib)
from cmoop_audio_processing_amd.session import NetSession, epoch_permutation

GRAPH_ON = os.environ.get("CMOOP_GRAPH", "")[:1] == "1"
IS_CHILD = __name__ == "__main__"
pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(GRAPH_ON, reason="started under CMOOP_GRAPH=1: this process cannot be the eager side")]

# each child's time limit: four to five times its measured wall time, interpreter start, torch import and library load included
# (a first run on a busy machine varies by that much)
SESSION_CHILD_TIMEOUT = 12        # s; measured 2.4 s wall, of which 0.53 s in the 24 scenarios
POPULATION_CHILD_TIMEOUT = 10     # s; measured 2.1 s wall, of which 0.19 s in the population call

T, F, CLASSES, BATCH, EVAL_BATCH, N_TRAIN, N_VAL, N_SHORT, SEED = 21, 12, 4, 8, 16, 52, 24, 44, 1234
NETS = {"A": ((16, 3, 1, 1, 2, 1), "A"),          # BatchNorm and dropout
        "B": ((16, 3, 0, 2, 1, 0), "B"),
        "A_ds": ((16, 3, 1, 1, 1, 1), "A_ds")}
AUG = AugmentConfig(time_shift=3, time_masks=1, time_mask_max=4, freq_masks=1, freq_mask_max=3, noise_std=0.1)
LOSS = LossConfig(label_smoothing=0.1, mixup_alpha=0.2)
KD = DistillConfig(alpha=0.7, temperature=4.0)
FORBID = {"adamw": dict(optim=OptimConfig(schedule="cosine", warmup_steps=2, warmup_start=0.25, decay_steps=6, alpha=0.1,
                                          weight_decay=0.05)),
          "ema": dict(ema=EmaConfig(0.9)),
          "quant": dict(quant=QuantConfig(bits=8)),
          "prune": dict(prune=PruneConfig(sparsity=0.5)),
          "actquant": dict(act_quant=ActQuantConfig(bits=8))}
POP = [NETS["A"][0], (16, 3, 1, 1, 1, 0), (16, 5, 0, 1, 2, 0), (16, 3, 1, 2, 1, 0)]
POP_SEEDS = [5, 6, 7, 8]
COUNT_KEYS = ("eager", "replays", "captures", "drops")


def cfg(variant, **kw):
    return EvalConfig(**{**dict(variant=variant, classes=CLASSES, batch=BATCH, eval_batch=EVAL_BATCH, epochs=3, early_stop=False,
                                shuffle=True, n_slots=2, seed=SEED), **kw})


def make_data(n, seed):
    """n labelled rows: a class prototype plus unit noise (the prototypes are shared by every split)"""
    rs = np.random.RandomState(seed)
    proto = np.random.RandomState(99).randn(CLASSES, T, F).astype(np.float32)
    y = rs.randint(0, CLASSES, size=n).astype(np.int32)
    X = (0.8 * proto[y] + rs.randn(n, T, F)).astype(np.float32)
    return X, y


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def split(n, seed):
    X, y = make_data(n, seed)
    return dev(X), dev(y)


class Sched:
    """What the library must do under CMOOP_GRAPH=1, counted from the scenario's own schedule: a step of the fit loop is
    replayed when it is a full batch, not profiled and not the net's first (step >= 1); the first such step after the net was
    created or after its capture was dropped captures.  Eagerly the same steps are all launched."""

    def __init__(self, profile_every=0, capturable=True):
        self.pe, self.capturable = profile_every, capturable
        self.step, self.live = 0, False
        self.eager = self.replays = self.captures = self.drops = 0

    def epoch(self, n_rows, times=1):
        for _ in range(times):
            for s in range(0, n_rows, BATCH):
                full = min(BATCH, n_rows - s) == BATCH
                profiled = self.pe > 0 and self.step % self.pe == 0
                if self.capturable and full and not profiled and self.step >= 1:
                    if not self.live:
                        self.captures, self.live = self.captures + 1, True
                    self.replays += 1
                else:
                    self.eager += 1
                self.step += 1

    def explicit_steps(self, k):
        self.step += k              # train_step: host arguments, not the fit loop -- neither counted nor captured

    def key_change(self):
        """the capture, if there is one, no longer matches: a setter ran, the step budget was rebuilt, or the call's tensors
        or split length differ"""
        if self.live:
            self.drops, self.live = self.drops + 1, False

    def counts(self, replay):
        if replay:
            return dict(eager=self.eager, replays=self.replays, captures=self.captures, drops=self.drops)
        return dict(eager=self.eager + self.replays, replays=0, captures=0, drops=0)


def record(net, Xv, fit=None):
    st = net.get_state()
    loss_sum, correct = net.train_metrics(reset=False)
    r = {"params": st["params"], "m": st["m"], "v": st["v"], "counters": np.array([st["iterations"], st["steps"]], np.int64),
         "grads": net.get_grads(), "loss_sum": np.array([loss_sum], np.float64), "correct": np.array([correct], np.int64),
         "val_logits": net.predict_logits(Xv).cpu().numpy()}
    if fit is not None:
        r["fit"] = np.array([fit["acc"], fit["fpr"], fit["val_loss"]], np.float64)
        r["fit_epochs"] = np.array([fit["epochs_run"], fit["best_epoch"]], np.int64)
        r["val_loss_history"] = np.asarray(fit["val_loss_history"], np.float64)
        r["val_accuracy_history"] = np.asarray(fit["val_accuracy_history"], np.float64)
    return r


def session(net, **kw):
    gene, variant = NETS[net]
    return NetSession(gene, cfg(variant, **kw), T, F, SEED)


# ---- the scenarios: each -> ([(tag, record)], Sched) ---------------------------------------------------------------------------
def scenario_a(net):
    """fit(), 3 epochs; then a second fit() on the same session: begin_fit is re-entered, the capture and the tables go"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, yv = split(N_VAL, 2)
    sched, recs = Sched(), []
    with session(net, epochs=3) as s:
        recs.append(("fit1", record(s, Xv, s.fit(Xt, yt, Xv, yv))))
        sched.epoch(N_TRAIN, 3)
        if IS_CHILD:
            assert sched.replays == 3 * 6 - 1
        sched.key_change()
        recs.append(("fit2", record(s, Xv, s.fit(Xt, yt, Xv, yv))))
        sched.epoch(N_TRAIN, 3)
    return recs, sched


def scenario_b(net):
    """run_epoch for epochs 0..4 with cfg.epochs = 1: every call after the first runs past the step budget"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, _ = split(N_VAL, 2)
    sched, recs = Sched(), []
    with session(net, epochs=1) as s:
        for e in range(5):
            if e:
                sched.key_change()
            s.run_epoch(Xt, yt, e)
            sched.epoch(N_TRAIN)
            recs.append((f"epoch{e}", record(s, Xv)))
    return recs, sched


def scenario_c(net):
    """three epochs on three training tensors, the last one shorter.  Every tensor lives until the session has closed and the
    longer splits come first: a stale capture reads valid memory and shows as other bytes, never as a fault"""
    X1, y1 = split(N_TRAIN, 1)
    X2, y2 = split(N_TRAIN, 11)
    X3, y3 = split(N_SHORT, 12)
    Xv, _ = split(N_VAL, 2)
    sched, recs = Sched(), []
    with session(net, epochs=3) as s:
        for e, (X, y) in enumerate(((X1, y1), (X2, y2), (X3, y3))):
            if e:
                sched.key_change()
            s.run_epoch(X, y, e)
            sched.epoch(len(X))
            recs.append((f"epoch{e}", record(s, Xv)))
    if IS_CHILD:
        assert (sched.captures, sched.drops) == (3, 2)
    del X1, y1, X2, y2, X3, y3
    return recs, sched


def scenario_d(net):
    """shuffle off (the index pointer of the key is null), two epochs; then the same net with shuffle on"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, _ = split(N_VAL, 2)
    sched, recs = Sched(), []
    for shuffle in (False, True):
        one = Sched()
        with session(net, epochs=2, shuffle=shuffle) as s:
            for e in range(2):
                s.run_epoch(Xt, yt, e)
                one.epoch(N_TRAIN)
                recs.append((f"shuffle{int(shuffle)}_epoch{e}", record(s, Xv)))
        for k in COUNT_KEYS:
            setattr(sched, k, getattr(sched, k) + getattr(one, k))
    return recs, sched


def scenario_e(net):
    """the fit loop interleaved with explicit steps (the capture stays, the device state is set again from the host's
    counters), with get_state -> set_state and with a setter (both drop the capture; the next one holds the augment launch)"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, _ = split(N_VAL, 2)
    idx = dev(epoch_permutation(SEED, 7, N_TRAIN))
    sched, recs = Sched(), []
    with session(net, epochs=8) as s:
        s.run_epoch(Xt, yt, 0)
        sched.epoch(N_TRAIN)
        recs.append(("epoch0", record(s, Xv)))
        for r0 in (0, BATCH):
            s.train_step(Xt, yt, idx, row0=r0, B=BATCH)
        sched.explicit_steps(2)
        recs.append(("explicit", record(s, Xv)))
        s.run_epoch(Xt, yt, 1)
        sched.epoch(N_TRAIN)
        recs.append(("epoch1", record(s, Xv)))
        s.set_state(s.get_state())
        sched.key_change()
        s.run_epoch(Xt, yt, 2)
        sched.epoch(N_TRAIN)
        recs.append(("epoch2", record(s, Xv)))
        s.set_augment(AugmentConfig(time_shift=3))
        sched.key_change()
        s.run_epoch(Xt, yt, 3)
        sched.epoch(N_TRAIN)
        recs.append(("epoch3", record(s, Xv)))
    return recs, sched


def scenario_f(net):
    """augmentation, mixup with label smoothing and distillation against a fixed teacher table, on from the start: their
    kernels read the step from the device state"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, yv = split(N_VAL, 2)
    teacher = dev((2.0 * np.random.RandomState(21).randn(N_TRAIN, CLASSES)).astype(np.float32))
    sched, recs = Sched(), []
    with session(net, epochs=2, augment=AUG, loss=LOSS, distill=KD) as s:
        s.set_distill(teacher_logits=teacher)
        recs.append(("fit", record(s, Xv, s.fit(Xt, yt, Xv, yv))))
        sched.epoch(N_TRAIN, 2)
    return recs, sched


def scenario_g(net):
    """profile_every = 3: the profiled steps stay eager between replays"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, yv = split(N_VAL, 2)
    sched, recs = Sched(profile_every=3), []
    with session(net, epochs=2, profile_every=3) as s:
        recs.append(("fit", record(s, Xv, s.fit(Xt, yt, Xv, yv))))
        sched.epoch(N_TRAIN, 2)
    return recs, sched


def scenario_h(option):
    """an option that forbids capture: one epoch of net A, no capture and no replay"""
    Xt, yt = split(N_TRAIN, 1)
    Xv, _ = split(N_VAL, 2)
    sched, recs = Sched(capturable=False), []
    with session("A", epochs=1, **FORBID[option]) as s:
        s.run_epoch(Xt, yt, 0)
        sched.epoch(N_TRAIN)
        recs.append(("epoch0", record(s, Xv)))
    return recs, sched


SCENARIOS = dict(a=scenario_a, b=scenario_b, c=scenario_c, d=scenario_d, e=scenario_e, f=scenario_f, g=scenario_g, h=scenario_h)
CASES = [f"{sc}-{net}" for sc in "abcdeg" for net in NETS] + ["f-A"] + [f"h-{o}" for o in FORBID]


def flatten(recs):
    return {f"{tag}/{name}": np.ascontiguousarray(a) for tag, r in recs for name, a in r.items()}


def differing(got, want):
    """names whose dtype, shape or bytes differ"""
    bad = sorted(set(got) ^ set(want))
    for k in sorted(set(got) & set(want)):
        g, w = got[k], want[k]
        if g.dtype != w.dtype or g.shape != w.shape or g.tobytes() != w.tobytes():
            bad.append(k)
    return bad


def run_case(key, out_dir, replay):
    """one scenario in THIS process -> dict(ok, msg, delta, expected, seconds).  Eager side: the records are written; replay
    side: they are compared with the written ones.  Both: the launch counters' change against the schedule's counts"""
    sc, arg = key.split("-", 1)
    before = _lib.step_launch_counts()
    t0 = time.time()
    recs, sched = SCENARIOS[sc](arg)
    torch.cuda.synchronize()
    seconds = time.time() - t0
    after = _lib.step_launch_counts()
    delta = {k: after[k] - before[k] for k in COUNT_KEYS}
    expected = sched.counts(replay)
    got = flatten(recs)
    path = os.path.join(out_dir, key + ".npz")
    problems = []
    if replay:
        with np.load(path) as z:
            want = {k: z[k] for k in z.files}
        bad = differing(got, want)
        if bad:
            problems.append(f"{len(bad)} of {len(want)} arrays differ from the eager run's bytes: {bad[:8]}")
        if sched.capturable and expected["replays"] == 0:
            problems.append("the schedule holds no replayable step: the scenario proves nothing")
    else:
        np.savez(path, **got)
    if delta != expected:
        problems.append(f"launch counts {delta}, the schedule gives {expected}")
    return dict(ok=not problems, msg="; ".join(problems), delta=delta, expected=expected, seconds=round(seconds, 3))


def population_rows():
    """(accuracy, size_mb, fpr, epochs_run) of the four candidates through the ordinary population call (the fifth column is
    wall time)"""
    Xt, yt = make_data(N_TRAIN, 1)
    Xv, yv = make_data(N_VAL, 2)
    ev = PopulationEvaluator(Xt, yt, Xv, yv, cfg("A", epochs=2))
    return np.ascontiguousarray(ev.evaluate_genes(POP, POP_SEEDS)[:, :4])


def population_expected():
    sched = Sched()
    sched.epoch(N_TRAIN, 2)
    return len(POP) * sched.replays


# ---- the child processes -------------------------------------------------------------------------------------------------------
def child_main(kind, out_dir):
    """runs under CMOOP_GRAPH=1; writes <kind>_report.json.  Any exception ends the child at once: nothing more is started on
    a device that may have faulted"""
    assert GRAPH_ON
    report, status = {}, 0
    t0 = time.time()
    try:
        if kind == "session":
            for key in CASES:
                report[key] = run_case(key, out_dir, replay=True)
        else:
            before = _lib.step_launch_counts()
            rows = population_rows()
            after = _lib.step_launch_counts()
            delta = {k: after[k] - before[k] for k in COUNT_KEYS}
            want = np.load(os.path.join(out_dir, "population.npy"))
            problems = []
            if rows.dtype != want.dtype or rows.shape != want.shape or rows.tobytes() != want.tobytes():
                problems.append(f"the results differ from the eager run's bytes: {rows.tolist()} against {want.tolist()}")
            if delta["replays"] != population_expected() or delta["captures"] < len(POP):
                problems.append(f"launch counts {delta}, the schedule gives {population_expected()} replays and at least {len(POP)} captures")
            report["population"] = dict(ok=not problems, msg="; ".join(problems), delta=delta,
                                        expected=dict(replays=population_expected(), captures=len(POP)), seconds=round(time.time() - t0, 3))
    except BaseException:
        report["__error__"] = traceback.format_exc()[-3000:]
        status = 1
    report["__seconds__"] = round(time.time() - t0, 3)
    with open(os.path.join(out_dir, kind + "_report.json"), "w") as f:
        json.dump(report, f)
    return status


if IS_CHILD:
    sys.exit(child_main(sys.argv[1], sys.argv[2]))


# ---- the parent ----------------------------------------------------------------------------------------------------------------
STOP = []           # why the module stopped: a child timed out or died on a signal
_MEMO = {}


@pytest.fixture(scope="module")
def out_dir(tmp_path_factory):
    return str(tmp_path_factory.mktemp("graph_replay"))


def eager_side(out_dir):
    """every session scenario and the population call, eagerly, in this process, once"""
    if "eager" not in _MEMO:
        _MEMO["eager"] = None       # a failure below is not run again
        res = {key: run_case(key, out_dir, replay=False) for key in CASES}
        before = _lib.step_launch_counts()
        np.save(os.path.join(out_dir, "population.npy"), population_rows())
        after = _lib.step_launch_counts()
        res["population"] = dict(ok=(after["replays"], after["captures"], after["drops"]) == (0, 0, 0) and
                                 after["eager"] - before["eager"] == len(POP) * 2 * 7, msg=f"launch counts {before} -> {after}")
        _MEMO["eager"] = res
    if _MEMO["eager"] is None:
        pytest.skip("the eager side failed")
    return _MEMO["eager"]


def child(kind, out_dir, timeout):
    """the report of the one child of this kind (started on first use)"""
    if STOP:
        pytest.skip(f"stopped: {STOP[0]}")
    if kind in _MEMO:
        return _MEMO[kind]
    eager_side(out_dir)
    env = dict(os.environ, CMOOP_GRAPH="1")
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [os.path.abspath(__file__), kind, out_dir]
    t0 = time.time()
    try:
        r = subprocess.run(cmd, capture_output=True, text=True, env=env, timeout=timeout, cwd=ROOT)
    except subprocess.TimeoutExpired:
        STOP.append(f"the {kind} child did not end within {timeout} s")
        raise
    wall = time.time() - t0
    if r.returncode < 0:
        STOP.append(f"the {kind} child died on signal {-r.returncode}")
        pytest.fail(STOP[0] + "\n" + r.stdout[-2000:] + r.stderr[-2000:])
    path = os.path.join(out_dir, kind + "_report.json")
    report = json.load(open(path)) if os.path.exists(path) else {"__error__": f"no report; exit status {r.returncode}\n" + r.stderr[-3000:]}
    print(f"   {kind} child: {wall:.1f} s wall, {report.get('__seconds__')} s in its scenarios, exit status {r.returncode}")
    _MEMO[kind] = report
    if "__error__" in report:       # an exception in the child, a device error perhaps: nothing more is started
        STOP.append(f"the {kind} child ended on an exception")
        pytest.fail(STOP[0] + ":\n" + report["__error__"])
    return report


def test_eager_side_never_captures_and_counts_every_step(out_dir):
    """in a process without CMOOP_GRAPH=1 replays, captures and drops stay 0 through every scenario, and the eager count is the
    number of fit-loop steps of each scenario's schedule"""
    res = eager_side(out_dir)
    for key, r in res.items():
        print(f"   {key:12s} {r.get('delta', '')} {r.get('seconds', '')}")
    bad = {k: r["msg"] for k, r in res.items() if not r["ok"]}
    assert not bad, bad
    c = _lib.step_launch_counts()
    assert (c["replays"], c["captures"], c["drops"]) == (0, 0, 0), c


@pytest.mark.parametrize("key", CASES)
def test_replay_equals_eager_in_bytes_and_the_counters_follow_the_schedule(key, out_dir):
    """state, gradients, train metrics, the fit's dict with both histories and the validation logits of every stage of the
    scenario, byte for byte; replays, captures and drops as the schedule gives them (h-*: none)"""
    report = child("session", out_dir, SESSION_CHILD_TIMEOUT)
    assert key in report, "the child stopped before this scenario:\n" + report.get("__error__", "")
    r = report[key]
    print(f"   {key:12s} {r['delta']} {r['seconds']} s")
    assert r["ok"], r["msg"]
    if not key.startswith("h-"):
        assert r["delta"]["replays"] > 0 and r["delta"]["captures"] > 0


def test_population_call_replays_and_equals_the_eager_run(out_dir):
    """PopulationEvaluator, 4 genes on 2 slots, 2 epochs: the same rows, 4 x 11 replays, at least 4 captures"""
    report = child("population", out_dir, POPULATION_CHILD_TIMEOUT)
    assert "population" in report, report.get("__error__", "")
    r = report["population"]
    print(f"   population   {r['delta']} {r['seconds']} s")
    assert r["ok"], r["msg"]
