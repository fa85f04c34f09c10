"""GPU: the soft-target training loss (mixup, label smoothing, class weights).  Bit equality everywhere a numpy twin
exists -- the blend and targets kernels against loss.mixup_reference / soft_targets_reference, train steps / epochs
against a second net stepped with train_step_targets on the twins' rows and targets, the one-hot identity against
cmoop_softmax_ce, the off path against nets that never had a loss -- and, for the cross-entropy itself, the float64
reference under the yardstick tests/test_gpu_elem_kernels.py applies to the sparse kernel (8 x the float32 autograd
restatement's own error).  Run with -s to see the per-case figures."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

import _elem_reference as R
from _elem_reference import U
from cmoop_audio_processing_amd import AugmentConfig, EvalConfig, LossConfig, PopulationEvaluator, _lib, genes as G
from cmoop_audio_processing_amd import augment as A
from cmoop_audio_processing_amd import loss as Ls
from cmoop_audio_processing_amd.session import NetSession, epoch_permutation
from test_gpu_augment import STEP_AUG, STEP_CASES, assert_same_step
from test_gpu_net import make_data, make_split
from test_loss_cpu import MIX_PAIRS, SEED, STEPS, case_coverage, mix_case_labels

pytestmark = pytest.mark.gpu

P = _lib.ptr
SHAPES = [(1, 21, 12), (37, 21, 12), (64, 21, 13), (5, 7, 3), (5, 101, 40)]      # (64, 21, 13): F % 4 != 0, the scalar kernel
ROW0_PLAIN, ROW0_PERM, SPARE_ROWS = 3, 2, 8
CW10 = tuple(0.5 + 0.25 * j for j in range(10))
STEP_LOSS = LossConfig(mixup_alpha=0.2, mixup_p=0.5, label_smoothing=0.1, class_weight=CW10)


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ok(rc):
    torch.cuda.synchronize()
    _lib.check(rc)


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def kernel_data(B, T, F):
    """(rows with a -0.0 planted at the head of every row, permutation) -- read-only."""
    X, _ = make_data(B + SPARE_ROWS, T, F, 10, 100 + B)
    X[:, 0, 0] = -0.0
    perm = np.random.RandomState(B).permutation(B + SPARE_ROWS).astype(np.int32)
    X.setflags(write=False)
    return X, perm


# ---- 1. the blend kernel against the numpy twin ----------------------------------------------------------------------------
@pytest.mark.parametrize("pair", MIX_PAIRS)
@pytest.mark.parametrize("shape", SHAPES)
def test_blend_kernel_equals_the_numpy_twin(shape, pair):
    case_coverage()
    B, T, F = shape
    cfg = LossConfig(mixup_alpha=pair[1], mixup_p=pair[0])
    X, perm = kernel_data(B, T, F)
    Xd, permd = dev(X), dev(perm)
    for idx, idxd, row0 in ((None, None, ROW0_PLAIN), (perm, permd, ROW0_PERM)):
        rows = X[row0:row0 + B] if idx is None else X[idx[row0:row0 + B]]
        for step in STEPS:
            want = Ls.mixup_reference(rows, cfg, SEED, step)
            got = Ls.mixup_batch(Xd, cfg, SEED, step, idx=idxd, row0=row0, B=B)
            assert tuple(got.shape) == (B, T, F) and got.dtype == torch.float32
            got = got.cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (shape, pair, idx is not None, step, int((bits(got) != bits(want)).sum()))
            _, q, _ = Ls.mixup_draws(cfg, SEED, step, B)
            plain = q == np.arange(B)
            assert (bits(got[plain, 0, 0]) == 0x80000000).all(), "an un-mixed row keeps the -0.0 planted in it"


def test_blend_kernel_with_mixup_off_is_a_plain_gather():
    B, T, F = 37, 21, 12
    X, perm = kernel_data(B, T, F)
    for cfg in (LossConfig(label_smoothing=0.1), LossConfig(mixup_alpha=0.4, mixup_p=0.0)):
        got = Ls.mixup_batch(dev(X), cfg, SEED, 7, idx=dev(perm), row0=ROW0_PERM, B=B).cpu().numpy()
        assert np.array_equal(bits(got), bits(X[perm[ROW0_PERM:ROW0_PERM + B]]))


def test_blend_kernel_on_a_view_that_is_not_16_byte_aligned():
    """F % 4 == 0 but the source starts 4 bytes into an allocation: the launcher takes the element-wise kernel."""
    B, T, F = 37, 21, 12
    cfg = LossConfig(mixup_alpha=0.4, mixup_p=0.5)
    X, _ = kernel_data(B, T, F)
    flat = torch.zeros(X.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = dev(X).reshape(-1)
    Xd = flat[1:].view(X.shape)
    assert Xd.data_ptr() % 16 == 4 and Xd.is_contiguous()
    got = Ls.mixup_batch(Xd, cfg, SEED, 7, row0=1, B=B).cpu().numpy()
    want = Ls.mixup_reference(X[1:1 + B], cfg, SEED, 7)
    assert not np.array_equal(want, X[1:1 + B])
    assert np.array_equal(bits(got), bits(want))


# ---- 2. the targets kernel against the numpy twin --------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [2, 10, 11, 35])
def test_targets_kernel_equals_the_numpy_twin(Cn):
    case_coverage()
    cw = tuple(0.25 + 0.5 * j for j in range(Cn))
    modes = 0
    for B in (1, 5, 37, 64):
        n = B + SPARE_ROWS
        rs = np.random.RandomState(B)
        perm = rs.permutation(n).astype(np.int32)
        labels = rs.randint(0, Cn, n).astype(np.int32)
        if Cn == 10:
            labels[ROW0_PLAIN:ROW0_PLAIN + B] = mix_case_labels(B)               # the labels the coverage check counted
        labd, permd = dev(labels), dev(perm)
        k = 0
        for step in STEPS:
            for p, alpha in MIX_PAIRS:
                for eps in (0.0, 0.1):
                    for weights in (None, cw):
                        cfg = LossConfig(mixup_alpha=alpha, mixup_p=p, label_smoothing=eps, class_weight=weights)
                        k += 1
                        through_idx = (k + (weights is None) + (eps == 0.0)) % 2 == 0
                        modes |= 1 << int(through_idx)
                        if through_idx:
                            y, got = labels[perm[ROW0_PERM:ROW0_PERM + B]], Ls.soft_targets(labd, cfg, Cn, SEED, step, idx=permd, row0=ROW0_PERM, B=B)
                        else:
                            y, got = labels[ROW0_PLAIN:ROW0_PLAIN + B], Ls.soft_targets(labd, cfg, Cn, SEED, step, row0=ROW0_PLAIN, B=B)
                        t, w, primary = (g.cpu().numpy() for g in got)
                        wt, ww, wp = Ls.soft_targets_reference(y, cfg, Cn, SEED, step)
                        what = (B, step, p, alpha, eps, weights is not None, through_idx)
                        assert np.array_equal(bits(t), bits(wt)), (what, "t", int((bits(t) != bits(wt)).sum()))
                        assert np.array_equal(bits(w), bits(ww)), (what, "w")
                        assert np.array_equal(primary, wp), (what, "primary")
    assert modes == 3


# ---- 3. / 4. cross-entropy against dense targets ---------------------------------------------------------------------------
def _acc(loss, correct):
    return torch.from_numpy(np.array([np.float64(loss).view(np.int64), correct], np.int64)).cuda()


def _read_acc(acc):
    a = acc.cpu().numpy()
    return float(a[:1].view(np.float64)[0]), int(a[1])


def soft_ce_autograd32(z, t, w):
    """The float32 restatement through autograd, as the oracle forms the sparse loss: softmax -> log(clamp) -> logsumexp."""
    zt = torch.from_numpy(np.asarray(z, np.float32)).requires_grad_(True)
    tt, wt = torch.from_numpy(np.asarray(t, np.float32)), torch.from_numpy(np.asarray(w, np.float32))
    p = torch.softmax(zt, dim=1)
    logp = torch.log(torch.clamp(p, R.CLIP_LO, R.CLIP_HI))
    term = tt * (logp - torch.logsumexp(logp, dim=1, keepdim=True))
    lps = -torch.where(tt > 0, term, torch.zeros_like(term)).sum(dim=1)
    (wt * lps).mean().backward()
    return lps.detach().numpy(), zt.grad.numpy()


def gate8(name, gpu, ref32, ref64):
    """max|gpu - ref64| <= max(8 max|ref32 - ref64|, 4 u max|ref64|), the gate of tests/test_gpu_elem_kernels.py."""
    ref64 = np.asarray(ref64, np.float64)
    e_gpu = float(np.abs(np.asarray(gpu, np.float64) - ref64).max())
    e_ref = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    gate = max(8.0 * e_ref, 4.0 * U * float(np.abs(ref64).max()))
    print(f"    {name}: gpu err {e_gpu:.3e}  float32-reference err {e_ref:.3e}  gate {gate:.3e}")
    return e_gpu <= gate, f"{name}: {e_gpu:.3e} > {gate:.3e}"


@pytest.mark.parametrize("Cn", [2, 10, 11, 35])
@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
def test_soft_cross_entropy_against_float64(family, Cn):
    """Loss sum and dZ on mixed, smoothed and weighted target rows from the twin, B in 1, 5, 255, 256, 257, 600."""
    fails = []
    cfg = LossConfig(mixup_alpha=0.4, mixup_p=0.5, label_smoothing=0.1, class_weight=tuple(0.25 + 0.5 * j for j in range(Cn)))
    for fam, B, C_, seed in R.softmax_cases():
        if fam != family or C_ != Cn:
            continue
        z, y = R.make_logits(fam, B, Cn, seed)
        good, msg = R.logits_conditions(z, y, fam)
        assert good, msg
        t, w, primary = Ls.soft_targets_reference(y, cfg, Cn, SEED, 7)
        _, l64, dz64 = Ls.softmax_ce_soft_ref(z, t, w)
        l32, dz32 = soft_ce_autograd32(z, t, w)
        pred_ref = z.argmax(axis=1)
        correct = int((pred_ref == primary).sum())
        zd, td, wd, pd, acc = dev(z), dev(t), dev(w), dev(primary), _acc(0.0, 7)
        dz, preds = nan(B, Cn), torch.full((B,), -1, device="cuda", dtype=torch.int32)
        ok(_lib.lib().cmoop_softmax_ce_soft(P(zd), P(td), P(wd), P(pd), B, Cn, P(dz), P(acc), P(preds)))
        loss1, c1 = _read_acc(acc)
        print(f"\n  softmax_ce_soft {fam} B={B} C={Cn}: loss sum {loss1:.6e} correct {c1 - 7}/{B}")
        assert c1 - 7 == correct and np.array_equal(preds.cpu().numpy(), pred_ref), "preds / correct are exact"
        w64 = w.astype(np.float64)
        e_gpu, e_ref = abs(loss1 - (w64 * l64).sum()), float(np.abs(w64 * l32.astype(np.float64) - w64 * l64).sum())
        gate = max(8 * e_ref, 4 * U * float(np.abs(w64 * l64).sum()))
        print(f"    loss sum: gpu err {e_gpu:.3e}  float32-reference err {e_ref:.3e}  gate {gate:.3e}")
        if not e_gpu <= gate:
            fails.append(f"{fam} B={B}: loss {e_gpu:.3e} > {gate:.3e}")
        res = gate8("dZ", dz.cpu().numpy(), dz32, dz64)
        if not res[0]:
            fails.append(f"{fam} B={B}: {res[1]}")
        # dz = NULL, preds = NULL: acc still adds up
        ok(_lib.lib().cmoop_softmax_ce_soft(P(zd), P(td), P(wd), P(pd), B, Cn, None, P(acc), None))
        assert _read_acc(acc) == (loss1 + loss1, 7 + 2 * correct)
    assert not fails, fails


@pytest.mark.parametrize("Cn", [2, 10, 11, 35])
@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
def test_one_hot_targets_give_the_sparse_kernels_bits(family, Cn):
    for fam, B, C_, seed in R.softmax_cases():
        if fam != family or C_ != Cn:
            continue
        z, y = R.make_logits(fam, B, Cn, seed)
        zd, yd, td = dev(z), dev(y), dev(np.eye(Cn, dtype=np.float32)[y])
        out = []
        for soft in (False, True):
            acc, dz, preds = _acc(0.0, 0), nan(B, Cn), torch.full((B,), -1, device="cuda", dtype=torch.int32)
            if soft:
                ok(_lib.lib().cmoop_softmax_ce_soft(P(zd), P(td), None, None, B, Cn, P(dz), P(acc), P(preds)))
            else:
                ok(_lib.lib().cmoop_softmax_ce(P(zd), P(yd), None, 0, 0, B, Cn, P(dz), P(acc), P(preds)))
            out.append((acc.cpu().numpy(), dz.cpu().numpy(), preds.cpu().numpy()))
        (a0, d0, p0), (a1, d1, p1) = out
        assert np.array_equal(a0, a1), (fam, B, "loss sum / correct", a0, a1)                # int64 views: the double's bits
        assert np.array_equal(bits(d0), bits(d1)), (fam, B, "dz", int((bits(d0) != bits(d1)).sum()))
        assert np.array_equal(p0, p1)


# ---- 5. train steps: loss on == train_step_targets on the twins' rows and targets -------------------------------------------
def twin_batch(X_rows, y_rows, loss, augment, step):
    """(rows, t, w, primary) a step of a net with (loss, augment) trains on at `step`, from the numpy twins."""
    if augment is not None:
        X_rows = A.augment_reference(X_rows, augment, SEED, step)
    Xm = Ls.mixup_reference(X_rows, loss, SEED, step)
    return (Xm,) + Ls.soft_targets_reference(y_rows, loss, 10, SEED, step)


@pytest.mark.parametrize("with_augment", [False, True])
@pytest.mark.parametrize("gene,variant,T,F,batch,B,steps", STEP_CASES)
def test_train_steps_equal_steps_on_the_twins_targets(gene, variant, T, F, batch, B, steps, with_augment):
    n = 80
    X, y = make_data(n, T, F, 10, 7)
    perm = np.random.RandomState(8).permutation(n).astype(np.int32)
    Xd, yd, permd = dev(X), dev(y), dev(perm)
    cfg = EvalConfig(variant=variant, classes=10, batch=batch, eval_batch=64)
    aug = STEP_AUG if with_augment else None
    with NetSession(gene, dataclasses.replace(cfg, loss=STEP_LOSS, augment=aug), T, F, SEED) as net, NetSession(gene, cfg, T, F, SEED) as ref:
        assert net.loss == STEP_LOSS and ref.loss is None and ref.loss_buffers() == dict(mix=0, t=0, w=0, primary=0)
        assert net.loss_buffers() == dict(mix=batch * T * F, t=batch * 10, w=batch, primary=batch)
        mixed_rows = 0
        for s in range(steps):
            row0 = 5 + s * B if steps > 1 else 0
            step = net.get_state()["steps"]
            assert step == s
            rows = perm[row0:row0 + B]
            Xm, t, w, primary = twin_batch(X[rows], y[rows], STEP_LOSS, aug, step)
            mixed_rows += int((Ls.mixup_draws(STEP_LOSS, SEED, step, B)[1] != np.arange(B)).sum())
            net.train_step(Xd, yd, permd, row0=row0, B=B)
            ref.train_step_targets(dev(Xm), dev(t), dev(w), dev(primary))
            assert_same_step(net, ref, (gene, with_augment, s))
        assert mixed_rows > 0
        sa, sr = net.get_state(), ref.get_state()
        assert (sa["iterations"], sa["steps"]) == (sr["iterations"], sr["steps"]) == (steps, steps)


# ---- 6. run_epoch, fit and the population path -----------------------------------------------------------------------------
def test_run_epoch_equals_explicit_steps_on_the_twins_targets():
    gene, T, F, n, batch = (16, 3, 1, 1, 2, 1), 21, 12, 80, 32
    X, y = make_data(n, T, F, 10, 9)
    Xd, yd = dev(X), dev(y)
    cfg = EvalConfig(variant="A", classes=10, batch=batch, eval_batch=64, epochs=2, shuffle=True)
    for aug in (None, STEP_AUG):
        with NetSession(gene, dataclasses.replace(cfg, loss=STEP_LOSS, augment=aug), T, F, SEED) as net, NetSession(gene, cfg, T, F, SEED) as ref:
            for epoch in range(2):
                net.run_epoch(Xd, yd, epoch)
                perm = epoch_permutation(SEED, epoch, n)
                for s in range(0, n, batch):
                    rows = perm[s:s + batch]                                       # 32, 32, 16: the last batch draws from its own size
                    Xm, t, w, primary = twin_batch(X[rows], y[rows], STEP_LOSS, aug, ref.get_state()["steps"])
                    ref.train_step_targets(dev(Xm), dev(t), dev(w), dev(primary))
                sa, sr = net.get_state(), ref.get_state()
                assert (sa["iterations"], sa["steps"]) == (sr["iterations"], sr["steps"]) == (3 * (epoch + 1), 3 * (epoch + 1))
                for k in ("params", "m", "v"):
                    assert np.array_equal(bits(sa[k]), bits(sr[k])), (aug is not None, epoch, k, int((bits(sa[k]) != bits(sr[k])).sum()))
                assert net.train_metrics(reset=False) == ref.train_metrics(reset=False)


def test_population_path_matches_session_fit_and_train_model_sees_the_loss():
    T, F = 21, 12
    Xtr, ytr, Xva, yva = make_split(96, 48, T, F, 10, 31)
    genes = [(16, 3, 1, 1, 2, 1), (16, 5, 1, 2, 3, 1)]
    pop = [G.gene_to_hparams(g) for g in genes]
    loss = LossConfig.balanced(ytr, 10, mixup_alpha=0.2, label_smoothing=0.1)
    aug = AugmentConfig(time_shift=4, time_masks=2, time_mask_max=5, freq_masks=2, freq_mask_max=3, noise_std=0.1)
    for augment in (None, aug):
        base = EvalConfig.preset("sa_nsga_penalty", classes=10, epochs=2, early_stop=False, batch=32, eval_batch=64, seed=5, loss=loss,
                                 augment=augment)
        results = {}
        for slots in (1, 2):
            ev = PopulationEvaluator(Xtr, ytr, Xva, yva, dataclasses.replace(base, n_slots=slots))
            res = ev.compute_objectives_and_constraints(pop)
            results[slots] = ([r["objs"] for r in res], list(ev.last_epochs_run), list(ev.last_seeds))
        assert results[1] == results[2]
        objs, epochs_run, seeds = results[2]
        assert epochs_run == [2, 2]
        Xd, yd, Xv, yv = ev.X_train, ev.y_train, ev.X_val, ev.y_val
        for g, o, sd in zip(genes, objs, seeds):
            with NetSession(g, base, T, F, sd) as net:
                r = net.fit(Xd, yd, Xv, yv)
            assert (r["acc"], r["fpr"], r["epochs_run"]) == (-o[0], o[2], 2), (g, r, o)
        on = ev.train_model(genes[0], seeds[0])
        assert (on.objectives["acc"], on.objectives["fpr"]) == (-objs[0][0], objs[0][2])
    off = PopulationEvaluator(Xtr, ytr, Xva, yva, dataclasses.replace(base, loss=None)).train_model(genes[0], seeds[0])
    assert on.params.shape == off.params.shape and not np.array_equal(on.params, off.params)


# ---- 7. off means off ------------------------------------------------------------------------------------------------------
def test_off_means_off():
    gene, T, F = (16, 5, 1, 2, 2, 1), 21, 12
    Xtr, ytr, Xva, yva = make_split(80, 40, T, F, 10, 13)
    Xd, yd, Xv, yv = dev(Xtr), dev(ytr), dev(Xva), dev(yva)
    permd = dev(np.random.RandomState(14).permutation(80).astype(np.int32))
    cfg = EvalConfig(variant="B", classes=10, batch=24, eval_batch=64, epochs=2, early_stop=False)
    disabled = LossConfig(mixup_alpha=0.4, mixup_p=0.0)
    assert not disabled.enabled
    with NetSession(gene, cfg, T, F, SEED) as never, NetSession(gene, cfg, T, F, SEED) as none, \
            NetSession(gene, dataclasses.replace(cfg, loss=disabled), T, F, SEED) as off, \
            NetSession(gene, dataclasses.replace(cfg, loss=STEP_LOSS), T, F, SEED) as was_on:
        none.set_loss(None)
        was_on.train_step(Xd, yd, permd, row0=0, B=24)            # really on once, then cleared
        never.train_step(Xd, yd, permd, row0=0, B=24)
        assert not np.array_equal(was_on.get_params(), never.get_params())
        was_on.set_loss(None)
        state = never.get_state()
        for net in (none, off, was_on):
            net.set_state(state)
            net.train_metrics(reset=True)
        never.train_metrics(reset=True)
        others = (("loss=None", none), ("disabled config", off), ("set and cleared", was_on))
        for s in range(3):
            never.train_step(Xd, yd, permd, row0=3 + 24 * s, B=24)
            for name, net in others:
                net.train_step(Xd, yd, permd, row0=3 + 24 * s, B=24)
                assert_same_step(never, net, (name, s))
        want = never.fit(Xd, yd, Xv, yv)
        sa = never.get_state()
        for name, net in others:
            got = net.fit(Xd, yd, Xv, yv)
            assert (got["acc"], got["fpr"], got["val_loss"], got["epochs_run"]) == (want["acc"], want["fpr"], want["val_loss"], want["epochs_run"]), name
            assert np.array_equal(got["val_loss_history"], want["val_loss_history"]), name
            sb = net.get_state()
            for k in ("params", "m", "v"):
                assert np.array_equal(bits(sa[k]), bits(sb[k])), (name, k)
        assert none.loss_buffers() == off.loss_buffers() == dict(mix=0, t=0, w=0, primary=0)


def test_inference_is_untouched():
    gene, T, F = (16, 3, 1, 1, 2, 1), 21, 12
    X, y = make_data(80, T, F, 10, 11)
    Xd, yd = dev(X), dev(y)
    cfg = EvalConfig(variant="A", classes=10, batch=32, eval_batch=32)
    with NetSession(gene, dataclasses.replace(cfg, loss=STEP_LOSS), T, F, SEED) as net, NetSession(gene, cfg, T, F, SEED) as ref:
        for s in range(2):
            net.train_step(Xd, yd, None, row0=32 * s, B=32)
        ref.set_state(net.get_state())
        la, aa, pa = net.evaluate(Xd, yd)
        lr, ar, pr = ref.evaluate(Xd, yd)
        assert (la, aa) == (lr, ar) and torch.equal(pa, pr)
        assert torch.equal(net.predict_proba(Xd), ref.predict_proba(Xd))


# ---- 8. smoothing alone: no blend launch, no mix buffer --------------------------------------------------------------------
@pytest.mark.parametrize("with_augment", [False, True])
def test_smoothing_alone_reads_todays_input_and_allocates_no_mix_buffer(with_augment):
    gene, variant, T, F, batch, B, steps = STEP_CASES[0]
    n = 80
    X, y = make_data(n, T, F, 10, 7)
    perm = np.random.RandomState(8).permutation(n).astype(np.int32)
    Xd, yd, permd = dev(X), dev(y), dev(perm)
    cfg = EvalConfig(variant=variant, classes=10, batch=batch, eval_batch=64)
    aug = STEP_AUG if with_augment else None
    for loss in (LossConfig(label_smoothing=0.1), LossConfig(class_weight=CW10), LossConfig(label_smoothing=0.1, mixup_alpha=0.4, mixup_p=0.0)):
        with NetSession(gene, dataclasses.replace(cfg, loss=loss, augment=aug), T, F, SEED) as net, NetSession(gene, cfg, T, F, SEED) as ref:
            assert net.loss_buffers() == dict(mix=0, t=batch * 10, w=batch, primary=batch)
            for s in range(steps):
                row0 = 5 + s * B
                rows = perm[row0:row0 + B]
                Xm, t, w, primary = twin_batch(X[rows], y[rows], loss, aug, s)
                if aug is None:
                    assert np.array_equal(bits(Xm), bits(X[rows]))
                net.train_step(Xd, yd, permd, row0=row0, B=B)
                ref.train_step_targets(dev(Xm), dev(t), dev(w), dev(primary))
                assert_same_step(net, ref, (loss, with_augment, s))
            assert net.loss_buffers()["mix"] == 0
            net.set_loss(STEP_LOSS)                                   # mixup turned on later: the buffer appears on first use
            assert net.loss_buffers()["mix"] == batch * T * F


def test_train_step_targets_with_default_weights_and_primary():
    """w = None is weight 1, primary = None is the arg max of the target row: one-hot targets then train as train_step does."""
    gene, variant, T, F, batch, B, _ = STEP_CASES[0]
    X, y = make_data(80, T, F, 10, 7)
    cfg = EvalConfig(variant=variant, classes=10, batch=batch, eval_batch=64)
    with NetSession(gene, cfg, T, F, SEED) as a, NetSession(gene, cfg, T, F, SEED) as b:
        for s in range(2):
            rows = np.arange(s * B, (s + 1) * B)
            a.train_step(dev(X), dev(y), None, row0=s * B, B=B)
            b.train_step_targets(dev(X[rows]), dev(np.eye(10, dtype=np.float32)[y[rows]]))
            assert_same_step(a, b, s)
