"""GPU: train-time augmentation.  Every gate here is bit equality: the kernel against its numpy twin
(augment.augment_reference), augmented train steps / epochs against a second net that is fed the pre-augmented rows,
inference and the off path against nets that never had an augmentation, and the population path against NetSession.fit."""
import dataclasses
import functools

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import AugmentConfig, EvalConfig, PopulationEvaluator, genes as G
from cmoop_audio_processing_amd import augment as A
from cmoop_audio_processing_amd.session import NetSession, epoch_permutation
from test_gpu_net import make_data, make_split

pytestmark = pytest.mark.gpu

SEED = 1234
SHAPES = [(1, 21, 12), (37, 21, 12), (64, 21, 13), (5, 7, 3), (5, 101, 40)]      # (64, 21, 13): F % 4 != 0, the scalar kernel
STEPS = (0, 7, 123456)
ROW0_PLAIN, ROW0_PERM, SPARE_ROWS = 3, 2, 8


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def kernel_configs(T, F):
    return {
        "shift": AugmentConfig(time_shift=T - 1, fill=-3.0),
        "masks": AugmentConfig(time_masks=4, time_mask_max=T, freq_masks=4, freq_mask_max=F, fill=0.5),
        "noise": AugmentConfig(noise_std=0.25),
        "all": AugmentConfig(p=0.5, time_shift=3, time_masks=4, time_mask_max=4, freq_masks=4, freq_mask_max=min(4, F), noise_std=0.1),
        "p0": AugmentConfig(p=0.0, time_shift=3, time_masks=2, time_mask_max=4, freq_masks=2, freq_mask_max=2, noise_std=0.1, fill=9.0),
    }


CONFIG_NAMES = list(kernel_configs(21, 12))


@functools.lru_cache(maxsize=None)
def case_coverage():
    """What the kernel cases exercise, from the draws alone (no GPU): asserted before the first launch."""
    seen = dict(s_plus=False, s_minus=False, w_zero=False, t_w_max=False, f_w_max=False, t_mask_at_end=False, mixed_gate=False)
    for B, T, F in SHAPES:
        for name, cfg in kernel_configs(T, F).items():
            for step in STEPS:
                d = A.augment_draws(cfg, SEED, step, B, T, F).astype(np.int64)
                on = d[:, 0] == 1
                if cfg.time_shift:
                    seen["s_plus"] |= bool((d[on, 1] == cfg.time_shift).any())
                    seen["s_minus"] |= bool((d[on, 1] == -cfg.time_shift).any())
                if cfg.time_masks and cfg.time_mask_max:
                    w, t0 = d[on][:, 2:2 + 2 * cfg.time_masks:2], d[on][:, 3:3 + 2 * cfg.time_masks:2]
                    seen["w_zero"] |= bool((w == 0).any())
                    seen["t_w_max"] |= bool((w == cfg.time_mask_max).any())
                    seen["t_mask_at_end"] |= bool(((w > 0) & (t0 + w == T)).any())
                if cfg.freq_masks and cfg.freq_mask_max:
                    w = d[on][:, 10:10 + 2 * cfg.freq_masks:2]
                    seen["f_w_max"] |= bool((w == cfg.freq_mask_max).any())
                seen["mixed_gate"] |= bool(on.any() and (~on).any())
    assert all(seen.values()), seen
    return seen


@functools.lru_cache(maxsize=None)
def kernel_data(B, T, F):
    """(rows, permutation) -- read-only."""
    X, _ = make_data(B + SPARE_ROWS, T, F, 10, 100 + B)
    perm = np.random.RandomState(B).permutation(B + SPARE_ROWS).astype(np.int32)
    return X, perm


# ---- 1. the kernel against the numpy twin ---------------------------------------------------------------------------
@pytest.mark.parametrize("name", CONFIG_NAMES)
@pytest.mark.parametrize("shape", SHAPES)
def test_kernel_equals_the_numpy_twin(shape, name):
    case_coverage()
    B, T, F = shape
    cfg = kernel_configs(T, F)[name]
    X, perm = kernel_data(B, T, F)
    Xd, permd = dev(X), dev(perm)
    for idx, idxd, row0 in ((None, None, ROW0_PLAIN), (perm, permd, ROW0_PERM)):
        rows = X[row0:row0 + B] if idx is None else X[idx[row0:row0 + B]]
        for step in STEPS:
            want = rows if name == "p0" else A.augment_reference(rows, cfg, SEED, step)      # p = 0: a plain gather
            got = A.augment_batch(Xd, cfg, SEED, step, idx=idxd, row0=row0, B=B)
            assert tuple(got.shape) == (B, T, F) and got.dtype == torch.float32
            got = got.cpu().numpy()
            assert np.array_equal(bits(got), bits(want)), (shape, name, idx is not None, step,
                                                           int((bits(got) != bits(want)).sum()))


def test_kernel_on_a_view_that_is_not_16_byte_aligned():
    """F % 4 == 0 but the source starts 4 bytes into an allocation: the launcher takes the element-wise kernel."""
    B, T, F = 6, 21, 12
    cfg = kernel_configs(T, F)["all"]
    X, _ = kernel_data(B, T, F)
    flat = torch.zeros(X.size + 1, dtype=torch.float32, device="cuda")
    flat[1:] = dev(X).reshape(-1)
    Xd = flat[1:].view(X.shape)
    assert Xd.data_ptr() % 16 == 4 and Xd.is_contiguous()
    got = A.augment_batch(Xd, cfg, SEED, 7, row0=1, B=B).cpu().numpy()
    assert np.array_equal(bits(got), bits(A.augment_reference(X[1:1 + B], cfg, SEED, 7)))


# ---- 2. one train step: augmentation on == augmentation off on the pre-augmented rows --------------------------------
STEP_AUG = AugmentConfig(p=0.5, time_shift=3, time_masks=2, time_mask_max=4, freq_masks=2, freq_mask_max=3, noise_std=0.1)
STEP_CASES = [
    ((16, 3, 1, 1, 2, 1), "A", 21, 12, 32, 24, 3),
    ((16, 5, 0, 2, 1, 0), "B", 21, 12, 32, 24, 3),
    ((16, 3, 1, 1, 1, 1), "A", 101, 40, 64, 64, 1),
]


def assert_same_step(a, b, what):
    pa, pb = a.get_params(), b.get_params()
    assert np.array_equal(bits(pa), bits(pb)), (what, "params", int((bits(pa) != bits(pb)).sum()))
    ga, gb = a.get_grads(), b.get_grads()
    assert np.array_equal(bits(ga), bits(gb)), (what, "grads", int((bits(ga) != bits(gb)).sum()))
    assert a.train_metrics(reset=False) == b.train_metrics(reset=False), (what, "train metrics")


@pytest.mark.parametrize("gene,variant,T,F,batch,B,steps", STEP_CASES)
def test_train_steps_equal_steps_on_pre_augmented_rows(gene, variant, T, F, batch, B, steps):
    n = 80
    X, y = make_data(n, T, F, 10, 7)
    perm = np.random.RandomState(8).permutation(n).astype(np.int32)
    Xd, yd, permd = dev(X), dev(y), dev(perm)
    cfg = EvalConfig(variant=variant, classes=10, batch=batch, eval_batch=64)
    with NetSession(gene, dataclasses.replace(cfg, augment=STEP_AUG), T, F, SEED) as aug, NetSession(gene, cfg, T, F, SEED) as ref:
        assert aug.augment == STEP_AUG and ref.augment is None
        changed = False
        for s in range(steps):
            row0 = 5 + s * B if steps > 1 else 0
            step = aug.get_state()["steps"]
            assert step == s
            rows = perm[row0:row0 + B]
            Xa = A.augment_reference(X[rows], STEP_AUG, SEED, step)
            changed |= not np.array_equal(Xa, X[rows])
            aug.train_step(Xd, yd, permd, row0=row0, B=B)
            ref.train_step(dev(Xa), dev(y[rows]), None, row0=0, B=B)
            assert_same_step(aug, ref, (gene, s))
        assert changed


# ---- 3. run_epoch (device step state, partial last batch) ------------------------------------------------------------
def test_run_epoch_equals_explicit_steps_on_pre_augmented_batches():
    gene, T, F, n, batch = (16, 3, 1, 1, 2, 1), 21, 12, 80, 32
    X, y = make_data(n, T, F, 10, 9)
    Xd, yd = dev(X), dev(y)
    cfg = EvalConfig(variant="A", classes=10, batch=batch, eval_batch=64, epochs=2, shuffle=True)
    with NetSession(gene, dataclasses.replace(cfg, augment=STEP_AUG), T, F, SEED) as aug, NetSession(gene, cfg, T, F, SEED) as ref:
        for epoch in range(2):
            aug.run_epoch(Xd, yd, epoch)
            perm = epoch_permutation(SEED, epoch, n)
            for s in range(0, n, batch):
                rows = perm[s:s + batch]                                       # 32, 32, 16
                step = ref.get_state()["steps"]
                Xa = A.augment_reference(X[rows], STEP_AUG, SEED, step)
                ref.train_step(dev(Xa), dev(y[rows]), None, row0=0, B=len(rows))
            sa, sr = aug.get_state(), ref.get_state()
            assert (sa["iterations"], sa["steps"]) == (sr["iterations"], sr["steps"]) == (3 * (epoch + 1), 3 * (epoch + 1))
            for k in ("params", "m", "v"):
                assert np.array_equal(bits(sa[k]), bits(sr[k])), (epoch, k, int((bits(sa[k]) != bits(sr[k])).sum()))
            assert aug.train_metrics(reset=False) == ref.train_metrics(reset=False)


# ---- 4. inference never augments -------------------------------------------------------------------------------------
def test_inference_is_untouched():
    gene, T, F = (16, 3, 1, 1, 2, 1), 21, 12
    X, y = make_data(80, T, F, 10, 11)
    Xd, yd = dev(X), dev(y)
    cfg = EvalConfig(variant="A", classes=10, batch=32, eval_batch=32)
    with NetSession(gene, dataclasses.replace(cfg, augment=STEP_AUG), T, F, SEED) as aug, NetSession(gene, cfg, T, F, SEED) as ref:
        for s in range(2):
            aug.train_step(Xd, yd, None, row0=32 * s, B=32)
        ref.set_state(aug.get_state())
        la, aa, pa = aug.evaluate(Xd, yd)
        lr, ar, pr = ref.evaluate(Xd, yd)
        assert (la, aa) == (lr, ar) and torch.equal(pa, pr)
        qa, qr = aug.predict_proba(Xd), ref.predict_proba(Xd)
        assert torch.equal(qa, qr)
        aug.set_augment(None)
        lb, ab, pb = aug.evaluate(Xd, yd)
        assert (la, aa) == (lb, ab) and torch.equal(pa, pb) and torch.equal(qa, aug.predict_proba(Xd))


# ---- 5. off means off ------------------------------------------------------------------------------------------------
def test_off_means_off():
    gene, T, F = (16, 5, 1, 2, 2, 1), 21, 12
    X, y = make_data(80, T, F, 10, 13)
    Xd, yd = dev(X), dev(y)
    permd = dev(np.random.RandomState(14).permutation(80).astype(np.int32))
    cfg = EvalConfig(variant="B", classes=10, batch=24, eval_batch=64)
    with NetSession(gene, cfg, T, F, SEED) as never, NetSession(gene, dataclasses.replace(cfg, augment=AugmentConfig()), T, F, SEED) as default, \
            NetSession(gene, dataclasses.replace(cfg, augment=STEP_AUG), T, F, SEED) as was_on:
        was_on.train_step(Xd, yd, permd, row0=0, B=24)            # really augmented once, then switched off
        never.train_step(Xd, yd, permd, row0=0, B=24)
        assert not np.array_equal(was_on.get_params(), never.get_params())
        was_on.set_augment(None)
        state = never.get_state()
        for net in (default, was_on):
            net.set_state(state)
            net.train_metrics(reset=True)
        never.train_metrics(reset=True)
        for s in range(3):
            for net in (never, default, was_on):
                net.train_step(Xd, yd, permd, row0=3 + 24 * s, B=24)
            assert_same_step(never, default, ("default config", s))
            assert_same_step(never, was_on, ("switched off", s))
        sa, sb, sc = never.get_state(), default.get_state(), was_on.get_state()
        for k in ("params", "m", "v"):
            assert np.array_equal(bits(sa[k]), bits(sb[k])) and np.array_equal(bits(sa[k]), bits(sc[k]))


# ---- 6. the population path ------------------------------------------------------------------------------------------
def test_population_path_matches_session_fit_and_train_model_sees_the_augmentation():
    T, F = 21, 12
    Xtr, ytr, Xva, yva = make_split(96, 48, T, F, 10, 31)
    genes = [(16, 3, 1, 1, 2, 1), (32, 5, 0, 1, 1, 0), (16, 5, 1, 2, 3, 1)]
    pop = [G.gene_to_hparams(g) for g in genes]
    aug = AugmentConfig(time_shift=4, time_masks=2, time_mask_max=5, freq_masks=2, freq_mask_max=3, noise_std=0.1)
    base = EvalConfig.preset("sa_nsga_penalty", classes=10, epochs=2, early_stop=False, batch=32, eval_batch=64, seed=5, augment=aug)
    results = {}
    for slots in (1, 3):
        ev = PopulationEvaluator(Xtr, ytr, Xva, yva, dataclasses.replace(base, n_slots=slots))
        res = ev.compute_objectives_and_constraints(pop)
        results[slots] = ([r["objs"] for r in res], [r["CV"] for r in res], list(ev.last_epochs_run), list(ev.last_seeds))
    assert results[1] == results[3]
    objs, _, epochs_run, seeds = results[3]
    assert epochs_run == [2, 2, 2]
    Xd, yd, Xv, yv = ev.X_train, ev.y_train, ev.X_val, ev.y_val
    for g, o, sd in zip(genes, objs, seeds):
        with NetSession(g, base, T, F, sd) as net:
            r = net.fit(Xd, yd, Xv, yv)
        assert (r["acc"], r["fpr"], r["epochs_run"]) == (-o[0], o[2], 2), (g, r, o)
    on = ev.train_model(genes[0], seeds[0])
    assert (on.objectives["acc"], on.objectives["fpr"]) == (-objs[0][0], objs[0][2])
    off = PopulationEvaluator(Xtr, ytr, Xva, yva, dataclasses.replace(base, augment=None)).train_model(genes[0], seeds[0])
    assert on.params.shape == off.params.shape and not np.array_equal(on.params, off.params)
