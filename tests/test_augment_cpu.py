"""CPU: train-time augmentation -- the ABI additions, the host draws against their numpy twin, the domain check and the
properties of the numpy restatement (augment.py).  No GPU."""
import ctypes as C
import dataclasses
import re

import numpy as np
import pytest

from cmoop_audio_processing_amd import AugmentConfig, EvalConfig, _lib
from cmoop_audio_processing_amd import augment as A

NEW_SYMBOLS = ["cmoop_augment_default", "cmoop_augment_check", "cmoop_augment_draws", "cmoop_augment_batch",
               "cmoop_net_set_augment", "cmoop_eval_population_aug"]


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
    assert L.cmoop_abi_version() == 3
    assert re.search(r"#define\s+CMOOP_ABI_VERSION\s+3\b", open(_lib.HEADER).read())


def test_struct_sizes():
    assert C.sizeof(_lib.Augment) == 48
    assert _lib.Augment.p.offset == 24 and _lib.Augment.fill.offset == 40
    # cmoop_config: 14 int32 + 7 doubles, unchanged
    assert C.sizeof(_lib.Config) == 14 * 4 + 7 * 8 == 112
    # cmoop_augment_default writes exactly the struct and gives the do-nothing config
    buf = (C.c_uint8 * 64)(*([0xAB] * 64))
    _lib.check(_lib.lib().cmoop_augment_default(C.cast(buf, C.c_void_p)))
    assert bytes(buf[48:]) == b"\xab" * 16
    assert A.default_augment_config() == AugmentConfig()
    assert not AugmentConfig().enabled


DRAW_CONFIGS = [
    AugmentConfig(p=0.5, time_shift=3, time_masks=4, time_mask_max=4, freq_masks=4, freq_mask_max=3),
    AugmentConfig(p=1.0, time_shift=6, time_masks=2, time_mask_max=7, freq_masks=1, freq_mask_max=3, noise_std=0.1),
    AugmentConfig(p=0.25, time_masks=1, time_mask_max=1),
]


@pytest.mark.parametrize("TF", [(21, 12), (101, 40), (7, 3)])
def test_host_draws_equal_the_numpy_twin(TF):
    T, F = TF
    L = _lib.lib()
    for cfg in DRAW_CONFIGS:
        st = cfg._struct()
        for seed in (0, 1234, 2 ** 32 - 1):
            for step in (0, 1, 7, 123456, 2 ** 31 - 1):
                want = A.augment_draws(cfg, seed, step, 64, T, F)
                assert want.shape == (64, 18) and want.dtype == np.int32
                got = np.zeros((64, 18), np.int32)
                for b in range(64):
                    out = (C.c_int32 * 18)()
                    _lib.check(L.cmoop_augment_draws(C.byref(st), seed, step, b, T, F, out))
                    got[b] = out
                assert np.array_equal(got, want), (cfg, seed, step)


REJECTED = [
    (dict(time_shift=21), "time_shift"), (dict(time_shift=-1), "time_shift"),
    (dict(time_masks=1, time_mask_max=22), "time_mask_max"),
    (dict(freq_masks=1, freq_mask_max=13), "freq_mask_max"),
    (dict(time_masks=5), "time_masks"), (dict(freq_masks=5), "freq_masks"),
    (dict(p=-0.01), r"\bp\b"), (dict(p=1.01), r"\bp\b"), (dict(p=float("nan")), r"\bp\b"),
    (dict(noise_std=-1e-3), "noise_std"), (dict(noise_std=float("inf")), "noise_std"), (dict(noise_std=float("nan")), "noise_std"),
    (dict(fill=float("inf")), "fill"),
]


@pytest.mark.parametrize("fields,names", REJECTED)
def test_check_rejects_and_names_the_field(fields, names):
    cfg = AugmentConfig(**fields)
    st = cfg._struct()
    L = _lib.lib()
    assert L.cmoop_augment_check(C.byref(st), 21, 12) != 0
    assert re.search(names, L.cmoop_last_error().decode())
    with pytest.raises(ValueError, match=names):
        cfg.check(21, 12)
    with pytest.raises(ValueError, match=names):          # the numpy twin restates the same domain
        A.augment_draws(cfg, 0, 0, 1, 21, 12)
    out = (C.c_int32 * 18)()
    assert L.cmoop_augment_draws(C.byref(st), 0, 0, 0, 21, 12, out) != 0


def test_check_accepts_the_edges_of_the_domain():
    AugmentConfig(p=0.0, time_shift=20, time_masks=4, time_mask_max=21, freq_masks=4, freq_mask_max=12, noise_std=0.0).check(21, 12)
    AugmentConfig.preset("kws").check(101, 40)
    with pytest.raises(ValueError, match="kws"):
        AugmentConfig.preset("nope")
    k = AugmentConfig.preset("kws")
    assert (k.time_shift, k.time_masks, k.time_mask_max, k.freq_masks, k.freq_mask_max, k.p, k.noise_std) == (10, 2, 10, 2, 5, 1.0, 0.0)
    assert AugmentConfig.preset("kws", noise_std=0.1).noise_std == 0.1


def test_enabled():
    assert not AugmentConfig().enabled
    assert not AugmentConfig(p=0.0, time_shift=3, noise_std=1.0).enabled
    assert not AugmentConfig(time_masks=3, freq_masks=2).enabled              # masks of largest width 0
    assert not AugmentConfig(time_mask_max=3, freq_mask_max=2).enabled        # widths without masks
    assert not AugmentConfig(fill=1.0).enabled
    for c in (AugmentConfig(time_shift=1), AugmentConfig(time_masks=1, time_mask_max=1), AugmentConfig(freq_masks=1, freq_mask_max=1),
              AugmentConfig(noise_std=1e-3), AugmentConfig(p=1e-9, noise_std=1.0)):
        assert c.enabled, c


def rows(B, T, F, seed=0):
    return np.random.RandomState(seed).randn(B, T, F).astype(np.float32)


def test_reference_default_and_p0_are_bit_exact_copies():
    X = rows(9, 21, 12)
    X[0, 0, 0] = -0.0
    for cfg in (AugmentConfig(), AugmentConfig(p=0.0, time_shift=5, time_masks=2, time_mask_max=8, freq_masks=2, freq_mask_max=6,
                                               noise_std=0.5, fill=3.0)):
        out = A.augment_reference(X, cfg, 11, 5)
        assert out.dtype == np.float32 and out is not X
        assert np.array_equal(out.view(np.uint32), X.view(np.uint32))


def test_every_mask_lies_inside_the_patch():
    for T, F in ((21, 12), (7, 3), (101, 40)):
        cfg = AugmentConfig(p=0.7, time_shift=T - 1, time_masks=4, time_mask_max=T, freq_masks=4, freq_mask_max=F)
        for step in range(6):
            d = A.augment_draws(cfg, 99, step, 64, T, F)
            assert set(np.unique(d[:, 0])) <= {0, 1}
            assert np.abs(d[:, 1]).max() <= T - 1
            w, t0 = d[:, 2:10:2], d[:, 3:10:2]
            assert (w >= 0).all() and (w <= T).all() and (t0 >= 0).all() and (t0 + w <= T).all()
            w, f0 = d[:, 10:18:2], d[:, 11:18:2]
            assert (w >= 0).all() and (w <= F).all() and (f0 >= 0).all() and (f0 + w <= F).all()
            assert not d[d[:, 0] == 0].any()                       # a gated-off row reports zeros
        few = A.augment_draws(dataclasses.replace(cfg, p=1.0, time_masks=1, freq_masks=2), 99, 0, 64, T, F)
        assert not few[:, 4:10].any() and not few[:, 14:18].any()  # unused masks are zero


def test_shift_only_equals_the_hand_shifted_input():
    B, T, F = 40, 21, 12
    X = rows(B, T, F, 3)
    cfg = AugmentConfig(time_shift=T - 1, fill=-7.5)
    seen = set()
    for step in range(4):
        d = A.augment_draws(cfg, 5, step, B, T, F)
        out = A.augment_reference(X, cfg, 5, step)
        for b in range(B):
            s = int(d[b, 1])
            seen.add(s)
            want = np.full((T, F), np.float32(-7.5))
            if s >= 0:
                want[s:] = X[b, :T - s]
            else:
                want[:T + s] = X[b, -s:]
            assert np.array_equal(out[b], want), (step, b, s)
    assert min(seen) < 0 < max(seen)


def test_masks_fill_and_noise_skips_the_filled_positions():
    B, T, F = 16, 21, 12
    X = rows(B, T, F, 4)
    cfg = AugmentConfig(time_masks=2, time_mask_max=6, freq_masks=2, freq_mask_max=4, noise_std=0.3, fill=2.0)
    d = A.augment_draws(cfg, 8, 2, B, T, F)
    out = A.augment_reference(X, cfg, 8, 2)
    for b in range(B):
        filled = np.zeros((T, F), bool)
        for j in range(4):
            filled[d[b, 3 + 2 * j]:d[b, 3 + 2 * j] + d[b, 2 + 2 * j], :] = True
            filled[:, d[b, 11 + 2 * j]:d[b, 11 + 2 * j] + d[b, 10 + 2 * j]] = True
        assert (out[b][filled] == np.float32(2.0)).all()
        delta = out[b][~filled] - X[b][~filled]
        assert np.abs(delta).max() <= 3.47 * 0.3 and np.abs(delta).max() > 0


def test_noise_moments():
    """2e5 values: the mean's standard error is 0.0022 noise_std, the standard deviation's 0.0016 (4-term Irwin-Hall)."""
    std = 0.25
    X = np.zeros((50, 100, 40), np.float32)                        # x = 0: out is the noise itself, exactly
    n = A.augment_reference(X, AugmentConfig(noise_std=std), 1234, 17).astype(np.float64).ravel()
    assert n.size == 200000
    mean, sd = n.mean() / std, n.std() / std
    print(f"noise over {n.size} values: mean / noise_std {mean:+.5f}, std / noise_std {sd:.5f}, max |n| / noise_std {np.abs(n).max() / std:.3f}")
    assert abs(mean) <= 0.02
    assert abs(sd - 1.0) <= 0.02
    assert np.abs(n).max() <= 3.4642 * std                         # 131070 sqrt(3) / 65536


def test_eval_config_carries_the_augmentation_and_its_struct_is_unchanged():
    aug = AugmentConfig.preset("kws", noise_std=0.1)
    cfg = EvalConfig(batch=32, augment=aug)
    assert cfg.augment == aug and dataclasses.replace(cfg).augment == aug
    assert EvalConfig(**dataclasses.asdict(EvalConfig(batch=32)), ).augment is None
    assert dataclasses.replace(cfg, augment=None) == EvalConfig(batch=32)
    assert EvalConfig.preset("sa_nsga_penalty", augment=aug).augment == aug
    assert hash(cfg) == hash(EvalConfig(batch=32, augment=AugmentConfig.preset("kws", noise_std=0.1)))
    assert EvalConfig().augment is None
    # to_struct(): field for field what it is without the feature
    want = dict(variant=0, classes=10, epochs=300, batch=64, patience=5, early_stop=1, restore_best=0, acc_readout=0, fpr_variant=1,
                shuffle=1, eval_batch=256, n_slots=8, profile_every=0, gemm_mode=0, lr=1e-3, beta1=0.9, beta2=0.999, adam_eps=1e-7,
                bn_eps=1e-3, bn_momentum=0.99, dropout=0.3)
    for c in (EvalConfig(), EvalConfig(augment=aug)):
        st = c.to_struct()
        assert [n for n, _ in st._fields_] == list(want)
        assert {n: getattr(st, n) for n, _ in st._fields_} == want
    assert bytes(EvalConfig(batch=32).to_struct()) == bytes(cfg.to_struct())
    # the augmentation travels beside the struct: None when off, checked when on
    assert EvalConfig().augment_struct(21, 12) is None and EvalConfig(augment=AugmentConfig()).augment_struct(21, 12) is None
    st = cfg.augment_struct(101, 40)
    assert (st.time_shift, st.time_masks, st.time_mask_max, st.freq_masks, st.freq_mask_max, st.reserved) == (10, 2, 10, 2, 5, 0)
    assert (st.p, st.noise_std, st.fill) == (1.0, 0.1, 0.0)
    with pytest.raises(ValueError, match="time_shift"):
        cfg.augment_struct(10, 40)
