"""CPU: knowledge distillation -- the ABI additions, the domain check, the float64 statement of the loss (its gradient against
finite differences, its zero at the teacher, its T = 1 identity with the soft-target loss) and the refusal of an enabled
config without a teacher.  No GPU."""
import ctypes as C
import re

import numpy as np
import pytest

import cmoop_audio_processing_amd as pkg
from cmoop_audio_processing_amd import DistillConfig, EvalConfig, LossConfig, _lib
from cmoop_audio_processing_amd import distill as D
from cmoop_audio_processing_amd import loss as Ls

NEW_SYMBOLS = ["cmoop_distill_default", "cmoop_distill_check", "cmoop_teacher_targets", "cmoop_softmax_ce_distill",
               "cmoop_net_set_distill", "cmoop_net_train_step_distill_targets", "cmoop_net_predict_logits",
               "cmoop_eval_population_kd"]
FAKE_TABLE = 0x1000          # the check is host-only: the table pointer is compared with NULL, never read


# ---- ABI -------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in _lib.DISTILL_PROTOTYPES, name
    assert sorted(_lib.DISTILL_PROTOTYPES) == sorted(NEW_SYMBOLS)
    assert L.cmoop_abi_version() == 3
    assert re.search(r"#define\s+CMOOP_ABI_VERSION\s+3\b", open(_lib.HEADER).read())
    assert pkg.DistillConfig is DistillConfig and "DistillConfig" in pkg.__all__


def test_struct_sizes():
    S = _lib.Distill
    assert C.sizeof(S) == 32
    assert (S.alpha.offset, S.temperature.offset, S.teacher_logits_dev.offset, S.n_rows.offset) == (0, 8, 16, 24)
    assert C.sizeof(_lib.Loss) == 40                                  # unchanged
    assert C.sizeof(_lib.Augment) == 48                               # unchanged
    assert C.sizeof(_lib.Config) == 14 * 4 + 7 * 8 == 112             # unchanged
    buf = (C.c_uint8 * 48)(*([0xAB] * 48))
    _lib.check(_lib.lib().cmoop_distill_default(C.cast(buf, C.c_void_p)))
    assert bytes(buf[32:]) == b"\xab" * 16                            # writes exactly the struct
    assert D.default_distill_config() == DistillConfig() == DistillConfig(alpha=0.0, temperature=1.0)
    assert not DistillConfig().enabled and EvalConfig().distill is None


def test_preset_and_enabled():
    kws = DistillConfig.preset("kws")
    assert (kws.alpha, kws.temperature) == (0.7, 4.0) and kws.enabled
    assert DistillConfig.preset("kws", alpha=0.5).alpha == 0.5
    with pytest.raises(ValueError):
        DistillConfig.preset("nope")
    with pytest.raises(Exception):
        kws.alpha = 0.1                                               # frozen


# ---- domain ----------------------------------------------------------------------------------------------------------------
def _struct(alpha=0.5, temperature=2.0, table=FAKE_TABLE, n_rows=80):
    return _lib.Distill(alpha, temperature, table, n_rows)


REJECTED = [
    (dict(alpha=-0.1), "alpha"), (dict(alpha=1.01), "alpha"), (dict(alpha=float("nan")), "alpha"),
    (dict(temperature=0.5), "temperature"), (dict(temperature=64.5), "temperature"), (dict(temperature=float("inf")), "temperature"),
    (dict(temperature=float("nan")), "temperature"),
    (dict(n_rows=79), "n_rows"), (dict(n_rows=81), "n_rows"), (dict(n_rows=0), "n_rows"),
]


@pytest.mark.parametrize("fields,name", REJECTED)
def test_check_rejects_and_names_the_field(fields, name):
    L = _lib.lib()
    st = _struct(**fields)
    assert L.cmoop_distill_check(C.byref(st), 10, 80) != 0
    msg = L.cmoop_last_error().decode()
    assert re.search(name, msg), msg
    with pytest.raises(ValueError, match=name):
        D.check_struct(st, 10, 80)
    if "n_rows" not in fields:
        with pytest.raises(ValueError, match=name):
            DistillConfig(**fields).check(10)


def test_check_accepts_the_domain_and_disabled_configs():
    L = _lib.lib()
    for st in (_struct(), _struct(alpha=1.0, temperature=64.0), _struct(alpha=0.0), _struct(temperature=1.0)):
        assert L.cmoop_distill_check(C.byref(st), 10, 80) == 0, L.cmoop_last_error()
    # disabled: alpha 0, or no table (n_rows is then not looked at) -- both pass, neither is enabled
    assert L.cmoop_distill_check(C.byref(_struct(alpha=0.0, n_rows=80)), 10, 80) == 0
    assert L.cmoop_distill_check(C.byref(_struct(table=None, n_rows=0)), 10, 80) == 0
    assert not DistillConfig(alpha=0.0, temperature=4.0).enabled
    cfg = DistillConfig(alpha=0.5, temperature=4.0)
    assert cfg.check(10) is cfg
    st = cfg._struct(None)
    assert not st.teacher_logits_dev and st.n_rows == 0


# ---- the float64 statement -------------------------------------------------------------------------------------------------
def _case(Cn, seed, B=6):
    rs = np.random.RandomState(seed)
    z = rs.randn(B, Cn)
    y = rs.randint(0, Cn, B)
    cfg = LossConfig(mixup_alpha=0.4, mixup_p=0.5, label_smoothing=0.1, class_weight=tuple(0.5 + 0.25 * j for j in range(Cn)))
    t, w, _ = Ls.soft_targets_reference(y, cfg, Cn, 1234, 7)
    q = D.teacher_targets_ref(2.0 * rs.randn(B, Cn), 3.0)
    return z, t.astype(np.float64), w.astype(np.float64), q


@pytest.mark.parametrize("Cn", [2, 10, 35])
def test_reference_gradient_equals_finite_differences(Cn):
    z, t, w, q = _case(Cn, 10 + Cn)
    p = np.exp(z - z.max(axis=1, keepdims=True))
    p /= p.sum(axis=1, keepdims=True)
    assert p.min() > 1e-5 and p.max() < 1 - 1e-5, "no probability near the clip bounds: the loss is smooth here"
    for alpha, T in ((0.5, 1.0), (0.7, 4.0), (1.0, 2.0), (0.0, 3.0)):
        _, dz = D.softmax_ce_distill_ref(z, t, w, q, alpha, T)
        h = 1e-6
        fd = np.zeros_like(z)
        for b in range(z.shape[0]):
            for j in range(Cn):
                zp, zm = z.copy(), z.copy()
                zp[b, j] += h
                zm[b, j] -= h
                fd[b, j] = (D.softmax_ce_distill_ref(zp, t, w, q, alpha, T)[0].mean() -
                            D.softmax_ce_distill_ref(zm, t, w, q, alpha, T)[0].mean()) / (2 * h)
        err = float(np.abs(fd - dz).max())
        print(f"\n  C={Cn} alpha={alpha} T={T}: |fd - dz| {err:.3e}, max|dz| {np.abs(dz).max():.3e}")
        # central differences at h = 1e-6: truncation ~ h^2 |f'''| / 6 ~ 1e-12, rounding ~ eps |f| / h ~ 2e-16 * 10 / 1e-6 = 2e-9
        assert err <= 2e-8


@pytest.mark.parametrize("Cn", [2, 10, 35])
def test_reference_is_zero_at_the_teacher(Cn):
    z, t, w, _ = _case(Cn, 20 + Cn)
    for T in (1.0, 2.0, 4.0):
        q = D.teacher_targets_ref(z, T)
        loss, dz = D.softmax_ce_distill_ref(z, t, w, q, 1.0, T)
        # log(exp(ls)) against ls: a few eps (|ls| + 1) per class, |ls| <= 2 max|z| + log C; then w T^2 (loss), w T / B (dz)
        eps = np.finfo(np.float64).eps * w.max() * (2 * np.abs(z).max() + np.log(Cn) + 1)
        assert np.abs(loss).max() <= 16 * T * T * eps
        assert np.abs(dz).max() <= 16 * T * eps


@pytest.mark.parametrize("Cn", [2, 10, 35])
def test_reference_at_temperature_one_is_the_soft_loss_on_blended_targets(Cn):
    z, t, w, q = _case(Cn, 30 + Cn)
    for alpha in (0.0, 0.3, 1.0):
        _, dz = D.softmax_ce_distill_ref(z, t, w, q, alpha, 1.0)
        _, _, want = Ls.softmax_ce_soft_ref(z, (1.0 - alpha) * t + alpha * q, w)
        assert np.abs(dz - want).max() <= 64 * np.finfo(np.float64).eps * np.abs(w).max()


def test_teacher_targets_reference_blends_with_the_mixup_draws():
    rs = np.random.RandomState(5)
    zt = rs.randn(64, 10)
    cfg = LossConfig(mixup_alpha=0.4, mixup_p=0.5)
    u = D.teacher_targets_ref(zt, 2.0)
    q = D.teacher_targets_ref(zt, 2.0, cfg, 1234, 7)
    _, partner, lam = Ls.mixup_draws(cfg, 1234, 7, 64)
    mixed = partner != np.arange(64)
    assert mixed.any() and (~mixed).any()
    assert np.array_equal(q[~mixed], u[~mixed])
    b = int(np.nonzero(mixed)[0][0])
    assert np.allclose(q[b], float(lam[b]) * u[b] + (1.0 - float(lam[b])) * u[partner[b]], rtol=0, atol=1e-16)
    assert np.allclose(q.sum(axis=1), 1.0, rtol=0, atol=1e-14)
    assert np.array_equal(D.teacher_targets_ref(zt, 2.0, LossConfig(label_smoothing=0.1), 1234, 7), u)


# ---- an enabled config needs a teacher -------------------------------------------------------------------------------------
def test_enabled_distill_without_a_teacher_is_refused_before_any_gpu_call():
    on = EvalConfig(classes=10, distill=DistillConfig(alpha=0.5, temperature=2.0))
    with pytest.raises(ValueError, match="set_teacher"):
        D.require_teacher(on.distill, None)
    with pytest.raises(ValueError, match="set_teacher"):
        on.distill_struct(None, 80)
    D.require_teacher(None, None)
    D.require_teacher(DistillConfig(alpha=0.0, temperature=2.0), None)
    assert EvalConfig(classes=10).distill_struct(None, 80) is None
    assert EvalConfig(classes=10, distill=DistillConfig(alpha=0.0, temperature=2.0)).distill_struct(None, 80) is None
