"""CPU: the weight EMA's host side -- the ABI (new symbols, struct size, the all-off default), the domain check, the rates
(``cmoop_ema_rates`` against ``EmaConfig.momentum_at`` and its float32 roundings, bit for bit), the numpy statement, and the
way the option travels beside ``EvalConfig.option_structs``."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from cmoop_audio_processing_amd import EmaConfig, EvalConfig, _lib
from cmoop_audio_processing_amd import ema as E

NEW_SYMBOLS = ["cmoop_ema_default", "cmoop_ema_check", "cmoop_ema_rates", "cmoop_ema_update", "cmoop_net_set_ema", "cmoop_net_get_ema",
               "cmoop_net_set_ema_params", "cmoop_net_use_ema", "cmoop_net_finalize_ema", "cmoop_eval_population_avg"]


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_version_and_struct_size():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert name in _lib.EMA_PROTOTYPES, name
    assert L.cmoop_abi_version() == 3, "functions are added only"
    assert C.sizeof(_lib.Ema) == 16                          # api.hip static_asserts the same of cmoop_ema
    assert (_lib.Ema.momentum.offset, _lib.Ema.warmup.offset, _lib.Ema.reserved.offset) == (0, 8, 12)
    # cmoop_eval_population_avg is _opt with one more struct pointer, after optim
    assert len(_lib.EMA_PROTOTYPES["cmoop_eval_population_avg"]) == len(_lib.OPTIM_PROTOTYPES["cmoop_eval_population_opt"]) + 1


def test_default_is_all_zero_and_disabled():
    st = _lib.Ema()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    _lib.check(_lib.lib().cmoop_ema_default(C.byref(st)))
    assert bytes(st) == bytes(C.sizeof(st)), "every byte zero"
    assert E.default_ema_config() == EmaConfig() and not EmaConfig().enabled
    assert bytes(EmaConfig()._struct()) == bytes(st)
    assert EmaConfig(0.99).enabled and EmaConfig(1e-9).enabled and not EmaConfig(0.0, warmup=True).enabled
    assert E.from_struct(EmaConfig(0.999, True)._struct()) == EmaConfig(0.999, True)
    assert _lib.lib().cmoop_ema_default(None) != 0


# ---- the domain ----------------------------------------------------------------------------------------------------------------
BAD = [(dict(momentum=-0.1), "momentum"), (dict(momentum=1.0), "momentum"), (dict(momentum=1.5), "momentum"),
       (dict(momentum=math.nan), "momentum"), (dict(momentum=math.inf), "momentum"), (dict(momentum=-math.inf), "momentum"),
       (dict(momentum=0.9, warmup=2), "warmup"), (dict(momentum=0.9, warmup=-1), "warmup"),
       (dict(momentum=0.9, reserved=1), "reserved"), (dict(momentum=0.0, reserved=-7), "reserved")]


@pytest.mark.parametrize("fields,word", BAD)
def test_check_rejects_and_names_the_field(fields, word):
    st = _lib.Ema()
    for k, v in fields.items():
        setattr(st, k, v)
    L = _lib.lib()
    assert L.cmoop_ema_check(C.byref(st)) != 0
    assert word in L.cmoop_last_error().decode()
    with pytest.raises(ValueError, match=word):
        E.check_struct(st)
    # the same struct is refused by the rates call
    assert L.cmoop_ema_rates(C.byref(st), 0, None, None, None) != 0 and word in L.cmoop_last_error().decode()


def test_check_accepts_the_domain():
    L = _lib.lib()
    for cfg in (EmaConfig(), EmaConfig(0.9), EmaConfig(0.99, True), EmaConfig(math.nextafter(1.0, 0.0)), EmaConfig(5e-324)):
        assert cfg.check() is cfg
    assert L.cmoop_ema_check(None) != 0 and "NULL" in L.cmoop_last_error().decode()
    with pytest.raises(ValueError, match="momentum"):
        EmaConfig(1.0).check()


# ---- the rates -----------------------------------------------------------------------------------------------------------------
ITERS = (0, 1, 8, 9, 89, 90, 891, 10 ** 6)


@pytest.mark.parametrize("warmup", [False, True])
@pytest.mark.parametrize("m", [0.9, 0.99, 0.999])
def test_rates_equal_momentum_at_and_its_float32_roundings(m, warmup):
    cfg = EmaConfig(m, warmup)
    for i in ITERS:
        md, mf, omf = E.rates(cfg, i)
        want = cfg.momentum_at(i)
        assert want == (min(m, (1.0 + i) / (10.0 + i)) if warmup else m)
        assert md == want, (i, md, want)
        assert bits(mf) == bits(np.float32(want)), i
        assert bits(omf) == bits(np.float32(1.0 - want)), (i, "the subtraction is done in double, then rounded once")
    # outputs may be NULL, each alone
    st = cfg._struct()
    one = C.c_float()
    _lib.check(_lib.lib().cmoop_ema_rates(C.byref(st), 5, None, None, C.byref(one)))
    assert bits(np.float32(one.value)) == bits(E.rates(cfg, 5)[2])
    assert _lib.lib().cmoop_ema_rates(C.byref(st), -1, None, None, None) != 0


@pytest.mark.parametrize("m", [0.9, 0.99, 0.999])
def test_warmup_is_non_decreasing_and_reaches_m(m):
    cfg = EmaConfig(m, True)
    seq = [E.rates(cfg, i)[0] for i in range(0, 12000)]
    assert all(b >= a for a, b in zip(seq, seq[1:]))
    assert seq[0] == 0.1 and seq[-1] == m and seq[0] < m
    first = next(i for i, v in enumerate(seq) if v == m)
    assert (1.0 + first) / (10.0 + first) >= m > (1.0 + first - 1) / (10.0 + first - 1)
    # the float32 sum of the pair is 1 to a rounding: the update is a convex combination
    for i in (0, 3, 89, first):
        _, mf, omf = E.rates(cfg, i)
        assert abs(float(mf) + float(omf) - 1.0) <= 2.0 ** -24


# ---- the statement -------------------------------------------------------------------------------------------------------------
def test_statement_kinds_fixed_point_and_signed_zeros():
    rs = np.random.RandomState(3)
    n = 4096
    a, w = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    kinds = rs.randint(0, 3, n).astype(np.uint8)
    w[:4] = np.array([np.nan, np.inf, -0.0, 1e-45], np.float32)
    kinds[:4] = 2
    _, mf, omf = E.rates(EmaConfig(0.99), 0)
    out = E.ema_step_ref(a, w, mf, omf, kinds)
    frozen = kinds == 2
    assert out.dtype == np.float32 and np.array_equal(bits(out[frozen]), bits(w[frozen])), "kind 2: a copy of w's bits"
    # one operation per line, in float32
    keep = (np.float32(mf) * a).astype(np.float32)
    take = (np.float32(omf) * w).astype(np.float32)
    assert np.array_equal(bits(out[~frozen]), bits((keep + take)[~frozen]))
    assert not np.array_equal(bits(out[~frozen]), bits(w[~frozen])) and not np.array_equal(bits(out[~frozen]), bits(a[~frozen]))
    # kinds None: every element is trainable
    assert np.array_equal(bits(E.ema_step_ref(a[4:], w[4:], mf, omf)), bits((keep + take)[4:]))
    # a == w is a fixed point exactly where mf a + omf a rounds back to a -- not everywhere: (float)0.99 + (float)0.01 != 1
    same = E.ema_step_ref(a, a, mf, omf)
    back = (np.float32(mf) * a).astype(np.float32) + (np.float32(omf) * a).astype(np.float32)
    assert np.array_equal(bits(same), bits(back))
    fixed = bits(same) == bits(a)
    assert fixed.any() and not fixed.all(), "some elements move by an ulp"
    assert np.array_equal(bits(E.ema_step_ref(a, a, mf, omf, np.full(n, 2, np.uint8))), bits(a)), "frozen: always a fixed point"
    # zeros keep their sign as IEEE gives it: (-0) + (-0) = -0, (+0) + (-0) = +0, and a NaN / inf weight propagates
    z = E.ema_step_ref(np.array([-0.0, 0.0, -0.0, 0.0], np.float32), np.array([-0.0, -0.0, 0.0, 0.0], np.float32), mf, omf)
    assert np.array_equal(np.signbit(z), [True, False, False, False]) and (z == 0).all()
    p = E.ema_step_ref(np.ones(3, np.float32), np.array([np.nan, np.inf, -np.inf], np.float32), mf, omf)
    assert np.isnan(p[0]) and p[1] == np.inf and p[2] == -np.inf


# ---- EvalConfig ----------------------------------------------------------------------------------------------------------------
def test_option_structs_stays_a_four_tuple_and_ema_travels_beside_it():
    for cfg in (EvalConfig(), EvalConfig(ema=None), EvalConfig(ema=EmaConfig())):
        assert cfg.option_structs(21, 12, None, 40) == (None, None, None, None)
        assert cfg.ema_struct() is None
    on = EvalConfig(ema=EmaConfig(0.99, True))
    assert on.option_structs(21, 12, None, 40) == (None, None, None, None)
    st = on.ema_struct()
    assert isinstance(st, _lib.Ema) and (st.momentum, st.warmup, st.reserved) == (0.99, 1, 0)
    assert bytes(on.to_struct()) == bytes(EvalConfig().to_struct()), "cmoop_config is what it is without the field"
    with pytest.raises(ValueError, match="momentum"):
        EvalConfig(ema=EmaConfig(1.0)).ema_struct()
    assert dataclasses.replace(on, ema=None).ema_struct() is None
