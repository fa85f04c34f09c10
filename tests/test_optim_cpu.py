"""CPU: the optimiser options' host side -- the ABI (new symbols, ABI version, struct size, the all-off default), the domain
check, the schedule (``cmoop_optim_rates`` against ``OptimConfig.lr_at`` at every edge of every schedule), the numpy
statement against the existing Adam statement, and the tensor-kind arena."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

import _elem_reference as R
from cmoop_audio_processing_amd import EvalConfig, OptimConfig, _lib, genes as G
from cmoop_audio_processing_amd import optim as O

NEW_SYMBOLS = ["cmoop_optim_default", "cmoop_optim_check", "cmoop_optim_rates", "cmoop_param_kinds", "cmoop_grad_finish", "cmoop_adamw",
               "cmoop_net_set_optim", "cmoop_net_optim_stats", "cmoop_eval_population_opt"]
CFG = EvalConfig(lr=3e-3)
B1, B2 = 0.9, 0.999                                    # cmoop_config_default's betas, as EvalConfig.to_struct leaves them


# ---- ABI ---------------------------------------------------------------------------------------------------------------------
def test_abi_symbols_version_and_struct_size():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert name in _lib.OPTIM_PROTOTYPES, name
    assert L.cmoop_abi_version() == 3
    assert C.sizeof(_lib.Optim) == 224                       # api.hip static_asserts the same of cmoop_optim
    assert _lib.Optim.values.offset == 48 and _lib.Optim.warmup_steps.offset == 120 and _lib.Optim.schedule.offset == 200


def test_default_is_all_off():
    st = _lib.Optim()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    _lib.check(_lib.lib().cmoop_optim_default(C.byref(st)))
    assert bytes(st) == bytes(C.sizeof(st)), "every byte zero"
    assert O.default_optim_config() == OptimConfig()
    assert bytes(OptimConfig()._struct()) == bytes(st)
    d = OptimConfig()
    assert not d.enabled and not d.finish_path and EvalConfig().optim is None and EvalConfig(optim=d).optim_struct() is None
    assert OptimConfig(schedule="cosine", decay_steps=5).enabled and not OptimConfig(schedule=1, decay_steps=5).finish_path
    for k in ("weight_decay", "global_clipnorm", "clipvalue"):
        assert OptimConfig(**{k: 0.5}).finish_path


# ---- the domain ----------------------------------------------------------------------------------------------------------------
BAD = [
    (dict(weight_decay=-1e-3), "weight_decay"), (dict(weight_decay=math.nan), "weight_decay"), (dict(weight_decay=math.inf), "weight_decay"),
    (dict(global_clipnorm=-1.0), "global_clipnorm"), (dict(global_clipnorm=math.inf), "global_clipnorm"),
    (dict(clipvalue=-0.5), "clipvalue"), (dict(clipvalue=math.nan), "clipvalue"),
    (dict(global_clipnorm=1.0, clipvalue=1.0), "both"),
    (dict(decay_mask=2), "decay_mask"), (dict(schedule=4), "schedule"), (dict(schedule=-1), "schedule"),
    (dict(schedule=1, decay_steps=0), "decay_steps"), (dict(schedule=1, decay_steps=5, warmup_steps=-1), "warmup_steps"),
    (dict(schedule=1, decay_steps=5, warmup_start=-0.1), "warmup_start"), (dict(schedule=1, decay_steps=5, alpha=math.nan), "alpha"),
    (dict(schedule=1, decay_steps=5, alpha=-1.0), "alpha"),
    (dict(schedule=2, decay_steps=0, decay_rate=0.5), "decay_steps"), (dict(schedule=2, decay_steps=3, decay_rate=-0.5), "decay_rate"),
    (dict(schedule=2, decay_steps=3, decay_rate=math.inf), "decay_rate"),
    (dict(schedule=3, boundaries=(5, 5), values=(1.0, 0.5, 0.1)), "boundaries"),
    (dict(schedule=3, boundaries=(5, 3), values=(1.0, 0.5, 0.1)), "boundaries"),
    (dict(schedule=3, boundaries=(-1,), values=(1.0, 0.5)), "boundaries"),
    (dict(schedule=3, boundaries=(5,), values=(1.0, -0.5)), "values"), (dict(schedule=3, boundaries=(5,), values=(math.nan, 0.5)), "values"),
]


@pytest.mark.parametrize("fields,word", BAD)
def test_check_refuses_each_bad_field_by_name(fields, word):
    with pytest.raises(ValueError, match=word):
        OptimConfig(**fields).check()


def test_check_accepts_the_domain_and_python_side_shape_errors():
    for c in (OptimConfig(), OptimConfig.preset("kws"), OptimConfig.cosine(10, 2, 7, warmup_start=0.1, alpha=0.01, weight_decay=1e-2, decay_mask=1),
              OptimConfig.exponential(2, 0.5, 7, staircase=True, clipvalue=0.5), OptimConfig.piecewise((3, 6), (1.0, 0.1, 0.01), 7, global_clipnorm=1.0),
              OptimConfig(schedule=3, values=(0.5,)), OptimConfig(schedule="piecewise", boundaries=tuple(range(8)), values=tuple([1.0] * 9))):
        assert c.check() is c
    st = _lib.Optim()
    st.schedule, st.n_boundaries = 3, 9
    with pytest.raises(ValueError, match="n_boundaries"):
        O.check_struct(st)
    with pytest.raises(ValueError, match="values"):
        OptimConfig(schedule=3, boundaries=(3,), values=(1.0,))._struct()
    with pytest.raises(ValueError, match="8 boundaries"):
        OptimConfig(schedule=3, boundaries=tuple(range(9)), values=tuple([1.0] * 10))._struct()
    with pytest.raises(ValueError, match="schedule"):
        OptimConfig(schedule="linear").check()
    with pytest.raises(ValueError, match="preset"):
        OptimConfig.preset("nope")
    assert "BUILD-DEFINED" in OptimConfig.preset.__doc__
    assert O.from_struct(OptimConfig.piecewise((3, 6), (1.0, 0.1, 0.01), 7, global_clipnorm=1.0)._struct()) == \
        OptimConfig.piecewise((3, 6), (1.0, 0.1, 0.01), 7, global_clipnorm=1.0)


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
WARM, DECAY = 6, 20
SCHEDULES = {
    "constant": (OptimConfig(weight_decay=1e-2), [0, 1, 5, 6, 26, 1000]),
    # warm-up start, second step, last warm-up step, first decay step, inside, end of decay, beyond
    "cosine": (OptimConfig(schedule=1, warmup_steps=WARM, warmup_start=0.1, decay_steps=DECAY, alpha=0.05),
               [0, 1, WARM - 1, WARM, WARM + 1, WARM + DECAY - 1, WARM + DECAY, WARM + DECAY + 1, 1000]),
    "cosine, no warm-up": (OptimConfig(schedule=1, decay_steps=DECAY), [0, 1, DECAY - 1, DECAY, DECAY + 7]),
    "exponential": (OptimConfig(schedule=2, decay_steps=7, decay_rate=0.5), [0, 1, 6, 7, 8, 13, 14, 700]),
    "exponential, staircase": (OptimConfig(schedule=2, decay_steps=7, decay_rate=0.5, staircase=True), [0, 1, 6, 7, 8, 13, 14, 15, 700]),
    # each boundary and the step after it
    "piecewise": (OptimConfig(schedule=3, boundaries=(0, 3, 4, 10), values=(1.0, 0.5, 0.25, 0.1, 0.01)), [0, 1, 2, 3, 4, 5, 9, 10, 11, 1000]),
    "piecewise, eight boundaries": (OptimConfig(schedule=3, boundaries=tuple(range(2, 18, 2)), values=tuple(0.9 ** k for k in range(9))),
                                    list(range(0, 19)) + [1000]),
}


def ulp32(x):
    return float(np.spacing(np.float32(abs(x))))


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_rates_against_lr_at(name):
    opt, iters = SCHEDULES[name]
    cfg = CFG.to_struct()
    for i in iters:
        lr, lr32, a32 = O.rates(opt, cfg, i)
        want = opt.lr_at(i, CFG.lr)
        assert abs(lr - want) <= 1e-12 * abs(want), (name, i, lr, want)
        assert lr32 == np.float32(lr), (name, i)
        want_a = opt.alpha_at(i, CFG.lr, B1, B2)
        assert abs(float(a32) - want_a) <= ulp32(want_a), (name, i, a32, want_a)
    # the closed forms at the edges
    f = lambda i: opt.factor_at(i)
    if name == "cosine":
        assert f(0) == 0.1 and f(WARM) == 1.0 and abs(f(WARM + DECAY) - 0.05) < 1e-15 and f(1000) == f(WARM + DECAY)
        assert f(WARM - 1) == 0.1 + 0.9 * (WARM - 1) / WARM and f(WARM + 1) < 1.0
    if name == "exponential, staircase":
        assert [f(i) for i in (0, 6, 7, 13, 14)] == [1.0, 1.0, 0.5, 0.5, 0.25]
    if name == "exponential":
        assert f(7) == 0.5 and 0.5 < f(6) < 1.0
    if name == "piecewise":
        assert [f(i) for i in (0, 1, 3, 4, 5, 10, 11)] == [1.0, 0.5, 0.5, 0.25, 0.1, 0.1, 0.01]


def test_constant_schedule_is_todays_expression_bit_for_bit():
    cfg = CFG.to_struct()
    assert (cfg.beta1, cfg.beta2) == (B1, B2)
    for opt in (None, OptimConfig(), OptimConfig(weight_decay=0.1, decay_mask=1), OptimConfig(global_clipnorm=2.0)):
        for i in (0, 1, 9, 10, 999, 1 << 20):
            lr, lr32, a32 = O.rates(opt, cfg, i)
            assert lr == CFG.lr and lr32 == np.float32(CFG.lr)
            want = np.float32(R.keras_alpha(CFG.lr, B1, B2, i + 1))
            assert a32.view(np.uint32) == want.view(np.uint32), (opt, i)
    with pytest.raises(_lib.CmoopError, match="iteration"):
        O.rates(None, cfg, -1)


def test_cosine_helper_counts_steps():
    c = OptimConfig.cosine(epochs=10, warmup_epochs=2, steps_per_epoch=7)
    assert (c.schedule_code, c.warmup_steps, c.decay_steps) == (1, 14, 56)
    assert c.lr_at(14, 1e-3) == 1e-3 and abs(c.lr_at(70, 1e-3)) < 1e-18
    e = OptimConfig.exponential(2, 0.5, 7, staircase=True)
    assert (e.schedule_code, e.decay_steps, e.decay_rate, e.staircase) == (2, 14, 0.5, True)
    p = OptimConfig.piecewise((3, 6), (1.0, 0.1, 0.01), 7)
    assert (p.schedule_code, p.boundaries, p.values) == (3, (21, 42), (1.0, 0.1, 0.01))


# ---- the numpy statement ---------------------------------------------------------------------------------------------------------
def same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def test_adamw_step_ref_with_everything_off_is_the_adam_statement():
    n = 4099
    rs = np.random.RandomState(3)
    w, m, v = rs.randn(n).astype(np.float32), np.zeros(n, np.float32), np.zeros(n, np.float32)
    w2, m2, v2 = w.copy(), m.copy(), v.copy()
    for t in range(1, 6):
        g = R.adam_gradients(n, 40 + t)
        alpha = R.keras_alpha(1e-3, 0.9, 0.999, t)
        w, m, v = R.adam_step_f32(w, g, m, v, alpha, 0.9, 0.999, 1e-7)
        w2, m2, v2 = O.adamw_step_ref(w2, g, m2, v2, alpha, 1e-3, 0.9, 0.999, 1e-7)
        assert same_bits(w, w2) and same_bits(m, m2) and same_bits(v, v2), t


def test_adamw_step_ref_semantics():
    f = np.float32
    w, g = np.array([1.0, -2.0, 3.0, 4.0], f), np.array([0.5, -3.0, 100.0, np.nan], f)
    kinds = np.array([O.KIND_KERNEL, O.KIND_TRAINABLE, O.KIND_FROZEN, O.KIND_KERNEL], np.uint8)
    z = np.zeros(4, f)
    # frozen: untouched; the clamp passes a NaN; decay on kernels only
    w1, m1, v1 = O.adamw_step_ref(w, g, z, z, 0.0, 0.5, 0.9, 0.999, 1e-7, weight_decay=0.5, clipvalue=1.0, kinds=kinds)
    assert w1[0] == f(0.75) and w1[1] == f(-2.0) and w1[2] == f(3.0) and np.isnan(w1[3])
    assert m1[0] == f(0.5) * f(1.0 - 0.9) and m1[1] == f(-1.0) * f(1.0 - 0.9) and m1[2] == 0 and v1[2] == 0 and np.isnan(m1[3])
    w1, _, _ = O.adamw_step_ref(w, g, z, z, 0.0, 0.5, 0.9, 0.999, 1e-7, weight_decay=0.5, decay_mask=1, kinds=kinds)
    assert w1[1] == f(-1.5) and w1[2] == f(3.0)
    _, m1, _ = O.adamw_step_ref(w, g, z, z, 0.0, 0.5, 0.9, 0.999, 1e-7, scale=0.5, kinds=kinds)
    assert m1[0] == f(0.25) * f(1.0 - 0.9)
    ss, norm = O.global_norm_ref(g[:3], kinds[:3])
    assert ss == 9.25 and norm == math.sqrt(9.25)
    assert O.clip_scale_ref(5.0, 5.0) == 1.0 and O.clip_scale_ref(5.0, 0.0) == 1.0 and O.clip_scale_ref(5.0, 2.5) == 0.5


# ---- the kind arena ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A", "B", "A_ds", "B_ds"])
def test_kind_arena_of_every_gene(variant):
    code = G.VARIANT_NAMES[variant]
    for gene in G.all_genes():
        kinds = O.param_kinds(gene, code, 10)
        assert kinds.size == G.param_count(gene, code, 10)
        pos = 0
        for name, shape, role in G.param_tensors(gene, code, 10):
            n = int(np.prod(shape))
            k = kinds[pos:pos + n]
            if role in ("moving_mean", "moving_var"):
                assert (k == O.KIND_FROZEN).all(), (gene, name)      # no moving statistic marked trainable
            elif role == "kernel":
                assert (k == O.KIND_KERNEL).all(), (gene, name)
            else:
                assert (k == O.KIND_TRAINABLE).all(), (gene, name)
            pos += n
        assert (kinds == O.KIND_FROZEN).sum() == (2 * sum(s[0] for _, s, r in G.param_tensors(gene, code, 10) if r == "gamma"))
        assert np.array_equal(kinds, O.param_kinds_lib(gene, code, 10)), (gene, variant)   # the trainer's own walk
    with pytest.raises(_lib.CmoopError, match="parameter count"):
        out = np.empty(5, np.uint8)
        _lib.check(_lib.lib().cmoop_param_kinds((C.c_int32 * 6)(16, 3, 1, 1, 1, 0), code, 10, _lib.ptr(out), 5))
