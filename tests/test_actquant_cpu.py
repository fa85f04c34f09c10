"""Activation fake quantisation, host side: the struct and its domain, the EvalConfig plumbing, the site rule (C == Python for
every gene and variant) and the properties of the numpy statement the kernels are tested against.  No GPU."""
import ctypes as C
import itertools

import numpy as np
import pytest

from cmoop_audio_processing_amd import EvalConfig, _lib, genes as G, quant as Q

NEW_SYMBOLS = ["cmoop_actquant_default", "cmoop_actquant_check", "cmoop_actquant_sites", "cmoop_fake_quant_act",
               "cmoop_fake_quant_act_time", "cmoop_net_set_actquant", "cmoop_net_get_act_ranges", "cmoop_net_set_act_ranges",
               "cmoop_net_get_act", "cmoop_eval_population_aq"]
GENES = list(itertools.product((16, 32, 64), (3, 5), (0, 1), (1, 2, 3), (1, 2, 3, 4), (0, 1)))
T, F, CLASSES = 21, 12, 10


def test_symbols_structs_and_prototype_arity():
    declared, L = _lib.declared_symbols(), _lib.lib()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name) and name in _lib.ACTQUANT_PROTOTYPES, name
    assert sorted(_lib.ACTQUANT_PROTOTYPES) == sorted(NEW_SYMBOLS)
    assert C.sizeof(_lib.ActQuant) == 16 and C.sizeof(_lib.ActRange) == 16 and Q.ACT_RANGE_DTYPE.itemsize == 16
    assert _lib.ActQuant.momentum.offset == 4 and _lib.ActRange.r.offset == 4 and _lib.ActRange.count.offset == 8
    # _aq is _p with the one more struct pointer
    assert len(_lib.ACTQUANT_PROTOTYPES["cmoop_eval_population_aq"]) == len(_lib.PRUNE_PROTOTYPES["cmoop_eval_population_p"]) + 1
    d = Q.default_act_quant_config()
    assert d.bits == 0 and not d.enabled and np.float32(d.momentum) == np.float32(0.99)


@pytest.mark.parametrize("kw, field", [(dict(bits=1), "bits"), (dict(bits=9), "bits"), (dict(bits=-8), "bits"),
                                       (dict(momentum=1.0), "momentum"), (dict(momentum=-0.1), "momentum"),
                                       (dict(momentum=float("nan")), "momentum")])
def test_domain_errors_name_the_field(kw, field):
    with pytest.raises(ValueError, match=field):
        Q.ActQuantConfig(**kw).check()


def test_reserved_must_be_zero_and_the_domain_passes():
    st = Q.ActQuantConfig(bits=8)._struct()
    st.reserved[1] = 1
    with pytest.raises(ValueError, match="reserved"):
        Q.check_act_struct(st)
    for bits in (0, 2, 3, 4, 5, 6, 7, 8):
        for m in (0.0, 0.5, 0.99, 0.999):
            Q.ActQuantConfig(bits=bits, momentum=m).check()


def test_a_disabled_config_is_no_config():
    assert EvalConfig().act_quant_struct() is None
    assert EvalConfig(act_quant=Q.ActQuantConfig(bits=0)).act_quant_struct() is None
    st = EvalConfig(act_quant=Q.ActQuantConfig(bits=4, momentum=0.9)).act_quant_struct()
    assert st.bits == 4 and np.float32(st.momentum) == np.float32(0.9) and st.reserved[0] == 0 and st.reserved[1] == 0
    with pytest.raises(ValueError, match="bits"):
        EvalConfig(act_quant=Q.ActQuantConfig(bits=12)).act_quant_struct()


def test_site_rule_c_equals_python_for_every_gene_and_variant():
    assert len(GENES) == 288
    for g in GENES:
        for v in range(4):
            assert Q.c_act_sites(g, v, CLASSES, T, F) == Q.act_sites(g, v, CLASSES, T, F), (g, v)


def test_every_site_feeds_a_mac_layer_and_no_other_act_is_a_site():
    for g in GENES:
        for v in range(4):
            acts, ops, logits = Q.act_plan(g, v, CLASSES, T, F)
            sites = {s[0] for s in Q.c_act_sites(g, v, CLASSES, T, F)}
            mac_inputs = {op[1] for op in ops if op[0] in ("conv", "dwconv", "dense", "gap")}
            other_inputs = {i for op in ops if op[0] not in ("conv", "dwconv", "dense", "gap") for i in op[1:3] if i >= 0}
            assert sites <= mac_inputs and 0 not in sites and logits not in sites, (g, v)
            assert not any(acts[i][3] for i in sites), (g, v)
            assert sites == {i for i in mac_inputs if i not in (0, logits) and not acts[i][3]}, (g, v)
            assert not (sites & other_inputs), (g, v)      # nothing that should see the unquantised tensor reads a site
            # the conv inputs are those of the C walk of the MFMA layers: (H, W, Cin) of cmoop_plan_convs, in op order
            convs = [(acts[op[1]][0], acts[op[1]][1], acts[op[1]][2]) for op in ops if op[0] == "conv"]
            assert convs == [tuple(r[:3]) for r in _lib.plan_convs(g, v, T, F)], (g, v)


def test_fake_quant_act_ref_reuses_the_weight_arithmetic():
    rs = np.random.RandomState(0)
    x = rs.randn(7, 33).astype(np.float32)
    for bits in (2, 4, 8):
        a, y = Q.fake_quant_act_ref(x, bits)
        a_w, _s, _q, wq = Q.fake_quant_ref(x.reshape(1, -1), bits)
        assert a.view(np.uint32) == a_w[0].view(np.uint32) and np.array_equal(y.reshape(1, -1).view(np.uint32), wq.view(np.uint32))


@pytest.mark.parametrize("bits", [2, 3, 4, 8])
def test_batch_mode_reaches_qmax_and_stays_within_half_a_step(bits):
    rs = np.random.RandomState(bits)
    qmax = Q.qmax_of(bits)
    for scale in (1e-30, 1e-3, 1.0, 7.5, 1e20):
        x = (rs.randn(4097) * scale).astype(np.float32)
        a, y = Q.fake_quant_act_ref(x, bits)
        s = np.float32(a / np.float32(qmax))
        q = np.rint(y.astype(np.float64) / np.float64(s))
        assert np.abs(q).max() == qmax                                   # the largest code is exactly qmax
        assert np.array_equal(y, (q.astype(np.float32) * s).astype(np.float32))
        bound = np.float64(s) / 2 + 2.0 ** -22 * np.float64(a) + qmax * 2.0 ** -149
        assert (np.abs(y.astype(np.float64) - x.astype(np.float64)) <= bound).all()


def test_tracked_mode_clamps_and_special_values():
    x = np.asarray([-9.0, -1.0, -0.0, 0.0, 0.26, 3.0, 100.0], np.float32)
    a, y = Q.fake_quant_act_ref(x, 8, a=np.float32(2.0))
    assert a == np.float32(2.0) and y[0] == -2.0 and y[-1] == 2.0 and y[-2] == 2.0 and np.abs(y).max() == 2.0
    assert y[2] == 0 and y[3] == 0
    _a, z = Q.fake_quant_act_ref(np.zeros(5, np.float32), 8)
    assert np.array_equal(z.view(np.uint32), np.zeros(5, np.uint32))
    a, n = Q.fake_quant_act_ref(np.asarray([1.0, np.nan, -2.0], np.float32), 8)
    assert np.isnan(a) and (n.view(np.uint32) == Q.CANONICAL_NAN).all()
    _a, t = Q.fake_quant_act_ref(np.asarray([0.5, 1.5, 2.5, -0.5, -1.5], np.float32), 8, a=np.float32(127.0))   # s = 1: exact ties
    assert np.array_equal(t, np.asarray([0.0, 2.0, 2.0, -0.0, -2.0], np.float32))


def test_range_recurrence_against_float64_rounded_once_per_operation():
    rs = np.random.RandomState(3)
    for momentum in (0.0, 0.5, 0.9, 0.99, 0.999):
        mu = np.float32(momentum)
        omu = np.float32(1.0 - np.float64(mu))
        assert Q.act_momentum_pair(momentum) == (mu, omu)
        r, count = np.float32(0), 0
        for m_b in np.abs(rs.randn(20)).astype(np.float32) * np.float32(3):
            new = Q.act_range_update_ref(r, m_b, count, momentum)
            if count == 0:
                want = m_b
            else:      # float64 holds every float32 product and sum of two float32 exactly enough to round once
                want = np.float32(np.float64(np.float32(np.float64(mu) * np.float64(r))) + np.float64(np.float32(np.float64(omu) * np.float64(m_b))))
            assert new.view(np.uint32) == np.float32(want).view(np.uint32)
            r, count = new, count + 1
    nan = Q.act_range_update_ref(np.float32(1.0), np.float32(np.nan), 3, 0.9)
    assert np.asarray([nan]).view(np.uint32)[0] == Q.CANONICAL_NAN
    assert np.asarray([Q.act_range_update_ref(np.float32(1.0), np.float32(np.nan), 0, 0.9)]).view(np.uint32)[0] == Q.CANONICAL_NAN


def test_trained_model_carries_ranges_through_save_and_load(tmp_path):
    from cmoop_audio_processing_amd.deploy import TrainedModel
    g = (16, 3, 1, 1, 1, 0)
    n = G.param_count(g, 0, CLASSES)
    sites = Q.act_sites(g, "A", CLASSES, T, F)
    rec = np.zeros(len(sites), Q.ACT_RANGE_DTYPE)
    rec["m_b"], rec["r"], rec["count"] = np.arange(len(sites)) + 1, np.arange(len(sites)) + 0.5, 7
    base = dict(gene=g, variant="A", classes=CLASSES, T=T, F=F, seed=1, params=np.zeros(n, np.float32), objectives={"acc": 0.5})
    m = TrainedModel(**base, act_bits=8, act_ranges=rec)
    m.save(tmp_path / "m.npz")
    back = TrainedModel.load(tmp_path / "m.npz")
    assert back.act_bits == 8 and np.array_equal(back.act_ranges, rec)
    plain = TrainedModel(**base)
    plain.save(tmp_path / "p.npz")
    with np.load(tmp_path / "p.npz") as z:
        assert not any(k.startswith("act_") for k in z.files)                # absent when off: old files load, new ones stay old
    assert TrainedModel.load(tmp_path / "p.npz").act_ranges is None
    with pytest.raises(ValueError, match="act_"):
        TrainedModel(**base, act_bits=8)
    with pytest.raises(ValueError, match="site"):
        TrainedModel(**base, act_bits=8, act_ranges=rec[:-1])
