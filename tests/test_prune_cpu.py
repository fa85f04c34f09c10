"""CPU: magnitude pruning in training (include/cmoop.h, cmoop_prune) -- the numpy restatement, the schedule against the C
function bit for bit, the size closed form and the table against the C ABI for every gene, the config's domain, and
TrainedModel's pruned kernels.  No GPU: everything here is host code of the library or pure numpy."""
import ctypes as C
import dataclasses
import struct

import numpy as np
import pytest

from cmoop_audio_processing_amd import (EvalConfig, PruneConfig, QuantConfig, TrainedModel, _lib, genes as G)
from cmoop_audio_processing_amd import prune as PR
from cmoop_audio_processing_amd import quant as Q

F32 = np.float32
NEW_SYMBOLS = ["cmoop_prune_default", "cmoop_prune_check", "cmoop_prune_sparsity_at", "cmoop_prune_table", "cmoop_prune_size_bytes",
               "cmoop_prune_weights", "cmoop_prune_weights_time", "cmoop_net_set_prune", "cmoop_net_get_pruned",
               "cmoop_eval_population_p"]


def bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def keys(a):
    return bits(a) & np.uint32(0x7FFFFFFF)


# ---- the restatement -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ln", [1, 2, 9, 64, 1000, 4097])
def test_prune_ref_prunes_exactly_k_on_tie_free_input(ln):
    rs = np.random.RandomState(ln)
    mag = (np.arange(ln) + 1).astype(F32) * F32(0.37)               # distinct magnitudes
    w = (rs.permutation(mag) * rs.choice([-1, 1], ln)).astype(F32)
    assert np.unique(keys(w)).size == ln
    for k in sorted({0, 1, ln // 2, ln - 1, ln}):
        out, zeros = PR.prune_ref(w, k)
        assert zeros == k and int((keys(out) == 0).sum()) == k
        order = np.argsort(keys(w), kind="stable")
        assert not out[order[:k]].any() and np.array_equal(bits(out[order[k:]]), bits(w[order[k:]])), "the k smallest, nothing else"
        assert not np.signbit(out[order[:k]]).any(), "a pruned element is +0.0"
    assert np.array_equal(bits(PR.prune_ref(w, 0)[0]), bits(w)), "k = 0 is a bit copy"
    with pytest.raises(ValueError):
        PR.prune_ref(w, ln + 1)


def test_prune_ref_prunes_at_least_k_under_ties_and_does_not_depend_on_order():
    w = np.array([0.5, -0.5, 0.25, 0.5, 2.0, -0.5, 1.0, -0.25], F32)
    out, zeros = PR.prune_ref(w, 3)              # the third smallest key is 0.5, and four keys tie there
    assert zeros == 6 and np.array_equal(out, np.array([0, 0, 0, 0, 2.0, 0, 1.0, 0], F32))
    out, zeros = PR.prune_ref(w, 2)
    assert zeros == 2 and np.array_equal(out, np.array([0.5, -0.5, 0, 0.5, 2.0, -0.5, 1.0, 0], F32))
    rs = np.random.RandomState(0)
    w = rs.choice(np.array([-2, -1, -.5, 0, .5, 1, 2, 3], F32), 500).astype(F32)
    for k in (1, 100, 250, 499):
        out, zeros = PR.prune_ref(w, k)
        assert zeros >= k
        p = rs.permutation(w.size)
        out_p, zeros_p = PR.prune_ref(w[p], k)
        assert zeros_p == zeros and np.array_equal(bits(out_p), bits(out[p]))
        t = np.sort(keys(w))[k - 1]
        assert np.array_equal(keys(out) == 0, keys(w) <= t)


def test_prune_ref_keeps_nan_and_inf_and_gives_plus_zero_from_minus_zero():
    w = np.array([1.0, -0.0, np.nan, np.inf, -2.0, 0.5, -np.inf, 3.0, 1e-45, -1e-40], F32)
    w.view(np.uint32)[2] = 0xFFC12345            # a negative NaN with a payload
    out, zeros = PR.prune_ref(w, 6)              # -0.0, two denormals, 0.5, 1.0, -2.0
    assert zeros == 6
    assert bits(out).tolist() == [0, 0, 0xFFC12345, 0x7F800000, 0, 0, 0xFF800000, bits(F32(3.0)).item(), 0, 0]
    out, zeros = PR.prune_ref(w, 9)              # everything but the NaN: a NaN outranks inf
    assert zeros == 9 and bits(out).tolist() == [0, 0, 0xFFC12345] + [0] * 7
    out, zeros = PR.prune_ref(np.array([-0.0, 0.0, -0.0, 1.0], F32), 1)
    assert zeros == 3 and bits(out).tolist() == [0, 0, 0, bits(F32(1.0)).item()], "-0.0 has key 0 and becomes +0.0"
    assert bits(PR.prune_ref(np.array([-0.0, 1.0], F32), 0)[0]).tolist() == [0x80000000, 0x3F800000], "k = 0 copies -0.0"


# ---- the schedule ----------------------------------------------------------------------------------------------------------------
def dbits(x):
    return struct.pack("<d", x)


SCHEDULES = [(0.8, 0, 0), (0.8, 0, 100), (0.5, 7, 53), (0.95, 10, 11), (0.95, 10, 10), (0.3, 20, 5), (0.999, 3, 1000),
             (0.123456789, 0, 7), (0.8, 1000000, 2000000000)]


@pytest.mark.parametrize("sparsity,begin,end", SCHEDULES)
def test_sparsity_at_equals_the_c_function_bit_for_bit(sparsity, begin, end):
    cfg = PruneConfig(sparsity=sparsity, begin_step=begin, end_step=end).check()
    its = sorted(set(list(range(0, 130)) + [begin - 1, begin, begin + 1, end - 1, end, end + 1, (begin + end) // 2, 10 ** 9,
                                           2 ** 31, 2 ** 40] + list(range(max(begin, 0), max(end, begin) + 2, max(1, (end - begin) // 97)))))
    prev = 0.0
    for it in (i for i in its if i >= 0):
        s = PR.sparsity_at(cfg, it)
        assert dbits(s) == dbits(PR.c_sparsity_at(cfg, it)), (it, s)
        assert 0.0 <= s <= sparsity and s >= prev, "monotone, inside [0, sparsity]"
        prev = s
        if it < begin:
            assert s == 0.0
        if it >= end or end <= begin:
            assert s == (sparsity if it >= begin else 0.0)
    if end > begin + 1:
        mid = begin + (end - begin) // 2
        u = (mid - begin) / (end - begin)
        assert PR.sparsity_at(cfg, mid) == pytest.approx(sparsity * (1 - (1 - u) ** 3), rel=1e-12)


def test_polynomial_counts_in_epochs():
    cfg = PruneConfig.polynomial(0.8, 1, 4, 25, objective=False)
    assert cfg == PruneConfig(sparsity=0.8, begin_step=25, end_step=100, objective=False, skip_small=True)
    assert PR.sparsity_at(cfg, 24) == 0.0 and PR.sparsity_at(cfg, 25) == 0.0 and PR.sparsity_at(cfg, 100) == 0.8
    assert 0.0 < PR.sparsity_at(cfg, 26) < PR.sparsity_at(cfg, 99) < 0.8


# ---- size and table ----------------------------------------------------------------------------------------------------------------
def c_param_kinds(gene, variant, classes):
    n = G.param_count(gene, variant, classes)
    kinds = np.zeros(n, np.uint8)
    g = (C.c_int32 * 6)(*gene)
    _lib.check(_lib.lib().cmoop_param_kinds(g, C.c_int32(variant), C.c_int32(classes), _lib.ptr(kinds), C.c_int64(n)))
    return kinds


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_size_c_equals_python_for_every_gene(variant):
    all_genes = list(G.all_genes())
    assert len(all_genes) == 288
    for gene in all_genes:
        fp32 = 4 * G.param_count(gene, variant, 10)
        for sparsity in (0.5, 0.8, 0.95):
            for nbits in (0, 8, 4):
                py = G.prune_size_bytes(gene, variant, 10, sparsity, nbits)
                assert py == PR.c_prune_size_bytes(gene, variant, 10, sparsity, nbits), (gene, sparsity, nbits)
                assert py < fp32, "below size_mb whenever sparsity > 1/8"
                if nbits:
                    assert py < G.quant_size_bytes(gene, variant, 10, nbits), "and, quantised, below the dense quantised model"
        assert G.prune_size_bytes(gene, variant, 10, 0.126) < fp32
        assert G.prune_size_mb(gene, variant, 10, 0.8, 8) == G.prune_size_bytes(gene, variant, 10, 0.8, 8) / 2 ** 20


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
@pytest.mark.parametrize("classes", [10, 11])
def test_table_equals_the_c_table_for_every_gene(variant, classes):
    for gene in G.all_genes():
        rows = PR.prune_table(gene, variant, classes)
        assert rows == PR.c_prune_table(gene, variant, classes), gene
        dense = PR.prune_table(gene, variant, classes, skip_small=False)
        assert dense == PR.c_prune_table(gene, variant, classes, skip_small=False)
        assert [r[:2] for r in rows] == [r[:2] for r in dense] and all(r[2] == -1 for r in dense)
        # the same tensors as the quantiser's table, each as one contiguous span, and exactly the KIND_KERNEL elements
        qrows = Q.quant_table(gene, variant, classes)
        assert [(r[0], r[1]) for r in rows] == [(q[0], q[1] * q[2]) for q in qrows]
        assert [r[2] for r in rows] == [-1 if (q[4] == 1 and i > 0) else 0 for i, q in enumerate(qrows)], "row tensors but the first conv"
        covered = np.zeros(G.param_count(gene, variant, classes), np.int32)
        for off, n, _k in rows:
            covered[off:off + n] += 1
        assert np.array_equal(covered == 1, c_param_kinds(gene, variant, classes) == 0) and covered.max() == 1


def test_size_formula_by_hand():
    gene, v = (16, 3, 1, 1, 1, 1), 2     # A_ds: conv1, a separable conv2, a skip, two separable body convs, fc1, output
    kernels = [(n, int(np.prod(s)), s) for n, s, r in G.param_tensors(gene, v, 10) if r == "kernel"]
    channels = sum(s[2] if n.endswith("/depthwise_kernel") else s[0] for n, _e, s in kernels)
    elems = sum(e for _n, e, _s in kernels)
    rest = 4 * (G.param_count(gene, v, 10) - elems)
    for sparsity in (0.5, 0.8, 0.999, 0.001):
        for nbits in (0, 2, 5, 8):
            want = rest + (4 * channels if nbits else 0)
            for i, (n, e, _s) in enumerate(kernels):
                k = 0 if (i == 0 or n.endswith("/depthwise_kernel")) else int(np.floor(sparsity * e))
                want += ((e + 7) // 8 if k else 0) + (((e - k) * nbits + 7) // 8 if nbits else 4 * (e - k))
            assert G.prune_size_bytes(gene, v, 10, sparsity, nbits) == want == PR.c_prune_size_bytes(gene, v, 10, sparsity, nbits)
    for nbits in (2, 8):
        assert G.prune_size_bytes(gene, v, 10, 0.0, nbits) == G.quant_size_bytes(gene, v, 10, nbits), "nothing pruned: the quantised size"
    assert G.prune_size_bytes(gene, v, 10, 0.0) == 4 * G.param_count(gene, v, 10), "nothing pruned, fp32: size_mb"
    assert G.prune_size_bytes(gene, v, 10, 0.8, 0, skip_small=False) == PR.c_prune_size_bytes(gene, v, 10, 0.8, 0, skip_small=False) \
        < G.prune_size_bytes(gene, v, 10, 0.8)
    with pytest.raises(ValueError):
        G.prune_size_bytes(gene, v, 10, 1.0)
    with pytest.raises(ValueError):
        G.prune_size_bytes(gene, v, 10, 0.5, 1)
    g, out = (C.c_int32 * 6)(*gene), C.c_int64()
    L = _lib.lib()
    assert L.cmoop_prune_size_bytes(g, v, 10, C.c_double(0.5), 9, 1, C.byref(out)) != 0 and "bits" in L.cmoop_last_error().decode()
    assert L.cmoop_prune_size_bytes(g, v, 10, C.c_double(1.0), 0, 1, C.byref(out)) != 0 and "sparsity" in L.cmoop_last_error().decode()
    small = np.zeros((2, 3), np.int64)
    assert L.cmoop_prune_table(g, v, 10, 1, _lib.ptr(small), 2, None) != 0


def test_prune_params_ref_layout():
    gene, v = (16, 5, 1, 1, 2, 0), 3
    rs = np.random.RandomState(7)
    flat = rs.randn(G.param_count(gene, v, 10)).astype(F32)
    out, zeros = PR.prune_params_ref(flat, gene, v, 10, 0.8)
    kinds = c_param_kinds(gene, v, 10)
    assert np.array_equal(bits(out[kinds != 0]), bits(flat[kinds != 0])), "everything but the kernels is a bit copy"
    rows = PR.prune_table(gene, v, 10)
    assert zeros.dtype == np.uint32 and zeros.size == len(rows)
    for (off, n, k), z in zip(rows, zeros):
        if k == 0:
            assert z == 0 and np.array_equal(bits(out[off:off + n]), bits(flat[off:off + n])), "the first conv and the depthwise kernels"
        else:
            assert z == PR.k_of(n, 0.8) == int((out[off:off + n] == 0).sum()), "randn has no ties"
    assert np.array_equal(bits(PR.prune_params_ref(flat, gene, v, 10, 0.0)[0]), bits(flat))
    # prune, then quantise: a pruned element has code 0
    wq, codes, _scales = Q.quantize_params_ref(out, gene, v, 10, 8)
    assert not codes[(out == 0) & (kinds == 0)].any() and not wq[(out == 0) & (kinds == 0)].any()


# ---- ABI and configs ---------------------------------------------------------------------------------------------------------------
def test_abi_symbols_version_and_struct_size():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert name in _lib.PRUNE_PROTOTYPES, name
    assert L.cmoop_abi_version() == 3, "functions are added only"
    assert C.sizeof(_lib.Prune) == 24                         # api.hip static_asserts the same of cmoop_prune
    P = _lib.Prune
    assert (P.sparsity.offset, P.begin_step.offset, P.end_step.offset, P.objective.offset, P.skip_small.offset) == (0, 8, 12, 16, 20)
    # cmoop_eval_population_p is _q with one more struct pointer and one more output
    assert len(_lib.PRUNE_PROTOTYPES["cmoop_eval_population_p"]) == len(_lib.QUANT_PROTOTYPES["cmoop_eval_population_q"]) + 2


def test_default_is_off():
    st = _lib.Prune()
    C.memset(C.byref(st), 0xFF, C.sizeof(st))
    _lib.check(_lib.lib().cmoop_prune_default(C.byref(st)))
    assert (st.sparsity, st.begin_step, st.end_step, st.objective, st.skip_small) == (0.0, 0, 0, 0, 1)
    assert PR.default_prune_config() == PruneConfig(sparsity=0.0, objective=False) and not PruneConfig(sparsity=0.0).enabled
    assert PruneConfig() == PruneConfig(0.8, 0, 0, True, True) and PruneConfig().enabled
    assert _lib.lib().cmoop_prune_default(None) != 0


BAD = [(dict(sparsity=1.0), "sparsity"), (dict(sparsity=-0.1), "sparsity"), (dict(sparsity=float("nan")), "sparsity"),
       (dict(sparsity=1.5), "sparsity"), (dict(sparsity=0.5, begin_step=-1), "begin_step"), (dict(sparsity=0.5, end_step=-2), "end_step"),
       (dict(sparsity=0.5, objective=2), "objective"), (dict(sparsity=0.0, skip_small=3), "skip_small"),
       (dict(sparsity=0.5, skip_small=-1), "skip_small")]


@pytest.mark.parametrize("fields,word", BAD)
def test_check_rejects_and_names_the_field(fields, word):
    st = _lib.Prune()
    st.skip_small = 1
    for k, v in fields.items():
        setattr(st, k, v)
    L = _lib.lib()
    assert L.cmoop_prune_check(C.byref(st)) != 0
    assert word in L.cmoop_last_error().decode()
    with pytest.raises(ValueError, match=word):
        PR.check_struct(st)
    out = C.c_double()
    assert L.cmoop_prune_sparsity_at(C.byref(st), 0, C.byref(out)) != 0


def test_check_accepts_the_domain_and_config_travels():
    for s in (0.0, 1e-9, 0.5, 0.999999):
        for o in (False, True):
            for sk in (False, True):
                cfg = PruneConfig(sparsity=s, begin_step=3, end_step=2, objective=o, skip_small=sk)
                assert cfg.check() is cfg
    L = _lib.lib()
    assert L.cmoop_prune_check(None) != 0 and "NULL" in L.cmoop_last_error().decode()
    assert EvalConfig().prune is None and EvalConfig().prune_struct() is None and EvalConfig().prune_size_mb((16, 3, 1, 1, 1, 1)) is None
    assert EvalConfig(prune=PruneConfig(sparsity=0.0)).prune_struct() is None, "a disabled config is no config"
    st = EvalConfig(prune=PruneConfig(sparsity=0.75, begin_step=5, end_step=9, objective=False, skip_small=False)).prune_struct()
    assert (st.sparsity, st.begin_step, st.end_step, st.objective, st.skip_small) == (0.75, 5, 9, 0, 0)
    with pytest.raises(ValueError, match="sparsity"):
        EvalConfig(prune=PruneConfig(sparsity=2.0)).prune_struct()
    gene = (16, 3, 1, 1, 1, 1)
    both = EvalConfig(variant="B_ds", prune=PruneConfig(sparsity=0.5), quant=QuantConfig(bits=4))
    assert both.prune_size_mb(gene) == G.prune_size_mb(gene, 3, 10, 0.5, 4)
    assert dataclasses.replace(both, quant=None).prune_size_mb(gene) == G.prune_size_mb(gene, 3, 10, 0.5)


def test_with_two_bad_options_the_earlier_one_is_reported():
    """The population call checks its structs in the order augment, loss, distill, optim, ema, opoint, quant, prune: a bad
    quantiser is reported before a bad pruner, a bad pruner when it is the only one.  Host only: the check precedes everything."""
    L = _lib.lib()
    cfg, ds = EvalConfig().to_struct(), _lib.DatasetStruct()
    ds.T, ds.F = 26, 10
    genes, seeds = np.array([[16, 3, 1, 1, 1, 1]], np.int32), np.array([1], np.uint32)
    bad_q, bad_p, good_p = _lib.Quant(), PruneConfig(sparsity=0.5)._struct(), PruneConfig(sparsity=0.5)._struct()
    bad_q.bits = 9
    bad_p.skip_small = 7

    def call(q, p):
        rc = L.cmoop_eval_population_p(C.byref(cfg), None, None, None, None, None, None, C.byref(q) if q is not None else None,
                                       C.byref(p) if p is not None else None, C.byref(ds), _lib.ptr(genes), _lib.ptr(seeds), 0, None,
                                       None, None, None, None, None, None, None, None, None, None, None)
        return rc, L.cmoop_last_error().decode()
    rc, msg = call(bad_q, bad_p)
    assert rc != 0 and "bits" in msg and "skip_small" not in msg
    rc, msg = call(None, bad_p)
    assert rc != 0 and "skip_small" in msg
    rc, msg = call(None, good_p)
    assert rc == 0, msg                       # n = 0: nothing to train, nothing touched


# ---- TrainedModel --------------------------------------------------------------------------------------------------------------------
GENE, VAR = (16, 3, 1, 1, 1, 1), "A_ds"


def make_model(sparsity=None, quant_bits=None):
    rs = np.random.RandomState(3)
    v = G.VARIANT_NAMES[VAR]
    flat = rs.randn(G.param_count(GENE, v, 10)).astype(F32)
    kw = {}
    if sparsity is not None:
        flat, _zeros = PR.prune_params_ref(flat, GENE, v, 10, sparsity)
        kw = dict(prune_sparsity=sparsity, prune_k=[PR.row_k(r, sparsity) for r in PR.prune_table(GENE, v, 10)])
    if quant_bits is not None:
        flat, codes, scales = Q.quantize_params_ref(flat, GENE, v, 10, quant_bits)
        kw.update(quant_bits=quant_bits, quant_codes=codes, quant_scales=scales)
    return TrainedModel(gene=GENE, variant=VAR, classes=10, T=21, F=12, seed=5, params=flat,
                        objectives={"acc": 0.5, "size_mb": 0.01, "fpr": 0.1, "epochs_run": 3}, **kw)


@pytest.mark.parametrize("sparsity,quant_bits", [(None, None), (0.8, None), (0.5, 8)])
def test_trained_model_round_trip_with_and_without_the_prune_keys(tmp_path, sparsity, quant_bits):
    m = make_model(sparsity, quant_bits)
    path = tmp_path / "model.npz"
    m.save(path)
    with np.load(path, allow_pickle=False) as z:
        assert [k in z.files for k in ("prune_sparsity", "prune_k")] == [sparsity is not None] * 2, "written only when present"
    back = TrainedModel.load(path)
    assert np.array_equal(bits(back.params), bits(m.params)) and back.prune_sparsity == sparsity and back.quant_bits == quant_bits
    if sparsity is None:
        assert back.prune_k is None
        with pytest.raises(ValueError, match="no pruned"):
            back.sparsity_report()
        return
    assert back.prune_k.dtype == np.int64 and np.array_equal(back.prune_k, m.prune_k)
    rep = back.sparsity_report()
    names = [n for n, _s, r in G.param_tensors(GENE, G.VARIANT_NAMES[VAR], 10) if r == "kernel"]
    assert list(rep) == names + ["total"]
    for name, k in zip(names, back.prune_k):
        r = rep[name]
        assert r["k"] == k and r["zeros"] >= k and r["sparsity"] == r["zeros"] / r["elements"]
        assert r["zeros"] == int((back.tensors()[name] == 0).sum())
        if k and quant_bits is None:
            assert r["zeros"] == k, "randn has no ties"
    assert rep["total"]["sparsity"] >= sparsity - 1e-3 and rep["total"]["k"] == int(back.prune_k.sum())


def test_post_init_rejects_a_model_that_is_not_as_sparse_as_it_says():
    m = make_model(0.8)
    i = int(np.argmax(m.prune_k))
    name, off, n = m._kernel_spans()[i]
    dense = m.params.copy()
    dense[off:off + n][dense[off:off + n] == 0] = 1.0
    with pytest.raises(ValueError, match=name):
        dataclasses.replace(m, params=dense)
    with pytest.raises(ValueError, match="one value per kernel tensor"):
        dataclasses.replace(m, prune_k=m.prune_k[:-1])
    with pytest.raises(ValueError, match="come together"):
        dataclasses.replace(m, prune_k=None)
    with pytest.raises(ValueError, match="prune_sparsity"):
        dataclasses.replace(m, prune_sparsity=1.0)
