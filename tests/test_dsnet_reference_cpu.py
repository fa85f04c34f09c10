"""Host-only checks of the depthwise-separable topologies A_ds / B_ds: the test reference itself (grouped convolution and
autograd against explicit float64 tap sums), the closed forms against the tensor list, the library's plan walk and the
oracle twin, the exports, the launch-shape coverage of tests/_ds_shapes.py and the TrainedModel round trip."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import _lib, genes as G
from cmoop_audio_processing_amd.deploy import TrainedModel
from oracle import net as ON

import _dsnet_reference as R
from _ds_shapes import DS_DWCONVS, DS_POINTWISE_CONVS

DS = {"A_ds": "A", "B_ds": "B"}


def _gene(g):
    return (C.c_int32 * 6)(*g)


def _abi_param_count(g, v, classes):
    out = C.c_int64()
    _lib.check(_lib.lib().cmoop_param_count(_gene(g), v, classes, C.byref(out)))
    return int(out.value)


def _abi_flops(g, v, classes, T, F):
    out = C.c_double()
    _lib.check(_lib.lib().cmoop_fwd_flops(_gene(g), v, classes, T, F, C.byref(out)))
    return float(out.value)


def _plan(op, case, stats=0):
    buf = C.create_string_buffer(200)
    _lib.check(_lib.lib().cmoop_conv_launch_plan(op, *case, stats, buf, 200))
    return buf.value.decode()


# ---- the reference -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,H,W,Cn,K", [(2, 3, 2, 4, 3), (1, 6, 7, 4, 5)])
def test_grouped_conv_and_autograd_equal_the_explicit_tap_sums(B, H, W, Cn, K):
    rs = np.random.RandomState(B + H + K)
    x, w, dy = rs.randn(B, H, W, Cn), rs.randn(K, K, Cn), rs.randn(B, H, W, Cn)
    xt = torch.from_numpy(x).permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).requires_grad_(True)
    z = R.depthwise_same(xt, wt)
    assert z.dtype == torch.float64
    z.backward(torch.from_numpy(dy).permute(0, 3, 1, 2))
    assert np.abs(z.detach().permute(0, 2, 3, 1).numpy() - R.dw_forward64(x, w)).max() <= 1e-12
    assert np.abs(xt.grad.permute(0, 2, 3, 1).numpy() - R.dw_dgrad64(dy, w)).max() <= 1e-12
    assert np.abs(wt.grad.numpy() - R.dw_wgrad64(x, dy, K)).max() <= 1e-12
    # the |terms| sums the GPU test's error bound uses dominate the signed ones
    assert (R.dw_forward64(x, w, absolute=True) >= np.abs(R.dw_forward64(x, w)) - 1e-12).all()
    assert (R.dw_wgrad64(x, dy, K, absolute=True) >= np.abs(R.dw_wgrad64(x, dy, K)) - 1e-12).all()


# ---- closed forms ----------------------------------------------------------------------------------------------------------
def test_closed_forms_tensor_list_plan_walk_and_oracle_agree_for_every_gene(monkeypatch):
    import oracle.rng as orng
    monkeypatch.setattr(orng, "glorot_uniform", lambda seed, ti, shape, fi, fo: np.zeros(shape, np.float32))   # skip the hashing
    T, F = 101, 40
    for g in G.all_genes():
        for name, full in DS.items():
            v = G.VARIANT_NAMES[name]
            for classes in (10, 35):
                n = G.param_count(g, v, classes)
                tensors = G.param_tensors(g, v, classes)
                assert n == sum(int(np.prod(s)) for _, s, _ in tensors) == _abi_param_count(g, v, classes)
                onet = R.SeparableOracleNet(g, ON.OracleConfig(variant=v, classes=classes), 0)
                assert n == onet.count_params() and onet.names == [t[0] for t in tensors]
                assert [tuple(onet.T[t[0]].shape) for t in tensors] == [t[1] for t in tensors]
                fl = G.fwd_flops_per_sample(g, v, classes, T, F)
                assert isinstance(fl, int) and float(fl) == _abi_flops(g, v, classes, T, F)
                assert G.model_size_mb(g, v, classes) == n * 4 / 1024 ** 2
                # strictly smaller and cheaper than the full-convolution topology
                assert n < G.param_count(g, G.VARIANT_NAMES[full], classes)
                assert fl < G.fwd_flops_per_sample(g, G.VARIANT_NAMES[full], classes, T, F)
            # per-layer closed forms: k^2 C_in + C_in C_out + C_out parameters
            specs = [s for s in G.layer_specs(g, v, 10) if s["kind"] == "sepconv"]
            assert specs and all(s["cin"] >= 16 and s["k"] == g[1] and s["stride"] == 1 for s in specs)
            by_name = {t[0]: int(np.prod(t[1])) for t in G.param_tensors(g, v, 10)}
            for s in specs:
                got = sum(by_name[s["name"] + sfx] for sfx in ("/depthwise_kernel", "/pointwise_kernel", "/bias"))
                assert got == s["k"] ** 2 * s["cin"] + s["cin"] * s["cout"] + s["cout"]
            # the plan walk lists exactly the separable layers: depthwise halves in cmoop_plan_dwconvs, pointwise halves as
            # the KS = 1, stride = 1 rows of cmoop_plan_convs (the skip projections are KS = 1, stride = 2)
            dws = _lib.plan_dwconvs(g, v, T, F)
            pws = [c for c in _lib.plan_convs(g, v, T, F) if c[4] == 1 and c[5] == 1]
            assert len(dws) == len(pws) == len(specs)
            for s, (H, W, Cn, K), (H2, W2, Ci, Co, _, _, bn) in zip(specs, dws, pws):
                assert (Cn, K) == (s["cin"], s["k"]) and (H2, W2, Ci, Co) == (H, W, s["cin"], s["cout"])
                assert bn == g[2]          # the pointwise half takes the "feeds a BatchNorm" role in both topologies
            assert not [c for c in _lib.plan_convs(g, v, T, F) if c[4] > 1]   # no full k x k GEMM layer is left
        for v in (G.VARIANT_A, G.VARIANT_B):
            assert _lib.plan_dwconvs(g, v, T, F) == []


def test_known_sizes_of_the_low_end():
    """The issue's arithmetic: a 64 -> 64 k5 layer holds 102 464 parameters as a full convolution, 5 760 as a separable one."""
    k, c = 5, 64
    assert k * k * c * c + c == 102464 and k * k * c + c * c + c == 5760
    a = dict((s["name"], s) for s in G.layer_specs((64, 5, 0, 1, 1, 0), G.VARIANT_A_DS, 10))
    assert a["conv2"]["kind"] == "sepconv" and a["conv1"]["kind"] == "conv" and a["res0_skip"]["kind"] == "conv"
    assert G.VARIANT_NAMES["A_ds"] == 2 and G.VARIANT_NAMES["B_ds"] == 3 and G.VARIANT_CODES[2] == "A_ds" and G.VARIANT_CODES[3] == "B_ds"


# ---- exports and unchanged behaviour ---------------------------------------------------------------------------------------
def test_new_symbols_are_exported_and_the_abi_version_stays_3():
    L = _lib.lib()
    for name in ("cmoop_dwconv_fwd", "cmoop_dwconv_bwd", "cmoop_dwconv_wgrad_slices", "cmoop_plan_dwconvs"):
        assert name in _lib.declared_symbols() and hasattr(L, name)
    assert L.cmoop_abi_version() == 3
    hdr = open(_lib.HEADER).read()
    assert "#define CMOOP_ABI_VERSION 3" in hdr and "#define CMOOP_VARIANT_A_DS 2" in hdr and "#define CMOOP_VARIANT_B_DS 3" in hdr
    # variants outside 0..3 are refused, not read as some topology
    out = C.c_int64()
    assert L.cmoop_param_count(_gene((16, 3, 1, 1, 1, 0)), 4, 10, C.byref(out)) != 0
    assert L.cmoop_plan_check(_gene((16, 3, 1, 1, 1, 0)), 4, 101, 40, 64) != 0
    for v in (0, 1, 2, 3):
        assert L.cmoop_plan_check(_gene((64, 5, 1, 3, 4, 1)), v, 101, 40, 256) == 0


KNOWN = [  # SURVEY.md section 2.2 known-answer table: (gene, variant, classes, params)
    ((16, 3, 0, 1, 1, 0), 0, 10, 19674), ((16, 3, 1, 1, 1, 0), 0, 10, 20058), ((16, 3, 1, 1, 1, 0), 0, 11, 20123),
    ((16, 3, 1, 1, 1, 0), 0, 35, 21683), ((32, 3, 1, 2, 2, 0), 0, 10, 324074), ((64, 5, 1, 3, 4, 0), 0, 10, 13624714),
    ((64, 5, 1, 3, 4, 0), 0, 35, 13626339), ((64, 3, 0, 3, 1, 0), 0, 10, 4890634), ((32, 5, 0, 2, 3, 0), 0, 10, 880106),
    ((16, 3, 1, 1, 1, 0), 1, 10, 8298), ((16, 3, 1, 1, 1, 0), 1, 11, 8363), ((16, 3, 1, 1, 1, 0), 1, 35, 9923),
    ((32, 3, 1, 2, 2, 0), 1, 10, 129418), ((64, 5, 1, 3, 4, 0), 1, 10, 4915914), ((64, 3, 0, 3, 1, 0), 1, 10, 1756234),
    ((32, 5, 0, 2, 3, 0), 1, 10, 342282),
]


def test_variants_a_and_b_count_what_they_counted(golden_dir):
    golden = {r["params"]: r["size_mb"] for r in json.load(open(os.path.join(golden_dir, "objectives_golden.json")))["size_mb"]}
    seen = set()
    for g, v, classes, params in KNOWN:
        assert _abi_param_count(g, v, classes) == G.param_count(g, v, classes) == params
        if params in golden:
            assert G.model_size_mb(g, v, classes) == golden[params]
            seen.add(params)
    assert len(seen) >= 10        # the golden file's inputs are the table's


# ---- coverage of the GPU parity cases -------------------------------------------------------------------------------------
def test_ds_shapes_cover_every_pointwise_launch_variant_and_every_depthwise_geometry():
    produced = set()
    for case in DS_POINTWISE_CONVS:
        assert case[5:] == (1, 1)
        produced |= {_plan(0, case, 1), _plan(0, case, 0), _plan(1, case), _plan(2, case)}
    missing, dw_seen = {}, set()
    genes = [g for g in G.all_genes() if g[4] == 1 and g[5] == 0]      # fc / dropout genes add no conv shape
    for g in genes:
        for v in (G.VARIANT_A_DS, G.VARIANT_B_DS):
            for (H, W, Ci, Co, KS, st, bn) in _lib.plan_convs(g, v, 101, 40):
                if (KS, st) != (1, 1):
                    continue
                for B in (64, 37):
                    case = (B, H, W, Ci, Co, 1, 1)
                    for name in (_plan(0, case, bn), _plan(0, case, 0), _plan(1, case), _plan(2, case)):
                        if name not in produced:
                            missing.setdefault(name, case)
            dw_seen |= set(_lib.plan_dwconvs(g, v, 101, 40))
    assert not missing, f"pointwise launch-path variants without a parity case in tests/_ds_shapes.py: {missing}"
    assert dw_seen == set(DS_DWCONVS) and len(DS_DWCONVS) == len(set(DS_DWCONVS)) == 30
    assert any("+stats" in n for n in produced) and any("+sk" in n for n in produced) and any("wgrad" in n for n in produced)


def test_depthwise_slice_counts_are_positive_and_a_function_of_the_shape():
    for (H, W, Cn, K) in DS_DWCONVS:
        s = [_lib.dwconv_wgrad_slices(B, H, W, Cn, K) for B in (1, 2, 37, 64)]
        assert min(s) >= 1 and s == [_lib.dwconv_wgrad_slices(B, H, W, Cn, K) for B in (1, 2, 37, 64)]
    out = C.c_int32()
    L = _lib.lib()
    assert L.cmoop_dwconv_wgrad_slices(1, 8, 8, 24, 3, C.byref(out)) != 0       # channels not a power of two
    assert L.cmoop_dwconv_wgrad_slices(1, 8, 8, 32, 7, C.byref(out)) != 0       # kernel size outside {3, 5}
    assert L.cmoop_dwconv_wgrad_slices(2 ** 12, 128, 128, 16, 3, C.byref(out)) != 0   # 2^30 elements


# ---- TrainedModel -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["A_ds", "B_ds", "A"])
def test_trained_model_round_trip(tmp_path, variant):
    gene, classes = (16, 5, 1, 2, 2, 1), 11
    n = G.param_count(gene, G.VARIANT_NAMES[variant], classes)
    params = np.random.RandomState(3).randn(n).astype(np.float32)
    m = TrainedModel(gene=gene, variant=variant, classes=classes, T=21, F=12, seed=5, params=params,
                     objectives={"acc": 0.5, "size_mb": n * 4 / 1024 ** 2, "fpr": 0.1, "epochs_run": 2})
    path = tmp_path / "m.npz"
    m.save(path)
    m2 = TrainedModel.load(path)
    assert m2.variant == variant and m2.gene == gene and m2.classes == classes and np.array_equal(m2.params, params)
    t = m2.tensors()
    assert list(t) == [x[0] for x in G.param_tensors(gene, G.VARIANT_NAMES[variant], classes)]
    if variant != "A":
        assert t["res0_conv1/depthwise_kernel"].shape == (5, 5, 16) and t["res0_conv1/pointwise_kernel"].shape == (32, 1, 1, 16)
    with np.load(path) as z:
        assert int(z["meta"][0]) == G.VARIANT_NAMES[variant]       # files written for A / B keep their 0 / 1
    with pytest.raises(ValueError):
        TrainedModel(gene=gene, variant="C", classes=classes, T=21, F=12, seed=5, params=params, objectives={})
