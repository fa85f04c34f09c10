"""Integer depthwise, the host side: the numpy statement against a plain loop nest (H = 1, W < K, the extreme accumulators,
scale 0), the plan (which ops run, their alignment, their sites and readers over the whole search space), the exported symbols
and the TrainedModel refusal.  No GPU.  Every test fails without the feature."""
import ctypes as C

import numpy as np
import pytest

from cmoop_audio_processing_amd import _lib, genes as G, quant as Q

NEW_SYMBOLS = ["cmoop_dwconv_fwd_i8", "cmoop_dwconv_fwd_i8_time", "cmoop_int8_dw_ops", "cmoop_net_set_int8_depthwise",
               "cmoop_net_int8_dw_ops", "cmoop_fake_quant_act_codes_time"]
T, F = 101, 40
ACC_MAX = 25 * 127 * 127


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _loop_dw(qx, qw, s_x, s_w):
    """A plain Python-int loop nest, SAME padding, then the float32 epilogue one operation at a time -> (acc, z)."""
    f = np.float32
    B, H, W, Cn = qx.shape
    K = qw.shape[0]
    p = (K - 1) // 2
    acc, z = np.zeros((B, H, W, Cn), np.int64), np.zeros((B, H, W, Cn), f)
    for b in range(B):
        for h in range(H):
            for w in range(W):
                for c in range(Cn):
                    a = 0
                    for ky in range(K):
                        for kx in range(K):
                            ih, iw = h + ky - p, w + kx - p
                            if 0 <= ih < H and 0 <= iw < W:
                                a += int(qx[b, ih, iw, c]) * int(qw[ky, kx, c])
                    acc[b, h, w, c] = a
                    z[b, h, w, c] = f(f(np.int32(a)) * f(f(s_x) * f(s_w[c])))
    return acc, z


@pytest.mark.parametrize("shape", [(1, 1, 1, 3, 3), (2, 1, 4, 2, 5),       # H = 1
                                   (1, 5, 3, 3, 5), (2, 4, 2, 2, 3),       # W < K
                                   (2, 6, 7, 3, 3), (1, 7, 6, 2, 5)])
def test_ref_equals_a_plain_loop_nest(shape):
    B, H, W, Cn, K = shape
    rs = np.random.RandomState(sum(shape))
    qx = rs.randint(-127, 128, (B, H, W, Cn)).astype(np.int8)
    qw = rs.randint(-127, 128, (K, K, Cn)).astype(np.int8)
    s_w = (rs.rand(Cn) * 0.01 + 1e-4).astype(np.float32)
    acc, z = _loop_dw(qx, qw, np.float32(0.031), s_w)
    assert np.array_equal(Q.dwconv_i8_acc(qx, qw), acc)
    assert np.array_equal(Q.dwconv_i8_acc(qx, qw.reshape(-1), KS=K), acc), "flat weight codes with KS"
    got = Q.dwconv_i8_ref(qx, qw, 0.031, s_w)
    assert got.dtype == np.float32 and got.shape == z.shape and np.array_equal(_bits(got), _bits(z))
    # with an output range the statement composes with the activation quantiser's
    for bits, a in ((8, float(np.abs(z).max()) / 3), (4, float(np.abs(z).max())), (8, 0.0)):
        y, q = Q.dwconv_i8_ref(qx, qw, 0.031, s_w, out_bits=bits, a_out=a)
        assert np.array_equal(_bits(y), _bits(Q.fake_quant_act_ref(z, bits, a)[1])) and np.array_equal(q, Q.act_codes_ref(z, bits, a))
        assert q.dtype == np.int8 and np.array_equal(_bits((q.astype(np.float32) * Q.act_scale_ref(a, bits)).astype(np.float32)), _bits(y))


@pytest.mark.parametrize("K", [3, 5])
def test_extreme_codes_reach_the_accumulator_bound_exactly(K):
    H = W = 2 * K - 1
    for sx, sw in ((127, 127), (-127, 127), (127, -127), (-127, -127)):
        qx, qw = np.full((1, H, W, 2), sx, np.int8), np.full((K, K, 2), sw, np.int8)
        acc, z = _loop_dw(qx, qw, np.float32(1.0), np.ones(2, np.float32))
        got = Q.dwconv_i8_acc(qx, qw)
        assert np.array_equal(got, acc)
        centre, want = got[0, H // 2, W // 2, 0], K * K * 127 * 127 * (1 if sx * sw > 0 else -1)
        assert centre == want and abs(int(got.min())) <= ACC_MAX and abs(int(got.max())) <= ACC_MAX
        if K == 5:
            assert abs(int(centre)) == 403225 and 403225 < 2 ** 24
        assert np.array_equal(_bits(Q.dwconv_i8_ref(qx, qw, 1.0, np.ones(2, np.float32))), _bits(z))
        assert Q.dwconv_i8_ref(qx, qw, 1.0, np.ones(2, np.float32))[0, H // 2, W // 2, 0] == np.float32(want)


def test_scale_zero_gives_plus_zero_in_bytes():
    rs = np.random.RandomState(5)
    qx = rs.randint(-127, 128, (1, 4, 3, 4)).astype(np.int8)
    qw = rs.randint(-127, 128, (3, 3, 4)).astype(np.int8)
    s_w = np.asarray([0.0, 0.01, 0.0, 0.02], np.float32)
    z = Q.dwconv_i8_ref(qx, qw, 0.5, s_w)
    assert (np.abs(z[..., 0]) == 0).all() and (np.abs(z[..., 2]) == 0).all() and np.abs(z[..., 1]).max() > 0
    # an output range of 0 (s > 0 false): codes 0 and y = +0.0 in bytes, whatever the sign of z
    y, q = Q.dwconv_i8_ref(qx, qw, 0.5, s_w, out_bits=8, a_out=0.0)
    assert (z < 0).any() and (_bits(y) == 0).all() and (q == 0).all()
    # an input scale of 0: z is a signed zero, the quantised value +0.0
    y, q = Q.dwconv_i8_ref(qx, qw, 0.0, s_w, out_bits=8, a_out=1.0)
    assert (_bits(y) == 0).all() and (q == 0).all()


def test_bad_weight_shapes_are_refused():
    qx = np.zeros((1, 3, 3, 2), np.int8)
    for qw, ks in ((np.zeros((3, 5, 2), np.int8), None), (np.zeros(18, np.int8), None), (np.zeros((7, 7, 2), np.int8), None),
                   (np.zeros(8, np.int8), 2)):
        with pytest.raises(ValueError):
            Q.dwconv_i8_acc(qx, qw, ks)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_int8_dw_ops_c_equals_python_and_every_op_fits_the_kernel(variant):
    for classes in (10, 35):
        for gene in G.all_genes():
            rows = Q.c_int8_dw_ops(gene, variant, classes, T, F)
            want = Q.int8_dw_ops(gene, variant, classes, T, F)
            assert [(r["op"], r["in_act"], r["out_act"]) for r in rows] == want, (gene, variant)
            assert bool(rows) == (variant >= 2), "empty for A / B, non-empty for the separable variants"
            if not rows:
                continue
            _acts, ops, _logits = Q.act_plan(gene, variant, classes, T, F)
            assert len(rows) == sum(op[0] == "dwconv" for op in ops)
            sites = {s[0]: k for k, s in enumerate(Q.act_sites(gene, variant, classes, T, F))}
            integer = {r[0] for r in Q.int8_ops(gene, variant, classes, T, F)}
            offs, pos = {}, 0
            for off, ch, ln, cs, es in Q.quant_table(gene, variant, classes):
                offs[off] = (pos, ch, ln, cs, es)
                pos += ch
            for r in rows:
                Cn = r["Cin"]
                assert r["kind"] == Q.INT8_DW_KIND == 2 and r["b_off"] == -1 and r["stride"] == 1 and r["relu"] == 0
                assert Cn == r["Cout"] and Cn % 16 == 0 and 16 <= Cn <= 512 and Cn & (Cn - 1) == 0 and r["KS"] in (3, 5)
                assert r["w_off"] % 16 == 0 and r["scale_off"] % 4 == 0, (gene, variant, r)
                assert sites.get(r["in_act"]) == r["site"], "the input is a site"
                assert sites.get(r["out_act"]) == r["out_site"], "the output is a site"
                readers = [i for i, op in enumerate(ops) if r["out_act"] in (op[1], op[2])]
                assert len(readers) == 1 and readers[0] in integer and ops[readers[0]][0] == "conv", "its only reader runs integer"
                assert offs[r["w_off"]] == (r["scale_off"], Cn, r["KS"] ** 2, 1, Cn), "scale_off and the layout match the quant table"
                assert r["KS"] ** 2 * 127 * 127 <= ACC_MAX < 2 ** 24


def test_int8_ops_keeps_its_rows():
    """The first level's list does not gain the depthwise ops."""
    for variant in (2, 3):
        gene = (16, 3, 1, 2, 2, 1)
        dw = {r["op"] for r in Q.c_int8_dw_ops(gene, variant, 10, T, F)}
        assert dw and not dw & {r["op"] for r in Q.c_int8_ops(gene, variant, 10, T, F)}
        assert all(r["kind"] in (0, 1) for r in Q.c_int8_ops(gene, variant, 10, T, F))


def test_symbols_are_exported_and_the_abi_stays_3():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert name in _lib.INT8_PROTOTYPES, name
    assert L.cmoop_abi_version() == 3, "functions are added only"


def test_int8_dw_ops_refuses_a_small_buffer():
    g = (C.c_int32 * 6)(16, 3, 1, 1, 1, 1)
    rows, n = np.zeros((1, 16), np.int64), C.c_int32()
    assert _lib.lib().cmoop_int8_dw_ops(g, 2, 10, T, F, _lib.ptr(rows), 1, C.byref(n)) != 0
    assert b"too small" in _lib.lib().cmoop_last_error()
    assert _lib.lib().cmoop_int8_dw_ops(g, 0, 10, T, F, None, 0, C.byref(n)) == 0 and n.value == 0, "no depthwise op: nothing to hold"


def test_trained_model_refuses_the_level_without_int8_before_any_session():
    from cmoop_audio_processing_amd.deploy import StreamScorer, TrainedModel
    from cmoop_audio_processing_amd.frontend import FrontendConfig
    gene = (16, 3, 1, 1, 1, 1)
    m = TrainedModel(gene=gene, variant="A_ds", classes=10, T=21, F=12, seed=1, params=np.zeros(G.param_count(gene, 2, 10), np.float32),
                     objectives={})
    with pytest.raises(ValueError, match="int8_depthwise=True needs int8=True"):
        m.session(int8_depthwise=True)
    with pytest.raises(ValueError, match="int8_depthwise=True needs int8=True"):
        m.logits(None, int8_depthwise=True)
    m.frontend = FrontendConfig(n_mels=12)
    with pytest.raises(ValueError, match="int8_depthwise=True needs int8=True"):
        StreamScorer(m, 4, int8_depthwise=True)
    with pytest.raises(ValueError, match="quant_codes"):
        m.session(int8=True, int8_depthwise=True)              # with int8 the model's own lacks are named, as before
    with pytest.raises(ValueError, match="quant_codes"):
        m.int8_report(None, depthwise=True)
