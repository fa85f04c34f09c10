"""Integer inference, the host side: the numpy statements against a plain loop nest, the plan (which ops run integer, their
alignment and accumulator bound over the whole search space), the exported symbols and the TrainedModel refusals.  No GPU."""
import ctypes as C

import numpy as np
import pytest

from cmoop_audio_processing_amd import _lib, genes as G, quant as Q

NEW_SYMBOLS = ["cmoop_conv_fwd_i8", "cmoop_dense_fwd_i8", "cmoop_conv_fwd_i8_time", "cmoop_fake_quant_act_codes", "cmoop_int8_ops",
               "cmoop_net_set_int8", "cmoop_net_int8_ops"]
T, F = 101, 40


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _loop_conv(qx, qw, s_x, s_w, bias, KS, stride, relu):
    """A plain int64 loop nest, TF SAME padding, then the float32 epilogue one operation at a time."""
    f = np.float32
    B, H, W, Cin = qx.shape
    Cout = qw.shape[0]
    OH, OW = -(-H // stride), -(-W // stride)
    pt = max((OH - 1) * stride + KS - H, 0) // 2
    pl = max((OW - 1) * stride + KS - W, 0) // 2
    y = np.zeros((B, OH, OW, Cout), f)
    for b in range(B):
        for oh in range(OH):
            for ow in range(OW):
                for c in range(Cout):
                    acc = 0
                    for kh in range(KS):
                        for kw in range(KS):
                            ih, iw = oh * stride - pt + kh, ow * stride - pl + kw
                            if 0 <= ih < H and 0 <= iw < W:
                                for ci in range(Cin):
                                    acc += int(qx[b, ih, iw, ci]) * int(qw[c, kh, kw, ci])
                    v = f(f(f(np.int32(acc)) * f(f(s_x) * f(s_w[c]))) + f(bias[c]))
                    if relu:
                        v = v if v > 0 else f(0)
                    y[b, oh, ow, c] = v
    return y


@pytest.mark.parametrize("shape", [(1, 3, 2, 4, 3, 5, 1),      # the window is larger than the image
                                   (2, 5, 3, 3, 4, 1, 2),      # stride 2, odd H and W
                                   (1, 4, 5, 2, 3, 3, 1)])
@pytest.mark.parametrize("relu", [0, 1])
def test_conv_ref_equals_a_plain_loop_nest(shape, relu):
    B, H, W, Cin, Cout, KS, stride = shape
    rs = np.random.RandomState(sum(shape))
    qx = rs.randint(-127, 128, (B, H, W, Cin)).astype(np.int8)
    qw = rs.randint(-127, 128, (Cout, KS, KS, Cin)).astype(np.int8)
    s_w = (rs.rand(Cout) * 0.01).astype(np.float32)
    s_w[0] = 0
    bias = rs.randn(Cout).astype(np.float32)
    got = Q.conv_i8_ref(qx, qw, 0.031, s_w, bias, KS, stride, relu)
    want = _loop_conv(qx, qw, np.float32(0.031), s_w, bias, KS, stride, relu)
    assert got.shape == want.shape and np.array_equal(_bits(got), _bits(want))
    # the dense statement is the 1x1 conv of a 1x1 image
    d = Q.dense_i8_ref(qx.reshape(-1, Cin), qw[:, 0, 0], 0.031, s_w, bias, relu)
    want_d = Q.conv_i8_ref(qx.reshape(-1, 1, 1, Cin), qw[:, :1, :1], 0.031, s_w, bias, 1, 1, relu)
    assert np.array_equal(_bits(d), _bits(want_d.reshape(d.shape)))


def test_epilogue_rounds_the_conversion_and_relu_gives_plus_zero():
    # 127 * 127 * 12800 > 2^24: the int32 -> float32 conversion rounds to nearest even
    qx, qw = np.full((1, 12800), 127, np.int8), np.full((2, 12800), -127, np.int8)
    qw[1] = 127
    qx[0, 0] = 126                                           # an odd sum: not a float32
    one = np.ones(2, np.float32)
    y = Q.dense_i8_ref(qx, qw, 1.0, one, np.zeros(2, np.float32), 0)
    acc = 127 * 127 * 12799 + 126 * 127
    assert acc > 2 ** 24 and int(np.float32(acc)) != acc and y[0, 1] == np.float32(acc) and y[0, 0] == -np.float32(acc)
    z = Q.dense_i8_ref(qx, qw, 1.0, one, np.zeros(2, np.float32), 1)
    assert _bits(z[0, :1])[0] == 0, "a clipped value is +0.0"
    z = Q.dense_i8_ref(qx, qw, 1.0, np.zeros(2, np.float32), np.asarray([-0.0, 2.5], np.float32), 1)
    assert _bits(z[0, :1])[0] == 0 and z[0, 1] == 2.5, "scale 0: y = bias; ReLU of -0.0 is +0.0"


@pytest.mark.parametrize("bits", [2, 4, 8])
def test_act_codes_times_scale_is_the_fake_quantised_tensor(bits):
    rs = np.random.RandomState(bits)
    x = (rs.randn(3, 7, 5) * 2).astype(np.float32)
    x.flat[::7] = -0.0
    x.flat[3] = np.inf
    x.flat[5] = np.nan
    for a in (0.0, 1e-42, 0.7, 3.0, float(np.abs(x[np.isfinite(x)]).max())):
        q = Q.act_codes_ref(x, bits, a)
        s = Q.act_scale_ref(a, bits)
        _a, y = Q.fake_quant_act_ref(x, bits, a)
        assert q.dtype == np.int8 and q.shape == x.shape and int(np.abs(q.astype(np.int32)).max()) <= Q.qmax_of(bits)
        assert np.array_equal(_bits((q.astype(np.float32) * s).astype(np.float32)), _bits(y)), (bits, a)


@pytest.mark.parametrize("variant", [0, 1, 2, 3])
def test_int8_ops_c_equals_python_and_every_op_fits_the_kernels(variant):
    for classes in (10, 35):
        for gene in G.all_genes():
            rows = Q.c_int8_ops(gene, variant, classes, T, F)
            want = Q.int8_ops(gene, variant, classes, T, F)
            assert [(r["op"], r["in_act"], r["out_act"]) for r in rows] == want, (gene, variant)
            assert rows, "every candidate has integer ops (its dense head at least)"
            table = Q.quant_table(gene, variant, classes)
            assert all(off % 16 == 0 for off, *_ in table), ("a kernel tensor starts off a 16-element boundary", gene, variant)
            offs, pos = {}, 0
            for off, ch, _ln, _cs, _es in table:
                offs[off] = (pos, ch)
                pos += ch
            for r in rows:
                assert r["Cin"] % 16 == 0 and r["w_off"] % 16 == 0, (gene, variant, r)
                assert r["kind"] in (0, 1) and r["KS"] in (1, 3, 5) and (r["stride"] == 1 or (r["stride"] == 2 and r["KS"] == 1))
                assert 127 * 127 * r["KS"] * r["KS"] * r["Cin"] < 2 ** 31, "the accumulator bound"
                assert offs[r["w_off"]] == (r["scale_off"], r["Cout"]), "scale_off is the tensor's first scale in the quant table"
                assert r["b_off"] == r["w_off"] + r["Cout"] * r["KS"] * r["KS"] * r["Cin"]


def test_the_largest_reduction_of_the_search_space_is_12800():
    kmax = max(r["KS"] * r["KS"] * r["Cin"] for v in range(4) for g in G.all_genes() for r in Q.c_int8_ops(g, v, 10, T, F))
    assert kmax == 12800 and 127 * 127 * kmax < 2 ** 31


def test_first_conv_depthwise_and_gap_never_run_integer():
    for variant in ("A", "B", "A_ds", "B_ds"):
        gene = (16, 3, 1, 2, 2, 1)
        _acts, ops, _l = Q.act_plan(gene, variant, 10, T, F)
        picked = {r[0] for r in Q.int8_ops(gene, variant, 10, T, F)}
        for i, op in enumerate(ops):
            if op[0] in ("conv1", "dwconv", "gap", "bn", "pool", "addrelu"):
                assert i not in picked
            elif op[0] == "dense":
                assert i in picked
        assert any(ops[i][0] == "conv" for i in picked)


def test_symbols_are_exported_and_the_abi_stays_3():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared and hasattr(L, name), name
        assert name in _lib.INT8_PROTOTYPES, name
    assert L.cmoop_abi_version() == 3, "functions are added only"


def test_int8_ops_refuses_a_small_buffer():
    g = (C.c_int32 * 6)(16, 3, 1, 1, 1, 1)
    rows, n = np.zeros((1, 16), np.int64), C.c_int32()
    assert _lib.lib().cmoop_int8_ops(g, 0, 10, T, F, _lib.ptr(rows), 1, C.byref(n)) != 0
    assert b"too small" in _lib.lib().cmoop_last_error()


def _plain_model(**kw):
    from cmoop_audio_processing_amd.deploy import TrainedModel
    gene = (16, 3, 1, 1, 1, 1)
    n = G.param_count(gene, 0, 10)
    return TrainedModel(gene=gene, variant="A", classes=10, T=21, F=12, seed=1, params=np.zeros(n, np.float32), objectives={}, **kw)


def test_trained_model_refuses_int8_without_codes_and_ranges_before_any_session():
    from cmoop_audio_processing_amd.deploy import StreamScorer
    from cmoop_audio_processing_amd.frontend import FrontendConfig
    m = _plain_model()
    with pytest.raises(ValueError, match="quant_codes.*act_ranges"):
        m.session(int8=True)
    with pytest.raises(ValueError, match="quant_codes"):
        m.logits(None, int8=True)
    with pytest.raises(ValueError, match="quant_codes"):
        m.int8_report(None)
    m.frontend = FrontendConfig(n_mels=12)
    with pytest.raises(ValueError, match="quant_codes"):
        StreamScorer(m, 4, int8=True)
    # codes alone: the ranges are still named
    n = m.params.size
    rows = Q.quant_table(m.gene, 0, 10)
    q = _plain_model(quant_bits=8, quant_codes=np.zeros(n, np.int8), quant_scales=np.zeros(sum(r[1] for r in rows), np.float32))
    with pytest.raises(ValueError) as e:
        q.session(int8=True)
    assert "act_ranges" in str(e.value) and "quant_codes" not in str(e.value)
