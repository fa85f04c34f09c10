"""Integer inference on the GPU: the lone conv / dense layers EQUAL the numpy statement in bytes (uniform, extreme, one-hot,
narrow and zero-scale operands; guards, halos and stale memory), they agree with the fp32 path on the dequantised operands
within the rounding bound, the activation quantiser's codes, whole nets op by op, off is off, the refusals, TrainedModel /
StreamScorer / int8_report, and the timing entry.  Every test fails without the feature."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 256                                     # bytes of 127 on either side of a code buffer: keeps the 16-byte loads aligned
GUARD = 64                                    # floats of NaN on either side of an output
GUARD_BITS = np.uint32(0x7FC12345)

CONV_SHAPES = [(1, 3, 2, 16, 32, 5, 1),       # the window is larger than the image, K tail: 400
               (3, 5, 3, 16, 32, 3, 1),       # M = 45 ragged, K = 144
               (2, 7, 5, 32, 64, 3, 1),
               (1, 4, 3, 64, 64, 5, 1),
               (1, 4, 3, 512, 512, 5, 1),     # K = 12800
               (2, 13, 5, 256, 512, 1, 2),    # odd H and W -> 7 x 3
               (64, 2, 2, 16, 16, 1, 1),      # the A_ds pointwise: one image per few rows
               (1, 1, 1, 128, 256, 3, 1)]     # all taps but the centre are padding
DENSE_SHAPES = [(1, 32, 10), (5, 32, 11), (17, 64, 35), (64, 512, 512), (65, 128, 64), (257, 256, 16)]


def _torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _codes_dev(q):
    """q int8 (any shape) inside a larger device buffer of 127s -> (buffer, 16-byte aligned view of q's elements)."""
    torch = _torch()
    q = np.ascontiguousarray(q, np.int8).reshape(-1)
    buf = torch.full((q.size + 2 * PAD,), 127, dtype=torch.int8, device="cuda")
    view = buf[PAD:PAD + q.size]
    view.copy_(torch.from_numpy(q))
    return buf, view


def _out_dev(n, fill):
    """n floats between NaN guards, every byte of the n pre-filled with `fill` -> (buffer, view)."""
    torch = _torch()
    raw = np.full(n + 2 * GUARD, GUARD_BITS, np.uint32)
    raw[GUARD:GUARD + n] = np.uint32(fill * 0x01010101)
    buf = torch.from_numpy(raw.view(np.float32).copy()).cuda()
    return buf, buf[GUARD:GUARD + n]


def _read_out(buf, n):
    raw = buf.cpu().numpy().view(np.uint32)
    assert (raw[:GUARD] == GUARD_BITS).all() and (raw[GUARD + n:] == GUARD_BITS).all(), "a guard was written"
    return raw[GUARD:GUARD + n].view(np.float32).copy()


def _weights_asym(N, K):
    """qw[c][k] = ((7 c + 3 k) mod 251) - 125: no two rows, no two columns alike -- locates a permuted k or a swapped index."""
    c, k = np.arange(N)[:, None], np.arange(K)[None, :]
    return (((7 * c + 3 * k) % 251) - 125).astype(np.int8)


def _families(shape_x, N, K, rs):
    """(name, qx, qw, s_x, bits-like qmax) of the operand families; qx in the shape of the activation, qw [N, K]."""
    n = int(np.prod(shape_x))
    extreme = np.full(n, 127, np.int8)
    extreme[0] = 126                     # the sums that take this element are odd: above 2^24 they are no float32 and round
    out = [("uniform", rs.randint(-127, 128, shape_x).astype(np.int8), rs.randint(-127, 128, (N, K)).astype(np.int8)),
           ("extreme", extreme.reshape(shape_x), np.full((N, K), -127, np.int8))]
    for pos in sorted({0, n // 3 + 1 if n > 3 else 0, n - 1}):          # one-hot: a single nonzero activation code
        qx = np.zeros(n, np.int8)
        qx[pos] = 3
        out.append((f"onehot@{pos}", qx.reshape(shape_x), _weights_asym(N, K)))
    for qmax in (1, 7):                                                  # bits 2 and 4
        out.append((f"qmax{qmax}", rs.randint(-qmax, qmax + 1, shape_x).astype(np.int8), rs.randint(-qmax, qmax + 1, (N, K)).astype(np.int8)))
    return out


def _scales(N, rs):
    s_w = (rs.rand(N) * 0.02 + 1e-3).astype(np.float32)
    s_w[N // 2] = 0.0                                                    # an all-zero channel's scale: y = bias there
    bias = rs.randn(N).astype(np.float32)
    return np.float32(0.0137), s_w, bias


def _fp32_check(name, y_int, y_fp, acc_abs, s_x, s_w, bias, n, worst):
    """|y_int - y_fp| <= gamma_(n+5) s_x s_w[c] sum|qx qw| + 2 u |y| per element.  Roundings: the fp32 path rounds each
    dequantised operand (2) and each product (1) and sums n terms (n - 1 additions, in any order): gamma_(n+2) on the sum of
    magnitudes; the integer path rounds the conversion, s_x s_w and their product: gamma_3 on the same sum; gamma_(n+2) +
    gamma_3 <= gamma_(n+5).  Both round the bias add: 2 u |y|."""
    k = n + 5
    gamma = k * U / (1 - k * U)
    t = np.float64(s_x) * s_w.astype(np.float64) * acc_abs.astype(np.float64)
    bound = gamma * t + 2 * U * np.maximum(np.abs(y_int), np.abs(y_fp)).astype(np.float64)
    err = np.abs(y_int.astype(np.float64) - y_fp.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    worst[0] = max(worst[0], float(q.max()))
    assert (err <= bound).all(), (name, float(q.max()))


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv_layer_equals_the_statement_in_bytes_and_the_fp32_path_within_the_bound(shape):
    torch = _torch()
    from cmoop_audio_processing_amd import _lib, quant as Q
    B, H, W, Cin, Cout, KS, stride = shape
    K = KS * KS * Cin
    OH, OW = -(-H // stride), -(-W // stride)
    n_out = B * OH * OW * Cout
    rs = np.random.RandomState(sum(shape))
    s_x, s_w, bias = _scales(Cout, rs)
    d_sw, d_bias = torch.from_numpy(s_w).cuda(), torch.from_numpy(bias).cuda()
    worst = [0.0]
    for name, qx, qw in _families((B, H, W, Cin), Cout, K, rs):
        acc = Q.conv_i8_acc(qx, qw, KS, stride)
        if name == "extreme" and K == 12800:
            assert (acc.astype(np.int32).astype(np.float32).astype(np.int64) != acc).any(), "no accumulator rounds in the conversion"
        xbuf, xv = _codes_dev(qx)
        wbuf, wv = _codes_dev(qw)
        xd = torch.from_numpy((qx.astype(np.float32) * s_x).astype(np.float32)).cuda()
        wd = torch.from_numpy((qw.astype(np.float32) * s_w[:, None]).astype(np.float32)).cuda()
        acc_abs = Q.conv_i8_acc(np.abs(qx), np.abs(qw), KS, stride).reshape(-1, Cout)
        for relu in (0, 1):
            want = Q.i8_epilogue_ref(acc, s_x, s_w, bias, relu).reshape(-1)
            got = []
            for fill in (0x00, 0xFF):
                ybuf, yv = _out_dev(n_out, fill)
                Q.conv_fwd_i8(xv, wv, s_x, d_sw, d_bias, yv, B, H, W, Cin, Cout, KS, stride, relu)
                got.append(_read_out(ybuf, n_out))
            assert np.array_equal(_bits(got[0]), _bits(got[1])), (name, relu, "the result depends on what the output held")
            assert np.array_equal(_bits(got[0]), _bits(want)), (name, relu, int((_bits(got[0]) != _bits(want)).sum()))
            # every family: the fp32 path on the dequantised operands
            yf = torch.zeros(n_out, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            _lib.check(_lib.lib().cmoop_conv_fwd_trainer(
                C.c_void_p(xd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(d_bias.data_ptr()), C.c_void_p(yf.data_ptr()),
                *(C.c_int32(v) for v in (B, H, W, Cin, Cout, KS, stride, relu)), None, None, None))
            _fp32_check(name, got[0].reshape(-1, Cout), yf.cpu().numpy().reshape(-1, Cout), acc_abs, s_x, s_w, bias, K, worst)
    print(f"    conv {shape}: worst |int8 - fp32| / bound {worst[0]:.3f}")


@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_dense_layer_equals_the_statement_in_bytes_and_the_fp32_path_within_the_bound(shape):
    torch = _torch()
    from cmoop_audio_processing_amd import _lib, quant as Q
    M, K, N = shape
    rs = np.random.RandomState(sum(shape))
    s_x, s_w, bias = _scales(N, rs)
    d_sw, d_bias = torch.from_numpy(s_w).cuda(), torch.from_numpy(bias).cuda()
    worst = [0.0]
    for name, qx, qw in _families((M, K), N, K, rs):
        acc = qx.astype(np.int64).dot(qw.astype(np.int64).T)
        xbuf, xv = _codes_dev(qx)
        wbuf, wv = _codes_dev(qw)
        xd = torch.from_numpy((qx.astype(np.float32) * s_x).astype(np.float32)).cuda()
        wd = torch.from_numpy((qw.astype(np.float32) * s_w[:, None]).astype(np.float32)).cuda()
        acc_abs = np.abs(qx).astype(np.int64).dot(np.abs(qw).astype(np.int64).T)
        for relu in (0, 1):
            want = Q.dense_i8_ref(qx, qw, s_x, s_w, bias, relu).reshape(-1)
            got = []
            for fill in (0x00, 0xFF):
                ybuf, yv = _out_dev(M * N, fill)
                Q.dense_fwd_i8(xv, wv, s_x, d_sw, d_bias, yv, M, N, K, relu)
                got.append(_read_out(ybuf, M * N))
            assert np.array_equal(_bits(got[0]), _bits(got[1])), (name, relu, "the result depends on what the output held")
            assert np.array_equal(_bits(got[0]), _bits(want)), (name, relu, int((_bits(got[0]) != _bits(want)).sum()))
            # every family: the fp32 path on the dequantised operands
            yf = torch.zeros(M * N, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            _lib.check(_lib.lib().cmoop_dense_fwd(C.c_void_p(xd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(d_bias.data_ptr()),
                                                  C.c_void_p(yf.data_ptr()), *(C.c_int32(v) for v in (M, N, K, relu))))
            _fp32_check(name, got[0].reshape(M, N), yf.cpu().numpy().reshape(M, N), acc_abs, s_x, s_w, bias, K, worst)
    print(f"    dense {shape}: worst |int8 - fp32| / bound {worst[0]:.3f}")


def test_empty_batch_writes_nothing_and_bad_shapes_are_refused():
    torch = _torch()
    from cmoop_audio_processing_amd import _lib, quant as Q
    xbuf, xv = _codes_dev(np.zeros(64, np.int8))
    wbuf, wv = _codes_dev(np.zeros(16 * 32, np.int8))
    sw, b = torch.ones(16, device="cuda"), torch.zeros(16, device="cuda")
    ybuf, yv = _out_dev(32, 0xFF)
    Q.dense_fwd_i8(xv, wv, 1.0, sw, b, yv, 0, 16, 32, 0)
    Q.conv_fwd_i8(xv, wv, 1.0, sw, b, yv, 0, 1, 1, 32, 16, 1, 1, 0)
    assert (_bits(_read_out(ybuf, 32)) == 0xFFFFFFFF).all()
    for call, what in ((lambda: Q.conv_fwd_i8(xv, wv, 1.0, sw, b, yv, 1, 1, 1, 24, 16, 1, 1, 0), "multiple of 16"),
                       (lambda: Q.conv_fwd_i8(xv, wv, 1.0, sw, b, yv, 1, 1, 1, 32, 16, 3, 2, 0), "stride"),
                       (lambda: Q.conv_fwd_i8(xv, wv, 1.0, sw, b, yv, 1, 1, 1, 32, 16, 7, 1, 0), "KS"),
                       (lambda: Q.dense_fwd_i8(xv, wv, 1.0, sw, b, yv, 1, 16, 40, 0), "multiple of 16"),
                       (lambda: Q.dense_fwd_i8(xbuf[PAD + 1:], wv, 1.0, sw, b, yv, 1, 16, 32, 0), "aligned")):
        with pytest.raises(_lib.CmoopError, match=what):
            call()
    assert (_bits(_read_out(ybuf, 32)) == 0xFFFFFFFF).all()


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 4 * 1024 * 1024 + 3])
def test_activation_codes_next_to_the_fp32_tensor(n):
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    rs = np.random.RandomState(n % 997)
    x = (rs.randn(n) * 3).astype(np.float32)
    x[::11] = -0.0
    # (bits, float offset of x, byte offset of the codes): packed 4-byte code stores, and the byte path off a 4-byte boundary
    for bits, offset, coff in ((8, 0, 0), (8, 1, 0), (4, 0, 2), (2, 3, 1)) if n < 2 ** 20 else ((8, 0, 0), (4, 1, 0)):
        a = np.float32(np.abs(x).max() / 2)                  # below the absmax: the clamp works
        _a, y = Q.fake_quant_act_ref(x, bits, a)
        q = Q.act_codes_ref(x, bits, a)
        buf = torch.full((n + 16,), 777.0, dtype=torch.float32, device="cuda")
        view = buf[4 + offset: 4 + offset + n]
        cbuf = torch.full((n + 32,), 99, dtype=torch.int8, device="cuda")
        cview = cbuf[16 + coff: 16 + coff + n]
        view.copy_(torch.from_numpy(x))
        Q.fake_quant_act_codes(view, bits, a, cview)
        out, codes = buf.cpu().numpy(), cbuf.cpu().numpy()
        assert np.array_equal(_bits(out[4 + offset: 4 + offset + n]), _bits(y)), (n, bits, offset)
        assert np.array_equal(codes[16 + coff: 16 + coff + n], q), (n, bits, offset, coff)
        assert (out[:4 + offset] == 777.0).all() and (out[4 + offset + n:] == 777.0).all()
        assert (codes[:16 + coff] == 99).all() and (codes[16 + coff + n:] == 99).all()
        # a null codes pointer: today's launch and bytes
        view.copy_(torch.from_numpy(x))
        Q.fake_quant_act_codes(view, bits, a, None)
        plain = buf.cpu().numpy()
        view.copy_(torch.from_numpy(x))
        Q.fake_quant_act(view, bits, a=a)
        assert plain.tobytes() == buf.cpu().numpy().tobytes() == out.tobytes()


# ---- nets ---------------------------------------------------------------------------------------------------------------------
T, F, CLASSES = 21, 12, 10
NETS = [("A", (16, 3, 1, 1, 1, 1)), ("B", (16, 3, 1, 1, 1, 1)), ("A", (32, 5, 0, 2, 3, 1)), ("B", (32, 5, 0, 2, 3, 1)),
        ("A_ds", (16, 3, 1, 1, 2, 0)), ("B_ds", (16, 3, 1, 1, 2, 0))]


def _data(n=8, seed=0):
    torch = _torch()
    rs = np.random.RandomState(seed)
    X = torch.from_numpy(rs.randn(n, T, F).astype(np.float32)).cuda()
    y = torch.from_numpy(rs.randint(0, CLASSES, n).astype(np.int32)).cuda()
    return X, y


def _cfg(variant, quant=True, act=True, **kw):
    from cmoop_audio_processing_amd import EvalConfig, quant as Q
    return EvalConfig(variant=variant, classes=CLASSES, batch=3, eval_batch=5, n_slots=1,
                      quant=Q.QuantConfig(bits=8) if quant else None,
                      act_quant=Q.ActQuantConfig(bits=8, momentum=0.9) if act else None, **kw)


def _ready_net(gene, variant, seed=3):
    from cmoop_audio_processing_amd.session import NetSession
    X, y = _data()
    net = NetSession(gene, _cfg(variant), T, F, seed)
    net.train_step(X, y, None, 0, 3)
    net.train_step(X, y, None, 3, 3)
    return net, X, y


def _acts(net, B):
    n = net.act_dims(0)[5]
    return {i: net.get_act(i, B) for i in range(1, n) if net.act_dims(i)[3]}


@pytest.mark.parametrize("variant, gene", NETS)
def test_every_integer_op_of_a_net_equals_the_statement_on_the_devices_own_operands(variant, gene):
    from cmoop_audio_processing_amd import quant as Q
    net, X, _y = _ready_net(gene, variant)
    with net:
        sites = {s[0]: k for k, s in enumerate(Q.act_sites(gene, variant, CLASSES, T, F))}
        off_logits = net.predict_logits(X).cpu().numpy()       # 8 rows: a full chunk of 5 and a partial one of 3
        off = _acts(net, 3)
        net.set_int8(True)
        assert net.int8
        on_logits = net.predict_logits(X).cpu().numpy()
        on = _acts(net, 3)
        ops = net.int8_ops()
        assert [(r["op"], r["in_act"], r["out_act"]) for r in ops] == Q.int8_ops(gene, variant, CLASSES, T, F) and ops
        _wq, codes, scales = net.get_quantized()
        params, rec = net.get_params(), net.get_act_ranges()
        first = min(r["out_act"] for r in ops)
        for i in off:
            if i < first:
                assert off[i].tobytes() == on[i].tobytes(), ("an act before the first integer op changed", i)
        for r in ops:
            r_in = rec["r"][sites[r["in_act"]]]
            qx = Q.act_codes_ref(on[r["in_act"]], 8, r_in)
            s_x = Q.act_scale_ref(r_in, 8)
            assert np.array_equal(_bits((qx.astype(np.float32) * s_x).astype(np.float32)), _bits(on[r["in_act"]])), "the site is off its grid"
            K = r["KS"] * r["KS"] * r["Cin"]
            qw = codes[r["w_off"]: r["w_off"] + r["Cout"] * K].reshape(r["Cout"], K)
            s_w = scales[r["scale_off"]: r["scale_off"] + r["Cout"]]
            bias = params[r["b_off"]: r["b_off"] + r["Cout"]]
            if r["kind"] == 0:
                want = Q.conv_i8_ref(qx, qw, s_x, s_w, bias, r["KS"], r["stride"], r["relu"])
            else:
                want = Q.dense_i8_ref(qx.reshape(3, -1), qw, s_x, s_w, bias, r["relu"])
            if r["out_act"] in sites:                          # the output is a site itself: quantised in place right after
                want = Q.fake_quant_act_ref(want, 8, rec["r"][sites[r["out_act"]]])[1]
            assert np.array_equal(_bits(want).reshape(-1), _bits(on[r["out_act"]]).reshape(-1)), (variant, gene, r)
        assert np.isfinite(on_logits).all() and on_logits.shape == off_logits.shape
        # enabled then disabled: today's path, in bytes
        net.set_int8(False)
        assert net.predict_logits(X).cpu().numpy().tobytes() == off_logits.tobytes()


def test_off_is_off_for_inference_and_for_a_train_step():
    gene, variant = (16, 3, 1, 1, 1, 1), "A"
    plain, X, y = _ready_net(gene, variant)
    mode, _X, _y = _ready_net(gene, variant)
    with plain, mode:
        want_p, want_z = plain.predict_proba(X).cpu().numpy(), plain.predict_logits(X).cpu().numpy()
        mode.set_int8(True)
        mode.predict_proba(X)
        mode.set_int8(False)
        assert mode.predict_proba(X).cpu().numpy().tobytes() == want_p.tobytes()
        assert mode.predict_logits(X).cpu().numpy().tobytes() == want_z.tobytes()
        mode.set_int8(True)                                     # a train step under the mode is the plain train step
        for net in (plain, mode):
            net.train_step(X, y, None, 2, 3)
        assert mode.get_grads().tobytes() == plain.get_grads().tobytes()
        assert mode.get_params().tobytes() == plain.get_params().tobytes()
        assert mode.get_act_ranges().tobytes() == plain.get_act_ranges().tobytes()
        assert mode.int8


def test_refusals_leave_the_net_working():
    from cmoop_audio_processing_amd import _lib, quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    gene, variant = (16, 3, 1, 1, 1, 1), "A"
    X, y = _data()
    for kw, what in ((dict(quant=False), "set_quant"), (dict(act=False), "set_actquant")):
        with NetSession(gene, _cfg(variant, **kw), T, F, 3) as net:
            net.train_step(X, y, None, 0, 3)
            with pytest.raises(_lib.CmoopError, match=what):
                net.set_int8(True)
            assert not net.int8 and np.isfinite(net.predict_logits(X).cpu().numpy()).all()
    with NetSession(gene, _cfg(variant), T, F, 3) as net:
        with pytest.raises(_lib.CmoopError, match="tracked ranges"):
            net.set_int8(True)                                  # no train step yet: no ranges
        net.train_step(X, y, None, 0, 3)
        want = net.predict_logits(X).cpu().numpy()
        rec = net.get_act_ranges()
        bad = rec.copy()
        bad["r"][1] = np.nan
        net.set_act_ranges(bad)
        with pytest.raises(_lib.CmoopError, match="not finite"):
            net.set_int8(True)
        assert not net.int8
        net.set_act_ranges(rec)
        assert net.predict_logits(X).cpu().numpy().tobytes() == want.tobytes()
        net.set_int8(True)                                      # and now it is accepted
        on = net.predict_logits(X).cpu().numpy()
        assert np.isfinite(on).all()
        with pytest.raises(_lib.CmoopError, match="not finite"):
            net.set_act_ranges(bad)                             # while the mode is on a non-finite range is not loaded
        assert net.get_act_ranges().tobytes() == rec.tobytes() and net.predict_logits(X).cpu().numpy().tobytes() == on.tobytes()
        net.set_quant(None)                                     # the weight codes go: the mode goes with them
        assert not net.int8 and np.isfinite(net.predict_logits(X).cpu().numpy()).all()


def test_trained_model_stream_scorer_and_report(tmp_path):
    torch = _torch()
    from cmoop_audio_processing_amd import PopulationEvaluator, quant as Q
    from cmoop_audio_processing_amd.deploy import StreamScorer, TrainedModel
    from cmoop_audio_processing_amd.frontend import FrontendConfig
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = "A", (16, 3, 1, 1, 1, 1)
    rs = np.random.RandomState(9)
    yy = rs.randint(0, CLASSES, 96).astype(np.int32)
    XX = (rs.randn(96, T, F) + yy[:, None, None] * 0.3).astype(np.float32)
    X, y = torch.from_numpy(XX).cuda(), torch.from_numpy(yy).cuda()
    cfg = _cfg(variant, epochs=2, early_stop=False, lr=1e-2, seed=2)
    model = PopulationEvaluator(X[:72], y[:72], X[72:], y[72:], cfg).train_model(gene, 2)
    assert model.quant_codes is not None and model.act_ranges is not None
    model.save(tmp_path / "m.npz")
    back = TrainedModel.load(tmp_path / "m.npz")
    # the live net: the model's arena under the same options, integer inference on
    with NetSession(gene, cfg, T, F, 2) as net:
        net.set_params(model.params)
        net.set_act_ranges(model.act_ranges)
        net.set_int8(True)
        want = net.predict_logits(X[72:]).cpu().numpy()
        _wq, codes, scales = net.get_quantized()
    assert codes.tobytes() == model.quant_codes.tobytes() and scales.tobytes() == model.quant_scales.tobytes(), \
        "quantising the dequantised arena gives the model's own codes and scales back"
    plain_cfg = _cfg(variant, quant=False, act=False)            # a config without the options: the model turns them on
    with back.session(plain_cfg, int8=True) as s:
        assert s.int8
        got = s.predict_logits(X[72:]).cpu().numpy()
        feat = X[72:80].reshape(-1, F).contiguous()
        stream_want = s.predict_stream(feat, 7).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert back.logits(X[72:], plain_cfg, int8=True).cpu().numpy().tobytes() == want.tobytes()
    back.frontend = FrontendConfig(n_mels=F)
    with StreamScorer(back, 7, plain_cfg, int8=True) as sc:
        assert sc.net.int8
        assert sc.net.predict_stream(feat, 7).cpu().numpy().tobytes() == stream_want.tobytes()
    rep = back.int8_report(X[72:], y[72:], plain_cfg)
    assert set(rep) == {"rows", "argmax_agree", "max_abs_logit_diff", "int8_ops", "acc_fakequant", "acc_int8"}
    assert rep["rows"] == 24 and 0.0 <= rep["argmax_agree"] <= 1.0 and np.isfinite(rep["max_abs_logit_diff"]) and rep["int8_ops"] > 0
    assert set(back.int8_report(X[72:], config=plain_cfg)) == {"rows", "argmax_agree", "max_abs_logit_diff", "int8_ops"}
    print(f"    int8_report: {rep}")


def test_the_timing_entry_runs():
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    B, H, W, Cin, Cout, KS = 4, 13, 5, 64, 64, 3
    rs = np.random.RandomState(1)
    xbuf, xv = _codes_dev(rs.randint(-127, 128, B * H * W * Cin).astype(np.int8))
    wbuf, wv = _codes_dev(rs.randint(-127, 128, Cout * KS * KS * Cin).astype(np.int8))
    sw, b = torch.ones(Cout, device="cuda"), torch.zeros(Cout, device="cuda")
    y = torch.empty(B * H * W * Cout, dtype=torch.float32, device="cuda")
    ms = Q.conv_fwd_i8_time(xv, wv, 0.01, sw, b, y, B, H, W, Cin, Cout, KS, 1, 1, iters=5)
    assert np.isfinite(ms) and ms > 0
