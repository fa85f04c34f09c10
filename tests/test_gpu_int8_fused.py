"""The requantising epilogue on the GPU.  Every comparison is EQUALITY OF BYTES with no excused element: the lone fused conv /
dense launch against the numpy statement (quant.conv_i8_q_ref / dense_i8_q_ref) and against the device's own un-fused chain
(cmoop_conv_fwd_i8 / cmoop_dense_fwd_i8 -> cmoop_bn_eval_fwd -> cmoop_fake_quant_act_codes) into sentinel-filled outputs between
guards; refusals and the empty batch; whole nets act by act against the pass without the level and every fused op against the
statement on the device's own operands; the level's contract; the Python surface; the timing entries.  Every test fails
without the feature."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAD = 256                                     # bytes of 127 on either side of a code buffer: keeps the 16-byte loads aligned
GUARD = 64                                    # floats of NaN on either side of an fp32 output
GUARD_BITS = np.uint32(0x7FC12345)
CODE_GUARD = 99
SENTINEL_CODE = 0x55

# (B, H, W, Cin, Cout, KS): a wave is 32 rows x 64 / 32 / 16 channels, a workgroup 128 rows, a K step 64
CONV_SHAPES = [(1, 1, 1, 16, 16, 1),          # K = 16, a quarter step, one row
               (2, 5, 3, 16, 32, 3),          # K = 144, zero tail fragments, W < KS
               (3, 7, 6, 32, 64, 5),          # M = 126, one row group short of a workgroup
               (2, 9, 8, 16, 16, 5),          # M = 144, a partial second workgroup; one step spans four taps
               (1, 13, 5, 64, 128, 3)]        # two 64-channel column blocks
DENSE_SHAPES = [(1, 64, 32),                  # K = 32, half a step
                (37, 128, 64),
                (130, 256, 512)]
# (relu, BatchNorm, relu_after)
TAILS = [(1, False, 0), (0, True, 1), (1, True, 0), (0, False, 0)]


def _torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _codes_dev(q):
    torch = _torch()
    q = np.ascontiguousarray(q, np.int8).reshape(-1)
    buf = torch.full((q.size + 2 * PAD,), 127, dtype=torch.int8, device="cuda")
    view = buf[PAD:PAD + q.size]
    view.copy_(torch.from_numpy(q))
    return buf, view


def _out_dev(n, fill=0xFF):
    torch = _torch()
    raw = np.full(n + 2 * GUARD, GUARD_BITS, np.uint32)
    raw[GUARD:GUARD + n] = np.uint32(fill * 0x01010101)
    buf = torch.from_numpy(raw.view(np.float32).copy()).cuda()
    return buf, buf[GUARD:GUARD + n]


def _read_out(buf, n):
    raw = buf.cpu().numpy().view(np.uint32)
    assert (raw[:GUARD] == GUARD_BITS).all() and (raw[GUARD + n:] == GUARD_BITS).all(), "a guard was written"
    return raw[GUARD:GUARD + n].view(np.float32).copy()


def _codes_out_dev(n):
    torch = _torch()
    buf = torch.full((n + 2 * PAD,), CODE_GUARD, dtype=torch.int8, device="cuda")
    buf[PAD:PAD + n] = SENTINEL_CODE
    return buf, buf[PAD:PAD + n]


def _read_codes(buf, n):
    raw = buf.cpu().numpy()
    assert (raw[:PAD] == CODE_GUARD).all() and (raw[PAD + n:] == CODE_GUARD).all(), "a code guard was written"
    return raw[PAD:PAD + n].copy()


def _dev(a):
    return _torch().from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def _weights_asym(N, K):
    """qw[n][k] = ((7 n + 11 k) mod 251) - 125: different for every channel at a fixed k -- with a one-hot activation row the
    output codes name their channel, which confirms the lane-to-channel map of the code word."""
    n, k = np.arange(N)[:, None], np.arange(K)[None, :]
    return (((7 * n + 11 * k) % 251) - 125).astype(np.int8)


def _families(x_shape, N, K, rs):
    """(name, qx, qw [N, K], out_bits, which ranges: 'all' or 'clamp' or 'both')."""
    n = int(np.prod(x_shape))
    out = [("uniform", rs.randint(-127, 128, x_shape).astype(np.int8), rs.randint(-127, 128, (N, K)).astype(np.int8), 8, "all"),
           ("extreme+", np.full(x_shape, 127, np.int8), np.full((N, K), 127, np.int8), 8, "clamp"),
           ("extreme-", np.full(x_shape, -127, np.int8), np.full((N, K), 127, np.int8), 8, "clamp")]
    for pos in sorted({0, n - 1}):
        qx = np.zeros(n, np.int8)
        qx[pos] = 3
        out.append((f"onehot@{pos}", qx.reshape(x_shape), _weights_asym(N, K), 8, "both"))
    for bits in (2, 4):                       # weight, activation AND output bits 2 and 4
        qmax = (1 << (bits - 1)) - 1
        out.append((f"bits{bits}", rs.randint(-qmax, qmax + 1, x_shape).astype(np.int8), rs.randint(-qmax, qmax + 1, (N, K)).astype(np.int8),
                    bits, "all"))
    return out


def _bn_eval(y1, gamma, beta, mm, mv, eps, relu_after, M, Cn):
    """cmoop_bn_eval_fwd on device tensors -> (y, scale, shift) device tensors."""
    torch = _torch()
    from cmoop_audio_processing_amd import _lib
    y2 = torch.empty(max(M * Cn, 1), dtype=torch.float32, device="cuda")
    scale, shift = torch.empty(Cn, dtype=torch.float32, device="cuda"), torch.empty(Cn, dtype=torch.float32, device="cuda")
    P = lambda t: C.c_void_p(t.data_ptr())
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_bn_eval_fwd(P(y1), P(gamma), P(beta), P(mm), P(mv), P(y2), P(scale), P(shift), C.c_int64(M), C.c_int32(Cn),
                                            C.c_double(eps), C.c_int32(relu_after)))
    return y2, scale, shift


def _bn_vectors(kind, Cn, t_plain, rs):
    """BatchNorm parameters (gamma, beta, moving mean, moving variance, eps).  'trained': random ones.  'hand': eps 0, variance
    1 and mean 0 make scale = gamma and shift = beta exactly; scale has negative, zero and large channels, and shift cancels
    t * scale of one output row to within a few ulp -- the family on which a fused multiply-add and two roundings part."""
    f = np.float32
    if kind == "trained":
        return ((rs.rand(Cn) + 0.5).astype(f), rs.randn(Cn).astype(f), rs.randn(Cn).astype(f), (rs.rand(Cn) + 0.1).astype(f), 1e-3)
    scale = (rs.randn(Cn) * 3).astype(f)
    scale[0::8] = 0.0
    scale[1::8] = -np.abs(scale[1::8]) - 1
    scale[2::8] = f(3.0e4) + scale[2::8]
    row = t_plain.reshape(-1, Cn)[rs.randint(t_plain.size // Cn)]
    with np.errstate(all="ignore"):
        shift = (-(row * scale)).astype(f)
    shift = (shift.view(np.uint32) + rs.randint(-2, 3, Cn).astype(np.int64)).astype(np.uint32).view(f)
    shift[~np.isfinite(shift)] = 0.5
    shift[shift == 0] = 0.0                    # +0: beta - 0 * scale keeps every other value's bytes
    return scale, shift, np.zeros(Cn, f), np.ones(Cn, f), 0.0


def _check_layer(conv, shape):
    """Every family x tail x BatchNorm family x range of one shape: the fused launch against the chain and the statement."""
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    f = np.float32
    if conv:
        B, H, W, Cin, N, KS = shape
        x_shape, K, M = (B, H, W, Cin), KS * KS * Cin, B * H * W
    else:
        M, N, K = shape
        x_shape = (M, K)
    n = M * N
    rs = np.random.RandomState(sum(shape))
    s_x = f(0.0137)
    s_w, bias = (rs.rand(N) * 0.02 + 1e-3).astype(f), rs.randn(N).astype(f)
    d_sw, d_bias = _dev(s_w), _dev(bias)
    checked = parted = 0
    for name, qx, qw, bits, which in _families(x_shape, N, K, rs):
        xbuf, xv = _codes_dev(qx)
        wbuf, wv = _codes_dev(qw)
        for relu, bn, relu_after in TAILS:
            y1 = torch.empty(n, dtype=torch.float32, device="cuda")
            if conv:
                Q.conv_fwd_i8(xv, wv, s_x, d_sw, d_bias, y1, B, H, W, Cin, N, KS, 1, relu)
                t_plain = Q.conv_i8_ref(qx, qw, s_x, s_w, bias, KS, 1, relu)
            else:
                Q.dense_fwd_i8(xv, wv, s_x, d_sw, d_bias, y1, M, N, K, relu)
                t_plain = Q.dense_i8_ref(qx, qw, s_x, s_w, bias, relu)
            assert np.array_equal(_bits(y1.cpu().numpy()), _bits(t_plain).reshape(-1)), (name, "the un-fused launch is off its statement")
            for bn_kind in (("trained", "hand") if bn else (None,)):
                if bn:
                    gamma, beta, mm, mv, eps = _bn_vectors(bn_kind, N, t_plain, rs)
                    y2, d_scale, d_shift = _bn_eval(y1, _dev(gamma), _dev(beta), _dev(mm), _dev(mv), eps, relu_after, M, N)
                    scale, shift = d_scale.cpu().numpy(), d_shift.cpu().numpy()
                    if bn_kind == "hand":
                        assert np.array_equal(_bits(scale), _bits(gamma)) and np.array_equal(_bits(shift), _bits(beta))
                    t = Q.fma32_ref(t_plain, scale, shift)
                    two = (t_plain * scale + shift).astype(f)
                    parted += int((_bits(two) != _bits(t)).sum())
                    if relu_after:
                        t = np.where(t > 0, t, f(0)).astype(f)
                    # the paragraph of the definition, checked on the device: the un-fused BatchNorm IS one fma
                    assert np.array_equal(_bits(y2.cpu().numpy()[:n]), _bits(t).reshape(-1)), (name, bn_kind, "scale_shift is not one fma")
                else:
                    y2, d_scale, d_shift, scale, shift, t = y1, None, None, None, None, t_plain
                tmax = float(np.abs(t).max())
                ranges = {"all": (f(tmax), f(tmax / 5), f(0.0)), "clamp": (f(tmax / 5),), "both": (f(tmax), f(tmax / 5))}[which]
                for a_out in ranges:
                    # the chain's last launch, on a copy: y2 serves every range
                    yc, cc = y2[:n].clone(), torch.empty(n, dtype=torch.int8, device="cuda")
                    Q.fake_quant_act_codes(yc, bits, a_out, cc)
                    ybuf, yv = _out_dev(n)
                    cbuf, cv = _codes_out_dev(n)
                    if conv:
                        Q.conv_fwd_i8_q(xv, wv, s_x, d_sw, d_bias, yv, cv, B, H, W, Cin, N, KS, 1, relu, bits, a_out, d_scale, d_shift, relu_after)
                        want_y, want_q = Q.conv_i8_q_ref(qx, qw, s_x, s_w, bias, KS, 1, relu, scale, shift, relu_after, bits, a_out)
                    else:
                        Q.dense_fwd_i8_q(xv, wv, s_x, d_sw, d_bias, yv, cv, M, N, K, relu, bits, a_out, d_scale, d_shift, relu_after)
                        want_y, want_q = Q.dense_i8_q_ref(qx, qw, s_x, s_w, bias, relu, scale, shift, relu_after, bits, a_out)
                    y, q = _read_out(ybuf, n), _read_codes(cbuf, n)
                    tag = (name, (relu, bn_kind, relu_after), float(a_out))
                    if a_out == f(tmax / 5) and tmax > 0:
                        assert int(np.abs(want_q.astype(np.int32)).max()) == Q.qmax_of(bits), "the clamp does not work in this case"
                    assert np.array_equal(_bits(y), _bits(yc.cpu().numpy())), (tag, "y against the chain", int((_bits(y) != _bits(yc.cpu().numpy())).sum()))
                    assert np.array_equal(q, cc.cpu().numpy()), (tag, "codes against the chain", int((q != cc.cpu().numpy()).sum()))
                    assert np.array_equal(_bits(y), _bits(want_y).reshape(-1)), (tag, "y against the statement")
                    assert np.array_equal(q, want_q.reshape(-1)), (tag, "codes against the statement")
                    if name.startswith("onehot") and a_out == f(tmax) and not bn and not relu:   # bias and weights: no two alike
                        assert len(set(want_q.reshape(M, N)[0].tolist())) > N // 8, "the codes of a row tell its channels apart"
                    checked += 1
    return checked, parted


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_lone_conv_equals_the_chain_and_the_statement_in_bytes(shape):
    checked, parted = _check_layer(True, shape)
    print(f"    conv i8 q {shape}: {checked} launches equal in bytes; fma and two roundings part on {parted} elements of the BatchNorm cases")
    assert parted > 0, "no element tells a fused multiply-add from two roundings: the BatchNorm families show nothing"


@pytest.mark.parametrize("shape", DENSE_SHAPES)
def test_lone_dense_equals_the_chain_and_the_statement_in_bytes(shape):
    checked, parted = _check_layer(False, shape)
    print(f"    dense i8 q {shape}: {checked} launches equal in bytes; fma and two roundings part on {parted} elements of the BatchNorm cases")
    assert parted > 0


def test_empty_batch_writes_nothing_refusals_are_refusals_and_the_library_works_afterwards():
    torch = _torch()
    from cmoop_audio_processing_amd import _lib, quant as Q
    rs = np.random.RandomState(5)
    qx, qw = rs.randint(-127, 128, (2, 2, 2, 16)).astype(np.int8), rs.randint(-127, 128, (16, 16)).astype(np.int8)
    xbuf, xv = _codes_dev(qx)
    wbuf, wv = _codes_dev(qw)
    sw, bias = torch.full((16,), 0.01, device="cuda"), torch.zeros(16, device="cuda")
    one = torch.ones(16, device="cuda")
    ybuf, yv = _out_dev(128)
    cbuf, cv = _codes_out_dev(128)
    Q.conv_fwd_i8_q(xv, wv, 0.01, sw, bias, yv, cv, 0, 2, 2, 16, 16, 1, 1, 1, 8, 1.0)
    Q.dense_fwd_i8_q(xv, wv, 0.01, sw, bias, yv, cv, 0, 16, 16, 1, 8, 1.0, one, one, 1)
    clean = lambda: (_bits(_read_out(ybuf, 128)) == 0xFFFFFFFF).all() and (_read_codes(cbuf, 128) == SENTINEL_CODE).all()
    assert clean(), "B = 0 wrote something"
    conv = lambda **kw: Q.conv_fwd_i8_q(xv, wv, 0.01, sw, bias, kw.pop("y", yv), kw.pop("codes", cv), 2, 2, 2, 16, kw.pop("Cout", 16), 1, 1, 1,
                                        kw.pop("bits", 8), kw.pop("a_out", 1.0), **kw)
    dense = lambda **kw: Q.dense_fwd_i8_q(xv, wv, 0.01, sw, bias, yv, kw.pop("codes", cv), 8, kw.pop("N", 16), 16, 1, kw.pop("bits", 8), 1.0, **kw)
    for call, what in ((lambda: conv(Cout=6), "multiple of 4"), (lambda: dense(N=14), "multiple of 4"),
                       (lambda: conv(codes=None), "NULL codes"), (lambda: dense(codes=None), "NULL codes"),
                       (lambda: conv(bn_scale=one), "together"), (lambda: conv(bn_shift=one), "together"),
                       (lambda: dense(bn_scale=one), "together"), (lambda: dense(bn_shift=one), "together"),
                       (lambda: conv(bits=1), "bits"), (lambda: conv(bits=9), "bits"), (lambda: dense(bits=9), "bits"),
                       (lambda: conv(a_out=None), "a_out"),
                       (lambda: conv(y=ybuf[GUARD + 1:]), "aligned"), (lambda: conv(codes=cbuf[PAD + 1:]), "aligned")):
        with pytest.raises(_lib.CmoopError, match=what):
            call()
    assert clean(), "a refused call wrote something"
    conv()
    want_y, want_q = Q.conv_i8_q_ref(qx, qw.reshape(16, 1, 1, 16), 0.01, np.full(16, 0.01, np.float32), np.zeros(16, np.float32), 1, 1, 1,
                                     out_bits=8, a_out=1.0)
    assert np.array_equal(_bits(_read_out(ybuf, 128)), _bits(want_y).reshape(-1)) and np.array_equal(_read_codes(cbuf, 128), want_q.reshape(-1))


# ---- nets: the patch size and harness of test_gpu_int8_dw.py ------------------------------------------------------------------
T, F, CLASSES = 21, 12, 10
# (variant, gene, the depthwise level)
NETS = [("A", (16, 3, 1, 1, 2, 0), False), ("A", (16, 3, 0, 2, 1, 1), False), ("B", (16, 3, 1, 1, 1, 0), False),
        ("A_ds", (16, 5, 1, 1, 1, 0), True), ("A_ds", (16, 5, 1, 1, 1, 0), False), ("B_ds", (16, 3, 1, 1, 1, 1), False)]


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


def _raw_set_level(net, on):
    from cmoop_audio_processing_amd import _lib
    return _lib.lib().cmoop_net_set_int8_fused(net._h, C.c_int32(int(on)))


def _bn_of(gene, variant, params, b_off, Cout):
    """(gamma, beta, moving mean, moving variance) of the BatchNorm whose tensors follow the bias at b_off in the arena."""
    from cmoop_audio_processing_amd import genes as G
    off, names = 0, []
    for name, shape, role in G.param_tensors(gene, G.VARIANT_NAMES[variant], CLASSES):
        names.append((off, role, int(np.prod(shape))))
        off += int(np.prod(shape))
    k = [i for i, (o, role, _n) in enumerate(names) if o == b_off and role == "bias"]
    assert len(k) == 1 and [r for _o, r, _n in names[k[0] + 1:k[0] + 5]] == ["gamma", "beta", "moving_mean", "moving_var"]
    return [params[o:o + Cout] for o, _r, _n in names[k[0] + 1:k[0] + 5]]


@pytest.mark.parametrize("variant, gene, dw", NETS)
def test_a_net_under_the_level_equals_the_pass_without_it_and_every_fused_op_the_statement(variant, gene, dw):
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    net, X, _y = _ready_net(gene, variant)
    with net:
        sites = {s[0]: k for k, s in enumerate(Q.act_sites(gene, variant, CLASSES, T, F))}
        net.set_int8(True, depthwise=dw)
        assert net.int8 and net.int8_depthwise == dw and not net.int8_fused
        ops1 = net.int8_ops()
        off = {rows: (net.predict_logits(X[:rows]).cpu().numpy(), _acts(net, 5 if rows == 5 else 3)) for rows in (5, 8)}
        fops = net.int8_fused_ops()
        assert [(r["op"], r["in_act"], r["out_act"], r["bn_op"], r["relu_after"], r["site_act"]) for r in fops] == \
            Q.int8_fused_ops(gene, variant, CLASSES, T, F) and fops
        _wq, codes, scales = net.get_quantized()
        params, rec = net.get_params(), net.get_act_ranges()
        net.set_int8(True, depthwise=dw, fused=True)
        assert net.int8 and net.int8_depthwise == dw and net.int8_fused and net.int8_ops() == ops1
        unwritten = {r["out_act"] for r in fops if r["bn_op"] >= 0}          # the pre-BatchNorm acts: nothing reads them
        for rows in (5, 8):                                                  # the last chunk: full (5 rows), partial (3 rows)
            B = 5 if rows == 5 else 3
            logits = net.predict_logits(X[:rows]).cpu().numpy()
            on = _acts(net, B)
            assert logits.tobytes() == off[rows][0].tobytes(), "the logits changed"
            assert on.keys() == off[rows][1].keys()
            for i, v in on.items():
                if i not in unwritten:
                    assert v.tobytes() == off[rows][1][i].tobytes(), (variant, gene, rows, "act", i)
            for r in fops:
                r_in, r_out = rec["r"][r["site"]], rec["r"][r["out_site"]]
                assert sites[r["in_act"]] == r["site"] and sites[r["site_act"]] == r["out_site"]
                qx = Q.act_codes_ref(on[r["in_act"]], 8, r_in)
                s_x = Q.act_scale_ref(r_in, 8)
                assert np.array_equal(_bits((qx.astype(np.float32) * s_x).astype(np.float32)), _bits(on[r["in_act"]])), "the site is off its grid"
                Cin, Cout, KS = r["Cin"], r["Cout"], r["KS"]
                qw = codes[r["w_off"]: r["w_off"] + Cout * KS * KS * Cin]
                s_w, bias = scales[r["scale_off"]: r["scale_off"] + Cout], params[r["b_off"]: r["b_off"] + Cout]
                scale = shift = None
                if r["bn_op"] >= 0:
                    gamma, beta, mm, mv = _bn_of(gene, variant, params, r["b_off"], Cout)
                    dummy = torch.zeros(4, device="cuda")
                    _y2, d_scale, d_shift = _bn_eval(dummy, _dev(gamma), _dev(beta), _dev(mm), _dev(mv), 1e-3, 0, 0, Cout)
                    scale, shift = d_scale.cpu().numpy(), d_shift.cpu().numpy()
                if r["kind"] == 0:
                    want = Q.conv_i8_q_ref(qx.reshape(B, r["H"], r["W"], Cin), qw, s_x, s_w, bias, KS, r["stride"], r["relu"], scale, shift,
                                           r["relu_after"], 8, r_out)[0]
                else:
                    want = Q.dense_i8_q_ref(qx.reshape(B, Cin), qw.reshape(Cout, Cin), s_x, s_w, bias, r["relu"], scale, shift, r["relu_after"],
                                            8, r_out)[0]
                assert np.array_equal(_bits(want).reshape(-1), _bits(on[r["site_act"]]).reshape(-1)), (variant, gene, rows, r)
        # the level off again: the launches it replaced are back, in bytes
        net.set_int8(True, depthwise=dw)
        assert not net.int8_fused and net.predict_logits(X).cpu().numpy().tobytes() == off[8][0].tobytes()
        assert all(v.tobytes() == off[8][1][i].tobytes() for i, v in _acts(net, 3).items())


def test_a_train_step_under_the_level_is_the_plain_train_step():
    gene, variant = (16, 3, 1, 1, 2, 0), "A"
    plain, X, y = _ready_net(gene, variant)
    mode, _X, _y = _ready_net(gene, variant)
    with plain, mode:
        mode.set_int8(True, fused=True)
        mode.predict_proba(X)
        losses = [net.train_step(X, y, None, 2, 3) for net in (plain, mode)]
        assert np.asarray(losses[0]).tobytes() == np.asarray(losses[1]).tobytes(), "the loss"
        assert mode.get_grads().tobytes() == plain.get_grads().tobytes()
        assert mode.get_params().tobytes() == plain.get_params().tobytes()
        assert mode.get_act_ranges().tobytes() == plain.get_act_ranges().tobytes()
        assert mode.int8 and mode.int8_fused
        two = mode.predict_logits(X).cpu().numpy()
        plain.set_int8(True)
        assert plain.predict_logits(X).cpu().numpy().tobytes() == two.tobytes()


def test_the_net_with_the_fewest_fusible_ops_changes_in_nothing_else():
    """Every candidate of the search space has a hidden dense layer (fc >= 1), so no real plan is without a fusible op: the
    nearest one is topology B at fc = 1, whose only fusible op is that layer.  Its convolutions, which all end in a pool, and its
    skip projection keep their launches: every act and the logits are the bytes of the pass without the level."""
    from cmoop_audio_processing_amd import quant as Q
    gene, variant = (16, 3, 1, 1, 1, 0), "B"
    net, X, _y = _ready_net(gene, variant)
    with net:
        net.set_int8(True)
        want, acts = net.predict_logits(X).cpu().numpy(), _acts(net, 3)
        net.set_int8(True, fused=True)
        fops = net.int8_fused_ops()
        assert net.int8_fused and all(r["kind"] == 1 for r in fops), "B: the hidden dense layers only"
        assert len(net.int8_ops()) > len(fops)
        assert net.predict_logits(X).cpu().numpy().tobytes() == want.tobytes()
        assert all(v.tobytes() == acts[i].tobytes() for i, v in _acts(net, 3).items())
        assert Q.int8_fused_ops(gene, variant, CLASSES, T, F) == [(r["op"], r["in_act"], r["out_act"], -1, 0, r["site_act"]) for r in fops]


def test_refusals_and_what_drops_the_level():
    from cmoop_audio_processing_amd import _lib, quant as Q
    gene, variant = (16, 3, 1, 1, 2, 0), "A"
    net, X, _y = _ready_net(gene, variant)
    with net:
        want = net.predict_logits(X).cpu().numpy()
        assert _raw_set_level(net, 1) != 0 and b"set_int8 first" in _lib.lib().cmoop_last_error()     # the level without set_int8
        with pytest.raises(ValueError, match="needs on=True"):
            net.set_int8(False, fused=True)
        assert not net.int8 and not net.int8_fused
        assert net.predict_logits(X).cpu().numpy().tobytes() == want.tobytes()
        net.set_int8(True)
        one = net.predict_logits(X).cpu().numpy()
        net.set_int8(True, fused=True)
        assert net.predict_logits(X).cpu().numpy().tobytes() == one.tobytes()
        net.set_int8(False)                                     # integer inference off drops it
        assert not net.int8 and not net.int8_fused and _raw_set_level(net, 1) != 0
        assert net.predict_logits(X).cpu().numpy().tobytes() == want.tobytes()
        net.set_int8(True, fused=True)
        net.set_quant(None)                                     # the weight codes go: the levels go with them
        assert not net.int8 and not net.int8_fused and np.isfinite(net.predict_logits(X).cpu().numpy()).all()
        assert _raw_set_level(net, 1) != 0, "the net itself dropped the level: it is refused again"
        net.set_quant(Q.QuantConfig(bits=8))
        net.set_int8(True)                                      # back on: level 1 alone
        assert not net.int8_fused and net.predict_logits(X).cpu().numpy().tobytes() == one.tobytes()
        net.set_int8(True, fused=True)
        assert net.predict_logits(X).cpu().numpy().tobytes() == one.tobytes()
        net.set_act_quant(None)                                 # the sites' codes go as well
        assert not net.int8 and not net.int8_fused and _raw_set_level(net, 1) != 0
        assert np.isfinite(net.predict_logits(X).cpu().numpy()).all()


def test_trained_model_stream_scorer_and_report(tmp_path):
    torch = _torch()
    from cmoop_audio_processing_amd import PopulationEvaluator
    from cmoop_audio_processing_amd.deploy import StreamScorer, TrainedModel
    from cmoop_audio_processing_amd.frontend import FrontendConfig
    variant, gene = "A", (16, 3, 1, 1, 2, 0)
    rs = np.random.RandomState(9)
    yy = rs.randint(0, CLASSES, 96).astype(np.int32)
    XX = (rs.randn(96, T, F) + yy[:, None, None] * 0.3).astype(np.float32)
    X, y = torch.from_numpy(XX).cuda(), torch.from_numpy(yy).cuda()
    cfg = _cfg(variant, epochs=2, early_stop=False, lr=1e-2, seed=2)
    model = PopulationEvaluator(X[:72], y[:72], X[72:], y[72:], cfg).train_model(gene, 2)
    fields = set(vars(model))
    model.save(tmp_path / "m.npz")
    back = TrainedModel.load(tmp_path / "m.npz")
    assert set(vars(back)) == fields, "no new stored field"
    plain_cfg = _cfg(variant, quant=False, act=False)
    for m in (model, back):                                     # a saved and reloaded model behaves the same
        want = m.logits(X[72:], plain_cfg, int8=True).cpu().numpy()
        assert m.logits(X[72:], plain_cfg, int8=True, int8_fused=True).cpu().numpy().tobytes() == want.tobytes()
        with m.session(plain_cfg, int8=True, int8_fused=True) as s:
            assert s.int8 and s.int8_fused and not s.int8_depthwise
            assert s.predict_logits(X[72:]).cpu().numpy().tobytes() == want.tobytes()
    feat = X[72:80].reshape(-1, F).contiguous()
    back.frontend = FrontendConfig(n_mels=F)
    with StreamScorer(back, 7, plain_cfg, int8=True) as sc:
        stream_want = sc.net.predict_stream(feat, 7).cpu().numpy()
    with StreamScorer(back, 7, plain_cfg, int8=True, int8_fused=True) as sc:
        assert sc.net.int8 and sc.net.int8_fused
        assert sc.net.predict_stream(feat, 7).cpu().numpy().tobytes() == stream_want.tobytes()
    with pytest.raises(ValueError, match="int8_fused=True needs int8=True"):
        back.session(plain_cfg, int8_fused=True)
    base = {"rows", "argmax_agree", "max_abs_logit_diff", "int8_ops", "acc_fakequant", "acc_int8"}
    plain_rep = back.int8_report(X[72:], y[72:], plain_cfg)
    rep = back.int8_report(X[72:], y[72:], plain_cfg, fused=True)
    assert set(plain_rep) == base and set(rep) == base | {"int8_fused_ops"}, "the key comes only when asked"
    from cmoop_audio_processing_amd import quant as Q
    assert rep["int8_fused_ops"] == len(Q.int8_fused_ops(gene, variant, CLASSES, T, F)) > 0
    assert {k: rep[k] for k in base} == plain_rep, "the same logits give the same report"
    print(f"    int8_report(fused=True): {rep}")


def test_the_timing_entries_run():
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    rs = np.random.RandomState(1)
    B, H, W, Cin, Cout, KS = 4, 13, 5, 32, 64, 3
    xbuf, xv = _codes_dev(rs.randint(-127, 128, B * H * W * Cin).astype(np.int8))
    wbuf, wv = _codes_dev(rs.randint(-127, 128, Cout * KS * KS * Cin).astype(np.int8))
    sw, bias, one = torch.full((Cout,), 0.01, device="cuda"), torch.zeros(Cout, device="cuda"), torch.ones(Cout, device="cuda")
    n = B * H * W * Cout
    y, codes = torch.empty(n, dtype=torch.float32, device="cuda"), torch.empty(n, dtype=torch.int8, device="cuda")
    for kw in (dict(), dict(bn_scale=one, bn_shift=bias, relu_after=1)):
        ms = Q.conv_fwd_i8_q_time(xv, wv, 0.01, sw, bias, y, codes, B, H, W, Cin, Cout, KS, 1, 1, 8, 50.0, iters=5, **kw)
        assert np.isfinite(ms) and ms > 0
        ms = Q.dense_fwd_i8_q_time(xv, wv, 0.01, sw, bias, y, codes, 65, Cout, Cin, 1, 8, 50.0, iters=5, **kw)
        assert np.isfinite(ms) and ms > 0
    # the launches of the chain they replace have timing entries as well (tools/int8_fused_time.py adds them up)
    z = torch.empty(n, dtype=torch.float32, device="cuda")
    for ms in (Q.dense_fwd_i8_time(xv, wv, 0.01, sw, bias, y, 65, Cout, Cin, 1, iters=5),
               Q.scale_shift_time(y, z, one, bias, B * H * W, Cout, 1, iters=5)):
        assert np.isfinite(ms) and ms > 0
