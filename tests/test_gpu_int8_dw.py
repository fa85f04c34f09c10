"""Integer depthwise on the GPU: the lone layer EQUALS the numpy statement in bytes -- z, y and the codes, no excused element
(uniform, extreme, one-hot against asymmetric weights, narrow codes; ranges that never clamp, that clamp, and 0; sentinel-filled
outputs between guards) -- and lies within the rounding bound of the fp32 depthwise kernel on the dequantised operands; whole
separable nets op by op on the device's own operands, off is off at every level, train steps, the refusals, TrainedModel /
StreamScorer / int8_report, and the timing entry.  Every test fails without the feature."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
PAD = 256                                     # bytes of 127 on either side of a code buffer: keeps the 16-byte loads aligned
GUARD = 64                                    # floats of NaN on either side of an fp32 output
GUARD_BITS = np.uint32(0x7FC12345)
CODE_GUARD = 99                               # the bytes on either side of a code output
SENTINEL_CODE = 0x55                          # what a code output holds before the launch; no family produces it everywhere

# (B, H, W, C, K).  The kernel's work split: a workgroup is min(C / 4, 16) channel quads x 256 / that many items, an item one
# column of a run of RH rows; RH starts at min(H, 16) and halves (rounding up, not below 4) until the launch has 2^18 lanes.
SMALL = [(1, 1, 1, 16, 3),                    # every tap but the centre is padding; 1 of 64 items of the workgroup
         (2, 5, 3, 16, 5),                    # W < K; runs of 4 rows + 1
         (3, 7, 6, 32, 3),                    # 36 items over workgroups of 32: a partial second workgroup
         (1, 17, 4, 64, 5),                   # one row past a 16-row run (here runs of 4: 4 full + 1)
         (2, 4, 5, 128, 3),                   # two channel chunks
         (1, 3, 2, 512, 5),                   # eight channel chunks, H < K
         (1, 13, 5, 512, 3)]
LARGE = [(32, 17, 32, 512, 3),                # 2^18 lanes at RH = 16: the runs stay 16 rows, 17 = one run + one row
         (32, 9, 32, 512, 5)]                 # RH = 9 -> 5 fills the chip: an odd run length, the last run one row short


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


def _codes_out_dev(n):
    torch = _torch()
    buf = torch.full((n + 2 * PAD,), CODE_GUARD, dtype=torch.int8, device="cuda")
    buf[PAD:PAD + n] = SENTINEL_CODE
    return buf, buf[PAD:PAD + n]


def _read_codes(buf, n):
    raw = buf.cpu().numpy()
    assert (raw[:PAD] == CODE_GUARD).all() and (raw[PAD + n:] == CODE_GUARD).all(), "a code guard was written"
    return raw[PAD:PAD + n].copy()


def _weights_asym(K, Cn):
    """qw[ky][kx][c] = ((11 ky + 5 kx + 7 c) mod 251) - 125: 11 ky + 5 kx is different for every tap, 7 c for every channel
    -- locates a flipped or transposed tap and a permuted channel."""
    ky, kx, c = np.arange(K)[:, None, None], np.arange(K)[None, :, None], np.arange(Cn)[None, None, :]
    return (((11 * ky + 5 * kx + 7 * c) % 251) - 125).astype(np.int8)


def _families(shape, rs):
    """(name, qx [B, H, W, C], qw [K, K, C], bits of the output quantiser)."""
    B, H, W, Cn, K = shape
    sx = (B, H, W, Cn)
    n = int(np.prod(sx))
    out = [("uniform", rs.randint(-127, 128, sx).astype(np.int8), rs.randint(-127, 128, (K, K, Cn)).astype(np.int8), 8),
           ("extreme+", np.full(sx, 127, np.int8), np.full((K, K, Cn), 127, np.int8), 8),
           ("extreme-", np.full(sx, -127, np.int8), np.full((K, K, Cn), 127, np.int8), 8)]
    for pos in sorted({0, n // 3 + 1 if n > 3 else 0, n - 1}):          # one-hot: a single nonzero activation code
        qx = np.zeros(n, np.int8)
        qx[pos] = 3
        out.append((f"onehot@{pos}", qx.reshape(sx), _weights_asym(K, Cn), 8))
    for bits in (2, 4):                                                  # weight and activation bits 2 and 4
        qmax = (1 << (bits - 1)) - 1
        out.append((f"bits{bits}", rs.randint(-qmax, qmax + 1, sx).astype(np.int8), rs.randint(-qmax, qmax + 1, (K, K, Cn)).astype(np.int8),
                    bits))
    return out


def _scales(Cn, rs):
    s_w = (rs.rand(Cn) * 0.02 + 1e-3).astype(np.float32)                # normal-range scales
    return np.float32(0.0137), s_w


def _run_lone(Q, xv, wv, s_x, d_sw, shape, bits, a_out, fill):
    """One launch into sentinel-filled outputs -> (y, codes or None)."""
    B, H, W, Cn, K = shape
    n = B * H * W * Cn
    ybuf, yv = _out_dev(n, fill)
    if a_out is None:
        Q.dwconv_fwd_i8(xv, wv, s_x, d_sw, yv, B, H, W, Cn, K)
        return _read_out(ybuf, n), None
    cbuf, cv = _codes_out_dev(n)
    Q.dwconv_fwd_i8(xv, wv, s_x, d_sw, yv, B, H, W, Cn, K, out_bits=bits, a_out=a_out, codes=cv)
    return _read_out(ybuf, n), _read_codes(cbuf, n)


def _check_lone(shape, families, worst, full=True):
    """Every family of a shape: z, then y and the codes under each range, in bytes; full: the remaining forms and the fp32 bound."""
    torch = _torch()
    from cmoop_audio_processing_amd import _lib, quant as Q
    B, H, W, Cn, K = shape
    n = B * H * W * Cn
    rs = np.random.RandomState(sum(shape))
    s_x, s_w = _scales(Cn, rs)
    d_sw = torch.from_numpy(s_w).cuda()
    for name, qx, qw, bits in families(shape, rs):
        xbuf, xv = _codes_dev(qx)
        wbuf, wv = _codes_dev(qw)
        acc = Q.dwconv_i8_acc(qx, qw)
        if name.startswith("extreme") and H >= K and W >= K:
            assert int(np.abs(acc).max()) == K * K * 127 * 127
        z = Q.dwconv_i8_ref(qx, qw, s_x, s_w)
        zmax = float(np.abs(z).max())
        # the lone form: z unquantised, whatever the output held
        got = [_run_lone(Q, xv, wv, s_x, d_sw, shape, bits, None, fill)[0] for fill in (0x00, 0xFF)]
        assert np.array_equal(_bits(got[0]), _bits(got[1])), (name, "z depends on what the output held")
        assert np.array_equal(_bits(got[0]), _bits(z).reshape(-1)), (name, "z", int((_bits(got[0]) != _bits(z).reshape(-1)).sum()))
        # the net form: a range that never clamps, one small enough that the clamp works, and 0
        for a_out in (np.float32(zmax), np.float32(zmax / 5), np.float32(0.0)) if full else (np.float32(zmax / 5),):
            want_y, want_q = Q.fake_quant_act_ref(z, bits, a_out)[1], Q.act_codes_ref(z, bits, a_out)   # dwconv_i8_ref's second form
            if a_out == np.float32(zmax / 5) and zmax > 0:
                assert int(np.abs(want_q.astype(np.int32)).max()) == Q.qmax_of(bits), "the clamp does not work in this case"
            y, q = _run_lone(Q, xv, wv, s_x, d_sw, shape, bits, a_out, 0xFF)
            assert np.array_equal(_bits(y), _bits(want_y).reshape(-1)), (name, float(a_out), "y", int((_bits(y) != _bits(want_y).reshape(-1)).sum()))
            assert np.array_equal(q, want_q.reshape(-1)), (name, float(a_out), "codes", int((q != want_q.reshape(-1)).sum()))
        if not full:
            continue
        # a_out given, codes NULL: y alone, the same bytes
        ybuf, yv = _out_dev(n, 0x00)
        a_clamp = np.float32(zmax / 5)
        Q.dwconv_fwd_i8(xv, wv, s_x, d_sw, yv, B, H, W, Cn, K, out_bits=bits, a_out=a_clamp)
        assert np.array_equal(_bits(_read_out(ybuf, n)), _bits(Q.dwconv_i8_ref(qx, qw, s_x, s_w, out_bits=bits, a_out=a_clamp)[0]).reshape(-1))
        # fidelity of z: the fp32 depthwise kernel on the dequantised operands float32(q) * s
        xd = torch.from_numpy((qx.astype(np.float32) * s_x).astype(np.float32)).cuda()
        wd = torch.from_numpy((qw.astype(np.float32) * s_w).astype(np.float32)).cuda()
        yf = torch.zeros(n, dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_dwconv_fwd(C.c_void_p(xd.data_ptr()), C.c_void_p(wd.data_ptr()), C.c_void_p(yf.data_ptr()),
                                               *(C.c_int32(v) for v in (B, H, W, Cn, K))))
        _fp32_check(name, got[0].reshape(-1, Cn), yf.cpu().numpy().reshape(-1, Cn),
                    Q.dwconv_i8_acc(np.abs(qx), np.abs(qw)).reshape(-1, Cn), s_x, s_w, K * K, worst)


def _fp32_check(name, z_int, z_fp, acc_abs, s_x, s_w, n, worst):
    """|z_int - z_fp| <= gamma_(n+4) s_x s_w[c] sum|qx qw| per element, n = K^2, gamma_k = k u / (1 - k u), u = 2^-24.  The fp32
    path rounds two dequantisations, each product and n - 1 additions: (1 + d)^(n+2) on every term; the integer path rounds
    s_x s_w and one product: (1 + d)^2; the conversion is exact.  gamma_(n+2) + gamma_2 <= gamma_(n+4)."""
    k = n + 4
    gamma = k * U / (1 - k * U)
    bound = gamma * np.float64(s_x) * s_w.astype(np.float64) * acc_abs.astype(np.float64)
    err = np.abs(z_int.astype(np.float64) - z_fp.astype(np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0, 0.0, err / bound)
    worst[0] = max(worst[0], float(q.max()))
    assert (err <= bound).all(), (name, float(q.max()))


@pytest.mark.parametrize("shape", SMALL)
def test_lone_layer_equals_the_statement_in_bytes_and_the_fp32_kernel_within_the_bound(shape):
    worst = [0.0]
    _check_lone(shape, _families, worst)
    print(f"    dwconv i8 {shape}: worst |int8 - fp32| / bound {worst[0]:.3f}")


@pytest.mark.parametrize("shape", LARGE)
def test_lone_layer_at_the_run_lengths_a_full_chip_takes(shape):
    """Runs of 16 rows, and of an odd length: only a launch of 2^18 lanes keeps them, so these are the smallest such shapes.
    Uniform codes; z, and y and the codes under a range that clamps, in bytes."""
    _check_lone(shape, lambda s, rs: _families(s, rs)[:1], [0.0], full=False)


def test_empty_batch_writes_nothing_and_bad_shapes_are_refused():
    torch = _torch()
    from cmoop_audio_processing_amd import _lib, quant as Q
    xbuf, xv = _codes_dev(np.zeros(1024, np.int8))
    wbuf, wv = _codes_dev(np.zeros(25 * 32, np.int8))
    sw = torch.ones(64, device="cuda")
    ybuf, yv = _out_dev(1024, 0xFF)
    cbuf, cv = _codes_out_dev(1024)
    Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 0, 2, 2, 16, 3)
    Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 0, 2, 2, 16, 3, out_bits=8, a_out=1.0, codes=cv)
    assert (_bits(_read_out(ybuf, 1024)) == 0xFFFFFFFF).all() and (_read_codes(cbuf, 1024) == SENTINEL_CODE).all()
    for call, what in ((lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 24, 3), "power of two"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 8, 3), "power of two"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 1, 1, 1024, 3), "power of two"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 16, 1), "KS"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 16, 7), "KS"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 16, 3, codes=cv), "a_out"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 16, 3, out_bits=9, a_out=1.0), "bits"),
                       (lambda: Q.dwconv_fwd_i8(xbuf[PAD + 4:], wv, 1.0, sw, yv, 1, 2, 2, 16, 3), "aligned"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, ybuf[GUARD + 1:], 1, 2, 2, 16, 3), "aligned"),
                       (lambda: Q.dwconv_fwd_i8(xv, wv, 1.0, sw, yv, 1, 2, 2, 16, 3, out_bits=8, a_out=1.0, codes=cbuf[PAD + 1:]), "aligned")):
        with pytest.raises(_lib.CmoopError, match=what):
            call()
    assert (_bits(_read_out(ybuf, 1024)) == 0xFFFFFFFF).all() and (_read_codes(cbuf, 1024) == SENTINEL_CODE).all()


# ---- nets: the patch size and harness of test_gpu_int8.py --------------------------------------------------------------------
T, F, CLASSES = 21, 12, 10
NETS = [("A_ds", (16, 3, 1, 1, 2, 0)), ("B_ds", (16, 3, 1, 1, 2, 0)),      # k = 3 with BatchNorm
        ("A_ds", (32, 5, 0, 2, 3, 1)), ("B_ds", (32, 5, 0, 2, 3, 1))]      # k = 5 without, two residual blocks


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
    return _lib.lib().cmoop_net_set_int8_depthwise(net._h, C.c_int32(int(on)))


@pytest.mark.parametrize("variant, gene", NETS)
def test_every_depthwise_op_of_a_net_equals_the_statement_on_the_devices_own_operands(variant, gene):
    from cmoop_audio_processing_amd import quant as Q
    net, X, _y = _ready_net(gene, variant)
    with net:
        sites = {s[0]: k for k, s in enumerate(Q.act_sites(gene, variant, CLASSES, T, F))}
        fq_logits = net.predict_logits(X).cpu().numpy()        # 8 rows: a full chunk of 5 and a partial one of 3
        net.set_int8(True)                                      # level 1 alone: today's op list
        assert net.int8 and not net.int8_depthwise
        ops1 = net.int8_ops()
        assert [(r["op"], r["in_act"], r["out_act"]) for r in ops1] == Q.int8_ops(gene, variant, CLASSES, T, F)
        one = {}
        for rows in (5, 8):                                     # the last chunk: full (5 rows), partial (3 rows)
            one[rows] = (net.predict_logits(X[:rows]).cpu().numpy(), _acts(net, 5 if rows == 5 else 3))
        dops = net.int8_dw_ops()
        assert [(r["op"], r["in_act"], r["out_act"]) for r in dops] == Q.int8_dw_ops(gene, variant, CLASSES, T, F) and dops
        _wq, codes, scales = net.get_quantized()
        params, rec = net.get_params(), net.get_act_ranges()
        net.set_int8(True, depthwise=True)
        assert net.int8 and net.int8_depthwise
        assert net.int8_ops() == ops1, "the first level's list is what it was"
        first = min(r["out_act"] for r in dops)
        for rows in (5, 8):
            B = 5 if rows == 5 else 3
            logits2 = net.predict_logits(X[:rows]).cpu().numpy()
            on = _acts(net, B)
            logits1, off = one[rows]
            assert np.isfinite(logits2).all() and logits2.shape == logits1.shape
            for i in off:
                if i < first:
                    assert off[i].tobytes() == on[i].tobytes(), ("an act before the first depthwise op changed", i)
            for r in dops:
                r_in, r_out = rec["r"][r["site"]], rec["r"][r["out_site"]]
                assert sites[r["in_act"]] == r["site"] and sites[r["out_act"]] == r["out_site"]
                qx = Q.act_codes_ref(on[r["in_act"]], 8, r_in)
                s_x = Q.act_scale_ref(r_in, 8)
                assert np.array_equal(_bits((qx.astype(np.float32) * s_x).astype(np.float32)), _bits(on[r["in_act"]])), "the site is off its grid"
                K, Cn = r["KS"], r["Cin"]
                qw = codes[r["w_off"]: r["w_off"] + K * K * Cn].reshape(K, K, Cn)
                s_w = scales[r["scale_off"]: r["scale_off"] + Cn]
                want = Q.fake_quant_act_ref(Q.dwconv_i8_ref(qx, qw, s_x, s_w), 8, r_out)[1]
                assert np.array_equal(_bits(want).reshape(-1), _bits(on[r["out_act"]]).reshape(-1)), (variant, gene, rows, r)
                # the pointwise op that follows read the codes this launch wrote
                (pw,) = [o for o in ops1 if o["in_act"] == r["out_act"]]
                assert pw["kind"] == 0 and pw["KS"] == 1 and pw["site"] == r["out_site"]
                qy = Q.act_codes_ref(on[r["out_act"]], 8, r_out)
                pqw = codes[pw["w_off"]: pw["w_off"] + pw["Cout"] * pw["Cin"]].reshape(pw["Cout"], pw["Cin"])
                want = Q.conv_i8_ref(qy, pqw, Q.act_scale_ref(r_out, 8), scales[pw["scale_off"]: pw["scale_off"] + pw["Cout"]],
                                     params[pw["b_off"]: pw["b_off"] + pw["Cout"]], 1, pw["stride"], pw["relu"])
                if pw["out_act"] in sites:
                    want = Q.fake_quant_act_ref(want, 8, rec["r"][sites[pw["out_act"]]])[1]
                assert np.array_equal(_bits(want).reshape(-1), _bits(on[pw["out_act"]]).reshape(-1)), (variant, gene, rows, pw)
        # the level off: level 1 in bytes; integer inference off: the fake-quantised pass in bytes
        net.set_int8(True)
        assert net.int8 and not net.int8_depthwise
        assert net.predict_logits(X).cpu().numpy().tobytes() == one[8][0].tobytes()
        assert _acts(net, 3).keys() == one[8][1].keys() and all(v.tobytes() == one[8][1][i].tobytes() for i, v in _acts(net, 3).items())
        net.set_int8(True, depthwise=True)
        net.set_int8(False)
        assert not net.int8 and not net.int8_depthwise
        assert net.predict_logits(X).cpu().numpy().tobytes() == fq_logits.tobytes()


def test_a_train_step_under_the_level_is_the_plain_train_step():
    gene, variant = (16, 3, 1, 1, 2, 0), "A_ds"
    plain, X, y = _ready_net(gene, variant)
    mode, _X, _y = _ready_net(gene, variant)
    with plain, mode:
        mode.set_int8(True, depthwise=True)
        mode.predict_proba(X)
        for net in (plain, mode):
            net.train_step(X, y, None, 2, 3)
        assert mode.get_grads().tobytes() == plain.get_grads().tobytes()
        assert mode.get_params().tobytes() == plain.get_params().tobytes()
        assert mode.get_act_ranges().tobytes() == plain.get_act_ranges().tobytes()
        assert mode.int8 and mode.int8_depthwise
        # and the level survives the step: the next pass differs from level 1 only through it
        two = mode.predict_logits(X).cpu().numpy()
        plain.set_int8(True, depthwise=True)
        assert plain.predict_logits(X).cpu().numpy().tobytes() == two.tobytes()


def test_a_net_without_a_depthwise_op_accepts_the_level_and_nothing_changes():
    net, X, _y = _ready_net((16, 3, 1, 1, 1, 1), "A")
    with net:
        net.set_int8(True)
        want, acts = net.predict_logits(X).cpu().numpy(), _acts(net, 3)
        net.set_int8(True, depthwise=True)
        assert net.int8_depthwise and net.int8_dw_ops() == []
        assert net.predict_logits(X).cpu().numpy().tobytes() == want.tobytes()
        assert all(v.tobytes() == acts[i].tobytes() for i, v in _acts(net, 3).items())


def test_refusals_leave_the_net_working():
    from cmoop_audio_processing_amd import _lib
    gene, variant = (16, 3, 1, 1, 2, 0), "A_ds"
    net, X, _y = _ready_net(gene, variant)
    with net:
        want = net.predict_logits(X).cpu().numpy()
        assert _raw_set_level(net, 1) != 0 and b"set_int8 first" in _lib.lib().cmoop_last_error()     # the level without set_int8
        with pytest.raises(ValueError, match="needs on=True"):
            net.set_int8(False, depthwise=True)
        assert not net.int8 and not net.int8_depthwise
        assert net.predict_logits(X).cpu().numpy().tobytes() == want.tobytes()
        net.set_int8(True)
        one = net.predict_logits(X).cpu().numpy()
        net.set_int8(True, depthwise=True)
        two = net.predict_logits(X).cpu().numpy()
        assert np.isfinite(two).all()
        net.set_quant(None)                                     # the weight codes go: both levels go with them
        assert not net.int8 and not net.int8_depthwise and np.isfinite(net.predict_logits(X).cpu().numpy()).all()
        assert _raw_set_level(net, 1) != 0, "the net itself dropped the level: it is refused again"
        from cmoop_audio_processing_amd import quant as Q
        net.set_quant(Q.QuantConfig(bits=8))
        net.set_int8(True)                                      # back on: level 1 alone, not the level that was on before
        assert net.predict_logits(X).cpu().numpy().tobytes() == one.tobytes()
        net.set_int8(True, depthwise=True)
        assert net.predict_logits(X).cpu().numpy().tobytes() == two.tobytes()
        net.set_act_quant(None)                                 # the sites' codes go as well
        assert not net.int8 and not net.int8_depthwise and _raw_set_level(net, 1) != 0
        assert np.isfinite(net.predict_logits(X).cpu().numpy()).all()


def test_trained_model_stream_scorer_and_report(tmp_path):
    torch = _torch()
    from cmoop_audio_processing_amd import PopulationEvaluator
    from cmoop_audio_processing_amd.deploy import StreamScorer, TrainedModel
    from cmoop_audio_processing_amd.frontend import FrontendConfig
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = "A_ds", (16, 3, 1, 1, 2, 0)
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
    with NetSession(gene, cfg, T, F, 2) as net:                 # the live net: the model's arena under the same options
        net.set_params(model.params)
        net.set_act_ranges(model.act_ranges)
        net.set_int8(True, depthwise=True)
        want = net.predict_logits(X[72:]).cpu().numpy()
    plain_cfg = _cfg(variant, quant=False, act=False)            # a config without the options: the model turns them on
    with back.session(plain_cfg, int8=True, int8_depthwise=True) as s:
        assert s.int8 and s.int8_depthwise
        got = s.predict_logits(X[72:]).cpu().numpy()
        feat = X[72:80].reshape(-1, F).contiguous()
        stream_want = s.predict_stream(feat, 7).cpu().numpy()
    assert got.tobytes() == want.tobytes()
    assert back.logits(X[72:], plain_cfg, int8=True, int8_depthwise=True).cpu().numpy().tobytes() == want.tobytes()
    level1 = back.logits(X[72:], plain_cfg, int8=True).cpu().numpy()
    with back.session(plain_cfg, int8=True) as s:
        assert s.int8 and not s.int8_depthwise and s.predict_logits(X[72:]).cpu().numpy().tobytes() == level1.tobytes()
    back.frontend = FrontendConfig(n_mels=F)
    with StreamScorer(back, 7, plain_cfg, int8=True, int8_depthwise=True) as sc:
        assert sc.net.int8 and sc.net.int8_depthwise
        assert sc.net.predict_stream(feat, 7).cpu().numpy().tobytes() == stream_want.tobytes()
    rep = back.int8_report(X[72:], y[72:], plain_cfg, depthwise=True)
    assert set(rep) == {"rows", "argmax_agree", "max_abs_logit_diff", "int8_ops", "acc_fakequant", "acc_int8", "int8_dw_ops"}
    assert rep["rows"] == 24 and 0.0 <= rep["argmax_agree"] <= 1.0 and np.isfinite(rep["max_abs_logit_diff"])
    assert rep["int8_ops"] > 0 and rep["int8_dw_ops"] == len(_dw_op_list(gene, variant))
    assert set(back.int8_report(X[72:], y[72:], plain_cfg)) == {"rows", "argmax_agree", "max_abs_logit_diff", "int8_ops", "acc_fakequant",
                                                                "acc_int8"}, "without the level: today's keys"
    print(f"    int8_report(depthwise=True): {rep}")


def _dw_op_list(gene, variant):
    from cmoop_audio_processing_amd import quant as Q
    return Q.int8_dw_ops(gene, variant, CLASSES, T, F)


def test_the_timing_entry_runs():
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    B, H, W, Cn, K = 4, 13, 5, 64, 3
    rs = np.random.RandomState(1)
    n = B * H * W * Cn
    xbuf, xv = _codes_dev(rs.randint(-127, 128, n).astype(np.int8))
    wbuf, wv = _codes_dev(rs.randint(-127, 128, K * K * Cn).astype(np.int8))
    sw = torch.ones(Cn, device="cuda")
    y = torch.empty(n, dtype=torch.float32, device="cuda")
    codes = torch.empty(n, dtype=torch.int8, device="cuda")
    for kw in (dict(), dict(out_bits=8, a_out=50.0, codes=codes)):
        ms = Q.dwconv_fwd_i8_time(xv, wv, 0.01, sw, y, B, H, W, Cn, K, iters=5, **kw)
        assert np.isfinite(ms) and ms > 0
    # the quantiser launch it replaces has a timing entry as well (tools/int8_depthwise_time.py compares the two)
    ms = Q.fake_quant_act_codes_time(y, 8, 50.0, codes, iters=5)
    assert np.isfinite(ms) and ms > 0
