"""Activation fake quantisation on the GPU: the kernels' bytes against the numpy statement, the net's sites on the grid and
nothing else touched, layer-local gradients on the GPU's own quantised operands, off is off, stale memory, the fit carries its
ranges, and the refusals.  Every test fails without the option."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, F, CLASSES = 21, 12, 10
GENES = [("A", (16, 3, 0, 1, 1, 0)), ("A", (16, 3, 1, 1, 2, 1)), ("B", (16, 3, 1, 1, 1, 0)), ("A_ds", (16, 3, 0, 1, 1, 0))]


def _torch():
    import torch
    return torch


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _inputs(n, kind, rs):
    x = (rs.randn(n) * 3).astype(np.float32)
    if kind == "ties":          # absmax 127 at 8 bits gives s = 1: k + 0.5 are exact ties
        x = (rs.randint(-120, 120, n) + 0.5).astype(np.float32)
        x[0] = 127.0
    elif kind == "zeros":
        x[:] = 0
    elif kind == "special":
        x[::3] = -0.0
        x[1::5] = np.float32(1e-41)     # denormals
    elif kind == "inf":
        x[n // 2] = np.inf
    elif kind == "nan":
        x[n // 2] = np.nan
    return x


@pytest.mark.parametrize("n", [1, 3, 4, 5, 255, 256, 1023, 4097, 2 ** 20 + 3])
def test_kernel_bytes_batch_and_tracked(n):
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    rs = np.random.RandomState(n % 1000)
    kinds = ["plain", "ties", "zeros", "special", "inf", "nan"] if n <= 4097 else ["plain", "special"]
    for offset in (0, 1):                                   # a start one float past a 16-byte boundary: the misaligned path
        for bits in (2, 4, 8):
            for kind in kinds:
                x = _inputs(n, kind, rs)
                buf = torch.full((n + offset + 8,), 777.0, dtype=torch.float32, device="cuda")
                view = buf[offset + 4: offset + 4 + n]      # buf is 256-byte aligned: offset 0 -> aligned, 1 -> misaligned
                view.copy_(torch.from_numpy(x))
                m_b, r, count = Q.fake_quant_act(view, bits, record=(0.0, 0.0, 0), momentum=0.9)
                a, y = Q.fake_quant_act_ref(x, bits)
                out = buf.cpu().numpy()
                assert np.array_equal(_bits(out[offset + 4: offset + 4 + n]), _bits(y)), (n, offset, bits, kind, "batch")
                assert (out[:offset + 4] == 777.0).all() and (out[offset + 4 + n:] == 777.0).all(), "sentinels"
                assert _bits([m_b])[0] == _bits([Q.act_range_update_ref(0, a, 0, 0.9)])[0] and count == 1
                assert _bits([r])[0] == _bits([m_b])[0]
                if kind in ("plain", "special"):            # tracked mode under a range below the absmax: the clamp works
                    rng = np.float32(np.abs(x).max() / 2)
                    view.copy_(torch.from_numpy(x))
                    Q.fake_quant_act(view, bits, a=rng)
                    _a, yt = Q.fake_quant_act_ref(x, bits, a=rng)
                    out = buf.cpu().numpy()
                    assert np.array_equal(_bits(out[offset + 4: offset + 4 + n]), _bits(yt)), (n, offset, bits, kind, "tracked")
                    # the clamp worked: the largest magnitude is the top code's, qmax * s (within an ulp of the range)
                    assert rng == 0 or (np.abs(yt).max() < np.abs(x).max() and np.abs(yt).max() <= rng * np.float32(1 + 2 ** -22))
                    assert (out[:offset + 4] == 777.0).all() and (out[offset + 4 + n:] == 777.0).all()


def test_record_after_one_two_and_three_calls():
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    rs = np.random.RandomState(5)
    rec, want_r = (0.0, 0.0, 0), np.float32(0)
    for call in range(3):
        x = (rs.randn(1000) * (call + 1)).astype(np.float32)
        d = torch.from_numpy(x).cuda()
        rec = Q.fake_quant_act(d, 8, record=rec, momentum=0.99)
        a, _y = Q.fake_quant_act_ref(x, 8)
        want_r = Q.act_range_update_ref(want_r, a, call, 0.99)
        assert _bits([rec[0]])[0] == _bits([a])[0] and _bits([rec[1]])[0] == _bits([want_r])[0] and rec[2] == call + 1


def _data(n=24, seed=0):
    torch = _torch()
    rs = np.random.RandomState(seed)
    X = torch.from_numpy(rs.randn(n, T, F).astype(np.float32)).cuda()
    y = torch.from_numpy(rs.randint(0, CLASSES, n).astype(np.int32)).cuda()
    return X, y


def _cfg(variant, **kw):
    from cmoop_audio_processing_amd import EvalConfig
    return EvalConfig(variant=variant, classes=CLASSES, batch=8, eval_batch=8, n_slots=1, **kw)


def _on_grid(y, a, bits):
    from cmoop_audio_processing_amd import quant as Q
    qmax = Q.qmax_of(bits)
    s = np.float32(np.float32(a) / np.float32(qmax))
    if not s > 0:
        return bool((y == 0).all())
    q = np.rint(y.astype(np.float64) / np.float64(s))
    return bool((np.abs(q) <= qmax).all() and np.array_equal(_bits(y), _bits(q.astype(np.float32) * s)))


def _max_code(y, a, bits):
    """The largest |code| of y on the grid of range a: qmax exactly when a is the absmax of the tensor y was quantised from."""
    from cmoop_audio_processing_amd import quant as Q
    s = np.float32(np.float32(a) / np.float32(Q.qmax_of(bits)))
    return int(np.abs(np.rint(y.astype(np.float64) / np.float64(s))).max()) if s > 0 else 0


@pytest.mark.parametrize("variant, gene", GENES)
def test_net_sites_are_on_the_grid_and_nothing_else_is(variant, gene):
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    X, y = _data()
    sites = [s[0] for s in Q.act_sites(gene, variant, CLASSES, T, F)]
    with NetSession(gene, _cfg(variant, act_quant=Q.ActQuantConfig(bits=8, momentum=0.9)), T, F, 3) as net:
        n_acts = net.act_dims(0)[5]
        net.train_step(X, y, None, 0, 8)
        rec = net.get_act_ranges()
        assert (rec["count"] == 1).all() and np.array_equal(_bits(rec["r"]), _bits(rec["m_b"]))
        for i in range(1, n_acts):
            if not net.act_dims(i)[3]:
                continue
            a = net.get_act(i, 8)
            if i in sites:
                k = sites.index(i)
                assert _max_code(a, rec["m_b"][k], 8) == 127, ("m_b is not the absmax of the batch", i)
                assert _on_grid(a, rec["m_b"][k], 8), ("site off the grid after the train step", i)
            elif a.size > 16:                                # the witness that only sites were touched
                mx = np.abs(a).max()
                assert not _on_grid(a, mx, 8), ("a non-site act lies on a quantisation grid", i)
        # a partial batch after a full one: m_b ignores the rows >= 5 the full step left in the buffer
        net.train_step(X, y, None, 8, 5)
        rec2 = net.get_act_ranges()
        for k, i in enumerate(sites):
            a = net.get_act(i, 8)
            assert _on_grid(a[:5], rec2["m_b"][k], 8) and _max_code(a[:5], rec2["m_b"][k], 8) == 127, ("partial batch", i)
            want = Q.act_range_update_ref(rec["r"][k], rec2["m_b"][k], 1, 0.9)
            assert _bits([want])[0] == _bits([rec2["r"][k]])[0] and rec2["count"][k] == 2
        # inference: 11 rows at eval_batch 8 -> a partial last chunk of 3 rows, quantised under the tracked ranges
        net.evaluate(X[:11], y[:11])
        rec3 = net.get_act_ranges()
        assert np.array_equal(rec3, rec2), "inference must not move the records"
        for k, i in enumerate(sites):
            a = net.get_act(i, 3)
            assert _on_grid(a, rec3["r"][k], 8), ("site off the tracked grid after evaluate", i)


def _step_bytes(cfg, gene, steps=2):
    from cmoop_audio_processing_amd.session import NetSession
    X, y = _data()
    with NetSession(gene, cfg, T, F, 11) as net:
        for s in range(steps):
            net.train_step(X, y, None, 8 * s, 8)
        st = net.get_state()
        return st["params"].tobytes() + st["m"].tobytes() + st["v"].tobytes() + repr(net.train_metrics(False)).encode()


def test_off_is_off_and_on_does_something():
    from cmoop_audio_processing_amd import PopulationEvaluator, genes as G, quant as Q
    variant, gene = GENES[1]
    base = _step_bytes(_cfg(variant), gene)
    assert _step_bytes(_cfg(variant, act_quant=None), gene) == base
    assert _step_bytes(_cfg(variant, act_quant=Q.ActQuantConfig(bits=0)), gene) == base
    assert _step_bytes(_cfg(variant, act_quant=Q.ActQuantConfig(bits=8)), gene) != base
    X, y = _data(32)
    res = []
    for aq in (None, Q.ActQuantConfig(bits=0), Q.ActQuantConfig(bits=4)):
        ev = PopulationEvaluator(X[:24], y[:24], X[24:], y[24:], _cfg(variant, epochs=1, early_stop=False, seed=5, act_quant=aq))
        res.append(ev.compute_objectives_and_constraints([G.gene_to_hparams(gene)])[0])
    assert res[0]["objs"] == res[1]["objs"] and "act_quant" not in res[0] and "act_quant" not in res[1]
    assert res[2]["act_quant"] == {"bits": 4}
    # the population call itself: the full result rows (acc, size_mb, fpr, epochs_run, val_loss) of _aq with NULL and with a
    # disabled struct are the bytes of _p; an enabled struct is another fit
    cfg = _cfg(variant, epochs=2, early_stop=False, seed=5)
    ev = PopulationEvaluator(X[:24], y[:24], X[24:], y[24:], cfg)
    pop, seeds = [gene, GENES[0][1]], [5, 6]
    base = _population(ev, cfg, "_p", None, pop, seeds)
    assert _population(ev, cfg, "_aq", None, pop, seeds) == base
    assert _population(ev, cfg, "_aq", Q.ActQuantConfig(bits=0)._struct(), pop, seeds) == base
    on = _population(ev, cfg, "_aq", Q.ActQuantConfig(bits=8)._struct(), pop, seeds)
    assert on[1] == base[1] and on[4] != base[4], "size_mb stays, the fit is another fit"


def _population(ev, cfg, symbol, aq, genes_, seeds_):
    """One direct call of cmoop_eval_population_p / _aq, every other option NULL -> bytes of acc, size_mb, fpr, epochs_run, val_loss"""
    torch = _torch()
    from cmoop_audio_processing_amd import _lib
    n = len(genes_)
    genes, seeds = np.ascontiguousarray(np.array(genes_, np.int32)), np.array(seeds_, np.uint32)
    acc, size, fpr, vl = (np.zeros(n, np.float64) for _ in range(4))
    ep = np.zeros(n, np.int32)
    c, ds = cfg.to_struct(), ev._dataset()
    extra = [C.byref(aq) if aq is not None else None] if symbol == "_aq" else []
    torch.cuda.synchronize()
    _lib.check(getattr(_lib.lib(), "cmoop_eval_population" + symbol)(
        C.byref(c), None, None, None, None, None, None, None, None, *extra, C.byref(ds), _lib.ptr(genes), _lib.ptr(seeds), C.c_int32(n),
        None, None, _lib.ptr(acc), _lib.ptr(size), _lib.ptr(fpr), _lib.ptr(ep), _lib.ptr(vl), None, None, None, None, None))
    return tuple(a.tobytes() for a in (acc, size, fpr, ep, vl))


def test_fit_snapshots_ranges_and_the_model_round_trips(tmp_path):
    torch = _torch()
    from cmoop_audio_processing_amd import PopulationEvaluator, quant as Q
    from cmoop_audio_processing_amd.deploy import TrainedModel
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = GENES[1]
    rs = np.random.RandomState(9)
    yy = rs.randint(0, CLASSES, 192).astype(np.int32)
    XX = (rs.randn(192, T, F) + yy[:, None, None] * 0.3).astype(np.float32)
    X, y = torch.from_numpy(XX).cuda(), torch.from_numpy(yy).cuda()
    cfg = _cfg(variant, epochs=6, patience=2, restore_best=True, acc_readout="evaluate", lr=3e-2, seed=2,
               act_quant=Q.ActQuantConfig(bits=8, momentum=0.9))
    with NetSession(gene, cfg, T, F, 2) as net:
        r = net.fit(X[:144], y[:144], X[144:], y[144:])
        assert np.isfinite(r["val_loss_history"]).all() and np.isfinite(r["val_accuracy_history"]).all()
        loss, _acc, _p = net.evaluate(X[144:], y[144:])
        assert loss == r["val_loss_history"][r["best_epoch"]], "the best-epoch model lost the ranges it was validated with"
        # a second net re-synchronised with set_state + set_act_ranges takes the same next step
        st, rng = net.get_state(), net.get_act_ranges()
        with NetSession(gene, cfg, T, F, 2) as twin:
            twin.set_state(st)
            twin.set_act_ranges(rng)
            assert twin.evaluate(X[144:], y[144:])[0] == loss
            for n_ in (net, twin):
                n_.train_step(X, y, None, 0, 8)
            assert net.get_params().tobytes() == twin.get_params().tobytes()
            assert net.get_act_ranges().tobytes() == twin.get_act_ranges().tobytes()
    ev = PopulationEvaluator(X[:144], y[:144], X[144:], y[144:], cfg)
    model = ev.train_model(gene, 2)
    assert model.act_bits == 8 and (model.act_ranges["count"] > 0).all()
    model.save(tmp_path / "m.npz")
    back = TrainedModel.load(tmp_path / "m.npz")
    with NetSession(gene, cfg, T, F, 2) as net:
        net.set_params(model.params)
        net.set_act_ranges(model.act_ranges)
        want = net.predict_logits(X[144:]).cpu().numpy()
    got = back.logits(X[144:], _cfg(variant)).cpu().numpy()            # a config without the option: the model turns it on
    assert np.array_equal(_bits(got), _bits(want))


def test_refusals_leave_the_net_working():
    from cmoop_audio_processing_amd import _lib, quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = GENES[0]
    X, y = _data()
    with NetSession(gene, _cfg(variant), T, F, 4) as net:
        with pytest.raises(_lib.CmoopError, match="site records"):
            net.get_act_ranges()
        net.set_act_quant(Q.ActQuantConfig(bits=8))
        for call in (lambda: net.evaluate(X, y), lambda: net.predict_proba(X), lambda: net.predict_logits(X)):
            with pytest.raises(_lib.CmoopError, match="tracked ranges"):
                call()
        for bad, field in ((Q.ActQuantConfig(bits=9), "bits"), (Q.ActQuantConfig(momentum=1.5), "momentum")):
            with pytest.raises(ValueError, match=field):
                net.set_act_quant(bad)
        st = Q.ActQuantConfig(bits=8)._struct()
        st.reserved[0] = 3
        assert _lib.lib().cmoop_net_set_actquant(net._h, C.byref(st)) != 0 and b"reserved" in _lib.lib().cmoop_last_error()
        net.train_step(X, y, None, 0, 8)                     # nothing was left in flight: the net works
        loss, acc, _p = net.evaluate(X, y)
        assert np.isfinite(loss)
        net.set_act_quant(None)                              # and off again is the plain net
        assert np.isfinite(net.evaluate(X, y)[0])


# ---- layer-local gradients on the GPU's own operands --------------------------------------------------------------------------
U = 2.0 ** -24


def _tensor_spans(gene, variant):
    """{name: (offset, shape)} of the parameter arena (genes.param_tensors order)."""
    from cmoop_audio_processing_amd import genes as G
    out, off = {}, 0
    for name, shape, _role in G.param_tensors(gene, G.VARIANT_NAMES[variant], CLASSES):
        out[name] = (off, tuple(int(v) for v in shape))
        off += int(np.prod(shape))
    return out


def _kernels_in_order(gene, variant):
    from cmoop_audio_processing_amd import genes as G
    return [(name, shape) for name, shape, role in G.param_tensors(gene, G.VARIANT_NAMES[variant], CLASSES) if role == "kernel"]


def test_dense_gradients_on_the_quantised_site():
    """The classifier and the last hidden dense layer of A (16,3,1,1,2,1), each the consumer of a site (a dropout + ReLU output):
    ia.grad against the float64 dgrad masked by site > 0 times in_mask_scale, the weight and bias gradients against the float64
    wgrad ON THE QUANTISED SITE, every operand the GPU's own.  Tolerance: the per-element bound of the dense head's own test,
    tests/test_gpu_dense_head.py:176 (R.dgrad_bound / R.wgrad_bound / R.db_bound, asserted err / bound < 1 at :191)."""
    import _dense_reference as R
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = GENES[1]
    X, y = _data()
    acts, ops, logits = Q.act_plan(gene, variant, CLASSES, T, F)
    sites = [s[0] for s in Q.act_sites(gene, variant, CLASSES, T, F)]
    dense_ops = [op for op in ops if op[0] == "dense"]
    spans = _tensor_spans(gene, variant)
    kernels = _kernels_in_order(gene, variant)[-len(dense_ops):]
    cfg = _cfg(variant, act_quant=Q.ActQuantConfig(bits=8, momentum=0.9))
    scale = R.keep_scale32(cfg.dropout)
    with NetSession(gene, cfg, T, F, 3) as net:
        p0 = net.get_params()                                # the kernels this step's forward and backward read
        net.train_step(X, y, None, 0, 8)
        g, rec = net.get_grads(), net.get_act_ranges()
        for (kind, i_in, _i2, i_out), (kname, kshape) in list(zip(dense_ops, kernels))[-2:]:
            assert i_in in sites, "the layer's input must be a site"
            site = net.get_act(i_in, 8).reshape(8, -1)
            assert _on_grid(site, rec["m_b"][sites.index(i_in)], 8)
            dy = net.get_act(i_out, 8, grad=True).reshape(8, -1)
            dx = net.get_act(i_in, 8, grad=True).reshape(8, -1)
            off, shape = spans[kname]
            N, K = dy.shape[1], site.shape[1]
            w = p0[off:off + N * K].reshape(N, K)
            dw, db = g[off:off + N * K].reshape(N, K), g[off + N * K:off + N * K + N]
            dw_ref, db_ref = R.wgrad_ref(site, dy)
            worst = {"dx": np.abs(dx - R.dgrad_ref(dy, w, site, scale)) / np.maximum(R.dgrad_bound(dy, w, scale), 1e-300),
                     "dw": np.abs(dw - dw_ref) / np.maximum(R.wgrad_bound(site, dy), 1e-300),
                     "db": np.abs(db - db_ref) / np.maximum(R.db_bound(dy), 1e-300)}
            worst = {k: float(v.max()) for k, v in worst.items()}
            print(f"\n  dense {kname} {N}x{K}: worst err/bound {worst}")
            assert np.abs(dy).max() > 0 and np.abs(dw_ref).max() > 0
            assert (dx[site <= 0] == 0).all(), "an element at code 0 passes no gradient"
            assert all(v < 1.0 for v in worst.values()), worst


def test_depthwise_gradients_on_the_quantised_site():
    """The first depthwise layer of A_ds (16,3,0,1,1,0), the consumer of the first conv's ReLU output (a site): ia.grad against
    dw_dgrad64 masked by site > 0, the kernel gradient against dw_wgrad64 on the quantised site.  Tolerance: that of
    tests/test_gpu_dwconv.py:94, gamma(n + 2) * (sum of |terms|) + U |ref| with n = K^2 (dgrad) or B H W (wgrad)."""
    import _dsnet_reference as R
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = GENES[3]
    X, y = _data()
    acts, ops, logits = Q.act_plan(gene, variant, CLASSES, T, F)
    sites = [s[0] for s in Q.act_sites(gene, variant, CLASSES, T, F)]
    kind, i_in, _i2, i_out = [op for op in ops if op[0] == "dwconv"][0]
    assert i_in in sites
    kname, kshape = [(n_, s_) for n_, s_ in _kernels_in_order(gene, variant) if n_.endswith("/depthwise_kernel")][0]
    off, shape = _tensor_spans(gene, variant)[kname]
    k = shape[0]
    gamma = lambda m: m * U / (1.0 - m * U)                 # noqa: E731
    with NetSession(gene, _cfg(variant, act_quant=Q.ActQuantConfig(bits=8, momentum=0.9)), T, F, 3) as net:
        p0 = net.get_params()
        net.train_step(X, y, None, 0, 8)
        g, rec = net.get_grads(), net.get_act_ranges()
        site, dy, dx = net.get_act(i_in, 8), net.get_act(i_out, 8, grad=True), net.get_act(i_in, 8, grad=True)
        assert _on_grid(site, rec["m_b"][sites.index(i_in)], 8)
        w = p0[off:off + int(np.prod(shape))].reshape(shape)
        dw = g[off:off + int(np.prod(shape))].reshape(shape)
        B, H, W_, _c = site.shape
        worst = {}
        for name, got, ref, mag, n in (("dx", dx, R.dw_dgrad64(dy, w) * (site > 0), R.dw_dgrad64(dy, w, absolute=True), k * k),
                                       ("dw", dw, R.dw_wgrad64(site, dy, k), R.dw_wgrad64(site, dy, k, absolute=True), B * H * W_)):
            bound = gamma(n + 2) * mag + U * np.abs(ref)
            worst[name] = float((np.abs(got.astype(np.float64) - ref) / np.maximum(bound, 1e-300)).max())
            assert np.abs(ref).max() > 0
        print(f"\n  depthwise {kname} {shape}: worst err/bound {worst}")
        assert max(worst.values()) <= 1.0, worst


# ---- stale memory -----------------------------------------------------------------------------------------------------------------
def test_results_do_not_depend_on_what_a_buffer_held():
    """The on-path steps (a full batch, then a partial one), a fit with its snapshot, evaluate and predict_logits under
    CMOOP_POOL_FILL=0x00 and =0xFF: identical bytes for parameters, ranges and logits."""
    import os
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    variant, gene = GENES[1]
    X, y = _data(40)

    def run(fill):
        before = os.environ.get("CMOOP_POOL_FILL")
        os.environ["CMOOP_POOL_FILL"] = fill
        try:
            cfg = _cfg(variant, epochs=3, patience=1, restore_best=True, act_quant=Q.ActQuantConfig(bits=8, momentum=0.9))
            with NetSession(gene, cfg, T, F, 7) as net:
                net.train_step(X, y, None, 0, 8)
                net.train_step(X, y, None, 8, 5)
                loss, acc, preds = net.evaluate(X[:11], y[:11])
                out = [net.get_params().tobytes(), net.get_act_ranges().tobytes(), repr((loss, acc)).encode(),
                       net.predict_logits(X[:11]).cpu().numpy().tobytes()]
                r = net.fit(X[:32], y[:32], X[32:], y[32:])
                out += [net.get_params().tobytes(), net.get_act_ranges().tobytes(), r["val_loss_history"].tobytes(),
                        net.predict_logits(X[32:]).cpu().numpy().tobytes()]
                assert np.isfinite(r["val_loss_history"]).all()
            return out
        finally:
            if before is None:
                os.environ.pop("CMOOP_POOL_FILL", None)
            else:
                os.environ["CMOOP_POOL_FILL"] = before
    a, b = run("0x00"), run("0xFF")
    for k, (u, v) in enumerate(zip(a, b)):
        assert u == v, f"result {k} depends on what a pooled buffer held"


def test_the_timing_entry_runs_both_modes():
    torch = _torch()
    from cmoop_audio_processing_amd import quant as Q
    x = torch.randn(4099, device="cuda")
    for a in (None, 1.5):
        ms = Q.fake_quant_act_time(x, 8, a=a, iters=3)
        assert np.isfinite(ms) and ms > 0
    assert _on_grid(x.cpu().numpy(), 1.5, 8)
