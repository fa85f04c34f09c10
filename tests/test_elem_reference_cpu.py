"""The references and input generators of tests/test_gpu_elem_kernels.py, checked on the CPU: the float64 references
against autograd through oracle/net.py, the float32 Adam restatement against OracleNet.train_step's update lines, and the
generators against the conditions the GPU tests rely on."""
import numpy as np
import pytest
import torch

import _elem_reference as R
from oracle.net import OracleConfig, OracleNet


@pytest.mark.parametrize("M,C,relu,mask", [(1, 16, 0, 0), (3, 16, 1, 0), (97, 4, 0, 1), (129, 40, 1, 1)])
def test_bn_reference_equals_float64_autograd_through_the_oracle(M, C, relu, mask):
    rs = np.random.RandomState(M + C)
    x = (rs.randn(M, C) * 2 + rs.randn(C)).astype(np.float32)
    gamma, beta = rs.randn(C).astype(np.float32), rs.randn(C).astype(np.float32)
    dy = rs.randn(M, C).astype(np.float32)
    eps = 1e-3
    y, dx, dg, db = R.bn_autograd(x, gamma, beta, dy, eps, torch.float64, relu)
    ref = R.bn_train_ref(x, gamma, beta, eps, relu)
    assert np.abs(ref["y"] - y).max() <= 1e-12 * max(1.0, np.abs(y).max())
    # the kernels' backward takes the gradient of the PRE-activation and optionally masks dx by (x > 0)
    dyp = dy * (y > 0) if relu else dy
    rdx, rdg, rdb = R.bn_bwd_ref(dyp, x, gamma, eps, 0)
    scale = max(1.0, np.abs(dx).max())
    assert np.abs(rdx - dx).max() <= 1e-10 * scale * (1e3 if M == 1 else 1)   # M = 1: dx is analytically 0, both are rounding noise
    assert np.abs(rdg - dg).max() <= 1e-10 * max(1.0, np.abs(dg).max()) and np.abs(rdb - db).max() <= 1e-12 * max(1.0, np.abs(db).max())
    if mask:
        mdx, _, _ = R.bn_bwd_ref(dyp, x, gamma, eps, 1)
        assert np.array_equal(mdx, np.where(x > 0, rdx, 0.0))
    # moving statistics: the oracle's update, two consecutive calls
    net = OracleNet((16, 3, 1, 0, 1, 0), OracleConfig(bn_eps=eps), 0, dtype=torch.float64)
    net.T["t/gamma"], net.T["t/beta"] = torch.ones(C, dtype=torch.float64), torch.zeros(C, dtype=torch.float64)
    net.T["t/moving_mean"], net.T["t/moving_var"] = torch.zeros(C, dtype=torch.float64), torch.ones(C, dtype=torch.float64)
    mm, mv = np.zeros(C), np.ones(C)
    for _ in range(2):
        net._bn(torch.from_numpy(x).double().t()[None, :, :, None], "t", True)
        mm, mv = R.bn_moving_ref(mm, mv, ref["mean"], ref["var"], 0.99)
    assert np.allclose(mm, net.T["t/moving_mean"].numpy(), rtol=1e-13, atol=1e-15)
    assert np.allclose(mv, net.T["t/moving_var"].numpy(), rtol=1e-13, atol=1e-15)


def test_bn_eval_reference_equals_the_oracle_in_eval_mode():
    rs = np.random.RandomState(5)
    M, C = 33, 24
    x, gamma, beta = rs.randn(M, C).astype(np.float32), rs.randn(C).astype(np.float32), rs.randn(C).astype(np.float32)
    mm, mv = rs.randn(C).astype(np.float32), (rs.rand(C) + 0.1).astype(np.float32)
    net = OracleNet((16, 3, 1, 0, 1, 0), OracleConfig(), 0, dtype=torch.float64)
    for k, v in (("gamma", gamma), ("beta", beta), ("moving_mean", mm), ("moving_var", mv)):
        net.T["t/" + k] = torch.from_numpy(v).double()
    y = net._bn(torch.from_numpy(x).double().t()[None, :, :, None], "t", False)[0, :, :, 0].t().numpy()
    assert np.abs(R.bn_eval_ref(x, gamma, beta, mm, mv, 1e-3, 0)["y"] - y).max() <= 1e-13 * np.abs(y).max()


@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
@pytest.mark.parametrize("C", [2, 10, 11, 35])
def test_loss_reference_equals_float64_autograd_through_the_oracle(family, C):
    z, y = R.make_logits(family, 37, C, 100 + C)
    p, loss, dz = R.softmax_ce_ref(z, y)
    pa, la, dza = R.softmax_ce_autograd(z, y, torch.float64)
    assert np.abs(p - pa).max() <= 1e-15
    assert np.abs(loss - la).max() <= 1e-12 * max(1.0, np.abs(la).max())
    assert np.abs(dz - dza).max() <= 1e-14 * max(1.0, np.abs(dza).max()) + 1e-18
    if family != "normal":                       # both clip sides are really exercised
        assert (p < R.CLIP_LO).any() and (p > R.CLIP_HI).any()


def test_logit_generators_meet_the_conditions_of_the_gpu_test_for_the_chosen_seeds():
    for fam, B, C, seed in R.softmax_cases():
        z, y = R.make_logits(fam, B, C, seed)
        ok, msg = R.logits_conditions(z, y, fam)
        assert ok, (fam, B, C, msg)
        assert z.dtype == np.float32 and y.dtype == np.int32 and y.min() >= 0 and y.max() < C
        p, _, _ = R.softmax_ce_ref(z, y)
        if fam == "confident_right":
            assert (z.argmax(axis=1) == y).all() and (p[np.arange(B), y] > R.CLIP_HI).all()
        if fam == "confident_wrong":
            assert (z.argmax(axis=1) != y).all() and (p[np.arange(B), y] < R.CLIP_LO).all()
        if fam == "normal" and B >= 5:
            first = int(z[0].argmax())
            assert (z[0] == z[0, first]).sum() == 2 and first < C - 1
    assert R.confident_logit(2) == R.confident_logit(11) == 20.0 and R.confident_logit(35) == 21.0


def test_adam_restatement_equals_the_update_lines_of_the_oracle_over_five_iterations():
    cfg = OracleConfig()
    rs = np.random.RandomState(3)
    n = 1025
    w = rs.randn(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    tw, tm, tv = (torch.from_numpy(a.copy()) for a in (w, m, v))
    for t in range(1, 6):
        g = R.adam_gradients(n, 10 + t)
        alpha = np.float32(R.keras_alpha(cfg.lr, cfg.beta1, cfg.beta2, t))
        w, m, v = R.adam_step_f32(w, g, m, v, alpha, cfg.beta1, cfg.beta2, cfg.adam_eps)
        tg = torch.from_numpy(g)
        # OracleNet.train_step, the three update lines
        tm.add_((tg - tm) * (1.0 - cfg.beta1))
        tv.add_((tg * tg - tv) * (1.0 - cfg.beta2))
        tw.sub_(tm * float(alpha) / (torch.sqrt(tv) + cfg.adam_eps))
        for a, b, name in ((w, tw, "w"), (m, tm, "m"), (v, tv, "v")):
            assert np.array_equal(a.view(np.uint32), b.numpy().view(np.uint32)), (t, name)
    g = R.adam_gradients(n, 11)
    assert (g == 0).any() and (g == np.float32(1e-25)).any() and np.float32(1e-25) * np.float32(1e-25) == 0


@pytest.mark.parametrize("M", [1, 3, 8, 42, 50, 97, 129, 195, 260, 301, 756, 1300, 2080, 5000, 8080])
def test_exact_regime_inputs_have_integer_mean_and_power_of_two_invstd(M):
    C = 16
    x, gamma, beta, eps, mu, k = R.exact_bn_input(M, C, M)
    assert np.array_equal(x, np.round(x)) and np.abs(x).max() <= 8
    ref = R.bn_train_ref(x, gamma, beta, eps, 0)
    assert np.array_equal(ref["mean"], mu) and np.array_equal(ref["var"], k)
    assert np.array_equal(np.log2(ref["invstd"]), np.round(np.log2(ref["invstd"])))
    assert np.array_equal(np.log2(np.abs(gamma)), np.round(np.log2(np.abs(gamma))))
    # every fp32 sum the kernels form stays below 2^24 units: exact in any order
    assert (x.astype(np.float64) ** 2).sum(axis=0).max() < 2 ** 24
    dy = R.exact_grad((M, C), M + 1)
    assert np.abs(dy).max() <= 4 and np.array_equal(dy, np.round(dy))
    _, _, a1, a2 = R.bn_bwd_sums_ref(dy, x, ref["mean"], ref["invstd"])
    assert max(a1.max(), a2.max() * 4) < 2 ** 24            # dy * xhat is a multiple of 1/4
    for name in ("y", "scale", "shift"):
        assert np.array_equal(ref[name], ref[name].astype(np.float32).astype(np.float64)), name


def test_one_pass_bound_grows_with_the_mean_to_std_ratio_and_holds_for_a_float32_emulation():
    """The derived bound of the one-pass variance, against a float32 emulation of the kernel's summation order."""
    M, C = 756, 16
    rs = np.random.RandomState(0)
    ratios = np.array([0, 10, 100, 1000] * 4, np.float64)
    x = (rs.randn(M, C) + ratios).astype(np.float32)
    blocks, rpp = R.colreduce_blocks(M, C), R.colreduce_rpp(C)
    rpb = R.cdiv(M, blocks)
    s1, s2 = np.zeros(C), np.zeros(C)
    for b in range(blocks):
        rows = x[b * rpb:min(M, (b + 1) * rpb)]
        t1, t2 = np.zeros((rpp, C), np.float32), np.zeros((rpp, C), np.float32)
        for r in range(len(rows)):
            t1[r % rpp] += rows[r]
            t2[r % rpp] += rows[r] * rows[r]
        a1, a2 = t1[0].copy(), t2[0].copy()
        for r in range(1, rpp):
            a1 += t1[r]
            a2 += t2[r]
        s1, s2 = s1 + a1, s2 + a2
    mu = s1 / M
    varf = np.maximum(s2 / M - mu * mu, 0).astype(np.float32)
    inv = (1.0 / np.sqrt(varf.astype(np.float64) + 1e-3)).astype(np.float32)
    bmu, binv, _ = R.one_pass_invstd_bound(x, M, C, blocks, 1e-3)
    ref = R.bn_train_ref(x, np.ones(C), np.zeros(C), 1e-3, 0)
    assert (np.abs(mu.astype(np.float32) - ref["mean"]) <= bmu).all()
    assert (np.abs(inv - ref["invstd"]) <= binv).all()
    assert binv[1] > binv[0] and binv[2] > binv[1] and binv[3] > binv[2]


def test_pool_and_confusion_references():
    rs = np.random.RandomState(1)
    y = rs.randint(-2, 3, (2, 7, 3, 8)).astype(np.float32)           # many exact ties
    v, arg = R.maxpool_ref(y)
    from oracle.net import maxpool_same
    t = maxpool_same(torch.from_numpy(y).permute(0, 3, 1, 2)).permute(0, 2, 3, 1).numpy()
    assert np.array_equal(v, t)
    g = rs.randn(*v.shape).astype(np.float32)
    full = R.maxpool_scatter_ref(g, arg, 7, 3)
    yt = torch.from_numpy(y).double().permute(0, 3, 1, 2).requires_grad_(True)
    # torch's max_pool2d also routes the gradient to the first maximum of a window
    maxpool_same(yt).backward(torch.from_numpy(g).double().permute(0, 3, 1, 2))
    assert np.array_equal(full, yt.grad.permute(0, 2, 3, 1).numpy())
    yt_, yp_ = np.array([0, 1, 5, -1, 2, 2], np.int32), np.array([1, 1, 0, 0, 7, 2], np.int32)
    assert R.confusion_ref(yt_, yp_, 3, 0).tolist() == [[0, 1, 0], [0, 1, 0], [0, 0, 1]]
    assert R.confusion_ref(yt_, yp_, 3, 1).tolist() == [[2, 2, 1], [0, 0, 0], [0, 0, 0]]
