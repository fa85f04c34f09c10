"""GPU parity, kernel by kernel, of the BatchNorm / pooling / loss / optimiser kernels of csrc/bn.hip, elem.hip, loss.hip
and optim.hip (through the per-kernel C ABI entries) against the float64 references of tests/_elem_reference.py.

Two regimes.  EXACT: small-integer inputs, integer means, power-of-two invstd / gamma -- every fp32 sum is exact in any
order, so the device result must EQUAL the float64 reference cast to float32.  FLOAT: random normal inputs, gated by
bounds derived from the kernel's structure (u = 2^-24; gamma_n = n u / (1 - n u) with n the longest fp32 chain, computed
from the launchers' own formulas), by one u per rounding of an element-wise expression evaluated in float64 from the
device's OWN read-back statistics, or -- end to end -- by 8 x the error of the same reference run in float32 on the CPU
(floor 4 u max|ref|).  Every output buffer starts NaN-filled (integers: -1).  Run with -s to see the per-case figures
(profiles/elem_kernel_parity.txt is one such run)."""

import numpy as np
import pytest
import torch

import _elem_reference as R
from _elem_reference import U, gamma_n
from cmoop_audio_processing_amd import _lib

pytestmark = pytest.mark.gpu

P = _lib.ptr
EPS = float(np.float32(1e-3))          # bn_eps as the kernels hold it (Net casts the double to float)
MOMENTUM = 0.99


def L():
    return _lib.lib()


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def nan(*shape):
    return torch.full(shape, float("nan"), device="cuda", dtype=torch.float32)


def host(t):
    return t.cpu().numpy()


def ok(rc):
    torch.cuda.synchronize()
    _lib.check(rc)


def equal(gpu, ref64):
    """Value-for-value equality with the float64 reference cast to float32 (a NaN left in the output fails; the sign of a
    zero is not compared: max(-0, 0) has no defined sign)."""
    return np.array_equal(np.asarray(gpu, np.float32), np.asarray(ref64, np.float64).astype(np.float32))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def gate8(name, gpu, ref32, ref64):
    """End-to-end gate: max|gpu - ref64| <= max(8 max|ref32 - ref64|, 4 u max|ref64|); prints both errors."""
    ref64 = np.asarray(ref64, np.float64)
    e_gpu = float(np.abs(np.asarray(gpu, np.float64) - ref64).max())
    e_ref = float(np.abs(np.asarray(ref32, np.float64) - ref64).max())
    gate = max(8.0 * e_ref, 4.0 * U * float(np.abs(ref64).max()))
    print(f"    {name}: gpu err {e_gpu:.3e}  float32-reference err {e_ref:.3e}  gate {gate:.3e}")
    return e_gpu <= gate, f"{name}: {e_gpu:.3e} > {gate:.3e}"


def within(name, gpu, ref64, bound):
    """|gpu - ref64| <= bound element-wise (a NaN fails); prints the worst ratio."""
    err = np.abs(np.asarray(gpu, np.float64) - np.asarray(ref64, np.float64))
    bound = np.broadcast_to(np.asarray(bound, np.float64), err.shape)
    bad = ~(err <= bound)
    worst = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print(f"    {name}: max err {float(err.max()) if err.size else 0.0:.3e}, worst err/bound {worst:.3f}")
    return not bad.any(), f"{name}: {int(bad.sum())} elements beyond the bound (worst err/bound {worst:.3f})"


# ---- thin wrappers ---------------------------------------------------------------------------------------------------------
def bn_train_fwd(x, gamma, beta, mm, mv, eps, momentum, relu, blocks):
    M, Cn = x.shape
    o = dict(y=nan(M, Cn), mean=nan(Cn), invstd=nan(Cn), scale=nan(Cn), shift=nan(Cn))
    rc = L().cmoop_bn_train_fwd(P(x), P(gamma), P(beta), P(mm), P(mv), P(o["y"]), P(o["mean"]), P(o["invstd"]), P(o["scale"]),
                                P(o["shift"]), M, Cn, eps, momentum, relu, blocks)
    ok(rc)
    return {k: host(v) for k, v in o.items()}


def bn_bwd(dy, x, mean, invstd, gamma, mask, blocks):
    M, Cn = x.shape
    o = dict(dx=nan(M, Cn), dgamma=nan(Cn), dbeta=nan(Cn), sums=nan(2, Cn))
    ok(L().cmoop_bn_bwd(P(dy), P(x), P(mean), P(invstd), P(gamma), P(o["dx"]), P(o["dgamma"]), P(o["dbeta"]), P(o["sums"]), M, Cn,
                        mask, blocks))
    return {k: host(v) for k, v in o.items()}


def bn_eval_fwd(x, gamma, beta, mm, mv, eps, relu):
    M, Cn = x.shape
    o = dict(y=nan(M, Cn), scale=nan(Cn), shift=nan(Cn))
    ok(L().cmoop_bn_eval_fwd(P(x), P(gamma), P(beta), P(mm), P(mv), P(o["y"]), P(o["scale"]), P(o["shift"]), M, Cn, eps, relu))
    return o


# (M, C, forced blocks): 0 = the trainer's count
BN_CASES = [
    pytest.param(1, 16, 0, id="M1-C16-zero-variance"),
    pytest.param(3, 16, 0, id="M3-C16-fewer-rows-than-rpp"),
    pytest.param(756, 16, 0, id="M756-C16"),
    pytest.param(2080, 64, 0, id="M2080-C64"),
    pytest.param(260, 512, 0, id="M260-C512-rpp2"),
    pytest.param(50, 1024, 0, id="M50-C1024-rpp1-colreduce-limit"),
    pytest.param(97, 4, 0, id="M97-C4-rpp256"),
    pytest.param(301, 24, 0, id="M301-C24-quarter-does-not-divide-256"),
    pytest.param(129, 40, 0, id="M129-C40-quarter-does-not-divide-256"),
] + [pytest.param(5000, 32, b, id=f"M5000-C32-forced-blocks-{b}" + ("-trailing-blocks-empty" if b == 4040 else ""))
     for b in (1, 64, 65, 257, 449, 4040)]


@pytest.mark.parametrize("M,Cn,blocks", BN_CASES)
def test_batchnorm_exact_regime(M, Cn, blocks):
    """Integer inputs: statistics, scale / shift, y, the moving statistics after two calls (momentum 3/4), dgamma, dbeta and
    the backward sums EQUAL the float64 reference; dx too where M is a power of two (invM is then exact), else dx is gated
    at one u per rounding from the device's own sums."""
    x, gamma, beta, eps, mu, k = R.exact_bn_input(M, Cn, 1000 + M + Cn)
    nb = blocks or R.colreduce_blocks(M, Cn)
    print(f"\n  exact M={M} C={Cn} blocks={nb} rpp={R.colreduce_rpp(Cn)}")
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    mom = 0.75
    for relu in (0, 1):
        ref = R.bn_train_ref(x, gamma, beta, eps, relu)
        mm, mv = dev(np.full(Cn, 4.0, np.float32)), dev(np.full(Cn, 8.0, np.float32))
        rmm, rmv = np.full(Cn, 4.0), np.full(Cn, 8.0)
        for _ in range(2):                                   # two consecutive calls: the moving statistics move twice
            o = bn_train_fwd(xd, gd, bd, mm, mv, eps, mom, relu, blocks)
            rmm, rmv = R.bn_moving_ref(rmm, rmv, ref["mean"], ref["var"], mom)
            for name in ("mean", "invstd", "scale", "shift", "y"):
                assert equal(o[name], ref[name]), (name, relu)
        assert equal(host(mm), rmm) and equal(host(mv), rmv), "moving statistics after two calls"
    assert np.array_equal(ref["mean"], mu) and np.array_equal(ref["var"], k)
    dy = R.exact_grad((M, Cn), 2000 + M)
    s1, s2, _, _ = R.bn_bwd_sums_ref(dy, x, ref["mean"], ref["invstd"])
    for mask in (0, 1):
        o = bn_bwd(dev(dy), xd, dev(ref["mean"].astype(np.float32)), dev(ref["invstd"].astype(np.float32)), gd, mask, blocks)
        assert equal(o["sums"][0], s1) and equal(o["sums"][1], s2), "backward sums"
        assert equal(o["dbeta"], s1) and equal(o["dgamma"], s2)
        dx, mag = R.bn_bwd_apply_ref(dy, x, ref["mean"], ref["invstd"], gamma, s1, s2, mask)
        if M & (M - 1) == 0:
            assert equal(o["dx"], dx), ("dx", mask)
            if M == 1:
                assert not o["dx"].any(), "M = 1: dx is analytically 0"
        else:
            # 10 roundings in bn_bwd_apply (see test_batchnorm_float_regime); here only those of invM are inexact
            good, msg = within(f"dx mask={mask}", o["dx"], dx, 10 * U * mag)
            assert good, msg


def _moving_bound(stat_err, prev, stat, mom, e_prev):
    # mm*momentum + stat*omm: the casts of momentum and of 1 - momentum, two multiplies and one add -- at most 3 roundings
    # on either term -- plus the carried errors of the previous value and of the statistic
    return mom * e_prev + (1.0 - mom) * stat_err + 3 * U * (np.abs(prev) * mom + np.abs(stat) * (1.0 - mom))


@pytest.mark.parametrize("M,Cn,blocks", BN_CASES)
def test_batchnorm_float_regime(M, Cn, blocks):
    """Random normal inputs: reductions within gamma_n sum|term|, the derived quantities of bn_finalize within the bound
    carried through var = s2/M - mu^2, element-wise kernels within one u per rounding from the device's own statistics,
    and forward / backward end to end against float64 autograd through the oracle at 8 x the float32 reference's error."""
    rs = np.random.RandomState(3000 + M + Cn + blocks)
    x = (rs.randn(M, Cn) * (0.5 + rs.rand(Cn)) + 0.3 * rs.randn(Cn)).astype(np.float32)
    gamma, beta = (1.0 + 0.5 * rs.randn(Cn)).astype(np.float32), rs.randn(Cn).astype(np.float32)
    dy = rs.randn(M, Cn).astype(np.float32)
    nb = blocks or R.colreduce_blocks(M, Cn)
    print(f"\n  float M={M} C={Cn} blocks={nb} rpp={R.colreduce_rpp(Cn)} chain n={R.colreduce_chain(M, Cn, nb, 1)}")
    xd, gd, bd, dyd = dev(x), dev(gamma), dev(beta), dev(dy)
    fails = []

    def check(res):
        if not res[0]:
            fails.append(res[1])

    ref0 = R.bn_train_ref(x, gamma, beta, EPS, 0)
    b_mean, b_inv, b_var = R.one_pass_invstd_bound(x, M, Cn, nb, EPS)
    for relu in (0, 1):
        mm0, mv0 = rs.randn(Cn).astype(np.float32), (0.5 + rs.rand(Cn)).astype(np.float32)
        mm, mv = dev(mm0), dev(mv0)
        rmm, rmv, emm, emv = mm0.astype(np.float64), mv0.astype(np.float64), 0.0, 0.0
        for _ in range(2):
            o = bn_train_fwd(xd, gd, bd, mm, mv, EPS, MOMENTUM, relu, blocks)
            emm = _moving_bound(b_mean, rmm, ref0["mean"], MOMENTUM, emm)
            emv = _moving_bound(b_var, rmv, ref0["var"], MOMENTUM, emv)
            rmm, rmv = R.bn_moving_ref(rmm, rmv, ref0["mean"], ref0["var"], MOMENTUM)
        check(within(f"relu={relu} mean (reduction bound)", o["mean"], ref0["mean"], b_mean))
        check(within(f"relu={relu} invstd (bound through var = s2/M - mu^2)", o["invstd"], ref0["invstd"], b_inv))
        check(within(f"relu={relu} moving mean after two calls", host(mm), rmm, emm))
        check(within(f"relu={relu} moving var after two calls", host(mv), rmv, emv))
        # scale = gamma * invstd is ONE rounding of the device's own invstd
        assert same_bits(o["scale"], gamma * o["invstd"]), "scale"
        mu_g, sc_g, sh_g = (o[n].astype(np.float64) for n in ("mean", "scale", "shift"))
        # shift = beta - mean*scale: a multiply and a subtract (or one fma): 2 roundings
        check(within(f"relu={relu} shift", o["shift"], beta - mu_g * sc_g, 2 * U * (np.abs(beta) + np.abs(mu_g * sc_g))))
        # y = x*scale + shift (+ReLU, exact): a multiply and an add (or one fma): 2 roundings
        y64 = x.astype(np.float64) * sc_g + sh_g
        check(within(f"relu={relu} y (scale_shift)", o["y"], np.maximum(y64, 0) if relu else y64,
                     2 * U * (np.abs(x * sc_g) + np.abs(sh_g))))
    # backward, from the device's own read-back mean / invstd
    mean_g, inv_g = o["mean"], o["invstd"]
    s1, s2, a1, a2 = R.bn_bwd_sums_ref(dy, x, mean_g, inv_g)
    for mask in (0, 1):
        ob = bn_bwd(dyd, xd, dev(mean_g), dev(inv_g), gd, mask, blocks)
        check(within(f"mask={mask} sum dy", ob["sums"][0], s1, gamma_n(R.colreduce_chain(M, Cn, nb, 0)) * a1))
        # a term dy*((x-mu)*is) carries 3 roundings of its own
        check(within(f"mask={mask} sum dy*xhat", ob["sums"][1], s2, gamma_n(R.colreduce_chain(M, Cn, nb, 3)) * a2))
        assert same_bits(ob["dbeta"], ob["sums"][0]) and same_bits(ob["dgamma"], ob["sums"][1])
        # bn_bwd_apply: xhat = (x-mu)*is [2], ga*is [1], invM = (float)(1/M) [1], s1*invM [1], s2*invM [1], xhat*(s2*invM) [1],
        # two subtractions [2], the final product [1] = 10 roundings, each relative to at most the sum of the terms' magnitudes
        dx, mag = R.bn_bwd_apply_ref(dy, x, mean_g, inv_g, gamma, ob["sums"][0], ob["sums"][1], mask)
        check(within(f"mask={mask} dx (bn_bwd_apply)", ob["dx"], dx, 10 * U * mag))
        if M == 1:
            assert not ob["dx"].any(), "M = 1: dx is analytically 0"
        if mask == 0:
            e2e = ob
    # end to end against float64 autograd through OracleNet._bn; yardstick: the same in float32
    r64 = R.bn_autograd(x, gamma, beta, dy, EPS, torch.float64)
    r32 = R.bn_autograd(x, gamma, beta, dy, EPS, torch.float32)
    o = bn_train_fwd(xd, gd, bd, dev(np.zeros(Cn, np.float32)), dev(np.ones(Cn, np.float32)), EPS, MOMENTUM, 0, blocks)
    for i, (name, g) in enumerate((("y", o["y"]), ("dx", e2e["dx"]), ("dgamma", e2e["dgamma"]), ("dbeta", e2e["dbeta"]))):
        check(gate8("end-to-end " + name, g, r32[i], r64[i]))
    assert not fails, fails


def test_batchnorm_rejects_more_than_1024_channels():
    """C = 2048 (C/4 > 256 lanes) must return an error and launch nothing: the outputs keep their NaN fill."""
    M, Cn = 8, 2048
    x, v = dev(np.ones((M, Cn), np.float32)), dev(np.ones(Cn, np.float32))
    y, st = nan(M, Cn), [nan(Cn) for _ in range(4)]
    rc = L().cmoop_bn_train_fwd(P(x), P(v), P(v), P(v.clone()), P(v.clone()), P(y), P(st[0]), P(st[1]), P(st[2]), P(st[3]), M, Cn, EPS,
                                MOMENTUM, 0, 0)
    torch.cuda.synchronize()
    assert rc != 0 and b"1024" in L().cmoop_last_error()
    assert torch.isnan(y).all() and all(torch.isnan(t).all() for t in st)
    dx, dg, db = nan(M, Cn), nan(Cn), nan(Cn)
    rc = L().cmoop_bn_bwd(P(x), P(x), P(v), P(v), P(v), P(dx), P(dg), P(db), None, M, Cn, 0, 0)
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(dx).all() and torch.isnan(dg).all()


def test_grid_stride_wrap_of_the_elementwise_kernels():
    """M = 66000, C = 128: n4 = 2 112 000 float4 elements, above the 8192 x 256 thread cap of the element-wise grids, so
    the grid-stride loops of scale_shift, bn_bwd_apply, add_relu, gap_bwd (as B = 50, HW = 1320) and adam_kernel take a
    second trip.  Integer inputs; EVERY element is checked."""
    M, Cn = 66000, 128
    assert M * Cn // 4 > R.EW_GRID_CAP and 50 * 1320 == M
    rs = np.random.RandomState(7)
    x = rs.randint(-8, 9, (M, Cn)).astype(np.float32)
    dy = R.exact_grad((M, Cn), 8)
    mu, var = rs.randint(-2, 3, Cn).astype(np.float32), np.where(np.arange(Cn) % 2, 14.0, 2.0).astype(np.float32)
    gamma = (2.0 ** rs.randint(-2, 3, Cn)).astype(np.float32)
    beta = rs.randint(-3, 4, Cn).astype(np.float32)
    xd, dyd = dev(x), dev(dy)
    # scale_shift through the inference entry (moving statistics: integer mean, var + eps a power of four)
    for relu in (0, 1):
        o = bn_eval_fwd(xd, dev(gamma), dev(beta), dev(mu), dev(var), 2.0, relu)
        ref = R.bn_eval_ref(x, gamma, beta, mu, var, 2.0, relu)
        assert equal(host(o["scale"]), ref["scale"]) and equal(host(o["shift"]), ref["shift"])
        assert equal(host(o["y"]), ref["y"]), f"scale_shift relu={relu}"
        del o
    # bn_bwd_apply
    inv = (1.0 / np.sqrt(var.astype(np.float64) + 2.0)).astype(np.float32)
    s1, s2, _, _ = R.bn_bwd_sums_ref(dy, x, mu, inv)
    ob = bn_bwd(dyd, xd, dev(mu), dev(inv), dev(gamma), 1, 0)
    assert equal(ob["sums"][0], s1) and equal(ob["sums"][1], s2) and equal(ob["dgamma"], s2) and equal(ob["dbeta"], s1)
    dx, mag = R.bn_bwd_apply_ref(dy, x, mu, inv, gamma, s1, s2, 1)
    good, msg = within("wrap dx (bn_bwd_apply, 10 roundings)", ob["dx"], dx, 10 * U * mag)
    assert good, msg
    del ob
    # add_relu
    y = nan(M, Cn)
    ok(L().cmoop_add_relu(P(xd), P(dyd), P(y), M * Cn))
    assert np.array_equal(host(y), np.maximum(x + dy, np.float32(0))), "add_relu"
    # gap_bwd: B = 50, HW = 1320
    B, HW = 50, 1320
    g = rs.randn(B, Cn).astype(np.float32)
    gd = dev(g)
    ok(L().cmoop_gap_bwd(P(gd), P(xd), P(y), B, HW, Cn))
    exp = np.where(x.reshape(B, HW, Cn) > 0, (g * np.float32(1.0 / HW))[:, None, :], np.float32(0))
    assert same_bits(host(y).reshape(B, HW, Cn), exp), "gap_bwd"
    del y
    _adam_run(M * Cn, 5, seed=9)


# ---- conditioning of the one-pass variance -----------------------------------------------------------------------------------
CONDITIONING = [("0", 0.0, 1.0), ("10", 10.0, 1.0), ("100", 100.0, 1.0), ("1000", 1000.0, 1.0), ("mean 50, std 0.05", 50.0, 0.05)]


@pytest.mark.parametrize("M,Cn", [(756, 16), (2080, 64)])
def test_one_pass_variance_conditioning(M, Cn):
    """bn_finalize forms var = s2/M - mu^2 from fp32 partial sums of x and x^2: its error grows with (mean/std)^2.  Asserted:
    the bound derived from the reduction (holds by construction unless the kernel is wrong), and that at ratio 0 the
    device's invstd is within 8 x the error of a two-pass float32 reference.  Printed: the measured relative invstd error
    per ratio beside the two-pass float32 reference's (DESIGN.md section 2 quotes this table)."""
    rs = np.random.RandomState(M)
    kind = np.arange(Cn) % len(CONDITIONING)
    mean = np.array([CONDITIONING[k][1] for k in kind])
    std = np.array([CONDITIONING[k][2] for k in kind])
    x = (rs.randn(M, Cn) * std + mean).astype(np.float32)
    ones, zeros = np.ones(Cn, np.float32), np.zeros(Cn, np.float32)
    nb = R.colreduce_blocks(M, Cn)
    o = bn_train_fwd(dev(x), dev(ones), dev(zeros), dev(zeros), dev(ones), EPS, MOMENTUM, 0, 0)
    ref = R.bn_train_ref(x, ones, zeros, EPS, 0)
    m32 = x.mean(axis=0, dtype=np.float32)
    v32 = ((x - m32) ** 2).mean(axis=0, dtype=np.float32)
    two_pass = (np.float32(1) / np.sqrt(v32 + np.float32(EPS))).astype(np.float32)
    b_mean, b_inv, _ = R.one_pass_invstd_bound(x, M, Cn, nb, EPS)
    rel_gpu = np.abs(o["invstd"] - ref["invstd"]) / ref["invstd"]
    rel_two = np.abs(two_pass - ref["invstd"]) / ref["invstd"]
    print(f"\n  one-pass variance, M={M} C={Cn} blocks={nb}: relative invstd error (max over the channels of a ratio)")
    print("    |mean|/std            device one-pass   two-pass float32   derived bound")
    for k, (name, _, _) in enumerate(CONDITIONING):
        sel = kind == k
        print(f"    {name:<20}  {rel_gpu[sel].max():.3e}         {rel_two[sel].max():.3e}          {(b_inv / ref['invstd'])[sel].max():.3e}")
    good, msg = within("invstd, derived bound", o["invstd"], ref["invstd"], b_inv)
    assert good, msg
    good, msg = within("mean, derived bound", o["mean"], ref["mean"], b_mean)
    assert good, msg
    z = kind == 0
    e_gpu, e_ref = np.abs(o["invstd"] - ref["invstd"])[z].max(), np.abs(two_pass - ref["invstd"])[z].max()
    gate = max(8 * e_ref, 4 * U * ref["invstd"][z].max())
    print(f"    ratio 0: device err {e_gpu:.3e}, two-pass float32 err {e_ref:.3e}, gate {gate:.3e}")
    assert e_gpu <= gate


# ---- fused BatchNorm + pool --------------------------------------------------------------------------------------------------
POOL_SHAPES = [(1, 1, 1, 16), (2, 2, 2, 4), (2, 7, 3, 128), (3, 13, 5, 64), (5, 26, 10, 32), (2, 101, 40, 16)]


def _maxpool_fwd(y_full, B, H, W, Cn):
    OH, OW = (H + 1) // 2, (W + 1) // 2
    y, arg = nan(B, OH, OW, Cn), torch.full((B, OH, OW, Cn), 255, device="cuda", dtype=torch.uint8)
    ok(L().cmoop_maxpool_fwd(P(y_full), P(y), P(arg), B, H, W, Cn))
    return y, arg


@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("B,H,W,Cn", POOL_SHAPES)
@pytest.mark.parametrize("regime", ["exact", "float"])
def test_fused_batchnorm_pool(regime, B, H, W, Cn, relu):
    """bn_pool_fwd equals scale_shift followed by maxpool_fwd (y and arg, bit for bit); bn_pool_bwd equals maxpool_bwd
    followed by bn_bwd (bit for bit); both against the float64 reference as well.  Integer inputs and ReLU zeros put exact
    ties inside windows: the first maximum must win."""
    M = B * H * W
    OH, OW = (H + 1) // 2, (W + 1) // 2
    rs = np.random.RandomState(B * 1000 + H * 10 + Cn + relu)
    if regime == "exact":
        x, gamma, beta, eps, _, _ = R.exact_bn_input(M, Cn, 50 + M)
        g = R.exact_grad((B, OH, OW, Cn), 60 + M)
    else:
        x = (rs.randn(M, Cn) + 0.3 * rs.randn(Cn)).astype(np.float32)
        x[rs.rand(M, Cn) < 0.2] = np.float32(0.25)                       # duplicated values: ties without the ReLU, too
        gamma, beta, eps = (1 + 0.5 * rs.randn(Cn)).astype(np.float32), rs.randn(Cn).astype(np.float32), EPS
        g = rs.randn(B, OH, OW, Cn).astype(np.float32)
    print(f"\n  fused bn+pool {regime} B={B} H={H} W={W} C={Cn} relu={relu} M={M}")
    xd, gd, bd = dev(x), dev(gamma), dev(beta)
    st = bn_train_fwd(xd, gd, bd, dev(np.zeros(Cn, np.float32)), dev(np.ones(Cn, np.float32)), eps, MOMENTUM, relu, 0)
    scale, shift = dev(st["scale"]), dev(st["shift"])
    y_full = dev(st["y"])
    # forward: unfused pair vs fused kernel
    y_u, arg_u = _maxpool_fwd(y_full, B, H, W, Cn)
    y_f, arg_f = nan(B, OH, OW, Cn), torch.full((B, OH, OW, Cn), 255, device="cuda", dtype=torch.uint8)
    ok(L().cmoop_bn_pool_fwd(P(xd), P(scale), P(shift), P(y_f), P(arg_f), B, H, W, Cn, relu))
    assert same_bits(host(y_f), host(y_u)) and np.array_equal(host(arg_f), host(arg_u)), "fused forward != scale_shift + maxpool"
    # ... and against the reference: the pool of the device's own full-resolution tensor is exact (first maximum wins)
    pv, parg = R.maxpool_ref(st["y"].reshape(B, H, W, Cn))
    assert equal(host(y_f), pv) and np.array_equal(host(arg_f), parg), "pooled values / first-maximum positions"
    srt = np.sort(_windows(st["y"].reshape(B, H, W, Cn)), axis=3)
    n_ties = int((srt[:, :, :, -1] == srt[:, :, :, -2]).sum())
    print(f"    windows with an exact tie for the maximum: {n_ties}")
    assert n_ties > 0 or M < 42, "the input must put exact ties inside windows"
    sc64, sh64 = st["scale"].astype(np.float64), st["shift"].astype(np.float64)
    y64 = x.astype(np.float64) * sc64 + sh64
    y64 = np.maximum(y64, 0) if relu else y64
    if regime == "exact":
        ref = R.bn_train_ref(x, gamma, beta, eps, relu)
        rv, rarg = R.maxpool_ref(ref["y"].reshape(B, H, W, Cn))
        assert equal(host(y_f), rv) and np.array_equal(host(arg_f), rarg)
    else:
        # 2 roundings of x*scale + shift; the maximum of values each within its bound is within the window's largest bound
        bound, _ = R.maxpool_ref((2 * U * (np.abs(x * sc64) + np.abs(sh64))).reshape(B, H, W, Cn))
        good, msg = within("pooled y vs float64", host(y_f), R.maxpool_ref(y64.reshape(B, H, W, Cn))[0], bound)
        assert good, msg
    # backward
    gdv, mean_d, inv_d = dev(g), dev(st["mean"]), dev(st["invstd"])
    for mask in (0, 1):
        dfull = nan(B, H, W, Cn)
        ok(L().cmoop_maxpool_bwd(P(gdv), P(arg_u), P(y_u), P(dfull), B, H, W, Cn, 0))
        ou = bn_bwd(dfull.reshape(M, Cn), xd, mean_d, inv_d, gd, mask, 0)
        of = dict(dx=nan(M, Cn), dgamma=nan(Cn), dbeta=nan(Cn), sums=nan(2, Cn))
        ok(L().cmoop_bn_pool_bwd(P(gdv), P(arg_f), P(xd), P(mean_d), P(inv_d), P(gd), P(of["dx"]), P(of["dgamma"]), P(of["dbeta"]),
                                 P(of["sums"]), B, H, W, Cn, mask, 0))
        of = {k: host(v) for k, v in of.items()}
        for name in ("dx", "dgamma", "dbeta", "sums"):
            assert same_bits(of[name], ou[name]), f"fused backward != maxpool_bwd + bn_bwd: {name} mask={mask}"
        dyf = R.maxpool_scatter_ref(g, parg, H, W).reshape(M, Cn)
        assert equal(host(dfull).reshape(M, Cn), dyf), "maxpool_bwd scatter"
        s1, s2, a1, a2 = R.bn_bwd_sums_ref(dyf, x, st["mean"], st["invstd"])
        nb = R.colreduce_blocks(M, Cn)
        if regime == "exact":
            assert equal(of["sums"][0], s1) and equal(of["sums"][1], s2) and equal(of["dbeta"], s1) and equal(of["dgamma"], s2)
        else:
            good, msg = within("pooled sum dy", of["sums"][0], s1, gamma_n(R.colreduce_chain(M, Cn, nb, 0)) * a1)
            assert good, msg
            good, msg = within("pooled sum dy*xhat", of["sums"][1], s2, gamma_n(R.colreduce_chain(M, Cn, nb, 3)) * a2)
            assert good, msg
        dx, mag = R.bn_bwd_apply_ref(dyf, x, st["mean"], st["invstd"], gamma, of["sums"][0], of["sums"][1], mask)
        if regime == "exact" and M & (M - 1) == 0:
            assert equal(of["dx"], dx), "dx (M a power of two)"
        else:
            good, msg = within(f"dx mask={mask} (bn_pool_bwd_apply, 10 roundings)", of["dx"], dx, 10 * U * mag)
            assert good, msg


def _windows(y):
    B, H, W, Cn = y.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    pad = np.full((B, 2 * OH, 2 * OW, Cn), -np.inf)
    pad[:, :H, :W] = y
    return pad.reshape(B, OH, 2, OW, 2, Cn).transpose(0, 1, 3, 2, 4, 5).reshape(B, OH, OW, 4, Cn)


# ---- GAP / add_relu ----------------------------------------------------------------------------------------------------------
GAP_CASES = [(1, 1, 16), (3, 2, 64), (2, 21, 128), (5, 65, 512), (2, 64, 1024), (4, 260, 4), (64, 35, 32)]


@pytest.mark.parametrize("B,HW,Cn", GAP_CASES)
def test_gap_forward_and_backward(B, HW, Cn):
    rs = np.random.RandomState(B + HW + Cn)
    print(f"\n  gap B={B} HW={HW} C={Cn} slices={256 // (Cn // 4)} chain n={R.gap_chain(HW, Cn)}")
    xi = rs.randint(-8, 9, (B, HW, Cn)).astype(np.float32)
    xf = rs.randn(B, HW, Cn).astype(np.float32)
    for name, x in (("exact", xi), ("float", xf)):
        y = nan(B, Cn)
        xd = dev(x)
        ok(L().cmoop_gap_fwd(P(xd), P(y), B, HW, Cn))
        ref, mag = R.gap_ref(x)
        if name == "exact" and HW & (HW - 1) == 0:
            assert equal(host(y), ref), "integer inputs, HW a power of two: exact"
        good, msg = within(f"gap_fwd {name}", host(y), ref, gamma_n(R.gap_chain(HW, Cn)) * mag)
        assert good, msg
        g = rs.randn(B, Cn).astype(np.float32)
        dx = nan(B, HW, Cn)
        gd = dev(g)
        ok(L().cmoop_gap_bwd(P(gd), P(xd), P(dx), B, HW, Cn))
        # one rounding: g * (float)(1/HW), masked by x > 0
        assert same_bits(host(dx), np.where(x > 0, (g * np.float32(1.0 / HW))[:, None, :], np.float32(0))), "gap_bwd"


def test_gap_rejects_a_channel_count_whose_quarter_does_not_divide_256():
    x, y = dev(np.ones((2, 3, 24), np.float32)), nan(2, 24)
    rc = L().cmoop_gap_fwd(P(x), P(y), 2, 3, 24)
    torch.cuda.synchronize()
    assert rc != 0 and torch.isnan(y).all()


@pytest.mark.parametrize("n", [4, 1028, 262148])
def test_add_relu(n):
    rs = np.random.RandomState(n)
    a, b = rs.randn(n).astype(np.float32), rs.randn(n).astype(np.float32)
    y = nan(n)
    ad, bd = dev(a), dev(b)
    ok(L().cmoop_add_relu(P(ad), P(bd), P(y), n))
    assert np.array_equal(host(y), np.maximum(a + b, np.float32(0)))          # one rounding


# ---- softmax + cross-entropy -------------------------------------------------------------------------------------------------
def _acc(loss, correct):
    return torch.from_numpy(np.array([np.float64(loss).view(np.int64), correct], np.int64)).cuda()


def _read_acc(acc):
    a = host(acc)
    return float(a[:1].view(np.float64)[0]), int(a[1])


@pytest.mark.parametrize("Cn", [2, 10, 11, 35])
@pytest.mark.parametrize("family", R.LOGIT_FAMILIES)
def test_softmax_cross_entropy(family, Cn):
    """Loss sum, dZ, predictions, correct count and softmax_probs for B in 1, 5, 255, 256, 257, 600 (one block of 256 threads
    strides over the rows).  Labels arrive through idx with row0 > 0 (n_rows clamp a no-op), then through idx = NULL;
    acc accumulates over the calls; the third call passes dz = NULL, the fourth preds = NULL.  The clip families put p beyond
    both clip bounds; the asserted conditions keep the clip gate on the same side in float32 and float64."""
    fails = []
    for fam, B, C_, seed in R.softmax_cases():
        if fam != family or C_ != Cn:
            continue
        z, y = R.make_logits(fam, B, Cn, seed)
        good, msg = R.logits_conditions(z, y, fam)
        assert good, msg
        rs = np.random.RandomState(seed)
        row0, n_rows = 3, B + 11
        idx = rs.permutation(n_rows).astype(np.int32)
        labels = rs.randint(0, Cn, n_rows).astype(np.int32)
        labels[idx[row0:row0 + B]] = y
        p64, l64, dz64 = R.softmax_ce_ref(z, y)
        p32, l32, dz32 = R.softmax_ce_autograd(z, y, torch.float32)
        pred_ref = z.argmax(axis=1)                              # numpy: the first maximum
        correct = int((pred_ref == y).sum())
        zd, acc = dev(z), _acc(0.0, 7)
        dz, preds = nan(B, Cn), torch.full((B,), -1, device="cuda", dtype=torch.int32)
        labd, idxd, yd = dev(labels), dev(idx), dev(y)
        ok(L().cmoop_softmax_ce(P(zd), P(labd), P(idxd), row0, n_rows, B, Cn, P(dz), P(acc), P(preds)))
        loss1, c1 = _read_acc(acc)
        print(f"\n  softmax_ce {fam} B={B} C={Cn}: loss sum {loss1:.6e} correct {c1 - 7}/{B}")
        assert c1 - 7 == correct and np.array_equal(host(preds), pred_ref), "preds / correct are exact"
        # the loss sum: yardstick = the float32 reference's per-row errors, summed as the kernel sums its rows
        e_gpu, e_ref = abs(loss1 - l64.sum()), float(np.abs(l32.astype(np.float64) - l64).sum())
        gate = max(8 * e_ref, 4 * U * float(np.abs(l64).sum()))
        print(f"    loss sum: gpu err {e_gpu:.3e}  float32-reference err {e_ref:.3e}  gate {gate:.3e}")
        if not e_gpu <= gate:
            fails.append(f"{fam} B={B}: loss {e_gpu:.3e} > {gate:.3e}")
        res = gate8("dZ", host(dz), dz32, dz64)
        if not res[0]:
            fails.append(f"{fam} B={B}: {res[1]}")
        # labels directly (idx = NULL, row0 = 0): same results, acc adds up
        dz2, preds2 = nan(B, Cn), torch.full((B,), -1, device="cuda", dtype=torch.int32)
        ok(L().cmoop_softmax_ce(P(zd), P(yd), None, 0, 0, B, Cn, P(dz2), P(acc), P(preds2)))
        assert same_bits(host(dz2), host(dz)) and np.array_equal(host(preds2), pred_ref)
        assert _read_acc(acc) == (loss1 + loss1, 7 + 2 * correct), "acc accumulates across calls"
        ok(L().cmoop_softmax_ce(P(zd), P(yd), None, 0, B, B, Cn, None, P(acc), P(preds2)))          # dz = NULL
        dz3 = nan(B, Cn)
        ok(L().cmoop_softmax_ce(P(zd), P(yd), None, 0, B, B, Cn, P(dz3), P(acc), None))             # preds = NULL
        l4, c4 = _read_acc(acc)
        assert c4 == 7 + 4 * correct and abs(l4 - 4 * loss1) <= 1e-15 * abs(4 * loss1) and same_bits(host(dz3), host(dz))
        # softmax_probs
        pr = nan(B, Cn)
        ok(L().cmoop_softmax_probs(P(zd), P(pr), B, Cn))
        pr = host(pr)
        assert np.array_equal(pr.argmax(axis=1), pred_ref), "the arg max of a row of probabilities is its prediction"
        assert (np.abs(pr.astype(np.float64).sum(axis=1) - 1.0) <= Cn * U).all(), "rows sum to 1 within C u"
        res = gate8("softmax_probs", pr, p32, p64)
        if not res[0]:
            fails.append(f"{fam} B={B}: {res[1]}")
    assert not fails, fails


def test_softmax_gradient_gate_is_closed_at_the_lower_clip_bound():
    """The gate of dZ is p >= lo && p <= hi, closed like the backward of torch.clamp.  Whether it is closed shows only where
    a float32 p EQUALS a bound, which the families above exclude on purpose (float64 cannot say on which side such a p
    lies).  Here 16384 rows (0, d, t) aim p_1 at lo = float32(1e-7) to within a dozen ulp; the rows whose device p_1
    (softmax_probs: the same loops, the same bits) is exactly lo -- and their neighbours on either side -- are checked
    against the float64 formula evaluated from the device's OWN probabilities, gate included.  The label is class 1, so
    the gated term p_1 / pc_1 is 1: an open gate (> for >=) loses the whole gradient of those rows."""
    B, Cn = 16384, 3
    t = np.linspace(-4.0, -2.0, B)
    d = np.log(1e-7 * (1.0 + np.exp(t)))
    z = np.stack([np.zeros(B), d, t], axis=1).astype(np.float32)
    y = np.ones(B, np.int32)
    zd, pr, dz = dev(z), nan(B, Cn), nan(B, Cn)
    ok(L().cmoop_softmax_probs(P(zd), P(pr), B, Cn))
    yd, acc = dev(y), _acc(0.0, 0)
    ok(L().cmoop_softmax_ce(P(zd), P(yd), None, 0, 0, B, Cn, P(dz), P(acc), None))
    p32 = host(pr)
    lo32, hi32 = np.float32(R.CLIP_LO), np.float32(R.CLIP_HI)
    at, below, above = (int(v) for v in ((p32[:, 1] == lo32).sum(), (p32[:, 1] < lo32).sum(), (p32[:, 1] > lo32).sum()))
    print(f"\n  softmax gate at the bound: p_1 == lo in {at} rows, below in {below}, above in {above}")
    assert at >= 8 and below >= 8 and above >= 8
    p = p32.astype(np.float64)
    gate = ((p32 >= lo32) & (p32 <= hi32)).astype(np.float64)
    pc = np.clip(p, R.CLIP_LO, R.CLIP_HI)
    S = pc.sum(axis=1, keepdims=True)
    q = np.repeat(1.0 / S, Cn, axis=1)
    q[:, 1] -= 1.0 / pc[:, 1]
    q *= gate
    dot = (p * q).sum(axis=1, keepdims=True)
    ref = p * (q - dot) / B
    # roundings from p on: S [2], 1/S [1], 1/pc_y [1], their difference [1], the dot product [6], q - dot [1], the product
    # with p [1], 1/B (a power of two: exact) -- 13, gated at 16, relative to |p_j| (|q_j| + sum_i |p_i q_i|) / B
    mag = np.abs(p) * (np.abs(q) + np.abs(p * q).sum(axis=1, keepdims=True)) / B
    good, msg = within("dZ from the device's own p", host(dz), ref, 16 * U * mag)
    assert good, msg
    hit = p32[:, 1] == lo32
    assert (np.abs(host(dz)[hit, 1]) * B > 0.5).all(), "rows with p_1 == lo keep the gradient of the true class"


# ---- Adam --------------------------------------------------------------------------------------------------------------------
LR, B1, B2, AEPS = 1e-3, 0.9, 0.999, 1e-7


def _adam_run(n, iters, seed):
    """w, m, v after each of `iters` consecutive cmoop_adam calls are bit-equal to the numpy float32 restatement.  The
    kernel pins contraction off and every operation is a single IEEE operation; the gfx950 assembly of adam_kernel holds
    the correctly rounded expansions (v_sqrt_f32 + the two-sided one-ulp fix-up, v_div_scale / v_div_fmas / v_div_fixup)."""
    rs = np.random.RandomState(seed)
    w = rs.randn(n).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    wd, md, vd = dev(w), dev(m), dev(v)
    for t in range(1, iters + 1):
        if t == 1 or n < (1 << 20):                          # the wrap-size run keeps one gradient: m and v still move every step
            g = R.adam_gradients(n, seed + t)
        alpha = R.keras_alpha(LR, B1, B2, t)
        gd = dev(g)
        ok(L().cmoop_adam(P(wd), P(gd), P(md), P(vd), n, alpha, B1, B2, AEPS))
        w, m, v = R.adam_step_f32(w, g, m, v, alpha, B1, B2, AEPS)
        for name, a, b in (("w", wd, w), ("m", md, m), ("v", vd, v)):
            assert same_bits(host(a), b), f"adam n={n} iteration {t}: {name}"


@pytest.mark.parametrize("n", [1, 255, 1025])
def test_adam_is_bit_equal_to_the_float32_restatement(n):
    _adam_run(n, 5, seed=n)


def test_adam_segments_mixed_arena():
    """Plain and slab segments mixed: S in 1, 3, 4, 5, 32, 33, 64 (across the s + 28 < S unrolled loop), a slab segment with
    n % 4 != 0 and one at off % 4 != 0 (both the scalar slab path), a plain segment longer than 1024 and one of length 1,
    stride > n.  Slab values are small integers: g is bit-equal to the integer sum, w / m / v to the restatement."""
    # (n, S): S = 0 plain
    segs = [(1, 0), (64, 1), (3, 0), (260, 3), (8, 4), (7, 5), (1501, 0), (128, 32), (300, 33), (68, 64), (5, 33)]
    rs = np.random.RandomState(11)
    off, n_, S_, stride, slab_off = [], [], [], [], []
    pos = spos = 0
    for n, S in segs:
        off.append(pos); n_.append(n); S_.append(S)
        st = (n + 7) // 4 * 4 if S else 0                                   # stride > n, a multiple of 4
        stride.append(st); slab_off.append(spos)
        pos += n
        spos += S * st
    total = pos
    scalar = [i for i, (n, S) in enumerate(segs) if S and (n % 4 or off[i] % 4)]
    assert any(segs[i][0] % 4 for i in scalar) and any(off[i] % 4 and segs[i][0] % 4 == 0 for i in scalar)
    slab = rs.randint(-4, 5, spos).astype(np.float32)
    w = rs.randn(total).astype(np.float32)
    m, v = np.zeros(total, np.float32), np.zeros(total, np.float32)
    wd, md, vd, slabd = dev(w), dev(m), dev(v), dev(slab)
    arr = lambda a, t: np.ascontiguousarray(a, t)
    for t in (1, 2, 3):
        g = R.adam_gradients(total, 20 + t)
        g_in = g.copy()
        for i, (n, S) in enumerate(segs):
            if S:
                sl = slab[slab_off[i]:slab_off[i] + S * stride[i]].reshape(S, stride[i])[:, :n]
                g[off[i]:off[i] + n] = sl.astype(np.float64).sum(axis=0)         # integers: exact in any order
                g_in[off[i]:off[i] + n] = np.nan                                   # the kernel must overwrite these
        gd = dev(g_in)
        alpha = R.keras_alpha(LR, B1, B2, t)
        a_off, a_n, a_S, a_st, a_so = arr(off, np.int64), arr(n_, np.int64), arr(S_, np.int32), arr(stride, np.int64), arr(slab_off, np.int64)
        ok(L().cmoop_adam_segments(P(wd), P(gd), P(md), P(vd), P(slabd), len(segs), P(a_off), P(a_n), P(a_S), P(a_st), P(a_so),
                                   alpha, B1, B2, AEPS))
        assert same_bits(host(gd), g), f"iteration {t}: g (slab sums)"
        w, m, v = R.adam_step_f32(w, g, m, v, alpha, B1, B2, AEPS)
        for name, a, b in (("w", wd, w), ("m", md, m), ("v", vd, v)):
            assert same_bits(host(a), b), f"adam_segments iteration {t}: {name}"


# ---- confusion / output-layer helpers ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("Cn", [2, 10, 35, 128])
@pytest.mark.parametrize("force_true_zero", [0, 1])
def test_confusion_matrix(Cn, force_true_zero):
    for n in (0, 1, 1000, 100000):
        rs = np.random.RandomState(Cn + n)
        yt = rs.randint(-2, Cn + 2, max(n, 1)).astype(np.int32)              # out-of-range labels are ignored
        yp = rs.randint(-2, Cn + 2, max(n, 1)).astype(np.int32)
        cm = torch.full((Cn, Cn), -1, device="cuda", dtype=torch.int64)
        ytd, ypd = dev(yt), dev(yp)
        ok(L().cmoop_confusion(P(ytd), P(ypd), n, Cn, force_true_zero, P(cm)))
        assert np.array_equal(host(cm), R.confusion_ref(yt[:n], yp[:n], Cn, force_true_zero)), (Cn, n)


@pytest.mark.parametrize("with_mask", [0, 1])
@pytest.mark.parametrize("M,N,K", [(1, 10, 64), (7, 35, 64), (300, 11, 16)])
def test_colsum_small_and_dense_dgrad_small(M, N, K, with_mask):
    rs = np.random.RandomState(M + N + K)
    dy, w = rs.randn(M, N).astype(np.float32), rs.randn(N, K).astype(np.float32)
    print(f"\n  output-layer helpers M={M} N={N} K={K} mask={with_mask}")
    out = nan(N)
    dyd, wd = dev(dy), dev(w)
    ok(L().cmoop_colsum_small(P(dyd), P(out), M, N))
    # a serial chain of M additions
    good, msg = within("colsum_small", host(out), dy.astype(np.float64).sum(axis=0), gamma_n(M) * np.abs(dy).sum(axis=0))
    assert good, msg
    mask = (rs.randn(M, K) * (rs.rand(M, K) < 0.7)).astype(np.float32) if with_mask else None
    scale = 1.0 / 0.7
    dx = nan(M, K)
    maskd = dev(mask) if with_mask else None
    ok(L().cmoop_dense_dgrad_small(P(dyd), P(wd), P(dx), M, N, K, P(maskd), scale))
    ref = dy.astype(np.float64) @ w.astype(np.float64)
    mag = np.abs(dy).astype(np.float64) @ np.abs(w).astype(np.float64)
    extra = 0
    if with_mask:                                   # mask > 0 ? s * (float)scale : 0 -- the cast and the multiply
        s = float(np.float32(scale))
        ref, mag, extra = np.where(mask > 0, ref * s, 0.0), mag * s, 2
        assert not host(dx)[~(mask > 0)].any()
    good, msg = within("dense_dgrad_small", host(dx), ref, gamma_n(N + extra) * mag)
    assert good, msg
