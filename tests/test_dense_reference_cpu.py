"""The references, generators and case lists of tests/test_gpu_dense_head.py, checked on the CPU: the float64 restatement
against torch autograd, the integer regime against its exactness claim, the dropout twin's masks against triviality, the
bf16 rounding against hand-worked ties, and the case lists against the coverage the GPU file states."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dense_reference as R
from cmoop_audio_processing_amd import _lib
from oracle import rng as ORNG


@pytest.mark.parametrize("M,N,K,relu", [(1, 1, 16, 0), (5, 11, 16, 1), (17, 35, 128, 1), (65, 10, 48, 0)])
def test_restatement_equals_float64_autograd(M, N, K, relu):
    x, w, bias, dy = R.gaussian_operands(M, N, K, 3 + M + N + K)
    xt, wt, bt = (torch.from_numpy(a).double().requires_grad_(True) for a in (x, w, bias))
    y = xt @ wt.t() + bt
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(dy).double())
    yn = y.detach().numpy()
    tol = 1e-12
    assert np.abs(R.fwd_ref(x, w, bias, relu) - yn).max() <= tol * max(1.0, np.abs(yn).max())
    # the kernels' backward takes the gradient of the PRE-activation; the mask is the layer INPUT's (x > 0), which autograd
    # of this one layer does not apply: it is checked as a where() of the unmasked gradient
    dyp = (dy * (yn > 0) if relu else dy).astype(np.float32)
    dx, (dw, db) = R.dgrad_ref(dyp, w), R.wgrad_ref(x, dyp)
    for got, want in ((dx, xt.grad.numpy()), (dw, wt.grad.numpy()), (db, bt.grad.numpy())):
        assert np.abs(got - want).max() <= tol * max(1.0, np.abs(want).max())
    assert np.array_equal(R.dgrad_ref(dyp, w, x, 1.5), np.where(x > 0, dx * 1.5, 0.0))


def test_dropout_reference_equals_autograd_of_the_composition():
    """h = where(keep, relu(z) * s, 0) feeding a second layer: the input gradient of that layer, gated by h > 0 and scaled,
    is autograd's gradient with respect to relu's input wherever z != 0."""
    M, N, K = 17, 35, 48
    x, w, bias, _ = R.integer_operands(M, N, K, 11)
    rate, seed, layer, step = 0.5, 42, 0, 7
    zt = (torch.from_numpy(x).double() @ torch.from_numpy(w).double().t() + torch.from_numpy(bias).double()).requires_grad_(True)
    keep = ORNG.dropout_keep(seed, layer, step, M, N, rate)
    ht = torch.where(torch.from_numpy(keep), torch.relu(zt) * float(R.keep_scale32(rate)), torch.zeros((), dtype=torch.float64))
    h, keep2 = R.dropout_ref(np.maximum(zt.detach().numpy(), 0.0), seed, layer, step, rate)
    assert np.array_equal(keep, keep2) and np.array_equal(R.f64(h), ht.detach().numpy())
    g = np.random.RandomState(5).randint(-2, 3, (M, N)).astype(np.float64)
    ht.backward(torch.from_numpy(g))
    assert np.array_equal(R.f64(R.dropout_dgrad_ref(g, h, rate)), zt.grad.numpy())
    assert h.dtype == np.float32 and (h[~keep] == 0).all() and np.signbit(h).sum() == 0


def test_keep_scales_and_thresholds():
    assert ORNG.dropout_threshold(0.3) == 5033164 and ORNG.dropout_threshold(0.5) == 1 << 23
    assert ORNG.dropout_threshold(R.SMALLEST_RATE) == 1 and ORNG.dropout_threshold(R.SMALLEST_RATE / 2) == 0
    assert R.keep_scale32(0.5) == np.float32(2.0)
    assert R.keep_scale32(R.SMALLEST_RATE) == np.float32(1.0) + np.float32(2.0 ** -23)
    s = R.keep_scale32(0.3)
    assert s.dtype == np.float32 and abs(float(s) - 1.0 / 0.7) <= 2.0 ** -24 * 2 and float(s) != 1.0 / 0.7


def test_bf16_rounding_is_round_to_nearest_even():
    a = np.array([1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, 1 + 2.0 ** -8 + 2.0 ** -20, -(1 + 2.0 ** -8), 256.0, 257.0, 259.0, 0.0, 3.0],
                 np.float32)
    want = np.array([1.0, 1 + 2.0 ** -6, 1 + 2.0 ** -7, -1.0, 256.0, 256.0, 260.0, 0.0, 3.0], np.float32)
    assert np.array_equal(R.bf16_round(a), want)
    ints = np.arange(-256, 257, dtype=np.float32)
    assert np.array_equal(R.bf16_round(ints), ints)              # what the integer regime relies on under GEMM_BF16
    g = R.gaussian_operands(4, 4, 16, 0)[0]
    r = R.bf16_round(g)
    assert np.all(r.view(np.uint32) & 0xFFFF == 0) and np.all(np.abs(r - g) <= 2.0 ** -8 * np.abs(g))
    assert not np.array_equal(r, g)


def all_integer_shapes():
    return R.INTEGER_SHAPES + R.EMPTY_BATCH_SHAPES


def test_integer_regime_is_exact_for_every_shape():
    for M, N, K in all_integer_shapes() + R.DROPOUT_SHAPES:
        assert R.integer_regime_exact(M, N, K), (M, N, K)
        c = R.integer_case(M, N, K)
        assert set(np.unique(c["x"])) <= {0.0, 1.0, 2.0, 3.0} and set(np.unique(c["w"])) <= {-2.0, -1.0, 0.0, 1.0, 2.0}
        assert np.abs(c["dy"]).max(initial=0) <= R.DY_MAX and np.abs(c["bias"]).max() <= R.B_MAX
        if M * K >= 64:
            assert 0.3 < (c["x"] == 0).mean() < 0.9 and (c["x"] == 3).any()      # real zeros, and the whole range
        for k in ("y", "y_relu", "dx", "dx_masked", "dw", "db"):
            assert R.is_small_integer(c[k]), (M, N, K, k)
            assert np.abs(c[k]).max(initial=0) <= R.partial_sum_limit(M, N, K)
        if M:
            assert (c["y"] < 0).any() or N * M < 4                               # the ReLU has something to do
            assert not np.array_equal(c["dx"], c["dx_masked"]) or M * K < 4
    # the dropout backward feeds h = 2 x (rate 0.5) to the weight gradient: still exact, by the predicate
    for M, N, K in R.DROPOUT_SHAPES:
        assert R.integer_regime_exact(M, N, K, x_max=2 * R.X_MAX)
        h, _ = R.dropout_ref(R.integer_case(M, N, K)["x"], 42, 0, 1, 0.5)
        assert R.is_small_integer(h) and h.max() == 2 * R.X_MAX and not R.is_small_integer(R.dropout_ref(h / 2, 42, 0, 1, 0.3)[0])
    assert not R.integer_regime_exact(64, 64, 2 ** 22) and not R.integer_regime_exact(2 ** 23, 16, 16)


def test_case_lists_cover_what_they_claim():
    shapes = R.INTEGER_SHAPES
    assert 28 <= len(shapes) <= 32 and len(set(shapes)) == len(shapes)
    for axis, values in ((0, R.M_VALUES), (1, R.N_VALUES), (2, R.K_VALUES)):
        assert {s[axis] for s in shapes} == set(values)
        for v in values:
            for other in {0, 1, 2} - {axis}:
                assert len({s[other] for s in shapes if s[axis] == v}) >= 2, (axis, v, other)
    assert [k // 16 for k in R.K_VALUES] == [1, 3, 5, 16, 17, 31, 32, 65]
    assert {-(-n // 16) for n in R.N_VALUES} >= {1, 4, 5, 9} and {-(-m // 16) for m in R.M_VALUES} >= {1, 4, 5, 17}
    assert all(m == 0 for m, _, _ in R.EMPTY_BATCH_SHAPES)
    assert {(64, 512, 512), (257, 512, 512), (17, 35, 128)} <= set(R.GAUSSIAN_SHAPES) and 8 <= len(R.GAUSSIAN_SHAPES) <= 12
    assert R.DROPOUT_SHAPES == [(17, 35, 128), (5, 11, 16), (64, 512, 512), (65, 130, 272)]
    for M, N, K in all_integer_shapes() + R.GAUSSIAN_SHAPES + R.DROPOUT_SHAPES:
        assert M <= R.MAX_SHAPE[0] and N <= R.MAX_SHAPE[1] and K <= R.MAX_SHAPE[2] and K % 16 == 0


def test_twin_masks_are_not_trivial_and_depend_on_step_layer_and_seed():
    for M, N, _ in R.DROPOUT_SHAPES:
        seen = {}
        for seed in R.DROPOUT_SEEDS:
            for layer in R.DROPOUT_LAYERS:
                for step in R.DROPOUT_STEPS:
                    for rate, lo, hi in ((0.3, 0.6, 0.8), (0.5, 0.4, 0.6)):
                        keep = ORNG.dropout_keep(seed, layer, step, M, N, rate)
                        if M * N >= 500:   # +-0.1 is 5.3 (rate 0.3) / 4.9 (rate 0.5) standard deviations at the smallest, 17x35
                            assert lo <= keep.mean() <= hi, (M, N, seed, layer, step, rate, keep.mean())
                        else:
                            assert keep.any() and not keep.all()
                        if rate == 0.3:
                            seen[(seed, layer, step)] = keep
                    # threshold 1 drops a draw of exactly 0 only: (nearly) everything is kept
                    assert ORNG.dropout_keep(seed, layer, step, M, N, R.SMALLEST_RATE).mean() > 0.999
        keys = list(seen)
        for i, a in enumerate(keys):
            for b in keys[i + 1:]:
                assert not np.array_equal(seen[a], seen[b]), (M, N, a, b)
        # a mask keyed by a padded row pitch is a different mask (what a ragged N is in the list for)
        if N % 16:
            Np = (N + 15) & ~15
            padded = ORNG.dropout_keep(42, 0, 0, M, Np, 0.3)[:, :N]
            assert not np.array_equal(padded, seen[(42, 0, 0)])


def test_float_bound_holds_for_a_float32_dot_product_in_three_orders():
    """The bound is order-free: a plain float32 matmul, a reversed-order one and a pairwise four-way split all stay inside."""
    M, N, K = 17, 35, 1040
    x, w, bias, _ = R.gaussian_operands(M, N, K, 9)
    ref, bound = R.fwd_ref(x, w, bias, 0), R.fwd_bound(x, w, bias)
    seq = np.zeros((M, N), np.float32)
    for k in range(K):
        seq += x[:, k:k + 1] * w[:, k][None, :]
    rev = np.zeros((M, N), np.float32)
    for k in reversed(range(K)):
        rev += x[:, k:k + 1] * w[:, k][None, :]
    quarters = sum((x[:, q::4] @ w[:, q::4].T for q in range(4)), np.zeros((M, N), np.float32))
    for got in (seq + bias, rev + bias, quarters + bias):
        assert got.dtype == np.float32 and np.all(np.abs(R.f64(got) - ref) <= bound)
    assert np.all(bound > 0) and bound.max() < 1e-3 * np.abs(ref).max()      # and it is a tight gate, not a loose one


def test_entry_points_are_declared_and_exported_and_the_abi_version_stays():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in _lib.DENSE_PROTOTYPES:
        assert name in declared and hasattr(L, name), name
    assert L.cmoop_abi_version() == 3
    hdr = open(_lib.HEADER).read()
    for name, value in (("FP32", R.GEMM_FP32), ("BF16", R.GEMM_BF16)):
        assert f"#define CMOOP_GEMM_{name} {value}" in hdr
    assert (_lib.GEMM_FP32, _lib.GEMM_BF16) == (R.GEMM_FP32, R.GEMM_BF16)


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = _lib.lib()
    z = C.c_void_p(0)
    assert L.cmoop_dense_fwd_ex(z, z, z, z, 0, 10, 16, 0, 7, 0.0, 0, 0, 0, z) != 0          # no such gemm mode
    assert b"gemm_mode" in L.cmoop_last_error()
    assert L.cmoop_dense_fwd_ex(z, z, z, z, 0, 10, 16, 0, R.GEMM_FP32, 1.0, 0, 0, 0, z) != 0
    assert b"dropout" in L.cmoop_last_error()
    assert L.cmoop_dense_fwd_ex(z, z, z, z, 0, 10, 16, 0, R.GEMM_FP32, -0.1, 0, 0, 0, z) != 0
    assert L.cmoop_dense_fwd_ex(z, z, z, z, 0, 10, 16, 0, R.GEMM_FP32, 0.3, 0, -1, 0, z) != 0
    assert L.cmoop_dense_bwd_ex(z, z, z, z, z, z, 0, 10, 16, 0, 1.0, 9, 1) != 0
