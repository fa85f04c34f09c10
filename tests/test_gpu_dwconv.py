"""GPU parity of the depthwise convolution kernels (csrc/dwconv.hip) through the C ABI: forward, data gradient (masked and
unmasked) and weight gradient against the explicit float64 tap sums of tests/_dsnet_reference.py.

(a) integer regime: x, w, dy integers in [-4, 4] -- every fp32 sum is exact whatever its order (the largest, a weight
    gradient entry, is at most 16 B H W < 2^24), so the results equal the float64 restatement bit for bit;
(b) real-valued regime: |gpu - ref64| <= gamma_{n+2} sum|terms| + u |ref64| elementwise, u = 2^-24, gamma_m = m u / (1 - m u),
    n = K^2 (forward, data gradient) or B H W (weight gradient): the bound of ANY summation order of n fp32 products
    (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2), plus the rounding of the reference to fp32;
(c) the weight gradient's slices: two calls give the same bits, slice counts are positive, the trainer-sized slab holds them.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import _lib

import _dsnet_reference as R
from _ds_shapes import DS_DWCONVS

pytestmark = pytest.mark.gpu

CASES = [(1, 1, 1, 16, 3), (1, 1, 1, 16, 5), (2, 2, 3, 16, 5), (3, 7, 5, 32, 3), (3, 7, 5, 32, 5), (5, 26, 10, 64, 3),
         (2, 51, 20, 128, 5), (3, 101, 40, 16, 3), (1, 101, 40, 64, 5), (37, 13, 5, 256, 3), (2, 13, 5, 512, 5), (256, 13, 5, 512, 3)]
U = 2.0 ** -24


def gamma(m):
    return m * U / (1.0 - m * U)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).cuda()


def run(x, w, dy, mask_relu):
    """-> y, dx, dw of the library for host arrays"""
    B, H, W, Cn = x.shape
    K = w.shape[0]
    L = _lib.lib()
    xd, wd, dyd = dev(x), dev(w), dev(dy)
    y = torch.full((B, H, W, Cn), float("nan"), device="cuda")
    dx = torch.full((B, H, W, Cn), float("nan"), device="cuda")
    dw = torch.full((K, K, Cn), float("nan"), device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cmoop_dwconv_fwd(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(y), B, H, W, Cn, K))
    _lib.check(L.cmoop_dwconv_bwd(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(dyd), _lib.ptr(dx), _lib.ptr(dw), B, H, W, Cn, K, int(mask_relu)))
    return y.cpu().numpy(), dx.cpu().numpy(), dw.cpu().numpy()


def integers(B, H, W, Cn, K, seed):
    rs = np.random.RandomState(seed)
    return (rs.randint(-4, 5, (B, H, W, Cn)).astype(np.float32), rs.randint(-4, 5, (K, K, Cn)).astype(np.float32),
            rs.randint(-4, 5, (B, H, W, Cn)).astype(np.float32))


def check_exact(B, H, W, Cn, K):
    assert 16 * B * H * W < 2 ** 24
    x, w, dy = integers(B, H, W, Cn, K, B + H + Cn + K)
    ref_y, ref_dx, ref_dw = R.dw_forward64(x, w), R.dw_dgrad64(dy, w), R.dw_wgrad64(x, dy, K)
    y, dx, dw = run(x, w, dy, mask_relu=False)
    assert np.array_equal(y.astype(np.float64), ref_y)
    assert np.array_equal(dx.astype(np.float64), ref_dx)
    assert np.array_equal(dw.astype(np.float64), ref_dw)
    _, dxm, dwm = run(x, w, dy, mask_relu=True)
    assert np.array_equal(dxm.astype(np.float64), ref_dx * (x > 0))
    assert np.array_equal(dwm, dw)


@pytest.mark.parametrize("B,H,W,Cn,K", CASES)
def test_exact_regime_equals_float64_bit_for_bit(B, H, W, Cn, K):
    check_exact(B, H, W, Cn, K)


def test_exact_regime_on_every_depthwise_geometry_of_the_search_space():
    """each (H, W, C, K) of tests/_ds_shapes.py at batch 3: images that split into several row runs at every stage"""
    for (H, W, Cn, K) in DS_DWCONVS:
        check_exact(3, H, W, Cn, K)


@pytest.mark.parametrize("B,H,W,Cn,K", CASES)
def test_real_valued_regime_within_the_summation_bound(B, H, W, Cn, K):
    rs = np.random.RandomState(B * 7 + H + Cn + K)
    x = rs.randn(B, H, W, Cn).astype(np.float32)
    w = rs.randn(K, K, Cn).astype(np.float32)
    dy = rs.randn(B, H, W, Cn).astype(np.float32)
    y, dx, dw = run(x, w, dy, mask_relu=True)
    worst = {}
    for name, got, ref, mag, n in (
            ("y", y, R.dw_forward64(x, w), R.dw_forward64(x, w, absolute=True), K * K),
            ("dx", dx, R.dw_dgrad64(dy, w) * (x > 0), R.dw_dgrad64(dy, w, absolute=True), K * K),
            ("dw", dw, R.dw_wgrad64(x, dy, K), R.dw_wgrad64(x, dy, K, absolute=True), B * H * W)):
        bound = gamma(n + 2) * mag + U * np.abs(ref)
        err = np.abs(got.astype(np.float64) - ref)
        worst[name] = float((err / np.maximum(bound, 1e-300)).max())
        print(f"{(B, H, W, Cn, K)} {name}: max err {err.max():.3e}, worst err / bound {worst[name]:.3f}")
        assert np.isfinite(got).all()
    assert max(worst.values()) <= 1.0, worst


def test_weight_gradient_is_reproducible_and_its_slices_fit_the_trainer_slab():
    B, H, W, Cn, K = 37, 26, 10, 64, 5
    rs = np.random.RandomState(0)
    x, w, dy = (rs.randn(B, H, W, Cn).astype(np.float32), rs.randn(K, K, Cn).astype(np.float32), rs.randn(B, H, W, Cn).astype(np.float32))
    _, dx1, dw1 = run(x, w, dy, mask_relu=True)
    _, dx2, dw2 = run(x, w, dy, mask_relu=True)
    assert np.array_equal(dw1, dw2) and np.array_equal(dx1, dx2)
    for (H, W, Cn, K) in ((101, 40, 16, 3), (13, 5, 512, 5)):
        s = [_lib.dwconv_wgrad_slices(b, H, W, Cn, K) for b in range(1, 65)]
        assert min(s) >= 1
        # the trainer sizes a layer's slab region as the maximum over the train batches 1..cfg.batch of slices K^2 C: the
        # region of a batch-64 net holds every partial batch, one sized for the full batch alone need not (not monotone)
        slab = max(s) * K * K * Cn
        assert all(v * K * K * Cn <= slab for v in s)
        print(f"{(H, W, Cn, K)}: slices at batch 64 {s[63]}, most {max(s)} at batch {1 + int(np.argmax(s))}")


def test_bad_shapes_fail_loudly():
    L = _lib.lib()
    t = torch.zeros(16 * 24, device="cuda")
    assert L.cmoop_dwconv_fwd(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 1, 4, 4, 24, 3) != 0
    assert L.cmoop_dwconv_fwd(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 1, 4, 4, 16, 4) != 0
    assert L.cmoop_dwconv_bwd(_lib.ptr(t), _lib.ptr(t), _lib.ptr(t), None, None, 1, 4, 4, 16, 3, 0) != 0
