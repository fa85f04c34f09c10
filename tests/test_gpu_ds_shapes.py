"""GPU parity of the pointwise (1 x 1, stride 1) halves of the separable layers at H W > 1, through the trainer's launch path
(cmoop_conv_fwd_trainer / cmoop_conv_bwd_trainer) against float64, under the gates tests/test_gpu_production_shapes.py applies
to the full convolutions.  The cases are tests/_ds_shapes.py's; the host test (tests/test_dsnet_reference_cpu.py) holds that
list against every pointwise layer of the search space.  Each launch must be the one the host-only plan names."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import _lib

from _ds_shapes import DS_POINTWISE_CONVS

pytestmark = pytest.mark.gpu

ENV_MODE = os.environ.get("CMOOP_GEMM_MODE", "")
if ENV_MODE not in ("", "bf16x3"):
    pytest.skip("pointwise-shape parity is defined for the exact-fp32 product path (and the fp32-accurate bf16x3 mode)",
                allow_module_level=True)


def rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def plan(op, case, stats=0):
    buf = C.create_string_buffer(200)
    _lib.check(_lib.lib().cmoop_conv_launch_plan(op, *case, stats, buf, 200))
    return buf.value.decode()


@pytest.mark.parametrize("B,H,W,Cin,Cout,KS,stride", DS_POINTWISE_CONVS)
def test_pointwise_shapes_through_the_trainer_launch_path(B, H, W, Cin, Cout, KS, stride):
    assert (KS, stride) == (1, 1) and H * W > 1
    case = (B, H, W, Cin, Cout, KS, stride)
    L = _lib.lib()
    rs = np.random.RandomState(B + H + Cin + Cout)
    x = rs.randn(B, H, W, Cin).astype(np.float32)                          # a depthwise output: signed, no ReLU in front
    w = (rs.randn(Cout, 1, 1, Cin) / np.sqrt(Cin)).astype(np.float32)
    b = (0.1 * rs.randn(Cout)).astype(np.float32)
    dy = rs.randn(B, H, W, Cout).astype(np.float32)
    M = B * H * W
    x64, w64, dy64 = x.reshape(M, Cin).astype(np.float64), w.reshape(Cout, Cin).astype(np.float64), dy.reshape(M, Cout).astype(np.float64)
    ref_y = (x64 @ w64.T + b.astype(np.float64)).reshape(B, H, W, Cout)
    ref_dx = (dy64 @ w64).reshape(B, H, W, Cin)
    ref_dw = (dy64.T @ x64).reshape(Cout, 1, 1, Cin)
    ref_db = dy64.sum(0)
    xd, wd, bd, dyd = dev(x), dev(w), dev(b), dev(dy)
    # ---- forward (bias, no ReLU) with the BatchNorm statistics epilogue: the layer in front of a BatchNorm -------------------
    y = torch.full((B, H, W, Cout), float("nan"), device="cuda")
    cs, cq, fused = np.zeros(Cout), np.zeros(Cout), C.c_int32(-1)
    torch.cuda.synchronize()
    _lib.check(L.cmoop_conv_fwd_trainer(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), B, H, W, Cin, Cout, 1, 1, 0,
                                        _lib.ptr(cs), _lib.ptr(cq), C.byref(fused)))
    assert _lib.last_kernels() == [plan(0, case, 1)]
    yh = y.cpu().numpy()
    e_y = rel(yh, ref_y)
    y64 = yh.reshape(M, Cout).astype(np.float64)
    e_s = float(np.abs(cs - y64.sum(0)).max() / np.abs(y64).sum(0).max())
    e_q = float(np.abs(cq - (y64 ** 2).sum(0)).max() / (y64 ** 2).sum(0).max())
    # ---- the same launch without statistics and with ReLU (the nets without BatchNorm, topology B_ds) ------------------------
    y2 = torch.full_like(y, float("nan"))
    torch.cuda.synchronize()
    _lib.check(L.cmoop_conv_fwd_trainer(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y2), B, H, W, Cin, Cout, 1, 1, 1, None, None, None))
    assert _lib.last_kernels() == [plan(0, case, 0)]
    e_y2 = rel(y2.cpu().numpy(), np.maximum(ref_y, 0))
    # ---- backward: weight-gradient slabs + fixed-order sum, bias gradient, the unmasked data gradient ------------------------
    dx = torch.full((B, H, W, Cin), float("nan"), device="cuda")
    dw = torch.full((Cout, 1, 1, Cin), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    _lib.check(L.cmoop_conv_bwd_trainer(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(dyd), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                        B, H, W, Cin, Cout, 1, 1, 0))
    assert _lib.last_kernels() == [plan(2, case), plan(1, case)]
    e_dx, e_dw, e_db = rel(dx.cpu().numpy(), ref_dx), rel(dw.cpu().numpy(), ref_dw), rel(db.cpu().numpy(), ref_db)
    print(f"{case}: y {e_y:.1e} relu-y {e_y2:.1e} stats {e_s:.1e}/{e_q:.1e} (fused={fused.value}) dx {e_dx:.1e} dw {e_dw:.1e} db {e_db:.1e}")
    assert e_y < 2e-5 and e_y2 < 2e-5 and e_dx < 2e-5 and e_dw < 5e-5 and e_db < 5e-5
    assert fused.value in (0, 1) and e_s < 2e-6 and e_q < 2e-6
