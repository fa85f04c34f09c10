"""GPU parity of the conv launch paths ACROSS THE GEOMETRIES AND BATCHES THE LAUNCHERS BRANCH ON, bit for bit.

Every conv kernel that carries training time is chosen per launch by host arithmetic on (B, H, W, Cin, Cout, KS, stride).
tests/_sweep_shapes.py lists cases that witness every launch-path variant of the domain (seven feature sizes, train batch
1..64, the inference batches) on every edge it can sit on -- ragged last tile, one image, tiles that hold whole images, odd
widths, windows larger than the image, halo tiles whose LDS row bound is exactly tight -- and the host test
test_geometry_sweep_covers_every_variant_and_edge_of_the_domain keeps that list complete.  Here each case runs through the
trainer's own launch path (cmoop_conv_fwd_trainer with and without the statistics epilogue / ReLU, cmoop_conv_bwd_trainer
with the ReLU mask) against oracle.net.conv_same + autograd in float64, in two regimes:

* integer: x in {0..3} (a ReLU output with real zeros), w and dy in {-2..2}, bias in {-4..4}.  Every product and every
  partial sum is an integer below 2^24 (asserted from the shape), so y, ReLU(y), dx, dw and db must EQUAL the float64
  reference whatever the kernel, the split, the slab order or the arithmetic mode: no tolerance.  The module re-runs this
  regime in child processes under CMOOP_GEMM_MODE=bf16x3, =bf16 (small integers are exact in bf16) and with the halo kernels
  switched off.
* gaussian (the sweep cases; the production shapes have it in tests/test_gpu_production_shapes.py): full-mantissa operands
  at that module's gates -- forward and dgrad 2e-5, weight and bias gradient 5e-5 of the tensor's max.

The fused BatchNorm statistics keep 2e-6 of the column's float64 sum of what the kernel stored in both regimes (their fp32
per-tile partials of squares can leave the exact range).  x, w, dy, y and dx live inside larger device tensors between
NaN guards: the outputs' guards must come back bit-unchanged, every payload element finite, and a stray read next to an
operand turns a result into NaN.  A CmoopError, any other runtime error of a device call (an asynchronous fault surfaces
in the next copy) or a child process that ends abnormally or not at all stops the module: later cases skip and no further
child process is started, with or without -x.  Run it with -x under a time limit (about 1 min of cases and 2.5 min of child
processes on one MI355X); a device error met here is a finding to diagnose from the printed case and kernel names, not
something to re-run.
"""
import ctypes as C
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import _lib
from oracle.net import conv_same

from _production_shapes import PRODUCTION_CONVS
from _sweep_shapes import SWEEP_CONVS, integer_regime_is_exact

pytestmark = pytest.mark.gpu

ENV_MODE = os.environ.get("CMOOP_GEMM_MODE", "")
IS_CHILD = os.environ.get("CMOOP_SWEEP_CHILD", "") == "1"
parent_only = pytest.mark.skipif(IS_CHILD or ENV_MODE != "", reason="runs the other modes in child processes of the default-mode run")

NAN_BITS = 0x7FC0F00D                 # a quiet NaN with a recognisable payload
#: set by the first CmoopError: what failed; every later case skips, the child processes are not started
DEVICE_ERROR = []
#: launch-path variants the GPU really launched / the host plan promised, per module run; worst gaussian error per variant
LAUNCHED, PLANNED, WORST = set(), set(), {}
T0 = [None, 0]

CASES = [("integer", c) for c in SWEEP_CONVS + PRODUCTION_CONVS] + [("gaussian", c) for c in SWEEP_CONVS]


def _plan(op, c, stats=0):
    buf = C.create_string_buffer(200)
    _lib.check(_lib.lib().cmoop_conv_launch_plan(op, *c, stats, buf, 200))
    return buf.value.decode()


def _operands(regime, B, H, W, Cin, Cout, KS, stride, seed):
    rs = np.random.RandomState(seed)
    OH, OW = -(-H // stride), -(-W // stride)
    if regime == "integer":
        x = rs.randint(0, 4, (B, H, W, Cin)).astype(np.float32)
        w = rs.randint(-2, 3, (Cout, KS, KS, Cin)).astype(np.float32)
        b = rs.randint(-4, 5, Cout).astype(np.float32)
        dy = rs.randint(-2, 3, (B, OH, OW, Cout)).astype(np.float32)
    else:                             # tests/test_gpu_production_shapes.py::_conv_case_ref's data
        x = np.maximum(rs.randn(B, H, W, Cin), 0).astype(np.float32)
        w = (rs.randn(Cout, KS, KS, Cin) / np.sqrt(KS * KS * Cin)).astype(np.float32)
        b = (0.1 * rs.randn(Cout)).astype(np.float32)
        dy = rs.randn(B, OH, OW, Cout).astype(np.float32)
    return x, w, b, dy


def _reference(x, w, b, dy, stride):
    xt = torch.from_numpy(x).double().permute(0, 3, 1, 2).requires_grad_(True)
    wt = torch.from_numpy(w).double().requires_grad_(True)
    bt = torch.from_numpy(b).double().requires_grad_(True)
    y = conv_same(xt, wt, bt, stride)
    y.backward(torch.from_numpy(dy).double().permute(0, 3, 1, 2))
    return dict(y=y.detach().permute(0, 2, 3, 1).numpy(), dx=xt.grad.permute(0, 2, 3, 1).numpy() * (x > 0),
                dw=wt.grad.numpy(), db=bt.grad.numpy())


def _guarded(n, guard, payload=None):
    """A device tensor of guard + n + guard floats, all NAN_BITS, and the n-float view in its middle (filled from payload)."""
    buf = torch.empty(guard + n + guard, dtype=torch.float32, device="cuda")
    buf.view(torch.int32).fill_(NAN_BITS)
    mid = buf[guard:guard + n]
    if payload is not None:
        mid.copy_(torch.from_numpy(np.ascontiguousarray(payload).reshape(-1)))
    return buf, mid


def _guards_intact(buf, guard, n):
    bits = buf.view(torch.int32)
    return bool((bits[:guard] == NAN_BITS).all()) and bool((bits[guard + n:] == NAN_BITS).all())


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.abs(a - b).max() / (np.abs(b).max() + 1e-300))


def _call(what, case, rc_fn):
    """Run one library call; a CmoopError stops the module (later cases skip, no child process starts)."""
    try:
        _lib.check(rc_fn())
    except _lib.CmoopError as e:
        DEVICE_ERROR.append(f"{what} of {case}: {e}")
        raise


def _id(p):
    return p if isinstance(p, str) else "x".join(map(str, p))


@pytest.mark.parametrize("regime,case", CASES, ids=_id)
def test_sweep_conv_through_the_trainer_launch_path(regime, case):
    if DEVICE_ERROR:
        pytest.skip(f"stopped at the first device error: {DEVICE_ERROR[0]}")
    if regime == "gaussian" and ENV_MODE not in ("", "bf16x3"):
        pytest.skip("the gaussian regime is defined for the exact-fp32 product path and the fp32-accurate bf16x3 mode")
    try:
        _run_case(regime, case)
    except RuntimeError as e:         # CmoopError (recorded by _call) or a fault torch meets in a later copy / reduction
        if not DEVICE_ERROR:
            DEVICE_ERROR.append(f"{regime} {case}: {type(e).__name__}: {e}")
        raise


def _run_case(regime, case):
    if T0[0] is None:
        T0[0] = time.time()
    B, H, W, Cin, Cout, KS, stride = case
    L = _lib.lib()
    OH, OW = -(-H // stride), -(-W // stride)
    M = B * OH * OW
    if regime == "integer":           # the bounds that make every partial sum an exact fp32 integer, from the shape alone
        assert integer_regime_is_exact(*case)
    x, w, b, dy = _operands(regime, *case, seed=B + H + Cin + Cout + KS + (1000 if regime == "integer" else 0))
    ref = _reference(x, w, b, dy, stride)
    if regime == "integer":
        for k, v in ref.items():      # the reference itself: integer-valued, exactly representable in fp32
            assert np.array_equal(v, np.rint(v)) and np.abs(v).max() < 2 ** 24, k
    G = 256 * max(Cin, Cout)
    ny, nx = M * Cout, B * H * W * Cin
    xb, xd = _guarded(nx, G, x)
    wb, wd = _guarded(w.size, G, w)
    dyb, dyd = _guarded(ny, G, dy)
    bd = torch.from_numpy(b).cuda()
    planned = {_plan(0, case, 1), _plan(0, case, 0), _plan(1, case), _plan(2, case)}
    # ---- forward (bias, no ReLU) with the BatchNorm statistics epilogue ---------------------------------------------
    yb, y = _guarded(ny, G)
    cs, cq, fused = np.zeros(Cout), np.zeros(Cout), C.c_int32(-1)
    torch.cuda.synchronize()
    _call("forward+stats", case, lambda: L.cmoop_conv_fwd_trainer(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y), B, H, W, Cin, Cout,
                                                                  KS, stride, 0, _lib.ptr(cs), _lib.ptr(cq), C.byref(fused)))
    fwd_names = _lib.last_kernels()
    names = list(fwd_names)
    assert _guards_intact(yb, G, ny), f"forward+stats wrote outside y {names}"
    assert bool(torch.isfinite(y).all()), f"forward+stats left elements of y unwritten or read a NaN guard {names}"
    yh = y.cpu().numpy().reshape(B, OH, OW, Cout)
    y64 = yh.reshape(M, Cout).astype(np.float64)
    e_s = float(np.abs(cs - y64.sum(0)).max() / np.abs(y64).sum(0).max())
    e_q = float(np.abs(cq - (y64 ** 2).sum(0)).max() / (y64 ** 2).sum(0).max())
    # ---- the same launch without statistics and with ReLU (the no-BatchNorm nets) ------------------------------------
    y2b, y2 = _guarded(ny, G)
    torch.cuda.synchronize()
    _call("forward+relu", case, lambda: L.cmoop_conv_fwd_trainer(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(bd), _lib.ptr(y2), B, H, W, Cin, Cout,
                                                                 KS, stride, 1, None, None, None))
    relu_names = _lib.last_kernels()
    names += relu_names
    assert _guards_intact(y2b, G, ny), f"forward+relu wrote outside y {names}"
    assert bool(torch.isfinite(y2).all()), f"forward+relu left elements of y unwritten or read a NaN guard {names}"
    y2h = y2.cpu().numpy().reshape(B, OH, OW, Cout)
    # ---- backward: dgrad with the ReLU mask of the input, wgrad (slabs or in place), bias gradient -------------------
    dxb, dx = _guarded(nx, G)
    dw = torch.full((Cout, KS, KS, Cin), float("nan"), device="cuda")
    db = torch.full((Cout,), float("nan"), device="cuda")
    torch.cuda.synchronize()
    _call("backward", case, lambda: L.cmoop_conv_bwd_trainer(_lib.ptr(xd), _lib.ptr(wd), _lib.ptr(dyd), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                                             B, H, W, Cin, Cout, KS, stride, 1))
    bwd_names = _lib.last_kernels()
    names += bwd_names
    assert _guards_intact(dxb, G, nx), f"backward wrote outside dx {bwd_names}"
    assert bool(torch.isfinite(dx).all()), f"backward left elements of dx unwritten or read a NaN guard {bwd_names}"
    for buf, n, nm in ((xb, nx, "x"), (wb, w.size, "w"), (dyb, ny, "dy")):
        assert _guards_intact(buf, G, n), f"an operand's guard changed: {nm} {names}"
    dxh, dwh, dbh = dx.cpu().numpy().reshape(B, H, W, Cin), dw.cpu().numpy(), db.cpu().numpy()
    got = dict(y=yh, relu_y=y2h, dx=dxh, dw=dwh, db=dbh)
    want = dict(ref, relu_y=np.maximum(ref["y"], 0))
    err = {k: _rel(got[k], want[k]) for k in got}
    wrong = {k: int((got[k].astype(np.float64) != want[k]).sum()) for k in got}
    print(f"{regime} {case}: " + " ".join(f"{k} {err[k]:.1e}" + (f" ({wrong[k]} differ)" if regime == "integer" else "") for k in got)
          + f" stats {e_s:.1e}/{e_q:.1e} (fused={fused.value})  {sorted(set(names))}")
    T0[1] = time.time() - T0[0]
    assert fused.value in (0, 1) and e_s < 2e-6 and e_q < 2e-6
    if regime == "integer":
        for k in got:
            assert np.array_equal(got[k].astype(np.float64), want[k]), (k, wrong[k], err[k], sorted(set(names)))
    else:
        assert err["y"] < 2e-5 and err["relu_y"] < 2e-5 and err["dx"] < 2e-5 and err["dw"] < 5e-5 and err["db"] < 5e-5, err
        # per launch: each call reports its own kernels; the backward call's are the weight gradient (dw, db) and the dgrad (dx)
        for ns, e in ((fwd_names, err["y"]), (relu_names, err["relu_y"]),
                      ([n for n in bwd_names if "wgrad" in n], max(err["dw"], err["db"])),
                      ([n for n in bwd_names if "wgrad" not in n], err["dx"])):
            for n in ns:
                WORST[n] = max(WORST.get(n, 0.0), e)
    LAUNCHED.update(names)
    PLANNED.update(planned)


def test_the_gpu_launched_every_variant_the_host_plan_promised():
    """The host coverage test reasons about cmoop_conv_launch_plan; the launches themselves report their variant through
    cmoop_last_kernels.  Over the whole list the names really launched must contain every name the plan gave, so that the
    CPU-side coverage and the GPU agree on what was run."""
    if DEVICE_ERROR:
        pytest.skip(f"stopped at the first device error: {DEVICE_ERROR[0]}")
    if not PLANNED:
        pytest.skip("run together with the sweep cases of this module (they fill the launch sets)")
    print(f"{len(LAUNCHED)} launch-path variants launched, {len(PLANNED)} planned; cases of this module took {T0[1]:.1f} s")
    for n in sorted(WORST):
        print(f"worst gaussian-regime error  {WORST[n]:.2e}  {n}")
    assert not sorted(PLANNED - LAUNCHED), f"planned by the host, never launched on the GPU: {sorted(PLANNED - LAUNCHED)}"


def _child(env_extra, select, n_cases, timeout):
    if DEVICE_ERROR:
        pytest.skip(f"stopped at the first device error: {DEVICE_ERROR[0]}")
    env = dict(os.environ, CMOOP_SWEEP_CHILD="1", **env_extra)
    try:
        r = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-q", "-x", "-k", select],
                           capture_output=True, text=True, env=env, timeout=timeout)
    except subprocess.TimeoutExpired:
        DEVICE_ERROR.append(f"child process {env_extra} did not end within {timeout} s")
        raise
    if r.returncode not in (0, 1) or "CmoopError" in r.stdout or "RuntimeError" in r.stdout:
        DEVICE_ERROR.append(f"child process {env_extra} ended with status {r.returncode}")
    assert r.returncode == 0 and f"{n_cases} passed" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]


N_INT, N_ALL = len(SWEEP_CONVS) + len(PRODUCTION_CONVS), len(CASES)


@parent_only
def test_integer_regime_is_exact_under_the_bf16x3_mode_and_the_gaussian_regime_holds_its_gates():
    """CMOOP_GEMM_MODE is read once per process: the whole list again in a child, both regimes (a small integer splits into
    one bf16 term and two zeros: exact; the gaussian regime at the exact path's gates, as the production shapes)."""
    _child(dict(CMOOP_GEMM_MODE="bf16x3"), "trainer_launch_path", N_ALL, 1100)


@parent_only
def test_integer_regime_is_exact_under_the_bf16_mode():
    """Operands rounded to bf16, fp32 accumulation: integers up to 256 are exact in bf16, so nothing may differ."""
    _child(dict(CMOOP_GEMM_MODE="bf16"), "trainer_launch_path and integer", N_INT, 900)


@parent_only
def test_integer_regime_is_exact_with_the_halo_kernels_switched_off():
    """CMOOP_HALO / CMOOP_HALO_WGRAD / CMOOP_HALO_BAL = 0: the implicit-GEMM fall-backs of every halo layer, same oracle."""
    _child(dict(CMOOP_HALO="0", CMOOP_HALO_WGRAD="0", CMOOP_HALO_BAL="0"), "trainer_launch_path and integer", N_INT, 900)
