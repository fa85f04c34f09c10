"""GPU parity of the MLP-head kernels of csrc/dense.hip (dense_fwd_kernel with its dropout epilogue in both key forms,
dense_dgrad_kernel with the mask scale, dense_wgrad_kernel, the merged dense_bwd_kernel), launched through
cmoop_dense_fwd_ex / cmoop_dense_bwd_ex with the trainer's own argument lists, against the float64 references of
tests/_dense_reference.py and the dropout twin oracle/rng.py::dropout_keep.

INTEGER regime: x in {0..3}, w and dy in {-2..2}, bias in {-4..4}; every partial sum is an integer below 2^24
(_dense_reference.integer_regime_exact, asserted per case), so each fp32 add is exact in any order and the device result must
EQUAL the float64 reference -- under GEMM_BF16 too (integers up to 256 are exact in bf16), merged and as two launches.
GAUSSIAN regime: |err| <= (n + 8) 2^-24 (sum |a_i||b_i| + |bias|) per element (_dense_reference.dot_bound: forward error
analysis, not a measured number), the reference's operands rounded to bf16 first under GEMM_BF16.
DROPOUT: integer regime again, so the mask AND the scaled values are exact against the independent twin.

Every operand lies between NaN guard bands (a read outside the tensor poisons the result), every output is NaN-filled
inside a sentinel-filled buffer (an unwritten element stays NaN, a write outside the tensor breaks a sentinel); operands and
guards are compared bit for bit after the launches of a case.  Run with -s for the per-case figures
(profiles/dense_head_parity.txt is one such run)."""
import ctypes as C

import numpy as np
import pytest
import torch

import _dense_reference as R
from cmoop_audio_processing_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64                                   # floats on either side: 256 bytes, keeps the float4 loads of x / w rows aligned
SENTINEL = np.float32(-777.25)


def L():
    return _lib.lib()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def sid(shape):
    return "x".join(str(v) for v in shape)


class Operand:
    """A read-only tensor between two NaN guard bands of one device buffer."""

    def __init__(self, a):
        a = np.ascontiguousarray(a, np.float32)
        self.host = np.full(a.size + 2 * GUARD, np.nan, np.float32)
        self.host[GUARD:GUARD + a.size] = a.ravel()
        self.dev = torch.from_numpy(self.host).cuda()
        self.ptr = C.c_void_p(self.dev.data_ptr() + 4 * GUARD)

    def intact(self):
        return np.array_equal(bits(self.dev.cpu().numpy()), bits(self.host))


class Output:
    """A NaN-filled tensor between two sentinel-filled guard bands of one device buffer."""

    def __init__(self, *shape):
        self.shape, self.n = shape, int(np.prod(shape))
        host = np.full(self.n + 2 * GUARD, SENTINEL, np.float32)
        host[GUARD:GUARD + self.n] = np.nan
        self.dev = torch.from_numpy(host).cuda()
        self.ptr = C.c_void_p(self.dev.data_ptr() + 4 * GUARD)

    def read(self, untouched=False):
        """The tensor, after asserting the guards intact and (unless untouched is expected) every element written."""
        buf = self.dev.cpu().numpy()
        guards = np.concatenate([buf[:GUARD], buf[GUARD + self.n:]])
        assert np.array_equal(bits(guards), bits(np.full(2 * GUARD, SENTINEL, np.float32))), "write outside the output tensor"
        out = buf[GUARD:GUARD + self.n].reshape(self.shape)
        if untouched:
            assert np.array_equal(bits(out), bits(np.full(self.shape, np.nan, np.float32))), "output written by an empty launch"
        else:
            assert not np.isnan(out).any(), f"{int(np.isnan(out).sum())} output elements left unwritten (or NaN)"
        return out


def ok(rc):
    torch.cuda.synchronize()
    _lib.check(rc)


def fwd(x, w, bias, M, N, K, relu, mode, rate=0.0, seed=0, layer=0, step=0, state=None, rows=None):
    y = Output(M if rows is None else rows, N)
    ok(L().cmoop_dense_fwd_ex(x.ptr, w.ptr, bias.ptr, y.ptr, M, N, K, relu, mode, rate, seed, layer, step,
                              None if state is None else _lib.ptr(state)))
    return y


def bwd(x, w, dy, M, N, K, mask, scale, mode, merged, rows=None):
    dx, dw, db = Output(M if rows is None else rows, K), Output(N, K), Output(N)
    ok(L().cmoop_dense_bwd_ex(x.ptr, w.ptr, dy.ptr, dx.ptr, dw.ptr, db.ptr, M, N, K, mask, float(scale), mode, merged))
    return dx, dw, db


def differing(gpu, ref):
    """Number of elements that do not EQUAL the reference cast to float32 (a NaN differs; the sign of a zero does not)."""
    return int(np.count_nonzero(~(np.asarray(gpu, np.float32) == np.asarray(ref, np.float64).astype(np.float32))))


def ratio(gpu, ref64, bound):
    """Worst |gpu - ref| / bound over the tensor; an element with a zero bound must be exact (ratio 0) or counts as inf."""
    err = np.abs(np.asarray(gpu, np.float64) - np.asarray(ref64, np.float64))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(err == 0.0, 0.0, err / np.asarray(bound, np.float64))
    return float(q.max()) if q.size else 0.0


LAUNCHES = ((1, "merged"), (0, "two launches"))


# ---- a. the integer regime --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", R.INTEGER_SHAPES, ids=[sid(s) for s in R.INTEGER_SHAPES])
def test_integer_regime_equals_the_float64_reference(M, N, K):
    """y, relu(y), dx with and without the (x > 0) mask, dw and db EQUAL the float64 reference: fp32 and GEMM_BF16, the
    backward merged and as two launches.  The K / 16, ceil(N / 16) and ceil(M / 16) of the list walk every edge of the three
    wave-strided reduction loops (a lone wave, ragged trips, a second trip of wave 0 only, a third trip)."""
    assert R.integer_regime_exact(M, N, K)
    c = R.integer_case(M, N, K)
    x, w, bias, dy = (Operand(c[k]) for k in ("x", "w", "bias", "dy"))
    total = 0
    print(f"\n  integer {M}x{N}x{K}  K/16={K // 16} n-groups={-(-N // 16)} m-groups={-(-M // 16)}")
    for mode, mname in R.MODES:
        d = {"y": differing(fwd(x, w, bias, M, N, K, 0, mode).read(), c["y"]),
             "relu(y)": differing(fwd(x, w, bias, M, N, K, 1, mode).read(), c["y_relu"])}
        print(f"    {mname} forward: differing elements " + "  ".join(f"{k} {v}" for k, v in d.items()))
        total += sum(d.values())
        for merged, lname in LAUNCHES:
            d = {}
            for mask, key in ((0, "dx"), (1, "dx_masked")):
                dx, dw, db = bwd(x, w, dy, M, N, K, mask, 1.0, mode, merged)
                d[key] = differing(dx.read(), c[key])
                d[f"dw({key})"] = differing(dw.read(), c["dw"])
                d[f"db({key})"] = differing(db.read(), c["db"])
            print(f"    {mname} backward, {lname}: differing elements " + "  ".join(f"{k} {v}" for k, v in d.items()))
            total += sum(d.values())
    assert all(o.intact() for o in (x, w, bias, dy)), "an operand or its guard band was written"
    assert total == 0, f"{total} elements differ from the float64 reference"


@pytest.mark.parametrize("M,N,K", R.EMPTY_BATCH_SHAPES, ids=[sid(s) for s in R.EMPTY_BATCH_SHAPES])
def test_empty_batch(M, N, K):
    """M = 0: dw and db exactly zero, y and dx untouched, no launch error (dense.hip makes no load)."""
    c = R.integer_case(M, N, K)
    x, w, bias, dy = (Operand(c[k]) for k in ("x", "w", "bias", "dy"))
    for mode, mname in R.MODES:
        fwd(x, w, bias, 0, N, K, 1, mode, rows=16).read(untouched=True)
        fwd(x, w, bias, 0, N, K, 1, mode, rate=0.3, seed=1, layer=0, step=2, rows=16).read(untouched=True)
        for merged, lname in LAUNCHES:
            dx, dw, db = bwd(x, w, dy, 0, N, K, 1, 1.0, mode, merged, rows=16)
            dx.read(untouched=True)
            nz = int(np.count_nonzero(dw.read())) + int(np.count_nonzero(db.read()))
            print(f"\n  empty batch 0x{N}x{K} {mname} {lname}: non-zero dw / db elements {nz}", end="")
            assert nz == 0
    assert all(o.intact() for o in (x, w, bias, dy))


# ---- b. the gaussian regime -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,K", R.GAUSSIAN_SHAPES, ids=[sid(s) for s in R.GAUSSIAN_SHAPES])
def test_gaussian_regime_within_the_per_element_bound(M, N, K):
    """|err| <= (n + 8) 2^-24 (sum |a_i||b_i| + |bias|) for every element, n = K (forward), N (dgrad), M (wgrad, db); under
    GEMM_BF16 against the reference of the bf16-rounded operands with the same bound.  The merged launch and the two
    launches must agree bit for bit."""
    xh, wh, bh, dyh = R.gaussian_operands(M, N, K, R.shape_seed(M, N, K))
    x, w, bias, dy = (Operand(a) for a in (xh, wh, bh, dyh))
    worst_all = 0.0
    print(f"\n  gaussian {M}x{N}x{K}")
    for mode, mname in R.MODES:
        fb = R.fwd_bound(xh, wh, bh, mode)
        q = {"y": [ratio(fwd(x, w, bias, M, N, K, 0, mode).read(), R.fwd_ref(xh, wh, bh, 0, mode), fb)],
             "relu(y)": [ratio(fwd(x, w, bias, M, N, K, 1, mode).read(), R.fwd_ref(xh, wh, bh, 1, mode), fb)],
             "dx": [], "dw": [], "db": []}
        dgb, wgb, dbb = R.dgrad_bound(dyh, wh, 1.0, mode), R.wgrad_bound(xh, dyh, mode), R.db_bound(dyh)
        dw_ref, db_ref = R.wgrad_ref(xh, dyh, mode)
        got = {}
        for merged, lname in LAUNCHES:
            for mask in (0, 1):
                dx, dw, db = (o.read() for o in bwd(x, w, dy, M, N, K, mask, 1.0, mode, merged))
                got[(merged, mask)] = (dx, dw, db)
                q["dx"].append(ratio(dx, R.dgrad_ref(dyh, wh, xh if mask else None, 1.0, mode), dgb))
                q["dw"].append(ratio(dw, dw_ref, wgb))
                q["db"].append(ratio(db, db_ref, dbb))
        for mask in (0, 1):
            for a, b in zip(got[(1, mask)], got[(0, mask)]):
                assert np.array_equal(bits(a), bits(b)), f"{mname} mask={mask}: the merged launch and the two launches differ"
        worst = {k: max(v) for k, v in q.items()}
        print(f"    {mname}: worst err/bound  " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items()))
        assert all(v < 1.0 for v in worst.values()), f"{mname}: beyond the bound: {worst}"
        worst_all = max(worst_all, max(worst.values()))
    assert all(o.intact() for o in (x, w, bias, dy))
    assert worst_all < 1.0


# ---- c. dropout against the twin --------------------------------------------------------------------------------------------
def rate_name(rate):
    return "2^-24" if rate == R.SMALLEST_RATE else str(rate)


@pytest.mark.parametrize("M,N,K", R.DROPOUT_SHAPES, ids=[sid(s) for s in R.DROPOUT_SHAPES])
def test_dropout_host_prefix_equals_the_twin(M, N, K):
    """Host-prefix form: for every rate, layer, seed and step the output EQUALS where(keep, fl32(relu(y) * fl32(scale)), 0)
    with keep from oracle.rng.dropout_keep and y the float64 integer reference (fp32 and GEMM_BF16); without the ReLU too."""
    c = R.integer_case(M, N, K)
    x, w, bias = (Operand(c[k]) for k in ("x", "w", "bias"))
    total = launches = 0
    print(f"\n  dropout, host prefix, {M}x{N} (K={K})")
    for rate in R.DROPOUT_RATES:
        n_bad, kept = 0, []
        for layer in R.DROPOUT_LAYERS:
            for seed in R.DROPOUT_SEEDS:
                for step in R.DROPOUT_STEPS:
                    for relu in ((1, 0) if step == 0 else (1,)):
                        ref, keep = R.dropout_ref(c["y_relu"] if relu else c["y"], seed, layer, step, rate)
                        kept.append(keep.mean())
                        for mode, _ in R.MODES:
                            got = fwd(x, w, bias, M, N, K, relu, mode, rate, seed, layer, step).read()
                            n_bad += differing(got, ref)
                            launches += 1
        print(f"    rate {rate_name(rate)} scale {float(R.keep_scale32(rate)):.9g}: kept share {min(kept):.3f}..{max(kept):.3f}, "
              f"differing elements {n_bad}")
        total += n_bad
    assert all(o.intact() for o in (x, w, bias))
    assert total == 0, f"{total} elements differ from the twin over {launches} launches"


@pytest.mark.parametrize("M,N,K", R.DROPOUT_SHAPES, ids=[sid(s) for s in R.DROPOUT_SHAPES])
def test_dropout_device_state_reads_the_step_from_device_memory(M, N, K):
    """Device-state form: the same host arguments for every launch (host step 777), a 16-byte StepState written from here
    with step in {0, 1, 12345} and junk in row0 / iter; each launch must give the mask of the step in device memory: EQUAL
    to the twin's, and bit-equal to the host-prefix form's output for that step."""
    c = R.integer_case(M, N, K)
    x, w, bias = (Operand(c[k]) for k in ("x", "w", "bias"))
    total = 0
    host_step = 777
    print(f"\n  dropout, device step state, {M}x{N} (K={K})")
    for rate in R.DROPOUT_RATES:
        n_bad = 0
        for layer in R.DROPOUT_LAYERS:
            for seed in R.DROPOUT_SEEDS:
                for i, step in enumerate(R.DROPOUT_STEPS):
                    words = np.array([0x9ABCDEF0 + i, 0x12345678, step, 0xCAFE0000 + 31 * i], np.uint32)   # row0 lo, hi, step, iter
                    state = torch.from_numpy(words.view(np.int32).copy()).cuda()
                    got = fwd(x, w, bias, M, N, K, 1, R.GEMM_FP32, rate, seed, layer, host_step, state).read()
                    ref, _ = R.dropout_ref(c["y_relu"], seed, layer, step, rate)
                    n_bad += differing(got, ref)
                    by_host = fwd(x, w, bias, M, N, K, 1, R.GEMM_FP32, rate, seed, layer, step).read()
                    n_bad += int(np.count_nonzero(bits(got) != bits(by_host)))
                    assert np.array_equal(state.cpu().numpy().view(np.uint32), words), "the step state was written"
        print(f"    rate {rate_name(rate)}: differing elements (twin, and bits of the host-prefix form) {n_bad}")
        total += n_bad
    # the twin's masks of these steps differ from the host step's, so a kernel that ignored the state could not pass
    assert not np.array_equal(R.dropout_ref(c["y_relu"], 42, 0, 0, 0.3)[1], R.dropout_ref(c["y_relu"], 42, 0, host_step, 0.3)[1])
    assert all(o.intact() for o in (x, w, bias))
    assert total == 0


@pytest.mark.parametrize("M,N,K", R.DROPOUT_SHAPES, ids=[sid(s) for s in R.DROPOUT_SHAPES])
def test_dropout_backward_gates_and_scales_the_input_gradient(M, N, K):
    """The layer input is h = dropout(relu(.)) [M][K] (the twin's mask on the integer x, one -0.0 planted where it was
    dropped), mask = h, mask_scale = the keep scale: dx == where(h > 0, fl32(dx0 * fl32(scale)), 0) EXACTLY and db exactly,
    merged and as two launches, fp32 and GEMM_BF16.  dw = dy^T h is exact where h is made of integers (rate 0.5: scale 2);
    at the other rates h = fl32(x * scale) is not, an fp32 sum of such terms depends on its order, and dw is held to the
    per-element bound instead, with the merged launch bit-equal to the two launches."""
    c = R.integer_case(M, N, K)
    assert R.integer_regime_exact(M, N, K, x_max=2 * R.X_MAX)
    w, dy = Operand(c["w"]), Operand(c["dy"])
    total = 0
    print(f"\n  dropout backward {M}x{N}x{K}")
    for rate in R.DROPOUT_RATES:
        scale = R.keep_scale32(rate)
        h, keep = R.dropout_ref(c["x"], 42, 0, 1, rate)
        h = h.copy()
        planted = np.argwhere((h == 0) & (c["dx"] != 0))
        assert len(planted), "no dropped / zero element with a non-zero gradient to plant -0.0 at"
        h[tuple(planted[0])] = np.float32(-0.0)
        assert np.signbit(h[tuple(planted[0])])
        dx_ref = R.dropout_dgrad_ref(c["dx"], h, rate)
        assert dx_ref[tuple(planted[0])] == 0 and np.count_nonzero(dx_ref) > 0
        hd = Operand(h)
        exact_dw = R.is_small_integer(h)
        assert exact_dw == (rate == 0.5)
        for mode, mname in R.MODES:
            dw_ref, db_ref = R.wgrad_ref(h, c["dy"], mode)
            out = {}
            for merged, lname in LAUNCHES:
                dx, dw, db = (o.read() for o in bwd(hd, w, dy, M, N, K, 1, scale, mode, merged))
                out[merged] = (dx, dw, db)
                n_dx, n_db = differing(dx, dx_ref), differing(db, db_ref)
                line = f"    rate {rate_name(rate)} {mname} {lname}: differing elements dx {n_dx} db {n_db}"
                if exact_dw:
                    n_dw = differing(dw, dw_ref)
                    line += f" dw {n_dw}"
                else:
                    q = ratio(dw, dw_ref, R.wgrad_bound(h, c["dy"], mode))
                    n_dw = 0 if q < 1.0 else 1
                    line += f"; dw worst err/bound {q:.3f}"
                print(line)
                total += n_dx + n_db + n_dw
            for a, b in zip(out[1], out[0]):
                assert np.array_equal(bits(a), bits(b)), "the merged launch and the two launches differ"
        assert hd.intact()
    assert w.intact() and dy.intact()
    assert total == 0
