"""GPU: the polyphase resampler (csrc/resample.hip) against its numpy statement and against scipy.signal.resample_poly.

Operands and outputs sit between NaN guards inside larger device tensors; the guards must come back bit-unchanged, the input
payload too, and every output element must be finite.

Exact regime -- no tolerance.  Taps are integers in -3..3 and x holds integers in -4..4, so every partial sum of an output is
an integer of magnitude at most 12 tpp <= 3072, far below 2^24 (asserted from the shape): fp32 holds it exactly, fused or not, and
y must EQUAL ``resample_reference`` in float64.  One wrong index, phase or edge fails.

Float regime, default filter -- per output, against scipy.signal.resample_poly of the fp32 input in float64:
``|err| <= (tpp + 3) 2^-24 sum_i |h[..]| |x[i]|``: the running-sum bound of tpp fused terms (each of the tpp additions rounds a
partial sum that is at most the sum of the magnitudes, tpp 2^-24 in all to first order) plus the rounding of each tap to fp32
(one more 2^-24 of the same sum), with two units of slack for the second-order terms and the difference between the two double
designs.  Derived, not fitted; each case prints its worst ratio."""
import ctypes as C
import functools
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.signal as ss
import torch

from cmoop_audio_processing_amd import EvalConfig, FrontendConfig, StreamScorer, TrainedModel, _lib, frontend, genes as G, resample_poly
from cmoop_audio_processing_amd import resample as R
from cmoop_audio_processing_amd.session import NetSession

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 67                                     # floats of NaN on either side; odd, so payloads are not 16-byte aligned
NAN_BITS = 0x7FC00000


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


def guarded(n_floats):
    return torch.full((GUARD + n_floats + GUARD,), float("nan"), device="cuda", dtype=torch.float32)


def guards_intact(buf, n_floats):
    bits = buf.view(torch.int32)
    return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + n_floats:] == NAN_BITS).all())


def launch(x, up, down, taps, finite_rows=None):
    """cmoop_resample on x [n, L] (host float32) between guards -> host float32 [n, n_out]."""
    x = np.ascontiguousarray(x, np.float32)
    assert x.ndim == 2
    n, L = x.shape
    taps = np.ascontiguousarray(taps, np.float32)
    n_out = R.resample_plan(L, up, down, taps.size)[0]
    xin, out = guarded(n * L), guarded(n * n_out)
    xin[GUARD:GUARD + n * L] = dev(x.reshape(-1))
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_resample(_lib.ptr(xin[GUARD:GUARD + n * L]), C.c_int64(n), C.c_int64(L), C.c_int32(up), C.c_int32(down),
                                         _lib.ptr(taps), C.c_int32(taps.size), _lib.ptr(out[GUARD:GUARD + n * n_out])))
    torch.cuda.synchronize()
    assert guards_intact(out, n * n_out), "the output's guards changed"
    assert guards_intact(xin, n * L), "the input's guards changed"
    assert np.array_equal(xin[GUARD:GUARD + n * L].cpu().numpy().view(np.uint32), x.reshape(-1).view(np.uint32)), "the input changed"
    y = out[GUARD:GUARD + n * n_out].cpu().numpy().reshape(n, n_out)
    rows = range(n) if finite_rows is None else finite_rows
    assert all(np.isfinite(y[r]).all() for r in rows), "non-finite output"
    return y


# ---- 1. exact regime ----------------------------------------------------------------------------------------------------------
#: (up, down, n_taps, taps per output, tile, where a lane's table row comes from): tpp takes 1, 2, 21, 56 and 256; two rows have
#: tiles below 512; "one" is the wave-uniform row of up = 1, "lds" a table copied into LDS by persistent workgroups, "global" a
#: table too large for that (the last row: 441 x 41 floats)
EXACT = [(1, 2, 21, 21, 512, "one"), (2, 1, 3, 2, 512, "lds"), (3, 2, 3, 1, 512, "lds"), (2, 3, 41, 21, 512, "lds"),
         (7, 5, 391, 56, 512, "lds"), (160, 441, 8821, 56, 512, "lds"), (441, 160, 8821, 21, 512, "lds"), (1, 8, 161, 161, 512, "one"),
         (8, 1, 161, 21, 512, "lds"), (2, 3, 511, 256, 512, "lds"), (3, 64, 21, 7, 320, "lds"), (1, 1024, 21, 21, 7, "one"),
         (441, 160, 17641, 41, 512, "global")]


def table_source(up, down, tpp, tile):
    """The launcher's rule (csrc/resample.hip): the table sits in LDS when the widest span of a tile, rounded up to four floats,
    and the table at an odd row stride fit 64 KiB together."""
    span = ((tile - 1) * down // up + tpp + 1 + 3) // 4 * 4
    return "one" if up == 1 else "lds" if (span + up * (tpp | 1)) * 4 <= 64 * 1024 else "global"


def integers(rs, lo, hi, shape):
    return rs.randint(lo, hi + 1, shape).astype(np.float32)


def lengths_for(up, down, n_taps):
    """L = 1, L below one tap spacing, and the shortest L whose n_out reaches 1, tile - 1, tile, tile + 1 and 2 tile + 1."""
    tile = R.resample_plan(1, up, down, n_taps)[1]
    out = {1: None, 3: None}
    for target in (1, tile - 1, tile, tile + 1, 2 * tile + 1):
        if target >= 1:
            L = max(1, (target - 1) * down // up + 1)
            n_out = R.resample_plan(L, up, down, n_taps)[0]
            assert n_out >= target and (n_out == target or up > down), (L, n_out, target)
            out[L] = target
    return tile, sorted(out)


@pytest.mark.parametrize("up,down,n_taps,tpp,tile,source", EXACT, ids=[f"{c[0]}-{c[1]}-taps{c[2]}" for c in EXACT])
def test_exact_regime_equals_the_reference(up, down, n_taps, tpp, tile, source):
    assert R.resample_plan(1, up, down, n_taps)[1:] == (tile, 1, tpp)
    assert table_source(up, down, tpp, tile) == source
    assert 3 * 4 * tpp < 2 ** 24                                             # every partial sum is an integer fp32 holds
    rs = np.random.RandomState(up * 7919 + down * 31 + n_taps)
    taps = integers(rs, -3, 3, n_taps)
    got_tile, lengths = lengths_for(up, down, n_taps)
    assert got_tile == tile
    seen = set()
    for L in lengths:
        for n_clips in (1, 3):
            x = integers(rs, -4, 4, (n_clips, L))
            y = launch(x, up, down, taps)
            want = R.resample_reference(x, up, down, taps)
            seen.add(y.shape[1])
            assert y.shape == want.shape == (n_clips, -(-L * up // down))
            bad = np.argwhere(y.astype(np.float64) != want)
            assert bad.size == 0, (up, down, n_taps, L, n_clips, bad[:5].tolist())
    if up <= down:
        assert {1, tile, tile + 1, 2 * tile + 1} <= seen and (tile == 1 or tile - 1 in seen)


def test_one_tap_is_the_identity_and_a_late_tap_a_shift():
    rs = np.random.RandomState(1)
    for L in (1, 5, 511, 512, 513, 1025):
        x = integers(rs, -4, 4, (3, L))
        assert np.array_equal(launch(x, 1, 1, [1.0]), x)
        shifted = launch(x, 1, 1, [0.0, 0.0, 1.0])                           # y[n] = x[n - 1]
        assert np.array_equal(shifted[:, 1:], x[:, :-1]) and not shifted[:, 0].any()
        early = launch(x, 1, 1, [1.0, 0.0, 0.0])                             # y[n] = x[n + 1]
        assert np.array_equal(early[:, :-1], x[:, 1:]) and not early[:, -1].any()


def test_more_work_items_than_workgroups():
    """16 500 rows of four tiles: 66 000 (row, tile) pairs on at most 65 536 workgroups, the grid strides.  The one-sample
    shift, compared on the device."""
    n, L = 16500, 2048
    assert n * R.resample_plan(L, 1, 1, 3)[2] > 65536
    x = torch.randint(-4, 5, (n, L), device="cuda").to(torch.float32)
    y = resample_poly(x, 16000, 16000, taps=[0.0, 0.0, 1.0])
    assert tuple(y.shape) == (n, L)
    assert torch.equal(y[:, 1:], x[:, :-1]) and not bool(y[:, 0].any())


# ---- 2. rows and grids --------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def float_rows(L):
    """[6, L] float32, read-only: two Gaussian rows, two tones (0.0227 and 0.45 of the rate, the second above the new Nyquist of
    every down-going pair below), and a unit impulse at the first, the middle and the last sample."""
    rs = np.random.RandomState(L)
    t = np.arange(L)
    x = np.zeros((6, L))
    x[0], x[1] = rs.randn(L), 0.1 * rs.randn(L)
    x[2] = 0.6 * np.sin(2 * np.pi * 0.0227 * t) + 0.4 * np.sin(2 * np.pi * 0.45 * t + 0.3)
    x[3, 0], x[4, L // 2], x[5, L - 1] = 1.0, 1.0, 1.0
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x


def test_rows_do_not_bleed():
    """Rows 0 and 2 are NaN: the zero padding of row 1 is its own, its bytes are those of the one-row call."""
    for up, down, taps, L in ((1, 3, R.resample_filter(1, 3), 1601), (160, 441, R.resample_filter(160, 441), 4410),
                              (3, 1, R.resample_filter(3, 1), 700)):
        x = np.full((3, L), np.nan, np.float32)
        x[1] = float_rows(4410)[0, :L]
        y = launch(x, up, down, taps, finite_rows=[1])
        alone = launch(x[1:2], up, down, taps)
        assert np.array_equal(y[1].view(np.uint32), alone[0].view(np.uint32)), (up, down)
        assert np.isnan(y[0]).all() and np.isnan(y[2]).all()


def test_a_row_of_a_batch_has_the_bytes_of_the_single_call():
    rs = np.random.RandomState(2)
    cases = [(44100, 16000, None, float_rows(4410)), (16000, 48000, None, float_rows(4410)[:, :1300]),
             (5, 7, integers(rs, -3, 3, 391), integers(rs, -4, 4, (4, 1500)))]
    for sr_in, sr_out, taps, x in cases:
        xd = dev(x)
        batch = resample_poly(xd, sr_in, sr_out, taps=taps)
        up, down = R.rational(sr_in, sr_out)
        assert tuple(batch.shape) == (x.shape[0], -(-x.shape[1] * up // down))
        for r in range(x.shape[0]):
            single = resample_poly(xd[r], sr_in, sr_out, taps=taps)
            assert single.dim() == 1 and torch.equal(single.view(torch.int32), batch[r].view(torch.int32)), (sr_in, sr_out, r)
    same = resample_poly(xd, 16000, 16000)                                   # equal rates without taps: a copy, nothing launched
    assert torch.equal(same, xd) and same.data_ptr() != xd.data_ptr()
    with pytest.raises(ValueError, match="CUDA float32"):
        resample_poly(xd.double(), 48000, 16000)


# ---- 3. the 32-bit product ----------------------------------------------------------------------------------------------------
def test_positions_beyond_2_31():
    """up 1024, down 1023, 2049 integer taps (three per output), L = 2 200 000: outputs from n = 2 099 202 on sit at positions
    n down + half above 2^31.  The whole output EQUALS the float64 reference."""
    up, down, n_taps, L = 1024, 1023, 2049, 2_200_000
    n_out, tile, n_tiles, tpp = R.resample_plan(L, up, down, n_taps)
    assert tpp == 3 and (n_out - 1) * down + 1024 > 2 ** 31 and 3 * 4 * tpp < 2 ** 24
    rs = np.random.RandomState(3)
    taps, x = integers(rs, -3, 3, n_taps), integers(rs, -4, 4, (1, L))
    y = launch(x, up, down, taps)
    want = R.resample_reference(x, up, down, taps)
    bad = np.argwhere(y.astype(np.float64) != want)
    assert bad.size == 0, (len(bad), bad[:5].tolist())
    assert np.abs(want[0, 2 ** 31 // down + 1:]).max() > 0


# ---- 4. float regime, default filter ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out", [(48000, 16000), (44100, 16000), (16000, 48000), (32000, 16000), (22050, 16000)])
@pytest.mark.parametrize("L", [4410, 16000])
def test_default_filter_against_scipy(sr_in, sr_out, L):
    up, down = R.rational(sr_in, sr_out)
    x = float_rows(L)
    taps = R.resample_filter(up, down)
    tpp = R.resample_plan(L, up, down, taps.size)[3]
    y = launch(x, up, down, taps)
    assert torch.equal(resample_poly(dev(x), sr_in, sr_out).cpu().view(torch.int32), torch.from_numpy(y).view(torch.int32))
    x64 = x.astype(np.float64)
    want = ss.resample_poly(x64, up, down, axis=-1)
    assert y.shape == want.shape
    m = max(up, down)
    h64 = ss.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up
    bound = (tpp + 3) * 2.0 ** -24 * R.resample_reference(np.abs(x64), up, down, np.abs(h64))
    err = np.abs(y.astype(np.float64) - want)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))
    print(f"\n{sr_in} -> {sr_out}, L {L}, tpp {tpp}: worst |err| / bound per row {[round(float(r), 4) for r in ratio.max(axis=1)]}")
    assert (err <= bound).all(), (sr_in, sr_out, L, float(ratio.max()))


# ---- 5. sr= on the scorer and the front end -----------------------------------------------------------------------------------
T, F, GENE, CLASSES = 21, 12, (16, 3, 1, 1, 2, 1), 10


def test_stream_scorer_and_the_front_end_take_a_sample_rate():
    cfg = EvalConfig(variant="A", classes=CLASSES, eval_batch=4)
    fcfg = FrontendConfig(n_mels=F)
    with NetSession(GENE, cfg, T, F, 5) as net:
        params = net.get_params()                                             # untrained: the seeded initial weights
    rs = np.random.RandomState(6)
    model = TrainedModel(gene=GENE, variant="A", classes=CLASSES, T=T, F=F, seed=5, params=params,
                         objectives={"acc": 0.1, "size_mb": G.model_size_mb(GENE, 0, CLASSES), "fpr": 0.5, "epochs_run": 0},
                         frontend=fcfg, mean=rs.randn(F) - 5.0, scale=1.0 + rs.rand(F))
    t = np.arange(48000) / 48000.0
    wav48 = dev((0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * rs.randn(48000)).astype(np.float32))     # 1 s at 48 kHz
    wav16 = resample_poly(wav48, 48000, 16000)
    assert tuple(wav16.shape) == (16000,)
    with StreamScorer(model, 10, cfg) as scorer:
        t_a, p_a = scorer.score(wav48, sr=48000)
        t_b, p_b = scorer.score(wav16)
        assert tuple(p_a.shape) == (1 + (101 - T) // 10, CLASSES) and np.isfinite(p_a.cpu().numpy()).all()
        assert np.array_equal(t_a, t_b) and t_a.dtype == np.float64 and t_a[1] == 10 * 160 / 16000.0
        assert torch.equal(p_a.view(torch.int32), p_b.view(torch.int32))
        t_c, p_c = scorer.score(wav16, sr=16000)
        assert np.array_equal(t_c, t_b) and torch.equal(p_c.view(torch.int32), p_b.view(torch.int32))
        for bad in (0, -16000, 16000.5, "48000"):
            with pytest.raises(ValueError, match="StreamScorer.score: sr "):
                scorer.score(wav16, sr=bad)
    clips = dev(float_rows(4410)[:3])
    clips16 = resample_poly(clips, 44100, 16000)
    for c in (None, fcfg, FrontendConfig(sr=32000, n_fft=1024, win=1024, hop=256, n_mels=64, fmax=16000.0, scale="db")):
        sr_model = 16000 if c is None else c.sr
        two_step = resample_poly(clips, 44100, sr_model)
        assert torch.equal(frontend.log_mel(clips, c, sr=44100).view(torch.int32), frontend.log_mel(two_step, c).view(torch.int32))
        assert torch.equal(frontend.log_mel(two_step, c, sr=sr_model), frontend.log_mel(two_step, c))
        assert torch.equal(frontend.log_mel_stream(clips[0], c, sr=44100).view(torch.int32),
                           frontend.log_mel_stream(two_step[0], c).view(torch.int32))
    assert torch.equal(clips16, resample_poly(clips, 44100, 16000))


# ---- 6. stale memory ----------------------------------------------------------------------------------------------------------
STALE_CASE = (44100, 16000, 4410)
_CHILD = """
import hashlib, os, sys
sys.path.insert(0, {root!r})
sys.path.insert(0, os.path.join({root!r}, "tests"))
import torch
from test_gpu_resample import STALE_CASE, float_rows, dev
from cmoop_audio_processing_amd import resample_poly
sr_in, sr_out, L = STALE_CASE
x = dev(float_rows(L))
for fill in ("", "0xFF", "0x7F"):
    os.environ["CMOOP_POOL_FILL"] = fill
    y = resample_poly(x, sr_in, sr_out).cpu().numpy()
    print("digest", fill or "unset", hashlib.sha256(y.tobytes()).hexdigest(), flush=True)
"""


def test_results_do_not_depend_on_what_the_pooled_table_held():
    """One float-regime case in a child process, unset and under CMOOP_POOL_FILL=0xFF (every float a NaN) and 0x7F (3.39e38): the
    bytes are those of this process's plain run."""
    sr_in, sr_out, L = STALE_CASE
    before = os.environ.pop("CMOOP_POOL_FILL", None)
    try:
        y = resample_poly(dev(float_rows(L)), sr_in, sr_out).cpu().numpy()
    finally:
        if before is not None:
            os.environ["CMOOP_POOL_FILL"] = before
    assert np.isfinite(y).all()
    want = hashlib.sha256(y.tobytes()).hexdigest()
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], capture_output=True, text=True, cwd=ROOT, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    digests = dict(line.split()[1:3] for line in r.stdout.splitlines() if line.startswith("digest "))
    assert sorted(digests) == ["0x7F", "0xFF", "unset"], r.stdout
    assert digests == {"unset": want, "0xFF": want, "0x7F": want}, digests
