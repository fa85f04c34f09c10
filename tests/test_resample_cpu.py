"""CPU: the resampler's host side -- symbols, rate pairs, the default filter against scipy.signal.firwin, the numpy reference
against scipy.signal.resample_poly, the launch plan and tile spans (positions far beyond 2^31, no data involved) and the domain.

Gates.  Filter: every fp32 tap equals scipy's double design rounded to fp32 or sits within 1 ulp of it (the two double designs
differ by <= 2e-15 relative, so at most a rounding tie flips), and lies within 1e-12 of the largest tap of scipy's double
design beyond its own fp32 rounding (observed 1.3e-15).  Reference: 1e-12 of the largest output against scipy in float64."""
import ctypes as C
import math

import numpy as np
import pytest
import scipy.signal as ss
import torch

import cmoop_audio_processing_amd as pkg
from cmoop_audio_processing_amd import _lib, frontend, resample as R

PAIRS = [(1, 3), (3, 1), (160, 441), (441, 160), (147, 160), (640, 441), (1, 8)]
SYMBOLS = ("cmoop_resample_filter", "cmoop_resample_plan", "cmoop_resample_tile_span", "cmoop_resample", "cmoop_resample_time")
LDS_FLOATS, MAX_TILE = 8192, 512


def scipy_filter(up, down):
    m = max(up, down)
    return ss.firwin(20 * m + 1, 1.0 / m, window=("kaiser", 5.0)) * up


# ---- symbols ------------------------------------------------------------------------------------------------------------------
def test_symbols_are_declared_exported_and_prototyped():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in SYMBOLS:
        assert name in declared and hasattr(L, name) and name in _lib.RESAMPLE_PROTOTYPES, name
        assert getattr(L, name).argtypes == _lib.RESAMPLE_PROTOTYPES[name]
    assert sorted(_lib.RESAMPLE_PROTOTYPES) == sorted(SYMBOLS)
    assert L.cmoop_abi_version() == 3
    assert "resample_poly" in pkg.__all__ and pkg.resample_poly is R.resample_poly is frontend.resample_poly


# ---- rate pairs ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sr_in,sr_out,want", [(48000, 16000, (1, 3)), (44100, 16000, (160, 441)), (16000, 44100, (441, 160)),
                                               (22050, 16000, (320, 441)), (32000, 16000, (1, 2)), (8000, 16000, (2, 1)),
                                               (16000, 16000, (1, 1))])
def test_rational_reduces_the_rates(sr_in, sr_out, want):
    assert R.rational(sr_in, sr_out) == want
    assert R.rational(np.int64(sr_in), np.int32(sr_out)) == want


@pytest.mark.parametrize("bad", [0, -16000, 16000.0, 44100.5, "16000", None, True])
def test_rational_refuses_what_is_not_a_positive_integer_rate(bad):
    with pytest.raises(ValueError, match="resample: sr_in "):
        R.rational(bad, 16000)
    with pytest.raises(ValueError, match="resample: sr_out "):
        R.rational(16000, bad)


# ---- the default filter -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", PAIRS)
def test_default_filter_is_scipys_firwin_times_up(up, down):
    h, ref = R.resample_filter(up, down), scipy_filter(up, down)
    assert h.dtype == np.float32 and h.shape == ref.shape == (20 * max(up, down) + 1,)
    ref32 = ref.astype(np.float32)
    ulps = np.abs(h.view(np.int32).astype(np.int64) - ref32.view(np.int32).astype(np.int64))
    beyond_rounding = np.abs(h.astype(np.float64) - ref) - 2.0 ** -24 * np.abs(ref)
    print(f"{up}/{down}: {int((ulps != 0).sum())} of {h.size} taps differ from scipy's rounded to fp32, at most {int(ulps.max())} ulp; "
          f"beyond fp32 rounding {max(0.0, beyond_rounding.max()) / np.abs(ref).max():.2e} of the maximum")
    assert ulps.max() <= 1
    assert beyond_rounding.max() <= 1e-12 * np.abs(ref).max()
    assert np.array_equal(h, h[::-1])                                        # centred and symmetric


def test_filter_arguments():
    assert R.resample_filter(1, 3, half_width=4).size == 25
    wide, narrow = R.resample_filter(1, 3, beta=0.0), R.resample_filter(1, 3, beta=12.0)
    assert abs(float(wide.sum()) - 1.0) < 1e-6 and abs(float(narrow.sum()) - 1.0) < 1e-6 and not np.array_equal(wide, narrow)
    L, n = _lib.lib(), C.c_int32()
    small = np.zeros(10, np.float32)
    assert L.cmoop_resample_filter(1, 3, 10, 5.0, _lib.ptr(small), 10, C.byref(n)) != 0
    assert L.cmoop_last_error().decode().startswith("resample: cap ") and n.value == 61 and not small.any()
    for kw, field in ((dict(half_width=0), "half_width"), (dict(half_width=5000), "half_width"), (dict(beta=-1.0), "beta"),
                      (dict(beta=float("nan")), "beta")):
        with pytest.raises(ValueError, match=f"^resample: {field} "):
            R.resample_filter(1, 3, **kw)


# ---- the reference against scipy ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("up,down", PAIRS)
def test_reference_is_scipys_resample_poly(up, down):
    h = scipy_filter(up, down)
    rs = np.random.RandomState(up * 1000 + down)
    for L in (1, 7, 41, 1601, 4410):
        x = rs.randn(L)
        got, want = R.resample_reference(x, up, down, h), ss.resample_poly(x, up, down)
        assert got.dtype == np.float64 and got.shape == want.shape == (-(-L * up // down),), (L, got.shape, want.shape)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (up, down, L)
    x = rs.randn(3, 41)                                                       # leading axes are rows
    assert np.array_equal(R.resample_reference(x, up, down, h)[1], R.resample_reference(x[1], up, down, h))
    assert R.resample_reference(x.astype(np.float32), up, down, h, dtype=np.float32).dtype == np.float32


# ---- plan and tile spans ------------------------------------------------------------------------------------------------------
PLAN_CASES = [(up, down, 20 * max(up, down) + 1) for up, down in PAIRS] + \
    [(1, 1, 1), (1, 1, 3), (1, 2, 1), (2, 1, 3), (7, 5, 391), (1024, 1023, 2049), (1, 1024, 255), (1024, 1, 1), (3, 2, 767), (1, 12, 241)]
PLAN_LENGTHS = (1, 7, 4410, 16000, 2_200_000, 2 ** 31 + 5, 2 ** 35)


def span_in_python(L, up, down, n_taps, tile, j):
    """The header's rule in Python integers."""
    half, tpp = (n_taps - 1) // 2, -(-n_taps // up)
    n_out = -(-L * up // down)
    out_first = j * tile
    out_count = min(tile, n_out - out_first)
    in_first = (out_first * down + half) // up - tpp + 1
    in_last = ((out_first + out_count - 1) * down + half) // up
    return out_first, out_count, in_first, in_last - in_first + 1


@pytest.mark.parametrize("up,down,n_taps", PLAN_CASES)
def test_plan_and_tile_spans(up, down, n_taps):
    half, tpp = (n_taps - 1) // 2, -(-n_taps // up)
    tiles_seen = set()
    for L in PLAN_LENGTHS:
        n_out, tile, n_tiles, got_tpp = R.resample_plan(L, up, down, n_taps)
        assert n_out == -(-L * up // down) and got_tpp == tpp and n_tiles == -(-n_out // tile)
        tiles_seen.add(tile)
        at_2_31 = (2 ** 31 // down) // tile                                   # the tile in which n down passes 2^31
        js = range(n_tiles) if n_tiles <= 64 else sorted(j for j in {0, 1, n_tiles // 2, at_2_31, at_2_31 + 1, n_tiles - 2, n_tiles - 1}
                                                         if 0 <= j < n_tiles)
        covered = 0
        for j in js:
            span = R.resample_tile_span(L, up, down, n_taps, j)
            assert span == span_in_python(L, up, down, n_taps, tile, j), (L, j)
            out_first, out_count, in_first, in_count = span
            assert out_first == j * tile and 1 <= out_count <= tile
            covered += out_count
            # every index an output of the tile reads under the definition lies inside the span
            for n in range(out_first, out_first + out_count):
                pos = n * down + half
                i_lo, i_hi = -((2 * half - pos) // up), pos // up             # ceil((pos - 2 half) / up), floor(pos / up)
                assert in_first <= i_lo and i_hi < in_first + in_count, (L, j, n)
                assert i_hi - i_lo + 1 <= tpp
            assert in_count <= min(LDS_FLOATS, -(-tile * down // up) + tpp + 2), (L, j, in_count)
        if n_tiles <= 64:
            assert covered == n_out                                           # consecutive tiles, each output once
        last = R.resample_tile_span(L, up, down, n_taps, n_tiles - 1)
        assert last[0] + last[1] == n_out
        with pytest.raises(ValueError, match="^resample: tile_index "):
            R.resample_tile_span(L, up, down, n_taps, n_tiles)
    assert len(tiles_seen) == 1, tiles_seen                                   # tile depends on (up, down, n_taps) alone
    tile = tiles_seen.pop()
    assert 1 <= tile <= MAX_TILE and (tile < 64 or tile % 64 == 0)


def test_tile_at_the_usual_ratios():
    assert R.resample_plan(16000, 1, 3, 61)[1] == 512 and R.resample_plan(16000, 160, 441, 8821)[1] == 512
    assert R.resample_plan(16000, 1, 8, 161)[1] == 512 and R.resample_plan(16000, 1, 1024, 255)[1] == 7


# ---- domain -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("args,field", [
    ((0, 1, 3, 61), "n_samples"), ((2 ** 36, 1, 3, 61), "n_samples"), ((10, 0, 3, 61), "up"), ((10, 1025, 1, 61), "up"),
    ((10, 1, 0, 61), "down"), ((10, 1, 1025, 61), "down"), ((10, 2, 4, 61), "up / down"), ((10, 1, 3, 60), "n_taps"),
    ((10, 1, 3, 0), "n_taps"), ((10, 1, 3, -1), "n_taps"), ((10, 1, 3, 257), "n_taps"), ((10, 4, 3, 1025), "n_taps")])
def test_plan_refuses_what_is_outside_the_domain(args, field):
    with pytest.raises(ValueError, match=f"^resample: {field} "):
        R.resample_plan(*args)
    with pytest.raises(ValueError, match=f"^resample: {field} "):
        R.resample_tile_span(*args, 0)


def test_the_edge_of_the_domain_is_inside():
    assert R.resample_plan(2 ** 36 - 1, 1024, 1023, 2049)[3] == 3
    assert R.resample_plan(10, 1, 3, 255)[3] == 255 and R.resample_plan(10, 4, 3, 1023)[3] == 256
    assert R.resample_plan(10, 1, 1, 1) == (10, 512, 1, 1)


@pytest.mark.parametrize("n_clips,n_samples,up,down,n_taps,taps,field", [
    (-1, 10, 1, 3, 61, True, "n_clips"), (2 ** 21, 2 ** 15, 1, 3, 61, True, "n_clips"), (2 ** 10, 2 ** 20, 64, 1, 65, True, "n_clips"),
    (1, 10, 1, 3, 61, False, "taps_host"), (1, 10, 1, 3, 62, True, "n_taps"), (1, 10, 6, 3, 61, True, "up / down"),
    (1, 0, 1, 3, 61, True, "n_samples"), (1, 10, 1, 3, 61, True, "wav_dev")])
def test_the_launch_checks_the_whole_domain_before_it_touches_the_device(n_clips, n_samples, up, down, n_taps, taps, field):
    """Each of these calls ends at its host check: the device pointers are NULL and no GPU is needed."""
    L, h, ms = _lib.lib(), np.zeros(2049, np.float32), C.c_double()
    for rc in (L.cmoop_resample(None, n_clips, n_samples, up, down, _lib.ptr(h) if taps else None, n_taps, None),
               L.cmoop_resample_time(None, n_clips, n_samples, up, down, _lib.ptr(h) if taps else None, n_taps, None, 1, C.byref(ms))):
        assert rc != 0
        assert L.cmoop_last_error().decode().startswith(f"resample: {field} "), L.cmoop_last_error().decode()
    assert L.cmoop_resample_time(None, 1, 10, 1, 3, _lib.ptr(h), 61, None, 0, C.byref(ms)) != 0
    assert L.cmoop_last_error().decode().startswith("resample: iters ")


def test_resample_poly_names_a_ratio_beyond_the_default_filter():
    """down > 12 up: the default filter would need more than 256 taps per output; the host check comes before any tensor check."""
    wav = torch.zeros(64)
    for sr_in, sr_out in ((16000, 1000), (48000, 3000), (13, 1)):
        with pytest.raises(ValueError, match=rf"^resample: the ratio sr_in / sr_out = {sr_in} / {sr_out} "):
            R.resample_poly(wav, sr_in, sr_out)
    with pytest.raises(ValueError, match="CUDA float32"):                    # 12 : 1 is inside; a host tensor is not
        R.resample_poly(wav, 12, 1)
    with pytest.raises(ValueError, match="resample: sr_in "):
        R.resample_poly(wav, 0, 16000)
    for up, down in ((1, 12), (5, 63)):
        assert -(-(20 * down + 1) // up) <= R.MAX_TAPS_PER_OUTPUT
    assert math.gcd(5, 63) == 1 and -(-(20 * 13 + 1) // 1) > R.MAX_TAPS_PER_OUTPUT


@pytest.mark.parametrize("bad", [0, -48000, 48000.0, "48000", True])
def test_the_sr_keyword_refuses_what_is_not_a_positive_integer_rate(bad):
    with pytest.raises(ValueError, match="log_mel: sr "):
        frontend.log_mel(torch.zeros(2, 64), sr=bad)
    with pytest.raises(ValueError, match="log_mel_stream: sr "):
        frontend.log_mel_stream(torch.zeros(64), sr=bad)
    with pytest.raises(ValueError, match="StreamScorer.score: sr "):
        R.to_rate(torch.zeros(64), bad, 16000, "StreamScorer.score")
