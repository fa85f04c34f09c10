"""Polyphase resampler on the GPU (libcmoop_hip.so): clips and recordings at any sample rate, brought to the front end's.

A trained model is bound to the ``FrontendConfig.sr`` it was trained at; field recorders run at 48 kHz, ESC-style sets at
44.1 kHz, telephony at 8 kHz.  ``resample_poly(wav, sr_in, sr_out)`` is ``scipy.signal.resample_poly`` with its default
filter, on the device; ``log_mel`` / ``log_mel_stream`` / ``StreamScorer.score`` take ``sr=`` and call it first.  No
audio-quality or accuracy claim is made beyond "it is scipy's ``resample_poly`` default filter".

Definition (include/cmoop.h).  Rational resampling by ``up / down`` with ``gcd(up, down) = 1`` (``rational`` reduces
``sr_out / sr_in``; the ABI refuses a common factor) and an odd-length centred FIR ``h`` of ``n_taps = 2 half + 1`` taps.
For a row ``x[0..L)``, ``x = 0`` outside::

    n_out = ceil(L up / down)
    y[n]  = sum_i x[i] h[n down - i up + half]    over all i with 0 <= n down - i up + half <= 2 half and 0 <= i < L

Default filter: ``half = half_width max(up, down)`` (``half_width`` 10), ``fc = 1 / max(up, down)``,
``h[k] = up w[k] fc sinc(fc (k - half)) / sum(w fc sinc)`` with ``w`` the Kaiser window of ``n_taps`` points (``beta`` 5.0),
designed in double on the host and rounded once to fp32.  ``taps=`` passes any odd number of fp32 taps instead (scipy's
``window=<array>`` form).

Device arithmetic: one fp32 accumulator per output, started at 0, terms in ascending ``i``, one fused multiply-add per
term; the order is part of the definition, so every launch shape gives the same bits.

Domain: ``1 <= up, down <= 1024``; ``n_taps`` odd; ``ceil(n_taps / up) <= 256`` taps per output (the default filter
therefore serves every ``down <= 12 up``; ``resample_poly`` raises beyond that and names the ratio); ``1 <= n_samples``;
``n_clips max(n_samples, n_out) < 2^36``.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib

MAX_TAPS_PER_OUTPUT = 256


def _error() -> str:
    return _lib.lib().cmoop_last_error().decode("utf-8", "replace")


def rational(sr_in, sr_out):
    """(up, down) = sr_out / sr_in reduced by their gcd; both rates positive integers (host only)."""
    for name, v in (("sr_in", sr_in), ("sr_out", sr_out)):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or int(v) < 1:
            raise ValueError(f"resample: {name} must be a positive integer sample rate (got {v!r})")
    g = math.gcd(int(sr_in), int(sr_out))
    return int(sr_out) // g, int(sr_in) // g


def resample_filter(up: int, down: int, half_width: int = 10, beta: float = 5.0) -> np.ndarray:
    """The default filter, float32 [2 half_width max(up, down) + 1] (host only, ``cmoop_resample_filter``)."""
    L, n = _lib.lib(), C.c_int32()
    if L.cmoop_resample_filter(C.c_int32(int(up)), C.c_int32(int(down)), C.c_int32(int(half_width)), C.c_double(float(beta)), None,
                               C.c_int32(0), C.byref(n)) != 0:
        raise ValueError(_error())
    taps = np.zeros(n.value, np.float32)
    if L.cmoop_resample_filter(C.c_int32(int(up)), C.c_int32(int(down)), C.c_int32(int(half_width)), C.c_double(float(beta)),
                               _lib.ptr(taps), C.c_int32(n.value), C.byref(n)) != 0:
        raise ValueError(_error())
    return taps


def resample_plan(n_samples: int, up: int, down: int, n_taps: int):
    """(n_out, tile, n_tiles, taps_per_output) of a row of n_samples (host only): ``n_out = ceil(n_samples up / down)``, a
    workgroup owns ``tile`` consecutive outputs -- a function of (up, down, n_taps) alone -- and a row has ``n_tiles``."""
    n_out, tile, n_tiles, tpp = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int32()
    if _lib.lib().cmoop_resample_plan(C.c_int64(int(n_samples)), C.c_int32(int(up)), C.c_int32(int(down)), C.c_int32(int(n_taps)),
                                      C.byref(n_out), C.byref(tile), C.byref(n_tiles), C.byref(tpp)) != 0:
        raise ValueError(_error())
    return int(n_out.value), int(tile.value), int(n_tiles.value), int(tpp.value)


def resample_tile_span(n_samples: int, up: int, down: int, n_taps: int, tile_index: int):
    """(out_first, out_count, in_first, in_count): the outputs workgroup ``tile_index`` of a row writes and the inputs it
    stages (host only, the launcher's own arithmetic).  ``in_first`` may be negative and the span may pass ``n_samples``."""
    of, oc, i_f, ic = C.c_int64(), C.c_int32(), C.c_int64(), C.c_int32()
    if _lib.lib().cmoop_resample_tile_span(C.c_int64(int(n_samples)), C.c_int32(int(up)), C.c_int32(int(down)), C.c_int32(int(n_taps)),
                                           C.c_int64(int(tile_index)), C.byref(of), C.byref(oc), C.byref(i_f), C.byref(ic)) != 0:
        raise ValueError(_error())
    return int(of.value), int(oc.value), int(i_f.value), int(ic.value)


def resample_reference(x, up: int, down: int, taps, dtype=np.float64) -> np.ndarray:
    """Host numpy: the definition above along the last axis of ``x [..., L]``, vectorised over the outputs, every operation in
    ``dtype``, terms in ascending ``i``; float32 is the plain restatement of the device arithmetic without its fused update."""
    up, down = int(up), int(down)
    if up < 1 or down < 1 or math.gcd(up, down) != 1:
        raise ValueError("resample: up / down must be positive and reduced")
    dt = np.dtype(dtype).type
    x, h = np.asarray(x, dtype=dt), np.asarray(taps, dtype=dt).reshape(-1)
    if x.ndim < 1 or x.shape[-1] < 1 or h.size % 2 != 1:
        raise ValueError("resample: x must be [..., L] with L >= 1 and n_taps odd")
    L, n_taps = x.shape[-1], h.size
    half, tpp = (n_taps - 1) // 2, -(-n_taps // up)
    n_out = -(-L * up // down)
    pos = np.arange(n_out, dtype=np.int64) * down + half
    first = pos // up - tpp + 1
    out = np.zeros(x.shape[:-1] + (n_out,), dt)
    for j in range(tpp):
        i = first + j
        k = pos - i * up
        ok = (i >= 0) & (i < L) & (k >= 0) & (k < n_taps)
        term = x[..., np.where(ok, i, 0)] * np.where(ok, h[np.where(ok, k, 0)], dt(0))
        out = out + np.where(ok, term, dt(0))
    assert out.dtype == np.dtype(dtype)
    return out


def _default_taps(up: int, down: int, sr_in, sr_out) -> np.ndarray:
    """The default filter of a ratio, after the host check that it is within the taps-per-output domain."""
    n_taps = 20 * max(up, down) + 1
    if -(-n_taps // up) > MAX_TAPS_PER_OUTPUT:
        raise ValueError(f"resample: the ratio sr_in / sr_out = {sr_in} / {sr_out} (down / up = {down} / {up}) is outside the default "
                         f"filter's domain, down <= 12 up ({-(-n_taps // up)} taps per output, at most {MAX_TAPS_PER_OUTPUT})")
    return resample_filter(up, down)


def resample_poly(wav, sr_in, sr_out, taps=None):
    """wav: CUDA float32 ``[N, L]`` or ``[L]`` at ``sr_in`` -> CUDA float32 ``[N, n_out]`` or ``[n_out]`` at ``sr_out``,
    ``n_out = ceil(L up / down)``: ``scipy.signal.resample_poly(wav, up, down, axis=-1)`` with its default filter, or with
    ``taps`` (any odd number of float32 values).  Equal rates without ``taps`` return a copy and launch nothing."""
    import torch
    up, down = rational(sr_in, sr_out)
    if taps is None:
        h = None if up == down else _default_taps(up, down, sr_in, sr_out)
    else:
        h = np.ascontiguousarray(np.asarray(taps, np.float32).reshape(-1))
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() in (1, 2)):
        raise ValueError("resample_poly expects a CUDA float32 tensor [n_clips, n_samples] or [n_samples]")
    wav = wav.contiguous()
    if h is None:
        return wav.clone()
    n, L = (1 if wav.dim() == 1 else int(wav.shape[0])), int(wav.shape[-1])
    if L < 1:
        raise ValueError("resample: n_samples must be at least 1 (got 0)")
    n_out = resample_plan(L, up, down, h.size)[0]
    out = torch.empty((n_out,) if wav.dim() == 1 else (n, n_out), dtype=torch.float32, device=wav.device)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_resample(_lib.ptr(wav), C.c_int64(n), C.c_int64(L), C.c_int32(up), C.c_int32(down), _lib.ptr(h),
                                         C.c_int32(h.size), _lib.ptr(out)))
    return out


def to_rate(wav, sr, sr_model, who: str):
    """``wav`` unchanged when ``sr`` is None or equals ``sr_model``, else ``resample_poly(wav, sr, sr_model)``; a non-positive or
    non-integer ``sr`` raises ValueError (what the ``sr=`` keyword of the front end calls and ``StreamScorer.score`` does)."""
    if sr is None:
        return wav
    if isinstance(sr, bool) or not isinstance(sr, numbers.Integral) or int(sr) < 1:
        raise ValueError(f"{who}: sr must be a positive integer sample rate (got {sr!r})")
    if int(sr) == int(sr_model):
        return wav
    return resample_poly(wav, int(sr), int(sr_model))
