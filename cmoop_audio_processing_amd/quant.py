"""Quantisation-aware training: int8 (or narrower) per-channel weights inside the train step, their size and their export.

Opt-in and off by default (the reference trains and sizes an fp32 model: everything here is BUILD-DEFINED; ``include/cmoop.h``
fixes the semantics at ``cmoop_quant``).  Symmetric, per-output-channel, weight-only fake quantisation of every kernel tensor;
``bits`` in 2..8, ``qmax = 2**(bits-1) - 1``.  Per channel with elements ``w_i``:

* ``a`` = the float whose bits are ``max_i (bits(w_i) & 0x7FFFFFFF)`` as uint32 (a NaN outranks inf and propagates);
* ``s = a / float32(qmax)``, one float32 division;
* ``s > 0`` false: every code is 0; else ``q_i = int8(clamp(rint(w_i / s), -qmax, qmax))``, a NaN quotient being code 0;
* ``wq_i = float32(q_i) * s``, one float32 product; a NaN scale or product is stored as the quiet NaN ``0x7FC00000``.

The gradients formed with ``wq`` go unchanged to the latent ``w`` (straight-through; the absmax scale never clips, so there
is no mask).  Activations stay fp32.  ``fake_quant_ref`` (numpy float32, one rounding per operation) is the statement the
kernel is tested against; no accuracy figure is measured or claimed.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, Tuple

import numpy as np

from . import _lib, genes as G

QuantStruct = _lib.Quant            # cmoop_quant (include/cmoop.h)
CANONICAL_NAN = np.uint32(0x7FC00000)


@dataclasses.dataclass(frozen=True)
class QuantConfig:
    """Mirrors ``cmoop_quant``.  Domain: ``bits`` 0 (off) or 2..8; ``objective`` a bool: the evaluator puts the quantised
    size in the place of ``size_mb`` in ``objs`` and in the size constraint (False only adds the numbers)."""
    bits: int = 8
    objective: bool = True

    @property
    def enabled(self) -> bool:
        return int(self.bits) != 0

    def _struct(self) -> QuantStruct:
        st = QuantStruct()
        st.bits, st.objective = int(self.bits), int(self.objective)
        st.reserved[0] = st.reserved[1] = 0
        return st

    def check(self) -> "QuantConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        return check_struct(self._struct(), self)


def check_struct(st: QuantStruct, ret=None):
    L = _lib.lib()
    if L.cmoop_quant_check(C.byref(st)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_quant_config() -> QuantConfig:
    """cmoop_quant_default as a QuantConfig: off."""
    st = QuantStruct()
    _lib.check(_lib.lib().cmoop_quant_default(C.byref(st)))
    return QuantConfig(bits=int(st.bits), objective=bool(st.objective))


def qmax_of(bits: int) -> int:
    if not 2 <= int(bits) <= 8:
        raise ValueError("bits must be in [2, 8]")
    return (1 << (int(bits) - 1)) - 1


def fake_quant_ref(w, bits: int):
    """The definition restated in numpy: ``w`` float32 [channels, len], one channel per row -> (absmax float32 [channels],
    scales float32 [channels], codes int8 [channels, len], wq float32 [channels, len]).  One IEEE single operation per line."""
    f = np.float32
    w = np.ascontiguousarray(w, f)
    if w.ndim != 2:
        raise ValueError("fake_quant_ref expects [channels, len]")
    qmax = f(qmax_of(bits))
    mag = w.view(np.uint32) & np.uint32(0x7FFFFFFF)
    a = (mag.max(axis=1) if w.shape[1] else np.zeros(w.shape[0], np.uint32)).astype(np.uint32).view(f)
    with np.errstate(all="ignore"):
        s = (a / qmax).astype(f)
        s.view(np.uint32)[np.isnan(s)] = CANONICAL_NAN
        live = s > 0                                   # false for 0, an underflowed quotient and NaN
        r = np.zeros_like(w)
        if live.any():
            r[live] = np.rint((w[live] / s[live, None]).astype(f))
        r[np.isnan(r)] = 0                             # inf / inf
        q = np.clip(r, -qmax, qmax).astype(np.int32)
        wq = (q.astype(f) * s[:, None]).astype(f)
        wq.view(np.uint32)[np.isnan(wq)] = CANONICAL_NAN
    return a, s, q.astype(np.int8), wq


def quant_table(gene, variant: int, classes: int) -> List[Tuple[int, int, int, int, int]]:
    """[(off, channels, len, chan_stride, elem_stride)] of the kernel tensors of a candidate in arena order, from
    ``genes.param_tensors``: channel c holds the elements ``off + c * chan_stride + t * elem_stride``, t < len.  The twin of
    ``cmoop_quant_table``."""
    rows, off = [], 0
    for name, shape, role in G.param_tensors(gene, variant, classes):
        n = int(np.prod(shape))
        if role == "kernel":
            if name.endswith("/depthwise_kernel"):
                rows.append((off, int(shape[2]), int(shape[0] * shape[1]), 1, int(shape[2])))
            else:
                ln = n // int(shape[0])
                rows.append((off, int(shape[0]), ln, ln, 1))
        off += n
    return rows


def c_quant_table(gene, variant: int, classes: int):
    """``cmoop_quant_table``: (rows as ``quant_table`` gives them, total channels)."""
    g, cap = (C.c_int32 * 6)(*(int(v) for v in gene)), 128
    rows, n, tc = np.zeros((cap, 5), np.int64), C.c_int32(), C.c_int64()
    _lib.check(_lib.lib().cmoop_quant_table(g, C.c_int32(int(variant)), C.c_int32(int(classes)), _lib.ptr(rows), C.c_int32(cap),
                                            C.byref(n), C.byref(tc)))
    return [tuple(int(v) for v in r) for r in rows[:n.value]], int(tc.value)


def c_quant_size_bytes(gene, variant: int, classes: int, bits: int) -> int:
    """``cmoop_quant_size_bytes``."""
    g, out = (C.c_int32 * 6)(*(int(v) for v in gene)), C.c_int64()
    _lib.check(_lib.lib().cmoop_quant_size_bytes(g, C.c_int32(int(variant)), C.c_int32(int(classes)), C.c_int32(int(bits)), C.byref(out)))
    return int(out.value)


def channel_view(flat: np.ndarray, row) -> np.ndarray:
    """The [channels, len] view (no copy) of one table row's tensor inside a flat arena."""
    off, ch, ln, cs, es = row
    item = flat.itemsize
    return np.lib.stride_tricks.as_strided(flat[off:], shape=(ch, ln), strides=(cs * item, es * item))


def quantize_table_ref(flat, rows, bits: int):
    """``fake_quant_ref`` over the tensors of ``rows`` inside the float32 arena ``flat`` -> (wq_flat: kernels dequantised, every
    other element a bit copy; codes int8 [len(flat)]: 0 outside the tensors; scales float32 [total channels], in row order)."""
    flat = np.ascontiguousarray(flat, np.float32).reshape(-1)
    wq, codes, scales = flat.copy(), np.zeros(flat.size, np.int8), []
    for row in rows:
        _a, s, q, x = fake_quant_ref(channel_view(flat, row), bits)
        channel_view(wq, row)[...] = x
        channel_view(codes, row)[...] = q
        scales.append(s)
    return wq, codes, (np.concatenate(scales) if scales else np.zeros(0, np.float32)).astype(np.float32)


def quantize_params_ref(flat, gene, variant: int, classes: int, bits: int):
    """The quantised arena of a candidate's parameters ``flat`` -> (wq_flat, codes, scales), as ``NetSession.get_quantized``."""
    flat = np.ascontiguousarray(flat, np.float32).reshape(-1)
    if flat.size != G.param_count(gene, variant, classes):
        raise ValueError("flat does not hold the candidate's parameters")
    return quantize_table_ref(flat, quant_table(gene, variant, classes), bits)


def dequantize(codes, scales, rows, like=None):
    """``float32(codes) * scales`` per channel at the tensors of ``rows``, one float32 product, a NaN as 0x7FC00000; every other
    element from ``like`` (zeros when None).  What ``TrainedModel`` checks its ``params`` against."""
    codes = np.ascontiguousarray(codes, np.int8).reshape(-1)
    scales = np.ascontiguousarray(scales, np.float32).reshape(-1)
    out = np.zeros(codes.size, np.float32) if like is None else np.array(like, np.float32).reshape(-1)
    pos = 0
    for row in rows:
        s = scales[pos:pos + row[1]]
        pos += row[1]
        with np.errstate(all="ignore"):
            x = (channel_view(codes, row).astype(np.float32) * s[:, None]).astype(np.float32)
        x.view(np.uint32)[np.isnan(x)] = CANONICAL_NAN
        channel_view(out, row)[...] = x
    if pos != scales.size:
        raise ValueError(f"scales holds {scales.size} values, the kernel tensors have {pos} channels")
    return out


def quantize_weights(w, rows, bits: int, wq, codes=None, scales=None) -> None:
    """``cmoop_quantize_weights``: the kernel alone.  ``w`` / ``wq`` CUDA float32 [n], ``codes`` CUDA int8 [n] or None, ``scales``
    CUDA float32 [total channels] or None; ``rows`` as ``quant_table`` gives them."""
    import torch
    st = QuantConfig(bits=int(bits)).check()._struct()
    tab = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 5))
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_quantize_weights(C.byref(st), _lib.ptr(w), C.c_int64(int(w.numel())), _lib.ptr(tab), C.c_int32(len(tab)),
                                                 _lib.ptr(wq), _lib.ptr(codes), _lib.ptr(scales)))


def quantize_weights_time(w, rows, bits: int, wq, iters: int = 100) -> float:
    """``cmoop_quantize_weights_time``: average milliseconds of the launch."""
    import torch
    st = QuantConfig(bits=int(bits)).check()._struct()
    tab = np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 5))
    ms = C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_quantize_weights_time(C.byref(st), _lib.ptr(w), C.c_int64(int(w.numel())), _lib.ptr(tab),
                                                      C.c_int32(len(tab)), _lib.ptr(wq), None, None, C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)
