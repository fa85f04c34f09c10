"""Quantisation-aware training: int8 (or narrower) per-channel weights inside the train step, their size and their export.

Opt-in and off by default (the reference trains and sizes an fp32 model: everything here is BUILD-DEFINED; ``include/cmoop.h``
fixes the semantics at ``cmoop_quant``).  Symmetric, per-output-channel, weight-only fake quantisation of every kernel tensor;
``bits`` in 2..8, ``qmax = 2**(bits-1) - 1``.  Per channel with elements ``w_i``:

* ``a`` = the float whose bits are ``max_i (bits(w_i) & 0x7FFFFFFF)`` as uint32 (a NaN outranks inf and propagates);
* ``s = a / float32(qmax)``, one float32 division;
* ``s > 0`` false: every code is 0; else ``q_i = int8(clamp(rint(w_i / s), -qmax, qmax))``, a NaN quotient being code 0;
* ``wq_i = float32(q_i) * s``, one float32 product; a NaN scale or product is stored as the quiet NaN ``0x7FC00000``.

The gradients formed with ``wq`` go unchanged to the latent ``w`` (straight-through; the absmax scale never clips, so there
is no mask).  Under ``QuantConfig`` activations stay fp32.  ``fake_quant_ref`` (numpy float32, one rounding per operation) is
the statement the kernel is tested against; no accuracy figure is measured or claimed.

``ActQuantConfig`` is the separate, opt-in activation quantiser (``cmoop_actquant``): the same element arithmetic on ONE
channel that spans a whole activation tensor, at the operand tensors of every MAC layer and of the global pool.  Train steps
take the batch's own absmax (never clips) and track it with a momentum; inference takes the tracked range (clips).
``fake_quant_act_ref`` / ``act_range_update_ref`` / ``act_sites`` are its numpy statements.

Integer inference (``NetSession.set_int8``; ``include/cmoop.h``, "Integer inference") executes a model trained under both: the
conv and dense layers whose input is a site multiply int8 codes, accumulate exactly in int32 and dequantise once per output.
``conv_i8_ref`` / ``dense_i8_ref`` / ``act_codes_ref`` / ``int8_ops`` are its numpy statements.  Its opt-in second level
(``NetSession.set_int8(True, depthwise=True)``; "Integer depthwise") runs the depthwise half of every separable layer on the
codes as well, in one launch that also applies the quantiser of the site it writes: ``dwconv_i8_acc`` / ``dwconv_i8_ref`` /
``int8_dw_ops`` state it.  Its opt-in third level (``NetSession.set_int8(True, fused=True)``; "Integer inference: requantising
epilogue") gives the conv and dense launches the tail of their op -- the eval BatchNorm as one fma, its ReLU and the quantiser of
the site written -- so they emit the next layer's codes themselves: ``fma32_ref`` / ``conv_i8_q_ref`` / ``dense_i8_q_ref`` /
``int8_fused_ops`` state it.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import List, NamedTuple, Tuple

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
    mag = w.view(np.uint32) & np.uint32(0x7FFFFFFF)
    a = (mag.max(axis=1) if w.shape[1] else np.zeros(w.shape[0], np.uint32)).astype(np.uint32).view(f)
    s, q, wq = _quant_elements(w, a, bits)
    return a, s, q, wq


def _quant_elements(w, a, bits: int):
    """THE element arithmetic of both fake quantisers: ``w`` float32 [channels, len] under the ranges ``a`` float32 [channels]
    -> (scales, codes int8, wq).  One IEEE single operation per line."""
    f = np.float32
    qmax = f(qmax_of(bits))
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
    return s, q.astype(np.int8), wq


# ---- activation fake quantisation (include/cmoop.h fixes the semantics at cmoop_actquant) -------------------------------
ActQuantStruct = _lib.ActQuant      # cmoop_actquant
ActRangeStruct = _lib.ActRange      # cmoop_act_range
ACT_RANGE_DTYPE = np.dtype([("m_b", np.float32), ("r", np.float32), ("count", np.int32), ("reserved", np.int32)])


@dataclasses.dataclass(frozen=True)
class ActQuantConfig:
    """Mirrors ``cmoop_actquant``: per-tensor, symmetric, signed fake quantisation of the operand tensors of every MAC layer
    and of the global pool, inside the train step (batch ranges, tracked with ``momentum``) and every inference pass (tracked
    ranges).  Domain: ``bits`` 0 (off) or 2..8; ``momentum`` in [0, 1).  Build-defined; no accuracy figure is claimed."""
    bits: int = 8
    momentum: float = 0.99

    @property
    def enabled(self) -> bool:
        return int(self.bits) != 0

    def _struct(self) -> ActQuantStruct:
        st = ActQuantStruct()
        st.bits, st.momentum = int(self.bits), float(self.momentum)
        st.reserved[0] = st.reserved[1] = 0
        return st

    def check(self) -> "ActQuantConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        return check_act_struct(self._struct(), self)


def check_act_struct(st: ActQuantStruct, ret=None):
    L = _lib.lib()
    if L.cmoop_actquant_check(C.byref(st)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_act_quant_config() -> ActQuantConfig:
    """cmoop_actquant_default as an ActQuantConfig: off, momentum 0.99 as float32 holds it."""
    st = ActQuantStruct()
    _lib.check(_lib.lib().cmoop_actquant_default(C.byref(st)))
    return ActQuantConfig(bits=int(st.bits), momentum=float(st.momentum))


def fake_quant_act_ref(x, bits: int, a=None):
    """The operator restated in numpy: ``x`` float32 of any shape, ONE channel that spans the whole tensor -> (a float32: the
    range that was used, y float32 in the shape of ``x``).  ``a`` None: batch mode, the tensor's own absmax; else tracked
    mode under that range (the clamp then works).  The element arithmetic is ``fake_quant_ref``'s."""
    x = np.ascontiguousarray(x, np.float32)
    flat = x.reshape(1, -1)
    if a is None:
        mag = flat.view(np.uint32) & np.uint32(0x7FFFFFFF)
        a = (mag.max(axis=1) if flat.shape[1] else np.zeros(1, np.uint32)).astype(np.uint32).view(np.float32)
    else:
        a = np.asarray([a], np.float32)
    _s, _q, y = _quant_elements(flat, a, bits)
    return a[0], y.reshape(x.shape)


def act_codes_ref(x, bits: int, a):
    """The codes of ``fake_quant_act_ref`` in tracked mode under the range ``a``: int8 in the shape of ``x``, with
    ``float32(codes) * s == fake_quant_act_ref(x, bits, a)[1]`` bit for bit, ``s = act_scale_ref(a, bits)``."""
    x = np.ascontiguousarray(x, np.float32)
    _s, q, _y = _quant_elements(x.reshape(1, -1), np.asarray([a], np.float32), bits)
    return q.reshape(x.shape)


def act_scale_ref(a, bits: int):
    """``s_x = a / float32(qmax)``: the tracked-mode scale of a site with range ``a`` (a NaN as 0x7FC00000)."""
    s = np.asarray([a], np.float32)
    with np.errstate(all="ignore"):
        s = (s / np.float32(qmax_of(bits))).astype(np.float32)
    s.view(np.uint32)[np.isnan(s)] = CANONICAL_NAN
    return s[0]


# ---- integer inference (include/cmoop.h fixes the arithmetic at "Integer inference") ------------------------------------
def i8_epilogue_ref(acc, s_x, s_w, bias, relu):
    """``fl(fl(float32(acc) * fl(s_x * s_w[c])) + bias[c])``, then ``max(y, 0)``: acc int64 [..., C], one IEEE single operation
    per line.  The ReLU is the fp32 epilogues' fmaxf(y, 0): a NaN becomes 0 and a zero result is +0.0."""
    f = np.float32
    acc = np.asarray(acc, np.int64)
    if acc.size and int(np.abs(acc).max()) >= 2 ** 31:
        raise ValueError("an accumulator left int32")
    with np.errstate(all="ignore"):
        sc = (f(s_x) * np.asarray(s_w, f)).astype(f)
        y = (acc.astype(np.int32).astype(f) * sc).astype(f)            # int32 -> float32 rounds to nearest even
        y = (y + np.asarray(bias, f)).astype(f)
        if relu:
            y = np.where(y > 0, y, f(0)).astype(f)
    return y


def conv_i8_acc(qx, qw, KS: int, stride: int) -> np.ndarray:
    """The exact accumulators of ``conv_i8_ref``, int64 [B, OH, OW, Cout] (of absolute codes: the sum a rounding bound scales)."""
    qx = np.asarray(qx, np.int8)
    B, H, W, Cin = qx.shape
    qw = np.asarray(qw, np.int8).reshape(-1, KS, KS, Cin)
    Cout = qw.shape[0]
    OH, OW = (H + stride - 1) // stride, (W + stride - 1) // stride
    pt, pl = max((OH - 1) * stride + KS - H, 0) // 2, max((OW - 1) * stride + KS - W, 0) // 2
    xp = np.zeros((B, max((OH - 1) * stride + KS, pt + H), max((OW - 1) * stride + KS, pl + W), Cin), np.int64)
    xp[:, pt:pt + H, pl:pl + W] = qx
    acc = np.zeros((B, OH, OW, Cout), np.int64)
    for kh in range(KS):
        for kw in range(KS):
            win = xp[:, kh:kh + (OH - 1) * stride + 1:stride, kw:kw + (OW - 1) * stride + 1:stride]
            acc += win.reshape(-1, Cin).dot(qw[:, kh, kw].astype(np.int64).T).reshape(B, OH, OW, Cout)
    return acc


def conv_i8_ref(qx, qw, s_x, s_w, bias, KS: int, stride: int, relu) -> np.ndarray:
    """The integer conv layer restated: ``qx`` int8 [B, H, W, Cin], ``qw`` int8 [Cout, KS, KS, Cin] (or [Cout, KS*KS*Cin]),
    ``s_w`` / ``bias`` float32 [Cout] -> float32 [B, ceil(H/stride), ceil(W/stride), Cout].  SAME padding (TF: total // 2 on
    the top / left) contributes 0; the sum is exact (int64), the epilogue float32."""
    return i8_epilogue_ref(conv_i8_acc(qx, qw, KS, stride), s_x, s_w, bias, relu)


def dense_i8_ref(qx, qw, s_x, s_w, bias, relu) -> np.ndarray:
    """The integer dense layer restated: ``qx`` int8 [M, K], ``qw`` int8 [N, K] -> float32 [M, N]."""
    acc = np.asarray(qx, np.int8).astype(np.int64).dot(np.asarray(qw, np.int8).astype(np.int64).T)
    return i8_epilogue_ref(acc, s_x, s_w, bias, relu)


INT8_OP_FIELDS = ("op", "kind", "in_act", "out_act", "site", "H", "W", "Cin", "Cout", "KS", "stride", "relu", "w_off", "b_off",
                  "scale_off")


def int8_ops(hparams, variant, classes: int, T: int, F: int) -> List[Tuple[int, int, int]]:
    """[(op index, input act, output act)] of the ops that run integer under ``NetSession.set_int8``, the rule restated on
    ``act_plan``: every conv / dense op whose input is an activation-quantisation site.  The twin of ``cmoop_int8_ops``."""
    _acts, ops, _logits = act_plan(hparams, variant, classes, T, F)
    sites = {s[0] for s in act_sites(hparams, variant, classes, T, F)}
    return [(i, op[1], op[3]) for i, op in enumerate(ops) if op[0] in ("conv", "dense") and op[1] in sites]


class Int8Levels(NamedTuple):
    """The three levels of integer inference as one value: integer inference itself, its depthwise level, its requantising
    epilogue.  THE place of "a level needs ``on``"."""
    on: bool = False
    depthwise: bool = False
    fused: bool = False

    @classmethod
    def of(cls, on, depthwise, fused, refusals) -> "Int8Levels":
        """The checked record.  ``refusals``: the caller's two ValueError texts, in its own keywords -- (depthwise without on,
        fused without on)."""
        if depthwise and not on:
            raise ValueError(refusals[0])
        if fused and not on:
            raise ValueError(refusals[1])
        return cls(bool(on), bool(depthwise), bool(fused))


def _plan_rows(fields, rows, n):
    """The first ``n`` plan rows of any level as dicts keyed by ``fields`` (a row's trailing zero column has no field)."""
    return [dict(zip(fields, (int(v) for v in r))) for r in rows[:n]]


def _c_plan_ops(entry: str, fields, width: int, gene, variant: int, classes: int, T: int, F: int, cap: int):
    """``cmoop_int8_ops`` / ``cmoop_int8_dw_ops`` / ``cmoop_int8_fused_ops`` by name: the plan rows of a gene (``width`` int64
    columns each), keyed by ``fields``."""
    g = (C.c_int32 * 6)(*(int(v) for v in gene))
    rows, n = np.zeros((max(int(cap), 1), int(width)), np.int64), C.c_int32()
    _lib.check(getattr(_lib.lib(), entry)(g, C.c_int32(int(variant)), C.c_int32(int(classes)), C.c_int32(int(T)), C.c_int32(int(F)),
                                          _lib.ptr(rows), C.c_int32(int(cap)), C.byref(n)))
    return _plan_rows(fields, rows, n.value)


def c_int8_ops(gene, variant: int, classes: int, T: int, F: int):
    """``cmoop_int8_ops``: a list of dicts keyed by ``INT8_OP_FIELDS`` (kind 0: conv, 1: dense)."""
    return _c_plan_ops("cmoop_int8_ops", INT8_OP_FIELDS, 16, gene, variant, classes, T, F, 64)


def _dev_ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def conv_fwd_i8(xq, wq, s_x, s_w, bias, y, B, H, W, Cin, Cout, KS, stride, relu) -> None:
    """``cmoop_conv_fwd_i8``: the lone integer conv layer.  ``xq`` / ``wq`` CUDA int8 (16-byte aligned views), ``s_w`` /
    ``bias`` / ``y`` CUDA float32."""
    import torch
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_conv_fwd_i8(_dev_ptr(xq), _dev_ptr(wq), C.c_float(float(s_x)), _dev_ptr(s_w), _dev_ptr(bias), _dev_ptr(y),
                                            *(C.c_int32(int(v)) for v in (B, H, W, Cin, Cout, KS, stride, relu))))


def dense_fwd_i8(xq, wq, s_x, s_w, bias, y, M, N, K, relu) -> None:
    """``cmoop_dense_fwd_i8``: the lone integer dense layer."""
    import torch
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_dense_fwd_i8(_dev_ptr(xq), _dev_ptr(wq), C.c_float(float(s_x)), _dev_ptr(s_w), _dev_ptr(bias), _dev_ptr(y),
                                             *(C.c_int32(int(v)) for v in (M, N, K, relu))))


def conv_fwd_i8_time(xq, wq, s_x, s_w, bias, y, B, H, W, Cin, Cout, KS, stride, relu, iters: int = 50) -> float:
    """``cmoop_conv_fwd_i8_time``: average milliseconds of the launch."""
    import torch
    ms = C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_conv_fwd_i8_time(_dev_ptr(xq), _dev_ptr(wq), C.c_float(float(s_x)), _dev_ptr(s_w), _dev_ptr(bias),
                                                 _dev_ptr(y), *(C.c_int32(int(v)) for v in (B, H, W, Cin, Cout, KS, stride, relu, iters)),
                                                 C.byref(ms)))
    return float(ms.value)


# ---- the requantising epilogue: the third level (include/cmoop.h, "Integer inference: requantising epilogue") -----------------
# For a conv / dense op of int8_ops whose output reaches a site through per-channel elementwise ops only (int8_fused_ops):
#     t    = i8_epilogue_ref(acc, s_x, s_w, bias, relu)                                       today's epilogue, unchanged
#     t    = fma32_ref(t, scale[c], shift[c]), then max(t, 0) under relu_after                only with a BatchNorm; ONE rounding
#     q, y = the tracked-mode code and dequantised value of t under the range of the site written (_quant_elements, unchanged)
def fma32_ref(a, b, c) -> np.ndarray:
    """The correctly rounded float32 ``a * b + c`` (ONE rounding), elementwise with broadcasting.  The product of two float32 is
    exact in float64 (48 bits); ``c`` is added with a TwoSum and the float64 sum is rounded to odd when the error term is
    non-zero; 53 >= 2 * 24 + 2, so the cast of that sum to float32 is the correctly rounded result."""
    f8 = np.float64
    with np.errstate(all="ignore"):
        p = np.asarray(a, np.float32).astype(f8) * np.asarray(b, np.float32).astype(f8)
        cc = np.broadcast_to(np.asarray(c, np.float32).astype(f8), p.shape)
        s = p + cc
        bb = s - p
        e = (p - (s - bb)) + (cc - bb)                                   # s + e == p + c exactly (finite operands)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((np.ascontiguousarray(s).view(np.uint64) & np.uint64(1)) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, f8(np.inf), f8(-np.inf))), s)
        return s.astype(np.float32)


def i8_requant_ref(t, bn_scale=None, bn_shift=None, relu_after=0, out_bits=None, a_out=None):
    """The tail of the requantising epilogue on ``t`` float32 [..., C] (what ``i8_epilogue_ref`` returns) -> ``(y, codes)``."""
    f = np.float32
    if (bn_scale is None) != (bn_shift is None):
        raise ValueError("bn_scale and bn_shift come together or not at all")
    if out_bits is None or a_out is None:
        raise ValueError("the site written needs out_bits and a_out")
    t = np.asarray(t, f)
    if bn_scale is not None:
        t = fma32_ref(t, np.asarray(bn_scale, f), np.asarray(bn_shift, f))
        if relu_after:
            with np.errstate(all="ignore"):
                t = np.where(t > 0, t, f(0)).astype(f)                  # fmaxf(t, 0): a NaN becomes 0
    return fake_quant_act_ref(t, out_bits, a_out)[1], act_codes_ref(t, out_bits, a_out)


def conv_i8_q_ref(qx, qw, s_x, s_w, bias, KS: int, stride: int, relu, bn_scale=None, bn_shift=None, relu_after=0, out_bits=None,
                  a_out=None):
    """The requantising integer conv layer restated: ``conv_i8_ref``'s operands, the eval BatchNorm vectors (both None: no
    BatchNorm) and the range ``a_out`` of the site written at ``out_bits`` -> ``(y float32, codes int8)``, both
    [B, OH, OW, Cout]."""
    t = i8_epilogue_ref(conv_i8_acc(qx, qw, KS, stride), s_x, s_w, bias, relu)
    return i8_requant_ref(t, bn_scale, bn_shift, relu_after, out_bits, a_out)


def dense_i8_q_ref(qx, qw, s_x, s_w, bias, relu, bn_scale=None, bn_shift=None, relu_after=0, out_bits=None, a_out=None):
    """The requantising integer dense layer restated: ``dense_i8_ref``'s operands and ``conv_i8_q_ref``'s tail -> ``(y, codes)``
    [M, N]."""
    return i8_requant_ref(dense_i8_ref(qx, qw, s_x, s_w, bias, relu), bn_scale, bn_shift, relu_after, out_bits, a_out)


def dense_fwd_i8_time(xq, wq, s_x, s_w, bias, y, M, N, K, relu, iters: int = 50) -> float:
    """``cmoop_dense_fwd_i8_time``: average milliseconds of ``dense_fwd_i8``'s launch."""
    import torch
    ms = C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_dense_fwd_i8_time(_dev_ptr(xq), _dev_ptr(wq), C.c_float(float(s_x)), _dev_ptr(s_w), _dev_ptr(bias), _dev_ptr(y),
                                                  *(C.c_int32(int(v)) for v in (M, N, K, relu, iters)), C.byref(ms)))
    return float(ms.value)


def scale_shift_time(x, y, scale, shift, M, Cn, relu, iters: int = 50) -> float:
    """``cmoop_scale_shift_time``: average milliseconds of the eval BatchNorm's apply launch alone."""
    import torch
    ms = C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_scale_shift_time(_dev_ptr(x), _dev_ptr(y), _dev_ptr(scale), _dev_ptr(shift), C.c_int64(int(M)),
                                                 *(C.c_int32(int(v)) for v in (Cn, relu, iters)), C.byref(ms)))
    return float(ms.value)


INT8_FUSED_OP_FIELDS = INT8_OP_FIELDS + ("zero", "bn_op", "relu_after", "out_site", "site_act")


def int8_fused_ops(hparams, variant, classes: int, T: int, F: int) -> List[Tuple[int, int, int, int, int, int]]:
    """[(op index, input act, output act, BatchNorm op index or -1, relu_after, act written)] of the ops that take the
    requantising epilogue under ``NetSession.set_int8(True, fused=True)``, the rule restated on ``act_plan``: an op of
    ``int8_ops`` whose own output act is a site (T0), or whose output is read by one op only, a BatchNorm whose output is
    materialised (no fused pool) and a site (T1).  Such a BatchNorm is topology A's, which carries the ReLU, so ``relu_after``
    is 1 exactly on the T1 rows.  The twin of ``cmoop_int8_fused_ops``."""
    _acts, ops, _logits = act_plan(hparams, variant, classes, T, F)
    sites = {s[0] for s in act_sites(hparams, variant, classes, T, F)}
    out = []
    for i, a_in, a_out in int8_ops(hparams, variant, classes, T, F):
        if a_out in sites:
            out.append((i, a_in, a_out, -1, 0, a_out))
            continue
        readers = [j for j, op in enumerate(ops) if a_out in (op[1], op[2])]
        if len(readers) == 1 and ops[readers[0]][0] == "bn" and ops[readers[0]][3] in sites:
            out.append((i, a_in, a_out, readers[0], 1, ops[readers[0]][3]))
    return out


def c_int8_fused_ops(gene, variant: int, classes: int, T: int, F: int, cap: int = 64):
    """``cmoop_int8_fused_ops``: a list of dicts keyed by ``INT8_FUSED_OP_FIELDS`` (``bn_op`` -1: the op's own output is the
    site)."""
    return _c_plan_ops("cmoop_int8_fused_ops", INT8_FUSED_OP_FIELDS, 20, gene, variant, classes, T, F, cap)


def _i8_q_args(xq, wq, s_x, s_w, bias, bn_scale, bn_shift, ints, a_out, y, codes):
    a = C.c_float(float(a_out)) if a_out is not None else None
    return a, (_dev_ptr(xq), _dev_ptr(wq), C.c_float(float(s_x)), _dev_ptr(s_w), _dev_ptr(bias), _dev_ptr(bn_scale), _dev_ptr(bn_shift),
               *(C.c_int32(int(v)) for v in ints), C.byref(a) if a is not None else None, _dev_ptr(y), _dev_ptr(codes))


def conv_fwd_i8_q(xq, wq, s_x, s_w, bias, y, codes, B, H, W, Cin, Cout, KS, stride, relu, out_bits, a_out, bn_scale=None,
                  bn_shift=None, relu_after=0) -> None:
    """``cmoop_conv_fwd_i8_q``: the lone requantising conv layer.  ``conv_fwd_i8``'s operands; ``y`` CUDA float32 (16-byte
    aligned) and ``codes`` CUDA int8 receive the site's dequantised values and codes under ``a_out`` at ``out_bits``;
    ``bn_scale`` / ``bn_shift`` CUDA float32 [Cout] or both None."""
    import torch
    _a, args = _i8_q_args(xq, wq, s_x, s_w, bias, bn_scale, bn_shift, (B, H, W, Cin, Cout, KS, stride, relu, relu_after, out_bits), a_out,
                          y, codes)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_conv_fwd_i8_q(*args))


def conv_fwd_i8_q_time(xq, wq, s_x, s_w, bias, y, codes, B, H, W, Cin, Cout, KS, stride, relu, out_bits, a_out, bn_scale=None,
                       bn_shift=None, relu_after=0, iters: int = 50) -> float:
    """``cmoop_conv_fwd_i8_q_time``: average milliseconds of the launch."""
    import torch
    ms = C.c_double()
    _a, args = _i8_q_args(xq, wq, s_x, s_w, bias, bn_scale, bn_shift, (B, H, W, Cin, Cout, KS, stride, relu, relu_after, out_bits), a_out,
                          y, codes)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_conv_fwd_i8_q_time(*args, C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)


def dense_fwd_i8_q(xq, wq, s_x, s_w, bias, y, codes, M, N, K, relu, out_bits, a_out, bn_scale=None, bn_shift=None,
                   relu_after=0) -> None:
    """``cmoop_dense_fwd_i8_q``: the lone requantising dense layer."""
    import torch
    _a, args = _i8_q_args(xq, wq, s_x, s_w, bias, bn_scale, bn_shift, (M, N, K, relu, relu_after, out_bits), a_out, y, codes)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_dense_fwd_i8_q(*args))


def dense_fwd_i8_q_time(xq, wq, s_x, s_w, bias, y, codes, M, N, K, relu, out_bits, a_out, bn_scale=None, bn_shift=None,
                        relu_after=0, iters: int = 50) -> float:
    """``cmoop_dense_fwd_i8_q_time``: average milliseconds of the launch."""
    import torch
    ms = C.c_double()
    _a, args = _i8_q_args(xq, wq, s_x, s_w, bias, bn_scale, bn_shift, (M, N, K, relu, relu_after, out_bits), a_out, y, codes)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_dense_fwd_i8_q_time(*args, C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)


# ---- integer depthwise: the second level (include/cmoop.h fixes the arithmetic at "Integer depthwise") ------------------------
# For a depthwise layer with input-site scale s_x = r_in / float32(qmax_act), weight codes qw[ky][kx][c], channel scales s_w[c]
# and the tracked range r_out of the site it writes:
#     acc[b,h,w,c] = sum over (ky, kx) of int32(qx[b,h+ky-p,w+kx-p,c]) * int32(qw[ky][kx][c])     p = (K-1)/2, padding taps give 0
#     z            = fl(float32(acc) * fl(s_x * s_w[c]))                                            no bias, no activation
#     q, y         = the tracked-mode code and dequantised value of z under r_out (_quant_elements, unchanged)
# |acc| <= 25 * 127^2 = 403 225 < 2^24: float32(acc) is exact.  Every fl is one float32 operation.  s > 0 false: codes 0, y = +0.0.
def _dw_weights(qw, KS, C):
    qw = np.asarray(qw, np.int8)
    if KS is None:
        if qw.ndim != 3 or qw.shape[0] != qw.shape[1]:
            raise ValueError("depthwise weight codes must be [K, K, C] (or flat with KS given)")
        KS = qw.shape[0]
    if int(KS) not in (3, 5):
        raise ValueError("depthwise kernel size must be 3 or 5")
    return qw.reshape(int(KS), int(KS), C), int(KS)


def dwconv_i8_acc(qx, qw, KS=None) -> np.ndarray:
    """The exact accumulators of ``dwconv_i8_ref``: ``qx`` int8 [B, H, W, C], ``qw`` int8 [K, K, C] (or flat with ``KS``) ->
    int64 [B, H, W, C].  SAME padding, stride 1; a padding tap contributes 0."""
    qx = np.asarray(qx, np.int8)
    B, H, W, Cn = qx.shape
    qw, K = _dw_weights(qw, KS, Cn)
    p = (K - 1) // 2
    xp = np.zeros((B, H + 2 * p, W + 2 * p, Cn), np.int64)
    xp[:, p:p + H, p:p + W] = qx
    acc = np.zeros((B, H, W, Cn), np.int64)
    for ky in range(K):
        for kx in range(K):
            acc += xp[:, ky:ky + H, kx:kx + W] * qw[ky, kx].astype(np.int64)
    return acc


def dwconv_i8_ref(qx, qw, s_x, s_w, KS=None, out_bits=None, a_out=None):
    """The integer depthwise layer restated.  ``a_out`` None: float32 ``z`` [B, H, W, C], the dequantised sums.  ``a_out``
    given: ``(y, codes)`` -- ``fake_quant_act_ref(z, out_bits, a_out)[1]`` and ``act_codes_ref(z, out_bits, a_out)``."""
    f = np.float32
    acc = dwconv_i8_acc(qx, qw, KS)
    with np.errstate(all="ignore"):
        sc = (f(s_x) * np.asarray(s_w, f)).astype(f)
        z = (acc.astype(np.int32).astype(f) * sc).astype(f)            # |acc| < 2^24: the conversion is exact
    if a_out is None:
        return z
    return fake_quant_act_ref(z, out_bits, a_out)[1], act_codes_ref(z, out_bits, a_out)


INT8_DW_OP_FIELDS = INT8_OP_FIELDS + ("out_site",)
INT8_DW_KIND = 2                    # the kind field of a depthwise row (cmoop_int8_ops uses 0: conv, 1: dense)


def int8_dw_ops(hparams, variant, classes: int, T: int, F: int) -> List[Tuple[int, int, int]]:
    """[(op index, input act, output act)] of the ops that run integer under ``NetSession.set_int8(True, depthwise=True)``:
    every depthwise op, the rule restated on ``act_plan``.  The twin of ``cmoop_int8_dw_ops``."""
    _acts, ops, _logits = act_plan(hparams, variant, classes, T, F)
    return [(i, op[1], op[3]) for i, op in enumerate(ops) if op[0] == "dwconv"]


def c_int8_dw_ops(gene, variant: int, classes: int, T: int, F: int, cap: int = 64):
    """``cmoop_int8_dw_ops``: a list of dicts keyed by ``INT8_DW_OP_FIELDS`` (kind 2, b_off -1)."""
    return _c_plan_ops("cmoop_int8_dw_ops", INT8_DW_OP_FIELDS, 16, gene, variant, classes, T, F, cap)


def _dwconv_i8_args(xq, wq, s_x, s_w, B, H, W, Cn, KS, out_bits, a_out, y, codes):
    a = C.c_float(float(a_out)) if a_out is not None else None
    return a, (_dev_ptr(xq), _dev_ptr(wq), C.c_float(float(s_x)), _dev_ptr(s_w),
               *(C.c_int32(int(v)) for v in (B, H, W, Cn, KS, out_bits if out_bits is not None else 0)),
               C.byref(a) if a is not None else None, _dev_ptr(y), _dev_ptr(codes))


def dwconv_fwd_i8(xq, wq, s_x, s_w, y, B, H, W, Cn, KS, out_bits=None, a_out=None, codes=None) -> None:
    """``cmoop_dwconv_fwd_i8``: the lone integer depthwise layer.  ``xq`` [B, H, W, C] / ``wq`` [KS, KS, C] CUDA int8 (16-byte
    aligned views), ``s_w`` / ``y`` CUDA float32.  ``a_out`` None: ``y = z``; else ``y`` and ``codes`` (CUDA int8 or None)
    under that range at ``out_bits``."""
    import torch
    _a, args = _dwconv_i8_args(xq, wq, s_x, s_w, B, H, W, Cn, KS, out_bits, a_out, y, codes)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_dwconv_fwd_i8(*args))


def dwconv_fwd_i8_time(xq, wq, s_x, s_w, y, B, H, W, Cn, KS, out_bits=None, a_out=None, codes=None, iters: int = 50) -> float:
    """``cmoop_dwconv_fwd_i8_time``: average milliseconds of the launch."""
    import torch
    ms = C.c_double()
    _a, args = _dwconv_i8_args(xq, wq, s_x, s_w, B, H, W, Cn, KS, out_bits, a_out, y, codes)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_dwconv_fwd_i8_time(*args, C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)


def fake_quant_act_codes(x, bits: int, a, codes=None) -> None:
    """``cmoop_fake_quant_act_codes``: tracked mode under ``a`` in place on ``x`` (CUDA float32), the codes into ``codes`` (CUDA
    int8 of as many elements, or None: the plain tracked launch)."""
    import torch
    a_in = C.c_float(float(a))
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_fake_quant_act_codes(C.c_void_p(x.data_ptr()), C.c_int64(int(x.numel())), C.c_int32(int(bits)),
                                                     C.byref(a_in), _dev_ptr(codes)))


def fake_quant_act_codes_time(x, bits: int, a, codes=None, iters: int = 50) -> float:
    """``cmoop_fake_quant_act_codes_time``: average milliseconds of ``fake_quant_act_codes``' launch."""
    import torch
    a_in, ms = C.c_float(float(a)), C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_fake_quant_act_codes_time(C.c_void_p(x.data_ptr()), C.c_int64(int(x.numel())), C.c_int32(int(bits)),
                                                          C.byref(a_in), _dev_ptr(codes), C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)


def act_momentum_pair(momentum):
    """(mu, omu) = (float32(momentum), float32(1.0 - float64(float32(momentum)))): what the kernel multiplies by."""
    mu = np.float32(momentum)
    return mu, np.float32(1.0 - np.float64(mu))


def act_range_update_ref(r, m_b, count: int, momentum):
    """The tracked range after a train step whose tensor had absmax ``m_b``: ``m_b`` when ``count == 0``, else
    ``fl(fl(mu * r) + fl(omu * m_b))`` in float32; a NaN in the canonical form."""
    f = np.float32
    m_b = np.asarray(m_b, f).reshape(1).copy()
    m_b.view(np.uint32)[np.isnan(m_b)] = CANONICAL_NAN
    if int(count) == 0:
        return m_b[0]
    mu, omu = act_momentum_pair(momentum)
    with np.errstate(all="ignore"):
        keep = f(mu * f(r))
        add = f(omu * m_b[0])
        out = np.asarray([f(keep + add)], f)
    out.view(np.uint32)[np.isnan(out)] = CANONICAL_NAN
    return out[0]


_MAC_KINDS = ("conv", "dwconv", "dense", "gap")


def act_plan(hparams, variant, classes: int, T: int, F: int):
    """The act / op walk of a candidate, restating plan_net: (acts [(H, W, C, virt)], ops [(kind, in, in2, out)], logits index).
    kinds: conv1, conv, dwconv, bn, pool, addrelu, gap, dense.  ``variant``: a name or a code."""
    g = G.normalize_hparams(hparams) if isinstance(hparams, dict) else tuple(int(v) for v in hparams)
    G.validate_gene(g)
    v = G.VARIANT_NAMES[variant] if isinstance(variant, str) else int(variant)
    f, _k, bn, R, fc, _dr = g
    A, ds = (v & 1) == 0, v >= 2
    acts, ops = [[int(T), int(F), 1, False]], []

    def new(H, W, Cn):
        acts.append([H, W, Cn, False])
        return len(acts) - 1

    def conv(kind, i, cout, stride=1):
        H, W = acts[i][0], acts[i][1]
        o = new((H + stride - 1) // stride, (W + stride - 1) // stride, cout)
        ops.append((kind, i, -1, o))
        return o

    def sepconv(i, cout):
        if not ds:
            return conv("conv", i, cout)
        return conv("conv", conv("dwconv", i, acts[i][2]), cout)

    def bnorm(i):
        o = new(*acts[i][:3])
        ops.append(("bn", i, -1, o))
        return o

    def pool(i, mask_y_pos):
        if ops and ops[-1][0] == "bn" and ops[-1][3] == i and not mask_y_pos:
            acts[i][3] = True                               # fused into the BatchNorm: never materialised
        o = new((acts[i][0] + 1) // 2, (acts[i][1] + 1) // 2, acts[i][2])
        ops.append(("pool", i, -1, o))
        return o

    x = conv("conv1", 0, f)
    if A:
        if bn:
            x = bnorm(x)
        x = sepconv(x, f)
        if bn:
            x = bnorm(x)
        x = pool(x, 0)
    else:
        if bn:
            x = bnorm(x)
        x = pool(x, not bn)
    c = f
    for _ in range(R):
        skip = conv("conv", x, 2 * c, 2)
        y = sepconv(x, 2 * c)
        if A:
            if bn:
                y = bnorm(y)
            y = sepconv(y, 2 * c)
            if bn:
                y = bnorm(y)
            y = pool(y, 0)
        else:
            if bn:
                y = bnorm(y)
            y = pool(y, not bn)
        o = new(*acts[y][:3])
        ops.append(("addrelu", y, skip, o))
        x, c = o, 2 * c
    o = new(1, 1, acts[x][2])
    ops.append(("gap", x, -1, o))
    x = o
    for width in G.FC_LAYER_CONFIGS[fc]:
        x = conv("dense", x, int(width))
    x = conv("dense", x, int(classes))
    return [tuple(a) for a in acts], ops, x


def act_sites(hparams, variant, classes: int, T: int, F: int) -> List[Tuple[int, int, int, int]]:
    """[(act, H, W, C)] of the activation-quantisation sites in site order, the rule restated: act i is a site iff it is not
    the input (0), not the logits, is materialised, and is the input of at least one conv / depthwise / dense / global-pool
    op.  The twin of ``cmoop_actquant_sites``."""
    acts, ops, logits = act_plan(hparams, variant, classes, T, F)
    out = []
    for i, (H, W, Cn, virt) in enumerate(acts):
        if i == 0 or i == logits or virt:
            continue
        if any(op[1] == i and op[0] in _MAC_KINDS for op in ops):
            out.append((i, H, W, Cn))
    return out


def c_act_sites(gene, variant: int, classes: int, T: int, F: int) -> List[Tuple[int, int, int, int]]:
    """``cmoop_actquant_sites``."""
    g, cap = (C.c_int32 * 6)(*(int(v) for v in gene)), 64
    rows, n = np.zeros((cap, 4), np.int32), C.c_int32()
    _lib.check(_lib.lib().cmoop_actquant_sites(g, C.c_int32(int(variant)), C.c_int32(int(classes)), C.c_int32(int(T)), C.c_int32(int(F)),
                                               _lib.ptr(rows), C.c_int32(cap), C.byref(n)))
    return [tuple(int(v) for v in r) for r in rows[:n.value]]


def fake_quant_act(x, bits: int, a=None, record=None, momentum: float = 0.99):
    """``cmoop_fake_quant_act``: the operator alone, in place on ``x`` (a CUDA float32 tensor, or a 4-byte-aligned view of one).
    ``a`` None: batch mode, and ``record`` (m_b, r, count) advances -> the new (m_b, r, count); else tracked mode under ``a``
    -> ``record`` unchanged."""
    import torch
    rec = ActRangeStruct()
    if record is not None:
        rec.m_b, rec.r, rec.count = float(record[0]), float(record[1]), int(record[2])
    a_in = C.c_float(float(a)) if a is not None else None
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_fake_quant_act(C.c_void_p(x.data_ptr()), C.c_int64(int(x.numel())), C.c_int32(int(bits)),
                                               C.byref(a_in) if a_in is not None else None, C.byref(rec), C.c_float(float(momentum))))
    return np.float32(rec.m_b), np.float32(rec.r), int(rec.count)


def fake_quant_act_time(x, bits: int, a=None, momentum: float = 0.99, iters: int = 100) -> float:
    """``cmoop_fake_quant_act_time``: average milliseconds of the call's launches (two in batch mode, one in tracked mode)."""
    import torch
    a_in, ms = (C.c_float(float(a)) if a is not None else None), C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_fake_quant_act_time(C.c_void_p(x.data_ptr()), C.c_int64(int(x.numel())), C.c_int32(int(bits)),
                                                    C.byref(a_in) if a_in is not None else None, C.c_float(float(momentum)),
                                                    C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)


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
