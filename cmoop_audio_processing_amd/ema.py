"""Weight EMA: an exponential moving average of the weights, read by validation, early stopping and the read-outs.

Opt-in and off by default (the reference builds ``Adam()`` without it -- Keras' ``use_ema=True, ema_momentum=...``:
everything here is BUILD-DEFINED; ``include/cmoop.h`` fixes the semantics at ``cmoop_ema``).  ``i`` is
``optimizer.iterations`` before the update.

* ``m(i) = momentum``, or with ``warmup`` ``min(momentum, (1 + i) / (10 + i))``, evaluated in double on the host; the kernel
  takes ``mf = float32(m(i))`` and ``omf = float32(1.0 - m(i))``, each rounded once.
* after every optimiser step, per element of the average arena ``a``: trainable ``a = (mf * a) + (omf * w)`` -- two float32
  products and one float32 add, no fused multiply-add; BatchNorm moving statistics ``a = w``.
* the training trajectory is never touched; a fit with the average on validates, early-stops and reads out on ``a`` and
  leaves the parameters equal to the weights that were scored.

``ema_step_ref`` (numpy float32, one rounding per operation) is the statement the kernel is tested against.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib

EmaStruct = _lib.Ema               # cmoop_ema (include/cmoop.h)
KIND_FROZEN = 2


@dataclasses.dataclass(frozen=True)
class EmaConfig:
    """Mirrors ``cmoop_ema``; the default is off.  Domain: ``0 <= momentum < 1`` and finite (0 = off; Keras' default
    ``ema_momentum`` is 0.99), ``warmup`` a bool."""
    momentum: float = 0.0
    warmup: bool = False

    @property
    def enabled(self) -> bool:
        return self.momentum > 0

    def _struct(self) -> EmaStruct:
        st = EmaStruct()
        st.momentum, st.warmup, st.reserved = float(self.momentum), int(self.warmup), 0
        return st

    def check(self) -> "EmaConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        return check_struct(self._struct(), self)

    def momentum_at(self, i: int) -> float:
        """m(i), in double."""
        m, i = float(self.momentum), int(i)
        return min(m, (1.0 + i) / (10.0 + i)) if self.warmup else m


def check_struct(st: EmaStruct, ret=None):
    L = _lib.lib()
    if L.cmoop_ema_check(C.byref(st)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_ema_config() -> EmaConfig:
    """cmoop_ema_default as an EmaConfig (equals EmaConfig())."""
    st = EmaStruct()
    _lib.check(_lib.lib().cmoop_ema_default(C.byref(st)))
    return from_struct(st)


def from_struct(st: EmaStruct) -> EmaConfig:
    return EmaConfig(momentum=st.momentum, warmup=bool(st.warmup))


def rates(ema: EmaConfig, i: int):
    """``cmoop_ema_rates``: (m(i) double, float32 m(i), float32 1 - m(i)) as the kernel consumes them."""
    m, mf, omf = C.c_double(), C.c_float(), C.c_float()
    st = ema._struct()
    _lib.check(_lib.lib().cmoop_ema_rates(C.byref(st), int(i), C.byref(m), C.byref(mf), C.byref(omf)))
    return float(m.value), np.float32(mf.value), np.float32(omf.value)


def ema_step_ref(a, w, mf, omf, kinds=None):
    """ema_kernel restated in numpy float32, one IEEE single operation per line: the new average of ``a`` against the updated
    weights ``w``.  Elements of kind 2 (``optim.param_kinds``; ``kinds`` None: none) are copies of ``w``'s bits."""
    f = np.float32
    a, w = np.array(a, f), np.array(w, f)
    mf, omf = f(mf), f(omf)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        keep = mf * a
        take = omf * w
        out = keep + take
    if kinds is not None:
        frozen = np.asarray(kinds, np.uint8) == KIND_FROZEN
        out.view(np.uint32)[frozen] = w.view(np.uint32)[frozen]
    return out
