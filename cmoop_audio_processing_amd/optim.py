"""Optimiser options: a learning-rate schedule, decoupled weight decay (AdamW) and gradient clipping.

Opt-in and off by default (the reference builds ``Adam()`` with none of them: everything here is BUILD-DEFINED;
``include/cmoop.h`` fixes the semantics at ``cmoop_optim``).  ``i`` is ``optimizer.iterations`` before the update.

* schedule: ``lr(i) = config.lr * f(i)`` with Keras' ``CosineDecay`` (with linear warm-up), ``ExponentialDecay`` or
  ``PiecewiseConstantDecay`` as f, evaluated in double on the host; Adam's bias correction is applied on top as before.
* ``weight_decay``: ``w -= (w * wd) * lr(i)`` before the Adam update, on kernels only (``decay_mask=0``) or on every
  trainable tensor (``decay_mask=1``, Keras' default).
* ``global_clipnorm``: every gradient is multiplied by ``clip / norm`` when the norm over all trainable tensors exceeds the
  clip, and by exactly 1 otherwise.  ``clipvalue``: gradients are clamped to [-c, c].  Not both.

BatchNorm moving statistics are not trainable: never decayed, never in the norm.  ``global_norm_ref`` (float64) and
``adamw_step_ref`` (numpy float32, one rounding per operation in the kernel's order) are the statements the kernels are
tested against.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import Sequence, Tuple

import numpy as np

from . import _lib

OptimStruct = _lib.Optim           # cmoop_optim (include/cmoop.h)

SCHEDULES = {"constant": 0, "cosine": 1, "exponential": 2, "piecewise": 3}
KIND_KERNEL, KIND_TRAINABLE, KIND_FROZEN = 0, 1, 2
#: genes.param_tensors role -> tensor kind
ROLE_KINDS = {"kernel": KIND_KERNEL, "bias": KIND_TRAINABLE, "gamma": KIND_TRAINABLE, "beta": KIND_TRAINABLE,
              "moving_mean": KIND_FROZEN, "moving_var": KIND_FROZEN}


@dataclasses.dataclass(frozen=True)
class OptimConfig:
    """Mirrors ``cmoop_optim``; the default is everything off (constant-rate Adam, as the reference trains).

    ``schedule``: "constant", "cosine", "exponential" or "piecewise" (or its code 0 .. 3); the fields a schedule does not
    read are ignored.  Domain: nothing negative or non-finite, ``decay_steps >= 1`` where the schedule reads it, at most 8
    strictly increasing ``boundaries`` with one more ``values``, ``global_clipnorm`` and ``clipvalue`` not both.
    """
    schedule: object = 0
    warmup_steps: int = 0
    warmup_start: float = 0.0
    decay_steps: int = 0
    alpha: float = 0.0
    decay_rate: float = 0.0
    staircase: bool = False
    boundaries: Tuple[int, ...] = ()
    values: Tuple[float, ...] = ()
    weight_decay: float = 0.0
    decay_mask: int = 0
    global_clipnorm: float = 0.0
    clipvalue: float = 0.0

    # -- constructors ------------------------------------------------------------------------------------------------------
    @classmethod
    def preset(cls, name: str = "kws", epochs: int = 30, steps_per_epoch: int = 100, **over) -> "OptimConfig":
        """Named recipes.

        "kws" -- cosine decay to zero over the whole fit after one tenth of it (at least one epoch) of linear warm-up from
                 0.1, weight decay 1e-2 on kernels, global-norm clip 1.  BUILD-DEFINED: the reference has no such options;
                 these are values small keyword-spotting models are commonly trained with, not something taken from it,
                 and no accuracy gain has been measured here.
        """
        if name == "kws":
            base = cls.cosine(epochs, max(1, epochs // 10), steps_per_epoch, warmup_start=0.1, weight_decay=1e-2, global_clipnorm=1.0)
            return dataclasses.replace(base, **over)
        raise ValueError(f"unknown optim preset {name!r} (known: 'kws')")

    @classmethod
    def cosine(cls, epochs: int, warmup_epochs: int, steps_per_epoch: int, warmup_start: float = 0.0, alpha: float = 0.0,
               **over) -> "OptimConfig":
        """``warmup_epochs`` of linear warm-up from ``warmup_start``, then cosine decay to ``alpha`` at the end of ``epochs``."""
        w = int(warmup_epochs) * int(steps_per_epoch)
        return cls(schedule=1, warmup_steps=w, warmup_start=float(warmup_start), decay_steps=int(epochs) * int(steps_per_epoch) - w,
                   alpha=float(alpha), **over)

    @classmethod
    def exponential(cls, decay_epochs: int, decay_rate: float, steps_per_epoch: int, staircase: bool = False, **over) -> "OptimConfig":
        """The rate is multiplied by ``decay_rate`` every ``decay_epochs`` (continuously, or in steps with ``staircase``)."""
        return cls(schedule=2, decay_steps=int(decay_epochs) * int(steps_per_epoch), decay_rate=float(decay_rate),
                   staircase=bool(staircase), **over)

    @classmethod
    def piecewise(cls, boundary_epochs: Sequence[int], values: Sequence[float], steps_per_epoch: int, **over) -> "OptimConfig":
        """``values[k]`` times the base rate from the end of epoch ``boundary_epochs[k-1]`` on (``values[0]`` first)."""
        return cls(schedule=3, boundaries=tuple(int(e) * int(steps_per_epoch) for e in boundary_epochs),
                   values=tuple(float(v) for v in values), **over)

    # -- properties --------------------------------------------------------------------------------------------------------
    @property
    def schedule_code(self) -> int:
        if isinstance(self.schedule, str):
            if self.schedule not in SCHEDULES:
                raise ValueError(f"optim: unknown schedule {self.schedule!r} (known: {sorted(SCHEDULES)})")
            return SCHEDULES[self.schedule]
        return int(self.schedule)

    @property
    def finish_path(self) -> bool:
        """Decay or a clip is set: the step takes the finish + update launches in place of the fused one."""
        return self.weight_decay > 0 or self.global_clipnorm > 0 or self.clipvalue > 0

    @property
    def enabled(self) -> bool:
        return self.schedule_code != 0 or self.finish_path

    def _struct(self) -> OptimStruct:
        if len(self.boundaries) > 8:
            raise ValueError("optim: at most 8 boundaries")
        piecewise = self.schedule_code == 3
        if piecewise and len(self.values) != len(self.boundaries) + 1:
            raise ValueError("optim: values must hold one entry more than boundaries")
        st = OptimStruct()
        st.weight_decay, st.global_clipnorm, st.clipvalue = float(self.weight_decay), float(self.global_clipnorm), float(self.clipvalue)
        st.warmup_start, st.alpha, st.decay_rate = float(self.warmup_start), float(self.alpha), float(self.decay_rate)
        st.warmup_steps, st.decay_steps = int(self.warmup_steps), int(self.decay_steps)
        st.schedule, st.staircase, st.decay_mask = self.schedule_code, int(bool(self.staircase)), int(self.decay_mask)
        if piecewise:
            st.n_boundaries = len(self.boundaries)
            for k, b in enumerate(self.boundaries):
                st.boundaries[k] = int(b)
            for k, v in enumerate(self.values):
                st.values[k] = float(v)
        return st

    def check(self) -> "OptimConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        return check_struct(self._struct(), self)

    # -- the schedule ------------------------------------------------------------------------------------------------------
    def factor_at(self, i: int) -> float:
        """f(i), in double."""
        s, i = self.schedule_code, int(i)
        if s == 1:
            if i < self.warmup_steps:
                return self.warmup_start + (1.0 - self.warmup_start) * i / self.warmup_steps
            t = min(i - self.warmup_steps, self.decay_steps)
            return (1.0 - self.alpha) * 0.5 * (1.0 + math.cos(math.pi * t / self.decay_steps)) + self.alpha
        if s == 2:
            p = i / self.decay_steps
            return self.decay_rate ** (math.floor(p) if self.staircase else p)
        if s == 3:
            k = 0
            while k < len(self.boundaries) and i > self.boundaries[k]:
                k += 1
            return self.values[k]
        return 1.0

    def lr_at(self, i: int, base_lr: float = 1e-3) -> float:
        """lr(i) = base_lr * f(i) in double: the un-corrected rate of iteration i (the one weight decay uses)."""
        return base_lr if self.schedule_code == 0 else base_lr * self.factor_at(i)

    def alpha_at(self, i: int, base_lr: float = 1e-3, beta1: float = 0.9, beta2: float = 0.999) -> float:
        """Adam's bias-corrected step size of iteration i, in double (the kernels take it rounded to float32 once)."""
        t = int(i) + 1
        return self.lr_at(i, base_lr) * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def check_struct(st: OptimStruct, ret=None):
    L = _lib.lib()
    if L.cmoop_optim_check(C.byref(st)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_optim_config() -> OptimConfig:
    """cmoop_optim_default as an OptimConfig (equals OptimConfig())."""
    st = OptimStruct()
    _lib.check(_lib.lib().cmoop_optim_default(C.byref(st)))
    return from_struct(st)


def from_struct(st: OptimStruct) -> OptimConfig:
    n = int(st.n_boundaries)
    piecewise = int(st.schedule) == 3
    return OptimConfig(schedule=int(st.schedule), warmup_steps=int(st.warmup_steps), warmup_start=st.warmup_start,
                       decay_steps=int(st.decay_steps), alpha=st.alpha, decay_rate=st.decay_rate, staircase=bool(st.staircase),
                       boundaries=tuple(int(b) for b in st.boundaries[:n]), values=tuple(st.values[:n + 1]) if piecewise else (),
                       weight_decay=st.weight_decay, decay_mask=int(st.decay_mask), global_clipnorm=st.global_clipnorm,
                       clipvalue=st.clipvalue)


def rates(optim, config_struct, i: int):
    """``cmoop_optim_rates``: (lr(i) double, float32 lr(i), float32 step size) as the kernels consume them; ``optim`` an
    OptimConfig or None, ``config_struct`` a ``cmoop_config`` (``EvalConfig.to_struct()``)."""
    lr, lr32, a32 = C.c_double(), C.c_float(), C.c_float()
    st = optim._struct() if optim is not None else None
    _lib.check(_lib.lib().cmoop_optim_rates(C.byref(st) if st is not None else None, C.byref(config_struct), int(i), C.byref(lr),
                                            C.byref(lr32), C.byref(a32)))
    return float(lr.value), np.float32(lr32.value), np.float32(a32.value)


def param_kinds(gene, variant: int, classes: int) -> np.ndarray:
    """uint8 kind of every parameter in arena order, from ``genes.param_tensors``: 0 kernel, 1 other trainable, 2 frozen."""
    from . import genes as G
    out = []
    for _, shape, role in G.param_tensors(gene, variant, classes):
        out.append(np.full(int(np.prod(shape)), ROLE_KINDS[role], np.uint8))
    return np.concatenate(out)


def param_kinds_lib(gene, variant: int, classes: int) -> np.ndarray:
    """The same from the trainer's own host walk (``cmoop_param_kinds``)."""
    from . import genes as G
    n = G.param_count(gene, variant, classes)
    out = np.empty(n, np.uint8)
    g = (C.c_int32 * 6)(*[int(v) for v in gene])
    _lib.check(_lib.lib().cmoop_param_kinds(g, int(variant), int(classes), _lib.ptr(out), n))
    return out


# ---- the statements ---------------------------------------------------------------------------------------------------------
def global_norm_ref(g, kinds=None):
    """Float64 (sum of squares, norm) of the gradients of every trainable element (kind != 2; ``kinds`` None: all)."""
    g = np.asarray(g, np.float64).ravel()
    if kinds is not None:
        g = g[np.asarray(kinds).ravel() != KIND_FROZEN]
    ss = float(np.sum(g * g))
    return ss, math.sqrt(ss)


def clip_scale_ref(norm: float, clip: float) -> float:
    """Float64 scale of the global-norm clip: clip / norm where norm > clip > 0, else 1."""
    return clip / norm if clip > 0 and norm > clip else 1.0


def adamw_step_ref(w, g, m, v, alpha, lr, beta1, beta2, eps, scale=1.0, weight_decay=0.0, decay_mask=0, clipvalue=0.0, kinds=None):
    """adamw_kernel restated in numpy float32, one IEEE single operation per line, in the kernel's order: g * scale, the
    value clamp, the masked decay with the float32 ``lr``, then the Adam update with the float32 step size ``alpha``.
    ``scale`` is the clip scale the device reported.  Elements of kind 2 keep w, m, v.  Returns the new (w, m, v)."""
    f = np.float32
    w, g, m, v = (np.array(a, f) for a in (w, g, m, v))
    kinds = np.zeros(w.shape, np.uint8) if kinds is None else np.asarray(kinds, np.uint8)
    w0, m0, v0 = w.copy(), m.copy(), v.copy()
    alpha, lr, c1, c2, eps = f(alpha), f(lr), f(1.0 - beta1), f(1.0 - beta2), f(eps)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        g = g * f(scale)
        if clipvalue > 0:
            c = f(clipvalue)
            g = np.where(g < -c, -c, np.where(g > c, c, g)).astype(f)
        if weight_decay > 0:
            d = w * f(weight_decay)
            dec = w - d * lr
            w = np.where((kinds == KIND_KERNEL) | bool(decay_mask), dec, w).astype(f)
        dm = (g - m) * c1
        m = m + dm
        gg = g * g
        dv = (gg - v) * c2
        v = v + dv
        num = m * alpha
        den = np.sqrt(v) + eps
        w = w - num / den
    frozen = kinds == KIND_FROZEN
    return (np.where(frozen, w0, w).astype(f), np.where(frozen, m0, m).astype(f), np.where(frozen, v0, v).astype(f))
