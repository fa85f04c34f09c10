"""Knowledge distillation: train a candidate against the tempered logits of a larger, already trained model.

Opt-in and off by default (the reference has no counterpart: everything here is BUILD-DEFINED; ``include/cmoop.h`` fixes
the semantics at ``cmoop_distill``).  OFFLINE: the teacher's logits of the resident training rows are computed once into one
device table shared by every candidate (``PopulationEvaluator.set_teacher``), so the teacher sees the un-augmented,
un-mixed row.  With it on a train step builds the dense targets ``t`` / row weights ``w`` of the soft-target loss (one-hot
and 1 under a default ``LossConfig``), the teacher rows ``q = softmax(zt[row] / T)`` -- blended with the mixup draws of the
step when a row is mixed -- and minimises

    w_b [ (1 - alpha) CE(t_b, softmax(z_b)) + alpha T^2 KL(q_b || softmax(z_b / T)) ]

Validation is never changed: ``evaluate``, ``predict_*``, the monitored ``val_loss`` and the read-outs stay the sparse
cross-entropy.  ``softmax_ce_distill_ref`` and ``teacher_targets_ref`` are the float64 statements the kernels are tested
against.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib
from .loss import LossConfig, mixup_draws, softmax_ce_soft_ref

DistillStruct = _lib.Distill       # cmoop_distill (include/cmoop.h)


@dataclasses.dataclass(frozen=True)
class DistillConfig:
    """How strongly, and how tempered, a candidate is trained against the teacher; mirrors ``cmoop_distill`` without its table.

    ``alpha``: weight of the distillation term, the hard-label term keeps 1 - alpha; 0 is off.  ``temperature`` T: both the
    teacher's and the student's logits are divided by T for that term, which is scaled by T^2 so its gradient keeps its
    size.  Domain: 0 <= alpha <= 1, T finite in [1, 64].  A config is enabled when alpha > 0; it only takes effect once a
    teacher table is set.
    """
    alpha: float = 0.0
    temperature: float = 1.0

    @classmethod
    def preset(cls, name: str = "kws", **over) -> "DistillConfig":
        """Named recipes.

        "kws" -- alpha 0.7, temperature 4.  BUILD-DEFINED: the reference has no distillation; these are values small
                 keyword-spotting models are commonly distilled with, not something taken from it, and no accuracy gain
                 has been measured here.
        """
        if name == "kws":
            return dataclasses.replace(cls(alpha=0.7, temperature=4.0), **over)
        raise ValueError(f"unknown distill preset {name!r} (known: 'kws')")

    @property
    def enabled(self) -> bool:
        """alpha > 0 (and, where it is applied, a teacher table)."""
        return self.alpha > 0

    def _struct(self, teacher_logits=None) -> DistillStruct:
        st = DistillStruct(float(self.alpha), float(self.temperature), None, 0)
        if teacher_logits is not None:
            st._keep = teacher_logits                      # the struct points into it
            st.teacher_logits_dev = teacher_logits.data_ptr()
            st.n_rows = int(teacher_logits.shape[0])
        return st

    def check(self, classes: int, teacher_logits=None, n_train: int = 0) -> "DistillConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only); with a table,
        its rows must equal ``n_train``."""
        return check_struct(self._struct(teacher_logits), classes, n_train, self)


def check_struct(st: DistillStruct, classes: int, n_train: int, ret=None):
    L = _lib.lib()
    if L.cmoop_distill_check(C.byref(st), int(classes), int(n_train)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_distill_config() -> DistillConfig:
    """cmoop_distill_default as a DistillConfig (equals DistillConfig())."""
    st = DistillStruct()
    _lib.check(_lib.lib().cmoop_distill_default(C.byref(st)))
    assert not st.teacher_logits_dev and st.n_rows == 0
    return DistillConfig(alpha=st.alpha, temperature=st.temperature)


def check_teacher_table(teacher_logits, n_train: int, classes: int):
    """The teacher table as the trainer reads it: a contiguous CUDA float32 tensor [n_train, classes]; raises otherwise."""
    import torch
    t = teacher_logits
    if not (isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.is_contiguous()):
        raise ValueError("teacher logits must be a contiguous CUDA float32 tensor [n_train, classes]")
    if tuple(t.shape) != (int(n_train), int(classes)):
        raise ValueError(f"teacher logits are {tuple(t.shape)}, the training split needs [{int(n_train)}, {int(classes)}]")
    return t


def require_teacher(distill, teacher_logits) -> None:
    """An enabled ``distill`` needs a teacher table: raise before anything is launched when there is none."""
    if distill is not None and distill.enabled and teacher_logits is None:
        raise ValueError("EvalConfig.distill is enabled but no teacher is set: call PopulationEvaluator.set_teacher(...) "
                         "(or NetSession.set_distill(teacher_logits=table); set_distill(None) to train without it) first")


# ---- float64 statements -----------------------------------------------------------------------------------------------------
def _softmax64(z):
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / e.sum(axis=1, keepdims=True)


def teacher_targets_ref(zt_rows, temperature: float, loss: LossConfig = None, seed: int = 0, step: int = 0) -> np.ndarray:
    """Float64 q [B, C] of the teacher logits ``zt_rows`` [B, C] (row b = the table row of batch position b):
    softmax(zt / T), and for a row the mixup draws of (``loss``, seed, step) mix, lam u[b] + (1 - lam) u[partner]."""
    u = _softmax64(np.asarray(zt_rows, np.float64) / float(temperature))
    if loss is None or not loss.mixup_on:
        return u
    _, q, lam = mixup_draws(loss, seed, step, u.shape[0])
    lam = lam.astype(np.float64)[:, None]
    return np.where((q != np.arange(u.shape[0]))[:, None], lam * u + (1.0 - lam) * u[q], u)


def softmax_ce_distill_ref(z, t, w, q, alpha: float, temperature: float):
    """Float64: (per-row weighted loss l [B], d(sum_b l_b / B)/dz [B, C]) of
    l_b = w_b [(1 - alpha) CE_b + alpha T^2 KD_b], CE_b the clipped cross-entropy of ``loss.softmax_ce_soft_ref`` against t
    and KD_b = sum_{q_j > 0} q_j (log q_j - log softmax(z / T)_j)."""
    z, q = np.asarray(z, np.float64), np.asarray(q, np.float64)
    B = z.shape[0]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    a, T = float(alpha), float(temperature)
    _, ce, dce = softmax_ce_soft_ref(z, t, w)                    # dce carries w and 1 / B
    zs = (z - z.max(axis=1, keepdims=True)) / T
    ls = zs - np.log(np.exp(zs).sum(axis=1, keepdims=True))
    pos = q > 0
    kd = np.where(pos, q * (np.log(np.where(pos, q, 1.0)) - ls), 0.0).sum(axis=1)
    loss = w * ((1.0 - a) * ce + a * T * T * kd)
    dz = (1.0 - a) * dce + w[:, None] * (a * T * (q.sum(axis=1, keepdims=True) * np.exp(ls) - q)) / B
    return loss, dz


# ---- the kernels alone (GPU) ----------------------------------------------------------------------------------------------
def teacher_targets(zt, temperature: float, loss: LossConfig = None, seed: int = 0, step: int = 0, idx=None, row0: int = 0,
                    B: int = None):
    """The teacher-targets kernel alone (``cmoop_teacher_targets``): zt CUDA float32 [N, C], idx CUDA int32 or None -> CUDA
    float32 q [B, C] of the batch positions b = rows idx[row0 + b] (idx None: row0 + b), clamped into [0, N)."""
    import torch
    if not (isinstance(zt, torch.Tensor) and zt.is_cuda and zt.dtype == torch.float32 and zt.dim() == 2 and zt.is_contiguous()):
        raise ValueError("teacher_targets expects a contiguous CUDA float32 tensor [N, C]")
    n = int(len(idx)) if idx is not None else int(zt.shape[0])
    if B is None:
        B = n - int(row0)
    if not (row0 >= 0 and B >= 0 and row0 + B <= n):
        raise ValueError("teacher_targets: rows row0 .. row0 + B lie outside the data")
    Cn = int(zt.shape[1])
    st = dataclasses.replace(loss, class_weight=None)._struct() if loss is not None else None
    q = torch.empty((B, Cn), dtype=torch.float32, device=zt.device)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_teacher_targets(C.byref(st) if st is not None else None, _lib.ptr(zt), _lib.ptr(idx), int(row0),
                                                int(zt.shape[0]), B, Cn, float(temperature), int(seed) & 0xFFFFFFFF,
                                                int(step) & 0xFFFFFFFF, _lib.ptr(q)))
    return q


def softmax_ce_distill(z, t, w, primary, q, alpha: float, temperature: float, acc, dz=None, preds=None) -> None:
    """The loss kernel alone (``cmoop_softmax_ce_distill``) on CUDA tensors: z, t, q float32 [B, C]; w float32 [B] or None;
    primary int32 [B] or None; acc int64 [2] (the loss sum's double bits, the correct count), added to; dz float32 [B, C]
    and preds int32 [B] written when given."""
    import torch
    B, Cn = int(z.shape[0]), int(z.shape[1])
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_softmax_ce_distill(_lib.ptr(z), _lib.ptr(t), _lib.ptr(w), _lib.ptr(primary), _lib.ptr(q), float(alpha),
                                                   float(temperature), B, Cn, _lib.ptr(dz), _lib.ptr(acc), _lib.ptr(preds)))
    torch.cuda.synchronize()
