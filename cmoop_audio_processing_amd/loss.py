"""Soft-target training loss: mixup, label smoothing and class weights.

Opt-in and off by default (the reference trains on one hard label per row, unweighted, and has no counterpart:
everything here is BUILD-DEFINED).  ``LossConfig`` mirrors ``cmoop_loss`` (include/cmoop.h, where the semantics are
fixed).  With it on, a train step blends pairs of batch rows (mixup only), builds a dense target row and a weight per
batch row, and takes cross-entropy against them.  Validation is never changed: ``evaluate``, ``predict_proba``,
``predict_stream``, the per-epoch ``val_loss`` EarlyStopping monitors and the read-outs stay the sparse cross-entropy, so
``val_loss`` is comparable between configs.

``mixup_draws`` / ``mixup_reference`` / ``soft_targets_reference`` restate the kernels in numpy, bit for bit: the draws are
the counter RNG (integer arithmetic) keyed by (net seed, global train step, position of the row in its batch), the lam
table comes from the host call ``cmoop_mixup_table``, and all floating-point work is separately rounded fp32 products
and sums.  ``softmax_ce_soft_ref`` is the float64 statement of the loss and its gradient.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import functools
import math
from typing import Optional, Tuple

import numpy as np

from . import _lib
from .augment import _prefix, _range, _u32

STREAM_MIXUP = 0x5000        # gate / partner / lam draws (csrc/common.h)
TABLE = 1024                 # entries of the lam table
CLIP_LO = float(np.float32(1e-7))
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))

LossStruct = _lib.Loss       # cmoop_loss (include/cmoop.h)


@dataclasses.dataclass(frozen=True)
class LossConfig:
    """What a train step trains against; mirrors ``cmoop_loss``.

    ``label_smoothing`` eps: the target row becomes (1 - eps) * target + eps / classes.  ``mixup_alpha`` > 0: with
    probability ``mixup_p`` a row b is blended with another row q of its batch, lam * x[b] + (1 - lam) * x[q], lam drawn
    from the upper half of Beta(alpha, alpha) (so lam >= 0.5 and the row's own label dominates), and its target is the
    same blend of the two labels.  ``class_weight``: one weight per class (Keras' ``class_weight=``); a row's loss and
    gradient are scaled by its label's weight (a mixed row: by the blend of the two), and the sum is still divided by
    the batch size.

    Domain: 0 <= label_smoothing < 1; mixup_alpha finite in [0, 64]; 0 <= mixup_p <= 1; class_weight None or ``classes``
    finite values > 0.  The default does nothing; a config that does nothing is the same as None.
    """
    label_smoothing: float = 0.0
    mixup_alpha: float = 0.0
    mixup_p: float = 1.0
    class_weight: Optional[Tuple[float, ...]] = None

    def __post_init__(self):
        if self.class_weight is not None:
            object.__setattr__(self, "class_weight", tuple(float(v) for v in np.asarray(self.class_weight, np.float64).reshape(-1)))

    @classmethod
    def preset(cls, name: str = "kws", **over) -> "LossConfig":
        """Named recipes.

        "kws" -- mixup with alpha 0.2 on every row (p = 1) and label smoothing 0.1, no class weights.  BUILD-DEFINED: the
                 reference has no such loss; these are the values keyword-spotting recipes commonly pair with SpecAugment,
                 not something taken from it, and no accuracy gain has been measured here.
        """
        if name == "kws":
            return dataclasses.replace(cls(mixup_alpha=0.2, label_smoothing=0.1), **over)
        raise ValueError(f"unknown loss preset {name!r} (known: 'kws')")

    @classmethod
    def balanced(cls, y, classes: int, **kw) -> "LossConfig":
        """Class weights n / (classes * count_c) from the labels ``y`` (sklearn's "balanced"); raises on an empty class."""
        y = np.asarray(y.cpu() if hasattr(y, "cpu") else y).reshape(-1).astype(np.int64)
        if y.size == 0 or y.min() < 0 or y.max() >= classes:
            raise ValueError(f"balanced: labels must be non-empty and lie in [0, {classes})")
        count = np.bincount(y, minlength=classes)
        if (count == 0).any():
            raise ValueError(f"balanced: class {int(np.nonzero(count == 0)[0][0])} has no rows")
        return cls(class_weight=tuple(float(y.size) / (float(classes) * float(c)) for c in count), **kw)

    @property
    def mixup_on(self) -> bool:
        return self.mixup_alpha > 0 and self.mixup_p > 0

    @property
    def enabled(self) -> bool:
        """label_smoothing > 0, or (mixup_alpha > 0 and mixup_p > 0), or class weights."""
        return self.label_smoothing > 0 or self.mixup_on or self.class_weight is not None

    def _struct(self) -> LossStruct:
        st = LossStruct(float(self.label_smoothing), float(self.mixup_alpha), float(self.mixup_p), None, 0, 0)
        if self.class_weight is not None:
            cw = (C.c_double * len(self.class_weight))(*self.class_weight)
            st._keep = cw                                   # the struct points into it
            st.class_weight = C.cast(cw, C.c_void_p)
            st.n_class_weight = len(self.class_weight)
        return st

    def check(self, classes: int) -> "LossConfig":
        """Raise ValueError naming the offending field when the config is outside the domain for ``classes`` classes (host only)."""
        st = self._struct()
        L = _lib.lib()
        if L.cmoop_loss_check(C.byref(st), int(classes)) != 0:
            raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
        return self


def default_loss_config() -> LossConfig:
    """cmoop_loss_default as a LossConfig (equals LossConfig())."""
    st = LossStruct()
    _lib.check(_lib.lib().cmoop_loss_default(C.byref(st)))
    assert not st.class_weight
    return LossConfig(label_smoothing=st.label_smoothing, mixup_alpha=st.mixup_alpha, mixup_p=st.mixup_p)


def mixup_table(alpha: float) -> np.ndarray:
    """float32 [1024]: tab[k] = (float)Q(0.5 + (k + 0.5) / 2048), Q the quantile function of Beta(alpha, alpha) -- the
    host call ``cmoop_mixup_table`` (no GPU)."""
    return _table(float(alpha)).copy()


@functools.lru_cache(maxsize=32)
def _table(alpha: float) -> np.ndarray:
    out = np.empty(TABLE, np.float32)
    _lib.check(_lib.lib().cmoop_mixup_table(alpha, _lib.ptr(out)))
    out.setflags(write=False)
    return out


def mixup_draws(config: LossConfig, seed: int, step: int, B: int, raw: bool = False):
    """(gate int32 [B], partner int32 [B], lam float32 [B]) of a batch of B rows -- what ``cmoop_mixup_draws`` returns:
    the gate bit (0 with mixup off), and partner / lam AFTER the MIXED rule (a row that is not mixed has partner b and
    lam 1).  ``raw``: the partner and lam as drawn, before that rule (what the coverage check of the tests counts)."""
    b = np.arange(B, dtype=np.uint64)
    gate, q, lam = np.zeros(B, np.int32), b.astype(np.int32), np.ones(B, np.float32)
    if not config.mixup_on or B == 0:
        return gate, q, lam
    pre = _prefix(seed, STREAM_MIXUP, step)
    base = np.uint64(4) * b
    gate = ((_u32(pre, base) >> np.uint64(8)) < np.uint64(int(math.floor(config.mixup_p * 16777216.0)))).astype(np.int32)
    q_raw = _range(_u32(pre, base + np.uint64(1)), B).astype(np.int32)
    lam_raw = _table(float(config.mixup_alpha))[_range(_u32(pre, base + np.uint64(2)), TABLE).astype(np.int64)]
    if raw:
        return gate, q_raw, lam_raw
    mixed = (gate == 1) & (q_raw != q) & (lam_raw < np.float32(1.0))
    return gate, np.where(mixed, q_raw, q).astype(np.int32), np.where(mixed, lam_raw, np.float32(1.0)).astype(np.float32)


def mixup_reference(X_rows, config: LossConfig, seed: int, step: int) -> np.ndarray:
    """The blended batch, float32 [B, T, F], of the float32 rows ``X_rows`` [B, T, F] (row b = batch position b, already
    gathered -- and already augmented when augmentation is on): the numpy restatement of the kernel, bit for bit."""
    X = np.ascontiguousarray(X_rows, np.float32)
    if X.ndim != 3:
        raise ValueError("mixup_reference expects rows [B, T, F]")
    _, q, lam = mixup_draws(config, seed, step, X.shape[0])
    out = X.copy()                                   # an un-mixed row keeps its bits
    for b in np.nonzero(q != np.arange(X.shape[0]))[0]:
        mu = np.float32(1.0) - lam[b]
        out[b] = lam[b] * X[b] + mu * X[q[b]]        # two fp32 products, one fp32 add, separately rounded
    return out


def soft_targets_reference(y_rows, config: LossConfig, classes: int, seed: int, step: int):
    """(t float32 [B, classes], w float32 [B], primary int32 [B]) of the labels ``y_rows`` [B] (entry b = the label of batch
    position b): the numpy restatement of the targets kernel, bit for bit."""
    y = np.asarray(y_rows).reshape(-1).astype(np.int64)
    B, Cn = y.size, int(classes)
    _, q, lam = mixup_draws(config, seed, step, B)
    mu = np.float32(1.0) - lam
    a, c = y, y[q]
    j = np.arange(Cn)[None, :]
    zero = np.float32(0.0)
    m = np.where(j == a[:, None], lam[:, None], zero) + np.where(j == c[:, None], mu[:, None], zero)
    sc = m.astype(np.float32) * np.float32(1.0 - float(config.label_smoothing))
    t = sc + np.float32(float(config.label_smoothing) / float(Cn))
    if config.class_weight is not None:
        cw = np.asarray(config.class_weight, np.float64).astype(np.float32)
        w = lam * cw[a] + mu * cw[c]
    else:
        w = np.ones(B, np.float32)
    return t.astype(np.float32), w.astype(np.float32), a.astype(np.int32)


def softmax_ce_soft_ref(z, t, w=None):
    """Float64: (p [B, C], per-row UNWEIGHTED loss l [B], d(sum_b w_b l_b / B)/dz [B, C]) of cross-entropy against the dense
    targets t with pc = clip(p, 1e-7, 1 - 1e-7):  l_b = -sum_{t_j > 0} t_j (log pc_j - log sum_j pc_j)."""
    z, t = np.asarray(z, np.float64), np.asarray(t, np.float64)
    B = z.shape[0]
    w = np.ones(B) if w is None else np.asarray(w, np.float64)
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    pc = np.clip(p, CLIP_LO, CLIP_HI)
    S = pc.sum(axis=1, keepdims=True)
    loss = -np.where(t > 0, t * (np.log(pc) - np.log(S)), 0.0).sum(axis=1)
    gate = ((p >= CLIP_LO) & (p <= CLIP_HI)).astype(np.float64)
    q = gate * (t.sum(axis=1, keepdims=True) / S - t / pc)
    dz = w[:, None] * p * (q - (p * q).sum(axis=1, keepdims=True)) / B
    return p, loss, dz


# ---- the kernels alone (GPU) ----------------------------------------------------------------------------------------------
def mixup_batch(X, config: LossConfig, seed: int, step: int, idx=None, row0: int = 0, B: int = None):
    """The blend kernel alone (``cmoop_mixup_batch``): X CUDA float32 [N, T, F], idx CUDA int32 or None -> CUDA float32
    [B, T, F], batch position b = row idx[row0 + b] (idx None: row0 + b).  Any config of the domain, enabled or not."""
    import torch
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 3 and X.is_contiguous()):
        raise ValueError("mixup_batch expects a contiguous CUDA float32 tensor [N, T, F]")
    n = int(len(idx)) if idx is not None else int(X.shape[0])
    if B is None:
        B = n - int(row0)
    if not (row0 >= 0 and B >= 0 and row0 + B <= n):
        raise ValueError("mixup_batch: rows row0 .. row0 + B lie outside the data")
    T, F = int(X.shape[1]), int(X.shape[2])
    out = torch.empty((B, T, F), dtype=torch.float32, device=X.device)
    st = dataclasses.replace(config, class_weight=None)._struct()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_mixup_batch(C.byref(st), _lib.ptr(X), _lib.ptr(idx), int(row0), B, T, F, int(seed) & 0xFFFFFFFF,
                                            int(step) & 0xFFFFFFFF, _lib.ptr(out)))
    return out


def soft_targets(y, config: LossConfig, classes: int, seed: int, step: int, idx=None, row0: int = 0, B: int = None):
    """The targets kernel alone (``cmoop_soft_targets``): y CUDA int32 [N] -> CUDA (t float32 [B, classes], w float32 [B],
    primary int32 [B]) of the batch positions b = rows idx[row0 + b] (idx None: row0 + b)."""
    import torch
    if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.int32 and y.dim() == 1 and y.is_contiguous()):
        raise ValueError("soft_targets expects a contiguous CUDA int32 tensor [N]")
    n = int(len(idx)) if idx is not None else int(y.shape[0])
    if B is None:
        B = n - int(row0)
    if not (row0 >= 0 and B >= 0 and row0 + B <= n):
        raise ValueError("soft_targets: rows row0 .. row0 + B lie outside the data")
    st = config.check(classes)._struct()
    t = torch.empty((B, int(classes)), dtype=torch.float32, device=y.device)
    w = torch.empty((B,), dtype=torch.float32, device=y.device)
    primary = torch.empty((B,), dtype=torch.int32, device=y.device)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_soft_targets(C.byref(st), _lib.ptr(y), _lib.ptr(idx), int(row0), int(y.shape[0]), B, int(classes),
                                             int(seed) & 0xFFFFFFFF, int(step) & 0xFFFFFFFF, _lib.ptr(t), _lib.ptr(w), _lib.ptr(primary)))
    return t, w, primary
