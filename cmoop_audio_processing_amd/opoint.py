"""Operating-point read-out: the false-positive rate at a target recall, the AUC and one threshold per class.

Opt-in and off by default (the reference scores arg-max predictions only -- ``calculate_fpr``, which stays the third
objective: everything here is BUILD-DEFINED; ``include/cmoop.h`` fixes the semantics at ``cmoop_opoint``).  A deployed
keyword spotter fires when a class posterior reaches a threshold, so the question is: at the threshold that still catches
``recall`` of a class's positives, how many negatives fire too?

* order: ``key(s) = b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)`` of the float32 bits ``b`` -- a total order on bit patterns
  (``-0 < +0``, NaNs at both ends), nothing special-cased;
* one-vs-rest: row j is positive for class c iff ``y[j] == c``; a label outside ``[0, C)`` is negative everywhere;
* ``cnt[c][i] = (ge_pos, ge_neg, gt_pos, gt_neg)``: rows whose key is >= (>) row i's, split by positive / negative;
* per class with ``P >= 1``: ``U2 = sum over positives of 2 (N - ge_neg) + (ge_neg - gt_neg)`` (twice the Mann-Whitney U),
  ``k = min(P, max(1, ceil(recall * P)))``, and among positives with ``ge_pos >= k`` the one with the largest key gives
  ``thr`` (its score), ``TP`` (its ge_pos) and ``FP`` (its ge_neg);
* summary, float64, left to right in class order: ``fpr_at_recall``, ``recall_achieved``, ``auc``, ``classes_scored``.

Everything is an integer or a float64 quotient of integers, so the device, ``cmoop_opoint_summary`` and the numpy
restatements below (``roc_counts_reference`` by sort + ``searchsorted``, ``operating_point_reference``) agree exactly.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np

from . import _lib

OpointStruct = _lib.Opoint          # cmoop_opoint (include/cmoop.h)
OpointClassStruct = _lib.OpointClass
MAX_ROWS = 262144                   # n^2 compares, as the device epoch permutation
MAX_CLASSES = 64
SUMMARY_KEYS = ("fpr_at_recall", "recall_achieved", "auc", "classes_scored")
CLASS_KEYS = ("thresholds", "tp", "fp", "positives", "negatives", "k", "u2")


@dataclasses.dataclass(frozen=True)
class OperatingPointConfig:
    """Mirrors ``cmoop_opoint``; the default is off.  Domain: ``0 <= recall <= 1`` and finite (0 = off), ``objective`` a bool:
    with it the evaluator ranks candidates by ``fpr_at_recall`` in the place of the arg-max FPR."""
    recall: float = 0.0
    objective: bool = False

    @property
    def enabled(self) -> bool:
        return self.recall > 0

    def _struct(self) -> OpointStruct:
        st = OpointStruct()
        st.recall, st.objective, st.reserved = float(self.recall), int(self.objective), 0
        return st

    def check(self) -> "OperatingPointConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        return check_struct(self._struct(), self)


def check_struct(st: OpointStruct, ret=None):
    L = _lib.lib()
    if L.cmoop_opoint_check(C.byref(st)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_opoint_config() -> OperatingPointConfig:
    """cmoop_opoint_default as an OperatingPointConfig (equals OperatingPointConfig())."""
    st = OpointStruct()
    _lib.check(_lib.lib().cmoop_opoint_default(C.byref(st)))
    return OperatingPointConfig(recall=st.recall, objective=bool(st.objective))


def score_keys(p) -> np.ndarray:
    """uint32 order keys of float32 scores (any shape): ``b ^ (0xFFFFFFFF if b >> 31 else 0x80000000)``."""
    b = np.ascontiguousarray(p, np.float32).view(np.uint32)
    return b ^ np.where(b >> np.uint32(31), np.uint32(0xFFFFFFFF), np.uint32(0x80000000)).astype(np.uint32)


def _check_shape(p, y):
    p = np.ascontiguousarray(p, np.float32)
    y = np.ascontiguousarray(y, np.int32).reshape(-1)
    if p.ndim != 2 or len(p) != len(y):
        raise ValueError("expects scores [n, C] and labels [n]")
    if not 1 <= p.shape[1] <= MAX_CLASSES:
        raise ValueError(f"classes must be in [1, {MAX_CLASSES}]")
    if len(p) > MAX_ROWS:
        raise ValueError(f"{len(p)} rows, the read-out ranks at most {MAX_ROWS}")
    return p, y


def roc_counts_reference(p, y) -> np.ndarray:
    """int32 [C, n, 4] = (ge_pos, ge_neg, gt_pos, gt_neg) per class and row, by one sort per group and ``searchsorted``
    (O(n log n) time, O(n) memory per class): the statement ``cmoop_roc_counts`` is tested against."""
    p, y = _check_shape(p, y)
    n, Cn = p.shape
    keys = score_keys(p)
    out = np.zeros((Cn, n, 4), np.int32)
    for c in range(Cn):
        k = keys[:, c]
        pos = np.sort(k[y == c])
        neg = np.sort(k[y != c])
        out[c, :, 0] = len(pos) - np.searchsorted(pos, k, side="left")
        out[c, :, 1] = len(neg) - np.searchsorted(neg, k, side="left")
        out[c, :, 2] = len(pos) - np.searchsorted(pos, k, side="right")
        out[c, :, 3] = len(neg) - np.searchsorted(neg, k, side="right")
    return out


def summary_reference(P, N, tp, fp, u2) -> np.ndarray:
    """float64 [4] = (fpr_at_recall, recall_achieved, auc, classes_scored) from the per-class integers, in the operation
    order of ``cmoop_opoint_summary``: one Python float (IEEE double) operation at a time, left to right in class order."""
    fpr = rec = auc = 0.0
    scored = ranked = 0
    for c in range(len(P)):
        if int(P[c]) < 1:
            continue
        scored += 1
        fpr += float(int(fp[c])) / float(int(N[c])) if int(N[c]) > 0 else 0.0
        rec += float(int(tp[c])) / float(int(P[c]))
        if int(N[c]) >= 1:
            auc += float(int(u2[c])) / (2.0 * float(int(P[c])) * float(int(N[c])))
            ranked += 1
    return np.array([fpr / float(scored) if scored else 0.0, rec / float(scored) if scored else 0.0,
                     auc / float(ranked) if ranked else float("nan"), float(scored)], np.float64)


def pack(thr, tp, fp, P, N, k, u2, summary) -> dict:
    """The dict ``NetSession.operating_point`` and ``operating_point_reference`` return."""
    d = {"thresholds": np.asarray(thr, np.float32), "tp": np.asarray(tp, np.int32), "fp": np.asarray(fp, np.int32),
         "positives": np.asarray(P, np.int32), "negatives": np.asarray(N, np.int32), "k": np.asarray(k, np.int32),
         "u2": np.asarray(u2, np.int64)}
    s = np.asarray(summary, np.float64)
    d.update(fpr_at_recall=float(s[0]), recall_achieved=float(s[1]), auc=float(s[2]), classes_scored=int(s[3]),
             summary=s.copy())
    return d


def from_records(rec, summary) -> dict:
    """``pack`` of a ctypes array of ``cmoop_opoint_class`` and a summary [4]."""
    a = np.frombuffer(rec, dtype=np.dtype([("u2", "<i8"), ("P", "<i4"), ("N", "<i4"), ("k", "<i4"), ("tp", "<i4"), ("fp", "<i4"),
                                           ("thr", "<f4")])).copy()
    return pack(a["thr"], a["tp"], a["fp"], a["P"], a["N"], a["k"], a["u2"], np.array(list(summary), np.float64))


def operating_point_reference(p, y, recall: float) -> dict:
    """The whole read-out in numpy: per-class ``thresholds`` (float32, bit patterns of ``p``), ``tp``, ``fp``, ``positives``,
    ``negatives``, ``k`` (int32), ``u2`` (int64) and the summary keys -- what ``cmoop_operating_point`` returns, exactly."""
    p, y = _check_shape(p, y)
    n, Cn = p.shape
    cnt = roc_counts_reference(p, y).astype(np.int64)
    thr = np.full(Cn, np.inf, np.float32)
    tp, fp, P, N, k = (np.zeros(Cn, np.int32) for _ in range(5))
    u2 = np.zeros(Cn, np.int64)
    keys = score_keys(p)
    for c in range(Cn):
        pos = np.nonzero(y == c)[0]
        P[c], N[c] = len(pos), n - len(pos)
        if not len(pos):
            continue
        ge_pos, ge_neg, gt_neg = cnt[c, pos, 0], cnt[c, pos, 1], cnt[c, pos, 3]
        u2[c] = int(np.sum(2 * (int(N[c]) - ge_neg) + (ge_neg - gt_neg)))
        k[c] = min(int(P[c]), max(1, int(math.ceil(float(recall) * float(int(P[c]))))))
        ok = np.nonzero(ge_pos >= int(k[c]))[0]
        best = ok[np.argmax(keys[pos[ok], c])]
        thr[c] = p[pos[best], c]
        tp[c], fp[c] = ge_pos[best], ge_neg[best]
    return pack(thr, tp, fp, P, N, k, u2, summary_reference(P, N, tp, fp, u2))


def summary_from_library(P, N, tp, fp, u2, k=None, thr=None) -> np.ndarray:
    """``cmoop_opoint_summary`` (host only) on per-class arrays -> float64 [4]."""
    Cn = len(P)
    rec = (OpointClassStruct * Cn)()
    for c in range(Cn):
        rec[c].u2, rec[c].P, rec[c].N, rec[c].tp, rec[c].fp = int(u2[c]), int(P[c]), int(N[c]), int(tp[c]), int(fp[c])
        rec[c].k = int(k[c]) if k is not None else 0
        rec[c].thr = float(thr[c]) if thr is not None else 0.0
    out = (C.c_double * 4)()
    _lib.check(_lib.lib().cmoop_opoint_summary(rec, C.c_int32(Cn), out))
    return np.array(list(out), np.float64)


def roc_counts(probs, y):
    """``cmoop_roc_counts``: probs CUDA float32 [n, C] and y CUDA int32 [n], both contiguous -> CUDA int32 [C, n, 4]."""
    import torch
    n, Cn = int(probs.shape[0]), int(probs.shape[1])
    out = torch.empty((Cn, n, 4), dtype=torch.int32, device=probs.device)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_roc_counts(_lib.ptr(probs), _lib.ptr(y), C.c_int64(n), C.c_int32(Cn), _lib.ptr(out)))
    return out


def operating_point(probs, y, recall: float) -> dict:
    """``cmoop_operating_point``: probs CUDA float32 [n, C] and y CUDA int32 [n], both contiguous -> the dict of
    ``operating_point_reference``."""
    import torch
    n, Cn = int(probs.shape[0]), int(probs.shape[1])
    st = OperatingPointConfig(recall=recall).check()._struct()
    rec, summary = (OpointClassStruct * Cn)(), (C.c_double * 4)()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_operating_point(_lib.ptr(probs), _lib.ptr(y), C.c_int64(n), C.c_int32(Cn), C.byref(st), rec, summary))
    return from_records(rec, summary)
