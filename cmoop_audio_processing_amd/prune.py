"""Magnitude pruning in training: sparse kernels inside the train step, their size and their export.

Opt-in and off by default (the reference trains and sizes a dense model: everything here is BUILD-DEFINED; ``include/cmoop.h``
fixes the semantics at ``cmoop_prune``).  Per pruned tensor (every convolution kernel after the first and every dense kernel;
the first convolution and the depthwise kernels are copied unless ``skip_small`` is False) at sparsity ``s``:

* ``key_i = bits(w_i) & 0x7FFFFFFF`` as uint32 (a NaN outranks inf, -0.0 has key 0);
* ``k = floor(s * len)`` in IEEE double; ``k == 0`` copies the tensor;
* else ``t`` = the k-th smallest key and ``w_eff_i = +0.0 if key_i <= t else w_i``: at least ``k`` zeros, exactly ``k`` unless
  keys tie at ``t``; no floating-point compare, no dependence on order.

Train steps prune the latent weights at ``sparsity_at(cfg, it)`` (TF-MOT's PolynomialDecay, power 3, from 0), ``it`` the Adam
iteration the step is about to take; the gradients go unchanged to the dense latent weights (straight-through), so a pruned
weight can regrow.  Inference -- every validation pass of a fit included -- always prunes at the final ``sparsity``: a fit
validates, early-stops and snapshots the model it would ship if it stopped now, and ``val_loss`` before ``end_step`` is
therefore that of a net that has not yet adapted to its final sparsity.  With ``QuantConfig`` on as well the order is prune,
then quantise.  ``prune_ref`` (numpy, integers only) is the statement the kernels are tested against; no accuracy figure is
measured or claimed.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
from typing import List, Tuple

import numpy as np

from . import _lib, genes as G

PruneStruct = _lib.Prune            # cmoop_prune (include/cmoop.h)
ABS_MASK = np.uint32(0x7FFFFFFF)


@dataclasses.dataclass(frozen=True)
class PruneConfig:
    """Mirrors ``cmoop_prune``.  Domain: ``sparsity`` 0 (off) or in (0, 1); ``begin_step`` / ``end_step`` >= 0, in Adam
    iterations; ``objective`` a bool: the evaluator puts the pruned size in the place of ``size_mb`` in ``objs`` and in the
    size constraint (False only adds the numbers); ``skip_small``: the first convolution and the depthwise kernels are copied."""
    sparsity: float = 0.8
    begin_step: int = 0
    end_step: int = 0
    objective: bool = True
    skip_small: bool = True

    @staticmethod
    def polynomial(sparsity: float, begin_epoch: int, end_epoch: int, steps_per_epoch: int, **over) -> "PruneConfig":
        """The cubic ramp from the first step of ``begin_epoch`` to the first step of ``end_epoch`` (epochs from 0)."""
        return PruneConfig(sparsity=float(sparsity), begin_step=int(begin_epoch) * int(steps_per_epoch),
                           end_step=int(end_epoch) * int(steps_per_epoch), **over)

    @property
    def enabled(self) -> bool:
        return float(self.sparsity) != 0.0

    def _struct(self) -> PruneStruct:
        st = PruneStruct()
        st.sparsity, st.begin_step, st.end_step = float(self.sparsity), int(self.begin_step), int(self.end_step)
        st.objective, st.skip_small = int(self.objective), int(self.skip_small)
        return st

    def check(self) -> "PruneConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        return check_struct(self._struct(), self)


def check_struct(st: PruneStruct, ret=None):
    L = _lib.lib()
    if L.cmoop_prune_check(C.byref(st)) != 0:
        raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
    return ret


def default_prune_config() -> PruneConfig:
    """cmoop_prune_default as a PruneConfig: off."""
    st = PruneStruct()
    _lib.check(_lib.lib().cmoop_prune_default(C.byref(st)))
    return PruneConfig(sparsity=float(st.sparsity), begin_step=int(st.begin_step), end_step=int(st.end_step),
                       objective=bool(st.objective), skip_small=bool(st.skip_small))


def sparsity_at(cfg: PruneConfig, it: int) -> float:
    """s(it) of the schedule, in IEEE double with products only (the twin of ``cmoop_prune_sparsity_at``, bit for bit)."""
    it, b, e = int(it), int(cfg.begin_step), int(cfg.end_step)
    if it < b:
        return 0.0
    if it >= e or e <= b:
        return float(cfg.sparsity)
    u = float(it - b) / float(e - b)
    r = 1.0 - u
    r2 = r * r
    r3 = r2 * r
    return float(cfg.sparsity) * (1.0 - r3)


def c_sparsity_at(cfg: PruneConfig, it: int) -> float:
    """``cmoop_prune_sparsity_at``."""
    st, out = cfg._struct(), C.c_double()
    _lib.check(_lib.lib().cmoop_prune_sparsity_at(C.byref(st), C.c_int64(int(it)), C.byref(out)))
    return float(out.value)


def k_of(length: int, s: float) -> int:
    """``floor(s * len)`` in IEEE double."""
    return int(math.floor(float(s) * float(int(length))))


def prune_ref(w, k: int):
    """The definition restated in numpy: ``w`` float32 (any shape, one tensor), ``k`` elements to prune -> (w_eff float32 of
    the same shape, the number of zeros written).  Integer compares only."""
    w = np.ascontiguousarray(w, np.float32)
    k = int(k)
    if not 0 <= k <= w.size:
        raise ValueError("k must be in [0, len]")
    if k == 0:
        return w.copy(), 0
    bits = w.reshape(-1).view(np.uint32)
    keys = bits & ABS_MASK
    t = np.partition(keys, k - 1)[k - 1]
    keep = keys > t
    out = np.where(keep, bits, np.uint32(0)).astype(np.uint32)
    return out.view(np.float32).reshape(w.shape), int((~keep).sum())


def prune_table(gene, variant: int, classes: int, skip_small: bool = True) -> List[Tuple[int, int, int]]:
    """[(off, len, k)] of the kernel tensors of a candidate in arena order, from ``genes.param_tensors``: k = -1 for a pruned
    tensor (``floor(s * len)`` at the s of each call), 0 for a copied one (the first convolution and the depthwise kernels
    under ``skip_small``).  The twin of ``cmoop_prune_table``."""
    rows, off, first = [], 0, True
    for name, shape, role in G.param_tensors(gene, variant, classes):
        n = int(np.prod(shape))
        if role == "kernel":
            small = first or name.endswith("/depthwise_kernel")
            rows.append((off, n, 0 if (small and skip_small) else -1))
            first = False
        off += n
    return rows


prune_table_ref = prune_table


def c_prune_table(gene, variant: int, classes: int, skip_small: bool = True):
    """``cmoop_prune_table``: rows as ``prune_table`` gives them."""
    g, cap = (C.c_int32 * 6)(*(int(v) for v in gene)), 128
    rows, n = np.zeros((cap, 3), np.int64), C.c_int32()
    _lib.check(_lib.lib().cmoop_prune_table(g, C.c_int32(int(variant)), C.c_int32(int(classes)), C.c_int32(int(skip_small)),
                                            _lib.ptr(rows), C.c_int32(cap), C.byref(n)))
    return [tuple(int(v) for v in r) for r in rows[:n.value]]


def c_prune_size_bytes(gene, variant: int, classes: int, sparsity: float, bits: int = 0, skip_small: bool = True) -> int:
    """``cmoop_prune_size_bytes``."""
    g, out = (C.c_int32 * 6)(*(int(v) for v in gene)), C.c_int64()
    _lib.check(_lib.lib().cmoop_prune_size_bytes(g, C.c_int32(int(variant)), C.c_int32(int(classes)), C.c_double(float(sparsity)),
                                                 C.c_int32(int(bits)), C.c_int32(int(skip_small)), C.byref(out)))
    return int(out.value)


def row_k(row, s: float) -> int:
    """The k of one table row at sparsity s."""
    return int(row[2]) if int(row[2]) >= 0 else k_of(row[1], s)


def prune_rows_ref(flat, rows, s: float):
    """``prune_ref`` over the tensors of ``rows`` inside the float32 arena ``flat`` -> (w_eff flat: every element outside the
    pruned tensors a bit copy; zeros uint32 [len(rows)])."""
    flat = np.ascontiguousarray(flat, np.float32).reshape(-1)
    out, zeros = flat.copy(), np.zeros(len(rows), np.uint32)
    for i, row in enumerate(rows):
        off, n = int(row[0]), int(row[1])
        out[off:off + n], zeros[i] = prune_ref(flat[off:off + n], row_k(row, s))
    return out, zeros


def prune_params_ref(flat, gene, variant: int, classes: int, s: float, skip_small: bool = True):
    """The pruned arena of a candidate's parameters ``flat`` at sparsity ``s`` -> (w_eff flat, zeros), as
    ``NetSession.get_pruned`` at ``s`` = the final sparsity."""
    flat = np.ascontiguousarray(flat, np.float32).reshape(-1)
    if flat.size != G.param_count(gene, variant, classes):
        raise ValueError("flat does not hold the candidate's parameters")
    return prune_rows_ref(flat, prune_table(gene, variant, classes, skip_small), s)


def _table(rows):
    return np.ascontiguousarray(np.asarray(rows, np.int64).reshape(-1, 3))


def prune_weights(w, rows, s: float, out, zeros=None) -> int:
    """``cmoop_prune_weights``: the launch sequence alone.  ``w`` / ``out`` CUDA float32 [n], ``zeros`` CUDA int32 [len(rows)]
    (read as uint32) or None; ``rows`` as ``prune_table`` gives them, or with explicit k.  Returns the number of launches."""
    import torch
    tab, n = _table(rows), C.c_int32()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_prune_weights(_lib.ptr(w), C.c_int64(int(w.numel())), _lib.ptr(tab), C.c_int32(len(tab)),
                                              C.c_double(float(s)), _lib.ptr(out), _lib.ptr(zeros), C.byref(n)))
    return int(n.value)


def prune_weights_time(w, rows, s: float, out, iters: int = 100) -> float:
    """``cmoop_prune_weights_time``: average milliseconds of the launch sequence."""
    import torch
    tab, ms = _table(rows), C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_prune_weights_time(_lib.ptr(w), C.c_int64(int(w.numel())), _lib.ptr(tab), C.c_int32(len(tab)),
                                                   C.c_double(float(s)), _lib.ptr(out), None, C.c_int32(int(iters)), C.byref(ms)))
    return float(ms.value)
