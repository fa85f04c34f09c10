"""Train-time augmentation of the [T, F] feature patches: time shift, SpecAugment masks, feature noise.

Opt-in and off by default (the reference trains on the same resident patches every epoch and has no counterpart).
``AugmentConfig`` mirrors ``cmoop_augment`` (include/cmoop.h, where the semantics are fixed); the HIP kernel applies it
to every train batch of a net.  ``augment_reference`` / ``augment_draws`` restate the same semantics in numpy, bit for
bit: all randomness is the counter RNG (integer arithmetic) keyed by (net seed, global train step, position of the row
in its batch), and the only floating-point work is one fp32 multiply and one fp32 add per noisy element.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math

import numpy as np

from . import _lib

STREAM_AUGMENT = 0x4000      # row draws; 0x4001 / 0x4002: the two noise words (csrc/common.h)
MAX_MASKS = 4
N_DRAWS = 18                 # gate, shift, 4 x (w, t0), 4 x (w, f0)


AugmentStruct = _lib.Augment   # cmoop_augment (include/cmoop.h)


@dataclasses.dataclass(frozen=True)
class AugmentConfig:
    """What a train step does to each row of its batch; mirrors ``cmoop_augment``.

    With probability ``p`` a row is augmented, otherwise it is copied: shifted by s frames, s uniform in
    [-time_shift, time_shift]; ``time_masks`` runs of at most ``time_mask_max`` frames and ``freq_masks`` runs of at most
    ``freq_mask_max`` bands (at most 4 each, placed after the shift) and the frames the shift uncovers are set to
    ``fill`` (0.0: the feature mean after the StandardScaler); ``noise_std`` > 0 adds a bounded, zero-mean variate of
    that standard deviation to every position that was not filled.

    Domain for [T, F] patches: 0 <= p <= 1, 0 <= time_shift < T, masks 0..4, time_mask_max <= T, freq_mask_max <= F,
    noise_std >= 0 and finite, fill finite.  The default does nothing; a config that does nothing is the same as None.
    """
    p: float = 1.0
    time_shift: int = 0
    time_masks: int = 0
    time_mask_max: int = 0
    freq_masks: int = 0
    freq_mask_max: int = 0
    noise_std: float = 0.0
    fill: float = 0.0

    @classmethod
    def preset(cls, name: str = "kws", **over) -> "AugmentConfig":
        """Named recipes.

        "kws" -- shift of up to 10 frames, 2 time masks of at most 10 frames, 2 frequency masks of at most 5 bands, every
                 row (p = 1), no noise.  BUILD-DEFINED: the reference has no augmentation; this is the usual keyword-
                 spotting recipe (random time shift + SpecAugment masks) scaled to the 101 x 40 log-mel patch of a 1 s
                 clip, not something taken from it.
        """
        if name == "kws":
            return dataclasses.replace(cls(time_shift=10, time_masks=2, time_mask_max=10, freq_masks=2, freq_mask_max=5), **over)
        raise ValueError(f"unknown augmentation preset {name!r} (known: 'kws')")

    @property
    def enabled(self) -> bool:
        """p > 0 and at least one of: a shift, a mask with a non-zero largest width, noise."""
        return self.p > 0 and (self.time_shift > 0 or (self.time_masks > 0 and self.time_mask_max > 0) or
                               (self.freq_masks > 0 and self.freq_mask_max > 0) or self.noise_std > 0)

    def _struct(self) -> AugmentStruct:
        return AugmentStruct(int(self.time_shift), int(self.time_masks), int(self.time_mask_max), int(self.freq_masks),
                             int(self.freq_mask_max), 0, float(self.p), float(self.noise_std), float(self.fill))

    def check(self, T: int, F: int) -> "AugmentConfig":
        """Raise ValueError naming the offending field when the config is outside the domain for [T, F] patches (host only)."""
        st = self._struct()
        L = _lib.lib()
        if L.cmoop_augment_check(C.byref(st), int(T), int(F)) != 0:
            raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
        return self


def default_augment_config() -> AugmentConfig:
    """cmoop_augment_default as an AugmentConfig (equals AugmentConfig())."""
    st = AugmentStruct()
    _lib.check(_lib.lib().cmoop_augment_default(C.byref(st)))
    return AugmentConfig(p=st.p, time_shift=st.time_shift, time_masks=st.time_masks, time_mask_max=st.time_mask_max,
                         freq_masks=st.freq_masks, freq_mask_max=st.freq_mask_max, noise_std=st.noise_std, fill=st.fill)


# ---- the counter RNG of csrc/common.h on uint32 arrays (kept in uint64 and masked: no overflow warnings) ----------------
_M32 = np.uint64(0xFFFFFFFF)


def _fmix32(h):
    h = np.asarray(h, np.uint64) & _M32
    h = h ^ (h >> np.uint64(16))
    h = (h * np.uint64(0x85EBCA6B)) & _M32
    h = h ^ (h >> np.uint64(13))
    h = (h * np.uint64(0xC2B2AE35)) & _M32
    return h ^ (h >> np.uint64(16))


def _prefix(seed: int, stream: int, ctr: int):
    h = _fmix32(np.uint64(((int(seed) & 0xFFFFFFFF) + 0x9E3779B9) & 0xFFFFFFFF))
    h = _fmix32(h ^ np.uint64(stream))
    return _fmix32(h ^ np.uint64(int(ctr) & 0xFFFFFFFF))


def _u32(prefix, idx):
    return _fmix32(prefix ^ (np.asarray(idx, np.uint64) & _M32))


def _range(u, n):
    """R(u, n) = (u * n) >> 32 on uint64 arrays holding 32-bit values."""
    return (u * np.asarray(n, np.uint64)) >> np.uint64(32)


def _checked(config: AugmentConfig, T: int, F: int) -> None:
    """The domain of cmoop_augment_check, restated (host arithmetic only; the library is not needed)."""
    c = config
    if not 0.0 <= c.p <= 1.0:
        raise ValueError("augment: p must be in [0, 1]")
    if not 0 <= c.time_shift < T:
        raise ValueError(f"augment: time_shift must be in [0, T = {T})")
    if not 0 <= c.time_masks <= MAX_MASKS:
        raise ValueError("augment: time_masks must be in [0, 4]")
    if not 0 <= c.time_mask_max <= T:
        raise ValueError(f"augment: time_mask_max must be in [0, T = {T}]")
    if not 0 <= c.freq_masks <= MAX_MASKS:
        raise ValueError("augment: freq_masks must be in [0, 4]")
    if not 0 <= c.freq_mask_max <= F:
        raise ValueError(f"augment: freq_mask_max must be in [0, F = {F}]")
    if not (math.isfinite(c.noise_std) and c.noise_std >= 0):
        raise ValueError("augment: noise_std must be finite and >= 0")
    if not math.isfinite(c.fill):
        raise ValueError("augment: fill must be finite")


def augment_draws(config: AugmentConfig, seed: int, step: int, B: int, T: int, F: int) -> np.ndarray:
    """int32 [B, 18]: per batch position the gate, the shift s, (w, t0) of the four time masks and (w, f0) of the four
    frequency masks -- what ``cmoop_augment_draws`` returns for b = 0 .. B-1.  Unused masks are zero, and so is everything
    after the gate of a gated-off row (it is a plain copy)."""
    _checked(config, T, F)
    pre = _prefix(seed, STREAM_AUGMENT, step)
    base = np.uint64(32) * np.arange(B, dtype=np.uint64)

    def u(k):
        return _u32(pre, base + np.uint64(k))
    d = np.zeros((B, N_DRAWS), np.int64)
    d[:, 0] = (u(0) >> np.uint64(8)) < np.uint64(int(math.floor(config.p * 16777216.0)))
    S = int(config.time_shift)
    d[:, 1] = _range(u(1), 2 * S + 1).astype(np.int64) - S
    for j in range(int(config.time_masks)):
        w = _range(u(2 + 2 * j), int(config.time_mask_max) + 1)
        d[:, 2 + 2 * j] = w
        d[:, 3 + 2 * j] = _range(u(3 + 2 * j), np.uint64(T + 1) - w)
    for j in range(int(config.freq_masks)):
        w = _range(u(10 + 2 * j), int(config.freq_mask_max) + 1)
        d[:, 10 + 2 * j] = w
        d[:, 11 + 2 * j] = _range(u(11 + 2 * j), np.uint64(F + 1) - w)
    d[d[:, 0] == 0, 1:] = 0
    return d.astype(np.int32)


def augment_reference(X_rows, config: AugmentConfig, seed: int, step: int) -> np.ndarray:
    """The augmented batch, float32 [B, T, F], of the float32 rows ``X_rows`` [B, T, F] (row b = batch position b, already
    gathered) for a net of ``seed`` at global train step ``step``: the numpy restatement of the kernel, bit for bit."""
    X = np.ascontiguousarray(X_rows, np.float32)
    if X.ndim != 3:
        raise ValueError("augment_reference expects rows [B, T, F]")
    B, T, F = X.shape
    if B * T * F >= 1 << 32:
        raise ValueError("augment_reference: B * T * F must stay below 2^32")
    d = augment_draws(config, seed, step, B, T, F).astype(np.int64)
    fill = np.float32(config.fill)
    out = X.copy()
    t, f = np.arange(T), np.arange(F)
    noisy = config.noise_std > 0
    if noisy:
        k = np.float32(np.float64(config.noise_std) * np.sqrt(np.float64(3.0)) / np.float64(65536.0))
        pa, pc = _prefix(seed, STREAM_AUGMENT + 1, step), _prefix(seed, STREAM_AUGMENT + 2, step)
    for b in range(B):
        if not d[b, 0]:
            continue
        ts = t - d[b, 1]
        drop_t = (ts < 0) | (ts >= T)
        drop_f = np.zeros(F, bool)
        for j in range(MAX_MASKS):
            drop_t |= (t >= d[b, 3 + 2 * j]) & (t < d[b, 3 + 2 * j] + d[b, 2 + 2 * j])
            drop_f |= (f >= d[b, 11 + 2 * j]) & (f < d[b, 11 + 2 * j] + d[b, 10 + 2 * j])
        row = X[b][np.clip(ts, 0, T - 1)]
        if noisy:
            e = (np.uint64(b * T) + t.astype(np.uint64))[:, None] * np.uint64(F) + f.astype(np.uint64)[None, :]
            a, c = _u32(pa, e), _u32(pc, e)
            lo = np.uint64(0xFFFF)
            n = ((a & lo) + (a >> np.uint64(16)) + (c & lo) + (c >> np.uint64(16))).astype(np.int64) - 131070
            nk = n.astype(np.float32) * k          # one fp32 multiply ...
            row = row + nk                         # ... and one fp32 add, separately rounded
        out[b] = np.where(drop_t[:, None] | drop_f[None, :], fill, row)
    return out


def augment_batch(X, config: AugmentConfig, seed: int, step: int, idx=None, row0: int = 0, B: int = None):
    """The kernel alone (``cmoop_augment_batch``): X CUDA float32 [N, T, F], idx CUDA int32 or None -> CUDA float32
    [B, T, F], the augmented rows idx[row0 + b] (idx None: row0 + b).  Any config of the domain, enabled or not."""
    import torch
    if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 3 and X.is_contiguous()):
        raise ValueError("augment_batch expects a contiguous CUDA float32 tensor [N, T, F]")
    n = int(len(idx)) if idx is not None else int(X.shape[0])
    if B is None:
        B = n - int(row0)
    if not (row0 >= 0 and B >= 0 and row0 + B <= n):
        raise ValueError("augment_batch: rows row0 .. row0 + B lie outside the data")
    T, F = int(X.shape[1]), int(X.shape[2])
    config.check(T, F)
    out = torch.empty((B, T, F), dtype=torch.float32, device=X.device)
    st = config._struct()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_augment_batch(C.byref(st), _lib.ptr(X), _lib.ptr(idx), int(row0), B, T, F, int(seed) & 0xFFFFFFFF,
                                              int(step) & 0xFFFFFFFF, _lib.ptr(out)))
    return out
