"""Audio front end + per-bin standardisation on the GPU (libcmoop_hip.so).

The reference loads pre-extracted log-mel features (nsga_penalty.py:64-71,
sa_nsga_penalty.py:58); the north-star adds the extraction beneath that loader:
1 s @ 16 kHz clips -> framing (n_fft 512, Hann 400, hop 160, centre-padded) ->
|STFT|^2 -> 40 Slaney mel bands 20-7600 Hz -> log(mel + 1e-6)  => [N,101,40].
``prepare_dataset`` mirrors nsga_penalty.py:85-155 (StandardScaler per mel bin
over the N*T rows) including the per-script quirks Q1/Q2 of SURVEY §8a.

``FrontendConfig`` names any other geometry the library serves (n_fft 256-2048,
up to 128 mel bands; log, dB, linear power or PCEN scale); ``log_mel`` / ``mfcc``
without a config are the fixed geometry above, unchanged.

PCEN (per-channel energy normalisation, ``PcenConfig``) divides every band's mel power by a
causal first-order smoothing of itself: the recording level and the stationary background
leave the features.  ``log_mel`` normalises each clip from its own first frame in the launch
that makes the power, ``log_mel_stream`` normalises ONE recording once (three more launches),
``pcen`` does either on a power tensor; ``pcen_reference`` / ``pcen_scan_reference`` are the
host restatements the tests hold the kernels to.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
from typing import Optional

import numpy as np

from . import _lib
from .resample import resample_poly, to_rate  # noqa: F401  (frontend.resample_poly)

HOP, N_MELS = 160, 40
MFCC_MAX_MELS = 64      # cmoop_mfcc's DCT kernel holds at most a 64 x 64 basis

SCALE_LOG, SCALE_DB, SCALE_POWER = 0, 1, 2
_SCALE_CODES = {"log": SCALE_LOG, "db": SCALE_DB, "power": SCALE_POWER, "pcen": SCALE_POWER}   # PCEN runs on the power scale


class FrontendConfigStruct(C.Structure):
    """cmoop_frontend_config (include/cmoop.h)."""
    _fields_ = [(n, C.c_int32) for n in ("sr", "n_fft", "win", "hop", "n_mels", "scale", "db_ref_max")] + \
        [(n, C.c_float) for n in ("fmin", "fmax", "log_eps", "db_amin", "top_db")]


class PcenStruct(C.Structure):
    """cmoop_pcen (include/cmoop.h), 48 bytes."""
    _fields_ = [(n, C.c_double) for n in ("s", "alpha", "delta", "r", "eps", "input_scale")]


@dataclasses.dataclass(frozen=True)
class PcenConfig:
    """Per-channel energy normalisation of mel power; mirrors ``cmoop_pcen``.

    For one band with mel power ``P[t]`` and ``E[t] = input_scale * P[t]``::

        M[-1] = E[0];   M[t] = M[t-1] + s * (E[t] - M[t-1])
        out[t] = (E[t] / (eps + M[t]) ** alpha + delta) ** r - delta ** r

    Domain, all finite: 0 < s <= 1, 0 <= alpha <= 1, delta >= 0, 0 < r <= 1, eps > 0, input_scale > 0.  The default is
    ``cmoop_pcen_default``: s 0.025, alpha 0.98, delta 2, r 0.5, eps 1e-6, input_scale 1 (the values of Wang et al. 2017,
    "Trainable frontend for robust and far-field keyword spotting"; s 0.025 is a 0.4 s time constant at a 10 ms hop).

    Presets are BUILD-DEFINED, as ``FrontendConfig.preset("birdclef_128")`` is: the reference ships pre-extracted
    features and no PCEN recipe, so these are common published settings, not the reference's.

    "speech"      -- the default above.
    "bioacoustic" -- a 60 ms time constant at the ``birdclef_128`` frame rate (32 kHz, hop 512: s = 0.2335), alpha 0.8,
                     delta 10, r 0.25, eps 1e-6, input_scale 1: the short smoother, weaker gain control and stronger
                     compression that Lostanlen et al. 2019 ("Per-channel energy normalization: why and how")
                     recommend for bird calls over far-field background.
    """
    s: float = 0.025
    alpha: float = 0.98
    delta: float = 2.0
    r: float = 0.5
    eps: float = 1e-6
    input_scale: float = 1.0

    @classmethod
    def preset(cls, name: str = "speech") -> "PcenConfig":
        if name == "speech":
            return cls()
        if name == "bioacoustic":
            return cls.from_time_constant(0.06, 32000, 512, alpha=0.8, delta=10.0, r=0.25)
        raise ValueError(f"unknown PCEN preset {name!r} (known: 'speech', 'bioacoustic')")

    @classmethod
    def from_time_constant(cls, time_constant_s: float, sr: int, hop: int, **kw) -> "PcenConfig":
        """``s`` from the smoother's time constant: ``Tf = time_constant_s * sr / hop`` frames,
        ``s = (sqrt(1 + 4 Tf^2) - 1) / (2 Tf^2)`` (host only); the other fields from ``kw``."""
        if "s" in kw:
            raise ValueError("from_time_constant computes s; do not pass it")
        s = C.c_double()
        L = _lib.lib()
        if L.cmoop_pcen_smoothing(C.c_double(float(time_constant_s)), C.c_int32(int(sr)), C.c_int32(int(hop)), C.byref(s)) != 0:
            raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
        return cls(s=float(s.value), **kw)

    def _struct(self) -> PcenStruct:
        return PcenStruct(*(float(getattr(self, f.name)) for f in dataclasses.fields(self)))

    def check(self) -> "PcenConfig":
        """Raise ValueError naming the offending field when a value is outside the domain (host only)."""
        st = self._struct()
        L = _lib.lib()
        if L.cmoop_pcen_check(C.byref(st)) != 0:
            raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
        return self


def default_pcen_config() -> PcenConfig:
    """cmoop_pcen_default as a PcenConfig (equals PcenConfig())."""
    st = PcenStruct()
    _lib.check(_lib.lib().cmoop_pcen_default(C.byref(st)))
    return PcenConfig(s=st.s, alpha=st.alpha, delta=st.delta, r=st.r, eps=st.eps, input_scale=st.input_scale)


def pcen_stream_plan(n_frames: int):
    """(chunk, n_chunks) of the stream form for a recording of n_frames frames (host only): chunk depends on n_frames
    alone, is a multiple of 64 and at least 64; n_chunks = ceil(n_frames / chunk)."""
    chunk, n_chunks = C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().cmoop_pcen_stream_plan(C.c_int64(int(n_frames)), C.byref(chunk), C.byref(n_chunks)))
    return int(chunk.value), int(n_chunks.value)


@dataclasses.dataclass(frozen=True)
class FrontendConfig:
    """Geometry and output scale of the front end; mirrors ``cmoop_frontend_config``.

    Domain: n_fft in {256, 512, 1024, 2048}, 1 <= win <= n_fft, hop >= 1, 1 <= n_mels <= 128,
    0 <= fmin < fmax <= sr/2.  ``scale`` is "log" (``log(mel + log_eps)``), "db"
    (``10 log10(max(db_amin, mel)) - 10 log10(max(db_amin, ref))`` with ref = 1.0, or the clip's own largest mel
    power when ``db_ref_max``; then values more than ``top_db`` below the clip's maximum are raised to that floor,
    ``top_db < 0`` turns the floor off), "power" (the linear mel power) or "pcen" (the mel power normalised per band
    by ``pcen``, see ``PcenConfig``; ``pcen=None`` means ``PcenConfig()``; the field is ignored on the other scales).
    The default is the build-defined GSC geometry of ``log_mel(wav)``.
    """
    sr: int = 16000
    n_fft: int = 512
    win: int = 400
    hop: int = 160
    n_mels: int = 40
    fmin: float = 20.0
    fmax: float = 7600.0
    log_eps: float = 1e-6
    scale: str = "log"
    db_ref_max: bool = False
    db_amin: float = 1e-10
    top_db: float = 80.0
    pcen: Optional[PcenConfig] = None

    @classmethod
    def preset(cls, name: str = "gsc") -> "FrontendConfig":
        """Named configurations.

        "gsc"          -- the default: 16 kHz, n_fft 512, Hann 400, hop 160, 40 mels 20-7600 Hz, log scale.
        "birdclef_128" -- 32 kHz, n_fft 2048, Hann 2048, hop 512, 128 mels 20-16000 Hz, dB scale relative to the
                          clip's maximum with an 80 dB floor; a 65 280-sample clip gives a 128 x 128 patch.
                          BUILD-DEFINED: the reference loads pre-extracted BirdCLEF mel spectrograms and does not
                          publish the recipe that made them ("true shape unknown"); this preset is the
                          common mel-spectrogram recipe that yields the 128 x 128 shape the B-variant path runs at.
        """
        if name == "gsc":
            return cls()
        if name == "birdclef_128":
            return cls(sr=32000, n_fft=2048, win=2048, hop=512, n_mels=128, fmin=20.0, fmax=16000.0, scale="db",
                       db_ref_max=True, db_amin=1e-10, top_db=80.0)
        raise ValueError(f"unknown front end preset {name!r} (known: 'gsc', 'birdclef_128')")

    def _struct(self) -> FrontendConfigStruct:
        if self.scale not in _SCALE_CODES:
            raise ValueError("front end config: scale must be 'log', 'db', 'power' or 'pcen'")
        if self.pcen is not None and not isinstance(self.pcen, PcenConfig):
            raise ValueError("front end config: pcen must be a PcenConfig or None")
        return FrontendConfigStruct(int(self.sr), int(self.n_fft), int(self.win), int(self.hop), int(self.n_mels),
                                    _SCALE_CODES[self.scale], int(bool(self.db_ref_max)),
                                    float(self.fmin), float(self.fmax), float(self.log_eps), float(self.db_amin),
                                    float(self.top_db))

    def check(self) -> "FrontendConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        st = self._struct()
        L = _lib.lib()
        if L.cmoop_frontend_check(C.byref(st)) != 0:
            raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
        if self.scale == "pcen":
            self.pcen_config().check()
        return self

    def pcen_config(self) -> PcenConfig:
        """The PCEN parameters the "pcen" scale runs with: the ``pcen`` field, or ``PcenConfig()`` when it is None."""
        return self.pcen if self.pcen is not None else PcenConfig()

    def frames(self, n_samples: int) -> int:
        """T = 1 + n_samples // hop (host only)."""
        st, T = self.check()._struct(), C.c_int32()
        _lib.check(_lib.lib().cmoop_frontend_frames(C.byref(st), C.c_int32(int(n_samples)), C.byref(T)))
        return int(T.value)

    def mel_basis(self) -> np.ndarray:
        """The mel table the kernel reads, dense: float32 [n_mels, 1 + n_fft // 2] (host only)."""
        st = self.check()._struct()
        out = np.zeros((self.n_mels, 1 + self.n_fft // 2), np.float32)
        _lib.check(_lib.lib().cmoop_frontend_mel_basis(C.byref(st), _lib.ptr(out)))
        return out


def default_frontend_config() -> FrontendConfig:
    """cmoop_frontend_config_default as a FrontendConfig (equals FrontendConfig())."""
    st = FrontendConfigStruct()
    _lib.check(_lib.lib().cmoop_frontend_config_default(C.byref(st)))
    return FrontendConfig(sr=st.sr, n_fft=st.n_fft, win=st.win, hop=st.hop, n_mels=st.n_mels, fmin=st.fmin, fmax=st.fmax,
                          log_eps=st.log_eps, scale={SCALE_DB: "db", SCALE_POWER: "power"}.get(st.scale, "log"),
                          db_ref_max=bool(st.db_ref_max),
                          db_amin=st.db_amin, top_db=st.top_db)


def _log_mel_config(wav, config: FrontendConfig):
    import torch
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2):
        raise ValueError("log_mel expects a CUDA float32 tensor [n_clips, n_samples]")
    wav = wav.contiguous()
    n, L = int(wav.shape[0]), int(wav.shape[1])
    out = torch.empty((n, config.frames(L), config.n_mels), dtype=torch.float32, device=wav.device)
    st = config._struct()
    torch.cuda.synchronize()
    if config.scale == "pcen":                                    # power and the per-clip recurrence in one launch
        pc = config.pcen_config()._struct()
        _lib.check(_lib.lib().cmoop_logmel_pcen(C.byref(st), C.byref(pc), _lib.ptr(wav), C.c_int64(n), C.c_int32(L), _lib.ptr(out)))
    else:
        _lib.check(_lib.lib().cmoop_logmel_ex(C.byref(st), _lib.ptr(wav), C.c_int64(n), C.c_int32(L), _lib.ptr(out)))
    return out


def log_mel(wav, config: FrontendConfig | None = None, sr: int | None = None):
    """wav: CUDA float32 [N, L] -> CUDA float32 [N, 1 + L//160, 40]; with a config, [N, 1 + L//hop, n_mels] in its scale.
    ``sr``: the rate the clips arrive at; when it differs from the config's (16000 without one) they are resampled to it first
    (``resample_poly``), so L above is then the resampled length."""
    import torch
    if sr is not None:
        wav = to_rate(wav, sr, 16000 if config is None else config.sr, "log_mel")
    if config is not None:
        return _log_mel_config(wav, config)
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 2):
        raise ValueError("log_mel expects a CUDA float32 tensor [n_clips, n_samples]")
    wav = wav.contiguous()
    n, L = int(wav.shape[0]), int(wav.shape[1])
    out = torch.empty((n, 1 + L // HOP, N_MELS), dtype=torch.float32, device=wav.device)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_logmel(_lib.ptr(wav), C.c_int64(n), C.c_int32(L), _lib.ptr(out)))
    return out


def log_mel_stream(wav, config: FrontendConfig | None = None, sr: int | None = None):
    """ONE recording, CUDA float32 [L] -> CUDA float32 [1 + L//hop, n_mels], its frames spread over the whole chip.

    Log scale: frame for frame the bits of ``log_mel(wav[None], config)[0]``.  dB scale: the UN-REFERENCED
    ``10 log10(max(db_amin, mel))`` -- the reference and the ``top_db`` floor are quantities of a window, applied by
    ``NetSession.predict_stream`` to each window it cuts from the stream.  Power scale: the clip call's bits.  PCEN scale:
    the recording is normalised ONCE, from its first frame, by the chunked three-launch scan (``pcen`` on the power
    stream, bit for bit); windows cut from it need no per-window step, and a recording of at most
    ``pcen_stream_plan(T)[0]`` frames carries the bits of ``log_mel(wav[None], config)[0]``.
    ``config=None`` is ``FrontendConfig()``.  ``sr``: the rate the recording arrives at; when it differs from the config's it
    is resampled to it first (``resample_poly``), so L above is then the resampled length."""
    import torch
    if config is None:
        config = FrontendConfig()
    if sr is not None:
        wav = to_rate(wav, sr, config.sr, "log_mel_stream")
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 1):
        raise ValueError("log_mel_stream expects a CUDA float32 tensor [n_samples]")
    wav = wav.contiguous()
    L = int(wav.shape[0])
    if L < 1:
        raise ValueError("log_mel_stream: the recording is empty")
    out = torch.empty((config.frames(L), config.n_mels), dtype=torch.float32, device=wav.device)
    st = config._struct()
    torch.cuda.synchronize()
    if config.scale == "pcen":
        pc = config.pcen_config()._struct()
        _lib.check(_lib.lib().cmoop_logmel_pcen_stream(C.byref(st), C.byref(pc), _lib.ptr(wav), C.c_int64(L), _lib.ptr(out)))
    else:
        _lib.check(_lib.lib().cmoop_logmel_stream(C.byref(st), _lib.ptr(wav), C.c_int64(L), _lib.ptr(out)))
    return out


def _as_pcen_config(config) -> PcenConfig:
    if config is None:
        return PcenConfig()
    if isinstance(config, FrontendConfig):
        return config.pcen_config()
    if isinstance(config, PcenConfig):
        return config
    raise ValueError("pcen expects a PcenConfig, a FrontendConfig or None")


def pcen(power, config=None):
    """PCEN of a mel-power tensor, returned as a new tensor (the input is only read).

    CUDA float32 ``[n, T, F]``: every clip from its own first frame (``cmoop_pcen_apply``).  CUDA float32 ``[T, F]``: ONE
    recording, its frames spread over the chip by the chunked scan (``cmoop_pcen_stream``).  ``config`` is a
    ``PcenConfig``, a ``FrontendConfig`` (its ``pcen_config()``) or None (``PcenConfig()``).  1 <= F <= 128."""
    import torch
    pc = _as_pcen_config(config)
    if not (isinstance(power, torch.Tensor) and power.is_cuda and power.dtype == torch.float32 and power.dim() in (2, 3)):
        raise ValueError("pcen expects a CUDA float32 tensor [n, T, F] or [T, F]")
    out = power.contiguous().clone()
    st = pc._struct()
    T, F = int(out.shape[-2]), int(out.shape[-1])
    torch.cuda.synchronize()
    if out.dim() == 3:
        _lib.check(_lib.lib().cmoop_pcen_apply(C.byref(st), _lib.ptr(out), C.c_int64(int(out.shape[0])), C.c_int32(T), C.c_int32(F)))
    else:
        _lib.check(_lib.lib().cmoop_pcen_stream(C.byref(st), _lib.ptr(out), C.c_int64(T), C.c_int32(F)))
    return out


def pcen_reference(P, config=None, dtype=np.float64) -> np.ndarray:
    """Host numpy: the serial definition of ``PcenConfig`` along axis -2 of ``P [..., T, F]``, every operation (the six
    parameters included) in ``dtype``; float32 is the plain restatement of the device arithmetic without its fused update."""
    pc = _as_pcen_config(config)
    dt = np.dtype(dtype).type
    s, alpha, delta, r, eps, gain = (dt(getattr(pc, k)) for k in ("s", "alpha", "delta", "r", "eps", "input_scale"))
    E = np.asarray(P, dtype=dt) * gain
    if E.ndim < 2:
        raise ValueError("pcen_reference expects [..., T, F]")
    out = np.empty_like(E)
    M = E[..., 0, :].copy()
    floor = np.power(np.zeros_like(M) + delta, r)
    for t in range(E.shape[-2]):
        e = E[..., t, :]
        M = M + s * (e - M)
        out[..., t, :] = np.power(e / np.power(eps + M, alpha) + delta, r) - floor
    assert out.dtype == np.dtype(dtype)
    return out


def pcen_scan_reference(P, config=None, chunk: int = 64) -> np.ndarray:
    """Host numpy, float64: the three-pass composition of the stream form on ``P [T, F]`` -- (1) every full chunk's end
    state from a zero start, (2) ``carry[0] = E[0]``, ``carry[c+1] = (1 - s)^chunk carry[c] + local[c]``, (3) the serial
    recurrence of each chunk from ``carry[c]``.  Equals ``pcen_reference`` up to rounding for any ``chunk >= 1``."""
    pc = _as_pcen_config(config)
    chunk = int(chunk)
    if chunk < 1:
        raise ValueError("chunk must be at least 1")
    E = np.asarray(P, np.float64) * float(pc.input_scale)
    if E.ndim != 2:
        raise ValueError("pcen_scan_reference expects [T, F]")
    T, F = E.shape
    s, n_chunks = float(pc.s), -(-T // chunk)
    local = np.zeros((n_chunks, F))
    for c in range(n_chunks - 1):
        M = np.zeros(F)
        for t in range(c * chunk, (c + 1) * chunk):
            M = M + s * (E[t] - M)
        local[c] = M
    carry = np.zeros((n_chunks, F))
    carry[0] = E[0]
    a_chunk = (1.0 - s) ** chunk
    for c in range(n_chunks - 1):
        carry[c + 1] = a_chunk * carry[c] + local[c]
    out = np.empty_like(E)
    floor = np.power(np.zeros(F) + float(pc.delta), float(pc.r))
    for c in range(n_chunks):
        M = carry[c]
        for t in range(c * chunk, min(T, (c + 1) * chunk)):
            M = M + s * (E[t] - M)
            out[t] = np.power(E[t] / np.power(float(pc.eps) + M, float(pc.alpha)) + float(pc.delta), float(pc.r)) - floor
    return out


def mfcc(wav, n_mfcc: int | None = None, config: FrontendConfig | None = None):
    """wav: CUDA float32 [N, L] -> CUDA float32 [N, T, n_mfcc]: DCT-II (ortho) of the log-mel frames.

    Without a config: T = 1 + L//160 and n_mfcc defaults to 40.  With one: the config's frames, n_mfcc defaults to its
    n_mels, which the DCT kernel limits to 64."""
    import torch
    if config is not None and config.scale in ("power", "pcen"):
        raise ValueError(f"mfcc: the DCT is taken of log-mel (or dB) frames, not of scale {config.scale!r}")
    if config is None:
        n_mels, bound = N_MELS, "1 <= n_mfcc <= 40"
    else:
        n_mels, bound = int(config.n_mels), f"1 <= n_mfcc <= n_mels = {int(config.n_mels)}"
        if n_mels > MFCC_MAX_MELS:
            raise ValueError(f"mfcc: n_mels <= {MFCC_MAX_MELS} (the config has {n_mels})")
    if n_mfcc is None:
        n_mfcc = n_mels
    lm = log_mel(wav, config)
    n, T = int(lm.shape[0]), int(lm.shape[1])
    if not 1 <= n_mfcc <= n_mels:
        raise ValueError(bound)
    out = torch.empty((n, T, n_mfcc), dtype=torch.float32, device=lm.device)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_mfcc(_lib.ptr(lm), C.c_int64(n * T), C.c_int32(n_mels), C.c_int32(n_mfcc), _lib.ptr(out)))
    return out


def standardize_fit(x):
    """StandardScaler.fit over x.reshape(-1, F): (mean, scale) float64 numpy arrays."""
    import torch
    x = x.contiguous()
    cols = int(x.shape[-1])
    rows = int(x.numel() // cols)
    mean, scale = np.zeros(cols, np.float64), np.zeros(cols, np.float64)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_standardize_fit(_lib.ptr(x), C.c_int64(rows), C.c_int32(cols), _lib.ptr(mean), _lib.ptr(scale)))
    return mean, scale


def standardize_apply(x, mean, scale):
    """In place (x - mean) / scale per last-axis column; returns x."""
    import torch
    assert x.is_contiguous()
    cols = int(x.shape[-1])
    rows = int(x.numel() // cols)
    mean = np.ascontiguousarray(mean, np.float64)
    scale = np.ascontiguousarray(scale, np.float64)
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_standardize_apply(_lib.ptr(x), C.c_int64(rows), C.c_int32(cols), _lib.ptr(mean), _lib.ptr(scale)))
    return x


def prepare_dataset(X_train, X_validation, X_test=None, mode="refit"):
    """Standardise the splits in place on the GPU.

    mode 'refit'      -- nsga_penalty.py:111,124,137: the scaler is RE-FIT on val and test (quirk Q1)
    mode 'train_only' -- mobo_penalty.py:69-79 and the ablations: fit on train, transform the rest
    mode 'none'       -- sa_nsga_penalty.py:61-85: no scaling (quirk Q2)
    """
    if mode == "none":
        return X_train, X_validation, X_test
    if mode not in ("refit", "train_only"):
        raise ValueError(mode)
    m, s = standardize_fit(X_train)
    standardize_apply(X_train, m, s)
    for X in (X_validation, X_test):
        if X is None:
            continue
        if mode == "refit":
            m2, s2 = standardize_fit(X)
            standardize_apply(X, m2, s2)
        else:
            standardize_apply(X, m, s)
    return X_train, X_validation, X_test
