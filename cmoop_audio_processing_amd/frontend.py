"""Audio front end + per-bin standardisation on the GPU (libcmoop_hip.so).

The reference loads pre-extracted log-mel features (nsga_penalty.py:64-71,
sa_nsga_penalty.py:58); the north-star adds the extraction beneath that loader:
1 s @ 16 kHz clips -> framing (n_fft 512, Hann 400, hop 160, centre-padded) ->
|STFT|^2 -> 40 Slaney mel bands 20-7600 Hz -> log(mel + 1e-6)  => [N,101,40].
``prepare_dataset`` mirrors nsga_penalty.py:85-155 (StandardScaler per mel bin
over the N*T rows) including the per-script quirks Q1/Q2 of SURVEY §8a.

``FrontendConfig`` names any other geometry the library serves (n_fft 256-2048,
up to 128 mel bands, log or dB scale); ``log_mel`` / ``mfcc`` without a config
are the fixed geometry above, unchanged.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _lib

HOP, N_MELS = 160, 40
MFCC_MAX_MELS = 64      # cmoop_mfcc's DCT kernel holds at most a 64 x 64 basis

SCALE_LOG, SCALE_DB = 0, 1


class FrontendConfigStruct(C.Structure):
    """cmoop_frontend_config (include/cmoop.h)."""
    _fields_ = [(n, C.c_int32) for n in ("sr", "n_fft", "win", "hop", "n_mels", "scale", "db_ref_max")] + \
        [(n, C.c_float) for n in ("fmin", "fmax", "log_eps", "db_amin", "top_db")]


@dataclasses.dataclass(frozen=True)
class FrontendConfig:
    """Geometry and output scale of the front end; mirrors ``cmoop_frontend_config``.

    Domain: n_fft in {256, 512, 1024, 2048}, 1 <= win <= n_fft, hop >= 1, 1 <= n_mels <= 128,
    0 <= fmin < fmax <= sr/2.  ``scale`` is "log" (``log(mel + log_eps)``) or "db"
    (``10 log10(max(db_amin, mel)) - 10 log10(max(db_amin, ref))`` with ref = 1.0, or the clip's own largest mel
    power when ``db_ref_max``; then values more than ``top_db`` below the clip's maximum are raised to that floor,
    ``top_db < 0`` turns the floor off).  The default is the build-defined GSC geometry of ``log_mel(wav)``.
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
        if self.scale not in ("log", "db"):
            raise ValueError("front end config: scale must be 'log' or 'db'")
        return FrontendConfigStruct(int(self.sr), int(self.n_fft), int(self.win), int(self.hop), int(self.n_mels),
                                    SCALE_DB if self.scale == "db" else SCALE_LOG, int(bool(self.db_ref_max)),
                                    float(self.fmin), float(self.fmax), float(self.log_eps), float(self.db_amin),
                                    float(self.top_db))

    def check(self) -> "FrontendConfig":
        """Raise ValueError naming the offending field when the config is outside the domain (host only)."""
        st = self._struct()
        L = _lib.lib()
        if L.cmoop_frontend_check(C.byref(st)) != 0:
            raise ValueError(L.cmoop_last_error().decode("utf-8", "replace"))
        return self

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
                          log_eps=st.log_eps, scale="db" if st.scale == SCALE_DB else "log", db_ref_max=bool(st.db_ref_max),
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
    _lib.check(_lib.lib().cmoop_logmel_ex(C.byref(st), _lib.ptr(wav), C.c_int64(n), C.c_int32(L), _lib.ptr(out)))
    return out


def log_mel(wav, config: FrontendConfig | None = None):
    """wav: CUDA float32 [N, L] -> CUDA float32 [N, 1 + L//160, 40]; with a config, [N, 1 + L//hop, n_mels] in its scale."""
    import torch
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


def log_mel_stream(wav, config: FrontendConfig | None = None):
    """ONE recording, CUDA float32 [L] -> CUDA float32 [1 + L//hop, n_mels], its frames spread over the whole chip.

    Log scale: frame for frame the bits of ``log_mel(wav[None], config)[0]``.  dB scale: the UN-REFERENCED
    ``10 log10(max(db_amin, mel))`` -- the reference and the ``top_db`` floor are quantities of a window, applied by
    ``NetSession.predict_stream`` to each window it cuts from the stream.  ``config=None`` is ``FrontendConfig()``."""
    import torch
    if config is None:
        config = FrontendConfig()
    if not (isinstance(wav, torch.Tensor) and wav.is_cuda and wav.dtype == torch.float32 and wav.dim() == 1):
        raise ValueError("log_mel_stream expects a CUDA float32 tensor [n_samples]")
    wav = wav.contiguous()
    L = int(wav.shape[0])
    if L < 1:
        raise ValueError("log_mel_stream: the recording is empty")
    out = torch.empty((config.frames(L), config.n_mels), dtype=torch.float32, device=wav.device)
    st = config._struct()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_logmel_stream(C.byref(st), _lib.ptr(wav), C.c_int64(L), _lib.ptr(out)))
    return out


def mfcc(wav, n_mfcc: int | None = None, config: FrontendConfig | None = None):
    """wav: CUDA float32 [N, L] -> CUDA float32 [N, T, n_mfcc]: DCT-II (ortho) of the log-mel frames.

    Without a config: T = 1 + L//160 and n_mfcc defaults to 40.  With one: the config's frames, n_mfcc defaults to its
    n_mels, which the DCT kernel limits to 64."""
    import torch
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
