"""CPU: the configurable front end's host-only calls (config check, frame count, mel table) and its Python surface.

No GPU is touched: the mel table the general kernel reads is pinned here against oracle/frontend.py."""
import ctypes as C

import numpy as np
import pytest

from cmoop_audio_processing_amd import FrontendConfig, _lib, frontend as fe
from oracle import frontend as ofe

# the geometries of tests/test_gpu_frontend_config.py
GEOMETRIES = {
    "bird128": dict(sr=32000, n_fft=2048, win=2048, hop=512, n_mels=128, fmin=20.0, fmax=16000.0),
    "g1024": dict(sr=16000, n_fft=1024, win=640, hop=320, n_mels=64, fmin=0.0, fmax=8000.0),
    "g256": dict(sr=22050, n_fft=256, win=200, hop=100, n_mels=20, fmin=50.0, fmax=11025.0),
    "g512m80": dict(sr=16000, n_fft=512, win=512, hop=128, n_mels=80, fmin=20.0, fmax=7600.0),
    "empty": dict(sr=16000, n_fft=256, win=256, hop=128, n_mels=128, fmin=0.0, fmax=8000.0),
    "gsc": dict(),
}
SIX = ["bird128", "g1024", "g256", "g512m80", "empty", "gsc"]


def _struct(**kw):
    return FrontendConfig(**kw)._struct()


@pytest.mark.parametrize("name", SIX)
def test_mel_basis_matches_oracle(name):
    """float32 storage of a float64 table: |diff| <= 1e-6 x the largest weight, and the same zero pattern."""
    cfg = FrontendConfig(**GEOMETRIES[name])
    got = cfg.mel_basis()
    ref = ofe.mel_filterbank(cfg.sr, cfg.n_fft, cfg.n_mels, cfg.fmin, cfg.fmax)
    assert got.shape == ref.shape == (cfg.n_mels, 1 + cfg.n_fft // 2) and got.dtype == np.float32
    err = np.abs(got.astype(np.float64) - ref).max()
    print(name, "mel basis max abs diff", err, "largest weight", ref.max())
    assert err <= 1e-6 * ref.max()
    assert np.array_equal(got != 0, ref != 0)
    assert (got != 0).sum() <= 2 * (1 + cfg.n_fft // 2)          # at most two bands per bin


def test_mel_basis_empty_bands_stay_empty():
    """sr 16000, n_fft 256, 128 mels over 0-8000 Hz: 13 of the 128 bands contain no bin, in the oracle and in the table."""
    cfg = FrontendConfig(**GEOMETRIES["empty"])
    got = cfg.mel_basis()
    ref = ofe.mel_filterbank(cfg.sr, cfg.n_fft, cfg.n_mels, cfg.fmin, cfg.fmax)
    empty_ref = np.flatnonzero((ref != 0).sum(axis=1) == 0)
    empty_got = np.flatnonzero((got != 0).sum(axis=1) == 0)
    assert len(empty_ref) == 13
    assert np.array_equal(empty_got, empty_ref)


@pytest.mark.parametrize("name", SIX)
def test_check_accepts_the_test_geometries(name):
    L = _lib.lib()
    for scale, ref_max, top_db in (("log", False, 80.0), ("db", False, -1.0), ("db", True, 80.0)):
        st = _struct(scale=scale, db_ref_max=ref_max, top_db=top_db, **GEOMETRIES[name])
        assert L.cmoop_frontend_check(C.byref(st)) == 0, L.cmoop_last_error()
        FrontendConfig(scale=scale, db_ref_max=ref_max, top_db=top_db, **GEOMETRIES[name]).check()


@pytest.mark.parametrize("field,kw", [
    ("n_fft", dict(n_fft=384, win=384)),
    ("n_fft", dict(n_fft=4096)),
    ("win", dict(win=513)),
    ("hop", dict(hop=0)),
    ("n_mels", dict(n_mels=129)),
    ("fmax", dict(fmax=8000.5)),
    ("fmin", dict(fmin=4000.0, fmax=4000.0)),
    ("fmin", dict(fmin=5000.0, fmax=4000.0)),
])
def test_check_rejects_with_a_message_naming_the_field(field, kw):
    L = _lib.lib()
    st = _struct(**kw)
    assert L.cmoop_frontend_check(C.byref(st)) != 0
    msg = L.cmoop_last_error().decode()
    assert field in msg, msg
    with pytest.raises(ValueError, match=field):
        FrontendConfig(**kw).check()
    # the other host-only calls and the launch refuse the same config before they do anything
    T = C.c_int32(-7)
    assert L.cmoop_frontend_frames(C.byref(st), 16000, C.byref(T)) != 0 and T.value == -7
    assert L.cmoop_logmel_ex(C.byref(st), None, C.c_int64(0), C.c_int32(16000), None) != 0


@pytest.mark.parametrize("name", SIX)
def test_frames(name):
    L = _lib.lib()
    cfg = FrontendConfig(**GEOMETRIES[name])
    st = cfg._struct()
    for n in sorted({1, max(1, cfg.hop - 1), cfg.hop, 65280}):
        T = C.c_int32()
        assert L.cmoop_frontend_frames(C.byref(st), n, C.byref(T)) == 0
        assert T.value == 1 + n // cfg.hop == cfg.frames(n)
    assert L.cmoop_frontend_frames(C.byref(st), 0, C.byref(T)) != 0


def test_presets():
    assert FrontendConfig.preset() == FrontendConfig.preset("gsc") == FrontendConfig()
    # the library's default, read back through float32 fields, is the same struct
    assert bytes(fe.default_frontend_config()._struct()) == bytes(FrontendConfig()._struct())
    bird = FrontendConfig.preset("birdclef_128").check()
    assert (bird.sr, bird.n_fft, bird.win, bird.hop, bird.n_mels, bird.fmin, bird.fmax) == (32000, 2048, 2048, 512, 128, 20.0, 16000.0)
    assert (bird.scale, bird.db_ref_max, bird.top_db) == ("db", True, 80.0)
    assert (bird.frames(65280), bird.n_mels) == (128, 128)
    with pytest.raises(ValueError):
        FrontendConfig.preset("nope")


def test_default_struct_is_todays_geometry():
    L = _lib.lib()
    st = fe.FrontendConfigStruct()
    assert L.cmoop_frontend_config_default(C.byref(st)) == 0
    assert (st.sr, st.n_fft, st.win, st.hop, st.n_mels, st.scale, st.db_ref_max) == (16000, 512, 400, 160, 40, 0, 0)
    assert (st.fmin, st.fmax) == (20.0, 7600.0) and st.log_eps == np.float32(1e-6)
    assert st.db_amin == np.float32(1e-10) and st.top_db == 80.0
    assert C.sizeof(fe.FrontendConfigStruct) == 48
    assert L.cmoop_frontend_config_default(None) != 0


def test_abi_version_and_new_symbols_load():
    L = _lib.lib()
    assert L.cmoop_abi_version() == 3
    names = _lib.declared_symbols()
    for n in ("cmoop_frontend_config_default", "cmoop_frontend_check", "cmoop_frontend_frames", "cmoop_frontend_mel_basis",
              "cmoop_logmel_ex"):
        assert n in names and hasattr(L, n), n
    for n in names:
        assert hasattr(L, n), n


def test_mfcc_refuses_more_than_64_mels_before_touching_the_gpu():
    with pytest.raises(ValueError, match="n_mels <= 64"):
        fe.mfcc(None, 20, FrontendConfig(**GEOMETRIES["g512m80"]))
