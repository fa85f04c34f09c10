"""CPU: the host-only side of PCEN -- exported symbols, the parameter check, the smoothing coefficient, the chunk plan,
the two numpy restatements (closed forms, and the algebra of the carry pass) and the TrainedModel file format.
No GPU is touched."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest

from cmoop_audio_processing_amd import FrontendConfig, PcenConfig, TrainedModel, _lib, frontend as fe, genes as G

NEW_SYMBOLS = ["cmoop_pcen_default", "cmoop_pcen_check", "cmoop_pcen_smoothing", "cmoop_pcen_apply", "cmoop_logmel_pcen",
               "cmoop_pcen_stream_plan", "cmoop_pcen_stream", "cmoop_logmel_pcen_stream", "cmoop_logmel_pcen_stream_time"]


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert getattr(L, name) is not None
        assert name in _lib.PCEN_PROTOTYPES
    assert L.cmoop_abi_version() == 3
    assert C.sizeof(fe.PcenStruct) == 48 and C.sizeof(fe.FrontendConfigStruct) == 48
    import cmoop_audio_processing_amd as pkg
    assert pkg.PcenConfig is fe.PcenConfig and "PcenConfig" in pkg.__all__


def test_default_struct_and_presets():
    st = fe.PcenStruct()
    assert _lib.lib().cmoop_pcen_default(C.byref(st)) == 0
    assert (st.s, st.alpha, st.delta, st.r, st.eps, st.input_scale) == (0.025, 0.98, 2.0, 0.5, 1e-6, 1.0)
    assert fe.default_pcen_config() == PcenConfig() == PcenConfig.preset() == PcenConfig.preset("speech")
    assert _lib.lib().cmoop_pcen_default(None) != 0
    bio = PcenConfig.preset("bioacoustic").check()
    assert (bio.alpha, bio.delta, bio.r, bio.eps, bio.input_scale) == (0.8, 10.0, 0.25, 1e-6, 1.0)
    assert bio.s == PcenConfig.from_time_constant(0.06, 32000, 512).s and abs(bio.s - 0.2335) < 1e-4
    with pytest.raises(ValueError):
        PcenConfig.preset("nope")
    with pytest.raises(dataclasses.FrozenInstanceError):
        PcenConfig().s = 0.5


@pytest.mark.parametrize("field,value", [
    ("s", 0.0), ("s", 1.0000001), ("s", -0.1),
    ("alpha", -1e-9), ("alpha", 1.0000001),
    ("delta", -1e-9), ("delta", math.inf),
    ("r", 0.0), ("r", 1.5),
    ("eps", 0.0), ("eps", -1e-6),
    ("input_scale", 0.0), ("input_scale", -2.0), ("input_scale", math.inf),
] + [(f, math.nan) for f in ("s", "alpha", "delta", "r", "eps", "input_scale")])
def test_check_rejects_with_a_message_naming_the_field(field, value):
    L = _lib.lib()
    cfg = PcenConfig(**{field: value})
    st = cfg._struct()
    assert L.cmoop_pcen_check(C.byref(st)) != 0
    msg = L.cmoop_last_error().decode()
    assert msg.startswith(f"pcen config: {field} "), msg
    with pytest.raises(ValueError, match=f"pcen config: {field} "):
        cfg.check()
    with pytest.raises(ValueError, match=f"pcen config: {field} "):
        FrontendConfig(scale="pcen", pcen=cfg).check()
    # the launches refuse the same struct before they touch the GPU
    assert L.cmoop_pcen_apply(C.byref(st), None, C.c_int64(0), C.c_int32(4), C.c_int32(4)) != 0
    assert f"pcen config: {field} " in L.cmoop_last_error().decode()


def test_check_accepts_the_domain_edges():
    L = _lib.lib()
    for kw in (dict(), dict(s=1.0), dict(s=1e-6), dict(alpha=0.0), dict(alpha=1.0), dict(delta=0.0), dict(r=1.0), dict(r=1e-3),
               dict(eps=1e-30), dict(input_scale=2.0 ** 31), dict(s=0.3, alpha=0.8, delta=10.0, r=0.25)):
        st = PcenConfig(**kw)._struct()
        assert L.cmoop_pcen_check(C.byref(st)) == 0, (kw, L.cmoop_last_error())
        assert PcenConfig(**kw).check() == PcenConfig(**kw)
    assert L.cmoop_pcen_check(None) != 0


def test_frontend_check_accepts_the_power_scale_and_still_rejects_scale_3():
    L = _lib.lib()
    for scale in ("power", "pcen"):
        cfg = FrontendConfig(scale=scale)
        st = cfg._struct()
        assert st.scale == 2
        assert L.cmoop_frontend_check(C.byref(st)) == 0, L.cmoop_last_error()
        assert cfg.check() is cfg and cfg.frames(16000) == 101
    st = FrontendConfig()._struct()
    for bad in (3, -1):
        st.scale = bad
        assert L.cmoop_frontend_check(C.byref(st)) != 0
        assert "scale" in L.cmoop_last_error().decode()
    with pytest.raises(ValueError, match="scale"):
        FrontendConfig(scale="mel")._struct()
    # existing fields keep their order and defaults; the new one comes last and defaults to None
    names = [f.name for f in dataclasses.fields(FrontendConfig)]
    assert names == ["sr", "n_fft", "win", "hop", "n_mels", "fmin", "fmax", "log_eps", "scale", "db_ref_max", "db_amin", "top_db", "pcen"]
    assert FrontendConfig().pcen is None and FrontendConfig().scale == "log"
    assert FrontendConfig(scale="pcen").pcen_config() == PcenConfig()
    # the bytes of the log and dB structs are what they were
    assert bytes(FrontendConfig(pcen=PcenConfig(s=0.5))._struct()) == bytes(FrontendConfig()._struct())


def test_a_pcen_struct_with_another_scale_is_an_error_that_says_so():
    L = _lib.lib()
    pc = PcenConfig()._struct()
    for scale in ("log", "db"):
        st = FrontendConfig(scale=scale)._struct()
        assert L.cmoop_logmel_pcen(C.byref(st), C.byref(pc), None, C.c_int64(0), C.c_int32(16000), None) != 0
        assert "scale 2" in L.cmoop_last_error().decode()
        assert L.cmoop_logmel_pcen_stream(C.byref(st), C.byref(pc), None, C.c_int64(16000), None) != 0
        assert "scale 2" in L.cmoop_last_error().decode()
    st = FrontendConfig(scale="power")._struct()
    assert L.cmoop_logmel_pcen(C.byref(st), None, None, C.c_int64(0), C.c_int32(16000), None) != 0     # NULL PCEN struct


def test_mfcc_refuses_the_power_and_pcen_scales_before_touching_the_gpu():
    for scale in ("power", "pcen"):
        with pytest.raises(ValueError, match="scale"):
            fe.mfcc(None, 20, FrontendConfig(scale=scale))


@pytest.mark.parametrize("tc,sr,hop", [(0.4, 16000, 160), (0.06, 32000, 512), (1.0, 22050, 100), (0.01, 16000, 160), (5.0, 8000, 1)])
def test_smoothing_matches_the_closed_form(tc, sr, hop):
    s = C.c_double()
    assert _lib.lib().cmoop_pcen_smoothing(C.c_double(tc), C.c_int32(sr), C.c_int32(hop), C.byref(s)) == 0
    tf = tc * sr / hop
    want = (math.sqrt(1.0 + 4.0 * tf * tf) - 1.0) / (2.0 * tf * tf)
    assert abs(s.value - want) <= 1e-15 * want
    assert 0.0 < s.value < 1.0
    assert PcenConfig.from_time_constant(tc, sr, hop, alpha=0.5).s == s.value
    assert PcenConfig.from_time_constant(tc, sr, hop, alpha=0.5).alpha == 0.5


def test_smoothing_rejects_bad_input():
    s = C.c_double(-7.0)
    L = _lib.lib()
    for tc, sr, hop in ((0.0, 16000, 160), (math.nan, 16000, 160), (0.4, 0, 160), (0.4, 16000, 0)):
        assert L.cmoop_pcen_smoothing(C.c_double(tc), C.c_int32(sr), C.c_int32(hop), C.byref(s)) != 0
        assert s.value == -7.0
    assert L.cmoop_pcen_smoothing(C.c_double(0.4), C.c_int32(16000), C.c_int32(160), None) != 0
    with pytest.raises(ValueError):
        PcenConfig.from_time_constant(0.0, 16000, 160)
    with pytest.raises(ValueError):
        PcenConfig.from_time_constant(0.4, 16000, 160, s=0.1)


# ---- pcen_reference: closed forms -----------------------------------------------------------------------------------
PARAMS = [dict(), dict(s=0.005), dict(s=0.3, alpha=0.8, delta=10.0, r=0.25), dict(s=1.0, alpha=0.0, delta=0.0, r=1.0),
          dict(input_scale=2.0 ** 10, eps=1e-3)]


def rel(a, b):
    return np.abs(a - b).max() / max(1.0, np.abs(b).max())


@pytest.mark.parametrize("kw", PARAMS)
def test_reference_constant_input_zeros_and_one_frame(kw):
    cfg = PcenConfig(**kw)
    for c in (1e-3, 1.0, 37.5):
        out = fe.pcen_reference(np.full((3, 50, 7), c), cfg)
        e = cfg.input_scale * c
        want = (e / (cfg.eps + e) ** cfg.alpha + cfg.delta) ** cfg.r - cfg.delta ** cfg.r
        assert out.shape == (3, 50, 7) and out.dtype == np.float64
        assert rel(out, np.full_like(out, want)) <= 1e-12                       # M stays at E in every frame
    for dt in (np.float64, np.float32):
        z = fe.pcen_reference(np.zeros((2, 9, 5)), cfg, dt)
        assert z.dtype == dt and np.all(z == 0.0)                               # exactly zero
    P = np.random.RandomState(0).rand(4, 1, 6) + 0.1
    one = fe.pcen_reference(P, cfg)                                             # T = 1: M[0] = E[0]
    e = cfg.input_scale * P
    assert rel(one, (e / (cfg.eps + e) ** cfg.alpha + cfg.delta) ** cfg.r - cfg.delta ** cfg.r) <= 1e-12
    assert fe.pcen_reference(P[0], cfg).shape == (1, 6)                         # [T, F] works as well


def test_reference_s_equal_one_gives_m_equal_e():
    rs = np.random.RandomState(1)
    P = np.exp(3.0 * rs.randn(2, 40, 5))
    cfg = PcenConfig(s=1.0, alpha=0.7, delta=1.5, r=0.4)
    want = (P / (cfg.eps + P) ** cfg.alpha + cfg.delta) ** cfg.r - cfg.delta ** cfg.r
    assert rel(fe.pcen_reference(P, cfg), want) <= 1e-12


def test_reference_float32_is_float32_throughout_and_close_to_float64():
    rs = np.random.RandomState(2)
    P = np.exp(2.0 * rs.randn(2, 101, 40)).astype(np.float32)
    for kw in PARAMS[:3]:
        o32, o64 = fe.pcen_reference(P, PcenConfig(**kw), np.float32), fe.pcen_reference(P, PcenConfig(**kw))
        assert o32.dtype == np.float32 and o64.dtype == np.float64
        err = (np.abs(o32 - o64) / (1.0 + np.abs(o64))).max()
        print(kw, "float32 restatement against float64:", err)
        assert 0.0 < err <= 2e-6


def test_reference_clips_are_independent_and_the_state_matters():
    P = np.full((2, 60, 3), 1e-3)
    P[:, :10] = 1e3
    cfg = PcenConfig(s=0.005)
    both = fe.pcen_reference(P, cfg)
    assert np.array_equal(both[0], fe.pcen_reference(P[0], cfg))
    # after the burst the smoother still holds it: the floor frames differ from a clip that never saw the burst
    quiet = fe.pcen_reference(np.full((60, 3), 1e-3), cfg)
    assert np.all(both[0, 10:] < 0.05 * quiet[10:])


# ---- pcen_scan_reference: the algebra of the carry pass ------------------------------------------------------------
def burst_then_floor(T, F, seed):
    P = np.full((T, F), 1e-3)
    P[:10] = 1e3
    return P * np.exp(np.random.RandomState(seed).randn(T, F))


@pytest.mark.parametrize("T", [1, 2, 257, 775])
@pytest.mark.parametrize("kw", PARAMS[:3] + [dict(s=0.005, delta=0.0), dict(s=0.04, alpha=1.0, delta=0.0, r=1.0)])
def test_scan_reference_agrees_with_the_serial_reference(T, kw):
    """1e-12 relative.  With delta = 0 the output is (E / (eps + M)^alpha)^r, whose relative error is r alpha times M's:
    there the bound is taken element by element and is a bound on the carried state itself.  With delta > 0 the output
    is a difference of two nearly equal powers wherever E << M, so its own rounding (1e-16 absolute) is a large
    fraction of a value of 1e-7; there the bound is relative to 1 + |value|."""
    cfg = PcenConfig(**kw)
    P = burst_then_floor(T, 5, T)
    want = fe.pcen_reference(P, cfg)
    for chunk in sorted({1, 64, max(1, T - 1), T, T + 1}):
        got = fe.pcen_scan_reference(P, cfg, chunk)
        err = (np.abs(got - want) / (np.abs(want) if cfg.delta == 0.0 else 1.0 + np.abs(want))).max()
        print(f"T {T} chunk {chunk} {kw}: scan against serial, max relative difference {err:.2e}")
        assert got.shape == want.shape and err <= 1e-12
    with pytest.raises(ValueError):
        fe.pcen_scan_reference(P, cfg, 0)


def test_scan_reference_would_see_a_wrong_carry():
    """The inputs make the carry matter: dropping it (every chunk restarted from its own first frame) is off by far more
    than any gate used on the device."""
    cfg = PcenConfig(s=0.005)
    P = burst_then_floor(257, 5, 3)
    want = fe.pcen_reference(P, cfg)
    restarted = np.concatenate([fe.pcen_reference(P[c:c + 64], cfg) for c in range(0, 257, 64)])
    assert (np.abs(restarted - want) / (1.0 + np.abs(want))).max() > 0.1
    assert 0.27 < (1 - 0.005) ** 256 < 0.29


# ---- the chunk plan -----------------------------------------------------------------------------------------------
def plan(T):
    chunk, n = C.c_int32(-1), C.c_int32(-1)
    rc = _lib.lib().cmoop_pcen_stream_plan(C.c_int64(T), C.byref(chunk), C.byref(n))
    return rc, chunk.value, n.value


def test_stream_plan():
    last = 0
    for T in (1, 63, 64, 65, 4096, 10 ** 4, 60001, 65536, 65537, 10 ** 7, 2 ** 31 - 1):
        rc, chunk, n = plan(T)
        assert rc == 0
        assert chunk >= 64 and chunk % 64 == 0
        assert n == -(-T // chunk) and (n - 1) * chunk < T <= n * chunk        # the chunks cover [0, T) with no empty one
        assert chunk >= last                                                    # monotone in T
        assert (4 * chunk) ** 2 >= T and (n - 1) ** 2 <= 16 * T                 # the carry pass walks at most 4 sqrt(T) chunks
        assert (4 * (chunk - 64)) ** 2 < T or chunk == 64                       # and a chunk is no longer than sqrt(T) / 4 + 64
        last = chunk
        assert fe.pcen_stream_plan(T) == (chunk, n)
    assert [plan(T)[1:] for T in (1, 63, 64, 65)] == [(64, 1), (64, 1), (64, 1), (64, 2)]
    assert plan(10 ** 4)[1:] == (64, 157) and plan(60001)[1:] == (64, 938) and plan(65537)[1:] == (128, 513)
    assert plan(10 ** 7)[1:] == (832, 12020)
    assert plan(0)[0] != 0 and plan(-5)[0] != 0 and plan(2 ** 31)[0] != 0
    assert _lib.lib().cmoop_pcen_stream_plan(C.c_int64(100), None, None) == 0


# ---- TrainedModel file format -------------------------------------------------------------------------------------
GENE, VARIANT, CLASSES = (16, 3, 1, 2, 2, 1), "B", 11
G256 = dict(sr=22050, n_fft=256, win=200, hop=100, n_mels=12, fmin=50.0, fmax=11025.0)
OLD_KEYS = {"gene", "meta", "params", "objectives"}


def make_model(**extra):
    n = G.param_count(GENE, G.VARIANT_NAMES[VARIANT], CLASSES)
    params = np.random.RandomState(4).randn(n).astype(np.float32)
    return TrainedModel(gene=GENE, variant=VARIANT, classes=CLASSES, T=21, F=12, seed=7, params=params,
                        objectives={"acc": 0.5, "size_mb": G.model_size_mb(GENE, G.VARIANT_NAMES[VARIANT], CLASSES), "fpr": 0.25,
                                    "epochs_run": 3}, **extra)


def keys_of(path):
    with np.load(path, allow_pickle=False) as z:
        return set(z.files)


def test_trained_model_round_trips_a_pcen_front_end_field_for_field(tmp_path):
    pc = PcenConfig(s=0.04321, alpha=0.8125, delta=9.75, r=0.3, eps=3e-7, input_scale=2.0 ** 20)
    fcfg = FrontendConfig(scale="pcen", pcen=pc, log_eps=3e-7, db_amin=1e-9, top_db=60.5, **G256)
    m = make_model(frontend=fcfg)
    m.save(tmp_path / "p.npz")
    r = TrainedModel.load(tmp_path / "p.npz")
    assert r.frontend == fcfg and r.frontend.pcen == pc and r.frontend.scale == "pcen"
    for f in dataclasses.fields(PcenConfig):
        assert getattr(r.frontend.pcen, f.name) == getattr(pc, f.name), f.name
    assert keys_of(tmp_path / "p.npz") == OLD_KEYS | {"frontend_int", "frontend_float", "frontend_scale", "frontend_pcen"}
    # pcen=None (the library default) and the power scale round-trip too, each with the keys it needs and no more
    for name, cfg, extra in (("d", FrontendConfig(scale="pcen", **G256), {"frontend_scale"}),
                             ("w", FrontendConfig(scale="power", **G256), {"frontend_scale"})):
        make_model(frontend=cfg).save(tmp_path / name)
        back = TrainedModel.load(tmp_path / name)
        assert back.frontend == cfg and back.frontend.pcen is None
        assert keys_of(tmp_path / name) == OLD_KEYS | {"frontend_int", "frontend_float"} | extra


def test_trained_model_log_and_db_files_are_what_they_were(tmp_path):
    make_model().save(tmp_path / "none")
    assert keys_of(tmp_path / "none") == OLD_KEYS
    assert TrainedModel.load(tmp_path / "none").frontend is None
    for scale in ("log", "db"):
        cfg = FrontendConfig(scale=scale, db_ref_max=True, db_amin=1e-9, top_db=60.5, log_eps=3e-7, **G256)
        m = make_model(frontend=cfg, mean=np.arange(12.0), scale=1.0 + np.arange(12.0))
        m.save(tmp_path / scale)
        assert keys_of(tmp_path / scale) == OLD_KEYS | {"frontend_int", "frontend_float", "mean", "scale"}
        with np.load(tmp_path / scale) as z:
            assert [int(v) for v in z["frontend_int"]] == [22050, 256, 200, 100, 12, int(scale == "db"), 1]
        r = TrainedModel.load(tmp_path / scale)
        assert r.frontend == cfg and r.frontend.pcen is None
        assert np.array_equal(r.params, m.params) and np.array_equal(r.mean, m.mean) and r.objectives == m.objectives
