"""GPU: the configurable front end (cmoop_logmel_ex / FrontendConfig) against oracle/frontend.py in float64.

Inputs follow test_frontend_logmel_and_standardize: a per-clip sinusoid plus 0.3 sigma noise, clip 0 scaled by 0.01.
Gates: 2e-4 absolute on the log scale (the gate the 512-point kernel is held to; a float32 restatement on the CPU stays
at or below 7.3e-6 on these inputs) and 2 x (10 / ln 10) x 2e-4 = 1.74e-3 dB on the dB scale (the log gate carried
through 10 log10, once for the value and once for the clip maximum).

The flat gates are for those broadband inputs only: the noise floor fills every band, so one number fits all of them.  The
structured signals of tests/_frontend_reference.py (tones, impulses, DC, the Nyquist alternation, very quiet, very loud,
silence) leave bands nearly empty, where the float32 error is comparable to log_eps; test_structured_signals holds the
general kernel to that module's derived per-element budget instead (by on the log scale, B on the power scale)."""
import functools

import numpy as np
import pytest
import torch

import _frontend_reference as R
from cmoop_audio_processing_amd import EvalConfig, FrontendConfig, PopulationEvaluator, frontend as fe, genes as G
from oracle import frontend as ofe

pytestmark = pytest.mark.gpu

LOG_GATE = 2e-4
DB_GATE = 2 * (10 / np.log(10)) * 2e-4

GEOMETRIES = {
    "bird128": (dict(sr=32000, n_fft=2048, win=2048, hop=512, n_mels=128, fmin=20.0, fmax=16000.0), 65280),
    "g1024": (dict(sr=16000, n_fft=1024, win=640, hop=320, n_mels=64, fmin=0.0, fmax=8000.0), 6400),
    "g256": (dict(sr=22050, n_fft=256, win=200, hop=100, n_mels=20, fmin=50.0, fmax=11025.0), 8820),
    "g512m80": (dict(sr=16000, n_fft=512, win=512, hop=128, n_mels=80, fmin=20.0, fmax=7600.0), 6400),
    "empty": (dict(sr=16000, n_fft=256, win=256, hop=128, n_mels=128, fmin=0.0, fmax=8000.0), 4000),
    "gsc": (dict(sr=16000, n_fft=512, win=400, hop=160, n_mels=40, fmin=20.0, fmax=7600.0), 6400),
}


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()          # a copy: the cached inputs stay read-only


def okw(geo):
    """FrontendConfig field names -> oracle.frontend.log_mel keyword names."""
    kw = dict(geo)
    kw["win_length"] = kw.pop("win")
    return kw


def make_wav(sr, L, n=4, seed=3):
    rs = np.random.RandomState(seed)
    t = np.arange(L) / float(sr)
    wav = np.stack([0.5 * np.sin(2 * np.pi * (200 + 300 * i) * t) + 0.3 * rs.randn(L) for i in range(n)]).astype(np.float32)
    wav[0, :] *= 0.01
    return wav


@functools.lru_cache(maxsize=None)
def case(name, n=4):
    """(geometry, wav, float64 mel power [n, T, n_mels]) -- computed once per geometry, never modified."""
    geo, L = GEOMETRIES[name]
    wav = make_wav(geo["sr"], L, n)
    wav.setflags(write=False)
    S = mel_power(wav, geo)
    S.setflags(write=False)
    return geo, wav, S


def mel_power(wav, geo):
    """float64 restatement from the oracle's window and mel basis and np.fft.rfft."""
    w64 = np.asarray(wav, np.float64)
    n_fft, hop = geo["n_fft"], geo["hop"]
    T = 1 + w64.shape[1] // hop
    x = np.pad(w64, ((0, 0), (n_fft // 2, n_fft // 2)))
    win = ofe.hann_padded(geo["win"], n_fft)
    fb = ofe.mel_filterbank(geo["sr"], n_fft, geo["n_mels"], geo["fmin"], geo["fmax"])
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    return np.stack([(np.abs(np.fft.rfft(x[i][idx] * win[None, :], axis=1)) ** 2) @ fb.T for i in range(len(w64))])


def db_reference(S, amin, ref_max, top_db):
    raw = 10.0 * np.log10(np.maximum(amin, S))
    ref = S.max(axis=(1, 2), keepdims=True) if ref_max else 1.0
    out = raw - 10.0 * np.log10(np.maximum(amin, ref))
    if top_db >= 0:
        out = np.maximum(out, out.max(axis=(1, 2), keepdims=True) - top_db)
    return out


@pytest.mark.parametrize("name", list(GEOMETRIES))
def test_log_parity(name):
    geo, wav, S = case(name)
    cfg = FrontendConfig(**geo)
    out = fe.log_mel(dev(wav), cfg).cpu().numpy()
    ref = ofe.log_mel(wav, eps=cfg.log_eps, **okw(geo))
    assert out.shape == ref.shape == (4, cfg.frames(wav.shape[1]), cfg.n_mels)
    assert np.abs(ref - np.log(S + cfg.log_eps)).max() < 1e-9        # the restatement used for the dB cases is the oracle's
    err = np.abs(out - ref).max()
    print(f"{name}: log-mel max abs err {err:.3e}")
    assert err < LOG_GATE
    if name == "empty":                                               # 13 bands hold no bin: log(eps) in every frame
        fb = ofe.mel_filterbank(geo["sr"], geo["n_fft"], geo["n_mels"], geo["fmin"], geo["fmax"])
        empty = np.flatnonzero((fb != 0).sum(axis=1) == 0)
        assert len(empty) == 13
        assert np.abs(out[:, :, empty] - np.log(cfg.log_eps)).max() < 1e-5


@pytest.mark.parametrize("ref_max,top_db", [(False, -1.0), (True, 80.0)])
@pytest.mark.parametrize("name", ["bird128", "g1024", "g256"])
def test_db_parity(name, ref_max, top_db):
    geo, wav, S = case(name)
    cfg = FrontendConfig(scale="db", db_ref_max=ref_max, top_db=top_db, **geo)
    wav0 = np.concatenate([wav, np.zeros_like(wav[:1])])             # an all-zero clip rides along
    S0 = np.concatenate([S, np.zeros_like(S[:1])])
    out = fe.log_mel(dev(wav0), cfg).cpu().numpy()
    ref = db_reference(S0, cfg.db_amin, ref_max, top_db)
    err = np.abs(out - ref).max()
    print(f"{name} ref_max={ref_max} top_db={top_db}: dB max abs err {err:.3e}")
    assert err < DB_GATE
    if ref_max:
        assert np.all(out[-1] == 0.0)                                 # silence: exactly 0 dB everywhere
        assert np.all(out.reshape(5, -1).max(axis=1) == 0.0) and out.min() >= -top_db
    else:
        assert np.abs(out[-1] - 10.0 * np.log10(cfg.db_amin)).max() < DB_GATE   # silence sits on the amin floor


@pytest.mark.parametrize("name", ["bird128", "g256"])
def test_edges(name):
    geo, _ = GEOMETRIES[name]
    cfg = FrontendConfig(**geo)
    hop, n_fft = geo["hop"], geo["n_fft"]
    odd = {"bird128": 3001, "g256": 1003}[name]
    assert odd % 2 == 1 and odd % 4 != 0
    for L in (1, hop - 1, hop, n_fft // 2 + 1, odd):
        wav = make_wav(geo["sr"], L, n=3, seed=11 + L % 7)
        out = fe.log_mel(dev(wav), cfg).cpu().numpy()
        ref = ofe.log_mel(wav, eps=cfg.log_eps, **okw(geo))
        assert out.shape == ref.shape == (3, 1 + L // hop, geo["n_mels"])
        err = np.abs(out - ref).max()
        print(f"{name} L={L}: log-mel max abs err {err:.3e}")
        assert err < LOG_GATE
    for c in (cfg, FrontendConfig(scale="db", db_ref_max=True, **geo)):
        empty = fe.log_mel(torch.zeros((0, 5000), dtype=torch.float32, device="cuda"), c)
        assert tuple(empty.shape) == (0, 1 + 5000 // hop, geo["n_mels"])
    silent = fe.log_mel(torch.zeros((2, 4 * hop + 3), dtype=torch.float32, device="cuda"), cfg).cpu().numpy()
    assert silent.shape == (2, 5, geo["n_mels"])
    assert np.abs(silent - np.log(cfg.log_eps)).max() < 1e-5


# elements with rho >= 0.5 (far bands of DC and of the Nyquist alternation at n_fft 1024), held to R.excused_window instead of by
STRUCTURED_EXCUSED = {"g256": 0, "g1024": 34, "bird128": 0, "g512m80": 0}


@pytest.mark.parametrize("name", list(STRUCTURED_EXCUSED))
def test_structured_signals(name):
    """The 13 structured clips at the geometry's own rate, 3 hops + 3 samples long (bird128: 2 hops + 1): log scale within by,
    power scale within B, elementwise."""
    geo, _ = GEOMETRIES[name]
    L = 2 * geo["hop"] + 1 if name == "bird128" else 3 * geo["hop"] + 3
    names, wav, ref, bud = R.case(geo, L)
    B, rho, _ = bud
    assert int((rho >= 0.5).sum()) == STRUCTURED_EXCUSED[name]
    out = fe.log_mel(dev(wav), FrontendConfig(**geo)).cpu().numpy()
    assert out.shape == (13, 1 + L // geo["hop"], geo["n_mels"]) and np.isfinite(out).all()
    R.assert_log_within(f"{name} general kernel", out, ref, bud, names, excusable=STRUCTURED_EXCUSED[name] > 0)
    power = fe.log_mel(dev(wav), FrontendConfig(scale="power", **geo)).cpu().numpy()
    err = np.abs(power.astype(np.float64) - ref["S"])
    ratios = R.worst_ratios(err, B, names)
    R.record(f"{name} general kernel, power: worst |S_gpu - S| / B {max(ratios.values()):.3f}  " +
          " ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert np.all(err <= B)


def test_default_config_is_bit_equal_to_the_fixed_call():
    wav = dev(make_wav(16000, 16000, n=4))
    assert torch.equal(fe.log_mel(wav), fe.log_mel(wav, FrontendConfig()))
    assert torch.equal(fe.log_mel(wav), fe.log_mel(wav, FrontendConfig.preset("gsc")))
    assert torch.equal(fe.mfcc(wav), fe.mfcc(wav, config=FrontendConfig()))
    assert torch.equal(fe.mfcc(wav, 13), fe.mfcc(wav, 13, FrontendConfig()))
    with pytest.raises(ValueError, match="1 <= n_mfcc <= 40"):
        fe.mfcc(wav, 41)


@pytest.mark.parametrize("name,scale", [("bird128", "log"), ("bird128", "db"), ("g512m80", "log")])
def test_deterministic_and_batch_independent(name, scale):
    geo, wav, _ = case(name, 5)
    cfg = FrontendConfig(scale=scale, db_ref_max=True, **geo)
    d = dev(wav)
    a, b = fe.log_mel(d, cfg), fe.log_mel(d, cfg)
    assert torch.equal(a, b)
    for i in range(5):
        assert torch.equal(fe.log_mel(d[i:i + 1].contiguous(), cfg)[0], a[i]), i


def test_mfcc_with_a_config():
    """End to end the log-mel gate passes through an orthonormal DCT over 64 bands: |err| <= 2e-4 * sqrt(64)."""
    geo, wav, _ = case("g1024")
    cfg = FrontendConfig(**geo)
    out = fe.mfcc(dev(wav), 20, cfg).cpu().numpy()
    ref = ofe.mfcc(wav, 20, eps=cfg.log_eps, **okw(geo))
    assert out.shape == ref.shape == (4, 21, 20)
    err = np.abs(out - ref).max()
    print(f"g1024 mfcc max abs err {err:.3e}")
    assert err < 2e-4 * np.sqrt(64.0)
    assert tuple(fe.mfcc(dev(wav), config=cfg).shape) == (4, 21, 64)
    with pytest.raises(ValueError):
        fe.mfcc(dev(wav), 65, cfg)
    bird, bwav, _ = case("bird128")
    with pytest.raises(ValueError, match="n_mels <= 64"):
        fe.mfcc(dev(bwav), 20, FrontendConfig(**bird))


def test_end_to_end_birdclef_preset_feeds_the_evaluator():
    classes, n, L = 11, 96, 65280
    cfg = FrontendConfig.preset("birdclef_128")
    rs = np.random.RandomState(5)
    y = (np.arange(n) % classes).astype(np.int32)
    t = np.arange(L) / float(cfg.sr)
    wav = np.stack([0.5 * np.sin(2 * np.pi * (400.0 + 900.0 * c) * t) + 0.1 * rs.randn(L) for c in y]).astype(np.float32)
    feats = fe.log_mel(dev(wav), cfg)
    assert tuple(feats.shape) == (n, 128, 128)
    assert bool(torch.isfinite(feats).all()) and float(feats.max()) == 0.0 and float(feats.min()) >= -80.0
    Xtr, Xva, _ = fe.prepare_dataset(feats[:64].contiguous(), feats[64:].contiguous(), None, mode="none")
    gene = (16, 3, 0, 1, 1, 0)
    ecfg = EvalConfig.preset("sa_nsga_penalty", classes=classes, epochs=1, batch=16, eval_batch=16, n_slots=1, seed=42)
    ev = PopulationEvaluator(Xtr, y[:64], Xva, y[64:], ecfg)
    res = ev.compute_objectives_and_constraints([G.gene_to_hparams(gene)])
    objs = np.asarray(res[0]["objs"], np.float64)
    print("objectives", objs)
    assert np.all(np.isfinite(objs))
    assert res[0]["objs"][1] == G.model_size_mb(gene, 1, classes)
