"""CPU: the host-only side of recording scoring -- exported symbols, the window count, posterior smoothing, event
detection and the TrainedModel file format.  No GPU is touched."""
import ctypes as C

import numpy as np
import pytest

from cmoop_audio_processing_amd import FrontendConfig, TrainedModel, _lib, detect_events, genes as G, smooth_posteriors

NEW_SYMBOLS = ["cmoop_net_predict", "cmoop_logmel_stream", "cmoop_logmel_stream_time", "cmoop_stream_windows",
               "cmoop_net_predict_stream"]


def test_new_symbols_are_declared_and_exported_and_the_abi_version_stays():
    L = _lib.lib()
    declared = _lib.declared_symbols()
    for name in NEW_SYMBOLS:
        assert name in declared, name
        assert getattr(L, name) is not None
    assert L.cmoop_abi_version() == 3


def windows(n_frames, T, hop):
    out = C.c_int64(-1)
    rc = _lib.lib().cmoop_stream_windows(C.c_int64(n_frames), C.c_int32(T), C.c_int32(hop), C.byref(out))
    return rc, int(out.value)


@pytest.mark.parametrize("n_frames,T,hop,want", [(68, 21, 3, 16), (21, 21, 7, 1), (68, 21, 1, 48), (68, 21, 25, 2)])
def test_stream_windows(n_frames, T, hop, want):
    assert windows(n_frames, T, hop) == (0, want)
    assert want == len(range(0, n_frames - T + 1, hop))            # every window start i * hop with i * hop + T <= n_frames


@pytest.mark.parametrize("n_frames,T,hop,word", [(20, 21, 1, "20 frames"), (68, 21, 0, "hop_frames")])
def test_stream_windows_rejects(n_frames, T, hop, word):
    rc, _ = windows(n_frames, T, hop)
    assert rc != 0
    msg = _lib.lib().cmoop_last_error().decode()
    assert word in msg, msg
    with pytest.raises(_lib.CmoopError, match=word):
        _lib.check(rc)


P6 = np.array([[0.9, 0.1, 0.0],
               [0.3, 0.6, 0.1],
               [0.0, 0.3, 0.7],
               [0.6, 0.0, 0.4],
               [0.3, 0.3, 0.4],
               [0.0, 0.9, 0.1]])


def test_smooth_posteriors():
    assert np.array_equal(smooth_posteriors(P6, 1), P6)
    s3 = smooth_posteriors(P6.astype(np.float32), 3)
    assert s3.dtype == np.float64 and s3.shape == P6.shape
    want = np.array([[0.9, 0.1, 0.0],
                     [0.6, 0.35, 0.05],
                     [0.4, 1.0 / 3, 0.8 / 3],
                     [0.3, 0.3, 0.4],
                     [0.3, 0.2, 0.5],
                     [0.3, 0.4, 0.3]])
    assert np.abs(s3 - want).max() < 1e-7                          # float32 input, float64 means
    s10 = smooth_posteriors(P6, 10)                                # w > n: the running mean from the start
    assert np.allclose(s10, np.cumsum(P6, axis=0) / np.arange(1, 7)[:, None], rtol=0, atol=1e-15)
    assert np.allclose(s10.sum(axis=1), 1.0)
    with pytest.raises(ValueError):
        smooth_posteriors(P6, 0)


def test_detect_events():
    t = np.arange(8) * 0.25
    p = np.array([[0.8, 0.1, 0.1],     # class 0 is not a keyword
                  [0.2, 0.7, 0.1],     # crossing: class 1 at t = 0.25
                  [0.1, 0.1, 0.8],     # refractory (2 windows): suppressed although class 2 is above the threshold
                  [0.1, 0.8, 0.1],     # refractory: suppressed
                  [0.2, 0.4, 0.4],     # below the threshold
                  [0.2, 0.4, 0.4],
                  [0.0, 0.5, 0.5],     # tie at the threshold: the lowest class id
                  [0.0, 0.1, 0.9]])    # refractory again
    assert detect_events(t, p, 0.5, [2, 1], 2) == [(0.25, 1, 0.7), (1.5, 1, 0.5)]
    # no refractory span: every crossing is its own event
    assert [(e[0], e[1]) for e in detect_events(t, p, 0.5, [1, 2], 0)] == [(0.25, 1), (0.5, 2), (0.75, 1), (1.5, 1), (1.75, 2)]
    assert detect_events(t, p, 0.95, [1, 2], 2) == []              # no event
    assert detect_events(t, p, 0.75, [0], 0) == [(0.0, 0, 0.8)]
    assert detect_events(t[:0], p[:0], 0.5, [1], 3) == []
    with pytest.raises(ValueError):
        detect_events(t, p, 0.5, [3], 0)
    with pytest.raises(ValueError):
        detect_events(t[:3], p, 0.5, [1], 0)


def make_model(gene, variant, classes, **extra):
    n = G.param_count(gene, G.VARIANT_NAMES[variant], classes)
    params = np.random.RandomState(4).randn(n).astype(np.float32)
    return TrainedModel(gene=gene, variant=variant, classes=classes, T=21, F=12, seed=2 ** 31 + 5, params=params,
                        objectives={"acc": 0.8125, "size_mb": G.model_size_mb(gene, G.VARIANT_NAMES[variant], classes),
                                    "fpr": 1.0 / 3, "epochs_run": 7}, **extra)


@pytest.mark.parametrize("with_extras", [False, True])
def test_trained_model_round_trip(tmp_path, with_extras):
    gene, variant, classes = (16, 3, 1, 2, 2, 1), "B", 11
    extra = {}
    if with_extras:
        rs = np.random.RandomState(1)
        extra = dict(frontend=FrontendConfig(sr=22050, n_fft=256, win=200, hop=100, n_mels=12, fmin=50.0, fmax=11025.0, scale="db",
                                             db_ref_max=True, db_amin=1e-9, top_db=60.5, log_eps=3e-7),
                     mean=rs.randn(12), scale=1.0 + rs.rand(12))
    m = make_model(gene, variant, classes, **extra)
    path = tmp_path / "candidate.model"                            # written to exactly this path, no suffix added
    m.save(path)
    assert path.exists()
    r = TrainedModel.load(path)
    assert (r.gene, r.variant, r.classes, r.T, r.F, r.seed) == (gene, variant, classes, 21, 12, 2 ** 31 + 5)
    assert r.params.dtype == np.float32 and np.array_equal(r.params.view(np.uint32), m.params.view(np.uint32))
    assert r.objectives == m.objectives and isinstance(r.objectives["epochs_run"], int)
    if with_extras:
        assert r.frontend == m.frontend
        assert r.mean.dtype == np.float64 and np.array_equal(r.mean, m.mean) and np.array_equal(r.scale, m.scale)
    else:
        assert r.frontend is None and r.mean is None and r.scale is None
    tensors = r.tensors()
    spec = G.param_tensors(gene, G.VARIANT_NAMES[variant], classes)
    assert list(tensors) == [name for name, _, _ in spec]
    assert [tensors[name].shape for name, _, _ in spec] == [tuple(shape) for _, shape, _ in spec]
    assert np.array_equal(np.concatenate([v.reshape(-1) for v in tensors.values()]), m.params)


def test_trained_model_rejects_inconsistent_fields():
    with pytest.raises(ValueError, match="params holds"):
        TrainedModel(gene=(16, 3, 0, 1, 1, 0), variant="A", classes=10, T=21, F=12, seed=0, params=np.zeros(5, np.float32), objectives={})
    m = make_model((16, 3, 0, 1, 1, 0), "A", 10)
    with pytest.raises(ValueError, match="both or neither"):
        TrainedModel(gene=m.gene, variant="A", classes=10, T=21, F=12, seed=0, params=m.params, objectives={}, mean=np.zeros(12))
