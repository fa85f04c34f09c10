"""GPU: scoring recordings -- Model.predict probabilities, the chip-wide stream front end, sliding-window prediction,
and the path from a search result to a StreamScorer.

Gates.  predict_proba against the float64 oracle run from the GPU's own float32 weights: 1e-5 absolute per probability
(the "inference from identical weights" loss gate of test_init_step_grads_and_eval_parity, 1e-5 relative on a loss of
about 2.3, carried to probabilities; the oracle's own float32 path stays at or below 3.6e-8 of its float64 path on these
cases) and |row sum - 1| <= 1e-6 (the float32 oracle: 1.6e-7).  Everything else here is bit equality: predict_stream
against predict_proba on hand-cut windows at the same eval_batch, log_mel_stream against the clip call."""
import functools

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import (EvalConfig, FrontendConfig, PopulationEvaluator, StreamScorer, TrainedModel, _lib,
                                        frontend as fe, genes as G, log_mel_stream)
from cmoop_audio_processing_amd.session import NetSession
from oracle import frontend as ofe
from oracle import net as ON
from test_gpu_frontend_config import GEOMETRIES, LOG_GATE, make_wav, okw
from test_gpu_net import make_data, make_split, ocfg

pytestmark = pytest.mark.gpu

T, F = 21, 12
PROB_GATE, ROWSUM_GATE = 1e-5, 1e-6


def dev(a):
    return torch.tensor(np.ascontiguousarray(a)).cuda()


# ---- 1. predict_proba against the float64 oracle ------------------------------------------------------------------
PROBA_CASES = [
    ((16, 3, 1, 2, 2, 1), "B", 10),
    ((32, 5, 1, 1, 4, 0), "A", 10),
    ((16, 5, 0, 3, 1, 1), "A", 35),
    ((16, 3, 1, 1, 1, 0), "B", 2),
]


@pytest.mark.parametrize("gene,variant,classes", PROBA_CASES)
def test_predict_proba_against_the_float64_oracle(gene, variant, classes):
    seed, B = 1234, 24
    cfg = EvalConfig(variant=variant, classes=classes, batch=32, eval_batch=16)
    X, y = make_data(80, T, F, classes, 1)
    Xd, yd = dev(X), dev(y)
    idxd = dev(np.random.RandomState(2).permutation(80).astype(np.int32))
    with NetSession(gene, cfg, T, F, seed) as net:
        for s in range(5):                                           # moving statistics leave their initial values
            net.train_step(Xd, yd, idxd, row0=4 + s * 8, B=B)
        o64 = ON.OracleNet(gene, ocfg(cfg), seed, dtype=torch.float64)
        o64.set_flat(net.get_params())
        with torch.no_grad():
            p64 = o64.forward(torch.from_numpy(X).to(torch.float64), False).numpy()
        _, _, preds = net.evaluate(Xd, yd)
        preds = preds.cpu().numpy()
        for n in (80, 37, 1):                                        # full chunks, a partial chunk, a single row
            p = net.predict_proba(Xd[:n].contiguous())
            assert tuple(p.shape) == (n, classes) and p.dtype == torch.float32 and p.is_cuda
            p = p.cpu().numpy()
            err = np.abs(p.astype(np.float64) - p64[:n]).max()
            rs = np.abs(p.astype(np.float64).sum(axis=1) - 1.0).max()
            print(f"{variant}{gene} classes {classes} n {n}: max |p - p64| {err:.3e}, max |row sum - 1| {rs:.3e}")
            assert err <= PROB_GATE
            assert rs <= ROWSUM_GATE
            assert np.array_equal(p[np.arange(n), preds[:n]], p.max(axis=1))     # evaluate's prediction holds the maximum
        assert tuple(net.predict_proba(Xd[:0].contiguous()).shape) == (0, classes)
        with pytest.raises(ValueError, match="the net reads"):
            net.predict_proba(Xd[:, :, :8].contiguous())


# ---- 2. predict_stream against predict_proba on hand-cut windows, bit for bit ---------------------------------------
STREAM_GENE, STREAM_VARIANT, STREAM_CLASSES = (16, 3, 1, 1, 2, 1), "A", 10
DB_COMBOS = [(False, 80.0), (False, -1.0), (True, 80.0), (True, -1.0)]


@functools.lru_cache(maxsize=None)
def stream_features(n_frames):
    """(plain stream, dB-like stream, scaler mean, scaler scale) -- read-only."""
    rs = np.random.RandomState(7)
    plain = rs.randn(n_frames, F).astype(np.float32)
    db = (20.0 * rs.randn(n_frames, F)).astype(np.float32)            # tens of dB of range: the 80 dB floor bites
    mean, scale = rs.randn(F), 0.5 + rs.rand(F)
    for a in (plain, db, mean, scale):
        a.setflags(write=False)
    return plain, db, mean, scale


def window_db_tail(w, ref_max, top_db):
    """Step (a) on one window in float32: subtract and maximum only (db_amin <= 1: the fixed reference is 0 dB)."""
    cmax = w.max()
    ref = cmax if ref_max else np.float32(0.0)
    floor = (cmax - ref) - np.float32(top_db) if top_db >= 0 else np.float32(-np.inf)
    out = np.maximum(w - ref, floor)
    assert out.dtype == np.float32
    return out, bool((w - ref < floor).any())


@pytest.mark.parametrize("n_frames,hop,eval_batch", [(68, 3, 16), (68, 3, 5), (68, 1, 16), (68, 25, 16), (21, 7, 16)],
                         ids=["one-chunk", "partial-last-chunk", "hop1-48-windows", "gap-between-windows", "one-window"])
def test_predict_stream_equals_predict_proba_on_hand_cut_windows(n_frames, hop, eval_batch):
    plain, dbs, mean, scale = stream_features(n_frames)
    cfg = EvalConfig(variant=STREAM_VARIANT, classes=STREAM_CLASSES, batch=16, eval_batch=eval_batch)
    n_windows = 1 + (n_frames - T) // hop
    assert n_windows == {(68, 3): 16, (68, 1): 48, (68, 25): 2, (21, 7): 1}[(n_frames, hop)]
    floor_bit = False
    with NetSession(STREAM_GENE, cfg, T, F, 99) as net:
        combos = [(None, False), (None, True)] + [(c, s) for c in DB_COMBOS for s in (False, True)]
        seen = []
        for db, use_scaler in combos:
            host = dbs if db is not None else plain
            feat = dev(host)
            fcfg = None
            wins = np.stack([host[i * hop:i * hop + T] for i in range(n_windows)])
            if db is not None:
                fcfg = FrontendConfig(n_mels=F, scale="db", db_ref_max=db[0], top_db=db[1], db_amin=1e-10)
                tails = [window_db_tail(w, *db) for w in wins]
                wins = np.stack([t[0] for t in tails])
                floor_bit |= any(t[1] for t in tails)
            Xw = dev(wins)
            if use_scaler:
                fe.standardize_apply(Xw, mean, scale)
            want = net.predict_proba(Xw).cpu().numpy()
            got = net.predict_stream(feat, hop, frontend_config=fcfg, mean=mean if use_scaler else None,
                                     scale=scale if use_scaler else None)
            assert tuple(got.shape) == (n_windows, STREAM_CLASSES)
            got = got.cpu().numpy()
            assert np.array_equal(got, want), (db, use_scaler, np.abs(got - want).max())
            assert np.array_equal(feat.cpu().numpy(), host)          # the stream is only read
            seen.append(want)
        # the combinations are different computations: the equalities above are not trivially satisfied
        assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[2], seen[6])
        # a log-scale config asks for no dB tail
        assert torch.equal(net.predict_stream(dev(plain), hop, frontend_config=FrontendConfig(n_mels=F)), net.predict_stream(dev(plain), hop))
    if n_frames == 68:
        assert floor_bit                                             # the 80 dB floor was active in some window


def test_predict_stream_rejects_bad_input():
    cfg = EvalConfig(variant=STREAM_VARIANT, classes=STREAM_CLASSES, batch=16, eval_batch=16)
    plain, _, mean, scale = stream_features(68)
    with NetSession(STREAM_GENE, cfg, T, F, 99) as net:
        with pytest.raises(_lib.CmoopError, match="20 frames"):
            net.predict_stream(dev(plain[:20]), 1)
        with pytest.raises(_lib.CmoopError, match="hop_frames"):
            net.predict_stream(dev(plain), 0)
        with pytest.raises(ValueError, match="features per frame"):
            net.predict_stream(dev(plain[:, :8]), 3)
        with pytest.raises(ValueError, match="both or neither"):
            net.predict_stream(dev(plain), 3, mean=mean)
        with pytest.raises(ValueError, match="both or neither"):
            net.predict_stream(dev(plain), 3, scale=scale)
        with pytest.raises(_lib.CmoopError, match="mel bands"):
            net.predict_stream(dev(plain), 3, frontend_config=FrontendConfig(n_mels=40, scale="db"))


# ---- 3. log_mel_stream against the clip call ------------------------------------------------------------------------
STREAM_FE_CASES = [
    ("bird128", 65280, 128), ("bird128", 70001, 137), ("g1024", 6400 + 37, 21), ("g256", 8820, 89), ("g512m80", 6400, 51),
    ("bird128", 100, 1), ("bird128", 1, 1), ("g256", 100, 2), ("g256", 1, 1),
]


@pytest.mark.parametrize("name,L,frames", STREAM_FE_CASES)
def test_log_mel_stream_equals_the_clip_call_on_the_general_kernel(name, L, frames):
    geo, _ = GEOMETRIES[name]
    wav = dev(make_wav(geo["sr"], L, n=2)[1])
    cfg = FrontendConfig(**geo)
    out = log_mel_stream(wav, cfg)
    assert tuple(out.shape) == (frames, geo["n_mels"]) == (cfg.frames(L), cfg.n_mels)
    assert torch.equal(out, fe.log_mel(wav[None], cfg)[0])
    assert torch.equal(out, log_mel_stream(wav, cfg))                # deterministic
    # dB scale: the un-referenced value = the clip call with a fixed reference of 1.0 and no floor (its tail is the identity)
    raw = log_mel_stream(wav, FrontendConfig(scale="db", db_ref_max=True, top_db=80.0, **geo))
    assert torch.equal(raw, fe.log_mel(wav[None], FrontendConfig(scale="db", db_ref_max=False, top_db=-1.0, **geo))[0])
    assert bool(torch.isfinite(raw).all())


def test_log_mel_stream_on_the_fixed_kernel_config():
    """n_fft 512 / 40 mels / log scale runs the 512-point kernel's own stream variant: bit equality with the clip call
    and with the fixed-geometry call; 301 frames are neither a multiple of the four waves nor of a frames-per-workgroup run."""
    geo, _ = GEOMETRIES["gsc"]
    L = 48077
    host = make_wav(geo["sr"], L, n=2)[1]
    wav = dev(host)
    out = log_mel_stream(wav)                                        # config=None: FrontendConfig()
    assert tuple(out.shape) == (301, 40)
    assert torch.equal(out, fe.log_mel(wav[None], FrontendConfig(**geo))[0])
    assert torch.equal(out, fe.log_mel(wav[None])[0])
    ref = ofe.log_mel(host[None], eps=FrontendConfig().log_eps, **okw(geo))[0]
    err = np.abs(out.cpu().numpy() - ref).max()
    print(f"gsc stream, 301 frames: log-mel max abs err against float64 {err:.3e}")
    assert err < LOG_GATE


def test_log_mel_stream_covers_every_frame_of_a_long_recording():
    """60 s at 16 kHz (6 001 frames, hundreds of workgroups, a partial last run): every frame equals the clip call's."""
    rs = np.random.RandomState(1)
    wav = dev((0.3 * rs.randn(960000)).astype(np.float32))
    for cfg in (FrontendConfig(), FrontendConfig(**GEOMETRIES["g512m80"][0])):
        out = log_mel_stream(wav, cfg)
        assert int(out.shape[0]) == cfg.frames(960000)
        assert torch.equal(out, fe.log_mel(wav[None], cfg)[0])
    with pytest.raises(ValueError, match=r"\[n_samples\]"):
        log_mel_stream(wav[None])


# ---- 4. search -> train_model -> StreamScorer -----------------------------------------------------------------------
def test_search_result_to_trained_model_reproduces_the_candidate():
    classes = 10
    Xtr, ytr, Xva, yva = make_split(192, 64, T, F, classes, 3)
    cfg = EvalConfig(variant="A", classes=classes, epochs=3, early_stop=False, batch=32, eval_batch=16, n_slots=2, seed=17)
    ev = PopulationEvaluator(Xtr, ytr, Xva, yva, cfg)
    assert ev.last_seeds == []
    genes = [(16, 3, 0, 1, 1, 0), (16, 3, 1, 1, 2, 1), (32, 5, 1, 2, 1, 0)]
    pop = [G.gene_to_hparams(g) for g in genes]
    ev.evaluate_individual(pop[0])
    assert ev.last_seeds == [17]
    res = ev.compute_objectives_and_constraints(pop)
    assert ev.last_seeds == [18, 19, 20]
    for i, (g, r) in enumerate(zip(genes, res)):
        tm = ev.train_model(pop[i], ev.last_seeds[i])
        assert isinstance(tm, TrainedModel) and tm.gene == g and (tm.T, tm.F, tm.seed) == (T, F, ev.last_seeds[i])
        print(g, "population objs", r["objs"], "train_model", tm.objectives)
        assert tm.objectives["acc"] == -r["objs"][0]                 # the same code on the same seed
        assert tm.objectives["fpr"] == r["objs"][2]
        assert tm.objectives["size_mb"] == r["objs"][1] and tm.objectives["epochs_run"] == 3 == ev.last_epochs_run[i]
        assert list(tm.tensors()) == [n for n, _, _ in G.param_tensors(g, 0, classes)]
        with tm.session(cfg) as net:
            _, acc, _ = net.evaluate(ev.X_val, ev.y_val)
            assert int(round(acc * 64)) == int(round(tm.objectives["acc"] * 64))
            assert np.array_equal(net.get_params(), tm.params)
    assert ev.train_model(genes[0], ev.last_seeds[0]).objectives == ev.train_model(pop[0], ev.last_seeds[0]).objectives


def test_stream_scorer_end_to_end(tmp_path):
    gene, classes, hop_frames = (16, 3, 0, 1, 1, 0), 10, 10
    cfg = EvalConfig(variant="B", classes=classes, eval_batch=4)
    with NetSession(gene, cfg, 101, 40, 5) as net:
        params = net.get_params()                                     # untrained: the seeded initial weights
    rs = np.random.RandomState(2)
    mean, scale = rs.randn(40) - 5.0, 1.0 + rs.rand(40)
    model = TrainedModel(gene=gene, variant="B", classes=classes, T=101, F=40, seed=5, params=params,
                         objectives={"acc": 0.1, "size_mb": G.model_size_mb(gene, 1, classes), "fpr": 0.5, "epochs_run": 0},
                         mean=mean, scale=scale)
    model.save(tmp_path / "m.npz")
    model = TrainedModel.load(tmp_path / "m.npz")
    assert np.array_equal(model.params, params) and model.frontend is None
    t = np.arange(32000) / 16000.0
    wav = dev((0.5 * np.sin(2 * np.pi * 440.0 * t) + 0.1 * rs.randn(32000)).astype(np.float32))     # 2 s at 16 kHz
    with StreamScorer(model, hop_frames, cfg) as scorer:
        t_start, probs = scorer.score(wav)
        assert tuple(probs.shape) == (11, classes) == (1 + (201 - 101) // hop_frames, classes)
        assert t_start.dtype == np.float64 and np.array_equal(t_start, np.arange(11) * hop_frames * 160 / 16000.0)
        p = probs.cpu().numpy()
        assert np.isfinite(p).all() and np.abs(p.astype(np.float64).sum(axis=1) - 1.0).max() <= ROWSUM_GATE
        # score = log_mel_stream + predict_stream: the same windows cut by hand, standardised, through predict_proba
        feat = log_mel_stream(wav)
        Xw = torch.stack([feat[i * hop_frames:i * hop_frames + 101] for i in range(11)]).contiguous()
        fe.standardize_apply(Xw, mean, scale)
        assert np.array_equal(p, scorer.net.predict_proba(Xw).cpu().numpy())
    with pytest.raises(ValueError, match="mel bands"):
        StreamScorer(dataclass_replace(model, frontend=FrontendConfig(n_mels=64)), hop_frames, cfg)


def dataclass_replace(model, **kw):
    import dataclasses
    return dataclasses.replace(model, **kw)
