"""GPU parity of whole candidates of the depthwise-separable topologies A_ds / B_ds through the C ABI against the oracle twin
(tests/_dsnet_reference.py::SeparableOracleNet, gradients from autograd), at the gates tests/test_gpu_net.py applies to A / B;
then the paths around a candidate: the device step path, the population loop, save / load, stream scoring."""
import os

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import EvalConfig, PopulationEvaluator, StreamScorer, TrainedModel, genes as G
from cmoop_audio_processing_amd.frontend import log_mel_stream
from cmoop_audio_processing_amd.session import NetSession, epoch_permutation
from oracle import net as ON

from _dsnet_reference import SeparableOracleNet

pytestmark = pytest.mark.gpu

ENV_MODE = os.environ.get("CMOOP_GEMM_MODE", "")


def ocfg(cfg: EvalConfig) -> ON.OracleConfig:
    compute = "bf16" if (cfg.compute == "bf16" or (cfg.compute == "fp32" and ENV_MODE == "bf16")) else "fp32"
    return ON.OracleConfig(compute=compute, variant=G.VARIANT_NAMES[cfg.variant], classes=cfg.classes, epochs=cfg.epochs, batch=cfg.batch,
                           patience=cfg.patience, early_stop=cfg.early_stop, restore_best=cfg.restore_best, lr=cfg.lr,
                           dropout=cfg.dropout, shuffle=cfg.shuffle)


def make_data(n, T, F, classes, seed):
    rs = np.random.RandomState(seed)
    y = rs.randint(0, classes, size=n).astype(np.int32)
    proto = rs.randn(classes, T, F).astype(np.float32)
    X = (0.8 * proto[y] + rs.randn(n, T, F)).astype(np.float32)
    return X, y


def per_tensor_err(gene, variant, classes, a, b):
    """max-abs error of each canonical tensor relative to that tensor's max magnitude.  A pointwise (or first-conv) bias
    directly in front of a train-mode BatchNorm (topology A_ds) has an analytically ZERO gradient: both sides hold the
    rounding noise of a long fp32 sum, so there the check is |g| <= 2e-5 * (largest gradient entry of the net) on BOTH sides,
    reported on the scale of the other tensors' 5e-4 gate (tests/test_gpu_net.py::per_tensor_err)."""
    out, off = {}, 0
    gmax = float(np.abs(b).max())
    tensors = G.param_tensors(gene, variant, classes)
    for i, (name, shape, role) in enumerate(tensors):
        n = int(np.prod(shape))
        ra, rb = a[off:off + n].astype(np.float64), b[off:off + n].astype(np.float64)
        zero_grad = role == "bias" and i + 1 < len(tensors) and tensors[i + 1][2] == "gamma" and G.variant_is_a(variant)
        if zero_grad:
            out[name] = float(max(np.abs(ra).max(), np.abs(rb).max()) / (2e-5 * gmax + 1e-30)) * 5e-4 * 0.999
        else:
            out[name] = float(np.abs(ra - rb).max() / max(np.abs(rb).max(), 1e-4 * gmax, 1e-30))
        off += n
    return out


GENES = [
    ((16, 3, 0, 1, 1, 0), "A_ds"),
    ((16, 5, 1, 2, 2, 1), "A_ds"),
    ((32, 5, 1, 3, 3, 0), "A_ds"),
    ((16, 3, 1, 1, 2, 1), "B_ds"),
    ((32, 5, 0, 3, 4, 0), "B_ds"),
    ((64, 3, 1, 2, 1, 1), "B_ds"),
]


def init_step_grads_and_eval_parity(gene, variant, compute="fp32"):
    T, F, classes, B, seed = 21, 12, 10, 24, 1234
    cfg = EvalConfig(variant=variant, classes=classes, batch=32, eval_batch=16, compute=compute)
    X, y = make_data(80, T, F, classes, 1)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    v = G.VARIANT_NAMES[variant]
    onet = SeparableOracleNet(gene, ocfg(cfg), seed)
    with NetSession(gene, cfg, T, F, seed) as net:
        assert net.n_params == G.param_count(gene, v, classes) == onet.count_params()
        # 1. seeded glorot init (Keras' fans of the depthwise and pointwise kernels): bit-exact
        assert np.array_equal(net.get_params(), onet.get_flat())
        # 2. inference from identical weights: loss 1e-5 rel, identical predictions
        l_o, a_o, p_o = onet.evaluate(X, y)
        l_g, a_g, p_g = net.evaluate(Xd, yd)
        print(f"{variant}{gene} inference loss gpu {l_g:.7f} oracle {l_o:.7f}")
        assert abs(l_g - l_o) < 1e-5 * max(1.0, abs(l_o)), (l_g, l_o)
        assert np.array_equal(p_g.cpu().numpy(), p_o) and a_g == a_o
        # 3. one training step on rows idx[4:4+B]: gradients, updated weights, BN moving stats
        idx = np.random.RandomState(2).permutation(80).astype(np.int32)
        idxd = torch.from_numpy(idx).cuda()
        net.train_step(Xd, yd, idxd, row0=4, B=B)
        lo, co = onet.train_step(X[idx[4:4 + B]], y[idx[4:4 + B]])
        lg, cg = net.train_metrics()
        assert abs(lg - lo) < 2e-5 * max(1.0, abs(lo)) and cg == co
        gerr = per_tensor_err(gene, v, classes, net.get_grads(), onet.grads_flat())
        worst = max(gerr, key=gerr.get)
        print(f"   worst grad err {worst}: {gerr[worst]:.2e}")
        assert gerr[worst] < 5e-4, gerr
        # Adam's first step is +-lr for every weight regardless of |g|: compare at 2.5*lr absolute
        d = np.abs(net.get_params() - onet.get_flat())
        print(f"   max abs weight diff {d.max():.2e}")
        assert d.max() <= 2.5 * cfg.lr
        # 4. four more steps, then inference with the moving statistics
        for s in range(4):
            r0 = 4 + (s + 1) * 8
            net.train_step(Xd, yd, idxd, row0=r0, B=B)
            onet.train_step(X[idx[r0:r0 + B]], y[idx[r0:r0 + B]])
        l_o, a_o, p_o = onet.evaluate(X, y)
        l_g, a_g, p_g = net.evaluate(Xd, yd)
        print(f"   after 5 steps: loss gpu {l_g:.6f} oracle {l_o:.6f}; preds differing {(p_g.cpu().numpy() != p_o).sum()}")
        assert abs(l_g - l_o) < 5e-3 * max(1.0, abs(l_o))


@pytest.mark.parametrize("gene,variant", GENES)
def test_init_step_grads_and_eval_parity(gene, variant):
    init_step_grads_and_eval_parity(gene, variant)


@pytest.mark.skipif(ENV_MODE != "", reason="the arithmetic is forced from outside")
def test_parity_under_the_fp32_accurate_bf16x3_mode():
    """gemm_mode applies to the pointwise GEMMs (the depthwise kernels stay fp32): the same gates, the fp32 oracle"""
    init_step_grads_and_eval_parity((16, 5, 1, 2, 2, 1), "A_ds", compute="bf16x3")


def test_partial_batch_and_full_feature_size():
    """T x F = 101 x 40, batch 5 < configured 64: the depthwise slab regions are sized for the worst batch, not this one"""
    gene, variant, classes, seed = (16, 3, 1, 1, 1, 0), "A_ds", 10, 7
    cfg = EvalConfig(variant=variant, classes=classes, batch=64, eval_batch=8)
    X, y = make_data(12, 101, 40, classes, 5)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    onet = SeparableOracleNet(gene, ocfg(cfg), seed)
    with NetSession(gene, cfg, 101, 40, seed) as net:
        net.train_step(Xd, yd, None, row0=3, B=5)
        onet.train_step(X[3:8], y[3:8])
        gerr = per_tensor_err(gene, G.VARIANT_A_DS, classes, net.get_grads(), onet.grads_flat())
        print({k: f"{e:.1e}" for k, e in gerr.items()})
        assert max(gerr.values()) < 5e-4, gerr
        l_o, a_o, p_o = onet.evaluate(X, y)
        l_g, a_g, p_g = net.evaluate(Xd, yd)
        assert abs(l_g - l_o) < 1e-4 * max(1.0, abs(l_o))


@pytest.mark.parametrize("gene,variant", [((16, 5, 1, 2, 2, 1), "A_ds"), ((32, 3, 1, 2, 2, 1), "B_ds")])
def test_device_step_path_equals_explicit_steps_bit_for_bit(gene, variant):
    """run_epoch (device permutation, device step state, last batch of 16 of 32) against the same three steps issued one by
    one with their host arguments"""
    T, F, classes, seed, n = 21, 12, 10, 99, 80
    cfg = EvalConfig(variant=variant, classes=classes, batch=32, eval_batch=16)
    X, y = make_data(n, T, F, classes, 4)
    Xd, yd = torch.from_numpy(X).cuda(), torch.from_numpy(y).cuda()
    with NetSession(gene, cfg, T, F, seed) as a, NetSession(gene, cfg, T, F, seed) as b:
        a.run_epoch(Xd, yd, 0)
        idxd = torch.from_numpy(epoch_permutation(seed, 0, n)).cuda()
        for s in range(0, n, 32):
            b.train_step(Xd, yd, idxd, row0=s, B=min(32, n - s))
        sa, sb = a.get_state(), b.get_state()
        assert sa["iterations"] == sb["iterations"] == 3 and sa["steps"] == sb["steps"] == 3
        for k in ("params", "m", "v"):
            assert np.array_equal(sa[k], sb[k]), k
    with NetSession(gene, cfg, T, F, seed) as fresh:
        assert not np.array_equal(sa["params"], fresh.get_params())          # the epoch did train


def test_population_results_do_not_depend_on_the_slot_count():
    T, F, classes = 21, 12, 10
    X, y = make_data(144, T, F, classes, 8)
    for variant in ("A_ds", "B_ds"):
        genes = [g for g, v in GENES if v == variant] + [g for g, v in GENES if v != variant]      # all six, in both spaces
        seeds = list(range(40, 40 + len(genes)))
        runs = []
        for slots in (4, 2):
            cfg = EvalConfig(variant=variant, classes=classes, epochs=2, early_stop=False, batch=32, eval_batch=16, n_slots=slots, seed=40)
            runs.append(PopulationEvaluator(X[:96], y[:96], X[96:], y[96:], cfg).evaluate_genes(genes, seeds))
        assert np.array_equal(runs[0][:, :4], runs[1][:, :4]), (runs[0][:, :4], runs[1][:, :4])
        assert (runs[0][:, 3] == 2).all() and np.isfinite(runs[0][:, :3]).all()
        for g, row in zip(genes, runs[0]):
            assert row[1] == G.model_size_mb(g, G.VARIANT_NAMES[variant], classes)


def test_train_model_save_load_predict_and_stream_scoring(tmp_path):
    gene, variant, classes, hop_frames = (16, 3, 1, 1, 1, 0), "B_ds", 10, 20
    rs = np.random.RandomState(6)
    X, y = make_data(64, 101, 40, classes, 9)
    cfg = EvalConfig(variant=variant, classes=classes, epochs=1, early_stop=False, batch=16, eval_batch=4, n_slots=1, seed=3)
    ev = PopulationEvaluator(X[:48], y[:48], X[48:], y[48:], cfg)
    tm = ev.train_model(G.gene_to_hparams(gene), 3)
    assert isinstance(tm, TrainedModel) and tm.variant == variant and tm.objectives["size_mb"] == G.model_size_mb(gene, G.VARIANT_B_DS, classes)
    Xd = torch.from_numpy(X[48:]).cuda()
    with tm.session(cfg) as net:
        p0 = net.predict_proba(Xd).cpu().numpy()
    tm.save(tmp_path / "ds.npz")
    tm2 = TrainedModel.load(tmp_path / "ds.npz")
    assert tm2.variant == variant and np.array_equal(tm2.params, tm.params)
    with tm2.session(cfg) as net:
        assert np.array_equal(net.predict_proba(Xd).cpu().numpy(), p0)
    with NetSession(gene, cfg, 101, 40, 3) as fresh:
        assert np.isfinite(p0).all() and not np.array_equal(tm.params, fresh.get_params())       # a trained model
    # a 3-second noise recording: the windows the scorer returns are predict_proba of the windows cut by hand
    wav = torch.from_numpy((0.3 * rs.randn(48000)).astype(np.float32)).cuda()
    with StreamScorer(tm2, hop_frames, cfg) as scorer:
        t_start, probs = scorer.score(wav)
        feat = log_mel_stream(wav)
        nw = 1 + (int(feat.shape[0]) - 101) // hop_frames
        assert tuple(probs.shape) == (nw, classes) and nw == 11 and len(t_start) == nw
        Xw = torch.stack([feat[i * hop_frames:i * hop_frames + 101] for i in range(nw)]).contiguous()
        assert np.array_equal(probs.cpu().numpy(), scorer.net.predict_proba(Xw).cpu().numpy())
