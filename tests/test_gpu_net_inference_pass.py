"""GPU: the four inference entry points of a net share one pass (Net::inference_pass).  What that makes easy to break -- the
partial last chunk, and the weight stage (prune, then quantise, of the arena inference reads) applied once and to the right
arena -- is held here by the entry points against each other and against a float64 restatement, never against recorded values:
under each of the eight EMA / prune / quant combinations, after a few train steps, for n rows in {1, eval_batch, eval_batch + 1}."""
import ctypes as C
import dataclasses
import itertools

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import EmaConfig, PruneConfig, QuantConfig, _lib
from cmoop_audio_processing_amd.session import NetSession
from test_gpu_optim import CFG, CLASSES, F_, GENE, SEED, T_, data, dev, host, same_bits

pytestmark = pytest.mark.gpu

P = _lib.ptr
NS = (1, CFG.eval_batch, CFG.eval_batch + 1)                # one partial chunk, one full chunk, a full chunk and a partial one
STEPS_B = (8, 5, 8)
COMBOS = list(itertools.product((False, True), repeat=3))


def cfg_of(ema, prune, quant):
    return dataclasses.replace(CFG, ema=EmaConfig(0.7) if ema else None, prune=PruneConfig(sparsity=0.8, begin_step=1, end_step=4) if prune else None,
                               quant=QuantConfig(bits=4) if quant else None)


def softmax_probs(z):
    p = torch.empty_like(z)
    _lib.check(_lib.lib().cmoop_softmax_probs(P(z), P(p), C.c_int32(z.shape[0]), C.c_int32(z.shape[1])))
    torch.cuda.synchronize()
    return p


def reads(net, Xn, yn):
    """(loss sum, preds, probs, logits, stream probs) of the n rows; the stream is the rows laid end to end, hop = T"""
    loss, _acc, preds = net.evaluate(Xn, yn)
    return (loss * len(Xn), host(preds), host(net.predict_proba(Xn)), host(net.predict_logits(Xn)),
            host(net.predict_stream(Xn.reshape(-1, F_), T_)))


def check_reads(net, Xn, yn, what):
    loss_sum, preds, probs, logits, stream = reads(net, Xn, yn)
    n = len(Xn)
    assert probs.shape == logits.shape == stream.shape == (n, CLASSES) and preds.shape == (n,), what
    assert same_bits(host(softmax_probs(dev(logits))), probs), (what, "predict is the softmax of predict_logits")
    assert np.array_equal(preds, probs.argmax(1)), (what, "evaluate's predictions are predict's first arg max")
    z = logits.astype(np.float64)
    zmax = z.max(1, keepdims=True)
    nll = np.log(np.exp(z - zmax).sum(1)) + zmax[:, 0] - z[np.arange(n), host(yn)]
    print(f"  {what}: loss sum {loss_sum:.9g}, float64 from the logits {nll.sum():.9g}")
    assert abs(loss_sum - nll.sum()) < 1e-5 * max(1.0, abs(nll.sum())), (what, loss_sum, nll.sum())
    assert same_bits(stream, probs), (what, "predict_stream over the rows laid end to end")
    return loss_sum, preds, probs, logits, stream


@pytest.mark.parametrize("ema,prune,quant", COMBOS)
def test_the_four_entry_points_agree_on_every_chunking(ema, prune, quant):
    X, y = data()
    Xd, yd = dev(X), dev(y)
    cfg = cfg_of(ema, prune, quant)
    with NetSession(GENE, cfg, T_, F_, SEED) as net, NetSession(GENE, dataclasses.replace(cfg, ema=None), T_, F_, SEED) as twin:
        row0 = 0
        for B in STEPS_B:
            net.train_step(Xd, yd, None, row0=row0, B=B)
            row0 += B
        raw = {n: check_reads(net, Xd[:n], yd[:n], f"n={n}") for n in NS}
        for a, b in zip(raw[NS[1]][1:], raw[NS[2]][1:]):
            assert a.tobytes() == b[:NS[1]].tobytes(), "the full first chunk is the same launches whatever follows it"
        if ema:     # all four read the average: a second net whose parameters ARE the average reads the same bytes
            avg = net.get_ema()
            assert not same_bits(avg, net.get_params())
            twin.set_params(avg)
            net.use_ema(True)
            for n in NS:
                got = check_reads(net, Xd[:n], yd[:n], f"n={n} average")
                want = reads(twin, Xd[:n], yd[:n])
                assert got[0] == want[0] and all(a.tobytes() == b.tobytes() for a, b in zip(got[1:], want[1:])), n
            net.use_ema(False)
            for n in NS:
                again = reads(net, Xd[:n], yd[:n])
                assert again[0] == raw[n][0] and all(a.tobytes() == b.tobytes() for a, b in zip(again[1:], raw[n][1:])), n
        # no rows: success, and nothing is written
        for symbol in ("cmoop_net_predict", "cmoop_net_predict_logits"):
            out = torch.full((3, CLASSES), -7.25, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            _lib.check(getattr(_lib.lib(), symbol)(net._h, P(Xd), C.c_int64(0), P(out)))
            torch.cuda.synchronize()
            assert (host(out) == np.float32(-7.25)).all(), symbol
