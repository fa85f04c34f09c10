"""Integer inference: the level state of a net does not depend on the path taken to reach it.

A net trained a few steps with weight and activation quantisation on is taken through chains of ``set_int8`` level
combinations, ``set_quant`` and ``set_act_quant``; wherever it ends, its logits are compared IN BYTES with those of a fresh
session holding the same weights and ranges that was set directly to that state.  Nets, patch and batch are those of the
net tests of test_gpu_int8_fused.py: the smallest B_ds gene (matrix-core, depthwise and fusible ops) and the A_ds gene whose
fused ops apply a BatchNorm."""
import itertools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T, F, CLASSES, BATCH = 21, 12, 10, 3
NETS = [("B_ds", (16, 3, 1, 1, 1, 1)), ("A_ds", (16, 5, 1, 1, 1, 0))]
COMBOS = list(itertools.product((False, True), repeat=3))           # (on, depthwise, fused)
ACCEPTED = [c for c in COMBOS if c[0] or not (c[1] or c[2])]         # a level needs `on`
ALL, ONLY_FUSED, ONLY_DW, PLAIN, OFF = (True, True, True), (True, False, True), (True, True, False), (True, False, False), (False,) * 3


def _cfg(variant, quant=True, act=True):
    from cmoop_audio_processing_amd import EvalConfig, quant as Q
    return EvalConfig(variant=variant, classes=CLASSES, batch=BATCH, eval_batch=5, n_slots=1,
                      quant=Q.QuantConfig(bits=8) if quant else None,
                      act_quant=Q.ActQuantConfig(bits=8, momentum=0.9) if act else None)


class Trained:
    """The weights and ranges of one trained net, and the logits of fresh sessions set directly to a state (computed once)."""

    def __init__(self, variant, gene):
        import torch
        from cmoop_audio_processing_amd.session import NetSession
        self.variant, self.gene = variant, gene
        rs = np.random.RandomState(0)
        self.X = torch.from_numpy(rs.randn(BATCH, T, F).astype(np.float32)).cuda()
        y = torch.from_numpy(rs.randint(0, CLASSES, BATCH).astype(np.int32)).cuda()
        with NetSession(gene, _cfg(variant), T, F, 3) as net:
            for _ in range(4):
                net.train_step(self.X, y, None, 0, BATCH)
            self.params, self.ranges = net.get_params(), net.get_act_ranges()
            ops = len(net.int8_ops()), len(net.int8_dw_ops()), len(net.int8_fused_ops())
        assert min(ops) >= 1, "the net must have matrix-core, depthwise and fusible ops: %s" % (ops,)
        self._fresh = {}

    def open(self, quant=True, act=True):
        from cmoop_audio_processing_amd.session import NetSession
        net = NetSession(self.gene, _cfg(self.variant, quant, act), T, F, 3)
        net.set_params(self.params)
        if act:
            net.set_act_ranges(self.ranges)
        return net

    def logits(self, net):
        return net.predict_logits(self.X).cpu().numpy().tobytes()

    def fresh(self, combo=OFF, quant=True, act=True):
        """The bytes of a fresh session with these options that was set to `combo` directly (OFF: never had integer inference)."""
        key = (combo, quant, act)
        if key not in self._fresh:
            with self.open(quant, act) as net:
                if combo != OFF:
                    net.set_int8(*combo)
                self._fresh[key] = self.logits(net)
        return self._fresh[key]


@pytest.fixture(scope="module", params=NETS, ids=lambda n: n[0])
def trained(request):
    return Trained(*request.param)


def _mirrors(net):
    return (net.int8, net.int8_depthwise, net.int8_fused)


def test_a_combination_set_directly_is_reproducible(trained):
    # the references the other tests compare against: a second fresh session gives the same bytes
    for combo in ACCEPTED:
        with trained.open() as net:
            if combo != OFF:
                net.set_int8(*combo)
            assert _mirrors(net) == combo and trained.logits(net) == trained.fresh(combo), combo


@pytest.mark.parametrize("combo", COMBOS, ids=lambda c: "on%d_dw%d_fused%d" % c)
def test_a_combination_reached_through_the_other_levels_equals_the_fresh_net(trained, combo):
    from cmoop_audio_processing_amd import quant as Q
    with trained.open() as net:
        for step in (OFF, ALL, ONLY_FUSED, ONLY_DW, PLAIN):
            net.set_int8(*step)
            assert _mirrors(net) == step and trained.logits(net) == trained.fresh(step), step
        if combo not in ACCEPTED:                                   # refused: the net is the net it was
            before = trained.logits(net)
            with pytest.raises(ValueError, match="needs on=True"):
                net.set_int8(*combo)
            assert _mirrors(net) == PLAIN and trained.logits(net) == before == trained.fresh(PLAIN)
            return
        net.set_int8(*combo)
        assert _mirrors(net) == combo and trained.logits(net) == trained.fresh(combo)

        net.set_int8(*ALL)                                          # the weight codes go: every level goes with them
        net.set_quant(None)
        assert _mirrors(net) == OFF and trained.logits(net) == trained.fresh(OFF, quant=False)
        net.set_quant(Q.QuantConfig(bits=8))
        assert _mirrors(net) == OFF and trained.logits(net) == trained.fresh(OFF)
        net.set_int8(*combo)
        assert _mirrors(net) == combo and trained.logits(net) == trained.fresh(combo)

        net.set_int8(*ALL)                                          # the sites' codes go
        net.set_act_quant(None)
        assert _mirrors(net) == OFF and trained.logits(net) == trained.fresh(OFF, act=False)
        net.set_act_quant(Q.ActQuantConfig(bits=8, momentum=0.9))
        net.set_act_ranges(trained.ranges)
        assert _mirrors(net) == OFF and trained.logits(net) == trained.fresh(OFF)
        net.set_int8(*combo)
        assert _mirrors(net) == combo and trained.logits(net) == trained.fresh(combo)


def test_a_refused_level_leaves_the_next_pass_as_the_pass_before_it(trained):
    with trained.open() as net:
        net.set_int8(*ALL)
        before = trained.logits(net)
        with pytest.raises(ValueError, match="depthwise=True needs on=True"):
            net.set_int8(False, depthwise=True)
        assert _mirrors(net) == ALL and trained.logits(net) == before == trained.fresh(ALL)
