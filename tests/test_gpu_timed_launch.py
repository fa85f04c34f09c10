"""GPU: the two timing modes of the MFMA conv launches.  A sampled launch (cfg.profile_every) is timed either by the kernel's own
begin / end events (the default) or, with CMOOP_PROFILE_PAIRS=1 -- what bench.py sets under a profiler -- by an event pair
recorded around it.  Both go through one launch_timed (csrc/gemm.hip); nothing else in the suite runs the event-pair mode."""
import math
import os

import numpy as np
import pytest
import torch

from cmoop_audio_processing_amd import _lib
from cmoop_audio_processing_amd.evaluator import EvalConfig
from cmoop_audio_processing_amd.session import NetSession

pytestmark = pytest.mark.gpu

#: (gene, T, F, batch, kernels its train step must reach -- checked against the host-only plan before anything is launched).
#: Topology A at 21x12: the implicit-GEMM forward / dgrad and weight gradient.  The 64-filter k3 net at 101x40: the halo weight
#: gradient at batch 2 (its forward launches are split-K there); batch 13 is the smallest at which cmoop_net_launch_plan names the
#: halo forward kernel too, un-split and with the balanced unit partition.
NETS = [
    ((16, 3, 1, 1, 1, 0), 21, 12, 8, ("igemm_fwd_kernel", "igemm_wgrad_kernel")),
    ((64, 3, 1, 1, 1, 0), 101, 40, 2, ("halo_wgrad_kernel",)),
    ((64, 3, 1, 1, 1, 0), 101, 40, 13, ("halo_fwd_kernel", "halo_wgrad_kernel")),
]
STEPS, CLASSES, SEED = 3, 10, 7


def _three_steps(gene, T, F, B, Xd, yd, profile_every, pairs):
    """Three train steps of a fresh net; CMOOP_PROFILE_PAIRS is read when the net is created."""
    cfg = EvalConfig(variant="A", classes=CLASSES, batch=B, eval_batch=B, profile_every=profile_every)
    before = os.environ.get("CMOOP_PROFILE_PAIRS")
    try:
        if pairs:
            os.environ["CMOOP_PROFILE_PAIRS"] = "1"
        else:
            os.environ.pop("CMOOP_PROFILE_PAIRS", None)
        net = NetSession(gene, cfg, T, F, SEED)
    finally:
        if before is None:
            os.environ.pop("CMOOP_PROFILE_PAIRS", None)
        else:
            os.environ["CMOOP_PROFILE_PAIRS"] = before
    with net:
        for i in range(STEPS):
            net.train_step(Xd, yd, None, row0=i * B, B=B)
        return net.get_state(), net.train_metrics()


@pytest.mark.parametrize("gene,T,F,B,reaches", NETS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else str(v))
def test_timing_a_launch_changes_no_result_and_both_modes_record_every_launch(gene, T, F, B, reaches):
    """Three train steps from one seed in a session timed by the kernels' own events, in one timed by event pairs and in one
    that is not timed: get_state() bit-equal and the train metrics equal across the three.  The two timed sessions sample
    every step (profile_every = 1): every launch-path variant cmoop_net_launch_plan names for the step is among
    profile_variants(), its kernel has launches > 0, the launches add up to two sessions x three steps x the plan's length,
    and every total_ms is finite and >= 0."""
    plan = _lib.net_launch_plan(gene, EvalConfig(variant="A", classes=CLASSES, batch=B, eval_batch=B, profile_every=1).to_struct(), T, F, B, 1)
    for kernel in reaches:
        assert any(n.startswith(kernel) for n in plan), (kernel, plan)
    rs = np.random.RandomState(11)
    Xd = torch.from_numpy(rs.randn(STEPS * B, T, F).astype(np.float32)).cuda()
    yd = torch.from_numpy(rs.randint(0, CLASSES, STEPS * B).astype(np.int32)).cuda()
    _lib.check(_lib.lib().cmoop_profile_reset())
    ext = _three_steps(gene, T, F, B, Xd, yd, 1, pairs=False)
    pairs = _three_steps(gene, T, F, B, Xd, yd, 1, pairs=True)
    variants = set(_lib.profile_variants())
    entries = {name: (launches, ms) for name, launches, ms, _ in _lib.profile_entries()}
    untimed = _three_steps(gene, T, F, B, Xd, yd, 0, pairs=False)

    for other in (pairs, untimed):
        for k in ("params", "m", "v"):
            assert np.array_equal(ext[0][k].view(np.uint32), other[0][k].view(np.uint32)), k
        assert (ext[0]["iterations"], ext[0]["steps"]) == (other[0]["iterations"], other[0]["steps"])
        assert ext[1] == other[1]
    assert np.isfinite(ext[0]["params"]).all() and math.isfinite(ext[1][0])

    print(f"{gene} {T}x{F} B={B}: plan {sorted(set(plan))}; sampled {sorted(entries.items())}")
    assert set(plan) <= variants, sorted(set(plan) - variants)
    for name in plan:
        assert entries[name.split("+")[0]][0] > 0, name
    assert sum(n for n, _ in entries.values()) == 2 * STEPS * len(plan)
    assert all(math.isfinite(ms) and ms >= 0.0 for _, ms in entries.values()), entries
