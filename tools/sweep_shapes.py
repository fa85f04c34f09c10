"""Host-only generator of tests/_sweep_shapes.py: the conv cases of the geometry / batch sweep (tests/test_gpu_geometry_sweep.py).

Usage: python tools/sweep_shapes.py > tests/_sweep_shapes.py

The domain is every implicit-GEMM conv layer of every gene, both topologies, at SWEEP_FEATURE_SIZES, forward at batch 1..64
and the inference batches, backward at batch 1..64.  cmoop_conv_launch_plan names the launch-path variant of each launch and
launch_variants.edge_flags the edges it sits on; the list printed here witnesses every (variant, flag) pair of the domain at
two different (H, W) where the domain has two.  Deterministic greedy cover (gain per cost, small cases first); the host test
test_geometry_sweep_covers_every_variant_and_edge_of_the_domain re-derives the requirement, so the list may also be edited by
hand."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import launch_variants as LV  # noqa: E402
from _production_shapes import PRODUCTION_CONVS  # noqa: E402

SWEEP_FEATURE_SIZES = [(101, 40), (101, 13), (128, 128), (41, 20), (21, 12), (11, 40), (26, 40)]
WITNESSES = 2
#: per-case overhead in multiply-adds (launches, allocations, the float64 reference's set-up): keeps the cover from trading one
#: mid-sized case for a dozen tiny ones
CASE_OVERHEAD = 2e8


def cost(c):
    B, H, W, Ci, Co, KS, st = c
    return B * (-(-H // st)) * (-(-W // st)) * Ci * Co * KS * KS


def exact(c):
    """The integer regime's bounds.  Restated here, not imported, because this script WRITES tests/_sweep_shapes.py (where
    integer_regime_is_exact lives) and has to run when that file is absent or broken; the host test holds the list to the
    committed function."""
    B, H, W, Ci, Co, KS, st = c
    return Ci * KS * KS * 6 + 4 < 2 ** 24 and Co * KS * KS * 4 < 2 ** 24 and B * (-(-H // st)) * (-(-W // st)) * 6 < 2 ** 24


def generate():
    dom = LV.sweep_domain(SWEEP_FEATURE_SIZES)
    cap = max(cost(c) for c in PRODUCTION_CONVS)
    need = {pr: min(WITNESSES, len(by_hw)) for pr, by_hw in dom.items()}
    have = {pr: set() for pr in dom}
    for c in PRODUCTION_CONVS:                      # the benchmark's shapes count for the `any` flag
        for pr in LV.pairs_of(*c):
            if pr in have and pr[1] == "any":
                have[pr].add(c[1:3])
    cand = {}
    for pr, by_hw in dom.items():
        for cases in by_hw.values():
            for c in cases:
                if exact(c) and cost(c) <= cap:
                    cand.setdefault(c, set()).add(pr)
    chosen = []
    while True:
        best, best_key = None, None
        for c, prs in cand.items():
            gain = sum(1 for pr in prs if len(have[pr]) < need[pr] and c[1:3] not in have[pr])
            if gain:
                key = (-gain / (cost(c) + CASE_OVERHEAD), cost(c), c)
                if best_key is None or key < best_key:
                    best, best_key = c, key
        if best is None:
            break
        new = sorted(pr for pr in cand[best] if len(have[pr]) < need[pr] and best[1:3] not in have[pr])
        for pr in new:
            have[pr].add(best[1:3])
        chosen.append((best, new))
    short = sorted(pr for pr in dom if len(have[pr]) < need[pr])
    assert not short, f"pairs the cover could not witness inside the exactness / size bounds: {short}"
    return chosen, dom


def short_name(v):
    return v.replace("_kernel", "").replace("igemm_", "").replace(" ", "")


if __name__ == "__main__":
    chosen, dom = generate()
    print('"""Conv launch shapes of the geometry / batch sweep (tests/test_gpu_geometry_sweep.py) -- importable without the library so that')
    print("the host-only coverage test (tests/test_host_cpu.py) can hold the list against the launch-path variants and edge flags of")
    print('the whole domain.  The list is printed by tools/sweep_shapes.py; what counts is this file and the host test."""')
    print()
    print("#: (T, F) of the features: the benchmark's, 13 MFCCs, BirdCLEF-shaped patches, the net tests' sizes, short clips")
    print(f"SWEEP_FEATURE_SIZES = {SWEEP_FEATURE_SIZES}")
    print("#: forward launches: every train batch (a partial last one is any of 1..63) and the inference batches; backward: train only")
    print("SWEEP_FWD_BATCHES = tuple(range(1, 65)) + (100, 255, 256)")
    print("SWEEP_BWD_BATCHES = tuple(range(1, 65))")
    print()
    print()
    print("def integer_regime_is_exact(B, H, W, Cin, Cout, KS, stride):")
    print('    """x in {0..3}, w and dy in {-2..2}, bias in {-4..4}: every partial sum of the forward (|.| <= Cin*KS*KS*6 + 4), of the dgrad')
    print("    (<= Cout*KS*KS*4) and of the weight / bias gradient (<= M*6) is an integer below 2^24, hence exact in fp32 in ANY")
    print('    summation order."""')
    print("    M = B * (-(-H // stride)) * (-(-W // stride))")
    print("    return Cin * KS * KS * 6 + 4 < 2 ** 24 and Cout * KS * KS * 4 < 2 ** 24 and M * 6 < 2 ** 24")
    print()
    print()
    print(f"# B, H, W, Cin, Cout, KS, stride -- {len(chosen)} cases, {sum(cost(c) for c, _ in chosen):.1e} multiply-adds; behind each case the")
    print("# (variant: flags) pairs it was picked for (it exercises more)")
    print("SWEEP_CONVS = [")
    for c, new in chosen:
        by_v = {}
        for v, f in new:
            by_v.setdefault(short_name(v), []).append(f)
        why = "; ".join(f"{v}: {' '.join(fs)}" for v, fs in sorted(by_v.items()))
        print(f"    {str(c) + ',':34s} # {why if len(why) <= 112 else why[:108] + ' ...'}")
    print("]")
