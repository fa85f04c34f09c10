"""Host-only: the launch-path variants (cmoop_conv_launch_plan) the trainer uses for every conv layer of a set of genes.
Usage: python tools/launch_variants.py [--all] [--T 101 --F 40] [--batches 1-64,100,255,256]
(default: the bench's 40 genes of random.Random(0), batches 64 / 37 / 256).  Every variant is printed with the edge flags
(edge_flags below) its launches sit on; with --batches all genes of both topologies are walked over that batch range and each
(variant, flag) pair is listed with its case count and its number of distinct (H, W): what to read when the geometry-sweep
host test (tests/test_host_cpu.py) reports a missing pair."""
import argparse
import ctypes as C
import itertools
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmoop_audio_processing_amd import _lib, genes as G  # noqa: E402


def plan(op, B, H, W, Ci, Co, KS, st, stats=0):
    buf = C.create_string_buffer(200)
    _lib.check(_lib.lib().cmoop_conv_launch_plan(op, B, H, W, Ci, Co, KS, st, stats, buf, 200))
    return buf.value.decode()


def conv_layers(gene, variant, T, F):
    """(H, W, Cin, Cout, KS, stride, feeds_bn) of every implicit-GEMM conv of a candidate (the library's own plan walk)."""
    return _lib.plan_convs(gene, variant, T, F)


def variants_of(genes, variant, T, F, batch=64, eval_batch=256, partial=(37,)):
    used = {}
    for g in genes:
        for (H, W, Ci, Co, KS, st, bn) in conv_layers(g, variant, T, F):
            for B in (batch,) + tuple(partial):
                used.setdefault(plan(0, B, H, W, Ci, Co, KS, st, bn), set()).add(("fwd", B, H, W, Ci, Co, KS, st))
                used.setdefault(plan(1, B, H, W, Ci, Co, KS, st), set()).add(("dgrad", B, H, W, Ci, Co, KS, st))
                used.setdefault(plan(2, B, H, W, Ci, Co, KS, st), set()).add(("wgrad", B, H, W, Ci, Co, KS, st))
            used.setdefault(plan(0, eval_batch, H, W, Ci, Co, KS, st, 0), set()).add(("fwd", eval_batch, H, W, Ci, Co, KS, st))
    return used


ALL_CONV_GENES = list(itertools.product((16, 32, 64), (3, 5), (0, 1), (1, 2, 3), (1,), (0,)))   # fc / dropout add no conv shape
FLAGS = ("any", "ragged", "one_image", "multi_image_tile", "odd_width", "window_exceeds_image", "tight_halo")
FWD_BATCHES = tuple(range(1, 65)) + (100, 255, 256)      # every train batch incl. a partial last one, inference launches
BWD_BATCHES = tuple(range(1, 65))


def tile_rows(name):
    """M-tile rows of a launch-path variant: first template argument of igemm_fwd_kernel, second of halo_fwd_kernel,
    256 rows per step of the weight-gradient kernels."""
    args = [a.strip() for a in name[name.index("<") + 1:name.index(">")].split(",")]
    if name.startswith("igemm_fwd_kernel"):
        return int(args[0])
    if name.startswith("halo_fwd_kernel"):
        return int(args[1])
    assert "wgrad" in name, name
    return 256


def launch_rows(op, B, H, W, st):
    """Output pixels (GEMM rows) of a launch: op 0 forward, 1 dgrad, 2 wgrad.  The strided skip projection's dgrad runs over
    the pixels of dY and scatters."""
    if op == 1 and st == 1:
        return B * H * W
    return B * (-(-H // st)) * (-(-W // st))


def halo_tight(B, H, W, Ci, Co, KS):
    b, n, c = C.c_int32(), C.c_int32(), C.c_int32()
    _lib.check(_lib.lib().cmoop_halo_tile_check(B, H, W, Ci, Co, KS, C.byref(b), C.byref(n), C.byref(c)))
    return b.value > 0 and b.value == n.value


def edge_flags(op, name, B, H, W, Ci, Co, KS, st):
    """Edge flags of one launch (pure arithmetic on the shape and the variant's tile)."""
    bm = tile_rows(name)
    out = ["any"]
    if launch_rows(op, B, H, W, st) % bm:
        out.append("ragged")
    if B == 1:
        out.append("one_image")
    if B >= 3 and 2 * H * W <= bm:
        out.append("multi_image_tile")             # a tile holds whole images: two or more gaps
    if W % 2:
        out.append("odd_width")
    if H < KS or W < KS:
        out.append("window_exceeds_image")
    if name.startswith("halo_fwd_kernel") and (halo_tight(B, H, W, Co, Ci, KS) if op == 1 else halo_tight(B, H, W, Ci, Co, KS)):
        out.append("tight_halo")                   # the closed-form LDS row bound is exactly what the worst tile needs
    return out


def launches(B, H, W, Ci, Co, KS, st, backward=True):
    """[(op, variant name)] of a conv layer at a batch: forward with and without the statistics epilogue, dgrad, wgrad."""
    out = [(0, plan(0, B, H, W, Ci, Co, KS, st, 1)), (0, plan(0, B, H, W, Ci, Co, KS, st, 0))]
    if backward:
        out += [(1, plan(1, B, H, W, Ci, Co, KS, st)), (2, plan(2, B, H, W, Ci, Co, KS, st))]
    return out


def pairs_of(B, H, W, Ci, Co, KS, st, backward=True):
    """{(variant, flag)} the launches of one case exercise."""
    return {(name, f) for op, name in launches(B, H, W, Ci, Co, KS, st, backward)
            for f in edge_flags(op, name, B, H, W, Ci, Co, KS, st)}


def sweep_layers(sizes):
    """Distinct (H, W, Cin, Cout, KS, stride) of every implicit-GEMM conv of every gene, both topologies, over feature sizes."""
    seen = set()
    for (T, F) in sizes:
        for variant in (0, 1):
            for g in ALL_CONV_GENES:
                seen.update(l[:6] for l in conv_layers(g, variant, T, F))
    return sorted(seen)


def sweep_domain(sizes, fwd_batches=FWD_BATCHES, bwd_batches=BWD_BATCHES):
    """{(variant, flag): {(H, W): [case, ...]}} over the layers of `sizes` and the batch domain; case = (B, H, W, Cin, Cout,
    KS, stride).  A batch outside bwd_batches (an inference launch) contributes its forward launches only."""
    dom = {}
    bwd = set(bwd_batches)
    for (H, W, Ci, Co, KS, st) in sweep_layers(sizes):
        for B in sorted(set(fwd_batches) | bwd):
            for pr in pairs_of(B, H, W, Ci, Co, KS, st, B in bwd):
                dom.setdefault(pr, {}).setdefault((H, W), []).append((B, H, W, Ci, Co, KS, st))
    return dom


def parse_batches(txt):
    out = []
    for part in txt.split(","):
        lo, _, hi = part.partition("-")
        out += range(int(lo), int(hi or lo) + 1)
    return tuple(out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--all", action="store_true")
    ap.add_argument("--T", type=int, default=101)
    ap.add_argument("--F", type=int, default=40)
    ap.add_argument("--variant", default="A")
    ap.add_argument("--batches", default="", help="e.g. 1-64,100,255,256: list every variant with its edge flags over these batches "
                    "(backward launches for batches up to 64), both topologies, all genes")
    a = ap.parse_args()
    if a.batches:
        bs = parse_batches(a.batches)
        dom = sweep_domain([(a.T, a.F)], bs, tuple(b for b in bs if b <= 64))
        for name in sorted({n for n, _ in dom}):
            print(name)
            for f in FLAGS:
                if (name, f) in dom:
                    by_hw = dom[(name, f)]
                    print(f"    {f:22s} {sum(map(len, by_hw.values())):5d} cases at {len(by_hw):2d} (H, W)  e.g. {min(min(v) for v in by_hw.values())}")
        sys.exit(0)
    if a.all:
        genes = ALL_CONV_GENES
    else:
        rng = random.Random(0)
        genes = [G.normalize_hparams(G.random_hparams(rng)) for _ in range(40)]
    used = variants_of(genes, G.VARIANT_NAMES[a.variant], a.T, a.F)
    op_of = {"fwd": 0, "dgrad": 1, "wgrad": 2}
    for k in sorted(used):
        flags = {f for (kind, *shape) in used[k] for f in edge_flags(op_of[kind], k, *shape)}
        print(f"{k:60s} {len(used[k]):3d}  e.g. {sorted(used[k])[0]}  [{' '.join(f for f in FLAGS if f in flags)}]")
