#!/usr/bin/env python3
"""What the operating-point read-out costs a candidate: (1) its three launches (keys, counts, select) between HIP events
(``cmoop_operating_point_time``, after its own warm-up) at (n, C) = (6000, 10), (6000, 35), (65536, 35) on softmax scores;
(2) the extra ``predict`` pass over n_val = 6000 rows of 101 x 40 features for the cheapest and the heaviest gene of the
benchmark population (``bench.py``'s: seed 0, 40 candidates) -- a host clock around calls that end in a stream synchronise,
median of the repeats after one warm-up pass; (3) beside them, one whole fit of each of the two genes WITHOUT the option --
launch for launch the fit of a build without the read-out -- on 24 000 training rows, and the same fit WITH it.

  python tools/opoint_time.py [--epochs 10] [--repeats 7] [--out profiles/opoint_time.txt]

No threshold is fixed here: the recorded value is the claim.
"""
import argparse
import ctypes as C
import json
import os
import random
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(6000, 10), (6000, 35), (65536, 35)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--epochs", type=int, default=10, help="epochs of the fits the read-out is set beside (early stopping off)")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10, help="iterations per HIP-event window")
    ap.add_argument("--n-train", type=int, default=24000)
    ap.add_argument("--n-val", type=int, default=6000)
    ap.add_argument("--recall", type=float, default=0.95)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "opoint_time.txt"), help="the lines are written here as well")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from cmoop_audio_processing_amd import EvalConfig, OperatingPointConfig, _lib, genes as G
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("opoint_time needs a GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    op = OperatingPointConfig(args.recall)
    st = op._struct()
    # (1) the three launches
    for n, Cn in SHAPES:
        p = torch.softmax(3.0 * torch.randn((n, Cn), device="cuda", generator=gen), dim=1).contiguous()
        y = (torch.arange(n, device="cuda") % Cn).to(torch.int32)
        rows = []
        for _ in range(args.repeats):
            out = (C.c_double * 4)()
            torch.cuda.synchronize()
            _lib.check(_lib.lib().cmoop_operating_point_time(_lib.ptr(p), _lib.ptr(y), C.c_int64(n), C.c_int32(Cn), C.byref(st),
                                                             C.c_int32(args.iters), out))
            rows.append(list(out))
        med = [statistics.median(r[k] for r in rows) for k in range(4)]
        emit({"what": "read-out launches, HIP events", "n": n, "C": Cn, "iters": args.iters, "repeats": args.repeats,
              "median_ms": {"all_three": round(med[0], 4), "keys": round(med[1], 4), "counts": round(med[2], 4), "select": round(med[3], 4)},
              "all_three_min_max_ms": [round(min(r[0] for r in rows), 4), round(max(r[0] for r in rows), 4)],
              "compares": n * n * Cn, "compares_per_s": round(n * n * Cn / (med[2] * 1e-3))})
    # (2) the extra predict pass and (3) the fits
    T, F, classes = 101, 40, 10
    rng = random.Random(0)
    pop = [G.normalize_hparams(G.random_hparams(rng)) for _ in range(40)]
    cost = [G.fwd_flops_per_sample(g, 0, classes, T, F) for g in pop]
    genes = {"cheapest": pop[cost.index(min(cost))], "heaviest": pop[cost.index(max(cost))]}
    Xtr = torch.randn((args.n_train, T, F), device="cuda", generator=gen)
    ytr = (torch.arange(args.n_train, device="cuda") % classes).to(torch.int32)
    Xva = torch.randn((args.n_val, T, F), device="cuda", generator=gen)
    yva = (torch.arange(args.n_val, device="cuda") % classes).to(torch.int32)
    cfg = EvalConfig.preset("nsga_penalty", variant="A", classes=classes, epochs=args.epochs, early_stop=False)
    for name, gene in genes.items():
        with NetSession(gene, cfg, T, F, 0) as net:
            net.predict_proba(Xva)                                    # warm-up: code objects, first-use allocations
            t = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net.predict_proba(Xva)                                # returns after a stream synchronise
                t.append((time.perf_counter() - t0) * 1e3)
            r = []
            for _ in range(args.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                net.operating_point(Xva, yva, recall=args.recall)     # the pass, the three launches, the copy back and the finish
                r.append((time.perf_counter() - t0) * 1e3)
            emit({"what": "extra predict pass, host clock around a synchronising call", "gene": name, "genes": list(gene), "n_val": args.n_val,
                  "params": net.n_params, "median_ms": round(statistics.median(t), 3), "min_max_ms": [round(min(t), 3), round(max(t), 3)],
                  "pass_plus_read_out_median_ms": round(statistics.median(r), 3)})
        fit_s = {}
        for mode, c in (("off", cfg), ("on", EvalConfig.preset("nsga_penalty", variant="A", classes=classes, epochs=args.epochs,
                                                                 early_stop=False, operating_point=op))):
            with NetSession(gene, c, T, F, 0) as net:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                res = net.fit(Xtr, ytr, Xva, yva)
                fit_s[mode] = time.perf_counter() - t0
                assert ("operating_point" in res) == (mode == "on")
        emit({"what": "one fit, host clock (off: launch for launch the fit of a build without the read-out)", "gene": name,
              "n_train": args.n_train, "n_val": args.n_val, "epochs": args.epochs, "fit_s_off": round(fit_s["off"], 3),
              "fit_s_on": round(fit_s["on"], 3),
              "pass_plus_read_out_over_fit_pct": round(100.0 * statistics.median(r) * 1e-3 / fit_s["off"], 3)})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
