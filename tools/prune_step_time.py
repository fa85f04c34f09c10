#!/usr/bin/env python3
"""What magnitude pruning in training costs: the four-launch sequence alone (``cmoop_prune_weights_time``) on the arena of a
small gene (16, 3, 1, 1, 1, 1) and of the heaviest gene of the benchmark population (64, 5, 0, 3, 4, 1; 13.6 M parameters), and
warm train steps of ONE NetSession per mode at 101 x 40 / batch 64 with the option off and on.

  python tools/prune_step_time.py [--steps 100] [--repeats 7] [--sparsity 0.8] [--out profiles/prune_step_time.txt]

The launch sequence is timed at the final sparsity (every pruned tensor selects) and at sparsity 0 rows (k = 0 everywhere: the
copy launch alone).  A timed step window is one ``run_epoch`` over steps * 64 resident rows between two HIP events, as
tools/quant_step_time.py: the first epoch of every net is a warm-up, off and on alternate within a repeat of the same process,
the figure of a mode is the median of its repeats with the min-max spread.  The "on" net runs with begin_step = end_step = 0, so
every timed step selects at the final sparsity (the most expensive case).  No threshold is fixed here: the recorded value is
the claim.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENES = [(16, 3, 1, 1, 1, 1), (64, 5, 0, 3, 4, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="train steps per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--sparsity", type=float, default=0.8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prune_step_time.txt"), help="the lines are written here as well")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from cmoop_audio_processing_amd import EvalConfig, PruneConfig, genes as G
    from cmoop_audio_processing_amd import prune as PR
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("prune_step_time needs a GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    T, F, batch, classes = 101, 40, 64, 10
    n = args.steps * batch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    X = torch.randn((n, T, F), device="cuda", generator=gen)
    y = (torch.arange(n, device="cuda") % classes).to(torch.int32)
    cfg = EvalConfig.preset("nsga_penalty", variant="A", classes=classes, epochs=2 + args.repeats, batch=batch, early_stop=False)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)
    for gene in GENES:
        rows = PR.prune_table(gene, 0, classes)
        kernel_elems = sum(r[1] for r in rows)
        pruned_elems = sum(r[1] for r in rows if r[2] != 0)
        nets = {"off": NetSession(gene, cfg, T, F, 0), "on": NetSession(gene, cfg, T, F, 0)}
        nets["on"].set_prune(PruneConfig(sparsity=args.sparsity))
        # the launch sequence alone, on a copy of this net's own initial weights
        w = torch.from_numpy(nets["off"].get_params()).cuda()
        out = torch.empty_like(w)
        for what, s, tab in (("select+apply", args.sparsity, rows), ("copy only", 0.0, [(o, ln, 0) for o, ln, _k in rows])):
            kt = [PR.prune_weights_time(w, tab, s, out, iters=200) for _ in range(args.repeats)]
            med = statistics.median(kt)
            traffic = 4 * (3 * pruned_elems + 2 * kernel_elems) if what == "select+apply" else 8 * kernel_elems
            emit({"gene": list(gene), "params": nets["off"].n_params, "kernel_params": kernel_elems, "pruned_params": pruned_elems,
                  "tensors": len(rows), "sparsity": s, "launch_sequence_alone": what, "launches": 4 if s else 1,
                  "median_ms": round(med, 5), "min": round(min(kt), 5), "max": round(max(kt), 5), "bytes": traffic,
                  "gb_per_s": round(traffic / (med * 1e-3) / 1e9, 1)})
        times = {m: [] for m in nets}
        for m in nets:
            nets[m].run_epoch(X, y, 0)                      # warm-up: code objects, first-use allocations, the rate tables
        for r in range(args.repeats):
            for m in nets:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                nets[m].run_epoch(X, y, 1 + r)
                e1.record()
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                ev_ms = e0.elapsed_time(e1)
                times[m].append(ev_ms / args.steps)
                emit({"gene": list(gene), "params": nets[m].n_params, "prune": m, "repeat": r, "steps": args.steps,
                      "event_ms_per_step": round(ev_ms / args.steps, 5), "wall_ms_per_step": round(wall * 1e3 / args.steps, 5)})
        for m in nets:
            t = times[m]
            line = {"gene": list(gene), "params": nets[m].n_params, "prune": m, "summary": True,
                    "median_ms_per_step": round(statistics.median(t), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                    "spread_pct": round(100.0 * (max(t) - min(t)) / statistics.median(t), 2)}
            if m == "on":
                d = statistics.median(t) - statistics.median(times["off"])
                line["sparsity"] = args.sparsity
                line["minus_off_ms_per_step"] = round(d, 5)
                line["minus_off_pct"] = round(100.0 * d / statistics.median(times["off"]), 2)
                line["prune_size_mb"] = G.prune_size_mb(gene, 0, classes, args.sparsity)
                line["fp32_size_mb"] = G.model_size_mb(gene, 0, classes)
            emit(line)
        for net in nets.values():
            net.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
