#!/usr/bin/env python3
"""What distillation costs a train step: warm train steps of ONE NetSession, the lightest and the heaviest gene of the
benchmark population (bench.py: 40 random genes of seed 0, topology A) at 101 x 40 / batch 64, distillation off and on.

  python tools/distill_time.py [--steps 200] [--repeats 5] [--off-only] [--root TREE]

A timed window is one ``run_epoch`` over steps * 64 resident rows -- the fit loop's own step path: the steps are enqueued
back to back and the call returns after a stream synchronise -- between two HIP events; both the event time and the host
clock around the same window are printed, per step.  The first epoch of every net is a warm-up and is not timed.  Off and
on alternate within a repeat, so a drift of the machine hits both.  On = DistillConfig.preset("kws") against a random
teacher table: two more launches than the sparse loss (targets, teacher rows) and the heavier single-workgroup loss kernel.

--off-only times the off path alone and needs nothing of distillation: with --root pointing at a built checkout of another
commit it gives that commit's figures in the same visit.  One JSON line per (gene, mode, repeat), then a summary line per
(gene, mode) with the median and the min-max spread.
"""
import argparse
import json
import os
import random
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200, help="train steps per timed window")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--off-only", action="store_true")
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    help="checkout whose package is timed (default: this one)")
    ap.add_argument("--label", default="", help="copied into every line")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.root))
    import torch
    from cmoop_audio_processing_amd import EvalConfig, genes as G
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("distill_time needs a GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    T, F, batch, classes = 101, 40, 64, 10
    rng = random.Random(0)
    pop = [G.normalize_hparams(G.random_hparams(rng)) for _ in range(40)]
    cost = [G.fwd_flops_per_sample(g, G.VARIANT_NAMES["A"], classes, T, F) for g in pop]
    picks = (("lightest", pop[cost.index(min(cost))]), ("heaviest", pop[cost.index(max(cost))]))
    n = args.steps * batch
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    X = torch.randn((n, T, F), device="cuda", generator=gen)
    y = (torch.arange(n, device="cuda") % classes).to(torch.int32)
    zt = 3.0 * torch.randn((n, classes), device="cuda", generator=gen)
    cfg = EvalConfig.preset("nsga_penalty", variant="A", classes=classes, epochs=2 + args.repeats, batch=batch, early_stop=False)
    modes = ("off",) if args.off_only else ("off", "on")
    for name, gene in picks:
        nets = {m: NetSession(gene, cfg, T, F, 0) for m in modes}
        if "on" in nets:
            from cmoop_audio_processing_amd import DistillConfig
            nets["on"].set_distill(DistillConfig.preset("kws"), zt)
        times = {m: [] for m in modes}
        for m in modes:
            nets[m].run_epoch(X, y, 0)                      # warm-up: code objects, first-use allocations, the step table
        for r in range(args.repeats):
            for m in modes:
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
                print(json.dumps({"label": args.label, "gene": list(gene), "which": name, "distill": m, "repeat": r, "steps": args.steps,
                                  "event_ms_per_step": round(ev_ms / args.steps, 5), "wall_ms_per_step": round(wall * 1e3 / args.steps, 5)}),
                      flush=True)
        for m in modes:
            t = times[m]
            print(json.dumps({"label": args.label, "gene": list(gene), "which": name, "distill": m, "summary": True,
                              "median_ms_per_step": round(statistics.median(t), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                              "spread_pct": round(100.0 * (max(t) - min(t)) / statistics.median(t), 2)}), flush=True)
        if len(modes) == 2:
            off, on = statistics.median(times["off"]), statistics.median(times["on"])
            print(json.dumps({"label": args.label, "which": name, "on_minus_off_ms_per_step": round(on - off, 5),
                              "on_over_off": round(on / off, 4)}), flush=True)
        for net in nets.values():
            net.close()


if __name__ == "__main__":
    main()
