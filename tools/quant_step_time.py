#!/usr/bin/env python3
"""What quantisation-aware training costs: the quantise launch alone (``cmoop_quantize_weights_time``) on the arena of a small
gene (16, 3, 1, 1, 1, 1) and of the heaviest gene of the benchmark population (64, 5, 0, 3, 4, 1; 13.6 M parameters), and warm
train steps of ONE NetSession per mode at 101 x 40 / batch 64 with the option off and on.

  python tools/quant_step_time.py [--steps 100] [--repeats 7] [--bits 8] [--out profiles/quant_step_time.txt]

A timed step window is one ``run_epoch`` over steps * 64 resident rows between two HIP events, as tools/ema_step_time.py:
the first epoch of every net is a warm-up, off and on alternate within a repeat of the same process, the figure of a mode is
the median of its repeats with the min-max spread.  No threshold is fixed here: the recorded value is the claim.
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
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "quant_step_time.txt"), help="the lines are written here as well")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from cmoop_audio_processing_amd import EvalConfig, QuantConfig, genes as G
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("quant_step_time needs a GPU: there is nothing to time without one")
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
        rows = Q.quant_table(gene, 0, classes)
        kernel_elems = sum(r[1] * r[2] for r in rows)
        nets = {"off": NetSession(gene, cfg, T, F, 0), "on": NetSession(gene, cfg, T, F, 0)}
        nets["on"].set_quant(QuantConfig(bits=args.bits))
        # the launch alone, on a copy of this net's own initial weights
        w = torch.from_numpy(nets["off"].get_params()).cuda()
        wq = torch.empty_like(w)
        kt = [Q.quantize_weights_time(w, rows, args.bits, wq, iters=200) for _ in range(args.repeats)]
        med = statistics.median(kt)
        emit({"gene": list(gene), "params": nets["off"].n_params, "kernel_params": kernel_elems, "tensors": len(rows),
              "channels": sum(r[1] for r in rows), "bits": args.bits, "launch_alone": True, "median_ms": round(med, 5),
              "min": round(min(kt), 5), "max": round(max(kt), 5), "bytes": 8 * kernel_elems,
              "gb_per_s": round(8 * kernel_elems / (med * 1e-3) / 1e9, 1)})
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
                emit({"gene": list(gene), "params": nets[m].n_params, "quant": m, "repeat": r, "steps": args.steps,
                      "event_ms_per_step": round(ev_ms / args.steps, 5), "wall_ms_per_step": round(wall * 1e3 / args.steps, 5)})
        for m in nets:
            t = times[m]
            line = {"gene": list(gene), "params": nets[m].n_params, "quant": m, "summary": True,
                    "median_ms_per_step": round(statistics.median(t), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                    "spread_pct": round(100.0 * (max(t) - min(t)) / statistics.median(t), 2)}
            if m == "on":
                d = statistics.median(t) - statistics.median(times["off"])
                line["bits"] = args.bits
                line["minus_off_ms_per_step"] = round(d, 5)
                line["minus_off_pct"] = round(100.0 * d / statistics.median(times["off"]), 2)
                line["quant_size_mb"] = G.quant_size_mb(gene, 0, classes, args.bits)
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
