#!/usr/bin/env python3
"""What activation fake-quantisation costs: the operator alone (``cmoop_fake_quant_act_time``: the two launches of batch mode,
the one launch of tracked mode) on the largest site of the heaviest gene of the benchmark population (64, 5, 0, 3, 4, 1) and of
a small gene (16, 3, 1, 1, 1, 1) at 101 x 40 / batch 64, and warm train steps of ONE NetSession per mode with the option off and
on.

  python tools/actquant_step_time.py [--steps 100] [--repeats 7] [--bits 8] [--out profiles/actquant_step_time.txt]

The operator: ``iters`` back-to-back calls between two HIP events, median of ``repeats`` windows; batch mode reads the tensor
twice and writes it once (12 bytes per element), tracked mode reads and writes it once (8 bytes per element); the achieved
bytes/s stand next to the 8 TB/s HBM figure of the MI355X.  A timed step window is one ``run_epoch`` over steps * 64 resident
rows between two HIP events, as tools/quant_step_time.py: the first epoch of every net is a warm-up, off and on alternate within
a repeat of the same process, the figure of a mode is the median of its repeats with the min-max spread.  No threshold is fixed
here: the recorded value is the claim.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GENES = [(16, 3, 1, 1, 1, 1), (64, 5, 0, 3, 4, 1)]
HBM_TB_PER_S = 8.0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100, help="train steps per timed window")
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--bits", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50, help="operator calls per timed window")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "actquant_step_time.txt"), help="the lines are written here as well")
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from cmoop_audio_processing_amd import ActQuantConfig, EvalConfig
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("actquant_step_time needs a GPU: there is nothing to time without one")
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
        sites = Q.act_sites(gene, "A", classes, T, F)
        elems = [batch * h * w * c for _a, h, w, c in sites]
        big = max(elems)
        x = torch.randn(big, device="cuda", generator=gen)
        for mode, a, bytes_per in (("batch", None, 12), ("tracked", 3.0, 8)):
            kt = [Q.fake_quant_act_time(x, args.bits, a=a, iters=args.iters) for _ in range(args.repeats)]
            med = statistics.median(kt)
            emit({"gene": list(gene), "sites": len(sites), "site_elems_per_step": sum(elems), "largest_site_elems": big,
                  "bits": args.bits, "operator_alone": mode, "launches": 2 if a is None else 1, "median_ms": round(med, 5),
                  "min": round(min(kt), 5), "max": round(max(kt), 5), "bytes": bytes_per * big,
                  "tb_per_s": round(bytes_per * big / (med * 1e-3) / 1e12, 3), "hbm_tb_per_s": HBM_TB_PER_S})
        nets = {"off": NetSession(gene, cfg, T, F, 0), "on": NetSession(gene, cfg, T, F, 0)}
        nets["on"].set_act_quant(ActQuantConfig(bits=args.bits))
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
                emit({"gene": list(gene), "params": nets[m].n_params, "act_quant": m, "repeat": r, "steps": args.steps,
                      "event_ms_per_step": round(ev_ms / args.steps, 5), "wall_ms_per_step": round(wall * 1e3 / args.steps, 5)})
        for m in nets:
            t = times[m]
            line = {"gene": list(gene), "params": nets[m].n_params, "act_quant": m, "summary": True,
                    "median_ms_per_step": round(statistics.median(t), 5), "min": round(min(t), 5), "max": round(max(t), 5),
                    "spread_pct": round(100.0 * (max(t) - min(t)) / statistics.median(t), 2)}
            if m == "on":
                d = statistics.median(t) - statistics.median(times["off"])
                line["bits"] = args.bits
                line["sites"] = len(sites)
                line["launches_per_step"] = 2 * len(sites)
                line["minus_off_ms_per_step"] = round(d, 5)
                line["minus_off_pct"] = round(100.0 * d / statistics.median(times["off"]), 2)
            emit(line)
        for net in nets.values():
            net.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
