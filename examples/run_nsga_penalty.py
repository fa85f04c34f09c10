#!/usr/bin/env python3
"""End-to-end example: the reference's nsga_penalty.py workflow on the MI355X evaluator.

Synthetic 1 s clips -> HIP log-mel front end -> StandardScaler -> constrained NSGA-II
(host) whose fitness evaluations run on the GPU; writes per-generation records (the
reference's column schema) and prints the hypervolume of each generation's population
against one shared reference point (compare.ipynb semantics).

    python examples/run_nsga_penalty.py --pop 4 --gen 2 --clips 2000 --epochs 3
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/run_nsga_penalty.py --pop 40 --gen 20
"""
import argparse
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_waveforms  # noqa: E402
from cmoop_audio_processing_amd import AugmentConfig, EmaConfig, EvalConfig, PopulationEvaluator, frontend, nsga  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=4)
    ap.add_argument("--gen", type=int, default=2)
    ap.add_argument("--clips", type=int, default=2000)
    ap.add_argument("--epochs", type=int, default=300)      # EPOCHS, nsga_penalty.py:177 (early stopping active)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--out", default="nsga_generations.csv")
    ap.add_argument("--trace", default="", help="write a JSON trace: per evaluate call wall-clock, epochs run, hypervolume")
    ap.add_argument("--compute", default="fp32", choices=["fp32", "bf16x3", "bf16"])
    ap.add_argument("--hard", action="store_true",
                    help="hypervolume runs: low SNR (--snr-db) and neighbouring classes share two of three partials, so accuracies "
                         "spread (like the reference's published Pareto range) instead of saturating at 1.0")
    ap.add_argument("--snr-db", type=float, default=-17.0, help="SNR of the --hard set")
    ap.add_argument("--fpr", default="v1_quirk", choices=["v1_quirk", "v1", "v3"],
                    help="v1_quirk = nsga_penalty.py:387 (y_true all zeros: FPR <= 1/C, constraint g3 inactive); v1 = every other script")
    ap.add_argument("--augment", default="", choices=["", "kws"],
                    help="train-time augmentation of every candidate's fit (AugmentConfig.preset; the reference has none): "
                         "kws = time shift <= 10 frames, 2 time masks <= 10, 2 frequency masks <= 5")
    ap.add_argument("--ema", type=float, default=0.0,
                    help="weight EMA momentum of every candidate's fit (EmaConfig, Keras' ema_momentum; the reference has none): "
                         "validation, early stopping and the read-outs take the averaged weights (0 = off, 0.99 is Keras' default)")
    ap.add_argument("--ema-warmup", action="store_true", help="--ema: m(i) = min(m, (1 + i) / (10 + i))")
    a = ap.parse_args()
    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    if world > 1:
        torch.distributed.init_process_group("nccl", device_id=torch.device("cuda", local))
    dev = torch.device("cuda", local)
    wav, y = synth_waveforms(a.clips, 10, 1234, dev, hard=a.hard, hard_snr_db=a.snr_db)
    feats = frontend.log_mel(wav)
    n_tr, n_va = int(a.clips * 0.8), int(a.clips * 0.1)
    Xtr, Xva = feats[:n_tr].contiguous(), feats[n_tr:n_tr + n_va].contiguous()
    frontend.prepare_dataset(Xtr, Xva, None, mode="refit")
    ev = PopulationEvaluator(Xtr, y[:n_tr], Xva, y[n_tr:n_tr + n_va],
                             EvalConfig.preset("nsga_penalty", epochs=a.epochs, seed=a.seed, verbose=(rank == 0),
                                               compute=a.compute, fpr_variant=a.fpr,
                                               augment=AugmentConfig.preset(a.augment) if a.augment else None,
                                               ema=EmaConfig(a.ema, a.ema_warmup) if a.ema > 0 else None))
    calls = []
    t_start = time.perf_counter()
    if rank == 0:      # a generation at full size takes minutes: keep stderr alive (job runners kill silent commands)
        import threading
        stop = threading.Event()

        def heartbeat():
            while not stop.wait(60.0):
                print(f"[search] running, {time.perf_counter() - t_start:.0f} s, {len(calls)} evaluate calls done", file=sys.stderr, flush=True)
        threading.Thread(target=heartbeat, daemon=True).start()

    def evaluate(population):
        t0 = time.perf_counter()
        res = ev.compute_objectives_and_constraints(population)
        calls.append({"candidates": len(population), "seconds": round(time.perf_counter() - t0, 3),
                      "wall_clock_s": round(time.perf_counter() - t_start, 3), "epochs_run": list(ev.last_epochs_run)})
        if rank == 0 and a.trace:      # partial trace after every call: a run cut off by a time limit still leaves its stamps
            with open(a.trace + ".partial", "w") as fh:
                json.dump({"pop": a.pop, "gen": a.gen, "clips": a.clips, "hard_synthetic": a.hard, "n_train": n_tr, "evaluate_calls": calls,
                           "objectives_of_last_call": [r["objs"] for r in res]}, fh)
        if rank == 0:
            print(f"[search] evaluate call {len(calls)}: {len(population)} candidates in {calls[-1]['seconds']} s, "
                  f"epochs run min/mean/max {min(ev.last_epochs_run)}/{sum(ev.last_epochs_run) / len(population):.1f}/"
                  f"{max(ev.last_epochs_run)}", file=sys.stderr, flush=True)
        return res
    pareto, hist = nsga.nsga2(evaluate, a.pop, a.gen, seed=a.seed)
    if rank == 0:
        nsga.write_records_csv(a.out, hist)
        fronts = [[[-r["Accuracy"], r["Size_MB"], r["FPR"]] for r in h] for h in hist]
        ref = nsga.shared_reference_point(fronts)
        hv = [nsga.hypervolume(f, ref) for f in fronts]
        for g, v in enumerate(hv):
            print(f"generation {g}: hypervolume {v:.6f}")
        if a.trace:
            with open(a.trace, "w") as fh:
                json.dump({"pop": a.pop, "gen": a.gen, "clips": a.clips, "hard_synthetic": a.hard, "fpr_variant": a.fpr,
                           "accuracy_min_mean_max_last_generation": [min(r["Accuracy"] for r in hist[-1]),
                                                                     sum(r["Accuracy"] for r in hist[-1]) / len(hist[-1]),
                                                                     max(r["Accuracy"] for r in hist[-1])], "n_train": n_tr, "max_epochs": a.epochs, "gpus": world,
                           "compute": a.compute, "reference_point": [float(v) for v in ref], "hypervolume_per_generation": hv,
                           "evaluate_calls": calls, "true_evaluations": ev.evals_done,
                           "evals_per_hour": round(ev.evals_done / (calls[-1]["wall_clock_s"] / 3600.0), 1)}, fh)
        print(f"{len(pareto)} feasible Pareto solutions; {ev.evals_done} true evaluations; records -> {a.out}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
