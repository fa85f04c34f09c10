#!/usr/bin/env python3
"""End-to-end example: the reference's sa_nsga_penalty.py workflow (surrogate-assisted NSGA-II, optionally the full
memetic method of ablation_study/sa_nsga_local.py) on the MI355X evaluator.

Synthetic 1 s clips with --classes classes -> HIP log-mel front end -> (no scaler: quirk Q2 of sa_nsga_penalty.py:61-85)
-> stratified 50/25/25 split (sa_nsga_penalty.py:71-85) -> SA-NSGA-II on the host: the Kriging surrogate predicts every
offspring, only max(1, int(pop * infill)) of them per generation get a TRUE evaluation on the GPU(s).

    python examples/run_sa_nsga_penalty.py --pop 8 --gen 2 --clips 1200 --epochs 6                       # smoke-sized
    python examples/run_sa_nsga_penalty.py --pop 40 --gen 20 --classes 35                                 # BASELINE configs[2]
    python examples/run_sa_nsga_penalty.py --pop 64 --gen 20 --infill 0.334 --memetic --compute bf16      # BASELINE configs[4]
    python examples/run_sa_nsga_penalty.py --audio birdclef --pop 8 --gen 2 --clips 264 --epochs 6       # 128 x 128 dB-mel patches
    python examples/run_sa_nsga_penalty.py --audio birdclef --scale pcen --pop 8 --gen 2 --clips 264 --epochs 6   # ... PCEN patches
    python examples/run_sa_nsga_penalty.py --audio birdclef --space ds --pop 20 --gen 20                 # BASELINE configs[3]: DS-CNN space
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 examples/run_sa_nsga_penalty.py --pop 40 --gen 20
"""
import argparse
import dataclasses
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench import synth_waveforms  # noqa: E402
from cmoop_audio_processing_amd import (AugmentConfig, DistillConfig, EmaConfig, EvalConfig, LossConfig, PopulationEvaluator, TrainedModel,  # noqa: E402
                                        datasets, frontend, nsga, surrogate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pop", type=int, default=8)
    ap.add_argument("--gen", type=int, default=2)
    ap.add_argument("--infill", type=float, default=0.2, help="INFILL_PERCENT, sa_nsga_penalty.py:566")
    ap.add_argument("--clips", type=int, default=1200)
    ap.add_argument("--classes", type=int, default=11, help="11 = the BirdCLEF subset of sa_nsga_penalty.py; 35 = GSC-35")
    ap.add_argument("--epochs", type=int, default=300)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--memetic", action="store_true", help="LHS initial population + Lamarckian LCB local search (sa_nsga_local.py:351-433)")
    ap.add_argument("--compute", default="fp32", choices=["fp32", "bf16x3", "bf16"])
    ap.add_argument("--audio", default="gsc", choices=["gsc", "birdclef"],
                    help="gsc: 1 s clips at 16 kHz -> [101, 40] log-mel; birdclef: 65 280-sample clips at 32 kHz -> [128, 128] dB-mel "
                         "patches through FrontendConfig.preset('birdclef_128') (a build-defined recipe, see its docstring)")
    ap.add_argument("--scale", default="db", choices=["db", "pcen"],
                    help="--audio birdclef only: db = the preset's dB scale relative to each clip's loudest bin; pcen = the same "
                         "geometry with per-channel energy normalisation (PcenConfig.preset('bioacoustic')), which takes the "
                         "recording level and the stationary background out of the patch")
    ap.add_argument("--space", default="full", choices=["full", "ds"],
                    help="full: the reference's topology B; ds: its depthwise-separable form (variant B_ds: every k x k stride-1 "
                         "convolution after the first becomes depthwise k x k + pointwise 1 x 1), the low-size end of the front")
    ap.add_argument("--out", default="sa_nsga_generations.csv")
    ap.add_argument("--trace", default="", help="write a JSON trace: per evaluate call wall-clock, epochs run, hypervolume")
    ap.add_argument("--augment", default="", choices=["", "kws"],
                    help="train-time augmentation of every candidate's fit (AugmentConfig.preset; the reference has none): "
                         "kws = time shift <= 10 frames, 2 time masks <= 10, 2 frequency masks <= 5")
    ap.add_argument("--mixup-alpha", type=float, default=0.0,
                    help="mixup of every candidate's train batches with lam from Beta(alpha, alpha) (LossConfig; the reference has "
                         "none; 0 = off, 0.2 is the usual keyword-spotting value)")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="label smoothing eps of the training loss (0 = off)")
    ap.add_argument("--class-weight", default="", choices=["", "balanced"],
                    help="balanced: weight class c by n / (classes * count_c) of the training split (Keras' class_weight=)")
    ap.add_argument("--teacher", default="", help="MODEL.npz (TrainedModel.save) of an already trained, larger model: every candidate is "
                                                 "distilled against its logits of the training rows, computed once (DistillConfig; "
                                                 "the reference has none).  Its classes and patch shape must be this run's")
    ap.add_argument("--kd-alpha", type=float, default=0.7, help="--teacher: weight of the distillation term, in (0, 1]")
    ap.add_argument("--kd-temperature", type=float, default=4.0, help="--teacher: temperature T of the distillation term, in [1, 64]")
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
    if a.audio == "birdclef":
        # the synthesiser's time axis is in 1/16000 s steps: read at 32 kHz its partials sit at 400-8000 Hz
        cfg = frontend.FrontendConfig.preset("birdclef_128")
        if a.scale == "pcen":
            cfg = dataclasses.replace(cfg, scale="pcen", pcen=frontend.PcenConfig.preset("bioacoustic"))
        wav, y = synth_waveforms(a.clips, a.classes, 1234, dev, n_samples=65280)
        feats = frontend.log_mel(wav, cfg).cpu().numpy()        # [N, 128, 128] dB-mel (or PCEN), unscaled (Q2)
    else:
        if a.scale != "db":
            ap.error("--scale applies to --audio birdclef")
        wav, y = synth_waveforms(a.clips, a.classes, 1234, dev)
        feats = frontend.log_mel(wav).cpu().numpy()             # [N, 101, 40]; no StandardScaler in this script (Q2)
    del wav
    Xtr, ytr, Xva, yva, _, _ = datasets.stratified_50_25_25(feats, y.cpu().numpy(), random_state=42)
    preset = "sa_nsga_local" if a.memetic else "sa_nsga_penalty"
    # this script's features are not standardised (Q2): masked cells take the training mean, not 0.0
    augment = AugmentConfig.preset(a.augment, fill=float(Xtr.mean())) if a.augment else None
    # the training objective only: validation loss, accuracy and FPR stay those of the sparse cross-entropy
    loss = LossConfig(mixup_alpha=a.mixup_alpha, label_smoothing=a.label_smoothing)
    if a.class_weight == "balanced":
        loss = LossConfig.balanced(ytr, a.classes, mixup_alpha=a.mixup_alpha, label_smoothing=a.label_smoothing)
    ev = PopulationEvaluator(Xtr, ytr, Xva, yva, EvalConfig.preset(preset, classes=a.classes, epochs=a.epochs, seed=a.seed,
                                                                   verbose=(rank == 0), compute=a.compute, augment=augment,
                                                                   loss=loss if loss.enabled else None,
                                                                   distill=DistillConfig(a.kd_alpha, a.kd_temperature) if a.teacher else None,
                                                                   ema=EmaConfig(a.ema, a.ema_warmup) if a.ema > 0 else None,
                                                                   **({"variant": "B_ds"} if a.space == "ds" else {})))
    if a.teacher:
        ev.set_teacher(TrainedModel.load(a.teacher))      # one pass of the teacher over the training rows, shared by every candidate
    calls = []
    t_start = time.perf_counter()

    def evaluate(population):
        t0 = time.perf_counter()
        res = ev.compute_objectives_and_constraints(population)
        calls.append({"candidates": len(population), "seconds": round(time.perf_counter() - t0, 3),
                      "wall_clock_s": round(time.perf_counter() - t_start, 3), "epochs_run": list(ev.last_epochs_run)})
        if rank == 0:
            print(f"[search] true evaluation {len(calls)}: {len(population)} candidates in {calls[-1]['seconds']} s",
                  file=sys.stderr, flush=True)
        return res
    pareto, hist, true_evals = surrogate.sa_nsga2(evaluate, a.pop, a.gen, infill_percent=a.infill, seed=a.seed,
                                                  init="lhs" if a.memetic else "random", local_search=a.memetic)
    if rank == 0:
        nsga.write_records_csv(a.out, hist)
        fronts = [[[-r["Accuracy"], r["Size_MB"], r["FPR"]] for r in h] for h in hist]
        ref = nsga.shared_reference_point(fronts)
        hv = [nsga.hypervolume(f, ref) for f in fronts]
        for g, v in enumerate(hv):
            print(f"generation {g}: hypervolume {v:.6f}")
        if a.trace:
            with open(a.trace, "w") as fh:
                json.dump({"pop": a.pop, "gen": a.gen, "infill": a.infill, "memetic": a.memetic, "classes": a.classes,
                           "clips": a.clips, "gpus": world, "compute": a.compute, "true_evaluations": true_evals,
                           "reference_point": [float(v) for v in ref], "hypervolume_per_generation": hv,
                           "evaluate_calls": calls}, fh)
        print(f"{len(pareto)} feasible Pareto solutions; {true_evals} true evaluations of {a.pop * (a.gen + 1)} candidates seen; "
              f"records -> {a.out}")
    if world > 1:
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    main()
