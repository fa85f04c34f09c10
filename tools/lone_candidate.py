#!/usr/bin/env python3
"""Step latency of ONE candidate alone on the GPU (the real-protocol tail: with early stopping a generation ends when
its slowest-converging candidate does, and that is often a small net).  Synthetic features of the bench's shape, one
stream, fixed epochs; prints train steps/s and the evaluation's wall time.  Run it under
`rocprofv3 --kernel-trace --stats` to get the sum of kernel durations and the launch count of the same command.

  python tools/lone_candidate.py 16,3,0,1,1,0 [--variant A] [--clips 6000] [--epochs 2] [--augment kws [--noise-std 0.1]]

--augment NAME trains with AugmentConfig.preset(NAME): one more launch (the augment kernel) and 2 * 4 * batch * T * F bytes
per step; compare the ms per step with and without it.
--mixup-alpha A / --label-smoothing E / --class-weight balanced train on the soft-target loss (LossConfig): two more launches
per step (targets, soft cross-entropy in place of the sparse one: one net launch more), and with mixup a third, the blend,
another streaming pass over one batch.
--ema M [--ema-warmup] trains with the weight EMA (EmaConfig): one more launch per step (12 bytes plus a kind byte per
parameter), and validation reads the averaged weights.  --history adds the per-epoch validation loss and accuracy of one
more fit of the same candidate and seed (NetSession.fit) to the line.
--quant-bits N trains quantisation-aware (QuantConfig): one more launch at the head of every step and of every validation
pass, 8 bytes per kernel parameter.
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmoop_audio_processing_amd import (AugmentConfig, EmaConfig, EvalConfig, LossConfig, PopulationEvaluator, QuantConfig,  # noqa: E402
                                        genes as G)
from cmoop_audio_processing_amd.session import NetSession  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("genes", nargs="+", help="one or more genes f,k,bn,R,fc,dr; each is timed alone")
    ap.add_argument("--variant", default="A")
    ap.add_argument("--clips", type=int, default=6000)
    ap.add_argument("--epochs", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=2)
    ap.add_argument("--augment", default="", help="AugmentConfig.preset name (kws); empty: no augmentation")
    ap.add_argument("--noise-std", type=float, default=0.0, help="feature noise on top of the --augment preset")
    ap.add_argument("--mixup-alpha", type=float, default=0.0, help="mixup with lam from Beta(alpha, alpha); 0: off")
    ap.add_argument("--label-smoothing", type=float, default=0.0, help="label smoothing eps; 0: off")
    ap.add_argument("--class-weight", default="", choices=["", "balanced"], help="balanced: n / (classes * count_c) of the train labels")
    ap.add_argument("--ema", type=float, default=0.0, help="weight EMA momentum (Keras' ema_momentum, e.g. 0.99); 0: off")
    ap.add_argument("--ema-warmup", action="store_true", help="--ema: m(i) = min(m, (1 + i) / (10 + i))")
    ap.add_argument("--quant-bits", type=int, default=0, help="quantisation-aware training at this width (2..8); 0: off")
    ap.add_argument("--history", action="store_true", help="add the per-epoch validation loss / accuracy of one more fit")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    n_tr, n_va = int(args.clips * 0.8), int(args.clips * 0.1)
    X = torch.randn((n_tr + n_va, 101, 40), device="cuda", generator=g)
    y = (torch.arange(n_tr + n_va, device="cuda") % 10).to(torch.int32)
    augment = AugmentConfig.preset(args.augment, noise_std=args.noise_std) if args.augment else None
    loss = LossConfig(mixup_alpha=args.mixup_alpha, label_smoothing=args.label_smoothing)
    if args.class_weight == "balanced":
        loss = LossConfig.balanced(y[:n_tr], 10, mixup_alpha=args.mixup_alpha, label_smoothing=args.label_smoothing)
    cfg = EvalConfig.preset("nsga_penalty", variant=args.variant, epochs=args.epochs, early_stop=False, n_slots=1, seed=0,
                            augment=augment, loss=loss if loss.enabled else None,
                            ema=EmaConfig(momentum=args.ema, warmup=args.ema_warmup) if args.ema > 0 else None,
                            quant=QuantConfig(bits=args.quant_bits) if args.quant_bits else None)
    ev = PopulationEvaluator(X[:n_tr], y[:n_tr], X[n_tr:], y[n_tr:], cfg)
    steps = args.epochs * ((n_tr + cfg.batch - 1) // cfg.batch)
    for gs in args.genes:
        gene = tuple(int(v) for v in gs.split(","))
        hp = G.gene_to_hparams(gene)
        best = 1e30
        for _ in range(args.repeat):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ev.evaluate_individual(hp)
            best = min(best, time.perf_counter() - t0)
        hist = {}
        if args.history:      # the seed evaluate_individual gave the candidate's first evaluation
            with NetSession(gene, cfg, 101, 40, cfg.seed) as net:
                r = net.fit(ev.X_train, ev.y_train, ev.X_val, ev.y_val)
            hist = {"val_loss_history": [float(v) for v in r["val_loss_history"]],
                    "val_accuracy_history": [float(v) for v in r["val_accuracy_history"]]}
        fl = G.eval_flops(gene, G.VARIANT_NAMES[args.variant], 10, 101, 40, n_tr, n_va, args.epochs, 1)
        print(json.dumps({"gene": gene, "variant": args.variant, "augment": args.augment or None, "noise_std": args.noise_std,
                          "mixup_alpha": args.mixup_alpha, "label_smoothing": args.label_smoothing, "class_weight": args.class_weight or None,
                          "ema": args.ema or None, "ema_warmup": bool(args.ema_warmup), "quant_bits": args.quant_bits or None, **hist,
                          "train_steps": steps, "wall_s": round(best, 4),
                          "steps_per_s": round(steps / best, 1), "ms_per_step_incl_val": round(best / steps * 1e3, 4),
                          "tflops": round(fl / best / 1e12, 2)}), flush=True)


if __name__ == "__main__":
    main()
