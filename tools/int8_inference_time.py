#!/usr/bin/env python3
"""What integer inference gains and how far it lies from the fake-quantised pass.

  python tools/int8_inference_time.py [--repeats 7] [--iters 50] [--out profiles/int8_inference_time.txt]
                                      [--parity-out profiles/int8_inference_parity.txt]

(a) Lone layers at batch 256: ``cmoop_conv_fwd_i8_time`` against the fp32 trainer forward (``cmoop_conv_time`` mode 0) on
    64->64 k5 @101x40, 128->128 k5 @51x20, 512->512 k3 @13x5 and the 64->128 1x1 stride-2 projection @51x20 (``cmoop_conv_time``
    has no strided form: the projection's fp32 column stays empty).  ``iters`` back-to-back launches between two HIP events,
    median of ``repeats`` windows.
(b) ``predict_proba`` of 4096 clips at 101x40 on the heaviest gene of the benchmark population (64, 5, 0, 3, 4, 1) and on
    (16, 3, 1, 1, 1, 1): ONE NetSession (8-bit weights and activations, two train steps for the ranges), integer inference off
    and on alternating within a repeat, HIP events around the call, median of ``repeats`` with the min-max spread.
Parity: a model fitted for a few epochs on a synthetic 10-class set, ``TrainedModel.int8_report`` on its validation split:
    arg-max agreement and max |delta logit| of integer inference against the fake-quantised pass.  A reported number, no gate.
No threshold is fixed here: the recorded value is the claim.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [("64->64 k5 @101x40", 101, 40, 64, 64, 5, 1), ("128->128 k5 @51x20", 51, 20, 128, 128, 5, 1),
          ("512->512 k3 @13x5", 13, 5, 512, 512, 3, 1), ("64->128 1x1 s2 @51x20", 51, 20, 64, 128, 1, 2)]
GENES = [(64, 5, 0, 3, 4, 1), (16, 3, 1, 1, 1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window of a lone layer")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_inference_time.txt"))
    ap.add_argument("--parity-out", default=os.path.join(ROOT, "profiles", "int8_inference_parity.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from cmoop_audio_processing_amd import ActQuantConfig, EvalConfig, PopulationEvaluator, QuantConfig, _lib
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("int8_inference_time needs a GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    lines = []

    def emit(d, sink=lines):
        sink.append(json.dumps(d))
        print(sink[-1], flush=True)

    # ---- (a) lone layers ------------------------------------------------------------------------------------------------------
    B = args.batch
    for name, H, W, Cin, Cout, KS, stride in LAYERS:
        OH, OW = -(-H // stride), -(-W // stride)
        K = KS * KS * Cin
        xq = torch.randint(-127, 128, (B * H * W * Cin,), device="cuda", generator=gen, dtype=torch.int32).to(torch.int8)
        wq = torch.randint(-127, 128, (Cout * K,), device="cuda", generator=gen, dtype=torch.int32).to(torch.int8)
        s_w = torch.full((Cout,), 0.01, device="cuda")
        bias = torch.zeros(Cout, device="cuda")
        y = torch.empty(B * OH * OW * Cout, device="cuda")
        ti = [Q.conv_fwd_i8_time(xq, wq, 0.02, s_w, bias, y, B, H, W, Cin, Cout, KS, stride, 1, iters=args.iters) for _ in range(args.repeats)]
        line = {"layer": name, "batch": B, "M": B * OH * OW, "N": Cout, "K": K, "int8_median_ms": round(statistics.median(ti), 5),
                "int8_min": round(min(ti), 5), "int8_max": round(max(ti), 5),
                "int8_tops": round(2.0 * B * OH * OW * Cout * K / (statistics.median(ti) * 1e-3) / 1e12, 2)}
        if stride == 1:
            x = xq.to(torch.float32) * 0.02
            w = wq.to(torch.float32) * 0.01
            tf = []
            for _ in range(args.repeats):
                ms = C.c_double()
                torch.cuda.synchronize()
                _lib.check(_lib.lib().cmoop_conv_time(C.c_int32(0), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), C.c_void_p(bias.data_ptr()),
                                                      C.c_void_p(y.data_ptr()), *(C.c_int32(v) for v in (B, H, W, Cin, Cout, KS, args.iters)),
                                                      C.byref(ms)))
                tf.append(float(ms.value))
            line.update({"fp32_median_ms": round(statistics.median(tf), 5), "fp32_min": round(min(tf), 5), "fp32_max": round(max(tf), 5),
                         "fp32_over_int8": round(statistics.median(tf) / statistics.median(ti), 3)})
            del x, w
        else:
            line["fp32_median_ms"] = None                     # cmoop_conv_time has no strided form
        emit(line)
        del xq, wq, y

    # ---- (b) whole inference passes -------------------------------------------------------------------------------------------
    T, F, classes = 101, 40, 10
    X = torch.randn((args.clips, T, F), device="cuda", generator=gen)
    yl = (torch.arange(args.clips, device="cuda") % classes).to(torch.int32)
    cfg = EvalConfig.preset("nsga_penalty", variant="A", classes=classes, batch=64, early_stop=False,
                            quant=QuantConfig(bits=8), act_quant=ActQuantConfig(bits=8))
    for gene in GENES:
        with NetSession(gene, cfg, T, F, 0) as net:
            net.train_step(X, yl, None, 0, 64)
            net.train_step(X, yl, None, 64, 64)
            times = {"off": [], "on": []}
            for m in times:                                   # warm-up of both modes: code objects, first-use allocations
                net.set_int8(m == "on")
                net.predict_proba(X)
            for r in range(args.repeats):
                for m in times:
                    net.set_int8(m == "on")
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    net.predict_proba(X)
                    e1.record()
                    torch.cuda.synchronize()
                    times[m].append(e0.elapsed_time(e1))
                    emit({"gene": list(gene), "int8": m, "repeat": r, "clips": args.clips, "predict_ms": round(times[m][-1], 4)})
            med = {m: statistics.median(t) for m, t in times.items()}
            for m, t in times.items():
                line = {"gene": list(gene), "params": net.n_params, "int8": m, "summary": True, "clips": args.clips,
                        "median_predict_ms": round(med[m], 4), "min": round(min(t), 4), "max": round(max(t), 4),
                        "spread_pct": round(100.0 * (max(t) - min(t)) / med[m], 2)}
                if m == "on":
                    line["int8_ops"] = len(net.int8_ops())
                    line["off_over_on"] = round(med["off"] / med["on"], 3)
                    line["faster_beyond_off_spread"] = bool(med["on"] < min(times["off"]))
                emit(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")

    # ---- parity of a fitted model -----------------------------------------------------------------------------------------------
    plines = []
    rs = np.random.RandomState(7)
    n_train, n_val = 1536, 512
    yy = rs.randint(0, classes, n_train + n_val).astype(np.int32)
    XX = (rs.randn(n_train + n_val, T, F) + yy[:, None, None] * 0.15).astype(np.float32)
    Xd, yd = torch.from_numpy(XX).cuda(), torch.from_numpy(yy).cuda()
    for variant, gene in (("A", (16, 3, 1, 1, 1, 1)), ("B", (32, 5, 0, 2, 3, 1)), ("A_ds", (16, 3, 1, 1, 2, 0))):
        pcfg = EvalConfig.preset("nsga_penalty", variant=variant, classes=classes, batch=64, epochs=3, early_stop=False, n_slots=1,
                                 quant=QuantConfig(bits=8), act_quant=ActQuantConfig(bits=8))
        model = PopulationEvaluator(Xd[:n_train], yd[:n_train], Xd[n_train:], yd[n_train:], pcfg).train_model(gene, 1)
        rep = model.int8_report(Xd[n_train:], yd[n_train:], pcfg)
        emit({"gene": list(gene), "variant": variant, "epochs": 3, "bits": 8, **{k: (round(v, 8) if isinstance(v, float) else v) for k, v in rep.items()}},
             plines)
    if args.parity_out:
        os.makedirs(os.path.dirname(os.path.abspath(args.parity_out)), exist_ok=True)
        with open(args.parity_out, "w") as f:
            f.write("\n".join(plines) + "\n")


if __name__ == "__main__":
    main()
