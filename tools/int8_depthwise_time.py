#!/usr/bin/env python3
"""What the second level of integer inference (integer depthwise) costs or gains, and how far it lies from the first level.

  python tools/int8_depthwise_time.py [--repeats 7] [--iters 50] [--out profiles/int8_depthwise_time.txt]

The protocol of tools/int8_inference_time.py: ``iters`` back-to-back launches between two HIP events, median of ``repeats``
windows, the two sides alternating within a repeat in one process.
(a) Lone layers at batch 256 on the four depthwise shapes of DESIGN section 4b: the ONE launch (``cmoop_dwconv_fwd_i8_time`` with
    an output range and the codes) against the PAIR it replaces -- the fp32 depthwise forward (``cmoop_dwconv_time`` mode 0) plus
    the tracked quantiser with codes (``cmoop_fake_quant_act_codes_time``), each timed alone and added.
(b) ``predict_proba`` of 4096 clips at 101x40 on the A_ds genes (64, 5, 1, 3, 4, 1) and (16, 3, 1, 1, 1, 1): ONE NetSession,
    ``set_int8(True)`` against ``set_int8(True, depthwise=True)``.
(c) Level 2 against level 1 on the A_ds model and data of profiles/int8_inference_parity.txt: arg-max agreement and max |delta
    logit|, plus ``int8_report(depthwise=True)`` (level 2 against the fake-quantised pass).
No threshold is fixed here: the recorded value is the claim.
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYERS = [(101, 40, 64, 5), (51, 20, 128, 5), (26, 10, 256, 3), (13, 5, 512, 3)]
GENES = [(64, 5, 1, 3, 4, 1), (16, 3, 1, 1, 1, 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window of a lone layer")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_depthwise_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    from cmoop_audio_processing_amd import ActQuantConfig, EvalConfig, PopulationEvaluator, QuantConfig, _lib
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("int8_depthwise_time needs a GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    # ---- (a) lone layers: one launch against the two it replaces -----------------------------------------------------------------
    B = args.batch
    for H, W, Cn, K in LAYERS:
        n = B * H * W * Cn
        xq = torch.randint(-127, 128, (n,), device="cuda", generator=gen, dtype=torch.int32).to(torch.int8)
        wq = torch.randint(-127, 128, (K * K * Cn,), device="cuda", generator=gen, dtype=torch.int32).to(torch.int8)
        s_x, s_w = 0.02, torch.full((Cn,), 0.01, device="cuda")
        x, w = xq.to(torch.float32) * s_x, wq.to(torch.float32) * 0.01
        y, z, codes = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.int8)
        a_out = float(0.5 * 127 * 127 * K * s_x * 0.01)      # about a third of the sums clamp
        t_one, t_dw, t_q = [], [], []
        for _ in range(args.repeats):
            t_one.append(Q.dwconv_fwd_i8_time(xq, wq, s_x, s_w, y, B, H, W, Cn, K, out_bits=8, a_out=a_out, codes=codes, iters=args.iters))
            ms = C.c_double()
            torch.cuda.synchronize()
            _lib.check(_lib.lib().cmoop_dwconv_time(C.c_int32(0), C.c_void_p(x.data_ptr()), C.c_void_p(w.data_ptr()), None, C.c_void_p(z.data_ptr()),
                                                    *(C.c_int32(v) for v in (B, H, W, Cn, K, args.iters)), C.byref(ms)))
            t_dw.append(float(ms.value))
            t_q.append(Q.fake_quant_act_codes_time(z, 8, a_out, codes, iters=args.iters))
        one, dw, q = statistics.median(t_one), statistics.median(t_dw), statistics.median(t_q)
        emit({"layer": f"dw k{K} C{Cn} @{H}x{W}", "batch": B, "elements": n, "one_launch_median_ms": round(one, 5),
              "one_min": round(min(t_one), 5), "one_max": round(max(t_one), 5), "fp32_dwconv_median_ms": round(dw, 5),
              "quantiser_codes_median_ms": round(q, 5), "pair_ms": round(dw + q, 5), "pair_over_one": round((dw + q) / one, 3),
              "one_launch_GBps_at_6B": round(6.0 * n / (one * 1e-3) / 1e9, 1)})
        del xq, wq, x, w, y, z, codes

    # ---- (b) whole inference passes ----------------------------------------------------------------------------------------------
    T, F, classes = 101, 40, 10
    X = torch.randn((args.clips, T, F), device="cuda", generator=gen)
    yl = (torch.arange(args.clips, device="cuda") % classes).to(torch.int32)
    cfg = EvalConfig.preset("nsga_penalty", variant="A_ds", classes=classes, batch=64, early_stop=False,
                            quant=QuantConfig(bits=8), act_quant=ActQuantConfig(bits=8))
    for gene in GENES:
        with NetSession(gene, cfg, T, F, 0) as net:
            net.train_step(X, yl, None, 0, 64)
            net.train_step(X, yl, None, 64, 64)
            times = {"level1": [], "level2": []}
            for m in times:                                   # warm-up of both levels: code objects, first-use allocations
                net.set_int8(True, depthwise=(m == "level2"))
                net.predict_proba(X)
            for r in range(args.repeats):
                for m in times:
                    net.set_int8(True, depthwise=(m == "level2"))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    net.predict_proba(X)
                    e1.record()
                    torch.cuda.synchronize()
                    times[m].append(e0.elapsed_time(e1))
            med = {m: statistics.median(t) for m, t in times.items()}
            for m, t in times.items():
                line = {"gene": list(gene), "variant": "A_ds", "params": net.n_params, "int8": m, "clips": args.clips,
                        "median_predict_ms": round(med[m], 4), "min": round(min(t), 4), "max": round(max(t), 4),
                        "spread_pct": round(100.0 * (max(t) - min(t)) / med[m], 2)}
                if m == "level2":
                    line.update({"int8_ops": len(net.int8_ops()), "int8_dw_ops": len(net.int8_dw_ops()),
                                 "level1_over_level2": round(med["level1"] / med["level2"], 3),
                                 "faster_beyond_level1_spread": bool(med["level2"] < min(times["level1"]))})
                emit(line)

    # ---- (c) level 2 against level 1 on a fitted model (the A_ds model and data of int8_inference_parity.txt) -------------------------
    rs = np.random.RandomState(7)
    n_train, n_val = 1536, 512
    yy = rs.randint(0, classes, n_train + n_val).astype(np.int32)
    XX = (rs.randn(n_train + n_val, T, F) + yy[:, None, None] * 0.15).astype(np.float32)
    Xd, yd = torch.from_numpy(XX).cuda(), torch.from_numpy(yy).cuda()
    variant, gene = "A_ds", (16, 3, 1, 1, 2, 0)
    pcfg = EvalConfig.preset("nsga_penalty", variant=variant, classes=classes, batch=64, epochs=3, early_stop=False, n_slots=1,
                             quant=QuantConfig(bits=8), act_quant=ActQuantConfig(bits=8))
    model = PopulationEvaluator(Xd[:n_train], yd[:n_train], Xd[n_train:], yd[n_train:], pcfg).train_model(gene, 1)
    z1 = model.logits(Xd[n_train:], pcfg, int8=True)
    z2 = model.logits(Xd[n_train:], pcfg, int8=True, int8_depthwise=True)
    rep = model.int8_report(Xd[n_train:], yd[n_train:], pcfg, depthwise=True)
    emit({"gene": list(gene), "variant": variant, "epochs": 3, "bits": 8, "rows": int(z1.shape[0]),
          "level2_vs_level1_argmax_agree": float((z1.argmax(dim=1) == z2.argmax(dim=1)).float().mean().item()),
          "level2_vs_level1_max_abs_logit_diff": round(float((z1 - z2).abs().max().item()), 8),
          "level2_vs_fakequant": {k: (round(v, 8) if isinstance(v, float) else v) for k, v in rep.items()}})
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
