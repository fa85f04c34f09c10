#!/usr/bin/env python3
"""What the third level of integer inference (the requantising epilogue) costs or gains.

  python tools/int8_fused_time.py [--repeats 7] [--iters 50] [--out profiles/int8_fused_time.txt]

The protocol of tools/int8_depthwise_time.py: ``iters`` back-to-back launches between two HIP events, median of ``repeats``
windows, the sides alternating within a repeat in one process.
(a) Lone layers at batch 256 on the fusible shapes of genes (64, 5, 1, 3, 4, 1) and (64, 5, 0, 3, 4, 1), once each with and
    without BatchNorm, and the 512 -> 256 dense layer: the ONE launch (``cmoop_conv_fwd_i8_q_time`` / ``cmoop_dense_fwd_i8_q_time``)
    against the CHAIN it replaces -- the i8 launch (``cmoop_conv_fwd_i8_time`` / ``cmoop_dense_fwd_i8_time``), with BatchNorm the
    apply launch (``cmoop_scale_shift_time``), and the tracked quantiser with codes (``cmoop_fake_quant_act_codes_time``), each
    timed alone and added.
(b) ``predict_proba`` of 4096 clips at 101x40: ONE NetSession per candidate, level 1 against level 1 + fused on A
    (64, 5, 1, 3, 4, 1) and A (16, 3, 1, 1, 1, 1); level 2 against level 2 + fused on A_ds (64, 5, 1, 3, 4, 1).  The logits of
    the two sides are compared in bytes as well.
No threshold is fixed here: the recorded value is the claim.
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVS = [(51, 20, 64, 128, 5), (26, 10, 128, 256, 5), (13, 5, 256, 512, 5)]      # (H, W, Cin, Cout, KS): res*_conv1
DENSE = (512, 256)                                                                # (K, N): fc1 -> fc2 of the fc = 4 ladder
NETS = [("A", (64, 5, 1, 3, 4, 1), False), ("A", (16, 3, 1, 1, 1, 1), False), ("A_ds", (64, 5, 1, 3, 4, 1), True)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50, help="launches per timed window of a lone layer")
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--clips", type=int, default=4096)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_fused_time.txt"))
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    from cmoop_audio_processing_amd import ActQuantConfig, EvalConfig, QuantConfig
    from cmoop_audio_processing_amd import quant as Q
    from cmoop_audio_processing_amd.session import NetSession
    if not torch.cuda.is_available():
        raise SystemExit("int8_fused_time needs a GPU: there is nothing to time without one")
    torch.cuda.set_device(0)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    lines = []

    def emit(d):
        lines.append(json.dumps(d))
        print(lines[-1], flush=True)

    def codes(n):
        return torch.randint(-127, 128, (n,), device="cuda", generator=gen, dtype=torch.int32).to(torch.int8)

    # ---- (a) lone layers: one launch against the chain it replaces ---------------------------------------------------------------
    B, it = args.batch, args.iters
    layers = [("conv",) + c for c in CONVS] + [("dense", 1, 1) + DENSE + (1,)]
    for kind, H, W, Cin, Cout, KS in layers:
        M, K = B * H * W, KS * KS * Cin
        n = M * Cout
        xq, wq = codes(M * Cin), codes(Cout * K)
        s_x = 0.02
        s_w, bias = torch.full((Cout,), 0.01, device="cuda"), torch.randn((Cout,), device="cuda", generator=gen)
        scale = torch.rand((Cout,), device="cuda", generator=gen) + 0.5
        shift = torch.randn((Cout,), device="cuda", generator=gen)
        y, z, q = torch.empty(n, device="cuda"), torch.empty(n, device="cuda"), torch.empty(n, device="cuda", dtype=torch.int8)
        a_out = float(0.5 * 127 * 127 * (K ** 0.5) * s_x * 0.01)          # a few standard deviations of the sums: some clamp
        for bn in (1, 0):
            relu, relu_after = (0, 1) if bn else (1, 0)                   # the tails of the two genes
            kw = dict(bn_scale=scale, bn_shift=shift, relu_after=relu_after) if bn else {}
            t_one, t_i8, t_ss, t_q = [], [], [], []
            for _ in range(args.repeats):
                if kind == "conv":
                    t_one.append(Q.conv_fwd_i8_q_time(xq, wq, s_x, s_w, bias, y, q, B, H, W, Cin, Cout, KS, 1, relu, 8, a_out, iters=it, **kw))
                    t_i8.append(Q.conv_fwd_i8_time(xq, wq, s_x, s_w, bias, y, B, H, W, Cin, Cout, KS, 1, relu, iters=it))
                else:
                    t_one.append(Q.dense_fwd_i8_q_time(xq, wq, s_x, s_w, bias, y, q, M, Cout, K, relu, 8, a_out, iters=it, **kw))
                    t_i8.append(Q.dense_fwd_i8_time(xq, wq, s_x, s_w, bias, y, M, Cout, K, relu, iters=it))
                t_ss.append(Q.scale_shift_time(y, z, scale, shift, M, Cout, relu_after, iters=it) if bn else 0.0)
                t_q.append(Q.fake_quant_act_codes_time(z if bn else y, 8, a_out, q, iters=it))
            one, i8, ss, qq = (statistics.median(t) for t in (t_one, t_i8, t_ss, t_q))
            chain = i8 + ss + qq
            name = f"conv {Cin}->{Cout} k{KS} @{H}x{W}" if kind == "conv" else f"dense {K}->{Cout}"
            emit({"layer": name, "batch": B, "batchnorm": bool(bn), "elements": n, "fused_median_ms": round(one, 5),
                  "fused_min": round(min(t_one), 5), "fused_max": round(max(t_one), 5), "i8_median_ms": round(i8, 5),
                  "scale_shift_median_ms": round(ss, 5), "quantiser_codes_median_ms": round(qq, 5), "chain_ms": round(chain, 5),
                  "chain_over_fused": round(chain / one, 3), "fused_slower_than_chain": bool(one > chain)})
        del xq, wq, y, z, q

    # ---- (b) whole inference passes ----------------------------------------------------------------------------------------------
    T, F, classes = 101, 40, 10
    X = torch.randn((args.clips, T, F), device="cuda", generator=gen)
    yl = (torch.arange(args.clips, device="cuda") % classes).to(torch.int32)
    for variant, gene, dw in NETS:
        cfg = EvalConfig.preset("nsga_penalty", variant=variant, classes=classes, batch=64, early_stop=False,
                                quant=QuantConfig(bits=8), act_quant=ActQuantConfig(bits=8))
        with NetSession(gene, cfg, T, F, 0) as net:
            net.train_step(X, yl, None, 0, 64)
            net.train_step(X, yl, None, 64, 64)
            times, probs = {"base": [], "fused": []}, {}
            for m in times:                                   # warm-up of both sides: code objects, first-use allocations
                net.set_int8(True, depthwise=dw, fused=(m == "fused"))
                probs[m] = net.predict_proba(X).cpu().numpy().tobytes()
            for _ in range(args.repeats):
                for m in times:
                    net.set_int8(True, depthwise=dw, fused=(m == "fused"))
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    torch.cuda.synchronize()
                    e0.record()
                    net.predict_proba(X)
                    e1.record()
                    torch.cuda.synchronize()
                    times[m].append(e0.elapsed_time(e1))
            med = {m: statistics.median(t) for m, t in times.items()}
            base = "level2" if dw else "level1"
            for m, t in times.items():
                line = {"gene": list(gene), "variant": variant, "params": net.n_params, "int8": base + ("+fused" if m == "fused" else ""),
                        "clips": args.clips, "median_predict_ms": round(med[m], 4), "min": round(min(t), 4), "max": round(max(t), 4),
                        "spread_pct": round(100.0 * (max(t) - min(t)) / med[m], 2)}
                if m == "fused":
                    line.update({"int8_ops": len(net.int8_ops()), "int8_fused_ops": len(net.int8_fused_ops()),
                                 "base_over_fused": round(med["base"] / med["fused"], 3),
                                 "faster_beyond_base_spread": bool(med["fused"] < min(times["base"])),
                                 "probabilities_equal_in_bytes": probs["base"] == probs["fused"]})
                emit(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
