#!/usr/bin/env python3
"""Where the integer and the fake-quantised pass part on the row with the largest logit difference.

  python tools/int8_logit_trace.py [--out profiles/int8_inference_parity_trace.txt]

Fits the variant-B model of tools/int8_inference_time.py's parity leg (same seeds), scores its validation split both ways,
takes the row with the largest |delta logit|, scores the eval_batch chunk that row was scored in again (the same batch: the same
launches) and compares every act of that row: elements that differ, the largest difference and, at the activation-quantisation
sites, how many int8 codes differ and by how many steps.  A reported record, no gate.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
ap = argparse.ArgumentParser()
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "int8_inference_parity_trace.txt"))
args = ap.parse_args()
from cmoop_audio_processing_amd import ActQuantConfig, EvalConfig, PopulationEvaluator, QuantConfig, quant as Q
T, F, classes = 101, 40, 10
rs = np.random.RandomState(7)
n_train, n_val = 1536, 512
yy = rs.randint(0, classes, n_train + n_val).astype(np.int32)
XX = (rs.randn(n_train + n_val, T, F) + yy[:, None, None] * 0.15).astype(np.float32)
Xd, yd = torch.from_numpy(XX).cuda(), torch.from_numpy(yy).cuda()
variant, gene = "B", (32, 5, 0, 2, 3, 1)
pcfg = EvalConfig.preset("nsga_penalty", variant=variant, classes=classes, batch=64, epochs=3, early_stop=False, n_slots=1,
                         quant=QuantConfig(bits=8), act_quant=ActQuantConfig(bits=8))
model = PopulationEvaluator(Xd[:n_train], yd[:n_train], Xd[n_train:], yd[n_train:], pcfg).train_model(gene, 1)
Xv = Xd[n_train:]
out = []
with model.session(pcfg, int8=True) as net:
    zi = net.predict_logits(Xv).cpu().numpy()
    net.set_int8(False)
    zf = net.predict_logits(Xv).cpu().numpy()
    d = np.abs(zi - zf).max(axis=1)
    row = int(d.argmax())
    out.append({"rows": len(d), "max_abs_logit_diff": float(d.max()), "worst_row": row, "rows_above_1e-4": int((d > 1e-4).sum()),
                "median_row_diff": float(np.median(d))})
    sites = {s[0]: k for k, s in enumerate(Q.act_sites(gene, variant, classes, T, F))}
    rec = net.get_act_ranges()
    eb = int(pcfg.eval_batch)
    c0 = row // eb * eb
    x1 = Xv[c0:c0 + eb].contiguous()          # the chunk the row was scored in: the same batch, the same launches
    nb, rr = int(x1.shape[0]), row - c0
    out[0].update({"eval_batch": eb, "chunk_rows": nb, "row_in_chunk": rr})
    n_acts = net.act_dims(0)[5]
    acts = {}
    for mode in (True, False):
        net.set_int8(mode)
        net.predict_logits(x1)
        acts[mode] = {i: net.get_act(i, nb)[rr:rr + 1] for i in range(1, n_acts) if net.act_dims(i)[3]}
    for i in sorted(acts[True]):
        a, b = acts[True][i], acts[False][i]
        line = {"act": i, "shape": list(a.shape[1:]), "differing": int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum()),
                "max_abs_diff": float(np.abs(a - b).max()), "absmax": float(np.abs(b).max())}
        if i in sites:
            r = rec["r"][sites[i]]
            qa, qb = Q.act_codes_ref(a, 8, r).astype(np.int32), Q.act_codes_ref(b, 8, r).astype(np.int32)
            line.update({"site": sites[i], "scale": float(Q.act_scale_ref(r, 8)), "codes_differing": int((qa != qb).sum()),
                         "max_code_step": int(np.abs(qa - qb).max())})
        out.append(line)
os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
with open(args.out, "w") as f:
    for l in out:
        f.write(json.dumps(l) + "\n")
        print(json.dumps(l))
