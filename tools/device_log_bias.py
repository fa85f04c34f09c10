#!/usr/bin/env python3
"""Signed error of the device's float32 log and exp against float64, in ulps of the result: the measurement behind the
double-precision logarithms of softmax_ce_kernel<CE_DISTILL> (csrc/loss.hip), recorded in profiles/distill_logf_bias.txt.

  python tools/device_log_bias.py

torch's float32 log / exp kernels on the GPU call the device math library the HIP kernels of this project link.  A mean
signed error away from zero matters where a kernel adds several logarithms with the same sign and then scales a small
difference of them, as the KL term of the distillation loss does (sum q log q + log seT - sum q x, times T^2).
"""
import numpy as np
import torch


def ulps(got, ref):
    ref, got = np.asarray(ref, np.float64), np.asarray(got, np.float64)
    u = 2.0 ** (np.floor(np.log2(np.abs(ref) + 1e-300)) - 23)
    e = (got - ref) / u
    return f"mean {e.mean():+.3f} ulp, mean |.| {np.abs(e).mean():.3f} ulp, max |.| {np.abs(e).max():.2f} ulp"


def main():
    if not torch.cuda.is_available():
        raise SystemExit("device_log_bias needs a GPU")
    for name, fn, ref, lo, hi in (("log", torch.log, np.log, 0.01, 1.0), ("log", torch.log, np.log, 1.0, 40.0),
                                  ("exp", torch.exp, np.exp, -3.0, 0.0)):
        x = torch.linspace(lo, hi, 100001, device="cuda", dtype=torch.float32)
        print(f"float32 {name} on [{lo}, {hi}], 100001 points: {ulps(fn(x).cpu().numpy(), ref(x.cpu().numpy().astype(np.float64)))}")


if __name__ == "__main__":
    main()
