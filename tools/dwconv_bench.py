#!/usr/bin/env python3
"""Time the three depthwise-convolution kernels alone (csrc/dwconv.hip) and hold them against the HBM roofline.

    python tools/dwconv_bench.py [--iters 50] [--out profiles/dwconv_kernel_bench.txt]

Each kernel is launched `iters` times back to back on the library stream between two HIP events, after three warm-up
launches (cmoop_dwconv_time).  Algorithmic bytes: forward and data gradient read the tensor once and write it once (the
data gradient's x > 0 mask is a second read, listed separately), the weight gradient reads x and dY once each; weights and
partials are negligible.  The roofline is the measured 6.29 TB/s of a float4 copy on an MI355X (8.0 TB/s on paper).  The
smaller tensors here (a few MB) fit the 256 MiB Infinity Cache, so their figures are cache-resident ones: a fraction above
1 means the launch never went to HBM, not that it beat it."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmoop_audio_processing_amd import _lib  # noqa: E402

GEOMETRIES = [(64, 101, 40, 64, 5), (64, 51, 20, 128, 5), (64, 26, 10, 256, 3), (64, 13, 5, 512, 3)]
HBM_MEASURED, HBM_PEAK = 6.29e12, 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    L = _lib.lib()
    lines = [f"# tools/dwconv_bench.py --iters {a.iters} on {torch.cuda.get_device_name(0)}",
             "# roofline: fraction of 6.29 TB/s (measured float4 copy); in brackets of the 8.0 TB/s peak",
             f"{'B,H,W,C,K':>20} {'kernel':>8} {'slices':>6} {'ms':>9} {'MB':>8} {'GB/s':>8} {'of HBM':>14}"]
    for (B, H, W, Cn, K) in GEOMETRIES:
        g = torch.Generator(device="cuda").manual_seed(1)
        x = torch.randn((B, H, W, Cn), device="cuda", generator=g)
        dy = torch.randn((B, H, W, Cn), device="cuda", generator=g)
        w = torch.randn((K, K, Cn), device="cuda", generator=g)
        out = torch.empty_like(x)
        tensor = x.numel() * 4
        torch.cuda.synchronize()
        for mode, name, nbytes in ((0, "fwd", 2 * tensor), (1, "dgrad", 2 * tensor), (2, "wgrad", 2 * tensor)):
            ms = C.c_double()
            _lib.check(L.cmoop_dwconv_time(mode, _lib.ptr(x), _lib.ptr(w), _lib.ptr(dy), _lib.ptr(out), B, H, W, Cn, K, a.iters, C.byref(ms)))
            rate = nbytes / (ms.value * 1e-3)
            s = _lib.dwconv_wgrad_slices(B, H, W, Cn, K) if mode == 2 else 0
            lines.append(f"{str((B, H, W, Cn, K)):>20} {name:>8} {s or '-':>6} {ms.value:9.4f} {nbytes / 1e6:8.2f} {rate / 1e9:8.0f} "
                         f"{rate / HBM_MEASURED:7.2f} ({rate / HBM_PEAK:.2f})")
    lines.append("# dgrad: timed with the x > 0 mask, whose read of x is a third tensor pass not counted in MB")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
