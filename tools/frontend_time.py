#!/usr/bin/env python3
"""HIP-event timing of the front end's kernels (cmoop_logmel_ex_time: 3 warm-up launches, then the average of --iters
launches between two events on the library's stream) with the share of the HBM roofline, taking clip bytes in plus feature
bytes out as the algorithmic bytes.  Cases: 4 096 clips at the birdclef_128 preset, 30 000 one-second clips at the default
geometry with 80 mel bands (general kernel), and the same clips at the default geometry (the 512-point kernel)."""
import argparse
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from cmoop_audio_processing_amd import FrontendConfig, _lib  # noqa: E402

HBM_PEAK = 8.0e12      # B/s, MI355X specification


def time_case(name, cfg, n_clips, n_samples, iters):
    wav = torch.randn((n_clips, n_samples), device="cuda")
    out = torch.empty((n_clips, cfg.frames(n_samples), cfg.n_mels), device="cuda")
    st, ms = cfg._struct(), C.c_double()
    torch.cuda.synchronize()
    _lib.check(_lib.lib().cmoop_logmel_ex_time(C.byref(st), _lib.ptr(wav), C.c_int64(n_clips), C.c_int32(n_samples), _lib.ptr(out),
                                               C.c_int32(iters), C.byref(ms)))
    nbytes = 4 * (wav.numel() + out.numel())
    rec = {"case": name, "n_clips": n_clips, "n_samples": n_samples, "out_shape": list(out.shape[1:]), "ms": round(ms.value, 4),
           "algorithmic_GB": round(nbytes / 1e9, 4), "TB_per_s": round(nbytes / (ms.value * 1e-3) / 1e12, 4),
           "share_of_hbm_roofline": round(nbytes / (ms.value * 1e-3) / HBM_PEAK, 4)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    gsc = FrontendConfig()
    time_case("birdclef_128 (general kernel, n_fft 2048, 128 mels, dB)", FrontendConfig.preset("birdclef_128"), 4096, 65280, a.iters)
    time_case("gsc geometry with 80 mels (general kernel, n_fft 512)", FrontendConfig(n_mels=80), 30000, 16000, a.iters)
    time_case("gsc geometry (512-point kernel)", gsc, 30000, 16000, a.iters)
    time_case("gsc geometry with 64 mels (512-point kernel)", FrontendConfig(n_mels=64), 30000, 16000, a.iters)


if __name__ == "__main__":
    main()
