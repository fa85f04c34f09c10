#!/usr/bin/env python3
"""The resampler, measured against its bandwidth bound.

Three cases, all to 16 kHz with the default filter: one hour of 48 kHz audio (one row), one hour of 44.1 kHz audio (one
row), and 30 000 one-second 44.1 kHz clips.  Each reports the median and the runs of five cmoop_resample_time calls (3
warm-up launches, then --iters back-to-back launches between two HIP events, so that a timed window holds tens of
milliseconds), the bytes a row must move, 4 (L + n_out), the achieved GB/s and its fraction of the 6.3 TB/s achievable HBM
rate.  For context the recordings also report cmoop_logmel_stream_time of the resampled audio at the
default front end.  There is no earlier implementation to compare with: what is reported is the distance to the bound.
Writes the record to --out (profiles/resample_time.txt)."""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cmoop_audio_processing_amd import FrontendConfig, _lib  # noqa: E402
from cmoop_audio_processing_amd import resample as R  # noqa: E402

REPEATS = 5
HBM_ACHIEVABLE_GBS = 6300.0


def resample_case(name, n_clips, L, sr_in, sr_out, iters, stream_iters):
    up, down = R.rational(sr_in, sr_out)
    taps = R.resample_filter(up, down)
    n_out, tile, n_tiles, tpp = R.resample_plan(L, up, down, taps.size)
    wav = 0.3 * torch.randn((n_clips, L), device="cuda")
    out = torch.empty((n_clips, n_out), device="cuda")
    ms = C.c_double()
    torch.cuda.synchronize()
    runs = []
    for _ in range(REPEATS):
        _lib.check(_lib.lib().cmoop_resample_time(_lib.ptr(wav), C.c_int64(n_clips), C.c_int64(L), C.c_int32(up), C.c_int32(down),
                                                  _lib.ptr(taps), C.c_int32(taps.size), _lib.ptr(out), C.c_int32(iters), C.byref(ms)))
        runs.append(ms.value)
    med = statistics.median(runs)
    moved = 4 * n_clips * (L + n_out)
    gbs = moved / (med * 1e-3) / 1e9
    lines = [f"{name}",
             f"  rows {n_clips}, L {L}, n_out {n_out}, up/down {up}/{down}, taps {taps.size}, taps per output {tpp}, tile {tile}, "
             f"workgroup tiles {n_clips * n_tiles}",
             f"  resample ms: median {med:.4f}, runs {[round(v, 4) for v in runs]} ({iters} launches per run)",
             f"  bytes moved 4 (L + n_out) per row: {moved} ({moved / 1e6:.1f} MB); FMA {tpp * n_out * n_clips / 1e9:.3f} G",
             f"  {gbs:.1f} GB/s = {gbs / HBM_ACHIEVABLE_GBS:.3f} of the {HBM_ACHIEVABLE_GBS / 1000:.1f} TB/s achievable HBM rate; "
             f"bound {moved / (HBM_ACHIEVABLE_GBS * 1e9) * 1e3:.4f} ms"]
    if n_clips == 1:
        cfg = FrontendConfig(sr=sr_out)
        feat = torch.empty((cfg.frames(n_out), cfg.n_mels), device="cuda")
        st, sruns = cfg._struct(), []
        for _ in range(REPEATS):
            _lib.check(_lib.lib().cmoop_logmel_stream_time(C.byref(st), _lib.ptr(out), C.c_int64(n_out), _lib.ptr(feat),
                                                           C.c_int32(stream_iters), C.byref(ms)))
            sruns.append(ms.value)
        lines.append(f"  for context, log_mel_stream of the resampled recording: median {statistics.median(sruns):.4f} ms, "
                     f"runs {[round(v, 4) for v in sruns]} ({stream_iters} launches per run)")
    del wav, out
    torch.cuda.empty_cache()
    for ln in lines:
        print(ln, flush=True)
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--clip-iters", type=int, default=10)
    ap.add_argument("--stream-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_time.txt"))
    a = ap.parse_args()
    lines = [f"tools/resample_bench.py on {torch.cuda.get_device_name(0)}: cmoop_resample_time, default filter, {REPEATS} runs per case", ""]
    lines += resample_case("one hour of 48 kHz audio -> 16 kHz", 1, 3600 * 48000, 48000, 16000, a.iters, a.stream_iters) + [""]
    lines += resample_case("one hour of 44.1 kHz audio -> 16 kHz", 1, 3600 * 44100, 44100, 16000, a.iters, a.stream_iters) + [""]
    lines += resample_case("30 000 one-second 44.1 kHz clips -> 16 kHz", 30000, 44100, 44100, 16000, a.clip_iters, a.stream_iters)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
