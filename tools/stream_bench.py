#!/usr/bin/env python3
"""Recording scoring, measured: the stream front end against the clip call on ONE long recording, and predict_stream.

Front end: 60 s and 600 s of 16 kHz noise at the default config, 60 s of 32 kHz noise at the birdclef_128 geometry in log
scale.  Each case reports the median of five cmoop_logmel_stream_time runs and the median and minimum of five
cmoop_logmel_ex_time runs on the same waveform passed as one clip (that call launches one workgroup per clip; both calls
take 3 warm-up launches and average the launches between two HIP events: --iters back-to-back launches of the stream
call, --clip-iters of the much longer clip call, so that every timed window holds milliseconds of work).

Scoring: windows per second of NetSession.predict_stream at hop_frames = 10 on the 101 x 40 features of the 16 kHz
recordings, for the cheapest and the heaviest gene, and the real-time factor: seconds of audio per second of GPU, front
end included.  Writes profiles/stream_bench.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from cmoop_audio_processing_amd import EvalConfig, FrontendConfig, _lib, log_mel_stream  # noqa: E402
from cmoop_audio_processing_amd.session import NetSession  # noqa: E402

REPEATS = 5


def frontend_case(name, cfg, seconds, iters, clip_iters):
    L = int(seconds * cfg.sr)
    wav = 0.3 * torch.randn(L, device="cuda")
    out = torch.empty((cfg.frames(L), cfg.n_mels), device="cuda")
    st, ms = cfg._struct(), C.c_double()
    torch.cuda.synchronize()
    stream_ms, clip_ms = [], []
    for _ in range(REPEATS):
        _lib.check(_lib.lib().cmoop_logmel_stream_time(C.byref(st), _lib.ptr(wav), C.c_int64(L), _lib.ptr(out), C.c_int32(iters), C.byref(ms)))
        stream_ms.append(ms.value)
    for _ in range(REPEATS):
        _lib.check(_lib.lib().cmoop_logmel_ex_time(C.byref(st), _lib.ptr(wav), C.c_int64(1), C.c_int32(L), _lib.ptr(out),
                                                   C.c_int32(clip_iters), C.byref(ms)))
        clip_ms.append(ms.value)
    rec = {"case": name, "audio_seconds": seconds, "sr": cfg.sr, "frames": int(out.shape[0]), "n_mels": cfg.n_mels,
           "stream_ms_median": round(statistics.median(stream_ms), 4), "stream_ms_runs": [round(v, 4) for v in stream_ms],
           "clip_ms_median": round(statistics.median(clip_ms), 4), "clip_ms_min": round(min(clip_ms), 4),
           "clip_ms_runs": [round(v, 4) for v in clip_ms],
           "clip_min_over_stream_median": round(min(clip_ms) / statistics.median(stream_ms), 2),
           "stream_below_clip_min": statistics.median(stream_ms) < min(clip_ms)}
    print(json.dumps(rec), flush=True)
    return rec


def scoring_case(name, gene, variant, seconds, hop_frames, frontend_ms, eval_batch):
    cfg, fcfg = EvalConfig(variant=variant, classes=10, eval_batch=eval_batch), FrontendConfig()
    wav = 0.3 * torch.randn(int(seconds * fcfg.sr), device="cuda")
    feat = log_mel_stream(wav, fcfg)
    with NetSession(gene, cfg, 101, 40, 1) as net:
        probs = net.predict_stream(feat, hop_frames)              # warm-up: allocations, first launches
        t0 = time.perf_counter()
        probs = net.predict_stream(feat, hop_frames)
        calls = max(1, int(0.05 / max(time.perf_counter() - t0, 1e-6)))     # at least ~50 ms of work per timing
        runs = []
        for _ in range(REPEATS):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(calls):
                probs = net.predict_stream(feat, hop_frames)      # returns after the library's stream has drained
            runs.append((time.perf_counter() - t0) / calls)
    s = statistics.median(runs)
    rec = {"case": name, "gene": list(gene), "variant": variant, "audio_seconds": seconds, "hop_frames": hop_frames,
           "eval_batch": eval_batch, "windows": int(probs.shape[0]), "calls_per_timing": calls, "predict_stream_s_median": round(s, 5),
           "predict_stream_s_runs": [round(v, 5) for v in runs], "windows_per_s": round(int(probs.shape[0]) / s, 1),
           "frontend_ms": frontend_ms, "real_time_factor": round(seconds / (s + frontend_ms * 1e-3), 1)}
    print(json.dumps(rec), flush=True)
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--clip-iters", type=int, default=10)
    ap.add_argument("--eval-batch", type=int, default=256)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "stream_bench.json"))
    a = ap.parse_args()
    gsc = FrontendConfig()
    bird = FrontendConfig(sr=32000, n_fft=2048, win=2048, hop=512, n_mels=128, fmin=20.0, fmax=16000.0, scale="log")
    fe = [frontend_case("60 s, 16 kHz, default config (512-point kernel)", gsc, 60, a.iters, a.clip_iters),
          frontend_case("600 s, 16 kHz, default config (512-point kernel)", gsc, 600, a.iters, a.clip_iters),
          frontend_case("60 s, 32 kHz, birdclef_128 geometry, log scale (general kernel)", bird, 60, a.iters, a.clip_iters)]
    sc = []
    for seconds, fms in ((60, fe[0]["stream_ms_median"]), (600, fe[1]["stream_ms_median"])):
        sc.append(scoring_case(f"cheapest gene, {seconds} s", (16, 3, 0, 1, 1, 0), "B", seconds, 10, fms, a.eval_batch))
        sc.append(scoring_case(f"heaviest gene, {seconds} s", (64, 5, 1, 3, 4, 1), "A", seconds, 10, fms, a.eval_batch))
    rec = {"device": torch.cuda.get_device_name(0), "stream_launches_per_timing": a.iters, "clip_launches_per_timing": a.clip_iters, "repeats": REPEATS, "frontend": fe, "scoring": sc}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    if not all(r["stream_below_clip_min"] for r in fe if r["audio_seconds"] == 60):
        print("stream front end is NOT below the clip call's minimum on a 60 s recording: the grid is wrong", file=sys.stderr)
        sys.exit(1)


if __name__ == "__main__":
    main()
