"""Front-end parity on structured signals: configs, signals, a float64 reference and a derived per-element error budget.

Shared by tests/test_frontend_bound_cpu.py (the budget is neither flaky nor vacuous), tests/test_gpu_frontend_fixed_kernel.py
(the 512-point kernel away from its default config) and tests/test_gpu_frontend_config.py (the general kernel).  Everything
here runs on the CPU; the only reference is oracle/frontend.py.

Why a budget and not a flat gate.  A flat 2e-4 on the log is usable on broadband inputs only: for a pure tone the float32
error in the far bands is comparable to log_eps, so a flat gate there is either wrong or vacuous.  With u = 2^-24,
N = n_fft, fr[t] the windowed frame, X its spectrum, S = |X|^2 @ fb.T, y = log(S + eps) and cnt[m] the number of non-zero
bins of band m:

    e[t]    = 8 u log2(N) sqrt(N) ||fr[t]||_2
    B[t,m]  = sum_k fb[m,k] (2 |X[t,k]| e[t] + e[t]^2)  +  (cnt[m] + 4) u S[t,m]
    rho     = (B + u (S + eps)) / (S + eps)
    by[t,m] = -log1p(-rho) + 4 u |y[t,m]|        where rho < 0.5; otherwise the element is excused

* 8 u log2 N: Higham, Accuracy and Stability of Numerical Algorithms, Thm 24.2 -- eta ~ u + gamma_4 sqrt(2) ~ 6.7 u per
  radix-2 stage with correctly rounded twiddles (radix 4 and the real split have no more stages), one more u for the window
  product.  sqrt(N) turns the 2-norm bound on the spectrum error into a per-bin bound.
* (cnt + 4) u S: the serial fmaf sum of cnt non-negative terms, plus the square and the add.
* u (S + eps) and 4 u |y|: acc + eps and logf.
B alone bounds the mel power (scale="power"); by bounds the log.  No element of the eight FIXED_CONFIGS below has
rho >= 0.5 on any signal (asserted); where one does elsewhere -- log_eps 1e-10, far bands of DC at n_fft 1024 -- it is held
to excused_window, the same budget without the symmetric linearisation.

The float32 restatement and its four perturbations exist for the CPU test only: the restatement must sit inside the budget
(not flaky), each perturbation must leave it (not vacuous).
"""
import functools
import os

import numpy as np

from oracle import frontend as ofe

U = 2.0 ** -24

# name -> (FrontendConfig fields, clip length); all n_fft 512, log scale, <= 64 mels: the 512-point register-FFT kernel
FIXED_CONFIGS = {
    "m64": (dict(sr=16000, n_fft=512, win=400, hop=160, n_mels=64, fmin=20.0, fmax=7600.0), 1603),
    "m63": (dict(sr=16000, n_fft=512, win=400, hop=160, n_mels=63, fmin=20.0, fmax=7600.0), 1603),
    "m1": (dict(sr=16000, n_fft=512, win=512, hop=256, n_mels=1, fmin=0.0, fmax=8000.0), 1603),
    "m2": (dict(sr=16000, n_fft=512, win=512, hop=256, n_mels=2, fmin=0.0, fmax=8000.0), 1603),
    "tel": (dict(sr=8000, n_fft=512, win=512, hop=512, n_mels=24, fmin=0.0, fmax=4000.0), 2049),
    "gap48": (dict(sr=48000, n_fft=512, win=255, hop=700, n_mels=64, fmin=0.0, fmax=24000.0), 4201),
    "hop1": (dict(sr=16000, n_fft=512, win=3, hop=1, n_mels=40, fmin=20.0, fmax=7600.0), 70),
    "narrow": (dict(sr=16000, n_fft=512, win=400, hop=160, n_mels=32, fmin=3000.0, fmax=3500.0), 1603),
}

# name -> (empty bands, one-bin bands, widest band in bins, lane splits = min(64 - n_mels, #bands with cnt >= 8))
BAND_STATS = {
    "m64": (0, 0, 22, 0),
    "m63": (0, 0, 22, 1),
    "m1": (0, 0, 255, 1),
    "m2": (0, 0, 223, 2),
    "tel": (0, 0, 45, 24),
    "gap48": (0, 13, 32, 0),
    "hop1": (0, 0, 34, 21),
    "narrow": (2, 30, 1, 0),
}

FAMILIES = ("tone", "imp", "dc", "nyq", "tiny", "loud", "noise", "zero")


def family(name):
    return "tone" if name.startswith("tone") else "imp" if name.startswith("imp") else name


def impulse_positions(L, hop):
    return [0, 1, min(L - 1, hop - 1), (L // 2) | 1, L - 1]


def make_signals(geo, L, seed=20):
    """(names, wav float32 [13, L]): two tones, five impulses (named by position; hop 1 repeats imp0), DC, the Nyquist
    alternation, very quiet, very loud and plain noise, silence."""
    sr, n_fft, hop = geo["sr"], geo["n_fft"], geo["hop"]
    rs = np.random.RandomState(seed)
    t = np.arange(L) / float(sr)
    names, rows = [], []

    def add(name, row):
        names.append(name)
        rows.append(np.asarray(row, np.float64))

    add("tone_bin", 0.5 * np.sin(2 * np.pi * 37.0 * sr / n_fft * t))
    add("tone_off", 0.5 * np.sin(2 * np.pi * 37.5 * sr / n_fft * t + 0.3))
    for p in impulse_positions(L, hop):
        row = np.zeros(L)
        row[p] = 1.0
        add(f"imp{p}", row)
    add("dc", np.ones(L))
    add("nyq", 1.0 - 2.0 * (np.arange(L) % 2))
    add("tiny", 1e-5 * rs.randn(L))
    add("loud", 1e3 * rs.randn(L))
    add("noise", 0.3 * rs.randn(L))
    add("zero", np.zeros(L))
    assert len(names) == 13
    return names, np.stack(rows).astype(np.float32)


def eps_of(log_eps):
    return float(np.float32(log_eps))                              # the value the kernel adds


def reference(wav, geo, log_eps=1e-6):
    """float64, from the oracle's window and mel basis and np.fft.rfft: dict of fr [n, T, N], X [n, T, N/2+1], S and
    y [n, T, n_mels], fb [n_mels, N/2+1] and eps."""
    w64 = np.asarray(wav, np.float64)
    n_fft, hop = geo["n_fft"], geo["hop"]
    T = 1 + w64.shape[1] // hop
    x = np.pad(w64, ((0, 0), (n_fft // 2, n_fft // 2)))
    win = ofe.hann_padded(geo["win"], n_fft)
    fb = ofe.mel_filterbank(geo["sr"], n_fft, geo["n_mels"], geo["fmin"], geo["fmax"])
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :]
    fr = x[:, idx] * win[None, None, :]
    X = np.fft.rfft(fr, axis=-1)
    S = (np.abs(X) ** 2) @ fb.T
    eps = eps_of(log_eps)
    return dict(fr=fr, X=X, S=S, y=np.log(S + eps), fb=fb, eps=eps)


def budget(ref, n_fft):
    """(B, rho, by) of the module docstring; by is inf where rho >= 0.5 (the element would be excused)."""
    fr, X, S, y, fb, eps = (ref[k] for k in ("fr", "X", "S", "y", "fb", "eps"))
    e = 8.0 * U * np.log2(n_fft) * np.sqrt(n_fft) * np.linalg.norm(fr, axis=-1)       # [n, T]
    cnt = (fb != 0).sum(axis=1)
    B = (2.0 * np.abs(X) * e[..., None] + (e ** 2)[..., None]) @ fb.T + (cnt + 4) * U * S
    rho = (B + U * (S + eps)) / (S + eps)
    with np.errstate(divide="ignore", invalid="ignore"):
        by = np.where(rho < 0.5, -np.log1p(-np.minimum(rho, 0.5)) + 4.0 * U * np.abs(y), np.inf)
    return B, rho, by


def excused_window(ref, bud):
    """(lo, hi) for the log output where rho >= 0.5 and by does not apply (a log_eps far below the float32 noise floor of
    the spectrum, a far band of a tone): the same budget without the symmetric linearisation.  The mel sum is a sum of
    non-negative terms, so fl(acc + eps) >= eps whatever the spectrum's error: lo = log(max(eps, S + eps - B')),
    hi = log(S + eps + B') with B' = B + u (S + eps), each widened by logf's 4 u |.|."""
    S, eps = ref["S"], ref["eps"]
    Bp = bud[0] + U * (S + eps)
    lo, hi = np.log(np.maximum(eps, S + eps - Bp)), np.log(S + eps + Bp)
    return lo - 4.0 * U * np.abs(lo), hi + 4.0 * U * np.abs(hi)


@functools.lru_cache(maxsize=None)
def fixed_case(name, log_eps=1e-6):
    """(geo, L, names, wav, reference, (B, rho, by)) of one fixed-kernel config -- computed once, never modified."""
    geo, L = FIXED_CONFIGS[name]
    return (geo, L) + _case(tuple(sorted(geo.items())), L, log_eps)


@functools.lru_cache(maxsize=None)
def _case(geo_items, L, log_eps):
    geo = dict(geo_items)
    names, wav = make_signals(geo, L)
    ref = reference(wav, geo, log_eps)
    bud = budget(ref, geo["n_fft"])
    for a in (wav,) + tuple(v for v in ref.values() if isinstance(v, np.ndarray)) + bud:
        a.setflags(write=False)
    return tuple(names), wav, ref, bud


def case(geo, L, log_eps=1e-6):
    """(names, wav, reference, (B, rho, by)) for any geometry and clip length, cached."""
    return _case(tuple(sorted(geo.items())), L, log_eps)


def worst_ratios(err, by, names):
    """{family: max err / by} over the rows of each signal family; by == 0 cannot occur (4 u |y| > 0 unless y == 0)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(by > 0, err / by, np.where(err > 0, np.inf, 0.0))
    out = {}
    for i, n in enumerate(names):
        f = family(n)
        out[f] = max(out.get(f, 0.0), float(ratio[i].max()))
    return out


def record(line):
    """Print a measured figure; with CMOOP_FRONTEND_BOUND_FILE set, append it to that file too (profiles/frontend_bound.txt
    is one such run)."""
    print(line)
    path = os.environ.get("CMOOP_FRONTEND_BOUND_FILE")
    if path:
        with open(path, "a") as f:
            f.write(line + "\n")


def assert_log_within(tag, out, ref, bud, names, excusable=False):
    """|out - y| <= by on every element with rho < 0.5 -- every element unless `excusable` -- and out inside
    excused_window on the others.  Records the worst ratio per signal family (and the excused share) before it asserts."""
    _, rho, by = bud
    excused = rho >= 0.5
    err = np.abs(np.asarray(out, np.float64) - ref["y"])
    ratios = worst_ratios(err, by, names)
    record(f"{tag}: worst |out - y| / by {max(ratios.values()):.3f}  " + " ".join(f"{k} {v:.3f}" for k, v in ratios.items()) +
           (f"  excused {excused.mean():.4f}" if excusable else ""))
    assert excusable or not excused.any(), (tag, "excused elements", int(excused.sum()))
    bad = np.argwhere(err > by)
    assert len(bad) == 0, (tag, [(names[i], int(t), int(m), float(err[i, t, m]), float(by[i, t, m])) for i, t, m in bad[:8]])
    if excused.any():
        lo, hi = excused_window(ref, bud)
        o = np.asarray(out, np.float64)
        assert np.all((o >= lo)[excused]) and np.all((o <= hi)[excused]), (tag, "outside the excused window")


def band_stats(fb, n_mels):
    cnt = (fb != 0).sum(axis=1)
    return int((cnt == 0).sum()), int((cnt == 1).sum()), int(cnt.max()), int(min(64 - n_mels, (cnt >= 8).sum()))


# ---- float32 restatement and its perturbations (CPU test only) ---------------------------------------------------------
PERTURBATIONS = ("dropbin", "symhann", "winshift", "frameshift")


def restate32(wav, geo, log_eps=1e-6, perturb=None):
    """The reference's steps with dtype=float32 (numpy keeps rfft of float32 in complex64) -> y [n, T, n_mels] float32.
    perturb: None, or one of PERTURBATIONS -- a front end that is subtly wrong."""
    assert perturb is None or perturb in PERTURBATIONS
    f32 = np.float32
    w = np.asarray(wav, f32)
    n_fft, hop, wl = geo["n_fft"], geo["hop"], geo["win"]
    T = 1 + w.shape[1] // hop
    x = np.pad(w, ((0, 0), (n_fft // 2, n_fft // 2 + 1)))
    win = ofe.hann_padded(wl, n_fft)
    if perturb == "symhann":                                       # symmetric instead of periodic
        win = np.zeros(n_fft)
        lpad = (n_fft - wl) // 2
        win[lpad:lpad + wl] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(wl) / max(1, wl - 1))
    if perturb == "winshift":
        win = np.roll(win, 1)
    fb = ofe.mel_filterbank(geo["sr"], n_fft, geo["n_mels"], geo["fmin"], geo["fmax"]).copy()
    if perturb == "dropbin":                                       # the middle non-zero weight of the widest band
        m = int(np.argmax((fb != 0).sum(axis=1)))
        nz = np.flatnonzero(fb[m])
        fb[m, nz[len(nz) // 2]] = 0.0
    idx = np.arange(T)[:, None] * hop + np.arange(n_fft)[None, :] + (1 if perturb == "frameshift" else 0)
    fr = x[:, idx] * win.astype(f32)[None, None, :]
    X = np.fft.rfft(fr, axis=-1)
    assert fr.dtype == f32 and X.dtype == np.complex64
    P = X.real * X.real + X.imag * X.imag
    S = P @ fb.astype(f32).T
    y = np.log(S + f32(log_eps))
    assert y.dtype == f32
    return y
