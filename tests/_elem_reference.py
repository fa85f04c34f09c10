"""Float64 references of the BatchNorm / pooling / loss / optimiser kernels (csrc/bn.hip, elem.hip, loss.hip, optim.hip), the numpy float32
restatement of adam_update, the host twins of the launchers' shape arithmetic, and the input generators of
tests/test_gpu_elem_kernels.py.  Everything here runs on the CPU; tests/test_elem_reference_cpu.py pins the references
to oracle/net.py and the generators to their stated conditions."""
import math

import numpy as np
import torch

from oracle.net import OracleConfig, OracleNet

U = 2.0 ** -24                                   # unit roundoff of float32
CLIP_LO = float(np.float32(1e-7))                # the clip bounds as the kernel and the oracle hold them (float32)
CLIP_HI = float(np.float32(1.0) - np.float32(1e-7))


def gamma_n(n):
    """Higham's gamma_n = n u / (1 - n u): |fl(sum of n+1 terms) - sum| <= gamma_n sum|term|."""
    return n * U / (1.0 - n * U)


def f64(a):
    return np.asarray(a, np.float64)


# ---- host twins of the launchers' shape arithmetic (bn.hip, elem.hip) ---------------------------------------------------------------
def cdiv(a, b):
    return -(-a // b)


def colreduce_rpp(C):
    return max(1, 256 // (C // 4))


def colreduce_blocks(M, C):
    return int(max(1, min(1024, cdiv(M, colreduce_rpp(C) * 16))))


def colreduce_chain(M, C, blocks, term_roundings):
    """Longest fp32 chain of colreduce_kernel: a thread's rows, the block's rpp row groups, the roundings inside one term
    (x*x: 1; dy*((x-mu)*is): 3) and the final cast of the double total.  term_roundings = 1 gives the
    ceil(rows_per_block / rpp) + rpp + 2 of the statistics pass."""
    rpp = colreduce_rpp(C)
    return cdiv(cdiv(M, blocks), rpp) + rpp + term_roundings + 1


def gap_chain(HW, C):
    slices = 256 // (C // 4)
    return cdiv(HW, slices) + slices + 1


EW_GRID_CAP = 8192 * 256                          # threads of the largest element-wise grid (ew_grid)


# ---- BatchNorm --------------------------------------------------------------------------------------------------------------
def bn_train_ref(x, gamma, beta, eps, relu):
    """Two-pass float64 BatchNorm (training) of x[M][C]: the statistics, the folded scale / shift and y."""
    x, gamma, beta = f64(x), f64(gamma), f64(beta)
    mean = x.mean(axis=0)
    var = ((x - mean) ** 2).mean(axis=0)
    invstd = 1.0 / np.sqrt(var + eps)
    scale = gamma * invstd
    shift = beta - mean * scale
    y = x * scale + shift
    return dict(mean=mean, var=var, invstd=invstd, scale=scale, shift=shift, y=np.maximum(y, 0.0) if relu else y)


def bn_eval_ref(x, gamma, beta, mm, mv, eps, relu):
    scale = f64(gamma) / np.sqrt(f64(mv) + eps)
    shift = f64(beta) - f64(mm) * scale
    y = f64(x) * scale + shift
    return dict(scale=scale, shift=shift, y=np.maximum(y, 0.0) if relu else y)


def bn_moving_ref(mm, mv, mean, var, momentum):
    return f64(mm) * momentum + f64(mean) * (1.0 - momentum), f64(mv) * momentum + f64(var) * (1.0 - momentum)


def bn_bwd_sums_ref(dy, x, mean, invstd):
    """(sum dy, sum dy xhat) per channel with the GIVEN mean / invstd, and the sums of the terms' magnitudes."""
    dy, xh = f64(dy), (f64(x) - f64(mean)) * f64(invstd)
    return dy.sum(axis=0), (dy * xh).sum(axis=0), np.abs(dy).sum(axis=0), np.abs(dy * xh).sum(axis=0)


def bn_bwd_apply_ref(dy, x, mean, invstd, gamma, s1, s2, mask_x_pos):
    """dx = gamma invstd (dy - s1/M - xhat s2/M) with the GIVEN statistics and sums; second value: the sum of the magnitudes
    of the three terms, scaled by |gamma invstd| (what one rounding of the expression is relative to)."""
    dy, x = f64(dy), f64(x)
    M = x.shape[0]
    gi, xh = f64(gamma) * f64(invstd), (x - f64(mean)) * f64(invstd)
    a, b = f64(s1) / M, xh * (f64(s2) / M)
    dx, mag = gi * (dy - a - b), np.abs(gi) * (np.abs(dy) + np.abs(a) + np.abs(b))
    if mask_x_pos:
        dx = np.where(x > 0, dx, 0.0)
    return dx, mag


def bn_bwd_ref(dy, x, gamma, eps, mask_x_pos):
    """Float64 backward of training-mode BatchNorm from its own two-pass statistics: dx, dgamma, dbeta."""
    r = bn_train_ref(x, gamma, np.zeros_like(f64(gamma)), eps, 0)
    s1, s2, _, _ = bn_bwd_sums_ref(dy, x, r["mean"], r["invstd"])
    dx, _ = bn_bwd_apply_ref(dy, x, r["mean"], r["invstd"], gamma, s1, s2, mask_x_pos)
    return dx, s2, s1


def bn_autograd(x, gamma, beta, dy, eps, dtype, relu=0):
    """y, dx, dgamma, dbeta of OracleNet._bn (training) by autograd in `dtype`; x, dy [M][C]."""
    net = OracleNet((16, 3, 1, 0, 1, 0), OracleConfig(bn_eps=eps), 0, dtype=dtype)
    C = x.shape[1]
    g = torch.from_numpy(np.asarray(gamma)).to(dtype).requires_grad_(True)
    b = torch.from_numpy(np.asarray(beta)).to(dtype).requires_grad_(True)
    net.T["t/gamma"], net.T["t/beta"] = g, b
    net.T["t/moving_mean"], net.T["t/moving_var"] = torch.zeros(C, dtype=dtype), torch.ones(C, dtype=dtype)
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    y = net._bn(xt.t()[None, :, :, None], "t", True)[0, :, :, 0].t()
    if relu:
        y = torch.relu(y)
    y.backward(torch.from_numpy(np.asarray(dy)).to(dtype))
    return tuple(t.detach().numpy() for t in (y, xt.grad, g.grad, b.grad))


def one_pass_invstd_bound(x, M, C, blocks, eps):
    """Error bounds of the mean, of invstd and of the variance that bn_finalize derives from one-pass fp32 partials
    (sum x, sum x^2): the reduction bound gamma_n sum|term| carried through var = s2/M - mu^2 and 1/sqrt(var + eps),
    plus the casts to float."""
    x = f64(x)
    g = gamma_n(colreduce_chain(M, C, blocks, 1))
    mu, e1, e2 = x.mean(axis=0), g * np.abs(x).sum(axis=0) / M, g * (x * x).sum(axis=0) / M
    var = np.maximum((x * x).mean(axis=0) - mu * mu, 0.0)            # the kernel's form, in float64
    ev = e2 + 2.0 * np.abs(mu) * e1 + e1 * e1
    ev = ev + U * (var + ev)                                          # the cast of var to float
    f = lambda v: 1.0 / np.sqrt(v + eps)
    lo, hi = np.maximum(var - ev, 0.0), var + ev
    return e1 + U * np.abs(mu), np.maximum(f(lo) - f(var), f(var) - f(hi)) + 2.0 * U * f(lo), ev


# ---- exact regime -----------------------------------------------------------------------------------------------------------
def exact_deviations(M, k):
    """Integers d[M], |d| <= 6, with sum d = 0 and sum d^2 = k M (k even): a channel x = mu + d then has the integer mean mu
    and the biased variance k exactly.  M = 1 gives d = 0 (variance 0)."""
    assert k % 2 == 0
    if M == 1:
        return np.zeros(1, np.int64)
    if M == 3:
        assert k == 2
        return np.array([1, 1, -2], np.int64)
    d, target = [], k * M // 2
    for a in (6, 5, 4, 3, 2, 1):
        while target >= a * a:
            d += [a, -a]
            target -= a * a
    assert target == 0 and len(d) <= M, (M, k)
    return np.array(d + [0] * (M - len(d)), np.int64)


def exact_bn_input(M, C, seed):
    """x[M][C] of small integers (|x| <= 8), channel c with integer mean mu[c] in -2..2 and variance k[c] in {2, 14}
    (M = 1: 0; M = 3: 2), gamma a power of two, beta an integer, and the eps that makes invstd a power of two:
    var + eps = 4 or 16 with eps = 2 (M = 1: eps = 0.25, invstd = 2)."""
    rs = np.random.RandomState(seed)
    mu = rs.randint(-2, 3, C)
    k = np.where(np.arange(C) % 3 == 1, 14, 2) if M >= 8 else np.full(C, 0 if M == 1 else 2)
    x = np.empty((M, C), np.float32)
    for c in range(C):
        x[:, c] = mu[c] + rs.permutation(exact_deviations(M, int(k[c])))
    gamma = (2.0 ** rs.randint(-2, 3, C)).astype(np.float32) * np.where(rs.rand(C) < 0.25, -1, 1).astype(np.float32)
    beta = rs.randint(-3, 4, C).astype(np.float32)
    eps = 0.25 if M == 1 else 2.0
    return x, gamma, beta, eps, mu.astype(np.float64), k.astype(np.float64)


def exact_grad(shape, seed):
    """Integer gradient, |dy| <= 4."""
    return np.random.RandomState(seed).randint(-4, 5, shape).astype(np.float32)


# ---- pooling / GAP ----------------------------------------------------------------------------------------------------------
def maxpool_ref(y):
    """MaxPooling2D((2,2), 2, 'same') of y[B,H,W,C] in float64: pooled values and the window position of the FIRST maximum."""
    B, H, W, C = y.shape
    OH, OW = (H + 1) // 2, (W + 1) // 2
    pad = np.full((B, 2 * OH, 2 * OW, C), -np.inf)
    pad[:, :H, :W] = f64(y)
    win = pad.reshape(B, OH, 2, OW, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, OH, OW, 4, C)
    return win.max(axis=3), win.argmax(axis=3).astype(np.uint8)       # numpy's argmax returns the first maximum


def maxpool_scatter_ref(g, arg, H, W):
    """The full-resolution gradient of the pool: g[B,OH,OW,C] placed at window position arg, zero elsewhere."""
    B, OH, OW, C = g.shape
    full = np.zeros((B, OH, OW, 4, C))
    np.put_along_axis(full, arg[:, :, :, None, :].astype(np.int64), f64(g)[:, :, :, None, :], axis=3)
    full = full.reshape(B, OH, OW, 2, 2, C).transpose(0, 1, 3, 2, 4, 5).reshape(B, 2 * OH, 2 * OW, C)
    return np.ascontiguousarray(full[:, :H, :W])


def gap_ref(x):
    """Global average of x[B][HW][C] in float64, and the per-output sum of magnitudes / HW."""
    return f64(x).mean(axis=1), np.abs(f64(x)).mean(axis=1)


# ---- softmax + clipped sparse cross-entropy ---------------------------------------------------------------------------------
def softmax_ce_ref(z, y):
    """Float64: probabilities, per-row loss -(log pc_y - log sum_j pc_j) with pc = clip(p, lo, hi), d(mean loss)/dz."""
    z = f64(z)
    B, C = z.shape
    e = np.exp(z - z.max(axis=1, keepdims=True))
    p = e / e.sum(axis=1, keepdims=True)
    pc = np.clip(p, CLIP_LO, CLIP_HI)
    S = pc.sum(axis=1)
    rows = np.arange(B)
    loss = -(np.log(pc[rows, y]) - np.log(S))
    gate = ((p >= CLIP_LO) & (p <= CLIP_HI)).astype(np.float64)
    q = 1.0 / S[:, None] * np.ones((B, C))
    q[rows, y] -= 1.0 / pc[rows, y]
    q *= gate
    dz = p * (q - (p * q).sum(axis=1, keepdims=True)) / B
    return p, loss, dz


def softmax_ce_autograd(z, y, dtype):
    """The oracle's path in `dtype`: torch.softmax -> OracleNet.loss_per_sample, gradient of the mean loss."""
    zt = torch.from_numpy(np.asarray(z)).to(dtype).requires_grad_(True)
    p = torch.softmax(zt, dim=1)
    lps = OracleNet.loss_per_sample(p, torch.from_numpy(np.asarray(y).astype(np.int64)))
    lps.mean().backward()
    return p.detach().numpy(), lps.detach().numpy(), zt.grad.numpy()


LOGIT_FAMILIES = ("normal", "confident_right", "confident_wrong")


def confident_logit(C):
    """Magnitude of the confident logit: 20, raised to the smallest integer at which the row's 1 - p (about
    (C - 1) e^-L) stays below 1e-7 / 1.5 with a 10 % margin.  C <= 11: 20.  C = 35: 21 -- at 20, 1 - p = 7.0e-8 lies inside
    the excluded band around 1e-7 (the float32 p_y = 1 / (1 + 2^-23) then lands exactly on the upper clip bound while the
    float64 p_y lies beyond it: the gate would differ between the precisions)."""
    L = 20
    while 1.1 * (C - 1) * math.exp(0.005 - L) >= 1e-7 / 1.5:
        L += 1
    return float(L)


def softmax_cases():
    """(family, B, C, seed) of the GPU loss test: every C with every B, every family."""
    return [(fam, B, C, 7 * B + C + 1000 * fi) for fi, fam in enumerate(LOGIT_FAMILIES) for C in (2, 10, 11, 35)
            for B in (1, 5, 255, 256, 257, 600)]


def make_logits(family, B, C, seed):
    """(z[B][C] float32, labels[B] int32).  normal: N(0,1); confident_right: z_y = +L, others N(0, 0.1);
    confident_wrong: z_y = -L, one other +L, the rest N(0, 0.1); L = confident_logit(C) (20; 21 at C = 35).  The top-two gap of every row is at least 1e-3, except
    row 0 of the normal family when B >= 5: an exact duplicate of its maximum at a LATER index (first index must win)."""
    rs = np.random.RandomState(seed)
    y = rs.randint(0, C, B).astype(np.int32)
    rows = np.arange(B)
    if family == "normal":
        z = rs.randn(B, C).astype(np.float32)
    else:
        z = (0.1 * rs.randn(B, C)).astype(np.float32)
        big = np.float32(confident_logit(C))
        if family == "confident_right":
            z[rows, y] = big
        else:
            z[rows, y] = -big
            z[rows, (y + 1 + rs.randint(0, C - 1, B)) % C] = big
    srt = np.sort(z, axis=1)
    close = (srt[:, -1] - srt[:, -2]) < 2e-3
    z[close, z[close].argmax(axis=1)] += np.float32(0.01)
    if family == "normal" and B >= 5:
        first = int(z[0].argmax())
        if first == C - 1:                                   # move the maximum to the front so that a later twin exists
            z[0, 0], z[0, first] = z[0, first], z[0, 0]
            first = 0
        z[0, C - 1] = z[0, first]
    return z, y


def logits_conditions(z, y, family):
    """(ok, message): in float64 no probability p and no 1 - p lies within a factor 1.5 of 1e-7 (the clip gate then falls
    on the same side in float32 and float64), and the top-two logit gap is >= 1e-3 outside the one duplicated row."""
    p, _, _ = softmax_ce_ref(z, y)
    one_minus = 1.0 - p
    for name, v, thr in (("p", p, 1e-7), ("1-p", one_minus, 1e-7)):
        bad = (v > thr / 1.5) & (v < thr * 1.5)
        if bad.any():
            return False, f"{name} within a factor 1.5 of {thr:.3e}: {v[bad][:4]}"
    srt = np.sort(f64(z), axis=1)
    gap = srt[:, -1] - srt[:, -2]
    dup = family == "normal" and z.shape[0] >= 5
    if dup and gap[0] != 0.0:
        return False, "row 0 has no duplicated maximum"
    if (gap[1 if dup else 0:] < 1e-3).any():
        return False, f"top-two gap below 1e-3: {gap.min()}"
    return True, ""


# ---- Adam -------------------------------------------------------------------------------------------------------------------
def keras_alpha(lr, beta1, beta2, t):
    """Bias-corrected step size of iteration t (1-based), in double as Net::step_body forms it."""
    return lr * math.sqrt(1.0 - beta2 ** t) / (1.0 - beta1 ** t)


def adam_step_f32(w, g, m, v, alpha, beta1, beta2, eps):
    """adam_update restated in numpy float32, one IEEE single operation per line, in the kernel's order.
    Returns the new (w, m, v); inputs are not modified."""
    f = np.float32
    w, g, m, v = (np.asarray(a, f) for a in (w, g, m, v))
    alpha, c1, c2, eps = f(alpha), f(1.0 - beta1), f(1.0 - beta2), f(eps)
    with np.errstate(under="ignore"):
        dm = (g - m) * c1
        m = m + dm
        gg = g * g
        dv = (gg - v) * c2
        v = v + dv
        num = m * alpha
        den = np.sqrt(v) + eps
        w = w - num / den
    return w.astype(f), m.astype(f), v.astype(f)


def adam_gradients(n, seed):
    """Random gradients with the edge values of the update mixed in: exact zeros and 1e-25 (g*g underflows to 0)."""
    rs = np.random.RandomState(seed)
    g = (rs.randn(n) * 10.0 ** rs.uniform(-4, 0, n)).astype(np.float32)
    g[rs.rand(n) < 0.1] = 0.0
    g[rs.rand(n) < 0.1] = np.float32(1e-25)
    if n >= 2:
        g[0], g[-1] = 0.0, np.float32(1e-25)
    return g


# ---- small output-layer helpers / confusion ---------------------------------------------------------------------------------
def confusion_ref(yt, yp, C, force_true_zero):
    cm = np.zeros((C, C), np.int64)
    a = np.zeros_like(yt) if force_true_zero else yt
    ok = (a >= 0) & (a < C) & (yp >= 0) & (yp < C)
    np.add.at(cm, (a[ok], yp[ok]), 1)
    return cm
