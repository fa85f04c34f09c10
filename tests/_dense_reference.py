"""Float64 references of the MLP-head kernels (csrc/dense.hip), the dropout composition on top of the declared mask twin
(oracle/rng.py::dropout_keep), the bf16 operand rounding, the integer-regime operand generator with its exactness predicate,
the per-element float bound and the case lists of tests/test_gpu_dense_head.py.  Everything here runs on the CPU;
tests/test_dense_reference_cpu.py pins the restatement to torch autograd and the generators and case lists to their stated
conditions."""
import functools

import numpy as np
import torch

from oracle import rng as ORNG

U = 2.0 ** -24                                   # unit roundoff of float32
EXACT_LIMIT = 2 ** 24                            # integers of magnitude <= 2^24 are exact in float32

# CMOOP_GEMM_* (include/cmoop.h): the two arithmetic modes of the dense kernels, named explicitly (never the default)
GEMM_FP32, GEMM_BF16 = 1, 3
MODES = ((GEMM_FP32, "fp32"), (GEMM_BF16, "bf16"))


def f64(a):
    return np.asarray(a, np.float64)


def fl32(a):
    """Round to float32 (round-to-nearest-even), returned as float32."""
    return np.asarray(a, np.float64).astype(np.float32)


def bf16_round(a):
    """Operand rounding of GEMM_BF16: float32 -> bfloat16 (round-to-nearest-even) -> float32."""
    t = torch.from_numpy(np.array(a, np.float32))                 # a copy: the shared cases are read-only arrays
    return t.to(torch.bfloat16).to(torch.float32).numpy()


def operands(mode, *arrays):
    """The arrays as the MFMA sees them under `mode`, in float64."""
    return tuple(f64(bf16_round(a)) if mode == GEMM_BF16 else f64(a) for a in arrays)


# ---- the operations ---------------------------------------------------------------------------------------------------------
def fwd_ref(x, w, bias, relu, mode=GEMM_FP32):
    """y[M][N] = act(x[M][K] w[N][K]^T + bias[N]); the bias is never rounded to bf16 (it is added in the fp32 epilogue)."""
    xr, wr = operands(mode, x, w)
    y = xr @ wr.T + f64(bias)
    return np.maximum(y, 0.0) if relu else y


def dgrad_ref(dy, w, mask=None, scale=1.0, mode=GEMM_FP32):
    """dx[M][K] = dy[M][N] w[N][K], then (mask given) dx = mask > 0 ? dx * scale : 0.  The product with the scale is NOT
    rounded here: where dx is an integer below 2^24, fl32(dx * fl32(scale)) of the result is the kernel's value."""
    dyr, wr = operands(mode, dy, w)
    dx = dyr @ wr
    if mask is not None:
        dx = np.where(f64(mask) > 0.0, dx * float(scale), 0.0)
    return dx


def wgrad_ref(x, dy, mode=GEMM_FP32):
    """dw[N][K] = dy^T x (operands rounded under bf16), db[N] = sum_m dy (a plain fp32 column sum: never rounded)."""
    xr, dyr = operands(mode, x, dy)
    return dyr.T @ xr, f64(dy).sum(axis=0)


def keep_scale32(rate):
    """The keep scale as the trainer holds it: the double 1 / (1 - rate) rounded to float32."""
    return np.float32(1.0 / (1.0 - float(rate)))


def dropout_ref(y, seed, layer, step, rate):
    """Inverted dropout of y[M][N] (float64, exactly representable in float32): where(keep, fl32(fl32(y) * fl32(scale)), 0)
    with keep from the declared twin.  Returns (h float32, keep bool)."""
    M, N = y.shape
    keep = ORNG.dropout_keep(seed, layer, step, M, N, rate)
    y32 = fl32(y)
    assert np.array_equal(f64(y32), f64(y)), "dropout_ref wants a float32-exact input"
    h = np.where(keep, y32 * keep_scale32(rate), np.float32(0.0)).astype(np.float32)
    return h, keep


def dropout_dgrad_ref(dx0, h, rate):
    """Dropout + ReLU backward of the layer input h: where(h > 0, fl32(fl32(dx0) * fl32(scale)), 0), dx0 float32-exact."""
    d32 = fl32(dx0)
    assert np.array_equal(f64(d32), f64(dx0)), "dropout_dgrad_ref wants a float32-exact input"
    return np.where(np.asarray(h) > 0, d32 * keep_scale32(rate), np.float32(0.0)).astype(np.float32)


SMALLEST_RATE = 2.0 ** -24                       # threshold (uint32)(rate 2^24) = 1: the smallest rate that can drop at all


# ---- the integer regime -----------------------------------------------------------------------------------------------------
X_MAX, W_MAX, DY_MAX, B_MAX = 3, 2, 2, 4


def integer_operands(M, N, K, seed):
    """x in {0..3} (half of it real zeros, as after a ReLU), w and dy in {-2..2}, bias in {-4..4}: float32 arrays."""
    rs = np.random.RandomState(seed)
    x = (rs.randint(0, X_MAX + 1, (M, K)) * (rs.rand(M, K) < 0.5)).astype(np.float32)
    w = rs.randint(-W_MAX, W_MAX + 1, (N, K)).astype(np.float32)
    bias = rs.randint(-B_MAX, B_MAX + 1, (N,)).astype(np.float32)
    dy = rs.randint(-DY_MAX, DY_MAX + 1, (M, N)).astype(np.float32)
    return x, w, bias, dy


def partial_sum_limit(M, N, K, x_max=X_MAX):
    """The largest magnitude any partial sum of the four results can reach, from the shape and the operand ranges alone:
    forward K x w + bias, dgrad N dy w, wgrad M dy x, bias gradient M dy.  x_max: the largest |layer input| (the dropout
    backward at rate 0.5 feeds h = 2 x)."""
    return max(K * X_MAX * W_MAX + B_MAX, N * DY_MAX * W_MAX, M * DY_MAX * x_max, M * DY_MAX)


def integer_regime_exact(M, N, K, x_max=X_MAX):
    """Every partial sum, in any order, is an integer below 2^24: each fp32 add is exact, so the result has ONE value."""
    return partial_sum_limit(M, N, K, x_max) < EXACT_LIMIT


def is_small_integer(a):
    a = f64(a)
    return bool(np.all(a == np.rint(a)) and (np.abs(a).max() if a.size else 0.0) < EXACT_LIMIT)


# ---- the float regime -------------------------------------------------------------------------------------------------------
def dot_bound(n, abs_a, abs_b, abs_bias=0.0):
    """|fl(sum of n products + bias) - exact| <= gamma (sum |a_i||b_i| + |bias|), gamma = (n + 8) 2^-24, for an fp32 dot
    product of length n accumulated in ANY order (standard forward error analysis: every term passes through at most
    n + 6 roundings -- its product, a chain of fewer than n adds, the three wave-sum adds, the bias add, the multiplication
    by a mask scale -- and (1 + u)^(n + 6) - 1 <= (n + 6) u / (1 - (n + 6) u) <= (n + 8) u whenever (n + 8)(n + 6) u <= 2,
    asserted).  abs_a [R][n], abs_b [n][C] -> [R][C]."""
    assert (n + 8) * (n + 6) * U <= 2.0
    return (n + 8) * U * (f64(abs_a) @ f64(abs_b) + f64(abs_bias))


def fwd_bound(x, w, bias, mode=GEMM_FP32):
    xr, wr = operands(mode, x, w)
    return dot_bound(x.shape[1], np.abs(xr), np.abs(wr).T, np.abs(f64(bias)))


def dgrad_bound(dy, w, scale=1.0, mode=GEMM_FP32):
    dyr, wr = operands(mode, dy, w)
    return dot_bound(dy.shape[1], np.abs(dyr), np.abs(wr)) * abs(float(scale))


def wgrad_bound(x, dy, mode=GEMM_FP32):
    xr, dyr = operands(mode, x, dy)
    return dot_bound(x.shape[0], np.abs(dyr).T, np.abs(xr))


def db_bound(dy):
    return dot_bound(dy.shape[0], np.abs(f64(dy)).T, np.ones((dy.shape[0], 1)))[:, 0]


def gaussian_operands(M, N, K, seed):
    """x = relu(normal), w = normal / sqrt(K), bias and dy normal: the data of test_dense_head_kernels."""
    rs = np.random.RandomState(seed)
    x = np.maximum(rs.randn(M, K), 0).astype(np.float32)
    w = (rs.randn(N, K) / np.sqrt(K)).astype(np.float32)
    bias = rs.randn(N).astype(np.float32)
    dy = rs.randn(M, N).astype(np.float32)
    return x, w, bias, dy


# ---- the cases --------------------------------------------------------------------------------------------------------------
# K / 16 = 1, 3, 5, 16, 17, 31, 32, 65: a lone wave, ragged first trips, exactly one full trip of the forward's 4 waves x 4
# groups, a second trip owned by wave 0 only, a ragged and a full second trip, a third trip
K_VALUES = (16, 48, 80, 256, 272, 496, 512, 1040)
# classifier widths, the 16-wide tile edges, and 1 / 4 / 5 / 9 n-groups of the data gradient's wave-stride-4 loop
N_VALUES = (1, 10, 15, 16, 17, 35, 64, 80, 130)
# 1 / 4 / 5 / 17 m-groups of the weight gradient's loop, the partial batches
M_VALUES = (1, 15, 16, 17, 64, 65, 100, 257)

INTEGER_SHAPES = [   # (M, N, K): every value above with at least two different values of each other axis
    (1, 1, 16), (1, 10, 48), (15, 1, 80), (15, 15, 16), (16, 16, 48), (16, 10, 256), (17, 17, 80), (17, 35, 272),
    (64, 64, 256), (64, 35, 496), (65, 80, 272), (65, 130, 512), (100, 15, 496), (100, 130, 1040), (257, 16, 512),
    (257, 17, 1040), (1, 64, 512), (15, 80, 1040), (16, 130, 16), (17, 10, 496), (64, 15, 48), (65, 17, 256),
    (100, 35, 80), (257, 64, 272), (64, 80, 512), (100, 16, 16), (1, 130, 80), (257, 1, 48), (16, 35, 1040), (65, 10, 16),
]
EMPTY_BATCH_SHAPES = [(0, 17, 80), (0, 130, 272)]

GAUSSIAN_SHAPES = [
    (64, 512, 512), (257, 512, 512), (17, 35, 128), (1, 10, 16), (15, 17, 48), (65, 130, 272), (100, 15, 496),
    (16, 64, 1040), (257, 1, 80), (64, 80, 256),
]

# (M, N, K) of the dropout cases: a ragged N makes the row * N + col key matter
DROPOUT_SHAPES = [(17, 35, 128), (5, 11, 16), (64, 512, 512), (65, 130, 272)]
DROPOUT_RATES = (0.3, 0.5, SMALLEST_RATE)
DROPOUT_LAYERS = (0, 3)
DROPOUT_SEEDS = (42, 0xDEADBEEF)
DROPOUT_STEPS = (0, 1, 12345)
MAX_SHAPE = (257, 512, 1040)


def shape_seed(M, N, K):
    return 7919 * M + 104729 * N + K


@functools.lru_cache(maxsize=None)
def integer_case(M, N, K):
    """Operands and float64 references of one integer-regime shape, computed once and shared (read-only arrays)."""
    x, w, bias, dy = integer_operands(M, N, K, shape_seed(M, N, K))
    y = fwd_ref(x, w, bias, 0)
    dw, db = wgrad_ref(x, dy)
    c = dict(x=x, w=w, bias=bias, dy=dy, y=y, y_relu=np.maximum(y, 0.0), dx=dgrad_ref(dy, w), dx_masked=dgrad_ref(dy, w, x, 1.0),
             dw=dw, db=db)
    for a in c.values():
        a.setflags(write=False)
    return c
