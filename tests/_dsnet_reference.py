"""TEST INFRASTRUCTURE for the depthwise-separable topologies A_ds / B_ds (importable without a GPU or the library).

* ``SeparableOracleNet``: oracle.net.OracleNet with every k x k stride-1 convolution of C_in >= 16 replaced by a
  Keras-``SeparableConv2D``-style layer, depth multiplier 1: depthwise k x k (SAME, no bias, no activation), then pointwise
  1 x 1 carrying the bias.  Only ``__init__`` (tensor creation in the canonical order depthwise_kernel [k][k][C_in],
  pointwise_kernel [C_out][1][1][C_in], bias [C_out]) and ``forward`` are restated; train_step, state exchange, evaluate and
  use by oracle.net.fit / run_epoch are inherited.  Gradients come from autograd.
* float64 restatements of the depthwise forward, data gradient and weight gradient as explicit tap sums (no autograd, no
  torch convolution): what the kernel tests compare with.
"""
from typing import Dict, List, Sequence

import numpy as np
import torch
import torch.nn.functional as F

from oracle import net as ON
from oracle import rng as orng

VARIANT_A_DS, VARIANT_B_DS = 2, 3


def depthwise_same(x: torch.Tensor, dw_kkc: torch.Tensor) -> torch.Tensor:
    """DepthwiseConv2D(padding='same', stride 1, depth multiplier 1, no bias); x NCHW, kernel [kh][kw][C]."""
    k, c = dw_kkc.shape[0], dw_kkc.shape[2]
    t, bt = ON._same_pad(x.shape[2], k, 1)
    l, r = ON._same_pad(x.shape[3], k, 1)
    if t or bt or l or r:
        x = F.pad(x, (l, r, t, bt))
    return F.conv2d(x, dw_kkc.permute(2, 0, 1)[:, None, :, :], None, stride=1, groups=c)


class SeparableOracleNet(ON.OracleNet):
    """One candidate of topology A_ds (cfg.variant == 2) or B_ds (3)."""

    def __init__(self, gene: Sequence[int], cfg: ON.OracleConfig, seed: int, dtype: torch.dtype = torch.float32):
        assert cfg.variant in (VARIANT_A_DS, VARIANT_B_DS), cfg.variant
        self.gene = tuple(int(v) for v in gene)
        self.cfg = cfg
        self.dtype = dtype
        self.seed = int(seed) & 0xFFFFFFFF
        f, k, bn, R, fc, dr = self.gene
        self.use_bn, self.use_dropout = bool(bn), bool(dr)
        self.names: List[str] = []
        self.T: Dict[str, torch.Tensor] = {}
        self.trainable: List[str] = []
        self.is_a = cfg.variant == VARIANT_A_DS

        def add(name, shape, role, fans=None):
            idx = len(self.names)
            if role == "kernel":
                arr = orng.glorot_uniform(self.seed, idx, shape, fans[0], fans[1])
            elif role in ("gamma", "moving_var"):
                arr = np.ones(shape, np.float32)
            else:
                arr = np.zeros(shape, np.float32)
            t = torch.from_numpy(arr.copy()).to(dtype)
            if role in ("kernel", "bias", "gamma", "beta"):
                t.requires_grad_(True)
                self.trainable.append(name)
            self.names.append(name)
            self.T[name] = t

        def conv(name, cin, cout, ks):
            add(name + "/kernel", (cout, ks, ks, cin), "kernel", (ks * ks * cin, ks * ks * cout))
            add(name + "/bias", (cout,), "bias")

        def sepconv(name, cin, cout, ks):
            # Keras' fans: depthwise kernel (k, k, cin, 1) -> (k*k*cin, k*k); pointwise (1, 1, cin, cout) -> (cin, cout)
            add(name + "/depthwise_kernel", (ks, ks, cin), "kernel", (ks * ks * cin, ks * ks))
            add(name + "/pointwise_kernel", (cout, 1, 1, cin), "kernel", (cin, cout))
            add(name + "/bias", (cout,), "bias")

        def bnl(name, c):
            add(name + "/gamma", (c,), "gamma")
            add(name + "/beta", (c,), "beta")
            add(name + "/moving_mean", (c,), "moving_mean")
            add(name + "/moving_var", (c,), "moving_var")

        conv("conv1", 1, f, k)
        if bn:
            bnl("bn1", f)
        if self.is_a:
            sepconv("conv2", f, f, k)
            if bn:
                bnl("bn2", f)
        c = f
        for r in range(R):
            conv(f"res{r}_skip", c, 2 * c, 1)
            sepconv(f"res{r}_conv1", c, 2 * c, k)
            if bn:
                bnl(f"res{r}_bn1", 2 * c)
            if self.is_a:
                sepconv(f"res{r}_conv2", 2 * c, 2 * c, k)
                if bn:
                    bnl(f"res{r}_bn2", 2 * c)
            c *= 2
        prev = c
        self.fc_names = []
        for i, units in enumerate(ON.FC_LADDER[fc]):
            add(f"fc{i + 1}/kernel", (units, prev), "kernel", (prev, units))
            add(f"fc{i + 1}/bias", (units,), "bias")
            self.fc_names.append(f"fc{i + 1}")
            prev = units
        add("output_layer/kernel", (cfg.classes, prev), "kernel", (prev, cfg.classes))
        add("output_layer/bias", (cfg.classes,), "bias")
        self.m = {n: torch.zeros_like(self.T[n]) for n in self.trainable}
        self.v = {n: torch.zeros_like(self.T[n]) for n in self.trainable}
        self.iterations = 0
        self.step = 0

    def _sepconv(self, x, name):
        """depthwise in fp32 in every compute mode (as the first conv), pointwise through the GEMM path of the mode"""
        z = depthwise_same(x, self.T[name + "/depthwise_kernel"])
        w, b = self.T[name + "/pointwise_kernel"], self.T[name + "/bias"]
        if self.cfg.compute == "bf16":
            return ON._Bf16Conv.apply(z, w, b, 1)
        return ON.conv_same(z, w, b, 1)

    def forward(self, x: torch.Tensor, train: bool) -> torch.Tensor:
        f, k, bn, R, fc, dr = self.gene
        x = x[:, None, :, :]
        if self.is_a:
            x = self._conv(x, "conv1")
            if bn:
                x = self._bn(x, "bn1", train)
            x = F.relu(x)
            x = self._sepconv(x, "conv2")
            if bn:
                x = self._bn(x, "bn2", train)
            x = F.relu(x)
            x = ON.maxpool_same(x)
        else:
            x = F.relu(self._conv(x, "conv1"))
            if bn:
                x = self._bn(x, "bn1", train)
            x = ON.maxpool_same(x)
        for r in range(R):
            skip = self._conv(x, f"res{r}_skip", stride=2)
            if self.is_a:
                y = self._sepconv(x, f"res{r}_conv1")
                if bn:
                    y = self._bn(y, f"res{r}_bn1", train)
                y = F.relu(y)
                y = self._sepconv(y, f"res{r}_conv2")
                if bn:
                    y = self._bn(y, f"res{r}_bn2", train)
            else:
                y = F.relu(self._sepconv(x, f"res{r}_conv1"))
                if bn:
                    y = self._bn(y, f"res{r}_bn1", train)
            y = ON.maxpool_same(y)
            x = F.relu(y + skip)
        x = x.mean(dim=(2, 3))
        for li, name in enumerate(self.fc_names):
            x = F.relu(self._dense(x, name))
            if dr and train:
                keep = orng.dropout_keep(self.seed, li, self.step, x.shape[0], x.shape[1], self.cfg.dropout)
                scale = np.float32(1.0 / (1.0 - self.cfg.dropout))
                x = x * torch.from_numpy(keep.astype(np.float32)).to(x.dtype) * float(scale)
        z = x @ self.T["output_layer/kernel"].t() + self.T["output_layer/bias"]
        return torch.softmax(z, dim=1)


# ---- float64 tap sums, NHWC ------------------------------------------------------------------------------------------
def _padded(x, k):
    p = (k - 1) // 2
    return np.pad(np.asarray(x, np.float64), ((0, 0), (p, p), (p, p), (0, 0)))


def dw_forward64(x, w, absolute=False):
    """z[b,h,w,c] = sum_{ky,kx} x[b,h+ky-p,w+kx-p,c] w[ky][kx][c] in float64; absolute: the sum of |terms| instead"""
    k = w.shape[0]
    B, H, W, _ = x.shape
    xp, w = _padded(x, k), np.asarray(w, np.float64)
    if absolute:
        xp, w = np.abs(xp), np.abs(w)
    z = np.zeros(x.shape, np.float64)
    for ky in range(k):
        for kx in range(k):
            z += xp[:, ky:ky + H, kx:kx + W, :] * w[ky, kx]
    return z


def dw_dgrad64(dy, w, absolute=False):
    """dx[b,h,w,c] = sum_{ky,kx} dy[b,h-ky+p,w-kx+p,c] w[ky][kx][c]: the forward with the taps reversed"""
    return dw_forward64(dy, np.asarray(w)[::-1, ::-1, :], absolute)


def dw_wgrad64(x, dy, k, absolute=False):
    """ddw[ky][kx][c] = sum_{b,h,w} x[b,h+ky-p,w+kx-p,c] dy[b,h,w,c]"""
    B, H, W, C = x.shape
    xp, dy = _padded(x, k), np.asarray(dy, np.float64)
    if absolute:
        xp, dy = np.abs(xp), np.abs(dy)
    out = np.zeros((k, k, C), np.float64)
    for ky in range(k):
        for kx in range(k):
            out[ky, kx] = (xp[:, ky:ky + H, kx:kx + W, :] * dy).sum(axis=(0, 1, 2))
    return out
