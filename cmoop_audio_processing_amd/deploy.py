"""From a search result to a model that scores recordings.

The search ranks candidates by (accuracy, size, FPR) and keeps no weights.  ``PopulationEvaluator.train_model`` trains
one candidate again on its own seed and returns a ``TrainedModel``: the gene, the parameters in canonical order
(BatchNorm moving statistics included) and, optionally, the front end and the StandardScaler the features were made
with.  ``StreamScorer`` runs such a model over ONE recording: ``log_mel_stream`` (the front end's frames spread over the
chip) followed by ``NetSession.predict_stream`` (overlapping windows of T frames every ``hop_frames``, each one forward
pass; the frames two windows share are convolved again -- there is no streaming convolution cache).

Train / serve difference to know about: a training clip is centre-padded, so its first and last ``n_fft / (2 hop)``
frames see zeros where a window inside a recording sees real audio.  With a PCEN front end there is a second one: a
training clip starts its smoother at its own first frame (``M[-1] = E[0]``), a window inside a recording inherits the
state the recording has built up since ITS first frame.  The smoother forgets with a time constant of ``1 / s`` frames
(40 at the default s = 0.025), which is not short beside a 101-frame clip: the first frames of a training patch are
normalised by a younger smoother than the same audio gets inside a stream.  There is no per-window reset in
``predict_stream``; train on clips cut with some lead-in, or use a larger ``s``, when that matters.

``smooth_posteriors`` and ``detect_events`` are the usual host-side read-out of the window posteriors (float64 numpy).
"""
from __future__ import annotations

import dataclasses
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import genes as G
from .evaluator import EvalConfig
from .frontend import FrontendConfig, PcenConfig, log_mel_stream
from .quant import Int8Levels
from .resample import to_rate

_OBJECTIVE_KEYS = ("acc", "size_mb", "fpr", "epochs_run")
_FE_INT = ("sr", "n_fft", "win", "hop", "n_mels")
_FE_FLOAT = ("fmin", "fmax", "log_eps", "db_amin", "top_db")
_FE_SCALES = ("log", "db", "power", "pcen")                 # "frontend_scale" holds the index; written for the last two only
_PCEN_FIELDS = ("s", "alpha", "delta", "r", "eps", "input_scale")


@dataclasses.dataclass
class TrainedModel:
    """One trained candidate: everything ``session()`` needs to rebuild the net, in plain numpy."""
    gene: Tuple[int, ...]
    variant: str                       # "A" / "B" / "A_ds" / "B_ds" (genes.VARIANT_NAMES)
    classes: int
    T: int
    F: int
    seed: int
    params: np.ndarray                 # float32, canonical order (genes.param_tensors), moving statistics included
    objectives: Dict[str, float]       # acc, size_mb, fpr, epochs_run
    frontend: Optional[FrontendConfig] = None
    mean: Optional[np.ndarray] = None  # StandardScaler of the training features, float64 [F]
    scale: Optional[np.ndarray] = None
    # one detection threshold per class, float32 [classes]: the operating point of the validation split under
    # EvalConfig.operating_point (opoint.py), what detect_events takes; None when the model was trained without it
    thresholds: Optional[np.ndarray] = None
    # a model trained under EvalConfig.quant (quant.py): the bit width, the int8 code of every kernel element at its index in
    # ``params`` (0 elsewhere) and one float32 scale per channel; ``params`` then holds the dequantised kernels,
    # float32(codes) * scales bit for bit, so every fp32 path scores the quantised model.  All three or none
    quant_bits: Optional[int] = None
    quant_codes: Optional[np.ndarray] = None
    quant_scales: Optional[np.ndarray] = None
    # a model trained under EvalConfig.prune (prune.py): the final sparsity and, per kernel tensor in arena order, the number
    # of elements k the pruning had to zero (0 for a tensor it copied); ``params`` then holds the pruned kernels (quantised on
    # top when the model carries codes as well), so every fp32 path scores the sparse model.  Both or neither
    prune_sparsity: Optional[float] = None
    prune_k: Optional[np.ndarray] = None
    # a model trained under EvalConfig.act_quant (quant.ActQuantConfig): the bit width and the tracked range records of the
    # sites, a structured array [sites] of (m_b, r, count, reserved) in site order (NetSession.get_act_ranges); ``session()``
    # turns the option on with them, so it scores exactly the model the fit scored.  Both or neither.  ``act_momentum``: the
    # momentum the fit tracked the ranges with (0.99 when absent), so that training on from ``session()`` continues as the fit did
    act_bits: Optional[int] = None
    act_ranges: Optional[np.ndarray] = None
    act_momentum: Optional[float] = None

    def __post_init__(self):
        self.gene = tuple(int(v) for v in self.gene)
        G.validate_gene(self.gene)
        if self.variant not in G.VARIANT_CODES.values():
            raise ValueError(f"variant must be one of {sorted(G.VARIANT_CODES.values())}, got {self.variant!r}")
        self.params = np.ascontiguousarray(self.params, np.float32).reshape(-1)
        want = G.param_count(self.gene, G.VARIANT_NAMES[self.variant], int(self.classes))
        if self.params.size != want:
            raise ValueError(f"params holds {self.params.size} values, gene {self.gene} has {want}")
        if (self.mean is None) != (self.scale is None):
            raise ValueError("mean and scale come together (both or neither)")
        if self.mean is not None:
            self.mean = np.ascontiguousarray(self.mean, np.float64).reshape(-1)
            self.scale = np.ascontiguousarray(self.scale, np.float64).reshape(-1)
            if self.mean.size != self.F or self.scale.size != self.F:
                raise ValueError(f"mean and scale must hold F = {self.F} values each")
        if self.thresholds is not None:
            self.thresholds = np.ascontiguousarray(self.thresholds, np.float32).reshape(-1)
            if self.thresholds.size != int(self.classes):
                raise ValueError(f"thresholds must hold classes = {self.classes} values")
        self.objectives = {k: (int(self.objectives[k]) if k == "epochs_run" else float(self.objectives[k]))
                           for k in _OBJECTIVE_KEYS if k in self.objectives}
        present = [v is not None for v in (self.quant_bits, self.quant_codes, self.quant_scales)]
        if any(present) and not all(present):
            raise ValueError("quant_bits, quant_codes and quant_scales come together (all three or none)")
        if all(present):
            from . import quant as Q
            self.quant_bits = int(self.quant_bits)
            qmax = Q.qmax_of(self.quant_bits)
            self.quant_codes = np.ascontiguousarray(self.quant_codes, np.int8).reshape(-1)
            self.quant_scales = np.ascontiguousarray(self.quant_scales, np.float32).reshape(-1)
            rows = Q.quant_table(self.gene, G.VARIANT_NAMES[self.variant], int(self.classes))
            if self.quant_codes.size != want or self.quant_scales.size != sum(r[1] for r in rows):
                raise ValueError("quant_codes must hold one value per parameter and quant_scales one per kernel channel")
            if int(np.abs(self.quant_codes.astype(np.int32)).max(initial=0)) > qmax:
                raise ValueError(f"quant_codes exceed the {self.quant_bits}-bit range [-{qmax}, {qmax}]")
            back = Q.dequantize(self.quant_codes, self.quant_scales, rows, like=self.params)
            if not np.array_equal(back.view(np.uint32), self.params.view(np.uint32)):
                raise ValueError("params do not equal float32(quant_codes) * quant_scales at the kernel tensors")

        if (self.prune_sparsity is None) != (self.prune_k is None):
            raise ValueError("prune_sparsity and prune_k come together (both or neither)")
        if self.prune_k is not None:
            self.prune_sparsity = float(self.prune_sparsity)
            if not 0.0 < self.prune_sparsity < 1.0:
                raise ValueError("prune_sparsity must be in (0, 1)")
            self.prune_k = np.ascontiguousarray(self.prune_k, np.int64).reshape(-1)
            spans = self._kernel_spans()
            if self.prune_k.size != len(spans):
                raise ValueError(f"prune_k must hold one value per kernel tensor ({len(spans)})")
            for (name, off, n), k in zip(spans, self.prune_k):
                zeros = int(((self.params[off:off + n].view(np.uint32) & np.uint32(0x7FFFFFFF)) == 0).sum())
                if not 0 <= k <= n or zeros < k:
                    raise ValueError(f"{name} holds {zeros} zeros, its prune_k asks for at least {int(k)}")

        if (self.act_bits is None) != (self.act_ranges is None):
            raise ValueError("act_bits and act_ranges come together (both or neither)")
        if self.act_ranges is not None:
            from . import quant as Q
            self.act_bits = int(self.act_bits)
            self.act_momentum = float(np.float32(0.99 if self.act_momentum is None else self.act_momentum))
            Q.ActQuantConfig(bits=self.act_bits, momentum=self.act_momentum).check()
            Q.qmax_of(self.act_bits)
            self.act_ranges = np.ascontiguousarray(self.act_ranges, Q.ACT_RANGE_DTYPE).reshape(-1)
            sites = Q.act_sites(self.gene, self.variant, int(self.classes), int(self.T), int(self.F))
            if self.act_ranges.size != len(sites):
                raise ValueError(f"act_ranges must hold one record per site ({len(sites)})")

    def _kernel_spans(self):
        """[(name, offset in ``params``, elements)] of the kernel tensors in arena order (the rows of ``prune.prune_table``)."""
        out, off = [], 0
        for name, shape, role in G.param_tensors(self.gene, G.VARIANT_NAMES[self.variant], self.classes):
            n = int(np.prod(shape))
            if role == "kernel":
                out.append((name, off, n))
            off += n
        return out

    def sparsity_report(self) -> Dict[str, Dict[str, float]]:
        """{kernel tensor name: {"elements", "zeros", "k", "sparsity"}} plus "total" over the tensors with k > 0 (zeros /
        elements there, 0.0 when there is none) of a model that carries ``prune_k``; raises otherwise.  ``zeros`` counts +0.0
        and -0.0 in ``params``, so it is at least ``k`` and more when keys tied at the threshold or weights were zero anyway."""
        if self.prune_k is None:
            raise ValueError("the model carries no pruned weights (train it under EvalConfig.prune)")
        out, tz, tn = {}, 0, 0
        for (name, off, n), k in zip(self._kernel_spans(), self.prune_k):
            zeros = int(((self.params[off:off + n].view(np.uint32) & np.uint32(0x7FFFFFFF)) == 0).sum())
            out[name] = {"elements": n, "zeros": zeros, "k": int(k), "sparsity": zeros / n}
            if k > 0:
                tz, tn = tz + zeros, tn + n
        out["total"] = {"elements": tn, "zeros": tz, "k": int(self.prune_k.sum()), "sparsity": tz / tn if tn else 0.0}
        return out

    def tensors(self) -> Dict[str, np.ndarray]:
        """{name: array} in the shapes of ``genes.param_tensors`` (views of ``params``)."""
        out, off = {}, 0
        for name, shape, _role in G.param_tensors(self.gene, G.VARIANT_NAMES[self.variant], self.classes):
            n = int(np.prod(shape))
            out[name] = self.params[off:off + n].reshape(shape)
            off += n
        return out

    def int8_tensors(self) -> Dict[str, Tuple[np.ndarray, np.ndarray]]:
        """{kernel tensor name: (int8 codes in the shape of ``genes.param_tensors``, float32 scales: one per channel -- per
        leading index, or per c of a depthwise kernel [kh][kw][C])} of a model that carries codes; raises otherwise."""
        if self.quant_codes is None:
            raise ValueError("the model carries no quantised weights (train it under EvalConfig.quant)")
        out, off, pos = {}, 0, 0
        for name, shape, role in G.param_tensors(self.gene, G.VARIANT_NAMES[self.variant], self.classes):
            n = int(np.prod(shape))
            if role == "kernel":
                ch = int(shape[2]) if name.endswith("/depthwise_kernel") else int(shape[0])
                out[name] = (self.quant_codes[off:off + n].reshape(shape), self.quant_scales[pos:pos + ch])
                pos += ch
            off += n
        return out

    def save(self, path) -> None:
        """One ``.npz`` (numeric arrays only, no pickle), written to exactly ``path``.

        Front end keys: ``frontend_int`` (sr, n_fft, win, hop, n_mels, 1 for the dB scale else 0, db_ref_max) and
        ``frontend_float`` as ever; ``frontend_scale`` (index into log / db / power / pcen) only for a power or PCEN
        front end, whose ``frontend_int[5]`` is 0; ``frontend_pcen`` (s, alpha, delta, r, eps, input_scale) only when
        the front end carries a ``PcenConfig``.  A model without a front end, or with a log or dB one, writes the keys
        it always wrote.  ``thresholds`` (float32 [classes]) only when the model carries them; ``quant_bits`` (int64 [1]),
        ``quant_codes`` (int8) and ``quant_scales`` (float32) only when it carries quantised weights; ``prune_sparsity`` (float64
        [1]) and ``prune_k`` (int64) only when it carries pruned ones; ``act_bits`` (int64 [1]), ``act_ranges`` (float32 [sites, 2]:
        m_b, r), ``act_counts`` (int64 [sites]) and ``act_momentum`` (float64 [1]) only when it carries activation ranges."""
        d = {"gene": np.asarray(self.gene, np.int32),
             "meta": np.asarray([G.VARIANT_NAMES[self.variant], self.classes, self.T, self.F, self.seed], np.int64),
             "params": self.params,
             "objectives": np.asarray([float(self.objectives.get(k, np.nan)) for k in _OBJECTIVE_KEYS], np.float64)}
        if self.frontend is not None:
            fe = self.frontend
            d["frontend_int"] = np.asarray([getattr(fe, k) for k in _FE_INT] + [int(fe.scale == "db"), int(bool(fe.db_ref_max))],
                                           np.int64)
            d["frontend_float"] = np.asarray([getattr(fe, k) for k in _FE_FLOAT], np.float64)
            if fe.scale not in _FE_SCALES:
                raise ValueError(f"front end scale {fe.scale!r} cannot be saved")
            if fe.scale in ("power", "pcen"):
                d["frontend_scale"] = np.asarray([_FE_SCALES.index(fe.scale)], np.int64)
            if fe.pcen is not None:
                d["frontend_pcen"] = np.asarray([getattr(fe.pcen, k) for k in _PCEN_FIELDS], np.float64)
        if self.mean is not None:
            d["mean"], d["scale"] = self.mean, self.scale
        if self.thresholds is not None:
            d["thresholds"] = self.thresholds
        if self.quant_codes is not None:
            d["quant_bits"] = np.asarray([self.quant_bits], np.int64)
            d["quant_codes"], d["quant_scales"] = self.quant_codes, self.quant_scales
        if self.prune_k is not None:
            d["prune_sparsity"], d["prune_k"] = np.asarray([self.prune_sparsity], np.float64), self.prune_k
        if self.act_ranges is not None:
            d["act_bits"] = np.asarray([self.act_bits], np.int64)
            d["act_ranges"] = np.stack([self.act_ranges["m_b"], self.act_ranges["r"]], axis=1).astype(np.float32)
            d["act_counts"] = self.act_ranges["count"].astype(np.int64)
            d["act_momentum"] = np.asarray([self.act_momentum], np.float64)
        with open(path, "wb") as f:
            np.savez(f, **d)

    @classmethod
    def load(cls, path) -> "TrainedModel":
        with np.load(path, allow_pickle=False) as z:
            variant, classes, T, F, seed = (int(v) for v in z["meta"])
            obj = {k: float(v) for k, v in zip(_OBJECTIVE_KEYS, z["objectives"]) if not np.isnan(v)}
            fe = None
            if "frontend_int" in z.files:
                fi, ff = [int(v) for v in z["frontend_int"]], [float(v) for v in z["frontend_float"]]
                scale = "db" if fi[5] else "log"
                if "frontend_scale" in z.files:
                    scale = _FE_SCALES[int(z["frontend_scale"][0])]
                pcen = None
                if "frontend_pcen" in z.files:
                    pcen = PcenConfig(**dict(zip(_PCEN_FIELDS, (float(v) for v in z["frontend_pcen"]))))
                fe = FrontendConfig(**dict(zip(_FE_INT, fi[:5])), scale=scale, db_ref_max=bool(fi[6]),
                                    **dict(zip(_FE_FLOAT, ff)), pcen=pcen)
            mean = z["mean"].copy() if "mean" in z.files else None
            scale = z["scale"].copy() if "scale" in z.files else None
            thresholds = z["thresholds"].copy() if "thresholds" in z.files else None
            quant = {}
            if "quant_codes" in z.files:
                quant = dict(quant_bits=int(z["quant_bits"][0]), quant_codes=z["quant_codes"].copy(),
                             quant_scales=z["quant_scales"].copy())
            prune = {}
            if "prune_k" in z.files:
                prune = dict(prune_sparsity=float(z["prune_sparsity"][0]), prune_k=z["prune_k"].copy())
            act = {}
            if "act_ranges" in z.files:
                from . import quant as Q
                rec = np.zeros(len(z["act_counts"]), Q.ACT_RANGE_DTYPE)
                rec["m_b"], rec["r"], rec["count"] = z["act_ranges"][:, 0], z["act_ranges"][:, 1], z["act_counts"]
                act = dict(act_bits=int(z["act_bits"][0]), act_ranges=rec,
                           act_momentum=float(z["act_momentum"][0]) if "act_momentum" in z.files else None)
            return cls(gene=tuple(int(v) for v in z["gene"]), variant=G.VARIANT_CODES[variant], classes=classes, T=T, F=F, seed=seed,
                       params=z["params"].copy(), objectives=obj, frontend=fe, mean=mean, scale=scale,
                       thresholds=thresholds, **quant, **prune, **act)

    def _require_int8(self, int8: bool = True, int8_depthwise: bool = False, int8_fused: bool = False) -> Int8Levels:
        """The level keywords of a public entry as one checked record (``_open`` takes it).  ValueError naming what a model
        lacks for integer inference, or ``int8_depthwise`` / ``int8_fused`` without ``int8`` (host only: before any session
        opens)."""
        levels = Int8Levels.of(int8, int8_depthwise, int8_fused, (
            "int8_depthwise=True needs int8=True: integer depthwise is a level of integer inference",
            "int8_fused=True needs int8=True: the requantising epilogue is a level of integer inference"))
        missing = [name for name, v in (("quant_codes (train it under EvalConfig.quant)", self.quant_codes),
                                        ("act_ranges (train it under EvalConfig.act_quant)", self.act_ranges)) if v is None]
        if levels.on and missing:
            raise ValueError("int8=True needs a full-int8 model; this one carries no " + " and no ".join(missing))
        return levels

    def session(self, config: Optional[EvalConfig] = None, int8: bool = False, int8_depthwise: bool = False,
                int8_fused: bool = False):
        """A ``NetSession`` holding these parameters (needs the GPU).  ``config`` supplies ``eval_batch`` and the like;
        its variant and class count must be the model's.  A model that carries ``act_ranges`` gets the activation quantiser
        at ``act_bits`` and ``act_momentum`` with those ranges, whatever ``config.act_quant`` says.  ``int8``: integer
        inference (``NetSession.set_int8``) -- the model must carry ``quant_codes`` and ``act_ranges`` (ValueError otherwise,
        before the session opens); the weight quantiser is turned on at ``quant_bits``, which gives the model's own codes and
        scales back from the dequantised ``params`` (the absmax element of a channel is code qmax, and
        ``fl(fl(qmax s) / qmax) == s``).  ``int8_depthwise``: the second level as well (``NetSession.set_int8(True,
        depthwise=True)``): it needs ``int8=True`` (ValueError otherwise, before the session opens), needs nothing more of the
        model, and has no effect on an A / B model.  ``int8_fused``: the third level (``NetSession.set_int8(True, fused=True)``),
        under the same terms; its logits are those of the levels it is added to, bit for bit."""
        return self._open(config, self._require_int8(int8, int8_depthwise, int8_fused))

    def _open(self, config: Optional[EvalConfig], levels: Int8Levels):
        """``session`` behind the public boundary: ``levels`` is what ``_require_int8`` returned."""
        from .session import NetSession
        if config is None:
            config = EvalConfig(variant=self.variant, classes=self.classes)
        if config.variant != self.variant or int(config.classes) != self.classes:
            raise ValueError(f"config is variant {config.variant} / {config.classes} classes, the model is "
                             f"{self.variant} / {self.classes}")
        net = NetSession(self.gene, config, self.T, self.F, self.seed)
        try:
            net.set_params(self.params)
            if self.act_ranges is not None:   # the activation quantiser the fit scored with, under its tracked ranges
                from .quant import ActQuantConfig
                net.set_act_quant(ActQuantConfig(bits=self.act_bits, momentum=self.act_momentum))
                net.set_act_ranges(self.act_ranges)
            if levels.on:
                from .quant import QuantConfig
                net.set_quant(QuantConfig(bits=self.quant_bits, objective=False))
                net.set_int8(True, depthwise=levels.depthwise, fused=levels.fused)
        except Exception:
            net.close()
            raise
        return net

    def logits(self, X, config: Optional[EvalConfig] = None, int8: bool = False, int8_depthwise: bool = False,
               int8_fused: bool = False):
        """CUDA float32 [n, classes]: this model's logits of the rows X (CUDA float32 [n, T, F]) -- ``session(config)`` and
        ``NetSession.predict_logits``; what ``PopulationEvaluator.set_teacher`` trains candidates against.  ``int8``: the
        integer-inference logits (``session(config, int8=True)``), ``int8_depthwise``: with its second level, ``int8_fused``: with
        its third."""
        with self._open(config, self._require_int8(int8, int8_depthwise, int8_fused)) as net:
            return net.predict_logits(X)

    def int8_report(self, X, y=None, config: Optional[EvalConfig] = None, depthwise: bool = False,
                    fused: bool = False) -> Dict[str, float]:
        """How far integer inference lies from the fake-quantised fp32 pass on the rows X (CUDA float32 [n, T, F]): one
        session, ``predict_logits`` with the mode off and on -> {"rows", "argmax_agree" (fraction of rows with the same arg
        max), "max_abs_logit_diff", "int8_ops" (how many ops ran integer)}, and with labels ``y`` (CUDA or host ints [n])
        "acc_fakequant" and "acc_int8" as well.  ``depthwise``: the integer side runs with the second level on, and the report
        gains "int8_dw_ops" (how many depthwise ops ran integer; 0 for an A / B model).  ``fused``: the integer side runs with the
        third level on, and the report gains "int8_fused_ops" (how many ops took the requantising epilogue).  A reported
        figure, no gate."""
        import torch
        levels = self._require_int8(True, depthwise, fused)
        with self._open(config, levels) as net:
            zi = net.predict_logits(X)
            n_ops = len(net.int8_ops())
            n_dw = len(net.int8_dw_ops()) if levels.depthwise else 0
            n_fused = len(net.int8_fused_ops()) if levels.fused else 0
            net.set_int8(False)
            zf = net.predict_logits(X)
        n = int(zi.shape[0])
        ai, af = zi.argmax(dim=1), zf.argmax(dim=1)
        out = {"rows": n, "argmax_agree": float((ai == af).float().mean().item()) if n else 1.0,
               "max_abs_logit_diff": float((zi - zf).abs().max().item()) if n else 0.0, "int8_ops": n_ops}
        if y is not None:
            yt = torch.as_tensor(y).to(device=zi.device, dtype=torch.int64).reshape(-1)
            out["acc_fakequant"] = float((af == yt).float().mean().item()) if n else 0.0
            out["acc_int8"] = float((ai == yt).float().mean().item()) if n else 0.0
        if depthwise:
            out["int8_dw_ops"] = n_dw
        if fused:
            out["int8_fused_ops"] = n_fused
        return out


class StreamScorer:
    """``score(recording)`` = ``log_mel_stream`` with the model's front end, then ``predict_stream`` every ``hop_frames``.

    A dB front end hands its config to ``predict_stream`` for the per-window reference and floor.  A PCEN front end
    does not: ``log_mel_stream`` has normalised the recording once, windows are plain cuts of it."""

    def __init__(self, model: TrainedModel, hop_frames: int, config: Optional[EvalConfig] = None, int8: bool = False,
                 int8_depthwise: bool = False, int8_fused: bool = False):
        if int(hop_frames) < 1:
            raise ValueError("hop_frames must be at least 1")
        levels = model._require_int8(int8, int8_depthwise, int8_fused)
        self.model, self.hop_frames = model, int(hop_frames)
        self.frontend = model.frontend if model.frontend is not None else FrontendConfig()
        if int(self.frontend.n_mels) != model.F:
            raise ValueError(f"the front end gives {self.frontend.n_mels} mel bands, the model reads F = {model.F}")
        # int8: the windows are scored by integer inference (int8_depthwise / int8_fused: with its second / third level)
        self.net = model._open(config, levels)

    def close(self):
        self.net.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def score(self, wav, sr=None):
        """wav: CUDA float32 [n_samples] -> (t_start seconds float64 [n_windows], CUDA float32 probs [n_windows, classes]);
        window i starts at frame i * hop_frames, i.e. at ``i * hop_frames * hop / sr`` seconds of the front end's rate.
        ``sr``: the rate the recording arrives at; when it differs from the front end's, the recording is resampled to that
        rate first (``resample_poly``).  ``t_start`` is in seconds either way.  A non-positive or non-integer ``sr`` raises
        ValueError; None or the front end's own rate is the plain path."""
        fe = self.frontend
        wav = to_rate(wav, sr, fe.sr, "StreamScorer.score")
        feat = log_mel_stream(wav, fe)
        probs = self.net.predict_stream(feat, self.hop_frames, frontend_config=fe if fe.scale == "db" else None,
                                        mean=self.model.mean, scale=self.model.scale)
        t = np.arange(int(probs.shape[0]), dtype=np.float64) * (self.hop_frames * int(fe.hop)) / float(fe.sr)
        return t, probs


def smooth_posteriors(p, w: int) -> np.ndarray:
    """Causal moving average over windows: ``out[i] = mean(p[max(0, i - w + 1) : i + 1])`` (float64 [n, classes])."""
    p = np.asarray(p, np.float64)
    if p.ndim != 2:
        raise ValueError("smooth_posteriors expects [n_windows, classes]")
    if int(w) < 1:
        raise ValueError("w must be at least 1")
    out = np.empty_like(p)
    for i in range(len(p)):
        out[i] = p[max(0, i - int(w) + 1):i + 1].mean(axis=0)
    return out


def detect_events(t, p, threshold, keyword_classes: Sequence[int], refractory_windows: int) -> List[Tuple[float, int, float]]:
    """[(t[i], class, score)]: scan the windows in order; outside a refractory span, when the largest posterior among
    ``keyword_classes`` reaches ``threshold`` emit that class (ties: the lowest class id) and skip the next
    ``refractory_windows`` windows.  ``threshold`` is one scalar for every class, or one value per class -- a sequence of
    length ``classes``, ``TrainedModel.thresholds`` for one: each keyword class is then compared with its own threshold, and
    the emitted class is the largest posterior among those that reach theirs (ties: the lowest class id)."""
    t, p = np.asarray(t, np.float64).reshape(-1), np.asarray(p, np.float64)
    if p.ndim != 2 or len(t) != len(p):
        raise ValueError("detect_events expects t [n] and p [n, classes]")
    kw = sorted(set(int(c) for c in keyword_classes))
    if not kw or kw[0] < 0 or kw[-1] >= p.shape[1]:
        raise ValueError("keyword_classes must name classes of p")
    if int(refractory_windows) < 0:
        raise ValueError("refractory_windows must not be negative")
    events, i = [], 0
    if np.ndim(threshold) != 0:
        thr = np.asarray(threshold, np.float64).reshape(-1)
        if thr.size != p.shape[1]:
            raise ValueError(f"per-class thresholds must hold classes = {p.shape[1]} values")
        thr = thr[kw]
        while i < len(p):
            scores = p[i, kw]
            reach = scores >= thr
            if reach.any():
                j = int(np.argmax(np.where(reach, scores, -np.inf)))     # first maximum among those that reach = lowest class id
                events.append((float(t[i]), kw[j], float(scores[j])))
                i += 1 + int(refractory_windows)
            else:
                i += 1
        return events
    while i < len(p):
        scores = p[i, kw]
        j = int(np.argmax(scores))          # first maximum = lowest class id
        if scores[j] >= threshold:
            events.append((float(t[i]), kw[j], float(scores[j])))
            i += 1 + int(refractory_windows)
        else:
            i += 1
    return events
