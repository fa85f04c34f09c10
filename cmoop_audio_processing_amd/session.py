"""Single-candidate session over the C ABI (cmoop_net_*): used by the parity
tests, ``__graft_entry__.smoke()`` and small interactive checks."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib, genes as G
from .evaluator import EvalConfig


FROM_CONFIG = object()      # set_distill's default: the session's config.distill


class NetSession:
    def __init__(self, gene, config: EvalConfig, T: int, F: int, seed: int):
        self.gene = tuple(int(v) for v in gene)
        G.validate_gene(self.gene)
        self.config = config
        self._h = C.c_void_p()
        g = (C.c_int32 * 6)(*self.gene)
        cfg = config.to_struct()
        _lib.check(_lib.lib().cmoop_net_create(g, C.byref(cfg), C.c_int32(T), C.c_int32(F), C.c_uint32(seed & 0xFFFFFFFF),
                                               C.byref(self._h)))
        n = C.c_int64()
        _lib.check(_lib.lib().cmoop_net_total_params(self._h, C.byref(n)))
        self.n_params = int(n.value)
        self.T, self.F = int(T), int(F)
        self.augment = self.loss = self.optim = self.ema = self.opoint = self.quant = self.prune = self.act_quant = None
        self.int8 = False
        self.int8_depthwise = False
        self.int8_fused = False
        for name, setter in (("augment", self.set_augment), ("loss", self.set_loss), ("optim", self.set_optim),
                             ("ema", self.set_ema), ("operating_point", self.set_operating_point), ("quant", self.set_quant),
                             ("prune", self.set_prune), ("act_quant", self.set_act_quant)):
            if getattr(config, name, None) is not None:
                try:
                    setter(getattr(config, name))
                except Exception:
                    self.close()
                    raise
        self.distill, self._teacher_logits = None, None     # what the net trains against now (None: no distillation)
        self._distill_pending = bool(getattr(getattr(config, "distill", None), "enabled", False))   # config.distill waits for a table

    def _set(self, symbol: str, struct) -> None:
        """One ``cmoop_net_set_*`` call: None travels as NULL, a struct by reference."""
        _lib.check(getattr(_lib.lib(), symbol)(self._h, C.byref(struct) if struct is not None else None))

    def set_distill(self, distill=FROM_CONFIG, teacher_logits=None) -> None:
        """Knowledge distillation (``DistillConfig``) of every following train step of this net -- ``train_step``,
        ``run_epoch`` and ``fit`` alike -- against ``teacher_logits``, a contiguous CUDA float32 [n_train, classes] table
        of a teacher's logits of the rows those steps gather from (``predict_logits`` of the teacher); the session keeps it
        alive.  ``distill`` defaults to the constructor's ``config.distill``: ``set_distill(teacher_logits=table)`` is how
        that config is applied, a config alone having nothing to train against -- until then ``train_step``, ``run_epoch``
        and ``fit`` of a session whose ``config.distill`` is enabled raise rather than train without it.  None, alpha 0 or
        no table turns distillation off, and ``self.distill`` is then None.  Composes with ``set_loss`` and
        ``set_augment``; ``evaluate``, ``predict_*`` and the validation loss of ``fit`` stay the sparse cross-entropy."""
        from .distill import check_teacher_table
        if distill is FROM_CONFIG:
            distill = getattr(self.config, "distill", None)
        if distill is None:
            self._set("cmoop_net_set_distill", None)
            teacher_logits = None
        else:
            n_rows = 0
            if teacher_logits is not None:
                n_rows = int(getattr(teacher_logits, "shape", (0,))[0])
                check_teacher_table(teacher_logits, n_rows, int(self.config.classes))
            distill.check(int(self.config.classes), teacher_logits, n_rows)
            self._set("cmoop_net_set_distill", distill._struct(teacher_logits))
        on = distill is not None and distill.enabled and teacher_logits is not None
        self.distill, self._teacher_logits = (distill, teacher_logits) if on else (None, None)
        self._distill_pending = False

    def _require_teacher(self) -> None:
        if self._distill_pending:
            from .distill import require_teacher
            require_teacher(self.config.distill, None)

    def predict_logits(self, X):
        """X: CUDA float32 [n, T, F] -> CUDA float32 [n, classes]: the logits ``predict_proba`` takes the softmax of
        (``cmoop_softmax_probs`` of them is ``predict_proba(X)`` bit for bit)."""
        import torch
        if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 3):
            raise ValueError("predict_logits expects a CUDA float32 tensor [n, T, F]")
        if (int(X.shape[1]), int(X.shape[2])) != (self.T, self.F):
            raise ValueError(f"predict_logits: rows are {int(X.shape[1])} x {int(X.shape[2])}, the net reads {self.T} x {self.F}")
        X = X.contiguous()
        n = int(X.shape[0])
        out = torch.empty((n, int(self.config.classes)), dtype=torch.float32, device=X.device)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_predict_logits(self._h, _lib.ptr(X), C.c_int64(n), _lib.ptr(out)))
        return out

    def train_step_distill_targets(self, X_rows, t, q, alpha: float, temperature: float, w=None, primary=None) -> None:
        """``train_step_targets`` with a caller-built teacher row per batch row, q CUDA float32 [B, classes], and the
        distillation loss at (alpha, temperature), whatever ``set_distill`` says."""
        import torch
        B = int(X_rows.shape[0])
        Cn = int(self.config.classes)
        if tuple(X_rows.shape) != (B, self.T, self.F) or tuple(t.shape) != (B, Cn) or tuple(q.shape) != (B, Cn):
            raise ValueError(f"train_step_distill_targets: rows must be [B, {self.T}, {self.F}], targets and teacher rows [B, {Cn}]")
        for name, v, dt in (("X_rows", X_rows, torch.float32), ("t", t, torch.float32), ("q", q, torch.float32), ("w", w, torch.float32),
                            ("primary", primary, torch.int32)):
            if v is not None and not (v.is_cuda and v.dtype == dt and v.is_contiguous() and int(v.shape[0]) == B):
                raise ValueError(f"train_step_distill_targets: {name} must be a contiguous CUDA {dt} tensor of {B} rows")
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_train_step_distill_targets(self._h, _lib.ptr(X_rows), _lib.ptr(t), _lib.ptr(w), _lib.ptr(primary),
                                                                   _lib.ptr(q), float(alpha), float(temperature), C.c_int32(B)))

    def set_optim(self, optim) -> None:
        """Optimiser options (``OptimConfig``: learning-rate schedule, decoupled weight decay, gradient clipping) of every
        following train step of this net -- ``train_step``, ``run_epoch`` and ``fit`` alike -- from the next step on.  None
        or a config with everything off turns them off (``self.optim`` is then None), and the net steps bit for bit as one
        that never had any.  The schedule is a function of ``iterations``, so ``get_state`` / ``set_state`` carry it."""
        self._set("cmoop_net_set_optim", None if optim is None else optim.check()._struct())
        self.optim = optim if optim is not None and optim.enabled else None

    def set_ema(self, ema) -> None:
        """Weight EMA (``EmaConfig``) of every following train step of this net -- ``train_step``, ``run_epoch`` and ``fit``
        alike -- from the next step on.  The first enabled config makes the average a bit copy of the parameters; a later one
        keeps it.  None or momentum 0 turns it off (``self.ema`` is then None), and the net steps bit for bit as one that
        never had any.  ``fit`` then validates, early-stops and reads out on the average and leaves ``get_params()`` equal to
        the weights that were scored.  ``set_state`` does not touch the average: ``set_ema_params`` does."""
        self._set("cmoop_net_set_ema", None if ema is None else ema.check()._struct())
        self.ema = ema if ema is not None and ema.enabled else None

    def get_ema(self) -> np.ndarray:
        """The average arena, in ``get_params``' layout; raises when the net has no average."""
        out = np.empty(self.n_params, np.float32)
        _lib.check(_lib.lib().cmoop_net_get_ema(self._h, _lib.ptr(out)))
        return out

    def set_ema_params(self, flat) -> None:
        flat = np.ascontiguousarray(flat, np.float32)
        assert flat.size == self.n_params
        _lib.check(_lib.lib().cmoop_net_set_ema_params(self._h, _lib.ptr(flat)))

    def use_ema(self, on) -> None:
        """While on, ``evaluate`` / ``predict_proba`` / ``predict_logits`` / ``predict_stream`` read the average in place of
        the parameters (no copy).  Turn it off again before the next train step: a step refuses otherwise."""
        _lib.check(_lib.lib().cmoop_net_use_ema(self._h, C.c_int32(int(bool(on)))))

    def finalize_ema(self) -> None:
        """parameters := average (Keras' ``finalize_variable_values``); ``fit`` does this itself."""
        _lib.check(_lib.lib().cmoop_net_finalize_ema(self._h))

    def set_operating_point(self, opoint) -> None:
        """Operating-point read-out (``OperatingPointConfig``) of every following ``fit`` of this net.  None or recall 0 turns
        it off (``self.opoint`` is then None), and ``fit`` is launch for launch the one of a net that never had it.  On, ``fit``
        changes none of its numbers and gains the key ``"operating_point"``: after the weights are final, one more inference
        pass over the validation split and the read-out of it (``operating_point`` below, at the config's recall)."""
        self._set("cmoop_net_set_opoint", None if opoint is None else opoint.check()._struct())
        self.opoint = opoint if opoint is not None and opoint.enabled else None

    def operating_point(self, X, y, recall=None) -> dict:
        """X: CUDA float32 [n, T, F], y: CUDA int32 [n] -> the read-out of ``predict_proba(X)`` against ``y`` at ``recall``
        (default: the recall of ``set_operating_point``): dict(thresholds float32 [classes], tp, fp, positives, negatives, k
        int32 [classes], u2 int64 [classes], fpr_at_recall, recall_achieved, auc, classes_scored, summary float64 [4]).
        Equal, value for value, to ``opoint.operating_point_reference(predict_proba(X), y, recall)``."""
        import torch
        from . import opoint as OP
        if recall is None:
            if self.opoint is None:
                raise ValueError("operating_point: no recall given and the session has no operating-point config")
            recall = self.opoint.recall
        if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 3):
            raise ValueError("operating_point expects a CUDA float32 tensor [n, T, F]")
        if (int(X.shape[1]), int(X.shape[2])) != (self.T, self.F):
            raise ValueError(f"operating_point: rows are {int(X.shape[1])} x {int(X.shape[2])}, the net reads {self.T} x {self.F}")
        if not (isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.int32 and y.dim() == 1 and len(y) == len(X)):
            raise ValueError("operating_point expects CUDA int32 labels [n]")
        X, y = X.contiguous(), y.contiguous()
        st = OP.OperatingPointConfig(recall=float(recall)).check()._struct()
        rec, summary = (_lib.OpointClass * int(self.config.classes))(), (C.c_double * 4)()
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_operating_point(self._h, _lib.ptr(X), _lib.ptr(y), C.c_int64(len(X)), C.byref(st), rec, summary))
        return OP.from_records(rec, summary)

    def last_operating_point(self) -> dict:
        """The read-out the last ``fit`` recorded (``cmoop_net_last_opoint``); raises when that fit ran without the option."""
        from . import opoint as OP
        rec, summary = (_lib.OpointClass * int(self.config.classes))(), (C.c_double * 4)()
        _lib.check(_lib.lib().cmoop_net_last_opoint(self._h, rec, summary))
        return OP.from_records(rec, summary)

    def set_quant(self, quant) -> None:
        """Quantisation-aware training (``QuantConfig``) of every following train step and inference call of this net.  None
        or bits 0 turns it off (``self.quant`` is then None), and the net is bit for bit one that never had it.  On, every
        train step first quantises the latent kernels and runs forward and backward on them (the gradients go unchanged to the
        latent weights), and ``evaluate`` / ``predict_proba`` / ``predict_logits`` / ``predict_stream`` quantise the arena they
        read first; ``get_params`` / ``set_params`` / ``get_state`` keep meaning the latent fp32 weights.  Switched on after a
        plain fit it is post-training quantisation."""
        self._set("cmoop_net_set_quant", None if quant is None else quant.check()._struct())
        self.quant = quant if quant is not None and quant.enabled else None
        self._int8_needs(self.quant)                    # the net drops integer inference with its weight codes

    def get_quantized(self):
        """(wq_params float32 [n_params]: kernels dequantised, every other element a copy; codes int8 [n_params]: 0 outside
        the kernel tensors; scales float32 [total channels]) of the arena inference would read now; raises while the option is
        off.  Equal, bit for bit, to ``quant.quantize_params_ref`` of that arena."""
        from . import quant as Q
        v = G.VARIANT_NAMES[self.config.variant]
        channels = sum(r[1] for r in Q.quant_table(self.gene, v, int(self.config.classes)))
        wq, codes, scales = np.empty(self.n_params, np.float32), np.empty(self.n_params, np.int8), np.empty(channels, np.float32)
        _lib.check(_lib.lib().cmoop_net_get_quantized(self._h, _lib.ptr(wq), _lib.ptr(codes), _lib.ptr(scales)))
        return wq, codes, scales

    def set_prune(self, prune) -> None:
        """Magnitude pruning (``PruneConfig``) of every following train step and inference call of this net.  None or sparsity
        0 turns it off (``self.prune`` is then None), and the net is bit for bit one that never had it.  On, every train step
        first prunes the latent kernels at ``prune.sparsity_at(cfg, iteration)`` and runs forward and backward on them (the
        gradients go unchanged to the dense latent weights), and ``evaluate`` / ``predict_proba`` / ``predict_logits`` /
        ``predict_stream`` prune the arena they read at the final sparsity; with ``set_quant`` on as well the pruned kernels
        are quantised.  ``get_params`` / ``set_params`` / ``get_state`` keep meaning the latent fp32 weights.  Switched on after
        a plain fit it is one-shot magnitude pruning."""
        self._set("cmoop_net_set_prune", None if prune is None else prune.check()._struct())
        self.prune = prune if prune is not None and prune.enabled else None

    def get_pruned(self):
        """(w_eff float32 [n_params]: the arena inference would read now pruned at the final sparsity, not quantised, every
        element outside the pruned tensors a copy; zeros uint32 [kernel tensors]: the elements of each tensor that became
        zero); raises while the option is off.  Equal, bit for bit, to ``prune.prune_params_ref`` of that arena."""
        from . import prune as PR
        v = G.VARIANT_NAMES[self.config.variant]
        rows = len(PR.prune_table(self.gene, v, int(self.config.classes)))
        w, zeros = np.empty(self.n_params, np.float32), np.empty(rows, np.uint32)
        _lib.check(_lib.lib().cmoop_net_get_pruned(self._h, _lib.ptr(w), _lib.ptr(zeros)))
        return w, zeros

    def set_act_quant(self, act_quant) -> None:
        """Activation fake quantisation (``quant.ActQuantConfig``) of every following train step and inference call of this
        net.  None or bits 0 turns it off (``self.act_quant`` is then None), and the net is bit for bit one that never had it.
        On, the forward pass quantises every site (``quant.act_sites``) in place: train steps with the batch's own range, which
        they also track, inference with the tracked range -- refused until a train step has run or ``set_act_ranges`` loaded
        some.  ``get_state`` / ``set_state`` do not carry the ranges: ``get_act_ranges`` / ``set_act_ranges`` do."""
        self._set("cmoop_net_set_actquant", None if act_quant is None else act_quant.check()._struct())
        self.act_quant = act_quant if act_quant is not None and act_quant.enabled else None
        self._int8_needs(self.act_quant)                # ... and with its activation codes

    def _int8_needs(self, option) -> None:
        """Dropping ``quant`` or ``act_quant`` drops every level of integer inference in the net: the mirrors follow."""
        if option is None:
            self.int8 = self.int8_depthwise = self.int8_fused = False

    # set_int8's refusals of a level without `on` (quant.Int8Levels.of)
    _INT8_LEVEL_REFUSALS = ("depthwise=True needs on=True: integer depthwise is a level of integer inference",
                            "fused=True needs on=True: the requantising epilogue is a level of integer inference")

    def set_int8(self, on, depthwise: bool = False, fused: bool = False) -> None:
        """Integer inference (``cmoop_net_set_int8``) of every following ``evaluate`` / ``predict_*`` call: every conv and dense
        op whose input is an activation-quantisation site (``int8_ops``) runs on int8 codes with exact int32 accumulation
        (``quant.conv_i8_ref`` / ``dense_i8_ref``); train steps never do.  Turning it on raises, and leaves the net as it was,
        unless ``set_quant`` and ``set_act_quant`` are both on, the ranges are ready and every range and weight scale is
        finite.  Off (the default), every launch and byte is that of a net that never had it.  ``depthwise``: the second level
        (``cmoop_net_set_int8_depthwise``; it needs ``on``): every depthwise op (``int8_dw_ops``) is one launch on the codes
        that also applies the quantiser of the site it writes (``quant.dwconv_i8_ref``).  False -- the default -- is
        ``set_int8(on)`` as it always was; a net without a depthwise op accepts it and nothing changes.  ``fused``: the third
        level (``cmoop_net_set_int8_fused``; it needs ``on`` and is independent of ``depthwise``): every op of
        ``int8_fused_ops`` is one launch that also applies the eval BatchNorm after it and the quantiser of the site it reaches
        (``quant.conv_i8_q_ref`` / ``dense_i8_q_ref``), with the bytes of the launches it replaces.  False is the default; a
        net without a fusible op accepts it and nothing changes."""
        from .quant import Int8Levels
        lv = Int8Levels.of(on, depthwise, fused, self._INT8_LEVEL_REFUSALS)
        L = _lib.lib()
        if not lv.fused:
            _lib.check(L.cmoop_net_set_int8_fused(self._h, C.c_int32(0)))
            self.int8_fused = False
        if not lv.depthwise:                             # the level goes first: turning integer inference off drops it anyway
            _lib.check(L.cmoop_net_set_int8_depthwise(self._h, C.c_int32(0)))
            self.int8_depthwise = False
        _lib.check(L.cmoop_net_set_int8(self._h, C.c_int32(int(lv.on))))
        self.int8 = lv.on
        if lv.depthwise:
            _lib.check(L.cmoop_net_set_int8_depthwise(self._h, C.c_int32(1)))
            self.int8_depthwise = True
        if lv.fused:
            _lib.check(L.cmoop_net_set_int8_fused(self._h, C.c_int32(1)))
            self.int8_fused = True

    def int8_ops(self):
        """``cmoop_net_int8_ops``: the ops that run integer under ``set_int8``, dicts keyed by ``quant.INT8_OP_FIELDS``."""
        from .quant import INT8_OP_FIELDS
        return self._plan_rows("cmoop_net_int8_ops", INT8_OP_FIELDS, 16)

    def int8_dw_ops(self):
        """``cmoop_net_int8_dw_ops``: the depthwise ops that run integer under ``set_int8(True, depthwise=True)``, dicts keyed
        by ``quant.INT8_DW_OP_FIELDS``; empty for variants A / B."""
        from .quant import INT8_DW_OP_FIELDS
        return self._plan_rows("cmoop_net_int8_dw_ops", INT8_DW_OP_FIELDS, 16)

    def int8_fused_ops(self):
        """``cmoop_net_int8_fused_ops``: the ops that take the requantising epilogue under ``set_int8(True, fused=True)``, dicts
        keyed by ``quant.INT8_FUSED_OP_FIELDS``."""
        from .quant import INT8_FUSED_OP_FIELDS
        return self._plan_rows("cmoop_net_int8_fused_ops", INT8_FUSED_OP_FIELDS, 20)

    def _plan_rows(self, entry: str, fields, width: int):
        """The rows of this net's plan at one level of integer inference (``cmoop_net_int8*_ops`` by name; ``width`` int64
        columns each), keyed by ``fields``."""
        from . import quant as Q
        cap = 64
        rows, n = np.zeros((cap, width), np.int64), C.c_int32()
        _lib.check(getattr(_lib.lib(), entry)(self._h, _lib.ptr(rows), C.c_int32(cap), C.byref(n)))
        return Q._plan_rows(fields, rows, n.value)

    def _n_sites(self) -> int:
        n = C.c_int32()                                  # the net's own count: the session cannot disagree with what it wraps
        _lib.check(_lib.lib().cmoop_net_get_act_ranges(self._h, None, C.c_int32(0), C.byref(n)))
        return int(n.value)

    def get_act_ranges(self) -> np.ndarray:
        """The site records, a structured array [sites] of (m_b, r, count, reserved) in site order; raises while the net has
        none (the option was never on)."""
        from . import quant as Q
        out, n = np.zeros(self._n_sites(), Q.ACT_RANGE_DTYPE), C.c_int32()
        _lib.check(_lib.lib().cmoop_net_get_act_ranges(self._h, _lib.ptr(out), C.c_int32(len(out)), C.byref(n)))
        assert n.value == len(out)
        return out

    def set_act_ranges(self, ranges) -> None:
        """Loads site records as ``get_act_ranges`` gives them; inference is possible once every count is positive."""
        from . import quant as Q
        ranges = np.ascontiguousarray(ranges, Q.ACT_RANGE_DTYPE).reshape(-1)
        _lib.check(_lib.lib().cmoop_net_set_act_ranges(self._h, _lib.ptr(ranges), C.c_int32(len(ranges))))

    def act_dims(self, i: int):
        """(H, W, C, materialised, has a gradient, number of acts) of act ``i`` of the plan (debug read-out)."""
        dims = (C.c_int32 * 6)()
        _lib.check(_lib.lib().cmoop_net_get_act(self._h, C.c_int32(int(i)), C.c_int32(0), dims, None, None))
        return tuple(int(v) for v in dims)

    def get_act(self, i: int, B: int, grad: bool = False):
        """Debug read-out: float32 [B, H, W, C] of act ``i`` as the last step or pass left it (``grad``: its gradient)."""
        H, W, Cn = self.act_dims(i)[:3]
        out = np.empty((int(B), H, W, Cn), np.float32)
        _lib.check(_lib.lib().cmoop_net_get_act(self._h, C.c_int32(int(i)), C.c_int32(int(B)), None, None if grad else _lib.ptr(out),
                                                _lib.ptr(out) if grad else None))
        return out

    def optim_stats(self) -> dict:
        """The last train step's optimiser read-out: dict(sumsq, norm, scale, path) -- the float64 sum of squares of the
        trainable gradients as the device summed it, the float32 norm and clip scale, and the launch path (0: the fused
        launch, which computes no norm and reports 0, 0, 1; 1: finish + update)."""
        out = (C.c_double * 4)()
        _lib.check(_lib.lib().cmoop_net_optim_stats(self._h, out))
        return dict(sumsq=float(out[0]), norm=float(out[1]), scale=float(out[2]), path=int(out[3]))

    def set_loss(self, loss) -> None:
        """Soft-target training loss (``LossConfig``: mixup, label smoothing, class weights) of every following train step
        of this net -- ``train_step``, ``run_epoch`` and ``fit`` alike; None or a config that does nothing turns it off.
        ``evaluate``, ``predict_proba``, ``predict_stream`` and the validation loss of ``fit`` stay the sparse cross-entropy;
        ``train_metrics`` then reports the weighted soft-target loss sum and the rows whose arg max is their own label."""
        self._set("cmoop_net_set_loss", None if loss is None else loss.check(int(self.config.classes))._struct())
        self.loss = loss

    def loss_buffers(self):
        """dict(mix, t, w, primary): floats the net has allocated for the training loss (0: that buffer does not exist)."""
        out = (C.c_int64 * 4)()
        _lib.check(_lib.lib().cmoop_net_loss_buffers(self._h, out))
        return dict(zip(("mix", "t", "w", "primary"), (int(v) for v in out)))

    def train_step_targets(self, X_rows, t, w=None, primary=None) -> None:
        """One optimiser step on caller-built rows and targets: X_rows CUDA float32 [B, T, F], t CUDA float32 [B, classes]
        (rows of a distribution), w CUDA float32 [B] or None (1), primary CUDA int32 [B] or None (arg max of t: the class a
        row counts as correct for).  No augmentation, no mixing, no target construction; dropout, Adam and the counters
        advance as in ``train_step``.  The hook for soft targets from elsewhere, a teacher's probabilities for one."""
        import torch
        B = int(X_rows.shape[0])
        if tuple(X_rows.shape) != (B, self.T, self.F) or tuple(t.shape) != (B, int(self.config.classes)):
            raise ValueError(f"train_step_targets: rows must be [B, {self.T}, {self.F}] and targets [B, {int(self.config.classes)}]")
        for name, v, dt in (("X_rows", X_rows, torch.float32), ("t", t, torch.float32), ("w", w, torch.float32), ("primary", primary, torch.int32)):
            if v is not None and not (v.is_cuda and v.dtype == dt and v.is_contiguous() and int(v.shape[0]) == B):
                raise ValueError(f"train_step_targets: {name} must be a contiguous CUDA {dt} tensor of {B} rows")
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_train_step_targets(self._h, _lib.ptr(X_rows), _lib.ptr(t), _lib.ptr(w), _lib.ptr(primary),
                                                           C.c_int32(B)))

    def set_augment(self, augment) -> None:
        """Train-time augmentation (``AugmentConfig``) of every following train step of this net -- ``train_step``,
        ``run_epoch`` and ``fit`` alike; None or a config that does nothing turns it off.  ``evaluate``, ``predict_proba``
        and ``predict_stream`` never augment; ``train_metrics`` then reports the loss and accuracy of the augmented batches."""
        self._set("cmoop_net_set_augment", None if augment is None else augment.check(self.T, self.F)._struct())
        self.augment = augment

    def close(self):
        if self._h:
            _lib.check(_lib.lib().cmoop_net_destroy(self._h))
            self._h = C.c_void_p()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get_params(self) -> np.ndarray:
        out = np.empty(self.n_params, np.float32)
        _lib.check(_lib.lib().cmoop_net_get_params(self._h, _lib.ptr(out)))
        return out

    def set_params(self, flat) -> None:
        flat = np.ascontiguousarray(flat, np.float32)
        assert flat.size == self.n_params
        _lib.check(_lib.lib().cmoop_net_set_params(self._h, _lib.ptr(flat)))

    def get_grads(self) -> np.ndarray:
        out = np.empty(self.n_params, np.float32)
        _lib.check(_lib.lib().cmoop_net_get_grads(self._h, _lib.ptr(out)))
        return out

    def train_step(self, X, y, idx=None, row0: int = 0, B: int = None) -> None:
        """X: CUDA float32 [N,T,F]; y: CUDA int32 [N]; idx: CUDA int32 permutation or None."""
        self._require_teacher()
        import torch
        torch.cuda.synchronize()
        if B is None:
            B = int(len(idx) if idx is not None else len(X)) - row0
        _lib.check(_lib.lib().cmoop_net_train_step(self._h, _lib.ptr(X), _lib.ptr(y), _lib.ptr(idx), C.c_int64(row0), C.c_int32(B)))

    def evaluate(self, X, y):
        """-> (mean loss, accuracy, int32 CUDA predictions)."""
        import torch
        torch.cuda.synchronize()
        n = int(len(X))
        preds = torch.empty(n, dtype=torch.int32, device=X.device)
        ls, corr = C.c_double(), C.c_int64()
        _lib.check(_lib.lib().cmoop_net_evaluate(self._h, _lib.ptr(X), _lib.ptr(y), C.c_int64(n), C.byref(ls), C.byref(corr), _lib.ptr(preds)))
        return ls.value / max(n, 1), corr.value / max(n, 1), preds

    # -- Model.predict: probabilities of rows, and of the overlapping windows of a feature stream ------------------
    def predict_proba(self, X):
        """X: CUDA float32 [n, T, F] -> CUDA float32 [n, classes], inference mode, ``eval_batch`` rows per launch.
        Row r's arg max is the prediction ``evaluate`` returns for it (the same softmax arithmetic)."""
        import torch
        if not (isinstance(X, torch.Tensor) and X.is_cuda and X.dtype == torch.float32 and X.dim() == 3):
            raise ValueError("predict_proba expects a CUDA float32 tensor [n, T, F]")
        if (int(X.shape[1]), int(X.shape[2])) != (self.T, self.F):
            raise ValueError(f"predict_proba: rows are {int(X.shape[1])} x {int(X.shape[2])}, the net reads {self.T} x {self.F}")
        X = X.contiguous()
        n = int(X.shape[0])
        probs = torch.empty((n, int(self.config.classes)), dtype=torch.float32, device=X.device)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_predict(self._h, _lib.ptr(X), C.c_int64(n), _lib.ptr(probs)))
        return probs

    def predict_stream(self, feat, hop_frames: int, frontend_config=None, mean=None, scale=None):
        """feat: CUDA float32 [n_frames, F] (``log_mel_stream``) -> CUDA float32 [n_windows, classes].

        Window i is rows [i * hop_frames, i * hop_frames + T).  Per window: with a dB-scale ``frontend_config`` its own
        reference / top_db floor first (``feat`` then holds the un-referenced dB values ``log_mel_stream`` gives), then
        ``(v - mean) / scale`` when the StandardScaler's float64 ``mean`` and ``scale`` [F] are given, then forward and
        softmax.  ``feat`` is only read; memory is one ``eval_batch`` chunk of windows however long the stream is."""
        import torch
        if not (isinstance(feat, torch.Tensor) and feat.is_cuda and feat.dtype == torch.float32 and feat.dim() == 2):
            raise ValueError("predict_stream expects a CUDA float32 tensor [n_frames, F]")
        if int(feat.shape[1]) != self.F:
            raise ValueError(f"predict_stream: the stream has {int(feat.shape[1])} features per frame, the net reads {self.F}")
        if (mean is None) != (scale is None):
            raise ValueError("predict_stream: mean and scale come together (both or neither)")
        if mean is not None:
            mean, scale = np.ascontiguousarray(mean, np.float64).reshape(-1), np.ascontiguousarray(scale, np.float64).reshape(-1)
            if mean.size != self.F or scale.size != self.F:
                raise ValueError(f"predict_stream: mean and scale must hold {self.F} values each")
        feat = feat.contiguous()
        n_frames, nw = int(feat.shape[0]), C.c_int64()
        _lib.check(_lib.lib().cmoop_stream_windows(C.c_int64(n_frames), C.c_int32(self.T), C.c_int32(int(hop_frames)), C.byref(nw)))
        st = frontend_config._struct() if frontend_config is not None else None
        probs = torch.empty((int(nw.value), int(self.config.classes)), dtype=torch.float32, device=feat.device)
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_predict_stream(self._h, _lib.ptr(feat), C.c_int64(n_frames), C.c_int32(int(hop_frames)),
                                                       C.byref(st) if st is not None else None, _lib.ptr(mean), _lib.ptr(scale),
                                                       _lib.ptr(probs)))
        return probs

    # -- full training state / epoch-granular driving (re-synchronised parity tests) -----------------------------
    def get_state(self):
        """-> dict(params, m, v, iterations, steps): parameters in canonical order incl. BatchNorm moving statistics,
        Adam's moments in the same layout, optimizer.iterations, global train-step count (dropout counter)."""
        p, m, v = (np.empty(self.n_params, np.float32) for _ in range(3))
        it, st = C.c_int64(), C.c_int64()
        _lib.check(_lib.lib().cmoop_net_get_state(self._h, _lib.ptr(p), _lib.ptr(m), _lib.ptr(v), C.byref(it), C.byref(st)))
        return {"params": p, "m": m, "v": v, "iterations": int(it.value), "steps": int(st.value)}

    def set_state(self, state) -> None:
        p, m, v = (np.ascontiguousarray(state[k], np.float32) for k in ("params", "m", "v"))
        assert p.size == m.size == v.size == self.n_params
        _lib.check(_lib.lib().cmoop_net_set_state(self._h, _lib.ptr(p), _lib.ptr(m), _lib.ptr(v),
                                                  C.c_int64(int(state["iterations"])), C.c_int64(int(state["steps"]))))

    def set_gather_rows(self, n_rows: int) -> None:
        _lib.check(_lib.lib().cmoop_net_set_gather_rows(self._h, C.c_int64(int(n_rows))))

    def run_epoch(self, X, y, epoch: int) -> None:
        """One epoch of Model.fit on the trainer's own path (device permutation, device step state)."""
        self._require_teacher()
        import torch
        torch.cuda.synchronize()
        _lib.check(_lib.lib().cmoop_net_run_epoch(self._h, _lib.ptr(X), _lib.ptr(y), C.c_int64(len(X)), C.c_int32(int(epoch))))

    def fit(self, X_train, y_train, X_val, y_val):
        """evaluate_individual's fit + read-outs on this net -> dict(acc, fpr, val_loss, epochs_run, best_epoch,
        val_loss_history, val_accuracy_history), and ``operating_point`` (the dict of ``operating_point``, of the validation
        split under the final weights) when ``set_operating_point`` is on."""
        self._require_teacher()
        import torch
        torch.cuda.synchronize()
        d = _lib.DatasetStruct()
        d.x_train, d.y_train, d.n_train = X_train.data_ptr(), y_train.data_ptr(), len(X_train)
        d.x_val, d.y_val, d.n_val = X_val.data_ptr(), y_val.data_ptr(), len(X_val)
        d.T, d.F = int(X_train.shape[1]), int(X_train.shape[2])
        cap = max(1, int(self.config.epochs))
        hl, ha = np.full(cap, np.nan), np.full(cap, np.nan)
        ep, be = C.c_int32(), C.c_int32()
        acc, fpr, vl = C.c_double(), C.c_double(), C.c_double()
        _lib.check(_lib.lib().cmoop_net_fit(self._h, C.byref(d), C.c_int32(cap), _lib.ptr(hl), _lib.ptr(ha), C.byref(ep), C.byref(be),
                                            C.byref(acc), C.byref(fpr), C.byref(vl)))
        n = int(ep.value)
        out = {"acc": acc.value, "fpr": fpr.value, "val_loss": vl.value, "epochs_run": n, "best_epoch": int(be.value),
               "val_loss_history": hl[:n].copy(), "val_accuracy_history": ha[:n].copy()}
        if self.opoint is not None:
            out["operating_point"] = self.last_operating_point()
        return out

    def train_metrics(self, reset=True):
        ls, corr = C.c_double(), C.c_int64()
        _lib.check(_lib.lib().cmoop_net_train_metrics(self._h, C.byref(ls), C.byref(corr), C.c_int32(int(reset))))
        return ls.value, int(corr.value)


def epoch_permutation(seed: int, epoch: int, n: int) -> np.ndarray:
    out = np.empty(n, np.int32)
    _lib.check(_lib.lib().cmoop_epoch_permutation(C.c_uint32(seed & 0xFFFFFFFF), C.c_uint32(epoch), C.c_int64(n), _lib.ptr(out)))
    return out
