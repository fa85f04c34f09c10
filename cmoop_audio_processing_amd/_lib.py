"""ctypes binding of libcmoop_hip.so (include/cmoop.h).

There is NO CPU fallback: if the HIP library is missing or a call fails the
product path raises.  ``build()`` compiles the library in-tree with hipcc for
gfx950 (works without a GPU); loading it needs libamdhip64 only.
"""
from __future__ import annotations

import ctypes as C
import os
import re
import subprocess
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(_HERE, "csrc")
LIB_PATH = os.environ.get("CMOOP_LIB_PATH") or os.path.join(CSRC, "libcmoop_hip.so")   # override: A/B kernel builds
HEADER = os.path.join(os.path.dirname(_HERE), "include", "cmoop.h")

_lock = threading.Lock()
_lib = None


class CmoopError(RuntimeError):
    pass


class Config(C.Structure):
    """cmoop_config (include/cmoop.h)."""
    _fields_ = [(n, C.c_int32) for n in (
        "variant", "classes", "epochs", "batch", "patience", "early_stop", "restore_best", "acc_readout",
        "fpr_variant", "shuffle", "eval_batch", "n_slots", "profile_every", "gemm_mode")] + \
        [(n, C.c_double) for n in ("lr", "beta1", "beta2", "adam_eps", "bn_eps", "bn_momentum", "dropout")]


class DatasetStruct(C.Structure):
    """cmoop_dataset (include/cmoop.h)."""
    _fields_ = [("x_train", C.c_void_p), ("y_train", C.c_void_p), ("n_train", C.c_int64),
                ("x_val", C.c_void_p), ("y_val", C.c_void_p), ("n_val", C.c_int64),
                ("T", C.c_int32), ("F", C.c_int32)]


class Augment(C.Structure):
    """cmoop_augment (include/cmoop.h), 48 bytes."""
    _fields_ = [(n, C.c_int32) for n in ("time_shift", "time_masks", "time_mask_max", "freq_masks", "freq_mask_max", "reserved")] + \
        [(n, C.c_double) for n in ("p", "noise_std", "fill")]


class Loss(C.Structure):
    """cmoop_loss (include/cmoop.h), 40 bytes."""
    _fields_ = [("label_smoothing", C.c_double), ("mixup_alpha", C.c_double), ("mixup_p", C.c_double),
                ("class_weight", C.c_void_p), ("n_class_weight", C.c_int32), ("reserved", C.c_int32)]


class Distill(C.Structure):
    """cmoop_distill (include/cmoop.h), 32 bytes."""
    _fields_ = [("alpha", C.c_double), ("temperature", C.c_double), ("teacher_logits_dev", C.c_void_p), ("n_rows", C.c_int64)]


class Optim(C.Structure):
    """cmoop_optim (include/cmoop.h), 224 bytes."""
    _fields_ = [("weight_decay", C.c_double), ("global_clipnorm", C.c_double), ("clipvalue", C.c_double), ("warmup_start", C.c_double),
                ("alpha", C.c_double), ("decay_rate", C.c_double), ("values", C.c_double * 9), ("warmup_steps", C.c_int64),
                ("decay_steps", C.c_int64), ("boundaries", C.c_int64 * 8), ("schedule", C.c_int32), ("staircase", C.c_int32),
                ("decay_mask", C.c_int32), ("n_boundaries", C.c_int32), ("reserved", C.c_int32 * 2)]


class Ema(C.Structure):
    """cmoop_ema (include/cmoop.h), 16 bytes."""
    _fields_ = [("momentum", C.c_double), ("warmup", C.c_int32), ("reserved", C.c_int32)]


class Opoint(C.Structure):
    """cmoop_opoint (include/cmoop.h), 16 bytes."""
    _fields_ = [("recall", C.c_double), ("objective", C.c_int32), ("reserved", C.c_int32)]


class Quant(C.Structure):
    """cmoop_quant (include/cmoop.h), 16 bytes."""
    _fields_ = [("bits", C.c_int32), ("objective", C.c_int32), ("reserved", C.c_int32 * 2)]


class Prune(C.Structure):
    """cmoop_prune (include/cmoop.h), 24 bytes."""
    _fields_ = [("sparsity", C.c_double), ("begin_step", C.c_int32), ("end_step", C.c_int32), ("objective", C.c_int32),
                ("skip_small", C.c_int32)]


class ActQuant(C.Structure):
    """cmoop_actquant (include/cmoop.h), 16 bytes."""
    _fields_ = [("bits", C.c_int32), ("momentum", C.c_float), ("reserved", C.c_int32 * 2)]


class ActRange(C.Structure):
    """cmoop_act_range (include/cmoop.h), 16 bytes."""
    _fields_ = [("m_b", C.c_float), ("r", C.c_float), ("count", C.c_int32), ("reserved", C.c_int32)]


class OpointClass(C.Structure):
    """cmoop_opoint_class (include/cmoop.h), 32 bytes."""
    _fields_ = [("u2", C.c_int64), ("P", C.c_int32), ("N", C.c_int32), ("k", C.c_int32), ("tp", C.c_int32), ("fp", C.c_int32),
                ("thr", C.c_float)]


#: cmoop_next_fn (include/cmoop.h): int32_t (*)(void* ctx)
NEXT_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p)


#: prototypes of the scoring entry points (include/cmoop.h); pointers travel as void*, None is NULL
STREAM_PROTOTYPES = {
    "cmoop_net_predict": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "cmoop_logmel_stream": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "cmoop_logmel_stream_time": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_stream_windows": [C.c_int64, C.c_int32, C.c_int32, C.c_void_p],
    "cmoop_net_predict_stream": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
}


#: prototypes of the train-time augmentation entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
AUGMENT_PROTOTYPES = {
    "cmoop_augment_default": [C.c_void_p],
    "cmoop_augment_check": [C.c_void_p, C.c_int32, C.c_int32],
    "cmoop_augment_draws": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
    "cmoop_augment_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                            C.c_void_p],
    "cmoop_net_set_augment": [C.c_void_p, C.c_void_p],
    "cmoop_eval_population_aug": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p] +
                                 [C.c_void_p] * 7,
}


#: prototypes of the soft-target training loss entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
LOSS_PROTOTYPES = {
    "cmoop_loss_default": [C.c_void_p],
    "cmoop_loss_check": [C.c_void_p, C.c_int32],
    "cmoop_mixup_table": [C.c_double, C.c_void_p],
    "cmoop_mixup_draws": [C.c_void_p, C.c_uint32, C.c_uint32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_mixup_batch": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                          C.c_void_p],
    "cmoop_soft_targets": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_uint32, C.c_uint32,
                           C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_softmax_ce_soft": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_net_set_loss": [C.c_void_p, C.c_void_p],
    "cmoop_net_train_step_targets": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32],
    "cmoop_net_loss_buffers": [C.c_void_p, C.c_void_p],
    "cmoop_eval_population_ex": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p] +
                                [C.c_void_p] * 7,
}


#: prototypes of the knowledge-distillation entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
DISTILL_PROTOTYPES = {
    "cmoop_distill_default": [C.c_void_p],
    "cmoop_distill_check": [C.c_void_p, C.c_int32, C.c_int64],
    "cmoop_teacher_targets": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_double, C.c_uint32,
                              C.c_uint32, C.c_void_p],
    "cmoop_softmax_ce_distill": [C.c_void_p] * 5 + [C.c_double, C.c_double, C.c_int32, C.c_int32] + [C.c_void_p] * 3,
    "cmoop_net_set_distill": [C.c_void_p, C.c_void_p],
    "cmoop_net_train_step_distill_targets": [C.c_void_p] * 6 + [C.c_double, C.c_double, C.c_int32],
    "cmoop_net_predict_logits": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "cmoop_eval_population_kd": [C.c_void_p] * 7 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 7,
}


#: prototypes of the optimiser-option entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
OPTIM_PROTOTYPES = {
    "cmoop_optim_default": [C.c_void_p],
    "cmoop_optim_check": [C.c_void_p],
    "cmoop_optim_rates": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_param_kinds": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int64],
    "cmoop_grad_finish": [C.c_void_p, C.c_void_p, C.c_int32] + [C.c_void_p] * 6 + [C.c_double, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
    "cmoop_adamw": [C.c_void_p] * 5 + [C.c_int64, C.c_void_p] + [C.c_double] * 6 + [C.c_int32, C.c_double],
    "cmoop_net_set_optim": [C.c_void_p, C.c_void_p],
    "cmoop_net_optim_stats": [C.c_void_p, C.c_void_p],
    "cmoop_eval_population_opt": [C.c_void_p] * 8 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 7,
}


#: prototypes of the weight-EMA entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
EMA_PROTOTYPES = {
    "cmoop_ema_default": [C.c_void_p],
    "cmoop_ema_check": [C.c_void_p],
    "cmoop_ema_rates": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_ema_update": [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64],
    "cmoop_net_set_ema": [C.c_void_p, C.c_void_p],
    "cmoop_net_get_ema": [C.c_void_p, C.c_void_p],
    "cmoop_net_set_ema_params": [C.c_void_p, C.c_void_p],
    "cmoop_net_use_ema": [C.c_void_p, C.c_int32],
    "cmoop_net_finalize_ema": [C.c_void_p],
    "cmoop_eval_population_avg": [C.c_void_p] * 9 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 7,
}


#: prototypes of the operating-point entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
OPOINT_PROTOTYPES = {
    "cmoop_opoint_default": [C.c_void_p],
    "cmoop_opoint_check": [C.c_void_p],
    "cmoop_roc_counts": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p],
    "cmoop_operating_point": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_opoint_summary": [C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_operating_point_time": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_net_set_opoint": [C.c_void_p, C.c_void_p],
    "cmoop_net_last_opoint": [C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_net_operating_point": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p],
    # cmoop_eval_population_avg with one more struct pointer after ema and one more output after evaluated
    "cmoop_eval_population_op": [C.c_void_p] * 10 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 8,
}


#: prototypes of the quantisation-aware-training entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
QUANT_PROTOTYPES = {
    "cmoop_quant_default": [C.c_void_p],
    "cmoop_quant_check": [C.c_void_p],
    "cmoop_quant_table": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p],
    "cmoop_quant_size_bytes": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
    "cmoop_quantize_weights": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_quantize_weights_time": [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                    C.c_int32, C.c_void_p],
    "cmoop_net_set_quant": [C.c_void_p, C.c_void_p],
    "cmoop_net_get_quantized": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    # cmoop_eval_population_op with one more struct pointer after op and one more output after opoint
    "cmoop_eval_population_q": [C.c_void_p] * 11 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 9,
}


#: prototypes of the magnitude-pruning entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
PRUNE_PROTOTYPES = {
    "cmoop_prune_default": [C.c_void_p],
    "cmoop_prune_check": [C.c_void_p],
    "cmoop_prune_sparsity_at": [C.c_void_p, C.c_int64, C.c_void_p],
    "cmoop_prune_table": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_prune_size_bytes": [C.c_void_p, C.c_int32, C.c_int32, C.c_double, C.c_int32, C.c_int32, C.c_void_p],
    "cmoop_prune_weights": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_prune_weights_time": [C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_int32,
                                 C.c_void_p],
    "cmoop_net_set_prune": [C.c_void_p, C.c_void_p],
    "cmoop_net_get_pruned": [C.c_void_p, C.c_void_p, C.c_void_p],
    # cmoop_eval_population_q with one more struct pointer after q and one more output after quant
    "cmoop_eval_population_p": [C.c_void_p] * 12 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 10,
}


#: prototypes of the activation-fake-quantisation entry points (include/cmoop.h); structs travel as void* (C.byref), None is NULL
ACTQUANT_PROTOTYPES = {
    "cmoop_actquant_default": [C.c_void_p],
    "cmoop_actquant_check": [C.c_void_p],
    "cmoop_actquant_sites": [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_fake_quant_act": [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_void_p, C.c_float],
    "cmoop_fake_quant_act_time": [C.c_void_p, C.c_int64, C.c_int32, C.c_void_p, C.c_float, C.c_int32, C.c_void_p],
    "cmoop_net_set_actquant": [C.c_void_p, C.c_void_p],
    "cmoop_net_get_act_ranges": [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_net_set_act_ranges": [C.c_void_p, C.c_void_p, C.c_int32],
    "cmoop_net_get_act": [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p],
    # cmoop_eval_population_p with one more struct pointer after pr
    "cmoop_eval_population_aq": [C.c_void_p] * 13 + [C.c_int32, C.c_void_p, C.c_void_p] + [C.c_void_p] * 10,
}


#: prototypes of the PCEN entry points (include/cmoop.h); structs travel as void* (C.byref)
PCEN_PROTOTYPES = {
    "cmoop_pcen_default": [C.c_void_p],
    "cmoop_pcen_check": [C.c_void_p],
    "cmoop_pcen_smoothing": [C.c_double, C.c_int32, C.c_int32, C.c_void_p],
    "cmoop_pcen_apply": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_int32],
    "cmoop_logmel_pcen": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p],
    "cmoop_pcen_stream_plan": [C.c_int64, C.c_void_p, C.c_void_p],
    "cmoop_pcen_stream": [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32],
    "cmoop_logmel_pcen_stream": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p],
    "cmoop_logmel_pcen_stream_time": [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p],
}


#: prototypes of the resampling entry points (include/cmoop.h); pointers travel as void*, None is NULL
RESAMPLE_PROTOTYPES = {
    "cmoop_resample_filter": [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_resample_plan": [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_resample_tile_span": [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p],
    "cmoop_resample": [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p],
    "cmoop_resample_time": [C.c_void_p, C.c_int64, C.c_int64, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_int32,
                            C.c_void_p],
}


#: prototypes of the per-kernel entry points of the BatchNorm / pooling / loss / optimiser kernels (include/cmoop.h)
_V, _I32, _I64, _F64 = C.c_void_p, C.c_int32, C.c_int64, C.c_double
ELEM_PROTOTYPES = {
    "cmoop_bn_train_fwd": [_V] * 10 + [_I64, _I32, _F64, _F64, _I32, _I32],
    "cmoop_bn_eval_fwd": [_V] * 8 + [_I64, _I32, _F64, _I32],
    "cmoop_bn_bwd": [_V] * 9 + [_I64, _I32, _I32, _I32],
    "cmoop_bn_pool_fwd": [_V] * 5 + [_I32] * 5,
    "cmoop_bn_pool_bwd": [_V] * 10 + [_I32] * 6,
    "cmoop_add_relu": [_V, _V, _V, _I64],
    "cmoop_gap_fwd": [_V, _V, _I32, _I32, _I32],
    "cmoop_gap_bwd": [_V, _V, _V, _I32, _I32, _I32],
    "cmoop_softmax_ce": [_V, _V, _V, _I64, _I64, _I32, _I32, _V, _V, _V],
    "cmoop_softmax_probs": [_V, _V, _I32, _I32],
    "cmoop_adam": [_V, _V, _V, _V, _I64, _F64, _F64, _F64, _F64],
    "cmoop_adam_segments": [_V] * 5 + [_I32] + [_V] * 5 + [_F64] * 4,
    "cmoop_confusion": [_V, _V, _I64, _I32, _I32, _V],
    "cmoop_colsum_small": [_V, _V, _I32, _I32],
    "cmoop_dense_dgrad_small": [_V, _V, _V, _I32, _I32, _I32, _V, _F64],
}


#: prototypes of the dense-head entry points that launch dense.hip as a train step does (include/cmoop.h)
_U32 = C.c_uint32
DENSE_PROTOTYPES = {
    "cmoop_dense_fwd_ex": [_V] * 4 + [_I32] * 5 + [_F64, _U32, _I32, _U32, _V],
    "cmoop_dense_bwd_ex": [_V] * 6 + [_I32] * 4 + [_F64, _I32, _I32],
}

#: prototypes of the depthwise-convolution entry points of the separable layers (include/cmoop.h)
DWCONV_PROTOTYPES = {
    "cmoop_dwconv_fwd": [_V] * 3 + [_I32] * 5,
    "cmoop_dwconv_bwd": [_V] * 5 + [_I32] * 6,
    "cmoop_dwconv_wgrad_slices": [_I32] * 5 + [_V],
    "cmoop_dwconv_time": [_I32] + [_V] * 4 + [_I32] * 6 + [_V],
    "cmoop_plan_dwconvs": [_V, _I32, _I32, _I32, _V, _I32, _V],
}

#: prototypes of the integer-inference entry points (include/cmoop.h); pointers travel as void*, None is NULL
_F32 = C.c_float
INT8_PROTOTYPES = {
    "cmoop_conv_fwd_i8": [_V, _V, _F32, _V, _V, _V] + [_I32] * 8,
    "cmoop_dense_fwd_i8": [_V, _V, _F32, _V, _V, _V] + [_I32] * 4,
    "cmoop_conv_fwd_i8_time": [_V, _V, _F32, _V, _V, _V] + [_I32] * 9 + [_V],
    "cmoop_fake_quant_act_codes": [_V, _I64, _I32, _V, _V],
    "cmoop_int8_ops": [_V, _I32, _I32, _I32, _I32, _V, _I32, _V],
    "cmoop_net_set_int8": [_V, _I32],
    "cmoop_net_int8_ops": [_V, _V, _I32, _V],
    "cmoop_fake_quant_act_codes_time": [_V, _I64, _I32, _V, _V, _I32, _V],
    # integer depthwise, the second level
    "cmoop_dwconv_fwd_i8": [_V, _V, _F32, _V] + [_I32] * 6 + [_V, _V, _V],
    "cmoop_dwconv_fwd_i8_time": [_V, _V, _F32, _V] + [_I32] * 6 + [_V, _V, _V, _I32, _V],
    "cmoop_int8_dw_ops": [_V, _I32, _I32, _I32, _I32, _V, _I32, _V],
    "cmoop_net_set_int8_depthwise": [_V, _I32],
    "cmoop_net_int8_dw_ops": [_V, _V, _I32, _V],
    # the requantising epilogue, the third level
    "cmoop_conv_fwd_i8_q": [_V, _V, _F32, _V, _V, _V, _V] + [_I32] * 10 + [_V, _V, _V],
    "cmoop_conv_fwd_i8_q_time": [_V, _V, _F32, _V, _V, _V, _V] + [_I32] * 10 + [_V, _V, _V, _I32, _V],
    "cmoop_dense_fwd_i8_q": [_V, _V, _F32, _V, _V, _V, _V] + [_I32] * 6 + [_V, _V, _V],
    "cmoop_dense_fwd_i8_q_time": [_V, _V, _F32, _V, _V, _V, _V] + [_I32] * 6 + [_V, _V, _V, _I32, _V],
    "cmoop_dense_fwd_i8_time": [_V, _V, _F32, _V, _V, _V] + [_I32] * 5 + [_V],
    "cmoop_scale_shift_time": [_V, _V, _V, _V, _I64, _I32, _I32, _I32, _V],
    "cmoop_int8_fused_ops": [_V, _I32, _I32, _I32, _I32, _V, _I32, _V],
    "cmoop_net_set_int8_fused": [_V, _I32],
    "cmoop_net_int8_fused_ops": [_V, _V, _I32, _V],
}

#: prototype of the train-step launch counters (include/cmoop.h)
STEP_PROTOTYPES = {
    "cmoop_step_launch_counts": [_V],
}

#: CMOOP_GEMM_* (include/cmoop.h)
GEMM_DEFAULT, GEMM_FP32, GEMM_BF16X3, GEMM_BF16 = 0, 1, 2, 3


def build(verbose: bool = False) -> str:
    """Compile libcmoop_hip.so for gfx950 in-tree (make; hipcc cross-compiles on CPU-only hosts)."""
    jobs = str(min(8, os.cpu_count() or 1))
    r = subprocess.run(["make", "-C", CSRC, "-j", jobs], capture_output=True, text=True)
    if r.returncode != 0:
        raise CmoopError("building libcmoop_hip.so failed:\n" + r.stdout[-4000:] + r.stderr[-4000:])
    if verbose:
        print(r.stdout[-2000:])
    return LIB_PATH


def declared_symbols():
    """Function names declared in include/cmoop.h."""
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"\b(cmoop_[a-z0-9_]+)\s*\(", txt)))


def lib():
    """The loaded library; raises CmoopError (never falls back) when it is absent."""
    global _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise CmoopError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(or `make -C cmoop_audio_processing_amd/csrc`). There is no CPU fallback for this path.")
        try:
            L = C.CDLL(LIB_PATH)
        except OSError as e:
            raise CmoopError(f"cannot load {LIB_PATH}: {e}") from e
        L.cmoop_last_error.restype = C.c_char_p
        L.cmoop_abi_version.restype = C.c_int
        for name in declared_symbols():
            fn = getattr(L, name)          # AttributeError if the header and the library disagree
            if name not in ("cmoop_last_error", "cmoop_config_default"):
                fn.restype = C.c_int
        L.cmoop_config_default.restype = None
        for table in (STREAM_PROTOTYPES, AUGMENT_PROTOTYPES, PCEN_PROTOTYPES, ELEM_PROTOTYPES, LOSS_PROTOTYPES, DENSE_PROTOTYPES,
                      DWCONV_PROTOTYPES, DISTILL_PROTOTYPES, OPTIM_PROTOTYPES, EMA_PROTOTYPES, OPOINT_PROTOTYPES, QUANT_PROTOTYPES,
                      PRUNE_PROTOTYPES, ACTQUANT_PROTOTYPES, RESAMPLE_PROTOTYPES, INT8_PROTOTYPES, STEP_PROTOTYPES):
            for name, argtypes in table.items():
                getattr(L, name).argtypes = argtypes
        _lib = L
        return L


def check(rc: int) -> None:
    if rc != 0:
        raise CmoopError(lib().cmoop_last_error().decode("utf-8", "replace"))


def step_launch_counts() -> dict:
    """Process-wide totals since load of the fit loop's train steps (cmoop_step_launch_counts): launched eagerly, replayed from
    a captured graph (CMOOP_GRAPH=1), captures made, captures dropped.  Host only."""
    out = (C.c_int64 * 4)()
    check(lib().cmoop_step_launch_counts(out))
    return {"eager": int(out[0]), "replays": int(out[1]), "captures": int(out[2]), "drops": int(out[3])}


def default_config() -> Config:
    c = Config()
    lib().cmoop_config_default(C.byref(c))
    return c


def last_kernels():
    """Launch-path variant names of the GEMM kernels the calling thread's last kernel-level call launched."""
    buf = C.create_string_buffer(1024)
    check(lib().cmoop_last_kernels(buf, C.c_int32(1024)))
    return [k for k in buf.value.decode().split(";") if k]


def plan_convs(gene, variant, T, F):
    """[(H, W, Cin, Cout, KS, stride, feeds_bn)] of the MFMA conv layers of a candidate, forward order (host-only)."""
    g, n, cap = (C.c_int32 * 6)(*gene), C.c_int32(), 16
    rows = (C.c_int32 * (7 * cap))()
    check(lib().cmoop_plan_convs(g, C.c_int32(variant), C.c_int32(T), C.c_int32(F), rows, C.c_int32(cap), C.byref(n)))
    assert n.value <= cap
    return [tuple(rows[7 * i:7 * i + 7]) for i in range(n.value)]


def plan_dwconvs(gene, variant, T, F):
    """[(H, W, C, KS)] of the depthwise layers of a candidate (variants A_ds / B_ds), forward order (host-only); their
    pointwise halves are the KS = 1, stride = 1 rows of plan_convs."""
    g, n, cap = (C.c_int32 * 6)(*gene), C.c_int32(), 16
    rows = (C.c_int32 * (4 * cap))()
    check(lib().cmoop_plan_dwconvs(g, C.c_int32(variant), C.c_int32(T), C.c_int32(F), rows, C.c_int32(cap), C.byref(n)))
    assert n.value <= cap
    return [tuple(rows[4 * i:4 * i + 4]) for i in range(n.value)]


def dwconv_wgrad_slices(B, H, W, Cn, KS):
    """Row-run slices of the depthwise weight gradient at this shape (host-only)."""
    out = C.c_int32()
    check(lib().cmoop_dwconv_wgrad_slices(B, H, W, Cn, KS, C.byref(out)))
    return int(out.value)


def net_launch_plan(gene, config, T, F, B, train):
    """Launch-path variants of the MFMA conv launches of one train step (train) or inference pass of a net at batch B,
    in launch order, under the net's shared split-K workspace (host-only); config: a Config struct."""
    g, buf = (C.c_int32 * 6)(*gene), C.create_string_buffer(8192)
    check(lib().cmoop_net_launch_plan(g, C.byref(config), C.c_int32(T), C.c_int32(F), C.c_int32(B), C.c_int32(int(train)), buf,
                                      C.c_int32(8192)))
    return [k for k in buf.value.decode().split(";") if k]


def profile_entries():
    """[(kernel name, launches, total ms, total flops)] of the HIP-event-sampled MFMA GEMM launches."""
    L, cnt, out = lib(), C.c_int32(), []
    check(L.cmoop_profile_count(C.byref(cnt)))
    for i in range(cnt.value):
        name, n, ms, fl = C.create_string_buffer(160), C.c_int64(), C.c_double(), C.c_double()
        check(L.cmoop_profile_entry(i, name, 160, C.byref(n), C.byref(ms), C.byref(fl)))
        out.append((name.value.decode(), int(n.value), float(ms.value), float(fl.value)))
    return out


def profile_variants():
    """Launch-path variants (instantiation + "+sk" / "+stats" / "+tab" / "+slabs") of the sampled launches."""
    L, cnt, out = lib(), C.c_int32(), []
    check(L.cmoop_profile_variant_count(C.byref(cnt)))
    for i in range(cnt.value):
        name = C.create_string_buffer(200)
        check(L.cmoop_profile_variant(i, name, 200))
        out.append(name.value.decode())
    return out


def ptr(t):
    """Raw device/host pointer of a torch tensor or numpy array (must be contiguous)."""
    if t is None:
        return None
    if hasattr(t, "data_ptr"):
        assert t.is_contiguous(), "tensor must be contiguous"
        return C.c_void_p(t.data_ptr())
    assert t.flags["C_CONTIGUOUS"], "array must be C-contiguous"
    return C.c_void_p(t.ctypes.data)
