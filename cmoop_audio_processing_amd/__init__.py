"""MI355X-native population-fitness evaluator for the SA-NSGA-II audio-NAS loop.

Drop-in for ONE path of sumansamui/CMOOP_Audio_Processing:
``compute_objectives_and_constraints -> evaluate_individual`` (reference
nsga_penalty.py:368-442, sa_nsga_penalty.py:205-253), implemented as
hand-written HIP kernels for gfx950 behind a C ABI (include/cmoop.h).
Importing this package never touches the GPU; the HIP library is loaded on
first use and there is no CPU fallback.
"""
from . import genes  # noqa: F401
from .evaluator import (AudioNASProblem, EvalConfig, PopulationEvaluator, calculate_fpr,  # noqa: F401
                        compute_model_size_mb, compute_objectives_and_constraints, evaluate_individual, install,
                        queued_map, sharded_map)
from .frontend import FrontendConfig, PcenConfig, log_mel_stream  # noqa: F401
from .resample import resample_poly  # noqa: F401
from .augment import AugmentConfig  # noqa: F401
from .loss import LossConfig  # noqa: F401
from .distill import DistillConfig  # noqa: F401
from .optim import OptimConfig  # noqa: F401
from .ema import EmaConfig  # noqa: F401
from .opoint import OperatingPointConfig  # noqa: F401
from .quant import QuantConfig  # noqa: F401
from .prune import PruneConfig  # noqa: F401
from .quant import ActQuantConfig  # noqa: F401
from .deploy import StreamScorer, TrainedModel, detect_events, smooth_posteriors  # noqa: F401

__all__ = ["genes", "AugmentConfig", "LossConfig", "DistillConfig", "OptimConfig", "EmaConfig", "OperatingPointConfig", "QuantConfig", "PruneConfig", "ActQuantConfig", "EvalConfig", "PopulationEvaluator", "AudioNASProblem", "install", "evaluate_individual",
           "compute_objectives_and_constraints", "compute_model_size_mb", "calculate_fpr", "sharded_map", "queued_map", "FrontendConfig", "PcenConfig",
           "log_mel_stream", "resample_poly", "TrainedModel", "StreamScorer", "smooth_posteriors", "detect_events"]
