"""spair_pytorch_amd -- MI355X-native SPAIR training step behind the reference's Python surface.

``from spair_pytorch_amd import config as cfg``; ``from spair_pytorch_amd.models import SPAIR``.
The compute lives in libspair_hip.so (hand-written gfx950 kernels, C ABI in include/spair_hip.h);
there is no PyTorch/CPU fallback.
"""
from . import config  # noqa: F401

__all__ = ["config", "SPAIR", "ParseResult", "ComposeResult", "GenerateResult", "EvalResult", "parse_boxes",
           "segmentation", "SegmentationResult", "DetectionAP", "DetectionBatch", "DetectionResult", "detection_ap"]


def __getattr__(name):
    # the model surface, resolved on first use (importing the package alone stays as light as it was: config only)
    if name in ("SPAIR", "ParseResult", "ComposeResult", "GenerateResult", "EvalResult", "parse_boxes"):
        from . import models
        return getattr(models, name)
    if name in ("segmentation", "SegmentationResult"):
        from . import metric
        return getattr(metric, name)
    if name in ("DetectionAP", "DetectionBatch", "DetectionResult", "detection_ap"):
        from . import detection
        return getattr(detection, name)
    raise AttributeError("module %r has no attribute %r" % (__name__, name))
