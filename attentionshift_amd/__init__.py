"""attentionshift_amd -- MI355X (gfx950) native hot path of AttentionShift.

Exposes the reference's plugin surface (mmdet-style registries, same class names / kwargs):
    BACKBONES: VisionTransformerDet, SwinTransformer (the detection-style Swin backbone of BASELINE config 5)
    HEADS:     AttnShiftRoIHead (also registered as StandardRoIHeadMaskPointSampleDeformAttnReppoints),
               RPNHead (test-time proposals; not pushed into mmdet's registry, whose RPNHead carries the losses)
    NECKS:     FPN
    DETECTORS: TwoStageDetectorPointSupAlign, FasterRCNNPointSupAlign
Compute goes through libattnshift_hip.so (include/attnshift.h); there is no CPU fallback.
"""
from .registry import (BACKBONES, DETECTORS, HEADS, NECKS, Registry, build_backbone, build_detector, build_from_cfg,  # noqa: F401
                       build_head, build_neck, register_into_mmdet)
from .config import Config, ConfigDict  # noqa: F401
from .backbone import VisionTransformerDet  # noqa: F401
from .swin_det import SwinTransformerDet  # noqa: F401  (BACKBONES: SwinTransformer)
from .roi_head import AttnShiftRoIHead  # noqa: F401
from .checkpoint import load_checkpoint, save_checkpoint  # noqa: F401
from .mil_head import MAEBoxHeadMIL  # noqa: F401  (registers into HEADS)
from .mae_heads import MAEBoxHeadRec, MAEMaskHeadPointSup  # noqa: F401
from .neck import FPN  # noqa: F401  (NECKS)
from .rpn import AnchorGenerator, RPNHead  # noqa: F401  (HEADS: RPNHead, test time only)
from .detector import FasterRCNNPointSupAlign, TwoStageDetectorPointSupAlign  # noqa: F401  (DETECTORS)
from .annotations import PointAnnotations, parse_ann_info  # noqa: F401

__version__ = "0.1.0"
