"""The proposal generator: mmdet's anchor generator and RPN head, restated.

    AnchorGenerator   mmdet/core/anchor/anchor_generator.py:142-270 (gen_single_level_base_anchors with centre offset 0,
                      scale-major; single_level_grid_anchors).  Only the base anchors [L,A,4] reach the device route:
                      csrc/rpn.hip computes an anchor from (level, index); grid_anchors serves the tensor-op route and tests.
    RPNHead           mmdet/models/dense_heads/rpn_head.py:16-47, 82-236 + rpn_test_mixin.py simple_test_rpn + AnchorHead.
                      get_bboxes: the 3x3 convolution, ReLU, the two 1x1 convolutions (through torch by default; with
                      compute_dtype=torch.bfloat16, on device inputs under no-grad, two launches of as_conv2d_fwd per
                      level), then inference.rpn_proposals.  Parameter names are the reference's (rpn_conv, rpn_cls, rpn_reg), so its
                      checkpoints load.
    RPNHead.loss /    AnchorHead.loss (mmdet/models/dense_heads/anchor_head.py:425-493) as RPNHead.loss renames it
    forward_train     (rpn_head.py:49-80) and BaseDenseHead.forward_train (base_dense_head.py:22-59): the anchor targets,
                      MaxIoUAssigner, RandomSampler and the two losses are in rpn_train (device tensors: csrc/rpn_train.hip).
                      Built: CrossEntropyLoss(use_sigmoid=True), L1Loss, reg_decoded_bbox=False; anything else raises in loss.
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import inference, ops, rpn_train
from .neck import PackedConvCache, nhwc_bf16, warn_once
from .registry import HEADS


def _pair(v):
    return (int(v), int(v)) if not isinstance(v, (tuple, list)) else (int(v[0]), int(v[1]))


def grid_anchors(base_anchors, featmap_size, stride):
    """base_anchors [A,4], (H, W), (sx, sy) -> [H * W * A, 4]: row (y * W + x) * A + a = base[a] + (x sx, y sy, x sx, y sy)"""
    H, W = int(featmap_size[0]), int(featmap_size[1])
    sx, sy = _pair(stride)
    shift_x = torch.arange(0, W, device=base_anchors.device) * sx
    shift_y = torch.arange(0, H, device=base_anchors.device) * sy
    xx, yy = shift_x.repeat(H), shift_y.view(-1, 1).repeat(1, W).view(-1)
    shifts = torch.stack([xx, yy, xx, yy], dim=-1).type_as(base_anchors)
    return (base_anchors[None, :, :] + shifts[:, None, :]).view(-1, 4)


class AnchorGenerator:
    def __init__(self, scales, ratios, strides, base_sizes=None, type=None):
        self.strides = [_pair(s) for s in strides]
        self.base_sizes = [min(s) for s in self.strides] if base_sizes is None else list(base_sizes)
        if len(self.base_sizes) != len(self.strides):
            raise ValueError(f"AnchorGenerator: {len(self.strides)} strides but {len(self.base_sizes)} base sizes")
        self.scales, self.ratios = torch.Tensor(scales), torch.Tensor(ratios)
        self.base_anchors = [self._base(b) for b in self.base_sizes]

    def _base(self, base_size):
        h_ratios = torch.sqrt(self.ratios)
        w_ratios = 1 / h_ratios
        ws = (base_size * w_ratios[:, None] * self.scales[None, :]).view(-1)
        hs = (base_size * h_ratios[:, None] * self.scales[None, :]).view(-1)
        return torch.stack([0 - 0.5 * ws, 0 - 0.5 * hs, 0 + 0.5 * ws, 0 + 0.5 * hs], dim=-1)

    @property
    def num_levels(self):
        return len(self.strides)

    @property
    def num_base_anchors(self):
        return [b.size(0) for b in self.base_anchors]

    def grid_anchors(self, featmap_sizes, device="cpu"):
        """(tests and the tensor-op route only) -> per level [H * W * A, 4]"""
        if len(featmap_sizes) != self.num_levels:
            raise ValueError(f"AnchorGenerator: {len(featmap_sizes)} feature maps for {self.num_levels} levels")
        return [grid_anchors(b.to(device), fs, s) for b, fs, s in zip(self.base_anchors, featmap_sizes, self.strides)]


@HEADS.register_module()
class RPNHead(nn.Module):
    def __init__(self, in_channels, feat_channels=256, anchor_generator=None, bbox_coder=None, loss_cls=None, loss_bbox=None,
                 train_cfg=None, test_cfg=None, compute_dtype=None, **unused):
        super().__init__()
        if compute_dtype not in (None, torch.bfloat16):
            raise ValueError(f"RPNHead: compute_dtype={compute_dtype!r} (None: the convolutions through torch; torch.bfloat16: "
                             "as_conv2d_fwd on device inputs under no-grad)")
        self.compute_dtype = compute_dtype
        ag = dict(anchor_generator or dict(scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]))
        if ag.pop("type", "AnchorGenerator") != "AnchorGenerator":
            raise ValueError("RPNHead: only AnchorGenerator anchors")
        self.anchor_generator = AnchorGenerator(**ag)
        if len(set(self.anchor_generator.num_base_anchors)) != 1:
            raise ValueError("RPNHead: every level needs the same number of base anchors")
        self.num_anchors = self.anchor_generator.num_base_anchors[0]
        bc = dict(bbox_coder or {})
        if bc.get("type", "DeltaXYWHBBoxCoder") != "DeltaXYWHBBoxCoder":
            raise ValueError("RPNHead: only DeltaXYWHBBoxCoder")
        self.target_means = tuple(float(v) for v in bc.get("target_means", (0., 0., 0., 0.)))
        self.target_stds = tuple(float(v) for v in bc.get("target_stds", (1., 1., 1., 1.)))
        if loss_cls is not None and not loss_cls.get("use_sigmoid", False):
            raise ValueError("RPNHead: the softmax (two-channel) objectness of loss_cls.use_sigmoid=False is not built")
        self.in_channels, self.feat_channels = in_channels, feat_channels
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.loss_cls_cfg, self.loss_bbox_cfg = dict(loss_cls or {}), dict(loss_bbox or {})
        self.reg_decoded_bbox = bool(unused.get("reg_decoded_bbox", False))
        self.rpn_conv = nn.Conv2d(in_channels, feat_channels, 3, padding=1)
        self.rpn_cls = nn.Conv2d(feat_channels, self.num_anchors, 1)
        self.rpn_reg = nn.Conv2d(feat_channels, self.num_anchors * 4, 1)
        self.register_buffer("base_anchors", torch.stack(self.anchor_generator.base_anchors), persistent=False)
        self._packed = PackedConvCache()
        self.init_weights()

    def init_weights(self):
        for m in (self.rpn_conv, self.rpn_cls, self.rpn_reg):
            nn.init.normal_(m.weight, 0, 0.01)
            nn.init.constant_(m.bias, 0)

    def forward_single(self, x):
        if x.dtype != self.rpn_conv.weight.dtype:                # (the neck's bf16 maps on the tensor-op route)
            x = x.to(self.rpn_conv.weight.dtype)
        x = F.relu(self.rpn_conv(x), inplace=True)
        return self.rpn_cls(x), self.rpn_reg(x)

    def _forward_single_hip(self, x):
        """forward_single as two launches of as_conv2d_fwd (csrc/conv.hip): the 3x3 trunk with ReLU in bf16, then rpn_cls |
        rpn_reg as ONE 1x1 convolution (A + 4A rows padded to 16) in fp32.  The two slices of its packed output leave as the
        dense [B,A,H,W] / [B,4A,H,W] tensors inference.rpn_proposals takes (15 of 16 channels: small copies)."""
        A = self.num_anchors
        w, b = self._packed.get("conv", [self.rpn_conv.weight], [self.rpn_conv.bias])
        t = ops.conv2d_nhwc(nhwc_bf16(x), w, b, ksize=3, act="relu")
        w, b = self._packed.get("heads", [self.rpn_cls.weight, self.rpn_reg.weight], [self.rpn_cls.bias, self.rpn_reg.bias])
        y = ops.conv2d_nhwc(t, w, b, ksize=1, out_dtype=torch.float32).permute(0, 3, 1, 2)
        return y[:, :A].contiguous(), y[:, A:5 * A].contiguous()

    def forward(self, feats):
        """feats: per level [B, in_channels, H_l, W_l] -> (cls_scores, bbox_preds), two per-level lists"""
        hip = self.compute_dtype == torch.bfloat16 and not torch.is_grad_enabled() and all(x.is_cuda for x in feats)
        if hip and (self.in_channels % 32 or self.feat_channels % 32):
            warn_once(("RPNHead", self.in_channels, self.feat_channels),
                      f"RPNHead: channels {self.in_channels} -> {self.feat_channels} miss as_conv2d_fwd's contract (multiples "
                      "of 32): taking the tensor-op route")
            hip = False
        outs = [self._forward_single_hip(x) if hip else self.forward_single(x) for x in feats]
        return [o[0] for o in outs], [o[1] for o in outs]

    def get_bboxes(self, cls_scores, bbox_preds, img_metas, cfg=None):
        """-> per image [m,5] proposals (x1, y1, x2, y2, score); cfg: nms_pre, max_per_img, nms.iou_threshold, min_bbox_size"""
        cfg = self.test_cfg if cfg is None else cfg
        if cfg is None:
            raise ValueError("RPNHead.get_bboxes: no cfg and no test_cfg")
        if len(cls_scores) != self.anchor_generator.num_levels:
            raise ValueError(f"RPNHead: {len(cls_scores)} levels for {self.anchor_generator.num_levels} strides")
        nms = cfg.get("nms") or dict(iou_threshold=cfg["nms_thr"])
        max_per_img = cfg["max_per_img"] if "max_per_img" in cfg else cfg["max_num"]
        return inference.rpn_proposals([c.detach() for c in cls_scores], [r.detach() for r in bbox_preds], self.base_anchors,
                                       self.anchor_generator.strides, [m["img_shape"] for m in img_metas], cfg["nms_pre"],
                                       max_per_img, nms["iou_threshold"], cfg.get("min_bbox_size", 0), self.target_means,
                                       self.target_stds)

    def simple_test_rpn(self, feats, img_metas):
        """-> the proposal_list AttnShiftRoIHead.simple_test takes"""
        cls_scores, bbox_preds = self.forward(feats)
        return self.get_bboxes(cls_scores, bbox_preds, img_metas)

    def _loss_settings(self):
        """-> (assigner, sampler, allowed_border, pos_weight, loss_cls weight, loss_bbox weight); raises on what is not built"""
        cfg = self.train_cfg
        if cfg is None:
            raise ValueError("RPNHead.loss: no train_cfg (assigner, sampler, allowed_border, pos_weight)")
        lc, lb = self.loss_cls_cfg, self.loss_bbox_cfg
        if lc.get("type", "CrossEntropyLoss") != "CrossEntropyLoss" or not lc.get("use_sigmoid", bool(not lc)) or \
                lc.get("class_weight") is not None or lc.get("reduction", "mean") != "mean":
            raise ValueError("RPNHead.loss: only CrossEntropyLoss(use_sigmoid=True) with the mean reduction is built")
        if lb.get("type", "L1Loss") != "L1Loss" or lb.get("reduction", "mean") != "mean":
            raise ValueError("RPNHead.loss: only L1Loss with the mean reduction is built")
        if self.reg_decoded_bbox:
            raise ValueError("RPNHead.loss: reg_decoded_bbox=True is not built")
        sampler = dict(cfg.get("sampler") or {})
        if sampler.get("type", "RandomSampler") != "RandomSampler" or sampler.get("add_gt_as_proposals", False):
            raise ValueError("RPNHead.loss: only RandomSampler without added GT boxes is built")
        return (dict(cfg.get("assigner") or {}), sampler, int(cfg.get("allowed_border", 0)), cfg.get("pos_weight", -1),
                float(lc.get("loss_weight", 1.0)), float(lb.get("loss_weight", 1.0)))

    def loss(self, cls_scores, bbox_preds, gt_bboxes, img_metas, gt_bboxes_ignore=None, generator=None):
        """-> dict(loss_rpn_cls=[L tensors], loss_rpn_bbox=[L tensors]), or None when an image has no anchor inside
        (anchor_head.py:353-354).  On the device route the one host sync is the readback of the [B,2] counts."""
        assigner, sampler, border, pos_weight, w_cls, w_bbox = self._loss_settings()
        if len(cls_scores) != self.anchor_generator.num_levels:
            raise ValueError(f"RPNHead: {len(cls_scores)} levels for {self.anchor_generator.num_levels} strides")
        sizes = [tuple(int(v) for v in c.shape[-2:]) for c in cls_scores]
        strides = self.anchor_generator.strides
        base = self.base_anchors.to(cls_scores[0].device)
        rpn_train._check_assigner(assigner, gt_bboxes_ignore)
        if not all(rpn_train.any_inside(self.anchor_generator.base_anchors, sizes, strides, m, border) for m in img_metas):
            return None
        asg = rpn_train.rpn_assign(base, sizes, strides, gt_bboxes, img_metas, assigner, border, gt_bboxes_ignore)
        smp = rpn_train.rpn_sample(asg, sampler.get("num", 256), sampler.get("pos_fraction", 0.5), sampler.get("neg_pos_ub", -1),
                                   generator)
        _, pos_delta = rpn_train.rpn_targets(asg, smp, self.target_means, self.target_stds)
        loss_cls, loss_bbox = rpn_train.rpn_loss(cls_scores, bbox_preds, asg, smp, pos_delta, pos_weight, w_cls, w_bbox)
        return dict(loss_rpn_cls=list(loss_cls.unbind(0)), loss_rpn_bbox=list(loss_bbox.unbind(0)))

    def forward_train(self, x, img_metas, gt_bboxes, gt_labels=None, gt_bboxes_ignore=None, proposal_cfg=None, generator=None):
        """One forward, the losses and, with a proposal_cfg, the proposals of the detached outputs -> losses, or
        (losses, proposal_list).  gt_labels are not used (the RPN is class agnostic)."""
        cls_scores, bbox_preds = self.forward(x)
        losses = self.loss(cls_scores, bbox_preds, gt_bboxes, img_metas, gt_bboxes_ignore=gt_bboxes_ignore, generator=generator)
        if proposal_cfg is None:
            return losses
        return losses, self.get_bboxes(cls_scores, bbox_preds, img_metas, cfg=proposal_cfg)
