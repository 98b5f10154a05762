"""The detector that ties backbone, neck, RPN and RoI head together: the reference's point-supervised two-stage detector,
restated (mmdet/models/detectors/two_stage_point_sup.py:18-127, 288-300 and two_stage_point_align.py:18-165, with
BaseDetector's forward / forward_test / train_step of mmdet/models/detectors/base.py).

    TwoStageDetectorPointSupAlign     extract_feat -> seed_pseudo_gt (the attention shift's pseudo boxes, labels, masks) ->
                                      rpn_head.forward_train on the pseudo boxes (losses + proposals by
                                      train_cfg.rpn_proposal) -> roi_head.forward_train; simple_test: extract_feat ->
                                      simple_test_rpn -> roi_head.simple_test.
    FasterRCNNPointSupAlign           the name the shipped config builds (configs/mae/attnshift_voc12aug.py).

aug_test, visualize=True and the teacher-student variants are not built (NotImplementedError).
"""
import torch
import torch.nn as nn

from . import dist
from .registry import DETECTORS, build_backbone, build_head, build_neck


def _get(cfg, key, default=None):
    if cfg is None:
        return default
    return cfg.get(key, default) if hasattr(cfg, "get") else getattr(cfg, key, default)


@DETECTORS.register_module()
class TwoStageDetectorPointSupAlign(nn.Module):
    def __init__(self, backbone, neck=None, rpn_head=None, roi_head=None, roi_skip_fpn=False, train_cfg=None, test_cfg=None,
                 pretrained=None, pos_mask_thr=0.35, neg_mask_thr=0.7, num_mask_point_gt=10, corr_size=21, obj_tau=0.9,
                 visualize=False, compute_dtype=None):
        super().__init__()
        if visualize:
            raise NotImplementedError("visualize=True (the attribute dump for the reference's plotting scripts) is not built")
        own = {} if compute_dtype is None else dict(compute_dtype=compute_dtype)
        self.backbone = build_backbone(backbone)
        if neck is not None:
            self.neck = build_neck({**own, **neck})
        if rpn_head is not None:
            self.rpn_head = build_head({**own, **rpn_head, "train_cfg": _get(train_cfg, "rpn"), "test_cfg": _get(test_cfg, "rpn")})
        if roi_head is not None:
            self.roi_head = build_head({**roi_head, "train_cfg": _get(train_cfg, "rcnn"), "test_cfg": _get(test_cfg, "rcnn")})
        self.roi_skip_fpn = roi_skip_fpn
        self.train_cfg, self.test_cfg = train_cfg, test_cfg
        self.pos_mask_thr, self.neg_mask_thr, self.num_mask_point_gt = pos_mask_thr, neg_mask_thr, num_mask_point_gt
        self.corr_size, self.obj_tau = corr_size, obj_tau
        self.visualize = False
        self.init_weights(pretrained=pretrained)

    @property
    def with_neck(self):
        return getattr(self, "neck", None) is not None

    @property
    def with_rpn(self):
        return getattr(self, "rpn_head", None) is not None

    @property
    def with_roi_head(self):
        return getattr(self, "roi_head", None) is not None

    @property
    def with_bbox(self):
        return self.with_roi_head and self.roi_head.with_bbox

    @property
    def with_mask(self):
        return self.with_roi_head and self.roi_head.with_mask

    def init_weights(self, pretrained=None):
        self.backbone.init_weights(pretrained=pretrained)
        if self.with_neck:
            self.neck.init_weights()
        if self.with_rpn:
            self.rpn_head.init_weights()
        if self.with_roi_head and hasattr(self.roi_head, "init_weights"):
            self.roi_head.init_weights(pretrained)

    def extract_feat(self, img):
        """backbone (+ neck on its `feature` maps) -> the backbone's dict"""
        feats = self.backbone(img)
        if self.with_neck:
            feats.update(dict(feature=self.neck(feats["feature"])))
        return feats

    def get_roi_feat(self, x, vit_feat):
        """what the RoI extractors read: the pyramid, or with roi_skip_fpn the last block's patch tokens as one stride-16 map"""
        if not self.roi_skip_fpn:
            return x
        B, _, H, W = x[2].shape
        return [vit_feat[:, 1:, :].transpose(1, 2).reshape(B, -1, H, W).contiguous()]

    def forward_train(self, img, img_metas, gt_labels, gt_centers, gt_bboxes_ignore=None, gt_masks=None, proposals=None, **kwargs):
        """two_stage_point_align.py:55-165 -> the dict of the MIL, RPN and RoI losses"""
        feats = self.extract_feat(img)
        x, vit_feat = feats["feature"], feats["last_feat"]
        outputs_class, outputs_coord, attns = feats["outputs_class"], feats["outputs_coord"], feats["attns"]
        patch_h, patch_w = x[2].size(-2), x[2].size(-1)
        imgs_whwh = torch.stack([x[0].new_tensor([m["img_shape"][1], m["img_shape"][0]]) for m in img_metas])[:, None, :]
        generator = kwargs.pop("generator", None)
        roi_feat = self.get_roi_feat(x, vit_feat)
        losses = dict()
        seed = self.roi_head.seed_pseudo_gt(
            x, img_metas, None, None, None, gt_bboxes_ignore, gt_masks,
            vit_feat=vit_feat.clone().detach().permute(0, 2, 1)[..., 1:].unflatten(-1, (patch_h, patch_w)), img=img,
            point_cls=outputs_class, point_reg=outputs_coord, imgs_whwh=imgs_whwh, attns=attns, gt_points=gt_centers,
            gt_points_labels=gt_labels, roi_feature_map=roi_feat, return_mask=True,
            pos_mask_thr=self.pos_mask_thr, neg_mask_thr=self.neg_mask_thr, num_mask_point_gt=self.num_mask_point_gt,
            corr_size=self.corr_size, obj_tau=self.obj_tau, **kwargs)
        pseudo_gt_labels, pseudo_gt_bboxes = seed["pseudo_gt_labels"], seed["pseudo_gt_bboxes"]
        losses.update(seed["mil_losses"])
        if self.with_rpn:
            proposal_cfg = _get(self.train_cfg, "rpn_proposal", _get(self.test_cfg, "rpn"))
            rpn_losses, proposal_list = self.rpn_head.forward_train(x, img_metas, pseudo_gt_bboxes, gt_labels=None,
                                                                    gt_bboxes_ignore=gt_bboxes_ignore, proposal_cfg=proposal_cfg,
                                                                    generator=generator)
            losses.update(rpn_losses or {})
        else:
            proposal_list = proposals
        losses.update(self.roi_head.forward_train(
            roi_feat, img_metas, proposal_list, pseudo_gt_bboxes, pseudo_gt_labels, gt_bboxes_ignore, seed["pseudo_gt_masks"],
            vit_feat=vit_feat, img=img, point_cls=outputs_class, point_reg=outputs_coord, imgs_whwh=imgs_whwh, attns=attns,
            gt_points=gt_centers, gt_points_labels=gt_labels, feats_point_tokens=feats.get("point_tokens"),
            mask_point_coords=seed["mask_points_coords"], mask_point_labels=seed["mask_points_labels"],
            semantic_centers=seed["semantic_centers"], semantic_centers_split=seed["semantic_centers_split"],
            sc_corres_gts=seed.get("corres_gts"), generator=generator))
        return losses

    def simple_test(self, img, img_metas, proposals=None, rescale=False):
        """-> per image (bbox_results, segm_results), num_classes lists each (bbox_results alone without a mask head)"""
        if not self.with_bbox:
            raise RuntimeError("simple_test needs a RoI head with a box head")
        feats = self.extract_feat(img)
        x, vit_feat = feats["feature"], feats["last_feat"]
        proposal_list = self.rpn_head.simple_test_rpn(x, img_metas) if proposals is None else proposals
        return self.roi_head.simple_test(self.get_roi_feat(x, vit_feat), proposal_list, img_metas, rescale=rescale)

    def aug_test(self, imgs, img_metas, rescale=False):
        raise NotImplementedError("aug_test (test-time augmentation) is not built")

    def forward_test(self, imgs, img_metas, **kwargs):
        """base.py:128-168 for single-augmentation lists: imgs = [tensor], img_metas = [[dict per image]]"""
        for var, name in ((imgs, "imgs"), (img_metas, "img_metas")):
            if not isinstance(var, list):
                raise TypeError(f"{name} must be a list, but got {type(var)}")
        if len(imgs) != len(img_metas):
            raise ValueError(f"num of augmentations ({len(imgs)}) != num of image meta ({len(img_metas)})")
        if len(imgs) != 1:
            return self.aug_test(imgs, img_metas, **kwargs)
        if "proposals" in kwargs:
            kwargs["proposals"] = kwargs["proposals"][0]
        return self.simple_test(imgs[0], img_metas[0], **kwargs)

    def forward(self, img, img_metas, return_loss=True, **kwargs):
        if return_loss:
            return self.forward_train(img, img_metas, **kwargs)
        return self.forward_test(img, img_metas, **kwargs)

    def train_step(self, data, optimizer=None):
        """base.py:220-254: the losses of one batch -> dict(loss, log_vars, num_samples); backward and the optimizer step are
        the caller's (the runner's hooks)."""
        losses = self(**data)
        loss, log_vars = dist.parse_losses(losses)
        return dict(loss=loss, log_vars=log_vars, num_samples=len(data["img_metas"]))


@DETECTORS.register_module()
class FasterRCNNPointSupAlign(TwoStageDetectorPointSupAlign):
    """mmdet/models/detectors/faster_rcnn_point_sup.py: the constructor arguments handed on unchanged"""
