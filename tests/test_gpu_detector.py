"""The detector (attentionshift_amd/detector.py) on the GPU: a small FasterRCNNPointSupAlign built by build_detector from a
model dict of the reference's shape -- the `h4` backbone of the parity fixtures (helpers.backbone_cfg), the FPN, the
shipped RPN head's dict (test_rpn.SHIPPED_RPN_HEAD) at the neck's width and the RoI head of test_gpu_path.py's training
test -- on two images of different img_shape.

simple_test / forward(return_loss=False) against the stages called by hand; forward_train / train_step on synthetic.py
inputs: every loss of the three stages, finite, with gradients down to the neck, the RPN trunk and the backbone.  With
random weights the roll-out is near uniform, so (as bench.py does) the roll-out rows of the objects are replaced by the
seeded CAMs of synthetic.shift_inputs and the point-token matching is given.
"""
import numpy as np
import pytest
import torch

import attentionshift_amd as A
from attentionshift_amd import synthetic
from helpers import backbone_cfg
from test_rpn import SHIPPED_RPN_HEAD

pytestmark = pytest.mark.gpu

G = 3                                                                    # objects per image


def model_dict(g):
    cfg = backbone_cfg(g)
    D, ncls, Lc = cfg["embed_dim"], cfg["num_classes"], cfg["cam_layer"]
    dec = dict(in_channels=D, embed_dim=64, depth=1, num_heads=2, num_classes=ncls)
    roi = dict(type="SingleRoIExtractor", featmap_strides=[16], out_channels=D)
    return cfg, dict(
        type="FasterRCNNPointSupAlign",
        backbone=dict(type="VisionTransformerDet", img_size=cfg["img_size"], patch_size=16, embed_dim=D, depth=cfg["depth"],
                      num_heads=cfg["num_heads"], mlp_ratio=4., qkv_bias=True, drop_path_rate=0., out_indices=cfg["out_indices"],
                      last_feat=True, point_tokens_num=cfg["point_tokens_num"], num_classes=ncls, return_attention=True),
        neck=dict(type="FPN", in_channels=[D] * 4, out_channels=64, num_outs=5),
        rpn_head=dict(SHIPPED_RPN_HEAD, in_channels=64, feat_channels=64,
                      anchor_generator=dict(type="AnchorGenerator", scales=[4], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64])),
        roi_head=dict(
            type="AttnShiftRoIHead", num_semantic_points=5, mean_shift_times_local=3, rng_mode="fast",
            bbox_roi_extractor=dict(roi, roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0)),
            mask_roi_extractor=dict(roi, roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0)),
            mil_head=dict(type="MAEBoxHeadMIL", in_channels=D, embed_dim=64, num_classes=ncls, num_layers_query=Lc, hidden_dim=128),
            bbox_head=dict(type="MAEBoxHeadRec", seed_thr=0.2, seed_multiple=0.5, cam_layer=Lc, with_reconstruct=False,
                           reg_decoded_bbox=True, loss_bbox=dict(type="GIoULoss", loss_weight=10.0), **dec),
            mask_head=dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **dec)),
        roi_skip_fpn=True, pos_mask_thr=0.35, neg_mask_thr=0.8, num_mask_point_gt=10, corr_size=21, obj_tau=0.9,
        train_cfg=dict(
            rpn=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True,
                                   ignore_iof_thr=-1),
                     sampler=dict(type="RandomSampler", num=64, pos_fraction=0.5, neg_pos_ub=-1, add_gt_as_proposals=False),
                     allowed_border=-1, pos_weight=-1, debug=False),
            rpn_proposal=dict(nms_pre=200, max_per_img=60, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0),
            rcnn=dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=0.5, neg_iou_thr=0.5, min_pos_iou=0.5),
                      sampler=dict(type="RandomSampler", num=32, pos_fraction=0.25, add_gt_as_proposals=True),
                      point_assigner=dict(type="HungarianPointAssigner", cls_cost=dict(weight=1.0), reg_cost=dict(weight=10.0)))),
        test_cfg=dict(rpn=dict(nms_pre=200, max_per_img=40, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0),
                      rcnn=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=10, mask_thr_binary=0.5)))


@pytest.fixture(scope="module")
def case(golden):
    g = golden("backbone_h4")
    cfg, model = model_dict(g)
    torch.manual_seed(0)
    det = A.build_detector(dict(model, compute_dtype=torch.bfloat16))   # neck and RPN trunk on as_conv2d_fwd at test time
    with torch.no_grad():
        for m in (det.rpn_head.rpn_cls, det.rpn_head.rpn_reg):
            m.weight.normal_(0, 0.05)                                    # spread the untrained proposals
    det = det.cuda()
    H, W = cfg["img_hw"]
    img = synthetic.images(2, H, W, seed=cfg["seed"]).cuda()
    one = np.ones(4, dtype=np.float32)
    metas = [dict(img_shape=(H, W, 3), ori_shape=(H, W, 3), pad_shape=(H, W, 3), scale_factor=one),
             dict(img_shape=(H - 16, W - 16, 3), ori_shape=(H - 16, W - 16, 3), pad_shape=(H, W, 3), scale_factor=one)]
    return det, img, metas, cfg


def same(a, b):
    if isinstance(a, (list, tuple)):
        return len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b))


def test_simple_test_is_the_stages_called_by_hand(case):
    det, img, metas, cfg = case
    det.eval()
    assert det.rpn_head.compute_dtype == torch.bfloat16 and det.neck.compute_dtype == torch.bfloat16
    with torch.no_grad():
        got = det.simple_test(img, metas)
        out = det.backbone(img)
        x = det.neck(out["feature"])
        assert len(x) == 5 and all(f.dtype == torch.bfloat16 and f.shape[1] == 64 for f in x)
        props = det.rpn_head.simple_test_rpn(x, metas)
        B, _, hp, wp = x[2].shape
        fmap = [out["last_feat"][:, 1:, :].transpose(1, 2).reshape(B, -1, hp, wp).contiguous()]
        want = det.roi_head.simple_test(fmap, props, metas, rescale=False)
        again = det.forward([img], [metas], return_loss=False)
    ncls = cfg["num_classes"]
    assert len(got) == 2
    for (boxes, segms), meta in zip(got, metas):
        assert len(boxes) == ncls and len(segms) == ncls and all(b.shape[1] == 5 for b in boxes)
        assert all(len(s) == b.shape[0] for s, b in zip(segms, boxes)) and sum(b.shape[0] for b in boxes) > 0
        assert all(np.asarray(m).shape == meta["ori_shape"][:2] for s in segms for m in s)
    assert same(got, want), "simple_test differs from backbone -> neck -> simple_test_rpn -> roi_head.simple_test"
    assert same(got, again), "forward(return_loss=False) differs from simple_test"
    with pytest.raises(NotImplementedError):
        det.forward([img, img], [metas, metas], return_loss=False)


def test_conv_launches_with_and_without_the_rpn_trunk_on_the_kernel(case, golden, monkeypatch):
    """compute_dtype handed down by the detector: neck and RPN trunk on as_conv2d_fwd, 8 + 10 launches; without it the neck's 8
    and the RPN head on torch's convolution.  (That detector's results are checked for their form only: the vendor's fp32
    convolution at the stride-4 level was measured to differ by some 4e-8 between two calls on the same input, so bit-equality
    with the stages called by hand is asserted above on the detector whose every stage is a kernel of this repository.)"""
    from attentionshift_amd import ops
    det, img, metas, cfg = case
    det.eval()
    _, model = model_dict(golden("backbone_h4"))
    plain = A.build_detector(model).cuda().eval()
    plain.load_state_dict(det.state_dict())
    assert plain.rpn_head.compute_dtype is None and plain.neck.compute_dtype == torch.bfloat16
    calls = []
    real = ops.conv2d_nhwc
    monkeypatch.setattr(ops, "conv2d_nhwc", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        det.simple_test(img, metas)
        assert len(calls) == 18
        got = plain.simple_test(img, metas)
        assert len(calls) == 18 + 8
    assert len(got) == 2 and all(len(b) == cfg["num_classes"] and sum(x.shape[0] for x in b) > 0 for b, _ in got)
    assert all(len(s) == b.shape[0] for bs, ss in got for s, b in zip(ss, bs))


def train_inputs(det, cfg, device):
    H, W = cfg["img_hw"]
    hp, wp, T, Lc = H // 16, W // 16, cfg["point_tokens_num"], cfg["cam_layer"]
    shift = [synthetic.shift_inputs(40 + b, hp, wp, cfg["embed_dim"], G, Lc) for b in range(2)]
    cams = torch.stack([s["cams"].flatten(2) for s in shift]).to(device)          # [B, Lc, G, Np]
    N = 1 + hp * wp + T

    def rollout_cams(attns, num_proposals, pos_inds=None):
        rows = torch.zeros(2, Lc, T, N, device=device)
        rows[:, :, :G, 1:-T] = cams
        return rows
    pos = [torch.arange(G, device=device) for _ in range(2)]
    return rollout_cams, dict(gt_labels=[(s["labels"] % cfg["num_classes"]).to(device) for s in shift],
                              gt_centers=[s["points"].to(device) for s in shift], pos_inds=pos, matched_gt=pos)


LOSSES = {"mil_loss", "loss_rpn_cls", "loss_rpn_bbox", "loss_point_cls", "loss_point", "loss_cls", "loss_bbox", "loss_mask"}


def test_forward_train_returns_every_stage_loss_with_gradients(case, monkeypatch):
    det, img, metas, cfg = case
    det.train()
    det.zero_grad(set_to_none=True)
    rollout_cams, kw = train_inputs(det, cfg, img.device)
    monkeypatch.setattr(det.roi_head, "rollout_cams", rollout_cams)
    with torch.enable_grad():                            # (allowed_border=-1: every anchor of the padded grid is inside)
        losses = det.forward_train(img, metas, generator=torch.Generator().manual_seed(4), **kw)
        assert LOSSES <= set(losses), sorted(losses)
        assert len(losses["loss_rpn_cls"]) == 5 and len(losses["loss_rpn_bbox"]) == 5
        total = sum(sum(v) if isinstance(v, list) else v for k, v in losses.items() if "loss" in k)
        assert bool(torch.isfinite(total))
        for k, v in losses.items():
            assert all(bool(torch.isfinite(t).all()) for t in (v if isinstance(v, list) else [v])), k
        total.backward()
    params = dict(det.named_parameters())
    for name in ("neck.lateral_convs.0.conv.weight", "neck.fpn_convs.3.conv.weight", "rpn_head.rpn_conv.weight",
                 "backbone.blocks.1.attn.qkv.weight", "roi_head.bbox_head.fc_cls.weight"):
        grad = params[name].grad
        assert grad is not None and bool(torch.isfinite(grad).all()), name
        assert float(grad.abs().sum()) > 0, name


def test_train_step_and_forward_with_losses(case, monkeypatch):
    det, img, metas, cfg = case
    det.train()
    rollout_cams, kw = train_inputs(det, cfg, img.device)
    monkeypatch.setattr(det.roi_head, "rollout_cams", rollout_cams)
    with torch.enable_grad():
        out = det.train_step(dict(img=img, img_metas=metas, generator=torch.Generator().manual_seed(4), **kw), None)
    assert sorted(out) == ["log_vars", "loss", "num_samples"] and out["num_samples"] == 2
    assert out["loss"].requires_grad and bool(torch.isfinite(out["loss"]))
    assert LOSSES <= set(out["log_vars"]) and "loss" in out["log_vars"]
    assert abs(sum(v for k, v in out["log_vars"].items() if "loss" in k and k != "loss") - out["log_vars"]["loss"]) \
        <= 1e-4 * abs(out["log_vars"]["loss"])
