"""Golden vectors for the proposal generator: executes the reference's own functions (extracted with ast, decorators
dropped, because `import mmdet` needs mmcv) on seeded inputs and stores inputs + outputs in tests/golden/rpn.npz.
Container-only (needs /root/reference).

    gen_single_level_base_anchors,   mmdet/core/anchor/anchor_generator.py:142-270
    single_level_grid_anchors
    delta2bbox                       mmdet/core/bbox/coder/delta_xywh_bbox_coder.py:134-237
    RPNHead._get_bboxes              mmdet/models/dense_heads/rpn_head.py:82-236
mmcv's batched_nms (absent here) is supplied as its definition: boxes offset by class * (largest coordinate + 1), then the
oracle's nms_mmcv.  B = 2 images of different shapes, A = 3, levels 8x12 / 4x6 / 2x3 at strides 8 / 16 / 32, nms_pre 100
(level 0 is cut, levels 1 and 2 pass whole), max_per_img 60, IoU 0.7.  Seeds are searched until no two logits of an image are
equal, no same-level candidate pair lies within 1e-3 of the IoU threshold and NMS both removes and keeps something on
every image; the seed and the achieved margin are stored.
"""
import copy
import os
import sys
import types
import warnings

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from attentionshift_amd.config import ConfigDict          # noqa: E402
from attnshift_oracle import nms_mmcv                      # noqa: E402
from gen_golden_mmdet_pure import REF, grab                # noqa: E402

SIZES, STRIDES = [(8, 12), (4, 6), (2, 3)], [8, 16, 32]
IMG_SHAPES = [(64, 96, 3), (60, 90, 3)]
SCALES, RATIOS = [4.0], [0.5, 1.0, 2.0]
NMS_PRE, MAX_PER_IMG, IOU, MARGIN = 100, 60, 0.7, 1e-3


def batched_nms(boxes, scores, idxs, nms_cfg):
    """mmcv.ops.batched_nms (class_agnostic=False, fewer than split_thr boxes)"""
    offsets = idxs.to(boxes) * (boxes.max() + 1)
    keep = torch.from_numpy(nms_mmcv((boxes + offsets[:, None]).numpy(), scores.numpy(), nms_cfg["iou_threshold"]))
    return torch.cat((boxes[keep], scores[keep, None]), -1), keep


def iou_matrix(b):
    b = b.double()
    area = (b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1])
    wh = (torch.min(b[:, None, 2:], b[None, :, 2:]) - torch.max(b[:, None, :2], b[None, :, :2])).clamp(min=0)
    inter = wh[..., 0] * wh[..., 1]
    return inter / (area[:, None] + area[None, :] - inter).clamp(min=1e-12)


def main():
    ns = {"torch": torch, "np": np, "copy": copy, "warnings": warnings, "ConfigDict": ConfigDict, "batched_nms": batched_nms}
    grab(ns, REF + "/core/anchor/anchor_generator.py", ("gen_single_level_base_anchors", "single_level_grid_anchors", "_meshgrid"),
         methods_of="AnchorGenerator")
    grab(ns, REF + "/core/bbox/coder/delta_xywh_bbox_coder.py", ("delta2bbox",))
    grab(ns, REF + "/models/dense_heads/rpn_head.py", ("_get_bboxes",), methods_of="RPNHead")
    AG = type("AG", (), {k: ns[k] for k in ("gen_single_level_base_anchors", "single_level_grid_anchors", "_meshgrid")})
    ag = AG()
    ag.center_offset, ag.scale_major = 0., True
    base = [ag.gen_single_level_base_anchors(s, torch.Tensor(SCALES), torch.Tensor(RATIOS)) for s in STRIDES]
    grids = [ag.single_level_grid_anchors(b, fs, (s, s), device="cpu") for b, fs, s in zip(base, SIZES, STRIDES)]
    means, stds = (0., 0., 0., 0.), (1., 1., 1., 1.)
    Head = type("Head", (), {"_get_bboxes": ns["_get_bboxes"]})
    head = Head()
    head.use_sigmoid_cls, head.test_cfg = True, None
    head.bbox_coder = types.SimpleNamespace(
        decode=lambda anchors, preds, max_shape=None: ns["delta2bbox"](anchors, preds, means, stds, max_shape, 16 / 1000, True))
    cfg = ConfigDict(nms_pre=NMS_PRE, max_per_img=MAX_PER_IMG, nms=ConfigDict(type="nms", iou_threshold=IOU), min_bbox_size=0)
    A, B = len(RATIOS) * len(SCALES), len(IMG_SHAPES)
    for seed in range(1000):
        gen = torch.Generator().manual_seed(seed)
        cls = [torch.randn(B, A, h, w, generator=gen) * 2 for h, w in SIZES]
        reg = [torch.randn(B, 4 * A, h, w, generator=gen) * 0.5 for h, w in SIZES]
        flat = [torch.cat([c[b].reshape(-1) for c in cls]) for b in range(B)]
        if any(f.unique().numel() != f.numel() for f in flat):
            continue
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            dets = head._get_bboxes(cls, reg, grids, IMG_SHAPES, None, cfg)
        # the candidates of the reference, to measure the margin and to name every kept box by (level, index)
        margin, ok, kept = 1.0, True, []
        for b in range(B):
            boxes, levels, index = [], [], []
            for l in range(len(SIZES)):
                lg = cls[l][b].permute(1, 2, 0).reshape(-1)
                idx = lg.sort(descending=True)[1][:NMS_PRE] if lg.numel() > NMS_PRE else torch.arange(lg.numel())
                dl = reg[l][b].permute(1, 2, 0).reshape(-1, 4)[idx]
                boxes.append(ns["delta2bbox"](grids[l][idx], dl, means, stds, IMG_SHAPES[b], 16 / 1000, True))
                levels.append(torch.full_like(idx, l)); index.append(idx)
            boxes, levels, index = torch.cat(boxes), torch.cat(levels), torch.cat(index)
            iou = iou_matrix(boxes)
            same = (levels[:, None] == levels[None, :]) & ~torch.eye(len(levels), dtype=torch.bool)
            margin = min(margin, float((iou[same] - IOU).abs().min()))
            d = dets[b]
            # a kept box is one of the candidates, bit for bit
            match = (boxes[None, :, :] == d[:, None, :4]).all(-1)
            if not bool((match.sum(1) == 1).all()):
                ok = False
                break
            pos = match.float().argmax(1)
            kept.append(torch.stack((levels[pos], index[pos]), 1))
            full = batched_nms(boxes, torch.cat([cls[l][b].permute(1, 2, 0).reshape(-1)[index[levels == l]].sigmoid()
                                                 for l in range(len(SIZES))]), levels, cfg.nms)[1]
            if not (0 < len(full) < len(boxes)) or len(d) == 0:
                ok = False
                break
        if ok and margin > MARGIN:
            break
    else:
        raise SystemExit("no seed satisfies the conditions")
    st = {"seed": np.int64(seed), "iou_margin": np.float64(margin), "scales": np.float32(SCALES), "ratios": np.float32(RATIOS),
          "strides": np.int64(STRIDES), "sizes": np.int64(SIZES), "img_shapes": np.int64(IMG_SHAPES),
          "nms_pre": np.int64(NMS_PRE), "max_per_img": np.int64(MAX_PER_IMG), "iou_threshold": np.float64(IOU)}
    for l in range(len(SIZES)):
        st[f"base_{l}"], st[f"grid_{l}"] = base[l].numpy(), grids[l].numpy()
        st[f"cls_{l}"], st[f"reg_{l}"] = cls[l].numpy(), reg[l].numpy()
    for b in range(B):
        st[f"dets_{b}"], st[f"kept_{b}"] = dets[b].numpy(), kept[b].numpy()
    path = os.path.join(ROOT, "tests", "golden", "rpn.npz")
    np.savez_compressed(path, **st)
    print("wrote", path, "seed", seed, "margin", margin, [tuple(d.shape) for d in dets], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
