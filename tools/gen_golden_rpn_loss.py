"""Golden vectors for the RPN's training targets and losses: executes the reference's own functions and classes (extracted
with ast, decorators dropped, because `import mmdet` needs mmcv) and stores inputs + outputs in tests/golden/rpn_loss.npz.
Needs the reference checkout (gen_golden_mmdet_pure.REF), like the other fixture generators.

    AnchorGenerator.grid_anchors, valid_flags,     mmdet/core/anchor/anchor_generator.py:142-328
      single_level_valid_flags
    anchor_inside_flags, images_to_levels          mmdet/core/anchor/utils.py:4-46
    unmap, multi_apply                             mmdet/core/utils/misc.py:10-42
    bbox_overlaps                                  mmdet/core/bbox/iou_calculators/iou2d_calculator.py
    MaxIoUAssigner, AssignResult                   mmdet/core/bbox/assigners
    BaseSampler, RandomSampler, SamplingResult     mmdet/core/bbox/samplers
    bbox2delta                                     mmdet/core/bbox/coder/delta_xywh_bbox_coder.py
    AnchorHead.get_anchors, _get_targets_single,   mmdet/models/dense_heads/anchor_head.py:140-493
      get_targets, loss_single, loss
    binary_cross_entropy, l1_loss,                 mmdet/models/losses/{cross_entropy_loss,smooth_l1_loss,utils}.py
      weighted_loss, weight_reduce_loss
The geometry is that of rpn.npz (levels 8x12 / 4x6 / 2x3 at strides 8 / 16 / 32, A = 3, two images of different img_shape);
the second image's pad_shape cuts the valid region below the feature maps.  Three calls under torch.manual_seed:
  0  the shipped setting (0.7 / 0.3 / 0.3, low-quality matches, allowed_border -1) with num = 32: the first image has more than
     16 positives (a draw), the second fewer (all taken).  The first image's boxes include a duplicate pair, a box equal to an
     anchor, a box whose best IoU is below min_pos_iou and a box centred between two anchors (a tie for its maximum).
  1  allowed_border 0, neg_pos_ub 3, pos_weight 2 on the same inputs
  2  the shipped setting with an image without boxes
"""
import os
import sys
import types
from abc import ABCMeta, abstractmethod
from functools import partial

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_golden_mmdet_pure import REF, grab                # noqa: E402
from gen_golden_sampler import NiceRepr, grab as grab_cls  # noqa: E402

SIZES, STRIDES = [(8, 12), (4, 6), (2, 3)], [8, 16, 32]
IMG_SHAPES, PAD_SHAPES = [(64, 96, 3), (60, 90, 3)], [(64, 96, 3), (56, 80, 3)]
SCALES, RATIOS = [4.0], [0.5, 1.0, 2.0]
MEANS, STDS = (0., 0., 0., 0.), (1., 1., 1., 1.)
SHIPPED = dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True, ignore_iof_thr=-1)
CALLS = [dict(allowed_border=-1, neg_pos_ub=-1, pos_weight=-1, boxes="full"),
         dict(allowed_border=0, neg_pos_ub=3, pos_weight=2, boxes="full"),
         dict(allowed_border=-1, neg_pos_ub=-1, pos_weight=-1, boxes="empty")]
NUM, POS_FRACTION = 32, 0.5


def namespace():
    ns = {"torch": torch, "np": np, "F": F, "ABCMeta": ABCMeta, "abstractmethod": abstractmethod, "partial": partial,
          "functools": __import__("functools"), "util_mixins": type("m", (), {"NiceRepr": NiceRepr})}
    B = REF + "/core/bbox"
    grab_cls(ns, B + "/iou_calculators/iou2d_calculator.py", ("bbox_overlaps",))
    ns["build_iou_calculator"] = lambda cfg: ns["bbox_overlaps"]
    grab_cls(ns, B + "/assigners/assign_result.py", ("AssignResult",))
    grab_cls(ns, B + "/assigners/base_assigner.py", ("BaseAssigner",))
    grab_cls(ns, B + "/assigners/max_iou_assigner.py", ("MaxIoUAssigner",))
    grab_cls(ns, B + "/samplers/sampling_result.py", ("SamplingResult",))
    grab_cls(ns, B + "/samplers/base_sampler.py", ("BaseSampler",))
    grab_cls(ns, B + "/samplers/random_sampler.py", ("RandomSampler",))
    dm = types.ModuleType("mmdet.core.bbox.demodata")                # RandomSampler.__init__ imports it for its rng argument
    dm.ensure_rng = lambda rng=None: np.random.mtrand._rand if rng is None else rng
    for name in ("mmdet", "mmdet.core", "mmdet.core.bbox"):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules["mmdet.core.bbox"].demodata = dm
    sys.modules["mmdet.core.bbox.demodata"] = dm
    grab(ns, B + "/coder/delta_xywh_bbox_coder.py", ("bbox2delta",))
    grab(ns, REF + "/core/anchor/utils.py", ("anchor_inside_flags", "images_to_levels"))
    grab(ns, REF + "/core/utils/misc.py", ("multi_apply", "unmap"))
    grab(ns, REF + "/models/losses/utils.py", ("reduce_loss", "weight_reduce_loss", "weighted_loss"))
    grab(ns, REF + "/models/losses/cross_entropy_loss.py", ("_expand_onehot_labels", "binary_cross_entropy"))
    grab(ns, REF + "/models/losses/smooth_l1_loss.py", ("l1_loss",))
    ag_names = ("gen_single_level_base_anchors", "single_level_grid_anchors", "_meshgrid", "grid_anchors", "valid_flags",
                "single_level_valid_flags")
    grab(ns, REF + "/core/anchor/anchor_generator.py", ag_names, methods_of="AnchorGenerator")
    ns["AG"] = type("AG", (), {k: ns[k] for k in ag_names})
    ah_names = ("get_anchors", "_get_targets_single", "get_targets", "loss_single", "loss")
    grab(ns, REF + "/models/dense_heads/anchor_head.py", ah_names, methods_of="AnchorHead")
    ns["Head"] = type("Head", (), {k: ns[k] for k in ah_names})
    return ns


def boxes_full(gen):
    """image 0: the special boxes + random ones; image 1: three boxes"""
    special = torch.tensor([[10., 12., 50., 44.], [10., 12., 50., 44.],        # a duplicate pair
                            [24., 8., 56., 40.],                               # = the square anchor of level 0 at (x 5, y 3)
                            [70., 50., 74., 53.],                              # best IoU below min_pos_iou
                            [28., 40., 60., 72.]])                             # centred between the square anchors x 5 / x 6 of row 7
    xy = torch.rand(19, 2, generator=gen) * torch.tensor([70., 40.])
    wh = 14 + torch.rand(19, 2, generator=gen) * 40
    rnd = torch.cat((xy, torch.min(xy + wh, torch.tensor([95., 63.]))), 1)
    img1 = torch.tensor([[5., 6., 40., 36.], [2., 0., 64., 48.], [20., 30., 36., 50.]])
    return [torch.cat((special, rnd)), img1]


def main():
    ns = namespace()
    ag = ns["AG"]()
    ag.center_offset, ag.scale_major = 0., True
    ag.strides = [(s, s) for s in STRIDES]
    ag.base_anchors = [ag.gen_single_level_base_anchors(s, torch.Tensor(SCALES), torch.Tensor(RATIOS)) for s in STRIDES]
    ag.num_levels, ag.num_base_anchors = len(STRIDES), [b.size(0) for b in ag.base_anchors]
    l1 = ns["weighted_loss"](ns["l1_loss"])
    gen = torch.Generator().manual_seed(2024)
    A, B = len(RATIOS) * len(SCALES), len(IMG_SHAPES)
    cls = [torch.randn(B, A, h, w, generator=gen) * 2 for h, w in SIZES]
    reg = [torch.randn(B, 4 * A, h, w, generator=gen) * 0.5 for h, w in SIZES]
    full = boxes_full(gen)
    metas = [dict(img_shape=i, pad_shape=p) for i, p in zip(IMG_SHAPES, PAD_SHAPES)]
    st = {"scales": np.float32(SCALES), "ratios": np.float32(RATIOS), "strides": np.int64(STRIDES), "sizes": np.int64(SIZES),
          "img_shapes": np.int64(IMG_SHAPES), "pad_shapes": np.int64(PAD_SHAPES), "num": np.int64(NUM),
          "pos_fraction": np.float64(POS_FRACTION), "assigner": np.float64([SHIPPED[k] for k in ("pos_iou_thr", "neg_iou_thr", "min_pos_iou")]),
          "n_calls": np.int64(len(CALLS))}
    for l in range(len(SIZES)):
        st[f"base_{l}"], st[f"cls_{l}"], st[f"reg_{l}"] = ag.base_anchors[l].numpy(), cls[l].numpy(), reg[l].numpy()
    for c, call in enumerate(CALLS):
        gts = full if call["boxes"] == "full" else [torch.zeros(0, 4), full[1]]
        head = ns["Head"]()
        head.anchor_generator, head.sampling, head.num_classes, head.cls_out_channels = ag, True, 1, 1
        head.use_sigmoid_cls, head.reg_decoded_bbox = True, False
        head.train_cfg = types.SimpleNamespace(allowed_border=call["allowed_border"], pos_weight=call["pos_weight"])
        head.assigner = ns["MaxIoUAssigner"](**SHIPPED)
        head.sampler = ns["RandomSampler"](num=NUM, pos_fraction=POS_FRACTION, neg_pos_ub=call["neg_pos_ub"], add_gt_as_proposals=False)
        head.bbox_coder = types.SimpleNamespace(encode=lambda a, g: ns["bbox2delta"](a, g, MEANS, STDS))
        head.loss_cls = lambda s, lab, w, avg_factor=None: 1.0 * ns["binary_cross_entropy"](s, lab, w, reduction="mean", avg_factor=avg_factor)
        head.loss_bbox = lambda p_, t, w, avg_factor=None: 1.0 * l1(p_, t, w, reduction="mean", avg_factor=avg_factor)
        rec = {"assign": [], "inside": [], "sample": [], "targets": None}
        assign0, sample0, inside0, targets0 = head.assigner.assign, head.sampler.sample, ns["anchor_inside_flags"], head.get_targets

        def assign(*a, **k):
            rec["assign"].append(assign0(*a, **k))
            return rec["assign"][-1]

        def sample(*a, **k):
            rec["sample"].append(sample0(*a, **k))
            return rec["sample"][-1]

        def inside(*a, **k):
            rec["inside"].append(inside0(*a, **k))
            return rec["inside"][-1]

        def targets(*a, **k):
            rec["targets"] = targets0(*a, **k)
            return rec["targets"]

        head.assigner.assign, head.sampler.sample, head.get_targets = assign, sample, targets
        ns["Head"]._get_targets_single.__globals__["anchor_inside_flags"] = inside
        seed = 300 + c
        torch.manual_seed(seed)
        losses = head.loss(cls, reg, gts, None, metas)
        ns["Head"]._get_targets_single.__globals__["anchor_inside_flags"] = inside0
        st[f"c{c}_seed"], st[f"c{c}_rng_after"] = np.int64(seed), torch.get_rng_state().numpy()
        st[f"c{c}_allowed_border"], st[f"c{c}_neg_pos_ub"] = np.int64(call["allowed_border"]), np.int64(call["neg_pos_ub"])
        st[f"c{c}_pos_weight"] = np.float64(call["pos_weight"])
        for b in range(B):
            st[f"c{c}_gt_{b}"] = gts[b].numpy()
            st[f"c{c}_inside_{b}"] = rec["inside"][b].numpy()
            st[f"c{c}_gt_inds_{b}"] = rec["assign"][b].gt_inds.numpy()
            st[f"c{c}_max_overlaps_{b}"] = rec["assign"][b].max_overlaps.numpy()
            st[f"c{c}_pos_inds_{b}"] = rec["sample"][b].pos_inds.numpy()
            st[f"c{c}_neg_inds_{b}"] = rec["sample"][b].neg_inds.numpy()
        for name, per_level in zip(("labels", "label_weights", "bbox_targets", "bbox_weights"), rec["targets"][:4]):
            for l, v in enumerate(per_level):
                st[f"c{c}_{name}_{l}"] = v.numpy()
        st[f"c{c}_loss_cls"] = torch.stack(losses["loss_cls"]).numpy()
        st[f"c{c}_loss_bbox"] = torch.stack(losses["loss_bbox"]).numpy()
        npos = [int(rec["assign"][b].gt_inds.gt(0).sum()) for b in range(B)]
        print(c, "positives", npos, "sampled", [(r.pos_inds.numel(), r.neg_inds.numel()) for r in rec["sample"]],
              "inside", [int(f.sum()) for f in rec["inside"]], "losses", st[f"c{c}_loss_cls"], st[f"c{c}_loss_bbox"])
        if c == 0:
            k = int(NUM * POS_FRACTION)
            assert npos[0] > k and 0 < npos[1] <= k, npos                        # a draw and a take-all
            ov = ns["bbox_overlaps"](gts[0], torch.cat(ag.grid_anchors(SIZES, "cpu")))
            gmax = ov.max(1)[0]
            assert float(gmax[2]) == 1.0 and float(gmax[3]) < SHIPPED["min_pos_iou"], gmax[:5]
            assert int((ov[4] == gmax[4]).sum()) >= 2                            # the tie
    path = os.path.join(ROOT, "tests", "golden", "rpn_loss.npz")
    np.savez_compressed(path, **st)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
