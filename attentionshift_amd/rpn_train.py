"""The RPN's training targets: mmdet's anchor-target stage restated once for two routes.

    rpn_assign       AnchorGenerator.valid_flags (mmdet/core/anchor/anchor_generator.py:272-328), anchor_inside_flags
                     (mmdet/core/anchor/utils.py:20-46) and MaxIoUAssigner.assign / assign_wrt_overlaps
                     (mmdet/core/bbox/assigners/max_iou_assigner.py:93-212) for all images of a batch
    rpn_sample       RandomSampler.sample without added GT boxes (samplers/base_sampler.py:34-100, random_sampler.py:31-79):
                     the draws come from the CPU generator exactly as the reference consumes it, after ONE readback of the
                     [B,2] counts; only rank lists go to the device
    rpn_targets      pos_assigned_gt_inds and DeltaXYWHBBoxCoder.encode of the sampled positives (anchor_head.py:237-243)
    dense_targets    the reference's dense per-level labels / label_weights / bbox_targets / bbox_weights
                     (_get_targets_single:227-268, images_to_levels) from the sparse result: tests and parity only
    rpn_loss         AnchorHead.loss / loss_single (anchor_head.py:375-493) evaluated on the sampled anchors alone

Anchor t of an image is level l, i = (y * W_l + x) * A + a, t = offset_l + i: the order of inference.rpn_candidates.
`assigned` is -2 on an anchor outside (it takes part in nothing), else -1 / 0 / box + 1.  CPU tensors take the tensor-op
route; device tensors run csrc/rpn_train.hip (ops.rpn_assign / rpn_sample / rpn_targets) unless AS_POST_HOST=1.  On the
device route no anchor, IoU matrix or dense target exists and `assigned` / `max_iou` are equal to the tensor-op route's on
every anchor.
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import inference, ops
from .assign import max_iou_assign
from .bbox_loss import bbox2delta

_CONSTS = {}


def _pair(v):
    return (int(v), int(v)) if not isinstance(v, (tuple, list)) else (int(v[0]), int(v[1]))


def _to_device(values, device, dtype=None):
    from .roi_head import to_device
    return to_device(values, device, dtype)


def _level_ends(sizes, A, device):
    """[L] int64 on `device`: the first anchor index past every level (uploaded once per geometry)"""
    key = (tuple(sizes), A, str(device))
    t = _CONSTS.get(key)
    if t is None:
        ends, n = [], 0
        for h, w in sizes:
            n += A * h * w
            ends.append(n)
        t = _CONSTS[key] = torch.tensor(ends, dtype=torch.int64).to(device)
    return t


def _valid_size(size, stride, pad_shape):
    """AnchorGenerator.valid_flags: (valid_h, valid_w) of a level"""
    (h, w), (sx, sy) = size, stride
    ph, pw = int(pad_shape[0]), int(pad_shape[1])
    return min(-(-ph // sy), h), min(-(-pw // sx), w)


def _all_anchors(base_anchors, sizes, strides):
    from .rpn import grid_anchors
    return torch.cat([grid_anchors(base_anchors[l], sizes[l], strides[l]) for l in range(len(sizes))])


def inside_flags(anchors, A, sizes, strides, img_meta, allowed_border):
    """valid_flags + anchor_inside_flags of one image -> bool [T]"""
    flags = []
    for size, stride in zip(sizes, strides):
        vh, vw = _valid_size(size, stride, img_meta["pad_shape"])
        vx = torch.arange(size[1], device=anchors.device) < vw
        vy = torch.arange(size[0], device=anchors.device) < vh
        flags.append((vy[:, None] & vx[None, :]).reshape(-1, 1).expand(-1, A).reshape(-1))
    flags = torch.cat(flags)
    if allowed_border >= 0:
        img_h, img_w = img_meta["img_shape"][:2]
        flags = flags & (anchors[:, 0] >= -allowed_border) & (anchors[:, 1] >= -allowed_border) & \
            (anchors[:, 2] < img_w + allowed_border) & (anchors[:, 3] < img_h + allowed_border)
    return flags


def any_inside(base_anchors, sizes, strides, img_meta, allowed_border):
    """Whether one image has an inside anchor, on the host and without the anchors: the flags are separable in x and y.
    base_anchors: per level [A,4] on the host (AnchorGenerator.base_anchors; a device tensor would be read back)."""
    base = torch.stack([b.detach().float().cpu() for b in base_anchors])
    for l, (size, stride) in enumerate(zip(sizes, strides)):
        vh, vw = _valid_size(size, stride, img_meta["pad_shape"])
        if vh <= 0 or vw <= 0:
            continue
        if allowed_border < 0:
            return True
        img_h, img_w = img_meta["img_shape"][:2]
        xs = (torch.arange(vw) * stride[0]).float()
        ys = (torch.arange(vh) * stride[1]).float()
        for a in range(base.shape[1]):
            okx = ((base[l, a, 0] + xs) >= -allowed_border) & ((base[l, a, 2] + xs) < img_w + allowed_border)
            oky = ((base[l, a, 1] + ys) >= -allowed_border) & ((base[l, a, 3] + ys) < img_h + allowed_border)
            if bool(okx.any()) and bool(oky.any()):
                return True
    return False


def _check_assigner(cfg, gt_bboxes_ignore):
    if cfg.get("type", "MaxIoUAssigner") != "MaxIoUAssigner":
        raise ValueError("rpn_assign: only MaxIoUAssigner")
    if isinstance(cfg.get("neg_iou_thr", 0.3), (tuple, list)):
        raise ValueError("rpn_assign: a tuple neg_iou_thr is not built")
    if not cfg.get("gt_max_assign_all", True):
        raise ValueError("rpn_assign: gt_max_assign_all=False is not built")
    if cfg.get("ignore_iof_thr", -1) > 0 and gt_bboxes_ignore is not None and \
            any(g is not None and g.numel() > 0 for g in gt_bboxes_ignore):
        raise ValueError("rpn_assign: ignore_iof_thr > 0 with gt_bboxes_ignore is not built")


def rpn_assign(base_anchors, featmap_sizes, strides, gt_bboxes, img_metas, assigner=None, allowed_border=-1,
               gt_bboxes_ignore=None):
    """base_anchors [L,A,4], featmap_sizes[l] = (H_l, W_l), strides[l] = (sx, sy), gt_bboxes[b] [G_b,4], img_metas[b] with
    pad_shape and img_shape, assigner = the MaxIoUAssigner settings (pos_iou_thr, neg_iou_thr, min_pos_iou,
    match_low_quality) -> a namespace with assigned [B,T] int32, max_iou [B,T] fp32 (0 outside), counts [B,2] int32 =
    (positives, negatives), and what rpn_sample / rpn_targets need.  The route follows base_anchors' device."""
    cfg = dict(assigner or {})
    _check_assigner(cfg, gt_bboxes_ignore)
    pos_thr, neg_thr = float(cfg.get("pos_iou_thr", 0.7)), float(cfg.get("neg_iou_thr", 0.3))
    min_pos, mlq = float(cfg.get("min_pos_iou", 0.0)), bool(cfg.get("match_low_quality", True))
    sizes = [(int(s[0]), int(s[1])) for s in featmap_sizes]
    strides = [_pair(s) for s in strides]
    dev, B = base_anchors.device, len(img_metas)
    L, A = int(base_anchors.shape[0]), int(base_anchors.shape[1])
    if len(sizes) != L or len(strides) != L or len(gt_bboxes) != B:
        raise ValueError(f"rpn_assign: {L} levels of base anchors, {len(sizes)} sizes, {len(strides)} strides; {B} images, "
                         f"{len(gt_bboxes)} box lists")
    base = base_anchors.detach().float().contiguous()
    gts = [g.detach().to(dev).float().reshape(-1, 4) for g in gt_bboxes]
    out = SimpleNamespace(base_anchors=base, sizes=sizes, strides=strides, A=A, gt_bboxes=gts, device_route=False,
                          T=sum(A * h * w for h, w in sizes))
    if inference._on_device(base):
        g_counts = [int(g.shape[0]) for g in gts]
        offs, n = [0], 0
        for c in g_counts:
            n += c
            offs.append(n)
        shapes = [[int(m["pad_shape"][0]), int(m["pad_shape"][1]), int(m["img_shape"][0]), int(m["img_shape"][1])] for m in img_metas]
        meta = _to_device(offs + [v for s in shapes for v in s], dev, torch.int32)       # one pinned copy
        out.gt_offsets, out.shapes = meta[:B + 1], meta[B + 1:].view(B, 4)
        out.gt_cat = torch.cat(gts).contiguous() if n else base.new_zeros(0, 4)
        out.sum_g, out.device_route = n, True
        out.assigned, out.max_iou, out.counts, out.workspace = ops.rpn_assign(
            base, sizes, strides, out.gt_cat, out.gt_offsets, n, max(g_counts, default=0), out.shapes, pos_thr, neg_thr, min_pos, mlq,
            int(allowed_border))
        return out
    anchors = _all_anchors(base, sizes, strides)
    assigned = torch.full((B, out.T), -2, dtype=torch.int32, device=dev)
    max_iou = base.new_zeros(B, out.T)
    for b in range(B):
        flags = inside_flags(anchors, A, sizes, strides, img_metas[b], allowed_border)
        if not bool(flags.any()):
            continue
        a, m = max_iou_assign(anchors[flags], gts[b], pos_thr, neg_thr, min_pos, mlq)
        assigned[b, flags] = a.to(torch.int32)
        max_iou[b, flags] = m
    out.anchors = anchors
    out.assigned, out.max_iou = assigned, max_iou
    out.counts = torch.stack(((assigned > 0).sum(1), (assigned == 0).sum(1)), 1).to(torch.int32)
    return out


def sample_plan(counts, num, pos_fraction, neg_pos_ub=-1, generator=None):
    """RandomSampler on the counts alone: counts = [(n_pos, n_neg)] per image in order -> per image
    (pos ranks | None = all, n_pos_sampled, neg ranks | None = all, n_neg_sampled).  A set that fits consumes no draw."""
    plan = []
    for n_pos, n_neg in counts:
        k = int(num * pos_fraction)
        pos_r = torch.randperm(n_pos, generator=generator)[:k] if n_pos > k else None
        n_ps = n_pos if pos_r is None else int(pos_r.numel())
        k_neg = num - n_ps
        if neg_pos_ub >= 0:
            k_neg = min(k_neg, int(neg_pos_ub * max(1, n_ps)))
        neg_r = torch.randperm(n_neg, generator=generator)[:k_neg] if n_neg > k_neg else None
        plan.append((pos_r, n_ps, neg_r, n_neg if neg_r is None else int(neg_r.numel())))
    return plan


def rpn_sample(asg, num=256, pos_fraction=0.5, neg_pos_ub=-1, generator=None):
    """-> a namespace with pos_inds / neg_inds [B,num] int64 (anchor indices ascending, -1 past their number) and the
    python lists n_pos / n_neg.  The counts of all images are read back once; the draws are the reference's."""
    num = int(num)
    B, dev = asg.assigned.shape[0], asg.assigned.device
    plan = sample_plan([tuple(c) for c in asg.counts.cpu().tolist()], num, pos_fraction, neg_pos_ub, generator)   # the readback
    n_pos, n_neg = [p[1] for p in plan], [p[3] for p in plan]
    if max(n_pos + n_neg, default=0) > num:
        raise ValueError(f"rpn_sample: a set larger than num = {num} (a negative pos_fraction or neg_pos_ub?)")
    out = SimpleNamespace(n_pos=n_pos, n_neg=n_neg, num=num)
    if asg.device_route:
        host = torch.zeros(B * 4 + B * 2 * num, dtype=torch.int32)
        hp, hr = host[:B * 4].view(B, 4), host[B * 4:].view(B, 2, num)
        for b, (pos_r, n_ps, neg_r, n_ns) in enumerate(plan):
            hp[b] = torch.tensor([n_ps, pos_r is None, n_ns, neg_r is None], dtype=torch.int32)
            if pos_r is not None:
                hr[b, 0, :n_ps] = pos_r.to(torch.int32)
            if neg_r is not None:
                hr[b, 1, :n_ns] = neg_r.to(torch.int32)
        both = _to_device(host, dev)                                                     # one pinned copy
        out.inds = ops.rpn_sample(asg.assigned, both[:B * 4].view(B, 4), both[B * 4:].view(B, 2, num), asg.workspace, asg.sum_g)
        out.pos_inds, out.neg_inds = out.inds[:, 0].long(), out.inds[:, 1].long()
        return out
    pos_inds = torch.full((B, num), -1, dtype=torch.int64, device=dev)
    neg_inds = torch.full((B, num), -1, dtype=torch.int64, device=dev)
    for b, (pos_r, n_ps, neg_r, n_ns) in enumerate(plan):
        pos_all = torch.nonzero(asg.assigned[b] > 0, as_tuple=False).flatten()
        neg_all = torch.nonzero(asg.assigned[b] == 0, as_tuple=False).flatten()
        pos_inds[b, :n_ps] = pos_all if pos_r is None else pos_all[pos_r.to(dev)].unique()
        neg_inds[b, :n_ns] = neg_all if neg_r is None else neg_all[neg_r.to(dev)].unique()
    out.pos_inds, out.neg_inds = pos_inds, neg_inds
    return out


def rpn_targets(asg, smp, means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """-> (pos_gt [B,num] int64: the box every sampled positive is assigned to, -1 past their number;
    pos_delta [B,num,4] fp32 = bbox2delta(anchor, that box, means, stds), zeros past their number)."""
    if asg.device_route:
        pos_gt, pos_delta = ops.rpn_targets(asg.base_anchors, asg.sizes, asg.strides, asg.gt_cat, asg.gt_offsets, asg.sum_g,
                                            asg.assigned, smp.inds, means, stds)
        return pos_gt.long(), pos_delta
    B, dev = asg.assigned.shape[0], asg.assigned.device
    pos_gt = torch.full((B, smp.num), -1, dtype=torch.int64, device=dev)
    pos_delta = asg.base_anchors.new_zeros(B, smp.num, 4)
    for b in range(B):
        n = smp.n_pos[b]
        if n:
            t = smp.pos_inds[b, :n]
            g = asg.assigned[b, t].long() - 1
            pos_gt[b, :n] = g
            pos_delta[b, :n] = bbox2delta(asg.anchors[t], asg.gt_bboxes[b][g], means, stds)
    return pos_gt, pos_delta


def dense_targets(asg, smp, pos_delta, pos_weight=-1):
    """(tests and parity only) the reference's per-level targets: lists over the levels of labels [B,n_l] int64 (0 = object,
    1 = background), label_weights [B,n_l], bbox_targets [B,n_l,4], bbox_weights [B,n_l,4]."""
    B, T, dev = asg.assigned.shape[0], asg.T, asg.assigned.device
    labels = torch.ones(B, T, dtype=torch.int64, device=dev)
    lw, bt, bw = pos_delta.new_zeros(B, T), pos_delta.new_zeros(B, T, 4), pos_delta.new_zeros(B, T, 4)
    for b in range(B):
        p, n = smp.pos_inds[b, :smp.n_pos[b]], smp.neg_inds[b, :smp.n_neg[b]]
        labels[b, p] = 0
        lw[b, p] = 1.0 if pos_weight <= 0 else float(pos_weight)
        lw[b, n] = 1.0
        bt[b, p] = pos_delta[b, :smp.n_pos[b]]
        bw[b, p] = 1.0
    ns = [asg.A * h * w for h, w in asg.sizes]
    return tuple(list(torch.split(v, ns, dim=1)) for v in (labels, lw, bt, bw))


def rpn_loss(cls_scores, bbox_preds, asg, smp, pos_delta, pos_weight=-1, loss_cls_weight=1.0, loss_bbox_weight=1.0):
    """AnchorHead.loss on the sampled anchors: cls_scores[l] [B,A,H_l,W_l], bbox_preds[l] [B,4A,H_l,W_l] ->
    (loss_cls [L], loss_bbox [L]): per level sum(BCE_with_logits(logit, label) * label_weight) / avg and
    sum(|delta - target| * bbox_weight) / avg, avg = sum_images max(n_pos, 1) + sum_images max(n_neg, 1).  Only the
    gathered logits and deltas are evaluated; the per-level sums are an index_add on every index's level."""
    B, L = cls_scores[0].shape[0], len(cls_scores)
    flat_cls = torch.cat([c.float().permute(0, 2, 3, 1).reshape(B, -1) for c in cls_scores], dim=1)
    flat_reg = torch.cat([r.float().permute(0, 2, 3, 1).reshape(B, -1, 4) for r in bbox_preds], dim=1)
    if flat_cls.shape[1] != asg.T:
        raise ValueError(f"rpn_loss: {flat_cls.shape[1]} logits per image for {asg.T} anchors")
    ends = _level_ends(asg.sizes, asg.A, flat_cls.device)
    avg = float(sum(max(n, 1) for n in smp.n_pos) + sum(max(n, 1) for n in smp.n_neg))
    pos_ok, neg_ok = smp.pos_inds >= 0, smp.neg_inds >= 0
    pos_i, neg_i = smp.pos_inds.clamp(min=0), smp.neg_inds.clamp(min=0)
    pos_l, neg_l = torch.bucketize(pos_i, ends, right=True), torch.bucketize(neg_i, ends, right=True)
    lp, ln = flat_cls.gather(1, pos_i), flat_cls.gather(1, neg_i)
    w_pos = 1.0 if pos_weight <= 0 else float(pos_weight)
    ce_p = F.binary_cross_entropy_with_logits(lp, torch.ones_like(lp), reduction="none") * (pos_ok.to(lp.dtype) * w_pos)
    ce_n = F.binary_cross_entropy_with_logits(ln, torch.zeros_like(ln), reduction="none") * neg_ok.to(ln.dtype)
    loss_cls = flat_cls.new_zeros(L).index_add(0, pos_l.reshape(-1), ce_p.reshape(-1)).index_add(0, neg_l.reshape(-1), ce_n.reshape(-1))
    dp = flat_reg.gather(1, pos_i[:, :, None].expand(-1, -1, 4))
    l1 = ((dp - pos_delta).abs() * pos_ok[:, :, None].to(dp.dtype)).sum(-1)
    loss_bbox = flat_cls.new_zeros(L).index_add(0, pos_l.reshape(-1), l1.reshape(-1))
    return loss_cls * (loss_cls_weight / avg), loss_bbox * (loss_bbox_weight / avg)
