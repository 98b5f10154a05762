"""Test-time post-processing of the RoI head (restated from their definitions because mmcv's ops are absent here).
CPU tensors take the tensor-op route below; device tensors run NMS and the mask paste on the HIP kernels of
csrc/detect_post.hip (ops.nms / ops.paste_masks), unless AS_POST_HOST=1 forces the tensor-op route there too (A/B):

    nms / multiclass_nms   mmcv.ops.nms (greedy, IoU without the +1 offset) + mmdet/core/post_processing/bbox_nms.py:
                           scores above score_thr, class-aware suppression through per-class coordinate offsets, the
                           max_per_img best detections (configs/mae/attnshift_voc12aug.py:200-204: 0.05 / IoU 0.5 / 100)
    get_det_bboxes         BBoxHead.get_bboxes: softmax scores, DeltaXYWH decode clipped to the image, rescale
    paste_masks            fcn_mask_head._do_paste_mask: the RoI-sized mask resampled onto the image grid of its box
    get_seg_masks          mae_mask_head_pointSup.py:277-375: sigmoid, paste, threshold, per-class lists
    bbox2result            mmdet/core/bbox/transforms.py: per-class [n,5] arrays
    rle_encode /           mmdet/core/mask/utils.py:36-63 (what mmdet/apis/test.py:60,100 does to every result):
    encode_mask_results    pycocotools.mask.encode of every mask in Fortran order, restated (pycocotools is not needed);
                           device tensors are encoded by the kernels of csrc/rle.hip (ops.rle_encode)
    rpn_candidates /       mmdet/models/dense_heads/rpn_head.py:82-236 (RPNHead._get_bboxes): per-level top nms_pre by
    rpn_nms /              logit, anchors (anchor_generator.py:142-270), delta2bbox, minimum size, then mmcv's batched_nms
    rpn_proposals          with the level as the class; device tensors run csrc/rpn.hip (ops.rpn_candidates) and as_nms
    det_candidates         get_det_bboxes up to the NMS as select / order / decode-the-survivors; device tensors run
                           csrc/det.hip (ops.det_candidates).  Opt-in: get_det_bboxes(fused=True), test_cfg.fused_det
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from .assign import bbox_overlaps
from .bbox_loss import delta2bbox


def _on_device(t):
    """True when `t` takes the HIP route: a device tensor, and the host route not forced."""
    return t.is_cuda and os.environ.get("AS_POST_HOST") != "1"


def nms(boxes, scores, iou_threshold, max_keep=-1):
    """Greedy NMS; returns kept indices sorted by decreasing score (device route: at most max_keep of them when
    max_keep > 0 -- the prefix of the full result; it takes up to 65535 boxes and raises beyond)."""
    if boxes.numel() == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes.device)
    order = scores.argsort(descending=True, stable=True)
    return order[_nms_in_order(boxes[order], iou_threshold, max_keep)]


def multiclass_nms(multi_bboxes, multi_scores, score_thr, iou_threshold, max_num=-1):
    """multi_bboxes [n, 4K] or [n, 4], multi_scores [n, K+1] (last column = background) ->
    (dets [m,5] sorted by score, labels [m])."""
    K = multi_scores.size(1) - 1
    if multi_bboxes.shape[1] > 4:
        bboxes = multi_bboxes.view(multi_scores.size(0), multi_bboxes.shape[1] // 4, 4)
    else:
        bboxes = multi_bboxes[:, None].expand(multi_scores.size(0), K, 4)
    scores = multi_scores[:, :-1]
    labels = torch.arange(K, dtype=torch.long, device=scores.device).view(1, -1).expand_as(scores)
    valid = scores > score_thr
    bboxes, scores, labels = bboxes[valid], scores[valid], labels[valid]
    if bboxes.numel() == 0:
        return multi_bboxes.new_zeros(0, 5), labels
    offsets = labels.to(bboxes) * (bboxes.max() + 1)                        # boxes of different classes never overlap
    keep = nms(bboxes + offsets[:, None], scores, iou_threshold, max_num)
    if max_num > 0:
        keep = keep[:max_num]
    return torch.cat((bboxes[keep], scores[keep, None]), dim=1), labels[keep]


def _nms_in_order(boxes_sorted, iou_threshold, max_keep=-1):
    """Greedy NMS over boxes that are in visiting order already -> kept positions, ascending (device route: at most
    max_keep of them when max_keep > 0)."""
    n = boxes_sorted.shape[0]
    if n == 0:
        return torch.zeros(0, dtype=torch.long, device=boxes_sorted.device)
    if _on_device(boxes_sorted):
        return ops.nms(boxes_sorted.contiguous().float(), iou_threshold, max_keep)
    iou = bbox_overlaps(boxes_sorted, boxes_sorted, eps=1e-12).cpu()
    alive = torch.ones(n, dtype=torch.bool)
    keep = []
    for i in range(n):
        if alive[i]:
            keep.append(i)
            alive &= ~(iou[i] > iou_threshold)
            alive[i] = False
    return torch.tensor(keep, dtype=torch.long, device=boxes_sorted.device)


def _rpn_candidates_host(cls_scores, bbox_preds, base_anchors, strides, img_shapes, nms_pre, min_bbox_size, means, stds):
    """The definition of rpn_candidates in tensor ops (any device)."""
    from .rpn import grid_anchors
    L, B, dev = len(cls_scores), cls_scores[0].shape[0], cls_scores[0].device
    C = ops.rpn_candidate_count(cls_scores, nms_pre)
    out_box, out_nms = cls_scores[0].new_zeros(B, C, 4), cls_scores[0].new_zeros(B, C, 4)
    out_score = cls_scores[0].new_zeros(B, C)
    out_level = torch.zeros(B, C, dtype=torch.int32, device=dev)
    out_index = torch.zeros(B, C, dtype=torch.int32, device=dev)
    out_count = torch.zeros(B, dtype=torch.int32, device=dev)
    anchors = [grid_anchors(base_anchors[l].to(dev), cls_scores[l].shape[2:], strides[l]) for l in range(L)]
    for b in range(B):
        logits, deltas, anch, levels, index = [], [], [], [], []
        for l in range(L):
            lg = cls_scores[l][b].permute(1, 2, 0).reshape(-1)
            dl = bbox_preds[l][b].permute(1, 2, 0).reshape(-1, 4)
            idx = torch.arange(lg.numel(), device=dev)
            if 0 < nms_pre < lg.numel():
                idx = torch.sort(lg, descending=True, stable=True)[1][:nms_pre]
            logits.append(lg[idx]); deltas.append(dl[idx]); anch.append(anchors[l][idx]); index.append(idx)
            levels.append(torch.full_like(idx, l))
        logits, deltas, anch, levels, index = (torch.cat(v) for v in (logits, deltas, anch, levels, index))
        order = torch.sort(logits, descending=True, stable=True)[1]        # ties keep (level, index) order
        logits, deltas, anch, levels, index = (v[order] for v in (logits, deltas, anch, levels, index))
        boxes = delta2bbox(anch, deltas, means, stds, max_shape=img_shapes[b])
        scores = 1 / (1 + torch.exp(-logits))
        if min_bbox_size > 0:
            ok = ((boxes[:, 2] - boxes[:, 0]) >= min_bbox_size) & ((boxes[:, 3] - boxes[:, 1]) >= min_bbox_size)
            boxes, scores, levels, index = boxes[ok], scores[ok], levels[ok], index[ok]
        m = boxes.shape[0]
        if m:
            out_box[b, :m], out_score[b, :m] = boxes, scores
            out_nms[b, :m] = boxes + (levels.to(boxes) * (boxes.max() + 1))[:, None]
            out_level[b, :m], out_index[b, :m] = levels.to(torch.int32), index.to(torch.int32)
        out_count[b] = m
    return out_box, out_nms, out_score, out_level, out_index, out_count


def rpn_candidates(cls_scores, bbox_preds, base_anchors, strides, img_shapes, nms_pre, min_bbox_size=0, means=(0., 0., 0., 0.),
                   stds=(1., 1., 1., 1.)):
    """The RPN's test-time stage before NMS (mmdet/models/dense_heads/rpn_head.py:82-231).  cls_scores[l] [B,A,H_l,W_l],
    bbox_preds[l] [B,4A,H_l,W_l] fp32, base_anchors [L,A,4], strides[l] = (sx, sy), img_shapes[b] = (h, w[, c]).
    Candidate i = (y * W_l + x) * A + a of level l has the logit cls[b,a,y,x] and the anchor base[l][a] + its grid shift.
    Everywhere the order is (logit descending, level ascending, i ascending; -0.0 == +0.0, NaN first).  Every (image,
    level) keeps its first min(nms_pre, n_l) candidates (nms_pre <= 0: all); they are decoded (delta2bbox clipped to the
    image, score = sigmoid of the logit), those narrower or lower than min_bbox_size (when > 0) are dropped, and the rest
    returned per image in that order:
        (cand_box [B,C,4], cand_nms_box [B,C,4], cand_score [B,C], cand_level [B,C] int32, cand_index [B,C] int32,
         cand_count [B] int32),  C = sum_l min(nms_pre, n_l);  rows past an image's count carry no meaning.
    cand_nms_box = box + level * (M + 1), M the image's largest remaining coordinate (batched_nms with the level as the
    class).  Device tensors run csrc/rpn.hip (ops.rpn_candidates) unless AS_POST_HOST=1; CPU tensors the tensor ops."""
    cls_scores = [c.float().contiguous() for c in cls_scores]
    bbox_preds = [r.float().contiguous() for r in bbox_preds]
    strides = [(s, s) if isinstance(s, int) else (int(s[0]), int(s[1])) for s in strides]
    if not torch.is_tensor(base_anchors):
        base_anchors = torch.stack(list(base_anchors))
    if _on_device(cls_scores[0]):
        return ops.rpn_candidates(cls_scores, bbox_preds, base_anchors, strides, img_shapes, nms_pre, min_bbox_size, means, stds)
    return _rpn_candidates_host(cls_scores, bbox_preds, base_anchors.float(), strides, img_shapes, nms_pre, min_bbox_size, means,
                                stds)


def rpn_nms(cand_box, cand_nms_box, cand_score, iou_threshold, max_per_img=-1):
    """One image's candidates in their order -> proposals [m,5]: greedy NMS over the level-offset boxes, the first
    max_per_img kept (all when <= 0), the un-offset boxes and the score; and the kept positions."""
    keep = _nms_in_order(cand_nms_box, iou_threshold, max_per_img)
    if max_per_img > 0:
        keep = keep[:max_per_img]
    return torch.cat((cand_box[keep], cand_score[keep, None]), dim=1), keep


def rpn_proposals(cls_scores, bbox_preds, base_anchors, strides, img_shapes, nms_pre, max_per_img, iou_threshold, min_bbox_size=0,
                  means=(0., 0., 0., 0.), stds=(1., 1., 1., 1.)):
    """RPNHead._get_bboxes (mmdet/models/dense_heads/rpn_head.py:82-236): rpn_candidates, then per image mmcv's batched_nms
    with the level as the class at iou_threshold and the first max_per_img survivors -> list of [m,5] (x1,y1,x2,y2,score),
    [0,5] when nothing survives.  On the device route nothing is read back before NMS unless min_bbox_size > 0 (the
    counts, once for all images)."""
    box, nms_box, score, _, _, count = rpn_candidates(cls_scores, bbox_preds, base_anchors, strides, img_shapes, nms_pre,
                                                      min_bbox_size, means, stds)
    B, C = score.shape
    counts = [C] * B if min_bbox_size <= 0 else count.tolist()
    return [rpn_nms(box[b, :m], nms_box[b, :m], score[b, :m], iou_threshold, max_per_img)[0] for b, m in enumerate(counts)]


def _final_boxes(rois, img_shape):
    """bbox_pred is None: the RoIs clamped to the image are the boxes (the tensor ops of BBoxHead.get_bboxes)"""
    bboxes = rois[:, 1:].clone()
    bboxes[:, 0::2] = bboxes[:, 0::2].clamp(0, img_shape[1])
    bboxes[:, 1::2] = bboxes[:, 1::2].clamp(0, img_shape[0])
    return bboxes


def _det_candidates_host(boxes_or_rois, bbox_pred, scores, img_shape, scale, score_thr, means, stds, apply_softmax=True,
                         return_prob=False):
    """The definition of det_candidates in the tensor ops of get_det_bboxes / multiclass_nms (any device).  boxes_or_rois:
    the RoIs [n,4] with bbox_pred, else final boxes [n,4] / [n,4K]; scale: 4 divisors or None."""
    n, K = scores.shape[0], scores.shape[1] - 1
    dev = scores.device
    prob = F.softmax(scores, dim=-1) if apply_softmax else scores
    if bbox_pred is not None:
        bboxes = delta2bbox(boxes_or_rois, bbox_pred, means, stds, max_shape=img_shape)
    else:
        bboxes = boxes_or_rois
    if scale is not None and bboxes.size(0) > 0:
        sf = bboxes.new_tensor(scale)
        bboxes = (bboxes.view(bboxes.size(0), bboxes.shape[1] // 4, 4) / sf).view(bboxes.size(0), -1)
    cap = min(n * K, ops.DET_MAX_CANDIDATES)
    out_box, out_nms = prob.new_zeros(cap, 4), prob.new_zeros(cap, 4)
    out_score = prob.new_zeros(cap)
    out_roi = torch.zeros(cap, dtype=torch.int32, device=dev)
    out_label = torch.zeros(cap, dtype=torch.int32, device=dev)
    if bboxes.shape[1] > 4:
        bboxes = bboxes.view(n, bboxes.shape[1] // 4, 4)
    else:
        bboxes = bboxes[:, None].expand(n, K, 4)
    sc = prob[:, :-1]
    labels = torch.arange(K, dtype=torch.long, device=dev).view(1, -1).expand_as(sc)
    rows = torch.arange(n, dtype=torch.long, device=dev).view(-1, 1).expand_as(sc)
    valid = sc > score_thr
    bboxes, sc, labels, rows = bboxes[valid], sc[valid], labels[valid], rows[valid]
    m = int(sc.numel())
    if 0 < m <= cap:
        offsets = labels.to(bboxes) * (bboxes.max() + 1)
        order = sc.argsort(descending=True, stable=True)
        out_box[:m], out_score[:m] = bboxes[order], sc[order]
        out_nms[:m] = (bboxes + offsets[:, None])[order]
        out_roi[:m], out_label[:m] = rows[order].to(torch.int32), labels[order].to(torch.int32)
    out = (out_box, out_nms, out_score, out_roi, out_label, torch.tensor([m], dtype=torch.int32, device=dev))
    return out + (prob,) if return_prob else out


def det_candidates(rois, cls_score, bbox_pred, img_shape, scale_factor, rescale, score_thr=0.05, means=(0., 0., 0., 0.),
                   stds=(0.1, 0.1, 0.2, 0.2), apply_softmax=True, return_prob=False):
    """The box head's test-time stage before NMS for ONE image: BBoxHead.get_bboxes and the front of multiclass_nms
    (mmdet/core/post_processing/bbox_nms.py:34-93) as select, order, decode only the survivors.  rois [n,5] (batch index
    first), cls_score [n,K+1] (the last column is the background), bbox_pred [n,4] / [n,4K] or None.
      Scores: p = cls_score, or with apply_softmax p[r,c] = exp(x[r,c] - max x[r,:]) / sum exp(x[r,:] - max) over the K + 1
        columns in fp32; a row holding NaN or +inf has NaN probabilities and no candidate.
      Candidates: all (r, c), c < K, with p[r,c] > fp32(score_thr), compared in fp32; a NaN never qualifies.
      Order: score descending, then the flat index r * K + c ascending; -0.0 == +0.0 (a stable descending argsort).
      Box of (r, c): delta2bbox of RoI r with the deltas of column block c (block 0 for [n,4] deltas): means, stds, dw / dh
        clamped to +-|log(16/1000)|, clipped to img_shape; bbox_pred None: the RoI clamped to the image.  With rescale each
        coordinate j is then divided by scale_factor[j] (a scalar factor divides all four).
    -> (cand_box [cap,4], cand_nms_box [cap,4], cand_score [cap], cand_roi [cap] int32, cand_label [cap] int32,
        cand_count [1] int32[, prob [n,K+1]]), cap = min(n * K, 65535), the first m = cand_count rows in that order;
    cand_nms_box = cand_box + label * (M + 1) in fp32, M the largest coordinate of all candidate boxes (batched_nms' class
    offset: the input of NMS).  With m > 65535 only the count is meaningful.  Device tensors run csrc/det.hip
    (ops.det_candidates: every step but exp rounds as the tensor ops, nothing is read back) unless AS_POST_HOST=1; CPU
    tensors the tensor ops of get_det_bboxes / multiclass_nms themselves."""
    cls_score = cls_score.float().contiguous()
    scale = None
    if rescale:
        scale = [float(v) for v in np.broadcast_to(np.asarray(scale_factor, dtype=np.float32).reshape(-1), (4,))]
    deltas = bbox_pred.float().contiguous() if bbox_pred is not None else None
    boxes = rois[:, 1:].float().contiguous() if bbox_pred is not None else _final_boxes(rois.float(), img_shape).contiguous()
    if _on_device(cls_score):
        return ops.det_candidates(boxes, deltas, cls_score, score_thr, img_shape, scale, means, stds, apply_softmax, return_prob)
    return _det_candidates_host(boxes, deltas, cls_score, img_shape, scale, score_thr, means, stds, apply_softmax, return_prob)


def get_det_bboxes(rois, cls_score, bbox_pred, img_shape, scale_factor, rescale, score_thr=0.05, iou_threshold=0.5,
                   max_per_img=100, means=(0., 0., 0., 0.), stds=(0.1, 0.1, 0.2, 0.2), fused=False):
    """rois [n,5] (batch index first) of ONE image -> (det_bboxes [m,5], det_labels [m]).  fused: det_candidates (one call of
    csrc/det.hip on device tensors), one readback of the count, NMS over the class-offset candidates in their order."""
    if fused:
        box, nms_box, score, _, label, count = det_candidates(rois, cls_score, bbox_pred, img_shape, scale_factor, rescale,
                                                              score_thr, means, stds)
        m = int(count.item())
        if m > ops.DET_MAX_CANDIDATES:
            raise ops.AttnShiftError(f"get_det_bboxes: {m} candidates above score_thr, NMS takes at most {ops.DET_MAX_CANDIDATES}")
        keep = _nms_in_order(nms_box[:m], iou_threshold, max_per_img)
        if max_per_img > 0:
            keep = keep[:max_per_img]
        return torch.cat((box[keep], score[keep, None]), dim=1), label[keep].long()
    scores = F.softmax(cls_score, dim=-1) if cls_score is not None else None
    if bbox_pred is not None:
        bboxes = delta2bbox(rois[:, 1:], bbox_pred, means, stds, max_shape=img_shape)
    else:
        bboxes = rois[:, 1:].clone()
        bboxes[:, 0::2] = bboxes[:, 0::2].clamp(0, img_shape[1])
        bboxes[:, 1::2] = bboxes[:, 1::2].clamp(0, img_shape[0])
    if rescale and bboxes.size(0) > 0:
        sf = bboxes.new_tensor(scale_factor)
        bboxes = (bboxes.view(bboxes.size(0), bboxes.shape[1] // 4, 4) / sf).view(bboxes.size(0), -1)
    return multiclass_nms(bboxes, scores, score_thr, iou_threshold, max_per_img)


def paste_masks(masks, boxes, img_h, img_w):
    """masks [n,1,h,w] probabilities, boxes [n,4] -> [n, img_h, img_w]: bilinear samples of every mask on the pixel
    centres of the image, zero outside its box."""
    n = masks.shape[0]
    if n == 0:
        return masks.new_zeros(0, img_h, img_w)
    if _on_device(masks):
        return ops.paste_masks(masks.float().contiguous(), None, boxes.float().contiguous(), img_h, img_w, False, 0)
    x0, y0, x1, y1 = torch.split(boxes, 1, dim=1)
    img_y = torch.arange(0, img_h, device=masks.device, dtype=torch.float32) + 0.5
    img_x = torch.arange(0, img_w, device=masks.device, dtype=torch.float32) + 0.5
    img_y = (img_y - y0) / (y1 - y0) * 2 - 1
    img_x = (img_x - x0) / (x1 - x0) * 2 - 1
    gx = img_x[:, None, :].expand(n, img_h, img_w)
    gy = img_y[:, :, None].expand(n, img_h, img_w)
    return F.grid_sample(masks.float(), torch.stack([gx, gy], dim=3), align_corners=False)[:, 0]


def _rle_counts_host(flat):
    """flat: one mask's pixels in Fortran order (bool) -> its COCO `counts` string (rleEncode + rleToString)."""
    a = flat.size
    pos = np.flatnonzero(flat[1:] != flat[:-1]) + 1                        # the value changes ...
    if a and flat[0]:
        pos = np.concatenate(([0], pos))                                   # ... pixel 0 is one when it is set
    cnts = np.diff(np.concatenate(([0], pos, [a]))).astype(np.int64)       # starts with a run of 0 (of length 0 then)
    x = cnts.copy()
    x[3:] -= cnts[1:-2]                                                    # i > 2: the difference to count i - 2
    chars = np.zeros((x.size, 7), dtype=np.uint8)                          # a 32-bit count takes at most 7 groups
    used = np.zeros((x.size, 7), dtype=bool)
    alive = np.ones(x.size, dtype=bool)
    for g in range(7):
        c = x & 0x1f
        x = x >> 5                                                         # arithmetic
        more = np.where((c & 0x10) != 0, x != -1, x != 0)
        chars[:, g] = (c | (more.astype(np.int64) << 5)) + 48
        used[:, g] = alive
        alive = alive & more
    return chars[used].tobytes()


def rle_encode(masks):
    """masks [n,H,W] (tensor or numpy array; bool or uint8, any nonzero value counts as 1) -> list of n COCO RLE dicts
    {'size': [H, W], 'counts': bytes}, what pycocotools.mask.encode returns for each mask in Fortran order: pixels column by
    column, counts alternating from a run of 0, count i > 2 stored as its difference to count i - 2, 5-bit groups low first
    with the continuation bit 0x20, + 48.  Device tensors run the kernels of csrc/rle.hip unless AS_POST_HOST=1."""
    if torch.is_tensor(masks):
        if masks.dim() != 3:
            raise ValueError(f"rle_encode: masks must be [n, H, W], got {tuple(masks.shape)}")
        H, W = int(masks.shape[1]), int(masks.shape[2])
        if _on_device(masks):
            if masks.dtype not in (torch.bool, torch.uint8):
                masks = masks != 0
            return [{"size": [H, W], "counts": c} for c in ops.rle_encode(masks.contiguous())]
        masks = masks.cpu().numpy()
    masks = np.asarray(masks)
    if masks.ndim != 3:
        raise ValueError(f"rle_encode: masks must be [n, H, W], got {masks.shape}")
    n, H, W = masks.shape
    flat = (masks != 0).transpose(0, 2, 1).reshape(n, H * W)
    return [{"size": [H, W], "counts": _rle_counts_host(flat[i])} for i in range(n)]


def encode_mask_results(mask_results):
    """mmdet/core/mask/utils.py:36-63: per-class lists of [H,W] bitmap masks -> per-class lists of RLE dicts; the
    (cls_segms, cls_mask_scores) tuple of mask scoring keeps its scores.  Entries that are RLE dicts already pass through."""
    cls_segms = mask_results[0] if isinstance(mask_results, tuple) else mask_results
    encoded = [[m if isinstance(m, dict) else rle_encode(np.asarray(m)[None])[0] for m in segms] for segms in cls_segms]
    return (encoded, mask_results[1]) if isinstance(mask_results, tuple) else encoded


def get_seg_masks(mask_pred, det_bboxes, det_labels, num_classes, ori_shape, scale_factor, rescale, mask_thr_binary=0.5,
                  class_agnostic=False, encode_rle=False):
    """mask_pred [n,K,h,w] logits -> list over classes of lists of bool numpy masks [H,W]; with encode_rle, of their COCO
    RLE dicts (encode_mask_results of the former; on the device route the masks are encoded there and never copied out)."""
    if encode_rle and mask_thr_binary < 0:
        raise ValueError("get_seg_masks: encode_rle needs binary masks (mask_thr_binary >= 0), not levels")
    cls_segms = [[] for _ in range(num_classes)]
    if mask_pred.shape[0] == 0:
        return cls_segms
    if _on_device(mask_pred):
        return _get_seg_masks_device(mask_pred, det_bboxes, det_labels, cls_segms, ori_shape, scale_factor, rescale,
                                     mask_thr_binary, class_agnostic, encode_rle)
    probs = mask_pred.sigmoid()
    boxes = det_bboxes[:, :4]
    if rescale:
        img_h, img_w = ori_shape[:2]
        boxes = boxes / boxes.new_tensor(scale_factor)
    else:
        sf = np.asarray(scale_factor, dtype=np.float64).reshape(-1)
        w_scale, h_scale = (sf[0], sf[1]) if sf.size > 1 else (sf[0], sf[0])
        img_h, img_w = int(np.round(ori_shape[0] * h_scale)), int(np.round(ori_shape[1] * w_scale))
    idx = torch.arange(probs.shape[0], device=probs.device)
    sel = probs[idx, torch.zeros_like(det_labels) if class_agnostic else det_labels][:, None]
    full = paste_masks(sel, boxes, img_h, img_w)
    full = (full >= mask_thr_binary) if mask_thr_binary >= 0 else (full * 255).to(torch.uint8)
    full = full.cpu().numpy()
    for i, lab in enumerate(det_labels.tolist()):
        cls_segms[lab].append(full[i])
    return encode_mask_results(cls_segms) if encode_rle else cls_segms


def _get_seg_masks_device(mask_pred, det_bboxes, det_labels, cls_segms, ori_shape, scale_factor, rescale, mask_thr_binary,
                          class_agnostic, encode_rle=False):
    """get_seg_masks on the device: sigmoid of the one class channel, paste and threshold in one kernel; the [n,H,W]
    byte result is the only thing copied to the host -- or, with encode_rle, stays on the device and only its run-length
    strings are."""
    boxes = det_bboxes[:, :4]
    if rescale:
        img_h, img_w = ori_shape[:2]
        boxes = boxes / boxes.new_tensor(scale_factor)
    else:
        sf = np.asarray(scale_factor, dtype=np.float64).reshape(-1)
        w_scale, h_scale = (sf[0], sf[1]) if sf.size > 1 else (sf[0], sf[0])
        img_h, img_w = int(np.round(ori_shape[0] * h_scale)), int(np.round(ori_shape[1] * w_scale))
    full = ops.paste_masks(mask_pred.float().contiguous(), None if class_agnostic else det_labels.long().contiguous(),
                           boxes.float().contiguous(), img_h, img_w, True, 1 if mask_thr_binary >= 0 else 2, mask_thr_binary)
    full = rle_encode(full) if encode_rle else full.cpu().numpy()
    for i, lab in enumerate(det_labels.tolist()):
        cls_segms[lab].append(full[i])
    return cls_segms


def bbox2result(bboxes, labels, num_classes):
    if bboxes.shape[0] == 0:
        return [np.zeros((0, 5), dtype=np.float32) for _ in range(num_classes)]
    b, l = bboxes.detach().cpu().numpy(), labels.detach().cpu().numpy()
    return [b[l == i, :] for i in range(num_classes)]
