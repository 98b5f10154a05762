"""Test-time NMS and mask paste on the device (csrc/detect_post.hip through ops.nms / ops.paste_masks and the dispatch of
attentionshift_amd/inference.py) against the tensor-op route of the same functions fed the CPU copies of the inputs, the
oracle's mmcv restatement, and the closed forms of tests/test_inference.py.

Where the paste tolerance 5e-5 comes from: in range |ix| <= 28; ix is one subtract, one divide and two multiply-adds on
operands of magnitude <= 2 scaled by w = 28, a few ulp(28) ~ 2e-6 each, so two correct implementations place a sample
within ~1e-5 of each other; probabilities in [0, 1] change by at most 1 per source pixel; the sigmoid adds ~1e-7; 5e-5 is
5x that bound."""
import numpy as np
import pytest
import torch

import attentionshift_amd as A
import attnshift_oracle as O
from attentionshift_amd import inference as I, ops

pytestmark = pytest.mark.gpu

BAND = 5e-5


# ------------------------------------------------------------------------------------------------
# NMS
# ------------------------------------------------------------------------------------------------
def _nms_case(n, size, seed):
    gen = torch.Generator().manual_seed(seed)
    xy = torch.rand(n, 2, generator=gen) * size
    boxes = torch.cat((xy, xy + 10 + torch.rand(n, 2, generator=gen) * 80), 1)
    scores = (torch.rand(n, generator=gen) * 64).round() / 64           # ties: the stable order decides
    if n >= 130:
        boxes[7] = boxes[3]                                             # duplicates (IoU exactly 1) ...
        boxes[n - 1] = boxes[64]                                        # ... one pair across a 64-box word boundary
    return boxes, scores


_HOST_KEEP = {}


def _host_keep(n, size, thr):
    key = (n, size, thr)
    if key not in _HOST_KEEP:
        boxes, scores = _nms_case(n, size, 100 + n)
        _HOST_KEEP[key] = (boxes, scores, I.nms(boxes, scores, thr))
    return _HOST_KEEP[key]


@pytest.mark.parametrize("thr", [0.5, 0.3])
@pytest.mark.parametrize("n,size", [(1, 150), (63, 150), (64, 150), (65, 150), (130, 60), (1000, 150), (4200, 150)])
def test_nms_equals_the_host_route(n, size, thr):
    boxes, scores, want = _host_keep(n, size, thr)
    got = I.nms(boxes.cuda(), scores.cuda(), thr)
    assert got.is_cuda and got.dtype == torch.long
    print(f"n={n} thr={thr}: host keeps {want.numel()}, device keeps {got.numel()}")
    assert got.cpu().tolist() == want.tolist()
    if n <= 1000:
        assert got.cpu().tolist() == O.nms_mmcv(boxes.numpy(), scores.numpy(), thr).tolist()
    assert n == 1 or 0 < want.numel() < n                               # the case suppresses something and keeps something


def test_nms_of_nothing():
    keep = I.nms(torch.zeros(0, 4).cuda(), torch.zeros(0).cuda(), 0.5)
    assert keep.numel() == 0 and keep.dtype == torch.long and keep.is_cuda
    assert ops.nms(torch.zeros(0, 4).cuda(), 0.5).numel() == 0


@pytest.mark.parametrize("n,size", [(130, 60), (1000, 150)])
def test_nms_max_keep_is_the_prefix_of_the_full_result(n, size):
    boxes, scores, want = _host_keep(n, size, 0.5)
    order = scores.argsort(descending=True, stable=True)
    sorted_boxes = boxes[order].contiguous().cuda()
    full = ops.nms(sorted_boxes, 0.5)
    assert order[full.cpu()].tolist() == want.tolist()
    for max_keep in (1, 7, 100):
        got = ops.nms(sorted_boxes, 0.5, max_keep)
        assert got.tolist() == full[:max_keep].tolist(), max_keep
        assert I.nms(boxes.cuda(), scores.cuda(), 0.5, max_keep).cpu().tolist() == want[:max_keep].tolist(), max_keep


def test_multiclass_nms_on_device_matches_the_oracle():
    gen = torch.Generator().manual_seed(1)                              # the inputs of tests/test_oracle_roi_nms.py
    n, K = 120, 5
    xy = torch.rand(n, 2, generator=gen) * 200
    shared = torch.cat((xy, xy + 10 + torch.rand(n, 2, generator=gen) * 90), 1)
    scores = torch.softmax(torch.randn(n, K + 1, generator=gen) * 2, 1)
    per_class = (shared[:, None, :] + torch.randn(n, K, 4, generator=gen) * 3).reshape(n, 4 * K)
    for boxes in (shared, per_class):
        for max_num in (-1, 100, 7):
            d, l = I.multiclass_nms(boxes.cuda(), scores.cuda(), 0.05, 0.5, max_num)
            dr, lr = O.multiclass_nms_mmdet(boxes.numpy(), scores.numpy(), 0.05, 0.5, max_num)
            assert d.is_cuda and l.cpu().tolist() == lr.tolist(), max_num
            assert np.allclose(d.cpu().numpy(), dr, rtol=1e-6, atol=1e-5), max_num


# ------------------------------------------------------------------------------------------------
# paste: closed forms (tests/test_inference.py::test_paste_masks_and_seg_masks on device tensors)
# ------------------------------------------------------------------------------------------------
def test_paste_closed_forms_on_device():
    boxes = torch.tensor([[10., 20., 30., 60.], [0., 0., 100., 80.]]).cuda()
    ones = torch.ones(2, 1, 28, 28).cuda()
    vals = I.paste_masks(ones, boxes, 80, 100)
    assert vals.is_cuda and vals.dtype == torch.float32 and vals.shape == (2, 80, 100)
    full = (vals >= 0.5).cpu()
    want0 = torch.zeros(80, 100, dtype=torch.bool)
    want0[20:60, 10:30] = True
    assert torch.equal(full[0], want0) and bool(full[1][1:-1, 1:-1].all())
    grad = torch.linspace(0, 1, 28).view(1, 1, 1, 28).expand(1, 1, 28, 28).cuda()
    ramp = I.paste_masks(grad, boxes[:1], 80, 100)[0, 40, 10:30].cpu()
    assert bool((ramp[1:] > ramp[:-1]).all())
    logits = torch.full((2, 3, 28, 28), -9.0)
    logits[0, 2] = 9.0
    logits[1, 0] = 9.0
    logits = logits.cuda()
    dets = torch.cat((boxes, torch.tensor([[0.9], [0.8]]).cuda()), 1)
    labels = torch.tensor([2, 0]).cuda()
    segm = I.get_seg_masks(logits, dets, labels, 3, (80, 100, 3), 1.0, True)
    assert [len(s) for s in segm] == [1, 0, 1] and segm[2][0].dtype == np.bool_ and segm[2][0].sum() == 40 * 20
    half = I.get_seg_masks(logits, dets, labels, 3, (40, 50, 3), (2.0, 2.0, 2.0, 2.0), True)
    assert half[2][0].shape == (40, 50) and half[2][0].sum() == 20 * 10
    same = I.get_seg_masks(logits, dets, labels, 3, (40, 50, 3), np.array([2.0, 2.0, 2.0, 2.0]), False)
    assert same[2][0].shape == (80, 100)
    empty = I.get_seg_masks(logits[:0], dets[:0], labels[:0], 3, (8, 8, 3), 1.0, True)
    assert [len(s) for s in empty] == [0, 0, 0]
    assert I.paste_masks(ones[:0], boxes[:0], 80, 100).shape == (0, 80, 100)


# ------------------------------------------------------------------------------------------------
# paste: against the host route (the same functions on the CPU copies)
# ------------------------------------------------------------------------------------------------
PASTE_BOXES = [[10, 20, 30, 60], [0, 0, 101, 83], [-15.5, -7.25, 40.3, 50.9],
               [60.2, 30.7, 130, 95], [50.3, 40.1, 50.9, 40.8], [20, 20, 20, 45]]
PASTE_LABELS = [2, 0, 1, 1, 0, 2]
H, W = 83, 101


@pytest.fixture(scope="module")
def paste_case():
    gen = torch.Generator().manual_seed(11)
    logits = torch.randn(6, 3, 28, 28, generator=gen) * 3
    boxes = torch.tensor(PASTE_BOXES, dtype=torch.float32)
    labels = torch.tensor(PASTE_LABELS)
    probs = logits.sigmoid()[torch.arange(6), labels][:, None]
    host = I.paste_masks(probs, boxes, H, W)                            # fp32 values of the host route, NaN for box 5
    host0 = I.paste_masks(logits.sigmoid()[:, :1], boxes, H, W)         # class-agnostic: channel 0
    return dict(logits=logits, boxes=boxes, labels=labels, host=host, host0=host0)


def _band_check(dev_mask, host_vals, thr, what):
    """masks equal wherever the host value is further than BAND from the threshold; the band holds <= 0.1 % of the pixels"""
    host_mask = host_vals >= thr
    inside = (host_vals - thr).abs() <= BAND
    print(f"{what}: {int(inside.sum())} of {inside.numel()} pixels within {BAND} of the threshold, "
          f"{int((dev_mask != host_mask).sum())} differ")
    assert int(inside.sum()) <= 0.001 * inside.numel(), what
    assert bool((dev_mask == host_mask)[~inside].all()), what


def _stack(segm, labels):
    it = [iter(s) for s in segm]
    return np.stack([next(it[lab]) for lab in labels])


def test_seg_masks_threshold_mode_against_the_host_route(paste_case):
    c = paste_case
    dets = torch.cat((c["boxes"], torch.ones(6, 1)), 1)
    got = I.get_seg_masks(c["logits"].cuda(), dets.cuda(), c["labels"].cuda(), 3, (H, W, 3), 1.0, True, 0.5)
    want = I.get_seg_masks(c["logits"], dets, c["labels"], 3, (H, W, 3), 1.0, True, 0.5)
    assert [len(s) for s in got] == [len(s) for s in want] == [2, 2, 2]
    dev, ref = _stack(got, PASTE_LABELS), _stack(want, PASTE_LABELS)
    assert dev.dtype == np.bool_ and dev.shape == (6, H, W)
    assert np.array_equal(ref, (c["host"] >= 0.5).numpy())
    _band_check(torch.from_numpy(dev)[:5], c["host"][:5], 0.5, "mode 1")
    assert not dev[5].any() and not ref[5].any()                        # zero width: all False on both routes
    assert dev[0].any() and dev[1].any() and dev[2].any() and dev[3].any()


def test_paste_values_against_the_host_route(paste_case):
    c = paste_case
    got = ops.paste_masks(c["logits"].cuda(), c["labels"].cuda(), c["boxes"].cuda(), H, W, True, 0).cpu()
    err = (got[:5] - c["host"][:5]).abs().max(dim=2)[0].max(dim=1)[0]
    print("mode 0 max |delta| per detection:", err.tolist())
    assert bool(torch.isfinite(c["host"][:5]).all()) and float(err.max()) <= BAND
    assert bool((got[5] == 0).all())                                    # defined as 0 where the host route has NaN
    assert bool(torch.isnan(c["host"][5]).all())
    probs = c["logits"].sigmoid()[torch.arange(6), c["labels"]][:, None]
    plain = I.paste_masks(probs.cuda(), c["boxes"].cuda(), H, W).cpu()  # mode 0 without the sigmoid, K = 1
    assert float((plain[:5] - c["host"][:5]).abs().max()) <= BAND and bool((plain[5] == 0).all())


def test_seg_masks_level_mode_against_the_host_route(paste_case):
    c = paste_case
    dets = torch.cat((c["boxes"], torch.ones(6, 1)), 1)
    got = I.get_seg_masks(c["logits"].cuda(), dets.cuda(), c["labels"].cuda(), 3, (H, W, 3), 1.0, True, -1)
    want = I.get_seg_masks(c["logits"], dets, c["labels"], 3, (H, W, 3), 1.0, True, -1)
    dev, ref = _stack(got, PASTE_LABELS), _stack(want, PASTE_LABELS)
    assert dev.dtype == np.uint8 and dev.shape == (6, H, W)
    diff = np.abs(dev[:5].astype(np.int32) - ref[:5].astype(np.int32))
    print("mode 2: max level difference", int(diff.max()), "pixels differing", int((diff > 0).sum()))
    assert int(diff.max()) <= 1
    assert not dev[5].any() and int(dev[1].max()) > 200


def test_class_agnostic_paste_uses_channel_zero(paste_case):
    c = paste_case
    dets = torch.cat((c["boxes"], torch.ones(6, 1)), 1)
    got = I.get_seg_masks(c["logits"].cuda(), dets.cuda(), c["labels"].cuda(), 3, (H, W, 3), 1.0, True, 0.5, class_agnostic=True)
    dev = _stack(got, PASTE_LABELS)
    _band_check(torch.from_numpy(dev)[:5], c["host0"][:5], 0.5, "class-agnostic")
    vals = ops.paste_masks(c["logits"].cuda(), None, c["boxes"].cuda(), H, W, True, 0).cpu()
    assert float((vals[:5] - c["host0"][:5]).abs().max()) <= BAND


# ------------------------------------------------------------------------------------------------
# composition and the A/B switch
# ------------------------------------------------------------------------------------------------
def test_simple_test_is_the_same_on_both_routes(monkeypatch):
    torch.manual_seed(0)
    dec = dict(in_channels=48, embed_dim=64, depth=1, num_heads=2, num_classes=5)
    head = A.build_head(dict(
        type="AttnShiftRoIHead",
        bbox_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0)),
        mask_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0)),
        bbox_head=dict(type="MAEBoxHeadRec", with_reconstruct=False, cam_layer=3, **dec),
        mask_head=dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **dec),
        test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=10, mask_thr_binary=0.5))).cuda()
    gen = torch.Generator().manual_seed(3)
    fmap = torch.rand(1, 48, 14, 14, generator=gen).cuda()
    xy = torch.rand(40, 2, generator=gen) * 120
    props = [torch.cat((xy, xy + 10 + torch.rand(40, 2, generator=gen) * 80), 1).cuda()]
    metas = [dict(img_shape=(224, 224, 3), ori_shape=(224, 224, 3), scale_factor=np.ones(4, dtype=np.float32))]
    calls = {"nms": 0, "paste": 0}
    real_nms, real_paste = ops.nms, ops.paste_masks
    monkeypatch.setattr(ops, "nms", lambda *a, **k: (calls.__setitem__("nms", calls["nms"] + 1), real_nms(*a, **k))[1])
    monkeypatch.setattr(ops, "paste_masks", lambda *a, **k: (calls.__setitem__("paste", calls["paste"] + 1), real_paste(*a, **k))[1])
    captured = {}
    host_paste, host_seg = I.paste_masks, I.get_seg_masks

    def keep_values(masks, boxes, img_h, img_w):                        # the host route's fp32 image, for the band rule
        captured["vals"] = host_paste(masks, boxes, img_h, img_w).cpu()
        return captured["vals"]

    def keep_labels(mask_pred, det_bboxes, det_labels, *a, **k):
        captured["labels"] = det_labels.cpu().numpy()
        return host_seg(mask_pred, det_bboxes, det_labels, *a, **k)
    with torch.no_grad():
        (boxes_dev, segm_dev), = head.simple_test(fmap, props, metas, rescale=False)
        assert calls == {"nms": 1, "paste": 1}
        monkeypatch.setenv("AS_POST_HOST", "1")
        monkeypatch.setattr(I, "paste_masks", keep_values)
        monkeypatch.setattr(I, "get_seg_masks", keep_labels)
        (boxes_host, segm_host), = head.simple_test(fmap, props, metas, rescale=False)
        assert calls == {"nms": 1, "paste": 1}                          # the switch keeps the kernels out
    n = sum(b.shape[0] for b in boxes_dev)
    assert 0 < n <= 10
    for bd, bh in zip(boxes_dev, boxes_host):
        assert np.array_equal(bd, bh)
    dev = np.stack([m for s in segm_dev for m in s])
    host = np.stack([m for s in segm_host for m in s])
    assert dev.shape == host.shape == (n, 224, 224)
    # the per-class lists keep the detection order inside a class: bring the captured values into the same order
    order = torch.from_numpy(np.argsort(captured["labels"], kind="stable"))
    vals = captured["vals"][order]
    assert np.array_equal(host, (vals >= 0.5).numpy())
    _band_check(torch.from_numpy(dev), vals, 0.5, "simple_test")
