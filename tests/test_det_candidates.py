"""The box head's detection candidates on CPU tensors (inference.det_candidates -> _det_candidates_host): followed by the host
NMS they give get_det_bboxes(fused=False) bit for bit, the labels of the reference's multiclass_nms, and the rules of the
definition -- order (score descending, flat index ascending, -0.0 == +0.0), the fp32 threshold, nothing to do."""
import numpy as np
import pytest
import torch

import attnshift_oracle as O
from attentionshift_amd import inference as I, ops

IMG = (240, 320, 3)
SCALES = {"none": None, "one": 1.5, "four": np.array([1.25, 1.5, 1.75, 2.0], dtype=np.float32)}


def oracle_inputs():
    """the inputs of test_multiclass_nms_on_device_matches_the_oracle (tests/test_oracle_roi_nms.py)"""
    gen = torch.Generator().manual_seed(1)
    n, K = 120, 5
    xy = torch.rand(n, 2, generator=gen) * 200
    shared = torch.cat((xy, xy + 10 + torch.rand(n, 2, generator=gen) * 90), 1)
    logits = torch.randn(n, K + 1, generator=gen) * 2
    scores = torch.softmax(logits, 1)
    per_class = (shared[:, None, :] + torch.randn(n, K, 4, generator=gen) * 3).reshape(n, 4 * K)
    return n, K, shared, per_class, logits, scores


def as_rois(boxes):
    return torch.cat((boxes.new_zeros(boxes.shape[0], 1), boxes), 1)


def fused_equals_default(rois, logits, pred, scale, max_per_img, stds=(0.1, 0.1, 0.2, 0.2)):
    rescale, sf = scale is not None, (scale if scale is not None else 1.0)
    d0, l0 = I.get_det_bboxes(rois, logits, pred, IMG, sf, rescale, 0.05, 0.5, max_per_img, stds=stds)
    d1, l1 = I.get_det_bboxes(rois, logits, pred, IMG, sf, rescale, 0.05, 0.5, max_per_img, stds=stds, fused=True)
    assert d0.shape == d1.shape and d0.shape[0] > 0
    assert torch.equal(d0.view(torch.int32), d1.view(torch.int32))                  # bit for bit
    assert l1.dtype == torch.long and torch.equal(l0, l1)
    return d1, l1


@pytest.mark.parametrize("max_per_img", [-1, 100, 7])
@pytest.mark.parametrize("scale", ["none", "one", "four"])
@pytest.mark.parametrize("kind", ["per_class", "agnostic", "no_pred"])
def test_candidates_then_nms_equal_the_default_route_bit_for_bit(kind, scale, max_per_img):
    n, K, shared, per_class, logits, _ = oracle_inputs()
    gen = torch.Generator().manual_seed(7)
    rois = as_rois(shared + torch.randn(n, 4, generator=gen) * 40)                  # some pass the image border
    pred = {"per_class": torch.randn(n, 4 * K, generator=gen), "agnostic": torch.randn(n, 4, generator=gen), "no_pred": None}[kind]
    if pred is not None:
        pred[::9] *= 30                                                             # dw / dh past the ratio clamp
    d, _ = fused_equals_default(rois, logits, pred, SCALES[scale], max_per_img)
    assert max_per_img < 0 or d.shape[0] <= max_per_img


@pytest.mark.parametrize("max_num", [-1, 100, 7])
@pytest.mark.parametrize("boxes", ["shared", "per_class"])
def test_final_boxes_and_given_scores_match_the_oracle(boxes, max_num):
    n, K, shared, per_class, _, scores = oracle_inputs()
    b = shared if boxes == "shared" else per_class
    box, nms_box, score, roi, label, count = I._det_candidates_host(b, None, scores, None, None, 0.05, None, None, apply_softmax=False)
    m = int(count)
    keep = I._nms_in_order(nms_box[:m], 0.5, max_num)
    keep = keep[:max_num] if max_num > 0 else keep
    d, l = I.multiclass_nms(b, scores, 0.05, 0.5, max_num)
    assert torch.equal(torch.cat((box[keep], score[keep, None]), 1), d) and torch.equal(label[keep].long(), l)
    dr, lr = O.multiclass_nms_mmdet(b.numpy(), scores.numpy(), 0.05, 0.5, max_num)
    assert label[keep].tolist() == lr.tolist()
    assert np.allclose(box[keep].numpy(), dr[:, :4], rtol=1e-6, atol=1e-5)
    # every candidate names its score and its box
    assert torch.equal(score[:m], scores[roi[:m].long(), label[:m].long()])
    assert torch.equal(box[:m], b.view(n, -1, 4)[roi[:m].long(), label[:m].long() if boxes == "per_class" else 0])


def test_order_is_score_descending_then_flat_index():
    gen = torch.Generator().manual_seed(3)
    n, K = 40, 6
    scores = torch.randint(-8, 64, (n, K + 1), generator=gen).float() / 64          # multiples of 1/64: ties abound
    scores[10:20] = scores[0:10]                                                    # duplicated rows
    scores[5, :4] = torch.tensor([0.0, -0.0, -0.0, 0.0])                            # mixed zeros stay in index order
    boxes = torch.rand(n, 4, generator=gen) * 100
    _, _, score, roi, label, count = I._det_candidates_host(boxes, None, scores, None, None, -1.0, None, None, apply_softmax=False)
    m = int(count)
    assert m == n * K
    flat = (roi[:m].long() * K + label[:m].long()).tolist()
    want = sorted(range(n * K), key=lambda f: (-float(scores[f // K, f % K]), f))    # -0.0 == 0.0 in the key
    assert flat == want
    assert torch.equal(score[:m].view(torch.int32), scores[:, :K].reshape(-1)[flat].view(torch.int32))   # the signs of zero too
    zeros = [f for f in flat if f // K == 5 and f % K < 4]
    assert zeros == [5 * K, 5 * K + 1, 5 * K + 2, 5 * K + 3]


def test_threshold_is_compared_in_fp32():
    thr = np.float32(0.05)
    above = np.nextafter(thr, np.float32(1))
    scores = torch.tensor([[float(thr), float(above), float("nan"), 0.5], [float(np.nextafter(thr, np.float32(0))), 0.049, 0.9, 0.5]])
    boxes = torch.tensor([[0., 0., 10., 10.], [5., 5., 20., 20.]])
    _, _, score, roi, label, count = I._det_candidates_host(boxes, None, scores, None, None, 0.05, None, None, apply_softmax=False)
    assert int(count) == 2                                                          # fp32(0.05) itself and the NaN are out
    assert list(zip(roi[:2].tolist(), label[:2].tolist())) == [(1, 2), (0, 1)]
    assert float(score[1]) == float(above)


def test_no_candidate_and_no_rois():
    boxes = torch.tensor([[0., 0., 10., 10.], [5., 5., 20., 20.]])
    out = I._det_candidates_host(boxes, None, torch.full((2, 4), 0.01), None, None, 0.05, None, None, apply_softmax=False)
    assert int(out[5]) == 0 and out[0].shape == (6, 4)
    for fused in (False, True):
        d, l = I.get_det_bboxes(as_rois(boxes), torch.tensor([[0., 0., 0., 9.]] * 2), torch.zeros(2, 12), IMG, 1.0, False, fused=fused)
        assert d.shape == (0, 5) and l.shape == (0,) and l.dtype == torch.long
        d, l = I.get_det_bboxes(torch.zeros(0, 5), torch.zeros(0, 4), torch.zeros(0, 12), IMG, 2.0, True, fused=fused)
        assert d.shape == (0, 5) and l.shape == (0,) and l.dtype == torch.long
    out = I.det_candidates(torch.zeros(0, 5), torch.zeros(0, 4), torch.zeros(0, 12), IMG, 2.0, True, return_prob=True)
    assert int(out[5]) == 0 and out[0].shape == (0, 4) and out[6].shape == (0, 4)


def test_prob_is_the_softmax_and_given_scores_pass_through():
    n, K, shared, _, logits, scores = oracle_inputs()
    out = I.det_candidates(as_rois(shared), logits, None, IMG, 1.0, False, return_prob=True)
    assert torch.equal(out[6], torch.softmax(logits, 1))
    out = I.det_candidates(as_rois(shared), scores, None, IMG, 1.0, False, apply_softmax=False, return_prob=True)
    assert torch.equal(out[6], scores)


def test_cpu_inputs_never_reach_the_kernels(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device route was taken for a CPU input")
    monkeypatch.setattr(ops, "det_candidates", boom)
    monkeypatch.setattr(ops, "nms", boom)
    n, K, shared, _, logits, _ = oracle_inputs()
    d, l = I.get_det_bboxes(as_rois(shared), logits, torch.zeros(n, 4 * K), IMG, 1.0, False, fused=True)
    assert d.shape[1] == 5 and 0 < d.shape[0] <= 100 and l.shape[0] == d.shape[0]
