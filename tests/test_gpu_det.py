"""The box head's detection candidates on the device (csrc/det.hip through ops.det_candidates and the dispatch of
attentionshift_amd/inference.py) against the tensor-op definition (_det_candidates_host) fed the CPU copies of the inputs, an
fp64 evaluation of the decode, and the host NMS.

Selection, order and the copied values (scores, final boxes, their correctly rounded division, the class offsets) are functions of
the inputs' bits: they must be EQUAL.  The softmax and the decode differ from ATen's by the roundings written at their tests."""
import math

import numpy as np
import pytest
import torch

import attentionshift_amd as A
from attentionshift_amd import inference as I, ops
from attentionshift_amd.assign import bbox_overlaps

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
IMG = (240, 320, 3)
SCALE4 = [1.25, 1.5, 1.75, 2.0]


def bits(t):
    return t.contiguous().view(torch.int32)


def cpu(ts):
    return [t.cpu() for t in ts]


# ------------------------------------------------------------------------------------------------
# given scores, final boxes: everything is a function of the bits
# ------------------------------------------------------------------------------------------------
def given_case(n, K):
    """scores in multiples of 1/64 (ties abound and straddle the seams of the kernels' 64-lane waves, 128-candidate workgroups
    and 1024-key tiles), duplicated rows, +-0, fp32(0.05) and its two neighbours; per-class boxes for odd K > 1, else shared"""
    gen = torch.Generator().manual_seed(1000 * n + K)
    scores = torch.randint(-8, 65, (n, K + 1), generator=gen).float() / 64
    if n >= 4:
        scores[n // 2:n // 2 + n // 4] = scores[:n // 4]
    thr = np.float32(0.05)
    special = [0.0, -0.0, float(thr), float(np.nextafter(thr, np.float32(1))), float(np.nextafter(thr, np.float32(0))), -0.0, 0.0]
    flat = scores.view(-1)
    for j, s in enumerate(range(0, flat.numel(), max(flat.numel() // 23, 1))):
        flat[s] = special[j % len(special)]
    Kb = K if K % 2 and K > 1 else 1
    xy = torch.rand(n, Kb, 2, generator=gen) * 200
    boxes = torch.cat((xy, xy + 5 + torch.rand(n, Kb, 2, generator=gen) * 90), 2).reshape(n, 4 * Kb)
    return scores, boxes


@pytest.mark.parametrize("K", [1, 5, 20, 80])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 300])
def test_given_scores_and_final_boxes_are_bit_equal_to_the_host_definition(n, K):
    scores, boxes = given_case(n, K)
    for thr, scale in ((0.05, None), (-1.0, SCALE4)):
        want = I._det_candidates_host(boxes, None, scores, None, scale, thr, None, None, apply_softmax=False)
        got = cpu(ops.det_candidates(boxes.cuda(), None, scores.cuda(), thr, None, scale, apply_softmax=False, return_prob=True))
        m = int(want[5])
        print(f"n={n} K={K} thr={thr}: {m} candidates of {n * K}")
        assert int(got[5]) == m and (m == n * K if thr < 0 else 0 < m < n * K or n * K < 4)
        assert got[3].dtype == torch.int32 and got[0].shape == (min(n * K, 65535), 4)
        assert torch.equal(got[3][:m], want[3][:m]) and torch.equal(got[4][:m], want[4][:m])        # roi, label
        assert torch.equal(bits(got[2][:m]), bits(want[2][:m]))                                      # score, the sign of zero too
        assert torch.equal(bits(got[0][:m]), bits(want[0][:m]))                                      # box
        assert torch.equal(bits(got[1][:m]), bits(want[1][:m]))                                      # nms box
        assert torch.equal(bits(got[6]), bits(scores))                                               # prob_out receives p


def test_no_candidate_and_no_rois():
    boxes = torch.rand(70, 4).cuda()
    out = ops.det_candidates(boxes, None, torch.full((70, 6), 0.01).cuda(), 0.05, apply_softmax=False)
    assert int(out[5]) == 0
    d, l = I.get_det_bboxes(torch.zeros(70, 5).cuda(), torch.zeros(70, 3).cuda(), torch.zeros(70, 8).cuda(), IMG, 1.0, False,
                            score_thr=0.5, fused=True)
    assert d.is_cuda and d.shape == (0, 5) and l.shape == (0,) and l.dtype == torch.long
    out = ops.det_candidates(torch.zeros(0, 4).cuda(), torch.zeros(0, 8).cuda(), torch.zeros(0, 3).cuda(), 0.05, IMG)
    assert int(out[5]) == 0 and out[0].shape == (0, 4)
    d, l = I.get_det_bboxes(torch.zeros(0, 5).cuda(), torch.zeros(0, 3).cuda(), torch.zeros(0, 8).cuda(), IMG, 2.0, True, fused=True)
    assert d.shape == (0, 5) and l.shape == (0,)


# ------------------------------------------------------------------------------------------------
# softmax
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,K", [(65, 1), (300, 20), (130, 80), (40, 255)])
def test_softmax_is_within_its_rounding_bound_and_selection_follows_its_bits(n, K):
    """prob_out lies within relative (2K + 10) * 2^-24 of torch.softmax on the CPU: both subtract the same exact maximum (one
    correctly rounded subtraction, the same in both), then differ by two exps at <= 2 ulp each (8 units of 2^-24), two sums of
    K + 1 positive terms in any order (K units each) and two correctly rounded divides (1 unit each).  The CPU softmax itself
    was measured against an fp64 evaluation of the fp32 logits at these shapes: at most 0.3 of the bound, no widening needed.
    Selection, order and scores must then EQUAL the host definition fed the device's own probabilities as given scores."""
    gen = torch.Generator().manual_seed(n + K)
    logits = torch.randn(n, K + 1, generator=gen) * 2
    logits[3] = logits[2]                                                   # a duplicated row: ties across rows
    if n > 10:
        logits[5, 0], logits[7, K] = float("nan"), float("inf")             # rows without a candidate
    boxes = torch.rand(n, 4, generator=gen) * 100
    got = cpu(ops.det_candidates(boxes.cuda(), None, logits.cuda(), 0.05, apply_softmax=True, return_prob=True))
    prob, ref = got[6], torch.softmax(logits, 1)
    bad = torch.isnan(ref)
    assert torch.equal(torch.isnan(prob), bad) and (int(bad.any(1).sum()) == 2 if n > 10 else not bad.any())
    rel = ((prob.double() - ref.double()).abs() / ref.double())[~bad]
    bound = (2 * K + 10) * 2.0 ** -24
    print(f"n={n} K={K}: softmax max relative difference {float(rel.max()):.3e}, bound {bound:.3e}")
    assert float(rel.max()) <= bound
    want = I._det_candidates_host(boxes, None, prob, None, None, 0.05, None, None, apply_softmax=False)
    m = int(want[5])
    assert int(got[5]) == m and 0 < m < n * K
    assert torch.equal(got[3][:m], want[3][:m]) and torch.equal(got[4][:m], want[4][:m])
    assert torch.equal(bits(got[2][:m]), bits(want[2][:m]))
    if n > 10:
        assert 5 not in got[3][:m].tolist() and 7 not in got[3][:m].tolist()


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def decode_fp64(rois, deltas, roi, label, Kb, means, stds, shape):
    """the definition in fp64 from the fp32 inputs (the clamp bound as ATen applies it to an fp32 tensor: rounded to fp32)
    -> (clipped boxes [m,4], pre-clip boxes [m,4], the bound of every box [m], the unclamped dw / dh [m,2])"""
    max_ratio = float(np.float32(abs(math.log(16 / 1000))))
    r = rois[roi.long()].double()
    cb = label.long() if Kb > 1 else torch.zeros_like(label.long())
    d = deltas.view(deltas.shape[0], Kb, 4)[roi.long(), cb].double() * torch.tensor(stds, dtype=torch.float64) \
        + torch.tensor(means, dtype=torch.float64)
    dw, dh = d[:, 2].clamp(-max_ratio, max_ratio), d[:, 3].clamp(-max_ratio, max_ratio)
    px, py, pw, ph = (r[:, 0] + r[:, 2]) * 0.5, (r[:, 1] + r[:, 3]) * 0.5, r[:, 2] - r[:, 0], r[:, 3] - r[:, 1]
    gw, gh, gx, gy = pw * dw.exp(), ph * dh.exp(), px + pw * d[:, 0], py + ph * d[:, 1]
    pre = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5], 1)
    box = pre.clone()
    box[:, 0::2] = box[:, 0::2].clamp(0, shape[1])
    box[:, 1::2] = box[:, 1::2].clamp(0, shape[0])
    bound = 4 * EPS * (torch.maximum(gx.abs(), gy.abs()) + torch.maximum(gw, gh))
    return box, pre, bound, d[:, 2:]


@pytest.mark.parametrize("Kb,scale", [(20, None), (1, None), (20, SCALE4), (1, [2.0] * 4)])
def test_decode_lies_within_the_fp32_bound_of_the_fp64_definition(Kb, scale):
    """Bound (tests/test_gpu_rpn.py): expf is good to 2 ulp and two roundings follow, so a correct fp32 decode lies within
    4 * 2^-23 * (max(|gx|, |gy|) + max(gw, gh)) of the pre-clip values; after a rescale that bound divided by the factor plus one
    spacing of the result (the divide's rounding).  The stds are powers of two, so d = delta * std + mean rounds once."""
    n, K = 150, 20
    gen = torch.Generator().manual_seed(11 + Kb)
    xy = torch.rand(n, 2, generator=gen) * 250
    rois = torch.cat((xy, xy + 8 + torch.rand(n, 2, generator=gen) * 120), 1)          # some reach past 320 x 240
    deltas = torch.randn(n, 4 * Kb, generator=gen) * 2
    deltas[::5] *= 12                                                                  # dw / dh past +-4.135: the ratio clamp
    logits = torch.randn(n, K + 1, generator=gen) * 2
    means, stds = (0.25, -0.125, 0.5, 0.0), (0.125, 0.125, 0.25, 0.25)
    got = cpu(ops.det_candidates(rois.cuda(), deltas.cuda(), logits.cuda(), 0.05, IMG, scale, means, stds))
    box, nms_box, _, roi, label, count = got
    m = int(count)
    assert m > 300
    want, pre, bound, dwh = decode_fp64(rois, deltas, roi[:m], label[:m], Kb, means, stds, IMG)
    max_ratio = float(np.float32(abs(math.log(16 / 1000))))
    clamped = int((dwh.abs() > max_ratio).any(1).sum())
    clipped = int(((pre[:, 0::2] < 0) | (pre[:, 0::2] > IMG[1]) | (pre[:, 1::2] < 0) | (pre[:, 1::2] > IMG[0])).any(1).sum())
    assert 0 < clamped < m and 0 < clipped < m                                         # both branches occurred, and their complements
    tol = bound[:, None].expand(m, 4)
    if scale is not None:
        sf = torch.tensor(scale, dtype=torch.float64)
        want, tol = want / sf, tol / sf
        tol = tol + torch.from_numpy(np.spacing(want.float().numpy())).double()        # one spacing of the result
    err = (box[:m].double() - want).abs()
    print(f"Kb={Kb} scale={scale}: m={m} clamped={clamped} clipped={clipped} worst error / bound {float((err / tol).max()):.3f}")
    assert bool((err <= tol).all())
    # the class offsets, recomputed from the device's own boxes
    off = label[:m].to(box) * (box[:m].max() + 1)
    assert torch.equal(bits(nms_box[:m]), bits(box[:m] + off[:, None]))


# ------------------------------------------------------------------------------------------------
# composition
# ------------------------------------------------------------------------------------------------
def test_fused_get_det_bboxes_is_the_host_nms_over_the_device_candidates():
    n, K = 200, 20
    gen = torch.Generator().manual_seed(21)
    xy = torch.rand(n, 2, generator=gen) * 200
    rois = torch.cat((torch.zeros(n, 1), xy, xy + 10 + torch.rand(n, 2, generator=gen) * 90), 1)
    pred = torch.randn(n, 4 * K, generator=gen) * 0.5
    logits = torch.randn(n, K + 1, generator=gen) * 2
    for max_per_img, rescale in ((100, False), (-1, True), (7, True)):
        args = (rois.cuda(), logits.cuda(), pred.cuda(), IMG, np.array(SCALE4, dtype=np.float32), rescale)
        box, nms_box, score, _, label, count = cpu(I.det_candidates(*args, 0.05))
        m = int(count)
        keep = I._nms_in_order(nms_box[:m], 0.5, max_per_img)                          # CPU tensors: the host NMS
        assert ops.nms(nms_box[:m].cuda(), 0.5).cpu().tolist() == keep.tolist()        # the keep list, exactly
        keep = keep[:max_per_img] if max_per_img > 0 else keep
        d, l = I.get_det_bboxes(*args, 0.05, 0.5, max_per_img, fused=True)
        assert d.is_cuda and l.dtype == torch.long and 0 < keep.numel() < m
        assert torch.equal(bits(d.cpu()), bits(torch.cat((box[keep], score[keep, None]), 1)))
        assert l.cpu().tolist() == label[keep].tolist()


def test_simple_test_with_fused_det_runs_the_kernel_once_per_image(monkeypatch):
    torch.manual_seed(0)
    dec = dict(in_channels=48, embed_dim=64, depth=1, num_heads=2, num_classes=5)
    head = A.build_head(dict(
        type="AttnShiftRoIHead",
        bbox_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0)),
        bbox_head=dict(type="MAEBoxHeadRec", with_reconstruct=False, cam_layer=3, **dec),
        test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=10))).cuda()
    gen = torch.Generator().manual_seed(3)
    fmap = torch.rand(2, 48, 14, 14, generator=gen).cuda()
    props = []
    for _ in range(2):
        xy = torch.rand(40, 2, generator=gen) * 120
        props.append(torch.cat((xy, xy + 10 + torch.rand(40, 2, generator=gen) * 80), 1).cuda())
    metas = [dict(img_shape=(224, 224, 3), ori_shape=(224, 224, 3), scale_factor=np.ones(4, dtype=np.float32))] * 2
    calls, seen = {"det": 0}, []
    real = ops.det_candidates

    def counted(*a, **k):
        calls["det"] += 1
        out = real(*a, **k)
        seen.append(out)
        return out
    monkeypatch.setattr(ops, "det_candidates", counted)
    with torch.no_grad():
        default = head.simple_test(fmap, props, metas, rescale=False)
        assert calls["det"] == 0                                                       # opt-in: the default route is untouched
        if isinstance(head.test_cfg, dict):
            head.test_cfg["fused_det"] = True
        else:
            head.test_cfg.fused_det = True
        fused = head.simple_test(fmap, props, metas, rescale=False)
    assert calls["det"] == 2
    for i, (res_d, res_f) in enumerate(zip(default, fused)):
        nd, nf = [r.shape[0] for r in res_d], [r.shape[0] for r in res_f]
        print(f"image {i}: detections per class, default {nd}, fused {nf}")
        assert 0 < sum(nf) <= 10
        if nd != nf:
            # a few ulp between the two softmaxes / exps can move a score across the threshold or flip one NMS decision
            box, nms_box, score, _, _, count = cpu(seen[i])
            m = int(count)
            iou = bbox_overlaps(nms_box[:m], nms_box[:m], eps=1e-12)
            near_thr = int(((score[:m] - 0.05).abs() < 1e-6).sum())
            near_iou = int(((iou - 0.5).abs() < 1e-5).sum())
            print(f"image {i}: the routes differ; scores within 1e-6 of the threshold: {near_thr}, IoUs within 1e-5 of 0.5: {near_iou}")
            assert near_thr + near_iou > 0, "the fused route differs from the default one without a near-tie to explain it"
        else:
            for bd, bf in zip(res_d, res_f):
                assert np.allclose(bd, bf, rtol=1e-5, atol=1e-4)


# ------------------------------------------------------------------------------------------------
# the candidate limit
# ------------------------------------------------------------------------------------------------
def test_more_candidates_than_nms_takes_raise():
    n, K = 3300, 20                                                                    # m = 66000 > 65535
    boxes = torch.rand(n, 4).cuda()
    out = ops.det_candidates(boxes, None, torch.full((n, K + 1), 0.5).cuda(), 0.05, apply_softmax=False)
    assert int(out[5]) == n * K and out[0].shape == (65535, 4)                         # only the count is meaningful
    rois = torch.cat((torch.zeros(n, 1), torch.rand(n, 4) * 50), 1).cuda()
    with pytest.raises(ops.AttnShiftError):                                            # softmax of equal logits: 1 / 21 each
        I.get_det_bboxes(rois, torch.zeros(n, K + 1).cuda(), None, IMG, 1.0, False, score_thr=0.01, fused=True)
