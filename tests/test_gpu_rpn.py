"""RPN proposals on the device (csrc/rpn.hip through ops.rpn_candidates and the dispatch of attentionshift_amd/inference.py)
against the tensor-op route of the same functions fed the CPU copies of the inputs, an fp64 evaluation of the decode, and the
fixture of the reference's own RPNHead._get_bboxes (tests/golden/rpn.npz).

Selection and order are functions of the logits' bits: they must be EQUAL.  The decode differs from the host's only in exp:
expf is good to 2 ulp and two roundings follow (pw * e, g +- half of it), so two correct fp32 implementations lie within about
4 spacings of the largest intermediate of each other: 4 * 2^-23 * (max(|gx|, |gy|) + max(gw, gh)) of the box's pre-clip values."""
import math
import os

import numpy as np
import pytest
import torch

import attentionshift_amd as A
from attentionshift_amd import inference as I, ops
from attentionshift_amd.rpn import AnchorGenerator
from test_rpn import SHIPPED_RPN_HEAD, check_against_fixture, fixture_inputs

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
AG1 = AnchorGenerator([4.0], [0.5, 1.0, 2.0], [8])


def dev(ts):
    return [t.cuda() for t in ts]


# ------------------------------------------------------------------------------------------------
# selection
# ------------------------------------------------------------------------------------------------
_LEVEL = {}


def one_level(h, w, kind):
    """-> (cls [2,3,h,w], reg) of one level; B = 2.  kind: continuous | ties (1/8 steps) | special (+-0, +-inf, NaN at the seams
    of the kernel's 1024-candidate chunks and 64-lane waves) | coarse (four values; at 64 x 96 the cut falls among 11 000 keys
    that share their first 11 bits, more than the kernel sorts in LDS: its full radix select and ordered collection run)"""
    key = (h, w, kind)
    if key not in _LEVEL:
        gen = torch.Generator().manual_seed(h * 1000 + w)
        cls = torch.randn(2, 3, h, w, generator=gen) * 2
        if kind == "coarse":
            u = torch.rand(2, 3, h, w, generator=gen)
            cls = torch.full_like(u, -1.0)
            for p, v in ((0.63, 2.0), (0.33, 2.25), (0.03, 3.0)):            # 3 %, 30 %, 30 %, the rest
                cls[u < p] = v
        elif kind != "continuous":
            cls = torch.round(cls * 8) / 8
        if kind == "special":
            n = 3 * h * w
            flat = cls.permute(0, 2, 3, 1).reshape(2, n)                    # candidate order (a copy)
            vals = [float("nan"), 0.0, -0.0, float("inf"), -float("inf"), 0.0, -0.0, float("inf")]
            seams = [s for s in (0, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 4095, 4096, n - 2, n - 1) if 0 <= s < n]
            for j, s in enumerate(seams):
                flat[0, s] = vals[j % len(vals)]
                flat[1, s] = vals[(j + 3) % len(vals)]
            cls = flat.reshape(2, h, w, 3).permute(0, 3, 1, 2).contiguous()
        reg = torch.randn(2, 12, h, w, generator=gen) * 0.3
        _LEVEL[key] = (cls, reg)
    return _LEVEL[key]


_HOST = {}


def host_candidates(h, w, kind, nms_pre):
    key = (h, w, kind, nms_pre)
    if key not in _HOST:
        cls, reg = one_level(h, w, kind)
        _HOST[key] = I.rpn_candidates([cls], [reg], torch.stack(AG1.base_anchors), AG1.strides, [(8 * h, 8 * w, 3)] * 2, nms_pre)
    return _HOST[key]


@pytest.mark.parametrize("kind", ["continuous", "ties", "special", "coarse"])
@pytest.mark.parametrize("h,w,nms_pre", [(5, 7, 104), (5, 7, 105), (5, 7, 106), (64, 96, 1000), (64, 96, 2000)])
def test_selection_and_order_equal_the_host_route(h, w, nms_pre, kind):
    cls, reg = one_level(h, w, kind)
    want = host_candidates(h, w, kind, nms_pre)
    got = I.rpn_candidates([cls.cuda()], [reg.cuda()], torch.stack(AG1.base_anchors), AG1.strides, [(8 * h, 8 * w, 3)] * 2, nms_pre)
    C = min(nms_pre, 3 * h * w)
    assert got[2].is_cuda and got[3].dtype == torch.int32 and tuple(got[3].shape) == (2, C)
    assert got[5].tolist() == [C, C] == want[5].tolist()
    if kind in ("ties", "coarse") and h == 64:
        lg = cls[0].permute(1, 2, 0).reshape(-1).sort(descending=True)[0]
        assert lg[C - 1] == lg[C]                                            # a tie straddles the cut
    assert torch.equal(got[3].cpu(), want[3])
    assert torch.equal(got[4].cpu(), want[4])
    nan = torch.isnan(want[2])
    assert torch.equal(torch.isnan(got[2].cpu()), nan) and (int(nan.sum()) >= 2 if kind == "special" else not nan.any())
    assert torch.allclose(got[2].cpu()[~nan], want[2][~nan], rtol=0, atol=1e-6)


# ------------------------------------------------------------------------------------------------
# decode
# ------------------------------------------------------------------------------------------------
def five_levels(seed, shape=(128, 192), B=2, dscale=0.5):
    gen = torch.Generator().manual_seed(seed)
    ag = AnchorGenerator([8.0], [0.5, 1.0, 2.0], [4, 8, 16, 32, 64])
    sizes = [(shape[0] // s, shape[1] // s) for s in (4, 8, 16, 32, 64)]
    cls = [torch.randn(B, 3, h, w, generator=gen) * 2 for h, w in sizes]
    reg = [torch.randn(B, 12, h, w, generator=gen) * dscale for h, w in sizes]
    return ag, cls, reg


def decode_fp64(ag, reg, level, index, b, shape, means, stds):
    """the definition in fp64 from the fp32 inputs (the clamp bound as ATen applies it to an fp32 tensor: rounded to fp32)
    -> (clipped boxes [m,4], the bound of every box [m])"""
    max_ratio = float(np.float32(abs(math.log(16 / 1000))))
    out, bound = [], []
    for l, i in zip(level.tolist(), index.tolist()):
        W = reg[l].shape[3]
        a, p = i % 3, i // 3
        y, x = p // W, p % W
        sx, sy = ag.strides[l]
        base = ag.base_anchors[l][a].double() + torch.tensor([x * sx, y * sy, x * sx, y * sy], dtype=torch.float64)
        d = reg[l][b, 4 * a:4 * a + 4, y, x].double() * torch.tensor(stds, dtype=torch.float64) + torch.tensor(means, dtype=torch.float64)
        dw, dh = d[2].clamp(-max_ratio, max_ratio), d[3].clamp(-max_ratio, max_ratio)
        px, py, pw, ph = (base[0] + base[2]) * 0.5, (base[1] + base[3]) * 0.5, base[2] - base[0], base[3] - base[1]
        gw, gh, gx, gy = pw * dw.exp(), ph * dh.exp(), px + pw * d[0], py + ph * d[1]
        box = torch.stack([gx - gw * 0.5, gy - gh * 0.5, gx + gw * 0.5, gy + gh * 0.5])
        box[0::2] = box[0::2].clamp(0, shape[1])
        box[1::2] = box[1::2].clamp(0, shape[0])
        out.append(box)
        bound.append(4 * EPS * (max(abs(float(gx)), abs(float(gy))) + max(float(gw), float(gh))))
    return torch.stack(out), torch.tensor(bound, dtype=torch.float64)


def test_decode_lies_within_the_fp32_bound_of_the_fp64_definition():
    ag, cls, reg = five_levels(5, dscale=1.5)                                # dw / dh beyond +-4.135 occur: the ratio clamp
    shapes = [(128, 192, 3), (120, 180, 3)]
    means, stds = (0.05, -0.05, 0.1, 0.0), (1.0, 1.0, 2.0, 2.0)
    args = (torch.stack(ag.base_anchors), ag.strides, shapes, 300)
    box, _, score, level, index, count = (t.cpu() for t in I.rpn_candidates(dev(cls), dev(reg), *args, means=means, stds=stds))
    host = I.rpn_candidates(cls, reg, *args, means=means, stds=stds)
    assert torch.equal(level, host[3]) and torch.equal(index, host[4]) and count.tolist() == host[5].tolist()
    assert torch.allclose(score, host[2], rtol=0, atol=1e-6)
    clamped = 0
    for b in range(2):
        want, bound = decode_fp64(ag, reg, level[b], index[b], b, shapes[b], means, stds)
        err = (box[b].double() - want).abs().max(1)[0]
        print(f"image {b}: worst error / bound = {float((err / bound).max()):.3f}, largest bound {float(bound.max()):.2e}")
        assert bool((err <= bound).all())
        H, W = shapes[b][:2]
        for c, edge in ((0, 0.0), (1, 0.0), (2, float(W)), (3, float(H))):   # boxes clip on every edge of either image
            assert int((box[b][:, c] == edge).sum()) > 0
        assert float(box[b][:, 2].max()) == W and float(box[b][:, 3].max()) == H
        for l, i in zip(level[b].tolist(), index[b].tolist()):
            a, p = i % 3, i // 3
            d = reg[l][b, 4 * a + 2:4 * a + 4, p // reg[l].shape[3], p % reg[l].shape[3]] * 2.0 + torch.tensor([0.1, 0.0])
            clamped += int((d.abs() > 4.1352).any())
    assert clamped > 0


# ------------------------------------------------------------------------------------------------
# NMS stage
# ------------------------------------------------------------------------------------------------
def test_nms_stage_equals_the_host_route_on_the_devices_own_candidates():
    ag, cls, reg = five_levels(7)
    shapes = [(128, 192, 3), (120, 180, 3)]
    cand = I.rpn_candidates(dev(cls), dev(reg), torch.stack(ag.base_anchors), ag.strides, shapes, 500)
    box, nms_box, score, level, index, count = cand
    C = 500 + 500 + 288 + 72 + 18
    assert count.tolist() == [C, C]
    for b in range(2):
        hb, hl = box[b].cpu(), level[b].cpu()
        assert int((hl[1:] != hl[:-1]).sum()) > 4                            # the levels interleave in the total order
        host_nms_box = hb + (hl.to(hb) * (hb.max() + 1))[:, None]
        assert torch.equal(nms_box[b].cpu(), host_nms_box)
        full = I.rpn_nms(hb, host_nms_box, score[b].cpu(), 0.7, -1)[1]
        assert 7 < full.numel() < C
        for max_per_img in (-1, 7, 1000):
            props, keep = I.rpn_nms(box[b], nms_box[b], score[b], 0.7, max_per_img)
            want = full if max_per_img <= 0 else full[:max_per_img]
            assert keep.cpu().tolist() == want.tolist()
            assert torch.equal(props.cpu(), torch.cat((hb[want], score[b].cpu()[want, None]), 1))


# ------------------------------------------------------------------------------------------------
# end to end
# ------------------------------------------------------------------------------------------------
def test_proposals_on_the_device_equal_the_reference(golden):
    """The fixture keeps every same-level pair at least 1e-3 of IoU away from the threshold.  Its boxes are a few pixels to
    a few tens of pixels wide inside a 96 x 64 image; under the decode bound above a coordinate moves by < 1e-4 px, which
    moves the IoU of such boxes by far less than 1e-3, so the kept lists must be the reference's exactly."""
    g = golden("rpn")
    ag, cls, reg, shapes = fixture_inputs(g)
    args = (dev(cls), dev(reg), torch.stack(ag.base_anchors), ag.strides, shapes, int(g["nms_pre"]))
    props = I.rpn_proposals(*args, int(g["max_per_img"]), float(g["iou_threshold"]))
    assert all(p.is_cuda for p in props) and float(g["iou_margin"]) > 1e-3
    check_against_fixture(g, props, I.rpn_candidates(*args))


def test_rpn_head_feeds_simple_test(monkeypatch):
    """simple_test_rpn on device features against the same call on the tensor-op route (AS_POST_HOST=1): the two differ in
    exp alone, so the proposals agree at the bars of the fixture test (the seeded candidates have no pair at the threshold)."""
    torch.manual_seed(0)
    rpn = A.build_head(dict(SHIPPED_RPN_HEAD, in_channels=48, feat_channels=32,
                            anchor_generator=dict(type="AnchorGenerator", scales=[4], ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32]),
                            test_cfg=dict(nms_pre=200, max_per_img=40, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)))
    for m in (rpn.rpn_cls, rpn.rpn_reg):
        torch.nn.init.normal_(m.weight, 0, 0.1)
    rpn = rpn.cuda()
    dec = dict(in_channels=48, embed_dim=64, depth=1, num_heads=2, num_classes=5)
    head = A.build_head(dict(                                                # the head of test_gpu_post.py
        type="AttnShiftRoIHead",
        bbox_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0)),
        mask_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0)),
        bbox_head=dict(type="MAEBoxHeadRec", with_reconstruct=False, cam_layer=3, **dec),
        mask_head=dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **dec),
        test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=10, mask_thr_binary=0.5))).cuda()
    gen = torch.Generator().manual_seed(3)
    feats = [torch.randn(2, 48, 224 // s, 224 // s, generator=gen).cuda() for s in (8, 16, 32)]
    metas = [dict(img_shape=(224, 224, 3), ori_shape=(224, 224, 3), scale_factor=np.ones(4, dtype=np.float32)),
             dict(img_shape=(200, 216, 3), ori_shape=(200, 216, 3), scale_factor=np.ones(4, dtype=np.float32))]
    calls = []
    real = ops.rpn_candidates
    monkeypatch.setattr(ops, "rpn_candidates", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        props = rpn.simple_test_rpn(feats, metas)
        assert len(calls) == 1
        monkeypatch.setenv("AS_POST_HOST", "1")
        host = rpn.simple_test_rpn(feats, metas)
        assert len(calls) == 1                                               # the switch keeps the kernels out
        monkeypatch.delenv("AS_POST_HOST")
        for p, h, meta in zip(props, host, metas):
            assert p.is_cuda and p.shape == h.shape and p.shape[1] == 5 and 0 < p.shape[0] <= 40
            assert torch.allclose(p[:, :4], h[:, :4], rtol=1e-6, atol=1e-5) and torch.allclose(p[:, 4], h[:, 4], rtol=0, atol=1e-6)
            assert float(p[:, 2].max()) <= meta["img_shape"][1] and float(p[:, 3].max()) <= meta["img_shape"][0]
        results = head.simple_test(feats[1], props, metas, rescale=False)
    assert len(results) == 2
    for (boxes, segms), meta in zip(results, metas):
        assert len(boxes) == 5 and len(segms) == 5 and all(b.shape[1] == 5 for b in boxes)
        assert all(len(s) == b.shape[0] for s, b in zip(segms, boxes))
        assert all(m.shape == meta["ori_shape"][:2] for s in segms for m in s)


# ------------------------------------------------------------------------------------------------
# empty and degenerate cases
# ------------------------------------------------------------------------------------------------
def test_levels_no_larger_than_nms_pre_pass_whole():
    ag, cls, reg, shapes = fixture_inputs(np.load(os.path.join(os.path.dirname(__file__), "golden", "rpn.npz")))
    args = (torch.stack(ag.base_anchors), ag.strides, shapes)
    for nms_pre in (288, 1000, -1, 0):                                       # level 0 has exactly 288 candidates
        want = I.rpn_candidates(cls, reg, *args, nms_pre)
        got = I.rpn_candidates(dev(cls), dev(reg), *args, nms_pre)
        assert tuple(got[3].shape) == (2, 288 + 72 + 18) and got[5].tolist() == [378, 378]
        assert torch.equal(got[3].cpu(), want[3]) and torch.equal(got[4].cpu(), want[4])


def test_min_bbox_size_on_the_device():
    ag, cls, reg = five_levels(11, dscale=1.0)
    shapes = [(128, 192, 3), (120, 180, 3)]
    args = (torch.stack(ag.base_anchors), ag.strides, shapes, 300)
    free = [t.cpu() for t in I.rpn_candidates(dev(cls), dev(reg), *args)]
    box, nms_box, score, level, index, count = (t.cpu() for t in I.rpn_candidates(dev(cls), dev(reg), *args, min_bbox_size=24))
    host = I.rpn_candidates(cls, reg, *args, min_bbox_size=24)
    assert count.tolist() == host[5].tolist()
    for b in range(2):
        fb = free[0][b]
        ok = ((fb[:, 2] - fb[:, 0]) >= 24) & ((fb[:, 3] - fb[:, 1]) >= 24)   # the filter of the definition on the device's boxes
        m = int(ok.sum())
        assert 0 < m < fb.shape[0] and int(count[b]) == m
        assert torch.equal(box[b, :m], fb[ok]) and torch.equal(score[b, :m], free[2][b][ok])
        assert torch.equal(level[b, :m], free[3][b][ok]) and torch.equal(index[b, :m], free[4][b][ok])
        assert torch.equal(level[b, :m], host[3][b, :m]) and torch.equal(index[b, :m], host[4][b, :m])
        M = fb[ok].max()                                                     # taken after the filter
        assert torch.equal(nms_box[b, :m], fb[ok] + (level[b, :m].float() * (M + 1))[:, None])
    props = I.rpn_proposals(dev(cls), dev(reg), *args, 50, 0.7, min_bbox_size=24)
    assert all(p.shape[1] == 5 and 0 < p.shape[0] <= 50 for p in props)
    none = I.rpn_proposals(dev(cls), dev(reg), *args, 50, 0.7, min_bbox_size=1000)
    assert all(p.is_cuda and tuple(p.shape) == (0, 5) for p in none)
    assert I.rpn_candidates(dev(cls), dev(reg), *args, min_bbox_size=1000)[5].tolist() == [0, 0]


def test_one_image_one_level_one_candidate():
    cls, reg = torch.tensor([[[[0.5]]]]), torch.tensor([0.1, -0.1, 0.2, 0.3]).view(1, 4, 1, 1)
    base = torch.tensor([[[-8.0, -6.0, 8.0, 6.0]]])
    want = I.rpn_proposals([cls], [reg], base, [16], [(32, 32, 3)], 1000, 1000, 0.7)
    got = I.rpn_proposals([cls.cuda()], [reg.cuda()], base, [16], [(32, 32, 3)], 1000, 1000, 0.7)
    assert len(got) == 1 and tuple(got[0].shape) == (1, 5)
    assert torch.allclose(got[0].cpu(), want[0], rtol=1e-6, atol=1e-5)
    assert ops.rpn_candidates([cls.cuda()[:0]], [reg.cuda()[:0]], base, [16], [], 10)[5].numel() == 0      # B = 0
