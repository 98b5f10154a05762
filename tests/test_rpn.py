"""The proposal generator on the tensor-op route (no GPU): anchors and proposals against the fixture produced by executing
the reference's own AnchorGenerator / delta2bbox / RPNHead._get_bboxes (tools/gen_golden_rpn.py), the tie rules of the
definition, the minimum-size filter, and the RPNHead module."""
import sys
import types

import numpy as np
import pytest
import torch

import attentionshift_amd as A
from attentionshift_amd import inference as I
from attentionshift_amd.bbox_loss import delta2bbox
from attentionshift_amd.rpn import AnchorGenerator, RPNHead, grid_anchors


def fixture_inputs(g, device="cpu"):
    L = len(g["strides"])
    ag = AnchorGenerator([float(s) for s in g["scales"]], [float(r) for r in g["ratios"]], [int(s) for s in g["strides"]])
    cls = [torch.from_numpy(g[f"cls_{l}"]).to(device) for l in range(L)]
    reg = [torch.from_numpy(g[f"reg_{l}"]).to(device) for l in range(L)]
    shapes = [tuple(int(v) for v in s) for s in g["img_shapes"]]
    return ag, cls, reg, shapes


def check_against_fixture(g, props, cands):
    """props: per image [m,5]; cands = rpn_candidates' result for the same inputs"""
    box, _, score, level, index, count = (t.cpu() for t in cands)
    for b, p in enumerate(props):
        p = p.cpu()
        want, kept = torch.from_numpy(g[f"dets_{b}"]), g[f"kept_{b}"]
        assert p.shape == want.shape
        # name every returned proposal by the candidate it is (bit-equal box and score among the candidates)
        m = int(count[b])
        hit = ((box[b, :m, None, :] == p[None, :, :4]).all(-1) & (score[b, :m, None] == p[None, :, 4])).float().argmax(0)
        got = np.stack((level[b, hit].numpy(), index[b, hit].numpy()), 1)
        assert np.array_equal(got, kept)
        assert torch.allclose(p[:, :4], want[:, :4], rtol=1e-6, atol=1e-5)
        assert torch.allclose(p[:, 4], want[:, 4], rtol=0, atol=1e-6)


def test_anchors_equal_the_reference_bit_for_bit(golden):
    g = golden("rpn")
    ag, cls, _, _ = fixture_inputs(g)
    grids = ag.grid_anchors([c.shape[2:] for c in cls])
    for l in range(ag.num_levels):
        assert np.array_equal(ag.base_anchors[l].numpy(), g[f"base_{l}"])
        assert np.array_equal(grids[l].numpy(), g[f"grid_{l}"])
    assert ag.num_base_anchors == [3, 3, 3] and ag.strides == [(8, 8), (16, 16), (32, 32)]


def test_proposals_equal_the_reference(golden):
    g = golden("rpn")
    ag, cls, reg, shapes = fixture_inputs(g)
    args = (cls, reg, torch.stack(ag.base_anchors), ag.strides, shapes, int(g["nms_pre"]))
    props = I.rpn_proposals(*args, int(g["max_per_img"]), float(g["iou_threshold"]))
    assert float(g["iou_margin"]) > 1e-3
    check_against_fixture(g, props, I.rpn_candidates(*args))


def definition_order(cls, nms_pre):
    """(level, index) of one image's candidates in the total order, by a plain Python sort of the definition"""
    out = []
    for l, c in enumerate(cls):
        lg = c.permute(1, 2, 0).reshape(-1).tolist()
        key = lambda i: ((0, 0.0) if lg[i] != lg[i] else (1, -lg[i]), i)     # noqa: E731  NaN first, -0.0 == 0.0
        order = sorted(range(len(lg)), key=key)
        out += [(key(i)[0], l, i) for i in (order[:nms_pre] if nms_pre > 0 else order)]
    return [(l, i) for _, l, i in sorted(out)]


def tie_inputs(seed=0, nan=True):
    gen = torch.Generator().manual_seed(seed)
    sizes = [(5, 7), (3, 4)]
    cls = [torch.round(torch.randn(1, 3, h, w, generator=gen) * 8) / 8 for h, w in sizes]
    cls[0][0, 0, 0, :4] = torch.tensor([0.0, -0.0, 0.0, -0.0])
    cls[1][0, 1, 1, :2] = torch.tensor([-0.0, 0.0])
    if nan:
        cls[1][0, 2, 2, 3] = float("nan")
    reg = [torch.randn(1, 12, h, w, generator=gen) * 0.3 for h, w in sizes]
    ag = AnchorGenerator([4.0], [0.5, 1.0, 2.0], [8, 16])
    return cls, reg, ag


@pytest.mark.parametrize("nms_pre", [20, 53, -1])
def test_ties_follow_logit_level_index_and_nan_ranks_first(nms_pre):
    cls, reg, ag = tie_inputs()
    want = definition_order([c[0] for c in cls], nms_pre)
    flat = cls[0][0].permute(1, 2, 0).reshape(-1)
    cut = flat.sort(descending=True)[0]
    if nms_pre > 0:
        assert cut[nms_pre - 1] == cut[nms_pre]                              # a tie straddles the cut of level 0
    _, _, score, level, index, count = I.rpn_candidates(cls, reg, torch.stack(ag.base_anchors), ag.strides, [(40, 56, 3)], nms_pre)
    assert int(count[0]) == len(want) == score.shape[1]
    assert list(zip(level[0].tolist(), index[0].tolist())) == want
    assert want[0] == (1, (2 * 4 + 3) * 3 + 2) and torch.isnan(score[0, 0]) and not torch.isnan(score[0, 1:]).any()


def test_min_bbox_size_drops_by_the_definition_and_m_is_taken_after_it():
    cls, reg, ag = tie_inputs(seed=1, nan=False)
    base, shape = torch.stack(ag.base_anchors), (40, 200, 3)
    reg[0][0, 2::4] -= 1.5                                                   # narrow boxes on level 0 ...
    cls[0][0, 0, 0, 0], reg[0][0, :4, 0, 0] = 50.0, torch.tensor([30.0, 0.0, 0.0, 0.0])
    free = I.rpn_candidates(cls, reg, base, ag.strides, [shape], -1)
    box, nms_box, score, level, index, count = I.rpn_candidates(cls, reg, base, ag.strides, [shape], -1, min_bbox_size=8)
    fb = free[0][0]
    ok = ((fb[:, 2] - fb[:, 0]) >= 8) & ((fb[:, 3] - fb[:, 1]) >= 8)
    m = int(ok.sum())
    assert 0 < m < fb.shape[0] and int(count[0]) == m
    assert torch.equal(box[0, :m], fb[ok]) and torch.equal(index[0, :m], free[4][0][ok]) and torch.equal(level[0, :m], free[3][0][ok])
    # the top candidate is shifted to the right edge: zero width, dropped -- and with it the largest coordinate
    assert not bool(ok[0]) and float(fb[0, 2]) == 200.0 and float(fb[ok].max()) < 200.0
    M = fb[ok].max()
    assert torch.equal(nms_box[0, :m], fb[ok] + (level[0, :m].float() * (M + 1))[:, None])
    props = I.rpn_proposals(cls, reg, base, ag.strides, [shape], -1, 1000, 0.7, min_bbox_size=8)
    assert props[0].shape[0] <= m and props[0].shape[1] == 5
    none = I.rpn_proposals(cls, reg, base, ag.strides, [shape], -1, 1000, 0.7, min_bbox_size=1000)
    assert none[0].shape == (0, 5)


def test_decode_of_the_host_route_is_delta2bbox_on_grid_anchors():
    cls, reg, ag = tie_inputs(seed=2, nan=False)
    box, _, score, level, index, _ = I.rpn_candidates(cls, reg, torch.stack(ag.base_anchors), ag.strides, [(33, 50, 3)], 30,
                                                      means=(0.1, 0., 0., 0.), stds=(1., 1., 2., 2.))
    for l in range(2):
        sel = level[0] == l
        idx = index[0][sel].long()
        anchors = grid_anchors(ag.base_anchors[l], cls[l].shape[2:], ag.strides[l])[idx]
        deltas = reg[l][0].permute(1, 2, 0).reshape(-1, 4)[idx]
        assert torch.equal(box[0][sel], delta2bbox(anchors, deltas, (0.1, 0., 0., 0.), (1., 1., 2., 2.), max_shape=(33, 50)))
        assert torch.equal(score[0][sel], 1 / (1 + torch.exp(-cls[l][0].permute(1, 2, 0).reshape(-1)[idx])))


SHIPPED_RPN_HEAD = dict(
    type="RPNHead", in_channels=256, feat_channels=256,
    anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
    bbox_coder=dict(type="DeltaXYWHBBoxCoder", target_means=[.0, .0, .0, .0], target_stds=[1.0, 1.0, 1.0, 1.0]),
    loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
    loss_bbox=dict(type="L1Loss", loss_weight=1.0))
SHIPPED_TEST_RPN = dict(nms_pre=1000, max_per_img=1000, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)


def test_rpn_head_builds_from_the_shipped_config_and_generates_proposals():
    torch.manual_seed(0)
    head = A.build_head(dict(SHIPPED_RPN_HEAD, test_cfg=SHIPPED_TEST_RPN))
    assert isinstance(head, RPNHead) and A.HEADS.get("RPNHead") is RPNHead
    assert sorted(head.state_dict()) == ["rpn_cls.bias", "rpn_cls.weight", "rpn_conv.bias", "rpn_conv.weight", "rpn_reg.bias",
                                         "rpn_reg.weight"]
    assert head.rpn_conv.weight.shape == (256, 256, 3, 3) and head.rpn_cls.weight.shape == (3, 256, 1, 1)
    assert head.rpn_reg.weight.shape == (12, 256, 1, 1) and tuple(head.base_anchors.shape) == (5, 3, 4)
    for m in (head.rpn_cls, head.rpn_reg):
        torch.nn.init.normal_(m.weight, 0, 0.05)                             # spread the untrained outputs
    gen = torch.Generator().manual_seed(1)
    feats = [torch.randn(2, 256, 64 // s, 96 // s, generator=gen) for s in (4, 8, 16, 32, 64)]
    metas = [dict(img_shape=(64, 96, 3)), dict(img_shape=(60, 90, 3))]
    with torch.no_grad():
        props = head.simple_test_rpn(feats, metas)
        cls, reg = head(feats)
        want = I.rpn_proposals(cls, reg, head.base_anchors, head.anchor_generator.strides, [m["img_shape"] for m in metas], 1000,
                               1000, 0.7)
    assert len(props) == 2 and all(p.shape[1] == 5 and 0 < p.shape[0] <= 1000 for p in props)
    for p, w, meta in zip(props, want, metas):
        assert torch.equal(p, w)
        assert (p[:, 0] >= 0).all() and (p[:, 2] <= meta["img_shape"][1]).all() and (p[:, 3] <= meta["img_shape"][0]).all()
        assert (p[1:, 4] <= p[:-1, 4]).all()


def test_register_into_mmdet_leaves_mmdets_rpn_head_alone(monkeypatch):
    class Reg:
        def __init__(self):
            self.names = []

        def register_module(self, name=None, force=False, module=None):
            self.names.append(name)

    backbones, heads = Reg(), Reg()
    for name in ("mmdet", "mmdet.models"):
        monkeypatch.setitem(sys.modules, name, types.ModuleType(name))
    builder = types.ModuleType("mmdet.models.builder")
    builder.BACKBONES, builder.HEADS = backbones, heads
    monkeypatch.setitem(sys.modules, "mmdet.models.builder", builder)
    assert "RPNHead" in A.HEADS
    A.register_into_mmdet()
    assert "AttnShiftRoIHead" in heads.names and "VisionTransformerDet" in backbones.names
    assert "RPNHead" not in heads.names
