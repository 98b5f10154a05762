"""The RPN's training targets and losses on the tensor-op route (no GPU) against the fixture produced by executing the
reference's own anchor flags, MaxIoUAssigner, RandomSampler, bbox2delta and AnchorHead.loss (tools/gen_golden_rpn_loss.py),
closed-form cases of the assignment rule, and RPNHead.loss / forward_train.

The route runs the same torch ops as the reference on the same machine, so the assignment, the overlaps, the flags, the
sampled sets under the stored seed, the generator state afterwards and the dense labels / weights must be EQUAL;
bbox_targets and the losses are held to 1e-6, the project's fp32 bar for restated host code."""
import numpy as np
import pytest
import torch

from attentionshift_amd import rpn_train as RT
from attentionshift_amd.dist import parse_losses
from attentionshift_amd.rpn import AnchorGenerator, RPNHead

SHIPPED_ASSIGNER = dict(type="MaxIoUAssigner", pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3, match_low_quality=True,
                        ignore_iof_thr=-1)


def fixture_call(g, c, device="cpu"):
    """-> (anchor generator, sizes, cls, reg, gt boxes, img_metas, train_cfg) of call c of rpn_loss.npz"""
    L = len(g["strides"])
    ag = AnchorGenerator([float(s) for s in g["scales"]], [float(r) for r in g["ratios"]], [int(s) for s in g["strides"]])
    sizes = [tuple(int(v) for v in s) for s in g["sizes"]]
    cls = [torch.from_numpy(g[f"cls_{l}"]).to(device) for l in range(L)]
    reg = [torch.from_numpy(g[f"reg_{l}"]).to(device) for l in range(L)]
    B = len(g["img_shapes"])
    gts = [torch.from_numpy(g[f"c{c}_gt_{b}"]).to(device) for b in range(B)]
    metas = [dict(img_shape=tuple(int(v) for v in g["img_shapes"][b]), pad_shape=tuple(int(v) for v in g["pad_shapes"][b]))
             for b in range(B)]
    pos_thr, neg_thr, min_pos = (float(v) for v in g["assigner"])
    train_cfg = dict(assigner=dict(type="MaxIoUAssigner", pos_iou_thr=pos_thr, neg_iou_thr=neg_thr, min_pos_iou=min_pos,
                                   match_low_quality=True, ignore_iof_thr=-1),
                     sampler=dict(type="RandomSampler", num=int(g["num"]), pos_fraction=float(g["pos_fraction"]),
                                  neg_pos_ub=int(g[f"c{c}_neg_pos_ub"]), add_gt_as_proposals=False),
                     allowed_border=int(g[f"c{c}_allowed_border"]), pos_weight=float(g[f"c{c}_pos_weight"]))
    return ag, sizes, cls, reg, gts, metas, train_cfg


def run_targets(g, c, device="cpu"):
    """the three target stages on call c -> (asg, smp, pos_gt, pos_delta, generator)"""
    ag, sizes, _, _, gts, metas, cfg = fixture_call(g, c, device)
    base = torch.stack(ag.base_anchors).to(device)
    asg = RT.rpn_assign(base, sizes, ag.strides, gts, metas, cfg["assigner"], cfg["allowed_border"])
    gen = torch.Generator().manual_seed(int(g[f"c{c}_seed"]))
    s = cfg["sampler"]
    smp = RT.rpn_sample(asg, s["num"], s["pos_fraction"], s["neg_pos_ub"], gen)
    pos_gt, pos_delta = RT.rpn_targets(asg, smp)
    return asg, smp, pos_gt, pos_delta, gen


def check_targets_against_fixture(g, c, asg, smp, pos_gt, pos_delta, gen, delta_tol=1e-6):
    assigned, max_iou = asg.assigned.cpu(), asg.max_iou.cpu()
    for b in range(assigned.shape[0]):
        inside = torch.from_numpy(g[f"c{c}_inside_{b}"])
        assert torch.equal(assigned[b] != -2, inside), (c, b)
        assert torch.equal(assigned[b][inside].long(), torch.from_numpy(g[f"c{c}_gt_inds_{b}"])), (c, b)
        assert torch.equal(max_iou[b][inside], torch.from_numpy(g[f"c{c}_max_overlaps_{b}"])), (c, b)
        assert not bool(max_iou[b][~inside].any())
        where = torch.nonzero(inside).flatten()                        # the reference indexes the inside anchors
        for name, inds, n in (("pos", smp.pos_inds, smp.n_pos), ("neg", smp.neg_inds, smp.n_neg)):
            want = where[torch.from_numpy(g[f"c{c}_{name}_inds_{b}"])]
            assert n[b] == want.numel(), (c, b, name)
            assert torch.equal(inds[b, :n[b]].cpu(), want), (c, b, name)
            assert bool((inds[b, n[b]:] == -1).all())
        assert torch.equal(pos_gt[b, :smp.n_pos[b]].cpu(), assigned[b][smp.pos_inds[b, :smp.n_pos[b]].cpu()].long() - 1)
    assert torch.equal(asg.counts.cpu(), torch.stack(((assigned > 0).sum(1), (assigned == 0).sum(1)), 1).to(torch.int32))
    assert np.array_equal(gen.get_state().numpy(), g[f"c{c}_rng_after"]), c
    labels, lw, bt, bw = RT.dense_targets(asg, smp, pos_delta, float(g[f"c{c}_pos_weight"]))
    for l in range(len(labels)):
        assert torch.equal(labels[l].cpu(), torch.from_numpy(g[f"c{c}_labels_{l}"])), (c, l)
        assert torch.equal(lw[l].cpu(), torch.from_numpy(g[f"c{c}_label_weights_{l}"])), (c, l)
        assert torch.equal(bw[l].cpu(), torch.from_numpy(g[f"c{c}_bbox_weights_{l}"])), (c, l)
        err = float((bt[l].cpu() - torch.from_numpy(g[f"c{c}_bbox_targets_{l}"])).abs().max())
        assert err <= delta_tol, (c, l, err)


def fixture_head(g, c, device="cpu"):
    ag, sizes, cls, reg, gts, metas, cfg = fixture_call(g, c, device)
    head = RPNHead(8, 8, anchor_generator=dict(type="AnchorGenerator", scales=[float(s) for s in g["scales"]],
                                               ratios=[float(r) for r in g["ratios"]], strides=[int(s) for s in g["strides"]]),
                   loss_cls=dict(type="CrossEntropyLoss", use_sigmoid=True, loss_weight=1.0),
                   loss_bbox=dict(type="L1Loss", loss_weight=1.0), train_cfg=cfg).to(device)
    return head, cls, reg, gts, metas


@pytest.mark.parametrize("c", [0, 1, 2])
def test_targets_equal_the_reference(golden, c):
    g = golden("rpn_loss")
    check_targets_against_fixture(g, c, *run_targets(g, c))


def test_fixture_covers_both_sampler_branches_and_the_box_cases(golden):
    g = golden("rpn_loss")
    asg, smp, _, _, _ = run_targets(g, 0)
    k = int(int(g["num"]) * float(g["pos_fraction"]))
    counts = asg.counts.tolist()
    assert counts[0][0] > k == smp.n_pos[0] and 0 < counts[1][0] == smp.n_pos[1] <= k      # a draw, and all taken
    assert bool((asg.assigned[1] == -2).any()) and not bool((asg.assigned[0] == -2).any())  # pad_shape cuts image 1 only
    a0 = asg.assigned[0]
    assert not bool((a0 == 1).any()) and bool((a0 == 2).any())         # the duplicate pair: the later box overwrites
    t = (3 * 12 + 5) * 3 + 1                                           # a box equal to the square anchor of (x 5, y 3): IoU 1,
    assert float(asg.max_iou[0, t]) == 1.0 and int(a0[t]) >= 3         # its own (a later box's best anchor too may overwrite)
    assert not bool((a0 == 4).any())                                   # best IoU below min_pos_iou: no anchor
    assert int((a0 == 5).sum()) >= 2                                   # the tie: every anchor at the maximum


@pytest.mark.parametrize("c", [0, 1, 2])
def test_losses_equal_the_reference(golden, c):
    g = golden("rpn_loss")
    head, cls, reg, gts, metas = fixture_head(g, c)
    gen = torch.Generator().manual_seed(int(g[f"c{c}_seed"]))
    losses = head.loss(cls, reg, gts, metas, generator=gen)
    assert sorted(losses) == ["loss_rpn_bbox", "loss_rpn_cls"] and len(losses["loss_rpn_cls"]) == len(cls)
    assert float((torch.stack(losses["loss_rpn_cls"]) - torch.from_numpy(g[f"c{c}_loss_cls"])).abs().max()) <= 1e-6
    assert float((torch.stack(losses["loss_rpn_bbox"]) - torch.from_numpy(g[f"c{c}_loss_bbox"])).abs().max()) <= 1e-6
    assert np.array_equal(gen.get_state().numpy(), g[f"c{c}_rng_after"])


# ------------------------------------------------------------------------------------------------
# closed-form cases of the rule: one level 4 x 4 at stride 8, one square 16-pixel anchor per position
# ------------------------------------------------------------------------------------------------
BASE1 = torch.tensor([[[-8., -8., 8., 8.]]])
META1 = [dict(img_shape=(32, 32, 3), pad_shape=(32, 32, 3))]


def assign1(boxes, **assigner):
    cfg = dict(SHIPPED_ASSIGNER, **assigner)
    return RT.rpn_assign(BASE1, [(4, 4)], [8], [torch.tensor(boxes).reshape(-1, 4)], META1, cfg, -1)


def test_a_box_equal_to_an_anchor_is_iou_one_and_positive():
    asg = assign1([[8., 8., 24., 24.]])                                # the anchor of (x 2, y 2): t = 10
    assert float(asg.max_iou[0, 10]) == 1.0 and int(asg.assigned[0, 10]) == 1
    assert int((asg.assigned[0] > 0).sum()) == 1 and asg.counts.tolist() == [[1, int((asg.assigned[0] == 0).sum())]]


def test_low_quality_match_overwrites_a_better_box():
    # anchor 10 = [8,8,24,24]: IoU 0.935 with box 0, 0.5625 with box 1 -- and it is box 1's best anchor
    asg = assign1([[8., 8., 24., 22.4 + 0.56], [12., 12., 24., 24.]])
    iou0 = 16 * 14.96 / 256
    assert abs(float(asg.max_iou[0, 10]) - iou0) < 1e-6 and int(asg.assigned[0, 10]) == 2
    assert int(assign1([[8., 8., 24., 22.4 + 0.56], [12., 12., 24., 24.]], match_low_quality=False).assigned[0, 10]) == 1


def test_ties_between_boxes_go_to_the_lowest_index_and_between_anchors_to_all():
    asg = assign1([[8., 8., 24., 24.], [8., 8., 24., 24.]], match_low_quality=False)
    assert int(asg.assigned[0, 10]) == 1                               # argmax of equal overlaps: the first box
    asg = assign1([[8., 8., 24., 24.], [8., 8., 24., 24.]])
    assert int(asg.assigned[0, 10]) == 2                               # low-quality matches run over the boxes in order
    asg = assign1([[4., 8., 20., 24.]], min_pos_iou=0.3)               # centred between anchors 9 and 10: IoU 0.6 with each
    assert asg.assigned[0, 9:11].tolist() == [1, 1] and float(asg.max_iou[0, 9]) == float(asg.max_iou[0, 10])


def test_no_boxes_makes_every_inside_anchor_negative():
    meta = [dict(img_shape=(32, 32, 3), pad_shape=(24, 17, 3))]        # valid region 3 rows x 3 columns
    asg = RT.rpn_assign(BASE1, [(4, 4)], [8], [torch.zeros(0, 4)], meta, SHIPPED_ASSIGNER, -1)
    want = torch.full((4, 4), -2, dtype=torch.int32)
    want[:3, :3] = 0
    assert torch.equal(asg.assigned[0], want.reshape(-1)) and asg.counts.tolist() == [[0, 9]]
    assert not bool(asg.max_iou.any())
    border = RT.rpn_assign(BASE1, [(4, 4)], [8], [torch.zeros(0, 4)], META1, SHIPPED_ASSIGNER, 0)
    want = torch.full((4, 4), -2, dtype=torch.int32)
    want[1:3, 1:3] = 0                                                 # x1 >= 0 and x2 < 32: positions 1 and 2
    assert torch.equal(border.assigned[0], want.reshape(-1))


def test_sets_that_fit_are_taken_whole_without_a_draw():
    asg = assign1([[8., 8., 24., 24.]])
    gen = torch.Generator().manual_seed(5)
    before = gen.get_state().clone()
    smp = RT.rpn_sample(asg, 32, 0.5, -1, gen)
    assert torch.equal(gen.get_state(), before)
    assert smp.n_pos == [1] and smp.pos_inds[0, :1].tolist() == [10]
    assert smp.n_neg == [int(asg.counts[0, 1])]
    assert torch.equal(smp.neg_inds[0, :smp.n_neg[0]], torch.nonzero(asg.assigned[0] == 0).flatten())
    smp = RT.rpn_sample(asg, 8, 0.5, -1, gen)                          # 7 of the negatives: one draw
    assert not torch.equal(gen.get_state(), before) and smp.n_neg == [7]
    assert smp.neg_inds[0, :7].tolist() == sorted(smp.neg_inds[0, :7].tolist())
    assert RT.rpn_sample(asg, 8, 0.5, 2, gen).n_neg == [2]             # neg_pos_ub


# ------------------------------------------------------------------------------------------------
# the head
# ------------------------------------------------------------------------------------------------
def test_forward_train_returns_losses_and_proposals(golden):
    g = golden("rpn_loss")
    head, _, _, gts, metas = fixture_head(g, 0)
    feats = [torch.randn(2, 8, h, w, generator=torch.Generator().manual_seed(l)) for l, (h, w) in enumerate(g["sizes"].tolist())]
    cfg = dict(nms_pre=100, max_per_img=20, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0)
    losses, props = head.forward_train(feats, metas, gts, proposal_cfg=cfg, generator=torch.Generator().manual_seed(0))
    assert len(props) == 2 and all(p.shape[1] == 5 and 0 < p.shape[0] <= 20 and not p.requires_grad for p in props)
    only = head.forward_train(feats, metas, gts, generator=torch.Generator().manual_seed(0))
    assert isinstance(only, dict)
    total, log_vars = parse_losses(losses)
    want = sum(float(v.detach()) for v in losses["loss_rpn_cls"] + losses["loss_rpn_bbox"])
    assert abs(float(total.detach()) - want) < 1e-6 and abs(log_vars["loss"] - want) < 1e-6
    assert abs(float(parse_losses(only)[0].detach()) - want) < 1e-6            # the same seed: the same samples


def test_gradients_reach_the_head_and_only_sampled_logits(golden):
    g = golden("rpn_loss")
    head, _, _, gts, metas = fixture_head(g, 0)
    feats = [torch.randn(2, 8, h, w, generator=torch.Generator().manual_seed(l)) for l, (h, w) in enumerate(g["sizes"].tolist())]
    with torch.enable_grad():                                          # (another test may have switched autograd off)
        cls, reg = head(feats)
        for t in cls + reg:
            t.retain_grad()
        losses = head.loss(cls, reg, gts, metas, generator=torch.Generator().manual_seed(int(g["c0_seed"])))
        parse_losses(losses)[0].backward()
    for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
        assert m.weight.grad is not None and float(m.weight.grad.abs().max()) > 0 and float(m.bias.grad.abs().max()) > 0
    asg, smp, _, _, _ = run_targets(g, 0)
    grad = torch.cat([c.grad.permute(0, 2, 3, 1).reshape(2, -1) for c in cls], 1)
    dgrad = torch.cat([r.grad.permute(0, 2, 3, 1).reshape(2, -1, 4) for r in reg], 1)
    for b in range(2):
        sampled = torch.zeros(asg.T, dtype=torch.bool)
        sampled[smp.pos_inds[b, :smp.n_pos[b]]] = True
        pos = sampled.clone()
        sampled[smp.neg_inds[b, :smp.n_neg[b]]] = True
        assert bool((grad[b][sampled] != 0).all()) and not bool(grad[b][~sampled].any())
        assert bool((dgrad[b][pos] != 0).all()) and not bool(dgrad[b][~pos].any())


def test_an_image_without_inside_anchors_gives_none(golden):
    g = golden("rpn_loss")
    head, cls, reg, gts, metas = fixture_head(g, 0)
    metas = [metas[0], dict(img_shape=(60, 90, 3), pad_shape=(0, 0, 3))]
    assert head.loss(cls, reg, gts, metas) is None
    head.train_cfg = dict(head.train_cfg, allowed_border=0)
    tiny = [metas[0], dict(img_shape=(20, 20, 3), pad_shape=(64, 96, 3))]     # no anchor fits into 20 x 20
    assert head.loss(cls, reg, gts, tiny) is None
    asg = RT.rpn_assign(torch.stack(head.anchor_generator.base_anchors), [c.shape[2:] for c in cls], head.anchor_generator.strides,
                        gts, tiny, head.train_cfg["assigner"], 0)
    assert bool((asg.assigned[1] == -2).all()) and bool((asg.assigned[0] != -2).any())


def test_unsupported_settings_raise_in_loss_not_in_the_constructor(golden):
    g = golden("rpn_loss")
    head, cls, reg, gts, metas = fixture_head(g, 0)
    cfg = head.train_cfg

    def with_cfg(**kw):
        head.train_cfg = dict(cfg, **kw)
        return head

    with pytest.raises(ValueError, match="tuple"):
        with_cfg(assigner=dict(cfg["assigner"], neg_iou_thr=(0.1, 0.3))).loss(cls, reg, gts, metas)
    with pytest.raises(ValueError, match="gt_max_assign_all"):
        with_cfg(assigner=dict(cfg["assigner"], gt_max_assign_all=False)).loss(cls, reg, gts, metas)
    with pytest.raises(ValueError, match="ignore"):
        with_cfg(assigner=dict(cfg["assigner"], ignore_iof_thr=0.5)).loss(cls, reg, gts, metas, gt_bboxes_ignore=[gts[0][:1], None])
    with_cfg(assigner=dict(cfg["assigner"], ignore_iof_thr=0.5)).loss(cls, reg, gts, metas, gt_bboxes_ignore=[gts[0][:0], None])
    with pytest.raises(ValueError, match="RandomSampler"):
        with_cfg(sampler=dict(cfg["sampler"], add_gt_as_proposals=True)).loss(cls, reg, gts, metas)
    head.train_cfg = None
    with pytest.raises(ValueError, match="train_cfg"):
        head.loss(cls, reg, gts, metas)
    kw = dict(anchor_generator=dict(type="AnchorGenerator", scales=[4.0], ratios=[0.5, 1.0, 2.0], strides=[8, 16, 32]), train_cfg=cfg)
    for bad, what in ((dict(loss_bbox=dict(type="SmoothL1Loss")), "L1Loss"), (dict(loss_cls=dict(type="FocalLoss", use_sigmoid=True)),
                                                                             "CrossEntropyLoss"),
                      (dict(reg_decoded_bbox=True), "reg_decoded_bbox")):
        other = RPNHead(8, 8, **kw, **bad)                             # the constructor takes them
        with pytest.raises(ValueError, match=what):
            other.loss(cls, reg, gts, metas)
