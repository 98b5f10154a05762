"""The RPN's training targets on the device (csrc/rpn_train.hip through ops.rpn_assign / rpn_sample / rpn_targets and the
dispatch of attentionshift_amd/rpn_train.py) against the tensor-op route of the same functions fed the CPU copies of the
inputs, an fp64 evaluation of bbox2delta, and the fixture of the reference's own AnchorHead.loss (tests/golden/rpn_loss.npz).

The assignment is a function of correctly rounded fp32 operations in a fixed order: `assigned`, `max_iou`, the counts and
the sampled index sets must be EQUAL.  The delta targets differ from the host's only in logf and the roundings after it:
both are correct fp32 evaluations, so the device's worst error against fp64 may be at most twice the tensor-op route's on
the same inputs.  Losses and gradients: within 1e-5 of the value / of the largest gradient magnitude, per tensor."""
import numpy as np
import pytest
import torch

from attentionshift_amd import ops, rpn_train as RT
from attentionshift_amd.dist import parse_losses
from attentionshift_amd.rpn import AnchorGenerator
from test_rpn_loss import SHIPPED_ASSIGNER, check_targets_against_fixture, fixture_head, run_targets

pytestmark = pytest.mark.gpu

# name -> (feature map sizes, strides, img_shape); one level of 105 anchors (less than two waves), one of 18 432 (72
# workgroups: the per-box maximum crosses them), the three fixture levels (level offsets)
GEOMS = {"5x7": ([(5, 7)], [8], (40, 56, 3)),
         "64x96": ([(64, 96)], [8], (512, 768, 3)),
         "levels": ([(8, 12), (4, 6), (2, 3)], [8, 16, 32], (64, 96, 3))}
_AG = {}


def generator_of(name):
    if name not in _AG:
        _AG[name] = AnchorGenerator([4.0], [0.5, 1.0, 2.0], GEOMS[name][1])
    return _AG[name]


def boxes_for(name, G, seed):
    """G boxes of one image: random ones (a third on a 4-pixel lattice: exact ties between anchors and between boxes), and
    from G >= 3 a box equal to an anchor, a zero-area box and a box wholly outside the image; at G = 65 also a duplicate pair,
    a box centred between two anchors and a box too small for min_pos_iou"""
    h, w = GEOMS[name][2][:2]
    gen = torch.Generator().manual_seed(seed)
    xy = torch.rand(G, 2, generator=gen) * torch.tensor([w - 24., h - 24.])
    wh = 12 + torch.rand(G, 2, generator=gen) * 40
    b = torch.cat((xy, torch.min(xy + wh, torch.tensor([w - 1., h - 1.]))), 1)
    b[::3] = torch.round(b[::3] / 4) * 4
    if G >= 3:
        b[0] = torch.tensor([8., 0., 40., 32.])                        # = the square anchor of level 0 at (x 3, y 2)
        b[1] = torch.tensor([20., 20., 20., 30.])                      # zero area
        b[2] = torch.tensor([w + 50., h + 50., w + 90., h + 80.])      # outside the image
    if G >= 65:
        b[10] = b[9]
        b[11] = torch.tensor([12., 8., 44., 40.])                      # between the square anchors x 3 / x 4 of row 3
        b[12] = torch.tensor([30., 20., 33., 22.])
    return b


# (geometry, boxes per image, allowed_border, match_low_quality, pad_shape cuts the valid region)
ASSIGN_CASES = [("5x7", (1, 0), -1, True, False),
                ("5x7", (3, 65), 0, True, True),
                ("64x96", (65, 3), -1, True, True),
                ("64x96", (3, 0), 0, False, False),
                ("levels", (65, 1), -1, True, True),
                ("levels", (3, 65), 0, True, False),
                ("levels", (65, 3), -1, False, True)]
_CASE = {}


def assign_case(case, device):
    """-> the assignment of a case on `device`, computed once"""
    key = (case, device)
    if key not in _CASE:
        name, Gs, border, mlq, cut = case
        sizes, strides, img = GEOMS[name]
        ag = generator_of(name)
        pad = (img[0] - 9, img[1] - 17, 3) if cut else img
        metas = [dict(img_shape=img, pad_shape=img), dict(img_shape=(img[0] - 4, img[1] - 6, 3), pad_shape=pad)]
        gts = [boxes_for(name, G, 10 * b + G).to(device) for b, G in enumerate(Gs)]
        _CASE[key] = RT.rpn_assign(torch.stack(ag.base_anchors).to(device), sizes, ag.strides, gts, metas,
                                   dict(SHIPPED_ASSIGNER, match_low_quality=mlq), border)
    return _CASE[key]


@pytest.mark.parametrize("case", ASSIGN_CASES, ids=lambda c: f"{c[0]}-G{c[1][0]}_{c[1][1]}-border{c[2]}-{'lq' if c[3] else 'nolq'}")
def test_assignment_is_equal_on_every_anchor(case):
    host, dev = assign_case(case, "cpu"), assign_case(case, "cuda")
    assert dev.device_route and not host.device_route
    assert torch.equal(dev.assigned.cpu(), host.assigned)
    assert torch.equal(dev.max_iou.cpu(), host.max_iou)
    assert torch.equal(dev.counts.cpu(), host.counts)
    assert int((host.assigned >= 0).sum()) > 0                          # the case is not empty
    if case[4]:
        assert bool((host.assigned[1] == -2).any())
    if max(case[1]) >= 3:
        assert float(host.max_iou.max()) == 1.0                        # the box equal to an anchor


def test_host_route_can_be_forced_on_device_tensors(monkeypatch):
    monkeypatch.setenv("AS_POST_HOST", "1")
    case = ASSIGN_CASES[1]
    name, Gs, border, mlq, _ = case
    sizes, strides, img = GEOMS[name]
    ag = generator_of(name)
    metas = [dict(img_shape=img, pad_shape=img)]
    asg = RT.rpn_assign(torch.stack(ag.base_anchors).cuda(), sizes, ag.strides, [boxes_for(name, 3, 3).cuda()], metas,
                        SHIPPED_ASSIGNER, border)
    assert not asg.device_route and asg.assigned.is_cuda
    monkeypatch.delenv("AS_POST_HOST")
    dev = RT.rpn_assign(torch.stack(ag.base_anchors).cuda(), sizes, ag.strides, [boxes_for(name, 3, 3).cuda()], metas,
                        SHIPPED_ASSIGNER, border)
    assert dev.device_route and torch.equal(dev.assigned, asg.assigned) and torch.equal(dev.max_iou, asg.max_iou)


# ------------------------------------------------------------------------------------------------
# sampling and targets
# ------------------------------------------------------------------------------------------------
SAMPLE_CASES = [(ASSIGN_CASES[4], 16, "draws"),                         # num 16: draws on both sets of image 0
                (ASSIGN_CASES[2], 256, "neg-draw"),                     # the shipped num on the 64 x 96 level: 106 positives, all taken
                (ASSIGN_CASES[0], 256, "all")]                          # 105 anchors: everything fits and is taken
_SAMPLE = {}


def sample_case(case, num, device):
    key = (case, num, device)
    if key not in _SAMPLE:
        asg = assign_case(case, device)
        gen = torch.Generator().manual_seed(77)
        smp = RT.rpn_sample(asg, num, 0.5, -1, gen)
        _SAMPLE[key] = (asg, smp, RT.rpn_targets(asg, smp, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2)), gen.get_state())
    return _SAMPLE[key]


@pytest.mark.parametrize("case,num,kind", SAMPLE_CASES, ids=["levels-16", "64x96-256", "5x7-all"])
def test_sampling_is_equal_under_the_same_seed(case, num, kind):
    hasg, hs, (hgt, _), hstate = sample_case(case, num, "cpu")
    _, ds, (dgt, _), dstate = sample_case(case, num, "cuda")
    assert ds.n_pos == hs.n_pos and ds.n_neg == hs.n_neg
    assert torch.equal(ds.pos_inds.cpu(), hs.pos_inds) and torch.equal(ds.neg_inds.cpu(), hs.neg_inds)
    assert torch.equal(dstate, hstate)
    assert torch.equal(dgt.cpu(), hgt)                                  # the positives' boxes
    counts = hasg.counts.tolist()
    if kind == "draws":
        assert counts[0][0] > num // 2 == hs.n_pos[0] and counts[0][1] > num // 2 == hs.n_neg[0]
        assert not torch.equal(hstate, torch.Generator().manual_seed(77).get_state())
    elif kind == "neg-draw":
        assert 64 < counts[0][0] == hs.n_pos[0] <= num // 2 and counts[0][1] > hs.n_neg[0] == num - hs.n_pos[0]
        assert not torch.equal(hstate, torch.Generator().manual_seed(77).get_state())
    else:
        assert hs.n_pos == [c[0] for c in counts] and hs.n_neg == [c[1] for c in counts]
        assert torch.equal(hstate, torch.Generator().manual_seed(77).get_state())
        for b in range(2):
            assert torch.equal(hs.neg_inds[b, :hs.n_neg[b]], torch.nonzero(hasg.assigned[b] == 0).flatten())


def delta_fp64(asg, smp, stds):
    """bbox2delta of the sampled positives in fp64 from the fp32 anchors and boxes -> [B, num, 4] (zeros past the count)"""
    out = torch.zeros(len(smp.n_pos), smp.num, 4, dtype=torch.float64)
    for b, n in enumerate(smp.n_pos):
        t = smp.pos_inds[b, :n]
        a, g = asg.anchors[t].double(), asg.gt_bboxes[b][asg.assigned[b, t].long() - 1].double()
        pw, ph, gw, gh = a[:, 2] - a[:, 0], a[:, 3] - a[:, 1], g[:, 2] - g[:, 0], g[:, 3] - g[:, 1]
        d = torch.stack((((g[:, 0] + g[:, 2]) * 0.5 - (a[:, 0] + a[:, 2]) * 0.5) / pw,
                         ((g[:, 1] + g[:, 3]) * 0.5 - (a[:, 1] + a[:, 3]) * 0.5) / ph, torch.log(gw / pw), torch.log(gh / ph)), 1)
        out[b, :n] = d / torch.tensor(stds, dtype=torch.float64)
    return out


@pytest.mark.parametrize("case,num", [(ASSIGN_CASES[2], 256), (ASSIGN_CASES[4], 16)], ids=["64x96-256", "levels-16"])
def test_delta_targets_are_as_close_to_fp64_as_the_host_route(case, num):
    hasg, hs, (_, hdelta), _ = sample_case(case, num, "cpu")
    _, _, (_, ddelta), _ = sample_case(case, num, "cuda")
    want = delta_fp64(hasg, hs, (0.1, 0.1, 0.2, 0.2))
    finite = torch.isfinite(want)                                      # (a zero-area box's log is -inf on every route)
    assert torch.equal(torch.isfinite(ddelta.cpu()), finite) and torch.equal(torch.isfinite(hdelta), finite)
    assert torch.equal(ddelta.cpu()[~finite], hdelta[~finite])
    err_host = float((hdelta.double() - want)[finite].abs().max())
    err_dev = float((ddelta.cpu().double() - want)[finite].abs().max())
    print(f"bbox2delta worst |error| against fp64: tensor-op route {err_host:.3e}, device {err_dev:.3e} ({int(finite.sum())} values)")
    assert err_host > 0 and err_dev <= 2 * err_host, (err_dev, err_host)
    for b, n in enumerate(hs.n_pos):
        assert not bool(ddelta[b, n:].any())


# ------------------------------------------------------------------------------------------------
# the head
# ------------------------------------------------------------------------------------------------
def test_losses_and_gradients_match_the_cpu_route(golden):
    g = golden("rpn_loss")
    results = {}
    for device in ("cpu", "cuda"):
        head, _, _, gts, metas = fixture_head(g, 0, "cpu")
        torch.manual_seed(3)
        for m in (head.rpn_conv, head.rpn_cls, head.rpn_reg):
            torch.nn.init.normal_(m.weight, 0, 0.1)
        head = head.to(device)
        feats = [torch.randn(2, 8, h, w, generator=torch.Generator().manual_seed(l)).to(device)
                 for l, (h, w) in enumerate(g["sizes"].tolist())]
        with torch.enable_grad():                                      # (another test may have switched autograd off)
            losses = head.forward_train(feats, metas, [t.to(device) for t in gts], generator=torch.Generator().manual_seed(9))
            parse_losses(losses)[0].backward()
        results[device] = ({k: torch.stack(v).detach().cpu() for k, v in losses.items()},
                           {k: p.grad.detach().cpu() for k, p in head.named_parameters()})
    (hl, hg), (dl, dg) = results["cpu"], results["cuda"]
    for k in hl:
        assert float(hl[k].abs().max()) > 0
        assert bool(((dl[k] - hl[k]).abs() <= 1e-5 * hl[k].abs()).all()), (k, dl[k], hl[k])
    for k in hg:
        assert float(hg[k].abs().max()) > 0
        assert float((dg[k] - hg[k]).abs().max()) <= 1e-5 * float(hg[k].abs().max()), k


@pytest.mark.parametrize("c", [0, 1, 2])
def test_fixture_through_the_device_route(golden, c):
    g = golden("rpn_loss")
    asg, smp, pos_gt, pos_delta, gen = run_targets(g, c, "cuda")
    assert asg.device_route
    check_targets_against_fixture(g, c, asg, smp, pos_gt, pos_delta, gen)
    head, cls, reg, gts, metas = fixture_head(g, c, "cuda")
    gen = torch.Generator().manual_seed(int(g[f"c{c}_seed"]))
    losses = head.loss(cls, reg, gts, metas, generator=gen)
    assert float((torch.stack(losses["loss_rpn_cls"]).cpu() - torch.from_numpy(g[f"c{c}_loss_cls"])).abs().max()) <= 1e-6
    assert float((torch.stack(losses["loss_rpn_bbox"]).cpu() - torch.from_numpy(g[f"c{c}_loss_bbox"])).abs().max()) <= 1e-6
    assert np.array_equal(gen.get_state().numpy(), g[f"c{c}_rng_after"])


def test_loss_reads_back_once():
    """the one host sync of RPNHead.loss on the device route is the [B,2] counts"""
    g = np.load(__file__.replace("test_gpu_rpn_train.py", "golden/rpn_loss.npz"))
    head, cls, reg, gts, metas = fixture_head(g, 0, "cuda")
    head.loss(cls, reg, gts, metas, generator=torch.Generator().manual_seed(0))      # warm the caches of constants
    torch.cuda.synchronize()
    import warnings
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        torch.cuda.set_sync_debug_mode("warn")
        try:
            head.loss(cls, reg, gts, metas, generator=torch.Generator().manual_seed(0))
        finally:
            torch.cuda.set_sync_debug_mode("default")
    syncs = [f"{w.filename}:{w.lineno}" for w in seen if "called a synchronizing" in str(w.message)]
    assert len(syncs) == 1, syncs


# ------------------------------------------------------------------------------------------------
# determinism
# ------------------------------------------------------------------------------------------------
def test_two_calls_are_bitwise_equal_with_a_dirty_workspace():
    case = ASSIGN_CASES[2]
    asg = assign_case(case, "cuda")
    _, smp, (pos_gt, pos_delta), _ = sample_case(case, 256, "cuda")
    ws = torch.full_like(asg.workspace, 0xFF)
    pos_thr, neg_thr, min_pos = (SHIPPED_ASSIGNER[k] for k in ("pos_iou_thr", "neg_iou_thr", "min_pos_iou"))
    assigned, max_iou, counts, ws = ops.rpn_assign(asg.base_anchors, asg.sizes, asg.strides, asg.gt_cat, asg.gt_offsets, asg.sum_g, 65,
                                                   asg.shapes, pos_thr, neg_thr, min_pos, case[3], case[2], workspace=ws)
    assert torch.equal(assigned, asg.assigned) and torch.equal(max_iou.view(torch.int32), asg.max_iou.view(torch.int32))
    assert torch.equal(counts, asg.counts) and torch.equal(ws, asg.workspace)
    gen = torch.Generator().manual_seed(77)
    again = SimpleNamespaceLike(asg, assigned=assigned, max_iou=max_iou, counts=counts, workspace=ws)
    smp2 = RT.rpn_sample(again, 256, 0.5, -1, gen)
    gt2, delta2 = RT.rpn_targets(again, smp2, (0., 0., 0., 0.), (0.1, 0.1, 0.2, 0.2))
    assert torch.equal(smp2.inds, smp.inds) and torch.equal(gt2, pos_gt)
    assert torch.equal(delta2.view(torch.int32), pos_delta.view(torch.int32))


def SimpleNamespaceLike(ns, **changes):
    from types import SimpleNamespace
    return SimpleNamespace(**dict(vars(ns), **changes))
