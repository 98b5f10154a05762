"""The FPN neck and the RPN head's opt-in trunk on as_conv2d_fwd (attentionshift_amd/neck.py, rpn.py).

The per-call arithmetic has its sharp bars in test_gpu_conv.py; here the plumbing is pinned -- which level feeds which, the
nearest indices, the extra level -- by bit-equality with a chain of ops.conv2d_nhwc calls written out below, and the whole
neck is held loosely against the fp32 route on the CPU with every stored tensor rounded to bf16 where the device route stores
one: two bf16 ulps (2 * 2^-8) of the level's largest magnitude.
"""
import warnings

import pytest
import torch
import torch.nn.functional as F

import attentionshift_amd as A
from attentionshift_amd import ops

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -23
SIZES = [(36, 52), (18, 26), (9, 13), (4, 6)]
B = 2


def bf(t):
    return t.to(torch.bfloat16).float()


@pytest.fixture(scope="module")
def case():
    torch.manual_seed(5)
    neck = A.build_neck(dict(type="FPN", in_channels=[64] * 4, out_channels=32, num_outs=5))
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.bias.normal_(0, 0.1)
    gen = torch.Generator().manual_seed(6)
    ins = [torch.randn(B, 64, h, w, generator=gen) for h, w in SIZES]
    # the fp32 route on the CPU with the device route's roundings: bf16 inputs and weights, bf16 stored laterals and outputs
    ref = A.build_neck(dict(type="FPN", in_channels=[64] * 4, out_channels=32, num_outs=5, compute_dtype=torch.float32))
    ref.load_state_dict(neck.state_dict())
    with torch.no_grad():
        for m in ref.modules():
            if isinstance(m, torch.nn.Conv2d):
                m.weight.copy_(bf(m.weight))
        lat = [None] * 4
        for i in range(3, -1, -1):
            y = ref.lateral_convs[i](bf(ins[i]))
            if i < 3:
                y = y + F.interpolate(lat[i + 1], size=y.shape[2:], mode="nearest")
            lat[i] = bf(y)
        want = [bf(ref.fpn_convs[i](lat[i])) for i in range(4)]
        want.append(want[-1][:, :, ::2, ::2])
    neck = neck.cuda()
    # channels-last device inputs, as the backbone hands them over: level 0 bf16, the others fp32
    dev = [x.cuda().permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2) for x in ins]
    dev[0] = dev[0].to(torch.bfloat16)
    return neck, dev, want


def count_calls(monkeypatch):
    calls = []
    real = ops.conv2d_nhwc
    monkeypatch.setattr(ops, "conv2d_nhwc", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_outputs_are_bit_equal_to_the_chain_written_out(case, monkeypatch):
    neck, dev, _ = case
    calls = count_calls(monkeypatch)
    with torch.no_grad():
        outs = neck(dev)
    assert len(calls) == 8 and len(outs) == 5
    monkeypatch.undo()
    pk = ops.pack_conv_weight
    x = [t.permute(0, 2, 3, 1).to(torch.bfloat16) for t in dev]
    lc, fc = [m.conv for m in neck.lateral_convs], [m.conv for m in neck.fpn_convs]
    with torch.no_grad():
        l3 = ops.conv2d_nhwc(x[3], pk(lc[3].weight), lc[3].bias.float(), ksize=1)
        l2 = ops.conv2d_nhwc(x[2], pk(lc[2].weight), lc[2].bias.float(), ksize=1, add=l3)
        l1 = ops.conv2d_nhwc(x[1], pk(lc[1].weight), lc[1].bias.float(), ksize=1, add=l2)
        l0 = ops.conv2d_nhwc(x[0], pk(lc[0].weight), lc[0].bias.float(), ksize=1, add=l1)
        want = [ops.conv2d_nhwc(l, pk(c.weight), c.bias.float(), ksize=3) for l, c in zip((l0, l1, l2, l3), fc)]
    want.append(want[3][:, ::2, ::2])
    for l, (o, w) in enumerate(zip(outs, want)):
        assert o.dtype == torch.bfloat16 and o.is_cuda, l
        assert o.permute(0, 2, 3, 1).stride()[-1] == 1                      # an NCHW-shaped view of channels-last memory
        assert tuple(o.shape) == (B, 32) + tuple(w.shape[1:3]), l
        assert torch.equal(o.permute(0, 2, 3, 1), w), f"level {l}"
    assert tuple(outs[4].shape[2:]) == (2, 3)


def test_levels_lie_within_two_bf16_ulps_of_the_fp32_route(case):
    neck, dev, want = case
    with torch.no_grad():
        outs = neck(dev)
    for l, (o, w) in enumerate(zip(outs, want)):
        err = float((o.float().cpu() - w).abs().max())
        bar = 2 * 2.0 ** -8 * float(w.abs().max())
        print(f"NECK_RATIO level {l}: worst error / bar = {err / bar:.4f}")
        assert err <= bar, f"level {l}: {err:.3e} > {bar:.3e}"


def test_fp32_and_grad_routes_launch_no_conv_kernel(case, monkeypatch):
    neck, dev, want = case
    calls = count_calls(monkeypatch)
    with torch.enable_grad():
        outs = neck(dev)
    assert len(calls) == 0 and outs[0].dtype == torch.float32 and outs[0].requires_grad
    ref = A.build_neck(dict(type="FPN", in_channels=[64] * 4, out_channels=32, num_outs=5, compute_dtype=torch.float32)).cuda()
    with torch.no_grad():
        outs = ref(dev)
    assert len(calls) == 0 and outs[0].dtype == torch.float32 and len(outs) == 5


def test_channels_outside_the_contract_warn_once_and_take_the_tensor_op_route(monkeypatch):
    calls = count_calls(monkeypatch)
    neck = A.build_neck(dict(type="FPN", in_channels=[48, 48], out_channels=32, num_outs=2)).cuda()
    x = [torch.randn(1, 48, 8, 8, device="cuda"), torch.randn(1, 48, 4, 4, device="cuda")]
    with torch.no_grad():
        with pytest.warns(RuntimeWarning, match="48"):
            outs = neck(x)
        with warnings.catch_warnings():
            warnings.simplefilter("error")                               # a second call is silent
            neck(x)
    assert len(calls) == 0 and tuple(outs[1].shape) == (1, 32, 4, 4)


def test_rpn_head_on_the_necks_outputs(case, monkeypatch):
    neck, dev, _ = case
    torch.manual_seed(8)
    cfg = dict(type="RPNHead", in_channels=32, feat_channels=32,
               anchor_generator=dict(type="AnchorGenerator", scales=[4], ratios=[0.5, 1.0, 2.0], strides=[4, 8, 16, 32, 64]),
               test_cfg=dict(nms_pre=200, max_per_img=40, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0))
    rpn = A.build_head(dict(cfg, compute_dtype=torch.bfloat16))
    plain = A.build_head(cfg)
    with torch.no_grad():
        for m in (rpn.rpn_conv, rpn.rpn_cls, rpn.rpn_reg):
            m.weight.normal_(0, 0.1)
            m.bias.normal_(0, 0.1)
    plain.load_state_dict(rpn.state_dict())
    rpn, plain = rpn.cuda(), plain.cuda()
    calls = count_calls(monkeypatch)
    with torch.no_grad():
        feats = neck(dev)
        n0 = len(calls)
        cls, reg = rpn(feats)
        assert len(calls) - n0 == 10                                     # two launches per level
        n0 = len(calls)
        plain(feats)
        assert len(calls) == n0                                          # the default head stays on torch's convolutions
        with torch.enable_grad():
            rpn(feats)
        assert len(calls) == n0                                          # ... and so does training
    # per-call bars (test_gpu_conv.py): the trunk against fp64 on its bf16 operands, then the heads on the device's trunk
    wt, bt = rpn.rpn_conv.weight.detach().cpu(), rpn.rpn_conv.bias.detach().cpu().double()
    wh = torch.cat([rpn.rpn_cls.weight, rpn.rpn_reg.weight]).detach().cpu()
    bh = torch.cat([rpn.rpn_cls.bias, rpn.rpn_reg.bias]).detach().cpu().double()
    monkeypatch.undo()
    for l, f in enumerate(feats):
        x = f.float().cpu().double()
        with torch.no_grad():
            t_dev = ops.conv2d_nhwc(f.permute(0, 2, 3, 1), ops.pack_conv_weight(rpn.rpn_conv.weight), rpn.rpn_conv.bias.float(),
                                    ksize=3, act="relu")
        t64 = F.conv2d(x, bf(wt).double(), bt, padding=1).clamp(min=0)
        S = F.conv2d(x.abs(), bf(wt).double().abs(), bt.abs(), padding=1)
        bar = (9 * 32 + 3) * EPS * S + 2.0 ** -8 * t64.abs()
        r1 = float(((t_dev.permute(0, 3, 1, 2).float().cpu().double() - t64).abs() / bar).max())
        td = t_dev.permute(0, 3, 1, 2).float().cpu().double()
        y64 = F.conv2d(td, bf(wh).double(), bh)
        S = F.conv2d(td.abs(), bf(wh).double().abs(), bh.abs())
        got = torch.cat([cls[l], reg[l]], 1).cpu().double()
        assert cls[l].dtype == torch.float32 and cls[l].is_contiguous() and tuple(reg[l].shape) == (B, 12) + tuple(f.shape[2:])
        r2 = float(((got - y64).abs() / ((32 + 3) * EPS * S)).max())
        print(f"RPN_RATIO level {l}: trunk {r1:.4f}, heads {r2:.4f}")
        assert r1 <= 1.0 and r2 <= 1.0, (l, r1, r2)
    metas = [dict(img_shape=(144, 208, 3)), dict(img_shape=(130, 200, 3))]
    with torch.no_grad():
        props = rpn.simple_test_rpn(feats, metas)
    assert len(props) == B
    for p, meta in zip(props, metas):
        assert p.is_cuda and p.shape[1] == 5 and 0 < p.shape[0] <= 40
        assert float(p[:, :4].min()) >= 0 and float(p[:, 2].max()) <= meta["img_shape"][1] and float(p[:, 3].max()) <= meta["img_shape"][0]
        assert bool((p[:, 4] >= 0).all()) and bool((p[:, 4] <= 1).all())
