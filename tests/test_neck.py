"""The FPN neck without a GPU: the fp32 route against the fixture of the reference's own FPN (tests/golden/fpn.npz, written
by tools/gen_golden_fpn.py), the nearest-index rule against ATen's, the constructor's refusals and the registries.

The accumulation bound.  A convolution that sums K products, a bias and (the laterals) the upsampled map above in fp32, in
any order, lies within err(K, S) = (K + 3) * 2^-23 * S of its exact value, S = the same convolution of |x| and |w| plus
|bias| (and |add|), evaluated in fp64: one fp32 ulp of the running magnitude per accumulated term.  Through the two stages:
a lateral's error is its own bound plus the upsampled error of the lateral above, an output's error is its own bound plus
the lateral's error pushed through |w|.  Both the module's fp32 route and the fixture (the reference, in fp32) must lie
within that of the fp64 chain this file evaluates from the fixture's state dict.
"""
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import attentionshift_amd as A
from attentionshift_amd import neck as N

EPS = 2.0 ** -23
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "fpn.npz")


@pytest.fixture(scope="module")
def fixture():
    g = np.load(GOLDEN)
    cfg = dict(type="FPN", in_channels=[int(v) for v in g["in_channels"]], out_channels=int(g["out_channels"]),
               num_outs=int(g["num_outs"]))
    sd = {str(k): torch.from_numpy(g["param." + str(k)]) for k in g["param_names"]}
    ins = [torch.from_numpy(g[f"in_{i}"]) for i in range(len(cfg["in_channels"]))]
    outs = [torch.from_numpy(g[f"out_{i}"]) for i in range(cfg["num_outs"])]
    return cfg, sd, ins, outs


def chain_fp64(sd, ins, num_outs):
    """-> (outputs, error bounds) of the neck in fp64 from a state dict, per level"""
    n = len(ins)
    lat, e_lat = [None] * n, [None] * n
    for i in range(n - 1, -1, -1):
        w, b = sd[f"lateral_convs.{i}.conv.weight"].double(), sd[f"lateral_convs.{i}.conv.bias"].double()
        x = ins[i].double()
        y = F.conv2d(x, w, b)
        S = F.conv2d(x.abs(), w.abs(), b.abs())
        e = torch.zeros_like(y)
        if i + 1 < n:
            up = F.interpolate(lat[i + 1], size=y.shape[2:], mode="nearest")
            y, S = y + up, S + up.abs()
            e = F.interpolate(e_lat[i + 1], size=y.shape[2:], mode="nearest")
        lat[i], e_lat[i] = y, e + (w.shape[1] + 3) * EPS * S
    outs, errs = [], []
    for i in range(n):
        w, b = sd[f"fpn_convs.{i}.conv.weight"].double(), sd[f"fpn_convs.{i}.conv.bias"].double()
        S = F.conv2d(lat[i].abs(), w.abs(), b.abs(), padding=1)
        outs.append(F.conv2d(lat[i], w, b, padding=1))
        errs.append((9 * w.shape[1] + 3) * EPS * S + F.conv2d(e_lat[i], w.abs(), None, padding=1))
    for _ in range(num_outs - n):
        outs.append(outs[-1][:, :, ::2, ::2])
        errs.append(errs[-1][:, :, ::2, ::2])
    return outs, errs


def test_fp32_route_reproduces_the_reference(fixture):
    cfg, sd, ins, want = fixture
    neck = A.build_neck(dict(cfg, compute_dtype=torch.float32))
    assert sorted(neck.state_dict()) == sorted(sd)
    neck.load_state_dict(sd, strict=True)
    with torch.no_grad():
        got = neck(ins)
    exact, errs = chain_fp64(sd, ins, cfg["num_outs"])
    assert len(got) == len(want) == 5
    for l, (g, w, x, e) in enumerate(zip(got, want, exact, errs)):
        assert g.dtype == torch.float32 and g.shape == w.shape, l
        for name, t in (("module", g), ("fixture", w)):
            ratio = float(((t.double() - x).abs() / e).max())
            assert ratio <= 1.0, f"level {l}: {name} lies {ratio:.3f} bounds from the fp64 chain"


def test_default_route_on_cpu_tensors_and_under_grad_is_the_tensor_op_sequence(fixture):
    cfg, sd, ins, want = fixture
    neck = A.build_neck(cfg)                                            # compute_dtype=torch.bfloat16, CPU inputs
    neck.load_state_dict(sd)
    with torch.no_grad():
        a = neck(ins)
    with torch.enable_grad():
        b = neck(tuple(ins))
        for x, y in zip(a, b):
            assert torch.equal(x, y.detach())
        sum(o.sum() for o in b).backward()
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in neck.parameters())


def test_init_weights_is_xavier_uniform_with_zero_bias():
    torch.manual_seed(1)
    neck = A.build_neck(dict(type="FPN", in_channels=[6, 8, 10, 12], out_channels=16, num_outs=5))
    for m in neck.modules():
        if isinstance(m, torch.nn.Conv2d):
            torch.nn.init.normal_(m.bias)
    neck.init_weights()
    convs = [m for m in neck.modules() if isinstance(m, torch.nn.Conv2d)]
    assert len(convs) == 8
    for m in convs:
        k = m.kernel_size[0] * m.kernel_size[1]
        bound = math.sqrt(6.0 / ((m.in_channels + m.out_channels) * k))
        assert float(m.bias.detach().abs().max()) == 0.0
        assert 0.5 * bound < float(m.weight.detach().abs().max()) <= bound


def test_nearest_index_equals_atens():
    for n_in in range(1, 129):
        src = torch.arange(n_in, dtype=torch.float32).view(1, 1, n_in, 1)
        for n_out in range(n_in, 2 * n_in + 2):
            want = F.interpolate(src, size=(n_out, 1), mode="nearest").view(-1).long()
            assert torch.equal(N.nearest_src_index(n_out, n_in), want), (n_out, n_in)


@pytest.mark.parametrize("kw", [dict(add_extra_convs=True), dict(add_extra_convs="on_output"), dict(norm_cfg=dict(type="BN")),
                                dict(act_cfg=dict(type="ReLU")), dict(conv_cfg=dict(type="ConvWS")),
                                dict(upsample_cfg=dict(mode="bilinear")), dict(upsample_cfg=dict(scale_factor=2, mode="nearest")),
                                dict(relu_before_extra_convs=True), dict(compute_dtype=torch.float16)])
def test_unsupported_arguments_raise_with_the_key_named(kw):
    with pytest.raises(ValueError, match=next(iter(kw))):
        A.build_neck(dict(type="FPN", in_channels=[32] * 4, out_channels=32, num_outs=5, **kw))


def test_levels():
    with pytest.raises(ValueError):
        A.build_neck(dict(type="FPN", in_channels=[32] * 4, out_channels=32, num_outs=3))
    with pytest.raises(ValueError):
        A.build_neck(dict(type="FPN", in_channels=[32] * 4, out_channels=32, num_outs=5, end_level=3))
    neck = A.build_neck(dict(type="FPN", in_channels=[8, 16, 24, 32], out_channels=16, num_outs=2, start_level=1, end_level=3,
                             compute_dtype=torch.float32))
    assert sorted(neck.state_dict()) == sorted(f"{g}.{i}.conv.{p}" for g in ("lateral_convs", "fpn_convs") for i in (0, 1)
                                               for p in ("weight", "bias"))
    with torch.no_grad():
        outs = neck([torch.randn(1, c, s, s) for c, s in ((8, 16), (16, 8), (24, 4), (32, 2))])
    assert [tuple(o.shape) for o in outs] == [(1, 16, 8, 8), (1, 16, 4, 4)]


def test_registries_resolve_the_references_type_names():
    assert isinstance(A.build_neck(dict(type="FPN", in_channels=[32] * 4, out_channels=32, num_outs=5)), N.FPN)
    from attentionshift_amd import detector as D
    from attentionshift_amd.registry import DETECTORS, NECKS
    assert "FPN" in NECKS
    assert DETECTORS.get("FasterRCNNPointSupAlign") is D.FasterRCNNPointSupAlign
    assert DETECTORS.get("TwoStageDetectorPointSupAlign") is D.TwoStageDetectorPointSupAlign
    assert issubclass(D.FasterRCNNPointSupAlign, D.TwoStageDetectorPointSupAlign)
    model = dict(type="FasterRCNNPointSupAlign",
                 backbone=dict(type="VisionTransformerDet", img_size=64, patch_size=16, embed_dim=128, depth=2, num_heads=2,
                               out_indices=(0, 0, 1, 1), last_feat=True, point_tokens_num=4, num_classes=5, return_attention=True),
                 neck=dict(type="FPN", in_channels=[128] * 4, out_channels=32, num_outs=5),
                 rpn_head=dict(type="RPNHead", in_channels=32, feat_channels=32,
                               anchor_generator=dict(type="AnchorGenerator", scales=[8], ratios=[0.5, 1.0, 2.0],
                                                     strides=[4, 8, 16, 32, 64])),
                 roi_head=dict(type="AttnShiftRoIHead", bbox_head=dict(type="MAEBoxHeadRec", cam_layer=2, num_classes=5),
                               mil_head=dict(type="MAEBoxHeadMIL", num_layers_query=2)),
                 roi_skip_fpn=True,
                 train_cfg=dict(rpn=dict(allowed_border=-1), rpn_proposal=dict(nms_pre=100, max_per_img=50, nms=dict(iou_threshold=0.7)),
                                rcnn=dict()),
                 test_cfg=dict(rpn=dict(nms_pre=100, max_per_img=50, nms=dict(type="nms", iou_threshold=0.7), min_bbox_size=0),
                               rcnn=dict(score_thr=0.05)))
    det = A.build_detector(model)
    assert isinstance(det, D.FasterRCNNPointSupAlign) and det.with_neck and det.with_rpn and det.with_roi_head
    assert det.rpn_head.test_cfg["nms_pre"] == 100 and det.rpn_head.train_cfg["allowed_border"] == -1
    assert det.neck.compute_dtype == torch.bfloat16 and det.rpn_head.compute_dtype is None
    det = A.build_detector(dict(model, compute_dtype=torch.bfloat16))
    assert det.rpn_head.compute_dtype == torch.bfloat16
    for call in (lambda: det.aug_test([], []), lambda: A.build_detector(dict(model, visualize=True))):
        with pytest.raises(NotImplementedError):
            call()
