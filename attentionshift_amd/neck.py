"""The feature pyramid between the backbone and the heads: mmdet's FPN, restated (mmdet/models/necks/fpn.py:66-222).

    FPN      lateral 1x1 convolutions, the top-down path (nearest upsample to the lower level's size, added), 3x3 output
             convolutions, extra levels by `max_pool2d(., 1, stride=2)`.  Built: add_extra_convs=False, no norm, no
             activation, upsample_cfg=dict(mode='nearest'); anything else raises in __init__.  Parameter names are mmcv's
             ConvModule keys (lateral_convs.{i}.conv.*, fpn_convs.{i}.conv.*), so the reference's checkpoints load.

Two routes.  compute_dtype=torch.float32, CPU tensors or grad enabled: the reference's tensor-op sequence (F.conv2d,
F.interpolate, F.max_pool2d) -- also the training path through autograd.  compute_dtype=torch.bfloat16 (default) on device
tensors under no-grad: 2 * levels launches of as_conv2d_fwd (csrc/conv.hip) on channels-last bf16 maps -- the laterals from
the top level down with the upsample + add folded into the epilogue, then the output convolutions; the extra levels are the
[::2, ::2] pixels of the last output.
"""
import warnings

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import ops
from .registry import NECKS


def nearest_src_index(out_size, in_size):
    """ATen's nearest-neighbour source index of F.interpolate(size=out_size, mode='nearest') along one axis, as a LongTensor
    [out_size]: min((int)floorf(i * ((float)in_size / out_size)), in_size - 1), evaluated in fp32 -- the rule the `add`
    epilogue of as_conv2d_fwd applies."""
    scale = torch.tensor(float(in_size), dtype=torch.float32) / torch.tensor(float(out_size), dtype=torch.float32)
    idx = torch.floor(torch.arange(int(out_size), dtype=torch.float32) * scale).long()
    return idx.clamp_(max=int(in_size) - 1)


class _Conv(nn.Module):
    """mmcv's ConvModule with its defaults here: a biased nn.Conv2d under the attribute `conv`, no norm, no activation"""

    def __init__(self, cin, cout, ksize):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, ksize, padding=(ksize - 1) // 2)

    def forward(self, x):
        return self.conv(x)


class PackedConvCache:
    """bf16 tap-major weights (ops.pack_conv_weight) and fp32 biases of convolutions, rebuilt when a parameter's version or
    device changes (the way VisionTransformerDet._deconv2x2 keeps its GEMM matrix)."""

    def __init__(self):
        self._hit = {}

    def get(self, key, weights, biases):
        """weights / biases: lists of parameters stacked along Cout (one entry for a plain convolution)"""
        srcs = list(weights) + list(biases)
        stamp = tuple(t._version for t in srcs) + tuple(t.data_ptr() for t in srcs) + (weights[0].device,)
        hit = self._hit.get(key)
        if hit is None or hit[0] != stamp:
            with torch.no_grad():
                w = ops.pack_conv_weight(torch.cat([t.detach() for t in weights]))
                b = torch.cat([t.detach().float() for t in biases])
                b = torch.cat([b, b.new_zeros(w.shape[0] - b.shape[0])]).contiguous()
            hit = self._hit[key] = (stamp, w, b)
        return hit[1], hit[2]


def nhwc_bf16(x):
    """An NCHW-shaped map (a view of channels-last memory, or not) -> its [B,H,W,C] bf16 form, cast at most once: bf16
    channels-last views pass through untouched."""
    x = x.permute(0, 2, 3, 1)
    return x if x.dtype == torch.bfloat16 else x.to(torch.bfloat16)


_WARNED = set()


def warn_once(key, msg):
    if key not in _WARNED:
        _WARNED.add(key)
        warnings.warn(msg, RuntimeWarning, stacklevel=3)


@NECKS.register_module()
class FPN(nn.Module):
    def __init__(self, in_channels, out_channels, num_outs, start_level=0, end_level=-1, add_extra_convs=False,
                 extra_convs_on_inputs=True, relu_before_extra_convs=False, no_norm_on_lateral=False, conv_cfg=None,
                 norm_cfg=None, act_cfg=None, upsample_cfg=dict(mode="nearest"), compute_dtype=torch.bfloat16):
        super().__init__()
        if not isinstance(in_channels, (list, tuple)):
            raise TypeError("FPN: in_channels must be a list")
        for key, val in (("add_extra_convs", add_extra_convs), ("relu_before_extra_convs", relu_before_extra_convs),
                         ("conv_cfg", conv_cfg), ("norm_cfg", norm_cfg), ("act_cfg", act_cfg)):
            if val:
                raise ValueError(f"FPN: {key}={val!r} is not built (plain biased convolutions, extra levels by striding)")
        if dict(upsample_cfg or {}) != dict(mode="nearest"):
            raise ValueError(f"FPN: upsample_cfg={upsample_cfg!r} is not built (only dict(mode='nearest'))")
        if compute_dtype not in (torch.bfloat16, torch.float32):
            raise ValueError(f"FPN: compute_dtype={compute_dtype!r} (torch.bfloat16 or torch.float32)")
        self.in_channels, self.out_channels = list(in_channels), int(out_channels)
        self.num_ins, self.num_outs = len(in_channels), int(num_outs)
        if end_level == -1:
            self.backbone_end_level = self.num_ins
            if num_outs < self.num_ins - start_level:
                raise ValueError("FPN: num_outs is smaller than the number of used input levels")
        else:
            self.backbone_end_level = end_level
            if end_level > self.num_ins or num_outs != end_level - start_level:
                raise ValueError("FPN: with an end_level, num_outs must equal end_level - start_level")
        self.start_level, self.end_level = start_level, end_level
        self.compute_dtype = compute_dtype
        self.lateral_convs, self.fpn_convs = nn.ModuleList(), nn.ModuleList()
        for i in range(self.start_level, self.backbone_end_level):
            self.lateral_convs.append(_Conv(in_channels[i], out_channels, 1))
            self.fpn_convs.append(_Conv(out_channels, out_channels, 3))
        self._packed = PackedConvCache()
        self.init_weights()

    def init_weights(self):
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.xavier_uniform_(m.weight, gain=1)
                nn.init.constant_(m.bias, 0)

    # ---- the reference's tensor-op sequence (fpn.py:170-222): fp32 parity, CPU tensors, training ---------------------
    def _forward_ops(self, inputs):
        dt = self.lateral_convs[0].conv.weight.dtype
        laterals = [lat(inputs[i + self.start_level].to(dt)) for i, lat in enumerate(self.lateral_convs)]
        n = len(laterals)
        for i in range(n - 1, 0, -1):
            laterals[i - 1] = laterals[i - 1] + F.interpolate(laterals[i], size=laterals[i - 1].shape[2:], mode="nearest")
        outs = [self.fpn_convs[i](laterals[i]) for i in range(n)]
        for _ in range(self.num_outs - n):
            outs.append(F.max_pool2d(outs[-1], 1, stride=2))
        return tuple(outs)

    # ---- channels-last bf16 on as_conv2d_fwd ---------------------------------------------------------------------------
    def _forward_hip(self, inputs):
        n = len(self.lateral_convs)
        laterals = [None] * n
        for i in range(n - 1, -1, -1):                      # top level first: the epilogue adds the stored map above
            c = self.lateral_convs[i].conv
            w, b = self._packed.get(("lat", i), [c.weight], [c.bias])
            laterals[i] = ops.conv2d_nhwc(nhwc_bf16(inputs[i + self.start_level]), w, b, ksize=1,
                                          add=laterals[i + 1] if i + 1 < n else None)
        outs = []
        for i in range(n):
            c = self.fpn_convs[i].conv
            w, b = self._packed.get(("out", i), [c.weight], [c.bias])
            outs.append(ops.conv2d_nhwc(laterals[i], w, b, ksize=3))
        for _ in range(self.num_outs - n):
            outs.append(outs[-1][:, ::2, ::2])
        return tuple(o.permute(0, 3, 1, 2) for o in outs)

    def forward(self, inputs):
        """inputs: the backbone's maps (a tuple, a list or a DeferredFPN), NCHW-shaped -> num_outs NCHW-shaped maps"""
        inputs = tuple(inputs)
        if len(inputs) != self.num_ins:
            raise ValueError(f"FPN: {len(inputs)} input maps for {self.num_ins} in_channels")
        hip = self.compute_dtype == torch.bfloat16 and not torch.is_grad_enabled() and all(x.is_cuda for x in inputs)
        if hip and (self.out_channels % 32 or any(c % 32 for c in self.in_channels[self.start_level:self.backbone_end_level])):
            warn_once(("FPN", tuple(self.in_channels), self.out_channels),
                      f"FPN: channels {self.in_channels} -> {self.out_channels} miss as_conv2d_fwd's contract (input channels "
                      "a multiple of 32, output channels a multiple of 16): taking the tensor-op route")
            hip = False
        return self._forward_hip(inputs) if hip else self._forward_ops(inputs)
