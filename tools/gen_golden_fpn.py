"""Golden vectors for the FPN neck: executes the reference's own FPN.__init__ / init_weights / forward
(mmdet/models/necks/fpn.py:66-222, extracted with ast, decorators dropped, because `import mmdet` needs mmcv) on seeded fp32
inputs and stores inputs, the state dict and the five outputs in tests/golden/fpn.npz.  Container-only (needs /root/reference).

mmcv's ConvModule (absent here) is supplied as its definition under the defaults the neck is built with: an nn.Conv2d with
bias under the attribute `conv`, no norm, no activation; mmcv's xavier_init as its definition (xavier_uniform_ on the weight,
the bias set to a constant).  B = 2, in_channels [6, 8, 10, 12], out_channels 16, num_outs 5, level sizes (13, 21), (7, 11),
(3, 5), (2, 3): no upsample is an exact 2x.  The biases are re-drawn after init_weights (which zeroes them) so that the
fixture pins them too.
"""
import os
import sys
import warnings

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tools")):
    if p not in sys.path:
        sys.path.insert(0, p)

from gen_golden_mmdet_pure import REF, grab                # noqa: E402

IN_CHANNELS, OUT_CHANNELS, NUM_OUTS, B = [6, 8, 10, 12], 16, 5, 2
SIZES = [(13, 21), (7, 11), (3, 5), (2, 3)]
SEED = 20


class ConvModule(nn.Module):
    """mmcv.cnn.ConvModule with conv_cfg = norm_cfg = act_cfg = None"""

    def __init__(self, in_channels, out_channels, kernel_size, stride=1, padding=0, conv_cfg=None, norm_cfg=None, act_cfg=None,
                 inplace=True):
        super().__init__()
        assert conv_cfg is None and norm_cfg is None and act_cfg is None
        self.conv = nn.Conv2d(in_channels, out_channels, kernel_size, stride=stride, padding=padding, bias=True)

    def forward(self, x):
        return self.conv(x)


def xavier_init(module, gain=1, bias=0, distribution="normal"):
    """mmcv.cnn.xavier_init"""
    assert distribution in ("uniform", "normal")
    if distribution == "uniform":
        nn.init.xavier_uniform_(module.weight, gain=gain)
    else:
        nn.init.xavier_normal_(module.weight, gain=gain)
    if hasattr(module, "bias") and module.bias is not None:
        nn.init.constant_(module.bias, bias)


def main():
    ns = {"torch": torch, "nn": nn, "F": F, "warnings": warnings, "ConvModule": ConvModule, "xavier_init": xavier_init}
    grab(ns, REF + "/models/necks/fpn.py", ("__init__", "init_weights", "forward"), methods_of="FPN")
    ns["FPN"] = FPN = type("FPN", (nn.Module,), {k: ns[k] for k in ("__init__", "init_weights", "forward")})
    torch.manual_seed(SEED)
    neck = FPN(IN_CHANNELS, OUT_CHANNELS, NUM_OUTS)
    neck.init_weights()
    gen = torch.Generator().manual_seed(SEED + 1)
    with torch.no_grad():
        for m in neck.modules():
            if isinstance(m, nn.Conv2d):
                assert float(m.bias.abs().max()) == 0.0
                m.bias.copy_(torch.randn(m.bias.shape, generator=gen) * 0.1)
    inputs = [torch.randn(B, c, h, w, generator=gen) for c, (h, w) in zip(IN_CHANNELS, SIZES)]
    with torch.no_grad():
        outs = neck(inputs)
    assert len(outs) == NUM_OUTS
    st = {"seed": np.int64(SEED), "in_channels": np.int64(IN_CHANNELS), "out_channels": np.int64(OUT_CHANNELS),
          "num_outs": np.int64(NUM_OUTS), "sizes": np.int64(SIZES)}
    for i, x in enumerate(inputs):
        st[f"in_{i}"] = x.numpy()
    for i, o in enumerate(outs):
        st[f"out_{i}"] = o.numpy()
    sd = neck.state_dict()
    st["param_names"] = np.array(list(sd))
    for k, v in sd.items():
        st["param." + k] = v.numpy()
    path = os.path.join(ROOT, "tests", "golden", "fpn.npz")
    np.savez_compressed(path, **st)
    print("wrote", path, [tuple(o.shape) for o in outs], os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
