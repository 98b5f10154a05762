"""The convolution entry point (csrc/conv.hip: as_conv2d_fwd) without a GPU: exports, the argument checks that return before
any launch (a launch here, without a device, would return AS_E_LAUNCH = -3), the tile choice as a pure host function, and
the rule that CPU tensors never reach the kernel."""
import ctypes

import pytest
import torch

from attentionshift_amd import _lib, ops

FAKE = 4096                                       # a non-null, 16-byte aligned address: every case below returns before a launch


def _call(lib, x=FAKE, w=FAKE, bias=FAKE, add=None, out=FAKE, B=2, H=8, W=12, Cin=64, Cout=32, ksize=3, act=0, dt=1, bs=None,
          Ha=0, Wa=0):
    bs = H * W * Cin if bs is None else bs
    return lib.as_conv2d_fwd(x, bs, w, bias, add, Ha, Wa, B, H, W, Cin, Cout, ksize, act, dt, out, None)


def test_library_exports_the_conv_entry_points():
    from attentionshift_amd.csrc import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("as_conv2d_fwd", "as_conv2d_tile_n"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    for k in ("x", "w", "out"):
        assert _call(lib, **{k: None}) == -1                             # AS_E_BADARG: null pointers
        assert b"null" in lib.as_last_error()
    assert _call(lib, Cin=48) == -1
    assert b"Cin = 48" in lib.as_last_error()
    assert _call(lib, Cout=8) == -1
    assert b"Cout = 8" in lib.as_last_error()
    assert _call(lib, ksize=2) == -1
    assert b"ksize = 2" in lib.as_last_error()
    assert _call(lib, H=0) == -1
    assert b"H = 0" in lib.as_last_error()
    assert _call(lib, W=0) == -1 and _call(lib, B=0) == -1 and _call(lib, Cin=0) == -1 and _call(lib, Cout=0) == -1
    assert _call(lib, ksize=5) == -1 and _call(lib, act=2) == -1 and _call(lib, dt=7) == -1
    for k in ("x", "w", "out", "bias"):
        assert _call(lib, **{k: FAKE + 8}) == -1                         # alignment
        assert b"aligned" in lib.as_last_error()
    assert _call(lib, add=FAKE + 2, Ha=4, Wa=6) == -1
    assert _call(lib, bs=8 * 12 * 64 - 8) == -1                          # images that overlap
    assert _call(lib, bs=8 * 12 * 64 + 4) == -1                          # a batch stride that breaks the 16-byte rows
    assert _call(lib, add=FAKE, Ha=0, Wa=6) == -1                        # an empty add
    assert _call(lib, add=FAKE, Ha=9, Wa=6) == -1                        # an add larger than the output
    assert _call(lib, B=4, H=4096, W=4096, Cin=32) == -2                 # AS_E_UNSUPPORTED: 32-bit byte offsets
    assert b"2^31" in lib.as_last_error()


def test_tile_choice_is_a_pure_host_function():
    lib = _lib.load()
    assert [lib.as_conv2d_tile_n(c) for c in (16, 32, 64, 80, 96, 128, 256)] == [32, 32, 32, 32, 128, 128, 128]
    assert lib.as_conv2d_tile_n(0) == 0 and lib.as_conv2d_tile_n(-16) == 0
    assert ops.conv2d_tile_n(256) == 128 and ops.conv2d_tile_n(16) == 32


def test_packed_weight_is_tap_major_bf16_with_padded_rows():
    w = torch.arange(15 * 32 * 9, dtype=torch.float32).reshape(15, 32, 3, 3) / 64
    p = ops.pack_conv_weight(w)
    assert p.dtype == torch.bfloat16 and tuple(p.shape) == (16, 3, 3, 32) and p.is_contiguous()
    assert torch.equal(p[:15], w.permute(0, 2, 3, 1).to(torch.bfloat16)) and float(p[15].abs().max()) == 0.0


def test_wrapper_refuses_cpu_tensors():
    with pytest.raises(ops.AttnShiftError):
        ops.conv2d_nhwc(torch.zeros(1, 4, 4, 32, dtype=torch.bfloat16), torch.zeros(16, 3, 3, 32, dtype=torch.bfloat16))


def test_cpu_inputs_never_reach_the_kernel(monkeypatch):
    import attentionshift_amd as A

    def boom(*a, **k):
        raise AssertionError("the device route was taken for a CPU input")
    monkeypatch.setattr(ops, "conv2d_nhwc", boom)
    neck = A.build_neck(dict(type="FPN", in_channels=[32, 32], out_channels=32, num_outs=3))
    with torch.no_grad():
        outs = neck([torch.zeros(1, 32, 6, 8), torch.zeros(1, 32, 3, 4)])
    assert [tuple(o.shape) for o in outs] == [(1, 32, 6, 8), (1, 32, 3, 4), (1, 32, 2, 2)]
    rpn = A.build_head(dict(type="RPNHead", in_channels=32, feat_channels=32, compute_dtype=torch.bfloat16))
    with torch.no_grad():
        cls, reg = rpn(outs)
    assert tuple(cls[0].shape) == (1, 3, 6, 8) and tuple(reg[2].shape) == (1, 12, 2, 2)
