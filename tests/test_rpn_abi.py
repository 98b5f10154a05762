"""The RPN candidate entry points (csrc/rpn.hip: as_rpn_candidates) without a GPU: exports, the workspace size, the
argument checks that return before any launch (a launch here, without a device, would return AS_E_LAUNCH = -3), and the
rule that CPU tensors never reach the kernels."""
import ctypes

import pytest
import torch

from attentionshift_amd import _lib, inference as I, ops

FAKE = 4096                                       # a non-null, 16-byte aligned address: every case below returns before a launch


def test_library_exports_the_rpn_entry_points():
    from attentionshift_amd.csrc import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("as_rpn_candidates", "as_rpn_candidates_workspace_bytes"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_is_the_keys_and_the_staged_candidates():
    lib = _lib.load()
    # per candidate: the 8-byte key + the staged box (16), score, level and index (4 each)
    for B, C in ((1, 1), (2, 219), (1, 4768), (2, 8819), (3, 16384), (65535, 16384)):
        assert lib.as_rpn_candidates_workspace_bytes(B, C) == 36 * B * C, (B, C)
    for B, C in ((0, 100), (2, 0), (-1, 100), (2, -5)):
        assert lib.as_rpn_candidates_workspace_bytes(B, C) == 0


def _levels(sizes, cls=FAKE, reg=FAKE, stride=8):
    arr = (_lib.RpnLevel * max(len(sizes), 1))()
    for l, (h, w) in enumerate(sizes):
        arr[l] = _lib.RpnLevel(cls, reg, h, w, stride, stride)
    return arr


def _call(lib, sizes, A=3, B=2, nms_pre=100, C=None, levels="make", L=None, base=FAKE, shapes=FAKE, norm="make", outs=FAKE, ws=FAKE,
          ws_bytes=1 << 60, **lv):
    arr = _levels(sizes, **lv) if levels == "make" else levels
    ms = (ctypes.c_float * 8)(0, 0, 0, 0, 1, 1, 1, 1) if norm == "make" else norm
    if C is None:
        C = sum(A * h * w if nms_pre <= 0 else min(nms_pre, A * h * w) for h, w in sizes)
    out = [outs] * 6 if not isinstance(outs, list) else outs
    return lib.as_rpn_candidates(ctypes.addressof(arr) if arr is not None else None, len(sizes) if L is None else L, B, A, base,
                                 shapes, nms_pre, 0.0, ctypes.addressof(ms) if ms is not None else None, 4.135, C, *out, ws,
                                 ws_bytes, None)


def test_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    sizes = [(8, 12), (4, 6), (2, 3)]
    assert _call(lib, sizes, levels=None) == -1                          # AS_E_BADARG: null pointers
    assert b"null" in lib.as_last_error()
    assert _call(lib, sizes, norm=None) == -1
    assert _call(lib, sizes, cls=None) == -1
    assert _call(lib, sizes, reg=None) == -1
    assert _call(lib, sizes, base=None) == -1
    assert _call(lib, sizes, shapes=None) == -1
    assert _call(lib, sizes, ws=None) == -1
    for k in range(6):
        assert _call(lib, sizes, outs=[FAKE] * k + [None] + [FAKE] * (5 - k)) == -1
    assert _call(lib, sizes, L=0) == -1                                  # L outside 1 .. 8
    assert _call(lib, [(2, 2)] * 9, L=9) == -1
    assert b"L = 9" in lib.as_last_error()
    assert _call(lib, sizes, A=0) == -1
    assert _call(lib, sizes, B=-1) == -1
    assert _call(lib, [(8, 12), (0, 6)]) == -1                           # an empty level
    assert _call(lib, sizes, C=100 + 72 + 18 + 1) == -1                  # C is not what the levels and nms_pre give
    assert _call(lib, sizes, stride=-8) == -1
    assert _call(lib, sizes, ws=FAKE + 8) == -1                          # alignment
    assert _call(lib, sizes, outs=[FAKE + 4] + [FAKE] * 5) == -1
    assert _call(lib, sizes, ws_bytes=36 * 2 * 190 - 1) == -4            # AS_E_WORKSPACE
    assert _call(lib, sizes, ws_bytes=36 * 2 * 190, B=0, base=None, shapes=None, outs=None, ws=None) == 0     # nothing to do


def test_problems_beyond_the_limits_are_unsupported_without_launching():
    lib = _lib.load()
    assert _call(lib, [(64, 96)], nms_pre=-1) == -2                      # AS_E_UNSUPPORTED: C = 18432 > 16384
    assert b"16384" in lib.as_last_error()
    assert _call(lib, [(64, 96)], nms_pre=2049) == -2                    # more than 2048 survivors in a level
    assert _call(lib, [(16384, 16384)], A=1, nms_pre=1000) == -2         # a level of 2^28 candidates
    assert _call(lib, [(26, 26)] * 8, nms_pre=-1, ws_bytes=0) == -4      # 8 x 2028 = 16224 fits: gets as far as the workspace
    assert _call(lib, [(8, 12)], B=65536) == -2


def test_wrapper_refuses_cpu_tensors():
    cls, reg = [torch.zeros(1, 3, 4, 4)], [torch.zeros(1, 12, 4, 4)]
    with pytest.raises(ops.AttnShiftError):
        ops.rpn_candidates(cls, reg, torch.zeros(1, 3, 4), [(8, 8)], [(32, 32, 3)], 10)


def test_cpu_inputs_never_reach_the_kernels(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device route was taken for a CPU input")
    monkeypatch.setattr(ops, "rpn_candidates", boom)
    monkeypatch.setattr(ops, "nms", boom)
    gen = torch.Generator().manual_seed(0)
    cls, reg = [torch.randn(1, 3, 4, 4, generator=gen)], [torch.randn(1, 12, 4, 4, generator=gen) * 0.2]
    base = torch.tensor([[[-8., -4., 8., 4.], [-6., -6., 6., 6.], [-4., -8., 4., 8.]]])
    props = I.rpn_proposals(cls, reg, base, [8], [(32, 32, 3)], 10, 5, 0.7)
    assert props[0].shape[1] == 5 and 0 < props[0].shape[0] <= 5
