"""The RPN training-target entry points (csrc/rpn_train.hip: as_rpn_assign, as_rpn_sample, as_rpn_targets) without a GPU:
exports, the workspace size, the argument checks that return before any launch (a launch here, without a device, would
return AS_E_LAUNCH = -3), and the rule that CPU tensors never reach the kernels."""
import ctypes

import pytest
import torch

from attentionshift_amd import _lib, ops, rpn_train as RT

FAKE = 4096                                       # a non-null, 16-byte aligned address: every case below returns before a launch
NAMES = ("as_rpn_assign_workspace_bytes", "as_rpn_assign", "as_rpn_sample", "as_rpn_targets")
SIZES = [(8, 12), (4, 6), (2, 3)]
T = 3 * (96 + 24 + 6)


def test_library_exports_the_entry_points():
    from attentionshift_amd.csrc import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_workspace_is_the_box_maxima_and_the_block_counts():
    lib = _lib.load()
    # 4 bytes per box rounded up to 16, then (positives, negatives) per 256 anchors of every image
    for B, t, G in ((1, 1, 0), (2, 378, 27), (2, 105, 1), (1, 18432, 65), (2, 261888, 40), (3, 256, 4), (3, 257, 5)):
        assert lib.as_rpn_assign_workspace_bytes(B, t, G) == 16 * ((G + 3) // 4) + 8 * B * ((t + 255) // 256), (B, t, G)
    for B, t, G in ((0, 100, 3), (2, 0, 3), (-1, 100, 3), (2, 100, -1)):
        assert lib.as_rpn_assign_workspace_bytes(B, t, G) == 0


def _levels(sizes, stride=8):
    arr = (_lib.RpnLevel * max(len(sizes), 1))()
    for l, (h, w) in enumerate(sizes):
        arr[l] = _lib.RpnLevel(None, None, h, w, stride, stride)
    return arr


def _assign(lib, sizes=SIZES, A=3, B=2, L=None, levels="make", base=FAKE, gt=FAKE, offs=FAKE, sum_g=5, max_g=3, shapes=FAKE,
            outs=FAKE, ws=FAKE, ws_bytes=1 << 60, stride=8):
    arr = _levels(sizes, stride) if levels == "make" else levels
    out = [outs] * 3 if not isinstance(outs, list) else outs
    return lib.as_rpn_assign(ctypes.addressof(arr) if arr is not None else None, len(sizes) if L is None else L, B, A, base, gt, offs,
                             sum_g, max_g, shapes, 0.7, 0.3, 0.3, 1, -1, *out, ws, ws_bytes, None)


def _sample(lib, B=2, t=T, sum_g=5, num=32, assigned=FAKE, plan=FAKE, ranks=FAKE, ws=FAKE, ws_bytes=1 << 60, inds=FAKE):
    return lib.as_rpn_sample(B, t, sum_g, num, assigned, plan, ranks, ws, ws_bytes, inds, None)


def _targets(lib, sizes=SIZES, A=3, B=2, levels="make", base=FAKE, gt=FAKE, offs=FAKE, sum_g=5, assigned=FAKE, inds=FAKE, stride_=64,
             num=32, norm="make", pos_gt=FAKE, delta=FAKE):
    arr = _levels(sizes) if levels == "make" else levels
    ms = (ctypes.c_float * 8)(0, 0, 0, 0, 1, 1, 1, 1) if norm == "make" else norm
    return lib.as_rpn_targets(ctypes.addressof(arr) if arr is not None else None, len(sizes), B, A, base, gt, offs, sum_g, assigned, inds,
                              stride_, num, ctypes.addressof(ms) if ms is not None else None, pos_gt, delta, None)


def test_assign_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    assert _assign(lib, levels=None) == -1                               # AS_E_BADARG: null pointers
    assert b"null" in lib.as_last_error()
    for name in ("base", "gt", "offs", "shapes", "ws"):
        assert _assign(lib, **{name: None}) == -1, name
    for k in range(3):
        assert _assign(lib, outs=[FAKE] * k + [None] + [FAKE] * (2 - k)) == -1
    assert _assign(lib, L=0) == -1                                       # L outside 1 .. 8
    assert _assign(lib, sizes=[(2, 2)] * 9) == -1
    assert b"L = 9" in lib.as_last_error()
    assert _assign(lib, A=0) == -1
    assert _assign(lib, B=-1) == -1
    assert _assign(lib, sizes=[(8, 12), (0, 6)]) == -1                   # an empty level
    assert _assign(lib, stride=0) == -1
    assert _assign(lib, sum_g=2, max_g=3) == -1                          # more boxes in one image than in all
    assert _assign(lib, sum_g=-1, max_g=0) == -1
    assert _assign(lib, ws=FAKE + 8) == -1                               # alignment
    need = 16 * 2 + 8 * 2 * 2
    assert _assign(lib, ws_bytes=need - 1) == -4                         # AS_E_WORKSPACE
    assert b"needed" in lib.as_last_error()
    assert _assign(lib, gt=None, sum_g=0, max_g=0, ws_bytes=0) == -4     # no boxes at all is a valid call: gets to the workspace
    assert _assign(lib, B=0, base=None, gt=None, offs=None, shapes=None, outs=None, ws=None, ws_bytes=0) == 0    # nothing to do


def test_assign_problems_beyond_the_limits_are_unsupported_without_launching():
    lib = _lib.load()
    assert _assign(lib, sum_g=2000, max_g=1025) == -2                    # AS_E_UNSUPPORTED: more than 1024 boxes in an image
    assert b"1024" in lib.as_last_error()
    assert _assign(lib, sum_g=2000, max_g=1024, ws_bytes=0) == -4        # 1024 fit
    assert _assign(lib, sizes=[(16384, 16384)], A=1, stride=1) == -2     # a level of 2^28 anchors
    assert _assign(lib, B=65536) == -2


def test_sample_and_targets_check_their_arguments_without_launching():
    lib = _lib.load()
    for name in ("assigned", "plan", "ranks", "ws", "inds"):
        assert _sample(lib, **{name: None}) == -1, name
    assert _sample(lib, t=0) == -1
    assert _sample(lib, num=0) == -1
    assert _sample(lib, B=-1) == -1
    assert _sample(lib, num=2049) == -2                                  # one sort of 2048 indices in LDS
    assert b"2048" in lib.as_last_error()
    assert _sample(lib, num=2048, ws_bytes=0) == -4
    assert _sample(lib, ws_bytes=16 * 2 + 8 * 2 * 2 - 1) == -4
    assert _sample(lib, B=0, assigned=None, plan=None, ranks=None, ws=None, inds=None) == 0
    assert _targets(lib, levels=None) == -1
    for name in ("base", "gt", "offs", "assigned", "inds", "norm", "pos_gt", "delta"):
        assert _targets(lib, **{name: None}) == -1, name
    assert _targets(lib, num=0) == -1
    assert _targets(lib, stride_=31) == -1                               # rows shorter than num
    assert _targets(lib, delta=FAKE + 4) == -1                           # alignment
    assert _targets(lib, num=2049, stride_=4098) == -2
    assert _targets(lib, sizes=[(16384, 16384)], A=1) == -2
    assert _targets(lib, B=0, base=None, gt=None, offs=None, assigned=None, inds=None, pos_gt=None, delta=None) == 0


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(ops.AttnShiftError):
        ops.rpn_assign(torch.zeros(1, 1, 4), [(4, 4)], [8], torch.zeros(1, 4), torch.zeros(2, dtype=torch.int32), 1, 1,
                       torch.zeros(1, 4, dtype=torch.int32), 0.7, 0.3, 0.3, True, -1)
    with pytest.raises(ops.AttnShiftError):
        ops.rpn_sample(torch.zeros(1, 16, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.int32),
                       torch.zeros(1, 2, 8, dtype=torch.int32), torch.zeros(64, dtype=torch.uint8), 1)
    with pytest.raises(ops.AttnShiftError):
        ops.rpn_targets(torch.zeros(1, 1, 4), [(4, 4)], [8], torch.zeros(1, 4), torch.zeros(2, dtype=torch.int32), 1,
                        torch.zeros(1, 16, dtype=torch.int32), torch.zeros(1, 2, 8, dtype=torch.int32))


def test_cpu_inputs_never_reach_the_kernels(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device route was taken for a CPU input")
    for name in ("rpn_assign", "rpn_sample", "rpn_targets"):
        monkeypatch.setattr(ops, name, boom)
    base = torch.tensor([[[-8., -8., 8., 8.]]])
    asg = RT.rpn_assign(base, [(4, 4)], [8], [torch.tensor([[8., 8., 24., 24.]])], [dict(img_shape=(32, 32, 3), pad_shape=(32, 32, 3))],
                        dict(pos_iou_thr=0.7, neg_iou_thr=0.3, min_pos_iou=0.3), -1)
    smp = RT.rpn_sample(asg, 8, 0.5, -1, torch.Generator().manual_seed(0))
    pos_gt, pos_delta = RT.rpn_targets(asg, smp)
    assert smp.n_pos == [1] and pos_gt[0, 0] == 0 and not bool(pos_delta[0, 0].any())
