"""The test-time post-processing entry points (csrc/detect_post.hip: as_nms, as_paste_masks) without a GPU: exports,
workspace sizes, the argument checks that return before any launch, and the rule that CPU tensors never reach the
device route."""
import ctypes

import numpy as np
import pytest
import torch

from attentionshift_amd import _lib, inference as I, ops


def test_library_exports_the_post_processing_entry_points():
    from attentionshift_amd.csrc import build
    lib = ctypes.CDLL(build.build(verbose=False))
    for name in ("as_nms", "as_nms_workspace_bytes", "as_paste_masks"):
        assert hasattr(lib, name), name
        assert name in _lib.SIGNATURES, name


def test_nms_workspace_is_the_pair_bit_mask():
    lib = _lib.load()
    assert lib.as_nms_workspace_bytes(130) == 130 * 3 * 8
    assert lib.as_nms_workspace_bytes(0) == 0
    assert lib.as_nms_workspace_bytes(-5) == 0
    assert lib.as_nms_workspace_bytes(64) == 64 * 8
    assert lib.as_nms_workspace_bytes(65) == 65 * 2 * 8
    assert lib.as_nms_workspace_bytes(65535) == 65535 * 1024 * 8          # past 2^31: a size_t, not an int


def test_bad_arguments_return_error_codes_without_launching():
    lib = _lib.load()
    fake = 4096                                   # a non-null, aligned address: every case below returns before a launch
    assert lib.as_nms(None, 10, 0.5, -1, None, None, None, 0, None) == -1               # AS_E_BADARG
    assert b"null" in lib.as_last_error()
    assert lib.as_nms(None, 10, 0.5, -1, fake, fake, fake, 10 * 8, None) == -1
    assert lib.as_nms(fake, 10, 0.5, -1, fake, None, fake, 10 * 8, None) == -1
    assert lib.as_nms(fake, -1, 0.5, -1, fake, fake, fake, 0, None) == -1
    assert lib.as_nms(fake, 70000, 0.5, -1, fake, fake, fake, 1 << 40, None) == -2      # AS_E_UNSUPPORTED
    assert b"65535" in lib.as_last_error()
    assert lib.as_nms(fake, 130, 0.5, -1, fake, fake, fake, 130 * 3 * 8 - 1, None) == -4   # AS_E_WORKSPACE
    assert lib.as_paste_masks(None, None, None, None, 2, 3, 28, 28, 80, 100, 1, 1, 0.5, None) == -1
    assert lib.as_paste_masks(fake, None, fake, None, 2, 3, 28, 28, 80, 100, 1, 1, 0.5, None) == -1
    assert lib.as_paste_masks(fake, None, fake, fake, 2, 3, 28, 28, 80, 100, 1, 3, 0.5, None) == -1     # no such mode
    assert lib.as_paste_masks(fake, None, fake, fake, 2, 0, 28, 28, 80, 100, 1, 1, 0.5, None) == -1
    assert lib.as_paste_masks(fake, None, fake, fake, 2, 3, 200, 200, 80, 100, 1, 1, 0.5, None) == -2   # beyond the LDS tile
    assert lib.as_paste_masks(None, None, None, None, 0, 3, 28, 28, 80, 100, 1, 1, 0.5, None) == 0      # nothing to do


def test_wrappers_refuse_cpu_tensors():
    with pytest.raises(ops.AttnShiftError):
        ops.nms(torch.zeros(4, 4), 0.5)
    with pytest.raises(ops.AttnShiftError):
        ops.paste_masks(torch.zeros(2, 1, 28, 28), None, torch.zeros(2, 4), 8, 8, False, 0)


def test_cpu_tensors_never_reach_the_device_route(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("the device route was taken for CPU tensors")
    monkeypatch.setattr(ops, "nms", boom)
    monkeypatch.setattr(ops, "paste_masks", boom)
    gen = torch.Generator().manual_seed(0)
    xy = torch.rand(40, 2, generator=gen) * 100
    boxes = torch.cat((xy, xy + 10 + torch.rand(40, 2, generator=gen) * 50), 1)
    keep = I.nms(boxes, torch.rand(40, generator=gen), 0.5)
    assert 0 < keep.numel() <= 40
    dets, labels = I.multiclass_nms(boxes, torch.softmax(torch.randn(40, 4, generator=gen), 1), 0.05, 0.5, 7)
    assert dets.shape == (7, 5) and labels.shape == (7,)
    pb = torch.tensor([[10., 20., 30., 60.], [0., 0., 100., 80.]])
    full = I.paste_masks(torch.ones(2, 1, 28, 28), pb, 80, 100)
    assert full.shape == (2, 80, 100) and int((full[0] >= 0.5).sum()) == 40 * 20
    logits = torch.full((2, 3, 28, 28), -9.0)
    logits[0, 2] = 9.0
    logits[1, 0] = 9.0
    segm = I.get_seg_masks(logits, torch.cat((pb, torch.ones(2, 1)), 1), torch.tensor([2, 0]), 3, (80, 100, 3), 1.0, True)
    assert [len(s) for s in segm] == [1, 0, 1] and segm[2][0].dtype == np.bool_ and segm[2][0].sum() == 40 * 20
