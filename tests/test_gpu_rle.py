"""COCO run-length encoding on the device (csrc/rle.hip through ops.rle_encode and the dispatch of inference.rle_encode /
get_seg_masks / simple_test).  The format is integer: every assertion is byte equality of the strings with the host route
(inference.rle_encode on the CPU copy, which tests/test_rle.py pins to the worked vectors and an independent decoder)."""
import numpy as np
import pytest
import torch

import attentionshift_amd as A
from attentionshift_amd import inference as I, ops

pytestmark = pytest.mark.gpu


def _check(masks):
    """masks: numpy [n,H,W] bool or uint8 -> the device strings equal the host route's"""
    want = I.rle_encode(masks)
    dev = torch.from_numpy(masks).cuda()
    got = I.rle_encode(dev)
    assert len(got) == len(want) == masks.shape[0]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g["size"] == w["size"] == list(masks.shape[1:])
        assert g["counts"] == w["counts"], (i, masks.shape, g["counts"][:40], w["counts"][:40])
    assert ops.rle_encode(dev) == [w["counts"] for w in want]
    return got


def test_single_pixel():
    assert _check(np.zeros((1, 1, 1), bool))[0]["counts"] == b"1"
    assert _check(np.ones((1, 1, 1), bool))[0]["counts"] == b"01"


def test_the_worked_vectors():
    rect = np.zeros((4, 6), bool)
    rect[1:3, 2:5] = True
    first = np.zeros((4, 6), bool)
    first[0, 0] = True
    last = np.zeros((4, 6), bool)
    last[3, 5] = True
    seam = np.zeros((4, 6), bool)
    seam[3, 1] = seam[0, 2] = True
    got = _check(np.stack([rect, first, last, seam]))
    assert [g["counts"] for g in got] == [b"9220003", b"01g0", b"g01", b"72?"]
    got = _check(np.stack([np.zeros((3, 5), bool), np.ones((3, 5), bool)]))
    assert [g["counts"] for g in got] == [b"?", b"0?"]
    yy, xx = np.mgrid[0:5, 0:7]
    assert _check(((xx + yy) % 2 == 1)[None])[0]["counts"] == b"111" + b"0" * 32


@pytest.mark.parametrize("density", [0.5, 0.02])
def test_noise_with_unaligned_rows(density):
    gen = np.random.default_rng(11)
    _check(gen.random((7, 67, 131)) < density)            # W = 131: rows start at every alignment, a ragged last lane


def test_checkerboard_has_a_count_per_pixel():
    yy, xx = np.mgrid[0:33, 0:65]
    board = (xx + yy) % 2 == 1
    _check(np.stack([board, ~board]))


def test_one_row_and_one_column():
    gen = np.random.default_rng(12)
    _check(gen.random((1, 1, 300)) < 0.4)
    _check(gen.random((1, 300, 1)) < 0.4)


def test_five_byte_counts():
    zeros = np.zeros((1, 1024, 1024), bool)
    assert _check(zeros)[0]["counts"] == b"PPPP1"
    zeros[0, 1023, 1023] = True
    assert len(_check(zeros)[0]["counts"]) == 6           # [2^20 - 1, 1]


def test_runs_across_the_seams_of_lanes_waves_and_workgroups():
    rows, cols = ops.rle_tile()                           # rows per row segment (a wave), columns per workgroup
    waves = 4                                             # row segments per workgroup (256 threads)
    H, W = waves * rows + rows + 7, cols + 37             # a second workgroup in both directions, neither a multiple
    gen = np.random.default_rng(13)
    masks = np.zeros((3, H, W), bool)
    masks[0, rows - 6:waves * rows + 9, cols - 12:cols + 18] = True      # one block over every kind of seam
    masks[0, :, 5] = True                                 # a column that is one run from top to bottom
    masks[0] ^= gen.random((H, W)) < 0.01
    masks[1] = True                                       # one run over everything
    masks[2, rows - 1:rows + 1, :] = True                 # two rows around a segment seam: changes on both sides of it
    masks[2, waves * rows - 1, ::3] = False
    masks[2, H - 1, 7:] = True                            # the last row: runs go on over the column seam
    masks[2, 0, :W - 9] = True
    _check(masks)


def test_many_masks_with_different_totals():
    gen = np.random.default_rng(14)
    n = 130
    masks = np.stack([gen.random((9, 13)) < i / (n - 1) for i in range(n)])     # 0 all zero ... 129 all one
    assert not masks[0].any() and masks[n - 1].all()
    masks[64] = False                                     # an empty one in the middle
    masks[65] = True
    _check(masks)


def test_nothing_to_encode():
    assert I.rle_encode(torch.zeros(0, 8, 8, dtype=torch.bool).cuda()) == []
    assert ops.rle_encode(torch.zeros(0, 8, 8, dtype=torch.uint8).cuda()) == []


def test_bool_and_uint8_views_and_nonzero_bytes():
    gen = np.random.default_rng(15)
    m = gen.random((3, 40, 23)) < 0.3
    want = [w["counts"] for w in I.rle_encode(m)]
    dev = torch.from_numpy(m).cuda()
    assert ops.rle_encode(dev) == want
    assert ops.rle_encode(dev.view(torch.uint8)) == want
    values = torch.from_numpy(gen.integers(1, 256, m.shape).astype(np.uint8)).cuda()
    assert ops.rle_encode(dev.view(torch.uint8) * values) == want         # any nonzero byte counts as 1
    assert [w["counts"] for w in I.rle_encode((m * 255).astype(np.uint8))] == want


def test_a_slice_that_is_not_16_byte_aligned():
    gen = np.random.default_rng(16)
    m = gen.random((4, 37, 53)) < 0.2
    want = [w["counts"] for w in I.rle_encode(m)]
    for shift in (3, 9):
        buf = torch.ones(m.size + 32, dtype=torch.uint8).cuda()           # ones around the slice: reading past it would show
        view = buf[shift:shift + m.size].view(m.shape)
        view.copy_(torch.from_numpy(m).cuda())
        assert view.data_ptr() % 16 == shift and view.is_contiguous()
        assert ops.rle_encode(view) == want


def _seg_inputs():
    gen = torch.Generator().manual_seed(4)
    logits = torch.randn(5, 3, 28, 28, generator=gen) * 3
    xy = torch.rand(5, 2, generator=gen) * 100
    dets = torch.cat((xy, xy + 20 + torch.rand(5, 2, generator=gen) * 80, torch.rand(5, 1, generator=gen)), 1)
    return logits.cuda(), dets.cuda(), torch.tensor([2, 0, 2, 1, 2]).cuda()


def test_get_seg_masks_encodes_on_the_device(monkeypatch):
    logits, dets, labels = _seg_inputs()
    args = (logits, dets, labels, 3, (200, 333, 3), 1.0, True)
    calls = []
    real = ops.rle_encode
    monkeypatch.setattr(ops, "rle_encode", lambda m: (calls.append(tuple(m.shape)), real(m))[1])
    got = I.get_seg_masks(*args, encode_rle=True)
    assert calls == [(5, 200, 333)]
    bitmaps = I.get_seg_masks(*args)                      # the same paste kernel: equal, not banded
    assert calls == [(5, 200, 333)]
    assert [len(c) for c in got] == [1, 1, 3]
    assert got == I.encode_mask_results(bitmaps)
    assert sum(m.sum() for c in bitmaps for m in c) > 0
    with pytest.raises(ValueError):
        I.get_seg_masks(*args, mask_thr_binary=-1, encode_rle=True)


def test_the_switch_takes_the_host_route(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("AS_POST_HOST=1 did not keep the kernels out")
    logits, dets, labels = _seg_inputs()
    args = (logits, dets, labels, 3, (200, 333, 3), 1.0, True)
    m = torch.from_numpy(np.random.default_rng(17).random((2, 20, 31)) < 0.4).cuda()
    want = I.rle_encode(m.cpu().numpy())
    monkeypatch.setenv("AS_POST_HOST", "1")
    monkeypatch.setattr(ops, "rle_encode", boom)
    monkeypatch.setattr(ops, "paste_masks", boom)
    assert I.rle_encode(m) == want
    got = I.get_seg_masks(*args, encode_rle=True)
    assert got == I.encode_mask_results(I.get_seg_masks(*args))


def test_simple_test_encodes_its_masks():
    torch.manual_seed(0)                                  # the head of test_gpu_post.py::test_simple_test_is_the_same_on_both_routes
    dec = dict(in_channels=48, embed_dim=64, depth=1, num_heads=2, num_classes=5)
    head = A.build_head(dict(
        type="AttnShiftRoIHead",
        bbox_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=7, sampling_ratio=0)),
        mask_roi_extractor=dict(type="SingleRoIExtractor", featmap_strides=[16], roi_layer=dict(type="RoIAlign", output_size=14, sampling_ratio=0)),
        bbox_head=dict(type="MAEBoxHeadRec", with_reconstruct=False, cam_layer=3, **dec),
        mask_head=dict(type="MAEMaskHeadPointSup", scale_factor=2, scale_mode="bicubic", **dec),
        test_cfg=dict(score_thr=0.05, nms=dict(type="nms", iou_threshold=0.5), max_per_img=10, mask_thr_binary=0.5))).cuda()
    gen = torch.Generator().manual_seed(3)
    fmap = torch.rand(1, 48, 14, 14, generator=gen).cuda()
    xy = torch.rand(40, 2, generator=gen) * 120
    props = [torch.cat((xy, xy + 10 + torch.rand(40, 2, generator=gen) * 80), 1).cuda()]
    metas = [dict(img_shape=(224, 224, 3), ori_shape=(224, 224, 3), scale_factor=np.ones(4, dtype=np.float32))]
    with torch.no_grad():
        (boxes_bmp, segm_bmp), = head.simple_test(fmap, props, metas, rescale=False)
        head.test_cfg.encode_rle = True
        (boxes_rle, segm_rle), = head.simple_test(fmap, props, metas, rescale=False)
    n = sum(b.shape[0] for b in boxes_bmp)
    assert 0 < n <= 10
    for a, b in zip(boxes_bmp, boxes_rle):
        assert np.array_equal(a, b)
    assert all(isinstance(m, np.ndarray) for c in segm_bmp for m in c)
    assert sum(len(c) for c in segm_rle) == n and all(isinstance(m, dict) for c in segm_rle for m in c)
    assert segm_rle == I.encode_mask_results(segm_bmp)
