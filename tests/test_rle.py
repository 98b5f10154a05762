"""COCO run-length encoding on the host route (inference.rle_encode / encode_mask_results, the restatement of
mmdet/core/mask/utils.py:36-63 without pycocotools): the worked vectors of the format, a round trip through an independent
decoder (rleFrString + fill, written here), the structure encode_mask_results keeps, and get_seg_masks(encode_rle=True).
CPU only."""
import numpy as np
import pytest
import torch

from attentionshift_amd import inference as I


def _table():
    """(name, mask [H,W], counts, string) of the format's worked examples"""
    rect = np.zeros((4, 6), bool)
    rect[1:3, 2:5] = True
    first = np.zeros((4, 6), bool)
    first[0, 0] = True
    last = np.zeros((4, 6), bool)
    last[3, 5] = True
    seam = np.zeros((4, 6), bool)
    seam[3, 1] = seam[0, 2] = True
    yy, xx = np.mgrid[0:5, 0:7]
    return [
        ("zeros 3x5", np.zeros((3, 5), bool), [15], b"?"),
        ("ones 3x5", np.ones((3, 5), bool), [0, 15], b"0?"),
        ("zeros 1024x1024", np.zeros((1024, 1024), bool), [1048576], b"PPPP1"),
        ("rectangle", rect, [9, 2, 2, 2, 2, 2, 5], b"9220003"),
        ("first pixel", first, [0, 1, 23], b"01g0"),
        ("last pixel", last, [23, 1], b"g01"),
        ("run across a column seam", seam, [7, 2, 15], b"72?"),
        ("checkerboard 5x7", (xx + yy) % 2 == 1, [1] * 35, b"111" + b"0" * 32),
    ]


def rle_counts_from_string(s):
    """pycocotools' rleFrString"""
    counts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 0x1f) << (5 * k)
            more = bool(c & 0x20)
            p += 1
            k += 1
            if not more and (c & 0x10):
                x |= -1 << (5 * k)
        if len(counts) > 2:
            x += counts[-2]
        counts.append(x)
    return counts


def rle_decode(rle):
    """{'size', 'counts'} -> bool [H,W]: runs of 0 and 1 in turn, filled column by column"""
    H, W = rle["size"]
    counts = rle_counts_from_string(rle["counts"])
    assert all(c >= 0 for c in counts) and sum(counts) == H * W, counts[:10]
    flat = np.repeat(np.arange(len(counts)) % 2 == 1, counts)
    return flat.reshape(W, H).T


@pytest.mark.parametrize("name,mask,counts,string", _table(), ids=[t[0] for t in _table()])
def test_host_route_reproduces_the_worked_vectors(name, mask, counts, string):
    rle, = I.rle_encode(mask[None])
    assert rle == {"size": list(mask.shape), "counts": string}
    assert isinstance(rle["counts"], bytes)
    assert rle_counts_from_string(string) == counts                      # the decoder agrees with the table as well
    assert I.rle_encode(torch.from_numpy(mask)[None]) == [rle]           # CPU tensors take the same route


def _round_trip_cases():
    gen = np.random.default_rng(5)
    hole = np.zeros((100, 90), bool)
    hole[10:80, 20:70] = True
    hole[30:50, 35:60] = False                                           # a hole: long and short runs in turn, negative deltas
    u8 = (gen.random((40, 23)) < 0.3).astype(np.uint8) * 255
    return [("rectangle with a hole", hole), ("noise 0.5", gen.random((67, 131)) < 0.5),
            ("noise 0.02", gen.random((67, 131)) < 0.02), ("H = 1", gen.random((1, 300)) < 0.4),
            ("W = 1", gen.random((300, 1)) < 0.4), ("uint8 0 / 255", u8)]


@pytest.mark.parametrize("name,mask", _round_trip_cases(), ids=[c[0] for c in _round_trip_cases()])
def test_an_independent_decoder_round_trips_the_host_route(name, mask):
    rle, = I.rle_encode(mask[None])
    assert rle["size"] == list(mask.shape)
    assert np.array_equal(rle_decode(rle), mask != 0)
    if name == "rectangle with a hole":                                  # a delta below zero really occurs
        counts = rle_counts_from_string(rle["counts"])
        assert any(counts[i] < counts[i - 2] for i in range(3, len(counts)))


def test_batches_and_bad_shapes():
    gen = np.random.default_rng(6)
    masks = gen.random((5, 17, 9)) < 0.3
    assert I.rle_encode(masks) == [I.rle_encode(m[None])[0] for m in masks]
    assert I.rle_encode(np.zeros((0, 4, 4), bool)) == []
    with pytest.raises(ValueError):
        I.rle_encode(np.zeros((4, 4), bool))
    with pytest.raises(ValueError):
        I.rle_encode(torch.zeros(4, 4, dtype=torch.bool))


def test_encode_mask_results_keeps_the_structure():
    gen = np.random.default_rng(7)
    segms = [[gen.random((12, 15)) < 0.5 for _ in range(k)] for k in (2, 0, 3)]
    enc = I.encode_mask_results(segms)
    assert [len(c) for c in enc] == [2, 0, 3]
    for cls, cls_enc in zip(segms, enc):
        for m, r in zip(cls, cls_enc):                                   # per-class order
            assert r["size"] == [12, 15] and np.array_equal(rle_decode(r), m)
    scores = [[0.9, 0.8], [], [0.7, 0.6, 0.5]]
    out = I.encode_mask_results((segms, scores))
    assert isinstance(out, tuple) and out[0] == enc and out[1] is scores
    again = I.encode_mask_results(enc)                                   # RLE dicts pass through untouched
    assert again == enc and all(a is b for ca, cb in zip(again, enc) for a, b in zip(ca, cb))
    mixed = I.encode_mask_results([[enc[0][0], segms[0][1]], [], []])
    assert mixed[0] == enc[0]


def _seg_inputs():
    gen = torch.Generator().manual_seed(4)
    logits = torch.randn(5, 3, 28, 28, generator=gen) * 3
    xy = torch.rand(5, 2, generator=gen) * 100
    dets = torch.cat((xy, xy + 20 + torch.rand(5, 2, generator=gen) * 80, torch.rand(5, 1, generator=gen)), 1)
    return logits, dets, torch.tensor([2, 0, 2, 1, 2])


def test_get_seg_masks_encode_rle_on_cpu_tensors():
    logits, dets, labels = _seg_inputs()
    args = (logits, dets, labels, 3, (200, 333, 3), 1.0, True)
    bitmaps = I.get_seg_masks(*args)
    got = I.get_seg_masks(*args, encode_rle=True)
    assert got == I.encode_mask_results(bitmaps)
    assert [len(c) for c in got] == [1, 1, 3] and got[2][0]["size"] == [200, 333]
    assert np.array_equal(rle_decode(got[2][1]), bitmaps[2][1])
    assert all(isinstance(m, np.ndarray) for c in I.get_seg_masks(*args, encode_rle=False) for m in c)   # the default stays
    assert I.get_seg_masks(logits[:0], dets[:0], labels[:0], 3, (200, 333, 3), 1.0, True, encode_rle=True) == [[], [], []]


def test_levels_cannot_be_run_length_encoded():
    logits, dets, labels = _seg_inputs()
    with pytest.raises(ValueError):
        I.get_seg_masks(logits, dets, labels, 3, (200, 333, 3), 1.0, True, mask_thr_binary=-1, encode_rle=True)
    levels = I.get_seg_masks(logits, dets, labels, 3, (200, 333, 3), 1.0, True, mask_thr_binary=-1)
    assert levels[2][0].dtype == np.uint8
