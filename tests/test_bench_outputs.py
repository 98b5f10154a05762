"""bench.py --dump-outputs / --full: the flattening and sampling of a step's outputs on the CPU, and on the GPU the dump of
one reduced-size headline step (every array written, float32 / float64, identical from the same seed)."""
import os

import numpy as np
import pytest
import torch

import bench


def test_dump_outputs_flattens_samples_and_casts(tmp_path):
    big = torch.arange(3 * bench.DUMP_ARRAY_ELEMS, dtype=torch.float32).reshape(3, -1)
    keep = dict(labels=dict(boxes=[torch.tensor([[1, 2, 3, 4]], dtype=torch.int64)], counts=[[2, 3], [1]], mask=[np.ones((2, 5), np.uint8)],
                            maps=(big.to(torch.bfloat16), torch.zeros(2, dtype=torch.float64)), losses={}, note="text", none=None),
                backbone=dict(last_feat=big, attns=[object()], feature=(torch.ones(2, 3),), outputs_class=torch.zeros(1, 4)))
    written = bench.dump_outputs(keep, str(tmp_path))
    assert sorted(written) == sorted(f[:-4] for f in os.listdir(tmp_path))
    assert set(written) == {"labels.boxes.0", "labels.counts.0", "labels.counts.1", "labels.mask.0", "labels.maps.0", "labels.maps.1",
                            "backbone.last_feat", "backbone.feature.0", "backbone.outputs_class"}
    load = lambda n: np.load(tmp_path / (n + ".npy"))
    assert load("labels.boxes.0").dtype == np.float64 and load("labels.boxes.0").tolist() == [[1, 2, 3, 4]]
    assert load("labels.counts.0").tolist() == [2, 3] and load("labels.mask.0").dtype == np.float32
    assert load("labels.maps.1").dtype == np.float64
    # above the cap: a fixed sample of the flat elements -- the same indices on every call, so two dumps compare one to one
    s = load("backbone.last_feat")
    assert s.dtype == np.float32 and s.shape == (bench.DUMP_ARRAY_ELEMS,) and written["backbone.last_feat"] == list(big.shape)
    idx = s.astype(np.int64)                                # (the values ARE the flat indices: arange)
    assert (np.diff(idx) >= 0).all() and idx.max() > 2 * bench.DUMP_ARRAY_ELEMS and len(np.unique(idx)) > 0.8 * len(idx)
    bench.dump_outputs(keep, str(tmp_path / "again"))
    assert np.array_equal(s, np.load(tmp_path / "again" / "backbone.last_feat.npy"))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path) if f.endswith(".npy")) <= 64e6


def test_dump_outputs_stays_below_the_size_limit_with_many_arrays(tmp_path):
    keep = dict(labels=[torch.zeros(40000, dtype=torch.int64) for _ in range(400)], backbone=None)
    bench.dump_outputs(keep, str(tmp_path))
    assert sum(os.path.getsize(tmp_path / f) for f in os.listdir(tmp_path)) <= 64e6


@pytest.mark.gpu
def test_step_outputs_are_dumped_and_repeat_from_the_same_seed(tmp_path, monkeypatch):
    """One headline step at a reduced size (512^2, 8 blocks; more than one image, every stage of the chain) with step.keep
    set, as `bench.py --dump-outputs` runs it without the roll-out check: the labels and the backbone's outputs are all
    written (the backbone's finite) and bitwise equal when the step is repeated from the same seed."""
    monkeypatch.setattr(bench, "CFG", dict(bench.CFG, img=512, depth=8))
    step = bench.build(torch.device("cuda", 0), "fast", check_rollout=False)
    step.keep = {}
    dumps = []
    with torch.no_grad():
        for k in range(2):
            torch.manual_seed(11)
            res = step()
            assert step.keep["labels"] is res and step.head.rollout_check is False
            dumps.append(bench.dump_outputs(step.keep, str(tmp_path / str(k))))
    names = set(dumps[0])
    assert names == set(dumps[1])
    for want in ("labels.pseudo_gt_bboxes.0", "labels.pseudo_gt_bboxes.1", "labels.pseudo_gt_masks.1", "labels.map_cos_fg.0",
                 "labels.mask_points_coords.1", "backbone.last_feat", "backbone.feature.0", "backbone.outputs_class",
                 "backbone.outputs_coord"):
        assert want in names, (want, sorted(names))
    assert dumps[0]["backbone.last_feat"] == [2, 1 + 32 * 32, bench.CFG["embed_dim"]]
    for n in names:
        a, b = (np.load(tmp_path / str(k) / (n + ".npy")) for k in range(2))
        assert a.dtype in (np.float32, np.float64), n
        assert not n.startswith("backbone.") or np.isfinite(a).all(), n
        assert np.array_equal(a, b, equal_nan=True), n
    assert np.load(tmp_path / "0" / "backbone.last_feat.npy").std() > 0
