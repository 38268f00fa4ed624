"""The host side of the segmentation scores (maskfusion_amd.eval: build_lut, match_objects, seg_metrics, default_radius,
read_segmentation_run), fed with counts from the numpy restatement of the definitions (tests/seg_restatement.py).  No GPU."""
import itertools
import os

import numpy as np
import pytest

import seg_restatement as sr
from maskfusion_amd import eval as ev


# ---------------------------------------------------------------- look-up tables ----------------------------------------------------------------
def test_lut_construction():
    lut, ids = ev.build_lut([7, 3, 200, 3])
    assert ids == [0, 3, 7, 200]                                  # ascending, raw 0 is class 0 whether it occurs or not
    assert lut[0] == 0 and lut[3] == 1 and lut[7] == 2 and lut[200] == 3
    assert (np.delete(lut, ids) == 255).all()                     # what does not occur is void
    lut, ids = ev.build_lut(np.array([0, 1, 2, 255], np.uint8), void=255)
    assert ids == [0, 1, 2] and lut[255] == 255
    lut, ids = ev.build_lut([0, 5, 255], also_background=(255,))
    assert ids == [0, 5] and lut[255] == 0 and lut[5] == 1
    flags = np.zeros(256, np.int64)
    flags[[4, 9]] = 12
    assert ev.build_lut(flags)[1] == [0, 4, 9]                    # 256 counts by value
    assert len(ev.build_lut(np.arange(64))[1]) == 64
    assert len(ev.build_lut(np.arange(1, 64))[1]) == 64           # 63 values and the background
    with pytest.raises(ValueError, match="65 distinct"):
        ev.build_lut(np.arange(65))
    assert len(ev.build_lut(np.arange(65), void=64)[1]) == 64     # the void value is no class
    with pytest.raises(ValueError):
        ev.build_lut([1], void=0)


# ---------------------------------------------------------------- the assignment ----------------------------------------------------------------
def _seq_iou(c, g, e):
    c = c.astype(np.int64).sum(0)
    inter = c[g, e]
    union = c[g].sum() + c[:, e].sum() - inter
    return inter / union if union else 0.0


def _brute_force(c):
    """the largest sum of sequence IoUs over all one-to-one matchings of the objects (classes >= 1)"""
    n_gt, n_est = c.shape[1:]
    gs, es = list(range(1, n_gt)), list(range(1, n_est))
    if len(gs) > len(es):
        return max(sum(_seq_iou(c, g, e) for g, e in zip(p, es)) for p in itertools.permutations(gs, len(es)))
    return max(sum(_seq_iou(c, g, e) for g, e in zip(gs, p)) for p in itertools.permutations(es, len(gs)))


@pytest.mark.parametrize("n_gt,n_est", [(2, 2), (4, 4), (7, 7), (7, 4), (3, 7), (1, 5), (5, 1)])
def test_assignment_matches_brute_force(n_gt, n_est):
    rng = np.random.default_rng(n_gt * 10 + n_est)
    for _ in range(5):
        c = rng.integers(0, 50, (3, n_gt, n_est)).astype(np.uint32)
        c[rng.random(c.shape) < 0.3] = 0
        pair = ev.match_objects(c)
        assert pair.dtype == np.uint8 and pair.shape == (n_gt,) and pair[0] == 0           # background is pinned
        used = [int(e) for e in pair[1:] if e != 255]
        assert len(used) == len(set(used)) and 0 not in used
        total = sum(_seq_iou(c, g, int(pair[g])) for g in range(1, n_gt) if pair[g] != 255)
        assert abs(total - _brute_force(c)) < 1e-12
        for g in range(1, n_gt):
            if pair[g] != 255:
                assert c[:, g, pair[g]].sum() > 0                                           # no pair without a common pixel


def test_zero_intersection_pairs_stay_unmatched_and_background_is_pinned():
    c = np.zeros((2, 3, 3), np.uint32)
    c[:, 0, 1] = 500          # the estimate's model 1 lies wholly on the ground truth's background
    c[:, 1, 0] = 40           # object 1 is wholly background in the estimate
    c[:, 2, 2] = 30
    c[:, 0, 0] = 1
    assert ev.match_objects(c).tolist() == [0, 255, 2]
    res = ev.seg_metrics(c, lambda pair: np.zeros((2, 3, 4), np.uint32), gt_ids=[0, 10, 20], est_ids=[0, 7, 9])
    o1, o2 = res["objects"]
    assert o1 == {"gt_id": 10, "model_id": None, "frames": 2, "iou": 0.0, "J": 0.0, "P": 0.0, "R": 0.0, "F": 0.0, "JF": 0.0}      # unmatched: 0 everywhere
    assert o2["model_id"] == 9 and o2["iou"] == 1.0 and o2["J"] == 1.0
    assert res["summary"]["unmatched_models"] == [7] and res["summary"]["matched"] == 1 and res["summary"]["objects"] == 2
    assert res["summary"]["background_iou"] == 2 / (2 + 1000 + 80)
    assert res["summary"]["iou"] == 0.5 and res["summary"]["J"] == 0.5


# ---------------------------------------------------------------- P, R, F and the frame means ----------------------------------------------------------------
def _metrics_one_object(counts_fg, rows):
    """one object matched to one model over len(rows) frames: counts_fg[f] = (inter, gt only, est only)"""
    n = len(rows)
    c = np.zeros((n, 2, 2), np.uint32)
    for f, (i, g_only, e_only) in enumerate(counts_fg):
        c[f, 1, 1], c[f, 1, 0], c[f, 0, 1], c[f, 0, 0] = i, g_only, e_only, 100
    b = np.zeros((n, 2, 4), np.uint32)
    b[:, 1] = rows
    return ev.seg_metrics(c, lambda pair: b)["objects"][0]


def test_zero_denominator_rules():
    # frame 0: no estimate boundary (P = 0 / 0 -> 0), R = 2 / 4;  F = 2 * 0 * .5 / .5 = 0
    # frame 1: no ground-truth boundary (R = 0 / 0 -> 0);         F = 0
    # frame 2: boundaries on both sides, no hits: P + R = 0 ->    F = 0
    # frame 3: P = 3 / 4, R = 1 / 2:                              F = 2 * .75 * .5 / 1.25 = .6
    o = _metrics_one_object([(10, 0, 0)] * 4, [(0, 0, 4, 2), (5, 5, 0, 0), (6, 0, 7, 0), (4, 3, 2, 1)])
    assert o["frames"] == 4
    assert o["P"] == (0 + 1 + 0 + 0.75) / 4 and o["R"] == (0.5 + 0 + 0 + 0.5) / 4
    assert abs(o["F"] - 0.6 / 4) < 1e-15 and o["J"] == 1.0 and abs(o["JF"] - (1.0 + 0.6 / 4) / 2) < 1e-15
    # a frame without a common pixel: J = 0 / 12 = 0
    o = _metrics_one_object([(0, 5, 7), (10, 0, 0)], [(1, 1, 1, 1), (1, 1, 1, 1)])
    assert o["J"] == 0.5 and o["P"] == o["R"] == o["F"] == 1.0 and o["JF"] == 0.75 and o["iou"] == 10 / 22


def test_object_absent_from_some_frames_is_averaged_over_the_others():
    # present in frames 0 and 2 (J = 1/2 and 1), absent from frame 1, where the model claims 9 pixels of background
    o = _metrics_one_object([(10, 10, 0), (0, 0, 9), (8, 0, 0)], [(4, 4, 4, 2), (3, 0, 0, 0), (4, 2, 4, 4)])
    assert o["frames"] == 2
    assert o["J"] == (0.5 + 1.0) / 2
    assert o["P"] == (1.0 + 0.5) / 2 and o["R"] == (0.5 + 1.0) / 2
    assert abs(o["F"] - (2 / 3 + 2 / 3) / 2) < 1e-15
    assert o["iou"] == 18 / (18 + 10 + 9)         # the sequence IoU counts every frame


def test_metrics_from_restated_counts_of_a_drawn_scene():
    """two objects drawn by hand, one model too many: every number worked out from the restatement's counts"""
    gt = np.zeros((2, 20, 30), np.uint8)
    est = np.zeros((2, 20, 30), np.uint8)
    gt[:, 2:10, 2:12], gt[0, 12:18, 15:25] = 5, 9          # object 9 only in frame 0
    est[:, 2:10, 4:14], est[:, 12:18, 15:25], est[1, 0:2, 20:30] = 3, 1, 8
    (le, est_ids), (lg, gt_ids) = ev.build_lut(np.unique(est)), ev.build_lut(np.unique(gt))
    assert est_ids == [0, 1, 3, 8] and gt_ids == [0, 5, 9]
    counts = sr.confusion(est, gt, le, lg, 4, 3)
    res = ev.seg_metrics(counts, lambda pair: sr.boundary(est, gt, le, lg, 3, pair, 2), gt_ids, est_ids)
    assert res["pair"].tolist() == [0, 2, 1]
    a, b = res["objects"]
    assert (a["gt_id"], a["model_id"], a["frames"]) == (5, 3, 2) and (b["gt_id"], b["model_id"], b["frames"]) == (9, 1, 1)
    assert a["iou"] == a["J"] == 64 / 96                   # 8 x 8 common, 8 x 12 union, in both frames
    assert b["J"] == 1.0 and b["iou"] == 60 / 120          # frame 1: the model stays, the object is gone
    assert b["P"] == b["R"] == b["F"] == 1.0
    # object 5: 8 x 10 rectangles two pixels apart along x, radius 2: the whole boundary is within reach of the other
    assert a["P"] == a["R"] == 1.0
    assert res["summary"]["unmatched_models"] == [8] and res["summary"]["matched"] == 2


def test_default_radius():
    assert ev.default_radius(640, 480) == 6
    assert ev.default_radius(1280, 960) == 13
    assert ev.default_radius(64, 48) == 1
    assert ev.default_radius(4000, 3000) == 16             # clamped


# ---------------------------------------------------------------- file pairing ----------------------------------------------------------------
def _png(path, a):
    from PIL import Image
    Image.fromarray(np.ascontiguousarray(a, np.uint8), "L").save(str(path))


@pytest.mark.parametrize("start", [0, 1])
def test_file_pairing(tmp_path, start):
    est_dir, gt_dir = tmp_path / "out", tmp_path / "seq"
    est_dir.mkdir()
    gt_dir.mkdir()
    for i in range(5):                                      # frames 0..4 -> files start..start + 4; frame k's mask is all k + 1
        _png(gt_dir / f"Mask{i + start:04d}.png", np.full((6, 8), i + 1))
    for t in (2, 3, 5):                                     # the frame processed at tick t is frame t - 1
        _png(est_dir / f"Segmentation{t}.png", np.full((6, 8), 10 * t))
    est, gt, ticks = ev.read_segmentation_run(str(est_dir), str(gt_dir))
    assert ticks == [2, 3, 5] and est.shape == gt.shape == (3, 6, 8)
    assert est[:, 0, 0].tolist() == [20, 30, 50] and gt[:, 0, 0].tolist() == [2, 3, 5]
    # a segmentation image without a mask file
    _png(est_dir / "Segmentation6.png", np.zeros((6, 8)))
    with pytest.raises(ValueError, match=r"Segmentation6\.png.*Mask%04d" % (5 + start)):
        ev.read_segmentation_run(str(est_dir), str(gt_dir))
    os.remove(est_dir / "Segmentation6.png")
    # ... and one of another size
    _png(est_dir / "Segmentation4.png", np.zeros((6, 9)))
    with pytest.raises(ValueError, match=r"Segmentation4\.png.*9 x 6.*Mask%04d.*8 x 6" % (3 + start)):
        ev.read_segmentation_run(str(est_dir), str(gt_dir))


def test_file_pairing_needs_files(tmp_path):
    (tmp_path / "out").mkdir()
    (tmp_path / "seq").mkdir()
    with pytest.raises(ValueError, match="no Segmentation"):
        ev.read_segmentation_run(str(tmp_path / "out"), str(tmp_path / "seq"))
    _png(tmp_path / "out" / "Segmentation2.png", np.zeros((4, 4)))
    with pytest.raises(ValueError, match="no Mask"):
        ev.read_segmentation_run(str(tmp_path / "out"), str(tmp_path / "seq"))
    for i in (1, 2):                                    # first index 1: tick 2 is frame 1 is file 2
        _png(tmp_path / "seq" / f"Other{i:04d}.pgm", np.full((4, 4), i))
    est, gt, ticks = ev.read_segmentation_run(str(tmp_path / "out"), str(tmp_path / "seq"), prefix="Other")
    assert ticks == [2] and (gt == 2).all()
