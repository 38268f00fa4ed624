"""The host side of the device hypothesis search (maskfusion_amd.eval.ransac_correspondences(device=True), register_global(ransac="device")) with
the device call replaced by its numpy restatement (tests/ransac_restatement.py), in the manner of global_scene.patch.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_scene as gs  # noqa: E402
import ransac_restatement as rs  # noqa: E402
import register_restatement as rr  # noqa: E402
from maskfusion_amd import eval as ev  # noqa: E402


def _patch(monkeypatch):
    calls = []

    def stand_in(src, dst, tri, inlier_distance, edge_tolerance):
        calls.append((len(src), len(tri)))
        return rs.device_stand_in(src, dst, tri, inlier_distance, edge_tolerance)
    monkeypatch.setattr(ev, "_pose_ransac_device", stand_in)
    return calls


def test_device_search_returns_the_documented_dictionary(monkeypatch):
    calls = _patch(monkeypatch)
    rng = np.random.default_rng(1)
    T = gs.motion()
    src = rng.uniform(-1, 1, (200, 3)).astype(np.float32)
    dst = (src.astype(np.float64) @ T[:3, :3].T + T[:3, 3])
    bad = rng.choice(200, 120, replace=False)                # 60 % outliers
    dst[bad] = rng.uniform(-3, 3, (120, 3))
    dst = dst.astype(np.float32)
    good = np.setdiff1d(np.arange(200), bad)
    res = ev.ransac_correspondences(src, dst, 0.01, hypotheses=4000, seed=3, device=True)
    assert calls == [(200, 4000)]
    assert set(res) == {"T", "inliers", "inlier_mask", "hypotheses", "tested"}
    assert res["inliers"] == 80 and res["inlier_mask"].dtype == bool and np.array_equal(np.flatnonzero(res["inlier_mask"]), good)
    assert res["hypotheses"] == 4000 and 0 < res["tested"] < 4000
    # the same draw as the host's, the same edge rule: the same triples are tested
    host = ev.ransac_correspondences(src, dst, 0.01, hypotheses=4000, seed=3)
    assert host["tested"] == res["tested"] and host["inliers"] == 80
    # T: align_horn on the device's mask
    assert np.array_equal(res["T"], ev.align_horn(src[good].astype(np.float64), dst[good].astype(np.float64)))
    dt, dr = rr.pose_error(res["T"], T)
    assert dt < 1e-6 and dr < 1e-6                           # dst is rounded to fp32
    again = ev.ransac_correspondences(src, dst, 0.01, hypotheses=4000, seed=3, device=True)
    assert np.array_equal(again["T"], res["T"]) and again["tested"] == res["tested"]
    # no pose: too few correspondences (the device is not asked), no triple passes
    assert ev.ransac_correspondences(src[:2], dst[:2], 0.01, device=True)["T"] is None and len(calls) == 2
    none = ev.ransac_correspondences(src, 2.0 * src, 10.0, hypotheses=500, seed=0, device=True)
    assert none["T"] is None and none["tested"] == 0 and none["inliers"] == 0 and not none["inlier_mask"].any()


def test_fewer_than_three_inliers_take_the_device_pose(monkeypatch):
    pose = np.hstack([np.eye(3), [[1.0], [2.0], [3.0]]])
    monkeypatch.setattr(ev, "_pose_ransac_device", lambda s, d, t, i, e: (np.zeros(len(t), np.uint8), np.full(len(t), 2, np.uint32), np.array([0, 2], np.int32),
                                                                          np.arange(len(s)) < 2, pose))
    res = ev.ransac_correspondences(np.zeros((5, 3)), np.ones((5, 3)), 0.1, hypotheses=7, device=True)
    assert np.array_equal(res["T"], np.vstack([pose, [0, 0, 0, 1]])) and res["inliers"] == 2 and res["tested"] == 7


def test_register_global_on_the_restated_device_search(monkeypatch):
    """the gates of the host search (tests/test_eval_global_host.py, tests/test_gpu_fpfh.py): coarse within 1.5 voxel and 5 degrees, final
    within 1e-5 m / rad"""
    gs.patch(monkeypatch, ev)
    calls = _patch(monkeypatch)
    est, en, ref, rn, T = gs.exact_pair()
    res = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, ransac="device")
    dt, dr = rr.pose_error(res["T"], T)
    ct, cr = rr.pose_error(res["coarse"]["T"], T)
    print("coarse", {k: v for k, v in res["coarse"].items() if k != "T"}, ct, np.degrees(cr), "final", dt, dr, res["iterations"])
    assert len(calls) == 1 and calls[0][1] == 20000
    assert ct <= 1.5 * gs.VOXEL and np.degrees(cr) <= 5.0
    assert res["converged"] and dt < 1e-5 and dr < 1e-5 and res["radius"] == gs.VOXEL / 2
    again = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, refine=False, ransac="device")
    assert again["reason"] == "not refined" and np.array_equal(again["T"], res["coarse"]["T"])
    host = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, refine=False)
    assert len(calls) == 2 and host["coarse"]["tested"] == res["coarse"]["tested"]
    with pytest.raises(ValueError):
        ev.register_global(est, ref, gs.VOXEL, ransac="gpu")


def test_the_driver_knows_redetect():
    from maskfusion_amd import cli
    assert cli.parse(["-redetect", "-ep", "-exportdir", "out"]) == {"-redetect": True, "-ep": True, "-exportdir": "out"}
