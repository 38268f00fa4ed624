"""The host side of the registration without a start (maskfusion_amd.eval): voxel_subsample against a Python loop, the RANSAC stage on
synthetic correspondences, register_global with the device calls replaced by the numpy restatements, the command's flags.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import global_scene as gs  # noqa: E402
import register_restatement as rr  # noqa: E402
from maskfusion_amd import eval as ev  # noqa: E402


def test_voxel_subsample_against_a_loop():
    rng = np.random.default_rng(0)
    pts = rng.uniform(-1, 1, (3000, 3)).astype(np.float32)
    pts[::97] = np.nan
    pts[5] = [np.inf, 0, 0]
    pts[100:110] = pts[50]                                  # copies: the first stays
    for voxel in (0.25, 0.1, 3.0):
        seen, want = set(), []
        for i, p in enumerate(pts.astype(np.float64)):
            if not np.isfinite(p).all():
                continue
            c = tuple(np.floor(p / voxel))
            if c not in seen:
                seen.add(c)
                want.append(i)
        got = ev.voxel_subsample(pts, voxel)
        assert got.dtype == np.int64 and got.tolist() == want
    assert ev.voxel_subsample(np.zeros((0, 3), np.float32), 0.1).shape == (0,)
    neg = np.array([[-0.01, 0, 0], [0.01, 0, 0], [-0.09, 0.05, 0.05]], np.float32)       # floor, not truncation: -0.01 and 0.01 are two cells
    assert ev.voxel_subsample(neg, 0.1).tolist() == [0, 1]
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError):
            ev.voxel_subsample(pts, bad)


def test_ransac_on_correspondences_with_outliers():
    rng = np.random.default_rng(1)
    T = gs.motion()
    src = rng.uniform(-1, 1, (200, 3))
    dst = src @ T[:3, :3].T + T[:3, 3]
    bad = rng.choice(200, 120, replace=False)                # 60 % outliers
    dst[bad] = rng.uniform(-3, 3, (120, 3))
    good = np.setdiff1d(np.arange(200), bad)
    res = ev.ransac_correspondences(src, dst, 0.01, hypotheses=4000, seed=3)
    dt, dr = rr.pose_error(res["T"], T)
    print("inliers", res["inliers"], "tested", res["tested"], "error", dt, dr)
    assert res["inliers"] == 80 and np.array_equal(np.flatnonzero(res["inlier_mask"]), good)
    assert dt < 1e-12 and dr < 1e-12                        # exact inliers: the best hypothesis and the re-fit are exact to rounding
    assert res["hypotheses"] == 4000 and 0 < res["tested"] < 4000          # the edge test drops the triples with an outlier
    again = ev.ransac_correspondences(src, dst, 0.01, hypotheses=4000, seed=3)
    assert np.array_equal(again["T"], res["T"]) and again["inliers"] == 80 and again["tested"] == res["tested"]
    other = ev.ransac_correspondences(src, dst, 0.01, hypotheses=4000, seed=4)
    assert other["tested"] != res["tested"] and other["inliers"] == 80
    # the edge test alone: every surviving triple keeps its lengths to 10 %
    assert ev.ransac_correspondences(src, 2.0 * src, 10.0, hypotheses=500, seed=0)["tested"] == 0
    # too few correspondences, or none that pass: no pose
    assert ev.ransac_correspondences(src[:2], dst[:2], 0.01)["T"] is None
    none = ev.ransac_correspondences(src[bad][:30], dst[bad][:30], 0.01, hypotheses=200, seed=0)
    assert none["T"] is None or none["inliers"] <= 4


def test_horn_batch_is_align_horn():
    rng = np.random.default_rng(2)
    src, dst = rng.normal(size=(50, 3, 3)), rng.normal(size=(50, 3, 3))
    dst[:25] = src[:25] @ gs.motion()[:3, :3].T + 1.0
    R, t = ev._horn_batch(src, dst)
    for k in range(50):
        T = ev.align_horn(src[k], dst[k])
        assert np.abs(T[:3, :3] - R[k]).max() < 1e-12 and np.abs(T[:3, 3] - t[k]).max() < 1e-12 and abs(np.linalg.det(R[k]) - 1) < 1e-12


def test_register_global_on_the_restatements(monkeypatch):
    """the asymmetric scene's exact image under 120 degrees and 3 m: the coarse pose lands in the basin for every seed used, the whole
    pipeline recovers the motion, and register() alone, from the identity, does not"""
    gs.patch(monkeypatch, ev)
    est, en, ref, rn, T = gs.exact_pair()
    res = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0)
    dt, dr = rr.pose_error(res["T"], T)
    ct, cr = rr.pose_error(res["coarse"]["T"], T)
    print("coarse", {k: v for k, v in res["coarse"].items() if k != "T"}, ct, np.degrees(cr), "final", dt, dr, res["iterations"])
    assert ct <= 1.5 * gs.VOXEL and np.degrees(cr) <= 5.0
    assert res["converged"] and dt < 1e-5 and dr < 1e-5 and res["radius"] == gs.VOXEL / 2
    assert res["coarse"]["mutual"] == res["coarse"]["correspondences"] >= ev.MIN_MUTUAL and res["coarse"]["inliers"] >= 50
    for seed in (1, 2):
        c = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=seed, refine=False)
        ct, cr = rr.pose_error(c["T"], T)
        assert c["reason"] == "not refined" and not c["converged"] and ct <= 1.5 * gs.VOXEL and np.degrees(cr) <= 5.0
    plain = ev.register(est, ref, gs.VOXEL / 2, ref_normals=rn, schedule=[1.5 * gs.VOXEL, 0.75 * gs.VOXEL, gs.VOXEL / 2])
    assert not plain["converged"] and rr.pose_error(plain["T"], T)[0] > 1.0
    # too few mutual matches: every est -> ref match is a correspondence
    c = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, refine=False, min_mutual=10 ** 9)
    assert c["coarse"]["correspondences"] > c["coarse"]["mutual"] and c["coarse"]["correspondences"] <= c["coarse"]["key_points"][0]
    # nothing to match: no pose, said so
    far = ev.register_global(est[:2], ref, gs.VOXEL, est_normals=en[:2], ref_normals=rn)
    assert not far["converged"] and "no coarse pose" in far["reason"] and np.array_equal(far["T"], np.eye(4)) and far["coarse"]["T"] is None
    for bad in (0.0, float("nan")):
        with pytest.raises(ValueError):
            ev.register_global(est, ref, bad)


def test_towards_centroid_moves_with_the_cloud():
    rng = np.random.default_rng(3)
    p, n = rng.normal(size=(200, 3)), rng.normal(size=(200, 3))
    T = gs.motion()
    a = ev._towards_centroid(p, n).astype(np.float64)
    b = ev._towards_centroid(p @ T[:3, :3].T + T[:3, 3], n @ T[:3, :3].T).astype(np.float64)
    assert np.abs(a @ T[:3, :3].T - b).max() < 1e-6 and (((p.mean(0) - p) * a).sum(1) >= 0).all()


def test_command_flag_errors(tmp_path, capsys):
    est = tmp_path / "est"
    est.mkdir()
    for args in (["--est", str(est), "--register-global"], ["--est", str(est), "--ref-cloud", "m.ply", "--register-global", "--init", "T.txt"],
                 ["--est", str(est), "--ref-cloud", "m.ply", "--register-global=0"], ["--est", str(est), "--ref-cloud", "m.ply", "--register-global=-1"],
                 ["--est", str(est), "--ref-cloud", "m.ply", "--register-global=x"], ["--est", str(est), "--ref", "a", "--register-seed", "3"],
                 ["--est", str(est), "--ref", "a", "--register-global", "--register-radius", "0.1,x"]):
        with pytest.raises(SystemExit) as e:
            ev.main(args)
        assert e.value.code == 2, args
    err = capsys.readouterr().err
    assert "--init" in err and "positive voxel" in err and "--register-seed needs" in err
    # it implies --register: the missing background cloud is met before any device work
    assert ev.main(["--est", str(est), "--ref-cloud", "model.ply", "--register-global"]) == 2
    assert "cloud-0.ply" in capsys.readouterr().err
