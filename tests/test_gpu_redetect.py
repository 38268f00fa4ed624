"""A returning object is recognised and gets its old id and map back (maskfusion_amd.redetect.match_model, MaskFusion.redetectModels): the
asymmetric scene of tests/global_scene.py at 0.5 m as the object, its exact image under a 120 degree motion as the new model, a look-alike
without the sphere and the box as the negative control (tests/redetect_scene.py).  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the
CPU-executed build."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redetect_scene as rsn  # noqa: E402
import register_restatement as rr  # noqa: E402
from test_gpu_inactive_models import drop, make, spawn  # noqa: E402

pytestmark = pytest.mark.gpu

_cache = {}


def objects():
    """(the object, its exact image: new -> old is motion(), the negative control under the same motion), built once; read-only"""
    if not _cache:
        obj = rsn.object_records()
        Ti = np.linalg.inv(rsn.motion())
        _cache["o"] = (obj, rsn.moved_records(obj, Ti), rsn.moved_records(rsn.negative_records(), Ti))
    return _cache["o"]


def context_with_5_inactive(new_records, new_class=41):
    """id 5 (class 41) archived, id 6 with `new_records` live at the age redetectModels() looks at and under a pose of its own"""
    from maskfusion_amd import MaskFusion, synth
    obj = objects()[0]
    mf = make(keepInactiveModels=1)
    spawn(mf, 5, 41, obj, age=30)
    drop(mf, 5)
    assert [i.id for i in mf.inactiveModels()] == [5] and mf.inactiveMap(0).tobytes() == obj.tobytes()
    i = spawn(mf, 6, new_class, new_records, age=MaskFusion.REDETECT_MIN_AGE)
    P_new = synth.make_pose(synth.rot_xyz(0.2, -0.1, 0.4), [0.1, 0.2, -0.3])
    mf.getModels()[i].overridePose(P_new)
    return mf, mf.getModels()[i].getPose()


def test_match_model_on_the_two_pairs(hip):
    from maskfusion_amd import redetect
    obj, new, neg = objects()
    assert 5500 <= len(obj) <= 6500
    pos = redetect.match_model(new, obj)
    dt, dr = rr.pose_error(pos["T"], rsn.motion())
    print("positive: share %.4f rmse %.3g error %.3g m %.3g rad voxel %.4f" % (pos["inlier_share"], pos["rmse"], dt, dr, pos["voxel"]))
    assert set(pos) == {"T", "inlier_share", "rmse", "accepted", "voxel", "converged", "reason", "coarse"}
    assert pos["accepted"] and pos["inlier_share"] >= redetect.MIN_SHARE and pos["rmse"] <= pos["voxel"] / 2 and dt < 1e-5 and dr < 1e-5
    assert abs(pos["voxel"] - redetect.VOXEL_FRACTION * np.linalg.norm(np.ptp(obj[:, :3].astype(np.float64), axis=0))) < 1e-12
    no = redetect.match_model(neg, obj)
    print("negative: share %.4f rmse %s accepted %s" % (no["inlier_share"], no["rmse"], no["accepted"]))
    assert not no["accepted"]
    assert not redetect.match_model(new[:2], obj)["accepted"] and not redetect.match_model(new, obj[:0])["accepted"]
    # reported, not gated: another sample of the object, 1 mm of noise, 70 % of its points
    noisy = redetect.match_model(rsn.noisy_records(np.linalg.inv(rsn.motion())), obj)
    dt, dr = rr.pose_error(noisy["T"], rsn.motion())
    print("noisy: share %.4f rmse %.3g accepted %s error %.3g m %.3g rad" % (noisy["inlier_share"], noisy["rmse"], noisy["accepted"], dt, dr))


def test_the_returning_object_gets_its_id_and_map_back(hip):
    obj, new, _ = objects()
    mf, P_new = context_with_5_inactive(new)
    try:
        assert mf.modelIDs() == [0, 6]
        assert mf.redetectModels() == [(6, 5)]
        assert mf.modelIDs() == [0, 5] and mf.inactiveModels() == []          # id 6 is gone for good: not kept
        m = mf.getModels()[1]
        assert m.downloadMap().tobytes() == obj.tobytes() and m.getClassID() == 41 and m.isNonstatic() and m.info().age == 30
        # the composed truth: o = T n and a surfel n is seen at P^-1 n, so P_old = T P_new
        T = rsn.motion()
        dt, dr = rr.pose_error(m.getPose(), T @ P_new)
        print("pose error %.3g m %.3g rad" % (dt, dr))
        assert dt < 1e-5 and dr < 1e-5
        # ... which says: the camera sees the old map where it saw the new one
        seen_new = (np.linalg.inv(P_new) @ np.c_[new[:, :3].astype(np.float64), np.ones(len(new))].T).T[:, :3]
        seen_old = (np.linalg.inv(m.getPose()) @ np.c_[obj[:, :3].astype(np.float64), np.ones(len(obj))].T).T[:, :3]
        assert np.abs(seen_new - seen_old).max() < 1e-5
        assert mf.redetectModels() == []
    finally:
        mf.close()


def test_a_look_alike_is_not_merged(hip):
    _, _, neg = objects()
    mf, _ = context_with_5_inactive(neg)
    try:
        assert mf.redetectModels() == []
        assert mf.modelIDs() == [0, 6] and [i.id for i in mf.inactiveModels()] == [5]
    finally:
        mf.close()


def test_only_models_of_the_age_and_the_class_are_compared(hip, monkeypatch):
    from maskfusion_amd import MaskFusion, redetect
    _, new, _ = objects()
    calls = []
    real = redetect.match_model
    monkeypatch.setattr(redetect, "match_model", lambda *a, **k: calls.append(1) or real(*a, **k))
    mf, _ = context_with_5_inactive(new, new_class=42)
    try:
        assert mf.redetectModels() == [] and calls == []                      # another class: never compared
        assert mf.modelIDs() == [0, 6] and [i.id for i in mf.inactiveModels()] == [5]
    finally:
        mf.close()
    mf, _ = context_with_5_inactive(new)
    try:
        assert mf.redetectModels(min_age=MaskFusion.REDETECT_MIN_AGE + 1) == [] and calls == []     # not its age
        mf.setEnableRedetection(True)
        assert mf.redetectModels(min_age=MaskFusion.REDETECT_MIN_AGE) == [(6, 5)] and calls == [1]
    finally:
        mf.close()
