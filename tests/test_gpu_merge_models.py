"""Map merging above the kernel: mf_model_merge_map against the three public calls it is defined as (state digests, right away and three frames
later; the overflow), re-detection that keeps the new model's map (MaskFusion.redetectModels(merge=True)) and the join of two sessions
(python -m maskfusion_amd.merge), each held to the numpy restatement of tests/merge_restatement.py bit for bit.  Contexts are 160 x 120.  Runs on
the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import merge_restatement as mr  # noqa: E402
import redetect_scene as rsn  # noqa: E402
from test_gpu_inactive_models import F, H, W, _lived, drop, make, patch, spawn, step  # noqa: E402
from test_gpu_redetect import objects  # noqa: E402

pytestmark = pytest.mark.gpu


def cos_half():
    from maskfusion_amd import merge
    return float(merge.COS_HALF_RAD)


def info_tuple(m):
    i = m.info()
    return (i.id, i.class_id, i.confidence_threshold, i.is_static, i.age, m.getPose().tobytes())


# ---------------- mf_model_merge_map ----------------
def test_merge_map_leaves_the_bits_of_its_three_calls(hip):
    from maskfusion_amd import merge, synth
    from maskfusion_amd.api import MFError, Model
    a, b = _lived({}, 0), _lived({}, 0)
    try:
        assert a.stateDigest() == b.stateDigest()
        T = synth.make_pose(synth.rot_xyz(0.01, -0.02, 0.015), [0.002, -0.001, 0.0015])
        src = rsn.moved_records(patch(3000, seed=9), np.linalg.inv(T))
        ma, mb = Model(a, 1), Model(b, 1)
        before = info_tuple(ma)
        target = mb.downloadMap()
        assert ma.downloadMap().tobytes() == target.tobytes() and len(target) > 1000
        want, match, stats = mr.merge(target, src, T, 0.004, cos_half())
        assert stats[0] > 100 and stats[2] > 100 and stats[3] == 0 and len(want) <= 1 << 14      # it merges and appends, and it fits
        # A: the call.  B: its definition, by hand
        got = ma.mergeMap(src, T, radius=0.004)
        rec, by_hand, _ = merge.merge_maps(target, src, T, 0.004)
        mb.uploadMap(rec)
        assert got == by_hand == stats and rec.tobytes() == want.tobytes()
        assert ma.downloadMap().tobytes() == want.tobytes() and ma.lastCount() == len(target) + stats[2]
        assert info_tuple(ma) == before == info_tuple(mb)
        da, db = a.stateDigest(), b.stateDigest()
        assert da == db, sorted(k for k in da if da[k] != db.get(k))
        for k in (3, 4, 5):
            step(a, k)
            step(b, k)
        da, db = a.stateDigest(), b.stateDigest()
        assert da == db, sorted(k for k in da if da[k] != db.get(k))
        # the overflow: the merged map would not fit the model's 2^14 surfels -- refused, and the model is what it was
        held, count, digest = ma.downloadMap(), ma.lastCount(), a.stateDigest()
        far = patch(1 << 14, seed=10)
        far[:, 0] += 5.0
        with pytest.raises(MFError) as e:
            ma.mergeMap(far, None, radius=0.004)
        assert "code -1" in str(e.value) or "code -5" in str(e.value), str(e.value)
        assert ma.lastCount() == count and ma.downloadMap().tobytes() == held.tobytes() and a.stateDigest() == digest
        # the background takes a map as well, and an empty source changes nothing
        bg = Model(a, 0)
        t0 = bg.downloadMap()
        assert bg.mergeMap(t0[:0], None, radius=0.01) == [0, 0, 0, 0] and bg.downloadMap().tobytes() == t0.tobytes()
        some = t0[::7].copy()
        assert bg.mergeMap(some, None, radius=0.01) == mr.merge(t0, some, None, 0.01, cos_half())[2]
        assert bg.downloadMap().tobytes() == mr.merge(t0, some, None, 0.01, cos_half())[0].tobytes()
    finally:
        a.close()
        b.close()


# ---------------- re-detection that keeps the new map ----------------
def holed():
    """(the archived map: the object without a patch of 6 cm around one of its surfels, the new model's map: the whole object under the
    inverse motion, the number of surfels in the hole)"""
    obj, new, _ = objects()
    hole = np.linalg.norm(obj[:, :3] - obj[0, :3], axis=1) < 0.06
    assert 60 < hole.sum() < 0.05 * len(obj)
    return obj[~hole].copy(), new, int(hole.sum())


def context_with_inactive(archived, new_records):
    """tests/test_gpu_redetect.py's context, with `archived` as the map of the dropped id 5"""
    from maskfusion_amd import MaskFusion, synth
    mf = make(keepInactiveModels=1)
    spawn(mf, 5, 41, archived, age=30)
    drop(mf, 5)
    assert [i.id for i in mf.inactiveModels()] == [5] and mf.inactiveMap(0).tobytes() == archived.tobytes()
    i = spawn(mf, 6, 41, new_records, age=MaskFusion.REDETECT_MIN_AGE)
    mf.getModels()[i].overridePose(synth.make_pose(synth.rot_xyz(0.2, -0.1, 0.4), [0.1, 0.2, -0.3]))
    return mf


@pytest.mark.parametrize("merge", [True, False])
def test_redetection_keeps_what_the_new_model_saw(hip, monkeypatch, merge):
    from maskfusion_amd import redetect
    archived, new, n_hole = holed()
    seen = []
    real = redetect.match_model
    monkeypatch.setattr(redetect, "match_model", lambda *a, **k: seen.append(real(*a, **k)) or seen[-1])
    mf = context_with_inactive(archived, new)
    try:
        assert mf.redetectModels(merge=merge) == [(6, 5)] and len(seen) == 1 and seen[0]["accepted"]
        assert mf.modelIDs() == [0, 5] and mf.inactiveModels() == []
        m = mf.getModels()[1]
        got = m.downloadMap()
        assert m.getClassID() == 41 and m.isNonstatic() and m.info().age == 30
        if not merge:                                                # today's behaviour: the new map is dropped
            assert got.tobytes() == archived.tobytes()
            return
        r = seen[0]
        want, match, stats = mr.merge(archived, new, r["T"], r["voxel"] / 2.0, cos_half())
        print("hole", n_hole, "stats", stats, "voxel", r["voxel"])
        assert stats[2] >= n_hole // 2 and stats[0] + stats[1] > 0.9 * len(new) and stats[3] == 0
        assert got.tobytes() == want.tobytes() and len(got) == len(archived) + stats[2]
        # the hole is filled.  A surfel the archive lacked was appended, or merged into a target within the radius; a merged target stays in the
        # hull of itself and its sources, all within the radius of where it stood: a surfel of the merged map lies within twice the radius
        obj = objects()[0]
        hole = obj[np.linalg.norm(obj[:, :3] - obj[0, :3], axis=1) < 0.06]
        d = np.linalg.norm(hole[:, None, :3] - got[None, :, :3], axis=2).min(1)
        before = np.linalg.norm(hole[:, None, :3] - archived[None, :, :3], axis=2).min(1)
        assert d.max() < r["voxel"] < before.max()
    finally:
        mf.close()


def test_the_switch_carries_the_choice(hip):
    mf = make()
    try:
        mf.setEnableRedetection(True, merge=True)
        assert mf._redetect and mf._redetect_merge
        mf.setEnableRedetection(True)
        assert mf._redetect and not mf._redetect_merge               # the default stays "drop"
    finally:
        mf.close()


# ---------------- the join of two sessions ----------------
K, O = 4, 2            # A takes frames [0, K), B frames [K - O, 2 K - O)


def test_session_join(hip, tmp_path, capsys):
    from maskfusion_amd import MaskFusion, merge, synth
    from maskfusion_amd import eval as ev
    st = synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=True)
    frames = [st.frame(k)[:2] for k in range(2 * K - O + 1)]
    A, B = make(), make()
    merged = None
    try:
        for k in range(K):
            A.processFrame(*frames[k], timestamp=33333 * (k + 1))
        for k in range(K - O, 2 * K - O):
            B.processFrame(*frames[k], timestamp=33333 * (k + 1))
        pa, pb = str(tmp_path / "A.mfs"), str(tmp_path / "B.mfs")
        A.saveSession(pa, user=b"kept")
        B.saveSession(pb)
        map_a, map_b, tick_a, tick_b = A.getBackgroundModel().downloadMap(), B.getBackgroundModel().downloadMap(), A.getTick(), B.getTick()
        assert tick_a == tick_b >= K and len(map_a) > 5000 and len(map_b) > 5000
    finally:
        A.close()
        B.close()
    # B started at the identity in the camera frame of frame K - O, A in that of frame 0: b -> a is P_0^-1 P_(K-O)
    T = np.linalg.inv(st.gt_pose(0)) @ st.gt_pose(K - O)
    pt, po, pp = str(tmp_path / "T.txt"), str(tmp_path / "merged.mfs"), str(tmp_path / "merged.ply")
    np.savetxt(pt, T, fmt="%.17g")
    T = ev.read_transform(pt)
    capsys.readouterr()
    assert merge.main(["--a", pa, "--b", pb, "--init", pt, "-o", po, "--ply", pp]) == 0
    line = json.loads(capsys.readouterr().out.strip().splitlines()[-1])
    radius = merge.default_radius(map_a)
    want, match, stats = mr.merge(map_a, merge.rewrite_stamps(map_b, tick_a, tick_b), T, radius, cos_half())
    print(line, "restatement", stats)
    assert [line[k] for k in ("averaged", "confidence_only", "appended", "dropped")] == stats and sum(stats) == len(map_b)
    assert line["n_out"] == len(want) == len(map_a) + stats[2] and line["radius"] == radius and line["inlier_share"] is None and line["rmse"] is None
    assert stats[0] > 1000 and stats[2] > 100                        # the overlap merges, the rest of B's view is new
    assert MaskFusion.sessionInfo(po)["user"] == b"kept" and len(ev.read_ply(pp)) == len(want)
    try:
        merged = MaskFusion.loadSession(po)
        assert merged.getTick() == tick_a and merged.getBackgroundModel().downloadMap().tobytes() == want.tobytes()
        assert (want[:, 6:8] >= 1).all() and (want[:, 6:8] <= tick_a).all()
        merged.processFrame(*frames[K], timestamp=33333 * (K + 1))
        assert merged.getTick() == tick_a + 1 and merged.getBackgroundModel().lastCount() > 0
    finally:
        if merged is not None:
            merged.close()
