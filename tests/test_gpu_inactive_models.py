"""The inactive list of a context ("keepInactiveModels", mf_inactive_*, mf_reactivate_model; include/maskfusion_amd.h "Inactive models"): what is
kept (line 702 of Core/MaskFusion.cpp at its two thresholds), that the archive is the map mf_download_map returned, that a reactivation leaves
the bits of the five public calls it is defined as, the jump rule's way in, and sessions.  Contexts are 160 x 120; object maps come in
through uploadMap.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import redetect_scene as rsn  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, F = 160, 120, 132.0
EINVAL = "code -1:"


def make(**params):
    from maskfusion_amd import MaskFusion
    mf = MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 16, numOSurfels=1 << 14, enableMultipleModels=True,
                    modelSpawnOffset=1000, trackAllModels=False)
    for k, v in params.items():
        mf.setParam(k, v)
    return mf


_frames = {}


def frame(k):
    from maskfusion_amd import synth
    if not _frames:
        st = synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=True)
        for i in range(8):
            _frames[i] = st.frame(i)[:2]
    return _frames[k]


def step(mf, k):
    rgb, depth = frame(k)
    mf.processFrame(rgb, depth, timestamp=33333 * (k + 1))


def patch(n, seed=0):
    """n surfels on a slanted patch a metre and a half in front of the first camera, as downloadMap records"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(-0.2, 0.2, (n, 2))
    p = np.stack([uv[:, 0], uv[:, 1], 1.5 + 0.3 * uv[:, 0]], 1).astype(np.float32)
    nm = np.tile(np.array([0.3, 0.0, -1.0], np.float32) / np.float32(np.sqrt(1.09)), (n, 1))
    return rsn.records(p, nm, confidence=10.0 + rng.uniform(0, 1, n).astype(np.float32))


def spawn(mf, id, cls, rec, age=None):
    """appends an object model with that map; age: Model::age with the confidence threshold the ramp of processFrame gives it"""
    from maskfusion_amd.api import Model
    mf._chk(mf._L.mf_spawn_object_model(mf._h, id, cls))
    i = len(mf.modelIDs()) - 1
    Model(mf, i).uploadMap(rec)
    if age is not None:
        mf._chk(mf._L.mf_model_set_age(mf._h, i, age, 0.0))
        mf._chk(mf._L.mf_update_object_params(mf._h))            # confThr = min(4.5, age / 25.0f)
    return i


def drop(mf, id):
    mf._chk(mf._L.mf_drop_model(mf._h, mf.modelIDs().index(id)))


def info_tuple(i):
    return (i.id, i.class_id, i.surfels, i.age, i.confidence_threshold, i.tick, tuple(i.pose))


def refused(call, text=""):
    from maskfusion_amd.api import MFError
    with pytest.raises(MFError) as e:
        call()
    assert EINVAL in str(e.value) and text in str(e.value), str(e.value)


# ---------------- 1. default off ----------------
def test_nothing_is_kept_by_default(hip):
    mf = make()
    try:
        assert [mf.getParam(k) for k in ("keepInactiveModels", "enableSmartModelDelete", "modelKeepMinSurfels")] == [0, 1, 4000]
        assert mf.getParam("modelKeepConfThreshold") == float(np.float32(0.3))
        spawn(mf, 5, 41, patch(5000), age=30)
        drop(mf, 5)
        assert mf.inactiveModels() == [] and mf.modelIDs() == [0]
        for call in (lambda: mf.inactiveMap(0), lambda: mf.discardInactive(0), lambda: mf.reactivateModel(0), lambda: mf.discardInactive(-1),
                     lambda: mf._chk(mf._L.mf_inactive_info(mf._h, 0, C.byref(C.c_int32(0)))),
                     lambda: mf._chk(mf._L.mf_inactive_map_dev(mf._h, 0, C.byref(C.c_void_p()), C.byref(C.c_uint32())))):
            refused(call, "no such inactive model")
    finally:
        mf.close()


# ---------------- 2. line 702 ----------------
def test_the_rule_of_line_702_at_its_thresholds(hip):
    mf = make(keepInactiveModels=1)
    try:
        kept = lambda: [i.id for i in mf.inactiveModels()]          # noqa: E731
        spawn(mf, 1, 41, patch(3999), age=8)                         # 8 / 25 > 0.3, one surfel short
        drop(mf, 1)
        assert kept() == []
        spawn(mf, 2, 41, patch(4000), age=8)                         # >= 4000
        drop(mf, 2)
        assert kept() == [2]
        thr = float(np.float32(7) / np.float32(25))
        mf.setParam("modelKeepConfThreshold", thr)
        assert mf.getParam("modelKeepConfThreshold") == thr
        spawn(mf, 3, 41, patch(4000), age=7)                         # the threshold itself: strictly greater is asked
        assert mf.getModels()[1].getConfidenceThreshold() == thr
        drop(mf, 3)
        assert kept() == [2]
        spawn(mf, 4, 41, patch(4000), age=8)
        drop(mf, 4)
        assert kept() == [2, 4]
        spawn(mf, 6, 41, patch(10))                                  # age 0
        drop(mf, 6)
        assert kept() == [2, 4]
        mf.setParam("enableSmartModelDelete", 0)
        spawn(mf, 7, 42, patch(10))
        drop(mf, 7)
        assert kept() == [2, 4, 7]
        i7 = mf.inactiveModels()[2]
        assert (i7.surfels, i7.age, i7.class_id) == (10, 0, 42) and mf.inactiveMap(2).shape == (10, 12)
        spawn(mf, 8, 42, np.zeros((0, 12), np.float32))              # an empty map is a map
        drop(mf, 8)
        assert kept() == [2, 4, 7, 8] and mf.inactiveMap(3).shape == (0, 12)
        mf.discardInactive(1)                                        # the later entries move up
        assert kept() == [2, 7, 8]
        mf.discardInactive(0)
        assert kept() == [7, 8] and mf.inactiveMap(0).shape == (10, 12)
    finally:
        mf.close()


# ---------------- 3. archive contents ----------------
def _lived(form, keep):
    """a context whose model 5 has lived through two frames in `form`"""
    mf = make(keepInactiveModels=keep, enableSmartModelDelete=0, **form)
    step(mf, 0)
    spawn(mf, 5, 41, patch(5000, seed=3), age=30)
    step(mf, 1)
    step(mf, 2)
    return mf


@pytest.mark.parametrize("form", [dict(), dict(bigMapElements=0, inPlaceElements=0)], ids=["dense", "runs"])
def test_the_archive_is_the_downloaded_map(hip, form):
    a, b = _lived(form, 0), _lived(form, 1)
    try:
        m = a.getModels()[1]
        before = a.getParam("densifyCount")
        want = m.downloadMap()                                       # (compacts a map kept as runs)
        runs = a.getParam("densifyCount") > before
        assert runs == bool(form), "the second form must leave the map as runs, the first must not"
        wi, wp = m.info(), m.getPose()
        tick = b.getTick()
        before = b.getParam("densifyCount")
        drop(b, 5)                                                   # ... without a download first: the keep compacts it itself
        assert (b.getParam("densifyCount") > before) == runs
        (info,) = b.inactiveModels()
        got = b.inactiveMap(0)
        assert 0 < len(want) and got.shape == want.shape and got.tobytes() == want.tobytes()
        assert (info.id, info.class_id, info.surfels, info.age, info.confidence_threshold, info.tick) == (5, 41, len(want), wi.age, wi.confidence_threshold, tick)
        assert np.array_equal(np.array(info.pose, np.float32).reshape(4, 4).T, wp.astype(np.float32))
        # the device pointer: a cloud the library's own nearest-neighbour search finds every record's position in, at distance 0
        import torch
        from maskfusion_amd.lib import load, torch_device
        L, dev = load(), torch_device()
        p, n = C.c_void_p(), C.c_uint32()
        b._chk(b._L.mf_inactive_map_dev(b._h, 0, C.byref(p), C.byref(n)))
        assert n.value == len(want) and p.value
        q = torch.from_numpy(np.ascontiguousarray(want[:, :3])).to(dev)
        need = C.c_uint64(0)
        assert L.mf_cloud_nn_workspace(n.value, C.byref(need)) == 0
        ws = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
        dist = torch.empty(n.value, dtype=torch.float32, device=dev)
        idx = torch.empty(n.value, dtype=torch.int32, device=dev)
        assert L.mf_cloud_nn_dev(p.value, 12, n.value, q.data_ptr(), 3, n.value, None, 0.01, dist.data_ptr(), idx.data_ptr(), ws.data_ptr(), int(need.value),
                                 None) == 0
        assert (dist.cpu().numpy() == 0).all() and np.array_equal(want[idx.cpu().numpy(), :3], want[:, :3])
    finally:
        a.close()
        b.close()


# ---------------- 4. reactivation ----------------
def test_a_reactivation_leaves_the_bits_of_its_five_calls(hip, tmp_path):
    from maskfusion_amd.api import Model
    a, b = _lived({}, 1), _lived({}, 0)
    try:
        assert a.stateDigest() == b.stateDigest()
        drop(a, 5)
        drop(b, 5)
        (info,) = a.inactiveModels()
        rec = a.inactiveMap(0)
        step(a, 3)
        step(b, 3)
        assert a.stateDigest() == b.stateDigest()                    # keeping changed nothing the frames see
        # the id is taken: refused, and the entry stays
        spawn(a, 5, 41, patch(10))
        refused(lambda: a.reactivateModel(0), "model id in use")
        assert [i.id for i in a.inactiveModels()] == [5] and a.inactiveMap(0).tobytes() == rec.tobytes()
        a.setParam("keepInactiveModels", 0)
        drop(a, 5)
        a.setParam("keepInactiveModels", 1)
        spawn(b, 5, 41, patch(10))
        drop(b, 5)
        assert a.stateDigest() == b.stateDigest()
        # A: the call.  B: its definition, by hand, from A's archive
        a.reactivateModel(0)
        b._chk(b._L.mf_spawn_object_model(b._h, info.id, info.class_id))
        i = len(b.modelIDs()) - 1
        mb = Model(b, i)
        mb.uploadMap(rec)
        mb.overridePose(np.array(info.pose, np.float32).reshape(4, 4).T)
        mb.makeNonStatic()
        b._chk(b._L.mf_model_set_age(b._h, i, info.age, info.confidence_threshold))
        assert a.inactiveModels() == [] and a.modelIDs() == b.modelIDs() == [0, 5]
        ia, ib = a.getModels()[1].info(), mb.info()
        assert (ia.id, ia.class_id, ia.surfels, ia.confidence_threshold, ia.is_static, ia.age) == (ib.id, ib.class_id, ib.surfels, ib.confidence_threshold,
                                                                                                 ib.is_static, ib.age) == (5, 41, len(rec), info.confidence_threshold, 0, info.age)
        assert a.getModels()[1].downloadMap().tobytes() == rec.tobytes()
        assert a.stateDigest() == b.stateDigest()
        for k in (4, 5, 6):
            step(a, k)
            step(b, k)
        da, db = a.stateDigest(), b.stateDigest()
        assert da == db, sorted(k for k in da if da[k] != db.get(k))
        # both segments of the pose log under the one id, in time order
        out = tmp_path / "poses"
        out.mkdir()
        a.exportPoses(str(out) + os.sep)
        rows = np.loadtxt(str(out / "poses-5.txt")).reshape(-1, 8)
        live = a.getPoseLog(a.modelIDs().index(5))[0] if 5 in a.modelIDs() else []
        print("pose log of id 5:", rows[:, 0].tolist(), "live entries", len(live))
        assert len(rows) > len(live) and len(rows) >= 3 and (np.diff(rows[:, 0]) > 0).all()
        assert abs(rows[0, 0] - 33333 * 2 * 1e-6) < 1e-6             # the retired segment starts with the model's first frame
    finally:
        a.close()
        b.close()


def test_reactivate_at_a_given_pose_and_out_of_range(hip):
    mf = make(keepInactiveModels=1, enableSmartModelDelete=0)
    try:
        spawn(mf, 5, 41, patch(100))
        spawn(mf, 6, 42, patch(200, seed=1))
        drop(mf, 5)
        drop(mf, 6)
        assert [i.id for i in mf.inactiveModels()] == [5, 6]
        for k in (-1, 2):
            refused(lambda: mf.reactivateModel(k), "no such inactive model")
        from maskfusion_amd import synth
        P = synth.make_pose(synth.rot_xyz(0.1, -0.2, 0.3), [0.25, -0.5, 0.125])
        mf.reactivateModel(1, P)
        assert mf.modelIDs() == [0, 6] and [i.id for i in mf.inactiveModels()] == [5]
        m = mf.getModels()[1]
        assert np.array_equal(m.getPose().astype(np.float32), P.astype(np.float32)) and m.isNonstatic() and m.lastCount() == 200
    finally:
        mf.close()


# ---------------- 5. the jump rule ----------------
def test_the_jump_rule_lists_what_it_drops(hip):
    """the scenario of tests/test_gpu_multimodel.py::test_pooled_model_reused_after_an_in_place_life: at 320 x 240 a tracked 0.3 m box falls to
    the 0.2 m jump rule and is re-spawned"""
    from maskfusion_amd import MaskFusion, synth
    from test_gpu_multimodel import SEG
    Wj, Hj, f = 320, 240, 264.0
    st = synth.Stream(W=Wj, H=Hj, fx=f, fy=f, cx=Wj / 2.0, cy=Hj / 2.0, n_objects=3, noise=True, object_motion=0.0)

    def run(keep):
        mf = MaskFusion(Wj, Hj, f, f, Wj / 2.0, Hj / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, numOSurfels=1 << 16, enableMultipleModels=True,
                        modelSpawnOffset=2, trackAllModels=True)
        for k, v in dict(mfThreshold=SEG["threshold"], mfWeightDistance=SEG["weightDistance"], mfWeightConvexity=SEG["weightConvexity"],
                         mfMorphEdgeIterations=0, mfMorphMaskIterations=0, newModelMinRelativeSize=SEG["minRelSizeNew"], keepInactiveModels=keep,
                         enableSmartModelDelete=0).items():
            mf.setParam(k, v)
        seen, maps = set(), {}
        for k in range(8):
            rgb, d, mask = st.frame(k)
            for m in mf.getModels()[1:]:
                maps[m.getID()] = m.downloadMap()                   # (a download compacts nothing here: these maps are dense)
            mf.processFrame(rgb, d, mask=mask, classIDs=[0, 41, 42, 43], timestamp=k)
            seen |= set(mf.modelIDs())
        out = (mf.modelIDs(), [m.downloadMap().tobytes() for m in mf.getModels()], mf.downloadSegmentation().tobytes())
        return mf, seen, maps, out
    off, seen0, _, out0 = run(0)
    on, seen1, maps, out1 = run(1)
    try:
        dropped = sorted(seen1 - set(on.modelIDs()))
        assert dropped and seen0 == seen1, "the scenario must drop a model"
        assert off.inactiveModels() == [] and sorted(i.id for i in on.inactiveModels()) == dropped
        assert out0 == out1                                          # keeping changes nothing else
        for k, i in enumerate(on.inactiveModels()):
            got = on.inactiveMap(k)
            assert i.surfels == len(got) and i.class_id in (41, 42, 43)
            # dropped before the frame's fusion, in the frame after the download: the map of the frame before
            assert got.tobytes() == maps[i.id].tobytes()
    finally:
        off.close()
        on.close()


# ---------------- 6. sessions ----------------
def section_names(path):
    """the names in a session file's section table (include/maskfusion_amd.h "Sessions")"""
    import struct
    with open(path, "rb") as f:
        head = f.read(64)
        table = f.read(64 * struct.unpack_from("<I", head, 48)[0])
    return [table[64 * i:64 * i + 32].rstrip(b"\0").decode() for i in range(len(table) // 64)]


def test_a_session_carries_the_list(hip, tmp_path):
    from maskfusion_amd import MaskFusion
    mf = make(keepInactiveModels=1, enableSmartModelDelete=0)
    again = plain = None
    try:
        step(mf, 0)
        mf.saveSession(str(tmp_path / "empty.mfs"))
        spawn(mf, 5, 41, patch(3000, seed=1), age=12)
        spawn(mf, 6, 42, patch(777, seed=2), age=3)
        step(mf, 1)
        drop(mf, 6)
        drop(mf, 5)
        infos = [info_tuple(i) for i in mf.inactiveModels()]
        maps = [mf.inactiveMap(k) for k in range(2)]
        assert [t[0] for t in infos] == [6, 5] and [len(m) for m in maps] == [infos[0][2], infos[1][2]]
        mf.saveSession(str(tmp_path / "two.mfs"))
        assert section_names(tmp_path / "two.mfs").count("inactive") == 1 and "inactive" not in section_names(tmp_path / "empty.mfs")
        again = MaskFusion.loadSession(str(tmp_path / "two.mfs"))
        assert [info_tuple(i) for i in again.inactiveModels()] == infos
        assert [again.inactiveMap(k).tobytes() for k in range(2)] == [m.tobytes() for m in maps]
        assert again.getParam("keepInactiveModels") == 1 and again.getParam("enableSmartModelDelete") == 0
        # the loaded list is live: the same reactivation and one more frame leave the same models on both sides
        again.reactivateModel(1)
        mf.reactivateModel(1)
        step(again, 2)
        step(mf, 2)
        assert again.modelIDs() == mf.modelIDs() == [0, 5] and [i.id for i in again.inactiveModels()] == [6]
        for x, y in zip(again.getModels(), mf.getModels()):
            assert x.downloadMap().tobytes() == y.downloadMap().tobytes() and np.array_equal(x.getPose(), y.getPose())
        plain = MaskFusion.loadSession(str(tmp_path / "empty.mfs"))  # a file without the section: an empty list
        assert plain.inactiveModels() == []
    finally:
        for m in (mf, again, plain):
            if m is not None:
                m.close()
