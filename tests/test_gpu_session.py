"""Sessions (mf_session_save / mf_session_load / mf_state_digest): a run that is saved, destroyed, loaded and continued leaves the same bits as a run
that never stopped.  Every comparison is between two runs of the same build and is bit for bit -- no tolerance appears anywhere: the pose logs with
their time stamps, ids, classes, counts, every surfel in its download slot, the prediction maps, the filtered depth, the three levels of the frame's
and of every model's pyramid, the tick, the fill-in decision, the label image and the tracking statistics.
Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build (tests/test_emu_session.py selects the single-model case, the
two-object case and the refusals that way, at the emulator's image size)."""
import os
import re
import struct

import numpy as np
import pytest

from gpu_util import EMU, dev

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# 328 x 248: partial filter, splat and pyramid tiles (tests/test_gpu_deferred_predict.py); MF_EMU=1: the emulator's size
SMALL = dict(W=160, H=120, f=132.0) if EMU else dict(W=328, H=248, f=270.0)
TAPS = (["pred_vertex", "pred_normal", "pred_image", "pred_time", "depthF"] +
        [f"{p}{i}" for p in ("vmap", "nmap", "vmap_g", "nmap_g") for i in range(3)])
MODEL_TAPS = ["pred_vertex", "pred_normal", "pred_image", "pred_time"] + [f"{p}{i}" for p in ("vmap_g", "nmap_g") for i in range(3)]
N = 12            # frames of a single-model run; the save falls behind frame SAVE
SAVE = 5
# the segmentation settings the multi-model tests use on synthetic scenes (tests/test_gpu_switches.py: SEG_D): objects spawn within a few frames
SEG_D = dict(mfThreshold=0.3, mfWeightDistance=150.0, mfWeightConvexity=2.8, mfMorphEdgeIterations=0, mfMorphMaskIterations=0,
             newModelMinRelativeSize=0.004)
_frames = {}
_refs = {}


def frames(n, **kw):
    key = (n, tuple(sorted(kw.items())))
    if key not in _frames:
        from maskfusion_amd import synth
        W, H, f = SMALL["W"], SMALL["H"], SMALL["f"]
        st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=True, **kw)
        _frames[key] = [st.frame(k) for k in range(n)]
    return _frames[key]


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint8) if a.dtype.kind == "f" else a


def same(a, b, what):
    if isinstance(a, dict):
        assert a.keys() == b.keys(), what
        for k in a:
            same(a[k], b[k], f"{what}.{k}")
    elif isinstance(a, (list, tuple)) and not (a and np.isscalar(a[0])):
        assert len(a) == len(b), what
        for i, (x, y) in enumerate(zip(a, b)):
            same(x, y, f"{what}[{i}]")
    elif a is None or b is None:
        assert a is None and b is None, what
    else:
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape and np.array_equal(bits(a), bits(b)), what


def snapshot(mf):
    """everything a sequence leaves behind (tests/test_gpu_deferred_predict.py: snapshot), for every model of the list, plus the label image, the
    classes and the tracking statistics"""
    ts, poses = mf.getPoseLog(0)
    s = dict(log_ts=np.asarray(ts), log=np.asarray(poses), ids=np.asarray(mf.modelIDs()), tick=np.asarray(mf.getTick()),
             fillin=np.asarray(int(mf.getLastFillIn())))
    models = mf.getModels()
    s["counts"] = np.asarray([m.lastCount() for m in models])
    s["maps"] = [m.downloadMap() for m in models]
    s["pose"] = mf.getCurrPose()
    for t in TAPS:
        s[t] = mf.debugRead(t)
    s["classes"] = np.asarray([m.getClassID() for m in models])
    s["icp"] = [np.asarray(m.getICPStats(), np.float32) for m in models]
    s["track"] = [np.asarray([v for _, v in sorted(mf.trackStats(i).items())], np.float32) for i in range(len(models))]
    s["seg"] = mf.downloadSegmentation()
    s["objects"] = []
    for i in range(1, len(models)):
        o = dict(log=[np.asarray(x) for x in mf.getPoseLog(i)], pose=models[i].getPose(), static=np.asarray(int(models[i].isNonstatic())),
                 thr=np.asarray(models[i].getConfidenceThreshold(), np.float32))
        for t in MODEL_TAPS:
            o[t] = mf.debugRead(t, model=i)
        s["objects"].append(o)
    return s


def digest(a):
    """the header's formula, restated: little-endian 32-bit words w_i of the bytes (tail zero-padded), sum (w_i + 1) (2 i + 1) mod 2^64"""
    b = np.ascontiguousarray(a).tobytes()
    b += b"\0" * (-len(b) % 4)
    w = np.frombuffer(b, "<u4").astype(np.uint64)
    i = np.arange(len(w), dtype=np.uint64)
    with np.errstate(over="ignore"):
        return int(((w + np.uint64(1)) * (np.uint64(2) * i + np.uint64(1))).sum(dtype=np.uint64))


# ---- the runs ----
SINGLE = dict(enableMultipleModels=False, numGSurfels=1 << 18)
MODES = {      # constructor arguments, parameters, frame entry
    "icp": (dict(icpThresh=100.0, so3=False), {}, "dev"),                       # the geometric term alone: the only context that defers
    "defaults": (dict(icpThresh=20.0, so3=True), {}, "host"),                   # the reference's defaults
    "ftf": (dict(icpThresh=20.0, so3=True), {"frameToFrameRGB": 1}, "host"),    # setFrameToFrameRGB(True)
}


def make(ctor, params):
    from maskfusion_amd import MaskFusion
    W, H, f = SMALL["W"], SMALL["H"], SMALL["f"]
    mf = MaskFusion(W, H, f, f, W / 2.0, H / 2.0, **ctor)
    for k, v in params.items():
        mf.setParam(k, v)
    return mf


class Run:
    """frames through one context, one at a time; `events` (frame -> call) run before their frame, in every run of a scenario alike"""

    def __init__(self, fr, ctor, params, entry="dev", masks=False, classIDs=(), events=None, mf=None):
        self.fr, self.entry, self.masks, self.classIDs, self.events = fr, entry, masks, classIDs, events or {}
        self.ctor, self.params = ctor, params
        self.mf = mf if mf is not None else make(ctor, params)
        self.held = []

    def step(self, k):
        if k in self.events:
            self.events[k](self.mf)
        rgb, depth, mask = self.fr[k]
        if self.entry == "dev":
            d = [dev(rgb), dev(depth)] + ([dev(mask)] if self.masks else [])
            self.held.append(d)       # (the frame is read asynchronously: its buffers stay alive)
            self.mf.processFrameDevice(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if self.masks else 0, timestamp=k)
        else:
            self.mf.processFrame(rgb, depth, mask if self.masks else None, timestamp=k, classIDs=self.classIDs)

    def reload(self, path, user=b""):
        """save, close, delete, load: nothing of the old context is left"""
        from maskfusion_amd import MaskFusion
        self.mf.saveSession(path, user)
        self.mf.close()
        del self.mf
        self.held = []
        self.mf = MaskFusion.loadSession(path)

    def exports(self, directory):
        """exportPoses + savePly -> {file name: bytes}"""
        d = str(directory) + os.sep
        os.makedirs(d, exist_ok=True)
        self.mf.exportPoses(d)
        self.mf.savePly(d)
        return {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}

    def close(self):
        self.mf.close()


def reference(key, tmp, n, **kw):
    """the run that never stops, with a snapshot behind every frame: computed once per scenario and left unchanged"""
    if key not in _refs:
        r = Run(**kw)
        snaps = []
        for k in range(n):
            r.step(k)
            snaps.append(snapshot(r.mf))
        _refs[key] = dict(snaps=snaps, files=r.exports(tmp.mktemp("ref")), digest=r.mf.stateDigest())
        r.close()
    return _refs[key]


def single_kw(mode, params=None, n=N):
    ctor, prm, entry = MODES[mode]
    return dict(fr=frames(n), ctor=dict(SINGLE, **ctor), params=dict(prm, **(params or {})), entry=entry)


def continue_and_compare(run, ref, first, n, what):
    for k in range(first, n):
        run.step(k)
        same(snapshot(run.mf), ref["snaps"][k], f"{what}: frame {k}")


# ---- 1. continuation, single model ----
@pytest.mark.parametrize("defer", (1, 0), ids=("defer1", "defer0"))
@pytest.mark.parametrize("mode", list(MODES))
def test_continuation_single_model(hip, tmp_path, tmp_path_factory, mode, defer):
    kw = single_kw(mode, {"deferPredict": defer})
    ref = reference(("single", mode, defer), tmp_path_factory, N, **kw)
    b = Run(**kw)
    for k in range(SAVE + 1):
        b.step(k)
    if mode == "icp":    # with deferPredict 1 the save meets a pending prediction (frames went in back to back)
        assert int(b.mf.getParam("deferredFrames")) == (SAVE + 1 if defer else 0)
    b.reload(str(tmp_path / "s.mfs"))
    continue_and_compare(b, ref, SAVE + 1, N, "continued")
    assert b.exports(tmp_path / "b") == ref["files"]
    assert b.mf.stateDigest() == ref["digest"]
    b.close()


# ---- 2. continuation with objects ----
OBJ_N = 14
OBJ_CTOR = dict(icpThresh=100.0, so3=False, enableMultipleModels=True, numGSurfels=1 << 18, numOSurfels=1 << 16, modelSpawnOffset=2,
                trackAllModels=False)
_spawn = {}


def drop(mf, i):
    mf._chk(mf._L.mf_drop_model(mf._h, i))


def object_kw():
    """two objects; model 1 is made non-static two frames behind the first spawn and dropped two frames later (mf_drop_model: its log is retired)"""
    fr = frames(OBJ_N, n_objects=2, object_motion=0.0)
    kw = dict(fr=fr, ctor=OBJ_CTOR, params=dict(SEG_D), entry="host", masks=True, classIDs=[0, 41, 42])
    if "frame" not in _spawn:     # the frame of the first spawn, from a run without events (they come behind it)
        r = Run(**kw)
        for k in range(OBJ_N):
            r.step(k)
            if len(r.mf.modelIDs()) > 1:
                _spawn["frame"] = k
                break
        r.close()
    s = _spawn.get("frame")
    assert s is not None and 1 <= s <= OBJ_N - 7, f"the scene must spawn an object early: {s}"
    kw["events"] = {s + 2: lambda mf: mf.getModels()[1].makeNonStatic(), s + 4: lambda mf: drop(mf, 1)}
    return kw, s


@pytest.mark.parametrize("point", ("before_spawn", "spawn", "nonstatic", "dropped"))
def test_continuation_with_objects(hip, tmp_path, tmp_path_factory, point):
    kw, s = object_kw()
    ref = reference("objects", tmp_path_factory, OBJ_N, **kw)
    assert len(ref["snaps"][s]["ids"]) == 2 and len(ref["snaps"][s - 1]["ids"]) == 1
    logged = {int(n[len("poses-"):-len(".txt")]) for n in ref["files"] if n.startswith("poses-")}
    assert logged > set(ref["snaps"][-1]["ids"].tolist()), logged          # the dropped model's retired log is among the exported ones
    save = {"before_spawn": s - 1, "spawn": s, "nonstatic": s + 2, "dropped": s + 4}[point]
    b = Run(**kw)
    for k in range(save + 1):
        b.step(k)
    if point == "nonstatic":     # the object is tracked on its own from here on -- or the jump rule has dropped it in this very frame and retired its log
        assert b.mf.getModels()[1].isNonstatic() or b.mf.modelIDs() != ref["snaps"][save - 1]["ids"].tolist()
    b.reload(str(tmp_path / "s.mfs"))
    continue_and_compare(b, ref, save + 1, OBJ_N, point)
    assert b.exports(tmp_path / "b") == ref["files"]
    b.close()


# ---- 3. run-structured buffers ----
SHAPES = {"runs": {"bigMapElements": 0}, "two_launch": {"bigMapElements": 1 << 30}, "densify_every": {"bigMapElements": 0, "densifyEvery": 1}}


@pytest.mark.parametrize("shape", list(SHAPES))
def test_continuation_of_a_run_structured_buffer(hip, tmp_path, tmp_path_factory, shape):
    kw = single_kw("icp", dict(SHAPES[shape], deferPredict=1))
    ref = reference(("shape", shape), tmp_path_factory, N, **kw)
    b, twin = Run(**kw), Run(**kw)      # the twin is never saved
    for k in range(SAVE + 1):
        b.step(k)
        twin.step(k)
    if shape == "runs":   # the background is a sparse buffer with a run table when it is saved
        assert b.mf.getParam("backgroundRuns") > 0
    before = (b.mf.getParam("densifyCount"), b.mf.getParam("backgroundRuns"), b.mf.stateDigest())
    path = str(tmp_path / "s.mfs")
    b.mf.saveSession(path)
    assert (b.mf.getParam("densifyCount"), b.mf.getParam("backgroundRuns"), b.mf.stateDigest()) == before     # nothing compacted, nothing changed
    same(snapshot(b.mf), snapshot(twin.mf), "behind the save")
    twin.close()
    b.close()
    from maskfusion_amd import MaskFusion
    c = Run(**kw, mf=MaskFusion.loadSession(path))
    continue_and_compare(c, ref, SAVE + 1, N, shape)
    c.close()


# ---- 4. a save is invisible ----
@pytest.mark.parametrize("mode,params", [("icp", {"deferPredict": 1}), ("icp", {"deferPredict": 1, "bigMapElements": 0}), ("ftf", {"deferPredict": 1})],
                         ids=("icp", "runs", "ftf"))
def test_a_save_is_invisible(hip, tmp_path, tmp_path_factory, mode, params):
    kw = single_kw(mode, params)
    key = ("shape", "runs") if "bigMapElements" in params else ("single", mode, 1)
    ref = reference(key, tmp_path_factory, N, **kw)
    c = Run(**kw)
    for k in range(N):
        c.step(k)
        c.mf.saveSession(str(tmp_path / "s.mfs"))
        same(snapshot(c.mf), ref["snaps"][k], f"frame {k}")
    c.close()


# ---- 5. parameters, the user blob, sessionInfo ----
def parameter_rows():
    """(key, type, access, legal values) of every row of the table, as tests/test_abi.py::test_every_parameter_key_is_documented_in_the_header
    finds the keys; every key is in the header"""
    table = open(os.path.join(ROOT, "maskfusion_amd", "csrc", "mf_params.inl")).read()
    header = open(os.path.join(ROOT, "include", "maskfusion_amd.h")).read()
    rows = []
    for line in re.findall(r'^    \{"[A-Za-z0-9_]+", k(?:In(?:Cfg|Seg|Sw)|Computed).*$', table, re.M):
        key = re.match(r'\s*\{"([A-Za-z0-9_]+)"', line).group(1)
        assert f'"{key}"' in header, key
        typ = re.search(r"\b(kFlag|kInt|kFloat)\b", line).group(1)
        acc = (re.search(r"\b(kReadWrite|kReadOnly|kWriteOnly)\b", line) or [None, "kReadWrite"])[1]
        legal = re.search(r"k(?:ReadWrite), \{([0-9, ]+)\}", line)
        rows.append((key, typ, acc, [int(v) for v in legal.group(1).split(",")] if legal else []))
    assert len(rows) >= 80
    return rows


def test_parameters_user_blob_and_info(hip, tmp_path):
    from maskfusion_amd import MaskFusion
    kw = single_kw("icp")
    a = Run(**kw)
    for k in range(2):
        a.step(k)
    rows = parameter_rows()
    written = 0
    for key, typ, acc, legal in rows:
        if acc != "kReadWrite":
            continue
        v = a.mf.getParam(key)
        if legal:
            new = [x for x in legal if x != int(v)][0]
        elif typ == "kFlag" or (typ == "kInt" and v in (0, 1) and key not in ("densifyEvery", "mfMorphEdgeIterations", "mfMorphMaskIterations")):
            new = 1 - int(v)
        elif typ == "kInt":
            new = int(v) - 1 if key == "splatTileEntries" else int(v) + 1
        else:
            new = float(np.float32(v * 0.5 + 0.125))
        a.mf.setParam(key, new)
        assert a.mf.getParam(key) == new and new != v, key
        written += 1
    assert written >= 60
    readable = [key for key, _, acc, _ in rows if acc != "kWriteOnly"]
    want = {key: a.mf.getParam(key) for key in readable}
    blob = bytes(range(256)) * 3 + b"tail"
    path = str(tmp_path / "p.mfs")
    a.mf.saveSession(path, blob)
    tick = a.mf.getTick()
    a.close()
    info = MaskFusion.sessionInfo(path)       # no context exists at this point
    assert (info["width"], info["height"], info["n_models"], info["tick"], info["frames"]) == (SMALL["W"], SMALL["H"], 1, tick, 2)
    assert info["user"] == blob and info["user_bytes"] == len(blob) and info["file_bytes"] == os.path.getsize(path)
    b = MaskFusion.loadSession(path)
    got = {key: b.getParam(key) for key in readable}
    assert got == want
    assert b.getTick() == tick
    b.close()


# ---- 6. digests ----
def test_digests_restate_the_formula_and_name_the_section_that_changed(hip, tmp_path):
    kw = single_kw("defaults", {"bigMapElements": 0})
    a, b = Run(**kw), Run(**kw)
    for k in range(4):
        a.step(k)
        b.step(k)
    d = a.mf.stateDigest()
    assert d == b.mf.stateDigest()                  # two identical runs
    assert a.mf.getParam("backgroundRuns") > 0       # ... whose surfels sit in a run-structured buffer
    frames_done = 4
    set_ = (frames_done + 1) & 1
    ts, poses = a.mf.getPoseLog(0)
    log = np.zeros((len(ts), 8), np.float32)
    log[:, :7] = poses
    readable = {"pred_vertex[0]": a.mf.debugRead("pred_vertex"), "pred_normal[0]": a.mf.debugRead("pred_normal"), "pred_image[0]": a.mf.debugRead("pred_image"),
                "pred_time[0]": a.mf.debugRead("pred_time"), f"depthF{(frames_done - 1) % 3}": a.mf.debugRead("depthF"), "pose_log[0]": log,
                "segmentation": a.mf.downloadSegmentation()}
    readable.update({f"gray{set_}{i}": a.mf.debugRead(f"gray{i}") for i in range(3)})
    for name, value in readable.items():
        assert d[name] == digest(value), name
    assert d == a.mf.stateDigest()                  # (the taps above compact nothing)
    # the same surfels in a run-structured buffer and, behind the download's compaction, in a dense one
    surfels = a.mf.getBackgroundModel().downloadMap()
    assert a.mf.getParam("backgroundRuns") == 0
    assert d["surfels[0]"] == digest(surfels) == a.mf.stateDigest()["surfels[0]"]
    # one flipped bit of one surfel: exactly that section's word changes
    a.mf.getBackgroundModel().uploadMap(surfels)
    base = a.mf.stateDigest()
    assert base["surfels[0]"] == d["surfels[0]"]
    flipped = surfels.copy()
    flipped.view(np.uint32)[len(flipped) // 2, 5] ^= np.uint32(1 << 9)
    a.mf.getBackgroundModel().uploadMap(flipped)
    after = a.mf.stateDigest()
    assert [k for k in base if base[k] != after[k]] == ["surfels[0]"]
    assert after["surfels[0]"] == digest(flipped)
    a.close()
    b.close()


# ---- 7. refusals ----
def parse_table(raw):
    n = struct.unpack_from("<I", raw, 48)[0]
    out = {}
    for i in range(n):
        name, owner, _, off, size, dig = struct.unpack_from("<32siIQQQ", raw, 64 + 64 * i)
        out[(name.rstrip(b"\0").decode(), owner)] = (off, size, dig)
    return out


def saved_session(tmp_path):
    kw = single_kw("icp")
    a = Run(**kw)
    for k in range(2):
        a.step(k)
    path = str(tmp_path / "good.mfs")
    a.mf.saveSession(path, b"blob")
    a.close()
    return path, open(path, "rb").read()


def test_malformed_files_are_refused_with_a_reason(hip, tmp_path):
    from maskfusion_amd import MaskFusion
    from maskfusion_amd.lib import MFError
    path, raw = saved_session(tmp_path)
    table = parse_table(raw)
    off, size, _ = table[("surfels", 0)]
    assert size > 48 and size % 48 == 0
    flipped = bytearray(raw)
    flipped[off + size // 2] ^= 0x10
    pose_size = struct.unpack_from("<I", raw, 12)[0]
    cases = {
        "truncated": (raw[: off + size // 2], "short"),
        "payload": (bytes(flipped), "surfels"),                                     # the digest mismatch names the section
        "magic": (b"XFSESSN1" + raw[8:], "magic"),
        "version": (raw[:8] + struct.pack("<I", 99) + raw[12:], "version"),
        "struct": (raw[:12] + struct.pack("<I", pose_size + 4) + raw[16:], "sizeof(PoseDev)"),
    }
    for name, (data, word) in cases.items():
        bad = str(tmp_path / (name + ".mfs"))
        open(bad, "wb").write(data)
        with pytest.raises(MFError) as e:
            MaskFusion.loadSession(bad)
        assert "code -1" in str(e.value) and word in str(e.value), (name, str(e.value))      # MF_EINVAL
    MaskFusion.loadSession(path).close()       # ... and the file they were made from loads


def test_a_failed_save_leaves_no_file_and_a_usable_context(hip, tmp_path, tmp_path_factory):
    from maskfusion_amd.lib import MFError
    kw = single_kw("icp", {"deferPredict": 1})
    ref = reference(("single", "icp", 1), tmp_path_factory, N, **kw)
    c = Run(**kw)
    for k in range(SAVE + 1):
        c.step(k)
    target = tmp_path / "no_such_directory" / "s.mfs"
    with pytest.raises(MFError) as e:
        c.mf.saveSession(str(target))
    assert "cannot write" in str(e.value)
    assert not target.exists() and not os.path.exists(str(target) + ".tmp") and os.listdir(str(tmp_path)) == []
    continue_and_compare(c, ref, SAVE + 1, N, "behind the failed save")
    c.close()


# ---- 8. the command-line driver: -savestate / -loadstate ----
def test_cli_two_halves_equal_one_run(hip, tmp_path):
    """-e 7 -savestate, then -loadstate to the end of the log: the -ep poses, -em clouds and -es images of the two halves are those of one run"""
    from maskfusion_amd import cli
    from maskfusion_amd.io import write_image_dir
    fr = frames(10, n_objects=2, object_motion=0.0)
    W, H, f = SMALL["W"], SMALL["H"], SMALL["f"]
    seq = str(tmp_path / "seq") + os.sep
    write_image_dir(seq, [(x[0], x[1]) for x in fr], masks=[x[2] for x in fr], class_ids=[[0, 41, 42]] * len(fr), calibration=(f, f, W / 2.0, H / 2.0, W, H))
    common = ["-dir", seq, "-run", "-q", "-ep", "-em", "-es", "-i", "100", "-nso", "-offset", "2", "-segMinNew", "0.004"]
    one, two = str(tmp_path / "one") + os.sep, str(tmp_path / "two") + os.sep
    state = str(tmp_path / "half.mfs")
    assert cli.main(common + ["-exportdir", one]) == 0
    assert cli.main(common + ["-exportdir", two, "-e", "7", "-savestate", state]) == 0
    first_half = set(os.listdir(two))
    assert cli.main(common + ["-exportdir", two, "-loadstate", state]) == 0
    files = lambda d: {n: open(os.path.join(d, n), "rb").read() for n in sorted(os.listdir(d))}   # noqa: E731
    assert files(one) == files(two)
    assert any(n.startswith("Segmentation") for n in first_half) and set(os.listdir(two)) > first_half
    import json
    from maskfusion_amd import MaskFusion
    blob = json.loads(MaskFusion.sessionInfo(state)["user"].decode())
    assert blob["frames"] == 6 and "-savestate" in blob["argv"]


# ---- 9. the C++ facade: saveSession / loadSession ----
def test_cpp_facade_session(hip, tmp_path):
    """tests/cpp/session_main.cpp: an uninterrupted run against one saved, destroyed, loaded and continued through include/maskfusion/MaskFusion.h"""
    import subprocess
    lib = hip._name if EMU else os.path.join(ROOT, "maskfusion_amd", "libmaskfusion_amd.so")
    exe = str(tmp_path / "session_main")
    r = subprocess.run(["g++", "-std=c++14", "-O1", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "session_main.cpp"), "-o", exe, lib, "-Wl,-rpath," + os.path.dirname(lib)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    fr = frames(N)[:8]
    with open(tmp_path / "frames.bin", "wb") as f:
        for rgb, depth, _ in fr:
            f.write(np.ascontiguousarray(rgb, np.uint8).tobytes())
            f.write(np.ascontiguousarray(depth, np.float32).tobytes())
    W, H, fl = SMALL["W"], SMALL["H"], SMALL["f"]
    out = subprocess.run([exe, str(W), str(H), str(fl), str(fl), str(W / 2.0), str(H / 2.0), "8", "3", str(tmp_path / "frames.bin"), str(tmp_path / "s.mfs")],
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0 and "session ok 4" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]


# ---- 10. a map of several staging chunks (2^18 surfels each): the double-buffered copies of save and load ----
def test_a_map_of_several_chunks_round_trips(hip, tmp_path):
    from maskfusion_amd import MaskFusion
    a = Run(fr=frames(N), ctor=dict(SINGLE, icpThresh=100.0, so3=False, numGSurfels=1 << 20), params={}, entry="host")
    a.step(0)
    n = 2 * (1 << 18) + 12345           # two full chunks and a partial one; no multiple of the kernels' 256 either
    rng = np.random.RandomState(7)
    m = rng.uniform(-2.0, 2.0, (n, 12)).astype(np.float32)
    m[:, 3] = 20.0                      # stable
    m[:, 6:8] = 1.0                     # initTime, lastTime
    m.view(np.uint32)[:, 5] = np.arange(n, dtype=np.uint32)          # every record names its ordinal: a misplaced chunk cannot hide
    a.mf.getBackgroundModel().uploadMap(m)
    path = str(tmp_path / "big.mfs")
    a.mf.saveSession(path)
    d = a.mf.stateDigest()
    assert d["surfels[0]"] == digest(m)
    a.close()
    b = MaskFusion.loadSession(path)
    got = b.getBackgroundModel().downloadMap()
    assert got.shape == m.shape and np.array_equal(got.view(np.uint32), m.view(np.uint32))
    assert b.stateDigest() == d
    raw = bytearray(open(path, "rb").read())
    off, size, _ = parse_table(raw)[("surfels", 0)]
    raw[off + size - 5] ^= 0x80         # one bit in the LAST chunk
    open(path, "wb").write(bytes(raw))
    b.close()
    from maskfusion_amd.lib import MFError
    with pytest.raises(MFError) as e:
        MaskFusion.loadSession(path)
    assert "surfels" in str(e.value) and "digest" in str(e.value)
