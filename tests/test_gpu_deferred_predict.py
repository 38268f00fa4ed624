"""The deferred prediction ("deferPredict") and the fused head of the next frame ("fusedBinFilter", "fusedFramePyramids") change WHEN and in
which launch the background's prediction, the depth filter and the two pyramids run -- never what they compute.  Every case runs a stream twice,
with deferPredict 0 (the reference: every prediction at the end of its own frame) and with the switches under test, and compares the bits of
everything a frame leaves behind: the pose log, ids and counts, every surfel in its slot, the prediction maps, the filtered depth, the three levels
of the frame's and the model's vertex / normal maps, the tick and the fill-in decision.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the
CPU-executed build (tests/test_emu_deferred_predict.py runs cases 1 and 2 that way, at the emulator's image size)."""
import itertools

import numpy as np
import pytest

from gpu_util import EMU, dev

pytestmark = pytest.mark.gpu

SWITCHES = ("deferPredict", "fusedBinFilter", "fusedFramePyramids")
# 328 x 248: the width is no multiple of 64, the height no multiple of 24 and W >> 2 no multiple of 4 -- partial filter, splat and pyramid tiles.
# (MF_EMU=1: the size of tests/test_emu_smoke.py; 160 is no multiple of 64 and 120 >> 2 = 30 no multiple of 4)
SMALL = dict(W=160, H=120, f=132.0) if EMU else dict(W=328, H=248, f=270.0)
TAPS = (["pred_vertex", "pred_normal", "pred_image", "pred_time", "depthF"] +
        [f"{p}{i}" for p in ("vmap", "nmap", "vmap_g", "nmap_g") for i in range(3)])

ON = dict(zip(SWITCHES, (1, 1, 1)))    # every run states its switches: the cases hold whatever the library's defaults are
_frames = {}
_refs = {}


def frames(W, H, f, n, **kw):
    key = (W, H, n, tuple(sorted(kw.items())))
    if key not in _frames:
        from maskfusion_amd import synth
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
    """everything a sequence leaves behind (the first read settles a pending prediction, as every library call does)"""
    ts, poses = mf.getPoseLog(0)
    s = dict(log_ts=np.asarray(ts), log=np.asarray(poses), ids=np.asarray(mf.modelIDs()), tick=np.asarray(mf.getTick()),
             fillin=np.asarray(int(mf.getLastFillIn())))
    s["counts"] = np.asarray([m.lastCount() for m in mf.getModels()])
    s["maps"] = [m.downloadMap() for m in mf.getModels()]
    s["pose"] = mf.getCurrPose()
    for t in TAPS:
        s[t] = mf.debugRead(t)
    return s


def make(W, H, f, **kw):
    from maskfusion_amd import MaskFusion
    args = dict(icpThresh=100.0, so3=False, enableMultipleModels=False, numGSurfels=1 << 18)
    args.update(kw)
    return MaskFusion(W, H, f, f, W / 2.0, H / 2.0, **args)


def run(fr, W, H, f, params, hook=None, entry="dev", masks=False, poses=None, ctor=None, classIDs=()):
    """the frames through one context; hook(mf, k) runs behind frame k.  Returns (snapshot, what the hook returned, counters)"""
    mf = make(W, H, f, **(ctor or {}))
    for k, v in params.items():
        mf.setParam(k, v)
    mf.view = mf.defaultRenderView(W, H)    # (for the render call of the settle points: built before any frame is in flight)
    held, got = [], []
    for k, (rgb, depth, mask) in enumerate(fr):
        if entry == "dev":
            d = [dev(rgb), dev(depth)] + ([dev(mask)] if masks else [])
            held.append(d)   # (the frame is read asynchronously: its buffers stay alive)
            mf.processFrameDevice(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr() if masks else 0, timestamp=k)
        else:
            mf.processFrame(rgb, depth, mask if masks else None, timestamp=k, inPose=None if poses is None else poses.get(k), classIDs=classIDs)
        if hook is not None:
            got.append(hook(mf, k))
    snap = snapshot(mf)
    counters = dict(deferred=int(mf.getParam("deferredFrames")), heads=int(mf.getParam("fusedHeadFrames")))
    mf.close()
    return snap, got, counters


def reference(key, fr, size, **kw):
    """the same run with deferPredict 0, computed once per case and left unchanged"""
    if key not in _refs:
        _refs[key] = run(fr, size["W"], size["H"], size["f"], kw.pop("params", {"deferPredict": 0}), **kw)
    return _refs[key]


# ---- 1. switches ----
@pytest.mark.parametrize("combo", list(itertools.product((1, 0), repeat=len(SWITCHES))), ids=lambda c: "".join(map(str, c)))
def test_every_switch_combination_leaves_the_same_bits(hip, combo):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)
    ref, _, rc = reference("small", fr, SMALL)
    assert rc == dict(deferred=0, heads=0)
    snap, _, cnt = run(fr, SMALL["W"], SMALL["H"], SMALL["f"], dict(zip(SWITCHES, combo)))
    same(snap, ref, "state")
    if combo[0]:      # frames go in back to back: every prediction is deferred, and all frames but the one that initialises the map take the head
        assert cnt == dict(deferred=10, heads=9), cnt
    else:
        assert cnt == dict(deferred=0, heads=0), cnt


# ---- 2. settle points ----
CALLS = {
    "getPose": lambda mf: mf.getCurrPose(),
    "lastCount": lambda mf: np.asarray(mf.getBackgroundModel().lastCount()),
    "downloadMap": lambda mf: mf.getBackgroundModel().downloadMap(),
    "debugRead": lambda mf: mf.debugRead("pred_vertex"),
    "sync": lambda mf: mf.sync(),
    "setParam": lambda mf: mf.setParam("deferPredict", 0),
    "enableTimings": lambda mf: mf.enableTimings(True),
    "render": lambda mf: list(mf.renderView(mf.view, depth=True)),
    "modelPredict": lambda mf: mf.getBackgroundModel().combinedPredict(3.0, 4, 4, 200),   # (tick 1 + three frames)
}


@pytest.mark.parametrize("call", list(CALLS))
def test_a_library_call_between_frames_settles_the_pending_prediction(hip, call):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)[:5]
    hook = lambda mf, k: CALLS[call](mf) if k == 2 else None   # noqa: E731
    ref, ref_got, _ = reference("settle:" + call, fr, SMALL, hook=hook)
    snap, got, cnt = run(fr, SMALL["W"], SMALL["H"], SMALL["f"], ON, hook=hook)
    same(got[2], ref_got[2], "value of " + call)
    same(snap, ref, "state")
    assert cnt["heads"] >= 2, cnt    # frames 1 and 2 took the head; the call settled frame 2's prediction


# ---- 3. the host-pointer entry, asynchronous form ----
def test_host_pointer_frames_take_the_fused_head(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)
    ref, _, _ = reference("small-host", fr, SMALL, entry="host")
    snap, _, cnt = run(fr, SMALL["W"], SMALL["H"], SMALL["f"], ON, entry="host")
    same(snap, ref, "state")
    assert cnt == dict(deferred=10, heads=9), cnt
    same(snap, reference("small", fr, SMALL)[0], "host entry against device entry")


# ---- 4. ineligible contexts ----
@pytest.mark.parametrize("name", ["objects", "photometric", "so3"])
def test_ineligible_contexts_never_defer(hip, name):
    size = dict(W=320, H=240, f=264.0)
    objects = name == "objects"
    ctor = {"objects": dict(enableMultipleModels=True, numOSurfels=1 << 16, modelSpawnOffset=1, trackAllModels=False),
            "photometric": dict(icpThresh=20.0), "so3": dict(so3=True)}[name]
    fr = frames(size["W"], size["H"], size["f"], 8 if objects else 6, **(dict(n_objects=3, object_motion=0.0) if objects else {}))
    kw = dict(ctor=ctor, entry="host", masks=objects, classIDs=[0, 41, 42, 43] if objects else ())
    # (the segmentation settings the multi-model tests use on synthetic scenes: objects spawn within a few frames)
    seg = dict(mfThreshold=0.3, mfWeightDistance=150.0, mfWeightConvexity=2.8, mfMorphEdgeIterations=0, mfMorphMaskIterations=0,
               newModelMinRelativeSize=0.004) if objects else {}
    ref, _, _ = reference("ineligible:" + name, fr, size, params=dict(seg, deferPredict=0), **kw)
    snap, _, cnt = run(fr, size["W"], size["H"], size["f"], dict(seg, **ON), **kw)
    same(snap, ref, "state")
    assert cnt == dict(deferred=0, heads=0), cnt
    if objects:
        assert len(snap["ids"]) >= 2, snap["ids"]   # ... and the scene did spawn objects


# ---- 5. edges ----
def test_the_initialising_frame_and_its_successor(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)[:2]
    ref, _, _ = reference("first-two", fr, SMALL)
    snap, _, cnt = run(fr, SMALL["W"], SMALL["H"], SMALL["f"], ON)
    same(snap, ref, "state")
    assert cnt == dict(deferred=2, heads=1), cnt
    one, _, cnt1 = run(fr[:1], SMALL["W"], SMALL["H"], SMALL["f"], ON)
    same(one, reference("first-one", fr[:1], SMALL)[0], "state after the initialising frame")
    assert cnt1 == dict(deferred=1, heads=0), cnt1


def test_a_supplied_pose_in_mid_sequence(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)[:6]
    ref0, _, _ = reference("small-host6", fr, SMALL, entry="host")
    poses = {3: ref0["pose"]}     # frame 3 is given the pose the tracker found for the last frame: no tracking step, hence no fused head
    ref, _, _ = reference("pose3", fr, SMALL, entry="host", poses=poses)
    snap, _, cnt = run(fr, SMALL["W"], SMALL["H"], SMALL["f"], ON, entry="host", poses=poses)
    same(snap, ref, "state")
    assert cnt == dict(deferred=6, heads=4), cnt   # frames 1, 2, 4, 5


def test_close_with_a_prediction_pending(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)[:3]
    mf = make(SMALL["W"], SMALL["H"], SMALL["f"])
    for k, v in ON.items():
        mf.setParam(k, v)
    held = []
    for k, (rgb, depth, _) in enumerate(fr):
        held.append((dev(rgb), dev(depth)))
        mf.processFrameDevice(held[-1][0].data_ptr(), held[-1][1].data_ptr(), 0, timestamp=k)
    mf.close()      # the record is dropped; nothing of it outlives the context
    snap, _, _ = run(fr, SMALL["W"], SMALL["H"], SMALL["f"], ON)     # ... and the next context starts clean
    same(snap, reference("first-three", fr, SMALL)[0], "state")


def test_two_contexts_fed_alternately(hip):
    fa = frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)[:4]
    fb = list(reversed(frames(SMALL["W"], SMALL["H"], SMALL["f"], 10)[4:8]))
    ra, _, _ = reference("alt-a", fa, SMALL)
    rb, _, _ = reference("alt-b", fb, SMALL)
    a, b = make(SMALL["W"], SMALL["H"], SMALL["f"]), make(SMALL["W"], SMALL["H"], SMALL["f"])
    for mf in (a, b):
        for k, v in ON.items():
            mf.setParam(k, v)
    held = []
    for k in range(4):
        for mf, fr in ((a, fa), (b, fb)):
            held.append((dev(fr[k][0]), dev(fr[k][1])))
            mf.processFrameDevice(held[-1][0].data_ptr(), held[-1][1].data_ptr(), 0, timestamp=k)
    for mf, ref in ((a, ra), (b, rb)):
        same(snapshot(mf), ref, "state")
        assert int(mf.getParam("fusedHeadFrames")) == 3
        mf.close()


# ---- 6. VGA with a 2^20-surfel buffer: 2 048 binning + 1 200 filter workgroups of 256 threads are more than the 2 048 that are resident at once --
# launch A deals its halves out in turns; launch C (1 200 + 304 workgroups) is resident at once there and takes its interleaved form at
# 960 x 720 (2 704 + 680 against 1 536) ----
@pytest.mark.parametrize("size,n", [((640, 480, 528.0), 6), ((960, 720, 792.0), 3)], ids=["vga", "960x720"])
def test_grids_beyond_one_round_of_residency(hip, size, n):
    size = dict(W=size[0], H=size[1], f=size[2])
    fr = frames(size["W"], size["H"], size["f"], n)
    ctor = dict(numGSurfels=1 << 20)
    ref, _, _ = reference("big%d" % size["W"], fr, size, ctor=ctor)
    snap, _, cnt = run(fr, size["W"], size["H"], size["f"], ON, ctor=ctor)
    same(snap, ref, "state")
    assert cnt == dict(deferred=n, heads=n - 1), cnt
