"""Two switches of the map half of a frame change how its passes run -- never what they leave behind:
  * "cleanTapGroup": Model::clean requests the 16-byte taps of its window one by one (1), a window column at a time (3) or all nine at once (9);
  * "maskFreeClean": a frame without a mask carries no mask / depth plane into the background's clean pass (1) or carries them (0).
Every case compares the bits of everything a run leaves behind (tests/test_gpu_deferred_predict.py: snapshot -- the pose log, the counts, every
surfel in its slot, the prediction maps, the tick, the fill-in decision) with the same run at the old values (1, 0).  The streams run in every form
the passes of a model take by its size (copy-update, in-place update, in-place clean), so both surfel buffers are the live one in turn.  Runs on the MI355X (-m gpu)
and, with MF_EMU=1, on the CPU-executed build (tests/test_emu_map_half.py runs groups 1 and 2 that way)."""
import itertools

import numpy as np
import pytest

from gpu_util import EMU
from test_gpu_deferred_predict import frames, make, run as run_frames, same, snapshot

pytestmark = pytest.mark.gpu

SWITCHES = ("cleanTapGroup", "maskFreeClean")
OLD = dict(cleanTapGroup=1, maskFreeClean=0)
NEW = dict(cleanTapGroup=3, maskFreeClean=1)
SIZE = dict(W=160, H=120, f=132.0)
# a surfel gains about a quarter of confidence per frame: with the threshold at 1 the window meets live taps after a few frames
QUICK = dict(confidenceThreshold=1.0)
N_STREAM = 12 if EMU else 24        # (the CPU-executed kernels take seconds per frame)
_refs = {}


def run(fr, params, size=SIZE, **kw):
    return run_frames(fr, size["W"], size["H"], size["f"], params, **kw)


def stream(n):
    return frames(SIZE["W"], SIZE["H"], SIZE["f"], N_STREAM)[:n]


def cached(key, fn):
    """a reference run, computed once and left unchanged"""
    if key not in _refs:
        _refs[key] = fn()
    return _refs[key]


def pass_stats(mf, k):
    """what frame k's fuse and clean passes did, from their intermediates: (surfels before, merges, appended, dropped, surfels after)"""
    nc = ((SIZE["W"] + 1) // 2) * ((SIZE["H"] + 1) // 2)       # (even sides: the candidate grid has this size at either parity of the tick)
    after = mf.getBackgroundModel().lastCount()
    op = mf.debugRead("cand_op", count=nc)
    before = pass_stats.prev
    flags = mf.debugRead("clean_flags", count=before + nc)
    pass_stats.prev = after
    return before, int((op == 1).sum()), int(flags[before:].sum()), int(before - flags[:before].sum()), after


def stream_reference(n):
    """old switch values, every prediction at the end of its own frame; with the per-frame statistics of the passes"""
    def go():
        pass_stats.prev = 0
        snap, got, _ = run(stream(n), dict(OLD, **QUICK, deferPredict=0), hook=pass_stats)
        return snap, got
    return cached(("stream", n), go)


# ---- 1. the stream: every combination, both deferPredict values, both buffers downloaded ----
@pytest.mark.parametrize("n", [N_STREAM - 1, N_STREAM], ids=["odd", "even"])
@pytest.mark.parametrize("defer", [0, 1])
@pytest.mark.parametrize("combo", list(itertools.product((3, 1), (1, 0))), ids=lambda c: "".join(map(str, c)))
def test_every_switch_combination_leaves_the_same_bits(hip, combo, defer, n):
    ref, stats = stream_reference(n)
    print("(before, merges, appended, dropped, after) per frame:", stats)
    for before, merges, appended, dropped, after in stats[1:]:
        assert after == before + appended - dropped
    # the stream meets all three kinds of work, each in several frames, or the comparison proves nothing
    assert min(sum(1 for s in stats[1:] if s[q] > 0) for q in (1, 2, 3)) >= 3, stats
    snap, _, cnt = run(stream(n), dict(zip(SWITCHES, combo), **QUICK, deferPredict=defer))
    same(snap, ref, "state")
    assert cnt["deferred"] == (n if defer else 0), cnt


def test_the_whole_window_at_once_leaves_the_same_bits(hip):
    ref, _ = stream_reference(N_STREAM)
    snap, _, _ = run(stream(N_STREAM), dict(NEW, **QUICK, cleanTapGroup=9, deferPredict=1))
    same(snap, ref, "state")


def test_the_switches_default_to_the_new_forms(hip):
    mf = make(SIZE["W"], SIZE["H"], SIZE["f"])
    try:
        assert {k: mf.getParam(k) for k in SWITCHES} == NEW
        with pytest.raises(Exception):
            mf.setParam("cleanTapGroup", 2)
    finally:
        mf.close()


# ---- 2. crafted windows: 32 x 24 maps loaded with uploadMap, one frame ----
CW, CH, CF = 32, 24, 30.0
f32 = np.float32


def slots_literal(c, size):
    """mf_surfel.hip: window_slots_literal, operation by operation in fp32 -> (texels, multiplicities, steps)"""
    fs = f32(size)
    step = f32(f32(1.0) / f32(fs * f32(1.0))) * f32(0.5)
    half = f32(f32(1.0) * step) * f32(2.0)
    end, i = f32(c + half), f32(c - half)
    u, m, s, last, steps = [0, 0, 0], [0, 0, 0], -1, -1, 0
    for _ in range(5):
        if i < end:
            t = int(np.clip(np.floor(f32(np.rint(f32(f32(i * fs) * f32(256.0))) * f32(1.0 / 256.0))), 0, size - 1))
            if t != last:
                s = min(s + 1, 2)
                u[s], last = t, t
            m[s] += 1
            steps += 1
        i = f32(i + step)
    return u, m, steps


def slots_exact(x, size):
    """clean_test's 4 x 4 window in exact arithmetic: fetches at x - 1, x - 0.5, x, x + 0.5 -> three static slots"""
    t = [int(np.clip(np.floor(f32(x + f32(d))), 0, size - 1)) for d in (-1.0, -0.5, 0.0, 0.5)]
    return [t[0], t[2], t[3]], [1 + (t[1] == t[0]), 1 + (t[1] != t[0]) + (t[3] == t[2]), int(t[3] != t[2])], 4


def project(p):
    """index_map.vert / copy_unstable.vert under the identity pose, in fp32"""
    x = f32(f32(f32(CF) * p[0]) / p[2]) + f32(CW / 2.0)
    y = f32(f32(f32(CF) * p[1]) / p[2]) + f32(CH / 2.0)
    return f32(x), f32(y)


def window(p, literal):
    x, y = project(p)
    if literal:
        ux, mx, sx = slots_literal(f32(x / f32(CW)), CW)
        uy, my, sy = slots_literal(f32(y / f32(CH)), CH)
    else:
        ux, mx, sx = slots_exact(x, CW)
        uy, my, sy = slots_exact(y, CH)
    return ux, mx, uy, my, sx, sy


def surfel(x, y, z, conf, init, last, radius=0.1):
    """a surfel that projects to (x, y) of the 32 x 24 image at depth z, facing the camera"""
    return [(x - CW / 2.0) * z / CF, (y - CH / 2.0) * z / CF, z, conf, 0.0, 0.0, init, last, 0.0, 0.0, -1.0, radius]


SUB = [0.5, 0.02, 0.25, 0.75, 0.98, 0.4]      # sub-pixel positions of the test surfels


def crafted_map(thr, tick):
    """A back layer B, one surfel per texel centre -- left half of the image 5 mm behind the test surfels and older than them (it feeds `count`), right
    half 20 mm behind and updated in this frame (it feeds `zCount`) -- with holes; and test surfels S every fourth texel and within a pixel of every
    border, at varying sub-pixel positions.  The holes put S surfels exactly on count 8 | 9 and zCount 4 | 5 under the literal walk.
    Returns (map, rows of S in it)."""
    zS = 1.0
    S, holes = [], set()
    pxs, pys = [0] + list(range(4, CW - 3, 4)) + [CW - 1], [0] + list(range(4, CH - 3, 4)) + [CH - 1]
    targets = {True: [8, 9, None, 8, 9, 0], False: [4, 5, None, 4, 5, 0]}
    for q, (px, py) in enumerate(itertools.product(pxs, pys)):
        s = surfel(px + SUB[q % len(SUB)], py + SUB[(q // 2) % len(SUB)], zS, thr + 5.0, 2.0, tick - 1.0)
        S.append(s)
        p = np.asarray(s[:3], f32)
        ux, mx, uy, my, _, _ = window(p, True)
        own = (int(np.floor(project(p)[0])), int(np.floor(project(p)[1])))
        taps = {}
        for (a, b) in itertools.product(range(3), range(3)):
            if mx[a] * my[b] > 0 and (ux[a], uy[b]) != own:
                taps[(ux[a], uy[b])] = taps.get((ux[a], uy[b]), 0) + mx[a] * my[b]
        want = targets[px < CW // 2][q % 6]
        if want is None:
            continue
        keys = [k for k in taps if k != (3, 4)]      # (texel (3, 4) holds the first surfel of the buffer: never a hole)
        total = sum(taps.values())
        for r in range(len(keys) + 1):               # the smallest set of holes that leaves exactly `want`
            hit = next((c for c in itertools.combinations(keys, r) if total - sum(taps[k] for k in c) == want), None)
            if hit is not None:
                holes.update(hit)
                break
    B = []
    order = [(3, 4)] + [t for t in itertools.product(range(CW), range(CH)) if t != (3, 4)]
    for (tx, ty) in order:
        if (tx, ty) in holes:
            continue
        left = tx < CW // 2
        B.append(surfel(tx + 0.5, ty + 0.5, zS + (0.005 if left else 0.02), thr + 5.0, 1.0, tick - 1.0 if left else tick))
    m = np.asarray(B + S, f32)
    return m, np.arange(len(B), len(m))


def expected_keep(m, rows, thr, tick, literal):
    """copy_unstable.vert's two counting rules for the surfels `rows` of map m, on the index map of m (nearest surfel per texel; the first surfel
    of the buffer reads as no surfel) -> (keep flags, counts, zCounts, per-axis steps, windows with an unused third slot)"""
    win = {}
    for i, p in enumerate(m[:, :3]):
        x, y = project(p)
        t = (int(np.floor(x)), int(np.floor(y)))
        assert 0 <= t[0] < CW and 0 <= t[1] < CH
        if t not in win or p[2] < m[win[t], 2]:
            win[t] = i
    keep, counts, zcounts, steps, unused = [], [], [], [], 0
    for i in rows:
        p, nz = m[i, :3], m[i, 10]
        ux, mx, uy, my, sx, sy = window(p, literal)
        steps += [sx, sy]
        unused += int(mx[2] == 0 or my[2] == 0)
        count = zc = 0
        for (a, b) in itertools.product(range(3), range(3)):
            mult, j = mx[a] * my[b], win.get((ux[a], uy[b]))
            if mult <= 0 or j is None or j == 0 or not (m[j, 3] > thr and m[j, 2] > 0):
                continue
            dz = f32(m[j, 2] - p[2])
            d = f32(np.sqrt(f32(f32(m[j, 0] - p[0]) ** 2 + f32(m[j, 1] - p[1]) ** 2)))
            if m[j, 6] < m[i, 6] and m[j, 2] > p[2] and dz < f32(0.01) and d < f32(m[i, 11] * f32(1.4)):
                count += mult
            if m[j, 7] == f32(tick) and m[j, 2] > p[2] and dz > f32(0.01) and abs(nz) > f32(0.85):
                zc += mult
        keep.append(not (count > 8 or zc > 4))
        counts.append(count)
        zcounts.append(zc)
    return np.asarray(keep), counts, zcounts, steps, unused


def crafted_run(params, literal):
    """two frames of a stream, then the crafted map through one frame that observes nothing, under the identity pose"""
    fr = frames(CW, CH, CF, 2)
    mf = make(CW, CH, CF, numGSurfels=1 << 14)
    try:
        for k, v in dict(params, cleanLiteralWindow=literal).items():
            mf.setParam(k, v)
        for k, (rgb, depth, _) in enumerate(fr):
            mf.processFrame(rgb, depth, timestamp=k)
        bg = mf.getBackgroundModel()
        tick = float(bg.downloadMap()[:, 7].max() + 1)        # the last frame stamped its surfels with its tick: the next frame's is one more
        thr = float(bg.getConfidenceThreshold())
        m, rows = crafted_map(thr, tick)
        bg.uploadMap(m)
        mf.processFrame(fr[0][0], np.zeros_like(fr[0][1]), timestamp=2, inPose=np.eye(4))
        snap = snapshot(mf)
    finally:
        mf.close()
    return snap, m, rows, thr, tick


@pytest.mark.parametrize("literal", [1, 0], ids=["literal", "exact"])
def test_crafted_windows(hip, literal):
    ref, m, rows, thr, tick = cached(("crafted", literal), lambda: crafted_run(OLD, literal))
    keep, counts, zcounts, steps, unused = expected_keep(m, rows, thr, tick, literal)
    print("count", sorted(set(counts)), "zCount", sorted(set(zcounts)), "steps", sorted(set(steps)), "windows with an unused slot", unused)
    # the cases are there: both sides of both limits, 4 and 5 steps of the literal walk, unused third slots, the first surfel of the buffer as a tap
    if literal:
        assert {8, 9} <= set(counts) and {4, 5} <= set(zcounts) and set(steps) == {4, 5}
    assert unused > 0 and 0 < keep.sum() < len(keep)
    x0, y0 = project(m[0, :3])
    assert any((int(np.floor(x0)), int(np.floor(y0))) in itertools.product(window(m[i, :3], literal)[0], window(m[i, :3], literal)[2]) for i in rows)
    near = [i for i in rows if min(project(m[i, :3])[0], CW - project(m[i, :3])[0], project(m[i, :3])[1], CH - project(m[i, :3])[1]) < 1.0]
    assert len(near) >= 8
    # the reference run dropped exactly the test surfels the rules drop: a miscounted tap flips a keep flag
    out = ref["maps"][0]
    left = {tuple(r) for r in out[:, :3].view(np.uint32).tolist()}
    got = np.asarray([tuple(r) in left for r in m[rows, :3].copy().view(np.uint32).tolist()])
    assert np.array_equal(got, keep), (np.flatnonzero(got != keep), counts, zcounts)
    for combo in itertools.product((3, 9, 1), (1, 0)):
        if dict(zip(SWITCHES, combo)) == OLD:
            continue
        snap = crafted_run(dict(zip(SWITCHES, combo)), literal)[0]
        same(snap, ref, "state " + str(combo))


# ---- 3. the form of the passes changes in mid-stream ----
QUARTER = SIZE["W"] * SIZE["H"] // 4
IN_PLACE, BIG = 3000 + QUARTER, 7000 + QUARTER     # (mf_frame.inl: update_copy / clean_small compare count + P / 4 with the thresholds)
UPLOADS = (1, 7)


def form_of(count):
    """0: copy-update + two-launch clean; 1: in-place update + two-launch clean; 2: in-place update + in-place clean"""
    return int(count + QUARTER >= IN_PLACE) + int(count + QUARTER >= BIG)


def form_run(params, small_map):
    """the stream with the two thresholds set; behind frames 1 and 7 a small map is uploaded: the model falls below both thresholds and grows
    through them again"""
    def hook(mf, k):
        if k in UPLOADS:
            mf.getBackgroundModel().uploadMap(small_map)
        return mf.getBackgroundModel().lastCount()
    return run(stream(N_STREAM), dict(params, **QUICK, inPlaceElements=IN_PLACE, bigMapElements=BIG, deferPredict=1), hook=hook)


def test_the_form_changes_in_mid_stream(hip):
    small_map = stream_reference(N_STREAM)[0]["maps"][0][:1000]
    ref, ref_counts, _ = cached("forms", lambda: form_run(OLD, small_map))
    forms = [form_of(c) for c in ref_counts[:-1]]       # the form of frame k + 1, from the count behind frame k
    print("surfels behind each frame:", ref_counts, "forms:", forms)
    steps = set(zip(forms, forms[1:]))
    assert {(0, 1), (1, 2)} <= steps and ((2, 0) in steps or {(2, 1), (1, 0)} <= steps), (ref_counts, forms)      # up and down through both
    for combo in [(3, 1), (1, 1), (3, 0)]:
        snap, counts, _ = form_run(dict(zip(SWITCHES, combo)), small_map)
        assert counts == ref_counts
        same(snap, ref, "state " + str(combo))


# ---- 4. calls between frames ----
def calls_run(params, pose):
    def hook(mf, k):
        bg = mf.getBackgroundModel()
        if k in (2, 3):                 # behind an even and an odd number of frames: either buffer is the live one
            return bg.downloadMap()
        if k == 4:
            bg.uploadMap(bg.downloadMap()[::2])
        if k in (5, 6):
            bg.predictIndices(mf.getTick(), 3.0, 200)
            return mf.debugRead("index")
        if k == 8:
            return mf.getCurrPose()     # a settle point
        return None
    return run(stream(N_STREAM)[:11], dict(params, **QUICK), hook=hook, entry="host", poses={7: pose})


def test_calls_between_frames(hip):
    pose = stream_reference(N_STREAM)[0]["pose"]       # frame 7 is given a pose: no tracking step
    ref, ref_got, _ = cached("calls", lambda: calls_run(dict(OLD, deferPredict=0), pose))
    for defer in (1, 0):
        snap, got, _ = calls_run(dict(NEW, deferPredict=defer), pose)
        same(got, ref_got, "values of the calls")
        same(snap, ref, "state")


# ---- 5. the guard of maskFreeClean: a real mask keeps its planes ----
def test_a_multi_model_context_keeps_the_planes(hip):
    fr = frames(SIZE["W"], SIZE["H"], SIZE["f"], 8, n_objects=3, object_motion=0.0)
    ctor = dict(enableMultipleModels=True, numOSurfels=1 << 16, modelSpawnOffset=1, trackAllModels=False)
    seg = dict(mfThreshold=0.3, mfWeightDistance=150.0, mfWeightConvexity=2.8, mfMorphEdgeIterations=0, mfMorphMaskIterations=0,
               newModelMinRelativeSize=0.004)
    kw = dict(ctor=ctor, entry="host", masks=True, classIDs=[0, 41, 42, 43])
    ref, _, _ = run(fr, dict(seg, **dict(NEW, maskFreeClean=0)), **kw)
    assert len(ref["ids"]) >= 2, ref["ids"]
    snap, _, _ = run(fr, dict(seg, **NEW), **kw)
    same(snap, ref, "state")


def test_the_model_api_clean_still_decays_under_a_mask(hip):
    """Model::clean through the model API in a context that takes masks: with a foreign label over the image the confidences of the surfels the
    frame observes decay, whatever maskFreeClean says"""
    snap, _ = stream_reference(N_STREAM - 1)
    S, pose, tick = snap["maps"][0], snap["pose"], int(snap["tick"])
    rgb, depth, _ = stream(N_STREAM)[-1]
    W, H = SIZE["W"], SIZE["H"]
    outs = {}
    for label, free in itertools.product((0, 5), (0, 1)):
        mf = make(W, H, SIZE["f"], enableMultipleModels=True, numOSurfels=1 << 14)
        try:
            mf.setParam("maskFreeClean", free)
            bg = mf.getBackgroundModel()
            bg.uploadMap(S)
            bg.overridePose(pose); bg.overridePose(pose)
            mf.setTick(tick)
            mf.stageFrame(rgb, depth, np.full((H, W), label, np.uint8))
            bg.predictIndices(tick, 3.0, 200)
            bg.fuse(tick, 3.0, 1.0)
            bg.predictIndices(tick, 3.0, 200)
            bg.clean(tick, 200, 3.0)
            outs[label, free] = bg.downloadMap()
        finally:
            mf.close()
    for label in (0, 5):
        same(outs[label, 1], outs[label, 0], f"label {label}")
    # the surfels of either result by their position: under the foreign label a good part of them lost confidence, none gained any
    plain = {tuple(r[:3]): r[3] for r in outs[0, 0].view(np.uint32).tolist()}
    pairs = np.asarray([(plain[tuple(r[:3])], r[3]) for r in outs[5, 0].view(np.uint32).tolist() if tuple(r[:3]) in plain], np.uint32).view(np.float32)
    assert len(pairs) > len(plain) // 2
    assert (pairs[:, 1] < pairs[:, 0]).sum() > len(pairs) // 10 and not (pairs[:, 1] > pairs[:, 0]).any()


# ---- 6. the other clean kernel: a map that is cleaned in place, run by run ----
def test_the_in_place_clean_groups_its_taps_too(hip):
    size = dict(W=320, H=240, f=264.0)
    fr = frames(size["W"], size["H"], size["f"], 4)
    forms = dict(QUICK, bigMapElements=0, inPlaceElements=0, deferPredict=1)
    ref, _, _ = run(fr, dict(OLD, **forms), size=size)
    assert ref["counts"][0] > 20_000 and (ref["maps"][0][:, 3] > 1.0).sum() > 5_000          # stable surfels: taps that are live
    for combo in [(3, 0), (3, 1), (9, 1), (1, 1)]:
        snap, _, _ = run(fr, dict(zip(SWITCHES, combo), **forms), size=size)
        same(snap, ref, "state " + str(combo))
