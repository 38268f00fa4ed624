"""The two window-tap forms of the surfel half leave every bit where it was:
  * "cleanTap16": inside a frame the index pass that feeds Model::clean writes 16-byte taps {x, y, z', initTime} (z' = NaN unless index > 0,
    confidence > threshold and z > 0; sign bit = lastTime == tick) instead of the 32-byte record {vertConf | initTime, lastTime, index, depth};
  * "fuseLanes": the data association handles a candidate on a quad of lanes (one window column per lane, merged in the serial order) or on one.
Whole frames through every combination of the two, in each of the three map forms, single model and background + objects; a crafted map with the
values the encoding has to survive; and the encoding itself against the 32-byte rules in numpy (no GPU)."""
import numpy as np
import pytest

FORMS = [(0, 0), (1 << 30, 1 << 30), (1 << 30, 0)]      # (bigMapElements, inPlaceElements): the forms of test_clean_forms_agree
SWITCHES = [(0, 1), (0, 4), (1, 1), (1, 4)]             # (cleanTap16, fuseLanes); the first is the reference


# ---------------------------------------------------------------------------------------------------------------------------------------
# the encoding, on the CPU
# ---------------------------------------------------------------------------------------------------------------------------------------
def encode_tap16(x, y, z, conf, init, last, idx, thr, tick):
    """the 16-byte tap of a resolved texel (mf_surfel.hip: tap16_encode)"""
    live = (idx > 0) & (conf > thr) & (z > 0)
    zs = np.where(last == np.float32(tick), -z, z).astype(np.float32)
    return x, y, np.where(live, zs, np.float32(np.nan)).astype(np.float32), init


def rules32(x, y, z, conf, init, last, idx, thr, time, lp, ctz, r, lnz):
    """copy_unstable.vert's two counting rules on the 32-byte record (mf_surfel.hip: clean_test)"""
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy = x - lp[0], y - lp[1]
        r1 = (idx > 0) & (init < ctz) & (conf > thr) & (z > lp[2]) & (z - lp[2] < np.float32(0.01)) & (np.sqrt(dx * dx + dy * dy) < r * np.float32(1.4))
        r2 = (idx > 0) & (last == time) & (conf > thr) & (z > lp[2]) & (z - lp[2] > np.float32(0.01)) & (np.abs(lnz) > np.float32(0.85))
    return r1, r2


def rules16(x, y, zt, init, lp, ctz, r, lnz):
    with np.errstate(invalid="ignore", over="ignore"):
        live = ~np.isnan(zt)
        z = np.abs(zt)
        upd = np.signbit(zt)
        dx, dy = x - lp[0], y - lp[1]
        r1 = live & (init < ctz) & (z > lp[2]) & (z - lp[2] < np.float32(0.01)) & (np.sqrt(dx * dx + dy * dy) < r * np.float32(1.4))
        r2 = live & upd & (z > lp[2]) & (z - lp[2] > np.float32(0.01)) & (np.abs(lnz) > np.float32(0.85))
    return r1, r2


def test_tap16_encoding_counts_what_the_32_byte_record_counts():
    """2 M random taps next to random surfels whose window is walked (lp.z > 0), salted with the values the encoding must survive: NaN, +-0, +-inf,
    negative and half-integer init times, confidence == threshold and one ulp around it, lastTime == tick and tick +- 1."""
    rng = np.random.default_rng(20261018)
    n = 2_000_000
    f32 = np.float32
    thr, tick = f32(10.0), 37
    special = np.array([np.nan, 0.0, -0.0, np.inf, -np.inf, 1e-30, -1e-30], f32)

    def salted(base, extra, p=0.15):
        pool = np.concatenate([special, np.asarray(extra, f32)])
        return np.where(rng.random(n) < p, pool[rng.integers(0, len(pool), n)], base).astype(f32)

    lpz = rng.uniform(0.3, 4.0, n).astype(f32)
    lp = (rng.uniform(-1, 1, n).astype(f32), rng.uniform(-1, 1, n).astype(f32), np.where(rng.random(n) < 0.02, f32(1e-30), lpz).astype(f32))
    # taps near their surfel: both rules really fire
    z = salted(lp[2] + rng.choice(np.array([-0.02, 0.0, 0.004, 0.0099, 0.01, 0.0101, 0.03, 0.5], f32), n), [-1.0, -2.5])
    x = salted(lp[0] + rng.normal(0, 0.01, n).astype(f32), [])
    y = salted(lp[1] + rng.normal(0, 0.01, n).astype(f32), [])
    conf = salted(rng.uniform(0, 20, n), [thr, np.nextafter(thr, f32(np.inf)), np.nextafter(thr, f32(-np.inf))], p=0.3)
    init = salted(rng.integers(1, tick + 1, n), [-3.0, -0.5, 2.5, 17.5])
    last = salted(rng.integers(tick - 3, tick + 2, n), [tick, tick - 1, tick + 1, -1.0, -2.0], p=0.3)
    idx = np.where(rng.random(n) < 0.2, rng.integers(-2, 1, n), rng.integers(1, 1 << 20, n)).astype(np.int32)
    ctz = salted(rng.integers(1, tick + 1, n), [-3.0, 2.5])
    r = salted(rng.uniform(0.001, 0.05, n), [])
    lnz = salted(rng.uniform(-1, 1, n), [0.85, -0.85])

    a1, a2 = rules32(x, y, z, conf, init, last, idx, thr, f32(tick), lp, ctz, r, lnz)
    tx, ty, tz, tw = encode_tap16(x, y, z, conf, init, last, idx, thr, tick)
    b1, b2 = rules16(tx, ty, tz, tw, lp, ctz, r, lnz)
    assert a1.sum() > 1_000 and a2.sum() > 1_000                 # ... on taps that do count
    assert int((a1 != b1).sum()) == 0 and int((a2 != b2).sum()) == 0


# ---------------------------------------------------------------------------------------------------------------------------------------
# whole frames
# ---------------------------------------------------------------------------------------------------------------------------------------
def _context(W, H, f, multi, tap16, lanes, big, in_place):
    from maskfusion_amd import MaskFusion
    # single model: a threshold the map passes within the test's frames (a merge adds at most 1 to a confidence), so that the window meets live
    # taps; with objects: the parameters of test_clean_forms_agree[multi-model]
    conf = 10.0 if multi else 1.0
    mf = MaskFusion(W, H, f, f, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, enableMultipleModels=multi, numGSurfels=1 << 19, numOSurfels=1 << 16,
                    modelSpawnOffset=2, trackAllModels=False, initConfidenceGlobal=conf, initConfidenceObject=0.01)
    if multi:      # (the parameters of test_clean_forms_agree[multi-model])
        for k, v in (("mfThreshold", 0.3), ("mfWeightDistance", 150.0), ("mfWeightConvexity", 2.8), ("mfMorphEdgeIterations", 0),
                     ("mfMorphMaskIterations", 0), ("newModelMinRelativeSize", 0.004)):
            mf.setParam(k, v)
    mf.setParam("bigMapElements", big)
    mf.setParam("inPlaceElements", in_place)
    mf.setParam("cleanTap16", tap16)
    mf.setParam("fuseLanes", lanes)
    assert mf.getParam("cleanTap16") == tap16 and mf.getParam("fuseLanes") == lanes
    return mf


def _run(frames, W, H, f, multi, tap16, lanes, big, in_place):
    mf = _context(W, H, f, multi, tap16, lanes, big, in_place)
    poses = []
    for k, (rgb, d, m) in enumerate(frames):
        mf.processFrame(rgb, d, mask=m if multi else None, classIDs=[0, 41, 42, 43] if multi else (), timestamp=k)
        poses.append([x.getPose() for x in mf.getModels()])
    assert mf.getParam("indexPackedTexelBytes") == (16 if tap16 else 32)       # the form the frames really ran with
    ms = mf.getModels()
    out = dict(poses=poses, ids=[x.getID() for x in ms], counts=[x.lastCount() for x in ms], clouds=[x.downloadMap() for x in ms],
               labels=mf.downloadSegmentation() if multi else None)
    mf.close()
    return out


def _same(a, b, multi):
    assert a["ids"] == b["ids"] and a["counts"] == b["counts"], (a["ids"], b["ids"], a["counts"], b["counts"])
    if multi:
        assert np.array_equal(a["labels"], b["labels"])
    for pa, pb in zip(a["poses"], b["poses"]):
        assert len(pa) == len(pb) and all(np.array_equal(x, y) for x, y in zip(pa, pb))
    for x, y in zip(a["clouds"], b["clouds"]):
        assert np.array_equal(x, y, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=["in-place", "copy-two-launch", "update-in-place"])
def test_switches_change_nothing_single_model(hip, form):
    """328 x 248 (neither side a multiple of the 16-pixel resolve tile), 8 frames: ids, counts, every pose, every surfel in its slot."""
    from maskfusion_amd import synth
    W, H, f = 328, 248, 270.0
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=True)
    frames = [st.frame(k) for k in range(8)]
    ref = _run(frames, W, H, f, False, *SWITCHES[0], *form)
    assert ref["counts"][0] > 20_000
    assert (ref["clouds"][0][:, 3] > 1.0).sum() > 5_000          # stable surfels: taps that are live
    for tap16, lanes in SWITCHES[1:]:
        _same(ref, _run(frames, W, H, f, False, tap16, lanes, *form), False)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS, ids=["in-place", "copy-two-launch", "update-in-place"])
def test_switches_change_nothing_with_objects(hip, form):
    """background + 3 objects at 320 x 240 with the label image: the batched launches, and the mask-disagreement rule reading its depth plane."""
    from maskfusion_amd import synth
    W, H, f = 320, 240, 264.0
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=True, n_objects=3, object_motion=0.0)
    frames = [st.frame(k) for k in range(8)]
    ref = _run(frames, W, H, f, True, *SWITCHES[0], *form)
    assert len(ref["ids"]) >= 3, ref["ids"]         # at least two objects: their passes really were batched
    for tap16, lanes in SWITCHES[1:]:
        _same(ref, _run(frames, W, H, f, True, tap16, lanes, *form), True)


@pytest.mark.gpu
def test_crafted_records_survive_the_encoding(hip):
    """The map after 6 frames with a fixed-seed fifth of its records rewritten -- confidence at the threshold, one ulp above it and NaN; initTime
    negative and non-integer; lastTime equal to the tick about to run and one below it -- and surfel 0 (which the index map cannot tell from "no
    surfel") in view, through one more frame with either tap form: maps and counts exactly equal."""
    from maskfusion_amd import synth
    W, H, f = 328, 248, 270.0
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=True)
    frames = [st.frame(k) for k in range(7)]
    ctxs = [_context(W, H, f, False, tap16, 4, 0, 0) for tap16 in (0, 1)]
    for mf in ctxs:
        for k, (rgb, d, _) in enumerate(frames[:6]):
            mf.processFrame(rgb, d, timestamp=k)
    base = ctxs[0].getBackgroundModel().downloadMap()
    assert np.array_equal(base, ctxs[1].getBackgroundModel().downloadMap(), equal_nan=True)
    thr = np.float32(ctxs[0].getBackgroundModel().getConfidenceThreshold())
    tick = np.float32(base[:, 7].max() + 1)         # the last frame stamped its surfels with its tick: the next frame's is one more
    n = len(base)
    crafted = base.copy()
    rng = np.random.default_rng(7)
    pick = rng.permutation(n)[: n // 5]
    kinds = np.arange(len(pick)) % 7
    crafted[pick[kinds == 0], 3] = thr
    crafted[pick[kinds == 1], 3] = np.nextafter(thr, np.float32(np.inf))
    crafted[pick[kinds == 2], 3] = np.nan
    crafted[pick[kinds == 3], 6] = -3.0
    crafted[pick[kinds == 4], 6] = 2.5
    crafted[pick[kinds == 5], 7] = tick
    crafted[pick[kinds == 6], 7] = tick - 1
    # surfel 0 takes the place of the stable surfel nearest to the image centre
    T = np.linalg.inv(ctxs[0].getCurrPose())
    lp = base[:, :3].astype(np.float64) @ T[:3, :3].T + T[:3, 3]
    u, v = f * lp[:, 0] / lp[:, 2] + W / 2.0, f * lp[:, 1] / lp[:, 2] + H / 2.0
    centre = np.where((lp[:, 2] > 0) & (base[:, 3] > thr), (u - W / 2.0) ** 2 + (v - H / 2.0) ** 2, np.inf)
    j = int(np.argmin(centre))
    assert np.isfinite(centre[j]) and centre[j] < 16.0
    crafted[0] = base[j]
    outs = []
    for mf in ctxs:
        mf.getBackgroundModel().uploadMap(crafted)
        mf.processFrame(frames[6][0], frames[6][1], timestamp=6)
        bg = mf.getBackgroundModel()
        outs.append((bg.lastCount(), bg.downloadMap(), mf.getCurrPose()))
        mf.close()
    (ca, ma, pa), (cb, mb, pb) = outs
    assert ca == cb and np.array_equal(pa, pb) and np.array_equal(ma, mb, equal_nan=True)
    assert ca > 0
