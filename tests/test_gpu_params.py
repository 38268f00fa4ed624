"""mf_set_param / mf_get_param over the whole table of keys (maskfusion_amd/csrc/mf_params.inl): the defaults, a round trip of every read-write
key, the refusals and their texts, and what setting a key does besides storing it.  One small single-model context; only the last group
processes frames.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build (tests/test_emu_params.py)."""
import math

import numpy as np
import pytest

from maskfusion_amd.api import MFError

pytestmark = pytest.mark.gpu

W, H, F = 128, 96, 105.6
EINVAL = "code -1:"

# the defaults of the implementation switches, tuning knobs and test knobs: spelled out, so that a changed default is a conscious edit
DEFAULTS = dict(
    cleanTap16=1, cleanTapGroup=3, maskFreeClean=1, fuseLanes=4, cleanLiteralWindow=1, globalTiles=1, earlyBackgroundFusion=1, objectSmallGrids=1,
    objectScatterSplat=1, literalFusionWeight=1, objectBoundingBoxLimit=1, batchObjectPasses=1, objectStream=1, fusedPreprocessLaunch=1,
    deferPredict=1, fusedBinFilter=1, fusedFramePyramids=1, tilePyramid=1, fusedTilePyramid=1, frameToFrameRGB=0, hostInputAsync=1, hostLockstep=1,
    hostWaitUpload=1, splatTiles=1, batchSolveInPixelPass=1, batchTracking=1, modelApiPackedIndex=0, fusedRgbPyramid=1, slabCulling=1, cullRuns=1,
    densifyEvery=0, bigMapElements=6000000, inPlaceElements=1000000, gpuLabels=1, timings=0, passTimings=0, icpProfile=0, splatProfile=0,
    spriteLanes=4, tileThreads=512, tileHeight=24)
# another legal value of every key above that is not a flag
OTHER = dict(cleanTapGroup=9, fuseLanes=1, densifyEvery=5, bigMapElements=12345, inPlaceElements=54321, spriteLanes=8, tileThreads=256, tileHeight=32)
FLAGS = sorted(k for k in DEFAULTS if k not in OTHER)
# the reference's parameters: their values come from the constructor; the round trip sets these (exact in fp32)
REFERENCE = dict(depthCutoff=2.5, icpWeight=12.5, confidenceThreshold=1.25, outlierCoefficient=0.75, maxDepthProcessed=7.5, fastOdom=3, so3=3, rgbOnly=3,
                 pyramid=3, timeDelta=77, enableMultipleModels=3, trackAllModels=3, modelSpawnOffset=9, newModelMinRelativeSize=0.015625,
                 newModelMaxRelativeSize=0.625, mfThreshold=0.375, mfWeightDistance=0.875, mfWeightConvexity=0.125, mfMorphEdgeIterations=7,
                 mfMorphEdgeRadius=6, mfMorphMaskIterations=5, mfMorphMaskRadius=4)
READ_WRITE = sorted(DEFAULTS) + sorted(REFERENCE) + ["splatTileEntries"]
READ_ONLY = ["indexPackedTexelBytes", "deferredFrames", "fusedHeadFrames", "pyramidFixupFrames", "densifyCount", "cleanRuns", "visibleRuns",
             "backgroundRuns", "unstampedRuns", "hostStageUs", "hostUploadUs", "hostEnqueueUs", "hostCallUs", "hostWaitUs"]
WRITE_ONLY = ["hostProfileReset", "rebuildRunTable"]


def make():
    from maskfusion_amd import MaskFusion
    return MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, enableMultipleModels=False, numGSurfels=1 << 16)


@pytest.fixture(scope="module")
def ctx(hip):
    mf = make()
    yield mf
    mf.close()


def refused(call, key):
    with pytest.raises(MFError) as e:
        call()
    assert EINVAL in str(e.value) and key in str(e.value), str(e.value)
    return str(e.value)


def test_the_table_has_eighty_keys():
    assert len(READ_WRITE) + len(READ_ONLY) + len(WRITE_ONLY) == 80 and len(set(READ_WRITE + READ_ONLY + WRITE_ONLY)) == 80


def test_a_fresh_context_returns_the_defaults(ctx):
    assert {k: ctx.getParam(k) for k in DEFAULTS} == DEFAULTS
    other = make()
    try:
        assert ctx.getParam("splatTileEntries") == other.getParam("splatTileEntries") > 1
        assert {k: other.getParam(k) for k in READ_WRITE} == {k: ctx.getParam(k) for k in READ_WRITE}
    finally:
        other.close()


def test_every_read_write_key_makes_the_round_trip_alone(ctx):
    before = {k: ctx.getParam(k) for k in READ_WRITE}
    for key in READ_WRITE:
        if key in FLAGS:
            new = 1 - before[key]
            ctx.setParam(key, 7 * new)            # flags normalise: 7 is 1
        else:
            new = before["splatTileEntries"] - 1 if key == "splatTileEntries" else OTHER.get(key, REFERENCE.get(key))
            ctx.setParam(key, new)
        assert new != before[key], key
        assert {k: ctx.getParam(k) for k in READ_WRITE} == dict(before, **{key: new}), key
        ctx.setParam(key, before[key])
    assert {k: ctx.getParam(k) for k in READ_WRITE} == before
    for key in FLAGS:                             # ... also from 0, and back
        ctx.setParam(key, 0)
        ctx.setParam(key, 7)
        assert ctx.getParam(key) == 1, key
        ctx.setParam(key, before[key])
    assert {k: ctx.getParam(k) for k in READ_WRITE} == before


def test_illegal_values_are_refused_and_change_nothing(ctx):
    entries = ctx.getParam("splatTileEntries")
    for key, value in [("cleanTapGroup", 2), ("fuseLanes", 3), ("tileHeight", 18), ("tileThreads", 100), ("spriteLanes", 3),
                       ("splatTileEntries", 0), ("splatTileEntries", entries + 1)]:
        before = ctx.getParam(key)
        text = refused(lambda: ctx.setParam(key, value), key)
        assert "legal values" in text, text
        assert ctx.getParam(key) == before, key
    assert {k: ctx.getParam(k) for k in DEFAULTS} == DEFAULTS


def test_access_is_refused_by_name(ctx):
    for key in READ_ONLY:
        assert "read-only" in refused(lambda: ctx.setParam(key, 1), key)
    for key in WRITE_ONLY:
        assert "write-only" in refused(lambda: ctx.getParam(key), key)
    assert "unknown" in refused(lambda: ctx.setParam("noSuchKey", 1), "noSuchKey")
    assert "unknown" in refused(lambda: ctx.getParam("noSuchKey"), "noSuchKey")


def test_taps_actions_and_a_dropped_visibility_list_after_three_frames(hip):
    from maskfusion_amd import synth
    st = synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=True)
    fr = [st.frame(k) for k in range(3)]
    plain, touched = make(), make()
    try:
        for k, (rgb, depth, _) in enumerate(fr):
            plain.processFrame(rgb, depth, timestamp=k)
            touched.processFrame(rgb, depth, timestamp=k)
            touched.setParam("cullRuns", 0)       # drops the cached visibility list; the next frame rebuilds it
            assert touched.getParam("cullRuns") == 0
            touched.setParam("cullRuns", 1)
        a, b = plain.getCurrPose(), touched.getCurrPose()
        assert np.array_equal(np.ascontiguousarray(a).view(np.uint8), np.ascontiguousarray(b).view(np.uint8))
        taps = {k: plain.getParam(k) for k in READ_ONLY}
        print(taps)
        assert all(math.isfinite(v) and v >= 0 for v in taps.values()), taps
        assert taps["indexPackedTexelBytes"] in (16, 32) and taps["hostCallUs"] > 0
        plain.setParam("rebuildRunTable", 1)
        plain.setParam("hostProfileReset", 1)
        assert plain.getParam("hostCallUs") == 0
        assert plain.getParam("backgroundRuns") > 0
    finally:
        plain.close()
        touched.close()
