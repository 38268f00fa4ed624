"""The model-side pyramid as an epilogue of the tile pass ("tilePyramid"), its fix-up launch, and the frame pyramid beside the tile pass
("fusedTilePyramid") change in which launch the two pyramids of the fused head are built -- never what they hold.  Every case runs a stream
twice, with deferPredict 0 (the reference: every prediction at the end of its own frame, the model-side pyramid a launch of its own) and with the
switches under test, and compares the bits of everything a frame leaves behind (tests/test_gpu_deferred_predict.py: snapshot), among them the
three levels of the model's and the frame's vertex / normal maps.  The reference run also reports, frame by frame, the fill-in decision its
tracking step ran with: "pyramidFixupFrames" must count exactly the fused heads among those frames.  Runs on the MI355X (-m gpu) and, with
MF_EMU=1, on the CPU-executed build (tests/test_emu_tile_pyramid.py runs cases 1 and 2 that way, at the emulator's image size)."""
import itertools

import numpy as np
import pytest

from gpu_util import EMU
from test_gpu_deferred_predict import SMALL, frames, reference, run as run_frames, same

pytestmark = pytest.mark.gpu

SWITCHES = ("tilePyramid", "fusedTilePyramid", "fusedFramePyramids")
HEAD = dict(deferPredict=1, fusedBinFilter=1)
NEW = dict(HEAD, tilePyramid=1, fusedTilePyramid=1, fusedFramePyramids=1)
# the first surfels of a map need ~30 frames to reach the default confidence threshold, and until then the prediction is empty and every
# tracking step fills in.  A surfel gains about a quarter per frame: with the threshold at 1 the prediction covers the image -- and the decision
# is 0 -- after a few frames, so a short stream holds both states.
QUICK = dict(confidenceThreshold=1.0)


def fill_hook(mf, k):
    return int(mf.getLastFillIn())     # the decision frame k's tracking step ran with (frame 0 initialises the map and tracks nothing)


def run(fr, size, params, **kw):
    """test_gpu_deferred_predict.run + the fix-up counter, read before the context closes"""
    box = {}
    inner = kw.pop("hook", None)
    last = len(fr) - 1

    def hook(mf, k):
        got = inner(mf, k) if inner is not None else None
        if k == last:
            box["fixups"] = int(mf.getParam("pyramidFixupFrames"))   # (behind the last frame: settles its prediction as the snapshot's reads do)
        return got
    snap, got, cnt = run_frames(fr, size["W"], size["H"], size["f"], params, hook=hook, **kw)
    cnt["fixups"] = box["fixups"]
    return snap, got, cnt


def ref_with_fills(key, fr, size, params=None, **kw):
    """the reference run (deferPredict 0) with the per-frame fill-in decisions: (snapshot, fills)"""
    snap, got, cnt = reference("tp:" + key, fr, size, params=dict(params or {}, deferPredict=0), hook=fill_hook, **kw)
    assert cnt == dict(deferred=0, heads=0), cnt
    return snap, list(got)


# ---- 1. switches, over a stream that holds both states of the fill-in decision ----
@pytest.mark.parametrize("combo", list(itertools.product((1, 0), repeat=len(SWITCHES))), ids=lambda c: "".join(map(str, c)))
def test_every_switch_combination_leaves_the_same_bits(hip, combo):
    n = 8 if EMU else 16
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:n]
    ref, fills = ref_with_fills("small", fr, SMALL, params=QUICK)
    print("fill-in decisions of the reference run:", fills)
    snap, _, cnt = run(fr, SMALL, dict(HEAD, **QUICK, **dict(zip(SWITCHES, combo))))
    same(snap, ref, "state")
    assert (cnt["deferred"], cnt["heads"]) == (n, n - 1), cnt
    if combo[0]:
        assert cnt["fixups"] == sum(fills[1:]), (cnt, fills)      # every frame but the first took the head
        assert 0 < cnt["fixups"] < cnt["heads"], (cnt, fills)      # ... and the stream met both states
    else:
        assert cnt["fixups"] == 0, cnt


# ---- 2. the decision flips in mid-stream: 0 -> 1 -> 0 ----
def has_010(fills):
    """a 0, later a 1, later a 0 among the decisions of the tracked frames"""
    t = fills[1:]
    if 0 not in t:
        return False
    i = t.index(0)
    return 1 in t[i:] and 0 in t[i + t[i:].index(1):]


def test_fill_in_flips_in_mid_stream(hip):
    n, j = (10, 8) if EMU else (14, 8)
    fr = list(frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:n])
    rgb, depth, mask = fr[j]
    depth = depth.copy()
    depth[:, : depth.shape[1] // 2] = 0          # frame j loses the left half of its depth ...
    fr[j] = (rgb, depth, mask)
    # ... and with timeDelta 1 a surfel that went unobserved for a frame leaves the prediction (at the default of 200 frames the map still covers
    # the erased half and the decision stays 0): the coverage falls below 3 / 4 until the map has grown back
    prm = dict(QUICK, timeDelta=1)
    ref, fills = ref_with_fills("flip", fr, SMALL, params=prm)
    print("fill-in decisions of the reference run:", fills)
    assert has_010(fills), fills
    snap, _, cnt = run(fr, SMALL, dict(NEW, **prm))
    same(snap, ref, "state")
    assert cnt["heads"] == n - 1 and cnt["fixups"] == sum(fills[1:]), (cnt, fills)


# ---- 3. holes: whole tiles, whole 4 x 4 blocks and single texels of a block without a winner ----
# far-wall: the back wall (z = 2.8) lies beyond maxDepthProcessed and is never drawn.  That is more than a quarter of the image, so every tracking
#           step of this stream fills in and the pyramid that stands is the fix-up's.
# erased:   a rectangle that no frame's depth covers -- whole tiles inside, its border through the middle of 4 x 4 blocks -- leaves the coverage above
#           3 / 4: the decision is 0 and the pyramid that stands is the tile pass's own.
@pytest.mark.parametrize("kind", ["far-wall", "erased"])
def test_holes_leave_the_same_nan_patterns(hip, kind):
    W, H = SMALL["W"], SMALL["H"]
    fr = list(frames(W, H, SMALL["f"], 16)[:8])
    prm = dict(QUICK)
    x0, x1, y0, y1 = W // 8 + 1, W // 2 + 2, H // 8 + 1, H // 2 + 26
    if kind == "far-wall":
        prm["maxDepthProcessed"] = 2.5
    else:
        for q, (rgb, depth, mask) in enumerate(fr):
            depth = depth.copy()
            depth[y0:y1, x0:x1] = 0
            fr[q] = (rgb, depth, mask)
    ref, fills = ref_with_fills("holes:" + kind, fr, SMALL, params=prm)
    print("fill-in decisions of the reference run:", fills)
    snap, _, cnt = run(fr, SMALL, dict(NEW, **prm))
    same(snap, ref, "state")
    assert cnt["heads"] == 7 and cnt["fixups"] == sum(fills[1:]), (cnt, fills)
    for i in range(3):
        v, nm = snap[f"vmap_g{i}"], snap[f"nmap_g{i}"]
        assert np.isnan(v).any() and (~np.isnan(v)).any(), i
        assert np.isnan(nm).any() and (~np.isnan(nm)).any(), i
    if kind == "erased":
        assert fills[-1] == 0, fills                  # the last frame's pyramid is the epilogue's, not the fix-up's
        # level 0: an empty tile (16 x 24 texels), empty 4 x 4 blocks beside full ones, and 4 x 4 blocks that are only partly empty
        hole = np.isnan(np.asarray(snap["vmap_g0"]).reshape(3, H, W)[2])
        blocks = hole[:H // 4 * 4, :W // 4 * 4].reshape(H // 4, 4, W // 4, 4).sum(axis=(1, 3))
        assert (blocks == 16).any() and (blocks == 0).any() and ((blocks > 0) & (blocks < 16)).any()
        tiles = hole[:H // 24 * 24, :W // 16 * 16].reshape(H // 24, 24, W // 16, 16).all(axis=(1, 3))
        assert tiles.any()


# ---- 4. tile shapes ----
@pytest.mark.parametrize("tile_h,threads", list(itertools.product((16, 20, 24, 32), (256, 512, 1024))), ids=lambda v: str(v))
def test_tile_shapes_give_the_same_bits(hip, tile_h, threads):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:8]
    ref, fills = ref_with_fills("small8", fr, SMALL, params=QUICK)
    snap, _, cnt = run(fr, SMALL, dict(NEW, **QUICK, tileHeight=tile_h, tileThreads=threads))
    same(snap, ref, "state")
    assert cnt["heads"] == 7 and 0 < cnt["fixups"] == sum(fills[1:]) < 7, (cnt, fills)


# (5. a height that is no multiple of 4 cannot be built: mf_create takes multiples of 8 only, so every level-0 texel belongs to a 4 x 4 block)


# ---- 6. 1280 x 960: 4 800 tile workgroups + 2 400 pyramid workgroups of 512 threads against 1 024 resident at once ----
def test_a_launch_beyond_one_round_of_residency(hip):
    size = dict(W=1280, H=960, f=1056.0)
    fr = frames(size["W"], size["H"], size["f"], 3)
    ctor = dict(numGSurfels=1 << 21)
    ref, fills = ref_with_fills("4n", fr, size, params=QUICK, ctor=ctor)
    snap, _, cnt = run(fr, size, dict(NEW, **QUICK), ctor=ctor)
    same(snap, ref, "state")
    assert cnt["heads"] == 2 and cnt["fixups"] == sum(fills[1:]), (cnt, fills)


# ---- 7. frames that do not take the fused head run as ever; a list overflow changes nothing ----
def test_settled_frames_build_no_pyramid_in_the_tile_pass(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:6]
    ref, fills = ref_with_fills("small6", fr, SMALL, params=QUICK)
    # a library call behind every frame settles every prediction: no head, no epilogue, no fix-up -- although the first frames fill in
    snap, got, cnt = run(fr, SMALL, dict(NEW, **QUICK), hook=fill_hook)
    same(snap, ref, "state")
    assert list(got) == fills and sum(fills[1:]) > 0
    assert (cnt["heads"], cnt["fixups"]) == (0, 0), cnt


def test_a_supplied_pose_in_mid_sequence(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:6]
    ref0, _ = ref_with_fills("small6-host", fr, SMALL, params=QUICK, entry="host")
    poses = {2: ref0["pose"]}       # frame 2 is given a pose: no tracking step, hence no fused head and no pyramid of either kind
    ref, fills = ref_with_fills("pose2", fr, SMALL, params=QUICK, entry="host", poses=poses)
    snap, _, cnt = run(fr, SMALL, dict(NEW, **QUICK), entry="host", poses=poses)
    same(snap, ref, "state")
    assert cnt["heads"] == 4, cnt                                     # frames 1, 3, 4, 5
    assert cnt["fixups"] == sum(fills[k] for k in (1, 3, 4, 5)), (cnt, fills)


def test_a_multi_model_context_is_untouched(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:5]
    ctor = dict(enableMultipleModels=True, numOSurfels=1 << 16)
    ref, fills = ref_with_fills("multi", fr, SMALL, params=QUICK, ctor=ctor, entry="host")
    snap, _, cnt = run(fr, SMALL, dict(NEW, **QUICK), ctor=ctor, entry="host")
    same(snap, ref, "state")
    assert sum(fills[1:]) > 0 and (cnt["deferred"], cnt["heads"], cnt["fixups"]) == (0, 0, 0), (cnt, fills)


def test_a_tile_list_overflow_with_the_epilogue_on(hip):
    fr = frames(SMALL["W"], SMALL["H"], SMALL["f"], 16)[:8]
    ref, fills = ref_with_fills("small8", fr, SMALL, params=QUICK)
    tiles = ((SMALL["W"] + 15) // 16) * ((SMALL["H"] + 15) // 16)
    snap, _, cnt = run(fr, SMALL, dict(NEW, **QUICK, splatTileEntries=tiles * 8))     # eight list slots per 16 x 16 pixels: every covered tile overflows
    same(snap, ref, "state")
    assert cnt["heads"] == 7 and cnt["fixups"] == sum(fills[1:]), (cnt, fills)
