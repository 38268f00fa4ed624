"""Every form of the sprite passes on the sprites that can go wrong.

The prediction (splat.vert + combo_splat.frag) and GlobalProjection (splat_models.vert + combo_splat_models.frag) draw surfels as screen-space
discs, each in a scatter form and a tiled form; all four run the set-up, ray and pixel test of mf_sprite_device.h.  The form tests elsewhere draw
synthetic rooms; here one crafted map puts a sprite on every edge of the rule, and every form has to give the bytes of the specification form
(the scatter with one lane per surfel) in the four prediction maps and in the 64-bit key image.  No tolerances, no exempt pixels.

Image 80 x 56: five tile columns; with "tileHeight" 24 two tile rows and a partial one of 8 rows (16 and 32 run too).  fx = fy = 64,
cx = 40.5, cy = 28, identity pose, tick 300, timeDelta 200, depth limits 4 m, confidence threshold 2 (12 for GlobalProjection): with these a
surfel at depth z projects EXACTLY to u = 64 x / z + 40.5, so a centre can be put on an image border or a pixel centre in fp32.

Hand-placed classes (each surfel has its own colour and initTime, so pred_image / pred_time name the winner of a pixel):
  a  centres projecting exactly to u = 0, u = W, v = 0, v = H: drawn (the test is 0 <= u <= W)
  b  the nearest centres whose projection lies outside: the float next to W and H, and one step of 64 x + c (3.8e-6) below 0 -- no centre
     projects onto the float next to 0 --: not drawn
  c  a far, small surfel (0.18 px): clamped to 1 px, covers the pixel its centre falls in
  d  a near, large surfel (87 px): clamped to 64 px, its box covers every tile column; behind everything else
  e  two coplanar surfels with bit-equal cp.z on shared pixels: the lower index wins (GlobalProjection: the lower model order)
  f  confidence exactly at the threshold: drawn (pc.w < thr rejects); one float below: not drawn -- at 2 for the prediction, at 12 for GlobalProjection
  g  lastTime = time - timeDelta: drawn; one less: not drawn; lastTime > time: not drawn
  h  h.z = maxDepth exactly: drawn; the next float beyond: not drawn; h.z < 0: not drawn
  i  a disc seen edge-on (dot(l, n) = 0 at its centre pixel): the division yields no finite point, nothing is covered
  j  sprites whose boxes straddle a tile corner (x = 64, y = 48 for tile heights 16 and 24; x = 16, y = 32 for 16 and 32): four tiles list them
  k  a few hundred random surfels in the middle of the image: more sprites per tile than the eight list slots "splatTileEntries" leaves

Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build (tests/test_emu_sprite_forms.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from gpu_util import empty, host  # noqa: E402
from test_gpu_inactive_models import spawn  # noqa: E402

pytestmark = pytest.mark.gpu

W, H, F, CX, CY = 80, 56, 64.0, 40.5, 28.0
TICK, TIME_DELTA, MAX_DEPTH, THR, GLOBAL_THR = 300, 200, 4.0, 2.0, 12.0
f32 = np.float32
UP, DOWN = f32(np.inf), f32(-np.inf)


def proj(x, z, c):
    """((f * x) / z) + c as the kernels round it"""
    return f32(f32(f32(F) * f32(x)) / f32(z)) + f32(c)


def just_outside(x, bound, c, direction):
    """x projects to `bound` at depth 1: the float nearest to x in `direction` whose projection lies outside it (every float between them still
    rounds onto the bound; at W and H the projection is then the float next to the bound, at 0 the smallest step of 64 x + c)"""
    for _ in range(8):
        x = np.nextafter(f32(x), direction)
        if proj(x, 1.0, c) != f32(bound):
            break
    p = proj(x, 1.0, c)
    assert (p < bound if direction < 0 else p == np.nextafter(f32(bound), direction)) and abs(float(p) - bound) < 1e-5, (x, p)
    return x


def at_pixel(px, py, z):
    """the point at depth z whose projection is the centre of pixel (px, py), exactly"""
    x, y = f32((px + 0.5 - CX) / F * z), f32((py + 0.5 - CY) / F * z)
    assert proj(x, z, CX) == f32(px + 0.5) and proj(y, z, CY) == f32(py + 0.5)
    return x, y


class Crafted:
    """the map (downloadMap's layout) and what is expected of each hand-placed surfel"""

    def __init__(self):
        self.rows, self.hand = [], {}
        px_x = lambda px: at_pixel(px, 0, 1.0)[0]
        px_y = lambda py: at_pixel(0, py, 1.0)[1]
        x0, xW, y0, yH = f32(-CX / F), f32((W - CX) / F), f32(-CY / F), f32((H - CY) / F)
        assert proj(x0, 1, CX) == 0 and proj(xW, 1, CX) == W and proj(y0, 1, CY) == 0 and proj(yH, 1, CY) == H
        # a / b: the image borders.  pixel: where the sprite shows (a) / would show (b)
        self.add("a_u0", x0, px_y(4), pixel=(0, 4), drawn=True)
        self.add("a_uW", xW, px_y(4), pixel=(W - 1, 4), drawn=True)
        self.add("a_v0", px_x(20), y0, pixel=(20, 0), drawn=True)
        self.add("a_vH", px_x(20), yH, pixel=(20, H - 1), drawn=True)
        self.add("b_u0", just_outside(x0, 0, CX, DOWN), px_y(10), pixel=(0, 10), drawn=False)
        self.add("b_uW", just_outside(xW, W, CX, UP), px_y(10), pixel=(W - 1, 10), drawn=False)
        self.add("b_v0", px_x(24), just_outside(y0, 0, CY, DOWN), pixel=(24, 0), drawn=False)
        self.add("b_vH", px_x(24), just_outside(yH, H, CY, UP), pixel=(24, H - 1), drawn=False)
        self.at("c", 36, 8, z=2.0, r=0.002, drawn=True)                       # 2 sqrt2 r f / z = 0.18 px
        self.at("d", 40, 28, z=2.5, r=1.2, drawn=True)                        # 87 px; the disc itself has a radius of 30.7 px
        self.at("e_first", 50, 40, r=0.04, drawn=True)                        # discs of 2.56 px, two pixels apart, in the plane z = 1:
        self.at("e_second", 52, 40, r=0.04, drawn=False, loses_to="e_first")  # ... every pixel of this one within 2.56 px of the first ties
        self.at("f_at_thr", 3, 16, conf=THR, drawn=True, in_global=False)
        self.at("f_below_thr", 3, 20, conf=np.nextafter(f32(THR), DOWN), drawn=False, in_global=False)
        self.at("f_at_12", 3, 24, conf=GLOBAL_THR, drawn=True)
        self.at("f_below_12", 3, 28, conf=np.nextafter(f32(GLOBAL_THR), DOWN), drawn=True, in_global=False)
        self.at("g_at_delta", 76, 16, last=TICK - TIME_DELTA, drawn=True)
        self.at("g_beyond_delta", 76, 20, last=TICK - TIME_DELTA - 1, drawn=False)
        self.at("g_future", 76, 24, last=TICK + 1, drawn=False)
        self.at("h_at_max", 3, 40, z=MAX_DEPTH, r=0.05, drawn=True)
        zb = np.nextafter(f32(MAX_DEPTH), UP)
        self.add("h_beyond_max", f32((3.5 - CX) / F * zb), f32((46.5 - CY) / F * zb), z=zb, r=0.05, pixel=(3, 46), drawn=False)
        self.add("h_behind", 0.0, 0.0, z=-1.0, pixel=(40, 28), drawn=False)
        self.at("i_edge_on", 40, 48, r=0.05, normal=(1.0, 0.0, 0.0), drawn=False)   # the ray of pixel column 40 has l.x = 0 exactly
        self.at("j_64_48", 64, 48, r=0.03, drawn=True)
        self.at("j_16_32", 16, 32, r=0.03, drawn=True)
        self.hand["d"]["pixel"] = self.hand["h_behind"]["pixel"] = (40, 38)     # (where nothing stands in front of d)
        # k: random surfels over pixels 24..60 x 15..30, 1.2 .. 2 m away, tilted up to ~23 degrees; a third of them below GlobalProjection's threshold
        rng = np.random.default_rng(7)
        for j in range(300):
            z = f32(rng.uniform(1.2, 2.0))
            n = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -1.0])
            self.row(f32((rng.uniform(24, 60) - CX) / F * z), f32((rng.uniform(15, 30) - CY) / F * z), z, 5.0 if j % 3 == 0 else 20.0, 0xF00000 | j, TICK,
                     n / np.linalg.norm(n), rng.uniform(0.008, 0.025))
        self.S = np.array(self.rows, np.float32)
        assert len(np.unique(self.S[:, 4])) == len(self.S) and len(np.unique(self.S[:, 6])) == len(self.S)

    def row(self, x, y, z, conf, colour, last, normal, r):
        self.rows.append([x, y, z, conf, float(colour), 0.0, float(len(self.rows) + 1), float(last), normal[0], normal[1], normal[2], r])

    def add(self, name, x, y, z=1.0, r=0.02, conf=20.0, last=TICK, normal=(0.0, 0.0, -1.0), pixel=None, drawn=True, in_global=None, loses_to=None, centred=False):
        k = len(self.rows)
        colour = ((2 * k + 2) << 16) | ((200 - 3 * k) << 8) | (k + 1)
        self.hand[name] = dict(index=k, pixel=pixel, drawn=drawn, in_global=drawn if in_global is None else in_global, loses_to=loses_to, centred=centred,
                               rgb=((colour >> 16) & 255, (colour >> 8) & 255, colour & 255), time=k + 1)
        self.row(x, y, z, conf, colour, last, normal, r)

    def at(self, name, px, py, z=1.0, **kw):
        x, y = at_pixel(px, py, z)
        self.add(name, x, y, z=z, pixel=(px, py), centred=True, **kw)

    def boxes(self):
        """the pixel box of every sprite that passes the gates of the prediction, to a pixel (numpy's fp32, not the kernels' bits): for counting only"""
        S = self.S
        out = []
        for s in S:
            x, y, z, conf, last, n, r = s[0], s[1], s[2], s[3], s[7], s[8:11].astype(np.float64), float(s[11])
            if conf < THR or z > MAX_DEPTH or z < 0 or TICK - last > TIME_DELTA or last > TICK:
                continue
            u, v = proj(x, z, CX), proj(y, z, CY)
            if not (0 <= u <= W and 0 <= v <= H):
                continue
            x1 = np.array([n[1] - n[2], -n[0], n[0]]); x1 = x1 / np.linalg.norm(x1) * r * 1.41421356
            y1 = np.cross(n, x1)
            c = np.array([x, y, z]) + np.array([x1, y1, -y1, -x1])
            pu, pv = F * c[:, 0] / c[:, 2] + CX, F * c[:, 1] / c[:, 2] + CY
            half = min(max(pu.max() - pu.min(), pv.max() - pv.min(), 1.0), 64.0) / 2
            out.append((max(0, int(np.ceil(u - half - 0.5))), min(W - 1, int(np.ceil(u + half - 0.5)) - 1),
                        max(0, int(np.ceil(v - half - 0.5))), min(H - 1, int(np.ceil(v + half - 0.5)) - 1)))
        return out


@pytest.fixture(scope="module")
def crafted():
    return Crafted()


def context(multi, **params):
    from maskfusion_amd import MaskFusion
    mf = MaskFusion(W, H, F, F, CX, CY, timeDelta=TIME_DELTA, initConfidenceGlobal=THR, depthCut=MAX_DEPTH, icpThresh=100.0, so3=False, numGSurfels=1 << 12,
                    numOSurfels=1 << 12, enableMultipleModels=multi, modelSpawnOffset=1000, trackAllModels=False)
    mf.setParam("maxDepthProcessed", MAX_DEPTH)
    for k, v in params.items():
        mf.setParam(k, v)
    return mf


def pred_maps(mf, model=0):
    return {k: mf.debugRead(k, model=model) for k in ("pred_vertex", "pred_normal", "pred_image", "pred_time")}


def key_image(mf, orders):
    out = empty((H, W), __import__("torch").int64)
    o = np.ascontiguousarray(orders, np.int32)
    mf._chk(mf._L.mf_export_projection_keys_dev(mf._h, o.ctypes.data, len(o), out.data_ptr()))
    mf._chk(mf._L.mf_sync(mf._h))
    return host(out).view(np.uint64)


def same_bytes(got, want, what):
    for k in got:
        assert got[k].tobytes() == want[k].tobytes(), f"{what}: {k} differs from the specification form in {int((got[k] != want[k]).sum())} entries"


@pytest.fixture(scope="module")
def background(hip, crafted):
    """one single-model context: uploadMap, tick, identity pose; the forms are switched between calls"""
    mf = context(False)
    mf.getBackgroundModel().uploadMap(crafted.S)
    mf.setTick(TICK)
    yield mf
    mf.close()


SPEC = dict(splatTiles=0, globalTiles=0, cullRuns=0)


def set_all(mf, params):
    for k, v in params.items():
        mf.setParam(k, v)


@pytest.fixture(scope="module")
def spec(background):
    """the specification form: the scatter kernels with one lane per surfel"""
    set_all(background, SPEC)
    background.predict()
    return dict(pred_maps(background), keys=key_image(background, [0]))


# ---------------- 1. premises, on the specification form ----------------
def winner(spec, pixel):
    px, py = pixel
    return tuple(int(v) for v in spec["pred_image"][py, px, :3]), int(spec["pred_time"][py, px])


def test_premises_of_the_prediction(crafted, spec):
    img, hand = spec["pred_image"], crafted.hand
    seen = 0
    for name, h in hand.items():
        shown = (img[..., :3] == np.array(h["rgb"], np.uint8)).all(-1)
        if h["drawn"]:
            assert winner(spec, h["pixel"]) == (h["rgb"], h["time"]), (name, winner(spec, h["pixel"]))
            seen += 1
        else:
            assert h["loses_to"] or not shown.any(), (name, "wins", int(shown.sum()), "pixels")
            # ... and its pixel is empty, or shows what stands there instead
            want = {(hand["d"]["rgb"], hand["d"]["time"]), ((0, 0, 0), 0)} if h["loses_to"] is None else {(hand[h["loses_to"]]["rgb"], hand[h["loses_to"]]["time"])}
            assert winner(spec, h["pixel"]) in want, (name, winner(spec, h["pixel"]))
    assert seen == 14 and len(hand) == 25
    # c: exactly its one pixel;  d: clamped to 64 px -- columns 8 .. 71, i.e. tile columns 0 .. 4 -- and the only sprite at 2.5 m
    assert (img[..., :3] == np.array(hand["c"]["rgb"], np.uint8)).all(-1).sum() == 1
    d = (img[..., :3] == np.array(hand["d"]["rgb"], np.uint8)).all(-1)
    cols = np.flatnonzero(d.any(0))
    assert cols.min() // 16 == 0 and cols.max() // 16 == 4 and cols.min() >= 8 and cols.max() <= 71, (cols.min(), cols.max())
    assert (spec["pred_vertex"][..., 2][d] > 2.4).all() and (spec["pred_vertex"][..., 2][~d] < 2.4).sum() > 300
    # e: the two discs tie bit for bit on the three pixels between their centres, and the lower index has them all
    z = spec["pred_vertex"][40, 50:53, 2]
    assert all(winner(spec, (px, 40)) == (hand["e_first"]["rgb"], hand["e_first"]["time"]) for px in (50, 51, 52)) and (z.view(np.uint32) == z.view(np.uint32)[0]).all()
    assert winner(spec, (54, 40)) == (hand["e_second"]["rgb"], hand["e_second"]["time"])      # (the second is drawn where the first does not reach)
    # i: the box is there, the pixel test rejects every pixel of it
    assert winner(spec, (40, 48)) == (hand["d"]["rgb"], hand["d"]["time"])
    # k: a random surfel wins somewhere
    assert (img[..., 0] == 0xF0).sum() > 100
    # empty pixels stay all zero
    empty_px = spec["pred_time"] == 0
    assert empty_px.sum() > 500 and not spec["pred_vertex"][empty_px].any() and not spec["pred_normal"][empty_px].any() and not img[empty_px].any()


def test_premises_of_the_tile_lists(crafted):
    boxes = crafted.boxes()
    for tile_h, corners in ((16, [(64, 48), (16, 32)]), (24, [(64, 48)]), (32, [(16, 32)])):
        for (x, y) in corners:       # j: a box on both sides of the corner in x and y -- listed by four tiles
            assert x % 16 == 0 and y % tile_h == 0 and any(b[0] < x <= b[1] and b[2] < y <= b[3] for b in boxes), (tile_h, x, y)
        count = np.zeros((-(-H // tile_h), 5), int)
        for b in boxes:
            count[b[2] // tile_h:b[3] // tile_h + 1, b[0] // 16:b[1] // 16 + 1] += 1
        print("tileHeight", tile_h, "sprites per tile\n", count)
        assert count.max() > 4 * 8, "k: the fullest tile must overrun a list of eight slots by far"
        assert (count > 8).sum() >= 3 and (count <= 8).sum() >= 3      # tiles of both kinds
        assert (count[:, :] > 0).all(1).any()                          # d: a sprite in every tile column of a row


def test_premises_of_global_projection(crafted, spec):
    keys, hand = spec["keys"], crafted.hand
    EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
    assert ((keys != EMPTY) & ((keys & np.uint64(0xFFFFFFFF)) != 0)).sum() == 0      # the background: order 0, id 0
    zbits = (keys >> np.uint64(32)).astype(np.uint32)
    pz = spec["pred_vertex"][..., 2].view(np.uint32)
    for name, h in hand.items():
        px, py = h["pixel"]
        if name in ("d", "h_behind", "e_second", "i_edge_on"):
            continue
        if h["in_global"]:     # the same fragment as in the prediction: confidence >= 12 and in front
            assert keys[py, px] != EMPTY and zbits[py, px] == pz[py, px], name
        elif np.hypot(px + 0.5 - 40.5, py + 0.5 - 28.5) > 31.5:      # outside d's disc: nothing else stands there
            assert keys[py, px] == EMPTY, name
    assert hand["f_below_12"]["drawn"] and keys[28, 3] == EMPTY and keys[24, 3] != EMPTY       # f at 12
    assert keys[16, 3] == EMPTY                                                                  # (a confidence of 2 is not 12)
    # fewer fragments than the prediction (a third of the random surfels have confidence 5), the same z where both have the same winner
    assert 300 < (keys != EMPTY).sum() < (spec["pred_time"] != 0).sum()


# ---------------- 2. forms ----------------
TILE_FORMS = [dict(spriteLanes=lanes, tileThreads=threads, tileHeight=th) for th in (16, 24, 32) for lanes in (1, 4, 16) for threads in (256, 512)]


def test_background_prediction_forms(background, spec):
    mf = background
    try:
        for form in TILE_FORMS:
            set_all(mf, dict(SPEC, splatTiles=1, **form))
            mf.predict()
            same_bytes(pred_maps(mf), spec, f"tiled {form}")
        # k: eight list slots per tile -- the tiles above them scan the map's sprite boxes instead of their lists
        full = mf.getParam("splatTileEntries")
        for th in (16, 24, 32):
            tiles = 5 * -(-H // th)
            set_all(mf, dict(SPEC, splatTiles=1, spriteLanes=4, tileThreads=512, tileHeight=th, splatTileEntries=8 * tiles))
            mf.predict()
            same_bytes(pred_maps(mf), spec, f"tileHeight {th}, eight slots per tile")
            mf.setParam("splatTileEntries", full)
        assert full >= 64 * 15
        # the visibility-list walk: every run of the table listed by k_cull
        for form in (dict(splatTiles=0), dict(splatTiles=1), dict(splatTiles=1, splatTileEntries=8 * 15)):
            set_all(mf, dict(SPEC, tileHeight=24, cullRuns=1, bigMapElements=1, **form))
            mf.predict()
            assert form["splatTiles"] == 0 or mf.getParam("visibleRuns") == 1        # (the scatter form walks the buffer, list or no list)
            same_bytes(pred_maps(mf), spec, f"cullRuns, {form}")
        mf.setParam("splatTileEntries", full)
    finally:
        set_all(mf, dict(SPEC, tileHeight=24, spriteLanes=4, tileThreads=512))


def test_background_global_projection_forms(background, spec):
    mf = background
    try:
        for form in (dict(), dict(tileHeight=16), dict(tileHeight=32, spriteLanes=1), dict(cullRuns=1, bigMapElements=1)):
            set_all(mf, dict(SPEC, splatTiles=1, globalTiles=1, **form))
            assert key_image(mf, [0]).tobytes() == spec["keys"].tobytes(), form
        full = mf.getParam("splatTileEntries")
        set_all(mf, dict(SPEC, splatTiles=1, globalTiles=1, tileHeight=24, splatTileEntries=8 * 15))
        assert key_image(mf, [0]).tobytes() == spec["keys"].tobytes(), "eight slots per tile"
        mf.setParam("splatTileEntries", full)
    finally:
        set_all(mf, dict(SPEC, tileHeight=24, spriteLanes=4))


def test_object_forms(hip, crafted, spec):
    """two object models with the crafted map (grid.z = 2 in the batched launches), threshold min(4.5, 50 / 25) = 2, identity poses"""
    mf = context(True)
    try:
        mf.getBackgroundModel().uploadMap(crafted.S[:1])
        for mid in (5, 6):
            spawn(mf, mid, 41, crafted.S, age=50)
        mf.stageFrame(np.zeros((H, W, 3), np.uint8), np.ones((H, W), np.float32))
        default_in_place = mf.getParam("inPlaceElements")
        assert default_in_place > len(crafted.S)
        results = {}
        for scatter in (1, 0):
            for batch in (0, 1):
                for in_place in (default_in_place, 1):
                    set_all(mf, dict(objectScatterSplat=scatter, batchObjectPasses=batch, inPlaceElements=in_place, splatTiles=1))
                    mf.setTick(TICK)
                    keys = key_image(mf, [-1, 1, 2])
                    mf.predictModels(firstModel=1)
                    results[(scatter, batch, in_place == 1)] = [dict(pred_maps(mf, model=i), keys=keys) for i in (1, 2)]
        # the specification form: one model after the other through k_splat_scatter / k_global_scatter
        ref = results[(1, 0, False)]
        for form, got in results.items():
            for i in range(2):
                same_bytes(got[i], ref[i], f"object model {i + 1}, (objectScatterSplat, batchObjectPasses, one lane per surfel) = {form}")
        # ... which draws what the background's specification form draws from the same map: the four maps, and the keys' depths
        same_bytes({k: v for k, v in ref[0].items() if k != "keys"}, spec, "object model 1 against the background")
        same_bytes({k: v for k, v in ref[1].items() if k != "keys"}, spec, "object model 2 against the background")
        keys = ref[0]["keys"]
        EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
        assert ((keys == EMPTY) == (spec["keys"] == EMPTY)).all() and ((keys >> np.uint64(32)) == (spec["keys"] >> np.uint64(32)))[keys != EMPTY].all()
        # e for GlobalProjection: both models tie on every pixel -- the lower model order has them all (order 1, id 5)
        assert (keys != EMPTY).sum() > 300 and ((keys[keys != EMPTY] & np.uint64(0xFFFFFFFF)) == np.uint64((1 << 8) | 5)).all()
        # ... and the order decides, not the id: the models' orders swapped
        mf.setTick(TICK)
        swapped = key_image(mf, [-1, 2, 1])
        assert ((swapped[swapped != EMPTY] & np.uint64(0xFFFFFFFF)) == np.uint64((1 << 8) | 6)).all() and ((swapped == EMPTY) == (keys == EMPTY)).all()
    finally:
        mf.close()


# ---------------- 3. the oracle, at the crafted centres that sit on a pixel centre ----------------
def test_centred_classes_against_the_oracle(oracle, crafted, spec):
    cam = oracle.Cam(W, H, F, F, CX, CY)
    img, v, n, tm = oracle.combined_predict(cam, np.eye(4, dtype=np.float32), crafted.S, len(crafted.S), MAX_DEPTH, THR, TICK, TICK, TIME_DELTA)
    checked = 0
    for name, h in crafted.hand.items():
        if not h["centred"] or name[0] not in "cefghj":
            continue
        px, py = h["pixel"]
        print(name, (px, py), "device", winner(spec, (px, py)), spec["pred_vertex"][py, px, 2], "oracle", tuple(img[py, px, :3]), tm[py, px], v[py, px, 2])
        assert winner(spec, (px, py)) == (tuple(int(c) for c in img[py, px, :3]), int(tm[py, px])), name
        assert abs(float(spec["pred_vertex"][py, px, 2]) - float(v[py, px, 2])) <= 1e-5, name
        checked += 1
    assert checked == 13
