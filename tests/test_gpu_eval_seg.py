"""Segmentation scores on the device: mf_label_confusion_dev and mf_label_boundary_dev against the numpy restatement of their definitions
(tests/seg_restatement.py), SegmentationScorer on a live context, and both command lines end to end.  Every count is an integer and every
comparison is exact equality.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import seg_restatement as sr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"
TILE_W, TILE_H = 64, 32          # the boundary kernel's tile (kBndTW x kBndTH in csrc/mf_eval_image.hip); its halo is radius + 1
RADII = (0, 1, 6, 16)


def _dev(a):
    import torch
    from maskfusion_amd.lib import torch_device
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch_device())


# ---------------------------------------------------------------- region counts ----------------------------------------------------------------
def _random64(rng, shape):
    """labels over the whole byte range, 64 classes per side, void entries in both tables, raw 255 present and mapped to a class on one side"""
    est = rng.integers(0, 256, shape, dtype=np.uint8)
    gt = rng.integers(0, 256, shape, dtype=np.uint8)
    est.flat[0] = 255
    gt.flat[-1] = 255
    le = rng.integers(0, 64, 256).astype(np.uint8)
    lg = rng.integers(0, 64, 256).astype(np.uint8)
    le[rng.random(256) < 0.1] = 255
    lg[rng.random(256) < 0.1] = 255
    le[255], lg[255] = 63, 255
    return est, gt, le, lg, 64, 64


def _one_pair(rng, shape):
    est = rng.integers(0, 256, shape, dtype=np.uint8)
    gt = rng.integers(0, 256, shape, dtype=np.uint8)
    return est, gt, np.zeros(256, np.uint8), np.zeros(256, np.uint8), 1, 1


@pytest.mark.parametrize("shape", [(1, 1, 1), (3, 23, 37), (2, 48, 64), (5, 19, 130)])
@pytest.mark.parametrize("make", [_random64, _one_pair])
def test_confusion_equals_restatement(hip, shape, make):
    from maskfusion_amd import eval as ev
    est, gt, le, lg, ne, ng = make(np.random.default_rng(sum(shape)), shape)
    want = sr.confusion(est, gt, le, lg, ne, ng)
    got = ev.label_confusion(est, gt, le, lg, ne, ng)
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert np.array_equal(got, want)
    if make is _one_pair:
        assert (got.reshape(-1) == shape[1] * shape[2]).all()


def test_confusion_all_void_frame_between_two_normal_ones(hip):
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(3)
    est = rng.integers(0, 5, (3, 23, 37), dtype=np.uint8)
    gt = rng.integers(0, 4, (3, 23, 37), dtype=np.uint8)
    gt[1] = 9
    le = np.full(256, 255, np.uint8)
    lg = np.full(256, 255, np.uint8)
    le[:5] = np.arange(5)
    lg[:4] = np.arange(4)
    got = ev.label_confusion(est, gt, le, lg, 5, 4)
    assert np.array_equal(got, sr.confusion(est, gt, le, lg, 5, 4))
    assert not got[1].any() and got[0].sum() == got[2].sum() == 23 * 37


def test_confusion_zeroes_its_output(hip):
    """two calls into the same buffer, filled with ones before the first"""
    import torch
    from maskfusion_amd.lib import load
    L = load()
    est, gt, le, lg, ne, ng = _random64(np.random.default_rng(4), (3, 23, 37))
    e, g = _dev(est), _dev(gt)
    out = torch.full((3, ng, ne), 0x01010101, dtype=torch.int32, device=e.device)
    res = []
    for _ in range(2):
        assert L.mf_label_confusion_dev(e.data_ptr(), g.data_ptr(), 3, 23, 37, le.ctypes.data, ne, lg.ctypes.data, ng, out.data_ptr(), None) == 0
        if e.device.type == "cuda":
            torch.cuda.synchronize()
        res.append(out.cpu().numpy().view(np.uint32).copy())
    assert np.array_equal(res[0], sr.confusion(est, gt, le, lg, ne, ng))
    assert np.array_equal(res[1], res[0])


@pytest.mark.parametrize("offsets", [(1, 1), (1, 3), (5, 16)])
def test_confusion_on_views_at_odd_byte_offsets(hip, offsets):
    """device tensors that are views into larger buffers: both streams misaligned alike (the wide loads' aligned middle), differently, and one only"""
    from maskfusion_amd import eval as ev
    shape = (2, 48, 64)
    est, gt, le, lg, ne, ng = _random64(np.random.default_rng(5), shape)
    n = est.size
    views = []
    for a, off in zip((est, gt), offsets):
        big = _dev(np.zeros(n + 64, np.uint8))
        base = (-big.data_ptr()) % 16                      # the buffer's first 16-byte boundary
        v = big[base + off:base + off + n].view(shape)
        v.copy_(_dev(a))
        assert v.data_ptr() % 16 == off % 16
        views.append(v)
    assert np.array_equal(ev.label_confusion(views[0], views[1], le, lg, ne, ng), sr.confusion(est, gt, le, lg, ne, ng))


# ---------------------------------------------------------------- boundary counts ----------------------------------------------------------------
def _identity_lut(n):
    """raw value v < n is class v, every other raw value (200 in the hand-made cases) is void"""
    lut = np.full(256, 255, np.uint8)
    lut[:n] = np.arange(n)
    return lut


def _blobs(seed, shape, n_obj=4):
    """unions of discs per object; the estimate is the ground truth with every disc moved and resized a little"""
    rng = np.random.default_rng(seed)
    F, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    est, gt = np.zeros(shape, np.uint8), np.zeros(shape, np.uint8)
    for f in range(F):
        for k in range(1, n_obj + 1):
            for _ in range(3):
                cx, cy, r = rng.uniform(0, W), rng.uniform(0, H), rng.uniform(2, 0.3 * min(H, W))
                gt[f][(xx - cx) ** 2 + (yy - cy) ** 2 <= r * r] = k
                dx, dy, dr = rng.uniform(-3, 3, 3)
                est[f][(xx - cx - dx) ** 2 + (yy - cy - dy) ** 2 <= (r + dr) ** 2] = k
    return est, gt


@pytest.mark.parametrize("radius", RADII)
@pytest.mark.parametrize("shape", [(2, 23, 37), (1, 80, 96), (3, 67, 131)])
def test_boundary_equals_restatement_on_blobs(hip, shape, radius):
    from maskfusion_amd import eval as ev
    est, gt = _blobs(shape[1] + radius, shape)
    lut = _identity_lut(5)
    pair = np.array([0, 2, 1, 255, 4], np.uint8)          # a swap and a class matched to nothing
    want = sr.boundary(est, gt, lut, lut, 5, pair, radius)
    got = ev.label_boundary(est, gt, lut, lut, pair, radius, n_est=5)
    assert got.dtype == np.uint32 and np.array_equal(got, want)
    assert want[:, :, 2].sum() > 0 and (want[:, 3, :2] == 0).all() and (want[:, 3, 3] == 0).all()


H0, W0 = 67, 131      # more than two tiles each way and no multiple of the tile


def _shift(img, dx, dy):
    """img moved by (dx, dy), zeros moving in"""
    out = np.zeros_like(img)
    H, W = img.shape
    out[max(0, dy):min(H, H + dy), max(0, dx):min(W, W + dx)] = img[max(0, -dy):min(H, H - dy), max(0, -dx):min(W, W - dx)]
    return out


def _handmade(radius):
    """(est, gt, names): one frame per case, classes 0..8, raw 200 = void"""
    frames, names = [], []

    def case(name, gt, est):
        frames.append((est.astype(np.uint8), gt.astype(np.uint8)))
        names.append(name)

    z = lambda: np.zeros((H0, W0), np.uint8)
    # one rectangle per image border and per corner; the estimate one pixel off, so its rectangles leave two borders
    g = z()
    g[0:9, 20:50], g[H0 - 7:, 60:100], g[20:40, 0:11], g[30:50, W0 - 5:] = 1, 2, 3, 4
    g[0:5, 0:6], g[0:4, W0 - 9:], g[H0 - 6:, 0:3], g[H0 - 3:, W0 - 4:] = 5, 6, 7, 8
    case("borders and corners", g, _shift(g, 1, 1))
    case("borders and corners, the same on both sides", g, g)
    # a one-pixel object, on a tile corner; and the estimate moved by exactly the radius / one more, along x, y and a diagonal whose squared
    # length crosses radius^2: (d, d) with 2 d^2 <= radius^2 < 2 (d + 1)^2
    d = int(np.floor(radius / np.sqrt(2.0)))
    assert 2 * d * d <= radius * radius < 2 * (d + 1) * (d + 1)
    for dx, dy in ((0, 0), (radius, 0), (radius + 1, 0), (0, radius), (0, radius + 1), (-radius, 0), (0, -radius - 1), (d, d), (d + 1, d + 1), (-d - 1, d + 1)):
        g = z()
        g[TILE_H, TILE_W] = 1
        case(f"one pixel moved by ({dx}, {dy})", g, _shift(g, dx, dy))
    # a rectangle whose edges lie on tile edges, the estimate moved by the radius and one more along x and y
    g = z()
    g[TILE_H:2 * TILE_H, TILE_W:2 * TILE_W] = 2
    for dx, dy in ((radius, 0), (radius + 1, 0), (0, radius), (0, -radius - 1)):
        case(f"tile-sized rectangle moved by ({dx}, {dy})", g, _shift(g, dx, dy))
    # two classes interleaved as a checkerboard: every pixel is a boundary pixel; the estimate is the inverse
    yy, xx = np.mgrid[0:H0, 0:W0]
    case("checkerboard", 1 + (xx + yy) % 2, 1 + (xx + yy + 1) % 2)
    # blocks whose edges run along every multiple of 8 (so of 16, 32 and 64: every tile edge), and one pixel to either side of them; the
    # estimate's edges one pixel further: the partner boundary lies across the tile edge
    for off in (-1, 0, 1):
        blocks = lambda o: 1 + ((xx - o) // 8 + (yy - o) // 8) % 2
        case(f"8 x 8 blocks, edges at 8 k + {off}", blocks(off), blocks(off + 1))
        case(f"8 x 8 blocks, edges at 8 k + {off}, partner behind", blocks(off), blocks(off - 1))
    # void stripes through an object, other ones through its estimate
    g = z()
    g[10:60, 10:120] = 5
    e = _shift(g, 2, -1)
    g[:, 30:33], g[25, :], g[:, TILE_W - 1] = 200, 200, 200
    e[:, 31:36], e[TILE_H, :] = 200, 200
    case("void stripes", g, e)
    # two ground-truth classes that name the same estimate class (5 and 6 -> 5)
    g = z()
    g[5:40, 5:70], g[5:40, 70:125] = 5, 6
    e = z()
    e[6:41, 6:124] = 5
    case("two objects against one", g, e)
    return np.stack([f[0] for f in frames]), np.stack([f[1] for f in frames]), names


HAND_PAIR = np.array([0, 1, 2, 255, 4, 5, 5, 7, 8], np.uint8)     # class 3 matched to nothing, 5 and 6 both to 5


@pytest.mark.parametrize("radius", RADII)
def test_boundary_equals_restatement_on_handmade_cases(hip, radius):
    from maskfusion_amd import eval as ev
    est, gt, names = _handmade(radius)
    lut = _identity_lut(9)
    want = sr.boundary(est, gt, lut, lut, 9, HAND_PAIR, radius)
    got = ev.label_boundary(est, gt, lut, lut, HAND_PAIR, radius, n_est=9)
    for f, name in enumerate(names):
        assert np.array_equal(got[f], want[f]), (name, radius, got[f].tolist(), want[f].tolist())
    # what the definitions say outright
    for f, name in enumerate(names):
        if name.startswith("one pixel moved by"):
            dx, dy = (int(v) for v in name[name.index("(") + 1:-1].split(","))
            hit = int(dx * dx + dy * dy <= radius * radius)
            assert got[f, 1].tolist() == [1, hit, 1, hit], name
        if name == "checkerboard":
            assert got[f, 1, 0] + got[f, 2, 0] == H0 * W0 == got[f, 1, 2] + got[f, 2, 2]
        if name == "borders and corners, the same on both sides":
            assert (got[f, :, 0] == got[f, :, 1])[HAND_PAIR == np.arange(9)].all() and got[f, 3].tolist() == [0, 0, int(want[f, 3, 2]), 0] and want[f, 3, 2] > 0
            assert got[f, 5, 2] == 5 + 6 - 1                    # the corner rectangle 5 x 6: its two sides inside the image
    assert (got[:, 3, [0, 1, 3]] == 0).all()


def test_counts_are_deterministic_and_frame_order_free(hip):
    from maskfusion_amd import eval as ev
    est, gt = _blobs(11, (4, 67, 131))
    lut = _identity_lut(5)
    pair = np.array([0, 1, 2, 3, 4], np.uint8)
    c0, b0 = ev.label_confusion(est, gt, lut, lut, 5, 5), ev.label_boundary(est, gt, lut, lut, pair, 6, n_est=5)
    for _ in range(4):
        assert np.array_equal(ev.label_confusion(est, gt, lut, lut, 5, 5), c0)
        assert np.array_equal(ev.label_boundary(est, gt, lut, lut, pair, 6, n_est=5), b0)
    assert np.array_equal(ev.label_confusion(est[::-1], gt[::-1], lut, lut, 5, 5), c0[::-1])
    assert np.array_equal(ev.label_boundary(est[::-1], gt[::-1], lut, lut, pair, 6, n_est=5), b0[::-1])


def test_argument_checks(hip):
    import torch
    from maskfusion_amd.lib import load
    L = load()
    F, H, W, n = 2, 23, 37, 5
    est, gt = _blobs(12, (F, H, W))
    e, g = _dev(est), _dev(gt)
    lut = _identity_lut(n)
    pair = np.arange(n, dtype=np.uint8)
    counts = torch.zeros((F, n, n), dtype=torch.int32, device=e.device)
    rows = torch.zeros((F, n, 4), dtype=torch.int32, device=e.device)

    def conf(**k):
        a = dict(e=e.data_ptr(), g=g.data_ptr(), F=F, H=H, W=W, le=lut.ctypes.data, ne=n, lg=lut.ctypes.data, ng=n, out=counts.data_ptr())
        a.update(k)
        return L.mf_label_confusion_dev(a["e"], a["g"], a["F"], a["H"], a["W"], a["le"], a["ne"], a["lg"], a["ng"], a["out"], None)

    def bnd(**k):
        a = dict(e=e.data_ptr(), g=g.data_ptr(), F=F, H=H, W=W, le=lut.ctypes.data, ne=n, lg=lut.ctypes.data, ng=n, pair=pair.ctypes.data, r=3,
                 out=rows.data_ptr())
        a.update(k)
        return L.mf_label_boundary_dev(a["e"], a["g"], a["F"], a["H"], a["W"], a["le"], a["ne"], a["lg"], a["ng"], a["pair"], a["r"], a["out"], None)

    bad_lut = lut.copy()
    bad_lut[7] = n                        # neither < n nor 255
    bad_pair = pair.copy()
    bad_pair[2] = n
    for call in (conf, bnd):
        for key in ("e", "g", "le", "lg", "out"):
            assert call(**{key: None}) == -1, (call.__name__, key)
        for key in ("W", "H", "F"):
            assert call(**{key: 0}) == -1 and call(**{key: -3}) == -1, (call.__name__, key)
        for key in ("ne", "ng"):
            assert call(**{key: 0}) == -1 and call(**{key: 65}) == -1, (call.__name__, key)
        assert call(le=bad_lut.ctypes.data) == -1 and call(lg=bad_lut.ctypes.data) == -1
        assert call(ne=n - 1) == -1       # the table's entry n - 1 is out of range for n - 1 classes
    assert bnd(pair=None) == -1
    assert bnd(pair=bad_pair.ctypes.data) == -1
    assert bnd(r=-1) == -1 and bnd(r=17) == -1
    # nothing was launched, nothing is broken: valid calls still succeed
    assert conf() == 0 and bnd() == 0 and bnd(r=0) == 0 and bnd(r=16) == 0
    if e.device.type == "cuda":
        torch.cuda.synchronize()
    assert np.array_equal(counts.cpu().numpy().view(np.uint32), sr.confusion(est, gt, lut, lut, n, n))
    assert np.array_equal(rows.cpu().numpy().view(np.uint32), sr.boundary(est, gt, lut, lut, n, pair, 16))


# ---------------------------------------------------------------- a live context ----------------------------------------------------------------
LW, LH, LF = 160, 120, 132.0
LIVE_FRAMES = 20      # the boxes spawn at frames 2, 4 and 6 and score J = 0.55 .. 0.75 per frame from then on (the label stage keeps off the
                      # geometric edges, so a model's label is smaller than the instance mask); the frames before a spawn count as misses, so
                      # a sequence IoU above 0.5 needs a run this long: 0.552 (object 1), 0.451 and 0.517 (object 3), on the MI355X and on the CPU-executed build alike.
                      # (Not longer: at frame 21 this camera path loses all three models and the run spawns new ones.)


def _live_run(score):
    """a short multi-model stream (tests/test_gpu_multimodel.py's small scene at 160 x 120); score: a SegmentationScorer fed after every frame"""
    from maskfusion_amd import MaskFusion, synth
    st = synth.Stream(W=LW, H=LH, fx=LF, fy=LF, cx=LW / 2.0, cy=LH / 2.0, n_objects=3, noise=True, object_motion=0.0)
    mf = MaskFusion(LW, LH, LF, LF, LW / 2.0, LH / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 17, numOSurfels=1 << 15, enableMultipleModels=True,
                    modelSpawnOffset=2, trackAllModels=False)
    for k, v in dict(mfThreshold=0.3, mfWeightDistance=150.0, mfWeightConvexity=2.8, mfMorphEdgeIterations=0, mfMorphMaskIterations=0,
                     newModelMinRelativeSize=0.003).items():
        mf.setParam(k, v)
    segs, masks = [], []
    for k in range(LIVE_FRAMES):
        rgb, d, mask = st.frame(k)
        mf.processFrame(rgb, d, mask=mask, classIDs=[0, 41, 42, 43], timestamp=k)
        if score is not None:
            score.add_from(mf, mask)
            segs.append(mf.downloadSegmentation())
            masks.append(mask)
    ms = mf.getModels()
    state = dict(ids=[m.getID() for m in ms], poses=[m.getPose().tobytes() for m in ms], counts=[m.lastCount() for m in ms])
    mf.close()
    return state, np.array(segs), np.array(masks)


def test_scorer_on_a_live_context(hip):
    from maskfusion_amd import eval as ev
    sc = ev.SegmentationScorer()
    with_scoring, segs, masks = _live_run(sc)
    without, _, _ = _live_run(None)
    assert with_scoring == without, "scoring must change nothing"
    assert len(with_scoring["ids"]) >= 2, "the scene must spawn an object"
    res = sc.result()
    (le, est_ids), (lg, gt_ids) = sc.tables()
    assert le[255] == 0 and gt_ids == sorted(set(masks.reshape(-1).tolist()) | {0})
    counts = sr.confusion(segs, masks, le, lg, len(est_ids), len(gt_ids))
    assert np.array_equal(res["counts"], counts)
    r = ev.default_radius(LW, LH)
    assert res["summary"]["radius"] == r == 2
    want = ev.seg_metrics(counts, lambda pair: sr.boundary(segs, masks, le, lg, len(gt_ids), pair, r), gt_ids, est_ids)
    assert res["objects"] == want["objects"] and res["summary"] == dict(want["summary"], radius=r)
    spawned = [o for o in res["objects"] if o["model_id"] is not None]
    print("live context:", json.dumps(res["objects"]), json.dumps(res["summary"]))
    assert spawned and max(o["iou"] for o in spawned) > 0.5      # a sanity condition, not a measurement


# ---------------------------------------------------------------- both command lines ----------------------------------------------------------------
def _python(module, args):
    if EMU:    # the child drives the same CPU-executed build as this process
        return [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import %s as m; "
                "sys.exit(m.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"), module)] + args
    return [sys.executable, "-m", "maskfusion_amd." + module] + args


@pytest.mark.parametrize("start_index", [0, 1])
def test_both_command_lines_end_to_end(hip, tmp_path, start_index):
    from maskfusion_amd import eval as ev
    from maskfusion_amd import synth
    from maskfusion_amd.io import writers
    from maskfusion_amd.io.readers import load_mask
    n = 7
    st = synth.Stream(W=LW, H=LH, fx=LF, fy=LF, cx=LW / 2.0, cy=LH / 2.0, n_objects=3, noise=False, object_motion=0.0)
    frames = [st.frame(k) for k in range(n)]
    masks = [f[2] for f in frames]
    assert all(not np.array_equal(masks[k], masks[k + 1]) for k in range(n - 1))     # the camera moves: pairing a tick with another mask changes the counts
    seq, out = tmp_path / "seq", tmp_path / "out"
    writers.write_image_dir(str(seq), [(f[0], f[1]) for f in frames], masks=masks, class_ids=[[0, 41, 42, 43]] * n,
                            calibration=(LF, LF, LW / 2.0, LH / 2.0, LW, LH), start_index=start_index)
    run = subprocess.run(_python("cli", ["-dir", str(seq), "-es", "-exportdir", str(out), "-q", "-offset", "2", "-segMinNew", "0.003"]),
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    ticks = sorted(int(fn[len("Segmentation"):-4]) for fn in os.listdir(out) if fn.startswith("Segmentation"))
    assert ticks == list(range(2, n + 1))                         # -es writes from the second frame on
    res = subprocess.run(_python("eval", ["--est", str(out), "--seg-gt", str(seq)]), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr
    lines = [json.loads(l) for l in res.stdout.strip().split("\n")]
    # the same files read directly: tick t <-> mask file index t - 1 + start_index, i.e. the mask of frame t - 1
    est = np.stack([load_mask(str(out / f"Segmentation{t}.png")) for t in ticks])
    gt = np.stack([load_mask(str(seq / f"Mask{t - 1 + start_index:04d}.png")) for t in ticks])
    assert np.array_equal(gt, np.stack([masks[t - 1] for t in ticks]))
    (le, est_ids), (lg, gt_ids) = ev.build_lut(np.unique(est)), ev.build_lut(np.unique(gt))
    r = ev.default_radius(LW, LH)
    counts = sr.confusion(est, gt, le, lg, len(est_ids), len(gt_ids))
    want = ev.seg_metrics(counts, lambda pair: sr.boundary(est, gt, le, lg, len(gt_ids), pair, r), gt_ids, est_ids)
    assert gt_ids == [0, 1, 2, 3]                                 # background and the boxes
    objs = [dict(segmentation_object=o["gt_id"], **{k: v for k, v in o.items() if k != "gt_id"}) for o in want["objects"]]
    assert lines[:-1] == json.loads(json.dumps(objs))
    assert lines[-1] == json.loads(json.dumps({"segmentation": dict(want["summary"], radius=r, first_tick=2, last_tick=n)}))
