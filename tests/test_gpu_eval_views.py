"""View scores on the device: mf_view_score_dev against the numpy restatement of its definition (tests/view_restatement.py), ViewScorer on a
live context, and the driver's -evalviews flag.  Every counter is an integer and every comparison is exact equality.  Runs on the MI355X
(-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import view_restatement as vr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"
TILE_W, TILE_H = 32, 16          # the kernel's tile (kViewTW x kViewTH in csrc/mf_eval_image.hip); its halo is 5
# exactly one SSIM pixel; none at all; odd sizes with no frame start aligned; windows across tile borders and partial last tiles
SHAPES = [(1, 11, 11), (1, 10, 40), (2, 23, 37), (1, 2 * TILE_H + 5, 2 * TILE_W + 6)]
MAX_DEPTH = 4.0
TAU = 0.0078125                  # 2^-7: |dz| = tau exactly is representable (see _depths)


def _dev(a):
    import torch
    from maskfusion_amd.lib import torch_device
    return torch.as_tensor(np.ascontiguousarray(a)).to(torch_device())


def _sync(t):
    import torch
    if t.device.type == "cuda":
        torch.cuda.synchronize()


# ---------------------------------------------------------------- inputs ----------------------------------------------------------------
def _random_bytes(rng, shape):
    F, H, W = shape
    return rng.integers(0, 256, (F, H, W, 4), dtype=np.uint8), rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)


def _smooth(rng, shape):
    """a smooth image, and two noisy copies of it: SSIM well away from 0"""
    F, H, W = shape
    yy, xx = np.mgrid[0:H, 0:W]
    base = np.stack([128 + 90 * np.sin(0.21 * xx + 0.13 * yy + c) * np.cos(0.08 * yy - 0.05 * xx * c) for c in range(4)], -1)
    noisy = lambda n: np.clip(base[None, :, :, :n] + rng.normal(0, 6, (F, H, W, n)), 0, 255).astype(np.uint8)
    return noisy(4), noisy(3)


def _depths(rng, shape):
    """render and input depth with zeros, NaN, +inf, negative values, values just above and below MAX_DEPTH, and -- in the first pixels of
    every frame -- pairs whose fp32 |dz| is exactly TAU, and one float above and below it"""
    F, H, W = shape
    rd = rng.uniform(0.3, 3.9, shape).astype(np.float32)
    d = (rd + rng.normal(0, 0.01, shape)).astype(np.float32)
    for a in (rd, d):
        kind = rng.integers(0, 24, shape)
        a[kind == 0] = 0.0
        a[kind == 1] = np.nan
        a[kind == 2] = np.inf
        a[kind == 3] = -1.5
    kind = rng.integers(0, 20, shape)
    d[kind == 0] = np.float32(MAX_DEPTH)
    d[kind == 1] = np.nextafter(np.float32(MAX_DEPTH), np.float32(np.inf))
    d[kind == 2] = np.nextafter(np.float32(MAX_DEPTH), np.float32(0))
    t = np.float32(TAU)
    pairs = [(1.0 + t, 1.0), (2.0 - t, 2.0), (np.nextafter(np.float32(1.0 + t), np.float32(9)), 1.0), (np.nextafter(np.float32(1.0 + t), np.float32(0)), 1.0)]
    for k, (a, b) in enumerate(pairs):
        rd.reshape(F, -1)[:, k], d.reshape(F, -1)[:, k] = a, b
    dz = np.abs(rd.reshape(F, -1)[0, :4] - d.reshape(F, -1)[0, :4])
    assert dz.dtype == np.float32 and dz[0] == t and dz[1] == t and dz[2] > t and dz[3] < t      # the boundary is hit, and missed by one float either side
    return rd, d


def _case(seed, shape, make):
    rng = np.random.default_rng(seed)
    r, c = make(rng, shape)
    rd, d = _depths(rng, shape)
    return r, rd, c, d


# ---------------------------------------------------------------- the definition ----------------------------------------------------------------
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("make", [_random_bytes, _smooth])
def test_counts_equal_restatement(hip, shape, make):
    """one group, no group image"""
    from maskfusion_amd import eval as ev
    r, rd, c, d = _case(sum(shape), shape, make)
    want = vr.counts(r, rd, c, d, None, 1, MAX_DEPTH, TAU)
    got = ev.view_counts(r, rd, c, d, None, 1, MAX_DEPTH, TAU)
    assert got.dtype == np.uint64 and got.shape == (shape[0], 1, 10)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    F, H, W = shape
    assert (got[:, 0, 0] == H * W).all() and (got[:, 0, 8] == max(0, H - 10) * max(0, W - 10)).all()
    assert (got[:, 0, 4] >= 2).all() and (got[:, 0, 3] > got[:, 0, 4]).all()             # the two pairs at |dz| = tau are within
    if shape == (1, 10, 40):
        assert got[0, 0, 8] == 0 and got[0, 0, 9] == 0 and got[0, 0, 6] > 0
    if make is _smooth and got[0, 0, 8]:
        ssim = got[:, 0, 9].view(np.int64).sum() / vr.FIX / got[:, 0, 8].sum()
        assert 0.3 < ssim < 1.0, ssim                                                      # the inputs are what they are meant to be


def test_no_depth_limit(hip):
    """max_depth = inf (passed on as FLT_MAX): every finite positive input depth is valid"""
    from maskfusion_amd import eval as ev
    r, rd, c, d = _case(8, SHAPES[2], _random_bytes)
    d.reshape(-1)[7] = np.finfo(np.float32).max
    rd.reshape(-1)[7] = 0.0
    got = ev.view_counts(r, rd, c, d)
    assert np.array_equal(got, vr.counts(r, rd, c, d))
    assert got[:, 0, 2].sum() == np.count_nonzero(np.isfinite(d) & (d > 0))


@pytest.mark.parametrize("shape", SHAPES)
def test_groups_over_the_whole_byte_range(hip, shape):
    """64 groups, random group bytes 0..255: three pixels in four are void -- counted nowhere, still read by their neighbours' windows"""
    from maskfusion_amd import eval as ev
    r, rd, c, d = _case(100 + sum(shape), shape, _smooth)
    g = np.random.default_rng(sum(shape)).integers(0, 256, shape, dtype=np.uint8)
    want = vr.counts(r, rd, c, d, g, 64, MAX_DEPTH, TAU)
    got = ev.view_counts(r, rd, c, d, g, 64, MAX_DEPTH, TAU)
    assert np.array_equal(got, want)
    assert got[:, :, 0].sum() == np.count_nonzero(g < 64)


def test_void_frame_between_two_normal_ones(hip):
    from maskfusion_amd import eval as ev
    shape = (3, 23, 37)
    r, rd, c, d = _case(3, shape, _smooth)
    g = np.random.default_rng(3).integers(0, 5, shape, dtype=np.uint8)
    g[1] = 9
    got = ev.view_counts(r, rd, c, d, g, 5, MAX_DEPTH, TAU)
    assert np.array_equal(got, vr.counts(r, rd, c, d, g, 5, MAX_DEPTH, TAU))
    assert not got[1].any() and got[0, :, 0].sum() == got[2, :, 0].sum() == 23 * 37


@pytest.mark.parametrize("shape", SHAPES[2:])
def test_identical_images_score_exactly_one(hip, shape):
    """Render RGB equal to the input RGB: no colour error, and every SSIM value is exactly 1.0.  With x = y the five filtered quantities
    come from the same operations on the same values, so mx = my and Exx = Exy = Eyy bit for bit, hence vx = vy = cxy.  Then
    mx mx + my my = 2 fl(mx mx) = fl(2 mx my) and vx + vy = 2 cxy, both exact (doubling is), so numerator and denominator are the same
    two factors: their quotient is exactly 1.0, the mean of three ones is 1.0, and llrint(1.0 2^24) = 2^24."""
    from maskfusion_amd import eval as ev
    r, rd, c, d = _case(5, shape, _random_bytes)
    r[..., :3] = c
    got = ev.view_counts(r, rd, c, d, None, 1, MAX_DEPTH, TAU)
    assert np.array_equal(got, vr.counts(r, rd, c, d, None, 1, MAX_DEPTH, TAU))
    assert (got[:, 0, 6] == 0).all() and (got[:, 0, 7] == 0).all()
    assert (got[:, 0, 8] > 0).all() and (got[:, 0, 9] == got[:, 0, 8] * (1 << 24)).all()


def _raw_call(L, t_r, t_rd, t_c, t_d, t_g, t_out, **k):
    F, H, W = t_rd.shape
    a = dict(r=t_r.data_ptr(), rd=t_rd.data_ptr(), c=t_c.data_ptr(), d=t_d.data_ptr(), g=t_g.data_ptr() if t_g is not None else None, F=F, H=H, W=W, n=1,
             max_depth=MAX_DEPTH, tau=TAU, out=t_out.data_ptr())
    a.update(k)
    return L.mf_view_score_dev(a["r"], a["rd"], a["c"], a["d"], a["g"], a["F"], a["H"], a["W"], a["n"], a["max_depth"], a["tau"], a["out"], None)


def test_output_is_zeroed(hip):
    """two calls into the same buffer, filled with ones before the first"""
    import torch
    from maskfusion_amd.lib import load
    shape = SHAPES[2]
    r, rd, c, d = _case(6, shape, _smooth)
    g = np.random.default_rng(6).integers(0, 80, shape, dtype=np.uint8)
    tr, trd, tc, td, tg = (_dev(a) for a in (r, rd, c, d, g))
    out = torch.full((shape[0], 64, 10), 0x0101010101010101, dtype=torch.int64, device=trd.device)
    res = []
    for _ in range(2):
        assert _raw_call(load(), tr, trd, tc, td, tg, out, n=64) == 0
        _sync(out)
        res.append(out.cpu().numpy().view(np.uint64).copy())
    assert np.array_equal(res[0], vr.counts(r, rd, c, d, g, 64, MAX_DEPTH, TAU))
    assert np.array_equal(res[1], res[0])


@pytest.mark.parametrize("offsets", [(1, 1, 1), (3, 1, 5), (2, 7, 16)])
def test_views_at_odd_byte_offsets(hip, offsets):
    """the three byte images are views into larger device buffers, at odd offsets from a 16-byte boundary"""
    from maskfusion_amd import eval as ev
    shape = SHAPES[3]
    r, rd, c, d = _case(7, shape, _smooth)
    g = np.random.default_rng(7).integers(0, 6, shape, dtype=np.uint8)
    views = []
    for a, off in zip((r, c, g), offsets):
        big = _dev(np.zeros(a.size + 64, np.uint8))
        base = (-big.data_ptr()) % 16
        v = big[base + off:base + off + a.size].view(a.shape)
        v.copy_(_dev(a))
        assert v.data_ptr() % 16 == off % 16
        views.append(v)
    got = ev.view_counts(views[0], _dev(rd), views[1], _dev(d), views[2], 5, MAX_DEPTH, TAU)
    assert np.array_equal(got, vr.counts(r, rd, c, d, g, 5, MAX_DEPTH, TAU))


def test_argument_checks(hip):
    """every refused call returns MF_EINVAL and leaves a sentinel-filled output untouched"""
    import torch
    from maskfusion_amd.lib import load
    L = load()
    shape = SHAPES[2]
    r, rd, c, d = _case(9, shape, _smooth)
    tr, trd, tc, td = (_dev(a) for a in (r, rd, c, d))
    SENTINEL = 0x5A5A5A5A5A5A5A5A
    out = torch.full((shape[0], 64, 10), SENTINEL, dtype=torch.int64, device=trd.device)
    call = lambda **k: _raw_call(L, tr, trd, tc, td, None, out, **k)
    for key in ("r", "rd", "c", "d", "out"):
        assert call(**{key: None}) == -1, key
    for key in ("W", "H", "F"):
        assert call(**{key: 0}) == -1 and call(**{key: -3}) == -1, key
    assert call(W=4097, H=4096) == -1 and call(W=1 << 16, H=1 << 16) == -1         # more than 2^24 pixels (the second: W H wraps an int32)
    assert call(n=0) == -1 and call(n=65) == -1 and call(n=-1) == -1
    for v in (0.0, -1.0, float("nan")):
        assert call(max_depth=v) == -1, v
    for v in (-1e-9, float("nan"), float("inf"), float("-inf")):
        assert call(tau=v) == -1, v
    _sync(out)
    assert (out.cpu().numpy() == SENTINEL).all()
    # nothing was launched, nothing is broken: valid calls still succeed, FLT_MAX ("no limit") and tau 0 among them
    assert call(max_depth=float(np.finfo(np.float32).max), tau=0.0) == 0
    written = lambda: out.cpu().numpy().view(np.uint64).reshape(-1)[:shape[0] * 10].reshape(shape[0], 1, 10)      # one group: [n_frames][1][10]
    _sync(out)
    assert np.array_equal(written(), vr.counts(r, rd, c, d, None, 1, np.inf, 0.0))
    assert call() == 0
    _sync(out)
    assert np.array_equal(written(), vr.counts(r, rd, c, d, None, 1, MAX_DEPTH, TAU))
    assert (out.cpu().numpy().reshape(-1)[shape[0] * 10:] == SENTINEL).all()


# ---------------------------------------------------------------- a live context ----------------------------------------------------------------
LW, LH, LF = 160, 120, 132.0
LIVE_FRAMES = 15      # tests/test_gpu_eval_seg.py's small scene: the boxes spawn at frames 2, 4 and 6


def _live_run(score):
    """a short multi-model stream; score: scored after every frame by two ViewScorers (the second with R and B of the input swapped), and
    rendered to the host for the comparison"""
    from maskfusion_amd import MaskFusion, synth
    from maskfusion_amd import eval as ev
    st = synth.Stream(W=LW, H=LH, fx=LF, fy=LF, cx=LW / 2.0, cy=LH / 2.0, n_objects=3, noise=True, object_motion=0.0)
    scorers = (ev.ViewScorer(), ev.ViewScorer()) if score else None      # before the context, as ViewScorer asks
    mf = MaskFusion(LW, LH, LF, LF, LW / 2.0, LH / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 17, numOSurfels=1 << 15, enableMultipleModels=True,
                    modelSpawnOffset=2, trackAllModels=False)
    for k, v in dict(mfThreshold=0.3, mfWeightDistance=150.0, mfWeightConvexity=2.8, mfMorphEdgeIterations=0, mfMorphMaskIterations=0,
                     newModelMinRelativeSize=0.003).items():
        mf.setParam(k, v)
    host = []
    for k in range(LIVE_FRAMES):
        rgb, d, mask = st.frame(k)
        mf.processFrame(rgb, d, mask=mask, classIDs=[0, 41, 42, 43], timestamp=k)
        if score:
            scorers[0].add_from(mf, rgb, d)
            scorers[1].add_from(mf, rgb[:, :, ::-1], d)
            host.append((mf.renderView(mf.sensorRenderView(), depth=True, models=True), mf.modelIDs(), rgb, d))
    ms = mf.getModels()
    state = dict(ids=[m.getID() for m in ms], poses=[m.getPose().tobytes() for m in ms], counts=[m.lastCount() for m in ms])
    mf.close()
    return state, scorers, host


def test_scorer_on_a_live_context(hip):
    """One run scored after every frame and one that is not (one test, so that the two runs happen once whichever worker takes it):
    1. device plumbing, id-to-group mapping and stream ordering: add_from's counters are view_counts of the host render of the same view;
    2. scoring changes nothing: the frames processed after it are bit-identical to the run without;
    3. the render's channel order is the input's: the input with R and B swapped scores strictly worse.
    No absolute score is asserted; they are printed (DESIGN.md "View evaluation" quotes them)."""
    from maskfusion_amd import eval as ev
    with_scoring, scorers, host = _live_run(True)
    without, _, _ = _live_run(False)
    # 1.
    assert len(with_scoring["ids"]) >= 2, "the scene must spawn an object"
    got = scorers[0].counts()
    assert got.shape == (LIVE_FRAMES, 64, 10)
    group_of = {}
    for f, ((rgba, dep, mod), ids, rgb, d) in enumerate(host):
        table = np.zeros(len(ids) + 1, np.uint8)
        for i, model_id in enumerate(ids):
            table[i + 1] = group_of.setdefault(model_id, len(group_of) + 1)
        want = ev.view_counts(rgba, dep, rgb, d, table[mod + 1], 64)
        assert np.array_equal(got[f], want[0]), f
        assert want[0, 0, 1] == 0 and want[0, 1:, 1].sum() == want[0, 1:, 0].sum()      # group 0 is exactly what no model drew
    res = scorers[0].result()
    assert res["frames"] == LIVE_FRAMES and np.array_equal(res["counts"], got)
    assert [o["model_id"] for o in res["groups"]] == [None] + list(group_of) and [o["group"] for o in res["groups"]] == list(range(len(group_of) + 1))
    objects = [o for o in res["groups"] if o["group"] >= 2]
    assert objects and all(o["pixels"] > 0 for o in objects)
    print("live context:", json.dumps(ev._clean({k: v for k, v in res.items() if k != "counts"})))
    # 2.
    assert with_scoring == without, "frames processed after scoring must be bit-identical to a run without it"
    # 3.
    colours = np.stack([h[2] for h in host]).astype(np.int64)
    assert np.abs(colours[..., 0] - colours[..., 2]).mean() > 10, "the scene must not be grey"
    straight, swapped = res["summary"]["psnr"], scorers[1].result()["summary"]["psnr"]
    print("pooled PSNR:", straight, "with R and B swapped:", swapped)
    assert swapped < straight


# ---------------------------------------------------------------- the driver ----------------------------------------------------------------
def _python(module, args):
    if EMU:    # the child drives the same CPU-executed build as this process
        return [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import %s as m; "
                "sys.exit(m.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"), module)] + args
    return [sys.executable, "-m", "maskfusion_amd." + module] + args


def test_driver_writes_views_json(hip, tmp_path):
    from maskfusion_amd import eval as ev
    from maskfusion_amd import synth
    from maskfusion_amd.io import writers
    n = 5
    st = synth.Stream(W=LW, H=LH, fx=LF, fy=LF, cx=LW / 2.0, cy=LH / 2.0, n_objects=3, noise=False, object_motion=0.0)
    frames = [st.frame(k) for k in range(n)]
    seq, out = tmp_path / "seq", tmp_path / "out"
    writers.write_image_dir(str(seq), [(f[0], f[1]) for f in frames], masks=[f[2] for f in frames], class_ids=[[0, 41, 42, 43]] * n,
                            calibration=(LF, LF, LW / 2.0, LH / 2.0, LW, LH))
    run = subprocess.run(_python("cli", ["-dir", str(seq), "-evalviews", "-exportdir", str(out), "-q", "-offset", "2", "-segMinNew", "0.003"]),
                         cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert run.returncode == 0, run.stderr
    assert f"processed {n} frames" in run.stdout
    with open(out / "views.json") as f:
        res = json.load(f)
    assert res["frames"] == n == res["summary"]["frames"] and "counts" not in res
    assert res["groups"][0]["model_id"] is None and res["groups"][1]["model_id"] == 0        # nothing drawn; the background
    assert set(ev.VIEW_KEYS) <= set(res["summary"]) and set(ev.VIEW_KEYS) == set(res["summary"]["mean"])
    assert sum(o["pixels"] for o in res["groups"]) == n * LW * LH
