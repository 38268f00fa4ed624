"""Headless rendering of the surfel maps (mf_render_view, MaskFusion.renderView) against the numpy restatement in render_restatement.py, and
the render's promise to change nothing.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import os
import numpy as np
import pytest

import render_restatement as rr

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, F = 320, 240, 264.0
SEG = (("mfThreshold", 0.3), ("mfWeightDistance", 150.0), ("mfWeightConvexity", 2.8), ("mfMorphEdgeIterations", 0), ("mfMorphMaskIterations", 0),
       ("newModelMinRelativeSize", 0.004))
CLS = [0, 41, 42]
PALETTE = np.array([[0.9, 0.1, 0.1], [0.1, 0.8, 0.2], [0.2, 0.3, 0.95], [0.9, 0.8, 0.1], [0.6, 0.2, 0.7]], np.float32)


def _context(**kw):
    from maskfusion_amd import MaskFusion
    m = MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, numOSurfels=1 << 16, enableMultipleModels=True,
                   modelSpawnOffset=3, trackAllModels=True, initConfidenceGlobal=1.0,
                   initConfidenceObject=0.01, **kw)
    for k, v in SEG:
        m.setParam(k, v)
    return m


def _frames(n):
    from maskfusion_amd import synth
    st = synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, n_objects=2, noise=True, object_motion=1.0)
    return st, [st.frame(k) for k in range(n)]


@pytest.fixture(scope="module")
def scene(hip):
    _, frames = _frames(7)
    m = _context()
    for k, (rgb, depth, mask) in enumerate(frames):
        m.processFrame(rgb, depth, mask=mask, classIDs=CLS, timestamp=k)
    assert len(m.getModels()) >= 2, "the stream must spawn an object model"
    yield m
    m.close()


def _camera_view(m):
    """the follow view with the camera's own focal length (at this image size fx = 420 crops the boxes out of the follow view)"""
    v = m.defaultRenderView(W, H)
    v.fx = v.fy = F
    return v


def _views(m):
    from maskfusion_amd.lib import RenderView
    follow = m.defaultRenderView(W, H)
    out = []
    for bg, ob in ((1, 1), (2, 4), (3, 3), (4, 4), (2, 2)):
        v = m.defaultRenderView(W, H)
        v.background_color_type, v.object_color_type = bg, ob
        out.append((f"follow types {bg}/{ob}", v))
    v = m.defaultRenderView(W, H); v.draw_points = 1; v.background_color_type = 1; v.object_color_type = 2
    out.append(("points", v))
    v = m.defaultRenderView(W, H); v.draw_unstable = 1; v.draw_window = 1; v.object_color_type = 4
    out.append(("unstable + window", v))
    v = _camera_view(m); v.draw_background = 0; v.object_color_type = 4
    out.append(("objects only", v))
    v = _camera_view(m); v.object_color_type = 4
    out.append(("camera view, labels", v))
    v = m.defaultRenderView(W, H); v.draw_objects = 0; v.background_color_type = 1
    out.append(("background only", v))
    # a free pose with other intrinsics and size: beside and above the follow view, looking back at the scene
    from maskfusion_amd import synth
    free = RenderView()
    free.width, free.height, free.fx, free.fy, free.cx, free.cy, free.near_z, free.far_z = 200, 150, 150.0, 160.0, 97.0, 80.0, 0.1, 50.0
    T = follow.pose() @ synth.make_pose(synth.rot_xyz(0.15, -0.3, 0.05), [0.4, -0.2, -0.3])
    free.set_pose(T)
    free.background_color_type, free.object_color_type, free.draw_background, free.draw_objects = 2, 4, 1, 1
    free.clear_rgba[:] = [10, 20, 30, 255]
    out.append(("free pose", free))
    return out


def test_render_agrees_with_restatement(scene):
    m = scene
    for name, v in _views(m):
        rgba, dep, mod = m.renderView(v, palette=PALETTE, depth=True, models=True)
        r_rgba, r_dep, r_mod, amb = rr.render(m, v, PALETTE)
        ok = ~amb
        n_amb = int(amb.sum())
        drawn = int((r_mod >= 0).sum())
        cdiff = np.abs(rgba.astype(int) - r_rgba.astype(int)).max(2)
        bad_c = int(((cdiff > 1) & ok).sum())
        bad_m = int(((mod != r_mod) & ok).sum())
        both = ok & (r_mod >= 0)
        rel = np.abs(dep[both] - r_dep[both]) / np.maximum(np.abs(r_dep[both]), 1e-30)
        print(name, "drawn", drawn, "ambiguous", n_amb, "colour mismatches", bad_c, "model mismatches", bad_m, "max depth rel", rel.max() if rel.size else 0)
        assert drawn > (0 if name == "objects only" else 0.05 * v.width * v.height), name
        assert bad_m == 0 and bad_c == 0, name
        assert rel.size == 0 or rel.max() <= 1e-5, name
        # (ambiguous: up to ~0.25 % of these renders, bound 0.5 %: the margins of render_restatement.py cover fp32's cancellation at the rim and
        # the 1 / cos growth of a grazing ray's depth error, and a fused surface is overlapping coplanar discs everywhere)
        assert (dep[ok & (r_mod < 0)] == 0).all() and n_amb < 5e-3 * v.width * v.height, name
    v = _camera_view(m)
    v.object_color_type = 4
    _, mod = m.renderView(v, palette=PALETTE, models=True)
    assert (mod > 0).any(), "an object model must be in view"


def _run(frames, render_every, object_stream=True, dev=False):
    import torch
    from gpu_util import empty
    m = _context()
    m.setParam("objectStream", int(object_stream))
    out = dict(pose=[], cnt=[], seg=[])
    d_rgba = empty((H, W, 4), torch.uint8) if dev else None
    d_dep = empty((H, W)) if dev else None
    for k, (rgb, depth, mask) in enumerate(frames):
        m.processFrame(rgb, depth, mask=mask, classIDs=CLS, timestamp=k)
        if render_every:
            v = _camera_view(m)
            v.object_color_type = 4
            m.renderView(v, palette=PALETTE, depth=True, models=True)
            if dev:
                m.renderViewDevice(v, d_rgba.data_ptr(), d_dep.data_ptr(), 0, palette=PALETTE)
        models = m.getModels()
        out["pose"].append([x.getPose() for x in models])
        out["cnt"].append([x.lastCount() for x in models])
        out["seg"].append(m.downloadSegmentation())
    out["maps"] = [x.downloadMap().tobytes() for x in m.getModels()]
    m.close()
    return out


@pytest.mark.parametrize("object_stream", [False, True])
def test_render_changes_nothing(hip, object_stream):
    _, frames = _frames(6)
    a = _run(frames, False, object_stream)
    b = _run(frames, True, object_stream, dev=True)
    assert a["cnt"] == b["cnt"]
    for pa, pb in zip(a["pose"], b["pose"]):
        assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    assert all(np.array_equal(x, y) for x, y in zip(a["seg"], b["seg"]))
    assert a["maps"] == b["maps"]


def test_sparse_map_renders_like_dense_upload(hip):
    from maskfusion_amd import MaskFusion, synth
    st = synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=True)
    m = MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, enableMultipleModels=False,
                   initConfidenceGlobal=1.0)
    m.setParam("bigMapElements", 1000)      # the background is kept as runs and cleaned in place
    for k in range(6):
        rgb, depth, _ = st.frame(k)
        m.processFrame(rgb, depth, timestamp=k)
    views = []
    for t in (1, 2):
        v = m.defaultRenderView(W, H)
        v.background_color_type = t
        views.append(v)
    v = m.defaultRenderView(W, H); v.draw_unstable = 1; v.background_color_type = 3
    views.append(v)
    got = [m.renderView(v, depth=True) for v in views]
    surfels = m.getBackgroundModel().downloadMap()
    tick = m.getTick()
    m2 = MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, enableMultipleModels=False,
                   initConfidenceGlobal=1.0)
    rgb, depth, _ = st.frame(0)
    m2.processFrame(rgb, depth, timestamp=0)
    m2.getBackgroundModel().uploadMap(surfels)
    m2.setTick(tick)
    for (c1, d1), v in zip(got, views):
        v2 = m2.defaultRenderView(W, H)   # (only its size matters: the view's pose is the first context's)
        v2.pose16[:] = v.pose16[:]
        v2.background_color_type, v2.draw_unstable = v.background_color_type, v.draw_unstable
        c2, d2 = m2.renderView(v2, depth=True)
        assert (d1 > 0).mean() > 0.3
        assert np.array_equal(c1, c2) and np.array_equal(d1, d2)
    m.close(); m2.close()


def test_render_deterministic_and_arguments(scene):
    from maskfusion_amd.lib import MFError
    m = scene
    v = _camera_view(m)
    v.object_color_type = 4
    a = m.renderView(v, palette=PALETTE, depth=True, models=True)
    b = m.renderView(v, palette=PALETTE, depth=True, models=True)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    L = m._L
    import ctypes as C
    out = np.zeros((H, W, 4), np.uint8)
    for wh in ((0, 10), (10, 0), (5000, 10), (10, 4097)):
        bad = m.defaultRenderView(W, H)
        bad.width, bad.height = wh
        assert L.mf_render_view(m._h, C.byref(bad), None, 0, out.ctypes.data, None, None) == -1
        assert m._L.mf_last_error(m._h)
    assert L.mf_render_view(m._h, C.byref(v), None, 0, None, None, None) == -1
    bad = m.defaultRenderView(W, H)
    bad.model_mask = 1 << 40
    assert L.mf_render_view(m._h, C.byref(bad), None, 0, out.ctypes.data, None, None) == -1
    with pytest.raises(MFError):
        m.renderView(v, palette=np.zeros((0, 3), np.float32))
    assert L.mf_default_render_view(m._h, 0, 10, 0, C.byref(bad)) == -1
    c = m.renderView(v, palette=PALETTE, depth=True, models=True)   # still usable, same bytes
    assert all(np.array_equal(x, y) for x, y in zip(a, c))
    # the library's palette (palette=None) indexes classes modulo its length
    pal = m.defaultPalette()
    assert pal.shape == (64, 3) and (pal >= 0).all() and (pal <= 1).all()
    d1 = m.renderView(v)
    d2 = m.renderView(v, palette=pal)
    assert np.array_equal(d1, d2)


def test_cli_writes_label_normal_viewport_series(hip, tmp_path):
    from maskfusion_amd.io import writers
    from PIL import Image
    st, frames = _frames(5)
    seq = tmp_path / "seq"
    writers.write_image_dir(str(seq), [(f[0], f[1]) for f in frames], masks=[f[2] for f in frames], class_ids=[CLS] * len(frames),
                            calibration=(F, F, W / 2.0, H / 2.0, W, H))
    out = tmp_path / "out"
    from maskfusion_amd import cli
    assert cli.main(["-dir", str(seq) + os.sep, "-maskdir", str(seq) + os.sep, "-run", "-q", "-el", "-en", "-ev", "-offset", "3", "-segMinNew", "0.004",
                     "-exportdir", str(out) + os.sep]) == 0
    for tick in range(1, len(frames) + 1):
        for name in ("Labels", "Normals", "Viewport"):
            p = out / f"{name}{tick}.png"
            assert p.exists(), p
            im = np.asarray(Image.open(p))
            assert im.shape[:2] == (980, 1280), im.shape
    # object pixels of the label image carry the palette's colours for their class (x max(|n.(1,1,1)|, 0.8), so: a positive multiple)
    from maskfusion_amd import MaskFusion
    pal = MaskFusion.defaultPalette()
    im = np.asarray(Image.open(out / f"Labels{len(frames)}.png"))[:, :, :3].astype(np.float64)
    cols = [pal[c % len(pal)] for c in CLS[1:]]
    hits = 0
    for c in cols:
        s = im / 255.0 / np.maximum(c, 1e-6)
        ratio_ok = (np.abs(s - s.mean(2, keepdims=True)) < 0.02).all(2) & (s.mean(2) >= 0.79)
        hits += int(ratio_ok.sum())
    assert hits > 500, hits
