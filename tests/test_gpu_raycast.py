"""Mesh rendering on the device (mf_trimesh_raycast_dev / mf_trimesh_render_dev, maskfusion_amd.eval.TriMesh.raycast / render, the meshseq
command, the mesh command's --views) against the numpy restatement of tests/raycast_restatement.py.  Runs on the MI355X (-m gpu) and, with
MF_EMU=1, on the CPU-executed build.

The gates.  The device and the restatement evaluate the same fp64 operations in the same order, none contracted, so the winning triangle
and the facing flag are the restatement's EXACTLY (ties included: the smallest index), and t and uv are bit-equal to the fp32 rounding of
the restated fp64 values -- which asks the hardware's fp64 division to be numpy's, correctly rounded."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_restatement as rr  # noqa: E402
import trimesh_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"

_cache = {}


def _fixture(name):
    """mesh, rays and the restatement's answer, computed once and shared (treat as read-only)"""
    if name not in _cache:
        if name == "sphere":
            V, F = tr.icosphere()
            assert V.shape == (162, 3) and F.shape == (320, 3) and (V.min(0) < 0).all() and (V.max(0) > 0).all()
            O, D, expect, groups = rr.sphere_rays(V, F)
            F, cell = rr.with_duplicates(F, 51), 0.05
        else:
            V, F, R, c2 = tr.mixed_mesh()
            assert len(F) == 1602
            O, D, expect, groups = rr.mixed_rays(V, F, R, c2)
            F, cell = rr.with_duplicates(F, 52), 0.02
        ref = rr.raycast(V, F, O, D)
        hit = ref["tri"] >= 0
        print("%s: %d triangles, %d rays, %d hits; rays per (kz, sign): %s" % (
            name, len(F), len(O), hit.sum(), [int(((ref["kz"] == k) & (ref["neg"] == s)).sum()) for k in range(3) for s in (False, True)]))
        # the fixture itself first: what is aimed at the surface hits, what grazes misses -- a fixture that drifts fails here, loudly
        assert 1900 <= len(O) <= 2300
        assert hit[expect == 1].all() and not hit[expect == 0].any() and (expect == 1).sum() > 1400 and (expect == 0).sum() > 150
        assert (~ref["valid"]).sum() == 6
        for kz in range(3):
            for neg in (False, True):
                assert ((ref["kz"] == kz) & (ref["neg"] == neg) & hit).sum() >= 2
        assert ref["front"].sum() > 300 and (hit & ~ref["front"]).sum() > 300                  # both sides are met
        assert (ref["tri"] < len(F) - 20).all()                                                # a duplicate never wins
        if name == "mixed":
            assert ((ref["tri"] >= 0) & (ref["tri"] < 2)).sum() > 300 and (ref["tri"] >= 2).sum() > 300      # wide and gridded triangles both win
        _cache[name] = dict(V=V, F=F, O=O, D=D, cell=cell, ref=ref, groups=groups, expect=expect)
    return _cache[name]


def _bits(a):
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (_bits(a) == _bits(b)).all()


def _check(ref, t, tri, uv, front):
    assert t.dtype == np.float32 and tri.dtype == np.int32 and uv.dtype == np.float32 and front.dtype == np.bool_
    bad = np.flatnonzero(tri != ref["tri"])
    with np.errstate(invalid="ignore"):
        dt = np.abs(np.where(np.isfinite(t), t, 0) - np.where(np.isfinite(ref["t"]), ref["t"], 0))
    print("triangles that differ: %d; t: %d not bit-equal, max |diff| %.3g; uv: %d not bit-equal; front: %d differ" % (
        len(bad), (_bits(t) != _bits(ref["t"])).sum(), dt.max() if len(dt) else 0.0, (_bits(uv) != _bits(ref["uv"])).any(1).sum() if len(uv) else 0,
        (front != ref["front"]).sum()))
    assert len(bad) == 0, (bad[:10], tri[bad[:10]], ref["tri"][bad[:10]])
    assert (front == ref["front"]).all()
    assert _same_bits(t, ref["t"]) and _same_bits(uv, ref["uv"])
    miss = tri < 0
    assert np.isposinf(t[miss]).all() and np.isnan(uv[miss]).all() and not front[miss].any()


def _cast(fx, cell=None, V=None, F=None, O=None, D=None, **kw):
    from maskfusion_amd import eval as ev
    with ev.TriMesh(fx["V"] if V is None else V, fx["F"] if F is None else F, fx["cell"] if cell is None else cell) as m:
        return m.raycast(fx["O"] if O is None else O, fx["D"] if D is None else D, **kw)


# ---------------- 1, 2: against the restatement ----------------
def test_icosphere_is_the_restatements(hip):
    fx = _fixture("sphere")
    _check(fx["ref"], *_cast(fx))


def test_mixed_sizes_are_the_restatements(hip):
    fx = _fixture("mixed")
    got = _cast(fx)
    _check(fx["ref"], *got)
    assert ((got[1] >= 0) & (got[1] < 2)).sum() > 300 and (got[1] >= 2).sum() > 300


# ---------------- 3: tmin and tmax ----------------
def test_limits_cut_the_nearer_hit(hip):
    fx = _fixture("sphere")
    out = fx["groups"]["outside"]
    for kw in (dict(tmin=1.3), dict(tmax=1.3), dict(tmin=1.3, tmax=1.6), dict(tmin=-5.0, tmax=0.45)):
        ref = rr.raycast(fx["V"], fx["F"], fx["O"], fx["D"], **kw)
        if kw == dict(tmin=1.3):
            assert (ref["tri"][out] >= 0).all() and not ref["front"][out].any() and (ref["t64"][out] > 1.7).all()      # the far side of the sphere
        if kw == dict(tmax=1.3):
            assert (ref["tri"][out] == fx["ref"]["tri"][out]).all()
        if kw == dict(tmin=1.3, tmax=1.6):
            assert (ref["tri"][out] == -1).all()
        _check(ref, *_cast(fx, **kw))


# ---------------- 4: the cell, and two builds ----------------
def test_result_depends_on_neither_cell_nor_build(hip):
    for name in ("mixed", "sphere"):
        fx = _fixture(name)
        base = _cast(fx)
        _check(fx["ref"], *base)
        for cell in (0.01, 0.02, 0.05, 0.3):                        # at 0.3 the quad's box has few cells: it is gridded, not wide
            got = _cast(fx, cell=cell)
            assert all(_same_bits(a, b) for a, b in zip(got, base)), (name, cell)
        again = _cast(fx)
        assert all(_same_bits(a, b) for a, b in zip(again, base))


# ---------------- 5: ineligible triangles ----------------
def test_ineligible_triangles_change_nothing(hip):
    fx = _fixture("sphere")
    V, F = fx["V"], fx["F"]
    V2 = np.concatenate([V, [[np.nan, 0.3, 0.1]], V[5:6]]).astype(np.float32)     # vertex 162 is NaN, 163 a copy of vertex 5
    nv = len(V2)
    junk = np.array([[5, 9, 163], [7, 7, 30], [3, 4, nv], [-1, 4, 8], [2, 162, 11]], np.int32)
    at = np.sort(np.random.default_rng(31).choice(len(F) + 50, 50, replace=False))
    keep = np.ones(len(F) + 50, bool)
    keep[at] = False
    F2 = np.zeros((len(keep), 3), np.int32)
    F2[keep] = F
    F2[at] = junk[np.arange(50) % len(junk)]
    assert not tr.eligible(V2, F2)[at].any() and tr.eligible(V2, F2)[keep].all()
    mapped = dict(fx["ref"])
    mapped["tri"] = np.where(fx["ref"]["tri"] >= 0, np.flatnonzero(keep)[np.maximum(fx["ref"]["tri"], 0)], -1).astype(np.int32)
    _check(mapped, *_cast(fx, V=V2, F=F2))


# ---------------- 6: the transform ----------------
def _pose(w, t):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = t
    return T


def test_transform_is_the_host_transform(hip):
    fx = _fixture("sphere")
    T = _pose([0.2, -0.3, 0.15], [0.04, -0.03, 0.02])
    a = _cast(fx, T=T)
    o2, d2 = rr.transform_rays(T, fx["O"], fx["D"])
    b = _cast(fx, O=o2, D=d2)
    assert all(_same_bits(x, y) for x, y in zip(a, b))
    _check(rr.raycast(fx["V"], fx["F"], fx["O"], fx["D"], T=T), *a)
    assert (a[1] != fx["ref"]["tri"]).any()                       # and it moved something


# ---------------- 7: the pinhole form ----------------
VIEW = dict(W=64, H=48, fx=52.8, fy=53.1, cx=31.5, cy=23.25)


def test_render_is_raycast_on_the_pinhole_rays(hip):
    from maskfusion_amd import eval as ev
    fx = _fixture("sphere")
    T = _pose([0.1, 0.25, -0.05], [0.2, -0.3, -1.4])              # the camera 1.5 m in front of the sphere, turned a little
    T2 = np.eye(4)
    T2[:3, 3] = tr.SPHERE_C                                         # and inside it
    o, d = rr.pinhole_rays(**VIEW)
    for pose, kw in ((T, {}), (T2, {}), (T, dict(tmin=1.2, tmax=1.9))):
        with ev.TriMesh(fx["V"], fx["F"], fx["cell"]) as m:
            depth, tri, uv, front = m.render(mesh_from_cam=pose, **VIEW, **kw)
            t2, tri2, uv2, front2 = m.raycast(o, d, T=pose, **kw)
        assert depth.shape == (48, 64) and tri.shape == (48, 64) and uv.shape == (48, 64, 2) and front.shape == (48, 64)
        hit = tri2 >= 0
        print("pinhole: %d of %d pixels hit" % (hit.sum(), hit.size))
        assert 300 < hit.sum() and (pose is T2 or hit.sum() < hit.size - 300)
        assert _same_bits(depth.reshape(-1), np.where(hit, t2, np.float32(0)).astype(np.float32))
        assert (tri.reshape(-1) == tri2).all() and _same_bits(uv.reshape(-1, 2), uv2) and (front.reshape(-1) == front2).all()
        ref = rr.raycast(fx["V"], fx["F"], o, d, T=pose, **kw)
        _check(ref, t2, tri2, uv2, front2)
    # a width and a height that are no multiple of the tile, and one tile only
    for W, H in ((13, 9), (5, 3)):
        with ev.TriMesh(fx["V"], fx["F"], fx["cell"]) as m:
            depth, tri, _, _ = m.render(W, H, 10.0, 10.0, W / 2, H / 2, T2)
        o2, d2 = rr.pinhole_rays(W, H, 10.0, 10.0, W / 2, H / 2)
        ref = rr.raycast(fx["V"], fx["F"], o2, d2, T=T2)
        assert (tri.reshape(-1) == ref["tri"]).all() and _same_bits(depth.reshape(-1), ref["t"]) and (tri >= 0).all()


# ---------------- 8: empty, tiny, and what is refused ----------------
def test_empty_tiny_and_refused(hip):
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import MFError
    fx = _fixture("sphere")
    O, D = fx["O"][:300], fx["D"][:300]
    with ev.TriMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.05) as m:
        t, tri, uv, front = m.raycast(O, D)
        assert np.isposinf(t).all() and (tri == -1).all() and np.isnan(uv).all() and not front.any()
        depth, tri, uv, front = m.render(mesh_from_cam=np.eye(4), **VIEW)
        assert (depth == 0).all() and (tri == -1).all() and np.isnan(uv).all() and not front.any()
    F1 = fx["F"][17:18]
    ref = rr.raycast(fx["V"], F1, fx["O"], fx["D"])
    assert (ref["tri"] == 0).sum() > 5
    with ev.TriMesh(fx["V"], F1, 0.05) as m:
        _check(ref, *m.raycast(fx["O"], fx["D"]))
        t, tri, uv, front = m.raycast(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32))          # no rays
        assert t.shape == (0,) and tri.shape == (0,) and uv.shape == (0, 2) and front.shape == (0,)
        L, h, s = m._L, m._h, m._stream
        import torch
        o, d = ev._device_points(O), ev._device_points(D)
        n = len(O)
        out_t, out_i = torch.empty(n, dtype=torch.float32, device=o.device), torch.empty(n, dtype=torch.int32, device=o.device)
        I = np.eye(4, dtype=np.float32).reshape(16)
        bad_T = I.copy()
        bad_T[5] = np.nan
        inf = float("inf")

        def cast(handle=h, po=o.data_ptr(), pd=d.data_ptr(), stride=3, count=n, T=None, tmin=0.0, tmax=inf, pt=out_t.data_ptr(), pi=out_i.data_ptr()):
            return L.mf_trimesh_raycast_dev(handle, po, pd, stride, count, None if T is None else T.ctypes.data, tmin, tmax, pt, pi, None, None, s)

        def render(handle=h, W=64, H=48, fx=50.0, fy=50.0, cx=32.0, cy=24.0, T=I, tmin=0.0, tmax=inf, pt=out_t.data_ptr(), pi=out_i.data_ptr()):
            return L.mf_trimesh_render_dev(handle, W, H, fx, fy, cx, cy, None if T is None else T.ctypes.data, tmin, tmax, pt, pi, None, None, s)
        assert cast() == 0 and render(W=16, H=16) == 0
        for what, rc in (("null handle", cast(handle=None)), ("null origins", cast(po=None)), ("null dirs", cast(pd=None)), ("null t", cast(pt=None)),
                         ("null tri", cast(pi=None)), ("count < 0", cast(count=-1)), ("count > 2^30", cast(count=2 ** 30 + 1)), ("stride", cast(stride=2)),
                         ("transform", cast(T=bad_T)), ("tmin inf", cast(tmin=-inf)), ("tmin nan", cast(tmin=float("nan"))), ("tmax nan", cast(tmax=float("nan"))),
                         ("tmax < tmin", cast(tmin=1.0, tmax=0.5)),
                         ("render: null handle", render(handle=None)), ("render: no transform", render(T=None)), ("render: transform", render(T=bad_T)),
                         ("render: null depth", render(pt=None)), ("render: null tri", render(pi=None)), ("render: fx 0", render(fx=0.0)),
                         ("render: fy inf", render(fy=inf)), ("render: fx nan", render(fx=float("nan"))), ("render: width 0", render(W=0)),
                         ("render: height", render(H=16385)), ("render: width", render(W=16385)), ("render: tmin", render(tmin=inf)),
                         ("render: tmax < tmin", render(tmin=2.0, tmax=1.0)), ("render: tmax nan", render(tmax=float("nan")))):
            assert rc == -1, what                                   # MF_EINVAL
            assert L.mf_last_error(None).decode().startswith("mf_trimesh: "), what
        assert cast(count=0, po=None, pd=None, pt=None, pi=None) == 0
        with pytest.raises(MFError, match="tmax"):
            m.raycast(O, D, tmin=1.0, tmax=0.5)
    # two small triangles 40 m apart at a cell of 1 mm: 40 000 layers
    V = np.array([[0, 0, 0], [0.01, 0, 0], [0, 0.01, 0], [40, 0, 0], [40.01, 0, 0], [40, 0.01, 0]], np.float32)
    with ev.TriMesh(V, np.array([[0, 1, 2], [3, 4, 5]], np.int32), 0.001) as m:
        with pytest.raises(MFError, match="larger cell"):
            m.raycast(O, D)
        with pytest.raises(MFError, match="larger cell"):
            m.render(mesh_from_cam=np.eye(4), **VIEW)
    with ev.TriMesh(V, np.array([[0, 1, 2], [3, 4, 5]], np.int32), 0.01) as m:
        t, tri, _, _ = m.raycast(np.array([[0.002, 0.002, 1], [40.002, 0.002, -1], [20, 0, 1]], np.float32), np.array([[0, 0, -1], [0, 0, 4], [0, 0, -1]], np.float32))
        assert (tri == [0, 1, -1]).all() and (t[:2] == [1.0, 0.25]).all()


# ---------------- 9: the commands ----------------
def _command(module, args):
    if EMU:    # the child drives the same CPU-executed build as this process
        cmd = [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import %s as m; "
               "sys.exit(m.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"), module)] + args
    else:
        cmd = [sys.executable, "-m", "maskfusion_amd." + module] + args
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)


def _scene_files(d, n_frames):
    """a room of 12 triangles, an icosphere of 30 cm that moves through three poses, and a camera that drifts: the files meshseq takes"""
    from maskfusion_amd import mesh as M
    from maskfusion_amd import meshseq
    Vr, Fr = rr.room()
    assert len(Fr) == 12
    Vs, Fs = tr.icosphere(centre=np.zeros(3), radius=0.3)
    M.write_obj(os.path.join(d, "room.obj"), Vr, Fr)
    M.write_mesh_ply(os.path.join(d, "ball.ply"), Vs, triangles=Fs)
    cam, obj = [], []
    for k in range(n_frames):
        cam.append(meshseq.tum_line(0.1 * k, _pose([0.0, 0.03 * k + 1e-9, 0.0], [0.02 * k, -0.01 * k, 0.0])))
    for k, t in enumerate((0.0, 0.1, 0.25)):
        obj.append(meshseq.tum_line(t, _pose([0.0, 0.0, 0.2 * k + 1e-9], [0.15 * k - 0.1, 0.05, 1.6 + 0.1 * k])))
    for name, lines in (("cam.txt", cam), ("ball.txt", obj)):
        with open(os.path.join(d, name), "w") as f:
            f.write("\n".join(lines) + "\n")
    return (Vr, Fr), (Vs, Fs)


def test_meshseq_writes_a_sequence_and_mesh_views_scores_it(hip, tmp_path):
    """meshseq end to end at 64 x 48, four frames, the depth written as float (--depth exr: the default 16-bit PNG rounds to millimetres),
    then the mesh command's --views with the room's own mesh and the ground-truth poses.  The room's mesh is scored on the room's pixels:
    --views counts a pixel in the group of its mask, the ball's pixels (where the room lies behind the ball) are group 1."""
    from maskfusion_amd import eval as ev
    from maskfusion_amd.io.readers import ImageLogReader
    d = str(tmp_path)
    (Vr, Fr), (Vs, Fs) = _scene_files(d, 4)
    seq = os.path.join(d, "seq")
    r = _command("meshseq", ["--mesh", os.path.join(d, "room.obj"), "--object", os.path.join(d, "ball.ply") + ":7:" + os.path.join(d, "ball.txt"),
                             "--poses", os.path.join(d, "cam.txt"), "--size", "64x48", "--depth", "exr", "-o", seq])
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    assert info["frames"] == 4 and info["objects"] == 1 and info["class_ids"] == [7] and info["triangles"] == [12, 320] and info["depth_coverage"] == 1.0
    reader = ImageLogReader(seq)
    assert reader.getNumFrames() == 4 and reader.hasMasksGT and reader.calibrationFile
    cal = (52.8, 52.8, 32.0, 24.0)
    cam, ball = ev.read_tum(os.path.join(d, "cam.txt")), ev.read_tum(os.path.join(d, "ball.txt"))
    gt, og = ev.read_tum(os.path.join(seq, "groundtruth.txt")), ev.read_tum(os.path.join(seq, "object-1.txt"))
    assert len(gt[0]) == 4 and len(og[0]) == 4 and np.abs(gt[1] - cam[1]).max() < 1e-12
    assert (gt[0] == np.array(reader.timestamps()) * 1e-6).all()
    masks = []
    with ev.TriMesh(Vr, Fr, 5.0 / 128) as room, ev.TriMesh(Vs, Fs, 0.6 / 128) as sphere:
        for k, f in enumerate(reader):
            T_obj = ball[1][[0, 1, 2, 2][k]]                          # the nearest stamp of 0, 0.1, 0.25 to 0.1 k
            assert np.abs(og[1][k] - T_obj).max() < 1e-12
            d_room = room.render(64, 48, *cal, cam[1][k])[0]
            d_ball = sphere.render(64, 48, *cal, np.linalg.inv(T_obj) @ cam[1][k])[0]
            wins = (d_ball > 0) & (d_ball <= d_room)
            assert (d_room > 0).all() and 50 < wins.sum() < 1500
            assert f.depth.dtype == np.float32 and _same_bits(f.depth, np.where(wins, d_ball, d_room))
            assert (f.mask == wins).all() and f.classIDs == [0, 7]
            assert (f.rgb[wins].max(1) > 0).all() and (f.rgb[~wins].max(1) > 0).all()
            masks.append(f.mask)
    assert (masks[0] != masks[3]).any()                               # the ball and the camera moved
    r = _command("mesh", ["--mesh", os.path.join(d, "room.obj"), "--views", seq, "--poses", os.path.join(seq, "groundtruth.txt")])
    assert r.returncode == 0, r.stderr
    v = json.loads(r.stdout)["mesh_views"]
    print(v["groups"], v["summary"])
    room_px = [g for g in v["groups"] if g["group"] == 0][0]
    assert v["frames"] == 4 and v["frames_skipped"] == 0 and room_px["pixels"] == sum(int((m == 0).sum()) for m in masks)
    assert room_px["coverage"] == 1.0 and room_px["depth_coverage"] == 1.0 and room_px["depth_l1"] == 0.0 and room_px["depth_within_tau"] == 1.0
    assert room_px["psnr"] is None and isinstance(room_px["ssim"], float)      # the same shading from the same pose: no colour error at all
    ball_px = [g for g in v["groups"] if g["group"] == 1][0]
    assert ball_px["coverage"] == 1.0 and ball_px["depth_l1"] > 0.5    # the wall behind the ball
    assert v["summary"]["coverage"] == 1.0
    r = _command("mesh", ["--mesh", os.path.join(d, "room.obj"), "--views", seq])
    assert r.returncode == 2 and "--poses" in r.stderr


def test_cli_runs_a_meshseq_sequence(hip, tmp_path):
    """eight frames at 160 x 120 through the driver: the run completes and exports eight poses.  No accuracy is gated."""
    d = str(tmp_path)
    _scene_files(d, 8)
    seq, out = os.path.join(d, "seq"), os.path.join(d, "out")
    r = _command("meshseq", ["--mesh", os.path.join(d, "room.obj"), "--object", os.path.join(d, "ball.ply") + ":7:" + os.path.join(d, "ball.txt"),
                             "--poses", os.path.join(d, "cam.txt"), "--size", "160x120", "--max-depth", "4.0", "-o", seq])
    assert r.returncode == 0, r.stderr
    assert json.loads(r.stdout)["frames"] == 8 and os.path.exists(os.path.join(seq, "Depth0007.png")) and os.path.exists(os.path.join(seq, "Mask0007.txt"))
    r = _command("cli", ["-dir", seq + os.sep, "-run", "-q", "-ep", "-exportdir", out])
    assert r.returncode == 0, r.stderr
    assert "processed 8 frames" in r.stdout
    with open(os.path.join(out, "poses-0.txt")) as f:
        assert len([x for x in f.read().splitlines() if x.strip() and not x.startswith("#")]) == 8
