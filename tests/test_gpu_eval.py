"""Run evaluation on the device: mf_cloud_nn_dev against an fp32 numpy brute force (bit for bit) and scipy's cKDTree, mf_model_cloud_nn_dev
on live (dense and sparse) maps and its promise to change nothing, and the eval command end to end.  Runs on the MI355X (-m gpu) and, with
MF_EMU=1, on the CPU-executed build."""
import ctypes as C
import json
import os
import struct
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"
W, H, F = 320, 240, 264.0


def brute(target, query, radius):
    """fp32 brute force with the library's rules: d2 = (dx*dx + dy*dy) + dz*dz, d2 <= fl(r*r), smallest d2 then smallest j"""
    t = np.ascontiguousarray(target[:, :3], np.float32)
    q = np.ascontiguousarray(query[:, :3], np.float32)
    r2 = np.float32(radius) * np.float32(radius)
    ok_t = np.isfinite(t).all(1)
    dist = np.full(len(q), np.inf, np.float32)
    idx = np.full(len(q), -1, np.int32)
    if len(t) == 0:
        return dist, idx
    for a in range(0, len(q), 512):
        qq = q[a:a + 512]
        with np.errstate(invalid="ignore", over="ignore"):
            dx = qq[:, None, 0] - t[None, :, 0]
            dy = qq[:, None, 1] - t[None, :, 1]
            dz = qq[:, None, 2] - t[None, :, 2]
            d2 = dx * dx + dy * dy + dz * dz
            d2 = np.where(ok_t[None, :] & (d2 <= r2), d2, np.float32(np.inf))
        j = np.argmin(d2, 1)            # first minimum: the smallest j
        m = d2[np.arange(len(qq)), j]
        hit = np.isfinite(m)
        dist[a:a + 512][hit] = np.sqrt(m[hit])
        idx[a:a + 512][hit] = j[hit]
    return dist, idx


def transform_host(T, p):
    """the library's query transform in fp32: x' = ((T00 x + T01 y) + T02 z) + T03"""
    T = np.asarray(T, np.float32)
    x, y, z = p[:, 0].astype(np.float32), p[:, 1].astype(np.float32), p[:, 2].astype(np.float32)
    return np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], 1)


def _cloud(rng, n, lo=-1.0, hi=1.0):
    return rng.uniform(lo, hi, (n, 3)).astype(np.float32)


def _rigid(rng):
    from maskfusion_amd import synth
    return synth.make_pose(synth.rot_xyz(*rng.uniform(-1, 1, 3)), rng.uniform(-0.2, 0.2, 3)).astype(np.float32)


def test_nn_matches_brute_force_bit_for_bit(hip):
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(1)
    t = _cloud(rng, 12000)
    t[100:140] = t[0:40]                     # exact duplicates: the smaller index must win
    r = np.float32(0.0625)
    # points at exactly the radius (dyadic coordinates: dx = r exactly) and one ulp beyond
    t[200] = [4.5, 4.5, 4.5]                 # (away from the random cloud)
    t[201] = [6.25, 6.25, 6.25]
    t[202:205] = [np.nan, 0, 0], [np.inf, 1, 1], [0, -np.inf, 0]
    q = _cloud(rng, 8000)
    q[0:40] = t[0:40]
    q[40] = [4.5 + r, 4.5, 4.5]
    q[41] = [np.nextafter(np.float32(6.25) - r, np.float32(-1)), 6.25, 6.25]
    q[42:45] = [np.nan, 0, 0], [0, np.inf, 0], [-np.inf, -np.inf, -np.inf]
    q[45:50] = t[100:105] + np.float32(1e-3)
    for radius in (r, np.float32(0.02), np.float32(0.3)):
        dist, idx = ev.nearest(t, q, radius)
        bd, bi = brute(t, q, radius)
        assert dist.tobytes() == bd.tobytes(), int((dist != bd).sum())
        assert (idx == bi).all(), int((idx != bi).sum())
    dist, idx = ev.nearest(t, q, r)
    assert dist[40] == r and idx[40] == 200          # at exactly the radius: in
    assert idx[41] == -1 and dist[41] == np.inf       # one ulp beyond: out
    assert (idx[0:40] == np.arange(40)).all() and (dist[0:40] == 0).all()
    assert (idx[42:45] == -1).all() and np.isinf(dist[42:45]).all()
    hits = (idx >= 0).mean()
    assert 0.1 < hits < 0.99, hits
    # an empty target, no queries
    dist, idx = ev.nearest(np.zeros((0, 3), np.float32), q[:100], 0.1)
    assert (idx == -1).all() and np.isinf(dist).all()
    dist, idx = ev.nearest(t, np.zeros((0, 3), np.float32), 0.1)
    assert dist.shape == (0,) and idx.shape == (0,)


def test_nn_is_deterministic_and_stride_and_transform_agnostic(hip):
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(2)
    t = _cloud(rng, 20000)
    t[5000:6000] = t[:1000]                   # ties in every bucket that holds them
    q = _cloud(rng, 20000)
    a = ev.nearest(t, q, 0.05)
    b = ev.nearest(t, q, 0.05)
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    for stride in (4, 12):
        ts = rng.normal(size=(len(t), stride)).astype(np.float32)
        ts[:, :3] = t
        qs = rng.normal(size=(len(q), stride)).astype(np.float32)
        qs[:, :3] = q
        c = ev.nearest(ts, qs, 0.05)
        assert c[0].tobytes() == a[0].tobytes() and c[1].tobytes() == a[1].tobytes(), stride
    T = _rigid(rng)
    qm = (q - T[:3, 3]) @ T[:3, :3]           # so that T brings them back near the targets
    d1 = ev.nearest(t, qm, 0.05, T=T)
    d2 = ev.nearest(t, transform_host(T, qm), 0.05)
    assert d1[0].tobytes() == d2[0].tobytes() and d1[1].tobytes() == d2[1].tobytes()
    assert (d1[1] >= 0).mean() > 0.5


def test_nn_agrees_with_ckdtree_on_1m_points(hip):
    from scipy.spatial import cKDTree
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(4)
    n = 1_000_000
    nq = 200_000 if EMU else n                # (the CPU-executed build: fewer queries, the same million targets)
    t = _cloud(rng, n, -5.0, 5.0)
    q = np.concatenate([t[rng.integers(0, n, nq // 2)] + rng.normal(scale=0.02, size=(nq // 2, 3)).astype(np.float32),
                        _cloud(rng, nq - nq // 2, -5.0, 5.0)])
    radius = 0.05
    dist, idx = ev.nearest(t, q, radius)
    kd, ki = cKDTree(t.astype(np.float64)).query(q.astype(np.float64), k=1, distance_upper_bound=radius)
    hit_g, hit_k = idx >= 0, np.isfinite(kd)
    both = hit_g & hit_k
    assert both.mean() > 0.4
    assert np.abs(dist[both] - kd[both]).max() < 1e-6
    # the same neighbour, or one at the same distance to within rounding
    other = both & (idx != ki)
    if other.any():
        d64 = np.linalg.norm(t[idx[other]].astype(np.float64) - q[other].astype(np.float64), axis=1)
        assert np.abs(d64 - kd[other]).max() < 1e-6
    # hit / miss sets differ only where the fp64 distance lies within rounding of the radius
    diff = hit_g != hit_k
    n_diff = int(diff.sum())
    if n_diff:
        d_any = np.where(hit_k, kd, np.inf)
        near = np.abs(np.where(hit_g, dist.astype(np.float64), d_any) - radius) < 1e-6
        assert near[diff].all()
    print(f"ulp-boundary hit/miss differences: {n_diff} of {len(q)}")
    assert n_diff <= max(10, len(q) // 100000)


def test_nn_argument_checks(hip):
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import MFError, load, torch_device
    import torch
    L = load()
    rng = np.random.default_rng(5)
    t, q = _cloud(rng, 100), _cloud(rng, 10)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(MFError):
            ev.nearest(t, q, bad)
    with pytest.raises(MFError):
        ev.nearest(t * np.float32(2 ** 31 * 0.01), q, 0.01)     # |x / r| >= 2^30
    with pytest.raises(MFError):
        ev.nearest(t, q * np.float32(2 ** 31), 1.0)
    need = C.c_uint64(0)
    assert L.mf_cloud_nn_workspace(100, C.byref(need)) == 0 and need.value > 0
    dev = torch_device()
    dt, dq = torch.from_numpy(t).to(dev), torch.from_numpy(q).to(dev)
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=dev)
    dist = torch.empty(10, dtype=torch.float32, device=dev)
    idx = torch.empty(10, dtype=torch.int32, device=dev)
    args = [dt.data_ptr(), 3, 100, dq.data_ptr(), 3, 10, None, 0.1, dist.data_ptr(), idx.data_ptr(), ws.data_ptr(), int(need.value), None]
    assert L.mf_cloud_nn_dev(*args) == 0
    for k, v in ((1, 2), (4, 2), (11, int(need.value) - 1), (5, (1 << 30) + 1), (2, (1 << 30) + 1)):
        bad = list(args)
        bad[k] = v
        assert L.mf_cloud_nn_dev(*bad) == -1, k
    assert L.mf_cloud_nn_workspace(-1, C.byref(need)) == -1


# ---------------- live models ----------------
def _context(**kw):
    from maskfusion_amd import MaskFusion
    return MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, enableMultipleModels=False,
                      initConfidenceGlobal=1.0, **kw)


def _stream():
    from maskfusion_amd import synth
    return synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=True)


def _check_live(m, rng, sparse):
    from maskfusion_amd import eval as ev
    thr = m.getBackgroundModel().getConfidenceThreshold()
    n = m.getBackgroundModel().lastCount()
    assert n > 1000
    # the queries come from the map's neighbourhood, read through the device (no download yet: a sparse map stays sparse)
    box = np.array([[-1.5, -1.0, 0.3], [1.5, 1.0, 3.0]], np.float32)
    q = rng.uniform(box[0], box[1], (6000, 3)).astype(np.float32)
    T = _rigid(rng)
    got = {}
    for name, ct, TT in (("own threshold", None, None), ("all", -1.0, None), ("transform", None, T)):
        got[name] = m.modelCloudNN(0, q, 0.05, transform=TT, confThreshold=ct)
    import torch
    from maskfusion_amd.lib import torch_device
    dq = torch.from_numpy(q).to(torch_device())
    dd, di = m.modelCloudNN(0, dq, 0.05)
    assert isinstance(dd, torch.Tensor) and dd.device.type == torch_device()
    assert dd.cpu().numpy().tobytes() == got["own threshold"][0].tobytes()
    surf = m.getBackgroundModel().downloadMap()
    assert len(surf) == n
    for name, ct, TT in (("own threshold", thr, None), ("all", -1.0, None), ("transform", thr, T)):
        tgt = surf.copy()
        tgt[~(surf[:, 3] > ct), :3] = np.nan    # filtered the same way, the download's indices kept
        d, i = ev.nearest(tgt, q, 0.05, T=TT)
        assert got[name][0].tobytes() == d.tobytes(), (name, sparse)
        assert (got[name][1] == i).all(), (name, sparse)
        hit = i >= 0
        assert hit.mean() > (0.005 if TT is not None else 0.02), name
        assert (surf[i[hit], 3] > ct).all()
    return got


def test_model_nn_on_a_dense_map(hip):
    m = _context()
    st = _stream()
    for k in range(4):
        rgb, depth, _ = st.frame(k)
        m.processFrame(rgb, depth, timestamp=k)
    _check_live(m, np.random.default_rng(6), False)
    with pytest.raises(Exception):
        m.modelCloudNN(0, np.zeros((4, 3), np.float32), 0.0)
    with pytest.raises(Exception):
        m.modelCloudNN(3, np.zeros((4, 3), np.float32), 0.05)
    m.close()


def test_model_nn_on_a_sparse_map(hip):
    m = _context()
    m.setParam("bigMapElements", 1000)      # the background is kept as runs and cleaned in place
    st = _stream()
    for k in range(6):
        rgb, depth, _ = st.frame(k)
        m.processFrame(rgb, depth, timestamp=k)
    _check_live(m, np.random.default_rng(7), True)
    m.close()


def test_model_nn_changes_nothing(hip):
    st = _stream()
    frames = [st.frame(k) for k in range(7)]
    a, b = _context(), _context()
    for c in (a, b):
        c.setParam("bigMapElements", 1000)
    q = np.random.default_rng(8).uniform(-1, 1, (3000, 3)).astype(np.float32)
    for k, (rgb, depth, _) in enumerate(frames):
        a.processFrame(rgb, depth, timestamp=k)
        b.processFrame(rgb, depth, timestamp=k)
        if k in (2, 4):
            a.modelCloudNN(0, q, 0.05)
    assert a.getCurrPose().tobytes() == b.getCurrPose().tobytes()
    assert a.getBackgroundModel().downloadMap().tobytes() == b.getBackgroundModel().downloadMap().tobytes()
    a.close()
    b.close()


def test_model_nn_orders_itself_after_torch_work(hip):
    """queries still being written by torch's stream, and outputs in blocks the caching allocator just recycled: the call must wait"""
    import torch
    from maskfusion_amd.lib import torch_device
    m = _context()
    st = _stream()
    for k in range(3):
        rgb, depth, _ = st.frame(k)
        m.processFrame(rgb, depth, timestamp=k)
    rng = np.random.default_rng(9)
    q = rng.uniform([-1.5, -1.0, 0.3], [1.5, 1.0, 3.0], (200000, 3)).astype(np.float32)
    want = m.modelCloudNN(0, q, 0.05)
    dev = torch_device()
    src = torch.from_numpy(q).to(dev)
    for _ in range(3):
        a = torch.randn(2048, 2048, device=dev)
        for _ in range(8):                       # keeps torch's stream busy ahead of the query tensor
            a = a @ a
            a = a / a.abs().max()
        dq = (src + a[0, 0] * 0.0).contiguous()  # written by torch's stream after that work
        del a
        d, i = m.modelCloudNN(0, dq, 0.05)
        assert d.cpu().numpy().tobytes() == want[0].tobytes() and (i.cpu().numpy() == want[1]).all()
    m.close()


# ---------------- end to end ----------------
def _write_ply(path, xyz):
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z\nend_header\n"
                 % len(xyz)).encode())
        f.write(np.ascontiguousarray(xyz, "<f4").tobytes())


def _visible(pts, st, frames, depth_cut):
    """the reference points some frame of the stream saw (within 2 cm of its rendered depth, nearer than the depth cut-off)"""
    seen = np.zeros(len(pts), bool)
    for k, (_, depth, _) in enumerate(frames):
        Tcw = np.linalg.inv(st.gt_pose(k))
        pc = pts @ Tcw[:3, :3].T + Tcw[:3, 3]
        z = pc[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            u = np.floor(st.fx * pc[:, 0] / z + st.cx).astype(np.int64)
            v = np.floor(st.fy * pc[:, 1] / z + st.cy).astype(np.int64)
        ok = (z > 0.1) & (z < depth_cut) & (u >= 0) & (u < st.W) & (v >= 0) & (v < st.H)
        dz = np.full(len(pts), np.inf)
        dz[ok] = np.abs(depth[v[ok], u[ok]] - z[ok])
        seen |= dz < 0.02
    return seen


def test_eval_command_end_to_end(hip, tmp_path):
    from scipy.spatial import cKDTree
    from maskfusion_amd import MaskFusion, synth
    from maskfusion_amd import eval as ev
    st = synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=False)
    n_frames = 30
    m = MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, enableMultipleModels=False)
    frames = [st.frame(k) for k in range(n_frames)]
    for k, (rgb, depth, _) in enumerate(frames):
        m.processFrame(rgb, depth, timestamp=33333 * (k + 1))
    est, ref = tmp_path / "est", tmp_path / "ref"
    est.mkdir()
    ref.mkdir()
    m.exportPoses(str(est) + os.sep)
    m.savePly(str(est) + os.sep)
    est_T = ev.read_tum(str(est / "poses-0.txt"))[1]
    m.close()
    gt_T = np.array([st.gt_pose(k) for k in range(n_frames)])
    with open(tmp_path / "gt.txt", "w") as f:
        f.write("# synthetic ground truth\n")
        from scipy.spatial.transform import Rotation
        for k in range(n_frames):
            q = Rotation.from_matrix(gt_T[k][:3, :3]).as_quat()
            f.write("%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n" % (33333 * (k + 1) * 1e-6, *gt_T[k][:3, 3], *q))
    # the reference surface: the room's dense map in camera-0 coordinates, cropped to what the stream saw
    room = synth.dense_room_map(st.scene, 400_000, last_time=0.0)[:, :3].astype(np.float64)
    T0 = np.linalg.inv(st.gt_pose(0))
    room = room @ T0[:3, :3].T + T0[:3, 3]
    room = room[_visible(room, st, frames, 3.0)].astype(np.float32)
    _write_ply(str(ref / "cloud-0.ply"), room)
    args = ["--est", str(est), "--ref", str(ref), "--gt", str(tmp_path / "gt.txt"), "--radius", "0.05", "--tau", "0.01,0.02,0.05"]
    if EMU:    # the child drives the same CPU-executed build as this process
        cmd = [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import eval as e; "
               "sys.exit(e.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"))] + args
    else:
        cmd = [sys.executable, "-m", "maskfusion_amd.eval"] + args
    out = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stderr
    objs = [json.loads(l) for l in out.stdout.strip().split("\n")]
    assert len(objs) == 1 and objs[0]["model"] == 0
    o = objs[0]
    a = o["trajectory_vs_gt"]["ate"]
    assert a["pairs"] == n_frames
    assert a["rmse"] <= synth.ate_rmse(est_T, gt_T) + 1e-9
    # the cloud statistics, recomputed with scipy on the same files
    e_pts, r_pts = ev.read_ply(str(est / "cloud-0.ply")), ev.read_ply(str(ref / "cloud-0.ply"))
    c = o["cloud"]
    for key, (src, dst) in (("accuracy", (e_pts, r_pts)), ("completeness", (r_pts, e_pts))):
        d, _ = cKDTree(dst.astype(np.float64)).query(src.astype(np.float64), k=1, distance_upper_bound=0.05)
        cl = np.minimum(d, 0.05)
        s = c[key]
        assert s["count"] == len(src) and s["misses"] == int(np.isinf(d).sum())
        assert abs(s["mean"] - cl.mean()) < 1e-6 and abs(s["rmse"] - np.sqrt((cl * cl).mean())) < 1e-6 and abs(s["median"] - np.median(cl)) < 1e-6
        for tau in ("0.01", "0.02", "0.05"):
            assert abs(s["fraction"][tau] - (d <= float(tau)).mean()) < 1e-6 + 2.0 / len(src), (key, tau)
    print("eval:", json.dumps(c["fscore"]), "accuracy mean", c["accuracy"]["mean"], "completeness mean", c["completeness"]["mean"], "ATE", a["rmse"])
    assert c["fscore"]["0.05"] > 0.9
