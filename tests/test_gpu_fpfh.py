"""FPFH descriptors, the descriptor matcher and the registration without a start on the device (mf_cloud_fpfh_dev, mf_feature_match_dev,
maskfusion_amd.eval.fpfh / match_features / register_global) against the brute-force numpy restatement of tests/fpfh_restatement.py: the
pair counts exactly, the descriptor where no pair of the point or of its neighbours sits within 1e-9 of a decision, the matcher bit for
bit, and a 120 degree / 3 m motion recovered without a start.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build.

The descriptor gate (1e-9) bounds fp64 values -- a part is a sum of at most K non-negative fp64 terms scaled to 100, so two orders of
summation differ by at most 100 K 2^-53, about 1e-11 for K of a few hundred -- and the device stores fp32: the stored value must lie in
[fl32(r - 1e-9), fl32(r + 1e-9)] of the restatement's fp64 r (_stored_within of tests/test_gpu_eval_normals.py)."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fpfh_restatement as fr  # noqa: E402
import global_scene as gs  # noqa: E402
import register_restatement as rr  # noqa: E402
from test_gpu_eval_normals import SIGMA, SPHERE_C, _sphere, _stored_within  # noqa: E402

pytestmark = pytest.mark.gpu


def _corner(rng, n):
    """three unit squares that meet in the origin, with their normals"""
    uv = rng.uniform(0, 1, (n, 2))
    axis = np.arange(n) % 3
    p, nm = np.zeros((n, 3)), np.zeros((n, 3))
    for a in range(3):
        m = axis == a
        p[np.ix_(m, [k for k in range(3) if k != a])] = uv[m]
        nm[m, a] = 1.0
    return p, nm


def _clouds():
    """name -> (points, normals, radius): 2 mm of noise on the positions, normals off by about a degree and not of unit length"""
    rng = np.random.default_rng(31)
    s = _sphere(rng, 2000)
    c, cn = _corner(rng, 2000)
    s2 = _sphere(rng, 1500)
    c2, cn2 = _corner(rng, 1500)
    raw = {"sphere": (s, (s - SPHERE_C) / 0.5, 0.15), "corner": (c, cn, 0.15), "both": (np.concatenate([s2, c2]), np.concatenate([(s2 - SPHERE_C) / 0.5, cn2]), 0.18)}
    out = {}
    for name, (p, nm, radius) in raw.items():
        nm = (nm + rng.normal(scale=0.02, size=nm.shape)) * rng.uniform(0.5, 2.0, (len(nm), 1))
        out[name] = ((p + rng.normal(scale=SIGMA, size=p.shape)).astype(np.float32), nm.astype(np.float32), radius)
    return out


_cache = {}


def _ref(name):
    """the cloud, its normals, its radius and the restatement's result, computed once and shared (treat as read-only)"""
    if name not in _cache:
        if "clouds" not in _cache:
            _cache["clouds"] = _clouds()
        p, nm, radius = _cache["clouds"][name]
        _cache[name] = (p, nm, radius, fr.fpfh(p, nm, radius))
    return _cache[name]


def _check(f, s, want, cap=0.01):
    """k everywhere, the counts and the descriptor on the gated points, NaN rows where the restatement has them"""
    g = want["gated"]
    print("mean k %.1f; outside the gate: %.3f %% of %d points" % (want["spfh"][:, 33].mean(), 100 * (1 - g.mean()) if len(g) else 0.0, len(g)))
    assert s.dtype == np.int32 and (s[:, 33] == want["spfh"][:, 33]).all()
    assert (s[g] == want["spfh"][g]).all()
    assert (s[:, :33].reshape(len(s), 3, 11).sum(2) == s[:, 33:34]).all()
    if cap is not None:       # (a point that is not eligible has no pairs to gate)
        assert (want["eligible"] & ~g).mean() <= cap
    nan = np.isnan(want["fpfh"]).any(1)
    assert (np.isnan(f).any(1) == nan).all() and (np.isnan(f).all(1) == nan).all()
    ok = g & ~nan
    diff = np.abs(f[ok].astype(np.float64) - want["fpfh64"][ok])
    print("gated rows %d: max |stored - fp64| %.3g; %d stored values are not the restatement's bits"
          % (ok.sum(), diff.max(initial=0.0), (f[ok] != want["fpfh"][ok]).sum()))
    assert f.dtype == np.float32 and _stored_within(f[ok], want["fpfh64"][ok]).all()


def _raw_fpfh(rec, noff, radius, with_spfh=True):
    """mf_cloud_fpfh_dev on records of any stride"""
    import torch
    from maskfusion_amd.lib import load, torch_device
    L = load()
    n = len(rec)
    d = torch.from_numpy(np.ascontiguousarray(rec, np.float32)).to(torch_device())
    need = C.c_uint64(0)
    assert L.mf_cloud_fpfh_workspace(n, C.byref(need)) == 0
    ws = torch.empty(int(need.value), dtype=torch.uint8, device=d.device)
    out = torch.zeros((n, 33), dtype=torch.float32, device=d.device)
    cnt = torch.zeros((n, 34), dtype=torch.int32, device=d.device)
    rc = L.mf_cloud_fpfh_dev(d.data_ptr(), rec.shape[1], noff, n, radius, out.data_ptr(), cnt.data_ptr() if with_spfh else None, ws.data_ptr(),
                             int(need.value), None)
    assert rc == 0, rc
    return out.cpu().numpy(), cnt.cpu().numpy()


# ---------------- 1. counts and descriptors ----------------
@pytest.mark.parametrize("name", ["sphere", "corner", "both"])
def test_counts_and_descriptors_on_the_gated_points(hip, name):
    from maskfusion_amd import eval as ev
    p, nm, radius, want = _ref(name)
    assert 30 <= want["spfh"][:, 33].mean() <= 80 and 1 - want["gated"].mean() <= 0.01          # the restatement alone: the clouds fit the gate
    f, s = ev.fpfh(p, nm, radius)
    assert f.shape == (len(p), 33) and s.shape == (len(p), 34)
    _check(f, s, want)
    ok = ~np.isnan(f).any(1)
    assert ok.mean() > 0.99 and np.abs(f[ok].astype(np.float64).reshape(-1, 3, 11).sum(2) - 100).max() < 1e-3 and (f[ok] >= 0).all()
    assert s.tobytes() == ev.fpfh(p, nm, radius)[1].tobytes()                                      # integer counts: the same for every call


def test_strides_and_rows_that_take_no_part(hip):
    p, nm, radius, want = _ref("corner")
    rng = np.random.default_rng(32)
    for stride, noff in ((6, 3), (11, 5), (11, 8)):
        rec = rng.normal(size=(len(p), stride)).astype(np.float32)
        rec[:, :3], rec[:, noff:noff + 3] = p, nm
        f, s = _raw_fpfh(rec, noff, radius)
        _check(f, s, want)
        _check(_raw_fpfh(rec, noff, radius, with_spfh=False)[0], s, want)          # without the counts' output
    # positions and normals that are not finite, zero normals: k = 0, a NaN row, and nobody's neighbour
    bp, bn = p.copy(), nm.copy()
    rows = rng.choice(len(p), 100, replace=False)
    bp[rows[:20], 0] = np.nan
    bp[rows[20:40], 1] = np.inf
    bn[rows[40:60], 2] = np.nan
    bn[rows[60:80]] = 0.0
    bn[rows[80:], 0] = -np.inf
    wb = fr.fpfh(bp, bn, radius)
    from maskfusion_amd import eval as ev
    f, s = ev.fpfh(bp, bn, radius)
    _check(f, s, wb)
    assert (s[rows] == 0).all() and np.isnan(f[rows]).all() and not wb["eligible"][rows].any()
    assert (s[:, 33] != want["spfh"][:, 33]).any()
    # duplicated points: L == 0, the pair is not counted (the copies still count their other neighbours)
    dp, dn = np.concatenate([p, p[:40]]), np.concatenate([nm, nm[:40]])
    wd = fr.fpfh(dp, dn, radius)
    f, s = ev.fpfh(dp, dn, radius)
    _check(f, s, wd, cap=0.03)
    assert (wd["neighbours"][:40] >= want["neighbours"][:40] + 1).all() and (s[:40, 33] == s[len(p):, 33]).all()
    assert (s[:40, 33] == wd["neighbours"][:40] - 1).all()            # its copy is a neighbour and the one pair that is not counted


def test_pairs_that_are_not_counted_and_tiny_clouds(hip):
    from maskfusion_amd import eval as ev
    # point 0 and point 1: d parallel to the normal, |v| == 0; point 0 and point 2: counted
    p = np.array([[0, 0, 0], [0, 0, 0.5], [0.25, 0, 0], [0.125, 0.375, 0.25]], np.float32)
    nm = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1], [0.6, 0, 0.8]], np.float32)
    want = fr.fpfh(p, nm, 1.0)
    f, s = ev.fpfh(p, nm, 1.0)
    assert (want["neighbours"] == 3).all() and want["spfh"][:, 33].tolist() == [2, 2, 3, 3]
    assert (s == want["spfh"]).all()
    assert (np.isnan(f) == np.isnan(want["fpfh"])).all() and _stored_within(f, want["fpfh64"])[~np.isnan(f)].all()
    # n = 0, 1, 2
    f, s = ev.fpfh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32), 0.1)
    assert f.shape == (0, 33) and s.shape == (0, 34)
    f, s = ev.fpfh(p[:1], nm[:1], 1.0)
    assert np.isnan(f).all() and (s == 0).all()
    f, s = ev.fpfh(p[[0, 3]], nm[[0, 3]], 1.0)
    w2 = fr.fpfh(p[[0, 3]], nm[[0, 3]], 1.0)
    assert (s == w2["spfh"]).all() and s[:, 33].tolist() == [1, 1] and not np.isnan(f).any()
    # two points: each row is the other's SPFH scaled to 100 a part -- one bin of 100 in every part
    assert (np.sort(f.reshape(2, 3, 11), 2)[:, :, -1] == 100).all() and (f.reshape(2, 3, 11).sum(2) == 100).all()
    f, s = ev.fpfh(p[[0, 3]], nm[[0, 3]], 0.25)       # out of each other's reach
    assert np.isnan(f).all() and (s == 0).all()


def test_radius_test_is_inclusive_on_a_lattice(hip):
    """a 5 x 5 x 5 lattice of spacing 2^-2 searched with radius 2^-2: the six axis neighbours lie at exactly d2 = fl(r * r)"""
    from maskfusion_amd import eval as ev
    g = np.arange(5, dtype=np.float32) * np.float32(0.25) - np.float32(0.5)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    rng = np.random.default_rng(33)
    nm = rng.normal(size=p.shape).astype(np.float32)            # no pair with d parallel to a normal or a1 = a2
    want = fr.fpfh(p, nm, 0.25)
    f, s = ev.fpfh(p, nm, 0.25)
    assert want["neighbours"][62] == 6 and want["neighbours"].min() == 3 and (want["spfh"][:, 33] == want["neighbours"]).all()      # 62: the centre
    _check(f, s, want, cap=None)
    f, s = ev.fpfh(p, nm, np.nextafter(np.float32(0.25), np.float32(0)))
    assert (s == 0).all() and np.isnan(f).all()


def test_argument_checks(hip):
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import MFError, load, torch_device
    import torch
    p, nm, radius, _ = _ref("corner")
    far = p.copy()
    far[17, 1] = np.float32(2.0 ** 31) * np.float32(radius)          # |x / radius| >= 2^30
    with pytest.raises(MFError):
        ev.fpfh(far, nm, radius)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(MFError):
            ev.fpfh(p, nm, bad)
    with pytest.raises(ValueError):
        ev.fpfh(p, nm[:-1], radius)
    L = load()
    need = C.c_uint64(0)
    assert L.mf_cloud_fpfh_workspace(100, C.byref(need)) == 0 and need.value > 0
    assert L.mf_cloud_fpfh_workspace(-1, C.byref(need)) == -1 and L.mf_cloud_fpfh_workspace(100, None) == -1
    assert L.mf_cloud_fpfh_workspace((1 << 30) + 1, C.byref(need)) == -1
    assert L.mf_cloud_fpfh_workspace(100, C.byref(need)) == 0
    dev = torch_device()
    rec = torch.from_numpy(np.concatenate([p[:100], nm[:100]], 1).copy()).to(dev)
    ws = torch.zeros(int(need.value), dtype=torch.uint8, device=dev)
    out = torch.zeros((100, 33), dtype=torch.float32, device=dev)
    cnt = torch.zeros((100, 34), dtype=torch.int32, device=dev)
    args = [rec.data_ptr(), 6, 3, 100, 0.1, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), int(need.value), None]
    assert L.mf_cloud_fpfh_dev(*args) == 0
    for k, v in ((0, None), (1, 5), (2, 2), (2, -1), (2, 4), (3, -1), (3, (1 << 30) + 1), (4, 0.0), (4, float("nan")), (5, None), (7, None),
                 (7, ws.data_ptr() + 4), (8, int(need.value) - 1)):
        bad = list(args)
        bad[k] = v
        assert L.mf_cloud_fpfh_dev(*bad) == -1, k
    ok = list(args)
    ok[6] = None                                                       # the counts are optional
    assert L.mf_cloud_fpfh_dev(*ok) == 0
    # the matcher
    t = torch.zeros((10, 33), dtype=torch.float32, device=dev)
    idx = torch.zeros(10, dtype=torch.int32, device=dev)
    d2 = torch.zeros(10, dtype=torch.float32, device=dev)
    margs = [t.data_ptr(), 10, t.data_ptr(), 10, 33, idx.data_ptr(), d2.data_ptr(), None]
    assert L.mf_feature_match_dev(*margs) == 0 and idx.cpu().tolist() == [0] * 10
    for k, v in ((0, None), (1, -1), (1, (1 << 30) + 1), (2, None), (3, -1), (3, (1 << 30) + 1), (4, 0), (4, 65), (5, None), (6, None)):
        bad = list(margs)
        bad[k] = v
        assert L.mf_feature_match_dev(*bad) == -1, k
    with pytest.raises(ValueError):
        ev.match_features(np.zeros((4, 33), np.float32), np.zeros((4, 32), np.float32))
    with pytest.raises(MFError):
        ev.match_features(np.zeros((4, 65), np.float32), np.zeros((4, 65), np.float32))


# ---------------- 2. the matcher ----------------
@pytest.mark.parametrize("dim", [1, 33, 64])
def test_match_is_bit_exact(hip, dim):
    """sizes across the tile of 64 targets and the workgroup of 128 queries; planted copies (ties go to the smallest index), NaN rows"""
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(40 + dim)
    for nt in (1, 63, 64, 65, 1000):
        for nq in (1, 63, 64, 65, 1000):
            if dim == 1:        # small integers: many exact ties
                t = rng.integers(0, 8, (nt, dim)).astype(np.float32)
                q = rng.integers(0, 8, (nq, dim)).astype(np.float32)
            else:
                t = (rng.uniform(0, 100, (nt, dim)) * rng.uniform(0, 1, (nt, 1))).astype(np.float32)
                q = (rng.uniform(0, 100, (nq, dim)) * rng.uniform(0, 1, (nq, 1))).astype(np.float32)
            if nt >= 63:
                t[[7, 40, nt - 1]] = t[3]                               # copies of a target ...
                q[0] = t[3]                                             # ... and a query on them: d2 = 0 four times
                t[[5, nt - 2], [0, dim - 1]] = np.nan                   # rows with a NaN
                if nq >= 63:
                    q[nq - 1] = t[40]
                    q[[2, nq - 3], [dim - 1, 0]] = np.nan
                    q[9] = t[5]                                         # a query equal to a NaN row: a NaN itself
            wi, wd = fr.match(t, q)
            gi, gd = ev.match_features(t, q)
            assert gi.dtype == np.int32 and gd.dtype == np.float32
            assert (gi == wi).all() and gd.tobytes() == wd.tobytes(), (nt, nq)
            if nt >= 63:
                assert gd[0] == 0 and (gi[0] == 3 or dim == 1) and not np.isin(gi, [5, nt - 2]).any()
                if nq >= 63:
                    assert (gi[nq - 1] == 3 or dim == 1) and gi[[2, nq - 3, 9]].tolist() == [-1] * 3 and np.isinf(gd[[2, nq - 3, 9]]).all()
    gi, gd = ev.match_features(np.zeros((0, dim), np.float32), q)
    assert (gi == -1).all() and np.isinf(gd).all()
    gi, gd = ev.match_features(t, np.zeros((0, dim), np.float32))
    assert gi.shape == (0,) and gd.shape == (0,)


# ---------------- 3. end to end ----------------
def _coarse_ok(res, T, voxel):
    dt, dr = rr.pose_error(res["coarse"]["T"], T)
    print("coarse:", {k: v for k, v in res["coarse"].items() if k != "T"}, "error %.3g m %.3g deg" % (dt, np.degrees(dr)))
    assert dt <= 1.5 * voxel and np.degrees(dr) <= 5.0


def test_recovers_a_large_motion_without_a_start(hip):
    from maskfusion_amd import eval as ev
    est, en, ref, rn, T = gs.exact_pair()
    res = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0)
    dt, dr = rr.pose_error(res["T"], T)
    print("device: iterations", res["iterations"], "error", dt, dr, "share", res["inlier_share"], "rmse", res["rmse"])
    assert set(res) == {"T", "iterations", "inliers", "inlier_share", "rmse", "converged", "reason", "radius", "method", "trace", "coarse"}
    assert set(res["coarse"]) == {"T", "correspondences", "mutual", "inliers", "hypotheses", "tested", "key_points"}
    _coarse_ok(res, T, gs.VOXEL)
    assert res["converged"] and res["reason"] is None and res["radius"] == gs.VOXEL / 2
    assert dt < 1e-5 and dr < 1e-5                     # est is an exact image of ref: the gate of test_recovers_a_known_motion
    # the same pair through register() alone, from the identity and with the same radii, does not get there
    plain = ev.register(est, ref, gs.VOXEL / 2, ref_normals=rn, schedule=[1.5 * gs.VOXEL, 0.75 * gs.VOXEL, gs.VOXEL / 2])
    pt, pr = rr.pose_error(plain["T"], T)
    print("register() from the identity:", plain["converged"], plain["reason"], pt, pr)
    assert not (plain["converged"] and pt < 1e-5 and pr < 1e-5) and pt > 1.0
    # the coarse stage repeats for a seed, and other seeds land in the basin too
    again = ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=0, refine=False)
    assert again["reason"] == "not refined" and again["coarse"]["inliers"] == res["coarse"]["inliers"]
    assert np.abs(again["T"] - res["coarse"]["T"]).max() < 1e-9
    _coarse_ok(ev.register_global(est, ref, gs.VOXEL, est_normals=en, ref_normals=rn, seed=1, refine=False), T, gs.VOXEL)


def test_noisy_partial_overlap_agrees_with_the_restatement_driven_pipeline(hip, monkeypatch):
    """1 mm of noise, two different samples, est covers 70 % of the scene, normals estimated: gated like the noisy registration test
    (test_gpu_eval_register.test_noisy_variant_agrees_with_the_restatement), on convergence of both; the distance of the two final poses
    is reported (a flipped match or nearest neighbour is discrete, so it is not bounded in advance)"""
    from maskfusion_amd import eval as ev
    est, ref, T = gs.noisy_pair()
    res = ev.register_global(est, ref, gs.VOXEL, seed=0)
    _coarse_ok(res, T, gs.VOXEL)
    gs.patch(monkeypatch, ev)
    want = ev.register_global(est, ref, gs.VOXEL, seed=0)
    _coarse_ok(want, T, gs.VOXEL)
    print("device vs restatement-driven:", rr.pose_error(res["T"], want["T"]), "iterations", res["iterations"], want["iterations"],
          "device vs truth:", rr.pose_error(res["T"], T), "coarse inliers", res["coarse"]["inliers"], want["coarse"]["inliers"])
    assert res["converged"] and want["converged"]


# ---------------- the command ----------------
def test_eval_command_registers_without_an_init(hip, tmp_path):
    """a small exported map against its exact image under the 120 degree / 3 m motion, as a single reference file and without --init"""
    import test_gpu_eval_register as tr
    from maskfusion_amd import MaskFusion
    from maskfusion_amd import eval as ev
    st = tr._stream()
    m = MaskFusion(tr.W, tr.H, tr.F, tr.F, tr.W / 2.0, tr.H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, enableMultipleModels=False,
                   initConfidenceGlobal=1.0)
    for k in range(12):
        rgb, depth, _ = st.frame(k)
        m.processFrame(rgb, depth, timestamp=33333 * (k + 1))
    est_dir = tmp_path / "est"
    est_dir.mkdir()
    m.savePly(str(est_dir) + os.sep)
    m.close()
    pts, nrm = ev.read_ply(str(est_dir / "cloud-0.ply"), normals=True)
    assert nrm is not None and len(pts) > 5000
    T = gs.motion()
    tr._write_ply(str(tmp_path / "model.ply"), gs.moved(pts, T), (nrm.astype(np.float64) @ T[:3, :3].T).astype(np.float32))
    base = ["--est", str(est_dir), "--ref-cloud", str(tmp_path / "model.ply")]
    voxel = 0.1
    out = tr._eval_command(base + ["--register-global=%g" % voxel, "--init", "T.txt"])
    assert out.returncode == 2 and "--init" in out.stderr and out.stdout == ""
    out = tr._eval_command(base + ["--register-global=%g" % voxel])
    assert out.returncode == 0, out.stderr
    o = json.loads(out.stdout)
    reg = o["registration"]
    assert set(reg) == {"T", "rotation_rad", "translation_m", "iterations", "inliers", "inlier_share", "rmse", "converged", "reason", "radius",
                        "method", "coarse"}
    assert set(reg["coarse"]) == {"T", "correspondences", "mutual", "inliers", "hypotheses", "tested", "key_points"}
    dt, dr = rr.pose_error(np.array(reg["T"]), T)
    ct, cr = rr.pose_error(np.array(reg["coarse"]["T"]), T)
    print("registration:", reg["iterations"], "iterations, error", dt, dr, "coarse", ct, cr, reg["coarse"]["inliers"], "of", reg["coarse"]["correspondences"],
          "cloud rmse", o["cloud"]["accuracy"]["rmse"], "->", o["cloud_registered"]["accuracy"]["rmse"])
    assert reg["converged"] and reg["method"] == "plane" and reg["inlier_share"] >= 0.99 and reg["radius"] == voxel / 2
    assert dt < 1e-5 and dr < 1e-5 and ct <= 1.5 * voxel and np.degrees(cr) <= 5.0          # the exact image: the gate of the recovery test
    assert abs(reg["rotation_rad"] - np.deg2rad(120.0)) < 1e-5 and abs(reg["translation_m"] - 3.0) < 1e-5
    assert o["cloud_registered"]["accuracy"]["rmse"] < o["cloud"]["accuracy"]["rmse"]
    assert o["cloud_registered"]["accuracy"]["rmse"] < dt + 8.0 * dr + 2e-6 and o["cloud_registered"]["fscore"]["0.01"] == 1.0   # (|x| < 8 m)
