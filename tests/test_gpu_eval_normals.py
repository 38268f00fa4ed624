"""Cloud normals on the device (mf_cloud_normals_dev, maskfusion_amd.eval.estimate_normals / normal_consistency) against the brute-force
numpy restatement of tests/normals_restatement.py: the neighbour counts exactly, the normal and the surface variation where the
restatement's eigenvalue gap defines them, the orientation and no-normal rules, the registration fed with estimated normals and the command
end to end.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build.

The normal gate (1e-9 rad, 1e-9 on the variation) bounds the fp64 results, and the device stores fp32.  Rounding to fp32 is monotonic, so
a device value d within 1e-9 of the restatement's fp64 value r is stored inside [fl32(r - 1e-9), fl32(r + 1e-9)], and that is what
_stored_within asserts, per component for the normal (unit vectors at an angle t differ by 2 sin(t / 2) <= t in every component).  The two
fp64 results differ by about k 2^-53 over the relative gap (1e-14), so the interval is the one fp32 value fl32(r) unless an fp32 rounding
boundary lies within 1e-9 of r (a few values in 100 for a component near 0.5, whose ulp is 6e-8), where it holds the value on either side
of the boundary: the bucket order of a call, which moves the device's last fp64 bits, cannot fail the gate."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import normals_restatement as nr  # noqa: E402
import register_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

SIGMA = 0.002
SPHERE_C = np.array([2.0, 0.5, 0.5])


def _sphere(rng, n, centre=SPHERE_C, R=0.5):
    v = rng.normal(size=(n, 3))
    return centre + R * v / np.linalg.norm(v, axis=1)[:, None]


def _corner(rng, n):
    """three unit squares that meet in the origin: the planes x = 0, y = 0 and z = 0"""
    uv = rng.uniform(0, 1, (n, 2))
    axis = np.arange(n) % 3
    p = np.zeros((n, 3))
    for a in range(3):
        m = axis == a
        p[np.ix_(m, [k for k in range(3) if k != a])] = uv[m]
    return p


def _noisy(rng, p):
    return (p + rng.normal(scale=SIGMA, size=p.shape)).astype(np.float32)


def _clouds():
    rng = np.random.default_rng(21)
    both = np.concatenate([_sphere(rng, 2000), _corner(rng, 2000)])
    return {"sphere": (_noisy(rng, _sphere(rng, 4000)), 0.15), "corner": (_noisy(rng, _corner(rng, 3000)), 0.10), "both": (_noisy(rng, both), 0.12)}


_cache = {}


def _ref(name, viewpoint=None):
    """the cloud, its radius and the restatement's result, computed once and shared (treat as read-only)"""
    key = (name, None if viewpoint is None else tuple(viewpoint))
    if key not in _cache:
        if "clouds" not in _cache:
            _cache["clouds"] = _clouds()
        pts, radius = _cache["clouds"][name]
        _cache[key] = (pts, radius, nr.estimate(pts, radius, 5, viewpoint))
    return _cache[key]


def _same_nan(n, var, want):
    assert (np.isnan(n).any(1) == np.isnan(want["normal"]).any(1)).all()
    assert (np.isnan(n).all(1) == np.isnan(n).any(1)).all() and (np.isnan(var) == np.isnan(n).any(1)).all()


TOL = 1e-9


def _stored_within(got32, want64, tol=TOL):
    """got32 can be the fp32 store of an fp64 value within tol of want64 (see the head of the file)"""
    want64 = np.asarray(want64, np.float64)
    return (got32 >= (want64 - tol).astype(np.float32)) & (got32 <= (want64 + tol).astype(np.float32))


def _check_gated(n, var, want, cap=0.05):
    """the issue's gate on the restatement's well-defined points; at most `cap` of the cloud outside them"""
    g = nr.gated(want)
    print("outside the gated set: %.2f %% (no normal: %.2f %%)" % (100 * (1 - g.mean()), 100 * np.isnan(want["normal"]).any(1).mean()))
    assert 1 - g.mean() <= cap
    ang = nr.angle(n[g], want["normal64"][g])
    dv = np.abs(var[g].astype(np.float64) - want["variation64"][g])
    other = (n[g] != want["normal"][g]).sum() + (var[g] != want["variation"][g]).sum()
    print("gated points %d: stored against fp64, max angle %.3g rad, max variation difference %.3g; %d stored values are not the "
          "restatement's bits" % (g.sum(), ang.max(initial=0.0), dv.max(initial=0.0), other))
    assert _stored_within(n[g], want["normal64"][g]).all() and _stored_within(var[g], want["variation64"][g]).all()
    return g


# ---------------- 1. counts ----------------
@pytest.mark.parametrize("name", ["sphere", "corner", "both"])
def test_counts_are_exact(hip, name):
    from maskfusion_amd import eval as ev
    pts, radius, want = _ref(name)
    _, _, cnt = ev.estimate_normals(pts, radius)
    assert cnt.dtype == np.int32 and (cnt == want["count"]).all() and cnt.min() >= 1


def test_counts_with_strides_nan_rows_and_tiny_clouds(hip):
    from maskfusion_amd import eval as ev
    pts, radius, want = _ref("corner")
    rng = np.random.default_rng(22)
    base = ev.estimate_normals(pts, radius)
    for stride in (3, 11):
        rec = rng.normal(size=(len(pts), stride)).astype(np.float32)
        rec[:, :3] = pts
        n, var, cnt = ev.estimate_normals(rec, radius)
        assert (cnt == want["count"]).all()
        _same_nan(n, var, want)
    # NaN / +-inf rows: count 0, no normal, and they are nobody's neighbour
    bad = pts.copy()
    rows = rng.choice(len(bad), 60, replace=False)
    bad[rows[:20], 0] = np.nan
    bad[rows[20:40], 1] = np.inf
    bad[rows[40:], 2] = -np.inf
    wb = nr.estimate(bad, radius)
    n, var, cnt = ev.estimate_normals(bad, radius)
    assert (cnt == wb["count"]).all() and (cnt[rows] == 0).all() and np.isnan(n[rows]).all() and np.isnan(var[rows]).all()
    assert (cnt != want["count"]).any()
    _same_nan(n, var, wb)
    _check_gated(n, var, wb)
    # one point, no point
    n, var, cnt = ev.estimate_normals(pts[:1], radius)
    assert cnt.tolist() == [1] and np.isnan(n).all() and np.isnan(var).all()
    n, var, cnt = ev.estimate_normals(np.zeros((0, 3), np.float32), radius)
    assert n.shape == (0, 3) and var.shape == (0,) and cnt.shape == (0,)
    assert base[2].tobytes() == ev.estimate_normals(pts, radius)[2].tobytes()


def test_radius_test_is_inclusive_on_a_lattice(hip):
    """a 5 x 5 x 5 lattice of spacing 2^-2 searched with radius 2^-2: the six axis neighbours lie at exactly d2 = fl(r * r)"""
    from maskfusion_amd import eval as ev
    g = np.arange(5, dtype=np.float32) * np.float32(0.25) - np.float32(0.5)
    pts = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    want = nr.estimate(pts, 0.25)
    n, var, cnt = ev.estimate_normals(pts, 0.25)
    assert (cnt == want["count"]).all() and cnt.max() == 7 and cnt.min() == 4 and cnt[62] == 7       # 62: the centre
    _same_nan(n, var, want)
    assert (ev.estimate_normals(pts, np.nextafter(np.float32(0.25), np.float32(0)))[2] == 1).all()


# ---------------- 2. normals ----------------
@pytest.mark.parametrize("name", ["sphere", "corner", "both"])
def test_normals_and_variation_on_the_gated_points(hip, name):
    from maskfusion_amd import eval as ev
    pts, radius, want = _ref(name)
    n, var, _ = ev.estimate_normals(pts, radius)
    assert n.dtype == np.float32 and n.shape == (len(pts), 3) and var.dtype == np.float32 and var.shape == (len(pts),)
    _same_nan(n, var, want)
    ok = ~np.isnan(var)
    assert np.abs(np.linalg.norm(n[ok].astype(np.float64), axis=1) - 1).max() < 2e-7 and (var[ok] <= 1 / 3 + 1e-7).all()
    g = _check_gated(n, var, want)
    if name == "corner":        # away from the edges the normal is the face's
        face = g & (pts.min(1) > -0.01) & (np.sort(pts, 1)[:, 1] > 0.12)
        assert face.sum() > 1500 and (np.abs(n[face]).max(1) > 0.99).all()


# ---------------- 3. rules ----------------
def test_a_line_has_no_normal(hip):
    from maskfusion_amd import eval as ev
    t = np.arange(40, dtype=np.float32)[:, None]
    pts = t * np.array([[1, 2, 3]], np.float32) / np.float32(8)          # exact in fp32: collinear to the bit
    radius = 1.5
    want = nr.estimate(pts, radius)
    n, var, cnt = ev.estimate_normals(pts, radius)
    assert (cnt == want["count"]).all() and cnt.max() == 7 and cnt.min() == 4
    assert np.isnan(n).all() and np.isnan(var).all() and np.isnan(want["normal"]).all()
    # coincident points
    n, var, cnt = ev.estimate_normals(np.tile(np.array([[0.3, -0.2, 0.1]], np.float32), (9, 1)), 0.1)
    assert (cnt == 9).all() and np.isnan(n).all()


def test_min_neighbours_is_honoured(hip):
    from maskfusion_amd import eval as ev
    pts, _, _ = _ref("sphere")
    radius, m = 0.03, 7
    want = nr.estimate(pts, radius, m)
    n, var, cnt = ev.estimate_normals(pts, radius, m)
    assert (cnt == want["count"]).all()
    at, below = cnt == m, cnt == m - 1
    assert at.sum() > 20 and below.sum() > 20
    assert np.isnan(n[below]).all() and np.isfinite(n[at]).all() and np.isnan(n[cnt < m]).all() and np.isfinite(n[cnt >= m]).all()
    _same_nan(n, var, want)


def test_orientation(hip):
    from maskfusion_amd import eval as ev
    for name, view in (("sphere", None), ("sphere", SPHERE_C), ("corner", None), ("corner", (0.9, 0.7, 1.3)), ("both", (5.0, -1.0, 2.5))):
        pts, radius, want = _ref(name, view)
        n, var, cnt = ev.estimate_normals(pts, radius, viewpoint=view)
        g = nr.gated(want)
        # the restatement's sign on every gated point (the gate of the normals holds the rest: an opposite sign is an angle of pi)
        assert ((n[g].astype(np.float64) * want["normal"][g]).sum(1) > 0).all(), (name, view)
        assert _stored_within(n[g], want["normal64"][g]).all()
        ok = ~np.isnan(var)
        if view is None:
            lead = np.take_along_axis(n[ok], np.argmax(np.abs(n[ok]), 1)[:, None], 1)
            assert (lead > 0).all()
        else:
            assert ((n[ok].astype(np.float64) * (np.asarray(view, np.float64) - pts[ok])).sum(1) >= 0).all()
        if name == "sphere" and view is not None:      # the centre as viewpoint: inwards everywhere
            assert ok.all() and ((n.astype(np.float64) * (pts - SPHERE_C)).sum(1) < -0.9 * 0.5).all()


def test_argument_checks(hip):
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import MFError, load, torch_device
    import torch
    pts, radius, _ = _ref("corner")
    far = pts.copy()
    far[17, 1] = np.float32(2.0 ** 31) * np.float32(radius)          # |x / radius| >= 2^30
    with pytest.raises(MFError):
        ev.estimate_normals(far, radius)
    for bad in (2, 0, -1):
        with pytest.raises(MFError):
            ev.estimate_normals(pts, radius, min_neighbours=bad)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(MFError):
            ev.estimate_normals(pts, bad)
    with pytest.raises(MFError):
        ev.estimate_normals(pts, radius, viewpoint=(0.0, np.nan, 0.0))
    assert ev.estimate_normals(pts, radius, min_neighbours=3)[2].min() >= 1
    L = load()
    need = C.c_uint64(0)
    assert L.mf_cloud_normals_workspace(100, C.byref(need)) == 0 and need.value > 0
    assert L.mf_cloud_normals_workspace(-1, C.byref(need)) == -1 and L.mf_cloud_normals_workspace(100, None) == -1
    assert L.mf_cloud_normals_workspace((1 << 30) + 1, C.byref(need)) == -1
    assert L.mf_cloud_normals_workspace(100, C.byref(need)) == 0
    dev = torch_device()
    p = torch.from_numpy(pts[:100].copy()).to(dev)
    ws = torch.zeros(int(need.value), dtype=torch.uint8, device=dev)
    out = torch.zeros((100, 4), dtype=torch.float32, device=dev)
    cnt = torch.zeros(100, dtype=torch.int32, device=dev)
    args = [p.data_ptr(), 3, 100, 0.1, 5, None, out.data_ptr(), cnt.data_ptr(), ws.data_ptr(), int(need.value), None]
    assert L.mf_cloud_normals_dev(*args) == 0
    for k, v in ((0, None), (1, 2), (2, -1), (2, (1 << 30) + 1), (3, 0.0), (4, 2), (6, None), (7, None), (8, None), (8, ws.data_ptr() + 4),
                 (9, int(need.value) - 1)):
        bad = list(args)
        bad[k] = v
        assert L.mf_cloud_normals_dev(*bad) == -1, k


# ---------------- 4. neighbourhoods ----------------
def test_two_radii_on_one_cloud(hip):
    """the corner cloud (about 1000 points per unit square: mean spacing 0.03) at its own radius and at 0.02, where most points stand alone"""
    from maskfusion_amd import eval as ev
    pts, radius, want = _ref("corner")
    small = nr.estimate(pts, 0.02)
    n, var, cnt = ev.estimate_normals(pts, 0.02)
    assert (cnt == small["count"]).all()
    _same_nan(n, var, small)
    assert np.isnan(var).mean() > 0.5 and (cnt[np.isnan(var)] < 5).all()
    # the few points with k >= 5 there: the solve on small neighbourhoods, no cap on how many the gap rule leaves out
    g = _check_gated(n, var, small, cap=1.0)
    assert g.sum() >= 20 and cnt[g].max() <= 12
    n2, var2, cnt2 = ev.estimate_normals(pts, radius)
    assert (cnt2 == want["count"]).all() and (cnt2 >= cnt).all() and not np.isnan(var2).any()


def test_a_radius_that_spans_the_cloud(hip):
    """300 points, every one the neighbour of every other: the whole 27-cell walk and long buckets"""
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(23)
    pts = (rng.uniform(-0.5, 0.5, (300, 3)) * [0.5, 0.3, 0.1] + [0.3, -0.2, 0.4]).astype(np.float32)
    want = nr.estimate(pts, 1.0)
    n, var, cnt = ev.estimate_normals(pts, 1.0)
    assert (cnt == 300).all() and (want["count"] == 300).all()
    g = _check_gated(n, var, want, cap=0.0)
    assert g.all() and (np.abs(n[:, 2]) > 0.9).all()


# ---------------- 5. registration with estimated normals ----------------
def test_registration_with_estimated_normals(hip):
    """the registration test's scene (an exact sample of the room's surface moved by a known small transform): point-to-plane on estimated
    normals ends where it ends on the analytic ones, and no later than point-to-point"""
    from maskfusion_amd import eval as ev
    import test_gpu_eval_register as tr
    ref, nrm, _ = tr._room(60_000)
    rng = np.random.default_rng(11)
    T_true = tr._pose([2.0, -3.0, 1.5], [0.03, -0.02, 0.04])
    est = tr._moved(ref[rng.choice(len(ref), 20_000, replace=False)], np.linalg.inv(T_true))
    en, _, cnt = ev.estimate_normals(ref, 0.08)
    missing = np.isnan(en).any(1)
    print("estimated normals: %d of %d without, median neighbours %d" % (missing.sum(), len(ref), np.median(cnt)))
    assert missing.mean() < 0.05
    a = ev.register(est, ref, 0.10, ref_normals=nrm)
    e = ev.register(est, ref, 0.10, ref_normals=en)
    p = ev.register(est, ref, 0.10, method="point")
    dt, dr = rr.pose_error(e["T"], a["T"])
    print("iterations: analytic normals %d, estimated normals %d, point-to-point %d (converged %s); estimated vs analytic %.3g m %.3g rad; "
          "vs truth %s" % (a["iterations"], e["iterations"], p["iterations"], p["converged"], dt, dr, rr.pose_error(e["T"], T_true)))
    assert a["converged"] and e["converged"] and e["method"] == "plane"
    assert dt <= 1e-5 and dr <= 1e-5
    assert e["iterations"] <= p["iterations"]
    # a row without a normal is no target.  Asking for 12 neighbours leaves a good part of the reference without one; at a radius of
    # 5 mm under the true transform an est point has its own reference point 1e-7 m away and hardly ever another within reach, so it
    # keeps its partner only while that row has a normal: the pairs of a step are nearest()'s against the reference without those rows
    en12 = ev.estimate_normals(ref, 0.08, min_neighbours=12)[0]
    missing = np.isnan(en12).any(1)
    assert missing.any() and not missing.all() and (np.isnan(en12).all(1) == missing).all()
    kept = ref.copy()
    kept[missing] = np.nan
    for radius in (0.005, 0.10):
        pairs_all = int(np.isfinite(ev.nearest(ref, est, radius, T=T_true)[0]).sum())
        pairs_kept = int(np.isfinite(ev.nearest(kept, est, radius, T=T_true)[0]).sum())
        pairs_step = int(ev.Registration(ref, radius, en12, len(est)).step(est, T_true)[28])
        print("radius %g: %d rows of %d without a normal; pairs %d with all rows, %d without those, the step's %d"
              % (radius, missing.sum(), len(ref), pairs_all, pairs_kept, pairs_step))
        assert pairs_step == pairs_kept and 0 < pairs_kept
        assert pairs_kept < pairs_all or radius == 0.10
        assert int(ev.Registration(ref, radius, nrm, len(est)).step(est, T_true)[28]) == pairs_all


# ---------------- 6. normal_consistency ----------------
def test_normal_consistency_of_a_known_rotation(hip):
    from maskfusion_amd import eval as ev
    pts, radius, want = _ref("sphere")
    n = want["normal64"]
    ok = np.isfinite(n).all(1)
    pts, n = pts[ok], n[ok]
    # rotate every normal by 5 degrees about an axis perpendicular to it
    axis = np.cross(n, [0.3, -0.5, 0.8])
    axis /= np.linalg.norm(axis, axis=1)[:, None]
    th = np.deg2rad(5.0)
    turned = n * np.cos(th) + np.cross(axis, n) * np.sin(th)
    res = ev.normal_consistency(pts, turned, pts, n, 0.01)
    print(res)
    assert res["count"] == res["pairs"] == len(pts)
    assert abs(res["mean_deg"] - 5.0) <= 1e-4 and abs(res["median_deg"] - 5.0) <= 1e-4
    assert res["below"] == {"10": 1.0, "20": 1.0, "30": 1.0}
    # the orientation of either side does not matter, and T turns the est normals with the points
    flipped = np.where((np.arange(len(n)) % 2 == 0)[:, None], -turned, turned)
    assert abs(ev.normal_consistency(pts, flipped, pts, n, 0.01)["mean_deg"] - 5.0) <= 1e-4
    T = tr_pose()
    back = (pts.astype(np.float64) - T[:3, 3]) @ T[:3, :3]
    res = ev.normal_consistency(back.astype(np.float32), turned @ T[:3, :3], pts, n, 0.01, T=T)
    assert res["pairs"] == len(pts) and abs(res["mean_deg"] - 5.0) <= 1e-4


def tr_pose():
    from maskfusion_amd import synth
    return synth.make_pose(synth.rot_xyz(*np.deg2rad([10.0, -20.0, 30.0])), [0.1, -0.2, 0.3]).astype(np.float64)


# ---------------- the command ----------------
def test_eval_command_estimates_the_reference_normals(hip, tmp_path):
    import test_gpu_eval_register as tr
    ref, nrm, _ = tr._room(40_000)
    M = tr._pose([1.5, -2.0, 1.0], [0.02, -0.015, 0.03])
    est_dir = tmp_path / "est"
    est_dir.mkdir()
    tr._write_ply(str(est_dir / "cloud-0.ply"), ref[::2], nrm[::2])
    moved = tr._moved(ref, M)
    tr._write_ply(str(tmp_path / "bare.ply"), moved)
    base = ["--est", str(est_dir), "--ref-cloud", str(tmp_path / "bare.ply"), "--register", "--register-radius", "0.2,0.1"]
    out = tr._eval_command(base)
    assert out.returncode == 2 and "has no normals" in out.stderr and out.stdout == ""
    out = tr._eval_command(base + ["--estimate-normals=0.08", "--normals"])
    assert out.returncode == 0, out.stderr
    o = json.loads(out.stdout)
    rn = o["reference_normals"]
    assert rn["estimated"] is True and rn["radius"] == 0.08 and 0 <= rn["without_normal"] < 0.05 * len(ref)
    reg = o["registration"]
    dt, dr = rr.pose_error(np.array(reg["T"]), M)
    print("registration on estimated normals:", reg["iterations"], "iterations, error", dt, dr, o["normal_consistency"])
    assert reg["method"] == "plane" and reg["converged"] and dt <= 1e-5 and dr <= 1e-5
    nc = o["normal_consistency"]
    assert nc["count"] == len(ref[::2]) and nc["pairs"] > 0.9 * nc["count"] and nc["median_deg"] < 1.0 and nc["below"]["30"] > 0.9
    # the default radius is twice --radius
    out = tr._eval_command(base + ["--estimate-normals", "--radius", "0.04"])
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["reference_normals"]["radius"] == 0.08
