"""Cloud registration on the device (mf_cloud_icp_build_dev / mf_cloud_icp_step_dev, maskfusion_amd.eval.register) against the numpy / scipy
restatement of tests/register_restatement.py: the correspondence set, the Gauss-Newton system within a bound derived from the restatement's
own terms, determinism, the loop teacher-forced step by step, recovery of a known motion, degenerate input and the command end to end.
Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import register_restatement as rr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"
W, H, F = 320, 240, 264.0


def _stream():
    from maskfusion_amd import synth
    return synth.Stream(W=W, H=H, fx=F, fy=F, cx=W / 2.0, cy=H / 2.0, noise=False)


def _room(n):
    """the synthetic room's surface (five planes and the standing boxes: well more than three non-parallel faces): positions, unit normals"""
    from maskfusion_amd import synth
    rec = synth.dense_room_map(_stream().scene, n, last_time=0.0)
    return np.ascontiguousarray(rec[:, :3]), np.ascontiguousarray(rec[:, 8:11]), rec


def _pose(deg, t):
    from maskfusion_amd import synth
    return synth.make_pose(synth.rot_xyz(*np.deg2rad(deg)), t).astype(np.float64)


def _moved(pts, T):
    return (pts.astype(np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def _case(n_ref, n_est, seed, noise=0.003):
    """ref with normals, est = a jittered sample of it moved away by a non-trivial T^-1, and T"""
    ref, nrm, rec = _room(n_ref)
    rng = np.random.default_rng(seed)
    T = _pose([3.0, -2.0, 4.0], [0.04, -0.03, 0.02])
    sub = rng.choice(len(ref), n_est, replace=False)
    est = _moved(ref[sub] + rng.normal(scale=noise, size=(n_est, 3)).astype(np.float32), np.linalg.inv(T))
    return ref, nrm, rec, est, T


def _within(dev, s, a, terms):
    """the derived gate: every entry within terms * 2^-53 * sum |term| * 4 of the restatement (rr.bound); the pair count exactly"""
    err, b = np.abs(dev - s), rr.bound(a, terms)
    print("max error / bound over the 29 entries: %.3g" % np.max(err / np.maximum(b, 1e-300)), "pairs", int(dev[28]))
    assert dev[28] == s[28]
    assert (err <= b).all(), (np.flatnonzero(err > b), err, b)


def test_step_counts_the_correspondences_of_nearest(hip):
    from maskfusion_amd import eval as ev
    ref, nrm, _, est, T = _case(200_000, 100_000, 1)
    Tn = T.copy()
    Tn[:3, 3] += [0.01, 0.02, -0.015]      # not the aligning transform: some queries lose their partner
    for radius in (0.05, 0.01):
        dist, idx = ev.nearest(ref, est, radius, T=Tn)
        n = int(np.isfinite(dist).sum())
        assert 0 < n and (n < len(est) or radius == 0.05)
        for normals in (nrm, None):
            s = ev.Registration(ref, radius, normals, len(est)).step(est, Tn)
            assert int(s[28]) == n, (radius, normals is None)
        # ... and they are the same pairs: the restatement's fp32-ranked cKDTree correspondences equal nearest()'s indices
        assert (rr.correspondences(ref, rr.transform_f32(Tn, est), radius) == idx).all()


@pytest.mark.parametrize("method", ["plane", "point"])
def test_system_within_the_derived_bound(hip, method):
    """the 29 doubles against the restatement evaluated on nearest()'s own correspondences and the same fp32 x'; NaN queries, targets and
    normals; strides 3, 4 and 12"""
    from maskfusion_amd import eval as ev
    ref, nrm, rec, est, T = _case(150_000, 120_000, 2)
    rng = np.random.default_rng(3)
    rec = rec.copy()
    bad_t = rng.choice(len(rec), 300, replace=False)
    rec[bad_t[:100], 0] = np.nan
    rec[bad_t[100:200], 2] = np.inf
    rec[bad_t[200:], 9] = np.nan                       # a NaN normal takes the target out (point-to-plane only)
    est = est.copy()
    est[rng.choice(len(est), 50, replace=False), 1] = np.nan
    T = T.copy()
    T[:3, 3] += [0.004, -0.006, 0.005]
    radius = 0.05
    plane = method == "plane"
    usable = np.isfinite(rec[:, :3]).all(1) & (np.isfinite(rec[:, 8:11]).all(1) if plane else True)
    tgt = rec[:, :3].copy()
    tgt[~usable] = np.nan
    dist, idx = ev.nearest(tgt, est, radius, T=T)
    hit = idx >= 0
    assert 0.5 < hit.mean() < 1.0
    xq = rr.transform_f32(T, est)
    s, a, terms = rr.system(xq[hit], rec[idx[hit], :3], rec[idx[hit], 8:11] if plane else None)
    assert terms == (1 if plane else 3) * int(hit.sum())
    got = []
    for q_stride in (3, 4, 12):
        q = rng.normal(size=(len(est), q_stride)).astype(np.float32)
        q[:, :3] = est
        if plane:       # targets: 12-float records with the normal at 8, and xyz | normal rows of 6 built from a separate normal array
            regs = [ev.Registration(rec, radius, 8, len(est)), ev.Registration(rec[:, :3], radius, rec[:, 8:11], len(est))]
        else:           # targets of stride 3, 4 and 12 without normals
            regs = [ev.Registration(np.ascontiguousarray(rec[:, :k]), radius, None, len(est)) for k in (3, 4, 12)]
        for reg in regs:
            dev = reg.step(q, T)
            _within(dev, s, a, terms)
            got.append(dev.tobytes())
    assert len(set(got)) == 1                           # strides change nothing


SCHEDULE_WORKER = r'''
import os, sys
sys.path[:0] = [%(root)r, os.path.join(%(root)r, "tests"), os.path.join(%(root)r, "tests", "hipcpu")]
import numpy as np
import emu
emu.activate()
import test_gpu_eval_register as t
from maskfusion_amd import eval as ev
ref, nrm, rec, est, T = t._case(60_000, 40_000, 4)
for normals in (nrm, None):
    print(ev.Registration(ref, 0.05, normals, len(est)).step(est, T).tobytes().hex())
'''


def test_step_is_deterministic(hip):
    from maskfusion_amd import eval as ev
    ref, nrm, _, est, T = _case(60_000, 40_000, 4)
    for normals in (nrm, None):
        reg = ev.Registration(ref, 0.05, normals, len(est))
        a, b = reg.step(est, T), reg.step(est, T)
        c = ev.Registration(ref, 0.05, normals, len(est)).step(est, T)
        assert a.tobytes() == b.tobytes() == c.tobytes() and a[28] > 1000
    # the CPU-executed build under the forward and the reversed thread / workgroup schedule: the same bits
    outs = []
    for schedule in (None, "reverse"):
        env = dict(os.environ)
        env.pop("HIPCPU_SCHEDULE", None)
        if schedule:
            env["HIPCPU_SCHEDULE"] = schedule
        r = subprocess.run([sys.executable, "-c", SCHEDULE_WORKER % dict(root=ROOT)], capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, r.stderr
        outs.append(r.stdout.split())
    assert len(outs[0]) == 2 and outs[0] == outs[1]


def test_loop_teacher_forced(hip):
    """register() with the trace on: at every iteration the device's T goes to the restatement, whose system must agree within the bound and
    whose solve (numpy LU, SciPy rotation) must give the same update to 1e-12 relative"""
    from maskfusion_amd import eval as ev
    ref, nrm, _, est, T_true = _case(150_000, 50_000, 5, noise=0.001)
    for method, normals in (("plane", nrm), ("point", None)):
        res = ev.register(est, ref, 0.10, ref_normals=normals, method=method, max_iterations=8, schedule=[0.10, 0.05], trace=True)
        assert len(res["trace"]) >= 4
        T_next = None
        for k, it in enumerate(res["trace"]):
            if T_next is not None:
                assert np.abs(it["T"] - T_next).max() <= 1e-12 * max(1.0, np.abs(T_next).max()), (method, k)
            s, a, terms, _ = rr.step_system(ref, normals, est, it["radius"], it["T"])
            _within(it["sys29"], s, a, terms)
            x = rr.solve(it["sys29"])
            assert np.abs(it["x"] - x).max() <= 1e-12 * np.abs(x).max() + 1e-300, (method, k, it["x"], x)
            T_next = rr.update(it["T"], it["x"])
        assert np.abs(res["T"] - T_next).max() <= 1e-12 * np.abs(T_next).max()
        dt, dr = rr.pose_error(res["T"], T_true)
        print(method, "iterations", res["iterations"], "converged", res["converged"], "error", dt, dr)
        # (1 mm of noise on the points; the recovery test gates the exact case.  Point-to-point slides along the lattice of the synthetic
        # surface and stalls within a cell of it: its pose is reported, not gated)
        assert method == "point" or (dt < 2e-3 and dr < 2e-3)


def _recovery_input(noisy):
    ref, nrm, _ = _room(200_000)
    rng = np.random.default_rng(11)
    sub = rng.choice(len(ref), 60_000, replace=False)
    # Chosen on the CPU with the restatement alone: rotations of 2, -3 and 1.5 degrees about x, y, z and 3, -2, 4 cm at a 10 cm radius; it
    # converges in 5 iterations to 5e-8 m / 2.5e-9 rad with every query paired (6 iterations, 1.3e-4 m / 1.4e-5 rad for the noisy variant)
    T_true = _pose([2.0, -3.0, 1.5], [0.03, -0.02, 0.04])
    pts = ref[sub]
    if noisy:       # 1 mm of Gaussian noise, and est's points removed from ref
        pts = pts.astype(np.float64) + rng.normal(scale=1e-3, size=pts.shape)
        keep = np.setdiff1d(np.arange(len(ref)), sub)
        ref, nrm = ref[keep], nrm[keep]
    est = _moved(np.asarray(pts), np.linalg.inv(T_true))
    return ref, nrm, est, T_true


def test_recovers_a_known_motion(hip):
    from maskfusion_amd import eval as ev
    ref, nrm, est, T_true = _recovery_input(False)
    Tr, it_r, conv_r, share_r = rr.register(est, ref, nrm, 0.10)
    dt_r, dr_r = rr.pose_error(Tr, T_true)
    print("restatement: iterations", it_r, "error", dt_r, dr_r, "share", share_r)
    assert conv_r and share_r == 1.0 and dt_r < 1e-5 and dr_r < 1e-5          # the input is fit for the gate
    res = ev.register(est, ref, 0.10, ref_normals=nrm)
    dt, dr = rr.pose_error(res["T"], T_true)
    print("device: iterations", res["iterations"], "error", dt, dr, "share", res["inlier_share"], "rmse", res["rmse"])
    assert res["converged"] and res["reason"] is None
    assert res["inlier_share"] >= 0.99
    # est is an exact subset of ref moved by T_true^-1: the truth is a fixed point (every residual 0) up to the fp32 transform's rounding,
    # 6e-8 x 5 m; 1e-5 leaves 20 x
    assert dt < 1e-5 and dr < 1e-5
    assert res["rmse"] < 1e-5
    # point-to-point on the same input, from a start within half a cell of the lattice (2 cm) everywhere: the same fixed point
    near = _pose([0.05, -0.05, 0.05], [0.002, -0.002, 0.002]) @ T_true
    res = ev.register(est, ref, 0.05, T0=near, method="point")
    dt, dr = rr.pose_error(res["T"], T_true)
    print("device, point-to-point: iterations", res["iterations"], "error", dt, dr)
    assert res["converged"] and dt < 1e-5 and dr < 1e-5


def test_noisy_variant_agrees_with_the_restatement(hip):
    """1 mm of noise, est disjoint from ref: gated on convergence only; the distance to the restatement's final T is reported (a flipped
    nearest-neighbour choice is discrete, so it is not bounded in advance)"""
    from maskfusion_amd import eval as ev
    ref, nrm, est, T_true = _recovery_input(True)
    Tr, it_r, conv_r, _ = rr.register(est, ref, nrm, 0.10)
    res = ev.register(est, ref, 0.10, ref_normals=nrm)
    print("device vs restatement:", rr.pose_error(res["T"], Tr), "iterations", res["iterations"], it_r, "device vs truth:", rr.pose_error(res["T"], T_true))
    assert res["converged"] and conv_r


def test_degenerate_input_is_reported(hip):
    from maskfusion_amd import eval as ev
    rng = np.random.default_rng(6)
    # a single plane: rank 3
    xy = rng.uniform(-1, 1, (20000, 2)).astype(np.float32)
    plane = np.concatenate([xy, np.full((len(xy), 1), 1.5, np.float32)], 1)
    nrm = np.tile(np.array([0, 0, 1], np.float32), (len(xy), 1))
    est = plane[:5000] + np.array([0, 0, 0.01], np.float32)
    res = ev.register(est, plane, 0.05, ref_normals=nrm)
    assert res["converged"] is False and "rank deficient" in res["reason"] and res["iterations"] == 0
    assert np.array_equal(res["T"], np.eye(4))
    # fewer than 6 correspondences
    ref, rn, _ = _room(20000)
    res = ev.register(ref[:5], ref, 0.05, ref_normals=rn)
    assert res["converged"] is False and "fewer than 6" in res["reason"] and res["inliers"] == 5
    res = ev.register(ref[:1000] + np.float32(50.0), ref, 0.05, ref_normals=rn)     # nothing in range
    assert res["converged"] is False and "fewer than 6" in res["reason"] and res["inliers"] == 0 and res["rmse"] is None
    res = ev.register(np.zeros((0, 3), np.float32), ref, 0.05, method="point")
    assert res["converged"] is False and res["inlier_share"] == 0.0
    with pytest.raises(ValueError, match="normals"):
        ev.register(ref[:100], ref, 0.05)                  # point-to-plane without normals
    # an iteration cap that is too small is said so
    _, _, est, _ = _recovery_input(False)
    ref, rn, _ = _room(200_000)
    res = ev.register(est, ref, 0.10, ref_normals=rn, max_iterations=1)
    assert res["converged"] is False and "within 1 iterations" in res["reason"] and res["iterations"] == 1


def test_argument_checks(hip):
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import MFError, load, torch_device
    import torch
    L = load()
    rng = np.random.default_rng(7)
    t = rng.uniform(-1, 1, (100, 6)).astype(np.float32)
    q = rng.uniform(-1, 1, (10, 3)).astype(np.float32)
    for bad in (0.0, -1.0, float("nan"), float("inf")):
        with pytest.raises(MFError):
            ev.Registration(t, bad, 3)
    with pytest.raises(MFError):
        ev.Registration(t * np.float32(2 ** 31 * 0.01), 0.01, None)        # |x / r| >= 2^30
    reg = ev.Registration(t, 1.0, 3, 10)
    with pytest.raises(MFError):
        reg.step(q * np.float32(2 ** 31), None)
    Tbad = np.eye(4)
    Tbad[1, 2] = np.nan
    with pytest.raises(MFError):
        reg.step(q, Tbad)
    with pytest.raises(MFError):
        reg.step(np.zeros((11, 3), np.float32))                               # more queries than the workspace was sized for
    assert reg.step(q)[28] >= 0
    need = C.c_uint64(0)
    assert L.mf_cloud_icp_workspace(100, 10, C.byref(need)) == 0 and need.value > 0
    assert L.mf_cloud_icp_workspace(-1, 10, C.byref(need)) == -1 and L.mf_cloud_icp_workspace(100, -1, C.byref(need)) == -1
    assert L.mf_cloud_icp_workspace(100, 10, None) == -1
    dev = torch_device()
    dt, dq = torch.from_numpy(t).to(dev), torch.from_numpy(q).to(dev)
    ws = torch.zeros(int(need.value), dtype=torch.uint8, device=dev)
    out = torch.zeros(29, dtype=torch.float64, device=dev)
    step = [ws.data_ptr(), int(need.value), dq.data_ptr(), 3, 10, None, out.data_ptr(), None]
    assert L.mf_cloud_icp_step_dev(*step) == -1                                # a workspace no build has filled
    build = [dt.data_ptr(), 6, 3, 100, 0.1, ws.data_ptr(), int(need.value), None]
    assert L.mf_cloud_icp_build_dev(*build) == 0
    assert L.mf_cloud_icp_step_dev(*step) == 0
    for k, v in ((1, 2), (2, 1), (2, 4), (3, (1 << 30) + 1), (0, None), (5, None), (5, ws.data_ptr() + 4), (6, 1024)):
        bad = list(build)
        bad[k] = v
        assert L.mf_cloud_icp_build_dev(*bad) == -1, k
    assert L.mf_cloud_icp_build_dev(*build) == 0                               # (the failed builds above cleared or kept it; build again)
    for k, v in ((0, None), (0, ws.data_ptr() + 4), (1, int(need.value) - 1), (2, None), (3, 2), (4, (1 << 30) + 1), (4, 100), (6, None)):
        bad = list(step)
        bad[k] = v
        assert L.mf_cloud_icp_step_dev(*bad) == -1, k
    assert L.mf_cloud_icp_step_dev(*step) == 0


def test_nearest_is_untouched_by_a_registration(hip):
    from maskfusion_amd import eval as ev
    from maskfusion_amd.lib import torch_device
    import torch
    ref, nrm, _, est, T = _case(60_000, 40_000, 8)
    dev = torch_device()
    dref, dest = torch.from_numpy(ref).to(dev), torch.from_numpy(est).to(dev)
    before = ev.nearest(dref, dest, 0.05, T=T)
    res = ev.register(dest, dref, 0.10, ref_normals=nrm, max_iterations=3)
    assert res["iterations"] == 3
    after = ev.nearest(dref, dest, 0.05, T=T)
    assert before[0].tobytes() == after[0].tobytes() and before[1].tobytes() == after[1].tobytes()
    assert dref.cpu().numpy().tobytes() == ref.tobytes() and dest.cpu().numpy().tobytes() == est.tobytes()


# ---------------- end to end ----------------
def _eval_command(args):
    if EMU:    # the child drives the same CPU-executed build as this process
        cmd = [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import eval as e; "
               "sys.exit(e.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"))] + args
    else:
        cmd = [sys.executable, "-m", "maskfusion_amd.eval"] + args
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)


def _write_ply(path, xyz, nrm=None):
    with open(path, "wb") as f:
        props = "property float x\nproperty float y\nproperty float z\n" + ("property float nx\nproperty float ny\nproperty float nz\n" if nrm is not None else "")
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\n%send_header\n" % (len(xyz), props)).encode())
        rows = xyz if nrm is None else np.concatenate([xyz, nrm], 1)
        f.write(np.ascontiguousarray(rows, "<f4").tobytes())


def test_eval_command_with_register_end_to_end(hip, tmp_path):
    from maskfusion_amd import MaskFusion
    from maskfusion_amd import eval as ev
    st = _stream()
    m = MaskFusion(W, H, F, F, W / 2.0, H / 2.0, icpThresh=100.0, so3=False, numGSurfels=1 << 18, enableMultipleModels=False,
                   initConfidenceGlobal=1.0)
    for k in range(12):
        rgb, depth, _ = st.frame(k)
        m.processFrame(rgb, depth, timestamp=33333 * (k + 1))
    est = tmp_path / "est"
    est.mkdir()
    m.exportPoses(str(est) + os.sep)
    m.savePly(str(est) + os.sep)
    m.close()
    pts, nrm = ev.read_ply(str(est / "cloud-0.ply"), normals=True)
    assert nrm is not None and len(pts) > 5000 and np.abs(np.linalg.norm(nrm, axis=1) - 1).max() < 1e-3
    # the reference: the exported cloud moved by a known rigid motion (the view of the room's corner holds three non-parallel faces)
    M = _pose([1.5, -2.0, 1.0], [0.02, -0.015, 0.03])
    moved = _moved(pts, M)
    mn = (nrm.astype(np.float64) @ M[:3, :3].T).astype(np.float32)
    _write_ply(str(tmp_path / "model.ply"), moved, mn)
    ref = tmp_path / "ref"
    ref.mkdir()
    _write_ply(str(ref / "cloud-0.ply"), moved, mn)
    base = ["--est", str(est), "--ref", str(ref), "--radius", "0.05", "--tau", "0.01,0.02,0.05"]
    # without --register: what the command printed before the flag existed -- exactly compare_clouds of the two files (the expectation is
    # made here, by the test)
    out = _eval_command(base)
    assert out.returncode == 0, out.stderr
    want = {"model": 0, "ref_model": 0, "cloud": ev.compare_clouds(pts, ev.read_ply(str(ref / "cloud-0.ply")), 0.05, (0.01, 0.02, 0.05))}
    assert out.stdout == json.dumps(ev._clean(want)) + "\n"
    # with: the same `cloud`, the motion recovered, a better score
    out = _eval_command(base + ["--register", "--register-radius", "0.2,0.1,0.05"])
    assert out.returncode == 0, out.stderr
    o = json.loads(out.stdout)
    assert o["cloud"] == json.loads(json.dumps(ev._clean(want["cloud"])))
    reg = o["registration"]
    assert set(reg) == {"T", "rotation_rad", "translation_m", "iterations", "inliers", "inlier_share", "rmse", "converged", "reason", "radius", "method"}
    dt, dr = rr.pose_error(np.array(reg["T"]), M)
    print("registration:", reg["iterations"], "iterations, error", dt, dr, "cloud rmse", o["cloud"]["accuracy"]["rmse"], "->", o["cloud_registered"]["accuracy"]["rmse"])
    assert reg["converged"] and reg["method"] == "plane" and reg["inlier_share"] >= 0.99
    assert dt < 1e-5 and dr < 1e-5                     # the moved copy is an exact image: the gate of the recovery test
    assert abs(reg["rotation_rad"] - rr.pose_error(M, np.eye(4))[1]) < 1e-5 and abs(reg["translation_m"] - np.linalg.norm(M[:3, 3])) < 1e-5
    assert o["cloud_registered"]["accuracy"]["rmse"] < o["cloud"]["accuracy"]["rmse"]
    assert o["cloud_registered"]["accuracy"]["rmse"] < dt + 4.0 * dr + 2e-6 and o["cloud_registered"]["fscore"]["0.01"] == 1.0   # (|x| < 4 m)
    # the same against a single reference file
    single = ["--est", str(est), "--ref-cloud", str(tmp_path / "model.ply")]
    out = _eval_command(single + ["--register", "--register-radius", "0.2,0.1,0.05"])
    assert out.returncode == 0, out.stderr
    o2 = json.loads(out.stdout)
    assert o2["ref_cloud"] == str(tmp_path / "model.ply") and o2["cloud"] == o["cloud"] and o2["registration"] == reg
    # --init: the start is used for `cloud`
    with open(tmp_path / "init.txt", "w") as f:
        f.write("# est -> ref\n" + "\n".join(" ".join("%.17g" % v for v in row) for row in M) + "\n")
    out = _eval_command(single + ["--init", str(tmp_path / "init.txt")])
    assert out.returncode == 0, out.stderr
    assert json.loads(out.stdout)["cloud"]["accuracy"]["rmse"] < 2e-6
    # a reference without normals: a clear error under point-to-plane, a fall-back with --point-to-point
    _write_ply(str(tmp_path / "bare.ply"), moved)
    bare = ["--est", str(est), "--ref-cloud", str(tmp_path / "bare.ply"), "--register", "--register-radius", "0.2,0.1,0.05"]
    out = _eval_command(bare)
    assert out.returncode == 2 and "no normals" in out.stderr and "--point-to-point" in out.stderr and out.stdout == ""
    out = _eval_command(bare + ["--point-to-point"])
    assert out.returncode == 0, out.stderr
    reg = json.loads(out.stdout)["registration"]
    dt, dr = rr.pose_error(np.array(reg["T"]), M)
    print("point-to-point:", reg["iterations"], "iterations, error", dt, dr)
    dt0, dr0 = rr.pose_error(np.eye(4), M)
    assert reg["method"] == "point" and reg["iterations"] >= 1 and dt < dt0 and dr < dr0      # (slow on planes: closer than the start)
