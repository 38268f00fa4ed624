"""Run evaluation, host half (maskfusion_amd/eval.py): TUM parsing and association, Horn alignment, ATE / RPE against closed forms, PLY
reading, and the eval command on trajectories alone.  No GPU needed."""
import json
import os
import struct
import subprocess
import sys

import numpy as np

from maskfusion_amd import eval as ev
from maskfusion_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _quat_xyzw(R):
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(R).as_quat()


def _write_tum(path, ts, T, header="# timestamp tx ty tz qx qy qz qw\n"):
    with open(path, "w") as f:
        f.write(header)
        for t, M in zip(ts, T):
            q = _quat_xyzw(M[:3, :3])
            f.write("%.6f %.9f %.9f %.9f %.9f %.9f %.9f %.9f\n" % (t, *M[:3, 3], *q))


def _random_rigid(rng):
    R = synth.rot_xyz(*rng.uniform(-np.pi, np.pi, 3))
    return synth.make_pose(R, rng.uniform(-2, 2, 3))


def test_read_tum_with_comments(tmp_path):
    p = tmp_path / "gt.txt"
    p.write_text("# ground truth trajectory\n# file: 'x.bag'\n\n1.000000 1 2 3 0 0 0 1\n  # indented comment\n"
                 "1.5,0.5,0,0,0,0,0.7071067811865476,0.7071067811865476  # trailing comment\n")
    ts, T = ev.read_tum(str(p))
    assert ts.tolist() == [1.0, 1.5]
    assert np.allclose(T[0], synth.make_pose(np.eye(3), [1, 2, 3]))
    assert np.allclose(T[1][:3, :3], synth.rot_xyz(0, 0, np.pi / 2), atol=1e-12) and np.allclose(T[1][:3, 3], [0.5, 0, 0])


def test_associate_is_greedy_by_smallest_dt():
    a, b = [0.0, 0.010], [0.008, 0.025]
    # nearest-first in a's order would give (0, 0), (1, 1); TUM's greedy pass takes the smallest |dt| first: (1, 0), after which
    # (0, 0) is blocked and (1, 1) too, and (0, 1) is 0.025 apart
    assert ev.associate(a, b, 0.02).tolist() == [[1, 0]]
    assert ev.associate([0.0, 1.0, 2.0], [2.001, 0.5, 0.999], 0.02).tolist() == [[1, 2], [2, 0]]
    assert ev.associate([], [1.0]).shape == (0, 2)


def test_align_horn_recovers_a_rigid_transform():
    rng = np.random.default_rng(3)
    gt = rng.uniform(-3, 3, (50, 3))
    A = _random_rigid(rng)
    est = (gt - A[:3, 3]) @ A[:3, :3]     # est = A^-1 gt
    T = ev.align_horn(est, gt)
    assert np.abs(T - A).max() < 1e-9


def test_ate_closed_form():
    # gt on the corners of a cube centred at 0 (|g| = sqrt 3); est = a rigid motion of 1.1 g: the optimal alignment undoes the motion and
    # leaves the radial residual 0.1 sqrt 3 at every pose
    g = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], np.float64)
    ts = np.arange(8) * 0.1
    G = np.array([synth.make_pose(np.eye(3), p) for p in g])
    A = _random_rigid(np.random.default_rng(5))
    E = np.array([A @ synth.make_pose(synth.rot_xyz(0.1 * k, 0, 0), 1.1 * p) for k, p in enumerate(g)])
    r = ev.ate((ts, E), (ts + 0.001, G))
    assert r["pairs"] == 8
    for k in ("rmse", "mean", "median", "min", "max"):
        assert abs(r[k] - 0.1 * np.sqrt(3)) < 1e-12, (k, r[k])
    assert r["std"] < 1e-12


def test_rpe_closed_forms():
    ts = np.round(np.arange(31) * 0.1, 6)
    # translation drift: gt moves 1 m/s along x, est 1.1 m/s -> 0.1 m per 1 s for every pair, no rotation
    G = np.array([synth.make_pose(np.eye(3), [t, 0, 0]) for t in ts])
    E = np.array([synth.make_pose(np.eye(3), [1.1 * t, 0, 0]) for t in ts])
    r = ev.rpe((ts, E), (ts, G), delta=1.0, unit="s")
    assert r["pairs"] == 20            # i = 0 .. 19; from i = 20 on the partner is the last pose (skipped, as upstream)
    assert abs(r["trans_rmse"] - 0.1) < 1e-9 and abs(r["trans_mean"] - 0.1) < 1e-9 and r["rot_mean_deg"] < 1e-6
    # rotation drift: est yaws at 0.2 rad/s in place, gt stands still -> 0.2 rad per 10 frames
    G = np.array([np.eye(4) for _ in ts])
    E = np.array([synth.make_pose(synth.rot_xyz(0, 0, 0.2 * t), [0, 0, 0]) for t in ts])
    r = ev.rpe((ts, E), (ts, G), delta=10, unit="f")
    assert r["pairs"] == 20
    assert r["trans_rmse"] < 1e-12 and abs(r["rot_mean_deg"] - np.degrees(0.2)) < 1e-9


def _ply_binary(path, xyz, rgb, nrm, rad):
    """the layout of mf_save_ply (tests/test_gpu_api.py::test_pose_log_exports_and_ply)"""
    with open(path, "wb") as f:
        f.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\nproperty float y\nproperty float z"
                 "\nproperty uchar red\nproperty uchar green\nproperty uchar blue\nproperty float nx\nproperty float ny"
                 "\nproperty float nz\nproperty float radius\nend_header\n" % len(xyz)).encode())
        for p, c, n, r in zip(xyz, rgb, nrm, rad):
            f.write(struct.pack("<3f3B4f", *p, *c, *n, r))


def test_read_ply_binary_and_ascii(tmp_path):
    rng = np.random.default_rng(7)
    xyz = rng.normal(size=(257, 3)).astype(np.float32)
    _ply_binary(str(tmp_path / "a.ply"), xyz, rng.integers(0, 256, (257, 3)), rng.normal(size=(257, 3)), rng.uniform(0, 1, 257))
    got = ev.read_ply(str(tmp_path / "a.ply"))
    assert got.dtype == np.float32 and got.tobytes() == xyz.tobytes()
    with open(tmp_path / "b.ply", "w") as f:
        f.write("ply\nformat ascii 1.0\ncomment made by hand\nelement vertex 3\nproperty float nx\nproperty float x\nproperty float y\n"
                "property float z\nelement face 1\nproperty list uchar int vertex_indices\nend_header\n"
                "9 1.5 2 3\n9 -1 0.25 0\n9 0 0 -7.125\n3 0 1 2\n")
    assert ev.read_ply(str(tmp_path / "b.ply")).tolist() == [[1.5, 2, 3], [-1, 0.25, 0], [0, 0, -7.125]]
    _ply_binary(str(tmp_path / "c.ply"), np.zeros((0, 3), np.float32), [], [], [])
    assert ev.read_ply(str(tmp_path / "c.ply")).shape == (0, 3)


def test_eval_command_with_gt_only(tmp_path):
    st = synth.Stream()
    ts = np.round((np.arange(40) + 1) * 0.033333, 6)
    G = np.array([st.gt_pose(k) for k in range(40)])
    rng = np.random.default_rng(11)
    E = G.copy()
    E[:, :3, 3] += rng.normal(scale=0.01, size=(40, 3))
    est = tmp_path / "est"
    est.mkdir()
    _write_tum(str(est / "poses-0.txt"), ts, E, header="")
    _write_tum(str(tmp_path / "gt.txt"), ts, G)
    out = subprocess.run([sys.executable, "-m", "maskfusion_amd.eval", "--est", str(est), "--gt", str(tmp_path / "gt.txt"), "--rpe-delta", "0.5"],
                         cwd=ROOT, capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    lines = out.stdout.strip().split("\n")
    assert len(lines) == 1
    o = json.loads(lines[0])
    assert o["model"] == 0
    a = o["trajectory_vs_gt"]["ate"]
    assert a["pairs"] == 40
    assert a["rmse"] <= synth.ate_rmse(E, G) + 1e-9
    ref = ev.ate(ev.read_tum(str(est / "poses-0.txt")), ev.read_tum(str(tmp_path / "gt.txt")))
    assert abs(a["rmse"] - ref["rmse"]) < 1e-12
    r = o["trajectory_vs_gt"]["rpe"]
    assert r["pairs"] > 20 and 0 < r["trans_rmse"] < 0.05


def test_rpe_is_the_tum_scripts_error():
    # one pair (0, 1): est turns by 90 degrees about z and moves 1 m along x, gt only moves 1 m along x.  evaluate_rpe.py's error
    # (est_0^-1 est_1)(gt_0^-1 gt_1)^-1 = [Rz, (1, 0, 0) - Rz (1, 0, 0)] has |t| = sqrt 2; the paper's (gt_0^-1 gt_1)^-1 (est_0^-1 est_1) would give 0
    ts = np.array([0.0, 1.0, 2.0])
    E = np.array([np.eye(4), synth.make_pose(synth.rot_xyz(0, 0, np.pi / 2), [1, 0, 0]), synth.make_pose(np.eye(3), [2, 0, 0])])
    G = np.array([synth.make_pose(np.eye(3), [x, 0, 0]) for x in (0.0, 1.0, 2.0)])
    r = ev.rpe((ts, E), (ts, G), delta=1.0, unit="s")
    assert r["pairs"] == 1
    assert abs(r["trans_rmse"] - np.sqrt(2)) < 1e-12 and abs(r["rot_mean_deg"] - 90.0) < 1e-9
    # partners are looked up among est's own stamps; a gt pose more than twice the median gt interval away drops the pair
    ts_e = np.array([0.0, 0.5, 1.0, 1.5, 2.0, 2.5])
    E = np.array([synth.make_pose(np.eye(3), [1.1 * t, 0, 0]) for t in ts_e])
    ts_g = np.array([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 1.5, 1.6, 1.7, 1.8, 1.9, 2.0, 2.1, 2.2, 2.3, 2.4, 2.5])   # nothing near t = 1.0
    G = np.array([synth.make_pose(np.eye(3), [t, 0, 0]) for t in ts_g])
    r = ev.rpe((ts_e, E), (ts_g, G), delta=1.0, unit="s")
    # i -> j: 0 -> 1.0 (gt gap: dropped), 0.5 -> 1.5, 1.0 -> 2.0 (dropped), 1.5 -> 2.5 (last pose: skipped), later ones: last
    assert r["pairs"] == 1 and abs(r["trans_rmse"] - 0.1) < 1e-12
