"""The host side of the cloud registration (maskfusion_amd.eval): PLY normals, the 6 x 6 solve and the SE(3) update against numpy and
SciPy, register()'s stop rules and result keys on a scripted device, the command's flags.  No GPU."""
import json
import math

import numpy as np
import pytest

from maskfusion_amd import eval as ev


def _ply(path, xyz, nrm=None, ascii_=False, extra=True):
    names = ["x", "y", "z"] + (["red"] if extra else []) + (["nx", "ny", "nz"] if nrm is not None else [])
    with open(path, "wb") as f:
        head = "ply\nformat %s 1.0\nelement vertex %d\n" % ("ascii" if ascii_ else "binary_little_endian", len(xyz))
        head += "".join("property %s %s\n" % ("uchar" if n == "red" else "float", n) for n in names) + "end_header\n"
        f.write(head.encode())
        for k in range(len(xyz)):
            row = list(xyz[k]) + ([7] if extra else []) + (list(nrm[k]) if nrm is not None else [])
            if ascii_:
                f.write((" ".join(repr(float(v)) if names[i] != "red" else "7" for i, v in enumerate(row)) + "\n").encode())
            else:
                for i, v in enumerate(row):
                    f.write(np.array(v, "u1" if names[i] == "red" else "<f4").tobytes())


@pytest.mark.parametrize("ascii_", [False, True])
def test_read_ply_with_normals(tmp_path, ascii_):
    rng = np.random.default_rng(0)
    xyz, nrm = rng.normal(size=(50, 3)).astype(np.float32), rng.normal(size=(50, 3)).astype(np.float32)
    p = str(tmp_path / "a.ply")
    _ply(p, xyz, nrm, ascii_)
    got = ev.read_ply(p)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and np.array_equal(got, xyz)      # the default return value is unchanged
    gx, gn = ev.read_ply(p, normals=True)
    assert np.array_equal(gx, xyz) and np.array_equal(gn, nrm) and gn.dtype == np.float32
    _ply(p, xyz, None, ascii_)
    gx, gn = ev.read_ply(p, normals=True)
    assert np.array_equal(gx, xyz) and gn is None
    # without normals: a clear error under point-to-plane (before any device work)
    with pytest.raises(ValueError, match="point-to-plane registration needs the reference's normals"):
        ev.register(xyz, gx, 0.1, ref_normals=gn)
    with pytest.raises(ValueError, match="method"):
        ev.register(xyz, gx, 0.1, method="icp")


def _pack(A, b, res, n):
    out = []
    for i in range(6):
        for j in range(i, 7):
            out.append(b[i] if j == 6 else A[i, j])
    return np.array(out + [res, n], np.float64)


def test_solve_and_update_against_numpy_and_scipy():
    from scipy.spatial.transform import Rotation
    rng = np.random.default_rng(1)
    for scale in (1e-9, 1e-4, 1e-2, 0.4, 2.0):
        J = rng.normal(size=(40, 6))
        A = J.T @ J * rng.uniform(1.0, 1e4)
        x_true = np.concatenate([rng.normal(size=3) * 0.01, scale * np.array([0.6, -0.64, 0.48])])
        s = _pack(A, -A @ x_true, 1.0, 40)
        A2, b2, res, n = ev.unpack_sys29(s)
        assert np.array_equal(A2, A2.T) and np.allclose(A2, A, rtol=0, atol=0) and res == 1.0 and n == 40
        x, why = ev.solve_step(s)
        assert why is None
        xn = np.linalg.solve(A, -b2)
        assert np.abs(x - xn).max() <= 50 * np.linalg.cond(A) * 2.2e-16 * np.abs(xn).max()
        T0 = np.eye(4)
        T0[:3, :3] = Rotation.from_rotvec([0.2, -0.1, 0.05]).as_matrix()
        T0[:3, 3] = [0.3, -0.2, 1.1]
        U = np.eye(4)
        U[:3, :3] = Rotation.from_rotvec(x[3:]).as_matrix()
        U[:3, 3] = x[:3]
        got = ev.update_se3(T0, x)
        assert np.abs(got - U @ T0).max() < 1e-14
        assert abs(ev.rotation_angle(U[:3, :3]) - np.linalg.norm(x[3:])) < 1e-14 * max(1.0, 1.0 / max(scale, 1e-9)) + 1e-15
    assert np.array_equal(ev.rodrigues([0, 0, 0]), np.eye(3))


def test_solve_refuses_systems_outside_its_domain():
    rng = np.random.default_rng(2)
    J = rng.normal(size=(40, 6))
    A = J.T @ J
    x, why = ev.solve_step(_pack(A, A @ np.ones(6), 1.0, 5))
    assert x is None and "fewer than 6" in why
    Jp = J.copy()
    Jp[:, 4] = Jp[:, 1] * 2.0                                      # rank 5
    x, why = ev.solve_step(_pack(Jp.T @ Jp, np.ones(6), 1.0, 40))
    assert x is None and "rank deficient" in why
    M = rng.normal(size=(6, 6))                                    # a pivot ratio of 1e-10: outside; 1e-6: inside
    Q, _ = np.linalg.qr(M)
    for small, inside in ((1e-10, False), (1e-6, True)):
        Ai = Q @ np.diag([1.0, 0.5, 0.3, 0.2, 0.1, small]) @ Q.T
        x, why = ev.solve_step(_pack((Ai + Ai.T) / 2, np.ones(6), 1.0, 40))
        assert (x is not None) == inside, (small, why)
    x, why = ev.solve_step(_pack(np.zeros((6, 6)), np.zeros(6), 0.0, 40))
    assert x is None and "rank deficient" in why


class _Scripted:
    """stands in for eval.Registration: a quadratic bowl around x_goal whose step halves (rate) the distance"""
    made = []

    def __init__(self, ref, radius, normals=None, n_query=0):
        self.radius = radius
        _Scripted.made.append(radius)

    def step(self, q, T=None):
        t = np.asarray(T)[:3, 3]
        x = np.concatenate([(_Scripted.goal - t) * _Scripted.rate, np.zeros(3)])
        A = np.eye(6) * 10.0
        return _pack(A, -A @ x, float(np.sum((_Scripted.goal - t) ** 2)) * len(q), len(q) if _Scripted.hits is None else _Scripted.hits)


def test_register_stop_rules_and_keys(monkeypatch):
    monkeypatch.setattr(ev, "Registration", _Scripted)
    monkeypatch.setattr(ev, "_device_points", lambda a: np.asarray(a, np.float32))
    _Scripted.goal, _Scripted.rate, _Scripted.hits, _Scripted.made = np.array([0.1, 0.0, -0.2]), 0.5, None, []
    est = np.zeros((100, 3), np.float32)
    res = ev.register(est, est, 0.05, method="point", trace=True)
    assert set(res) == {"T", "iterations", "inliers", "inlier_share", "rmse", "converged", "reason", "radius", "method", "trace"}
    # steps halve from 0.112: below 1e-6 after 18 iterations
    assert res["converged"] and res["reason"] is None and res["iterations"] == 18 and len(res["trace"]) == 18
    assert np.linalg.norm(res["T"][:3, 3] - _Scripted.goal) < 2e-6 and res["inliers"] == 100 and res["inlier_share"] == 1.0
    assert set(res["trace"][0]) == {"radius", "T", "sys29", "x", "inliers", "rmse"} and np.array_equal(res["trace"][0]["T"], np.eye(4))
    # looser tolerances stop earlier; the cap stops without convergence and says so
    assert ev.register(est, est, 0.05, method="point", tol_translation=1e-3)["iterations"] == 8
    res = ev.register(est, est, 0.05, method="point", max_iterations=5)
    assert not res["converged"] and res["iterations"] == 5 and "within 5 iterations" in res["reason"] and res["trace"] == []
    # a rotation step above its tolerance keeps the loop going even when the translation is small
    res = ev.register(est, est, 0.05, method="point", tol_translation=1.0, tol_rotation=0.0, max_iterations=4)
    assert not res["converged"] and res["iterations"] == 4
    # the schedule: one grid per radius, in order; only the last radius decides convergence
    _Scripted.made = []
    res = ev.register(est, est, 0.05, method="point", schedule=[0.2, 0.1, 0.05], T0=np.eye(4))
    assert _Scripted.made == [0.2, 0.1, 0.05] and res["converged"] and res["radius"] == 0.05
    # too few correspondences: no update, a reason
    _Scripted.hits = 3
    res = ev.register(est, est, 0.05, method="point", T0=None)
    assert not res["converged"] and "fewer than 6" in res["reason"] and res["iterations"] == 0 and np.array_equal(res["T"], np.eye(4))
    s = ev.registration_summary(res)
    assert set(s) == {"T", "rotation_rad", "translation_m", "iterations", "inliers", "inlier_share", "rmse", "converged", "reason", "radius", "method"}
    json.dumps(s)
    with pytest.raises(ValueError):
        ev.register(est, est, 0.05, method="point", schedule=[])


def test_init_file_parsing(tmp_path):
    from scipy.spatial.transform import Rotation
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec([0.1, 0.2, -0.3]).as_matrix()
    T[:3, 3] = [1, 2, 3]
    p = tmp_path / "T.txt"
    p.write_text("# est -> ref\n" + "\n".join(", ".join("%.17g" % v for v in r) for r in T) + "\n")
    assert np.array_equal(ev.read_transform(str(p)), T)
    p.write_text(" ".join("%.17g" % v for v in T.reshape(16)))
    assert np.array_equal(ev.read_transform(str(p)), T)
    for bad, what in (("1 2 3", "16 numbers"), (" ".join(["1"] * 16), "last row"), (" ".join("%g" % v for v in (2 * np.eye(4) - np.diag([0, 0, 0, 1])).reshape(16)), "rotation"),
                      (" ".join(["nan"] * 16), "finite")):
        p.write_text(bad)
        with pytest.raises(ValueError, match=what):
            ev.read_transform(str(p))


def test_command_flag_errors(tmp_path, capsys):
    est = tmp_path / "est"
    est.mkdir()
    for args in (["--est", str(est), "--init", "x.txt", "--gt", "g.txt"], ["--est", str(est), "--ref", "a", "--ref-cloud", "b.ply"],
                 ["--est", str(est), "--register"], ["--est", str(est), "--ref", "a", "--point-to-point"],
                 ["--est", str(est), "--ref", "a", "--register-radius", "0.1"], ["--est", str(est), "--ref", "a", "--register", "--register-radius", "0.1,x"],
                 ["--est", str(est), "--ref", "a", "--register", "--register-radius", "0.1,-1"],
                 ["--est", str(est), "--ref", "a", "--register", "--register-iterations", "0"], ["--est", str(est)]):
        with pytest.raises(SystemExit) as e:
            ev.main(args)
        assert e.value.code == 2, args
    capsys.readouterr()
    # --ref-cloud without a background cloud, and an --init that is not a transform: exit code 2 with a message, before any device work
    assert ev.main(["--est", str(est), "--ref-cloud", "model.ply"]) == 2
    assert "cloud-0.ply" in capsys.readouterr().err
    _ply(str(est / "cloud-0.ply"), np.zeros((3, 3), np.float32), extra=False)
    (tmp_path / "bad.txt").write_text("1 0 0")
    assert ev.main(["--est", str(est), "--ref-cloud", "model.ply", "--init", str(tmp_path / "bad.txt")]) == 2
    assert "16 numbers" in capsys.readouterr().err
    assert math.isclose(ev.rotation_angle(np.eye(3)), 0.0)
