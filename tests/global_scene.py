"""The scene of the global-registration tests (tests/test_gpu_fpfh.py, tests/test_eval_global_host.py): three unequal rectangles that meet in
a corner, an off-centre sphere and a box on the floor -- no symmetry maps it onto itself -- sampled with its analytic normals, and a motion of
120 degrees and 3 m.  Also the restatement-driven stand-ins for the device calls of maskfusion_amd.eval.register_global."""
from __future__ import annotations

import numpy as np

import fpfh_restatement as fr
import normals_restatement as nr
import register_restatement as rr

VOXEL = 0.07


def _rect(rng, n, origin, u, v, normal):
    a = rng.uniform(0, 1, (n, 2))
    return np.asarray(origin, np.float64) + a[:, :1] * np.asarray(u, np.float64) + a[:, 1:] * np.asarray(v, np.float64), np.tile(np.asarray(normal, np.float64), (n, 1))


def scene(n=9000, seed=5):
    """(points float32 (n', 3), unit normals float32): surfaces sampled uniformly by area, n' close to n"""
    rng = np.random.default_rng(seed)
    rects = [((0, 0, 0), (2.0, 0, 0), (0, 1.4, 0), (0, 0, 1)),            # the floor
             ((0, 0, 0), (0, 1.4, 0), (0, 0, 1.0), (1, 0, 0)),            # two walls of unequal height
             ((0, 0, 0), (2.0, 0, 0), (0, 0, 0.7), (0, 1, 0)),
             ((0.3, 0.5, 0.3), (0.4, 0, 0), (0, 0.3, 0), (0, 0, 1)),      # the box: top and four sides
             ((0.3, 0.5, 0), (0.4, 0, 0), (0, 0, 0.3), (0, -1, 0)),
             ((0.3, 0.8, 0), (0.4, 0, 0), (0, 0, 0.3), (0, 1, 0)),
             ((0.3, 0.5, 0), (0, 0.3, 0), (0, 0, 0.3), (-1, 0, 0)),
             ((0.7, 0.5, 0), (0, 0.3, 0), (0, 0, 0.3), (1, 0, 0))]
    centre, R = np.array([1.35, 0.85, 0.40]), 0.25
    areas = [np.linalg.norm(np.cross(u, v)) for _, u, v, _ in rects] + [4 * np.pi * R * R]
    counts = np.round(n * np.array(areas) / sum(areas)).astype(int)
    P, N = [], []
    for (o, u, v, nm), c in zip(rects, counts):
        p, q = _rect(rng, c, o, u, v, nm)
        P.append(p)
        N.append(q)
    d = rng.normal(size=(counts[-1], 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    P.append(centre + R * d)
    N.append(d)
    return np.concatenate(P).astype(np.float32), np.concatenate(N).astype(np.float32)


def motion():
    """est -> ref: 120 degrees about (1, 2, 3) and 3 m"""
    from scipy.spatial.transform import Rotation
    axis = np.array([1.0, 2.0, 3.0]) / np.sqrt(14.0)
    T = np.eye(4)
    T[:3, :3] = Rotation.from_rotvec(np.deg2rad(120.0) * axis).as_matrix()
    T[:3, 3] = np.array([2.0, -1.0, 2.0])
    return T


def moved(pts, T):
    return (np.asarray(pts, np.float64) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)


def exact_pair(n=9000):
    """ref with normals, est = ref's exact image under motion()^-1 with its normals, and motion()"""
    ref, rn = scene(n)
    T = motion()
    Ti = np.linalg.inv(T)
    return moved(ref, Ti), (rn.astype(np.float64) @ Ti[:3, :3].T).astype(np.float32), ref, rn, T


def noisy_pair(n=4500, sigma=1e-3, seed=6):
    """two different samples of the scene with `sigma` of noise; est keeps the 70 % of its points with the smallest x + y: the clouds
    overlap in part.  Normals are left to the pipeline."""
    ref, _ = scene(n, seed=seed)
    est, _ = scene(n, seed=seed + 1)
    rng = np.random.default_rng(seed + 2)
    ref = (ref + rng.normal(scale=sigma, size=ref.shape)).astype(np.float32)
    est = (est + rng.normal(scale=sigma, size=est.shape)).astype(np.float32)
    s = est[:, 0] + est[:, 1]
    est = est[s <= np.quantile(s, 0.7)]
    T = motion()
    return moved(est, np.linalg.inv(T)), ref, T


# ---- the device calls of register_global, restated ----
def normals_stand_in(points, radius, min_neighbours=5, viewpoint=None):
    r = nr.estimate(np.asarray(points, np.float32), radius, min_neighbours, viewpoint)
    return r["normal"], r["variation"], r["count"]


_fpfh_memo = {}


def fpfh_stand_in(points, normals, radius):
    """(the O(n^2) restatement, kept per input: a test calls the pipeline on one cloud several times)"""
    p, n = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(normals, np.float32)
    key = (p.tobytes(), n.tobytes(), float(radius))
    if key not in _fpfh_memo:
        r = fr.fpfh(p, n, radius)
        _fpfh_memo[key] = (r["fpfh"], r["spfh"])
    return _fpfh_memo[key]


def match_stand_in(target, query):
    return fr.match(target, query)


class RegistrationStandIn:
    """eval.Registration on the restatement: the same system from the same correspondences"""

    def __init__(self, ref, radius, normals=None, n_query=0):
        self.ref, self.radius, self.normals = np.asarray(ref, np.float32), float(radius), normals

    def step(self, q, T=None):
        usable = None if self.normals is None else np.isfinite(np.asarray(self.normals)).all(1)
        s, _, _, _ = rr.step_system(self.ref, self.normals, np.asarray(q, np.float32), self.radius, np.eye(4) if T is None else np.asarray(T, np.float64),
                                    usable)
        return s


def patch(monkeypatch, ev):
    monkeypatch.setattr(ev, "estimate_normals", normals_stand_in)
    monkeypatch.setattr(ev, "fpfh", fpfh_stand_in)
    monkeypatch.setattr(ev, "match_features", match_stand_in)
    monkeypatch.setattr(ev, "Registration", RegistrationStandIn)
    monkeypatch.setattr(ev, "_device_points", lambda a: np.asarray(a, np.float32))
