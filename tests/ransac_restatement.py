"""mf_pose_ransac_dev restated in numpy fp64, operation by operation from include/maskfusion_amd.h: status, fit and score of every triple,
the winner, its mask and its pose.  Every numpy operation below is one IEEE operation per element (no matmul, no einsum, no sum over an
axis: those may contract or reorder), so the results are the header's bits."""
from __future__ import annotations

import numpy as np


def _len3(d):
    return np.sqrt((d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2])


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def _frame(p):
    """p (K, 3, 3): the triple's points -> rows e1, e2, e3 (K, 3, 3) and |w|"""
    a, b = p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    w = _cross(a, b)
    la, lw = _len3(a), _len3(w)
    with np.errstate(invalid="ignore", divide="ignore"):
        e1, e3 = a / la[:, None], w / lw[:, None]
    return np.stack([e1, _cross(e3, e1), e3], 1), lw


def status_and_fit(src, dst, tri, edge_tolerance):
    """src, dst (m, 3) float32; tri (h, 3) integers -> status uint8 (h,), pose fp64 (h, 3, 4): rows R_r0 R_r1 R_r2 t_r, NaN where not tested"""
    s64, d64 = np.asarray(src, np.float32).astype(np.float64), np.asarray(dst, np.float32).astype(np.float64)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    m, h = len(s64), len(tri)
    status = np.zeros(h, np.uint8)
    pose = np.full((h, 3, 4), np.nan)
    bad = ((tri < 0) | (tri >= m)).any(1) | (tri[:, 0] == tri[:, 1]) | (tri[:, 0] == tri[:, 2]) | (tri[:, 1] == tri[:, 2])
    status[bad] = 1
    ok = np.flatnonzero(~bad)
    if ok.size == 0:
        return status, pose
    s, d = s64[tri[ok]], d64[tri[ok]]                                   # (K, 3, 3)
    fin = np.isfinite(s).all((1, 2)) & np.isfinite(d).all((1, 2))
    keep = 1.0 - float(edge_tolerance)
    edges = np.ones(len(ok), bool)
    with np.errstate(invalid="ignore", over="ignore"):
        for a, b in ((0, 1), (0, 2), (1, 2)):
            ls, ld = _len3(s[:, b] - s[:, a]), _len3(d[:, b] - d[:, a])
            lo, hi = np.where(ls < ld, ls, ld), np.where(ls < ld, ld, ls)
            edges &= (lo > 0.0) & (lo >= keep * hi)
        E, lws = _frame(s)
        F, lwd = _frame(d)
    degenerate = (lws == 0.0) | (lwd == 0.0)
    st = np.where(~fin, 3, np.where(~edges, 2, np.where(degenerate, 3, 0))).astype(np.uint8)
    status[ok] = st
    t = st == 0
    E, F, s, d = E[t], F[t], s[t], d[t]
    R = np.empty((t.sum(), 3, 3))
    for r in range(3):
        for c in range(3):
            R[:, r, c] = (F[:, 0, r] * E[:, 0, c] + F[:, 1, r] * E[:, 1, c]) + F[:, 2, r] * E[:, 2, c]
    cs, cd = ((s[:, 0] + s[:, 1]) + s[:, 2]) / 3.0, ((d[:, 0] + d[:, 1]) + d[:, 2]) / 3.0
    P = np.empty((t.sum(), 3, 4))
    P[:, :, :3] = R
    for r in range(3):
        P[:, r, 3] = cd[:, r] - ((R[:, r, 0] * cs[:, 0] + R[:, r, 1] * cs[:, 1]) + R[:, r, 2] * cs[:, 2])
    pose[ok[t]] = P
    return status, pose


def inliers(pose, src, dst, inlier_distance):
    """pose (K, 3, 4) -> bool (K, m)"""
    s64, d64 = np.asarray(src, np.float32).astype(np.float64), np.asarray(dst, np.float32).astype(np.float64)
    thr2 = float(inlier_distance) * float(inlier_distance)
    P = np.asarray(pose, np.float64).reshape(-1, 3, 4)[:, :, :, None]   # (K, 3, 4, 1)
    x, y, z = s64[None, :, 0], s64[None, :, 1], s64[None, :, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        e2 = None
        for r in range(3):
            dr = (((P[:, r, 0] * x + P[:, r, 1] * y) + P[:, r, 2] * z) + P[:, r, 3]) - d64[None, :, r]
            e2 = dr * dr if e2 is None else e2 + dr * dr                 # (dx*dx + dy*dy) + dz*dz
        return e2 <= thr2


def search(src, dst, tri, inlier_distance, edge_tolerance, chunk=256):
    """the call's outputs: {"status" uint8 (h,), "counts" uint32 (h,), "best" int32 (2,), "inlier" uint8 (m,), "pose" fp64 (12,) or None,
    "poses" (h, 3, 4)}"""
    src, dst = np.asarray(src, np.float32).reshape(-1, 3), np.asarray(dst, np.float32).reshape(-1, 3)
    tri = np.asarray(tri, np.int64).reshape(-1, 3)
    status, poses = status_and_fit(src, dst, tri, edge_tolerance)
    counts = np.zeros(len(tri), np.uint32)
    t = np.flatnonzero(status == 0)
    for a in range(0, len(t), chunk):
        counts[t[a:a + chunk]] = inliers(poses[t[a:a + chunk]], src, dst, inlier_distance).sum(1)
    return pick({"status": status, "counts": counts, "poses": poses}, src, dst, inlier_distance)


def pick(res, src, dst, inlier_distance, h=None):
    """the winner, its mask and pose over the first h triples of a search (all of them by default): a triple's status and count do not depend
    on the others"""
    h = len(res["status"]) if h is None else h
    status, counts, poses = res["status"][:h], res["counts"][:h], res["poses"][:h]
    t = np.flatnonzero(status == 0)
    out = {"status": status, "counts": counts, "poses": poses, "best": np.array([-1, 0], np.int32), "inlier": np.zeros(len(src), np.uint8), "pose": None}
    if t.size:
        j = int(t[np.argmax(counts[t])])                               # the first of equal counts
        out["best"] = np.array([j, counts[j]], np.int32)
        out["inlier"] = inliers(poses[j], src, dst, inlier_distance)[0].astype(np.uint8)
        out["pose"] = poses[j].reshape(12).copy()
    return out


def device_stand_in(src, dst, tri, inlier_distance, edge_tolerance):
    """what maskfusion_amd.eval._pose_ransac_device returns, from the restatement: (status, counts, best, inlier mask bool, pose 3 x 4 or None)"""
    r = search(src, dst, tri, inlier_distance, edge_tolerance)
    return r["status"], r["counts"], r["best"], r["inlier"].astype(bool), None if r["pose"] is None else r["pose"].reshape(3, 4)
