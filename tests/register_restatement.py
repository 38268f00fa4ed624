"""A from-scratch numpy / scipy restatement of the cloud registration (DESIGN.md "Cloud registration", include/maskfusion_amd.h
mf_cloud_icp_step_dev, maskfusion_amd.eval.register): correspondences by scipy.spatial.cKDTree re-ranked with the library's fp32 rule, the
Gauss-Newton system in fp64 from the fp32 x', numpy's solve and SciPy's rotation for the update.  Sums are taken in extended precision and
come with the sum of the terms' magnitudes, from which the tests derive their bound.
"""
from __future__ import annotations

import numpy as np

U64 = 2.0 ** -53     # unit roundoff of fp64


def transform_f32(T, p):
    """the library's query transform in fp32: x' = ((T00 x + T01 y) + T02 z) + T03"""
    T = np.asarray(T, np.float32)
    x, y, z = (np.ascontiguousarray(p[:, k], np.float32) for k in range(3))
    return np.stack([T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3)], 1)


def correspondences(ref, xq, radius, usable=None, k=8):
    """For every x' the index of its partner in ref, -1 for none, by the library's rule: fp32 d2 = (dx*dx + dy*dy) + dz*dz, kept when
    d2 <= fl(r*r), the smallest d2 and then the smallest index.  cKDTree (fp64) proposes the k nearest within a slightly larger radius and
    the fp32 rule ranks them.  usable: mask of the targets that take part (finite position and normal)."""
    from scipy.spatial import cKDTree
    ref = np.ascontiguousarray(ref[:, :3], np.float32)
    ok = np.isfinite(ref).all(1)
    if usable is not None:
        ok &= usable
    ids = np.flatnonzero(ok)
    out = np.full(len(xq), -1, np.int64)
    fin = np.isfinite(xq).all(1)
    if len(ids) == 0 or not fin.any():
        return out
    tree = cKDTree(ref[ids].astype(np.float64))
    k = min(k, len(ids))
    _, nb = tree.query(xq[fin].astype(np.float64), k=k, distance_upper_bound=float(radius) * (1.0 + 1e-5))
    nb = nb.reshape(-1, k)
    miss = nb >= len(ids)
    cand = ids[np.where(miss, 0, nb)]
    q = xq[fin][:, None, :]
    p = ref[cand]
    d = q - p
    d2 = d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]
    r2 = np.float32(radius) * np.float32(radius)
    d2 = np.where(miss | ~(d2 <= r2), np.float32(np.inf), d2)
    best = d2.min(1)
    cj = np.where(d2 == best[:, None], cand, np.iinfo(np.int64).max).min(1)
    out[np.flatnonzero(fin)] = np.where(np.isfinite(best), cj, -1)
    return out


def rows(xq, p, n=None):
    """(J [m, 6], r [m]) in fp64: point-to-plane (n given) r = n . (x' - p), J = [n, x' x n]; point-to-point the three rows of
    [I, -[x']x] per pair, r = x' - p (pair-major: 3 m rows)"""
    X = np.asarray(xq, np.float64)
    P = np.asarray(p, np.float64)
    d = X - P
    if n is not None:
        N = np.asarray(n, np.float64)
        r = (N[:, 0] * d[:, 0] + N[:, 1] * d[:, 1]) + N[:, 2] * d[:, 2]
        c = np.stack([X[:, 1] * N[:, 2] - X[:, 2] * N[:, 1], X[:, 2] * N[:, 0] - X[:, 0] * N[:, 2], X[:, 0] * N[:, 1] - X[:, 1] * N[:, 0]], 1)
        return np.concatenate([N, c], 1), r
    m = len(X)
    J = np.zeros((m, 3, 6))
    J[:, 0, 0] = J[:, 1, 1] = J[:, 2, 2] = 1.0
    J[:, 0, 4], J[:, 0, 5] = X[:, 2], -X[:, 1]
    J[:, 1, 3], J[:, 1, 5] = -X[:, 2], X[:, 0]
    J[:, 2, 3], J[:, 2, 4] = X[:, 1], -X[:, 0]
    return J.reshape(3 * m, 6), d.reshape(3 * m)


def system(xq, p, n=None):
    """(sys29, abs29, terms): the packed system (for i: JtJ[i][i..5], Jtr[i]; sum r^2; pairs), the sum of |term| of every entry and the number
    of terms of a sum.  Each product is one fp64 multiplication, as on the device; the sums are taken in extended precision."""
    J, r = rows(xq, p, n)
    s, a = np.zeros(29), np.zeros(29)
    k = 0

    def put(t):
        nonlocal k
        s[k] = float(t.sum(dtype=np.longdouble))
        a[k] = float(np.abs(t).sum(dtype=np.longdouble))
        k += 1
    for i in range(6):
        for j in range(i, 6):
            put(J[:, i] * J[:, j])
        put(J[:, i] * r)
    put(r * r)
    s[28] = a[28] = float(len(xq))
    return s, a, len(r)


def bound(abs29, terms):
    """|device - restatement| per entry: terms * 2^-53 * sum |term| bounds a sum of fp64 terms in any order to first order; times 4 for the
    depth of the reduction tree, the products' own rounding against the extended sum and this side's final rounding.  The pair count is exact."""
    b = 4.0 * terms * U64 * np.asarray(abs29)
    b[28] = 0.0
    return b


def step_system(ref, normals, est, radius, T, usable=None):
    """one step for the transform T: (sys29, abs29, terms, idx)"""
    xq = transform_f32(T, est)
    idx = correspondences(ref, xq, radius, usable)
    hit = idx >= 0
    s, a, terms = system(xq[hit], ref[idx[hit], :3], None if normals is None else normals[idx[hit]])
    return s, a, terms, idx


def unpack(sys29):
    A, b, k = np.zeros((6, 6)), np.zeros(6), 0
    for i in range(6):
        for j in range(i, 7):
            if j == 6:
                b[i] = sys29[k]
            else:
                A[i, j] = A[j, i] = sys29[k]
            k += 1
    return A, b


def solve(sys29):
    """x = (t, w) with JtJ x = -Jtr (numpy's LU solve)"""
    A, b = unpack(sys29)
    return np.linalg.solve(A, -b)


def update(T, x):
    """T <- [exp(w) | t] T"""
    from scipy.spatial.transform import Rotation
    U = np.eye(4)
    U[:3, :3] = Rotation.from_rotvec(x[3:]).as_matrix()
    U[:3, 3] = x[:3]
    return U @ T


def register(est, ref, normals, radius, T0=None, max_iterations=50, tol_t=1e-6, tol_r=1e-6):
    """the loop on this side alone: (T, iterations, converged, inlier share at the returned T)"""
    T = np.eye(4) if T0 is None else np.array(T0, np.float64)
    converged, it = False, 0
    for it in range(1, max_iterations + 1):
        s, _, _, _ = step_system(ref, normals, est, radius, T)
        if s[28] < 6:
            break
        x = solve(s)
        T = update(T, x)
        if np.linalg.norm(x[:3]) < tol_t and np.linalg.norm(x[3:]) < tol_r:
            converged = True
            break
    idx = correspondences(ref, transform_f32(T, est), radius)
    return T, it, converged, float((idx >= 0).mean())


def pose_error(T, T_true):
    """(translation difference in m, rotation difference in rad)"""
    from scipy.spatial.transform import Rotation
    dR = T[:3, :3] @ T_true[:3, :3].T
    return float(np.linalg.norm(T[:3, 3] - T_true[:3, 3])), float(np.linalg.norm(Rotation.from_matrix(dR).as_rotvec()))
