"""A brute-force numpy restatement of the cloud normals (DESIGN.md "Cloud normals", include/maskfusion_amd.h mf_cloud_normals_dev,
maskfusion_amd.eval.estimate_normals): every pair of points through the library's fp32 radius test bit for bit, the moments in fp64,
numpy.linalg.eigh for the decomposition, the header's orientation and no-normal rules, and the outputs rounded to fp32 as the device stores
them.  O(n^2): for the few thousand points of the tests.
"""
from __future__ import annotations

import numpy as np


def neighbour_mask(points, radius, rows):
    """[len(rows), n] bool: j is a neighbour of rows[i] by the library's rule -- both finite, and the fp32 d2 = (dx*dx + dy*dy) + dz*dz of
    d = p_j - p_i (every operation rounded to fp32 on its own) with d2 <= fl(radius * radius)"""
    p = np.ascontiguousarray(points[:, :3], np.float32)
    fin = np.isfinite(p).all(1)
    with np.errstate(invalid="ignore", over="ignore"):
        dx, dy, dz = (p[None, :, k] - p[rows, None, k] for k in range(3))
        d2 = dx * dx + dy * dy + dz * dz
        r2 = np.float32(radius) * np.float32(radius)
        return (d2 <= r2) & fin[None, :] & fin[rows, None]


def estimate(points, radius, min_neighbours=5, viewpoint=None, chunk=500):
    """{"normal" float32 (n, 3), "variation" float32 (n,), "count" int32 (n,), "eig" float64 (n, 3) ascending (NaN where count is 0),
    "normal64", "variation64": the same before the rounding to fp32}"""
    p32 = np.ascontiguousarray(points[:, :3], np.float32)
    p = p32.astype(np.float64)
    n = len(p)
    count = np.zeros(n, np.int32)
    C = np.full((n, 3, 3), np.nan)
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        M = neighbour_mask(p32, radius, rows)
        with np.errstate(invalid="ignore"):
            D = np.where(M[:, :, None], p[None, :, :] - p[rows, None, :], 0.0)
        k = M.sum(1)
        count[rows] = k
        has = k > 0
        kk = np.maximum(k, 1).astype(np.float64)
        m = D.sum(1) / kk[:, None]
        S = np.einsum("ija,ijb->iab", D, D) / kk[:, None, None]
        Cc = S - m[:, :, None] * m[:, None, :]
        C[rows[has]] = Cc[has]
    has = count > 0
    eig = np.full((n, 3), np.nan)
    vec = np.full((n, 3), np.nan)
    if has.any():
        w, V = np.linalg.eigh(C[has])
        eig[has] = w
        vec[has] = V[:, :, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        ok = has & (count >= min_neighbours) & ~(eig[:, 1] <= 1e-12 * eig[:, 2])
        nrm = vec / np.linalg.norm(vec, axis=1)[:, None]
        # the sign: the component of largest magnitude positive, ties to the lowest axis (argmax takes the first) ...
        lead = np.take_along_axis(nrm, np.argmax(np.abs(nrm), 1)[:, None], 1)[:, 0]
        flip = lead < 0
        if viewpoint is not None:          # ... unless a viewpoint decides
            v = np.asarray(viewpoint, np.float32).astype(np.float64)
            t = v[None, :] - p
            dot = (nrm[:, 0] * t[:, 0] + nrm[:, 1] * t[:, 1]) + nrm[:, 2] * t[:, 2]
            flip = np.where(dot != 0, dot < 0, flip)
        nrm = np.where(flip[:, None], -nrm, nrm)
        var = eig[:, 0] / ((eig[:, 0] + eig[:, 1]) + eig[:, 2])
    nrm[~ok] = np.nan
    var[~ok] = np.nan
    return {"normal": nrm.astype(np.float32), "variation": var.astype(np.float32), "count": count, "eig": eig, "normal64": nrm, "variation64": var}


def gated(res, share=0.05):
    """the points whose normal is well defined: a normal exists and the gap l1 - l0 is at least `share` of l2"""
    e = res["eig"]
    with np.errstate(invalid="ignore"):
        return np.isfinite(res["normal64"]).all(1) & (e[:, 1] - e[:, 0] >= share * e[:, 2])


def angle(a, b):
    """angle in radians between the rows of a and b (atan2 of cross and dot in fp64: exact 0 for equal rows)"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.arctan2(np.linalg.norm(np.cross(a, b), axis=1), (a * b).sum(1))
