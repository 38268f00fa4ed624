"""A brute-force numpy restatement of the FPFH descriptors and the descriptor matcher (DESIGN.md "Global registration",
include/maskfusion_amd.h mf_cloud_fpfh_dev / mf_feature_match_dev): every pair of points through the library's fp32 radius test bit for bit,
the pair features and the weighted sums in fp64, the outputs rounded to fp32 as the device stores them.  O(n^2) in time and memory: for the
few thousand points of the tests.

Next to the counts it returns, for every point, the smallest margin of its pairs: how far a pair's decisions are from going the other way --
the distance of each feature to the nearest bin border (in bins), ||a1| - |a2|| (the swap) and |v| / L (the pair that is not counted).  A
point is GATED when all its pairs, and all pairs of its neighbours, have every margin above 1e-9: fp64 rounding (1e-15) and the last bits of
atan2 cannot change a count there.
"""
from __future__ import annotations

import numpy as np

import normals_restatement as nr

BINS, DIM = 11, 33
GATE = 1e-9


def _eligible(points, normals):
    p = np.ascontiguousarray(points[:, :3], np.float32)
    n = np.ascontiguousarray(normals[:, :3], np.float32).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        length = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        ok = np.isfinite(p).all(1) & np.isfinite(n).all(1) & (length > 0)
        unit = n / length[:, None]
    unit[~ok] = 0.0
    p = p.copy()
    p[~ok] = np.nan
    return p, unit, ok


def _bin(t):
    return np.clip(np.floor(t), 0, BINS - 1).astype(np.int64)


def _border(t):
    """distance of t (in bins) to the nearest border 1 .. 10 (below 0 and above 11 the bin is clamped: no border there)"""
    return np.abs(t - np.clip(np.round(t), 1, BINS - 1))


def pair_features(d, ni, nj):
    """the header's steps 1 - 5 on arrays of pairs (fp64): (counted, b1, b2, b3, margin)"""
    with np.errstate(invalid="ignore", divide="ignore"):
        dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
        L2 = (dx * dx + dy * dy) + dz * dz
        L = np.sqrt(L2)
        a1 = ((ni[..., 0] * dx + ni[..., 1] * dy) + ni[..., 2] * dz) / L
        a2 = ((nj[..., 0] * dx + nj[..., 1] * dy) + nj[..., 2] * dz) / L
        swap = np.abs(a1) < np.abs(a2)
        s3 = swap[..., None]
        n1, n2 = np.where(s3, nj, ni), np.where(s3, ni, nj)
        dd = np.where(s3, -d, d)
        f3 = np.where(swap, -a2, a1)
        dx, dy, dz = dd[..., 0], dd[..., 1], dd[..., 2]
        vx = dy * n1[..., 2] - dz * n1[..., 1]
        vy = dz * n1[..., 0] - dx * n1[..., 2]
        vz = dx * n1[..., 1] - dy * n1[..., 0]
        vl2 = (vx * vx + vy * vy) + vz * vz
        vl = np.sqrt(vl2)
        vx, vy, vz = vx / vl, vy / vl, vz / vl
        wx = n1[..., 1] * vz - n1[..., 2] * vy
        wy = n1[..., 2] * vx - n1[..., 0] * vz
        wz = n1[..., 0] * vy - n1[..., 1] * vx
        f2 = (vx * n2[..., 0] + vy * n2[..., 1]) + vz * n2[..., 2]
        f1 = np.arctan2((wx * n2[..., 0] + wy * n2[..., 1]) + wz * n2[..., 2],
                        (n1[..., 0] * n2[..., 0] + n1[..., 1] * n2[..., 1]) + n1[..., 2] * n2[..., 2])
        t1, t2, t3 = 11.0 * (f1 + np.pi) / (2.0 * np.pi), 11.0 * (f2 + 1.0) / 2.0, 11.0 * (f3 + 1.0) / 2.0
        counted = (L2 > 0) & (vl2 > 0)
        margin = np.minimum.reduce([_border(t1), _border(t2), _border(t3), np.abs(np.abs(a1) - np.abs(a2)), vl / L])
        margin = np.where(counted, margin, np.inf)          # (an exact zero of fp64 products of the same operands on either side)
        t1, t2, t3 = (np.where(counted, t, 0.0) for t in (t1, t2, t3))
    return counted, _bin(t1), _bin(t2), _bin(t3), margin, L2


def fpfh(points, normals, radius, chunk=250):
    """{"spfh" int32 (n, 34): 33 counts and k; "fpfh" float32 (n, 33); "fpfh64" the same before the rounding; "eligible" bool (n,);
    "margin" float64 (n,): the smallest margin over the point's pairs; "gated" bool (n,); "neighbours" int (n,)}"""
    p32, unit, ok = _eligible(points, normals)
    p = p32.astype(np.float64)
    n = len(p)
    spfh = np.zeros((n, DIM + 1), np.int32)
    margin = np.full(n, np.inf)
    M = np.zeros((n, n), bool)
    W = []
    for a in range(0, n, chunk):
        rows = np.arange(a, min(n, a + chunk))
        m = nr.neighbour_mask(p32, radius, rows)
        m[np.arange(len(rows)), rows] = False
        M[rows] = m
        with np.errstate(invalid="ignore"):
            d = p[None, :, :] - p[rows, None, :]
        d = np.where(m[:, :, None], d, 0.0)
        counted, b1, b2, b3, mg, L2 = pair_features(d, np.broadcast_to(unit[rows, None, :], d.shape), np.broadcast_to(unit[None, :, :], d.shape))
        counted &= m
        r = np.broadcast_to(np.arange(len(rows))[:, None], counted.shape)[counted]
        for part, b in enumerate((b1, b2, b3)):
            h = np.bincount(r * BINS + b[counted], minlength=len(rows) * BINS).reshape(len(rows), BINS)
            spfh[rows, part * BINS:(part + 1) * BINS] = h
        spfh[rows, DIM] = counted.sum(1)
        margin[rows] = np.where(m, mg, np.inf).min(1, initial=np.inf)
        with np.errstate(divide="ignore"):
            W.append(np.where(m & (L2 > 0), 1.0 / np.where(L2 > 0, L2, 1.0), 0.0))
    k = spfh[:, DIM].astype(np.float64)
    has = k > 0
    S = np.where(has[:, None], spfh[:, :DIM] / np.maximum(k, 1.0)[:, None], 0.0)
    acc = np.concatenate([w @ S for w in W]) if n else np.zeros((0, DIM))
    out = np.full((n, DIM), np.nan)
    parts = acc.reshape(n, 3, BINS).sum(2)
    good = ok & (parts > 0).all(1)
    with np.errstate(invalid="ignore", divide="ignore"):
        out[good] = (100.0 * acc[good].reshape(-1, 3, BINS) / parts[good][:, :, None]).reshape(-1, DIM)
    fine = margin > GATE
    gated = ok & fine & ~(M & ~fine[None, :]).any(1)
    return {"spfh": spfh, "fpfh": out.astype(np.float32), "fpfh64": out, "eligible": ok, "margin": margin, "gated": gated, "neighbours": M.sum(1)}


def match(target, query):
    """(idx int32 [nq], d2 float32 [nq]): for every query row the target row with the smallest fp32 d2, summed over the bins in order, every
    operation rounded to fp32 on its own; ties to the smallest index; a row with a NaN is nobody's match; -1 and +inf without a match"""
    t = np.ascontiguousarray(target, np.float32)
    q = np.ascontiguousarray(query, np.float32)
    nt, nq = len(t), len(q)
    if nt == 0 or nq == 0:
        return np.full(nq, -1, np.int32), np.full(nq, np.inf, np.float32)
    d2 = np.zeros((nq, nt), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for b in range(t.shape[1]):
            d = q[:, b, None] - t[None, :, b]
            d2 = d2 + d * d
    d2 = np.where(np.isnan(d2), np.float32(np.inf), d2)
    j = np.argmin(d2, 1)                       # the first of equal minima: the smallest index
    best = d2[np.arange(nq), j]
    return np.where(best < np.inf, j, -1).astype(np.int32), best.astype(np.float32)
