"""mf_cloud_merge_dev restated in numpy fp32, operation by operation from include/maskfusion_amd.h: the transform, the eligibility rules, a
brute-force partner search over all targets, and a Python loop for the merges of a target in ascending source index (reverse=True: in
descending index, which the tests use to show that the order is under test).  The colour code is the oracle's (color_encoding.glsl, roundf half
away from zero)."""
from __future__ import annotations

import numpy as np

F = np.float32


def _colour():
    from oracle import mfo
    return mfo.lib()


def transform(source, T=None):
    """the records as the merge sees them: x' = ((T00 x + T01 y) + T02 z) + T03, n' = (T00 nx + T01 ny) + T02 nz, the rest as it is"""
    s = np.array(source, np.float32).reshape(-1, 12)
    if T is None:
        return s
    T = np.asarray(T, np.float32)
    x, y, z = s[:, 0].copy(), s[:, 1].copy(), s[:, 2].copy()
    nx, ny, nz = s[:, 8].copy(), s[:, 9].copy(), s[:, 10].copy()
    with np.errstate(all="ignore"):
        for r in range(3):
            s[:, r] = ((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3]
            s[:, 8 + r] = (T[r, 0] * nx + T[r, 1] * ny) + T[r, 2] * nz
    return s


def eligible_sources(st):
    return (np.isfinite(st[:, :3]).all(1) & np.isfinite(st[:, 8:11]).all(1) & np.isfinite(st[:, 3]) & (st[:, 3] > 0) & np.isfinite(st[:, 11]) &
            (st[:, 11] > 0))


def eligible_targets(t):
    return np.isfinite(t[:, :3]).all(1) & np.isfinite(t[:, 8:11]).all(1)


def partners(target, st, radius, min_cos, chunk=512):
    """d_match: for every transformed source the eligible target with the smallest d2 among those that pass the radius and the normal test
    (ties: the smallest index), -1 without one, -2 for a dropped source"""
    t = np.asarray(target, np.float32).reshape(-1, 12)
    r2 = F(radius) * F(radius)
    mc = F(min_cos)
    ok_s, ok_t = eligible_sources(st), eligible_targets(t)
    match = np.where(ok_s, -1, -2).astype(np.int32)
    if len(t) == 0:
        return match
    with np.errstate(all="ignore"):
        for b in range(0, len(st), chunk):
            s = st[b:b + chunk]
            dx, dy, dz = (s[:, None, k] - t[None, :, k] for k in range(3))
            d2 = dx * dx + dy * dy + dz * dz
            dot = (s[:, None, 8] * t[None, :, 8] + s[:, None, 9] * t[None, :, 9]) + s[:, None, 10] * t[None, :, 10]
            cand = (d2 <= r2) & (dot >= mc) & ok_t[None, :]
            d2 = np.where(cand, d2, F(np.inf))
            j = d2.argmin(1)                                   # the first of equal minima: the smallest index
            has = cand[np.arange(len(s)), j] & ok_s[b:b + chunk]
            match[b:b + chunk][has] = j[has]
    return match


def merge_one(q, s, L=None):
    """update.vert:64-93 on one target record q (changed in place) and one transformed source record s; True: the averaging branch"""
    L = L or _colour()
    with np.errstate(all="ignore"):
        c, a = F(q[3]), F(s[3])
        w = c + a
        avg = bool(F(s[11]) < F(1.5) * F(q[11]))
        if avg:
            for k in range(3):
                q[k] = ((c * F(q[k])) + (a * F(s[k]))) / w
            ok, nk = np.zeros(3, np.float32), np.zeros(3, np.float32)
            L.mfo_decode_color(float(q[4]), ok)
            L.mfo_decode_color(float(s[4]), nk)
            ch = [((c * F(ok[k])) + (a * F(nk[k]))) / w for k in range(3)]
            q[4] = F(L.mfo_encode_color(float(ch[0]), float(ch[1]), float(ch[2])))
            n = [((c * F(q[8 + k])) + (a * F(s[8 + k]))) / w for k in range(4)]
            inv = F(1.0) / np.sqrt((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2])
            q[8], q[9], q[10], q[11] = n[0] * inv, n[1] * inv, n[2] * inv, n[3]
        q[3] = w
        q[7] = s[7] if F(s[7]) > F(q[7]) else q[7]
    return avg


def merge(target, source, T=None, radius=0.01, min_cos=0.0, reverse=False):
    """-> (records (n_out, 12) float32, match int32 (n_source,), stats [averaged, confidence-only, appended, dropped])"""
    t = np.array(target, np.float32).reshape(-1, 12)
    st = transform(source, T)
    match = partners(t, st, radius, min_cos)
    L = _colour()
    out = t.copy()
    averaged = conf_only = 0
    order = np.argsort(match, kind="stable")                   # sources by partner, ascending source index inside a partner
    order = order[match[order] >= 0]
    if reverse:
        order = order[::-1]
    for i in order:
        if merge_one(out[match[i]], st[i], L):
            averaged += 1
        else:
            conf_only += 1
    app = st[match == -1]
    stats = [averaged, conf_only, len(app), int(np.count_nonzero(match == -2))]
    return np.concatenate([out, app]).astype(np.float32), match, stats


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
