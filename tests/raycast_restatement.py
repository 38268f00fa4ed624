"""The numpy restatement of mf_trimesh_raycast_dev / mf_trimesh_render_dev (include/maskfusion_amd.h): a brute force of the watertight
ray-triangle test over (rays x eligible triangles) in fp64 with every operation rounded on its own -- numpy evaluates one ufunc at a time, so
nothing is contracted --, the two transforms in fp32, the pinhole rays, a long-double Moeller-Trumbore to hold it against, and the
fixtures tests/test_raycast_host.py and tests/test_gpu_raycast.py share.  Not a test module."""
import numpy as np

import trimesh_restatement as tr


def transform_rays(T, origins, dirs):
    """the header's fp32 transforms: o' = ((T00 x + T01 y) + T02 z) + T03, d' = (T00 x + T01 y) + T02 z"""
    T = np.asarray(T, np.float32)
    o, d = np.asarray(origins, np.float32), np.asarray(dirs, np.float32)
    with np.errstate(all="ignore"):
        o2 = np.stack([T[r, 0] * o[:, 0] + T[r, 1] * o[:, 1] + T[r, 2] * o[:, 2] + T[r, 3] for r in range(3)], 1)
        d2 = np.stack([T[r, 0] * d[:, 0] + T[r, 1] * d[:, 1] + T[r, 2] * d[:, 2] for r in range(3)], 1)
    return o2, d2


def pinhole_rays(W, H, fx, fy, cx, cy):
    """(origins, dirs) of mf_trimesh_render_dev's camera-frame rays in pixel order: (((float)x - cx) (1 / fx), ((float)y - cy) (1 / fy), 1)"""
    fx, fy, cx, cy = (np.float32(v) for v in (fx, fy, cx, cy))
    y, x = np.meshgrid(np.arange(H, dtype=np.float32), np.arange(W, dtype=np.float32), indexing="ij")
    d = np.stack([(x - cx) * (np.float32(1) / fx), (y - cy) * (np.float32(1) / fy), np.ones_like(x)], -1).reshape(-1, 3).astype(np.float32)
    return np.zeros_like(d), d


def axes(d):
    """(kx, ky, kz, negative) per ray: kz the first axis with the largest |d|; kx, ky follow it and swap when d[kz] < 0"""
    kz = np.argmax(np.abs(d), 1)
    kx = (kz + 1) % 3
    ky = (kx + 1) % 3
    neg = np.take_along_axis(d, kz[:, None], 1)[:, 0] < 0
    return np.where(neg, ky, kx), np.where(neg, kx, ky), kz, neg


def _pick(a, k):
    return np.take_along_axis(a, k.reshape((-1,) + (1,) * (a.ndim - 1)), a.ndim - 1)[..., 0]


def raycast(V, F, origins, dirs, T=None, tmin=0.0, tmax=np.inf, chunk=128):
    """The definition: dict with t (float32, +inf: none), tri (int32), uv (float32 (n, 2)), front (bool), t64 / uv64 (the fp64 values),
    kz, neg (the axis choice) and valid"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    o, d = np.asarray(origins, np.float32)[:, :3], np.asarray(dirs, np.float32)[:, :3]
    if T is not None:
        o, d = transform_rays(T, o, d)
    n = len(o)
    valid = np.isfinite(o).all(1) & np.isfinite(d).all(1) & (d != 0).any(1)
    idx = np.flatnonzero(tr.eligible(V, F))
    out = dict(t=np.full(n, np.inf, np.float32), tri=np.full(n, -1, np.int32), uv=np.full((n, 2), np.nan, np.float32), front=np.zeros(n, bool),
               t64=np.full(n, np.inf), uv64=np.full((n, 2), np.nan), kz=np.full(n, -1), neg=np.zeros(n, bool), valid=valid)
    if not len(idx) or not valid.any():
        return out
    Vd = np.asarray(V, np.float32).astype(np.float64)
    tri = [Vd[F[idx, k], :3] for k in range(3)]
    lo, hi = np.float64(np.float32(tmin)), np.float64(np.float32(tmax))
    rows_all = np.flatnonzero(valid)
    for s in range(0, len(rows_all), chunk):
        rows = rows_all[s:s + chunk]
        oc, dc = o[rows].astype(np.float64), d[rows].astype(np.float64)
        kx, ky, kz, neg = axes(dc)
        out["kz"][rows], out["neg"][rows] = kz, neg
        dz = _pick(dc, kz)
        Sx, Sy, Sz = _pick(dc, kx) / dz, _pick(dc, ky) / dz, 1.0 / dz
        P = []
        for v in tri:
            p = v[None, :, :] - oc[:, None, :]                                     # P' = P - o
            pz = np.take_along_axis(p, kz[:, None, None], 2)[..., 0]
            px = np.take_along_axis(p, kx[:, None, None], 2)[..., 0] - Sx[:, None] * pz
            py = np.take_along_axis(p, ky[:, None, None], 2)[..., 0] - Sy[:, None] * pz
            P.append((px, py, Sz[:, None] * pz))
        (Ax, Ay, Az), (Bx, By, Bz), (Cx, Cy, Cz) = P
        U, Vv, W = Cx * By - Cy * Bx, Ax * Cy - Ay * Cx, Bx * Ay - By * Ax
        miss = ((U < 0) | (Vv < 0) | (W < 0)) & ((U > 0) | (Vv > 0) | (W > 0))
        det = (U + Vv) + W
        miss |= det == 0
        with np.errstate(all="ignore"):
            t = ((U * Az + Vv * Bz) + W * Cz) / det
            count = ~miss & (t >= lo) & (t <= hi)
            key = np.where(count, t, np.inf)
            k = np.argmin(key, 1)                                                  # the first minimum: the smallest triangle index
            r = np.arange(len(rows))
            k = np.where(count[r, k], k, np.argmax(count, 1))                      # (a counting t of +inf: the first counting triangle)
            hit = count[r, k]
            u64, v64 = (Vv / det)[r, k], (W / det)[r, k]
        g = rows[hit]
        out["t64"][g] = t[r, k][hit]
        out["t"][g] = t[r, k][hit].astype(np.float32)
        out["tri"][g] = idx[k][hit]
        out["uv64"][g] = np.stack([u64, v64], 1)[hit]
        out["uv"][g] = np.stack([u64, v64], 1)[hit].astype(np.float32)
        out["front"][g] = (det[r, k] > 0)[hit]
    return out


def render(V, F, W, H, fx, fy, cx, cy, mesh_from_cam, tmin=0.0, tmax=np.inf):
    """mf_trimesh_render_dev: (depth (H, W) float32 with 0 for a miss, and raycast()'s dict)"""
    o, d = pinhole_rays(W, H, fx, fy, cx, cy)
    res = raycast(V, F, o, d, mesh_from_cam, tmin, tmax)
    return np.where(res["tri"] >= 0, res["t"], np.float32(0)).reshape(H, W), res


def moller_trumbore(V, F, origins, dirs):
    """Moeller-Trumbore with inclusive edges over all (ray, triangle) pairs in long double: (t (n, T), barycentric weights (n, T, 3) of
    a, b, c, hit (n, T))"""
    L = np.longdouble
    Vd = np.asarray(V, np.float32).astype(L)
    a, b, c = (Vd[F[:, k], :3][None] for k in range(3))
    o, d = np.asarray(origins, np.float32).astype(L)[:, None, :], np.asarray(dirs, np.float32).astype(L)[:, None, :]
    e1, e2 = b - a, c - a
    p = np.cross(d, e2)
    det = (e1 * p).sum(-1)
    with np.errstate(all="ignore"):
        s = o - a
        u = (s * p).sum(-1) / det
        q = np.cross(s, e1)
        v = (d * q).sum(-1) / det
        t = (e2 * q).sum(-1) / det
    hit = (det != 0) & (u >= 0) & (v >= 0) & (u + v <= 1)
    return t, np.stack([1 - u - v, u, v], -1), hit


# ---------------- fixtures ----------------
def edges(F):
    return np.unique(np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1), axis=0)


def with_duplicates(F, seed, n=20):
    """F and n of its triangles appended once more: a copy never wins, the original having the smaller index"""
    return np.concatenate([F, F[np.random.default_rng(seed).choice(len(F), n, replace=False)]]).astype(np.int32)


def _unit(x):
    return x / np.linalg.norm(x, axis=-1, keepdims=True)


BAD_RAYS = (np.array([[0.3, -0.2, 0.1]] * 5 + [[np.nan, 0.0, 0.0]], np.float32),
            np.array([[0, 0, 0], [np.nan, 1, 0], [0, np.inf, 0], [1, 0, -np.inf], [-0.0, 0.0, -0.0], [0, 0, 1]], np.float32))


def sphere_rays(V, F, seed=41):
    """(origins, dirs, expect, groups): expect 1 a hit, 0 a miss; groups: name -> slice.  The icosphere of trimesh_restatement (centre
    SPHERE_C, its vertices at SPHERE_R): from inside at every vertex and every edge's fp32 midpoint, from the origin with the vertex as the
    direction, random from inside, from outside with unit directions (first hit at t in 0.9 .. 1.2, second beyond 1.7), along every axis in
    both senses, grazing past the silhouette, and rays that are not valid"""
    rng = np.random.default_rng(seed)
    C, R = tr.SPHERE_C, tr.SPHERE_R
    E = edges(F)
    mids = ((V[E[:, 0]] + V[E[:, 1]]) * np.float32(0.5)).astype(np.float32)
    parts, names = [], []

    def add(name, o, d, expect):
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        parts.append((np.broadcast_to(o, d.shape).copy(), d, np.full(len(d), expect)))
        names.append(name)
    o = (C + rng.uniform(-0.1, 0.1, (len(V), 3))).astype(np.float32)
    add("vertices", o, V - o, 1)
    o = (C + rng.uniform(-0.1, 0.1, (len(mids), 3))).astype(np.float32)
    add("midpoints", o, mids - o, 1)
    add("origin0", np.zeros(3), V, 1)
    add("inside", C + rng.uniform(-0.2, 0.2, (520, 3)), _unit(rng.normal(size=(520, 3))), 1)
    o = C + 1.5 * _unit(rng.normal(size=(400, 3)))
    target = C + 0.25 * rng.uniform(-1, 1, (400, 1)) * _unit(rng.normal(size=(400, 3)))
    add("outside", o, _unit(target - o), 1)
    for k in range(3):
        for sgn in (1.0, -1.0):
            off = rng.uniform(-0.25, 0.25, (20, 3))
            off[:, k] = -2.0 * sgn
            d = np.zeros((20, 3))
            d[:, k] = sgn * rng.uniform(0.5, 2.0, 20)
            add("axis%d%s" % (k, "+" if sgn > 0 else "-"), C + off, d, 1)
    w = _unit(rng.normal(size=(150, 3)))
    tau = _unit(np.cross(w, rng.normal(size=(150, 3))))
    p = C + R * rng.uniform(1.002, 1.3, (150, 1)) * w                              # the closest approach to the centre: outside the sphere
    add("grazing", p - 1.5 * tau, tau, 0)
    add("bad", BAD_RAYS[0], BAD_RAYS[1], 0)
    groups, at = {}, 0
    for name, (o, d, e) in zip(names, parts):
        groups[name] = slice(at, at + len(d))
        at += len(d)
    return (np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts]), np.concatenate([x[2] for x in parts]), groups)


def mixed_rays(V, F, R, c2, seed=42):
    """the same for trimesh_restatement.mixed_mesh: the quad (triangles 0, 1: wide at small cells), patch 1 on it, patch 2 around c2"""
    rng = np.random.default_rng(seed)
    n1 = 441
    parts, names = [], []

    def add(name, o, d, expect):
        o, d = np.asarray(o, np.float32), np.asarray(d, np.float32)
        parts.append((o, d, np.full(len(d), expect)))
        names.append(name)

    def off(n, h):                                                                  # offsets in the quad's frame: h along its normal
        return np.concatenate([rng.uniform(-0.3, 0.3, (n, 2)), np.full((n, 1), h)], 1) @ R.T
    for name, base, h, n in (("patch1_above", 4, 1.0, 300), ("patch1_below", 4, -1.0, 200)):
        v = V[base + rng.integers(0, n1, n)]
        o = (v + off(n, h)).astype(np.float32)
        add(name, o, v - o, 1)
    v = V[4 + n1 + rng.integers(0, n1, 300)]
    o = (v + np.concatenate([rng.uniform(-0.3, 0.3, (300, 2)), rng.choice([-1.0, 1.0], (300, 1))], 1)).astype(np.float32)
    add("patch2", o, v - o, 1)
    E, shared = np.unique(np.sort(np.concatenate([F[802:][:, [0, 1]], F[802:][:, [1, 2]], F[802:][:, [2, 0]]]), 1), axis=0, return_counts=True)
    E = E[shared == 2][::5][:200]                                                   # inner edges: past a border's rounded midpoint lies nothing
    mids = ((V[E[:, 0]] + V[E[:, 1]]) * np.float32(0.5)).astype(np.float32)
    o = (mids + np.concatenate([rng.uniform(-0.2, 0.2, (len(mids), 2)), np.full((len(mids), 1), 0.7)], 1)).astype(np.float32)
    add("patch2_mid", o, mids - o, 1)
    tq = np.concatenate([rng.uniform(-1.9, 1.9, (400, 2)), np.zeros((400, 1))], 1)
    oq = tq + np.concatenate([rng.uniform(-0.5, 0.5, (400, 2)), rng.choice([-1.0, 1.0], (400, 1)) * rng.uniform(1.0, 2.0, (400, 1))], 1)
    add("quad", oq @ R.T, (tq - oq) @ R.T, 1)
    for k in range(3):
        for sgn in (1.0, -1.0):
            t = (np.concatenate([rng.uniform(-1.2, 1.2, (20, 2)), np.zeros((20, 1))], 1) @ R.T).astype(np.float32)
            d = np.zeros((20, 3), np.float32)
            d[:, k] = sgn
            add("axis%d%s" % (k, "+" if sgn > 0 else "-"), t - d, d * np.float32(rng.uniform(0.5, 2.0)), 1)
    og = np.concatenate([np.full((150, 1), -3.0), rng.uniform(-2, 2, (150, 1)), rng.choice([-0.5, 0.5], (150, 1))], 1)
    dg = np.concatenate([np.ones((150, 1)), rng.uniform(-0.2, 0.2, (150, 1)), np.zeros((150, 1))], 1)
    add("grazing", og @ R.T, dg @ R.T, 0)                                          # parallel to the quad, 0.5 off it: past everything
    add("bad", BAD_RAYS[0], BAD_RAYS[1], 0)
    add("random", c2 * 0.5 + rng.uniform(-1, 1, (300, 3)), rng.normal(size=(300, 3)), -1)
    groups, at = {}, 0
    for name, (o, d, e) in zip(names, parts):
        groups[name] = slice(at, at + len(d))
        at += len(d)
    return (np.concatenate([x[0] for x in parts]), np.concatenate([x[1] for x in parts]), np.concatenate([x[2] for x in parts]), groups)


def room(size=(4.0, 3.0, 5.0), centre=(0.0, 0.0, 2.0)):
    """a box room of 12 triangles seen from inside (counter-clockwise from inside): (V float32 (8, 3), F int32 (12, 3))"""
    s, c = np.asarray(size) / 2, np.asarray(centre)
    V = np.array([[x, y, z] for z in (-1, 1) for y in (-1, 1) for x in (-1, 1)], np.float64) * s + c
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    F = []
    for q in quads:
        F += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    V, F = V.astype(np.float32), np.array(F, np.int32)
    n = tr.cross_norm2(V, F)[0]                                                      # turn every face towards the centre
    flip = ((c - V[F[:, 0]].astype(np.float64)) * n).sum(1) < 0
    F[flip] = F[flip][:, [0, 2, 1]]
    return V, F
