"""The numpy restatement of mf_trimesh_* (include/maskfusion_amd.h): a brute force of the point-to-triangle distance over (queries x
triangles) in fp64 with every operation rounded on its own -- numpy evaluates one ufunc at a time, so nothing is contracted --, the sampler,
and the fixtures tests/test_trimesh_host.py and tests/test_gpu_trimesh.py share.  Not a test module."""
import numpy as np

R2_A, R2_B = 0.7548776662466927, 0.5698402909980532


def _dot(u, v):
    return (u[..., 0] * v[..., 0] + u[..., 1] * v[..., 1]) + u[..., 2] * v[..., 2]


def cross_norm2(V, F):
    """(b - a) x (c - a) and its squared norm in fp64 from the fp32 vertices, in the header's order"""
    V = np.asarray(V, np.float32).astype(np.float64)
    a, b, c = V[F[:, 0], :3], V[F[:, 1], :3], V[F[:, 2], :3]
    ab, ac = b - a, c - a
    n = np.stack([ab[:, 1] * ac[:, 2] - ab[:, 2] * ac[:, 1], ab[:, 2] * ac[:, 0] - ab[:, 0] * ac[:, 2], ab[:, 0] * ac[:, 1] - ab[:, 1] * ac[:, 0]], 1)
    return n, (n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2]


def eligible(V, F, cell=1.0):
    """one bool per triangle; F may hold indices out of range"""
    V = np.asarray(V, np.float32)
    F = np.asarray(F, np.int64).reshape(-1, 3)
    ok = ((F >= 0) & (F < len(V))).all(1)
    Fc = np.where(ok[:, None], F, 0)
    with np.errstate(all="ignore"):
        co = V[Fc][:, :, :3].astype(np.float64)                        # (T, 3, 3)
        ok &= np.isfinite(co).all((1, 2)) & (np.abs(co * (1.0 / np.float64(np.float32(cell)))) < 2.0 ** 30).all((1, 2))
        ok &= cross_norm2(np.nan_to_num(V), Fc)[1] > 0
    return ok


def closest_points(V, F, P):
    """Ericson 5.1.5 in the book's order for every (query, triangle): (closest (Q, T, 3), D2 (Q, T), region (Q, T) in 0..6)"""
    V = np.asarray(V, np.float32).astype(np.float64)
    a, b, c = (V[F[:, k], :3][None] for k in range(3))
    p = np.asarray(P, np.float32).astype(np.float64)[:, None, :]
    with np.errstate(all="ignore"):
        ab, ac, ap = b - a, c - a, p - a
        d1, d2 = _dot(ab, ap), _dot(ac, ap)
        bp = p - b
        d3, d4 = _dot(ab, bp), _dot(ac, bp)
        vc = d1 * d4 - d3 * d2
        cp = p - c
        d5, d6 = _dot(ab, cp), _dot(ac, cp)
        vb = d5 * d2 - d1 * d6
        va = d3 * d6 - d5 * d4
        e43, e56 = d4 - d3, d5 - d6
        conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
                 (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (e43 >= 0) & (e56 >= 0)]
        v_ab = (d1 / (d1 - d3))[..., None]
        w_ac = (d2 / (d2 - d6))[..., None]
        w_bc = (e43 / (e43 + e56))[..., None]
        den = 1.0 / ((va + vb) + vc)
        v, w = (vb * den)[..., None], (vc * den)[..., None]
        shape = np.broadcast(a, p).shape
        choices = [np.broadcast_to(a, shape), np.broadcast_to(b, shape), a + v_ab * ab, np.broadcast_to(c, shape), a + w_ac * ac, b + w_bc * (c - b)]
        face = (a + ab * v) + ac * w
        region = np.select(conds, list(range(6)), 6)
        q = np.select([k[..., None] for k in conds], choices, face)
        e = p - q
        D2 = (e[..., 0] * e[..., 0] + e[..., 1] * e[..., 1]) + e[..., 2] * e[..., 2]
    return q, D2, region


def distance(V, F, P, radius, chunk=256):
    """The definition of mf_trimesh_distance_dev: dict with dist (float32), tri (int32), closest (float32 (Q, 3)), D2 (fp64, inf: none),
    second (the runner-up's D2), region (the winner's Ericson branch, -1: none)"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    P = np.asarray(P, np.float32)
    ok = eligible(V, F)
    idx = np.flatnonzero(ok)
    r2 = np.float64(np.float32(radius)) * np.float64(np.float32(radius))
    nq = len(P)
    out = dict(dist=np.full(nq, np.inf, np.float32), tri=np.full(nq, -1, np.int32), closest=np.full((nq, 3), np.nan, np.float32),
               D2=np.full(nq, np.inf), second=np.full(nq, np.inf), region=np.full(nq, -1, np.int32))
    if not len(idx) or not nq:
        return out
    Fe = F[idx]
    for s in range(0, nq, chunk):
        q, D2, region = closest_points(V, Fe, P[s:s + chunk])
        with np.errstate(invalid="ignore"):
            D2 = np.where(D2 <= r2, D2, np.inf)
        k = np.argmin(D2, 1)                                   # the first minimum: the smallest triangle index
        rows = np.arange(len(k))
        best = D2[rows, k]
        hit = np.isfinite(best)
        D2s = D2.copy()
        D2s[rows, k] = np.inf
        sl = slice(s, s + len(k))
        out["D2"][sl] = best
        out["second"][sl] = D2s.min(1) if D2.shape[1] > 1 else np.inf
        out["tri"][sl] = np.where(hit, idx[k], -1)
        out["region"][sl] = np.where(hit, region[rows, k], -1)
        out["dist"][sl] = np.where(hit, np.sqrt(np.where(hit, best, 0.0)), np.inf).astype(np.float32)
        out["closest"][sl] = np.where(hit[:, None], q[rows, k], np.nan).astype(np.float32)
    return out


def tie_fraction(res):
    """the share of the queries whose two best triangles have the same fp64 D2"""
    return float(np.mean(np.isfinite(res["D2"]) & (res["D2"] == res["second"])))


def sample_units(V, F, density):
    F = np.asarray(F, np.int64).reshape(-1, 3)
    ok = eligible(V, F)
    n2 = np.zeros(len(F))
    n2[ok] = cross_norm2(V, F[ok])[1]
    u = np.rint(0.5 * np.sqrt(n2) * np.float64(np.float32(density)) * 256.0).astype(np.int64)
    u[~ok] = 0
    return u


def sample(V, F, density):
    """The definition of the sampler: dict with n, points (float32), normals (float32), tri (int32), bary (r1, r2 in fp64), units"""
    F = np.asarray(F, np.int64).reshape(-1, 3)
    u = sample_units(V, F, density)
    S = np.concatenate([[0], np.cumsum(u)])
    assert S[-1] < 2 ** 32
    n = int(S[-1] // 256)
    k = np.arange(n, dtype=np.int64)
    t = np.searchsorted(S, 256 * k + 128, side="right") - 1
    k1 = (k + 1).astype(np.float64)
    r1, r2 = k1 * R2_A, k1 * R2_B
    r1, r2 = r1 - np.floor(r1), r2 - np.floor(r2)
    flip = r1 + r2 > 1.0
    r1, r2 = np.where(flip, 1.0 - r1, r1), np.where(flip, 1.0 - r2, r2)
    Vd = np.asarray(V, np.float32).astype(np.float64)
    a, b, c = Vd[F[t, 0], :3], Vd[F[t, 1], :3], Vd[F[t, 2], :3]
    p = (a + r1[:, None] * (b - a)) + r2[:, None] * (c - a)
    nrm, n2 = cross_norm2(V, F[t]) if n else (np.zeros((0, 3)), np.zeros(0))
    return dict(n=n, points=p.astype(np.float32), normals=(nrm / np.sqrt(n2)[:, None]).astype(np.float32), normals64=nrm / np.sqrt(n2)[:, None],
                tri=t.astype(np.int32), bary=np.stack([r1, r2], 1), units=u, S=S)


# ---------------- fixtures ----------------
SPHERE_C, SPHERE_R = np.array([0.31, -0.22, 0.13]), 0.5


def icosphere(subdivisions=2, centre=SPHERE_C, radius=SPHERE_R):
    """(vertices float32 (10 * 4^s + 2, 3), triangles int32 (20 * 4^s, 3)), counter-clockwise seen from outside"""
    g = (1.0 + np.sqrt(5.0)) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(subdivisions):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    V = (np.asarray(centre) + radius * np.array(v)).astype(np.float32)
    return V, np.array(f, np.int32)


def icosphere_queries(V, F, seed=21):
    """2 000 near the surface, the first 50 vertices, 50 edge midpoints, 20 beyond reach, and three that are not finite"""
    rng = np.random.default_rng(seed)
    d = rng.normal(size=(2000, 3))
    d /= np.linalg.norm(d, axis=1)[:, None]
    near = SPHERE_C + d * (SPHERE_R + rng.uniform(-0.05, 0.05, (2000, 1)))
    e = np.unique(np.sort(np.concatenate([F[:, [0, 1]], F[:, [1, 2]], F[:, [2, 0]]]), 1), axis=0)[::9][:50]
    mids = (V[e[:, 0]] + V[e[:, 1]]) * np.float32(0.5)
    d = rng.normal(size=(20, 3))
    far = SPHERE_C + 0.8 * d / np.linalg.norm(d, axis=1)[:, None]
    bad = np.array([[np.nan, 0.1, 0.1], [0.3, np.inf, 0.1], [0.3, -0.2, -np.inf]])
    return np.concatenate([near, V[:50], mids, far, bad]).astype(np.float32)


def _rot(ax_deg, ay_deg):
    ax, ay = np.radians(ax_deg), np.radians(ay_deg)
    Rx = np.array([[1, 0, 0], [0, np.cos(ax), -np.sin(ax)], [0, np.sin(ax), np.cos(ax)]])
    Ry = np.array([[np.cos(ay), 0, np.sin(ay)], [0, 1, 0], [-np.sin(ay), 0, np.cos(ay)]])
    return Ry @ Rx


def _patch(rng, n=21, step=0.01, bump=0.003):
    """a bumpy n x n-vertex height field around the origin and its 2 (n - 1)^2 triangles"""
    i, j = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    v = np.stack([(i - (n - 1) / 2) * step, (j - (n - 1) / 2) * step, rng.uniform(-bump, bump, (n, n))], -1).reshape(-1, 3)
    q = (i[:-1, :-1] * n + j[:-1, :-1]).reshape(-1)
    f = np.concatenate([np.stack([q, q + n, q + n + 1], 1), np.stack([q, q + n + 1, q + 1], 1)])
    return v, f


def mixed_mesh(seed=22):
    """Two triangles of a 4 m x 4 m quad turned 30 degrees about x and 20 about y (triangles 0 and 1: their boxes are fat), a bumpy patch of
    800 1 cm triangles 3 cm above it, and a second such patch around (-2, -1, -3).  Returns (V float32, F int32, R, patch-2 centre)."""
    rng = np.random.default_rng(seed)
    R = _rot(30.0, 20.0)
    quad = np.array([[-2, -2, 0], [2, -2, 0], [2, 2, 0], [-2, 2, 0]], np.float64)
    p1, f1 = _patch(rng)
    p1 = p1 + np.array([0.4, -0.3, 0.03])
    p2, f2 = _patch(rng)
    c2 = np.array([-2.0, -1.0, -3.0])
    V = np.concatenate([quad @ R.T, p1 @ R.T, p2 + c2]).astype(np.float32)
    F = np.concatenate([[[0, 1, 2], [0, 2, 3]], f1 + 4, f2 + 4 + len(p1)]).astype(np.int32)
    return V, F, R, c2


def mixed_queries(V, F, R, seed=23):
    """2 000: jittered around both patches' vertices, and over the quad up to 10 cm off it"""
    rng = np.random.default_rng(seed)
    n1 = 441
    a = V[4 + rng.integers(0, n1, 700)] + rng.normal(scale=0.02, size=(700, 3))
    b = V[4 + n1 + rng.integers(0, n1, 700)] + rng.normal(scale=0.02, size=(700, 3))
    on = np.concatenate([rng.uniform(-2.1, 2.1, (600, 2)), rng.uniform(-0.1, 0.1, (600, 1))], 1) @ R.T
    return np.concatenate([a, b, on]).astype(np.float32)
