"""A dense-lattice brute force in numpy of the surfel meshing (include/maskfusion_amd.h mf_cloud_mesh_build_dev, DESIGN.md "Surfel meshing"):
every lattice corner against every point through the library's fp32 radius test in its operation order, everything else in fp64.  No grid,
no blocks, no scans: what the device result is compared with (tests/test_gpu_mesh.py), and the source of the fixtures both suites share."""
import numpy as np


def eligible(points, normals):
    p, n = np.asarray(points, np.float32), np.asarray(normals, np.float32)
    with np.errstate(invalid="ignore"):
        return np.isfinite(p).all(1) & np.isfinite(n).all(1) & (n != 0).any(1)


def corner_positions(origin, voxel, dims):
    """per axis: xf = (float)((double)origin + (double)i * (double)voxel)"""
    o = np.asarray(origin, np.float32).astype(np.float64)
    return [(o[a] + np.arange(dims[a], dtype=np.float64) * np.float64(np.float32(voxel))).astype(np.float32) for a in range(3)]


def field(points, normals, colors, origin, voxel, dims, support, min_neighbours=3):
    """the corners of the dense lattice: count, valid, f, a (.., 3), c (.., 3 or None), indexed [i, j, k]"""
    ok = eligible(points, normals)
    p = np.asarray(points, np.float32)[ok]
    n = np.asarray(normals, np.float32)[ok].astype(np.float64)
    n /= np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])[:, None]
    col = None if colors is None else np.asarray(colors, np.float32)[ok].astype(np.float64)
    dims = [int(d) for d in dims]
    xs, ys, zs = corner_positions(origin, voxel, dims)
    s32 = np.float32(support)
    r2 = s32 * s32
    inv_s2 = 1.0 / (np.float64(s32) * np.float64(s32))
    count = np.zeros(dims, np.int64)
    W = np.zeros(dims)
    F = np.zeros(dims)
    A = np.zeros(dims + [3])
    Cc = None if col is None else np.zeros(dims + [3])
    X, Y = np.meshgrid(xs, ys, indexing="ij")
    X, Y = X.reshape(-1, 1), Y.reshape(-1, 1)
    for k, z in enumerate(zs):
        near = np.abs(p[:, 2].astype(np.float64) - np.float64(z)) <= 1.001 * np.float64(s32)      # (a superset of what can pass the test)
        q, qn = p[near], n[near]
        if not len(q):
            continue
        fx, fy, fz = q[None, :, 0] - X, q[None, :, 1] - Y, q[None, :, 2] - z                       # fp32, d = p - x
        d2 = fx * fx + fy * fy + fz * fz
        hit = d2 <= r2
        dx, dy, dz = X.astype(np.float64) - q[None, :, 0], Y.astype(np.float64) - q[None, :, 1], np.float64(z) - q[None, :, 2].astype(np.float64)
        w = np.maximum(1.0 - ((dx * dx + dy * dy) + dz * dz) * inv_s2, 0.0) ** 2 * hit
        count[:, :, k] = hit.sum(1).reshape(dims[0], dims[1])
        W[:, :, k] = w.sum(1).reshape(dims[0], dims[1])
        F[:, :, k] = (w * ((qn[None, :, 0] * dx + qn[None, :, 1] * dy) + qn[None, :, 2] * dz)).sum(1).reshape(dims[0], dims[1])
        A[:, :, k] = (w @ qn).reshape(dims[0], dims[1], 3)
        if Cc is not None:
            Cc[:, :, k] = (w @ col[near]).reshape(dims[0], dims[1], 3)
    valid = (count >= min_neighbours) & (W > 0)
    Ws = np.where(valid, W, 1.0)
    return {"count": count, "valid": valid, "f": np.where(valid, F / Ws, 0.0), "a": A / Ws[..., None], "c": None if Cc is None else Cc / Ws[..., None],
            "pos": (xs, ys, zs), "dims": dims}


def _shift(a, off):
    """a[i + off] over the cells: the array of corner values at offset `off` (0 / 1 per axis) of every cell"""
    return a[off[0]:a.shape[0] - 1 + off[0], off[1]:a.shape[1] - 1 + off[1], off[2]:a.shape[2] - 1 + off[2]]


def extract(fd):
    """cells -> vertices and the quads of the field: {"cells": (nv, 3) int in lexicographic order, "pos" / "normal" / "color" (nv, 3) float64,
    "quads": (nq, 4, 3) int, the four cells of every quad in the definition's order}"""
    valid, f = fd["valid"], fd["f"]
    inside = valid & (f < 0)
    offs = [(c & 1, (c >> 1) & 1, c >> 2) for c in range(8)]
    allv = np.logical_and.reduce([_shift(valid, o) for o in offs])
    n_in = sum(_shift(inside, o).astype(np.int64) for o in offs)
    active = allv & (n_in > 0) & (n_in < 8)
    quads = []
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        e = np.zeros(3, int); e[a] = 1
        lo = np.zeros(3, int); lo[u] = 1; lo[w] = 1
        hi = np.array(valid.shape) - 1                                                       # c + e_a exists; cells c and c - e_u - e_w exist
        hi[u] -= 1; hi[w] -= 1
        if (hi <= lo).any():
            continue
        c = np.stack(np.meshgrid(*[np.arange(lo[d], hi[d]) for d in range(3)], indexing="ij"), -1).reshape(-1, 3)
        c2 = c + e
        at = lambda arr, idx: arr[idx[:, 0], idx[:, 1], idx[:, 2]]  # noqa: E731
        cond = at(valid, c) & at(valid, c2) & (at(inside, c) != at(inside, c2))
        eu = np.zeros(3, int); eu[u] = 1
        ew = np.zeros(3, int); ew[w] = 1
        ring = [c, c - eu, c - eu - ew, c - ew]
        for r in ring:
            cond &= at(active, r)
        sel = np.nonzero(cond)[0]
        qa = np.stack([r[sel] for r in ring], 1)
        rev = ~at(inside, c[sel])
        qa[rev] = qa[rev][:, ::-1]
        quads.append(qa)
    quads = np.concatenate(quads) if quads else np.zeros((0, 4, 3), int)
    cells = np.unique(quads.reshape(-1, 3), axis=0) if len(quads) else np.zeros((0, 3), int)
    xs = fd["pos"]
    P, A, Cc, cnt = np.zeros((len(cells), 3)), np.zeros((len(cells), 3)), np.zeros((len(cells), 3)), np.zeros(len(cells))
    for a in range(3):
        u, w = (a + 1) % 3, (a + 2) % 3
        for ed in range(4):
            oa = np.zeros(3, int); oa[u] = ed & 1; oa[w] = ed >> 1
            ob = oa.copy(); ob[a] = 1
            ia, ib = cells + oa, cells + ob
            fa, fb = f[ia[:, 0], ia[:, 1], ia[:, 2]], f[ib[:, 0], ib[:, 1], ib[:, 2]]
            m = (fa < 0) != (fb < 0)
            with np.errstate(all="ignore"):
                t = np.where(m, fa / (fa - fb), 0.0)
            for d in range(3):
                xa, xb = xs[d][ia[:, d]].astype(np.float64), xs[d][ib[:, d]].astype(np.float64)
                P[:, d] += np.where(m, xa + t * (xb - xa), 0.0)
            aa, ab = fd["a"][ia[:, 0], ia[:, 1], ia[:, 2]], fd["a"][ib[:, 0], ib[:, 1], ib[:, 2]]
            A += np.where(m[:, None], aa + t[:, None] * (ab - aa), 0.0)
            if fd["c"] is not None:
                ka, kb = fd["c"][ia[:, 0], ia[:, 1], ia[:, 2]], fd["c"][ib[:, 0], ib[:, 1], ib[:, 2]]
                Cc += np.where(m[:, None], ka + t[:, None] * (kb - ka), 0.0)
            cnt += m
    P, A, Cc = P / cnt[:, None], A / cnt[:, None], Cc / cnt[:, None]
    ln = np.sqrt((A[:, 0] * A[:, 0] + A[:, 1] * A[:, 1]) + A[:, 2] * A[:, 2])
    N = np.where(ln[:, None] > 0, A / np.where(ln > 0, ln, 1.0)[:, None], 0.0)
    return {"cells": cells, "pos": P, "normal": N, "color": Cc if fd["c"] is not None else None, "quads": quads, "active": active}


def mesh(points, normals, colors, origin, voxel, dims, support, min_neighbours=3):
    fd = field(points, normals, colors, origin, voxel, dims, support, min_neighbours)
    out = extract(fd)
    out["field"] = fd
    return out


def min_abs_f_in_voxels(fd, voxel):
    """the evaluated (valid) corner closest to zero, in voxels: a fixture must keep it above the fp64 rounding of the sums"""
    v = fd["valid"]
    return float(np.abs(fd["f"][v]).min() / voxel) if v.any() else np.inf


def cell_key(cells):
    """(n, 3) cells -> int64 keys"""
    c = np.asarray(cells, np.int64)
    return (c[..., 0] << 42) | (c[..., 1] << 21) | c[..., 2]


def normalised_quads(quad_cells):
    """(nq, 4, 3) cells -> sorted (nq, 4) keys, each quad rotated so that its smallest key comes first: orientation is kept"""
    k = cell_key(quad_cells)
    if not len(k):
        return k.reshape(0, 4)
    first = np.argmin(k, 1)
    k = np.stack([np.roll(row, -s) for row, s in zip(k, first)])
    return k[np.lexsort(k.T[::-1])]


# ---------------- topology of a quad mesh given as vertex indices ----------------
def edge_use(quads):
    """{undirected edge: uses} and {directed edge: uses} of (nq, 4) vertex indices"""
    q = np.asarray(quads, np.int64)
    a, b = q.reshape(-1), np.roll(q, -1, 1).reshape(-1)
    und = np.stack([np.minimum(a, b), np.maximum(a, b)], 1)
    _, und_counts = np.unique(und, axis=0, return_counts=True)
    _, dir_counts = np.unique(np.stack([a, b], 1), axis=0, return_counts=True)
    return und_counts, dir_counts


def euler(n_vertices, quads):
    und, _ = edge_use(quads)
    return n_vertices - len(und) + len(quads)


# ---------------- fixtures ----------------
def sphere_cloud(seed, n, centre, R, sigma=0.002, outward=True):
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1)[:, None]
    p = (np.asarray(centre) + R * v + rng.normal(scale=sigma, size=(n, 3))).astype(np.float32)
    nrm = (v if outward else -v).astype(np.float32) * rng.uniform(0.5, 2.0, (n, 1)).astype(np.float32)     # (any length: normalised in fp64)
    col = (np.clip(v * 0.5 + 0.5, 0, 1) * 255).astype(np.float32)
    return p, nrm, col


def corner_cloud(seed, n, shift, sigma=0.002):
    """three unit squares of side 1 that meet in `shift`: the planes x, y, z = shift, normals towards +"""
    rng = np.random.default_rng(seed)
    uv = rng.uniform(0, 1, (n, 2))
    axis = np.arange(n) % 3
    p = np.zeros((n, 3))
    nrm = np.zeros((n, 3), np.float32)
    for a in range(3):
        m = axis == a
        p[np.ix_(m, [k for k in range(3) if k != a])] = uv[m]
        nrm[m, a] = 1.0
    p = (p + np.asarray(shift) + rng.normal(scale=sigma, size=p.shape)).astype(np.float32)
    col = rng.uniform(0, 255, (n, 3)).astype(np.float32)
    return p, nrm, col


def plane_cloud(seed, n, side=1.0, z=0.3, sigma=0.002):
    rng = np.random.default_rng(seed)
    p = np.concatenate([rng.uniform(0, side, (n, 2)), z + rng.normal(scale=sigma, size=(n, 1))], 1).astype(np.float32)
    nrm = np.tile(np.array([[0, 0, 1]], np.float32), (n, 1))
    return p, nrm, None


def lattice(points, normals, voxel, support):
    """origin (float32[3]) and dims of the eligible points' bounding box grown by support -- maskfusion_amd.mesh.lattice_for's rule"""
    ok = eligible(points, normals)
    p = np.asarray(points, np.float32)[ok].astype(np.float64)
    origin = (p.min(0) - support).astype(np.float32)
    dims = np.ceil((p.max(0) + support - origin.astype(np.float64)) / voxel).astype(np.int64) + 2
    return origin, np.maximum(dims, 2).astype(np.int32)
