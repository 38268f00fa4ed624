"""The definition of mf_trimesh_raycast_dev / mf_trimesh_render_dev, held on the host (no GPU): the numpy restatement of
tests/raycast_restatement.py against a long-double Moeller-Trumbore, its watertightness on the icosphere's edges and vertices, the facing
flag, the tie rule and the pinhole rays against the pipeline's vertex-map expression.  tests/test_gpu_raycast.py holds the device to this
restatement bit for bit."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import raycast_restatement as rr  # noqa: E402
import trimesh_restatement as tr  # noqa: E402

_cache = {}


def _sphere():
    if not _cache:
        V, F = tr.icosphere()
        O, D, expect, groups = rr.sphere_rays(V, F)
        _cache.update(V=V, F=F, O=O, D=D, expect=expect, groups=groups, res=rr.raycast(V, F, O, D))
    return _cache


def test_agrees_with_long_double_moller_trumbore():
    """away from the edges (all three weights > 1e-6) both tests choose the same triangle, and t agrees to 1e-12"""
    s = _sphere()
    rows = np.concatenate([np.arange(s["groups"][g].start, s["groups"][g].stop) for g in ("inside", "outside", "grazing")])
    t, w, hit = rr.moller_trumbore(s["V"], s["F"], s["O"][rows], s["D"][rows])
    with np.errstate(invalid="ignore"):
        key = np.where(hit & (t >= 0), t, np.inf)
    k = np.argmin(key, 1)
    r = np.arange(len(rows))
    found = np.isfinite(key[r, k].astype(np.float64))
    clear = found & (w[r, k].min(1) > 1e-6)
    res = s["res"]
    print("rays %d, hits by Moeller-Trumbore %d, away from edges %d" % (len(rows), found.sum(), clear.sum()))
    assert clear.sum() > 700 and (~found).sum() >= 150
    assert (res["tri"][rows][clear] == k[clear]).all()
    dt = np.abs(res["t64"][rows][clear] - t[r, k][clear].astype(np.float64))
    print("max |dt| %.3g" % dt.max())
    assert dt.max() <= 1e-12
    assert (res["tri"][rows][~found] == -1).all()                 # and what it misses by more than an edge's width is missed here


def test_watertight_on_edges_and_vertices():
    s = _sphere()
    assert len(rr.edges(s["F"])) == 480 and len(s["V"]) == 162
    for g, n in (("midpoints", 480), ("vertices", 162), ("origin0", 162)):
        sl = s["groups"][g]
        assert sl.stop - sl.start == n
        assert (s["res"]["tri"][sl] >= 0).all(), (g, np.flatnonzero(s["res"]["tri"][sl] < 0))
    sl = s["groups"]["origin0"]
    assert (s["O"][sl] == 0).all() and (s["D"][sl] == s["V"]).all()
    # the hit is the vertex: t = 1 to fp64 rounding
    assert np.abs(s["res"]["t64"][sl] - 1.0).max() <= 1e-12


def test_expected_hits_and_misses_and_every_axis_branch():
    s = _sphere()
    hit = s["res"]["tri"] >= 0
    assert (hit == (s["expect"] == 1)).all()
    v = s["res"]["valid"]
    assert (~v).sum() == 6
    for kz in range(3):
        for neg in (False, True):
            assert ((s["res"]["kz"] == kz) & (s["res"]["neg"] == neg) & v).sum() >= 2


def test_front_is_the_side_of_the_normal():
    s = _sphere()
    res = s["res"]
    hit = np.flatnonzero(res["tri"] >= 0)
    n = tr.cross_norm2(s["V"], s["F"][res["tri"][hit]])[0]
    d = s["D"][hit].astype(np.float64)
    nd = (n * d).sum(1)
    sure = np.abs(nd) > 1e-9 * np.linalg.norm(n, axis=1) * np.linalg.norm(d, axis=1)
    assert sure.sum() > 1500
    assert (res["front"][hit][sure] == (nd[sure] < 0)).all()
    out = s["groups"]["outside"]
    assert res["front"][out].all() and not res["front"][s["groups"]["inside"]].any()      # counter-clockwise seen from outside


def test_a_tie_goes_to_the_smaller_index():
    s = _sphere()
    sl = s["groups"]["inside"]
    a = rr.raycast(s["V"], s["F"], s["O"][sl], s["D"][sl])
    p, q = (int(x) for x in np.unique(a["tri"])[[3, -3]])          # two triangles that some ray hits
    assert p != q and p >= 0
    F2 = np.concatenate([s["F"][p:p + 1], s["F"], s["F"][q:q + 1]])             # triangle p again in front, triangle q again behind
    b = rr.raycast(s["V"], F2, s["O"][sl], s["D"][sl])
    want = np.where(a["tri"] == p, 0, a["tri"] + 1)
    assert (b["tri"] == want).all() and (b["t64"] == a["t64"]).all() and (b["tri"] == q + 1).sum() >= 1 and (b["tri"] == 0).sum() >= 1


def test_limits_cut_the_nearer_hit():
    s = _sphere()
    sl = s["groups"]["outside"]
    base = s["res"]
    assert (base["t64"][sl] > 0.9).all() and (base["t64"][sl] < 1.2).all()
    far = rr.raycast(s["V"], s["F"], s["O"][sl], s["D"][sl], tmin=1.3)
    assert (far["tri"] >= 0).all() and (far["t64"] > 1.7).all() and not far["front"].any()
    near = rr.raycast(s["V"], s["F"], s["O"][sl], s["D"][sl], tmax=1.3)
    assert (near["tri"] == base["tri"][sl]).all() and (near["t64"] == base["t64"][sl]).all()
    none = rr.raycast(s["V"], s["F"], s["O"][sl], s["D"][sl], tmin=1.3, tmax=1.6)
    assert (none["tri"] == -1).all() and np.isposinf(none["t"]).all() and np.isnan(none["uv"]).all()


def test_pinhole_ray_is_the_vertex_maps():
    """k_vmap_nmap's vertex of pixel (u, v) at depth z is (z (u - cx) (1 / fx), z (v - cy) (1 / fy), z) in fp32, left to right; the ray's
    direction is that vertex at z = 1, bit for bit, and z times it is the vertex to the two roundings the order of the products may differ by"""
    W, H, fx, fy, cx, cy = 64, 48, np.float32(52.8), np.float32(53.1), np.float32(31.5), np.float32(23.25)
    o, d = rr.pinhole_rays(W, H, fx, fy, cx, cy)
    assert (o == 0).all() and d.dtype == np.float32
    y, x = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    u, v = x.reshape(-1).astype(np.float32), y.reshape(-1).astype(np.float32)
    fxi, fyi = np.float32(1) / fx, np.float32(1) / fy
    for z in (np.float32(1.0), np.float32(0.37), np.float32(2.9)):
        vm = np.stack([z * (u - cx) * fxi, z * (v - cy) * fyi, np.full(len(u), z)], 1)
        assert vm.dtype == np.float32
        p = (d * z).astype(np.float32)
        if z == 1:
            assert (p.view(np.uint32) == vm.view(np.uint32)).all()
        assert (np.abs(p.astype(np.float64) - vm) <= 2 * np.spacing(np.abs(vm))).all()
    # and through the restatement: a plane at depth 2 in front of the camera renders as depth 2 at every pixel
    V = np.array([[-9, -9, 2], [9, -9, 2], [9, 9, 2], [-9, 9, 2]], np.float32)
    F = np.array([[0, 1, 2], [0, 2, 3]], np.int32)
    depth, res = rr.render(V, F, W, H, fx, fy, cx, cy, np.eye(4))
    assert (depth == 2).all() and (res["tri"] >= 0).all()
