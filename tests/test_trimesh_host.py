"""Mesh evaluation without a GPU: the numpy restatement of the point-to-triangle distance (tests/trimesh_restatement.py: what the device is
compared with in tests/test_gpu_trimesh.py) against an independent formula, the sampler's invariants, the OBJ reader, and the argument checks
of the mf_trimesh_* calls, which come before the first device call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trimesh_restatement as tr  # noqa: E402


def _segment(p, a, b):
    """distance from p (Q, 1, 3) to the segments a-b (1, T, 3), long double"""
    ab = b - a
    t = np.clip(((p - a) * ab).sum(-1) / (ab * ab).sum(-1), 0, 1)
    return np.sqrt((((a + t[..., None] * ab) - p) ** 2).sum(-1))


def _independent(V, F, P):
    """min over the triangles of: the distance to the plane where the projection falls inside the triangle, and the three clamped
    segments -- no region tests, in np.longdouble"""
    V = V.astype(np.longdouble)
    a, b, c = (V[F[:, k]][None] for k in range(3))
    p = P.astype(np.longdouble)[:, None, :]
    n = np.cross(b - a, c - a)
    n = n / np.sqrt((n * n).sum(-1))[..., None]
    h = ((p - a) * n).sum(-1)
    q = p - h[..., None] * n
    inside = np.ones(h.shape, bool)
    for u, v in ((a, b), (b, c), (c, a)):
        inside &= (np.cross(v - u, q - u) * n).sum(-1) >= 0
    d = np.minimum(np.minimum(_segment(p, a, b), _segment(p, b, c)), _segment(p, c, a))
    return np.where(inside, np.minimum(np.abs(h), d), d).min(1)


def test_restatement_against_an_independent_formula():
    V, F = tr.icosphere()
    assert V.shape == (162, 3) and F.shape == (320, 3)
    Q = tr.icosphere_queries(V, F)
    Q = Q[np.isfinite(Q).all(1)]
    res = tr.distance(V, F, Q, 10.0)                         # every query in range: the plain minimum over all triangles
    want = _independent(V, F, Q)
    err = np.abs(np.sqrt(res["D2"]).astype(np.longdouble) - want).max()
    print("restatement against projection-and-segments: max |d - d'| = %.3g" % float(err))
    assert err <= 1e-12
    # the fixture exercises the tie rule and every branch
    near = tr.distance(V, F, Q, 0.1)
    assert tr.tie_fraction(near) >= 0.03
    assert (np.bincount(near["region"][near["region"] >= 0], minlength=7) >= 2).all()
    assert (near["tri"][-20:] == -1).all() and np.isinf(near["dist"][-20:]).all() and np.isnan(near["closest"][-20:]).all()


def test_sampler_invariants():
    V, F = tr.icosphere()
    density = 2000.0
    s = tr.sample(V, F, density)
    assert s["n"] == 6164 == int(s["units"].sum() // 256) and len(s["points"]) == s["n"]
    r1, r2 = s["bary"][:, 0], s["bary"][:, 1]
    assert min(r1.min(), r2.min(), (1.0 - r1 - r2).min()) >= -1e-12
    assert (np.diff(s["tri"]) >= 0).all()
    area = 0.5 * np.sqrt(tr.cross_norm2(V, F)[1])
    count = np.bincount(s["tri"], minlength=len(F))
    assert (np.abs(count - area * density) <= 1.0 + 1e-9).all(), np.abs(count - area * density).max()
    # the samples lie on their triangles, the normals are the faces' and point outward
    d = tr.distance(V, F, s["points"], 0.01)
    assert d["dist"].max() <= 2e-7                          # (the fp32 store of a point with coordinates below 1)
    assert np.abs(np.linalg.norm(s["normals64"], axis=1) - 1).max() <= 1e-12 and ((s["points"] - tr.SPHERE_C) * s["normals"]).sum(1).min() > 0.4
    # triangles that are not eligible get nothing and keep their index
    F2 = np.concatenate([[[0, 0, 1]], F[:100], [[0, 1, 400]], F[100:]]).astype(np.int32)
    s2 = tr.sample(V, F2, density)
    assert s2["n"] == s["n"] and not np.isin(s2["tri"], [0, 101]).any()
    assert (s2["points"] == s["points"]).all() and (s2["tri"] == np.where(s["tri"] < 100, s["tri"] + 1, s["tri"] + 2)).all()


def test_read_obj(tmp_path):
    from maskfusion_amd import mesh as M
    path = str(tmp_path / "hand.obj")
    with open(path, "w") as f:
        f.write("# a quad, a triangle by negative indices, one by i//k and one by i/j/k\nmtllib x.mtl\no thing\n"
                "v 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvn 0 0 1\nvt 0.5 0.5\n"
                "f 1 2 3 4\n"
                "v 0.5 0.5 1.25\n"
                "f -1 -5 -4\n"
                "f 1//1 3//1 5//1\ns off\nusemtl m\n"
                "f 2/1/1 3/1/1 5/1/1\n"
                "f 1/1 2/1 5/1\n")
    m = M.read_obj(path)
    assert m["vertices"].dtype == np.float32 and m["vertices"].shape == (5, 3) and (m["vertices"][4] == [0.5, 0.5, 1.25]).all()
    assert m["triangles"].dtype == np.int32
    assert m["triangles"].tolist() == [[0, 1, 2], [0, 2, 3], [4, 0, 1], [0, 2, 4], [1, 2, 4], [0, 1, 4]]
    assert m["normals"] is None and m["colors"] is None
    assert M.read_triangle_mesh(path)["triangles"].shape == (6, 3)
    with open(path, "w") as f:
        f.write("v 0 0 0\nf 1 two 3\n")
    with pytest.raises(ValueError, match="hand.obj:2"):
        M.read_obj(path)
    with pytest.raises(ValueError):
        M.read_triangle_mesh(str(tmp_path / "mesh.stl"))


def test_ply_and_obj_round_trip(tmp_path):
    from maskfusion_amd import mesh as M
    V, F = tr.icosphere(1)
    M.write_mesh_ply(str(tmp_path / "m.ply"), V, triangles=F)
    M.write_obj(str(tmp_path / "m.OBJ"), V, F)
    a, b = M.read_triangle_mesh(str(tmp_path / "m.ply")), M.read_triangle_mesh(str(tmp_path / "m.OBJ"))
    for got in (a, b):
        assert got["vertices"].dtype == np.float32 and got["triangles"].dtype == np.int32
        assert (got["vertices"] == V).all() and (got["triangles"] == F).all()


def test_calls_check_their_arguments_before_they_touch_a_device():
    """every MF_EINVAL of the five calls that depends on the arguments alone, with the product library and no device call: no pointer to
    device memory is followed"""
    from maskfusion_amd.lib import load
    L = load()
    nan, inf = float("nan"), float("inf")
    h, ne = C.c_void_p(), C.c_uint32(7)
    fake = 4096                                                   # "device" memory nobody reads

    def refused(fn, args, word):
        assert fn(*args) == -1, args
        why = L.mf_last_error(None).decode()
        assert why.startswith("mf_trimesh: ") and word in why, (args, why)

    ok = [fake, 3, 100, fake, 50, 0.05, C.byref(h), C.byref(ne), None]
    for k, val, word in [(0, None, "null"), (1, 2, "stride"), (2, -1, "count"), (2, (1 << 30) + 1, "count"), (3, None, "null"), (4, -1, "count"),
                         (4, (1 << 30) + 1, "count"), (5, 0.0, "cell"), (5, -1.0, "cell"), (5, nan, "cell"), (5, inf, "cell"), (6, None, "null"),
                         (7, None, "null")]:
        bad = list(ok)
        bad[k] = val
        refused(L.mf_trimesh_build_dev, bad, word)
        assert not h.value
    # a mesh of no triangles needs no device; its handle serves the checks of the other calls
    assert L.mf_trimesh_build_dev(None, 3, 0, None, 0, 0.05, C.byref(h), C.byref(ne), None) == 0 and h.value and ne.value == 0
    T = np.eye(4, dtype=np.float32).T.copy()
    bad_T = T.copy()
    bad_T[3, 1] = np.nan
    ok = [h, fake, 3, 10, T.ctypes.data, 0.1, fake, fake, fake, None]
    for k, val, word in [(0, None, "null"), (1, None, "null"), (2, 2, "stride"), (3, -1, "count"), (3, (1 << 30) + 1, "count"), (4, bad_T.ctypes.data, "transform"),
                         (5, 0.0, "radius"), (5, -0.1, "radius"), (5, nan, "radius"), (5, inf, "radius"), (5, 0.81, "16 cell"), (6, None, "null"),
                         (7, None, "null")]:
        bad = list(ok)
        bad[k] = val
        refused(L.mf_trimesh_distance_dev, bad, word)
    assert L.mf_trimesh_distance_dev(h, None, 3, 0, None, 0.1, None, None, None, None) == 0            # no queries: nothing to do
    n = C.c_uint64(7)
    refused(L.mf_trimesh_sample_emit_dev, [h, None, None, None, None], "plan")
    refused(L.mf_trimesh_sample_emit_dev, [None, fake, None, None, None], "null")
    for bad in ([None, 100.0, C.byref(n), None], [h, 100.0, None, None]):
        refused(L.mf_trimesh_sample_plan_dev, bad, "null")
    for d in (0.0, -5.0, nan, inf):
        refused(L.mf_trimesh_sample_plan_dev, [h, d, C.byref(n), None], "density")
    assert L.mf_trimesh_sample_plan_dev(h, 100.0, C.byref(n), None) == 0 and n.value == 0
    assert L.mf_trimesh_sample_emit_dev(h, None, None, None, None) == 0
    L.mf_trimesh_free(h)
    L.mf_trimesh_free(None)
