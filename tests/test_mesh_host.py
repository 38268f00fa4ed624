"""Surfel meshing without a GPU: the numpy restatement by itself (tests/mesh_restatement.py: what the device is compared with in
tests/test_gpu_mesh.py), the PLY mesh writer, and the argument checks of mf_cloud_mesh_build_dev, which come before the first device call."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402


def test_restatement_sphere_is_closed_and_faces_outward():
    centre, R, voxel, support = np.array([0.31, -0.22, 0.13]), 0.5, 0.07, 0.16
    p, n, c = mr.sphere_cloud(3, 2500, centre, R)
    origin, dims = mr.lattice(p, n, voxel, support)
    m = mr.mesh(p, n, c, origin, voxel, dims, support, 3)
    assert mr.min_abs_f_in_voxels(m["field"], voxel) >= 1e-9
    key = {k: i for i, k in enumerate(mr.cell_key(m["cells"]).tolist())}
    q = np.array([[key[k] for k in row] for row in mr.cell_key(m["quads"]).tolist()])
    und, drc = mr.edge_use(q)
    assert len(q) > 500 and (und == 2).all() and (drc == 1).all() and mr.euler(len(m["cells"]), q) == 2
    P = m["pos"][q]
    fn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) + np.cross(P[:, 2] - P[:, 0], P[:, 3] - P[:, 0])
    assert ((fn * (P.mean(1) - centre)).sum(1) > 0).all() and ((m["normal"] * (m["pos"] - centre)).sum(1) > 0).all()
    off = np.abs(np.linalg.norm(m["pos"] - centre, axis=1) - R).max()
    print("restatement: %d vertices within %.3f voxel of the sphere" % (len(q), off / voxel))
    assert off <= voxel / 4
    assert m["color"].min() >= 0 and m["color"].max() <= 255
    # inward normals turn every face round
    p2, n2, _ = mr.sphere_cloud(3, 2500, centre, R, outward=False)
    m2 = mr.mesh(p2, n2, None, origin, voxel, dims, support, 3)
    assert (mr.cell_key(m2["cells"]) == mr.cell_key(m["cells"])).all() and m2["color"] is None
    assert (mr.normalised_quads(m2["quads"][:, ::-1]) == mr.normalised_quads(m["quads"])).all()


def test_restatement_slab_has_two_sheets():
    """a wall thinner than a voxel, seen from both sides: two sheets (DESIGN.md "Surfel meshing", known limits)"""
    rng = np.random.default_rng(4)
    n_pts, voxel, support = 3000, 0.05, 0.1
    xy = rng.uniform(0, 0.8, (n_pts, 2))
    side = np.where(np.arange(n_pts) % 2 == 0, 1.0, -1.0)
    p = np.concatenate([xy, (0.01 * side)[:, None]], 1).astype(np.float32)
    n = np.zeros((n_pts, 3), np.float32)
    n[:, 2] = side
    origin, dims = mr.lattice(p, n, voxel, support)
    m = mr.mesh(p, n, None, origin, voxel, dims, support, 3)
    z = m["pos"][:, 2]
    assert (z > 0.005).sum() > 100 and (z < -0.005).sum() > 100
    assert (m["normal"][z > 0.005, 2] > 0).all() and (m["normal"][z < -0.005, 2] < 0).all()


def test_mesh_ply_round_trip(tmp_path):
    from maskfusion_amd import eval as ev
    from maskfusion_amd import mesh as M
    rng = np.random.default_rng(5)
    v = rng.normal(size=(40, 3)).astype(np.float32)
    n = rng.normal(size=(40, 3)).astype(np.float32)
    c = rng.uniform(-20, 300, (40, 3)).astype(np.float32)
    q = rng.integers(0, 40, (25, 4)).astype(np.int32)
    t = M.quads_to_triangles(q)
    assert t.shape == (50, 3) and (t[0] == q[0, [0, 1, 2]]).all() and (t[1] == q[0, [0, 2, 3]]).all()
    path = str(tmp_path / "m.ply")
    M.write_mesh_ply(path, v, n, c, t)
    head = open(path, "rb").read().split(b"end_header\n")[0].decode().split("\n")
    assert head[:3] == ["ply", "format binary_little_endian 1.0", "element vertex 40"]
    assert [l for l in head if l.startswith("property")] == [
        "property float x", "property float y", "property float z", "property uchar red", "property uchar green", "property uchar blue",
        "property float nx", "property float ny", "property float nz", "property list uchar int vertex_indices"]
    assert head.index("element face 50") > head.index("property float nz")
    got = M.read_mesh_ply(path)
    assert (got["vertices"] == v).all() and (got["normals"] == n).all() and (got["triangles"] == t).all()
    assert (got["colors"] == np.clip(np.rint(c), 0, 255).astype(np.uint8)).all()
    pts, nrm = ev.read_ply(path, normals=True)                 # the evaluation reads the vertices and ignores the faces
    assert (pts == v).all() and (nrm == n).all()
    p3, n3, c3 = M.read_cloud_ply(path)
    assert (p3 == v).all() and (c3 == got["colors"]).all()
    # bare: no normals, no colours, no faces
    M.write_mesh_ply(path, v)
    got = M.read_mesh_ply(path)
    assert (got["vertices"] == v).all() and got["normals"] is None and got["colors"] is None and got["triangles"].shape == (0, 3)
    with pytest.raises(ValueError):
        M.read_cloud_ply(path)


def test_build_checks_its_arguments_before_it_touches_a_device():
    """every MF_EINVAL of mf_cloud_mesh_build_dev that depends on the arguments alone, with the product library and no device call: the
    pointer to the points is never followed"""
    from maskfusion_amd.lib import load
    L = load()
    f32 = lambda *x: np.array(x, np.float32)  # noqa: E731
    i32 = lambda *x: np.array(x, np.int32)  # noqa: E731
    origin, dims = f32(-1, -1, -1), i32(20, 20, 20)
    h, nv, nq = C.c_void_p(), C.c_uint32(7), C.c_uint32(7)
    fake = 4096                                                   # "device" memory nobody reads
    ok = [fake, 9, 3, 6, 100, origin.ctypes.data, 0.1, dims.ctypes.data, 0.25, 3, C.byref(h), C.byref(nv), C.byref(nq), None, None]
    cases = [(0, None, "null"), (1, 5, "stride"), (2, 2, "stride"), (2, 7, "stride"), (3, 1, "colour"), (3, 8, "colour"), (4, -1, "count"),
             (4, (1 << 30) + 1, "count"), (5, None, "null"), (5, f32(np.nan, 0, 0), "origin"), (5, f32(2.0 ** 31, 0, 0), "2^30"), (6, 0.0, "voxel"),
             (6, float("nan"), "voxel"), (7, None, "null"), (7, i32(20, 1, 20), "dims"), (7, i32(5000, 5000, 5000), "blocks"), (8, 0.09, "support"),
             (8, 0.81, "support"), (8, float("inf"), "support"), (9, 0, "min_neighbours"), (10, None, "null"), (11, None, "null"), (12, None, "null")]
    for k, val, word in cases:
        bad = list(ok)
        bad[k] = val.ctypes.data if isinstance(val, np.ndarray) else val
        assert L.mf_cloud_mesh_build_dev(*bad) == -1, (k, val)
        why = L.mf_last_error(None).decode()
        assert why.startswith("mf_cloud_mesh: ") and word in why, (k, val, why)
        assert not h.value
    # an empty cloud needs no device either
    empty = list(ok)
    empty[0], empty[4] = None, 0
    assert L.mf_cloud_mesh_build_dev(*empty) == 0 and h.value and nv.value == 0 and nq.value == 0
    assert L.mf_cloud_mesh_emit_dev(h, None, None, None, None, None, None) == 0
    L.mf_cloud_mesh_free(h)
    assert L.mf_cloud_mesh_emit_dev(None, None, None, None, None, None, None) == -1
