"""Surfel meshing on the device (mf_cloud_mesh_build_dev / mf_cloud_mesh_emit_dev, maskfusion_amd.mesh, MaskFusion.saveMesh, -emesh) against the
dense brute-force restatement of tests/mesh_restatement.py: the vertex cells and the quads exactly, positions, normals and colours inside
the stored-fp32 interval of the restatement's fp64 value +- 1e-9; topology on a sphere and a plane patch; ineligible points; a lattice of
900^3 corners that only a sparse structure can hold; the argument checks; the command and the driver end to end.  Runs on the MI355X (-m gpu)
and, with MF_EMU=1, on the CPU-executed build.

The gate is test_gpu_eval_normals.py's, with its argument: the device's fp64 sums differ from the restatement's by the order of the addends
(about k 2^-53 relative, k the neighbours of a corner: below 1e-12 here), the store rounds monotonically, so the stored fp32 value lies in
[fl32(r - 1e-9), fl32(r + 1e-9)] of the restatement's fp64 r.  A side decision (f < 0) could only differ for a corner with |f| inside that
rounding: every fixture asserts that none of its evaluated corners has |f| < 1e-9 voxel.  Two DEVICE results of the same input (two builds;
a part of the cloud meshed alone) are two stores of fp64 values within 2e-9 of each other: equal, or neighbouring fp32 values."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import mesh_restatement as mr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"
TOL = 1e-9
VOXEL = 0.06
SUPPORT = 2.5 * VOXEL
SPHERE_C, SPHERE_R = np.array([0.31, -0.22, 0.13]), 0.5
CORNER_AT = np.array([-0.45, -0.37, -0.52])          # the three squares reach from here to +0.55: across zero on every axis

_cache = {}


def _fixture(name):
    """cloud, lattice and the restatement's mesh, computed once and shared (treat as read-only)"""
    if name not in _cache:
        if name == "sphere":
            p, n, c = mr.sphere_cloud(5, 3000, SPHERE_C, SPHERE_R)
            voxel, support = VOXEL, SUPPORT
        elif name == "corner":
            p, n, c = mr.corner_cloud(6, 4500, CORNER_AT)
            voxel, support = VOXEL, 2.0 * VOXEL
        else:
            p, n, c = mr.plane_cloud(7, 3000)
            voxel, support = 0.05, 0.125
        origin, dims = mr.lattice(p, n, voxel, support)
        assert len(p) <= 6000 and dims.max() <= 30 and (dims > 8).sum() >= 2, dims          # several 8-corner blocks
        if name == "corner":
            assert (np.abs(np.rint(origin / np.float32(voxel)) - origin / np.float32(voxel)) > 0.01).all() and (origin < 0).all()
        ref = mr.mesh(p, n, c, origin, voxel, dims, support, 3)
        lowest = mr.min_abs_f_in_voxels(ref["field"], voxel)
        print("%s: %d points, lattice %s, %d vertices, %d quads, min |f| = %.3g voxel" % (name, len(p), dims, len(ref["cells"]), len(ref["quads"]), lowest))
        assert lowest >= 1e-9
        _cache[name] = dict(p=p, n=n, c=c, voxel=voxel, support=support, origin=origin, dims=dims, ref=ref)
    return _cache[name]


def _mesh(fx, p=None, n=None, c="fixture", min_neighbours=3):
    """the device mesh of a fixture's lattice: vertices, normals, colours, quads (vertex indices), cells"""
    from maskfusion_amd import mesh as M
    c = fx["c"] if isinstance(c, str) else c
    return M.mesh_cloud(fx["p"] if p is None else p, fx["n"] if n is None else n, c, voxel=fx["voxel"], support=fx["support"],
                        min_neighbours=min_neighbours, origin=fx["origin"], dims=fx["dims"], return_quads=True)


def _stored_within(got32, want64, tol=TOL):
    want64 = np.asarray(want64, np.float64)
    return (got32 >= (want64 - tol).astype(np.float32)) & (got32 <= (want64 + tol).astype(np.float32))


def _same_or_neighbours(a, b):
    return (a == b) | (np.nextafter(a, b) == b)


def _check_against(ref, v, nr, co, q, ce):
    order = np.argsort(mr.cell_key(ce))
    assert len(ce) == len(ref["cells"]) and (mr.cell_key(ce)[order] == mr.cell_key(ref["cells"])).all()
    assert len(q) == len(ref["quads"]) and (mr.normalised_quads(ce[q]) == mr.normalised_quads(ref["quads"])).all()
    print("max |stored - fp64|: position %.3g, normal %.3g, colour %.3g" % (
        np.abs(v[order] - ref["pos"]).max(), np.abs(nr[order] - ref["normal"]).max(), 0.0 if co is None else np.abs(co[order] - ref["color"]).max()))
    assert _stored_within(v[order], ref["pos"]).all() and _stored_within(nr[order], ref["normal"]).all()
    if ref["color"] is not None:
        assert _stored_within(co[order], ref["color"]).all()


# ---------------- against the restatement ----------------
@pytest.mark.parametrize("name", ["sphere", "corner"])
def test_mesh_is_the_restatements(hip, name):
    fx = _fixture(name)
    v, nr, co, q, ce = _mesh(fx)
    assert v.dtype == np.float32 and q.dtype == np.int32 and ce.dtype == np.int32 and len(v) > 500 and len(q) > 500
    _check_against(fx["ref"], v, nr, co, q, ce)
    # the cells come in the order of the scan: blocks, then corners in a block -- no two alike, every vertex named by a quad
    assert len(np.unique(mr.cell_key(ce))) == len(ce) and len(np.unique(q)) == len(v)


def test_sphere_is_closed_and_faces_outward(hip):
    fx = _fixture("sphere")
    v, nr, _, q, _ = _mesh(fx)
    und, drc = mr.edge_use(q)
    assert (und == 2).all() and (drc == 1).all()                  # every edge in exactly two quads, once in each direction
    assert mr.euler(len(v), q) == 2
    P = v[q].astype(np.float64)
    fn = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]) + np.cross(P[:, 2] - P[:, 0], P[:, 3] - P[:, 0])
    assert ((fn * (P.mean(1) - SPHERE_C)).sum(1) > 0).all()
    assert ((nr * (v - SPHERE_C)).sum(1) > 0.9 * SPHERE_R * 0.9).all()
    off = np.abs(np.linalg.norm(v.astype(np.float64) - SPHERE_C, axis=1) - SPHERE_R).max()
    print("vertices within %.3f voxel of the sphere" % (off / fx["voxel"]))
    assert off <= fx["voxel"] / 2


def test_plane_patch_is_open_and_min_neighbours_only_removes(hip):
    fx = _fixture("plane")
    v, nr, co, q, ce = _mesh(fx)
    assert co is None
    _check_against(fx["ref"], v, nr, None, q, ce)
    und, drc = mr.edge_use(q)
    assert set(np.unique(und)) == {1, 2} and (drc == 1).all()    # an open border, nothing non-manifold
    assert len(np.unique(q)) == len(v)                            # no unreferenced vertex
    assert (nr[:, 2] > 0.99).all() and np.abs(v[:, 2] - 0.3).max() <= fx["voxel"] / 2
    more = _mesh(fx, min_neighbours=12)
    k3, k12 = set(mr.cell_key(ce).tolist()), set(mr.cell_key(more[4]).tolist())
    print("cells: %d with min_neighbours 3, %d with 12" % (len(k3), len(k12)))
    assert k12 < k3 and len(k12) > 100


def test_ineligible_points_change_nothing(hip):
    fx = _fixture("sphere")
    rng = np.random.default_rng(8)
    n_bad = 200
    at = np.sort(rng.choice(len(fx["p"]) + n_bad, n_bad, replace=False))
    keep = np.ones(len(fx["p"]) + n_bad, bool)
    keep[at] = False
    p = np.zeros((len(keep), 3), np.float32); n = np.zeros_like(p); c = np.zeros_like(p)
    p[keep], n[keep], c[keep] = fx["p"], fx["n"], fx["c"]
    p[at] = (SPHERE_C + rng.normal(scale=0.3, size=(n_bad, 3))).astype(np.float32)       # in the middle of the lattice
    n[at] = rng.normal(size=(n_bad, 3)).astype(np.float32)
    c[at] = 255.0
    p[at[:50], 0] = np.nan
    p[at[50:70], 2] = np.inf
    n[at[70:120]] = 0.0
    n[at[120:160], 1] = np.nan
    n[at[160:], 2] = -np.inf
    assert not mr.eligible(p, n)[at].any() and mr.eligible(p, n)[keep].all()
    _check_against(fx["ref"], *_mesh(fx, p, n, c))


def test_two_builds_of_one_input(hip):
    fx = _fixture("corner")
    a, b = _mesh(fx), _mesh(fx)
    assert (a[3] == b[3]).all() and (a[4] == b[4]).all()
    for k in range(3):
        assert _same_or_neighbours(a[k], b[k]).all()


# ---------------- sparsity ----------------
def test_two_spheres_on_a_900_cube_lattice(hip):
    """Two spheres of 8 cm radius at a 1 cm voxel, 8.7 m apart on EVERY axis (the lattice diagonal; 15 m between the centres): the lattice has
    about 900^3 corners -- 5.8 GB of fp64 for one dense scalar field -- and 113^3 blocks, of which a few hundred are occupied.  The result
    equals the two spheres meshed alone on the same lattice, one after the other."""
    from maskfusion_amd import mesh as M
    voxel, support = 0.01, 0.025
    a = mr.sphere_cloud(9, 1200, [-4.31, -4.42, -4.27], 0.08, sigma=0.0005)
    b = mr.sphere_cloud(10, 1200, [4.39, 4.28, 4.43], 0.08, sigma=0.0005)
    both = [np.concatenate([x, y]) for x, y in zip(a, b)]
    origin, dims = mr.lattice(both[0], both[1], voxel, support)
    print("lattice", dims)
    assert (dims > 850).all()
    kw = dict(voxel=voxel, support=support, origin=origin, dims=dims, return_quads=True)
    va, na, ca, qa, cea = M.mesh_cloud(*a, **kw)
    vb, nb, cb, qb, ceb = M.mesh_cloud(*b, **kw)
    v, n, c, q, ce = M.mesh_cloud(*both, **kw)
    for part, cen in ((va, a[0].mean(0)), (vb, b[0].mean(0))):
        und, _ = mr.edge_use(qa if part is va else qb)
        assert len(part) > 300 and (und == 2).all() and np.abs(np.linalg.norm(part - cen, axis=1) - 0.08).max() <= voxel / 2
    # block order is lattice order: the low sphere's vertices come first
    assert len(v) == len(va) + len(vb) and (ce == np.concatenate([cea, ceb])).all()
    assert (q == np.concatenate([qa, qb + len(va)])).all()
    for got, parts in ((v, (va, vb)), (n, (na, nb)), (c, (ca, cb))):
        assert _same_or_neighbours(got, np.concatenate(parts)).all()


# ---------------- arguments ----------------
def _raw_args(fx, n_points=None):
    import torch
    from maskfusion_amd.lib import load, torch_device
    L = load()
    rec = torch.from_numpy(np.concatenate([fx["p"], fx["n"], fx["c"]], 1)).to(torch_device()).contiguous()
    origin = np.ascontiguousarray(fx["origin"], np.float32)
    dims = np.ascontiguousarray(fx["dims"], np.int32)
    h, nv, nq = C.c_void_p(), C.c_uint32(7), C.c_uint32(7)
    n = len(fx["p"]) if n_points is None else n_points
    args = [rec.data_ptr(), 9, 3, 6, n, origin.ctypes.data, float(fx["voxel"]), dims.ctypes.data, float(fx["support"]), 3, C.byref(h), C.byref(nv),
            C.byref(nq), None, None]
    return L, args, (rec, origin, dims, h, nv, nq)


def test_argument_checks(hip):
    fx = _fixture("sphere")
    L, args, keep = _raw_args(fx, 500)
    rec, origin, dims, h, nv, nq = keep
    assert L.mf_cloud_mesh_build_dev(*args) == 0 and h.value
    L.mf_cloud_mesh_free(h)
    L.mf_cloud_mesh_free(None)
    f32 = lambda *x: np.array(x, np.float32)  # noqa: E731
    i32 = lambda *x: np.array(x, np.int32)  # noqa: E731
    big = f32(2.0 ** 31, 0, 0)
    cases = [(0, None), (1, 5), (1, 0), (2, 2), (2, 7), (2, -1), (3, 2), (3, 7), (4, -1), (4, (1 << 30) + 1), (5, None),
             (5, f32(np.nan, 0, 0)), (5, f32(0, np.inf, 0)), (5, big), (6, 0.0), (6, -0.06), (6, float("nan")), (6, float("inf")), (7, None),
             (7, i32(1, 24, 24)), (7, i32(24, 24, -3)), (7, i32(1 << 30, 1 << 30, 8)), (7, i32(5000, 5000, 5000)), (8, 0.05), (8, 0.49), (8, float("nan")),
             (8, float("inf")), (9, 0), (9, -2), (10, None), (11, None), (12, None)]
    for k, val in cases:
        bad = list(args)
        bad[k] = val.ctypes.data if isinstance(val, np.ndarray) else val
        h.value = None
        assert L.mf_cloud_mesh_build_dev(*bad) == -1, (k, val)
        why = L.mf_last_error(None).decode()
        assert why.startswith("mf_cloud_mesh: ") and len(why) > 20, why
        assert not h.value
    # a lattice corner beyond the grid's cell limit: the origin is fine, the far end is not
    far = list(args)
    far[5], far[6], far[8] = f32(0, 0, 0).ctypes.data, 1e-3, 1e-3
    far[7] = i32(2, 2, (1 << 30) + 5).ctypes.data
    assert L.mf_cloud_mesh_build_dev(*far) == -1
    # an eligible point beyond it
    import torch
    moved = rec.clone()
    moved[17, 1] = float(np.float32(2.0 ** 31) * np.float32(fx["support"]))
    far = list(args)
    far[0] = moved.data_ptr()
    assert L.mf_cloud_mesh_build_dev(*far) == -1 and "2^30" in L.mf_last_error(None).decode() and not h.value
    # the colour may be left out; emit refuses colours then, and a null handle or output
    no_col = list(args)
    no_col[3] = -1
    assert L.mf_cloud_mesh_build_dev(*no_col) == 0 and nv.value > 0 and nq.value > 0
    dev = rec.device
    v = torch.empty((nv.value, 3), dtype=torch.float32, device=dev)
    q = torch.empty((nq.value, 4), dtype=torch.int32, device=dev)
    assert L.mf_cloud_mesh_emit_dev(h, v.data_ptr(), None, None, None, q.data_ptr(), None) == 0
    assert L.mf_cloud_mesh_emit_dev(h, v.data_ptr(), None, v.data_ptr(), None, q.data_ptr(), None) == -1
    assert L.mf_cloud_mesh_emit_dev(h, None, None, None, None, q.data_ptr(), None) == -1
    assert L.mf_cloud_mesh_emit_dev(h, v.data_ptr(), None, None, None, None, None) == -1
    assert L.mf_cloud_mesh_emit_dev(None, v.data_ptr(), None, None, None, q.data_ptr(), None) == -1
    L.mf_cloud_mesh_free(h)
    from maskfusion_amd import mesh as M
    from maskfusion_amd.lib import MFError
    with pytest.raises(MFError, match="support"):
        M.mesh_cloud(fx["p"], fx["n"], voxel=0.06, support=0.7)


def test_empty_clouds(hip):
    from maskfusion_amd import mesh as M
    fx = _fixture("sphere")
    L, args, (rec, origin, dims, h, nv, nq) = _raw_args(fx, 0)
    args[0] = None
    assert L.mf_cloud_mesh_build_dev(*args) == 0 and h.value and nv.value == 0 and nq.value == 0
    assert L.mf_cloud_mesh_emit_dev(h, None, None, None, None, None, None) == 0
    L.mf_cloud_mesh_free(h)
    z = np.zeros((0, 3), np.float32)
    v, n, c, t = M.mesh_cloud(z, z, z, voxel=0.05)
    assert v.shape == (0, 3) and n.shape == (0, 3) and c.shape == (0, 3) and t.shape == (0, 3)
    # points, but none eligible; and points that reach no lattice corner's neighbourhood in numbers
    p = fx["p"][:50]
    assert len(M.mesh_cloud(p, np.zeros_like(p), voxel=0.05)[0]) == 0
    assert len(_mesh(fx, fx["p"][:2], fx["n"][:2], fx["c"][:2])[0]) == 0


# ---------------- end to end ----------------
def _mesh_command(args):
    if EMU:    # the child drives the same CPU-executed build as this process
        cmd = [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import mesh as m; "
               "sys.exit(m.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"))] + args
    else:
        cmd = [sys.executable, "-m", "maskfusion_amd.mesh"] + args
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_mesh_command_on_a_saved_cloud(hip, tmp_path):
    """a sphere uploaded as a model's map, written by mf_save_ply, meshed by the command: faces, and vertices on the sphere"""
    from maskfusion_amd import MaskFusion
    from maskfusion_amd import eval as ev
    from maskfusion_amd import mesh as M
    centre, R, voxel = np.array([0.1, -0.05, 1.5]), 0.4, 0.04
    p, n, col = mr.sphere_cloud(11, 4000, centre, R, sigma=0.001)
    n /= np.linalg.norm(n, axis=1)[:, None]
    rec = np.zeros((len(p), 12), np.float32)
    rec[:, :3], rec[:, 3] = p, 20.0
    rgb = col.astype(np.int64)
    rec[:, 4] = (rgb[:, 0] << 16 | rgb[:, 1] << 8 | rgb[:, 2]).astype(np.float32)
    rec[:, 6], rec[:, 7] = 1.0, 1.0
    rec[:, 8:11], rec[:, 11] = -n, 0.02                     # the map's normals face away from the camera; mf_save_ply negates them
    rec[::40, 3] = 0.5                                      # unstable surfels, which mf_save_ply leaves out
    m = MaskFusion(160, 120, 132.0, 132.0, 80.0, 60.0, numGSurfels=1 << 16, enableMultipleModels=False, initConfidenceGlobal=4.0)
    m.getBackgroundModel().uploadMap(rec)
    out = str(tmp_path) + os.sep
    m.savePly(out)
    paths = m.saveMesh(out, voxel)
    m.close()
    assert len(ev.read_ply(out + "cloud-0.ply")) == len(p) - len(p[::40])
    r = _mesh_command(["--cloud", out + "cloud-0.ply", "--voxel", str(voxel), "-o", out + "by-command.ply"])
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    truth = mr.sphere_cloud(12, 200_000, centre, R, sigma=0.0)[0]
    for path in (out + "by-command.ply", paths[0]):
        got = M.read_mesh_ply(path)
        v, t = got["vertices"], got["triangles"]
        assert len(t) > 500 and t.min() == 0 and t.max() == len(v) - 1 and got["colors"] is not None and got["normals"] is not None
        assert (ev.read_ply(path) == v).all()
        acc = ev.compare_clouds(v, truth, radius=0.1, taus=(voxel / 2,))["accuracy"]
        print(path, "accuracy", acc)
        assert acc["misses"] == 0 and acc["fraction"]["%g" % (voxel / 2)] == 1.0 and acc["mean"] <= voxel / 2
        und, _ = mr.edge_use(np.concatenate([t[0::2], t[1::2, 2:3]], 1))      # the quads back from their two triangles
        assert (und == 2).all()
        assert ((got["normals"] * (v - centre)).sum(1) > 0).all()             # mf_save_ply's normals face outward, and so do the mesh's
    assert info["vertices"] == len(M.read_mesh_ply(out + "by-command.ply")["vertices"]) and paths == [out + "mesh-0.ply"]
    # the driver's mesh is the command's mesh of the driver's cloud
    a, b = M.read_mesh_ply(paths[0]), M.read_mesh_ply(out + "by-command.ply")
    assert (a["triangles"] == b["triangles"]).all() and _same_or_neighbours(a["vertices"], b["vertices"]).all()
    r = _mesh_command(["--cloud", out + "missing.ply", "--voxel", "0.04", "-o", out + "x.ply"])
    assert r.returncode == 2 and "error" in r.stderr


def test_cli_writes_a_mesh_per_model(hip, tmp_path, capsys):
    from maskfusion_amd import cli, synth
    from maskfusion_amd import mesh as M
    from maskfusion_amd.io import write_image_dir
    W, H = 320, 240
    f = 528.0 * W / 640.0
    st = synth.Stream(W=W, H=H, fx=f, fy=f, cx=W / 2.0, cy=H / 2.0, noise=False)
    fr = [st.frame(k) for k in range(4)]
    seq = str(tmp_path / "seq") + os.sep
    write_image_dir(seq, [(x[0], x[1]) for x in fr], calibration=(st.fx, st.fy, st.cx, st.cy, st.W, st.H))
    out = str(tmp_path / "out") + os.sep
    assert cli.main(["-dir", seq, "-static", "-run", "-q", "-em", "-emesh", "0.05", "-exportdir", out, "-i", "100", "-nso", "-confG", "1"]) == 0
    clouds = sorted(x for x in os.listdir(out) if x.startswith("cloud-"))
    meshes = sorted(x for x in os.listdir(out) if x.startswith("mesh-"))
    assert clouds == ["cloud-0.ply"] and meshes == ["mesh-0.ply"]
    got = M.read_mesh_ply(out + "mesh-0.ply")
    print("mesh-0.ply: %d vertices, %d triangles" % (len(got["vertices"]), len(got["triangles"])))
    assert len(got["triangles"]) > 1000 and got["triangles"].max() == len(got["vertices"]) - 1
