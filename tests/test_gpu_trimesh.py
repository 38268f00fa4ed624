"""Mesh evaluation on the device (mf_trimesh_*, maskfusion_amd.eval.TriMesh / compare_cloud_mesh, --ref-mesh, the mesh command's --fidelity)
against the numpy restatement of tests/trimesh_restatement.py.  Runs on the MI355X (-m gpu) and, with MF_EMU=1, on the CPU-executed build.

The gates.  The device and the restatement evaluate the same fp64 operations in the same order, none contracted, so the winning triangle is
the restatement's EXACTLY (ties included: the smallest index) and the closest point is bit-equal to the fp32 rounding of the restated
point.  The distance is (float)sqrt(D2): within one fp32 ulp of the restatement's, for a last-bit difference of the device's fp64 sqrt
before the fp32 rounding and nothing else.  The sampler's count, triangle indices and points are exact; its normals are within one fp32 ulp
per component (the same sqrt, and a division by it)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trimesh_restatement as tr  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU = os.environ.get("MF_EMU") == "1"

_cache = {}


def _fixture(name):
    """mesh, queries and the restatement's answer, computed once and shared (treat as read-only)"""
    if name not in _cache:
        if name == "sphere":
            V, F = tr.icosphere()
            Q, radius, cell = tr.icosphere_queries(V, F), 0.1, 0.05
            assert V.shape == (162, 3) and F.shape == (320, 3) and (V.min(0) < 0).all() and (V.max(0) > 0).all()
        else:
            V, F, R, _ = tr.mixed_mesh()
            Q, radius, cell = tr.mixed_queries(V, F, R), 0.08, 0.02
            assert len(F) == 1602 and len(Q) == 2000
        ref = tr.distance(V, F, Q, radius)
        ties = tr.tie_fraction(ref)
        print("%s: %d triangles, %d queries, %d hits, %.1f %% exact ties, branches %s" % (
            name, len(F), len(Q), (ref["tri"] >= 0).sum(), 100 * ties, np.bincount(ref["region"][ref["region"] >= 0], minlength=7)))
        if name == "sphere":
            assert ties >= 0.03                               # the smallest-index rule is exercised
        else:
            assert ((ref["tri"] >= 0) & (ref["tri"] < 2)).sum() > 100 and (ref["tri"] >= 2).sum() > 100      # wide and gridded triangles both win
        _cache[name] = dict(V=V, F=F, Q=Q, radius=radius, cell=cell, ref=ref)
    return _cache[name]


def _one_ulp(got, want):
    return (got == want) | (np.nextafter(got, want) == want)


def _same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and (a.view(np.uint32 if a.dtype == np.float32 else a.dtype) == b.view(np.uint32 if b.dtype == np.float32 else b.dtype)).all()


def _check(ref, dist, tri, closest):
    assert dist.dtype == np.float32 and tri.dtype == np.int32 and closest.dtype == np.float32
    bad = np.flatnonzero(tri != ref["tri"])
    print("triangles that differ: %d; dist: %d not bit-equal, max |diff| %.3g" % (
        len(bad), (dist != ref["dist"]).sum(), np.abs(np.where(np.isfinite(dist), dist, 0) - np.where(np.isfinite(ref["dist"]), ref["dist"], 0)).max()))
    assert len(bad) == 0, (bad[:10], tri[bad[:10]], ref["tri"][bad[:10]])
    assert _same_bits(closest, ref["closest"])
    assert _one_ulp(dist, ref["dist"]).all()
    miss = tri < 0
    assert np.isposinf(dist[miss]).all() and np.isnan(closest[miss]).all() and np.isfinite(dist[~miss]).all()


def _query(fx, cell=None, radius=None, V=None, F=None, Q=None, T=None):
    from maskfusion_amd import eval as ev
    with ev.TriMesh(fx["V"] if V is None else V, fx["F"] if F is None else F, fx["cell"] if cell is None else cell) as m:
        return m.distance(fx["Q"] if Q is None else Q, fx["radius"] if radius is None else radius, T=T, closest=True) + (m.n_eligible,)


# ---------------- 1, 2: against the restatement ----------------
def test_icosphere_is_the_restatements(hip):
    fx = _fixture("sphere")
    dist, tri, closest, ne = _query(fx)
    assert ne == 320
    _check(fx["ref"], dist, tri, closest)
    assert (tri[-23:] == -1).all()                               # beyond reach, NaN, +-inf


def test_mixed_sizes_are_the_restatements(hip):
    fx = _fixture("mixed")
    dist, tri, closest, ne = _query(fx)
    assert ne == 1602
    _check(fx["ref"], dist, tri, closest)
    assert ((tri >= 0) & (tri < 2)).sum() > 100 and (tri >= 2).sum() > 100


# ---------------- 3: the cell and the radius ----------------
def test_result_depends_on_neither_cell_nor_reach(hip):
    fx = _fixture("mixed")
    base = _query(fx)
    for cell in (0.01, 0.05, 0.3):                               # at 0.3 the quad's box has few cells: it is gridded, not wide
        got = _query(fx, cell=cell)
        assert all(_same_bits(a, b) for a, b in zip(got[:3], base[:3])), cell
    small = _query(fx, radius=0.04)
    within = base[0] <= np.float32(0.04)
    assert within.sum() > 500 and (~within).sum() > 100
    assert all(_same_bits(a[within], b[within]) for a, b in zip(small[:3], base[:3]))
    assert np.isposinf(small[0][~within]).all() and (small[1][~within] == -1).all() and np.isnan(small[2][~within]).all()


# ---------------- 4: ineligible triangles ----------------
def test_ineligible_triangles_change_nothing(hip):
    fx = _fixture("sphere")
    V, F = fx["V"], fx["F"]
    V2 = np.concatenate([V, [[np.nan, 0.3, 0.1]], V[5:6]]).astype(np.float32)     # vertex 162 is NaN, 163 a copy of vertex 5
    nv = len(V2)
    junk = np.array([[5, 9, 163],          # zero area: c - a is zero, though no index repeats
                     [7, 7, 30],           # a repeated index
                     [3, 4, nv],           # an index = n_vertices
                     [-1, 4, 8],           # a negative index
                     [2, 162, 11]], np.int32)   # a NaN vertex
    at = np.sort(np.random.default_rng(31).choice(len(F) + 50, 50, replace=False))
    keep = np.ones(len(F) + 50, bool)
    keep[at] = False
    F2 = np.zeros((len(keep), 3), np.int32)
    F2[keep] = F
    F2[at] = junk[np.arange(50) % len(junk)]
    assert not tr.eligible(V2, F2)[at].any() and tr.eligible(V2, F2)[keep].all()
    dist, tri, closest, ne = _query(fx, V=V2, F=F2)
    assert ne == 320
    mapped = dict(fx["ref"])
    mapped["tri"] = np.where(fx["ref"]["tri"] >= 0, np.flatnonzero(keep)[np.maximum(fx["ref"]["tri"], 0)], -1).astype(np.int32)
    _check(mapped, dist, tri, closest)


# ---------------- 5: the transform ----------------
def test_transform_is_the_host_transform(hip):
    from maskfusion_amd import eval as ev
    fx = _fixture("sphere")
    w = np.array([0.02, -0.03, 0.015])
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) / th
    T = np.eye(4)
    T[:3, :3] = np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K
    T[:3, 3] = [0.004, -0.003, 0.002]
    a = _query(fx, T=T)
    b = _query(fx, Q=ev.transform_f32(T, fx["Q"]))
    assert all(_same_bits(x, y) for x, y in zip(a[:3], b[:3]))
    assert (a[1] != fx["ref"]["tri"]).any()                       # and it moved something


# ---------------- 6: the sampler ----------------
@pytest.mark.parametrize("name", ["sphere", "mixed"])
def test_sampler_is_the_restatements(hip, name):
    from maskfusion_amd import eval as ev
    fx = _fixture(name)
    ref = tr.sample(fx["V"], fx["F"], 2000.0)
    if name == "sphere":
        assert ref["n"] == 6164
    with ev.TriMesh(fx["V"], fx["F"], fx["cell"]) as m:
        p, nr, tri = m.sample(2000.0)
        p_lo, _, tri_lo = m.sample(500.0)                         # a second plan on the same handle emits its own set
        p_again, nr_again, tri_again = m.sample(2000.0)
    assert len(p) == ref["n"] and (tri == ref["tri"]).all() and _same_bits(p, ref["points"])
    assert _one_ulp(nr, ref["normals"]).all()
    low = tr.sample(fx["V"], fx["F"], 500.0)
    assert len(p_lo) == low["n"] < ref["n"] and (tri_lo == low["tri"]).all() and _same_bits(p_lo, low["points"])
    assert _same_bits(p_again, p) and _same_bits(nr_again, nr) and (tri_again == tri).all()


# ---------------- 7: empty and tiny ----------------
def test_empty_and_tiny(hip):
    from maskfusion_amd import eval as ev
    fx = _fixture("sphere")
    Q = fx["Q"][:300]
    with ev.TriMesh(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), 0.05) as m:
        dist, tri, closest = m.distance(Q, 0.1, closest=True)
        assert m.n_eligible == 0 and np.isposinf(dist).all() and (tri == -1).all() and np.isnan(closest).all()
        p, nr, st = m.sample(2000.0)
        assert p.shape == (0, 3) and nr.shape == (0, 3) and st.shape == (0,)
    with ev.TriMesh(fx["V"], np.zeros((0, 3), np.int32), 0.05) as m:       # vertices, no triangles
        assert (m.distance(Q, 0.1)[1] == -1).all()
    F1 = fx["F"][17:18]
    ref = tr.distance(fx["V"], F1, fx["Q"], 0.1)
    assert (ref["tri"] == 0).sum() > 10
    with ev.TriMesh(fx["V"], F1, 0.05) as m:
        _check(ref, *m.distance(fx["Q"], 0.1, closest=True))
        s = tr.sample(fx["V"], F1, 2000.0)
        p, _, st = m.sample(2000.0)
        assert len(p) == s["n"] > 10 and (st == 0).all() and _same_bits(p, s["points"])
        dist, tri = m.distance(np.zeros((0, 3), np.float32), 0.1)          # no queries
        assert dist.shape == (0,) and tri.shape == (0,)
        from maskfusion_amd.lib import MFError
        with pytest.raises(MFError, match="16 cell"):
            m.distance(Q, 0.9)
        far = Q.copy()
        far[7, 1] = float(np.float32(2.0 ** 31) * np.float32(0.05))
        with pytest.raises(MFError, match="2\\^30"):
            m.distance(far, 0.1)


# ---------------- 8: two builds ----------------
def test_two_builds_of_one_input(hip):
    fx = _fixture("mixed")
    a, b = _query(fx), _query(fx)
    assert all(_same_bits(x, y) for x, y in zip(a[:3], b[:3]))


# ---------------- 9: end to end ----------------
def test_compare_cloud_mesh(hip):
    from maskfusion_amd import eval as ev
    fx = _fixture("sphere")
    taus = (0.001, 0.01)
    with ev.TriMesh(fx["V"], fx["F"], 0.025) as m:
        p, nr, tri = m.sample(2000.0)
        same = ev.compare_cloud_mesh(p, m, p, 0.05, taus)
        print("est = the samples:", same["accuracy"], same["reference"])
        assert same["accuracy"]["mean"] <= 1e-6 and same["accuracy"]["misses"] == 0
        assert all(v == 1.0 for v in same["completeness"]["fraction"].values()) and all(v == 1.0 for v in same["fscore"].values())
        assert same["reference"] == {"triangles": 320, "eligible": 320, "samples": len(p), "density": 2000.0}
        # pushed out along the face normals by 5 mm; interior samples only: the closest point of one near an edge may lie on the neighbour
        ref = tr.sample(fx["V"], fx["F"], 2000.0)
        r1, r2 = ref["bary"][:, 0], ref["bary"][:, 1]
        interior = np.minimum(np.minimum(r1, r2), 1.0 - r1 - r2) > 0.15
        assert interior.sum() > 1500
        out = (p.astype(np.float64) + 0.005 * nr)[interior].astype(np.float32)
        moved = ev.compare_cloud_mesh(out, m, p, 0.05, taus)
        print("5 mm off:", moved["accuracy"])
        assert 0.0049 <= moved["accuracy"]["median"] <= 0.0051
        # a transform, and a mask over the samples
        T = np.eye(4)
        T[:3, 3] = [0.0, 0.0, 0.002]
        keep = np.arange(len(p)) % 2 == 0
        part = ev.compare_cloud_mesh(p, m, p, 0.05, taus, T=T, ref_keep=keep)
        assert part["completeness"]["count"] == keep.sum() and 0 < part["accuracy"]["mean"] <= 0.002 + 1e-6


def _command(module, args):
    if EMU:    # the child drives the same CPU-executed build as this process
        cmd = [sys.executable, "-c", "import sys; sys.path[:0] = [%r, %r]; import emu; emu.activate(); from maskfusion_amd import %s as m; "
               "sys.exit(m.main(sys.argv[1:]))" % (ROOT, os.path.join(ROOT, "tests", "hipcpu"), module)] + args
    else:
        cmd = [sys.executable, "-m", "maskfusion_amd." + module] + args
    return subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_eval_command_scores_against_ply_and_obj(hip, tmp_path):
    from maskfusion_amd import mesh as M
    fx = _fixture("sphere")
    est = tmp_path / "est"
    est.mkdir()
    s = tr.sample(fx["V"], fx["F"], 1500.0)
    M.write_mesh_ply(str(est / "cloud-0.ply"), s["points"] + np.float32(0.001), s["normals"])
    M.write_mesh_ply(str(tmp_path / "m.ply"), fx["V"], triangles=fx["F"])
    M.write_obj(str(tmp_path / "m.obj"), fx["V"], fx["F"])
    lines = []
    for name in ("m.ply", "m.obj"):
        r = _command("eval", ["--est", str(est), "--ref-mesh", str(tmp_path / name), "--mesh-density", "3000", "--normals"])
        assert r.returncode == 0, r.stderr
        out = [json.loads(x) for x in r.stdout.splitlines() if x.startswith("{")]
        assert len(out) == 1 and out[0]["ref_mesh"].endswith(name)
        lines.append(out[0])
    c = lines[0]["cloud"]
    print(c)
    assert c["reference"]["triangles"] == 320 and c["reference"]["eligible"] == 320 and c["reference"]["density"] == 3000.0
    assert c["reference"]["samples"] == tr.sample(fx["V"], fx["F"], 3000.0)["n"]
    assert c["accuracy"]["misses"] == 0 and c["accuracy"]["mean"] <= 0.002 and "normal_consistency" in lines[0]
    for o in lines:
        del o["ref_mesh"]
    assert lines[0] == lines[1]
    for bad, word in ((["--ref-mesh", str(tmp_path / "m.ply"), "--ref-cloud", str(tmp_path / "m.ply")], "--ref-mesh"), (["--mesh-density", "100", "--gt", "x"], "need --ref-mesh"),
                      (["--ref-mesh", str(tmp_path / "m.ply"), "--mesh-cell", "0"], "positive")):
        r = _command("eval", ["--est", str(est)] + bad)
        assert r.returncode == 2 and word in r.stderr, r.stderr
    r = _command("eval", ["--est", str(est), "--ref-mesh", str(tmp_path / "missing.obj")])
    assert r.returncode == 2 and "--ref-mesh" in r.stderr


def test_mesh_command_reports_fidelity(hip, tmp_path):
    """the sphere cloud of tests/test_gpu_mesh.py's command test, meshed with --fidelity: every input point has the mesh within the support"""
    import mesh_restatement as mr
    from maskfusion_amd import mesh as M
    centre, R, voxel = np.array([0.1, -0.05, 1.5]), 0.4, 0.04
    p, n, col = mr.sphere_cloud(11, 4000, centre, R, sigma=0.001)
    n /= np.linalg.norm(n, axis=1)[:, None]
    M.write_mesh_ply(str(tmp_path / "cloud-0.ply"), p, n, col)
    r = _command("mesh", ["--cloud", str(tmp_path / "cloud-0.ply"), "--voxel", str(voxel), "-o", str(tmp_path / "mesh.ply"), "--fidelity"])
    assert r.returncode == 0, r.stderr
    info = json.loads(r.stdout)
    print(info["cloud_to_mesh"])
    assert info["cloud_to_mesh"]["count"] == len(p) and info["cloud_to_mesh"]["misses"] == 0 and info["cloud_to_mesh"]["mean"] <= voxel / 4
    r = _command("mesh", ["--cloud", str(tmp_path / "cloud-0.ply"), "--voxel", str(voxel), "-o", str(tmp_path / "mesh.ply")])
    assert r.returncode == 0 and "cloud_to_mesh" not in json.loads(r.stdout)
